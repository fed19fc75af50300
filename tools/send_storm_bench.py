"""Measure the storm send program (rlo_program_send_storm: open-loop bcasts of caller-owned device buffers on the
progress kernel) on one MI355X:

  python tools/send_storm_bench.py [--ranks 8 64 256] [--lens 64 1008] [--big-lens 4096 32768] [--big-ranks 8 64]
                                   [--seconds 0.5] [--out profiles/send_storm_bench.json]

Per world size and message length, in one run:
  storm_send : the storm send program, every rank originating k / n messages (message i from rank i mod n)
  hop_send   : the hop kernel's send program, open loop, the same origins and length (lengths <= 1008 B only)
  storm      : the storm program with kernel-generated payloads of the same length, k and order (RLO_ORDER_SLOTS)
Each leg warms up with one launch, then the legs take turns, one launch (a timed window: HIP events around the kernel)
each, until every leg has --seconds of kernel time.  Per leg: messages/s, deliveries/s, delivered payload GB/s, the HBM
bytes (each delivery's slot written and read once, 2 x (16 + round16(len)); the caller-buffer legs add the dst write
per delivery and the src read per message) over kernel time as a share of the peak, and the spread of messages/s over
the leg's windows.  `verdict`: storm_send's messages/s against hop_send's, and whether the difference exceeds the two
legs' combined window-to-window spread.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rootless-coll-mpi-ops_amd"))
PEAK_HBM = 8.0e12  # bytes/s, MI355X
ORDER_SLOTS = 1


def legs_of(rlo, torch, n, ln, seconds, max_windows, names=("storm_send", "hop_send", "storm")):
    slot = (ln + 15) // 16 * 16
    k = int(max(n, min(1 << 17, (2 << 30) // (n * slot)) // n * n))
    kh = int(max(n, min(k, 16384) // n * n))  # the hop leg: one message per rank-wave at a time, a shorter list
    rng = np.random.default_rng(n * 4096 + ln)
    legs, worlds = {}, []
    try:
        for name in names:
            if name == "hop_send" and ln > 1008:
                continue
            w = rlo.World(n, max_payload=slot)
            worlds.append(w)
            kk = kh if name == "hop_send" else k
            if name == "storm":
                w.program_storm(kk, ln, seed=21, order=ORDER_SLOTS)
            else:
                src = torch.from_numpy(rng.integers(0, 256, kk * slot, dtype=np.uint8)).cuda()
                dst = torch.zeros(n * kk * slot, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                origins = np.arange(kk) % n
                lens = np.full(kk, ln, dtype=np.uint32)
                if name == "storm_send":
                    w.program_send_storm(origins, src, dst, slot, lens=lens)
                else:
                    w.program_send(origins, src, dst, slot, lens=lens)
            w.run()  # warm-up
            assert (w.info_now()["last_kernel"] == 1) == (name == "hop_send"), (name, n, ln)
            st = w.stats()
            assert (st["error"] == 0).all() and int(st["originated"].sum()) == kk, (name, n, ln)
            legs[name] = {"w": w, "k": kk, "ms": []}
        while any(sum(g["ms"]) < seconds * 1e3 and len(g["ms"]) < max_windows for g in legs.values()):
            for g in legs.values():  # the legs take turns
                if sum(g["ms"]) < seconds * 1e3 and len(g["ms"]) < max_windows:
                    g["ms"].append(g["w"].run())
        out = {}
        for name, g in legs.items():
            ms = np.asarray(g["ms"], dtype=np.float64)
            t = float(ms.sum()) * 1e-3
            msgs = g["k"] * len(ms)
            deliveries = msgs * (n - 1)
            hbm = deliveries * 2 * (16 + slot)
            if name != "storm":
                hbm += deliveries * slot + msgs * slot
            rate = g["k"] / (ms * 1e-3)  # messages/s of each window
            out[name] = {"k": g["k"], "windows": len(ms), "kernel_s": round(t, 4), "msgs_per_s": round(msgs / t),
                         "deliveries_per_s": round(deliveries / t), "payload_GBps": round(deliveries * ln / t / 1e9, 3),
                         "hbm_GBps": round(hbm / t / 1e9, 3), "hbm_share_of_peak": round(hbm / t / PEAK_HBM, 5),
                         "window_msgs_per_s": {"min": round(float(rate.min())), "median": round(float(np.median(rate))),
                                               "max": round(float(rate.max()))},
                         "waves": g["w"].info["waves"]}
        ss = out.get("storm_send")
        if ss and "storm" in out:
            out["ratio_to_storm"] = round(ss["msgs_per_s"] / out["storm"]["msgs_per_s"], 4)
        if ss and "hop_send" in out:
            hp = out["hop_send"]
            spread = sum(x["window_msgs_per_s"]["max"] - x["window_msgs_per_s"]["min"] for x in (ss, hp))
            diff = ss["window_msgs_per_s"]["median"] - hp["window_msgs_per_s"]["median"]
            out["verdict"] = {"ratio_to_hop_send": round(ss["msgs_per_s"] / hp["msgs_per_s"], 3), "median_difference": diff,
                              "combined_spread": spread, "storm_send_wins": bool(diff > spread)}
        return out
    finally:
        for w in worlds:
            w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--lens", type=int, nargs="+", default=[64, 1008])
    ap.add_argument("--big-ranks", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--big-lens", type=int, nargs="*", default=[4096, 32768])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-windows", type=int, default=400)
    ap.add_argument("--legs", nargs="+", default=["storm_send", "hop_send", "storm"],
                    help="the legs to run (an A/B of two builds, RLO_LIB_DIR=lib_<name>: storm_send alone)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import rlo

    res = {"bench": "send_storm", "lib": os.path.basename(os.path.dirname(rlo.LIB_PATH)), "device": torch.cuda.get_device_name(0), "peak_hbm_Bps": PEAK_HBM, "legs": []}
    shapes = [(n, ln) for n in a.ranks for ln in a.lens] + [(n, ln) for n in a.big_ranks for ln in a.big_lens]
    for n, ln in shapes:
        leg = {"n": n, "len": ln}
        leg.update(legs_of(rlo, torch, n, ln, a.seconds, a.max_windows, tuple(a.legs)))
        res["legs"].append(leg)
        print("# n %d len %d: %s" % (n, ln, json.dumps({k: v for k, v in leg.items() if k not in ("n", "len")})),
              file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

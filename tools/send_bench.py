"""Measure the send program (rlo_program_send: bcasts of caller-owned device buffers) on one MI355X:

  python tools/send_bench.py [--ranks 8 64 256] [--lens 64 1008] [--seconds 0.5] [--out FILE]

Per world size and message length, in one run:
  open    : open-loop send, every rank originating k / n messages -- messages/s, delivered payload GB/s, and the
            HBM bytes (each delivery's slot written and read once, 2 x (16 + round16(len)), plus its dst write) over
            kernel time as a share of the peak
  ordered : ordered send (one message in flight) -- p50 / p99 of the per-message completion time
  latency : the latency program (kernel-generated payloads) on the same world shape, for comparison
  host    : the same user bytes through the host-service program (rlo.HostWorld.bcast: read back from device memory,
            posted, every rank's pickup polled from Python), the only way to move them before this program -- host
            clock, closed loop, Python's polling included
Each device leg warms up with one launch, then the three legs take turns, one launch (a timed window: HIP events
around the kernel) each, until every leg has --seconds of kernel time.  One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rootless-coll-mpi-ops_amd"))
PEAK_HBM = 8.0e12  # bytes/s, MI355X


def pct(x, p):
    return round(float(np.percentile(np.asarray(x, dtype=np.float64), p)), 3)


def device_legs(rlo, torch, n, ln, seconds, max_windows):
    slot = (ln + 15) // 16 * 16
    k = int(max(n, min(16384, (256 << 20) // (n * slot)) // n * n))
    ko = 2000
    rng = np.random.default_rng(n * 4096 + ln)
    legs = {}
    worlds = []
    try:
        for name in ("open", "ordered", "latency"):
            w = rlo.World(n, max_payload=slot)
            worlds.append(w)
            kk = k if name == "open" else ko
            if name == "latency":
                w.program_latency(ko, ln, seed=21)
            else:
                src = torch.from_numpy(rng.integers(0, 256, kk * slot, dtype=np.uint8)).cuda()
                dst = torch.zeros(n * kk * slot, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                origins = (np.arange(kk) % n) if name == "open" else rng.integers(0, n, kk)
                w.program_send(origins, src, dst, slot, lens=np.full(kk, ln, dtype=np.uint32), ordered=name == "ordered")
            w.run()  # warm-up
            hop = w.info_now()["last_kernel"] == 1
            assert hop or name == "latency", (name, n, ln)
            legs[name] = {"w": w, "k": kk, "ms": [], "lat": [], "kernel": "hop" if hop else "progress"}
        while any(sum(g["ms"]) < seconds * 1e3 and len(g["ms"]) < max_windows for g in legs.values()):
            for name, g in legs.items():  # the legs take turns
                if sum(g["ms"]) >= seconds * 1e3 or len(g["ms"]) >= max_windows:
                    continue
                g["ms"].append(g["w"].run())
                if name != "open":
                    g["lat"].append(g["w"].latencies_ticks().astype(np.float64) * 0.01)
        out = {}
        g = legs["open"]
        t = sum(g["ms"]) * 1e-3
        msgs = g["k"] * len(g["ms"])
        deliveries = msgs * (n - 1)
        hbm = deliveries * (2 * (16 + slot) + slot)
        out["open"] = {"k": g["k"], "windows": len(g["ms"]), "kernel_s": round(t, 4), "msgs_per_s": round(msgs / t),
                       "deliveries_per_s": round(deliveries / t), "payload_GBps": round(deliveries * ln / t / 1e9, 3),
                       "hbm_GBps": round(hbm / t / 1e9, 3), "hbm_share_of_peak": round(hbm / t / PEAK_HBM, 5)}
        for name in ("ordered", "latency"):
            g = legs[name]
            lat = np.concatenate(g["lat"])
            out[name] = {"k": g["k"], "windows": len(g["ms"]), "kernel_s": round(sum(g["ms"]) * 1e-3, 4),
                         "p50_us": pct(lat, 50), "p99_us": pct(lat, 99), "kernel": g["kernel"]}
        return out
    finally:
        for w in worlds:
            w.close()


def host_leg(rlo, torch, n, ln, rounds):
    """closed loop on the host clock: the message's bytes read back from device memory, posted, and every other
    rank's pickup polled"""
    src = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (rounds, ln), dtype=np.uint8)).cuda()
    us = []
    with rlo.HostWorld(n, max_payload=max(ln, 64), idle_timeout_s=15) as hw:
        for i in range(rounds + 4):
            o = i % n
            t0 = time.perf_counter()
            hw.bcast(o, src[i % rounds].cpu().numpy().tobytes(), seq=i)
            got = 0
            while got < n - 1:
                for r in range(n):
                    got += len(hw.poll(r))
                if time.perf_counter() - t0 > 20:
                    raise RuntimeError("host leg stalled")
            if i >= 4:  # (warm-up rounds)
                us.append((time.perf_counter() - t0) * 1e6)
    return {"rounds": rounds, "p50_us": pct(us, 50), "p99_us": pct(us, 99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--lens", type=int, nargs="+", default=[64, 1008])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-windows", type=int, default=400)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import rlo

    res = {"bench": "send", "device": torch.cuda.get_device_name(0), "peak_hbm_Bps": PEAK_HBM, "legs": []}
    for n in a.ranks:
        for ln in a.lens:
            leg = {"n": n, "len": ln}
            leg.update(device_legs(rlo, torch, n, ln, a.seconds, a.max_windows))
            if not a.no_host:
                try:
                    leg["host"] = host_leg(rlo, torch, n, ln, {8: 300, 64: 60}.get(n, 20))
                except Exception as e:  # noqa: BLE001 - the comparison leg must not lose the device legs' figures
                    leg["host"] = {"error": repr(e)[:200]}
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

"""A/B of the decide program against the iar program on one MI355X, same proposals, one session:

  python tools/decide_ab.py [--ranks 8] [--per 2000] [--len 16] [--ppm 10000] [--runs 7] [--out profiles/decide_ab.txt]

  iar    : rlo_program_iar, RLO_JUDGE_HASH(seed, ppm), the proposal data uploaded from the host
  decide : rlo_program_decide, the same proposals (pid = index) read from a device buffer, judged by a verdict table
           that holds the same hash's verdicts, the received data and the decisions written to device buffers

Both run the hop kernel (checked).  The two take turns, one launch each (HIP events around the kernel), `runs` launches
each after one warm-up, and must decide alike (own_approved, judge_calls compared).  What decide adds per judged proposal:
one dependent byte load (the verdict), the data chunks' stores to dst, and per delivered decision one byte store.
Printed and written: decisions/s of every run, each leg's median, the iar leg's own run-to-run spread (max - min over
its median), and the decide median relative to the iar median.

--anatomy (with RLO_DIAG_LIB=1, the diagnostics build): also each leg's section profile of its last launch (rlo_hop.hip
kHopProf, as tools/hop_anatomy.py reads it): shader clocks per section of a round and per part of a take, per decision
of one rank.  That build's rates are its own, not the product's."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rootless-coll-mpi-ops_amd"))
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def judge_hash(seed, rank, pid):
    """rlo_kernel_common.hpp judge_hash: splitmix64(seed ^ rank << 32 ^ pid) % 1e6, vectorised over rank / pid"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) ^ (rank.astype(np.uint64) << np.uint64(32)) ^ pid.astype(np.uint64)
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(1000000)).astype(np.uint32)


SECTIONS = ["poll", "bells", "publish", "loads", "votes", "slots", "own", "books"]  # (tools/hop_anatomy.py)


def section_profile(tag, st, units):
    prof = st["prof"].astype(np.float64)
    tk = st["hist"][:, -4:].astype(np.float64)  # a take's clocks: checks, forward, effects; takes
    ntk = np.maximum(tk[:, 3], 1)
    pre = st["hist"][:, -5].astype(np.float64)  # of the checks: entry -> the child set's computation
    return ["  %-6s sections: %s" % (tag, " ".join("%s %.0f" % (s, v) for s, v in zip(SECTIONS, np.median(prof, axis=0) / units))),
            "  %-6s per take: checks %.0f (header / pending / judge %.0f) forward %.0f effects %.0f; %.1f takes" % (
                tag, np.median(tk[:, 0] / ntk), np.median(pre / ntk), np.median(tk[:, 1] / ntk), np.median(tk[:, 2] / ntk),
                np.median(tk[:, 3]) / units)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--per", type=int, default=2000, help="proposals per rank")
    ap.add_argument("--len", type=int, default=16, help="data bytes per proposal")
    ap.add_argument("--ppm", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=99)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--anatomy", action="store_true", help="the diagnostics build's section profile of each leg")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.anatomy and os.environ.get("RLO_DIAG_LIB") != "1":
        ap.error("--anatomy reads the diagnostics build's profile: run with RLO_DIAG_LIB=1")
    import torch

    import rlo
    from rlo import _lib as L

    n, k = a.ranks, a.ranks * a.per
    slot = max(16, (a.len + 15) // 16 * 16)
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, (k, slot), dtype=np.uint8)
    origins = np.arange(k) % n  # proposal i: rank i % n's, pid i (it-major, as the benchmark's)
    props = [(int(origins[i]), i, data[i, :a.len].tobytes()) for i in range(k)]
    h = judge_hash(a.seed, np.arange(n)[:, None].repeat(k, 1), np.arange(k)[None, :].repeat(n, 0))
    verdict = np.where(h < a.ppm, 0, 1 + h % 255).astype(np.uint8)

    src = torch.from_numpy(data.reshape(-1)).cuda()
    ver = torch.from_numpy(verdict.reshape(-1)).cuda()
    dst = torch.zeros(n * k * slot, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n * k, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    legs = {}
    with rlo.World(n, max_payload=16 + slot) as wi, rlo.World(n, max_payload=16 + slot) as wd:
        wi.program_iar(props, judge=L.RLO_JUDGE_HASH, seed=a.seed, ppm=a.ppm)
        wd.program_decide(origins, src, dst, dec, slot, lens=np.full(k, a.len, dtype=np.uint32), verdict=ver)
        for name, w in (("iar", wi), ("decide", wd)):
            w.run()  # warm-up
            assert w.info_now()["last_kernel"] == 1, name
            st = w.stats()
            assert (st["error"] == 0).all() and int(st["own_decided"].sum()) == k, name
            legs[name] = {"w": w, "ms": [], "approved": int(st["own_approved"].sum()), "judged": int(st["judge_calls"].sum())}
        assert legs["iar"]["approved"] == legs["decide"]["approved"] and legs["iar"]["judged"] == legs["decide"]["judged"]
        torch.cuda.synchronize()
        assert int(dec.view(n, k)[0].sum()) == legs["decide"]["approved"] and bool((dec.view(n, k) == dec.view(n, k)[0]).all())
        for _ in range(a.runs):
            for g in legs.values():  # the legs take turns
                g["ms"].append(g["w"].run())
        anatomy = [section_profile(name, g["w"].stats(), a.per) for name, g in legs.items()] if a.anatomy else []
    rate = {name: np.array([k / (ms * 1e-3) for ms in g["ms"]]) for name, g in legs.items()}
    med = {name: float(np.median(r)) for name, r in rate.items()}
    spread = float(rate["iar"].max() - rate["iar"].min()) / med["iar"]
    lines = ["decide vs iar, %s, %d ranks, %d proposals per rank of %d data bytes, hash judge %d ppm: %d of %d approved, %d judge calls"
             % (torch.cuda.get_device_name(0), n, a.per, a.len, a.ppm, legs["iar"]["approved"], k, legs["iar"]["judged"]),
             "interleaved, %d launches each after one warm-up, hop kernel both; decisions/s per launch:" % a.runs]
    for name in ("iar", "decide"):
        lines.append("  %-6s %s  median %.0f" % (name, " ".join("%.0f" % x for x in rate[name]), med[name]))
    lines.append("iar run-to-run spread (max - min) / median: %.2f %%" % (100 * spread))
    lines.append("decide median / iar median: %.4f (%+.2f %%)" % (med["decide"] / med["iar"], 100 * (med["decide"] / med["iar"] - 1)))
    if anatomy:
        lines.append("the diagnostics build's section profile (shader clocks, median over ranks, per decision of one rank):")
        lines += [ln for leg in anatomy for ln in leg]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()

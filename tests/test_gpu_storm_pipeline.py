"""GPU tests of the 8-wave storm kernel's pipelined iteration: wave 0 consumes iteration i, polls and selects iteration
i + 1 while waves 1-7 copy iteration i's messages into the out-rings, one barrier behind both, the out-ring tails
published behind it.  Every case is an 8-wave world against the oracle (the method of test_gpu_storm_overlap.py):
per-rank delivery rows (bid, origin, parent), every delivered byte, counts and checksums."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as orc

pytestmark = pytest.mark.gpu
LOG_DELIVER = 1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rootless-coll-mpi-ops_amd")


@pytest.fixture(scope="module")
def rlo():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rlo as _rlo

    return _rlo


def _check(st, n, k, ln, seed, logs=None):
    """logs: {rank: (rows, payload)} of a logged storm, or None (counts and checksums only)"""
    ref = orc.storm(n, seed, k, ln, want_parent=logs is not None)
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    assert np.array_equal(st["bcast_delivered"].astype(np.int64), ref["count"])
    assert np.array_equal(st["bcast_sum"], ref["sum"])
    if logs is None:
        return
    org = [orc.origin_of(seed, b, n) for b in range(k)]
    pay = [orc.payload(org[b], b, ln) for b in range(k)]
    for r in range(n):
        rows, payload = logs[r]
        got = sorted((row[4], row[2], row[3]) for row in rows if row[0] == LOG_DELIVER)
        want = sorted((b, org[b], int(ref["parent"][b, r])) for b in range(k) if org[b] != r)
        assert got == want, r
        for row in rows:  # (origin and bid are the oracle's by the rows above)
            assert row[5] == ln
            assert bytes(payload[row[8]][:ln]) == pay[row[4]], (r, row[2], row[4])


def _storm(w, n, k, ln, seed, window=64, log=True, **kw):
    w.program_storm(k, ln, seed=seed, window=window, log=log, log_cap=k + 8 if log else 0, **kw)
    w.run()
    st = w.stats()
    logs = {r: w.log(r, cap=k + 8, payload=True) for r in range(n)} if log else None
    return st, logs


# 16-slot rings: the wall ranks refuse, admit prefixes shorter than their take and shrink their windows, and all of
# that is consume's result, which the select beside the copy starts from.  256 ranks: the flagship's world; window 1:
# a rank's own bcasts one at a time; 112 B: a full 8-chunk slot; 8 and 4 ranks: the lone-message path at the storm's
# tail, often
@pytest.mark.parametrize("n,k,ln,window", [(256, 4096, 64, 64), (256, 2048, 64, 1), (8, 2000, 112, 64), (4, 500, 1, 64)])
def test_ring_pressure(rlo, n, k, ln, window):
    seed = 41
    with rlo.World(n, max_payload=ln if ln > 64 else 64, ring_slots=16) as w:
        assert w.info["waves"] == 8
        st, logs = _storm(w, n, k, ln, seed, window=window)
    _check(st, n, k, ln, seed, logs)


def test_launch_to_launch_state(rlo):
    """launches of one world end on different iteration counts (k = 1 and k = 5: most ranks only ever forward or idle):
    nothing that indexes the kernel's buffers may survive a launch.  Each launch against its own oracle run"""
    n, ln, sa, sb = 64, 64, 5, 77
    with rlo.World(n, max_payload=64, ring_slots=16) as w:
        assert w.info["waves"] == 8
        for k, seed in ((1, 11), (4096, sa), (5, 13), (4096, sb)):
            st, logs = _storm(w, n, k, ln, seed)
            _check(st, n, k, ln, seed, logs)
        rounds, lseed = 48, 9
        w.program_latency(rounds, ln, seed=lseed)
        w.run()
        st = w.stats()
        assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
        org = [orc.origin_of(lseed, i, n) for i in range(rounds)]
        assert [int(x) for x in st["bcast_delivered"]] == [sum(o != r for o in org) for r in range(n)]
        assert np.array_equal(st["bcast_sum"], orc.storm(n, lseed, rounds, ln)["sum"])
        st, logs = _storm(w, n, 4096, ln, sa)
        _check(st, n, 4096, ln, sa, logs)


# a storm on the diagnostics build in a process of its own (the library is chosen at import): one JSON line.  A logged
# storm's rows per rank, sorted; with prof, no log: rank 0's phase cycles and diagnostics words
CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import rlo
n, k, ln, seed, slots, prof = (int(x) for x in sys.argv[2:8])
with rlo.World(n, max_payload=64, ring_slots=slots) as w:
    waves = w.info["waves"]
    w.program_storm(k, ln, seed=seed, window=64, log=not prof, log_cap=0 if prof else k + 8, prof=bool(prof))
    w.run()
    st = w.stats()
    logs = []
    for r in range(n if not prof else 0):
        rows, pay = w.log(r, cap=k + 8, payload=True)
        # (aux is a clock, payload_idx the record's place: the row's content is the rest and its bytes)
        logs.append(sorted([list(row[:7]) + [bytes(pay[row[8]][:ln]).hex()] for row in rows]))
    print(json.dumps({"waves": waves, "error": st["error"].tolist(), "sum": st["bcast_sum"].tolist(),
                      "count": st["bcast_delivered"].tolist(), "logs": logs,
                      "prof0": st["prof"][0].tolist(), "dbg0": st["dbg"][0].tolist()}))
'''


def _child(n, k, ln, seed, slots, prof=False, **sw):
    assert os.path.exists(os.path.join(PKG, "lib_diag", "librlo_hip.so")), "diagnostics build (make DIAG=1) not built"
    env = dict({k_: v for k_, v in os.environ.items() if k_ != "RLO_NO_PIPELINE"}, RLO_DIAG_LIB="1", **sw)
    r = subprocess.run([sys.executable, "-c", CHILD, PKG] + [str(x) for x in (n, k, ln, seed, slots, int(prof))],
                       capture_output=True, text=True, timeout=150, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["waves"] == 8 and not any(d["error"]), d["error"]
    return d


@pytest.mark.parametrize("n", [64, 256])
def test_old_order_equals_new_order(n):
    """the diagnostics build's RLO_NO_PIPELINE runs the iteration in its old order (every wave copies, then wave 0
    alone consumes, polls and selects) in the same binary: the same logged storm gives the same rows, rank by rank,
    and both equal the oracle's"""
    k, ln, seed, slots = 4096, 64, 29, 16
    new = _child(n, k, ln, seed, slots)
    old = _child(n, k, ln, seed, slots, RLO_NO_PIPELINE="1")
    assert new["logs"] == old["logs"]
    assert new["sum"] == old["sum"] and new["count"] == old["count"]
    ref = orc.storm(n, seed, k, ln, want_parent=True)
    assert np.array_equal(np.array(new["count"], dtype=np.int64), ref["count"])
    assert np.array_equal(np.array(new["sum"], dtype=np.uint64), ref["sum"])
    org = [orc.origin_of(seed, b, n) for b in range(k)]
    pay = [orc.payload(org[b], b, ln) for b in range(k)]
    for r in range(n):
        got = sorted((row[4], row[2], row[3]) for row in new["logs"][r] if row[0] == LOG_DELIVER)
        assert got == sorted((b, org[b], int(ref["parent"][b, r])) for b in range(k) if org[b] != r), r
        for row in new["logs"][r]:
            assert bytes.fromhex(row[7]) == pay[row[4]], (r, row[2], row[4])


def test_prof_storm():
    """MODE_PROF: the lone-message path is off, every iteration takes the full path.  Counts and checksums are the
    oracle's, and rank 0 reports a copying wave's copy cycles (dbg[3]) and wave 0's wait at the barrier behind the
    copy (dbg[4])"""
    n, k, ln, seed = 64, 4096, 64, 33
    d = _child(n, k, ln, seed, 0, prof=True)
    ref = orc.storm(n, seed, k, ln)
    assert np.array_equal(np.array(d["count"], dtype=np.int64), ref["count"])
    assert np.array_equal(np.array(d["sum"], dtype=np.uint64), ref["sum"])
    assert d["dbg0"][3] != 0 and d["dbg0"][4] != 0, d["dbg0"]


def test_two_unequal_parts_on_one_gpu(rlo):
    """a world of 24 + 40 ranks, each part a kernel of its own storing into the other's 16-slot rings: the tails behind
    the barrier are published system-scope"""
    from rlo import sharded

    n, k, ln, seed = 64, 4096, 64, 23
    spec = {"kind": "storm", "k": k, "len": ln, "seed": seed, "log": True, "log_cap": k + 8}
    (st, logs, _), rcs = sharded.run_inprocess(n, [0, 24, 64], spec, max_payload=64, ring_slots=16)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    _check(st, n, k, ln, seed, logs)

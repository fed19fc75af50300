"""GPU tests of the 8-wave storm kernel (the flagship's instantiation): its forwarding tables, filled per launch where
the large-message stage used to be, and the launches around them.  Small worlds and small rings, every one against
the oracle: per-rank deliveries (bid, origin, parent), every delivered byte, counts and checksums.  The workload's own
size stays with bench.py and test_gpu_engine.py::test_storm_full_size_checksums."""
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
    for r in range(n):
        rows, payload = logs[r]
        got = sorted((row[4], row[2], row[3]) for row in rows if row[0] == LOG_DELIVER)
        want = sorted((b, org[b], int(ref["parent"][b, r])) for b in range(k) if org[b] != r)
        assert got == want, r
        for row in rows:
            assert row[5] == ln
            assert bytes(payload[row[8]][:ln]) == orc.payload(row[2], row[4], ln), (r, row[2], row[4])


def _storm(w, n, k, ln, seed, window=64, log=True, **kw):
    w.program_storm(k, ln, seed=seed, window=window, log=log, log_cap=k + 8 if log else 0, **kw)
    w.run()
    st = w.stats()
    logs = {r: w.log(r, cap=k + 8, payload=True) for r in range(n)} if log else None
    return st, logs


# 16- and 32-slot rings: refusals, FIFO prefixes and the credit selection stay busy; 255 / 256 ranks: the tables at
# the flagship's size (every CU a rank), 3 / 5 / 13 / 100: worlds that are no power of two (ranks without a wall)
@pytest.mark.parametrize("n,k,ln,slots", [(3, 300, 1, 16), (5, 500, 64, 16), (13, 2000, 112, 16), (64, 4096, 64, 16),
                                          (100, 3000, 48, 32), (255, 2048, 64, 0), (256, 4096, 64, 64)])
def test_logged_storms(rlo, n, k, ln, slots):
    seed = 29
    with rlo.World(n, max_payload=ln if ln > 64 else 64, ring_slots=slots) as w:
        assert w.info["waves"] == 8
        st, logs = _storm(w, n, k, ln, seed)
    _check(st, n, k, ln, seed, logs)


@pytest.mark.parametrize("n,k", [(8, 1), (64, 5)])
def test_fewer_bcasts_than_a_window(rlo, n, k):
    """the first iterations, the idle spin and the exit: most ranks originate nothing"""
    ln, seed = 64, 17
    with rlo.World(n, max_payload=64) as w:
        assert w.info["waves"] == 8
        st, logs = _storm(w, n, k, ln, seed)
    _check(st, n, k, ln, seed, logs)


def test_one_world_five_launches(rlo):
    """nothing of a launch's tables or selection survives it: storms of two shapes, a latency program and an iar
    program between them, then the first storm again, each against its own oracle run"""
    n, ln = 64, 64
    with rlo.World(n, max_payload=64, ring_slots=16) as w:
        assert w.info["waves"] == 8
        st, logs = _storm(w, n, 4096, ln, 5, window=64)
        _check(st, n, 4096, ln, 5, logs)
        st, logs = _storm(w, n, 1500, ln, 77, window=1)
        _check(st, n, 1500, ln, 77, logs)
        rounds, lseed = 48, 9
        w.program_latency(rounds, ln, seed=lseed)
        w.run()
        st = w.stats()
        assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
        org = [orc.origin_of(lseed, i, n) for i in range(rounds)]
        assert [int(x) for x in st["bcast_delivered"]] == [sum(o != r for o in org) for r in range(n)]
        assert np.array_equal(st["bcast_sum"], orc.storm(n, lseed, rounds, ln)["sum"])
        w.program_iar([(r, r, b"0123456789abcdef") for r in range(n)])
        w.run()
        st = w.stats()
        assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
        assert int(st["own_approved"].sum()) == n and (st["dec_delivered"] == n - 1).all()
        st, logs = _storm(w, n, 4096, ln, 5, window=64)
        _check(st, n, 4096, ln, 5, logs)


def test_hist_storm(rlo):
    n, k, ln, seed = 64, 4096, 64, 3
    with rlo.World(n, max_payload=64) as w:
        assert w.info["waves"] == 8
        st, _ = _storm(w, n, k, ln, seed, log=False, hist=True)
    assert int(st["hist"].sum()) == k * (n - 1)
    _check(st, n, k, ln, seed)


# a logged storm's rows per rank in the order the rank logged them, one JSON line
LOG_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import rlo
n, k, ln, seed, slots = (int(x) for x in sys.argv[2:7])
with rlo.World(n, max_payload=64, ring_slots=slots) as w:
    waves = w.info["waves"]
    w.program_storm(k, ln, seed=seed, window=64, log=True, log_cap=k + 8)
    w.run()
    st = w.stats()
    logs = []
    for r in range(n):
        rows, pay = w.log(r, cap=k + 8, payload=True)
        # (aux is a clock, payload_idx the record's place: the row's content is the rest and its bytes)
        logs.append(sorted([list(row[:7]) + [bytes(pay[row[8]][:ln]).hex()] for row in rows]))
    print(json.dumps({"waves": waves, "error": st["error"].tolist(), "sum": st["bcast_sum"].tolist(),
                      "count": st["bcast_delivered"].tolist(), "logs": logs}))
'''


def test_computed_path_equals_the_tables():
    """the diagnostics build's RLO_NO_NEED_TABLE makes the kernel compute every ring message's out-rings, as before
    the tables: the same logged storm gives the same rows, rank by rank, and both equal the oracle's"""
    assert os.path.exists(os.path.join(PKG, "lib_diag", "librlo_hip.so")), "diagnostics build (make DIAG=1) not built"
    n, k, ln, seed, slots = 64, 4096, 64, 29, 16
    out = []
    for sw in ({}, {"RLO_NO_NEED_TABLE": "1"}):
        env = dict({k_: v for k_, v in os.environ.items() if k_ != "RLO_NO_NEED_TABLE"}, RLO_DIAG_LIB="1", **sw)
        r = subprocess.run([sys.executable, "-c", LOG_CHILD, PKG, str(n), str(k), str(ln), str(seed), str(slots)],
                           capture_output=True, text=True, timeout=150, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["waves"] == 8 and not any(d["error"]), d["error"]
        out.append(d)
    tab, comp = out
    assert tab["logs"] == comp["logs"]
    assert tab["sum"] == comp["sum"] and tab["count"] == comp["count"]
    ref = orc.storm(n, seed, k, ln, want_parent=True)
    assert np.array_equal(np.array(tab["count"], dtype=np.int64), ref["count"])
    assert np.array_equal(np.array(tab["sum"], dtype=np.uint64), ref["sum"])
    org = [orc.origin_of(seed, b, n) for b in range(k)]
    for r in range(n):
        got = sorted((row[4], row[2], row[3]) for row in tab["logs"][r] if row[0] == LOG_DELIVER)
        assert got == sorted((b, org[b], int(ref["parent"][b, r])) for b in range(k) if org[b] != r), r
        for row in tab["logs"][r]:
            assert bytes.fromhex(row[7]) == orc.payload(row[2], row[4], ln), (r, row[2], row[4])


def test_two_parts_on_one_gpu(rlo):
    """a world of 2 x 32 ranks, each part a kernel of its own storing into the other's rings (16 slots)"""
    from rlo import sharded

    n, k, ln, seed = 64, 4096, 64, 21
    spec = {"kind": "storm", "k": k, "len": ln, "seed": seed, "log": True, "log_cap": k + 8}
    (st, logs, _), rcs = sharded.run_inprocess(n, [0, 32, 64], spec, max_payload=64, ring_slots=16)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    _check(st, n, k, ln, seed, logs)

"""GPU parity of plain bcasts at every boundary length, on the three carriers the send programs' tests do not cover.

The rest of the suite runs the latency program at 1 .. 112 bytes, the generated storm at fifteen lengths up to 4096 and
the host service at four.  Here every carrier runs the lengths on both sides of each chunk count at which the engine
takes another path (tests/bcast_length_cases.py: 0 bytes up to the largest slot, 65520), in the worlds that put each
length on each path: the hop kernel up to 64 chunks, the 4-wave progress kernel's large-message rounds pulled and
pushed beyond, worlds without doorbells, a bulk world's ring lengths, the 8-wave kernel under the latency program, the
storm's small, medium and large paths and two parts of one process at system scope.  Every launch has one length and is
compared with the oracle bit for bit: per-rank delivery counts and checksums, the kernel that ran and the world's
layout, and from a logged launch every rank's delivery set with tree parents, every record's length and every
delivered byte with its zero padding up to the chunk's end.  After its last length every world runs its first length
again: a length's state (relay slots, staged chunks, the hop kernel's chunk count) must not outlive its launch.
tests/test_bcast_lengths_oracle.py checks the cases' inputs and the comparisons themselves on the CPU.
"""
import re
import time

import numpy as np
import pytest

import bcast_length_cases as bc
import pyoracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rlo():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rlo as _rlo

    return _rlo


_EXPECTED = {}


def expected(c, ln):
    """the oracle's launch of (case, length): computed once, shared by every launch that compares with it"""
    key = (c.n, c.seed, c.k, ln, ln > c.max_payload)
    if key not in _EXPECTED:
        _EXPECTED[key] = bc.Expected(c.n, c.seed, c.k, ln, bulk=ln > c.max_payload)
    return _EXPECTED[key]


def _occupancy(e):
    return "[-3]" in str(e)  # RLO_E_OCCUPANCY


def _world(rlo, c):
    try:
        return bc.create(rlo, lambda: rlo.World(c.n, **c.world), c.pull_env)
    except rlo.RloError as e:
        if c.may_skip and _occupancy(e):
            pytest.skip("%d rank-workgroups are not co-resident on this device: the world was refused" % c.n)
        raise


def _run(rlo, w, c):
    try:
        return w.run()
    except rlo.RloError as e:
        if c.may_skip and _occupancy(e):
            pytest.skip("%d rank-workgroups are not co-resident on this device: the launch was refused" % c.n)
        raise


def _check_layout(c, info):
    got = {k: info[k] for k in ("waves", "nsmall", "pull", "ll_ok")}
    assert got == {"waves": c.waves, "nsmall": c.nsmall, "pull": c.pull, "ll_ok": c.ll_ok}, (c.id, got)
    # (the device's own occupancy answer may exceed the plan's model of it; two per CU is what 300 ranks need)
    assert info["blocks_per_cu"] >= c.per_cu and (c.per_cu == 1 or info["blocks_per_cu"] == 2), (c.id, info["blocks_per_cu"])
    assert info["pend_hbm"] == (1 if c.world.get("pend_hbm") else 0) and info["bulk_max"] == c.bulk_max, (c.id, info)


def _report(c, ln, info, ms, what):
    print("bcast length case %s len %d %s: last_kernel %d waves %d nsmall %d pull %d ll_ok %d per_cu %d kernel %.3f ms" %
          (c.id, ln, what, info["last_kernel"], info["waves"], info["nsmall"], info["pull"], info["ll_ok"],
           info["blocks_per_cu"], ms))


def _check_logs(c, exp, w):
    for r in range(c.n):
        recs, payload = bc.log_arrays(w, r, c.k + 8)
        bc.check_log(c.id, exp, r, recs, payload)


def _lat_launch(rlo, w, c, ln, log):
    exp = expected(c, ln)
    w.program_latency(c.k, ln, seed=c.seed, log=log, prof=c.prof)
    ms = _run(rlo, w, c)
    info = dict(w.info_now())
    st = w.stats()
    _report(c, ln, info, ms, "logged" if log else "plain")
    assert info["last_kernel"] == c.kernel, (c.id, ln, info["last_kernel"])
    _check_layout(c, info)
    bc.check_stats(c.id, exp, st)
    lat = w.latencies_ticks()
    assert len(lat) == c.k and (lat > 0).all(), (c.id, ln, lat)
    bc.check_round_ticks(c.id, ln, w.round_ticks(), c.k)
    if log:
        _check_logs(c, exp, w)
    return st["bcast_sum"].copy()


@pytest.mark.parametrize("cid", bc.ids("lat"))
def test_latency_program_lengths(rlo, cid):
    """one world per case, one length per launch: `launches` plain launches (kernel, layout, counts, checksums,
    latencies, round ticks) and a logged one (delivery sets, lengths, bytes and padding), then the first length again"""
    c = bc.BY_ID[cid]
    with _world(rlo, c) as w:
        _check_layout(c, w.info)
        first = None
        for ln in c.lens + c.lens[:1]:
            for _ in range(c.launches):
                s = _lat_launch(rlo, w, c, ln, False)
            assert np.array_equal(_lat_launch(rlo, w, c, ln, True), s), (cid, ln)
            first = s if first is None else first
        assert np.array_equal(s, first), cid  # the relaunch of the first length: the same result


@pytest.mark.parametrize("cid", bc.ids("storm"))
def test_storm_lengths(rlo, cid):
    """one world per case, one length per logged launch (and per window), then the first length again"""
    c = bc.BY_ID[cid]
    with _world(rlo, c) as w:
        _check_layout(c, w.info)
        for window in c.windows:
            first = None
            for ln in c.lens + c.lens[:1]:
                exp = expected(c, ln)
                w.program_storm(c.k, ln, seed=c.seed, window=window, log=True, log_cap=c.k + 8)
                ms = _run(rlo, w, c)
                info = dict(w.info_now())
                st = w.stats()
                _report(c, ln, info, ms, "window %d" % window)
                assert info["last_kernel"] == c.kernel, (cid, ln, info["last_kernel"])
                _check_layout(c, info)
                bc.check_stats(cid, exp, st)
                assert int(st["originated"].sum()) == c.k, (cid, ln)
                _check_logs(c, exp, w)
                first = st["bcast_sum"].copy() if first is None else first
            assert np.array_equal(st["bcast_sum"], first), cid


def _forge_bus(blob):
    m = re.search(rb"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-9]", blob)
    assert m, "no PCI bus id in the exported blob"
    return blob[:m.start()] + b"ffff:ff:1f.7" + blob[m.end():]


@pytest.mark.parametrize("cid", bc.ids("lat", parts=True) + bc.ids("storm", parts=True))
def test_two_parts_lengths(rlo, cid):
    """two parts in one process, every part seeing its peer "on another GPU" (a forged PCI bus, as
    tests/test_gpu_send_storm.py::test_parts), so both store at system scope; a world per length (rlo.sharded runs one
    launch per world).  The latency program: counts, checksums and round ticks; the storm: its logs too"""
    from rlo import sharded

    c = bc.BY_ID[cid]

    def forge(p, blobs):
        return [b if q == p else _forge_bus(b) for q, b in enumerate(blobs)]

    for ln in c.lens:
        exp = expected(c, ln)
        if c.carrier == "lat":
            spec = {"kind": "lat", "rounds": c.k, "len": ln, "seed": c.seed}
        else:
            spec = {"kind": "storm", "k": c.k, "len": ln, "seed": c.seed, "log": True, "log_cap": c.k + 8}
        (st, logs, ms), rcs = bc.create(rlo, lambda: sharded.run_inprocess(
            c.n, c.bounds, spec, max_payload=c.max_payload, uncached=True, blobs_for=forge), c.pull_env)
        print("bcast length case %s len %d parts: last_kernel %s sys_scope %s kernel ms %s" %
              (cid, ln, st["part_last_kernel"].tolist(), st["part_sys_scope"].tolist(), ms))
        assert rcs == [0, 0], (cid, ln, st["error"], st["error_aux"])
        assert (st["part_last_kernel"] == c.kernel).all(), (cid, ln, st["part_last_kernel"])
        assert (st["part_sys_scope"] == c.sys_scope).all(), (cid, ln, st["part_sys_scope"])
        bc.check_stats(cid, exp, st)
        if c.carrier == "lat":
            bc.check_round_ticks(cid, ln, st["round_ticks"], c.k)
        else:
            for r in range(c.n):
                rows, payload = logs[r]
                bc.check_log(cid, exp, r, bc.rows_arrays(rows), payload)


@pytest.mark.parametrize("cid", bc.ids("host"))
def test_host_bcast_lengths(rlo, cid):
    """one HostWorld per case: every rank broadcasts every length that fits through its command ring, in a seeded
    shuffle; per rank the sorted (origin, seq, parent, payload bytes) equals the expected set (parents: orc.tree), and
    the kernel's final counters say that nothing beyond it was delivered"""
    from rlo import abi

    c = bc.BY_ID[cid]
    plan = bc.host_plan(c)
    trees = [orc.tree(c.n, o)[0] for o in range(c.n)]
    sent = {(o, seq): orc.payload(o, seq, ln) for o, seq, ln in plan}
    got = [[] for _ in range(c.n)]
    per_rank = (c.n - 1) * len(c.lens)

    def take(r, ev):
        assert ev["kind"] == abi.RLO_EV_DELIVER_BCAST, (cid, r, ev)
        data = ev.get("payload", b"")
        assert ev["len"] == len(data), (cid, "rank", r, "origin", ev["origin"], "seq", ev["id"], ev["len"], len(data))
        got[r].append((ev["origin"], ev["id"], ev["from"], data))

    with bc.create(rlo, lambda: rlo.HostWorld(c.n, max_payload=c.max_payload), c.pull_env) as hw:
        _check_layout(c, hw.world.info)
        for o, seq, ln in plan:
            hw.bcast(o, sent[(o, seq)], seq=seq)
        t0 = time.time()
        while not all(len(g) >= per_rank for g in got):
            hw.flush()
            for r in range(c.n):
                for ev in hw.poll(r):
                    take(r, ev)
            if time.time() - t0 > 30.0:
                raise AssertionError("%s: host-service world stalled at %s of %d deliveries per rank; errors %s" %
                                     (cid, [len(g) for g in got], per_rank, hw.stats()["error"]))
        for r in range(c.n):  # (what else lies in the pickup rings now; the final counters below say the rest)
            for ev in hw.poll(r):
                take(r, ev)
        info = dict(hw.world.info_now())
    print("bcast length case %s host: last_kernel %d waves %d nsmall %d pull %d ll_ok %d per_cu %d, %d bcasts" %
          (cid, info["last_kernel"], info["waves"], info["nsmall"], info["pull"], info["ll_ok"], info["blocks_per_cu"], len(plan)))
    st = hw.final_stats
    assert info["last_kernel"] == c.kernel
    assert (st["error"] == 0).all(), (cid, st["error"], st["error_aux"])
    for r in range(c.n):
        want = sorted((o, seq, int(trees[o][r]), sent[(o, seq)]) for o, seq, ln in plan if o != r)
        have = sorted(got[r])
        if have != want:
            keys_h, keys_w = [x[:3] for x in have], [x[:3] for x in want]
            assert keys_h == keys_w, (cid, "rank", r, "the (origin, seq, parent) set differs", sorted(set(keys_h) ^ set(keys_w))[:8])
            o, seq, par, data = next(h for h, w_ in zip(have, want) if h != w_)
            exp = sent[(o, seq)]
            at = next((i for i in range(min(len(data), len(exp))) if data[i] != exp[i]), None)
            raise AssertionError("%s rank %d origin %d seq %d parent %d: %d bytes for %d, first differing byte %s" %
                                 (cid, r, o, seq, par, len(data), len(exp), at))
    assert (st["bcast_delivered"] == per_rank).all(), (cid, st["bcast_delivered"])
    assert (st["originated"] == len(c.lens)).all(), (cid, st["originated"])

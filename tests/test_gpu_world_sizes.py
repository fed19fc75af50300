"""GPU parity of every program at every world size 2 .. 33 and on both sides of every power of two up to 256.

The shape of the rootless skip-ring tree is a function of the world size alone, and every kernel derives a message's
children from it with its own code: the hop kernel's register table (worlds of at most 16 ranks), its LDS table (up to
256), the 8-wave storm kernel's forwarding tables, the per-message forms elsewhere, and the vote counts of the
consensus programs.  The rest of the suite runs each program at a handful of sizes; here every size of
tests/world_size_cases.py runs every program, on two worlds per size (A: max_payload 64, 8 waves, doorbells; B:
max_payload 1008, 4 waves, pulled payloads), each world created once per size so that every program also runs behind
another one on it, on a one-XCD world up to 32 ranks, and in two parts of one process with a part of one rank.
Expected values never come from the engine; tests/test_world_sizes_oracle.py checks the inputs on the CPU.
"""
from collections import Counter

import pytest

import bcast_length_cases as bc
import world_size_cases as ws
from decide_cases import launch as decide_launch
from send_cases import check, check_trees_fifo, forge_bus, rlo  # noqa: F401  (rlo: the fixture)
from send_cases import launch_send as send_launch, launch_send_storm as storm_send_launch

pytestmark = pytest.mark.gpu

KERNELS = Counter()  # (world, program, last_kernel) -> launches seen, printed when the module is done


@pytest.fixture(scope="module")
def worlds(rlo):
    """get(kind, n): the world of that kind and size, created once; the worlds of another size are closed first, so at
    most one size's worlds are alive.  drop(kind, n) closes one (after a failure: what it left is not the next test's)"""
    live = {}

    def get(kind, n):
        for key in [key for key in live if key[1] != n]:
            live.pop(key).close()
        if (kind, n) not in live:
            kw, want = ws.WORLDS[kind]
            w = rlo.World(n, **kw)
            got = {key: w.info[key] for key in want}
            if got != want:
                w.close()
                raise AssertionError((kind, n, got, want))
            live[(kind, n)] = w
        return live[(kind, n)]

    def drop(kind, n):
        if (kind, n) in live:
            live.pop((kind, n)).close()

    get.drop = drop
    yield get
    for w in live.values():
        w.close()
    live.clear()
    for world in ws.PROGRAMS:
        for pid, _, _ in ws.PROGRAMS[world]:
            print("world-size launches %s/%s: hop kernel %d, progress kernel %d" %
                  (world, pid, KERNELS[(world, pid, ws.HOP)], KERNELS[(world, pid, ws.PROGRESS)]))


def _seen(w, world, pid, n):
    k = w.info_now()["last_kernel"]
    KERNELS[(world, pid, k)] += 1
    assert k == ws.kernel_of(world, pid, n), (world, pid, n, k)


def _send(w, world, pid, n):
    """the send program, logged: exact dst, counts, checksums, every delivery's tree parent (and per-origin FIFO)"""
    origins, lens, src = ws.send_load(world, pid, n)
    st, got = send_launch(w, origins, lens, src, log=True, log_cap=len(origins))
    _seen(w, world, pid, n)
    check(st, got, n, origins, lens, src)
    check_trees_fifo(w, n, origins, lens)


def _send_storm(w, world, pid, n):
    origins, lens, src = ws.send_load(world, pid, n)
    k, slot = src.shape
    st, got = storm_send_launch(w, origins, lens, src, log=True, log_cap=k)
    _seen(w, world, pid, n)
    check(st, got.reshape(n, k, slot), n, origins, lens, src)
    check_trees_fifo(w, n, origins, lens)


def _storm(w, world, pid, n):
    """the generated storm, logged with payload: delivery sets with parents, payload bytes, counts, checksums"""
    exp = ws.storm_expected(n)
    w.program_storm(exp.k, exp.ln, seed=exp.seed, log=True, log_cap=exp.k + 8)
    w.run()
    _seen(w, world, pid, n)
    bc.check_stats((world, pid, n), exp, w.stats())
    for r in range(n):
        recs, payload = bc.log_arrays(w, r, exp.k + 8)
        bc.check_log("%s/%s n=%d" % (world, pid, n), exp, r, recs, payload)


def _latency(w, world, pid, n):
    """the latency program unlogged and logged (tests/test_gpu_engine.py::test_latency_program): counts, checksums,
    latencies and rank 0's round clock of both launches, and every delivery's parent and bytes from the logged one"""
    exp = ws.latency_expected(n)
    for log in (False, True):
        w.program_latency(exp.k, exp.ln, seed=exp.seed, log=log)
        w.run()
        _seen(w, world, pid, n)
        bc.check_stats((world, pid, n, log), exp, w.stats())
        lat = w.latencies_ticks()
        assert len(lat) == exp.k and (lat > 0).all(), (n, lat)
        bc.check_round_ticks((world, pid, n), exp.ln, w.round_ticks(), exp.k)
    for r in range(n):
        recs, payload = bc.log_arrays(w, r, exp.k + 8)
        bc.check_log("%s/%s n=%d" % (world, pid, n), exp, r, recs, payload)


def _iar(w, world, pid, n):
    """the oracle's judge calls, actions, pickups and results as exact multisets, the lengths in the records, the
    per-rank counters (iar_sets.check_events)"""
    import iar_sets
    from rlo import abi

    c = ws.iar_case(world, n)
    w.program_iar(c.props, judge=abi.RLO_JUDGE_HASH, seed=c.seed, ppm=c.ppm, log=True, log_cap=c.log_cap, pool=1)
    w.run()
    _seen(w, world, pid, n)
    st = w.stats()
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    logs = {r: w.log(r, cap=c.log_cap) for r in range(n)}
    iar_sets.check_events(logs, n, c.props, c.cfg, 1, stats=st, ev=c.ev)


def _decide(w, world, pid, n):
    c = ws.decide_case(n)
    st, logs, dst, dec = decide_launch(w, c)
    _seen(w, world, pid, n)
    c.check(st, logs, dst, dec)


RUN = {"send": _send, "send_storm": _send_storm, "storm": _storm, "latency": _latency, "iar": _iar, "decide": _decide}


def _item(worlds, world, n, pid):
    what = next(p[1] for p in ws.PROGRAMS[world] if p[0] == pid)
    w = worlds(world, n)
    try:
        RUN[what](w, world, pid, n)
    except BaseException:
        worlds.drop(world, n)
        raise


@pytest.mark.parametrize("n,pid", ws.items("A"), ids=lambda v: str(v))
def test_world_a(rlo, worlds, n, pid):
    """World(n, max_payload=64): 8 waves, doorbells -- storm send, the generated storm, the latency program, the send
    program, storm send again with other origins, lengths and buffers"""
    _item(worlds, "A", n, pid)


@pytest.mark.parametrize("n,pid", ws.items("B"), ids=lambda v: str(v))
def test_world_b(rlo, worlds, n, pid):
    """World(n, max_payload=1008): 4 waves, large slots, pulled payloads -- the send program (doorbell and ring), iar
    (the hop kernel up to 16 ranks, the progress kernel beyond), decide (up to 16 ranks), storm send (the small copy
    path and the large-message rounds in one launch), the send program again"""
    _item(worlds, "B", n, pid)


@pytest.mark.parametrize("n,pid", ws.items("X"), ids=lambda v: str(v))
def test_one_xcd(rlo, worlds, n, pid):
    """World(n, max_payload=64, one_xcd=True), 2 .. 32 ranks: the LOC instantiation's placement rendezvous at every
    size -- the latency program, and iar up to 16 ranks"""
    _item(worlds, "X", n, pid)


@pytest.mark.parametrize("forged", [False, True], ids=["agent", "system"])
@pytest.mark.parametrize("n,split,kind", ws.part_items(), ids=lambda v: str(v))
def test_a_part_of_one_rank(rlo, n, split, kind, forged):
    """two parts in one process, one of them a single rank (the first or the last of the world); forged: every part
    sees its peer "on another GPU", so both run at system scope.  Exact outputs, as the programs' own test_parts"""
    from rlo import sharded

    bounds = ws.part_bounds(n)[split]

    def forge(p, blobs):
        return [b if q == p else forge_bus(b) for q, b in enumerate(blobs)]

    if kind == "decide":
        c = ws.decide_case(n)
        spec = {"kind": "decide", "origins": c.origins, "lens": c.lens, "slot": c.slot, "src": c.src,
                "verdict": c.verdict, "log": True, "log_cap": 4 * c.k + 16}
        maxp = 1008
    else:
        origins, lens, src = ws.part_send_load(kind, n)
        spec = {"kind": kind, "origins": origins, "lens": lens, "slot": src.shape[1], "src": src}
        maxp = src.shape[1]
    (st, logs, _), rcs = sharded.run_inprocess(n, bounds, spec, max_payload=maxp, uncached=forged,
                                               blobs_for=forge if forged else None)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == ws.PART_KERNEL[kind]).all(), st["part_last_kernel"]
    assert (st["part_sys_scope"] == (1 if forged else 0)).all()
    if kind == "decide":
        c.check(st, logs, st["dst"], st["decision"])
    else:
        check(st, st["dst"], n, origins, lens, src)

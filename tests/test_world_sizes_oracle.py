"""The inputs of tests/test_gpu_world_sizes.py, checked on the CPU with the oracle alone (no GPU): the table is the one
the issue wrote down, every workload can show what it is meant to show at every size -- a bad seed fails here, not on
the device --, the sizes that leave a program are the listed ones, and the figures the table's comments quote for the
tree (in-degrees, send-list lengths, the LDS table's fill) are the oracle's."""
import numpy as np
import pytest

import iar_sets
import pyoracle as orc
import world_size_cases as ws


def test_the_table_is_the_one_written_down():
    want = list(range(2, 34)) + [63, 64, 65, 100, 127, 128, 129, 200, 255, 256]
    assert list(ws.SIZES) == want and len(set(ws.SIZES)) == 42
    assert ws.PART_SIZES == (2, 3, 5, 16, 17, 33) and set(ws.PART_SIZES) <= set(ws.SIZES)
    assert [p[0] for p in ws.PROGRAMS["A"]] == ["storm-send", "storm", "latency", "send", "storm-send-again"]
    assert [p[0] for p in ws.PROGRAMS["B"]] == ["send", "iar", "decide", "storm-send", "send-again"]
    assert [p[0] for p in ws.PROGRAMS["X"]] == ["latency", "iar"]
    assert ws.WORLDS["A"][0] == {"max_payload": 64} and ws.WORLDS["B"][0] == {"max_payload": 1008}
    assert ws.WORLDS["X"][0] == {"max_payload": 64, "one_xcd": True}


def test_only_the_listed_sizes_leave_a_program():
    """every (world, program, size) runs but decide and hop iar beyond 16 ranks and one-XCD beyond 32"""
    assert set(ws.LEFT_OUT) == {("B", "decide"), ("X", "latency"), ("X", "iar")}
    over16 = [n for n in ws.SIZES if n > 16]
    over32 = [n for n in ws.SIZES if n > 32]
    assert len(over16) == 27 and len(over32) == 11
    gone = {"A": set(), "B": {("decide", n) for n in over16},
            "X": {("latency", n) for n in over32} | {("iar", n) for n in over16}}
    for world, progs in ws.PROGRAMS.items():
        every = {(p[0], n) for n in ws.SIZES for p in progs}
        run = ws.items(world)
        assert len(run) == len(set(run)) and {(pid, n) for n, pid in run} == every - gone[world], world
        assert [n for n, _ in run] == sorted(n for n, _ in run)  # size by size: one world per size at a time
    assert len(ws.items("A")) == 5 * 42 and len(ws.items("B")) == 5 * 42 - 27 and len(ws.items("X")) == 31 + 15
    # iar stays at every size of world B: the hop kernel up to 16 ranks, the progress kernel beyond
    assert [ws.kernel_of("B", "iar", n) for n in (2, 16, 17, 256)] == [1, 1, 0, 0]
    assert all(n <= 16 or kind != "decide" for n, _, kind in ws.part_items())
    assert len(ws.part_items()) == 11 * 2 + 7  # 11 splits of 6 sizes; 7 of them in worlds of at most 16 ranks
    for n in ws.PART_SIZES:
        b = ws.part_bounds(n)
        assert b == ([[0, 1, 2]] if n == 2 else [[0, 1, n], [0, n - 1, n]])


@pytest.mark.parametrize("n", ws.SIZES)
def test_send_lists(n):
    """each send and storm-send list: every rank originates at least twice, every rank receives over each of its
    in-edges on each virtual channel it has, and the lengths the list is there for occur"""
    for (world, pid), (slot, per, storm, base, must) in ws.SENDS.items():
        origins, lens, src = ws.send_load(world, pid, n)
        k = len(origins)
        assert k == n * max(per, -(-len(must) // n)) and src.shape == (k, slot) and lens.min() >= 1 and lens.max() <= slot
        assert k == per * n or (world, pid, n) in {("B", "storm-send", 2), ("B", "storm-send", 3), ("B", "storm-send", 4)}
        assert sorted(origins[:n].tolist()) == list(range(n))  # a permutation of the ranks,
        assert np.array_equal(origins, np.tile(origins[:n], k // n))  # repeated
        ws.send_conditions(n, origins, lens, must, per=2)
    if n in ws.PART_SIZES:
        for kind, (slot, per, storm, base, must) in ws.PART_SENDS.items():
            origins, lens, src = ws.part_send_load(kind, n)
            ws.send_conditions(n, origins, lens, must, per=2)
    # two launches of one program on one world differ in origins, lengths and bytes
    a, b = ws.send_load("A", "storm-send", n), ws.send_load("A", "storm-send-again", n)
    assert not np.array_equal(a[2], b[2]) and (n == 2 or not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1]))


def test_both_virtual_channels_occur():
    """the wrap past rank n - 1 (child < origin) is on some in-edge of every world, and from 3 ranks on some rank
    receives over one edge on both channels"""
    for n in ws.SIZES:
        e = ws.in_edges(n)
        assert {vc for s in e.values() for _, vc in s} == {0, 1}, n
        both = [r for r, s in e.items() if any((p, 0) in s and (p, 1) in s for p, _ in s)]
        assert both or n == 2, n


@pytest.mark.parametrize("n", ws.SIZES)
def test_iar_cases(n):
    for world in ("B", "X"):
        if world == "X" and n > ws.HOP_CONSENSUS_MAX:
            continue
        c = ws.iar_case(world, n)
        per = 8 if (world, n) == ("B", 2) else 2
        assert len(c.props) == per * n and {len(d) for _, _, d in c.props} <= set(ws.IAR_LENS[world])
        assert all(16 + len(d) <= ws.WORLDS[world][0]["max_payload"] for _, _, d in c.props)
        assert abs((1 - c.ppm / 1e6) ** (n - 1) - 0.75) < 1e-3  # about a quarter of the proposals is declined
        iar_sets.input_conditions(c.props, c.ev)
        for seed in range(1, c.seed):  # the first seed that meets them
            cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_HASH, seed=seed, ppm=c.ppm)
            with pytest.raises(AssertionError):
                iar_sets.input_conditions(c.props, iar_sets.oracle_events(n, c.props, cfg, 1, cap=4 * len(c.props) * n + 1024))
        assert c.log_cap >= max(np.bincount([e[1] for e in c.ev]))
    if n >= 5:  # every length of world B's list occurs (2 proposals per rank walk the list)
        assert {len(d) for _, _, d in ws.iar_case("B", n).props} == set(ws.IAR_LENS["B"])


def test_iar_two_ranks_need_more_proposals():
    """why world B takes 8 proposals per rank at 2 ranks: 2 per rank are four proposals of four lengths"""
    props = iar_sets.mixed_props(2, 2, ws.IAR_LENS["B"], 9002)
    assert len({len(d) for _, _, d in props}) == len(props) == 4


@pytest.mark.parametrize("n", range(2, 17))
def test_decide_cases(n):
    c = ws.decide_case(n)
    ws.decide_conditions(n, c)
    assert c.slot == 992 and c.k == (16 if n == 2 else 4 * n) and c.ppm == 60000 * 7 // (n - 1)
    seeds = {2: 569, 3: 421, 4: 141, 5: 67, 6: 4}
    assert c.seed == seeds.get(n, c.seed) and 1 <= c.seed <= (4 if n > 6 else 569)
    if n == 2:  # what Case.conditions asks cannot hold: one judge, always reached
        with pytest.raises(AssertionError, match="every proposal reached every rank"):
            c.conditions()
        assert any(v == 0 for v in c.result.values())


def test_tree_figures():
    """the figures the table quotes, from orc.tree alone: the largest in-degree is <= 4 iff n <= 16 (the hop kernel's
    register table holds for exactly those worlds), 5 from 17, 6 from 33, 7 from 65, 8 from 129; n x the largest
    in-degree stays within the hop kernel's LDS table of 2048 pairs and fills it exactly at 256 ranks"""
    deg = {n: ws.max_in_degree(n) for n in ws.SIZES}
    for n, d in deg.items():
        assert (d <= 4) == (n <= 16), (n, d)
        assert d == (8 if n >= 129 else 7 if n >= 65 else 6 if n >= 33 else 5 if n >= 17 else d), (n, d)
        assert n * d <= 2048 and (n * d == 2048) == (n == 256), (n, d)
        # an in-degree is a send-list length seen from the other side: the largest of both agree
        assert d == max(orc.topology(n, r)["send_list_len"] for r in range(n)), n
    assert deg[16] == 4 and deg[255] * 255 == 2040
    # the first world past the LDS table: 257 ranks, 9 in-edges (the send program's computed path, which
    # tests/test_gpu_send.py runs at 300 ranks; no size of this table reaches it)
    assert ws.max_in_degree(257) == 9 and 257 * 9 > 2048


@pytest.mark.parametrize("n", ws.SIZES)
def test_generated_programs(n):
    """the generated storm (8 n bcasts) and the latency program (64 rounds) draw random origins, and their expectations
    are the oracle's, per rank.  With its seed the storm has every rank originate at every size of the table; the
    latency program's 64 rounds cannot from 65 ranks on and do not at most sizes below: that every rank originates
    and receives over each of its in-edges is what the send and storm-send lists are for (test_send_lists)"""
    exp = ws.storm_expected(n)
    assert exp.k == 8 * n and exp.ln == 64 and int(exp.count.sum()) == exp.k * (n - 1)
    assert set(exp.origin.tolist()) == set(range(n))
    lat = ws.latency_expected(n)
    assert lat.k == 64 and lat.ln == 64 and int(lat.count.sum()) == 64 * (n - 1)


class _FakeLogs:
    """what send_cases.check_trees_fifo reads of a world, served from arrays made here: rlo_log's records per rank"""

    def __init__(self, recs):
        self.recs, self.info, self.h, self.lib = recs, {"slot_stride": 80}, None, self

    def rlo_log(self, h, rank, out, cap, payload, stride):
        import ctypes

        r = np.ascontiguousarray(self.recs[rank][:cap], dtype=np.uint32)
        ctypes.memmove(out, r.ctypes.data, r.nbytes)
        return len(r)


def _true_logs(n, origins, lens, rng):
    """a log a correct launch could leave: at every rank each origin's messages in sending order, the origins
    interleaved at random"""
    parent = [orc.tree(n, o)[0] for o in range(n)]
    logs = []
    for r in range(n):
        by_origin = {}
        for i in range(len(origins)):
            if origins[i] != r:
                by_origin.setdefault(int(origins[i]), []).append(i)
        order = rng.permutation([o for o, v in by_origin.items() for _ in v]).tolist()
        rows = []
        for o in order:
            i = by_origin[o].pop(0)
            rows.append((1, o, parent[o][r], i, lens[i], 0, 0, 0xFFFFFFFF))
        logs.append(np.array(rows, dtype=np.int64).astype(np.uint32))
    return logs


@pytest.mark.parametrize("n", [2, 5, 17])
def test_the_log_comparison_notices(n):
    """send_cases.check_trees_fifo (the comparison the send and storm-send tests share) passes a correct log and fails
    on a wrong parent, a wrong length, two of an origin's messages swapped, a record twice, a record missing, a
    record of the rank's own message and a record that carries a payload copy"""
    from send_cases import check_trees_fifo

    origins, lens, _ = ws.send_load("A", "storm-send", n)
    rng = np.random.default_rng(n)
    good = _true_logs(n, origins, lens, rng)
    check_trees_fifo(_FakeLogs(good), n, origins, lens)
    r = n - 1
    o = int(good[r][0, 1])
    mine = np.nonzero(good[r][:, 1] == o)[0]
    assert len(mine) >= 2

    def broken(change):
        logs = [g.copy() for g in good]
        logs[r] = change(logs[r])
        with pytest.raises(AssertionError):
            check_trees_fifo(_FakeLogs(logs), n, origins, lens)

    def put(col, value, row=0):
        def change(a):
            a[row, col] = value
            return a
        return change

    def swap(a):
        a[[mine[0], mine[1]]] = a[[mine[1], mine[0]]]
        return a

    own = int(np.nonzero(origins == r)[0][0])
    broken(put(2, r))                                     # `from` is never the rank itself
    broken(put(2, (int(good[r][0, 2]) + 1) % n) if n > 2 else put(2, 7))  # another rank than the tree's parent
    broken(put(4, int(good[r][0, 4]) + 1))               # the length
    broken(swap)                                          # per-origin FIFO
    broken(lambda a: np.concatenate([a, a[:1]]))          # a delivery twice
    broken(lambda a: a[1:])                               # a delivery missing
    broken(lambda a: np.concatenate([a[1:], np.array([[1, r, 0, own, lens[own], 0, 0, 0xFFFFFFFF]], dtype=np.uint32)]))
    broken(put(7, 0))                                     # a payload copy
    broken(put(0, 1 | 4 << 8))                            # another tag

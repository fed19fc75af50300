"""What tests/test_gpu_iar_payloads.py and the long-proposal cases of tests/test_gpu_host.py rely on, on the CPU.

Those tests give the oracle inputs no fixture of the compiled reference covers (proposals of up to 4080 bytes), and
take their expected values from it.  Pinned here: the oracle's events do not depend on the data length but for the
one field that carries it; its ISP judge is the rule of testcases.c:18-37, restated; and every GPU case's inputs
(generator, seed) meet the conditions the case asserts, so that a bad seed fails here and not on the GPU.
"""
import numpy as np
import pytest

import iar_payload_cases as pc
import iar_sets
import pyoracle as orc


def test_mixed_props_rule():
    n, per, lens = 5, 4, (0, 7, 33, 100)
    props = iar_sets.mixed_props(n, per, lens, 3)
    assert props == iar_sets.mixed_props(n, per, lens, 3)  # seeded
    assert [(o, pid) for o, pid, _ in props] == [(r, it * n + r) for it in range(per) for r in range(n)]
    assert [len(d) for _, _, d in props] == [lens[(it * n + r + it) % len(lens)] for it in range(per) for r in range(n)]
    for r in range(n):  # every rank: several different lengths in succession
        mine = [len(d) for o, _, d in props if o == r]
        assert all(a != b for a, b in zip(mine, mine[1:])), (r, mine)
    assert iar_sets.blob_offsets(props)[:3] == [0, len(props[0][2]), len(props[0][2]) + len(props[1][2])]
    long = iar_sets.mixed_props(8, 2, (4080,), 1)
    assert len(set(b"".join(d for _, _, d in long))) == 256  # all byte values


@pytest.mark.parametrize("pool", [0, 1, 4])
@pytest.mark.parametrize("judge", ["mask", "hash"])
def test_oracle_events_do_not_depend_on_the_data_length(judge, pool):
    """orc.iar on proposals of 0 .. 4080 bytes equals orc.iar on the same proposals with 16-byte data, event for
    event and in order, once the ACTION event's length field is mapped"""
    n, per = 13, (1 if pool == 0 else 5)
    props = iar_sets.mixed_props(n, per, pc.L, 7)
    assert pool == 0 or {len(d) for _, _, d in props} == set(pc.L)
    short = [(o, pid, b"0123456789abcdef") for o, pid, _ in props]
    if judge == "mask":
        decline = np.zeros(n, dtype=np.uint8)
        decline[4] = 1  # (rank 4 alone: its own proposals are approved, every other one declined)
        cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_MASK, decline=decline)
    else:
        cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_HASH, seed=7, ppm=24000)
    ev_long = orc.iar(n, props, cfg, cap=1 << 18, pool=pool)
    ev_short = orc.iar(n, short, cfg, cap=1 << 18, pool=pool)
    dl = {(o, pid): len(d) for o, pid, d in props}
    assert not [e for e in ev_long if e[0] == orc.ORC_EV_ERROR]
    assert any(e[0] == orc.ORC_EV_ACTION for e in ev_long) and any(e[0] == orc.ORC_EV_RESULT and e[3] == 0 for e in ev_long)
    mapped = [(e[0], e[1], e[2], e[3], dl[(e[5], e[2])], e[5]) if e[0] == orc.ORC_EV_ACTION else e for e in ev_short]
    assert all(e[4] == 16 for e in ev_short if e[0] == orc.ORC_EV_ACTION)
    assert ev_long == mapped


def isp_rule(mine, arg):
    """testcases.c:18-37 from its definition.  mine: this rank's string (bytes, no NUL); arg: the proposal's data as
    the judge gets it, a C string in a zeroed buffer one byte longer than the data (None: the NULL call)"""
    if not mine or arg is None:
        return 1
    text = arg.split(b"\0")[0]  # what strcmp sees
    if mine == text:
        return 1
    first = arg[0] if arg else 0  # (the terminator of an empty argument)
    first = first - 256 if first >= 128 else first  # char is signed
    return 0 if first < mine[0] else 1


def _isp_verdicts(n, props, isp):
    cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_ISP, isp=isp)
    ev = orc.iar(n, props, cfg, cap=1 << 18)
    assert not [e for e in ev if e[0] == orc.ORC_EV_ERROR]
    data = {(o, pid): d for o, pid, d in props}
    calls = [(e[1], e[5], e[2], e[3], e[4]) for e in ev if e[0] == orc.ORC_EV_JUDGE]
    for rank, origin, pid, null, verdict in calls:
        want = isp_rule(isp[rank].encode(), None if null else data[(origin, pid)])
        assert verdict == want, (rank, origin, pid, null, verdict, want)
    return ev, calls


@pytest.mark.parametrize("n,maxp,dl,kernel", pc.ISP_WORLDS)
def test_isp_subcases_behave_as_described(n, maxp, dl, kernel):
    for name in pc.ISP_SUBCASES:
        props, isp = pc.isp_case(n, dl, name)
        assert all(s and s.isascii() and "\0" not in s for s in isp)
        ev, calls = _isp_verdicts(n, props, isp)
        asked = [(rank, verdict) for rank, origin, pid, null, verdict in calls if not null]
        assert iar_sets.outcomes(ev) == {(3, 103): pc.ISP_DECISION[name]}, name
        if pc.ISP_DECISION[name]:
            assert len(asked) == n - 1 and all(v == 1 for _, v in asked), name
        elif name == "one-larger-first":  # that rank alone declines
            assert [r for r, v in asked if v == 0] == [n - 1], name
        else:  # the first receivers decline: nothing is forwarded
            kids = orc.children(n, 3, 3, -1)
            assert sorted(asked) == sorted((k, 0) for k in kids), name
    data = pc.isp_case(n, dl, "high-first-byte")[0][0][2]
    assert data[0] >= 0x80 and pc.isp_case(n, dl, "embedded-nul")[0][0][2].count(0) == 1


def test_isp_rule_on_seeded_pairs():
    """a few hundred (string, data) pairs of up to 4080 bytes: equal, differing late, differing in the first byte
    either way, bytes >= 0x80, NULs, and one a prefix of the other"""
    rng = np.random.default_rng(11)
    n, asked = 4, 0
    for i in range(120):
        dl = int(rng.choice([0, 1, 2, 15, 16, 17, 97, 353, 993, 4080]))
        data = bytearray(rng.integers(0x21, 0x7f, size=dl, dtype=np.uint8).tobytes())
        isp = []
        for r in range(n):
            s = bytearray(data)
            how = int(rng.integers(0, 7))
            if how == 1 and s:
                s[-1] = 0x21 + (s[-1] - 0x20) % 0x5e  # another last byte
            elif how == 2 and s:
                s[0] = 0x21 + (s[0] - 0x20) % 0x5e  # another first byte
            elif how == 3:
                s = s[:len(s) // 2]
            elif how == 4:
                s += b"tail"
            elif how == 5:
                s = bytearray(rng.integers(0x21, 0x7f, size=int(rng.integers(1, 40)), dtype=np.uint8).tobytes())
            elif how == 6:
                s = bytearray()  # an empty own string approves
            isp.append(s.decode("ascii"))
        what = int(rng.integers(0, 4))
        if what == 1 and dl:
            data[0] = int(rng.integers(0x80, 0x100))
        elif what == 2 and dl > 1:
            data[int(rng.integers(0, dl))] = 0
        elif what == 3 and dl:
            data[int(rng.integers(0, dl))] = int(rng.integers(0x80, 0x100))
        ev, calls = _isp_verdicts(n, [(i % n, 500 + i, bytes(data))], isp)
        asked += sum(1 for c in calls if not c[3])
    assert asked >= 200, asked


def _all_cases():
    return [(c.id, c) for c in pc.CASES] + [(c[0], pc.part_case(c[0])[1]) for c in pc.PART_CASES]


@pytest.mark.parametrize("cid", [cid for cid, _ in _all_cases()])
def test_device_case_inputs(cid):
    """the conditions every GPU case asserts on its inputs hold: every length it uses has an approved proposal, a
    proposal is declined, and where the case asks for it the data offsets of the proposals beyond 16 bytes cover
    every residue mod 4; the world each case names has the layout the case is about"""
    import rlo

    c = dict(_all_cases())[cid]
    props = c.proposals()
    assert len(props) <= 400 and 1 <= c.per <= 6
    assert set(len(d) for _, _, d in props) == set(c.lens)
    cfg, keep = c.oracle_cfg()
    c.check_inputs(props, iar_sets.oracle_events(c.n, props, cfg, c.pool))
    if c.judge == "mask":  # the one declining rank submits every length
        assert sorted(len(d) for o, _, d in props if o == c.n - 2) == sorted(c.lens)
    kw = {k: v for k, v in c.world.items() if k != "one_xcd"}
    plan = rlo.layout_plan(c.n, **kw)
    assert c.waves in (None, plan["waves"]) and c.nsmall in (None, plan["nsmall"]), plan
    assert plan["ll_ok"] == 1  # doorbells: the hop kernel where the launch allows it, the bell pass elsewhere


def test_device_cases_cover_the_lengths():
    assert set(pc.L) == {0, 1, 15, 16, 17, 32, 33, 48, 49, 96, 97, 352, 353, 992, 993, 4079, 4080}
    used = set()
    for c in pc.CASES:
        used |= set(c.lens)
    assert used >= set(pc.L)
    assert pc.lens_for(1008)[-1] == 992 and pc.lens_for(112)[-1] == 96 and pc.lens_for(64)[-1] == 48
    assert pc.lens_for(368)[-1] == 352 and pc.lens_for(4096)[-1] == 4080
    for ident in ("hop-mixed", "n16-mixed", "n17-mixed", "n64-mixed", "w8-n17-112-mixed", "w8-n17-64-mixed",
                  "w4-n17-368-mixed"):  # a mixed launch holds every length its world takes
        c = pc.BY_ID[ident]
        assert c.lens == pc.lens_for(c.world["max_payload"]), ident
    assert pc.BY_ID["hop-mixed"].offsets


@pytest.mark.parametrize("n,maxp,lens,pool,pend_hbm,seed", pc.HOST_CASES)
def test_host_case_inputs(n, maxp, lens, pool, pend_hbm, seed):
    props, cfg, keep, ppm = pc.host_case(n, lens, seed)
    assert all(16 + len(d) <= maxp for _, _, d in props) and max(lens) == maxp - 16
    for r in range(n):
        assert sorted(len(d) for o, _, d in props if o == r) == sorted(lens)
    iar_sets.input_conditions(props, iar_sets.oracle_events(n, props, cfg, pool))

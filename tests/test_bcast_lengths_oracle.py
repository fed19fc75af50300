"""What tests/test_gpu_bcast_lengths.py relies on, on the CPU: the oracle, rlo.layout_plan and rlo_kernel_pick alone.

The GPU tests take every expected count, checksum, parent and byte from the oracle at lengths no fixture of the
compiled reference covers (0 .. 65520 bytes).  Pinned here: every case's inputs (seed, rounds) meet the conditions the
case is about, so that a bad seed fails here and not on the GPU; the oracle's two ways to a storm's checksums agree at
every length; the message checksum tells lengths, chunk positions and padding bytes apart, which is what lets a row
compared by checksum alone stand for the bytes; every case's world has the layout it names and its launches pick the
kernel it names; and the case table leaves no boundary length out.
"""
import ctypes
import os

import numpy as np
import pytest

import bcast_length_cases as bc
import pyoracle as orc

ALL_IDS = [c.id for c in bc.CASES]


def test_the_table():
    assert bc.L == (0, 1, 15, 16, 17, 64, 65, 112, 113, 368, 369, 1008, 1009, 1024, 1025, 2048, 2049, 4096, 4097, 32767,
                    32768, 65519, 65520)
    assert [bc.chunks(x) for x in (0, 1, 16, 17, 64, 65, 112, 113, 368, 369, 1008, 1009)] == [1, 2, 2, 3, 5, 6, 8, 9, 24, 25,
                                                                                             64, 65]
    assert bc.lens_for(112) == (0, 1, 15, 16, 17, 64, 65, 111, 112)
    assert bc.lens_for(368) == (0, 1, 15, 16, 17, 64, 65, 112, 113, 367, 368)
    assert bc.lens_for(1008)[-4:] == (368, 369, 1007, 1008) and bc.lens_for(4096)[-3:] == (2049, 4095, 4096)
    assert bc.lens_for(65520)[-3:] == (32768, 65519, 65520) and len(bc.lens_for(65520)) == len(bc.L)
    for a, b in bc.PAIRS:  # every table length is one side of a pair
        assert b == a + 1
    assert {x for p in bc.PAIRS for x in p} >= set(bc.L)


@pytest.mark.parametrize("cid", [c.id for c in bc.CASES if c.carrier != "host"])
def test_case_inputs(cid):
    """in every launch (whatever its length: originators and trees do not depend on it) of a world of at most 64
    ranks every rank originates, receives as a leaf and receives as a forwarding rank; and at every length of the case
    the simulated storm's counts and checksums equal the analytic ones"""
    c = bc.BY_ID[cid]
    assert 48 <= c.k <= 64 or (c.n > 17 and c.k <= 4 * c.n), (c.n, c.k)
    par0 = None
    for ln in c.lens:
        ref = orc.storm(c.n, c.seed, c.k, ln, want_parent=True)
        exp = orc.storm_expected(c.n, c.seed, c.k, ln)
        assert np.array_equal(ref["sum"], exp["sum"]) and np.array_equal(ref["count"], exp["count"]), (cid, ln)
        assert ref["deliveries"] == exp["deliveries"] == c.k * (c.n - 1)
        if par0 is None:
            par0 = ref["parent"]
        assert np.array_equal(ref["parent"], par0), (cid, ln)
    if c.n <= 64:
        leaves, fwds = bc.input_conditions(c.n, c.seed, c.k, par0)
        assert leaves == c.n and fwds >= c.n // 2  # (in a skip-ring tree only every other rank ever forwards)
    for b in range(c.k):  # the parents are tree edges of the origin's tree
        o = orc.origin_of(c.seed, b, c.n)
        if b < 8 or c.n <= 17:
            assert np.array_equal(np.delete(par0[b], o), np.delete(orc.tree(c.n, o)[0], o)), (cid, b)


@pytest.mark.parametrize("cid", bc.ids("host"))
def test_host_case_inputs(cid):
    c = bc.BY_ID[cid]
    plan = bc.host_plan(c)
    assert plan == bc.host_plan(c) and plan != sorted(plan)  # seeded, and shuffled
    assert len({seq for _, seq, _ in plan}) == len(plan) == c.n * len(c.lens)
    for r in range(c.n):
        assert sorted(ln for o, _, ln in plan if o == r) == list(c.lens)
    assert c.lens == bc.lens_for(c.max_payload)
    leaf, fwd = bc.roles(c.n)  # every rank broadcasts, so every rank takes every role its trees give it
    assert len(leaf) == c.n and len(fwd) >= c.n // 2


def py_checksum(origin, bid, tag, padded, ln):
    """orc_msg_checksum restated over a buffer that already holds its padding: the header term carries the length, each
    16-byte chunk its index"""
    mix = orc.lib().orc_chunk_mix
    s = mix(0xFFFFFFFF, origin, bid, tag, ln)
    w = np.frombuffer(padded, dtype="<u4")
    for q in range((ln + 15) // 16):
        s += mix(q, int(w[4 * q]), int(w[4 * q + 1]), int(w[4 * q + 2]), int(w[4 * q + 3]))
    return s & 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("a,b", bc.PAIRS)
def test_checksum_tells_lengths_positions_and_padding_apart(a, b):
    origin, bid = 3, 41
    long = orc.payload(origin, bid, b)
    short = long[:a]
    assert orc.payload(origin, bid, a) == short  # equal leading bytes: the payload is a prefix of the longer one
    cs = {orc.msg_checksum(origin, bid, 0, short), orc.msg_checksum(origin, bid, 0, long),
          orc.msg_checksum(origin, bid, 0, short + b"\0")}  # (a zero byte more: the length alone differs)
    assert len(cs) == 3, (a, b)
    for ln in (a, b):
        data = orc.payload(origin, bid, ln)
        pad = (ln + 15) // 16 * 16
        padded = bytearray(data + bytes(pad - ln))
        assert py_checksum(origin, bid, 0, bytes(padded), ln) == orc.msg_checksum(origin, bid, 0, data), ln
        if pad > ln:  # one padding byte set: the last, and the first
            for at in {pad - 1, ln}:
                bad = bytearray(padded)
                bad[at] = 1
                assert py_checksum(origin, bid, 0, bytes(bad), ln) != orc.msg_checksum(origin, bid, 0, data), (ln, at)
        if ln >= 32:  # two 16-byte chunks exchanged: the first and the last whole one
            last = (ln // 16 - 1) * 16
            sw = bytearray(data)
            sw[0:16], sw[last:last + 16] = data[last:last + 16], data[0:16]
            assert bytes(sw) != data and orc.msg_checksum(origin, bid, 0, bytes(sw)) != orc.msg_checksum(origin, bid, 0, data), ln
        if ln:  # one byte of the last chunk flipped
            fl = bytearray(data)
            fl[ln - 1] ^= 0x80
            assert orc.msg_checksum(origin, bid, 0, bytes(fl)) != orc.msg_checksum(origin, bid, 0, data), ln
    # ... and another origin or bid with the same bytes
    assert orc.msg_checksum(origin + 1, bid, 0, long) != orc.msg_checksum(origin, bid, 0, long)
    assert orc.msg_checksum(origin, bid + 1, 0, long) != orc.msg_checksum(origin, bid, 0, long)


def _plans(c):
    import rlo

    parts = 1 if c.bounds is None else len(c.bounds) - 1
    if c.pull_env is not None:
        os.environ["RLO_PULL"] = c.pull_env
    try:
        return [rlo.layout_plan(c.n, parts, p, cus=256, **c.plan_kw()) for p in range(parts)]
    finally:
        os.environ.pop("RLO_PULL", None)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_layout(cid):
    """the world each case names has the layout the case is about (rlo.layout_plan on a GPU of 256 CUs)"""
    c = bc.BY_ID[cid]
    for plan in _plans(c):
        got = {k: plan[k] for k in ("waves", "nsmall", "pull", "ll_ok", "blocks_per_cu")}
        assert got == {"waves": c.waves, "nsmall": c.nsmall, "pull": c.pull, "ll_ok": c.ll_ok, "blocks_per_cu": c.per_cu}, (cid, got)
        assert plan["slot_stride"] == c.max_payload + 16 and plan["pend_hbm"] == (1 if c.world.get("pend_hbm") else 0)
        assert plan["bulk_max"] == c.bulk_max
        if "ring_slots" in c.world:
            assert plan["ring_slots"] == c.world["ring_slots"]
    if cid == "storm-small-stage":
        assert _plans(c)[0]["stage2_bytes"] == 5 * 1024  # five 1-KiB units: a 4096-B message's group does not fit twice
    assert c.may_skip == (c.n > 256)  # only worlds of more ranks than CUs may skip, on RLO_E_OCCUPANCY


def _pick(kernel, variant, mode, pend_hbm, sys_scope):
    from rlo import _lib as lib

    out = (ctypes.c_uint32 * 5)()
    rc = lib.load().rlo_kernel_pick(kernel, variant, mode, pend_hbm, sys_scope, out)
    return tuple(out) if rc == lib.RLO_OK else None


def hop_takes(c, ln):
    """plan_hop's rule for the latency program, restated: doorbells, no bulk world, no phase profile, at most 64
    chunks"""
    return bool(c.ll_ok) and not c.bulk_max and not c.prof and bc.chunks(ln) <= 64


@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_kernel_pick(cid):
    """rlo_kernel_pick gives the instantiation the case names for the mode bits of its program, and every length of
    a latency case falls on the side of plan_hop's limit its expected kernel says"""
    c = bc.BY_ID[cid]
    pend_hbm = 1 if c.world.get("pend_hbm") else 0
    got = _pick(c.kernel, 0 if c.kernel == bc.HOP else c.variant(), c.mode(), pend_hbm, c.sys_scope)
    assert got == c.inst, (cid, got, c.inst)
    if c.carrier == "lat":
        for ln in c.lens:
            assert hop_takes(c, ln) == (c.kernel == bc.HOP), (cid, ln)
        # the 8-wave kernel has bells only while the message fits its staged chunks (ll_mode)
        assert c.waves != 8 or all(bc.chunks(ln) <= c.nsmall for ln in c.lens)
    else:
        assert c.kernel == bc.PROGRESS
    if cid == "lat-bulk-ring":
        assert [ln for ln in c.lens if ln > c.max_payload] == [c.max_payload + 1]  # one bulk length, the first


def test_table_coverage():
    """every boundary length appears in at least one case of every carrier whose slots can hold it; every length up to
    1008 in a hop-kernel latency case; every length in 1009 .. 4097 in a pulled and in a pushed progress-kernel
    latency case.  The share of table cells left out is zero"""
    missing = []
    for carrier in ("lat", "storm", "host"):
        cases = [c for c in bc.CASES if c.carrier == carrier]
        slot = max(c.max_payload for c in cases)
        used = {ln for c in cases for ln in c.lens if ln <= c.max_payload}
        missing += [(carrier, ln) for ln in bc.L if ln <= slot and ln not in used]
        for c in cases:  # and the slot's own last two lengths where the case takes all that fit
            if len(c.lens) > 8 and c.carrier != "lat" or c.id in ("lat-hop-112", "lat-hop-1008"):
                assert c.lens == bc.lens_for(c.max_payload), c.id
    lat = [c for c in bc.CASES if c.carrier == "lat"]
    hop = {ln for c in lat if c.kernel == bc.HOP for ln in c.lens}
    missing += [("lat hop", ln) for ln in bc.L if ln <= 1008 and ln not in hop]
    for pull in (1, 0):
        big = {ln for c in lat if c.kernel == bc.PROGRESS and c.pull == pull and c.ll_ok and not c.bulk_max and not c.prof
               for ln in c.lens}
        missing += [("lat progress pull %d" % pull, ln) for ln in bc.L if 1009 <= ln <= 4097 and ln not in big]
    storm = [c for c in bc.CASES if c.carrier == "storm"]
    for pull in (1, 0):  # the storm's large path pulled and pushed, to the largest slot
        big = {ln for c in storm if c.pull == pull and c.nsmall == 5 and c.max_payload > 64 for ln in c.lens}
        missing += [("storm pull %d" % pull, ln) for ln in bc.L if ln not in big]
    cells = 3 * len(bc.L)
    print("table cells left out: %d of %d" % (len(missing), cells))
    assert not missing, missing
    # the cases the table must at least hold
    assert {c.id for c in bc.CASES} >= {
        "lat-hop-112", "lat-hop-1008", "lat-hop-1008-n13", "lat-hop-1008-n64", "lat-hop-pend-hbm", "lat-hop-one-xcd-n8",
        "lat-hop-one-xcd-n32", "lat-hop-parts", "lat-big-pull", "lat-big-push", "lat-big-n13", "lat-max-pull", "lat-max-push",
        "lat-big-parts", "lat-medium", "lat-no-bells-64", "lat-no-bells-1008", "lat-bulk-ring", "lat-prof-8w", "storm-8w-n8",
        "storm-8w-n64", "storm-8w-64", "storm-medium-n8", "storm-medium-n17", "storm-large-pull-n8", "storm-large-pull-n13",
        "storm-large-push-n8", "storm-large-push-n13", "storm-max-pull", "storm-max-push", "storm-small-stage",
        "storm-parts", "host-112", "host-368", "host-4096", "host-32784"}
    assert bc.BY_ID["storm-8w-n8"].windows == bc.BY_ID["storm-8w-n64"].windows == (64, 1)
    assert bc.BY_ID["lat-hop-one-xcd-n8"].launches == bc.BY_ID["lat-hop-one-xcd-n32"].launches == 3


def _fake_log(exp, rank):
    """the log a correct device would return for one rank: records in bid order and the padded payload rows"""
    bids = np.nonzero(exp.origin != rank)[0]
    recs = np.zeros((len(bids), 8), dtype=np.uint32)
    recs[:, 0] = bc.LOG_DELIVER | bc.TAG_BCAST << 8
    recs[:, 1], recs[:, 2], recs[:, 3], recs[:, 4] = exp.origin[bids], exp.parent[bids, rank], bids, exp.ln
    recs[:, 7] = np.arange(len(bids))
    payload = np.zeros((len(bids) + 8, 4096), dtype=np.uint8)
    payload[:len(bids), :exp.pad] = exp.bytes[bids, :exp.pad]
    return recs, payload


def test_comparisons_fail_on_a_wrong_byte_length_parent_or_padding():
    """the GPU tests' comparison (bc.check_log) on the expectation side alone: a correct log passes; one byte of the last
    partial chunk of a 1009-byte message, one record's length, two exchanged parents, one nonzero padding byte, a
    delivery missing or twice each fail with a message that names the rank, the bid and the length"""
    n, seed, k, ln, rank = 8, 1, 64, 1009, 4  # (rank 4 has three different parents)
    exp = bc.Expected(n, seed, k, ln)
    recs, payload = _fake_log(exp, rank)
    bc.check_log("case", exp, rank, recs[::-1].copy(), payload)  # in any order
    bid = int(recs[7, 3])
    bad = payload.copy()
    bad[7, 1008] ^= 1
    with pytest.raises(AssertionError, match=r"len 1009 rank 4 bid %d .*byte 1008 " % bid):
        bc.check_log("case", exp, rank, recs, bad)
    bad = payload.copy()
    bad[7, 1023] = 9  # the padding's last byte
    with pytest.raises(AssertionError, match=r"len 1009 rank 4 bid %d .*byte 1023 .*padding" % bid):
        bc.check_log("case", exp, rank, recs, bad)
    short = recs.copy()
    short[7, 4] = ln - 1
    with pytest.raises(AssertionError, match=r"len 1009 rank 4 bid %d: the record's len is 1008" % bid):
        bc.check_log("case", exp, rank, short, payload)
    i, j = next((i, j) for i in range(len(recs)) for j in range(i) if recs[i, 2] != recs[j, 2])
    swapped = recs.copy()
    swapped[i, 2], swapped[j, 2] = recs[j, 2], recs[i, 2]
    with pytest.raises(AssertionError, match=r"len 1009 rank 4: delivery set differs, first at \(bid, origin, parent\) \(%d, "
                       % min(int(recs[i, 3]), int(recs[j, 3]))):
        bc.check_log("case", exp, rank, swapped, payload)
    with pytest.raises(AssertionError, match=r"len 1009 rank 4: delivery set differs"):
        bc.check_log("case", exp, rank, recs[1:], payload)
    with pytest.raises(AssertionError, match=r"len 1009 rank 4: delivery set differs"):
        bc.check_log("case", exp, rank, np.concatenate([recs, recs[:1]]), payload)
    st = {"error": np.zeros(n, dtype=np.uint64), "error_aux": np.zeros(n, dtype=np.uint64),
          "bcast_delivered": exp.count.astype(np.uint64), "bcast_sum": exp.sum.copy()}
    bc.check_stats("case", exp, st)
    st["bcast_sum"][2] += np.uint64(1)
    with pytest.raises(AssertionError, match=r"checksum differs at ranks"):
        bc.check_stats("case", exp, st)

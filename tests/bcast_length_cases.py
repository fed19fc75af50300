"""The bcast-length cases of tests/test_gpu_bcast_lengths.py -- TEST INFRASTRUCTURE ONLY.

One table, read by the GPU tests (which run each case) and by tests/test_bcast_lengths_oracle.py (which checks on the
CPU, with the oracle and rlo.layout_plan alone, that every case's inputs meet their conditions, that its world has the
layout it names and that its launches pick the kernel it names: a bad seed or a changed plan fails there).

A bcast of `len` payload bytes occupies 1 + ceil(len / 16) slot chunks (the 16-byte header and the payload).  The
lengths sit on both sides of what changes with the chunk count:
   0              header only
   1, 15, 16, 17  one payload chunk, two from 17; a partial last chunk (zero padded in the checksum)
   64 / 65        5 / 6 chunks: what a 64-B world and every large slot stage (nsmall = 5)
   112 / 113      8 / 9 chunks: the most a doorbell carries (kBellChunks); the 8-wave kernel's largest slot
   368 / 369      24 / 25 chunks: the most a medium slot holds whole on the small copy path
   1008 / 1009    64 / 65 chunks: the most the hop kernel takes (plan_hop)
   1024 / 1025    1 / 2 one-KiB units of the large path
   2048 / 2049    2 / 3 units (kPair)
   4096 / 4097    one full group of 4 units / two groups (kSubMax)
   32767 / 32768  what the send-storm tests reach
   65519 / 65520  the last partial chunk and the largest slot slot_config admits

Three carriers take a bcast of any of these lengths: the latency program ("lat": the hop kernel up to 1008 B where the
launch allows it, else the progress kernel), the generated storm ("storm": the progress kernel) and the host service
("host": HostWorld.bcast, the drop-in's path).  The comparison helpers the GPU tests share are at the end.
"""
import ctypes
import os

import numpy as np

import pyoracle as orc

L = (0, 1, 15, 16, 17, 64, 65, 112, 113, 368, 369, 1008, 1009, 1024, 1025, 2048, 2049, 4096, 4097, 32767, 32768,
     65519, 65520)
# boundary pairs (ln, ln + 1): the chunk count, the kernel or the copy path changes between the two
PAIRS = tuple((a, a + 1) for a in (0, 15, 16, 64, 112, 368, 1008, 1024, 2048, 4096, 32767, 65519))


def chunks(ln):
    """slot chunks of a bcast of ln payload bytes"""
    return 1 + (ln + 15) // 16


def lens_for(max_payload):
    """the table's lengths that fit the slot, and the slot's own last two"""
    return tuple(sorted({x for x in L if x <= max_payload} | {max_payload - 1, max_payload}))


# rlo_device.hpp Mode bits and the progress kernel's program masks (as tests/test_kernel_pick.py names them)
STORM, LAT, IAR, HOST, LL, XCD1 = 1, 2, 4, 128, 16384, 524288
ALL, P_LAT, P_STORM, P_HOST = 0xFFFFFFFF, 0xFFFFFF7A, 0xFFFFFF79, 0xFFFFFFFC
HOP, PROGRESS = 1, 0  # rlo_world_info_t.last_kernel


class Case:
    def __init__(self, cid, carrier, n, lens, kernel, inst, seed, k, waves, nsmall, pull, ll_ok=1, pull_env=None,
                 bounds=None, sys_scope=0, prof=False, windows=(64,), launches=1, per_cu=1, may_skip=False, **world):
        """carrier: "lat" / "storm" / "host"; lens: one launch each (host: all mixed in one run); kernel: the
        last_kernel expected (1: the hop kernel); inst: the instantiation rlo_kernel_pick names for the case's mode
        bits -- (W, BULK, LL, PH, PM) of the progress kernel, (PH, SYS, LOC, SEND, 0) of the hop kernel; seed, k: of the
        program (k: rounds of the latency program, bcasts of the storm; unused by host); waves / nsmall / pull /
        ll_ok / per_cu (rank-workgroups per CU): the world's layout; pull_env: RLO_PULL while the world is created;
        bounds: the part bounds of a two-part world in one process (sys_scope 1: every part sees its peer "on another
        GPU"); prof: program_latency(prof=True); windows: the storm windows run; launches: per length (the first is
        compared whole, every one by counts and checksums); may_skip: RLO_E_OCCUPANCY at creation or launch skips"""
        self.id, self.carrier, self.n, self.lens, self.kernel, self.inst = cid, carrier, n, tuple(lens), kernel, tuple(inst)
        self.seed, self.k, self.waves, self.nsmall, self.pull, self.ll_ok = seed, k, waves, nsmall, pull, ll_ok
        self.pull_env, self.bounds, self.sys_scope, self.prof, self.windows = pull_env, bounds, sys_scope, prof, windows
        self.launches, self.per_cu, self.may_skip, self.world = launches, per_cu, may_skip, world
        self.max_payload = world["max_payload"]
        self.bulk_max = world.get("bulk_max", 0)
        assert carrier in ("lat", "storm", "host") and self.lens == tuple(sorted(set(self.lens)))
        assert all(x <= (self.bulk_max or self.max_payload) for x in self.lens), cid
        assert carrier != "lat" or k <= 1016  # (the latency program's log has 1024 records)

    def mode(self):
        """the mode bits that pick the kernel (rlo_world.cpp: the storm never asks for doorbells; the latency program
        does where the world has them)"""
        if self.carrier == "storm":
            return STORM
        if self.carrier == "host":
            return HOST | IAR | (LL if self.ll_ok else 0)
        return LAT | (LL if self.ll_ok else 0) | (XCD1 if self.world.get("one_xcd") else 0)

    def variant(self):
        return 5 if self.bulk_max else self.waves

    def plan_kw(self):
        """rlo.layout_plan's arguments (one_xcd changes no layout: the same plan)"""
        return {k: v for k, v in self.world.items() if k != "one_xcd"}


def _hop(cid, n, maxp, lens, seed, k, waves=4, nsmall=5, pull=1, inst=(0, 0, 0, 0, 0), **kw):
    return Case(cid, "lat", n, lens, HOP, inst, seed, k, waves, nsmall, pull, max_payload=maxp, **kw)


def _big(cid, n, maxp, lens, seed, k, pull, pull_env=None, inst=(4, 0, 1, 0, ALL), **kw):
    return Case(cid, "lat", n, lens, PROGRESS, inst, seed, k, 4, 5, pull, pull_env=pull_env, max_payload=maxp, **kw)


def _storm(cid, n, maxp, lens, seed, k, waves, nsmall, pull, pull_env=None, **kw):
    inst = (8, 0, 0, 0, P_STORM) if waves == 8 else (4, 0, 0, 0, ALL)
    return Case(cid, "storm", n, lens, PROGRESS, inst, seed, k, waves, nsmall, pull, pull_env=pull_env, max_payload=maxp, **kw)


BIG = (1009, 1024, 1025, 2048, 2049, 4095, 4096)
MAX_LAT = (4097, 32767, 32768, 65519, 65520)
MAX_STORM = (4097, 8192, 32767, 32768, 65519, 65520)
# seeds: the first from 1 on that meets input_conditions() for the case's (n, k) -- found on the CPU, pinned by
# tests/test_bcast_lengths_oracle.py.  n <= 17 run 64 bcasts a launch; 32 ranks 128 and 64 ranks 256, since with
# random originators 64 bcasts cannot come from 64 different ranks
CASES = [
    # ---- the latency program on the hop kernel: messages of at most 64 chunks in worlds with doorbells
    _hop("lat-hop-112", 8, 112, lens_for(112), 1, 64, waves=8, nsmall=8, pull=0),
    _hop("lat-hop-1008", 8, 1008, lens_for(1008), 1, 64),
    _hop("lat-hop-1008-n13", 13, 1008, (113, 369, 1007, 1008), 46, 64),
    _hop("lat-hop-1008-n64", 64, 1008, (113, 369, 1007, 1008), 227, 256),
    _hop("lat-hop-pend-hbm", 8, 1008, (113, 1008), 1, 64, inst=(1, 0, 0, 0, 0), pend_hbm=True),
    _hop("lat-hop-one-xcd-n8", 8, 1008, (113, 368, 369, 1008), 1, 64, inst=(0, 0, 1, 0, 0), launches=3, one_xcd=True),
    _hop("lat-hop-one-xcd-n32", 32, 1008, (113, 368, 369, 1008), 1, 128, inst=(0, 0, 1, 0, 0), launches=3, one_xcd=True),
    _hop("lat-hop-parts", 8, 1008, (113, 1008), 1, 64, inst=(0, 1, 0, 0, 0), bounds=[0, 3, 8], sys_scope=1),
    _hop("lat-medium", 8, 368, (113, 367, 368), 1, 64, nsmall=24, pull=0),
    # ---- the latency program on the progress kernel
    # 4 waves with doorbells: the large-message rounds, one relay slot in flight, released and reused next round
    _big("lat-big-pull", 8, 4096, BIG, 1, 64, 1),
    _big("lat-big-push", 8, 4096, BIG, 1, 64, 0, pull_env="0"),
    _big("lat-big-n13", 13, 4096, (1009, 4096), 46, 64, 1),
    _big("lat-max-pull", 4, 65520, MAX_LAT, 1, 48, 1, ring_slots=16),
    _big("lat-max-push", 4, 65520, MAX_LAT, 1, 48, 0, pull_env="0", ring_slots=16),
    _big("lat-big-parts", 8, 4096, (1009, 4096), 1, 64, 1, bounds=[0, 3, 8], sys_scope=1),
    # more than 256 ranks: two rank-workgroups per CU, no doorbells (the non-LL instantiation)
    Case("lat-no-bells-64", "lat", 300, (64,), PROGRESS, (4, 0, 0, 0, ALL), 1, 64, 4, 5, 0, ll_ok=0, per_cu=2, may_skip=True,
         max_payload=64),
    Case("lat-no-bells-1008", "lat", 300, (65, 1008), PROGRESS, (4, 0, 0, 0, ALL), 1, 64, 4, 5, 1, ll_ok=0, per_cu=2,
         may_skip=True, max_payload=1008),
    # a bulk world never takes the hop kernel: ring lengths run (4, BULK, LL, kPmLat); 4097 is the first bulk length
    Case("lat-bulk-ring", "lat", 8, (0, 64, 65, 113, 1009, 4096, 4097), PROGRESS, (4, 1, 1, 0, P_LAT), 1, 64, 4, 5, 0,
         max_payload=4096, bulk_max=1 << 20),
    # the phase profile keeps the progress kernel (plan_hop declines MODE_PROF): 8 waves under the latency program
    Case("lat-prof-8w", "lat", 8, (0, 17, 112), PROGRESS, (8, 0, 1, 0, P_LAT), 1, 64, 8, 8, 0, prof=True, max_payload=112),
    # ---- the generated storm
    _storm("storm-8w-n8", 8, 112, lens_for(112), 1, 64, 8, 8, 0, windows=(64, 1)),
    _storm("storm-8w-n64", 64, 112, lens_for(112), 227, 256, 8, 8, 0, windows=(64, 1)),
    _storm("storm-8w-64", 256, 64, (0, 1, 15, 16, 17, 63, 64), 1, 768, 8, 5, 0),
    _storm("storm-medium-n8", 8, 368, lens_for(368), 1, 64, 4, 24, 0),
    _storm("storm-medium-n17", 17, 368, lens_for(368), 20, 64, 4, 24, 0),
    _storm("storm-large-pull-n8", 8, 4096, lens_for(4096), 1, 64, 4, 5, 1, pull_env="1"),
    _storm("storm-large-pull-n13", 13, 4096, lens_for(4096), 46, 64, 4, 5, 1, pull_env="1"),
    _storm("storm-large-push-n8", 8, 4096, lens_for(4096), 1, 64, 4, 5, 0, pull_env="0"),
    _storm("storm-large-push-n13", 13, 4096, lens_for(4096), 46, 64, 4, 5, 0, pull_env="0"),
    _storm("storm-max-pull", 4, 65520, MAX_STORM, 1, 48, 4, 5, 1, pull_env="1", ring_slots=16),
    _storm("storm-max-push", 4, 65520, MAX_STORM, 1, 48, 4, 5, 0, pull_env="0", ring_slots=16),
    _storm("storm-small-stage", 300, 4096, (65, 1025, 4096), 1, 320, 4, 5, 1, ll_ok=0, per_cu=2, may_skip=True),
    _storm("storm-parts", 8, 4096, (65, 1025, 4096), 1, 64, 4, 5, 1, bounds=[0, 3, 8], sys_scope=1),
    # ---- the host service: every rank broadcasts every length that fits, mixed in one run
    Case("host-112", "host", 8, lens_for(112), PROGRESS, (8, 0, 1, 0, P_HOST), 1, 0, 8, 8, 0, max_payload=112),
    Case("host-368", "host", 8, lens_for(368), PROGRESS, (4, 0, 1, 0, P_HOST), 1, 0, 4, 24, 0, max_payload=368),
    Case("host-4096", "host", 8, lens_for(4096), PROGRESS, (4, 0, 1, 0, P_HOST), 1, 0, 4, 5, 1, max_payload=4096),
    Case("host-32784", "host", 4, lens_for(32784), PROGRESS, (4, 0, 1, 0, P_HOST), 1, 0, 4, 5, 1, max_payload=32784),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def ids(carrier, parts=False):
    return [c.id for c in CASES if c.carrier == carrier and (c.bounds is not None) == parts]


# ------------------------------------------------------------------------------------------------ the inputs
def origins(n, seed, k):
    return np.array([orc.origin_of(seed, b, n) for b in range(k)], dtype=np.int64)


def split(par, origin):
    """(leaves, forwarding ranks) of one bcast's tree: par[r] is the rank r received it from"""
    fwd = {int(p) for r, p in enumerate(par) if r != origin} - {int(origin)}
    return {r for r in range(len(par)) if r != origin and r not in fwd}, fwd


def roles(n):
    """what the trees allow: the ranks that are a leaf of some origin's tree, and those that forward in some"""
    leaf, fwd = set(), set()
    for o in range(n):
        lf, fw = split(orc.tree(n, o)[0], o)
        leaf |= lf
        fwd |= fw
    return leaf, fwd


def input_conditions(n, seed, k, parent):
    """every rank originates at least once, and receives at least once as a leaf and at least once as a forwarding
    rank (wherever some origin's tree gives it that role at all: orc.tree); parent: orc.storm(..., want_parent=True)"""
    org = origins(n, seed, k)
    assert set(org.tolist()) == set(range(n)), ("ranks that never originate", sorted(set(range(n)) - set(org.tolist())))
    leaf, fwd = set(), set()
    for b in range(k):
        lf, fw = split(parent[b], org[b])
        leaf |= lf
        fwd |= fw
    can_leaf, can_fwd = roles(n)
    assert leaf == can_leaf, ("ranks never a leaf", sorted(can_leaf - leaf))
    assert fwd == can_fwd, ("ranks never forwarding", sorted(can_fwd - fwd))
    return len(can_leaf), len(can_fwd)


def host_plan(c):
    """the host case's bcasts in posting order: (origin, seq, length), every rank every length, shuffled by the seed"""
    rng = np.random.default_rng(c.seed)
    plan = [(o, i * c.n + o, ln) for i, ln in enumerate(c.lens) for o in range(c.n)]
    return [plan[i] for i in rng.permutation(len(plan))]


# ------------------------------------------------------------------------------------------------ comparisons
LOG_DELIVER, TAG_BCAST, TAG_BULK = 1, 0, 10  # rlo_device.hpp


class Expected:
    """what one launch of (n, seed, k, ln) delivers, from the oracle alone; computed once per (case, length) and
    never changed (the fields are read-only arrays)"""

    def __init__(self, n, seed, k, ln, bulk=False):
        ref = orc.storm(n, seed, k, ln, want_parent=True)
        self.n, self.seed, self.k, self.ln = n, seed, k, ln
        self.count, self.sum, self.parent = ref["count"], ref["sum"], ref["parent"].astype(np.int64)
        self.origin = origins(n, seed, k)
        self.pad = (ln + 15) // 16 * 16
        self.bulk = bulk
        if bulk:  # the receiver's copy by its checksum (tests/test_gpu_bulk.py::_check)
            self.checksum = np.array([orc.msg_checksum(int(self.origin[b]), b, 0, orc.payload(int(self.origin[b]), b, ln))
                                      for b in range(k)], dtype=np.uint64)
        else:  # the payload and its zero padding up to the chunk's end
            self.bytes = np.zeros((k, max(self.pad, 1)), dtype=np.uint8)
            for b in range(k):
                self.bytes[b, :ln] = np.frombuffer(orc.payload(int(self.origin[b]), b, ln), dtype=np.uint8)
        for a in (self.count, self.sum, self.parent, self.origin):
            a.setflags(write=False)


def log_arrays(w, rank, cap, payload=True):
    """rlo_log as arrays: (records [count][8] uint32 -- kind | tag << 8, origin, from, id, len, vote, aux, payload_idx --
    and the payload rows [cap][max_payload], None without `payload`); what World.log returns, without a tuple per record"""
    from rlo import _lib as lib

    stride = w.info["slot_stride"] - 16
    recs = np.zeros((cap, 8), dtype=np.uint32)
    buf = np.zeros((cap, stride), dtype=np.uint8) if payload else None
    cnt = lib.check(w.lib.rlo_log(w.h, rank, recs.ctypes.data_as(ctypes.POINTER(lib.LogRec)), cap,
                                  buf.ctypes.data if payload else None, stride), "rlo_log")
    return recs[:cnt], buf


def rows_arrays(rows):
    """World.log's tuples (rlo.sharded returns them) as log_arrays' records"""
    out = np.zeros((len(rows), 8), dtype=np.uint32)
    for i, (kind, tag, origin, frm, bid, ln, vote, aux, pidx) in enumerate(rows):
        out[i] = (kind | tag << 8, origin & 0xFFFFFFFF, frm & 0xFFFFFFFF, bid, ln, vote & 0xFFFFFFFF, aux, pidx)
    return out


def check_stats(cid, exp, st):
    """per-rank delivery counts and checksums of one launch"""
    what = (cid, "len", exp.ln)
    assert (st["error"] == 0).all(), what + ("error", st["error"], st["error_aux"])
    got = st["bcast_delivered"].astype(np.int64)
    bad = np.nonzero(got != exp.count)[0]
    assert bad.size == 0, what + ("rank", int(bad[0]) if bad.size else -1, "delivered", got, exp.count)
    bad = np.nonzero(st["bcast_sum"] != exp.sum)[0]
    assert bad.size == 0, what + ("checksum differs at ranks", bad[:8].tolist())


def check_round_ticks(cid, ln, rt, rounds):
    """world rank 0 saw (nearly) every round complete, on its own clock, in order (tests/test_gpu_engine.py
    ::test_latency_program, tests/test_gpu_sharded.py::_check_lat)"""
    rt = np.asarray(rt).astype(np.int64)
    seen = rt[rt > 0]
    assert len(seen) >= rounds - 1 and (np.diff(seen) >= 0).all(), (cid, "len", ln, len(seen), rounds)


def check_log(cid, exp, rank, recs, payload):
    """one rank's log of one launch: the delivery set (bid, origin, parent), every record's length, and every
    delivered payload byte for byte with its zero padding up to the chunk's end (a bulk message: its checksum)"""
    n, k, ln = exp.n, exp.k, exp.ln
    recs = recs[(recs[:, 0] & 0xff) == LOG_DELIVER].astype(np.int64)
    recs = recs[np.argsort(recs[:, 3], kind="stable")]
    bids = np.nonzero(exp.origin != rank)[0]
    want = np.stack([bids, exp.origin[bids], exp.parent[bids, rank]], axis=1)
    got = recs[:, (3, 1, 2)]
    if got.shape != want.shape or not np.array_equal(got, want):
        g, w_ = {tuple(x) for x in got.tolist()}, {tuple(x) for x in want.tolist()}
        first = sorted(g ^ w_)[0] if g ^ w_ else None  # (a set that is equal: a delivery twice)
        raise AssertionError("%s len %d rank %d: delivery set differs, first at (bid, origin, parent) %s: got %s, want %s; "
                             "%d records for %d deliveries" %
                             (cid, ln, rank, first, sorted(x for x in g if first and x[0] == first[0]),
                              sorted(x for x in w_ if first and x[0] == first[0]), len(got), len(want)))
    bad = np.nonzero(recs[:, 4] != ln)[0]
    assert bad.size == 0, "%s len %d rank %d bid %d: the record's len is %d" % (
        cid, ln, rank, recs[bad[0], 3] if bad.size else -1, recs[bad[0], 4] if bad.size else -1)
    tag = (recs[:, 0] >> 8) & 0xff
    if exp.bulk:
        assert (tag == TAG_BULK).all(), (cid, ln, rank, tag)
        cs = recs[:, 6].astype(np.uint64) | (recs[:, 7].astype(np.uint64) << np.uint64(32))
        bad = np.nonzero(cs != exp.checksum[recs[:, 3]])[0]
        assert bad.size == 0, "%s len %d rank %d bid %d: the bulk copy's checksum differs" % (
            cid, ln, rank, recs[bad[0], 3] if bad.size else -1)
        return
    assert (tag == TAG_BCAST).all(), (cid, ln, rank, tag)
    if exp.pad == 0:
        return
    got_b = payload[recs[:, 7], :exp.pad]
    want_b = exp.bytes[recs[:, 3], :exp.pad]
    if not np.array_equal(got_b, want_b):
        i, j = (int(x[0]) for x in np.nonzero(got_b != want_b))
        raise AssertionError("%s len %d rank %d bid %d origin %d parent %d: byte %d is 0x%02x, expected 0x%02x%s (%d bytes differ)" %
                             (cid, ln, rank, recs[i, 3], recs[i, 1], recs[i, 2], j, got_b[i, j], want_b[i, j],
                              " (padding)" if j >= ln else "", int((got_b[i] != want_b[i]).sum())))


def create(rlo, factory, pull_env=None):
    """factory() with RLO_PULL set as the case asks (read at creation, tests/test_gpu_engine.py::test_storm_large_groups)"""
    if pull_env is None:
        return factory()
    os.environ["RLO_PULL"] = pull_env
    try:
        return factory()
    finally:
        del os.environ["RLO_PULL"]

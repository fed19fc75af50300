"""GPU tests of the bulk send program (rlo_program_send_bulk): closed-loop rootless bcasts of large caller-owned device
buffers -- the movers read every message from a caller-owned source buffer and write every receiver's copy into a
caller-owned destination buffer -- on the direct and the chunked plan, in one part, two parts and two processes, and
through World.bcast_tensor of a world with bulk messages.

Expected values never come from the engine: bytes are this file's seeded NumPy source, tree parents pyoracle.tree,
checksums pyoracle.msg_checksum(origin, i, 0, bytes) summed over what a rank must receive.  dst is pre-filled with 0xA5
and compared whole, so a stray store anywhere fails."""
import ctypes

import numpy as np
import pytest

import pyoracle as orc
from send_cases import FILL, MASK64, TAG_BCAST, rlo  # noqa: F401  (rlo: the fixture)

pytestmark = pytest.mark.gpu
TAG_BULK = 10
KIB, MIB = 1 << 10, 1 << 20


def _source(k, stride, seed):
    """k x stride seeded source bytes (cheap for large strides: a random 64-KiB block tiled, each row rolled by a
    different odd amount and stamped with its index, so rows, tiles and granules all differ from their neighbours)"""
    rng = np.random.default_rng(seed)
    block = rng.integers(0, 256, 64 * KIB + 24, dtype=np.uint8)  # (no power of two: tiles of a message differ)
    src = np.empty((k, stride), dtype=np.uint8)
    for i in range(k):
        src[i] = np.resize(np.roll(block, 2 * i + 1), stride)
        src[i, :8] = np.frombuffer(np.uint64(seed * 1000003 + i).tobytes(), dtype=np.uint8)
    return src


def _sums(n, origins, lens, src):
    cs = [orc.msg_checksum(int(origins[i]), i, TAG_BCAST, src[i, :int(lens[i])].tobytes()) for i in range(len(origins))]
    total = sum(cs)
    own = [0] * n
    for i, o in enumerate(origins):
        own[int(o)] += cs[i]
    return cs, np.array([(total - own[r]) & MASK64 for r in range(n)], dtype=np.uint64)


def _want_np(ranks, origins, lens, src):
    """the destination bytes [rank][message][stride] of `ranks` after a correct run (NumPy)"""
    k, stride = src.shape
    want = np.full((len(ranks), k, stride), FILL, dtype=np.uint8)
    for i in range(k):
        ln = int(lens[i])
        want[:, i, :ln] = src[i, :ln]
        want[:, i, ln:(ln + 15) // 16 * 16] = 0
        for j, r in enumerate(ranks):
            if r == origins[i]:
                want[j, i] = FILL  # the origin's own place is not written
    return want


def _check_stats(st, n, origins, lens, src):
    origins = np.asarray(origins)
    own = np.bincount(origins, minlength=n)
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    assert np.array_equal(st["bcast_delivered"].astype(np.int64), len(origins) - own)
    assert np.array_equal(st["originated"].astype(np.int64), own)
    assert np.array_equal(st["bcast_sum"], _sums(n, origins, lens, src)[1])


def _launch(w, origins, lens, src, **kw):
    """one launch of a one-part world on device buffers made here; the whole of dst is compared on the device with
    what the NumPy source says (built there from the uploaded source bytes); returns the stats"""
    import torch

    n = w.n
    k, stride = src.shape
    s = torch.from_numpy(src).cuda()
    d = torch.full((n, k, stride), FILL, dtype=torch.uint8, device="cuda")
    want = torch.full((n, k, stride), FILL, dtype=torch.uint8, device="cuda")
    for i in range(k):
        ln = int(lens[i])
        want[:, i, :ln] = s[i, :ln]
        want[:, i, ln:(ln + 15) // 16 * 16] = 0
        want[int(origins[i]), i] = FILL
    torch.cuda.synchronize()
    w.program_send_bulk(origins, s, d, stride, lens=lens, **kw)
    w.run()
    assert w.info_now()["last_kernel"] == 0  # the progress kernel, never the hop kernel
    st = w.stats()
    _check_stats(st, n, origins, lens, src)
    if not torch.equal(d, want):
        r, i, b = (int(x) for x in torch.nonzero(d != want)[0])
        raise AssertionError("rank %d message %d (origin %d, len %d) byte %d: got 0x%02x, want 0x%02x; %d bytes differ" %
                             (r, i, origins[i], lens[i], b, int(d[r, i, b]), int(want[r, i, b]), int((d != want).sum())))
    return st


# ---- the direct plan (one part).  The 1-KiB stripe rounding, the 16-KiB tile, the 64-KiB delivery tile, the switch to
# 64-KiB tiles at 8 MiB; at most two messages of >= 1 MiB per case
BULK_MAX = 8 * MIB + 16
SMALL = [1, 15, 16, 17, 1023, 1024, 1025, 16384, 16385, 65552]
DIRECT = {
    "small": (SMALL + SMALL[::-1][:6], 65552 + 64),
    "big_a": ([MIB + 16, 17, 8 * MIB - 1, 1025], 8 * MIB + 64),
    "big_b": ([8 * MIB, 1, 65552, MIB + 16], 8 * MIB + 64),
}
_worlds = {}


@pytest.fixture(scope="module")
def direct_world(rlo):
    def get(n):
        if n not in _worlds:
            _worlds[n] = rlo.World(n, max_payload=64, bulk_max=BULK_MAX)
        return _worlds[n]

    yield get
    for w in _worlds.values():
        w.close()
    _worlds.clear()


@pytest.mark.parametrize("case", sorted(DIRECT))
@pytest.mark.parametrize("n", [2, 3, 8])
def test_direct_plan_exact_bytes(rlo, direct_world, n, case):
    lens, stride = DIRECT[case]
    k = len(lens)
    assert stride > (max(lens) + 15) // 16 * 16 and sum(ln >= MIB for ln in lens) <= 2
    rng = np.random.default_rng(100 * n + k)
    origins = rng.integers(0, n, k).astype(np.int32)
    origins[:2] = [n - 1, 0]  # mixed origins, the first and the last rank among them
    w = direct_world(n)
    assert w.info["bulk_max"] == BULK_MAX
    _launch(w, origins, lens, _source(k, stride, 7 * n + k))


@pytest.mark.parametrize("slots", [2, 1])
def test_slot_reuse(rlo, slots):
    """one origin sends 5 messages in a row through `slots` heap slots: a slot is reused only after every receiver
    released it"""
    n, lens = 4, [5000, 70000, 5000, 70000, 70000]
    with rlo.World(n, max_payload=64, bulk_max=70000, bulk_slots=slots) as w:
        assert w.info["bulk_slots"] == slots
        _launch(w, [2] * 5, lens, _source(5, 70000 + 32, 31 + slots))


# ---- the chunked plan (scatter + all-gather, what a world across GPUs runs), two parts with their own buffers
CH_LENS = [5000, 3 * MIB + 123, 16 * MIB + 48]


def _check_parts(st, n, origins, lens, src):
    _check_stats(st, n, origins, lens, src)
    got, want = st["dst"], _want_np(list(range(n)), origins, lens, src)
    if not np.array_equal(got, want):
        r, i, b = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("rank %d message %d (origin %d, len %d) byte %d: got 0x%02x, want 0x%02x" %
                             (r, i, origins[i], lens[i], b, got[r, i, b], want[r, i, b]))


@pytest.mark.parametrize("n,bounds", [(4, [0, 1, 4]), (8, [0, 3, 8])], ids=["4", "8"])
def test_chunked_plan_two_parts(rlo, n, bounds):
    from rlo import sharded

    stride = 16 * MIB + 64
    assert rlo.bulk_plan(n, CH_LENS[2], True)["nchunks"] == 2
    origins = np.array([n - 1, 0, bounds[1]], dtype=np.int32)  # both parts originate
    src = _source(3, stride, 50 + n)
    spec = {"kind": "send_bulk", "origins": origins, "lens": CH_LENS, "stride": stride, "src": src}
    (st, _, _), rcs = sharded.run_inprocess(n, bounds, spec, max_payload=64, bulk_max=CH_LENS[2], movers=16, chunked=True)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == 0).all()
    _check_parts(st, n, origins, CH_LENS, src)


def test_two_processes(rlo):
    """two part processes on one GPU (hipIpc mappings, system-scope stores), the chunked plan"""
    from rlo import sharded

    n, bounds, lens = 4, [0, 2, 4], [5000, 3 * MIB + 123, 17, MIB]
    stride = 3 * MIB + 256
    origins = np.array([3, 0, 2, 1], dtype=np.int32)
    src = _source(4, stride, 77)
    spec = {"kind": "send_bulk", "origins": origins, "lens": lens, "stride": stride, "src": src}
    (st, _, _), rcs = sharded.run_processes(n, bounds, spec, max_payload=64, bulk_max=4 * MIB, movers=8, uncached=True,
                                            chunked=True, timeout=60)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_sys_scope"] == 1).all() and (st["part_last_kernel"] == 0).all()
    _check_parts(st, n, origins, lens, src)


def test_three_launches_then_a_latency_program(rlo):
    """different origins, lengths and buffers each time, then a latency program of a bulk length in the same world,
    which must still verify: no stale flag, release count or job-ring word survives a launch"""
    n, ln, rounds, seed = 8, 300000, 4, 5
    with rlo.World(n, max_payload=64, bulk_max=MIB) as w:
        for j, lens in enumerate(([MIB, 17, 70000], [1, 65552, 5000, 16385, MIB - 1], [200000, 200000])):
            rng = np.random.default_rng(900 + j)
            _launch(w, rng.integers(0, n, len(lens)).astype(np.int32), lens, _source(len(lens), MIB + 16 * (j + 1), 60 + j))
        w.program_latency(rounds, ln, seed=seed)
        w.run()
        st = w.stats()
    org = [orc.origin_of(seed, i, n) for i in range(rounds)]
    want = np.zeros(n, dtype=np.uint64)
    for i, o in enumerate(org):
        cs = np.uint64(orc.msg_checksum(o, i, TAG_BCAST, orc.payload(o, i, ln)))
        for r in range(n):
            if r != o:
                want[r] += cs
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    assert [int(x) for x in st["bcast_delivered"]] == [sum(o != r for o in org) for r in range(n)]
    assert np.array_equal(st["bcast_sum"], want)


def test_log_and_latencies(rlo):
    n, lens = 8, [5000, 70000, 1, 16384, 300000, 17]
    k = len(lens)
    origins = np.array([5, 0, 7, 3, 5, 2], dtype=np.int32)
    src = _source(k, 300000 + 16, 11)
    cs, _ = _sums(n, origins, lens, src)
    parent = {o: orc.tree(n, o)[0] for o in range(n)}
    with rlo.World(n, max_payload=64, bulk_max=MIB) as w:
        _launch(w, origins, lens, src, log=True, log_cap=k)
        for r in range(n):
            rows = w.log(r, cap=k)
            assert [row[4] for row in rows] == [i for i in range(k) if origins[i] != r]  # every message, in order
            for kind, tag, origin, frm, ident, ln, _vote, aux, pidx in rows:
                assert (kind, tag) == (1, TAG_BULK)
                assert origin == origins[ident] and ln == lens[ident]
                assert frm == parent[origin][r], (r, origin, ident, frm)
                assert (aux | (pidx << 32)) == cs[ident], (r, ident)
        lat = w.latencies_ticks()
        print("bulk send, %d ranks: completion ticks %s" % (n, lat))
        assert len(lat) == k
        assert (lat > 0).all() and (lat < 100000000).all(), lat  # positive and below 1 s per round


def _storm_runs_clean(ws, n):
    from rlo import _lib as L

    k, ln, seed = 32, 48, 3
    for w in ws:
        w.program_storm(k, ln, seed=seed)
    for w in ws:
        w.reset()
    streams = []
    try:
        for w in ws:
            s = ctypes.c_void_p()
            L.check(L.load().rlo_stream_create(-1, ctypes.byref(s)), "rlo_stream_create")
            streams.append(s)
            w.launch(stream=s, no_reset=True)
        for w in ws:
            w.wait()
        exp = orc.storm_expected(n, seed, k, ln)
        got = np.concatenate([w.stats()["bcast_sum"] for w in ws])
        assert np.array_equal(got, exp["sum"])
    finally:
        for s in streams:
            L.load().rlo_stream_destroy(s)


def test_refusals(rlo):
    import torch

    n = 4
    s = torch.zeros(8193 * 16, dtype=torch.uint8, device="cuda")
    d = torch.full((n * 8193 * 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rlo.World(n, max_payload=64) as w:  # a world without bulk messages
        with pytest.raises(rlo.RloError):
            w.program_send_bulk([0, 1], s, d, 64)
        _storm_runs_clean([w], n)
    with rlo.World(n, max_payload=64, bulk_max=MIB) as w:  # arguments outside the ranges, in a world that has them
        for kw in ({"lens": [0, 1]}, {"lens": [1, 65]}, {"rank_stride": 16}):
            with pytest.raises(rlo.RloError):
                w.program_send_bulk([0, 1], s, d, 64, **kw)
        with pytest.raises(rlo.RloError):  # len > bulk_max (extents as numbers: refused before anything is read)
            w.program_send_bulk([0, 1], (s.data_ptr(), 1 << 40), (d.data_ptr(), 1 << 40), 2 * MIB, lens=[1, MIB + 1])
        with pytest.raises(ValueError):  # the extents are checked before the library sees them
            w.program_send_bulk([0, 1], s[:64], d, 64)
        _storm_runs_clean([w], n)
    bounds = [0, 2, 4]
    ws = [rlo.World.part(n, 2, p, part_begin=bounds, max_payload=64, bulk_max=MIB, movers=8) for p in range(2)]
    try:
        blobs = [w.export() for w in ws]
        for w in ws:
            w.connect(blobs)
        for w in ws:
            with pytest.raises(rlo.RloError):  # k > 8192 in a world of several parts
                w.program_send_bulk([0] * 8193, s, d, 16)
            w.program_send_bulk([0] * 8192, s, d, 16)  # (the limit itself is taken)
        _storm_runs_clean(ws, n)
    finally:
        for w in ws:
            w.close()
    torch.cuda.synchronize()
    assert bool((d == FILL).all())  # no refused program wrote anything


# ---- World.bcast_tensor in a world with bulk messages
BT_MAX = MIB


@pytest.fixture(scope="module")
def bt_world(rlo):
    with rlo.World(8, bulk_max=BT_MAX) as w:
        yield w


def _bt(w, t, origin=5):
    import torch

    before = t.clone()
    out = w.bcast_tensor(origin, t)
    assert out.shape == (w.n,) + tuple(t.shape) and out.dtype == t.dtype
    for r in range(w.n):
        assert torch.equal(out[r], before), r
    assert torch.equal(t, before)  # the input is unchanged
    if t.numel():
        assert w.info_now()["last_kernel"] == 0
        want = -(-t.numel() * t.element_size() // (BT_MAX // 16 * 16))
        assert int(w.stats()["originated"].sum()) == want  # messages of at most bulk_max, not of 1008 bytes


@pytest.mark.parametrize("dtype,nbytes", [("uint8", b) for b in (0, 1, 1000, BT_MAX, BT_MAX + 16, 3 * BT_MAX + 5)] +
                         [(dt, b) for dt in ("float16", "float32", "int64") for b in (0, 1000, BT_MAX, BT_MAX + 16)])
def test_bcast_tensor_bulk_world(rlo, bt_world, dtype, nbytes):
    """the tensor is produced by torch kernels on the current stream right before the call, no synchronise"""
    import torch

    dt = getattr(torch, dtype)
    numel = nbytes // torch.empty(0, dtype=dt).element_size()
    base = torch.arange(numel, device="cuda", dtype=torch.int64)
    t = (base * 2654435761 % 251).to(dt) if dt != torch.int64 else base * 2654435761 + 12345
    assert t.numel() * t.element_size() == nbytes
    _bt(bt_world, t)


@pytest.mark.parametrize("offset", [16, 3], ids=["aligned_view", "odd_view"])
def test_bcast_tensor_views(rlo, bt_world, offset):
    import torch

    base = (torch.arange(3 * MIB, device="cuda", dtype=torch.int64) * 40503 % 256).to(torch.uint8)
    for nbytes in (4992, BT_MAX + 32):  # (multiples of 16: the aligned view is the source buffer itself)
        t = base[offset:offset + nbytes]
        assert t.is_contiguous() and t.data_ptr() % 16 == offset % 16
        _bt(bt_world, t, origin=0)
    assert torch.equal(base, (torch.arange(3 * MIB, device="cuda", dtype=torch.int64) * 40503 % 256).to(torch.uint8))

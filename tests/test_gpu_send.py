"""GPU tests of the send program (rlo_program_send): rootless bcasts whose payloads are read from a caller-owned
source buffer in device memory and written, at every receiver, to a caller-owned destination buffer in device
memory -- on the hop kernel, open loop and ordered, in one part and several, and through World.bcast_tensor.

Expected values never come from the engine: payload bytes are this file's seeded NumPy source, tree parents
pyoracle.tree, checksums pyoracle.msg_checksum summed over what a rank must receive, counts k minus the rank's own."""
import functools

import numpy as np
import pytest

from send_cases import FILL, check, check_trees_fifo, forge_bus, gen, latency_runs_clean, rlo  # noqa: F401  (rlo: the fixture)
from send_cases import launch_send as _launch

pytestmark = pytest.mark.gpu
_gen = functools.partial(gen, storm=False)


# 16 / 17 straddle the register out-ring table, 64 / 256 use the LDS table (256: its last size), 300 the computed path
CASES = [(4, 1008, 64), (8, 1008, 128), (13, 112, 104), (16, 1008, 128), (17, 64, 136), (64, 64, 256), (256, 64, 512),
         (300, 16, 600)]


@pytest.mark.parametrize("n,slot,k", CASES, ids=lambda v: str(v))
def test_exact_bytes_open_loop(rlo, n, slot, k):
    origins, lens, src = _gen(n, slot, k, 1000 + n)
    with rlo.World(n, max_payload=slot) as w:
        try:
            st, got = _launch(w, origins, lens, src)
        except rlo.RloError as e:
            if n == 300 and str(e).startswith("rlo_run failed") and "[-1]" in str(e):  # (RLO_E_INVAL from the launch itself)
                pytest.skip("300 rank-waves of the send program are not co-resident on this device: the launch was refused")
            raise
        check(st, got, n, origins, lens, src)


@pytest.mark.parametrize("n", [8, 13, 64])
def test_trees_and_per_origin_fifo(rlo, n):
    slot, k = 64, 12 * n
    origins, lens, src = _gen(n, slot, k, 2000 + n)
    with rlo.World(n, max_payload=slot) as w:
        st, got = _launch(w, origins, lens, src, log=True, log_cap=k)
        check(st, got, n, origins, lens, src)
        check_trees_fifo(w, n, origins, lens)


@pytest.mark.parametrize("pattern", ["rank0", "odd", "all"])
def test_back_pressure_and_ring_wrap(rlo, pattern):
    """the smallest rings a world takes, every origin sending >= 4 x the ring capacity: tails wrap, originations are
    refused and retried.  (The issue asked for ring_slots=8; rlo_world_create refuses rings below 16 slots, as it did
    before this program existed, so the rings here have 16 and every origin sends at least 64.)"""
    n, slot, cap = 8, 64, 16
    with pytest.raises(rlo.RloError):
        rlo.World(n, max_payload=slot, ring_slots=8)
    if pattern == "rank0":
        org = [0] * (8 * cap)
    elif pattern == "odd":
        org = [1 + 2 * (i % 4) for i in range(4 * 4 * cap)]
    else:
        org = [i % n for i in range(n * 64)]
    origins, lens, src = _gen(n, slot, len(org), 3000 + len(org), origins=org)
    assert np.bincount(origins, minlength=n)[np.unique(origins)].min() >= 4 * cap
    with rlo.World(n, max_payload=slot, ring_slots=cap) as w:
        assert w.info["ring_slots"] == cap
        st, got = _launch(w, origins, lens, src)
        check(st, got, n, origins, lens, src)


@pytest.mark.parametrize("n", [8, 64])
def test_ordered(rlo, n):
    slot, k = 64, 64
    origins, lens, src = _gen(n, slot, k, 4000 + n)
    with rlo.World(n, max_payload=slot) as w:
        st, got = _launch(w, origins, lens, src, ordered=True, log=True, log_cap=k)
        check(st, got, n, origins, lens, src)
        for r in range(n):
            ids = [row[4] for row in w.log(r, cap=k)]
            assert ids == sorted(set(ids)) and len(ids) == k - int((origins == r).sum())  # strictly ascending: a total order
        lat = w.latencies_ticks()
        print("ordered send, %d ranks: completion ticks min %d median %d max %d" % (n, lat.min(), np.median(lat), lat.max()))
        assert len(lat) == k
        assert (lat > 0).all() and (lat < 100000).all(), lat  # below 1 ms: no stale origination clock


def test_three_launches_of_one_world(rlo):
    import torch

    n, slot = 8, 112
    with rlo.World(n, max_payload=slot) as w:
        dst = torch.empty(n * 96 * slot, dtype=torch.uint8, device="cuda")
        for j, k in enumerate((40, 96, 24)):  # (the last one into a buffer the second filled: re-filled by _launch)
            origins, lens, src = _gen(n, slot, k, 5000 + j)
            st, got = _launch(w, origins, lens, src, dst=dst, ordered=(j == 1))
            check(st, got, n, origins, lens, src)


@pytest.mark.parametrize("forged", [False, True], ids=["agent", "system"])
@pytest.mark.parametrize("n,bounds", [(8, [0, 3, 8]), (16, [0, 8, 16])], ids=["8", "16"])
def test_parts(rlo, n, bounds, forged):
    """two parts in one process, each with its own src and dst; forged: every part sees its peer "on another GPU", so
    both run the system-scope instantiation"""
    from rlo import sharded

    slot, k = 64, 16 * n
    origins, lens, src = _gen(n, slot, k, 6000 + n)

    def forge(p, blobs):
        return [b if q == p else forge_bus(b) for q, b in enumerate(blobs)]

    spec = {"kind": "send", "origins": origins, "lens": lens, "slot": slot, "src": src}
    (st, _, _), rcs = sharded.run_inprocess(n, bounds, spec, max_payload=slot, uncached=forged,
                                            blobs_for=forge if forged else None)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == 1).all()
    assert (st["part_sys_scope"] == (1 if forged else 0)).all()
    check(st, st["dst"], n, origins, lens, src)


def test_refusals(rlo):
    import torch

    n, slot, k = 8, 64, 16
    origins, lens, src = _gen(n, slot, k, 7000)
    s = torch.from_numpy(src.reshape(-1)).cuda()
    d = torch.full((n * k * 128,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rlo.World(n, max_payload=slot, one_xcd=True) as w:  # one-XCD worlds: refused at the program
        with pytest.raises(rlo.RloError):
            w.program_send(origins, s, d, slot, lens=lens)
        latency_runs_clean(w)
    with rlo.World(n, max_payload=slot, bulk_max=1 << 20) as w:  # a bulk world: the launch is refused
        w.program_send(origins, s, d, slot, lens=lens)
        with pytest.raises(rlo.RloError):
            w.run()
        latency_runs_clean(w)
    with rlo.World(n, max_payload=slot) as w:  # a slot above max_payload
        with pytest.raises(rlo.RloError):
            w.program_send(origins, torch.cat([s, s]), d, 128)
        latency_runs_clean(w)
        with pytest.raises(ValueError):  # extents and alignment are checked before the library sees them
            w.program_send(origins, s[:-16], d, slot)
        with pytest.raises(ValueError):
            w.program_send(origins, s, d[:n * k * slot - 16], slot)
        with pytest.raises(ValueError):
            w.program_send(origins, (s.data_ptr() + 8, s.numel()), d, slot)
    torch.cuda.synchronize()
    assert bool((d == FILL).all())  # no refused launch wrote anything


@pytest.mark.parametrize("dtype,numel", [("float32", 1250), ("bfloat16", 3)])
def test_bcast_tensor(rlo, dtype, numel):
    """the tensor is produced by a torch kernel on the current stream right before the call, no synchronise"""
    import torch

    n, origin = 8, 5
    with rlo.World(n) as w:
        base = torch.arange(numel, device="cuda", dtype=torch.float32)
        t = (base * 0.37 - 11.0).to(getattr(torch, dtype))
        out = w.bcast_tensor(origin, t)
        assert w.info_now()["last_kernel"] == 1
        assert out.shape == (n,) + tuple(t.shape) and out.dtype == t.dtype
        for r in range(n):
            assert torch.equal(out[r], t), r

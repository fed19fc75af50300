"""GPU tests of the storm send program (rlo_program_send_storm): open-loop rootless bcasts from any ranks in any mix
whose payloads are read from a caller-owned source buffer in device memory and written, at every receiver, to a
caller-owned destination buffer in device memory -- on the progress kernel's storm-send instantiations (8 waves: the
small copy path with the forwarding tables; 4 waves: the small and the large path), in one part and two, and through
World.bcast_rows.

Expected values never come from the engine: payload bytes are this file's seeded NumPy source, tree parents
pyoracle.tree, checksums pyoracle.msg_checksum summed over what a rank must receive, counts k minus the rank's own.
dst is pre-filled with 0xA5, so the bytes that must stay unwritten are checked too."""
import functools

import numpy as np
import pytest

import pyoracle as orc
from send_cases import FILL, check, check_trees_fifo, forge_bus, gen, latency_runs_clean, rlo  # noqa: F401  (rlo: the fixture)
from send_cases import launch_send_storm as _launch

pytestmark = pytest.mark.gpu
_gen = functools.partial(gen, storm=True)


# (n, max_payload, k, waves): 8 waves -- slots the small copy path stages whole, the forwarding tables (256: a CU per
# rank; 300: two rank-workgroups per CU); 4 waves -- 368: the small path's longest slot; 4096 / 32768: the large path
CASES = [(4, 112, 256, 8), (13, 112, 832, 8), (64, 64, 4096, 8), (256, 64, 4096, 8), (8, 368, 512, 4), (17, 368, 544, 4),
         (300, 64, 1200, 4), (8, 4096, 96, 4), (13, 4096, 104, 4), (4, 32768, 16, 4)]


@pytest.mark.parametrize("n,mp,k,waves", CASES, ids=lambda v: str(v))
def test_exact_bytes(rlo, n, mp, k, waves):
    origins, lens, src = _gen(n, mp, k, 1000 + n + mp)
    try:
        w = rlo.World(n, max_payload=mp)
    except rlo.RloError as e:
        if n == 300 and "[-3]" in str(e):  # RLO_E_OCCUPANCY
            pytest.skip("300 rank-workgroups are not co-resident on this device: the world was refused")
        raise
    with w:
        assert w.info["waves"] == waves
        try:
            st, got = _launch(w, origins, lens, src)
        except rlo.RloError as e:
            if n == 300 and str(e).startswith("rlo_run failed") and "[-1]" in str(e):  # (RLO_E_INVAL from the launch itself)
                pytest.skip("300 rank-workgroups are not co-resident on this device: the launch was refused")
            raise
        check(st, got.reshape(n, k, mp), n, origins, lens, src)
        if mp >= 4096:
            assert w.info["pull"] == 1  # pulled payloads: the default of large-slot worlds


@pytest.mark.parametrize("org", [[0], [1, 5]], ids=["one", "opposite"])
def test_ring_wrap_and_refused_admissions(rlo, org):
    """the smallest rings a world takes, every originator sending 8 x the ring capacity: tails wrap, originations
    are refused and retried"""
    n, slot, cap = 8, 112, 16
    origins = [org[i % len(org)] for i in range(8 * cap * len(org))]
    origins, lens, src = _gen(n, slot, len(origins), 3000 + len(org), origins=origins)
    assert np.bincount(origins, minlength=n)[org].min() >= 8 * cap
    with rlo.World(n, max_payload=slot, ring_slots=cap) as w:
        assert w.info["ring_slots"] == cap
        st, got = _launch(w, origins, lens, src)
        check(st, got.reshape(n, len(origins), slot), n, origins, lens, src)


@pytest.mark.parametrize("n,mp", [(8, 64), (13, 64), (64, 64), (8, 4096)], ids=lambda v: str(v))
def test_trees_and_per_origin_fifo(rlo, n, mp):
    k = 12 * n
    origins, lens, src = _gen(n, mp, k, 2000 + n + mp)
    with rlo.World(n, max_payload=mp) as w:
        st, got = _launch(w, origins, lens, src, log=True, log_cap=k)
        check(st, got.reshape(n, k, mp), n, origins, lens, src)
        check_trees_fifo(w, n, origins, lens)


def test_pushed_large_payloads(rlo, monkeypatch):
    """RLO_PULL=0 (read when the world is created): large messages travel whole through the rings"""
    monkeypatch.setenv("RLO_PULL", "0")
    n, mp, k = 8, 4096, 96
    origins, lens, src = _gen(n, mp, k, 1500)
    with rlo.World(n, max_payload=mp) as w:
        assert w.info["pull"] == 0
        st, got = _launch(w, origins, lens, src)
        check(st, got.reshape(n, k, mp), n, origins, lens, src)


def test_three_launches_then_other_programs(rlo):
    """different seeds, origins, lengths, k and buffers every time, then the storm and the send program on the same
    world: no stale schedule, length or pointer state"""
    n, slot = 8, 112
    with rlo.World(n, max_payload=slot) as w:
        for j, k in enumerate((40, 96, 24)):
            origins, lens, src = _gen(n, slot, k, 5000 + j)
            st, got = _launch(w, origins, lens, src)
            check(st, got.reshape(n, k, slot), n, origins, lens, src)
        ks, ln, seed = 128, 64, 11
        w.program_storm(ks, ln, seed=seed)
        w.run()
        st = w.stats()
        ref = orc.storm(n, seed, ks, ln)
        assert (st["error"] == 0).all()
        assert np.array_equal(st["bcast_delivered"].astype(np.int64), ref["count"])
        assert np.array_equal(st["bcast_sum"], ref["sum"])
        import torch

        k = 32
        origins, lens, src = _gen(n, slot, k, 5100)
        s = torch.from_numpy(src.reshape(-1)).cuda()
        d = torch.full((n * k * slot,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w.program_send(origins, s, d, slot, lens=lens)
        w.run()
        assert w.info_now()["last_kernel"] == 1
        check(w.stats(), d.cpu().numpy().reshape(n, k, slot), n, origins, lens, src)


def test_rank_stride_gap_stays_unwritten(rlo):
    n, slot, k = 8, 112, 64
    origins, lens, src = _gen(n, slot, k, 6500)
    rs = k * slot + 256
    with rlo.World(n, max_payload=slot) as w:
        st, got = _launch(w, origins, lens, src, rank_stride=rs)
        assert (got[:, k * slot:] == FILL).all()  # the gap up to rank_stride
        check(st, got[:, :k * slot].reshape(n, k, slot), n, origins, lens, src)


@pytest.mark.parametrize("forged", [False, True], ids=["agent", "system"])
def test_parts(rlo, forged):
    """two parts in one process, each with its own src and dst; forged: every part sees its peer "on another GPU", so
    both store at system scope"""
    from rlo import sharded

    n, bounds, slot = 8, [0, 3, 8], 64
    k = 16 * n
    origins, lens, src = _gen(n, slot, k, 6000 + n)

    def forge(p, blobs):
        return [b if q == p else forge_bus(b) for q, b in enumerate(blobs)]

    spec = {"kind": "send_storm", "origins": origins, "lens": lens, "slot": slot, "src": src}
    (st, _, _), rcs = sharded.run_inprocess(n, bounds, spec, max_payload=slot, uncached=forged,
                                            blobs_for=forge if forged else None)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == 0).all()
    assert (st["part_sys_scope"] == (1 if forged else 0)).all()
    check(st, st["dst"], n, origins, lens, src)


def test_refusals(rlo):
    import torch

    n, slot, k = 8, 64, 16
    origins, lens, src = _gen(n, slot, k, 7000)
    s = torch.from_numpy(src.reshape(-1)).cuda()
    d = torch.full((n * k * 128,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    inval = r"rlo_program_send_storm failed.*\[-1\]"  # RLO_E_INVAL from the program call, before anything is uploaded
    with rlo.World(n, max_payload=slot, bulk_max=1 << 20) as w:  # a bulk world
        latency_runs_clean(w)
        with pytest.raises(rlo.RloError, match=inval):
            w.program_send_storm(origins, s, d, slot, lens=lens)
        w.run()  # the previous program still runs
        assert (w.stats()["error"] == 0).all() and int(w.stats()["originated"].sum()) == 16
    with rlo.World(n, max_payload=slot, one_xcd=True) as w:  # a one-XCD world
        latency_runs_clean(w)
        with pytest.raises(rlo.RloError, match=inval):
            w.program_send_storm(origins, s, d, slot, lens=lens)
        w.run()
        assert (w.stats()["error"] == 0).all() and int(w.stats()["originated"].sum()) == 16
    with rlo.World(n, max_payload=slot) as w:  # a slot beyond max_payload
        latency_runs_clean(w)
        with pytest.raises(rlo.RloError, match=inval):
            w.program_send_storm(origins, torch.cat([s, s]), d, 128)
        w.run()
        assert (w.stats()["error"] == 0).all() and int(w.stats()["originated"].sum()) == 16
        with pytest.raises(ValueError):  # extents are checked before the library sees them
            w.program_send_storm(origins, s[:-16], d, slot)
        with pytest.raises(ValueError):
            w.program_send_storm(origins, s, d[:n * k * slot - 16], slot)
    torch.cuda.synchronize()
    assert bool((d == FILL).all())  # no refused program wrote anything


@pytest.mark.parametrize("dtype,shape,n,mp", [("float32", (96, 24), 8, 4096), ("uint8", (40, 1000), 8, 1008),
                                               ("bfloat16", (12, 2048), 4, 4096)], ids=lambda v: str(v))
def test_bcast_rows(rlo, dtype, shape, n, mp):
    """the tensor is produced by a torch kernel on the current stream right before the call, no synchronise"""
    import torch

    rng = np.random.default_rng(8000 + shape[0])
    origins = rng.integers(0, n, shape[0])
    with rlo.World(n, max_payload=mp) as w:
        base = torch.arange(shape[0] * shape[1], device="cuda", dtype=torch.float32).reshape(shape)
        t = ((base * 0.37 - 11.0) % 251).to(getattr(torch, dtype))
        keep = t.clone()
        out = w.bcast_rows(origins, t)
        assert w.info_now()["last_kernel"] == 0
        assert out.shape == (n,) + tuple(t.shape) and out.dtype == t.dtype
        assert torch.equal(t, keep)  # t itself is unchanged
        for r in range(n):
            assert torch.equal(out[r], t), r

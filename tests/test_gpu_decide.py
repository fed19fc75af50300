"""GPU tests of the decide program (rlo_program_decide): proposal / vote / decision rounds whose proposal data, verdict
table, received data and decisions are caller-owned device buffers -- on the hop kernel, in one part and two, over
several launches of one world, and through World.decide_rows.

Expected values never come from the engine (decide_cases.py): decisions and who judged what are pyoracle.iar's with
ORC_JUDGE_HASH, the device's verdict table is built on the host from the oracle library's orc_judge_hash, the logs and
counters are compared by iar_sets.check_events as exact multisets."""
import numpy as np
import pytest

import decide_cases as dc
from decide_cases import launch as _launch
import iar_sets
import pyoracle as orc
from send_cases import FILL, forge_bus, latency_runs_clean, rlo  # noqa: F401  (rlo: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [4, 8, 13, 16])
def test_exact_outputs(rlo, n):
    """4 proposals per rank (the next one's prefetch and the reuse of a pending entry both run), places of 992 bytes,
    lengths around every chunk edge; the oracle's outcome has every length approved, a decline and an unreached pair"""
    c = dc.picked(n, 4)
    c.conditions()
    with rlo.World(n, max_payload=1008) as w:
        st, logs, dst, dec = _launch(w, c)
        c.check(st, logs, dst, dec)


def test_no_verdict_table_approves_everything(rlo):
    n = 8
    c = dc.Case(n, iar_sets.mixed_props(n, 2, list(dc.LENS), 811), 992, 0, 0)
    assert all(v == 1 for v in c.result.values()) and len(c.judged) == c.k * (n - 1)
    with rlo.World(n, max_payload=1008) as w:
        st, logs, dst, dec = _launch(w, c, verdict=False)
        c.check(st, logs, dst, dec)
        assert (dec == 1).all()  # (and every non-origin place is filled: c.judged is every such pair, compared exactly)


def test_three_launches_of_one_world(rlo):
    import torch

    n = 8
    with rlo.World(n, max_payload=1008) as w:
        dst = torch.empty(n * 32 * 992, dtype=torch.uint8, device="cuda")
        dec = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        for j, (per, slot, lens) in enumerate(((3, 992, dc.LENS), (4, 64, (0, 1, 15, 16, 17, 63, 64)), (1, 496, (5, 480, 496, 33)))):
            # (the last one into buffers the second filled: re-filled by _launch)
            c = dc.picked(n, per, slot=slot, lens=lens, data_seed=2 + j)
            st, logs, got, out = _launch(w, c, dst=dst, dec=dec)
            c.check(st, logs, got, out)


@pytest.mark.parametrize("forged", [False, True], ids=["agent", "system"])
@pytest.mark.parametrize("n,bounds", [(8, [0, 3, 8]), (16, [0, 8, 16])], ids=["8", "16"])
def test_parts(rlo, n, bounds, forged):
    """two parts in one process, each with its own src, verdict, dst and decision; forged: every part sees its peer "on
    another GPU", so both run the system-scope instantiation"""
    from rlo import sharded

    c = dc.picked(n, 2)

    def forge(p, blobs):
        return [b if q == p else forge_bus(b) for q, b in enumerate(blobs)]

    spec = {"kind": "decide", "origins": c.origins, "lens": c.lens, "slot": c.slot, "src": c.src, "verdict": c.verdict,
            "log": True, "log_cap": 4 * c.k + 16}
    (st, logs, _), rcs = sharded.run_inprocess(n, bounds, spec, max_payload=1008, uncached=forged,
                                               blobs_for=forge if forged else None)
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == 1).all()
    assert (st["part_sys_scope"] == (1 if forged else 0)).all()
    c.check(st, logs, st["dst"], st["decision"])


def test_refusals(rlo):
    import torch

    k, slot = 8, 64
    origins = [i % 8 for i in range(k)]
    s = torch.zeros(k * 1008, dtype=torch.uint8, device="cuda")
    d = torch.full((17 * k * 1008,), FILL, dtype=torch.uint8, device="cuda")
    o = torch.full((17 * k,), FILL, dtype=torch.uint8, device="cuda")
    v = torch.ones(17 * k, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    worlds = [dict(n=17, max_payload=1008), dict(n=8, max_payload=1008, one_xcd=True),
              dict(n=8, max_payload=1008, bulk_max=1 << 20), dict(n=8, max_payload=1008, pend_hbm=True)]
    for kw in worlds:  # refused at the program, whatever the arguments
        with rlo.World(**kw) as w:
            with pytest.raises(rlo.RloError):
                w.program_decide(origins, s, d, o, slot, verdict=v)
            latency_runs_clean(w)
    with rlo.World(8, max_payload=1008) as w:
        with pytest.raises(rlo.RloError):  # beyond the hop kernel's 64 lanes
            w.program_decide(origins, s, d, o, 1008, verdict=v)
        latency_runs_clean(w)
        for bad in ((s[:k * slot - 16], d, o, v), (s, d[:8 * k * slot - 16], o, v), (s, d, o[:8 * k - 1], v),
                    (s, d, o, v[:8 * k - 1]), ((s.data_ptr() + 8, s.numel() - 8), d, o, v),
                    (s, (d.data_ptr() + 4, d.numel() - 4), o, v)):
            with pytest.raises(ValueError):  # extents and alignment are checked before the library sees them
                w.program_decide(origins, bad[0], bad[1], bad[2], slot, verdict=bad[3])
        latency_runs_clean(w)
    with rlo.World(8, max_payload=64) as w:  # 16 + slot > max_payload
        with pytest.raises(rlo.RloError):
            w.program_decide(origins, s, d, o, 64, verdict=v)
        w.program_decide(origins, s, d, o, 48, verdict=v)  # (16 + 48: fits; loaded, not launched)
        latency_runs_clean(w)
    torch.cuda.synchronize()
    assert bool((d == FILL).all()) and bool((o == FILL).all())  # no refused program wrote anything


def test_decide_rows_refuses_long_rows(rlo):
    import torch

    with rlo.World(8) as w:
        with pytest.raises(ValueError):
            w.decide_rows([0, 1], torch.zeros((2, 1250), dtype=torch.float32, device="cuda"))  # 5,000 bytes a row
        with pytest.raises(ValueError):
            w.decide_rows([0, 1], torch.zeros((2, 249), dtype=torch.float32, device="cuda"))   # 996 bytes: beyond 992
        latency_runs_clean(w)


@pytest.mark.parametrize("dtype,numel", [("float32", 248), ("bfloat16", 3)])
def test_decide_rows(rlo, dtype, numel):
    """rows produced by a torch kernel on the current stream right before the call, no synchronise; the verdict tensor
    declines some proposals; decided and rows are the oracle's"""
    import torch

    n, k = 8, 24
    origins = [(5 * i + 2) % n for i in range(k)]
    base = torch.arange(k * numel, device="cuda", dtype=torch.float32).reshape(k, numel)
    t = (base * 0.37 - 11.0).to(getattr(torch, dtype))
    host = t.cpu().view(torch.uint8).reshape(k, -1).numpy()
    props = [(origins[i], i, host[i].tobytes()) for i in range(k)]
    for seed in range(1, 2000):  # chosen on the oracle's output alone: both outcomes occur
        c = dc.Case(n, props, -(-host.shape[1] // 16) * 16, seed, 60000)
        if 0 < sum(c.result.values()) < k:
            break
    want_dec = c.expected()[1]
    want_rows = np.zeros((n, k, host.shape[1]), dtype=np.uint8)
    want_rows[want_dec == 1] = np.broadcast_to(host, (n,) + host.shape)[want_dec == 1]
    with rlo.World(n) as w:
        decided, rows = w.decide_rows(origins, t, verdict=torch.from_numpy(c.verdict).cuda())
        assert w.info_now()["last_kernel"] == 1
        assert decided.dtype == torch.uint8 and tuple(decided.shape) == (n, k)
        assert rows.dtype == t.dtype and tuple(rows.shape) == (n,) + tuple(t.shape)
        assert np.array_equal(decided.cpu().numpy(), want_dec)
        assert np.array_equal(rows.cpu().view(torch.uint8).reshape(n, k, -1).numpy(), want_rows)

"""CPU tests of the decide program's host side: rlo_decide_check (the argument checks of rlo_program_decide that need
no GPU), the rlo_decide_cfg_t mirror, the kernel pick of the program's two hop instantiations, and the pure-Python
helpers of World.decide_rows.  The workloads the GPU tests run are checked against their conditions here as well, so
a case that no longer meets them fails without a GPU."""
import ctypes
import itertools

import numpy as np
import pytest

from send_cases import header_layout

# rlo_device.hpp Mode
STORM, LAT, IAR, HOST, LL, XCD1, SEND, DECIDE = 1, 2, 4, 128, 16384, 524288, 1048576, 33554432


def _check(k=4, slot=64, origins=None, lens=None, src=0x1000, dst=0x2000, decision=0x3000, verdict=0x4000, n=8,
           max_payload=4096, flags=0, null_origin=False):
    """rlo_decide_check of one configuration (the device pointers are never dereferenced by it)"""
    from rlo import _lib as L

    origin = np.asarray(origins if origins is not None else [i % n for i in range(max(k, 1))], dtype=np.int32)
    ln = None if lens is None else np.asarray(lens, dtype=np.uint32)
    cfg = L.DecideCfg()
    cfg.k = k
    cfg.origin = None if null_origin else origin.ctypes.data
    cfg.len = None if ln is None else ln.ctypes.data
    cfg.src, cfg.dst, cfg.decision, cfg.verdict = src, dst, decision, verdict
    cfg.slot = slot
    cfg.flags = flags
    return L.load().rlo_decide_check(ctypes.byref(cfg), n, max_payload)


def test_decide_check_accepts_the_boundaries():
    from rlo import _lib as L

    assert _check() == L.RLO_OK
    assert _check(slot=16, lens=[0, 16, 1, 15]) == L.RLO_OK  # len 0 and len == slot
    assert _check(slot=992, lens=[0, 992, 991, 1]) == L.RLO_OK
    assert _check(slot=992, max_payload=1008) == L.RLO_OK  # 16 + slot == max_payload
    assert _check(slot=992, max_payload=993) == L.RLO_OK   # ... == max_payload rounded up to 16
    assert _check(slot=64, max_payload=80) == L.RLO_OK and _check(slot=64, max_payload=65) == L.RLO_OK
    assert _check(verdict=None) == L.RLO_OK  # no table: approve everything
    assert _check(verdict=0x4001, decision=0x3003) == L.RLO_OK  # byte tables: no alignment asked
    assert _check(k=1, origins=[7]) == L.RLO_OK and _check(k=1, origins=[0]) == L.RLO_OK
    assert _check(n=2, origins=[0, 1, 1, 0]) == L.RLO_OK and _check(n=16, origins=[15, 0, 8, 15]) == L.RLO_OK
    assert _check(flags=L.RLO_FLAG_LOG) == L.RLO_OK


@pytest.mark.parametrize("kw", [
    {"k": 0}, {"k": -1}, {"k": 1 << 31},
    {"slot": 0}, {"slot": 8}, {"slot": 24}, {"slot": 1000}, {"slot": 1008}, {"slot": 1024},
    {"slot": 64, "max_payload": 64}, {"slot": 64, "max_payload": 48},
    {"slot": 992, "max_payload": 992},
    {"lens": [0, 1, 1, 65]}, {"lens": [1 << 31, 1, 1, 1]},
    {"origins": [0, 1, -1, 2]}, {"origins": [0, 8, 1, 2]},
    {"n": 17}, {"n": 1, "origins": [0, 0, 0, 0]}, {"n": 0, "origins": [0, 0, 0, 0]}, {"n": 16, "origins": [0, 16, 1, 2]},
    {"src": 0}, {"dst": 0}, {"decision": 0}, {"src": 0x1008}, {"dst": 0x2004},
    {"null_origin": True},
    {"flags": 2}, {"flags": 4}, {"flags": 0x100},
], ids=str)
def test_decide_check_refuses(kw):
    from rlo import _lib as L

    if kw.get("k", 0) == 1 << 31:  # (no origin list of that size: the count is refused before it is read)
        kw = dict(kw, origins=[0])
    assert _check(**kw) == L.RLO_E_INVAL


@pytest.mark.parametrize("slot", [16, 64, 496, 976, 992])
def test_decide_check_max_payload_boundary(slot):
    """16 + slot against round16(max_payload), one byte either side of every edge"""
    from rlo import _lib as L

    for mp in range(slot - 32, slot + 48):
        want = L.RLO_OK if 16 + slot <= -(-mp // 16) * 16 else L.RLO_E_INVAL
        assert _check(slot=slot, max_payload=max(mp, 0)) == want, (slot, mp)


def test_decide_check_grid():
    """k x slot x a length at each end x n_ranks: accepted exactly where every argument is in range"""
    from rlo import _lib as L

    for k, slot, ln, n in itertools.product((1, 3, 40), (16, 480, 992, 1008), (0, 1, 16, 992, 993), (2, 16, 17)):
        ok = slot <= 992 and ln <= slot and n <= 16
        got = _check(k=k, slot=slot, lens=[ln] * k, n=n, origins=[(n - 1) * (i % 2) for i in range(k)] if n <= 16 else [0] * k)
        assert got == (L.RLO_OK if ok else L.RLO_E_INVAL), (k, slot, ln, n)


def test_decide_check_null_cfg_and_wrapper():
    import rlo
    from rlo import _lib as L

    assert L.load().rlo_decide_check(None, 8, 64) == L.RLO_E_INVAL
    assert rlo.decide_check([0, 1, 2], 64, 8, 4096) == L.RLO_OK
    assert rlo.decide_check([0, 1, 2], 64, 8, 4096, lens=[0, 64, 7], verdict=0x5000, flags=L.RLO_FLAG_LOG) == L.RLO_OK
    assert rlo.decide_check([0, 1, 2], 64, 17, 4096) == L.RLO_E_INVAL
    assert rlo.decide_check([0, 1, 2], 64, 8, 4096, src=0x1004) == L.RLO_E_INVAL
    with pytest.raises(ValueError):
        rlo.decide_check([0, 1, 2], 64, 8, 4096, lens=[1, 2])


def test_decide_cfg_matches_the_c_header(tmp_path):
    """sizeof and every field offset of rlo_decide_cfg_t against its ctypes mirror"""
    from rlo import _lib as L

    got = header_layout(tmp_path, "rlo_decide_cfg_t", L.DecideCfg, macros=["RLO_FLAG_LOG"])
    assert got["sizeof"] == 72 and got["RLO_FLAG_LOG"] == L.RLO_FLAG_LOG
    assert [f for f, _ in L.DecideCfg._fields_] == ["k", "origin", "len", "src", "verdict", "dst", "decision", "slot", "flags",
                                                    "log_cap", "pad"]


def _pick(kernel, variant, mode, pend_hbm, sys_scope):
    from rlo import _lib as L

    out = (ctypes.c_uint32 * 5)()
    rc = L.load().rlo_kernel_pick(kernel, variant, mode, pend_hbm, sys_scope, out)
    assert rc in (L.RLO_OK, L.RLO_E_INVAL), rc
    return tuple(out) if rc == L.RLO_OK else None


def test_hop_pick_of_the_decide_rows():
    for sys_scope in (0, 1):
        assert _pick(1, 0, LL | IAR | DECIDE, 0, sys_scope) == (0, sys_scope, 0, 0, 1)
        assert _pick(1, 0, LL | IAR | DECIDE | XCD1, 0, sys_scope) is None   # no one-XCD form
        assert _pick(1, 0, LL | IAR | DECIDE | SEND, 0, sys_scope) is None   # not beside the send program
        assert _pick(1, 0, LL | IAR | DECIDE, 1, sys_scope) is None          # no pending table in HBM
        assert _pick(1, 0, LL | DECIDE, 0, sys_scope) is None                # always beside MODE_IAR | MODE_LL
        assert _pick(1, 0, IAR | DECIDE, 0, sys_scope) is None
        # without the bit: the iar program's rows, fifth argument 0
        assert _pick(1, 0, LL | IAR, 0, sys_scope) == (0, sys_scope, 0, 0, 0)
        assert _pick(1, 0, LL | IAR, 1, sys_scope) == (1, sys_scope, 0, 0, 0)


def test_progress_pick_ignores_the_decide_bit():
    for variant, pend_hbm, ll, prog in itertools.product((8, 4, 5), (0, 1), (0, 1), (STORM, LAT, IAR, HOST, HOST | IAR, LAT | IAR)):
        mode = prog | (LL if ll else 0)
        assert _pick(0, variant, mode | DECIDE, pend_hbm, 0) == _pick(0, variant, mode, pend_hbm, 0) is not None


def test_decide_slot():
    import rlo

    assert [rlo.decide_slot(b, 4096) for b in (0, 1, 6, 16, 17, 976, 977, 992)] == [16, 16, 16, 16, 32, 976, 992, 992]
    assert rlo.decide_slot(992, 1008) == 992 and rlo.decide_slot(992, 993) == 992 and rlo.decide_slot(48, 64) == 48
    for row, mp in ((993, 4096), (5000, 4096), (992, 992), (49, 64), (-1, 4096)):
        with pytest.raises(ValueError):
            rlo.decide_slot(row, mp)


@pytest.mark.parametrize("n", [4, 8, 13, 16])
def test_gpu_cases_meet_their_conditions(n):
    """the workloads of tests/test_gpu_decide.py, on the oracle alone: every length approved once, a decline, a pair
    never reached, and the verdict table equal to the oracle's judge entry by entry (Case.__init__)"""
    import decide_cases as dc

    c = dc.picked(n, 4)
    c.conditions()
    assert c.k == 4 * n and c.slot == 992
    assert set(int(x) for x in c.lens) == set(dc.LENS) or n == 4  # (4 ranks x 4 proposals: 12 of the 13 lengths)
    nz = c.verdict[c.verdict != 0]
    assert len(set(nz.tolist())) > 8 and (c.verdict == 0).any()  # varied non-zero bytes, and declines
    dst, dec = c.expected()
    assert (dec == dec[0]).all() and set(np.unique(dec).tolist()) == {0, 1}

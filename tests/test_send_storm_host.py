"""CPU tests of the storm send program's host side: rlo_send_storm_check (the argument checks of
rlo_program_send_storm that need no GPU), the rlo_send_storm_cfg_t mirror, the kernel pick of the program's mode, and
rlo.rows_slot (the row and padding arithmetic of World.bcast_rows)."""
import ctypes
import itertools

import pytest

import test_kernel_pick as kp

SENDS, SENDB, SEND, TL, HDIAG = 8388608, 2097152, 1048576, 32768, 4096  # rlo_device.hpp MODE_SENDS, _SENDB, _SEND, _TL, _HDIAG
# rlo_kernel.hip kPmStormSend
P_SENDS = 0xFFFFFFFF & ~(kp.LAT | kp.IAR | kp.HOST | TL | kp.LL | SEND | SENDB | HDIAG)


def _check(origins=(0, 1, 2, 7), slot=64, n=8, max_payload=64, **kw):
    import rlo

    return rlo.send_storm_check(list(origins), slot, n, max_payload, **kw)


def test_check_accepts_the_ranges():
    from rlo import _lib as L

    assert _check() == L.RLO_OK
    assert _check(slot=16, lens=[1, 16, 15, 1]) == L.RLO_OK
    assert _check(slot=64, lens=[1, 64, 63, 17]) == L.RLO_OK  # len 1, len == slot
    assert _check(slot=112, max_payload=100) == L.RLO_OK  # max_payload rounded up to 16
    assert _check(slot=65520, max_payload=65520, lens=[1, 65520, 1008, 1025]) == L.RLO_OK  # the largest slot
    assert _check(slot=48, max_payload=4096) == L.RLO_OK  # a slot below max_payload
    assert _check(origins=[7]) == L.RLO_OK and _check(origins=[0], n=1) == L.RLO_OK
    assert _check(lens=[64, 64, 64, 17], rank_stride=3 * 64 + 32) == L.RLO_OK  # holds the last message
    assert _check(rank_stride=4 * 64) == L.RLO_OK and _check(rank_stride=1 << 33) == L.RLO_OK
    assert _check(window=1) == L.RLO_OK and _check(window=64) == L.RLO_OK
    assert _check(flags=L.RLO_FLAG_LOG | L.RLO_FLAG_HIST | L.RLO_FLAG_PROF) == L.RLO_OK


@pytest.mark.parametrize("kw", [
    {"origins": []},                                   # k 0
    {"src": 0x1008}, {"dst": 0x2004}, {"src": 0}, {"dst": 0},  # a misaligned / null pointer
    {"slot": 0}, {"slot": 24}, {"slot": 80}, {"slot": 128, "max_payload": 100},  # slot 0 / no multiple of 16 / > round16(max_payload)
    {"origins": [0, 8, 1, 2]}, {"origins": [0, -1, 1, 2]},  # an origin out of range
    {"lens": [1, 0, 1, 1]},                            # len 0
    {"lens": [1, 65, 1, 1]},                           # len > slot
    {"rank_stride": 3 * 64 + 48}, {"lens": [64, 64, 64, 17], "rank_stride": 3 * 64 + 16},  # a rank stride too small
    {"rank_stride": 4 * 64 + 8},                       # ... or no multiple of 16
    {"flags": 8}, {"flags": 0x100},                    # an unknown flag (the timeline, the send program's ORDERED)
    {"n": 0},
], ids=str)
def test_check_refuses(kw):
    from rlo import _lib as L

    assert _check(**kw) == L.RLO_E_INVAL


def test_check_null_cfg_and_count():
    from rlo import _lib as L

    lib = L.load()
    assert lib.rlo_send_storm_check(None, 8, 64) == L.RLO_E_INVAL
    cfg = L.SendStormCfg()
    cfg.k, cfg.origin, cfg.src, cfg.dst, cfg.slot = 4, None, 0x1000, 0x1000, 64  # no origin list
    assert lib.rlo_send_storm_check(ctypes.byref(cfg), 8, 64) == L.RLO_E_INVAL
    org = (ctypes.c_int32 * 1)(0)
    cfg.origin = ctypes.cast(org, ctypes.c_void_p)
    cfg.k = 1 << 32  # beyond the storm's id width (refused before the list is read)
    assert lib.rlo_send_storm_check(ctypes.byref(cfg), 8, 64) == L.RLO_E_INVAL
    cfg.k = 1
    assert lib.rlo_send_storm_check(ctypes.byref(cfg), 8, 64) == L.RLO_OK
    with pytest.raises(ValueError):
        _check(lens=[1, 2, 3])  # the wrapper: one length per message


def test_pick_of_the_new_bit_alone():
    for pend_hbm, sys_scope in itertools.product((0, 1), (0, 1)):  # neither changes it
        assert kp.pick(0, 8, SENDS, pend_hbm, sys_scope) == (8, 0, 0, 0, P_SENDS)
        assert kp.pick(0, 4, SENDS, pend_hbm, sys_scope) == (4, 0, 0, 0, P_SENDS)
        assert kp.pick(0, 5, SENDS, pend_hbm, sys_scope) is None  # a bulk world: the bulk send program's
    # logs, histograms and the phase profile pick no other kernel
    assert kp.pick(0, 8, SENDS | 16 | 32 | 64, 0, 0) == (8, 0, 0, 0, P_SENDS)
    # no doorbells: the storm never runs with them
    assert kp.pick(0, 8, SENDS | kp.LL, 0, 0) is None and kp.pick(0, 4, SENDS | kp.LL, 0, 0) is None
    # the masks are what rlo_kernel.hip says: every existing one is another value
    assert P_SENDS not in (kp.ALL, kp.P_LAT, kp.P_IAR, kp.P_STORM, kp.P_HOST)


def test_pick_of_every_existing_program_is_unchanged_by_the_new_bit():
    for variant, pend_hbm, ll, prog in itertools.product((8, 4, 5), (0, 1), (0, 1), kp.PROGRAMS):
        mode = prog | (kp.LL if ll else 0)
        want = kp.PROGRESS[(variant, pend_hbm, ll)][kp.PROGRAMS.index(prog)]
        assert kp.pick(0, variant, mode | SENDS, pend_hbm, 0) == want == kp.pick(0, variant, mode, pend_hbm, 0)
    # the bulk send program's pick too
    assert kp.pick(0, 5, SENDB | kp.LL, 0, 0) == kp.pick(0, 5, SENDB | kp.LL | 16, 0, 0) != None  # noqa: E711


def test_rows_slot():
    """bcast_rows' row and padding arithmetic: the place is the row rounded up to 16 bytes; rows beyond the world's
    max_payload (and empty rows) are refused"""
    import rlo

    assert rlo.rows_slot(96, 4096) == 96          # float32 [.., 24]: no padding
    assert rlo.rows_slot(1000, 1008) == 1008      # uint8 [.., 1000]: 8 bytes of padding
    assert rlo.rows_slot(4096, 4096) == 4096      # bfloat16 [.., 2048]
    assert rlo.rows_slot(1, 64) == 16 and rlo.rows_slot(17, 64) == 32 and rlo.rows_slot(64, 64) == 64
    assert rlo.rows_slot(100, 100) == 112         # a world whose max_payload is itself no multiple of 16
    for bad in ((0, 64), (65, 64), (4097, 4096), (-1, 64)):
        with pytest.raises(ValueError):
            rlo.rows_slot(*bad)

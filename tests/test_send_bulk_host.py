"""CPU tests of the bulk send program's host side: rlo_send_bulk_check (the argument checks of rlo_program_send_bulk
that need no GPU), the rlo_send_bulk_cfg_t mirror, rlo.bulk_fragments (the fragmentation World.bcast_tensor uses in a
world with bulk messages), and the kernel pick of the program's mode."""
import ctypes

import pytest

import test_kernel_pick as kp

MIB = 1 << 20
SENDB = 2097152  # rlo_device.hpp MODE_SENDB
P_SENDB = 0xFFFFFFFF & ~(kp.STORM | kp.IAR | kp.HOST | 32768 | 65536)  # rlo_kernel.hip kPmSendBulk


def _check(origins=(0, 1, 2, 7), stride=64, n=8, bulk_max=MIB, **kw):
    import rlo

    return rlo.send_bulk_check(list(origins), stride, n, bulk_max, **kw)


def test_check_accepts_the_ranges():
    from rlo import _lib as L

    assert _check() == L.RLO_OK
    assert _check(stride=16, lens=[1, 16, 15, 1]) == L.RLO_OK
    assert _check(stride=MIB, lens=[1, MIB, MIB - 1, 17]) == L.RLO_OK  # len 1, len == stride == bulk_max
    assert _check(stride=MIB) == L.RLO_OK  # no lengths: every message is `stride` bytes
    assert _check(stride=2 * MIB, lens=[MIB] * 4) == L.RLO_OK  # a stride beyond bulk_max, lengths within it
    assert _check(stride=(1 << 32) - 16, lens=[1] * 4) == L.RLO_OK
    assert _check(origins=[7]) == L.RLO_OK and _check(origins=[0], n=1) == L.RLO_OK
    assert _check(stride=64, lens=[64, 64, 64, 17], rank_stride=3 * 64 + 32) == L.RLO_OK  # holds the last message
    assert _check(stride=64, rank_stride=4 * 64) == L.RLO_OK and _check(stride=64, rank_stride=4096) == L.RLO_OK
    assert _check(flags=L.RLO_FLAG_LOG | L.RLO_FLAG_HIST) == L.RLO_OK


@pytest.mark.parametrize("kw", [
    {"origins": []},                                   # k 0
    {"origins": [0, 8, 1, 2]}, {"origins": [0, -1, 1, 2]},  # an origin out of range
    {"lens": [1, 0, 1, 1]},                            # len 0
    {"lens": [1, 65, 1, 1]},                           # len > stride
    {"stride": 2 * MIB, "lens": [1, MIB + 1, 1, 1]},   # len > bulk_max
    {"stride": 2 * MIB},                               # ... and every message `stride` bytes
    {"stride": 24}, {"stride": 0}, {"stride": 1 << 32},  # a stride that is no multiple of 16 / out of range
    {"rank_stride": 3 * 64 + 48}, {"lens": [64, 64, 64, 17], "rank_stride": 3 * 64 + 16},  # a rank stride too small
    {"rank_stride": 4 * 64 + 8},
    {"src": 0x1008}, {"dst": 0x2004}, {"src": 0}, {"dst": 0},  # a misaligned / null pointer
    {"flags": 4}, {"flags": 0x100},                    # an unknown flag (RLO_SEND_ORDERED is the send program's)
    {"bulk_max": 0},
], ids=str)
def test_check_refuses(kw):
    from rlo import _lib as L

    assert _check(**kw) == L.RLO_E_INVAL


def test_check_null_cfg_and_count():
    from rlo import _lib as L

    lib = L.load()
    assert lib.rlo_send_bulk_check(None, 8, MIB) == L.RLO_E_INVAL
    cfg = L.SendBulkCfg()
    cfg.k, cfg.stride, cfg.src, cfg.dst = 1 << 31, 64, 0x1000, 0x1000  # (refused before the origin list is read)
    org = (ctypes.c_int32 * 1)(0)
    cfg.origin = ctypes.addressof(org)
    assert lib.rlo_send_bulk_check(ctypes.byref(cfg), 8, MIB) == L.RLO_E_INVAL
    cfg.k, cfg.origin = 1, None
    assert lib.rlo_send_bulk_check(ctypes.byref(cfg), 8, MIB) == L.RLO_E_INVAL
    cfg.origin = ctypes.addressof(org)
    assert lib.rlo_send_bulk_check(ctypes.byref(cfg), 8, MIB) == L.RLO_OK
    assert lib.rlo_send_bulk_check(ctypes.byref(cfg), 0, MIB) == L.RLO_E_INVAL


@pytest.mark.parametrize("bulk_max", [MIB, MIB + 16, MIB + 5, 48])
def test_bulk_fragments_tile_the_bytes(bulk_max):
    import rlo

    frag = bulk_max // 16 * 16
    for nbytes in (1, 15, 16, bulk_max - 1, bulk_max, bulk_max + 1, 3 * bulk_max + 5):
        fr = rlo.bulk_fragments(nbytes, bulk_max)
        at = 0
        for off, ln in fr:
            assert off == at and 1 <= ln <= frag
            at += ln
        assert at == nbytes  # they tile [0, nbytes) exactly
        assert all(ln == frag and ln % 16 == 0 for _, ln in fr[:-1])  # every one but the last: a multiple of 16
        assert len(fr) == -(-nbytes // frag)
    assert rlo.bulk_fragments(0, bulk_max) == []


def test_bulk_fragments_refuses_a_world_without_bulk():
    import rlo

    for bad in (0, 15):
        with pytest.raises(ValueError):
            rlo.bulk_fragments(100, bad)


def test_pick_of_the_bulk_send_program():
    """mode MODE_SENDB | MODE_LL, no other program bit: the program's own instantiation in a bulk world with doorbells,
    no kernel anywhere else -- never the hop kernel, never another row"""
    row = (4, 1, 1, 0, P_SENDB)
    assert row not in kp.PROGRESS_ROWS
    for pend_hbm, sys_scope in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert kp.pick(0, 5, SENDB | kp.LL, pend_hbm, sys_scope) == row
        assert kp.pick(0, 5, SENDB | kp.LL | 16 | 32, pend_hbm, sys_scope) == row  # (log, histogram)
        assert kp.pick(0, 5, SENDB, pend_hbm, sys_scope) is None          # no doorbells
        for variant in (8, 4):
            assert kp.pick(0, variant, SENDB | kp.LL, pend_hbm, sys_scope) is None  # no bulk messages


def test_pick_of_every_other_mode_is_unchanged():
    """every mode tests/test_kernel_pick.py lists picks the row it picked before, with the new bit in the mode or not"""
    for (variant, pend_hbm, ll), rows in sorted(kp.PROGRESS.items()):
        for prog, want in zip(kp.PROGRAMS, rows):
            for extra in (0, SENDB, 0xFFFFFFFF & ~(kp.STORM | kp.LAT | kp.IAR | kp.HOST | kp.LL)):
                assert kp.pick(0, variant, prog | (kp.LL if ll else 0) | extra, pend_hbm, 0) == want
    for (pend_hbm, sys_scope, xcd1, send), want in sorted(kp.HOP.items()):
        mode = kp.LL | kp.LAT | (kp.XCD1 if xcd1 else 0) | (kp.SEND if send else 0)
        assert kp.pick(1, 0, mode, pend_hbm, sys_scope) == (want + (0,) if want else None)

"""CPU tests of the send program's host side: rlo_send_check (the argument checks of rlo_program_send that need no
GPU), the rlo_send_cfg_t mirror, and rlo.send_fragments (the fragmentation World.bcast_tensor uses)."""
import ctypes
import os

import numpy as np
import pytest

from send_cases import header_layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")


def _check(k=4, slot=64, origins=None, lens=None, src=0x1000, dst=0x2000, n=8, max_payload=4096, flags=0, null_origin=False):
    """rlo_send_check of one configuration (src / dst are never dereferenced by it: any aligned non-NULL number does)"""
    from rlo import _lib as L

    origin = np.asarray(origins if origins is not None else [i % n for i in range(max(k, 1))], dtype=np.int32)
    ln = None if lens is None else np.asarray(lens, dtype=np.uint32)
    cfg = L.SendCfg()
    cfg.k = k
    cfg.origin = None if null_origin else origin.ctypes.data
    cfg.len = None if ln is None else ln.ctypes.data
    cfg.src, cfg.dst = src, dst
    cfg.slot = slot
    cfg.flags = flags
    return L.load().rlo_send_check(ctypes.byref(cfg), n, max_payload)


def test_send_check_accepts_the_boundaries():
    from rlo import _lib as L

    assert _check() == L.RLO_OK
    assert _check(slot=16, lens=[1, 16, 1, 16]) == L.RLO_OK
    assert _check(slot=1008, lens=[1, 1008, 1007, 1008]) == L.RLO_OK
    assert _check(slot=64, lens=[1, 64, 63, 17]) == L.RLO_OK  # len 1 and len == slot
    assert _check(slot=64, max_payload=64) == L.RLO_OK
    assert _check(slot=64, max_payload=50) == L.RLO_OK  # max_payload rounded up to 16
    assert _check(k=1, origins=[7]) == L.RLO_OK and _check(k=1, origins=[0]) == L.RLO_OK
    assert _check(flags=L.RLO_FLAG_LOG | L.RLO_FLAG_HIST | L.RLO_SEND_ORDERED) == L.RLO_OK


@pytest.mark.parametrize("kw", [
    {"k": 0},
    {"k": -1},
    {"k": 1 << 31},
    {"slot": 0}, {"slot": 8}, {"slot": 24}, {"slot": 1000}, {"slot": 1024}, {"slot": 1009},
    {"slot": 64, "max_payload": 48},
    {"slot": 1008, "max_payload": 512},
    {"lens": [0, 1, 1, 1]}, {"lens": [1, 1, 1, 65]},
    {"origins": [0, 1, -1, 2]}, {"origins": [0, 8, 1, 2]},
    {"src": 0}, {"dst": 0}, {"src": 0x1008}, {"dst": 0x2004},
    {"null_origin": True},
    {"flags": 4},
], ids=str)
def test_send_check_refuses(kw):
    from rlo import _lib as L

    if kw.get("k", 0) == 1 << 31:  # (no origin list of that size: the count is refused before it is read)
        kw = dict(kw, origins=[0])
    assert _check(**kw) == L.RLO_E_INVAL


def test_send_check_null_cfg():
    from rlo import _lib as L

    assert L.load().rlo_send_check(None, 8, 64) == L.RLO_E_INVAL


@pytest.mark.parametrize("cname,mirror", [("rlo_send_cfg_t", "SendCfg"), ("rlo_send_bulk_cfg_t", "SendBulkCfg"),
                                          ("rlo_send_storm_cfg_t", "SendStormCfg")])
def test_send_cfgs_match_the_c_header(tmp_path, cname, mirror):
    """sizeof and every field offset of the three send cfgs against their ctypes mirrors, and the flag's value"""
    from rlo import _lib as L

    py = getattr(L, mirror)
    got = header_layout(tmp_path, cname, py, macros=["RLO_SEND_ORDERED"])
    assert got["RLO_SEND_ORDERED"] == L.RLO_SEND_ORDERED
    if mirror != "SendCfg":
        assert got["sizeof"] == 64
    if mirror == "SendStormCfg":
        assert [f for f, _ in py._fields_] == ["k", "origin", "len", "src", "dst", "slot", "window", "rank_stride", "flags", "log_cap"]


def test_device_error_names_cover_the_header():
    """every RLO_DERR_* code of rlo_hip.h has a name in L.DERR (9, the one-XCD placement error, was missing)"""
    import re

    from rlo import _lib as L

    codes = {int(v) for v in re.findall(r"#define RLO_DERR_[A-Z_]+ (\d+)", open(os.path.join(INCLUDE, "rlo_hip.h")).read())}
    assert codes and codes == set(L.DERR)
    assert L.DERR[9] == "xcd placement"


@pytest.mark.parametrize("slot", [1008, 16])
@pytest.mark.parametrize("nbytes", [1, 1007, 1008, 1009, 5000, 2 * 1008])
def test_send_fragments_tile_the_bytes(nbytes, slot):
    import rlo

    fr = rlo.send_fragments(nbytes, slot)
    at = 0
    for off, ln in fr:
        assert off == at and 1 <= ln <= slot
        at += ln
    assert at == nbytes  # they tile [0, nbytes) exactly
    assert all(ln == slot for _, ln in fr[:-1])  # only the last is short
    assert len(fr) == -(-nbytes // slot)


def test_send_fragments_default_and_bad_slots():
    import rlo

    assert rlo.send_fragments(5000) == [(0, 1008), (1008, 1008), (2016, 1008), (3024, 1008), (4032, 968)]
    assert rlo.send_fragments(0) == []
    for bad in (0, 8, 1024, -16):
        with pytest.raises(ValueError):
            rlo.send_fragments(100, bad)

"""CPU tests of the kernel pick (rlo_kernel_pick, no GPU): which instantiation of the progress kernel and of the hop
kernel a launch runs, for every (world, program) combination, against tables written out here by hand from the launch
ladders the pick functions replaced -- not derived from the tables of instantiations in rlo_kernel.hip / rlo_hop.hip."""
import ctypes
import itertools

from rlo import _lib as L

# rlo_device.hpp Mode
STORM, LAT, IAR, HOST, LL, XCD1, SEND = 1, 2, 4, 128, 16384, 524288, 1048576
# the program masks (rlo_kernel.hip kPm*): every mode bit but the other programs'
ALL, P_LAT, P_IAR, P_STORM, P_HOST = 0xFFFFFFFF, 0xFFFFFF7A, 0xFFFFFF7C, 0xFFFFFF79, 0xFFFFFFFC

PROGRAMS = (STORM, LAT, IAR, HOST, HOST | IAR, LAT | IAR)

# (variant, pend_hbm, MODE_LL) -> (W, BULK, LL, PH, PM) per program, in the order of PROGRAMS
PROGRESS = {
    (8, 0, 0): ((8, 0, 0, 0, P_STORM), (8, 0, 0, 0, ALL), (8, 0, 0, 0, ALL), (8, 0, 0, 0, ALL), (8, 0, 0, 0, ALL),
                (8, 0, 0, 0, ALL)),
    (8, 0, 1): ((8, 0, 1, 0, ALL), (8, 0, 1, 0, P_LAT), (8, 0, 1, 0, P_IAR), (8, 0, 1, 0, P_HOST), (8, 0, 1, 0, P_HOST),
                (8, 0, 1, 0, ALL)),
    (8, 1, 0): ((8, 0, 0, 0, P_STORM), (8, 0, 0, 0, ALL), (8, 0, 0, 1, ALL), (8, 0, 0, 1, ALL), (8, 0, 0, 1, ALL),
                (8, 0, 0, 1, ALL)),
    (8, 1, 1): ((8, 0, 1, 0, ALL), (8, 0, 1, 0, P_LAT), (8, 0, 1, 1, P_IAR), (8, 0, 1, 1, P_HOST), (8, 0, 1, 1, P_HOST),
                (8, 0, 1, 1, ALL)),
    (4, 0, 0): ((4, 0, 0, 0, ALL), (4, 0, 0, 0, ALL), (4, 0, 0, 0, ALL), (4, 0, 0, 0, ALL), (4, 0, 0, 0, ALL),
                (4, 0, 0, 0, ALL)),
    (4, 0, 1): ((4, 0, 1, 0, ALL), (4, 0, 1, 0, ALL), (4, 0, 1, 0, ALL), (4, 0, 1, 0, P_HOST), (4, 0, 1, 0, P_HOST),
                (4, 0, 1, 0, ALL)),
    (4, 1, 0): ((4, 0, 0, 0, ALL), (4, 0, 0, 0, ALL), (4, 0, 0, 1, ALL), (4, 0, 0, 1, ALL), (4, 0, 0, 1, ALL),
                (4, 0, 0, 1, ALL)),
    (4, 1, 1): ((4, 0, 1, 0, ALL), (4, 0, 1, 0, ALL), (4, 0, 1, 1, ALL), (4, 0, 1, 1, P_HOST), (4, 0, 1, 1, P_HOST),
                (4, 0, 1, 1, ALL)),
    # bulk worlds keep the pending table in LDS: no PH form, with or without pend_hbm
    (5, 0, 0): ((4, 1, 0, 0, P_STORM), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL),
                (4, 1, 0, 0, ALL)),
    (5, 0, 1): ((4, 1, 1, 0, ALL), (4, 1, 1, 0, P_LAT), (4, 1, 1, 0, ALL), (4, 1, 1, 0, P_HOST), (4, 1, 1, 0, P_HOST),
                (4, 1, 1, 0, ALL)),
    (5, 1, 0): ((4, 1, 0, 0, P_STORM), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL), (4, 1, 0, 0, ALL),
                (4, 1, 0, 0, ALL)),
    (5, 1, 1): ((4, 1, 1, 0, ALL), (4, 1, 1, 0, P_LAT), (4, 1, 1, 0, ALL), (4, 1, 1, 0, P_HOST), (4, 1, 1, 0, P_HOST),
                (4, 1, 1, 0, ALL)),
}

# the 21 instantiations the library is built with
PROGRESS_ROWS = {
    (8, 0, 1, 1, P_IAR), (8, 0, 1, 1, P_HOST), (8, 0, 1, 1, ALL), (8, 0, 0, 1, ALL),
    (4, 0, 1, 1, P_HOST), (4, 0, 1, 1, ALL), (4, 0, 0, 1, ALL),
    (8, 0, 1, 0, P_LAT), (8, 0, 1, 0, P_IAR), (8, 0, 0, 0, P_STORM), (8, 0, 1, 0, P_HOST), (8, 0, 1, 0, ALL), (8, 0, 0, 0, ALL),
    (4, 1, 1, 0, P_LAT), (4, 1, 0, 0, P_STORM), (4, 1, 1, 0, P_HOST), (4, 1, 1, 0, ALL), (4, 1, 0, 0, ALL),
    (4, 0, 1, 0, P_HOST), (4, 0, 1, 0, ALL), (4, 0, 0, 0, ALL),
}

# (pend_hbm, sys_scope, MODE_XCD1, MODE_SEND) -> (PH, SYS, LOC, SEND), None: refused
HOP = {
    (0, 0, 0, 0): (0, 0, 0, 0), (1, 0, 0, 0): (1, 0, 0, 0), (0, 1, 0, 0): (0, 1, 0, 0), (1, 1, 0, 0): (1, 1, 0, 0),
    (0, 0, 1, 0): (0, 0, 1, 0), (1, 0, 1, 0): (1, 0, 1, 0), (0, 1, 1, 0): None, (1, 1, 1, 0): None,
    (0, 0, 0, 1): (0, 0, 0, 1), (1, 0, 0, 1): (0, 0, 0, 1), (0, 1, 0, 1): (0, 1, 0, 1), (1, 1, 0, 1): (0, 1, 0, 1),
    (0, 0, 1, 1): None, (1, 0, 1, 1): None, (0, 1, 1, 1): None, (1, 1, 1, 1): None,
}


def pick(kernel, variant, mode, pend_hbm, sys_scope):
    out = (ctypes.c_uint32 * 5)()
    rc = L.load().rlo_kernel_pick(kernel, variant, mode, pend_hbm, sys_scope, out)
    assert rc in (L.RLO_OK, L.RLO_E_INVAL), rc
    return tuple(out) if rc == L.RLO_OK else None


def test_progress_pick_is_the_ladders():
    assert len(PROGRESS_ROWS) == 21
    reached = set()
    for (variant, pend_hbm, ll), rows in sorted(PROGRESS.items()):
        assert len(rows) == len(PROGRAMS)
        for prog, want in zip(PROGRAMS, rows):
            for sys_scope in (0, 1):  # (the hop kernel's: no part in this pick)
                got = pick(0, variant, prog | (LL if ll else 0), pend_hbm, sys_scope)
                assert got == want, (variant, pend_hbm, ll, prog, got, want)
            assert got in PROGRESS_ROWS, got
            reached.add(got)
    assert len(PROGRESS) == 3 * 2 * 2
    assert reached == PROGRESS_ROWS


def test_progress_pick_looks_at_the_mode_bits_it_names_only():
    """logs, histograms, the diagnostics bits: none of them picks another kernel"""
    other = 0xFFFFFFFF & ~(STORM | LAT | IAR | HOST | LL)
    for variant, pend_hbm, ll, prog in itertools.product((8, 4, 5), (0, 1), (0, 1), PROGRAMS):
        mode = prog | (LL if ll else 0)
        assert pick(0, variant, mode | other, pend_hbm, 0) == pick(0, variant, mode, pend_hbm, 0)


def test_hop_pick():
    reached = set()
    for (pend_hbm, sys_scope, xcd1, send), want in sorted(HOP.items()):
        mode = LL | LAT | (XCD1 if xcd1 else 0) | (SEND if send else 0)
        got = pick(1, 0, mode, pend_hbm, sys_scope)
        assert got == (want + (0,) if want else None), (pend_hbm, sys_scope, xcd1, send, got, want)
        if got:
            reached.add(got[:4])
    assert len(HOP) == 16 and len(reached) == 8  # every instantiation
    for sys_scope in (0, 1):  # the send program has no pending table, whatever the world's
        assert pick(1, 0, LL | SEND, 1, sys_scope) == pick(1, 0, LL | SEND, 0, sys_scope) == (0, sys_scope, 0, 1, 0)
    assert pick(1, 0, LL | SEND | XCD1, 0, 0) is None  # the send program on one XCD
    assert pick(1, 0, LL | LAT | XCD1, 0, 1) is None   # system scope on one XCD


def test_pick_refuses_bad_arguments():
    lib = L.load()
    out = (ctypes.c_uint32 * 5)()
    assert lib.rlo_kernel_pick(2, 8, STORM, 0, 0, out) == L.RLO_E_INVAL
    assert lib.rlo_kernel_pick(0, 7, STORM, 0, 0, out) == L.RLO_E_INVAL
    assert lib.rlo_kernel_pick(0, 8, STORM, 0, 0, None) == L.RLO_E_INVAL

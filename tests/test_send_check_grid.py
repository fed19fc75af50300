"""CPU characterisation test of the send programs' argument checks: rlo_send_check, rlo_send_bulk_check and
rlo_send_storm_check answer every case of the grid of tests/golden/gen_send_check_grid.py exactly as the library did
before the three checks were folded into one (tests/golden/send_check_grid.json, recorded from that library)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import gen_send_check_grid as grid  # noqa: E402

# the single-factor refusals of tests/test_send_host.py, test_send_bulk_host.py and test_send_storm_host.py, as
# (factor, value) of the grid; origins and len by what the variant is
K0, K_NEG, K_PAST, NO_ORIGIN, ORIGIN_N, ORIGIN_NEG = (("origins", i) for i in (5, 6, 7, 4, 2, 3))
LEN_0, LEN_PAST, LEN_0_FIRST, LEN_PAST_LAST = (("len", i) for i in (2, 3, 5, 6))
RS_SHORT, RS_ODD = ("rank_stride", 1), ("rank_stride", 3)  # need - 16, need + 8
POINTERS = [("src", 0), ("dst", 0), ("src", 0x1008), ("dst", 0x2004)]
HOST_REFUSALS = {
    "send": [K0, K_NEG, K_PAST, NO_ORIGIN, ORIGIN_N, ORIGIN_NEG, LEN_0_FIRST, LEN_PAST_LAST, ("flags", 4)] + POINTERS
            + [("place", p) for p in (0, 8, 24, 1000, 1024, 1009)],
    "send_bulk": [K0, ORIGIN_N, ORIGIN_NEG, LEN_0, LEN_PAST, RS_SHORT, RS_ODD, ("flags", 4), ("flags", 0x100), ("cap", 0)]
                 + POINTERS + [("place", p) for p in (1 << 21, 24, 0, 1 << 32)],
    "send_storm": [K0, ORIGIN_N, ORIGIN_NEG, LEN_0, LEN_PAST, RS_SHORT, RS_ODD, ("flags", 8), ("flags", 0x100),
                   ("n_ranks", 0)] + POINTERS + [("place", p) for p in (0, 24, 80)],
}


@pytest.fixture(scope="module")
def lib():
    return grid.load()


@pytest.mark.parametrize("prog", grid.PROGRAMS)
def test_every_case_answers_as_before_the_fold(lib, golden, prog):
    want = golden("send_check_grid.json")[prog]
    got = grid.run(lib, prog)
    assert len(got) == len(want) > 1000
    differ = [(case, ch, w) for (case, ch), w in zip(got, want) if ch != w]
    assert not differ, "%d of %d cases differ, the first: %r" % (len(differ), len(want), differ[:5])


@pytest.mark.parametrize("prog", grid.PROGRAMS)
def test_the_grid_holds_both_outcomes_and_the_host_tests_refusals(lib, golden, prog):
    want = golden("send_check_grid.json")[prog]
    cases = [case for case, _ in grid.run(lib, prog)]
    assert set(want) == {"A", "R"} and want[0] == "A" and cases[0] == {}  # (the base case is accepted)
    f = grid.factors(prog)
    for name, value in HOST_REFUSALS[prog]:
        index = value if name in ("origins", "len", "rank_stride") else f[name].index(value)
        assert want[cases.index({name: index})] == "R", (name, value)

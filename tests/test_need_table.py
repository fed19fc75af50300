"""CPU test of the storm kernel's forwarding tables (rlo_need_table, no GPU: the host side of the function the kernel
fills its tables with).  For every (rank, origin) pair of a world the rank's parent in the origin's tree picks the
table, and the entry, decoded, must name the children the oracle gives that rank, each on the virtual channel of a
message that has or has not wrapped past rank n - 1.  The oracle alone decides the expectation."""
import ctypes

import pytest

import pyoracle as orc
from rlo import _lib as L

WORLDS = (3, 4, 5, 8, 13, 16, 17, 33, 64, 100, 255, 256, 257)


def tables(n, rank):
    below, above = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    assert L.load().rlo_need_table(n, rank, below, above) == L.RLO_OK
    return below, above


def check_rank(n, rank, parents):
    """parents[o]: the parent array of origin o's tree"""
    topo = orc.topology(n, rank)
    sl, lw = topo["send_list"], topo["last_wall"]
    below, above = tables(n, rank)
    for o in range(n):
        if o == rank:
            continue
        frm = int(parents[o][rank])
        assert frm >= 0, (n, rank, o)
        mask = (above if frm > lw else below)[o]
        assert mask >> (2 * len(sl)) == 0, (n, rank, o, hex(mask))
        kids = []
        for j, child in enumerate(sl):
            bits = (mask >> (2 * j)) & 3
            assert bits in (0, 1, 2), (n, rank, o, j)  # one virtual channel per child
            if bits:
                assert (bits >> 1) == (1 if child < o else 0), (n, rank, o, child)
                kids.append(child)
        assert sorted(kids) == sorted(orc.children(n, rank, o, frm)), (n, rank, o, frm)


@pytest.mark.parametrize("n", WORLDS)
def test_every_rank_every_origin(n):
    parents = [orc.tree(n, o)[0] for o in range(n)]
    for rank in range(n):
        check_rank(n, rank, parents)


def test_2048_ranks():
    n = 2048
    parents = [orc.tree(n, o)[0] for o in range(n)]
    for rank in (0, 1, 1024, 1792, 2046, 2047):
        check_rank(n, rank, parents)


def test_refusals():
    lib = L.load()
    a = (ctypes.c_uint32 * 4)()
    assert lib.rlo_need_table(1, 0, a, a) == L.RLO_E_INVAL
    assert lib.rlo_need_table(4, 4, a, a) == L.RLO_E_INVAL
    assert lib.rlo_need_table(4, -1, a, a) == L.RLO_E_INVAL
    assert lib.rlo_need_table(4, 0, None, a) == L.RLO_E_INVAL

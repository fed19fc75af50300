"""The world-size cases of tests/test_gpu_world_sizes.py -- TEST INFRASTRUCTURE ONLY.

One table, read by the GPU tests (which run every program on every world of every size) and by
tests/test_world_sizes_oracle.py (which checks on the CPU, with the oracle alone, that every workload can show what
it is meant to show: a bad seed fails there, not on the device).

The shape of the rootless skip-ring tree is a function of the world size n alone, and every kernel derives a
message's children from it with code of its own.  SIZES walks that axis:
   2 .. 16        every world whose largest in-degree is <= 4: the hop kernel's register table of out-rings (ntab), and
                  every world in which the hop kernel runs iar and decide
   17             the first world of the hop kernel's LDS table (ltab), the first whose iar runs on the progress kernel
   17, 33, 65, 129   where the send list (sll) and the largest in-degree grow: 5, 6, 7, 8 in-edges
   18 .. 32       every size between two powers of two once: each has another deepest level and another last_wall
   63 / 64 / 65, 127 / 128 / 129, 255 / 256   both sides of a power of two, where the wrap past rank n - 1 (virtual
                  channel 1, child < origin) changes; 255 / 256 are the LDS table's last entries (256 x 8 = 2048 pairs,
                  the table's size exactly); 256 is the last world whose progress kernel has its
                  doorbell instantiation co-resident (ll_ok) on a 256-CU device
   100, 200       far from any power of two

Per n, two worlds, every program on each in a fixed order (PROGRAMS), so that every program also runs behind another
one on the same world; a one-XCD world for 2 .. 32; two-part worlds for PART_SIZES.  A size leaves a program only
for a reason in LEFT_OUT.

Expected values never come from the engine: send_cases.expected, decide_cases.Case, iar_sets.oracle_events,
bcast_length_cases.Expected.
"""
import functools

import numpy as np

import bcast_length_cases as bc
import decide_cases as dc
import iar_sets
import pyoracle as orc
from send_cases import gen

SIZES = tuple(range(2, 34)) + (63, 64, 65, 100, 127, 128, 129, 200, 255, 256)
HOP_CONSENSUS_MAX = 16  # the hop kernel runs iar (one own proposal in flight) and decide up to here (plan_hop)
ONE_XCD_MAX = 32        # the one-XCD worlds of this file: every size at which the LOC instantiation's rank-waves
#                         rendezvous on one XCD's 32 CUs with a CU each
PART_SIZES = (2, 3, 5, 16, 17, 33)
HOP, PROGRESS = 1, 0    # rlo_world_info_t.last_kernel

# world -> its creation arguments and what rlo_world_query must say of it
WORLDS = {
    "A": (dict(max_payload=64), dict(waves=8, ll_ok=1)),                # 8 waves, doorbells
    "B": (dict(max_payload=1008), dict(waves=4, pull=1)),               # 4 waves, large slots, pulled payloads
    "X": (dict(max_payload=64, one_xcd=True), dict(waves=8, ll_ok=1)),  # cached rings, one XCD
}
# world -> (program id, what runs, the last_kernel expected: a value or a function of n), in launch order
PROGRAMS = {
    "A": (("storm-send", "send_storm", PROGRESS), ("storm", "storm", PROGRESS), ("latency", "latency", HOP),
          ("send", "send", HOP), ("storm-send-again", "send_storm", PROGRESS)),
    "B": (("send", "send", HOP), ("iar", "iar", lambda n: HOP if n <= HOP_CONSENSUS_MAX else PROGRESS),
          ("decide", "decide", HOP), ("storm-send", "send_storm", PROGRESS), ("send-again", "send", HOP)),
    "X": (("latency", "latency", HOP), ("iar", "iar", HOP)),
}
# (world, program id) -> (the sizes that leave it, why): the only exceptions; the CPU test counts them
LEFT_OUT = {
    ("B", "decide"): (lambda n: n > HOP_CONSENSUS_MAX,
                      "rlo_program_decide refuses worlds of more than 16 ranks (the hop kernel's one-proposal worlds)"),
    ("X", "latency"): (lambda n: n > ONE_XCD_MAX, "one-XCD worlds here stop at 32 ranks, a CU of the XCD each"),
    ("X", "iar"): (lambda n: n > HOP_CONSENSUS_MAX,
                   "a one-XCD world runs the hop kernel or nothing, and the hop kernel runs iar up to 16 ranks"),
}
# B / iar beyond 16 ranks stays in: the launch goes to the progress kernel (PROGRAMS names the kernel per size)


def kernel_of(world, pid, n):
    k = next(p[2] for p in PROGRAMS[world] if p[0] == pid)
    return k(n) if callable(k) else k


def items(world):
    """(n, program id) in the order the GPU tests run them: size by size, each size's programs in launch order"""
    return [(n, p[0]) for n in SIZES for p in PROGRAMS[world]
            if not ((world, p[0]) in LEFT_OUT and LEFT_OUT[(world, p[0])][0](n))]


# ------------------------------------------------------------------------------------------------ send workloads
# (world, program id) -> (slot, messages per rank, storm lengths, seed base, lengths that must occur)
SENDS = {
    ("A", "storm-send"): (64, 4, True, 11000, (1, 15, 16, 17, 63, 64)),
    ("A", "send"): (64, 2, False, 12000, ()),
    ("A", "storm-send-again"): (64, 4, True, 13000, (1, 15, 16, 17, 63, 64)),
    # a short message goes to the doorbell and through the ring, a long one through the ring alone
    ("B", "send"): (1008, 2, False, 14000, (1, 17, 1007, 1008)),
    # the small copy path and the large-message rounds in one launch.  Ten lengths must occur, so the worlds of 2, 3
    # and 4 ranks send 5, 4 and 3 messages per rank, not 2
    ("B", "storm-send"): (1008, 2, True, 15000, (1, 15, 16, 17, 64, 65, 368, 369, 1007, 1008)),
    ("B", "send-again"): (1008, 2, False, 16000, (1, 17, 1007, 1008)),
}
PART_SENDS = {"send": (64, 4, False, 17000, ()), "send_storm": (64, 4, True, 18000, (1, 15, 16, 17, 63, 64))}


def _send_load(n, slot, per, storm, seed, must):
    per = max(per, -(-len(must) // n))
    rng = np.random.default_rng(seed)
    origins = np.tile(rng.permutation(n), per).astype(np.int32)  # a seeded permutation of the ranks, repeated
    origins, lens, src = gen(n, slot, len(origins), seed, origins=origins, storm=storm)
    if not storm:
        lens[:len(must)] = must  # (gen(storm=True) does the same with its own list)
    return origins, lens, src


@functools.lru_cache(maxsize=4)
def send_load(world, pid, n):
    """(origins, lens, src [k][slot]) of a send or storm-send launch: every rank an origin `per` times"""
    slot, per, storm, base, must = SENDS[(world, pid)]
    return _send_load(n, slot, per, storm, base + n, must)


def part_send_load(kind, n):
    slot, per, storm, base, must = PART_SENDS[kind]
    return _send_load(n, slot, per, storm, base + n, must)


def in_edges(n):
    """{rank: {(parent, virtual channel)}} over all n trees: what a rank can receive over (vc 1: the message has
    wrapped past rank n - 1, child < origin)"""
    out = {r: set() for r in range(n)}
    for o in range(n):
        par = orc.tree(n, o)[0]
        for r in range(n):
            if r != o:
                out[r].add((int(par[r]), 1 if r < o else 0))
    return out


def send_conditions(n, origins, lens, must, per=2):
    """every rank originates at least `per` times; over the list's origins every rank receives over each of its
    in-edges, on each virtual channel the oracle has for it; every length of `must` occurs.  (A list in which every
    rank originates meets the in-edge condition by construction -- in_edges is the union over all n trees --, so the
    second assertion pins nothing beyond the first; it is computed from the list's own origins so that a list thinned
    to fewer origins also says which edges it lost)"""
    own = np.bincount(origins, minlength=n)
    assert len(own) == n and own.min() >= per, ("originations per rank", own.min())
    seen = {r: set() for r in range(n)}
    for o in sorted(set(int(x) for x in origins)):
        par = orc.tree(n, o)[0]
        for r in range(n):
            if r != o:
                seen[r].add((int(par[r]), 1 if r < o else 0))
    assert seen == in_edges(n)
    missing = sorted(set(must) - set(int(x) for x in lens))
    assert not missing, ("lengths that never occur", missing)


# ------------------------------------------------------------------------------------------------ generated programs
STORM_SEED, LAT_SEED, LAT_ROUNDS, LEN = 21000, 22000, 64, 64


@functools.lru_cache(maxsize=4)
def storm_expected(n):
    """world A's generated storm: 8 n bcasts of 64 bytes from random origins"""
    return bc.Expected(n, STORM_SEED + n, 8 * n, LEN)


@functools.lru_cache(maxsize=4)
def latency_expected(n):
    """the latency program of worlds A and X: 64 rounds of 64 bytes"""
    return bc.Expected(n, LAT_SEED + n, LAT_ROUNDS, LEN)


# ------------------------------------------------------------------------------------------------ iar
IAR_LENS = {"B": (0, 16, 33, 97, 992), "X": (0, 16, 33)}
# proposals per rank: 2.  At 2 ranks world B's two proposals per rank have four different lengths, and "every length
# approved, one proposal declined" cannot hold of four proposals of four lengths: 8 per rank there
IAR_PER = {("B", 2): 8}


def decline_ppm(n):
    """declines per million judge calls so that about a quarter of the proposals is declined by one of n - 1 judges"""
    return int(round(1e6 * (1.0 - 0.75 ** (1.0 / (n - 1)))))


class IarCase:
    def __init__(self, world, n):
        self.n, self.ppm = n, decline_ppm(n)
        self.props = iar_sets.mixed_props(n, IAR_PER.get((world, n), 2), IAR_LENS[world], 9000 + n)
        room = 4 * len(self.props) * n + 1024
        for seed in range(1, 200):  # the judge seed: the first that meets the conditions, on the oracle's output alone
            self.cfg, self._keep = orc.judge_cfg(orc.ORC_JUDGE_HASH, seed=seed, ppm=self.ppm)
            self.ev = iar_sets.oracle_events(n, self.props, self.cfg, 1, cap=room)
            try:
                iar_sets.input_conditions(self.props, self.ev)
            except AssertionError:
                continue
            self.seed = seed
            break
        else:
            raise AssertionError("no judge seed below 200 meets the conditions at %d ranks" % n)
        per_rank = np.bincount([e[1] for e in self.ev], minlength=n)
        self.log_cap = int(per_rank.max()) + 16  # the most records any rank writes, and some room


@functools.lru_cache(maxsize=4)
def iar_case(world, n):
    return IarCase(world, n)


# ------------------------------------------------------------------------------------------------ decide
def _decide_n2():
    """2 ranks have one judge per proposal and it is always reached, so Case.conditions' "some (rank, proposal) pair is
    never reached" cannot hold, and 4 proposals per rank all differ in length, so none could be declined: 8 proposals
    per rank, the data seed of decide_cases.picked's rule, and the first judge seed for which every occurring length
    has an approved proposal and at least one proposal is declined"""
    props = iar_sets.mixed_props(2, 8, list(dc.LENS), 7000 + 31 * 2 + 1)
    for seed in range(1, 2000):
        c = dc.Case(2, props, 992, seed, dc.start_ppm(2))
        try:
            iar_sets.input_conditions(c.props, c.ev)
        except AssertionError:
            continue
        return c
    raise AssertionError("no judge seed below 2000 meets the conditions at 2 ranks")


@functools.lru_cache(maxsize=None)
def decide_case(n):
    """places of 992 bytes, decide_cases.LENS, on world B and in the two-part worlds; n >= 3: decide_cases.picked(n, 4)
    (2 proposals per rank, as tests/test_gpu_decide.py::test_parts takes, all differ in length at 3 ranks, so none
    could be declined); 2 ranks: see _decide_n2"""
    return _decide_n2() if n == 2 else dc.picked(n, 4)


def decide_conditions(n, c):
    if n == 2:
        iar_sets.input_conditions(c.props, c.ev)
        assert len(c.judged) == c.k  # one judge each, always reached
    else:
        c.conditions()


# ------------------------------------------------------------------------------------------------ parts
def part_bounds(n):
    """a part of one rank at either end of the world (the same split at 2 ranks)"""
    return [[0, 1, n]] if n == 2 else [[0, 1, n], [0, n - 1, n]]


def part_items():
    """(n, bounds index, program kind): send and storm send everywhere, decide up to 16 ranks"""
    return [(n, b, kind) for n in PART_SIZES for b in range(len(part_bounds(n)))
            for kind in ("send", "send_storm", "decide") if kind != "decide" or n <= HOP_CONSENSUS_MAX]


PART_KERNEL = {"send": HOP, "send_storm": PROGRESS, "decide": HOP}


# ------------------------------------------------------------------------------------------------ the tree's figures
def max_in_degree(n):
    return max(len({p for p, _ in e}) for e in in_edges(n).values())

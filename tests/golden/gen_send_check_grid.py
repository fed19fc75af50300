#!/usr/bin/env python3
"""Record rlo_send_check, rlo_send_bulk_check and rlo_send_storm_check over a grid of cfgs into send_check_grid.json.

TEST INFRASTRUCTURE ONLY.  The fixture is what the library at the commit BEFORE a change to the send programs' host
side (rlo_world.cpp: the three *_check functions and what they share) answers: tests/test_send_check_grid.py holds
every later library to exactly these outcomes.  Run it against a build of that commit, never against the change it
is to check:

    python tests/golden/gen_send_check_grid.py path/to/that/build/librlo_hip.so

The grid: per program one accepted base case, and from it every single factor and every pair of factors varied over
the values below (FACTORS; a value is named by its index, a case by {factor: index}).  The cfgs are filled by hand
and the exported functions called through ctypes, so the Python wrappers (rlo.send_bulk_check ...) are not part of
what is pinned.  One character per case, 'A' RLO_OK, 'R' RLO_E_INVAL, in the order of cases().
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "rootless-coll-mpi-ops_amd"))

from rlo import _lib as L  # noqa: E402  (the cfg mirrors and constants only: the library is loaded here)

FIXTURE = os.path.join(HERE, "send_check_grid.json")
PROGRAMS = ("send", "send_bulk", "send_storm")
FUNC = {"send": "rlo_send_check", "send_bulk": "rlo_send_bulk_check", "send_storm": "rlo_send_storm_check"}
CFG = {"send": L.SendCfg, "send_bulk": L.SendBulkCfg, "send_storm": L.SendStormCfg}
PLACE = {"send": "slot", "send_bulk": "stride", "send_storm": "slot"}
K_PAST = {"send": 1 << 31, "send_bulk": 1 << 31, "send_storm": 1 << 32}  # (2^31 is a valid storm count: never passed)
ALLOWED = {"send": L.RLO_FLAG_LOG | L.RLO_FLAG_HIST | L.RLO_SEND_ORDERED, "send_bulk": L.RLO_FLAG_LOG | L.RLO_FLAG_HIST,
           "send_storm": L.RLO_FLAG_LOG | L.RLO_FLAG_HIST | L.RLO_FLAG_PROF}
BASE_CAP = {"send": 4096, "send_bulk": 1 << 20, "send_storm": 64}  # max_payload / bulk_max of the base case
U32, U64 = (1 << 32) - 1, (1 << 64) - 1

# origins: (k, the list behind it; None = a NULL pointer).  An in-range k is never larger than its list
ORIGINS = [(4, [0, 1, 2, 7]), (1, [7]), (4, [0, 8, 1, 2]), (4, [0, -1, 1, 2]), (4, None), (0, [0]), (-1, [0]), ("past", [0])]
# len: None = a NULL pointer, else a function of the place P (a variant with a value outside uint32_t is skipped).
# The last two are the host tests' own spellings of a zero length and a length past the place
LENS = [None, lambda P: [1, P, P - 1, min(17, P)], lambda P: [1, 0, 1, 1], lambda P: [1, P + 1, 1, 1],
        lambda P: [P, P, P, 17], lambda P: [0, 1, 1, 1], lambda P: [1, 1, 1, P + 1]]
# rank_stride: a function of need = (k - 1) * P + round16(the last length) (a value outside uint64_t is skipped)
RANK_STRIDE = [lambda need: 0, lambda need: need - 16, lambda need: need, lambda need: need + 8,
               lambda need: need + 16, lambda need: 1 << 33]


def factors(prog):
    """the program's factors, in order: name -> values, the base case's first"""
    f = {
        "n_ranks": [8, 0, 1],
        "origins": ORIGINS,
        "src": [0x1000, 0, 0x1008],
        "dst": [0x2000, 0, 0x2004],
        "flags": [0] + [1 << b for b in range(10)] + [ALLOWED[prog]],
        # (1000 and 2^21: single-factor refusals of tests/test_send_host.py and tests/test_send_bulk_host.py)
        "place": [64, 0, 8, 16, 24, 80, 1000, 1008, 1009, 1024, 65520, 65536, 1 << 21, (1 << 32) - 16]
                 + ([1 << 32] if prog == "send_bulk" else []),
        "cap": [BASE_CAP[prog]] + [c for c in (0, 48, 50, 64, 100, 512, 1008, 4096, 65520, 65521, 65536, 1 << 20,
                                              (1 << 20) + 16) if c != BASE_CAP[prog]],
        "len": LENS,
    }
    if prog != "send":
        f["rank_stride"] = RANK_STRIDE
    return f


def cases(prog):
    """every case of the program's grid as {factor: value index}, in the fixture's order: the base case (every index
    0), each single factor's other values, each pair of factors' other values"""
    f = factors(prog)
    names = list(f)
    out = [{}]
    for a in names:
        out += [{a: i} for i in range(1, len(f[a]))]
    for a, b in itertools.combinations(names, 2):
        out += [{a: i, b: j} for i in range(1, len(f[a])) for j in range(1, len(f[b]))]
    return out


def build(prog, case):
    """the hand-filled cfg of one case: (cfg, n_ranks, cap, the arrays it points into), or None where a value of the
    case does not fit its field (such a case is not part of the grid)"""
    f = factors(prog)
    v = {name: f[name][case.get(name, 0)] for name in f}
    k, olist = v["origins"]
    k = K_PAST[prog] if k == "past" else k
    P = v["place"]
    lens = None if v["len"] is None else v["len"](P)
    if P > (U64 if prog == "send_bulk" else U32) or (lens is not None and not all(0 <= x <= U32 for x in lens)):
        return None
    cfg = CFG[prog]()
    origin = None if olist is None else (ctypes.c_int32 * len(olist))(*olist)
    ln = None if lens is None else (ctypes.c_uint32 * len(lens))(*lens)
    assert not 0 < k < K_PAST[prog] or ((olist is None or k <= len(olist)) and (lens is None or k <= len(lens)))
    cfg.k = k
    cfg.origin = None if origin is None else ctypes.addressof(origin)
    cfg.len = None if ln is None else ctypes.addressof(ln)
    cfg.src, cfg.dst, cfg.flags = v["src"], v["dst"], v["flags"]
    setattr(cfg, PLACE[prog], P)
    if "rank_stride" in v:
        last = P if lens is None else -(-lens[k - 1 if 0 < k <= len(lens) else -1] // 16) * 16
        rs = v["rank_stride"]((k - 1) * P + last)
        if not 0 <= rs <= U64:
            return None
        cfg.rank_stride = rs
    return cfg, v["n_ranks"], v["cap"], (origin, ln)


def load(path=None):
    lib = ctypes.CDLL(path or L.LIB_PATH)
    for prog in PROGRAMS:
        fn = getattr(lib, FUNC[prog])
        fn.argtypes = [ctypes.POINTER(CFG[prog]), ctypes.c_int, ctypes.c_uint64 if prog == "send_bulk" else ctypes.c_uint32]
        fn.restype = ctypes.c_int
    return lib


def run(lib, prog):
    """the grid's outcomes: (case, character) of every case that fits its fields"""
    out = []
    for case in cases(prog):
        b = build(prog, case)
        if b is None:
            continue
        cfg, n_ranks, cap, _keep = b
        rc = getattr(lib, FUNC[prog])(ctypes.byref(cfg), n_ranks, cap)
        out.append((case, {L.RLO_OK: "A", L.RLO_E_INVAL: "R"}.get(rc, "?")))
    return out


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    grid = {prog: "".join(ch for _, ch in run(lib, prog)) for prog in PROGRAMS}
    with open(FIXTURE, "w") as fh:
        json.dump(grid, fh, indent=0, sort_keys=True)
        fh.write("\n")
    for prog in PROGRAMS:
        print("%s: %d cases, %d accepted" % (prog, len(grid[prog]), grid[prog].count("A")), file=sys.stderr)


if __name__ == "__main__":
    main()

"""Exact-set IAR parity: the device's event records against the pool oracle
(orc_iar_rounds_pool), per (origin, pid) -- TEST INFRASTRUCTURE ONLY.

Every rank runs p proposals (pid = it * n + r) keeping `pool` in flight; judge = the seeded hash judge
(ppm declines per judge call; 0 = approve-all).  The sets compared:
  judge   (rank, origin, pid, NULL arg, verdict)   -- every judge call, the originator's final one too
  action  (rank, origin, pid)                      -- action() at every rank that approved, decision 1
  pickup  (rank, origin, pid, decision)            -- every decision delivery
  result  (rank, pid, decision)                    -- every originator's result
A record seen twice fails (a set would hide it), and so does any swap of pids between two
proposals that keeps the sums equal.

check_events() is the same comparison for an arbitrary proposal list (any data lengths, any judge), as
exact multisets, with the lengths the records carry: a JUDGE record's len is the proposal message's
(16-byte PBuf header + data), an ACTION record's aux the data length kept in the pending entry.
mixed_props() generates such lists; pick_seed() chooses a seed on the oracle's output alone.
"""
from collections import Counter

import numpy as np

import pyoracle as orc

LOG_DELIVER, LOG_JUDGE, LOG_ACTION, LOG_RESULT = 1, 2, 3, 4
TAG_DECISION = 4


def props(n, p, data=b"0123456789abcdef"):
    return [(r, it * n + r, data) for it in range(p) for r in range(n)]


def mixed_props(n, per, lens, seed):
    """`per` proposals per rank in submission order (it-major, as props()): rank r's it-th has pid it * n + r,
    lens[(it * n + r + it) % len(lens)] bytes of data (so a rank's successive proposals differ in length and the
    ranks together walk the whole list), the bytes seeded NumPy ones over all 256 values"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(per):
        for r in range(n):
            dl = lens[(it * n + r + it) % len(lens)]
            out.append((r, it * n + r, rng.integers(0, 256, size=dl, dtype=np.uint8).tobytes()))
    return out


def blob_offsets(proposals):
    """the offset of each proposal's data in the program's data blob: rlo_program_iar appends the data in the
    caller's list order (one part holding every rank), so the cumulative lengths in that order"""
    off, out = 0, []
    for _, _, d in proposals:
        out.append(off)
        off += len(d)
    return out


def oracle_pool(proposals, pool):
    """the oracle entry for a proposal list (as check() and test_gpu_host.py): the proposal pool's (orc_iar_pool) where
    a rank submits more than one, else the reference's one own proposal submitted up front (orc_iar, pool 0)"""
    per = Counter(o for o, _, _ in proposals)
    return pool if per and max(per.values()) > 1 else 0


def oracle_events(n, proposals, cfg, pool, cap=1 << 18):
    """cap: room for the oracle's events (a judge call, an action and a pickup per proposal and rank at the most)"""
    ev = orc.iar(n, proposals, cfg, cap=cap, pool=oracle_pool(proposals, pool))
    assert not [e for e in ev if e[0] == orc.ORC_EV_ERROR]
    return ev


def outcomes(ev):
    """{(origin, pid): decision} from the oracle's RESULT events"""
    return {(rank, pid): a for e, rank, pid, a, b, c in ev if e == orc.ORC_EV_RESULT}


def input_conditions(proposals, ev):
    """What a payload case's inputs must meet, on the oracle's output alone: every data length in the list has an
    approved proposal (so its ACTION records carry that length) and at least one proposal is declined"""
    dec = outcomes(ev)
    assert len(dec) == len(proposals)
    approved = {len(d) for o, pid, d in proposals if dec[(o, pid)] == 1}
    missing = sorted({len(d) for _, _, d in proposals} - approved)
    assert not missing, ("no approved proposal of length", missing)
    assert any(v == 0 for v in dec.values()), "no declined proposal"


def check_events(logs, n, proposals, cfg, pool, stats=None, ev=None):
    """logs: {rank: rows of World.log(rank)} of a program_iar run of `proposals` (origin, pid, data) with the
    judge cfg describes (orc.judge_cfg) and `pool` own proposals in flight; ev: the oracle's events where the
    caller already has them.  Exact multisets per (origin, pid), and the lengths in the records"""
    if ev is None:
        ev = oracle_events(n, proposals, cfg, pool)
    dl = {(o, pid): len(d) for o, pid, d in proposals}
    assert len(dl) == len(proposals)
    want = {k: Counter() for k in ("judge", "action", "pickup", "result")}
    for e, rank, pid, a, b, c in ev:
        if e == orc.ORC_EV_JUDGE:
            want["judge"][(rank, c, pid, a, b)] += 1
        elif e == orc.ORC_EV_ACTION:
            assert b == dl[(c, pid)], ("oracle ACTION length", rank, c, pid, b)
            want["action"][(rank, c, pid)] += 1
        elif e == orc.ORC_EV_PICKUP:
            assert c == 7
            want["pickup"][(rank, b, pid, a)] += 1
        elif e == orc.ORC_EV_RESULT:
            want["result"][(rank, pid, a)] += 1
    got = {k: Counter() for k in want}
    bad_len = []
    for r in range(n):
        for kind_, tag, origin, frm, pid, ln, vote, aux, _ in logs[r]:
            if kind_ == LOG_JUDGE:
                got["judge"][(r, origin, pid, aux, vote)] += 1
                if not aux and ln != 16 + dl.get((origin, pid), -1):  # (the NULL call has no argument)
                    bad_len.append(("judge len", r, origin, pid, ln, 16 + dl.get((origin, pid), -1)))
            elif kind_ == LOG_ACTION:
                got["action"][(r, origin, pid)] += 1
                if aux != dl.get((origin, pid), -1):
                    bad_len.append(("action aux", r, origin, pid, aux, dl.get((origin, pid), -1)))
            elif kind_ == LOG_DELIVER and tag == TAG_DECISION:
                got["pickup"][(r, origin, pid, vote)] += 1
                if ln != 7:
                    bad_len.append(("pickup len", r, origin, pid, ln, 7))
            elif kind_ == LOG_RESULT:
                got["result"][(r, pid, vote)] += 1
            else:
                raise AssertionError(("unexpected record", r, kind_, tag, origin, pid))
    for k in want:
        assert got[k] == want[k], (k, sum(got[k].values()), sum(want[k].values()),
                                   sorted((got[k] - want[k]).items())[:6], sorted((want[k] - got[k]).items())[:6])
    assert not bad_len, bad_len[:8]
    assert sum(want["result"].values()) == len(proposals)
    if stats is not None:
        assert (stats["error"] == 0).all(), stats["error"]
        assert int(stats["own_decided"].sum()) == len(proposals)
        per_rank = {"judge_calls": Counter(), "actions": Counter(), "own_approved": Counter(), "dec_delivered": Counter()}
        for (rank, *_), c in want["judge"].items():
            per_rank["judge_calls"][rank] += c
        for (rank, *_), c in want["action"].items():
            per_rank["actions"][rank] += c
        for (rank, _, d), c in want["result"].items():
            per_rank["own_approved"][rank] += c if d else 0
        for (rank, *_), c in want["pickup"].items():
            per_rank["dec_delivered"][rank] += c
        for k, cnt in per_rank.items():
            exp = [cnt[r] for r in range(n)]
            assert [int(x) for x in stats[k]] == exp, (k, [int(x) for x in stats[k]], exp)
    return ev


def check(logs, n, p, ppm, pool, seed=99):
    """logs: {rank: rows of World.log(rank)} for every world rank"""
    cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_HASH if ppm else orc.ORC_JUDGE_APPROVE, seed=seed, ppm=ppm)
    ev = orc.iar_rounds(n, p, cfg, pool=pool)
    want = {"judge": set(), "action": set(), "pickup": set(), "result": set()}
    for e, rank, pid, a, b, c in ev:
        if e == orc.ORC_EV_JUDGE:
            want["judge"].add((rank, c, pid, a, b))
        elif e == orc.ORC_EV_ACTION:
            want["action"].add((rank, c, pid))
        elif e == orc.ORC_EV_PICKUP:
            want["pickup"].add((rank, b, pid, a))
        elif e == orc.ORC_EV_RESULT:
            want["result"].add((rank, pid, a))
    got = {k: set() for k in want}
    counts = {k: 0 for k in want}
    for r in range(n):
        for kind_, tag, origin, frm, pid, ln, vote, aux, _ in logs[r]:
            if kind_ == LOG_JUDGE:
                got["judge"].add((r, origin, pid, aux, vote)); counts["judge"] += 1
            elif kind_ == LOG_ACTION:
                got["action"].add((r, origin, pid)); counts["action"] += 1
            elif kind_ == LOG_DELIVER and tag == TAG_DECISION:
                got["pickup"].add((r, origin, pid, vote)); counts["pickup"] += 1
            elif kind_ == LOG_RESULT:
                got["result"].add((r, pid, vote)); counts["result"] += 1
    for k in want:
        assert counts[k] == len(got[k]), (k, "duplicate records")
        assert got[k] == want[k], (k, len(got[k]), len(want[k]), sorted(got[k] ^ want[k])[:6])
    assert len(want["result"]) == n * p
    declined = sum(1 for (_, _, d) in want["result"] if d == 0)
    if 0 < ppm < 10000:
        assert 0 < declined < n * p and want["action"], declined  # both outcomes exercised
    return declined

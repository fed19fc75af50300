"""What the tests of the decide program (rlo_program_decide) share: workloads, the verdict table, expected values.

Expected values never come from the engine.  Decisions, and who judged what, are pyoracle.iar's (through
iar_sets.oracle_events) run with ORC_JUDGE_HASH on the proposals (origin[i], i, data_i); the device's verdict table is
built here from the oracle library's own orc_judge_hash(seed, rank, pid): 0 where hash % 1_000_000 < ppm, a varied
non-zero byte elsewhere (so "any non-zero byte approves" is exercised)."""
import functools

import numpy as np

import iar_sets
import pyoracle as orc
from send_cases import FILL

LENS = (0, 1, 15, 16, 17, 31, 32, 33, 975, 976, 977, 991, 992)  # around every 16-B chunk edge of a 992-byte place


def verdict_table(n, k, seed, ppm):
    """uint8 [n][k]: rank r's verdict byte for proposal (pid) i"""
    L = orc.lib()
    out = np.zeros((n, k), dtype=np.uint8)
    for r in range(n):
        for i in range(k):
            h = L.orc_judge_hash(seed, r, i) % 1_000_000
            out[r, i] = 0 if h < ppm else 1 + h % 255
    return out


class Case:
    """proposals (origin, pid = index, data) with the oracle's events for the hash judge (seed, ppm); ppm 0: approve-all"""

    def __init__(self, n, props, slot, seed, ppm):
        assert all(pid == i for i, (_, pid, _) in enumerate(props)) and all(len(d) <= slot for _, _, d in props)
        self.n, self.props, self.slot, self.seed, self.ppm, self.k = n, props, slot, seed, ppm, len(props)
        self.cfg, self._keep = orc.judge_cfg(orc.ORC_JUDGE_HASH if ppm else orc.ORC_JUDGE_APPROVE, seed=seed, ppm=ppm)
        self.ev = iar_sets.oracle_events(n, props, self.cfg, 1)
        self.origins = np.array([o for o, _, _ in props], dtype=np.int32)
        self.lens = np.array([len(d) for _, _, d in props], dtype=np.uint32)
        self.src = np.zeros((self.k, slot), dtype=np.uint8)
        for i, (_, _, d) in enumerate(props):
            self.src[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            self.src[i, len(d):] = 0x3C  # (bytes past a proposal's data in its source place: never to be seen in dst)
        self.verdict = verdict_table(n, self.k, seed, ppm)
        # who judged what: the oracle's JUDGE events with an argument (a == 0; the originator's final call passes NULL)
        self.judged = {(rank, pid) for e, rank, pid, a, b, c in self.ev if e == orc.ORC_EV_JUDGE and a == 0}
        self.result = iar_sets.outcomes(self.ev)  # {(origin, pid): decision}
        for e, rank, pid, a, b, c in self.ev:  # the table is the oracle's judge, entry by entry
            assert e != orc.ORC_EV_JUDGE or a or b == (self.verdict[rank, pid] != 0), (rank, pid, b, self.verdict[rank, pid])

    def conditions(self):
        """on the oracle's output alone: every data length has an approved proposal, at least one proposal is declined,
        at least one (rank, proposal) pair is never reached"""
        iar_sets.input_conditions(self.props, self.ev)
        assert len(self.judged) < self.k * (self.n - 1), "every proposal reached every rank"
        for (o, pid), d in self.result.items():  # (what the issue derives: decided 1 -> every other rank judged it)
            if d == 1:
                assert all((r, pid) in self.judged for r in range(self.n) if r != o)

    def expected(self, fill=FILL):
        """(dst [n][k][slot], decision [n][k]) a correct run leaves in buffers pre-filled with `fill`"""
        dst = np.full((self.n, self.k, self.slot), fill, dtype=np.uint8)
        for r, i in self.judged:
            ln = int(self.lens[i])
            dst[r, i, :ln] = self.src[i, :ln]
            dst[r, i, ln:(ln + 15) // 16 * 16] = 0
        dec = np.empty((self.n, self.k), dtype=np.uint8)
        for i, (o, pid, _) in enumerate(self.props):
            dec[:, i] = self.result[(o, pid)]
        return dst, dec

    def check(self, st, logs, got_dst, got_dec, fill=FILL):
        want_dst, want_dec = self.expected(fill)
        assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
        if not np.array_equal(got_dec, want_dec):
            r, i = (int(x[0]) for x in np.nonzero(got_dec != want_dec))
            raise AssertionError("rank %d proposal %d (origin %d): decision byte 0x%02x, want %d; %d differ" %
                                 (r, i, self.origins[i], got_dec[r, i], want_dec[r, i], int((got_dec != want_dec).sum())))
        if not np.array_equal(got_dst, want_dst):
            r, i, b = (int(x[0]) for x in np.nonzero(got_dst != want_dst))
            raise AssertionError("rank %d proposal %d (origin %d, len %d, judged %s) byte %d: got 0x%02x, want 0x%02x; %d bytes differ" %
                                 (r, i, self.origins[i], self.lens[i], (r, i) in self.judged, b, got_dst[r, i, b],
                                  want_dst[r, i, b], int((got_dst != want_dst).sum())))
        iar_sets.check_events(logs, self.n, self.props, self.cfg, 1, stats=st, ev=self.ev)


def launch(w, c, dst=None, dec=None, verdict=True):
    """one launch of Case c on device buffers made here (dst and the decisions pre-filled with 0xA5): the hop kernel
    ran; returns (stats, logs, dst bytes [n][k][slot], decision bytes [n][k])"""
    import torch

    n, k, slot = w.n_local, c.k, c.slot
    s = torch.from_numpy(c.src.reshape(-1)).cuda()
    v = torch.from_numpy(c.verdict.reshape(-1)).cuda() if verdict else None
    if dst is None:
        dst = torch.empty(n * k * slot, dtype=torch.uint8, device="cuda")
    if dec is None:
        dec = torch.empty(n * k, dtype=torch.uint8, device="cuda")
    d, o = dst[:n * k * slot], dec[:n * k]
    d.fill_(FILL)
    o.fill_(FILL)
    torch.cuda.synchronize()
    w.program_decide(c.origins, s, d, o, slot, lens=c.lens, verdict=v, log=True, log_cap=4 * k + 16)
    w.run()
    assert w.info_now()["last_kernel"] == 1
    st = w.stats()
    logs = {r: w.log(r, cap=4 * k + 16) for r in range(n)}
    return st, logs, d.cpu().numpy().reshape(n, k, slot), o.cpu().numpy().reshape(n, k)


def start_ppm(n):
    """about 60,000 ppm at 8 ranks, scaled so a proposal's chance to pass its n - 1 judges stays about the same"""
    return 60000 * 7 // (n - 1)


@functools.lru_cache(maxsize=None)
def picked(n, per, slot=992, lens=LENS, data_seed=1):
    """a Case of `per` proposals per rank (iar_sets.mixed_props: pid = index, lengths walking `lens`) whose judge seed
    is the first, from 1 up, for which conditions() hold -- chosen on the oracle's output alone"""
    props = iar_sets.mixed_props(n, per, [x for x in lens if x <= slot], 7000 + 31 * n + data_seed)
    for seed in range(1, 2000):
        c = Case(n, props, slot, seed, start_ppm(n))
        try:
            c.conditions()
        except AssertionError:
            continue
        return c
    raise AssertionError("no judge seed below 2000 meets the conditions at %d ranks" % n)

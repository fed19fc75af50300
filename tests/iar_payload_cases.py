"""The proposal-payload cases of tests/test_gpu_iar_payloads.py -- TEST INFRASTRUCTURE ONLY.

One table, read by the GPU tests (which run each case) and by tests/test_iar_payloads_oracle.py (which checks on
the CPU, with the oracle alone, that every case's inputs meet their conditions: a bad seed fails there).

A proposal message is the 16-byte slot header, the 16-byte PBuf header and the data: 2 + ceil(dl / 16) chunks.
The lengths sit on both sides of what changes with the chunk count:
   0           no data (plen == 16)
   1 .. 17     one data chunk, two from 17
   32 / 33     4 / 5 chunks
   48 / 49     5 / 6 chunks: what a world staging 5 chunks (max_payload 64, and every large slot) copies whole
   96 / 97     8 / 9 chunks: the most a doorbell carries (kBellChunks)
   352 / 353   24 / 25 chunks: the most a medium slot (max_payload 368) holds
   992 / 993   64 / 65 chunks: the most the hop kernel takes (plan_hop)
   4079 / 4080 the last partial chunk and the full slot of a default world (max_payload 4096)
"""
import numpy as np

import iar_sets
import pyoracle as orc

L = (0, 1, 15, 16, 17, 32, 33, 48, 49, 96, 97, 352, 353, 992, 993, 4079, 4080)


def lens_for(max_payload):
    return tuple(x for x in L if x <= max_payload - 16)


# declines per million judge calls: (1 - ppm / 1e6) ** (n - 1) ~ 0.75, so about a quarter of the proposals is declined
PPM = {8: 40000, 16: 18000, 17: 18000, 64: 4500}
LARGE = (48, 49, 96, 97, 353, 1000, 4079, 4080)


class Case:
    def __init__(self, cid, n, lens, per, kernel, seed, pool=1, judge="hash", pull=None, offsets=False, waves=None,
                 nsmall=None, **world):
        """lens: one length (a uniform launch) or several (mixed); per: proposals per rank; kernel: the
        last_kernel expected (1: the hop kernel); seed: of the data and of the hash judge; judge "mask": one rank
        declines whatever it is asked; pull: RLO_PULL while the world is created; offsets: the data offsets of the
        proposals beyond 16 bytes must cover every residue mod 4; waves / nsmall: the world's layout"""
        self.id, self.n, self.lens, self.per, self.kernel, self.seed = cid, n, tuple(lens), per, kernel, seed
        self.pool, self.judge, self.pull, self.offsets, self.waves, self.nsmall = pool, judge, pull, offsets, waves, nsmall
        self.world = world
        assert all(16 + x <= world["max_payload"] for x in self.lens)

    def proposals(self):
        return iar_sets.mixed_props(self.n, self.per, self.lens, self.seed)

    def mask(self):
        """the MASK judge's one declining rank: only its own proposals are approved, so per == len(lens) and the
        length rule of mixed_props gives that rank every length once"""
        m = np.zeros(self.n, dtype=np.uint8)
        m[self.n - 2] = 1
        return m

    def oracle_cfg(self):
        if self.judge == "mask":
            return orc.judge_cfg(orc.ORC_JUDGE_MASK, decline=self.mask())
        return orc.judge_cfg(orc.ORC_JUDGE_HASH, seed=self.seed, ppm=PPM[self.n])

    def program_kw(self, abi):
        if self.judge == "mask":
            return {"judge": abi.RLO_JUDGE_MASK, "mask": self.mask()}
        return {"judge": abi.RLO_JUDGE_HASH, "seed": self.seed, "ppm": PPM[self.n]}

    def check_inputs(self, props, ev):
        iar_sets.input_conditions(props, ev)
        if self.offsets:
            res = {off % 4 for off, (_, _, d) in zip(iar_sets.blob_offsets(props), props) if len(d) > 16}
            assert res == {0, 1, 2, 3}, res


HOP = lens_for(1008)
CASES = [
    # 1. the hop kernel: 8 ranks, one own proposal in flight, messages of at most 64 chunks
    *[Case("hop-u%d" % dl, 8, (dl,), 3, 1, 1, max_payload=1008) for dl in (0, 32, 33, 96, 97, 992)],
    Case("hop-mixed", 8, HOP, 4, 1, 1, offsets=True, max_payload=1008),
    Case("hop-mixed-pend-hbm", 8, HOP, 4, 1, 1, max_payload=1008, pend_hbm=True),
    Case("hop-mixed-one-xcd", 8, HOP, 4, 1, 1, max_payload=1008, one_xcd=True),
    Case("hop-mask", 8, (0, 33, 97, 353, 992), 5, 1, 1, judge="mask", max_payload=1008),
    # 2. where the launch changes kernel
    Case("n8-4096-u992", 8, (992,), 3, 1, 1, max_payload=4096),
    Case("n8-4096-u993", 8, (993,), 3, 0, 1, max_payload=4096),
    Case("n16-mixed", 16, HOP, 3, 1, 1, max_payload=1008),
    Case("n17-mixed", 17, HOP, 3, 0, 1, max_payload=1008),
    Case("n8-pool2-mixed", 8, HOP, 4, 0, 1, pool=2, max_payload=1008, proposal_pool=2),
    # 3. the progress kernel, 8 waves
    Case("w8-n17-112-mixed", 17, lens_for(112), 3, 0, 1, waves=8, max_payload=112),
    Case("w8-n17-112-u96", 17, (96,), 3, 0, 1, waves=8, max_payload=112),
    Case("w8-n17-112-mask", 17, (0, 17, 33, 49, 96), 5, 0, 1, judge="mask", waves=8, max_payload=112),
    Case("w8-n8-112-pool4-mixed", 8, lens_for(112), 6, 0, 1, pool=4, waves=8, max_payload=112, proposal_pool=4),
    Case("w8-n8-112-pool4-u96", 8, (96,), 6, 0, 1, pool=4, waves=8, max_payload=112, proposal_pool=4),
    Case("w8-n17-64-mixed", 17, lens_for(64), 3, 0, 1, waves=8, nsmall=5, max_payload=64),
    Case("w8-n17-64-u48", 17, (48,), 3, 0, 1, waves=8, nsmall=5, max_payload=64),
    Case("w8-n17-64-u0", 17, (0,), 3, 0, 1, waves=8, nsmall=5, max_payload=64),
    # 4. the progress kernel, 4 waves, medium slots: the small copy path with 24 chunks staged
    *[Case("w4-n17-368-u%d" % dl, 17, (dl,), 3, 0, 1, waves=4, nsmall=24, max_payload=368) for dl in (0, 96, 97, 352)],
    Case("w4-n17-368-mixed", 17, lens_for(368), 3, 0, 1, waves=4, nsmall=24, max_payload=368),
    Case("w4-n17-368-mask", 17, (0, 17, 49, 97, 352), 5, 0, 1, judge="mask", waves=4, nsmall=24, max_payload=368),
    # 5. the progress kernel, 4 waves, large slots (5 chunks staged): the large-message rounds, pulled and pushed
    Case("w4-n17-4096-mixed", 17, LARGE, 4, 0, 1, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-pool4-mixed", 17, LARGE, 4, 0, 1, pool=4, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-u4080", 17, (4080,), 3, 0, 1, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-pool4-u4080", 17, (4080,), 3, 0, 1, pool=4, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-push-mixed", 17, LARGE, 4, 0, 1, waves=4, nsmall=5, pull="0", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-push-pool4-mixed", 17, LARGE, 4, 0, 1, pool=4, waves=4, nsmall=5, pull="0", max_payload=4096, proposal_pool=4),
    Case("w4-n17-4096-pend-hbm-mixed", 17, LARGE, 4, 0, 1, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4, pend_hbm=True),
    Case("w4-n17-4096-pend-hbm-pool4-mixed", 17, LARGE, 4, 0, 1, pool=4, waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4, pend_hbm=True),
    Case("w4-n17-4096-mask", 17, (49, 97, 353, 1000, 4080), 5, 0, 1, judge="mask", waves=4, nsmall=5, pull="", max_payload=4096, proposal_pool=4),
    # 6. a deeper tree
    Case("n64-mixed", 64, HOP, 2, 0, 1, max_payload=1008),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# 7. two parts in one process: (id, n, bounds, max_payload, lens, per, kernel, seed)
PART_CASES = [("parts-n8-hop", 8, [0, 3, 8], 1008, HOP, 4, 1, 1),
              ("parts-n17-progress", 17, [0, 6, 17], 4096, LARGE, 4, 0, 1)]


def part_case(cid):
    cid_, n, bounds, maxp, lens, per, kernel, seed = next(c for c in PART_CASES if c[0] == cid)
    return bounds, Case(cid_, n, lens, per, kernel, seed, max_payload=maxp)


# 8. the ISP judge (testcases.c:18-37) on long data: (n, max_payload, data bytes, kernel)
ISP_WORLDS = [(8, 1008, 992, 1), (17, 4096, 4080, 0), (17, 368, 352, 0)]
ISP_SUBCASES = ("equal", "last-byte", "high-first-byte", "one-larger-first", "embedded-nul", "data-longer", "data-shorter",
                "empty-data")
# the decision each sub-case comes to by the rule (strcmp, then the signed first byte); the oracle is checked against
# it on the CPU (tests/test_iar_payloads_oracle.py), the device against the oracle
ISP_DECISION = {"equal": 1, "last-byte": 1, "high-first-byte": 0, "one-larger-first": 0, "embedded-nul": 1,
                "data-longer": 1, "data-shorter": 1, "empty-data": 0}


def isp_case(n, dl, name, seed=5):
    """-> (proposals, the ranks' strings): one proposal from rank 3 of dl data bytes (printable ASCII unless the
    sub-case says otherwise); what each sub-case decides is the oracle's to say"""
    rng = np.random.default_rng(seed + dl)
    data = bytearray(rng.integers(0x21, 0x7e, size=dl, dtype=np.uint8).tobytes())  # (0x7e itself never drawn: + 1 stays ASCII)
    text = data.decode("ascii")
    isp = [text] * n
    if name == "equal":
        pass
    elif name == "last-byte":
        isp = [text[:-1] + chr(data[-1] + 1)] * n
    elif name == "high-first-byte":
        data[0] = 0xC3
    elif name == "one-larger-first":
        isp[n - 1] = chr(data[0] + 1) + text[1:]
    elif name == "embedded-nul":
        data[dl // 2] = 0
        isp = [text[:dl // 2]] * n
    elif name == "data-longer":
        isp = [text[:-1]] * n
    elif name == "data-shorter":
        isp = [text + "x"] * n
    elif name == "empty-data":
        data = bytearray()
    else:
        raise ValueError(name)
    return [(3, 103, bytes(data))], isp


# the host-service path (tests/test_gpu_host.py): (n, max_payload, lens, pool, pend_hbm, seed); every rank submits
# one proposal of each length.  {0, 1, 96, 97, 240} cross the command doorbell's limit (kLLCmdSlot) and the bell's
# (kBellChunks) and fill a 256-byte slot; {48 .. 4080} cross the staged chunks and fill a default one
PPM[13] = 24000
HOST_SMALL, HOST_LARGE = (0, 1, 96, 97, 240), (48, 49, 353, 1000, 4080)
HOST_CASES = [(8, 256, HOST_SMALL, 1, False, 1), (8, 256, HOST_SMALL, 4, False, 1),
              (16, 256, HOST_SMALL, 1, False, 1), (16, 256, HOST_SMALL, 4, False, 1), (16, 256, HOST_SMALL, 4, True, 1),
              (13, 4096, HOST_LARGE, 1, False, 1), (13, 4096, HOST_LARGE, 4, False, 1)]


def host_case(n, lens, seed):
    """-> (proposals, oracle judge cfg, its keepalive, ppm): the seeded hash judge, which the test's callback evaluates"""
    cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_HASH, seed=seed, ppm=PPM[n])
    return iar_sets.mixed_props(n, len(lens), lens, seed), cfg, keep, PPM[n]

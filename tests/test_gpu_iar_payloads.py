"""GPU parity of the proposal (IAR) paths at every payload size they carry.

The rest of the suite submits proposals of at most 22 data bytes: 3 or 4 chunks.  Here a proposal has 0 .. 4080
bytes (tests/iar_payload_cases.py: the lengths on both sides of every chunk count at which the engine takes another
path), uniform launches that put the program's largest message on such a boundary and mixed ones in which messages
carried by the ring and by the doorbell share edges and pool slots are reused with changing lengths.  Every run is
compared with the oracle (orc.iar) per (origin, pid) as exact multisets of judge calls, actions, decision pickups
and results, with the lengths the records carry (iar_sets.check_events), the per-rank counters, and the kernel
that ran.  The device IAR program logs no payload bytes: beyond what the ISP judge reads (below), the proposal's
bytes are compared through the host-service path (test_gpu_host.py), which shares the forwarding code.
"""
import os
from collections import Counter

import pytest

import iar_payload_cases as pc
import iar_sets
import pyoracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rlo():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rlo as _rlo

    return _rlo


def _cap(ev, n):
    """a log capacity from the oracle's event count: the most records any rank writes, and some room"""
    per = Counter(e[1] for e in ev)
    return max(per.values()) + 16


def _world(rlo, c):
    if c.pull in (None, ""):
        return rlo.World(c.n, **c.world)
    os.environ["RLO_PULL"] = c.pull  # (read at creation, as test_gpu_engine.py::test_storm_large_groups sets it)
    try:
        return rlo.World(c.n, **c.world)
    finally:
        del os.environ["RLO_PULL"]


def _report(cid, info, ms):
    print("iar payload case %s: last_kernel %d waves %d nsmall %d pull %d pend_hbm %d ll_ok %d kernel %.2f ms" %
          (cid, info["last_kernel"], info["waves"], info["nsmall"], info["pull"], info["pend_hbm"], info["ll_ok"], ms))


def _run(rlo, w, c, props, cfg, program_kw, kernel, cid=None):
    """one launch of props in world w against the oracle; returns the oracle's events"""
    ev = iar_sets.oracle_events(c.n, props, cfg, c.pool)
    cap = _cap(ev, c.n)
    w.program_iar(props, log=True, log_cap=cap, pool=c.pool, **program_kw)
    ms = w.run()
    info = dict(w.info_now())
    st = w.stats()
    logs = {r: w.log(r, cap=cap) for r in range(c.n)}
    _report(cid or c.id, info, ms)
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    assert info["last_kernel"] == kernel, info
    iar_sets.check_events(logs, c.n, props, cfg, c.pool, stats=st, ev=ev)
    return ev


@pytest.mark.parametrize("cid", [c.id for c in pc.CASES])
def test_iar_payloads_match_oracle(rlo, cid):
    c = pc.BY_ID[cid]
    props = c.proposals()
    cfg, keep = c.oracle_cfg()
    c.check_inputs(props, iar_sets.oracle_events(c.n, props, cfg, c.pool))  # the inputs, on the oracle alone
    with _world(rlo, c) as w:
        if c.waves is not None:
            assert w.info["waves"] == c.waves, w.info
        if c.nsmall is not None:
            assert w.info["nsmall"] == c.nsmall, w.info
        if c.pull is not None:  # pulled by default: large proposals must still arrive whole (they are pushed)
            assert w.info["pull"] == (0 if c.pull == "0" else 1), w.info
        if c.world.get("pend_hbm"):
            assert w.info["pend_hbm"] == 1, w.info
        _run(rlo, w, c, props, cfg, c.program_kw(rlo.abi), c.kernel)


def _forge_bus(blob):
    import re

    m = re.search(rb"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-9]", blob)
    assert m, "no PCI bus id in the exported blob"
    return blob[:m.start()] + b"ffff:ff:1f.7" + blob[m.end():]


@pytest.mark.parametrize("forged", [False, True], ids=["agent", "system"])
@pytest.mark.parametrize("cid", [c[0] for c in pc.PART_CASES])
def test_iar_payloads_two_parts(rlo, cid, forged):
    """two parts in one process; forged: every part sees its peer "on another GPU" (as
    test_gpu_send_storm.py::test_parts), so both store at system scope"""
    from rlo import sharded

    bounds, c = pc.part_case(cid)
    props = c.proposals()
    cfg, keep = c.oracle_cfg()
    ev = iar_sets.oracle_events(c.n, props, cfg, c.pool)
    c.check_inputs(props, ev)
    cap = _cap(ev, c.n)

    def forge(p, blobs):
        return [b if q == p else _forge_bus(b) for q, b in enumerate(blobs)]

    spec = dict(kind="iar", props=props, log=True, log_cap=cap, pool=c.pool, **c.program_kw(rlo.abi))
    (st, logs, ms), rcs = sharded.run_inprocess(c.n, bounds, spec, max_payload=c.world["max_payload"], uncached=forged,
                                                blobs_for=forge if forged else None)
    print("iar payload case %s-%s: last_kernel %s sys_scope %s kernel ms %s" %
          (cid, "system" if forged else "agent", st["part_last_kernel"], st["part_sys_scope"], ms))
    assert rcs == [0, 0], (st["error"], st["error_aux"])
    assert (st["part_last_kernel"] == c.kernel).all(), st["part_last_kernel"]
    assert (st["part_sys_scope"] == (1 if forged else 0)).all()
    iar_sets.check_events(logs, c.n, props, cfg, c.pool, stats=st, ev=ev)


@pytest.mark.parametrize("n,maxp,dl,kernel", pc.ISP_WORLDS)
def test_iar_isp_judge_on_long_data(rlo, n, maxp, dl, kernel):
    """the ISP judge (testcases.c:18-37: strcmp, then a SIGNED compare of the first bytes) reads the proposal's
    data where the message lies: the hop kernel's LDS copy of all its chunks, the progress kernel's ring slot (a
    proposal this long never travels by doorbell).  Whatever it reads wrong changes a verdict: every sub-case's
    judge calls, with their verdicts, equal the oracle's"""
    c = pc.Case("isp", n, (dl,), 1, kernel, 0, max_payload=maxp)
    with rlo.World(n, max_payload=maxp) as w:
        for name in pc.ISP_SUBCASES:
            props, isp = pc.isp_case(n, dl, name)
            assert len(props[0][2]) == (0 if name == "empty-data" else dl)
            cfg, keep = orc.judge_cfg(orc.ORC_JUDGE_ISP, isp=isp)
            ev = _run(rlo, w, c, props, cfg, {"judge": rlo.abi.RLO_JUDGE_ISP, "isp": isp}, kernel,
                      cid="isp-n%d-%d-%s" % (n, dl, name))
            assert iar_sets.outcomes(ev) == {(3, 103): pc.ISP_DECISION[name]}, name


def test_iar_payload_refusal(rlo):
    """a proposal one byte beyond the slot (16 + dl == max_payload + 1) is refused by the program call and leaves
    the program loaded before it in place; one that fills the slot exactly runs"""
    n, maxp = 8, 1008
    c = pc.Case("refusal", n, (17, 96, 97), 2, 1, 1, max_payload=maxp)
    props = c.proposals()
    cfg, keep = c.oracle_cfg()
    with rlo.World(n, max_payload=maxp) as w:
        _run(rlo, w, c, props, cfg, c.program_kw(rlo.abi), 1, cid="refusal-before")
        with pytest.raises(rlo.RloError, match=r"rlo_program_iar failed.*\[-1\]"):
            w.program_iar([(0, 1, bytes(maxp + 1 - 16))])
        w.run()  # the program loaded before the refusal still runs, and clean
        st = w.stats()
        cap = _cap(iar_sets.oracle_events(n, props, cfg, c.pool), n)
        iar_sets.check_events({r: w.log(r, cap=cap) for r in range(n)}, n, props, cfg, c.pool, stats=st)
        full = pc.Case("refusal-full-slot", n, (maxp - 16,), 1, 1, 1, max_payload=maxp)
        fprops = full.proposals()
        fcfg, fkeep = full.oracle_cfg()
        _run(rlo, w, full, fprops, fcfg, full.program_kw(rlo.abi), 1)

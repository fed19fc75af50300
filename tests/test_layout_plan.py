"""The LDS layout of a part (rlo_layout_plan, host arithmetic: no GPU).

VERDICT r3 "next" 1: the 8-GPU bench world (2,048 ranks, 256 per part) used to size every rank's
pending-proposal table by the WORLD size (N x pool x 16 B of LDS: 64 KiB at N = 2,048), which pushed the
8-wave kernel's staged chunks per message down to 2 and every 64-B message off the small copy path.  The
table now moves to HBM where it would crowd the stage out, and the staged chunk count is never lowered
below a slot's chunks.  The same function sizes every part a GPU creates (rlo_world.cpp plan_lds; there
with the runtime's occupancy answers, tests/test_gpu_scale.py compares the two).
"""
import json
import os

import pytest

import rlo


@pytest.mark.parametrize("gpus", [1, 2, 4, 8])
def test_bench_storm_world_keeps_the_small_path(gpus):
    """bench.py --gpus G: one world of 256 G ranks, 256 per part, 64-B slots"""
    n = 256 * gpus
    for part in range(gpus):
        i = rlo.layout_plan(n, gpus, part, max_payload=64)
        assert i["rank_end"] - i["rank_begin"] == 256
        assert i["waves"] == 8, i
        assert i["nsmall"] == 5, i           # header + 64 B: every storm message on the small copy path
        assert i["ll_ok"] == 1, i            # the latency / iar legs run with doorbells
        assert i["static_lds"] + i["dyn_lds"] <= 160 * 1024
    # the table stays in LDS while it fits beside a full stage, and moves to HBM at 8 GPUs
    assert rlo.layout_plan(256, 1, 0, max_payload=64)["pend_hbm"] == 0
    assert rlo.layout_plan(2048, 8, 0, max_payload=64)["pend_hbm"] == 1


@pytest.mark.parametrize("n,parts", [(2048, 8), (4096, 16), (512, 1)])
def test_pool16_worlds(n, parts):
    """the proposal pool at 16 (N x 16 x 16 B per rank: 512 KiB at N = 2,048) still plans"""
    i = rlo.layout_plan(n, parts, 0, max_payload=32, proposal_pool=16)
    assert i["pend_hbm"] == 1 and i["nsmall"] == 3 and i["proposal_pool"] == 16


@pytest.mark.parametrize("payload", [16, 64, 112, 128, 256, 368, 1024, 4096])
@pytest.mark.parametrize("n,parts", [(64, 1), (256, 1), (500, 1), (1024, 4), (2048, 8)])
def test_nsmall_never_below_the_slot(payload, n, parts):
    """small / medium slots (<= 24 chunks) are staged whole; large slots stage 5 chunks (header + 64 B)"""
    i = rlo.layout_plan(n, parts, 0, max_payload=payload, proposal_pool=2)
    chunks = (16 + ((payload + 15) // 16) * 16) // 16
    full = chunks if chunks <= 24 else 5
    if i["rank_end"] - i["rank_begin"] <= 256:
        assert i["nsmall"] == full, i
    else:  # two rank-workgroups per CU (4 waves, half the LDS each): medium slots may be staged in part,
        # the 4-wave kernel's large-message path takes the rest; a 64-B message and a proposal never
        assert i["waves"] == 4 and min(full, 5) <= i["nsmall"] <= full, i
    if chunks > 8 or i["rank_end"] - i["rank_begin"] > 256:
        assert i["waves"] == 4, i


def test_forced_hbm_tables():
    """RLO_PART_PEND_HBM: the tests' way onto the 8-GPU layout at a smaller N"""
    assert rlo.layout_plan(256, 1, 0, max_payload=64, pend_hbm=True)["pend_hbm"] == 1
    assert rlo.layout_plan(8, 1, 0, max_payload=64, pend_hbm=True)["pend_hbm"] == 1


@pytest.mark.parametrize("gpus", [1, 2, 4, 8])
def test_c5_bulk_worlds_plan(gpus):
    """bench.py's C5 leg: 64 ranks per GPU, 4-KiB slots, bulk messages to 1 MiB.  N x B pending bulk
    receptions per rank (<= kMaxPend = 1,024): at 8 GPUs (512 ranks) the world used to be refused"""
    n = 64 * gpus
    i = rlo.layout_plan(n, gpus, 0, max_payload=4096, bulk_max=1 << 20)
    assert i["waves"] == 4 and i["nsmall"] == 5 and n * i["bulk_slots"] <= 1024
    assert i["bulk_slots"] == 2


def _recorded_plans():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_plan.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", _recorded_plans(), ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c["args"].items())))
def test_plans_as_recorded(case):
    """every field of the plan, and every refusal, as the library answered before the part's regions, the plan and
    the configuration's normalisation each came to one place (tests/golden/gen_layout_plan.py recorded them)"""
    if "refused" in case:
        with pytest.raises(rlo.RloError) as e:
            rlo.layout_plan(**case["args"])
        assert str(e.value) == case["refused"]
    else:
        assert rlo.layout_plan(**case["args"]) == case["plan"]


def test_bulk_slots_auto_beyond_512_ranks():
    assert rlo.layout_plan(1024, 8, 0, max_payload=4096, bulk_max=1 << 20)["bulk_slots"] == 1
    with pytest.raises(rlo.RloError):
        rlo.layout_plan(1024, 8, 0, max_payload=4096, bulk_max=1 << 20, bulk_slots=2)

#!/usr/bin/env python3
"""Record rlo.layout_plan over a grid of configurations into layout_plan.json.

TEST INFRASTRUCTURE ONLY.  The fixture is what the library at the commit BEFORE a change to the host-side
planning (rlo_world.cpp: build_layout, plan_lds, the configuration's normalisation, the info fill) answers:
tests/test_layout_plan.py holds every later library to exactly these dictionaries and these refusals.  Run it
against a build of that commit, never against the change it is to check:

    python tests/golden/gen_layout_plan.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "rootless-coll-mpi-ops_amd"))

import rlo  # noqa: E402

BULK = dict(max_payload=4096, bulk_max=1 << 20)
GRID = [
    dict(n=256, n_parts=1, part=0, max_payload=64),
    dict(n=2048, n_parts=8, part=0, max_payload=64),
    dict(n=2048, n_parts=8, part=7, max_payload=64),
    dict(n=512, n_parts=1, part=0, max_payload=32, proposal_pool=16),
    dict(n=500, n_parts=1, part=0, max_payload=368),
    dict(n=1024, n_parts=4, part=2, max_payload=1024),
    dict(n=8, n_parts=1, part=0, max_payload=64, pend_hbm=True),
    dict(n=64, n_parts=1, part=0, **BULK),
    dict(n=512, n_parts=8, part=3, **BULK),
    dict(n=1024, n_parts=8, part=0, **BULK),
    dict(n=64, n_parts=1, part=0, movers=32, **BULK),
    dict(n=64, n_parts=2, part=1, movers=2, bulk_slots=4, **BULK),
    dict(n=256, n_parts=1, part=0, max_payload=64, ring_slots=100),
    dict(n=256, n_parts=1, part=0, max_payload=64, cus=304),
    dict(n=64, n_parts=1, part=0, cus=304, **BULK),
    dict(n=16, n_parts=1, part=0, max_payload=0),        # the default payload
    dict(n=16, n_parts=1, part=0, max_payload=1),        # rounded up to a chunk
    dict(n=300, n_parts=3, part=1, max_payload=113),     # uneven parts, the first slot past the 8-wave path
    dict(n=2, n_parts=1, part=0, max_payload=64),
    dict(n=4096, n_parts=16, part=15, max_payload=32, proposal_pool=16),
    # what may be refused: the slot header's 16-bit length, the proposal pool, the part index, the world size
    dict(n=64, n_parts=1, part=0, max_payload=65520),
    dict(n=64, n_parts=1, part=0, max_payload=65521),
    dict(n=64, n_parts=1, part=0, max_payload=64, proposal_pool=3),
    dict(n=64, n_parts=1, part=0, max_payload=64, proposal_pool=32),
    dict(n=64, n_parts=2, part=2, max_payload=64),
    dict(n=1, n_parts=1, part=0, max_payload=64),
    dict(n=64, n_parts=1, part=0, movers=1, **BULK),
]


def main():
    out = []
    for args in GRID:
        try:
            out.append({"args": args, "plan": rlo.layout_plan(**args)})
        except rlo.RloError as e:
            out.append({"args": args, "refused": str(e)})
    path = os.path.join(HERE, "layout_plan.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in out) + "\n]\n")
    print("wrote %s: %d plans, %d refusals" % (os.path.relpath(path, REPO), sum("plan" in c for c in out),
                                               sum("refused" in c for c in out)), file=sys.stderr)


if __name__ == "__main__":
    main()

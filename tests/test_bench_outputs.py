"""bench.py's plain run and --dump-outputs: the timed storm alone, its result line, and the per-rank results of the
last timed step written as DIR/<name>.npy (float64), checked against the oracle's expectation of the same storm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bcast_delivered", "bcast_sum_lo32", "bcast_sum_hi32", "originated", "error", "unmarked_slots")


def test_dump_outputs_writes_exact_float64(tmp_path):
    """64-bit checksums leave as two 32-bit halves, each exact in float64"""
    import bench

    sums = np.array([0xFFFFFFFFFFFFFFFF, 1, (1 << 40) + 5, 0], dtype=np.uint64)
    st = {f: np.arange(4, dtype=np.uint64) for f in bench._OUTPUT_FIELDS}
    st["bcast_sum"] = sums
    bench.dump_outputs(str(tmp_path), st, 1, 0)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float64 and a.shape == (4,) for a in got.values())
    back = (got["bcast_sum_hi32"].astype(np.uint64) << np.uint64(32)) | got["bcast_sum_lo32"].astype(np.uint64)
    assert np.array_equal(back, sums)
    assert np.array_equal(got["bcast_delivered"], np.arange(4.0))
    # a part of a sharded world names its files after itself
    bench.dump_outputs(str(tmp_path / "p"), st, 2, 1)
    assert sorted(os.listdir(tmp_path / "p")) == sorted(n + ".part1.npy" for n in NAMES)


@pytest.mark.gpu
def test_plain_run_is_the_timed_storm_alone_and_dumps_its_outputs(tmp_path):
    import pyoracle as orc

    n, k, ln, steps = 64, 4096, 64, 3
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        "1", "--ranks", str(n), "--k", str(k), "--len", str(ln), "--dump-outputs", out], cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.strip()]
    assert len(lines) == 1, lines  # the result line is the only stdout
    line = json.loads(lines[0])
    assert line["metric"] == "rootless bcast msgs/s" and line["unit"] == "msgs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == steps and line["verified"] is True
    assert line["ms_per_step"] > 0
    # value is bcasts per second of the timed steps: k bcasts in ms_per_step, which the line rounds to 1 us
    assert line["value"] == pytest.approx(k / (line["ms_per_step"] * 1e-3), rel=0.0006 / line["ms_per_step"] + 1e-6)
    # nothing beside the timed storm ran
    for leg in ("p50_us", "decisions_per_s", "payload_sizes", "small_worlds", "bulk", "c5_mixed", "dropin_api",
                "cpu_baseline"):
        assert leg not in line, leg
    assert line["roofline"]["traffic"] is None
    got = {f: np.load(os.path.join(out, f + ".npy")) for f in NAMES}
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in NAMES)
    assert all(a.dtype == np.float64 and a.shape == (n,) for a in got.values())
    want = orc.storm_expected(n, 0x5EED, k, ln)
    assert np.array_equal(got["bcast_delivered"].astype(np.int64), want["count"])
    sums = (got["bcast_sum_hi32"].astype(np.uint64) << np.uint64(32)) | got["bcast_sum_lo32"].astype(np.uint64)
    assert np.array_equal(sums, np.asarray(want["sum"], dtype=np.uint64))
    assert int(got["originated"].sum()) == k and not got["error"].any() and not got["unmarked_slots"].any()

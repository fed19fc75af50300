"""What the tests of the three send programs (rlo_program_send, _send_bulk, _send_storm) share: the struct-against-
header check of the host tests, and the workloads, expected values and helpers of the GPU tests.

Expected values never come from the engine: payload bytes are the seeded NumPy source, checksums pyoracle.msg_checksum
summed over what a rank must receive, counts k minus the rank's own."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FILL = 0xA5  # what the GPU tests pre-fill dst with: the bytes that must stay unwritten are checked too
TAG_BCAST = 0
MASK64 = (1 << 64) - 1


def header_layout(tmp_path, cname, py, macros=()):
    """sizeof and every field offset of the C struct `cname` of rlo_hip.h, asserted equal to the ctypes mirror `py`;
    returns {"sizeof": its size, macro: its value (unsigned) for each of `macros`}"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rlo_hip.h"', 'int main(void) {',
             'printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%u\\n", %s);' % (m, m) for m in macros]
    lines += ['printf(".%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname) for fname, _ in py._fields_]
    lines += ['return 0;', '}']
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert int(got["." + fname]) == getattr(py, fname).offset, fname
    return {key: int(v) for key, v in got.items() if not key.startswith(".")}


@pytest.fixture(scope="module")
def rlo():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rlo as _rlo

    return _rlo


def gen(n, slot, k, seed, origins=None, storm=False):
    """a seeded workload: origins (any rank, any mix), lengths from {1, 15, 16, 17, slot - 1, slot} within [1, slot],
    and k x slot source bytes.  storm: large slots add {64, 65, 368, 369, 1008, 1024, 1025} -- the staged 5 chunks,
    the small copy path's 24 chunks, the hop kernel's limit --, and every boundary occurs at least once"""
    rng = np.random.default_rng(seed)
    if origins is None:
        origins = rng.integers(0, n, k)
    origins = np.asarray(origins, dtype=np.int32)
    pool = {1, 15, 16, 17, slot - 1, slot}
    if storm and slot > 112:
        pool |= {64, 65, 368, 369, 1008, 1024, 1025}
    choices = sorted(x for x in pool if 1 <= x <= slot)
    lens = rng.choice(choices, len(origins)).astype(np.uint32)
    if storm:
        lens[:len(choices)] = choices[:len(origins)]
    src = rng.integers(0, 256, (len(origins), slot), dtype=np.uint8)
    return origins, lens, src


def expected(n, origins, lens, src):
    """(dst bytes [n][k][slot], deliveries [n], originated [n], checksum [n]) a correct run leaves"""
    import pyoracle as orc

    k, slot = src.shape
    col = np.arange(slot)[None, :]
    ln = lens.astype(np.int64)[:, None]
    msg = np.where(col < ln, src, np.where(col < (ln + 15) // 16 * 16, 0, FILL)).astype(np.uint8)
    want = np.broadcast_to(msg, (n, k, slot)).copy()
    want[origins, np.arange(k)] = FILL  # the origin's own place is not written
    cs = [orc.msg_checksum(int(origins[i]), i, TAG_BCAST, bytes(src[i, :lens[i]])) for i in range(k)]
    total = sum(cs) & MASK64
    own_sum = [0] * n
    for i in range(k):
        own_sum[origins[i]] += cs[i]
    sums = np.array([(total - own_sum[r]) & MASK64 for r in range(n)], dtype=np.uint64)
    own = np.bincount(origins, minlength=n)
    return want, k - own, own, sums


def check(st, got, n, origins, lens, src):
    want, cnt, own, sums = expected(n, origins, lens, src)
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    assert np.array_equal(st["bcast_delivered"].astype(np.int64), cnt)
    assert np.array_equal(st["originated"].astype(np.int64), own)
    if not np.array_equal(got, want):
        r, i, b = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("rank %d message %d (origin %d, len %d) byte %d: got 0x%02x, want 0x%02x; %d bytes differ" %
                             (r, i, origins[i], lens[i], b, got[r, i, b], want[r, i, b], int((got != want).sum())))
    assert np.array_equal(st["bcast_sum"], sums)


def forge_bus(blob):
    """the exported blob of a part, as if the part were on another GPU"""
    m = re.search(rb"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-9]", blob)
    assert m, "no PCI bus id in the exported blob"
    return blob[:m.start()] + b"ffff:ff:1f.7" + blob[m.end():]


def latency_runs_clean(w):
    w.program_latency(16, 64)
    w.run()
    st = w.stats()
    assert (st["error"] == 0).all() and int(st["originated"].sum()) == 16

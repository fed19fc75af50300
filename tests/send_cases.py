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


def launch_send(w, origins, lens, src, dst=None, **kw):
    """one launch on device buffers made here (dst pre-filled with 0xA5): the hop kernel ran, no rank erred;
    returns (stats, dst bytes [n_local][k][slot])"""
    import torch

    k, slot = src.shape
    s = torch.from_numpy(src.reshape(-1)).cuda()
    if dst is None:
        dst = torch.empty(w.n_local * k * slot, dtype=torch.uint8, device="cuda")
    d = dst[:w.n_local * k * slot]
    d.fill_(FILL)
    torch.cuda.synchronize()
    w.program_send(origins, s, d, slot, lens=lens, **kw)
    w.run()
    assert w.info_now()["last_kernel"] == 1
    st = w.stats()
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    return st, d.cpu().numpy().reshape(w.n_local, k, slot)


def launch_send_storm(w, origins, lens, src, rank_stride=0, **kw):
    """one launch on device buffers made here (dst pre-filled with 0xA5): the progress kernel ran, no rank erred;
    returns (stats, dst bytes [n_local][rank_stride or k * slot])"""
    import torch

    k, slot = src.shape
    rs = rank_stride or k * slot
    s = torch.from_numpy(src.reshape(-1)).cuda()
    d = torch.full((w.n_local * rs,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w.program_send_storm(origins, s, d, slot, lens=lens, rank_stride=rank_stride, **kw)
    w.run()
    assert w.info_now()["last_kernel"] == 0
    st = w.stats()
    assert (st["error"] == 0).all(), (st["error"], st["error_aux"])
    return st, d.cpu().numpy().reshape(w.n_local, rs)


def check_trees_fifo(w, n, origins, lens):
    """every rank's log of a logged launch of the send or the storm send program (log_cap = k): one delivery record
    per message of another rank's, without a payload copy, naming the message's origin and length; `from` is the
    rank's parent in the origin's tree (pyoracle.tree); an origin's messages arrive in the order it sent them"""
    import bcast_length_cases as bc
    import pyoracle as orc

    org, ln, k = np.asarray(origins, dtype=np.int64), np.asarray(lens, dtype=np.int64), len(origins)
    parent = np.stack([orc.tree(n, o)[0] for o in range(n)]).astype(np.int64)  # [origin][rank]
    for r in range(n):
        recs = bc.log_arrays(w, r, k, payload=False)[0].astype(np.int64)
        assert len(recs) == k - int((org == r).sum()), (r, len(recs))
        kind_tag, origin, frm, ident, rlen, pidx = (recs[:, c] for c in (0, 1, 2, 3, 4, 7))
        assert ((kind_tag & 0xffff) == (1 | TAG_BCAST << 8)).all() and (pidx == 0xFFFFFFFF).all(), r
        assert (ident < k).all(), (r, ident.max())
        assert (origin == org[ident]).all() and (origin != r).all() and (rlen == ln[ident]).all(), r
        bad = np.nonzero(frm != parent[origin, r])[0]
        assert bad.size == 0, (r, int(origin[bad[0]]), int(ident[bad[0]]), int(frm[bad[0]]))
        by = np.argsort(origin, kind="stable")  # per-origin FIFO: an origin's records, in log order, ascend in id
        o_s, i_s = origin[by], ident[by]
        bad = np.nonzero((o_s[1:] == o_s[:-1]) & (i_s[1:] <= i_s[:-1]))[0]
        assert bad.size == 0, (r, int(o_s[bad[0] + 1]), int(i_s[bad[0] + 1]))


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

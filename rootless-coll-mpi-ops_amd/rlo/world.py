"""Python host mirror of the device engine (librlo_hip.so).

World(n) hosts n virtual ranks on one MI355X (one persistent workgroup each).
Programs map the reference's application loops onto the device:

  storm()    -- K bcasts from random originators: RLO_msg_new_bc + RLO_bcast_gen at the
                originator, RLO_make_progress_all + RLO_user_pickup_next everywhere
                (rootless_ops.c:311, :1581, :538, :938; testcases.c:638-697)
  latency()  -- one bcast at a time (test_gen_bcast style, testcases.c:59-108)
  iar()      -- RLO_submit_proposal / vote / decision (rootless_ops.c:668-917)
  send()     -- bcasts of the caller's own device buffers, device memory to device memory (program_send,
                bcast_tensor; the hop kernel only)
  send_bulk() -- the same for large buffers in a world with bulk messages: closed-loop bulk bcasts read from and
                written to the caller's device buffers by the mover workgroups (program_send_bulk; bcast_tensor of a
                bulk world)
  send_storm() -- the same at storm rate: open-loop bcasts from any ranks in any mix on the progress kernel, small
                and medium messages up to max_payload (program_send_storm; bcast_rows)
  decide()   -- iar() on the caller's own device buffers: proposal data, each rank's verdict table, the data every
                judging rank received and every rank's decisions all in device memory (program_decide, decide_rows;
                the hop kernel only, worlds of at most 16 ranks)
"""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import check


class World:
    """A world of n ranks.  World(n) hosts all of them on one GPU; World.part(...) creates one
    part of a sharded world (export() -> exchange blobs -> connect(blobs))."""

    def __init__(self, n, max_payload=4096, ring_slots=0, device=-1, _part=None, bulk_max=0, bulk_slots=0, movers=0,
                 proposal_pool=0, pend_hbm=False, one_xcd=False):
        """bulk_max > 0: messages longer than max_payload (up to bulk_max bytes) are bulk messages --
        announced through the rings, moved by `movers` mover workgroups (0 = auto) between per-rank
        heaps of bulk_slots slots per origin (rlo_hip.h).  proposal_pool: pending entries per origin
        = the most own proposals a rank can keep in flight (power of two <= 16; 0 = 2).  pend_hbm: the
        pending-proposal tables in HBM whatever N (the 8-GPU world's layout, rehearsed at a smaller N).
        one_xcd (no bulk, as many ranks as one XCD holds: <= 256): cached rings and every rank-wave of the hop kernel on one XCD, hand-offs
        through its L2 (RLO_PART_ONE_XCD); only the hop kernel's programs run in such a world."""
        self.lib = L.load()
        h = ctypes.c_void_p()
        if _part is None:
            cfg = L.WorldCfg(n, max_payload, ring_slots, device, bulk_max, bulk_slots, movers, proposal_pool,
                             (L.RLO_PART_PEND_HBM if pend_hbm else 0) | (L.RLO_PART_ONE_XCD if one_xcd else 0))
            check(self.lib.rlo_world_create(ctypes.byref(cfg), ctypes.byref(h)), "rlo_world_create")
        else:
            n_parts, part, begin, flags = _part
            self._pb = None
            pb = None
            if begin is not None:
                self._pb = (ctypes.c_int32 * (n_parts + 1))(*begin)
                pb = ctypes.cast(self._pb, ctypes.c_void_p)
            cfg = L.PartCfg(n, n_parts, part, pb, max_payload, ring_slots, device, flags, bulk_max, bulk_slots, movers,
                            proposal_pool)
            check(self.lib.rlo_part_create(ctypes.byref(cfg), ctypes.byref(h)), "rlo_part_create")
        self.h = h
        self.n = n
        self.device = device
        self._query()
        self._lat_rounds = 0

    @classmethod
    def part(cls, n, n_parts, part, part_begin=None, max_payload=4096, ring_slots=0, device=-1, uncached=False,
             bulk_max=0, bulk_slots=0, movers=0, proposal_pool=0, chunked=False, pend_hbm=False):
        """pend_hbm: the pending-proposal tables in HBM whatever N (the layout of the 8-GPU world's parts,
        rehearsed at a smaller N)"""
        return cls(n, max_payload, ring_slots, device,
                   _part=(n_parts, part, part_begin, (L.RLO_PART_UNCACHED if uncached else 0) |
                          (L.RLO_PART_CHUNKED if chunked else 0) | (L.RLO_PART_PEND_HBM if pend_hbm else 0)),
                   bulk_max=bulk_max,
                   bulk_slots=bulk_slots, movers=movers, proposal_pool=proposal_pool)

    def _query(self):
        info = L.WorldInfo()
        check(self.lib.rlo_world_query(self.h, ctypes.byref(info)), "rlo_world_query")
        self.info = {f: getattr(info, f) for f, _ in L.WorldInfo._fields_}
        self.rank_begin, self.rank_end = self.info["rank_begin"], self.info["rank_end"]
        self.n_local = self.rank_end - self.rank_begin

    def info_now(self):
        """rlo_world_query now (self.info is the answer at creation / connection): e.g. last_kernel after a launch"""
        self._query()
        return self.info

    def export(self):
        buf = ctypes.create_string_buffer(L.RLO_PART_BLOB_BYTES)
        check(self.lib.rlo_part_export(self.h, buf, L.RLO_PART_BLOB_BYTES), "rlo_part_export")
        return buf.raw

    def connect(self, blobs):
        joined = b"".join(blobs)
        check(self.lib.rlo_part_connect(self.h, joined, len(blobs)), "rlo_part_connect")
        self._query()

    def reset(self, stream=None):
        check(self.lib.rlo_reset(self.h, stream), "rlo_reset")

    def import_part(self, blob, q):
        """rlo_part_import: map part q's regions now (connect() then skips q)"""
        check(self.lib.rlo_part_import(self.h, blob, q), "rlo_part_import")

    def staged_connect(self, blobs, barrier, bcast=None):
        """connect in n_parts stages: in stage k every other part imports part k's regions while part k imports
        nothing, then barrier() (rlo_hip.h rlo_part_import).  bcast(blob or None, k) -> part k's blob: part k
        exports its handles afresh at the start of its stage and every part imports those (a handle exported
        before its exporter imported anything).  An import error is raised after the last stage, so every part
        still joins every barrier"""
        err = None
        me = self.info["part"]
        for k, b in enumerate(blobs):
            if bcast is not None:
                b = bcast(self.export() if k == me else None, k)
            if k != me and err is None:
                try:
                    self.import_part(b, k)
                except Exception as e:  # noqa: BLE001 - re-raised below
                    err = e
            barrier()
        if err is not None:
            raise err
        self.connect(blobs)

    def close_imports(self):
        """rlo_part_close_imports: drop the hipIpc imports of the peers' regions (the part can no longer launch)"""
        if self.h:
            check(self.lib.rlo_part_close_imports(self.h), "rlo_part_close_imports")

    def close(self):
        if self.h:
            self.lib.rlo_world_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ programs
    def program_storm(self, k, length, seed=0x5EED, window=64, log=False, hist=False, log_cap=0, prof=False,
                      len_max=0, order=L.RLO_ORDER_RANDOM):
        """len_max > length: mixed sizes (piecewise log-uniform per bcast); order RLO_ORDER_SLOTS: bcast b
        originates at rank b % n (every rank originates in every slot of n bcasts)."""
        flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_HIST if hist else 0) | (L.RLO_FLAG_PROF if prof else 0)
        cfg = L.StormCfg(seed, k, length, window, flags, log_cap, len_max, order)
        check(self.lib.rlo_program_storm(self.h, ctypes.byref(cfg)), "rlo_program_storm")

    def program_latency(self, rounds, length, seed=0x5EED, hist=False, log=False, prof=False, timeline=False):
        flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_HIST if hist else 0) | (L.RLO_FLAG_PROF if prof else 0)
        flags |= L.RLO_FLAG_TIMELINE if timeline else 0
        check(self.lib.rlo_program_latency(self.h, rounds, length, seed, flags), "rlo_program_latency")
        self._lat_rounds = rounds

    def program_iar(self, proposals, judge=L.RLO_JUDGE_APPROVE, mask=None, isp=None, seed=0, ppm=0, log=False,
                    log_cap=0, prof=False, pool=1):
        """proposals: list of (origin, pid, data bytes) in per-origin submission order; every rank keeps
        up to `pool` of its own in flight (the proposal pool, <= the world's proposal_pool)."""
        origin = np.array([p[0] for p in proposals], dtype=np.int32)
        pid = np.array([p[1] for p in proposals], dtype=np.int32)
        blob = np.frombuffer(b"".join(p[2] for p in proposals) or b"\0", dtype=np.uint8).copy()
        dlen = np.array([len(p[2]) for p in proposals], dtype=np.uint32)
        doff = (np.cumsum(dlen) - dlen).astype(np.uint32)
        self._keep = [origin, pid, blob, dlen, doff]
        cfg = L.IarCfg()
        cfg.judge_kind = judge
        cfg.judge_ppm = ppm
        cfg.judge_seed = seed
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8))
            self._keep.append(m)
            cfg.judge_mask = m.ctypes.data
        if isp is not None:
            cfg.judge_isp = b"".join(s.encode() + b"\0" for s in isp)
            self._keep.append(cfg.judge_isp)
        cfg.flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_PROF if prof else 0)
        cfg.log_cap = log_cap
        cfg.pool = pool
        self._keep.append(cfg)
        d = lambda a: a.ctypes.data
        check(self.lib.rlo_program_iar(self.h, ctypes.byref(cfg), len(proposals), d(origin), d(pid), d(blob), d(doff),
                                       d(dlen)), "rlo_program_iar")

    def program_send(self, origins, src, dst, slot, lens=None, ordered=False, log=False, hist=False, log_cap=0):
        """rlo_program_send: message i (len(origins) of them) is a bcast from rank origins[i] of the lens[i] (None: slot)
        bytes at src + i * slot, DEVICE memory; local rank lr's copy lands at dst + (lr * k + i) * slot, DEVICE memory.
        src / dst: anything with data_ptr() and numel() * element_size() (a torch tensor), or an (int pointer, nbytes)
        pair; src holds k * slot bytes, dst n_local * k * slot, both 16-B aligned.  ordered: one message in flight (a
        total order; latencies_ticks() as for the latency program).  Only the hop kernel runs this program: a launch
        that cannot run it raises."""
        flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_HIST if hist else 0) | (L.RLO_SEND_ORDERED if ordered else 0)
        cfg, self._keep = _send_cfg("send", origins, src, dst, slot, lens, 0, 0, flags, log_cap, self.n_local)
        check(self.lib.rlo_program_send(self.h, ctypes.byref(cfg)), "rlo_program_send")
        self._lat_rounds = cfg.k if ordered else 0

    def program_send_bulk(self, origins, src, dst, stride, lens=None, rank_stride=0, log=False, hist=False, log_cap=0):
        """rlo_program_send_bulk (worlds with bulk messages): message i (len(origins) of them, closed loop) is a bulk
        bcast from rank origins[i] of the lens[i] (None: stride) bytes at src + i * stride, DEVICE memory; local rank
        lr's copy lands at dst + lr * rank_stride + i * stride (rank_stride 0: k * stride), DEVICE memory.  src / dst
        as for program_send, 16-B aligned; src is read for round16(lens[i]) bytes of each message.  latencies_ticks()
        as for a bulk round of the latency program."""
        flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_HIST if hist else 0)
        cfg, self._keep = _send_cfg("send_bulk", origins, src, dst, stride, lens, rank_stride, 0, flags, log_cap, self.n_local)
        check(self.lib.rlo_program_send_bulk(self.h, ctypes.byref(cfg)), "rlo_program_send_bulk")
        self._lat_rounds = cfg.k

    def program_send_storm(self, origins, src, dst, slot, lens=None, rank_stride=0, window=64, log=False, hist=False,
                           log_cap=0, prof=False):
        """rlo_program_send_storm (worlds without bulk messages): message i (len(origins) of them, open loop, per-origin
        FIFO) is a bcast from rank origins[i] of the lens[i] (None: slot) bytes at src + i * slot, DEVICE memory; local
        rank lr's copy lands at dst + lr * rank_stride + i * slot (rank_stride 0: k * slot), DEVICE memory.  slot: a
        multiple of 16, at most the world's max_payload.  src / dst as for program_send, 16-B aligned; src is read for
        round16(lens[i]) bytes of each message.  The progress kernel's storm-send instantiation runs it."""
        flags = (L.RLO_FLAG_LOG if log else 0) | (L.RLO_FLAG_HIST if hist else 0) | (L.RLO_FLAG_PROF if prof else 0)
        cfg, self._keep = _send_cfg("send_storm", origins, src, dst, slot, lens, rank_stride, window, flags, log_cap,
                                    self.n_local)
        check(self.lib.rlo_program_send_storm(self.h, ctypes.byref(cfg)), "rlo_program_send_storm")
        self._lat_rounds = 0

    def program_decide(self, origins, src, dst, decision, slot, lens=None, verdict=None, log=False, log_cap=0):
        """rlo_program_decide (worlds of at most 16 ranks without bulk messages): proposal i (len(origins) of them, pid =
        i) is submitted by rank origins[i] with the lens[i] (None: slot) bytes at src + i * slot, DEVICE memory, each
        rank's proposals in list order, one in flight.  Local rank lr declines proposal i iff verdict[lr * k + i] == 0
        (DEVICE bytes; None approves everything).  A rank that judges proposal i writes the data it received to
        dst + (lr * k + i) * slot, and every rank the decision (0 / 1) to decision[lr * k + i], both DEVICE memory.
        src / dst / verdict / decision: as program_send's buffers; src holds k * slot bytes, dst n_local * k * slot (both
        16-B aligned), verdict and decision n_local * k.  slot: a multiple of 16, 16 .. 992, 16 + slot within the
        world's max_payload.  Only the hop kernel runs this program: a launch that cannot run it raises."""
        cfg, self._keep = _decide_cfg(origins, src, dst, decision, slot, lens, verdict, L.RLO_FLAG_LOG if log else 0,
                                      log_cap, self.n_local)
        check(self.lib.rlo_program_decide(self.h, ctypes.byref(cfg)), "rlo_program_decide")
        self._lat_rounds = 0

    def decide_rows(self, origins, t, verdict=None, stream=None):
        """One consensus round per row of the contiguous CUDA tensor t of shape [k, ...]: row i (at most 992 bytes, and
        16 bytes less than the world's max_payload) is rank origins[i]'s proposal in a one-part world of at most 16
        ranks, all k in ONE decide launch on torch's current stream (or `stream`, a raw hipStream_t).  verdict: a uint8
        CUDA tensor [n, k] -- rank r declines proposal i iff verdict[r, i] == 0 (its own proposals' entries are not
        read) -- or None: everything is approved.  Returns (decided, rows): decided uint8 [n, k], 1 where rank r
        learnt that proposal i was approved; rows of shape [n, k, ...] and t's dtype, rows[r, i] = t[i] where
        decided[r, i] == 1 (the origin's own row included, copied in from t here) and zero elsewhere.  A row that is no
        multiple of 16 bytes goes through a padded staging copy: t is never read past its end."""
        import torch

        if self.n_local != self.n:
            raise ValueError("decide_rows: one-part worlds only")
        if not (t.is_cuda and t.is_contiguous()) or t.dim() < 1:
            raise ValueError("decide_rows: a contiguous tensor [k, ...] in device memory")
        origin = np.asarray(origins, dtype=np.int64).reshape(-1)
        k, n = int(t.shape[0]), self.n
        if origin.size != k or (k and (origin.min() < 0 or origin.max() >= n)):
            raise ValueError("decide_rows: one origin in [0, %d) per row" % n)
        row = t[0].numel() * t.element_size() if k else 0
        slot = decide_slot(row, self.info["slot_stride"] - 16)
        if verdict is not None and not (verdict.is_cuda and verdict.is_contiguous() and verdict.dtype == torch.uint8 and
                                        tuple(verdict.shape) == (n, k)):
            raise ValueError("decide_rows: verdict is a contiguous uint8 tensor [%d, %d] in device memory" % (n, k))
        if k == 0:
            return torch.zeros((n, 0), dtype=torch.uint8, device=t.device), t.unsqueeze(0).repeat((n,) + (1,) * t.dim())
        flat = t.reshape(k, -1).view(torch.uint8)
        if slot == row and flat.data_ptr() % 16 == 0:
            src = flat
        else:  # a padded staging copy: t is never read past its end
            src = torch.zeros((k, slot), dtype=torch.uint8, device=t.device)
            src[:, :row].copy_(flat)
        dst = torch.zeros((n, k, slot), dtype=torch.uint8, device=t.device)
        decided = torch.zeros((n, k), dtype=torch.uint8, device=t.device)
        self.program_decide(origin, src, dst, decided, slot, lens=None if slot == row else [row] * k, verdict=verdict)
        if stream is None:
            stream = torch.cuda.current_stream(t.device).cuda_stream
        self.launch(stream=stream)
        self.wait()
        out = dst[:, :, :row].contiguous()
        out[torch.as_tensor(origin, device=t.device), torch.arange(k, device=t.device)] = flat
        out *= decided.unsqueeze(-1)  # (a rank that judged a proposal holds its data whatever was decided)
        return decided, out.view(t.dtype).reshape((n,) + tuple(t.shape))

    def bcast_rows(self, origins, t, stream=None):
        """Broadcast every row of the contiguous CUDA tensor t of shape [k, ...]: row i (at most max_payload bytes)
        from rank origins[i] of a one-part world without bulk messages, all k in ONE storm-send launch on torch's
        current stream (or `stream`, a raw hipStream_t).  Returns a tensor of shape [n, k, ...] and t's dtype: [r, i]
        is rank r's copy of row i (an origin's own rows are copied in from t here).  A row that is no multiple of 16
        bytes goes through a padded staging copy: t is never read past its end.
        Which call suits which shape: many rows from many origins -- this one, the progress kernel's batched storm
        path, whose rate grows with the world; one tensor from one origin, or a few messages in a small world where
        each one's latency counts -- bcast_tensor (the hop kernel's send program, one message per rank-wave at a
        time); rows beyond max_payload -- a world with bulk messages and bcast_tensor."""
        import torch

        if self.n_local != self.n:
            raise ValueError("bcast_rows: one-part worlds only")
        if self.info["bulk_max"]:
            raise ValueError("bcast_rows: a world without bulk messages")
        if not (t.is_cuda and t.is_contiguous()) or t.dim() < 1:
            raise ValueError("bcast_rows: a contiguous tensor [k, ...] in device memory")
        origin = np.asarray(origins, dtype=np.int64).reshape(-1)
        k, n = int(t.shape[0]), self.n
        if origin.size != k or (k and (origin.min() < 0 or origin.max() >= n)):
            raise ValueError("bcast_rows: one origin in [0, %d) per row" % n)
        row = t[0].numel() * t.element_size() if k else 0
        if k == 0 or row == 0:
            return t.unsqueeze(0).repeat((n,) + (1,) * t.dim())
        slot = rows_slot(row, self.info["slot_stride"] - 16)
        flat = t.reshape(k, -1).view(torch.uint8)
        if slot == row and flat.data_ptr() % 16 == 0:
            src = flat
        else:  # a padded staging copy: t is never read past its end
            src = torch.zeros((k, slot), dtype=torch.uint8, device=t.device)
            src[:, :row].copy_(flat)
        dst = torch.empty((n, k, slot), dtype=torch.uint8, device=t.device)
        self.program_send_storm(origin, src, dst, slot, lens=None if slot == row else [row] * k)
        if stream is None:
            stream = torch.cuda.current_stream(t.device).cuda_stream
        self.launch(stream=stream)
        self.wait()
        out = dst[:, :, :row].contiguous().view(t.dtype).reshape((n,) + tuple(t.shape))
        idx = torch.as_tensor(origin, device=t.device)
        ar = torch.arange(k, device=t.device)
        out[idx, ar] = t
        return out

    def _bcast_tensor_bulk(self, origin, t, stream):
        """bcast_tensor in a world with bulk messages: the bulk send program, fragments of at most bulk_max"""
        import torch

        n, nbytes = self.n, t.numel() * t.element_size()
        frags = bulk_fragments(nbytes, self.info["bulk_max"])
        k, stride = len(frags), frags[0][1] + (-frags[0][1]) % 16
        row = nbytes + (-nbytes) % 16
        flat = t.reshape(-1).view(torch.uint8)
        if nbytes % 16 == 0 and flat.data_ptr() % 16 == 0:
            src = flat
        else:  # a padded staging copy: t is never read past its end
            src = torch.empty(row, dtype=torch.uint8, device=t.device)
            src[:nbytes].copy_(flat)
        dst = torch.empty((n, row), dtype=torch.uint8, device=t.device)
        self.program_send_bulk([origin] * k, src, dst, stride, lens=[f[1] for f in frags], rank_stride=row)
        if stream is None:
            stream = torch.cuda.current_stream(t.device).cuda_stream
        self.launch(stream=stream)
        self.wait()
        out = dst[:, :nbytes].contiguous().view(t.dtype).reshape((n,) + tuple(t.shape))
        out[origin].copy_(t)
        return out

    def bcast_tensor(self, origin, t, stream=None):
        """Broadcast the contiguous CUDA tensor t (any dtype, any size) from rank `origin` of a one-part world, on
        torch's current stream (or `stream`, a raw hipStream_t): a kernel that produced t on that stream just before
        needs no synchronise.  A world without bulk messages sends it through the send program in messages of at most
        1008 bytes; a world with bulk messages through the bulk send program in messages of at most bulk_max bytes
        (bulk_fragments), moved at the bulk path's bandwidth.  Returns a tensor of
        shape [n, *t.shape] and t's dtype: row r is rank r's copy (the origin's row is t itself, copied here)."""
        import torch

        if self.n_local != self.n:
            raise ValueError("bcast_tensor: one-part worlds only")
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("bcast_tensor: a contiguous tensor in device memory")
        if not 0 <= origin < self.n:
            raise ValueError("bcast_tensor: origin %d of %d ranks" % (origin, self.n))
        n, nbytes = self.n, t.numel() * t.element_size()
        if nbytes == 0:
            return t.unsqueeze(0).repeat((n,) + (1,) * t.dim())
        if self.info["bulk_max"]:
            return self._bcast_tensor_bulk(origin, t, stream)
        slot = min(1008, self.info["slot_stride"] - 16)
        frags = send_fragments(nbytes, slot)
        k = len(frags)
        flat = t.reshape(-1).view(torch.uint8)
        if nbytes == k * slot and flat.data_ptr() % 16 == 0:
            src = flat
        else:  # a padded staging copy: t is never read past its end
            src = torch.empty(k * slot, dtype=torch.uint8, device=t.device)
            src[:nbytes].copy_(flat)
        dst = torch.empty((n, k * slot), dtype=torch.uint8, device=t.device)
        self.program_send([origin] * k, src, dst, slot, lens=[f[1] for f in frags])
        if stream is None:
            stream = torch.cuda.current_stream(t.device).cuda_stream
        self.launch(stream=stream)
        self.wait()
        out = dst[:, :nbytes].contiguous().view(t.dtype).reshape((n,) + tuple(t.shape))
        out[origin].copy_(t)
        return out

    # ------------------------------------------------------------ run
    def launch(self, stream=None, no_reset=False):
        check(self.lib.rlo_launch_ex(self.h, stream, L.RLO_LAUNCH_NO_RESET if no_reset else 0), "rlo_launch")

    def wait(self, raise_on_device_error=True):
        rc = self.lib.rlo_wait(self.h)
        if rc == L.RLO_E_DEVICE and not raise_on_device_error:
            return rc
        if rc == L.RLO_E_DEVICE:
            errs = {(self.rank_begin + r, L.DERR.get(s.error, s.error), s.error_aux)
                    for r, s in enumerate(self.stats_raw()) if s.error}
            code, aux = self.device_error()
            raise L.RloError("device engine error: %s; part error word %s aux 0x%08x" %
                             (sorted(errs)[:8], L.DERR.get(code, code), aux))
        return check(rc, "rlo_wait")

    def device_error(self):
        """(code, aux) of this part's device error word (rlo_device_error)"""
        c, a = ctypes.c_uint32(), ctypes.c_uint32()
        check(self.lib.rlo_device_error(self.h, ctypes.byref(c), ctypes.byref(a)), "rlo_device_error")
        return c.value, a.value

    def run(self, stream=None):
        """launch + wait; returns the kernel time in ms (HIP events on the launch stream)."""
        ms = ctypes.c_float()
        rc = self.lib.rlo_run(self.h, stream, ctypes.byref(ms))
        if rc == L.RLO_E_DEVICE:
            self.wait()
        check(rc, "rlo_run")
        return ms.value

    def kernel_ms(self):
        ms = ctypes.c_float()
        check(self.lib.rlo_last_kernel_ms(self.h, ctypes.byref(ms)), "rlo_last_kernel_ms")
        return ms.value

    # ------------------------------------------------------------ results
    def stats_raw(self):
        arr = (L.RankStats * self.n_local)()
        check(self.lib.rlo_stats(self.h, arr, self.n_local), "rlo_stats")
        return list(arr)

    def stats(self):
        raw = self.stats_raw()
        out = {}
        for f, _ in L.RankStats._fields_:
            if f in ("hist", "prof", "dbg"):
                out[f] = np.array([list(getattr(s, f)) for s in raw], dtype=np.uint64)
            else:
                out[f] = np.array([getattr(s, f) for s in raw], dtype=np.uint64)
        return out

    def log(self, rank, cap=1 << 16, payload=False):
        recs = (L.LogRec * cap)()
        stride = self.info["slot_stride"] - 16
        buf = np.zeros(cap * stride, dtype=np.uint8) if payload else None
        n = check(self.lib.rlo_log(self.h, rank, recs, cap, buf.ctypes.data if payload else None, stride), "rlo_log")
        rows = [(r.kind & 0xff, (r.kind >> 8) & 0xff, r.origin, r.from_, r.id, r.len, r.vote, r.aux, r.payload_idx)
                for r in recs[:n]]
        if payload:
            return rows, buf.reshape(cap, stride)
        return rows

    def latencies_ticks(self):
        arr = (ctypes.c_uint64 * self._lat_rounds)()
        n = check(self.lib.rlo_latencies(self.h, arr, self._lat_rounds), "rlo_latencies")
        return np.array(arr[:n], dtype=np.uint64)

    def round_ticks(self):
        """Clock of world rank 0 (10 ns ticks) when it saw each round complete (the part holding rank 0)."""
        arr = (ctypes.c_uint64 * self._lat_rounds)()
        n = check(self.lib.rlo_round_ticks(self.h, arr, self._lat_rounds), "rlo_round_ticks")
        return np.array(arr[:n], dtype=np.uint64)


    def timeline(self):
        """RLO_FLAG_TIMELINE rows (rlo_hip.h rlo_timeline): uint32 array [rounds][8 global + 9 x local ranks]
        of 10-ns clock values (0 = not seen on this part); the third per-rank column is the tree parent + 1."""
        stride = ctypes.c_uint32()
        check(self.lib.rlo_timeline(self.h, (ctypes.c_uint32 * 1)(), 0, ctypes.byref(stride)), "rlo_timeline")
        cap = 64 * stride.value
        arr = (ctypes.c_uint32 * cap)()
        n = check(self.lib.rlo_timeline(self.h, arr, cap, ctypes.byref(stride)), "rlo_timeline")
        return np.array(arr[:n * stride.value], dtype=np.uint32).reshape(n, stride.value)


def _dev_extent(x):
    """(pointer, bytes) of a device buffer: an (int pointer, nbytes) pair, or anything with data_ptr() / numel() /
    element_size() (a torch tensor)"""
    if isinstance(x, (tuple, list)):
        return int(x[0]), int(x[1])
    return int(x.data_ptr()), int(x.numel()) * int(x.element_size())


# the send programs' cfgs: kind -> (the mirror, its field of the message place)
_SEND_CFG = {"send": (L.SendCfg, "slot"), "send_bulk": (L.SendBulkCfg, "stride"), "send_storm": (L.SendStormCfg, "slot")}


def _send_cfg(kind, origins, src, dst, place, lens, rank_stride, window, flags, log_cap, n_local=None):
    """(cfg, what it points into) of a send program.  n_local: the local ranks of the world that is to run it -- src /
    dst are device buffers (_dev_extent) that must hold what the program reads and writes; None: the check wrappers'
    pointers as integers.  The argument ranges themselves are the library's (rlo_send_check and its kin)"""
    who = kind + "_check" if n_local is None else "program_" + kind
    struct, field = _SEND_CFG[kind]
    origin = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1))
    k = int(origin.size)
    ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.uint32).reshape(-1))
    if ln is not None and ln.size != k:
        raise ValueError("%s: %d lengths for %d messages" % (who, ln.size, k))
    sp, dp = src, dst
    if n_local is not None:
        (sp, sn), (dp, dn) = _dev_extent(src), _dev_extent(dst)
        if kind == "send":
            if sp % 16 or dp % 16:
                raise ValueError("program_send: src and dst must be 16-byte aligned")
            if sn < k * place or dn < n_local * k * place:
                raise ValueError("program_send: src holds %d bytes (needs %d), dst %d (needs %d)" %
                                 (sn, k * place, dn, n_local * k * place))
        elif k and place > 0 and place % 16 == 0 and rank_stride % 16 == 0:  # (else: the library's RloError)
            last = -(-int(ln[-1] if ln is not None else place) // 16) * 16
            rs = rank_stride or k * place
            if sn < (k - 1) * place + last or dn < (n_local - 1) * rs + (k - 1) * place + last:
                raise ValueError("%s: src holds %d bytes, dst %d: too small for %d messages of %s %d"
                                 % (who, sn, dn, k, field, place))
    cfg = struct()
    cfg.k = k
    cfg.origin = origin.ctypes.data if k else None
    cfg.len = None if ln is None or not k else ln.ctypes.data
    cfg.src, cfg.dst = sp, dp
    setattr(cfg, field, place)
    if kind != "send":
        cfg.rank_stride = rank_stride
    if kind == "send_storm":
        cfg.window = window
    cfg.flags, cfg.log_cap = flags, log_cap
    return cfg, [origin, ln, src, dst, cfg]


def _decide_cfg(origins, src, dst, decision, slot, lens, verdict, flags, log_cap, n_local=None):
    """(cfg, what it points into) of the decide program.  n_local: the local ranks of the world that is to run it -- the
    four buffers are device buffers (_dev_extent) that must hold what the program reads and writes, src and dst 16-B
    aligned; None: decide_check's pointers as integers.  The argument ranges themselves are the library's
    (rlo_decide_check)"""
    origin = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1))
    k = int(origin.size)
    ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.uint32).reshape(-1))
    if ln is not None and ln.size != k:
        raise ValueError("%s: %d lengths for %d proposals" % ("decide_check" if n_local is None else "program_decide", ln.size, k))
    sp, dp, vp, op = src, dst, verdict, decision
    if n_local is not None:
        (sp, sn), (dp, dn), (op, on) = _dev_extent(src), _dev_extent(dst), _dev_extent(decision)
        vp, vn = _dev_extent(verdict) if verdict is not None else (None, n_local * k)
        if sp % 16 or dp % 16:
            raise ValueError("program_decide: src and dst must be 16-byte aligned")
        if sn < k * slot or dn < n_local * k * slot or vn < n_local * k or on < n_local * k:
            raise ValueError("program_decide: src holds %d bytes (needs %d), dst %d (needs %d), verdict %d and decision %d "
                             "(need %d)" % (sn, k * slot, dn, n_local * k * slot, vn, on, n_local * k))
    cfg = L.DecideCfg()
    cfg.k = k
    cfg.origin = origin.ctypes.data if k else None
    cfg.len = None if ln is None or not k else ln.ctypes.data
    cfg.src, cfg.verdict, cfg.dst, cfg.decision = sp, vp, dp, op
    cfg.slot, cfg.flags, cfg.log_cap = slot, flags, log_cap
    return cfg, [origin, ln, src, dst, verdict, decision, cfg]


def decide_check(origins, slot, n_ranks, max_payload, lens=None, src=0x1000, dst=0x1000, decision=0x1000, verdict=None,
                 flags=0):
    """rlo_decide_check: the argument checks of the decide program that need no GPU; returns RLO_OK or RLO_E_INVAL
    (src / dst / decision / verdict: pointers as integers, never dereferenced)"""
    cfg, _keep = _decide_cfg(origins, src, dst, decision, slot, lens, verdict, flags, 0)
    return L.load().rlo_decide_check(ctypes.byref(cfg), n_ranks, max_payload)


def decide_slot(row_bytes, max_payload):
    """the proposal place World.decide_rows gives a row of row_bytes bytes: the row rounded up to 16 bytes, at least 16
    (a row that is no multiple of 16 is padded in a staging copy); a row beyond 992 bytes, or beyond what a proposal
    of the world carries (max_payload less its 16-byte frame), is refused.  Pure Python, no GPU"""
    row_bytes, cap = int(row_bytes), -(-int(max_payload) // 16) * 16 - 16
    if row_bytes < 0:
        raise ValueError("decide_slot: a negative row size")
    if row_bytes > 992:
        raise ValueError("decide_slot: a row of %d bytes (a proposal carries at most 992)" % row_bytes)
    slot = max(16, -(-row_bytes // 16) * 16)
    if slot > cap:
        raise ValueError("decide_slot: a row of %d bytes in a world of max_payload %d" % (row_bytes, max_payload))
    return slot


def send_fragments(nbytes, slot=1008):
    """the (offset, len) fragments of at most `slot` bytes that cover nbytes, in order (only the last is short): the
    messages World.bcast_tensor sends.  Pure Python, no GPU"""
    if slot <= 0 or slot % 16 or slot > 1008:
        raise ValueError("send_fragments: slot must be a multiple of 16 in 16 .. 1008")
    return [(off, min(slot, nbytes - off)) for off in range(0, max(int(nbytes), 0), slot)]


def rows_slot(row_bytes, max_payload):
    """the message place World.bcast_rows gives a row of row_bytes bytes: the row rounded up to 16 bytes (a row that
    is no multiple of 16 is padded in a staging copy); a row beyond the world's max_payload is refused.  Pure
    Python, no GPU"""
    row_bytes, cap = int(row_bytes), -(-int(max_payload) // 16) * 16
    if row_bytes <= 0:
        raise ValueError("rows_slot: an empty row")
    if row_bytes > int(max_payload):
        raise ValueError("rows_slot: a row of %d bytes in a world of max_payload %d" % (row_bytes, max_payload))
    slot = -(-row_bytes // 16) * 16
    assert slot <= cap
    return slot


def bulk_fragments(nbytes, bulk_max):
    """the (offset, len) fragments that cover nbytes as bulk messages of a world with this bulk_max, in order: each at
    most bulk_max rounded down to 16 bytes, every one but the last that long (a multiple of 16, so every fragment
    starts 16-B aligned): the messages World.bcast_tensor sends in a bulk world.  Pure Python, no GPU"""
    frag = int(bulk_max) // 16 * 16
    if frag <= 0:
        raise ValueError("bulk_fragments: bulk_max must be at least 16")
    return [(off, min(frag, nbytes - off)) for off in range(0, max(int(nbytes), 0), frag)]


def send_bulk_check(origins, stride, n_ranks, bulk_max, lens=None, rank_stride=0, src=0x1000, dst=0x1000, flags=0):
    """rlo_send_bulk_check: the argument checks of the bulk send program that need no GPU; returns RLO_OK or
    RLO_E_INVAL (src / dst: pointers as integers, never dereferenced)"""
    cfg, _keep = _send_cfg("send_bulk", origins, src, dst, stride, lens, rank_stride, 0, flags, 0)
    return L.load().rlo_send_bulk_check(ctypes.byref(cfg), n_ranks, bulk_max)


def send_storm_check(origins, slot, n_ranks, max_payload, lens=None, rank_stride=0, window=0, src=0x1000, dst=0x1000,
                     flags=0):
    """rlo_send_storm_check: the argument checks of the storm send program that need no GPU; returns RLO_OK or
    RLO_E_INVAL (src / dst: pointers as integers, never dereferenced)"""
    cfg, _keep = _send_cfg("send_storm", origins, src, dst, slot, lens, rank_stride, window, flags, 0)
    return L.load().rlo_send_storm_check(ctypes.byref(cfg), n_ranks, max_payload)


def pool_trim(what):
    """rlo_pool_trim: give pooled device regions / idle peer imports back (rlo_hip.h RLO_TRIM_*); returns bytes freed"""
    lib = L.load()
    freed = ctypes.c_uint64()
    check(lib.rlo_pool_trim(what, ctypes.byref(freed)), "rlo_pool_trim")
    return int(freed.value)


def pool_stats():
    """rlo_pool_stats: bytes live / free / free exported / retired, imports in use / idle"""
    lib = L.load()
    out = (ctypes.c_uint64 * 6)()
    check(lib.rlo_pool_stats(out, 6), "rlo_pool_stats")
    return dict(zip(("live", "free", "free_exported", "retired", "imports_used", "imports_idle"), [int(x) for x in out]))


def hist_percentile(hist, p):
    """Percentile (in 10 ns ticks) from the device log-bucket histogram (4 sub-bins per octave)."""
    hist = np.asarray(hist, dtype=np.float64)
    tot = hist.sum()
    if tot == 0:
        return 0.0
    c = np.cumsum(hist)
    b = int(np.searchsorted(c, p / 100.0 * tot))
    if b < 4:
        return float(b)
    o, sub = b // 4 + 1, b % 4
    lo = (4 + sub) << (o - 2)
    hi = (5 + sub) << (o - 2)
    return 0.5 * (lo + hi)


def bulk_plan(n, nbytes, cross=False):
    """rlo_bulk_plan: the chunk / stripe / tile plan every rank derives for a bulk message (host
    arithmetic, no GPU)"""
    out = L.BulkPlan()
    check(L.load().rlo_bulk_plan(n, nbytes, 1 if cross else 0, ctypes.byref(out)), "rlo_bulk_plan")
    return {"nchunks": out.nchunks, "stripe": out.stripe, "chunk": out.chunk, "tile": out.tile,
            "total_tiles": out.total_tiles, "direct": out.direct}


def layout_plan(n, n_parts=1, part=0, max_payload=4096, ring_slots=0, bulk_max=0, bulk_slots=0, movers=0,
                proposal_pool=0, pend_hbm=False, cus=256):
    """rlo_layout_plan: the LDS layout (waves, nsmall, stage2_bytes, ll_ok, pend_hbm, ...) a part of this world
    would get, from host arithmetic and the build's register guarantees (no GPU)"""
    cfg = L.PlanCfg(n, n_parts, part, max_payload, ring_slots, L.RLO_PART_PEND_HBM if pend_hbm else 0, bulk_max,
                    bulk_slots, movers, proposal_pool, cus)
    out = L.WorldInfo()
    check(L.load().rlo_layout_plan(ctypes.byref(cfg), ctypes.byref(out)), "rlo_layout_plan")
    return {f: getattr(out, f) for f, _ in L.WorldInfo._fields_}


def storm_lengths(seed, k, length, len_max=0):
    """rlo_storm_lengths: the payload length of each of the storm program's k bcasts (uint32 array)"""
    out = np.zeros(max(k, 1), dtype=np.uint32)
    check(L.load().rlo_storm_lengths(seed, k, length, len_max, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
          "rlo_storm_lengths")
    return out[:k]


def topology(n, rank):
    lib = L.load()
    v = [ctypes.c_int() for _ in range(4)]
    sl = (ctypes.c_int * 16)()
    check(lib.rlo_topology(n, rank, *[ctypes.byref(x) for x in v], sl), "rlo_topology")
    level, lw, scc, sll = (x.value for x in v)
    return {"level": level, "last_wall": lw, "send_channel_cnt": scc, "send_list_len": sll, "send_list": list(sl[:sll])}


def children(n, rank, origin, frm):
    out = (ctypes.c_int * 16)()
    k = check(L.load().rlo_children(n, rank, origin, frm, out), "rlo_children")
    return list(out[:k])

"""Sharded worlds: the ranks of one world split into parts, each part its own kernel and
its own rings, producers storing into peer parts' rings.

run_inprocess(): every part in this process, one HIP stream each (same GPU or several).
run_processes(): one spawned process per part; blobs are exchanged through a queue, the
                 regions are mapped with hipIpc (dmabuf), launches start after a barrier
                 that follows every part's reset.
A program spec is a dict: {"kind": "storm", "k", "len", "seed", "window", "log", "len_max", "order"} or
{"kind": "iar", "props": [(origin, pid, bytes)], "judge", "mask", "isp", "seed", "ppm", "log", "pool"} or
{"kind": "lat", "rounds", "len", "seed"} (the round word lives in part 0; st["round_ticks"] is world
rank 0's clock at each round's completion) or
{"kind": "send", "origins", "slot", "src": the k * slot source bytes (NumPy), "lens", "ordered", "log", "fill"}: each
part creates its own device buffers (dst pre-filled with `fill`, 0xA5), and st["dst"] is the world's destination
bytes as a NumPy array [rank][message][slot]; or
{"kind": "send_bulk", "origins", "stride", "src": the source bytes (NumPy, message i at i * stride), "lens", "log",
"fill"} (worlds with bulk messages): likewise, st["dst"] [rank][message][stride]; or
{"kind": "send_storm", "origins", "slot", "src", "lens", "window", "log", "fill"} (run_inprocess only): the storm send
program, buffers and st["dst"] as for "send"; or
{"kind": "decide", "origins", "slot", "src": the k * slot proposal data bytes (NumPy), "lens", "verdict": the world's
[rank][proposal] verdict bytes (NumPy) or None, "log", "fill"} (worlds of at most 16 ranks): each part creates its own
four device buffers (dst and the decisions pre-filled with `fill`, 0xA5); st["dst"] is the world's [rank][proposal][slot]
places and st["decision"] its [rank][proposal] decision bytes.
"""
import ctypes
import multiprocessing as mp
import os

import numpy as np


def even_bounds(n, parts):
    return [n * p // parts for p in range(parts + 1)]


def _hip():
    """the HIP runtime the engine's library is linked to, which its load brought in (no second copy is loaded)"""
    from . import _lib as L

    L.load()
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            return ctypes.CDLL(name, mode=os.RTLD_NOLOAD)
        except OSError:
            continue
    raise ImportError("the HIP runtime of librlo_hip.so is not loaded")


class _HipBuf:
    """a device buffer of a part: `init` a NumPy byte array (uploaded) or a byte count (filled with `fill`)"""

    def __init__(self, device, init, fill=0):
        self.hip = _hip()
        self.device = device
        self.nbytes = int(init.nbytes if isinstance(init, np.ndarray) else init)
        self.p = ctypes.c_void_p()
        self._set_device()
        self._chk(self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(max(self.nbytes, 16))), "hipMalloc")
        if isinstance(init, np.ndarray):
            self._chk(self.hip.hipMemcpy(self.p, ctypes.c_void_p(init.ctypes.data), ctypes.c_size_t(self.nbytes), 1), "hipMemcpy")
        else:
            self._chk(self.hip.hipMemset(self.p, ctypes.c_int(fill), ctypes.c_size_t(self.nbytes)), "hipMemset")
        self._chk(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def _set_device(self):
        if self.device >= 0:
            self._chk(self.hip.hipSetDevice(self.device), "hipSetDevice")

    @staticmethod
    def _chk(rc, what):
        if rc:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def extent(self):
        return (self.p.value, self.nbytes)

    def download(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        self._set_device()
        self._chk(self.hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), self.p, ctypes.c_size_t(self.nbytes), 2), "hipMemcpy")
        return out

    def free(self):
        if self.p:
            self._set_device()
            self.hip.hipFree(self.p)
            self.p = ctypes.c_void_p()


# the send programs' specs: kind -> (the World's method, the spec's key of the message place, further keys: defaults)
_SEND = {"send": ("program_send", "slot", {"ordered": False}), "send_bulk": ("program_send_bulk", "stride", {}),
         "send_storm": ("program_send_storm", "slot", {"window": 64})}


def _program(w, spec):
    if spec["kind"] == "storm":
        w.program_storm(spec["k"], spec["len"], seed=spec.get("seed", 0x5EED), window=spec.get("window", 64),
                        log=spec.get("log", False), log_cap=spec.get("log_cap", 0), hist=spec.get("hist", False),
                        len_max=spec.get("len_max", 0), order=spec.get("order", 0))
    elif spec["kind"] == "iar":
        from . import _lib as L
        w.program_iar(spec["props"], judge=spec.get("judge", L.RLO_JUDGE_APPROVE), mask=spec.get("mask"),
                      isp=spec.get("isp"), seed=spec.get("seed", 0), ppm=spec.get("ppm", 0),
                      log=spec.get("log", False), log_cap=spec.get("log_cap", 0), pool=spec.get("pool", 1))
    elif spec["kind"] == "lat":
        w.program_latency(spec["rounds"], spec["len"], seed=spec.get("seed", 0x5EED))
    elif spec["kind"] in _SEND:
        # the part's own device buffers: the whole source (a part reads only its own ranks' messages) and its ranks'
        # destination places, pre-filled; both are in place before the launch (which runs on a stream of its own).
        # Allocated through the HIP runtime the engine itself uses: a spawned part process has no other (torch found
        # no GPU there once the engine's runtime was up)
        method, place, extra = _SEND[spec["kind"]]
        src = _HipBuf(w.device, np.ascontiguousarray(spec["src"], dtype=np.uint8).reshape(-1))
        dst = _HipBuf(w.device, w.n_local * len(spec["origins"]) * spec[place], fill=spec.get("fill", 0xA5))
        w._send_bufs = (src, dst)
        getattr(w, method)(spec["origins"], src.extent(), dst.extent(), spec[place], lens=spec.get("lens"),
                           log=spec.get("log", False), log_cap=spec.get("log_cap", 0), hist=spec.get("hist", False),
                           **{key: spec.get(key, default) for key, default in extra.items()})
    elif spec["kind"] == "decide":
        # the part's own device buffers, as for the send programs: the whole source, its ranks' rows of the verdict
        # table (None: approve everything), and its ranks' places and decisions, pre-filled
        k, slot = len(spec["origins"]), spec["slot"]
        src = _HipBuf(w.device, np.ascontiguousarray(spec["src"], dtype=np.uint8).reshape(-1))
        ver = None
        if spec.get("verdict") is not None:
            rows = np.asarray(spec["verdict"], dtype=np.uint8).reshape(-1, k)[w.rank_begin:w.rank_end]
            ver = _HipBuf(w.device, np.ascontiguousarray(rows).reshape(-1))
        dst = _HipBuf(w.device, w.n_local * k * slot, fill=spec.get("fill", 0xA5))
        dec = _HipBuf(w.device, w.n_local * k, fill=spec.get("fill", 0xA5))
        w._decide_bufs = (src, ver, dst, dec)
        w.program_decide(spec["origins"], src.extent(), dst.extent(), dec.extent(), slot, lens=spec.get("lens"),
                         verdict=ver.extent() if ver else None, log=spec.get("log", False), log_cap=spec.get("log_cap", 0))
    else:
        raise ValueError(spec["kind"])


def _collect(w, spec):
    st = w.stats()
    w.info_now()  # (last_kernel: the kernel this launch ran)
    out = {"rank_begin": w.rank_begin, "stats": st, "ms": w.kernel_ms(), "info": dict(w.info)}
    if spec["kind"] == "lat" and w.rank_begin == 0:
        out["rounds"] = w.round_ticks()
    if spec["kind"] in _SEND:  # this part's destination buffer: [local rank][message][place] bytes
        out["dst"] = w._send_bufs[1].download().reshape(w.n_local, len(spec["origins"]), spec[_SEND[spec["kind"]][1]])
        for b in w._send_bufs:
            b.free()
    if spec["kind"] == "decide":  # this part's places [local rank][proposal][slot] and decisions [local rank][proposal]
        src, ver, dst, dec = w._decide_bufs
        out["dst"] = dst.download().reshape(w.n_local, len(spec["origins"]), spec["slot"])
        out["decision"] = dec.download().reshape(w.n_local, len(spec["origins"]))
        for b in (src, ver, dst, dec):
            if b is not None:
                b.free()
    if spec.get("log"):
        cap = spec.get("log_cap", 0) or 1024
        out["logs"] = {r: w.log(r, cap=cap, payload=spec["kind"] == "storm") for r in range(w.rank_begin, w.rank_end)}
    return out


def merge(results):
    """Concatenate per-part stats (ordered by rank) into world-wide arrays."""
    results = sorted(results, key=lambda r: r["rank_begin"])
    st = {}
    for key in results[0]["stats"]:
        st[key] = np.concatenate([r["stats"][key] for r in results])
    # per world rank: its part's rlo_world_info_t.peers / sys_scope (where that part's peers are)
    # (and last_kernel: the kernel its launch ran)
    for key in ("peers", "sys_scope", "last_kernel"):
        st["part_" + key] = np.concatenate([np.full(len(r["stats"]["error"]), r["info"][key]) for r in results])
    if "dst" in results[0]:  # the send program: every part's destination buffer, by world rank
        st["dst"] = np.concatenate([r["dst"] for r in results])
    if "decision" in results[0]:  # the decide program: every part's decisions, by world rank
        st["decision"] = np.concatenate([r["decision"] for r in results])
    logs = {}
    for r in results:
        logs.update(r.get("logs", {}))
        if "rounds" in r:
            st["round_ticks"] = r["rounds"]
    return st, logs, [r["ms"] for r in results]


def run_inprocess(n, bounds, spec, max_payload=4096, ring_slots=0, devices=None, uncached=False, blobs_for=None,
                  **world_kw):
    """world_kw: bulk_max / bulk_slots / movers / chunked (World.part).  blobs_for(p, blobs): the blobs part p
    connects with (tests: a forged PCI bus puts a peer "on another GPU", so the part runs system scope)"""
    from . import _lib as L
    from .world import World

    parts = len(bounds) - 1
    devices = devices or [0] * parts
    streams = []
    ws = [World.part(n, parts, p, part_begin=bounds, max_payload=max_payload, ring_slots=ring_slots,
                     device=devices[p], uncached=uncached, **world_kw) for p in range(parts)]
    try:
        blobs = [w.export() for w in ws]
        for p, w in enumerate(ws):
            w.connect(blobs_for(p, blobs) if blobs_for else blobs)
        for w in ws:
            _program(w, spec)
        for w in ws:
            w.reset()
        lib = L.load()
        for d in devices:
            s = ctypes.c_void_p()
            L.check(lib.rlo_stream_create(d, ctypes.byref(s)), "rlo_stream_create")
            streams.append(s)
        for w, s in zip(ws, streams):
            w.launch(stream=s, no_reset=True)
        rcs = [w.wait(raise_on_device_error=False) for w in ws]
        res = [_collect(w, spec) for w in ws]
        return merge(res), rcs
    finally:
        for w in ws:
            w.close()
        for s in streams:
            L.load().rlo_stream_destroy(s)


def _worker(n, bounds, part, device, spec, max_payload, ring_slots, uncached, blob_q, blobs_q, barrier, out_q,
            world_kw, repeat=1):
    try:
        from . import _lib as L
        from .world import World, pool_trim

        for it in range(repeat):
            w = World.part(n, len(bounds) - 1, part, part_begin=bounds, max_payload=max_payload, ring_slots=ring_slots,
                           device=device, uncached=uncached, **world_kw)
            blob_q.put((part, w.export()))
            blobs = blobs_q.get(timeout=120)

            def bcast(blob, k):  # part k's fresh blob, relayed by the parent
                if blob is not None:
                    blob_q.put((k, blob))
                return blobs_q.get(timeout=120)

            # one exporter at a time, its handles exported at its own stage (rlo_hip.h rlo_part_import)
            w.staged_connect(blobs, lambda: barrier.wait(timeout=120), bcast)
            _program(w, spec)
            w.reset()
            barrier.wait(timeout=120)  # every part is reset before any part launches
            w.launch(no_reset=True)
            rc = w.wait(raise_on_device_error=False)
            res = _collect(w, spec)
            barrier.wait(timeout=120)  # no peer still stores into this part's rings
            # every part drops its imports of its peers' regions before any part frees its own (a part that frees and
            # re-exports memory a peer still imports can hand that peer its OLD memory for the new handle)
            w.close_imports()
            barrier.wait(timeout=120)
            w.close()
            if os.environ.get("RLO_POOL_CAP_BYTES"):
                # a lowered pool cap (the test hook): the world-wide close, so exported regions beyond it are freed --
                # every part drops its idle imports, then every part frees its retired regions (rlo_hip.h rlo_pool_trim)
                pool_trim(L.RLO_TRIM_IMPORTS | L.RLO_TRIM_FREE)
                barrier.wait(timeout=120)
                res["pool_freed"] = pool_trim(L.RLO_TRIM_RETIRED)
                barrier.wait(timeout=120)
            out_q.put((part, rc, res, None))
    except Exception as e:  # report instead of hanging the parent
        out_q.put((part, -99, None, repr(e)))


def run_processes(n, bounds, spec, max_payload=4096, ring_slots=0, devices=None, uncached=False, timeout=300,
                  repeat=1, **world_kw):
    """repeat > 1: every part process creates, connects (hipIpc), runs and destroys the world `repeat` times
    in a row -- the per-leg churn of bench.py's N-part run; returns the list of per-repeat results"""
    parts = len(bounds) - 1
    devices = devices or [0] * parts
    ctx = mp.get_context("spawn")
    blob_q, out_q = ctx.Queue(), ctx.Queue()
    blobs_qs = [ctx.Queue() for _ in range(parts)]
    barrier = ctx.Barrier(parts)
    procs = [ctx.Process(target=_worker, args=(n, bounds, p, devices[p], spec, max_payload, ring_slots, uncached,
                                               blob_q, blobs_qs[p], barrier, out_q, world_kw, repeat))
             for p in range(parts)]
    for p in procs:
        p.start()
    runs = []
    try:
        for _ in range(repeat):
            got = dict(blob_q.get(timeout=timeout) for _ in range(parts))
            blobs = [got[p] for p in range(parts)]
            for q in blobs_qs:
                q.put(blobs)
            for k in range(parts):  # staged connect: part k's fresh blob to every part
                pk, bk = blob_q.get(timeout=timeout)
                assert pk == k, (pk, k)
                for q in blobs_qs:
                    q.put(bk)
            outs = [out_q.get(timeout=timeout) for _ in range(parts)]
            errs = [(p, e) for p, rc, r, e in outs if e]
            if errs:
                raise RuntimeError("part failed: %s" % errs)
            runs.append((merge([r for _, _, r, _ in outs]), [rc for _, rc, _, _ in sorted(outs, key=lambda x: x[0])]))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return runs[0] if repeat == 1 else runs

"""Device-side plumbing: torch owns the HBM buffers and the stream, libdtfill.so does the work.

`DtFill` is the batched operator behind the reference-named functions in tools.py.  It holds one
workspace + output set per (B, H, W) so that repeated calls (the reference calls the op once per
frame in a loop, demo.py:268-290 / eval_NYU.py:138-195) allocate nothing.
"""
import contextlib
import ctypes
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib

_NP_DTYPES = {"depth": np.float32, "dt": np.float32, "index": np.int32, "status": np.int32}
WANT_ALL = ("depth", "dt", "index")


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError(
            "dtfill needs a HIP device (torch.cuda.is_available() is False); the operator has "
            "no CPU fallback -- the CPU restatement under oracle/ is test infrastructure only"
        )


def _check_tensor(t, what, dtype=torch.float32, layout="[B,H,W]", like=None, like_name=None):
    """The one rule for a tensor argument: contiguous, of `dtype`, on a GPU, of the rank `layout` spells out (one more than
    its commas; at least that many where it ends in "...]"), and, with like=, of that tensor's shape and device."""
    rank = layout.count(",") + 1
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (t.dim() < rank if layout.endswith("...]") else t.dim() != rank):
        raise ValueError("%s must be a contiguous %s CUDA tensor %s" % (what, str(dtype).replace("torch.", ""), layout))
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError("%s must have %s's shape and device" % (what, like_name))


def _ptr(t):
    """The device pointer the C side takes: NULL for an optional tensor that is not there."""
    return None if t is None else t.data_ptr()


def _stream(device):
    """The current stream of `device` as the handle the C side takes."""
    return torch.cuda.current_stream(device).cuda_stream


def _sized(nbytes):
    """A *_workspace_bytes() result: 0 is how the C side refuses a shape (DTFILL_ERR_SHAPE), raised here as that error."""
    if nbytes == 0:
        _lib.check(-2)
    return nbytes


def _workspace(nbytes, device):
    """(a fresh uint8 tensor, the first 256-byte aligned address in it): nbytes of workspace as the C side wants them aligned."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


class DtFill:
    """Batched DT + nearest-valid-depth fill on one GPU.

    Parameters mirror the literals of the reference: src_thr is the 0.1 of tools.py:8 (0.001 in
    eval_NYU.py:115), val_thr the 0.1 of tools.py:22; metric "l1_cv" is the reference's
    cv2.DIST_L1 / mask 5 / DIST_LABEL_PIXEL transform.

    Threads and streams.  One pass in flight at a time per object: the workspace, the output buffers and the staging buffers
    are this object's, so a second pass may start only where it is ordered behind the first -- on the same stream, or behind an
    event of it.  Host threads that share an object serialise on its lock instead of corrupting it: run() holds the lock from
    the buffer check to the last launch (one pass's launches stay contiguous on their stream), run_numpy() from the staging copy
    to the stream synchronisation (the staging buffers and the returned frames are one caller's).  The tensors run() returns
    without `out=` are still overwritten by the next pass, another thread's included: threads that share an object pass `out=`
    or use run_numpy().  The buffers belong to the stream that was current when they were allocated; a pass on another stream
    records itself on them (Tensor.record_stream), so that dropping or reshaping the object while that pass is in flight does
    not hand their memory out again before the pass is done.
    """

    def __init__(self, device=None, metric="l1_cv"):
        _require_gpu()
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if metric not in _lib.METRICS:
            raise ValueError("metric must be one of %s" % sorted(_lib.METRICS))
        self.metric = _lib.METRICS[metric]
        self._shape = None
        self._ws = None
        self._out = None
        self._crop = None
        self._dev_in = None
        self._pin_in = self._pin_status = self._pin_shape = None  # upload()'s page-locked staging
        self._home = {}  # buffer attribute -> the stream it was allocated under
        self._lock = threading.RLock()

    # -- buffers -------------------------------------------------------------------------------
    def _ensure(self, B, H, W):
        with self._lock:
            self._ensure_locked(B, H, W)

    def _ensure_locked(self, B, H, W):
        if self._shape == (B, H, W):
            return
        nbytes = _sized(self.lib.dtfill_workspace_bytes(B, H, W, self.metric))
        self._ws, aligned = _workspace(nbytes, self.device)
        self._ws_off = aligned - self._ws.data_ptr()
        self._ws_bytes = nbytes
        self._out = {
            "depth": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
            "dt": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
            "index": torch.empty((B, H, W), dtype=torch.int32, device=self.device),
            "status": torch.empty((B,), dtype=torch.int32, device=self.device),
        }
        self._shape = (B, H, W)
        self._home["_ws"] = self._home["_out"] = _stream(self.device)

    def _on_stream(self, stream):
        """Before a pass on `stream` (holding the lock): every buffer of this object that was allocated under another stream
        records the pass, so that the caching allocator keeps its memory until the pass is done."""
        for name in ("_ws", "_out", "_crop", "_dev_in"):
            if self._home.get(name) == stream.cuda_stream:  # (a buffer somebody else put there has no home: it records)
                continue
            buf = getattr(self, name)
            for t in (buf.values() if isinstance(buf, dict) else () if buf is None else (buf,)):
                t.record_stream(stream)

    def workspace_bytes(self, B, H, W):
        return int(self.lib.dtfill_workspace_bytes(B, H, W, self.metric))

    # -- the op --------------------------------------------------------------------------------
    def run(self, x, src_thr=0.1, val_thr=0.1, want=WANT_ALL, timed=False, path="auto", depth_rows_from=0, depth_floor=None,
            outlier_removal=False, separate_frame=False, out=None):
        """x: float32 CUDA tensor [B,H,W] (contiguous).  Returns a dict of device tensors
        (views of buffers owned by this object, overwritten by the next call) for the names in
        `want`, plus "status" (int32 [B], bit set of _lib.FRAME_*).  Asynchronous on the current
        stream unless timed.  path: "auto" (window kernel for dense frames, any-distance kernels for the
        others), "general" or "fused" (tests / benchmarks).  depth_rows_from / depth_floor: the drivers'
        post-fill steps folded into the depth stores (demo.py:292-293 rows 96:, eval_NYU.py:205
        relu(d - 0.9) + 0.9): "depth" is then [B, H - depth_rows_from, W]; l1_cv only.  outlier_removal: the loader's filter
        (data_read.py:103-128, 168-169) in front of the predicates -- the pass equals run(outlier_removal_device(x)) without
        the filtered map being written.  separate_frame: l1_cv, the frame facts in a k_frame launch of their own instead of inside
        the window kernel's launch (_lib.FLAG_SEPARATE_FRAME: tests and A/B timing; the results are the same).  out: a dict of the
        caller's own tensors, name -> contiguous tensor of that output's shape and dtype on this device ("depth", "dt", "index",
        "status"), written in place of this object's buffers and returned: tensors no later call overwrites."""
        _check_tensor(x, "x")
        B, H, W = x.shape
        with torch.cuda.device(x.device), self._lock:
            if x.device != self.device:
                raise ValueError("x lives on %s, operator on %s" % (x.device, self.device))
            self._ensure_locked(B, H, W)
            o = self._out
            epi = depth_rows_from != 0 or depth_floor is not None
            if out is not None:
                for name, t in out.items():
                    if name not in o:
                        raise ValueError("out: no output named %r" % (name,))
                    shape = (B, H - depth_rows_from, W) if name == "depth" else tuple(o[name].shape)
                    if t.dtype != o[name].dtype or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                        raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (name, o[name].dtype, shape, self.device))
            if epi:
                if timed or not (0 <= depth_rows_from < H):
                    raise ValueError("depth epilogue: 0 <= depth_rows_from < H, and not with timed=True")
                if self._crop is None or self._crop.shape != (B, H - depth_rows_from, W):
                    self._crop = torch.empty((B, H - depth_rows_from, W), dtype=torch.float32, device=self.device)
                    self._home["_crop"] = _stream(self.device)
                if out is None or "depth" not in out:
                    o = dict(o, depth=self._crop)
            if out is not None:
                o = dict(o, **out)
            ptr = lambda name: o[name].data_ptr() if name in want else None
            current = torch.cuda.current_stream(self.device)
            self._on_stream(current)
            stream = current.cuda_stream
            args = [
                x.data_ptr(), B, H, W, float(src_thr), float(val_thr), self.metric,
                ptr("depth"), ptr("dt"), ptr("index"), o["status"].data_ptr(),
                self._ws.data_ptr() + self._ws_off, self._ws_bytes, stream,
            ]
            flags = _lib.PATHS[path] | (_lib.FLAG_OUTLIER_REMOVAL if outlier_removal else 0) | (_lib.FLAG_SEPARATE_FRAME if separate_frame else 0)
            if timed:
                nk = self.lib.dtfill_num_kernels(self.metric)
                ms = (ctypes.c_float * nk)()
                _lib.check(self.lib.dtfill_batch_timed(*args, flags, ctypes.cast(ms, ctypes.c_void_p)))
                names = [self.lib.dtfill_kernel_name(self.metric, k).decode() for k in range(nk)]
                self.last_kernel_ms = dict(zip(names, [float(v) for v in ms]))
            elif epi:
                _lib.check(self.lib.dtfill_batch_epilogue(*args, flags, int(depth_rows_from), int(depth_floor is not None),
                                                          float(depth_floor or 0.0)))
            else:
                _lib.check(self.lib.dtfill_batch_flags(*args, flags))
        res = {k: o[k] for k in want}
        res["status"] = o["status"]
        return res

    def upload(self, xh):
        """Host frames [B,H,W] (any real dtype / strides) -> this operator's float32 device input buffer, asynchronously on the
        current stream (the staging buffer is this object's: a caller that shares the object with other threads holds its lock
        until the copy has run, as run_numpy does): a small thread pool copies the caller's pageable array into pinned staging
        memory a few frames at a time (numpy releases the GIL inside the copy), every chunk's DMA starting as soon as its copy
        is done."""
        B, H, W = xh.shape
        nchunk = min(B, 8)
        cuts = [B * c // nchunk for c in range(nchunk + 1)]
        pool = _copy_pool()
        with torch.cuda.device(self.device), self._lock:
            self._ensure_locked(B, H, W)
            current = torch.cuda.current_stream(self.device)
            if self._pin_shape != (B, H, W):
                self._pin_in = torch.empty((B, H, W), dtype=torch.float32).pin_memory()
                self._dev_in = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
                self._pin_status = torch.empty((B,), dtype=torch.int32).pin_memory()
                self._pin_shape = (B, H, W)
                self._home["_dev_in"] = current.cuda_stream
            self._on_stream(current)
            pin_in = self._pin_in.numpy()
            stage = [pool.submit(np.copyto, pin_in[cuts[c]:cuts[c + 1]], xh[cuts[c]:cuts[c + 1]], "same_kind") for c in range(nchunk)]
            for c in range(nchunk):
                stage[c].result()  # (one pass: gathers strided input, casts if needed)
                self._dev_in[cuts[c]:cuts[c + 1]].copy_(self._pin_in[cuts[c]:cuts[c + 1]], non_blocking=True)
        return self._dev_in

    def pass_stats(self):
        """Which kernel family owned how many pixels in the last run() of this operator (dtfill_pass_stats): dict of ints."""
        out = torch.zeros(len(_lib.STATS), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device), self._lock:
            B, H, W = self._shape
            self._on_stream(torch.cuda.current_stream(self.device))
            _lib.check(self.lib.dtfill_pass_stats(self._ws.data_ptr() + self._ws_off, self._ws_bytes, B, H, W, self.metric, out.data_ptr(),
                                                  _stream(self.device)))
        return dict(zip(_lib.STATS, [int(v) for v in out.cpu().tolist()]))

    def run_numpy(self, x, src_thr=0.1, val_thr=0.1, want=WANT_ALL, depth_rows_from=0, depth_floor=None, outlier_removal=False):
        """numpy in / numpy out: H2D, run, D2H.  x: float32 [B,H,W].  Raises IndexError exactly
        where numpy would in depth_list[label_list-1] (tools.py:26) when depth is wanted.

        Host side of the transfer (what a reference-style caller pays on top of the pass):
          in   the caller's pageable array is copied into pinned staging memory a few frames at a time by a small thread
               pool (numpy releases the GIL inside the copy), every chunk's DMA starting as soon as its copy is done;
          out  the device-to-host DMA lands directly in the array that is returned: a page-locked buffer taken from a
               rotating pool (_HostPool).  A buffer goes back to the pool when the caller has dropped the array it was handed
               (and every view of it), so each call still returns arrays nothing else will ever write to -- the contract of
               the reference, which builds fresh arrays (tools.py:29-35) -- without the extra host copy."""
        xh = np.asarray(x)
        if xh.ndim != 3:
            raise ValueError("x must be [B,H,W]")
        B, H, W = xh.shape
        # the lock from the staging copy to the synchronisation: the pinned staging buffer, the device input, the outputs and the
        # status buffer are this call's until its last DMA has landed
        with torch.cuda.device(self.device), self._lock:
            stream = torch.cuda.current_stream(self.device)
            dev_in = self.upload(xh)
            res = self.run(dev_in, src_thr, val_thr, want, depth_rows_from=depth_rows_from, depth_floor=depth_floor,
                           outlier_removal=outlier_removal)
            self._pin_status.copy_(res["status"], non_blocking=True)
            out = {}
            for k, v in res.items():
                if v.dim() != 3:
                    continue
                # contiguous in the shape that is returned (a cropped depth is [B, H - r0, W]): one DMA per output
                host = _host_pool.take(tuple(v.shape), _NP_DTYPES[k])
                host.tensor.copy_(v, non_blocking=True)
                out[k] = host.array
            stream.synchronize()
            out["status"] = self._pin_status.numpy().copy()
        if "depth" in want:
            bad = np.nonzero(out["status"] & _lib.FRAME_INDEX_ERROR)[0]
            if bad.size:
                raise IndexError(
                    "frame %d: index out of bounds in depth_list[label_list-1] "
                    "(value list shorter than a label, or empty with label 0)" % int(bad[0])
                )
        return out


class _HostBuf:
    __slots__ = ("tensor", "array", "alive")


class _HostPool:
    """Page-locked host buffers handed out as numpy arrays.  A buffer is free again once the array made from it (and every
    view: numpy views keep their base alive) has been garbage collected; until then nobody writes to it.  At most
    `cap_bytes` stay cached; beyond that a request gets a buffer that is simply released with its array."""

    def __init__(self, cap_bytes=2 << 30):
        self._free = {}
        self._lock = threading.Lock()
        self._cached = 0
        self._cap = cap_bytes

    def take(self, shape, dtype):
        key = (tuple(shape), np.dtype(dtype).str)
        with self._lock:
            lst = self._free.get(key)
            t = lst.pop() if lst else None
        if t is None:
            t = torch.empty(shape, dtype=torch.from_numpy(np.empty(0, dtype)).dtype).pin_memory()
        else:
            with self._lock:
                self._cached -= t.numel() * t.element_size()
        # a fresh ndarray object over the pinned memory.  numpy collapses the base of every view (slices, expand_dims, ...) to
        # this object, so it is alive exactly as long as anything of the caller's still looks at the buffer; when it dies the
        # tensor goes back to the pool
        a = t.numpy()
        h = _HostBuf()
        h.tensor, h.array = t, a
        weakref.finalize(a, self._give_back, key, t)
        return h

    def _give_back(self, key, t):
        nbytes = t.numel() * t.element_size()
        with self._lock:
            if self._cached + nbytes <= self._cap:
                self._free.setdefault(key, []).append(t)
                self._cached += nbytes


_host_pool = _HostPool()
_pool = None


def _copy_pool():
    """Threads for host-side staging copies (numpy's copy loops release the GIL)."""
    global _pool
    if _pool is None:
        from concurrent.futures import ThreadPoolExecutor

        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        _pool = ThreadPoolExecutor(max(1, min(8, n)), thread_name_prefix="dtfill-copy")
    return _pool


def host_link_bandwidth(nbytes=64 << 20, device=None, repeats=5):
    """Measured pinned host <-> device copy rates of this box in GB/s: what bounds a numpy-in / numpy-out caller."""
    _require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rates = {}
    for name, (dst, src) in (("h2d", (d, h)), ("d2h", (h, d))):
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(repeats):
            dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize(dev)
        rates[name] = nbytes * repeats / (e0.elapsed_time(e1) * 1e-3) / 1e9
    return rates


def outlier_removal_device(x):
    """x: contiguous float32 CUDA tensor [B,H,W] -> new tensor, data_read.py:103-128 on the device."""
    _require_gpu()
    _check_tensor(x, "x")
    out = torch.empty_like(x)
    B, H, W = x.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_outlier_removal(x.data_ptr(), B, H, W, out.data_ptr(), _stream(x.device)))
    return out


def generate_multi_channel_device(data, mask, table_size=7, scale_num=4, outs=None):
    """net.py:83-122 on the device.  data, mask: contiguous float32 CUDA tensors [B,H,W].
    Returns (lidar_1, lidar_2, lidar_3, lidar_4) with None beyond scale_num, like the reference.  outs: scale_num - 1 tensors
    like data to hold lidar_2.. (a caller that keeps its buffers); new ones by default."""
    _require_gpu()
    _check_tensor(data, "data")
    _check_tensor(mask, "mask")
    if data.shape != mask.shape:
        raise ValueError("data and mask shapes differ")
    B, H, W = data.shape
    if outs is None:
        outs = [torch.empty_like(data) for _ in range(scale_num - 1)]
    else:
        outs = list(outs)
        if len(outs) != scale_num - 1:
            raise ValueError("outs must hold scale_num - 1 = %d tensors, got %d" % (scale_num - 1, len(outs)))
        for k, o in enumerate(outs):
            _check_tensor(o, "outs[%d]" % k, like=data, like_name="data")
    ptrs = [o.data_ptr() for o in outs] + [None] * (4 - scale_num)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().dtfill_generate_multi_channel(
            data.data_ptr(), mask.data_ptr(), B, H, W, table_size, scale_num, ptrs[0], ptrs[1], ptrs[2], _stream(data.device)))
    return tuple([data] + outs + [None] * (4 - scale_num))


class _Scratch:
    """(device index, stream) -> one scratch tensor for one entry point's workspace, grown on demand, and the lock that goes with
    it.  Calls on one stream are ordered, so they can share the scratch -- as long as one call's launches are contiguous in the
    stream: hold() keeps the entry's lock while the caller enqueues, so a second host thread on the same stream enqueues its call
    behind this one's last launch, not between two of them.  The lock is held across the enqueue only, never across a host
    synchronisation.  Another stream has another entry: its calls run beside these in scratch of their own."""

    def __init__(self):
        self._entries = {}
        self._lock = threading.Lock()

    @contextlib.contextmanager
    def hold(self, device, nbytes):
        """A 256-byte aligned pointer to at least nbytes of scratch on `device`, the current stream's, for one call's enqueue."""
        key = (device.index, _stream(device))
        with self._lock:
            entry = self._entries.get(key)
            if entry is None:
                entry = self._entries[key] = [threading.Lock(), None, None]  # the lock, the tensor, its aligned address
        with entry[0]:
            if entry[1] is None or entry[1].numel() < nbytes + 256:
                # (the tensor it replaces goes back to this stream's pool, behind the launches that still use it)
                entry[1:] = _workspace(nbytes, device)
            yield entry[2]


_gmcb_ws = _Scratch()  # the backward's workspace


def generate_multi_channel_backward_device(mask, out2, out3, grads, table_size=7, scale_num=4):
    """The backward of generate_multi_channel_device (include/dtfill.h, dtfill_generate_multi_channel_backward): the gradient
    with respect to data.  mask: the forward's; out2, out3: the forward's lidar_2 and lidar_3 (needed for scale_num >= 3 and
    4, None otherwise is fine); grads: the gradients of (lidar_1, .., lidar_4), a 4-sequence, None for a zero gradient.  All
    contiguous float32 CUDA tensors [B,H,W] on one device.  Returns a new tensor; asynchronous on the current stream."""
    _require_gpu()
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    grads = tuple(grads)
    if len(grads) != 4:
        raise ValueError("grads must hold four gradients (None for a zero one), got %d" % len(grads))
    need = (("mask", mask, True), ("out2", out2, scale_num >= 3), ("out3", out3, scale_num == 4))
    named = need + tuple(("grads[%d]" % k, g, False) for k, g in enumerate(grads))
    for what, t, required in named:
        if t is None:
            if required:
                raise ValueError("%s is needed for scale_num %d" % (what, scale_num))
            continue
        _check_tensor(t, what, like=mask, like_name="mask")
    B, H, W = mask.shape
    L = _lib.load()
    out = torch.empty_like(mask)
    with torch.cuda.device(mask.device):
        nbytes = L.dtfill_generate_multi_channel_backward_workspace_bytes(B, H, W, scale_num)
        with (_gmcb_ws.hold(mask.device, nbytes) if nbytes else contextlib.nullcontext()) as ws:
            _lib.check(L.dtfill_generate_multi_channel_backward(
                mask.data_ptr(), _ptr(out2), _ptr(out3), B, H, W, int(table_size), int(scale_num), *[_ptr(g) for g in grads],
                out.data_ptr(), ws, nbytes, _stream(mask.device)))
    return out


def demo_multi_channel_device(lidar, rgb=None, table_size=7, scale_range=90.0, scale_num=4):
    """demo.py:108-149 (rgb None) / :151-198 on the device (include/dtfill.h, dtfill_demo_multi_channel).  lidar: contiguous
    float32 CUDA tensor [B,H,W]; rgb: contiguous float32 CUDA tensor [B,H,W,C] or None.  Returns (out_1, .., out_4) with None
    beyond scale_num: [B,H,W] = raw_k / scale_range without rgb, [B,H,W,C+1] = concat(rgb, raw_k / scale_range) /
    scale_range with it.  Asynchronous on the current stream."""
    _require_gpu()
    _check_tensor(lidar, "lidar")
    B, H, W = lidar.shape
    C = 0
    if rgb is not None:
        _check_tensor(rgb, "rgb", layout="[B,H,W,C]")
        if tuple(rgb.shape[:3]) != (B, H, W) or rgb.device != lidar.device:
            raise ValueError("rgb must hold lidar's frames: [%d,%d,%d,C] on %s" % (B, H, W, lidar.device))
        C = rgb.shape[3]
    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    L = _lib.load()
    nbytes = L.dtfill_demo_multi_channel_workspace_bytes(B, H, W, scale_num)
    ws, ws_ptr = _workspace(nbytes, lidar.device)
    shape = (B, H, W) if rgb is None else (B, H, W, C + 1)
    outs = [torch.empty(shape, dtype=torch.float32, device=lidar.device) for _ in range(scale_num)]
    ptrs = [o.data_ptr() for o in outs] + [None] * (4 - scale_num)
    with torch.cuda.device(lidar.device):
        _lib.check(L.dtfill_demo_multi_channel(lidar.data_ptr(), _ptr(rgb), C, B, H, W, int(table_size), int(scale_num),
                                               float(scale_range), *ptrs, ws_ptr, nbytes, _stream(lidar.device)))
    return tuple(outs + [None] * (4 - scale_num))


def crop_floor_device(x, rows=None, cols=None, floor=None):
    """out = f(x[:, rows[0]:rows[1], cols[0]:cols[1]]); f = relu(d - floor) + floor when floor is given
    (demo.py:292-293, eval_NYU.py:202-205).  x: contiguous float32 CUDA tensor [B,H,W] -> new tensor."""
    _require_gpu()
    _check_tensor(x, "x")
    B, H, W = x.shape
    r0, r1 = (0, H) if rows is None else rows
    c0, c1 = (0, W) if cols is None else cols
    if not (0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W):
        raise ValueError("empty or out-of-frame crop rows=%s cols=%s of a %dx%d frame" % (rows, cols, H, W))
    out = torch.empty((B, r1 - r0, c1 - c0), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_crop_floor(x.data_ptr(), B, H, W, r0, r1, c0, c1, int(floor is not None),
                                                 float(floor or 0.0), out.data_ptr(), _stream(x.device)))
    return out


def png16_device(x, pad_top=96, floor=0.9, lo=0.0, hi=100.0, scale=256.0):
    """test.py:133-148 on the device: x float32 CUDA [B,H,W] -> uint16 CUDA [B, pad_top+H, W]."""
    _require_gpu()
    _check_tensor(x, "x")
    B, H, W = x.shape
    out = torch.empty((B, H + pad_top, W), dtype=torch.uint16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dtfill_png16(x.data_ptr(), B, H, W, pad_top, int(floor is not None), float(floor or 0.0),
                                            lo, hi, scale, out.data_ptr(), _stream(x.device)))
    return out


def metrics_device(output, target, kind="kitti"):
    """evaluation.py:82-123 (kind "kitti") / :196-239 ("nyu"), one row per frame.  output, target: contiguous
    float32 CUDA tensors [B, ...] of equal shape -> float64 CUDA tensor [B, 9], columns _lib.METRICS_COLUMNS."""
    _require_gpu()
    kinds = {"kitti": _lib.METRICS_KITTI, "nyu": _lib.METRICS_NYU}
    if kind not in kinds:
        raise ValueError("kind must be 'kitti' or 'nyu'")
    _check_tensor(output, "output", layout="[B, ...]")
    _check_tensor(target, "target", layout="[B, ...]")
    if output.shape != target.shape:
        raise ValueError("output and target shapes differ")
    B = output.shape[0]
    n = output[0].numel()
    L = _lib.load()
    nbytes = L.dtfill_metrics_workspace_bytes(B)
    ws, ws_ptr = _workspace(nbytes, output.device)
    out = torch.empty((B, len(_lib.METRICS_COLUMNS)), dtype=torch.float64, device=output.device)
    with torch.cuda.device(output.device):
        _lib.check(L.dtfill_metrics(output.data_ptr(), target.data_ptr(), B, n, kinds[kind], out.data_ptr(), ws_ptr, nbytes,
                                    _stream(output.device)))
    return out


LOSS_PRESETS = {  # dataset -> (kind, gt_thr, in_thr, rows, cols) of train.py:215-216, :244 and :220-221, :242
    "KITTI": (_lib.LOSS_KITTI, 0.1, 0.1, None, None),
    "NYU": (_lib.LOSS_NYU, 0.0001, 0.001, (6, 228), (8, 304)),
}
_loss_ws = _Scratch()  # the forward's partial sums


def _loss_args(pred, gt, lidar, correction, dataset, gt_thr, in_thr, rows, cols):
    """The checked C arguments both loss entry points share: (pointers, B, H, W, kind, gt_thr, in_thr, r0, r1, c0, c1)."""
    _require_gpu()
    if dataset not in LOSS_PRESETS:
        raise ValueError("dataset must be 'KITTI' or 'NYU', got %r" % (dataset,))
    if (lidar is None) != (correction is None):
        raise ValueError("lidar and correction come together (train.py's --correct) or not at all")
    for what, t in (("pred", pred), ("gt", gt), ("lidar", lidar), ("correction", correction)):
        if t is None:
            continue
        _check_tensor(t, what, like=pred, like_name="pred")
    kind, gthr, ithr, prows, pcols = LOSS_PRESETS[dataset]
    B, H, W = pred.shape
    r0, r1 = (prows or (0, H)) if rows is None else rows
    c0, c1 = (pcols or (0, W)) if cols is None else cols
    if not (0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W):
        raise ValueError("empty or out-of-frame window rows=%s cols=%s of a %dx%d frame" % ((r0, r1), (c0, c1), H, W))
    ptrs = (pred.data_ptr(), _ptr(correction), gt.data_ptr(), _ptr(lidar))
    return ptrs + (B, H, W, kind, float(gthr if gt_thr is None else gt_thr), float(ithr if in_thr is None else in_thr),
                   int(r0), int(r1), int(c0), int(c1))


def train_loss_device(pred, gt, lidar=None, correction=None, dataset="KITTI", gt_thr=None, in_thr=None, rows=None, cols=None):
    """The objective of train.py:210-251 (include/dtfill.h, dtfill_train_loss).  pred, gt and, with --correct, lidar and
    correction: contiguous float32 CUDA tensors [B,H,W].  dataset "KITTI": thresholds 0.1 / 0.1, whole frame, no root; "NYU":
    1e-4 / 1e-3, rows (6,228), cols (8,304), root; gt_thr, in_thr, rows and cols override the preset.  Returns the float64 CUDA
    tensor [6] = main, aux, n_gt, n_in, S_main, S_aux (_lib.LOSS_COLUMNS).  Asynchronous on the current stream, no host sync."""
    args = _loss_args(pred, gt, lidar, correction, dataset, gt_thr, in_thr, rows, cols)
    L = _lib.load()
    stats = torch.empty(len(_lib.LOSS_COLUMNS), dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        nbytes = L.dtfill_train_loss_workspace_bytes(*args[4:7])
        with _loss_ws.hold(pred.device, nbytes) as ws:
            _lib.check(L.dtfill_train_loss(*args, stats.data_ptr(), ws, nbytes, _stream(pred.device)))
    return stats


def train_loss_backward_device(pred, gt, stats, g_main=None, g_aux=None, lidar=None, correction=None, dataset="KITTI",
                               gt_thr=None, in_thr=None, rows=None, cols=None, want_pred=True, want_correction=None):
    """The gradients of g_main * main + g_aux * aux (include/dtfill.h, dtfill_train_loss_backward).  stats: what
    train_loss_device returned for the same arguments; g_main, g_aux: float32 CUDA scalars (one element), None for a zero
    gradient.  Returns (grad_pred, grad_corr): new tensors, None for one that was not asked for (want_correction defaults to
    "correction is given").  Asynchronous on the current stream, no host sync."""
    args = _loss_args(pred, gt, lidar, correction, dataset, gt_thr, in_thr, rows, cols)
    want_correction = correction is not None if want_correction is None else want_correction
    if want_correction and correction is None:
        raise ValueError("a gradient for correction needs correction")
    if not (want_pred or want_correction):
        raise ValueError("no gradient asked for")
    if stats.dtype != torch.float64 or stats.device != pred.device or stats.numel() != len(_lib.LOSS_COLUMNS) or not stats.is_contiguous():
        raise ValueError("stats must be train_loss_device's float64 [6] tensor on pred's device")
    for what, g in (("g_main", g_main), ("g_aux", g_aux)):
        if g is not None and (g.dtype != torch.float32 or g.device != pred.device or g.numel() != 1):
            raise ValueError("%s must be a float32 scalar on pred's device" % what)
    grad_pred = torch.empty_like(pred) if want_pred else None
    grad_corr = torch.empty_like(pred) if want_correction else None
    with torch.cuda.device(pred.device):
        _lib.check(_lib.load().dtfill_train_loss_backward(*args, stats.data_ptr(), _ptr(g_main), _ptr(g_aux), _ptr(grad_pred),
                                                          _ptr(grad_corr), _stream(pred.device)))
    return grad_pred, grad_corr


_fillb_ws = _Scratch()  # the fill backward's accumulators


def fill_backward_device(x, index, grad_depth, val_thr=0.1):
    """The backward of the exact fill depth = depth_list[index - 1] (include/dtfill.h, dtfill_fill_backward): the gradient with
    respect to x.  x: the forward's input; index: its "index" output (either metric); grad_depth: the gradient of its "depth"
    output.  x, grad_depth: contiguous float32 CUDA tensors [B,H,W]; index: contiguous int32, same shape and device.  Returns
    (grad_x, status): new tensors, status int32 [B] with _lib.FRAME_INDEX_ERROR for a frame whose gather would have raised (its
    gradient is all zeros).  Asynchronous on the current stream, no host synchronisation."""
    _require_gpu()
    _check_tensor(x, "x")
    _check_tensor(index, "index", torch.int32, like=x, like_name="x")
    _check_tensor(grad_depth, "grad_depth", like=x, like_name="x")
    B, H, W = x.shape
    L = _lib.load()
    nbytes = _sized(L.dtfill_fill_backward_workspace_bytes(B, H, W))
    grad_x = torch.empty_like(x)
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        with _fillb_ws.hold(x.device, nbytes) as ws:
            _lib.check(L.dtfill_fill_backward(x.data_ptr(), index.data_ptr(), grad_depth.data_ptr(), B, H, W, float(val_thr),
                                              grad_x.data_ptr(), status.data_ptr(), ws, nbytes, _stream(x.device)))
    return grad_x, status


_near_ws = _Scratch()  # the nearest gather's workspace (forward and backward)


def _check_near(x, index, payload, what):
    """The argument checks of the two nearest-gather calls (fill_backward_device's): x float32 [B,H,W], index int32 of x's
    shape, payload None or float32 [B,C,H,W] with x's frames, all contiguous CUDA tensors on x's device."""
    _check_tensor(x, "x")
    _check_tensor(index, "index", torch.int32, like=x, like_name="x")
    if payload is None:
        return 0
    _check_tensor(payload, what, layout="[B,C,H,W]")
    if payload.shape[0] != x.shape[0] or payload.shape[2:] != x.shape[1:] or payload.device != x.device:
        raise ValueError("%s must have x's frames [B,C,H,W] and device" % what)
    C = payload.shape[1]
    if not 1 <= C <= 64:
        raise ValueError("%s must have 1 to 64 channels, got %d" % (what, C))
    return C


def nearest_gather_device(x, index, values=None, src_thr=0.1, want_pixel=True):
    """Label -> source pixel (include/dtfill.h, dtfill_nearest_gather).  x: the tensor that decides the sources, NOT((1 - x) >
    src_thr); index: DtFill.run(x)'s "index" (either metric); values: None or [B,C,H,W], the channels to fill from the nearest
    source.  x, values: contiguous float32 CUDA tensors; index: contiguous int32 of x's shape [B,H,W], all on one device.
    Returns (filled or None, pixel or None, status): filled [B,C,H,W] holds values' bits at the nearest source (+0.0 where the
    label names none), pixel int32 [B,H,W] the source's flat pixel row*W + col (-1 where none), status int32 [B] the bits
    _lib.FRAME_NO_SOURCE and _lib.FRAME_INDEX_ERROR.  New tensors; asynchronous on the current stream, no host
    synchronisation."""
    C = _check_near(x, index, values, "values")
    if values is None and not want_pixel:
        raise ValueError("nothing to compute: values is None and want_pixel is False")
    _require_gpu()
    B, H, W = x.shape
    L = _lib.load()
    nbytes = _sized(L.dtfill_nearest_gather_workspace_bytes(B, H, W))
    filled = torch.empty_like(values) if values is not None else None
    pixel = torch.empty_like(index) if want_pixel else None
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        with _near_ws.hold(x.device, nbytes) as ws:
            _lib.check(L.dtfill_nearest_gather(x.data_ptr(), index.data_ptr(), _ptr(values), C, B, H, W, float(src_thr),
                                               _ptr(filled), _ptr(pixel), status.data_ptr(), ws, nbytes, _stream(x.device)))
    return filled, pixel, status


def nearest_gather_backward_device(x, index, grad_out, src_thr=0.1):
    """The backward of nearest_gather_device with respect to values (include/dtfill.h, dtfill_nearest_gather_backward): every
    source pixel receives, per channel, the cell sum of grad_out over the pixels whose label names it; every other pixel +0.0.
    x, index: as in the forward; grad_out: contiguous float32 CUDA tensor [B,C,H,W].  Returns (grad_values, status): new
    tensors, bitwise reproducible.  Asynchronous on the current stream, no host synchronisation."""
    if grad_out is None:
        raise ValueError("grad_out must be a contiguous float32 CUDA tensor [B,C,H,W]")
    C = _check_near(x, index, grad_out, "grad_out")
    _require_gpu()
    B, H, W = x.shape
    L = _lib.load()
    nbytes = _sized(L.dtfill_nearest_gather_backward_workspace_bytes(B, H, W, C))
    grad_values = torch.empty_like(grad_out)
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        with _near_ws.hold(x.device, nbytes) as ws:
            _lib.check(L.dtfill_nearest_gather_backward(x.data_ptr(), index.data_ptr(), grad_out.data_ptr(), C, B, H, W,
                                                        float(src_thr), grad_values.data_ptr(), status.data_ptr(), ws, nbytes,
                                                        _stream(x.device)))
    return grad_values, status


def keep_every_of(keep_ratio):
    """1 / keep_ratio as the integer the kernel takes (sample()'s `label % (1.0 / keep_ratio) == 0`): 0.5 -> 2 (the
    reference's 32-line input), 0.25 -> 4 (16 lines).  ValueError unless 1 / keep_ratio is an integer >= 1."""
    try:
        inv = 1.0 / float(keep_ratio)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError("keep_ratio must be a number whose inverse is an integer >= 1, got %r" % (keep_ratio,)) from None
    if not (np.isfinite(inv) and inv >= 1.0 and inv == np.round(inv) and inv < 2 ** 31):
        raise ValueError("keep_ratio must be 1/k for an integer k >= 1, got %r" % (keep_ratio,))
    return int(inv)


def _calibration(m, n, B, device, what):
    """[n,n] (broadcast to B) or [B,n,n], numpy or tensor of any real dtype -> contiguous float64 CUDA tensor [B,n,n]."""
    t = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.asarray(m, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64)
    if t.dim() == 2 and tuple(t.shape) == (n, n):
        t = t.unsqueeze(0).expand(B, n, n)
    if tuple(t.shape) != (B, n, n):
        raise ValueError("%s must be [%d,%d] or [B,%d,%d] with B = %d, got shape %s" % (what, n, n, n, n, B, tuple(t.shape)))
    return t.contiguous()


def line_subsample_device(x, K, E, keep_ratio=0.25, n_bins=64):
    """subsample_Lidar_{train,val}.py's get_all_points -> calculate_angle -> sample -> map_points_on_image on the device
    (include/dtfill.h, dtfill_line_subsample): keep the valid pixels whose pitch bin (n_bins equal bins over the frame's
    pitch range) is a multiple of 1 / keep_ratio.  x: contiguous float32 CUDA tensor [B,H,W]; K: intrinsics [3,3] or
    [B,3,3]; E: velo->cam extrinsics [4,4] or [B,4,4] (numpy or tensors, any real dtype; used in float64).
    Returns (out float32 [B,H,W] -- kept pixels hold their input value, the others +0.0 --, status int32 [B], bits
    _lib.LINES_*; a frame with a bit set is all zeros)."""
    keep_every = keep_every_of(keep_ratio)
    if int(n_bins) != n_bins or n_bins < 1:
        raise ValueError("n_bins must be an integer >= 1, got %r" % (n_bins,))
    _require_gpu()
    _check_tensor(x, "x")
    B, H, W = x.shape
    Kd = _calibration(K, 3, B, x.device, "K")
    Ed = _calibration(E, 4, B, x.device, "E")
    L = _lib.load()
    nbytes = _sized(L.dtfill_line_subsample_workspace_bytes(B, H, W))
    ws, ws_ptr = _workspace(nbytes, x.device)
    out = torch.empty_like(x)
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.dtfill_line_subsample(x.data_ptr(), B, H, W, Kd.data_ptr(), Ed.data_ptr(), int(n_bins), keep_every,
                                           out.data_ptr(), status.data_ptr(), ws_ptr, nbytes, _stream(x.device)))
    return out, status


def _read_size(size, what="size"):
    """PIL's (width, height) -> (H, W) as ints >= 1."""
    try:
        W, H = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s must be (width, height), got %r" % (what, size)) from None
    if W < 1 or H < 1 or (W, H) != tuple(size):
        raise ValueError("%s must be two integers >= 1 in PIL's (width, height) order, got %r" % (what, size))
    return H, W


def _dims_arg(dims, B, device):
    """The reads' `dims`: (h_b, w_b) per frame as numpy, list or tensor -> contiguous int32 tensor [B, 2] on `device`; None
    (every frame fills its slot) stays None."""
    if dims is None:
        return None
    d = dims if isinstance(dims, torch.Tensor) else torch.from_numpy(np.asarray(dims, dtype=np.int32))
    d = d.to(device=device, dtype=torch.int32).contiguous()
    if tuple(d.shape) != (B, 2):
        raise ValueError("dims must be [B, 2] = [%d, 2], got shape %s" % (B, tuple(d.shape)))
    return d


def _first_row(first_row, H):
    """The first row an rgb read keeps, as an int in [0, H)."""
    if first_row != int(first_row) or not 0 <= first_row < H:
        raise ValueError("first_row must be an integer in [0, %d), got %r" % (H, first_row))
    return int(first_row)


def depth_read_device(raw, dims=None, size=(1216, 352)):
    """data_read.py:81-99 after the PNG decode, on the device (include/dtfill.h, dtfill_depth_read): the values / 256 and
    Pillow's NEAREST resize to size = (width, height), PIL's order as data_read.py:96 writes it.  raw: contiguous uint16
    CUDA tensor [B, hmax, wmax]; dims: (h_b, w_b) per frame as int [B, 2] (numpy, list or tensor; None: every frame
    hmax x wmax), the padding beyond them is never read.  Returns (out float32 [B, H, W], status int32 [B], bits
    _lib.READ_*: NOT_16BIT where every value of the frame is <= 255, the reference's assert; BAD_DIMS, with an all-zero
    frame, for dims outside [1, hmax] x [1, wmax]).  Asynchronous on the current stream; out feeds DtFill.run as it is."""
    _require_gpu()
    _check_tensor(raw, "raw", torch.uint16, "[B,hmax,wmax]")
    H, W = _read_size(size)
    B, hmax, wmax = raw.shape
    d = _dims_arg(dims, B, raw.device)
    L = _lib.load()
    nbytes = _sized(L.dtfill_depth_read_workspace_bytes(B, H, W))
    ws, ws_ptr = _workspace(nbytes, raw.device)
    out = torch.empty((B, H, W), dtype=torch.float32, device=raw.device)
    status = torch.empty((B,), dtype=torch.int32, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(L.dtfill_depth_read(raw.data_ptr(), _ptr(d), B, hmax, wmax, H, W, out.data_ptr(), status.data_ptr(), ws_ptr,
                                       nbytes, _stream(raw.device)))
    return out, status


RGB_WANT = ("float", "uint8", "both")
RGB_LAYOUTS = {"nhwc": _lib.RGB_NHWC, "nchw": _lib.RGB_NCHW}


def rgb_read_device(raw, dims=None, size=(1216, 352), first_row=0, want="float", layout="nhwc", normalize=True):
    """data_read.py:66-73 after the PNG decode, and the drivers' rgb = img_batch[:, first_row:] / 255.0 as float32
    (train.py:213-214 and its kin), on the device (include/dtfill.h, dtfill_rgb_read): Pillow's NEAREST resize of uint8
    images to size = (width, height), PIL's order.  raw: contiguous uint8 CUDA tensor [B, hmax, wmax, C], C in 1..4; dims:
    (h_b, w_b) per frame as int [B, 2] (numpy, list or tensor; None: every frame hmax x wmax), the padding beyond them is
    never read.  want: "float", "uint8" or "both"; layout of the float output: "nhwc" [B, H - first_row, W, C] (what
    demo_multi_channel_device takes as rgb) or "nchw" [B, C, H - first_row, W] (nearest_gather_device's values);
    normalize=False keeps (float)v.  Returns (uint8 [B, H - first_row, W, C] or None, float32 or None, status int32 [B]:
    _lib.READ_BAD_DIMS, with an all-zero frame, for dims outside [1, hmax] x [1, wmax]).  New tensors, asynchronous on the
    current stream."""
    _require_gpu()
    _check_tensor(raw, "raw", torch.uint8, "[B,hmax,wmax,C]")
    if want not in RGB_WANT:
        raise ValueError("want must be one of %s, got %r" % (RGB_WANT, want))
    if layout not in RGB_LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (sorted(RGB_LAYOUTS), layout))
    H, W = _read_size(size)
    B, hmax, wmax, C = raw.shape
    first_row = _first_row(first_row, H)
    d = _dims_arg(dims, B, raw.device)
    L = _lib.load()
    nbytes = _sized(L.dtfill_rgb_read_workspace_bytes(B, H, W))
    ws, ws_ptr = _workspace(nbytes, raw.device)
    OH = H - first_row
    u8 = f32 = None
    if want != "float":
        u8 = torch.empty((B, OH, W, C), dtype=torch.uint8, device=raw.device)
    if want != "uint8":
        f32 = torch.empty((B, OH, W, C) if layout == "nhwc" else (B, C, OH, W), dtype=torch.float32, device=raw.device)
    status = torch.empty((B,), dtype=torch.int32, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(L.dtfill_rgb_read(raw.data_ptr(), _ptr(d), B, hmax, wmax, C, H, W, first_row, 1 if normalize else 0,
                                     RGB_LAYOUTS[layout], _ptr(u8), _ptr(f32), status.data_ptr(), ws_ptr, nbytes,
                                     _stream(raw.device)))
    return u8, f32, status


def __getattr__(name):
    # the point projection's device function is defined in projection.py (which imports this module's helpers)
    if name in ("project_points_device", "unproject_device", "unproject_backward_device"):
        from . import projection

        return getattr(projection, name)
    if name == "nyu_read_device":  # likewise in nyu.py
        from . import nyu

        return nyu.nyu_read_device
    if name in ("conv2d_device", "conv2d_strided_device", "conv2d_transpose_device", "conv2d_backward_data_device",
                "conv2d_backward_weights_device", "conv2d_backward_workspace_bytes", "conv2d_strided_backward_data_device",
                "conv2d_strided_backward_weights_device", "conv2d_transpose_backward_data_device",
                "conv2d_transpose_backward_weights_device", "conv2d_wide_backward_workspace_bytes", "conv2d_image_device",
                "conv2d_image_backward_weights_device", "conv2d_image_backward_workspace_bytes", "pack_bf16_device",
                "conv2d_strided_bf16_device", "conv2d_transpose_bf16_device", "conv2d_strided_bf16",
                "conv2d_transpose_bf16", "conv2d_strided_backward_data_bf16_device", "conv2d_strided_backward_weights_bf16_device", "conv2d_transpose_backward_data_bf16_device",
                "conv2d_transpose_backward_weights_bf16_device", "conv2d_wide_backward_bf16_workspace_bytes"):  # likewise in conv.py
        from . import conv

        return getattr(conv, name)
    if name in ("max_pool_pyramid_device", "max_pool_pyramid_backward_device"):  # likewise in pool.py
        from . import pool

        return getattr(pool, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


_default_ops = {}
_default_ops_lock = threading.Lock()


def default_op(metric="l1_cv"):
    """The process-wide operator of the current CUDA device and the current stream (what the reference-named functions and the
    autograd operators use).  One per stream: passes on different streams run beside each other in workspaces of their own, and
    an operator's buffers are always used on the stream they were allocated under.  Host threads on one stream share the
    operator and serialise on its lock (DtFill).  Like the workspaces of the other entry points, an operator stays for the life
    of the process: a caller that goes through many short-lived streams constructs a DtFill of its own instead."""
    _require_gpu()
    dev = torch.cuda.current_device()
    key = (dev, _stream(dev), metric)
    with _default_ops_lock:
        op = _default_ops.get(key)
        if op is None:
            op = _default_ops[key] = DtFill(metric=metric)
    return op


def fill(x, src_thr=0.1, val_thr=0.1, metric="l1_cv", want=WANT_ALL):
    """Batched numpy API: x [B,H,W] float32 -> dict(depth, dt, index, status)."""
    return default_op(metric).run_numpy(x, src_thr, val_thr, want)

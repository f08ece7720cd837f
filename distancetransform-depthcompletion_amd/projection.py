"""Device-side plumbing of the LiDAR point projection (include/dtfill.h, dtfill_project_points): point clouds in, sparse depth
frames out, and of its inverse (dtfill_unproject, dtfill_unproject_backward): frames in, ordered point clouds out.  Reached as
device.project_points_device, device.unproject_device and device.unproject_backward_device as well; it lives here, beside device.py's helpers, with its argument
checks tabled in tests/test_gpu_project_points.py.
"""
import numpy as np
import torch

from . import _lib
from .device import _calibration, _check_tensor, _ptr, _require_gpu, _sized, _stream, _workspace

PROJ_MODES = {"reference": _lib.PROJ_REFERENCE, "zbuffer": _lib.PROJ_ZBUFFER}
PROJ_WANT = ("float32", "float64", "both")


def _frame_hw(hw):
    """(H, W) of the output frames as ints >= 1."""
    try:
        H, W = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError("hw must be (H, W), got %r" % (hw,)) from None
    if H < 1 or W < 1 or (H, W) != tuple(hw):
        raise ValueError("hw must be two integers >= 1, (H, W), got %r" % (hw,))
    return H, W


def _counts_arg(counts, B, device):
    """n_b per frame as numpy, list or tensor -> contiguous int32 tensor [B] on `device`; None (every frame holds N records)
    stays None."""
    if counts is None:
        return None
    c = counts if isinstance(counts, torch.Tensor) else torch.from_numpy(np.asarray(counts, dtype=np.int32))
    c = c.to(device=device, dtype=torch.int32).contiguous()
    if tuple(c.shape) != (B,):
        raise ValueError("counts must be [B] = [%d], got shape %s" % (B, tuple(c.shape)))
    return c


def project_points_device(points, counts, K, E, hw, mode="zbuffer", min_z=0.0, want="float32"):
    """subsample_Lidar_{train,val}.py's map_points_on_image on the device, for B clouds at once, and its z-buffered form
    (include/dtfill.h, dtfill_project_points).  points: contiguous float32 CUDA tensor [B, N, 3 or 4] in the Velodyne frame
    (the 4th float, KITTI's reflectance, is carried and ignored); counts: the records in use per frame as int [B] (numpy, list
    or tensor; None: N everywhere), the padding beyond them is never read; K: intrinsics [3,3] or [B,3,3]; E: velo->cam
    extrinsics [4,4] or [B,4,4] (numpy or tensors, any real dtype; used in float64); hw = (H, W) of the frames.  mode "zbuffer":
    the nearest return per pixel, points with z <= min_z or outside the frame dropped; "reference": the reference's in-order
    assignment, last writer wins, negative indices wrap.  Returns (frame float32 [B,H,W], status int32 [B]: bits
    _lib.PROJ_*, a frame with INDEX_ERROR or BAD_COUNT is all zeros, counts4 int32 [B,4]: _lib.PROJ_COLUMNS); with want =
    "float64" or "both" a fourth element, the float64 map the reference returns (and frame is None for "float64").  New
    tensors, asynchronous on the current stream; frame feeds DtFill.run as it is."""
    _require_gpu()
    _check_tensor(points, "points", layout="[B,N,stride]")
    B, N, stride = points.shape
    if stride not in (3, 4):
        raise ValueError("points must hold 3 or 4 floats per record, got %d" % stride)
    if mode not in PROJ_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(PROJ_MODES), mode))
    if want not in PROJ_WANT:
        raise ValueError("want must be one of %s, got %r" % (PROJ_WANT, want))
    H, W = _frame_hw(hw)
    min_z = float(min_z)
    if not (np.isfinite(min_z) and min_z >= 0.0):
        raise ValueError("min_z must be finite and >= 0, got %r" % (min_z,))
    c = _counts_arg(counts, B, points.device)
    Kd = _calibration(K, 3, B, points.device, "K")
    Ed = _calibration(E, 4, B, points.device, "E")
    L = _lib.load()
    nbytes = _sized(L.dtfill_project_points_workspace_bytes(B, N, H, W))
    ws, ws_ptr = _workspace(nbytes, points.device)
    f32 = torch.empty((B, H, W), dtype=torch.float32, device=points.device) if want != "float64" else None
    f64 = torch.empty((B, H, W), dtype=torch.float64, device=points.device) if want != "float32" else None
    status = torch.empty((B,), dtype=torch.int32, device=points.device)
    counts4 = torch.empty((B, len(_lib.PROJ_COLUMNS)), dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        _lib.check(L.dtfill_project_points(points.data_ptr(), _ptr(c), B, N, stride, H, W, Kd.data_ptr(), Ed.data_ptr(),
                                           PROJ_MODES[mode], min_z, _ptr(f32), _ptr(f64), status.data_ptr(), counts4.data_ptr(),
                                           ws_ptr, nbytes, _stream(points.device)))
    return (f32, status, counts4) if want == "float32" else (f32, status, counts4, f64)


UNPROJ_WANT = ("pitch", "pixel")


def unproject_device(x, K, E, val_thr=0.1, payload=None, capacity=None, stride=None, keep_ratio=None, n_bins=64, want=("pixel",)):
    """The inverse of project_points_device (include/dtfill.h, dtfill_unproject): depth frames to ordered point clouds in the
    Velodyne frame, get_all_points of subsample_Lidar_{train,val}.py, and with keep_ratio its `left_points` (get_all_points ->
    calculate_angle -> sample).  x: contiguous float32 CUDA tensor [B,H,W]; a pixel is a point iff x > val_thr in float32.
    payload: like x, a scalar per pixel carried into the fourth float of its record.  capacity: records per frame in the
    output (default H*W: every frame fits); stride: floats per record (default 3, 4 with a payload; 4 without one carries
    +0.0).  keep_ratio: None for every valid pixel, else 1/k as line_subsample_device takes it, with n_bins.  want: which of
    "pitch" (float64 [B,N]) and "pixel" (int32 [B,N], row*W + col) to return besides.  Returns (points float32
    [B,N,stride], counts int32 [B,2]: _lib.UNPROJ_WRITTEN, _lib.UNPROJ_TOTAL, status int32 [B]: bits _lib.UNPROJ_*, pitch or
    None, pixel or None).  A frame's points come in raster order; records beyond counts[b, written] are not written (the
    tensors are torch.empty).  points and counts[:, 0] feed project_points_device as they are.  New tensors, asynchronous on
    the current stream, no host synchronisation."""
    _require_gpu()
    _check_tensor(x, "x")
    if payload is not None:
        _check_tensor(payload, "payload", like=x, like_name="x")
    B, H, W = x.shape
    val_thr = float(val_thr)
    if np.isnan(val_thr):
        raise ValueError("val_thr must not be NaN")
    if stride is None:
        stride = 3 if payload is None else 4
    if stride not in (3, 4) or (payload is not None and stride != 4):
        raise ValueError("stride must be 3 or 4, and 4 with a payload, got %r" % (stride,))
    N = H * W if capacity is None else capacity
    if int(N) != N or N < 1:
        raise ValueError("capacity must be an integer >= 1, got %r" % (capacity,))
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in UNPROJ_WANT for w in want):
        raise ValueError("want must be drawn from %s, got %r" % (UNPROJ_WANT, want))
    keep_every = 0
    if keep_ratio is not None:
        from .device import keep_every_of

        keep_every = keep_every_of(keep_ratio)
        if int(n_bins) != n_bins or n_bins < 1:
            raise ValueError("n_bins must be an integer >= 1, got %r" % (n_bins,))
    N = int(N)
    Kd = _calibration(K, 3, B, x.device, "K")
    Ed = _calibration(E, 4, B, x.device, "E")
    L = _lib.load()
    nbytes = _sized(L.dtfill_unproject_workspace_bytes(B, H, W))
    ws, ws_ptr = _workspace(nbytes, x.device)
    points = torch.empty((B, N, stride), dtype=torch.float32, device=x.device)
    pitch = torch.empty((B, N), dtype=torch.float64, device=x.device) if "pitch" in want else None
    pixel = torch.empty((B, N), dtype=torch.int32, device=x.device) if "pixel" in want else None
    counts = torch.empty((B, 2), dtype=torch.int32, device=x.device)
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.dtfill_unproject(x.data_ptr(), _ptr(payload), B, H, W, val_thr, Kd.data_ptr(), Ed.data_ptr(),
                                      int(n_bins) if keep_every else 0, keep_every, N, stride, points.data_ptr(), _ptr(pitch),
                                      _ptr(pixel), counts.data_ptr(), status.data_ptr(), ws_ptr, nbytes, _stream(x.device)))
    return points, counts, status, pitch, pixel


def unproject_backward_device(grad_points, pixel, counts, K, E, hw, want_payload=False):
    """The backward of unproject_device (include/dtfill.h, dtfill_unproject_backward): grad_points float32 [B,N,stride], the
    gradient with respect to the records; pixel int32 [B,N] and counts int32 [B,2] as the forward returned them; hw = (H, W).
    Returns (grad_x float32 [B,H,W], grad_payload float32 [B,H,W] or None, status int32 [B]: _lib.UNPROJ_SINGULAR,
    UNPROJ_BAD_PIXEL, UNPROJ_BAD_COUNT; a frame with a bit set has zero gradients).  The map is affine in the depth, so x is
    not an argument.  New tensors, asynchronous on the current stream, no host synchronisation."""
    _require_gpu()
    _check_tensor(grad_points, "grad_points", layout="[B,N,stride]")
    B, N, stride = grad_points.shape
    if stride not in (3, 4) or (want_payload and stride != 4):
        raise ValueError("grad_points must hold 3 or 4 floats per record, 4 with want_payload, got %d" % stride)
    _check_tensor(pixel, "pixel", dtype=torch.int32, layout="[B,N]")
    _check_tensor(counts, "counts", dtype=torch.int32, layout="[B,2]")
    if tuple(pixel.shape) != (B, N) or tuple(counts.shape) != (B, 2) or pixel.device != grad_points.device or \
            counts.device != grad_points.device:
        raise ValueError("pixel must be [B,N] = [%d,%d] and counts [B,2], on grad_points' device" % (B, N))
    H, W = _frame_hw(hw)
    dev = grad_points.device
    Kd = _calibration(K, 3, B, dev, "K")
    Ed = _calibration(E, 4, B, dev, "E")
    L = _lib.load()
    nbytes = _sized(L.dtfill_unproject_backward_workspace_bytes(B, H, W))
    ws, ws_ptr = _workspace(nbytes, dev)
    grad_x = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    grad_payload = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_payload else None
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.dtfill_unproject_backward(grad_points.data_ptr(), pixel.data_ptr(), counts.data_ptr(), B, N, stride, H, W,
                                               Kd.data_ptr(), Ed.data_ptr(), grad_x.data_ptr(), _ptr(grad_payload),
                                               status.data_ptr(), ws_ptr, nbytes, _stream(dev)))
    return grad_x, grad_payload, status

"""Device-side plumbing of the LiDAR point projection (include/dtfill.h, dtfill_project_points): point clouds in, sparse depth
frames out.  Reached as device.project_points_device as well; it lives here, beside device.py's helpers, with its argument
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

"""Device-side plumbing of the NYU loaders' per-sample work (include/dtfill.h, dtfill_nyu_read): stored images and dense depths
in, resized image, ground truth and sampled depth out.  Reached as device.nyu_read_device as well; it lives here, beside
device.py's helpers, with its argument checks tabled in tests/test_gpu_nyu_read.py.
"""
import torch

from . import _lib
from .device import RGB_LAYOUTS, _check_tensor, _ptr, _require_gpu, _sized, _stream, _workspace
from .tools import nyu_taps


def _nyu_size(size, h, w):
    """skimage's output_shape (rows, cols) -> (H, W) as ints in [1, h] x [1, w]: the stage reduces, it never enlarges."""
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (rows, cols), got %r" % (size,)) from None
    if (H, W) != tuple(size) or not (1 <= H <= h and 1 <= W <= w):
        raise ValueError("size must be two integers (rows, cols) within [1, %d] x [1, %d], got %r" % (h, w, size))
    return H, W


def nyu_read_device(rgb, depth, samples=None, size=(240, 320), normalize=False, layout="nhwc"):
    """What the reference's NYU loaders do to a stored sample (data_read.py:307-330 and its copies), on the device
    (include/dtfill.h, dtfill_nyu_read): skimage's anti-aliased resize of the image and the dense depth to size = (rows,
    cols) -- a Gaussian pre-filter and a linear resample, scipy.ndimage's arithmetic bit for bit --, rgb * 255, and
    lidar = gt * Mask.  rgb: contiguous uint8 CUDA tensor [B, C, h, w], the stored layout, C in 1..4, or None; depth:
    contiguous float32 [B, h, w] or None (not both None); samples: int32 [B, n, 2] of (row, col) with the loaders' + 6 / + 8
    added, or None for no sample.  normalize=True gives the drivers' rgb / 255.0 as float32 (eval_NYU.py:164-165); layout of
    the image: "nhwc" [B, H, W, C] (the reference's) or "nchw".  Returns (rgb float32 or None, gt float32 [B, H, W] or None,
    lidar float32 [B, H, W] or None, status int32 [B]: _lib.NYU_INDEX_ERROR where a sample lies outside the frame; it was
    skipped, numpy would have raised IndexError).  New tensors, asynchronous on the current stream; gt and lidar feed
    DtFill.run and train_loss_device as they are."""
    _require_gpu()
    if rgb is None and depth is None:
        raise ValueError("rgb and depth are both None")
    if layout not in RGB_LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (sorted(RGB_LAYOUTS), layout))
    if rgb is not None:
        _check_tensor(rgb, "rgb", torch.uint8, "[B,C,h,w]")
    if depth is not None:
        _check_tensor(depth, "depth", torch.float32, "[B,h,w]")
    first = rgb if rgb is not None else depth
    B, (h, w) = first.shape[0], first.shape[-2:]
    C = rgb.shape[1] if rgb is not None else 1
    if rgb is not None and depth is not None and (tuple(depth.shape) != (B, h, w) or depth.device != rgb.device):
        raise ValueError("depth must be [B, h, w] = [%d, %d, %d] on rgb's device, got %s" % (B, h, w, tuple(depth.shape)))
    n = 0
    if samples is not None:
        _check_tensor(samples, "samples", torch.int32, "[B,n,2]")
        if samples.shape[0] != B or samples.shape[2] != 2 or samples.device != first.device:
            raise ValueError("samples must be [B, n, 2] = [%d, n, 2] on the frames' device, got %s" % (B, tuple(samples.shape)))
        n = samples.shape[1]
    H, W = _nyu_size(size, h, w)
    (wy, ry), (wx, rx) = nyu_taps(h, H), nyu_taps(w, W)
    if max(ry, rx) > _lib.NYU_MAX_RADIUS:
        raise ValueError("a reduction of (%d, %d) to (%d, %d) needs a filter radius of %d; the kernel holds %d"
                         % (h, w, H, W, max(ry, rx), _lib.NYU_MAX_RADIUS))
    L = _lib.load()
    nbytes = _sized(L.dtfill_nyu_read_workspace_bytes(B, H, W))
    dev = first.device
    ws, ws_ptr = _workspace(nbytes, dev)
    out = gt = lidar = None
    if rgb is not None:
        out = torch.empty((B, H, W, C) if layout == "nhwc" else (B, C, H, W), dtype=torch.float32, device=dev)
    if depth is not None:
        gt = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        lidar = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    taps = lambda t: None if t is None else t.ctypes.data  # host pointers, read before the call returns
    with torch.cuda.device(dev):
        _lib.check(L.dtfill_nyu_read(_ptr(rgb), _ptr(depth), B, C, h, w, H, W, taps(wy), ry, taps(wx), rx, _ptr(samples), n,
                                     1 if normalize else 0, RGB_LAYOUTS[layout], _ptr(out), _ptr(gt), _ptr(lidar),
                                     status.data_ptr(), ws_ptr, nbytes, _stream(dev)))
    return out, gt, lidar, status

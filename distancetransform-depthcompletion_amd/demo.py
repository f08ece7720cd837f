"""Drop-in mirror of the module-level functions of the reference's demo driver (numpy in, numpy out).

Same names and argument meaning as
  solution_DeepNet/demo.py:65-75     create_weight_matrix (powers of ten, not net.py's linear weights)
  solution_DeepNet/demo.py:108-149   generate_multi_channel
  solution_DeepNet/demo.py:151-198   generate_multi_channel_with_image
which demo.py calls at :309-313 with its default --model_type DT; the work is done by libdtfill.so on the current HIP
device (include/dtfill.h, dtfill_demo_multi_channel, states the arithmetic).  These are not the net.py:83-122 form behind
the package's top-level generate_multi_channel.  Differences from the reference, all widening: any batch size B >= 1 (the
reference's np.squeeze only admits B = 1), numpy arrays come back where the reference returns TF tensors, and a scale_num
outside 1..4 raises ValueError where the reference returns None.
"""
import numpy as np

from . import device as _device
from .tools import _as_f32_frames


def create_weight_matrix(size=11):
    """demo.py:65-75: float32 [size * size] in row-major tap order, ten to the power size - |di| - |dj| for the tap at offset
    (di, dj) from the centre, rounded from double to float32 once.  Host arithmetic, as in the reference; the kernels hold
    the same float32 constants."""
    assert size % 2 == 1, "create_weight_matrix needs an odd size"
    ring = np.abs(np.arange(size) - (size - 1) // 2)
    exponent = size - np.add.outer(ring, ring)
    return np.float32(np.power(10.0, exponent.astype(np.float64))).ravel()


def _run(rgb_data, lidar_data, table_size, scale_range, scale_num):
    import torch

    if scale_num not in (1, 2, 3, 4):
        raise ValueError("scale_num must be 1, 2, 3 or 4, got %r" % (scale_num,))
    d = _as_f32_frames(lidar_data)
    if d.ndim != 4 or d.shape[-1] != 1:
        raise ValueError("lidar_data must be [B,H,W,1], got shape %s" % (d.shape,))
    rgb = None
    if rgb_data is not None:
        rgb = _as_f32_frames(rgb_data)
        if rgb.ndim != 4 or rgb.shape[:3] != d.shape[:3] or rgb.shape[3] < 1:
            raise ValueError("rgb_data must be [B,H,W,C] over lidar_data's frames %s, got shape %s" % (d.shape[:3], rgb.shape))
    dev = _device.default_op().device
    dd = torch.from_numpy(np.ascontiguousarray(d[..., 0])).to(dev)
    rr = None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)
    outs = _device.demo_multi_channel_device(dd, rr, table_size, scale_range, scale_num)
    return tuple(None if o is None else o.cpu().numpy() for o in outs)


def generate_multi_channel(lidar_data, table_size, scale_range=90.0, scale_num=4):
    """demo.py:108-149: lidar_data [B,H,W,1] -> (lidar_1, .., lidar_4) / scale_range, each float32 [B,H,W], None beyond
    scale_num."""
    return _run(None, lidar_data, table_size, scale_range, scale_num)


def generate_multi_channel_with_image(rgb_data, lidar_data, table_size, scale_range=90.0, scale_num=4):
    """demo.py:151-198: rgb_data [B,H,W,C], lidar_data [B,H,W,1] -> four float32 [B,H,W,C+1], None beyond scale_num:
    concat([rgb, lidar_k / scale_range], 3) / scale_range -- the lidar channel is divided twice, as in the reference."""
    return _run(rgb_data, lidar_data, table_size, scale_range, scale_num)

"""MI355X-native distance-transform + nearest-valid-depth fill operator.

Drop-in for the preprocessing path of placeforyiming/DistanceTransform-DepthCompletion
(solution_DeepNet/tools.py, demo.py:78-106, eval_NYU.py:114-133): same function names, numpy in /
numpy out, computed by hand-written gfx950 HIP kernels behind the C ABI of include/dtfill.h.

The directory name contains a '-', so import it with
    importlib.import_module("distancetransform-depthcompletion_amd")
or through the `dtfill_amd` alias module at the repository root.
"""
from . import _lib
from ._lib import METRICS, DtfillError, build, load
from .sharding import shard_range, gather_frames, fill_sharded, release_host_slab
from .tools import DT_complete_batch, Distance_Transform, generate_multi_channel, nearest_point, outlier_removal, subsample_lidar
from .tools import depth_read, depth_read_batch, nearest_source, rgb_read, rgb_read_batch
from .tools import map_points_on_image, project_points
from .tools import get_all_points, unproject_frames
from .tools import nyu_read_batch, nyu_taps
from .tools import conv2d, max_pool
from . import demo  # demo.py's own generate_multi_channel / _with_image / create_weight_matrix, reached as <package>.demo.*
from .postfill import Result, Result_NYU, depth_floor, depth_to_png16, kitti_rows, nyu_eval_crop


def __getattr__(name):
    # device.py imports torch; keep `import package` cheap for tooling that only needs the ABI
    if name in ("DtFill", "fill", "default_op", "rgb_read_device", "device"):
        import importlib

        mod = importlib.import_module(__name__ + ".device")
        return mod if name == "device" else getattr(mod, name)
    if name in ("project_points_device", "unproject_device", "unproject_backward_device"):
        import importlib

        return getattr(importlib.import_module(__name__ + ".projection"), name)
    if name == "nyu_read_device":
        import importlib

        return importlib.import_module(__name__ + ".nyu").nyu_read_device
    if name in ("conv2d_strided", "conv2d_transpose", "conv2d_image", "pack_transpose_kernel",  # numpy forms of the wide and image convolutions
                "conv2d_strided_bf16", "conv2d_transpose_bf16", "pack_bf16_device", "conv2d_strided_bf16_device",
                "conv2d_transpose_bf16_device",  # and the bf16 forms of the wide ones, forward and backward
                "conv2d_strided_backward_data_bf16_device", "conv2d_strided_backward_weights_bf16_device", "conv2d_transpose_backward_data_bf16_device",
                "conv2d_transpose_backward_weights_bf16_device", "conv2d_wide_backward_bf16_workspace_bytes",
                "conv2d_strided_backward_data_bf16", "conv2d_strided_backward_weights_bf16", "conv2d_transpose_backward_data_bf16",
                "conv2d_transpose_backward_weights_bf16"):
        import importlib

        return getattr(importlib.import_module(__name__ + ".conv"), name)
    if name == "net":  # <package>.net: the networks, inference classes and their torch.nn.Module forms; imports torch
        import importlib

        return importlib.import_module(__name__ + ".net")
    if name == "autograd":  # <package>.autograd.generate_multi_channel (net.py form) and .train_loss (imports torch too)
        import importlib

        return importlib.import_module(__name__ + ".autograd")
    if name == "optim":  # <package>.optim.KerasAdam, adam_step_device and the numpy adam_step: train.py's optimizer (imports torch)
        import importlib

        return importlib.import_module(__name__ + ".optim")
    raise AttributeError(name)


__all__ = [
    "nearest_point", "DT_complete_batch", "Distance_Transform", "outlier_removal", "generate_multi_channel", "subsample_lidar",
    "depth_read", "depth_read_batch", "rgb_read", "rgb_read_batch", "rgb_read_device", "nearest_source",
    "map_points_on_image", "project_points", "project_points_device", "get_all_points", "unproject_frames",
    "unproject_device", "unproject_backward_device", "nyu_read_batch", "nyu_read_device", "nyu_taps",
    "conv2d", "max_pool", "conv2d_strided", "conv2d_transpose", "conv2d_image", "pack_transpose_kernel", "conv2d_strided_bf16",
    "conv2d_transpose_bf16", "pack_bf16_device", "conv2d_strided_bf16_device", "conv2d_transpose_bf16_device", "net", "optim", "demo", "fill", "DtFill",
    "shard_range", "gather_frames", "fill_sharded", "release_host_slab", "build", "load", "METRICS", "DtfillError",
    "Result", "Result_NYU", "depth_floor", "depth_to_png16", "kitti_rows", "nyu_eval_crop",
]

"""ctypes binding of libdtfill.so (the C ABI declared in include/dtfill.h).

The HIP library is the product: there is no CPU fallback here.  If the shared object is missing
or cannot be loaded, every entry point raises -- loudly -- instead of computing something else.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "libdtfill.so")

METRIC_L1_CV = 0
METRIC_L2 = 1
METRICS = {"l1_cv": METRIC_L1_CV, "l2": METRIC_L2}

FRAME_OK = 0
FRAME_INDEX_ERROR = 1  # bit
FRAME_GENERAL_PATH = 2  # bit, informational
FRAME_NO_SOURCE = 4  # bit (nearest_gather): the frame has no source pixel
FLAG_GENERAL_ONLY = 1
FLAG_FUSED_ONLY = 2
FLAG_OUTLIER_REMOVAL = 4  # outlier_removal() (data_read.py:103-128) in front of the predicates
FLAG_SEPARATE_FRAME = 8  # l1_cv: the frame facts in a k_frame launch of their own (tests, A/B timing); same results
LINES_NO_POINTS = 1  # bit: no valid pixel in the frame (DTFILL_LINES_*)
LINES_BAD_INTERVAL = 2  # bit: the pitch interval is 0 or not finite
LINES_SINGULAR = 4  # bit: K or E is singular
READ_NOT_16BIT = 1  # bit: every source value of the frame is <= 255 (DTFILL_READ_*)
READ_BAD_DIMS = 2  # bit: the frame's dims lie outside [1, hmax] x [1, wmax]; its output is all zeros
RGB_NHWC = 0  # out_f32 [B, H - first_row, W, C] (DTFILL_RGB_*)
RGB_NCHW = 1  # out_f32 [B, C, H - first_row, W]
NYU_MAX_RADIUS = 8  # the largest filter radius per axis dtfill_nyu_read takes (DTFILL_NYU_*)
NYU_INDEX_ERROR = 1  # bit: a sample of the frame lies outside it and was skipped; numpy would raise IndexError
PROJ_REFERENCE = 0  # mode: map_points_on_image literally, last writer wins (DTFILL_PROJ_*)
PROJ_ZBUFFER = 1  # mode: the nearest return per pixel
PROJ_NO_POINTS = 1  # bit: nothing landed in the frame
PROJ_INDEX_ERROR = 2  # bit (reference mode): the reference's assignment would raise IndexError; the frame is all zeros
PROJ_BAD_COUNT = 4  # bit: counts[b] outside [0, N]; the frame is all zeros
PROJ_COLUMNS = ("pixels", "inside", "behind", "outside")  # frame_counts' columns, DTFILL_PROJ_N of them
UNPROJ_NO_POINTS = 1  # bit: no valid pixel in the frame (DTFILL_UNPROJ_*)
UNPROJ_BAD_INTERVAL = 2  # bit (keep mode): the pitch interval is 0 or not finite; nothing is written
UNPROJ_SINGULAR = 4  # bit: K or E is singular; nothing is written
UNPROJ_OVERFLOW = 8  # bit: more points than capacity; the first N in raster order are written
UNPROJ_BAD_PIXEL = 16  # bit (backward): the pixel list is not strictly increasing inside the frame; zero gradients
UNPROJ_BAD_COUNT = 32  # bit (backward): counts[b, written] outside [0, N]; zero gradients
UNPROJ_WRITTEN = 0  # counts' columns
UNPROJ_TOTAL = 1
CONV_LINEAR = 0  # act of dtfill_conv2d (DTFILL_CONV_*)
CONV_LEAKY = 1  # y > 0 ? y : y * alpha
CONV_ACTS = {"linear": CONV_LINEAR, "leaky": CONV_LEAKY}
CONV_BW_ROWS, CONV_BW_COLS = 32, 64  # DTFILL_CONV_BW_ROWS, _COLS: a segment of dtfill_conv2d_backward_weights' sum
PATHS = {"auto": 0, "general": FLAG_GENERAL_ONLY, "fused": FLAG_FUSED_ONLY}

# the C ABI of include/dtfill.h: symbol -> (restype, argtypes), in the header's order.  tests/test_binding.py holds every entry to
# the header's prototype; tests/test_abi.py checks the .so exports exactly these
vp, ci, cf, sz, cu, ll, cs = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint, ctypes.c_longlong,
                              ctypes.c_char_p)
_ABI = {
    "dtfill_abi_version": (ci, []),
    "dtfill_strerror": (cs, [ci]),
    "dtfill_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "dtfill_batch": (ci, [vp, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_batch_flags": (ci, [vp, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp, sz, vp, cu]),
    "dtfill_batch_epilogue": (ci, [vp, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp, sz, vp, cu, ci, ci, cf]),
    "dtfill_num_kernels": (ci, [ci]),
    "dtfill_kernel_name": (cs, [ci, ci]),
    "dtfill_batch_timed": (ci, [vp, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp, sz, vp, cu, vp]),
    "dtfill_pass_stats": (ci, [vp, sz, ci, ci, ci, ci, vp, vp]),
    "dtfill_outlier_removal": (ci, [vp, ci, ci, ci, vp, vp]),
    "dtfill_generate_multi_channel": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "dtfill_generate_multi_channel_backward_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "dtfill_generate_multi_channel_backward": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_demo_multi_channel_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "dtfill_demo_multi_channel": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_crop_floor": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp]),
    "dtfill_png16": (ci, [vp, ci, ci, ci, ci, ci, cf, cf, cf, cf, vp, vp]),
    "dtfill_line_subsample_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_line_subsample": (ci, [vp, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, sz, vp]),
    "dtfill_depth_read_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_depth_read": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]),
    "dtfill_rgb_read_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_rgb_read": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
    "dtfill_nyu_read_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_nyu_read": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_project_points_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "dtfill_project_points": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, cf, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_unproject_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_unproject": (ci, [vp, vp, ci, ci, ci, cf, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_unproject_backward_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_unproject_backward": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "dtfill_metrics_workspace_bytes": (sz, [ci]),
    "dtfill_metrics": (ci, [vp, vp, ci, ll, ci, vp, vp, sz, vp]),
    "dtfill_train_loss_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_train_loss": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, cf, ci, ci, ci, ci, vp, vp, sz, vp]),
    "dtfill_train_loss_backward": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, cf, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "dtfill_fill_backward_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_fill_backward": (ci, [vp, vp, vp, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_nearest_gather_workspace_bytes": (sz, [ci, ci, ci]),
    "dtfill_nearest_gather": (ci, [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, sz, vp]),
    "dtfill_nearest_gather_backward_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "dtfill_nearest_gather_backward": (ci, [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_backward_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
    "dtfill_conv2d_backward_data": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, sz, vp]),
    "dtfill_conv2d_backward_weights": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_wide_backward_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci, ci, ci]),
    "dtfill_conv2d_strided_backward_data": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, vp, sz, vp]),
    "dtfill_conv2d_strided_backward_weights": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_transpose_backward_data": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, sz, vp]),
    "dtfill_conv2d_transpose_backward_weights": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_image_backward_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
    "dtfill_conv2d_image_backward_weights": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_image": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, cf, vp, ci, ci, vp]),
    "dtfill_max_pool_pyramid": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, ci, ci, vp, ci, ci, vp]),
    "dtfill_max_pool_pyramid_backward": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, ci, ci, vp, ci, ci, vp, vp]),
    "dtfill_adam_state_floats": (sz, [vp, ci]),
    "dtfill_adam_record_bytes": (sz, []),
    "dtfill_adam_init": (ci, [vp, vp]),
    "dtfill_adam_step": (ci, [vp, vp, vp, ci, vp, vp, vp, cf, cf, cf, cf, vp]),
    "dtfill_conv2d_bf16_packed_elems": (sz, [ci, ci, ci]),
    "dtfill_conv2d_pack_bf16": (ci, [vp, ci, ci, ci, vp, vp]),
    "dtfill_conv2d_strided_bf16": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp, ci, cf, vp, ci, ci, vp]),
    "dtfill_conv2d_transpose_bf16": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, cf, vp, ci, ci, vp]),
    "dtfill_conv2d_wide_backward_bf16_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci, ci, ci]),
    "dtfill_conv2d_strided_backward_data_bf16": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, vp, sz, vp]),
    "dtfill_conv2d_strided_backward_weights_bf16": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_transpose_backward_data_bf16": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, sz, vp]),
    "dtfill_conv2d_transpose_backward_weights_bf16": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, sz, vp]),
    "dtfill_conv2d_strided": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp, ci, cf, vp, ci, ci, vp]),
    "dtfill_conv2d_transpose": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, cf, vp, ci, ci, vp]),
    "dtfill_conv2d": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, cf, vp, ci, ci, vp]),
}
POOL_LEVELS = (2, 4, 8)  # the window sizes of dtfill_max_pool_pyramid, in the order of its out and dy arguments
ADAM_GROUP = 128  # DTFILL_ADAM_GROUP: the variables one launch of dtfill_adam_step takes
ADAM_CHUNK = 4096  # DTFILL_ADAM_CHUNK: the elements a block of it owns
SYMBOLS = tuple(_ABI)
del vp, ci, cf, sz, cu, ll, cs  # (the table's shorthands, not names of this module)
STATS = ("all", "window", "anydist", "sky", "points", "colt")  # DTFILL_STATS_*
METRICS_KITTI = 0
METRICS_NYU = 1
METRICS_COLUMNS = ("mse", "rmse", "mae", "irmse", "imae", "delta1", "delta2", "delta3", "count")
LOSS_KITTI = 0
LOSS_NYU = 1
LOSS_COLUMNS = ("main", "aux", "n_gt", "n_in", "S_main", "S_aux")

_lib = None


class DtfillError(RuntimeError):
    """A negative DTFILL_ERR_* return code from the C ABI."""

    def __init__(self, code, msg):
        super().__init__("dtfill error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile csrc/dtfill.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))]
    srcs.append(os.path.join(_HERE, "..", "include", "dtfill.h"))
    stale = force or not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < max(os.path.getmtime(f) for f in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-C", CSRC, "libdtfill.so"])
    return SO_PATH


def load():
    """Load libdtfill.so; raises ImportError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "libdtfill.so is missing at %s -- build it with __graft_entry__.build() or "
            "`make -C %s`; this package has no CPU fallback" % (SO_PATH, CSRC)
        )
    L = ctypes.CDLL(SO_PATH)
    for name, (restype, argtypes) in _ABI.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def check(code):
    if code != 0:
        raise DtfillError(code, load().dtfill_strerror(code).decode())

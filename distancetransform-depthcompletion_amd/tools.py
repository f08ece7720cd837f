"""Drop-in mirror of the reference operator interface (numpy in, numpy out).

Same names, argument meaning and error behaviour as
  solution_DeepNet/tools.py:7-35      nearest_point, DT_complete_batch
  solution_DeepNet/eval_NYU.py:114-133 nearest_point (threshold 0.001), Distance_Transform
  data_read.py:81-99                   depth_read (and depth_read_batch for Data_load.read_batch's stack of them)
  data_read.py:66-73                   rgb_read (and rgb_read_batch for read_batch's img_batch and the drivers' / 255.0)
  subsample_Lidar_train.py:180-193     map_points_on_image (and project_points for a batch of ragged clouds, z-buffered)
  subsample_Lidar_train.py:125-153     get_all_points (and unproject_frames for a batch, a payload, the pitches, keep_ratio)
but the work is done by libdtfill.so on the current HIP device.  Differences from the reference,
all widening: DT_complete_batch accepts any HxW (the reference hard-codes 352x1216 in its
reshapes, tools.py:25,27), and the thresholds the reference writes as literals are keyword
arguments whose defaults are those literals.
"""
import os

import numpy as np
import torch

from . import _lib
from . import device as _device


def _as_f32_frames(a):
    """Input checking shared by the three functions: the kernels compute the predicates in
    float32, which is what numpy does for the float32 arrays the reference's loaders produce
    (data_read.py:81-99).  float64 input is accepted when it is exactly float32-representable."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a
    if a.dtype.kind not in "fiub":
        raise TypeError("expected a real-valued array, got dtype %s" % a.dtype)
    a32 = a.astype(np.float32)
    if a.dtype.kind == "f" and not np.array_equal(a32.astype(a.dtype), a, equal_nan=True):
        raise TypeError(
            "float64 input that is not exactly representable in float32 is not supported: "
            "the source/value predicates (tools.py:8,22) are evaluated in float32 on the device"
        )
    return a32


def _upload(a, device):
    """A host array -> a contiguous tensor of its dtype and shape on `device`."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def nearest_point(refined_lidar, src_thr=0.1):
    """tools.py:7-10.  Returns (dt float32 [H,W], lbl int32 [H,W]) exactly as
    cv2.distanceTransformWithLabels(uint8((1.0-x) > src_thr), DIST_L1, 5, DIST_LABEL_PIXEL)."""
    x = np.squeeze(_as_f32_frames(refined_lidar))
    if x.ndim != 2:
        raise ValueError("nearest_point expects an array squeezable to [H,W], got shape %s" % (np.shape(refined_lidar),))
    out = _device.default_op().run_numpy(x[None], src_thr=src_thr, val_thr=0.1, want=("dt", "index"))
    return out["dt"][0], out["index"][0]


def DT_complete_batch(lidar_batch, src_thr=0.1, val_thr=0.1, first_row=0, floor=None, if_removal=False):
    """tools.py:13-35.  lidar_batch [B,H,W,C>=1] (channel 0 is used, tools.py:18) ->
    float32 [B,H,W,1].  Raises IndexError like tools.py:26 when a frame's value list is too short.
    first_row / floor fold the caller's next lines into the same pass: demo.py:292-293
    (lidar_batch[:, 96:, :, :] -> first_row=96, result [B,H-96,W,1]) and the depth floor relu(d - 0.9) + 0.9.
    if_removal folds the loader's outlier_removal() (data_read.py:103-128, the flag of data_read.py:168) into the same pass:
    DT_complete_batch(x, if_removal=True) == DT_complete_batch(outlier_removal(x_i) for every frame)."""
    lb = _as_f32_frames(lidar_batch)
    if lb.ndim != 4:
        raise IndexError("too many indices for array: DT_complete_batch indexes lidar_batch[i,:,:,0]")
    x = lb[:, :, :, 0]
    out = _device.default_op().run_numpy(x, src_thr=src_thr, val_thr=val_thr, want=("depth",), depth_rows_from=first_row,
                                         depth_floor=floor, outlier_removal=if_removal)
    return np.expand_dims(out["depth"], axis=-1)  # already a fresh float32 array


def nearest_source(x, values=None, src_thr=0.1, metric="l1_cv"):
    """The nearest-source pixel map, and any channels filled from it (include/dtfill.h, dtfill_nearest_gather).  x: squeezed
    like nearest_point's argument, to one frame [H,W] or to a batch [B,H,W]; a pixel is a source iff NOT((1 - x) > src_thr) in
    float32.  Returns (dt, pixel): the distance map and, int32, the flat pixel row*W + col of every pixel's nearest source (-1
    in a frame without one) -- with metric="l2" the raveled scipy.ndimage.distance_transform_edt(return_indices=True), ties to
    the smallest raster index.  values: float32, [H,W] or [C,H,W] for a frame, [B,H,W] or [B,C,H,W] for a batch; then
    (dt, pixel, filled), filled of values' shape with values' bits at the nearest source and +0.0 where there is none."""
    a = np.squeeze(_as_f32_frames(x))
    if a.ndim not in (2, 3):
        raise ValueError("nearest_source expects an array squeezable to [H,W] or [B,H,W], got shape %s" % (np.shape(x),))
    batch = a.ndim == 3
    a = a if batch else a[None]
    B, H, W = a.shape
    v = None
    if values is not None:
        v = np.asarray(values)
        if v.dtype != np.float32:
            raise TypeError("values must be float32 (they are copied as bits), got dtype %s" % v.dtype)
        lead = v.shape[:-2]
        if v.shape[-2:] != (H, W) or (lead not in ((B,), ) and not (len(lead) == 2 and lead[0] == B) if batch else len(lead) > 1):
            raise ValueError("values of shape %s do not go with frames of shape %s" % (v.shape, np.shape(x)))
        v = v.reshape(B, -1, H, W)
    op = _device.default_op(metric)
    xd = _upload(a, op.device)
    vd = None if v is None else _upload(v, op.device)
    # dt and index in tensors of this call's own (the operator's buffers are the next caller's, on any thread), and the
    # operator's lock over both launches
    res = dict(dt=torch.empty_like(xd), index=torch.empty_like(xd, dtype=torch.int32))
    with op._lock:
        op.run(xd, src_thr=src_thr, val_thr=0.1, want=("dt", "index"), out=res)
        filled, pixel, _ = _device.nearest_gather_device(xd, res["index"], vd, src_thr)
    dt, pixel = res["dt"].cpu().numpy(), pixel.cpu().numpy()
    if not batch:
        dt, pixel = dt[0], pixel[0]
    if v is None:
        return dt, pixel
    return dt, pixel, filled.cpu().numpy().reshape(np.shape(values))


def Distance_Transform(lidar, src_thr=0.001, val_thr=0.1, floor=None):
    """eval_NYU.py:120-133 (src_thr=0.001 as eval_NYU.py:115; the notebooks use 0.1).
    One frame squeezable to [H,W]; the result keeps the input's dtype like the reference.
    floor=0.9 folds eval_NYU.py:205 (relu(depth - 0.9) + 0.9, float32) into the same pass."""
    src = np.asarray(lidar)
    x = np.squeeze(_as_f32_frames(src))
    if x.ndim != 2:
        raise ValueError("not enough values to unpack: Distance_Transform expects a frame squeezable to [H,W]")
    if np.count_nonzero(x > np.float32(val_thr)) == 1:
        # eval_NYU.py:125 squeezes the value list; with exactly one valid pixel it becomes 0-d and
        # the gather on the next line raises -- kept, so callers see the reference's behaviour
        raise IndexError("too many indices for array: array is 0-dimensional, but 1 were indexed")
    out = _device.default_op().run_numpy(x[None], src_thr=src_thr, val_thr=val_thr, want=("depth",), depth_floor=floor)
    depth = out["depth"][0]
    return depth.astype(src.dtype) if src.dtype.kind == "f" else depth


def outlier_removal(lidar):
    """data_read.py:103-128 (the loader's optional filter in front of the fill, data_read.py:168-169):
    zero every pixel that exceeds the mean of the valid pixels in its 7x7 diamond by more than 1.0.
    Input squeezable to [H,W]; float32 [H,W] back, like the reference."""
    x = np.squeeze(_as_f32_frames(lidar))
    if x.ndim != 2:
        raise ValueError("outlier_removal expects an array squeezable to [H,W], got shape %s" % (np.shape(lidar),))
    xd = _upload(x[None], _device.default_op().device)
    return _device.outlier_removal_device(xd)[0].cpu().numpy()


def generate_multi_channel(lidar_data, lidar_mask, table_size=7, scale_num=4):
    """net.py:83-122 as a numpy function: lidar_data, lidar_mask [B,H,W,1] -> (lidar_1, .., lidar_4), each
    [B,H,W,1] float32, None beyond scale_num (the reference returns TF tensors of the same shapes)."""
    d = _as_f32_frames(lidar_data)
    m = _as_f32_frames(lidar_mask)
    if d.ndim != 4 or d.shape[-1] != 1 or m.shape != d.shape:
        raise ValueError("generate_multi_channel expects lidar_data and lidar_mask of shape [B,H,W,1]")
    dev = _device.default_op().device
    dd = _upload(d[..., 0], dev)
    mm = _upload(m[..., 0], dev)
    outs = _device.generate_multi_channel_device(dd, mm, table_size, scale_num)
    return tuple(None if o is None else o.cpu().numpy()[..., None] for o in outs)


def conv2d(x, kernel, bias=None, act="linear", alpha=0.2):
    """A stride-1 'same' float32 convolution as a numpy function, in the fixed summation order of include/dtfill.h
    (dtfill_conv2d): what a tf.keras.layers.Conv2D(Cout, ksize, padding="same") of net.py's SparsityCNN computes, followed by
    tf.nn.leaky_relu for act="leaky".  x [B,H,W,Cin]; kernel [ksize,ksize,Cin,Cout] and bias [Cout] as Keras stores them.
    Returns float32 [B,H,W,Cout]."""
    a = _as_f32_frames(x)
    k = _as_f32_frames(kernel)
    if a.ndim != 4 or k.ndim != 4:
        raise ValueError("conv2d expects x [B,H,W,Cin] and kernel [ksize,ksize,Cin,Cout]")
    dev = _device.default_op().device
    b = None if bias is None else _upload(_as_f32_frames(bias), dev)
    return _device.conv2d_device(_upload(a, dev), _upload(k, dev), b, act, alpha).cpu().numpy()


def max_pool(x, ksize):
    """tf.nn.max_pool(x, ksize, ksize, 'SAME') as a numpy function (include/dtfill.h, dtfill_max_pool_pyramid with one level):
    x [B,H,W,C] with C a multiple of 4, ksize 2, 4 or 8, H and W multiples of it.  The winner of a window is its first NaN if
    it holds one, else its raster-first maximum.  Returns float32 [B,H/ksize,W/ksize,C]."""
    a = _as_f32_frames(x)
    if a.ndim != 4:
        raise ValueError("max_pool expects x [B,H,W,C]")
    dev = _device.default_op().device
    return _device.max_pool_pyramid_device(_upload(a, dev), (int(ksize),))[0].cpu().numpy()


def subsample_lidar(sparse_depth, intrinsic, extrinsic, keep_ratio=0.25, n_bins=64):
    """subsample_Lidar_train.py / subsample_Lidar_val.py: get_all_points -> calculate_angle -> sample(keep_ratio) ->
    map_points_on_image, in one call (the caller's `* 256 -> uint16` PNG write stays as it is).  sparse_depth [H,W],
    [H,W,1], [B,H,W] or [B,H,W,1]; intrinsic [3,3] or [B,3,3]; extrinsic (velo->cam) [4,4] or [B,4,4].  Returns float32
    of the input's shape: the kept pixels hold their input value, the others 0.  Raises np.linalg.LinAlgError for a
    singular intrinsic / extrinsic and ValueError for a frame without a valid pixel (> 0.1), as the reference does; a
    frame whose pitch interval is 0 or not finite comes back all zeros, as the reference's NaN labels keep nothing."""
    _device.keep_every_of(keep_ratio)  # ValueError before any device work
    a = _as_f32_frames(sparse_depth)
    shape = a.shape
    if a.ndim in (3, 4) and a.shape[-1] == 1:
        a = a[..., 0]  # [H,W,1] / [B,H,W,1] (a [B,H,W] batch of one-column frames reads as [H,W,1])
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("subsample_lidar expects [H,W], [H,W,1], [B,H,W] or [B,H,W,1], got shape %s" % (shape,))
    x = _upload(a, _device.default_op().device)
    out, status = _device.line_subsample_device(x, intrinsic, extrinsic, keep_ratio=keep_ratio, n_bins=n_bins)
    st = status.cpu().numpy()
    bad = np.flatnonzero(st & _lib.LINES_SINGULAR)
    if bad.size:
        raise np.linalg.LinAlgError("Singular matrix (intrinsic or extrinsic of frame %d)" % bad[0])
    bad = np.flatnonzero(st & _lib.LINES_NO_POINTS)
    if bad.size:
        raise ValueError("zero-size array to reduction operation maximum which has no identity (frame %d has no point "
                         "with depth > 0.1)" % bad[0])
    return out.cpu().numpy().reshape(shape)


def _cloud(a, what):
    """A point cloud as the kernel reads it: float32 [n, 3 or 4] (n may be 0), under _as_f32_frames' rule for other dtypes."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError("%s: expected points [n, 3] or [n, 4], got shape %s" % (what, a.shape))
    return _as_f32_frames(a)


def _stage_clouds(clouds, device):
    """A ragged batch of clouds on the device: (points float32 [B, N, stride], counts int32 [B], stage): views of one device
    tensor filled by one H2D copy from `stage`, a page-locked buffer that carries the counts (as bits) behind the records; the
    padding records are never read and are left as they are.  The caller keeps `stage` until it has synchronised."""
    B = len(clouds)
    N = max(1, max(c.shape[0] for c in clouds))
    stride = max(c.shape[1] for c in clouds)
    n = B * N * stride
    stage = _device._host_pool.take((n + B,), np.float32)
    raw = stage.array[:n].reshape(B, N, stride)
    for b, c in enumerate(clouds):
        raw[b, :c.shape[0], :c.shape[1]] = c
    stage.array[n:].view(np.int32)[:] = [c.shape[0] for c in clouds]
    d = torch.empty((n + B,), dtype=torch.float32, device=device)
    d.copy_(stage.tensor, non_blocking=True)
    return d[:n].view(B, N, stride), d[n:].view(torch.int32), stage


def _raise_index_error(status):
    bad = np.flatnonzero(status & _lib.PROJ_INDEX_ERROR)
    if bad.size:
        raise IndexError("frame %d: a point's pixel index is out of bounds for the depth map (depth_map[v,u]=z)" % bad[0])


def map_points_on_image(left_points, intrinsic, extrinsic, hw=(352, 1216)):
    """subsample_Lidar_train.py:180-193 / subsample_Lidar_val.py:167-180: left_points [n, 3] in the Velodyne frame through
    extrinsic [4,4] (velo->cam) and intrinsic [3,3], rounded to a pixel, depth_map[v, u] = z in point order (the last writer of
    a pixel wins, negative indices wrap).  Returns the float64 [H, W] depth map, hw = (352, 1216) as the reference hard-codes
    it.  Raises IndexError where the reference's assignment would (an index outside the wrap range, or not finite), and
    ValueError for points that are not [n, 3].  The points are read as float32: float64 input must be exactly
    float32-representable (TypeError otherwise), which holds for what get_all_points returns from float32 calibration."""
    p = np.asarray(left_points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("map_points_on_image expects left_points of shape [n, 3], got shape %s" % (p.shape,))
    cloud = _cloud(p, "left_points")  # (the argument errors come before any device work)
    pts, counts, stage = _stage_clouds([cloud], _device.default_op().device)
    _, status, _, f64 = _device.project_points_device(pts, counts, intrinsic, extrinsic, hw, mode="reference", want="float64")
    out, st = _read_back(f64[0], status, np.float64)
    _raise_index_error(st)
    return out


def project_points(clouds, K, E, hw=(352, 1216), mode="zbuffer", min_z=0.0):
    """A batch of point clouds -> sparse depth frames (include/dtfill.h, dtfill_project_points).  clouds: a list of ragged
    [n_i, 3 or 4] arrays in the Velodyne frame (a KITTI .bin read as float32 and reshaped to [-1, 4] goes in as it is; n_i may
    be 0); K: intrinsics [3,3] or [B,3,3]; E: velo->cam extrinsics [4,4] or [B,4,4]; hw = (H, W).  mode "zbuffer" keeps the
    nearest return per pixel and drops points with z <= min_z or outside the frame; "reference" is map_points_on_image's
    assignment (IndexError where it would raise).  One page-locked staging buffer, one copy each way.  Returns (float32
    [B, H, W] in an array of its own, counts int32 [B, 4]: pixels written, points inside, behind, outside)."""
    clouds = [_cloud(c, "cloud %d" % b) for b, c in enumerate(clouds)]
    if not clouds:
        raise ValueError("project_points needs at least one cloud")
    pts, counts, stage = _stage_clouds(clouds, _device.default_op().device)
    frame, status, counts4 = _device.project_points_device(pts, counts, K, E, hw, mode=mode, min_z=min_z)
    out, tail = _read_back(frame, torch.cat([status[:, None], counts4], 1), np.float32)
    _raise_index_error(tail[:, 0])
    return out, tail[:, 1:].copy()


def unproject_frames(x, K, E, val_thr=0.1, payload=None, keep_ratio=None, n_bins=64, with_pitch=False):
    """Depth frames -> their point clouds in the Velodyne frame (include/dtfill.h, dtfill_unproject).  x: [H,W] or [B,H,W];
    a pixel is a point iff x > val_thr in float32; K: intrinsics [3,3] or [B,3,3]; E: velo->cam extrinsics [4,4] or [B,4,4];
    payload: float32 of x's shape, carried as each point's fourth float.  keep_ratio = None gives every valid pixel
    (get_all_points), keep_ratio = 1/k the reference's left_points, sample(calculate_angle(get_all_points(...))), with
    subsample_lidar's errors: np.linalg.LinAlgError for a singular calibration, ValueError for a frame without a valid pixel
    (only with keep_ratio: get_all_points of an empty frame is an empty cloud); a frame whose pitch interval is 0 or not finite
    keeps nothing.  Returns a list of B ragged float32 arrays [n_b, 3 or 4] in raster order, and with with_pitch a second
    list of float64 [n_b] pitches.  One page-locked staging buffer, one copy each way."""
    if keep_ratio is not None:
        _device.keep_every_of(keep_ratio)  # ValueError before any device work
    a = _as_f32_frames(x)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or 0 in a.shape:
        raise ValueError("unproject_frames expects [H,W] or [B,H,W], got shape %s" % (np.shape(x),))
    B, H, W = a.shape
    p = None
    if payload is not None:
        p = np.asarray(payload)
        if p.dtype != np.float32:
            raise TypeError("payload must be float32 (it is copied as bits), got dtype %s" % p.dtype)
        if p.size != a.size or p.shape[-2:] != (H, W):
            raise ValueError("payload of shape %s does not go with frames of shape %s" % (p.shape, np.shape(x)))
        p = p.reshape(a.shape)
    n = a.size
    stage = _device._host_pool.take((n * (1 if p is None else 2),), np.float32)
    stage.array[:n] = a.reshape(-1)
    if p is not None:
        stage.array[n:] = p.reshape(-1)
    dev = _device.default_op().device
    d = torch.empty(stage.array.shape, dtype=torch.float32, device=dev)
    d.copy_(stage.tensor, non_blocking=True)
    want = ("pitch",) if with_pitch else ()
    points, counts, status, pitch, _ = _device.unproject_device(
        d[:n].view(B, H, W), K, E, val_thr, None if p is None else d[n:].view(B, H, W), keep_ratio=keep_ratio, n_bins=n_bins,
        want=want)
    # the clouds' capacity is H*W a frame: copy back what the counts say is in use, packed on the device first
    cnt = torch.cat([counts[:, 0], status]).cpu().numpy()  # synchronises: the staging buffer is done with
    nb, st = cnt[:B], cnt[B:]
    bad = np.flatnonzero(st & _lib.UNPROJ_SINGULAR)
    if bad.size:
        raise np.linalg.LinAlgError("Singular matrix (intrinsic or extrinsic of frame %d)" % bad[0])
    bad = np.flatnonzero(st & _lib.UNPROJ_NO_POINTS)
    if bad.size and keep_ratio is not None:
        raise ValueError("zero-size array to reduction operation maximum which has no identity (frame %d has no point "
                         "with depth > %r)" % (bad[0], val_thr))
    total = int(nb.sum())
    stride = points.shape[2]
    if total:
        out, _ = _read_back(torch.cat([points[b, :nb[b]] for b in range(B)]), status[:0], np.float32)
    else:
        out = np.zeros((0, stride), np.float32)
    ends = np.cumsum(nb)
    clouds = [out[e - k:e] for e, k in zip(ends, nb)]
    if not with_pitch:
        return clouds
    if total:
        ph, _ = _read_back(torch.cat([pitch[b, :nb[b]] for b in range(B)]), status[:0], np.float64)
    else:
        ph = np.zeros((0,), np.float64)
    return clouds, [ph[e - k:e] for e, k in zip(ends, nb)]


def get_all_points(lidar, intrinsic, extrinsic, image_coor_tensor=None):
    """subsample_Lidar_train.py:125-153 / subsample_Lidar_val.py:112-140: the points of every pixel of `lidar` (squeezable to
    [H,W]; any size, where the reference hard-codes 352 x 1216) with depth > 0.1, back-projected through the inverses of
    intrinsic [3,3] and extrinsic [4,4] (velo->cam), as float32 [n, 3] in raster order.  image_coor_tensor, the reference's
    precomputed pixel grid, is accepted and ignored.  Raises np.linalg.LinAlgError for a singular calibration, as the
    reference's np.linalg.inv does.  The arithmetic is the contract's float64 with one rounding to float32 at the end
    (include/dtfill.h, dtfill_unproject), where the reference computes in float32 throughout."""
    x = np.squeeze(_as_f32_frames(lidar))
    if x.ndim != 2:
        raise ValueError("get_all_points expects an array squeezable to [H,W], got shape %s" % (np.shape(lidar),))
    return unproject_frames(x, np.reshape(intrinsic, [3, 3]), np.reshape(extrinsic, [4, 4]))[0]


KITTI_SIZE = (1216, 352)  # data_read.py:96: PIL's (width, height)


def _png_values(a, what):
    """A decoded PNG frame as the kernel reads it: 2-D, integer values that fit uint16 (TypeError otherwise: the kernel takes
    16-bit values, where the reference would go on with any int)."""
    a = np.asarray(a)
    if a.ndim != 2 or 0 in a.shape:
        raise ValueError("%s: expected a non-empty 2-D array of decoded PNG values, got shape %s" % (what, a.shape))
    if a.dtype == np.uint16 or a.dtype == np.uint8:
        return a
    if a.dtype.kind not in "iu":
        raise TypeError("%s: expected integer PNG values, got dtype %s" % (what, a.dtype))
    if a.min() < 0 or a.max() > 65535:
        raise TypeError("%s: values in [%d, %d] do not fit uint16" % (what, a.min(), a.max()))
    return a


def _frame_size(frames, size):
    """(H, W) of a batch read's output: size = (width, height) as PIL writes it, or, with size=None, the frames' own size."""
    if size is not None:
        return _device._read_size(size)
    if any(f.shape != frames[0].shape for f in frames):
        raise ValueError("size=None keeps the source size, so every frame must have the same shape; got %s"
                         % sorted({f.shape for f in frames}))
    return frames[0].shape[:2]


def _stage_frames(frames, C, dtype):
    """A ragged batch on the device.  frames: checked arrays [h, w] or [h, w, C] of any mixed sizes -> (raw [B, hmax, wmax, C]
    of `dtype` (uint16 or uint8), dims int32 [B, 2], stage): the first two are views of one device tensor, filled by one H2D
    copy from `stage`, a padded page-locked buffer that carries the dims behind the values.  The copy is asynchronous: the
    caller keeps `stage` until it has synchronised (_read_back does), only then may the buffer go back to the pool."""
    B = len(frames)
    hmax = max(f.shape[0] for f in frames)
    wmax = max(f.shape[1] for f in frames)
    n = B * hmax * wmax * C
    per = 4 // np.dtype(dtype).itemsize  # values per int32
    n4 = -(-n // per) * per  # the dims start 4-byte aligned
    stage = _device._host_pool.take((n4 + 2 * per * B,), dtype)
    raw = stage.array[:n].reshape(B, hmax, wmax, C)  # the padding is never read: left as it is
    for b, f in enumerate(frames):
        raw[b, :f.shape[0], :f.shape[1]] = f.reshape(f.shape[0], f.shape[1], C)
    stage.array[n4:].view(np.int32).reshape(B, 2)[:] = [f.shape[:2] for f in frames]
    d = torch.empty((n4 + 2 * per * B,), dtype=stage.tensor.dtype, device=_device.default_op().device)
    d.copy_(stage.tensor, non_blocking=True)
    return d[:n].view(B, hmax, wmax, C), d[n4:].view(torch.int32).view(B, 2), stage


def _read_back(out, status, dtype):
    """(the device tensor `out` in a page-locked array of its own, by one D2H copy; status as numpy)."""
    host = _device._host_pool.take(tuple(out.shape), dtype)
    host.tensor.copy_(out, non_blocking=True)
    return host.array, status.cpu().numpy()  # synchronises: the staging buffer and the result are done with


def _depth_read_frames(frames, size):
    """The frames (checked by _png_values) -> (float32 [B, H, W, 1] in a page-locked array of its own, status int32 [B]):
    one staged H2D copy, one dtfill_depth_read, one D2H copy of the result."""
    if not frames:
        raise ValueError("depth_read_batch needs at least one frame")
    H, W = _frame_size(frames, size)
    raw, dims, stage = _stage_frames(frames, 1, np.uint16)  # (stage: held to the end, past _read_back's synchronisation)
    out, status = _device.depth_read_device(raw.squeeze(3), dims, (W, H))
    return _read_back(out.unsqueeze(3), status, np.float32)


def depth_read(filename):
    """data_read.py:81-99 (KITTI_demo_loader.depth_read, :404-422, is the same): a 16-bit depth PNG -> float32
    [352, 1216, 1], the values / 256 NEAREST-resized as Pillow does.  The PNG is decoded on the host, the rest runs on the
    device.  Raises the reference's AssertionErrors (file missing; every value <= 255) with its messages; values that do
    not fit uint16 raise TypeError."""
    assert os.path.exists(filename), "file not found: {}".format(filename)
    from PIL import Image

    img_file = Image.open(filename)
    depth_png = _png_values(np.array(img_file), filename)
    img_file.close()
    out, st = _depth_read_frames([depth_png], KITTI_SIZE)
    assert not st[0] & _lib.READ_NOT_16BIT, "np.max(depth_png)={}, path={}".format(np.max(depth_png), filename)
    return out[0]


def depth_read_batch(frames, size=KITTI_SIZE, check=True):
    """depth_read for a batch: frames is a list of decoded 2-D integer PNG arrays (np.array(Image.open(path))) of any mixed
    sizes; returns float32 [B, H, W, 1], size = (width, height) as PIL writes it -- np.asarray of the list Data_load.
    read_batch stacks (data_read.py:166, 172).  size=None keeps the source size, the read_one_val / read_one_test path
    (data_read.py:215, 261: / 256 without a resize); every frame must then have the same shape.  With check=True an
    AssertionError names the first frame whose values are all <= 255 (the reference's assert)."""
    frames = [_png_values(f, "frame %d" % b) for b, f in enumerate(frames)]
    out, st = _depth_read_frames(frames, size)
    if check:
        bad = np.flatnonzero(st & _lib.READ_NOT_16BIT)
        if bad.size:
            b = int(bad[0])
            raise AssertionError("np.max(depth_png)={}, frame {}".format(np.max(frames[b]), b))
    return out


def _rgb_values(a, what):
    """A decoded image as the kernel reads it: [h, w] or [h, w, C <= 4] of integer values that fit uint8 (TypeError otherwise:
    the reference's np.array(img, dtype='uint8') would wrap them silently)."""
    a = np.asarray(a)
    if a.ndim not in (2, 3) or 0 in a.shape or (a.ndim == 3 and a.shape[2] > 4):
        raise ValueError("%s: expected a non-empty decoded image [h, w] or [h, w, C <= 4], got shape %s" % (what, a.shape))
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind not in "iub":
        raise TypeError("%s: expected integer pixel values, got dtype %s" % (what, a.dtype))
    if a.min() < 0 or a.max() > 255:
        raise TypeError("%s: values in [%d, %d] do not fit uint8" % (what, a.min(), a.max()))
    return a


def rgb_read_batch(frames, size=KITTI_SIZE, first_row=0, dtype=np.uint8):
    """rgb_read for a batch: frames is a list of decoded images (np.array(Image.open(path))) of any mixed sizes and one channel
    count, [h, w, C] or all [h, w]; size = (width, height) as PIL writes it.  dtype=np.uint8 returns np.asarray of the
    img_batch Data_load.read_batch stacks (data_read.py:163, 175), uint8 [B, H, W, C] ([B, H, W] for 2-D frames);
    dtype=np.float32 the drivers' next two lines, img_batch[:, first_row:] / 255.0 as float32 (train.py:213-214).  first_row
    crops either form.  size=None keeps the source size, the read_one_val path (data_read.py:206-210); every frame must then
    have the same shape.  One staged H2D copy, one dtfill_rgb_read, one D2H copy of the result, which is an array of its own."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise ValueError("dtype must be np.uint8 or np.float32, got %s" % dtype)
    frames = [_rgb_values(f, "frame %d" % b) for b, f in enumerate(frames)]
    if not frames:
        raise ValueError("rgb_read_batch needs at least one frame")
    if any(f.shape[2:] != frames[0].shape[2:] for f in frames):
        raise ValueError("every frame must have the same channel count; got shapes %s" % sorted({f.shape for f in frames}))
    C = frames[0].shape[2] if frames[0].ndim == 3 else 1
    H, W = _frame_size(frames, size)
    first_row = _device._first_row(first_row, H)
    raw, dims, stage = _stage_frames(frames, C, np.uint8)  # (stage: held to the end, past _read_back's synchronisation)
    u8, f32, status = _device.rgb_read_device(raw, dims, (W, H), first_row=first_row, want="uint8" if dtype == np.uint8 else "float")
    out, st = _read_back(u8 if f32 is None else f32, status, dtype)
    assert not st.any(), "dtfill_rgb_read: frame status %s" % st  # the dims are the frames' own
    return out if frames[0].ndim == 3 else out[..., 0]


def rgb_read(filename):
    """data_read.py:66-73 (KITTI_demo_loader.rgb_read, :395-402, is the same): an image file -> uint8 [352, 1216, 3]
    ([352, 1216] for a greyscale one, four channels for RGBA), NEAREST-resized as Pillow does.  The file is decoded on the
    host, the resize runs on the device.  Raises the reference's AssertionError for a missing file; pixel values that do not
    fit uint8 (a 16-bit PNG) raise TypeError where the reference's dtype='uint8' wraps them."""
    assert os.path.exists(filename), "file not found: {}".format(filename)
    from PIL import Image

    img_file = Image.open(filename)
    rgb_png = _rgb_values(np.array(img_file), filename)
    img_file.close()
    return rgb_read_batch([rgb_png], KITTI_SIZE)[0]


def nyu_taps(n_in, n_out):
    """The Gaussian pre-filter of skimage's anti-aliased resize for one axis reduced from n_in to n_out, as
    scipy.ndimage.gaussian_filter builds it: sigma = (f - 1) / 2 at f = n_in / n_out, radius r = int(4 sigma + 0.5),
    w[k] = exp(-0.5 / sigma^2 * k^2) over the sum of all 2r + 1.  Returns (the half kernel w[0..r] as contiguous float64, r),
    or (None, 0) where the axis has no filter pass (r == 0: f < 1.25).  The one statement of the taps: dtfill_nyu_read takes
    them from its caller, so that numpy's exp and sum, not a C library's, decide their bits."""
    n_in, n_out = int(n_in), int(n_out)
    if not 1 <= n_out <= n_in:
        raise ValueError("nyu_taps: need 1 <= n_out <= n_in, got %d -> %d" % (n_in, n_out))
    sigma = (n_in / n_out - 1) / 2
    r = int(4.0 * sigma + 0.5)
    if r == 0:
        return None, 0
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:]), r


def nyu_read_batch(rgb, depth, sample_rate=64, size=(240, 320), rng=None, samples=None):
    """read_one_val_NYU (data_read.py:337-371; Data_load_NYU.read_batch, :295-335, does the same per frame) on arrays, since
    the h5 read stays on the host: rgb uint8 [B, 3, h, w] (or one [3, h, w]) and depth float32 [B, h, w] (or [h, w]) as the
    files store them -> (img float32 [B, H, W, 3] = resize(rgb) * 255, lidar float32 [B, H, W] = gt * Mask, gt float32
    [B, H, W] = resize(depth)), size = (rows, cols) as the reference passes it to skimage.  Per frame sample_rate rows are
    drawn with randint(H - 12) and then sample_rate columns with randint(W - 16), + 6 / + 8, in the reference's order: from
    numpy's legacy global state when rng is None (np.random.seed(s) before the call gives the reference's mask), else from
    rng (a RandomState's randint or a Generator's integers).  samples: int [B, n, 2] of (row, col) to mark instead of any
    draw (nothing is added to them); IndexError, as numpy's Mask[...] = 1 raises it, for one outside the frame.  One staged
    H2D copy, one dtfill_nyu_read, one D2H copy per result."""
    rgb, depth = np.asarray(rgb), np.asarray(depth)
    if rgb.ndim == 3 and depth.ndim == 2:
        rgb, depth = rgb[None], depth[None]
    if rgb.ndim != 4 or depth.ndim != 3 or rgb.shape[0] != depth.shape[0] or rgb.shape[2:] != depth.shape[1:] or 0 in rgb.shape:
        raise ValueError("expected rgb [B, C, h, w] and depth [B, h, w], got shapes %s and %s" % (rgb.shape, depth.shape))
    if rgb.dtype != np.uint8:
        raise TypeError("rgb must be uint8 as the files store it, got dtype %s" % rgb.dtype)
    depth = _as_f32_frames(depth)
    B, C, h, w = rgb.shape
    from . import nyu as _nyu  # (nyu.py imports this module)

    H, W = _nyu._nyu_size(size, h, w)
    if samples is not None:
        samples = np.asarray(samples)
        if samples.ndim != 3 or samples.shape[0] != B or samples.shape[2] != 2 or samples.dtype.kind not in "iu":
            raise ValueError("samples must be integers [B, n, 2] = [%d, n, 2], got %s %s" % (B, samples.dtype, samples.shape))
        if samples.size and (samples.min() < -2 ** 31 or samples.max() >= 2 ** 31):
            raise IndexError("a sample index does not fit int32")
        samples = samples.astype(np.int32)
        n = samples.shape[1]
    else:
        n = int(sample_rate)
        if n != sample_rate or n < 0 or H <= 12 or W <= 16:
            raise ValueError("sample_rate must be an integer >= 0 and size larger than (12, 16), got %r and %r"
                             % (sample_rate, size))
        draw = np.random.randint if rng is None else getattr(rng, "integers", None) or rng.randint
        samples = np.empty((B, n, 2), np.int32)
        for b in range(B):
            samples[b, :, 0] = draw(H - 12, size=n) + 6  # first_index, then second_index: the reference's order
            samples[b, :, 1] = draw(W - 16, size=n) + 8
    nd, ns = depth.size * 4, samples.size * 4
    stage = _device._host_pool.take((nd + ns + rgb.size,), np.uint8)  # depth | samples | rgb, the 4-byte values first
    stage.array[:nd].view(np.float32)[:] = depth.reshape(-1)
    stage.array[nd:nd + ns].view(np.int32)[:] = samples.reshape(-1)
    stage.array[nd + ns:] = rgb.reshape(-1)
    d = torch.empty((nd + ns + rgb.size,), dtype=torch.uint8, device=_device.default_op().device)
    d.copy_(stage.tensor, non_blocking=True)
    img, gt, lidar, status = _nyu.nyu_read_device(
        d[nd + ns:].view(B, C, h, w), d[:nd].view(torch.float32).view(B, h, w),
        d[nd:nd + ns].view(torch.int32).view(B, n, 2) if n else None, (H, W))
    hosts = [_device._host_pool.take(tuple(t.shape), np.float32) for t in (img, lidar, gt)]
    for host, t in zip(hosts, (img, lidar, gt)):
        host.tensor.copy_(t, non_blocking=True)
    st = status.cpu().numpy()  # synchronises: the staging buffer and the results are done with
    bad = np.flatnonzero(st & _lib.NYU_INDEX_ERROR)
    if bad.size:  # (never after the draws: they lie inside the frame)
        raise IndexError("frame %d: a sample index is out of bounds for the %d x %d mask" % (bad[0], H, W))
    return tuple(host.array for host in hosts)

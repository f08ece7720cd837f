"""A literal numpy statement of the demo driver's generate_multi_channel() and generate_multi_channel_with_image()
(solution_DeepNet/demo.py:108-149, :151-198, weights :65-75), for the tests only.

Written from demo.py, not from the kernels (the product does not import this file):
  - the taps are those of tf.image.extract_patches(padding='SAME') over a zero-padded frame, in row-major order
    (sliding_window_view; tap (i, j) of every pixel is one strided view of the padded frames);
  - the weights are create_weight_matrix(), 10 ** (size - |i - middle| - |j - middle|) in float64, rounded to float32;
  - p = data * w in float32; its maximum runs over all ts^2 taps, padding taps included (reduce_max);
  - sel = (p == max); raw = reduce_sum(data * sel) / (0.000001 + count_nonzero(data * sel)), all float32;
  - nothing is masked between the steps: the next step reads raw;
  - every output is divided by scale_range; the image form concatenates [rgb, raw / scale_range] and divides again.
reduce_sum is stated as the contract of include/dtfill.h fixes it: a float32 accumulator that starts at +0 and is advanced
tap by tap in row-major order by np.where(sel, v, 0).  With that order fixed a float32 evaluation has exactly one result, so
the comparisons are bit for bit (+0 and -0 equal).  For finite inputs only: data * sel would turn inf * 0 into NaN, from which
the product deviates on purpose.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ROWS = 64  # rows evaluated per slice: bounds the temporaries on large frames


def create_weight_matrix(size=11):
    """The weights of demo.py:65-75, float32 [size * size] in row-major tap order: the exponent of tap (i, j) is size less its
    L1 distance from the centre tap; ten to that power is a double (exact up to 10^22), rounded to float32 once."""
    assert size % 2 == 1, "an even table has no centre tap"
    off = np.abs(np.arange(size) - size // 2)
    e = size - off[:, None] - off[None, :]
    return np.array([np.float32(10.0 ** int(k)) for k in e.ravel()], np.float32)


def step(data, ts):
    """One step on data float32 [B,H,W].  Returns (raw float32, cnt int64: the non-zero selected taps), each [B,H,W]."""
    data = np.asarray(data, np.float32)
    B, H, W = data.shape
    half = (ts - 1) // 2
    w = create_weight_matrix(ts)
    pd = np.pad(data, ((0, 0), (half, half), (half, half)))
    raw = np.empty((B, H, W), np.float32)
    cnt = np.empty((B, H, W), np.int64)
    zero = np.float32(0)
    for r0 in range(0, H, ROWS):
        r1 = min(H, r0 + ROWS)
        win = sliding_window_view(pd[:, r0 : r1 + 2 * half], (ts, ts), axis=(1, 2))  # [B, rows, W, ts, ts]
        taps = [win[..., t // ts, t % ts] for t in range(ts * ts)]
        mx = np.full((B, r1 - r0, W), -np.inf, np.float32)
        for t, v in enumerate(taps):
            mx = np.maximum(mx, v * w[t])
        acc = np.zeros((B, r1 - r0, W), np.float32)
        c = np.zeros((B, r1 - r0, W), np.int64)
        for t, v in enumerate(taps):
            sel = (v * w[t]) == mx
            acc = acc + np.where(sel, v, zero)
            c += (v * sel.astype(np.float32)) != 0  # count_nonzero(data * sel) over the taps, one tap at a time
        raw[:, r0:r1] = acc / (np.float32(0.000001) + c.astype(np.float32))
        cnt[:, r0:r1] = c
    return raw, cnt


def chain(lidar, ts, scale_num=4):
    """[raw_1, .., raw_scale_num], raw_1 the input itself, each step reading the one before."""
    raws = [np.asarray(lidar, np.float32)]
    for _ in range(scale_num - 1):
        raws.append(step(raws[-1], ts)[0])
    return raws


def outputs(raws, rgb, scale_range):
    """What the functions return for the raw steps: raw / sr ([B,H,W]) without rgb; concat([rgb, raw / sr], 3) / sr
    ([B,H,W,C+1]) with rgb [B,H,W,C]."""
    sr = np.float32(scale_range)
    if rgb is None:
        return [r / sr for r in raws]
    rgb = np.asarray(rgb, np.float32)
    return [np.concatenate([rgb, (r / sr)[..., None]], axis=3) / sr for r in raws]


def generate_multi_channel(lidar_data, table_size, scale_range=90.0, scale_num=4):
    """demo.py:108-149 on lidar_data [B,H,W,1]: four [B,H,W] outputs, None beyond scale_num."""
    outs = outputs(chain(np.asarray(lidar_data, np.float32)[..., 0], table_size, scale_num), None, scale_range)
    return tuple(outs + [None] * (4 - scale_num))


def generate_multi_channel_with_image(rgb_data, lidar_data, table_size, scale_range=90.0, scale_num=4):
    """demo.py:151-198 on rgb_data [B,H,W,C], lidar_data [B,H,W,1]: four [B,H,W,C+1] outputs, None beyond scale_num."""
    outs = outputs(chain(np.asarray(lidar_data, np.float32)[..., 0], table_size, scale_num), rgb_data, scale_range)
    return tuple(outs + [None] * (4 - scale_num))


def assert_same(got, want, what=""):
    """Bit for bit, +0 and -0 equal; no NaN on either side (the inputs are finite)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d value(s) differ, first at %s: got %r, want %r" % (what, bad.sum(), bad.size, k, got[k], want[k]))


# ---- the inputs the tests feed, all finite ----------------------------------------------------------------------------------

DATA_KINDS = ("sparse", "dense", "signed", "planted")


def plant(x, ts=7):
    """The hand cases, written into frame 0 of x [B,H,W] wherever a 2 ts + 3 square of zeros fits (blocks laid out left to
    right, top to bottom; a frame too small for one is returned as it is).  Each block is cleared first and sits far enough
    from the next that its centre window sees nothing else:
      0  80 at L1 distance 2 and 1 at distance 1 of the centre;         1  2.5 at distance 1 and 25.0 at distance 2;
      2  a checkerboard of 4.0;                                          3  nothing (an empty window);
      4  a block of negative values all over;                            5  0.0005 alone (it is below 0.001 and still propagates)."""
    S = 2 * ts + 3
    H, W = x.shape[1:]
    sites = [(r, c) for r in range(0, H - S + 1, S) for c in range(0, W - S + 1, S)]
    for k, (r, c) in enumerate(sites[:6]):
        blk = x[0, r : r + S, c : c + S]
        blk[:] = 0
        m = S // 2
        if k == 0:
            blk[m, m + 1], blk[m + 2, m] = 1.0, 80.0
        elif k == 1:
            blk[m - 1, m], blk[m + 1, m + 1] = 2.5, 25.0
        elif k == 2:
            ii, jj = np.indices(blk.shape)
            blk[(ii + jj) % 2 == 0] = 4.0
        elif k == 4:
            ii, jj = np.indices(blk.shape)
            blk[:] = -1.0 - ((3 * ii + 5 * jj) % 7).astype(np.float32)
        elif k == 5:
            blk[m, m] = 0.0005
    return x


def make_data(kind, rng, shape, ts=7):
    """sparse: 5 % depths on the KITTI k/256 grid in [1, 80); dense: a depth everywhere; signed: signed values, zeros and -0.0;
    planted: sparse with the hand cases of plant() in frame 0."""
    shape = tuple(shape)
    grid = lambda lo, hi: (rng.integers(int(lo * 256), int(hi * 256), shape) / 256.0).astype(np.float32)
    if kind in ("sparse", "planted"):
        x = np.where(rng.random(shape) < 0.05, grid(1, 80), 0).astype(np.float32)
        return plant(x, ts) if kind == "planted" else x
    if kind == "dense":
        return rng.uniform(1, 80, shape).astype(np.float32)
    if kind == "signed":
        v = np.where(rng.random(shape) < 0.3, rng.uniform(-50, 50, shape), 0).astype(np.float32)
        v[rng.random(shape) < 0.1] = np.float32(-0.0)
        return v
    raise ValueError(kind)

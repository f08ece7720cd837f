"""A literal numpy statement of one step of generate_multi_channel() (solution_DeepNet/net.py:83-122), for the tests only.

Written from the reference, not from oracle/oracle.py, so that the two cannot share a misreading:
  - the taps are those of tf.image.extract_patches(padding='SAME') over a zero-padded frame, in row-major order;
  - the weights are create_weight_matrix() (net.py:71-81), ts - |i - middle| - |j - middle|, cast to float32;
  - s = mask * w in float32, and its maximum runs over all ts^2 taps, padding taps included (reduce_max);
  - sel = (s == max); out = reduce_sum(data * sel) / (0.000001 + reduce_sum(sel)).
The sum runs in float64 and is rounded to float32 once, so a pixel with ONE selected tap is bit-exact whatever order a
kernel adds in; the division is float32.  Where more taps are selected, a float32 sum in any order lies within
sum_bound() of this one.  data * sel makes every window that holds a +-inf or NaN input NaN: that is net.py's arithmetic,
from which the product deviates on purpose (include/dtfill.h), so compare it with the product on finite data only.
The product does not import this file.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

CHUNK = 1 << 21  # taps evaluated per slice of rows: ts = 15 on a large frame stays a few tens of MB


def weights(ts):
    """create_weight_matrix(), net.py:71-81: float32 [ts * ts] in row-major tap order."""
    assert (ts + 1) % 2 == 0
    middle = (ts - 1) / 2
    w = np.zeros((ts, ts))
    for i in range(ts):
        for j in range(ts):
            w[i, j] = ts - abs(i - middle) - abs(j - middle)
    return w.reshape(ts * ts).astype(np.float32)


def gmc_step(data, mask, ts):
    """One step on data, mask float32 [B,H,W].  Returns (out float32, count int64: the selected taps, abs_sum float64: the
    sum of |data| over the selected taps), each [B,H,W]."""
    data = np.asarray(data, np.float32)
    mask = np.asarray(mask, np.float32)
    B, H, W = data.shape
    half = (ts - 1) // 2
    w = weights(ts)
    pd = np.pad(data, ((0, 0), (half, half), (half, half)))
    pm = np.pad(mask, ((0, 0), (half, half), (half, half)))
    out = np.empty((B, H, W), np.float32)
    cnt = np.empty((B, H, W), np.int64)
    abs_sum = np.empty((B, H, W), np.float64)
    rows = max(1, CHUNK // (B * W * ts * ts))
    for r0 in range(0, H, rows):
        r1 = min(H, r0 + rows)
        taps = lambda a: sliding_window_view(a[:, r0 : r1 + 2 * half], (ts, ts), axis=(1, 2)).reshape(B, r1 - r0, W, ts * ts)
        v, m = taps(pd), taps(pm)
        s = m * w
        sel = (s == s.max(axis=-1, keepdims=True)).astype(np.float32)
        c = sel.sum(axis=-1, dtype=np.float64)
        total = (v * sel).sum(axis=-1, dtype=np.float64).astype(np.float32)
        out[:, r0:r1] = total / (np.float32(0.000001) + c.astype(np.float32))
        cnt[:, r0:r1] = c.astype(np.int64)
        abs_sum[:, r0:r1] = (np.abs(v) * sel).sum(axis=-1, dtype=np.float64)
    return out, cnt, abs_sum


def next_mask(out):
    """The next step's mask, net.py:95-96: tf.cast(out > 0.001, tf.float32)."""
    return (np.asarray(out, np.float32) > np.float32(0.001)).astype(np.float32)


def sum_bound(cnt, abs_sum):
    """How far a float32 evaluation of a step may lie from gmc_step's: its cnt - 1 float32 additions, the rounding of the float64
    sum to float32 and the two divisions each err by at most 2^-24 of sum |v|, over the divisor 1e-6 + cnt.  Zero where cnt = 1."""
    return np.where(cnt > 1, (cnt + 2) * 2.0 ** -24 * abs_sum / (1e-6 + cnt), 0.0)


def assert_step_matches(got, out, cnt, abs_sum, what=""):
    """got: a float32 evaluation of the step; (out, cnt, abs_sum): gmc_step's.  Bit-exact where one tap is selected (+0 and
    -0 compare equal), within sum_bound() elsewhere."""
    got = np.asarray(got, np.float32)
    assert got.shape == out.shape, (what, got.shape, out.shape)
    err = np.abs(got.astype(np.float64) - out.astype(np.float64))
    bad = ~(err <= sum_bound(cnt, abs_sum))  # a NaN on either side is bad
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d pixel(s) off, first at %s: got %r, want %r (count %d, sum |v| %r)"
                             % (what, bad.sum(), k, got[k], out[k], cnt[k], abs_sum[k]))


# ---- the inputs the tests feed: data kinds x mask kinds, all finite --------------------------------------------------------

DATA_KINDS = ("sparse", "dense", "straddle", "mixed")
MASK_KINDS = ("gt01", "binary", "fraction", "negative", "neg_band", "neg_tap", "neg_zero", "zero")


def make_data(kind, rng, shape):
    """sparse: 5 % depths in [1, 80); dense: a depth everywhere (every pixel passes the next step's mask); straddle: values at
    and around 0.001 (0.001f and its neighbours included); mixed: signed values, some of them -0.0."""
    shape = tuple(shape)
    if kind == "sparse":
        return np.where(rng.random(shape) < 0.05, rng.uniform(1, 80, shape), 0).astype(np.float32)
    if kind == "dense":
        return rng.uniform(1, 80, shape).astype(np.float32)
    if kind == "straddle":
        t = np.float32(0.001)
        edge = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), np.float32(0.002)], np.float32)
        v = np.where(rng.random(shape) < 0.5, rng.choice(edge, shape), rng.uniform(0.0009, 0.0011, shape)).astype(np.float32)
        return np.where(rng.random(shape) < 0.2, v, 0).astype(np.float32)
    if kind == "mixed":
        v = np.where(rng.random(shape) < 0.15, rng.uniform(-50, 50, shape), 0).astype(np.float32)
        v[rng.random(shape) < 0.05] = np.float32(-0.0)
        return v
    raise ValueError(kind)


def make_mask(kind, rng, x):
    """gt01: x > 0.1 (the kernels' 0 / 1 path); binary: 0 / 1 unrelated to x; fraction: weights that are neither 0 nor 1;
    negative: negative everywhere (a window of negative weights selects its largest product, padding taps at 0 win near the
    border); neg_band: negative in an interior band of rows, x > 0.1 elsewhere; neg_tap: x > 0.1 with one negative tap;
    neg_zero: x > 0.1 with -0.0 in many of its zeros; zero: all zero (every tap of every window ties)."""
    shape = x.shape
    gt = (x > np.float32(0.1)).astype(np.float32)
    if kind == "gt01":
        return gt
    if kind == "binary":
        return (rng.random(shape) < 0.05).astype(np.float32)
    if kind == "fraction":
        return np.where(rng.random(shape) < 0.3, rng.choice(np.float32([0.25, 0.5, 1.5, 2.0, 3.75]), shape), 0).astype(np.float32)
    if kind == "negative":
        return -rng.choice(np.float32([0.5, 1.0, 1.0, 2.0, 0.3]), shape).astype(np.float32)
    if kind == "neg_band":
        m = gt.copy()
        H = shape[1]
        lo, hi = H // 4, max(H // 4 + 1, 3 * H // 4)
        m[:, lo:hi] = -rng.uniform(0.1, 3.0, m[:, lo:hi].shape).astype(np.float32)
        return m
    if kind == "neg_tap":
        m = gt.copy()
        m[(0,) + tuple(s // 2 for s in shape[1:])] = np.float32(-2.0)
        return m
    if kind == "neg_zero":
        return np.where((gt == 0) & (rng.random(shape) < 0.5), np.float32(-0.0), gt).astype(np.float32)
    if kind == "zero":
        return np.zeros(shape, np.float32)
    raise ValueError(kind)

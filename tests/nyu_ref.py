"""The NYU loaders' per-sample work (data_read.py:278-371 and its two copies) as literal numpy: the contract of
dtfill_nyu_read (include/dtfill.h), stated once more and independently of the product.  skimage.transform.resize of a
reduction is scipy.ndimage.gaussian_filter(mode='mirror') followed by scipy.ndimage.zoom(order=1, mode='mirror',
grid_mode=True); tests/test_nyu_read.py holds taps(), filter_pass() and resample() to those two scipy functions.

Everything here is float64 arithmetic, one rounding per operation, in the order written: numpy never contracts a multiply and
an add, and no sum below is handed to np.sum (whose pairwise order is its own).  Helpers only: no fixtures, no hooks."""
import numpy as np

INDEX_ERROR = 1  # DTFILL_NYU_INDEX_ERROR
MAX_RADIUS = 8  # DTFILL_NYU_MAX_RADIUS


def taps(n_in, n_out):
    """(w[0..r] float64, r) of one axis, scipy's _gaussian_kernel1d at sigma = (f - 1) / 2 and radius int(4 sigma + 0.5);
    (None, 0) where the axis has no filter pass (sigma == 0, or a radius of 0: a single tap of 1.0)."""
    assert 1 <= n_out <= n_in
    f = n_in / n_out
    sigma = (f - 1) / 2
    r = int(4.0 * float(sigma) + 0.5)
    if r == 0:
        return None, 0
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:]), r


def mirror(i, n):
    """scipy's 'mirror' of index array i into [0, n): period 2(n-1), the edge sample not repeated, any number of reflections."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def filter_pass(x, axis, w, r, dtype):
    """One correlate1d pass of the symmetric taps w[0..r] along `axis` of x (any rank), accumulated in float64 in scipy's
    order (the centre first, then the pairs from the outermost inwards), the result rounded to `dtype`."""
    x = np.moveaxis(np.asarray(x), axis, 0)
    if r == 0:
        return np.moveaxis(x.astype(dtype), 0, axis)
    n = x.shape[0]
    xd = x.astype(np.float64)
    i = np.arange(n)
    acc = xd * w[0]
    for k in range(r, 0, -1):
        acc = acc + (xd[mirror(i - k, n)] + xd[mirror(i + k, n)]) * w[k]
    return np.moveaxis(acc.astype(dtype), 0, axis)


def gaussian(x, H, W, dtype):
    """Both filter passes on the two leading axes of x [h, w, ...]: axis 0, then axis 1, each rounded to dtype."""
    h, w = x.shape[:2]
    wy, ry = taps(h, H)
    wx, rx = taps(w, W)
    return filter_pass(filter_pass(x, 0, wy, ry, dtype), 1, wx, rx, dtype)


def coords(n_in, n_out):
    """(i0, t) per output index of one axis: c = (j + 0.5) f - 0.5, i0 = floor(c), t = c - i0."""
    f = n_in / n_out
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * f - 0.5
    i0 = np.floor(c)
    return i0.astype(np.int64), c - i0


def resample(x, H, W):
    """The linear resample of x [h, w] (any float dtype) to [H, W] in float64: four products summed from 0.0 on, each a
    sample times its row weight times its column weight, in the order 00, 01, 10, 11."""
    x = np.asarray(x).astype(np.float64)
    h, w = x.shape
    r0, tr = coords(h, H)
    c0, tc = coords(w, W)
    ra, rb = mirror(r0, h)[:, None], mirror(r0 + 1, h)[:, None]
    ca, cb = mirror(c0, w)[None, :], mirror(c0 + 1, w)[None, :]
    tr, tc = tr[:, None], tc[None, :]
    out = 0.0 + x[ra, ca] * (1 - tr) * (1 - tc)
    out = out + x[ra, cb] * (1 - tr) * tc
    out = out + x[rb, ca] * tr * (1 - tc)
    out = out + x[rb, cb] * tr * tc
    return out


def depth_frame(d, H, W):
    """gt float32 [H, W] of one stored float32 depth [h, w]: float32 after each filter pass, the resample in float64, one
    rounding to float32."""
    d = np.asarray(d)
    assert d.dtype == np.float32
    return resample(gaussian(d, H, W, np.float32), H, W).astype(np.float32)


def rgb_frame(u8, H, W, normalize=False, layout="nhwc"):
    """The loader's image of one stored uint8 [C, h, w]: float32(r * 255), or with normalize the drivers'
    float32(float64(float32(r * 255)) / 255.0), as [H, W, C] or [C, H, W]."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 3
    planes = []
    for c in range(u8.shape[0]):
        v = u8[c].astype(np.float64) * (1.0 / 255.0)
        r = resample(gaussian(v, H, W, np.float64), H, W)
        o = (r * 255.0).astype(np.float32)
        if normalize:
            o = (o.astype(np.float64) / 255.0).astype(np.float32)
        planes.append(o)
    out = np.stack(planes)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "nhwc" else out


def sample(gt, samples):
    """(lidar, status) of one frame: gt where a sample marks the pixel, gt * 0.0f elsewhere (the reference's gt * Mask); a
    sample outside the frame is skipped and sets INDEX_ERROR."""
    H, W = gt.shape
    mask = np.zeros((H, W), bool)
    status = 0
    if samples is not None:
        for r, c in np.asarray(samples).reshape(-1, 2):
            if 0 <= r < H and 0 <= c < W:
                mask[r, c] = True
            else:
                status |= INDEX_ERROR
    with np.errstate(invalid="ignore"):
        lidar = np.where(mask, gt, gt * np.float32(0.0))
    return lidar.astype(np.float32), status


def nyu_read(rgb, depth, samples, H, W, normalize=False, layout="nhwc"):
    """The whole call on a batch: rgb uint8 [B, C, h, w] or None, depth float32 [B, h, w] or None, samples int [B, n, 2] or
    None -> (out_rgb or None, gt or None, lidar or None, status int32 [B])."""
    B = len(rgb) if rgb is not None else len(depth)
    out = gt = lidar = None
    status = np.zeros(B, np.int32)
    if rgb is not None:
        out = np.stack([rgb_frame(f, H, W, normalize, layout) for f in rgb])
    if samples is not None:
        for b in range(B):
            status[b] = sample(np.zeros((H, W), np.float32), samples[b])[1]
    if depth is not None:
        gt = np.stack([depth_frame(d, H, W) for d in depth])
        lidar = np.stack([sample(gt[b], None if samples is None else samples[b])[0] for b in range(B)])
    return out, gt, lidar, status


def draw_samples(H, W, sample_rate):
    """The reference's two draws for one frame from numpy's legacy global state (data_read.py:361-363): sample_rate rows
    first, then sample_rate columns, the +6 / +8 added; int32 [sample_rate, 2]."""
    first = np.random.randint(H - 12, size=sample_rate) + 6
    second = np.random.randint(W - 16, size=sample_rate) + 8
    return np.stack([first, second], axis=1).astype(np.int32)


def ulp_distance(a, b):
    """Elementwise distance in units in the last place between two float64 arrays of finite values."""
    def key(x):
        i = np.ascontiguousarray(x, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(key(a) - key(b))

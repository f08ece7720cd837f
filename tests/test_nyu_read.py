"""The NYU loaders' resize and sampling (include/dtfill.h, dtfill_nyu_read) without a GPU: the numpy statement in
tests/nyu_ref.py against scipy.ndimage.gaussian_filter and scipy.ndimage.zoom, bit for bit in both dtypes; hand cases; the
sampling; the legacy-seed parity of nyu_read_batch's draws; the ABI's and the Python layer's argument errors."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import nyu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NYU = ((480, 640, 240, 320), (480, 640, 256, 320))
SMALL = ((13, 17, 6, 8), (12, 9, 5, 9), (3, 5, 1, 2))  # the last: r > n - 1, indices reflect more than once
NON_DYADIC = ((13, 17, 6, 8), (37, 41, 11, 23), (480, 640, 228, 304))
DTYPES = (np.float64, np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), "%s: %d elements differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _field(h, w, dtype, seed=0):
    return (np.random.default_rng(seed).random((h, w)) * 9.5 + 0.5).astype(dtype)


def _sigmas(h, w, H, W):
    return [(h / H - 1) / 2, (w / W - 1) / 2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", NYU + SMALL)
def test_filter_equals_scipy_gaussian_filter(shape, dtype):
    h, w, H, W = shape
    x = _field(h, w, dtype, seed=h + W)
    ref = ndi.gaussian_filter(x, _sigmas(*shape), mode="mirror")
    _same_bits(R.gaussian(x, H, W, dtype), ref, "gaussian %s" % (shape,))


def test_plain_left_to_right_sum_is_not_scipy():
    """The order of the pass is part of the contract: the sum from k = -r to r differs from scipy's in float64."""
    h, w, H, W = NYU[1]
    x = _field(h, w, np.float64)
    wy, ry = R.taps(h, H)
    full = np.concatenate([wy[:0:-1], wy])
    i = np.arange(h)
    acc = np.zeros_like(x)
    for k in range(-ry, ry + 1):
        acc = acc + x[R.mirror(i + k, h)] * full[k + ry]
    ref = ndi.gaussian_filter(x, [_sigmas(h, w, H, W)[0], 0], mode="mirror")
    assert (_bits(acc) != _bits(ref)).any()


@pytest.mark.parametrize("shape", NYU)
def test_resample_equals_scipy_zoom_float64_nyu(shape):
    h, w, H, W = shape
    g = ndi.gaussian_filter(_field(h, w, np.float64, 3), _sigmas(*shape), mode="mirror")
    _same_bits(R.resample(g, H, W), ndi.zoom(g, [H / h, W / w], order=1, mode="mirror", grid_mode=True), "zoom %s" % (shape,))


@pytest.mark.parametrize("shape", NYU + SMALL + NON_DYADIC[1:])
def test_resample_equals_scipy_zoom_float32(shape):
    h, w, H, W = shape
    g = ndi.gaussian_filter(_field(h, w, np.float32, 4), _sigmas(*shape), mode="mirror")
    ref = ndi.zoom(g, [H / h, W / w], order=1, mode="mirror", grid_mode=True)
    _same_bits(R.resample(g, H, W).astype(np.float32), ref, "zoom %s" % (shape,))
    _same_bits(R.depth_frame(_field(h, w, np.float32, 4), H, W), ref, "depth_frame %s" % (shape,))


@pytest.mark.parametrize("shape", NON_DYADIC)
def test_resample_float64_non_dyadic(shape):
    """Largest ulp distance to scipy.ndimage.zoom in float64, measured with scipy 1.15.3: 0 at 13x17->6x8,
    0 at 37x41->11x23, 0 at 480x640->228x304.  scipy's order of operations was found: from 0.0 on, each sample times its row
    weight and then its column weight.  (The sum of x * (wr * wc) is 2, 2 and 4 ulp away at these shapes.)  So the bound
    asserted is the measured 0 and no slack: these shapes are bit for bit too."""
    h, w, H, W = shape
    g = ndi.gaussian_filter(_field(h, w, np.float64, 5), _sigmas(*shape), mode="mirror")
    ref = ndi.zoom(g, [H / h, W / w], order=1, mode="mirror", grid_mode=True)
    got = R.resample(g, H, W)
    print("largest ulp distance at %s: %d" % (shape, R.ulp_distance(got, ref).max()))
    _same_bits(got, ref, "zoom %s" % (shape,))


def test_taps_are_scipys_and_the_products():
    from scipy.ndimage._filters import _gaussian_kernel1d

    for n_in, n_out in ((480, 240), (480, 256), (13, 6), (17, 8), (12, 5), (3, 1), (5, 2), (640, 304), (64, 31), (100, 21)):
        w, r = R.taps(n_in, n_out)
        sigma = (n_in / n_out - 1) / 2
        assert r == int(4.0 * sigma + 0.5)
        full = _gaussian_kernel1d(sigma, 0, r)
        _same_bits(w, np.ascontiguousarray(full[r:]), "taps %d -> %d" % (n_in, n_out))
        _same_bits(np.ascontiguousarray(full[:r + 1][::-1]), w, "symmetric")
    assert R.taps(9, 9) == (None, 0) and R.taps(64, 64) == (None, 0)
    assert R.taps(100, 81) == (None, 0)  # sigma > 0 but a radius of 0: a single tap of 1.0, no pass


def test_product_taps_equal_the_statement(pkg):
    for n_in, n_out in ((480, 240), (480, 256), (640, 320), (13, 6), (3, 1), (64, 31), (9, 9), (100, 81), (100, 21)):
        w, r = pkg.nyu_taps(n_in, n_out)
        rw, rr = R.taps(n_in, n_out)
        assert r == rr and (w is None) == (rw is None)
        if w is not None:
            assert w.dtype == np.float64 and w.flags.c_contiguous and w.shape == (r + 1,)
            _same_bits(w, rw, "taps %d -> %d" % (n_in, n_out))
    for bad in ((4, 5), (0, 0), (5, 0)):
        with pytest.raises(ValueError):
            pkg.nyu_taps(*bad)
    assert R.MAX_RADIUS == pkg._lib.NYU_MAX_RADIUS and R.INDEX_ERROR == pkg._lib.NYU_INDEX_ERROR


def test_mirror():
    assert R.mirror(np.arange(-7, 9), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert R.mirror(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert R.mirror(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]


def test_single_impulse_gives_the_tap_products():
    h, w, H, W = 24, 32, 12, 16  # f = 2 on both axes: r = 2, every resample weight 1/4... the filter is what is looked at
    wy, ry = R.taps(h, H)
    wx, rx = R.taps(w, W)
    x = np.zeros((h, w))
    x[11, 15] = 1.0
    g = R.gaussian(x, H, W, np.float64)
    fy = np.concatenate([wy[:0:-1], wy])
    fx = np.concatenate([wx[:0:-1], wx])
    want = np.zeros((h, w))
    want[11 - ry:11 + ry + 1, 15 - rx:15 + rx + 1] = fy[:, None] * fx[None, :]
    _same_bits(g, want, "impulse")
    # next to the edge the mirrored taps fold onto their images: row 0's response to an impulse in row 1 is w[1] twice
    x = np.zeros((h, w))
    x[1, 15] = 1.0
    g = R.filter_pass(x, 0, wy, ry, np.float64)
    assert g[0, 15] == (0.0 * wy[0] + (0.0 + 0.0) * wy[2]) + (1.0 + 1.0) * wy[1]
    assert g[1, 15] == wy[0] + wy[2] and g[3, 15] == wy[2]  # row 1 is its own image two rows up: m(1 - 2) = 1


def test_identity_axis_is_copied():
    h, w, H, W = 64, 64, 64, 31
    x = _field(h, w, np.float64, 6)
    assert R.taps(h, H) == (None, 0)
    g = R.gaussian(x, H, W, np.float64)
    only_x = ndi.gaussian_filter(x, [0, _sigmas(h, w, H, W)[1]], mode="mirror")
    _same_bits(g, only_x, "axis 0 has no pass")
    out = R.resample(g, H, W)
    # f == 1 on axis 0: t = 0, row i of the output is the column resample of row i alone
    for i in (0, 17, 63):
        _same_bits(out[i:i + 1], R.resample(g[i:i + 1], 1, W), "row %d" % i)
    _same_bits(R.resample(x, h, w), x, "f == 1 on both axes: the identity")
    # the neighbour of weight 0 is still read: a NaN in row i + 1 reaches row i
    y = x.copy()
    y[18, 5] = np.nan
    got = R.resample(y, h, w)
    assert np.isnan(got[17, 5]) and np.isnan(got[18, 5]) and np.isfinite(got[19, 5])


def test_rgb_frame_paths():
    u8 = np.random.default_rng(8).integers(0, 256, (3, 13, 17)).astype(np.uint8)
    H, W = 6, 8
    out = R.rgb_frame(u8, H, W)
    assert out.dtype == np.float32 and out.shape == (H, W, 3)
    for c in range(3):
        v = u8[c].astype(np.float64) * (1.0 / 255.0)
        g = ndi.gaussian_filter(v, _sigmas(13, 17, H, W), mode="mirror")
        z = ndi.zoom(g, [H / 13, W / 17], order=1, mode="mirror", grid_mode=True)
        _same_bits(out[..., c], (z * 255).astype(np.float32), "channel %d" % c)
        nrm = R.rgb_frame(u8, H, W, normalize=True, layout="nchw")
        _same_bits(nrm[c], ((z * 255).astype(np.float32) / 255.0).astype(np.float32), "normalized channel %d" % c)


def test_sampling():
    gt = _field(20, 30, np.float32, 9)
    gt[7, 9] = -2.5
    gt[8, 9] = np.nan
    gt[9, 9] = np.inf
    samples = np.array([[6, 8], [6, 8], [13, 21], [6, 8], [19, 29], [0, 0]], np.int32)  # duplicates
    lidar, st = R.sample(gt, samples)
    assert st == 0 and lidar.dtype == np.float32
    with np.errstate(invalid="ignore"):
        ref = gt * np.zeros((20, 30))  # the reference's float64 Mask
        zeros = ref.astype(np.float32)
    ref[[6, 13, 19, 0], [8, 21, 29, 0]] = gt[[6, 13, 19, 0], [8, 21, 29, 0]]
    _same_bits(lidar, ref.astype(np.float32), "gt * Mask")
    assert np.signbit(lidar[7, 9]) and lidar[7, 9] == 0  # -0.0 under a negative gt
    assert np.isnan(lidar[8, 9]) and np.isnan(lidar[9, 9])  # NaN * 0 and inf * 0
    assert not np.signbit(lidar[0, 1]) and lidar[0, 1] == 0
    # n == 0 and no samples at all
    for none in (np.zeros((0, 2), np.int32), None):
        lidar, st = R.sample(gt, none)
        _same_bits(lidar, zeros, "no sample")
        assert st == 0
    # an index outside the frame is skipped and flagged; the others still count
    for bad in ([20, 3], [3, 30], [-1, 3], [3, -1]):
        lidar, st = R.sample(gt, np.array([[6, 8], bad], np.int32))
        assert st == R.INDEX_ERROR and lidar[6, 8] == gt[6, 8] and np.count_nonzero(lidar == gt) == 1


def test_draws_follow_the_legacy_seed():
    H, W, n = 240, 320, 64
    np.random.seed(5)
    a = R.draw_samples(H, W, n)
    np.random.seed(5)
    first = np.random.randint(H - 12, size=n)
    second = np.random.randint(W - 16, size=n)
    assert np.array_equal(a[:, 0], first + 6) and np.array_equal(a[:, 1], second + 8)
    Mask = np.zeros((H, W))
    Mask[first + 6, second + 8] = 1  # data_read.py:360-363
    gt = _field(H, W, np.float32, 10)
    _same_bits(R.sample(gt, a)[0], (gt * Mask).astype(np.float32), "the reference's mask")


def test_argument_errors_without_gpu(pkg):
    """Every return code and the workspace rule, through the ABI: the checks come before the first HIP call."""
    L = pkg.load()
    wsb = L.dtfill_nyu_read_workspace_bytes
    ws = wsb(2, 240, 320)
    assert ws == (2 * (240 * 320 // 32) * 4 + 255) // 256 * 256 and ws % 256 == 0
    assert wsb(1, 1, 1) == 256 and wsb(3, 5, 7) == 256  # one bit per output pixel, a word at least per frame
    assert wsb(0, 8, 8) == 0 and wsb(1, 0, 8) == 0 and wsb(1, 8, -1) == 0 and wsb(65536, 1, 1) == 0
    assert wsb(2, 1 << 15, 1 << 15) == 0 and wsb(1, 1 << 15, (1 << 16) - 1) > 0
    import ctypes

    wy, ry = pkg.nyu_taps(480, 240)
    wx, rx = pkg.nyu_taps(640, 320)
    WY, WX = wy.ctypes.data, wx.ctypes.data
    big = (ctypes.c_double * 16)(*([1.0 / 17] * 16))
    BIG = ctypes.addressof(big)

    def call(rgb=256, depth=512, B=2, C=3, hin=480, win=640, H=240, W=320, wy=WY, ry=ry, wx=WX, rx=rx, samples=768, n=64,
             normalize=0, layout=0, out_rgb=1024, gt=1280, lidar=1536, st=1792, w=4096, nws=None):
        return L.dtfill_nyu_read(rgb, depth, B, C, hin, win, H, W, wy, ry, wx, rx, samples, n, normalize, layout, out_rgb, gt,
                                 lidar, st, w, ws if nws is None else nws, None)

    for kw in (dict(rgb=None, depth=None, out_rgb=None, gt=None, lidar=None), dict(w=None),
               dict(rgb=None), dict(depth=None),              # an output without its input
               dict(depth=None, gt=None), dict(depth=None, lidar=None),
               dict(out_rgb=None), dict(gt=None, lidar=None)):  # an input without an output
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(hin=0), dict(win=-2), dict(H=0), dict(W=0), dict(B=65536, hin=1, win=1, H=1, W=1),
               dict(H=481), dict(W=641),                      # an enlargement
               dict(ry=9, wy=BIG), dict(rx=9, wx=BIG), dict(ry=-1), dict(rx=-1),  # a radius outside [0, DTFILL_NYU_MAX_RADIUS]
               dict(wy=None), dict(wx=None), dict(ry=0), dict(rx=0),  # taps and radius disagree about the pass
               dict(C=0), dict(C=5), dict(layout=2), dict(layout=-1), dict(n=-1),
               dict(B=2, hin=1 << 15, win=1 << 15, C=1),       # 2^31 source pixels
               dict(B=1, hin=1 << 15, win=1 << 14, C=4),       # 2^31 source bytes of the image
               dict(B=1, hin=1 << 15, win=1 << 14, H=1 << 15, W=1 << 14, C=4, nws=1 << 40),  # 2^31 output elements too
               dict(B=2, n=1 << 29)):                          # 2^31 sample coordinates
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3
    assert call(w=4100) == -3  # not 256-byte aligned
    # the largest shapes inside the limits are no shape error (too small a workspace is the next check); C and layout are
    # not looked at without an image; a radius at the cap is taken
    assert call(B=1, hin=1 << 15, win=(1 << 14) - 1, C=4, nws=0) == -3
    assert call(rgb=None, out_rgb=None, C=0, layout=7, nws=0) == -3
    assert call(ry=8, wy=BIG, rx=8, wx=BIG, nws=0) == -3
    assert call(samples=None, n=0, nws=0) == -3 and call(gt=None, nws=0) == -3 and call(lidar=None, st=None, nws=0) == -3
    import re

    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    assert int(re.search(r"#define DTFILL_NYU_MAX_RADIUS\s+(\d+)", src).group(1)) == pkg._lib.NYU_MAX_RADIUS >= 8
    assert int(re.search(r"#define DTFILL_NYU_INDEX_ERROR\s+(\d+)", src).group(1)) == pkg._lib.NYU_INDEX_ERROR


def test_python_layer_errors_without_gpu(pkg):
    rgb = np.zeros((2, 3, 48, 64), np.uint8)
    depth = np.zeros((2, 48, 64), np.float32)
    for bad_rgb, bad_depth, exc in ((rgb.astype(np.float32), depth, TypeError), (rgb, depth.astype(np.complex64), TypeError),
                                    (rgb, depth[:1], ValueError), (rgb, depth[:, :40], ValueError), (rgb[0], depth, ValueError),
                                    (rgb[:, :, :0], depth[:, :0], ValueError)):
        with pytest.raises(exc):
            pkg.nyu_read_batch(bad_rgb, bad_depth, size=(24, 32))
    for kw in (dict(size=(49, 32)), dict(size=(24, 65)), dict(size=(0, 32)), dict(size=(24.5, 32)), dict(size=24),
               dict(size=(12, 32)), dict(size=(24, 16)), dict(sample_rate=-1), dict(sample_rate=2.5)):
        with pytest.raises(ValueError):
            pkg.nyu_read_batch(rgb, depth, **{"size": (24, 32), **kw})
    assert callable(pkg.nyu_read_device) and callable(pkg.device.nyu_read_device)
    import dtfill_amd

    assert dtfill_amd.nyu_read_batch is pkg.nyu_read_batch and dtfill_amd.nyu_taps is pkg.nyu_taps


def test_nyu_dense_scenes(pkg):
    synth = __import__("importlib").import_module(pkg.__name__ + ".synth")
    depth, rgb = synth.nyu_dense(2, seed=3, hw=(60, 80))
    assert depth.dtype == np.float32 and depth.shape == (2, 60, 80) and rgb.dtype == np.uint8 and rgb.shape == (2, 3, 60, 80)
    assert depth.min() >= 0.5 and depth.max() <= 10.0 and np.ptp(depth) > 1.0 and len(np.unique(rgb)) > 100
    again = synth.nyu_dense(2, seed=3, hw=(60, 80))
    assert np.array_equal(depth, again[0]) and np.array_equal(rgb, again[1])
    assert synth.nyu_dense(1)[0].shape == (1, 480, 640)


def test_product_does_not_import_nyu_ref():
    pkgdir = os.path.join(ROOT, "distancetransform-depthcompletion_amd")
    for dp, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp")):
                assert "nyu_ref" not in open(os.path.join(dp, f)).read(), f

"""The NYU loaders' resize and sampling on the device (dtfill_nyu_read, nyu_read_device, nyu_read_batch) against the numpy
statement in tests/nyu_ref.py, which tests/test_nyu_read.py pins to scipy.ndimage.  Bit for bit everywhere (a NaN is compared
as a NaN: which payload an operation on NaNs returns is the hardware's).  Every call through the C ABI here runs in guarded
buffers with poisoned outputs and a poisoned workspace, inputs and outputs only element-aligned (_abi)."""
import functools
import importlib

import numpy as np
import pytest

import concurrency
import nyu_ref as R
from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("nhwc", "nchw")
TH, TW = 16, 32  # dtfill_nyu.hpp: NY_TH, NY_TW, the tile of output pixels
NYU = ((480, 640, 240, 320), (480, 640, 256, 320))
SHAPES = NYU + ((13, 17, 6, 8), (12, 9, 5, 9), (3, 5, 1, 2), (37, 41, 11, 23), (480, 640, 228, 304))
SEAMS = ((2 * (TH - 1), 2 * (TW - 1), TH - 1, TW - 1),  # one tile - 1 on each axis
         (2 * TH, 2 * TW, TH, TW),                      # one tile exactly
         (2 * (TH + 1), 2 * (TW + 1), TH + 1, TW + 1),  # one tile + 1: a second tile of one row / one column
         (2 * TH, 2 * (TW + 1), TH, TW + 1),            # ... on one axis only
         (2 * (TH + 1), 2 * TW, TH + 1, TW),
         (2 * (2 * TH + 1), 2 * (2 * TW + 1), 2 * TH + 1, 2 * TW + 1),  # two tiles + 1
         (80, 150, 2 * TH + 1, 2 * TW + 1),             # f = 2.42 / 2.31, r = 3: the halo crosses both seams at odd offsets
         (50, 100, 2 * TH + 1, 2 * TW + 1))             # f = 1.52 / 1.54, r = 1


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


@functools.lru_cache(maxsize=None)
def _inputs(B, C, h, w, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * h + w + C)
    rgb = rng.integers(0, 256, (B, C, h, w)).astype(np.uint8)
    depth = (rng.random((B, h, w)) * 9.5 + 0.5).astype(np.float32)
    for a in (rgb, depth):
        a.setflags(write=False)
    return rgb, depth


def _samples(B, H, W, n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))], axis=2).astype(np.int32)


def _same(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    if got.dtype == np.float32:
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), "%s: the NaNs lie elsewhere" % what
        bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    else:
        bad = got != ref
    assert not bad.any(), "%s: %d elements differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _abi(pkg, rgb, depth, samples, H, W, normalize=False, layout="nhwc", offsets=(1, 4, 4, 4, 4), kind="ones", seed=0,
         want=("rgb", "gt", "lidar", "status"), stream=None, ws_stream=None):
    """dtfill_nyu_read on numpy rgb uint8 [B, C, h, w] / depth float32 [B, h, w] / samples int32 [B, n, 2] (each may be None),
    the inputs and outputs `offsets` bytes (rgb, depth, out_rgb, gt, lidar) after a 256-byte boundary, every buffer between
    guards, outputs and workspace poisoned.  Checks the guards, that the inputs are unchanged and that no output element is
    left poisoned; returns (out_rgb, gt, lidar, status) as numpy, None for what was not asked for."""
    import torch

    L = pkg._lib.load()
    first = rgb if rgb is not None else depth
    B, (h, w) = first.shape[0], first.shape[-2:]
    C = rgb.shape[1] if rgb is not None else 1
    (wy, ry), (wx, rx) = pkg.nyu_taps(h, H), pkg.nyu_taps(w, W)
    nws = L.dtfill_nyu_read_workspace_bytes(B, H, W)
    assert nws > 0
    ro, do, oo, go, lo = offsets
    bufs = []

    def put(a, off, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        g = GuardedBuffer(a.nbytes, off, DEV, a.nbytes // B)
        g.payload().copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        bufs.append((g, what))
        return g

    def out(n, off, what, pname):
        g = GuardedBuffer(4 * n, off, DEV, 4 * n // B)
        poison_output(g.view(torch.int32 if pname == "status" else torch.float32, (n,)), pname)
        bufs.append((g, what))
        return g

    rg, dg, sg = put(rgb, ro, "rgb"), put(depth, do, "depth"), put(samples, 0, "samples")
    og = out(B * H * W * C, oo, "out_rgb", "depth") if rgb is not None and "rgb" in want else None
    gg = out(B * H * W, go, "out_gt", "depth") if depth is not None and "gt" in want else None
    lg = out(B * H * W, lo, "out_lidar", "depth") if depth is not None and "lidar" in want else None
    tg = out(B, 0, "status", "status") if "status" in want else None
    if ws_stream is None:
        wg = GuardedBuffer(nws, 0, DEV)
    else:
        with torch.cuda.stream(ws_stream):  # the workspace belongs to another stream's pool
            wg = GuardedBuffer(nws, 0, DEV)
        ws_stream.synchronize()
    poison(wg.payload(), kind, seed=seed)
    bufs.append((wg, "workspace"))
    ptr = lambda g: None if g is None else g.ptr
    tap = lambda t: None if t is None else t.ctypes.data
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    rc = L.dtfill_nyu_read(ptr(rg), ptr(dg), B, C, h, w, H, W, tap(wy), ry, tap(wx), rx, ptr(sg),
                           0 if samples is None else samples.shape[1], int(normalize), LAYOUTS.index(layout), ptr(og), ptr(gg),
                           ptr(lg), ptr(tg), wg.ptr, nws, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in bufs:
        g.check(what)
    for g, a, what in ((rg, rgb, "rgb"), (dg, depth, "depth"), (sg, samples, "samples")):
        if g is not None:
            assert np.array_equal(g.payload().cpu().numpy(), np.ascontiguousarray(a).reshape(-1).view(np.uint8)), what + " changed"
    res = []
    for g, shape in ((og, (B, H, W, C) if layout == "nhwc" else (B, C, H, W)), (gg, (B, H, W)), (lg, (B, H, W))):
        if g is None:
            res.append(None)
            continue
        a = g.view(torch.float32, shape).cpu().numpy()
        assert not is_poison(a, "depth").any(), "output elements left unwritten"
        res.append(a)
    if tg is None:
        res.append(None)
    else:
        s = tg.view(torch.int32, (B,)).cpu().numpy()
        assert not is_poison(s, "status").any()
        res.append(s)
    return res


def _check_abi(pkg, shape, B=3, C=3, samples="some", what="", seed=0, **kw):
    h, w, H, W = shape
    rgb, depth = _inputs(B, C, h, w, seed)
    smp = _samples(B, H, W, max(1, H * W // 7), seed) if samples == "some" else samples
    got = _abi(pkg, rgb, depth, smp, H, W, seed=seed, **kw)
    ref = R.nyu_read(rgb, depth, smp, H, W, kw.get("normalize", False), kw.get("layout", "nhwc"))
    for g, r, name in zip(got, ref, ("rgb", "gt", "lidar", "status")):
        _same(g, r, "%s %s %s" % (what, shape, name))
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_bit_exact(pkg, shape):
    k = SHAPES.index(shape)
    _check_abi(pkg, shape, normalize=k % 2 == 1, layout=LAYOUTS[k % 2], kind=KINDS[k % 3], seed=k)


@pytest.mark.parametrize("shape", SEAMS)
def test_tile_seams(pkg, shape):
    k = SEAMS.index(shape)
    _check_abi(pkg, shape, layout=LAYOUTS[k % 2], kind=KINDS[k % 3], seed=20 + k, offsets=(3, 12, 4, 8, 12))


def test_one_axis_without_a_pass(pkg):
    assert pkg.nyu_taps(64, 64) == (None, 0)
    _check_abi(pkg, (64, 64, 64, 31), seed=40)
    _check_abi(pkg, (64, 64, 31, 64), seed=41, layout="nchw")
    _check_abi(pkg, (20, 33, 20, 33), seed=42)  # neither: the identity, through the resample's weights of 1 and 0


def test_factor_that_shrinks_the_tile(pkg):
    """f = 5, r = 8 (the cap): the source of a 16 x 32 tile of the depth does not fit the LDS budget, the tile is halved."""
    assert pkg.nyu_taps(100, 20)[1] == R.MAX_RADIUS
    _check_abi(pkg, (100, 200, 20, 40), B=2, seed=43)
    _check_abi(pkg, (90, 170, 19, 37), B=2, seed=44, layout="nchw", normalize=True)


@pytest.mark.parametrize("C", [1, 2, 4])
def test_channels(pkg, C):
    for layout in LAYOUTS:
        _check_abi(pkg, (37, 41, 17, 33), C=C, layout=layout, normalize=C == 4, seed=50 + C)


def test_layouts_and_normalize(pkg):
    n = 0
    for layout in LAYOUTS:
        for normalize in (False, True):
            got = _check_abi(pkg, (48, 70, 24, 35), layout=layout, normalize=normalize, seed=60, kind=KINDS[n % 3])
            n += 1
            if normalize:
                assert got[0].min() >= 0.0 and got[0].max() < 1.001
    # the two forms of one image: / 255 of the loader's values
    rgb, depth = _inputs(3, 3, 48, 70, 60)
    a = _abi(pkg, rgb, None, None, 24, 35)[0]
    b = _abi(pkg, rgb, None, None, 24, 35, normalize=True)[0]
    _same(b, (a.astype(np.float64) / 255.0).astype(np.float32), "img / 255.0")
    assert a.max() > 200.0


def test_parts_of_the_call(pkg):
    shape = (37, 41, 17, 33)
    h, w, H, W = shape
    rgb, depth = _inputs(3, 3, h, w, 70)
    smp = _samples(3, H, W, 50, 70)
    ref = R.nyu_read(rgb, depth, smp, H, W)
    got = _abi(pkg, rgb, None, smp, H, W)  # the image alone (the samples are still checked)
    assert got[1] is None and got[2] is None
    _same(got[0], ref[0], "rgb alone")
    _same(got[3], ref[3], "status, rgb alone")
    got = _abi(pkg, None, depth, smp, H, W)  # the depth alone
    assert got[0] is None
    _same(got[1], ref[1], "gt, depth alone")
    _same(got[2], ref[2], "lidar, depth alone")
    for want in (("gt",), ("lidar",), ("rgb", "gt"), ("rgb", "lidar", "status")):  # one output of the depth at a time, no status
        got = _abi(pkg, rgb if "rgb" in want else None, depth, smp, H, W, want=want)  # (an input needs an output)
        for g, r, name in zip(got, ref, ("rgb", "gt", "lidar", "status")):
            if name in want:
                _same(g, r, "%s of %s" % (name, want))
            else:
                assert g is None
    zeros = R.nyu_read(None, depth, None, H, W)
    assert not zeros[2].any() and not zeros[3].any()
    for none in (None, np.zeros((3, 0, 2), np.int32)):  # samples NULL, and n == 0
        got = _abi(pkg, rgb, depth, none, H, W, kind="random", seed=5)
        _same(got[2], zeros[2], "lidar without samples")
        _same(got[1], ref[1], "gt without samples")
        _same(got[3], zeros[3], "status without samples")


def test_sampling_cases(pkg):
    h, w, H, W = 40, 66, 20, 33
    rgb, depth = _inputs(2, 3, h, w, 80)
    depth = depth.copy()
    depth[0, :12, :14] = -3.0      # a negative patch: gt < 0 there, lidar -0.0
    depth[1, 30, 40] = np.nan      # a planted NaN: gt is NaN around it, lidar NaN whether marked or not
    depth[1, 5, 60] = np.inf
    smp = np.array([[[2, 3], [2, 3], [10, 30], [2, 3], [19, 32], [0, 0], [10, 30], [15, 20]],          # duplicates
                    [[15, 20], [20, 3], [3, 33], [-1, 3], [3, -1], [19, 32], [15, 19], [2, 30]]], np.int32)  # four outside
    got = _abi(pkg, rgb, depth, smp, H, W)
    ref = R.nyu_read(rgb, depth, smp, H, W)
    for g, r, name in zip(got, ref, ("rgb", "gt", "lidar", "status")):
        _same(g, r, name)
    gt, lidar, st = got[1:]
    assert st.tolist() == [0, R.INDEX_ERROR]
    assert gt[0, 1, 1] < 0 and lidar[0, 1, 1] == 0 and np.signbit(lidar[0, 1, 1])    # unmarked under a negative gt: -0.0
    assert lidar[0, 2, 3] == gt[0, 2, 3] < 0                                         # marked: the value
    assert lidar[0, 10, 31] == 0 and not np.signbit(lidar[0, 10, 31])
    assert np.isnan(gt[1, 15, 20]) and np.isnan(lidar[1, 15, 20]) and np.isnan(lidar[1, 15, 21])
    assert np.isnan(lidar[1, 15, 19])                                                # marked, and gt is NaN there
    assert np.isinf(gt[1, 2, 30]) and lidar[1, 2, 30] == gt[1, 2, 30]                # marked under the inf: the value
    assert np.isinf(gt[1, 2, 29]) and np.isnan(lidar[1, 2, 29])                      # unmarked: inf * 0
    assert lidar[1, 19, 32] == gt[1, 19, 32] > 0
    assert np.count_nonzero(lidar[0] == gt[0]) == 5                                  # five distinct pixels marked


@functools.lru_cache(maxsize=None)
def _nyu_case(H, W):
    """Two synthetic stored samples and what the statement makes of them at (H, W), 64 samples a frame drawn as the reference
    draws them."""
    pkg = importlib.import_module("distancetransform-depthcompletion_amd")
    synth = importlib.import_module(pkg.__name__ + ".synth")
    depth, rgb = synth.nyu_dense(2, seed=H)
    np.random.seed(H)
    smp = np.stack([R.draw_samples(H, W, 64) for _ in range(2)])
    ref = R.nyu_read(rgb, depth, smp, H, W)
    for a in (rgb, depth, smp) + ref:
        a.setflags(write=False)
    return rgb, depth, smp, ref


@pytest.mark.parametrize("size", [(240, 320), (256, 320)])
def test_nyu_geometry_on_dense_scenes(pkg, dev, size):
    import torch

    rgb, depth, smp, ref = _nyu_case(*size)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    got = dev.nyu_read_device(up(rgb), up(depth), up(smp), size)
    for g, r, name in zip(got, ref, ("rgb", "gt", "lidar", "status")):
        _same(g.cpu().numpy(), r, "%s %s" % (size, name))
    assert tuple(got[0].shape) == (2,) + size + (3,) and int((got[2] != 0).sum()) > 100
    # the numpy function: the reference's seed gives the reference's mask, and its three arrays in its order
    np.random.seed(size[0])
    img, lidar, gt = pkg.nyu_read_batch(rgb, depth, 64, size)
    _same(img, ref[0], "nyu_read_batch img")
    _same(lidar, ref[2], "nyu_read_batch lidar")
    _same(gt, ref[1], "nyu_read_batch gt")
    with pytest.raises(IndexError):
        pkg.nyu_read_batch(rgb, depth, size=size, samples=np.array([[[6, 8]], [[size[0], 8]]]))
    one = pkg.nyu_read_batch(rgb[0], depth[0], size=size, samples=smp[:1])  # one stored sample, as read_one_val_NYU
    _same(one[1], ref[2][:1], "one sample")


@pytest.mark.parametrize("metric", ["l1_cv", "l2"])
@pytest.mark.parametrize("sample_rate", [20, 500])
def test_lidar_feeds_the_fill(pkg, dev, oracle, metric, sample_rate):
    import torch

    rgb, depth, _, ref = _nyu_case(240, 320)
    np.random.seed(sample_rate)
    smp = np.stack([R.draw_samples(240, 320, sample_rate) for _ in range(2)])
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    _, gt, lidar, st = dev.nyu_read_device(None, up(depth), up(smp), (240, 320))
    want_lidar = np.stack([R.sample(ref[1][b], smp[b])[0] for b in range(2)])
    _same(lidar.cpu().numpy(), want_lidar, "lidar")
    assert not st.cpu().numpy().any()
    got = pkg.device.DtFill(device=DEV, metric=metric).run(lidar, 0.001, 0.1)  # eval_NYU.py's thresholds
    d, dt, idx, status = oracle.fill_batch(want_lidar, 0.001, 0.1, metric=metric)
    assert np.array_equal(got["status"].cpu().numpy() & 1, status)
    assert np.array_equal(got["index"].cpu().numpy(), idx)
    _same(got["dt"].cpu().numpy(), dt, "dt")
    ok = status == 0
    assert ok.any()
    _same(got["depth"].cpu().numpy()[ok], d[ok], "filled depth")


def test_python_layer_errors(pkg, dev):
    import torch

    rgb, depth = (torch.from_numpy(np.array(a)).to(DEV) for a in _inputs(2, 3, 100, 100, 90))
    with pytest.raises(ValueError, match="radius"):
        dev.nyu_read_device(rgb, depth, None, (10, 10))  # f = 10: a radius of 18
    for bad in (dict(rgb=rgb.float()), dict(depth=depth.double()), dict(depth=depth[:1]), dict(rgb=rgb.cpu()),
                dict(samples=torch.zeros((2, 4, 2), dtype=torch.int64, device=DEV)),
                dict(samples=torch.zeros((2, 4, 3), dtype=torch.int32, device=DEV)), dict(size=(101, 50)), dict(size=(50,)),
                dict(layout="hwc"), dict(rgb=None, depth=None)):
        kw = dict(rgb=rgb, depth=depth, samples=None, size=(50, 50))
        kw.update(bad)
        with pytest.raises(ValueError):
            dev.nyu_read_device(kw.pop("rgb"), kw.pop("depth"), **kw)


def test_streams_and_threads(pkg, dev):
    """One ABI call on a non-default stream in a workspace that another stream allocated; then nyu_read_device from two host
    threads, each on a stream of its own, two rounds."""
    import torch

    A, B = (torch.cuda.Stream(device=DEV) for _ in range(2))
    shape = (80, 150, 2 * TH + 1, 2 * TW + 1)
    h, w, H, W = shape
    rgb, depth = _inputs(3, 3, h, w, 95)
    smp = _samples(3, H, W, 300, 95)
    ref = R.nyu_read(rgb, depth, smp, H, W)
    got = _abi(pkg, rgb, depth, smp, H, W, stream=B, ws_stream=A, kind="random", seed=9)
    for g, r, name in zip(got, ref, ("rgb", "gt", "lidar", "status")):
        _same(g, r, "stream B, workspace of stream A: " + name)
    streams = (A, B)
    dev_in = [tuple(torch.from_numpy(np.array(a)).to(DEV) for a in (rgb, depth, smp)) for _ in streams]
    refs = (ref, R.nyu_read(rgb, depth, smp, H, W, True, "nchw"))
    torch.cuda.synchronize()

    def work(k, r):
        with torch.cuda.stream(streams[k]):
            out = dev.nyu_read_device(*dev_in[k], size=(H, W), normalize=(k + r) % 2 == 1, layout=LAYOUTS[(k + r) % 2])
            out = [t.cpu().numpy() for t in out]  # (.cpu() waits for the current stream)
        for g, want, name in zip(out, refs[(k + r) % 2], ("rgb", "gt", "lidar", "status")):
            _same(g, want, "thread %d round %d %s" % (k, r, name))

    failures = concurrency.run_rounds(work, 2, 2)
    assert not failures, concurrency.describe(failures)

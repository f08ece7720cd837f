"""dtfill_conv2d on the device against the numpy statement of its contract (tests/conv_ref.py), bit for bit (+0 == -0, a NaN
matches a NaN), through the ABI on guarded buffers.  This is also the measurement of what the contract rests on: that gfx950's
float32-input MFMA adds its k-products to the accumulator in k order with one rounding each, as an fmaf chain does."""
import numpy as np
import pytest

import conv_ref as R
from guarded import GuardedBuffer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
TILE_H, TILE_W, MFMA_M = 8, 32, 16  # CV_TH, CV_TW, CV_M of csrc/dtfill_conv.hpp
POISON = 0x7FA7C3D1  # a NaN payload no case computes
# (B, H, W): one pixel; a frame smaller than the 7x7 window; H and W one below, at and one above the block tile (W: and the
# 16-pixel MFMA row), two frames
SHAPES = ((1, 1, 1), (1, 3, 5), (2, TILE_H - 1, MFMA_M - 1), (1, TILE_H, MFMA_M), (1, TILE_H + 1, MFMA_M + 1),
          (1, TILE_H - 1, TILE_W - 1), (1, TILE_H, TILE_W), (2, TILE_H + 1, TILE_W + 1))
LAYERS = R.NET_LAYERS  # every layer of the net; Cin 32 and 48 are conv1a's at scale_num 2 and 3


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def _up(a, offset=0):
    import torch

    a = np.ascontiguousarray(a)
    g = GuardedBuffer(a.nbytes, offset, DEV)
    g.payload().copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    return g


def _poisoned(shape, offset=0):
    import torch

    g = GuardedBuffer(int(np.prod(shape)) * 4, offset, DEV)
    g.view(torch.int32, shape).fill_(POISON)
    return g


def run(L, x, w, bias, act, alpha=0.2, out_channels=None, out_offset=0, x_offset=0, out_offset_bytes=0, stream=None):
    """One call through the ABI on guarded buffers; returns the whole out tensor [B,H,W,out_channels], poison where the call
    wrote nothing."""
    import torch

    B, H, W, cin = x.shape
    ksize, cout = w.shape[0], w.shape[3]
    out_channels = cout if out_channels is None else out_channels
    gx, gw = _up(x, x_offset), _up(w)
    gb = None if bias is None else _up(bias)
    go = _poisoned((B, H, W, out_channels), out_offset_bytes)
    rc = L.dtfill_conv2d(gx.ptr, B, H, W, cin, gw.ptr, gb.ptr if gb else None, ksize, cout, act, alpha, go.ptr, out_channels,
                         out_offset, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in ((gx, "x"), (gw, "w"), (go, "out")) + (((gb, "bias"),) if gb else ()):
        g.check(what)
    return go.view(torch.float32, (B, H, W, out_channels)).cpu().numpy()


def case(ksize, cin, cout, shape, seed):
    """Values with long mantissas and mixed magnitudes, a third of the inputs zero: a chain whose roundings depend on its order."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape + (cin,)) * 2.0 ** rng.integers(-3, 4, shape + (cin,))).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    return x, w, rng.standard_normal(cout).astype(F)


_reference = {}


def reference(ksize, cin, cout, act, shape, seed, bias=True):
    """conv_ref of case(), worked out once per case and shared."""
    key = (ksize, cin, cout, act, shape, seed, bias)
    if key not in _reference:
        x, w, b = case(ksize, cin, cout, shape, seed)
        _reference[key] = R.conv_ref(x, w, b if bias else None, act, 0.2)
    return _reference[key]


@pytest.mark.parametrize("ksize,cin,cout,act", LAYERS)
def test_every_layer_at_every_tile_seam(L, ksize, cin, cout, act):
    for n, shape in enumerate(SHAPES):
        x, w, b = case(ksize, cin, cout, shape, n)
        got = run(L, x, w, b, act)
        R.assert_same(got, reference(ksize, cin, cout, act, shape, n), "%dx%dx%d->%d at %s" % (ksize, ksize, cin, cout, shape))


@pytest.mark.parametrize("ksize,cin,cout,act", ((7, 64, 16, R.LEAKY), (3, 1, 16, R.LEAKY), (3, 16, 1, R.LINEAR)))
def test_out_offset_misalignment_and_null_bias(L, ksize, cin, cout, act):
    shape = (1, TILE_H + 1, MFMA_M + 1)
    x, w, b = case(ksize, cin, cout, shape, 3)
    want = reference(ksize, cin, cout, act, shape, 3)
    # into channels 16 .. 16 + Cout - 1 of a wider tensor: the others keep their poison
    wide = run(L, x, w, b, act, out_channels=40, out_offset=16)
    R.assert_same(wide[..., 16:16 + cout], want, "out_offset")
    rest = np.delete(wide, np.s_[16:16 + cout], axis=-1)
    assert (rest.view(np.uint32) == POISON).all()
    # x and out 4 bytes off a 16-byte boundary
    R.assert_same(run(L, x, w, b, act, x_offset=4, out_offset_bytes=4), want, "misaligned")
    R.assert_same(run(L, x, w, None, act), reference(ksize, cin, cout, act, shape, 3, bias=False), "NULL bias")


@pytest.mark.parametrize("ksize,cin,cout,act", ((7, 32, 16, R.LEAKY), (7, 1, 16, R.LEAKY), (3, 16, 1, R.LINEAR)))
def test_non_finite_values_follow_fmaf(L, ksize, cin, cout, act):
    """An inf and a NaN input, and an infinite weight on a corner tap: the pixels whose window holds them are inf or NaN as the
    chain makes them (a padding tap under the infinite weight is +0 * inf = NaN), every other pixel is untouched by them."""
    shape = (1, TILE_H + 1, MFMA_M + 1)
    x, w, b = case(ksize, cin, cout, shape, 5)
    x[0, 2, 3, 0], x[0, 6, 12, cin - 1] = np.inf, np.nan
    want = R.conv_ref(x, w, b, act, 0.2)
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    R.assert_same(run(L, x, w, b, act), want, "inf and NaN inputs")
    w[0, 0, 0, 0] = np.inf
    want = R.conv_ref(x, w, b, act, 0.2)
    assert np.isnan(want[0, 0, 0, 0])  # the corner's tap (0, 0) is padding
    R.assert_same(run(L, x, w, b, act), want, "an infinite weight")


def test_bits_do_not_depend_on_the_run_or_the_batch_position(L):
    ksize, cin, cout, act = 7, 64, 16, R.LEAKY
    shape = (1, TILE_H + 1, TILE_W + 1)
    x, w, b = case(ksize, cin, cout, shape, 9)
    first = run(L, x, w, b, act)
    R.assert_same(first, reference(ksize, cin, cout, act, shape, 9), "alone")
    assert (run(L, x, w, b, act).view(np.uint32) == first.view(np.uint32)).all()
    others = case(ksize, cin, cout, (4,) + shape[1:], 10)[0]
    batch = np.concatenate([others[:2], x, others[2:]])
    assert (run(L, batch, w, b, act)[2:3].view(np.uint32) == first.view(np.uint32)).all()


def test_device_layer(pkg, L):
    """conv2d_device and the numpy conv2d: [B,H,W] for Cin = 1, out and out_offset, the current stream, and the refusals that
    need a device."""
    import torch

    dev = pkg.device
    shape = (2, TILE_H + 1, TILE_W + 1)
    x, w, b = case(3, 1, 16, shape, 11)
    want = reference(3, 1, 16, R.LEAKY, shape, 11)
    t = lambda a: torch.from_numpy(a).to(DEV)
    tx, tw, tb = t(x[..., 0].copy()), t(w), t(b)
    R.assert_same(dev.conv2d_device(tx, tw, tb, "leaky").cpu().numpy(), want, "[B,H,W]")
    out = torch.full(shape + (48,), float("nan"), device=DEV)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        assert dev.conv2d_device(tx, tw, tb, "leaky", out=out, out_offset=32) is out
    s.synchronize()
    got = out.cpu().numpy()
    R.assert_same(got[..., 32:], want, "out_offset on a side stream")
    assert np.isnan(got[..., :32]).all()
    R.assert_same(pkg.conv2d(x, w, b, "leaky"), want, "numpy conv2d")
    for bad in (dict(w=tw[:, :2].contiguous()), dict(w=t(np.zeros((3, 3, 2, 16), F))), dict(bias=tb[:3].contiguous()),
                dict(out=out[:1]), dict(out_offset=16), dict(out=tx)):
        with pytest.raises(ValueError):
            dev.conv2d_device(**dict(dict(x=tx, w=tw, bias=tb), **bad))
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_device(tx, t(np.zeros((2, 2, 1, 16), F)))  # ksize 2: the library's DTFILL_ERR_SHAPE
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_device(tx, tw, tb, out=out, out_offset=40)

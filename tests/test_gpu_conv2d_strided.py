"""dtfill_conv2d_strided and dtfill_conv2d_transpose on the device against the numpy statements of their contracts
(tests/conv2_ref.py), bit for bit (+0 == -0, a NaN matches a NaN), through the ABI on guarded buffers with poisoned outputs."""
import numpy as np
import pytest

import conv2_ref as R2
import conv_ref as R
from guarded import GuardedBuffer
from test_gpu_conv2d import DEV, POISON, _poisoned, _up, case
from test_gpu_conv2d import run as run_conv2d

pytestmark = pytest.mark.gpu

F = np.float32
TILE_H, TILE_W = 8, 32  # the block tile of csrc/dtfill_conv.hpp: output pixels at stride 1, input pixels of the transpose
TILE_H2 = 4  # rows of output pixels at stride 2
WIDTHS = ((16, 16), (32, 48), (16, 80))  # one, three and five N-tiles: a full pass of four and partial last ones
# (B, H, W) in input pixels.  Stride 1 and the transpose: one pixel, 3 x 5, one below, at and one above the tile, two frames
SHAPES_1 = ((1, 1, 1), (1, 3, 5), (2, TILE_H - 1, TILE_W - 1), (1, TILE_H, TILE_W), (2, TILE_H + 1, TILE_W + 1))
# stride 2: the same in output pixels (3 x 31, 4 x 32, 5 x 33), each from an odd and from an even input extent
SHAPES_2 = ((1, 1, 1), (1, 3, 5), (2, 2 * TILE_H2 - 3, 2 * TILE_W - 3), (1, 2 * TILE_H2 - 2, 2 * TILE_W - 2),
            (1, 2 * TILE_H2 - 1, 2 * TILE_W), (1, 2 * TILE_H2, 2 * TILE_W - 1), (2, 2 * TILE_H2 + 1, 2 * TILE_W + 2),
            (1, 2 * TILE_H2 + 2, 2 * TILE_W + 1))


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def out_frame(shape, stride, transposed):
    B, H, W = shape
    return (B, 2 * H, 2 * W) if transposed else (B, -(-H // stride), -(-W // stride))


def run(L, x, w, bias, act, stride=1, residual=None, transposed=False, alpha=0.2, out_channels=None, out_offset=0, x_offset=0,
        out_offset_bytes=0):
    """One call through the ABI on guarded buffers; returns the whole out tensor, poison where the call wrote nothing."""
    import torch

    B, H, W, cin = x.shape
    ksize, cout = w.shape[0], w.shape[3]
    out_channels = cout if out_channels is None else out_channels
    shape = out_frame((B, H, W), stride, transposed) + (out_channels,)
    gx, gw = _up(x, x_offset), _up(w)
    gb = None if bias is None else _up(bias)
    gr = None if residual is None else _up(residual)
    go = _poisoned(shape, out_offset_bytes)
    if transposed:
        rc = L.dtfill_conv2d_transpose(gx.ptr, B, H, W, cin, gw.ptr, gb.ptr if gb else None, cout, act, alpha, go.ptr, out_channels,
                                       out_offset, None)
    else:
        rc = L.dtfill_conv2d_strided(gx.ptr, B, H, W, cin, gw.ptr, gb.ptr if gb else None, ksize, cout, stride,
                                     gr.ptr if gr else None, act, alpha, go.ptr, out_channels, out_offset, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in ((gx, "x"), (gw, "w"), (go, "out"), (gb, "bias"), (gr, "residual")):
        if g is not None:
            g.check(what)
    return go.view(torch.float32, shape).cpu().numpy()


def residual_of(shape, cout, stride, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal(out_frame(shape, stride, False) + (cout,)).astype(F)


def ref(x, w, bias, act, stride=1, residual=None, transposed=False):
    return R2.transpose_ref(x, w, bias, act, 0.2) if transposed else R2.strided_ref(x, w, bias, stride, residual, act, 0.2)


@pytest.mark.parametrize("cin,cout", WIDTHS)
@pytest.mark.parametrize("kind", ("stride 1", "stride 2", "transpose"))
def test_every_width_at_every_tile_seam(L, kind, cin, cout):
    stride, transposed = (2 if kind == "stride 2" else 1), kind == "transpose"
    for n, shape in enumerate(SHAPES_2 if stride == 2 else SHAPES_1):
        x, w, b = case(3, cin, cout, shape, n)
        res = None if transposed or n % 2 else residual_of(shape, cout, stride, n)
        got = run(L, x, w, b, R.LEAKY, stride, res, transposed)
        R.assert_same(got, ref(x, w, b, R.LEAKY, stride, res, transposed), "%s 3x3x%d->%d at %s" % (kind, cin, cout, shape))


@pytest.mark.parametrize("ksize,stride", ((1, 1), (5, 1), (7, 1), (1, 2)))
def test_the_other_kernel_sizes(L, ksize, stride):
    for n, shape in enumerate(((1, 3, 5), (2, TILE_H + 1, TILE_W + 1), (1, 2 * TILE_H2 + 2, 2 * TILE_W - 1))):
        x, w, b = case(ksize, 32, 48, shape, 20 + n)
        res = residual_of(shape, 48, stride, n)
        got = run(L, x, w, b, R.LEAKY, stride, res)
        R.assert_same(got, ref(x, w, b, R.LEAKY, stride, res), "%dx%d stride %d at %s" % (ksize, ksize, stride, shape))


@pytest.mark.parametrize("cin,stride,transposed", ((512, 1, False), (256, 2, False), (512, 1, True)))
def test_deep_chains(L, cin, stride, transposed):
    """ResNet18's longest chains, 32 groups of 16 channels, on a 1 x 3 x 5 frame."""
    x, w, b = case(3, cin, 32, (1, 3, 5), 30)
    R.assert_same(run(L, x, w, b, R.LEAKY, stride, None, transposed), ref(x, w, b, R.LEAKY, stride, None, transposed), "deep chain")


@pytest.mark.parametrize("stride", (1, 2))
def test_residual_with_and_without_bias_and_aliasing_x(L, stride):
    import torch

    shape = (1, TILE_H + 1, TILE_W + 1)
    x, w, b = case(3, 32, 48, shape, 40)
    res = residual_of(shape, 48, stride, 40)
    for bias in (b, None):
        for act in (R.LEAKY, R.LINEAR):
            R.assert_same(run(L, x, w, bias, act, stride, res), ref(x, w, bias, act, stride, res), "residual, bias %s" % (bias is not None))
    # the residual may be x itself (a block's skip tensor is the next layer's input): 3x3x48->48 at stride 1
    x, w, b = case(3, 48, 48, shape, 41)
    gx, gw, go = _up(x), _up(w), _poisoned(x.shape)
    assert L.dtfill_conv2d_strided(gx.ptr, *x.shape, gw.ptr, None, 3, 48, 1, gx.ptr, R.LEAKY, 0.2, go.ptr, 48, 0, None) == 0
    torch.cuda.synchronize()
    R.assert_same(go.view(torch.float32, x.shape).cpu().numpy(), ref(x, w, None, R.LEAKY, 1, x), "residual is x")


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (1, True)))
def test_out_offset_misalignment_and_null_bias(L, stride, transposed):
    shape = (1, TILE_H + 1, TILE_W + 1)
    cin, cout = 32, 48
    x, w, b = case(3, cin, cout, shape, 3)
    res = None if transposed else residual_of(shape, cout, stride, 3)
    want = ref(x, w, b, R.LEAKY, stride, res, transposed)
    # into channels 16 .. 16 + Cout - 1 of a wider tensor: the others keep their poison
    wide = run(L, x, w, b, R.LEAKY, stride, res, transposed, out_channels=80, out_offset=16)
    R.assert_same(wide[..., 16:16 + cout], want, "out_offset")
    rest = np.delete(wide, np.s_[16:16 + cout], axis=-1)
    assert (rest.view(np.uint32) == POISON).all()
    # x and out 4 bytes off a 16-byte boundary
    R.assert_same(run(L, x, w, b, R.LEAKY, stride, res, transposed, x_offset=4, out_offset_bytes=4), want, "misaligned")
    R.assert_same(run(L, x, w, None, R.LEAKY, stride, res, transposed), ref(x, w, None, R.LEAKY, stride, res, transposed), "NULL bias")


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (1, True)))
def test_non_finite_values_follow_fmaf(L, stride, transposed):
    """An inf and a NaN input, and an infinite weight on a corner tap: the pixels whose window holds them are inf or NaN as the
    chain makes them (a padding tap under the infinite weight is +0 * inf = NaN), every other pixel is untouched by them."""
    shape = (1, TILE_H + 1, TILE_W + 1)
    cin = 32
    x, w, b = case(3, cin, 48, shape, 5)
    x[0, 2, 3, 0], x[0, 6, 12, cin - 1] = np.inf, np.nan
    want = ref(x, w, b, R.LEAKY, stride, None, transposed)
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    R.assert_same(run(L, x, w, b, R.LEAKY, stride, None, transposed), want, "inf and NaN inputs")
    # tap (0, 0) is padding at the first output of stride 1 (pt = 1) and of stride 2 on this odd frame; the transpose's
    # padding tap at output (0, 0) is (2, 2)
    corner = (2, 2) if transposed else (0, 0)
    w[corner + (0, 0)] = np.inf
    want = ref(x, w, b, R.LEAKY, stride, None, transposed)
    assert np.isnan(want[0, 0, 0, 0])
    R.assert_same(run(L, x, w, b, R.LEAKY, stride, None, transposed), want, "an infinite weight")


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (1, True)))
def test_bits_do_not_depend_on_the_run_or_the_batch_position(L, stride, transposed):
    shape = (1, TILE_H + 1, TILE_W + 1)
    x, w, b = case(3, 32, 80, shape, 9)
    first = run(L, x, w, b, R.LEAKY, stride, None, transposed)
    R.assert_same(first, ref(x, w, b, R.LEAKY, stride, None, transposed), "alone")
    assert (run(L, x, w, b, R.LEAKY, stride, None, transposed).view(np.uint32) == first.view(np.uint32)).all()
    others = case(3, 32, 80, (4,) + shape[1:], 10)[0]
    batch = np.concatenate([others[:2], x, others[2:]])
    assert (run(L, batch, w, b, R.LEAKY, stride, None, transposed)[2:3].view(np.uint32) == first.view(np.uint32)).all()


@pytest.mark.parametrize("ksize,cin", ((3, 16), (7, 64)))
def test_stride_1_with_16_outputs_is_dtfill_conv2d(L, ksize, cin):
    shape = (2, TILE_H + 1, TILE_W + 1)
    x, w, b = case(ksize, cin, 16, shape, 50)
    got, old = run(L, x, w, b, R.LEAKY), run_conv2d(L, x, w, b, R.LEAKY)
    assert (got.view(np.uint32) == old.view(np.uint32)).all()
    R.assert_same(got, R.conv_ref(x, w, b, R.LEAKY, 0.2), "and both are the statement")


def test_device_layer(pkg):
    """The device functions and the numpy forms: out and out_offset on a side stream, the Keras layout of the transposed
    kernel, and the refusals that need a device."""
    import torch

    dev = pkg.device
    shape = (2, TILE_H + 1, TILE_W + 1)
    x, w, b = case(3, 32, 48, shape, 11)
    res = residual_of(shape, 48, 2, 11)
    want = ref(x, w, b, R.LEAKY, 2, res)
    t = lambda a: torch.from_numpy(a).to(DEV)
    tx, tw, tb, tr = t(x), t(w), t(b), t(res)
    R.assert_same(dev.conv2d_strided_device(tx, tw, tb, 2, tr, "leaky").cpu().numpy(), want, "new out")
    out = torch.full(want.shape[:3] + (80,), float("nan"), device=DEV)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        assert dev.conv2d_strided_device(tx, tw, tb, 2, tr, "leaky", out=out, out_offset=32) is out
    s.synchronize()
    got = out.cpu().numpy()
    R.assert_same(got[..., 32:], want, "out_offset on a side stream")
    assert np.isnan(got[..., :32]).all()
    R.assert_same(pkg.conv2d_strided(x, w, b, 2, res, "leaky"), want, "numpy conv2d_strided")
    kernel = np.ascontiguousarray(w.transpose(0, 1, 3, 2))  # Keras's [3,3,Cout,Cin] of the packed w
    want_t = ref(x, w, b, R.LEAKY, transposed=True)
    R.assert_same(pkg.conv2d_transpose(x, kernel, b, "leaky"), want_t, "numpy conv2d_transpose")
    wide = torch.full(want_t.shape[:3] + (64,), float("nan"), device=DEV)
    with torch.cuda.stream(s):
        assert dev.conv2d_transpose_device(tx, tw, tb, "leaky", out=wide, out_offset=16) is wide
    s.synchronize()
    R.assert_same(wide.cpu().numpy()[..., 16:], want_t, "transpose, out_offset on a side stream")
    good = dict(x=tx, w=tw, bias=tb, stride=2, residual=tr)
    for bad in (dict(w=tw[:, :2].contiguous()), dict(w=t(np.zeros((3, 3, 16, 48), F))), dict(bias=tb[:3].contiguous()),
                dict(out=out[:1]), dict(out_offset=16), dict(out=tx), dict(residual=tr[:, :2].contiguous()), dict(stride=1),
                dict(out=tr), dict(out=torch.empty(shape + (48,), device=DEV))):
        with pytest.raises(ValueError):
            dev.conv2d_strided_device(**dict(good, **bad))
    for bad in (dict(w_packed=t(np.zeros((5, 5, 32, 48), F))), dict(out=wide[:, :4].contiguous()), dict(out_offset=16)):
        with pytest.raises(ValueError):
            dev.conv2d_transpose_device(**dict(dict(x=tx, w_packed=tw, bias=tb), **bad))
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_strided_device(tx, t(np.zeros((2, 2, 32, 48), F)))  # ksize 2: the library's DTFILL_ERR_SHAPE
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_strided_device(tx, t(np.zeros((5, 5, 32, 48), F)), stride=2)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_strided_device(tx, tw, tb, 2, out=out, out_offset=40)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_transpose_device(tx, t(np.zeros((3, 3, 32, 8), F)))  # Cout 8

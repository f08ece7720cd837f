"""dtfill_conv2d_image and dtfill_conv2d_image_backward_weights on the device against the numpy statements of their contracts
(tests/conv_ref.py, tests/convb_ref.py, which hold for any Cin and Cout), bit for bit (+0 == -0, a NaN matches a NaN), through
the ABI on guarded buffers with poisoned outputs and a poisoned workspace, in the manner of test_gpu_conv2d.py and
test_gpu_conv2d_backward.py, whose helpers these are."""
import numpy as np
import pytest

import conv_ref as R
import convb_ref as RB
import test_gpu_conv2d as fwd
import test_gpu_conv2d_backward as bwd
from guarded import GuardedBuffer

pytestmark = pytest.mark.gpu

DEV = fwd.DEV
F = np.float32
POISON = fwd.POISON
SHAPES = fwd.SHAPES  # (1,1,1), (1,3,5), (2,7,15), (1,8,16), (1,9,17), (1,7,31), (1,8,32), (2,9,33): every seam of the 8 x 32 tile
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
# one pixel; smaller than the 7x7 window with a k-step of one pixel; a partial strip; a k-step of four and of one pixel beside
# whole ones; one below, at and one above the segment, the last with four segments a frame
BW_SHAPES = ((1, 1, 1), (1, 3, 5), (1, 4, 7), (1, 5, 8), (2, ROWS - 1, COLS - 1), (1, ROWS, COLS), (1, ROWS + 1, COLS + 1))
BW_LAYERS = ((3, 3, 64), (1, 2, 16), (7, 2, 16), (1, 4, 16), (7, 4, 16))  # (ksize, Cin, Cout)
WIDE, AT = 96, 16  # dy and y of the backward: channels AT .. AT + Cout - 1 of a tensor WIDE wide
MAX_BLOCKS = 1 << 20  # CV_MAX_BLOCKS of csrc/dtfill_conv.hpp


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def run(L, x, w, bias, act, alpha=0.2, out_channels=None, out_offset=0, x_offset=0, out_offset_bytes=0, stream=None):
    """One call of dtfill_conv2d_image on guarded buffers; returns the whole out tensor, poison where the call wrote nothing."""
    import torch

    B, H, W, cin = x.shape
    ksize, cout = w.shape[0], w.shape[3]
    out_channels = cout if out_channels is None else out_channels
    gx, gw = fwd._up(x, x_offset), fwd._up(w)
    gb = None if bias is None else fwd._up(bias)
    go = fwd._poisoned((B, H, W, out_channels), out_offset_bytes)
    rc = L.dtfill_conv2d_image(gx.ptr, B, H, W, cin, gw.ptr, gb.ptr if gb else None, ksize, cout, act, alpha, go.ptr, out_channels,
                               out_offset, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in ((gx, "x"), (gw, "w"), (go, "out")) + (((gb, "bias"),) if gb else ()):
        g.check(what)
    return go.view(torch.float32, (B, H, W, out_channels)).cpu().numpy()


_reference = {}


def reference(ksize, cin, cout, act, shape, seed, bias=True):
    """conv_ref of fwd.case(), worked out once per case and shared."""
    key = (ksize, cin, cout, act, shape, seed, bias)
    if key not in _reference:
        x, w, b = fwd.case(ksize, cin, cout, shape, seed)
        _reference[key] = R.conv_ref(x, w, b if bias else None, act, 0.2)
    return _reference[key]


@pytest.mark.parametrize("cout", (16, 64, 80))  # one N-tile, a whole pass, the pass seam (a second pass of one tile)
@pytest.mark.parametrize("ksize", (1, 3, 5, 7))
@pytest.mark.parametrize("cin", (2, 3, 4))
def test_forward_at_every_tile_seam(L, cin, ksize, cout):
    act = R.LEAKY if (cin + ksize) % 2 else R.LINEAR
    for n, shape in enumerate(SHAPES):
        x, w, b = fwd.case(ksize, cin, cout, shape, n)
        R.assert_same(run(L, x, w, b, act), reference(ksize, cin, cout, act, shape, n), "%dx%dx%d->%d at %s" % (ksize, ksize, cin, cout, shape))


@pytest.mark.parametrize("ksize,cin,cout", ((3, 3, 64), (7, 4, 16), (5, 2, 80)))
def test_out_offset_misalignment_and_null_bias(L, ksize, cin, cout):
    shape, act = (1, 9, 17), R.LEAKY
    x, w, b = fwd.case(ksize, cin, cout, shape, 3)
    want = reference(ksize, cin, cout, act, shape, 3)
    wide = run(L, x, w, b, act, out_channels=cout + 40, out_offset=24)  # the others keep their poison
    R.assert_same(wide[..., 24:24 + cout], want, "out_offset")
    assert (np.delete(wide, np.s_[24:24 + cout], axis=-1).view(np.uint32) == POISON).all()
    R.assert_same(run(L, x, w, b, act, x_offset=4, out_offset_bytes=4), want, "x and out 4 bytes off a 16-byte boundary")
    R.assert_same(run(L, x, w, None, act), reference(ksize, cin, cout, act, shape, 3, bias=False), "NULL bias")


@pytest.mark.parametrize("ksize,cin,cout", ((3, 3, 64), (7, 2, 16), (1, 3, 16)))
def test_non_finite_values_follow_fmaf(L, ksize, cin, cout):
    """An inf and a NaN input; an infinite weight over a padding tap makes NaN (+0 * inf); and an infinite input makes no NaN
    through the links that pad the chain's last k-step: both of their operands are +0, the x operand is not read."""
    shape, act = (1, 9, 17), R.LEAKY
    x, w, b = fwd.case(ksize, cin, cout, shape, 5)
    x[0, 2, 3, 0], x[0, 6, 12, cin - 1] = np.inf, np.nan
    want = R.conv_ref(x, w, b, act, 0.2)
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    R.assert_same(run(L, x, w, b, act), want, "inf and NaN inputs")
    if ksize > 1:
        w[0, 0, 0, 0] = np.inf
        want = R.conv_ref(x, w, b, act, 0.2)
        assert np.isnan(want[0, 0, 0, 0])  # the corner's tap (0, 0) is padding
        R.assert_same(run(L, x, w, b, act), want, "an infinite weight")
    # every input +inf under positive weights: +inf everywhere by the statement, NaN nowhere (K = ksize^2 Cin is 27, 98 or 3 here:
    # the last step has 1, 2 or 1 padding links)
    x = np.full(shape + (cin,), np.inf, F)
    w = np.abs(w)
    w[~np.isfinite(w)] = 1
    w[w == 0] = 1
    got = run(L, x, w, None, R.LINEAR)
    assert (ksize * ksize * cin) % 4 != 0 and not np.isnan(got[0, 4, 8]).any() and (got[0, 4, 8] == np.inf).all()


def test_bits_do_not_depend_on_the_run_or_the_batch_position(L):
    ksize, cin, cout, act = 3, 3, 64, R.LEAKY
    shape = (1, 9, 33)
    x, w, b = fwd.case(ksize, cin, cout, shape, 9)
    first = run(L, x, w, b, act)
    R.assert_same(first, reference(ksize, cin, cout, act, shape, 9), "alone")
    assert (run(L, x, w, b, act).view(np.uint32) == first.view(np.uint32)).all()
    others = fwd.case(ksize, cin, cout, (4,) + shape[1:], 10)[0]
    batch = np.concatenate([others[:2], x, others[2:]])
    assert (run(L, batch, w, b, act)[2:3].view(np.uint32) == first.view(np.uint32)).all()


def test_a_block_takes_a_second_work_item(L):
    """2^20 + 3 frames of 1 x 1, one work item each, past CV_MAX_BLOCKS: four distinct frames repeated, every frame's bits
    compared on the device with those of its first occurrence, which are held to conv_ref."""
    import torch

    ksize, cin, cout, B = 3, 3, 16, MAX_BLOCKS + 3
    four, w, b = fwd.case(ksize, cin, cout, (4, 1, 1), 12)
    tx = torch.from_numpy(four).to(DEV).repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    tw, tb = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    out = torch.full((B, 1, 1, cout), float("nan"), device=DEV)
    rc = L.dtfill_conv2d_image(tx.data_ptr(), B, 1, 1, cin, tw.data_ptr(), tb.data_ptr(), ksize, cout, R.LEAKY, 0.2, out.data_ptr(),
                               cout, 0, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    R.assert_same(out[:4].cpu().numpy(), R.conv_ref(four, w, b, R.LEAKY, 0.2), "the first four")
    bits = out.view(torch.int32)
    assert bool((bits == bits[:4].repeat((B + 3) // 4, 1, 1, 1)[:B]).all())


# ---- the weight gradient ------------------------------------------------------------------------------------------------


def bw_case(ksize, cin, cout, shape, seed):
    x, _, _ = fwd.case(ksize, cin, cout, shape, seed)
    dy, _, _ = fwd.case(ksize, cout, cout, shape, seed + 1000)
    y, _, _ = fwd.case(ksize, cout, cout, shape, seed + 2000)
    y[np.random.default_rng(seed).random(y.shape) < 0.05] = -0.0
    return x, dy, y


def _wide(a):
    out = np.full(a.shape[:3] + (WIDE,), POISON, np.uint32).view(F)
    out[..., AT:AT + a.shape[3]] = a
    return out


def run_weights(L, x, dy, y, ksize, act, alpha=0.2, want_db=True, mis=0, wide=True, ws_fill=0xFF, stream=None):
    """dtfill_conv2d_image_backward_weights on guarded buffers; returns (dw, db or None).  wide: dy and y are the channels AT ..
    of tensors WIDE wide whose other channels hold poison that must survive."""
    import torch

    B, H, W, cin = x.shape
    cout = dy.shape[3]
    wdy, wy = (_wide(dy), _wide(y)) if wide else (dy, y)
    width, at = (WIDE, AT) if wide else (cout, 0)
    gx, gdy, gy = fwd._up(x, mis), fwd._up(wdy, mis), fwd._up(wy)
    gdw = fwd._poisoned((ksize, ksize, cin, cout))
    gdb = fwd._poisoned((cout,)) if want_db else None
    nbytes = L.dtfill_conv2d_image_backward_workspace_bytes(B, H, W, cin, ksize, cout)
    assert nbytes > 0
    ws = GuardedBuffer(nbytes, 0, DEV)
    ws.payload().fill_(ws_fill)
    rc = L.dtfill_conv2d_image_backward_weights(gx.ptr, gdy.ptr, width, at, gy.ptr if act == R.LEAKY else None, width, at, B, H, W, cin,
                                                ksize, cout, act, alpha, gdw.ptr, gdb.ptr if gdb else None, ws.ptr, nbytes, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bwd._unchanged(gx, x, "x")
    bwd._unchanged(gdy, wdy, "dy")
    bwd._unchanged(gy, wy, "y")
    gdw.check("dw")
    ws.check("workspace")
    if gdb:
        gdb.check("db")
    return (gdw.view(torch.float32, (ksize, ksize, cin, cout)).cpu().numpy(),
            gdb.view(torch.float32, (cout,)).cpu().numpy() if gdb else None)


_bw_reference = {}


def bw_reference(ksize, cin, cout, act, shape, seed):
    key = (ksize, cin, cout, act, shape, seed)
    if key not in _bw_reference:
        x, dy, y = bw_case(ksize, cin, cout, shape, seed)
        _bw_reference[key] = RB.dw_ref(x, dy, y, ksize, act)
    return _bw_reference[key]


@pytest.mark.parametrize("ksize,cin,cout", BW_LAYERS)
def test_weight_gradient_at_every_segment_seam(L, ksize, cin, cout):
    act = R.LEAKY
    for n, shape in enumerate(BW_SHAPES):
        what = "%dx%dx%d->%d at %s" % (ksize, ksize, cin, cout, shape)
        x, dy, y = bw_case(ksize, cin, cout, shape, n)
        dw, db = bw_reference(ksize, cin, cout, act, shape, n)
        got_dw, got_db = run_weights(L, x, dy, y, ksize, act)  # dy and y at an offset of a wider tensor
        R.assert_same(got_dw, dw, "dw of " + what)
        R.assert_same(got_db, db, "db of " + what)


def test_weight_gradient_buffer_rules(L):
    """Linear with y NULL, db NULL, dense dy and y, 4 bytes off a 16-byte boundary, two differently poisoned workspaces, a
    stream."""
    import torch

    ksize, cin, cout, shape = 3, 3, 64, (1, 5, 8)
    x, dy, y = bw_case(ksize, cin, cout, shape, 3)
    dw, db = bw_reference(ksize, cin, cout, R.LEAKY, shape, 3)
    lin_dw, lin_db = RB.dw_ref(x, dy, None, ksize, R.LINEAR)
    got_dw, got_db = run_weights(L, x, dy, y, ksize, R.LINEAR)  # (run_weights passes a NULL y for a linear layer)
    R.assert_same(got_dw, lin_dw, "linear dw")
    R.assert_same(got_db, lin_db, "linear db")
    got_dw, none = run_weights(L, x, dy, y, ksize, R.LEAKY, want_db=False)
    assert none is None
    R.assert_same(got_dw, dw, "NULL db")
    for kw, what in ((dict(wide=False), "dense"), (dict(mis=4), "misaligned"), (dict(ws_fill=0x00), "a zeroed workspace"),
                     (dict(ws_fill=0x7F), "another poison")):
        got_dw, got_db = run_weights(L, x, dy, y, ksize, R.LEAKY, **kw)
        R.assert_same(got_dw, dw, "dw, " + what)
        R.assert_same(got_db, db, "db, " + what)
    s = torch.cuda.Stream(device=DEV)
    got_dw, got_db = run_weights(L, x, dy, y, ksize, R.LEAKY, stream=s.cuda_stream)
    R.assert_same(got_dw, dw, "dw on a stream")
    R.assert_same(got_db, db, "db on a stream")


def test_device_layer_and_autograd(pkg, L):
    """conv2d_image_device, the numpy conv2d_image, conv2d_image_backward_weights_device and autograd.conv2d_image: the bits of
    the ABI calls, a gradient read in place out of torch.cat's wider tensor, and an x that requires a gradient refused."""
    import torch

    dev = pkg.device
    ksize, cin, cout, shape = 3, 3, 64, (1, 5, 8)
    x, w, b = fwd.case(ksize, cin, cout, shape, 3)
    _, dy, _ = bw_case(ksize, cin, cout, shape, 3)
    want = reference(ksize, cin, cout, R.LEAKY, shape, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tx, tw, tb = t(x), t(w), t(b)
    R.assert_same(dev.conv2d_image_device(tx, tw, tb, "leaky").cpu().numpy(), want, "conv2d_image_device")
    out = torch.full(shape + (96,), float("nan"), device=DEV)
    assert dev.conv2d_image_device(tx, tw, tb, "leaky", out=out, out_offset=32) is out
    got = out.cpu().numpy()
    R.assert_same(got[..., 32:], want, "out_offset")
    assert np.isnan(got[..., :32]).all()
    R.assert_same(pkg.conv2d_image(x, w, b, "leaky"), want, "numpy conv2d_image")
    dw, db = RB.dw_ref(x, dy, want, ksize, R.LEAKY)
    got_dw, got_db = dev.conv2d_image_backward_weights_device(tx, t(_wide(dy)), ksize, t(_wide(want)), "leaky", 0.2, AT, AT, cout)
    R.assert_same(got_dw.cpu().numpy(), dw, "dw")
    R.assert_same(got_db.cpu().numpy(), db, "db")
    assert dev.conv2d_image_backward_workspace_bytes(*shape, cin, ksize, cout) == L.dtfill_conv2d_image_backward_workspace_bytes(*shape, cin, ksize, cout)
    # under the tape, the output concatenated behind 16 other channels: dy arrives as a slice of the 80-wide gradient
    pw, pb = tw.clone().requires_grad_(), tb.clone().requires_grad_()
    y = pkg.autograd.conv2d_image(tx, pw, pb, "leaky")
    R.assert_same(y.detach().cpu().numpy(), want, "autograd forward")
    other = torch.zeros(shape + (16,), device=DEV, requires_grad=True)
    upstream = torch.cat([torch.zeros(shape + (16,), device=DEV), t(dy)], dim=3)
    torch.cat([other, y], dim=3).backward(upstream)
    R.assert_same(pw.grad.cpu().numpy(), dw, "autograd dw")
    R.assert_same(pb.grad.cpu().numpy(), db, "autograd db")
    with pytest.raises(ValueError, match="image is data"):
        pkg.autograd.conv2d_image(tx.clone().requires_grad_(), pw, pb, "leaky")
    for bad in (dict(w=t(np.zeros((3, 3, 2, 64), F))), dict(bias=tb[:3].contiguous()), dict(out=out[:, :1].contiguous()), dict(out_offset=16)):
        with pytest.raises(ValueError):
            dev.conv2d_image_device(**dict(dict(x=tx, w=tw, bias=tb), **bad))
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_image_device(tx, t(np.zeros((3, 3, 3, 24), F)))  # Cout 24: the library's DTFILL_ERR_SHAPE
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_image_backward_workspace_bytes(1, 5, 8, 16, 3, 64)

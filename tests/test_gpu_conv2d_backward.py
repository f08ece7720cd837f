"""dtfill_conv2d_backward_data and dtfill_conv2d_backward_weights on the device against the numpy statement of their contracts
(tests/convb_ref.py), bit for bit (+0 == -0, a NaN matches a NaN), through the ABI on guarded buffers with poisoned outputs and
a poisoned workspace.  dy and y are read out of wider tensors whose other channels hold a NaN poison that must survive."""
import numpy as np
import pytest

import conv_ref as R
import convb_ref as RB
import test_gpu_conv2d as fwd
from guarded import GuardedBuffer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
POISON = fwd.POISON
WIDE, AT = 40, 16  # dy and y: channels AT .. AT + Cout - 1 of a tensor WIDE wide
# (B, H, W): one pixel; smaller than the 7x7 window and with a k-step of one pixel; one below, at and one above the segment,
# the last with four segments a frame and two frames; the forward's tile seams (the input gradient runs on its kernels)
SHAPES = ((1, 1, 1), (1, 3, 5), (2, ROWS - 1, COLS - 1), (1, ROWS, COLS), (2, ROWS + 1, COLS + 1), (1, 8, 32), (2, 9, 33))
LAYERS = R.NET_LAYERS
EDGE = (1, 9, 17)  # the shape of the tests of the buffer rules: a partial strip, a k-step of one pixel


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def case(ksize, cin, cout, shape, seed):
    """x, w as test_gpu_conv2d.case's; dy and y of its kind too: mixed binades, a third of them zero, y with a few -0."""
    x, w, _ = fwd.case(ksize, cin, cout, shape, seed)
    dy, _, _ = fwd.case(ksize, cout, cout, shape, seed + 1000)
    y, _, _ = fwd.case(ksize, cout, cout, shape, seed + 2000)
    y[np.random.default_rng(seed).random(y.shape) < 0.05] = -0.0
    return x, w, dy, y


def _wide(a):
    """a [B,H,W,C] as the channels AT .. AT + C - 1 of a [B,H,W,WIDE] tensor of poison."""
    out = np.full(a.shape[:3] + (WIDE,), POISON, np.uint32).view(F)
    out[..., AT:AT + a.shape[3]] = a
    return out


def _workspace(L, shape, cin, ksize, cout):
    import torch

    nbytes = L.dtfill_conv2d_backward_workspace_bytes(*shape, cin, ksize, cout)
    assert nbytes > 0
    g = GuardedBuffer(nbytes, 0, DEV)
    g.payload().fill_(0xFF)  # NaNs
    return g, nbytes


def _unchanged(g, a, what):
    import torch

    g.check(what)
    assert (g.payload().cpu().numpy().view(np.uint32) == np.ascontiguousarray(a).reshape(-1).view(np.uint32)).all(), what + " was written"


def run_data(L, dy, y, w, act, alpha=0.2, dx_channels=None, dx_offset=0, mis=0):
    """dtfill_conv2d_backward_data on guarded buffers; returns the whole dx tensor [B,H,W,dx_channels]."""
    import torch

    B, H, W, cout = dy.shape
    ksize, cin = w.shape[0], w.shape[2]
    dx_channels = cin if dx_channels is None else dx_channels
    wdy, wy = _wide(dy), _wide(y)
    gdy, gy, gw = fwd._up(wdy, mis), fwd._up(wy), fwd._up(w)
    gdx = fwd._poisoned((B, H, W, dx_channels), mis)
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout)
    rc = L.dtfill_conv2d_backward_data(gdy.ptr, WIDE, AT, gy.ptr if act == R.LEAKY else None, WIDE, AT, gw.ptr, B, H, W, cin, ksize,
                                       cout, act, alpha, gdx.ptr, dx_channels, dx_offset, ws.ptr, nbytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _unchanged(gdy, wdy, "dy")
    _unchanged(gy, wy, "y")
    _unchanged(gw, w, "w")
    gdx.check("dx")
    ws.check("workspace")
    return gdx.view(torch.float32, (B, H, W, dx_channels)).cpu().numpy()


def run_weights(L, x, dy, y, ksize, act, alpha=0.2, want_db=True, mis=0):
    """dtfill_conv2d_backward_weights on guarded buffers; returns (dw, db or None)."""
    import torch

    B, H, W, cin = x.shape
    cout = dy.shape[3]
    wdy, wy = _wide(dy), _wide(y)
    gx, gdy, gy = fwd._up(x, mis), fwd._up(wdy, mis), fwd._up(wy)
    gdw = fwd._poisoned((ksize, ksize, cin, cout))
    gdb = fwd._poisoned((cout,)) if want_db else None
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout)
    rc = L.dtfill_conv2d_backward_weights(gx.ptr, gdy.ptr, WIDE, AT, gy.ptr if act == R.LEAKY else None, WIDE, AT, B, H, W, cin,
                                          ksize, cout, act, alpha, gdw.ptr, gdb.ptr if gdb else None, ws.ptr, nbytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _unchanged(gx, x, "x")
    _unchanged(gdy, wdy, "dy")
    _unchanged(gy, wy, "y")
    gdw.check("dw")
    ws.check("workspace")
    if gdb:
        gdb.check("db")
    return (gdw.view(torch.float32, (ksize, ksize, cin, cout)).cpu().numpy(),
            gdb.view(torch.float32, (cout,)).cpu().numpy() if gdb else None)


_reference = {}


def reference(ksize, cin, cout, act, shape, seed):
    """(dx, dw, db) of case() by convb_ref, worked out once per case and shared."""
    key = (ksize, cin, cout, act, shape, seed)
    if key not in _reference:
        x, w, dy, y = case(ksize, cin, cout, shape, seed)
        _reference[key] = (RB.dx_ref(dy, y, w, act),) + RB.dw_ref(x, dy, y, ksize, act)
    return _reference[key]


@pytest.mark.parametrize("ksize,cin,cout,act", LAYERS)
def test_every_layer_at_every_segment_seam(L, ksize, cin, cout, act):
    for n, shape in enumerate(SHAPES):
        what = "%dx%dx%d->%d at %s" % (ksize, ksize, cin, cout, shape)
        x, w, dy, y = case(ksize, cin, cout, shape, n)
        dx, dw, db = reference(ksize, cin, cout, act, shape, n)
        R.assert_same(run_data(L, dy, y, w, act), dx, "dx of " + what)
        got_dw, got_db = run_weights(L, x, dy, y, ksize, act)
        R.assert_same(got_dw, dw, "dw of " + what)
        R.assert_same(got_db, db, "db of " + what)


@pytest.mark.parametrize("ksize,cin,cout,act", ((1, 16, 16, R.LEAKY), (5, 1, 16, R.LINEAR), (1, 1, 16, R.LEAKY), (3, 32, 1, R.LEAKY),
                                                (5, 64, 1, R.LINEAR), (1, 1, 1, R.LEAKY), (3, 1, 1, R.LINEAR)))
def test_the_domain_beyond_the_net(L, ksize, cin, cout, act):
    """Shapes of dtfill_conv2d's domain that no layer of the net has: a 1x1 kernel on the matrix cores, 25 taps of one channel
    (db's row of ones in the second tile), one output channel under many input channels (dx: one launch per 16 of them)."""
    for n, shape in enumerate((EDGE, (2, ROWS + 1, COLS + 1))):
        x, w, dy, y = case(ksize, cin, cout, shape, 20 + n)
        dx, dw, db = reference(ksize, cin, cout, act, shape, 20 + n)
        R.assert_same(run_data(L, dy, y, w, act), dx, "dx")
        got_dw, got_db = run_weights(L, x, dy, y, ksize, act)
        R.assert_same(got_dw, dw, "dw")
        R.assert_same(got_db, db, "db")


@pytest.mark.parametrize("ksize,cin,cout,act", ((7, 64, 16, R.LEAKY), (5, 16, 16, R.LEAKY), (3, 1, 16, R.LEAKY), (3, 16, 1, R.LINEAR)))
def test_dx_offset_misalignment_and_null_db(L, ksize, cin, cout, act):
    x, w, dy, y = case(ksize, cin, cout, EDGE, 3)
    dx, dw, db = reference(ksize, cin, cout, act, EDGE, 3)
    # into channels 8 .. 8 + Cin - 1 of a wider tensor: the others keep their poison
    wide = run_data(L, dy, y, w, act, dx_channels=cin + 24, dx_offset=8)
    R.assert_same(wide[..., 8:8 + cin], dx, "dx_offset")
    assert (np.delete(wide, np.s_[8:8 + cin], axis=-1).view(np.uint32) == POISON).all()
    # x, dy and dx 4 bytes off a 16-byte boundary
    R.assert_same(run_data(L, dy, y, w, act, mis=4), dx, "misaligned dx")
    got_dw, got_db = run_weights(L, x, dy, y, ksize, act, mis=4)
    R.assert_same(got_dw, dw, "misaligned dw")
    R.assert_same(got_db, db, "misaligned db")
    got_dw, none = run_weights(L, x, dy, y, ksize, act, want_db=False)
    assert none is None
    R.assert_same(got_dw, dw, "NULL db")


@pytest.mark.parametrize("ksize,cin,cout,act", ((7, 32, 16, R.LEAKY), (7, 1, 16, R.LEAKY), (3, 16, 1, R.LINEAR)))
def test_non_finite_values_follow_fmaf(L, ksize, cin, cout, act):
    """An inf and a NaN in x, dy and y.  A NaN y takes the alpha branch; an infinite x at the frame's right edge lies under a
    tap of the pixels beyond the edge that pad the row's last k-step, and must not reach dw: those pixels are no links."""
    x, w, dy, y = case(ksize, cin, cout, EDGE, 5)
    x[0, 2, 3, 0], x[0, 6, 12, cin - 1], x[0, 4, EDGE[2] - 1, 0] = np.inf, np.nan, np.inf
    dy[0, 1, 2, 0], dy[0, 7, 9, cout - 1] = np.nan, -np.inf
    y[0, 3, 3, 0], y[0, 5, 5, cout - 1] = np.nan, np.inf
    dy[0, 3, 3, 0] = 1.5
    dx, (dw, db) = RB.dx_ref(dy, y, w, act), RB.dw_ref(x, dy, y, ksize, act)
    assert np.isnan(dx).any() and np.isfinite(dx).any() and np.isnan(dw).any() and np.isnan(db).any()
    R.assert_same(run_data(L, dy, y, w, act), dx, "dx")
    got_dw, got_db = run_weights(L, x, dy, y, ksize, act)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")
    # x alone non-finite: every gradient of g stays finite, and dw is NaN or inf only under the taps that meet those pixels
    x, w, dy, y = case(ksize, cin, cout, EDGE, 6)
    x[0, 4, EDGE[2] - 1, 0] = np.inf
    dw, db = RB.dw_ref(x, dy, y, ksize, act)
    assert np.isfinite(db).all() and np.isfinite(dw[..., 1:, :]).all() and not np.isfinite(dw[..., 0, :]).all()
    assert np.isfinite(dw[:, (ksize - 1) // 2 - 1, 0]).all()  # the tap that reads the edge column only from the pixel beyond it
    got_dw, got_db = run_weights(L, x, dy, y, ksize, act)
    R.assert_same(got_dw, dw, "dw under an infinite x at the right edge")
    R.assert_same(got_db, db, "db under an infinite x")


def test_bits_do_not_depend_on_the_run(L):
    ksize, cin, cout, act = 7, 64, 16, R.LEAKY
    shape = (2, 9, 33)
    x, w, dy, y = case(ksize, cin, cout, shape, 6)
    first_dx = run_data(L, dy, y, w, act)
    first_dw, first_db = run_weights(L, x, dy, y, ksize, act)
    assert (run_data(L, dy, y, w, act).view(np.uint32) == first_dx.view(np.uint32)).all()
    dw, db = run_weights(L, x, dy, y, ksize, act)
    assert (dw.view(np.uint32) == first_dw.view(np.uint32)).all() and (db.view(np.uint32) == first_db.view(np.uint32)).all()


@pytest.mark.parametrize("ksize,cin,cout,act", LAYERS)
def test_dx_is_the_forward_on_g_and_the_flipped_kernel(L, ksize, cin, cout, act):
    """dx against dtfill_conv2d on the device (dtfill_conv2d_strided for Cin of 32, 48 and 64) on a materialised g and a
    host-repacked wT."""
    import torch

    shape = (2, 9, 33)
    x, w, dy, y = case(ksize, cin, cout, shape, 6)
    g, wt = RB.g_ref(dy, y, act), RB.flipped(w)
    if cin <= 16:
        want = fwd.run(L, g, wt, None, R.LINEAR)
    else:
        gg, gw, go = fwd._up(g), fwd._up(wt), fwd._poisoned(shape + (cin,))
        assert L.dtfill_conv2d_strided(gg.ptr, *shape, cout, gw.ptr, None, ksize, cin, 1, None, R.LINEAR, 0.0, go.ptr, cin, 0, None) == 0
        torch.cuda.synchronize()
        want = go.view(torch.float32, shape + (cin,)).cpu().numpy()
    R.assert_same(run_data(L, dy, y, w, act), want, "dx")


def test_device_layer(pkg, L):
    """conv2d_backward_data_device and conv2d_backward_weights_device: slices of wider tensors, [B,H,W] for one channel, a side
    stream, and the refusals."""
    import torch

    dev = pkg.device
    shape = (2, 9, 33)
    x, w, dy, y = case(3, 1, 16, shape, 11)
    dx, dw, db = reference(3, 1, 16, R.LEAKY, shape, 11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tx, tw, tdy, ty = t(x[..., 0]), t(w), t(_wide(dy)), t(_wide(y))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = dev.conv2d_backward_data_device(tdy, tw, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT)
        got_dw, got_db = dev.conv2d_backward_weights_device(tx, tdy, 3, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, cout=16)
    s.synchronize()
    R.assert_same(got.cpu().numpy(), dx, "dx on a side stream")
    R.assert_same(got_dw.cpu().numpy(), dw, "dw")
    R.assert_same(got_db.cpu().numpy(), db, "db")
    assert dev.conv2d_backward_weights_device(tx, t(dy), 3, t(y), "leaky", want_bias=False)[1] is None
    assert dev.conv2d_backward_workspace_bytes(2, 9, 33, 1, 3, 16) == L.dtfill_conv2d_backward_workspace_bytes(2, 9, 33, 1, 3, 16)
    for bad in (dict(y=None), dict(alpha=-0.1), dict(act="relu"), dict(dy_offset=30), dict(y=ty[:1].contiguous()),
                dict(w=tw[:, :2].contiguous()), dict(dx=tdy)):
        with pytest.raises(ValueError):
            dev.conv2d_backward_data_device(**dict(dict(dy=tdy, w=tw, y=ty, act="leaky", dy_offset=AT, y_offset=AT), **bad))
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_backward_data_device(t(dy), t(np.zeros((2, 2, 1, 16), F)), t(y), "leaky")  # ksize 2
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_backward_workspace_bytes(2, 9, 33, 8, 3, 16)

"""dtfill_conv2d_strided_backward_data / _weights and dtfill_conv2d_transpose_backward_data / _weights on the device against the
numpy statement of their contracts (tests/conv2b_ref.py), bit for bit (+0 == -0, a NaN matches a NaN), through the ABI on
guarded buffers with poisoned outputs and a poisoned workspace.  dy and y are read out of wider tensors whose other channels
hold a NaN poison that must survive.

The shapes are the smallest that cross every seam the kernels have: an output frame of 33 x 65 is 2 x 2 segments, both cut, whose
last k-step ends inside the frame (the transposed layer: that input frame); B = 2 for level 2's frame order; Cin 16 and 48, one
and several groups; Cout 16 and 80, one tile and one more than a pass of four; ksize 1 and 3 at both strides."""
import numpy as np
import pytest

import conv2b_ref as RW
import conv_ref as R
import test_gpu_conv2d as fwd
import test_gpu_conv2d_backward as bwd
from guarded import GuardedBuffer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
POISON = fwd.POISON
WIDE, AT = 112, 16  # dy and y: channels AT .. AT + Cout - 1 of a tensor WIDE wide
FRAME = (2, 33, 65)  # the frame the segments lie over
STRIDED = [(ksize, stride, cin, cout, act) for ksize in (1, 3) for stride in (1, 2) for cin, cout, act in
           ((16, 16, R.LEAKY), (48, 80, R.LEAKY), (16, 80, R.LINEAR), (48, 16, R.LINEAR))] + [(7, 1, 16, 32, R.LEAKY), (5, 1, 32, 16, R.LEAKY)]
TRANSPOSED = ((16, 16, R.LEAKY), (48, 80, R.LEAKY), (16, 80, R.LINEAR), (48, 16, R.LINEAR))


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def out_frame(ksize):
    return (2, 9, 33) if ksize > 3 else FRAME


def strided_case(ksize, stride, cin, cout, seed, frame=None):
    """x [B,stride Ho,stride Wo,Cin], w, dy and y [B,Ho,Wo,Cout] of test_gpu_conv2d.case's kind; y with a few -0."""
    B, Ho, Wo = frame or out_frame(ksize)
    x, w, _ = fwd.case(ksize, cin, cout, (B, stride * Ho, stride * Wo), seed)
    dy, _, _ = fwd.case(1, cout, cout, (B, Ho, Wo), seed + 1000)
    y, _, _ = fwd.case(1, cout, cout, (B, Ho, Wo), seed + 2000)
    y[np.random.default_rng(seed).random(y.shape) < 0.05] = -0.0
    return x, w, dy, y


def transposed_case(cin, cout, seed, frame=FRAME):
    B, H, W = frame
    x, w, _ = fwd.case(3, cin, cout, (B, H, W), seed)
    dy, _, _ = fwd.case(1, cout, cout, (B, 2 * H, 2 * W), seed + 1000)
    y, _, _ = fwd.case(1, cout, cout, (B, 2 * H, 2 * W), seed + 2000)
    y[np.random.default_rng(seed).random(y.shape) < 0.05] = -0.0
    return x, w, dy, y


def _width(cout):
    return max(WIDE, AT + cout + 16)  # (level 4's 512 channels need a wider tensor)


def _wide(a, at=AT):
    width = _width(a.shape[3])
    out = np.full(a.shape[:3] + (width,), POISON, np.uint32).view(F)
    out[..., at:at + a.shape[3]] = a
    return out


def _workspace(L, shape, cin, ksize, cout, stride, transposed):
    nbytes = L.dtfill_conv2d_wide_backward_workspace_bytes(*shape, cin, ksize, cout, stride, transposed)
    assert nbytes > 0
    g = GuardedBuffer(nbytes, 0, DEV)
    g.payload().fill_(0xFF)  # NaNs
    return g, nbytes


def run_data(L, dy, y, w, stride, act, transposed=False, alpha=0.2, dx_channels=None, dx_offset=0, mis=0, residual=False, stream=None):
    """The data gradient on guarded buffers; returns the whole dx tensor [B,H,W,dx_channels] (and dresidual with `residual`)."""
    import torch

    B, Hg, Wg, cout = dy.shape
    ksize, cin = w.shape[0], w.shape[2]
    H, W = (Hg // 2, Wg // 2) if transposed else (stride * Hg, stride * Wg)
    dx_channels = cin if dx_channels is None else dx_channels
    wdy, wy = _wide(dy), _wide(y)
    gdy, gy, gw = fwd._up(wdy, mis), fwd._up(wy, mis), fwd._up(w, mis)
    gdx = fwd._poisoned((B, H, W, dx_channels), mis)
    gres = fwd._poisoned(dy.shape, mis) if residual else None
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout, 2 if transposed else stride, int(transposed))
    yp = gy.ptr if act == R.LEAKY else None
    torch.cuda.synchronize()  # the buffers were filled on the default stream; `stream` may be another
    if transposed:
        rc = L.dtfill_conv2d_transpose_backward_data(gdy.ptr, _width(cout), AT, yp, _width(cout), AT, gw.ptr, B, H, W, cin, cout, act, alpha, gdx.ptr,
                                                     dx_channels, dx_offset, ws.ptr, nbytes, stream)
    else:
        rc = L.dtfill_conv2d_strided_backward_data(gdy.ptr, _width(cout), AT, yp, _width(cout), AT, gw.ptr, B, H, W, cin, ksize, cout, stride, act,
                                                   alpha, gdx.ptr, dx_channels, dx_offset, gres.ptr if gres else None, ws.ptr,
                                                   nbytes, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bwd._unchanged(gdy, wdy, "dy")
    bwd._unchanged(gy, wy, "y")
    bwd._unchanged(gw, w, "w")
    gdx.check("dx")
    ws.check("workspace")
    dx = gdx.view(torch.float32, (B, H, W, dx_channels)).cpu().numpy()
    if not residual:
        return dx
    gres.check("dresidual")
    return dx, gres.view(torch.float32, dy.shape).cpu().numpy()


def run_weights(L, x, dy, y, ksize, stride, act, transposed=False, alpha=0.2, want_db=True, mis=0, stream=None):
    """The weight gradient on guarded buffers; returns (dw, db or None)."""
    import torch

    B, H, W, cin = x.shape
    cout = dy.shape[3]
    wdy, wy = _wide(dy), _wide(y)
    gx, gdy, gy = fwd._up(x, mis), fwd._up(wdy, mis), fwd._up(wy, mis)
    gdw = fwd._poisoned((ksize, ksize, cin, cout), mis)
    gdb = fwd._poisoned((cout,), mis) if want_db else None
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout, 2 if transposed else stride, int(transposed))
    yp = gy.ptr if act == R.LEAKY else None
    torch.cuda.synchronize()  # the buffers were filled on the default stream; `stream` may be another
    if transposed:
        rc = L.dtfill_conv2d_transpose_backward_weights(gx.ptr, gdy.ptr, _width(cout), AT, yp, _width(cout), AT, B, H, W, cin, cout, act, alpha,
                                                        gdw.ptr, gdb.ptr if gdb else None, ws.ptr, nbytes, stream)
    else:
        rc = L.dtfill_conv2d_strided_backward_weights(gx.ptr, gdy.ptr, _width(cout), AT, yp, _width(cout), AT, B, H, W, cin, ksize, cout, stride, act,
                                                      alpha, gdw.ptr, gdb.ptr if gdb else None, ws.ptr, nbytes, stream)
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


_reference = {}


def strided_reference(ksize, stride, cin, cout, act, seed, frame=None):
    """(dx, dw, db) of strided_case() by conv2b_ref, worked out once per case and shared."""
    key = ("s", ksize, stride, cin, cout, act, seed, frame)
    if key not in _reference:
        x, w, dy, y = strided_case(ksize, stride, cin, cout, seed, frame)
        _reference[key] = (RW.strided_dx_ref(dy, y, w, stride, act),) + RW.strided_dw_ref(x, dy, y, ksize, stride, act)
    return _reference[key]


def transposed_reference(cin, cout, act, seed, frame=FRAME):
    key = ("t", cin, cout, act, seed, frame)
    if key not in _reference:
        x, w, dy, y = transposed_case(cin, cout, seed, frame)
        _reference[key] = (RW.transpose_dx_ref(dy, y, w, act),) + RW.transpose_dw_ref(x, dy, y, act)
    return _reference[key]


@pytest.mark.parametrize("ksize,stride,cin,cout,act", STRIDED)
def test_strided_layers_at_every_seam(L, ksize, stride, cin, cout, act):
    what = "%dx%dx%d->%d stride %d" % (ksize, ksize, cin, cout, stride)
    x, w, dy, y = strided_case(ksize, stride, cin, cout, 1)
    dx, dw, db = strided_reference(ksize, stride, cin, cout, act, 1)
    got_dx, got_res = run_data(L, dy, y, w, stride, act, residual=True)
    R.assert_same(got_dx, dx, "dx of " + what)
    R.assert_same(got_res, RW.g_ref(dy, y, act), "dresidual of " + what)
    R.assert_same(run_data(L, dy, y, w, stride, act), dx, "dx without dresidual of " + what)
    got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, act)
    R.assert_same(got_dw, dw, "dw of " + what)
    R.assert_same(got_db, db, "db of " + what)


@pytest.mark.parametrize("cin,cout,act", TRANSPOSED)
def test_transposed_layers_at_every_seam(L, cin, cout, act):
    what = "transposed %d->%d" % (cin, cout)
    x, w, dy, y = transposed_case(cin, cout, 2)
    dx, dw, db = transposed_reference(cin, cout, act, 2)
    R.assert_same(run_data(L, dy, y, w, 2, act, transposed=True), dx, "dx of " + what)
    got_dw, got_db = run_weights(L, x, dy, y, 3, 2, act, transposed=True)
    R.assert_same(got_dw, dw, "dw of " + what)
    R.assert_same(got_db, db, "db of " + what)


@pytest.mark.parametrize("ksize,stride,transposed", ((3, 1, False), (3, 2, False), (1, 2, False), (3, 2, True)))
def test_dx_offset_misalignment_and_null_db(L, ksize, stride, transposed):
    cin, cout, act = 48, 80, R.LEAKY
    if transposed:
        (x, w, dy, y), (dx, dw, db) = transposed_case(cin, cout, 2), transposed_reference(cin, cout, act, 2)
    else:
        (x, w, dy, y), (dx, dw, db) = strided_case(ksize, stride, cin, cout, 1), strided_reference(ksize, stride, cin, cout, act, 1)
    # into channels 8 .. 8 + Cin - 1 of a wider tensor: the others keep their poison
    wide = run_data(L, dy, y, w, stride, act, transposed, dx_channels=cin + 24, dx_offset=8)
    R.assert_same(wide[..., 8:8 + cin], dx, "dx_offset")
    assert (np.delete(wide, np.s_[8:8 + cin], axis=-1).view(np.uint32) == POISON).all()
    # every tensor 4 bytes off a 16-byte boundary
    if transposed:
        R.assert_same(run_data(L, dy, y, w, stride, act, transposed, mis=4), dx, "misaligned dx")
    else:
        got_dx, got_res = run_data(L, dy, y, w, stride, act, mis=4, residual=True)
        R.assert_same(got_dx, dx, "misaligned dx")
        R.assert_same(got_res, RW.g_ref(dy, y, act), "misaligned dresidual")
    got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, act, transposed, mis=4)
    R.assert_same(got_dw, dw, "misaligned dw")
    R.assert_same(got_db, db, "misaligned db")
    got_dw, none = run_weights(L, x, dy, y, ksize, stride, act, transposed, want_db=False)
    assert none is None
    R.assert_same(got_dw, dw, "NULL db")


def test_dx_is_the_forward_entry_points_on_g(L):
    """The identities on the device: dx at stride 1 is dtfill_conv2d_strided(g, wT); at stride 2, 3x3 it is
    dtfill_conv2d_transpose(g, wX); the transposed dx is dtfill_conv2d_strided(g, wX, stride 2)."""
    import torch

    import convb_ref as RB

    def forward(g, w, stride, transposed, frame):
        gg, gw = fwd._up(g), fwd._up(w)
        cin_f, cout_f = w.shape[2], w.shape[3]
        go = fwd._poisoned(frame + (cout_f,))
        B, H, W = g.shape[:3]
        if transposed:
            rc = L.dtfill_conv2d_transpose(gg.ptr, B, H, W, cin_f, gw.ptr, None, cout_f, R.LINEAR, 0.0, go.ptr, cout_f, 0, None)
        else:
            rc = L.dtfill_conv2d_strided(gg.ptr, B, H, W, cin_f, gw.ptr, None, w.shape[0], cout_f, stride, None, R.LINEAR, 0.0, go.ptr,
                                         cout_f, 0, None)
        assert rc == 0
        torch.cuda.synchronize()
        return go.view(torch.float32, frame + (cout_f,)).cpu().numpy()

    cin, cout, act = 48, 80, R.LEAKY
    B, Ho, Wo = FRAME
    x, w, dy, y = strided_case(3, 1, cin, cout, 1)
    R.assert_same(run_data(L, dy, y, w, 1, act), forward(RW.g_ref(dy, y, act), RB.flipped(w), 1, False, FRAME), "stride 1")
    x, w, dy, y = strided_case(3, 2, cin, cout, 1)
    R.assert_same(run_data(L, dy, y, w, 2, act), forward(RW.g_ref(dy, y, act), RW.exchanged(w), 1, True, (B, 2 * Ho, 2 * Wo)), "stride 2")
    x, w, dy, y = transposed_case(cin, cout, 2)
    R.assert_same(run_data(L, dy, y, w, 2, act, transposed=True), forward(RW.g_ref(dy, y, act), RW.exchanged(w), 2, False, FRAME),
                  "transposed")


@pytest.mark.parametrize("ksize,cin", ((3, 16), (1, 48), (7, 64)))
def test_strided_dw_is_the_existing_entry_point_on_the_shared_domain(L, ksize, cin):
    """Stride 1, Cout == 16: the bits of dtfill_conv2d_backward_weights."""
    x, w, dy, y = strided_case(ksize, 1, cin, 16, 4, (2, 33, 65) if ksize < 7 else (2, 9, 33))
    dw, db = bwd.run_weights(L, x, dy, y, ksize, R.LEAKY)
    got_dw, got_db = run_weights(L, x, dy, y, ksize, 1, R.LEAKY)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")


def test_the_one_by_one_stride_two_spread_under_a_non_finite_g(L):
    """dx is +0 off the even grid also where g is infinite or NaN: no zero weight stands in for a missing tap."""
    x, w, dy, y = strided_case(1, 2, 16, 32, 5, (1, 5, 9))
    dy[0, 2, 3, 0], dy[0, 1, 1, 5] = np.inf, np.nan
    dx = RW.strided_dx_ref(dy, y, w, 2, R.LEAKY)
    got = run_data(L, dy, y, w, 2, R.LEAKY)
    R.assert_same(got, dx, "dx")
    odd = np.ones(dx.shape[1:3], bool)
    odd[::2, ::2] = False
    assert (got[:, odd] == 0).all() and not np.isfinite(got[:, ::2, ::2]).all()


def test_non_finite_values_follow_fmaf(L):
    """An inf and a NaN in x, dy and y of a stride-2 and of the transposed layer; an infinite x in the frame's last column lies
    under the pixels that pad a row's last k-step, and must not reach dw."""
    ksize, stride, cin, cout, act = 3, 2, 16, 32, R.LEAKY
    frame = (1, 5, 9)
    x, w, dy, y = strided_case(ksize, stride, cin, cout, 6, frame)
    x[0, 2, 3, 0], x[0, 6, 12, cin - 1], x[0, 4, x.shape[2] - 1, 0] = np.inf, np.nan, np.inf
    dy[0, 1, 2, 0], dy[0, 4, 8, cout - 1] = np.nan, -np.inf
    y[0, 3, 3, 0] = np.nan
    dx, (dw, db) = RW.strided_dx_ref(dy, y, w, stride, act), RW.strided_dw_ref(x, dy, y, ksize, stride, act)
    assert np.isnan(dw).any() and np.isfinite(dw).any() and np.isnan(db).any()
    R.assert_same(run_data(L, dy, y, w, stride, act), dx, "dx")
    got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, act)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")
    x, w, dy, y = transposed_case(cin, cout, 7, frame)
    x[0, 2, 3, 0], x[0, 4, 8, 1] = np.inf, np.nan
    dy[0, 1, 2, 0], dy[0, 9, 17, cout - 1] = np.nan, -np.inf
    dx, (dw, db) = RW.transpose_dx_ref(dy, y, w, act), RW.transpose_dw_ref(x, dy, y, act)
    R.assert_same(run_data(L, dy, y, w, 2, act, transposed=True), dx, "transposed dx")
    got_dw, got_db = run_weights(L, x, dy, y, 3, 2, act, transposed=True)
    R.assert_same(got_dw, dw, "transposed dw")
    R.assert_same(got_db, db, "transposed db")


def test_bits_do_not_depend_on_the_run_or_the_stream(L):
    import torch

    cin, cout, act = 48, 80, R.LEAKY
    x, w, dy, y = strided_case(3, 2, cin, cout, 1)
    dx, dw, db = strided_reference(3, 2, cin, cout, act, 1)
    xt, wt, dyt, yt = transposed_case(cin, cout, 2)
    tdx, tdw, tdb = transposed_reference(cin, cout, act, 2)
    for stream in (torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)):
        for _ in range(2):
            R.assert_same(run_data(L, dy, y, w, 2, act, stream=stream.cuda_stream), dx, "dx")
            got_dw, got_db = run_weights(L, x, dy, y, 3, 2, act, stream=stream.cuda_stream)
            R.assert_same(got_dw, dw, "dw")
            R.assert_same(got_db, db, "db")
        got_dw, got_db = run_weights(L, xt, dyt, yt, 3, 2, act, transposed=True, stream=stream.cuda_stream)
        R.assert_same(got_dw, tdw, "transposed dw")
        R.assert_same(got_db, tdb, "transposed db")
        R.assert_same(run_data(L, dyt, yt, wt, 2, act, transposed=True, stream=stream.cuda_stream), tdx, "transposed dx")


def test_the_channel_counts_of_level_four(L):
    """512 -> 512 3x3 at 2 x 3 pixels and its transposed partner 512 -> 256: the work items are almost all channel groups."""
    frame = (1, 2, 3)
    x, w, dy, y = strided_case(3, 1, 512, 512, 8, frame)
    dx, dw, db = strided_reference(3, 1, 512, 512, R.LEAKY, 8, frame)
    R.assert_same(run_data(L, dy, y, w, 1, R.LEAKY), dx, "dx")
    got_dw, got_db = run_weights(L, x, dy, y, 3, 1, R.LEAKY)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")
    x, w, dy, y = transposed_case(512, 256, 9, frame)
    dx, dw, db = transposed_reference(512, 256, R.LEAKY, 9, frame)
    R.assert_same(run_data(L, dy, y, w, 2, R.LEAKY, transposed=True), dx, "transposed dx")
    got_dw, got_db = run_weights(L, x, dy, y, 3, 2, R.LEAKY, transposed=True)
    R.assert_same(got_dw, dw, "transposed dw")
    R.assert_same(got_db, db, "transposed db")


def test_device_layer(pkg, L):
    """The four device functions: slices of wider tensors, a side stream, dresidual, and the refusals."""
    import torch

    dev = pkg.device
    cin, cout, act = 48, 80, R.LEAKY
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x, w, dy, y = strided_case(3, 2, cin, cout, 1)
    dx, dw, db = strided_reference(3, 2, cin, cout, act, 1)
    tx, tw, tdy, ty = t(x), t(w), t(_wide(dy)), t(_wide(y))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got, res = dev.conv2d_strided_backward_data_device(tdy, tw, 2, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, want_residual=True)
        got_dw, got_db = dev.conv2d_strided_backward_weights_device(tx, tdy, 3, 2, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, cout=cout)
    s.synchronize()
    R.assert_same(got.cpu().numpy(), dx, "dx on a side stream")
    R.assert_same(res.cpu().numpy(), RW.g_ref(dy, y, act), "dresidual")
    R.assert_same(got_dw.cpu().numpy(), dw, "dw")
    R.assert_same(got_db.cpu().numpy(), db, "db")
    assert dev.conv2d_strided_backward_weights_device(tx, t(dy), 3, 2, t(y), "leaky", want_bias=False)[1] is None
    x, w, dy, y = transposed_case(cin, cout, 2)
    dx, dw, db = transposed_reference(cin, cout, act, 2)
    tx, tw, tdy, ty = t(x), t(w), t(_wide(dy)), t(_wide(y))
    R.assert_same(dev.conv2d_transpose_backward_data_device(tdy, tw, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT).cpu().numpy(), dx, "dx")
    got_dw, got_db = dev.conv2d_transpose_backward_weights_device(tx, tdy, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, cout=cout)
    R.assert_same(got_dw.cpu().numpy(), dw, "transposed dw")
    R.assert_same(got_db.cpu().numpy(), db, "transposed db")
    assert dev.conv2d_wide_backward_workspace_bytes(2, 33, 65, cin, 3, cout, 2, True) == \
        L.dtfill_conv2d_wide_backward_workspace_bytes(2, 33, 65, cin, 3, cout, 2, 1)
    for bad in (dict(y=None), dict(alpha=-0.1), dict(act="relu"), dict(dy_offset=40), dict(w_packed=tw[:, :2].contiguous()), dict(dx=tdy)):
        with pytest.raises(ValueError):
            dev.conv2d_transpose_backward_data_device(**dict(dict(dy=tdy, w_packed=tw, y=ty, act="leaky", dy_offset=AT, y_offset=AT), **bad))
    with pytest.raises(ValueError):  # an odd frame at stride 2
        dev.conv2d_strided_backward_weights_device(t(np.zeros((1, 5, 6, 16), F)), t(np.zeros((1, 3, 3, 16), F)), 3, 2)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_wide_backward_workspace_bytes(2, 9, 33, 8, 3, 16)


SHARED = (2, 33, 67)  # 2 x 2 segments, a ragged last strip, a row end that is no multiple of the four-pixel k-step


def _shared_domain_layer(ksize, cin, seed):
    """A leaky layer of Cout == 16 on SHARED as device tensors: x, w, and dy and y at channel AT of wider tensors."""
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x, w, dy, y = strided_case(ksize, 1, cin, 16, seed, SHARED)
    return t(x), t(w), t(_wide(dy)), t(_wide(y))


@pytest.mark.parametrize("ksize,cin", ((3, 16), (7, 64), (1, 32)))
def test_device_layer_dw_of_both_entry_points_on_the_shared_domain(pkg, L, ksize, cin):
    """include/dtfill.h on dtfill_conv2d_strided_backward_weights: at stride 1 and Cout == 16 dw and db are
    dtfill_conv2d_backward_weights' values (the sign of a zero aside), here through the two device functions."""
    dev = pkg.device
    tx, _, tdy, ty = _shared_domain_layer(ksize, cin, 11)
    dw, db = dev.conv2d_backward_weights_device(tx, tdy, ksize, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, cout=16)
    got_dw, got_db = dev.conv2d_strided_backward_weights_device(tx, tdy, ksize, 1, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT, cout=16)
    R.assert_same(got_dw.cpu().numpy(), dw.cpu().numpy(), "dw")
    R.assert_same(got_db.cpu().numpy(), db.cpu().numpy(), "db")


@pytest.mark.parametrize("ksize,cin", ((3, 32), (5, 64)))
def test_device_layer_dx_of_both_entry_points_on_the_shared_domain(pkg, L, ksize, cin):
    """Cin >= 32, Cout == 16, stride 1: both data calls run the same chain, and dx is the same bit for bit."""
    dev = pkg.device
    _, tw, tdy, ty = _shared_domain_layer(ksize, cin, 12)
    dx = dev.conv2d_backward_data_device(tdy, tw, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT)
    got = dev.conv2d_strided_backward_data_device(tdy, tw, 1, ty, "leaky", 0.2, dy_offset=AT, y_offset=AT)
    assert got.shape == dx.shape == SHARED + (cin,)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), dx.cpu().numpy().view(np.uint32))


def test_autograd_conv2d_reads_a_sliced_gradient_in_place(pkg, L):
    """Two stems joined by torch.cat under a 3x3 layer: each stem's gradient arrives as 16 channels of the layer's 32-wide dx.
    The stems' kernel and bias gradients are those of contiguous copies of the two halves, bit for bit."""
    import torch

    dev, conv2d = pkg.device, pkg.autograd.conv2d
    B, H, W = 1, 5, 9
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    planes = [t(fwd.case(3, 1, 16, (B, H, W), 20 + i)[0][..., 0]) for i in range(2)]
    stems = [[t(a).requires_grad_() for a in fwd.case(3, 1, 16, (B, H, W), 30 + i)[1:]] for i in range(2)]
    w, bias = (t(a).requires_grad_() for a in fwd.case(3, 32, 16, (B, H, W), 40)[1:])
    ys = [conv2d(p, k, b, "leaky", 0.2) for p, (k, b) in zip(planes, stems)]
    out = conv2d(torch.cat(ys, dim=3), w, bias, "leaky", 0.2)
    upstream = t(fwd.case(1, 16, 16, (B, H, W), 50)[0])
    out.backward(upstream)
    with torch.no_grad():
        dx = dev.conv2d_backward_data_device(upstream, w.detach(), out.detach(), "leaky", 0.2)
        for i, (p, (k, b), y) in enumerate(zip(planes, stems, ys)):
            half = dx[..., 16 * i:16 * i + 16].contiguous()
            dw, db = dev.conv2d_backward_weights_device(p, half, 3, y.detach(), "leaky", 0.2)
            assert np.array_equal(k.grad.cpu().numpy().view(np.uint32), dw.cpu().numpy().view(np.uint32)), "stem %d: kernel" % i
            assert np.array_equal(b.grad.cpu().numpy().view(np.uint32), db.cpu().numpy().view(np.uint32)), "stem %d: bias" % i

"""dtfill_conv2d_strided_backward_data_bf16 / _weights_bf16 and dtfill_conv2d_transpose_backward_data_bf16 / _weights_bf16 on the
device against the numpy statement of their contracts (tests/convb_bf16_ref.py), through the ABI on guarded buffers with poisoned
outputs and a poisoned workspace, as the float32 twins' tests (test_gpu_conv2d_wide_backward.py, whose helpers are used).

The shapes are the smallest that cross every seam: the small frame (the strided layers' output frame, the transposed layer's input
frame) is (2, 33, 65), one row past the 32-row segment and one column past the 64-column one, so the last k-step of 32 pixels has
ONE real pixel; (1, 3, 40) is a whole k-step plus 8.  Cin = 48 and Cout = 80: three and five tiles, a full pass of four and a
partial one, and a half group of 32 for dx's forward over g.  Five layers: 3x3 and 1x1 at both strides, and the transposed one."""
import numpy as np
import pytest

import conv_bf16_ref as RH
import conv_ref as R
import convb_bf16_ref as RHB
import test_gpu_conv2d as fwd
import test_gpu_conv2d_backward as bwd
import test_gpu_conv2d_wide_backward as wb
from guarded import GuardedBuffer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
POISON = fwd.POISON
AT = wb.AT
FRAME, FRAME40 = (2, 33, 65), (1, 3, 40)
CIN, COUT = 48, 80
LAYERS = ((3, 1, False), (1, 1, False), (3, 2, False), (1, 2, False), (3, 2, True))  # ksize, stride, transposed
IDS = ["3x3s1", "1x1s1", "3x3s2", "1x1s2", "transposed"]
ACT, ALPHA = R.LEAKY, RHB.ALPHA_INT


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def _symbol(L, transposed, what, bf16):
    return getattr(L, "dtfill_conv2d_%s_backward_%s%s" % ("transpose" if transposed else "strided", what, "_bf16" if bf16 else ""))


def _workspace(L, shape, cin, ksize, cout, stride, transposed, bf16):
    size = L.dtfill_conv2d_wide_backward_bf16_workspace_bytes if bf16 else L.dtfill_conv2d_wide_backward_workspace_bytes
    nbytes = size(*shape, cin, ksize, cout, stride, transposed)
    assert nbytes > 0
    g = GuardedBuffer(nbytes, 0, DEV)
    g.payload().fill_(0xFF)  # NaNs
    return g, nbytes


def _placed(a, dense):
    """dy or y as the call reads it: (array, width, offset): at channel AT of a wider poisoned tensor, or dense.  y = None (a
    linear layer's NULL) stays None."""
    if a is None:
        return None, 0, 0
    return (a, a.shape[3], 0) if dense else (wb._wide(a), wb._width(a.shape[3]), AT)


def run_data(L, dy, y, w, stride, transposed=False, alpha=ALPHA, dx_channels=None, dx_offset=0, mis=0, residual=False, stream=None,
             dense=False, bf16=True, act=ACT):
    """The data gradient on guarded buffers; returns the whole dx tensor [B,H,W,dx_channels] (and dresidual with `residual`).
    y = None passes NULL (act = R.LINEAR)."""
    import torch

    B, Hg, Wg, cout = dy.shape
    ksize, cin = w.shape[0], w.shape[2]
    H, W = (Hg // 2, Wg // 2) if transposed else (stride * Hg, stride * Wg)
    dx_channels = cin if dx_channels is None else dx_channels
    (wdy, width, at), (wy, _, _) = _placed(dy, dense), _placed(y, dense)
    gdy, gy, gw = fwd._up(wdy, mis), (None if y is None else fwd._up(wy, mis)), fwd._up(w, mis)
    gdx = fwd._poisoned((B, H, W, dx_channels), mis)
    gres = fwd._poisoned(dy.shape, mis) if residual else None
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout, 2 if transposed else stride, int(transposed), bf16)
    torch.cuda.synchronize()
    head = (gdy.ptr, width, at, gy.ptr if gy else None, width, at, gw.ptr, B, H, W, cin)
    if transposed:
        rc = _symbol(L, True, "data", bf16)(*head, cout, act, alpha, gdx.ptr, dx_channels, dx_offset, ws.ptr, nbytes, stream)
    else:
        rc = _symbol(L, False, "data", bf16)(*head, ksize, cout, stride, act, alpha, gdx.ptr, dx_channels, dx_offset,
                                             gres.ptr if gres else None, ws.ptr, nbytes, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bwd._unchanged(gdy, wdy, "dy")
    if gy:
        bwd._unchanged(gy, wy, "y")
    bwd._unchanged(gw, w, "w")
    gdx.check("dx")
    ws.check("workspace")
    dx = gdx.view(torch.float32, (B, H, W, dx_channels)).cpu().numpy()
    if not residual:
        return dx
    gres.check("dresidual")
    return dx, gres.view(torch.float32, dy.shape).cpu().numpy()


def run_weights(L, x, dy, y, ksize, stride, transposed=False, alpha=ALPHA, want_db=True, mis=0, stream=None, dense=False, bf16=True,
                act=ACT):
    """The weight gradient on guarded buffers; returns (dw, db or None).  y = None passes NULL (act = R.LINEAR)."""
    import torch

    B, H, W, cin = x.shape
    cout = dy.shape[3]
    (wdy, width, at), (wy, _, _) = _placed(dy, dense), _placed(y, dense)
    gx, gdy, gy = fwd._up(x, mis), fwd._up(wdy, mis), (None if y is None else fwd._up(wy, mis))
    gdw = fwd._poisoned((ksize, ksize, cin, cout), mis)
    gdb = fwd._poisoned((cout,), mis) if want_db else None
    ws, nbytes = _workspace(L, (B, H, W), cin, ksize, cout, 2 if transposed else stride, int(transposed), bf16)
    torch.cuda.synchronize()
    head = (gx.ptr, gdy.ptr, width, at, gy.ptr if gy else None, width, at, B, H, W, cin)
    tail = (act, alpha, gdw.ptr, gdb.ptr if gdb else None, ws.ptr, nbytes, stream)
    if transposed:
        rc = _symbol(L, True, "weights", bf16)(*head, cout, *tail)
    else:
        rc = _symbol(L, False, "weights", bf16)(*head, ksize, cout, stride, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bwd._unchanged(gx, x, "x")
    bwd._unchanged(gdy, wdy, "dy")
    if gy:
        bwd._unchanged(gy, wy, "y")
    gdw.check("dw")
    ws.check("workspace")
    if gdb:
        gdb.check("db")
    return (gdw.view(torch.float32, (ksize, ksize, cin, cout)).cpu().numpy(),
            gdb.view(torch.float32, (cout,)).cpu().numpy() if gdb else None)


_shared = {}


def integer_layer(ksize, stride, transposed, frame=FRAME):
    """(x, w, dy, y) of convb_bf16_ref.integer_case and (dx, dresidual, dw, db) of its int64 reference: worked out once."""
    key = ("int", ksize, stride, transposed, frame)
    if key not in _shared:
        case = RHB.integer_case(ksize, stride, CIN, COUT, frame, 7 + ksize + 2 * stride + transposed, transposed)
        _shared[key] = case, RHB.integer_ref(*case, stride, ACT, transposed)
    return _shared[key]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


# ---- exact integer cases, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", (FRAME, FRAME40), ids=("33x65", "3x40"))
@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_integer_cases_are_exact(L, ksize, stride, transposed, frame):
    (x, w, dy, y), (dx, g, dw, db) = integer_layer(ksize, stride, transposed, frame)
    out = run_data(L, dy, y, w, stride, transposed, dx_channels=CIN + 24, dx_offset=8, residual=not transposed)
    wide, res = out if not transposed else (out, None)
    R.assert_same(wide[..., 8:8 + CIN], dx, "dx")
    assert (np.delete(wide, np.s_[8:8 + CIN], axis=-1).view(np.uint32) == POISON).all(), "channels outside the dx slice"
    if res is not None:
        R.assert_same(res, g, "dresidual")
    got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, transposed)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")


# ---- one-hot sweeps ------------------------------------------------------------------------------------------------------------

def _seams(H, W, count):
    """Pixels of an [H,W] frame at its corners and at the segment and k-step seams, at most `count` of them, distinct."""
    rows = sorted({r for r in (0, 1, 30, 31, 32, 33, 63, 64, 65, H - 2, H - 1) if 0 <= r < H})
    cols = sorted({c for c in (0, 1, 15, 16, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129, W - 2, W - 1) if 0 <= c < W})
    pts = [(r, c) for r in rows for c in cols if (r, c) != (H - 1, W - 1)]
    step = max(1, len(pts) // count)
    pts = pts[::step][:count - 1] + [(H - 1, W - 1)]
    assert len(set(pts)) == len(pts)
    return pts


@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_one_hot_sweep(L, ksize, stride, transposed):
    """Output channel k of g (then input channel k of x) is zero but for ONE pixel, a different corner or seam for every k, in the
    second frame; the other operand is dense integers.  Column k of dw then holds exactly the taps the contract names for that
    pixel: the int64 reference, which is a single product per entry."""
    (x, w, dy, y), _ = integer_layer(ksize, stride, transposed)
    y = np.abs(y) + F(1)  # g = dy
    hot = np.zeros_like(dy)
    pts = _seams(dy.shape[1], dy.shape[2], COUT)
    for k, (r, c) in enumerate(pts):
        hot[1, r, c, k] = F(k % 5 + 1)
    _, _, dw, db = RHB.integer_ref(x, w, hot, y, stride, ACT, transposed)
    assert len(pts) >= 40 and np.count_nonzero(db) == len(pts) and np.count_nonzero(dw) > len(pts)
    got_dw, got_db = run_weights(L, x, hot, y, ksize, stride, transposed)
    R.assert_same(got_dw, dw, "dw under a one-hot g")
    R.assert_same(got_db, db, "db under a one-hot g")
    hot = np.zeros_like(x)
    for k, (r, c) in enumerate(_seams(x.shape[1], x.shape[2], CIN)):
        hot[1, r, c, k] = F(k % 7 + 1)
    _, _, dw, db = RHB.integer_ref(hot, w, dy, y, stride, ACT, transposed)
    got_dw, got_db = run_weights(L, hot, dy, y, ksize, stride, transposed)
    R.assert_same(got_dw, dw, "dw under a one-hot x")
    R.assert_same(got_db, db, "db under a one-hot x")


# ---- the identities on the device ------------------------------------------------------------------------------------------------

def forward_bf16(L, g, w, ksize, stride, transposed, out_frame):
    """dtfill_conv2d_pack_bf16 of w, then the bf16 forward entry point over g, linear, no bias: [B,Ho,Wo,Cout of w]."""
    import torch

    cin_f, cout_f = w.shape[2], w.shape[3]
    gg, gw = fwd._up(g), fwd._up(w)
    packed = GuardedBuffer(2 * RH.packed_elems(ksize, cin_f, cout_f), 0, DEV)
    go = fwd._poisoned(out_frame + (cout_f,))
    B, H, W = g.shape[:3]
    assert L.dtfill_conv2d_pack_bf16(gw.ptr, ksize, cin_f, cout_f, packed.ptr, None) == 0
    if transposed:
        rc = L.dtfill_conv2d_transpose_bf16(gg.ptr, B, H, W, cin_f, packed.ptr, None, cout_f, R.LINEAR, 0.0, go.ptr, cout_f, 0, None)
    else:
        rc = L.dtfill_conv2d_strided_bf16(gg.ptr, B, H, W, cin_f, packed.ptr, None, ksize, cout_f, stride, None, R.LINEAR, 0.0, go.ptr, cout_f,
                                          0, None)
    assert rc == 0
    torch.cuda.synchronize()
    packed.check("packed")
    return go.view(torch.float32, out_frame + (cout_f,)).cpu().numpy()


def random_layer(ksize, stride, transposed, frame=FRAME, seed=0):
    """N(0,1) x, w, dy and y: (x, w, dy, y)."""
    key = ("rnd", ksize, stride, transposed, frame, seed)
    if key not in _shared:
        rng = np.random.default_rng(100 + seed + ksize + 2 * stride + transposed)
        B, Hs, Ws = frame
        xs = (B, Hs, Ws) if transposed else (B, stride * Hs, stride * Ws)
        ys = (B, 2 * Hs, 2 * Ws) if transposed else (B, Hs, Ws)
        _shared[key] = (rng.standard_normal(xs + (CIN,)).astype(F), rng.standard_normal((ksize, ksize, CIN, COUT)).astype(F),
                        rng.standard_normal(ys + (COUT,)).astype(F), rng.standard_normal(ys + (COUT,)).astype(F))
    return _shared[key]


@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_dx_is_the_bf16_forward_over_g_and_dresidual_the_twins(L, ksize, stride, transposed):
    x, w, dy, y = random_layer(ksize, stride, transposed)
    g = RHB.g_ref(dy, y, ACT, 0.2)
    B, Hs, Ws = FRAME
    kernel = RHB.dx_kernel(w, stride, transposed)
    if transposed:
        want = forward_bf16(L, g, kernel, 3, 2, False, FRAME)
    elif stride == 1:
        want = forward_bf16(L, g, kernel, ksize, 1, False, FRAME)
    elif ksize == 3:
        want = forward_bf16(L, g, kernel, 3, 2, True, (B, 2 * Hs, 2 * Ws))
    else:
        want = np.zeros((B, 2 * Hs, 2 * Ws, CIN), F)
        want[:, ::2, ::2] = forward_bf16(L, g, kernel, 1, 1, False, FRAME)
    if transposed:
        got = run_data(L, dy, y, w, 2, True, alpha=0.2)
    else:
        got, res = run_data(L, dy, y, w, stride, alpha=0.2, residual=True)
        _, twin_res = run_data(L, dy, y, w, stride, alpha=0.2, residual=True, bf16=False)
        assert same_bits(res, twin_res) and same_bits(res, g), "dresidual"
    assert same_bits(got, want), "dx against the forward entry point"
    if ksize == 1 and stride == 2:
        odd = np.ones(got.shape[1:3], bool)
        odd[::2, ::2] = False
        assert (got[:, odd].view(np.uint32) == 0).all(), "+0 literally off the even grid"


# ---- random data within the derived bound ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_random_data_within_the_bound(L, ksize, stride, transposed):
    x, w, dy, y = random_layer(ksize, stride, transposed)
    dx, S, n = RHB.dx_ref(dy, y, w, stride, ACT, 0.2, transposed)
    dw, db, bw, bb = RHB.dw_ref(x, dy, y, ksize, stride, ACT, 0.2, transposed)
    got_dx = run_data(L, dy, y, w, stride, transposed, alpha=0.2)
    got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, transposed, alpha=0.2)
    ratios = [float((np.abs(got - want) / bound).max()) for got, want, bound in
              ((got_dx, dx, RHB.dx_bound(S, n)), (got_dw, dw, bw), (got_db, db, bb))]
    print("bf16 backward %dx%d stride %d%s: worst |error| / bound  dx %.2e  dw %.2e  db %.2e"
          % (ksize, ksize, stride, " transposed" if transposed else "", *ratios))
    assert ratios[0] <= 1 and ratios[1] <= 1 and ratios[2] <= 1, ratios
    assert np.abs(dw).max() > 1 and np.abs(dx).max() > 1


# ---- determinism, misalignment, NaN sets, NULL db ----------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_bits_do_not_depend_on_the_frame_the_run_the_stream_or_the_alignment(L, ksize, stride, transposed):
    import torch

    x, w, dy, y = (a[:1] if i != 1 else a for i, a in enumerate(random_layer(ksize, stride, transposed)))
    twice = lambda a: np.concatenate([a, a])
    dx2 = run_data(L, twice(dy), twice(y), w, stride, transposed, alpha=0.2)
    assert same_bits(dx2[0], dx2[1]), "dx of one frame twice"
    dx = run_data(L, dy, y, w, stride, transposed, alpha=0.2)
    assert same_bits(dx[0], dx2[0]), "dx of the frame alone"
    dw, db = run_weights(L, x, dy, y, ksize, stride, transposed, alpha=0.2)
    stream = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(stream=stream.cuda_stream), dict(mis=4), dict(dense=True)):
        assert same_bits(run_data(L, dy, y, w, stride, transposed, alpha=0.2, **kw), dx), ("dx", kw)
        got_dw, got_db = run_weights(L, x, dy, y, ksize, stride, transposed, alpha=0.2, **kw)
        assert same_bits(got_dw, dw) and same_bits(got_db, db), ("dw, db", kw)
    got_dw, none = run_weights(L, x, dy, y, ksize, stride, transposed, alpha=0.2, want_db=False)
    assert none is None and same_bits(got_dw, dw), "NULL db"


@pytest.mark.parametrize("ksize,stride,transposed", LAYERS, ids=IDS)
def test_nan_sets_are_the_float32_twins(L, ksize, stride, transposed):
    """One NaN in g and one in x, each beside a frame's edge so that padding meets it: +0 * NaN = NaN on both paths."""
    (x, w, dy, y), _ = integer_layer(ksize, stride, transposed, FRAME40)
    x, dy = x.copy(), dy.copy()
    dy[0, dy.shape[1] - 1, dy.shape[2] - 1, 3] = np.nan
    x[0, 0, x.shape[2] - 1, 5] = np.nan
    dw, db = run_weights(L, x, dy, y, ksize, stride, transposed)
    tdw, tdb = run_weights(L, x, dy, y, ksize, stride, transposed, bf16=False)
    assert np.array_equal(np.isnan(dw), np.isnan(tdw)) and np.array_equal(np.isnan(db), np.isnan(tdb))
    assert np.isnan(dw).any() and not np.isnan(dw).all() and np.isnan(db).sum() == 1
    finite = ~np.isnan(tdw)
    R.assert_same(dw[finite], tdw[finite], "the finite entries (exact integers on both paths)")

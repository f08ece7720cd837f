"""The backward of dtfill_conv2d without a device: the numpy statement of its contracts (tests/convb_ref.py) against float64
autograd within derived bounds, what the statement pins (which pixel meets which tap, the padding, the flip, the derivative at
zero and NaN, the two-level order of the weight gradient), tests/netgrad_ref.py against float64 autograd of the same network,
and everything of the entry points that needs no GPU (return codes, the workspace rule, the binding, the Python layer's checks).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import conv_ref as R
import convb_ref as RB
import netgrad_ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
U = 2.0 ** -24


def _case(ksize, cin, cout, shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape + (cin,)) * 2.0 ** rng.integers(-3, 4, shape + (cin,))).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    dy = (rng.standard_normal(shape + (cout,)) * 2.0 ** rng.integers(-3, 4, shape + (cout,))).astype(F)
    return x, w, rng.standard_normal(cout).astype(F), dy


# ---- against float64 autograd --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize,cin,cout,act", R.NET_LAYERS)
def test_against_float64_autograd(ksize, cin, cout, act):
    """F.conv2d + leaky_relu in float64 under torch's tape.  y, which only decides the derivative's branch, is the float64
    forward rounded to float32 (a rounding keeps the sign), so both sides take the same branch everywhere.  The bounds, derived:
      g   one rounded multiply: |g - g64| <= u |g64|, u = 2^-24; both gradients are linear in g, so this passes into them as
          u sum |g64| |w| and u sum |x| |g64|, beside the chains' own error:
      dx  a chain of K = ksize^2 Cout links over g: gamma_K sum |g| |w|
      dw  level 1 is a chain of at most n1 = min(R C, H W) links, level 2 adds the S segments' partials, so every product
          passes through at most n1 + S roundings: gamma_(n1 + S) sum |x| |g|;  db likewise with |x| = 1.
    With |g| <= (1 + u) |g64| the two together are (gamma_n (1 + u) + u) times the absolute sum over g64.
    (The float64 side's own error is 2^-29 of these and is not added.)"""
    import torch
    import torch.nn.functional as TF

    shape = (2, 9, 11) if ksize * ksize * cin > 1000 else (2, ROWS + 1, COLS + 3)  # (more than one segment where it is cheap)
    x, w, bias, dy = _case(ksize, cin, cout, shape, 11 * ksize + cin)
    alpha = float(F(0.2))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    tx, tw, tb = t(x).permute(0, 3, 1, 2).requires_grad_(True), t(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True), t(bias).requires_grad_(True)
    y64 = TF.conv2d(tx, tw, tb, padding=ksize // 2)
    if act == R.LEAKY:
        y64 = TF.leaky_relu(y64, alpha)
    y64.backward(t(dy).permute(0, 3, 1, 2))
    y = y64.detach().permute(0, 2, 3, 1).numpy().astype(F)
    assert (y != 0).all()
    g64 = np.where(y > 0, dy.astype(np.float64), dy.astype(np.float64) * alpha) if act == R.LEAKY else dy.astype(np.float64)
    dx = RB.dx_ref(dy, y, w, act, 0.2)
    dw, db = RB.dw_ref(x, dy, y, ksize, act, 0.2)
    want_dx = tx.grad.permute(0, 2, 3, 1).numpy()
    with_g = lambda n: R.gamma(n) * (1 + U) + U
    bound = with_g(ksize * ksize * cout) * R.abs_sum(g64, RB.flipped(w))
    assert (np.abs(dx - want_dx) <= bound).all() and np.abs(want_dx).max() > 0
    B, H, W = shape
    nseg = len(RB.segments(B, H, W))
    n = min(ROWS * COLS, H * W) + nseg
    want_dw = tw.grad.permute(2, 3, 1, 0).numpy()
    # sum |x| |g| per (i, j, c, o): the same correlation on absolute values, in float64
    tax, tag = t(np.abs(x)).permute(3, 0, 1, 2), t(np.abs(g64)).permute(3, 0, 1, 2)
    abs_dw = TF.conv2d(tax, tag, padding=ksize // 2).permute(2, 3, 0, 1).numpy()  # [ksize, ksize, Cin, Cout]
    assert abs_dw.shape == dw.shape
    err = np.abs(dw - want_dw)
    assert (err <= with_g(n) * abs_dw).all() and np.abs(want_dw).max() > 0, (err / abs_dw).max() / with_g(n)
    assert (np.abs(db - tb.grad.numpy()) <= with_g(n) * np.abs(g64).sum(axis=(0, 1, 2))).all()


# ---- what the statement pins -----------------------------------------------------------------------------------------------

def test_which_pixel_meets_which_tap_and_the_padding():
    """A 3 x 3 frame, 3x3 kernel, one channel each way.  dy = 1 at the centre alone: dw[i, j] is x[1 + i - 1, 1 + j - 1], the
    frame itself, and dx is the kernel as stored (each pixel receives the weight of the tap it was read through).  dy = 1 at
    the corner (0, 0): its window hangs over the frame, dw[i, j] = x[i - 1, j - 1] inside and +0 on the padding, and dx[h, v] =
    w[h + 1, v + 1] on the four pixels the window covers."""
    x = np.arange(1, 10, dtype=F).reshape(1, 3, 3, 1)
    w = np.arange(10, 19, dtype=F).reshape(3, 3, 1, 1)
    dy = np.zeros((1, 3, 3, 1), F)
    dy[0, 1, 1, 0] = 1
    dw, db = RB.dw_ref(x, dy, None, 3, R.LINEAR)
    assert (dw[:, :, 0, 0] == x[0, :, :, 0]).all() and db[0] == 1
    dx = RB.dx_ref(dy, None, w, R.LINEAR)
    # x[h, v] reached y[1, 1] through tap (h, v), so dx[h, v] = w[h, v]: as a correlation over g that is the kernel flipped,
    # dx[h, v] = g[h + i - 1, v + j - 1] wT[i, j] at i = 2 - h, j = 2 - v
    assert (dx[0, :, :, 0] == w[:, :, 0, 0]).all() and (dx[0, :, :, 0] == RB.flipped(w)[::-1, ::-1, 0, 0]).all()
    dy[:] = 0
    dy[0, 0, 0, 0] = 1
    dw, db = RB.dw_ref(x, dy, None, 3, R.LINEAR)
    want = np.zeros((3, 3), F)
    want[1:, 1:] = x[0, :2, :2, 0]  # taps (0, .) and (., 0) read the padding
    assert (dw[:, :, 0, 0] == want).all()
    dx = RB.dx_ref(dy, None, w, R.LINEAR)
    want = np.zeros((3, 3), F)
    want[:2, :2] = w[1:, 1:, 0, 0]  # y[0, 0] read x[h, v] through tap (h + 1, v + 1)
    assert (dx[0, :, :, 0] == want).all()
    # the flip exchanges the channel axes too: Cin = 2, Cout = 3, a 1x1 kernel is a plain matrix
    w = np.arange(6, dtype=F).reshape(1, 1, 2, 3)
    assert RB.flipped(w).shape == (1, 1, 3, 2) and (RB.flipped(w)[0, 0] == w[0, 0].T).all()
    w = np.arange(18, dtype=F).reshape(3, 3, 2, 1)
    assert RB.flipped(w)[0, 2, 0, 1] == w[2, 0, 1, 0]


def test_the_derivative_at_zero_minus_zero_and_nan():
    dy = np.full(6, 3, F)
    y = F([2, 0.0, -0.0, -1, np.nan, np.inf])
    g = RB.g_ref(dy, y, R.LEAKY, 0.2)
    slope = F(3) * F(0.2)
    assert (g == F([3, slope, slope, slope, slope, 3])).all()  # y > 0 alone takes dy: +-0 and NaN take the alpha branch
    assert (RB.g_ref(dy, y, R.LINEAR) == dy).all() and (RB.g_ref(dy, None, R.LINEAR) == dy).all()
    assert np.isnan(RB.g_ref(F([np.nan, np.nan]), F([1, -1]), R.LEAKY)).all()
    # one rounded multiply: dy * alpha in float32, not dy * 0.2 in double rounded
    dy = F([1 + 2.0 ** -23])
    assert RB.g_ref(dy, F([-1]), R.LEAKY, 0.2)[0] == dy[0] * F(0.2)


def _literal_dx(g, w):
    """The header's statement of dx with scalar loops."""
    B, H, W, cout = g.shape
    ksize, cin = w.shape[0], w.shape[2]
    r = (ksize - 1) // 2
    dx = np.zeros((B, H, W, cin), F)
    for b in range(B):
        for h in range(H):
            for v in range(W):
                for c in range(cin):
                    acc = F(0)
                    for G in range(0, cout, 16):
                        for i in range(ksize):
                            for j in range(ksize):
                                for o in range(G, min(G + 16, cout)):
                                    hh, vv = h + i - r, v + j - r
                                    a = g[b, hh, vv, o] if 0 <= hh < H and 0 <= vv < W else F(0)
                                    acc = R.fma32(a, w[ksize - 1 - i, ksize - 1 - j, c, o], acc).reshape(())[()]
                    dx[b, h, v, c] = acc
    return dx


def test_dx_is_the_forward_on_g_under_the_flipped_kernel():
    """The header's loops over (G, i, j, o) with w indexed flipped, against conv_ref.conv_ref(g, wT): the identity the device
    test repeats against dtfill_conv2d."""
    x, w, _, dy = _case(3, 2, 20, (1, 3, 4), 5)  # Cout = 20: two groups of the backward's chain
    y = np.random.default_rng(6).standard_normal(dy.shape).astype(F)
    g = RB.g_ref(dy, y, R.LEAKY, 0.2)
    R.assert_same(RB.dx_ref(dy, y, w, R.LEAKY, 0.2), _literal_dx(g, w), "dx")
    R.assert_same(R.conv_ref(g, RB.flipped(w)), _literal_dx(g, w), "conv_ref(g, wT)")


def test_the_two_level_order_is_told_apart():
    """A 1x1 kernel on one channel with x = 1 makes dw the sum of g in the contract's order.  Two frames of one row and two
    segments each, u = 2^-23 (the last place of 1):
      against one chain over the whole frame: 1 in segment 0, 0.5 u twice in segment 1.  The segment's partial is u and the sum
        1 + u; a single chain adds 0.5 u to 1 twice, each a tie that goes to even: 1.
      against the (s, t, b) order: frame 0 holds 1 in segment 0 and 0.75 u twice in segment 1 (the partial 1.5 u is exact),
        frame 1 holds u in segment 0.  (b, t, s): 1, + 1.5 u is a tie, to even: 1 + 2 u, + u = 1 + 3 u.  (s, t, b): 1, + u =
        1 + u, + 1.5 u = 1 + 2.5 u is a tie, to even: 1 + 2 u."""
    u = 2.0 ** -23
    dw = lambda g, **kw: RB.dw_ref(np.ones_like(g), g, None, 1, R.LINEAR, **kw)[0][0, 0, 0, 0]
    g = np.zeros((1, 1, 2 * COLS, 1), F)
    g[0, 0, 0, 0] = 1
    g[0, 0, COLS, 0] = g[0, 0, COLS + 1, 0] = 0.5 * u
    assert dw(g) == F(1 + u) and dw(g, rows=1, cols=2 * COLS) == F(1)
    g = np.zeros((2, 1, 2 * COLS, 1), F)
    g[0, 0, 0, 0] = 1
    g[0, 0, COLS, 0] = g[0, 0, COLS + 1, 0] = 0.75 * u
    g[1, 0, 0, 0] = u
    assert dw(g) == F(1 + 3 * u) and dw(g, order="stb") == F(1 + 2 * u)
    # the same between segment rows: t outside s
    g = np.zeros((1, 2 * ROWS, 2 * COLS, 1), F)
    g[0, 0, 0, 0], g[0, 0, COLS, 0], g[0, 0, COLS + 1, 0], g[0, ROWS, 0, 0] = 1, 0.75 * u, 0.75 * u, u
    assert dw(g) == F(1 + 3 * u) and dw(g, order="stb") == F(1 + 2 * u)
    assert [s[1:] for s in RB.segments(1, ROWS + 1, COLS + 1)] == [(0, ROWS, 0, COLS), (0, ROWS, COLS, COLS + 1),
                                                                   (ROWS, ROWS + 1, 0, COLS), (ROWS, ROWS + 1, COLS, COLS + 1)]
    assert [s[0] for s in RB.segments(2, 1, 1)] == [0, 1]


# ---- netgrad_ref against float64 autograd ---------------------------------------------------------------------------------

@pytest.mark.parametrize("joint_train", (False, True))
def test_netgrad_ref_against_float64_autograd(pkg, joint_train):
    """The same forward in float64 torch ops under the tape (F.conv2d, leaky_relu, gmc_grad_ref.torch_statement for the fill,
    train.py's loss expression), on a frame where no float32 rounding flips a compare (checked: the masks and the signs of every
    activation agree).  The net is a composition of chains, so its gradient's error is not one gamma: each variable's gradient
    is held to 1e-4 of its largest entry, four digits where float32 carries seven, which a wrong term (a missing second call
    of lidar_conv_extra_1, a wrong flip, a gradient that skips the fill) misses by orders of magnitude."""
    import importlib

    import torch
    import torch.nn.functional as TF

    import gmc_grad_ref

    net = importlib.import_module(pkg.__name__ + ".net")
    B, H, W = 2, 7, 12
    rng = np.random.default_rng(3)
    depth = rng.uniform(1, 80, (B, H, W))
    lidar = np.where(rng.random((B, H, W)) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random((B, H, W)) < 0.65, depth + rng.normal(0, 0.5, (B, H, W)), 0).astype(F)
    weights = net.glorot_weights(7, 4, True, bias=0.1)
    got, fw, stats = netgrad_ref.loss_gradients(lidar, gt, weights, joint_train=joint_train)

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    var = {n: (t(k).requires_grad_(True), t(b).requires_grad_(True)) for n, (k, b) in weights.items()}
    signs = []

    def conv(x, name, act):
        k, b = var[name]
        y = TF.conv2d(x, k.permute(3, 2, 0, 1), b, padding=k.shape[0] // 2)
        signs.append((name, (y.detach() > 0).permute(0, 2, 3, 1).numpy()))
        return TF.leaky_relu(y, float(F(0.2))) if act else y

    x = t(lidar)
    mask = (x > float(F(0.1))).double()
    c = (x / 90.0)[:, None]
    for name in ("correct_1", "correct_2", "correct_3"):
        c = conv(c, name, True)
    correct = conv(c, "correct_4", False)[:, 0] * mask
    fill_in = correct if joint_train else correct.detach()
    lidars = gmc_grad_ref.torch_statement(fill_in, mask, 7, 4)
    for a, b in zip(lidars, fw["lidars"]):
        assert np.array_equal(a.detach().numpy() > 0.001, b > F(0.001)) and np.allclose(a.detach().numpy(), b, rtol=1e-4, atol=1e-6)
    stems = [conv(l[:, None], name, True) for l, name in zip(lidars, ("lidar_conv", "lidar_conv_extra_1", "lidar_conv_extra_2", "lidar_conv_extra_1"))]
    z = torch.cat(stems, dim=1)
    for name in ("conv1a", "conv1b", "conv1c", "conv1d"):
        z = conv(z, name, True)
    pred, corr = conv(z, "conv_output", False)[:, 0] * 90.0, correct * 90.0
    g64 = t(gt)
    with_gt = g64 > float(F(0.1))
    with_in = with_gt & (x > float(F(0.1)))
    total = ((pred - g64) ** 2 * with_gt).sum() / with_gt.sum() + \
        ((corr - g64) ** 2 * with_in + (corr - g64).abs() * with_in).sum() / with_in.sum()
    total.backward()
    # the float32 forward took every branch the float64 one took
    for name, calls in fw["tape"].items():
        mine = [s for n, s in signs if n == name]
        for (xin, y, act), s in zip(calls, mine):
            if act == R.LEAKY:
                assert np.array_equal(y > 0, s), name
    assert set(got) == set(net.layer_shapes(4, True))
    for name, (dw, db) in got.items():
        for mine, want in ((dw, var[name][0].grad.numpy()), (db, var[name][1].grad.numpy())):
            scale = np.abs(want).max()
            assert scale > 0 and np.abs(mine - want).max() <= 1e-4 * scale, (name, np.abs(mine - want).max() / scale)


# ---- the entry points, without a device ------------------------------------------------------------------------------------

GOOD = dict(x=1, dy=1, dy_channels=16, dy_offset=0, y=1, y_channels=16, y_offset=0, w=1, B=1, H=4, W=4, Cin=16, ksize=3, Cout=16,
            act=1, alpha=0.2, dx=1, dx_channels=16, dx_offset=0, dw=1, db=1, ws=1, ws_bytes=None)
DATA = ("dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "w", "B", "H", "W", "Cin", "ksize", "Cout", "act", "alpha",
        "dx", "dx_channels", "dx_offset", "ws", "ws_bytes")
WEIGHTS = ("x", "dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "B", "H", "W", "Cin", "ksize", "Cout", "act", "alpha",
           "dw", "db", "ws", "ws_bytes")
POINTERS = ("x", "dy", "y", "w", "dx", "dw", "db")


def _call(L, which, **change):
    a = dict(GOOD, **change)
    buf = ctypes.create_string_buffer(1024)  # never read: every call here returns before any HIP call
    base = ctypes.addressof(buf)
    base += (-base) % 256
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.dtfill_conv2d_backward_workspace_bytes(a["B"], a["H"], a["W"], a["Cin"], a["ksize"], a["Cout"]) or 1 << 20
    val = lambda k: (base if a[k] else None) if k in POINTERS else (base + (a[k] if a[k] > 1 else 0) if a[k] else None) if k == "ws" else a[k]
    fn, order = (L.dtfill_conv2d_backward_data, DATA) if which == "data" else (L.dtfill_conv2d_backward_weights, WEIGHTS)
    return fn(*[val(k) for k in order], None)


def test_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    NULL, SHAPE, WORKSPACE = -1, -2, -3
    for which, names in (("data", ("dy", "y", "w", "dx", "ws")), ("weights", ("x", "dy", "y", "dw", "ws"))):
        for name in names:
            assert _call(L, which, **{name: 0}) == NULL, (which, name)
        bad = [dict(ksize=k) for k in (0, 2, 4, 9, -1)] + [dict(Cin=c) for c in (0, 2, 8, 17, 24, 80, -16)] + \
            [dict(Cout=c, dy_channels=64, y_channels=64) for c in (0, 2, 8, 32)] + \
            [dict(dy_offset=-1), dict(dy_offset=1), dict(dy_channels=15), dict(dy_channels=0), dict(y_offset=-1), dict(y_offset=1),
             dict(y_channels=15), dict(dy_offset=2 ** 31 - 1), dict(Cout=1, dy_channels=4, dy_offset=4)] + \
            [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 15, H=1 << 8, W=1 << 8), dict(B=1 << 9, H=1 << 9, W=1 << 9),
             dict(B=1, H=1 << 13, W=1 << 13, dy_channels=32), dict(B=1, H=1 << 13, W=1 << 12, Cin=64)] + \
            [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-0.2), dict(alpha=-1e-30)]
        if which == "data":
            bad += [dict(dx_offset=-1), dict(dx_offset=1), dict(dx_channels=15), dict(dx_channels=0),
                    dict(B=1, H=1 << 13, W=1 << 13, dx_channels=32)]
        for change in bad:
            assert _call(L, which, ws_bytes=1 << 40, **change) == SHAPE, (which, change)
        assert _call(L, which, dy=0, ksize=2) == NULL  # the pointers first, as everywhere in the ABI
        # y is not needed, and not looked at, for a linear layer; alpha = 0 (a ReLU) is in the domain
        assert _call(L, which, act=0, y=0, y_channels=0, y_offset=-5, ws_bytes=0) == WORKSPACE
        assert _call(L, which, alpha=0.0, ws_bytes=0) == WORKSPACE
        assert _call(L, which, ws_bytes=L.dtfill_conv2d_backward_workspace_bytes(1, 4, 4, 16, 3, 16) - 1) == WORKSPACE
        assert _call(L, which, ws=16) == WORKSPACE  # not 256-byte aligned
        assert _call(L, which, db=0, ws_bytes=0) == WORKSPACE  # (a NULL db is allowed)


def test_the_workspace_rule(pkg):
    """Pure host arithmetic: the larger of g and wT (the data gradient) and the segments' partials (the weights'), each part
    rounded up to 256 bytes; 0 outside the domain."""
    pkg.build()
    ws = pkg.load().dtfill_conv2d_backward_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    for B, H, W, cin, ksize, cout in ((1, 1, 1, 1, 1, 1), (4, 256, 1216, 64, 7, 16), (4, 256, 1216, 16, 3, 1), (2, ROWS + 1, COLS + 1, 1, 7, 16),
                                      (1, ROWS, COLS, 48, 7, 16), (3, 5, 2 * COLS, 16, 5, 16), (1, 3000, 3000, 64, 1, 16)):
        nseg = B * -(-H // ROWS) * -(-W // COLS)
        data = up(4 * B * H * W * cout) + up(4 * ksize * ksize * cin * cout)
        weights = up(4 * nseg * (ksize * ksize * cin + 1) * cout)
        assert ws(B, H, W, cin, ksize, cout) == max(data, weights), (B, H, W, cin, ksize, cout)
    assert ws(4, 256, 1216, 64, 7, 16) == up(4 * 608 * 3137 * 16)  # the KITTI crop's largest layer: 122 MB of partials
    for bad in ((0, 4, 4, 16, 3, 16), (1, 0, 4, 16, 3, 16), (1, 4, -1, 16, 3, 16), (1, 4, 4, 8, 3, 16), (1, 4, 4, 16, 2, 16),
                (1, 4, 4, 16, 3, 32), (1, 1 << 13, 1 << 12, 64, 3, 16), (1 << 11, 1 << 10, 1 << 10, 1, 3, 16)):
        assert ws(*bad) == 0, bad


def test_binding_and_constants(pkg):
    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    consts = dict(re.findall(r"\b(DTFILL_CONV_BW_\w+)\s*=\s*(\d+)", src))
    assert consts == {"DTFILL_CONV_BW_ROWS": str(ROWS), "DTFILL_CONV_BW_COLS": str(COLS)}
    assert (pkg._lib.CONV_BW_ROWS, pkg._lib.CONV_BW_COLS) == (ROWS, COLS)
    assert ROWS % 4 == 0 and COLS % 4 == 0  # whole strips of whole matrix-core k-steps
    pkg.build()
    L = pkg.load()
    assert len(L.dtfill_conv2d_backward_data.argtypes) == 21 and len(L.dtfill_conv2d_backward_weights.argtypes) == 20
    assert L.dtfill_conv2d_backward_workspace_bytes.restype is ctypes.c_size_t
    assert re.search(r"#define DTFILL_ABI_VERSION 1\b", src) and L.dtfill_abi_version() == 1


def test_python_layer_argument_checks_without_gpu(pkg):
    import importlib

    import torch

    dev = pkg.device
    dy, w, x = torch.zeros((1, 4, 4, 16)), torch.zeros((3, 3, 16, 16)), torch.zeros((1, 4, 4, 16))
    with pytest.raises(ValueError, match="act must be"):
        dev.conv2d_backward_data_device(dy, w, dy, act="relu")
    with pytest.raises(ValueError, match="alpha"):
        dev.conv2d_backward_data_device(dy, w, dy, act="leaky", alpha=-0.5)
    with pytest.raises(ValueError, match="alpha"):
        pkg.autograd.conv2d(x, w, act="leaky", alpha=float("nan"))
    # host tensors where device tensors are asked for are refused before any device work
    for call in (lambda: dev.conv2d_backward_data_device(dy, w, dy, "leaky"), lambda: dev.conv2d_backward_weights_device(x, dy, 3),
                 lambda: pkg.autograd.conv2d(x, w)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    assert dev.conv2d_backward_workspace_bytes(1, 4, 4, 16, 3, 16) == pkg.load().dtfill_conv2d_backward_workspace_bytes(1, 4, 4, 16, 3, 16)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_backward_workspace_bytes(1, 4, 4, 8, 3, 16)
    # the trainable network checks its weights as the inference class does, on the host
    net = importlib.import_module(pkg.__name__ + ".net")
    weights = net.glorot_weights(1, 4, True)
    model = net.SparsityCNNTrainable(weights, joint_train=True)
    assert isinstance(model, torch.nn.Module) and model.joint_train and len(list(model.parameters())) == 2 * len(net.layer_shapes(4, True))
    assert tuple(model.conv1a.kernel.shape) == (7, 7, 64, 16) and not hasattr(model, "lidar_conv_extra_3")
    assert set(model.state_dict()) == {"%s.%s" % (n, v) for n in net.layer_shapes(4, True) for v in ("kernel", "bias")}
    with pytest.raises(ValueError):
        net.SparsityCNNTrainable({k: v for k, v in weights.items() if k != "conv1b"})
    with pytest.raises(ValueError):
        net.SparsityCNNTrainable(weights, scale_num=5)

"""The backward of dtfill_conv2d_strided and dtfill_conv2d_transpose without a device: the numpy statement of the contracts
(tests/conv2b_ref.py) against float64 autograd within bounds derived from the chain lengths, the identities that tie it to the
forward statements and to convb_ref, what the statement pins (which pixel meets which tap at stride 2 and in the transposed form,
the +0 of the 1x1 stride-2 spread, the transposed db's four chains, dresidual), and everything of the five entry points that needs
no GPU (return codes, the workspace rule, the binding)."""
import ctypes
import os
import re

import numpy as np
import pytest

import conv2_ref as R2
import conv2b_ref as RW
import conv_ref as R
import convb_ref as RB

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
U = 2.0 ** -24
with_g = lambda n: R.gamma(n) * (1 + U) + U  # a chain of n roundings over g, itself one rounded product (test_conv2d_backward)


def _case(ksize, cin, cout, in_shape, out_shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(in_shape + (cin,)) * 2.0 ** rng.integers(-3, 4, in_shape + (cin,))).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    dy = (rng.standard_normal(out_shape + (cout,)) * 2.0 ** rng.integers(-3, 4, out_shape + (cout,))).astype(F)
    return x, w, rng.standard_normal(cout).astype(F), dy


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _conv64(tx, tw, tb, ksize, stride):
    """conv2_ref.strided_f64's construction under the tape: NCHW tensors, the 'same' rule's explicit padding."""
    import torch.nn.functional as TF

    (_, pt, pb), (_, pl, pr) = R2.same_rule(tx.shape[2], ksize, stride), R2.same_rule(tx.shape[3], ksize, stride)
    return TF.conv2d(TF.pad(tx, (pl, pr, pt, pb)), tw, tb, stride=stride)


def _vjp(f, at, cotangent):
    import torch

    at = at.clone().requires_grad_(True)
    return torch.autograd.grad(f(at), at, cotangent)[0]


# ---- against float64 autograd --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize,stride,cin,cout,act", ((3, 1, 16, 32, R.LEAKY), (3, 2, 32, 16, R.LEAKY), (1, 2, 16, 32, R.LEAKY),
                                                        (1, 1, 16, 16, R.LINEAR), (5, 1, 16, 16, R.LEAKY)))
def test_strided_against_float64_autograd(ksize, stride, cin, cout, act):
    """The float64 forward is conv2_ref.strided_f64 (checked), differentiated by torch's tape.  y is that forward rounded to
    float32, so both sides take the same branch.  The bounds, from the chain lengths:
      dx  stride 1: K = ksize^2 Cout links; stride 2, 3x3: at most 4 taps an output, K = 4 Cout; 1x1: K = Cout
      dw  level 1 at most n1 = min(R C, Ho Wo) links, level 2 adds S partials: n1 + S roundings; db the same with |x| = 1
    each times the sum of the absolute products, worked out by the same float64 graph on absolute values, with g's own
    rounding passed through (with_g)."""
    import torch

    B, Ho, Wo = (2, ROWS + 1, COLS + 3) if ksize * ksize * cin * cout <= 9 * 16 * 32 else (2, 5, 7)
    x, w, bias, dy = _case(ksize, cin, cout, (B, stride * Ho, stride * Wo), (B, Ho, Wo), 7 * ksize + stride)
    alpha = float(F(0.2))
    tx, tw, tb = _t(x).permute(0, 3, 1, 2), _t(w).permute(3, 2, 0, 1).contiguous(), _t(bias)
    fwd = lambda vx, vw, vb: _conv64(vx, vw, vb, ksize, stride)
    y64 = fwd(tx, tw, tb).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(y64, R2.strided_f64(x, w, bias, stride))
    y = (np.where(y64 > 0, y64, y64 * alpha) if act == R.LEAKY else y64).astype(F)
    assert (y != 0).all()
    g64 = np.where(y > 0, dy.astype(np.float64), dy.astype(np.float64) * alpha) if act == R.LEAKY else dy.astype(np.float64)
    tg, tag = _t(g64).permute(0, 3, 1, 2), _t(np.abs(g64)).permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    khwio = lambda t: t.permute(2, 3, 1, 0).numpy()

    dx = RW.strided_dx_ref(dy, y, w, stride, act, 0.2)
    want = nhwc(_vjp(lambda v: fwd(v, tw, None), tx, tg))
    scale = nhwc(_vjp(lambda v: fwd(v, tw.abs(), None), tx, tag))
    K = ksize * ksize * cout if stride == 1 else (4 if ksize == 3 else 1) * cout
    assert (np.abs(dx - want) <= with_g(K) * scale).all() and np.abs(want).max() > 0

    dw, db = RW.strided_dw_ref(x, dy, y, ksize, stride, act, 0.2)
    n = min(ROWS * COLS, Ho * Wo) + len(RB.segments(B, Ho, Wo))
    want = khwio(_vjp(lambda v: fwd(tx, v, None), tw, tg))
    scale = khwio(_vjp(lambda v: fwd(tx.abs(), v, None), tw, tag))
    assert dw.shape == want.shape and (np.abs(dw - want) <= with_g(n) * scale).all() and np.abs(want).max() > 0
    assert (np.abs(db - g64.sum(axis=(0, 1, 2))) <= with_g(n) * np.abs(g64).sum(axis=(0, 1, 2))).all()


def test_transposed_against_float64_autograd():
    """The float64 forward is the definition, conv2_ref.transpose_f64_vjp (checked against the tape's own forward here), under
    the Keras kernel [3,3,Cout,Cin].  dx: K = 9 Cout links.  dw: n1 + S roundings over the INPUT frame's segments; db: the four
    chains add three more roundings, n1 + S + 3."""
    import torch
    import torch.nn.functional as TF

    cin, cout, act = 32, 16, R.LEAKY
    B, H, W = 2, ROWS + 1, COLS + 3
    x, w, bias, dy = _case(3, cin, cout, (B, H, W), (B, 2 * H, 2 * W), 5)  # w: the packed [3,3,Cin,Cout]
    kernel = np.ascontiguousarray(w.transpose(0, 1, 3, 2))  # Keras's [3,3,Cout,Cin]
    alpha = float(F(0.2))
    tx, tk = _t(x).permute(0, 3, 1, 2), _t(kernel).permute(3, 2, 0, 1).contiguous()  # tk: [Cin, Cout, 3, 3]
    fwd = lambda vx, vk: TF.conv_transpose2d(vx, vk, stride=2)[:, :, :2 * H, :2 * W]
    y64 = fwd(tx, tk).permute(0, 2, 3, 1).numpy() + bias.astype(np.float64)
    assert np.allclose(y64, R2.transpose_f64_vjp(x, kernel, bias), rtol=1e-12, atol=1e-12)
    y = np.where(y64 > 0, y64, y64 * alpha).astype(F)
    assert (y != 0).all()
    g64 = np.where(y > 0, dy.astype(np.float64), dy.astype(np.float64) * alpha)
    tg, tag = _t(g64).permute(0, 3, 1, 2), _t(np.abs(g64)).permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    packed = lambda t: t.permute(2, 3, 0, 1).numpy()  # [Cin, Cout, 3, 3] -> [3, 3, Cin, Cout]

    dx = RW.transpose_dx_ref(dy, y, w, act, 0.2)
    want, scale = nhwc(_vjp(lambda v: fwd(v, tk), tx, tg)), nhwc(_vjp(lambda v: fwd(v, tk.abs()), tx, tag))
    assert (np.abs(dx - want) <= with_g(9 * cout) * scale).all() and np.abs(want).max() > 0
    dw, db = RW.transpose_dw_ref(x, dy, y, act, 0.2)
    n = min(ROWS * COLS, H * W) + len(RB.segments(B, H, W))
    want, scale = packed(_vjp(lambda v: fwd(tx, v), tk, tg)), packed(_vjp(lambda v: fwd(tx.abs(), v), tk, tag))
    assert dw.shape == want.shape and (np.abs(dw - want) <= with_g(n) * scale).all() and np.abs(want).max() > 0
    assert (np.abs(db - g64.sum(axis=(0, 1, 2))) <= with_g(n + 3) * np.abs(g64).sum(axis=(0, 1, 2))).all()


# ---- the identities --------------------------------------------------------------------------------------------------------

def test_the_identities():
    x, w, _, dy = _case(3, 16, 32, (2, 10, 14), (2, 5, 7), 3)
    y = np.random.default_rng(4).standard_normal(dy.shape).astype(F)
    g = RW.g_ref(dy, y, R.LEAKY)
    R.assert_same(RW.strided_dx_ref(dy, y, w, 2, R.LEAKY), R2.transpose_ref(g, RW.exchanged(w)), "stride 2, 3x3")
    assert RW.exchanged(w).shape == (3, 3, 32, 16) and RW.exchanged(w)[0, 2, 5, 3] == w[0, 2, 3, 5]  # exchanged, not flipped
    xt, wt, _, dyt = _case(3, 16, 32, (2, 5, 7), (2, 10, 14), 6)
    yt = np.random.default_rng(7).standard_normal(dyt.shape).astype(F)
    R.assert_same(RW.transpose_dx_ref(dyt, yt, wt, R.LEAKY), R2.strided_ref(RW.g_ref(dyt, yt, R.LEAKY), RW.exchanged(wt), stride=2),
                  "transposed")
    # stride 1, Cout == 16: the bits of convb_ref, over several segments
    x, w, _, dy = _case(3, 16, 16, (2, ROWS + 1, COLS + 3), (2, ROWS + 1, COLS + 3), 8)
    y = np.random.default_rng(9).standard_normal(dy.shape).astype(F)
    got, want = RW.strided_dw_ref(x, dy, y, 3, 1, R.LEAKY), RB.dw_ref(x, dy, y, 3, R.LEAKY)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    R.assert_same(RW.strided_dx_ref(dy, y, w, 1, R.LEAKY), RB.dx_ref(dy, y, w, R.LEAKY), "stride 1 dx")


# ---- what the statement pins -----------------------------------------------------------------------------------------------

def test_which_pixel_meets_which_tap_at_stride_two():
    """A 4 x 4 input, 3x3, stride 2, one channel each way: output (h, v) reads x[2 h + i, 2 v + j] (pt = pl = 0), index 4 is the
    padding.  dy one-hot at (1, 1): dw[i, j] = x[2 + i, 2 + j] inside, +0 on the padding row and column; dx has w[i, j] at
    (2 + i, 2 + j)."""
    x = np.arange(1, 17, dtype=F).reshape(1, 4, 4, 1)
    w = np.arange(10, 19, dtype=F).reshape(3, 3, 1, 1)
    dy = np.zeros((1, 2, 2, 1), F)
    dy[0, 1, 1, 0] = 1
    dw, db = RW.strided_dw_ref(x, dy, None, 3, 2, R.LINEAR)
    want = np.zeros((3, 3), F)
    want[:2, :2] = x[0, 2:, 2:, 0]
    assert (dw[:, :, 0, 0] == want).all() and db[0] == 1
    dx = RW.strided_dx_ref(dy, None, w, 2, R.LINEAR)
    want = np.zeros((4, 4), F)
    want[2:, 2:] = w[:2, :2, 0, 0]
    assert (dx[0, :, :, 0] == want).all()
    dy[:] = 0
    dy[0, 0, 0, 0] = 1  # the window of output (0, 0) lies inside: every tap meets a pixel
    dw, _ = RW.strided_dw_ref(x, dy, None, 3, 2, R.LINEAR)
    assert (dw[:, :, 0, 0] == x[0, :3, :3, 0]).all()
    # 1x1 at stride 2: output (h, v) reads x[2 h, 2 v] alone
    dy = np.arange(1, 5, dtype=F).reshape(1, 2, 2, 1)
    dw, db = RW.strided_dw_ref(x, dy, None, 1, 2, R.LINEAR)
    assert dw[0, 0, 0, 0] == (x[0, ::2, ::2, 0] * dy[0, :, :, 0]).sum() and db[0] == 10


def test_which_pixel_meets_which_tap_in_the_transposed_form():
    """Input 2 x 2, output 4 x 4: x[h, v] reaches y[2 h + ky, 2 v + kx] under tap (ky, kx).  x one-hot at (1, 1): dw[ky, kx] =
    g[2 + ky, 2 + kx] inside [4, 4], +0 at row and column 4.  dy one-hot at (2, 3) = (2 * 1 + 0, 2 * 1 + 1): dx[1, 1] = w[0, 1],
    and x[0, 1] reaches it under tap (2, 1)."""
    x = np.zeros((1, 2, 2, 1), F)
    x[0, 1, 1, 0] = 1
    g = np.arange(1, 17, dtype=F).reshape(1, 4, 4, 1)
    dw, db = RW.transpose_dw_ref(x, g, None, R.LINEAR)
    want = np.zeros((3, 3), F)
    want[:2, :2] = g[0, 2:, 2:, 0]
    assert (dw[:, :, 0, 0] == want).all() and db[0] == g.sum()
    w = np.arange(10, 19, dtype=F).reshape(3, 3, 1, 1)
    dy = np.zeros((1, 4, 4, 1), F)
    dy[0, 2, 3, 0] = 1
    dx = RW.transpose_dx_ref(dy, None, w, R.LINEAR)
    want = np.zeros((2, 2), F)
    want[1, 1], want[0, 1] = w[0, 1, 0, 0], w[2, 1, 0, 0]
    assert (dx[0, :, :, 0] == want).all()
    # and it is the transpose of the forward: <transpose_ref(x), dy> = <x, dx> on small integers, exactly
    rng = np.random.default_rng(2)
    x = rng.integers(-3, 4, (1, 3, 2, 2)).astype(F)
    w = rng.integers(-3, 4, (3, 3, 2, 3)).astype(F)
    dy = rng.integers(-3, 4, (1, 6, 4, 3)).astype(F)
    assert (R2.transpose_ref(x, w) * dy).sum() == (x * RW.transpose_dx_ref(dy, None, w, R.LINEAR)).sum()
    assert (R2.transpose_ref(x, w) * dy).sum() == (w * RW.transpose_dw_ref(x, dy, None, R.LINEAR)[0]).sum()


def test_the_one_by_one_stride_two_dx_is_plus_zero_off_the_even_grid():
    x, w, _, dy = _case(1, 16, 32, (1, 6, 10), (1, 3, 5), 1)
    dy[0, 1, 2, 0], dy[0, 2, 4, 3] = np.inf, np.nan
    dx = RW.strided_dx_ref(dy, None, w, 2, R.LINEAR)
    off = np.ones((6, 10), bool)
    off[::2, ::2] = False
    assert (dx[0][off].view(np.uint32) == 0).all()  # +0 bit for bit, beside an infinite and a NaN g
    assert np.isinf(dx[0, 2, 4]).any() and np.isnan(dx[0, 4, 8]).all() and np.isfinite(dx[0, 0, 0]).all()
    # a zero-padded 3x3 kernel is NOT the contract: the transposed chain under it multiplies the infinite g by a zero weight
    w3 = np.zeros((3, 3, 16, 32), F)
    w3[0, 0] = w[0, 0]
    assert np.isnan(R2.transpose_ref(RW.g_ref(dy, None, R.LINEAR), RW.exchanged(w3))[0][off]).any()
    R.assert_same(dx[:, ::2, ::2], R2.strided_ref(dy, RW.exchanged(w)), "the even grid: a chain over o")


def test_the_transposed_db_counts_every_output_pixel_once_in_four_chains():
    """g = 1 everywhere: db = B 2H 2W exactly.  The order: u = 2^-23; one input row of two pixels, so an output of 2 x 4.  Output
    row 0 = [1, 0.5 u, 0.5 u, 0], row 1 = 0.  The four chains: q00 over columns 0 and 2 = 1 + 0.5 u, a tie, to even: 1;
    q01 over columns 1 and 3 = 0.5 u; (q00 + q01) = 1 + 0.5 u -> 1.  One raster chain over the row adds 0.5 u to 1 twice: 1 as
    well; so take [1, 0.75 u, 0.75 u, 0]: q00 = 1 + 0.75 u -> 1 + u, q01 = 0.75 u, sum 1 + 1.75 u -> 1 + 2 u; the raster chain:
    1 + 0.75 u -> 1 + u, + 0.75 u = 1 + 1.75 u -> 1 + 2 u.  They part at [1, 0.5 u, 0.25 u, 0.25 u]: four chains q00 = 1 +
    0.25 u -> 1, q01 = 0.75 u, sum 1 + 0.75 u -> 1 + u; raster: 1 + 0.5 u -> 1 (tie to even), + 0.25 u -> 1, + 0.25 u -> 1."""
    x = np.zeros((2, 3, 5, 1), F)
    db = RW.transpose_dw_ref(x, np.ones((2, 6, 10, 2), F), None, R.LINEAR)[1]
    assert (db == 2 * 6 * 10).all()
    u = 2.0 ** -23
    g = np.zeros((1, 2, 4, 1), F)
    g[0, 0, :, 0] = [1, 0.5 * u, 0.25 * u, 0.25 * u]
    x = np.zeros((1, 1, 2, 1), F)
    assert RW.transpose_dw_ref(x, g, None, R.LINEAR)[1][0] == F(1 + u)
    assert RW.transpose_dw_ref(x, g, None, R.LINEAR, db_chains=1)[1][0] == F(1)


def test_dresidual_is_g():
    dy = np.full((1, 1, 6, 1), 3, F)
    y = F([2, 0.0, -0.0, -1, np.nan, np.inf]).reshape(1, 1, 6, 1)
    slope = F(3) * F(0.2)
    assert (RW.g_ref(dy, y, R.LEAKY, 0.2).reshape(-1) == F([3, slope, slope, slope, slope, 3])).all()  # +-0 and NaN: the alpha branch
    assert RW.g_ref is RB.g_ref


# ---- the entry points, without a device ------------------------------------------------------------------------------------

GOOD = dict(x=1, dy=1, dy_channels=16, dy_offset=0, y=1, y_channels=16, y_offset=0, w=1, B=1, H=4, W=4, Cin=16, ksize=3, Cout=16, stride=1,
            act=1, alpha=0.2, dx=1, dx_channels=16, dx_offset=0, dres=1, dw=1, db=1, ws=1, ws_bytes=None)
ORDER = {
    "strided_data": ("dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "w", "B", "H", "W", "Cin", "ksize", "Cout", "stride",
                     "act", "alpha", "dx", "dx_channels", "dx_offset", "dres", "ws", "ws_bytes"),
    "strided_weights": ("x", "dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "B", "H", "W", "Cin", "ksize", "Cout", "stride",
                        "act", "alpha", "dw", "db", "ws", "ws_bytes"),
    "transpose_data": ("dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "w", "B", "H", "W", "Cin", "Cout", "act", "alpha",
                       "dx", "dx_channels", "dx_offset", "ws", "ws_bytes"),
    "transpose_weights": ("x", "dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "B", "H", "W", "Cin", "Cout", "act", "alpha",
                          "dw", "db", "ws", "ws_bytes"),
}
POINTERS = ("x", "dy", "y", "w", "dx", "dres", "dw", "db")


def _call(L, which, **change):
    a = dict(GOOD, **change)
    transposed = which.startswith("transpose")
    if transposed:
        a.update(ksize=3, stride=2)
    buf = ctypes.create_string_buffer(1024)  # never read: every call here returns before any HIP call
    base = ctypes.addressof(buf)
    base += (-base) % 256
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.dtfill_conv2d_wide_backward_workspace_bytes(a["B"], a["H"], a["W"], a["Cin"], a["ksize"], a["Cout"], a["stride"],
                                                                      int(transposed)) or 1 << 20
    val = lambda k: (base if a[k] else None) if k in POINTERS else (base + (a[k] if a[k] > 1 else 0) if a[k] else None) if k == "ws" else a[k]
    fn = getattr(L, "dtfill_conv2d_%s_backward_%s" % tuple(which.split("_")))
    return fn(*[val(k) for k in ORDER[which]], None)


def test_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    NULL, SHAPE, WORKSPACE = -1, -2, -3
    for which in ORDER:
        data, transposed = which.endswith("data"), which.startswith("transpose")
        for name in ("dy", "y", "w", "dx", "ws") if data else ("x", "dy", "y", "dw", "ws"):
            assert _call(L, which, **{name: 0}) == NULL, (which, name)
        bad = [dict(Cin=c) for c in (0, 1, 8, 17, 24, -16)] + [dict(Cout=c, dy_channels=64, y_channels=64) for c in (0, 1, 2, 8, 24)] + \
            [dict(dy_offset=-1), dict(dy_offset=1), dict(dy_channels=15), dict(dy_channels=0), dict(y_offset=-1), dict(y_offset=1),
             dict(y_channels=15), dict(dy_offset=2 ** 31 - 1)] + \
            [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 9, H=1 << 9, W=1 << 9), dict(B=1, H=1 << 12, W=1 << 12, Cin=128),
             dict(B=1, H=1 << 12, W=1 << 12, Cout=128, dy_channels=128, y_channels=128), dict(B=1, H=1 << 12, W=1 << 12, dy_channels=128)] + \
            [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-0.2), dict(alpha=-1e-30)] + \
            [dict(Cin=1 << 14, Cout=1 << 14, dy_channels=1 << 14, y_channels=1 << 14)]  # (ksize^2 Cin + 1) Cout >= 2^31
        if not transposed:
            bad += [dict(ksize=k) for k in (0, 2, 4, 9, -1)] + [dict(stride=s) for s in (0, 3, -1)] + \
                [dict(stride=2, ksize=5), dict(stride=2, ksize=7), dict(stride=2, H=5), dict(stride=2, W=3), dict(stride=2, ksize=1, H=1, W=1)]
        if data:
            bad += [dict(dx_offset=-1), dict(dx_offset=1), dict(dx_channels=15), dict(dx_channels=0), dict(B=1, H=1 << 12, W=1 << 12, dx_channels=128)]
        for change in bad:
            assert _call(L, which, ws_bytes=1 << 40, **change) == SHAPE, (which, change)
        assert _call(L, which, dy=0, Cin=8) == NULL  # the pointers first, as everywhere in the ABI
        # y is not needed, and not looked at, for a linear layer; alpha = 0 (a ReLU) is in the domain
        assert _call(L, which, act=0, y=0, y_channels=0, y_offset=-5, ws_bytes=0) == WORKSPACE
        assert _call(L, which, alpha=0.0, ws_bytes=0) == WORKSPACE
        full = L.dtfill_conv2d_wide_backward_workspace_bytes(1, 4, 4, 16, 3, 16, 2 if transposed else 1, int(transposed))
        assert full > 0 and _call(L, which, ws_bytes=full - 1) == WORKSPACE
        assert _call(L, which, ws=16) == WORKSPACE  # not 256-byte aligned
        assert _call(L, which, **({"dres": 0} if which == "strided_data" else {} if data else {"db": 0}), ws_bytes=0) == WORKSPACE  # nullable
    # an even frame at stride 2 is in the domain, for both kernel sizes
    for k in (1, 3):
        assert _call(L, "strided_data", stride=2, ksize=k, ws_bytes=0) == WORKSPACE
        assert _call(L, "strided_weights", stride=2, ksize=k, ws_bytes=0) == WORKSPACE


def test_the_workspace_rule(pkg):
    """Pure host arithmetic: the larger of g, the repacked weights and (1x1 at stride 2) the chain's values before the spread (the
    data gradient) and the segments' partials (the weights'), each part rounded up to 256 bytes; 0 outside the domain."""
    pkg.build()
    ws = pkg.load().dtfill_conv2d_wide_backward_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    nseg = lambda B, H, W: B * -(-H // ROWS) * -(-W // COLS)
    for B, H, W, cin, k, cout, stride in ((1, 1, 1, 16, 1, 16, 1), (4, 256, 1216, 128, 3, 64, 1), (4, 128, 608, 64, 3, 128, 2),
                                          (2, 66, 130, 48, 1, 80, 2), (4, 32, 152, 512, 3, 512, 1), (1, ROWS, COLS, 16, 7, 32, 1)):
        Ho, Wo = H // stride, W // stride
        data = up(4 * B * Ho * Wo * cout) + up(4 * k * k * cin * cout) + (up(4 * B * Ho * Wo * cin) if (stride, k) == (2, 1) else 0)
        weights = up(4 * nseg(B, Ho, Wo) * (k * k * cin + 1) * cout)
        assert ws(B, H, W, cin, k, cout, stride, 0) == max(data, weights), (B, H, W, cin, k, cout, stride)
    for B, H, W, cin, cout in ((1, 1, 1, 16, 16), (4, 32, 152, 512, 256), (2, 33, 65, 48, 80)):
        data = up(4 * B * 4 * H * W * cout) + up(4 * 9 * cin * cout)
        assert ws(B, H, W, cin, 3, cout, 2, 1) == max(data, up(4 * nseg(B, H, W) * (9 * cin + 1) * cout))
    # the KITTI crop at B = 4: the largest partials are upsample_1_post's, 179 MB; the call's workspace is its g, 319 MB
    assert up(4 * 608 * (9 * 128 + 1) * 64) == 179_462_144
    assert ws(4, 256, 1216, 128, 3, 64, 1, 0) == up(4 * 4 * 256 * 1216 * 64) + up(4 * 9 * 128 * 64) == 319_062_016
    for bad in ((0, 4, 4, 16, 3, 16, 1, 0), (1, 4, 4, 8, 3, 16, 1, 0), (1, 4, 4, 16, 2, 16, 1, 0), (1, 4, 4, 16, 3, 24, 1, 0),
                (1, 5, 4, 16, 3, 16, 2, 0), (1, 4, 4, 16, 5, 16, 2, 0), (1, 4, 4, 16, 3, 16, 3, 0), (1, 4, 4, 16, 1, 16, 2, 1),
                (1, 4, 4, 16, 3, 16, 1, 1), (1, 1 << 13, 1 << 12, 64, 3, 16, 1, 0), (1, 1 << 12, 1 << 12, 16, 3, 64, 2, 1)):
        assert ws(*bad) == 0, bad


def test_binding(pkg):
    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    pkg.build()
    L = pkg.load()
    counts = {"strided_backward_data": 23, "strided_backward_weights": 21, "transpose_backward_data": 20, "transpose_backward_weights": 19}
    for name, n in counts.items():
        assert len(getattr(L, "dtfill_conv2d_" + name).argtypes) == n and ("dtfill_conv2d_%s(" % name) in src, name
    assert L.dtfill_conv2d_wide_backward_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.dtfill_conv2d_wide_backward_workspace_bytes.argtypes) == 8
    assert pkg._lib.SYMBOLS.index("dtfill_conv2d_wide_backward_workspace_bytes") == pkg._lib.SYMBOLS.index("dtfill_conv2d_backward_weights") + 1


def test_python_layer_argument_checks_without_gpu(pkg):
    import torch

    dev = pkg.device
    dy, w, x = torch.zeros((1, 4, 4, 16)), torch.zeros((3, 3, 16, 16)), torch.zeros((1, 4, 4, 16))
    with pytest.raises(ValueError, match="act must be"):
        dev.conv2d_strided_backward_data_device(dy, w, 1, dy, act="relu")
    with pytest.raises(ValueError, match="alpha"):
        dev.conv2d_transpose_backward_data_device(dy, w, dy, act="leaky", alpha=-0.5)
    with pytest.raises(ValueError, match="alpha"):
        pkg.autograd.conv2d_strided(x, w, act="leaky", alpha=float("nan"))
    with pytest.raises(ValueError, match="alpha"):
        pkg.autograd.conv2d_transpose(x, w, act="leaky", alpha=-1.0)
    for call in (lambda: dev.conv2d_strided_backward_data_device(dy, w, 1, dy, "leaky"),
                 lambda: dev.conv2d_strided_backward_weights_device(x, dy, 3), lambda: dev.conv2d_transpose_backward_weights_device(x, dy),
                 lambda: pkg.autograd.conv2d_strided(x, w), lambda: pkg.autograd.conv2d_transpose(x, w)):
        with pytest.raises((ValueError, RuntimeError)):  # host tensors are refused before any device work
            call()
    assert dev.conv2d_wide_backward_workspace_bytes(1, 4, 4, 16, 3, 16, 2) == pkg.load().dtfill_conv2d_wide_backward_workspace_bytes(1, 4, 4, 16, 3, 16, 2, 0)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_wide_backward_workspace_bytes(1, 5, 4, 16, 3, 16, 2)

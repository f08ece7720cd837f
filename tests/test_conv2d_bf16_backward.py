"""The bf16 backward of the wide layers without a device: the numpy statement of its contracts (tests/convb_bf16_ref.py) against
float64 torch autograd of the convolution over the rounded operands and against an int64 reference, every return code and the
workspace function through the ABI (the float32 twins' cases, by their own helper, on the bf16 symbols), the binding, and the
precision argument's ValueError."""
import ctypes
import os

import numpy as np
import pytest

import conv2_ref as R2
import conv2b_ref as RW
import conv_bf16_ref as RH
import conv_ref as R
import convb_bf16_ref as RHB
import test_conv2d_wide_backward as twin

F = np.float32
ROWS, COLS = RHB.ROWS, RHB.COLS
CASES = ((3, 1, False), (1, 1, False), (3, 2, False), (1, 2, False), (3, 2, True))  # ksize, stride, transposed


class _Bf16Symbols:
    """The library with the float32 backward symbols of the wide layers answered by their bf16 forms: twin._call as it is."""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        if name == "dtfill_conv2d_wide_backward_workspace_bytes":
            return self._L.dtfill_conv2d_wide_backward_bf16_workspace_bytes
        if name.startswith("dtfill_conv2d_") and "_backward_" in name:
            return getattr(self._L, name + "_bf16")
        return getattr(self._L, name)


# ---- the statement against float64 autograd over the rounded operands --------------------------------------------------------

@pytest.mark.parametrize("ksize,stride,transposed", CASES)
def test_the_statement_against_float64_autograd(ksize, stride, transposed):
    """The exact sums of the statement are float64 sums of products of bf16 values (16-bit products, a few thousand terms: the
    float64 error is 2^-53 relative per addition, a millionth of the bound's 2^-23); torch differentiates the float64
    convolution of x^, w^ under the cotangent g^.  So the two agree within the contract's bound, with a wide margin."""
    import torch
    import torch.nn.functional as TF

    cin, cout = 16, 32
    B, Hs, Ws = 2, 5, 7
    rng = np.random.default_rng(10 * ksize + stride + transposed)
    xs = (B, Hs, Ws) if transposed else (B, stride * Hs, stride * Ws)
    ys = (B, 2 * Hs, 2 * Ws) if transposed else (B, Hs, Ws)
    x, w = rng.standard_normal(xs + (cin,)).astype(F), rng.standard_normal((ksize, ksize, cin, cout)).astype(F)
    dy, y = rng.standard_normal(ys + (cout,)).astype(F), rng.standard_normal(ys + (cout,)).astype(F)
    g = RHB.g_ref(dy, y, R.LEAKY, 0.2)
    xr, wr, gr = (RH.bf16_round(a).astype(np.float64) for a in (x, w, g))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tx, tg = t(xr).permute(0, 3, 1, 2), t(gr).permute(0, 3, 1, 2)
    if transposed:
        tw = t(wr).permute(2, 3, 0, 1).contiguous()  # [Cin, Cout, 3, 3]
        fwd = lambda vx, vw: TF.conv_transpose2d(vx, vw, stride=2)[:, :, :2 * Hs, :2 * Ws]
        layout = lambda v: v.permute(2, 3, 0, 1).numpy()
    else:
        tw = t(wr).permute(3, 2, 0, 1).contiguous()
        fwd = lambda vx, vw: twin._conv64(vx, vw, None, ksize, stride)
        layout = lambda v: v.permute(2, 3, 1, 0).numpy()
    dx, S, n = RHB.dx_ref(dy, y, w, stride, R.LEAKY, 0.2, transposed)
    want = twin._vjp(lambda v: fwd(v, tw), tx, tg).permute(0, 2, 3, 1).numpy()
    assert dx.shape == want.shape and (np.abs(dx - want) <= RHB.dx_bound(S, n)).all() and np.abs(want).max() > 0
    dw, db, bw, bb = RHB.dw_ref(x, dy, y, ksize, stride, R.LEAKY, 0.2, transposed)
    want = layout(twin._vjp(lambda v: fwd(tx, v), tw, tg))
    assert dw.shape == want.shape and (np.abs(dw - want) <= bw).all() and np.abs(want).max() > 0
    assert (np.abs(db - gr.sum(axis=(0, 1, 2))) <= bb).all()
    assert (bw > 0).all() and (bw < 1e-2 * np.abs(x).max() * np.abs(g).max() * B * Hs * Ws).all()  # a bound worth the name


@pytest.mark.parametrize("ksize,stride,transposed", CASES)
def test_the_integer_cases_are_exact_in_both_references(ksize, stride, transposed):
    """On integer_case the statement's float64 sums equal the int64 reference, and so does the float32 contract of the twins:
    every order gives the same value."""
    x, w, dy, y = RHB.integer_case(ksize, stride, 16, 32, (2, 3, 5), 3, transposed)
    dx, g, dw, db = RHB.integer_ref(x, w, dy, y, stride, R.LEAKY, transposed)
    sdx, _, _ = RHB.dx_ref(dy, y, w, stride, R.LEAKY, RHB.ALPHA_INT, transposed)
    sdw, sdb, _, _ = RHB.dw_ref(x, dy, y, ksize, stride, R.LEAKY, RHB.ALPHA_INT, transposed)
    assert np.array_equal(sdx, dx) and np.array_equal(sdw, dw) and np.array_equal(sdb, db)
    if transposed:
        fdx, (fdw, fdb) = RW.transpose_dx_ref(dy, y, w, R.LEAKY, RHB.ALPHA_INT), RW.transpose_dw_ref(x, dy, y, R.LEAKY, RHB.ALPHA_INT)
    else:
        fdx = RW.strided_dx_ref(dy, y, w, stride, R.LEAKY, RHB.ALPHA_INT)
        fdw, fdb = RW.strided_dw_ref(x, dy, y, ksize, stride, R.LEAKY, RHB.ALPHA_INT)
    assert np.array_equal(fdx, dx) and np.array_equal(fdw, dw) and np.array_equal(fdb, db)
    assert np.abs(dw).max() > 0 and np.abs(dx).max() > 0


def test_the_bound_terms():
    """n = the padded pixel count plus the segments: a row of a segment counts as whole k-steps of 32."""
    assert RHB.bound_terms((1, 1, 1)) == 32 + 1
    assert RHB.bound_terms((2, 33, 65)) == 2 * (33 * 64 + 33 * 32) + 2 * 2 * 2
    assert RHB.bound_terms((1, 33, 40)) == 33 * 64 + 2
    assert RHB.bound_terms((4, 256, 1216)) == 4 * 256 * 1216 + 4 * 8 * 19
    assert RHB.bound_terms((1, 4, 4), True) == 4 * (4 * 32 + 1)


# ---- the entry points, without a device ------------------------------------------------------------------------------------------

def test_return_codes_without_a_device(pkg):
    """The twins' cases, in the twins' order, on the bf16 symbols; then what the bf16 domain refuses beyond them."""
    pkg.build()
    L = _Bf16Symbols(pkg.load())
    NULL, SHAPE, WORKSPACE = -1, -2, -3
    for which in twin.ORDER:
        data, transposed = which.endswith("data"), which.startswith("transpose")
        for name in ("dy", "y", "w", "dx", "ws") if data else ("x", "dy", "y", "dw", "ws"):
            assert twin._call(L, which, **{name: 0}) == NULL, (which, name)
        bad = [dict(Cin=c) for c in (0, 1, 8, 17, 24, -16)] + [dict(Cout=c, dy_channels=64, y_channels=64) for c in (0, 1, 2, 8, 24)] + \
            [dict(dy_offset=-1), dict(dy_offset=1), dict(dy_channels=15), dict(dy_channels=0), dict(y_offset=-1), dict(y_offset=1),
             dict(y_channels=15), dict(dy_offset=2 ** 31 - 1)] + \
            [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 9, H=1 << 9, W=1 << 9), dict(B=1, H=1 << 12, W=1 << 12, Cin=128),
             dict(B=1, H=1 << 12, W=1 << 12, Cout=128, dy_channels=128, y_channels=128), dict(B=1, H=1 << 12, W=1 << 12, dy_channels=128)] + \
            [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-0.2), dict(alpha=-1e-30)] + \
            [dict(Cin=1 << 14, Cout=1 << 14, dy_channels=1 << 14, y_channels=1 << 14)]
        if not transposed:
            bad += [dict(ksize=k) for k in (0, 2, 4, 5, 7, 9, -1)] + [dict(stride=s) for s in (0, 3, -1)] + \
                [dict(stride=2, ksize=5), dict(stride=2, H=5), dict(stride=2, W=3), dict(stride=2, ksize=1, H=1, W=1)]
        if data:
            bad += [dict(dx_offset=-1), dict(dx_offset=1), dict(dx_channels=15), dict(dx_channels=0), dict(B=1, H=1 << 12, W=1 << 12, dx_channels=128)]
        for change in bad:
            assert twin._call(L, which, ws_bytes=1 << 40, **change) == SHAPE, (which, change)
        assert twin._call(L, which, dy=0, Cin=8) == NULL  # the pointers first
        assert twin._call(L, which, act=0, y=0, y_channels=0, y_offset=-5, ws_bytes=0) == WORKSPACE
        assert twin._call(L, which, alpha=0.0, ws_bytes=0) == WORKSPACE
        full = L.dtfill_conv2d_wide_backward_workspace_bytes(1, 4, 4, 16, 3, 16, 2 if transposed else 1, int(transposed))
        assert full > 0 and twin._call(L, which, ws_bytes=full - 1) == WORKSPACE
        assert twin._call(L, which, ws=16) == WORKSPACE  # not 256-byte aligned
        assert twin._call(L, which, **({"dres": 0} if which == "strided_data" else {} if data else {"db": 0}), ws_bytes=0) == WORKSPACE
    for k in (1, 3):
        assert twin._call(L, "strided_data", stride=2, ksize=k, ws_bytes=0) == WORKSPACE
        assert twin._call(L, "strided_weights", stride=2, ksize=k, ws_bytes=0) == WORKSPACE


def test_the_workspace_rule(pkg):
    """Host arithmetic: g, the packed bf16 kernel of the forward over g (Cout in, Cin out: ksize^2 ceil(Cout / 32) (Cin / 16)
    fragments of 1024 bytes) and the 1x1 stride-2 values for the data call, the float32 partials for the weights call, each
    part rounded up to 256 bytes; the larger of the two; 0 outside the domain."""
    pkg.build()
    ws = pkg.load().dtfill_conv2d_wide_backward_bf16_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    nseg = lambda B, H, W: B * -(-H // ROWS) * -(-W // COLS)
    packed = lambda k, cin, cout: 2 * RH.packed_elems(k, cout, cin)
    for B, H, W, cin, k, cout, stride in ((1, 1, 1, 16, 1, 16, 1), (4, 256, 1216, 128, 3, 64, 1), (4, 128, 608, 64, 3, 128, 2),
                                          (2, 66, 130, 48, 1, 80, 2), (4, 32, 152, 512, 3, 512, 1), (2, 33, 65, 48, 3, 80, 1)):
        Ho, Wo = H // stride, W // stride
        data = up(4 * B * Ho * Wo * cout) + up(packed(k, cin, cout)) + (up(4 * B * Ho * Wo * cin) if (stride, k) == (2, 1) else 0)
        weights = up(4 * nseg(B, Ho, Wo) * (k * k * cin + 1) * cout)
        assert ws(B, H, W, cin, k, cout, stride, 0) == max(data, weights), (B, H, W, cin, k, cout, stride)
    for B, H, W, cin, cout in ((1, 1, 1, 16, 16), (4, 32, 152, 512, 256), (2, 33, 65, 48, 80)):
        data = up(4 * B * 4 * H * W * cout) + up(packed(3, cin, cout))
        assert ws(B, H, W, cin, 3, cout, 2, 1) == max(data, up(4 * nseg(B, H, W) * (9 * cin + 1) * cout))
    for bad in ((0, 4, 4, 16, 3, 16, 1, 0), (1, 4, 4, 8, 3, 16, 1, 0), (1, 4, 4, 16, 2, 16, 1, 0), (1, 4, 4, 16, 3, 24, 1, 0),
                (1, 5, 4, 16, 3, 16, 2, 0), (1, 4, 4, 16, 5, 16, 1, 0), (1, 4, 4, 16, 7, 16, 1, 0), (1, 4, 4, 16, 3, 16, 3, 0),
                (1, 4, 4, 16, 1, 16, 2, 1), (1, 4, 4, 16, 3, 16, 1, 1), (1, 1 << 13, 1 << 12, 64, 3, 16, 1, 0)):
        assert ws(*bad) == 0, bad


def test_binding(pkg):
    src = open(os.path.join(twin.ROOT, "include", "dtfill.h")).read()
    pkg.build()
    L = pkg.load()
    counts = {"strided_backward_data": 23, "strided_backward_weights": 21, "transpose_backward_data": 20, "transpose_backward_weights": 19}
    for name, n in counts.items():
        fn = getattr(L, "dtfill_conv2d_%s_bf16" % name)
        assert fn.argtypes == getattr(L, "dtfill_conv2d_" + name).argtypes and len(fn.argtypes) == n
        assert ("dtfill_conv2d_%s_bf16(" % name) in src, name
    assert L.dtfill_conv2d_wide_backward_bf16_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.dtfill_conv2d_wide_backward_bf16_workspace_bytes.argtypes) == 8
    assert "#define DTFILL_ABI_VERSION 1" in src


def test_the_precision_argument(pkg):
    import torch

    net, dev, autograd = pkg.net, pkg.device, pkg.autograd
    x, w, dy = torch.zeros((1, 4, 4, 16)), torch.zeros((3, 3, 16, 16)), torch.zeros((1, 4, 4, 16))
    for bad in ("fp16", "bfloat16", None, 16):
        with pytest.raises(ValueError, match="precision"):
            autograd.conv2d_strided(x, w, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            autograd.conv2d_transpose(x, w, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            net._backward_data("strided", dy, w, 1, None, "linear", 0.2, 0, 0, None, 0, precision=bad)
    with pytest.raises(ValueError, match="no bf16 backward"):
        net._backward_weights("narrow", x, dy, 3, 1, None, "linear", 0.2, 0, 0, None, True, precision="bf16")
    weights = net.glorot_weights_resnet18(0, scale_num=1)
    for cls, make in ((net.ResNet18Trainable, net.glorot_weights_resnet18), (net.ResNet18ImageTrainable, net.glorot_weights_resnet18_image),
                      (net.ResNet18LightImageTrainable, net.glorot_weights_resnet18_light_image)):
        model = cls(weights if cls is net.ResNet18Trainable else make(0, scale_num=1), scale_num=1)
        assert model.precision == "float32"
        for bad in ("fp16", "half", None, 16, "BF16"):
            with pytest.raises(ValueError, match="precision"):
                model.precision = bad
            assert model.precision == "float32"
        model.precision = "bf16"
        assert model.precision == "bf16" and "precision" not in model.state_dict() and cls(weights if cls is net.ResNet18Trainable else
                                                                                             make(0, scale_num=1), scale_num=1).precision == "float32"
        model.precision = "float32"
        assert model.precision == "float32"
    for call in (lambda: dev.conv2d_strided_backward_data_bf16_device(dy, w, 1), lambda: dev.conv2d_strided_backward_weights_bf16_device(x, dy, 3),
                 lambda: dev.conv2d_transpose_backward_data_bf16_device(dy, w), lambda: dev.conv2d_transpose_backward_weights_bf16_device(x, dy)):
        with pytest.raises((ValueError, RuntimeError)):  # host tensors are refused before any device work
            call()
    assert dev.conv2d_wide_backward_bf16_workspace_bytes(1, 4, 4, 16, 3, 16, 2) == \
        pkg.load().dtfill_conv2d_wide_backward_bf16_workspace_bytes(1, 4, 4, 16, 3, 16, 2, 0)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_wide_backward_bf16_workspace_bytes(1, 4, 4, 16, 5, 16)

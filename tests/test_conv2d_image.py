"""dtfill_conv2d_image and dtfill_conv2d_image_backward_weights without a device: the numpy statement of the contract
(tests/conv_ref.py, which holds for any Cin and Cout) at the image layer's channel counts against a float64 convolution, and
everything of the three entry points that needs no GPU: every return code in the header's order, the workspace formula, the
binding, and the Python layer's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import conv_ref as R
import convb_ref as RB

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS


@pytest.mark.parametrize("cout", (16, 64))
@pytest.mark.parametrize("ksize,cin", ((3, 3), (7, 2), (5, 4), (1, 3)))
def test_conv_ref_against_float64(ksize, cin, cout):
    """Within gamma_(K+2) (sum |x| |w| + |bias|) of a float64 convolution, K = ksize^2 Cin: one rounding per link of the
    chain, one for the bias, one for the leaky product -- derived, not measured."""
    import torch

    rng = np.random.default_rng(7 * ksize + cin)
    x = rng.standard_normal((2, 5, 9, cin)).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    bias = rng.standard_normal(cout).astype(F)
    got = R.conv_ref(x, w, bias, R.LEAKY, 0.2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    y = torch.nn.functional.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(3, 2, 0, 1), t(bias), padding=ksize // 2)
    y = y.permute(0, 2, 3, 1).numpy()
    y = np.where(y > 0, y, y * np.float64(F(0.2)))
    bound = R.gamma(ksize * ksize * cin + 2) * R.abs_sum(x, w, bias)
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= bound).all(), (err.max(), bound[err > bound].min())
    assert err.max() > 0  # (a comparison of two different evaluations, not of one with itself)


def test_the_chain_is_one_group_taps_then_channels():
    """Cin < 16 is a single group: the two orders conv_ref knows are one, raster taps outermost and the channels inside."""
    for ksize, cin in ((3, 3), (7, 4), (1, 2)):
        order = R.chain_order(ksize, cin)
        assert order == R.chain_order(ksize, cin, "taps") == [(i, j, c) for i in range(ksize) for j in range(ksize) for c in range(cin)]
        assert (len(order) + 1) % 16 != 0  # the weight gradient's tiles of 16 rows always have a free one for db
    assert len(R.chain_order(3, 3)) == 27  # the RGB stem: six whole matrix-core steps and three links of a seventh


# ---- the entry points, without a device ------------------------------------------------------------------------------------

NULL, SHAPE, WORKSPACE = -1, -2, -3
FWD_GOOD = dict(x=1, B=1, H=4, W=4, Cin=3, w=1, bias=1, ksize=3, Cout=64, act=1, alpha=0.2, out=1, out_channels=64, out_offset=0)
FWD_ORDER = ("x", "B", "H", "W", "Cin", "w", "bias", "ksize", "Cout", "act", "alpha", "out", "out_channels", "out_offset")
BW_GOOD = dict(x=1, dy=1, dy_channels=64, dy_offset=0, y=1, y_channels=64, y_offset=0, B=1, H=4, W=4, Cin=3, ksize=3, Cout=64, act=1,
               alpha=0.2, dw=1, db=1, ws=1, ws_bytes=None)
BW_ORDER = ("x", "dy", "dy_channels", "dy_offset", "y", "y_channels", "y_offset", "B", "H", "W", "Cin", "ksize", "Cout", "act", "alpha",
            "dw", "db", "ws", "ws_bytes")
BW_POINTERS = ("x", "dy", "y", "dw", "db")


def _fwd(L, **change):
    a = dict(FWD_GOOD, **change)
    buf = ctypes.create_string_buffer(64)  # never read: every call here returns before any HIP call
    ptr = lambda v: ctypes.addressof(buf) if v else None
    return L.dtfill_conv2d_image(*[ptr(a[k]) if k in ("x", "w", "bias", "out") else a[k] for k in FWD_ORDER], None)


def _bw(L, **change):
    a = dict(BW_GOOD, **change)
    buf = ctypes.create_string_buffer(1024)  # never read
    base = ctypes.addressof(buf)
    base += (-base) % 256
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.dtfill_conv2d_image_backward_workspace_bytes(a["B"], a["H"], a["W"], a["Cin"], a["ksize"], a["Cout"]) or 1 << 20
    val = lambda k: (base if a[k] else None) if k in BW_POINTERS else (base + (a[k] if a[k] > 1 else 0) if a[k] else None) if k == "ws" else a[k]
    return L.dtfill_conv2d_image_backward_weights(*[val(k) for k in BW_ORDER], None)


def test_forward_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    for name in ("x", "w", "out"):
        assert _fwd(L, **{name: 0}) == NULL, name
    bad = [dict(Cin=c) for c in (1, 5, 16, 0, -3)] + [dict(Cout=c) for c in (1, 8, 24, 0, -16)] + [dict(ksize=k) for k in (0, 2, 9, 4, -1)] + \
        [dict(out_offset=-1), dict(out_offset=1), dict(out_channels=63), dict(out_channels=0), dict(out_offset=2 ** 31 - 1),
         dict(Cout=16, out_channels=64, out_offset=49)] + \
        [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 11, H=1 << 10, W=1 << 10), dict(B=1, H=1 << 13, W=1 << 12),
         dict(B=1, H=1 << 12, W=1 << 11, out_channels=256), dict(B=1, H=1 << 15, W=1 << 14, Cin=4, Cout=16, out_channels=16)] + \
        [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf"))]
    for change in bad:
        assert _fwd(L, **change) == SHAPE, change
    assert _fwd(L, x=0, ksize=2) == NULL  # the pointers first, as everywhere in the ABI
    # just inside the limits: 2^24 pixels of 64 channels is 2^30 floats (refused only for its NULL), a NULL bias is allowed,
    # alpha < 0 is the forward's business
    assert _fwd(L, x=0, B=1, H=1 << 12, W=1 << 12) == NULL
    assert _fwd(L, x=0, bias=0, alpha=-0.1, Cin=2, ksize=7, Cout=16, out_channels=80, out_offset=64) == NULL


def test_backward_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    for name in ("x", "dy", "y", "dw", "ws"):
        assert _bw(L, **{name: 0}) == NULL, name
    bad = [dict(Cin=c) for c in (1, 5, 16, 0)] + [dict(Cout=c) for c in (1, 8, 24, 0)] + [dict(ksize=k) for k in (0, 2, 9)] + \
        [dict(dy_offset=-1), dict(dy_offset=1), dict(dy_channels=63), dict(dy_channels=0), dict(y_offset=-1), dict(y_offset=1),
         dict(y_channels=63), dict(dy_offset=2 ** 31 - 1), dict(Cout=16, dy_offset=49)] + \
        [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 11, H=1 << 10, W=1 << 10), dict(B=1, H=1 << 13, W=1 << 12),
         dict(B=1, H=1 << 12, W=1 << 11, dy_channels=256), dict(B=1, H=1 << 12, W=1 << 11, y_channels=256),
         dict(Cin=4, ksize=7, Cout=1 << 24, dy_channels=1 << 24, y_channels=1 << 24)] + \
        [dict(act=2), dict(act=-1), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-1e-30)]
    for change in bad:
        assert _bw(L, ws_bytes=1 << 40, **change) == SHAPE, change
    assert _bw(L, dy=0, Cin=8) == NULL  # the pointers first
    assert _bw(L, Cin=8, ws_bytes=0) == SHAPE  # the shape before the workspace
    # y is not needed, and not looked at, for a linear layer; alpha = 0 (a ReLU) is in the domain; db may be NULL
    assert _bw(L, act=0, y=0, y_channels=0, y_offset=-5, ws_bytes=0) == WORKSPACE
    assert _bw(L, alpha=0.0, ws_bytes=0) == WORKSPACE
    assert _bw(L, db=0, ws_bytes=0) == WORKSPACE
    full = L.dtfill_conv2d_image_backward_workspace_bytes(1, 4, 4, 3, 3, 64)
    assert full > 0 and _bw(L, ws_bytes=full - 1) == WORKSPACE  # one byte short
    assert _bw(L, ws=16) == WORKSPACE  # not 256-byte aligned


def test_the_workspace_formula(pkg):
    """Pure host arithmetic: the segments' partials, 4 S (ksize^2 Cin + 1) Cout bytes, rounded up to 256; 0 outside the domain."""
    pkg.build()
    ws = pkg.load().dtfill_conv2d_image_backward_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    for B, H, W, cin, ksize, cout in ((1, 1, 1, 2, 1, 16), (4, 256, 1216, 3, 3, 64), (1, 352, 1216, 3, 3, 64), (2, ROWS + 1, COLS + 1, 4, 7, 16),
                                      (1, ROWS, COLS, 2, 5, 80), (3, 5, 2 * COLS, 4, 1, 128)):
        nseg = B * -(-H // ROWS) * -(-W // COLS)
        assert ws(B, H, W, cin, ksize, cout) == up(4 * nseg * (ksize * ksize * cin + 1) * cout), (B, H, W, cin, ksize, cout)
    assert ws(4, 256, 1216, 3, 3, 64) == 4 * 608 * 28 * 64  # the stem at the KITTI crop, B = 4: 4.4 MB of partials
    for bad in ((0, 4, 4, 3, 3, 64), (1, 0, 4, 3, 3, 64), (1, 4, -1, 3, 3, 64), (1, 4, 4, 1, 3, 64), (1, 4, 4, 5, 3, 64), (1, 4, 4, 16, 3, 64),
                (1, 4, 4, 3, 2, 64), (1, 4, 4, 3, 9, 64), (1, 4, 4, 3, 3, 1), (1, 4, 4, 3, 3, 8), (1, 4, 4, 3, 3, 24),
                (1, 1 << 13, 1 << 12, 3, 3, 64), (1 << 11, 1 << 10, 1 << 10, 3, 3, 16)):
        assert ws(*bad) == 0, bad


def test_binding(pkg):
    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    pkg.build()
    L = pkg.load()
    assert len(L.dtfill_conv2d_image.argtypes) == 15 and L.dtfill_conv2d_image.restype is ctypes.c_int
    assert len(L.dtfill_conv2d_image_backward_weights.argtypes) == 20 and L.dtfill_conv2d_image_backward_weights.restype is ctypes.c_int
    assert L.dtfill_conv2d_image_backward_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.dtfill_conv2d_image_backward_workspace_bytes.argtypes) == 6
    symbols = pkg._lib.SYMBOLS
    at = symbols.index("dtfill_conv2d_image_backward_workspace_bytes")
    assert symbols[at:at + 3] == ("dtfill_conv2d_image_backward_workspace_bytes", "dtfill_conv2d_image_backward_weights", "dtfill_conv2d_image")
    assert "dtfill_conv2d_image_backward_data" not in src  # there is no data gradient: the image is data
    assert re.search(r"#define DTFILL_ABI_VERSION 1\b", src) and L.dtfill_abi_version() == 1  # the ABI only grew
    for name in ("conv2d_image_device", "conv2d_image_backward_weights_device", "conv2d_image_backward_workspace_bytes"):
        assert callable(getattr(pkg.device, name))
    assert callable(pkg.conv2d_image) and callable(pkg.autograd.conv2d_image)


def test_python_layer_argument_checks_without_gpu(pkg):
    import torch

    dev = pkg.device
    x, w, dy = torch.zeros((1, 4, 4, 3)), torch.zeros((3, 3, 3, 64)), torch.zeros((1, 4, 4, 64))
    with pytest.raises(ValueError, match="act must be"):
        dev.conv2d_image_device(x, w, act="relu")
    with pytest.raises(ValueError, match="alpha"):
        dev.conv2d_image_backward_weights_device(x, dy, 3, dy, act="leaky", alpha=-0.5)
    with pytest.raises(ValueError, match="alpha"):
        pkg.autograd.conv2d_image(x, w, act="leaky", alpha=float("nan"))
    with pytest.raises(ValueError, match="image is data"):
        pkg.autograd.conv2d_image(x.clone().requires_grad_(), w)
    # host tensors where device tensors are asked for, and wrong ranks and dtypes, are refused before any device work
    for bad in (dict(x=x), dict(x=x.double()), dict(x=x[0])):
        with pytest.raises((ValueError, RuntimeError)):
            dev.conv2d_image_device(**dict(dict(x=x, w=w), **bad))
    for call in (lambda: dev.conv2d_image_backward_weights_device(x, dy, 3), lambda: pkg.autograd.conv2d_image(x, w)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    with pytest.raises(ValueError):
        pkg.conv2d_image(np.zeros((4, 4, 3), F), np.zeros((3, 3, 3, 64), F))
    with pytest.raises(TypeError):
        pkg.conv2d_image(np.zeros((1, 4, 4, 3), complex), np.zeros((3, 3, 3, 64), F))
    assert dev.conv2d_image_backward_workspace_bytes(1, 4, 4, 3, 3, 64) == pkg.load().dtfill_conv2d_image_backward_workspace_bytes(1, 4, 4, 3, 3, 64)
    with pytest.raises(pkg.DtfillError):
        dev.conv2d_image_backward_workspace_bytes(1, 4, 4, 16, 3, 64)

"""dtfill_conv2d_strided and dtfill_conv2d_transpose without a device: the numpy statements of their contracts
(tests/conv2_ref.py) against conv_ref's, against float64 convolutions and against the definition of the transposed convolution,
what the statements pin (TensorFlow's 'same' rule at stride 2, which input each output parity reads, bias before residual), and
everything of the entry points that needs no GPU (return codes, the binding, the Python layer's argument checks)."""
import ctypes

import numpy as np
import pytest

import conv2_ref as R2
import conv_ref as R

F = np.float32


def _case(ksize, cin, cout, shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (cin,)).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    return x, w, rng.standard_normal(cout).astype(F)


@pytest.mark.parametrize("ksize,cin,cout", ((1, 16, 16), (3, 32, 48), (5, 16, 16), (7, 64, 16)))
def test_stride_1_without_residual_is_conv_ref(ksize, cin, cout):
    x, w, b = _case(ksize, cin, cout, (2, 5, 9), ksize)
    for bias, act in ((b, R.LEAKY), (None, R.LINEAR)):
        got, want = R2.strided_ref(x, w, bias, 1, None, act, 0.2), R.conv_ref(x, w, bias, act, 0.2)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_same_rule_numbers():
    """The header's own examples of TensorFlow's rule: (output extent, front, behind)."""
    assert [R2.same_rule(n, 3, 1) for n in (1, 4, 5)] == [(1, 1, 1), (4, 1, 1), (5, 1, 1)]
    assert [R2.same_rule(n, 7, 1) for n in (1, 9)] == [(1, 3, 3), (9, 3, 3)]
    assert [R2.same_rule(n, 3, 2) for n in (1, 2, 4, 5, 7, 8)] == [(1, 1, 1), (1, 0, 1), (2, 0, 1), (3, 1, 1), (4, 1, 1), (4, 0, 1)]
    assert [R2.same_rule(n, 1, 2) for n in (1, 2, 5, 8)] == [(1, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0)]


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("H,W", ((4, 6), (5, 7), (4, 7), (5, 6), (1, 1), (2, 1)))
def test_stride_2_padding_against_float64(ksize, H, W):
    """Against a float64 torch conv2d of the explicitly padded input, within gamma_(K+3) (sum |x| |w| + |bias| + |residual|),
    K = ksize^2 Cin: one rounding per link, one each for the bias, the residual and the leaky product -- derived, not measured."""
    cin, cout = 32, 16
    x, w, b = _case(ksize, cin, cout, (2, H, W), 10 * H + W + ksize)
    Ho, Wo = -(-H // 2), -(-W // 2)
    res = np.random.default_rng(H).standard_normal((2, Ho, Wo, cout)).astype(F)
    got = R2.strided_ref(x, w, b, 2, res, R.LEAKY, 0.2)
    assert got.shape == (2, Ho, Wo, cout)
    want = R2.strided_f64(x, w, b, 2, res, R.LEAKY, 0.2)
    bound = R.gamma(ksize * ksize * cin + 3) * R2.abs_sum_strided(x, w, b, 2, res)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (err.max(), bound[err > bound].min())
    assert err.max() > 0
    # the other split of the padding (the larger half in front) is another function: where the two splits differ, so do the results
    if ksize == 3 and H % 2 == 0 and H > 1:
        shifted = R2.strided_f64(np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0)))[:, :H, :W], w, b, 2, res, R.LEAKY, 0.2)
        assert (np.abs(shifted - want) > bound).any()


@pytest.mark.parametrize("H,W", ((1, 1), (2, 3), (3, 4)))
def test_transposed_statement_is_the_gradient_of_the_stride_2_convolution(H, W):
    """Against the definition (the float64 vector-Jacobian product of the stride-2 'same' convolution of a [2H,2W] frame) and
    against torch's conv_transpose2d cropped to [:2H, :2W], within gamma_(K+3) of the absolute sum, K = 4 Cin links at most."""
    cin, cout = 32, 16
    rng = np.random.default_rng(H * W)
    x = rng.standard_normal((2, H, W, cin)).astype(F)
    kernel = (rng.standard_normal((3, 3, cout, cin)) / 3).astype(F)  # Keras's layout
    b = rng.standard_normal(cout).astype(F)
    got = R2.transpose_ref(x, R2.pack(kernel), b, R.LEAKY, 0.2)
    assert got.shape == (2, 2 * H, 2 * W, cout)
    bound = R.gamma(4 * cin + 3) * R2.abs_sum_transpose(x, kernel, b)
    for want in (R2.transpose_f64_vjp(x, kernel, b, R.LEAKY, 0.2), R2.transpose_f64_torch(x, kernel, b, R.LEAKY, 0.2)):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (err.max(), bound[err > bound].min())
        assert err.max() > 0


def test_which_input_each_parity_reads():
    """A 2 x 3 frame of distinct values, one channel in and out (of 16, the others zero), under a kernel of distinct powers of
    ten: every output names its inputs and taps."""
    x = np.zeros((1, 2, 3, 16), F)
    x[0, :, :, 0] = [[1, 2, 3], [4, 5, 6]]
    w = np.zeros((3, 3, 16, 16), F)
    w[:, :, 0, 0] = [[1, 10, 100], [1e3, 1e4, 1e5], [1e6, 1e7, 1e8]]
    y = R2.transpose_ref(x, w)[0, :, :, 0]
    assert y.shape == (4, 6)
    # (odd, odd): the pixel itself under the centre tap alone
    assert y[1, 1] == 1 * 1e4 and y[3, 5] == 6 * 1e4 and y[1, 3] == 2 * 1e4
    # (odd, even): tap (1, 0) on the pixel, tap (1, 2) on its left neighbour -- padding at u = 0
    assert y[1, 0] == 1 * 1e3 and y[1, 2] == 2 * 1e3 + 1 * 1e5 and y[3, 4] == 6 * 1e3 + 5 * 1e5
    # (even, odd): tap (0, 1) on the pixel, tap (2, 1) on the one above -- padding at y = 0
    assert y[0, 1] == 1 * 10 and y[2, 1] == 4 * 10 + 1 * 1e7 and y[2, 5] == 6 * 10 + 3 * 1e7
    # (even, even): four taps, the corner ones; at (0, 0) only tap (0, 0) is inside
    assert y[0, 0] == 1 * 1 and y[0, 2] == 2 * 1 + 1 * 100 and y[2, 0] == 4 * 1 + 1 * 1e6
    assert y[2, 2] == 5 * 1 + 4 * 100 + 2 * 1e6 + 1 * 1e8
    # and the forward stride-2 rule: an even frame pads behind only, an odd one on both sides
    xs = np.zeros((1, 2, 4, 16), F)
    xs[0, :, :, 0] = [[1, 2, 3, 4], [5, 6, 7, 8]]
    ws = np.zeros((3, 3, 16, 16), F)
    ws[:, :, 0, 0] = w[:, :, 0, 0]
    s = R2.strided_ref(xs, ws, stride=2)[0, :, :, 0]
    assert s.shape == (1, 2) and s[0, 0] == 1 + 2 * 10 + 3 * 100 + 5 * 1e3 + 6 * 1e4 + 7 * 1e5  # window rows 0..2, columns 0..2
    assert s[0, 1] == 3 + 4 * 10 + 7 * 1e3 + 8 * 1e4
    s = R2.strided_ref(xs[:, :1, :3], ws, stride=2)[0, :, :, 0]  # 1 x 3: pt = 1, pl = 1
    assert s.shape == (1, 2) and s[0, 0] == 1 * 1e4 + 2 * 1e5 and s[0, 1] == 2 * 1e3 + 3 * 1e4


def test_bias_is_added_before_the_residual():
    """acc = 1, bias = u / 2, residual = u, u = 2^-23.  Bias first: 1 + u / 2 is a tie and rounds to even, 1; then 1 + u.
    Residual first: 1 + u; then 1 + 1.5 u is a tie and rounds to even, 1 + 2 u."""
    x = np.zeros((1, 1, 1, 16), F)
    w = np.zeros((1, 1, 16, 16), F)
    x[0, 0, 0, 0] = w[0, 0, 0, :] = 1
    u = 2.0 ** -23
    b, r = np.full(16, u / 2, F), np.full((1, 1, 1, 16), u, F)
    first = R2.strided_ref(x, w, b, 1, r)[0, 0, 0, 0]
    other = R2.strided_ref(x, w, b, 1, r, residual_first=True)[0, 0, 0, 0]
    assert first == F(1 + u) and other == F(1 + 2 * u) and first != other
    # and the activation comes last: a negative sum is scaled once, after both adds
    assert R2.strided_ref(x, -w, np.full(16, -1, F), 1, np.full((1, 1, 1, 16), -2, F), R.LEAKY, 0.5)[0, 0, 0, 0] == -2


def test_pack_transpose_kernel(pkg):
    import importlib

    net = importlib.import_module(pkg.__name__ + ".net")
    kernel = np.arange(3 * 3 * 32 * 16, dtype=np.float64).reshape(3, 3, 32, 16)  # [3,3,Cout = 32,Cin = 16]
    packed = net.pack_transpose_kernel(kernel)
    assert packed.shape == (3, 3, 16, 32) and packed.dtype == F and packed.flags["C_CONTIGUOUS"]
    assert packed[2, 1, 5, 7] == kernel[2, 1, 7, 5] and (packed == R2.pack(kernel)).all()
    assert pkg.pack_transpose_kernel is net.pack_transpose_kernel
    for bad in (np.zeros((3, 3, 16)), np.zeros((5, 5, 16, 16)), np.zeros((3, 1, 16, 16))):
        with pytest.raises(ValueError):
            net.pack_transpose_kernel(bad)


# ---- the entry points, without a device ------------------------------------------------------------------------------

GOOD = dict(x=1, B=1, H=4, W=4, Cin=16, w=1, bias=1, ksize=3, Cout=32, stride=1, residual=1, act=1, alpha=0.2, out=1,
            out_channels=32, out_offset=0)
STRIDED = ("x", "B", "H", "W", "Cin", "w", "bias", "ksize", "Cout", "stride", "residual", "act", "alpha", "out", "out_channels",
           "out_offset")
TRANSPOSE = ("x", "B", "H", "W", "Cin", "w", "bias", "Cout", "act", "alpha", "out", "out_channels", "out_offset")
POINTERS = ("x", "w", "bias", "residual", "out")


def _call(f, order, **change):
    a = dict(GOOD, **change)
    buf = ctypes.create_string_buffer(64)  # never read: every call here returns before any HIP call
    ptr = lambda v: ctypes.addressof(buf) if v else None
    return f(*[ptr(a[k]) if k in POINTERS else a[k] for k in order], None)


def test_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    NULL, SHAPE = -1, -2
    shared = [dict(Cin=c) for c in (0, 1, 8, 17, 24, -16)] + [dict(Cout=c, out_channels=64) for c in (0, 1, 8, 17, 40, -16)] + \
        [dict(out_offset=-1), dict(out_offset=1), dict(out_channels=31), dict(out_channels=0), dict(out_offset=2 ** 31 - 1)] + \
        [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 15, H=1 << 8, W=1 << 8), dict(B=1 << 9, H=1 << 9, W=1 << 9)] + \
        [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf"))]
    for f, order in ((L.dtfill_conv2d_strided, STRIDED), (L.dtfill_conv2d_transpose, TRANSPOSE)):
        for name in ("x", "w", "out"):
            assert _call(f, order, **{name: 0}) == NULL, name
        for change in shared:
            assert _call(f, order, **change) == SHAPE, (order is STRIDED, change)
        assert _call(f, order, x=0, Cin=8) == NULL  # the pointers first, as everywhere in the ABI
    strided = lambda **c: _call(L.dtfill_conv2d_strided, STRIDED, **c)
    for change in [dict(stride=s) for s in (0, 3, -1, 4)] + [dict(ksize=k) for k in (0, 2, 4, 9, -1)] + \
            [dict(stride=2, ksize=5), dict(stride=2, ksize=7), dict(stride=2, ksize=2)] + \
            [dict(B=1, H=1 << 12, W=1 << 12, Cin=128), dict(B=1, H=1 << 12, W=1 << 12, Cout=128, out_channels=128),
             dict(B=1, H=1 << 12, W=1 << 12, out_channels=128)]:
        assert strided(**change) == SHAPE, change
    # at stride 2 the output is a quarter of the frame: 2^24 pixels x 64 channels in, 2^22 x 128 out is within the rule
    assert strided(x=0, B=1, H=1 << 12, W=1 << 12, Cin=64, stride=2, Cout=128, out_channels=128) == NULL
    transpose = lambda **c: _call(L.dtfill_conv2d_transpose, TRANSPOSE, **c)
    # the output is four times the frame: 2^22 pixels in, 2^24 x 128 channels out is not
    for change in (dict(B=1, H=1 << 11, W=1 << 11, Cout=128, out_channels=128), dict(B=1, H=1 << 15, W=1 << 14)):
        assert transpose(**change) == SHAPE, change
    assert b"shape" in L.dtfill_strerror(SHAPE)


def test_binding(pkg):
    pkg.build()
    L = pkg.load()
    assert len(L.dtfill_conv2d_strided.argtypes) == 17 and len(L.dtfill_conv2d_transpose.argtypes) == 14
    assert L.dtfill_conv2d_strided.restype is ctypes.c_int and L.dtfill_conv2d_transpose.restype is ctypes.c_int
    symbols = pkg._lib.SYMBOLS
    assert symbols.index("dtfill_conv2d_strided") + 1 == symbols.index("dtfill_conv2d_transpose") == len(symbols) - 2
    for name in ("conv2d_strided_device", "conv2d_transpose_device"):
        assert callable(getattr(pkg.device, name))
    assert callable(pkg.conv2d_strided) and callable(pkg.conv2d_transpose)


def test_python_layer_argument_checks_without_gpu(pkg):
    import torch

    dev = pkg.device
    x, w = torch.zeros((1, 4, 4, 16)), torch.zeros((3, 3, 16, 16))
    with pytest.raises(ValueError, match="act must be"):
        dev.conv2d_strided_device(x, w, act="relu")
    with pytest.raises(ValueError, match="act must be"):
        dev.conv2d_transpose_device(x, w, act="relu")
    with pytest.raises(ValueError, match="stride must be"):
        dev.conv2d_strided_device(x, w, stride=3)
    # host tensors where device tensors are asked for, and wrong ranks and dtypes, are refused before any device work
    for f in (dev.conv2d_strided_device, dev.conv2d_transpose_device):
        for bad in (dict(x=x), dict(x=x.double()), dict(x=x[0])):
            with pytest.raises((ValueError, RuntimeError)):
                f(**dict(dict(x=x, w=w) if f is dev.conv2d_strided_device else dict(x=x, w_packed=w), **bad))
    with pytest.raises(ValueError):
        pkg.conv2d_strided(np.zeros((4, 4, 16), F), np.zeros((3, 3, 16, 16), F))
    with pytest.raises(ValueError):
        pkg.conv2d_transpose(np.zeros((1, 4, 4, 16), F), np.zeros((3, 16, 16), F))
    with pytest.raises(TypeError):
        pkg.conv2d_strided(np.zeros((1, 4, 4, 16), complex), np.zeros((3, 3, 16, 16), F))

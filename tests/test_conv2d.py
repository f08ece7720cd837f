"""dtfill_conv2d without a device: the numpy statement of its contract (tests/conv_ref.py) against exact arithmetic and against
a float64 convolution, what the statement pins (cross-correlation, 'same' padding, the groups-outermost order, out_offset), and
everything of the entry point that needs no GPU (return codes, the binding, the Python layer's argument checks)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import conv_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_LAYERS = R.NET_LAYERS


def round_f32(fr):
    """A Fraction to the nearest float32, ties to even, subnormals included: the integer arithmetic of the definition."""
    if fr == 0:
        return F(0)
    sign, fr = (-1 if fr < 0 else 1), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    e += (Fraction(2) ** (e + 1) <= fr) - (Fraction(2) ** e > fr)  # 2^e <= fr < 2^(e+1)
    quantum = Fraction(2) ** max(e - 23, -149)
    n = fr / quantum
    whole, rest = n.numerator // n.denominator, n - n.numerator // n.denominator
    whole += rest > Fraction(1, 2) or (rest == Fraction(1, 2) and whole % 2 == 1)
    return F(sign * float(whole * quantum))  # (exact: at most 24 bits)


def exact_fma(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma32_is_correctly_rounded():
    # the triple where float32(float64(a) * b + c) rounds twice: the float64 sum lands on the midpoint the exact sum lies below
    a, b, c = F(1 + 2.0 ** -23), F((1 - 2.0 ** -23) * 2.0 ** -24), F(1 + 2.0 ** -23)
    assert F(np.float64(a) * np.float64(b) + np.float64(c)) == F(1 + 2.0 ** -22)
    assert R.fma32(a, b, c) == exact_fma(a, b, c) == F(1 + 2.0 ** -23)
    assert R.fma32(-a, b, -c) == -F(1 + 2.0 ** -23)
    rng = np.random.default_rng(1)
    n = 3000
    scale = lambda lo, hi: 2.0 ** rng.integers(lo, hi, n)
    a, b = (rng.standard_normal(n) * scale(-20, 20)).astype(F), (rng.standard_normal(n) * scale(-20, 20)).astype(F)
    j = (1 + rng.integers(1, 9, n) * 2.0 ** -23).astype(F)
    cases = {
        "random": (a, b, (rng.standard_normal(n) * scale(-40, 40)).astype(F)),
        "cancelling": (a, b, (-a.astype(np.float64) * b + rng.standard_normal(n) * scale(-60, 5)).astype(F)),
        "subnormal": ((rng.standard_normal(n) * 2.0 ** -70).astype(F), (rng.standard_normal(n) * 2.0 ** -70).astype(F),
                      (rng.standard_normal(n) * 2.0 ** -141).astype(F)),
        # the triple's family: a b = +-2^-24 (1 - j^2 2^-46), so the float64 sum is c +- 2^-24 exactly, a float32 midpoint
        "midpoint": (j, ((2 - j.astype(np.float64)) * 2.0 ** -24 * rng.choice([-1, 1], n)).astype(F),
                     (1 + rng.integers(0, 1 << 23, n) * 2.0 ** -23).astype(F)),
    }
    for what, (x, y, z) in cases.items():
        got = R.fma32(x, y, z)
        want = np.array([exact_fma(*t) for t in zip(x, y, z)], F)
        assert (got.view(np.uint32) == want.view(np.uint32)).all() or (got == want).all(), what
    x, y, z = cases["midpoint"]  # (the family is the one the two-rounding route gets wrong)
    assert ((x.astype(np.float64) * y + z).astype(F) != R.fma32(x, y, z)).any()
    assert np.isnan(R.fma32(F(np.inf), F(0), F(1))) and R.fma32(F(np.inf), F(1), F(1)) == np.inf
    assert R.fma32(F(3e38), F(3e38), F(0)) == np.inf and R.fma32(np.zeros((2, 1), F), np.ones(3, F), F(0)).shape == (2, 3)


def _layer_case(ksize, cin, cout, seed, shape=(2, 5, 9)):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (cin,)).astype(F)
    x[rng.random(x.shape) < 0.3] = 0
    w = (rng.standard_normal((ksize, ksize, cin, cout)) / ksize).astype(F)
    return x, w, rng.standard_normal(cout).astype(F)


@pytest.mark.parametrize("ksize,cin,cout,act", NET_LAYERS)
def test_conv_ref_against_float64(ksize, cin, cout, act):
    """Within gamma_(K+2) (sum |x| |w| + |bias|) of a float64 convolution: one rounding per link of the chain, one for the bias,
    one for the leaky product -- derived, not measured.  (The float64 side's own error is 2^-29 of that and is not added.)"""
    import torch

    x, w, bias = _layer_case(ksize, cin, cout, 7 * ksize + cin)
    got = R.conv_ref(x, w, bias, act, 0.2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    y = torch.nn.functional.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(3, 2, 0, 1), t(bias), padding=ksize // 2)
    y = y.permute(0, 2, 3, 1).numpy()
    if act == R.LEAKY:
        y = np.where(y > 0, y, y * np.float64(F(0.2)))
    bound = R.gamma(ksize * ksize * cin + 2) * R.abs_sum(x, w, bias)
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= bound).all(), (err.max(), bound[err > bound].min())
    assert err.max() > 0  # (a comparison of two different evaluations, not of one with itself)


def test_cross_correlation_and_same_padding():
    """One non-zero pixel under an asymmetric kernel: out[h, v] = x[p] * w[p - (h, v) + r], so the kernel appears flipped around
    the pixel in the output (cross-correlation), cut off at the frame's edge ('same' padding with zeros)."""
    w = np.arange(1, 10, dtype=F).reshape(3, 3, 1, 1)
    x = np.zeros((1, 4, 5, 1), F)
    x[0, 0, 1, 0] = 2
    want = np.zeros((4, 5), F)
    want[0, 0:3] = 2 * w[1, ::-1, 0, 0]  # the pixel's own row: taps (1, 2), (1, 1), (1, 0)
    want[1, 0:3] = 2 * w[0, ::-1, 0, 0]  # the row below sees it through the kernel's top row
    assert (R.conv_ref(x, w)[0, :, :, 0] == want).all()
    w5 = np.arange(1, 26, dtype=F).reshape(5, 5, 1, 1)
    y = R.conv_ref(np.ones((1, 1, 1, 1), F), w5)  # a 1 x 1 frame: only the centre tap is inside
    assert y.shape == (1, 1, 1, 1) and y[0, 0, 0, 0] == w5[2, 2, 0, 0]


def test_the_statement_tells_group_order_from_tap_order():
    """A 1 x 2 frame, Cin = 32, 3x3: the left output has two taps inside the frame, (1, 1) itself and (1, 2) its neighbour, and
    three non-zero links under weights of 1: (1, 1, c 0) = 1, (1, 1, c 16) = 2^-23, (1, 2, c 0) = 3 2^-24.  With u = 2^-23:
      groups outermost  1;  + 1.5 u, a tie, to even: 1 + 2 u;  then group 1: + u = 1 + 3 u
      taps outermost    1;  + u = 1 + u;  then tap (1, 2): + 1.5 u = 1 + 2.5 u, a tie, to even: 1 + 2 u"""
    x = np.zeros((1, 1, 2, 32), F)
    w = np.zeros((3, 3, 32, 1), F)
    x[0, 0, 0, 0], x[0, 0, 0, 16], x[0, 0, 1, 0] = 1, 2.0 ** -23, 3 * 2.0 ** -24
    w[1, 1, 0, 0] = w[1, 1, 16, 0] = w[1, 2, 0, 0] = 1
    groups = R.conv_ref(x, w)[0, 0, 0, 0]
    taps = R.conv_ref(x, w, order="taps")[0, 0, 0, 0]
    assert groups == F(1 + 3 * 2.0 ** -23) and taps == F(1 + 2.0 ** -22)
    assert sorted(R.chain_order(3, 32)) == sorted(R.chain_order(3, 32, "taps")) and R.chain_order(3, 32) != R.chain_order(3, 32, "taps")
    assert R.chain_order(3, 16) == R.chain_order(3, 16, "taps")  # one group: the two orders are one
    assert R.chain_order(3, 32)[:17] == [(0, 0, c) for c in range(16)] + [(0, 1, 0)]


def test_bias_and_activation_are_single_operations():
    x = np.ones((1, 1, 1, 1), F)
    w = np.full((1, 1, 1, 1), -3, F)
    assert R.conv_ref(x, w, F([1]), R.LEAKY, 0.2)[0, 0, 0, 0] == F(-2) * F(0.2)
    assert R.conv_ref(x, w, F([5]), R.LEAKY, 0.2)[0, 0, 0, 0] == 2 and R.conv_ref(x, w, None, R.LINEAR)[0, 0, 0, 0] == -3


# ---- the entry point, without a device -------------------------------------------------------------------------------

GOOD = dict(x=1, B=1, H=4, W=4, Cin=16, w=1, bias=1, ksize=3, Cout=16, act=1, alpha=0.2, out=1, out_channels=16, out_offset=0)
ORDER = ("x", "B", "H", "W", "Cin", "w", "bias", "ksize", "Cout", "act", "alpha", "out", "out_channels", "out_offset")


def _call(L, **change):
    a = dict(GOOD, **change)
    buf = ctypes.create_string_buffer(64)  # never read: every call here returns before any HIP call
    ptr = lambda v: ctypes.addressof(buf) if v else None
    args = [ptr(a[k]) if k in ("x", "w", "bias", "out") else a[k] for k in ORDER]
    return L.dtfill_conv2d(*args, None)


def test_return_codes_without_a_device(pkg):
    pkg.build()
    L = pkg.load()
    NULL, SHAPE = -1, -2
    for name in ("x", "w", "out"):
        assert _call(L, **{name: 0}) == NULL, name
    bad = [dict(ksize=k) for k in (0, 2, 4, 9, -1)] + [dict(Cin=c) for c in (0, 2, 8, 17, 24, 80, -16)] + \
        [dict(Cout=c) for c in (0, 2, 8, 32)] + [dict(out_offset=-1), dict(out_offset=1), dict(out_channels=15), dict(out_channels=0),
                                                  dict(Cout=1, out_channels=4, out_offset=4), dict(out_offset=2 ** 31 - 1)] + \
        [dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 15, H=1 << 8, W=1 << 8), dict(B=1 << 9, H=1 << 9, W=1 << 9),
         dict(B=1, H=1 << 13, W=1 << 13, out_channels=32), dict(B=1, H=1 << 13, W=1 << 12, Cin=64)] + \
        [dict(act=2), dict(act=-1), dict(alpha=float("nan")), dict(alpha=float("inf"))]
    for change in bad:
        assert _call(L, **change) == SHAPE, change
    assert _call(L, x=0, ksize=2) == NULL  # the pointers first, as everywhere in the ABI
    assert b"shape" in L.dtfill_strerror(SHAPE)


def test_binding_and_constants(pkg):
    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dtfill_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(pkg._lib.SYMBOLS) and pkg._lib.SYMBOLS[-1] == "dtfill_conv2d"
    pkg.build()
    L = pkg.load()
    assert len(L.dtfill_conv2d.argtypes) == 15 and L.dtfill_conv2d.restype is ctypes.c_int
    conv = dict(re.findall(r"^#define DTFILL_(CONV_\w+)[ \t]+(\d+)\b", src, flags=re.M))
    assert conv == {"CONV_LINEAR": "0", "CONV_LEAKY": "1"}
    assert (pkg._lib.CONV_LINEAR, pkg._lib.CONV_LEAKY) == (R.LINEAR, R.LEAKY) == (0, 1)
    assert pkg._lib.CONV_ACTS == {"linear": 0, "leaky": 1}
    assert re.search(r"#define DTFILL_ABI_VERSION 1\b", src) and L.dtfill_abi_version() == 1
    assert hasattr(pkg.device, "conv2d_device") and callable(pkg.conv2d)


def test_python_layer_argument_checks_without_gpu(pkg):
    import torch

    conv = pkg.device.conv2d_device
    x, w = torch.zeros((1, 4, 4, 16)), torch.zeros((3, 3, 16, 16))
    with pytest.raises(ValueError, match="act must be"):
        conv(x, w, act="relu")
    # host tensors where device tensors are asked for, and wrong ranks and dtypes, are refused before any device work
    for bad in (dict(x=x), dict(x=x.double()), dict(x=x[0, 0])):
        with pytest.raises((ValueError, RuntimeError)):
            conv(**dict(dict(x=x, w=w), **bad))
    with pytest.raises(ValueError):
        pkg.conv2d(np.zeros((4, 4, 16), F), np.zeros((3, 3, 16, 16), F))
    with pytest.raises(TypeError):
        pkg.conv2d(np.zeros((1, 4, 4, 16), complex), np.zeros((3, 3, 16, 16), F))

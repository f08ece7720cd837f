"""The bf16 convolutions without a device: the numpy statement (tests/conv_bf16_ref.py) against torch's bfloat16 rounding, an
integer convolution and the float32 statement; every return code of the four entry points (all checked before any HIP call);
dtfill_conv2d_bf16_packed_elems; and the networks' precision argument."""
import numpy as np
import pytest

import conv2_ref as R2
import conv_bf16_ref as H

F = np.float32
LOW_HALVES = (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def _same_or_both_nan(got, want):
    g, w = got.view(np.uint32), want.view(np.uint32)
    return (g == w) | (np.isnan(got) & np.isnan(want))


def _torch_round(a):
    import torch

    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_round_against_torch_on_every_upper_half():
    upper = np.arange(65536, dtype=np.uint32) << 16
    for low in LOW_HALVES:
        a = (upper | low).view(F)
        got, want = H.bf16_round(a), _torch_round(a)
        assert _same_or_both_nan(got, want).all(), "low half %#06x" % low
        assert ((got.view(np.uint32) & 0xFFFF) == 0).all()
        assert (np.isnan(got) == np.isnan(a)).all()


def test_bf16_round_against_torch_on_random_patterns():
    a = np.random.default_rng(7).integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32).view(F)
    assert _same_or_both_nan(H.bf16_round(a), _torch_round(a)).all()


def test_bf16_round_named_cases():
    cases = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80, 0x80000000: 0x8000,
             0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80}  # ties to even both ways, just above a tie, overflow to inf, -0
    a = np.array(list(cases), np.uint32).view(F)
    assert H.bf16_bits(a).tolist() == list(cases.values())
    assert np.isnan(H.bf16_round(np.array([0x7F800001], np.uint32).view(F))).all()  # a NaN whose payload is in the low half


def _ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(F)


@pytest.mark.parametrize("ksize,stride", ((3, 1), (1, 1), (3, 2), (1, 2)))
def test_statement_is_the_integer_convolution(ksize, stride):
    x, w = _ints((2, 5, 7, 48), -8, 8, 1), _ints((ksize, ksize, 48, 32), -4, 4, 2)
    b, res = _ints((32,), -9, 9, 3), _ints((2, -(-5 // stride), -(-7 // stride), 32), -9, 9, 4)
    want = R2.strided_f64(x, w, b, stride, res, R2.LEAKY, 0.5)  # torch's float64 convolution: exact on these integers
    got, S = H.conv2d_strided_bf16_ref(x, w, b, stride, res, R2.LEAKY, 0.5)
    assert (got.astype(np.float64) == want).all()
    assert (H.strided_sum(x, w, stride, np.int64) == R2.strided_f64(x, w, None, stride)).all()
    assert (S == R2.strided_f64(np.abs(x), np.abs(w), None, stride)).all()


def test_transposed_statement_is_the_integer_convolution():
    x, kernel = _ints((2, 3, 5, 48), -8, 8, 5), _ints((3, 3, 32, 48), -4, 4, 6)  # Keras' [3,3,Cout,Cin]
    b = _ints((32,), -9, 9, 7)
    got, S = H.conv2d_transpose_bf16_ref(x, R2.pack(kernel), b, R2.LEAKY, 0.5)
    assert (got.astype(np.float64) == R2.transpose_f64_vjp(x, kernel, b, R2.LEAKY, 0.5)).all()
    assert (H.transpose_sum(x, R2.pack(kernel), np.int64) == R2.transpose_f64_torch(x, kernel)).all()
    assert (S == R2.transpose_f64_torch(np.abs(x), np.abs(kernel))).all()


def _gamma(n):
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


def test_statement_against_the_float32_statement_on_bf16_exact_operands():
    """On operands that are bf16 values already the two contracts differ by the float32 chain's own error only."""
    rng = np.random.default_rng(11)
    x, w = H.bf16_round(rng.standard_normal((1, 5, 9, 48)).astype(F)), H.bf16_round(rng.standard_normal((3, 3, 48, 16)).astype(F) / 3)
    b = rng.standard_normal(16).astype(F)
    for stride in (1, 2):
        got, S = H.conv2d_strided_bf16_ref(x, w, b, stride, None, R2.LINEAR)
        want = R2.strided_ref(x, w, b, stride, None, R2.LINEAR)
        assert (np.abs(got.astype(np.float64) - want) <= _gamma(9 * 48 + 2) * (S + np.abs(b))).all()
    wt = H.bf16_round(rng.standard_normal((3, 3, 48, 16)).astype(F) / 3)
    got, S = H.conv2d_transpose_bf16_ref(x, wt, b, R2.LINEAR)
    assert (np.abs(got.astype(np.float64) - R2.transpose_ref(x, wt, b, R2.LINEAR)) <= _gamma(4 * 48 + 2) * (S + np.abs(b))).all()


def test_pack_ref_is_the_headers_index_rule():
    w = np.random.default_rng(3).standard_normal((3, 3, 48, 32)).astype(F)
    packed, bits = H.pack_ref(w), H.bf16_bits(w).reshape(9, 48, 32)
    assert packed.size == H.packed_elems(3, 48, 32) == 9 * 2 * 2 * 512
    G, N = 2, 2
    for T, g, n, kq, m, j in ((0, 0, 0, 0, 0, 0), (8, 1, 1, 1, 15, 7), (4, 0, 1, 3, 5, 2), (2, 1, 0, 0, 9, 1)):
        assert packed[(((T * G + g) * N + n) * 64 + 16 * kq + m) * 8 + j] == bits[T, 32 * g + 8 * kq + j, 16 * n + m]
    assert packed[(((5 * G + 1) * N + 1) * 64 + 16 * 2 + 3) * 8 + 4] == 0  # channel 32 + 16 + 4 = 52 is past Cin: the half group


P = 4096  # a non-NULL, 16-byte aligned address: no call below gets as far as using it
NULL, SHAPE = -1, -2


def test_packed_elems(pkg):
    L = pkg.load()
    for ksize, cin, cout in ((1, 16, 16), (3, 16, 16), (3, 48, 80), (3, 64, 64), (1, 128, 512), (3, 1024, 512)):
        assert L.dtfill_conv2d_bf16_packed_elems(ksize, cin, cout) == H.packed_elems(ksize, cin, cout)
    for ksize, cin, cout in ((5, 32, 32), (7, 32, 32), (2, 32, 32), (0, 32, 32), (3, 8, 16), (3, 0, 16), (3, 24, 16), (3, 16, 0), (3, 16, 24),
                             (3, -16, 16), (3, 16, -16), (3, 1 << 16, 1 << 15), (3, 1 << 20, 1 << 20)):
        assert L.dtfill_conv2d_bf16_packed_elems(ksize, cin, cout) == 0, (ksize, cin, cout)


def test_pack_return_codes(pkg):
    L = pkg.load()
    assert L.dtfill_conv2d_pack_bf16(None, 3, 32, 32, P, None) == NULL
    assert L.dtfill_conv2d_pack_bf16(P, 3, 32, 32, None, None) == NULL
    for ksize, cin, cout in ((5, 32, 32), (3, 8, 16), (3, 24, 16), (3, 16, 24), (3, 16, 0), (3, 1 << 16, 1 << 15)):
        assert L.dtfill_conv2d_pack_bf16(P, ksize, cin, cout, P, None) == SHAPE, (ksize, cin, cout)
    assert L.dtfill_conv2d_pack_bf16(P, 3, 32, 32, P + 8, None) == SHAPE  # out must be 16-byte aligned


def _strided(L, x=P, B=1, H=8, W=8, Cin=32, w=P, ksize=3, Cout=32, stride=1, act=0, alpha=0.2, out=P, out_channels=32, out_offset=0):
    return L.dtfill_conv2d_strided_bf16(x, B, H, W, Cin, w, None, ksize, Cout, stride, None, act, alpha, out, out_channels, out_offset, None)


def _transposed(L, x=P, B=1, H=8, W=8, Cin=32, w=P, Cout=32, act=0, alpha=0.2, out=P, out_channels=32, out_offset=0):
    return L.dtfill_conv2d_transpose_bf16(x, B, H, W, Cin, w, None, Cout, act, alpha, out, out_channels, out_offset, None)


@pytest.mark.parametrize("call", (_strided, _transposed))
def test_convolution_return_codes(pkg, call):
    L = pkg.load()
    for name in ("x", "w", "out"):
        assert call(L, **{name: None}) == NULL, name
    bad = (dict(B=0), dict(H=0), dict(W=0), dict(Cin=8), dict(Cin=24), dict(Cin=0), dict(Cout=0), dict(Cout=24), dict(Cout=8),
           dict(out_offset=-1), dict(out_offset=16), dict(out_channels=0), dict(out_channels=16), dict(act=2), dict(act=-1),
           dict(alpha=float("nan")), dict(alpha=float("inf")), dict(w=P + 4), dict(w=P + 8),
           dict(B=1 << 10, H=1 << 10, W=1 << 10), dict(B=1, H=1 << 14, W=1 << 13, Cin=16), dict(H=1 << 12, W=1 << 12, Cout=512, out_channels=512))
    for kw in bad:
        assert call(L, **kw) == SHAPE, kw
    if call is _strided:
        for kw in (dict(stride=0), dict(stride=3), dict(ksize=5), dict(ksize=7), dict(ksize=2), dict(ksize=0), dict(ksize=5, stride=2)):
            assert call(L, **kw) == SHAPE, kw


def test_precision_argument(pkg):
    net = pkg.net
    weights = net.glorot_weights_resnet18(0, scale_num=1)
    for cls, make in ((net.ResNet18, net.glorot_weights_resnet18), (net.ResNet18Image, net.glorot_weights_resnet18_image),
                      (net.ResNet18LightImage, net.glorot_weights_resnet18_light_image)):
        for bad in ("fp16", "bfloat16", None, 32, "BF16"):
            with pytest.raises(ValueError, match="precision"):
                cls({}, precision=bad)  # (refused before the weights are looked at)
        w = weights if cls is net.ResNet18 else make(0, scale_num=1)
        assert cls(w, scale_num=1).precision == "float32"
        assert cls(w, scale_num=1, precision="float32").precision == "float32"
        n = cls(w, scale_num=1, precision="bf16")
        assert n.precision == "bf16"
        # the layers that run in bf16: the trunk's, and none of the head, the stems, img_conv or conv_output
        assert set(n.shapes) - set(n.wide_layers) == set(net._head_shapes(1, True)) | ({"img_conv"} if cls.IMAGE_WIDTH else set()) | {"conv_output"}
        for name in n.wide_layers:
            ksize, cin, cout = n.shapes[name]
            assert ksize in (1, 3) and cin % 16 == 0 and cin >= 16 and cout % 16 == 0, name
    for cls in (net.ResNet18Trainable, net.ResNet18ImageTrainable, net.ResNet18LightImageTrainable, net.SparsityCNNTrainable):
        with pytest.raises(TypeError):
            cls(weights, precision="bf16")
    with pytest.raises(TypeError):
        net.SparsityCNN(net.glorot_weights(0), precision="bf16")


def test_names_are_exported(pkg):
    from importlib import import_module

    conv = import_module(pkg.__name__ + ".conv")
    for name in ("pack_bf16_device", "conv2d_strided_bf16_device", "conv2d_transpose_bf16_device", "conv2d_strided_bf16",
                 "conv2d_transpose_bf16"):
        assert getattr(pkg.device, name) is getattr(conv, name) is getattr(pkg, name) is getattr(pkg.net, name)
        assert name in pkg.__all__

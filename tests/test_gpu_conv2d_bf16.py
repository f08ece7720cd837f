"""dtfill_conv2d_strided_bf16, dtfill_conv2d_transpose_bf16 and dtfill_conv2d_pack_bf16 on the device against the numpy
statement of their contract (tests/conv_bf16_ref.py), through the ABI on guarded buffers with poisoned outputs.  The exact cases
are the indexing check, bit for bit (+0 == -0): small integers, every partial sum exact in any order, so a dropped or doubled
term at any depth of K shows, which no tolerance can see.  The random cases hold the derived bound of the contract."""
import numpy as np
import pytest

import conv2_ref as R2
import conv_bf16_ref as H
import conv_ref as R
from guarded import GuardedBuffer
from test_gpu_conv2d import DEV, POISON, _poisoned, _up

pytestmark = pytest.mark.gpu

F = np.float32
ALPHA = 0.5  # exact on the integer cases


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def packed(L, w):
    """w [ksize,ksize,Cin,Cout] through dtfill_conv2d_pack_bf16 on guarded buffers -> the guarded packed array."""
    import torch

    ksize, _, cin, cout = w.shape
    n = L.dtfill_conv2d_bf16_packed_elems(ksize, cin, cout)
    assert n == H.packed_elems(ksize, cin, cout)
    gw, gp = _up(w), GuardedBuffer(2 * n, 0, DEV)
    assert L.dtfill_conv2d_pack_bf16(gw.ptr, ksize, cin, cout, gp.ptr, None) == 0
    torch.cuda.synchronize()
    gw.check("w")
    gp.check("packed")
    return gp


def run(L, x, w, bias=None, act=R.LINEAR, stride=1, residual=None, transposed=False, alpha=ALPHA, out_channels=None, out_offset=0,
        x_offset=0, stream=None, gp=None):
    """One call through the ABI on guarded buffers; returns the whole out tensor, poison where the call wrote nothing."""
    import torch

    B, Hh, W, cin = x.shape
    ksize, cout = w.shape[0], w.shape[3]
    out_channels = cout if out_channels is None else out_channels
    shape = ((B, 2 * Hh, 2 * W) if transposed else (B, -(-Hh // stride), -(-W // stride))) + (out_channels,)
    gp = packed(L, w) if gp is None else gp
    gx = _up(x, x_offset)
    gb = None if bias is None else _up(bias)
    gr = None if residual is None else _up(residual)
    go = _poisoned(shape)
    torch.cuda.synchronize()  # the uploads are on torch's stream, the call may be on another
    if transposed:
        rc = L.dtfill_conv2d_transpose_bf16(gx.ptr, B, Hh, W, cin, gp.ptr, gb.ptr if gb else None, cout, act, alpha, go.ptr, out_channels,
                                            out_offset, stream)
    else:
        rc = L.dtfill_conv2d_strided_bf16(gx.ptr, B, Hh, W, cin, gp.ptr, gb.ptr if gb else None, ksize, cout, stride,
                                          gr.ptr if gr else None, act, alpha, go.ptr, out_channels, out_offset, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in ((gx, "x"), (gp, "packed w"), (go, "out"), (gb, "bias"), (gr, "residual")):
        if g is not None:
            g.check(what)
    return go.view(torch.float32, shape).cpu().numpy()


def ref(x, w, bias=None, act=R.LINEAR, stride=1, residual=None, transposed=False, alpha=ALPHA):
    """(the statement's output, S)"""
    if transposed:
        return H.conv2d_transpose_bf16_ref(x, w, bias, act, alpha)
    return H.conv2d_strided_bf16_ref(x, w, bias, stride, residual, act, alpha)


def out_frame(shape, stride, transposed):
    B, Hh, W = shape
    return (B, 2 * Hh, 2 * W) if transposed else (B, -(-Hh // stride), -(-W // stride))


# (name, ksize, stride, transposed, (B,H,W), Cin, Cout, out_channels, out_offset, residual): the shapes of every test below
CASES = (
    ("3x3 two tile rows, a column remainder, a half group, a pass and one N-tile", 3, 1, False, (2, 9, 33), 48, 80, 96, 16, True),
    ("1x1 stride 1", 1, 1, False, (2, 9, 33), 48, 32, 32, 0, True),
    ("1x1 stride 2", 1, 2, False, (2, 9, 33), 48, 32, 32, 0, True),
    ("3x3 stride 2, odd H (pt = 1)", 3, 2, False, (2, 9, 66), 32, 32, 32, 0, True),
    ("3x3 stride 2, even H (pt = 0)", 3, 2, False, (2, 8, 66), 32, 32, 32, 0, False),
    ("transposed", 3, 2, True, (2, 9, 33), 48, 32, 48, 16, False),
    ("3x3 K = 4608", 3, 1, False, (2, 8, 8), 512, 16, 16, 0, True),
)
IDS = [c[0] for c in CASES]


def integer_case(ksize, shape, cin, cout, stride, transposed, residual, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, shape + (cin,)).astype(F)
    w = rng.integers(-4, 5, (ksize, ksize, cin, cout)).astype(F)
    b = rng.integers(-9, 10, cout).astype(F)
    res = rng.integers(-9, 10, out_frame(shape, stride, transposed) + (cout,)).astype(F) if residual else None
    return x, w, b, res


def int64_finish(total, bias, residual, alpha):
    y = total.astype(np.float64) + bias + (0 if residual is None else residual)
    return np.where(y > 0, y, y * alpha).astype(F)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_integer_cases_bit_for_bit(L, case):
    name, ksize, stride, transposed, shape, cin, cout, out_channels, out_offset, residual = case
    x, w, b, res = integer_case(ksize, shape, cin, cout, stride, transposed, residual, 1)
    total = H.transpose_sum(x, w, np.int64) if transposed else H.strided_sum(x, w, stride, np.int64)
    want = int64_finish(total, b, res, ALPHA)  # every partial sum is an integer below 2^24: exact in any order
    R.assert_same(ref(x, w, b, R.LEAKY, stride, res, transposed)[0], want, "the statement, " + name)
    got = run(L, x, w, b, R.LEAKY, stride, res, transposed, out_channels=out_channels, out_offset=out_offset)
    R.assert_same(got[..., out_offset:out_offset + cout], want, name)
    rest = np.delete(got, np.s_[out_offset:out_offset + cout], axis=-1)
    assert (rest.view(np.uint32) == POISON).all(), "channels outside the slice were written"


def test_exact_on_a_misaligned_x(L):
    """x 4 bytes off a 16-byte boundary: the kernels without 16-byte loads."""
    for ksize, stride, transposed, shape in ((3, 1, False, (2, 9, 33)), (3, 2, False, (1, 9, 66)), (3, 2, True, (1, 9, 33))):
        x, w, b, res = integer_case(ksize, shape, 48, 32, stride, transposed, not transposed, 2)
        total = H.transpose_sum(x, w, np.int64) if transposed else H.strided_sum(x, w, stride, np.int64)
        got = run(L, x, w, b, R.LEAKY, stride, res, transposed, x_offset=4)
        R.assert_same(got, int64_finish(total, b, res, ALPHA), "misaligned x, stride %d, transposed %s" % (stride, transposed))


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (2, True)))
def test_one_hot_sweep(L, stride, transposed):
    """Frame b holds a single 1, at pixel b of a 10 x 34 frame, under weights that name their tap and channel: which tap meets
    which pixel, at every tile seam."""
    Hh, W, cin, cout = 10, 34, 16, 16
    x = np.zeros((Hh * W, Hh, W, cin), F)
    b = np.arange(Hh * W)
    x[b, b // W, b % W, b % cin] = 1
    t, c, o = np.meshgrid(np.arange(9), np.arange(cin), np.arange(cout), indexing="ij")
    w = ((t * cin + c + 1 + o // 2) * np.where(o % 2, -1, 1)).astype(F).reshape(3, 3, cin, cout)  # |w| <= 151: bf16 values
    assert (H.bf16_round(w) == w).all() and np.unique(w).size == 2 * (9 * cin + cout // 2 - 1)
    total = H.transpose_sum(x, w, np.int64) if transposed else H.strided_sum(x, w, stride, np.int64)
    R.assert_same(run(L, x, w, None, R.LINEAR, stride, None, transposed), total.astype(F), "one-hot sweep")


TABLE = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF,
                  0x80000000, 0x00000000, 0x7FC00000, 0x7F800001, 0xFFC00001, 0x7F800000, 0x3F800000, 0x40490FDB, 0xC2F6E979,
                  0x00800000, 0x477FE000, 0x33800000, 0x3F7FFFFF], np.uint32).view(F)
# ties both ways (even stays, odd goes up), either sign, just above and below a tie, the largest finite float32 (-> inf) and the
# largest that stays finite, -0, +0, NaNs (one with its payload in the low half only), inf, and ordinary values


def test_rounding_table_through_x(L):
    """A 1x1 layer with weight 1 on one channel and 0 elsewhere returns bf16(x) bit for bit (a NaN as a NaN)."""
    n = TABLE.size
    x = np.zeros((1, 1, n, 16), F)
    x[0, 0, :, 5] = TABLE
    w = np.zeros((1, 1, 16, 16), F)
    w[0, 0, 5, 3] = 1
    got = run(L, x, w)[0, 0, :, 3]
    R.assert_same(got, H.bf16_round(TABLE), "bf16(x)")
    x = np.zeros((1, 2, n + 7, 16), F)  # and off the 16-byte path
    x[0, 1, 7:, 5] = TABLE
    R.assert_same(run(L, x, w, x_offset=4)[0, 1, 7:, 3], H.bf16_round(TABLE), "bf16(x), misaligned")


def test_rounding_table_through_the_pack_function(L):
    import torch

    n = TABLE.size
    cout = 16 * -(-n // 16)
    w = np.zeros((1, 1, 16, cout), F)
    w[0, 0, 5, :n] = TABLE
    x = np.zeros((1, 1, 1, 16), F)
    x[..., 5] = 1
    R.assert_same(run(L, x, w)[0, 0, 0, :n], H.bf16_round(TABLE), "bf16(w)")
    # the packed array itself is the statement's, NaNs as NaNs: a half group (Cin 48) and three N-tiles
    w = np.random.default_rng(5).standard_normal((3, 3, 48, 48)).astype(F)
    w.reshape(-1)[:n] = TABLE
    got = packed(L, w).view(torch.int16, (H.packed_elems(3, 48, 48),)).cpu().numpy().view(np.uint16)
    want = H.pack_ref(w)
    as_f32 = lambda a: (a.astype(np.uint32) << 16).view(F)
    R.assert_same(as_f32(got), as_f32(want), "packed layout")


def normal_case(ksize, shape, cin, cout, stride, transposed, residual, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (cin,)).astype(F)
    w = rng.standard_normal((ksize, ksize, cin, cout)).astype(F)
    b = rng.standard_normal(cout).astype(F)
    res = rng.standard_normal(out_frame(shape, stride, transposed) + (cout,)).astype(F) if residual else None
    return x, w, b, res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_data_within_the_contracts_bound(L, case):
    name, ksize, stride, transposed, shape, cin, cout, out_channels, out_offset, residual = case
    x, w, b, res = normal_case(ksize, shape, cin, cout, stride, transposed, residual, 3)
    want, S = ref(x, w, b, R.LEAKY, stride, res, transposed, 0.2)
    got = run(L, x, w, b, R.LEAKY, stride, res, transposed, 0.2)
    err, lim = np.abs(got.astype(np.float64) - want), H.bound(ksize, cin, S, b, res)
    print("%s: max |out - ref| / bound = %.4g (max err %.3g)" % (name, (err / lim).max(), err.max()))
    assert (err <= lim).all(), "%s: %d outputs outside the bound, worst ratio %g" % (name, (err > lim).sum(), (err / lim).max())


def test_bits_do_not_depend_on_the_batch_position_the_call_or_the_stream(L):
    import torch

    for name, ksize, stride, transposed, shape, cin, cout, _, _, residual in CASES[:1] + CASES[3:4] + CASES[5:6]:
        x, w, b, res = normal_case(ksize, (1,) + shape[1:], cin, cout, stride, transposed, residual, 4)
        x3 = np.repeat(x, 3, axis=0)
        res3 = None if res is None else np.repeat(res, 3, axis=0)
        gp = packed(L, w)
        first = run(L, x3, w, b, R.LEAKY, stride, res3, transposed, gp=gp)
        assert not np.isnan(first).any()
        assert (first[1].view(np.uint32) == first[0].view(np.uint32)).all() and (first[2].view(np.uint32) == first[0].view(np.uint32)).all(), name
        again = run(L, x3, w, b, R.LEAKY, stride, res3, transposed, gp=gp)
        assert (again.view(np.uint32) == first.view(np.uint32)).all(), name + ": two calls"
        s = torch.cuda.Stream(DEV)
        other = run(L, x3, w, b, R.LEAKY, stride, res3, transposed, gp=gp, stream=s.cuda_stream)
        assert (other.view(np.uint32) == first.view(np.uint32)).all(), name + ": two streams"
        alone = run(L, x, w, b, R.LEAKY, stride, res, transposed, gp=gp)
        assert (alone[0].view(np.uint32) == first[0].view(np.uint32)).all(), name + ": B = 1 against B = 3"


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (2, True)))
def test_bits_do_not_depend_on_the_tile_position(L, stride, transposed):
    """The same 8 x 32 patch at three places of a zero frame, tile-aligned and not: the outputs it reaches have the same bits."""
    rng = np.random.default_rng(6)
    patch = rng.standard_normal((8, 32, 48)).astype(F)
    w = rng.standard_normal((3, 3, 48, 32)).astype(F)
    gp = packed(L, w)
    outs = []
    for r0, c0 in ((2, 2), (8, 32), (6, 18)):  # (even offsets: a stride-2 layer sees the patch at the same phase)
        x = np.zeros((1, 24, 96, 48), F)
        x[0, r0:r0 + 8, c0:c0 + 32] = patch
        y = run(L, x, w, None, R.LINEAR, stride, None, transposed, gp=gp)[0]
        if transposed:
            outs.append(y[2 * r0 - 2:2 * r0 + 18, 2 * c0 - 2:2 * c0 + 66])
        else:
            outs.append(y[(r0 - 2) // stride:(r0 + 10) // stride, (c0 - 2) // stride:(c0 + 34) // stride])
    assert np.abs(outs[0]).max() > 0
    for k in (1, 2):
        assert outs[k].shape == outs[0].shape and (outs[k].view(np.uint32) == outs[0].view(np.uint32)).all(), k


@pytest.mark.parametrize("stride,transposed", ((1, False), (2, False), (2, True)))
def test_a_nan_reaches_exactly_the_outputs_whose_window_holds_it(L, stride, transposed):
    x, w, b, res = normal_case(3, (1, 9, 34), 48, 32, stride, transposed, not transposed, 8)
    gp = packed(L, w)
    clean = run(L, x, w, b, R.LEAKY, stride, res, transposed, gp=gp)
    bad = x.copy()
    bad[0, 4, 17, 40] = np.nan
    got = run(L, bad, w, b, R.LEAKY, stride, res, transposed, gp=gp)
    hot = np.zeros_like(x)
    hot[0, 4, 17, 40] = 1
    wone = np.ones_like(w)
    reach = (H.transpose_sum(hot, wone) if transposed else H.strided_sum(hot, wone, stride)) > 0  # the outputs with the pixel in their window
    assert reach.any() and not reach.all()
    assert np.isnan(got[reach]).all()
    assert (got[~reach].view(np.uint32) == clean[~reach].view(np.uint32)).all()

"""dtfill_conv2d_strided_bf16 and dtfill_conv2d_transpose_bf16 (k_convh_wide) where tests/test_gpu_conv2d_bf16.py does not go, by
the method and with the machinery of tests/test_gpu_conv2d_limits.py (tests/conv_cases.py has the cases: HLOOP, HLARGE, HREFUSED,
HCLASSES; tests/test_conv_cases.py what they are held to on the CPU):

A. past CV_MAX_BLOCKS = 2^20 work items, where a block of k_convh_wide takes a second item, restages its LDS tile and asks for
   its weights anew: all five geometries at Cin = Cout = 16, one case with a half group and two groups an item (Cin 48), one
   with two passes and a residual (Cout 128), and a stride-2 and the transposed case again on the VEC = false body;
B. x, out and residual past byte offset 4 GiB, a case past 2 GiB and one at the shape rule's largest batch per entry point, and
   the calls that stand exactly at 2^31 elements refused;
C. bf16's range: S next to FLT_MAX, one-signed sums beyond it, products and sums below 2^-126, subnormal bf16 operands.

A and B: bf16 output bits are not stated by a chain, so the tiles are small integers whose partial sums are exact in any order;
the contract then promises the exact result and the comparison is bit for bit on the device against an int64 sum, on poisoned
outputs, with the inputs compared again afterwards.  C runs through test_gpu_conv2d_bf16.run on guarded buffers.

What C measured (one MI355X; profiles/r33/limits.txt): the matrix cores underflow gradually.  No small product or partial sum is
flushed; the worst error is 0.036 of the bound with its absolute term n 2^-149, and 6.7 x 2^-149 at n = 288 where S is below
2^-126 and every addition exact.  Subnormal bf16 operands are kept, in x and in w.  Sums with S below FLT_MAX stay finite and
one-signed sums beyond it are infinite.

Mutation check (each built once on a scratch copy and run once; profiles/r33/limits.txt has them beside every case's device bytes
and duration):
  the item loop left after the first item    all eight cases of A fail (frames 349525 .., 524288 .., 87381 .. still poison), and the
                                             transposed case at the limit; no test of test_gpu_conv2d_bf16.py fails.
  a later item keeps its first item's tile   the cases with 3 and 12 items a frame fail in the one frame where item 2^20 lies
                                             (349525, 87381); the case with two items a frame passes, as it must.
  a 32-bit byte offset for a frame of x      "x past 4 GiB" fails, first mismatching frames 56489, 56490, 56491: exactly the frames
                                             that start past 4 GiB; the two cases at the limit fail from there on.
  the same for the store's pixel offset      "out and residual past 4 GiB" and the transposed "out past 4 GiB" fail: frames 0 .. 3
                                             overwritten, 56488 .. 56491 still poison.
  ch_round truncates                         the rounding tables and the random-data bound of test_gpu_conv2d_bf16.py fail, and so do
                                             all four cases of C's class 1 (worst ratio 61 to 580): the range classes do not mask it.
"""
import numpy as np
import pytest

import conv_bf16_ref as H
import conv_cases as CC
import conv_ref as R
import large_cases as LC
import test_gpu_conv2d_bf16 as HT
from test_gpu_conv2d_limits import DEV, L, _release, _tile, _up, poisoned, tiled, unchanged  # noqa: F401 (L, _release: fixtures)
from test_gpu_large import need, no_mismatch

pytestmark = pytest.mark.gpu

F = np.float32
T = CC.T


def _ptr(t):
    return None if t is None else t.data_ptr()


def call(L, c, x, w, bias, res, out):
    """The bf16 entry point of case c on raw pointers."""
    oc, at = c.get("out_channels", c["cout"]), c.get("out_offset", 0)
    if c["entry"] == "transpose":
        return L.dtfill_conv2d_transpose_bf16(x, c["B"], c["H"], c["W"], c["cin"], w, bias, c["cout"], R.LEAKY, CC.HALPHA, out, oc, at, None)
    return L.dtfill_conv2d_strided_bf16(x, c["B"], c["H"], c["W"], c["cin"], w, bias, c["ksize"], c["cout"], c["stride"], res, R.LEAKY,
                                        CC.HALPHA, out, oc, at, None)


def run_tiled(L, what, c, chunk, mis=0):
    """Case c of conv_cases.HLOOP or HLARGE: the call on a tiled batch, the comparison on the device, the inputs afterwards."""
    import torch

    d = _tile(what, c)
    B = c["B"]
    for name, period in CC.periods(c, d):
        LC.assert_alias_free(T, period // T)
    need(CC.device_bytes(c, chunk), "%s%s: B %d, %d work items" % (what, ", x 4 bytes off" if mis else "", B, CC.items(c)))
    gp = HT.packed(L, d["w"])  # packed once, through dtfill_conv2d_pack_bf16, on a guarded buffer
    x, b, res = tiled(d["x"], B, mis), _up(d["bias"]), tiled(d["residual"], B)
    out = poisoned((B,) + CC.out_frame(c) + (c.get("out_channels", c["cout"]),))
    torch.cuda.synchronize()
    rc = call(L, c, x.data_ptr(), gp.ptr, b.data_ptr(), _ptr(res), out.data_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    # `want` is the whole out tensor of a period: the channels beside the slice hold the poison, which must have survived
    no_mismatch(LC.mismatching_frames(out, _up(d["want"]), B, chunk_bytes=chunk), what + ": out")
    unchanged((("x", x, d["x"]), ("residual", res, d["residual"])), B, what, chunk)
    gp.check("packed w")
    assert torch.equal(b, _up(d["bias"]))


# ================================================================================================ A. past 2^20 work items
LOOP_RUNS = [(name, 0) for name in CC.HLOOP] + [(name, 4) for name, c in CC.HLOOP.items() if c.get("misaligned")]


@pytest.mark.parametrize("name,mis", LOOP_RUNS, ids=["%s%s" % (n, ", x 4 bytes off" if m else "") for n, m in LOOP_RUNS])
def test_a_block_takes_a_second_work_item(L, name, mis):
    c = CC.HLOOP[name]
    assert CC.MAX_BLOCKS < CC.items(c) < CC.MAX_BLOCKS + 2 ** 10
    run_tiled(L, name, c, CC.COMPARE_CHUNK, mis)


# ================================================================================================ B. large tensors
@pytest.mark.parametrize("name", list(CC.HLARGE))
def test_tensors_past_2_gib_4_gib_and_at_the_limit(L, name):
    run_tiled(L, name, CC.HLARGE[name], LC.CHUNK_BYTES)


def test_calls_at_2_to_the_31_elements_are_refused(L):
    """Exactly 2^31 elements of x and of out (by Cout and by out_channels), either entry point: DTFILL_ERR_SHAPE before any launch,
    so that small real buffers serve.  The calls just below each rule, which must run, are the "at the limit" cases above."""
    import torch

    buf = lambda: torch.zeros(4096, dtype=torch.float32, device=DEV)  # noqa: E731
    x, w, b, out = buf(), buf(), buf(), buf()
    assert w.data_ptr() % 16 == 0
    for entry, what, a in CC.HREFUSED:
        assert CC.refused_count(entry, a) == 2 ** 31
        c = dict(a, entry=entry)
        assert call(L, c, x.data_ptr(), w.data_ptr(), b.data_ptr(), None, out.data_ptr()) == CC.ERR_SHAPE, (entry, what)
    torch.cuda.synchronize()
    for t in (x, w, b, out):
        assert not t.any()


# ================================================================================================ C. bf16's range
def _layers(f):
    return pytest.mark.parametrize("ksize,stride,transposed,cin,cout", CC.HLAYERS, ids=CC.HLAYER_IDS)(f)


@_layers
def test_sums_next_to_flt_max_stay_finite_and_within_the_bound(L, ksize, stride, transposed, cin, cout):
    """The largest S of the outputs lies in [FLT_MAX / 4, FLT_MAX / 2): no partial sum in any order can overflow, so the device
    must give finite outputs within bound (b).  x and w go in unrounded: the rounding is the kernel's (and the statement's)."""
    for seed, shape in enumerate(CC.SMALL_SHAPES):
        x, w, b = CC.hclass_case("near the top", ksize, cin, cout, shape, seed, stride, transposed)
        want, S = HT.ref(x, w, b, R.LEAKY, stride, None, transposed, CC.ALPHA)
        assert CC.FLT_MAX / 8 <= S.max() < CC.FLT_MAX / 2
        got = HT.run(L, x, w, b, R.LEAKY, stride, None, transposed, CC.ALPHA)
        assert np.isfinite(got).all()
        err, lim = np.abs(got.astype(np.float64) - want), H.bound(ksize, cin, S, b)
        print("near the top, %s: max S / FLT_MAX = %.3g, max |out - ref| / bound = %.4g" % (shape, S.max() / CC.FLT_MAX, (err / lim).max()))
        assert (err <= lim).all(), "%d outputs outside the bound, worst ratio %g" % ((err > lim).sum(), (err / lim).max())


@_layers
@pytest.mark.parametrize("sign", (1, -1), ids=("positive", "negated w"))
def test_one_signed_sums_beyond_flt_max_are_infinite(L, sign, ksize, stride, transposed, cin, cout):
    """Every product has one sign and the exact sum lies beyond FLT_MAX by more than the bound: the partial sums are monotone in
    any order, so the output is +inf (negated w: -inf).  Mixed-sign sums with S beyond FLT_MAX are open (an inner order may meet
    inf - inf) and are not tested."""
    for seed, shape in enumerate(CC.SMALL_SHAPES):
        x, w, _ = CC.hclass_case("over the top", ksize, cin, cout, shape, seed, stride, transposed, sign)
        got = HT.run(L, x, w, None, R.LEAKY, stride, None, transposed, CC.ALPHA)
        assert (got == sign * np.inf).all(), "%s: %d outputs are not %sinf" % (shape, (got != sign * np.inf).sum(), "-" if sign < 0 else "+")


def exact(x, w, b, stride, transposed):
    """(the sum and the finish in float64, S) for operands that are bf16 values: every float64 step here is exact or rounds at
    2^-53 of a value below 2^-100, far below 2^-149."""
    total = H.transpose_sum(x, w) if transposed else H.strided_sum(x, w, stride)
    S = H.transpose_sum(np.abs(x), np.abs(w)) if transposed else H.strided_sum(np.abs(x), np.abs(w), stride)
    y = total + (0 if b is None else b.astype(np.float64))
    return np.where(y > 0, y, y * np.float64(F(CC.ALPHA))), S


@_layers
@pytest.mark.parametrize("name", ("small products", "tiny products"))
def test_products_and_sums_below_2_to_the_minus_126(L, name, ksize, stride, transposed, cin, cout):
    """Normal bf16 operands whose products and sums lie from 2^-149 to 2^-120, where a product of two bf16 values is no longer
    exact in float32.  Held to the contract's bound with its absolute term, n 2^-149, and no further slack; the worst error is
    printed in units of 2^-149 and of 2^-126 beside n.  "tiny products" has S below 2^-126 in every output: every partial sum in
    any order is subnormal and every addition exact, the products' roundings are all there is, and the absolute term alone must
    hold."""
    n = H.bound_terms(ksize, cin)
    for seed, shape in enumerate(CC.SMALL_SHAPES):
        x, w, b = CC.hclass_case(name, ksize, cin, cout, shape, seed, stride, transposed)
        want, S = exact(x, w, b, stride, transposed)
        got = HT.run(L, x, w, b, R.LEAKY, stride, None, transposed, CC.ALPHA).astype(np.float64)
        err, lim = np.abs(got - want), H.bound(ksize, cin, S, b)
        print("%s, %s: n = %d, max |out - exact| = %.4g x 2^-149 = %.4g x 2^-126, max err / bound = %.4g, outputs below 2^-126: "
              "%.2f, zeros among them: %d" % (name, shape, n, err.max() * 2.0 ** 149, err.max() * 2.0 ** 126, (err / lim).max(),
                                              (np.abs(want) < 2.0 ** -126).mean(), ((got == 0) & (np.abs(want) >= 2.0 ** -149)).sum()))
        assert (err <= lim).all(), "%d outputs outside the bound, worst ratio %g" % ((err > lim).sum(), (err / lim).max())
        if name == "tiny products":
            assert S.max() < 2.0 ** -126 and (err <= n * H.TINY).all(), "worst error %g x 2^-149" % (err.max() * 2.0 ** 149)


@_layers
@pytest.mark.parametrize("name", ("subnormal x", "subnormal w"))
def test_subnormal_bf16_operands_are_kept_or_flushed_as_one(L, name, ksize, stride, transposed, cin, cout):
    """The contract leaves subnormal bf16 operands open: an output is right if it is within the bound of the reference with the
    operands kept or of the one with them flushed to zeros of their sign.  But one call must match one of the two throughout:
    bits that depend on the tile or the lane would show as a mixture."""
    for seed, shape in enumerate(CC.SMALL_SHAPES):
        x, w, b = CC.hclass_case(name, ksize, cin, cout, shape, seed, stride, transposed)
        got = HT.run(L, x, w, b, R.LEAKY, stride, None, transposed, CC.ALPHA).astype(np.float64)
        ok = {}
        for which, (xx, ww) in (("kept", (x, w)), ("flushed", (CC.flushed(x), CC.flushed(w)))):
            want, S = exact(xx, ww, b, stride, transposed)
            ok[which] = np.abs(got - want) <= H.bound(ksize, cin, S, b)
        print("%s, %s: within the bound of kept: %.3f of the outputs, of flushed: %.3f" % (name, shape, ok["kept"].mean(), ok["flushed"].mean()))
        assert (ok["kept"] | ok["flushed"]).all(), "%d outputs match neither reference" % (~(ok["kept"] | ok["flushed"])).sum()
        assert ok["kept"].all() or ok["flushed"].all(), "some outputs match the kept operands, some the flushed ones"

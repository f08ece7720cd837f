"""A literal numpy statement of dtfill_conv2d's contract (include/dtfill.h), for the tests only: one float32 fmaf chain per
output, groups of 16 input channels outermost, then the taps in raster order, then the group's channels; padding taps are
links of the chain with a = +0.0.  The product does not import this file.

fma32 is a correctly rounded float32 fused multiply-add on arrays.  Python 3.10 has no math.fma, and
float32(float64(a) * b + c) rounds twice.  Here the product is exact in float64 (24 + 24 bits), the float64 sum s = p + c is
rounded once, and rounding s to float32 is the second rounding.  The two roundings differ from one only where s lies exactly
on the midpoint of two neighbouring float32 values while the exact sum does not: there round-to-even picks by s alone, and the
exact sum p + c = s + err (err by TwoSum, exact) lies on err's side.  Those elements are found by their bits and redone.
"""
import numpy as np

F = np.float32
GROUP = 16  # input channels per group of the chain
LINEAR, LEAKY = 0, 1
# (ksize, Cin, Cout, act) of every layer of SparsityCNN (net.py:11-69), scale_num 1..4 (conv1a reads 16 scale_num channels)
NET_LAYERS = ((7, 1, 16, LEAKY), (5, 16, 16, LEAKY), (3, 16, 16, LEAKY), (3, 16, 1, LINEAR), (3, 1, 16, LEAKY),
              (7, 16, 16, LEAKY), (7, 32, 16, LEAKY), (7, 48, 16, LEAKY), (7, 64, 16, LEAKY), (1, 16, 1, LINEAR))


def _midpoints(s, r):
    """Where float64 s lies exactly halfway between two neighbouring float32 values, r = float32(s) being one of them."""
    with np.errstate(over="ignore", invalid="ignore"):
        r64 = r.astype(np.float64)
        cand = np.isfinite(r64) & (r64 != s)
        other = np.where(r64 < s, np.nextafter(r, F(np.inf)), np.nextafter(r, F(-np.inf))).astype(np.float64)
        return cand & np.isfinite(other) & (2.0 * s == r64 + other)  # (both sides exact: a 25-bit sum, a doubling)


def fma32(a, b, c):
    """float32(a * b + c) with one rounding, elementwise on float32 arrays (broadcast); NaN and inf as IEEE has them."""
    a, b, c = (np.asarray(v, F) for v in (a, b, c))
    shape = np.broadcast_shapes(a.shape, b.shape, c.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = np.atleast_1d(p + c64)
        r = s.astype(F)
        # a midpoint of the float32 grid has, as a float64, bit 28 set and bits 0..27 clear when its float32 neighbours are
        # normal; below 2^-125 the grid is coarser and every non-zero element is looked at
        maybe = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | ((np.abs(s) < 2.0 ** -125) & (s != 0))
        if maybe.any():
            k = np.nonzero(maybe)
            sk, rk = s[k], r[k]
            pk, ck = np.broadcast_to(p, s.shape)[k], np.broadcast_to(c64, s.shape)[k]
            bb = sk - pk
            err = (pk - (sk - bb)) + (ck - bb)  # TwoSum: p + c == s + err exactly
            above = rk.astype(np.float64) > sk
            hi = np.where(above, rk, np.nextafter(rk, F(np.inf)))
            lo = np.where(above, np.nextafter(rk, F(-np.inf)), rk)
            r[k] = np.where(_midpoints(sk, rk) & (err != 0), np.where(err > 0, hi, lo), rk)
    return r.reshape(shape)


def padded(x, r):
    """x [B,H,W,Cin] with r pixels of +0.0 on every side of each frame."""
    return np.pad(np.asarray(x, F), ((0, 0), (r, r), (r, r), (0, 0)))


def chain_order(ksize, cin, order="groups"):
    """The links (i, j, c) of one output's chain, in order.  "groups" is the contract; "taps" is the tap-outermost order it is
    told apart from in the tests."""
    groups = [range(g, min(g + GROUP, cin)) for g in range(0, cin, GROUP)]
    if order == "groups":
        return [(i, j, c) for g in groups for i in range(ksize) for j in range(ksize) for c in g]
    return [(i, j, c) for i in range(ksize) for j in range(ksize) for g in groups for c in g]


def finish(acc, bias, act, alpha):
    y = np.asarray(acc, F)
    with np.errstate(over="ignore", invalid="ignore"):
        if bias is not None:
            y = y + np.asarray(bias, F)
        if act == LEAKY:
            y = np.where(y > 0, y, y * F(alpha))
    return y.astype(F)


def conv_ref(x, w, bias=None, act=LINEAR, alpha=0.2, order="groups"):
    """x float32 [B,H,W,Cin], w [ksize,ksize,Cin,Cout], bias [Cout] or None -> float32 [B,H,W,Cout], the contract."""
    x, w = np.asarray(x, F), np.asarray(w, F)
    B, H, W, cin = x.shape
    ksize, _, _, cout = w.shape
    assert w.shape == (ksize, ksize, cin, cout) and ksize % 2 == 1
    xp = padded(x, (ksize - 1) // 2)
    acc = np.zeros((B, H, W, cout), F)
    for i, j, c in chain_order(ksize, cin, order):
        acc = fma32(xp[:, i:i + H, j:j + W, c:c + 1], w[i, j, c], acc)
    return finish(acc, bias, act, alpha)


def abs_sum(x, w, bias=None):
    """sum |x| |w| + |bias| per output, in float64: what the rounding bound of a float32 evaluation scales with."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, cin = x.shape
    ksize = w.shape[0]
    r = (ksize - 1) // 2
    xp = np.abs(np.pad(x, ((0, 0), (r, r), (r, r), (0, 0))))
    total = np.zeros((B, H, W, w.shape[3]))
    for i in range(ksize):
        for j in range(ksize):
            total += xp[:, i:i + H, j:j + W] @ np.abs(w[i, j])
    return total + (0 if bias is None else np.abs(np.asarray(bias, np.float64)))


def gamma(n):
    """The standard bound on n float32 roundings in sequence: n u / (1 - n u), u = 2^-24."""
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


def same_bits(got, want):
    """Elementwise: the same float32 bits, +0 == -0, and a NaN matches any NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return (got == want) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~same_bits(got, want))
    if bad.size:
        k = tuple(bad[0])
        raise AssertionError("%s: %d of %d outputs differ, first at %s: got %r (%#x), want %r (%#x)" % (
            what, len(bad), got.size, k, got[k], np.asarray(got[k], F).view(np.uint32), want[k], np.asarray(want[k], F).view(np.uint32)))

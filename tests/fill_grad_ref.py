"""The backward pass of the exact fill, stated literally in numpy and Python integers (helpers only: no tests, no fixtures).

Written from include/dtfill.h (dtfill_fill_backward) and the reference's gather, tools.py:22-26:
    with_value = x > val_thr;  depth_list = x[with_value];  out = depth_list[lbl - 1]
numpy wraps a negative index once (oracle/dtfill_oracle.c:174-176 says it the same way) and raises IndexError beyond that.  The
transposed gather sends grad_depth[p] to the (lbl[p] - 1)-th valued pixel; the sum of a cell is S(C) of the header, computed
here in unbounded Python integers and exact fractions, the two float32 roundings done in integers.
"""
from fractions import Fraction

import numpy as np

F = np.float32
QNAN = np.uint32(0x7FC00000)
INDEX_ERROR = 1  # DTFILL_FRAME_INDEX_ERROR


def _rhe_shift(a, r):
    """a / 2^r for integers a >= 0, r >= 0, rounded half to even."""
    if r == 0:
        return a
    q, rem, half = a >> r, a & ((1 << r) - 1), 1 << (r - 1)
    return q + 1 if rem > half or (rem == half and q & 1) else q


def f32_of_int(T):
    """The single round-to-nearest-even conversion of the integer T to float32, as (mantissa, exponent): T ~ m * 2^e with
    |m| <= 2^24.  (np.float32(int) goes through a double and rounds twice above 2^53.)"""
    a = abs(T)
    sh = max(a.bit_length() - 24, 0)
    m = _rhe_shift(a, sh)
    return (-m if T < 0 else m), sh


def ldexp_f32(m, e):
    """m * 2^e (|m| <= 2^24) rounded once to float32, IEEE: subnormal results round half to even on the 2^-149 grid, overflow
    gives the infinity."""
    if m == 0:
        return F(0.0)
    a = abs(m)
    top = a.bit_length() - 1 + e  # the true exponent
    if top > 127:
        v = float("inf")
    elif top >= -126:
        v = float(Fraction(a) * Fraction(2) ** e)  # at most 24 significant bits: exact in a double, and in float32
    else:
        k = _rhe_shift(a, -149 - e) if e < -149 else a << (e + 149)  # in units of 2^-149
        v = float(Fraction(k) * Fraction(2) ** -149)  # (k may round up to 2^23: the smallest normal, still exact)
    return F(-v if m < 0 else v)


def true_exponent(g):
    """floor(log2 |g|) of a finite non-zero float32, subnormals by their true exponent."""
    u = int(np.array([g], F).view(np.uint32)[0])
    ef, fr = (u >> 23) & 0xFF, u & 0x7FFFFF
    return ef - 127 if ef else fr.bit_length() - 1 - 149


def cell_sum(terms):
    """S(C) of include/dtfill.h for a sequence of float32 terms, as a float32."""
    terms = np.asarray(terms, F).reshape(-1)  # (the classification on the whole array: a frame has a term per pixel)
    nan = bool(np.isnan(terms).any())
    pinf = bool(np.isposinf(terms).any())
    ninf = bool(np.isneginf(terms).any())
    if nan or (pinf and ninf):
        return np.array([QNAN], np.uint32).view(F)[0]
    if pinf or ninf:
        return F(np.inf) if pinf else F(-np.inf)
    finite = terms[terms != 0]
    if not finite.size:
        return F(0.0)
    q = true_exponent(np.abs(finite).max()) - 37  # the largest magnitude has the largest exponent
    T = sum(round(Fraction(float(g)) / Fraction(2) ** q) for g in finite)  # round(Fraction): half to even
    m, e = f32_of_int(T)
    return ldexp_f32(m, e + q)


def cell_bound(terms, exact):
    """The header's error bound of S(C) against the exact sum, for finite terms: |C| 2^(E-38) + 2^-24 |exact| + 2^-149."""
    finite = [g for g in terms if g != 0]
    if not finite:
        return 0.0
    E = max(true_exponent(g) for g in finite)
    return len(terms) * 2.0 ** (E - 38) + 2.0 ** -24 * abs(exact) + 2.0 ** -149


def frame_cells(x, index, val_thr):
    """One frame: (pixels of the value list in raster order as flat indices, idx per pixel as int64 flat, ok).  ok is False for
    an index-error frame: some idx outside [0, n) after the one wrap."""
    with np.errstate(invalid="ignore"):
        valued = np.flatnonzero(x.reshape(-1) > F(val_thr))
    n = valued.size
    idx = index.reshape(-1).astype(np.int64) - 1
    idx = np.where(idx < 0, idx + n, idx)
    ok = bool(((idx >= 0) & (idx < n)).all())
    return valued, idx, ok


def backward(x, index, grad_depth, val_thr=0.1):
    """dtfill_fill_backward on numpy arrays [B,H,W] (float32, int32, float32): (grad_x float32 [B,H,W], status int32 [B])."""
    x, grad_depth = np.asarray(x, F), np.asarray(grad_depth, F)
    index = np.asarray(index, np.int32)
    B = x.shape[0]
    grad_x = np.zeros(x.shape, F)
    status = np.zeros(B, np.int32)
    for b in range(B):
        valued, idx, ok = frame_cells(x[b], index[b], val_thr)
        if not ok:
            status[b] = INDEX_ERROR
            continue
        g = grad_depth[b].reshape(-1)
        order = np.argsort(idx, kind="stable")
        cuts = np.flatnonzero(np.diff(idx[order])) + 1
        out = grad_x[b].reshape(-1)
        for cell in np.split(order, cuts):
            out[valued[idx[cell[0]]]] = cell_sum(g[cell])
    return grad_x, status


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def gather(x, index, val_thr=0.1):
    """The forward's gather of one batch (tools.py:22-26) for frames without an index error: depth_list[lbl - 1]."""
    out = np.empty(x.shape, F)
    for b in range(x.shape[0]):
        valued, idx, ok = frame_cells(x[b], index[b], val_thr)
        assert ok
        out[b] = x[b].reshape(-1)[valued[idx]].reshape(x[b].shape)
    return out


def random_gradient(rng, shape, binades=40, special=True, nonfinite=True):
    """A seeded float32 gradient whose magnitudes span `binades` binades around 1, with (special) planted zeros of both signs,
    subnormals, cancelling pairs and (nonfinite) a NaN, both infinities and a pair whose sum overflows."""
    n = int(np.prod(shape))
    mag = np.exp2(rng.uniform(-binades / 2, binades / 2, n))
    g = (mag * rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n)).astype(F)
    if special and n >= 16:
        at = rng.permutation(n)
        plant = (0.0, -0.0, 1e-40, -3e-42, 1e8, -1e8) + ((np.nan, np.inf, -np.inf, 3.0e38, 3.0e38) if nonfinite else ())
        for k, v in enumerate(plant):
            g[at[k]] = F(v)
        pairs = at[16:16 + 2 * (n // 16)].reshape(-1, 2)  # cancelling pairs, wherever their cells fall
        g[pairs[:, 1]] = -g[pairs[:, 0]]
    return g.reshape(shape)


HAND_HW = (4, 6)


def hand_cases():
    """name -> (x, index, grad_depth, grad_x, status), frames of HAND_HW at val_thr 0.1, the expected grad_x and status written
    down by hand from the contract (not computed by backward() above)."""
    H, W = HAND_HW
    N = H * W
    inf, nan = F(np.inf), F(np.nan)
    cases = {}

    def add(name, x, index, grad, want, status=0):
        cases[name] = (np.asarray(x, F).reshape(H, W), np.asarray(index, np.int32).reshape(H, W),
                       np.asarray(grad, F).reshape(H, W), np.asarray(want, F).reshape(H, W), status)

    ramp = np.arange(1, N + 1, dtype=F)  # exact sums: 1 + .. + 24 = 300
    # label 0 (no source) with a non-empty value list wraps to the LAST value: pixels 2, 9 and 20 are valued
    x = np.zeros(N, F)
    x[[2, 9, 20]] = 0.5
    want = np.zeros(N, F)
    want[20] = 300
    add("label 0 wraps to the last value", x, np.zeros(N), ramp, want)
    # all 0.5 under (0.1, 0.1): no pixel is a source (1 - 0.5 > 0.1), every pixel is valued: all of it lands on the last pixel
    want = np.zeros(N, F)
    want[N - 1] = 300
    add("all 0.5", np.full(N, 0.5), np.zeros(N), ramp, want)
    # all zero: label 0 and an empty list
    add("all zero", np.zeros(N), np.zeros(N), ramp, np.zeros(N), INDEX_ERROR)
    # valued but not sources: the value list is pixels 0 (0.5), 3 (5.0), 14 (7.0); the sources are pixels 3 and 14, labels 1
    # and 2.  Label 1 reads depth_list[0] = the 0.5 at pixel 0, label 2 the 5.0 at pixel 3: the gradient lands where the gather
    # reads, and the second source gets nothing.
    x = np.zeros(N, F)
    x[[0, 3, 14]] = (0.5, 5.0, 7.0)
    index = np.where(np.arange(N) % W < 4, 1, 2)
    want = np.zeros(N, F)
    want[0] = ramp[index == 1].sum()
    want[3] = ramp[index == 2].sum()
    add("valued pixels that are no sources", x, index, ramp, want)
    # a label n + 1: the frame is zero with its bit set
    index2 = index.copy()
    index2[17] = 4
    add("a label n + 1", x, index2, ramp, np.zeros(N), INDEX_ERROR)
    # a label -1 wraps to n - 2 = 1: pixel 3
    index3 = index.copy()
    index3[17] = -1  # (was label 2 -> pixel 3 as well: nothing moves) ...
    index3[0] = -1  # ... and this one was label 1
    want3 = want.copy()
    want3[0] -= ramp[0]
    want3[3] += ramp[0]
    add("a label -1", x, index3, ramp, want3)
    # the cells of the cell sum: eight valued pixels 0 .. 7, cell k at pixel k
    x = np.zeros(N, F)
    x[:8] = np.arange(1, 9)
    sub = F(2.0 ** -149)
    cells = [(1, 1e8), (1, 1.0), (1, -1e8),  # cancellation: 1.0, where a float32 running sum gives 0.0
             (2, 2.5), (2, nan), (2, -inf),  # any NaN: NaN
             (3, inf), (3, 3.0), (3, inf),  # +inf
             (4, inf), (4, -inf), (4, 1.0),  # both infinities: NaN
             (5, -0.0), (5, -0.0), (5, 0.0),  # only zeros: +0.0
             (6, sub), (6, sub), (6, 2 * sub), (6, -sub),  # subnormals, exactly: 3 * 2^-149
             (7, -inf), (7, 1.0),  # -inf
             (5, -0.0), (5, 0.0), (5, -0.0)]  # (cell 8, at pixel 7, stays empty: +0.0)
    assert len(cells) == N
    want = np.zeros(N, F)
    want[:7] = (1.0, nan, inf, nan, 0.0, 3 * sub, -inf)
    add("the cells of the cell sum", x, [c[0] for c in cells], [c[1] for c in cells], want)
    return cases

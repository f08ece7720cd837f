"""The cases of tests/test_gpu_conv2d_bf16_backward_edges.py (builders only: no tests, no fixtures, no torch), and what
tests/test_convb_bf16_edges.py asserts of them on the CPU.  Every expectation is convb_bf16_ref's statement in float64 over
operands rounded by conv_bf16_ref.bf16_round; each builder asserts why that float64 value is the exact one.

A1 rounding_case   a table of float32 values through ONE staging site of k_convhb_dw_wide, the other operand 1.0 at the one pixel
                   it pairs with: every entry of dw and db is a sum with at most one non-zero term.
A2 edge_case       integer operands on a small frame two rows high and Ws wide, +inf and NaN in the large operand's last column.
A4 channel_case    integer operands at the networks' channel counts, summed in float64 (exact: integers far below 2^53).
"""
import numpy as np

import conv2_ref as R2
import conv_bf16_ref as RH
import conv_ref as R
import convb_bf16_ref as RHB
import test_gpu_conv2d_bf16 as HT  # TABLE: numpy only at import

F = np.float32
LAYERS = ((3, 1, False), (1, 1, False), (3, 2, False), (1, 2, False), (3, 2, True))  # ksize, stride, transposed
IDS = ["3x3s1", "1x1s1", "3x3s2", "1x1s2", "transposed"]
STRIDED = LAYERS[:4]
KSTEP = RHB.KSTEP

# the forward's table: ties both ways (even stays, odd goes up), either sign, just above and below a tie, the largest finite
# float32 (-> inf) and the largest that stays finite, -0, +0, NaNs (one with its payload in the low half only), inf, ordinary values
TABLE = HT.TABLE
# the bf16 subnormal range, multiples of u = 2^-133 below 2^-126: 2^-127; the ties 1.5 u (up to the even 2 u), 2.5 u (down to
# 2 u) and 3.5 u (up to 4 u); -5 u; the largest float32 subnormal (rounds up to the NORMAL 2^-126); u itself; 0.75 u (up to u);
# 0.4 u (below 2^-134: rounds to 0); 8 u + 2^-149 (down to 8 u)
_U = 2.0 ** -133
SUBNORMALS = np.array([2.0 ** -127, 1.5 * _U, 2.5 * _U, 3.5 * _U, -5 * _U, 2.0 ** -126 - 2.0 ** -149, _U, 0.75 * _U, 0.4 * _U,
                       8 * _U + 2.0 ** -149], np.float64).astype(F)
VALUES = np.concatenate([TABLE, SUBNORMALS])
CHANNELS = 32  # one table value a channel: two tiles
ROUND_FRAME = (2, 40)  # the small frame of A1: a whole k-step and one of 8 pixels
ALPHA_ROUND = 0.2  # not a power of two: under y < 0, g is a rounded float32 product, then rounded to bf16


def is_subnormal(a):
    a = np.asarray(a, np.float64)
    return (a != 0) & (np.abs(a) < 2.0 ** -126)


def pt_pl(ksize, stride, frame):
    """The padding in front of a strided layer over the LARGE frame stride * frame."""
    return R2.same_rule(stride * frame[0], ksize, stride)[1], R2.same_rule(stride * frame[1], ksize, stride)[1]


def large_pixel(layer, frame, h, v, tap):
    """The pixel of the large operand that the small frame's pixel (h, v) meets under tap (i, j), or None outside its frame."""
    ksize, stride, transposed = layer
    if transposed:
        r, c = 2 * h + tap[0], 2 * v + tap[1]
        return (r, c) if r < 2 * frame[0] and c < 2 * frame[1] else None
    pt, pl = pt_pl(ksize, stride, frame)
    r, c = stride * h + tap[0] - pt, stride * v + tap[1] - pl
    return (r, c) if 0 <= r < stride * frame[0] and 0 <= c < stride * frame[1] else None


def statement(x, dy, y, layer, act, alpha):
    """(dw, db) float64: convb_bf16_ref.dw_sum over the rounded operands, NaN and inf as float64 arithmetic has them."""
    ksize, stride, transposed = layer
    xr, gr = RH.bf16_round(x), RH.bf16_round(RHB.g_ref(dy, y, act, alpha))
    with np.errstate(over="ignore", invalid="ignore"):
        return RHB.dw_sum(xr, gr, ksize, stride, transposed)


def terms(x, dy, y, layer, act, alpha):
    """(of dw, of db): the number of non-zero terms (NaN and inf count) of every entry's sum."""
    ksize, stride, transposed = layer
    xr, gr = RH.bf16_round(x), RH.bf16_round(RHB.g_ref(dy, y, act, alpha))
    return RHB.dw_sum(xr != 0, gr != 0, ksize, stride, transposed, np.int64)


SITES = ("x", "g", "g alpha", "g linear")  # where the table goes: x, or dy under y > 0, under y < 0 (g = dy * alpha), linear with y NULL


def rounding_case(layer, site, tap=None):
    """VALUES[k] at one pixel of channel k of the site's tensor, 1.0 in channel k of the other operand at the pixel that meets it
    under `tap` (default: the centre tap, (0, 0) of a 1x1 layer), +0 elsewhere; B = 1, Cin = Cout = 32.  The pixels differ from
    channel to channel: small-frame column 3 k mod 40, row k mod 2, so both k-steps, the edge step and every 4-pixel block of a
    fragment hold some.  Returns dict(x, dy, y (None: NULL), act, alpha, tap, dw, db: the float64 statement)."""
    ksize, stride, transposed = layer
    tap = ((ksize // 2, ksize // 2) if tap is None else tap)
    Hs, Ws = ROUND_FRAME
    n, C = VALUES.size, CHANNELS
    assert n <= C and Ws >= n
    xs = (1, Hs, Ws, C) if transposed else (1, stride * Hs, stride * Ws, C)
    gs = (1, 2 * Hs, 2 * Ws, C) if transposed else (1, Hs, Ws, C)
    x, dy = np.zeros(xs, F), np.zeros(gs, F)
    in_x = site == "x"
    for k in range(n):
        h, v = k % Hs, 3 * k % Ws
        big = large_pixel(layer, ROUND_FRAME, h, v, tap)
        assert big is not None
        px, pg = ((h, v), big) if transposed else (big, (h, v))
        x[0, px[0], px[1], k] = VALUES[k] if in_x else 1
        dy[0, pg[0], pg[1], k] = 1 if in_x else VALUES[k]
    act = R.LINEAR if site == "g linear" else R.LEAKY
    y = None if site == "g linear" else np.full(gs, -1.5 if site == "g alpha" else 1.5, F)
    d = dict(x=x, dy=dy, y=y, act=act, alpha=ALPHA_ROUND, tap=tap)
    d["dw"], d["db"] = statement(x, dy, y, layer, act, ALPHA_ROUND)
    tw, tb = terms(x, dy, y, layer, act, ALPHA_ROUND)
    assert tw.max() == 1 and tb.max() == 1, "an entry is a sum of more than one non-zero term"
    # the diagonal of the tap holds the rounded table, a product with 1.0; a finite float64 entry is a float32 value
    r = RH.bf16_round(VALUES if site != "g alpha" else RHB.g_ref(VALUES, -np.ones(n, F), R.LEAKY, ALPHA_ROUND)).astype(np.float64)
    diag = d["dw"][tap[0], tap[1], np.arange(n), np.arange(n)]
    assert np.array_equal(diag, r, equal_nan=True) and np.array_equal(d["db"][:n], np.ones(n) if in_x else r, equal_nan=True)
    for a in (d["dw"], d["db"]):
        fin = np.isfinite(a)
        assert np.array_equal(a[fin].astype(F).astype(np.float64), a[fin])
    return d


def rounding_runs():
    """(layer id, layer, site, tap) of A1: every site of the four strided layers; the transposed layer's x, and its g at each of
    the four parities (tap (ky, kx) with ky, kx < 2: one of db's four chains each)."""
    runs = [(i, l, s, None) for i, l in zip(IDS[:4], STRIDED) for s in SITES]
    runs.append((IDS[4], LAYERS[4], "x", None))
    runs += [(IDS[4], LAYERS[4], s, t) for s in ("g",) for t in ((0, 0), (0, 1), (1, 0), (1, 1))]
    runs += [(IDS[4], LAYERS[4], "g alpha", (1, 1)), (IDS[4], LAYERS[4], "g linear", (1, 0))]
    return runs


# ---- A2 ----------------------------------------------------------------------------------------------------------------------------
EDGE_WIDTHS = {(3, 1, False): tuple(range(1, 97))}
for _l in LAYERS:
    EDGE_WIDTHS.setdefault(_l, (1, 31, 33, 63) + tuple(range(65, 96)))
EDGE_ROWS, EDGE_C = 2, 16


def edge_left(Ws):
    """(left, whole k-steps before it, segment) of the edge k-step of a row of a small frame Ws wide; None if Ws is whole steps."""
    cols = Ws % RHB.COLS or RHB.COLS
    return None if cols % KSTEP == 0 else (cols % KSTEP, cols // KSTEP, (Ws - 1) // RHB.COLS)


def edge_case(layer, Ws, seed=0, sentinels=True):
    """integer_case at B = 1, Hs = 2, Cin = Cout = 16; in row 0 of the large operand's last column (the transposed layer: its
    last two columns, the last small pixel's taps 0 and 1) the first 8 channels are +inf and the others NaN; the small operand is
    made non-zero at its last two columns, which are all the pixels the sentinels meet: no accidental inf * 0.
    sentinels = False: the same integers without them (the 1x1 stride-1 layer, where every input channel holds a sentinel that
    every entry of dw meets, runs both).
    Returns dict(x, dy, y, dw, db (the float64 statement), sentinel: the large operand's sentinel columns)."""
    ksize, stride, transposed = layer
    x, _, dy, y = RHB.integer_case(ksize, stride, EDGE_C, EDGE_C, (1, EDGE_ROWS, Ws), 1000 * seed + Ws, transposed)
    big, small = (dy, x) if transposed else (x, dy)
    big, small = big.copy(), small.copy()
    last = big.shape[2] - 1
    cols = (last - 1, last) if transposed else (last,)
    for c in cols if sentinels else ():
        big[0, 0, c, :8], big[0, 0, c, 8:] = np.inf, np.nan
    tail = small[0, :, max(Ws - 2, 0):]
    tail[tail == 0] = 1
    x, dy = (small, big) if transposed else (big, small)
    d = dict(x=x, dy=dy, y=y, sentinel=cols)
    d["dw"], d["db"] = statement(x, dy, y, layer, R.LEAKY, RHB.ALPHA_INT)
    g = RHB.g_ref(dy, y, R.LEAKY, RHB.ALPHA_INT)
    for a in (x, g):  # integers and quarters (inf, NaN): exact in bf16, and every finite sum a small multiple of 2^-2
        assert np.array_equal(RH.bf16_round(a), a, equal_nan=True)
    fin = np.isfinite(d["dw"])
    assert np.abs(d["dw"][fin]).max(initial=0) * 4 < 2 ** 24 and np.array_equal(np.rint(d["dw"][fin] * 4), d["dw"][fin] * 4)
    assert not np.isnan(d["dw"][..., :8, :] if not transposed else d["dw"][..., :8]).any(), "an accidental inf * 0"
    return d


# ---- A4 ----------------------------------------------------------------------------------------------------------------------------
CHANNEL_FRAME = (1, 3, 40)
STRIDED_CHANNELS = ((16, 16), (16, 512), (512, 16), (64, 128), (256, 512), (512, 512), (32, 48))
TRANSPOSED_CHANNELS = ((512, 256), (128, 64), (16, 16), (16, 512))


def channel_runs():
    runs = [(i, l, c) for i, l in zip(IDS[:4], STRIDED) for c in STRIDED_CHANNELS]
    return runs + [(IDS[4], LAYERS[4], c) for c in TRANSPOSED_CHANNELS]


def channel_case(layer, cin, cout, seed=0):
    """integer_case at CHANNEL_FRAME with the sums in float64 on 4 g: integers whose partial sums stay far below 2^53, so the
    float64 sums are the int64 ones; asserted below 2^24 quarter-units, where float32 holds every partial sum in any order.
    Returns ((x, w, dy, y), (dx, dresidual, dw, db) as float32)."""
    ksize, stride, transposed = layer
    x, w, dy, y = RHB.integer_case(ksize, stride, cin, cout, CHANNEL_FRAME, seed + 31 * cin + cout + ksize + 2 * stride, transposed)
    g = RHB.g_ref(dy, y, R.LEAKY, RHB.ALPHA_INT)
    g4 = g.astype(np.float64) * 4
    for a in (x, w, g4):
        assert np.array_equal(np.rint(a), a) and np.array_equal(RH.bf16_round(a), np.asarray(a, F))
    dx = RHB.dx_sum(g4, w, stride, transposed)
    dw, db = RHB.dw_sum(x, g4, ksize, stride, transposed)
    # the largest sum of magnitudes bounds every partial sum in any order
    worst = max(RHB.dx_sum(np.abs(g4), np.abs(w), stride, transposed).max(), *(a.max() for a in RHB.dw_sum(np.abs(x), np.abs(g4), ksize, stride, transposed)))
    assert worst < 2 ** 24, worst
    for a in (dx, dw, db):
        assert np.array_equal(np.rint(a), a)
    return (x, w, dy, y), ((dx / 4).astype(F), g, (dw / 4).astype(F), (db / 4).astype(F))


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def compare(got, want, what):
    """got float32 against the float64 statement `want`: the NaN sets equal, inf as inf of its sign, every finite entry the same
    value (+0 == -0).  Entries whose statement is a subnormal float32 are left to subnormal_choice()."""
    got, want = np.asarray(got, F), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the NaN sets differ: %d against the statement's %d, first at %s" % (
        what, np.isnan(got).sum(), np.isnan(want).sum(), tuple(np.argwhere(np.isnan(got) != np.isnan(want))[0]))
    inf = np.isinf(want)
    assert np.array_equal(got[inf].astype(np.float64), want[inf]), "%s: an inf of the statement is not that inf" % what
    held = np.isfinite(want) & ~is_subnormal(want)
    bad = np.argwhere(held & (got.astype(np.float64) != want))
    if bad.size:
        k = tuple(bad[0])
        raise AssertionError("%s: %d of %d finite entries differ, first at %s: got %r (%#x), want %r" % (
            what, len(bad), held.sum(), k, got[k], got[k].view(np.uint32), want[k]))


def subnormal_choice(pairs):
    """pairs: (got, want) of one call.  Over every entry whose statement is subnormal: "kept" if all equal it, "flushed" if all
    are zeros, None if there is none; anything else, a mixture included, fails."""
    got = np.concatenate([np.asarray(g, F)[is_subnormal(w)].astype(np.float64) for g, w in pairs])
    want = np.concatenate([np.asarray(w, np.float64)[is_subnormal(w)] for g, w in pairs])
    if not want.size:
        return None
    kept, flushed = got == want, got == 0
    assert kept.all() or flushed.all(), "subnormal rows: %d kept, %d flushed, %d neither, of %d" % (
        kept.sum(), flushed.sum(), (~kept & ~flushed).sum(), want.size)
    return "kept" if kept.all() else "flushed"

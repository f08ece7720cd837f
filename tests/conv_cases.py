"""The cases of tests/test_gpu_conv2d_limits.py (builders only: no tests, no fixtures, no torch at import), and what
tests/test_conv_cases.py asserts of them on the CPU.

A. LOOP: one call per kernel body of csrc/dtfill_conv.hpp and dtfill_convb.hpp whose work items lie a hundred above
   CV_MAX_BLOCKS = 2^20, on tiny frames: most blocks take one item, a hundred take a second one.  items() restates the
   launchers' item counts from the tile constants.
B. LARGE: every tensor argument of the five entry points past byte offset 4 GiB (two tensors past 2 GiB, one batch within a
   frame of the shape rule's limit, 8 GiB of x), and the calls that stand exactly at 2^31 elements and are refused.
   A and B are tiled batches in the sense of tests/large_cases.py: T frames of test_gpu_conv2d.case() values repeated, a
   reference on the tile only, every period T * (elements of a frame) with an odd factor, and no zero in any expected output
   (the contracts leave the sign of a zero open; the device comparison is by bits).
C. CLASSES: float32's range on the matrix cores.  Values are a seeded normal times 2^(an integer exponent from a range), as
   case() builds them; the ranges are chosen so that the reference itself shows subnormal operands that matter, sums that cross
   2^-126 both ways, subnormal sums, sums that cross FLT_MAX inside the chain, and an epilogue that underflows and overflows.
"""
import numpy as np

import conv2_ref as R2
import conv_ref as R
import convb_ref as RB
import test_gpu_conv2d as fwd  # case(): numpy only at import
import test_gpu_conv2d_backward as bwd  # case()

F = np.float32
TILE_H, TILE_W, TILE_H2 = 8, 32, 4  # CV_TH, CV_TW and the rows of a stride-2 tile of csrc/dtfill_conv.hpp
PASS_CHANNELS = 64  # 16 CV_NB: the output channels of one pass of k_conv_wide
GROUP = R.GROUP  # CV_G
MAX_BLOCKS = 1 << 20  # CV_MAX_BLOCKS
SEG_ROWS, SEG_COLS = RB.CONV_BW_ROWS, RB.CONV_BW_COLS
POISON = fwd.POISON
ALPHA = 0.2
T = 3  # frames of every tile
ERR_SHAPE = -2  # DTFILL_ERR_SHAPE


def _cdiv(a, b):
    return -(-a // b)


def out_frame(c):
    """(Ho, Wo) of a forward case."""
    if c["entry"] == "transpose":
        return 2 * c["H"], 2 * c["W"]
    s = c.get("stride", 1)
    return _cdiv(c["H"], s), _cdiv(c["W"], s)


def items(c):
    """The work items of case c's MFMA launch, as conv_launch_items and convb_dw_launch count them."""
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    if c["entry"] == "dw":
        return B * _cdiv(H, SEG_ROWS) * _cdiv(W, SEG_COLS) * (1 if cin == 1 else cin // GROUP)
    if c["entry"] == "dx":  # the forward kernels on g, Cout -> Cin channels: k_conv_mfma for Cin <= 16, k_conv_wide's passes beyond
        assert cout == GROUP and cin % GROUP == 0
        return B * _cdiv(H, TILE_H) * _cdiv(W, TILE_W) * _cdiv(cin, PASS_CHANNELS)
    if c["entry"] == "transpose":
        return B * _cdiv(H, TILE_H) * _cdiv(W, TILE_W) * 4 * _cdiv(cout, PASS_CHANNELS)
    Ho, Wo = out_frame(c)
    th = TILE_H2 if c.get("stride", 1) == 2 else TILE_H
    return B * _cdiv(Ho, th) * _cdiv(Wo, TILE_W) * _cdiv(cout, PASS_CHANNELS)


def items_per_frame(c):
    return items(c) // c["B"]


def tiles(c):
    """(tile or segment rows, columns) of a frame of case c."""
    if c["entry"] == "dw":
        return _cdiv(c["H"], SEG_ROWS), _cdiv(c["W"], SEG_COLS)
    if c["entry"] in ("dx", "transpose"):
        return _cdiv(c["H"], TILE_H), _cdiv(c["W"], TILE_W)
    Ho, Wo = out_frame(c)
    return _cdiv(Ho, TILE_H2 if c.get("stride", 1) == 2 else TILE_H), _cdiv(Wo, TILE_W)


# ---- A.  body: the kernel the case is for.  misaligned: the case runs a second time with x four bytes off a 16-byte boundary.
# items = 2^20 + about 100.  Where a frame has 3 or 12 items, no power of two, item k + 2^20 differs from item k in its tile
# row or column, parity or group as well as in its frame; where it has 2, only in the frame.
_B2, _B3, _B12 = 524338, 349559, 87390  # 2 (2^19 + 50), 3 * 349559 = 2^20 + 101, 12 * 87390 = 2^20 + 104
LOOP = {
    "conv2d 3x3x16->16": dict(entry="conv2d", body="k_conv_mfma<3,false>", ksize=3, cin=16, cout=16, B=_B3, H=17, W=1, misaligned=True),
    "conv2d 7x7x1->16": dict(entry="conv2d", body="k_conv_mfma<7,true>", ksize=7, cin=1, cout=16, B=_B2, H=1, W=33),
    "strided 3x3x16->128 residual": dict(entry="strided", body="k_conv_wide<ConvPlain<3,1>>", ksize=3, cin=16, cout=128, stride=1,
                                         residual=True, B=_B2, H=1, W=3),
    "strided 3x3x16->16 stride 2": dict(entry="strided", body="k_conv_wide<ConvPlain<3,2>>", ksize=3, cin=16, cout=16, stride=2, B=_B3,
                                        H=17, W=1, misaligned=True),
    "transpose 16->16": dict(entry="transpose", body="k_conv_wide<ConvTransposed>", ksize=3, cin=16, cout=16, B=_B12, H=1, W=65),
    "dw 1x1x32->16": dict(entry="dw", body="k_convb_dw<1,false>", ksize=1, cin=32, cout=16, act=R.LEAKY, B=_B2, H=1, W=5),
    "dw 1x1x48->16": dict(entry="dw", body="k_convb_dw<1,false>", ksize=1, cin=48, cout=16, act=R.LEAKY, B=_B3, H=1, W=5),
    "dw 3x3x1->16": dict(entry="dw", body="k_convb_dw<3,true>", ksize=3, cin=1, cout=16, act=R.LINEAR, B=_B2, H=1, W=65),
    "dx 3x3x16->16": dict(entry="dx", body="k_convb_g, k_conv_mfma<3,false>", ksize=3, cin=16, cout=16, act=R.LEAKY, B=_B3, H=17, W=1),
}

# ---- B.  past: the threshold in elements (2^29: 2 GiB of float32, 2^30: 4 GiB) that `by` (elements of a frame of the tensor
# the case is about) passes with the batch's last T frames, or "limit": the largest batch the shape rule admits.
FRAME = (9, 33)  # 297 = 3^3 * 11 pixels: two tile rows, two tile columns, odd
SEGMENT = (SEG_ROWS, SEG_COLS)  # one segment a frame: 2^11 pixels (T = 3 is the period's odd factor)
_PX, _SPX = FRAME[0] * FRAME[1], SEGMENT[0] * SEGMENT[1]


def batch_past(threshold, frame_elems, t=T):
    """The smallest batch whose last t frames start at or beyond element `threshold`."""
    return _cdiv(threshold, frame_elems) + t


def _large(past, by, **kw):
    B = (2 ** 31 - 1) // by if past == "limit" else batch_past(past, by)
    return dict(kw, B=B, past=past, by=by)


LARGE = {
    "conv2d 3x3x64->16, x past 2 GiB": _large(2 ** 29, _PX * 64, entry="conv2d", ksize=3, cin=64, cout=16, H=FRAME[0], W=FRAME[1]),
    "conv2d 3x3x64->16, x past 4 GiB": _large(2 ** 30, _PX * 64, entry="conv2d", ksize=3, cin=64, cout=16, H=FRAME[0], W=FRAME[1]),
    "conv2d 3x3x64->16, x at the limit": _large("limit", _PX * 64, entry="conv2d", ksize=3, cin=64, cout=16, H=FRAME[0], W=FRAME[1]),
    "strided 3x3x64->16 stride 2, x past 4 GiB": _large(2 ** 30, _PX * 64, entry="strided", ksize=3, cin=64, cout=16, stride=2,
                                                        H=FRAME[0], W=FRAME[1]),
    "strided 1x1x16->64 at 16 of 80, out and residual past 4 GiB": _large(2 ** 30, _PX * 64, entry="strided", ksize=1, cin=16, cout=64,
                                                                          stride=1, residual=True, out_channels=80, out_offset=16,
                                                                          H=FRAME[0], W=FRAME[1]),
    "transpose 16->16, out past 4 GiB": _large(2 ** 30, 4 * _PX * 16, entry="transpose", ksize=3, cin=16, cout=16, H=FRAME[0], W=FRAME[1]),
    "dx 3x3x64->16, dy, y and dx past 4 GiB": _large(2 ** 30, _PX * 64, entry="dx", ksize=3, cin=64, cout=16, act=R.LEAKY, width=64, at=32,
                                                     H=FRAME[0], W=FRAME[1]),
    "dw 1x1x64->16, x, dy and y past 4 GiB": _large(2 ** 30, _SPX * 64, entry="dw", ksize=1, cin=64, cout=16, act=R.LEAKY, width=64, at=32,
                                          H=SEGMENT[0], W=SEGMENT[1]),
    "conv2d 3x3x16->16 at 16 of 128, out at the limit": _large("limit", _PX * 128, entry="conv2d", ksize=3, cin=16, cout=16, out_channels=128,
                                                               out_offset=16, H=FRAME[0], W=FRAME[1]),
    "dx 3x3x16->16, dy and y 128 wide at the limit": _large("limit", _PX * 128, entry="dx", ksize=3, cin=16, cout=16, act=R.LEAKY, width=128,
                                                            at=48, H=FRAME[0], W=FRAME[1]),
    "dw 3x3x16->1, x past 2 GiB, dy past 4 GiB": _large(2 ** 29, _SPX * 16, entry="dw", ksize=3, cin=16, cout=1, act=R.LINEAR, width=32, at=8,
                                                        H=SEGMENT[0], W=SEGMENT[1]),
}

# calls that stand exactly at 2^31 elements: (entry, what is at 2^31, arguments).  They are refused before any launch.
REFUSED = (
    ("conv2d", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3)),
    ("strided", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3, stride=1)),
    ("transpose", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3)),
    ("conv2d", "B Ho Wo out_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, out_channels=128)),
    ("strided", "B Ho Wo Cout", dict(B=2 ** 14, H=32, W=32, cin=16, cout=128, ksize=1, stride=1)),
    ("strided", "B Ho Wo out_channels", dict(B=2 ** 14, H=64, W=64, cin=16, cout=16, ksize=3, stride=2, out_channels=128)),
    ("transpose", "B Ho Wo out_channels", dict(B=2 ** 14, H=16, W=32, cin=16, cout=16, ksize=3, out_channels=64)),
    ("dx", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3)),
    ("dw", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3)),
    ("dx", "B H W dy_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, dy_channels=128)),
    ("dw", "B H W y_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, y_channels=128)),
    ("dx", "B H W dx_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, dx_channels=128)),  # needs a real workspace
)


def refused_count(entry, a):
    """The element count of the call that the rule it is refused by looks at."""
    n = a["B"] * a["H"] * a["W"]
    if entry in ("dx", "dw"):
        return n * max(a["cin"], a.get("dy_channels", 0), a.get("y_channels", 0), a.get("dx_channels", 0))
    ho, wo = out_frame(dict(a, entry=entry))
    return max(n * a["cin"], a["B"] * ho * wo * max(a["cout"], a.get("out_channels", 0)))


def tile(c, seed=0):
    """The T frames of a tiled case and the reference on them.  Returns a dict of float32 arrays: the inputs (x, w, bias,
    residual / x, w, dy, y: dy and y as their whole tensors, `width` wide with poison beside the slice) and `want`, the
    expected output of one period ([T, ...]; dw: the level-1 partials of the tile's segments in (b, t, s) order)."""
    ksize, cin, cout, H, W = c["ksize"], c["cin"], c["cout"], c["H"], c["W"]
    shape = (T, H, W)
    if c["entry"] in ("dx", "dw"):
        x, w, dy, y = bwd.case(ksize, cin, cout, shape, seed)
        act = c["act"]
        width, at = c.get("width", cout), c.get("at", 0)
        d = dict(x=x, w=w, dy=widened(dy, width, at), y=widened(y, width, at), act=act, width=width, at=at)
        if c["entry"] == "dx":
            d["want"] = RB.dx_ref(dy, y, w, act, ALPHA)
        else:
            d["want"] = RB.partials(x, RB.g_ref(dy, y, act, ALPHA), ksize)
        return d
    x, w, b = fwd.case(ksize, cin, cout, shape, seed)
    d = dict(x=x, w=w, bias=b, residual=None)
    if c["entry"] == "transpose":
        want = R2.transpose_ref(x, w, b, R.LEAKY, ALPHA)
    elif c["entry"] == "strided":
        if c.get("residual"):
            d["residual"] = np.random.default_rng(1000 + seed).standard_normal((T,) + out_frame(c) + (cout,)).astype(F)
        want = R2.strided_ref(x, w, b, c["stride"], d["residual"], R.LEAKY, ALPHA)
    else:
        want = R.conv_ref(x, w, b, R.LEAKY, ALPHA)
    d["want"] = widened(want, c.get("out_channels", cout), c.get("out_offset", 0))
    return d


def widened(a, width, at):
    """a [..., C] as the channels at .. at + C - 1 of a [..., width] tensor whose other channels hold POISON."""
    if width == a.shape[-1]:
        return np.ascontiguousarray(a, F)
    out = np.full(a.shape[:-1] + (width,), POISON, np.uint32).view(F)
    out[..., at:at + a.shape[-1]] = a
    return out


def level2(part, nseg):
    """Level 2 of dw and db over a tiled batch: segment n's partials are part[n % len(part)]; one rounded float32 add a
    segment, in order, from +0 (a plain loop of row adds: about 1 s per million rows of 160 floats)."""
    total = np.zeros(part.shape[1:], F)
    rows = [np.ascontiguousarray(p) for p in part]
    n_rows = len(rows)
    with np.errstate(over="ignore", invalid="ignore"):
        for n in range(nseg):
            np.add(total, rows[n % n_rows], out=total)
    return total


def split_dw(total, ksize, cin):
    """level2()'s [ksize^2 Cin + 1, Cout] -> (dw [ksize,ksize,Cin,Cout], db [Cout])."""
    return total[:-1].reshape(ksize, ksize, cin, -1).copy(), total[-1].copy()


def _align(n):
    return (n + 255) & ~255


def workspace_bytes(c):
    """dtfill_conv2d_backward_workspace_bytes restated: the larger of g + wT (dx) and the segments' partials (dw); either call
    asks for it."""
    B, H, W, cin, cout, taps = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["ksize"] ** 2
    data = _align(4 * B * H * W * cout) + _align(4 * taps * cin * cout)
    return max(data, _align(4 * B * _cdiv(H, SEG_ROWS) * _cdiv(W, SEG_COLS) * (taps * cin + 1) * cout))


COMPARE_CHUNK = 32 << 20  # bytes of a tensor per step of the device comparison of A and B's smaller tensors
COMPARE_BYTES = 4 * COMPARE_CHUNK  # what a step allocates beside the tensors, generously


def device_bytes(c, chunk=COMPARE_CHUNK):
    """The device memory case c holds at once: its tensors, the workspace, and the comparison's scratch."""
    n = 4 * c["B"] * c["H"] * c["W"]
    if c["entry"] in ("dx", "dw"):
        width = c.get("width", c["cout"])
        total = n * width * (2 if c["act"] == R.LEAKY else 1) + n * c["cin"] + workspace_bytes(c)
    else:
        Ho, Wo = out_frame(c)
        no = 4 * c["B"] * Ho * Wo
        total = n * c["cin"] + no * c.get("out_channels", c["cout"]) + (no * c["cout"] if c.get("residual") else 0)
    return total + 4 * chunk


def periods(c, d):
    """(name, T * elements of a frame) of every tiled tensor of case c with tile d: what assert_alias_free looks at."""
    names = ("x", "dy", "y") if c["entry"] in ("dx", "dw") else ("x", "residual")
    out = [(k, d[k].size) for k in names if d.get(k) is not None]
    if c["entry"] != "dw":
        out.append(("out", d["want"].size))
    return out


# ---- C.  (exponent range of x, of w, of the bias); both ends included.  backward: dx takes dy from x's range and w from w's,
# dw takes x from x's range and dy from w's ("huge": from DW_HUGE, a chain of 153 or 297 pixels and two frames at level 2)
CLASSES = {
    "subnormal x": ((-149, -127), (20, 40), (-100, -96)),
    "subnormal w": ((20, 40), (-149, -127), (-100, -96)),
    "straddling": ((-68, -63), (-68, -63), (-127, -125)),
    "tiny": ((-71, -69), (-71, -69), (-141, -139)),
    "huge": ((58, 63), (58, 63), (120, 124)),
    "leaky": None,  # leaky_case()
}
BACKWARD_CLASSES = ("subnormal x", "subnormal w", "straddling", "tiny", "huge")
DW_HUGE = {153: (60, 65), 297: (58, 63)}  # by the pixels of a segment, a frame of SMALL_SHAPES: the links of dw's level-1 chain
SMALL_SHAPES = ((1, 9, 17), (2, 9, 33))
# (entry, ksize, Cin, Cout, stride)
FORWARD_LAYERS = (("conv2d", 3, 32, 16, 1), ("conv2d", 7, 1, 16, 1), ("strided", 3, 32, 48, 1), ("strided", 3, 32, 48, 2),
                  ("transpose", 3, 32, 48, 1), ("conv2d", 3, 16, 1, 1))
BACKWARD_LAYERS = ((3, 32, 16), (3, 1, 16))


def scaled(rng, shape, lo, hi):
    """A normal times 2^e, e an integer drawn from lo .. hi, rounded to float32 once."""
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(lo, hi + 1, shape)).astype(F)


def leaky_case(ksize, cin, cout, shape, seed):
    """Even output channels: subnormal sums under a bias of -3 .. -3.5 times 2^-126, so that y is normal and y * alpha is
    subnormal; odd ones: finite sums of 2^103 and more under a bias of +-FLT_MAX, so that the bias add overflows wherever the
    sum has the bias's sign and stays finite, next to FLT_MAX, wherever it has the other.  Cout == 1 has one channel: it is of the
    even kind under an even seed and of the odd kind under an odd one."""
    rng = np.random.default_rng(seed)
    x = scaled(rng, shape + (cin,), -3, 3)
    small = (np.arange(cout) + (seed if cout == 1 else 0)) % 2 == 0
    w = np.empty((ksize, ksize, cin, cout), F)
    w[..., small] = scaled(rng, w[..., small].shape, -136, -132)
    w[..., ~small] = scaled(rng, w[..., ~small].shape, 105, 115)
    b = np.empty(cout, F)
    b[small] = (-(3.0 + 0.5 * rng.random(int(small.sum()))) * 2.0 ** -126).astype(F)
    b[~small] = (rng.choice([-1.0, 1.0], int((~small).sum())) * float(np.finfo(F).max)).astype(F)
    return x, w, b


def huge_shift(links):
    """The exponents added to w's range in "huge" for a chain of `links` links, so that chains shorter than 3x3x32's 288 cross
    FLT_MAX about as often (a sum of n terms of mixed binades grows roughly as sqrt(n))."""
    return 0 if links >= 288 else 1 if links >= 64 else 2


def class_case(name, ksize, cin, cout, shape, seed, entry="conv2d"):
    """x [shape, Cin], w [ksize,ksize,Cin,Cout], bias [Cout] of value class `name`."""
    if name == "leaky":
        return leaky_case(ksize, cin, cout, shape, seed)
    (x0, x1), (w0, w1), (b0, b1) = CLASSES[name]
    if name == "huge":  # (the transpose: 1, 2, 2 and 4 taps of 9 by parity)
        up = huge_shift(ksize * ksize * cin * (0.25 if entry == "transpose" else 1))
        w0, w1 = w0 + up, w1 + up
    rng = np.random.default_rng(seed)
    return scaled(rng, shape + (cin,), x0, x1), scaled(rng, (ksize, ksize, cin, cout), w0, w1), scaled(rng, (cout,), b0, b1)


def backward_class_case(name, ksize, cin, cout, shape, seed):
    """(x, w, y, dy for dx, dy for dw): y of ordinary values decides the branch."""
    (x0, x1), (w0, w1), _ = CLASSES[name]
    if name == "huge":  # g is dy * alpha in half of the links
        w0, w1 = w0 + 1, w1 + 1
    rng = np.random.default_rng(seed)
    x, w = scaled(rng, shape + (cin,), x0, x1), scaled(rng, (ksize, ksize, cin, cout), w0, w1)
    y = scaled(rng, shape + (cout,), -3, 3)
    dy_dx = scaled(rng, shape + (cout,), x0, x1)
    dy_dw = scaled(rng, shape + (cout,), *(DW_HUGE[shape[1] * shape[2]] if name == "huge" else (w0, w1)))
    return x, w, y, dy_dx, dy_dw


def forward_ref(entry, x, w, b, stride=1, act=R.LEAKY):
    """The reference of a part C forward case (alpha 0.2)."""
    if entry == "transpose":
        return R2.transpose_ref(x, w, b, act, ALPHA)
    if entry == "strided":
        return R2.strided_ref(x, w, b, stride, None, act, ALPHA)
    return R.conv_ref(x, w, b, act, ALPHA)


def flushed(a):
    """a with its subnormal values replaced by zeros of their sign: what a flushing operand read makes of it."""
    a = np.asarray(a, F)
    return np.where(np.abs(a) < np.finfo(F).tiny, np.copysign(F(0), a), a).astype(F)


def is_subnormal(a):
    a = np.asarray(a, F)
    return (a != 0) & (np.abs(a) < np.finfo(F).tiny)


def is_normal(a):
    a = np.asarray(a, F)
    return np.isfinite(a) & (np.abs(a) >= np.finfo(F).tiny)

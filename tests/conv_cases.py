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
import conv2b_ref as RW
import conv_bf16_ref as HB
import conv_ref as R
import convb_bf16_ref as HBB
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
    if c.get("bf16"):
        return bf16_tile(c, seed)
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


# ================================================================================================ the newer backward kernels
# Part A for k_convb_dw_wide, k_convb_dw_image and the data gradients of the wide layers (tests/test_gpu_conv2d_backward_limits.py).
# k_convb_dw_wide takes its segment from the grid's z axis, and convb_dw_wide_launch repeats the launch from seg0 = 65535 on:
# frames whose SEGMENT frame is 1 x 129 have three segments (the last of one column), and B = 21879 of them 65637 = 65535 + 102,
# so that segment 65535 is column 0 of frame 21845: the second launch begins on a frame boundary and ends inside a frame.
# k_convb_dw_image has an item loop past CV_MAX_BLOCKS as k_convb_dw has: one segment a frame, 2^20 + 101 frames, or two
# passes a segment and 2^19 + 50 frames.  H, W: the layer's input frame.  dy and y are the channels at .. of tensors `width` wide.
GRID_Z = 65535  # the segments of one launch of k_convb_dw_wide
_BW = 21879  # 3 * 21879 = 65637


def _w(entry, ksize, stride, cin, cout, act, H, W, B=_BW, transposed=False, width=None, at=0, dres=False, mis=0):
    return dict(entry=entry, ksize=ksize, stride=stride, cin=cin, cout=cout, act=act, H=H, W=W, B=B, transposed=transposed,
                width=cout if width is None else width, at=at, dres=dres, mis=mis)


WLOOP = {
    "dw wide 1x1x16->32": _w("dw_wide", 1, 1, 16, 32, R.LEAKY, 1, 129, width=48, at=16),
    "dw wide 3x3x16->32": _w("dw_wide", 3, 1, 16, 32, R.LEAKY, 1, 129, width=48, at=16),
    "dw wide 3x3x16->32, x, dy and y 4 bytes off": _w("dw_wide", 3, 1, 16, 32, R.LEAKY, 1, 129, width=48, at=16, mis=4),
    "dw wide 5x5x16->32": _w("dw_wide", 5, 1, 16, 32, R.LINEAR, 1, 129, width=48, at=16),
    "dw wide 7x7x16->32": _w("dw_wide", 7, 1, 16, 32, R.LINEAR, 1, 129, width=48, at=16),
    "dw wide 1x1x16->32 stride 2": _w("dw_wide", 1, 2, 16, 32, R.LEAKY, 2, 258, width=48, at=16),
    "dw wide 3x3x16->32 stride 2": _w("dw_wide", 3, 2, 16, 32, R.LINEAR, 2, 258, width=48, at=16),
    "dw wide transposed 16->32": _w("dw_wide", 3, 2, 16, 32, R.LINEAR, 1, 129, transposed=True),
    "dx wide 1x1x16->32 stride 2": _w("dx_wide", 1, 2, 16, 32, R.LEAKY, 2, 258, width=48, at=16),
    "dx wide transposed 16->32": _w("dx_wide", 3, 2, 16, 32, R.LINEAR, 1, 129, transposed=True),
    "dw image 3x3x3->16": _w("dw_image", 3, 1, 3, 16, R.LEAKY, 1, 5, B=MAX_BLOCKS + 101),
    "dw image 7x7x4->16": _w("dw_image", 7, 1, 4, 16, R.LINEAR, 1, 1, B=MAX_BLOCKS + 101),
    "dw image 3x3x3->128": _w("dw_image", 3, 1, 3, 128, R.LINEAR, 1, 1, B=MAX_BLOCKS // 2 + 50),
}


# Part B for the same entry points and for dtfill_conv2d_image: every tensor argument past byte offset 4 GiB in some case, a
# case past 2 GiB and one at the largest batch the shape rule admits per group, on FRAME (the stride-2 layers: its double, the
# image weight gradient: SEGMENT).  x of the image layers has at most 4 channels and cannot pass 4 GiB within the rule
# (B H W max(Cin, Cout) < 2^31 with Cout >= 16).  The workspace of the data gradient holds g for the whole batch: where dy of a
# 64-channel layer passes 4 GiB, so does the workspace.  All dy and y of the dw wide cases of A and B but the "4 bytes off"
# one are 16-byte aligned with widths that are multiples of 4: the VEC = true bodies; that one case runs VEC = false.
_P4, _P2 = 2 ** 30, 2 ** 29
WLARGE = {
    "dx strided 1x1x64->64, dy, dx, dresidual and the workspace past 4 GiB": _w("dx_wide", 1, 1, 64, 64, R.LINEAR, *FRAME, B=batch_past(_P4, _PX * 64),
                                                                             dres=True),
    "dx strided 1x1x64->64 stride 2, dx past 4 GiB": _w("dx_wide", 1, 2, 64, 64, R.LEAKY, 18, 66, B=batch_past(_P4, 4 * _PX * 64)),
    "dx strided 3x3x16->16, dy 128 wide at the limit": _w("dx_wide", 3, 1, 16, 16, R.LINEAR, *FRAME, B=(2 ** 31 - 1) // (_PX * 128), width=128, at=48),
    "dx transposed 64->16, dy, y, dx and the workspace past 4 GiB": _w("dx_wide", 3, 2, 64, 16, R.LEAKY, *FRAME, B=batch_past(_P4, 4 * _PX * 16),
                                                                    transposed=True),
    "dw strided 1x1x64->16, x, dy and y past 4 GiB": _w("dw_wide", 1, 1, 64, 16, R.LEAKY, *FRAME, B=batch_past(_P4, _PX * 64), width=64, at=32),
    "dw strided 3x3x16->16 stride 2, x past 2 GiB": _w("dw_wide", 3, 2, 16, 16, R.LEAKY, 18, 66, B=batch_past(_P2, 4 * _PX * 16)),
    "dw strided 1x1x64->16, x at the limit": _w("dw_wide", 1, 1, 64, 16, R.LINEAR, *FRAME, B=(2 ** 31 - 1) // (_PX * 64)),
    "dw transposed 64->16, x, dy and y past 4 GiB": _w("dw_wide", 3, 2, 64, 16, R.LEAKY, *FRAME, B=batch_past(_P4, _PX * 64), transposed=True),
    "dw image 3x3x4->16, dy and y past 4 GiB": _w("dw_image", 3, 1, 4, 16, R.LEAKY, *SEGMENT, B=batch_past(_P4, _SPX * 64), width=64, at=32),
    "dw image 3x3x3->16, dy past 2 GiB": _w("dw_image", 3, 1, 3, 16, R.LINEAR, *SEGMENT, B=batch_past(_P2, _SPX * 32), width=32, at=16),
    "dw image 3x3x4->16, dy 128 wide at the limit": _w("dw_image", 3, 1, 4, 16, R.LINEAR, *SEGMENT, B=(2 ** 31 - 1) // (_SPX * 128), width=128, at=48),
}
# dtfill_conv2d_image itself: records of LARGE's kind (entry "conv2d": conv_ref is its statement too), read by tile(),
# device_bytes() and periods()
ILARGE = {
    "image 3x3x3->64, out past 2 GiB": _large(_P2, _PX * 64, entry="conv2d", ksize=3, cin=3, cout=64, H=FRAME[0], W=FRAME[1]),
    "image 3x3x4->64, out past 4 GiB": _large(_P4, _PX * 64, entry="conv2d", ksize=3, cin=4, cout=64, H=FRAME[0], W=FRAME[1]),
    "image 3x3x4->16 at 16 of 128, out at the limit": _large("limit", _PX * 128, entry="conv2d", ksize=3, cin=4, cout=16, out_channels=128,
                                                             out_offset=16, H=FRAME[0], W=FRAME[1]),
}
# (entry, what is at 2^31, arguments); H, W: the layer's input frame.  "ws0": the size function answers 0 there too.
WREFUSED = (
    ("image", "B H W Cout", dict(B=2 ** 15, H=32, W=32, cin=4, cout=64, ksize=3)),
    ("image", "B H W out_channels", dict(B=2 ** 14, H=32, W=32, cin=4, cout=16, ksize=3, out_channels=128)),
    ("dw_image", "B H W Cout", dict(B=2 ** 15, H=32, W=32, cin=4, cout=64, ksize=3, ws0=True)),
    ("dw_image", "B H W dy_channels", dict(B=2 ** 14, H=32, W=32, cin=4, cout=16, ksize=3, dy_channels=128)),
    ("dw_image", "B H W y_channels", dict(B=2 ** 14, H=32, W=32, cin=4, cout=16, ksize=3, y_channels=128)),
    ("dx_wide", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3, stride=1, ws0=True)),
    ("dw_wide", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3, stride=1, ws0=True)),
    ("dx_wide", "B Ho Wo Cout", dict(B=2 ** 15, H=32, W=32, cin=16, cout=64, ksize=3, stride=1, ws0=True)),
    ("dw_wide", "B 2H 2W Cout", dict(B=2 ** 15, H=16, W=16, cin=16, cout=64, ksize=3, stride=2, transposed=True, ws0=True)),
    ("dx_wide", "B Ho Wo dy_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, stride=1, dy_channels=128)),
    ("dw_wide", "B Ho Wo y_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=1, stride=1, y_channels=128)),
    ("dx_wide", "B 2H 2W dy_channels", dict(B=2 ** 14, H=16, W=16, cin=16, cout=16, ksize=3, stride=2, transposed=True, dy_channels=128)),
    ("dw_wide", "B 2H 2W y_channels", dict(B=2 ** 14, H=16, W=16, cin=16, cout=16, ksize=3, stride=2, transposed=True, y_channels=128)),
    ("dx_wide", "B H W dx_channels", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, stride=1, dx_channels=128)),  # needs a real workspace
    ("dx_wide", "B H W dx_channels (transposed)", dict(B=2 ** 14, H=32, W=32, cin=16, cout=16, ksize=3, stride=2, transposed=True,
                                                      dx_channels=128)),
)


def wrefused_count(entry, a):
    """The element count the rule that refuses the call looks at."""
    n = a["B"] * a["H"] * a["W"]
    if entry == "image":
        return n * max(a["cin"], a["cout"], a.get("out_channels", 0))
    (Ho, Wo), _ = wframes(dict(a, transposed=a.get("transposed", False), stride=a.get("stride", 1)))
    no = a["B"] * Ho * Wo
    return max(n * max(a["cin"], a.get("dx_channels", 0)), no * max(a["cout"], a.get("dy_channels", 0), a.get("y_channels", 0)))


def wframes(c):
    """((Ho, Wo) of dy, the frame the segments lie over) of a case of WLOOP."""
    H, W = c["H"], c["W"]
    if c["transposed"]:
        return (2 * H, 2 * W), (H, W)
    return (H // c["stride"], W // c["stride"]), (H // c["stride"], W // c["stride"])


def wsegments(c):
    Hs, Ws = wframes(c)[1]
    return c["B"] * _cdiv(Hs, SEG_ROWS) * _cdiv(Ws, SEG_COLS)


def witems(c):
    """The work items of k_convb_dw_image's launch: segments times passes of four N-tiles."""
    assert c["entry"] == "dw_image"
    return wsegments(c) * _cdiv(c["cout"] // 16, 4)


def wworkspace_bytes(c):
    """dtfill_conv2d_wide_backward_workspace_bytes and dtfill_conv2d_image_backward_workspace_bytes restated: the larger of g,
    the repacked kernel and the 1x1 stride-2 chain's values (dx; none for the image layer) and the segments' partials (dw)."""
    (Ho, Wo), _ = wframes(c)
    taps, cin, cout, pixels = c["ksize"] ** 2, c["cin"], c["cout"], c["B"] * Ho * Wo
    spread = not c["transposed"] and c["stride"] == 2 and c["ksize"] == 1
    # the kernel the data gradient runs under: float32, or (bf16) the packed array of the forward over g, Cout in and Cin out
    kernel = 2 * HB.packed_elems(c["ksize"], cout, cin) if c.get("bf16") else 4 * taps * cin * cout
    data = 0 if c["entry"] == "dw_image" else _align(4 * pixels * cout) + _align(kernel) + (_align(4 * pixels * cin) if spread else 0)
    return max(data, _align(4 * wsegments(c) * (taps * cin + 1) * cout))


def wdevice_bytes(c, chunk=COMPARE_CHUNK):
    (Ho, Wo), _ = wframes(c)
    n = 4 * c["B"] * c["H"] * c["W"] * c["cin"]  # x, or dx
    dres = 4 * c["B"] * Ho * Wo * c["cout"] if c["dres"] else 0
    return n + 4 * c["B"] * Ho * Wo * c["width"] * (2 if c["act"] == R.LEAKY else 1) + dres + wworkspace_bytes(c) + 4 * chunk


def wtile(c, seed=0):
    """The T frames of a case of WLOOP and the reference on them: x, w, dy and y (whole tensors, poison beside the slice) and
    `want`: dx of the tile, or the level-1 partials [T * segments of a frame, ksize^2 Cin + 1, Cout] in (b, t, s) order."""
    if c.get("bf16"):
        return bf16_wtile(c, seed)
    ksize, stride, cin, cout, act = c["ksize"], c["stride"], c["cin"], c["cout"], c["act"]
    (Ho, Wo), _ = wframes(c)
    x, w, _ = fwd.case(ksize, cin, cout, (T, c["H"], c["W"]), seed)
    dy, _, _ = fwd.case(1, cout, cout, (T, Ho, Wo), seed + 1000)
    y, _, _ = fwd.case(1, cout, cout, (T, Ho, Wo), seed + 2000)
    y[np.random.default_rng(seed).random(y.shape) < 0.05] = -0.0
    g = RB.g_ref(dy, y, act, ALPHA)
    if c["entry"] == "dx_wide":
        want = RW.transpose_dx_ref(dy, y, w, act, ALPHA) if c["transposed"] else RW.strided_dx_ref(dy, y, w, stride, act, ALPHA)
    elif c["entry"] == "dw_image":
        want = RB.partials(x, g, ksize)
    elif c["transposed"]:
        part, pb = RW.transpose_partials(x, g)
        want = np.concatenate([part.reshape(len(part), 9 * cin, cout), pb[:, None, :]], axis=1)
    else:
        want = RW.strided_partials(x, g, ksize, stride)
    return dict(x=x, w=w, dy=widened(dy, c["width"], c["at"]), y=widened(y, c["width"], c["at"]), want=want, dres=g if c["dres"] else None)


# ================================================================================================ the bf16 calls (k_convh_wide)
# The same three parts for dtfill_conv2d_strided_bf16 and dtfill_conv2d_transpose_bf16 (tests/test_gpu_conv2d_bf16_limits.py).
# bf16 output bits are not stated by a chain, so the tiles of A and B are small integers (x in -8 .. 8, w in -4 .. 4, the
# residual in -9 .. 9, the bias an odd multiple of 0.5, alpha 0.5): every partial sum is exact in any order, the contract then
# promises the exact result, the expectation is an int64 sum, and no output is a zero.  Cases carry bf16=True and are otherwise
# the float32 tables' records: items(), tiles(), out_frame(), device_bytes() and periods() read them as they are (TH, NPAR and
# the passes of k_convh_wide are k_conv_wide's; w is the packed array, a few KB).
HALPHA = 0.5


def _h(**kw):
    return dict(kw, bf16=True, ksize=kw.get("ksize", 3))


HLOOP = {
    "bf16 1x1x16->16": _h(entry="strided", body="k_convh_wide<ConvPlain<1,1>>", ksize=1, cin=16, cout=16, stride=1, B=_B3, H=17, W=1),
    "bf16 3x3x16->128 residual": _h(entry="strided", body="k_convh_wide<ConvPlain<3,1>>", cin=16, cout=128, stride=1, residual=True, B=_B2,
                                    H=1, W=3),
    "bf16 3x3x48->16": _h(entry="strided", body="k_convh_wide<ConvPlain<3,1>>", cin=48, cout=16, stride=1, B=_B3, H=17, W=1),
    "bf16 1x1x16->16 stride 2": _h(entry="strided", body="k_convh_wide<ConvPlain<1,2>>", ksize=1, cin=16, cout=16, stride=2, B=_B3, H=17, W=1),
    "bf16 3x3x16->16 stride 2": _h(entry="strided", body="k_convh_wide<ConvPlain<3,2>>", cin=16, cout=16, stride=2, B=_B3, H=17, W=1,
                                   misaligned=True),
    "bf16 transpose 16->16": _h(entry="transpose", body="k_convh_wide<ConvTransposed>", cin=16, cout=16, B=_B12, H=1, W=65, misaligned=True),
}


def _hlarge(past, by, **kw):
    return _h(**_large(past, by, H=FRAME[0], W=FRAME[1], **kw))


HLARGE = {
    "bf16 strided 3x3x64->16, x past 2 GiB": _hlarge(2 ** 29, _PX * 64, entry="strided", cin=64, cout=16, stride=1),
    "bf16 strided 3x3x64->16 stride 2, x past 4 GiB": _hlarge(2 ** 30, _PX * 64, entry="strided", cin=64, cout=16, stride=2),
    "bf16 strided 1x1x16->64 at 16 of 80, out and residual past 4 GiB": _hlarge(2 ** 30, _PX * 64, entry="strided", ksize=1, cin=16, cout=64,
                                                                               stride=1, residual=True, out_channels=80, out_offset=16),
    "bf16 strided 1x1x64->16 stride 2, x at the limit": _hlarge("limit", _PX * 64, entry="strided", ksize=1, cin=64, cout=16, stride=2),
    "bf16 transpose 64->16, x and out past 2 GiB": _hlarge(2 ** 29, _PX * 64, entry="transpose", cin=64, cout=16),
    "bf16 transpose 16->16, out past 4 GiB": _hlarge(2 ** 30, 4 * _PX * 16, entry="transpose", cin=16, cout=16),
    "bf16 transpose 64->16, x and out at the limit": _hlarge("limit", _PX * 64, entry="transpose", cin=64, cout=16),
}

# (entry, what is at 2^31, arguments) for the bf16 calls, as REFUSED
HREFUSED = (
    ("strided", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3, stride=1)),
    ("strided", "B Ho Wo Cout", dict(B=2 ** 14, H=32, W=32, cin=16, cout=128, ksize=1, stride=1)),
    ("strided", "B Ho Wo out_channels", dict(B=2 ** 14, H=64, W=64, cin=16, cout=16, ksize=3, stride=2, out_channels=128)),
    ("transpose", "B H W Cin", dict(B=2 ** 15, H=32, W=32, cin=64, cout=16, ksize=3)),
    ("transpose", "B Ho Wo Cout", dict(B=2 ** 14, H=16, W=32, cin=16, cout=64, ksize=3)),
    ("transpose", "B Ho Wo out_channels", dict(B=2 ** 14, H=16, W=32, cin=16, cout=16, ksize=3, out_channels=64)),
)


def bf16_tile(c, seed=0):
    """tile() for a bf16 case: integer frames and the int64 sum, finished in float64 (exact: quarters of small integers)."""
    ksize, cin, cout, H, W = c["ksize"], c["cin"], c["cout"], c["H"], c["W"]
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (T, H, W, cin)).astype(F)
    w = rng.integers(-4, 5, (ksize, ksize, cin, cout)).astype(F)
    b = (rng.integers(-9, 9, cout) + 0.5).astype(F)
    res = rng.integers(-9, 10, (T,) + out_frame(c) + (cout,)).astype(F) if c.get("residual") else None
    total = HB.transpose_sum(x, w, np.int64) if c["entry"] == "transpose" else HB.strided_sum(x, w, c["stride"], np.int64)
    y = total.astype(np.float64) + b + (0 if res is None else res)
    want = np.where(y > 0, y, y * HALPHA).astype(F)
    return dict(x=x, w=w, bias=b, residual=res, want=widened(want, c.get("out_channels", cout), c.get("out_offset", 0)))


# ---- C for the bf16 calls.  Values are scaled() values rounded to bf16 on the host, so that the reference's operands are the
# kernel's.  (exponent range of x, of w, of the bias; None: no bias)
HLAYERS = ((3, 1, False, 32, 48), (3, 2, False, 32, 48), (1, 1, False, 48, 32), (3, 2, True, 32, 48))  # ksize, stride, transposed, Cin, Cout
HLAYER_IDS = ["3x3x32->48", "3x3x32->48 stride 2", "1x1x48->32", "transposed 32->48"]
FLT_MAX = float(np.finfo(F).max)
HCLASSES = {
    "near the top": ((58, 61), (58, 61), (100, 110)),  # w is then scaled by a power of two: top_case()
    "over the top": ((62, 63), (63, 64), None),
    "small products": ((-75, -66), (-66, -58), (-135, -128)),
    "tiny products": ((-82, -74), (-66, -58), None),  # S below 2^-126: every partial sum is subnormal, every addition exact
    "subnormal x": ((-134, -128), (20, 30), (-108, -100)),
    "subnormal w": ((20, 30), (-134, -128), (-108, -100)),
}


def hclass_case(name, ksize, cin, cout, shape, seed, stride=1, transposed=False, sign=1):
    """x, w, bias (or None) of bf16 value class `name`; x and w hold bf16 values, except in "near the top".
    near the top: x and w are left unrounded on purpose.  The statement rounds them itself, so the reference's operands are still
    the kernel's, and the kernel's own rounding (ch_round) stays under test: with operands rounded on the host a ch_round that
    truncates would change nothing here, and this class is the control that the range classes do not mask it.  w is scaled by the power of two that puts the largest S of the outputs into [FLT_MAX / 4, FLT_MAX / 2).
    over the top: x > 0 and sign * w > 0 throughout, so that every product has one sign and the partial sums are monotone."""
    (x0, x1), (w0, w1), bexp = HCLASSES[name]
    rng = np.random.default_rng(seed)
    x, w = scaled(rng, shape + (cin,), x0, x1), scaled(rng, (ksize, ksize, cin, cout), w0, w1)
    b = None if bexp is None else scaled(rng, (cout,), *bexp)
    if name == "near the top":  # unrounded: here the rounding is the kernel's own, which the statement repeats
        xr, wr = np.abs(HB.bf16_round(x)), np.abs(HB.bf16_round(w))
        S = HB.transpose_sum(xr, wr) if transposed else HB.strided_sum(xr, wr, stride)
        return x, np.ldexp(w, int(np.floor(np.log2(FLT_MAX / 2 / S.max())))).astype(F), b
    x, w = HB.bf16_round(x), HB.bf16_round(w)
    if name == "over the top":
        x, w = np.abs(x), (sign * np.abs(w)).astype(F)
    return x, w, b


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


# ================================================================================================ the bf16 backward calls
# Parts A and B for dtfill_conv2d_strided_backward_data_bf16 / _weights_bf16 and the transposed pair (k_convhb_dw_wide,
# k_convhb_pack and k_convh_wide behind the workspace plan; tests/test_gpu_conv2d_bf16_backward_limits.py).  The records are
# WLOOP's and WLARGE's own, with bf16=True: wframes(), wsegments(), wworkspace_bytes() and wdevice_bytes() read them as they are.
# k_convhb_dw_wide has its own seg0 / gl0 launch loop and its own 32-bit frame offsets; the group axis's repeat (gl0) needs
# more than a million channels, a weight tensor past the shape rule's own limit, and stays unreachable as for the twin.
# Tiles are small integers (bf16_wtile): every level-1 partial is exact in any order, `want` is the int64 partials, and level2()
# is the contract's stated float32 chain over them.
HBALPHA = 0.25  # exact on the integers
HBLOOP = {"bf16 " + n: dict(c, bf16=True) for n, c in WLOOP.items() if c["entry"] != "dw_image" and c["ksize"] <= 3}
HBLARGE = {"bf16 " + n: dict(c, bf16=True) for n, c in WLARGE.items()
           if c["entry"] != "dw_image" and n != "dx strided 3x3x16->16, dy 128 wide at the limit"}
HBREFUSED = tuple(r for r in WREFUSED if r[0] in ("dx_wide", "dw_wide"))


def bf16_partials(x, g4, ksize, stride, transposed):
    """Level 1 of the bf16 weight sum over integer operands (g4 = 4 g), in int64: [segments, ksize^2 Cin + 1, Cout] in (b, t, s)
    order, each row the sum over the segment's pixels alone, the last row db's."""
    xi, g4 = np.rint(x).astype(np.int64), np.asarray(g4, np.int64)
    cout = g4.shape[3]
    Hs, Ws = (x.shape[1], x.shape[2]) if transposed else (g4.shape[1], g4.shape[2])
    rows = []
    for b, h0, h1, v0, v1 in RB.segments(len(x), Hs, Ws):
        small = xi if transposed else g4
        cut = np.zeros_like(small[b:b + 1])
        cut[0, h0:h1, v0:v1] = small[b, h0:h1, v0:v1]
        if transposed:
            dw, _ = HBB.dw_sum(cut, g4[b:b + 1], 3, 2, True, np.int64)
            db = g4[b, 2 * h0:2 * h1, 2 * v0:2 * v1].reshape(-1, cout).sum(axis=0)  # the segment's four parities
        else:
            dw, db = HBB.dw_sum(xi[b:b + 1], cut, ksize, stride, False, np.int64)
        rows.append(np.concatenate([dw.reshape(-1, cout), db[None]], axis=0))
    return np.stack(rows)


def bf16_wtile(c, seed=0):
    """wtile() for a bf16 case: x in -8 .. 8, w in -4 .. 4, dy in -3 .. 3, alpha 0.25, y of either sign with a few -0.  The dx
    cases take w in 1 .. 4 and dy in 1 .. 3: every sum is positive, so no expected dx or dresidual is a zero (the device
    comparison is by bits, and the contracts leave a zero's sign open).  Every operand is exact in bf16 and every partial sum a
    multiple of 2^-2 below 2^22: exact in any order, asserted."""
    ksize, stride, cin, cout, act, tr = c["ksize"], c["stride"], c["cin"], c["cout"], c["act"], c["transposed"]
    (Ho, Wo), _ = wframes(c)
    rng = np.random.default_rng(seed)
    dx_case = c["entry"] == "dx_wide"
    x = rng.integers(-8, 9, (T, c["H"], c["W"], cin)).astype(F)
    w = rng.integers(1 if dx_case else -4, 5, (ksize, ksize, cin, cout)).astype(F)
    dy = rng.integers(1 if dx_case else -3, 4, (T, Ho, Wo, cout)).astype(F)
    y = rng.standard_normal((T, Ho, Wo, cout)).astype(F)
    y[rng.random(y.shape) < 0.05] = -0.0
    g = RB.g_ref(dy, y, act, HBALPHA)
    g4 = np.rint(g.astype(np.float64) * 4).astype(np.int64)
    assert np.array_equal(g4 / 4.0, g.astype(np.float64))
    for a in (x, w, g):
        assert np.array_equal(HB.bf16_round(a), a), "an operand is not exact in bf16"
    if dx_case:
        total = HBB.dx_sum(g4, np.rint(w).astype(np.int64), stride, tr, np.int64)
    else:
        total = bf16_partials(x, g4, ksize, stride, tr)
    assert np.abs(total).max() < 2 ** 24
    return dict(x=x, w=w, dy=widened(dy, c["width"], c["at"]), y=widened(y, c["width"], c["at"]), want=(total / 4.0).astype(F),
                dres=g if c["dres"] else None)

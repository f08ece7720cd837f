"""The l2 contract of include/dtfill.h by brute force: every pixel against every source, in integers, with numpy.

Independent of the oracle's algorithm (oracle/dtfill_oracle.c runs a two-pass transform) and of the kernels': nothing here is
separable, windowed or searched.  For a set of pixels and the frame's sources it gives, per pixel,
  d2      the smallest exact squared distance (int64),
  d2_2nd  the second smallest, counted with multiplicity: d2_2nd == d2 where two sources tie for the nearest,
  nbest   how many sources lie at d2,
  near    the canonical winner's raster index: the smallest (d2, row, column),
  label   its 1-based raster rank among the frame's sources -- what out_index holds,
  dt      np.sqrt(d2.astype(np.float32)) -- what out_dt holds, compared as uint32 bit patterns (bits()),
and for the set
  big         the pixels with d2 >= 2^24, where float32 no longer tells neighbouring integers apart,
  collisions  the big pixels whose d2 and d2_2nd are DIFFERENT integers that round to the SAME float32: a key compared or
              carried in float picks either source there,
  ties        the big pixels with d2 == d2_2nd: the canonical rule alone picks the winner.
Large frames are checked on a sample of their pixels.  Where the sources that can matter are known (a dense part far from the
pixels: only its edge), `keep` cuts the candidates, and the cut is proved exact before anything is returned: every excluded
source is strictly farther from every pixel than that pixel's runner-up (by the distance to the excluded sources' bounding
box), so neither d2, d2_2nd, nbest nor the winner can change."""
import numpy as np

BIG = 1 << 24
_CELLS = 1 << 22  # pixel x source pairs per chunk


def source_mask(x, src_thr=0.1):
    """The source predicate of the reference, in float32 as the kernels evaluate it: NOT ((1 - x) > src_thr)."""
    return ~((np.float32(1.0) - np.asarray(x, np.float32)) > np.float32(src_thr))


def sources_of(x, src_thr=0.1):
    """(n, 2) int64 rows and columns of the frame's sources in raster order (position k <-> label k + 1)."""
    return np.argwhere(source_mask(x, src_thr)).astype(np.int64)


def bits(dt):
    return np.ascontiguousarray(dt, np.float32).view(np.uint32)


class Nearest:
    """Result of nearest(): the per-pixel arrays above (all of the pixel set's length) and the three index sets."""

    def __init__(self, pix, W, d2, d2_2nd, nbest, near, label):
        self.pix, self.W = pix, W
        self.d2, self.d2_2nd, self.nbest, self.near, self.label = d2, d2_2nd, nbest, near, label
        with np.errstate(invalid="ignore"):
            self.dt = np.where(label > 0, np.sqrt(np.where(label > 0, d2, 0).astype(np.float32)), np.float32(np.inf)).astype(np.float32)
        has2 = d2_2nd >= 0
        self.big = np.flatnonzero((label > 0) & (d2 >= BIG))
        b = np.zeros(len(d2), bool)
        b[self.big] = True
        self.ties = np.flatnonzero(b & has2 & (d2 == d2_2nd))
        self.collisions = np.flatnonzero(b & has2 & (d2 != d2_2nd) & (d2.astype(np.float32) == d2_2nd.astype(np.float32)))

    def frame(self, name, H):
        """A per-pixel array as an H x W map (the pixel set must be the whole frame in raster order)."""
        return getattr(self, name).reshape(H, self.W)


def all_pixels(H, W):
    ii, jj = np.indices((H, W))
    return np.stack([ii.ravel(), jj.ravel()], 1).astype(np.int64)


_INF = np.int64(1) << 62


def _scan(src, cand, pix):
    """The pixels against the candidate sources (indices into src, ascending): smallest and second smallest d2, the number of
    sources at the smallest, the winner's position in src (-1 without candidates)."""
    P = len(pix)
    d2, d2b = np.full(P, _INF), np.full(P, _INF)
    nbest, win = np.zeros(P, np.int64), np.full(P, -1, np.int64)
    step_s = max(1, min(len(cand), 512))
    step_p = max(1, _CELLS // step_s)
    for p0 in range(0, P, step_p):
        sl = slice(p0, p0 + step_p)
        pi, pj = pix[sl, 0, None], pix[sl, 1, None]
        rows = np.arange(len(pi))
        for s0 in range(0, len(cand), step_s):
            k = cand[s0:s0 + step_s]
            d = (pi - src[None, k, 0]) ** 2 + (pj - src[None, k, 1]) ** 2
            a = d.argmin(1)  # the first minimum: the sources are in raster order, so the smallest (row, column) among equals
            m = d[rows, a]
            cnt = (d == m[:, None]).sum(1)
            d[rows, a] = _INF
            m2 = d.min(1)
            o1, o2, oc, ow = d2[sl], d2b[sl], nbest[sl], win[sl]
            less, same = m < o1, m == o1
            d2b[sl] = np.where(less, np.minimum(o1, m2), np.minimum(o2, m))  # the two smallest of {o1, o2, m, m2}, with multiplicity
            nbest[sl] = np.where(less, cnt, np.where(same, oc + cnt, oc))
            win[sl] = np.where(less, k[a], ow)  # an equal minimum of a later chunk has a larger raster index: it does not win
            d2[sl] = np.where(less, m, o1)
    return d2, d2b, nbest, win


def _result(src, pix, W, d2, d2b, nbest, win):
    found = win >= 0
    w = np.maximum(win, 0)
    near = np.where(found, src[w, 0] * W + src[w, 1], -1) if len(src) else np.full(len(pix), -1, np.int64)
    return Nearest(pix, W, np.where(found, d2, -1), np.where(d2b < _INF, d2b, -1), nbest, near, np.where(found, win + 1, 0))


def _raster_order(src, W):
    return len(src) == 0 or bool(np.all(np.diff(src[:, 0] * W + src[:, 1]) > 0))


def nearest(src, pix, W, keep=None):
    """src: (n, 2) sources in raster order (sources_of); pix: (P, 2) pixels; W: the frame's width (for raster indices).
    keep: optional boolean mask over the sources -- only those are compared, the others are proved irrelevant (module
    docstring).  Without sources: label 0, near -1, dt +inf, d2 = d2_2nd = -1.  With one source d2_2nd is -1."""
    src, pix = np.asarray(src, np.int64).reshape(-1, 2), np.asarray(pix, np.int64).reshape(-1, 2)
    assert _raster_order(src, W), "sources must be in raster order"
    cand = np.arange(len(src)) if keep is None else np.flatnonzero(keep)
    d2, d2b, nbest, win = _scan(src, cand, pix)
    if len(cand) < len(src):
        out = src[~np.asarray(keep, bool)]
        r0, r1, c0, c1 = out[:, 0].min(), out[:, 0].max(), out[:, 1].min(), out[:, 1].max()
        dy = np.maximum(np.maximum(r0 - pix[:, 0], pix[:, 0] - r1), 0)
        dx = np.maximum(np.maximum(c0 - pix[:, 1], pix[:, 1] - c1), 0)
        assert np.all(dy * dy + dx * dx > np.where(d2b < _INF, d2b, d2)), "the cut of the candidate sources is not exact for these pixels"
    return _result(src, pix, W, d2, d2b, nbest, win)


def nearest_whole_frame(src, H, W, margin=24, th=32, tw=64):
    """nearest() of every pixel of an H x W frame in raster order, tile by tile: a tile of th x tw pixels is compared with the
    sources inside the tile's box grown by `margin` on every side.  Every source outside that box is at least margin + 1 from
    every pixel of the tile, so the cut is exact for a tile whose every runner-up is nearer than that; a tile where that does
    not hold (a hole) is compared with every source instead.  Same results as nearest(), a dense frame in a tenth of the time."""
    src = np.asarray(src, np.int64).reshape(-1, 2)
    assert _raster_order(src, W), "sources must be in raster order"
    out = [np.empty(H * W, np.int64) for _ in range(4)]
    every = np.arange(len(src))
    for i0 in range(0, H, th):
        rows_in = (src[:, 0] >= i0 - margin) & (src[:, 0] < i0 + th + margin)
        for j0 in range(0, W, tw):
            ii, jj = np.indices((min(th, H - i0), min(tw, W - j0)))
            pix = np.stack([ii.ravel() + i0, jj.ravel() + j0], 1).astype(np.int64)
            cand = np.flatnonzero(rows_in & (src[:, 1] >= j0 - margin) & (src[:, 1] < j0 + tw + margin))
            res = _scan(src, cand, pix)
            if len(cand) < len(src) and not np.all(np.where(res[1] < _INF, res[1], res[0]) < (margin + 1) ** 2):
                res = _scan(src, every, pix)
            at = pix[:, 0] * W + pix[:, 1]
            for o, r in zip(out, res):
                o[at] = r
    return _result(src, all_pixels(H, W), W, *out)


def nearest_in_frame(x, pix=None, src_thr=0.1, keep=None):
    """nearest() of a frame: its sources by the predicate, every pixel unless a set is given."""
    H, W = x.shape
    if pix is None and keep is None:
        return nearest_whole_frame(sources_of(x, src_thr), H, W)
    return nearest(sources_of(x, src_thr), all_pixels(H, W) if pix is None else pix, W, keep)


def l2_route(nsrc, H, W):
    """k_frame's rule for an l2 frame on the default path: "points" (1..512 sources: l2pts_tile), 16 / 32 (k_l2win<10> / <15>),
    0 (the row search, l2env_row).  A frame without sources is the row search's as well."""
    if 1 <= nsrc <= 512:
        return "points"
    if nsrc * 545 >= 14 * H * W:
        return 16
    if nsrc * 2113 >= 14 * H * W:
        return 32
    return 0


def row_threshold(W):
    """A window-kernel frame's row with this many far pixels is redone whole (l2sky_row) instead of pixel by pixel (k_l2far)."""
    return max(32, W >> 3)

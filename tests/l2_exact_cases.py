"""Inputs of test_l2_exact.py (their conditions, from l2_ref alone) and test_gpu_l2_exact.py (the kernels on them).

Every source of every frame carries a value of its own (1 + k / 1024 for a permutation k of the sources), so a wrong winner shows
in the gathered depth as well as in the label.  A case names its frame, the pixel sets it is checked on (each with the mask of
candidate sources l2_ref may cut to), and -- for the hand-built frames -- the planted pixels with the winner each must have.
Cases are built once per process (lru_cache) and never written to.

Far near-ties (d2 >= 2^24), wide and, transposed, tall:
  cluster   120 x 8000, n random sources in the 150 columns at one end; checked on pixels sampled from columns >= 4400.
            n = 500: a handful of sources (l2pts_tile); n = 1200: too thin for a window (l2env_row).
  edge      40 x 8100, 30 % sources in columns < 3700, nothing beyond: a window-kernel frame (route 16) whose every row has 4400
            far pixels and is redone whole (l2sky_row).  Checked on every pixel of columns >= 7800 and a sample of the others.
            (Why 30 %: 4100 columns away a step of one column costs 8200 in d2, more than any difference of two squared row
            offsets in 40 rows, so only the sources of the dense part's LAST column compete for the far pixels.  A collision
            needs two of them in adjacent rows, d2 and d2 + 1; at 8 % that column holds three sources and the far pixels have
            no collision at all.  With seed 5 at 30 %: 12000 far pixels, 600 collisions, 1800 ties.)
  line      120 x 8000 with column 0 full of sources: the runner-up of every far pixel is at d2 + 1.
Ties exactly on a stop bound (small frames, checked on every pixel): ring17, ring33, farpixel, rowcount, win15 -- see each."""
import functools

import numpy as np

import l2_ref

WIDE, TALL = "wide", "tall"


def with_values(mask, seed):
    """float32 frame: the mask's pixels are sources with distinct values 1 + k / 1024 (exact in float32), the rest 0."""
    n = int(mask.sum())
    assert n < (1 << 16)  # values below 65: float32 holds them to 2^-17
    x = np.zeros(mask.shape, np.float32)
    x[mask] = np.float32(1.0) + np.random.default_rng(seed).permutation(n).astype(np.float32) * np.float32(1.0 / 1024)
    return x


class Case:
    """x: the frame; sets: [(pixels (P, 2), keep mask over sources_of(x) or None)]; planted: {name: ((i, j), (winner row, column))}"""

    def __init__(self, name, x, sets, planted=None):
        self.name, self.x, self.sets, self.planted = name, x, sets, planted or {}
        self.src = l2_ref.sources_of(x)

    @functools.cached_property
    def refs(self):
        H, W = self.x.shape
        return [l2_ref.nearest_whole_frame(self.src, H, W) if pix is None else l2_ref.nearest(self.src, pix, W, keep)
                for pix, keep in self.sets]

    @property
    def route(self):
        return l2_ref.l2_route(len(self.src), *self.x.shape)

    def far_rows(self, R):
        """Per row, the number of pixels with no source within R (whole-frame cases: the first set is every pixel)."""
        H, W = self.x.shape
        return (self.refs[0].frame("d2", H) > R * R).sum(1)

    def transposed(self):
        xt = np.ascontiguousarray(self.x.T)
        order = np.lexsort((self.src[:, 0], self.src[:, 1]))  # raster order of the transposed sources, as indices into src
        sets = [(np.ascontiguousarray(pix[:, ::-1]), None if keep is None else keep[order]) for pix, keep in self.sets]
        return Case(self.name, xt, sets)


def _sample(rng, n, rows, cols):
    return np.stack([rng.integers(rows[0], rows[1], n), rng.integers(cols[0], cols[1], n)], 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def cluster(n, orient=WIDE, H=120, W=8000, seed=11, npix=40000, front=0.0):
    """front: that share of the band's last column is made sources as well (a frame of a few rows has its collisions between
    vertical neighbours of that column only: a column's step costs more than any two row offsets differ)"""
    if orient == TALL:
        return cluster(n, WIDE, H, W, seed, npix, front).transposed()
    rng = np.random.default_rng(seed)
    mask = np.zeros((H, W), bool)
    pos = rng.choice(H * 150, n, replace=False)
    mask[pos // 150, pos % 150] = True
    mask[:, 149] |= np.random.default_rng(seed + 1).random(H) < front
    return Case("cluster%d" % n, with_values(mask, seed), [(_sample(rng, npix, (0, H), (4400, W)), None)])


EDGE_H, EDGE_W, EDGE_C, EDGE_P, EDGE_SEED = 40, 8100, 3700, 0.3, 5


@functools.lru_cache(maxsize=None)
def edge(orient=WIDE):
    """sets[0]: every pixel of columns >= 7800 (all of them at d2 >= 2^24: 4101^2 > 2^24) -- the candidates cut to the sources
    of the dense part's last 64 columns; sets[1]: a sample of the other empty columns from 3764 on, the same cut; sets[2]: a
    sample of the dense part and the columns next to it against every source."""
    if orient == TALL:
        return edge(WIDE).transposed()
    H, W, C = EDGE_H, EDGE_W, EDGE_C
    rng = np.random.default_rng(EDGE_SEED)
    mask = np.zeros((H, W), bool)
    mask[:, :C] = rng.random((H, C)) < EDGE_P
    x = with_values(mask, EDGE_SEED)
    ii, jj = np.indices((H, W - 7800))
    far = np.stack([ii.ravel(), jj.ravel() + 7800], 1).astype(np.int64)
    keep = l2_ref.sources_of(x)[:, 1] >= C - 64
    return Case("edge", x, [(far, keep), (_sample(rng, 8000, (0, H), (C + 64, 7800)), keep), (_sample(rng, 1500, (0, H), (0, C + 64)), None)])


def edge_sky_rows(orient):
    """The rows of edge(orient) with at least w2_row_t far pixels (no source within 10) -- the rows k_l2env redoes whole.
    wide: all 40 (columns >= 3711 are far in every row).  tall: the reference counts rows 3690 .. 3719; the rows below 3719 are
    far as a whole (40 >= w2_row_t(40) = 32), and a row above 3690 has fewer far pixels than those farther than 10 from every
    source of the row itself, which is checked to be below 32."""
    c = edge(orient)
    H, W = c.x.shape
    if orient == WIDE:
        assert c.src[:, 1].max() < EDGE_C and W - (EDGE_C + 10) >= l2_ref.row_threshold(W)
        return H
    t = l2_ref.row_threshold(W)
    rows = np.arange(EDGE_C - 10, EDGE_C + 20)
    ii, jj = np.meshgrid(rows, np.arange(W), indexing="ij")
    r = l2_ref.nearest(c.src, np.stack([ii.ravel(), jj.ravel()], 1), W, keep=c.src[:, 0] >= EDGE_C - 100)
    mid = int(((r.d2.reshape(len(rows), W) > 100).sum(1) >= t).sum())
    m = l2_ref.source_mask(c.x[:EDGE_C - 10])
    cols = np.arange(W)
    hx = np.where(m[:, None, :], np.abs(cols[None, :, None] - cols[None, None, :]), W).min(2)  # to the row's own nearest source
    assert ((hx > 10).sum(1) < t).all()
    return mid + (H - (EDGE_C + 20))


@functools.lru_cache(maxsize=None)
def line(orient=WIDE, H=120, W=8000, seed=3, npix=20000):
    if orient == TALL:
        return line(WIDE, H, W, seed, npix).transposed()
    mask = np.zeros((H, W), bool)
    mask[:, 0] = True
    return Case("line", with_values(mask, seed), [(_sample(np.random.default_rng(seed), npix, (0, H), (4100, W)), None)])


# ---- ties exactly on a stop bound ------------------------------------------------------------------------------------

def _dense(H, W, p, seed):
    return np.random.default_rng(seed).random((H, W)) < p


def _clear_disc(mask, i, j, d2max):
    """No source within squared distance d2max of (i, j)."""
    H, W = mask.shape
    r = int(np.sqrt(d2max)) + 1
    i0, i1, j0, j1 = max(i - r, 0), min(i + r + 1, H), max(j - r, 0), min(j + r + 1, W)
    ii, jj = np.indices((i1 - i0, j1 - j0))
    mask[i0:i1, j0:j1] &= ((ii + i0 - i) ** 2 + (jj + j0 - j) ** 2) > d2max


def _whole(name, mask, seed, planted):
    H, W = mask.shape
    return Case(name, with_values(mask, seed), [(None, None)], planted)  # every pixel, in raster order


def _ring(name, H, g, gmin, off, seed):
    """l2sky_row's stop test best >= gmin^2 + (R + 1)^2 met with equality.  W = 256 (32 far pixels make a sky row); nothing
    above row g + 1 but four sources: row 0's pixel j has the source of its own column g rows below, and the column `off`
    (= R + 1) to one side has its source gmin rows below -- the row's smallest column distance -- with off^2 + gmin^2 == g^2.
    Every other column's first source lies deeper than g (12 % below row g).  The two tie at d2 = g^2, and the winner is the
    smaller source row, in the column just OUTSIDE the window that has been searched.  Planted on either side: j - off for the
    pixel (0, 60 + off), j + off for (0, 180)."""
    assert off * off + gmin * gmin == g * g
    W = 256
    mask = np.zeros((H, W), bool)
    mask[g + 1:] = _dense(H - g - 1, W, 0.12, seed)
    ja, jb = 60 + off, 180
    mask[g, ja] = mask[gmin, ja - off] = mask[g, jb] = mask[gmin, jb + off] = True
    return _whole(name, mask, seed, {"left": ((0, ja), (gmin, ja - off)), "right": ((0, jb), (gmin, jb + off))})


@functools.lru_cache(maxsize=None)
def ring17():
    """first ring, R = 16 -> 17: 17^2 + 144^2 = 145^2"""
    return _ring("ring17", 200, 145, 144, 17, 21)


@functools.lru_cache(maxsize=None)
def ring33():
    """second ring, R = 32 -> 33: 33^2 + 56^2 = 65^2"""
    return _ring("ring33", 120, 65, 56, 33, 22)


def _plant(mask, i, j, d2clear, offsets):
    _clear_disc(mask, i, j, d2clear)
    for di, dj in offsets:
        mask[i + di, j + dj] = True


R10_TIE = [(0, -10), (0, 10), (-6, -8), (-6, 8), (6, -8), (6, 8)]   # d2 = 100: the window's; winner (-6, -8)
R10_FAR = [(-1, -10), (-1, 10), (1, -10), (1, 10)]                  # d2 = 101: handed on; winner (-1, -10)
R15_TIE = [(0, -15), (0, 15), (-9, -12), (-9, 12), (9, -12), (9, 12)]  # d2 = 225; winner (-9, -12)
R15_FAR = [(-1, -15), (-1, 15), (1, -15), (1, 15)]                  # d2 = 226; winner (-1, -15)


@functools.lru_cache(maxsize=None)
def farpixel():
    """128 x 640 at 3.2 % (route 16, row threshold 80).
    P = (64, 160): no source within 32 but the four at exactly 32 on the axes; the winner (32, 160) is seen only in
    l2far_pixel's round base = 32, which runs only because base^2 <= best admits equality (two pixels share a wave and the wave
    goes on while EITHER wants to: every other far pixel of the frame is nearer than 32 to a source -- asserted -- so P's
    partner never keeps the wave going).
    A = (64, 420): nearest sources at d2 = 100 = R^2 of k_l2win<10>: decided by the window; B = (64, 500): at d2 = 101: handed on."""
    mask = _dense(128, 640, 0.032, 23)
    _plant(mask, 64, 160, 1024, [(0, 32), (0, -32), (32, 0), (-32, 0)])
    _plant(mask, 64, 420, 100, R10_TIE)
    _plant(mask, 64, 500, 101, R10_FAR)
    return _whole("farpixel", mask, 23, {"P": ((64, 160), (32, 160)), "A": ((64, 420), (58, 412)), "B": ((64, 500), (63, 490))})


ROWCOUNT_ROWS = {20: 79, 64: 80, 108: 81}


@functools.lru_cache(maxsize=None)
def rowcount():
    """128 x 640 at 3.2 % (route 16): rows 20, 64 and 108 hold exactly 79, 80 and 81 pixels with no source within 10 -- one
    below, on and one above the threshold w2_row_t(640) = 80 between the far list and the sky rows.  Around each of the rows 21
    rows are emptied in three stretches of columns, one per 256-column tile of the window kernel and each across a wave's seam
    (columns 128, 320, 576), with a source at either end of the stretch in the row itself: a stretch of n columns leaves the
    n - 20 pixels in its middle far from every source, so several waves of several blocks add up the row's count."""
    mask = _dense(128, 640, 0.032, 24)
    for r, total in ROWCOUNT_ROWS.items():
        lens = [total // 3 + (1 if k < total % 3 else 0) + 20 for k in range(3)]
        for a, n in zip((100, 300, 560), lens):
            mask[r - 10:r + 11, a:a + n] = False
            mask[r, a - 1] = mask[r, a + n] = True
    return _whole("rowcount", mask, 24, {})


@functools.lru_cache(maxsize=None)
def win15():
    """130 x 1216 at 0.9 % (route 32): A = (64, 300) with its nearest sources at d2 = 225 = R^2 of k_l2win<15>, B = (64, 700) at 226."""
    mask = _dense(130, 1216, 0.009, 25)
    _plant(mask, 64, 300, 225, R15_TIE)
    _plant(mask, 64, 700, 226, R15_FAR)
    return _whole("win15", mask, 25, {"A": ((64, 300), (55, 288)), "B": ((64, 700), (63, 685))})


SMALL = (ring17, ring33, farpixel, rowcount, win15)

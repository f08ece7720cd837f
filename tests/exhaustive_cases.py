"""Exhaustive source patterns on the seams of the kernels' own geometry (builders only: no GPU, no torch, no fixtures).

The random frames of the other tests almost never put a dense cluster of sources in sparse surroundings on a boundary of a
kernel's geometry: at 5 % density a given 3 x 3 pattern with four or more sources occurs about once in 10^5 positions.  Here
every pattern is enumerated: all 2^(ph*pw) masks of a small patch over one fixed background, the patch placed so that it
straddles a bit word, a 32-row band, a tile seam, the frame's corner, or is the sky's base rows; and every non-empty mask of
a whole frame of at most 16 pixels.

Every source's value is 1 + (row * W + col) / 256: exact in float32, >= 0.95 (a source and a value alike), and distinct, so
that the filled depth names the label's source.

The kernels' constants are restated below, each with the place it is defined at (paths under
distancetransform-depthcompletion_amd/csrc/); route() restates frame_facts' routing rule, window_tiles() the window kernel's
tile origins, so that a sweep can say on the CPU which kernel family its frames go to (tests/test_exhaustive_cases.py holds
every sweep to that; tests/test_gpu_exhaustive.py holds the device's pass_stats() to it).
"""
import functools
import zlib

import numpy as np

import parallel_model as PM

# ---- the kernels' constants ---------------------------------------------------------------------------------------------
F_WHM, F_WWM = 128, 192      # dtfill_fused.hpp:26-27   the window kernel's window: rows, columns
L2_PTS_MAX = 512             # dtfill_common.hpp:24     a frame with at most this many sources can be a points frame
W2_R = {16: 10, 32: 15}      # dtfill_common.hpp:25     l2: k_l2win's radius on route 16 / 32 (W2_R16, W2_R32)
PTS_BAND_MAX = 96            # dtfill_common.hpp:31     l1_cv points frame: at most this many sources in a band of 32 rows
PREMARK = {16: 8, 32: 16}         # dtfill_common.hpp:36     l1_cv: rows farther than this from every source row are pre-marked (PM16, PM32)
SKY_MAX, SKY_MIN = 320, 9    # dtfill_common.hpp:37-38  the rows above the first source row are k_sky's from SKY_MIN rows on
BAND = 32                    # dtfill_prepass.hpp:281-284 (bandmax), dtfill_common.hpp:140 (ct): the any-distance kernels' row bands
WORDS = (32, 64)             # dtfill_common.hpp:45 (32-pixel words of the bit rows), :134 (64-pixel words of srcbits / valbits)
PTS_TILES = {False: (32, 256), True: (64, 128)}  # dtfill_pts.hpp:37-38, dtfill.hip:328-331  k_pts's tile: wide / tall
PTS_WAVE = (32, 64)          # dtfill_pts.hpp:37        ... of waves of 32 rows x 64 columns
PT_T = 32                    # dtfill_l2.hpp:697        l2 points route: 32 x 32 tiles
W2_TH, W2_TW = 32, 256       # dtfill_l2.hpp:56         k_l2win's tile


def w2_row_t(W):             # dtfill_l2.hpp:59         l2: a row with this many far pixels is handed to the row search
    return max(32, W >> 3)


WHOLE_SHAPES = [(1, 16), (16, 1), (2, 8), (8, 2), (4, 4), (3, 5), (5, 3)]  # whole_frames(): every mask of each, as one batch
B_MAX = 65535                # the largest batch (include/dtfill.h): whole_frames(4, 4) is exactly that many frames
RING = 6                     # background sources keep this far (Chebyshev) from the patch


def value_frame(H, W):
    """The value a source at (row, col) carries: 1 + (row * W + col) / 256, float32 (exact: row * W + col + 256 < 2^24)."""
    assert H * W + 256 < 1 << 24
    return (np.float32(1.0) + np.arange(H * W, dtype=np.float32).reshape(H, W) / np.float32(256.0)).astype(np.float32)


def sources(x, src_thr=0.1):
    """The source predicate of the pass, NOT((1 - x) > src_thr), in float32."""
    return ~((np.float32(1.0) - np.asarray(x, np.float32)) > np.float32(src_thr))


def patch_batch(H, W, r, c, ph, pw, background):
    """float32 [2^(ph*pw), H, W]: frame k = background + a source at (r + i // pw, c + i % pw) for every set bit i of k.
    The background must hold nothing on the patch."""
    background = np.asarray(background, np.float32)
    assert background.shape == (H, W) and 0 <= r and r + ph <= H and 0 <= c and c + pw <= W
    assert not background[r:r + ph, c:c + pw].any()
    n = ph * pw
    bits = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool).reshape(1 << n, ph, pw)
    x = np.repeat(background[None], 1 << n, axis=0)
    x[:, r:r + ph, c:c + pw] = np.where(bits, value_frame(H, W)[r:r + ph, c:c + pw], np.float32(0.0))
    return x


def whole_frames(H, W):
    """float32 [2^(H*W) - 1, H, W]: every non-empty source mask of an H x W frame of at most 16 pixels (mask k + 1 in frame k)."""
    assert H * W <= 16
    return patch_batch(H, W, 0, 0, H, W, np.zeros((H, W), np.float32))[1:]


def misaligned(x):
    """The batch with a valued pixel that is no source at (0, 0) (0.5: above val_thr 0.1, not within src_thr 0.1 of 1): every
    label then reads depth_list one entry further on."""
    x = np.array(x, np.float32)
    assert not x[:, 0, 0].any()
    x[:, 0, 0] = 0.5
    return x


# ---- where the seams are ------------------------------------------------------------------------------------------------
def window_tiles(H, W, R, tbase=0):
    """The window kernel's tiling for halo R: (row origins, column origins).  dtfill.hip:250-262 (the host: nty, ntx from
    the whole frame, TW in whole 32-pixel words when the window allows it), dtfill_fused.hpp:385-387 (the tile rows split
    the rows from tbase = FI_TR0 on evenly; dtfill_prepass.hpp:438: tbase is the first source row under a sky, else 0)."""
    THM, TWM = F_WHM - 2 * R, F_WWM - 2 * R
    nty, ntx = -(-H // THM), -(-W // TWM)
    TW = -(-W // ntx)
    if ((TW + 31) & ~31) <= TWM:
        TW = (TW + 31) & ~31
    TH = -(-(H - tbase) // nty)
    rows = [tbase + t * TH for t in range(nty) if tbase + t * TH < H]
    cols = [t * TW for t in range(ntx) if t * TW < W]
    return np.array(rows), np.array(cols)


def pts_tall(H, W):
    """dtfill.hip:329-330: k_pts takes 64 x 128 tiles where they waste fewer waves than 32 x 256."""
    nwide = -(-W // 256) * -(-H // 32)
    ntall = -(-W // 128) * -(-H // 64)
    return ntall < nwide


# win16, win32: the window kernel with halo 16 / 32 (l2: k_l2win with radius 10 / 15); anydist: the smallest frame with a 32-row band
# boundary, a handful of sources (k_pts's 32 x 256 tiles and the l2 points route on the default path, the any-distance kernels on the
# forced one); pts: the smallest frame on which k_pts takes its 64 x 128 tiles and has a seam in both directions (dtfill.hip:329-330:
# W in 257..384, H in 97..128); thin: more than L2_PTS_MAX sources, too thin for halo 32 -- the any-distance kernels and the l2 row
# search on the default path, distances of 40 and more; sky: a window frame under SKY_MIN or more empty rows
FAMILIES = ("win16", "win32", "anydist", "pts", "thin", "sky")
SHAPES = {"win16": (104, 200), "win32": (104, 200), "anydist": (40, 136), "pts": (100, 264), "thin": (104, 768), "sky": (40, 200)}
PATCHES = {"anydist": (3, 4)}  # 3 x 4 (4096 masks) where the frame is under 6000 pixels, 3 x 3 (512) elsewhere


def patch_of(family):
    return PATCHES.get(family, (3, 3))


SKY_TOP = 12   # the sky sweeps: the patch's first row (>= SKY_MIN empty rows above it); the body starts SKY_GAP rows below the patch
SKY_GAP = 1


def anchors(family, H, W):
    """name -> (r, c): where the family's patch goes so that it straddles a boundary (rows r | r + 1, r + 2 or columns likewise: a
    boundary at b puts the patch at b - 1, one line before it and the others behind)."""
    ph, pw = patch_of(family)
    out = {}
    # an interior position off every boundary below, for the anchors that pin only one coordinate
    rmid, cmid = {"win16": (20, 78), "win32": (20, 78), "anydist": (12, 100), "pts": (20, 200), "thin": (20, 200), "sky": (SKY_TOP, 78)}[family]
    if family == "sky":
        # the patch is the frame's first three source rows; on a 64-pixel word boundary, and on the window kernel's column seam
        cols = window_tiles(H, W, 16, SKY_TOP)[1]
        assert len(cols) == 2 and np.array_equal(cols, window_tiles(H, W, 32, SKY_TOP)[1])
        return {"word63": (SKY_TOP, WORDS[1] - 1), "colseam": (SKY_TOP, int(cols[1]) - 1)}
    # every family: the bit words' boundaries and the frame's corners
    out["col31"] = (rmid, WORDS[0] - 1)
    out["col63"] = (rmid, WORDS[1] - 1)  # (also a seam of k_pts's waves, PTS_WAVE)
    out["topleft"] = (0, 0)
    out["bottomright"] = (H - ph, W - pw)
    if family in ("win16", "win32"):
        rows, cols = window_tiles(H, W, int(family[3:]))
        assert len(rows) == 2 and len(cols) == 2
        out["colseam"] = (rmid, int(cols[1]) - 1)
        out["rowseam"] = (int(rows[1]) - 1, cmid)
        out["cross"] = (int(rows[1]) - 1, int(cols[1]) - 1)
        out["row31"] = (W2_TH - 1, cmid)  # l2: a row seam of k_l2win's tiles (their 256 columns leave no column seam in this frame)
    if family == "anydist":
        # the any-distance kernels' 32-row band; with column 31 | 32 also the corner of four of the l2 points route's 32 x 32 tiles,
        # and (H x W takes k_pts's 32 x 256 tiles) a row seam of those
        assert H > BAND and not pts_tall(H, W)
        out["band31"] = (BAND - 1, cmid)
        out["cross31"] = (PT_T - 1, PT_T - 1)
    if family == "thin":
        # the band boundary again, on a 64-pixel word boundary; the other anchors of "every family" are left to the smaller frames
        # (a sweep here is 41 M pixels)
        return {"col31": out["col31"], "band31x63": (BAND - 1, 63)}
    if family == "pts":
        assert pts_tall(H, W)
        th, tw = PTS_TILES[True]
        assert H > th and W > tw
        out["rowseam"] = (th - 1, cmid)
        out["colseam"] = (rmid, tw - 1)
        out["cross"] = (th - 1, tw - 1)
    for name, (r, c) in out.items():
        assert 0 <= r <= H - ph and 0 <= c <= W - pw, (family, name)
    return out


# ---- which kernel family takes a frame ----------------------------------------------------------------------------------
def route(src, metric="l1_cv", path="auto"):
    """frame_facts' routing (dtfill_prepass.hpp:366-441) for a pass without a depth epilogue, restated: a dict with
      r       16 / 32 (the window kernel with that halo; l2: k_l2win with radius W2_R[r]), -1 (the points route), 0 (any distance)
      sky     rows [0, sky) are k_sky's (l1_cv)
      far     rows handed to the any-distance kernels up front (l1_cv: pre-marked rows, culled tile rows, a sky that is not k_sky's;
              l2: rows farther than the radius from every source row)
    as the publishing block decides them: rows the window kernels hand on later (a pixel beyond the halo) are not in it."""
    src = np.asarray(src, bool)
    H, W = src.shape
    nsrc = int(src.sum())
    l2, general = metric == "l2", path == "general"
    has = src.any(axis=1)
    ii = np.arange(H)
    srows = np.flatnonzero(has)
    r0 = int(srows[0]) if srows.size else H
    vd = np.abs(ii[:, None] - srows[None, :]).min(axis=1) if srows.size else np.full(H, 1 << 20)
    premark = not l2 and not general  # (mode bits 4 | 8, dtfill.hip:268-272)
    sky_ok = premark and SKY_MIN <= r0 <= SKY_MAX and r0 < H                                        # :367
    far = {R: (vd > W2_R[R]) if l2 else ((ii >= r0) & (vd > PREMARK[R])) for R in (16, 32)}               # :346
    dlb = int(vd.max()) if srows.size else 0

    def fits(R):                                                                                     # :380-386
        ball = 2 * R * R + 2 * R + 1
        if l2:
            return nsrc * ball >= 14 * H * W
        if not premark:
            return nsrc * ball >= 14 * H * W and dlb <= R
        rest = H - (r0 if sky_ok else 0) - int(far[R].sum())
        return rest > 0 and nsrc * ball >= 14 * rest * W

    bandmax = max(int(src[a:a + BAND].sum()) for a in range(0, H, BAND))
    points = l2 and not general and 0 < nsrc <= L2_PTS_MAX                                           # :390
    points1 = premark and 0 < nsrc <= L2_PTS_MAX and bandmax <= PTS_BAND_MAX                         # :393
    window = 16 if fits(16) else 32 if fits(32) else 0
    r = 0 if general else -1 if points else window if window else -1 if points1 else 0               # :395
    out = dict(r=r, sky=0, far=0, nsrc=nsrc, r0=r0)
    if r <= 0:
        return out
    f = far[r].copy()
    if l2:
        out["far"] = int(f.sum())
        return out
    if not premark:
        return out
    tbase = r0 if sky_ok else 0
    rows = window_tiles(H, W, r, tbase)[0]
    for a, e in zip(rows, list(rows[1:]) + [H]):                                                     # :412-424
        keep = int((~f[a:e]).sum())
        if keep and 4 * keep <= e - a:
            f[a:e] = True
    sky = sky_ok and not f[r0] and not (r0 + 1 < H and f[r0 + 1])                                    # :427
    out["sky"] = r0 if sky else 0
    out["far"] = int(f.sum()) + (r0 if sky_ok and not sky else 0)
    return out


def expected_stats(x, metric="l1_cv", path="auto"):
    """What DtFill.pass_stats() reports for batch x when no window block hands a row on: dict all, window, anydist, sky, points
    in pixels (dtfill_post.hpp:154-188)."""
    B, H, W = x.shape
    s = dict(all=B * H * W, window=0, anydist=0, sky=0, points=0)
    for f in x:
        rt = route(sources(f), metric, path)
        if rt["r"] > 0:
            s["sky"] += rt["sky"] * W
            s["anydist"] += rt["far"] * W
            s["window"] += (H - rt["sky"] - rt["far"]) * W
        elif rt["r"] == 0:
            s["anydist"] += H * W
        else:
            s["points"] += H * W
    return s


# ---- the sweeps -----------------------------------------------------------------------------------------------------------
# what a family's background must make of every frame of its sweeps on path "auto": {metric: route r}
WANT_ROUTE = {"win16": {"l1_cv": 16, "l2": 16}, "win32": {"l1_cv": 32, "l2": 32}, "anydist": {"l1_cv": -1, "l2": -1},
              "pts": {"l1_cv": -1, "l2": -1}, "thin": {"l1_cv": 0, "l2": 0}, "sky": {"l1_cv": 16, "l2": 16}}
# sources in the background.  win16: 5 %; win32: above L2_PTS_MAX (else l2 takes the points route) and under the 2.57 % halo 16 asks
# for; anydist, pts: a handful, too thin for halo 32 (nsrc * 2113 < 14 * H * W), all of them far from the patch; thin: just above L2_PTS_MAX with
# the patch's own still under what halo 32 asks for (529 in 104 x 768); sky: a 15 % body
NBG = {"win16": 1040, "win32": 520, "anydist": 24, "pts": 60, "thin": 515}
SKY_BODY = 0.15


def _background(family, H, W, r, c, seed):
    ph, pw = patch_of(family)
    rng = np.random.default_rng(seed)
    ok = np.ones((H, W), bool)
    ok[max(0, r - RING):r + ph + RING, max(0, c - RING):c + pw + RING] = False
    ok[0, 0] = False  # (free for misaligned()'s valued pixel)
    val = value_frame(H, W)
    bg = np.zeros((H, W), np.float32)
    if family == "sky":
        body = rng.random((H, W)) < SKY_BODY
        body[:r + ph + SKY_GAP] = False
        body[0, 0] = False
        return np.where(body, val, np.float32(0.0))
    pos = rng.choice(np.flatnonzero(ok), NBG[family], replace=False)
    bg.flat[pos] = val.flat[pos]
    return bg


def sweep_ok(family, x, metric):
    """Does every frame of the sweep go where the family wants it, and can no window block hand a row on?  Checked on mask 0 and
    mask all-ones: the route's inputs (source count, empty rows) and every distance are monotone in the mask in between.
    Returns None or the reason."""
    H, W = x.shape[1:]
    for k in (0, len(x) - 1):
        src = sources(x[k])
        rt = route(src, metric)
        want = WANT_ROUTE[family][metric]
        if rt["r"] != want:
            return "mask %d: route %d, wanted %d" % (k, rt["r"], want)
        if family == "sky" and metric == "l1_cv" and (rt["sky"] < SKY_MIN or rt["far"]):
            return "mask %d: sky %d far %d" % (k, rt["sky"], rt["far"])
        if family in ("win16", "win32") and (rt["sky"] or rt["far"]):
            return "mask %d: sky %d far %d in a window sweep" % (k, rt["sky"], rt["far"])
    if want > 0:
        # the largest distances are mask 0's (fewest sources); under a sky the rows from the first source row on count, so the masks
        # of one source are looked at too (every other mask holds one of them with the same first row, and only smaller distances)
        for k in [0] + ([1 << i for i in range(9)] if family == "sky" else []):
            src = sources(x[k])
            if metric == "l1_cv":
                # exact L1 distances by the separable scans of the model (tests/test_parallel_model.py holds them to the oracle)
                gu, g = PM.colscan(src)
                below = PM.rowscan(g, gu, np.full(src.shape, PM.BIG, np.int64))[0][route(src)["sky"]:]
                if below.max() > want:
                    return "mask %d: a pixel %d from every source, halo %d" % (k, below.max(), want)
            elif family != "sky":
                nfar = (~PM.l2_window(src, W2_R[want])[2]).sum(axis=1)
                if nfar.max() >= w2_row_t(W):
                    return "mask %d: a row with %d far pixels" % (k, nfar.max())
    return None


def sweep_names():
    """Every (family, anchor) of the GPU sweeps."""
    return [(f, a) for f in FAMILIES for a in anchors(f, *SHAPES[f])]


@functools.lru_cache(maxsize=2)
def sweep(family, anchor):
    """(x float32 [2^(ph*pw), H, W], (r, c)) of one sweep: the first background (seeds in order from a hash of the names) that sends mask 0
    and mask all-ones where the family wants them in both metrics.  Shared: callers do not write to it."""
    H, W = SHAPES[family]
    r, c = anchors(family, H, W)[anchor]
    seed0 = zlib.crc32(("%s/%s" % (family, anchor)).encode())
    why = None
    for t in range(64):
        x = patch_batch(H, W, r, c, *patch_of(family), _background(family, H, W, r, c, seed0 + t))
        why = sweep_ok(family, x, "l1_cv") or sweep_ok(family, x, "l2")
        if why is None:
            x.setflags(write=False)
            return x, (r, c)
    raise AssertionError("no background for %s/%s: %s" % (family, anchor, why))


def sky_first_rows(family, anchor):
    """r0 of every frame of a sky sweep, from the masks alone: the patch's first row that holds a set bit, the body's first row
    for mask 0."""
    x, (r, c) = sweep(family, anchor)
    return np.array([int(np.flatnonzero(sources(f).any(axis=1))[0]) for f in x])


# ---- the CPU-only set: small enough for the numpy models ------------------------------------------------------------------
def cpu_sets():
    """name -> float32 batch for tests/test_exhaustive_cases.py: every 3 x 4 whole frame, a lone 3 x 4 patch, and a 3 x 3 patch beside
    sources that lie farther off than a patch is wide.  The lone patch cannot tie the left neighbour (0, -1) with the tap one row up and
    two to the right (-1, +2): that takes two sources one row and five columns apart -- the background source at (5, 9) and the patch
    pixel (6, 4)."""
    sets = {"whole3x4": whole_frames(3, 4)}
    sets["patch3x4_in_7x8"] = patch_batch(7, 8, 2, 2, 3, 4, np.zeros((7, 8), np.float32))
    H, W = 12, 16
    val = value_frame(H, W)
    bg = np.zeros((H, W), np.float32)
    for p in ((5, 9), (0, 15), (11, 0), (1, 2), (10, 13), (11, 7)):
        bg[p] = val[p]
    sets["patch3x3_in_12x16"] = patch_batch(H, W, 6, 4, 3, 3, bg)
    return sets


# ---- regression cases -----------------------------------------------------------------------------------------------------
# (family, anchor, mask index, metric, path) of a mask on which a kernel differed from the oracle: kept by name once a sweep finds
# one.  Empty: every sweep above agrees with the oracle on every path.
REGRESSIONS = ()

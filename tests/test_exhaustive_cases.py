"""CPU side of the exhaustive sweeps (tests/exhaustive_cases.py): the oracle against brute force on every mask of a tiny frame, the
numpy models of the kernels' formulations (tests/parallel_model.py) against the oracle on every mask of the small sets, the
sweeps' routing arithmetic, and the sets' power to tell a wrong tie-break from the right one."""
import contextlib

import numpy as np
import pytest

import exhaustive_cases as E
import parallel_model as PM
from helpers import dt_bits

WHOLE_SHAPES = E.WHOLE_SHAPES


# ---- whole frames: the oracle against brute force over all pixel / source pairs ------------------------------------------------
def _brute(x):
    """From the masks alone: (d1 [B, P] minimum L1 distance, isnear1 [B, P, P] "source q is a nearest one of pixel p" in L1,
    d2 [B, P] minimum squared distance, near2 [B, P] the nearest source of smallest raster index in L2, rank [B, P] 1-based raster rank
    of every source, 0 elsewhere)."""
    B, H, W = x.shape
    src = E.sources(x).reshape(B, -1)
    ii, jj = np.divmod(np.arange(H * W), W)
    di, dj = np.abs(ii[:, None] - ii[None, :]), np.abs(jj[:, None] - jj[None, :])
    big = 1 << 20
    m1 = np.where(src[:, None, :], (di + dj)[None], big)
    m2 = np.where(src[:, None, :], (di * di + dj * dj)[None], big)
    d1, d2 = m1.min(axis=2), m2.min(axis=2)
    rank = np.cumsum(src, axis=1) * src
    return d1, (m1 == d1[..., None]) & src[:, None, :], d2, m2.argmin(axis=2), rank


@pytest.mark.parametrize("shape", WHOLE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_on_every_mask_of_a_whole_frame(oracle, shape):
    """Every non-empty mask of the frame, both metrics.  dt is the minimum L1 distance and every l1_cv label one of the nearest
    sources (cv2's choice among them is the oracle's to make); the l2 label is the nearest source of smallest raster index, d2 exact and
    dt its correctly rounded root (tests/l2_ref.py's contract); depth is the labelled source's own value."""
    x = E.whole_frames(*shape)
    B, H, W = x.shape
    assert B == (1 << H * W) - 1
    d1, isnear1, d2, near2, rank = _brute(x)
    frames, pix = np.arange(B)[:, None], np.arange(H * W)[None, :]
    val = E.value_frame(H, W).ravel()
    pixel_of = lambda lbl: np.argmax(rank[:, None, :] == lbl.reshape(B, -1, 1), axis=2)  # label -> the source's pixel
    depth, dt, lbl, status = oracle.fill_batch(x)
    assert not status.any() and lbl.min() >= 1
    assert np.array_equal(dt.reshape(B, -1), d1.astype(np.float32))
    at = pixel_of(lbl)
    assert (rank[frames, at] == lbl.reshape(B, -1)).all() and isnear1[frames, pix, at].all()
    assert np.array_equal(depth.reshape(B, -1), val[at])
    depth, dt, lbl, status = oracle.fill_batch(x, metric="l2")
    assert not status.any()
    assert np.array_equal(lbl.reshape(B, -1), rank[frames, near2])
    assert np.array_equal(dt_bits(dt.reshape(B, -1)), dt_bits(np.sqrt(d2.astype(np.float32))))
    assert np.array_equal(depth.reshape(B, -1), val[near2])
    for k in range(0, B, max(1, B // 64)):  # d2 itself, and the source's raster index, from the exact transform's own entry point
        d2o, nearo = oracle.edt_l2((~E.sources(x[k])).astype(np.uint8))
        assert np.array_equal(d2o.ravel(), d2[k]) and np.array_equal(nearo.ravel(), near2[k])


def test_whole_frames_fill_the_largest_batch():
    assert len(E.whole_frames(4, 4)) == E.B_MAX
    x = E.whole_frames(2, 2)
    assert np.array_equal(E.sources(x).reshape(-1, 4) @ (1 << np.arange(4)), np.arange(1, 16))
    assert np.array_equal(x[14], np.float32(1.0) + np.arange(4, dtype=np.float32).reshape(2, 2) / 256)


# ---- the builders and the routing arithmetic -------------------------------------------------------------------------------
def test_patch_batch_layout():
    bg = np.zeros((9, 11), np.float32)
    bg[0, 10] = E.value_frame(9, 11)[0, 10]
    x = E.patch_batch(9, 11, 4, 5, 2, 3, bg)
    assert x.shape == (64, 9, 11) and x.dtype == np.float32
    src = E.sources(x)
    for k in (0, 1, 8, 37, 63):
        want = np.zeros((9, 11), bool)
        want[0, 10] = True
        for i in range(6):
            if k >> i & 1:
                want[4 + i // 3, 5 + i % 3] = True
        assert np.array_equal(src[k], want)
        assert np.array_equal(x[k][want], E.value_frame(9, 11)[want]) and not x[k][~want].any()
    m = E.misaligned(x)
    assert np.array_equal(E.sources(m), src) and (m[:, 0, 0] == 0.5).all() and ((m > 0.1).sum(axis=(1, 2)) == src.sum(axis=(1, 2)) + 1).all()


def test_anchors_straddle_the_boundaries():
    for fam in E.FAMILIES:
        H, W = E.SHAPES[fam]
        a = E.anchors(fam, H, W)
        if fam == "sky":
            assert a["word63"][1] == 63 and a["colseam"][1] == 127 and a["word63"][0] >= E.SKY_MIN
            continue
        ph, pw = E.patch_of(fam)
        assert a["col31"][1] == 31
        if fam == "thin":
            assert a["band31x63"] == (31, 63)
            continue
        assert a["col63"][1] == 63 and a["topleft"] == (0, 0) and a["bottomright"] == (H - ph, W - pw)
    # 104 x 200: both halos split the rows 52 | 52 and the columns 128 | 72 (whole words)
    for R in (16, 32):
        rows, cols = E.window_tiles(104, 200, R)
        assert list(rows) == [0, 52] and list(cols) == [0, 128]
    a = E.anchors("win16", 104, 200)
    assert a["rowseam"][0] == 51 and a["colseam"][1] == 127 and a["cross"] == (51, 127) and a["row31"][0] == 31
    # the tile rows split the rows below a sky evenly: 352 rows from row 100 on in four tile rows of halo 16 (96 rows a tile at most)
    assert list(E.window_tiles(352, 1216, 16, 100)[0]) == [100, 163, 226, 289] and list(E.window_tiles(352, 1216, 16)[1][:3]) == [0, 160, 320]
    assert E.anchors("anydist", 40, 136)["band31"][0] == 31
    p = E.anchors("pts", 100, 264)
    assert E.pts_tall(100, 264) and not E.pts_tall(72, 136) and p["rowseam"][0] == 63 and p["colseam"][1] == 127


@pytest.mark.parametrize("family", E.FAMILIES)
def test_sweeps_go_to_the_family_under_test(family):
    """frame_publish's routing rule, restated in exhaustive_cases.route(), on mask 0 and mask all-ones of every sweep: the window
    backgrounds are the window kernel's with the intended halo and nothing pre-marked, the sparse ones k_pts's (l2: the points
    route), the sky sweeps a window frame under a sky; and on the forced path everything is the any-distance kernels'."""
    for fam, anchor in E.sweep_names():
        if fam != family:
            continue
        x, (r, c) = E.sweep(fam, anchor)
        H, W = x.shape[1:]
        ph, pw = E.patch_of(fam)
        last = (1 << ph * pw) - 1
        assert x.shape[0] == last + 1 and (H, W) == E.SHAPES[fam]
        for metric in ("l1_cv", "l2"):
            for k in (0, last):
                src = E.sources(x[k])
                rt = E.route(src, metric)
                assert rt["r"] == E.WANT_ROUTE[fam][metric], (anchor, metric, k, rt)
                assert E.route(src, metric, "general")["r"] == 0
                # the rule itself, spelled out once more for the frames at hand
                n = int(src.sum())
                if fam in ("win16", "win32"):
                    assert n * 545 >= 14 * H * W if fam == "win16" else n * 545 < 14 * H * W <= n * 2113
                    assert n > 512
                if fam == "thin":
                    assert n > 512 and n * 2113 < 14 * H * W and src.any(axis=1).all()
                if fam in ("anydist", "pts"):
                    assert n <= 512 and n * 2113 < 14 * H * W and max(src[a:a + 32].sum() for a in range(0, H, 32)) <= 96
        # the ring: no background source within RING of the patch
        box = E.sources(x[0])[max(0, r - E.RING):r + ph + E.RING, max(0, c - E.RING):c + pw + E.RING]
        assert fam == "sky" or not box.any()
        if fam == "sky":
            src = E.sources(x[0])
            assert not src[:r + 3 + E.SKY_GAP].any() and src[r + 3 + E.SKY_GAP:].mean() > 0.1
            assert E.route(E.sources(x[1]))["sky"] == r and E.route(src)["sky"] == r + 3 + E.SKY_GAP


# ---- the models on every mask of the small sets ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_sets(oracle):
    """name -> (x, dt, lbl) of the CPU sets: one oracle call per set, shared (nobody writes to them)."""
    out = {}
    for name, x in E.cpu_sets().items():
        _, dt, lbl, status = oracle.fill_batch(x)
        assert not status[1 if name != "whole3x4" else 0:].any()
        out[name] = (x, dt, lbl)
    return out


@pytest.mark.parametrize("model", ["nearest_point", "nearest_point_levels", "nearest_point_argmin"])
def test_l1_models_on_every_mask(cpu_sets, model):
    fn = getattr(PM, model)
    for name, (x, dt, lbl) in cpu_sets.items():
        for k in range(len(x)):
            if not (x[k] >= 0.9).any():
                continue  # (a frame without sources: test_parallel_model.py's edge frames)
            d, l = fn(x[k])
            assert np.array_equal(d, dt[k]) and np.array_equal(l, lbl[k]), (name, k)


def test_l2_models_on_every_mask(oracle, cpu_sets):
    for name, (x, _, _) in cpu_sets.items():
        for k in range(len(x)):
            src = E.sources(x[k])
            if not src.any():
                continue
            d2o, nearo = oracle.edt_l2((~src).astype(np.uint8))
            R = 3 if name == "whole3x4" else 7
            d2, near, decided = PM.l2_window(src, R)
            assert np.array_equal(decided, d2o <= R * R), (name, k)
            assert np.array_equal(d2[decided], d2o[decided]) and np.array_equal(near[decided], nearo[decided]), (name, k)
            d2, near, _ = PM.l2_envelope(src)
            assert np.array_equal(d2, d2o) and np.array_equal(near, nearo), (name, k)


@pytest.mark.parametrize("anchor", sorted(E.anchors("sky", *E.SHAPES["sky"])))
def test_sky_models_on_the_sky_sweeps(oracle, anchor):
    """k_sky's two statements on every mask of the sky sweeps: the rows above the first source row from rows r0 and r0 + 1 alone."""
    x, _ = E.sweep("sky", anchor)
    _, dt, lbl, _ = oracle.fill_batch(x)
    r0 = E.sky_first_rows("sky", anchor)
    assert r0.min() == E.SKY_TOP and (r0 >= E.SKY_MIN).all()
    for k in range(len(x)):
        jd, jl = dt[k].copy(), lbl[k].copy()
        jd[:r0[k]], jl[:r0[k]] = -1, -7  # the models must not look at the rows they are to produce
        for fn in (PM.sky_rows, PM.sky_rows_closed_form):
            d, l = fn(jd, jl)
            assert np.array_equal(d, dt[k]) and np.array_equal(l, lbl[k]), (anchor, k, fn.__name__)


# ---- discriminating power: a wrong order of the parent rule's taps -----------------------------------------------------------
# swapping entries i and i + 1 of PM.FWD / PM.BWD.  On the 600 random frames of test_parallel_model.py::test_small_random these eight
# change a label; the other six change none there (nor on the sets here: the taps they swap cannot tie as first choices)
MUTANTS_THAT_MATTER = [("FWD", 0), ("FWD", 1), ("FWD", 3), ("FWD", 4), ("FWD", 6), ("BWD", 0), ("BWD", 1), ("BWD", 3)]
ALL_MUTANTS = [(t, i) for t in ("FWD", "BWD") for i in range(7)]


@contextlib.contextmanager
def swapped(table, i):
    taps = getattr(PM, table)
    taps[i], taps[i + 1] = taps[i + 1], taps[i]
    try:
        yield
    finally:
        taps[i], taps[i + 1] = taps[i + 1], taps[i]


def mismatches(x, lbl, stop_at_first=False):
    """Frames of the set on which PM.nearest_point's labels differ from the oracle's."""
    n = 0
    for k in range(len(x)):
        if (x[k] >= 0.9).any() and not np.array_equal(PM.nearest_point(x[k])[1], lbl[k]):
            n += 1
            if stop_at_first:
                break
    return n


@pytest.mark.parametrize("table,i", MUTANTS_THAT_MATTER, ids=lambda v: str(v))
def test_every_tap_order_mutant_fails_on_the_cpu_sets(cpu_sets, table, i):
    """The model with two adjacent taps swapped differs from the oracle on some mask of the small sets (the table of counts:
    profiles/r13/exhaustive.txt, written by scripts/exhaustive_profile.py)."""
    fwd, bwd = list(PM.FWD), list(PM.BWD)
    with swapped(table, i):
        caught = any(mismatches(x, lbl, stop_at_first=True) for x, _, lbl in cpu_sets.values())
    assert PM.FWD == fwd and PM.BWD == bwd
    assert caught, "swapping %s[%d] and [%d] changes no label of the CPU sets" % (table, i, i + 1)

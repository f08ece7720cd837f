"""The inputs of test_gpu_l2_exact.py hold what that file relies on -- asserted here from the brute-force reference alone
(tests/l2_ref.py), without a GPU -- and the oracle agrees with that reference bit for bit, in index and distance.

l2 contract (include/dtfill.h): out_dt is sqrtf of the EXACT squared distance, out_index the nearest source under the canonical
tie-break (smallest raster index).  float32 stops telling neighbouring integers apart at 2^24, so an input probes the contract
there only if it has competing sources beyond d2 = 2^24: pixels whose best and second best d2 are different integers with the
same float32 (`collisions`), and pixels whose two best are equal (`ties`)."""
import numpy as np
import pytest

import l2_exact_cases as C
import l2_ref


def test_reference_forms_agree_and_match_exhaustive_search(oracle):
    """nearest() (chunked), nearest_whole_frame() (tiled, proven cuts) and the oracle's exhaustive C search on frames with
    ties everywhere (a lattice), a hole wider than the tiles' margin, one source, and none."""
    rng = np.random.default_rng(1)
    frames = [rng.random((50, 70)) < 0.05, rng.random((70, 150)) < 0.02, np.zeros((40, 90), bool), np.zeros((9, 7), bool), np.zeros((5, 6), bool)]
    frames[1][10:60, 30:120] = False
    frames[2][::10, ::10] = True
    frames[3][4, 2] = True
    for mask in frames:
        H, W = mask.shape
        src = np.argwhere(mask)
        a, b = l2_ref.nearest(src, l2_ref.all_pixels(H, W), W), l2_ref.nearest_whole_frame(src, H, W)
        for k in ("d2", "d2_2nd", "nbest", "near", "label"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert np.array_equal(l2_ref.bits(a.dt), l2_ref.bits(b.dt))
        if not len(src):
            assert (a.label == 0).all() and np.isinf(a.dt).all() and (a.near == -1).all()
            continue
        d2, near = oracle.brute_nearest((~mask).astype(np.uint8), 2)
        assert np.array_equal(a.frame("d2", H), d2) and np.array_equal(a.frame("near", H), near)
        two = np.sort((l2_ref.all_pixels(H, W)[:, None, :] - src[None]).__pow__(2).sum(2), 1)[:, :2]
        assert np.array_equal(two[:, 0], a.d2) and (len(src) < 2 or np.array_equal(two[:, 1], a.d2_2nd))


FAR = {"cluster500": (lambda o: C.cluster(500, o), "points"), "cluster1200": (lambda o: C.cluster(1200, o), 0),
       "edge": (C.edge, 16), "line": (C.line, "points")}


@pytest.mark.parametrize("orient", (C.WIDE, C.TALL))
@pytest.mark.parametrize("name", sorted(FAR))
def test_far_near_tie_inputs(name, orient):
    """Every far input: the shape is one the l2 mode takes (H + W - 2 < 8192), the source count sends it where
    test_gpu_l2_exact.py means it to go, every checked pixel of its first set lies at d2 >= 2^24, and among them at least 50
    collisions and 50 ties (the random inputs) or a runner-up at d2 + 1 everywhere, colliding on 40 % of the pixels at least
    (the line: c^2 and c^2 + 1 share a float32 for every even c from 4096 on, and for every c from 5793 on)."""
    case = FAR[name][0](orient)
    H, W = case.x.shape
    assert (H, W) == ((120, 8000) if name != "edge" else (40, 8100))[::1 if orient == C.WIDE else -1]
    assert H + W - 2 < 8192
    assert case.route == FAR[name][1], (len(case.src), case.route)
    r = case.refs[0]
    assert len(r.big) == len(r.d2) >= 10000 and r.d2.max() < 1 << 31
    assert np.unique(case.x[case.x > 0]).size == len(case.src), "every source a value of its own"
    print(name, orient, "pixels", len(r.d2), "collisions", len(r.collisions), "ties", len(r.ties), "max d2", int(r.d2.max()))
    if name == "line":
        assert np.array_equal(r.d2_2nd, r.d2 + 1) and 5 * len(r.collisions) >= 2 * len(r.d2)
    else:
        assert len(r.collisions) >= 50 and len(r.ties) >= 50
    if name == "edge":
        n = C.edge_sky_rows(orient)  # the rows that are redone whole: all of the wide frame, the empty part of the tall one
        assert n == H if orient == C.WIDE else H - C.EDGE_C - 20 <= n <= H - C.EDGE_C


def _small(name):
    case = getattr(C, name)()
    H, W = case.x.shape
    return case, H, W, case.refs[0]


@pytest.mark.parametrize("name", [f.__name__ for f in C.SMALL])
def test_bound_tie_inputs(name):
    """Every hand-built frame: its route, and each planted pixel a tie of exactly the planted sources at the planted distance,
    won by the source the case names."""
    case, H, W, r = _small(name)
    assert H + W - 2 < 8192 and case.route == (32 if name == "win15" else 16)
    want = {"ring17": {"left": (145 ** 2, 2), "right": (145 ** 2, 2)}, "ring33": {"left": (65 ** 2, 2), "right": (65 ** 2, 2)},
            "farpixel": {"P": (1024, 4), "A": (100, 6), "B": (101, 4)}, "rowcount": {}, "win15": {"A": (225, 6), "B": (226, 4)}}[name]
    assert sorted(want) == sorted(case.planted)
    for k, ((i, j), (wi, wj)) in case.planted.items():
        p = i * W + j
        assert (r.d2[p], r.d2_2nd[p], r.nbest[p]) == (want[k][0], want[k][0], want[k][1]), (k, r.d2[p], r.d2_2nd[p], r.nbest[p])
        assert r.near[p] == wi * W + wj and case.x[wi, wj] > 0.9, k
        assert r.label[p] == 1 + np.count_nonzero(l2_ref.source_mask(case.x).ravel()[:wi * W + wj])


@pytest.mark.parametrize("name", ("ring17", "ring33"))
def test_sky_ring_inputs(name):
    """Row 0 is a sky row (every pixel far), the winner's column distance is the row's smallest, the loser's the next, every
    other column's is larger: best == gmin^2 + (R + 1)^2 exactly, with the winner R + 1 columns away."""
    case, H, W, r = _small(name)
    g, gmin, off = {"ring17": (145, 144, 17), "ring33": (65, 56, 33)}[name]
    assert off in (l2 + 1 for l2 in (16, 32)) and W == 256 and l2_ref.row_threshold(W) == 32
    assert case.far_rows(10)[0] == W
    col = np.where(l2_ref.source_mask(case.x).any(0), l2_ref.source_mask(case.x).argmax(0), 1 << 20)  # row 0's column distances
    for (i, j), (wi, wj) in case.planted.values():
        assert i == 0 and col[j] == g and col[wj] == gmin == col.min() and abs(wj - j) == off
        assert r.d2[j] == gmin * gmin + off * off
    assert sorted(np.flatnonzero(col <= g)) == sorted(q for (_, j), (_, wj) in case.planted.values() for q in (j, wj))


def test_far_pixel_input():
    """P's row keeps P on the far list (fewer than 80 far pixels; no row of the frame has 80), P is the only far pixel as far
    as 32 from every source (its partner in the wave stops before the round base = 32), and its four nearest lie on the axes:
    the winner, straight above, is seen in that round alone.  A is the window's (d2 == 10^2), B is handed on (10^2 + 1)."""
    case, H, W, r = _small("farpixel")
    far = case.far_rows(10)
    assert l2_ref.row_threshold(W) == 80 and far.max() < 80 and 0 < far[64]
    d2 = r.frame("d2", H)
    other = d2 > 100
    other[64, 160] = False
    assert d2[64, 160] == 32 * 32 and d2[other].max() < 32 * 32
    assert d2[64, 420] == 100 and d2[64, 500] == 101


def test_row_count_input():
    """Rows with exactly 79, 80 and 81 far pixels by the reference, spread over the three 256-column tiles and over two waves in
    each; the frame has rows on either side of the threshold."""
    case, H, W, r = _small("rowcount")
    far = case.far_rows(10)
    assert l2_ref.row_threshold(W) == 80
    for row, n in C.ROWCOUNT_ROWS.items():
        assert far[row] == n
        cols = np.flatnonzero(r.frame("d2", H)[row] > 100)
        assert [((cols >= a) & (cols < b)).sum() > 0 for a, b in ((64, 128), (128, 192), (256, 320), (320, 384), (512, 576), (576, 640))] == [True] * 6
    assert (far >= 80).any() and ((far > 0) & (far < 80)).any()


def test_window_split_inputs():
    """k_l2win<15>'s frame: A at d2 == 15^2, B at 15^2 + 1, no row with as many far pixels as the row threshold."""
    case, H, W, r = _small("win15")
    assert case.far_rows(15).max() < l2_ref.row_threshold(W) == 152
    d2 = r.frame("d2", H)
    assert d2[64, 300] == 225 and d2[64, 700] == 226


def _assert_oracle_is_reference(oracle, x, r):
    depth, dt, idx, status = oracle.fill_batch(x[None], metric="l2")
    H, W = x.shape
    assert status[0] == 0
    assert np.array_equal(idx[0], r.frame("label", H))
    assert np.array_equal(l2_ref.bits(dt[0]), l2_ref.bits(r.frame("dt", H)))
    assert np.array_equal(depth[0], x.ravel()[r.frame("near", H)])


@pytest.mark.parametrize("name", [f.__name__ for f in C.SMALL])
def test_oracle_is_the_reference_on_the_bound_ties(oracle, name):
    case, H, W, r = _small(name)
    _assert_oracle_is_reference(oracle, case.x, r)


def test_oracle_is_the_reference_beyond_2_to_24(oracle):
    """A crop of the cluster layout, 24 x 8000 (192 000 pixels; 400 sources in the first 150 columns and half of column 149):
    every pixel against the reference, distances up to 6e7, the pixels beyond 2^24 with collisions and ties by the thousand."""
    case = C.cluster(400, C.WIDE, 24, 8000, front=0.5)
    H, W = case.x.shape
    r = l2_ref.nearest(case.src, l2_ref.all_pixels(H, W), W)
    print("big", len(r.big), "collisions", len(r.collisions), "ties", len(r.ties))
    assert len(r.big) > 70000 and len(r.collisions) >= 50 and len(r.ties) >= 50
    _assert_oracle_is_reference(oracle, case.x, r)

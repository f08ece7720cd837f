"""The LiDAR point projection (include/dtfill.h, dtfill_project_points) without a GPU: the numpy statement in tests/proj_ref.py
against hand-written cases; its ordered form against the reference's np.dot form (identical pixels, z within the bound that
rounding allows); the ABI's argument errors and workspace rule; the Python layer's argument errors; the point generator."""
import os

import numpy as np
import pytest

import proj_cases as C
import proj_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------
# the statement against values worked out by hand
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.cases()))
def test_hand_case_reference_mode(name):
    c = C.cases()[name]
    status, pixels = c["ref"]
    out, st, cnt = R.project_frame(c["pts"], c["K"], c["E"], C.H, C.W, R.REFERENCE)
    assert st == status
    assert _same_bits(out, C.expected_frame(pixels))  # +0.0 everywhere else, -inf and +inf by their bits
    assert list(cnt) == ([len(pixels), len(c["pts"]), 0, 0] if status in (0, R.NO_POINTS) else [0, 0, 0, 0])


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_hand_case_zbuffer_mode(name):
    c = C.cases()[name]
    status, pixels, (inside, behind, outside) = c["zbuf"]
    out, st, cnt = R.project_frame(c["pts"], c["K"], c["E"], C.H, C.W, R.ZBUFFER, 0.0)
    assert st == status
    assert _same_bits(out, C.expected_frame(pixels))
    assert list(cnt) == [len(pixels), inside, behind, outside]
    assert inside + behind + outside == len(c["pts"])


def test_half_to_even_columns():
    z, u, v = R.ordered_form(np.array([[0.5, 0, 1], [1.5, 0, 1], [2.5, 0, 1]], np.float32), np.eye(3), np.eye(4))
    assert list(u) == [0.0, 2.0, 2.0] and list(v) == [0.0, 0.0, 0.0] and list(z) == [1.0, 1.0, 1.0]


def test_min_z_is_compared_as_the_float_it_is_passed_as():
    pts = np.array([[0, 0, np.float32(0.1)], [1, 1, 1]], np.float32)  # z = (double)0.1f is not > (double)0.1f, but is > 0.1
    out, st, cnt = R.project_frame(pts, np.eye(3), np.eye(4), C.H, C.W, R.ZBUFFER, 0.1)
    assert list(cnt) == [1, 1, 1, 0] and out[1, 1] == 1.0 and out[0, 0] == 0.0


def test_batch_statement_counts_and_padding():
    cs = C.cases()
    names = sorted(cs)
    for stride in (3, 4):
        pts, counts, K, E = C.batch([cs[n] for n in names], stride)
        for mode, key in ((R.REFERENCE, "ref"), (R.ZBUFFER, "zbuf")):
            o32, o64, st, cnt = R.project(pts, counts, K, E, C.H, C.W, mode)
            for b, n in enumerate(names):
                assert st[b] == cs[n][key][0], n
                assert _same_bits(o64[b], C.expected_frame(cs[n][key][1])), n
            assert _same_bits(o32, o64.astype(np.float32))
    bad = counts.copy()
    bad[0], bad[1] = -1, pts.shape[1] + 1
    o32, o64, st, cnt = R.project(pts, bad, K, E, C.H, C.W, R.ZBUFFER)
    assert list(st[:2]) == [R.BAD_COUNT, R.BAD_COUNT] and not o64[:2].any() and not cnt[:2].any()
    # counts None: every record, the poison included -- NaN coordinates: an index-error frame / all behind
    o32, o64, st, cnt = R.project(pts, None, K, E, C.H, C.W, R.REFERENCE)
    assert (st == R.INDEX_ERROR).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the ordered form against the reference's np.dot form
# ---------------------------------------------------------------------------------------------------------------------------
def _back_projected(pkg):
    """The points velodyne_scan(3, seed=5)'s frames came from, as a LiDAR file would hold them: every valid pixel taken back
    through K^-1 and E^-1 in float64 and cast to float32.  [(pts float32 [n,3], K, E)] per frame."""
    x, K, E = pkg.synth.velodyne_scan(3, seed=5)
    out = []
    for b in range(3):
        v, u = np.nonzero(x[b] > np.float32(0.1))
        d = x[b][v, u].astype(np.float64)
        cam = np.linalg.inv(K[b]) @ (np.stack([u, v, np.ones_like(u)]).astype(np.float64) * d)
        p = (np.linalg.inv(E[b]) @ np.vstack([cam, np.ones((1, cam.shape[1]))]))[:3].T
        out.append((p.astype(np.float32), K[b], E[b]))
    return out


def _uniform_cloud(pkg):
    """200 000 seeded uniform points in the box in front of the sensor, through frame 0's calibration."""
    _, K, E = pkg.synth.velodyne_scan(3, seed=5)
    rng = np.random.default_rng(15)
    p = rng.uniform([1.0, -40.0, -3.0], [80.0, 40.0, 3.0], (200000, 3)).astype(np.float32)
    return [(p, K[0], E[0])]


@pytest.fixture(scope="module")
def clouds(pkg):
    import importlib

    importlib.import_module(pkg.__name__ + ".synth")
    return {"back_projected": _back_projected(pkg), "uniform": _uniform_cloud(pkg)}


U = 2.0 ** -53  # unit roundoff of IEEE double


def _gamma(n):
    return n * U / (1 - n * U)


def _z_bound(pts, K, E):
    """|z_a - z_b| for any two evaluations a, b of z = sum_j K[2][j] c_j, c_j = E[j][0] X + E[j][1] Y + E[j][2] Z + E[j][3], each
    sum taken in any order, with or without fused multiply-add.

    Stage 1: c_j is a sum of four products (the constant is a product with 1).  A term goes through at most one rounding of its
    product and three of additions, or fewer with an fma, so the computed cj satisfies |cj - c_j| <= gamma_4 * S1_j with
    S1_j = |E[j][0] X| + |E[j][1] Y| + |E[j][2] Z| + |E[j][3]|, and |cj| <= (1 + gamma_4) * S1_j  (Higham, Accuracy and Stability
    of Numerical Algorithms, section 3.1: the bound holds for every order of summation).
    Stage 2: the computed z is a sum of three products of the computed cj: |zc - sum_j K[2][j] cj| <= gamma_3 * sum_j |K[2][j]| |cj|,
    and the exact sum over the computed cj is within sum_j |K[2][j]| gamma_4 S1_j of the exact z.  Together, per evaluation,
      |zc - z| <= (gamma_3 (1 + gamma_4) + gamma_4) * T,   T = sum_j |K[2][j]| S1_j,
    and two evaluations lie within twice that of each other.  T itself is computed in floating point here: seven roundings of
    positive terms, covered by the factor (1 + gamma_8)."""
    K, E = np.abs(np.asarray(K, np.float64)), np.abs(np.asarray(E, np.float64))
    X, Y, Z = (np.abs(np.asarray(pts, np.float32)[:, k].astype(np.float64)) for k in range(3))
    S1 = [E[j, 0] * X + E[j, 1] * Y + E[j, 2] * Z + E[j, 3] for j in range(3)]
    T = K[2, 0] * S1[0] + K[2, 1] * S1[1] + K[2, 2] * S1[2]
    return 2 * (_gamma(3) * (1 + _gamma(4)) + _gamma(4)) * T * (1 + _gamma(8))


@pytest.mark.parametrize("which", ["back_projected", "uniform"])
def test_ordered_form_and_dot_form_pixels_are_identical(clouds, which):
    n = 0
    for pts, K, E in clouds[which]:
        z, u, v = R.ordered_form(pts, K, E)
        zd, ud, vd = R.dot_form(pts, K, E)
        assert np.isfinite(u).all() and np.isfinite(v).all()
        differ = (u != ud) | (v != vd)
        print("%s: %d of %d points differ in (u, v)" % (which, int(differ.sum()), len(pts)))
        assert not differ.any()
        n += len(pts)
    assert n == (103704 if which == "back_projected" else 200000)


@pytest.mark.parametrize("which", ["back_projected", "uniform"])
def test_ordered_form_and_dot_form_z_within_the_rounding_bound(clouds, which):
    for pts, K, E in clouds[which]:
        z, _, _ = R.ordered_form(pts, K, E)
        zd, _, _ = R.dot_form(pts, K, E)
        bound = _z_bound(pts, K, E)
        print("%s: %d of %d z differ, largest |dz| / bound = %.3g" % (which, int((z != zd).sum()), len(pts),
                                                                     float(np.max(np.abs(z - zd) / bound))))
        assert (bound > 0).all() and (bound < 1e-12).all()  # a bound in the last bits of a depth below 100 m, not a tolerance
        assert (np.abs(z - zd) <= bound).all()


def test_back_projected_points_land_on_their_pixels(clouds):
    """The clouds are what they claim to be: projected again they give velodyne_scan's frames back (z to float32's rounding
    of a float32 point; the pixel exactly, but for the few points the cast moved across a half)."""
    for pts, K, E in clouds["back_projected"]:
        out, st, cnt = R.project_frame(pts, K, E, 352, 1216, R.ZBUFFER)
        assert st == 0 and cnt[R.INSIDE] == len(pts) and cnt[R.PIXELS] > 0.99 * len(pts)


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI's argument errors (all checked before any HIP call) and the workspace rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu(pkg):
    L = pkg.load()
    wsb = L.dtfill_project_points_workspace_bytes
    ws = wsb(2, 1000, 352, 1216)
    assert ws % 256 == 0 and ws >= 2 * 352 * 1216 * 8
    assert ws == wsb(2, 5, 352, 1216)  # the keys are per pixel: N does not enter
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, -1), (65536, 1, 1, 1), (1, (1 << 31) // 3 + 1, 1, 1),
                (2, 8, 1 << 15, 1 << 15)):
        assert wsb(*bad) == 0, bad
    assert wsb(1, (1 << 31) // 3, 1, 1) > 0 and wsb(65535, 1, 1, 1) > 0

    def call(points=256, counts=512, B=2, N=1000, stride=4, H=352, W=1216, K=768, E=1024, mode=1, min_z=0.0, f32=1280, f64=1536,
             st=1792, cnt=2048, w=4096, nws=None):
        return L.dtfill_project_points(points, counts, B, N, stride, H, W, K, E, mode, min_z, f32, f64, st, cnt, w,
                                       ws if nws is None else nws, None)

    for kw in (dict(points=None), dict(K=None), dict(E=None), dict(w=None), dict(f32=None, f64=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(N=0), dict(H=0), dict(W=-3), dict(B=65536, N=1, H=1, W=1), dict(stride=2), dict(stride=5),
               dict(stride=0), dict(mode=2), dict(mode=-1), dict(min_z=-1.0), dict(min_z=float("inf")), dict(min_z=float("nan")),
               dict(B=1, N=1 << 29, stride=4, H=1, W=1),  # 2^31 floats of records
               dict(B=1, N=(1 << 31) // 3 + 1, stride=3, H=1, W=1),
               dict(B=2, N=8, H=1 << 15, W=1 << 15, nws=1 << 40)):  # 2^31 pixels
        assert call(**kw) == -2, kw
    assert call(mode=0, min_z=-1.0, nws=0) == -3  # REFERENCE ignores min_z: the next check answers
    assert call(nws=ws - 1) == -3
    assert call(w=4100) == -3  # not 256-byte aligned
    # the largest record counts just inside the limit are no shape error (too small a workspace is the next check)
    assert call(B=1, N=(1 << 29) - 1, stride=4, H=1, W=1, nws=0) == -3
    assert call(B=1, N=(1 << 31) // 3, stride=3, H=1, W=1, nws=0) == -3
    lib = pkg._lib
    assert (lib.PROJ_REFERENCE, lib.PROJ_ZBUFFER) == (R.REFERENCE, R.ZBUFFER)
    assert (lib.PROJ_NO_POINTS, lib.PROJ_INDEX_ERROR, lib.PROJ_BAD_COUNT) == (R.NO_POINTS, R.INDEX_ERROR, R.BAD_COUNT)


def test_constants_match_the_header(pkg):
    import re

    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define DTFILL_PROJ_(\w+)[ \t]+(\d+)\b", src, flags=re.M)}
    lib = pkg._lib
    assert len(defines) == 10
    for n in ("REFERENCE", "ZBUFFER", "NO_POINTS", "INDEX_ERROR", "BAD_COUNT"):
        assert getattr(lib, "PROJ_" + n) == defines[n], n
    assert len(lib.PROJ_COLUMNS) == defines["N"]
    assert [defines[c.upper()] for c in lib.PROJ_COLUMNS] == list(range(defines["N"]))
    assert (R.PIXELS, R.INSIDE, R.BEHIND, R.OUTSIDE) == tuple(range(4))


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer's argument errors, and the generator
# ---------------------------------------------------------------------------------------------------------------------------
def test_map_points_on_image_errors_without_gpu(pkg):
    K, E = np.eye(3), np.eye(4)
    for bad in (np.zeros((4, 4)), np.zeros((3,)), np.zeros((2, 3, 3)), np.zeros((5, 2))):  # the reference unpacks [n, 3] and hstacks a one
        with pytest.raises(ValueError, match="left_points"):
            pkg.map_points_on_image(bad, K, E)
    with pytest.raises(TypeError, match="float32"):
        pkg.map_points_on_image(np.array([[0.1, 0.2, 0.3]]), K, E)  # float64 that float32 does not hold
    with pytest.raises(TypeError):
        pkg.map_points_on_image(np.array([["a", "b", "c"]]), K, E)


def test_project_points_errors_without_gpu(pkg):
    K, E = np.eye(3), np.eye(4)
    with pytest.raises(ValueError, match="at least one"):
        pkg.project_points([], K, E)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4,), np.float32), np.zeros((2, 4, 3), np.float32)):
        with pytest.raises(ValueError, match="cloud 1"):
            pkg.project_points([np.zeros((2, 3), np.float32), bad], K, E)
    with pytest.raises(TypeError, match="float32"):
        pkg.project_points([np.array([[0.1, 0.2, 0.3, 0.0]])], K, E)


def test_velodyne_points_generator(pkg):
    import importlib

    synth = importlib.import_module(pkg.__name__ + ".synth")
    clouds, K, E = synth.velodyne_points(2, seed=3)
    again, K2, E2 = synth.velodyne_points(2, seed=3)
    assert K.shape == (2, 3, 3) and E.shape == (2, 4, 4) and np.array_equal(K, K2) and np.array_equal(E, E2)
    for c, a, Kb, Eb in zip(clouds, again, K, E):
        assert c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 4 and 80000 < c.shape[0] < 200000
        assert np.array_equal(c, a) and np.isfinite(c).all()
        out, st, cnt = R.project_frame(c, Kb, Eb, 352, 1216, R.ZBUFFER)
        # a whole sweep: most of it is behind or beside the camera, the rest fills a KITTI-like frame
        assert st == 0 and cnt[R.PIXELS] > 10000 and cnt[R.BEHIND] + cnt[R.OUTSIDE] > 0.7 * len(c)
        assert R.project_frame(c, Kb, Eb, 352, 1216, R.REFERENCE)[1] == R.INDEX_ERROR  # the reference's function would raise
    assert clouds[0].shape != clouds[1].shape  # ragged
    # velodyne_scan is untouched by its sibling: the frame count the projection tests rely on
    x, _, _ = synth.velodyne_scan(3, seed=5)
    assert int((x > 0.1).sum()) == 103704

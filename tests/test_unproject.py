"""The back-projection (include/dtfill.h, dtfill_unproject, dtfill_unproject_backward) without a GPU: the numpy statement in
tests/unproj_ref.py against hand-worked cases, against lines_ref and proj_ref, and against torch's float64 autograd; the ABI's
return codes; the Python layer's argument checks."""
import importlib
import math

import numpy as np
import pytest

import lines_ref
import proj_ref
import unproj_ref as R

F = np.float32
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53  # unit roundoffs


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


@pytest.fixture(scope="module")
def scans(synth):
    return synth.velodyne_scan(2, seed=3)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------------
# hand cases: 5 x 7 frames under R.exact_calibration(): K^-1 [u v 1]^T = [(u - 3.5) / 512, (v - 2.25) / 256, 1] and E^-1 maps a
# camera point c to (c_z + 0.5, 0.25 - c_x, -0.125 - c_y), so pixel (v, u) at depth d is the point
#   (d + 0.5,  0.25 - (u - 3.5) d / 512,  -0.125 - (v - 2.25) d / 256),
# every term a dyadic rational that float64 and, for these depths, float32 hold exactly.
# ---------------------------------------------------------------------------------------------------------------------------
def _hand(u, v, d):
    return [d + 0.5, 0.25 - (u - 3.5) * d / 512, -0.125 - (v - 2.25) * d / 256]


def _frame(**pixels):
    x = np.zeros((5, 7), F)
    for k, d in pixels.items():
        x[int(k[1]), int(k[2])] = d
    return x


def test_hand_one_pixel():
    K, E = R.exact_calibration()
    r = R.forward(_frame(p23=8.0), K, E)
    assert r["counts"].tolist() == [[1, 1]] and r["status"].tolist() == [0] and r["pixel"][0].tolist() == [2 * 7 + 3]
    assert r["points"][0].tolist() == [[8.5, 0.2578125, -0.1171875]] == [_hand(3, 2, 8.0)]
    assert r["pitch"][0][0] == math.asin(-0.1171875 / math.sqrt(8.5 * 8.5 + 0.2578125 ** 2 + 0.1171875 ** 2))


def test_hand_last_pixel_only_and_payload():
    K, E = R.exact_calibration()
    pay = np.arange(35, dtype=F).reshape(5, 7) + F(0.5)
    r = R.forward(_frame(p46=16.0), K, E, payload=pay, stride=4)
    assert r["pixel"][0].tolist() == [34] and r["counts"].tolist() == [[1, 1]]
    assert r["points"][0].tolist() == [_hand(6, 4, 16.0) + [34.5]] == [[16.5, 0.171875, -0.234375, 34.5]]
    r3 = R.forward(_frame(p46=16.0), K, E, stride=4)  # no payload: +0.0f
    assert _bits(r3["points"][0][:, 3]).tolist() == [0]


def test_hand_inf_and_nan_depths():
    K, E = R.exact_calibration()
    r = R.forward(_frame(p11=np.inf, p12=np.nan, p30=2.0), K, E)
    # NaN is never valid; +inf is, and its point is NaN in every coordinate (E^-1 holds zeros: 0 * inf)
    assert r["pixel"][0].tolist() == [8, 21] and r["status"].tolist() == [0]
    assert np.isnan(r["points"][0][0]).all() and np.isnan(r["pitch"][0][0])
    assert r["points"][0][1].tolist() == _hand(0, 3, 2.0)
    rk = R.forward(_frame(p11=np.inf, p12=np.nan, p30=2.0), K, E, keep_every=2)  # the NaN pitch makes the range NaN
    assert rk["status"].tolist() == [R.BAD_INTERVAL] and rk["counts"].tolist() == [[0, 0]]


def test_hand_negative_threshold():
    K, E = R.exact_calibration()
    x = _frame(p00=-0.5, p01=-1.0, p02=-2.0, p03=np.nan, p46=4.0)
    r = R.forward(x, K, E, val_thr=-1.0)  # zeros are points now (at E^-1's origin), -1.0 itself and below are not
    want = [p for p in range(35) if p not in (1, 2, 3)]
    assert r["pixel"][0].tolist() == want and r["counts"].tolist() == [[32, 32]]
    assert r["points"][0][0].tolist() == _hand(0, 0, -0.5)
    assert r["points"][0][1].tolist() == [0.5, 0.25, -0.125] == _hand(4, 0, 0.0)
    assert r["points"][0][-1].tolist() == _hand(6, 4, 4.0)


def test_capacity_status_and_layout():
    K, E = R.exact_calibration(3)
    x = np.stack([_frame(), _frame(p23=8.0), np.full((5, 7), 3.0, F)])
    r = R.forward(x, K, E, N=20)
    assert r["status"].tolist() == [R.NO_POINTS, 0, R.OVERFLOW] and r["counts"].tolist() == [[0, 0], [1, 1], [20, 35]]
    assert r["pixel"][2].tolist() == list(range(20))
    p0 = np.full((3, 20, 3), 7.0, F)
    pts, _, pix = R.expected(r, p0, None, np.full((3, 20), -9, np.int32))
    assert (pts[0] == 7.0).all() and (pts[1, 1:] == 7.0).all() and pix[1].tolist() == [17] + [-9] * 19
    Ks = K.copy()
    Ks[1, 1] = 0.0
    Es = E.copy()
    Es[2, 2] = 0.0
    r = R.forward(x, Ks, Es)
    assert r["status"].tolist() == [R.NO_POINTS, R.SINGULAR, R.SINGULAR] and not r["counts"].any()
    r = R.forward(x, K, E, keep_every=2)
    assert r["status"][1] == R.BAD_INTERVAL and r["counts"][1].tolist() == [0, 0]  # one point: interval 0


# ---------------------------------------------------------------------------------------------------------------------------
# against lines_ref: the same pitch bits, and keep mode selects dtfill_line_subsample's pixels
# ---------------------------------------------------------------------------------------------------------------------------
def test_pitch_bits_equal_lines_ref(scans):
    x, K, E = scans
    r = R.forward(x, K, E)
    for b in range(2):
        want = lines_ref.pitch64(x[b], np.linalg.inv(K[b]), np.linalg.inv(E[b]))
        assert np.array_equal(_bits(r["pitch"][b]), _bits(want))
        assert np.array_equal(r["pixel"][b], np.flatnonzero(x[b].reshape(-1) > F(0.1)))


@pytest.mark.parametrize("keep_every", [1, 2, 4])
def test_keep_mode_selects_line_subsample_pixels(scans, keep_every):
    x, K, E = scans
    out, st, _ = lines_ref.ref64(x, K, E, 64, keep_every)
    r = R.forward(x, K, E, keep_every=keep_every)
    assert not st.any() and not r["status"].any()
    for b in range(2):
        assert np.array_equal(r["pixel"][b], np.flatnonzero(out[b].reshape(-1)))
        assert r["counts"][b].tolist() == [np.count_nonzero(out[b])] * 2


def test_points_agree_with_the_reference_precision(scans):
    """lines_ref.ref32_like_reference runs the scripts' float32 chain (float32 calibration, inverses, back-projection) and
    re-projects its points in float64; with every point kept its PNG is the frame's own depth * 256, truncated.  The same
    re-projection of unproj_ref's float32 points must give that PNG.  The bound: a float32 point carries at most 1 rounding
    (EPS32 relative per coordinate) here and about 10 in the float32 chain; re-projected, z moves by at most about
    12 EPS32 (|p|_1 + |t|_1) <= 12 * 2^-24 * 2 * 85 m < 1.3e-4 m = 0.032 PNG counts, so after truncation the two differ by at
    most one count, and only where depth * 256 lies within that distance of an integer."""
    x, K, E = scans
    K32, E32 = K.astype(F).astype(np.float64), E.astype(F).astype(np.float64)
    for b in range(2):
        png, kept = lines_ref.ref32_like_reference(x[b], K[b], E[b], 64, 1)
        assert np.array_equal(kept, x[b] > F(0.1))
        r = R.forward(x[b], K32[b], E32[b])
        z, st, _ = proj_ref.project_frame(r["points"][0], K32[b], E32[b], 352, 1216, proj_ref.ZBUFFER)
        mine = (z * 256.0).astype(np.uint16)
        assert np.array_equal(mine != 0, png != 0)
        diff = np.abs(mine.astype(np.int64) - png.astype(np.int64))
        assert diff.max() <= 1
        frac = np.abs(z * 256.0 - np.round(z * 256.0))
        assert (frac[diff == 1] < 0.07).all()  # two chains, 0.032 counts each


# ---------------------------------------------------------------------------------------------------------------------------
# the round trip on the references alone: un-project, project back (z-buffer)
# ---------------------------------------------------------------------------------------------------------------------------
def _round_trip(x, K, E):
    H, W = x.shape
    r = R.forward(x, K, E)
    z, st, cnt = proj_ref.project_frame(r["points"][0], K, E, H, W, proj_ref.ZBUFFER)
    valid = x > F(0.1)
    assert st == 0 and np.array_equal(z != 0, valid) and cnt[proj_ref.PIXELS] == valid.sum() == cnt[proj_ref.INSIDE]
    rel = np.abs(z[valid] - x[valid].astype(np.float64)) / x[valid]
    return rel.max() / EPS32


def test_round_trip_scans(scans):
    x, K, E = scans
    for b in range(2):
        assert _round_trip(x[b], K[b], E[b]) <= 2.0


def test_round_trip_dense_frame(scans):
    _, K, E = scans
    x = np.random.default_rng(5).uniform(1.0, 80.0, (352, 1216)).astype(F)
    assert _round_trip(x, K[0], E[0]) <= 2.0


# ---------------------------------------------------------------------------------------------------------------------------
# the backward against torch's float64 autograd of the forward expression
# ---------------------------------------------------------------------------------------------------------------------------
def test_backward_matches_float64_autograd(scans):
    """The contract's backward computes, per record, k (2 products, 2 sums per row), j (3 products, 2 sums per row) and the
    final 3 products and 2 sums: every path from an input to the result passes at most 4 + 5 + 5 = 14 roundings; autograd's
    chain through the forward expression passes no more.  So both lie within gamma = 14 EPS64 / (1 - 14 EPS64) of the exact
    value relative to the sum of absolute terms A = sum_r |g_r| sum_c |Einv[r][c]| sum_m |Kinv[c][m]| |(u, v, 1)_m|, and within
    2 gamma A of each other.  Compared before the final float32 rounding."""
    import torch

    x, K, E = scans
    H, W = x.shape[1:]
    rng = np.random.default_rng(7)
    for b in range(2):
        r = R.forward(x[b], K[b], E[b])
        n = int(r["counts"][0, 0])
        pix = r["pixel"][0]
        g = rng.standard_normal((1, n, 3)).astype(F)
        got, _, st = R.backward(g, pix[None], r["counts"], K[b], E[b], H, W, rounded=False)
        assert st.tolist() == [0]
        Ki, Ei = torch.from_numpy(np.linalg.inv(K[b])), torch.from_numpy(np.linalg.inv(E[b]))
        d = torch.from_numpy(x[b].reshape(-1)[pix].astype(np.float64)).requires_grad_(True)
        uv1 = torch.stack([torch.from_numpy((pix % W).astype(np.float64)), torch.from_numpy((pix // W).astype(np.float64)),
                           torch.ones(n, dtype=torch.float64)])
        cam = (Ki @ uv1) * d
        p = (Ei @ torch.cat([cam, torch.ones(1, n, dtype=torch.float64)]))[:3]
        (p * torch.from_numpy(g[0, :n].astype(np.float64).T)).sum().backward()
        A = np.einsum("nr,rn->n", np.abs(g[0].astype(np.float64)),
                      np.abs(Ei.numpy()[:3, :3]) @ (np.abs(Ki.numpy()) @ np.abs(uv1.numpy())))
        gamma = 14 * EPS64 / (1 - 14 * EPS64)
        err = np.abs(got.reshape(-1)[pix] - d.grad.numpy())
        assert (err <= 2 * gamma * A).all(), (err / A).max() / EPS64
        off = np.ones(H * W, bool)
        off[pix] = False
        assert not _bits(got.reshape(-1)[off]).any()
        # the Python-float statement holds the same bits as the numpy one
        Kl, El = np.linalg.inv(K[b]).tolist(), np.linalg.inv(E[b]).tolist()
        for i in (0, n // 2, n - 1):
            assert R.backward_py(g[0, i], int(pix[i]), Kl, El, W) == got.reshape(-1)[pix[i]]


def test_backward_statuses():
    K, E = R.exact_calibration(4)
    g = np.ones((4, 6, 4), F)
    g[..., 3] = np.arange(24, dtype=F).reshape(4, 6)
    pixel = np.tile(np.array([0, 3, 4, 9, 34, 35], np.int32), (4, 1))
    pixel[1, 1:3] = 4, 3  # a swapped pair
    counts = np.array([[5, 5], [5, 5], [6, 6], [7, 9]], np.int32)
    gx, gp, st = R.backward(g, pixel, counts, K, E, 5, 7, want_payload=True)
    assert st.tolist() == [0, R.BAD_PIXEL, R.BAD_PIXEL, R.BAD_COUNT]
    assert not _bits(gx[1:]).any() and not _bits(gp[1:]).any()
    assert np.flatnonzero(gx[0]).tolist() == [0, 3, 4, 9, 34] and gp[0].reshape(-1)[[0, 3, 4, 9, 34]].tolist() == [0, 1, 2, 3, 4]
    # d point / d depth of pixel (v, u) = (1, -(u - 3.5) / 512, -(v - 2.25) / 256); with g = (1, 1, 1):
    assert gx[0, 0, 3] == 1.0 + 0.5 / 512 + 2.25 / 256 and gx[0, 4, 6] == 1.0 - 2.5 / 512 - 1.75 / 256


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI's return codes (all checked before any HIP call) and the workspace rules
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_return_codes_without_gpu(pkg):
    L = pkg.load()
    wsb = L.dtfill_unproject_workspace_bytes
    ws = wsb(2, 352, 1216)
    assert ws % 256 == 0 and ws > 0
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (65536, 1, 1), (2, 1 << 15, 1 << 15)):
        assert wsb(*bad) == 0, bad
    assert wsb(65535, 1, 1) > 0

    def call(x=256, payload=512, B=2, H=352, W=1216, thr=0.1, K=768, E=1024, n_bins=64, keep=0, N=1000, stride=4, points=1280,
             pitch=1536, pixel=1792, counts=2048, st=2304, w=4096, nws=None):
        return L.dtfill_unproject(x, payload, B, H, W, thr, K, E, n_bins, keep, N, stride, points, pitch, pixel, counts, st, w,
                                  ws if nws is None else nws, None)

    for kw in (dict(x=None), dict(K=None), dict(E=None), dict(points=None), dict(counts=None), dict(w=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(H=0), dict(W=-3), dict(N=0), dict(N=-1), dict(B=65536, H=1, W=1), dict(stride=2), dict(stride=5),
               dict(B=2, H=1 << 15, W=1 << 15, nws=1 << 40),  # 2^31 pixels
               dict(B=1, H=1, W=1, N=1 << 29, stride=4), dict(B=1, H=1, W=1, N=(1 << 31) // 3 + 1, stride=3),  # 2^31 floats
               dict(keep=-1), dict(keep=1, n_bins=0), dict(keep=4, n_bins=-2), dict(thr=float("nan"))):
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3 and call(w=4100) == -3 and call(nws=0) == -3
    # legal: n_bins is ignored without keep mode; the nullable pointers; an infinite threshold; the largest record counts
    for kw in (dict(n_bins=0), dict(payload=None, pitch=None, pixel=None, st=None), dict(thr=float("inf")), dict(thr=-1.0),
               dict(B=1, H=1, W=1, N=(1 << 29) - 1, stride=4), dict(B=1, H=1, W=1, N=(1 << 31) // 3, stride=3)):
        assert call(nws=0, **kw) == -3, kw  # past the shape checks: the workspace is the next one


def test_backward_return_codes_without_gpu(pkg):
    L = pkg.load()
    wsb = L.dtfill_unproject_backward_workspace_bytes
    ws = wsb(2, 352, 1216)
    assert ws % 256 == 0 and ws > 0
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (65536, 1, 1), (2, 1 << 15, 1 << 15)):
        assert wsb(*bad) == 0, bad

    def call(g=256, pixel=512, counts=768, B=2, N=1000, stride=4, H=352, W=1216, K=1024, E=1280, gx=1536, gp=1792, st=2048, w=4096,
             nws=None):
        return L.dtfill_unproject_backward(g, pixel, counts, B, N, stride, H, W, K, E, gx, gp, st, w, ws if nws is None else nws,
                                           None)

    for kw in (dict(g=None), dict(pixel=None), dict(counts=None), dict(K=None), dict(E=None), dict(gx=None), dict(w=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(N=0), dict(H=0), dict(W=-3), dict(B=65536, N=1, H=1, W=1), dict(stride=2), dict(stride=5),
               dict(B=2, H=1 << 15, W=1 << 15, nws=1 << 40), dict(B=1, H=1, W=1, N=1 << 29, stride=4),
               dict(B=1, H=1, W=1, N=(1 << 31) // 3 + 1, stride=3)):
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3 and call(w=4100) == -3
    assert call(gp=None, st=None, nws=0) == -3


def test_constants_match_the_header(pkg):
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtfill.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define DTFILL_UNPROJ_(\w+)[ \t]+(\d+)\b", src, flags=re.M)}
    assert len(defines) == 8
    for n, v in defines.items():
        assert getattr(pkg._lib, "UNPROJ_" + n) == v == getattr(R, n), n
    lines = {k: int(v) for k, v in re.findall(r"^#define DTFILL_LINES_(\w+)[ \t]+(\d+)\b", src, flags=re.M)}
    assert all(defines[k] == v for k, v in lines.items()) and len(lines) == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer's argument checks that come before any device work
# ---------------------------------------------------------------------------------------------------------------------------
def test_numpy_layer_argument_errors_without_gpu(pkg):
    K, E = R.exact_calibration()
    x = _frame(p23=8.0)
    for bad in (np.zeros((2, 3, 4, 5), F), np.zeros((7,), F), np.zeros((0, 4), F)):
        with pytest.raises(ValueError, match="unproject_frames expects"):
            pkg.unproject_frames(bad, K[0], E[0])
    with pytest.raises(ValueError, match="keep_ratio"):
        pkg.unproject_frames(x, K[0], E[0], keep_ratio=0.3)
    with pytest.raises(TypeError, match="float32"):
        pkg.unproject_frames(np.full((5, 7), 0.1), K[0], E[0])  # float64 that float32 does not hold
    with pytest.raises(TypeError, match="payload"):
        pkg.unproject_frames(x, K[0], E[0], payload=np.zeros((5, 7)))
    with pytest.raises(ValueError, match="payload"):
        pkg.unproject_frames(x, K[0], E[0], payload=np.zeros((5, 6), F))
    with pytest.raises(ValueError, match="get_all_points"):
        pkg.get_all_points(np.zeros((2, 5, 7), F), K[0], E[0], None)
    assert pkg.device.unproject_device is pkg.unproject_device

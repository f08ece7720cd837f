"""Scan-line subsampling without a GPU: the float64 statement of the contract on simulated Velodyne frames, the reference's
float32 precision against it, the simulated scan itself, and the C ABI's argument checks (include/dtfill.h)."""
import importlib
import os

import numpy as np
import pytest

import lines_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


@pytest.fixture(scope="module")
def scan(synth):
    return synth.velodyne_scan(3, seed=7)


def test_ref64_keep_sets_are_nested(scan):
    x, K, E = scan
    valid = x > np.float32(0.1)
    kept = {}
    for ke in (1, 2, 4):
        out, status, q = R.ref64(x, K, E, 64, ke)
        assert not status.any()
        kept[ke] = out > 0
        assert np.array_equal(out[kept[ke]].view(np.uint32), x[kept[ke]].view(np.uint32))  # input values, bit for bit
        assert not (out[~kept[ke]].view(np.uint32)).any()  # +0.0 elsewhere
    assert np.array_equal(kept[1], valid)
    assert not (kept[4] & ~kept[2]).any() and not (kept[2] & ~kept[1]).any()
    assert 0.15 < kept[4].sum() / valid.sum() < 0.4 and 0.35 < kept[2].sum() / valid.sum() < 0.65


def test_ref64_labels_and_extremes(scan):
    x, K, E = scan
    _, _, q = R.ref64(x, K, E, 64, 4)
    out, _, _ = R.ref64(x, K, E, 64, 4)
    for b in range(x.shape[0]):
        qb = q[b][x[b] > np.float32(0.1)]
        lab = np.ceil(qb)
        assert lab.min() == 0 and lab.max() == 64 and ((lab >= 0) & (lab <= 64)).all()
        # the minimum and the maximum point are kept (labels 0 and 64, multiples of 4)
        Ki, Ei = np.linalg.inv(K[b]), np.linalg.inv(E[b])
        pitch = R.pitch64(x[b], Ki, Ei)
        vv, uu = np.nonzero(x[b] > np.float32(0.1))
        for k in (np.argmin(pitch), np.argmax(pitch)):
            assert out[b, vv[k], uu[k]] == x[b, vv[k], uu[k]]
        assert len(np.unique(lab)) >= 40  # the rings spread over the bins


def test_ref64_reprojection_is_the_identity(scan):
    """The reference re-projects the kept points through the same K and E: in float64 every point lands on its own pixel
    at its own depth, which is why the kernels do not scatter."""
    x, K, E = scan
    for b in range(x.shape[0]):
        Ki, Ei = np.linalg.inv(K[b]), np.linalg.inv(E[b])
        v, u = np.nonzero(x[b] > np.float32(0.1))
        d = x[b][v, u].astype(np.float64)
        cam = (Ki @ np.stack([u, v, np.ones_like(u)]).astype(np.float64)) * d
        p = (Ei @ np.vstack([cam, np.ones_like(d)]))[:3]
        img = K[b] @ (E[b] @ np.vstack([p, np.ones_like(d)]))[:3]
        assert np.array_equal(np.round(img[0] / img[2]).astype(np.int64), u)
        assert np.array_equal(np.round(img[1] / img[2]).astype(np.int64), v)
        assert np.allclose(img[2], d, rtol=1e-12, atol=0)


def test_ref64_degenerate_frames(scan):
    x, K, E = scan
    H, W = x.shape[1:]
    f = np.zeros((5, H, W), np.float32)
    Kb = np.broadcast_to(K[0], (5, 3, 3)).copy()
    f[1, 200, 300] = 12.5  # one point
    f[2] = x[0]
    f[2, 250, 400] = np.inf  # a +inf depth: NaN pitch, NaN interval
    f[3] = x[1]
    Kb[3, 2] = 0.0  # singular K
    f[4] = x[2]
    f[4][(f[4] > 0) & (f[4] < 0.2)] = 0.05
    f[4, 10, 10], f[4, 11, 11], f[4, 12, 12] = np.nan, -np.inf, 0.1  # not points
    out, status, _ = R.ref64(f, Kb, E[0], 64, 2)
    assert list(status) == [R.NO_POINTS, R.BAD_INTERVAL, R.BAD_INTERVAL, R.SINGULAR, 0]
    assert not out[:4].any()
    ref, _, _ = R.ref64(x[2], K[0], E[0], 64, 2)
    assert np.array_equal(out[4], ref[0])
    _, st, _ = R.ref64(np.zeros((1, H, W), np.float32), Kb[3], E[0])
    assert st[0] == R.NO_POINTS | R.SINGULAR


def test_reference_precision_against_ref64(scan):
    """The reference's float32 labels differ from the float64 contract only at bin edges, and rarely; its uint16 PNG holds
    k or k - 1 for a kept point of depth k / 256 (the float32 round trip lands just below the grid for many points)."""
    x, K, E = scan
    npts = ndiff = nkm1 = nboth = 0
    for ke in (2, 4):
        out, _, q = R.ref64(x, K, E, 64, ke)
        for b in range(x.shape[0]):
            png, kept32 = R.ref32_like_reference(x[b], K[b], E[b], 64, ke)
            kept64 = out[b] > 0
            diff = kept32 != kept64
            assert (np.abs(q[b] - np.round(q[b]))[diff] < 1e-4).all()
            npts += int((x[b] > np.float32(0.1)).sum())
            ndiff += int(diff.sum())
            both = kept32 & kept64
            k = (x[b][both].astype(np.float64) * 256).astype(np.int64)
            pv = png[both].astype(np.int64)
            assert np.isin(pv - k, (0, -1)).all()
            nkm1 += int((pv == k - 1).sum())
            nboth += int(both.sum())
    assert ndiff <= 1e-3 * npts
    assert nkm1 > 0.05 * nboth  # the divergence INTEGRATION.md documents is real on these frames


def test_velodyne_scan_is_deterministic_and_scan_like(synth):
    x, K, E = synth.velodyne_scan(4, seed=3)
    x2, K2, E2 = synth.velodyne_scan(4, seed=3)
    assert np.array_equal(x, x2) and np.array_equal(K, K2) and np.array_equal(E, E2)
    assert not np.array_equal(x, synth.velodyne_scan(4, seed=4)[0])
    assert x.dtype == np.float32 and x.shape == (4, 352, 1216) and K.shape == (4, 3, 3) and E.shape == (4, 4, 4)
    assert np.array_equal(x, np.round(x * 256) / 256)  # the k/256 grid
    assert x.max() <= 80.0 + 1e-3
    for b in range(4):
        valid = x[b] > 0
        assert 0.03 < valid.mean() < 0.15
        assert not valid[:100].any()  # sky rows above the top laser
        assert valid[250:].any(axis=1).all()  # rings reach the bottom rows
        assert 600 < K[b, 0, 0] < 850 and 0 < K[b, 0, 2] < 1216 and 0 < K[b, 1, 2] < 352
        assert np.allclose(E[b, :3, :3] @ E[b, :3, :3].T, np.eye(3), atol=1e-12) and np.abs(E[b, :3, 3]).max() < 0.4
    # per-frame calibration
    assert len({K[b, 0, 0] for b in range(4)}) == 4 and len({E[b, 0, 3] for b in range(4)}) == 4


def test_argument_errors_without_gpu(pkg):
    L = pkg.load()
    ws = L.dtfill_line_subsample_workspace_bytes(2, 8, 8)
    assert ws > 0 and L.dtfill_line_subsample_workspace_bytes(0, 8, 8) == 0
    assert L.dtfill_line_subsample_workspace_bytes(1, 0, 8) == 0 and L.dtfill_line_subsample_workspace_bytes(70000, 4, 4) == 0
    assert L.dtfill_line_subsample_workspace_bytes(1 << 11, 1 << 10, 1 << 10) == 0  # 2^31 pixels

    def call(x=256, B=2, H=8, W=8, K=256, E=256, nb=64, ke=2, out=512, st=768, w=1024, nws=None):
        return L.dtfill_line_subsample(x, B, H, W, K, E, nb, ke, out, st, w, ws if nws is None else nws, None)

    for kw in (dict(x=None), dict(K=None), dict(E=None), dict(out=None), dict(st=None), dict(w=None), dict(nb=0), dict(ke=0),
               dict(ke=-4)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(H=0), dict(W=-3), dict(B=70000, H=1, W=1), dict(B=1 << 11, H=1 << 10, W=1 << 10)):
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3
    assert call(w=1028) == -3  # not 256-byte aligned


def test_subsample_lidar_rejects_bad_keep_ratio(pkg):
    x = np.zeros((8, 8), np.float32)
    for kr in (0.3, 0.4, 3.0, 0.0, -0.5, float("nan"), "half"):
        with pytest.raises(ValueError):
            pkg.subsample_lidar(x, np.eye(3), np.eye(4), keep_ratio=kr)
    dev = importlib.import_module(pkg.__name__ + ".device")
    assert [dev.keep_every_of(k) for k in (1.0, 0.5, 0.25, 0.125)] == [1, 2, 4, 8]


def test_product_does_not_import_lines_ref():
    pkgdir = os.path.join(ROOT, "distancetransform-depthcompletion_amd")
    for dp, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp")):
                assert "lines_ref" not in open(os.path.join(dp, f)).read(), f

"""Scan-line subsampling on the device (dtfill_line_subsample, line_subsample_device, subsample_lidar) against the float64
statement of the contract in tests/lines_ref.py.

The device and ref64 compute the same float64 expressions; they may round K^-1, E^-1 and asin differently in the last
bit, so a pixel whose q = (pitch - pmin) / interval lies within 1e-9 of an integer (a bin edge) may be decided
differently.  Everywhere else the output must be bitwise equal, and such edge pixels must be rare."""
import importlib

import numpy as np
import pytest

import lines_ref as R
from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSETS = (0, 4, 12, 64, 132)


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


def _run(dev, x, K, E, keep_ratio, n_bins=64):
    import torch

    out, st = dev.line_subsample_device(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), K, E, keep_ratio, n_bins)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _assert_matches_ref64(out, status, x, K, E, n_bins, keep_every):
    """Bitwise equality with ref64 except on bin edges; returns the number of edge pixels inside the range."""
    ref, st, q = R.ref64(x, K, E, n_bins, keep_every)
    assert np.array_equal(status, st), (status, st)
    with np.errstate(invalid="ignore"):
        edge = np.abs(q - np.round(q)) < 1e-9  # NaN (not a point, or a frame with a status bit): False
        inner = edge & (q > 0) & (q < n_bins - 1e-9)  # not the frame's minimum (q = 0) nor its maximum
    bad = (out.view(np.uint32) != ref.view(np.uint32)) & ~edge
    assert not bad.any(), "%d pixels differ off the bin edges, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    npts = int(np.count_nonzero(x > np.float32(0.1)))
    assert inner.sum() <= max(1e-4 * npts, 0), (inner.sum(), npts)
    return int(inner.sum())


@pytest.mark.parametrize("n_bins", [64, 48])
def test_device_matches_ref64(dev, synth, n_bins):
    import torch

    x, K, E = synth.velodyne_scan(6, seed=11)
    for ke in (1, 2, 4, 8):
        # calibration as float32 tensors for half the calls: converted to float64 on the device, ref64 sees the same values
        Kc, Ec = (K, E) if ke % 4 else (torch.from_numpy(K.astype(np.float32)), torch.from_numpy(E.astype(np.float32)))
        out, st = _run(dev, x, Kc, Ec, 1.0 / ke, n_bins)
        Kr, Er = (K, E) if ke % 4 else (K.astype(np.float32).astype(np.float64), E.astype(np.float32).astype(np.float64))
        _assert_matches_ref64(out, st, x, Kr, Er, n_bins, ke)
        assert not st.any()
    # one calibration broadcast over the batch
    out, st = _run(dev, x, K[2], E[2], 0.5, n_bins)
    _assert_matches_ref64(out, st, x, K[2], E[2], n_bins, 2)


def _edge_batch(synth):
    x, K, E = synth.velodyne_scan(3, seed=5)
    H, W = x.shape[1:]
    f = np.zeros((9, H, W), np.float32)
    Kb = np.stack([K[b % 3] for b in range(9)])
    Eb = np.stack([E[b % 3] for b in range(9)])
    f[0] = x[0]  # ordinary
    # 1: empty
    f[2, 180, 640] = 23.25  # one point
    f[3, 4, 3] = f[3, 3, 4] = 7.5  # two points at one pitch: identity calibration, u^2 + v^2 equal
    Kb[3], Eb[3] = np.eye(3), np.eye(4)
    f[4] = x[1]
    f[4, 300, 700] = np.inf  # NaN pitch -> NaN range
    f[5] = x[1]
    f[5, 0, :6] = [np.nan, -np.inf, 0.1, 0.05, 1e-30, -3.0]  # not points; the frame stays ordinary
    f[6] = x[2]
    Kb[6, 1] = 0.0  # singular K
    f[7] = x[2]
    Eb[7, 1] = 0.0  # singular E
    f[8] = x[2]  # ordinary
    return f, Kb, Eb


def test_edge_frames(dev, synth):
    f, K, E = _edge_batch(synth)
    for ke in (2, 4):
        out, st = _run(dev, f, K, E, 1.0 / ke)
        assert list(st) == [0, R.NO_POINTS, R.BAD_INTERVAL, R.BAD_INTERVAL, R.BAD_INTERVAL, 0, R.SINGULAR, R.SINGULAR, 0]
        assert not out[[1, 2, 3, 4, 6, 7]].view(np.uint32).any()  # +0.0 everywhere
        _assert_matches_ref64(out, st, f, K, E, 64, ke)


def _crop(x, K, r0, r1, c0, c1):
    """Rows [r0, r1) and columns [c0, c1) of the frames, with the principal point moved to match (same geometry)."""
    Kc = K.copy()
    Kc[:, 0, 2] -= c0
    Kc[:, 1, 2] -= r0
    return np.ascontiguousarray(x[:, r0:r1, c0:c1]), Kc


def test_guarded_poisoned_buffers(pkg, dev, synth):
    import torch

    L = pkg._lib.load()
    x0, K0, E0 = synth.velodyne_scan(3, seed=9)
    cases = [(x0[:2], K0[:2], E0[:2])] + [_crop(x0, K0, 180, 241, 400, 531) + (E0,)]
    f, Ke, Ee = _edge_batch(synth)
    cases.append(_crop(f, Ke, 0, 352, 1, 1216) + (Ee,))  # W = 1215: the scalar path on every frame
    n = 0
    for x, K, E in cases:
        B, H, W = x.shape
        Kd = torch.from_numpy(np.ascontiguousarray(K)).to(DEV)
        Ed = torch.from_numpy(np.ascontiguousarray(E)).to(DEV)
        nws = L.dtfill_line_subsample_workspace_bytes(B, H, W)
        for ke in (2, 4):
            xo, oo, so = OFFSETS[n % 5], OFFSETS[(n + 1) % 5], OFFSETS[(n + 2) % 5]
            kind = KINDS[n % 3]  # zero / ones / random workspace
            n += 1
            xg = GuardedBuffer(x.nbytes, xo, DEV, H * W * 4)
            xg.view(torch.float32, x.shape).copy_(torch.from_numpy(x))
            og = GuardedBuffer(x.nbytes, oo, DEV, H * W * 4)
            sg = GuardedBuffer(4 * B, so, DEV)
            wg = GuardedBuffer(nws, 0, DEV)
            poison_output(og.view(torch.float32, x.shape), "depth")
            poison_output(sg.view(torch.int32, (B,)), "status")
            poison(wg.payload(), kind, seed=n)
            rc = L.dtfill_line_subsample(xg.ptr, B, H, W, Kd.data_ptr(), Ed.data_ptr(), 64, ke, og.ptr, sg.ptr, wg.ptr, nws,
                                         torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            for g, what in ((xg, "x"), (og, "out"), (sg, "status"), (wg, "workspace")):
                g.check(what)
            assert np.array_equal(xg.view(torch.float32, x.shape).cpu().numpy().view(np.uint32), x.view(np.uint32))
            out = og.view(torch.float32, x.shape).cpu().numpy()
            st = sg.view(torch.int32, (B,)).cpu().numpy()
            assert not is_poison(out, "depth").any() and not is_poison(st, "status").any()
            _assert_matches_ref64(out, st, x, K, E, 64, ke)


def test_batch_equals_frame_by_frame(dev, synth):
    x0, K0, E0 = synth.velodyne_scan(40, seed=13)
    for x, K, E in ((x0[:5], K0[:5], E0[:5]), _crop(x0, K0, 150, 257, 300, 1003) + (E0,)):  # 107 x 703, B = 40
        out, st = _run(dev, x, K, E, 0.25)
        for b in range(x.shape[0]):
            ob, sb = _run(dev, x[b:b + 1], K[b], E[b], 0.25)
            assert np.array_equal(ob[0].view(np.uint32), out[b].view(np.uint32)) and sb[0] == st[b], b
        _assert_matches_ref64(out, st, x, K, E, 64, 4)


def test_end_to_end_with_the_fill(pkg, dev, synth, oracle, gpu_op):
    import torch

    x, K, E = synth.velodyne_scan(4, seed=17)
    xd = torch.from_numpy(x).to(DEV)
    sub, st = dev.line_subsample_device(xd, K, E, 0.25)
    res = gpu_op.run(sub)
    torch.cuda.synchronize()
    ref, rst, _ = R.ref64(x, K, E, 64, 4)
    assert np.array_equal(sub.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(st.cpu().numpy(), rst)
    depth, dt, lbl, status = oracle.fill_batch(ref)
    assert np.array_equal(res["dt"].cpu().numpy(), dt)
    assert np.array_equal(res["index"].cpu().numpy(), lbl)
    assert np.array_equal(res["depth"].cpu().numpy(), depth)
    assert np.array_equal(res["status"].cpu().numpy() & 1, status)


def test_numpy_shim(pkg, dev, synth):
    x, K, E = synth.velodyne_scan(3, seed=19)
    out, _ = _run(dev, x, K, E, 0.5)
    got = pkg.subsample_lidar(x[1][..., None], K[1], E[1], keep_ratio=0.5)  # [H,W,1], as the scripts load it
    assert got.shape == x[1][..., None].shape and got.dtype == np.float32
    one, _ = _run(dev, x[1:2], K[1], E[1], 0.5)
    assert np.array_equal(got[..., 0].view(np.uint32), one[0].view(np.uint32))
    got = pkg.subsample_lidar(x, K, E, keep_ratio=0.5)  # [B,H,W]
    assert got.shape == x.shape and np.array_equal(got.view(np.uint32), out.view(np.uint32))
    got = pkg.subsample_lidar(x[0], K[0], E[0])  # [H,W], keep_ratio 0.25
    assert np.array_equal(got, _run(dev, x[:1], K[0], E[0], 0.25)[0][0])
    with pytest.raises(np.linalg.LinAlgError):
        pkg.subsample_lidar(x[0], np.zeros((3, 3)), E[0])
    with pytest.raises(ValueError):
        pkg.subsample_lidar(np.zeros_like(x[0]), K[0], E[0])
    one_point = np.zeros_like(x[0])
    one_point[200, 500] = 5.0
    assert not pkg.subsample_lidar(one_point, K[0], E[0]).any()  # NaN labels keep nothing
    with pytest.raises(ValueError):
        pkg.subsample_lidar(x[0], K[0], E[0], keep_ratio=0.3)

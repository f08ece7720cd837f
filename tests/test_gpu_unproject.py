"""The back-projection on the device (dtfill_unproject, dtfill_unproject_backward, unproject_device, autograd.unproject) against
the numpy statement of the contract in tests/unproj_ref.py, bit for bit (the pitch: to the arcsine's last bits, see
_pitch_close), through the ABI on guarded and poisoned buffers.

The calibrations are unproj_ref.exact_calibration's wherever a host reference is compared bit for bit: their inverses are
exact in any order of operations, so the device's Gauss-Jordan and np.linalg.inv hold the same bits (for a general calibration
the two may differ in the last bit, as tests/test_gpu_lines.py says of the pitch).  The cross-checks against the device's own
dtfill_line_subsample and dtfill_project_points run on synth.velodyne_scan's calibrations."""
import importlib

import numpy as np
import pytest

import concurrency
import proj_ref
import unproj_ref as R
from guarded import KINDS, GuardedBuffer, poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
TILE = 2048  # pixels per tile of the kernels (LS_TILE), 8 consecutive pixels a lane, 4 waves of 64 lanes
SEAM_SHAPES = ((2, 1024), (1, 2047), (3, 683))  # one tile exactly, one pixel short of it, one pixel past it (2049)
TWO_TILES_PLUS_ONE = (1, 2 * TILE + 1)
SHAPES = ((1, 1), (5, 7), (64, 65)) + SEAM_SHAPES + (TWO_TILES_PLUS_ONE,)
# poisons no call can produce here: NaNs with payloads of their own, a negative pixel, status bits beyond the defined ones
POISON = dict(points=0x7FA1B2C3, pitch=0x7FF1234512345678, pixel=-0x7F7F7F7F, counts=0x5A5A5A5A, status=0x5A5A5A5A,
              grad=0x7FB3C4D5)


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert not bad.size, "%s: %d of %d elements differ, first at %s" % (what, len(bad), a.size, bad[0])


def _pitch_close(got, want, what):
    """The pitch against numpy's: the same bits wherever want holds a NaN (the poison beyond n_b), elsewhere within 5 ulp.
    The argument of the arcsine, p.z / |p|, is IEEE arithmetic (products, sums, a square root, a division: correctly rounded
    on both sides) and so holds the same bits; the arcsine itself is each library's: glibc's, behind numpy, is within 1 ulp,
    the device library's within the 4 ulp OpenCL allows a double asin, so the two lie within 5 ulp of each other and a
    bitwise comparison cannot hold (measured here: 1 of 70 pitches of a 5 x 7 batch differed in the last bit).  That the
    stored pitch is the one the labels are decided with is checked bit-exactly through the selection, against
    dtfill_line_subsample."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    _same(got[nan], want[nan], what + " (not written)")
    err = np.abs(got[~nan] - want[~nan]) / np.spacing(np.abs(want[~nan]))
    assert not err.size or err.max() <= 5, "%s: %d of %d pitches beyond 5 ulp, worst %.1f" % (what, (err > 5).sum(), err.size, err.max())


def _filled(nbytes, dtype, shape, bits, offset=0):
    """A guarded buffer whose payload holds one bit pattern, and that pattern as a host array of the same shape."""
    import torch

    g = GuardedBuffer(nbytes, offset, DEV)
    host = np.full(shape, bits, {4: np.int64, 8: np.int64}[np.dtype(dtype).itemsize]).astype(
        {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]).view(dtype)
    g.payload().copy_(torch.from_numpy(host.reshape(-1).view(np.uint8)))
    return g, host


def _up(a, offset=0):
    import torch

    a = np.ascontiguousarray(a)
    g = GuardedBuffer(a.nbytes, offset, DEV)
    g.payload().copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    return g


def _down(g, dtype, shape):
    return g.payload().cpu().numpy().view(dtype).reshape(shape)


def run_forward(L, x, K, E, val_thr=0.1, payload=None, n_bins=64, keep_every=0, N=None, stride=3, pitch=True, pixel=True,
                status=True, x_off=0, p_off=0, kind="random", stream=None):
    """One dtfill_unproject through the ABI; every buffer guarded, outputs poisoned.  Returns the outputs as numpy (None for a
    NULL one) after checking the guards and that the inputs are unchanged."""
    import torch

    B, H, W = x.shape
    N = H * W if N is None else N
    Kd, Ed = _up(np.broadcast_to(K, (B, 3, 3))), _up(np.broadcast_to(E, (B, 4, 4)))
    xg = _up(x, x_off)
    pg = None if payload is None else _up(payload, x_off)
    og, _ = _filled(B * N * stride * 4, F, (B, N, stride), POISON["points"], p_off)
    tg = _filled(B * N * 8, np.float64, (B, N), POISON["pitch"])[0] if pitch else None
    ig = _filled(B * N * 4, np.int32, (B, N), POISON["pixel"])[0] if pixel else None
    cg = _filled(B * 8, np.int32, (B, 2), POISON["counts"])[0]
    sg = _filled(B * 4, np.int32, (B,), POISON["status"])[0] if status else None
    nws = L.dtfill_unproject_workspace_bytes(B, H, W)
    wg = GuardedBuffer(nws, 0, DEV)
    poison(wg.payload(), kind, seed=B * H + W)
    ptr = lambda g: None if g is None else g.ptr
    s = torch.cuda.current_stream() if stream is None else stream
    rc = L.dtfill_unproject(xg.ptr, ptr(pg), B, H, W, val_thr, Kd.ptr, Ed.ptr, n_bins, keep_every, N, stride, og.ptr, ptr(tg),
                            ptr(ig), cg.ptr, ptr(sg), wg.ptr, nws, s.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in ((xg, "x"), (pg, "payload"), (og, "points"), (tg, "pitch"), (ig, "pixel"), (cg, "counts"), (sg, "status"),
                    (wg, "workspace"), (Kd, "K"), (Ed, "E")):
        if g is not None:
            g.check(what)
    _same(_down(xg, F, x.shape), x, "x after the call")
    if pg is not None:
        _same(_down(pg, F, x.shape), payload, "payload after the call")
    return dict(points=_down(og, F, (B, N, stride)), pitch=_down(tg, np.float64, (B, N)) if pitch else None,
                pixel=_down(ig, np.int32, (B, N)) if pixel else None, counts=_down(cg, np.int32, (B, 2)),
                status=_down(sg, np.int32, (B,)) if status else None)


def check_forward(L, x, K, E, what="", **kw):
    """run_forward against unproj_ref.forward, bit for bit, the poison beyond n_b included."""
    got = run_forward(L, x, K, E, **kw)
    B, H, W = x.shape
    N = kw.get("N") or H * W
    stride = kw.get("stride", 3)
    ref = R.forward(x, K, E, kw.get("val_thr", 0.1), kw.get("payload"), kw.get("n_bins", 64), kw.get("keep_every", 0), N, stride)
    assert np.array_equal(got["counts"], ref["counts"]), (what, got["counts"][:8], ref["counts"][:8])
    if got["status"] is not None:
        assert np.array_equal(got["status"], ref["status"]), (what, got["status"][:8], ref["status"][:8])
    poisoned = lambda name, dtype, shape: np.full(shape, POISON[name], np.int64).astype(
        {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]).view(dtype)
    want = R.expected(ref, poisoned("points", F, (B, N, stride)),
                      poisoned("pitch", np.float64, (B, N)) if got["pitch"] is not None else None,
                      poisoned("pixel", np.int32, (B, N)) if got["pixel"] is not None else None)
    if got["pixel"] is not None:
        _same(got["pixel"], want[2], what + " pixel")
    _same(got["points"], want[0], what + " points")
    if got["pitch"] is not None:
        _pitch_close(got["pitch"], want[1], what + " pitch")
    return got, ref


def _frames(B, H, W, seed, p=0.3):
    rng = np.random.default_rng(seed)
    d = (np.round(rng.uniform(1.0, 80.0, (B, H, W)) * 256.0) / 256.0).astype(F)
    return np.where(rng.random((B, H, W)) < p, d, F(0)).astype(F)


def _payload(shape, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(F)  # any bits


# ---------------------------------------------------------------------------------------------------------------------------
# shapes, options, alignment
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
def test_shapes_and_options(pkg, dev, hw):
    L = pkg._lib.load()
    H, W = hw
    B = 2
    K, E = R.exact_calibration(B)
    x = _frames(B, H, W, seed=H * 131 + W, p=0.3)
    x[0].reshape(-1)[-1] = 5.0  # the frame's last pixel
    pay = _payload(x.shape, 3)
    n = 0
    for keep in (0, 2):
        for stride, payload in ((3, None), (4, None), (4, pay)):
            opt = dict(pitch=n % 3 != 1, pixel=n % 3 != 2, status=n % 4 != 3, x_off=4 * (n % 2), p_off=4 * ((n // 2) % 2),
                       kind=KINDS[n % 3])
            check_forward(L, x, K, E, "%s keep %d stride %d %r" % (hw, keep, stride, opt), payload=payload, keep_every=keep,
                          stride=stride, **opt)
            n += 1


def test_empty_one_pixel_and_full_frames_side_by_side(pkg, dev):
    L = pkg._lib.load()
    H, W = SEAM_SHAPES[2]
    K, E = R.exact_calibration(3)
    x = np.zeros((3, H, W), F)
    x[1, 1, 17] = 9.5
    x[2] = _frames(1, H, W, 4, p=2.0)[0]
    for keep in (0, 4):
        got, _ = check_forward(L, x, K, E, "side by side keep %d" % keep, keep_every=keep, stride=4, payload=_payload(x.shape, 9))
        assert got["status"].tolist() == [R.NO_POINTS, R.BAD_INTERVAL if keep else 0, 0]
    assert got["counts"][0].tolist() == [0, 0]


def test_last_lane_last_wave_last_tile(pkg, dev):
    L = pkg._lib.load()
    H, W = TWO_TILES_PLUS_ONE
    K, E = R.exact_calibration(4)
    x = np.zeros((4, H, W), F)
    x[0, 0, 2 * TILE] = 3.0  # the last tile's only pixel
    x[1, 0, TILE - 8:TILE] = np.arange(8) + 2.0  # tile 0's last lane
    x[2, 0, TILE - 512:TILE] = _frames(1, 1, 512, 2, p=0.5)[0, 0]  # its last wave
    x[3, 0, TILE:] = _frames(1, 1, TILE + 1, 3, p=0.7)[0, 0]  # nothing in tile 0
    for keep in (0, 2):
        check_forward(L, x, K, E, "last lanes keep %d" % keep, keep_every=keep)


def test_every_mask_of_a_3x4_frame(pkg, dev):
    L = pkg._lib.load()
    B = 4096
    K, E = R.exact_calibration(B)
    bits = (np.arange(B)[:, None] >> np.arange(12)[None]) & 1
    depth = (np.arange(12, dtype=F) * F(0.75) + F(1.5))[None]
    x = (bits * depth).astype(F).reshape(B, 3, 4)
    got, ref = check_forward(L, x, K, E, "all masks", stride=4, payload=_payload(x.shape, 1))
    assert got["counts"][:, 0].tolist() == [bin(b).count("1") for b in range(B)]
    check_forward(L, x, K, E, "all masks, keep mode", keep_every=2, n_bins=8)


def test_capacity(pkg, dev):
    L = pkg._lib.load()
    H, W = 64, 65
    K, E = R.exact_calibration(2)
    x = _frames(2, H, W, 21, p=0.4)
    x[1, H // 2:] = 0  # fewer points in frame 1
    total = int(np.count_nonzero(x[0]))
    assert np.count_nonzero(x[1]) < total - 1
    for N, over in ((total, 0), (total - 1, R.OVERFLOW), (1, R.OVERFLOW)):
        got, _ = check_forward(L, x, K, E, "N = %d" % N, N=N, stride=4)
        assert got["status"].tolist() == [over, over if N == 1 else 0] and got["counts"][0].tolist() == [N, total]


def test_status_frames(pkg, dev):
    L = pkg._lib.load()
    H, W = 5, 7
    K, E = R.exact_calibration(5)
    x = _frames(5, H, W, 8, p=0.6)
    K[0, 1] = 0.0  # singular K
    E[1, 2] = 0.0  # singular E
    x[2] = 0
    x[2, 3, 3] = 4.0  # a single point
    x[3] = 0  # empty
    got, _ = check_forward(L, x, K, E, "status")
    assert got["status"].tolist() == [R.SINGULAR, R.SINGULAR, 0, R.NO_POINTS, 0]
    got, _ = check_forward(L, x, K, E, "status, keep mode", keep_every=2)
    assert got["status"].tolist() == [R.SINGULAR, R.SINGULAR, R.BAD_INTERVAL, R.NO_POINTS, 0]
    assert not got["counts"][:4].any()


# ---------------------------------------------------------------------------------------------------------------------------
# cross-checks on the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_keep_mode_selects_what_line_subsample_keeps(pkg, dev, synth):
    import torch

    x, K, E = synth.velodyne_scan(2, seed=3)
    xd = torch.from_numpy(x).to(DEV)
    for ke in (1, 2, 4):
        sub, st = dev.line_subsample_device(xd, K, E, 1.0 / ke)
        pts, counts, status, pitch, pixel = dev.unproject_device(xd, K, E, keep_ratio=1.0 / ke, want=("pitch", "pixel"))
        torch.cuda.synchronize()
        sub, counts, pixel = sub.cpu().numpy(), counts.cpu().numpy(), pixel.cpu().numpy()
        assert not st.cpu().numpy().any() and not status.cpu().numpy().any()
        for b in range(2):
            want = np.flatnonzero(sub[b].reshape(-1))
            assert counts[b].tolist() == [want.size, want.size]
            assert np.array_equal(pixel[b, :want.size], want)
    # the whole frame (ke = 1): the points next to unproj_ref's, whose inverses are LAPACK's.  The calibration's inverse
    # enters every coordinate linearly, so a last-bit difference in it moves a float64 coordinate by a few ulp and its
    # float32 rounding by at most one float32 ulp, and that only for coordinates within that distance of a rounding boundary
    ref = R.forward(x, K, E)
    pts, counts, _, _, _ = dev.unproject_device(xd, K, E)
    got, counts = pts.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, ref["counts"])
    for b in range(2):
        n = int(counts[b, 0])
        ulp = np.abs(_bits(got[b, :n]).astype(np.int64) - _bits(ref["points"][b]).astype(np.int64))
        assert ulp.max() <= 1 and (ulp != 0).mean() < 1e-3, (ulp.max(), (ulp != 0).mean())


def test_chain_with_project_points(pkg, dev, synth):
    import torch

    # exact calibration: the device chain equals proj_ref of unproj_ref's points bit for bit, and gives the input's pixel set
    H, W = 64, 65
    K, E = R.exact_calibration(2, fx=64.0, fy=64.0, cx=32.0, cy=31.5)
    x = _frames(2, H, W, 33, p=0.2)
    xd = torch.from_numpy(x).to(DEV)
    pts, counts, status, _, _ = dev.unproject_device(xd, K, E)
    f32, st, n4, f64 = dev.project_points_device(pts, counts[:, 0].contiguous(), K, E, (H, W), mode="zbuffer", want="both")
    torch.cuda.synchronize()
    ref = R.forward(x, K, E)
    for b in range(2):
        z, rst, cnt = proj_ref.project_frame(ref["points"][b], K[b], E[b], H, W, proj_ref.ZBUFFER)
        _same(f64[b].cpu().numpy(), z, "frame %d z" % b)
        assert np.array_equal(f32[b].cpu().numpy() != 0, x[b] > F(0.1)) and np.array_equal(n4[b].cpu().numpy(), cnt)
    # KITTI scans under their own calibration, on the device alone: the pixel set, and the depths within the round trip's bound
    # (tests/test_unproject.py: 2 * 2^-24 relative)
    x, K, E = synth.velodyne_scan(2, seed=3)
    xd = torch.from_numpy(x).to(DEV)
    pts, counts, status, _, _ = dev.unproject_device(xd, K, E)
    f32, st, n4, f64 = dev.project_points_device(pts, counts[:, 0].contiguous(), K, E, x.shape[1:], mode="zbuffer", want="both")
    z = f64.cpu().numpy()
    valid = x > F(0.1)
    assert np.array_equal(z != 0, valid)
    assert (np.abs(z[valid] - x[valid]) / x[valid]).max() <= 2.0 * 2.0 ** -24


@pytest.mark.parametrize("metric", ["l1_cv", "l2"])
def test_unproject_a_filled_frame(pkg, dev, metric):
    import torch

    H, W = 64, 65
    K, E = R.exact_calibration(2)
    x = _frames(2, H, W, 41, p=0.05)
    depth = torch.from_numpy(np.ascontiguousarray(dev.fill(x, metric=metric)["depth"])).to(DEV)
    pts, counts, status, pitch, pixel = dev.unproject_device(depth, K, E, want=("pitch", "pixel"))
    torch.cuda.synchronize()
    d = depth.cpu().numpy()
    assert (d > 0.1).all()  # dense
    ref = R.forward(d, K, E)
    assert counts.cpu().numpy().tolist() == [[H * W, H * W]] * 2 and not status.cpu().numpy().any()
    for b in range(2):
        _same(pts[b].cpu().numpy(), ref["points"][b], "points")
        _pitch_close(pitch[b].cpu().numpy(), ref["pitch"][b], "pitch")
        assert np.array_equal(pixel[b].cpu().numpy(), np.arange(H * W))


# ---------------------------------------------------------------------------------------------------------------------------
# the backward
# ---------------------------------------------------------------------------------------------------------------------------
def run_backward(L, g, pixel, counts, K, E, H, W, want_payload=False, status=True, g_off=0, kind="random"):
    import torch

    B, N, stride = g.shape
    Kd, Ed = _up(np.broadcast_to(K, (B, 3, 3))), _up(np.broadcast_to(E, (B, 4, 4)))
    gg, ig, cg = _up(g, g_off), _up(pixel), _up(counts)
    xg = _filled(B * H * W * 4, F, (B, H, W), POISON["grad"], 4 - g_off)[0]
    pg = _filled(B * H * W * 4, F, (B, H, W), POISON["grad"])[0] if want_payload else None
    sg = _filled(B * 4, np.int32, (B,), POISON["status"])[0] if status else None
    nws = L.dtfill_unproject_backward_workspace_bytes(B, H, W)
    wg = GuardedBuffer(nws, 0, DEV)
    poison(wg.payload(), kind, seed=N)
    rc = L.dtfill_unproject_backward(gg.ptr, ig.ptr, cg.ptr, B, N, stride, H, W, Kd.ptr, Ed.ptr, xg.ptr,
                                     None if pg is None else pg.ptr, None if sg is None else sg.ptr, wg.ptr, nws,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for gd, what in ((gg, "grad_points"), (ig, "pixel"), (cg, "counts"), (xg, "grad_x"), (pg, "grad_payload"), (sg, "status"),
                     (wg, "workspace")):
        if gd is not None:
            gd.check(what)
    return (_down(xg, F, (B, H, W)), _down(pg, F, (B, H, W)) if want_payload else None,
            _down(sg, np.int32, (B,)) if status else None)


def check_backward(L, g, pixel, counts, K, E, H, W, what="", **kw):
    got = run_backward(L, g, pixel, counts, K, E, H, W, **kw)
    ref = R.backward(g, pixel, counts, K, E, H, W, kw.get("want_payload", False))
    _same(got[0], ref[0], what + " grad_x")
    if ref[1] is not None:
        _same(got[1], ref[1], what + " grad_payload")
    if got[2] is not None:
        assert np.array_equal(got[2], ref[2]), (what, got[2], ref[2])
    return got


def _lists(x, N, seed):
    """(pixel int32 [B,N], counts int32 [B,2]) as the forward writes them for x, the padding beyond n_b arbitrary."""
    B = x.shape[0]
    pixel = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, (B, N)).astype(np.int32)
    counts = np.zeros((B, 2), np.int32)
    for b in range(B):
        p = np.flatnonzero(x[b].reshape(-1) > F(0.1))[:N]
        pixel[b, :p.size] = p
        counts[b] = p.size, np.count_nonzero(x[b] > F(0.1))
    return pixel, counts


@pytest.mark.parametrize("hw", SHAPES)
def test_backward_shapes(pkg, dev, hw):
    L = pkg._lib.load()
    H, W = hw
    B = 2
    K, E = R.exact_calibration(B)
    x = _frames(B, H, W, seed=H * 17 + W, p=0.3)
    x[0].reshape(-1)[-1] = 5.0
    n = 0
    for N in (H * W, max(1, H * W // 5)):
        pixel, counts = _lists(x, N, 5)
        for stride, wp in ((3, False), (4, True), (4, False), (3, True)):
            g = _payload((B, N, stride), n) if stride == 4 else np.random.default_rng(n).standard_normal((B, N, 3)).astype(F)
            if stride == 4:  # any bits in the payload column, numbers in the three that enter arithmetic
                g[..., :3] = np.random.default_rng(n).standard_normal((B, N, 3)).astype(F)
            check_backward(L, g, pixel, counts, K, E, H, W, "%s N %d stride %d" % (hw, N, stride), want_payload=wp,
                           status=n % 3 != 2, g_off=4 * (n % 2), kind=KINDS[n % 3])
            n += 1


def test_backward_bad_lists_and_counts(pkg, dev):
    L = pkg._lib.load()
    H, W = 64, 65
    B = 6
    K, E = R.exact_calibration(B)
    x = _frames(B, H, W, 77, p=0.3)
    N = 3000
    pixel, counts = _lists(x, N, 6)
    n1 = int(counts[1, 0])
    pixel[1, [n1 - 2, n1 - 1]] = pixel[1, [n1 - 1, n1 - 2]]  # a swapped pair, in the last block
    pixel[2, int(counts[2, 0]) - 1] = H * W  # one past the frame
    pixel[3, 1] = pixel[3, 0]  # a repeated pixel
    counts[4, 0] = N + 1
    K[5, 1] = 0.0  # singular
    g = np.random.default_rng(3).standard_normal((B, N, 4)).astype(F)
    gx, gp, st = check_backward(L, g, pixel, counts, K, E, H, W, "bad lists", want_payload=True)
    assert st.tolist() == [0, R.BAD_PIXEL, R.BAD_PIXEL, R.BAD_PIXEL, R.BAD_COUNT, R.SINGULAR]
    assert gx[0].any() and not _bits(gx[1:]).any() and not _bits(gp[1:]).any()
    counts[4, 0] = -1
    _, _, st = check_backward(L, g, pixel, counts, K, E, H, W, "negative count")
    assert st[4] == R.BAD_COUNT


@pytest.mark.parametrize("with_payload", [False, True])
def test_autograd_unproject(pkg, dev, with_payload):
    import torch

    H, W = 64, 65
    K, E = R.exact_calibration(2)
    xh = _frames(2, H, W, 55, p=0.3)  # about 1250 points a frame: more than the capacity
    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    pay = torch.from_numpy(np.random.default_rng(2).standard_normal(xh.shape).astype(F)).to(DEV).requires_grad_(True) \
        if with_payload else None
    points, counts, pixel, status = pkg.autograd.unproject(x, K, E, payload=pay, capacity=1000)
    assert not counts.requires_grad and not pixel.requires_grad and not status.requires_grad and points.requires_grad
    wh = np.random.default_rng(4).standard_normal(tuple(points.shape)).astype(F)
    n = counts[:, 0].cpu().numpy()
    mask = (np.arange(1000)[None, :] < n[:, None])[..., None]  # the records beyond n_b are not written: they take no part
    w = torch.from_numpy(wh * mask).to(DEV)
    (torch.where(torch.from_numpy(np.broadcast_to(mask, wh.shape).copy()).to(DEV), points, torch.zeros_like(points)) * w).sum().backward()
    torch.cuda.synchronize()
    ref = R.forward(xh, K, E, payload=None if pay is None else pay.detach().cpu().numpy(), N=1000, stride=4 if with_payload else 3)
    assert np.array_equal(counts.cpu().numpy(), ref["counts"]) and (ref["status"] == R.OVERFLOW).any()
    for b in range(2):
        _same(points[b, :n[b]].detach().cpu().numpy(), ref["points"][b], "points")
    gx, gp, _ = R.backward(wh * mask, pixel.cpu().numpy(), ref["counts"], K, E, H, W, want_payload=with_payload)
    _same(x.grad.cpu().numpy(), gx, "x.grad")
    if with_payload:
        _same(pay.grad.cpu().numpy(), gp, "payload.grad")


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer: arguments, the numpy functions
# ---------------------------------------------------------------------------------------------------------------------------
def test_device_function_argument_errors(pkg, dev):
    import torch

    K, E = R.exact_calibration()
    x = torch.zeros((1, 5, 7), device=DEV)
    for bad, kw in ((x[0], {}), (x.double(), {}), (x.cpu(), {}), (x.transpose(1, 2), {}), (x, dict(payload=x[:, :4])),
                    (x, dict(val_thr=float("nan"))), (x, dict(stride=5)), (x, dict(stride=3, payload=x)), (x, dict(capacity=0)),
                    (x, dict(capacity=2.5)), (x, dict(want=("pitch", "ring"))), (x, dict(keep_ratio=0.3)),
                    (x, dict(keep_ratio=0.5, n_bins=0)), (x, dict(K=np.eye(4)))):
        kw = dict(kw)
        with pytest.raises(ValueError):
            dev.unproject_device(bad, kw.pop("K", K), E, **kw)
    g = torch.zeros((1, 9, 3), device=DEV)
    pixel, counts = torch.zeros((1, 9), dtype=torch.int32, device=DEV), torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    for args, kw in (((g[0], pixel, counts), {}), ((g, pixel.long(), counts), {}), ((g, pixel[:, :8].contiguous(), counts), {}),
                     ((g, pixel, counts[:, 0].contiguous()), {}), ((g, pixel, counts), dict(want_payload=True)),
                     ((g, pixel, counts), dict(hw=(5, 0)))):
        with pytest.raises(ValueError):
            dev.unproject_backward_device(*args, K, E, kw.pop("hw", (5, 7)), **kw)
    assert dev.unproject_device(x, K, E, want=())[3:] == (None, None)


def test_numpy_functions(pkg, dev, synth):
    x, K, E = synth.velodyne_scan(2, seed=3)
    Ke, Ee = R.exact_calibration(2)
    ref = R.forward(x, Ke, Ee)
    got = pkg.get_all_points(x[0][..., None], Ke[0].reshape(-1), Ee[0], image_coor_tensor=object())
    assert got.dtype == F
    _same(got, ref["points"][0], "get_all_points")
    small = x[:, 200:264, 300:365]
    ref = R.forward(small, Ke, Ee, keep_every=2, stride=4, payload=small * 2)
    clouds, pitches = pkg.unproject_frames(small, Ke, Ee, payload=small * 2, keep_ratio=0.5, with_pitch=True)
    for b in range(2):
        _same(clouds[b], ref["points"][b], "cloud %d" % b)
        _pitch_close(pitches[b], ref["pitch"][b], "pitch %d" % b)
    assert [c.shape for c in pkg.unproject_frames(np.zeros((2, 5, 7), F), Ke, Ee)] == [(0, 3)] * 2
    with pytest.raises(ValueError, match="no point"):
        pkg.unproject_frames(np.zeros((5, 7), F), Ke[0], Ee[0], keep_ratio=0.5)
    with pytest.raises(np.linalg.LinAlgError):
        pkg.get_all_points(x[0], np.zeros((3, 3)), Ee[0])
    one = np.zeros((5, 7), F)
    one[2, 2] = 3.0
    assert pkg.unproject_frames(one, Ke[0], Ee[0], keep_ratio=0.25)[0].shape == (0, 3)  # NaN labels keep nothing


# ---------------------------------------------------------------------------------------------------------------------------
# streams and threads
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_streams_and_four_threads(pkg, dev):
    import torch

    H, W = TWO_TILES_PLUS_ONE[1] // 61 + 1, 61  # 68 x 61 = 4148 px: three tiles
    cases = []
    for k in range(4):
        K, E = R.exact_calibration(3)
        x = _frames(3, H, W, 100 + k, p=0.1 + 0.2 * k)
        keep = (0, 2)[k % 2]
        ref = R.forward(x, K, E, keep_every=keep, N=600)
        g = np.random.default_rng(k).standard_normal((3, 600, 3)).astype(F)
        pix = np.zeros((3, 600), np.int32)
        for b in range(3):
            pix[b, :ref["counts"][b, 0]] = ref["pixel"][b]
        cases.append(dict(x=torch.from_numpy(x).to(DEV), K=K, E=E, keep=keep, ref=ref, g=torch.from_numpy(g).to(DEV),
                          gx=R.backward(g, pix, ref["counts"], K, E, H, W)[0]))
    torch.cuda.synchronize()

    def step(c):
        pts, counts, status, pitch, pixel = dev.unproject_device(c["x"], c["K"], c["E"], capacity=600,
                                                                 keep_ratio=0.5 if c["keep"] else None, want=("pitch", "pixel"))
        gx, _, _ = dev.unproject_backward_device(c["g"], pixel, counts, c["K"], c["E"], (H, W))
        return pts, counts, status, pitch, pixel, gx

    def verify(c, out):
        pts, counts, status, pitch, pixel, gx = (t.cpu().numpy() for t in out)
        ref = c["ref"]
        assert np.array_equal(counts, ref["counts"]) and np.array_equal(status, ref["status"])
        for b in range(3):
            n = int(counts[b, 0])
            _same(pts[b, :n], ref["points"][b], "points")
            _pitch_close(pitch[b, :n], ref["pitch"][b], "pitch")
            assert np.array_equal(pixel[b, :n], ref["pixel"][b])
        _same(gx, c["gx"], "grad_x")

    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    outs = []
    for k, s in enumerate(streams * 2):  # all four queued before any is waited for
        with torch.cuda.stream(s):
            outs.append(step(cases[k]))
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        verify(cases[k], out)

    def work(k, r):
        out = step(cases[(k + r) % 4])
        torch.cuda.current_stream().synchronize()
        verify(cases[(k + r) % 4], out)

    failures = concurrency.run_rounds(work, 4, 3)
    assert not failures, concurrency.describe(failures)

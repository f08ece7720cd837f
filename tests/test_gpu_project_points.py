"""The LiDAR point projection on the device (dtfill_project_points, project_points_device, project_points,
map_points_on_image) against the numpy statement in tests/proj_ref.py, which tests/test_project_points.py holds to
hand-written values and to the reference's np.dot form.  Bit for bit everywhere: both outputs, the status and the counts.
Every call through the C ABI here runs in guarded buffers with poisoned outputs, a poisoned workspace and NaN bit patterns in
every record the call must not read (_abi)."""
import functools
import importlib
import itertools

import numpy as np
import pytest

import proj_cases as C
import proj_ref as R
from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"reference": R.REFERENCE, "zbuffer": R.ZBUFFER}
F64_POISON = 0x7FF5A5A5A5A5A5A5  # a NaN payload no projection produces
REC_POISON = 0x7FA5A5A5  # float32 NaN bit pattern in the padding records
_KIND = itertools.count()


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


def _bits_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(ref).view(view)
    assert not bad.any(), "%s: %d elements differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _abi(L, pts, counts, K, E, H, W, mode, min_z=0.0, po=0, want="both", status=True, cnt=True, stream=None):
    """dtfill_project_points on pts float32 [B, N, stride] (numpy) with the records po bytes after a 256-byte boundary, every
    buffer between guards, the outputs and the workspace poisoned.  Checks the guards, that the inputs are unchanged and that no
    output element is left poisoned; returns (f32 or None, f64 or None, status or None, counts4 or None) as numpy."""
    import torch

    pts = np.ascontiguousarray(pts, np.float32)
    B, N, stride = pts.shape
    K = np.array(np.broadcast_to(np.asarray(K, np.float64), (B, 3, 3)))  # (a copy: writable, contiguous)
    E = np.array(np.broadcast_to(np.asarray(E, np.float64), (B, 4, 4)))
    nws = L.dtfill_project_points_workspace_bytes(B, N, H, W)
    assert nws > 0
    pg = GuardedBuffer(pts.nbytes, po, DEV, N * stride * 4)
    pg.view(torch.int32, (pts.size,)).copy_(torch.from_numpy(pts.reshape(-1).view(np.int32).copy()))  # (as bits: NaN payloads stay)
    kg, eg = GuardedBuffer(K.nbytes, 0, DEV), GuardedBuffer(E.nbytes, 0, DEV)
    kg.view(torch.float64, (B, 3, 3)).copy_(torch.from_numpy(K))
    eg.view(torch.float64, (B, 4, 4)).copy_(torch.from_numpy(E))
    bufs = [(pg, "points"), (kg, "K"), (eg, "E")]
    cg = fg = dg = sg = ng = None
    if counts is not None:
        cg = GuardedBuffer(4 * B, 0, DEV)
        cg.view(torch.int32, (B,)).copy_(torch.from_numpy(np.asarray(counts, np.int32)))
        bufs.append((cg, "counts"))
    if want != "float64":
        fg = GuardedBuffer(4 * B * H * W, 4, DEV, 4 * H * W)  # only element-aligned
        poison_output(fg.view(torch.float32, (B * H * W,)), "depth")
        bufs.append((fg, "out_f32"))
    if want != "float32":
        dg = GuardedBuffer(8 * B * H * W, 8, DEV, 8 * H * W)
        dg.view(torch.int64, (B * H * W,)).fill_(F64_POISON)
        bufs.append((dg, "out_f64"))
    if status:
        sg = GuardedBuffer(4 * B, 0, DEV)
        poison_output(sg.view(torch.int32, (B,)), "status")
        bufs.append((sg, "status"))
    if cnt:
        ng = GuardedBuffer(16 * B, 0, DEV)
        poison_output(ng.view(torch.int32, (4 * B,)), "status")
        bufs.append((ng, "frame_counts"))
    wg = GuardedBuffer(nws, 0, DEV)
    k = next(_KIND)
    poison(wg.payload(), KINDS[k % 3], seed=k)  # zero, ones, random in turn
    bufs.append((wg, "workspace"))
    ptr = lambda g: None if g is None else g.ptr
    st = torch.cuda.current_stream() if stream is None else stream
    if stream is not None:
        torch.cuda.synchronize()  # the buffers were filled on the current stream
    rc = L.dtfill_project_points(pg.ptr, ptr(cg), B, N, stride, H, W, kg.ptr, eg.ptr, mode, float(min_z), ptr(fg), ptr(dg),
                                 ptr(sg), ptr(ng), wg.ptr, nws, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in bufs:
        g.check(what)
    assert np.array_equal(pg.view(torch.int32, (pts.size,)).cpu().numpy(), pts.reshape(-1).view(np.int32)), "points changed"
    f32 = f64 = s = n4 = None
    if fg is not None:
        f32 = fg.view(torch.float32, (B, H, W)).cpu().numpy()
        assert not is_poison(f32, "depth").any(), "out_f32 elements left unwritten"
    if dg is not None:
        f64 = dg.view(torch.float64, (B, H, W)).cpu().numpy()
        assert not (f64.view(np.int64) == F64_POISON).any(), "out_f64 elements left unwritten"
    if sg is not None:
        s = sg.view(torch.int32, (B,)).cpu().numpy()
    if ng is not None:
        n4 = ng.view(torch.int32, (B, 4)).cpu().numpy()
    return f32, f64, s, n4


def _check(L, pts, counts, K, E, H, W, mode, what, ref=None, **kw):
    """One guarded call against the statement: both outputs, status and counts, bit for bit.  Returns the statement's result."""
    ref = R.project(pts, counts, K, E, H, W, mode, kw.get("min_z", 0.0)) if ref is None else ref
    f32, f64, st, n4 = _abi(L, pts, counts, K, E, H, W, mode, **kw)
    if f32 is not None:
        _bits_equal(f32, ref[0], what + " out_f32")
    if f64 is not None:
        _bits_equal(f64, ref[1], what + " out_f64")
    if st is not None:
        assert np.array_equal(st, ref[2]), (what, st, ref[2])
    if n4 is not None:
        assert np.array_equal(n4, ref[3]), (what, n4, ref[3])
    return ref


def _padded(clouds, stride, N=None):
    """Ragged clouds [n_b, 3|4] -> (points [B, N, stride] with NaN bit patterns in every float the call must not use, counts)."""
    N = max(1, max(len(c) for c in clouds)) if N is None else N
    pts = np.zeros((len(clouds), N, stride), np.float32)
    pts.view(np.uint32)[:] = REC_POISON
    for b, c in enumerate(clouds):
        pts[b, :len(c), :3] = c[:, :3]
    return pts, np.array([len(c) for c in clouds], np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# small frames: the hand cases, block edges, one pixel under thousands of points, ragged batches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("po", [0, 4], ids=["aligned", "one_float_off"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_hand_cases(pkg, dev, mode, stride, po):
    cs = C.cases()
    names = sorted(cs)
    pts, counts, K, E = C.batch([cs[n] for n in names], stride, N=64)
    ref = _check(pkg._lib.load(), pts, counts, K, E, C.H, C.W, MODES[mode], "hand cases", po=po)
    key = "ref" if mode == "reference" else "zbuf"
    for b, n in enumerate(names):  # ... and the statement still says what the cases say
        assert ref[2][b] == cs[n][key][0], n
        _bits_equal(ref[1][b], C.expected_frame(cs[n][key][1]), n)


SMALL_HW = (9, 13)


@functools.lru_cache(maxsize=None)
def _small_calibration(B):
    """Per-frame K and E of a 9 x 13 camera: the axis permutation with a small rotation and an offset, focal length 6."""
    rng = np.random.default_rng(77)
    K = np.zeros((B, 3, 3))
    E = np.zeros((B, 4, 4))
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    for b in range(B):
        a = rng.normal(0.0, 0.02, 3)
        rot = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])  # near a rotation: any matrix is legal
        K[b] = [[6.0 + 0.1 * b, 0.0, 6.3], [0.0, 6.1, 4.2 + 0.05 * b], [0.0, 0.0, 1.0]]
        E[b, :3, :3] = rot @ perm
        E[b, :3, 3] = [-0.004, -0.076, -0.272]
        E[b, 3, 3] = 1.0
    return K, E


def _cloud_on(rng, n, K, E, wrap, behind=0.0):
    """n float32 points of the Velodyne frame that project 0.3 px or less from the centre of a pixel drawn uniformly from the
    frame (wrap: from the wrap range [-W + 1, W - 2] x [-H + 1, H - 2] of the REFERENCE mode) at depths 1..50 m; a share of them
    mirrored behind the camera.  The pixels are few, so nearly every pixel is fought over."""
    H, W = SMALL_HW
    u = rng.integers(-W + 1, W - 1, n) if wrap else rng.integers(-2, W + 2, n)
    v = rng.integers(-H + 1, H - 1, n) if wrap else rng.integers(-2, H + 2, n)
    z = rng.uniform(1.0, 50.0, n) * np.where(rng.random(n) < behind, -1.0, 1.0)
    pix = np.stack([u + rng.uniform(-0.3, 0.3, n), v + rng.uniform(-0.3, 0.3, n), np.ones(n)])
    cam = np.linalg.inv(K) @ (pix * z)
    return (np.linalg.inv(E) @ np.vstack([cam, np.ones((1, n))]))[:3].T.astype(np.float32)


def _point_at(K, E, u, v, z):
    """The float32 point of the Velodyne frame that projects to the centre of pixel (v, u) at depth z."""
    cam = np.linalg.inv(K) @ (np.array([u, v, 1.0]) * z)
    return (np.linalg.inv(E) @ np.append(cam, 1.0))[:3].astype(np.float32)


EDGE_COUNTS = (1, 255, 256, 257, 1025, 2048, 2049)  # around a tile of 256 points, across tiles, around a block of 2048


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_block_edges_ragged_batch_with_an_index_error_frame(pkg, dev, mode, stride):
    """B = 9 with different K and E: n_b around and across a block, one frame with a point past the wrap range among the valid
    ones, one frame with a bad count; NaN bit patterns in every padding record."""
    rng = np.random.default_rng(1)
    counts = EDGE_COUNTS + (300, 40)
    K, E = _small_calibration(len(counts))
    clouds = [_cloud_on(rng, n, K[b], E[b], wrap=mode == "reference", behind=0.2) for b, n in enumerate(counts)]
    # frame 7, point 100: three frame widths to the left -- an IndexError in the reference, outside in the z-buffer
    clouds[7][100] = _point_at(K[7], E[7], -3 * SMALL_HW[1], 4, 7.0)
    pts, n = _padded(clouds, stride)
    n[8] = pts.shape[1] + 1  # a bad count: nothing of the frame is read
    H, W = SMALL_HW
    ref = _check(pkg._lib.load(), pts, n, K, E, H, W, MODES[mode], "block edges " + mode, po=4)
    assert ref[2][8] == R.BAD_COUNT and not ref[3][8].any()
    if mode == "reference":
        assert list(ref[2]) == [0] * 7 + [R.INDEX_ERROR, R.BAD_COUNT]  # (the other frames are what they were made to be)
        assert (ref[3][:7, R.INSIDE] == EDGE_COUNTS).all() and (ref[3][1:7, R.PIXELS] > 50).all()
    else:
        assert not ref[2][1:8].any() and (ref[3][1:8, R.BEHIND] > 0).all() and (ref[3][1:8, R.OUTSIDE] > 0).all()
        assert (ref[3][1:8, R.INSIDE] > ref[3][1:8, R.PIXELS]).all()  # pixels were fought over


@pytest.mark.parametrize("mode", sorted(MODES))
def test_4096_points_on_one_pixel(pkg, dev, mode):
    """Every point lands on pixel (2, 3) of a 5 x 7 frame: depths 1 + k / 64 increasing, decreasing and shuffled."""
    z = 1.0 + np.arange(4096) / 64.0
    orders = [z, z[::-1], np.random.default_rng(4).permutation(z)]
    pts = np.stack([np.stack([3 * o, 2 * o, o], 1) for o in orders]).astype(np.float32)  # exact in float32
    ref = _check(pkg._lib.load(), pts, None, np.eye(3), np.eye(4), C.H, C.W, MODES[mode], "one pixel " + mode)
    want = [o[-1] for o in orders] if mode == "reference" else [1.0] * 3
    assert [ref[1][b, 2, 3] for b in range(3)] == want and (ref[3][:, R.PIXELS] == 1).all() and (ref[3][:, R.INSIDE] == 4096).all()


def test_counts_null_and_single_outputs(pkg, dev):
    rng = np.random.default_rng(2)
    K, E = _small_calibration(2)
    H, W = SMALL_HW
    L = pkg._lib.load()
    for mode in sorted(MODES):
        pts, _ = _padded([_cloud_on(rng, 300, K[b], E[b], wrap=mode == "reference") for b in range(2)], 4)
        ref = _check(L, pts, None, K, E, H, W, MODES[mode], "counts NULL " + mode)
        assert not ref[2].any() and ref[1].any()
        _check(L, pts, None, K, E, H, W, MODES[mode], "float32 alone " + mode, ref=ref, want="float32", status=False)
        _check(L, pts, None, K, E, H, W, MODES[mode], "float64 alone " + mode, ref=ref, want="float64", cnt=False)
        _check(L, pts, None, K, E, H, W, MODES[mode], "no status, no counts " + mode, ref=ref, status=False, cnt=False)


def test_min_z(pkg, dev):
    rng = np.random.default_rng(3)
    K, E = _small_calibration(1)
    pts, n = _padded([_cloud_on(rng, 500, K[0], E[0], wrap=False)], 3)
    L = pkg._lib.load()
    H, W = SMALL_HW
    near = _check(L, pts, n, K, E, H, W, R.ZBUFFER, "min_z 0")
    far = _check(L, pts, n, K, E, H, W, R.ZBUFFER, "min_z 25.3", min_z=25.3)
    assert far[3][0, R.BEHIND] > near[3][0, R.BEHIND] and far[1][far[1] != 0].min() > np.float64(np.float32(25.3))
    # REFERENCE ignores it, whatever it holds
    pts, n = _padded([_cloud_on(rng, 500, K[0], E[0], wrap=True)], 3)
    _check(L, pts, n, K, E, H, W, R.REFERENCE, "reference ignores min_z", min_z=float("nan"))


# ---------------------------------------------------------------------------------------------------------------------------
# KITTI-sized: whole sweeps into 352 x 1216, and the fill behind them
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweeps(synth):
    """velodyne_points(2) with the statement's z-buffered projection, worked out once."""
    clouds, K, E = synth.velodyne_points(2)
    pts, n = _padded(clouds, 4)
    ref = R.project(pts, n, K, E, 352, 1216, R.ZBUFFER)
    for a in ref:
        a.setflags(write=False)
    return clouds, pts, n, K, E, ref


def test_kitti_sized_sweeps(pkg, dev, sweeps):
    clouds, pts, n, K, E, ref = sweeps
    L = pkg._lib.load()
    _check(L, pts, n, K, E, 352, 1216, R.ZBUFFER, "sweeps z-buffer", ref=ref, po=4)
    assert not ref[2].any() and (ref[3][:, R.PIXELS] > 10000).all() and (ref[3][:, R.BEHIND] > ref[3][:, R.INSIDE]).all()
    # the reference's function on a whole sweep: points behind the camera and far beside it raise
    whole = _check(L, pts, n, K, E, 352, 1216, R.REFERENCE, "sweeps reference")
    assert (whole[2] == R.INDEX_ERROR).all() and not whole[1].any()
    # ... and on the points a caller would have cut to the frame first: a valid frame, the last writer's depth
    cut = []
    for c, Kb, Eb in zip(clouds, K, E):
        z, u, v = R.ordered_form(c, Kb, Eb)
        cut.append(c[(z > 0) & (u >= 0) & (u < 1216) & (v >= 0) & (v < 352)])
    cpts, cn = _padded(cut, 4)
    valid = _check(L, cpts, cn, K, E, 352, 1216, R.REFERENCE, "cut sweeps reference")
    assert not valid[2].any() and np.array_equal(valid[3][:, R.INSIDE], cn)


@pytest.mark.parametrize("metric", ["l1_cv", "l2"])
def test_projected_frame_fills_like_the_statements(pkg, dev, oracle, sweeps, metric):
    """DtFill.run on the projected frame, with no copy in between, equals the oracle's fill of the statement's frame."""
    import torch

    clouds, pts, n, K, E, ref = sweeps
    frame, status, counts4 = dev.project_points_device(torch.from_numpy(pts).to(DEV), n, K, E, (352, 1216))
    op = pkg.device.DtFill(device=DEV, metric=metric)
    got = op.run(frame)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and np.array_equal(counts4.cpu().numpy(), ref[3])
    depth, dt, idx, st = oracle.fill_batch(np.ascontiguousarray(ref[0]), 0.1, 0.1, metric=metric)
    assert not st.any() and np.array_equal(got["status"].cpu().numpy() & 1, st)
    assert np.array_equal(got["index"].cpu().numpy(), idx)
    _bits_equal(got["dt"].cpu().numpy(), dt, metric + " dt")
    _bits_equal(got["depth"].cpu().numpy(), depth, metric + " depth")


# ---------------------------------------------------------------------------------------------------------------------------
# the same bits on every run and on every stream
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_calls_and_a_second_stream_give_identical_bits(pkg, dev, mode):
    import torch

    rng = np.random.default_rng(5)
    counts = (4000, 2500, 1)
    K, E = _small_calibration(3)
    clouds = [_cloud_on(rng, c, K[b], E[b], wrap=mode == "reference", behind=0.1) for b, c in enumerate(counts)]
    pts, n = _padded(clouds, 3)
    H, W = SMALL_HW
    ref = R.project(pts, n, K, E, H, W, MODES[mode])
    pd = torch.from_numpy(pts).to(DEV)
    torch.cuda.synchronize()
    res = [dev.project_points_device(pd, n, K, E, (H, W), mode=mode, want="both") for _ in range(2)]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    for s in streams:  # both queued before either is waited for
        with torch.cuda.stream(s):
            res.append(dev.project_points_device(pd, n, K, E, (H, W), mode=mode, want="both"))
    torch.cuda.synchronize()
    for k, (f32, st, n4, f64) in enumerate(res):
        _bits_equal(f32.cpu().numpy(), ref[0], "call %d out_f32" % k)
        _bits_equal(f64.cpu().numpy(), ref[1], "call %d out_f64" % k)
        assert np.array_equal(st.cpu().numpy(), ref[2]) and np.array_equal(n4.cpu().numpy(), ref[3]), k
    # through the ABI on a stream of its own, in guarded buffers
    _check(pkg._lib.load(), pts, n, K, E, H, W, MODES[mode], "second stream " + mode, ref=ref, stream=streams[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_map_points_on_image_is_the_reference_function(pkg, dev):
    rng = np.random.default_rng(6)
    K, E = _small_calibration(1)
    H, W = SMALL_HW
    p = _cloud_on(rng, 700, K[0], E[0], wrap=True, behind=0.2)
    got = pkg.map_points_on_image(p.astype(np.float64), K[0], E[0], hw=(H, W))  # float64 that float32 holds, as get_all_points gives
    ref = R.project_frame(p, K[0], E[0], H, W, R.REFERENCE)
    assert ref[1] == 0 and got.dtype == np.float64
    _bits_equal(got, ref[0], "map_points_on_image")
    # numpy's own in-order assignment, the reference's last three lines, on the statement's z, u, v
    z, u, v = R.ordered_form(p, K[0], E[0])
    depth_map = np.zeros((H, W))
    depth_map[v.astype(int), u.astype(int)] = z
    _bits_equal(got, depth_map, "depth_map[v, u] = z")
    assert not pkg.map_points_on_image(np.zeros((0, 3)), K[0], E[0], hw=(H, W)).any()  # no point: the reference returns zeros
    with pytest.raises(IndexError):
        pkg.map_points_on_image(np.array([[1.0, 50.0, 0.0]], np.float32), K[0], E[0], hw=(H, W))  # far to the left
    with pytest.raises(IndexError):
        pkg.map_points_on_image(np.array([[0.0, 0.0, 0.0]], np.float32), np.eye(3), np.eye(4))  # z = 0: u is NaN
    assert pkg.map_points_on_image(np.array([[3.0, 2.0, 1.0]]), np.eye(3), np.eye(4))[2, 3] == 1.0  # 352 x 1216 by default


def test_project_points_batch(pkg, dev, sweeps):
    clouds, pts, n, K, E, ref = sweeps
    frames, counts = pkg.project_points(clouds, K, E)
    assert frames.shape == (2, 352, 1216) and counts.dtype == np.int32
    _bits_equal(frames, ref[0], "project_points")
    assert np.array_equal(counts, ref[3])
    keep = frames.copy()
    # a second call: arrays of its own; three-column clouds, an empty one, min_z, one calibration for all
    three = [clouds[1][:, :3], np.zeros((0, 3), np.float32), clouds[0][:5000].astype(np.float64)]
    f2, c2 = pkg.project_points(three, K[0], E[0], min_z=5.0)
    p3, n3 = _padded(three, 3)
    r2 = R.project(p3, n3, K[0], E[0], 352, 1216, R.ZBUFFER, 5.0)
    _bits_equal(f2, r2[0], "three columns, min_z 5")
    assert np.array_equal(c2, r2[3]) and not c2[1].any() and not np.shares_memory(frames, f2)
    _bits_equal(frames, keep, "the first result after the second call")
    with pytest.raises(IndexError):
        pkg.project_points(clouds, K, E, mode="reference")


def _good():
    import torch

    return dict(points=torch.zeros((2, 5, 4), device=DEV), counts=[5, 3], K=np.eye(3), E=np.eye(4), hw=(4, 6))


def _spoilt(**changes):
    kw = _good()
    kw.update({k: v(kw[k]) if callable(v) else v for k, v in changes.items()})
    return kw


BAD_CALLS = {  # id -> (the spoilt arguments, the words the ValueError must hold): one bad call per row, nothing is launched
    "points-dtype": (lambda: _spoilt(points=lambda t: t.double()), "points must"),
    "points-rank": (lambda: _spoilt(points=lambda t: t[0]), "points must"),
    "points-strided": (lambda: _spoilt(points=lambda t: t.repeat(1, 1, 2)[..., ::2]), "points must"),
    "points-host": (lambda: _spoilt(points=lambda t: t.cpu()), "points must"),
    "points-stride-5": (lambda: _spoilt(points=lambda t: t.repeat(1, 1, 2)[..., :5].contiguous()), "3 or 4 floats"),
    "counts-shape": (lambda: _spoilt(counts=[5, 3, 1]), "counts must be [B]"),
    "counts-rank": (lambda: _spoilt(counts=[[5, 3]]), "counts must be [B]"),
    "K-shape": (lambda: _spoilt(K=np.eye(4)), "K must be"),
    "E-batch": (lambda: _spoilt(E=np.zeros((3, 4, 4))), "E must be"),
    "hw-zero": (lambda: _spoilt(hw=(0, 6)), "hw must"),
    "hw-fraction": (lambda: _spoilt(hw=(4.5, 6)), "hw must"),
    "hw-one-number": (lambda: _spoilt(hw=6), "hw must"),
    "mode": (lambda: _spoilt(mode="painter"), "mode must"),
    "want": (lambda: _spoilt(want="float16"), "want must"),
    "min_z-negative": (lambda: _spoilt(min_z=-0.5), "min_z must"),
    "min_z-inf": (lambda: _spoilt(min_z=float("inf")), "min_z must"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_bad_call_raises_and_names_the_argument(dev, name):
    make, word = BAD_CALLS[name]
    with pytest.raises(ValueError) as e:
        dev.project_points_device(**make())
    assert word in str(e.value), "%s does not name %r" % (e.value, word)


def test_the_device_function_is_reachable_under_its_names(pkg, dev):
    proj = importlib.import_module(pkg.__name__ + ".projection")
    assert dev.project_points_device is proj.project_points_device is pkg.project_points_device
    out = dev.project_points_device(**_good())
    assert len(out) == 3 and out[0].shape == (2, 4, 6) and out[2].shape == (2, 4)
    assert len(dev.project_points_device(**_good(), want="float64")) == 4

"""Synthetic inputs of the shapes and sparsity patterns the reference's loaders produce.

There is no dataset in the container, so bench.py and the tests draw frames from these generators
(definitions fixed in SURVEY.md section 8d):
  kitti_iid       352x1216, Bernoulli(p) valid mask, depths on KITTI's k/256 grid in [1,80] m
                  (data_read.py:81-99: uint16 PNG / 256)
  kitti_scanline  rows 0..99 empty, valid pixels only on every 4th row (Velodyne-like rings)
  nyu_pattern     the reference's own sampling: Mask[randint(H-12,n)+6, randint(W-16,n)+8] = 1
                  (data_read.py:360-364), n = 200 by default (eval_NYU.py:40)
  iid             generic HxW Bernoulli mask, depths U(lo,hi)
All return float32 [B,H,W] with zeros at invalid pixels.
  nyu_dense       a stored NYU sample before the loader: dense float32 depth [B,480,640] (planes and boxes, 0.5-10 m) and a
                  uint8 image [B,3,480,640]: the input of nyu_read_device.  Tests and scripts only; not a bench.py config.
  velodyne_points whole 360-degree sweeps of the same kind of scanner as point clouds in the Velodyne frame, float32
                  [n, 4] (x, y, z, reflectance: the layout of a KITTI raw .bin), with K and E: the input of the point
                  projection (project_points_device); most of a sweep lies behind or beside the camera.
  velodyne_scan   a simulated 64-laser spinning scanner projected into the camera, with the calibration that goes with
                  it: (x, K, E).  The input of the scan-line subsampling (line_subsample_device); not a bench.py config.
"""
import numpy as np

KITTI_HW = (352, 1216)
NYU_HW = (480, 640)


def _kitti_depths(rng, shape):
    return (np.round(rng.uniform(1.0, 80.0, size=shape) * 256.0) / 256.0).astype(np.float32)


def kitti_iid(B, p=0.05, seed=0, hw=KITTI_HW):
    rng = np.random.default_rng(seed)
    H, W = hw
    mask = rng.random((B, H, W)) < p
    return np.where(mask, _kitti_depths(rng, (B, H, W)), np.float32(0)).astype(np.float32)


def kitti_scanline(B, seed=0, hw=KITTI_HW, empty_rows=100, row_step=4, p=0.25):
    rng = np.random.default_rng(seed)
    H, W = hw
    mask = rng.random((B, H, W)) < p
    rows = np.zeros(H, bool)
    rows[empty_rows::row_step] = True
    mask &= rows[None, :, None]
    return np.where(mask, _kitti_depths(rng, (B, H, W)), np.float32(0)).astype(np.float32)


def nyu_pattern(B, n=200, seed=0, hw=NYU_HW, lo=1.0, hi=10.0):
    rng = np.random.default_rng(seed)
    H, W = hw
    x = np.zeros((B, H, W), np.float32)
    for b in range(B):
        r = rng.integers(0, H - 12, size=n) + 6
        c = rng.integers(0, W - 16, size=n) + 8
        x[b, r, c] = rng.uniform(lo, hi, size=n).astype(np.float32)
    return x


def nyu_dense(B, seed=0, hw=NYU_HW):
    """A stored NYU sample before the loader: (depth float32 [B, h, w], rgb uint8 [B, 3, h, w], the h5 files' layouts).  The
    depth is dense, 0.5-10 m: a tilted back plane, a floor plane below a horizon, and a few boxes in front of them (sharp
    depth edges for the resize to smear).  The image is shaded from the depth, with a texture per channel, over the whole
    0..255 range.  For the tests and scripts/bench_nyu_read.py: the input of nyu_read_device."""
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = xx / max(w - 1, 1), yy / max(h - 1, 1)
    depth = np.empty((B, h, w), np.float32)
    rgb = np.empty((B, 3, h, w), np.uint8)
    for b in range(B):
        d = rng.uniform(5.0, 10.0) + rng.uniform(-2.0, 2.0) * (u - 0.5) + rng.uniform(-1.0, 1.0) * (v - 0.5)
        horizon = rng.uniform(0.45, 0.7)
        floor = rng.uniform(1.2, 1.8) / np.maximum(v - horizon + 0.05, 1e-3)  # a floor under the camera: nearer lower down
        d = np.where(v > horizon, np.minimum(d, floor), d)
        for _ in range(int(rng.integers(3, 7))):
            y0, x0 = rng.uniform(0.0, 0.8), rng.uniform(0.0, 0.8)
            y1, x1 = y0 + rng.uniform(0.1, 0.4), x0 + rng.uniform(0.05, 0.3)
            box = (v >= y0) & (v < y1) & (u >= x0) & (u < x1)
            d = np.where(box, np.minimum(d, rng.uniform(0.8, 6.0) + 0.3 * (u - x0)), d)
        d = np.clip(d, 0.5, 10.0)
        depth[b] = d.astype(np.float32)
        for c in range(3):
            shade = 1.0 - (d - 0.5) / 9.5  # near is bright
            tex = 0.5 + 0.5 * np.sin(2 * np.pi * (rng.uniform(2, 9) * u + rng.uniform(2, 9) * v + rng.uniform()))
            noise = rng.uniform(-0.05, 0.05, size=(h, w))
            rgb[b, c] = np.clip(np.rint(255.0 * (0.6 * shade + 0.4 * tex + noise)), 0, 255).astype(np.uint8)
    return depth, rgb


def iid(B, H, W, p, seed=0, lo=1.0, hi=80.0):
    rng = np.random.default_rng(seed)
    mask = rng.random((B, H, W)) < p
    vals = rng.uniform(lo, hi, size=(B, H, W)).astype(np.float32)
    return np.where(mask, vals, np.float32(0)).astype(np.float32)


def _rot(rng, sigma_deg):
    """A small random rotation (Rodrigues), angle ~ N(0, sigma) degrees about a random axis."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.normal(0.0, sigma_deg))
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)


def _ray_box(o_dirs, lo, hi):
    """Entry distance of rays from the origin along unit directions [N,3] into the box [lo, hi]; inf where they miss."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = lo[None] / o_dirs
        t2 = hi[None] / o_dirs
    tmin = np.nanmax(np.minimum(t1, t2), axis=1)
    tmax = np.nanmin(np.maximum(t1, t2), axis=1)
    return np.where((tmax >= tmin) & (tmin > 0), tmin, np.inf)


def velodyne_scan(B, seed=0, hw=KITTI_HW, lasers=64, max_range=80.0):
    """B frames of a simulated spinning `lasers`-beam LiDAR (elevations spread over +2 .. -24.9 degrees, 0.08-degree
    azimuth steps across the camera's field of view) in a simple scene -- a ground plane 1.73 m below the sensor, a wall
    on either side, a few boxes, returns up to max_range -- projected into a KITTI-like camera with the nearest return kept
    per pixel and depths rounded to the k/256 grid.  Each frame has its own scene and its own slightly jittered
    calibration.  Returns (x float32 [B,H,W], K float64 [B,3,3] intrinsics, E float64 [B,4,4] velo->cam extrinsics).
    Deterministic for a given seed."""
    rng = np.random.default_rng(seed)
    H, W = hw
    x = np.zeros((B, H, W), np.float32)
    K = np.zeros((B, 3, 3))
    E = np.zeros((B, 4, 4))
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # velo (x fwd, y left, z up) -> cam (x right, y down, z fwd)
    for b in range(B):
        f = 721.5 * (1.0 + rng.normal(0.0, 0.01))
        K[b] = [[f, 0.0, W * 0.4906 + rng.normal(0.0, 2.0)], [0.0, f * (1.0 + rng.normal(0.0, 0.001)), H * 0.4585 + rng.normal(0.0, 2.0)],
                [0.0, 0.0, 1.0]]
        E[b, :3, :3] = _rot(rng, 0.5) @ perm
        E[b, :3, 3] = np.array([-0.004, -0.076, -0.272]) + rng.normal(0.0, 0.01, 3)
        E[b, 3, 3] = 1.0
        # rays: per-laser elevation with a small calibration offset, azimuth steps with a per-laser phase (ragged rings)
        elev = np.deg2rad(np.linspace(2.0, -24.9, lasers) + rng.normal(0.0, 0.02, lasers))
        half = np.arctan2(W * 0.55, f) + np.deg2rad(3.0)
        az = np.arange(-half, half, np.deg2rad(0.08))
        azl = az[None, :] + rng.uniform(0.0, np.deg2rad(0.08), (lasers, 1))
        el = np.broadcast_to(elev[:, None], azl.shape)
        d = np.stack([np.cos(el) * np.cos(azl), np.cos(el) * np.sin(azl), np.sin(el)], -1).reshape(-1, 3)
        t = np.full(d.shape[0], np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            ground = -1.73 / d[:, 2]
            t = np.where(d[:, 2] < 0, ground, t)
            for side, off in ((1.0, rng.uniform(5.0, 9.0)), (-1.0, rng.uniform(4.0, 8.0))):
                tw = side * off / d[:, 1]
                pw = tw[:, None] * d
                hit = (tw > 0) & (pw[:, 0] > 3.0) & (pw[:, 2] < 2.5)
                t = np.where(hit & (tw < t), tw, t)
        for _ in range(int(rng.integers(2, 6))):
            c = np.array([rng.uniform(6.0, 45.0), rng.uniform(-5.0, 5.0), -1.73])
            size = np.array([rng.uniform(1.5, 4.5), rng.uniform(1.5, 2.0), rng.uniform(1.2, 2.5)])
            tb = _ray_box(d, c - [size[0] / 2, size[1] / 2, 0.0], c + [size[0] / 2, size[1] / 2, size[2]])
            t = np.minimum(t, tb)
        keep = (t <= max_range) & (rng.random(t.shape) > 0.03)  # range cap, a few dropped returns
        p = t[keep, None] * d[keep]
        pc = p @ E[b, :3, :3].T + E[b, :3, 3]
        pc = pc[pc[:, 2] > 0.5]
        u = np.round(K[b, 0, 0] * pc[:, 0] / pc[:, 2] + K[b, 0, 2]).astype(np.int64)
        v = np.round(K[b, 1, 1] * pc[:, 1] / pc[:, 2] + K[b, 1, 2]).astype(np.int64)
        z = pc[:, 2]
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        u, v, z = u[inside], v[inside], z[inside]
        order = np.argsort(-z, kind="stable")  # farthest first: the nearest return of a pixel is written last
        frame = np.zeros(H * W)
        frame[v[order] * W + u[order]] = z[order]
        x[b] = (np.round(frame * 256.0) / 256.0).reshape(H, W).astype(np.float32)
    return x, K, E


def velodyne_points(B, seed=0, hw=KITTI_HW, lasers=64, max_range=80.0, az_step_deg=0.16):
    """B whole sweeps of a simulated spinning `lasers`-beam LiDAR: the full 360 degrees of azimuth in az_step_deg steps, in a
    scene of velodyne_scan's kind (ground plane, a wall on either side, a few boxes, a few dropped returns), as the scanner
    delivers them: ragged point clouds in the Velodyne frame, not projected.  Only about a quarter of a sweep lies in the
    camera's field of view; the rest is behind or beside it.  Returns (clouds: a list of B float32 [n_b, 4] arrays, x, y, z,
    reflectance, in firing order (azimuth-major), K float64 [B,3,3] intrinsics, E float64 [B,4,4] velo->cam extrinsics).
    Deterministic for a given seed; a generator of its own, velodyne_scan's frames do not change with it."""
    rng = np.random.default_rng(seed)
    H, W = hw
    clouds = []
    K = np.zeros((B, 3, 3))
    E = np.zeros((B, 4, 4))
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # velo (x fwd, y left, z up) -> cam (x right, y down, z fwd)
    for b in range(B):
        f = 721.5 * (1.0 + rng.normal(0.0, 0.01))
        K[b] = [[f, 0.0, W * 0.4906 + rng.normal(0.0, 2.0)], [0.0, f * (1.0 + rng.normal(0.0, 0.001)), H * 0.4585 + rng.normal(0.0, 2.0)],
                [0.0, 0.0, 1.0]]
        E[b, :3, :3] = _rot(rng, 0.5) @ perm
        E[b, :3, 3] = np.array([-0.004, -0.076, -0.272]) + rng.normal(0.0, 0.01, 3)
        E[b, 3, 3] = 1.0
        elev = np.deg2rad(np.linspace(2.0, -24.9, lasers) + rng.normal(0.0, 0.02, lasers))
        az = np.arange(-np.pi, np.pi, np.deg2rad(az_step_deg))
        azl = az[:, None] + rng.uniform(0.0, np.deg2rad(az_step_deg), (1, lasers))  # [azimuth, laser]: firing order
        el = np.broadcast_to(elev[None, :], azl.shape)
        d = np.stack([np.cos(el) * np.cos(azl), np.cos(el) * np.sin(azl), np.sin(el)], -1).reshape(-1, 3)
        t = np.full(d.shape[0], np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d[:, 2] < 0, -1.73 / d[:, 2], t)
            for side, off in ((1.0, rng.uniform(5.0, 9.0)), (-1.0, rng.uniform(4.0, 8.0))):
                tw = side * off / d[:, 1]
                hit = (tw > 0) & (tw * d[:, 2] < 2.5)
                t = np.where(hit & (tw < t), tw, t)
        for _ in range(int(rng.integers(2, 6))):
            c = np.array([rng.uniform(6.0, 45.0) * rng.choice([-1.0, 1.0]), rng.uniform(-5.0, 5.0), -1.73])
            size = np.array([rng.uniform(1.5, 4.5), rng.uniform(1.5, 2.0), rng.uniform(1.2, 2.5)])
            t = np.minimum(t, _ray_box(d, c - [size[0] / 2, size[1] / 2, 0.0], c + [size[0] / 2, size[1] / 2, size[2]]))
        keep = (t <= max_range) & (t > 0.9) & (rng.random(t.shape) > 0.03)  # range cap, blind zone, a few dropped returns
        p = t[keep, None] * d[keep]
        refl = rng.uniform(0.0, 1.0, (p.shape[0], 1))
        clouds.append(np.hstack([p, refl]).astype(np.float32))
    return clouds, K, E


# BASELINE.json configs (index = position in BASELINE.json "configs")
CONFIGS = {
    "kitti_b1": dict(gen="kitti_iid", B=1, H=352, W=1216, kwargs=dict(p=0.05, seed=0)),
    "kitti_b32": dict(gen="kitti_iid", B=32, H=352, W=1216, kwargs=dict(p=0.05, seed=0)),
    "kitti_b32_scanline": dict(gen="kitti_scanline", B=32, H=352, W=1216, kwargs=dict(seed=0)),
    "nyu_b64": dict(gen="nyu_pattern", B=64, H=480, W=640, kwargs=dict(n=200, seed=0)),
    "synth2048_b16": dict(gen="iid", B=16, H=2048, W=2048, kwargs=dict(p=0.01, seed=2)),
    # the reference's other real shapes: the KITTI frame as eval_NYU.py:157 feeds it (rows 96: of 352 x 1216 -> 256 x 1216) and
    # NYU after the loader's resize to 240 x 320 (data_read.py:350-352) with the sampling pattern of data_read.py:360-364
    "kitti_crop256": dict(gen="kitti_scanline", B=4, H=256, W=1216, kwargs=dict(seed=3, hw=(256, 1216), empty_rows=4)),
    "nyu_240x320": dict(gen="nyu_pattern", B=4, H=240, W=320, kwargs=dict(n=200, seed=4, hw=(240, 320))),
}


def make(name, B=None, seed=None):
    cfg = CONFIGS[name]
    kw = dict(cfg["kwargs"])
    if seed is not None:
        kw["seed"] = seed
    B = cfg["B"] if B is None else B
    if cfg["gen"] == "kitti_iid":
        return kitti_iid(B, **kw)
    if cfg["gen"] == "kitti_scanline":
        return kitti_scanline(B, **kw)
    if cfg["gen"] == "nyu_pattern":
        return nyu_pattern(B, **kw)
    return iid(B, cfg["H"], cfg["W"], **kw)

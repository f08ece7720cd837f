"""numpy statements of the scan-line subsampling (include/dtfill.h, dtfill_line_subsample), for the tests only.

ref64                 the contract the kernels implement: float64 throughout, np.linalg.inv, the kept pixels keep their
                      input value.  Returns q = (pitch - pmin) / interval of every valid pixel, so that a test can tell the
                      pixels that sit on a bin edge.
ref32_like_reference  the precision of subsample_Lidar_{train,val}.py: calibration read as float32, float32 back-projection,
                      inverses, norm and arcsin, the frame's range and labels in float32; the kept points re-projected in
                      float64 through the float32 calibration and written as the uint16 PNG (* 256, truncated).

Both are written from the contract in include/dtfill.h; the product does not import this file.
"""
import numpy as np

NO_POINTS, BAD_INTERVAL, SINGULAR = 1, 2, 4  # DTFILL_LINES_*


def _frames(x, K, E):
    x = np.asarray(x, np.float32)
    if x.ndim == 2:
        x = x[None]
    B = x.shape[0]
    K = np.broadcast_to(np.asarray(K, np.float64), (B, 3, 3))
    E = np.broadcast_to(np.asarray(E, np.float64), (B, 4, 4))
    return x, K, E


def pitch64(x, Ki, Ei):
    """float64 pitch of every valid pixel of one frame (raster order) in the contract's order of operations."""
    v, u = np.nonzero(x > np.float32(0.1))
    u = u.astype(np.float64)
    v = v.astype(np.float64)
    d = x[x > np.float32(0.1)].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # a +inf depth: NaN pitch, as in numpy
        cx = (Ki[0, 0] * u + Ki[0, 1] * v + Ki[0, 2]) * d
        cy = (Ki[1, 0] * u + Ki[1, 1] * v + Ki[1, 2]) * d
        cz = (Ki[2, 0] * u + Ki[2, 1] * v + Ki[2, 2]) * d
        px = Ei[0, 0] * cx + Ei[0, 1] * cy + Ei[0, 2] * cz + Ei[0, 3]
        py = Ei[1, 0] * cx + Ei[1, 1] * cy + Ei[1, 2] * cz + Ei[1, 3]
        pz = Ei[2, 0] * cx + Ei[2, 1] * cy + Ei[2, 2] * cz + Ei[2, 3]
        return np.arcsin(pz / np.sqrt(px * px + py * py + pz * pz))


def ref64(x, K, E, n_bins=64, keep_every=4):
    """x float32 [B,H,W] (or [H,W]); K [3,3] / [B,3,3]; E [4,4] / [B,4,4].  Returns (out float32 [B,H,W], status int32
    [B], q float64 [B,H,W]: (pitch - pmin) / interval at the valid pixels of the frames without a status bit, NaN
    elsewhere)."""
    x, K, E = _frames(x, K, E)
    B = x.shape[0]
    out = np.zeros_like(x)
    q = np.full(x.shape, np.nan)
    status = np.zeros(B, np.int32)
    for b in range(B):
        valid = x[b] > np.float32(0.1)
        if not valid.any():
            status[b] |= NO_POINTS
        try:
            Ki, Ei = np.linalg.inv(K[b]), np.linalg.inv(E[b])
        except np.linalg.LinAlgError:
            status[b] |= SINGULAR
            continue
        if status[b]:
            continue
        pitch = pitch64(x[b], Ki, Ei)
        pmin, pmax = np.min(pitch), np.max(pitch)
        interval = (pmax - pmin) / n_bins
        if not (interval > 0 and np.isfinite(interval)):
            status[b] |= BAD_INTERVAL
            continue
        qb = (pitch - pmin) / interval
        kept = np.fmod(np.ceil(qb), keep_every) == 0
        q[b][valid] = qb
        ob = out[b]
        ob[valid] = np.where(kept, x[b][valid], np.float32(0))
    return out, status, q


def ref32_like_reference(x, K, E, n_bins=64, keep_every=4):
    """The reference's precision on one frame x [H,W] (float32).  Returns (png uint16 [H,W] -- the depth map * 256
    truncated, as the scripts write it --, kept bool [H,W] -- the pixels whose points the float32 labels keep)."""
    x = np.asarray(x, np.float32)
    H, W = x.shape
    K32 = np.asarray(K, np.float64).astype(np.float32)  # the calibration files are read as float32
    E32 = np.asarray(E, np.float64).astype(np.float32)
    valid = x > np.float32(0.1)
    v, u = np.nonzero(valid)
    pix = np.stack([u, v, np.ones_like(u)]).astype(np.float32)  # [3, N]
    cam = (np.linalg.inv(K32) @ pix) * x[valid][None]  # float32
    hom = np.concatenate([cam, np.ones((1, cam.shape[1]), np.float32)])
    pts = (np.linalg.inv(E32) @ hom)[:3].T  # float32 [N, 3]
    dist = np.linalg.norm(pts, 2, axis=1)
    pitch = np.arcsin(pts[:, 2] / dist)  # float32
    pmax, pmin = np.max(pitch), np.min(pitch)
    interval = np.float32((pmax - pmin) / np.float32(n_bins))
    label = np.ceil((pitch - pmin) / interval)
    keep = np.fmod(label, np.float32(keep_every)) == 0
    kept = np.zeros((H, W), bool)
    kept[v[keep], u[keep]] = True
    # map_points_on_image: float64 re-projection through the float32 calibration, last write wins
    left = np.hstack([pts[keep].astype(np.float64), np.ones((int(keep.sum()), 1))])
    img = E32.astype(np.float64) @ left.T
    img = K32.astype(np.float64) @ img[:3]
    z = img[2]
    uu = np.round(img[0] / z).astype(np.int64)
    vv = np.round(img[1] / z).astype(np.int64)
    depth = np.zeros((H, W))
    ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
    depth[vv[ok], uu[ok]] = z[ok]
    return (depth * 256.0).astype(np.uint16), kept

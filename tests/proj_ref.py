"""numpy statements of the LiDAR point projection (include/dtfill.h, dtfill_project_points), for the tests only.

ordered_form   z, u, v of every point in the contract's order of operations: float64, one rounding per operation, left to right.
dot_form       what the reference's expression evaluates: hstack a one, np.dot through BLAS twice.  Its sums may run in another
               order or fused, so z may differ in the last bits; the tests bound that and hold u, v equal.
project        both modes of the contract over a ragged batch: the two outputs, the status bits and the counts.

Written from the contract in include/dtfill.h; the product does not import this file.
"""
import numpy as np

REFERENCE, ZBUFFER = 0, 1  # DTFILL_PROJ_* modes
NO_POINTS, INDEX_ERROR, BAD_COUNT = 1, 2, 4  # DTFILL_PROJ_* status bits
PIXELS, INSIDE, BEHIND, OUTSIDE = 0, 1, 2, 3  # frame_counts columns

_QUIET = dict(invalid="ignore", divide="ignore", over="ignore")


def ordered_form(pts, K, E):
    """pts float32 [n, 3|4]; K [3,3]; E [4,4] -> (z, u, v) float64 [n]; u, v rounded half to even, not yet integers."""
    K = np.asarray(K, np.float64)
    E = np.asarray(E, np.float64)
    with np.errstate(**_QUIET):  # (a signalling NaN in a record is legal input: the cast quiets it)
        X, Y, Z = (np.asarray(pts, np.float32)[:, k].astype(np.float64) for k in range(3))
        c = [E[r, 0] * X + E[r, 1] * Y + E[r, 2] * Z + E[r, 3] for r in range(3)]
        h = [K[r, 0] * c[0] + K[r, 1] * c[1] + K[r, 2] * c[2] for r in range(3)]
        z = h[2]
        return z, np.round(h[0] / z), np.round(h[1] / z)


def dot_form(pts, K, E):
    """The same through map_points_on_image's expression: np.dot(K, np.dot(E, [pts 1]^T)[:3])."""
    with np.errstate(**_QUIET):
        p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
        left = np.hstack((p, np.ones((p.shape[0], 1))))
        hom = np.dot(np.asarray(K, np.float64), np.dot(np.asarray(E, np.float64), np.transpose(left))[:3, :])
        z = hom[2, :]
        return z, np.round(hom[0, :] / z), np.round(hom[1, :] / z)


def _fin(a):
    return np.isfinite(a)


def project_frame(pts, K, E, H, W, mode, min_z=0.0):
    """One frame's n points [n, 3|4] -> (out64 float64 [H,W], status, counts int [4])."""
    out = np.zeros(H * W)
    cnt = np.zeros(4, np.int64)
    n = len(pts)
    z, u, v = ordered_form(pts, K, E) if n else (np.zeros(0),) * 3
    if mode == REFERENCE:
        ok = _fin(u) & _fin(v) & (u >= -W) & (u < W) & (v >= -H) & (v < H)
        if not ok.all():
            return out.reshape(H, W), INDEX_ERROR, cnt
        ui, vi = u.astype(np.int64), v.astype(np.int64)
        ui[ui < 0] += W
        vi[vi < 0] += H
        last = np.zeros(H * W, np.int64)  # 1 + the largest i that landed on the pixel
        np.maximum.at(last, vi * W + ui, np.arange(1, n + 1))
        hit = last > 0
        out[hit] = z[last[hit] - 1]
        cnt[[PIXELS, INSIDE]] = hit.sum(), n
    else:
        with np.errstate(**_QUIET):
            X, Y, Z = (np.asarray(pts, np.float32)[:, k].astype(np.float64) for k in range(3)) if n else (np.zeros(0),) * 3
            front = _fin(X) & _fin(Y) & _fin(Z) & _fin(z) & (z > np.float64(np.float32(min_z)))
            inside = front & _fin(u) & _fin(v) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        zmin = np.full(H * W, np.inf)
        np.minimum.at(zmin, v[inside].astype(np.int64) * W + u[inside].astype(np.int64), z[inside])
        hit = zmin < np.inf
        out[hit] = zmin[hit]
        cnt[:] = hit.sum(), inside.sum(), n - front.sum(), (front & ~inside).sum()
    return out.reshape(H, W), 0 if cnt[INSIDE] else NO_POINTS, cnt


def project(points, counts, K, E, H, W, mode, min_z=0.0):
    """points float32 [B, N, 3|4]; counts int [B] or None; K [3,3] / [B,3,3]; E [4,4] / [B,4,4] -> (out32 float32 [B,H,W], out64
    float64 [B,H,W], status int32 [B], counts int32 [B,4]).  The records beyond counts[b] are not looked at."""
    points = np.asarray(points, np.float32)
    B, N = points.shape[:2]
    K = np.broadcast_to(np.asarray(K, np.float64), (B, 3, 3))
    E = np.broadcast_to(np.asarray(E, np.float64), (B, 4, 4))
    out64 = np.zeros((B, H, W))
    status = np.zeros(B, np.int32)
    cnt = np.zeros((B, 4), np.int32)
    for b in range(B):
        n = N if counts is None else int(counts[b])
        if n < 0 or n > N:
            status[b] = BAD_COUNT
            continue
        out64[b], status[b], cnt[b] = project_frame(points[b, :n], K[b], E[b], H, W, mode, min_z)
    with np.errstate(over="ignore"):
        return out64.astype(np.float32), out64, status, cnt

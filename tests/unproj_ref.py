"""numpy statements of the back-projection and its backward (include/dtfill.h, dtfill_unproject, dtfill_unproject_backward), for
the tests only.

forward       the contract literally, frame by frame: validity, the point and its pitch in float64 in the contract's order of
              operations (the pitch is lines_ref.pitch64's expression, the inverses np.linalg.inv as in lines_ref.ref64), the
              selection, raster order, capacity, counts and status.
expected      the forward laid out in the caller's buffers: what was there stays beyond n_b.
backward      the contract's backward in numpy float64; backward_py the same for one record in Python floats.
exact_calibration   K and E whose inverses are exact in any order of operations (powers of two, a signed permutation, dyadic
              offsets): the device's Gauss-Jordan and np.linalg.inv then hold the same bits, so the points compare bit for bit.

Written from the contract in include/dtfill.h; the product does not import this file.
"""
import numpy as np

import lines_ref

NO_POINTS, BAD_INTERVAL, SINGULAR, OVERFLOW, BAD_PIXEL, BAD_COUNT = 1, 2, 4, 8, 16, 32  # DTFILL_UNPROJ_*
WRITTEN, TOTAL = 0, 1  # counts columns

_QUIET = dict(invalid="ignore", divide="ignore", over="ignore")


def exact_calibration(B=1, fx=512.0, fy=256.0, cx=3.5, cy=2.25):
    """(K [B,3,3], E [B,4,4]): focal lengths powers of two, dyadic principal point, E a signed axis permutation (velo x forward,
    y left, z up -> cam z, -x, -y) with dyadic translations; frame b's translation differs by b / 8."""
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    E = np.array([[0, -1, 0, 0.25], [0, 0, -1, -0.125], [1, 0, 0, -0.5], [0, 0, 0, 1]], np.float64)
    Ks = np.repeat(K[None], B, 0)
    Es = np.repeat(E[None], B, 0)
    Es[:, 0, 3] += np.arange(B) / 8.0
    return Ks, Es


def _frames(x, K, E):
    return lines_ref._frames(x, K, E)


def points64(x, Ki, Ei, val_thr=0.1):
    """(valid bool [H,W], px, py, pz float64 [n]) of one frame, raster order, in the contract's order of operations."""
    valid = x > np.float32(val_thr)
    v, u = np.nonzero(valid)
    u = u.astype(np.float64)
    v = v.astype(np.float64)
    d = x[valid].astype(np.float64)
    with np.errstate(**_QUIET):
        cx = (Ki[0, 0] * u + Ki[0, 1] * v + Ki[0, 2]) * d
        cy = (Ki[1, 0] * u + Ki[1, 1] * v + Ki[1, 2]) * d
        cz = (Ki[2, 0] * u + Ki[2, 1] * v + Ki[2, 2]) * d
        px = Ei[0, 0] * cx + Ei[0, 1] * cy + Ei[0, 2] * cz + Ei[0, 3]
        py = Ei[1, 0] * cx + Ei[1, 1] * cy + Ei[1, 2] * cz + Ei[1, 3]
        pz = Ei[2, 0] * cx + Ei[2, 1] * cy + Ei[2, 2] * cz + Ei[2, 3]
    return valid, px, py, pz


def pitch_of(px, py, pz):
    """lines_ref.pitch64's last line on points64's result."""
    with np.errstate(**_QUIET):
        return np.arcsin(pz / np.sqrt(px * px + py * py + pz * pz))


def forward(x, K, E, val_thr=0.1, payload=None, n_bins=64, keep_every=0, N=None, stride=3):
    """x float32 [B,H,W] (or [H,W]).  Returns a dict: points (list of float32 [n_b, stride]), pitch (list of float64 [n_b]),
    pixel (list of int32 [n_b]), counts int32 [B,2], status int32 [B]; n_b = min(total_b, N), N = H*W by default."""
    x, K, E = _frames(x, K, E)
    B, H, W = x.shape
    N = H * W if N is None else N
    pay = None if payload is None else np.asarray(payload, np.float32).reshape(x.shape)
    res = dict(points=[], pitch=[], pixel=[], counts=np.zeros((B, 2), np.int32), status=np.zeros(B, np.int32))
    for b in range(B):
        empty = (np.zeros((0, stride), np.float32), np.zeros(0), np.zeros(0, np.int32))
        st = 0
        if not (x[b] > np.float32(val_thr)).any():
            st |= NO_POINTS
        try:
            Ki, Ei = np.linalg.inv(K[b]), np.linalg.inv(E[b])
        except np.linalg.LinAlgError:
            st |= SINGULAR
        rec = empty
        if st == 0:
            valid, px, py, pz = points64(x[b], Ki, Ei, val_thr)
            pitch = pitch_of(px, py, pz)
            sel = np.ones(pitch.shape, bool)
            if keep_every >= 1:
                pmin, pmax = np.min(pitch), np.max(pitch)
                with np.errstate(**_QUIET):
                    interval = (pmax - pmin) / n_bins
                    if not (interval > 0 and np.isfinite(interval)):
                        st |= BAD_INTERVAL
                        sel[:] = False
                    else:
                        sel = np.fmod(np.ceil((pitch - pmin) / interval), keep_every) == 0
            pix = np.flatnonzero(valid.reshape(-1))[sel].astype(np.int32)
            with np.errstate(over="ignore"):
                pts = np.zeros((pix.size, stride), np.float32)
                pts[:, 0], pts[:, 1], pts[:, 2] = px[sel].astype(np.float32), py[sel].astype(np.float32), pz[sel].astype(np.float32)
            if stride == 4 and pay is not None:
                pts.view(np.uint32)[:, 3] = pay[b].reshape(-1).view(np.uint32)[pix]
            rec = (pts, pitch[sel], pix)
        total = rec[2].size
        if total > N:
            st |= OVERFLOW
        n = min(total, N)
        res["points"].append(rec[0][:n])
        res["pitch"].append(rec[1][:n])
        res["pixel"].append(rec[2][:n])
        res["counts"][b] = n, total
        res["status"][b] = st
    return res


def expected(res, points0, pitch0=None, pixel0=None):
    """The buffers after the call: copies of the caller's points0 [B,N,stride] (pitch0 [B,N], pixel0 [B,N]) with the first n_b
    records of every frame replaced by res's."""
    out = [points0.copy(), None if pitch0 is None else pitch0.copy(), None if pixel0 is None else pixel0.copy()]
    for b in range(points0.shape[0]):
        n = int(res["counts"][b, WRITTEN])
        out[0][b, :n] = res["points"][b]
        if out[1] is not None:
            out[1][b, :n] = res["pitch"][b]
        if out[2] is not None:
            out[2][b, :n] = res["pixel"][b]
    return out


def jacobian64(pix, Ki, Ei, W):
    """j_r of the contract for flat pixels pix: float64 [3, n]."""
    pix = np.asarray(pix, np.int64)
    u = (pix % W).astype(np.float64)
    v = (pix // W).astype(np.float64)
    k = [Ki[r, 0] * u + Ki[r, 1] * v + Ki[r, 2] for r in range(3)]
    return np.stack([Ei[r, 0] * k[0] + Ei[r, 1] * k[1] + Ei[r, 2] * k[2] for r in range(3)])


def backward(grad_points, pixel, counts, K, E, H, W, want_payload=False, rounded=True):
    """grad_points float32 [B,N,stride]; pixel int32 [B,N]; counts int32 [B,2].  Returns (grad_x [B,H,W], grad_payload [B,H,W] or
    None, status int32 [B]); grad_x is float32, or with rounded=False the float64 sum before the final conversion."""
    g = np.asarray(grad_points, np.float32)
    B, N, stride = g.shape
    K = np.broadcast_to(np.asarray(K, np.float64), (B, 3, 3))
    E = np.broadcast_to(np.asarray(E, np.float64), (B, 4, 4))
    gx = np.zeros((B, H * W), np.float64)
    gp = np.zeros((B, H * W), np.float32) if want_payload else None
    status = np.zeros(B, np.int32)
    for b in range(B):
        n = int(counts[b, WRITTEN])
        if n < 0 or n > N:
            status[b] |= BAD_COUNT
        else:
            p = np.asarray(pixel[b, :n], np.int64)
            if ((p < 0) | (p >= H * W)).any() or (np.diff(p) <= 0).any():
                status[b] |= BAD_PIXEL
        try:
            Ki, Ei = np.linalg.inv(K[b]), np.linalg.inv(E[b])
        except np.linalg.LinAlgError:
            status[b] |= SINGULAR
        if status[b]:
            continue
        j = jacobian64(p, Ki, Ei, W)
        gd = g[b, :n, :3].astype(np.float64)
        with np.errstate(**_QUIET):
            gx[b, p] = gd[:, 0] * j[0] + gd[:, 1] * j[1] + gd[:, 2] * j[2]
        if gp is not None and stride == 4:
            gp[b].view(np.uint32)[p] = g[b, :n, 3].view(np.uint32)
    with np.errstate(over="ignore"):
        gx = gx.astype(np.float32) if rounded else gx
    return gx.reshape(B, H, W), None if gp is None else gp.reshape(B, H, W), status


def backward_py(g3, pix, Ki, Ei, W):
    """One record's gradient with respect to its pixel's depth in Python floats, left to right: the double before (float)."""
    u, v = float(pix % W), float(pix // W)
    k = [float(Ki[r][0]) * u + float(Ki[r][1]) * v + float(Ki[r][2]) for r in range(3)]
    j = [float(Ei[r][0]) * k[0] + float(Ei[r][1]) * k[1] + float(Ei[r][2]) * k[2] for r in range(3)]
    return float(g3[0]) * j[0] + float(g3[1]) * j[1] + float(g3[2]) * j[2]

"""Label -> source pixel, stated literally in numpy (helpers only: no tests, no fixtures).

Written from include/dtfill.h (dtfill_nearest_gather, dtfill_nearest_gather_backward):
    src = ~((1 - x) > src_thr) in float32;  pix = flatnonzero(src);  m = len(pix)
    1 <= L <= m:       pixel = pix[L - 1], filled[c] = values[c].flat[pix[L - 1]]
    L == 0:            pixel = -1, filled = +0.0
    L < 0 or L > m:    pixel = -1, filled = +0.0, the frame's status carries INDEX_ERROR
    status = (m == 0 ? NO_SOURCE : 0) | (a bad label ? INDEX_ERROR : 0)
The backward sends grad_out[c][p] to source L - 1 of every pixel with 1 <= L <= m; the sum of a cell is the cell sum of
tests/fill_grad_ref.py (the header's S), imported from there.
"""
import numpy as np

from fill_grad_ref import cell_bound, cell_sum  # noqa: F401  (cell_bound: for the tests that import this module)

F = np.float32
INDEX_ERROR = 1  # DTFILL_FRAME_INDEX_ERROR
NO_SOURCE = 4  # DTFILL_FRAME_NO_SOURCE
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def source_pixels(x, src_thr=0.1):
    """One frame: the flat pixels of the source list, in raster order."""
    with np.errstate(invalid="ignore"):
        src = ~((F(1) - np.asarray(x, F)) > F(src_thr))
    return np.flatnonzero(src.reshape(-1))


def frame_ranks(x, index, src_thr=0.1):
    """One frame: (pix, k int64 flat with L - 1 where 1 <= L <= m and -1 elsewhere, status)."""
    pix = source_pixels(x, src_thr)
    m = pix.size
    L = np.asarray(index, np.int32).reshape(-1).astype(np.int64)
    ok = (L >= 1) & (L <= m)
    bad = ~ok & (L != 0)
    status = (NO_SOURCE if m == 0 else 0) | (INDEX_ERROR if bad.any() else 0)
    return pix, np.where(ok, L - 1, -1), status


def gather(x, index, values=None, src_thr=0.1):
    """dtfill_nearest_gather on numpy arrays: x float32 [B,H,W], index int32 [B,H,W], values None or float32 [B,C,H,W].
    Returns (filled float32 [B,C,H,W] or None, pixel int32 [B,H,W], status int32 [B]); the payload moves as bits."""
    x = np.asarray(x, F)
    B, H, W = x.shape
    pixel = np.full((B, H * W), -1, np.int32)
    status = np.zeros(B, np.int32)
    filled = None
    if values is not None:
        vbits = np.ascontiguousarray(values, F).view(np.uint32).reshape(B, -1, H * W)
        fbits = np.zeros(vbits.shape, np.uint32)
    for b in range(B):
        pix, k, status[b] = frame_ranks(x[b], index[b], src_thr)
        hit = k >= 0
        pixel[b, hit] = pix[k[hit]]
        if values is not None:
            fbits[b][:, hit] = vbits[b][:, pix[k[hit]]]
    if values is not None:
        filled = fbits.view(F).reshape(np.shape(values))
    return filled, pixel.reshape(B, H, W), status


def backward(x, index, grad_out, src_thr=0.1):
    """dtfill_nearest_gather_backward on numpy arrays: grad_out float32 [B,C,H,W] -> (grad_values float32 [B,C,H,W], status)."""
    x, grad_out = np.asarray(x, F), np.asarray(grad_out, F)
    B, C = grad_out.shape[:2]
    grad_values = np.zeros(grad_out.shape, F)
    status = np.zeros(B, np.int32)
    for b in range(B):
        pix, k, status[b] = frame_ranks(x[b], index[b], src_thr)
        order = np.argsort(k, kind="stable")
        order = order[k[order] >= 0]
        if order.size == 0:
            continue
        cuts = np.flatnonzero(np.diff(k[order])) + 1
        for cell in np.split(order, cuts):
            for c in range(C):
                grad_values[b, c].reshape(-1)[pix[k[cell[0]]]] = cell_sum(grad_out[b, c].reshape(-1)[cell])
    return grad_values, status


def hand_cases():
    """name -> (x [H,W], index [H,W], values [H,W], pixel [H,W], filled [H,W], status, grad_values [H,W] for grad_out = 1 + the
    flat pixel number): expected outputs written down by hand from the contract, not computed by the functions above.  The
    first frame is 5 x 7, the others HAND_HW = 4 x 6."""
    cases = {}
    # sources (0,5) = 10, (2,1) = 20, (4,4) = 30, the printed labels of the l1_cv transform
    x = np.zeros((5, 7), F)
    x[0, 5], x[2, 1], x[4, 4] = 10, 20, 30
    lbl = np.array([[2, 2, 2, 1, 1, 1, 1], [2, 2, 2, 1, 1, 1, 1], [2, 2, 2, 2, 3, 1, 1], [2, 2, 2, 3, 3, 3, 3], [2, 2, 3, 3, 3, 3, 3]],
                   np.int32)
    vals = np.arange(100, 135, dtype=F).reshape(5, 7)  # values[p] = 100 + p
    at = {1: 5, 2: 15, 3: 32}
    pixel = np.array([[at[int(v)] for v in row] for row in lbl], np.int32)
    g = np.zeros((5, 7), F)
    # cells, by hand from the printed labels: label 1 owns pixels 3-6, 10-13, 19, 20; label 3 owns 18, 24-27, 30-34; the rest 2
    one = [3, 4, 5, 6, 10, 11, 12, 13, 19, 20]
    three = [18, 24, 25, 26, 27, 30, 31, 32, 33, 34]
    two = [p for p in range(35) if p not in one and p not in three]
    g.reshape(-1)[[5, 15, 32]] = [sum(p + 1 for p in cell) for cell in (one, two, three)]
    cases["survey 8c"] = (x, lbl, vals, pixel, (pixel + 100).astype(F), 0, g)

    H, W = 4, 6
    N = H * W
    vals = np.arange(100, 100 + N, dtype=F).reshape(H, W)
    # planted labels: sources at pixels 3 and 14 (m = 2); columns 0-3 read label 1, columns 4-5 label 2, then pixels 0, 7, 8,
    # 16 and 23 get 0, -1, m + 1, INT32_MIN and INT32_MAX
    x = np.zeros(N, F)
    x[[3, 14]] = (5.0, 7.0)
    lbl = np.where(np.arange(N) % W < 4, 1, 2).astype(np.int64)
    lbl[[0, 7, 8, 16, 23]] = (0, -1, 3, I32_MIN, I32_MAX)
    pixel = np.where(np.arange(N) % W < 4, 3, 14).astype(np.int32)
    pixel[[0, 7, 8, 16, 23]] = -1
    filled = np.where(pixel >= 0, pixel + 100, 0).astype(F)
    g = np.zeros(N, F)
    # label 1: columns 0-3 of four rows = pixels {0,1,2,3, 6,7,8,9, 12,13,14,15, 18,19,20,21} without 0, 7, 8 (16 is in column 4)
    g[3] = sum(p + 1 for p in (1, 2, 3, 6, 9, 12, 13, 14, 15, 18, 19, 20, 21))
    # label 2: columns 4-5 = pixels {4,5, 10,11, 16,17, 22,23} without 16 and 23
    g[14] = sum(p + 1 for p in (4, 5, 10, 11, 17, 22))
    cases["planted labels"] = (x.reshape(H, W), lbl.astype(np.int32).reshape(H, W), vals, pixel.reshape(H, W), filled.reshape(H, W),
                               INDEX_ERROR, g.reshape(H, W))
    # all zero: no source, the transform's label 0 everywhere
    z = np.zeros((H, W), F)
    cases["all zero"] = (z, np.zeros((H, W), np.int32), vals, np.full((H, W), -1, np.int32), z, NO_SOURCE, z)
    # a valued pixel that is no source (0.5 at pixel 0): never read, and it receives +0.0; the one source is pixel 9
    x = np.zeros(N, F)
    x[[0, 9]] = (0.5, 6.0)
    g = np.zeros(N, F)
    g[9] = N * (N + 1) // 2
    cases["a valued pixel that is no source"] = (x.reshape(H, W), np.ones((H, W), np.int32), vals, np.full((H, W), 9, np.int32),
                                                 np.full((H, W), 109, F), 0, g.reshape(H, W))
    return cases


def hand_grad(shape):
    """The upstream gradient of the hand cases: 1 + the flat pixel number."""
    return np.arange(1, 1 + int(np.prod(shape)), dtype=F).reshape(shape)

"""Hand cases of the LiDAR point projection (include/dtfill.h, dtfill_project_points) on 5 x 7 frames, shared by the CPU tests
(which hold tests/proj_ref.py to the values written here by hand) and the GPU tests (which hold the kernels to proj_ref).

With K = I and E = I a point (X, Y, Z) has z = Z, u = rint(X / Z), v = rint(Y / Z); with Z = 1 the pixel is (rint(Y), rint(X)).
A case: name -> dict(pts float32 [n, 3], K, E, ref=(status, {(v, u): z}) expected in REFERENCE mode, zbuf=(status, {(v, u): z},
(inside, behind, outside)) expected in ZBUFFER mode with min_z = 0).
"""
import itertools

import numpy as np

H, W = 5, 7
NO_POINTS, INDEX_ERROR, BAD_COUNT = 1, 2, 4
I3, I4 = np.eye(3), np.eye(4)
INF, NAN = np.inf, np.nan
K_HUGE = np.diag([1.0, 1.0, 1e308])  # z = 1e308 * Z overflows to +-inf for |Z| = 10 while u = rint(X / inf) = 0 stays finite


def _case(pts, ref, zbuf, K=I3, E=I4):
    return dict(pts=np.asarray(pts, np.float32).reshape(-1, 3), K=K, E=E, ref=ref, zbuf=zbuf)


def cases():
    c = {}
    # round half to even: columns 0.5, 1.5, 2.5 -> 0, 2, 2; rows 0.5, 3.5 -> 0, 4
    c["half_to_even"] = _case([[0.5, 0.5, 1], [1.5, 0, 1], [2.5, 3.5, 1]],
                              (0, {(0, 0): 1.0, (0, 2): 1.0, (4, 2): 1.0}), (0, {(0, 0): 1.0, (0, 2): 1.0, (4, 2): 1.0}, (3, 0, 0)))
    # three points of pixel (2, 3) at depths 1, 2, 3 in all six orders: the last writer against the nearest
    for order in itertools.permutations((1.0, 2.0, 3.0)):
        c["one_pixel_%d%d%d" % order] = _case([[3 * z, 2 * z, z] for z in order], (0, {(2, 3): order[-1]}),
                                              (0, {(2, 3): 1.0}, (3, 0, 0)))
    # negative indices wrap in REFERENCE (u = -1 -> W - 1, v = -H -> 0), and are outside in ZBUFFER
    c["negative_wrap"] = _case([[-1, 1, 1], [2, -5, 1], [-7, -1, 1]], (0, {(1, 6): 1.0, (0, 2): 1.0, (4, 0): 1.0}),
                               (NO_POINTS, {}, (0, 0, 3)))
    c["past_the_wrap"] = _case([[1, 1, 1], [-8, 0, 1]], (INDEX_ERROR, {}), (0, {(1, 1): 1.0}, (1, 0, 1)))
    c["row_past_the_wrap"] = _case([[1, 1, 1], [0, -6, 1]], (INDEX_ERROR, {}), (0, {(1, 1): 1.0}, (1, 0, 1)))
    c["column_w"] = _case([[7, 0, 1]], (INDEX_ERROR, {}), (NO_POINTS, {}, (0, 0, 1)))
    # z = 0: u = X / 0 is +-inf or NaN
    c["z_zero"] = _case([[1, 1, 0], [2, 2, 1]], (INDEX_ERROR, {}), (0, {(2, 2): 1.0}, (1, 1, 0)))
    c["z_zero_nan"] = _case([[0, 0, 0]], (INDEX_ERROR, {}), (NO_POINTS, {}, (0, 1, 0)))
    # a negative z is written by REFERENCE (u = -2 / -1 = 2) and behind in ZBUFFER
    c["z_negative"] = _case([[-2, -1, -1], [1, 1, 2]], (0, {(1, 2): -1.0, (0, 0): 2.0}), (0, {(0, 0): 2.0}, (1, 1, 0)))
    # non-finite coordinates: 0 * inf = NaN poisons every sum
    c["inf_coordinate"] = _case([[1, 1, INF], [1, 1, 1]], (INDEX_ERROR, {}), (0, {(1, 1): 1.0}, (1, 1, 0)))
    c["minus_inf_coordinate"] = _case([[-INF, 1, 1], [1, 1, 1]], (INDEX_ERROR, {}), (0, {(1, 1): 1.0}, (1, 1, 0)))
    c["nan_coordinate"] = _case([[1, NAN, 1], [3, 1, 1]], (INDEX_ERROR, {}), (0, {(1, 3): 1.0}, (1, 1, 0)))
    # z overflows to +-inf with finite pixel indices: REFERENCE writes it, ZBUFFER counts it as behind
    c["z_overflow"] = _case([[3, 2, 10], [1, 1, -10]], (0, {(0, 0): -INF}), (NO_POINTS, {}, (0, 2, 0)), K=K_HUGE)
    c["z_overflow_plus"] = _case([[3, 2, 10]], (0, {(0, 0): INF}), (NO_POINTS, {}, (0, 1, 0)), K=K_HUGE)
    # equal z on one pixel: either point gives the same bits
    c["equal_z"] = _case([[4, 6, 2], [3.9, 6.1, 2], [4.1, 5.9, 2]], (0, {(3, 2): 2.0}), (0, {(3, 2): 2.0}, (3, 0, 0)))
    c["empty"] = _case(np.zeros((0, 3)), (NO_POINTS, {}), (NO_POINTS, {}, (0, 0, 0)))
    return c


def expected_frame(pixels):
    out = np.zeros((H, W))
    for (v, u), z in pixels.items():
        out[v, u] = z
    return out


def batch(cs, stride, N=64, poison=True):
    """The cases as one ragged batch: (points float32 [B, N, stride], counts int32 [B], K [B,3,3], E [B,4,4]); the padding records
    and, with stride 4, the 4th floats hold NaN bit patterns when poison is set."""
    B = len(cs)
    pts = np.zeros((B, N, stride), np.float32)
    if poison:
        pts.view(np.uint32)[:] = 0x7FA5A5A5
    counts = np.zeros(B, np.int32)
    K = np.zeros((B, 3, 3))
    E = np.zeros((B, 4, 4))
    for b, c in enumerate(cs):
        n = len(c["pts"])
        pts[b, :n, :3] = c["pts"]
        counts[b], K[b], E[b] = n, c["K"], c["E"]
    return pts, counts, K, E

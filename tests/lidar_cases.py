"""Projected LiDAR frames for the fill tests (tests/test_gpu_lidar.py runs them, tests/test_lidar_frames.py pins what they are).

Every frame here starts from synth.velodyne_scan: a ragged first ring under an empty sky, walls, boxes, dropped returns,
depths on the k/256 grid.  The facts the GPU module relies on (first source row, rows farther than the window kernels reach,
rows an l2 window tile row has to hand on) are computed from the oracle's distance maps, never assumed.
"""
import numpy as np

SEEDS = (17, 23)  # velodyne_scan(B, seed) batches the GPU module fills
B = 6
CROP = 96  # eval_NYU.py:157 feeds rows 96: of the 352 x 1216 frame (256 x 1216)
REACH = 32  # the largest halo of a window kernel: a pixel farther than this from every source is no window's
L2_ROW_T = 152  # w2_row_t(1216): a row with this many far pixels is handed from k_l2win to k_l2env
SKY_MIN, SKY_MAX = 9, 320  # dtfill_common.hpp: first source rows whose sky k_sky can take
F32_MIN = np.float32(np.finfo(np.float32).tiny)

# (src_thr, val_thr) pairs the planted frames run under: tools.py's (0.1, 0.1), eval_NYU.py's (0.001, 0.1), and (0.1, 0.6),
# where NaN sources outnumber the values and the gather runs off the end of the value list (IndexError frames)
THRESHOLDS = ((0.1, 0.1), (0.001, 0.1), (0.1, 0.6))
# ... and degenerate ones the CPU module pins the oracle's glue under
DEGENERATE = ((1.0, -1.0), (float("nan"), 0.1), (-0.5, float("nan")))


def source_mask(x, st):
    """The reference's source predicate (tools.py:8): a pixel is a source unless (1 - x) > src_thr, in float32."""
    with np.errstate(invalid="ignore"):
        return ~((np.float32(1) - x) > np.float32(st))


def first_source_row(frame, st=0.1):
    rows = np.nonzero(source_mask(frame, st).any(1))[0]
    return int(rows[0]) if rows.size else -1


def rows_beyond(dt, d=REACH):
    """Per frame, the rows holding a pixel farther than d from every source: bool [B, H]."""
    return (dt > d).any(2)


def rows_to_hand_on(dt2, d=REACH, n=L2_ROW_T):
    """l2, per frame: the rows with at least n pixels farther than d from every source -- more far pixels than k_l2win keeps
    on its far list, whatever its radius (<= 15 < d): bool [B, H]."""
    return (dt2 > d).sum(2) >= n


def planted_values():
    """Edge values for the predicates and the gather (float32): name -> value."""
    v = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "negative": np.float32(-3.5),
         "-0.0": np.float32(-0.0), "denormal": np.float32(F32_MIN / 8), "near 0.25": np.float32(0.25),
         "near 0.5": np.float32(0.5), "near 0.9": np.float32(0.9)}
    for thr in (0.1, 0.001):  # 1 - thr in float32 and its neighbours: the source predicate flips between them
        c = np.float32(1) - np.float32(thr)
        v["1-%g" % thr] = c
        v["1-%g-ulp" % thr] = np.nextafter(c, np.float32(0))
        v["1-%g+ulp" % thr] = np.nextafter(c, np.float32(2))
    return v


def plant_sites(frame, dt):
    """Where to plant in one frame (row, column): the sky, row r0, the farthest pixel of the rows below r0, and the empty pixel
    next to the densest cluster of sources (a wall)."""
    H, W = frame.shape
    src = source_mask(frame, 0.1)
    r0 = first_source_row(frame)
    far = np.unravel_index(int(np.argmax(np.where(np.arange(H)[:, None] > r0 + 1, dt, -1))), dt.shape)
    # sources in the 5 x 5 box around every pixel (a box sum over the integral image); the empty pixel with the most
    c = np.pad(np.cumsum(np.cumsum(src.astype(np.int32), 0), 1), ((1, 0), (1, 0)))
    i0, i1 = np.clip(np.arange(H) - 2, 0, H), np.clip(np.arange(H) + 3, 0, H)
    j0, j1 = np.clip(np.arange(W) - 2, 0, W), np.clip(np.arange(W) + 3, 0, W)
    box = c[i1][:, j1] - c[i0][:, j1] - c[i1][:, j0] + c[i0][:, j0]
    wall = np.unravel_index(int(np.argmax(np.where(src, -1, box))), box.shape)
    return {"sky": (r0 // 2, W // 3), "r0": (r0, W // 2 + 7), "far": (int(far[0]), int(far[1])), "wall": (int(wall[0]), int(wall[1]))}


def plant(x, dt):
    """A copy of frames x with the planted values: frame 0 stays as it is; frames 1 .. B-2 get every third value (a different
    third per frame and site) at each of their four sites, 3 columns apart along the site's row; the last frame gets two NaN
    sources (sky, far row) and two 0.5 values (row r0, wall): as many values as sources under val_thr 0.1, two sources too
    many under 0.6."""
    x = x.copy()
    vals = list(planted_values().values())
    last = x.shape[0] - 1
    for b in range(1, x.shape[0]):
        for k, (i, j) in enumerate(plant_sites(x[b], dt[b]).values()):
            pick = [v for n, v in enumerate(vals) if (n + b + k) % 3 == 0]
            if b == last:
                pick = [np.float32(np.nan) if k % 2 == 0 else np.float32(0.5)]
            for n, v in enumerate(pick):
                x[b, i, min(max(j + 3 * (n - len(pick) // 2), 0), x.shape[2] - 1)] = v
    return x


def plant_negatives(x, n=3, seed=0):
    """A copy of x with n negative depths planted in every frame below its first source row (the fused outlier filter then
    takes its exhaustive second launch)."""
    x = x.copy()
    rng = np.random.default_rng(seed)
    H, W = x.shape[1:]
    for b in range(x.shape[0]):
        r0 = first_source_row(x[b])
        x[b, rng.integers(r0, H, n), rng.integers(0, W, n)] = -np.round(rng.uniform(1.0, 40.0, n) * 256) / 256
    return x


def hand_over_band(x, width=300, rows=150):
    """A copy of x with a band `width` columns wide and `rows` high emptied below each frame's first source row, at a
    different column in every frame: its rows hold more far pixels than k_l2win keeps on its list, spread over two or three
    of its tiles."""
    x = x.copy()
    W = x.shape[2]
    for b in range(x.shape[0]):
        r0 = first_source_row(x[b])
        c = (137 + 211 * b) % (W - width)
        x[b, r0:r0 + rows, c:c + width] = 0
    return x

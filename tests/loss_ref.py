"""The literal numpy statement of dtfill_train_loss and dtfill_train_loss_backward (include/dtfill.h): the objective of the
reference's training step, train.py:215-251, and its gradient.  float32 elementwise arithmetic, one rounding per operation; the
sums are math.fsum of the float32 terms taken as float64 (the exact sum, rounded once), the counts are integers.  Helpers only:
no fixtures, no hooks."""
import math

import numpy as np

F = np.float32
KITTI, NYU = 0, 1
# dataset -> (kind, gt_thr, in_thr, rows, cols): train.py:215-216, :244 and :220-221, :242
PRESETS = {"KITTI": (KITTI, 0.1, 0.1, None, None), "NYU": (NYU, 0.0001, 0.001, (6, 228), (8, 304))}
COLUMNS = ("main", "aux", "n_gt", "n_in", "S_main", "S_aux")


def window_mask(shape, rows, cols):
    B, H, W = shape
    r0, r1 = (0, H) if rows is None else rows
    c0, c1 = (0, W) if cols is None else cols
    w = np.zeros(shape, bool)
    w[:, r0:r1, c0:c1] = True
    return w


def masks(gt, lidar, gt_thr, in_thr):
    """m, mi (mi None without lidar): float32 compares, so a NaN is in neither."""
    m = gt > F(gt_thr)
    return m, (None if lidar is None else m & (lidar > F(in_thr)))


def terms(pred, corr, gt):
    """e = (pred - gt)^2 and a = (corr - gt)^2 + |corr - gt| in float32, one rounding per operation (a None without corr)."""
    with np.errstate(all="ignore"):
        t = (pred - gt).astype(F)
        e = (t * t).astype(F)
        if corr is None:
            return e, None
        u = (corr - gt).astype(F)
        return e, ((u * u).astype(F) + np.abs(u)).astype(F)


def forward(pred, gt, lidar=None, corr=None, kind=KITTI, gt_thr=0.1, in_thr=0.1, rows=None, cols=None):
    """float64 [6] = main, aux, n_gt, n_in, S_main, S_aux, and the numbers of terms of the two sums."""
    assert all(a is None or (a.dtype == F and a.shape == pred.shape) for a in (pred, gt, lidar, corr))
    assert (lidar is None) == (corr is None)
    m, mi = masks(gt, lidar, gt_thr, in_thr)
    e, a = terms(pred, corr, gt)
    sel = m & window_mask(pred.shape, rows, cols)  # the sum runs over the window, the count over the frame
    n_gt = int(m.sum())
    S_main = math.fsum(e[sel].astype(np.float64).tolist())
    with np.errstate(all="ignore"):
        q = np.float64(S_main) / np.float64(n_gt)
        main = np.sqrt(q) if kind == NYU else q
        if corr is None:
            aux, n_in, S_aux, nt_aux = 0.0, 0, 0.0, 0
        else:
            n_in = int(mi.sum())
            S_aux = math.fsum(a[mi].astype(np.float64).tolist())
            aux = np.float64(S_aux) / np.float64(n_in)
            nt_aux = n_in
    return np.array([main, aux, n_gt, n_in, S_main, S_aux], np.float64), (int(sel.sum()), nt_aux)


def k_factors(stats, kind, g_main, g_aux):
    """k_main, k_aux: the divisions in double from stats and the float32 scalars g_*, rounded to float32 once."""
    with np.errstate(all="ignore"):
        main, n_gt, n_in = np.float64(stats[0]), np.float64(stats[2]), np.float64(stats[3])
        k_main = k_aux = None
        if g_main is not None:
            g = np.float64(F(g_main))
            k_main = F(g / ((np.float64(2.0) * main) * n_gt)) if kind == NYU else F(g / n_gt)
        if g_aux is not None:
            k_aux = F(np.float64(F(g_aux)) / n_in)
    return k_main, k_aux


def backward(pred, gt, stats, g_main=None, g_aux=None, lidar=None, corr=None, kind=KITTI, gt_thr=0.1, in_thr=0.1, rows=None,
             cols=None):
    """(grad_pred, grad_corr) in float32, grad_corr None without corr; +0 wherever nothing is selected or g_* is None."""
    m, mi = masks(gt, lidar, gt_thr, in_thr)
    k_main, k_aux = k_factors(stats, kind, g_main, g_aux)
    grad_pred = np.zeros(pred.shape, F)
    with np.errstate(all="ignore"):
        if k_main is not None:
            sel = m & window_mask(pred.shape, rows, cols)
            t = (pred - gt).astype(F)
            grad_pred[sel] = ((F(2) * t).astype(F) * k_main).astype(F)[sel]
        if corr is None:
            return grad_pred, None
        grad_corr = np.zeros(pred.shape, F)
        if k_aux is not None:
            u = (corr - gt).astype(F)
            sgn = np.where(u > 0, F(1), np.where(u < 0, F(-1), F(0))).astype(F)
            grad_corr[mi] = (((F(2) * u).astype(F) + sgn).astype(F) * k_aux).astype(F)[mi]
    return grad_pred, grad_corr


def make_case(rng, shape, nyu=False, special=True, on_grid=True):
    """(pred, gt, lidar, corr) whose every term is zero or a normal float32 (depths of 0.5 .. 80 on a 2^-10 grid, so a non-zero
    difference is at least 2^-10): the device's and numpy's float32 terms are then the same bits whatever the denormal mode.
    About a third of gt is invalid (0, -0.0, the threshold itself, a NaN), a fifth of the valid pixels have a LiDAR return;
    some predictions are exact (t = 0); with `special`, unselected pixels of pred and corr hold NaN and +-inf.  on_grid = False
    draws every value from the whole float32 grid instead, so that every operation rounds (for the CPU tests)."""
    if on_grid:
        grid = lambda lo, hi: (rng.integers(int(lo * 1024), int(hi * 1024), shape) / 1024.0).astype(F)
    else:
        grid = lambda lo, hi: rng.uniform(lo, hi, shape).astype(F)
    thr_gt, thr_in = (F(0.0001), F(0.001)) if nyu else (F(0.1), F(0.1))
    gt = grid(0.5, 80)
    r = rng.random(shape)
    gt[r < 0.30] = 0
    gt[r < 0.06] = F(-0.0)
    gt[r < 0.04] = thr_gt  # the threshold itself is not selected
    gt[r < 0.02] = np.nan
    lidar = np.where(rng.random(shape) < 0.2, gt, F(0)).astype(F)
    s = rng.random(shape)
    lidar[s < 0.05] = thr_in
    lidar[s < 0.02] = grid(0.5, 80)[s < 0.02]  # a return where gt may be invalid
    pred = (gt + grid(0, 8) - F(4)).astype(F)
    corr = (gt + grid(0, 4) - F(2)).astype(F)
    pred[np.isnan(pred)] = 1
    corr[np.isnan(corr)] = 1
    q = rng.random(shape)
    pred[q < 0.05] = gt[q < 0.05]  # exact predictions: t = 0 (and NaN where gt is)
    corr[q > 0.95] = gt[q > 0.95]
    if special:
        m, mi = masks(gt, lidar, thr_gt, thr_in)
        bad = np.array([np.nan, np.inf, -np.inf, 3e38], F)
        z = rng.random(shape)
        pred[~m & (z < 0.3)] = bad[rng.integers(0, 4, shape)][~m & (z < 0.3)]
        corr[~mi & (z > 0.7)] = bad[rng.integers(0, 4, shape)][~mi & (z > 0.7)]
    return pred, gt, lidar, corr

"""Literal numpy statements of what the reference's drivers do with a filled frame, and of evaluation.py's metrics, for the
tests only.  Written from the reference, not from oracle/oracle.py.

depth_floor     np.squeeze(tf.nn.relu(d - 0.9) + 0.9) (eval_NYU.py:205, test.py:133) in float32: relu is max(x, 0), which
                keeps a NaN (TF's relu and np.maximum alike).
png16           test.py:133-148: the floor, tf.clip_by_value(d, 0.0, 100.0) (minimum(maximum(d, lo), hi): NaN kept), pad_top
                copies of row 0 on top (np.tile + np.vstack), * 256.0, astype(np.uint16) -- with NaN written as 0
                explicitly, since numpy's cast of NaN to an integer is platform-defined.
evaluate_kitti  Result.evaluate (evaluation.py:82-123) and Result_NYU.evaluate (:196-239): per element the float32
evaluate_nyu    expressions exactly as written; the means are math.fsum of those float32 terms over the count, in float64 --
                the contract include/dtfill.h states (numpy's own float32 pairwise means are within ~1e-6 of it).
The product does not import this file.
"""
import math

import numpy as np

COLUMNS = ("mse", "rmse", "mae", "irmse", "imae", "delta1", "delta2", "delta3", "count")


def depth_floor(d, floor=0.9):
    d = np.asarray(d, np.float32)
    f = np.float32(floor)
    with np.errstate(invalid="ignore"):  # inf - inf
        return np.maximum(d - f, np.float32(0.0)) + f


def clip_by_value(d, lo=0.0, hi=100.0):
    return np.minimum(np.maximum(np.asarray(d, np.float32), np.float32(lo)), np.float32(hi))


def png16(depth, pad_top=96, floor=0.9, lo=0.0, hi=100.0, scale=256.0):
    """One frame [H,W] -> uint16 [pad_top + H, W]; floor=None skips the floor."""
    d = np.asarray(depth, np.float32)
    if floor is not None:
        d = depth_floor(d, floor)
    d = clip_by_value(d, lo, hi)
    extra = np.tile(d[0, :], (pad_top, 1)).astype(np.float32)
    d = np.vstack((extra, d))
    with np.errstate(invalid="ignore"):
        d = d * np.float32(scale)
    return np.where(np.isnan(d), np.float32(0.0), d).astype(np.uint16)


def _mean(terms, count):
    """math.fsum of the float32 terms over count, in float64: NaN without a valid element, as numpy's mean of nothing."""
    return math.fsum(terms.astype(np.float64).tolist()) / count if count else math.nan


def evaluate_kitti(output, target):
    """Result.evaluate: mm for mse / rmse / mae, 1/km for irmse / imae; the deltas stay at their initial 0."""
    output, target = np.asarray(output, np.float32), np.asarray(target, np.float32)
    valid_mask = np.logical_and(output > 0.01, target > 0.01)
    n = int(valid_mask.sum())
    with np.errstate(all="ignore"):
        output_mm = 1e3 * output[valid_mask]
        target_mm = 1e3 * target[valid_mask]
        abs_diff = np.abs(output_mm - target_mm)
        inv_output_km = (1e-3 * output[valid_mask]) ** (-1)
        inv_target_km = (1e-3 * target[valid_mask]) ** (-1)
        abs_inv_diff = np.abs(inv_output_km - inv_target_km)
        terms = (np.power(abs_diff, 2), abs_diff, np.power(abs_inv_diff, 2), abs_inv_diff)
    assert all(t.dtype == np.float32 for t in terms)
    mse, mae, imse, imae = (_mean(t, n) for t in terms)
    return dict(zip(COLUMNS, (mse, math.sqrt(mse), mae, math.sqrt(imse), imae, 0.0, 0.0, 0.0, float(n))))


def evaluate_nyu(output, target):
    """Result_NYU.evaluate: metres, mae = mean(|o - t| / t), delta_k = mean(max(o/t, t/o) < 1.25^k)."""
    output, target = np.asarray(output, np.float32), np.asarray(target, np.float32)
    valid_mask = np.logical_and(output > 0.01, target > 0.01)
    n = int(valid_mask.sum())
    with np.errstate(all="ignore"):
        output_mm = output[valid_mask]
        target_mm = target[valid_mask]
        abs_diff = np.abs(output_mm - target_mm)
        maxRatio = np.maximum(output_mm / target_mm, target_mm / output_mm)
        inv_output_km = (output[valid_mask]) ** (-1)
        inv_target_km = (target[valid_mask]) ** (-1)
        abs_inv_diff = np.abs(inv_output_km - inv_target_km)
        terms = (np.power(abs_diff, 2), abs_diff / target_mm, np.power(abs_inv_diff, 2), abs_inv_diff)
    assert all(t.dtype == np.float32 for t in terms + (maxRatio,))
    mse, mae, imse, imae = (_mean(t, n) for t in terms)
    deltas = [int((maxRatio < 1.25 ** k).sum()) / n if n else math.nan for k in (1, 2, 3)]
    return dict(zip(COLUMNS, (mse, math.sqrt(mse), mae, math.sqrt(imse), imae, *deltas, float(n))))

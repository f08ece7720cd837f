"""k_mask's bit words at every seam of its lane mapping, through the public entry point, both metrics.

The plain prepass reads pixel 64 k + lane of word k, so a word is the compare's lane mask: lane k of a wave collects word k
of a batch of 20 words, a partial last word of a row is handled apart (its pixels at or beyond W are no source and no value),
a block's four waves share rows (the last group of a frame is partial), and a narrow frame's wave takes several rows.  The
outlier instances keep the 16-byte / dword split of their loads.  Every case compares depth, distance, index and the
IndexError bit of the frame status with the oracle bit for bit.

Shapes are the smallest that reach each seam: W on both sides of 64, 256 (the outlier instances' chunk), 512 and of a KITTI
row's 19 words (1216, 1217 = one pixel in a twentieth word), W = 1 and W < 64 (a partial word only, several rows per wave);
H in {1, 3, 4, 5} (less than a block's four waves, exactly four, one more); B = 1 and 9.

Mutation check (run once on a scratch build, not committed): with the `& tail` of the partial last word taken out, the lanes
at or beyond W (they hold 0.0f) count wherever 0.0f is a source; the "every pixel a source" pass of
test_widths_around_every_seam (src_thr = 1) then fails at every W that is no multiple of 64 and passes at 64 and 256
(profiles/r27/mutation_check.txt).
"""
import itertools

import numpy as np
import pytest

from guarded import poison_op
from helpers import dt_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRICS = ("l1_cv", "l2")
WIDTHS = (1, 31, 63, 64, 65, 255, 256, 257, 511, 513, 1216, 1217)
HEIGHTS = (1, 3, 4, 5)
_POISON = itertools.count(26000)
_OPS = {}


def _op(pkg, metric):
    if metric not in _OPS:
        _OPS[metric] = pkg.device.DtFill(device=DEV, metric=metric)
    return _OPS[metric]


def _depths(rng, shape):
    return (np.round(rng.uniform(1.0, 80.0, shape) * 256) / 256).astype(np.float32)


def _run(op, xd, poison=True, **kw):
    import torch

    if poison:
        poison_op(op, next(_POISON), xd.shape)
    res = op.run(xd, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _assert_equal(got, ref, what):
    depth, dt, idx, status = ref
    assert np.array_equal(got["index"], idx), "%s: index differs in %d px" % (what, (got["index"] != idx).sum())
    assert np.array_equal(dt_bits(got["dt"]), dt_bits(dt)), "%s: distance differs" % what
    assert np.array_equal(got["status"] & 1, status), "%s: frames_with_index_error %s, oracle %s" % (what, got["status"] & 1, status)
    ok = status == 0
    assert np.array_equal(got["depth"][ok], depth[ok], equal_nan=True), "%s: depth differs" % what


def _check(pkg, oracle, x, what, metrics=METRICS, **thr):
    import torch

    xd = torch.from_numpy(x).to(DEV)
    for metric in metrics:
        got = _run(_op(pkg, metric), xd, **thr)
        _assert_equal(got, oracle.fill_batch(x, metric=metric, **thr), "%s %s" % (what, metric))


def _ends(rng, H, W):
    """the first and the last pixel of every row are the only sources"""
    a = np.zeros((H, W), np.float32)
    a[:, 0] = _depths(rng, H)
    a[:, W - 1] = _depths(rng, H)
    return a


def _seams(rng, H, W):
    """a source at every multiple of 64 and one pixel to each side of it"""
    a = np.zeros((H, W), np.float32)
    j = np.arange(W)
    on = ((j % 64) <= 1) | ((j % 64) == 63)
    a[:, on] = _depths(rng, (H, int(on.sum())))
    return a


@pytest.mark.parametrize("W", WIDTHS)
def test_widths_around_every_seam(pkg, oracle, W):
    rng = np.random.default_rng(100 + W)
    for H in HEIGHTS:
        for make in (_ends, _seams):
            _check(pkg, oracle, make(rng, H, W)[None], "%s 1x%dx%d" % (make.__name__, H, W))
        # src_thr = 1, val_thr = -1: every pixel is a source and a value, 0.0f too -- a lane past W must still not count
        _check(pkg, oracle, _ends(rng, H, W)[None], "all sources 1x%dx%d" % (H, W), src_thr=1.0, val_thr=-1.0)
        nine = np.stack([(_ends, _seams)[b & 1](rng, H, W) for b in range(9)])
        nine[8] = np.where(rng.random((H, W)) < 0.05, _depths(rng, (H, W)), 0)  # ... and one frame of scattered sources
        nine[8, 0, 0] = 2.0
        _check(pkg, oracle, nine, "9x%dx%d" % (H, W))


@pytest.mark.parametrize("W", (1216, 1217, 70))
@pytest.mark.parametrize("outlier", (False, True), ids=("plain", "outlier"))
def test_misaligned_input_pointer(pkg, oracle, W, outlier):
    """x one float past a 16-byte boundary, and W % 4 != 0: the outlier instances then read dwords, not 16 bytes; the plain
    instance reads dwords anyway.  Same results as from the aligned tensor, which equal the oracle's."""
    import torch

    B, H = 2, 5
    rng = np.random.default_rng(7 + W)
    x = np.where(rng.random((B, H, W)) < 0.05, _depths(rng, (B, H, W)), 0).astype(np.float32)
    x[0, 2, W - 1] = 60.0  # (an outlier among its neighbours, in the last word)
    x[:, 0, 0] = 3.0
    flat = torch.zeros(B * H * W + 4, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    xm = flat[1:1 + B * H * W].view(B, H, W)
    xm.copy_(torch.from_numpy(x))
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    xa = torch.from_numpy(x).to(DEV)
    xo = np.stack([oracle.outlier_removal(f) for f in x]).astype(np.float32) if outlier else x
    for metric in METRICS:
        op = _op(pkg, metric)
        a = _run(op, xa, outlier_removal=outlier)
        m = _run(op, xm, outlier_removal=outlier)
        for k in ("depth", "dt", "index", "status"):
            assert np.array_equal(dt_bits(a[k]) if k == "dt" else a[k], dt_bits(m[k]) if k == "dt" else m[k], equal_nan=(k == "depth")), (metric, k)
        _assert_equal(m, oracle.fill_batch(xo, metric=metric), "misaligned %s W=%d" % (metric, W))


@pytest.mark.parametrize("where", ("first word", "last full word", "partial last word", "nowhere"))
def test_masks_differ_in_exactly_one_pixel(pkg, oracle, where):
    """val_thr = 0.95: the one pixel of 0.92 is a source (1 - 0.92 <= 0.1) and no value.  Its frame, and only its frame, has an
    IndexError where the oracle has one."""
    B, H, W = 3, 5, 200  # three full words and one of eight pixels
    rng = np.random.default_rng(11)
    x = np.where(rng.random((B, H, W)) < 0.1, _depths(rng, (B, H, W)), 0).astype(np.float32)
    x[:, :, 0] = 5.0
    j = {"first word": 5, "last full word": 64 * 2 + 10, "partial last word": 195, "nowhere": None}[where]
    if j is not None:
        x[1, 3, j] = 0.92
    ref = oracle.fill_batch(x, val_thr=0.95)
    assert ref[3].tolist() == [0, int(j is not None), 0]
    _check(pkg, oracle, x, where, val_thr=0.95)


def test_values_at_both_thresholds(pkg, oracle):
    """Values exactly at, one ulp above and one ulp below the source threshold (1 - x against 0.1f) and the value threshold
    (0.1f), in full and partial words; -inf among the non-sources (by both predicates neither a source nor a value; NaN and
    +inf are sources by the predicate `not (1 - x) > thr`, so they are no non-sources and stay out)."""
    H, W = 4, 130
    rng = np.random.default_rng(12)
    t = np.float32(0.1)
    near_src = [np.float32(0.9), np.nextafter(np.float32(0.9), np.float32(2)), np.nextafter(np.float32(0.9), np.float32(0))]
    near_val = [t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))]
    frames = []
    for vals in (near_src, near_val, near_src + near_val):
        a = np.where(rng.random((H, W)) < 0.1, _depths(rng, (H, W)), 0).astype(np.float32)
        a[0, 0] = 4.0
        for r, v in enumerate(vals):
            a[r % H, [3 + r, 63, 64, 127, 128 + (r % 2)]] = v
        a[2, 70] = -np.inf
        frames.append(a)
    _check(pkg, oracle, np.stack(frames), "thresholds")
    _check(pkg, oracle, np.stack(frames), "thresholds nyu", src_thr=0.001)


def test_outlier_removal_in_the_partial_last_word(pkg, oracle):
    """12 x 70: one outlier in the partial last word (columns 64..69), one negative value (the frame is redone by the
    exhaustive launch)."""
    import torch

    rng = np.random.default_rng(13)
    x = np.zeros((2, 12, 70), np.float32)
    x[:, ::2, ::3] = _depths(rng, (2, 6, 24)) % 4 + 2  # depths in [2, 6)
    x[0, 6, 67] = 70.0  # far above the mean of its neighbours
    x[0, 3, 10] = -1.0
    xf = np.stack([oracle.outlier_removal(f) for f in x]).astype(np.float32)
    assert xf[0, 6, 67] == 0 and (xf != x).sum() >= 1
    xd = torch.from_numpy(x).to(DEV)
    for metric in METRICS:
        got = _run(_op(pkg, metric), xd, outlier_removal=True)
        _assert_equal(got, oracle.fill_batch(xf, metric=metric), "outlier %s" % metric)


def test_dense_batch_after_sparse_one_meets_no_stale_flags(pkg, oracle):
    """Two passes on one workspace: frames with an empty sky, a handful of sources or none, then dense frames of the same shape
    without touching the workspace in between.  The second pass equals the oracle, every frame's status is 0 and every pixel is
    the window kernel's: what k_mask clears (row flags, the any-distance flag, status, the called-off sky, the route) is clean."""
    import torch

    B, H, W = 9, 200, 330
    rng = np.random.default_rng(14)
    sparse = np.where(rng.random((B, H, W)) < 0.05, _depths(rng, (B, H, W)), 0).astype(np.float32)
    sparse[0::3, :30] = 0  # a sky
    sparse[0::3, 30, W // 2] = 7.5
    sparse[1::3] = 0  # a handful
    sparse[1::3, 100, 5:300:40] = 3.0
    sparse[2] = 0  # none
    dense = np.where(rng.random((B, H, W)) < 0.05, _depths(rng, (B, H, W)), 0).astype(np.float32)
    op = _op(pkg, "l1_cv")
    first = _run(op, torch.from_numpy(sparse).to(DEV))
    _assert_equal(first, oracle.fill_batch(sparse), "sparse pass")
    assert (first["status"][[0, 1, 3, 4]] & 2).all(), first["status"]
    second = _run(op, torch.from_numpy(dense).to(DEV), poison=False)
    _assert_equal(second, oracle.fill_batch(dense), "dense pass")
    assert not second["status"].any(), "stale status: %s" % second["status"]
    st = op.pass_stats()
    assert st["window"] == B * H * W and st["sky"] == 0 and st["anydist"] == 0 and st["points"] == 0, st

"""The side entry points' references without a GPU: the literal numpy statements of net.py's generate_multi_channel
(tests/gmc_ref.py) and of the drivers' post-fill steps and evaluation.py's metrics (tests/post_ref.py) against
oracle/oracle.py, which the older parity tests compare the kernels with.  Where the two agree, the kernels' tests against
either pin the same thing; where they would not, one of them misreads the reference."""
import math

import numpy as np
import pytest

import gmc_ref as G
import post_ref as P

TABLE_SIZES = (1, 3, 5, 7, 9, 11, 13, 15)


def _steps(oracle, x, m, ts, what, n=3):
    """n chained steps, each checked on its own: counts equal, values within the ref's bar."""
    for k in range(n):
        out, cnt, abs_sum = G.gmc_step(x, m, ts)
        o, ocnt = oracle.gmc_step(x, m, ts)
        assert np.array_equal(ocnt.astype(np.int64), cnt), (what, k)
        G.assert_step_matches(o, out, cnt, abs_sum, "%s step %d" % (what, k + 2))
        x, m = out, G.next_mask(out)


def test_weights_are_create_weight_matrix():
    w = G.weights(7).reshape(7, 7)
    assert w.dtype == np.float32 and w[3, 3] == 7 and w[0, 0] == 1 and w[0, 3] == 4 and w[3, 6] == 4
    assert G.weights(1).tolist() == [1.0] and G.weights(15).min() == 1 and G.weights(15).max() == 15


def test_gmc_ref_hand_worked():
    x = np.zeros((1, 3, 3), np.float32)
    x[0, 0, 0], x[0, 2, 2] = 2.0, 4.0
    m = (x > 0).astype(np.float32)
    out, cnt, abs_sum = G.gmc_step(x, m, 3)
    # the centre sees both sources at weight 1 (corners): they tie and are averaged
    assert cnt[0, 1, 1] == 2 and out[0, 1, 1] == np.float32(np.float32(6.0) / (np.float32(1e-6) + np.float32(2.0)))
    assert cnt[0, 0, 0] == 1 and out[0, 0, 0] == np.float32(2.0) / (np.float32(1e-6) + np.float32(1.0))
    # no source in the window: all 9 taps tie at 0, the zero padding counted
    assert cnt[0, 0, 2] == 9 and out[0, 0, 2] == 0 and abs_sum[0, 1, 1] == 6.0
    # table size 1: the pixel's own value whatever its (finite) mask, negative included
    for mk in (m, -np.ones_like(m), np.full_like(m, -0.0), np.full_like(m, 0.5)):
        assert np.array_equal(G.gmc_step(x, mk, 1)[0], x / (np.float32(1e-6) + np.float32(1.0)))


@pytest.mark.parametrize("ts", TABLE_SIZES)
def test_gmc_ref_vs_oracle_nonnegative_masks(oracle, ts):
    """Finite data, masks >= 0: the counts agree, one-tap pixels bit for bit, the others within the float32 summation bar."""
    rng = np.random.default_rng(100 + ts)
    for shape in ((1, 1, 1), (2, 17, 65), (1, 33, 40)):
        for mk in ("gt01", "binary", "fraction", "neg_zero", "zero"):
            for dk in G.DATA_KINDS:
                x = G.make_data(dk, rng, shape)
                _steps(oracle, x, G.make_mask(mk, rng, x), ts, (ts, shape, mk, dk))


@pytest.mark.parametrize("ts", TABLE_SIZES)
def test_gmc_ref_vs_oracle_negative_masks(oracle, ts):
    """Windows whose every weight is negative select their largest product (net.py's reduce_max runs over all the taps), not
    nothing: a maximum that starts at 0 turns such a window into 0 / 1e-6 = 0."""
    rng = np.random.default_rng(200 + ts)
    for shape in ((1, 20, 30), (2, 33, 40), (1, 1, 1)):
        for mk in ("negative", "neg_band", "neg_tap"):
            for dk in ("sparse", "mixed", "dense"):
                x = G.make_data(dk, rng, shape)
                _steps(oracle, x, G.make_mask(mk, rng, x), ts, (ts, shape, mk, dk), n=1)


def test_gmc_nonfinite_data_deviation(oracle):
    """include/dtfill.h: net.py's sum(data * selected) turns every window that holds a +-inf or NaN input into NaN (inf * 0);
    the product adds such a value only where it is selected.  Pinned here so that a change of either side is noticed."""
    x = np.zeros((1, 9, 9), np.float32)
    x[0, 4, 4] = np.inf
    m = np.ones_like(x)
    m[0, 4, 4] = 0  # every window has a masked tap of a larger weight: the inf is never selected
    with np.errstate(invalid="ignore"):
        ref = G.gmc_step(x, m, 3)[0]
    got = oracle.gmc_step(x, m, 3)[0]
    near = np.zeros_like(x, bool)
    near[0, 3:6, 3:6] = True
    assert np.isnan(ref[near]).all() and np.isfinite(ref[~near]).all()
    assert np.isfinite(got).all() and np.array_equal(got[~near], ref[~near])


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.9, np.nextafter(np.float32(0.9), np.float32(1)),
                     np.nextafter(np.float32(0.9), np.float32(0)), 1.5, 0.5, -3.0, 1e-40, 99.99, 100.0, 100.5, 255.99609375,
                     255.99608, 3e38, -3e38], np.float32)


def _same_bits(a, b):
    """equal values, NaN equal to NaN (any payload), +0 != -0"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("floor", [0.9, 0.0, 1.5])
def test_floor_and_png16_specials_vs_oracle(oracle, floor):
    d = np.concatenate([SPECIALS, -SPECIALS]).reshape(2, -1)
    f = P.depth_floor(d, floor)
    assert f.dtype == np.float32 and _same_bits(f, oracle.depth_floor(d, floor))
    assert np.isnan(f[0, 0]) and f[0, 2] == np.float32(floor) and f[0, 1] == np.inf
    for pad_top in (0, 1, 3):
        for lo, hi, scale in ((0.0, 100.0, 256.0), (0.5, 255.99609375, 256.0), (0.0, 1.0, 65535.0)):
            want = P.png16(d, pad_top, floor, lo, hi, scale)
            assert want.dtype == np.uint16 and want.shape == (pad_top + 2, d.shape[1])
            assert np.array_equal(oracle.depth_to_png16(d, pad_top, floor, lo, hi, scale), want), (pad_top, lo, hi, scale)
            assert want[pad_top, 0] == 0  # NaN: 0, written explicitly
    # no floor: the clip alone; the oracle's floor 0 equals it wherever the clip's lower end is 0
    assert np.array_equal(P.png16(d, 2, None), oracle.depth_to_png16(d, 2, 0.0))
    c = P.clip_by_value(d)
    assert np.isnan(c[0, 0]) and c[0, 1] == 100 and c[0, 2] == 0


def test_metrics_refs_vs_oracle(oracle):
    """post_ref's fsum means against the oracle's numpy float32 means: the counts and the deltas exactly, the rest within
    numpy's float32 pairwise summation (the bar the older device test keeps)."""
    rng = np.random.default_rng(9)
    gt = (rng.random((3, 97, 131)) * 80 + 0.5).astype(np.float32)
    pred = (gt * (1 + 0.1 * rng.standard_normal(gt.shape))).astype(np.float32)
    gt[rng.random(gt.shape) < 0.5] = 0
    pred[0, :4, :6] = [[1.25, 1.5625, 1.953125, 0.8, 0.64, 0.512]] * 4
    gt[0, :4, :6] = 1.0
    for b in range(3):
        for ref, orc in ((P.evaluate_kitti, oracle.evaluate_kitti), (P.evaluate_nyu, oracle.evaluate_nyu)):
            want, got = ref(pred[b], gt[b]), orc(pred[b], gt[b])
            for k in P.COLUMNS:
                if k in ("count", "delta1", "delta2", "delta3"):
                    assert got[k] == want[k], k
                else:
                    assert got[k] == pytest.approx(want[k], rel=1e-5, abs=0), k
    # nothing valid: NaN throughout, as numpy's mean of nothing
    with np.errstate(all="ignore"):
        n = P.evaluate_nyu(np.zeros(5, np.float32), np.ones(5, np.float32))
    assert n["count"] == 0 and all(math.isnan(n[k]) for k in P.COLUMNS[:-1])
    # the ratio thresholds are < 1.25^k on float32 ratios: exactly 1.25 fails delta1, 1 ulp below passes
    below = np.nextafter(np.float32(1.25), np.float32(0))
    n = P.evaluate_nyu(np.float32([1.25, below, 1.0]), np.float32([1.0, 1.0, 1.25]))
    assert n["delta1"] == 1 / 3 and n["delta2"] == 1.0

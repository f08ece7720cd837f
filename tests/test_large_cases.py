"""tests/large_cases.py on tiny stand-in shapes, on the CPU: the comparer reports what it must, the poison is what catches a
store that landed on another copy of the same tile frame, the alias condition rejects a power of two, and the chunking visits
every element."""
import numpy as np
import pytest
import torch

import large_cases as LC

T, H, W = 3, 5, 7


def _tile(seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 1000, (T, H, W)).astype(dtype)


def test_tiers_cross_what_they_promise():
    assert LC.tier_shape("a") == (1255, 352, 1216) and 1255 * 352 * 1216 == 2 ** 29 + 309248
    assert LC.tier_shape("b") == (2509, 352, 1216) and 2509 * 352 * 1216 == 2 ** 30 + 190464
    assert LC.tier_shape("c") == (5017, 352, 1216) and 5017 * 352 * 1216 == 2 ** 31 - 47104
    assert LC.tier_shape("96x352")[0] * 96 * 352 == 2 ** 31 - 2048
    assert LC.tier_shape("40x8150")[0] * 40 * 8150 == 2147362000


def test_upload_tiled_repeats_the_tile():
    tile = _tile()
    for B in (1, T, 2 * T, 3 * T + 2):
        got = LC.upload_tiled(tile, B, "cpu").numpy()
        assert all(np.array_equal(got[b], tile[b % T]) for b in range(B))


def test_planted_mismatch_in_the_last_frame_is_reported():
    tile = _tile()
    B = 4 * T + 1
    out = LC.upload_tiled(tile, B, "cpu")
    exp = torch.from_numpy(tile)
    assert LC.mismatching_frames(out, exp, B) == []
    out[B - 1, H - 1, W - 1] += 1
    assert LC.mismatching_frames(out, exp, B) == [B - 1]
    out[2, 0, 0] += 1
    assert LC.mismatching_frames(out, exp, B, chunk_bytes=2 * H * W * 4) == [2, B - 1]
    assert LC.mismatching_frames(out, exp, B, limit=1) == [2]


def test_comparison_is_of_bit_patterns():
    """-0.0 differs from +0.0, a NaN equals the same NaN and differs from another one; uint16 rows compare as 16-bit words."""
    tile = np.zeros((T, H, W), np.float32)
    tile[1, 2, 3] = np.nan
    out = LC.upload_tiled(tile, 2 * T, "cpu")
    exp = torch.from_numpy(tile)
    assert LC.mismatching_frames(out, exp, 2 * T) == []
    out[3, 0, 0] = -0.0
    out.view(torch.int32)[4, 2, 3] = 0x7FA00001
    assert LC.mismatching_frames(out, exp, 2 * T) == [3, 4]
    t16 = _tile(dtype=np.uint16)
    o16 = LC.upload_tiled(t16, T + 1, "cpu")
    o16[T, 0, 1] ^= 0x8000
    assert LC.mismatching_frames(o16, torch.from_numpy(t16), T + 1) == [T]


def test_frame_copied_from_T_frames_earlier_needs_the_poison():
    """A store whose frame base wrapped by k*T frames writes frame b's (correct) content over frame b - T, which expects the
    same content.  Into outputs that held the right values nothing shows; into poisoned outputs frame b keeps its poison."""
    tile = _tile()
    B = 3 * T
    exp = torch.from_numpy(tile)

    def wrapped_kernel(out):
        for b in range(B):
            dst = b - T if b >= 2 * T else b  # the last T frames land T frames early
            out[dst] = exp[b % T]

    stale = LC.upload_tiled(tile, B, "cpu")  # what an earlier, correct call left there
    wrapped_kernel(stale)
    assert LC.mismatching_frames(stale, exp, B) == []
    poisoned = LC.poison_bits(torch.empty((B, H, W), dtype=torch.float32))
    wrapped_kernel(poisoned)
    assert LC.mismatching_frames(poisoned, exp, B) == [2 * T, 2 * T + 1, 2 * T + 2]


def test_alias_condition_rejects_a_power_of_two():
    assert LC.has_odd_factor(352 * 1216) and LC.has_odd_factor(6 * 4096) and not LC.has_odd_factor(4096) and not LC.has_odd_factor(1)
    with pytest.raises(AssertionError):
        LC.assert_alias_free(4, 64 * 64)
    LC.assert_alias_free(6, 64 * 64)
    LC.assert_alias_free(4, 352 * 1216)
    with pytest.raises(AssertionError):
        LC.payload_planes(8, 16, 16)


def test_chunking_visits_every_element():
    """B is no multiple of the rows per chunk: the ranges tile [0, B) exactly, and a flipped bit at any element of any frame
    is found."""
    tile = _tile()
    B = 5 * T + 2
    exp = torch.from_numpy(tile)
    chunk = 4 * H * W * 4  # four rows per chunk; 17 rows
    seen = []
    assert LC.mismatching_frames(LC.upload_tiled(tile, B, "cpu"), exp, B, chunk_bytes=chunk, visited=seen) == []
    assert seen == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 17)]
    base = LC.upload_tiled(tile, B, "cpu")
    for b in range(B):
        for p in range(H * W):
            out = base.clone()
            out.view(torch.int32).reshape(B, -1)[b, p] ^= 1
            assert LC.mismatching_frames(out, exp, B, chunk_bytes=chunk) == [b], (b, p)


def test_frames_mask_leaves_unselected_tile_frames_out():
    tile = _tile()
    B = 2 * T + 1
    out = LC.upload_tiled(tile, B, "cpu")
    out[1] += 1
    out[T + 2] += 1
    exp = torch.from_numpy(tile)
    assert LC.mismatching_frames(out, exp, B) == [1, T + 2]
    assert LC.mismatching_frames(out, exp, B, frames=[True, False, True]) == [T + 2]


def test_planes_follow_tile_frame_and_payload_plane():
    """[B, C, H, W] payloads: plane (b, c) holds payload plane (b*C + c) % P and expects expected[b % T][that plane]."""
    C, P, B = 4, 3, 2 * T + 1
    planes = LC.payload_planes(P, H, W, seed=1)
    values = LC.upload_tiled(planes, B * C, "cpu").view(B, C, H, W)
    for b, c in ((0, 0), (1, 2), (B - 1, C - 1)):
        assert np.array_equal(values[b, c].numpy().view(np.uint32), planes[(b * C + c) % P].view(np.uint32))
    # an "operator" that adds the tile frame's number to the payload's bits
    exp = np.stack([np.stack([(planes[p].view(np.uint32) + np.uint32(t)).view(np.float32) for p in range(P)]) for t in range(T)])
    out = torch.empty((B, C, H, W), dtype=torch.float32)
    for b in range(B):
        out[b] = torch.from_numpy((values[b].numpy().view(np.uint32) + np.uint32(b % T)).view(np.float32))
    expd = torch.from_numpy(exp)
    assert LC.mismatching_planes(out, expd, B, C) == []
    out.view(torch.int32)[B - 1, C - 1, H - 1, W - 1] ^= 4
    out.view(torch.int32)[2, 1, 0, 0] ^= 4
    assert LC.mismatching_planes(out, expd, B, C, chunk_bytes=5 * H * W * 4) == [(2, 1), (B - 1, C - 1)]


def test_fill_tile_covers_the_families():
    for h, w in ((200, 330), (40, 330), (352, 1216)):
        x = LC.fill_tile(h, w, 3)
        assert x.shape == (len(LC.FAMILIES), h, w) and x.dtype == np.float32
    xo = LC.with_outliers(x)
    assert (xo < 0).sum() == 1 and (xo != x).sum() > 40


def test_exact_sum_is_the_fraction_sum():
    from fractions import Fraction

    rng = np.random.default_rng(5)
    t = (rng.uniform(0, 64, 5000) ** 2).astype(np.float32)
    t[::7] = 0
    t[1::11] = np.float32(2.0 ** -20)
    assert LC.exact_sum(t) == sum(Fraction(float(v)) for v in t)
    assert LC.exact_sum(np.zeros(4, np.float32)) == 0


def test_cell_sums_equal_the_literal_cell_sum(oracle):
    """cell_sums against fill_grad_ref.cell_sum cell by cell (gradients over 40 binades with the planted non-finite values and
    cancelling pairs), and the two tile backwards against fill_grad_ref.backward and near_ref.backward."""
    import fill_grad_ref as R
    import near_ref as N

    rng = np.random.default_rng(9)
    g = R.random_gradient(rng, (1, 40, 50)).reshape(-1)
    ids = rng.integers(-1, 30, g.size)
    ids[ids == 7] = 8  # an empty cell
    got = LC.cell_sums(ids, g, 31)
    for c in range(31):
        assert got[c:c + 1].view(np.uint32)[0] == np.array([R.cell_sum(g[ids == c])], np.float32).view(np.uint32)[0], c
    assert np.isnan(got).any() and np.isinf(got).any() and got[7] == 0 and got[30] == 0
    x = np.where(rng.random((3, 24, 37)) < 0.1, np.round(rng.uniform(1, 80, (3, 24, 37)) * 256) / 256, 0).astype(np.float32)
    x[1, 3, :9] = 0.5  # values that are no sources
    x[2] = 0  # no source: an index-error frame
    index = oracle.fill_batch(x)[2]
    grad = R.random_gradient(rng, x.shape)
    want, wst = R.backward(x, index, grad)
    got, gst = LC.fill_backward_tile(x, index, grad)
    assert np.array_equal(gst, wst) and gst.tolist() == [0, 0, 1] and R.same_bits(got, want)
    planes = R.random_gradient(rng, (2, 24, 37))
    gv, st = LC.gather_backward_tile(x, index, planes)
    for p in range(2):
        want, wst = N.backward(x, index, np.broadcast_to(planes[p], x.shape)[:, None])
        assert np.array_equal(st, wst) and R.same_bits(gv[:, p], want[:, 0]), p

"""The window kernel's chain walk (k_fused, P3) against the CPU oracle: chains that run to the halo's limit, long tie chains
between two sources on an exact diagonal, one long chain among short ones in a wave, and value lists that do not line up
with the sources.  Each case runs at halo 16 (5 % dense frames) and halo 32 (1.2 %), with rows of whole 128-byte lines
(W % 32 == 0: streaming stores) and without, with all outputs and with the depth epilogue."""
import itertools

import numpy as np
import pytest

from guarded import poison_op

pytestmark = pytest.mark.gpu
_POISON = itertools.count(91000)

HALOS = {16: 0.05, 32: 0.012}  # halo -> a source density that k_frame routes to it
WIDTHS = (1216, 1000)           # streaming stores / plain stores


def frames(B, H, W, p, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((B, H, W)) < p, rng.uniform(0.95, 80, (B, H, W)), 0).astype(np.float32)


def run(op, x, st=0.1, vt=0.1, path="auto", **kw):
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
    poison_op(op, next(_POISON), xd.shape, path=path, depth_rows_from=kw.get("depth_rows_from", 0))
    res = op.run(xd, st, vt, path=path, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def check(op, oracle, x, st=0.1, vt=0.1):
    """Every output against the oracle, without and with the depth epilogue; returns which frames took the any-distance
    kernels (status bit 2) in the plain pass."""
    depth, dt, lbl, status = oracle.fill_batch(x, st, vt)
    got = run(op, x, st, vt)
    assert np.array_equal(got["dt"], dt), "distance map differs"
    assert np.array_equal(got["index"], lbl), "label map differs: %d px" % (got["index"] != lbl).sum()
    assert np.array_equal(got["status"] & 1, status)
    ok = status == 0
    assert np.array_equal(got["depth"][ok], depth[ok], equal_nan=True), "filled depth differs"
    general = (got["status"] & 2) != 0
    # the depth epilogue (its own instance of the window kernel): the whole frame's depths go through the crop and the floor;
    # label and distance are stored as without it
    r0 = x.shape[1] // 4
    got = run(op, x, st, vt, want=("depth", "dt", "index"), depth_rows_from=r0, depth_floor=0.9)
    assert np.array_equal(got["dt"], dt), "epilogue pass: distance map differs"
    assert np.array_equal(got["index"], lbl), "epilogue pass: label map differs"
    assert np.array_equal(got["depth"][ok], oracle.depth_floor(depth[:, r0:], 0.9)[ok], equal_nan=True), "epilogue depth differs"
    return general


def hole(x, b, r, c, h, w, sources=()):
    x[b, r:r + h, c:c + w] = 0
    for (i, j, v) in sources:
        x[b, i, j] = v


def ringed(x, b, r, c, a, v=7.0):
    """An empty square of side 2a + 1 at (r, c) inside a ring of sources: its centre (r + a, c + a) is exactly a + 1 from
    the nearest source, and the pixels around it a, a - 1, ..."""
    x[b, r - 1:r + 2 * a + 2, c - 1:c + 2 * a + 2] = v
    x[b, r:r + 2 * a + 1, c:c + 2 * a + 1] = 0


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("halo", sorted(HALOS))
def test_chains_to_the_halo_limit(gpu_op, oracle, halo, W):
    """Empty squares inside rings of sources, so that the distances are exact: centres at d = halo - 1 and d = halo (the
    longest chains the window can decide, kept), and one at d = halo + 1 (its rows are handed on)."""
    x = frames(3, 352, W, HALOS[halo], 5 + halo)
    ringed(x, 0, 40, 100, halo - 2)           # centre at d = halo - 1
    ringed(x, 0, 200, 600, halo - 1)          # centre at d = halo
    ringed(x, 1, 150, 300, halo)              # centre at d = halo + 1: one past the halo
    ringed(x, 2, 100, 150 - halo, halo - 1)   # d = halo across a tile seam
    dt = oracle.fill_batch(x)[1]
    assert dt[0, 40 + halo - 2, 100 + halo - 2] == halo - 1 and dt[0, 200 + halo - 1, 600 + halo - 1] == halo
    assert dt[1, 150 + halo, 300 + halo] == halo + 1
    general = check(gpu_op, oracle, x)
    assert general.tolist() == [False, True, False]  # the window decided d = halo itself (frames 0 and 2)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("halo", sorted(HALOS))
def test_diagonal_tie_chains(gpu_op, oracle, halo, W):
    """Two sources on an exact diagonal inside an empty square: every pixel of the band between them is a tie, and their
    chains run along it."""
    x = frames(2, 352, W, HALOS[halo], 17 + halo)
    k = halo - 2
    for b, (r, c) in enumerate([(60, 200), (180, 500)]):
        hole(x, b, r, c, 2 * halo, 2 * halo, [(r + 2, c + 2, 3.0), (r + 2 + k, c + 2 + k, 4.0)])
        hole(x, b, r + 20, c + 300, halo + 4, halo + 4, [(r + 20 + halo + 3, c + 300, 5.0), (r + 20, c + 300 + halo + 3, 6.0)])
    check(gpu_op, oracle, x)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("halo", sorted(HALOS))
def test_one_long_chain_among_short_ones(gpu_op, oracle, halo, W):
    """Frames at the halo's density (short chains) with, per tile row, one wide empty region whose only nearby source is a
    single distant one: the few walkers of a wave that go there walk a chain of halo - 1 among chains of a hop or two.
    The frames are decided by the window itself -- at halo 16 a pixel 31 from its source could not be -- so they really
    ran at their halo."""
    x = frames(2, 352, W, HALOS[halo], 29 + halo)
    for b in range(2):
        for k, r in enumerate(range(20, 352 - 2 * halo, 3 * halo)):
            c = 40 + (k * 173 + 90 * b) % (W - 3 * halo)
            # an empty square inside a ring of sources, and one source in its corner: the pixels at its centre are halo - 1
            # from every source and walk the longest chains of their wave
            ringed(x, b, r, c, halo - 2)
            x[b, r, c] = 9.0
    depth, dt, lbl, _ = oracle.fill_batch(x)
    assert dt.max() <= halo and dt.max() >= halo - 1
    general = check(gpu_op, oracle, x)
    assert not general.any()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("halo", sorted(HALOS))
def test_value_list_not_aligned_with_the_sources(gpu_op, oracle, halo, W):
    """Masks that differ: values that are not sources shift the value list against the sources' ranks (the gather goes to the
    value list, and an index past its end is an IndexError), next to frames whose masks agree."""
    x = frames(3, 352, W, HALOS[halo], 41 + halo)
    x[0, 5, :40] = 0.5
    hole(x, 1, 100, 100, 2 * halo - 2, 2 * halo - 2, [(101, 101, 2.0), (100 + halo - 1, 100 + halo - 1, 2.5)])
    x[1, 300, ::7] = 0.05
    check(gpu_op, oracle, x)
    check(gpu_op, oracle, x, st=0.6, vt=0.1)  # values in (0.1, 0.6] are in the value list but no sources

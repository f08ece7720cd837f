"""The window kernel with parent codes in four planes, codes 13 and 14 meaning "source" and "undecided" and backward taps 5 and 6
not asked (csrc/dtfill_fused.hpp): index, distance and depth bit for bit against the oracle, with the window kernel alone
(path="fused") and in the whole pass (path="auto").  The cases also cover what a kernel that skips the taps of levels 1 and 2
that have nothing to read, or zeroes its ring only in part, would have to get right (b, d).

  a  64 x 200: an isolated source and two adjacent sources, the two motifs that between them make every code win that can win --
     asserted on the parallel model alone (all 14 winning codes appear, codes 13 and 14 never).  A frame of three sources is
     never the window kernel's (dtfill_route.hpp: halo 16 wants 14 H W / 545 = 329 sources at this shape), so the motifs are
     laid on a lattice, 6 rows by 8 columns, which routes the frame to the halo-16 window; the pass statistics say it did.
  b  100 x 200: sources in rows 0-1 and H-2..H-1, columns 0-1 and W-2..W-1, and on both sides of the tile seams: the seams of
     this shape's tilings (window_tiling: row 50 and column 128 with either halo) and column 160 / row 88, the largest tile's.
     The first levels then read the ring's guard rows and pad words next to live words.
  c  200 x 320 with 1 % sources: too thin for halo 16 (1644 sources), enough for halo 32 (424): the other body runs.
  d  one batch of a 50 %-dense frame and a frame with three sources, two passes on one workspace: what a pass leaves behind
     must never show in the next.  (The thin frame is not the window kernel's: with path="fused" only the dense one is compared.)
Every frame is small: a pass takes milliseconds."""
import itertools

import numpy as np
import pytest

import parallel_model as pm
from guarded import poison_op

pytestmark = pytest.mark.gpu
_POISON = itertools.count(9100)
WINNERS = set(range(13)) | {15}  # every parent code but backward taps 5 and 6


def _depths(rng, n):
    return (np.round(rng.uniform(1.0, 80.0, n) * 256) / 256).astype(np.float32)


def frame_a():
    H, W = 64, 200
    rng = np.random.default_rng(11)
    x = np.zeros((H, W), np.float32)
    k = 0
    for i in range(3, H, 6):
        for j in range(4, W - 1, 8):
            x[i, j] = 1.0
            if k % 2:
                x[i, j + 1] = 1.0  # every other lattice point is a pair
            k += 1
    x[x > 0] = _depths(rng, int((x > 0).sum()))
    return x


def frame_b():
    H, W = 100, 200
    rng = np.random.default_rng(12)
    x = np.zeros((H, W), np.float32)
    for i in (0, 1, H - 2, H - 1, 49, 50, 87, 88):  # the border rows, both sides of the row seams
        x[i, (i % 3)::3] = 1.0
    for j in (0, 1, W - 2, W - 1, 127, 128, 159, 160):  # the border columns, both sides of the column seams
        x[(j % 5)::5, j] = 1.0
    x[rng.random((H, W)) < 0.02] = 1.0
    x[x > 0] = _depths(rng, int((x > 0).sum()))
    return x


def frame_c():
    H, W = 200, 320
    rng = np.random.default_rng(13)
    x = np.zeros(H * W, np.float32)
    n = H * W // 100
    x[rng.choice(H * W, n, replace=False)] = _depths(rng, n)
    return x.reshape(H, W)


def batch_d():
    H, W = 100, 200
    rng = np.random.default_rng(14)
    x = np.zeros((2, H, W), np.float32)
    m = rng.random((H, W)) < 0.5
    x[0][m] = _depths(rng, int(m.sum()))
    for (i, j), v in zip(((20, 30), (20, 31), (70, 150)), (3.5, 7.25, 11.0)):
        x[1, i, j] = v
    return x


def model_codes(x):
    src = ~((np.float32(1.0) - x) > np.float32(0.1))
    gu, g = pm.colscan(src)
    d, live = pm.rowscan(g, gu, pm.skew(gu))
    return set(np.unique(pm.parent(d, live)).tolist())


def run(op, x, path, poisoned=True):
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
    if poisoned:
        poison_op(op, next(_POISON), xd.shape, path=path)
    res = op.run(xd, path=path)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    return out, op.pass_stats()


def assert_frames_equal(got, ref, frames, what):
    depth, dt, lbl, status = ref
    for b in frames:
        assert np.array_equal(got["index"][b], lbl[b]), "%s: index of frame %d differs in %d px" % (what, b, (got["index"][b] != lbl[b]).sum())
        assert np.array_equal(got["dt"][b].view(np.uint32), dt[b].view(np.uint32)), "%s: distance of frame %d differs" % (what, b)
        assert (got["status"][b] & 1) == status[b], (what, b)
        if status[b] == 0:
            assert np.array_equal(got["depth"][b].view(np.uint32), depth[b].view(np.uint32)), "%s: depth of frame %d differs" % (what, b)


_refs = {}


def reference(oracle, name, x):
    if name not in _refs:
        _refs[name] = oracle.fill_batch(x)
    return _refs[name]


def test_motifs_alone_make_every_winning_code_win():
    """On the model: one interior source, then two adjacent sources, each alone in the 64 x 200 frame."""
    one = np.zeros((64, 200), np.float32)
    one[30, 100] = 5.0
    pair = np.zeros((64, 200), np.float32)
    pair[30, 100] = 5.0
    pair[30, 101] = 6.0
    assert (model_codes(one) | model_codes(pair)) == WINNERS | {255}


@pytest.mark.parametrize("path", ["fused", "auto"])
def test_a_every_winning_code(gpu_op, oracle, path):
    x = frame_a()[None]
    assert model_codes(x[0]) == WINNERS | {255}, "the frame must make all 14 winning codes win, and no other"
    ref = reference(oracle, "a", x)
    assert ref[1].max() <= 16
    got, stats = run(gpu_op, x, path)
    assert stats["window"] == x.size and not (got["status"] & 2).any(), (stats, got["status"])
    assert_frames_equal(got, ref, [0], "a, " + path)


@pytest.mark.parametrize("path", ["fused", "auto"])
def test_b_borders_and_seams(gpu_op, oracle, path):
    x = frame_b()[None]
    ref = reference(oracle, "b", x)
    got, stats = run(gpu_op, x, path)
    assert stats["window"] == x.size and not (got["status"] & 2).any(), (stats, got["status"])
    assert_frames_equal(got, ref, [0], "b, " + path)


@pytest.mark.parametrize("path", ["fused", "auto"])
def test_c_halo_32_body(gpu_op, oracle, path):
    x = frame_c()[None]
    n = int((x > 0).sum())
    assert 14 * x.size // 2113 < n < 14 * x.size // 545, "thin enough for halo 32 only"
    ref = reference(oracle, "c", x)
    assert 16 < ref[1].max() <= 32  # no pixel beyond the halo: the window kernel decides the whole frame
    got, stats = run(gpu_op, x, path)
    assert stats["window"] == x.size and not (got["status"] & 2).any(), (stats, got["status"])
    assert_frames_equal(got, ref, [0], "c, " + path)


@pytest.mark.parametrize("path", ["fused", "auto"])
def test_d_dense_beside_thin_twice_on_one_workspace(gpu_op, oracle, path):
    x = batch_d()
    ref = reference(oracle, "d", x)
    frames = [0] if path == "fused" else [0, 1]
    first, s1 = run(gpu_op, x, path)
    assert not (first["status"][0] & 2) and s1["window"] >= x[0].size, (first["status"], s1)
    assert_frames_equal(first, ref, frames, "d, %s, first pass" % path)
    second, s2 = run(gpu_op, x, path, poisoned=False)  # outputs and workspace as the first pass left them
    assert s2 == s1 and np.array_equal(second["status"], first["status"])
    assert_frames_equal(second, ref, frames, "d, %s, second pass" % path)
    # ... and with the frames swapped: each block's neighbours in the launch are the other frame's
    xs = x[::-1].copy()
    refs = tuple(v[::-1] for v in ref)
    third, _ = run(gpu_op, xs, path, poisoned=False)
    assert_frames_equal(third, refs, [1] if path == "fused" else [0, 1], "d, %s, swapped" % path)

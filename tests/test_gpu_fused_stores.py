"""The window kernel's outputs leave through range-checked buffer stores (dtfill_fused.hpp, fused_walk_epilogue): a store the
pass does not make -- an undecided pixel, a cropped row, a map that was not asked for -- is dropped by its offset.  These
compare every such case against the oracle, bit-exact, on the shapes the kernel's tilings meet."""
import itertools

import numpy as np
import pytest

from guarded import poison_op

pytestmark = pytest.mark.gpu

_POISON = itertools.count(9100)
ALL = ("depth", "dt", "index")


def _run(op, x, st=0.1, vt=0.1, want=ALL, path="auto", **kw):
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
    poison_op(op, next(_POISON), xd.shape, path=path, depth_rows_from=kw.get("depth_rows_from"))
    res = op.run(xd, st, vt, want, path=path, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _iid(rng, B, H, W, p):
    return np.where(rng.random((B, H, W)) < p, rng.uniform(0.95, 80, (B, H, W)), 0).astype(np.float32)


def _check(oracle, op, x, st=0.1, vt=0.1, want=ALL, path="auto"):
    depth, dt, lbl, status = oracle.fill_batch(x, st, vt)
    got = _run(op, x, st, vt, want, path)
    if "dt" in want:
        assert np.array_equal(got["dt"], dt), "%s %s: distance map differs" % (path, want)
    if "index" in want:
        assert np.array_equal(got["index"], lbl), "%s %s: label map differs: %d px" % (path, want, (got["index"] != lbl).sum())
    assert np.array_equal(got["status"] & 1, status), (path, want)
    if "depth" in want:
        ok = status == 0
        assert np.array_equal(got["depth"][ok], depth[ok]), "%s %s: filled depth differs" % (path, want)


@pytest.mark.parametrize("B", [1, 3, 8, 33, 64])
def test_kitti_batches(gpu_op, oracle, B):
    x = _iid(np.random.default_rng(100 + B), B, 352, 1216, 0.05)
    _check(oracle, gpu_op, x)


def test_both_halos_in_one_batch(gpu_op, oracle):
    rng = np.random.default_rng(11)
    x = np.concatenate([_iid(rng, 2, 352, 1216, 0.05), _iid(rng, 2, 352, 1216, 0.012), _iid(rng, 1, 352, 1216, 0.3)])
    _check(oracle, gpu_op, x)


def test_output_subsets(gpu_op, oracle):
    x = _iid(np.random.default_rng(12), 3, 352, 1216, 0.05)
    for want in (("depth",), ("dt",), ("index",), ("dt", "index"), ("depth", "index"), ("depth", "dt")):
        for path in ("auto", "fused"):
            _check(oracle, gpu_op, x, want=want, path=path)


def test_scanline_batch(gpu_op, oracle):
    # sky rows above the first source row, sources on every 4th row below: flagged rows and the sky split
    rng = np.random.default_rng(13)
    x = _iid(rng, 4, 352, 1216, 0.25)
    x[:, :100] = 0
    x[:, 100:][:, np.arange(252) % 4 != 0] = 0
    _check(oracle, gpu_op, x)


def test_misaligned_masks(gpu_op, oracle):
    rng = np.random.default_rng(14)
    x = _iid(rng, 3, 352, 1216, 0.05)
    x[0, 10, :64] = rng.uniform(0.001, 0.95, 64)  # values that are sources under one threshold only
    x[2, 200, :32] = 0.5
    _check(oracle, gpu_op, x, 0.001, 0.1)
    _check(oracle, gpu_op, x, 0.1, 0.6)  # fewer values than sources: IndexError frames


def test_crop_and_floor_epilogue(gpu_op, oracle):
    x = _iid(np.random.default_rng(15), 3, 352, 1216, 0.05)
    want = oracle.fill_batch(x)[0]
    for r0, fl in ((96, None), (0, 0.9), (96, 0.9), (1, 0.9)):
        got = _run(gpu_op, x, want=("depth",), depth_rows_from=r0, depth_floor=fl)["depth"]
        ref = want[:, r0:]
        if fl is not None:
            ref = oracle.depth_floor(ref, fl)
        assert np.array_equal(got, ref), (r0, fl)


def test_width_without_streaming_stores(gpu_op, oracle):
    _check(oracle, gpu_op, _iid(np.random.default_rng(16), 3, 352, 1000, 0.05))
    _check(oracle, gpu_op, _iid(np.random.default_rng(17), 2, 353, 1001, 0.02))


def test_2048_square_frame(gpu_op, oracle):
    _check(oracle, gpu_op, _iid(np.random.default_rng(18), 1, 2048, 2048, 0.01))

"""Every source pattern of a small patch on every seam of the kernels' geometry, and every mask of a whole tiny frame, through the
HIP path in both metrics against the CPU oracle: bit-exact labels, distances and depths (tests/exhaustive_cases.py builds the
batches and says which kernel family each goes to; pass_stats() must agree)."""
import itertools

import numpy as np
import pytest

import exhaustive_cases as E
from guarded import poison_op
from helpers import dt_bits

pytestmark = pytest.mark.gpu
_POISON = itertools.count(13000)  # every pass starts from poisoned outputs and workspace (tests/guarded.py)
ALL = ("depth", "dt", "index")
METRICS = ("l1_cv", "l2")


@pytest.fixture(scope="module")
def ops(gpu_op, pkg):
    return {"l1_cv": gpu_op, "l2": pkg.device.DtFill(device="cuda:0", metric="l2")}


def _pass(op, xd, path="auto", want=ALL, separate_frame=False):
    import torch

    poison_op(op, next(_POISON), xd.shape, path=path)
    res = op.run(xd, want=want, path=path, separate_frame=separate_frame)
    stats = op.pass_stats()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}, stats


def _compare(got, ref, metric, what, want=ALL):
    depth, dt, lbl, status = ref
    if "index" in want:
        bad = np.argwhere(got["index"] != lbl)
        assert bad.size == 0, "%s: %d labels differ, first at (mask, row, col) %s" % (what, len(bad), tuple(bad[0]))
    if "dt" in want:
        if metric == "l2":
            assert np.array_equal(dt_bits(got["dt"]), dt_bits(dt)), "%s: distance bits differ" % what
        else:
            assert np.array_equal(got["dt"], dt), "%s: distances differ" % what
    assert np.array_equal(got["status"] & 1, status), "%s: status differs" % what
    if "depth" in want:
        ok = status == 0
        bad = np.argwhere(got["depth"][ok] != depth[ok])
        assert bad.size == 0, "%s: %d depths differ, first at %s" % (what, len(bad), tuple(bad[0]))


def _device(x):
    import torch

    return torch.from_numpy(np.array(x, np.float32)).to("cuda:0")  # (a copy: the sweeps are shared and read-only)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", E.WHOLE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_mask_of_a_whole_frame(ops, oracle, shape, metric):
    """All 2^(H*W) - 1 source masks of a frame of at most 16 pixels as one batch (4 x 4: 65 535 frames, the largest batch there is),
    on the default path and through the any-distance kernels alone; 4 x 4 also with one output wanted at a time."""
    x = E.whole_frames(*shape)
    ref = oracle.fill_batch(x, metric=metric)
    xd = _device(x)
    for path in ("auto", "general"):
        got, stats = _pass(ops[metric], xd, path)
        _compare(got, ref, metric, "%s %s" % (metric, path))
        assert stats["all"] == x.size
        if path == "general":
            assert stats["anydist"] == stats["all"]
        if shape == (4, 4):
            for want in (("index",), ("depth",)):
                got, _ = _pass(ops[metric], xd, path, want=want)
                _compare(got, ref, metric, "%s %s want=%s" % (metric, path, want), want)


def _family_did_the_work(family, metric, path, stats):
    a = stats["all"]
    if path == "general":
        assert stats["anydist"] == a, stats
    elif family in ("win16", "win32"):
        assert stats["window"] == a, stats
    elif family in ("anydist", "pts"):  # (on the default path a frame this small with a handful of sources is k_pts's / the l2 points route's)
        assert stats["points"] == a, stats
    elif family == "thin":  # more than 512 sources, too thin for a window: the any-distance kernels (l2: the row search) by the route itself
        assert stats["anydist"] == a, stats
    elif metric == "l1_cv":
        assert stats["sky"] > 0 and stats["sky"] + stats["window"] + stats["anydist"] == a, stats
    else:  # l2 knows no sky: the rows above the body are the row search's from the start
        assert stats["window"] > 0 and stats["window"] + stats["anydist"] == a, stats


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family,anchor", E.sweep_names(), ids=lambda v: str(v))
def test_patch_sweep(ops, oracle, family, anchor, metric):
    """All masks of a 3 x 3 (3 x 4) patch that straddles one boundary, over a background that sends the frame to the family under test:
    one batch, one oracle call, every path; pass_stats() says that the intended family did the work.  The window sweeps also with the
    frame facts in a launch of their own."""
    x, _ = E.sweep(family, anchor)
    ref = oracle.fill_batch(x, metric=metric)
    xd = _device(x)
    runs = [("auto", False), ("general", False)]
    if metric == "l1_cv" and family in ("win16", "win32", "sky"):
        runs.append(("auto", True))
    for path, separate in runs:
        got, stats = _pass(ops[metric], xd, path, separate_frame=separate)
        _compare(got, ref, metric, "%s/%s %s %s%s" % (family, anchor, metric, path, " separate_frame" if separate else ""))
        assert stats["all"] == x.size
        _family_did_the_work(family, metric, path, stats)


@pytest.mark.parametrize("metric", METRICS)
def test_patch_sweep_misaligned(ops, oracle, metric):
    """The sweep on the window kernel's column seam with a valued pixel that is no source at (0, 0): every label reads the value list
    one entry further on."""
    x = E.misaligned(E.sweep("win16", "colseam")[0])
    ref = oracle.fill_batch(x, metric=metric)
    assert not ref[3].any()
    xd = _device(x)
    for path in ("auto", "general"):
        got, stats = _pass(ops[metric], xd, path)
        _compare(got, ref, metric, "misaligned %s %s" % (metric, path))
        _family_did_the_work("win16", metric, path, stats)

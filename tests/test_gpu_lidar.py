"""The fill on projected LiDAR scans (synth.velodyne_scan; the cases are tests/lidar_cases.py, what they are is pinned by
tests/test_lidar_frames.py): 64-line frames, the 32- and 16-line frames the device subsampling makes from them, the 256-row
crop, the drivers' epilogue, the loader's filter in front, output subsets, planted edge values and a forced l2 hand-over --
both metrics, the auto and the general path, against the oracle.

Bar: index, l1_cv dt and status bit 0 bit-exact; depth bit-exact where the status is 0; l2 dt as sqrtf of the exact integer.
Every pass starts from poisoned outputs and workspace (tests/guarded.py).  After each pass the route is checked from
op.pass_stats() against facts computed from the oracle's distance maps, so that a routing change that stops these frames from
reaching a kernel family fails here instead of quietly testing less."""
import importlib
import itertools

import numpy as np
import pytest

import lidar_cases as C
import lines_ref as R
from guarded import poison_op

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATHS = ("auto", "general")
METRICS = ("l1_cv", "l2")
ALL = ("depth", "dt", "index")
_POISON = itertools.count(9100)


@pytest.fixture(scope="module")
def scans(pkg):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    return {seed: synth.velodyne_scan(C.B, seed=seed) for seed in C.SEEDS}


@pytest.fixture(scope="module")
def ops(pkg, gpu_op):
    return {"l1_cv": gpu_op, "l2": pkg.device.DtFill(device=DEV, metric="l2")}


def fill(op, x, st=0.1, vt=0.1, want=ALL, path="auto", outlier_removal=False, depth_rows_from=0, depth_floor=None):
    """One pass from poisoned outputs and workspace.  x: numpy frames or a device tensor.  Returns (numpy outputs, the
    pass's stats)."""
    import torch

    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    poison_op(op, next(_POISON), tuple(xd.shape), path=path, outlier_removal=outlier_removal,
              depth_rows_from=depth_rows_from or None)
    res = op.run(xd, st, vt, want, path=path, outlier_removal=outlier_removal, depth_rows_from=depth_rows_from,
                 depth_floor=depth_floor)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    return got, op.pass_stats()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_matches(metric, got, ref, want=ALL, what=""):
    depth, dt, idx, status = ref
    if "index" in want:
        bad = got["index"] != idx
        assert not bad.any(), "%s: index differs at %d px, first %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())
    if "dt" in want:
        if metric == "l1_cv":
            assert np.array_equal(bits(got["dt"]), bits(dt)), "%s: distance map differs" % what
        else:
            assert np.array_equal(bits(got["dt"]), bits(dt)), "%s: l2 distance differs" % what
            assert np.array_equal(np.isinf(got["dt"]), np.isinf(dt)), what
    if "depth" in want:
        assert np.array_equal(got["status"] & 1, status), "%s: IndexError frames differ: %s vs %s" % (what, got["status"] & 1, status)
        ok = status == 0
        assert np.array_equal(bits(got["depth"][ok]), bits(depth[ok])), "%s: filled depth differs" % what


def assert_route(stats, metric, path, dt, W, what="", windows=True):
    """What the pass's kernel families must have covered, from the oracle's distance map dt of the frames filled.
    windows: the pass had the window kernels' row flags (l1_cv: no depth epilogue) -- these frames must then reach them."""
    fams = stats["window"] + stats["anydist"] + stats["sky"] + stats["points"]
    assert fams == stats["all"], "%s: every pixel belongs to exactly one kernel family: %s" % (what, stats)
    if path == "general":
        assert stats["anydist"] == stats["all"], "%s: the general path leaves every pixel to the any-distance kernels: %s" % (what, stats)
        return
    if metric == "l1_cv":
        need = W * int(C.rows_beyond(dt).sum())
        assert need > 0, what
        # no window reaches past 32: a row holding a pixel that far from every source is k_sky's or the any-distance kernels'
        assert stats["anydist"] + stats["sky"] >= need, "%s: rows past every window's reach left to a window: %s, need %d" % (what, stats, need)
        if windows:  # ... and the window kernel's tiles decide the rest, in the same frames
            assert stats["window"] > 0, "%s: the window kernel took no row of these frames: %s" % (what, stats)
    else:
        # a row with 152 or more pixels farther than 32 from every source holds more far pixels than k_l2win lists (whatever its
        # radius): the row must have been handed to k_l2env, up front or by the window kernel's count
        need = W * int(C.rows_to_hand_on(dt).sum())
        assert stats["anydist"] >= need, "%s: rows k_l2win must hand on were kept: %s, need %d" % (what, stats, need)
        assert stats["window"] > 0, "%s: k_l2win took no row of these frames: %s" % (what, stats)


def check(oracle, op, metric, x, ref_x=None, st=0.1, vt=0.1, want=ALL, what="", **kw):
    """x through both paths against the oracle on ref_x (default x: what the pass must equal), the route checked after each
    pass.  Returns the oracle's outputs."""
    ref_x = x if ref_x is None else ref_x
    ref = oracle.fill_batch(np.ascontiguousarray(ref_x, np.float32), st, vt, metric=metric)
    for path in PATHS:
        got, stats = fill(op, x, st, vt, want, path, **kw)
        w = "%s %s %s" % (what, metric, path)
        assert_matches(metric, got, ref, want, w)
        assert_route(stats, metric, path, ref[1], ref_x.shape[2], w)
    return ref


def assert_fused_flags(op, x, what=""):
    """l1_cv, the window kernel alone (path "fused"): it finishes no realistic frame -- every one reports that it needed the
    any-distance kernels."""
    got, _ = fill(op, x, path="fused", want=("dt",))
    assert ((got["status"] & 2) != 0).all(), "%s: fused-only path: frames not flagged for the general path: %s" % (what, got["status"])


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("seed", C.SEEDS)
def test_64_line_frames(scans, ops, oracle, metric, seed):
    """Six full 352 x 1216 64-line frames: sky, ragged first ring, walls and boxes, dropped returns."""
    x = scans[seed][0]
    check(oracle, ops[metric], metric, x, what="64 lines seed %d" % seed)
    if metric == "l1_cv":
        assert_fused_flags(ops[metric], x, "64 lines seed %d" % seed)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("keep_ratio", (0.5, 0.25))
def test_device_subsampled_frames(pkg, scans, ops, oracle, metric, keep_ratio):
    """The demo flow: 32 / 16 lines made on the device (bit-identical to ref64 first), then that device tensor filled."""
    import torch

    dev = importlib.import_module(pkg.__name__ + ".device")
    for seed in C.SEEDS:
        x, K, E = scans[seed]
        sub, st = dev.line_subsample_device(torch.from_numpy(x).to(DEV), K, E, keep_ratio)
        torch.cuda.synchronize()
        ref, rst, _ = R.ref64(x, K, E, 64, dev.keep_every_of(keep_ratio))
        assert np.array_equal(bits(sub.cpu().numpy()), bits(ref)) and np.array_equal(st.cpu().numpy(), rst), seed
        what = "%d lines seed %d" % (64 * keep_ratio, seed)
        check(oracle, ops[metric], metric, sub, ref_x=ref, what=what)
        if metric == "l1_cv":
            assert_fused_flags(ops[metric], sub, what)


@pytest.mark.parametrize("metric", METRICS)
def test_eval_crop(scans, ops, oracle, metric):
    """Rows 96: of the 64-line frames, the 256 x 1216 input eval_NYU.py:157 feeds: the sky is a dozen rows high."""
    for seed in C.SEEDS:
        x = np.ascontiguousarray(scans[seed][0][:, C.CROP:])
        check(oracle, ops[metric], metric, x, what="crop seed %d" % seed)
        if metric == "l1_cv":
            assert_fused_flags(ops[metric], x, "crop seed %d" % seed)


def test_drivers_epilogue(pkg, scans, gpu_op, oracle):
    """l1_cv with the drivers' next lines folded into the depth stores (rows 96:, relu(d - 0.9) + 0.9), and the numpy-facing
    DT_complete_batch, against the composed oracle calls."""
    for seed in C.SEEDS:
        x = scans[seed][0]
        depth, dt, idx, status = oracle.fill_batch(x)
        assert not status.any()
        want = oracle.depth_floor(depth[:, C.CROP:], 0.9)
        for path in PATHS:
            got, stats = fill(gpu_op, x, path=path, depth_rows_from=C.CROP, depth_floor=0.9)
            w = "epilogue seed %d %s" % (seed, path)
            assert got["depth"].shape == want.shape and np.array_equal(bits(got["depth"]), bits(want)), w
            assert np.array_equal(bits(got["dt"]), bits(dt)) and np.array_equal(got["index"], idx), w
            assert_route(stats, "l1_cv", path, dt, x.shape[2], w, windows=False)
        batch = x[:3, :, :, None]
        op = pkg.device.default_op()
        poison_op(op, next(_POISON), batch.shape[:3])
        assert np.array_equal(bits(pkg.DT_complete_batch(batch)), bits(oracle.DT_complete_batch(batch))), seed
        poison_op(op, next(_POISON), batch.shape[:3], depth_rows_from=C.CROP)
        got = pkg.DT_complete_batch(batch, first_row=C.CROP, floor=0.9)
        want = oracle.depth_floor(oracle.kitti_rows(oracle.DT_complete_batch(batch), C.CROP), 0.9)
        assert np.array_equal(bits(got), bits(want)), seed


@pytest.mark.parametrize("metric", METRICS)
def test_outlier_filter_in_front(scans, ops, oracle, metric):
    """outlier_removal=True equals the loader's filter (per frame, numpy) and then the fill; a copy with negative depths
    planted takes the filter's exhaustive second launch."""
    x = scans[C.SEEDS[0]][0][:2]
    for name, f in (("plain", x), ("negatives", C.plant_negatives(x, seed=3))):
        xf = np.stack([oracle.outlier_removal(fr) for fr in f]).astype(np.float32)
        assert (xf != f).any(), name
        check(oracle, ops[metric], metric, f, ref_x=xf, outlier_removal=True, what="outlier filter, %s" % name)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("want", (("index",), ("dt",), ("depth",)), ids=lambda w: w[0])
def test_output_subsets(scans, ops, oracle, metric, want):
    x = scans[C.SEEDS[1]][0]
    check(oracle, ops[metric], metric, x, want=want, what="want %s" % (want,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("thr", C.THRESHOLDS, ids=lambda t: "st%s-vt%s" % t)
def test_planted_edge_values(scans, ops, oracle, metric, thr):
    """Edge values planted into real frames -- in the sky, on row r0, in a far row, next to a wall: NaN (a source that is not
    a value), +-inf, a negative value, -0.0, a denormal, 1 - thr and its float32 neighbours for both source thresholds, near
    returns in (0.1, 0.9] (values that are not sources); under (0.1, 0.6) a frame has more sources than values."""
    st, vt = thr
    x = scans[C.SEEDS[0]][0]
    xp = C.plant(x, oracle.fill_batch(x)[1])
    ref = check(oracle, ops[metric], metric, xp, st=st, vt=vt, what="planted st %g vt %g" % thr)
    assert ref[3].any() == (thr == (0.1, 0.6)), ref[3]  # the IndexError frames are there to be reported


@pytest.mark.parametrize("metric", METRICS)
def test_forced_l2_hand_over(scans, ops, oracle, metric):
    """A band of 300 columns emptied below the first source row: its rows hold more far pixels than k_l2win lists, counted by
    two or three of its tiles at once, and go to k_l2env while the rest of the frame stays with the window kernel."""
    for seed in C.SEEDS:
        x = C.hand_over_band(scans[seed][0][:4])
        ref = check(oracle, ops[metric], metric, x, what="band seed %d" % seed)
        if metric == "l2":
            assert C.rows_to_hand_on(ref[1]).sum(1).min() >= 60  # (pinned on the CPU as well)

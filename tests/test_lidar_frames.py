"""What the projected LiDAR frames of tests/test_gpu_lidar.py are (tests/lidar_cases.py), pinned on the CPU: the routing facts
the GPU module's route checks stand on, so that a change to synth.velodyne_scan cannot make it pass by testing something
easier, and the oracle's glue against numpy's own statement of the reference on the planted edge values."""
import importlib

import numpy as np
import pytest

import lidar_cases as C
import lines_ref as R


@pytest.fixture(scope="module")
def scans(pkg):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    return {seed: synth.velodyne_scan(C.B, seed=seed) for seed in C.SEEDS}


@pytest.mark.parametrize("seed", C.SEEDS)
def test_frames_reach_past_every_window(scans, oracle, seed):
    """Every frame (64 lines, 32 and 16 made from them, the 256-row crop) has its first source row where k_sky could take
    the sky above it, yet rows r0 and r0 + 1 -- the two rows k_sky starts from -- hold a pixel farther than any window's halo
    from every source: the window kernel has to hand them on, and the l1_cv pass runs the any-distance kernels next to it."""
    x, K, E = scans[seed]
    frames = {"64": x, "32": R.ref64(x, K, E, 64, 2)[0], "16": R.ref64(x, K, E, 64, 4)[0],
              "crop": np.ascontiguousarray(x[:, C.CROP:])}
    for name, f in frames.items():
        _, dt, _, status = oracle.fill_batch(f)
        assert not status.any(), name
        far = C.rows_beyond(dt)
        for b in range(C.B):
            r0 = C.first_source_row(f[b])
            assert C.SKY_MIN <= r0 <= C.SKY_MAX, (name, b, r0)
            assert far[b, r0] and far[b, r0 + 1], (name, b, r0)
            assert far[b, r0 + 2:].any(), (name, b)  # rows below the sky edge too
            assert (~far[b]).sum() > 64, (name, b)  # ... and plenty of rows a window decides


@pytest.mark.parametrize("seed", C.SEEDS)
def test_device_subsampling_has_no_bin_edge_pixel(scans, seed):
    """The 32- and 16-line frames are compared bit for bit with ref64: no valid pixel of these scans sits within 1e-9 of a
    bin edge inside the pitch range, where the device's float64 rounding could decide differently."""
    x, K, E = scans[seed]
    for ke in (2, 4):
        _, status, q = R.ref64(x, K, E, 64, ke)
        assert not status.any()
        with np.errstate(invalid="ignore"):
            edge = (np.abs(q - np.round(q)) < 1e-9) & (q > 0) & (q < 64 - 1e-9)
        assert not edge.any(), (ke, np.argwhere(edge)[:3])


@pytest.mark.parametrize("seed", C.SEEDS)
def test_forced_hand_over_rows(scans, oracle, seed):
    """Case 8: the emptied band leaves rows with at least 152 pixels farther than 32 from every source (more far pixels than
    k_l2win lists: the rows go to k_l2env) below the first source row, in every frame; and not all of them (the window
    kernel keeps rows of these frames)."""
    x = C.hand_over_band(scans[seed][0][:4])
    _, dt2, _, _ = oracle.fill_batch(x, metric="l2")
    _, dt2_before, _, _ = oracle.fill_batch(scans[seed][0][:4], metric="l2")
    hand = C.rows_to_hand_on(dt2)
    for b in range(4):
        r0 = C.first_source_row(x[b])
        n = int(hand[b, r0:].sum())
        assert 60 <= n <= x.shape[1] - r0 - 60, (b, n)
    assert not (C.rows_to_hand_on(dt2_before) & (np.arange(x.shape[1]) >= 130)).any()  # the band made them


def _numpy_glue(frame, lbl, vt):
    """tools.py:22-27 by numpy itself: (depth, raised)."""
    try:
        with np.errstate(invalid="ignore"):
            values = frame[frame > np.float32(vt)]
        return values[lbl.ravel() - 1].reshape(frame.shape), False
    except IndexError:
        return None, True


@pytest.mark.parametrize("seed", C.SEEDS)
@pytest.mark.parametrize("thr", C.THRESHOLDS + C.DEGENERATE, ids=lambda t: "st%s-vt%s" % t)
def test_oracle_glue_on_planted_values(scans, oracle, seed, thr):
    """On the planted frames, per frame and metric: dt == 0 exactly at the sources of the reference's predicate; a frame's
    status bit 0 is set exactly where numpy's depth_list[label_list - 1] raises; elsewhere depth is that gather, bit for bit
    (label 0 wraps to the last value, as numpy does)."""
    st, vt = thr
    x = scans[seed][0]
    _, dt, _, _ = oracle.fill_batch(x)
    xp = C.plant(x, dt)
    vals = C.planted_values()
    assert all(np.isin(xp.view(np.uint32), np.float32(v).view(np.uint32)).any() for v in vals.values())
    for metric in ("l1_cv", "l2"):
        depth, dt, lbl, status = oracle.fill_batch(xp, st, vt, metric=metric)
        for b in range(C.B):
            src = C.source_mask(xp[b], st)
            assert np.array_equal(dt[b] == 0, src), (metric, b)
            want, raised = _numpy_glue(xp[b], lbl[b], vt)
            assert bool(status[b] & 1) == raised, (metric, b)
            if not raised:
                assert np.array_equal(depth[b].view(np.uint32), want.view(np.uint32)), (metric, b)
    if thr in C.THRESHOLDS:
        # the GPU module's cases: (0.1, 0.6) holds IndexError frames next to ordinary ones, the others none
        assert status.any() == (thr == (0.1, 0.6)) and not status.all()

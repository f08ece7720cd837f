"""Every C ABI entry point on poisoned, guarded and misaligned buffers (through _lib.load(), not through DtFill).

Each output sits in a GuardedBuffer at its own payload offset (0, 4, 12, 64 or 132 bytes past a 256-byte boundary: the
store variants that only unaligned outputs select -- k_fused<false>, k_rows' scalar and 16-byte modes, k_fin's scalar
mode -- run wherever an offset is not 0), starts filled with an impossible value (tests/guarded.py), and the workspace
starts as zero, 0xFF, random bytes or the state a pass over a different input on the other path left.  After every call:
every guard is intact (the workspace's tail guard sits right behind dtfill_workspace_bytes() bytes), x is bit-for-bit
unchanged, no requested output still holds poison, and every output equals the oracle (depth on the frames without
IndexError; everything exact, an l2 dt as sqrtf of the exact integer bit for bit).

Workspace regions of one pass (include/dtfill.h promises no initialisation contract): who writes each region a later kernel
of the same pass reads.  Audited before these tests first ran; no region is read as an index or a count before this pass
has written it.
  region                         written (this pass)                                  read by
  srcbits valbits wpre_* rowcnt_* k_mask: every word of every row                     k_frame, window kernels, k_colT, k_pts, k_l2*
  negflag                        memset in launch_mask (OUTLIER_REMOVAL), k_frame      second k_mask launch (k_mask<2>)
  rowbase_*                      k_frame, every row                                   every later kernel (ranks)
  finfo (all FI_* fields)        k_frame, every frame; FI_NUNRES = 0, then counted up  k_fused, k_sky, k_fin, k_tiesx (FI_NUNRES
                                 by k_fin / k_pts / k_l2win; FI_SKY cleared by k_fused  bounds the xlist loop), k_l2far, k_stats
  route fflag2 rowfar            k_frame, every frame / row; k_fused, k_l2win raise     every later kernel, k_stats
                                 row flags
  status (frame_status NULL)     k_frame, every frame                                 gathers (IndexError bit)
  vlist                          k_frame, misaligned frames only                       gathers of misaligned frames only
  ptslist (l1) / xlist slice (l2) k_frame (l1 ROUTE_POINTS) / k_l2win's blocks (l2)   k_pts / k_l2env tiles, FI_NSRC entries
  ct, rec                        k_colT, frames with fflag2 != 0                       k_rows; k_fin, k_l2env
  spix, planes D0..TIE           k_rows, the rows it takes                            k_fin, same rows
  planes UNRES, xptr, xlist      k_fin / k_pts: every word of the rows they redo;     k_tiesx: only redone rows, FI_NUNRES
                                 xlist up to FI_NUNRES                                 entries, pointers clamped to the frame
  xlist (l2 far list)            k_l2win, FI_NUNRES entries                           k_l2far
  dscratch                       k_fused (distance map when the caller wants none),   k_sky's two base rows; k_tiesx (depths
                                 k_fin (depths of the rows an epilogue drops)          of dropped rows)
"""
import importlib

import numpy as np
import pytest

from guarded import KINDS, GuardedBuffer, is_poison, other_input, poison, poison_output
from helpers import dt_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEN, FUSED, OR = 1, 2, 4  # DTFILL_FLAG_*
ALL = ("depth", "dt", "index")
SUBSETS = (ALL, ("depth",), ("dt",), ("index",), ("depth", "index"))
OFFSETS = (0, 4, 12, 64, 132)
EPILOGUES = (None, (96, None), (0, 0.9), (17, 1.5))
L1_FLAGS = (0, GEN, FUSED, OR, GEN | OR, FUSED | OR)
L2_FLAGS = (0, GEN, OR, GEN | OR)
STATS = ("all", "window", "anydist", "sky", "points", "colt")


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _fill(L, metric, x, st, vt, flags, bufs, ws, nws, epi):
    B, H, W = x["shape"]
    ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
    args = [x["ptr"], B, H, W, st, vt, metric, ptr("depth"), ptr("dt"), ptr("index"), ptr("status"), ws.ptr, nws, _stream(), flags]
    if epi is not None:
        return L.dtfill_batch_epilogue(*args, epi[0], int(epi[1] is not None), float(epi[1] or 0.0))
    return L.dtfill_batch_flags(*args)


def guarded_pass(L, xh, metric=0, flags=0, want=ALL, status=True, offs=None, epi=None, kind="random", seed=0, st=0.1, vt=0.1):
    """One pass over numpy frames xh with every buffer guarded.  Checks the guards and x; returns the outputs (numpy) and
    the pass statistics read right after it (dtfill_pass_stats on the same workspace)."""
    import torch

    B, H, W = xh.shape
    offs = offs or {}
    fb = H * W * 4
    xg = GuardedBuffer(xh.nbytes, offs.get("x", 0), DEV, fb)
    xv = xg.view(torch.float32, xh.shape)
    xv.copy_(torch.from_numpy(np.ascontiguousarray(xh, np.float32)))
    row0 = epi[0] if epi is not None else 0
    shapes = {"depth": (B, H - row0, W), "dt": (B, H, W), "index": (B, H, W), "status": (B,)}
    dtypes = {"depth": torch.float32, "dt": torch.float32, "index": torch.int32, "status": torch.int32}
    names = list(want) + (["status"] if status else [])
    bufs = {k: GuardedBuffer(int(np.prod(shapes[k])) * 4, offs.get(k, 0), DEV, fb) for k in names}
    nws = L.dtfill_workspace_bytes(B, H, W, metric)
    assert nws > 0
    ws = GuardedBuffer(nws, 0, DEV, fb)
    if kind == "previous":
        # what a pass over a different input on the other path leaves in every buffer (values that look valid)
        xp = other_input((B, H, W), seed, DEV)
        prev = {"ptr": xp.data_ptr(), "shape": (B, H, W)}
        assert _fill(L, metric, prev, st, vt, (flags & ~(GEN | FUSED)) | (0 if flags & GEN else GEN), bufs, ws, nws, epi) == 0
    else:
        for k in names:
            poison_output(bufs[k].view(dtypes[k], shapes[k]), k)
        poison(ws.payload(), kind, seed)
    torch.cuda.synchronize()
    x_before = xv.clone()
    rc = _fill(L, metric, {"ptr": xg.ptr, "shape": (B, H, W)}, st, vt, flags, bufs, ws, nws, epi)
    assert rc == 0, L.dtfill_strerror(rc)
    stats = torch.zeros(len(STATS), dtype=torch.int64, device=DEV)
    assert L.dtfill_pass_stats(ws.ptr, nws, B, H, W, metric, stats.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    for k, g in bufs.items():
        g.check(k)
    ws.check("workspace")
    xg.check("x")
    assert torch.equal(xv.view(torch.int32), x_before.view(torch.int32)), "x was written"
    out = {k: bufs[k].view(dtypes[k], shapes[k]).cpu().numpy() for k in names}
    return out, dict(zip(STATS, stats.cpu().tolist()))


def assert_pass_equals_oracle(out, ref, metric, flags, want, epi=None, what=""):
    """Outputs of guarded_pass against oracle.fill_batch: exact (an l2 dt bit for bit), no poison left; with FUSED_ONLY the
    frames that carry DTFILL_FRAME_GENERAL_PATH are left undefined by contract and not compared."""
    depth, dt, idx, status = ref
    B = dt.shape[0]
    keep = np.ones(B, bool)
    if "status" in out:
        s = out["status"]
        assert not (s & ~3).any(), "%s: undefined status bits %s" % (what, np.unique(s & ~3)[:4])
        if flags & FUSED:
            keep = (s & 2) == 0
        if "depth" in want:
            assert np.array_equal((s & 1)[keep], status[keep]), "%s: IndexError bit" % what
    else:
        assert not flags & FUSED, "FUSED_ONLY passes report which frames they left undefined: pass a status buffer"
    if "index" in want:
        got = out["index"][keep]
        assert not is_poison(got, "index").any(), "%s: index poison left" % what
        assert np.array_equal(got, idx[keep]), "%s: index differs at %d px" % (what, (got != idx[keep]).sum())
    if "dt" in want:
        got = out["dt"][keep]
        assert not is_poison(got, "dt").any(), "%s: dt poison left" % what
        if metric == 1:
            assert np.array_equal(dt_bits(got), dt_bits(dt[keep])) and np.array_equal(np.isinf(got), np.isinf(dt[keep])), what
        else:
            assert np.array_equal(got, dt[keep]), "%s: dt differs at %d px" % (what, (got != dt[keep]).sum())
    if "depth" in want:
        ok = keep & (status == 0)
        r0 = epi[0] if epi is not None else 0
        ref_d = depth[:, r0:]
        if epi is not None and epi[1] is not None:
            from oracle import oracle as O

            ref_d = O.depth_floor(ref_d, epi[1])
        got = out["depth"][ok]
        assert not is_poison(got, "depth").any(), "%s: depth poison left" % what
        assert np.array_equal(got, ref_d[ok], equal_nan=True), "%s: depth differs" % what
    return keep


# ------------------------------------------------------------------------------------------------ workloads
def _rings(rng, H, W, top, step, p):
    a = np.where(rng.random((H, W)) < p, np.round(rng.uniform(1.0, 80.0, (H, W)) * 256) / 256, 0.0).astype(np.float32)
    keep = np.zeros(H, bool)
    keep[top::step] = True
    a[~keep] = 0
    return a


def workloads(synth, metric):
    """(name, frames, thresholds, expectations for the pass statistics with flags 0)."""
    rng = np.random.default_rng(1234 + metric)
    w = []
    w.append(("dense kitti 5%", synth.kitti_iid(2, p=0.05, seed=3, hw=(128, 640)), {"window": True}))
    sl = synth.kitti_scanline(2, seed=4, hw=(224, 640), empty_rows=100)
    w.append(("scan-line", sl, {"sky_rows": 100} if metric == 0 else {}))
    a = _rings(rng, 224, 640, 100, 4, 0.25)  # a ragged top: one stray source 30 rows above the rings -> the sky is called off
    a[70, 640 // 3] = 2.5
    b = _rings(rng, 224, 640, 90, 4, 0.25)
    for _ in range(6):
        b[rng.integers(0, 85), rng.integers(0, 640)] = 3.0
    w.append(("ragged top, strays in the sky", np.stack([a, b]), {}))
    pts = np.zeros((2, 240, 320), np.float32)
    for k in range(2):
        pos = rng.choice(240 * 320, 60, replace=False)
        pts[k].flat[pos] = rng.uniform(0.95, 10, 60).astype(np.float32)
    pts[0, 40, 40] = pts[0, 70, 70] = 3.0  # a diagonal pair: tie chains that cross tiles (k_tiesx)
    w.append(("a handful of sources", pts, {"points": True}))
    w.append(("sparse", synth.iid(2, 200, 640, 0.003, seed=5), {}))
    mis = synth.kitti_iid(2, p=0.05, seed=6, hw=(128, 640))
    mis[0, 5, :40] = 0.5  # values that are not sources: the value list is materialised
    mis[1, 9, ::7] = 0.5
    w.append(("misaligned value list", mis, {}))
    ie = synth.kitti_iid(3, p=0.05, seed=7, hw=(96, 320))
    ie[1] = 0  # no source, no value: IndexError
    ie[2] = 0
    ie[2, 3, 4:9] = 0.5  # no source, values: label 0 gathers the last value
    w.append(("IndexError / no source", ie, {}))
    w.append(("W % 4 != 0", synth.iid(2, 61, 131, 0.1, seed=8), {}))
    if metric == 1:
        hole = synth.iid(2, 160, 600, 0.06, seed=9)
        hole[0, 40:120, 200:420] = 0  # far pixels: k_l2win hands rows on to k_l2env
        hole[1, :, 500:] = 0
        w.append(("l2 window hands rows on", hole, {}))
    return w


def _sample_configs(rng, n, flags_set, metric, H):
    cfgs = []
    for i in range(n):
        flags = flags_set[(i + rng.integers(0, len(flags_set))) % len(flags_set)]
        epi = EPILOGUES[i % len(EPILOGUES)] if metric == 0 else None
        if epi is not None and epi[0] >= H:
            epi = None
        offs = {k: int(rng.choice(OFFSETS)) for k in ("x", "depth", "dt", "index", "status")}
        if i % 3 == 0:
            offs.update(depth=0, dt=0, index=0)  # the 128-byte-line variants as well
        cfgs.append(dict(flags=int(flags), want=SUBSETS[i % len(SUBSETS)], status=bool(i % 2 == 0 or flags & FUSED), offs=offs,
                         epi=epi, kind=KINDS[i % len(KINDS)]))
    return cfgs


def _assert_stats(stats, shape, metric, flags, epi, expect):
    B, H, W = shape
    assert stats["all"] == B * H * W
    assert stats["window"] + stats["anydist"] + stats["sky"] + stats["points"] == stats["all"], stats
    if flags & GEN:
        assert stats["anydist"] == stats["all"], stats
    plain = (flags & ~OR) == 0 and epi is None
    if plain and expect.get("window") and metric == 0:
        assert stats["window"] == stats["all"], stats
    if plain and expect.get("points"):
        assert stats["points"] == stats["all"], stats
    if flags == 0 and epi is None and "sky_rows" in expect:
        assert stats["sky"] == B * W * expect["sky_rows"], stats


@pytest.mark.parametrize("metric", [0, 1], ids=["l1_cv", "l2"])
def test_batch_entry_points_on_guarded_poisoned_buffers(L, oracle, synth, metric):
    rng = np.random.default_rng(77 + metric)
    flags_set = L1_FLAGS if metric == 0 else L2_FLAGS
    seed = 0
    for name, x, expect in workloads(synth, metric):
        B, H, W = x.shape
        refs = {}
        for cfg in _sample_configs(rng, 6, flags_set, metric, H):
            flags = cfg["flags"]
            if flags & OR and (H < 4 or W < 4):
                flags &= ~OR
            key = bool(flags & OR)
            if key not in refs:
                xin = np.stack([oracle.outlier_removal(f) for f in x]).astype(np.float32) if key else x
                refs[key] = oracle.fill_batch(xin, metric=("l1_cv", "l2")[metric])
            seed += 1
            what = "%s flags=%d want=%s status=%s offs=%s epi=%s poison=%s" % (name, flags, cfg["want"], cfg["status"], cfg["offs"],
                                                                             cfg["epi"], cfg["kind"])
            out, stats = guarded_pass(L, x, metric, flags, cfg["want"], cfg["status"], cfg["offs"], cfg["epi"], cfg["kind"], seed)
            keep = assert_pass_equals_oracle(out, refs[key], metric, flags, cfg["want"], cfg["epi"], what)
            if flags & FUSED and expect.get("window"):
                assert keep.all(), "%s: a dense frame left to the any-distance kernels" % what
            _assert_stats(stats, x.shape, metric, flags, cfg["epi"], expect)


def test_fused_only_keeps_its_promise(L, oracle, synth):
    """include/dtfill.h FLAG_FUSED_ONLY: frames without DTFILL_FRAME_GENERAL_PATH are complete and exact, with no poison left;
    dense frames are never flagged.  A batch of dense frames and frames the window kernel cannot finish, every output offset."""
    x = synth.kitti_iid(4, p=0.05, seed=11, hw=(128, 640))
    x[1, 20:100] = 0  # a band no window reaches across (distances up to 40)
    x[3] = synth.iid(1, 128, 640, 0.002, seed=12)[0]
    ref = oracle.fill_batch(x)
    for k, off in enumerate(OFFSETS):
        offs = dict(x=0, depth=off, dt=OFFSETS[(k + 1) % 5], index=OFFSETS[(k + 2) % 5], status=OFFSETS[(k + 3) % 5])
        out, _ = guarded_pass(L, x, 0, FUSED, ALL, True, offs, None, KINDS[k % 4], 500 + k)
        keep = assert_pass_equals_oracle(out, ref, 0, FUSED, ALL, None, "fused only, offs %s" % offs)
        assert keep.tolist() == [True, False, True, False], out["status"]


def test_status_holds_defined_bits_only(L, oracle, synth):
    """A poisoned frame_status comes back with DTFILL_FRAME_* bits only, on every path and metric, and bit 0 is the oracle's
    IndexError whenever depth is requested."""
    x = synth.kitti_iid(3, p=0.05, seed=13, hw=(96, 320))
    x[1] = 0
    x[2, :60] = 0
    for metric, flags_set in ((0, L1_FLAGS), (1, L2_FLAGS)):
        ref = oracle.fill_batch(x, metric=("l1_cv", "l2")[metric])
        for flags in flags_set:
            for want in (ALL, ("dt",)):
                out, _ = guarded_pass(L, x, metric, flags, want, True, {"status": 4}, None, "ones", flags)
                s = out["status"]
                assert not (s & ~3).any(), (metric, flags, s)
                if "depth" in want:
                    keep = (s & 2) == 0 if flags & FUSED else np.ones(3, bool)
                    assert np.array_equal((s & 1)[keep], ref[3][keep]), (metric, flags, s)


# ------------------------------------------------------------------------------------------------ side entry points
def test_outlier_removal_guarded(L, oracle):
    import torch

    rng = np.random.default_rng(21)
    for (B, H, W) in ((2, 61, 131), (2, 64, 320), (1, 4, 4), (3, 7, 9)):
        x = np.where(rng.random((B, H, W)) < 0.3, np.round(rng.uniform(1, 80, (B, H, W)) * 256) / 256, 0).astype(np.float32)
        x[:, rng.integers(0, H, 8), rng.integers(0, W, 8)] = 75.0
        want = np.stack([oracle.outlier_removal(f) for f in x])
        for xo, oo in ((0, 0), (4, 12), (12, 64), (64, 132), (132, 4)):
            xg = GuardedBuffer(x.nbytes, xo, DEV, H * W * 4)
            xg.view(torch.float32, x.shape).copy_(torch.from_numpy(x))
            og = GuardedBuffer(x.nbytes, oo, DEV, H * W * 4)
            poison_output(og.view(torch.float32, x.shape), "depth")
            assert L.dtfill_outlier_removal(xg.ptr, B, H, W, og.ptr, _stream()) == 0
            torch.cuda.synchronize()
            xg.check("x")
            og.check("out")
            assert np.array_equal(xg.view(torch.float32, x.shape).cpu().numpy().view(np.uint32), x.view(np.uint32))
            got = og.view(torch.float32, x.shape).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, H, W, xo, oo)


def test_generate_multi_channel_guarded(L, oracle):
    """scale_num 1..4 with NULL beyond it: the buffers that would have been those outputs stay untouched too."""
    import torch

    rng = np.random.default_rng(22)
    for (B, H, W), ts in (((2, 40, 131), 7), ((1, 33, 64), 5), ((2, 17, 19), 3)):
        x = np.where(rng.random((B, H, W)) < 0.06, rng.uniform(1, 80, (B, H, W)), 0).astype(np.float32)
        m = (x > 0.1).astype(np.float32)
        for sn in (1, 2, 3, 4):
            want = oracle.generate_multi_channel(x, m, ts, sn)
            dg, mg = GuardedBuffer(x.nbytes, 4 * sn, DEV, H * W * 4), GuardedBuffer(x.nbytes, 132, DEV, H * W * 4)
            dg.view(torch.float32, x.shape).copy_(torch.from_numpy(x))
            mg.view(torch.float32, x.shape).copy_(torch.from_numpy(m))
            outs = [GuardedBuffer(x.nbytes, OFFSETS[(sn + k) % 5], DEV, H * W * 4) for k in range(3)]
            for o in outs:
                poison_output(o.view(torch.float32, x.shape), "depth")
            ptrs = [o.ptr if k < sn - 1 else None for k, o in enumerate(outs)]
            assert L.dtfill_generate_multi_channel(dg.ptr, mg.ptr, B, H, W, ts, sn, ptrs[0], ptrs[1], ptrs[2], _stream()) == 0
            torch.cuda.synchronize()
            for g in [dg, mg] + outs:
                g.check("gmc sn=%d" % sn)
            for k, o in enumerate(outs):
                got = o.view(torch.float32, x.shape).cpu().numpy()
                if k < sn - 1:
                    assert np.array_equal(got, want[k + 1], equal_nan=True), (B, H, W, ts, sn, k)
                else:
                    assert is_poison(got, "depth").all(), "output %d beyond scale_num %d was written" % (k + 2, sn)


def test_crop_floor_and_png16_guarded(L, oracle, synth):
    import torch

    x = synth.kitti_iid(2, p=0.3, seed=23, hw=(240, 320)) * np.float32(0.05)  # depths around the 0.9 m floor
    B, H, W = x.shape
    xg = GuardedBuffer(x.nbytes, 12, DEV, H * W * 4)
    xg.view(torch.float32, x.shape).copy_(torch.from_numpy(x))
    for (r0, r1, c0, c1) in ((6, 234, 8, 312), (96, 240, 0, 320)):
        for use_floor in (0, 1):
            for oo in (0, 4, 132):
                OH, OW = r1 - r0, c1 - c0
                og = GuardedBuffer(B * OH * OW * 4, oo, DEV, H * W * 4)
                poison_output(og.view(torch.float32, (B, OH, OW)), "depth")
                assert L.dtfill_crop_floor(xg.ptr, B, H, W, r0, r1, c0, c1, use_floor, 0.9, og.ptr, _stream()) == 0
                torch.cuda.synchronize()
                og.check("crop")
                want = x[:, r0:r1, c0:c1]
                want = oracle.depth_floor(want, 0.9) if use_floor else want
                assert np.array_equal(og.view(torch.float32, (B, OH, OW)).cpu().numpy(), want), (r0, r1, c0, c1, use_floor, oo)
    xg.check("x")
    y = synth.kitti_iid(3, p=0.3, seed=24, hw=(37, 131))  # odd W
    y[1, 0, :5] = 150.0  # above the clip
    B, H, W = y.shape
    yg = GuardedBuffer(y.nbytes, 4, DEV, H * W * 4)
    yg.view(torch.float32, y.shape).copy_(torch.from_numpy(y))
    for pad in (0, 96):
        for oo in (0, 2, 130):
            og = GuardedBuffer(B * (H + pad) * W * 2, oo, DEV, H * W * 4)
            og.payload().fill_(0x5A)
            assert L.dtfill_png16(yg.ptr, B, H, W, pad, 1, 0.9, 0.0, 100.0, 256.0, og.ptr, _stream()) == 0
            torch.cuda.synchronize()
            og.check("png16")
            got = og.view(torch.uint16, (B, H + pad, W)).cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b], oracle.depth_to_png16(y[b], pad_top=pad)), (pad, oo, b)
    yg.check("x")


def _metrics_guarded(L, pred, gt, kind, off=(4, 12, 0)):
    import torch

    B = pred.shape[0]
    n = int(np.prod(pred.shape[1:]))
    pg, tg = GuardedBuffer(pred.nbytes, off[0], DEV, n * 4), GuardedBuffer(gt.nbytes, off[1], DEV, n * 4)
    pg.view(torch.float32, pred.shape).copy_(torch.from_numpy(pred))
    tg.view(torch.float32, gt.shape).copy_(torch.from_numpy(gt))
    og = GuardedBuffer(B * 9 * 8, off[2], DEV, 4096)
    og.view(torch.float64, (B, 9)).fill_(float("nan"))
    nws = L.dtfill_metrics_workspace_bytes(B)
    wg = GuardedBuffer(nws, 0, DEV, 4096)
    wg.payload().view(torch.float64).fill_(float("nan"))
    assert L.dtfill_metrics(pg.ptr, tg.ptr, B, n, kind, og.ptr, wg.ptr, nws, _stream()) == 0
    torch.cuda.synchronize()
    for g, w in ((pg, "output"), (tg, "target"), (og, "out"), (wg, "workspace")):
        g.check(w)
    return og.view(torch.float64, (B, 9)).cpu().numpy()


def _assert_metric_row(got, want):
    keys = ("mse", "rmse", "mae", "irmse", "imae", "delta1", "delta2", "delta3")
    assert got[8] == want["count"]
    for k, key in enumerate(keys):
        if np.isnan(want[key]):
            assert np.isnan(got[k]), key
        else:
            assert got[k] == pytest.approx(want[key], rel=1e-5, abs=0.0), key


def test_metrics_guarded(L, oracle):
    import warnings

    rng = np.random.default_rng(25)
    for shape, scale in (((3, 37, 131), 80.0), ((2, 228, 304), 10.0), ((2, 1, 7), 5.0)):
        gt = (rng.random(shape) * scale + 0.5).astype(np.float32)
        pred = (gt * (1.0 + 0.1 * rng.standard_normal(shape))).astype(np.float32)
        gt[rng.random(shape) < 0.6] = 0.0
        gt[-1] = 0.0  # a frame with no valid element: NaN and count 0
        for kind, ref in ((0, oracle.evaluate_kitti), (1, oracle.evaluate_nyu)):
            got = _metrics_guarded(L, pred, gt, kind)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for b in range(shape[0]):
                    _assert_metric_row(got[b], ref(pred[b], gt[b]))
            assert got[-1, 8] == 0 and np.isnan(got[-1, 1])


# ------------------------------------------------------------------------------------------------ batch-size limits
def _many_small_frames(rng, B, H, W):
    p = rng.choice([0.0, 0.1, 0.3, 0.7, 1.0], B)[:, None, None]
    x = np.where(rng.random((B, H, W)) < p, rng.uniform(0.95, 80, (B, H, W)), 0).astype(np.float32)
    x[rng.random(B) < 0.1, 0, 0] = 0.5  # misaligned value lists here and there
    return x


@pytest.mark.parametrize("hw", [(3, 5), (4, 4), (1, 7)])
def test_b65535_small_frames(L, oracle, hw):
    """B = 65535 (the largest grid dimension the header allows) against the oracle: l1_cv both paths, l2; for 4 x 4 also the
    fused outlier filter and dtfill_outlier_removal; crop_floor, png16 and metrics on the same batch."""
    import torch

    H, W = hw
    B = 65535
    rng = np.random.default_rng(H * 100 + W)
    x = _many_small_frames(rng, B, H, W)
    runs = [(0, 0), (0, GEN), (1, 0)] + ([(0, OR)] if H >= 4 else [])
    for k, (metric, flags) in enumerate(runs):
        xin = np.stack([oracle.outlier_removal(f) for f in x[:64]]) if flags & OR else x
        ref = oracle.fill_batch(xin, metric=("l1_cv", "l2")[metric])
        out, stats = guarded_pass(L, x, metric, flags, ALL, True, {"x": 4, "depth": 12, "dt": 64, "index": 132, "status": 4}, None,
                                  KINDS[k % 3], 900 + k)
        if flags & OR:  # the filter's oracle is per frame and slow: the first 64 frames
            out = {n: v[:64] for n, v in out.items()}
        assert_pass_equals_oracle(out, ref, metric, flags, ALL, None, "B=65535 %dx%d metric %d flags %d" % (H, W, metric, flags))
        _assert_stats(stats, x.shape, metric, flags, None, {})
    xd = torch.from_numpy(x).to(DEV)
    if H >= 4:
        og = GuardedBuffer(x.nbytes, 12, DEV, H * W * 4)
        assert L.dtfill_outlier_removal(xd.data_ptr(), B, H, W, og.ptr, _stream()) == 0
        torch.cuda.synchronize()
        og.check("outlier out")
        got = og.view(torch.float32, x.shape).cpu().numpy()
        for b in list(range(64)) + list(range(B - 64, B)):
            assert np.array_equal(got[b].view(np.uint32), oracle.outlier_removal(x[b]).view(np.uint32)), b
    og = GuardedBuffer(B * (H - 1 if H > 1 else 1) * W * 4, 4, DEV, H * W * 4)
    r0 = 1 if H > 1 else 0
    assert L.dtfill_crop_floor(xd.data_ptr(), B, H, W, r0, H, 0, W, 1, 0.9, og.ptr, _stream()) == 0
    pg = GuardedBuffer(B * (H + 2) * W * 2, 2, DEV, H * W * 4)
    assert L.dtfill_png16(xd.data_ptr(), B, H, W, 2, 1, 0.9, 0.0, 100.0, 256.0, pg.ptr, _stream()) == 0
    torch.cuda.synchronize()
    og.check("crop")
    pg.check("png16")
    assert np.array_equal(og.view(torch.float32, (B, H - r0, W)).cpu().numpy(), oracle.depth_floor(x[:, r0:], 0.9))
    png = pg.view(torch.uint16, (B, H + 2, W)).cpu().numpy()
    for b in (0, 1, B // 2, B - 1):
        # (the oracle squeezes its frame: stacked twice, a one-row frame stays two-dimensional; the top H + 2 rows are the answer)
        assert np.array_equal(png[b], oracle.depth_to_png16(np.vstack([x[b], x[b]]), pad_top=2)[:H + 2]), b
    gt = np.roll(x, 1, axis=0)
    got = _metrics_guarded(L, x, gt, 1)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in (0, 1, 2, 3, B // 2, B - 2, B - 1):
            _assert_metric_row(got[b], oracle.evaluate_nyu(x[b], gt[b]))


def test_batch_past_2g_byte_offsets(L, oracle):
    """B*H*W just above 2^29 pixels (1300 frames of 352 x 1216): byte offsets into the float arrays pass 2^31.  The input is
    generated on the device; the first frame and the last three (dense, a sky over rings, sparse) against the oracle."""
    import torch

    B, H, W = 1300, 352, 1216
    assert B * H * W > (1 << 29)
    nws = L.dtfill_workspace_bytes(B, H, W, 0)
    need = B * H * W * 4 * 4 + B * 4 + nws
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * need:
        pytest.skip("needs %.1f GB free twice over, %.1f GB free on this shared device" % (need / 1e9, free / 1e9))
    xg = GuardedBuffer(B * H * W * 4, 0, DEV, H * W * 4)
    xv = xg.view(torch.float32, (B, H, W))
    g = torch.Generator(device=DEV).manual_seed(1300)
    for b0 in range(0, B, 100):  # in chunks: no temporaries the size of the batch
        b1 = min(B, b0 + 100)
        u = torch.rand((b1 - b0, H, W), generator=g, device=DEV)
        v = torch.round((torch.rand((b1 - b0, H, W), generator=g, device=DEV) * 79 + 1) * 256) / 256
        xv[b0:b1] = torch.where(u < 0.05, v, torch.zeros((), device=DEV))
    rows = torch.arange(H, device=DEV)
    xv[B - 2, (rows < 100) | (rows % 4 != 0)] = 0  # a sky over rings
    xv[B - 1] = torch.where(torch.rand((H, W), generator=g, device=DEV) < 0.001, xv[B - 1] + 1.0, torch.zeros((), device=DEV))
    bits_sum = lambda: sum(int(xv[b0:b0 + 100].view(torch.int32).to(torch.int64).sum()) for b0 in range(0, B, 100))  # noqa: E731
    x_sum = bits_sum()
    bufs = {k: GuardedBuffer(B * H * W * 4, 0, DEV, H * W * 4) for k in ALL}
    sg = GuardedBuffer(B * 4, 0, DEV, 4096)
    ws = GuardedBuffer(nws, 0, DEV, H * W * 4)
    try:
        for k in ALL:
            poison_output(bufs[k].payload().view(torch.int32), k)
        poison_output(sg.payload().view(torch.int32), "status")
        poison(ws.payload(), "random", 1300)
        rc = L.dtfill_batch_flags(xg.ptr, B, H, W, 0.1, 0.1, 0, bufs["depth"].ptr, bufs["dt"].ptr, bufs["index"].ptr, sg.ptr, ws.ptr, nws,
                                  _stream(), 0)
        assert rc == 0, L.dtfill_strerror(rc)
        torch.cuda.synchronize()
        for name, gb in list(bufs.items()) + [("status", sg), ("workspace", ws), ("x", xg)]:
            gb.check(name)
        assert bits_sum() == x_sum, "x was written"
        frames = [0, B - 3, B - 2, B - 1]
        xh = xv[frames].cpu().numpy()
        depth, dt, idx, status = oracle.fill_batch(xh)
        st = sg.view(torch.int32, (B,)).cpu().numpy()
        assert not (st & ~3).any() and not (st & 1).any()
        for k, b in enumerate(frames):
            assert np.array_equal(bufs["dt"].view(torch.float32, (B, H, W))[b].cpu().numpy(), dt[k]), b
            assert np.array_equal(bufs["index"].view(torch.int32, (B, H, W))[b].cpu().numpy(), idx[k]), b
            assert np.array_equal(bufs["depth"].view(torch.float32, (B, H, W))[b].cpu().numpy(), depth[k]), b
    finally:
        del bufs, sg, ws, xg, xv
        torch.cuda.empty_cache()

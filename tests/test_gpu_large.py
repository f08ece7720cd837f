"""Every entry point of include/dtfill.h that takes a size, past 2 GiB, past 4 GiB and at the shape rule's limit
(B*H*W just under 2^31; payloads and dtfill_metrics' n beyond it), with the tiled batches and the on-device comparer of
tests/large_cases.py.

The method is the same everywhere: a batch is a tile of T frames repeated on the device, the literal reference runs on the
tile only, every output is poisoned before the call, the result is compared bit for bit on the device against
expected[b % T], and the inputs are compared with the tile again afterwards.  A wrapped offset here would not fault: it would
read or write another frame of the same buffer, which the alias condition and the poison turn into a mismatch
(tests/large_cases.py).  At the limit the last T frames of a batch lie above 4 GiB and both byte thresholds lie inside the
batch, so every frame of the tile is exercised at the high offsets; tiers a and b end less than one frame past their
threshold and serve to localise a failure.

Tiers a / b / c are KITTI frames crossing 2^29 and 2^30 elements and ending 47 104 px below 2^31; two more geometries run at
the limit only.  Each test prints the device bytes it needs beside torch.cuda.mem_get_info() and skips only when the free
memory is below that need plus 10 %.

Where the contract leaves a summation order open to the last place (generate_multi_channel with several selected taps) the
expectation is the device's own result on the tile alone, itself held to the literal reference's bar there; everything else
is compared with the literal reference's bits.

Mutation check (each run once on a scratch build, profiles/r11/large_tests.txt): k_fin's frame base kept to 30 bits fails the
l1_cv pass of tier c (index, frames 0, 1, 4, ...); k_ng_gather's channel plane in u32 fails test_nearest_gather[B 157, C 64];
the metrics kernel's n narrowed to int fails test_metrics_long_rows[B 1, n over 2^31].  The same file holds the device bytes,
the duration and the result of every case.
"""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest

import large_cases as LC
from guarded import _bits, poison_output

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
T = len(LC.FAMILIES)
GB = 1e9


def _sync():
    import torch

    torch.cuda.synchronize()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def need(nbytes, what):
    """Print the test's device bytes beside the free memory; skip only below need + 10 %."""
    import torch

    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    print("\n[large] %s: needs %.2f GB, free %.2f GB of %.2f GB" % (what, nbytes / GB, free / GB, total / GB))
    if free < 1.1 * nbytes:
        pytest.skip("%s needs %.2f GB + 10 %%, %.2f GB are free" % (what, nbytes / GB, free / GB))


def no_mismatch(bad, what):
    assert not bad, "%s: first mismatching frames %s" % (what, bad)


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


@pytest.fixture(scope="module")
def dev(pkg, L):
    return importlib.import_module(pkg.__name__ + ".device")


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


# ================================================================================================ 1. the fill
FILL_TIERS = ("a", "b", "c", "96x352", "40x8150")


class FillRig:
    """One allocation of x, the three outputs, the status, the cropped depth and the workspace for one (B, H, W): an l1_cv
    DtFill whose buffers an l2 DtFill shares (the workspace size does not depend on the metric), so that every pass goes
    through DtFill.run and the ctypes binding carries the workspace's size."""

    def __init__(self, pkg, oracle, name):
        import torch

        self.name = name
        self.B, self.H, self.W = B, H, W = LC.tier_shape(name)
        self.oracle = oracle
        N = B * H * W
        self.row0 = 96 if H > 96 else H // 4
        op = pkg.device.DtFill(DEV, "l1_cv")
        ws = op.workspace_bytes(B, H, W)
        assert ws == pkg.device.DtFill(DEV, "l2").workspace_bytes(B, H, W) and ws > 16 * N
        self.bytes = 4 * N * 5 + 4 * B * (H - self.row0) * W + ws + 4 * LC.CHUNK_BYTES
        print("\n[large] fill %s: B %d x %d x %d = %d px, workspace %.2f GB (%.1f B/px)" % (name, B, H, W, N, ws / GB, ws / N))
        need(self.bytes, "fill tier %s (x, a second x, 3 outputs, cropped depth, workspace)" % name)
        self.tile = LC.fill_tile(H, W, 5)
        self.tile.setflags(write=False)
        # coverage of the high offsets: at the limit the last T frames (every family) lie above 4 GiB, and both thresholds lie
        # inside the batch; tiers a and b end less than a frame past their threshold (they localise a failure): their last
        # frame crosses it
        thr = {"a": 2 ** 31, "b": 2 ** 32}.get(name)
        assert (B - 1) * H * W * 4 < thr < N * 4 if thr else (B - T) * H * W * 4 > 2 ** 32
        self.tile_dev = _up(self.tile)
        self.x = LC.fill_tiled(torch.empty((B, H, W), dtype=torch.float32, device=DEV), self.tile_dev)
        op._ensure(B, H, W)
        op._crop = torch.empty((B, H - self.row0, W), dtype=torch.float32, device=DEV)
        op._home["_crop"] = _stream()
        self.op = op
        self.op2 = pkg.device.DtFill(DEV, "l2")
        for k in ("_shape", "_ws", "_ws_off", "_ws_bytes", "_out"):
            setattr(self.op2, k, getattr(op, k))
        self.op2._home.update(op._home)
        self._refs = {}
        self.passes = 0

    def ref(self, key):
        """The oracle's outputs on the tile (numpy): depth, dt, index, status."""
        if key not in self._refs:
            O = self.oracle
            if key == "l1":
                r = O.fill_batch(self.tile)
            elif key == "l2":
                r = O.fill_batch(self.tile, metric="l2")
            else:
                self.tile_or = LC.with_outliers(self.tile)
                r = O.fill_batch(np.stack([O.outlier_removal(f) for f in self.tile_or]).astype(F))
            self._refs[key] = dict(depth=r[0], dt=r[1], index=r[2], status=r[3])
        return self._refs[key]

    def poison(self):
        """Every output its impossible value, the workspace all zeros or all ones in turn."""
        for k, t in self.op._out.items():
            poison_output(t, k)
        poison_output(self.op._crop, "depth")
        self.op._ws.fill_(0xFF if self.passes % 2 else 0)
        self.passes += 1

    def run(self, op=None, x=None, **kw):
        self.poison()
        res = (op or self.op).run(self.x if x is None else x, **kw)
        _sync()
        return res

    def check(self, res, ref, want, what, x=None, tile=None, epi=None):
        """index, dt (bit patterns), depth where the oracle's status is 0 and status & 1 against the oracle's tile; no
        undefined status bit; the input still equals its tile."""
        import torch

        B = self.B
        if "index" in want:
            no_mismatch(LC.mismatching_frames(res["index"], _up(ref["index"]), B), what + ": index")
        if "dt" in want:
            no_mismatch(LC.mismatching_frames(res["dt"], _up(ref["dt"]), B), what + ": dt")
        if "depth" in want:
            d = ref["depth"]
            if epi is not None:
                d = self.oracle.depth_floor(d[:, epi[0]:], epi[1])
            assert tuple(res["depth"].shape[1:]) == d.shape[1:]
            no_mismatch(LC.mismatching_frames(res["depth"], _up(d), B, frames=ref["status"] == 0), what + ": depth")
            st = res["status"]
            exp = _up(ref["status"])[torch.arange(B, device=DEV) % T]
            no_mismatch(torch.nonzero((st & 1) != exp).reshape(-1)[:8].tolist(), what + ": status & 1")
        assert not bool((res["status"] & ~3).any()), what + ": undefined status bits"
        no_mismatch(LC.mismatching_frames(self.x if x is None else x, self.tile_dev if tile is None else tile, B), what + ": the input changed")

    def close(self):
        import torch

        for o in (self.op, self.op2):
            o._ws = o._out = o._crop = o._shape = None
        self.x = self.tile_dev = None
        self._refs.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=FILL_TIERS)
def rig(request, pkg, oracle, L):
    r = FillRig(pkg, oracle, request.param)
    yield r
    r.close()


ALL = ("depth", "dt", "index")


def test_fill_l1_auto_and_pass_stats(rig, pkg):
    """l1_cv, path auto; dtfill_pass_stats: ALL == B*H*W exactly and every family's share is the tile frames' shares (each
    frame run alone) times their repetitions."""
    res = rig.run(want=ALL)
    rig.check(res, rig.ref("l1"), ALL, "l1_cv auto %s" % rig.name)
    stats = rig.op.pass_stats()
    small = pkg.device.DtFill(DEV, "l1_cv")
    per_frame = []
    for t in range(T):
        small.run(rig.tile_dev[t:t + 1].contiguous())
        per_frame.append(small.pass_stats())
    reps = [len(range(t, rig.B, T)) for t in range(T)]
    want = {k: sum(reps[t] * per_frame[t][k] for t in range(T)) for k in stats}
    print("[large] pass stats %s: %s" % (rig.name, stats))
    assert stats["all"] == rig.B * rig.H * rig.W
    assert stats == want, (stats, want, per_frame)
    print("[large] per tile frame: %s" % (per_frame,))
    hw = rig.H * rig.W
    assert per_frame[3]["points"] == hw and per_frame[5]["anydist"] == hw, per_frame
    if (rig.H, rig.W) == LC.KITTI:  # (the routing of the low and of the wide frames is the kernels' own business)
        assert per_frame[0]["window"] == hw and per_frame[1]["anydist"] == hw and per_frame[2]["sky"] == 30 * rig.W, per_frame


def test_fill_l1_general_path(rig):
    res = rig.run(want=ALL, path="general")
    rig.check(res, rig.ref("l1"), ALL, "l1_cv general %s" % rig.name)


def test_fill_l2(rig):
    res = rig.run(op=rig.op2, want=ALL)
    rig.check(res, rig.ref("l2"), ALL, "l2 %s" % rig.name)


def test_fill_l1_outlier_removal(rig):
    """DTFILL_FLAG_OUTLIER_REMOVAL on a tile with planted outliers and one negative value (the exhaustive second launch)."""
    import torch

    ref = rig.ref("or")
    tile = _up(rig.tile_or)
    x = LC.fill_tiled(torch.empty_like(rig.x), tile)
    res = rig.run(x=x, want=ALL, outlier_removal=True)
    rig.check(res, ref, ALL, "l1_cv outlier removal %s" % rig.name, x=x, tile=tile)
    assert not np.array_equal(ref["index"], rig.ref("l1")["index"]), "the filter removed no source"


def test_fill_l1_epilogue_rows_and_floor(rig):
    """dtfill_batch_epilogue, depth_row0 = 96 (a quarter of the rows of the low frames) and the 0.9 floor: out_depth has its own
    frame pitch (H - row0) * W."""
    res = rig.run(want=ALL, depth_rows_from=rig.row0, depth_floor=0.9)
    assert res["depth"].data_ptr() == rig.op._crop.data_ptr()
    rig.check(res, rig.ref("l1"), ALL, "l1_cv epilogue %s" % rig.name, epi=(rig.row0, 0.9))


@pytest.mark.parametrize("only", ["index", "dt"])
def test_fill_l1_one_output(rig, only):
    """Only out_index, only out_dt: the NULL-output branches; the outputs not asked for keep their poison."""
    import torch

    res = rig.run(want=(only,))
    rig.check(res, rig.ref("l1"), (only,), "l1_cv only %s %s" % (only, rig.name))
    for k in ALL:
        if k != only:
            t = rig.op._out[k].view(torch.int32)  # (every 64th frame or so, and the last T)
            assert bool((t[::max(1, rig.B // 64)] == _bits(k)).all()) and bool((t[-T:] == _bits(k)).all()), "%s was written" % k


# ================================================================================================ 2. the other entry points
_kitti = {}


def kitti_tile(oracle):
    """The KITTI fill tile and the oracle's l1_cv outputs on it, computed once and shared (read-only)."""
    if not _kitti:
        H, W = LC.KITTI
        x = LC.fill_tile(H, W, 5)
        depth, dt, index, status = oracle.fill_batch(x)
        _kitti.update(x=x, depth=depth, index=np.ascontiguousarray(index, np.int32), status=status)
        for a in _kitti.values():
            a.setflags(write=False)
    return _kitti


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    import torch

    _kitti.clear()
    torch.cuda.empty_cache()


def poisoned(shape, dtype=None):
    """A device buffer holding the depth poison (a NaN payload no call produces; INT32-wise a value no label, pixel or status
    takes), or all ones for two-byte types."""
    import torch

    t = torch.empty(shape, dtype=dtype or torch.float32, device=DEV)
    return poison_output(t, "depth") if t.element_size() == 4 else LC.poison_bits(t)


def aligned_ws(nbytes):
    import torch

    ws = LC.poison_bits(torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV))
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def check_rc(L, rc):
    assert rc == 0, L.dtfill_strerror(rc).decode()


def status_mismatch(st, exp_tile, B, mask=-1):
    import torch

    exp = _up(np.asarray(exp_tile, np.int32))[torch.arange(B, device=DEV) % len(exp_tile)]
    return torch.nonzero((st & mask) != exp).reshape(-1)[:8].tolist()


@pytest.mark.parametrize("tier", ["b", "c"])
def test_outlier_removal(L, oracle, tier):
    B, H, W = LC.tier_shape(tier)
    need(2 * 4 * B * H * W + 4 * LC.CHUNK_BYTES, "outlier_removal tier %s" % tier)
    tile = LC.with_outliers(kitti_tile(oracle)["x"])
    want = np.stack([oracle.outlier_removal(f) for f in tile]).astype(F)
    assert (want != tile).sum() > 100
    x, out = LC.upload_tiled(tile, B, DEV), poisoned((B, H, W))
    check_rc(L, L.dtfill_outlier_removal(x.data_ptr(), B, H, W, out.data_ptr(), _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(out, _up(want), B), "outlier_removal")
    no_mismatch(LC.mismatching_frames(x, _up(tile), B), "outlier_removal: x changed")


@pytest.mark.parametrize("tier", ["b", "c"])
def test_fill_backward(L, oracle, tier):
    """index: the oracle's labels, tiled; grad_depth: a gradient over 40 binades with the planted non-finite values and
    cancelling pairs of tests/test_gpu_fill_backward.py, tiled; grad_x and the status bit for bit."""
    import torch

    B, H, W = LC.tier_shape(tier)
    k = kitti_tile(oracle)
    nws = L.dtfill_fill_backward_workspace_bytes(B, H, W)
    assert nws >= 16 * B * H * W
    need(4 * 4 * B * H * W + nws + 4 * LC.CHUNK_BYTES, "fill_backward tier %s (workspace %.2f GB)" % (tier, nws / GB))
    if "fb" not in _kitti:
        import fill_grad_ref as R

        g = R.random_gradient(np.random.default_rng(77), k["x"].shape)
        _kitti["fb"] = (g,) + LC.fill_backward_tile(k["x"], k["index"], g)
    g, want, wst = _kitti["fb"]
    assert wst.tolist() == [0, 0, 0, 0, 0, 1] and np.isnan(want).any()
    x, idx, gd = LC.upload_tiled(k["x"], B, DEV), LC.upload_tiled(k["index"], B, DEV), LC.upload_tiled(g, B, DEV)
    gx, st = poisoned((B, H, W)), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_fill_backward(x.data_ptr(), idx.data_ptr(), gd.data_ptr(), B, H, W, 0.1, gx.data_ptr(), st.data_ptr(), wp, nws,
                                       _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(gx, _up(want), B), "fill_backward grad_x")
    no_mismatch(status_mismatch(st, wst, B), "fill_backward status")
    for t, tile, what in ((x, k["x"], "x"), (idx, k["index"], "index"), (gd, g, "grad_depth")):
        no_mismatch(LC.mismatching_frames(t, _up(tile), B), "fill_backward: %s changed" % what)


# ---- nearest gather: B*H*W at the limit with one channel, and payloads past 2^31 and 2^32 elements with 64
NEAR_SHAPES = {"tier c, C 1": (5017, 1), "B 80, C 64": (80, 64), "B 157, C 64": (157, 64)}
PV, PG = 7, 3  # distinct payload planes of the forward / gradient planes of the backward: coprime to 64


@pytest.mark.parametrize("case", list(NEAR_SHAPES))
def test_nearest_gather(L, oracle, case):
    import near_ref as N
    import torch

    B, C = NEAR_SHAPES[case]
    H, W = LC.KITTI
    n = B * C * H * W
    assert (case == "tier c, C 1" and B == LC.TIERS["c"]) or n > (2 ** 31 if B == 80 else 2 ** 32)
    k = kitti_tile(oracle)
    nws = L.dtfill_nearest_gather_workspace_bytes(B, H, W)
    need(2 * 4 * n + 3 * 4 * B * H * W + nws + 4 * LC.CHUNK_BYTES, "nearest_gather %s (%d payload elements)" % (case, n))
    planes = LC.payload_planes(PV, H, W, seed=3)
    if "ng" not in _kitti:
        _kitti["ng"] = N.gather(k["x"], k["index"], np.broadcast_to(planes, (T, PV, H, W)))
    wv, wp_, wst = _kitti["ng"]
    assert wst.tolist() == [0, 0, 0, 0, 0, N.NO_SOURCE]
    x, idx = LC.upload_tiled(k["x"], B, DEV), LC.upload_tiled(k["index"], B, DEV)
    vals = LC.upload_tiled(planes, B * C, DEV).view(B, C, H, W)
    ov, op, st = poisoned((B, C, H, W)), poisoned((B, H, W), torch.int32), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_nearest_gather(x.data_ptr(), idx.data_ptr(), vals.data_ptr(), C, B, H, W, 0.1, ov.data_ptr(), op.data_ptr(),
                                        st.data_ptr(), wp, nws, _stream()))
    _sync()
    bad = LC.mismatching_planes(ov, _up(wv), B, C)
    assert not bad, "nearest_gather %s: first mismatching (frame, channel) %s" % (case, bad)
    no_mismatch(LC.mismatching_frames(op, _up(wp_), B), "nearest_gather pixel map")
    no_mismatch(status_mismatch(st, wst, B), "nearest_gather status")
    no_mismatch(LC.mismatching_frames(vals.view(B * C, H, W), _up(planes), B * C), "nearest_gather: values changed")
    no_mismatch(LC.mismatching_frames(x, _up(k["x"]), B), "nearest_gather: x changed")
    no_mismatch(LC.mismatching_frames(idx, _up(k["index"]), B), "nearest_gather: index changed")


def test_nearest_gather_pixel_map_only_at_the_limit(L, oracle):
    """C = 0: the pixel map alone, B*H*W at the limit."""
    import near_ref as N
    import torch

    B, H, W = LC.tier_shape("c")
    k = kitti_tile(oracle)
    nws = L.dtfill_nearest_gather_workspace_bytes(B, H, W)
    need(3 * 4 * B * H * W + nws + 4 * LC.CHUNK_BYTES, "nearest_gather pixel map, tier c")
    _, wpix, wst = N.gather(k["x"], k["index"])
    x, idx = LC.upload_tiled(k["x"], B, DEV), LC.upload_tiled(k["index"], B, DEV)
    op, st = poisoned((B, H, W), torch.int32), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_nearest_gather(x.data_ptr(), idx.data_ptr(), None, 0, B, H, W, 0.1, None, op.data_ptr(), st.data_ptr(), wp, nws,
                                        _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(op, _up(wpix), B), "pixel map")
    no_mismatch(status_mismatch(st, wst, B), "pixel map status")


@pytest.mark.parametrize("case", list(NEAR_SHAPES))
def test_nearest_gather_backward(L, oracle, case):
    import fill_grad_ref as R
    import near_ref as N
    import torch

    B, C = NEAR_SHAPES[case]
    H, W = LC.KITTI
    n = B * C * H * W
    k = kitti_tile(oracle)
    nws = L.dtfill_nearest_gather_backward_workspace_bytes(B, H, W, C)
    need(2 * 4 * n + 2 * 4 * B * H * W + nws + 4 * LC.CHUNK_BYTES, "nearest_gather_backward %s (workspace %.2f GB)" % (case, nws / GB))
    if "ngb" not in _kitti:
        gp = R.random_gradient(np.random.default_rng(78), (PG, H, W))
        LC.assert_alias_free(PG, H * W)
        _kitti["ngb"] = (gp,) + LC.gather_backward_tile(k["x"], k["index"], gp)
    gp, want, wst = _kitti["ngb"]
    assert wst.tolist() == [0, 0, 0, 0, 0, N.NO_SOURCE]
    x, idx = LC.upload_tiled(k["x"], B, DEV), LC.upload_tiled(k["index"], B, DEV)
    go = LC.upload_tiled(gp, B * C, DEV).view(B, C, H, W)
    gv, st = poisoned((B, C, H, W)), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_nearest_gather_backward(x.data_ptr(), idx.data_ptr(), go.data_ptr(), C, B, H, W, 0.1, gv.data_ptr(), st.data_ptr(),
                                                 wp, nws, _stream()))
    _sync()
    bad = LC.mismatching_planes(gv, _up(want), B, C)
    assert not bad, "nearest_gather_backward %s: first mismatching (frame, channel) %s" % (case, bad)
    no_mismatch(status_mismatch(st, wst, B), "nearest_gather_backward status")
    no_mismatch(LC.mismatching_frames(go.view(B * C, H, W), _up(gp), B * C), "nearest_gather_backward: grad_out changed")


# ---- crop_floor, png16
def _depth_tile(H, W, seed, nan=True):
    from test_gpu_side_refs import special_frames

    x = special_frames(np.random.default_rng(seed), T, H, W)
    if not nan:  # (the floor's NaN is compared as a NaN elsewhere; here every bit is compared)
        x[np.isnan(x)] = F(0.45)
    LC.assert_alias_free(T, H * W)
    return x


NYU_LIMIT = (27962, 240, 320)  # 2 147 481 600 px: 2 048 below 2^31


@pytest.mark.parametrize("form", ["nyu crop + floor", "nyu crop", "kitti rows 96:", "kitti floor"])
def test_crop_floor_at_the_limit(L, form):
    """The NYU evaluation crop [6:234, 8:312] of 240 x 320 frames and the KITTI forms, B*H*W at the limit."""
    import post_ref as P

    B, H, W = NYU_LIMIT if form.startswith("nyu") else LC.tier_shape("c")
    assert 2 ** 31 - H * W <= B * H * W < 2 ** 31
    r0, r1, c0, c1 = (6, 234, 8, 312) if form.startswith("nyu") else (96, H, 0, W) if "rows" in form else (0, H, 0, W)
    floor = 0.9 if "floor" in form else None
    need(4 * B * (H * W + (r1 - r0) * (c1 - c0)) + 4 * LC.CHUNK_BYTES, "crop_floor %s" % form)
    tile = _depth_tile(H, W, 41, nan=floor is None)
    sub = np.ascontiguousarray(tile[:, r0:r1, c0:c1])
    want = sub if floor is None else P.depth_floor(sub, floor)
    x, out = LC.upload_tiled(tile, B, DEV), poisoned((B, r1 - r0, c1 - c0))
    check_rc(L, L.dtfill_crop_floor(x.data_ptr(), B, H, W, r0, r1, c0, c1, int(floor is not None), float(floor or 0.0), out.data_ptr(),
                                    _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(out, _up(want), B), "crop_floor %s" % form)
    no_mismatch(LC.mismatching_frames(x, _up(tile), B), "crop_floor: x changed")


@pytest.mark.parametrize("case", ["tier b", "output at the limit"])
def test_png16_kitti_pad_96(L, case):
    """test.py's form, pad_top 96: the uint16 output crosses 2 GiB at tier b (1 367 M elements) and ends just under 2^31
    elements, just under 4 GiB, with B = 3942."""
    import post_ref as P
    import torch

    H, W = LC.KITTI
    B = LC.TIERS["b"] if case == "tier b" else 3942
    n_out = B * (H + 96) * W
    assert (2 ** 30 < n_out < 2 ** 31) if case == "tier b" else (2 ** 31 - (H + 96) * W <= n_out < 2 ** 31)
    need(4 * B * H * W + 2 * n_out + 4 * LC.CHUNK_BYTES, "png16 %s" % case)
    tile = _depth_tile(H, W, 43)
    want = np.stack([P.png16(f, 96, 0.9) for f in tile])
    x, out = LC.upload_tiled(tile, B, DEV), poisoned((B, H + 96, W), torch.uint16)
    check_rc(L, L.dtfill_png16(x.data_ptr(), B, H, W, 96, 1, 0.9, 0.0, 100.0, 256.0, out.data_ptr(), _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(out, _up(want), B), "png16 %s" % case)
    no_mismatch(LC.mismatching_frames(x, _up(tile), B), "png16: x changed")


# ---- train_loss and its backward at the limit
@pytest.mark.parametrize("dataset", ["KITTI", "NYU"])
@pytest.mark.parametrize("correct", [False, True], ids=["plain", "correct"])
def test_train_loss_at_the_limit(L, dev, dataset, correct):
    """n_gt and n_in exact, the sums within n_terms * 2^-53 relative of the exact sum (the tile's exact sums times the
    repetitions plus the remainder's), main and aux the double divisions of those, the gradients bit for bit."""
    import loss_ref as R

    B, H, W = LC.tier_shape("c")
    N = B * H * W
    need((6 if correct else 3) * 4 * N + 4 * LC.CHUNK_BYTES, "train_loss %s %s, tier c" % (dataset, "correct" if correct else "plain"))
    kind, gthr, ithr, rows, cols = R.PRESETS[dataset]
    pred, gt, lidar, corr = R.make_case(np.random.default_rng(91 + kind), (T, H, W), nyu=dataset == "NYU")
    if not correct:
        lidar = corr = None
    # the exact sums and counts of the batch: frame t of the tile occurs reps[t] times
    reps = [len(range(t, B, T)) for t in range(T)]
    m, mi = R.masks(gt, lidar, gthr, ithr)
    e, a = R.terms(pred, corr, gt)
    sel = m & R.window_mask(pred.shape, rows, cols)
    n_gt = sum(reps[t] * int(m[t].sum()) for t in range(T))
    S_main = sum(reps[t] * LC.exact_sum(e[t][sel[t]]) for t in range(T))
    nt_main = sum(reps[t] * int(sel[t].sum()) for t in range(T))
    n_in = sum(reps[t] * int(mi[t].sum()) for t in range(T)) if correct else 0
    S_aux = sum(reps[t] * LC.exact_sum(a[t][mi[t]]) for t in range(T)) if correct else Fraction(0)
    assert n_gt > 2 ** 30 and (not correct or n_in > 2 ** 27)
    up = lambda t: None if t is None else LC.upload_tiled(t, B, DEV)  # noqa: E731
    pd, gd, ld, cd = up(pred), up(gt), up(lidar), up(corr)
    stats_d = dev.train_loss_device(pd, gd, ld, cd, dataset=dataset)
    _sync()
    stats = stats_d.cpu().numpy()
    print("[large] train_loss %s stats %s; exact n_gt %d n_in %d S_main %.17g S_aux %.17g" % (dataset, stats.tolist(), n_gt, n_in, float(S_main), float(S_aux)))
    assert stats[2] == n_gt and stats[3] == n_in
    assert abs(Fraction(float(stats[4])) - S_main) <= nt_main * Fraction(2) ** -53 * S_main
    assert abs(Fraction(float(stats[5])) - S_aux) <= n_in * Fraction(2) ** -53 * S_aux
    q = np.float64(stats[4]) / np.float64(stats[2])
    assert stats[0] == (np.sqrt(q) if dataset == "NYU" else q)
    assert stats[1] == (np.float64(stats[5]) / np.float64(stats[3]) if correct else 0.0)
    # the gradients, from the device's own statistics
    g_main, g_aux = F(0.75), F(-1.5)
    want_p, want_c = R.backward(pred, gt, stats, g_main, g_aux if correct else None, lidar, corr, kind, gthr, ithr, rows, cols)
    gp, gc = poisoned((B, H, W)), (poisoned((B, H, W)) if correct else None)
    args = dev._loss_args(pd, gd, ld, cd, dataset, None, None, None, None)
    gm, ga = _up(np.array([g_main], F)), _up(np.array([g_aux], F))
    check_rc(L, L.dtfill_train_loss_backward(*args, stats_d.data_ptr(), gm.data_ptr(), ga.data_ptr() if correct else None, gp.data_ptr(),
                                             gc.data_ptr() if correct else None, _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(gp, _up(want_p), B), "train_loss grad_pred")
    if correct:
        no_mismatch(LC.mismatching_frames(gc, _up(want_c), B), "train_loss grad_corr")
    for t, tile, what in ((pd, pred, "pred"), (gd, gt, "gt"), (ld, lidar, "lidar"), (cd, corr, "corr")):
        if t is not None:
            no_mismatch(LC.mismatching_frames(t, _up(tile), B), "train_loss: %s changed" % what)


# ---- metrics: n beyond 2^31, B * n beyond 2^32
M_TILE = 1000003  # a prime: the period of a row


def _tile_rows(Bn, n, tiles):
    """[Bn, n] on the device, row b = tiles[b] repeated (the last repetition cut short)."""
    import torch

    out = torch.empty((Bn, n), dtype=torch.float32, device=DEV)
    for b in range(Bn):
        t = _up(tiles[b])
        full = n // t.numel()
        out[b, :full * t.numel()].view(full, -1).copy_(t.unsqueeze(0).expand(full, -1))
        out[b, full * t.numel():].copy_(t[:n - full * t.numel()])
    return out


@pytest.mark.parametrize("case", ["B 1, n over 2^31", "B 3, B*n over 2^32"])
def test_metrics_long_rows(L, pkg, case):
    """dtfill_metrics' long long n as more than an int.  The expected row: the counts exactly, every mean the exact combination
    of the tile's and the remainder's math.fsum means (post_ref), under assert_metrics_row's tolerances."""
    import post_ref as P
    import torch
    from test_gpu_side_refs import EDGES, assert_metrics_row, metric_frames

    Bn, n = (1, 2 ** 31 + 4099) if case.startswith("B 1") else (3, 2 ** 32 // 3 + 1001)
    assert n > 2 ** 31 or Bn * n > 2 ** 32
    need(2 * 4 * Bn * n + (1 << 30), "metrics %s" % case)
    pred, gt = metric_frames(np.random.default_rng(93), Bn, M_TILE, EDGES)
    od, td = _tile_rows(Bn, n, pred), _tile_rows(Bn, n, gt)
    nws = L.dtfill_metrics_workspace_bytes(Bn)
    ws = LC.poison_bits(torch.empty(nws, dtype=torch.uint8, device=DEV))
    full, rem = divmod(n, M_TILE)
    for kind, ref in ((pkg._lib.METRICS_KITTI, P.evaluate_kitti), (pkg._lib.METRICS_NYU, P.evaluate_nyu)):
        out = torch.full((Bn, 9), float("nan"), dtype=torch.float64, device=DEV)
        check_rc(L, L.dtfill_metrics(od.data_ptr(), td.data_ptr(), Bn, n, kind, out.data_ptr(), ws.data_ptr(), nws, _stream()))
        _sync()
        rows = out.cpu().numpy()
        for b in range(Bn):
            whole, part = ref(pred[b], gt[b]), ref(pred[b, :rem], gt[b, :rem])
            cw, cp = int(whole["count"]), int(part["count"])
            count = full * cw + cp
            assert count > 2 ** 29 and cp > 0
            want = {"count": float(count)}
            for col in P.COLUMNS[:-1]:
                if col.startswith("delta"):  # k / count with the integer k of every part, one correctly rounded division
                    want[col] = (full * round(whole[col] * cw) + round(part[col] * cp)) / count
                    continue
                # a mean over the row = (reps * count_t * mean_t + count_r * mean_r) / count, in exact fractions of the two
                # correctly rounded means; rmse and irmse are the roots of such means
                sq = col in ("rmse", "irmse")
                mw, mp = (Fraction(v) ** 2 if sq else Fraction(v) for v in (whole[col], part[col]))
                mean = (full * cw * mw + cp * mp) / count
                want[col] = math.sqrt(mean) if sq else float(mean)
            print("[large] metrics %s kind %d row %d: %s" % (case, kind, b, rows[b].tolist()))
            assert_metrics_row(rows[b], want, (case, kind, b))
    for t, tiles, what in ((od, pred, "output"), (td, gt, "target")):  # the inputs still hold their tiles, bit for bit
        for b in range(Bn):
            tile = _up(tiles[b:b + 1])
            no_mismatch(LC.mismatching_frames(t[b, :full * M_TILE].view(full, M_TILE), tile, full), "metrics: %s row %d changed" % (what, b))
            assert torch.equal(t[b, full * M_TILE:].view(torch.int32), tile[0, :rem].view(torch.int32)), (what, b)


# ---- generate_multi_channel (net.py form, table 7) and its backward; the demo driver's form
GT = 4  # frames of the multi-channel tiles: the dense, the sparse, the scan-line and the misaligned frame of the fill tile


def _gmc_tile(oracle):
    x = np.ascontiguousarray(kitti_tile(oracle)["x"][[0, 1, 2, 4]])
    LC.assert_alias_free(GT, x[0].size)
    return x


def _gmc_on_tile(L, x, m, sn):
    """dtfill_generate_multi_channel on the tile alone, held to gmc_ref step by step under its own bar (bit for bit where one
    tap is selected, the float32 summation bound elsewhere).  Returns [lidar_2 .. lidar_sn] as numpy."""
    import gmc_ref as G

    xd, md = _up(x), _up(m)
    outs = [poisoned(x.shape) for _ in range(sn - 1)]
    ptrs = [o.data_ptr() for o in outs] + [None] * (4 - sn)
    check_rc(L, L.dtfill_generate_multi_channel(xd.data_ptr(), md.data_ptr(), *x.shape, 7, sn, *ptrs, _stream()))
    _sync()
    got = [o.cpu().numpy() for o in outs]
    data, mask = x, m
    for k, g in enumerate(got):
        G.assert_step_matches(g, *G.gmc_step(data, mask, 7), what="tile lidar_%d" % (k + 2))
        data, mask = g, G.next_mask(g)
    return got


@pytest.mark.parametrize("tier,sn", [("b", 4), ("c", 2)], ids=["tier b, scale_num 4", "tier c, scale_num 2"])
def test_generate_multi_channel_and_backward(L, oracle, tier, sn):
    """Forward: every output of the batch equals, bit for bit, the device's output on the tile alone, which is held to the
    literal reference.  Backward: the literal reference (gmc_grad_ref.backward) on the tile, bit for bit."""
    import gmc_grad_ref as GG

    B, H, W = LC.tier_shape(tier)
    N = B * H * W
    nws = L.dtfill_generate_multi_channel_backward_workspace_bytes(B, H, W, sn)
    assert nws >= (2 * 4 * N if sn == 4 else 0)
    need(4 * N * (2 + 2 * sn) + nws + 4 * LC.CHUNK_BYTES, "generate_multi_channel + backward %s scale_num %d (forward %d frames, backward %d frames + %.2f GB)"
         % (tier, sn, sn + 1, sn + 2 + (2 if sn > 2 else 0), nws / GB))
    x = _gmc_tile(oracle)
    m = (x > F(0.1)).astype(F)
    tile_outs = _gmc_on_tile(L, x, m, sn)
    xd, md = LC.upload_tiled(x, B, DEV), LC.upload_tiled(m, B, DEV)
    outs = [poisoned((B, H, W)) for _ in range(sn - 1)]
    ptrs = [o.data_ptr() for o in outs] + [None] * (4 - sn)
    check_rc(L, L.dtfill_generate_multi_channel(xd.data_ptr(), md.data_ptr(), B, H, W, 7, sn, *ptrs, _stream()))
    _sync()
    for k, o in enumerate(outs):
        no_mismatch(LC.mismatching_frames(o, _up(tile_outs[k]), B), "generate_multi_channel lidar_%d" % (k + 2))
    no_mismatch(LC.mismatching_frames(xd, _up(x), B), "generate_multi_channel: data changed")
    no_mismatch(LC.mismatching_frames(md, _up(m), B), "generate_multi_channel: mask changed")
    del xd
    # backward: gradients on the 2^-10 grid of moderate size, one of them missing with scale_num 4
    rng = np.random.default_rng(95)
    gs = [(rng.integers(-4096, 4096, x.shape) / 1024.0).astype(F) for _ in range(sn)] + [None] * (4 - sn)
    if sn == 4:
        gs[2] = None
    o2, o3 = (tile_outs + [None, None])[:2] if sn > 2 else (None, None)
    want = GG.backward(m, o2, o3 if sn == 4 else None, 7, sn, tuple(gs))
    gd = [None if g is None else LC.upload_tiled(g, B, DEV) for g in gs]
    grad = poisoned((B, H, W))
    ws, wp = aligned_ws(nws) if nws else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check_rc(L, L.dtfill_generate_multi_channel_backward(md.data_ptr(), ptr(outs[0]) if sn >= 3 else None, ptr(outs[1]) if sn == 4 else None,
                                                         B, H, W, 7, sn, *[ptr(g) for g in gd], grad.data_ptr(), wp, nws, _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(grad, _up(want), B), "generate_multi_channel_backward grad_data")
    no_mismatch(LC.mismatching_frames(md, _up(m), B), "generate_multi_channel_backward: mask changed")


@pytest.mark.parametrize("case", ["plain, tier b", "rgb C 3, B 1254"])
def test_demo_multi_channel(L, oracle, case):
    """demo.py's form.  Plain at tier b; with a three-channel image at B = 1254 the [B,H,W,4] outputs hold 2 147 008 512
    elements, just under their own limit, while the input is a quarter of that.  The batch equals, bit for bit, the device's
    outputs on the tile alone, which are held to the literal reference (gmcv_ref, +0 and -0 equal)."""
    import gmcv_ref as V

    H, W = LC.KITTI
    rgb = case.startswith("rgb")
    B, C = (1254, 3) if rgb else (LC.TIERS["b"], 0)
    N = B * H * W
    n_out = N * (C + 1)
    assert 2 ** 31 - H * W * (C + 1) <= n_out < 2 ** 31 if rgb else 2 ** 30 < n_out
    nws = L.dtfill_demo_multi_channel_workspace_bytes(B, H, W, 4)
    need(4 * (N * (1 + C) + 4 * n_out) + nws + 4 * LC.CHUNK_BYTES, "demo_multi_channel %s (workspace %.2f GB)" % (case, nws / GB))
    x = _gmc_tile(oracle)
    img = np.random.default_rng(96).uniform(0, 255, (GT, H, W, 3)).astype(F) if rgb else None
    want = V.outputs(V.chain(x, 7, 4), img, 90.0)
    oshape = lambda b: (b, H, W, C + 1) if rgb else (b, H, W)  # noqa: E731

    def call(b, xd, rd):
        outs = [poisoned(oshape(b)) for _ in range(4)]
        n = L.dtfill_demo_multi_channel_workspace_bytes(b, H, W, 4)
        ws, wp = aligned_ws(n)
        check_rc(L, L.dtfill_demo_multi_channel(xd.data_ptr(), rd.data_ptr() if rgb else None, C, b, H, W, 7, 4, 90.0,
                                                *[o.data_ptr() for o in outs], wp, n, _stream()))
        _sync()
        return outs

    tile_outs = call(GT, _up(x), _up(img) if rgb else None)
    for k in range(4):
        V.assert_same(tile_outs[k].cpu().numpy(), want[k], "tile out_%d" % (k + 1))
    xd = LC.upload_tiled(x, B, DEV)
    rd = LC.upload_tiled(img, B, DEV) if rgb else None
    outs = call(B, xd, rd)
    for k in range(4):
        no_mismatch(LC.mismatching_frames(outs[k], tile_outs[k], B), "demo_multi_channel out_%d" % (k + 1))
    no_mismatch(LC.mismatching_frames(xd, _up(x), B), "demo_multi_channel: lidar changed")
    if rgb:
        no_mismatch(LC.mismatching_frames(rd, _up(img), B), "demo_multi_channel: rgb changed")


# ---- depth_read
@pytest.mark.parametrize("case", ["input at the limit", "output at the limit"])
def test_depth_read(L, case):
    """Raw [B, 375, 1242] uint16 with B*hmax*wmax just under 2^31 and frames of mixed sizes (one of them outside the buffer:
    BAD_DIMS, an all-zero frame) resized to 352 x 1216; and a small input whose output is at the limit."""
    import read_ref as R
    import torch

    H, W = LC.KITTI
    B, hmax, wmax = (4610, 375, 1242) if case.startswith("input") else (LC.TIERS["c"], 100, 300)
    n_in, n_out = B * hmax * wmax, B * H * W
    assert 2 ** 31 - hmax * wmax <= n_in < 2 ** 31 if case.startswith("input") else 2 ** 31 - H * W <= n_out < 2 ** 31
    nws = L.dtfill_depth_read_workspace_bytes(B, H, W)
    need(2 * n_in + 4 * n_out + nws + 4 * LC.CHUNK_BYTES, "depth_read %s" % case)
    LC.assert_alias_free(T, hmax * wmax)
    rng = np.random.default_rng(97)
    raw = rng.integers(0, 65536, (T, hmax, wmax)).astype(np.uint16)
    raw[3] = rng.integers(0, 256, (hmax, wmax))  # every value <= 255: NOT_16BIT
    dims = np.array([(hmax, wmax), (hmax - 5, wmax - 16), (min(hmax, H), min(wmax, W)), (hmax - 1, wmax - 4), (hmax + 1, wmax),
                     (hmax // 2, wmax // 2)], np.int32)
    want = np.zeros((T, H, W), F)
    wst = np.zeros(T, np.int32)
    for t, (h, w) in enumerate(dims):
        if h > hmax or w > wmax:
            wst[t] = R.BAD_DIMS
        else:
            want[t], wst[t] = R.depth_read_frame(raw[t, :h, :w], H, W)
    assert wst.tolist() == [0, 0, 0, R.NOT_16BIT, R.BAD_DIMS, 0]
    rd, dd = LC.upload_tiled(raw, B, DEV), LC.upload_tiled(dims, B, DEV)
    out, st = poisoned((B, H, W)), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_depth_read(rd.data_ptr(), dd.data_ptr(), B, hmax, wmax, H, W, out.data_ptr(), st.data_ptr(), wp, nws, _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(out, _up(want), B), "depth_read %s" % case)
    no_mismatch(status_mismatch(st, wst, B), "depth_read status")
    no_mismatch(LC.mismatching_frames(rd, _up(raw), B), "depth_read: raw changed")


# ---- line_subsample
@pytest.mark.parametrize("tier", ["b", "c"])
def test_line_subsample(L, synth, tier):
    """Per-frame K and E.  Compared as tests/test_gpu_lines.py does: bit-equal off the bin edges (|q - round(q)| < 1e-9), and
    such edge pixels inside the range at most 1e-4 of the points."""
    import lines_ref as R
    import torch

    B, H, W = LC.tier_shape(tier)
    nws = L.dtfill_line_subsample_workspace_bytes(B, H, W)
    need(2 * 4 * B * H * W + nws + 4 * LC.CHUNK_BYTES, "line_subsample tier %s" % tier)
    x, K, E = synth.velodyne_scan(T, seed=11)
    x[5] = 0  # no point: NO_POINTS, an all-zero frame
    ref, wst, q = R.ref64(x, K, E, 64, 4)
    assert wst.tolist() == [0, 0, 0, 0, 0, R.NO_POINTS]
    with np.errstate(invalid="ignore"):
        edge = np.abs(q - np.round(q)) < 1e-9
        inner = edge & (q > 0) & (q < 64 - 1e-9)
    assert inner.sum() <= 1e-4 * int(np.count_nonzero(x > F(0.1)))
    xd = LC.upload_tiled(x, B, DEV)
    Kd, Ed = LC.upload_tiled(K, B, DEV), LC.upload_tiled(E, B, DEV)
    out, st = poisoned((B, H, W)), poisoned((B,), torch.int32)
    ws, wp = aligned_ws(nws)
    check_rc(L, L.dtfill_line_subsample(xd.data_ptr(), B, H, W, Kd.data_ptr(), Ed.data_ptr(), 64, 4, out.data_ptr(), st.data_ptr(), wp, nws,
                                        _stream()))
    _sync()
    no_mismatch(LC.mismatching_frames(out, _up(ref), B, ignore=_up(edge)), "line_subsample tier %s" % tier)
    no_mismatch(status_mismatch(st, wst, B), "line_subsample status")
    no_mismatch(LC.mismatching_frames(xd, _up(x), B), "line_subsample: x changed")

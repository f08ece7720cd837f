"""The frame facts inside the window kernel's launch (k_fused's window blocks work them out themselves, a frame's first
block publishes them) against the oracle and against DTFILL_FLAG_SEPARATE_FRAME (the k_frame launch of its own), through the raw ABI
on guarded, poisoned buffers (tests/guarded.py, as tests/test_gpu_buffers.py does).

Every case is compared (i) bit for bit with the oracle and (ii) between the two launch sequences: outputs, frame_status and
dtfill_pass_stats must be identical.

Shapes: just above one window tile in each axis (tiles are at most 96 x 160), just below it, and small: 200 x 330,
100 x 170, 40 x 64; and one height on each side of the bound above which a frame does not ride (RIDE_MAX_H rows: 70 columns
wide, to keep them small).  Batches of 3 and 9 frames (no multiples of eight, and above eight); every case alone in a batch,
and all of them mixed in one batch (12 frames; its first nine as a batch of nine as well).

Where a case does not fit a small shape it is clipped to it (bands leave eight rows above and below, a hole five pixels on
every side).  At these sizes a frame of 0.3 % has fewer than 513 sources and would be k_pts's like the "handful" case: at
200 x 330 it holds 100 more sources in one stretch of pixels (more than 96 in a band of 32 rows), which keeps it with the
any-distance kernels and still too thin for a window; at the smaller shapes every frame of more than 96 sources is dense
enough for the halo-32 window, so the frame stays as it is.  Which kernel family took a frame is asserted
(dtfill_pass_stats) where the routing rule leaves no doubt.

Mutation check (run once, on a scratch build with k_mask's clearing of the per-pass flags taken out, the first pass on a
zeroed workspace): test_second_pass_meets_no_stale_flags fails in the two cases that ride (200 x 330 and the height at the bound: the
status keeps what its buffer held) and passes in the four that have a k_frame launch, which stores every word itself (profiles/r05/mutation_check_pytest.txt).  """
import os
import re

import numpy as np
import pytest

from guarded import KINDS, GuardedBuffer, poison, poison_output
from test_gpu_buffers import assert_pass_equals_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OR, SEP = 4, 8  # DTFILL_FLAG_OUTLIER_REMOVAL, DTFILL_FLAG_SEPARATE_FRAME
ALL = ("depth", "dt", "index")
STATS = ("all", "window", "anydist", "sky", "points", "colt")
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtfill.h")
RIDE_MAX_H = int(re.search(r"#define\s+DTFILL_FRAME_RIDE_MAX_H\s+(\d+)", open(_HEADER).read()).group(1))
SHAPES = [(200, 330), (100, 170), (40, 64), (RIDE_MAX_H, 70), (RIDE_MAX_H + 1, 70)]
GENERAL_PATH = 2


# ------------------------------------------------------------------------------------------------ frames
def _depths(rng, n):
    return (np.round(rng.uniform(1.0, 80.0, n) * 256) / 256).astype(np.float32)


def _iid(rng, H, W, p):
    """exactly round(p H W) sources (at least one) at random pixels"""
    a = np.zeros(H * W, np.float32)
    n = max(int(round(p * H * W)), 1)
    pos = rng.choice(H * W, n, replace=False)
    a[pos] = _depths(rng, n)
    return a.reshape(H, W)


def _band(H, n):
    n = min(n, H - 16)
    top = (H - n) // 2
    return top, top + n


def _hole(a, top, rng=None):
    H, W = a.shape
    hh, hw = min(50, H - 10), min(50, W - 10)
    top = min(top, H - hh)
    left = (W - hw) // 2
    a[top:top + hh, left:left + hw] = 0
    return a


def frame(kind, rng, H, W):
    d = lambda: _iid(rng, H, W, 0.05)  # noqa: E731
    if kind == "5%":
        return d()
    if kind == "1.5%":
        return _iid(rng, H, W, 0.015)
    if kind == "0.3%":
        a = _iid(rng, H, W, 0.003)
        if H * W >= 60000:  # more than PTS_BAND_MAX = 96 in one band of 32 rows: not k_pts's, and still too thin for a window
            top = (H // 3) & ~31
            a.reshape(-1)[top * W:top * W + 100] = _depths(rng, 100)
        return a
    if kind == "handful":
        a = np.zeros(H * W, np.float32)
        n = min(60, H * W // 200)
        a[rng.choice(H * W, n, replace=False)] = _depths(rng, n)
        return a.reshape(H, W)
    if kind == "none":
        return np.zeros((H, W), np.float32)
    if kind == "sky30":
        a = d()
        a[:30] = 0
        a[30, W // 2] = 7.5
        return a
    if kind in ("band20", "band40"):
        a = d()
        lo, hi = _band(H, int(kind[4:]))
        a[lo:hi] = 0
        return a
    if kind == "hole":
        return _hole(d(), (H - min(50, H - 10)) // 2)
    if kind == "hole under sky":
        a = d()
        a[:30] = 0
        a = _hole(a, 30)
        a[30, 0] = 7.5  # row r0 = 30 still holds a source, beside the hole
        return a
    if kind == "misaligned":
        a = d()
        a[H // 4, : W // 3] = 0.5  # values that are no sources: the two masks disagree
        a[H // 2, ::7] = 0.25
        return a
    if kind == "negative":
        a = d()
        a[H // 2, W // 2] = -1.0
        a[H // 3, W // 3] = 200.0
        return a
    raise ValueError(kind)


KINDS_OF_FRAME = ("5%", "1.5%", "0.3%", "handful", "none", "sky30", "band20", "band40", "hole", "hole under sky", "misaligned",
                  "negative")


def batch(kind, B, H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([frame(kind, rng, H, W) for _ in range(B)])


def mixed(B, H, W, seed, order=KINDS_OF_FRAME):
    rng = np.random.default_rng(seed)
    return np.stack([frame(order[k % len(order)], rng, H, W) for k in range(B)])


# ------------------------------------------------------------------------------------------------ the rig
class Rig:
    """Guarded x, outputs, status and workspace of one (B, H, W, depth rows): passes run on the same buffers, so that a
    second pass meets the workspace the first one left."""

    def __init__(self, L, B, H, W, row0=0):
        import torch

        self.L, self.shape, self.row0 = L, (B, H, W), row0
        fb = H * W * 4
        self.shapes = {"depth": (B, H - row0, W), "dt": (B, H, W), "index": (B, H, W), "status": (B,)}
        self.dtypes = {"depth": torch.float32, "dt": torch.float32, "index": torch.int32, "status": torch.int32}
        self.x = GuardedBuffer(B * fb, 0, DEV, fb)
        self.bufs = {k: GuardedBuffer(int(np.prod(s)) * 4, 0, DEV, fb) for k, s in self.shapes.items()}
        self.nws = L.dtfill_workspace_bytes(B, H, W, 0)
        assert self.nws > 0
        self.ws = GuardedBuffer(self.nws, 0, DEV, fb)

    def run(self, xh, flags=0, want=ALL, epi=None, ws_poison=None, seed=0):
        import torch

        B, H, W = self.shape
        assert xh.shape == self.shape and (epi[0] if epi else 0) == self.row0
        xv = self.x.view(torch.float32, self.shape)
        xv.copy_(torch.from_numpy(xh))
        for k, g in self.bufs.items():
            poison_output(g.view(self.dtypes[k], self.shapes[k]), k)
        if ws_poison is not None:
            poison(self.ws.payload(), ws_poison, seed)
        ptr = lambda k: self.bufs[k].ptr if k in want else None  # noqa: E731
        st = torch.cuda.current_stream().cuda_stream
        args = [self.x.ptr, B, H, W, 0.1, 0.1, 0, ptr("depth"), ptr("dt"), ptr("index"), self.bufs["status"].ptr, self.ws.ptr, self.nws, st,
                flags]
        if epi is not None:
            rc = self.L.dtfill_batch_epilogue(*args, epi[0], int(epi[1] is not None), float(epi[1] or 0.0))
        else:
            rc = self.L.dtfill_batch_flags(*args)
        assert rc == 0, self.L.dtfill_strerror(rc)
        stats = torch.zeros(len(STATS), dtype=torch.int64, device=DEV)
        assert self.L.dtfill_pass_stats(self.ws.ptr, self.nws, B, H, W, 0, stats.data_ptr(), st) == 0
        torch.cuda.synchronize()
        for k, g in self.bufs.items():
            g.check(k)
        self.ws.check("workspace")
        self.x.check("x")
        assert np.array_equal(xv.cpu().numpy().view(np.uint32), xh.view(np.uint32)), "x was written"
        out = {k: self.bufs[k].view(self.dtypes[k], self.shapes[k]).cpu().numpy() for k in tuple(want) + ("status",)}
        return out, dict(zip(STATS, stats.cpu().tolist()))


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.load()


_rigs = {}


def rig(L, B, H, W, row0=0):
    key = (B, H, W, row0)
    if key not in _rigs:
        _rigs[key] = Rig(L, B, H, W, row0)
    return _rigs[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_rigs():
    yield
    _rigs.clear()


def both_ways(L, oracle, x, what, flags=0, want=ALL, epi=None, seed=0, ref=None):
    """x through the default sequence and through DTFILL_FLAG_SEPARATE_FRAME, each on a freshly poisoned workspace: both equal
    the oracle, and each other in outputs, status and pass statistics.  Returns (outputs, stats) of the default sequence."""
    B, H, W = x.shape
    if ref is None:
        xin = np.stack([oracle.outlier_removal(f) for f in x]).astype(np.float32) if flags & OR else x
        ref = oracle.fill_batch(xin)
    r = rig(L, B, H, W, epi[0] if epi else 0)
    got = []
    for k, f in enumerate((flags, flags | SEP)):
        out, stats = r.run(x, f, want, epi, KINDS[(seed + k) % 3], seed)
        assert_pass_equals_oracle(out, ref, 0, f, want, epi, "%s flags=%d" % (what, f))
        assert stats["all"] == B * H * W and stats["window"] + stats["anydist"] + stats["sky"] + stats["points"] == stats["all"], (what, stats)
        got.append((out, stats))
    (a, sa), (b, sb) = got
    assert sa == sb, "%s: pass statistics differ: %s (default) / %s (separate k_frame)" % (what, sa, sb)
    assert np.array_equal(a["status"], b["status"]), "%s: status %s / %s" % (what, a["status"], b["status"])
    for k in want:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs between the two sequences" % (what, k)
    return a, sa


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_case_alone(L, oracle, hw):
    """Every case in a batch of its own: three frames, and nine at the shape just above one tile."""
    H, W = hw
    for k, kind in enumerate(KINDS_OF_FRAME):
        for B in ((3, 9) if hw == SHAPES[0] else (3,)):
            x = batch(kind, B, H, W, 1000 + 10 * k + B)
            what = "%s, %d frames of %dx%d" % (kind, B, H, W)
            flags = OR if kind == "negative" else 0
            out, stats = both_ways(L, oracle, x, what, flags, seed=k + B)
            px = B * H * W
            if kind == "5%":
                assert stats["window"] == px and not out["status"].any(), (what, stats, out["status"])
            if kind == "none" or (H * W >= 60000 and kind == "0.3%"):
                assert stats["anydist"] == px, (what, stats)
            if hw == SHAPES[0] and kind in ("handful", "1.5%"):
                assert stats["points" if kind == "handful" else "window"] == px, (what, stats)
            if kind == "sky30" and H >= 100:
                assert stats["sky"] == B * 30 * W, (what, stats)
            if kind == "hole under sky" and H >= 100:
                assert stats["sky"] == 0 and stats["anydist"] >= B * 32 * W, (what, stats)  # the sky was called off
            if kind in ("hole", "band20", "band40") and H >= 100:
                assert 0 < stats["anydist"] < px and (out["status"] & GENERAL_PATH).all(), (what, stats)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_all_cases_mixed_in_one_batch(L, oracle, hw):
    """All twelve frames in one batch (and its first nine), plain, with the outlier filter, with a depth epilogue (the EPI
    instance of k_fused: no row flags) and without a distance map from the caller."""
    H, W = hw
    x = mixed(12, H, W, 77)
    ref = oracle.fill_batch(x)
    both_ways(L, oracle, x, "mixed 12 of %dx%d" % hw, ref=ref, seed=1)
    both_ways(L, oracle, x[:9].copy(), "mixed 9 of %dx%d" % hw, ref=tuple(v[:9] for v in ref), seed=2)
    both_ways(L, oracle, x, "mixed 12 of %dx%d, outlier filter" % hw, OR, seed=3)
    both_ways(L, oracle, x, "mixed 12 of %dx%d, out_dt NULL" % hw, want=("depth", "index"), ref=ref, seed=4)
    both_ways(L, oracle, x, "mixed 12 of %dx%d, only out_dt" % hw, want=("dt",), ref=ref, seed=5)
    for epi in ((17, None), (0, 0.9)):
        both_ways(L, oracle, x, "mixed 12 of %dx%d, epilogue %s" % (hw + (epi,)), epi=epi, ref=ref, seed=6)


@pytest.mark.parametrize("hw", SHAPES[:1] + SHAPES[3:], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flags", [0, SEP], ids=["ride", "separate"])
def test_second_pass_meets_no_stale_flags(L, oracle, hw, flags):
    """Two passes on one workspace, the frames swapping roles: what was a sky, a band, a hole (row flags 1 and 2, fflag2, the
    general-path status, a sky called off) is a clean dense frame in the second pass and the other way round.  The second
    pass equals the oracle, and its dense frames are all the window kernel's with status 0: nothing of the first pass's
    flags survives (k_mask clears them; the publishing block and the window blocks only raise)."""
    H, W = hw
    first = ("sky30", "hole", "hole under sky", "band40", "5%", "0.3%", "5%", "handful", "5%")
    second = ("5%", "5%", "5%", "5%", "sky30", "5%", "hole under sky", "5%", "hole")
    B = len(first)
    x1, x2 = mixed(B, H, W, 5, first), mixed(B, H, W, 6, second)
    r = rig(L, B, H, W)
    out1, st1 = r.run(x1, flags, ALL, None, "random", 9)
    assert_pass_equals_oracle(out1, oracle.fill_batch(x1), 0, flags, ALL, None, "first pass")
    assert (out1["status"][[0, 1, 2, 3, 5, 7]] & GENERAL_PATH).all() and st1["sky"] == 30 * W, (out1["status"], st1)
    out2, st2 = r.run(x2, flags, ALL, None, None)  # the workspace as the first pass left it
    assert_pass_equals_oracle(out2, oracle.fill_batch(x2), 0, flags, ALL, None, "second pass")
    dense = [k for k, kind in enumerate(second) if kind == "5%"]
    assert not out2["status"][dense].any(), "stale status: %s" % out2["status"]
    assert (out2["status"][[4, 6, 8]] == GENERAL_PATH).all(), out2["status"]
    # frame 4's sky is k_sky's, frame 6's is called off; every other row that is not in or near a hole is the window kernel's
    assert st2["sky"] == 30 * W and st2["points"] == 0 and st2["window"] >= (len(dense) * H + 2 * (H - 30 - 60)) * W, st2
    # ... and the same frames as a first pass on a clean workspace leave the same statistics
    out3, st3 = r.run(x2, flags, ALL, None, "zero")
    assert st3 == st2 and np.array_equal(out3["status"], out2["status"]), (st2, st3)


@pytest.mark.parametrize("hw", SHAPES[:1] + SHAPES[3:], ids=lambda s: "%dx%d" % s)
def test_k_frame_slot_of_the_timed_pass(L, hw):
    """dtfill_batch_timed says which sequence ran: without the flag a frame of up to DTFILL_FRAME_RIDE_MAX_H rows has no
    k_frame launch (the slot reads exactly 0 ms, as that of any kernel that does not run), with DTFILL_FLAG_SEPARATE_FRAME,
    on the forced any-distance path and above the bound it has one (two events around a launch are microseconds apart)."""
    import ctypes

    import torch

    H, W = hw
    r = rig(L, 3, H, W)
    x = batch("5%", 3, H, W, 31)
    r.x.view(torch.float32, r.shape).copy_(torch.from_numpy(x))
    nk = L.dtfill_num_kernels(0)
    names = [L.dtfill_kernel_name(0, k).decode() for k in range(nk)]

    def slots(flags):
        ms = (ctypes.c_float * nk)(*([-1.0] * nk))
        rc = L.dtfill_batch_timed(r.x.ptr, 3, H, W, 0.1, 0.1, 0, r.bufs["depth"].ptr, r.bufs["dt"].ptr, r.bufs["index"].ptr,
                                  r.bufs["status"].ptr, r.ws.ptr, r.nws, torch.cuda.current_stream().cuda_stream, flags,
                                  ctypes.cast(ms, ctypes.c_void_p))
        assert rc == 0, L.dtfill_strerror(rc)
        torch.cuda.synchronize()
        return dict(zip(names, [float(v) for v in ms]))

    rides = H <= RIDE_MAX_H
    t = slots(0)
    assert (t["k_frame"] == 0.0) == rides and t["k_fused"] > 0.0 and t["k_mask"] > 0.0, (hw, t)
    assert slots(SEP)["k_frame"] > 0.0
    assert slots(1)["k_frame"] > 0.0  # DTFILL_FLAG_GENERAL_ONLY


def test_late_blocks_of_many_small_frames(L, oracle):
    """Many small frames in one batch, passes repeated: every block of the launch is resident together with the frames' first
    blocks, so the blocks beyond the tiling with fewer tiles look at route[b] just while it is being published.  Whatever a
    block sees there, it stays or leaves whole: halo-32 frames (whose late blocks have to work), k_pts frames and halo-16
    frames (whose late blocks leave), interleaved, equal the oracle in every pass."""
    H, W, B = 100, 170, 96
    x = mixed(B, H, W, 123, ("1.5%", "handful", "5%", "1.5%", "none", "hole"))
    ref = oracle.fill_batch(x)
    r = rig(L, B, H, W)
    first = None
    for k in range(12):
        out, stats = r.run(x, 0, ALL, None, KINDS[k % 3] if k % 4 == 0 else None, k)
        assert_pass_equals_oracle(out, ref, 0, 0, ALL, None, "pass %d" % k)
        first = first or (out["status"].copy(), stats)
        assert np.array_equal(out["status"], first[0]) and stats == first[1], (k, stats, first[1])

"""The side entry points on the device against the literal references of tests/gmc_ref.py and tests/post_ref.py (not the
oracle): dtfill_generate_multi_channel (k_gmc7, k_gmc) step by step, dtfill_crop_floor and dtfill_png16 on special values
and at their grid limits, the depth floor folded into dtfill_batch_epilogue, and dtfill_metrics against math.fsum.

Bars:
  gmc          one selected tap: bit-exact (+0 and -0 equal); more: within gmc_ref.sum_bound(), the float32 summation error
  crop, png16  bit-exact; NaN compares as NaN after the floor, identity crops compare raw bits
  epilogue     bit-exact against the literal floor of the oracle's fill
  metrics      count and delta1..3 exactly k / count; the other columns within 1e-12 relative where the reference is finite
               (the device sums the same float32 terms in float64), the same NaN or inf where it is not"""
import itertools
import math

import numpy as np
import pytest

import gmc_ref as G
import post_ref as P
from guarded import poison_op, poison_value

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLE_SIZES = (1, 3, 5, 7, 9, 11, 13, 15)
_POISON = itertools.count(7100)  # seeds (and so kinds) of the fill's poisoned buffers
GMC_SHAPES = ((1, 1, 1), (2, 1, 97), (2, 97, 1), (1, 15, 63), (2, 16, 64), (2, 17, 65), (1, 33, 130), (2, 70, 150))


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(shape, value=None):
    """A float32 device buffer holding what no pass may leave behind: by default the depth poison NaN (gmc of finite data is
    finite), or `value`."""
    import torch

    return torch.full(shape, float(poison_value("depth")) if value is None else value, dtype=torch.float32, device=DEV)


def _check(L, rc):
    assert rc == 0, L.dtfill_strerror(rc).decode()


# ---------------------------------------------------------------- generate_multi_channel

def gmc_device(L, x, m, ts, sn):
    """The outputs lidar_2 .. lidar_sn of one dtfill_generate_multi_channel call, from poisoned buffers."""
    import torch

    xd, md = _up(x), _up(m)
    outs = [_poisoned(x.shape) for _ in range(3)]
    ptrs = [o.data_ptr() if k < sn - 1 else None for k, o in enumerate(outs)]
    _check(L, L.dtfill_generate_multi_channel(xd.data_ptr(), md.data_ptr(), *x.shape, ts, sn, *ptrs, _stream()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs[: sn - 1]]


@pytest.mark.parametrize("ts", TABLE_SIZES)
def test_gmc_every_step_vs_literal_ref(L, ts):
    """Each step on its own: step 1 from the caller's data and mask, step k from the device's step k - 1 output and that
    output > 0.001 (so k_gmc7's values carried forward from step k - 1 into steps k and k + 1 are checked where they land).
    Every mask kind -- 0 / 1 from the data or not, fractional, negative everywhere / in a band / in one tap, -0.0, all zero --
    on every shape: single pixels and rows, one tile exactly, a tile plus one, frames of several tiles; scale_num 1 .. 3 must
    give the first outputs of scale_num 4 bit for bit."""
    rng = np.random.default_rng(300 + ts)
    shapes = GMC_SHAPES + (((1, 256, 1216),) if ts == 7 else ())
    for si, shape in enumerate(shapes):
        for mi, mk in enumerate(G.MASK_KINDS):
            dk = G.DATA_KINDS[(mi + si) % len(G.DATA_KINDS)]
            x = G.make_data(dk, rng, shape)
            m = G.make_mask(mk, rng, x)
            outs = gmc_device(L, x, m, ts, 4)
            data, mask = x, m
            for k, got in enumerate(outs):
                G.assert_step_matches(got, *G.gmc_step(data, mask, ts), what="ts %d %s %s/%s lidar_%d" % (ts, shape, mk, dk, k + 2))
                data, mask = got, G.next_mask(got)
            for sn in (1, 2, 3):
                for k, got in enumerate(gmc_device(L, x, m, ts, sn)):
                    assert np.array_equal(got.view(np.uint32), outs[k].view(np.uint32)), (ts, shape, mk, dk, sn, k)


# ---------------------------------------------------------------- crop_floor, png16

CROP_WIDTHS = (1, 255, 256, 257, 2048, 2049, 5000)
CROP_POISON = -1234.5  # neither an input below nor a floor of one (>= the floor, or NaN)
FLOORS = (None, 0.9, 0.0, 1.5)
PNG_SCALES = ((0.0, 100.0, 256.0), (0.9, 255.99609375, 256.0), (0.0, 1.0, 65535.0), (0.0, 65535.0, 1.0))


def _on_scale(scale, rng, n):
    """Values whose float32 product with scale is an integer, and the values 1 ulp below them."""
    k = rng.integers(1, 60000, 4 * n).astype(np.float64)
    v = (k / scale).astype(np.float32)
    v = v[(v * np.float32(scale)) == np.round(v * np.float32(scale))][:n]
    return np.concatenate([v, np.nextafter(v, np.float32(0))])


def special_frames(rng, B, H, W):
    """Depths in [-5, 130) with a third of the pixels special: NaN (two payloads, both signs), +-inf, +-0, 0.9f and its
    neighbours, 1.5f, subnormals, and values on the uint16 grid of every PNG scale and 1 ulp below them."""
    x = rng.uniform(-5, 130, (B, H, W)).astype(np.float32)
    nan_bits = np.uint32([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7FA00001]).view(np.float32)
    f9 = np.float32(0.9)
    sp = [nan_bits, np.float32([np.inf, -np.inf, 0.0, -0.0, f9, np.nextafter(f9, np.float32(1)), np.nextafter(f9, np.float32(0)),
                                1.5, 1e-40, -1e-40, 100.0, 3e38])]
    sp += [_on_scale(s, rng, 16) for _, _, s in PNG_SCALES]
    sp = np.concatenate(sp).astype(np.float32)
    pick = rng.random(x.shape) < 1 / 3
    x[pick] = rng.choice(sp, int(pick.sum()))
    x.reshape(-1)[: min(x.size, sp.size)] = sp[: min(x.size, sp.size)]  # every special at least once where there is room
    return x


def _same(got, want):
    """bit-exact, NaN equal to NaN"""
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def crop_device(L, xd, shape, r0, r1, c0, c1, floor):
    import torch

    B = shape[0]
    out = _poisoned((B, r1 - r0, c1 - c0), CROP_POISON)
    _check(L, L.dtfill_crop_floor(xd.data_ptr(), *shape, r0, r1, c0, c1, int(floor is not None), float(floor or 0.0),
                                  out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def png_device(L, xd, shape, pad_top, floor, lo, hi, scale):
    import torch

    B, H, W = shape
    out = torch.full((B, H + pad_top, W), 0xA5A5 - 0x10000, dtype=torch.int16, device=DEV).view(torch.uint16)
    _check(L, L.dtfill_png16(xd.data_ptr(), B, H, W, pad_top, int(floor is not None), float(floor or 0.0), lo, hi, scale,
                             out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _crops(H, W):
    """The whole frame, its corners and edges, its interior, one column at each side."""
    h, w = max(1, H // 2), max(1, W // 3)
    c = {(0, H, 0, W), (0, h, 0, w), (H - h, H, W - w, W), (0, H, W - 1, W), (H - 1, H, 0, W), (0, 1, 0, 1)}
    if H > 2 and W > 2:
        c.add((1, H - 1, 1, W - 1))
    return sorted(c)


@pytest.mark.parametrize("W", CROP_WIDTHS)
def test_crop_floor_special_values(L, W):
    """Rows wider than one pass of k_crop_floor's grid (8 blocks of 256 columns) take its column loop."""
    rng = np.random.default_rng(400 + W)
    shape = (2, 5, W)
    x = special_frames(rng, *shape)
    xd = _up(x)
    for r0, r1, c0, c1 in _crops(5, W):
        sub = x[:, r0:r1, c0:c1]
        for floor in FLOORS:
            got = crop_device(L, xd, shape, r0, r1, c0, c1, floor)
            if floor is None:  # identity: raw bits, NaN payloads included
                assert np.array_equal(got.view(np.uint32), sub.view(np.uint32)), (W, r0, r1, c0, c1)
            else:
                assert _same(got, P.depth_floor(sub, floor)), (W, r0, r1, c0, c1, floor)


@pytest.mark.parametrize("W", CROP_WIDTHS)
def test_png16_special_values(L, W):
    rng = np.random.default_rng(500 + W)
    shape = (2, 4, W)
    x = special_frames(rng, *shape)
    xd = _up(x)
    for pad_top in (0, 1, 96):
        for floor in FLOORS:
            for lo, hi, scale in PNG_SCALES:
                got = png_device(L, xd, shape, pad_top, floor, lo, hi, scale)
                for b in range(2):
                    want = P.png16(x[b], pad_top, floor, lo, hi, scale)
                    assert np.array_equal(got[b], want), (W, pad_top, floor, lo, hi, scale, b)


def test_crop_floor_and_png16_at_the_grid_y_limit(L):
    """65535 output rows: grid y at its limit (crop_floor: OH; png16: H + pad_top), both with W <= 3."""
    rng = np.random.default_rng(600)
    x = special_frames(rng, 1, 65535, 3)
    xd = _up(x)
    got = crop_device(L, xd, x.shape, 0, 65535, 1, 3, 0.9)
    assert _same(got, P.depth_floor(x[:, :, 1:3], 0.9))
    assert np.array_equal(crop_device(L, xd, x.shape, 0, 65535, 0, 3, None).view(np.uint32), x.view(np.uint32))
    H = 65535 - 96
    y = np.ascontiguousarray(x[:, :H, :2])
    got = png_device(L, _up(y), y.shape, 96, 0.9, 0.0, 100.0, 256.0)
    assert got.shape == (1, 65535, 2) and np.array_equal(got[0], P.png16(y[0], 96, 0.9))


# ---------------------------------------------------------------- the depth floor of dtfill_batch_epilogue

def test_epilogue_floor_of_negative_and_infinite_depths(gpu_op, oracle):
    """val_thr = -1 makes zeros and negative pixels values, so the gather hands out depths <= 0 (the value list no longer lines
    up with the sources); +inf sources hand out +inf.  Both kernel families' depth stores must apply the literal floor."""
    import torch

    rng = np.random.default_rng(700)
    dense = np.where(rng.random((2, 64, 200)) < 0.3, rng.uniform(0.2, 40, (2, 64, 200)), 0).astype(np.float32)
    sparse = np.where(rng.random((2, 97, 130)) < 0.01, rng.uniform(0.2, 40, (2, 97, 130)), 0).astype(np.float32)
    for x in (dense, sparse):
        x[rng.random(x.shape) < 0.02] = np.inf
        neg = rng.random(x.shape) < 0.1
        x[neg] = rng.choice(np.float32([-0.5, -0.0, -0.95, -3.0]), int(neg.sum()))
        depth, _, _, status = oracle.fill_batch(x, 0.1, -1.0)
        assert not status.any() and (depth < 0).any() and np.isinf(depth).any()
        for r0, fl in ((0, 0.9), (17, 0.0), (1, 1.5)):
            want = P.depth_floor(depth[:, r0:], fl)
            for path in ("auto", "general"):
                xd = _up(x)
                poison_op(gpu_op, next(_POISON), x.shape, path=path, depth_rows_from=r0)
                res = gpu_op.run(xd, 0.1, -1.0, want=("depth",), path=path, depth_rows_from=r0, depth_floor=fl)
                torch.cuda.synchronize()
                got = res["depth"].cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (x.shape, r0, fl, path)


# ---------------------------------------------------------------- metrics

METRIC_NS = (1, 3, 1023, 1024, 1025, 65535, 65536, 65537, 352 * 1216, 3 * 2 ** 20 + 7)
_G = np.float32(0.01)
EDGES = (np.nan, 0.0, -0.0, _G, np.nextafter(_G, np.float32(1)), 1e-40)  # the gate's edges (a NaN is gated out)
HUGE = (np.inf, 1e30)  # +inf, and 1e30: its KITTI square overflows float32 -- either makes a column inf or NaN


def metric_frames(rng, B, n, specials):
    """Depth pairs around 10 % apart with half the targets missing; unless specials is None, up to 64 places per frame hold
    one of `specials` (in the output or the target) or a pair whose ratio is exactly 1.25, 1.5625 or 1.953125 or 1 ulp
    below, in either order."""
    gt = rng.uniform(0.5, 80, (B, n)).astype(np.float32)
    pred = (gt * (1 + 0.1 * rng.standard_normal((B, n)))).astype(np.float32)
    gt[rng.random((B, n)) < 0.5] = 0
    if specials is None:
        return pred, gt
    for b in range(B):
        for p in rng.choice(n, min(n, 64), replace=False):
            kind = rng.integers(0, 3)
            if kind < 2:
                (pred if kind == 0 else gt)[b, p] = rng.choice(np.float32(specials))
            else:
                r = np.float32(rng.choice([1.25, 1.5625, 1.953125]))
                if rng.random() < 0.5:
                    r = np.nextafter(r, np.float32(0))
                t = np.float32(2.0 ** rng.integers(-2, 5))  # a power of two: t * r / t is exactly r
                pred[b, p], gt[b, p] = (t * r, t) if rng.random() < 0.5 else (t, t * r)
    return pred, gt


def metrics_device(L, pred, gt, kind):
    import torch

    B, n = pred.shape
    ws_bytes = L.dtfill_metrics_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((B, len(P.COLUMNS)), float(poison_value("depth")), dtype=torch.float64, device=DEV)
    od, td = _up(pred), _up(gt)
    _check(L, L.dtfill_metrics(od.data_ptr(), td.data_ptr(), B, n, kind, out.data_ptr(), ws.data_ptr(), ws_bytes, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_metrics_row(row, want, what):
    got = dict(zip(P.COLUMNS, row.tolist()))
    for k in P.COLUMNS:
        g, w = got[k], want[k]
        if k in ("count", "delta1", "delta2", "delta3"):
            assert g == w or (math.isnan(g) and math.isnan(w)), (what, k, g, w)
        elif math.isfinite(w):
            assert abs(g - w) <= 1e-12 * abs(w), (what, k, g, w)
        else:
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, k, g, w)


@pytest.mark.parametrize("n", METRIC_NS)
def test_metrics_vs_fsum(L, pkg, n):
    """Three frames: every special value; the finite ones only, so that each column stays finite and carries every element's
    rounding (an FMA in a term moves a mean by ~1e-8); plain pairs."""
    rng = np.random.default_rng(800 + n % 1000)
    frames = [metric_frames(rng, 1, n, sp) for sp in (EDGES + HUGE, EDGES, None)]
    pred, gt = np.concatenate([f[0] for f in frames]), np.concatenate([f[1] for f in frames])
    for kind, ref in ((pkg._lib.METRICS_KITTI, P.evaluate_kitti), (pkg._lib.METRICS_NYU, P.evaluate_nyu)):
        rows = metrics_device(L, pred, gt, kind)
        for b in range(3):
            want = ref(pred[b], gt[b])
            assert b == 0 or n < 1000 or all(math.isfinite(v) for v in want.values()), (n, kind, b, want)
            assert_metrics_row(rows[b], want, (n, kind, b))


def test_metrics_many_short_frames(L, pkg):
    """B = 300 frames of 5 elements: one block row per frame, most frames holding a special value."""
    rng = np.random.default_rng(900)
    pred, gt = metric_frames(rng, 300, 5, EDGES + HUGE)
    for kind, ref in ((pkg._lib.METRICS_KITTI, P.evaluate_kitti), (pkg._lib.METRICS_NYU, P.evaluate_nyu)):
        rows = metrics_device(L, pred, gt, kind)
        with np.errstate(all="ignore"):
            for b in range(300):
                assert_metrics_row(rows[b], ref(pred[b], gt[b]), (kind, b))

"""demo.py's value-weighted multi-channel fill without a GPU: the literal reference of tests/gmcv_ref.py on hand cases (what
the device tests compare against has to be right first), the argument checks and the workspace sizing of the new ABI entry
points (all made before any HIP call), and the numpy shim's refusal to compute anything on the CPU."""
import numpy as np
import pytest

import gmcv_ref as V

F = np.float32


def one(frame, ts=7):
    """raw_2 and the count of one [H,W] frame."""
    raw, cnt = V.step(np.asarray(frame, F)[None], ts)
    return raw[0], cnt[0]


def quot(total, n):
    return F(total) / (F(0.000001) + F(n))


@pytest.mark.parametrize("ts", (7, 11, 15))
def test_weight_table(ts):
    """10^(ts - |di| - |dj|): the double power is exact, the float32 is its one rounding (exact up to 10^10 only)."""
    w = V.create_weight_matrix(ts).reshape(ts, ts)
    half = (ts - 1) // 2
    assert w.dtype == np.float32
    for i in range(ts):
        for j in range(ts):
            e = ts - abs(i - half) - abs(j - half)
            assert 1 <= e <= ts
            assert w[i, j] == F(float(10 ** e)), (i, j)  # 10 ** e: a Python int, converted to double exactly, rounded once
            assert (int(w[i, j]) == 10 ** e) == (e <= 10), (i, j, e)
    assert w[half, half] == F(float(10 ** ts)) and w[0, half] == w[half, 0] == F(float(10 ** (half + 1)))
    assert w[0, 0] == w[0, -1] == w[-1, 0] == w[-1, -1] == F(10.0)


def test_farther_but_larger_depth_wins():
    x = np.zeros((15, 15), F)
    x[7, 8], x[9, 7] = 1.0, 80.0  # distance 1 and distance 2 of (7, 7): 1e6 against 80e5
    raw, cnt = one(x)
    assert raw[7, 7] == quot(80.0, 1) and cnt[7, 7] == 1
    x[9, 7] = 8.0  # 8e5 < 1e6: now the nearer one
    raw, cnt = one(x)
    assert raw[7, 7] == quot(1.0, 1) and cnt[7, 7] == 1


def test_cross_ring_tie():
    x = np.zeros((15, 15), F)
    x[6, 7], x[8, 8] = 2.5, 25.0  # 2.5e6 == 25.0e5: both selected
    raw, cnt = one(x)
    assert cnt[7, 7] == 2 and raw[7, 7] == quot(F(2.5) + F(25.0), 2)
    assert abs(float(raw[7, 7]) - 13.75) < 1e-4


def test_checkerboard_ties():
    ii, jj = np.indices((9, 9))
    x = np.where((ii + jj) % 2 == 0, 4.0, 0.0).astype(F)
    raw, cnt = one(x)
    assert cnt[4, 3] == 4 and raw[4, 3] == quot(16.0, 4)  # interior zero: four neighbours at distance 1
    assert cnt[0, 3] == 3 and raw[0, 3] == quot(12.0, 3)  # top edge: three
    assert cnt[0, 1] == 3 and cnt[8, 7] == 3
    y = np.where((ii + jj) % 2 == 1, 4.0, 0.0).astype(F)
    raw, cnt = one(y)
    assert cnt[0, 0] == 2 and raw[0, 0] == quot(8.0, 2)  # corner zero: two
    assert cnt[4, 4] == 4
    raw, cnt = one(x)
    assert cnt[4, 4] == 1 and raw[4, 4] == quot(4.0, 1)  # a data pixel is its own maximum


def test_empty_window_is_zero():
    x = np.zeros((20, 20), F)
    x[0, 0] = 5.0
    raw, cnt = one(x)
    assert cnt[10, 10] == 0 and raw[10, 10] == 0 and not np.signbit(raw[10, 10])
    assert cnt[19, 19] == 0 and raw[19, 19] == 0
    raw, cnt = one(np.zeros((1, 1), F), ts=15)
    assert cnt[0, 0] == 0 and raw[0, 0] == 0


def test_negative_interior_window():
    """No zero in the window: the maximum is the largest (least negative) product, not a padding zero."""
    x = np.full((9, 9), -2.0, F)
    x[4, 5] = -1.0
    raw, cnt = one(x)
    # centre (4, 4): own tap -2e7, (4, 5) -1e6; the corners of the window give -2e1, the largest product: four of them
    assert cnt[4, 4] == 4 and raw[4, 4] == quot(-8.0, 4)
    # near the border a padding tap (p = 0) wins: selected taps hold 0, the count is 0 and the result 0
    assert cnt[0, 0] == 0 and raw[0, 0] == 0


def test_no_remasking_between_steps():
    """net.py's form re-masks with > 0.001 between the steps; demo.py's does not: 0.0005 is carried on."""
    x = np.zeros((1, 21, 21), F)
    x[0, 10, 10] = 0.0005
    raws = V.chain(x, 7, 4)
    assert raws[1][0, 10, 12] == quot(0.0005, 1) and raws[1][0, 10, 14] == 0
    assert raws[2][0, 10, 15] > 0 and raws[2][0, 10, 15] <= F(0.0005)  # step 3 reaches three further
    assert raws[3][0, 10, 18] > 0 and raws[3][0, 10, 19] > 0 and raws[3][0, 10, 20] == 0


def test_image_form_divides_lidar_twice():
    rng = np.random.default_rng(5)
    x = V.make_data("sparse", rng, (2, 12, 20))
    rgb = rng.uniform(0, 255, (2, 12, 20, 3)).astype(F)
    plain = V.generate_multi_channel(x[..., None], 7, 90.0, 3)
    img = V.generate_multi_channel_with_image(rgb, x[..., None], 7, 90.0, 3)
    assert plain[3] is None and img[3] is None
    for k in range(3):
        assert img[k].shape == (2, 12, 20, 4) and img[k].dtype == np.float32
        assert np.array_equal(img[k][..., :3], rgb / F(90.0))  # rgb: once
        assert np.array_equal(img[k][..., 3], plain[k] / F(90.0))  # lidar: twice, both roundings kept
    assert np.array_equal(plain[0], x / F(90.0))
    raws = V.chain(x, 7, 3)
    assert any(not np.array_equal((r / F(90.0)) / F(90.0), r / F(8100.0)) for r in raws), "the two roundings are visible"
    one_ = V.generate_multi_channel(x[..., None], 7, 1.0, 3)
    for k in range(3):
        assert np.array_equal(one_[k], raws[k])  # scale_range 1: the raw steps


def test_planted_cases_are_what_they_say():
    """The blocks gmcv_ref.plant() writes give the counts the GPU tests rely on seeing."""
    x = V.plant(np.zeros((1, 40, 120), F), 7)
    raw, cnt = V.step(x, 7)
    S, m = 17, 8
    at = lambda k: (0, (k // 7) * S + m, (k % 7) * S + m)
    assert raw[at(0)] == quot(80.0, 1)
    assert cnt[at(1)] == 2
    assert cnt[0, m, 2 * S + m] == 1 and cnt[0, m, 2 * S + m + 1] == 4
    assert cnt[at(3)] == 0 and raw[at(3)] == 0
    assert raw[at(4)] < 0
    assert raw[at(5)] == quot(0.0005, 1)


# ---------------------------------------------------------------- the ABI without a GPU

def test_argument_errors(pkg):
    """Every argument check of dtfill_demo_multi_channel comes before any HIP call."""
    L = pkg.load()
    P = 256  # stands for a valid, aligned device pointer: no call below gets as far as using it
    f = L.dtfill_demo_multi_channel
    ok = dict(lidar=P, rgb=None, C=0, B=1, H=8, W=8, ts=7, sn=4, sr=90.0, o1=P, o2=P, o3=P, o4=P, ws=P, nb=1 << 20, st=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["lidar"], a["rgb"], a["C"], a["B"], a["H"], a["W"], a["ts"], a["sn"], a["sr"], a["o1"], a["o2"], a["o3"],
                 a["o4"], a["ws"], a["nb"], a["st"])

    NULL, SHAPE, WORKSPACE = -1, -2, -3
    assert call(lidar=None) == NULL
    for k in ("o1", "o2", "o3", "o4"):
        assert call(**{k: None}) == NULL, k
    assert call(sn=3, o3=None) == NULL and call(sn=2, o2=None) == NULL and call(sn=1, o1=None) == NULL
    assert call(ws=None) == NULL and call(sn=3, o4=None, ws=None) == NULL  # a later step reads raw_2: workspace needed
    for ts in (0, 2, 6, 16, 17, -1, -7):
        assert call(ts=ts) == SHAPE, ts
    for sn in (0, 5, -1):
        assert call(sn=sn) == SHAPE, sn
    for sr in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        assert call(sr=sr) == SHAPE, sr
    assert call(rgb=P, C=0) == SHAPE and call(rgb=P, C=-3) == SHAPE
    for k in ("B", "H", "W"):
        assert call(**{k: 0}) == SHAPE and call(**{k: -4}) == SHAPE, k
    assert call(B=1 << 15, H=1 << 8, W=1 << 8) == SHAPE  # B*H*W = 2^31
    assert call(B=1 << 13, H=1 << 8, W=1 << 8, rgb=P, C=3) == SHAPE  # B*H*W*(C+1) = 2^31
    M = 2 ** 31 - 1  # products that do not fit 64 bits are rejected like any other
    assert call(B=M, H=M, W=M) == SHAPE and call(B=M, H=M, W=M, rgb=P, C=M) == SHAPE and call(rgb=P, C=M) == SHAPE
    assert call(B=3, H=M, W=1) == SHAPE and call(B=1, H=1, W=M // 4 + 1, rgb=P, C=3) == SHAPE
    need = L.dtfill_demo_multi_channel_workspace_bytes(1, 8, 8, 4)
    assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    assert call(ws=P + 4) == WORKSPACE and call(ws=P + 128) == WORKSPACE
    # the first failed check decides
    assert call(lidar=None, ts=6) == NULL and call(ts=6, nb=0) == SHAPE


def test_workspace_sizing(pkg):
    L = pkg.load()
    f = L.dtfill_demo_multi_channel_workspace_bytes
    frame = lambda B, H, W: (B * H * W * 4 + 255) // 256 * 256
    for B, H, W in ((1, 1, 1), (1, 8, 8), (3, 17, 65), (32, 256, 1216)):
        assert f(B, H, W, 1) == 0 and f(B, H, W, 2) == 0  # no step's raw result is read again
        assert f(B, H, W, 3) == frame(B, H, W)
        assert f(B, H, W, 4) == 2 * frame(B, H, W)
    for bad in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, -1, 4), (1, 8, 8, 0), (1, 8, 8, 5), (1 << 15, 1 << 8, 1 << 8, 4)):
        assert f(*bad) == 0, bad
    assert f(70000, 4, 4, 4) == 2 * frame(70000, 4, 4)  # B is no grid dimension here
    M = 2 ** 31 - 1
    assert f(M, M, M, 4) == 0 and f(2, M, 1, 4) == 0 and f(M, 1, 2, 3) == 0
    assert f(M, 1, 1, 3) == frame(M, 1, 1) and f(1 << 15, 1 << 8, (1 << 8) - 1, 4) == 2 * frame(1 << 15, 1 << 8, (1 << 8) - 1)


def test_demo_module_mirrors_the_reference(pkg):
    assert pkg.demo.create_weight_matrix.__defaults__ == (11,)
    for ts in (1, 3, 7, 11, 15):
        assert np.array_equal(pkg.demo.create_weight_matrix(ts), V.create_weight_matrix(ts))
    with pytest.raises(AssertionError):
        pkg.demo.create_weight_matrix(6)
    x = np.zeros((1, 4, 4, 1), F)
    for sn in (0, 5):
        with pytest.raises(ValueError, match="scale_num"):
            pkg.demo.generate_multi_channel(x, 7, scale_num=sn)
        with pytest.raises(ValueError, match="scale_num"):
            pkg.demo.generate_multi_channel_with_image(np.zeros((1, 4, 4, 3), F), x, 7, scale_num=sn)
    # the net.py form keeps the top-level name
    assert pkg.generate_multi_channel is not pkg.demo.generate_multi_channel
    assert pkg.generate_multi_channel.__module__.endswith(".tools")


def test_no_gpu_means_loud_failure(pkg, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (so that the box with a GPU runs this too)
    x = np.zeros((1, 4, 4, 1), F)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.demo.generate_multi_channel(x, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.demo.generate_multi_channel_with_image(np.zeros((1, 4, 4, 3), F), x, 7)

"""The backward of generate_multi_channel (net.py:83-122) without a GPU: the literal numpy statement of tests/gmc_grad_ref.py
against torch's float64 autograd through a literal F.unfold statement of the forward, hand cases by value, and the argument
checks of dtfill_generate_multi_channel_backward through ctypes (they come before any HIP call)."""
import numpy as np
import pytest

import gmc_grad_ref as G
import gmc_ref as R

F = np.float32

# (B, H, W, table_size, scale_num, data kind, mask kind)
CASES = (
    (2, 19, 70, 7, 4, "sparse", "gt01"),
    (1, 3, 5, 7, 4, "sparse", "gt01"),
    (1, 1, 1, 7, 3, "dense", "gt01"),
    (2, 17, 66, 5, 4, "mixed", "fraction"),
    (1, 20, 40, 3, 4, "sparse", "binary"),
    (1, 18, 30, 15, 3, "sparse", "negative"),
    (1, 16, 64, 7, 4, "straddle", "gt01"),
    (1, 9, 9, 7, 4, "sparse", "zero"),
)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_numpy_statement_against_float64_autograd(case):
    """loss = sum_k <g_k, lidar_k>; d loss / d data by torch float64 autograd of torch_statement against the float32 numpy
    statement, within chain_bound.  The derived masks of the float32 and the float64 forward must be the same ones."""
    import torch

    B, H, W, ts, sn, dkind, mkind = case
    rng = np.random.default_rng(0)
    data = R.make_data(dkind, rng, (B, H, W))
    mask = R.make_mask(mkind, rng, data)
    gs = [rng.uniform(-1, 1, (B, H, W)).astype(F) for _ in range(sn)] + [None] * (4 - sn)
    outs = G.forward(data, mask, ts, sn) + [None] * (4 - sn)
    x = torch.from_numpy(data.astype(np.float64)).requires_grad_(True)
    touts = G.torch_statement(x, torch.from_numpy(mask.astype(np.float64)), ts, sn)
    for k in range(1, sn):
        assert np.array_equal(touts[k].detach().numpy() > float(G.THR), outs[k] > G.THR), "derived mask of lidar_%d differs" % (k + 1)
    loss = sum((torch.from_numpy(gs[k].astype(np.float64)) * touts[k]).sum() for k in range(sn))
    loss.backward()
    want = x.grad.numpy()
    got = G.backward(mask, outs[1], outs[2], ts, sn, gs)
    assert got.dtype == F
    bound = G.chain_bound(mask, outs[1], outs[2], ts, sn, gs)
    err = np.abs(got.astype(np.float64) - want)
    print("%s: max |grad| %.3g, max err %.3g, max bound %.3g" % (case, np.abs(want).max(), err.max(), bound.max()))
    assert (err <= bound).all(), (case, err.max(), bound.max())


def test_one_source_collects_every_window():
    """One masked pixel in a 5 x 5 frame, table 7: every window holds it and selects it alone, so its gradient is the sum of
    g_p / (1 + 1e-6) in raster order and every other pixel gets +0."""
    rng = np.random.default_rng(1)
    mask = np.zeros((1, 5, 5), F)
    mask[0, 1, 3] = 1
    g2 = rng.uniform(-2, 2, (1, 5, 5)).astype(F)
    mx, cnt = G.step_stats(mask, 7)
    assert (cnt == 1).all() and (mx > 0).all()
    got = G.backward(mask, None, None, 7, 2, (None, g2, None, None))
    acc = F(0)
    for v in g2.reshape(-1):
        acc = F(acc + F(v / (F(1e-6) + F(1))))
    want = np.zeros((1, 5, 5), F)
    want[0, 1, 3] = acc
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_all_zero_mask_selects_every_tap():
    """Every product is 0, padding taps included: each window selects all ts^2 taps, divisor 1e-6f + ts^2 also near the border,
    and a pixel collects g_p / that from every in-image window around it."""
    rng = np.random.default_rng(2)
    for ts, (H, W) in ((7, (6, 9)), (3, (4, 4))):
        half = ts // 2
        g2 = rng.uniform(-2, 2, (1, H, W)).astype(F)
        mx, cnt = G.step_stats(np.zeros((1, H, W), F), ts)
        assert (cnt == ts * ts).all() and (mx == 0).all()
        got = G.backward(np.zeros((1, H, W), F), None, None, ts, 2, (None, g2, None, None))
        c = g2 / (F(1e-6) + F(ts * ts))
        want = np.zeros((1, H, W), F)
        for i in range(H):
            for j in range(W):
                acc = F(0)
                for pi in range(max(0, i - half), min(H, i + half + 1)):
                    for pj in range(max(0, j - half), min(W, j + half + 1)):
                        acc = F(acc + c[0, pi, pj])
                want[0, i, j] = acc
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ts


def test_scale_num_1_and_null_gradients():
    rng = np.random.default_rng(3)
    data = R.make_data("sparse", rng, (1, 8, 9))
    mask = R.make_mask("gt01", rng, data)
    outs = G.forward(data, mask, 7, 4)
    g = [rng.uniform(-1, 1, data.shape).astype(F) for _ in range(4)]
    g[0][0, 0, 0] = F(-0.0)
    got = G.backward(mask, None, None, 7, 1, (g[0], g[1], g[2], g[3]))  # scale_num 1: g1 as it is, the others unused
    assert np.array_equal(got.view(np.uint32), g[0].view(np.uint32))
    for sn in (1, 2, 3, 4):  # every gradient NULL: exact +0
        got = G.backward(mask, outs[1], outs[2], 7, sn, (None,) * 4)
        assert got.dtype == F and not got.view(np.uint32).any(), sn
    # a NULL g_k adds nothing: the chain with g3 alone equals A_1^T A_2^T g3
    got = G.backward(mask, outs[1], outs[2], 7, 4, (None, None, g[2], None))
    want = G.step_transpose(G.step_transpose(g[2], R.next_mask(outs[1]), 7), mask, 7)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- the ABI without a GPU

def test_argument_errors(pkg):
    """Every argument check of dtfill_generate_multi_channel_backward comes before any HIP call."""
    L = pkg.load()
    P = 256  # stands for a valid, aligned device pointer: no call below gets as far as using it
    f = L.dtfill_generate_multi_channel_backward
    ok = dict(mask=P, o2=P, o3=P, B=1, H=8, W=8, ts=7, sn=4, g1=P, g2=P, g3=P, g4=P, gd=P, ws=P, nb=1 << 20, st=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["mask"], a["o2"], a["o3"], a["B"], a["H"], a["W"], a["ts"], a["sn"], a["g1"], a["g2"], a["g3"], a["g4"],
                 a["gd"], a["ws"], a["nb"], a["st"])

    NULL, SHAPE, WORKSPACE = -1, -2, -3
    assert call(mask=None) == NULL and call(gd=None) == NULL
    assert call(o2=None) == NULL and call(o3=None) == NULL  # scale_num 4 derives masks from both
    assert call(sn=3, o2=None) == NULL
    assert call(ws=None) == NULL and call(sn=3, ws=None) == NULL
    for ts in (0, 2, 6, 16, 17, -1, -7):
        assert call(ts=ts) == SHAPE, ts
    for sn in (0, 5, -1):
        assert call(sn=sn) == SHAPE, sn
    for k in ("B", "H", "W"):
        assert call(**{k: 0}) == SHAPE and call(**{k: -4}) == SHAPE, k
    assert call(B=1 << 15, H=1 << 8, W=1 << 8) == SHAPE  # B*H*W = 2^31
    M = 2 ** 31 - 1  # a product that does not fit 64 bits is rejected like any other
    assert call(B=M, H=M, W=M) == SHAPE and call(B=3, H=M, W=1) == SHAPE
    need = L.dtfill_generate_multi_channel_backward_workspace_bytes(1, 8, 8, 4)
    assert call(nb=need - 1) == WORKSPACE and call(nb=0) == WORKSPACE
    assert call(ws=P + 4) == WORKSPACE and call(ws=P + 128) == WORKSPACE
    need3 = L.dtfill_generate_multi_channel_backward_workspace_bytes(1, 8, 8, 3)
    assert call(sn=3, o3=None, nb=need3 - 1) == WORKSPACE


def test_workspace_sizing(pkg):
    L = pkg.load()
    f = L.dtfill_generate_multi_channel_backward_workspace_bytes
    frame = lambda B, H, W: (B * H * W * 4 + 255) // 256 * 256
    for B, H, W in ((1, 1, 1), (1, 8, 8), (3, 17, 65), (32, 256, 1216)):
        assert f(B, H, W, 1) == 0 and f(B, H, W, 2) == 0  # no G_k is kept
        assert 0 < f(B, H, W, 3) <= frame(B, H, W)
        assert 0 < f(B, H, W, 4) <= 2 * frame(B, H, W)
    M = 2 ** 31 - 1
    for bad in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, -1, 4), (1, 8, 8, 0), (1, 8, 8, 5), (1 << 15, 1 << 8, 1 << 8, 4), (M, M, M, 4)):
        assert f(*bad) == 0, bad


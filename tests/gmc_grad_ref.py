"""A literal numpy statement of the backward of generate_multi_channel() (solution_DeepNet/net.py:83-122), for the tests only.

Written from the reference and from the contract in include/dtfill.h, not from the kernel.  tf.equal, tf.cast and tf.greater
have no gradient, so one forward step (gmc_ref.gmc_step: s = mask * w, sel = (s == max s), out = sum(data * sel) / (1e-6 +
sum(sel))) is a fixed sparse linear map of its data, and its backward is the transpose of that map:
  mx_p, cnt_p  the window maximum of mask * w over all ts^2 taps of the zero-padded frame and the number of taps reaching it;
  c_p          G_p / (1e-6f + cnt_p), one float32 division;
  (A^T G)_q    the float32 sum, from +0, in ascending raster order of p, of c_p over the in-image p whose window selected q:
               mask[q] * w(q - p) == mx_p.  Where p did not select q nothing is added (not even c_p * 0).
The chain: G_3 = g3 + A_3^T g4, G_2 = g2 + A_2^T G_3, grad_data = g1 + A_1^T G_2, the mask of step k >= 2 being
(lidar_k > 0.001f); a None gradient adds nothing.
torch_statement() is the same forward as an F.unfold expression in any dtype: float64 autograd through it is the independent
oracle the numpy statement is pinned to (tests/test_gmc_backward.py).  The product does not import this file.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import gmc_ref as R

F32 = np.float32
EPS = F32(0.000001)
THR = F32(0.001)


def step_stats(mask, ts):
    """mx float32 [B,H,W] and cnt int64 [B,H,W] of one forward step: the maximum over all ts^2 taps, padding taps included
    (product 0); a NaN product is never selected."""
    mask = np.asarray(mask, F32)
    B, H, W = mask.shape
    half = (ts - 1) // 2
    pm = np.pad(mask, ((0, 0), (half, half), (half, half)))
    s = sliding_window_view(pm, (ts, ts), axis=(1, 2)).reshape(B, H, W, ts * ts) * R.weights(ts)
    mx = np.fmax.reduce(s, axis=-1, initial=-np.inf).astype(F32)
    return mx, (s == mx[..., None]).sum(axis=-1)


def step_transpose(G, mask, ts, dtype=F32):
    """(A^T G) for the step with this mask.  dtype float32: the contract's arithmetic; float64: the same sums without the
    float32 roundings (the selection stays that of the float32 products), for chain_bound()."""
    mask = np.asarray(mask, F32)
    G = np.asarray(G, dtype)
    B, H, W = mask.shape
    half = (ts - 1) // 2
    mx, cnt = step_stats(mask, ts)
    with np.errstate(all="ignore"):
        c = G / (dtype(EPS) + cnt.astype(dtype))
        pmx = np.pad(mx, ((0, 0), (half, half), (half, half)), constant_values=np.nan)  # a window off the image selects nothing
        pc = np.pad(c, ((0, 0), (half, half), (half, half)))
        acc = np.zeros((B, H, W), dtype)
        for i in range(ts):  # p = q + (i - half, j - half): ascending raster order
            for j in range(ts):
                w = F32(ts - abs(i - half) - abs(j - half))  # q is tap q - p of p's window
                sel = mask * w == pmx[:, i:i + H, j:j + W]
                acc = np.where(sel, acc + pc[:, i:i + H, j:j + W], acc)
    return acc.astype(dtype)


def forward(data, mask, ts, sn):
    """[lidar_1 .. lidar_sn] by gmc_ref.gmc_step."""
    outs = [np.asarray(data, F32)]
    m = np.asarray(mask, F32)
    for _ in range(sn - 1):
        outs.append(R.gmc_step(outs[-1], m, ts)[0])
        m = R.next_mask(outs[-1])
    return outs


def step_masks(mask, out2, out3, sn):
    """The masks of steps 1 .. sn - 1: the caller's, then (lidar_k > 0.001f)."""
    return [np.asarray(mask, F32)] + [R.next_mask(o) for o in (out2, out3)[:max(0, sn - 2)]]


def backward(mask, out2, out3, ts, sn, gs, dtype=F32):
    """grad_data of the whole call.  gs: (g1, g2, g3, g4), None for a zero gradient; out2 / out3: the forward's lidar_2 / 3."""
    masks = step_masks(mask, out2, out3, sn)
    shape = np.asarray(mask).shape
    gs = [None if g is None else np.asarray(g, dtype) for g in gs]
    up = gs[sn - 1]
    with np.errstate(all="ignore"):
        for k in range(sn - 1, 0, -1):
            t = step_transpose(np.zeros(shape, dtype) if up is None else up, masks[k - 1], ts, dtype)
            up = t if gs[k - 1] is None else gs[k - 1] + t
    return np.zeros(shape, dtype) if up is None else up.astype(dtype)


def chain_bound(mask, out2, out3, ts, sn, gs):
    """How far a float32 evaluation of backward() may lie from the exact one: each of at most three steps errs by at most its
    at most ts^2 additions, one division and one add, each within 2^-24 of the absolute sum: 3 (ts^2 + 3) 2^-24 times the same
    chain evaluated in float64 on |g_k|."""
    absg = [None if g is None else np.abs(np.asarray(g, np.float64)) for g in gs]
    return 3 * (ts * ts + 3) * 2.0 ** -24 * backward(mask, out2, out3, ts, sn, absg, np.float64)


def torch_statement(data, mask, ts, sn):
    """The forward as a literal F.unfold expression on torch tensors [B,H,W] of any float dtype.  Returns [lidar_1 .. lidar_sn];
    the constants are the float32 ones in every dtype, so that the derived masks can be compared across dtypes."""
    import torch
    import torch.nn.functional as F

    half = (ts - 1) // 2
    w = torch.from_numpy(R.weights(ts)).to(data.dtype)[None, :, None]
    eps, thr = float(EPS), float(THR)
    outs, d, m = [data], data, mask
    B, H, W = data.shape
    for _ in range(sn - 1):
        pd = F.unfold(d[:, None], ts, padding=half)  # [B, ts^2, H W], kernel positions in row-major order
        s = F.unfold(m[:, None], ts, padding=half) * w
        sel = (s == s.max(dim=1, keepdim=True).values).to(data.dtype)
        d = ((pd * sel).sum(dim=1) / (eps + sel.sum(dim=1))).reshape(B, H, W)
        m = (d > thr).to(data.dtype).detach()
        outs.append(d)
    return outs


def assert_same(got, want, what=""):
    """Bit for bit, a NaN of any payload matching a NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d pixel(s) differ, first at %s: got %r, want %r" % (what, bad.sum(), k, got[k], want[k]))

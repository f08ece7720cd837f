"""dtfill_generate_multi_channel_backward (k_gmcb<7>, k_gmcb<0>, k_gmcb_first) on the device against the literal reference of
tests/gmc_grad_ref.py, and the autograd operator built on it.

The bar is bit for bit (a NaN matching a NaN): include/dtfill.h fixes the order of the additions, so a float32 evaluation has
one result.  Through the raw ABI every buffer is a guarded allocation; grad_data and the workspace are poisoned first, and the
inputs must come back unchanged.  Shapes sit at the seams of the 16 x 64 tiling: 1 x 1, 3 x 5 (smaller than the window), one
tile exactly, 19 x 70 (two tiles each way, ragged, B = 2) and 33 x 129; each at table 7 (the compile-time kernel), 19 x 70 also
at tables 3, 5 and 15 (the runtime one); scale_num 1..4; the mask kinds gt01, binary, fraction, negative, neg_zero and zero; every
g_k NULL in some case; one case off the 256-byte grid; one with a +inf in g4."""
import itertools

import numpy as np
import pytest

import gmc_grad_ref as G
import gmc_ref as R
from guarded import GuardedBuffer, is_poison, poison, poison_value, KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SHAPES = ((1, 1, 1), (1, 3, 5), (1, 16, 64), (2, 19, 70), (1, 33, 129))
MASK_KINDS = ("gt01", "binary", "fraction", "negative", "neg_zero", "zero")
# which of g1..g4 are NULL, cycled through the cases: each is NULL in some case and given in some other, all NULL once
NULLS = ((), (0,), (3,), (1, 2), (0, 2, 3), (0, 1, 2, 3), (1,), (2, 3))
assert all(any(k in n for n in NULLS) and any(k not in n for n in NULLS) for k in range(4))
_SEED = itertools.count(9700)


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def make_case(rng, shape, ts, mkind, nulls, dkind="sparse"):
    """(mask, [lidar_1..4], [g1..g4 or None]) for one case: the forward by the reference, chained from the caller's mask."""
    data = R.make_data(dkind, rng, shape)
    mask = R.make_mask(mkind, rng, data)
    outs = G.forward(data, mask, ts, 4)
    gs = [None if k in nulls else rng.uniform(-2, 2, shape).astype(F) for k in range(4)]
    return mask, outs, gs


def _guarded(a, offset=0):
    import torch

    g = GuardedBuffer(a.nbytes, offset, DEV, frame_bytes=a[0].nbytes)
    g.view(torch.float32, a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return g


def run_device(L, mask, out2, out3, ts, sn, gs, offset=0, null_ws=False, twice=False):
    """One dtfill_generate_multi_channel_backward call (two on the same stream with `twice`, into separate outputs) from
    guarded buffers.  Returns grad_data (a list of two with `twice`) after checking guards, inputs and poison."""
    import torch

    seed = next(_SEED)
    B, H, W = shape = mask.shape
    ins = [mask, out2 if sn >= 3 else None, out3 if sn == 4 else None] + list(gs)
    gin = [None if a is None else _guarded(a, offset) for a in ins]
    outs = [GuardedBuffer(mask.nbytes, offset, DEV, frame_bytes=H * W * 4) for _ in range(2 if twice else 1)]
    for o in outs:
        o.view(torch.int32, shape).fill_(int(poison_value("depth").view(np.int32)))
    need = L.dtfill_generate_multi_channel_backward_workspace_bytes(B, H, W, sn)
    assert (need == 0) == (sn <= 2) and need <= 2 * ((B * H * W * 4 + 255) // 256 * 256)
    ws = GuardedBuffer(need, 0, DEV, frame_bytes=H * W * 4)
    what = "ts %d %s sn %d nulls %s" % (ts, shape, sn, [k for k in range(4) if gs[k] is None])
    for o in outs:
        if need:
            poison(ws.payload(), KINDS[seed % 3], seed)
        rc = L.dtfill_generate_multi_channel_backward(*[None if g is None else g.ptr for g in gin[:3]], B, H, W, ts, sn,
                                                      *[None if g is None else g.ptr for g in gin[3:]], o.ptr,
                                                      None if null_ws else ws.ptr, need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, what + ": " + L.dtfill_strerror(rc).decode()
    torch.cuda.synchronize()
    for k, g in enumerate(gin + [ws] + outs):
        if g is not None:
            g.check("%s buffer %d" % (what, k))
    for a, g in zip(ins, gin):
        if a is not None:
            assert np.array_equal(g.view(torch.float32, shape).cpu().numpy().view(np.uint32), a.view(np.uint32)), what + ": an input changed"
    got = [o.view(torch.float32, shape).cpu().numpy() for o in outs]
    for g in got:
        assert not is_poison(g, "depth").any(), what + ": grad_data keeps poison"
    return got if twice else got[0]


def check_case(L, rng, shape, ts, mkind, nulls, sns=(1, 2, 3, 4), dkind="sparse", offset=0):
    mask, outs, gs = make_case(rng, shape, ts, mkind, nulls, dkind)
    for sn in sns:
        want = G.backward(mask, outs[1], outs[2], ts, sn, gs)
        got = run_device(L, mask, outs[1], outs[2], ts, sn, gs, offset=offset, null_ws=sn <= 2 and shape[0] == 1)
        G.assert_same(got, want, "ts %d %s %s sn %d nulls %s" % (ts, shape, mkind, sn, nulls))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_table_7_at_the_tile_seams(L, shape):
    rng = np.random.default_rng(800 + shape[2])
    for k, mkind in enumerate(MASK_KINDS):
        check_case(L, rng, shape, 7, mkind, NULLS[(k + shape[1]) % len(NULLS)], dkind="mixed" if mkind == "fraction" else "sparse")


@pytest.mark.parametrize("ts", (3, 5, 15))
def test_runtime_table_sizes(L, ts):
    rng = np.random.default_rng(810 + ts)
    for k, mkind in enumerate(MASK_KINDS):
        check_case(L, rng, (2, 19, 70), ts, mkind, NULLS[(k + ts) % len(NULLS)], sns=(4, 2) if k else (1, 2, 3, 4))


def test_every_null_pattern(L):
    """Each of g1..g4 NULL, alone and together, at 19 x 70, table 7, scale_num 4 and 3."""
    rng = np.random.default_rng(820)
    for nulls in NULLS:
        check_case(L, rng, (2, 19, 70), 7, "gt01", nulls, sns=(4, 3))


def test_buffers_off_the_256_byte_grid(L):
    """Inputs and grad_data 4 bytes after a 256-byte boundary (the workspace itself must stay aligned)."""
    rng = np.random.default_rng(830)
    check_case(L, rng, (2, 19, 70), 7, "gt01", (), sns=(4,), offset=4)
    check_case(L, rng, (2, 19, 70), 5, "fraction", (0,), sns=(3,), offset=4)


def test_an_infinite_gradient_stays_where_it_was_selected(L):
    rng = np.random.default_rng(840)
    shape = (1, 33, 129)
    mask, outs, gs = make_case(rng, shape, 7, "gt01", ())
    gs[3][0, 16, 64] = np.inf
    want = G.backward(mask, outs[1], outs[2], 7, 4, gs)
    got = run_device(L, mask, outs[1], outs[2], 7, 4, gs)
    G.assert_same(got, want, "+inf in g4")
    bad = ~np.isfinite(got)
    assert np.array_equal(bad, ~np.isfinite(want))
    ii, jj = np.nonzero(bad[0])
    # three transposed 7 x 7 steps reach at most 9 pixels each way; a sum over unselected windows would spread much further
    assert 0 < bad.sum() < 19 * 19 and np.abs(ii - 16).max() <= 9 and np.abs(jj - 64).max() <= 9
    gs[3][0, 16, 64] = 1.0
    finite = G.backward(mask, outs[1], outs[2], 7, 4, gs)
    assert np.array_equal(got[~bad].view(np.uint32), finite[~bad].view(np.uint32))  # every other pixel as if it were finite


def test_two_calls_give_the_same_bits(L):
    rng = np.random.default_rng(850)
    for ts, mkind in ((7, "gt01"), (5, "fraction")):
        mask, outs, gs = make_case(rng, (2, 19, 70), ts, mkind, ())
        a, b = run_device(L, mask, outs[1], outs[2], ts, 4, gs, twice=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- the autograd operator

@pytest.fixture(scope="module")
def grad_case():
    rng = np.random.default_rng(860)
    return make_case(rng, (2, 19, 70), 7, "gt01", ())


def test_autograd_matches_the_reference(pkg, L, grad_case):
    import torch

    mask, outs, gs = grad_case
    data = torch.from_numpy(outs[0]).to(DEV).requires_grad_(True)
    m = torch.from_numpy(mask).to(DEV).requires_grad_(True)
    lidar = pkg.autograd.generate_multi_channel(data, m, 7, 4)
    assert len(lidar) == 4 and lidar[0] is data
    plain = pkg.generate_multi_channel(outs[0][..., None], mask[..., None], 7)
    for k in range(4):
        assert np.array_equal(lidar[k].detach().cpu().numpy().view(np.uint32), np.asarray(plain[k], F).reshape(mask.shape).view(np.uint32)), k
        if k:  # the masks the backward derives on the device are the reference's
            assert np.array_equal(lidar[k].detach().cpu().numpy() > G.THR, outs[k] > G.THR), k
    loss = sum((torch.from_numpy(gs[k]).to(DEV) * lidar[k]).sum() for k in range(4))
    loss.backward()
    G.assert_same(data.grad.cpu().numpy(), G.backward(mask, outs[1], outs[2], 7, 4, gs), "data.grad")
    assert m.grad is None


def test_autograd_unused_outputs_arrive_as_null(pkg, L, grad_case):
    import torch

    mask, outs, gs = grad_case
    data = torch.from_numpy(outs[0]).to(DEV).requires_grad_(True)
    lidar = pkg.autograd.generate_multi_channel(data, torch.from_numpy(mask).to(DEV), 7, 4)
    (torch.from_numpy(gs[2]).to(DEV) * lidar[2]).sum().backward()
    G.assert_same(data.grad.cpu().numpy(), G.backward(mask, outs[1], outs[2], 7, 4, (None, None, gs[2], None)), "lidar_3 alone")
    # scale_num 2 and 1: shorter chains, None beyond scale_num
    data.grad = None
    lidar = pkg.autograd.generate_multi_channel(data, torch.from_numpy(mask).to(DEV), 7, 2)
    assert lidar[2] is None and lidar[3] is None
    (torch.from_numpy(gs[1]).to(DEV) * lidar[1]).sum().backward()
    G.assert_same(data.grad.cpu().numpy(), G.backward(mask, None, None, 7, 2, (None, gs[1], None, None)), "scale_num 2")
    lidar = pkg.autograd.generate_multi_channel(data, torch.from_numpy(mask).to(DEV), 7, 1)
    assert lidar[0] is data and lidar[1:] == (None, None, None)


def test_autograd_detached_call_cuts_the_gradient(pkg, L, grad_case):
    """joint_train off (net.py:491-496) is the caller's .detach()."""
    import torch

    mask, outs, gs = grad_case
    data = torch.from_numpy(outs[0]).to(DEV).requires_grad_(True)
    lidar = pkg.autograd.generate_multi_channel(data.detach(), torch.from_numpy(mask).to(DEV), 7, 4)
    assert not any(t.requires_grad for t in lidar)
    w = torch.ones((), device=DEV, requires_grad=True)  # something else in the loss that does need a gradient
    (w * lidar[3]).sum().backward()
    assert data.grad is None and w.grad is not None


def test_backward_device_wrapper_checks(pkg, L, grad_case):
    import torch

    mask, outs, gs = grad_case
    m, o2, o3 = (torch.from_numpy(a).to(DEV) for a in (mask, outs[1], outs[2]))
    g = [torch.from_numpy(a).to(DEV) for a in gs]
    f = pkg.device.generate_multi_channel_backward_device
    G.assert_same(f(m, o2, o3, g).cpu().numpy(), G.backward(mask, outs[1], outs[2], 7, 4, gs), "wrapper")
    G.assert_same(f(m, None, None, (g[0], g[1], None, None), scale_num=2).cpu().numpy(),
                  G.backward(mask, None, None, 7, 2, (gs[0], gs[1], None, None)), "wrapper scale_num 2")
    with pytest.raises(ValueError):
        f(m, None, o3, g)  # out2 is needed for scale_num 4
    with pytest.raises(ValueError):
        f(m, o2, o3, g[:3])
    with pytest.raises(ValueError):
        f(m, o2, o3, [g[0][:, :-1].contiguous()] + g[1:])
    with pytest.raises(ValueError):
        f(m, o2, o3, g, scale_num=5)
    with pytest.raises(pkg.DtfillError):
        f(m, o2, o3, g, table_size=8)

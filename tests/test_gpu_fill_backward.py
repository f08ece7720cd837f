"""dtfill_fill_backward (k_fb_count, k_fb_scan, k_fb_acc<0|1>, k_fb_out) on the device against the literal reference of
tests/fill_grad_ref.py, bit for bit (a NaN matching a NaN), and the autograd operator built on it.

Through the raw ABI every buffer is a guarded allocation; grad_x, the status and the workspace are poisoned first and the inputs
must come back unchanged.  Every case runs with its payloads on a 256-byte boundary and again 4 bytes past one, twice each: the
accumulators are integers, so all four runs must agree bit for bit.  The shapes are the smallest at which each mechanism can go
wrong (a strip is 64 columns x 32 rows, a block four strips):
  1x1x1; 2x5x37 (odd, a partial strip); 1x3x200 with one source (runs that cross lanes, waves and strips); 1x96x130 with one
  source (one accumulator for 12 480 pixels, from 9 strips); 1x40x70 with every pixel a source (n = H*W accumulators, nothing to
  combine, a flush on every row); 2x64x96, a projected LiDAR frame beside an index-error frame; the hand cases as one batch.
The gradients (fill_grad_ref.random_gradient) span 40 binades and hold planted non-finite values (not in the frames that are one
cell) and cancelling pairs."""
import numpy as np
import pytest

import fill_grad_ref as R
from guarded import GuardedBuffer, is_poison, poison, poison_value, KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
CASES = ("1x1x1", "2x5x37", "1x3x200-one-source", "1x96x130-one-source", "1x40x70-all-sources", "2x64x96-lidar-and-error", "hand")
_cache = {}


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def lidar_frame(pkg):
    """One projected LiDAR frame of lidar_cases' generator at 64 x 96."""
    import lidar_cases as LC

    synth = __import__("importlib").import_module(pkg.__name__ + ".synth")
    return synth.velodyne_scan(1, seed=LC.SEEDS[0], hw=(64, 96))[0]


def case(name, pkg, oracle):
    """Inputs and the reference's outputs of one case, computed once and shared (nobody writes to them).  The labels are the
    oracle's (the reference's cv2 transform), except in the hand cases, which carry their own."""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    index = None
    if name == "hand":
        hc = R.hand_cases()
        x, index, grad = (np.stack([c[k] for c in hc.values()]) for k in range(3))
    elif name == "1x1x1":
        x = np.full((1, 1, 1), 5, F)
    elif name == "2x5x37":
        x = np.where(rng.random((2, 5, 37)) < 0.3, np.round(rng.uniform(1, 80, (2, 5, 37)) * 256) / 256, 0).astype(F)
        x[0, 2, 5], x[1, 4, 36] = 0.5, 0.25  # valued, not sources
    elif name.endswith("one-source"):
        x = np.zeros(tuple(int(v) for v in name.split("-")[0].split("x")), F)
        x[0, x.shape[1] // 2, (2 * x.shape[2]) // 3] = 7.5
    elif name == "1x40x70-all-sources":
        x = (np.round(rng.uniform(1, 80, (1, 40, 70)) * 256) / 256).astype(F)
    else:
        x = np.concatenate([lidar_frame(pkg), np.zeros((1, 64, 96), F)])
    if index is None:
        index = oracle.fill_batch(x)[2]
        # (a frame that is one cell keeps its sum finite: a NaN would be all there is to see)
        grad = R.random_gradient(rng, x.shape, nonfinite=not name.endswith("one-source"))
    grad_x, status = R.backward(x, index, grad)
    if name == "hand":  # the reference agrees with what was written down by hand
        for b, c in enumerate(hc.values()):
            assert status[b] == c[4] and np.array_equal(np.nan_to_num(grad_x[b], nan=7), np.nan_to_num(c[3], nan=7))
    elif name.startswith("2x64x96"):
        assert status.tolist() == [0, 1] and (x[0] > 0.1).sum() > 200
    else:
        assert not status.any()
    c = dict(name=name, shape=x.shape, x=x, index=np.ascontiguousarray(index, np.int32), grad=grad, grad_x=grad_x, status=status)
    for a in (c["x"], c["index"], c["grad"], grad_x, status):
        a.setflags(write=False)
    _cache[name] = c
    return c


def bits_match(got, want):
    """Bit for bit, a NaN matching a NaN."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def run_abi(L, x, index, grad, offset, calls=2, val_thr=0.1, what=""):
    """`calls` dtfill_fill_backward calls on guarded copies of the inputs at `offset`, each into freshly poisoned outputs and a
    differently poisoned workspace.  Checks the guards, that the inputs are unchanged and that no poison is left; returns
    [(grad_x, status)] as numpy."""
    import torch

    B, H, W = x.shape
    fb = H * W * 4
    ins = []
    for a, dt in ((x, torch.float32), (index, torch.int32), (grad, torch.float32)):
        g = GuardedBuffer(a.nbytes, offset, DEV, frame_bytes=fb)
        g.view(dt, a.shape).copy_(torch.from_numpy(np.array(a)))  # (a copy: the shared case is read-only)
        ins.append((g, dt, a))
    need = L.dtfill_fill_backward_workspace_bytes(B, H, W)
    assert need >= 16 * B * H * W
    ws = GuardedBuffer(need, 0, DEV, frame_bytes=fb)
    out = GuardedBuffer(B * H * W * 4, offset, DEV, frame_bytes=fb)
    status = GuardedBuffer(B * 4, offset, DEV)
    res = []
    for k in range(calls):
        out.view(torch.int32, x.shape).fill_(int(poison_value("depth").view(np.int32)))
        status.view(torch.int32, (B,)).fill_(int(poison_value("status")))
        poison(ws.payload(), KINDS[(k + offset // 4) % 3], 31 + k)
        rc = L.dtfill_fill_backward(ins[0][0].ptr, ins[1][0].ptr, ins[2][0].ptr, B, H, W, val_thr, out.ptr, status.ptr, ws.ptr, need,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, what + ": " + L.dtfill_strerror(rc).decode()
        torch.cuda.synchronize()
        gx = out.view(torch.float32, x.shape).cpu().numpy()
        assert not is_poison(gx, "depth").any(), what + ": grad_x keeps poison"
        res.append((gx, status.view(torch.int32, (B,)).cpu().numpy()))
    for g, dt, a in ins:
        g.check(what + " input")
        assert same_bits(g.view(dt, a.shape).cpu().numpy(), a), what + ": an input changed"
    for g, nm in ((ws, "workspace"), (out, "grad_x"), (status, "status")):
        g.check(what + " " + nm)
    return res


@pytest.mark.parametrize("name", CASES)
def test_abi_against_the_reference(L, pkg, oracle, name):
    c = case(name, pkg, oracle)
    runs = []
    for offset in (0, 4):
        what = "%s offset %d" % (name, offset)
        res = run_abi(L, c["x"], c["index"], c["grad"], offset, what=what)
        for gx, st in res:
            bad = ~((gx.view(np.uint32) == c["grad_x"].view(np.uint32)) | (np.isnan(gx) & np.isnan(c["grad_x"])))
            assert np.array_equal(st, c["status"]), what
            assert bits_match(gx, c["grad_x"]), "%s: %d of %d differ, first at %s: got %r want %r" % (
                what, bad.sum(), gx.size, tuple(np.argwhere(bad)[0]), gx[bad][0], c["grad_x"][bad][0])
            assert (gx.view(np.uint32)[np.isnan(gx)] == R.QNAN).all(), what + ": not the quiet NaN of the contract"
        assert same_bits(res[0][0], res[1][0]), what + ": two runs differ"
        runs.append(res[0][0])
    assert same_bits(runs[0], runs[1]), name + ": alignment changes the bits"


def test_frame_status_is_nullable(L, pkg, oracle):
    import torch

    c = case("2x64x96-lidar-and-error", pkg, oracle)
    B, H, W = c["shape"]
    x, index, grad = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("x", "index", "grad"))
    out = torch.empty_like(x)
    need = L.dtfill_fill_backward_workspace_bytes(B, H, W)
    ws = GuardedBuffer(need, 0, DEV)
    rc = L.dtfill_fill_backward(x.data_ptr(), index.data_ptr(), grad.data_ptr(), B, H, W, 0.1, out.data_ptr(), None, ws.ptr, need,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    ws.check("workspace")
    assert bits_match(out.cpu().numpy(), c["grad_x"])


@pytest.mark.parametrize("metric", ("l1_cv", "l2"))
def test_forward_into_backward(L, pkg, oracle, metric):
    """DtFill.run's index goes into the backward as it comes out, in both metrics."""
    import torch

    c = case("2x64x96-lidar-and-error", pkg, oracle)
    x = torch.from_numpy(np.array(c["x"])).to(DEV)
    op = pkg.device.DtFill(device=DEV, metric=metric)
    res = op.run(x)
    index = res["index"].clone()
    fwd_status = res["status"].cpu().numpy()
    want_index = oracle.fill_batch(c["x"], metric=metric)[2]
    assert np.array_equal(index.cpu().numpy(), want_index)
    grad = torch.from_numpy(np.array(c["grad"])).to(DEV)
    gx, st = pkg.device.fill_backward_device(x, index, grad)
    want, wst = R.backward(c["x"], want_index, c["grad"])
    assert np.array_equal(st.cpu().numpy(), wst) and np.array_equal(fwd_status & 1, wst)  # the call derives the forward's bit itself
    assert bits_match(gx.cpu().numpy(), want)
    if metric == "l2":  # the two metrics label differently somewhere, and the gradient follows the labels
        assert (want_index != c["index"]).any()
    with pytest.raises(ValueError):
        pkg.device.fill_backward_device(x, index.float(), grad)
    with pytest.raises(ValueError):
        pkg.device.fill_backward_device(x, index[:, :-1].contiguous(), grad)
    with pytest.raises(ValueError):
        pkg.device.fill_backward_device(x.double(), index, grad)


def test_autograd(L, pkg, oracle, monkeypatch):
    """autograd.fill under loss.backward() gives the ABI's bits; dt, index and status carry no gradient; tensors of the call's
    own; an unused depth launches nothing."""
    import torch

    c = case("2x64x96-lidar-and-error", pkg, oracle)
    x = torch.from_numpy(np.array(c["x"])).to(DEV).requires_grad_(True)
    w = torch.from_numpy(np.array(c["grad"])).to(DEV)
    depth, dt, index, status = pkg.autograd.fill(x)
    assert depth.requires_grad and not dt.requires_grad and not index.requires_grad and not status.requires_grad
    want_depth, want_dt, want_index, want_status = oracle.fill_batch(c["x"])
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(dt.cpu().numpy(), want_dt)
    assert np.array_equal(depth.detach().cpu().numpy()[0], want_depth[0]) and np.array_equal(status.cpu().numpy() & 1, want_status)
    # a second call on another input does not overwrite the first call's tensors
    other = pkg.autograd.fill(torch.full_like(x, 3.0))
    assert np.array_equal(index.cpu().numpy(), want_index) and (other[2].cpu().numpy() != want_index).any()
    # d(sum(depth * w)) / d depth = w, bit for bit
    (depth * w).sum().backward()
    abi = run_abi(L, c["x"], c["index"], c["grad"], 0, calls=1, what="autograd")[0][0]
    assert same_bits(x.grad.cpu().numpy(), abi) and bits_match(abi, c["grad_x"])
    with pytest.raises(RuntimeError):  # once differentiable
        x2 = x.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((pkg.autograd.fill(x2)[0] * w).sum(), x2, create_graph=True)
        g.sum().backward()

    # an unused depth: nothing is launched
    calls = []
    real = pkg.device.fill_backward_device
    monkeypatch.setattr(pkg.device, "fill_backward_device", lambda *a, **k: calls.append(1) or real(*a, **k))

    class Drop(torch.autograd.Function):  # hands a None gradient upstream
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            return None

    x3 = x.detach().clone().requires_grad_(True)
    d3 = pkg.autograd.fill(x3)[0]
    (Drop.apply(d3).sum() + (2 * x3).sum()).backward()
    assert not calls and (x3.grad == 2).all()
    x4 = x.detach().clone().requires_grad_(True)
    pkg.autograd.fill(x4)
    (2 * x4).sum().backward()
    assert not calls
    (pkg.autograd.fill(x4)[0] * w).sum().backward()
    assert calls == [1]
    with pytest.raises(ValueError):
        pkg.autograd.fill(x.detach()[0])
    with pytest.raises(ValueError):
        pkg.autograd.fill(x.detach(), metric="l3")


def test_no_host_synchronisation(L, pkg, oracle):
    """Forward and backward under torch's synchronisation debug mode: any blocking call raises."""
    import torch

    c = case("2x64x96-lidar-and-error", pkg, oracle)
    w = torch.from_numpy(np.array(c["grad"])).to(DEV)

    def step():
        x = torch.from_numpy(np.array(c["x"])).to(DEV).requires_grad_(True)
        torch.cuda.synchronize()
        return x

    x = step()
    (pkg.autograd.fill(x)[0] * w).sum().backward()  # the allocator's pools, the operator and the workspace exist
    warm = x.grad.cpu().numpy()
    x = step()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (pkg.autograd.fill(x)[0] * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert same_bits(x.grad.cpu().numpy(), warm) and bits_match(warm, c["grad_x"])

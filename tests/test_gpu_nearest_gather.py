"""dtfill_nearest_gather (k_ng_count, k_ng_scan, k_ng_list, k_ng_gather) and dtfill_nearest_gather_backward (k_ng_count,
k_ng_scan, k_ngb_acc<0|1>, k_ngb_out) on the device against the literal reference of tests/near_ref.py, bit for bit (a NaN payload
matching exactly), and the Python layers built on them.

Through the raw ABI every buffer is a guarded allocation; the outputs, the status and the workspace are poisoned first and the
inputs must come back unchanged.  Every case runs with its payloads on a 256-byte boundary (the 16-byte path where W % 4 == 0)
and again 4 bytes past one (the scalar path), twice each; the backward's accumulators are integers, so its four runs must agree
bit for bit.  The shapes are the smallest at which each mechanism can go wrong (a bit word is 64 columns, a block four rows, a
backward strip 64 columns x 32 rows, a channel round two channels):
  1x1x1 with a source and empty; 2x5x37, C=3 (odd, under one word, two frames with different m, a planted 0.5); 1x3x200 with one
  source, C=2 (runs that cross words and waves); 1x40x70 with every pixel a source (pixel[p] == p, filled has values' bits);
  1x96x130 with one source, C=5 (three channel rounds, nine strips into one accumulator per channel); 2x64x96, a projected LiDAR
  frame beside an all-zero frame, at C=3 and at C=0 (the pixel map alone); the hand cases as one batch.
The values are seeded floats with planted 0x7FC12345, -0.0, +-inf and subnormals; the gradients (fill_grad_ref.random_gradient)
span 40 binades and hold planted non-finite values (not in the frames that are one cell) and cancelling pairs."""
import numpy as np
import pytest

import fill_grad_ref as G
import near_ref as R
from guarded import GuardedBuffer, is_poison, poison, poison_value, KINDS
from helpers import load_l2_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
NAN_PAYLOAD = 0x7FC12345
CASES = ("1x1x1-source", "1x1x1-empty", "2x5x37", "1x3x200-one-source", "1x40x70-all-sources", "1x96x130-one-source",
         "2x64x96-lidar-and-empty", "2x64x96-pixel-map-only", "hand")
CHANNELS = {"1x1x1-source": 1, "1x1x1-empty": 1, "2x5x37": 3, "1x3x200-one-source": 2, "1x40x70-all-sources": 1,
            "1x96x130-one-source": 5, "2x64x96-lidar-and-empty": 3, "2x64x96-pixel-map-only": 0, "hand": 1}
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


def payload(rng, shape):
    """Seeded float32 values with the bit patterns a copy must carry through."""
    v = rng.uniform(-100, 100, shape).astype(F)
    flat = v.reshape(-1)
    plant = np.array([NAN_PAYLOAD, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32).view(F)
    if flat.size >= 16:
        flat[rng.permutation(flat.size)[:plant.size]] = plant
    return v


def case(name, pkg, oracle):
    """Inputs and the reference's outputs of one case, computed once and shared (nobody writes to them).  The labels are the
    oracle's (the reference's cv2 transform), except in the hand cases, which carry their own."""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    C = CHANNELS[name]
    index = None
    if name == "hand":  # the 4 x 6 frames as one batch (the 5 x 7 frame runs in test_survey_frame)
        hc = {k: v for k, v in R.hand_cases().items() if v[0].shape == (4, 6)}
        x, index = (np.stack([c[k] for c in hc.values()]) for k in range(2))
        values = np.stack([c[2] for c in hc.values()])[:, None]
        grad = np.stack([R.hand_grad((4, 6))] * len(hc))[:, None]
    elif name.startswith("1x1x1"):
        x = np.full((1, 1, 1), 5 if name.endswith("source") else 0, F)
    elif name == "2x5x37":
        x = np.where(rng.random((2, 5, 37)) < 0.3, np.round(rng.uniform(1, 80, (2, 5, 37)) * 256) / 256, 0).astype(F)
        x[1, :3] = 0  # the frames' m differ
        x[0, 2, 5], x[1, 4, 36] = 0.5, 0.25  # valued, not sources
    elif name.endswith("one-source"):
        x = np.zeros(tuple(int(v) for v in name.split("-")[0].split("x")), F)
        x[0, x.shape[1] // 2, (2 * x.shape[2]) // 3] = 7.5
    elif name == "1x40x70-all-sources":
        x = (np.round(rng.uniform(1, 80, (1, 40, 70)) * 256) / 256).astype(F)
    else:
        x = np.concatenate([lidar_frame(pkg), np.zeros((1, 64, 96), F)])
    B, H, W = x.shape
    if index is None:
        index = oracle.fill_batch(x)[2]
        values = payload(rng, (B, C, H, W)) if C else None
        # (a frame that is one cell keeps its sum finite: a NaN would be all there is to see)
        grad = G.random_gradient(rng, (B, C, H, W), nonfinite=not name.endswith("one-source")) if C else None
    index = np.ascontiguousarray(index, np.int32)
    filled, pixel, status = R.gather(x, index, values)
    grad_values = R.backward(x, index, grad)[0] if C else None
    if name == "hand":  # the reference agrees with what was written down by hand
        for b, c in enumerate(hc.values()):
            assert status[b] == c[5] and np.array_equal(pixel[b], c[3])
            assert G.same_bits(filled[b, 0], c[4]) and G.same_bits(grad_values[b, 0], c[6])
    elif name.startswith("2x64x96"):
        assert status.tolist() == [0, R.NO_SOURCE] and (x[0] >= 0.9).sum() > 200
    elif name == "1x1x1-empty":
        assert status.tolist() == [R.NO_SOURCE] and pixel[0, 0, 0] == -1
    else:
        assert not status.any()
    if name == "1x40x70-all-sources":
        assert np.array_equal(pixel.reshape(-1), np.arange(H * W)) and G.same_bits(filled, values)
    if name == "2x5x37":
        assert len(set(R.source_pixels(x[b]).size for b in range(2))) == 2
    c = dict(name=name, shape=x.shape, C=C, x=x, index=index, values=values, grad=grad, filled=filled, pixel=pixel, status=status,
             grad_values=grad_values)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _cache[name] = c
    return c


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def bits_match(got, want):
    """Bit for bit, a NaN matching a NaN (the cell sum's NaN is the one quiet NaN; checked apart)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _guarded_inputs(arrays, offset, fb):
    import torch

    ins = []
    for a in arrays:
        dt = torch.int32 if a.dtype == np.int32 else torch.float32
        g = GuardedBuffer(a.nbytes, offset, DEV, frame_bytes=fb)
        g.view(torch.int32, a.shape).copy_(torch.from_numpy(np.array(a).view(np.int32)))  # (bits: a NaN payload stays what it is)
        ins.append((g, dt, a))
    return ins


def _check_inputs(ins, what):
    import torch

    for g, dt, a in ins:
        g.check(what + " input")
        assert same_bits(g.view(torch.int32, a.shape).cpu().numpy(), a), what + ": an input changed"


def run_forward(L, c, offset, calls=2, what="", status=True, want_pixel=True, want_values=True):
    """`calls` dtfill_nearest_gather calls on guarded copies of the inputs at `offset`, each into freshly poisoned outputs and a
    differently poisoned workspace.  Checks the guards, that the inputs are unchanged and that no poison is left; returns
    [(filled or None, pixel or None, status or None)] as numpy."""
    import torch

    B, H, W = c["shape"]
    C = c["C"] if want_values else 0
    fb = H * W * 4
    ins = _guarded_inputs([c["x"], c["index"]] + ([c["values"]] if C else []), offset, fb)
    need = L.dtfill_nearest_gather_workspace_bytes(B, H, W)
    assert need >= 4 * B * H * W
    ws = GuardedBuffer(need, 0, DEV, frame_bytes=fb)
    out = GuardedBuffer(B * C * H * W * 4, offset, DEV, frame_bytes=fb) if C else None
    pix = GuardedBuffer(B * H * W * 4, offset, DEV, frame_bytes=fb) if want_pixel else None
    st = GuardedBuffer(B * 4, offset, DEV) if status else None
    res = []
    for k in range(calls):
        if out:
            out.view(torch.int32, (B, C, H, W)).fill_(int(poison_value("depth").view(np.int32)))
        if pix:
            pix.view(torch.int32, (B, H, W)).fill_(int(poison_value("index")))
        if st:
            st.view(torch.int32, (B,)).fill_(int(poison_value("status")))
        poison(ws.payload(), KINDS[(k + offset // 4) % 3], 31 + k)
        rc = L.dtfill_nearest_gather(ins[0][0].ptr, ins[1][0].ptr, ins[2][0].ptr if C else None, C, B, H, W, 0.1,
                                     out.ptr if out else None, pix.ptr if pix else None, st.ptr if st else None, ws.ptr, need,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, what + ": " + L.dtfill_strerror(rc).decode()
        torch.cuda.synchronize()
        f = out.view(torch.int32, (B, C, H, W)).cpu().numpy().view(F) if out else None
        p = pix.view(torch.int32, (B, H, W)).cpu().numpy() if pix else None
        assert f is None or not is_poison(f, "depth").any(), what + ": out_values keeps poison"
        assert p is None or not is_poison(p, "index").any(), what + ": out_pixel keeps poison"
        res.append((f, p, st.view(torch.int32, (B,)).cpu().numpy() if st else None))
    _check_inputs(ins, what)
    for g, nm in ((ws, "workspace"), (out, "out_values"), (pix, "out_pixel"), (st, "status")):
        if g:
            g.check(what + " " + nm)
    return res


def run_backward(L, c, offset, calls=2, what="", status=True):
    """The same for dtfill_nearest_gather_backward; returns [(grad_values, status or None)]."""
    import torch

    B, H, W = c["shape"]
    C = c["C"]
    fb = H * W * 4
    ins = _guarded_inputs([c["x"], c["index"], c["grad"]], offset, fb)
    need = L.dtfill_nearest_gather_backward_workspace_bytes(B, H, W, C)
    assert need >= 16 * B * H * W
    ws = GuardedBuffer(need, 0, DEV, frame_bytes=fb)
    out = GuardedBuffer(B * C * H * W * 4, offset, DEV, frame_bytes=fb)
    st = GuardedBuffer(B * 4, offset, DEV) if status else None
    res = []
    for k in range(calls):
        out.view(torch.int32, (B, C, H, W)).fill_(int(poison_value("depth").view(np.int32)))
        if st:
            st.view(torch.int32, (B,)).fill_(int(poison_value("status")))
        poison(ws.payload(), KINDS[(k + offset // 4) % 3], 31 + k)
        rc = L.dtfill_nearest_gather_backward(ins[0][0].ptr, ins[1][0].ptr, ins[2][0].ptr, C, B, H, W, 0.1, out.ptr,
                                              st.ptr if st else None, ws.ptr, need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, what + ": " + L.dtfill_strerror(rc).decode()
        torch.cuda.synchronize()
        g = out.view(torch.float32, (B, C, H, W)).cpu().numpy()
        assert not is_poison(g, "depth").any(), what + ": grad_values keeps poison"
        res.append((g, st.view(torch.int32, (B,)).cpu().numpy() if st else None))
    _check_inputs(ins, what)
    for g, nm in ((ws, "workspace"), (out, "grad_values"), (st, "status")):
        if g:
            g.check(what + " " + nm)
    return res


@pytest.mark.parametrize("name", CASES)
def test_forward_against_the_reference(L, pkg, oracle, name):
    c = case(name, pkg, oracle)
    for offset in (0, 4):
        what = "%s offset %d" % (name, offset)
        for f, p, st in run_forward(L, c, offset, what=what):
            assert np.array_equal(st, c["status"]), (what, st)
            bad = p != c["pixel"]
            assert not bad.any(), "%s: %d pixels differ, first at %s: got %d want %d" % (
                what, bad.sum(), tuple(np.argwhere(bad)[0]), p[bad][0], c["pixel"][bad][0])
            if c["C"]:
                bad = f.view(np.uint32) != c["filled"].view(np.uint32)
                assert not bad.any(), "%s: %d values differ, first at %s: got %r want %r" % (
                    what, bad.sum(), tuple(np.argwhere(bad)[0]), f[bad][0], c["filled"][bad][0])
            else:
                assert f is None
    if c["C"] and c["values"].size >= 16 and name != "hand":
        assert (c["values"].view(np.uint32) == NAN_PAYLOAD).any()  # (and it arrives: 1x40x70-all-sources' filled is values)


@pytest.mark.parametrize("name", [n for n in CASES if CHANNELS[n]])
def test_backward_against_the_reference(L, pkg, oracle, name):
    c = case(name, pkg, oracle)
    runs = []
    for offset in (0, 4):
        what = "%s offset %d" % (name, offset)
        res = run_backward(L, c, offset, what=what)
        for g, st in res:
            bad = ~((g.view(np.uint32) == c["grad_values"].view(np.uint32)) | (np.isnan(g) & np.isnan(c["grad_values"])))
            assert np.array_equal(st, c["status"]), (what, st)
            assert bits_match(g, c["grad_values"]), "%s: %d of %d differ, first at %s: got %r want %r" % (
                what, bad.sum(), g.size, tuple(np.argwhere(bad)[0]), g[bad][0], c["grad_values"][bad][0])
            assert (g.view(np.uint32)[np.isnan(g)] == G.QNAN).all(), what + ": not the quiet NaN of the contract"
        assert same_bits(res[0][0], res[1][0]), what + ": two runs differ"
        runs.append(res[0][0])
    assert same_bits(runs[0], runs[1]), name + ": alignment changes the bits"


def test_survey_frame(L):
    """SURVEY section 8c's 5 x 7 frame, by hand: label 1 -> pixel 5, 2 -> 15, 3 -> 32."""
    x, index, vals, pixel, filled, status, grad_values = R.hand_cases()["survey 8c"]
    c = dict(shape=(1, 5, 7), C=1, x=x[None], index=index[None], values=vals[None, None], grad=R.hand_grad((1, 1, 5, 7)))
    f, p, st = run_forward(L, c, 0, calls=1, what="survey 8c")[0]
    assert st.tolist() == [status] and np.array_equal(p[0], pixel) and same_bits(f[0, 0], filled)
    g, st = run_backward(L, c, 0, calls=1, what="survey 8c")[0]
    assert st.tolist() == [status] and same_bits(g[0, 0], grad_values)


@pytest.mark.parametrize("drop", ("frame_status", "out_pixel", "out_values"))
def test_nullable_arguments(L, pkg, oracle, drop):
    c = case("2x64x96-lidar-and-empty", pkg, oracle)
    kw = dict(status=drop != "frame_status", want_pixel=drop != "out_pixel", want_values=drop != "out_values")
    for offset in (0, 4):
        f, p, st = run_forward(L, c, offset, calls=1, what="no " + drop, **kw)[0]
        assert (st is None) == (drop == "frame_status") and (p is None) == (drop == "out_pixel") and (f is None) == (drop == "out_values")
        assert st is None or np.array_equal(st, c["status"])
        assert p is None or np.array_equal(p, c["pixel"])
        assert f is None or same_bits(f, c["filled"])
    if drop == "frame_status":
        g, st = run_backward(L, c, 0, calls=1, what="backward, no frame_status", status=False)[0]
        assert st is None and bits_match(g, c["grad_values"])


@pytest.mark.parametrize("metric", ("l1_cv", "l2"))
def test_forward_into_gather(L, pkg, oracle, metric):
    """DtFill.run's index goes into the gather as it comes out, in both metrics: l2 gives the scipy-pinned `near` of every case of
    l2_cases.npz, l1_cv the reference on the oracle's labels."""
    import torch

    op = pkg.device.DtFill(device=DEV, metric=metric)
    if metric == "l2":
        cases, _ = load_l2_cases()
        for name, lc in cases.items():
            x = torch.from_numpy(np.ascontiguousarray(lc["x"], F)[None]).to(DEV)
            filled, pixel, status = pkg.device.nearest_gather_device(x, op.run(x, want=("index",))["index"])
            assert filled is None and np.array_equal(pixel.cpu().numpy()[0], lc["near"].reshape(lc["x"].shape)), name
            assert status.cpu().numpy()[0] == (R.NO_SOURCE if (lc["near"] < 0).all() else 0), name
        return
    c = case("2x64x96-lidar-and-empty", pkg, oracle)
    x = torch.from_numpy(np.array(c["x"])).to(DEV)
    values = torch.from_numpy(np.array(c["values"]).view(np.int32)).to(DEV).view(torch.float32)
    index = op.run(x, want=("index",))["index"]
    assert np.array_equal(index.cpu().numpy(), c["index"])
    filled, pixel, status = pkg.device.nearest_gather_device(x, index, values)
    assert np.array_equal(status.cpu().numpy(), c["status"]) and np.array_equal(pixel.cpu().numpy(), c["pixel"])
    assert same_bits(filled.view(torch.int32).cpu().numpy(), c["filled"])
    only, none, _ = pkg.device.nearest_gather_device(x, index, values, want_pixel=False)
    assert none is None and same_bits(only.view(torch.int32).cpu().numpy(), c["filled"])
    grad = torch.from_numpy(np.array(c["grad"])).to(DEV)
    gv, st = pkg.device.nearest_gather_backward_device(x, index, grad)
    assert np.array_equal(st.cpu().numpy(), c["status"]) and bits_match(gv.cpu().numpy(), c["grad_values"])
    for bad in (lambda: pkg.device.nearest_gather_device(x, index.float(), values),
                lambda: pkg.device.nearest_gather_device(x, index[:, :-1].contiguous(), values),
                lambda: pkg.device.nearest_gather_device(x.double(), index, values),
                lambda: pkg.device.nearest_gather_device(x, index, values[:, :, :-1].contiguous()),
                lambda: pkg.device.nearest_gather_device(x, index, values.transpose(2, 3)),
                lambda: pkg.device.nearest_gather_device(x, index, None, want_pixel=False),
                lambda: pkg.device.nearest_gather_backward_device(x, index, grad[:, 0]),
                lambda: pkg.device.nearest_gather_backward_device(x, index.long(), grad)):
        with pytest.raises(ValueError):
            bad()


def test_nearest_source_numpy(pkg, oracle):
    """tools.nearest_source: numpy in, numpy out, frames squeezed like nearest_point."""
    c = case("2x64x96-lidar-and-empty", pkg, oracle)
    dt, pixel, filled = pkg.nearest_source(np.array(c["x"]), np.array(c["values"]))
    assert np.array_equal(pixel, c["pixel"]) and same_bits(filled, c["filled"]) and np.array_equal(dt, oracle.fill_batch(c["x"])[1])
    dt1, pixel1 = pkg.nearest_source(np.array(c["x"][0])[..., None])
    assert dt1.shape == (64, 96) and np.array_equal(pixel1, c["pixel"][0]) and np.array_equal(dt1, dt[0])
    _, pixel1, filled1 = pkg.nearest_source(np.array(c["x"][0]), np.array(c["values"][0, 1]))
    assert filled1.shape == (64, 96) and same_bits(filled1, c["filled"][0, 1]) and np.array_equal(pixel1, c["pixel"][0])
    with pytest.raises(ValueError):
        pkg.nearest_source(c["x"], c["values"][:, :, :-1])
    with pytest.raises(TypeError):
        pkg.nearest_source(c["x"], c["values"].astype(np.float64))


def test_autograd(L, pkg, oracle, monkeypatch):
    """autograd.fill_values: the outputs against the reference; a gradient only through filled and only to values; the ABI's
    bits under backward(); the C = 1 squeeze; once differentiable; an unused filled launches nothing; tensors of the call's own;
    the net.py:131-155 recipe end to end."""
    import torch

    c = case("2x64x96-lidar-and-empty", pkg, oracle)
    x = torch.from_numpy(np.array(c["x"])).to(DEV).requires_grad_(True)
    values = torch.from_numpy(np.array(c["values"]).view(np.int32)).to(DEV).view(torch.float32).requires_grad_(True)
    w = torch.from_numpy(np.array(c["grad"])).to(DEV)
    filled, dt, index, pixel, status = pkg.autograd.fill_values(x, values)
    assert filled.requires_grad and not any(t.requires_grad for t in (dt, index, pixel, status))
    want_dt, want_index = oracle.fill_batch(c["x"])[1:3]
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(dt.cpu().numpy(), want_dt)
    assert np.array_equal(pixel.cpu().numpy(), c["pixel"]) and np.array_equal(status.cpu().numpy(), c["status"])
    assert same_bits(filled.detach().view(torch.int32).cpu().numpy(), c["filled"])
    # a second call on another input does not overwrite the first call's tensors
    other = pkg.autograd.fill_values(torch.full_like(x, 3.0), values.detach())
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(pixel.cpu().numpy(), c["pixel"])
    assert (other[2].cpu().numpy() != want_index).any() and same_bits(filled.detach().view(torch.int32).cpu().numpy(), c["filled"])
    # d(sum(filled * w)) / d filled = w, bit for bit; x is a constant
    (filled * w).sum().backward()
    abi = run_backward(L, c, 0, calls=1, what="autograd")[0][0]
    assert x.grad is None and same_bits(values.grad.cpu().numpy(), abi) and bits_match(abi, c["grad_values"])
    # [B,H,W] values are C = 1, and filled comes back [B,H,W]
    v1 = values.detach()[:, 1].contiguous().requires_grad_(True)
    f1 = pkg.autograd.fill_values(x.detach(), v1)[0]
    assert f1.shape == x.shape and same_bits(f1.detach().view(torch.int32).cpu().numpy(), c["filled"][:, 1])
    (f1 * w[:, 1]).sum().backward()
    one = dict(c, C=1, grad=np.ascontiguousarray(c["grad"][:, 1:2]))
    assert v1.grad.shape == v1.shape and same_bits(v1.grad.cpu().numpy()[:, None], run_backward(L, one, 0, calls=1, what="C=1")[0][0])
    with pytest.raises(RuntimeError):  # once differentiable
        v2 = values.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad((pkg.autograd.fill_values(x.detach(), v2)[0] * w).sum(), v2, create_graph=True)
        g.sum().backward()

    # an unused filled: nothing is launched
    calls = []
    real = pkg.device.nearest_gather_backward_device
    monkeypatch.setattr(pkg.device, "nearest_gather_backward_device", lambda *a, **k: calls.append(1) or real(*a, **k))

    class Drop(torch.autograd.Function):  # hands a None gradient upstream
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            return None

    v3 = values.detach().clone().requires_grad_(True)
    f3 = pkg.autograd.fill_values(x.detach(), v3)[0]
    (Drop.apply(f3).sum() + (2 * v3).sum()).backward()
    assert not calls and (v3.grad == 2).all()
    v4 = values.detach().clone().requires_grad_(True)
    pkg.autograd.fill_values(x.detach(), v4)
    (2 * v4).sum().backward()
    assert not calls
    (pkg.autograd.fill_values(x.detach(), v4)[0] * w).sum().backward()
    assert calls == [1]
    with pytest.raises(ValueError):
        pkg.autograd.fill_values(x.detach()[0], values.detach())
    with pytest.raises(ValueError):
        pkg.autograd.fill_values(x.detach(), values.detach(), metric="l3")

    # the recipe: the raw LiDAR decides the sources, the corrected one in /90 units is the payload
    raw = x.detach()
    a = torch.tensor(1.25, device=DEV, requires_grad=True)
    corrected = (raw / 90) * a + 0.5
    fr = pkg.autograd.fill_values(raw, corrected)[0]
    want = R.gather(c["x"], c["index"], corrected.detach().cpu().numpy()[:, None])[0][:, 0]
    assert same_bits(fr.detach().cpu().numpy(), want) and (want[0] != 0).all() and not want[1].any()
    w1 = G.random_gradient(np.random.default_rng(5), (2, 1, 64, 96), nonfinite=False)  # finite: a.grad is one number
    (fr * torch.from_numpy(w1[:, 0]).to(DEV)).sum().backward()
    gv = R.backward(c["x"], c["index"], w1)[0][:, 0]  # d loss / d corrected, by the reference (the device gives its bits)
    want_a = float((gv.astype(np.float64) * (c["x"].astype(np.float64) / 90)).sum())
    scale = float((np.abs(gv.astype(np.float64)) * (c["x"].astype(np.float64) / 90)).sum())
    # torch forms x / 90 and each product in float32 (2^-24 relative each) and adds the 64 * 96 products of frame 0 (frame 1's
    # are zeros) in float32, every addition within 2^-24 of a partial sum that is at most `scale`
    assert abs(a.grad.item() - want_a) <= (64 * 96 + 2) * 2.0 ** -24 * scale


def test_no_host_synchronisation(L, pkg, oracle):
    """Forward and backward under torch's synchronisation debug mode: any blocking call raises."""
    import torch

    c = case("2x64x96-lidar-and-empty", pkg, oracle)
    w = torch.from_numpy(np.array(c["grad"])).to(DEV)
    x = torch.from_numpy(np.array(c["x"])).to(DEV)

    def step():
        v = torch.from_numpy(np.array(c["values"]).view(np.int32)).to(DEV).view(torch.float32).requires_grad_(True)
        torch.cuda.synchronize()
        return v

    v = step()
    (pkg.autograd.fill_values(x, v)[0] * w).sum().backward()  # the allocator's pools, the operator and the workspace exist
    warm = v.grad.cpu().numpy()
    v = step()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = pkg.autograd.fill_values(x, v)
        (out[0] * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert same_bits(v.grad.cpu().numpy(), warm) and bits_match(warm, c["grad_values"])
    assert np.array_equal(out[3].cpu().numpy(), c["pixel"])

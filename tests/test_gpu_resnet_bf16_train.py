"""The three trainable ResNets under precision = "bf16" on the device: the forward's bits are the inference class's under the same
precision; every wide layer's three gradients lie within their contracts (tests/convb_bf16_ref.py) on the tensors the tape
actually fed that layer, captured at conv.py's cores as tests/test_gpu_resnet_bf16.py captures the forward's calls; two runs give
the same bits; the default precision is the float32 tape bit for bit; one KerasAdam step runs without a host synchronisation
and leaves float32 parameters.  One frame of 16 x 32 (level 4 is 2 x 4), scale_num 4, and scale_num 1 for conv1a's half group."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import convb_bf16_ref as RHB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SHAPE = (1, 16, 32)
CLASSES = {"ResNet18Trainable": ("ResNet18", "glorot_weights_resnet18"),
           "ResNet18ImageTrainable": ("ResNet18Image", "glorot_weights_resnet18_image"),
           "ResNet18LightImageTrainable": ("ResNet18LightImage", "glorot_weights_resnet18_light_image")}


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


def _batch(image):
    import torch

    rng = np.random.default_rng(43)
    depth = rng.uniform(1, 80, SHAPE)
    lidar = np.where(rng.random(SHAPE) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random(SHAPE) < 0.65, depth + rng.normal(0, 0.5, SHAPE), 0).astype(F)
    rgb = (rng.integers(0, 256, SHAPE + (3,)).astype(F) / F(255.0)).astype(F)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return ((t(lidar), t(rgb)) if image else (t(lidar),)), t(gt)


def _model(net, cls, scale_num=4, precision=None):
    weights = getattr(net, CLASSES[cls][1])(700 + scale_num, scale_num, True, bias=0.1)
    model = getattr(net, cls)(weights, scale_num=scale_num, joint_train=True).to(DEV)
    if precision is not None:
        model.precision = precision
    return model, weights


def _step(pkg, model, inputs, gt):
    """train.py:232-253: the forward, the loss, backward().  Returns (total, output)."""
    output, correction = model(*inputs)
    main, aux = pkg.autograd.train_loss(output, gt, inputs[0], correction)
    total = main + aux
    total.backward()
    return total, output


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("cls", CLASSES)
def test_forward_bits_are_the_inference_class_under_bf16(net, cls):
    import torch

    inputs, _ = _batch(cls != "ResNet18Trainable")
    model, weights = _model(net, cls, precision="bf16")
    want = [t.clone() for t in getattr(net, CLASSES[cls][0])(weights, precision="bf16")(*inputs)]
    plain = [t.clone() for t in getattr(net, CLASSES[cls][0])(weights)(*inputs)]
    output, correct = model(*inputs)
    assert output.requires_grad and output.dtype == torch.float32
    C.assert_same(output.detach().cpu().numpy(), want[0].cpu().numpy(), "output * scale_range")
    C.assert_same(correct.detach().cpu().numpy(), want[1].cpu().numpy(), "lidar_correct * scale_range")
    assert not torch.equal(want[0], plain[0]) and torch.equal(want[1], plain[1])  # bf16 is another path; the head is float32


def _recorded_step(pkg, monkeypatch, model, inputs, gt):
    """One training step with conv.py's backward cores wrapped where autograd.py calls them; -> [record]."""
    autograd = pkg.autograd
    records = []

    def wrap(name):
        inner = getattr(autograd, name)

        def f(*args):
            out = inner(*args)
            records.append((name, args, out))
            return out

        return f

    with monkeypatch.context() as m:
        for name in ("_backward_data", "_backward_weights"):
            m.setattr(autograd, name, wrap(name))
        _step(pkg, model, inputs, gt)
    return records


@pytest.mark.parametrize("scale_num", (4, 1))
def test_every_wide_layers_gradients_within_their_contract(pkg, net, monkeypatch, scale_num):
    model, _ = _model(net, "ResNet18Trainable", scale_num, precision="bf16")
    inputs, gt = _batch(False)
    records = _recorded_step(pkg, monkeypatch, model, inputs, gt)
    n_wide = len(net.ResNet18(_model(net, "ResNet18Trainable", scale_num)[1], scale_num=scale_num).wide_layers)
    acts = {"leaky": C.LEAKY, "linear": C.LINEAR}
    worst = {"dx": 0.0, "dw": 0.0, "db": 0.0}
    seen = {"_backward_data": 0, "_backward_weights": 0}
    np_ = lambda t: None if t is None else t.detach().cpu().numpy()
    for name, args, out in records:
        kind, precision = args[0], args[-1]
        assert (precision == "bf16") == (kind in ("strided", "transposed")), (name, kind, precision)
        if precision != "bf16":
            continue
        seen[name] += 1
        tr = kind == "transposed"
        if name == "_backward_data":
            _, dy, w, stride, y, act, alpha, at, y_at, _, _, want_r, _ = args
            cout = w.shape[3]
            dys, ys = np_(dy)[..., at:at + cout], None if y is None else np_(y)[..., y_at:y_at + cout]
            dx, res = out if want_r else (out, None)
            want, S, n = RHB.dx_ref(dys, ys, np_(w), stride, acts[act], alpha, tr)
            ratio = np.abs(np_(dx).astype(np.float64) - want) / RHB.dx_bound(S, n)
            assert want.shape == tuple(dx.shape) and ratio.max() <= 1, ("dx", tuple(w.shape), stride, tr, ratio.max())
            worst["dx"] = max(worst["dx"], float(ratio.max()))
            if res is not None:
                C.assert_same(np_(res), RHB.g_ref(dys, ys, acts[act], alpha), "dresidual")
        else:
            _, x, dy, ksize, stride, y, act, alpha, at, y_at, cout, want_b, _ = args
            dys, ys = np_(dy)[..., at:at + cout], None if y is None else np_(y)[..., y_at:y_at + cout]
            dw, db = out
            want_w, want_bias, bw, bb = RHB.dw_ref(np_(x), dys, ys, ksize, stride, acts[act], alpha, tr)
            ratio = np.abs(np_(dw).astype(np.float64) - want_w) / bw
            assert want_w.shape == tuple(dw.shape) and ratio.max() <= 1, ("dw", tuple(dw.shape), stride, tr, ratio.max())
            worst["dw"] = max(worst["dw"], float(ratio.max()))
            if db is not None:
                ratio = np.abs(np_(db).astype(np.float64) - want_bias) / bb
                assert ratio.max() <= 1, ("db", tuple(dw.shape), stride, tr, ratio.max())
                worst["db"] = max(worst["db"], float(ratio.max()))
    assert seen["_backward_weights"] == n_wide and seen["_backward_data"] >= n_wide - 1, (seen, n_wide)
    print("ResNet18Trainable bf16, scale_num %d: worst |gradient - exact| / bound over %d wide layers: dx %.2e dw %.2e db %.2e"
          % (scale_num, n_wide, worst["dx"], worst["dw"], worst["db"]))


def test_two_runs_give_equal_bits_and_the_default_is_the_float32_tape(pkg, net):
    import torch

    inputs, gt = _batch(False)
    runs = {}
    for key, kw in (("bf16 a", dict(precision="bf16")), ("bf16 b", dict(precision="bf16")), ("default", {}), ("float32", dict(precision="float32"))):
        model, weights = _model(net, "ResNet18Trainable", **kw)
        total, output = _step(pkg, model, inputs, gt)
        runs[key] = (_grads(model), output.detach().clone(), total.detach().clone())
    for n, g in runs["bf16 a"][0].items():
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), n
        assert torch.equal(g.view(torch.int32), runs["bf16 b"][0][n].view(torch.int32)), "two bf16 runs: d " + n
        assert torch.equal(runs["default"][0][n].view(torch.int32), runs["float32"][0][n].view(torch.int32)), "default: d " + n
    want = net.ResNet18(weights)(*inputs)[0]
    assert torch.equal(runs["default"][1].view(torch.int32), want.view(torch.int32)), "the default forward is ResNet18's float32 bits"
    moved = [n for n, g in runs["bf16 a"][0].items() if not torch.equal(g, runs["float32"][0][n])]
    assert any(n.startswith("conv1a.") for n in moved), "bf16 took the float32 path"
    # for the record: how far the two tapes' gradients lie apart under glorot weights
    rel = {n: float((g - runs["float32"][0][n]).norm() / runs["float32"][0][n].norm().clamp_min(1e-30)) for n, g in runs["bf16 a"][0].items()}
    print("relative L2 distance of the bf16 tape's gradients from the float32 tape's: median %.3g, max %.3g (%s)"
          % (float(np.median(list(rel.values()))), max(rel.values()), max(rel, key=rel.get)))


@pytest.mark.parametrize("cls", CLASSES)
def test_one_keras_adam_step_without_a_host_synchronisation(pkg, net, cls):
    import torch

    inputs, gt = _batch(cls != "ResNet18Trainable")
    model, _ = _model(net, cls, precision="bf16")
    opt = pkg.optim.KerasAdam(model.parameters(), lr=1e-5)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    _step(pkg, model, inputs, gt)  # warm: the allocator's pools, the workspaces and the optimizer's state exist
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first, _ = _step(pkg, model, inputs, gt)
        opt.step()
        opt.zero_grad()
        with torch.no_grad():
            output, correction = model(*inputs)
            main, aux = pkg.autograd.train_loss(output, gt, inputs[0], correction)
            after = main + aux
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert p.dtype == torch.float32 and torch.isfinite(p).all(), n
        assert not torch.equal(p.detach(), before[n]), n + " did not move"
    assert np.isfinite(after.item()) and after.item() < first.item(), (first.item(), after.item())

"""SparsityCNNTrainable on the device: its forward against SparsityCNN bit for bit, the gradient of train.py:240-251's loss
with respect to every variable against tests/netgrad_ref.py bit for bit (+0 == -0), and one optimizer step without a host
synchronisation."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import netgrad_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
B, H, W = 2, 9, 33  # two frames, one above the forward's 8 x 32 tile each way


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


@pytest.fixture(scope="module")
def batch():
    """(lidar, gt): a third of the pixels carry a LiDAR return of 1 .. 80 m, two thirds a ground truth near it."""
    rng = np.random.default_rng(41)
    depth = rng.uniform(1, 80, (B, H, W))
    lidar = np.where(rng.random((B, H, W)) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random((B, H, W)) < 0.65, depth + rng.normal(0, 0.5, (B, H, W)), 0).astype(F)
    return lidar, gt


def _weights(net, scale_num=4, if_correct=True):
    return net.glorot_weights(200 + 10 * scale_num + if_correct, scale_num, if_correct, bias=0.1)


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 2, 3, 4))
def test_forward_bits_are_the_inference_class(net, batch, scale_num, if_correct):
    import torch

    weights = _weights(net, scale_num, if_correct)
    x = torch.from_numpy(batch[0]).to(DEV)
    want = [t.clone() for t in net.SparsityCNN(weights, if_correct=if_correct, scale_num=scale_num)(x)]
    model = net.SparsityCNNTrainable(weights, if_correct=if_correct, scale_num=scale_num).to(DEV)
    names = {n for n, _ in model.named_parameters()}
    assert names == {"%s.%s" % (layer, v) for layer in net.layer_shapes(scale_num, if_correct) for v in ("kernel", "bias")}
    output, correct = model(x)
    assert output.requires_grad and correct.requires_grad == if_correct
    C.assert_same(output.detach().cpu().numpy(), want[0].cpu().numpy(), "output * scale_range")
    C.assert_same(correct.detach().cpu().numpy(), want[1].cpu().numpy(), "lidar_correct * scale_range")
    assert want[0].abs().max().item() > 0


def _step(pkg, model, lidar, gt, correct=True, use=("main", "aux")):
    """train.py:232-253: the forward, the loss, backward().  Returns total."""
    output, correction = model(lidar)
    if correct:
        main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
        total = sum(t for name, t in (("main", main), ("aux", aux)) if name in use)
    else:
        total = pkg.autograd.train_loss(output, gt)[0]
    total.backward()
    return total


def _check_grads(model, want, what):
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        assert p.grad is not None, "%s: %s has no gradient" % (what, name)
        C.assert_same(p.grad.cpu().numpy(), want[layer][var == "bias"], "%s: d %s" % (what, name))
        assert np.isfinite(want[layer][0]).all() and (want[layer][0] != 0).any(), name


@pytest.mark.parametrize("joint_train", (False, True))
def test_every_gradient_is_netgrad_ref_bit_for_bit(pkg, net, batch, joint_train):
    """scale_num 4, if_correct and --correct: total = main + aux through every layer, lidar_conv_extra_1 through both its calls,
    and with joint_train through the fill's backward into the correction branch."""
    import torch

    weights = _weights(net)
    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    want, fw, stats = netgrad_ref.loss_gradients(batch[0], batch[1], weights, joint_train=joint_train)
    assert stats[2] > 100 and stats[3] > 20  # both losses have terms
    model = net.SparsityCNNTrainable(weights, joint_train=joint_train).to(DEV)
    total = _step(pkg, model, lidar, gt)
    assert total.item() == F(F(stats[0]) + F(stats[1]))
    _check_grads(model, want, "joint_train=%s" % joint_train)
    # a second step on the same batch: the same bits (gradients accumulate: x + x is exact)
    _step(pkg, model, lidar, gt)
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        C.assert_same(p.grad.cpu().numpy(), 2 * want[layer][var == "bias"], "twice: d " + name)


def test_the_correction_branch_learns_from_the_auxiliary_loss_alone(pkg, net, batch):
    """joint_train = False (net.py:157-162): the main loss reaches no variable of correct_1..4, the auxiliary loss reaches
    nothing else, and the branch's gradient under total is the auxiliary loss's."""
    import torch

    weights = _weights(net)
    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    branch = lambda name: name.startswith("correct_")
    grads = {}
    for use in (("main",), ("aux",), ("main", "aux")):
        model = net.SparsityCNNTrainable(weights).to(DEV)
        _step(pkg, model, lidar, gt, use=use)
        grads[use] = {n: p.grad for n, p in model.named_parameters()}
    for name in grads[("main",)]:
        if branch(name):
            assert grads[("main",)][name] is None, name
            assert torch.equal(grads[("aux",)][name], grads[("main", "aux")][name]) and grads[("aux",)][name].abs().max() > 0, name
        else:
            assert grads[("aux",)][name] is None, name
            assert torch.equal(grads[("main",)][name], grads[("main", "aux")][name]), name
    # with joint_train the main loss reaches the branch through the fill
    model = net.SparsityCNNTrainable(weights, joint_train=True).to(DEV)
    _step(pkg, model, lidar, gt, use=("main",))
    assert all(p.grad is not None and p.grad.abs().max() > 0 for n, p in model.named_parameters() if branch(n))


def test_without_the_correction(pkg, net, batch):
    """if_correct = False and no --correct: the main loss alone, bit for bit."""
    import torch

    weights = _weights(net, 2, False)
    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    want, _, _ = netgrad_ref.loss_gradients(batch[0], batch[1], weights, correct=False, if_correct=False, scale_num=2)
    model = net.SparsityCNNTrainable(weights, if_correct=False, scale_num=2).to(DEV)
    _step(pkg, model, lidar, gt, correct=False)
    _check_grads(model, want, "if_correct=False")


def test_one_adam_step_without_a_host_synchronisation(pkg, net, batch):
    """train.py:253-254 with torch.optim.Adam: every parameter moves, the loss on the same batch drops, and nothing between the
    forward and the optimizer's step blocks the host (torch's synchronisation debug mode raises on any blocking call)."""
    import torch

    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    model = net.SparsityCNNTrainable(_weights(net), joint_train=True).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, capturable=True)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    _step(pkg, model, lidar, gt)  # warm: the allocator's pools, the workspaces and Adam's state exist
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = _step(pkg, model, lidar, gt)
        opt.step()
        opt.zero_grad()
        with torch.no_grad():
            output, correction = model(lidar)
            main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
            after = main + aux
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n + " did not move"
    assert np.isfinite(after.item()) and after.item() < first.item(), (first.item(), after.item())

"""ResNet18Trainable on the device: its forward against ResNet18 bit for bit, the gradient of train.py:240-251's loss with
respect to every variable against tests/resnetgrad_ref.py bit for bit (+0 == -0), the two-term rule on the tape itself, and one
optimizer step without a host synchronisation.

The settings.  (1, 8, 72) with scale_num 4: level 1 has two column segments of the weight gradient, the second cut to 8 columns,
and level 4 is 1 x 9 pixels.  (2, 16, 24) with scale_num 1, test_gpu_resnet.py's frame: two frames, level 4 is 2 x 3.  Both with
joint_train off and on; the two share the numpy forward and everything behind the stems (resnetgrad_ref.backward_trunk).
The numpy reference of a setting's whole gradient, measured on the CPU the shapes were chosen on: 16 s for (1, 8, 72) at
scale_num 4 and 22 s for (2, 16, 24) at scale_num 1, each worked out once a module and shared.
"""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnetgrad_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SETTINGS = (((1, 8, 72), 4), ((2, 16, 24), 1))  # ((B, H, W), scale_num)


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


def batch(shape):
    """(lidar, gt): a third of the pixels carry a LiDAR return of 1 .. 80 m, two thirds a ground truth near it."""
    rng = np.random.default_rng(41)
    depth = rng.uniform(1, 80, shape)
    lidar = np.where(rng.random(shape) < 0.3, depth, 0).astype(F)
    gt = np.where(rng.random(shape) < 0.65, depth + rng.normal(0, 0.5, shape), 0).astype(F)
    return lidar, gt


def _weights(net, scale_num):
    return net.glorot_weights_resnet18(300 + scale_num, scale_num, True, bias=0.1)


_reference = {}


def reference(net, shape, scale_num):
    """({joint_train: {layer: (dw, db)}}, forward, stats) by resnetgrad_ref, once per setting."""
    key = (shape, scale_num)
    if key not in _reference:
        lidar, gt = batch(shape)
        _reference[key] = resnetgrad_ref.loss_gradients(lidar, gt, _weights(net, scale_num), joint_train=(False, True), scale_num=scale_num)
    return _reference[key]


def _step(pkg, model, lidar, gt):
    """train.py:232-253: the forward, the loss, backward().  Returns total."""
    output, correction = model(lidar)
    main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
    total = main + aux
    total.backward()
    return total


@pytest.mark.parametrize("shape,scale_num", SETTINGS)
def test_forward_bits_are_the_inference_class(net, shape, scale_num):
    import torch

    weights = _weights(net, scale_num)
    x = torch.from_numpy(batch(shape)[0]).to(DEV)
    want = [t.clone() for t in net.ResNet18(weights, scale_num=scale_num)(x)]
    model = net.ResNet18Trainable(weights, scale_num=scale_num).to(DEV)
    output, correct = model(x)
    assert output.requires_grad and correct.requires_grad
    C.assert_same(output.detach().cpu().numpy(), want[0].cpu().numpy(), "output * scale_range")
    C.assert_same(correct.detach().cpu().numpy(), want[1].cpu().numpy(), "lidar_correct * scale_range")
    assert want[0].abs().max().item() > 0
    again, _ = model(x)
    assert again.data_ptr() != output.data_ptr() and torch.equal(again, output)  # activations are new tensors of each call


@pytest.mark.parametrize("joint_train", (False, True))
@pytest.mark.parametrize("shape,scale_num", SETTINGS)
def test_every_gradient_is_resnetgrad_ref_bit_for_bit(pkg, net, shape, scale_num, joint_train):
    import torch

    weights = _weights(net, scale_num)
    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch(shape))
    wants, fw, stats = reference(net, shape, scale_num)
    want = wants[joint_train]
    assert stats[2] > 100 and stats[3] > 20  # both losses have terms
    model = net.ResNet18Trainable(weights, scale_num=scale_num, joint_train=joint_train).to(DEV)
    total = _step(pkg, model, lidar, gt)
    assert total.item() == F(F(stats[0]) + F(stats[1]))
    assert set(want) == set(net.layer_shapes_resnet18(scale_num, True))
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        assert p.grad is not None, name + " has no gradient"
        C.assert_same(p.grad.cpu().numpy(), want[layer][var == "bias"], "d " + name)
        assert np.isfinite(want[layer][0]).all() and (want[layer][0] != 0).any(), name
    # a second backward() on the same batch doubles the gradients exactly (x + x is exact)
    _step(pkg, model, lidar, gt)
    for name, p in model.named_parameters():
        layer, var = name.split(".")
        C.assert_same(p.grad.cpu().numpy(), 2 * want[layer][var == "bias"], "twice: d " + name)


def test_every_gradient_sum_of_the_tape_has_two_terms(net):
    """No (node, output) of the autograd graph has more than two consumers, so every float32 sum the engine makes is a + b,
    which is commutative: the order in which it runs the nodes cannot change a bit."""
    import torch

    shape, scale_num = SETTINGS[0]
    model = net.ResNet18Trainable(_weights(net, scale_num), scale_num=scale_num, joint_train=True).to(DEV)
    output, correct = model(torch.from_numpy(batch(shape)[0]).to(DEV))
    uses, seen, todo = {}, set(), [output.grad_fn, correct.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        for nxt, nr in node.next_functions:
            if nxt is not None:
                uses[(nxt, nr)] = uses.get((nxt, nr), 0) + 1
                todo.append(nxt)
    assert len(seen) > 100 and max(uses.values()) == 2
    three = [type(n).__name__ for (n, _), c in uses.items() if c > 2]
    assert not three, three


def test_one_adam_step_without_a_host_synchronisation(pkg, net):
    """train.py:253-254 with torch.optim.Adam: every parameter moves, the loss on the same batch drops, and nothing between the
    forward and the optimizer's step blocks the host (torch's synchronisation debug mode raises on any blocking call)."""
    import torch

    shape, scale_num = SETTINGS[0]
    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch(shape))
    model = net.ResNet18Trainable(_weights(net, scale_num), scale_num=scale_num, joint_train=True).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5, capturable=True)
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

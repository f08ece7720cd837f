"""KerasAdam under the trainable networks: train.py:232-254 whole, the forward, the loss, backward() and the optimizer's step,
with every variable after every step equal to tests/adam_ref.py applied to the gradients the device produced; no host
synchronisation in a warmed step; reset(), state_dict() and the lr schedule.

No captured-graph test: lr and the pointer lists are launch arguments, so a replay would freeze them (optim.py says so)."""
import numpy as np
import pytest

import adam_ref as A
from test_gpu_net_train import B, H, W, _step, _weights, batch, net  # noqa: F401  (the small shape, its batch and its weights)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


def _grads(model):
    """Every gradient copied to the host (the step may not be what changes them, but zero_grad() frees them)."""
    return {n: None if p.grad is None else p.grad.cpu().numpy().copy() for n, p in model.named_parameters()}


def _values(model):
    return {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}


class Reference:
    """adam_ref's copy of an optimizer: parameters, moments and state on the host."""

    def __init__(self, model):
        self.p = _values(model)
        self.m = {n: np.zeros_like(a) for n, a in self.p.items()}
        self.v = {n: np.zeros_like(a) for n, a in self.p.items()}
        self.state = A.adam_state0()

    def step(self, grads, lr):
        state = self.state
        for n, g in grads.items():
            if g is not None:
                self.p[n], self.m[n], self.v[n], state = A.adam_step_ref(self.p[n], g, self.m[n], self.v[n], self.state, lr)
        self.state = state

    def check(self, pkg, model, opt, what):
        for i, (n, p) in enumerate(model.named_parameters()):
            A.assert_same(p.detach().cpu().numpy(), self.p[n], "%s: %s" % (what, n))
            m, v = opt.moments(i)
            A.assert_same(m.cpu().numpy(), self.m[n], "%s: m of %s" % (what, n))
            A.assert_same(v.cpu().numpy(), self.v[n], "%s: v of %s" % (what, n))
        assert pkg.optim.read_record(opt.record) == self.state, what


def test_every_variable_of_sparsity_cnn_three_steps_and_the_schedule(pkg, net, batch):
    """Three steps on one batch, lr halved before the third (train.py:166-167).  Without joint_train the correction branch
    learns from the auxiliary loss alone; with `use` = main only in step 2 it has NO gradient there and must keep its values
    and its moments, while t advances for everybody."""
    import torch

    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    model = net.SparsityCNNTrainable(_weights(net)).to(DEV)
    opt = pkg.optim.KerasAdam(model.parameters(), lr=1e-3)
    assert len(opt.offsets) == 2 * len(net.layer_shapes()) < pkg._lib.ADAM_GROUP and opt.m.numel() == A.segment_offsets([p.numel() for p in model.parameters()])[1]
    ref = Reference(model)
    for step, (lr, use) in enumerate(((1e-3, ("main", "aux")), (1e-3, ("main",)), (5e-4, ("main", "aux"))), 1):
        opt.lr = lr
        _step(pkg, model, lidar, gt, use=use)
        grads = _grads(model)
        assert (sum(g is None for g in grads.values()) > 0) == (use == ("main",))
        before = _values(model)
        opt.step()
        opt.zero_grad()
        ref.step(grads, lr)
        ref.check(pkg, model, opt, "step %d" % step)
        for n, p in model.named_parameters():
            moved = not np.array_equal(p.detach().cpu().numpy(), before[n])
            assert moved == (grads[n] is not None), (step, n)
    assert pkg.optim.read_record(opt.record)[0] == 3


def test_a_warmed_step_never_waits_for_the_device(pkg, net, batch):
    """torch's synchronisation debug mode raises on any blocking call between the forward and the end of the step; the .grad
    tensors are new ones (zero_grad sets them to None), and the allocator hands the optimizer nothing."""
    import torch

    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    model = net.SparsityCNNTrainable(_weights(net), joint_train=True).to(DEV)
    opt = pkg.optim.KerasAdam(model.parameters(), lr=1e-4)
    _step(pkg, model, lidar, gt)  # warm: the allocator's pools and the workspaces exist
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    grads_first = [p.grad for p in model.parameters()]
    assert all(g is None for g in grads_first)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = _step(pkg, model, lidar, gt)
        allocated = torch.cuda.memory_allocated(DEV)
        opt.step()
        assert torch.cuda.memory_allocated(DEV) == allocated, "the step allocated on the device"
        opt.zero_grad()
        with torch.no_grad():
            output, correction = model(lidar)
            main, aux = pkg.autograd.train_loss(output, gt, lidar, correction)
            after = main + aux
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert pkg.optim.read_record(opt.record)[0] == 2
    assert np.isfinite(after.item()) and after.item() < first.item(), (first.item(), after.item())


def test_reset_and_resume(pkg, net, batch):
    """reset() is a new optimizer (train.py:169 builds one every epoch): the step after it is a first step.  state_dict() into
    a new instance over a copy of the model: the next step gives the same bits as the original's."""
    import torch

    lidar, gt = (torch.from_numpy(a).to(DEV) for a in batch)
    model = net.SparsityCNNTrainable(_weights(net), joint_train=True).to(DEV)
    opt = pkg.optim.KerasAdam(model.parameters(), lr=1e-3)
    for _ in range(2):
        _step(pkg, model, lidar, gt)
        opt.step()
        opt.zero_grad()
    # resume: a copy of the model and of the optimizer's state, one more step on both
    twin = net.SparsityCNNTrainable(_weights(net), joint_train=True).to(DEV)
    twin.load_state_dict(model.state_dict())
    state = opt.state_dict()
    assert (state["t"], state["b1p"], state["b2p"]) == A.adam_advance(A.adam_advance(A.adam_state0()))
    opt2 = pkg.optim.KerasAdam(twin.parameters(), lr=7.0, beta_1=0.5)  # (every setting comes from the state)
    opt2.load_state_dict(state)
    assert (opt2.lr, opt2.beta_1) == (1e-3, 0.9)
    for mdl, o in ((model, opt), (twin, opt2)):
        _step(pkg, mdl, lidar, gt)
        o.step()
        o.zero_grad()
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert p.data_ptr() != q.data_ptr()
        A.assert_same(q.detach().cpu().numpy(), p.detach().cpu().numpy(), "resumed: " + n)
    A.assert_same(opt2.m.cpu().numpy(), opt.m.cpu().numpy(), "resumed: m")
    A.assert_same(opt2.v.cpu().numpy(), opt.v.cpu().numpy(), "resumed: v")
    assert pkg.optim.read_record(opt2.record) == pkg.optim.read_record(opt.record) and pkg.optim.read_record(opt.record)[0] == 3
    with pytest.raises(ValueError):
        pkg.optim.KerasAdam([torch.zeros(3, device=DEV, requires_grad=True)], lr=1e-3).load_state_dict(state)
    # reset: the next step is adam_ref's first step from the values the model has now
    opt.reset()
    assert pkg.optim.read_record(opt.record) == A.adam_state0() and not opt.m.any() and not opt.v.any()
    ref = Reference(model)
    _step(pkg, model, lidar, gt)
    grads = _grads(model)
    opt.step()
    ref.step(grads, 1e-3)
    ref.check(pkg, model, opt, "after reset()")


def test_one_step_of_resnet18(pkg, net):
    """ResNet18Trainable at (1, 8, 72): 72 variables of 1 to 2 359 296 floats, 576 chunks the largest.  72 < DTFILL_ADAM_GROUP, so
    the step is ONE launch and does not cross the group seam; test_gpu_adam.py crosses it with made-up tensors."""
    import torch

    import test_gpu_resnet_train as R

    lidar, gt = (torch.from_numpy(a).to(DEV) for a in R.batch((1, 8, 72)))
    model = net.ResNet18Trainable(R._weights(net, 4), scale_num=4, joint_train=True).to(DEV)
    assert len(list(model.parameters())) == 72 < pkg._lib.ADAM_GROUP
    opt = pkg.optim.KerasAdam(model.parameters(), lr=1e-3)
    ref = Reference(model)
    R._step(pkg, model, lidar, gt)
    grads = _grads(model)
    assert all(g is not None for g in grads.values())
    opt.step()
    ref.step(grads, 1e-3)
    ref.check(pkg, model, opt, "ResNet18")

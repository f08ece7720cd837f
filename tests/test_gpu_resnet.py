"""ResNet18 on the device against tests/resnet_ref.py, bit for bit (+0 == -0, a NaN matches a NaN): the head, the residual
blocks at strides 1 and 2, the transposed convolutions, the concatenations and the elementwise steps together."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnet_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
BATCHES = ((1, 8, 16), (2, 16, 24))  # level 4 is 1 x 2 and 2 x 3 pixels


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


_want = {}


def want(net, synth, shape, scale_num, if_correct):
    """(frames, weights, resnet_ref's forward) of a setting, worked out once per module and shared (2 to 5 seconds each)."""
    key = (shape, scale_num, if_correct)
    if key not in _want:
        B, H, W = shape
        frames = synth.kitti_iid(B, p=0.2, seed=20 + H, hw=(H, W))
        weights = net.glorot_weights_resnet18(200 + 10 * scale_num + if_correct, scale_num, if_correct, bias=0.1)
        _want[key] = frames, weights, resnet_ref.forward(frames, weights, if_correct=if_correct, scale_num=scale_num)
    return _want[key]


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 4))
@pytest.mark.parametrize("shape", BATCHES)
def test_forward_is_resnet_ref_bit_for_bit(net, synth, shape, scale_num, if_correct):
    import torch

    frames, weights, ref = want(net, synth, shape, scale_num, if_correct)
    model = net.ResNet18(weights, if_correct=if_correct, scale_num=scale_num)
    x = torch.from_numpy(frames).to(DEV)
    output, correct = model(x)
    assert output.shape == correct.shape == shape and not output.requires_grad
    C.assert_same(correct.cpu().numpy(), ref["correct"], "lidar_correct * scale_range")
    C.assert_same(model._buffers[(x.device,) + shape].stems.cpu().numpy(), ref["stems"], "the stems")
    C.assert_same(output.cpu().numpy(), ref["output"], "output * scale_range")
    assert np.abs(ref["output"]).max() > 0 and (ref["correct"] != 0).any()


def test_second_call_allocates_nothing_and_returns_the_same_tensors(net, synth):
    import torch

    frames, weights, ref = want(net, synth, BATCHES[1], 4, True)
    model = net.ResNet18(weights)
    x = torch.from_numpy(frames).to(DEV).requires_grad_(True)  # detached: no graph is built, nothing is kept
    first = model(x)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    second = model(x)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    assert torch.cuda.max_memory_allocated(DEV) == before, "a call at a known shape allocated a temporary"
    assert second[0] is first[0] and second[1] is first[1]
    C.assert_same(second[0].cpu().numpy(), ref["output"], "second call")
    with pytest.raises(ValueError, match="multiples of 8"):
        model(torch.zeros((1, 12, 16), device=DEV))

"""ResNet18LightImage on the device against tests/resnet_light_image_ref.py, bit for bit (+0 == -0, a NaN matches a NaN), at every
scale_num and both values of if_correct: the outputs, the [image | total] tensor and the pooled channels of the three levels'
wide tensors, which the one pyramid call writes in place; and no allocation on the second call."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnet_light_image_ref as RL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
BATCHES = ((1, 8, 8), (2, 16, 24))  # level 4 is one pixel, and 2 x 3 pixels of two frames


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
    """(frames, rgb, weights, resnet_light_image_ref's forward) of a setting, worked out once per module and shared."""
    key = (shape, scale_num, if_correct)
    if key not in _want:
        B, H, W = shape
        frames = synth.kitti_iid(B, p=0.2, seed=20 + H, hw=(H, W))
        rgb = (np.random.default_rng(30 + H).integers(0, 256, shape + (3,)).astype(F) / F(255.0)).astype(F)
        weights = net.glorot_weights_resnet18_light_image(400 + 10 * scale_num + if_correct, scale_num, if_correct, bias=0.1)
        _want[key] = frames, rgb, weights, RL.forward(frames, rgb, weights, if_correct=if_correct, scale_num=scale_num)
    return _want[key]


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", BATCHES)
def test_forward_is_resnet_light_image_ref_bit_for_bit(net, synth, shape, scale_num, if_correct):
    import torch

    frames, rgb, weights, ref = want(net, synth, shape, scale_num, if_correct)
    model = net.ResNet18LightImage(weights, if_correct=if_correct, scale_num=scale_num)
    x, r = torch.from_numpy(frames).to(DEV), torch.from_numpy(rgb).to(DEV)
    output, correct = model(x, r)
    assert output.shape == correct.shape == shape and not output.requires_grad
    t = model._buffers[(x.device,) + shape]
    C.assert_same(correct.cpu().numpy(), ref["correct"], "lidar_correct * scale_range")
    C.assert_same(t.stems.cpu().numpy(), ref["stems"], "the stems")
    C.assert_same(t.total1.cpu().numpy(), ref["total1"], "[image | lidar_conv_total]")
    for level, k in ((2, 2), (3, 4), (4, 8)):  # the pooled channels directly, then the whole wide tensor
        C.assert_same(t.pooled[k][..., 64:].cpu().numpy(), ref["pooled"][level][..., 64:], "max_pool by %d of lidar_conv_total" % k)
        C.assert_same(t.pooled[k].cpu().numpy(), ref["pooled"][level], "the 128-wide tensor of level %d" % level)
    C.assert_same(output.cpu().numpy(), ref["output"], "output * scale_range")
    assert np.abs(ref["output"]).max() > 0 and (ref["total"] < 0).any() and (ref["pooled"][4][..., 64:] != 0).any()


def test_second_call_allocates_nothing_and_returns_the_same_tensors(net, synth):
    import torch

    frames, rgb, weights, ref = want(net, synth, BATCHES[1], 4, True)
    model = net.ResNet18LightImage(weights)
    x = torch.from_numpy(frames).to(DEV).requires_grad_(True)  # detached: no graph is built, nothing is kept
    r = torch.from_numpy(rgb).to(DEV).requires_grad_(True)
    first = model(x, r)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    second = model(x, r)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    assert torch.cuda.max_memory_allocated(DEV) == before, "a call at a known shape allocated a temporary"
    assert second[0] is first[0] and second[1] is first[1]
    C.assert_same(second[0].cpu().numpy(), ref["output"], "second call")
    with pytest.raises(ValueError, match="multiples of 8"):
        model(torch.zeros((1, 12, 16), device=DEV), torch.zeros((1, 12, 16, 3), device=DEV))
    for bad in (r.detach()[:1].contiguous(), r.detach()[..., :2].contiguous(), r.detach().double(), r.detach().cpu()):
        with pytest.raises(ValueError, match="input_rgb"):
            model(x, bad)

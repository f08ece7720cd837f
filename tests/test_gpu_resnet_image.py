"""ResNet18Image on the device against tests/resnet_image_ref.py, bit for bit (+0 == -0, a NaN matches a NaN), at every
scale_num and both values of if_correct; no allocation on the second call; the zeroed-image identity against ResNet18 on the
device; and the rgb_read_device -> ResNet18Image chain on a small uint8 image."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import resnet_image_ref as RI

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


def image(shape, seed):
    """uint8 [B,H,W,3] and what rgb_read emits of it: bytes / 255.0 in float32."""
    raw = np.random.default_rng(seed).integers(0, 256, shape + (3,)).astype(np.uint8)
    return raw, (raw.astype(F) / F(255.0)).astype(F)


_want = {}


def want(net, synth, shape, scale_num, if_correct):
    """(frames, rgb, weights, resnet_image_ref's forward) of a setting, worked out once per module and shared."""
    key = (shape, scale_num, if_correct)
    if key not in _want:
        B, H, W = shape
        frames = synth.kitti_iid(B, p=0.2, seed=20 + H, hw=(H, W))
        rgb = image(shape, 30 + H)[1]
        weights = net.glorot_weights_resnet18_image(200 + 10 * scale_num + if_correct, scale_num, if_correct, bias=0.1)
        _want[key] = frames, rgb, weights, RI.forward(frames, rgb, weights, if_correct=if_correct, scale_num=scale_num)
    return _want[key]


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", BATCHES)
def test_forward_is_resnet_image_ref_bit_for_bit(net, synth, shape, scale_num, if_correct):
    import torch

    frames, rgb, weights, ref = want(net, synth, shape, scale_num, if_correct)
    model = net.ResNet18Image(weights, if_correct=if_correct, scale_num=scale_num)
    x, r = torch.from_numpy(frames).to(DEV), torch.from_numpy(rgb).to(DEV)
    output, correct = model(x, r)
    assert output.shape == correct.shape == shape and not output.requires_grad
    C.assert_same(correct.cpu().numpy(), ref["correct"], "lidar_correct * scale_range")
    C.assert_same(model._buffers[(x.device,) + shape].stems.cpu().numpy(), ref["stems"], "[image | stems]")
    C.assert_same(output.cpu().numpy(), ref["output"], "output * scale_range")
    assert np.abs(ref["output"]).max() > 0 and (ref["stems"][..., :64] != 0).any()


def test_second_call_allocates_nothing_and_returns_the_same_tensors(net, synth):
    import torch

    frames, rgb, weights, ref = want(net, synth, BATCHES[1], 4, True)
    model = net.ResNet18Image(weights)
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


@pytest.mark.parametrize("scale_num", (1, 4))
def test_with_a_zeroed_image_layer_it_is_resnet18_on_the_device(net, synth, scale_num):
    """img_conv's kernel and bias zero: the image's groups add +-0 to the chains they stand in, and the outputs are ResNet18's
    under the three kernels with the image rows cut out."""
    import torch

    shape = BATCHES[1]
    frames, rgb, weights, _ = want(net, synth, shape, scale_num, True)
    weights = dict(weights, img_conv=tuple(np.zeros_like(a) for a in weights["img_conv"]))
    x, r = torch.from_numpy(frames).to(DEV), torch.from_numpy(rgb).to(DEV)
    got = [t.cpu().numpy() for t in net.ResNet18Image(weights, scale_num=scale_num)(x, r)]
    plain = [t.cpu().numpy() for t in net.ResNet18(RI.plain_weights(weights, scale_num), scale_num=scale_num)(x)]
    C.assert_same(got[0], plain[0], "output * scale_range")
    C.assert_same(got[1], plain[1], "lidar_correct * scale_range")
    assert np.abs(plain[0]).max() > 0


def test_rgb_read_device_into_the_network(pkg, net, synth):
    """The chain INTEGRATION.md gives: uint8 images -> rgb_read_device (resize to the frame, the row crop, / 255) -> the network's
    second input as it is, no copy between."""
    import torch

    shape = BATCHES[1]
    frames, rgb, weights, ref = want(net, synth, shape, 4, True)
    B, H, W = shape
    raw = image((B, H + 8, W), 30 + H)[0]  # 8 rows above the crop, which the drivers cut off (img_batch[:, 96:] at full size)
    raw[:, 8:] = image(shape, 30 + H)[0]
    _, r, status = pkg.device.rgb_read_device(torch.from_numpy(raw).to(DEV), size=(W, H + 8), first_row=8)
    assert r.shape == shape + (3,) and r.is_contiguous() and int(status.abs().sum()) == 0
    C.assert_same(r.cpu().numpy(), rgb, "rgb_read_device's frames")
    output, correct = net.ResNet18Image(weights)(torch.from_numpy(frames).to(DEV), r)
    C.assert_same(output.cpu().numpy(), ref["output"], "output * scale_range")

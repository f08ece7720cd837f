"""SparsityCNN on the device against tests/net_ref.py, bit for bit (+0 == -0, a NaN matches a NaN): the convolutions' chains, the
multi-channel fill's tap-order sums and the elementwise steps together, at every scale_num and both if_correct settings."""
import importlib

import numpy as np
import pytest

import conv_ref as C
import net_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
# two frames that span three of the conv kernels' 8 x 32 block tiles each way, neither a multiple of the tile
B, H, W = 2, 19, 70


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


@pytest.fixture(scope="module")
def frames(pkg):
    return importlib.import_module(pkg.__name__ + ".synth").kitti_iid(B, p=0.05, seed=19, hw=(H, W))


_want = {}


def want(net, frames, scale_num, if_correct):
    """(weights, net_ref's forward) of a setting, worked out once and shared."""
    key = (scale_num, if_correct)
    if key not in _want:
        weights = net.glorot_weights(100 + 10 * scale_num + if_correct, scale_num, if_correct, bias=0.1)
        _want[key] = weights, net_ref.forward(frames, weights, if_correct=if_correct, scale_num=scale_num)
    return _want[key]


@pytest.mark.parametrize("if_correct", (True, False))
@pytest.mark.parametrize("scale_num", (1, 2, 3, 4))
def test_forward_is_net_ref_bit_for_bit(net, frames, scale_num, if_correct):
    import torch

    weights, ref = want(net, frames, scale_num, if_correct)
    model = net.SparsityCNN(weights, if_correct=if_correct, scale_num=scale_num)
    x = torch.from_numpy(frames).to(DEV)
    output, correct = model(x)
    assert output.shape == correct.shape == (B, H, W) and not output.requires_grad
    C.assert_same(correct.cpu().numpy(), ref["correct"], "lidar_correct * scale_range")
    C.assert_same(model._buffers[(x.device, B, H, W)].stems.cpu().numpy(), ref["stems"], "the stems")
    C.assert_same(output.cpu().numpy(), ref["output"], "output * scale_range")
    assert np.abs(ref["output"]).max() > 0 and (ref["correct"] != 0).any()


def test_second_call_allocates_nothing_and_side_stream(net, frames):
    import torch

    weights, ref = want(net, frames, 4, True)
    model = net.SparsityCNN(weights)
    x = torch.from_numpy(frames).to(DEV).requires_grad_(True)  # detached: no graph is built, nothing is kept
    model(x)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    output, correct = model(x)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    assert torch.cuda.max_memory_allocated(DEV) == before, "a call at a known shape allocated a temporary"
    C.assert_same(output.cpu().numpy(), ref["output"], "second call")
    # on a stream of its own (the buffers of a shape are per instance: a fresh instance for the other stream)
    side = net.SparsityCNN(weights)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        xs = torch.from_numpy(frames).to(DEV)
        output, correct = side(xs)
    s.synchronize()
    C.assert_same(output.cpu().numpy(), ref["output"], "side stream: output")
    C.assert_same(correct.cpu().numpy(), ref["correct"], "side stream: correct")

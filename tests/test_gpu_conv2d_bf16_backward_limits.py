"""The bf16 backward calls (k_convhb_dw_wide, k_convhb_pack, and k_convh_wide behind the workspace plan) where
tests/test_gpu_conv2d_bf16_backward.py does not go: the twin of tests/test_gpu_conv2d_backward_limits.py, whose run_case, call and
workspace_bytes serve here (a record with bf16=True goes to the bf16 symbol).  tests/conv_cases.py has the cases (HBLOOP,
HBLARGE, HBREFUSED: WLOOP's, WLARGE's and WREFUSED's own records) and tests/test_conv_cases.py what they are held to on the CPU.

  A. k_convhb_dw_wide's second launch.  It has its own seg0 / gl0 loop: B = 21879 frames whose segment frame is 1 x 129, 65637
     segments, so that segment 65535 begins the second launch on a frame boundary and the launch ends inside a frame.  One call
     for each instantiation convhb_weights_launch asks for (1x1 and 3x3 at both strides, the transposed layer), the 3x3 stride-1
     one again 4 bytes off (VEC = false), and the two dx shapes on the bf16 data symbols.  The group axis's repeat (gl0) needs
     more than a million channels, a weight tensor past the shape rule's limit: no legal call reaches it, as for the twin.
  B. x, dy and y of the weight calls past byte offset 4 GiB (k_convhb_dw_wide's 32-bit fs and fl frame offsets, cast to size_t
     before the multiply by the channel count), a case past 2 GiB and one at the shape rule's largest batch; dy, dx, dresidual
     and the workspace of the data calls past 4 GiB, where the packed kernel (p.wt) lies behind a g of more than 4 GiB, and the
     1x1 stride-2 layer, where p.tmp is in use; the calls at exactly 2^31 elements refused on the bf16 symbols.

Tiles are small integers: every level-1 partial is exact in any order, so `want` is the int64 partials and level2() the
contract's stated float32 chain over them; dx and dresidual are exact integers, compared bit for bit on the device.
profiles/r35/bf16_backward_edges.txt has every case's device bytes and duration on one MI355X, and the seeded faults:
  k_convhb_dw_wide takes blockIdx.z without seg0   all six dw cases of A and "x at the limit" (112977 segments) fail: the later
                                                   segments' partials are still poison when level 2 adds them; the dx cases
                                                   pass; no test of test_gpu_conv2d_bf16_backward.py or test_gpu_resnet_bf16_train.py fails.
  the (size_t) cast dropped from fs * Cin          NOT a fault: fs, fl and Cin are unsigned and B H W Cin < 2^31 by the shape
                                                   rule, so the 32-bit product cannot wrap; every test passes, as it must.
  x's frame offset kept to 32 bits of BYTES        the fault of that kind that does wrap: both "x, dy and y past 4 GiB" dw cases and
                                                   "x at the limit" fail (every entry of dw); "x past 2 GiB" passes; no older test fails.
"""
import pytest

import conv_cases as CC
import conv_ref as R
import large_cases as LC
import test_gpu_conv2d_backward_limits as TW
from test_gpu_conv2d_limits import L, _release  # noqa: F401 (fixtures)
from test_gpu_large import need

pytestmark = pytest.mark.gpu


def _report(name, c, chunk):
    print("%s: B %d, %d segments, %.2f GB on the device" % (name, c["B"], CC.wsegments(c), CC.wdevice_bytes(c, chunk) / 1e9))


@pytest.mark.parametrize("name", list(CC.HBLOOP))
def test_the_second_launch(L, name):
    c = CC.HBLOOP[name]
    _report(name, c, CC.COMPARE_CHUNK)
    TW.run_case(L, name, c, CC.COMPARE_CHUNK)


@pytest.mark.parametrize("name", list(CC.HBLARGE))
def test_backward_tensors_past_2_gib_4_gib_and_at_the_limit(L, name):
    c = CC.HBLARGE[name]
    _report(name, c, LC.CHUNK_BYTES)
    if "workspace past 4 GiB" in name:  # the packed kernel and the 1x1 stride-2 values lie behind g
        assert TW.workspace_bytes(L, c) > 2 ** 32
    TW.run_case(L, name, c, LC.CHUNK_BYTES)


def test_calls_at_2_to_the_31_elements_are_refused(L):
    """WREFUSED's wide rows on the bf16 symbols: DTFILL_ERR_SHAPE at exactly 2^31 elements before any launch, so that small real
    buffers serve, and dtfill_conv2d_wide_backward_bf16_workspace_bytes answers 0 where the twin's does.  dx's rule stands
    behind the workspace check and gets a whole workspace."""
    import torch

    buf = lambda: torch.zeros(4096, dtype=torch.float32, device="cuda:0")  # noqa: E731
    x, w, b, out, y = buf(), buf(), buf(), buf(), buf()
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    assert small.data_ptr() % 256 == 0
    for entry, what, a in CC.HBREFUSED:
        assert CC.wrefused_count(entry, a) == 2 ** 31
        c = dict(a, entry=entry, act=R.LEAKY, bf16=True)
        nws = TW.workspace_bytes(L, c)
        assert (nws == 0) == bool(a.get("ws0")) == (TW.workspace_bytes(L, dict(c, bf16=False)) == 0), (entry, what, nws)
        ws = small
        if "dx_channels" in a:
            need(nws, "refused %s, %s: the workspace" % (entry, what))
            ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
            assert ws.data_ptr() % 256 == 0
        cout = a["cout"]
        grad = (out.data_ptr(), a.get("dy_channels", cout), 0, y.data_ptr(), a.get("y_channels", cout), 0)
        rc = TW.call(L, c, x.data_ptr(), grad, w.data_ptr(), x.data_ptr(), None, w.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.numel())
        assert rc == CC.ERR_SHAPE, (entry, what, rc)
        del ws
    torch.cuda.synchronize()
    for t in (x, w, b, out, y):
        assert not t.any()

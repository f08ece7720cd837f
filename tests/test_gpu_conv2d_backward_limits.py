"""The weight gradients of the wide, transposed and image layers (k_convb_dw_wide, k_convb_dw_image) and the data gradients of
the wide layers where tests/test_gpu_conv2d_wide_backward.py and test_gpu_conv2d_image.py do not go, by the method and with the
machinery of tests/test_gpu_conv2d_limits.py (tests/conv_cases.py has the cases, WLOOP; tests/test_conv_cases.py what they are
held to on the CPU):

  k_convb_dw_wide's second launch.  It takes its segment from the grid's z axis, and convb_dw_wide_launch repeats the launch
  from seg0 = 65535 on.  Frames whose segment frame is 1 x 129 have three segments, the last of one column, and B = 21879 of
  them 65637: segment 65535 is column 0 of frame 21845, so the second launch begins on a frame boundary and ends inside a
  frame.  One call for each instantiation dtfill.hip asks convb_dw_wide_launch for: stride 1 at ksize 1, 3, 5 and 7, stride 2
  at 1 and 3, and the transposed layer.  The group axis's repeat (gl0) needs more than a million channels, a weight tensor past
  the shape rule's own limit: no legal call reaches it, and it is left.
  The data gradients of the same shapes: the 1x1 stride-2 layer (k_convb_g, k_convb_flip, the forward kernel and
  k_convb_spread over B H W Cin elements) and the transposed one.
  k_convb_dw_image's item loop past CV_MAX_BLOCKS: one segment a frame and 2^20 + 101 frames at 3x3x3->16 and 7x7x4->16
  (thirteen row tiles), and 3x3x3->128 with two passes a segment and half as many frames, where a block's second item is
  another pass of another segment.

  Part B: dy, y, dx, dresidual and x of the four wide backward calls past byte offset 4 GiB (the data gradient's workspace, which
  holds g for the whole batch, with them), dy and y of the image layer's weight gradient and out of dtfill_conv2d_image
  past 4 GiB, a case past 2 GiB and one at the shape rule's largest batch per group, and the calls at exactly 2^31 elements
  refused.  x of the image layers has at most 4 channels and cannot pass 4 GiB within the rule.
  dy and y of every dw wide case are 16-byte aligned slices: the VEC = true bodies; one case of A runs again 4 bytes off, on
  the VEC = false body.

dw and db are level 1 on the tile and conv_cases.level2() over every segment; dx, dresidual and out are compared bit for bit on
the device.  profiles/r33/limits.txt has every case's device bytes and duration on one MI355X.

Mutation check (each built once on a scratch copy and run once; in the same profile):
  k_convb_dw_wide takes blockIdx.z without seg0    all seven dw wide cases of A fail (segments 65535 .. are still poison when level 2
                                                   adds them); the dx cases pass; no test of test_gpu_conv2d_wide_backward.py fails.
  k_convb_dw_image leaves its loop after one item  the three dw image cases of A fail; no test of test_gpu_conv2d_image.py fails.
"""
import numpy as np
import pytest

import conv_cases as CC
import conv_ref as R
import large_cases as LC
from test_gpu_conv2d_limits import L, _release, _tile as lim_tile, _up, poisoned, tiled, unchanged  # noqa: F401 (L, _release: fixtures)
from test_gpu_large import need, no_mismatch

pytestmark = pytest.mark.gpu

_tiles = {}


def _tile(name, c):
    if name not in _tiles:
        _tiles[name] = CC.wtile(c)
        for a in _tiles[name].values():
            if a is not None:
                a.setflags(write=False)
    return _tiles[name]


def _ptr(t):
    return None if t is None else t.data_ptr()


def workspace_bytes(L, c):
    B, H, W, cin, cout, ksize = (c[k] for k in ("B", "H", "W", "cin", "cout", "ksize"))
    if c["entry"] == "dw_image":
        return L.dtfill_conv2d_image_backward_workspace_bytes(B, H, W, cin, ksize, cout)
    if c.get("bf16"):
        return L.dtfill_conv2d_wide_backward_bf16_workspace_bytes(B, H, W, cin, ksize, cout, c.get("stride", 1), int(c.get("transposed", False)))
    return L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, cin, ksize, cout, c.get("stride", 1), int(c.get("transposed", False)))


def call(L, c, x, grad, w, dx, dres, dw, db, ws, nws):
    """The entry point of record c on raw pointers; grad: (dy, width, at, y, width, at).  bf16=True in the record: the bf16 twin
    of the wide call, under conv_cases.HBALPHA."""
    B, H, W, cin, cout, ksize, act = (c[k] for k in ("B", "H", "W", "cin", "cout", "ksize", "act"))
    stride, tr = c.get("stride", 1), c.get("transposed", False)
    dxc = c.get("dx_channels", cin)
    if c.get("bf16"):
        name = "dtfill_conv2d_%s_backward_%s_bf16" % ("transpose" if tr else "strided", "data" if c["entry"] == "dx_wide" else "weights")
        layer = (B, H, W, cin, cout) if tr else (B, H, W, cin, ksize, cout, stride)
        if c["entry"] == "dx_wide":
            return getattr(L, name)(*grad, w, *layer, act, CC.HBALPHA, dx, dxc, 0, *(() if tr else (dres,)), ws, nws, None)
        return getattr(L, name)(x, *grad, *layer, act, CC.HBALPHA, dw, db, ws, nws, None)
    if c["entry"] == "dx_wide":
        if tr:
            return L.dtfill_conv2d_transpose_backward_data(*grad, w, B, H, W, cin, cout, act, CC.ALPHA, dx, dxc, 0, ws, nws, None)
        return L.dtfill_conv2d_strided_backward_data(*grad, w, B, H, W, cin, ksize, cout, stride, act, CC.ALPHA, dx, dxc, 0, dres, ws, nws, None)
    tail = (act, CC.ALPHA, dw, db, ws, nws, None)
    if c["entry"] == "dw_image":
        return L.dtfill_conv2d_image_backward_weights(x, *grad, B, H, W, cin, ksize, cout, *tail)
    if tr:
        return L.dtfill_conv2d_transpose_backward_weights(x, *grad, B, H, W, cin, cout, *tail)
    return L.dtfill_conv2d_strided_backward_weights(x, *grad, B, H, W, cin, ksize, cout, stride, *tail)


def run_case(L, name, c, chunk):
    """Record c of conv_cases.WLOOP or WLARGE: the call on a tiled batch, dx and dresidual compared on the device, dw and db
    against level 2 over every segment, the inputs afterwards."""
    import torch

    d = _tile(name, c)
    B, H, W, cin, cout, ksize, act, mis = (c[k] for k in ("B", "H", "W", "cin", "cout", "ksize", "act", "mis"))
    width, at, nseg = c["width"], c["at"], CC.wsegments(c)
    (Ho, Wo), _ = CC.wframes(c)
    for key in ("x", "dy", "y"):
        LC.assert_alias_free(CC.T, d[key].size // CC.T)
    need(CC.wdevice_bytes(c, chunk), "%s: B %d, %d segments" % (name, B, nseg))
    nws = workspace_bytes(L, c)
    assert nws == CC.wworkspace_bytes(c)
    ws = LC.poison_bits(torch.empty(nws, dtype=torch.uint8, device="cuda:0"))
    assert ws.data_ptr() % 256 == 0
    dy, y = tiled(d["dy"], B, mis), (tiled(d["y"], B, mis) if act == R.LEAKY else None)
    grad = (dy.data_ptr(), width, at, _ptr(y), width, at)
    x = w = dx = dres = dw = db = None
    if c["entry"] == "dx_wide":
        w, dx = _up(d["w"]), poisoned((B, H, W, cin))
        dres = poisoned((B, Ho, Wo, cout)) if c["dres"] else None
    else:
        x, dw, db = tiled(d["x"], B, mis), poisoned((ksize, ksize, cin, cout)), poisoned((cout,))
    rc = call(L, c, _ptr(x), grad, _ptr(w), _ptr(dx), _ptr(dres), _ptr(dw), _ptr(db), ws.data_ptr(), nws)
    assert rc == 0, rc
    torch.cuda.synchronize()
    del ws
    if c["entry"] == "dx_wide":
        no_mismatch(LC.mismatching_frames(dx, _up(d["want"]), B, chunk_bytes=chunk), name + ": dx")
        if dres is not None:
            no_mismatch(LC.mismatching_frames(dres, _up(d["dres"]), B, chunk_bytes=chunk), name + ": dresidual")
        assert torch.equal(w, _up(d["w"]))
    else:
        want_dw, want_db = CC.split_dw(CC.level2(d["want"], nseg), ksize, cin)
        R.assert_same(dw.cpu().numpy(), want_dw, name + ": dw")
        R.assert_same(db.cpu().numpy(), want_db, name + ": db")
    unchanged((("x", x, d["x"]), ("dy", dy, d["dy"]), ("y", y, d["y"])), B, name, chunk)


@pytest.mark.parametrize("name", list(CC.WLOOP))
def test_the_second_launch_and_the_second_work_item(L, name):
    run_case(L, name, CC.WLOOP[name], CC.COMPARE_CHUNK)


@pytest.mark.parametrize("name", list(CC.WLARGE))
def test_backward_tensors_past_2_gib_4_gib_and_at_the_limit(L, name):
    c = CC.WLARGE[name]
    if "workspace past 4 GiB" in name:
        assert workspace_bytes(L, c) > 2 ** 32
    run_case(L, name, c, LC.CHUNK_BYTES)


@pytest.mark.parametrize("name", list(CC.ILARGE))
def test_image_forward_out_past_2_gib_4_gib_and_at_the_limit(L, name):
    """dtfill_conv2d_image: out past 2 GiB, past 4 GiB and, as the 16 channels at 16 of 128, at the shape rule's limit.  x has at
    most 4 channels and cannot pass 4 GiB within the rule."""
    import torch

    c = CC.ILARGE[name]
    d = lim_tile(name, c)
    B, cout, oc = c["B"], c["cout"], c.get("out_channels", c["cout"])
    for _, period in CC.periods(c, d):
        LC.assert_alias_free(CC.T, period // CC.T)
    need(CC.device_bytes(c, LC.CHUNK_BYTES), "%s: B %d" % (name, B))
    x, w, b = tiled(d["x"], B), _up(d["w"]), _up(d["bias"])
    out = poisoned((B,) + CC.out_frame(c) + (oc,))
    rc = L.dtfill_conv2d_image(x.data_ptr(), B, c["H"], c["W"], c["cin"], w.data_ptr(), b.data_ptr(), c["ksize"], cout, R.LEAKY, CC.ALPHA,
                               out.data_ptr(), oc, c.get("out_offset", 0), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    no_mismatch(LC.mismatching_frames(out, _up(d["want"]), B), name + ": out")
    unchanged((("x", x, d["x"]),), B, name, LC.CHUNK_BYTES)
    assert torch.equal(w, _up(d["w"])) and torch.equal(b, _up(d["bias"]))


def test_calls_at_2_to_the_31_elements_are_refused(L):
    """Exactly 2^31 elements of x, of dy (by Cout and by dy_channels), of y and of dx, for the image layer and its weight gradient
    and the four wide backward calls: DTFILL_ERR_SHAPE before any launch, so that small real buffers serve; where the count is
    the layer's own, the workspace size function answers 0 as well.  dx's rule stands behind the workspace check and gets a
    whole workspace."""
    import torch

    buf = lambda: torch.zeros(4096, dtype=torch.float32, device="cuda:0")  # noqa: E731
    x, w, b, out, y = buf(), buf(), buf(), buf(), buf()
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    assert small.data_ptr() % 256 == 0
    for entry, what, a in CC.WREFUSED:
        assert CC.wrefused_count(entry, a) == 2 ** 31
        if entry == "image":
            rc = L.dtfill_conv2d_image(x.data_ptr(), a["B"], a["H"], a["W"], a["cin"], w.data_ptr(), b.data_ptr(), a["ksize"], a["cout"], R.LEAKY,
                                       CC.ALPHA, out.data_ptr(), a.get("out_channels", a["cout"]), 0, None)
            assert rc == CC.ERR_SHAPE, (entry, what, rc)
            continue
        c = dict(a, entry=entry, act=R.LEAKY)
        nws = workspace_bytes(L, c)
        assert (nws == 0) == bool(a.get("ws0")), (entry, what, nws)
        ws = small
        if "dx_channels" in a:
            need(nws, "refused %s, %s: the workspace" % (entry, what))
            ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
            assert ws.data_ptr() % 256 == 0
        cout = a["cout"]
        grad = (out.data_ptr(), a.get("dy_channels", cout), 0, y.data_ptr(), a.get("y_channels", cout), 0)
        rc = call(L, c, x.data_ptr(), grad, w.data_ptr(), x.data_ptr(), None, w.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.numel())
        assert rc == CC.ERR_SHAPE, (entry, what, rc)
        del ws
    torch.cuda.synchronize()
    for t in (x, w, b, out, y):
        assert not t.any()

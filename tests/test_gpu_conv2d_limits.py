"""The five convolution entry points where their other tests do not go (tests/conv_cases.py has the cases,
tests/test_conv_cases.py what they are held to on the CPU):

A. past CV_MAX_BLOCKS = 2^20 work items, where a block of k_conv_mfma, k_conv_wide and k_convb_dw takes a second item: one
   call per kernel body on tiny frames, a hundred items past the grid; in one case per kernel a frame has 3 or 12 items, so
   that a block's second item differs from its first in the tile, parity or group and not only in the frame;
B. past 2 GiB, past 4 GiB and within a frame of the shape rule's limit (8 GiB of x): every tensor argument of every entry
   point extends past byte offset 4 GiB in some case, and the calls that stand exactly at 2^31 elements are refused;
C. over float32's range: subnormal operands on either side of the MFMA, sums that cross 2^-126 both ways, subnormal sums,
   sums that cross FLT_MAX inside the chain, an epilogue that underflows and overflows, and the same on the gradients.

A and B follow tests/test_gpu_large.py: a batch is a tile of T frames repeated on the device, the numpy reference runs on the
tile, every output is poisoned before the call and compared bit for bit on the device against expected[b % T], and the inputs
are compared with the tile again afterwards.  The tiles have no zero output (a zero's sign is the one thing the contracts
leave open), and every period has an odd factor.  dw and db are level 1 on the tile and level 2 as a loop of float32 row adds
over all 2^20-odd segments.  C runs through the other conv tests' run helpers on guarded buffers, against the same
references, with assert_same.

Mutation check (each built once on a scratch copy and run once; profiles/r23/conv_limits.txt has them beside every case's
device bytes and duration on the MI355X):
  the item loop left after the first item    k_conv_mfma: its three cases of A and the dx case fail; k_conv_wide: its four cases
                                             of A fail; k_convb_dw: its dw cases of A fail.  No other conv test fails in any
                                             of the three builds.
  a later item keeps its first item's tile     k_conv_wide decodes only the frame anew: the stride-2 and the transposed case of A
                                             fail in the frame where item 2^20 lies; the case with two items a frame passes.
  a 32-bit byte offset for a frame of x      k_conv_wide's `(size_t)it.b * a.H * a.W * Cin` kept to 30 bits of elements: "strided
                                             3x3x64->16 stride 2, x past 4 GiB" fails, first mismatching frames 56489, 56490, 56491:
                                             exactly the frames that start past 4 GiB.
  the same for conv_store's pixel * out_channels   "strided 1x1x16->64 at 16 of 80", "transpose 16->16, out past 4 GiB" and the
                                             dx case fail: frames 0 .. 3 (overwritten) and 56488 .. 56491 (still poison).
  built with -fgpu-flush-denormals-to-zero   all 12 forward and all 4 gradient cases of "subnormal x" and "subnormal w" fail,
                                             and so do "straddling", "tiny" and "leaky"; "huge" and tests/test_gpu_conv2d.py pass.
A narrowing of those element offsets to 32 bits, as opposed to byte offsets, changes nothing and was seen to pass: the shape
rule keeps every element offset below 2^31.
"""
import numpy as np
import pytest

import conv_cases as CC
import conv_ref as R
import convb_ref as RB
import large_cases as LC
import test_gpu_conv2d as fwd
import test_gpu_conv2d_backward as bwd
import test_gpu_conv2d_strided as strided
from test_gpu_large import need, no_mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
T = CC.T
POISON = CC.POISON


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


@pytest.fixture(autouse=True)
def _release():
    yield
    import torch

    torch.cuda.empty_cache()


def _up(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def tiled(tile, B, mis=0):
    """numpy tile [T, ...] -> a device tensor [B, ...] with frame b = tile[b % T], `mis` bytes off a 256-byte boundary."""
    import torch

    if tile is None:
        return None
    if not mis:
        return LC.upload_tiled(tile, B, DEV)
    t = _up(tile)
    n = B * int(np.prod(tile.shape[1:]))
    flat = torch.empty(n + mis // 4, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 256 == 0 and mis % 4 == 0
    return LC.fill_tiled(flat[mis // 4:].view((B,) + tuple(tile.shape[1:])), t)


def poisoned(shape):
    import torch

    return torch.full(tuple(shape), POISON, dtype=torch.int32, device=DEV).view(torch.float32)


def workspace(L, c):
    import torch

    nws = L.dtfill_conv2d_backward_workspace_bytes(c["B"], c["H"], c["W"], c["cin"], c["ksize"], c["cout"])
    assert nws == CC.workspace_bytes(c)
    ws = LC.poison_bits(torch.empty(nws, dtype=torch.uint8, device=DEV))
    assert ws.data_ptr() % 256 == 0
    return ws, nws


def unchanged(pairs, B, what, chunk):
    for name, t, tile in pairs:
        if t is not None:
            no_mismatch(LC.mismatching_frames(t, _up(tile), B, chunk_bytes=chunk), "%s: %s changed" % (what, name))


def run_tiled(L, what, c, chunk, mis=0):
    """Case c of conv_cases.LOOP or LARGE: the call on a tiled batch, the comparison on the device, the inputs afterwards."""
    import torch

    d = _tile(what, c)
    B, H, W, cin, cout, ksize = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["ksize"]
    for name, period in CC.periods(c, d):
        LC.assert_alias_free(T, period // T)
    need(CC.device_bytes(c, chunk), "%s%s: B %d, %d work items" % (what, ", x 4 bytes off" if mis else "", B, CC.items(c)))
    w = _up(d["w"])
    if c["entry"] in ("dx", "dw"):
        act, width, at = d["act"], d["width"], d["at"]
        dy, y = tiled(d["dy"], B, mis), (tiled(d["y"], B) if act == R.LEAKY else None)
        ws, nws = workspace(L, c)
        if c["entry"] == "dx":
            x, out = None, poisoned((B, H, W, cin))
            rc = L.dtfill_conv2d_backward_data(dy.data_ptr(), width, at, _ptr(y), width, at, w.data_ptr(), B, H, W, cin, ksize, cout, act,
                                               CC.ALPHA, out.data_ptr(), cin, 0, ws.data_ptr(), nws, None)
        else:
            x, dw, db = tiled(d["x"], B, mis), poisoned((ksize, ksize, cin, cout)), poisoned((cout,))
            rc = L.dtfill_conv2d_backward_weights(x.data_ptr(), dy.data_ptr(), width, at, _ptr(y), width, at, B, H, W, cin, ksize, cout,
                                                  act, CC.ALPHA, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nws, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        del ws
        if c["entry"] == "dx":
            no_mismatch(LC.mismatching_frames(out, _up(d["want"]), B, chunk_bytes=chunk), what + ": dx")
        else:
            nseg = B * CC.tiles(c)[0] * CC.tiles(c)[1]
            want_dw, want_db = CC.split_dw(CC.level2(d["want"], nseg), ksize, cin)
            R.assert_same(dw.cpu().numpy(), want_dw, what + ": dw")
            R.assert_same(db.cpu().numpy(), want_db, what + ": db")
        unchanged((("x", x, d["x"]), ("dy", dy, d["dy"]), ("y", y, d["y"])), B, what, chunk)
        assert torch.equal(w, _up(d["w"]))
        return
    Ho, Wo = CC.out_frame(c)
    oc, at = c.get("out_channels", cout), c.get("out_offset", 0)
    x, b, res = tiled(d["x"], B, mis), _up(d["bias"]), tiled(d["residual"], B)
    out = poisoned((B, Ho, Wo, oc))
    if c["entry"] == "conv2d":
        rc = L.dtfill_conv2d(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), ksize, cout, R.LEAKY, CC.ALPHA, out.data_ptr(), oc, at, None)
    elif c["entry"] == "strided":
        rc = L.dtfill_conv2d_strided(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), ksize, cout, c["stride"], _ptr(res), R.LEAKY,
                                     CC.ALPHA, out.data_ptr(), oc, at, None)
    else:
        rc = L.dtfill_conv2d_transpose(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), cout, R.LEAKY, CC.ALPHA, out.data_ptr(), oc, at,
                                       None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    # `want` is the whole out tensor of a period: the channels beside the slice hold the poison, which must have survived
    no_mismatch(LC.mismatching_frames(out, _up(d["want"]), B, chunk_bytes=chunk), what + ": out")
    unchanged((("x", x, d["x"]), ("residual", res, d["residual"])), B, what, chunk)
    assert torch.equal(w, _up(d["w"])) and torch.equal(b, _up(d["bias"]))


_tiles = {}


def _tile(what, c):
    """conv_cases.tile(c), worked out once: the aligned and the misaligned run share it, and it is left unchanged."""
    if what not in _tiles:
        _tiles[what] = CC.tile(c)
        for a in _tiles[what].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _tiles[what]


# ================================================================================================ A. past 2^20 work items
LOOP_RUNS = [(name, 0) for name in CC.LOOP] + [(name, 4) for name, c in CC.LOOP.items() if c.get("misaligned")]


@pytest.mark.parametrize("name,mis", LOOP_RUNS, ids=["%s%s" % (n, ", x 4 bytes off" if m else "") for n, m in LOOP_RUNS])
def test_a_block_takes_a_second_work_item(L, name, mis):
    c = CC.LOOP[name]
    assert CC.MAX_BLOCKS < CC.items(c) < CC.MAX_BLOCKS + 2 ** 10
    run_tiled(L, name, c, CC.COMPARE_CHUNK, mis)


# ================================================================================================ B. large tensors
@pytest.mark.parametrize("name", list(CC.LARGE))
def test_tensors_past_2_gib_4_gib_and_at_the_limit(L, name):
    run_tiled(L, name, CC.LARGE[name], LC.CHUNK_BYTES)


def test_calls_at_2_to_the_31_elements_are_refused(L):
    """Exactly 2^31 elements of x, of out (by Cout and by out_channels) and of the backward's dy, y and dx: DTFILL_ERR_SHAPE before
    any launch, so that small real buffers serve (dx's rule stands behind the workspace check and gets a whole workspace).  The
    calls just below each rule, which must run, are the "at the limit" cases above."""
    import torch

    buf = lambda: torch.zeros(4096, dtype=torch.float32, device=DEV)  # noqa: E731
    x, w, b, out, y = buf(), buf(), buf(), buf(), buf()
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    for entry, what, a in CC.REFUSED:
        assert CC.refused_count(entry, a) == 2 ** 31
        B, H, W, cin, cout, ksize = (a[k] for k in ("B", "H", "W", "cin", "cout", "ksize"))
        oc = a.get("out_channels", cout)
        if entry == "conv2d":
            rc = L.dtfill_conv2d(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), ksize, cout, R.LEAKY, CC.ALPHA, out.data_ptr(), oc, 0, None)
        elif entry == "strided":
            rc = L.dtfill_conv2d_strided(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), ksize, cout, a["stride"], None, R.LEAKY,
                                         CC.ALPHA, out.data_ptr(), oc, 0, None)
        elif entry == "transpose":
            rc = L.dtfill_conv2d_transpose(x.data_ptr(), B, H, W, cin, w.data_ptr(), b.data_ptr(), cout, R.LEAKY, CC.ALPHA, out.data_ptr(), oc, 0,
                                           None)
        elif entry == "dx":
            big = None
            if "dx_channels" in a:  # the rule behind the workspace check: a workspace of the size the call asks for
                nws = L.dtfill_conv2d_backward_workspace_bytes(B, H, W, cin, ksize, cout)
                need(nws, "refused dx, dx_channels at 2^31: the workspace")
                big = torch.empty(nws, dtype=torch.uint8, device=DEV)
                assert big.data_ptr() % 256 == 0
            rc = L.dtfill_conv2d_backward_data(x.data_ptr(), a.get("dy_channels", cout), 0, y.data_ptr(), a.get("y_channels", cout), 0,
                                               w.data_ptr(), B, H, W, cin, ksize, cout, R.LEAKY, CC.ALPHA, out.data_ptr(),
                                               a.get("dx_channels", cin), 0, (ws if big is None else big).data_ptr(),
                                               (ws if big is None else big).numel(), None)
            del big
        else:
            rc = L.dtfill_conv2d_backward_weights(x.data_ptr(), out.data_ptr(), a.get("dy_channels", cout), 0, y.data_ptr(),
                                                  a.get("y_channels", cout), 0, B, H, W, cin, ksize, cout, R.LEAKY, CC.ALPHA, w.data_ptr(),
                                                  b.data_ptr(), ws.data_ptr(), ws.numel(), None)
        assert rc == CC.ERR_SHAPE, (entry, what, rc)
    torch.cuda.synchronize()
    for t in (x, w, b, out, y):
        assert not t.any()


# ================================================================================================ C. float32's range
@pytest.mark.parametrize("entry,ksize,cin,cout,stride", CC.FORWARD_LAYERS,
                         ids=["%s %dx%dx%d->%d stride %d" % (e, k, k, ci, co, s) for e, k, ci, co, s in CC.FORWARD_LAYERS])
@pytest.mark.parametrize("name", list(CC.CLASSES))
def test_the_chain_over_float32s_range(L, name, entry, ksize, cin, cout, stride):
    for n, shape in enumerate(CC.SMALL_SHAPES):
        x, w, b = CC.class_case(name, ksize, cin, cout, shape, n, entry)
        want = CC.forward_ref(entry, x, w, b, stride)
        if entry == "conv2d":
            got = fwd.run(L, x, w, b, R.LEAKY)
        else:
            got = strided.run(L, x, w, b, R.LEAKY, stride, None, entry == "transpose")
        R.assert_same(got, want, "%s, %s %dx%dx%d->%d at %s" % (name, entry, ksize, ksize, cin, cout, shape))


@pytest.mark.parametrize("ksize,cin,cout", CC.BACKWARD_LAYERS, ids=["%dx%dx%d->%d" % (k, k, ci, co) for k, ci, co in CC.BACKWARD_LAYERS])
@pytest.mark.parametrize("name", CC.BACKWARD_CLASSES)
def test_the_gradients_over_float32s_range(L, name, ksize, cin, cout):
    for n, shape in enumerate(CC.SMALL_SHAPES):
        what = "%s, %dx%dx%d->%d at %s" % (name, ksize, ksize, cin, cout, shape)
        x, w, y, dy_dx, dy_dw = CC.backward_class_case(name, ksize, cin, cout, shape, n)
        R.assert_same(bwd.run_data(L, dy_dx, y, w, R.LEAKY), RB.dx_ref(dy_dx, y, w, R.LEAKY, CC.ALPHA), "dx, " + what)
        dw, db = RB.dw_ref(x, dy_dw, y, ksize, R.LEAKY, CC.ALPHA)
        got_dw, got_db = bwd.run_weights(L, x, dy_dw, y, ksize, R.LEAKY)
        R.assert_same(got_dw, dw, "dw, " + what)
        R.assert_same(got_db, db, "db, " + what)

"""dtfill_demo_multi_channel (k_gmcv7, k_gmcv, k_gmcv_first) on the device against the literal reference of tests/gmcv_ref.py,
through the C ABI, from poisoned and guarded buffers.

The bar is bit for bit (+0 and -0 equal), on every pixel of every output: include/dtfill.h fixes the order of the additions,
so a float32 evaluation has one result.  Every step of a scale_num 4 call is compared with the reference chained from the
input (not from the device's previous step), in the plain form and in the image form with C = 3 and C = 1, under
scale_range 90 and 1 (with 1 the outputs are the raw steps); scale_num 1..3 must give the first outputs of scale_num 4 bit for
bit.  Around every call: guards intact, inputs unchanged, nothing of the poison left in an output.

Cases: table sizes 3, 7, 11, 15; shapes 1 x 1, single rows and columns, one tile exactly, a tile plus one, several tiles with
an odd W -- each with every data kind (sparse 5 % on the KITTI k/256 grid, dense, signed with -0.0, sparse with the planted
ties and hand cases of gmcv_ref.plant) -- and 256 x 1216 at B = 8, with every data kind at table size 7 and the sparse KITTI
kind at the other sizes (the reference takes a minute per step there at table size 15)."""
import itertools

import numpy as np
import pytest

import gmcv_ref as V
from guarded import GuardedBuffer, is_poison, poison, poison_value, KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLE_SIZES = (3, 7, 11, 15)
SMALL_SHAPES = ((1, 1, 1), (2, 1, 97), (2, 97, 1), (2, 16, 64), (2, 17, 65), (1, 33, 131), (2, 70, 150))
KITTI_SHAPE = (8, 256, 1216)  # demo.py's [:, 96:] crop
_SEED = itertools.count(9100)


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def _guarded_input(a):
    import torch

    g = GuardedBuffer(a.nbytes, 0, DEV, frame_bytes=a[0].nbytes)
    g.view(torch.float32, a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return g


def run_device(L, x, rgb, ts, sn, sr, out_offset=0, null_ws=False):
    """One dtfill_demo_multi_channel call.  Inputs, outputs and workspace live in guarded allocations; the outputs hold the
    depth poison (a NaN no finite input produces), the workspace zero / one / random bytes in turn.  Returns the sn outputs
    as numpy arrays after checking the guards, the inputs and that no poison is left."""
    import torch

    seed = next(_SEED)
    B, H, W = x.shape
    C = 0 if rgb is None else rgb.shape[3]
    shape = (B, H, W) if rgb is None else (B, H, W, C + 1)
    nbytes = int(np.prod(shape)) * 4
    gx = _guarded_input(x)
    grgb = None if rgb is None else _guarded_input(rgb)
    outs = [GuardedBuffer(nbytes, out_offset, DEV, frame_bytes=nbytes // B) for _ in range(sn)]
    for o in outs:
        o.view(torch.int32, shape).fill_(int(poison_value("depth").view(np.int32)))
    need = L.dtfill_demo_multi_channel_workspace_bytes(B, H, W, sn)
    assert need == (0 if sn <= 2 else (sn - 2) * ((B * H * W * 4 + 255) // 256 * 256))
    ws = GuardedBuffer(need, 0, DEV, frame_bytes=H * W * 4)
    if need:
        poison(ws.payload(), KINDS[seed % 3], seed)
    ptrs = [o.ptr for o in outs] + [None] * (4 - sn)
    rc = L.dtfill_demo_multi_channel(gx.ptr, None if grgb is None else grgb.ptr, C, B, H, W, ts, sn, sr, *ptrs,
                                     None if null_ws else ws.ptr, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dtfill_strerror(rc).decode()
    torch.cuda.synchronize()
    what = "ts %d %s C %d sn %d sr %g" % (ts, x.shape, C, sn, sr)
    for k, g in enumerate([gx, grgb, ws] + outs):
        if g is not None:
            g.check("%s buffer %d" % (what, k))
    assert np.array_equal(gx.view(torch.float32, x.shape).cpu().numpy().view(np.uint32), x.view(np.uint32)), what + ": lidar changed"
    if rgb is not None:
        assert np.array_equal(grgb.view(torch.float32, rgb.shape).cpu().numpy().view(np.uint32), rgb.view(np.uint32)), what + ": rgb changed"
    got = [o.view(torch.float32, shape).cpu().numpy() for o in outs]
    for k, g in enumerate(got):
        assert not is_poison(g, "depth").any(), "%s: out_%d keeps poison" % (what, k + 1)
    return got


def check_case(L, x, ts, rng, what):
    """Every form and scale_range of one input against the reference chain; scale_num 1..3 against scale_num 4."""
    B, H, W = x.shape
    raws = V.chain(x, ts, 4)
    rgb3 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    rgb1 = rng.uniform(-1, 1, (B, H, W, 1)).astype(np.float32)
    for sr in (90.0, 1.0):
        for rgb in (None, rgb3, rgb1):
            form = "%s sr %g %s" % (what, sr, "plain" if rgb is None else "image C=%d" % rgb.shape[3])
            want = V.outputs(raws, rgb, sr)
            got = run_device(L, x, rgb, ts, 4, sr)
            for k in range(4):
                V.assert_same(got[k], want[k], "%s out_%d" % (form, k + 1))
            if sr == 1.0 and rgb is None:
                for k in range(4):
                    V.assert_same(got[k], raws[k], "%s raw_%d" % (form, k + 1))
            for sn in (1, 2, 3):
                less = run_device(L, x, rgb, ts, sn, sr, null_ws=sn <= 2 and B == 1)
                for k in range(sn):
                    assert np.array_equal(less[k].view(np.uint32), got[k].view(np.uint32)), "%s scale_num %d out_%d" % (form, sn, k + 1)


@pytest.mark.parametrize("ts", TABLE_SIZES)
def test_small_shapes_every_kind(L, ts):
    rng = np.random.default_rng(500 + ts)
    for shape in SMALL_SHAPES:
        for kind in V.DATA_KINDS:
            check_case(L, V.make_data(kind, rng, shape, ts), ts, rng, "ts %d %s %s" % (ts, shape, kind))


@pytest.mark.parametrize("ts,kind", [(7, k) for k in V.DATA_KINDS] + [(ts, "sparse") for ts in TABLE_SIZES if ts != 7])
def test_kitti_crop_batch(L, ts, kind):
    rng = np.random.default_rng(600 + ts)
    check_case(L, V.make_data(kind, rng, KITTI_SHAPE, ts), ts, rng, "ts %d %s %s" % (ts, KITTI_SHAPE, kind))


def test_planted_ties_reach_the_device(L):
    """The hand cases by value, not only by comparison: the farther larger depth, the cross-ring tie, the checkerboard, the
    empty window, the negative block and the value below 0.001, as the device's raw_2 (scale_range 1)."""
    x = V.plant(np.zeros((1, 40, 120), np.float32), 7)
    got = run_device(L, x, None, 7, 2, 1.0)[1][0]
    q = lambda total, n: np.float32(total) / (np.float32(0.000001) + np.float32(n))
    S, m = 17, 8
    assert got[m, m] == q(80.0, 1)
    assert got[m, S + m] == q(np.float32(2.5) + np.float32(25.0), 2)
    assert got[m, 2 * S + m] == q(4.0, 1) and got[m, 2 * S + m + 1] == q(16.0, 4)
    assert got[m, 3 * S + m] == 0
    assert got[m, 4 * S + m] < 0
    assert got[m, 5 * S + m] == q(0.0005, 1)


@pytest.mark.parametrize("ts", (7, 11))
def test_outputs_off_the_16_byte_grid(L, ts):
    """Outputs that start 4 bytes after a 16-byte boundary: the three-channel image form cannot store a pixel whole."""
    rng = np.random.default_rng(700 + ts)
    x = V.make_data("planted", rng, (2, 40, 130), ts)
    rgb = rng.uniform(0, 255, (2, 40, 130, 3)).astype(np.float32)
    raws = V.chain(x, ts, 4)
    for r, off in ((None, 4), (rgb, 4), (rgb, 8)):
        got = run_device(L, x, r, ts, 4, 90.0, out_offset=off)
        for k, want in enumerate(V.outputs(raws, r, 90.0)):
            V.assert_same(got[k], want, "ts %d offset %d out_%d" % (ts, off, k + 1))


def test_device_wrapper(pkg, L):
    import torch

    rng = np.random.default_rng(41)
    x = V.make_data("sparse", rng, (3, 20, 70))
    rgb = rng.uniform(0, 255, (3, 20, 70, 3)).astype(np.float32)
    xd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(rgb).to(DEV)
    outs = pkg.device.demo_multi_channel_device(xd, rd, table_size=7, scale_range=90.0, scale_num=2)
    assert len(outs) == 4 and outs[2] is None and outs[3] is None
    for k, want in enumerate(V.outputs(V.chain(x, 7, 2), rgb, 90.0)):
        V.assert_same(outs[k].cpu().numpy(), want, "wrapper out_%d" % (k + 1))
    outs = pkg.device.demo_multi_channel_device(xd)  # defaults: table 7, scale_range 90, scale_num 4, no image
    for k, want in enumerate(V.outputs(V.chain(x, 7, 4), None, 90.0)):
        V.assert_same(outs[k].cpu().numpy(), want, "wrapper defaults out_%d" % (k + 1))
    with pytest.raises(ValueError):
        pkg.device.demo_multi_channel_device(xd, rd[:, :, :-1])
    with pytest.raises(ValueError):
        pkg.device.demo_multi_channel_device(xd, scale_num=5)
    with pytest.raises(pkg.DtfillError):
        pkg.device.demo_multi_channel_device(xd, table_size=8)


def test_demo_module_on_a_kitti_crop_frame(pkg):
    """<package>.demo.*, numpy in and numpy out, as demo.py:309-313 calls them: one 256 x 1216 frame, table 7."""
    rng = np.random.default_rng(43)
    lidar = V.make_data("planted", rng, (1, 256, 1216))[..., None]
    rgb = rng.integers(0, 256, (1, 256, 1216, 3)).astype(np.float32)
    got = pkg.demo.generate_multi_channel(lidar, 7)
    want = V.generate_multi_channel(lidar, 7)
    for k in range(4):
        assert got[k].shape == (1, 256, 1216)
        V.assert_same(got[k], want[k], "demo.generate_multi_channel lidar_%d" % (k + 1))
    got = pkg.demo.generate_multi_channel_with_image(rgb, lidar, 7)
    want = V.generate_multi_channel_with_image(rgb, lidar, 7)
    for k in range(4):
        assert got[k].shape == (1, 256, 1216, 4)
        V.assert_same(got[k], want[k], "demo.generate_multi_channel_with_image lidar_%d" % (k + 1))
    got = pkg.demo.generate_multi_channel(lidar, 7, scale_range=1.0, scale_num=2)
    assert got[2] is None and got[3] is None
    V.assert_same(got[1], V.chain(lidar[..., 0], 7, 2)[1], "demo.generate_multi_channel raw_2")

"""depth_read on the device (dtfill_depth_read, depth_read_device, depth_read_batch, depth_read) against the numpy
statement in tests/read_ref.py, whose maps tests/test_read.py pins to Pillow's (tests/golden/read_maps.npz).  Bit-exact
everywhere; no test here needs Pillow except the PNG round trip, which skips without it."""
import importlib

import numpy as np
import pytest

import read_ref as R
from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output
from read_ref import golden_pairs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KITTI = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


def _frame(h, w, seed, density=0.05):
    """A KITTI-like 16-bit depth PNG frame: ~5 % valid values in [256, 65535], a few 255s and 65535s, zeros elsewhere."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w), np.uint16)
    u = rng.random((h, w))
    f[u < density] = rng.integers(256, 65536, int((u < density).sum()))
    f[(u >= density) & (u < density + 0.01)] = 255
    f[(u >= density + 0.01) & (u < density + 0.012)] = 65535
    f[0, 0] = 300  # every frame holds a value > 255, even a 1 x 1 one
    return f


def _padded(frames, fill=0xFFFF):
    """uint16 [B, hmax, wmax] with the padding poisoned, and the dims [B, 2]."""
    hmax = max(f.shape[0] for f in frames)
    wmax = max(f.shape[1] for f in frames)
    raw = np.full((len(frames), hmax, wmax), fill, np.uint16)
    for b, f in enumerate(frames):
        raw[b, :f.shape[0], :f.shape[1]] = f
    return raw, np.array([f.shape for f in frames], np.int32)


def _run(dev, raw, dims, H, W):
    import torch

    out, st = dev.depth_read_device(torch.from_numpy(raw).to(DEV), dims, (W, H))
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _assert_bits(got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%d pixels differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize("name", sorted(golden_pairs()))
def test_golden_pairs_bit_exact(dev, name):
    (h, w, H, W), ry, rx = golden_pairs()[name]
    frames = [_frame(h, w, seed) for seed in range(3)]
    raw = np.stack(frames)
    out, st = _run(dev, raw, None, H, W)
    for b, f in enumerate(frames):
        _assert_bits(out[b], f[ry][:, rx].astype(np.float32) / np.float32(256))  # Pillow's maps, straight from the file
    ref, rst = R.depth_read_batch(frames, H, W)
    _assert_bits(out, ref)
    assert not st.any()


def test_ragged_batch_padding_unread(dev):
    frames = [_frame(h, w, 10 + i) for i, (h, w) in enumerate(KITTI)]
    low = _frame(372, 1230, 20)
    low[low > 255] = 255  # max <= 255: the reference's assert
    frames.insert(2, low)
    raw, dims = _padded(frames, 0xFFFF)
    for H, W in ((352, 1216), (240, 320), (400, 1300)):
        out, st = _run(dev, raw, dims, H, W)
        ref, rst = R.depth_read_batch(frames, H, W)
        _assert_bits(out, ref)  # 0xFFFF padding would show as 255.99609375
        assert list(st) == [0, 0, R.NOT_16BIT, 0, 0] and list(rst) == list(st)
    # the check covers every source row, those no output row samples included: a frame whose only value > 255 sits in
    # such a row and column passes it, with an all-zero output; without that value it fails
    r = sorted(set(range(376)) - set(R.running_map(376, 352).tolist()))
    c = sorted(set(range(1241)) - set(R.running_map(1241, 1216).tolist()))
    f = np.zeros((376, 1241), np.uint16)
    f[r[len(r) // 2], c[-1]] = 256
    g = np.zeros((376, 1241), np.uint16)
    g[r[len(r) // 2], c[-1]] = 255
    raw, dims = _padded([f, g], 0xFFFF)
    out, st = _run(dev, raw, dims, 352, 1216)
    assert list(st) == [0, R.NOT_16BIT] and not out.any()


def test_bad_device_dims(dev):
    import torch

    frames = [_frame(40, 50, s) for s in range(6)]
    raw, dims = _padded(frames)
    dims[1] = (0, 50)
    dims[2] = (41, 50)  # > hmax
    dims[3] = (40, -1)
    dims[4] = (40, 51)  # > wmax
    out, st = dev.depth_read_device(torch.from_numpy(raw).to(DEV), torch.from_numpy(dims).to(DEV), (64, 32))
    torch.cuda.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert list(st) == [0, R.BAD_DIMS, R.BAD_DIMS, R.BAD_DIMS, R.BAD_DIMS, 0]
    assert not out[1:5].view(np.uint32).any()  # +0.0
    ref, _ = R.depth_read_batch([frames[0], frames[5]], 32, 64)
    _assert_bits(out[[0, 5]], ref)


def test_guarded_poisoned_misaligned_buffers(pkg, dev):
    import torch

    L = pkg._lib.load()
    rng = np.random.default_rng(7)
    cases = [([_frame(h, w, i) for i, (h, w) in enumerate(KITTI[:2])], 352, 1216, True),
             ([_frame(37, 61, 3), _frame(20, 13, 4), _frame(1, 1, 5)], 29, 45, True),  # W % 4 != 0: the scalar stores
             ([_frame(64, 96, 6), _frame(33, 70, 8)], 48, 100, False)]  # dims = NULL: the whole padded frame
    n = 0
    for frames, H, W, with_dims in cases:
        raw, dims = _padded(frames, 0xFFFF)
        if not with_dims:
            raw = rng.integers(0, 65536, raw.shape).astype(np.uint16)
            frames = list(raw)
        B, hmax, wmax = raw.shape
        nws = L.dtfill_depth_read_workspace_bytes(B, H, W)
        for ro, oo in ((0, 0), (2, 4), (6, 12), (130, 64), (64, 132)):
            kind = KINDS[n % 3]
            n += 1
            rg = GuardedBuffer(raw.nbytes, ro, DEV, hmax * wmax * 2)
            rg.view(torch.uint16, raw.shape).copy_(torch.from_numpy(raw))
            dg = GuardedBuffer(dims.nbytes, 0, DEV)
            dg.view(torch.int32, dims.shape).copy_(torch.from_numpy(dims))
            og = GuardedBuffer(B * H * W * 4, oo, DEV, H * W * 4)
            sg = GuardedBuffer(4 * B, oo, DEV)
            wg = GuardedBuffer(nws, 0, DEV)
            poison_output(og.view(torch.float32, (B, H, W)), "depth")
            poison_output(sg.view(torch.int32, (B,)), "status")
            poison(wg.payload(), kind, seed=n)
            rc = L.dtfill_depth_read(rg.ptr, dg.ptr if with_dims else None, B, hmax, wmax, H, W, og.ptr, sg.ptr, wg.ptr, nws,
                                     torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            for g, what in ((rg, "raw"), (dg, "dims"), (og, "out"), (sg, "status"), (wg, "workspace")):
                g.check(what)
            assert np.array_equal(rg.view(torch.uint16, raw.shape).cpu().numpy(), raw)
            out = og.view(torch.float32, (B, H, W)).cpu().numpy()
            st = sg.view(torch.int32, (B,)).cpu().numpy()
            assert not is_poison(out, "depth").any() and not is_poison(st, "status").any()
            ref, rst = R.depth_read_batch(frames, H, W)
            _assert_bits(out, ref)
            assert np.array_equal(st, rst)
    # status is nullable
    raw, dims = _padded([_frame(30, 40, 9)])
    rd = torch.from_numpy(raw).to(DEV)
    out = torch.empty((1, 16, 16), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.dtfill_depth_read_workspace_bytes(1, 16, 16), dtype=torch.uint8, device=DEV)
    assert L.dtfill_depth_read(rd.data_ptr(), None, 1, 30, 40, 16, 16, out.data_ptr(), None, ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    _assert_bits(out.cpu().numpy(), R.depth_read_batch([raw[0]], 16, 16)[0])


@pytest.mark.parametrize("outlier", [False, True])
def test_feeds_the_fill(pkg, dev, oracle, gpu_op, outlier):
    import torch

    frames = [_frame(h, w, 30 + i) for i, (h, w) in enumerate(KITTI)]
    raw, dims = _padded(frames, 0xFFFF)
    x, st = dev.depth_read_device(torch.from_numpy(raw).to(DEV), dims)
    res = gpu_op.run(x, outlier_removal=outlier)
    torch.cuda.synchronize()
    ref, _ = R.depth_read_batch(frames, 352, 1216)
    _assert_bits(x.cpu().numpy(), ref)
    if outlier:
        ref = np.stack([oracle.outlier_removal(f) for f in ref]).astype(np.float32)
    depth, dt, lbl, status = oracle.fill_batch(ref)
    assert np.array_equal(res["dt"].cpu().numpy(), dt)
    assert np.array_equal(res["index"].cpu().numpy(), lbl)
    assert np.array_equal(res["depth"].cpu().numpy(), depth)
    assert np.array_equal(res["status"].cpu().numpy() & 1, status)


def test_depth_read_batch_arrays_of_its_own(pkg, dev):
    frames = [_frame(h, w, 40 + i) for i, (h, w) in enumerate(KITTI)]
    a = pkg.depth_read_batch(frames)
    ref, _ = R.depth_read_batch(frames, 352, 1216)
    assert a.shape == (4, 352, 1216, 1) and a.dtype == np.float32
    _assert_bits(a[..., 0], ref)
    keep = a.copy()
    other = [_frame(h, w, 60 + i).astype(np.int64) for i, (h, w) in enumerate(KITTI)]  # the reference's dtype=int arrays
    b = pkg.depth_read_batch(other)
    assert not np.shares_memory(a, b)
    _assert_bits(a, keep)  # the second call did not write into the first result
    _assert_bits(b[..., 0], R.depth_read_batch(other, 352, 1216)[0])
    # size=None: the read_one_val path, / 256 without a resize
    same = [_frame(375, 1242, s) for s in (1, 2)]
    c = pkg.depth_read_batch(same, size=None)
    _assert_bits(c[..., 0], np.stack(same).astype(np.float32) / np.float32(256))
    with pytest.raises(ValueError):
        pkg.depth_read_batch(frames, size=None)
    c = pkg.depth_read_batch(same, size=(320, 240))
    assert c.shape == (2, 240, 320, 1)
    low = frames[3].copy()
    low[low > 255] = 7
    with pytest.raises(AssertionError, match="frame 1"):
        pkg.depth_read_batch([frames[0], low, low])
    got = pkg.depth_read_batch([frames[0], low], check=False)
    _assert_bits(got[..., 0], R.depth_read_batch([frames[0], low], 352, 1216)[0])


def test_depth_read_png(pkg, dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    f = _frame(375, 1242, 50)
    path = str(tmp_path / "depth.png")
    Image.fromarray(f).save(path)
    got = pkg.depth_read(path)
    assert got.shape == (352, 1216, 1) and got.dtype == np.float32
    _assert_bits(got[..., 0], R.depth_read_frame(f, 352, 1216)[0])
    _assert_bits(got, R.reference_depth_read(f))
    low = np.full((40, 50), 200, np.uint16)
    Image.fromarray(low).save(path)
    with pytest.raises(AssertionError, match=r"np.max\(depth_png\)=200, path="):
        pkg.depth_read(path)

"""rgb_read on the device (dtfill_rgb_read, rgb_read_device, rgb_read_batch, rgb_read) against the numpy statement in
tests/rgb_ref.py, which tests/test_rgb_read.py pins to Pillow's own resize and to its stored maps.  Bit for bit everywhere.
Every call through the C ABI here runs in guarded buffers with poisoned outputs and a poisoned workspace (_abi)."""
import functools
import importlib

import numpy as np
import pytest

import concurrency
import gmcv_ref as V
import near_ref as N
import rgb_ref as G
from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output
from read_ref import golden_pairs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KITTI = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))
U8_POISON = 0x5A  # no frame of _frame() holds it, so an out_u8 byte that still does was not written
LAYOUTS = ("nhwc", "nchw")


@pytest.fixture(scope="module")
def dev(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".device")


@functools.lru_cache(maxsize=None)
def _frame(h, w, C, seed=0):
    f = G.hashed_frame(h, w, C, seed)
    f[f == U8_POISON] = U8_POISON + 1
    f.setflags(write=False)
    return f


def _bits_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    as_bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    bad = as_bits(got) != as_bits(ref)
    assert not bad.any(), "%s: %d elements differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _abi(L, raw, dims, H, W, first_row=0, normalize=True, layout="nhwc", ro=0, uo=0, fo=0, want="both", kind="ones", seed=0,
         status=True):
    """dtfill_rgb_read on raw uint8 [B, hmax, wmax, C] (numpy) with raw / out_u8 / out_f32 at byte offsets ro / uo / fo from a
    256-byte boundary, every buffer between guards, the outputs and the workspace poisoned.  Checks the guards, that raw is
    unchanged and that no output element is left poisoned; returns (u8 or None, f32 or None, status or None) as numpy."""
    import torch

    raw = np.ascontiguousarray(raw)
    B, hmax, wmax, C = raw.shape
    OH = H - first_row
    n = B * OH * W * C
    nws = L.dtfill_rgb_read_workspace_bytes(B, H, W)
    assert nws > 0
    rg = GuardedBuffer(raw.nbytes, ro, DEV, hmax * wmax * C)
    rg.payload().copy_(torch.from_numpy(raw.reshape(-1).copy()))
    bufs = [(rg, "raw")]
    dg = ug = fg = sg = None
    if dims is not None:
        dg = GuardedBuffer(8 * B, 0, DEV)
        dg.view(torch.int32, (B, 2)).copy_(torch.from_numpy(np.asarray(dims, np.int32)))
        bufs.append((dg, "dims"))
    if want != "float":
        ug = GuardedBuffer(n, uo, DEV, OH * W * C)
        ug.payload().fill_(U8_POISON)
        bufs.append((ug, "out_u8"))
    if want != "uint8":
        fg = GuardedBuffer(4 * n, fo, DEV, 4 * OH * W * C)
        poison_output(fg.view(torch.float32, (n,)), "depth")
        bufs.append((fg, "out_f32"))
    if status:
        sg = GuardedBuffer(4 * B, 0, DEV)
        poison_output(sg.view(torch.int32, (B,)), "status")
        bufs.append((sg, "status"))
    wg = GuardedBuffer(nws, 0, DEV)
    poison(wg.payload(), kind, seed=seed)
    bufs.append((wg, "workspace"))
    ptr = lambda g: None if g is None else g.ptr
    rc = L.dtfill_rgb_read(rg.ptr, ptr(dg), B, hmax, wmax, C, H, W, first_row, int(normalize), LAYOUTS.index(layout), ptr(ug),
                           ptr(fg), ptr(sg), wg.ptr, nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, what in bufs:
        g.check(what)
    assert np.array_equal(rg.payload().cpu().numpy().reshape(raw.shape), raw), "raw changed"
    u8 = f32 = st = None
    if ug is not None:
        u8 = ug.payload().cpu().numpy().reshape(B, OH, W, C)
        assert not (u8 == U8_POISON).any(), "out_u8 bytes left unwritten"
    if fg is not None:
        f32 = fg.view(torch.float32, (B, OH, W, C) if layout == "nhwc" else (B, C, OH, W)).cpu().numpy()
        assert not is_poison(f32, "depth").any(), "out_f32 elements left unwritten"
    if sg is not None:
        st = sg.view(torch.int32, (B,)).cpu().numpy()
        assert not is_poison(st, "status").any()
    return u8, f32, st


def _dev_run(dev, raw, dims, H, W, **kw):
    import torch

    u8, f32, st = dev.rgb_read_device(torch.from_numpy(np.ascontiguousarray(raw).copy()).to(DEV), dims, (W, H), **kw)
    torch.cuda.synchronize()
    return (None if u8 is None else u8.cpu().numpy()), (None if f32 is None else f32.cpu().numpy()), st.cpu().numpy()


@pytest.mark.parametrize("name", sorted(golden_pairs()))
def test_golden_pairs_bit_exact(dev, name):
    (h, w, H, W), ry, rx = golden_pairs()[name]
    frames = [_frame(h, w, 3, seed) for seed in range(3)]
    maps = np.stack([f[ry][:, rx] for f in frames])  # Pillow's maps, straight from the file
    for layout in LAYOUTS:
        u8, f32, st = _dev_run(dev, np.stack(frames), None, H, W, want="both", layout=layout)
        ru8, rf32, rst = G.rgb_read_batch(frames, H, W, layout=layout)
        _bits_equal(u8, maps, "u8 against the stored maps")
        _bits_equal(f32, G.UNIT[maps] if layout == "nhwc" else G.UNIT[maps].transpose(0, 3, 1, 2), "f32 against the stored maps")
        _bits_equal(u8, ru8, "u8")
        _bits_equal(f32, rf32, "f32 " + layout)
        assert not st.any()


def test_division_table(pkg, dev):
    L = pkg._lib.load()
    i, j, c = np.meshgrid(np.arange(16), np.arange(16), np.arange(3), indexing="ij")
    f = ((16 * i + j + 85 * c) % 256).astype(np.uint8)
    assert all(len(set(f[..., k].ravel().tolist())) == 256 for k in range(3))
    ref = (np.arange(256) / 255.0).astype(np.float32)
    for layout in LAYOUTS:
        u8, f32, st = _dev_run(dev, f[None], None, 16, 16, want="both", layout=layout)
        want = ref[f][None] if layout == "nhwc" else ref[f].transpose(2, 0, 1)[None]
        _bits_equal(f32, want, "v / 255 " + layout)
        _bits_equal(u8, f[None], "identity")
        _, raw, _ = _dev_run(dev, f[None], None, 16, 16, layout=layout, normalize=False)
        assert np.array_equal(raw, (f if layout == "nhwc" else f.transpose(2, 0, 1))[None].astype(np.float32))
    # the same through the ABI at an odd raw address (the poison byte is one of the 256 values: float output only)
    _, f32, _ = _abi(L, f[None], None, 16, 16, ro=1, fo=4, want="float")
    _bits_equal(f32, ref[f][None], "v / 255, ABI")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_and_widths(pkg, C):
    L = pkg._lib.load()
    frames = [_frame(37, 61, C, 1), _frame(1, 1, C, 2), _frame(20, 13, C, 3)]  # (20, 13) -> (29, 45) is an upscale
    raw, dims = G.padded(frames)
    n = 0
    for H in (1, 29):
        for W in (1, 5, 45, 100):
            layout = LAYOUTS[n % 2]
            u8, f32, st = _abi(L, raw, dims, H, W, layout=layout, kind=KINDS[n % 3], seed=n)
            n += 1
            ru8, rf32, rst = G.rgb_read_batch(frames, H, W, layout=layout)
            _bits_equal(u8, ru8, "u8 C %d H %d W %d" % (C, H, W))
            _bits_equal(f32, rf32, "f32 C %d H %d W %d %s" % (C, H, W, layout))
            assert not st.any()


def test_first_row(pkg):
    L = pkg._lib.load()
    n = 0
    for frames, H, W, rows in (([_frame(375, 1242, 3, 4)], 352, 1216, (0, 96, 351)),
                               ([_frame(37, 61, 3, 5)] * 2, 29, 45, (0, 11, 28))):
        raw, dims = G.padded(frames)
        for first_row in rows:
            for layout in LAYOUTS:
                u8, f32, st = _abi(L, raw, dims, H, W, first_row=first_row, layout=layout, kind=KINDS[n % 3], seed=n)
                n += 1
                ru8, rf32, _ = G.rgb_read_batch(frames, H, W, first_row=first_row, layout=layout)
                assert u8.shape == (len(frames), H - first_row, W, 3)
                assert f32.shape == ((len(frames), H - first_row, W, 3) if layout == "nhwc" else (len(frames), 3, H - first_row, W))
                _bits_equal(u8, ru8, "u8 first_row %d" % first_row)
                _bits_equal(f32, rf32, "f32 first_row %d %s" % (first_row, layout))
                _bits_equal(u8, G.rgb_read_batch(frames, H, W)[0][:, first_row:], "the rows of the uncropped result")
                assert not st.any()


def test_ragged_batch_padding_unread(dev):
    frames = [_frame(h, w, 3, 10 + i) for i, (h, w) in enumerate(KITTI)]
    frames.insert(2, _frame(100, 300, 3, 20))
    raw, dims = G.padded(frames, 0xFF)  # padding that would read as 1.0
    for layout in LAYOUTS:
        u8, f32, st = _dev_run(dev, raw, dims, 352, 1216, first_row=96, want="both", layout=layout)
        ru8, rf32, _ = G.rgb_read_batch(frames, 352, 1216, first_row=96, layout=layout)
        _bits_equal(u8, ru8, "u8")
        _bits_equal(f32, rf32, "f32 " + layout)
        assert not st.any()


def test_bad_device_dims(pkg):
    L = pkg._lib.load()
    frames = [_frame(40, 50, 3, s) for s in range(6)]
    raw, dims = G.padded(frames)
    dims[1] = (0, 50)
    dims[2] = (41, 50)  # > hmax
    dims[3] = (40, -1)
    dims[4] = (40, 51)  # > wmax
    for layout in LAYOUTS:
        u8, f32, st = _abi(L, raw, dims, 32, 64, first_row=3, layout=layout, uo=1, fo=4)
        ru8, rf32, rst = G.rgb_read_batch(frames, 32, 64, first_row=3, layout=layout, dims=dims, hmax=40, wmax=50)
        assert list(st) == [0, G.BAD_DIMS, G.BAD_DIMS, G.BAD_DIMS, G.BAD_DIMS, 0] and list(rst) == list(st)
        assert not u8[1:5].any() and not f32[1:5].view(np.uint32).any()  # 0 and +0.0
        _bits_equal(u8, ru8, "u8")
        _bits_equal(f32, rf32, "f32 " + layout)
        u8, f32, st = _abi(L, raw, dims, 32, 64, first_row=3, layout=layout, status=False)  # frame_status = NULL
        assert st is None
        _bits_equal(u8, ru8, "u8, no status")
        _bits_equal(f32, rf32, "f32, no status")


def test_guarded_poisoned_misaligned_buffers(pkg):
    L = pkg._lib.load()
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (2, 64, 96, 4)).astype(np.uint8)
    noise[noise == U8_POISON] = 0
    cases = [([_frame(h, w, 3, i) for i, (h, w) in enumerate(KITTI[:2])], 352, 1216, 96, True),
             ([_frame(37, 61, 3, 3), _frame(20, 13, 3, 4), _frame(1, 1, 3, 5)], 29, 45, 0, True),  # W * C % 4 != 0
             (list(noise), 48, 100, 5, False),                    # dims = NULL: the whole padded frame
             ([_frame(30, 300, 3, 6), _frame(9, 131, 3, 7)], 7, 45, 2, True),     # more than 2 : 1 down: picks from global memory
             ([_frame(5, 3000, 3, 8), _frame(3, 2800, 3, 9)], 7, 1501, 1, True)]  # rows longer than the LDS image
    offsets = ((0, 0, 0), (1, 1, 4), (3, 5, 12), (13, 0, 132), (130, 1, 4))
    n = 0
    for frames, H, W, first_row, with_dims in cases:
        raw, dims = G.padded(frames, 0xFF)
        for ro, uo, fo in offsets:
            layout, normalize = LAYOUTS[n % 2], n % 4 < 3
            u8, f32, st = _abi(L, raw, dims if with_dims else None, H, W, first_row=first_row, normalize=normalize, layout=layout,
                               ro=ro, uo=uo, fo=fo, kind=KINDS[n % 3], seed=n)
            n += 1
            ru8, rf32, rst = G.rgb_read_batch(frames, H, W, first_row=first_row, normalize=normalize, layout=layout)
            _bits_equal(u8, ru8, "u8 %s offsets %s" % ((H, W), (ro, uo, fo)))
            _bits_equal(f32, rf32, "f32 %s offsets %s %s" % ((H, W), (ro, uo, fo), layout))
            assert np.array_equal(st, rst)
    # one output at a time
    frames = cases[1][0]
    raw, dims = G.padded(frames)
    ru8, rf32, _ = G.rgb_read_batch(frames, 29, 45, layout="nchw")
    u8, f32, _ = _abi(L, raw, dims, 29, 45, uo=5, want="uint8")
    assert f32 is None
    _bits_equal(u8, ru8, "u8 alone")
    u8, f32, _ = _abi(L, raw, dims, 29, 45, layout="nchw", fo=12, want="float")
    assert u8 is None
    _bits_equal(f32, rf32, "f32 alone")


def test_feeds_its_consumers(pkg, dev, gpu_op):
    import torch

    B, H, W = 2, 40, 64
    frames = [_frame(45, 70, 3, 30), _frame(43, 66, 3, 31)]
    raw, dims = G.padded(frames)
    rd = torch.from_numpy(raw).to(DEV)
    lidar = V.make_data("sparse", np.random.default_rng(5), (B, H, W))
    xd = torch.from_numpy(lidar).to(DEV)
    # NHWC -> the demo driver's value-weighted fill with image
    _, rgb, _ = dev.rgb_read_device(rd, dims, (W, H))
    outs = dev.demo_multi_channel_device(xd, rgb)
    want = V.generate_multi_channel_with_image(G.rgb_read_batch(frames, H, W)[1], lidar[..., None], 7)
    for k in range(4):
        V.assert_same(outs[k].cpu().numpy(), want[k], "demo_multi_channel out_%d" % (k + 1))
    # NCHW -> the fill's labels -> every channel from the nearest source
    _, values, _ = dev.rgb_read_device(rd, dims, (W, H), layout="nchw")
    index = gpu_op.run(xd, want=("index",))["index"]
    filled, pixel, st = dev.nearest_gather_device(xd, index, values)
    torch.cuda.synchronize()
    rfilled, rpixel, rst = N.gather(lidar, index.cpu().numpy(), G.rgb_read_batch(frames, H, W, layout="nchw")[1])
    _bits_equal(filled.cpu().numpy(), rfilled, "nearest_gather filled")
    assert np.array_equal(pixel.cpu().numpy(), rpixel) and np.array_equal(st.cpu().numpy(), rst)


def test_rgb_read_batch_arrays_of_its_own(pkg, dev):
    frames = [_frame(h, w, 3, 40 + i) for i, (h, w) in enumerate(KITTI)]
    a = pkg.rgb_read_batch(frames)
    ru8, rf32, _ = G.rgb_read_batch(frames, 352, 1216)
    assert a.shape == (4, 352, 1216, 3)
    _bits_equal(a, ru8, "uint8")
    keep = a.copy()
    other = [_frame(h, w, 3, 60 + i).astype(np.int64) for i, (h, w) in enumerate(KITTI)]  # any integer dtype that fits
    b = pkg.rgb_read_batch(other, first_row=96, dtype=np.float32)
    assert not np.shares_memory(a, b)
    _bits_equal(a, keep, "the first result after the second call")
    _bits_equal(b, G.rgb_read_batch([f.astype(np.uint8) for f in other], 352, 1216, first_row=96)[1], "float32, first_row 96")
    # the reference's own two lines on the uint8 form
    _bits_equal(b, np.asarray(pkg.rgb_read_batch(other)[:, 96:] / 255.0).astype(np.float32), "img_batch[:, 96:] / 255.0")
    # size=None: the read_one_val path, no resize
    same = [_frame(375, 1242, 3, s) for s in (1, 2)]
    _bits_equal(pkg.rgb_read_batch(same, size=None), np.stack(same), "size=None")
    with pytest.raises(ValueError):
        pkg.rgb_read_batch(frames, size=None)
    c = pkg.rgb_read_batch(same, size=(320, 240), first_row=40)
    assert c.shape == (2, 200, 320, 3)
    # greyscale frames keep the reference's rank; four channels
    grey = [_frame(h, w, 1, 70 + i)[..., 0] for i, (h, w) in enumerate(KITTI[:2])]
    g = pkg.rgb_read_batch(grey)
    _bits_equal(g, np.stack([G.resize(f, 352, 1216) for f in grey]), "greyscale")
    rgba = [_frame(37, 61, 4, 80), _frame(20, 13, 4, 81)]
    _bits_equal(pkg.rgb_read_batch(rgba, size=(45, 29), dtype=np.float32), G.rgb_read_batch(rgba, 29, 45)[1], "RGBA")


def test_rgb_read_png(pkg, dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    nearest = Image.Resampling.NEAREST if hasattr(Image, "Resampling") else Image.NEAREST
    for C, shape in ((3, (352, 1216, 3)), (1, (352, 1216)), (4, (352, 1216, 4))):
        f = _frame(375, 1242, C, 50 + C)
        path = str(tmp_path / ("image%d.png" % C))
        Image.fromarray(f[..., 0] if C == 1 else f).save(path)
        got = pkg.rgb_read(path)
        img_file = Image.open(path)  # data_read.py:68-72
        rgb_png = np.array(img_file, dtype="uint8")
        ref = np.array(Image.fromarray(rgb_png).resize((1216, 352), nearest))
        img_file.close()
        assert got.shape == shape and ref.shape == shape
        _bits_equal(got, ref, "rgb_read, %d channel(s)" % C)
    deep = np.full((40, 50), 300, np.uint16)  # a 16-bit PNG: the reference's dtype='uint8' wraps it
    path = str(tmp_path / "deep.png")
    Image.fromarray(deep).save(path)
    with pytest.raises(TypeError):
        pkg.rgb_read(path)


@functools.lru_cache(maxsize=None)
def _thread_case(k):
    frames = [_frame(h, w, 3, 100 + 10 * k + i) for i, (h, w) in enumerate(KITTI[k % 2:k % 2 + 2])]
    ru8, rf32, _ = G.rgb_read_batch(frames, 352, 1216, first_row=96)
    for a in (ru8, rf32):
        a.setflags(write=False)
    return frames, ru8, rf32


def test_threads_and_streams(pkg, dev):
    import torch

    cases = [_thread_case(k) for k in range(4)]
    pkg.rgb_read_batch(cases[0][0])  # the default operator exists

    def work(k, r):
        frames, ru8, rf32 = cases[k]
        if (k + r) % 2:
            got = pkg.rgb_read_batch(frames, first_row=96)
            assert got.dtype == np.uint8 and np.array_equal(got, ru8), "uint8"
        else:
            got = pkg.rgb_read_batch(frames, first_row=96, dtype=np.float32)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), rf32.view(np.uint32)), "float32"

    failures = concurrency.run_rounds(work, 4, 3)
    assert not failures, concurrency.describe(failures)
    # the same call on two streams, both queued before either is waited for
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    raws = [G.padded(cases[k][0]) for k in range(2)]
    rd = [(torch.from_numpy(raw).to(DEV), torch.from_numpy(dims).to(DEV)) for raw, dims in raws]
    torch.cuda.synchronize()
    res = []
    for s, (raw, dims) in zip(streams, rd):
        with torch.cuda.stream(s):
            res.append(dev.rgb_read_device(raw, dims, first_row=96, want="both"))
    torch.cuda.synchronize()
    for k, (u8, f32, st) in enumerate(res):
        _bits_equal(u8.cpu().numpy(), cases[k][1], "stream %d u8" % k)
        _bits_equal(f32.cpu().numpy(), cases[k][2], "stream %d f32" % k)
        assert not st.cpu().numpy().any()

"""depth_read (data_read.py:81-99) without a GPU: the numpy statement in tests/read_ref.py against Pillow's maps
(tests/golden/read_maps.npz) and, where Pillow imports, against a reference-style depth_read; the ABI's argument errors."""
import os

import numpy as np
import pytest

import read_ref as R
from read_ref import golden_pairs


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


@pytest.mark.parametrize("name", sorted(golden_pairs()))
def test_statement_maps_equal_pillow_maps(name):
    (h, w, H, W), ry, rx = golden_pairs()[name]
    assert ry.shape == (H,) and rx.shape == (W,)
    assert np.array_equal(R.running_map(h, H), ry) and np.array_equal(R.running_map(w, W), rx)
    assert (np.diff(ry) >= 0).all() and ry[-1] < h and (np.diff(rx) >= 0).all() and rx[-1] < w


def test_golden_covers_the_issue_pairs():
    pairs = {v[0] for v in golden_pairs().values()}
    for hw in ((375, 1242), (370, 1224), (374, 1238), (376, 1241), (352, 1216), (480, 640), (240, 320), (1, 1), (1000, 7),
               (100, 3000)):
        assert hw + (352, 1216) in pairs, hw
    assert (352, 320, 240, 320) in pairs


def test_closed_form_is_not_pillows():
    g = golden_pairs()
    (h, w, H, W), ry, rx = g["vga_480x640"]
    assert not np.array_equal(R.closed_form_map(w, W), rx)  # 640 -> 1216 columns
    (h, w, H, W), ry, rx = g["nyu_352x320_to_240x320"]
    assert not np.array_equal(R.closed_form_map(h, H), ry)
    # the KITTI raw sizes happen to agree
    (h, w, H, W), ry, rx = g["kitti_375x1242"]
    assert np.array_equal(R.closed_form_map(h, H), ry) and np.array_equal(R.closed_form_map(w, W), rx)


def _frames(seed):
    """Random frames over the KITTI sizes and a few odd ones, values drawn from 0, 255, 256, 65535 and the rest of the range."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in ((375, 1242), (370, 1224), (37, 61), (480, 640), (5, 3)):
        f = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        pick = rng.random((h, w))
        f[pick < 0.5] = 0
        f[(pick >= 0.5) & (pick < 0.6)] = 255
        f[(pick >= 0.6) & (pick < 0.7)] = 256
        f[(pick >= 0.7) & (pick < 0.75)] = 65535
        out.append(f)
    return out


def test_statement_equals_reference_style_depth_read():
    if _pillow() is None:
        pytest.skip("Pillow is not installed")
    for size in ((1216, 352), (320, 240), (1242, 375)):
        for f in _frames(3):
            ref = R.reference_depth_read(f.astype(np.int64), size)
            got, st = R.depth_read_frame(f, size[1], size[0])
            assert ref.dtype == np.float32 and ref.shape == (size[1], size[0], 1)
            assert np.array_equal(ref[..., 0].view(np.uint32), got.view(np.uint32)), (f.shape, size)
            assert st == 0


def test_statement_status():
    f = np.full((4, 6), 255, np.uint16)
    assert R.depth_read_frame(f, 3, 3)[1] == R.NOT_16BIT
    f[3, 5] = 256  # a value no output pixel samples still counts
    out, st = R.depth_read_frame(f, 2, 2)
    assert st == 0 and (out == np.float32(255 / 256)).all()


def test_argument_errors_without_gpu(pkg):
    L = pkg.load()
    ws = L.dtfill_depth_read_workspace_bytes(2, 352, 1216)
    assert ws >= 2 * 352 * 4 + 2 * 1216 * 4 and ws % 256 == 0
    assert L.dtfill_depth_read_workspace_bytes(0, 8, 8) == 0 and L.dtfill_depth_read_workspace_bytes(1, 0, 8) == 0
    assert L.dtfill_depth_read_workspace_bytes(1, 8, -1) == 0 and L.dtfill_depth_read_workspace_bytes(65536, 1, 1) == 0
    assert L.dtfill_depth_read_workspace_bytes(1 << 11, 1 << 10, 1 << 10) == 0  # 2^31 output elements

    def call(raw=256, dims=512, B=2, hmax=375, wmax=1242, H=352, W=1216, out=768, st=1024, w=4096, nws=None):
        return L.dtfill_depth_read(raw, dims, B, hmax, wmax, H, W, out, st, w, ws if nws is None else nws, None)

    for kw in (dict(raw=None), dict(out=None), dict(w=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(hmax=0), dict(wmax=-2), dict(H=0), dict(W=0), dict(B=65536, hmax=1, wmax=1, H=1, W=1),
               dict(B=2, hmax=1 << 15, wmax=1 << 15), dict(B=1 << 11, H=1 << 10, W=1 << 10)):
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3
    assert call(w=4100) == -3  # not 256-byte aligned
    assert pkg._lib.READ_NOT_16BIT == 1 and pkg._lib.READ_BAD_DIMS == 2


def test_depth_read_errors_without_gpu(pkg, tmp_path):
    with pytest.raises(AssertionError, match="file not found: "):
        pkg.depth_read(str(tmp_path / "missing.png"))
    for bad, exc in (([np.zeros((3, 4, 3), np.uint16)], ValueError), ([np.zeros((0, 4), np.uint16)], ValueError),
                     ([np.full((3, 4), 65536)], TypeError), ([np.full((3, 4), -1)], TypeError),
                     ([np.zeros((3, 4), np.float32)], TypeError), ([], ValueError)):
        with pytest.raises(exc):
            pkg.depth_read_batch(bad)


def test_import_does_not_need_pillow():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.modules['PIL'] = None; sys.path.insert(0, %r); import dtfill_amd; "
            "assert callable(dtfill_amd.depth_read)" % root)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_product_does_not_import_read_ref():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkgdir = os.path.join(root, "distancetransform-depthcompletion_amd")
    for dp, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp")):
                assert "read_ref" not in open(os.path.join(dp, f)).read(), f

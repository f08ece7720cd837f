"""rgb_read (data_read.py:66-73) and the drivers' / 255.0 without a GPU: the numpy statement in tests/rgb_ref.py against
Pillow's own NEAREST resize of uint8 images and against Pillow's stored maps (tests/golden/read_maps.npz); the bits of the
division; the ABI's argument errors; the Python layer's argument errors."""
import os

import numpy as np
import pytest

import rgb_ref as G
from read_ref import golden_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_PAIRS = {"up_7x5_to_13x11": (7, 5, 13, 11), "down_13x11_to_7x5": (13, 11, 7, 5)}


def _pairs():
    p = {name: v[0] for name, v in golden_pairs().items()}
    p.update(EXTRA_PAIRS)
    return p


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name", sorted(_pairs()))
def test_statement_equals_pillow_resize(name, C):
    Image = pytest.importorskip("PIL.Image")
    nearest = Image.Resampling.NEAREST if hasattr(Image, "Resampling") else Image.NEAREST
    h, w, H, W = _pairs()[name]
    a = G.hashed_frame(h, w, C, seed=C)
    ref = np.array(Image.fromarray(a[..., 0] if C == 1 else a).resize((W, H), nearest))
    got = G.resize(a[..., 0] if C == 1 else a, H, W)
    assert ref.dtype == np.uint8 and ref.shape == got.shape
    assert np.array_equal(ref, got)


@pytest.mark.parametrize("name", sorted(golden_pairs()))
def test_statement_equals_stored_maps(name):
    (h, w, H, W), ry, rx = golden_pairs()[name]
    a = G.hashed_frame(h, w, 3)
    u8, f32 = G.rgb_read_frame(a, H, W)
    assert np.array_equal(u8, a[ry][:, rx])
    assert np.array_equal(f32.view(np.uint32), G.UNIT[a[ry][:, rx]].view(np.uint32))
    u8c, nchw = G.rgb_read_frame(a, H, W, first_row=H // 2, normalize=False, layout="nchw")
    assert np.array_equal(u8c, a[ry[H // 2:]][:, rx])
    assert np.array_equal(nchw, a[ry[H // 2:]][:, rx].astype(np.float32).transpose(2, 0, 1))


def test_division_bits():
    v = np.arange(256)
    ref = (v.astype(np.float64) / 255.0).astype(np.float32)  # the drivers' img / 255.0, then astype(np.float32)
    assert np.array_equal((v.astype(np.float32) / np.float32(255)).view(np.uint32), ref.view(np.uint32))
    # the trap: the product with the rounded reciprocal is NOT the division
    mul = v.astype(np.float32) * (np.float32(1) / np.float32(255))
    assert mul.dtype == np.float32 and int((mul.view(np.uint32) != ref.view(np.uint32)).sum()) == 126
    # the kernel's form (dtfill_rgb.hpp, rg_unit): one Newton step on that product, in exact arithmetic rounded once per fma
    from fractions import Fraction

    def f32(x):  # the float32 nearest to the Fraction x, ties to even
        c = np.float32(float(x))
        near = (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))
        return min(near, key=lambda t: (abs(Fraction(float(t)) - x), int(t.view(np.uint32)) & 1))

    r = np.float32(1) / np.float32(255)
    for k in v:
        q = np.float32(k) * r
        res = f32(Fraction(int(k)) - Fraction(float(q)) * 255)
        got = f32(Fraction(float(res)) * Fraction(float(r)) + Fraction(float(q)))
        assert got.view(np.uint32) == ref[k].view(np.uint32), k


def test_argument_errors_without_gpu(pkg):
    L = pkg.load()
    ws = L.dtfill_rgb_read_workspace_bytes(2, 352, 1216)
    assert ws == L.dtfill_depth_read_workspace_bytes(2, 352, 1216) and ws % 256 == 0 and ws > 0
    assert L.dtfill_rgb_read_workspace_bytes(0, 8, 8) == 0 and L.dtfill_rgb_read_workspace_bytes(1, 0, 8) == 0
    assert L.dtfill_rgb_read_workspace_bytes(1, 8, -1) == 0 and L.dtfill_rgb_read_workspace_bytes(65536, 1, 1) == 0

    def call(raw=256, dims=512, B=2, hmax=375, wmax=1242, C=3, H=352, W=1216, first_row=96, normalize=1, layout=0, u8=768,
             f32=1024, st=1280, w=4096, nws=None):
        return L.dtfill_rgb_read(raw, dims, B, hmax, wmax, C, H, W, first_row, normalize, layout, u8, f32, st, w,
                                 ws if nws is None else nws, None)

    for kw in (dict(raw=None), dict(w=None), dict(u8=None, f32=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(B=0), dict(hmax=0), dict(wmax=-2), dict(H=0), dict(W=0), dict(B=65536, hmax=1, wmax=1, H=1, W=1, first_row=0),
               dict(C=0), dict(C=5), dict(first_row=-1), dict(first_row=352), dict(layout=2), dict(layout=-1),
               dict(B=2, hmax=1 << 15, wmax=1 << 14, C=4),  # 2^31 source bytes
               dict(B=2, hmax=1 << 15, wmax=1 << 15, C=1),
               dict(B=1, hmax=4, wmax=4, C=4, H=1 << 15, W=1 << 14, first_row=0, nws=1 << 40),  # 2^31 output elements
               dict(B=1, hmax=4, wmax=4, C=1, H=1 << 16, W=1 << 15, first_row=(1 << 16) - 1, nws=1 << 40)):  # 2^31 map entries
        assert call(**kw) == -2, kw
    assert call(nws=ws - 1) == -3
    assert call(w=4100) == -3  # not 256-byte aligned
    # the largest shapes just inside the limits are no shape error (too small a workspace is the next check)
    assert call(B=1, hmax=1 << 15, wmax=(1 << 14) - 1, C=4, nws=0) == -3
    assert pkg._lib.RGB_NHWC == 0 and pkg._lib.RGB_NCHW == 1


def test_rgb_read_errors_without_gpu(pkg, tmp_path):
    with pytest.raises(AssertionError, match="file not found: "):
        pkg.rgb_read(str(tmp_path / "missing.png"))
    rgb = np.zeros((3, 4, 3), np.uint8)
    for bad, exc in (([np.full((3, 4, 3), 256)], TypeError), ([np.full((3, 4, 3), -1)], TypeError),
                     ([np.zeros((3, 4, 3), np.float32)], TypeError), ([np.zeros((3, 4, 3), np.float64)], TypeError),
                     ([rgb, np.zeros((3, 4, 4), np.uint8)], ValueError), ([rgb, np.zeros((3, 4), np.uint8)], ValueError),
                     ([np.zeros((3, 4, 5), np.uint8)], ValueError), ([np.zeros((0, 4, 3), np.uint8)], ValueError),
                     ([], ValueError)):
        with pytest.raises(exc):
            pkg.rgb_read_batch(bad)
    with pytest.raises(ValueError, match="size=None"):
        pkg.rgb_read_batch([rgb, np.zeros((3, 5, 3), np.uint8)], size=None)
    with pytest.raises(ValueError, match="first_row"):
        pkg.rgb_read_batch([rgb], first_row=352)
    with pytest.raises(ValueError, match="dtype"):
        pkg.rgb_read_batch([rgb], dtype=np.float64)


def test_import_does_not_need_pillow():
    import subprocess
    import sys

    code = ("import sys; sys.modules['PIL'] = None; sys.path.insert(0, %r); import dtfill_amd; "
            "assert callable(dtfill_amd.rgb_read) and callable(dtfill_amd.rgb_read_batch) "
            "and callable(dtfill_amd.rgb_read_device)" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_product_does_not_import_rgb_ref():
    pkgdir = os.path.join(ROOT, "distancetransform-depthcompletion_amd")
    for dp, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp")):
                assert "rgb_ref" not in open(os.path.join(dp, f)).read(), f

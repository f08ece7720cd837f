"""dtfill_unproject and its backward with a `points` buffer past 2^32 bytes: a tile of three dense 352 x 1216 frames repeated to
B = 640 with N = H * W and stride 4 (4.38 GB of records, about 9 GB in all), compared on the device against the tile's
reference (tests/unproj_ref.py) with large_cases.mismatching_frames.  The memory rule is tests/test_gpu_large.py's: the test
prints what it needs beside the free memory and skips only below need + 10 %."""
import numpy as np
import pytest

import large_cases as LC
import unproj_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
GB = 1e9
T, B = 3, 640
H, W = LC.KITTI


def _need(nbytes, what):
    import torch

    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    print("\n[large] %s: needs %.2f GB, free %.2f GB of %.2f GB" % (what, nbytes / GB, free / GB, total / GB))
    if free < 1.1 * nbytes:
        pytest.skip("%s needs %.2f GB + 10 %%, %.2f GB are free" % (what, nbytes / GB, free / GB))


def test_points_past_4_gib(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    L = pkg._lib.load()
    N, stride = H * W, 4
    assert B * N * stride * 4 > 2 ** 32 and B * N * stride < 2 ** 31
    LC.assert_alias_free(T, H * W)
    px = B * H * W
    _need(px * 4 * (2 + stride + 1 + 1), "unproject, B = %d dense frames" % B)  # x, payload, points, pixel, grad_x
    rng = np.random.default_rng(12)
    x = rng.uniform(1.0, 80.0, (T, H, W)).astype(F)
    pay = LC.payload_planes(T, H, W, seed=2)
    K, E = R.exact_calibration(T)
    ref = R.forward(x, K, E, payload=pay, stride=stride)
    assert ref["counts"].tolist() == [[N, N]] * T
    xd, pd = LC.upload_tiled(x, B, DEV), LC.upload_tiled(pay, B, DEV)
    Kd, Ed = LC.upload_tiled(K, B, DEV), LC.upload_tiled(E, B, DEV)
    points = LC.poison_bits(torch.empty((B, N, stride), dtype=torch.float32, device=DEV))
    pixel = LC.poison_bits(torch.empty((B, N), dtype=torch.int32, device=DEV))
    counts = LC.poison_bits(torch.empty((B, 2), dtype=torch.int32, device=DEV))
    status = LC.poison_bits(torch.empty((B,), dtype=torch.int32, device=DEV))
    nws = L.dtfill_unproject_workspace_bytes(B, H, W)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    s = torch.cuda.current_stream().cuda_stream
    assert L.dtfill_unproject(xd.data_ptr(), pd.data_ptr(), B, H, W, 0.1, Kd.data_ptr(), Ed.data_ptr(), 0, 0, N, stride,
                              points.data_ptr(), None, pixel.data_ptr(), counts.data_ptr(), status.data_ptr(), wp, nws, s) == 0
    torch.cuda.synchronize()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert not LC.mismatching_frames(points, up(np.stack(ref["points"])), B), "points"
    assert not LC.mismatching_frames(pixel, up(np.stack(ref["pixel"])), B), "pixel"
    assert not LC.mismatching_frames(counts, up(ref["counts"]), B) and not status.any().item()
    # the backward with the records themselves as the gradient (the payload column holds any bits: it is not read without
    # grad_payload)
    gx_ref, _, st_ref = R.backward(np.stack(ref["points"]), np.stack(ref["pixel"]), ref["counts"], K, E, H, W)
    assert not st_ref.any()
    del pd
    grad_x = LC.poison_bits(torch.empty((B, H, W), dtype=torch.float32, device=DEV))
    nwb = L.dtfill_unproject_backward_workspace_bytes(B, H, W)
    assert nwb <= nws
    assert L.dtfill_unproject_backward(points.data_ptr(), pixel.data_ptr(), counts.data_ptr(), B, N, stride, H, W, Kd.data_ptr(),
                                       Ed.data_ptr(), grad_x.data_ptr(), None, status.data_ptr(), wp, nwb, s) == 0
    torch.cuda.synchronize()
    assert not LC.mismatching_frames(grad_x, up(gx_ref), B), "grad_x"
    assert not status.any().item()

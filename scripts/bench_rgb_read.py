"""Measures rgb_read on the device (dtfill_rgb_read: data_read.py:66-73 after the PNG decode, and the drivers'
img_batch[:, 96:] / 255.0) on 32 KITTI-like 375 x 1242 x 3 uint8 frames resized to 352 x 1216 and cropped at row 96, float32
NHWC and NCHW: the call's time and GB/s against the bytes it has to move at least (the sampled source rows read once, every
output element written once); the same result from eager torch ops on the device (two index_selects, the crop, the
convert-and-divide, the permute for NCHW); and the host time of rgb_read_batch (numpy frames in, numpy out).
--lib PATH loads another build of the library (make HIPFLAGS+=-DRGB_NO_STAGE: every byte pick from global memory instead of
the LDS image of the row).  Run on the GPU box."""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
if args.lib:
    pkg._lib.SO_PATH = os.path.abspath(args.lib)
dev = pkg.device
import rgb_ref
from read_ref import running_map
B, h, w, C, H, W, R0 = 32, 375, 1242, 3, 352, 1216, 96
OH = H - R0
rng = np.random.default_rng(0)
frames = [rng.integers(0, 256, (h, w, C)).astype(np.uint8) for _ in range(B)]
raw = torch.from_numpy(np.stack(frames)).cuda()
dims = torch.tensor([[h, w]] * B, dtype=torch.int32, device="cuda:0")
L = pkg._lib.load()
nws = L.dtfill_rgb_read_workspace_bytes(B, H, W)
ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
out = torch.empty((B * OH * W * C,), dtype=torch.float32, device="cuda:0")
u8 = torch.empty((B, OH, W, C), dtype=torch.uint8, device="cuda:0")
st = torch.empty(B, dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ry = torch.from_numpy(running_map(h, H)).cuda()
rx = torch.from_numpy(running_map(w, W)).cuda()
d255 = torch.full((1,), 255.0, device="cuda:0")  # a tensor divisor: torch turns a division by a Python scalar into a product


def timed(fn, n=args.iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def eager(layout):
    x = raw.index_select(1, ry).index_select(2, rx)[:, R0:]
    x = x.to(torch.float32) / d255
    return x.permute(0, 3, 1, 2).contiguous() if layout else x


# host side first, as a loader's process would call it: numpy frames in, numpy out
for dtype in (np.uint8, np.float32):
    for _ in range(3):
        a = pkg.rgb_read_batch(frames, first_row=R0, dtype=dtype)  # (two result buffers alternate once `a` is held)
    t = time.perf_counter()
    reps = 10
    for _ in range(reps):
        a = pkg.rgb_read_batch(frames, first_row=R0, dtype=dtype)
    dt = (time.perf_counter() - t) / reps
    print(json.dumps({"op": "rgb_read_batch (numpy uint8 frames -> %s [B,256,1216,3], host wall)" % np.dtype(dtype).name, "B": B,
                      "ms_per_batch": round(dt * 1e3, 3), "ms_per_frame": round(dt * 1e3 / B, 3)}))
rows = len(set(running_map(h, H)[R0:].tolist()))  # distinct source rows the cropped output samples
ref = {0: None, 1: None}
for layout, name in ((0, "NHWC"), (1, "NCHW")):
    for what, u8p in (("float32 %s" % name, None), ("float32 %s + uint8" % name, u8.data_ptr())):
        nbytes = B * rows * w * C + B * OH * W * C * (4 + (1 if u8p else 0))
        floor_us = nbytes / 8000e9 * 1e6
        ms = timed(lambda: L.dtfill_rgb_read(raw.data_ptr(), dims.data_ptr(), B, h, w, C, H, W, R0, 1, layout, u8p,
                                             out.data_ptr(), st.data_ptr(), ws.data_ptr(), nws, stream))
        print(json.dumps({"op": "dtfill_rgb_read, C ABI, preallocated buffers, %s" % what, "lib": args.lib or "default",
                          "shape": "B=%d %dx%dx%d -> %dx%d rows %d:" % (B, h, w, C, H, W, R0), "us_per_batch": round(ms * 1e3, 2),
                          "frames_per_s": round(B / ms * 1e3, 1), "achieved_GBs": round(nbytes / ms / 1e6, 1),
                          "floor_MB": round(nbytes / 1e6, 1), "floor_us_8TBs": round(floor_us, 2),
                          "x_floor": round(ms * 1e3 / floor_us, 2)}))
    shape = (B, OH, W, C) if layout == 0 else (B, C, OH, W)
    assert torch.allclose(out.view(shape), eager(layout), rtol=0, atol=1e-7), "the kernel and the eager form differ"
    bits = torch.equal(out.view(shape), eager(layout))
    ms = timed(lambda: eager(layout))
    print(json.dumps({"op": "eager torch on the device, float32 %s (index_select x2, crop, convert, divide%s)"
                      % (name, ", permute" if layout else ""), "us_per_batch": round(ms * 1e3, 2),
                      "same_bits_as_the_kernel": bits}))
ms = timed(lambda: dev.rgb_read_device(raw, dims, first_row=R0))
print(json.dumps({"op": "rgb_read_device (torch, allocates workspace and output per call)", "us_per_batch": round(ms * 1e3, 2)}))
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is not None:
    nearest = Image.Resampling.NEAREST if hasattr(Image, "Resampling") else Image.NEAREST
    t = time.perf_counter()
    for f in frames[:8]:
        r = (np.array(Image.fromarray(f).resize((W, H), nearest))[R0:] / 255.0).astype(np.float32)
    print(json.dumps({"op": "reference-style host rgb_read after the decode + [96:] / 255.0 (numpy + Pillow)",
                      "ms_per_frame": round((time.perf_counter() - t) * 1e3 / 8, 3)}))
else:
    print(json.dumps({"op": "reference-style host rgb_read", "skipped": "Pillow does not import here"}))

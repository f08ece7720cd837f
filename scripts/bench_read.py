"""Measures depth_read on the device (dtfill_depth_read: data_read.py:81-99 after the PNG decode) on 32 KITTI-like
375 x 1242 16-bit frames (5 % valid) resized to 352 x 1216: the call's time and GB/s against the bytes it has to move at
least (every source value read once for the max check, every output float written once: 84.6 MB, 10.6 us at 8 TB/s); and
the per-frame host time of depth_read_batch (numpy frames in, numpy out) against a reference-style host depth_read (numpy /
Pillow, only where Pillow imports).  Run on the GPU box."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
dev = pkg.device
B, h, w, H, W = 32, 375, 1242, 352, 1216
rng = np.random.default_rng(0)
frames = []
for b in range(B):
    f = np.zeros((h, w), np.uint16)
    u = rng.random((h, w))
    f[u < 0.05] = rng.integers(256, 65536, int((u < 0.05).sum()))
    frames.append(f)
raw = torch.from_numpy(np.stack(frames)).cuda()
dims = torch.tensor([[h, w]] * B, dtype=torch.int32, device="cuda:0")
L = pkg._lib.load()
nws = L.dtfill_depth_read_workspace_bytes(B, H, W)
ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
out = torch.empty((B, H, W), dtype=torch.float32, device="cuda:0")
st = torch.empty(B, dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
N = 200


def timed(fn, n=N):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


nbytes = B * h * w * 2 + B * H * W * 4
floor_us = nbytes / 8000e9 * 1e6
for name, dp in (("dims on the device", dims.data_ptr()), ("dims NULL", None)):
    ms = timed(lambda: L.dtfill_depth_read(raw.data_ptr(), dp, B, h, w, H, W, out.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                           nws, stream))
    print(json.dumps({"op": "dtfill_depth_read, C ABI, preallocated buffers, %s" % name,
                      "shape": "B=%d %dx%d -> %dx%d" % (B, h, w, H, W), "us_per_batch": round(ms * 1e3, 2),
                      "frames_per_s": round(B / ms * 1e3, 1), "achieved_GBs": round(nbytes / ms / 1e6, 1),
                      "floor_MB": round(nbytes / 1e6, 1), "floor_us_8TBs": round(floor_us, 2),
                      "x_floor": round(ms * 1e3 / floor_us, 2)}))
ms = timed(lambda: dev.depth_read_device(raw, dims))
print(json.dumps({"op": "depth_read_device (torch, allocates workspace and output per call)", "us_per_batch": round(ms * 1e3, 2)}))
# host side: numpy frames in, numpy [B,H,W,1] out
for _ in range(3):
    pkg.depth_read_batch(frames)
t = time.perf_counter()
reps = 10
for _ in range(reps):
    a = pkg.depth_read_batch(frames)
dt = (time.perf_counter() - t) / reps
print(json.dumps({"op": "depth_read_batch (numpy uint16 frames -> float32 [B,H,W,1], host wall)", "B": B,
                  "ms_per_batch": round(dt * 1e3, 3), "ms_per_frame": round(dt * 1e3 / B, 3)}))
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is not None:
    import read_ref
    t = time.perf_counter()
    for f in frames[:8]:
        assert f.max() > 255
        read_ref.reference_depth_read(f, (W, H))
    print(json.dumps({"op": "reference-style host depth_read after the decode (numpy + Pillow)",
                      "ms_per_frame": round((time.perf_counter() - t) * 1e3 / 8, 3)}))
else:
    print(json.dumps({"op": "reference-style host depth_read", "skipped": "Pillow does not import here"}))

"""Measures the scan-line subsampling (dtfill_line_subsample: subsample_Lidar_{train,val}.py on the device) on 32 simulated
Velodyne frames (synth.velodyne_scan): frames/s and achieved GB/s against the 8 B/pixel it has to move at least (read f32,
write f32), alone and followed by the fill; and, for context, the CPU time of the float64 numpy statement the tests
check it against, on one frame.  Run on the GPU box."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import lines_ref
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
dev = pkg.device
xh, Kh, Eh = synth.velodyne_scan(32, seed=0)
x = torch.from_numpy(xh).cuda()
K = torch.from_numpy(Kh).cuda()
E = torch.from_numpy(Eh).cuda()
B, H, W = x.shape
op = dev.DtFill(device="cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
N = 200


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(N):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N


floor_us = 8.0 * B * H * W / 8000e9 * 1e6
fill = timed(lambda: op.run(x))
for kr in (0.5, 0.25):
    ms = timed(lambda: dev.line_subsample_device(x, K, E, kr))
    both = timed(lambda: op.run(dev.line_subsample_device(x, K, E, kr)[0]))
    print(json.dumps({"op": "line_subsample (velodyne_scan B=32, %dx%d)" % (H, W), "keep_ratio": kr,
                      "us_per_batch": round(ms * 1e3, 2), "frames_per_s": round(B / ms * 1e3, 1),
                      "achieved_GBs": round(8 * B * H * W / ms / 1e6, 1), "floor_us_8B_per_px": round(floor_us, 2),
                      "roofline_frac": round(floor_us / (ms * 1e3), 3),
                      "then_fill_us": round(both * 1e3, 2), "fill_alone_us": round(fill * 1e3, 2),
                      "then_fill_frames_per_s": round(B / both * 1e3, 1),
                      "note": "host-side calibration copies, workspace and output allocation per call included"}))
# the two kernels alone: the C ABI on preallocated buffers (what a caller holding its buffers pays)
L = pkg._lib.load()
nws = L.dtfill_line_subsample_workspace_bytes(B, H, W)
ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
out = torch.empty_like(x)
st = torch.empty(B, dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
for kr in (0.5, 0.25):
    ke = int(round(1 / kr))
    ms = timed(lambda: L.dtfill_line_subsample(x.data_ptr(), B, H, W, K.data_ptr(), E.data_ptr(), 64, ke, out.data_ptr(),
                                               st.data_ptr(), ws.data_ptr(), nws, stream))
    print(json.dumps({"op": "dtfill_line_subsample, C ABI, preallocated buffers", "keep_ratio": kr,
                      "us_per_batch": round(ms * 1e3, 2), "frames_per_s": round(B / ms * 1e3, 1),
                      "achieved_GBs": round(8 * B * H * W / ms / 1e6, 1), "roofline_frac": round(floor_us / (ms * 1e3), 3),
                      "valid_px_frac": round(float((x > 0.1).float().mean()), 4)}))
t = time.perf_counter()
lines_ref.ref64(xh[:1], Kh[0], Eh[0], 64, 4)
print(json.dumps({"op": "tests/lines_ref.ref64 on one frame (numpy, CPU)", "ms": round((time.perf_counter() - t) * 1e3, 2)}))

"""Measures the LiDAR point projection on the device (dtfill_project_points) on B = 32 whole 360-degree sweeps of
synth.velodyne_points into 352 x 1216 frames: the z-buffered mode on the sweeps as they are, the reference mode on the sweeps cut
to the camera's frame (on a whole sweep the reference's assignment raises, and the call only writes zeros: timed too).  Per
call: microseconds, points per second, and GB/s against the bytes it has to move at least (the records in use read once, every
output element written once), the floor printed beside the achieved figure.  Then the time of the same result from eager torch
ops on the device (float64 bmm, round, a scatter); only timed: index_put_ with duplicate indices is not deterministic, so it is
no checker.  Every time is the median of --windows windows of --iters calls between two device events.  Run on the GPU box."""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--no-eager", action="store_true", help="the library's calls alone (for a kernel trace)")
args = ap.parse_args()
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module(pkg.__name__ + ".synth")
B, H, W, HW = args.frames, 352, 1216, 352 * 1216
clouds, K, E = synth.velodyne_points(B)


def in_frame(c, Kb, Eb):
    cam = c[:, :3].astype(np.float64) @ Eb[:3, :3].T + Eb[:3, 3]
    h = cam @ Kb.T
    u, v = np.round(h[:, 0] / h[:, 2]), np.round(h[:, 1] / h[:, 2])
    return (h[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)


def padded(cs):
    N = max(len(c) for c in cs)
    p = np.zeros((len(cs), N, 4), np.float32)
    for b, c in enumerate(cs):
        p[b, :len(c)] = c
    return torch.from_numpy(p).cuda(), torch.tensor([len(c) for c in cs], dtype=torch.int32, device="cuda:0")


cut = [c[in_frame(c, K[b], E[b])] for b, c in enumerate(clouds)]
L = pkg._lib.load()
Kd, Ed = torch.from_numpy(K).cuda(), torch.from_numpy(E).cuda()
f32 = torch.empty((B, H, W), dtype=torch.float32, device="cuda:0")
f64 = torch.empty((B, H, W), dtype=torch.float64, device="cuda:0")
st = torch.empty(B, dtype=torch.int32, device="cuda:0")
c4 = torch.empty((B, 4), dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    for _ in range(10):
        fn()
    ms = []
    for _ in range(args.windows):
        torch.cuda.synchronize(); e0.record()
        for _ in range(args.iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.iters)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def eager(pts, counts, zbuffer):
    n = pts.shape[1]
    xyz1 = torch.cat([pts[:, :, :3].double(), torch.ones((B, n, 1), dtype=torch.float64, device=pts.device)], 2)
    h = torch.bmm(Kd, torch.bmm(Ed, xyz1.transpose(1, 2))[:, :3])  # [B, 3, n]
    z = h[:, 2]
    u, v = torch.round(h[:, 0] / z), torch.round(h[:, 1] / z)
    ok = torch.arange(n, device=pts.device)[None] < counts[:, None]
    ok &= (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    flat = (torch.arange(B, device=pts.device)[:, None] * HW + v.long() * W + u.long())[ok]
    if zbuffer:
        out = torch.full((B * HW,), float("inf"), dtype=torch.float64, device=pts.device)
        out.scatter_reduce_(0, flat, z[ok], "amin")
        return torch.where(out == float("inf"), 0.0, out).float().view(B, H, W)
    out = torch.zeros((B * HW,), dtype=torch.float32, device=pts.device)
    out.index_put_((flat,), z[ok].float())  # duplicates: whichever write lands last
    return out.view(B, H, W)


for name, cs, mode, both in (("zbuffer, whole sweeps, float32 out", clouds, 1, False),
                            ("zbuffer, whole sweeps, float32 + float64 out", clouds, 1, True),
                            ("reference, sweeps cut to the frame, float32 out", cut, 0, False),
                            ("reference, sweeps cut to the frame, float32 + float64 out", cut, 0, True),
                            ("reference, whole sweeps (every frame an index error: zeros), float32 out", clouds, 0, False)):
    pts, counts = padded(cs)
    N = pts.shape[1]
    nws = L.dtfill_project_points_workspace_bytes(B, N, H, W)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device="cuda:0")
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    call = lambda: L.dtfill_project_points(pts.data_ptr(), counts.data_ptr(), B, N, 4, H, W, Kd.data_ptr(), Ed.data_ptr(), mode, 0.0,
                                           f32.data_ptr(), f64.data_ptr() if both else None, st.data_ptr(), c4.data_ptr(), wp, nws,
                                           stream)
    assert call() == 0
    torch.cuda.synchronize()
    npts = int(sum(len(c) for c in cs))
    nbytes = npts * 16 + B * HW * (12 if both else 4)
    ms, lo, hi = timed(call)
    cnt = c4.cpu().numpy()
    print(json.dumps({"op": "dtfill_project_points, C ABI, preallocated buffers: " + name, "B": B, "points": npts,
                      "pixels_written": int(cnt[:, 0].sum()), "frames_with_status": int((st.cpu().numpy() != 0).sum()),
                      "us_per_call": round(ms * 1e3, 2), "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                      "points_per_s": round(npts / ms * 1e3), "floor_MB": round(nbytes / 1e6, 2),
                      "floor_us_8TBs": round(nbytes / 8000e9 * 1e6, 2), "achieved_GBs": round(nbytes / ms / 1e6, 1),
                      "x_floor": round(ms * 1e-3 / (nbytes / 8000e9), 2)}), flush=True)
    if not args.no_eager and not both and st.cpu().numpy().sum() == 0:
        got = f32.clone()
        ref = eager(pts, counts, mode == 1)
        same = bool(torch.equal(got, ref))
        ms, lo, hi = timed(lambda: eager(pts, counts, mode == 1))
        print(json.dumps({"op": "eager torch on the device (float64 bmm x2, round, %s): %s"
                          % ("scatter_reduce amin" if mode else "index_put_", name), "us_per_call": round(ms * 1e3, 2),
                          "us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)], "same_bits_as_the_kernel_this_run": same}),
              flush=True)
if not args.no_eager:
    pts, counts = padded(clouds)
    ms, lo, hi = timed(lambda: pkg.device.project_points_device(pts, counts, Kd, Ed, (H, W)))
    print(json.dumps({"op": "project_points_device (torch, allocates workspace and outputs per call), zbuffer, whole sweeps",
                      "us_per_call": round(ms * 1e3, 2)}), flush=True)

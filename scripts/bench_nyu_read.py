"""Measures the NYU loaders' per-sample work on the device (dtfill_nyu_read: data_read.py:307-330 after the h5 read) on 64
stored samples, uint8 [3,480,640] images and float32 [480,640] depths, resized to 240 x 320 (and 256 x 320) with 64 samples a
frame: the call's time and GB/s against the bytes it has to move at least (every input byte read once, every output element
written once); the same result from eager torch ops on the device (float64 conv2d with mirror padding for each filter pass,
then a gather of the four neighbours); the stage in front of the fill (nyu_read -> DtFill.run against DtFill.run alone); the
host time of nyu_read_batch (numpy in, numpy out) and of the same work in scipy.  Run on the GPU box."""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module(pkg.__name__ + ".synth")
dev = pkg.device
B, C, h, w, N = args.batch, 3, 480, 640, 64
d8, r8 = synth.nyu_dense(8, seed=0)
depth_np = np.concatenate([d8] * (B // 8 + 1))[:B]
rgb_np = np.concatenate([r8] * (B // 8 + 1))[:B]
rgb, depth = torch.from_numpy(rgb_np).cuda(), torch.from_numpy(depth_np).cuda()
L = pkg._lib.load()
stream = torch.cuda.current_stream().cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, n=args.iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def eager_axis(x, axis, n_in, n_out, f32):
    """One filter pass of x [B, C, h, w] float64 along `axis` (2 or 3): mirror padding, a float64 conv2d."""
    wk, r = pkg.nyu_taps(n_in, n_out)
    if r == 0:
        return x
    k = torch.from_numpy(np.concatenate([wk[:0:-1], wk])).cuda()
    pad = (0, 0, r, r) if axis == 2 else (r, r, 0, 0)
    k = k.view(1, 1, -1, 1) if axis == 2 else k.view(1, 1, 1, -1)
    b, c = x.shape[:2]
    y = F.conv2d(F.pad(x.reshape(b * c, 1, *x.shape[2:]), pad, mode="reflect"), k).reshape(b, c, *x.shape[2:])
    return y.float().double() if f32 else y


def eager(x, H, W, f32):
    """x [B, C, h, w] float64 -> the resized [B, C, H, W] float64: both passes, then the four neighbours and their weights."""
    x = eager_axis(eager_axis(x, 2, h, H, f32), 3, w, W, f32)
    cr = (torch.arange(H, device="cuda", dtype=torch.float64) + 0.5) * (h / H) - 0.5
    cc = (torch.arange(W, device="cuda", dtype=torch.float64) + 0.5) * (w / W) - 0.5
    r0, c0 = cr.floor().long(), cc.floor().long()
    tr, tc = (cr - cr.floor()).view(1, 1, H, 1), (cc - cc.floor()).view(1, 1, 1, W)
    mir = lambda i, n: torch.where(i >= n, 2 * (n - 1) - i, i)
    top, bot = x.index_select(2, r0), x.index_select(2, mir(r0 + 1, h))
    c1 = mir(c0 + 1, w)
    return (top.index_select(3, c0) * (1 - tr) * (1 - tc) + top.index_select(3, c1) * (1 - tr) * tc
            + bot.index_select(3, c0) * tr * (1 - tc) + bot.index_select(3, c1) * tr * tc)


def eager_all(H, W, samples):
    img = (eager(rgb.double() * (1.0 / 255.0), H, W, False) * 255.0).float().permute(0, 2, 3, 1).contiguous()
    gt = eager(depth.double().unsqueeze(1), H, W, True).float().squeeze(1)
    mask = torch.zeros((B, H * W), dtype=torch.bool, device="cuda")
    mask.scatter_(1, (samples[..., 0].long() * W + samples[..., 1].long()), True)
    return img, gt, torch.where(mask.view(B, H, W), gt, gt * 0.0)


for H, W in ((240, 320), (256, 320)):
    rs = np.random.RandomState(0)
    smp_np = np.stack([np.stack([rs.randint(H - 12, size=N) + 6, rs.randint(W - 16, size=N) + 8], 1) for _ in range(B)])
    samples = torch.from_numpy(smp_np.astype(np.int32)).cuda()
    (wy, ry), (wx, rx) = pkg.nyu_taps(h, H), pkg.nyu_taps(w, W)
    tap = lambda t: None if t is None else t.ctypes.data
    nws = L.dtfill_nyu_read_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, H, W, C), dtype=torch.float32, device="cuda")
    gt, lidar = (torch.empty((B, H, W), dtype=torch.float32, device="cuda") for _ in range(2))
    st = torch.empty(B, dtype=torch.int32, device="cuda")
    shape = "B=%d %dx%d -> %dx%d, %d samples a frame" % (B, h, w, H, W, N)
    for what, rp, dp, nbytes in (("image + depth", rgb.data_ptr(), depth.data_ptr(), B * (h * w * (C + 4) + H * W * 4 * (C + 2) + N * 8)),
                                 ("image alone", rgb.data_ptr(), None, B * (h * w * C + H * W * 4 * C)),
                                 ("depth alone", None, depth.data_ptr(), B * (h * w * 4 + H * W * 8 + N * 8))):
        call = lambda: L.dtfill_nyu_read(rp, dp, B, C, h, w, H, W, tap(wy), ry, tap(wx), rx, samples.data_ptr(), N, 0, 0,
                                         out.data_ptr() if rp else None, gt.data_ptr() if dp else None,
                                         lidar.data_ptr() if dp else None, st.data_ptr(), ws.data_ptr(), nws, stream)
        assert call() == 0
        ms = timed(call)
        floor_us = nbytes / 8000e9 * 1e6
        print(json.dumps({"op": "dtfill_nyu_read, C ABI, preallocated buffers, " + what, "shape": shape,
                          "us_per_batch": round(ms * 1e3, 2), "frames_per_s": round(B / ms * 1e3, 1),
                          "achieved_GBs": round(nbytes / ms / 1e6, 1), "floor_MB": round(nbytes / 1e6, 1),
                          "floor_us_8TBs": round(floor_us, 2), "x_floor": round(ms * 1e3 / floor_us, 2)}))
    L.dtfill_nyu_read(rgb.data_ptr(), depth.data_ptr(), B, C, h, w, H, W, tap(wy), ry, tap(wx), rx, samples.data_ptr(), N, 0, 0,
                      out.data_ptr(), gt.data_ptr(), lidar.data_ptr(), st.data_ptr(), ws.data_ptr(), nws, stream)
    try:
        ei, eg, el = eager_all(H, W, samples)
        ms = timed(lambda: eager_all(H, W, samples), max(5, args.iters // 10))
        print(json.dumps({"op": "eager torch on the device (float64 conv2d, mirror padding, gather), image + depth", "shape": shape,
                          "us_per_batch": round(ms * 1e3, 2), "max_abs_diff_image": float((ei - out).abs().max()),
                          "max_abs_diff_gt": float((eg - gt).abs().max()), "same_bits_image": torch.equal(ei, out),
                          "same_bits_gt": torch.equal(eg, gt), "same_bits_lidar": torch.equal(el, lidar)}))
    except Exception as e:  # (a float64 convolution the installed libraries do not have: the other rows still count)
        print(json.dumps({"op": "eager torch on the device", "shape": shape, "skipped": str(e).splitlines()[0][:200]}))
    ms = timed(lambda: dev.nyu_read_device(rgb, depth, samples, (H, W)))
    print(json.dumps({"op": "nyu_read_device (torch, allocates workspace and outputs per call)", "shape": shape,
                      "us_per_batch": round(ms * 1e3, 2)}))
    # the stage in front of the fill: eval_NYU.py's Distance_Transform thresholds
    op = dev.DtFill(device="cuda:0")
    _, _, lid, _ = dev.nyu_read_device(None, depth, samples, (H, W))
    fill_ms = timed(lambda: op.run(lid, 0.001, 0.1))
    both_ms = timed(lambda: op.run(dev.nyu_read_device(None, depth, samples, (H, W))[2], 0.001, 0.1))
    print(json.dumps({"op": "in front of the fill: nyu_read_device(depth) -> DtFill.run", "shape": shape,
                      "fill_alone_us": round(fill_ms * 1e3, 2), "read_then_fill_us": round(both_ms * 1e3, 2)}))
    for _ in range(2):
        a = pkg.nyu_read_batch(rgb_np, depth_np, N, (H, W))
    t = time.perf_counter()
    reps = 5
    for _ in range(reps):
        a = pkg.nyu_read_batch(rgb_np, depth_np, N, (H, W))
    dt = (time.perf_counter() - t) / reps
    print(json.dumps({"op": "nyu_read_batch (numpy in, numpy out, host wall)", "shape": shape, "ms_per_batch": round(dt * 1e3, 3),
                      "ms_per_frame": round(dt * 1e3 / B, 3)}))
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    if ndi is not None:
        sig = [(h / H - 1) / 2, (w / W - 1) / 2]
        t = time.perf_counter()
        for b in range(2):
            v = np.transpose(rgb_np[b], (1, 2, 0)) * (1.0 / 255.0)
            g = ndi.gaussian_filter(v, sig + [0], mode="mirror")
            img = ndi.zoom(g, [H / h, W / w, 1], order=1, mode="mirror", grid_mode=True) * 255
            g = ndi.gaussian_filter(depth_np[b], sig, mode="mirror")
            z = ndi.zoom(g, [H / h, W / w], order=1, mode="mirror", grid_mode=True)
        print(json.dumps({"op": "the same resizes on the host in scipy.ndimage (what skimage's resize calls)", "shape": shape,
                          "ms_per_frame": round((time.perf_counter() - t) * 1e3 / 2, 3)}))

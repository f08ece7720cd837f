"""Measures the max-pool pyramid of ResNet18_NO_BN_l2_light_image (dtfill_max_pool_pyramid and dtfill_max_pool_pyramid_backward:
one 64-channel tensor pooled by 2, 4 and 8) in both directions, and the inference and the training step of ResNet18LightImage /
ResNet18LightImageTrainable beside ResNet18Image's, float32, on the same tensors, on the same device, in the same run.
Shapes: the reference's KITTI frames 256 x 1216 (the training crop) and 352 x 1216 (the full frame), B = 1 and 4, 64 channels.

What each direction is held against.
- Its BYTE FLOOR: forward, one read of x and 21/64 of it written; backward, one read of x and of the three dys (21/64 of x) and one
  write of dx.  floor_us = read bytes / read rate + written bytes / store rate, the rates measured here on tensors of those very
  sizes by scripts/hbm_rates.py's method (torch sum for the read rate, fill_ for the store rate); over_floor = ours / floor.
  GBps is all those bytes over our time.
- THREE SINGLE-LEVEL CALLS of the same entry point, which read x three times (the backward: and two torch adds of the three dx
  tensors, which is what three separate pools cost under a tape).
- Eager torch on channels-last tensors: three F.max_pool2d forward; three aten.max_pool2d_with_indices_backward and two adds
  backward, with the indices a forward stored (this library stores none and finds the winners again from x).

The method is scripts/bench_resnet_image.py's: microseconds per call from HIP events over five rounds, the candidates alternating
within a round, the median and the (min .. max) spread.  One JSON line per row.  --ops-only and --nets-only run one half."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as Fn
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
net = importlib.import_module(pkg.__name__ + ".net")
synth = importlib.import_module(pkg.__name__ + ".synth")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
pkg._lib.load()
dev, autograd = pkg.device, pkg.autograd
OPS, NETS = "--nets-only" not in sys.argv, "--ops-only" not in sys.argv
ROUNDS, WINDOW_US = 5, 30e3
FRAMES, BATCHES, SCALE_NUM, C, LEVELS = ((256, 1216), (352, 1216)), (1, 4), 4, 64, (2, 4, 8)
aten = torch.ops.aten


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def compare(fs):
    """Median and spread of ROUNDS alternating rounds of each of fs, in microseconds per call."""
    counts = []
    for f in fs:
        for _ in range(3):
            f()
        counts.append(max(3, int(WINDOW_US / max(timed(f, 3), 1.0))))
    rounds = [[] for _ in fs]
    for _ in range(ROUNDS):
        for k, f in enumerate(fs):
            rounds[k].append(timed(f, counts[k]))
    return [{"us": round(statistics.median(r), 2), "min": round(min(r), 2), "max": round(max(r), 2)} for r in rounds]


def rates(read_bytes, write_bytes):
    """(read GB/s, store GB/s) on tensors of these sizes: scripts/hbm_rates.py's sum and fill_."""
    r, w = torch.empty(read_bytes // 4, device="cuda"), torch.empty(write_bytes // 4, device="cuda")
    t = compare([lambda: r.sum(), lambda: w.fill_(1.0)])
    return read_bytes / t[0]["us"] / 1e3, write_bytes / t[1]["us"] / 1e3


def op_rows(B, H, W):
    gen = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn((B, H, W, C), device="cuda", generator=gen)
    outs = [torch.empty((B, H // k, W // k, C), device="cuda") for k in LEVELS]
    dys = [torch.randn((B, H // k, W // k, C), device="cuda", generator=gen) for k in LEVELS]
    nchw = lambda t: t.permute(0, 3, 1, 2)  # the same memory as a channels-last tensor
    xbytes = 4 * B * H * W * C
    small = xbytes * 21 // 64
    row = {"input": [B, H, W, C], "levels": list(LEVELS)}
    # ---- forward: read x, write 21/64 of it ----
    rate_r, rate_w = rates(xbytes, small)
    fused = lambda: dev.max_pool_pyramid_device(x, LEVELS, outs=outs)
    three = lambda: [dev.max_pool_pyramid_device(x, (k,), outs=[o]) for k, o in zip(LEVELS, outs)]
    eager = lambda: [Fn.max_pool2d(nchw(x), k) for k in LEVELS]
    t = compare([fused, three, eager])
    floor = xbytes / rate_r / 1e3 + small / rate_w / 1e3
    same = all(torch.equal(nchw(a), b) for a, b in zip(fused(), eager()))
    print(json.dumps(dict(op="forward", **row, fused=t[0], three_calls=t[1], eager=t[2], read_bytes=xbytes, written_bytes=small,
                          GBps=round((xbytes + small) / t[0]["us"] / 1e3, 1), read_rate_GBps=round(rate_r, 1), store_rate_GBps=round(rate_w, 1),
                          floor_us=round(floor, 2), over_floor=round(t[0]["us"] / floor, 2), three_over_fused=round(t[1]["us"] / t[0]["us"], 2),
                          eager_over_fused=round(t[2]["us"] / t[0]["us"], 2), equals_eager=same)), flush=True)
    # ---- backward: read x and the dys, write dx ----
    rate_r, rate_w = rates(xbytes + small, xbytes)
    fused = lambda: dev.max_pool_pyramid_backward_device(x, dys)
    def three():
        d = [dev.max_pool_pyramid_backward_device(x, [dy], (k,)) for k, dy in zip(LEVELS, dys)]
        return (d[0] + d[1]) + d[2]
    indices = [aten.max_pool2d_with_indices(nchw(x), [k, k], [k, k])[1] for k in LEVELS]
    def eager():
        d = [aten.max_pool2d_with_indices_backward(nchw(dy), nchw(x), [k, k], [k, k], [0, 0], [1, 1], False, i) for k, dy, i in zip(LEVELS, dys, indices)]
        return (d[0] + d[1]) + d[2]
    t = compare([fused, three, eager])
    floor = (xbytes + small) / rate_r / 1e3 + xbytes / rate_w / 1e3
    diff = (nchw(fused()) - eager()).abs().max().item()  # (random values: no ties, the same winners)
    print(json.dumps(dict(op="backward", **row, fused=t[0], three_calls=t[1], eager=t[2], read_bytes=xbytes + small, written_bytes=xbytes,
                          GBps=round((2 * xbytes + small) / t[0]["us"] / 1e3, 1), read_rate_GBps=round(rate_r, 1), store_rate_GBps=round(rate_w, 1),
                          floor_us=round(floor, 2), over_floor=round(t[0]["us"] / floor, 2), three_over_fused=round(t[1]["us"] / t[0]["us"], 2),
                          eager_over_fused=round(t[2]["us"] / t[0]["us"], 2), max_abs_diff=diff)), flush=True)


def training_step(model, opt, inputs, gt):
    def step():
        output, correction = model(*inputs)
        main, aux = autograd.train_loss(output, gt, inputs[0], correction)
        (main + aux).backward()
        opt.step()
        opt.zero_grad()
    return step


def net_rows(B, H, W):
    lidar = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
    gt = torch.from_numpy(synth.kitti_iid(B, p=0.3, seed=100 + B, hw=(H, W))).cuda()
    rgb = torch.rand((B, H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
    wl = net.glorot_weights_resnet18_light_image(0, SCALE_NUM, True, bias=0.1)
    wi = net.glorot_weights_resnet18_image(0, SCALE_NUM, True, bias=0.1)
    light, image = net.ResNet18LightImage(wl), net.ResNet18Image(wi)
    t = dict(zip(("light", "image"), compare([lambda: light(lidar, rgb), lambda: image(lidar, rgb)])))
    print(json.dumps({"op": "inference", "net": "ResNet18_NO_BN_l2_light_image", "scale_num": SCALE_NUM, "shape": [B, H, W], **t,
                      "image_over_light": round(t["image"]["us"] / t["light"]["us"], 2)}), flush=True)
    del light, image
    torch.cuda.empty_cache()
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=1e-6, capturable=True)
    models = [net.ResNet18LightImageTrainable(wl, scale_num=SCALE_NUM).cuda(), net.ResNet18ImageTrainable(wi, scale_num=SCALE_NUM).cuda()]
    t = dict(zip(("light", "image"), compare([training_step(m, adam(m), (lidar, rgb), gt) for m in models])))
    print(json.dumps({"op": "training_step", "net": "ResNet18_NO_BN_l2_light_image", "joint_train": False, "scale_num": SCALE_NUM,
                      "shape": [B, H, W], **t, "image_over_light": round(t["image"]["us"] / t["light"]["us"], 2)}), flush=True)


for H, W in FRAMES:
    for B in BATCHES:
        if OPS:
            op_rows(B, H, W)
            torch.cuda.empty_cache()
        if NETS:
            net_rows(B, H, W)
            torch.cuda.empty_cache()

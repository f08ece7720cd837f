"""Measures the image path of ResNet18_NO_BN_l2_image: img_conv (dtfill_conv2d_image, 3x3x3 -> 64, leaky) and its weight
gradient (dtfill_conv2d_image_backward_weights) alone, and the whole inference and training step of ResNet18Image /
ResNet18ImageTrainable, float32, on the same tensors, on the same device, in the same run.
Shapes: the reference's KITTI frames 256 x 1216 (the training crop) and 352 x 1216 (the full frame), B = 1 and 4.

What each is held against.
- The layer, against its BYTE FLOOR: the bytes it must move (forward: read x, write y; weight gradient: read x, dy and y; the
  partials and the weights are kilobytes) at the rates this device reaches on tensors of those very sizes, measured here by
  scripts/hbm_rates.py's method (torch fill_ for the store rate, sum for the read rate).  floor_us = read bytes / read rate +
  written bytes / store rate; over_floor = ours / floor.  GBps is all those bytes over our time.
- The layer, against eager torch: F.conv2d + leaky_relu, and aten.convolution_backward behind aten.leaky_relu_backward,
  channels-last.
- The networks, against eager torch (the same graph in F.conv2d / F.conv_transpose2d; the fill and the loss stay this library's
  operators) and against ResNet18 / ResNet18Trainable on the same LiDAR frames: what the image path adds is the stem, the doubled
  Cin of conv1a and conv1a_extra and the 192-wide upsample_1_post.

The method is scripts/bench_resnet_backward.py's: microseconds per call from HIP events over five rounds, the candidates
alternating within a round, the median and the (min .. max) spread.  One JSON line per row.  --no-eager leaves the eager side
out; --layers-only and --nets-only run one half."""
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
EAGER = "--no-eager" not in sys.argv
LAYERS, NETS = "--nets-only" not in sys.argv, "--layers-only" not in sys.argv
ROUNDS, WINDOW_US = 5, 30e3
FRAMES, BATCHES, SCALE_NUM, ALPHA = ((256, 1216), (352, 1216)), (1, 4), 4, net.LEAKY_ALPHA
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


def layer_rows(B, H, W):
    gen = torch.Generator(device="cuda").manual_seed(B)
    rand = lambda *shape: torch.randn(shape, device="cuda", generator=gen)
    x, dy, y = torch.rand((B, H, W, 3), device="cuda", generator=gen), rand(B, H, W, 64), rand(B, H, W, 64)
    kernel, bias = rand(3, 3, 3, 64) / 27 ** 0.5, rand(64) / 10
    out = torch.empty((B, H, W, 64), device="cuda")
    nchw = lambda t: t.permute(0, 3, 1, 2)  # the same memory as a channels-last tensor
    ekernel = kernel.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)
    row = {"layer": "img_conv", "ksize": 3, "Cin": 3, "Cout": 64, "input": [B, H, W]}
    pixels = B * H * W
    # ---- forward: read x, write y ----
    rd, wr = 4 * pixels * 3, 4 * pixels * 64
    rate_r, rate_w = rates(rd, wr)
    ours = lambda: dev.conv2d_image_device(x, kernel, bias, "leaky", ALPHA, out)
    eager = lambda: Fn.leaky_relu(Fn.conv2d(nchw(x), ekernel, bias, padding=1), ALPHA)
    t = compare([ours] + ([eager] if EAGER else []))
    floor = rd / rate_r / 1e3 + wr / rate_w / 1e3
    res = dict(op="forward", **row, ours=t[0], read_bytes=rd, written_bytes=wr, GBps=round((rd + wr) / t[0]["us"] / 1e3, 1),
               read_rate_GBps=round(rate_r, 1), store_rate_GBps=round(rate_w, 1), floor_us=round(floor, 2), over_floor=round(t[0]["us"] / floor, 2),
               MFMAs=pixels // 16 * 4 * 7, TFLOPs=round(2.0 * 27 * 64 * pixels / t[0]["us"] / 1e6, 2))
    if EAGER:
        res.update(eager=t[1], eager_over_ours=round(t[1]["us"] / t[0]["us"], 2), max_abs_diff=(nchw(ours()) - eager()).abs().max().item())
    print(json.dumps(res), flush=True)
    # ---- the weight gradient: read x, dy and y ----
    rd = 4 * pixels * (3 + 64 + 64)
    rate_r, _ = rates(rd, 1 << 20)
    ours = lambda: dev.conv2d_image_backward_weights_device(x, dy, 3, y, "leaky", ALPHA)
    eager = lambda: aten.convolution_backward(aten.leaky_relu_backward(nchw(dy), nchw(y), ALPHA, True), nchw(x), ekernel, [64], [1, 1], [1, 1],
                                              [1, 1], False, [0, 0], 1, [False, True, True])[1:]
    t = compare([ours] + ([eager] if EAGER else []))
    floor = rd / rate_r / 1e3
    res = dict(op="backward_weights", **row, ours=t[0], read_bytes=rd, GBps=round(rd / t[0]["us"] / 1e3, 1), read_rate_GBps=round(rate_r, 1),
               floor_us=round(floor, 2), over_floor=round(t[0]["us"] / floor, 2),
               workspace_bytes=dev.conv2d_image_backward_workspace_bytes(B, H, W, 3, 3, 64))
    if EAGER:
        mine, theirs = ours(), eager()
        res.update(eager=t[1], eager_over_ours=round(t[1]["us"] / t[0]["us"], 2),
                   max_abs_diff=max((mine[0] - theirs[0].permute(2, 3, 1, 0)).abs().max().item(), (mine[1] - theirs[1]).abs().max().item()))
    print(json.dumps(res), flush=True)


class EagerNet(torch.nn.Module):
    """ResNet18Trainable's / ResNet18ImageTrainable's forward (image: with img_conv in front of the stems) with F.conv2d and
    F.conv_transpose2d; the fill and the loss stay this library's operators."""

    def __init__(self, weights, image):
        super().__init__()
        self.image = image
        for n, (k, b) in weights.items():
            if n != "lidar_conv_extra_3":
                kernel = torch.from_numpy(k).permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)  # OIHW; transposed: [Cin,Cout,3,3]
                self.register_parameter(n + "_kernel", torch.nn.Parameter(kernel))
                self.register_parameter(n + "_bias", torch.nn.Parameter(torch.from_numpy(b.copy())))
        self.register_buffer("threshold", torch.tensor(0.1))
        self.register_buffer("scale", torch.tensor(90.0))

    def layer(self, x, name, act="leaky", stride=1, residual=None):
        kernel, bias = getattr(self, name + "_kernel"), getattr(self, name + "_bias")
        if name in net.RESNET_TRANSPOSED:
            y = Fn.conv_transpose2d(x, kernel, bias, stride=2)[:, :, :2 * x.shape[2], :2 * x.shape[3]]  # the 'same' crop
        elif stride == 2 and kernel.shape[2] == 3:
            y = Fn.conv2d(Fn.pad(x, (0, 1, 0, 1)), kernel, bias, stride=2)
        else:
            y = Fn.conv2d(x, kernel, bias, stride=stride, padding=kernel.shape[2] // 2)
        if residual is not None:
            y = y + residual
        return Fn.leaky_relu(y, ALPHA) if act == "leaky" else y

    def forward(self, x, rgb=None):
        mask = torch.gt(x, self.threshold).float()
        t = (x / self.scale)[:, None]
        for name in ("correct_1", "correct_2", "correct_3"):
            t = self.layer(t, name)
        correct = self.layer(t, "correct_4", "linear")[:, 0].contiguous() * mask
        lidars = autograd.generate_multi_channel(correct.detach(), mask, 7, SCALE_NUM)
        stems = [self.layer(rgb.permute(0, 3, 1, 2), "img_conv")] if self.image else []
        stems = torch.cat(stems + [self.layer(l[:, None], n) for l, n in zip(lidars, net.stem_layers(SCALE_NUM))], dim=1)
        below, totals = stems, []
        for level in (1, 2, 3, 4):
            name, stride = "conv%d" % level, 1 if level == 1 else 2
            t = self.layer(below, name + "a", stride=stride)
            add = self.layer(below, name + "a_extra", "linear", stride)
            total = self.layer(t, name + "b", residual=add)
            below = self.layer(self.layer(total, name + "c"), name + "d", residual=total if level < 4 else None)
            totals.append(below)
        for level in (4, 3, 2):
            below = self.layer(torch.cat([self.layer(below, "upsample_%d" % level), totals[level - 2]], dim=1), "upsample_%d_post" % level)
        t = self.layer(torch.cat([self.layer(below, "upsample_1"), stems], dim=1), "upsample_1_post")
        return (self.layer(t, "conv_output", "linear")[:, 0] * self.scale).contiguous(), correct * self.scale


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
    wi = net.glorot_weights_resnet18_image(0, SCALE_NUM, True, bias=0.1)
    wp = net.glorot_weights_resnet18(0, SCALE_NUM, True, bias=0.1)
    names = ["image", "plain"] + (["eager_image", "eager_plain"] if EAGER else [])
    # ---- inference ----
    image, plain = net.ResNet18Image(wi), net.ResNet18(wp)
    fs = [lambda: image(lidar, rgb), lambda: plain(lidar)]
    if EAGER:
        ei, ep = EagerNet(wi, True).cuda(), EagerNet(wp, False).cuda()
        def no_grad(m, *a):
            def f():
                with torch.no_grad():
                    return m(*a)
            return f
        fs += [no_grad(ei, lidar, rgb), no_grad(ep, lidar)]
    t = dict(zip(names, compare(fs)))
    res = {"op": "inference", "net": "ResNet18_NO_BN_l2_image", "scale_num": SCALE_NUM, "shape": [B, H, W], **t,
           "image_over_plain": round(t["image"]["us"] / t["plain"]["us"], 3), "image_minus_plain_us": round(t["image"]["us"] - t["plain"]["us"], 1)}
    if EAGER:
        res["eager_over_ours"] = round(t["eager_image"]["us"] / t["image"]["us"], 2)
        res["max_abs_diff"] = (fs[0]()[0] - fs[2]()[0]).abs().max().item()
    print(json.dumps(res), flush=True)
    del image, plain, fs
    torch.cuda.empty_cache()
    # ---- the whole step of train.py:232-254 ----
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=1e-6, capturable=True)
    models = [net.ResNet18ImageTrainable(wi, scale_num=SCALE_NUM).cuda(), net.ResNet18Trainable(wp, scale_num=SCALE_NUM).cuda()]
    inputs = [(lidar, rgb), (lidar,)]
    if EAGER:
        models += [ei, ep]
        inputs += [(lidar, rgb), (lidar,)]
    t = dict(zip(names, compare([training_step(m, adam(m), i, gt) for m, i in zip(models, inputs)])))
    res = {"op": "training_step", "net": "ResNet18_NO_BN_l2_image", "joint_train": False, "scale_num": SCALE_NUM, "shape": [B, H, W], **t,
           "image_over_plain": round(t["image"]["us"] / t["plain"]["us"], 3), "image_minus_plain_us": round(t["image"]["us"] - t["plain"]["us"], 1)}
    if EAGER:
        res["eager_over_ours"] = round(t["eager_image"]["us"] / t["image"]["us"], 2)
    print(json.dumps(res), flush=True)


for H, W in FRAMES:
    for B in BATCHES:
        if LAYERS:
            layer_rows(B, H, W)
            torch.cuda.empty_cache()
        if NETS:
            net_rows(B, H, W)
            torch.cuda.empty_cache()

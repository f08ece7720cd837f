"""Measures the backward pass of ResNet18_NO_BN_l2's wide layers (dtfill_conv2d_strided_backward_data / _weights,
dtfill_conv2d_transpose_backward_data / _weights) for every distinct layer shape of net.layer_shapes_resnet18, and one whole
training step of ResNet18Trainable (forward, autograd.train_loss, backward, Adam), against the same layers' and the same net's
backward in eager torch (aten.convolution_backward behind aten.leaky_relu_backward; F.conv2d / F.conv_transpose2d under the
tape), float32, channels-last, on the same tensors, on the same device, in the same run.
Shape: the reference's cropped KITTI frame 256 x 1216 at B = 1 and B = 4, scale_num 4, if_correct; level k lives at 1 / 2^(k-1).

The method is scripts/bench_conv_backward.py's: microseconds per call from HIP events over five rounds, ours and eager
alternating within a round, the median and the (min .. max) spread, the TFLOP/s of our call as a share of the 157.3 TF FP32
peak (2 taps Cin Cout FLOP per output pixel for dx and again for dw; a transposed layer has 9 taps per INPUT pixel), the
workspace bytes, and the largest absolute difference between the two results (the eager side sums in another order).  One JSON
line per row.  --no-eager leaves the eager side out; --layers-only and --step-only run one half."""
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
LAYERS, STEP = "--step-only" not in sys.argv, "--layers-only" not in sys.argv
ROUNDS, WINDOW_US, PEAK_TF = 5, 30e3, 157.3
H, W, SCALE_NUM, ALPHA = 256, 1216, 4, net.LEAKY_ALPHA
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


def report(res, flop, ours, eager, diff):
    t = compare([ours] + ([eager] if EAGER else []))
    res["ours"] = t[0]
    res["TFLOPs"] = round(flop / t[0]["us"] / 1e6, 2)
    res["share_of_fp32_peak"] = round(flop / t[0]["us"] / 1e6 / PEAK_TF, 3)
    if EAGER:
        res["eager"] = t[1]
        res["eager_over_ours"] = round(t[1]["us"] / t[0]["us"], 2)
        res["max_abs_diff"] = diff()
    print(json.dumps(res), flush=True)


def nchw(t):
    """[B,H,W,C] contiguous -> the same memory as a channels-last [B,C,H,W] tensor."""
    return t.permute(0, 3, 1, 2)


def eager_backward(x, dy, y, kernel, stride, pads, transposed, mask):
    """aten's backward of the convolution + leaky_relu: mask = (dx, dw, db) wanted.  A stride-2 'same' layer pads behind only:
    the eager side convolves an input padded by one row and one column (a view of a larger tensor made once, outside the timing)."""
    g = aten.leaky_relu_backward(dy, y, ALPHA, True)
    cout = kernel.shape[1] if transposed else kernel.shape[0]
    return aten.convolution_backward(g, x, kernel, [cout], [stride, stride], pads, [1, 1], transposed, [1, 1] if transposed else [0, 0], 1, mask)


def geometry(name):
    """(level of the layer's input frame, stride, transposed) of a wide layer: level k lives at 1 / 2^(k-1) of the frame."""
    transposed, stride = name in net.RESNET_TRANSPOSED, 2 if name in net.RESNET_STRIDE2 else 1
    if name.startswith("conv") and name[4].isdigit():
        return int(name[4]) - (stride == 2), stride, False  # conv<k>a and conv<k>a_extra read level k - 1
    if name.startswith("upsample"):
        k = int(name.split("_")[1])
        return (k if transposed else max(k - 1, 1)), 1 if not transposed else 2, transposed  # upsample_<k>_post runs on level k - 1
    return 1, 1, False


def chain_pixels(name):
    """The pixels a layer's taps are counted on: its output's, a transposed layer's input's."""
    level, stride, transposed = geometry(name)
    return (H >> (level - 1)) * (W >> (level - 1)) // (1 if transposed else stride * stride)


def distinct_layers():
    """(level, ksize, Cin, Cout, stride, transposed, a layer's name) of every distinct wide layer shape, at its level's frame."""
    seen, out = set(), []
    for name, (k, cin, cout) in net.layer_shapes_resnet18(SCALE_NUM, True).items():
        if name in net._head_shapes(SCALE_NUM, True) or cout == 1:  # the head and conv_output are dtfill_conv2d's layers
            continue
        key = (geometry(name)[0], k, cin, cout) + geometry(name)[1:]
        if key not in seen:
            seen.add(key)
            out.append(key + (name,))
    return out


class EagerNet(torch.nn.Module):
    """ResNet18Trainable's forward with F.conv2d and F.conv_transpose2d; the fill and the loss stay this library's operators."""

    def __init__(self, weights):
        super().__init__()
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

    def forward(self, x):
        mask = torch.gt(x, self.threshold).float()
        t = (x / self.scale)[:, None]
        for name in ("correct_1", "correct_2", "correct_3"):
            t = self.layer(t, name)
        correct = self.layer(t, "correct_4", "linear")[:, 0].contiguous() * mask
        lidars = autograd.generate_multi_channel(correct.detach(), mask, 7, SCALE_NUM)
        stems = torch.cat([self.layer(l[:, None], n) for l, n in zip(lidars, net.stem_layers(SCALE_NUM))], dim=1)
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


def training_step(model, opt, lidar, gt):
    def step():
        output, correction = model(lidar)
        main, aux = autograd.train_loss(output, gt, lidar, correction)
        (main + aux).backward()
        opt.step()
        opt.zero_grad()
    return step


for B in (1, 4):
    gen = torch.Generator(device="cuda").manual_seed(B)
    rand = lambda *shape: torch.randn(shape, device="cuda", generator=gen)
    for level, k, cin, cout, stride, transposed, name in (distinct_layers() if LAYERS else ()):
        h, w = H >> (level - 1), W >> (level - 1)  # the layer's input frame
        ho, wo = (2 * h, 2 * w) if transposed else (h // stride, w // stride)
        x, dy, y = rand(B, h, w, cin), rand(B, ho, wo, cout), rand(B, ho, wo, cout)
        kernel = rand(k, k, cin, cout) / (k * cin ** 0.5)  # ours: [k,k,Cin,Cout], the packed layout of a transposed layer too
        row = {"layer": name, "ksize": k, "Cin": cin, "Cout": cout, "stride": stride, "transposed": transposed, "input": [B, h, w],
               "workspace_bytes": dev.conv2d_wide_backward_workspace_bytes(B, h, w, cin, k, cout, stride, transposed)}
        flop = 2.0 * k * k * cin * cout * B * (h * w if transposed else ho * wo)
        edy, ey = nchw(dy), nchw(y)
        if transposed:
            # aten's padding = 1, output_padding = 1 form puts tap k of input h at 2 h + k - 1, the 'same' rule at 2 h + k: on
            # frames and taps mirrored in both axes the two are one function, so the eager side gets mirrored copies (made once,
            # outside the timing) and the difference is taken on its results mirrored back
            mirror = lambda t: t.flip(1, 2).contiguous()
            ekernel = kernel.flip(0, 1).permute(2, 3, 0, 1).contiguous(memory_format=torch.channels_last)  # [Cin,Cout,3,3]
            ex, edy, ey, pads = nchw(mirror(x)), nchw(mirror(dy)), nchw(mirror(y)), [1, 1]
        else:
            ekernel = kernel.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)  # OIHW
            if stride == 2 and k == 3:  # 'same' pads one row below and one column to the right
                ex, pads = nchw(Fn.pad(x, (0, 0, 0, 1, 0, 1))), [0, 0]
            else:
                ex, pads = nchw(x), [k // 2, k // 2]
        crop = (lambda t: t[:, :, :h, :w]) if ex.shape[2] != h else (lambda t: t.flip(2, 3)) if transposed else (lambda t: t)
        dx = torch.empty((B, h, w, cin), device="cuda")
        if transposed:
            ours = lambda: dev.conv2d_transpose_backward_data_device(dy, kernel, y, "leaky", ALPHA, dx=dx)
        else:
            ours = lambda: dev.conv2d_strided_backward_data_device(dy, kernel, stride, y, "leaky", ALPHA, dx=dx)
        eager = lambda: eager_backward(ex, edy, ey, ekernel, stride, pads, transposed, [True, False, False])[0]
        report(dict(op="backward_data", **row), flop, ours, eager, lambda: (nchw(ours()) - crop(eager())).abs().max().item())
        if transposed:
            ours = lambda: dev.conv2d_transpose_backward_weights_device(x, dy, y, "leaky", ALPHA)
            back = lambda t: t.permute(2, 3, 0, 1).flip(0, 1)
        else:
            ours = lambda: dev.conv2d_strided_backward_weights_device(x, dy, k, stride, y, "leaky", ALPHA)
            back = lambda t: t.permute(2, 3, 1, 0)
        eager = lambda: eager_backward(ex, edy, ey, ekernel, stride, pads, transposed, [False, True, True])[1:]
        diff = lambda: max((a - b).abs().max().item() for a, b in zip(ours(), (back(eager()[0]), eager()[1])))
        report(dict(op="backward_weights", **row), flop, ours, eager, diff)
        del x, dy, y, dx, ex, edy, ey, kernel, ekernel
        torch.cuda.empty_cache()
    if not STEP:
        continue
    # ---- the whole step of train.py:232-254 on the paper's network ----
    weights = net.glorot_weights_resnet18(0, SCALE_NUM, True, bias=0.1)
    lidar = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
    gt = torch.from_numpy(synth.kitti_iid(B, p=0.3, seed=100 + B, hw=(H, W))).cuda()
    # per frame: forward, dx and dw of every layer (an upper count: the first layers need no dx)
    flop = sum(3 * 2.0 * k * k * cin * cout * chain_pixels(name) for name, (k, cin, cout) in net.layer_shapes_resnet18(SCALE_NUM, True).items())
    model = net.ResNet18Trainable(weights, scale_num=SCALE_NUM).cuda()
    ours = training_step(model, torch.optim.Adam(model.parameters(), lr=1e-6, capturable=True), lidar, gt)
    if EAGER:
        emodel = EagerNet(weights).cuda()
        eager = training_step(emodel, torch.optim.Adam(emodel.parameters(), lr=1e-6, capturable=True), lidar, gt)
    else:
        eager = None
    report({"op": "training_step", "net": "ResNet18_NO_BN_l2", "if_correct": True, "joint_train": False, "scale_num": SCALE_NUM,
            "shape": [B, H, W], "FLOP_per_frame": flop}, flop * B, ours, eager, lambda: None)
    del model, ours, eager
    torch.cuda.empty_cache()

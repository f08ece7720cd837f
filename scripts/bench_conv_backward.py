"""Measures the backward pass of SparsityCNN's layers (dtfill_conv2d_backward_data, dtfill_conv2d_backward_weights) layer by
layer, and one whole training step of SparsityCNNTrainable (forward, autograd.train_loss, backward, Adam), against the same
layers' and the same net's backward in eager torch (aten.convolution_backward behind aten.leaky_relu_backward; F.conv2d under
the tape), float32, channels-last, on the same tensors, on the same device, in the same run.
Shape: the reference's cropped KITTI frame 256 x 1216 at B = 1 and B = 4, scale_num 4, if_correct.

Per row, microseconds per call from HIP events over ROUNDS rounds, ours and eager alternating within a round; a round times
enough calls to fill about WINDOW_US after a warm-up of the same calls.  Reported: the median and the (min .. max) spread of
the rounds, the TFLOP/s of our call (2 ksize^2 Cin Cout FLOP per pixel for dx and again for dw) as a share of the 157.3 TF
FP32 peak, the workspace bytes of the layer, and the largest absolute difference between the two results (the eager side sums
in another order: close, not equal).  One JSON line per row.  --no-eager leaves the eager side out."""
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


def nchw_view(t):
    """[B,H,W,C] contiguous -> the same memory as a channels-last [B,C,H,W] tensor."""
    return t.permute(0, 3, 1, 2)


def eager_backward(x_cl, dy_cl, y_cl, kernel_oihw, act, mask):
    """aten's backward of conv2d + leaky_relu: mask = (dx, dw, db) wanted."""
    g = aten.leaky_relu_backward(dy_cl, y_cl, ALPHA, True) if act == "leaky" else dy_cl
    pad = kernel_oihw.shape[2] // 2
    return aten.convolution_backward(g, x_cl, kernel_oihw, [kernel_oihw.shape[0]], [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)


class EagerNet(torch.nn.Module):
    """SparsityCNNTrainable's forward with F.conv2d; the fill and the loss stay this library's operators on both sides."""

    def __init__(self, weights):
        super().__init__()
        for n, (k, b) in weights.items():
            if n != "lidar_conv_extra_3":
                kernel = torch.from_numpy(k).permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)
                self.register_parameter(n + "_kernel", torch.nn.Parameter(kernel))
                self.register_parameter(n + "_bias", torch.nn.Parameter(torch.from_numpy(b.copy())))
        self.register_buffer("threshold", torch.tensor(0.1))
        self.register_buffer("scale", torch.tensor(90.0))

    def layer(self, x, name, act):
        kernel = getattr(self, name + "_kernel")
        y = Fn.conv2d(x, kernel, getattr(self, name + "_bias"), padding=kernel.shape[2] // 2)
        return Fn.leaky_relu(y, ALPHA) if act == "leaky" else y

    def forward(self, x):
        mask = torch.gt(x, self.threshold).float()
        t = (x / self.scale)[:, None]
        for name in ("correct_1", "correct_2", "correct_3"):
            t = self.layer(t, name, "leaky")
        correct = self.layer(t, "correct_4", "linear")[:, 0].contiguous() * mask
        lidars = autograd.generate_multi_channel(correct.detach(), mask, 7, SCALE_NUM)
        t = torch.cat([self.layer(l[:, None], n, "leaky") for l, n in zip(lidars, net.stem_layers(SCALE_NUM))], dim=1)
        for name in ("conv1a", "conv1b", "conv1c", "conv1d"):
            t = self.layer(t, name, "leaky")
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
    weights = net.glorot_weights(0, SCALE_NUM, True, bias=0.1)
    up = lambda a: torch.from_numpy(a).cuda()
    ours_w = {n: up(k) for n, (k, b) in weights.items()}
    eager_w = {n: k.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last) for n, k in ours_w.items()}
    gen = torch.Generator(device="cuda").manual_seed(B)
    pixels = B * H * W
    # ---- layer by layer: each layer of the net on random tensors of its shape ----
    for name, (k, cin, cout) in net.layer_shapes(SCALE_NUM, True).items():
        act = "linear" if cout == 1 else "leaky"
        x, dy, y = (torch.randn((B, H, W, c), device="cuda", generator=gen) for c in (cin, cout, cout))
        kernel = ours_w[name]
        row = {"layer": name, "ksize": k, "Cin": cin, "Cout": cout, "shape": [B, H, W],
               "workspace_bytes": dev.conv2d_backward_workspace_bytes(B, H, W, cin, k, cout)}
        flop = 2.0 * k * k * cin * cout * pixels
        dx = torch.empty((B, H, W, cin), device="cuda")
        ours = lambda: dev.conv2d_backward_data_device(dy, kernel, y, act, ALPHA, dx=dx)
        eager = lambda: eager_backward(nchw_view(x), nchw_view(dy), nchw_view(y), eager_w[name], act, [True, False, False])[0]
        report(dict(op="conv2d_backward_data", **row), flop, ours, eager, lambda: (nchw_view(ours()) - eager()).abs().max().item())
        ours = lambda: dev.conv2d_backward_weights_device(x, dy, k, y, act, ALPHA)
        eager = lambda: eager_backward(nchw_view(x), nchw_view(dy), nchw_view(y), eager_w[name], act, [False, True, True])[1:]
        diff = lambda: max((a - b).abs().max().item() for a, b in zip(ours(), (eager()[0].permute(2, 3, 1, 0), eager()[1])))
        report(dict(op="conv2d_backward_weights", **row), flop, ours, eager, diff)
        del x, dy, y, dx
    # ---- the whole step of train.py:232-254 ----
    lidar = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
    gt = torch.from_numpy(synth.kitti_iid(B, p=0.3, seed=100 + B, hw=(H, W))).cuda()
    shapes = net.layer_shapes(SCALE_NUM, True)
    flop = 3 * sum(2.0 * k * k * cin * cout for k, cin, cout in shapes.values())  # forward, dx and dw of every layer (an upper count)
    model = net.SparsityCNNTrainable(weights, scale_num=SCALE_NUM).cuda()
    ours = training_step(model, torch.optim.Adam(model.parameters(), lr=1e-5, capturable=True), lidar, gt)
    if EAGER:
        emodel = EagerNet(weights).cuda()
        eager = training_step(emodel, torch.optim.Adam(emodel.parameters(), lr=1e-5, capturable=True), lidar, gt)
    else:
        eager = None
    report({"op": "training_step", "net": "SparsityCNN", "if_correct": True, "joint_train": False, "scale_num": SCALE_NUM,
            "shape": [B, H, W], "FLOP_per_pixel": flop}, flop * pixels, ours, eager, lambda: None)
    del ours_w, eager_w, model
    torch.cuda.empty_cache()

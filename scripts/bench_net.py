"""Measures SparsityCNN's forward (net.py, dtfill_conv2d) layer by layer and as a whole against the same layers and the same
net in eager torch.nn.functional.conv2d, float32, channels-last, on the same tensors, on the same device, in the same run.
Shape: the reference's cropped KITTI frame 256 x 1216 at B = 1 and B = 8, scale_num 4, both if_correct settings.

Per row, microseconds per call from HIP events over ROUNDS rounds, ours and eager alternating within a round; a round times
enough calls to fill about WINDOW_US after a warm-up of the same calls.  Reported: the median and the (min .. max) spread of
the rounds, the TFLOP/s of our call (2 ksize^2 Cin Cout FLOP per pixel, padding taps counted) as a share of the 157.3 TF FP32
peak, and the largest absolute difference between the two results (the eager side sums in another order: close, not equal).
The eager net is the same forward with F.conv2d and F.leaky_relu around the same dtfill_generate_multi_channel call.
One JSON line per row.  --no-eager leaves the eager side out (it builds its kernels on first use, which can take minutes)."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as Fn
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
net = importlib.import_module(pkg.__name__ + ".net")
synth = importlib.import_module(pkg.__name__ + ".synth")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
pkg._lib.load()
dev = pkg.device
EAGER = "--no-eager" not in sys.argv
ROUNDS, WINDOW_US, PEAK_TF = 5, 30e3, 157.3
H, W, SCALE_NUM = 256, 1216, 4


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
        counts.append(max(5, int(WINDOW_US / max(timed(f, 5), 1.0))))
    rounds = [[] for _ in fs]
    for _ in range(ROUNDS):
        for k, f in enumerate(fs):
            rounds[k].append(timed(f, counts[k]))
    return [{"us": round(statistics.median(r), 2), "min": round(min(r), 2), "max": round(max(r), 2)} for r in rounds]


def report(res, flop, ours, eager, diff):
    fs = [ours] + ([eager] if EAGER else [])
    t = compare(fs)
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


def eager_layer(x_cl, kernel_oihw, bias, act):
    y = Fn.conv2d(x_cl, kernel_oihw, bias, padding=kernel_oihw.shape[2] // 2)
    return Fn.leaky_relu(y, net.LEAKY_ALPHA) if act == "leaky" else y


def eager_net(x, wts, if_correct, scale, threshold):
    """SparsityCNN.__call__ with eager convolutions; wts: {name: (OIHW channels-last kernel, bias)}."""
    B = x.shape[0]
    mask = torch.gt(x, threshold).float()
    scaled = x / scale
    if if_correct:
        t = scaled[:, None]
        for name in ("correct_1", "correct_2", "correct_3"):
            t = eager_layer(t, *wts[name], "leaky")
        correct = eager_layer(t, *wts["correct_4"], "linear")[:, 0].contiguous() * mask
    else:
        correct = scaled * mask
    lidars = dev.generate_multi_channel_device(correct, mask, 7, SCALE_NUM)
    t = torch.cat([eager_layer(l[:, None], *wts[n], "leaky") for l, n in zip(lidars, net.stem_layers(SCALE_NUM))], dim=1)
    for name in ("conv1a", "conv1b", "conv1c", "conv1d"):
        t = eager_layer(t, *wts[name], "leaky")
    return eager_layer(t, *wts["conv_output"], "linear")[:, 0] * scale, correct * scale


for B in (1, 8):
    weights = net.glorot_weights(0, SCALE_NUM, True, bias=0.1)
    up = lambda a: torch.from_numpy(a).cuda()
    ours_w = {n: (up(k), up(b)) for n, (k, b) in weights.items()}
    eager_w = {n: (k.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last), b) for n, (k, b) in ours_w.items()}
    gen = torch.Generator(device="cuda").manual_seed(B)
    pixels = B * H * W
    with torch.no_grad():
        # ---- layer by layer: the layers of the forward, each on a random input of its shape ----
        for name, (k, cin, cout) in net.layer_shapes(SCALE_NUM, True).items():
            act = "linear" if cout == 1 else "leaky"
            x = torch.randn((B, H, W, cin), device="cuda", generator=gen)
            out = torch.empty((B, H, W, cout), device="cuda")
            kernel, bias = ours_w[name]
            ours = lambda: dev.conv2d_device(x, kernel, bias, act, net.LEAKY_ALPHA, out)
            eager = lambda: eager_layer(nchw_view(x), *eager_w[name], act)
            diff = lambda: (nchw_view(ours()) - eager()).abs().max().item()
            report({"op": "conv2d", "layer": name, "ksize": k, "Cin": cin, "Cout": cout, "shape": [B, H, W]},
                   2.0 * k * k * cin * cout * pixels, ours, eager, diff)
        # ---- the whole forward ----
        frames = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
        threshold, scale = torch.tensor(0.1, device="cuda"), torch.tensor(90.0, device="cuda")
        for if_correct in (True, False):
            shapes = net.layer_shapes(SCALE_NUM, if_correct)
            stems = net.stem_layers(SCALE_NUM)
            flop = sum(2.0 * k * k * cin * cout for n, (k, cin, cout) in shapes.items() if n not in stems)
            flop += sum(2.0 * 9 * 16 for _ in stems)
            model = net.SparsityCNN(weights, if_correct=if_correct, scale_num=SCALE_NUM)
            ours = lambda: model(frames)
            eager = lambda: eager_net(frames, eager_w, if_correct, scale, threshold)
            diff = lambda: max((a - b).abs().max().item() for a, b in zip(ours(), eager()))
            report({"op": "SparsityCNN", "if_correct": if_correct, "scale_num": SCALE_NUM, "shape": [B, H, W],
                    "FLOP_per_pixel": flop}, flop * pixels, ours, eager, diff)
    del ours_w, eager_w
    torch.cuda.empty_cache()

"""Measures ResNet18's forward (net.py: dtfill_conv2d_strided, dtfill_conv2d_transpose) layer shape by layer shape and as a
whole against the same layers and the same net in eager torch.nn.functional.conv2d / conv_transpose2d / add / leaky_relu,
float32, channels-last, on the same tensors, on the same device, in the same run.  Shape: the reference's cropped KITTI frame
256 x 1216 at B = 1 and B = 8, scale_num 4, if_correct on.  The method is scripts/bench_net.py's: microseconds per call from HIP
events over ROUNDS rounds, ours and eager alternating within a round, a round of about WINDOW_US after a warm-up of the same
calls; the median and the (min .. max) spread of the rounds; the TFLOP/s of our call as a share of the 157.3 TF FP32 peak (2 FLOP
per link of the chain, padding taps counted; the transposed convolution has 9 / 4 taps per output on average); the largest
absolute difference between the two results (the eager side sums in another order: close, not equal).

The yardstick of the same run is the parent's kernel, k_conv_mfma on 7x7x64->16 (SparsityCNN's conv1a), first row of a batch.
A residual block's second convolution is timed with its residual: ours fuses the add and the leaky_relu, eager runs them.
One JSON line per row.  --no-eager leaves the eager side out (it builds its kernels on first use, which can take minutes);
--batches 1,8 chooses the batch sizes; --no-net leaves the whole forward out."""
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
EAGER, NET = "--no-eager" not in sys.argv, "--no-net" not in sys.argv
BATCHES = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(",")) if "--batches" in sys.argv else (1, 8)
ROUNDS, WINDOW_US, PEAK_TF = 5, 30e3, 157.3
H, W, SCALE_NUM = 256, 1216, 4
ALPHA = net.LEAKY_ALPHA


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
    fs = [ours] + ([eager] if EAGER and eager else [])
    t = compare(fs)
    res["ours"] = t[0]
    res["TFLOPs"] = round(flop / t[0]["us"] / 1e6, 2)
    res["share_of_fp32_peak"] = round(flop / t[0]["us"] / 1e6 / PEAK_TF, 3)
    if len(fs) > 1:
        res["eager"] = t[1]
        res["eager_over_ours"] = round(t[1]["us"] / t[0]["us"], 2)
        res["max_abs_diff"] = diff()
    print(json.dumps(res), flush=True)


def nchw_view(t):
    """[B,H,W,C] contiguous -> the same memory as a channels-last [B,C,H,W] tensor."""
    return t.permute(0, 3, 1, 2)


def level_of(name):
    """The level (0: the full frame, k: 1 / 2^k each way) a layer's INPUT lives at."""
    if name.startswith("conv") and name[4].isdigit():
        k = int(name[4]) - 1
        return k - 1 if name in net.RESNET_STRIDE2 else k
    if name.startswith("upsample_"):
        k = int(name[9])  # upsample_k reads level k (0-based: k - 1), upsample_k_post the level above; upsample_1 stays
        return 0 if k == 1 else k - 2 if name.endswith("_post") else k - 1
    return 0


def flop_per_call(name, k, cin, cout, pixels_in):
    """2 FLOP per link; pixels_in: pixels of the layer's input."""
    if name in net.RESNET_TRANSPOSED:
        return 2.0 * 9 * cin * cout * pixels_in  # 4 outputs a pixel, 9 / 4 taps each
    return 2.0 * k * k * cin * cout * pixels_in / (4 if name in net.RESNET_STRIDE2 else 1)


def eager_conv(x_cl, w_oihw, bias, stride=1):
    """TensorFlow's 'same' rule for the even frames of this benchmark: stride 1 pads (k - 1) / 2 all round; stride 2 pads one
    row below and one column to the right for 3x3 and nothing for 1x1."""
    k = w_oihw.shape[2]
    if stride == 1:
        return Fn.conv2d(x_cl, w_oihw, bias, padding=k // 2)
    return Fn.conv2d(Fn.pad(x_cl, (0, 1, 0, 1)) if k == 3 else x_cl, w_oihw, bias, stride=2)


def eager_up(x_cl, w_iohw, bias):
    y = Fn.conv_transpose2d(x_cl, w_iohw, bias, stride=2)
    return y[:, :, :2 * x_cl.shape[2], :2 * x_cl.shape[3]]


def eager_net(x, wts, scale, threshold):
    """ResNet18.__call__ with eager convolutions; wts: {name: (OIHW channels-last kernel -- IOHW for the transposed --, bias)}."""
    lk = lambda y: Fn.leaky_relu(y, ALPHA)
    conv = lambda t, name, stride=1: eager_conv(t, *wts[name], stride)
    mask = torch.gt(x, threshold).float()
    t = (x / scale)[:, None]
    for name in ("correct_1", "correct_2", "correct_3"):
        t = lk(conv(t, name))
    correct = conv(t, "correct_4")[:, 0].contiguous() * mask
    lidars = dev.generate_multi_channel_device(correct, mask, 7, SCALE_NUM)
    stems = torch.cat([lk(conv(l[:, None], n)) for l, n in zip(lidars, net.stem_layers(SCALE_NUM))], dim=1)
    below, totals = stems, []
    for level in (1, 2, 3, 4):
        name, stride = "conv%d" % level, 1 if level == 1 else 2
        total = lk(conv(lk(conv(below, name + "a", stride)), name + "b") + conv(below, name + "a_extra", stride))
        t = conv(lk(conv(total, name + "c")), name + "d")
        below = lk(t + total if level < 4 else t)
        totals.append(below)
    for level in (4, 3, 2):
        below = lk(conv(torch.cat([lk(eager_up(below, *wts["upsample_%d" % level])), totals[level - 2]], 1), "upsample_%d_post" % level))
    t = lk(conv(torch.cat([lk(conv(below, "upsample_1")), stems], 1), "upsample_1_post"))
    return conv(t, "conv_output")[:, 0] * scale, correct * scale


shapes = net.layer_shapes_resnet18(SCALE_NUM, True)
stem_names = net.stem_layers(SCALE_NUM)
HEAD = tuple(n for n in shapes if n.startswith("correct")) + tuple(stem_names) + ("conv_output",)
FLOP_FRAME = sum(flop_per_call(n, k, cin, cout, (H >> level_of(n)) * (W >> level_of(n))) for n, (k, cin, cout) in shapes.items()
                 if n not in stem_names) + sum(2.0 * 9 * 16 * H * W for _ in stem_names)
print(json.dumps({"FLOP_per_frame": FLOP_FRAME, "ms_at_peak": round(FLOP_FRAME / PEAK_TF / 1e9, 3), "shape": [H, W],
                  "scale_num": SCALE_NUM}), flush=True)

for B in BATCHES:
    weights = net.glorot_weights_resnet18(0, SCALE_NUM, True, bias=0.1)
    up = lambda a: torch.from_numpy(a).cuda()
    keras = {n: (up(k), up(b)) for n, (k, b) in weights.items()}
    # ours: [k,k,Cin,Cout], the transposed packed; eager: OIHW (conv2d) and IOHW (conv_transpose2d), both = permute(3, 2, 0, 1)
    # of Keras's [k,k,Cin,Cout] and [3,3,Cout,Cin]
    ours_w = {n: (k.permute(0, 1, 3, 2).contiguous() if n in net.RESNET_TRANSPOSED else k, b) for n, (k, b) in keras.items()}
    eager_w = {n: (k.permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last), b) for n, (k, b) in keras.items()}
    gen = torch.Generator(device="cuda").manual_seed(B)
    with torch.no_grad():
        # ---- the yardstick: the parent's kernel on SparsityCNN's conv1a ----
        x = torch.randn((B, H, W, 64), device="cuda", generator=gen)
        yk, yb = torch.randn((7, 7, 64, 16), device="cuda", generator=gen) / 56, torch.zeros(16, device="cuda")
        out = torch.empty((B, H, W, 16), device="cuda")
        report({"op": "conv2d", "layer": "yardstick: k_conv_mfma 7x7x64->16", "shape": [B, H, W]}, 2.0 * 49 * 64 * 16 * B * H * W,
               lambda: dev.conv2d_device(x, yk, yb, "leaky", ALPHA, out), None, None)
        del x, out
        # ---- every distinct layer shape of the forward, each on a random input of its shape ----
        seen = set()
        for name, (k, cin, cout) in shapes.items():
            if name in HEAD:
                continue  # dtfill_conv2d's layers: scripts/bench_net.py
            lv, transposed = level_of(name), name in net.RESNET_TRANSPOSED
            stride = 2 if name in net.RESNET_STRIDE2 else 1
            residual = name[-1] in "bd" and name.startswith("conv") and name != "conv4d"
            act = "linear" if name.endswith("_extra") else "leaky"
            key = (k, cin, cout, lv, stride, transposed, residual, act)
            if key in seen:
                continue
            seen.add(key)
            h, w = H >> lv, W >> lv
            ho, wo = (2 * h, 2 * w) if transposed else (h // stride, w // stride)
            x = torch.randn((B, h, w, cin), device="cuda", generator=gen)
            res = torch.randn((B, ho, wo, cout), device="cuda", generator=gen) if residual else None
            out = torch.empty((B, ho, wo, cout), device="cuda")
            kernel, bias = ours_w[name]
            ek, eb = eager_w[name]
            if transposed:
                ours = lambda: dev.conv2d_transpose_device(x, kernel, bias, act, ALPHA, out)
                eager = lambda: Fn.leaky_relu(eager_up(nchw_view(x), ek, eb), ALPHA)
            else:
                ours = lambda: dev.conv2d_strided_device(x, kernel, bias, stride, res, act, ALPHA, out)

                def eager():
                    y = eager_conv(nchw_view(x), ek, eb, stride)
                    if residual:
                        y = y + nchw_view(res)
                    return Fn.leaky_relu(y, ALPHA) if act == "leaky" else y
            diff = lambda: (nchw_view(ours()) - eager()).abs().max().item()
            report({"op": "conv2d_transpose" if transposed else "conv2d_strided", "layer": name, "ksize": k, "Cin": cin, "Cout": cout,
                    "stride": stride, "residual": residual, "shape": [B, h, w]}, flop_per_call(name, k, cin, cout, B * h * w),
                   ours, eager, diff)
            del x, res, out
        # ---- the whole forward ----
        if NET:
            frames = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
            threshold, scale = torch.tensor(0.1, device="cuda"), torch.tensor(90.0, device="cuda")
            model = net.ResNet18(weights, scale_num=SCALE_NUM)
            ours = lambda: model(frames)
            eager = lambda: eager_net(frames, eager_w, scale, threshold)
            diff = lambda: max((a - b).abs().max().item() for a, b in zip(ours(), eager()))
            report({"op": "ResNet18", "if_correct": True, "scale_num": SCALE_NUM, "shape": [B, H, W],
                    "FLOP_per_pixel": FLOP_FRAME / (H * W)}, FLOP_FRAME * B, ours, eager, diff)
            del model, frames
    del ours_w, eager_w, keras
    torch.cuda.empty_cache()

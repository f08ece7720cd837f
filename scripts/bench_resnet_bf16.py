"""Measures the bf16 wide layers (dtfill_conv2d_strided_bf16, dtfill_conv2d_transpose_bf16) beside their float32 twins, layer
shape by layer shape and as whole forwards of the three inference ResNets, in the same run.  Shape: the reference's cropped
KITTI frame 256 x 1216 at B = 1 and B = 8, scale_num 4, if_correct on.  The method is scripts/bench_resnet.py's: microseconds
per call from HIP events over ROUNDS rounds, the two sides alternating within a round, a round of about WINDOW_US after a warm-up
of the same calls; the median and the (min .. max) spread of the rounds.

The layer shapes are not restated here: one forward of each network at B = 1 is run with net.py's layer functions wrapped, and
every distinct (kind, ksize, Cin, Cout, frame, stride, residual, activation) that goes through _wide or _up is a row.  Per row:
the two times, their ratio, the layer's byte floor (x read once and out written once, float32, and the residual where there is
one) at the 6.29 TB/s a float4 copy reaches on this chip, and how many floors the bf16 call took.  Per network and batch: the
float32 and the bf16 forward and the max and mean |bf16 - float32| of the outputs under glorot weights (for the record; the
accuracy of trained checkpoints is unmeasured).  One-off: the pack time and the packed bytes of each network.
One JSON line per row.  --batches 1,8 chooses the batch sizes; --no-layers and --no-net leave a part out."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
net = importlib.import_module(pkg.__name__ + ".net")
synth = importlib.import_module(pkg.__name__ + ".synth")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
pkg._lib.load()
dev = pkg.device
LAYERS, NET = "--no-layers" not in sys.argv, "--no-net" not in sys.argv
BATCHES = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(",")) if "--batches" in sys.argv else (1, 8)
ROUNDS, WINDOW_US, COPY_TBS = 5, 30e3, 6.29
H, W, SCALE_NUM = 256, 1216, 4
ALPHA = net.LEAKY_ALPHA
NETS = (("ResNet18", net.ResNet18, net.glorot_weights_resnet18), ("ResNet18Image", net.ResNet18Image, net.glorot_weights_resnet18_image),
        ("ResNet18LightImage", net.ResNet18LightImage, net.glorot_weights_resnet18_light_image))


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


def faster_by_more_than_the_spread(a, b):
    """b's slowest round is faster than a's fastest"""
    return b["max"] < a["min"]


def wide_calls(model, inputs):
    """The (kind, ksize, Cin, Cout, h, w, stride, residual, act) of every call one forward makes through _wide and _up."""
    calls = []
    strided, transpose = net.conv2d_strided_device, net.conv2d_transpose_device

    def rec_strided(x, kernel, bias, stride, residual, act, alpha, out, out_offset):
        calls.append(("strided", kernel.shape[0], x.shape[3], kernel.shape[3], x.shape[1], x.shape[2], stride, residual is not None, act))
        return strided(x, kernel, bias, stride, residual, act, alpha, out, out_offset)

    def rec_transpose(x, kernel, bias, act, alpha, out):
        calls.append(("transposed", 3, x.shape[3], kernel.shape[3], x.shape[1], x.shape[2], 2, False, act))
        return transpose(x, kernel, bias, act, alpha, out)

    net.conv2d_strided_device, net.conv2d_transpose_device = rec_strided, rec_transpose
    try:
        model(*inputs)
    finally:
        net.conv2d_strided_device, net.conv2d_transpose_device = strided, transpose
    return calls


def inputs_of(name, B):
    frames = torch.from_numpy(synth.kitti_iid(B, p=0.05, seed=B, hw=(H, W))).cuda()
    if name == "ResNet18":
        return (frames,)
    rgb = torch.rand((B, H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
    return (frames, rgb)


weights = {name: glorot(0, SCALE_NUM, True, bias=0.1) for name, _, glorot in NETS}
with torch.no_grad():
    rows, users = [], {}
    for name, cls, _ in NETS:
        model = cls(weights[name], scale_num=SCALE_NUM)
        for call in wide_calls(model, inputs_of(name, 1)):
            if call not in users:
                rows.append(call)
            users.setdefault(call, set()).add(name)
        del model
    torch.cuda.empty_cache()
    print(json.dumps({"distinct_wide_layer_shapes": len(rows), "shape": [H, W], "scale_num": SCALE_NUM, "floor_rate_TBs": COPY_TBS}), flush=True)
    for B in BATCHES:
        gen = torch.Generator(device="cuda").manual_seed(B)
        # ---- every distinct wide layer shape, each on a random input of its shape, glorot-scaled weights ----
        for kind, k, cin, cout, h, w, stride, residual, act in rows if LAYERS else ():
            transposed = kind == "transposed"
            ho, wo = (2 * h, 2 * w) if transposed else (-(-h // stride), -(-w // stride))
            x = torch.randn((B, h, w, cin), device="cuda", generator=gen)
            res = torch.randn((B, ho, wo, cout), device="cuda", generator=gen) if residual else None
            kernel = (torch.rand((k, k, cin, cout), device="cuda", generator=gen) * 2 - 1) * float(np.sqrt(6.0 / (k * k * (cin + cout))))
            bias = torch.rand((cout,), device="cuda", generator=gen) * 0.1
            packed = dev.pack_bf16_device(kernel, transposed)
            o32, o16 = torch.empty((B, ho, wo, cout), device="cuda"), torch.empty((B, ho, wo, cout), device="cuda")
            if transposed:
                f32 = lambda: dev.conv2d_transpose_device(x, kernel, bias, act, ALPHA, o32)
                f16 = lambda: dev.conv2d_transpose_bf16_device(x, packed, bias, act, ALPHA, o16)
            else:
                f32 = lambda: dev.conv2d_strided_device(x, kernel, bias, stride, res, act, ALPHA, o32)
                f16 = lambda: dev.conv2d_strided_bf16_device(x, packed, bias, stride, res, act, ALPHA, o16)
            t32, t16 = compare([f32, f16])
            nbytes = 4.0 * (x.numel() + o16.numel() + (res.numel() if residual else 0))
            floor_us = nbytes / COPY_TBS / 1e6
            taps = 9.0 / 4 if transposed else k * k
            flop = 2.0 * taps * cin * cout * B * ho * wo
            print(json.dumps({"op": "conv2d_%s" % kind, "ksize": k, "Cin": cin, "Cout": cout, "stride": stride, "residual": residual, "act": act,
                              "shape": [B, h, w], "nets": sorted(users[(kind, k, cin, cout, h, w, stride, residual, act)]), "float32": t32,
                              "bf16": t16, "float32_over_bf16": round(t32["us"] / t16["us"], 2),
                              "faster_by_more_than_the_spread": faster_by_more_than_the_spread(t32, t16), "MB": round(nbytes / 1e6, 2),
                              "byte_floor_us": round(floor_us, 2), "bf16_over_byte_floor": round(t16["us"] / floor_us, 2),
                              "bf16_TFLOPs": round(flop / t16["us"] / 1e6, 1), "max_abs_diff": round((o32 - o16).abs().max().item(), 6),
                              "max_abs_out": round(o32.abs().max().item(), 4)}), flush=True)
            del x, res, kernel, packed, o32, o16
        # ---- the whole forwards ----
        for name, cls, _ in NETS if NET else ():
            inputs = inputs_of(name, B)
            m32 = cls(weights[name], scale_num=SCALE_NUM)
            m16 = cls(weights[name], scale_num=SCALE_NUM, precision="bf16")
            m32._state(inputs[0].device)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            m16._on[inputs[0].device] = m32._on[inputs[0].device]  # (the float32 uploads are shared: the pack alone is timed)
            e0.record(); m16._state(inputs[0].device); e1.record(); torch.cuda.synchronize()
            packed_bytes = sum(p.numel() * 2 for p in m16._packed[inputs[0].device].values())
            t32, t16 = compare([lambda: m32(*inputs), lambda: m16(*inputs)])
            d = [(a - b).abs() for a, b in zip(m32(*inputs), m16(*inputs))]
            print(json.dumps({"op": name, "scale_num": SCALE_NUM, "shape": [B, H, W], "float32": t32, "bf16": t16,
                              "float32_over_bf16": round(t32["us"] / t16["us"], 2),
                              "faster_by_more_than_the_spread": faster_by_more_than_the_spread(t32, t16),
                              "pack_us_first_call": round(e0.elapsed_time(e1) * 1e3, 1), "packed_MB": round(packed_bytes / 1e6, 2),
                              "wide_layers": len(m16.wide_layers), "output_max_abs_diff": round(d[0].max().item(), 5),
                              "output_mean_abs_diff": round(d[0].mean().item(), 6), "output_max_abs": round(m32(*inputs)[0].abs().max().item(), 4)}),
                  flush=True)
            del m32, m16, inputs
            torch.cuda.empty_cache()

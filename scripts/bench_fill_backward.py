"""Measures the backward pass of the exact fill (dtfill_fill_backward: k_fb_count, k_fb_scan, k_fb_acc<0>, k_fb_acc<1>, k_fb_out)
against the same gradient written as eager torch ops (compare, cumsum, index_add_, gather), on the same tensors, on the same
device, in the same run.  Frames: the KITTI batch 32 x 352 x 1216 of bench.py's scan-line workload, a 240 x 320 NYU frame with
500 sources, and one frame of each size with a single source (every pixel of the frame adds into one accumulator).

Per frame set, microseconds per call from HIP events over ROUNDS rounds, fused and eager alternating within a round; a round
times enough calls to fill about 50 ms after a warm-up of the same calls.  Reported: the median and the (min .. max) spread of
the rounds, the fused call's GB/s against its byte floor of 24 B/px (x 4 + index 2 x 4 + grad_depth 2 x 4 read, grad_x 4 written:
index and grad_depth are read twice, DESIGN.md says why), ns per pixel, and the two results' largest difference (the eager
index_add_ is a float32 atomic sum in arrival order: close, not equal, and not the same from run to run).  The eager form has
no host synchronisation either (no nonzero): the label-to-pixel map comes from the cumsum.
One JSON line per frame set."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
L = pkg._lib.load()
st = torch.cuda.current_stream().cuda_stream
ROUNDS, WINDOW_US = 7, 50e3
VAL_THR = 0.1


def check(rc):
    assert rc == 0, L.dtfill_strerror(rc).decode()


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def compare(fused, eager):
    """Median and spread of ROUNDS alternating rounds of each, in microseconds per call."""
    counts = []
    for f in (fused, eager):
        for _ in range(10):
            f()
        counts.append(max(20, int(WINDOW_US / max(timed(f, 20), 1.0))))
    rounds = ([], [])
    for _ in range(ROUNDS):
        for k, f in enumerate((fused, eager)):
            rounds[k].append(timed(f, counts[k]))
    return [{"us": round(statistics.median(r), 2), "min": round(min(r), 2), "max": round(max(r), 2)} for r in rounds]


def eager_backward(x, index, grad):
    """The transposed gather in eager ops, frames without an index error: sums per value-list entry by index_add_, then every
    valued pixel reads the sum of its own rank."""
    B, H, W = x.shape
    HW = H * W
    valued = (x > VAL_THR).reshape(B, HW)
    rank = valued.cumsum(1)  # 1-based rank of a valued pixel in its frame's list; the last column is n
    idx = index.reshape(B, HW).long() - 1
    idx = torch.where(idx < 0, idx + rank[:, -1:], idx)
    idx = idx + torch.arange(B, device=x.device).unsqueeze(1) * HW
    sums = torch.zeros(B * HW, dtype=torch.float32, device=x.device).index_add_(0, idx.reshape(-1), grad.reshape(-1))
    mine = sums.reshape(B, HW).gather(1, (rank - 1).clamp_(min=0))
    return torch.where(valued, mine, torch.zeros((), device=x.device)).reshape(B, H, W)


def frames():
    kitti = synth.make("kitti_b32_scanline")
    yield "kitti_b32_scanline", kitti
    nyu = np.zeros((1, 240, 320), np.float32)
    rng = np.random.default_rng(7)
    at = rng.choice(240 * 320, 500, replace=False)
    nyu.reshape(-1)[at] = (np.round(rng.uniform(1, 10, 500) * 256) / 256).astype(np.float32)
    yield "nyu_240x320_500_sources", nyu
    for name, (B, H, W) in (("single_source_b32_352x1216", (32, 352, 1216)), ("single_source_1_240x320", (1, 240, 320))):
        one = np.zeros((B, H, W), np.float32)
        one[:, H // 2, W // 3] = 5.0
        yield name, one


op = pkg.device.DtFill(device="cuda:0")
for name, xh in frames():
    B, H, W = xh.shape
    n = B * H * W
    x = torch.from_numpy(xh).to("cuda:0")
    res = op.run(x)
    index = res["index"].clone()
    assert not (res["status"] & 1).any().item()
    gen = torch.Generator(device="cuda").manual_seed(B)
    grad = torch.randn((B, H, W), device="cuda", generator=gen)
    out = torch.empty_like(x)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    need = L.dtfill_fill_backward_workspace_bytes(B, H, W)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    fused = lambda: check(L.dtfill_fill_backward(x.data_ptr(), index.data_ptr(), grad.data_ptr(), B, H, W, VAL_THR, out.data_ptr(),
                                                 status.data_ptr(), ws_ptr, need, st))
    eager = lambda: eager_backward(x, index, grad)
    fu, ea = compare(fused, eager)
    fused()
    first = out.clone()
    fused()
    eg = eager()
    rec = {"op": "fill_backward", "frames": name, "shape": [B, H, W], "sources_per_frame": int((x > VAL_THR).sum().item()) // B,
           "fused": fu, "eager": ea, "eager_over_fused": round(ea["us"] / fu["us"], 2),
           "fused_GBs_vs_24B_floor": round(24 * n / fu["us"] / 1e3, 1), "fused_ns_per_px": round(fu["us"] * 1e3 / n, 4),
           "fused_two_calls_same_bits": bool(torch.equal(first.view(torch.int32), out.view(torch.int32))),
           "max_abs_diff_vs_eager": (eg - out).abs().max().item(), "max_abs_eager": eg.abs().max().item(),
           "workspace_MiB": round(need / 2 ** 20, 1)}
    del eg, first, ws
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)

"""Measures the nearest-source gather and its backward (dtfill_nearest_gather: k_ng_count, k_ng_scan, k_ng_list, k_ng_gather;
dtfill_nearest_gather_backward: k_ng_count, k_ng_scan, then k_ngb_acc<0>, k_ngb_acc<1>, k_ngb_out per round of two channels)
against the same results written as eager torch ops, on the same tensors, on the same device, in the same run.
  eager forward   the source mask, its cumsum, a scatter that builds rank -> pixel, then gathers (the pixel map, every channel);
  eager backward  index_add_ per channel into per-source sums, then a scatter of the sums to the source pixels.
Neither eager form calls nonzero or synchronises with the host.  Frames: the KITTI batch 32 x 352 x 1216 of bench.py's scan-line
workload at C = 1 and C = 3, a 240 x 320 NYU frame with 500 sources (C = 3), and one frame of each size with a single source
(C = 1).

Per frame set, microseconds per call from HIP events over ROUNDS rounds, fused and eager alternating within a round; a round
times enough calls to fill about 50 ms after a warm-up of the same calls.  Reported: the median and the (min .. max) spread of
the rounds, eager / fused, the fused call's GB/s against its byte floor, and the two results' largest difference.  The floors,
from the shapes: forward 4 (x) + 4 (index) + 4 (pixel) + 4 C (filled) bytes per pixel, the gathered reads of spix and values
counted apart (4 + 4 C per pixel, mostly broadcast and cached); backward 4 (x) + 8 per round (index, read in both passes) + 8 C
(grad_out, read in both passes) + 4 C (grad_values), a round being two channels.  The forward copies bits, so its difference
from the eager gather is 0; the eager index_add_ is a float32 atomic sum in arrival order: close, not equal.
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
SRC_THR = 0.1


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


def rank_table(x):
    """(src [B,HW], rank [B,HW] 1-based among the frame's sources, table [B,HW+1] rank - 1 -> pixel; slot HW takes the rest)."""
    B, H, W = x.shape
    HW = H * W
    src = ~((1.0 - x) > SRC_THR).reshape(B, HW)
    rank = src.cumsum(1)
    slot = torch.where(src, rank - 1, torch.full((), HW, dtype=torch.int64, device=x.device))
    table = torch.zeros((B, HW + 1), dtype=torch.int64, device=x.device)
    table.scatter_(1, slot, torch.arange(HW, device=x.device).expand(B, HW))
    return src, rank, table


def eager_forward(x, index, values):
    B, C, H, W = values.shape
    HW = H * W
    src, rank, table = rank_table(x)
    lab = index.reshape(B, HW).long()
    ok = (lab >= 1) & (lab <= rank[:, -1:])
    pix = table.gather(1, (lab - 1).clamp_(0, HW - 1))
    pixel = torch.where(ok, pix, torch.full((), -1, dtype=torch.int64, device=x.device)).to(torch.int32).reshape(B, H, W)
    got = values.reshape(B, C, HW).gather(2, pix.unsqueeze(1).expand(B, C, HW))
    return torch.where(ok.unsqueeze(1), got, torch.zeros((), device=x.device)).reshape(B, C, H, W), pixel


def eager_backward(x, index, grad):
    B, C, H, W = grad.shape
    HW = H * W
    src, rank, table = rank_table(x)
    m = rank[:, -1:]
    lab = index.reshape(B, HW).long()
    ok = (lab >= 1) & (lab <= m)
    spare = torch.full((), HW, dtype=torch.int64, device=x.device)  # the slot of what goes nowhere
    to = torch.where(ok, lab - 1, spare) + torch.arange(B, device=x.device).unsqueeze(1) * (HW + 1)
    dest = torch.where(torch.arange(HW, device=x.device).unsqueeze(0) < m, table[:, :HW], spare)
    out = torch.zeros((B, C, HW + 1), dtype=torch.float32, device=x.device)
    for c in range(C):
        sums = torch.zeros(B * (HW + 1), dtype=torch.float32, device=x.device).index_add_(0, to.reshape(-1), grad[:, c].reshape(-1))
        out[:, c].scatter_(1, dest, sums.reshape(B, HW + 1)[:, :HW])
    return out[:, :, :HW].reshape(B, C, H, W)


def frames():
    kitti = synth.make("kitti_b32_scanline")
    yield "kitti_b32_scanline", kitti, 1
    yield "kitti_b32_scanline", kitti, 3
    nyu = np.zeros((1, 240, 320), np.float32)
    rng = np.random.default_rng(7)
    at = rng.choice(240 * 320, 500, replace=False)
    nyu.reshape(-1)[at] = (np.round(rng.uniform(1, 10, 500) * 256) / 256).astype(np.float32)
    yield "nyu_240x320_500_sources", nyu, 3
    for name, (B, H, W) in (("single_source_b32_352x1216", (32, 352, 1216)), ("single_source_1_240x320", (1, 240, 320))):
        one = np.zeros((B, H, W), np.float32)
        one[:, H // 2, W // 3] = 5.0
        yield name, one, 1


def aligned(nbytes):
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


op = pkg.device.DtFill(device="cuda:0")
for name, xh, C in frames():
    B, H, W = xh.shape
    n = B * H * W
    x = torch.from_numpy(xh).to("cuda:0")
    res = op.run(x, want=("index",))
    index = res["index"].clone()
    gen = torch.Generator(device="cuda").manual_seed(B + C)
    values = torch.randn((B, C, H, W), device="cuda", generator=gen)
    grad = torch.randn((B, C, H, W), device="cuda", generator=gen)
    filled, pixel, gvals = torch.empty_like(values), torch.empty_like(index), torch.empty_like(grad)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    need_f = L.dtfill_nearest_gather_workspace_bytes(B, H, W)
    need_b = L.dtfill_nearest_gather_backward_workspace_bytes(B, H, W, C)
    ws, ws_ptr = aligned(max(need_f, need_b))
    fwd = lambda: check(L.dtfill_nearest_gather(x.data_ptr(), index.data_ptr(), values.data_ptr(), C, B, H, W, SRC_THR,
                                                filled.data_ptr(), pixel.data_ptr(), status.data_ptr(), ws_ptr, need_f, st))
    bwd = lambda: check(L.dtfill_nearest_gather_backward(x.data_ptr(), index.data_ptr(), grad.data_ptr(), C, B, H, W, SRC_THR,
                                                         gvals.data_ptr(), status.data_ptr(), ws_ptr, need_b, st))
    common = {"frames": name, "shape": [B, H, W], "C": C, "sources_per_frame": int((x >= 0.9).sum().item()) // B}

    fu, ea = compare(fwd, lambda: eager_forward(x, index, values))
    fwd()
    ef, ep = eager_forward(x, index, values)
    floor = 12 + 4 * C
    rec = dict(common, op="nearest_gather", fused=fu, eager=ea, eager_over_fused=round(ea["us"] / fu["us"], 2),
               floor_bytes_per_px=floor, gathered_bytes_per_px=4 + 4 * C, fused_GBs_vs_floor=round(floor * n / fu["us"] / 1e3, 1),
               max_abs_diff_vs_eager=(ef - filled).abs().max().item(), pixels_differing_from_eager=int((ep != pixel).sum().item()),
               status=sorted(set(status.tolist())), workspace_MiB=round(need_f / 2 ** 20, 1))
    del ef, ep
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)

    fu, ea = compare(bwd, lambda: eager_backward(x, index, grad))
    bwd()
    first = gvals.clone()
    bwd()
    eg = eager_backward(x, index, grad)
    floor = 4 + 8 * ((C + 1) // 2) + 12 * C
    rec = dict(common, op="nearest_gather_backward", fused=fu, eager=ea, eager_over_fused=round(ea["us"] / fu["us"], 2),
               floor_bytes_per_px=floor, fused_GBs_vs_floor=round(floor * n / fu["us"] / 1e3, 1),
               fused_two_calls_same_bits=bool(torch.equal(first.view(torch.int32), gvals.view(torch.int32))),
               max_abs_diff_vs_eager=(eg - gvals).abs().max().item(), max_abs_eager=eg.abs().max().item(),
               workspace_MiB=round(need_b / 2 ** 20, 1))
    del eg, first, ws
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)

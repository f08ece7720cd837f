"""Measures the backward of generate_multi_channel (dtfill_generate_multi_channel_backward: k_gmcb) on the reference's cropped
KITTI input (256 x 1216), B = 4 and B = 32, table 7, scale_num 4, 0 / 1 mask (x > 0.1) at 5 % density, every g_k given.
Per batch size, from HIP events (10 warm-up + 50 timed calls): microseconds per backward call and the achieved GB/s against the
byte floor of 16 B per pixel and step (mask or out_k + G + g_k read, one frame written); the forward call in the same run; and
torch's own backward through a literal F.unfold statement of the operator on the same device and inputs.  The two C entry
points are called directly on buffers allocated once, so a call's host side is the ctypes call alone."""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
L = pkg._lib.load()
st = torch.cuda.current_stream().cuda_stream
TS, SN, WARM, TIMED = 7, 4, 10, 50


def per_call_us(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARM):
        f()
    torch.cuda.synchronize(); e0.record()
    for _ in range(TIMED):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / TIMED * 1e3


def check(rc):
    assert rc == 0, L.dtfill_strerror(rc).decode()


def unfold_statement(d, m):
    """net.py:83-122 as it reads, on [B,H,W] tensors: extract_patches -> F.unfold."""
    w = torch.tensor([TS - abs(i - TS // 2) - abs(j - TS // 2) for i in range(TS) for j in range(TS)], dtype=d.dtype, device=d.device)[None, :, None]
    outs = [d]
    for _ in range(SN - 1):
        pd = F.unfold(d[:, None], TS, padding=TS // 2)
        s = F.unfold(m[:, None], TS, padding=TS // 2) * w
        sel = (s == s.max(dim=1, keepdim=True).values).to(d.dtype)
        d = ((pd * sel).sum(dim=1) / (0.000001 + sel.sum(dim=1))).reshape(outs[0].shape)
        m = (d > 0.001).to(d.dtype)
        outs.append(d)
    return outs


frames = synth.make("kitti_b32")[:, 96:, :].copy()
for B in (4, 32):
    x = torch.from_numpy(frames[:B]).cuda()
    m = (x > 0.1).float()
    _, H, W = x.shape
    n = B * H * W
    outs = [torch.empty_like(x) for _ in range(3)]
    fwd = lambda: check(L.dtfill_generate_multi_channel(x.data_ptr(), m.data_ptr(), B, H, W, TS, SN, *[o.data_ptr() for o in outs], st))
    fwd()
    gen = torch.Generator(device="cuda").manual_seed(B)
    gs = [torch.rand(x.shape, device="cuda", generator=gen) * 2 - 1 for _ in range(4)]
    grad = torch.empty_like(x)
    need = L.dtfill_generate_multi_channel_backward_workspace_bytes(B, H, W, SN)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    bwd = lambda: check(L.dtfill_generate_multi_channel_backward(m.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, H, W, TS, SN,
                                                                 *[g.data_ptr() for g in gs], grad.data_ptr(), ws_ptr, need, st))
    us_b, us_f = per_call_us(bwd), per_call_us(fwd)
    floor_bytes = 16 * n * (SN - 1)
    # torch's backward through the unfold statement: the graph is built once, each timed call is one backward through it
    xr = x.clone().requires_grad_(True)
    loss = sum((g * o).sum() for g, o in zip(gs, unfold_statement(xr, m)))
    tor = lambda: torch.autograd.grad(loss, xr, retain_graph=True)[0]
    us_t = per_call_us(tor)
    err = (tor() - grad).abs().max().item()  # (float32 sums in another order: close, not equal)
    del loss, xr
    torch.cuda.empty_cache()
    print(json.dumps({"op": "generate_multi_channel backward", "shape": [B, H, W], "table_size": TS, "scale_num": SN,
                      "us_backward": round(us_b, 1), "GBs_backward_vs_16B_per_px_step": round(floor_bytes / us_b / 1e3, 1),
                      "frac_of_8TBs": round(floor_bytes / us_b / 1e3 / 8000.0, 4), "us_forward": round(us_f, 1),
                      "us_torch_unfold_backward": round(us_t, 1), "torch_over_kernel": round(us_t / us_b, 1),
                      "max_abs_diff_to_torch": err}), flush=True)

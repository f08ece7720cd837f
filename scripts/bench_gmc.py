"""Measures generate_multi_channel (net.py:83-122 on the device), the three window steps of scale_num=4 on the
reference's cropped KITTI input (256x1216): frames/s and achieved GB/s against the 8 B/pixel/step it must move.  Then its
first step alone (k_gmc7), and demo.py's value-weighted form (demo.py:108-198, dtfill_demo_multi_channel) at the same shape,
plain and with a three-channel image: microseconds per step and GB/s against each step's own bytes (plain: 4 read + 4
written, 8 when the raw step is stored for a later one; image: 4 + 12 read, 16 written, + 4 likewise)."""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
x = torch.from_numpy(synth.make("kitti_b32")[:, 96:, :].copy()).cuda()
m = (x > 0.1).float()
for _ in range(5):
    pkg.device.generate_multi_channel_device(x, m)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize(); e0.record(); K = 30
for _ in range(K):
    pkg.device.generate_multi_channel_device(x, m)
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / K
B, H, W = x.shape
byt = 3 * 8 * B * H * W + 4 * B * H * W  # three steps (read data, write data) + the first step's mask read
print(json.dumps({"op": "generate_multi_channel", "shape": [B, H, W], "frames_per_s": round(B / ms * 1e3, 1),
                  "ms_per_batch": round(ms, 4), "achieved_GBs": round(byt / ms / 1e6, 1), "peak_GBs": 8000.0,
                  "frac": round(byt / ms / 1e6 / 8000.0, 4)}))


def per_call_us(f, K=30):
    for _ in range(5):
        f()
    torch.cuda.synchronize(); e0.record()
    for _ in range(K):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K * 1e3


# From here on every figure is launch against launch: the C entry points called directly on outputs and a workspace allocated
# once, outside the timed loop, so a call's host side is the ctypes call alone.
L = pkg._lib.load()
st = torch.cuda.current_stream().cuda_stream
n = B * H * W


def check(rc):
    assert rc == 0, L.dtfill_strerror(rc).decode()


# The first (non-derived) step of the net.py form alone: one k_gmc7<false> launch, the yardstick of the demo.py form's steps.
g_out = torch.empty_like(x)
us = per_call_us(lambda: check(L.dtfill_generate_multi_channel(x.data_ptr(), m.data_ptr(), B, H, W, 7, 2, g_out.data_ptr(), None,
                                                                None, st)))
print(json.dumps({"op": "generate_multi_channel first step (k_gmc7)", "shape": [B, H, W], "us": round(us, 1),
                  "GBs": round(12 * n / us / 1e3, 1)}))

# demo.py's value-weighted form (demo.py:108-198), table 7, scale_num 4, plain and with a three-channel image.  A step alone
# is a scale_num 2 call on that step's true input (the raw steps are the outputs under scale_range 1) less the out_1 pass;
# the same step storing its raw result for a later one is a scale_num 3 call less the scale_num 2 call on the next input.
raws = pkg.device.demo_multi_channel_device(x, None, 7, 1.0, 4)
rgb = torch.rand((B, H, W, 3), device=x.device) * 255.0
need = L.dtfill_demo_multi_channel_workspace_bytes(B, H, W, 4)
ws = torch.empty(need + 256, dtype=torch.uint8, device=x.device)
ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
for form, img, rd, wr in (("plain", None, 4, 4), ("image C=3", rgb, 16, 16)):
    outs = [torch.empty((B, H, W) if img is None else (B, H, W, 4), dtype=torch.float32, device=x.device) for _ in range(4)]

    def demo(src, sn):
        ptrs = [o.data_ptr() for o in outs[:sn]] + [None] * (4 - sn)
        check(L.dtfill_demo_multi_channel(src.data_ptr(), None if img is None else img.data_ptr(), 0 if img is None else 3, B, H,
                                          W, 7, sn, 90.0, *ptrs, ws_ptr, need, st))

    whole = per_call_us(lambda: demo(x, 4))
    first = per_call_us(lambda: demo(x, 1))
    rec = {"op": "demo_multi_channel " + form, "shape": [B, H, W], "table_size": 7, "us_call_scale_num_4": round(whole, 1),
           "us_out_1": round(first, 1), "GBs_out_1": round((rd + wr) * n / first / 1e3, 1)}
    two = [per_call_us(lambda k=k: demo(raws[k], 2)) for k in range(3)]
    for k in range(3):  # step k + 2 reads raw_(k+1)
        alone = two[k] - first
        rec["us_step_%d" % (k + 2)] = round(alone, 1)
        rec["GBs_step_%d" % (k + 2)] = round((rd + wr) * n / alone / 1e3, 1)
        if k < 2:
            storing = per_call_us(lambda k=k: demo(raws[k], 3)) - two[k + 1]
            rec["us_step_%d_storing_raw" % (k + 2)] = round(storing, 1)
            rec["GBs_step_%d_storing_raw" % (k + 2)] = round((rd + wr + 4) * n / storing / 1e3, 1)
    print(json.dumps(rec))

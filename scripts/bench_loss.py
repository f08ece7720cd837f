"""Measures the training losses of train.py:215-251 (dtfill_train_loss: k_loss_part + k_loss_final; dtfill_train_loss_backward:
k_loss_bwd) against the same loss and gradient written as eager torch ops, on the same tensors, on the same device, in the same
run.  Shapes: the reference's cropped KITTI frame 256 x 1216 and its NYU frame 240 x 320 (with the NYU window and root), each at
B = 2 (train.py:32's batch) and B = 32, with a correction (both gradients).

Per shape, microseconds per call from HIP events over ROUNDS rounds, fused and eager alternating within a round; a round times
enough calls to fill about 50 ms after a warm-up of the same calls.  Reported: the median and the (min .. max) spread of the
rounds, for
  forward    the two C calls on buffers allocated once  |  the eager expression under no_grad (counts stay on the device)
  backward   the C call with both gradients             |  torch.autograd.grad through the eager graph, built once
  step       autograd.train_loss(...) and .backward()   |  the eager expression and .backward(), both through torch's autograd
and the fused kernels' GB/s against the byte floors of 16 B/px (forward) and 24 B/px (backward: 16 read, 8 written).
One JSON line per shape."""
import importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
L = pkg._lib.load()
st = torch.cuda.current_stream().cuda_stream
ROUNDS, WINDOW_US = 7, 50e3
PRESETS = pkg.device.LOSS_PRESETS


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


def eager_loss(pred, corr, gt, lidar, dataset):
    """train.py:215-249 as it reads, the counts left on the device."""
    kind, gthr, ithr, rows, cols = PRESETS[dataset]
    with_gt = gt > gthr
    with_input = torch.logical_and(with_gt, lidar > ithr)
    n_gt, n_in = with_gt.sum(), with_input.sum()
    with_gt, with_input = with_gt.float(), with_input.float()
    total = (pred - gt) ** 2 * with_gt
    if dataset == "NYU":
        main = torch.sqrt(total[:, rows[0]:rows[1], cols[0]:cols[1]].sum() / n_gt)
    else:
        main = total.sum() / n_gt
    aux = ((corr - gt) ** 2 * with_input + torch.abs(corr - gt) * with_input).sum() / n_in
    return main + aux


for dataset, (H, W) in (("KITTI", (256, 1216)), ("NYU", (240, 320))):
    for B in (2, 32):
        kind, gthr, ithr, rows, cols = PRESETS[dataset]
        gen = torch.Generator(device="cuda").manual_seed(B)
        rnd = lambda: torch.rand((B, H, W), device="cuda", generator=gen)
        gt = torch.where(rnd() < 0.3, rnd() * 79 + 1, torch.zeros((), device="cuda")).contiguous()
        lidar = torch.where(rnd() < 0.2, gt, torch.zeros((), device="cuda")).contiguous()
        pred = (gt + rnd() * 8 - 4).contiguous()
        corr = (gt + rnd() * 4 - 2).contiguous()
        n = B * H * W
        r0, r1 = rows or (0, H)
        c0, c1 = cols or (0, W)
        head = (pred.data_ptr(), corr.data_ptr(), gt.data_ptr(), lidar.data_ptr(), B, H, W, kind, gthr, ithr, r0, r1, c0, c1)
        stats = torch.empty(6, dtype=torch.float64, device="cuda")
        need = L.dtfill_train_loss_workspace_bytes(B, H, W)
        ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
        g1 = torch.ones((), device="cuda")
        gp, gc = torch.empty_like(pred), torch.empty_like(pred)
        fwd = lambda: check(L.dtfill_train_loss(*head, stats.data_ptr(), ws_ptr, need, st))
        bwd = lambda: check(L.dtfill_train_loss_backward(*head, stats.data_ptr(), g1.data_ptr(), g1.data_ptr(), gp.data_ptr(), gc.data_ptr(), st))
        fwd()

        def eager_fwd():
            with torch.no_grad():
                return eager_loss(pred, corr, gt, lidar, dataset)

        pr, cr = pred.clone().requires_grad_(True), corr.clone().requires_grad_(True)
        graph = eager_loss(pr, cr, gt, lidar, dataset)
        eager_bwd = lambda: torch.autograd.grad(graph, (pr, cr), retain_graph=True)

        def fused_step():
            pr.grad = cr.grad = None
            main, aux = pkg.autograd.train_loss(pr, gt, lidar, cr, dataset=dataset)
            (main + aux).backward()

        def eager_step():
            pr.grad = cr.grad = None
            eager_loss(pr, cr, gt, lidar, dataset).backward()

        res = {"op": "train_loss", "dataset": dataset, "shape": [B, H, W]}
        for name, f, e, floor in (("forward", fwd, eager_fwd, 16 * n), ("backward", bwd, eager_bwd, 24 * n), ("step", fused_step, eager_step, 40 * n)):
            fu, ea = compare(f, e)
            res[name] = {"fused": fu, "eager": ea, "eager_over_fused": round(ea["us"] / fu["us"], 2),
                         "fused_GBs_vs_floor": round(floor / fu["us"] / 1e3, 1)}
        # the two agree: float32 sums in another order on the eager side (close, not equal)
        eg = eager_bwd()
        bwd()
        res["rel_diff_loss"] = abs((stats[0] + stats[1]).item() - graph.item()) / abs(graph.item())
        res["max_abs_diff_grads"] = max((eg[0] - gp).abs().max().item(), (eg[1] - gc).abs().max().item())
        del graph, pr, cr
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)

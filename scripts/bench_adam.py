"""Measures the optimizer step (dtfill_adam_step through optim.KerasAdam: Keras' Adam over every variable in one fused pass) on the
parameter sets of SparsityCNNTrainable, ResNet18Trainable and ResNet18LightImageTrainable, float32, built from the glorot_weights*
helpers with random gradients of the same shapes, beside torch.optim.Adam(capturable=True) in its default (foreach) form and
with fused=True where this torch build offers it -- on the same tensors' copies, on the same device, in the same run.

What the step is held against.
- Its BYTE FLOOR: 28 bytes an element, p, g, m and v read (16) and p, m and v written (12).  floor_us = read bytes / read rate +
  written bytes / store rate, the rates measured here on tensors of those very sizes by scripts/hbm_rates.py's method (torch sum
  for the read rate, fill_ for the store rate).  "abi" is the step through dtfill_adam_step alone, its argument arrays built
  once: what the device takes; "ours" is KerasAdam.step(), which reads every .grad and pointer afresh, the host's ~1 us a
  tensor included.  over_floor = abi / floor, and GBps is the 28 N bytes over abi.  The small sets lie in the caches and are
  bound by the launches, not by bytes: their GBps says so.
- torch's two forms of the same step (another rule: eps inside the bias correction; no stated bits).

The method is scripts/bench_max_pool.py's: microseconds per step from HIP events over five rounds, the candidates alternating
within a round, the median and the (min .. max) spread; the events bracket the enqueue of n steps and their run, so a form
that is bound by its host-side launches is charged for them.  One JSON line per parameter set."""
import ctypes, importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
net = importlib.import_module(pkg.__name__ + ".net")
assert torch.cuda.is_available(), "this benchmark needs the GPU"
pkg._lib.load()
optim = pkg.optim
ROUNDS, WINDOW_US = 5, 30e3
SETS = (("SparsityCNNTrainable", net.glorot_weights), ("ResNet18Trainable", net.glorot_weights_resnet18),
        ("ResNet18LightImageTrainable", net.glorot_weights_resnet18_light_image))


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


def rates(read_bytes, write_bytes):
    """(read GB/s, store GB/s) on tensors of these sizes: scripts/hbm_rates.py's sum and fill_."""
    r, w = torch.empty(read_bytes // 4, device="cuda"), torch.empty(write_bytes // 4, device="cuda")
    t = compare([lambda: r.sum(), lambda: w.fill_(1.0)])
    return read_bytes / t[0]["us"] / 1e3, write_bytes / t[1]["us"] / 1e3


def variables(weights, seed):
    """(parameters, gradients): a layer's kernel then its bias, in the weights dict's order, and random gradients of their shapes."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.from_numpy(a).cuda().requires_grad_() for layer in weights.values() for a in layer]
    return params, [torch.randn(p.shape, device="cuda", generator=gen) * 1e-2 for p in params]


def with_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g
    return params


def row(name, weights):
    params, grads = variables(weights, 1)
    n = sum(p.numel() for p in params)
    copies = lambda: with_grads([p.detach().clone().requires_grad_() for p in params], grads)
    forms = {"ours": optim.KerasAdam(with_grads(params, grads), lr=1e-6)}
    forms["torch_foreach"] = torch.optim.Adam(copies(), lr=1e-6, eps=1e-7, capturable=True)
    try:
        forms["torch_fused"] = torch.optim.Adam(copies(), lr=1e-6, eps=1e-7, capturable=True, fused=True)
        forms["torch_fused"].step()
    except Exception as e:  # this torch build has no fused Adam for this device
        forms.pop("torch_fused", None)
        fused_missing = "%s: %s" % (type(e).__name__, str(e)[:80])
    ours = forms["ours"]  # the same step through the ABI alone, its argument arrays built once: what the device takes
    n_t = len(params)
    args = ((ctypes.c_void_p * n_t)(*[p.data_ptr() for p in params]), (ctypes.c_void_p * n_t)(*[g.data_ptr() for g in grads]),
            (ctypes.c_longlong * n_t)(*[p.numel() for p in params]), n_t, ours.m.data_ptr(), ours.v.data_ptr(), ours.record.data_ptr(),
            1e-6, 0.9, 0.999, 1e-7, None)
    abi = lambda: pkg._lib.check(pkg._lib.load().dtfill_adam_step(*args))
    t = dict(zip(["abi"] + list(forms), compare([abi] + [o.step for o in forms.values()])))
    rate_r, rate_w = rates(16 * n, 12 * n)
    floor = 16 * n / rate_r / 1e3 + 12 * n / rate_w / 1e3
    out = {"op": "adam_step", "set": name, "tensors": len(params), "elements": n, "bytes": 28 * n, **t,
           "GBps": round(28 * n / t["abi"]["us"] / 1e3, 1), "read_rate_GBps": round(rate_r, 1), "store_rate_GBps": round(rate_w, 1),
           "floor_us": round(floor, 2), "over_floor": round(t["abi"]["us"] / floor, 2),
           "foreach_over_ours": round(t["torch_foreach"]["us"] / t["ours"]["us"], 2)}
    if "torch_fused" in t:
        out["fused_over_ours"] = round(t["torch_fused"]["us"] / t["ours"]["us"], 2)
    else:
        out["torch_fused"] = "not offered (%s)" % fused_missing
    print(json.dumps(out), flush=True)


for name, make in SETS:
    row(name, make(0, 4, True, bias=0.1))
    torch.cuda.empty_cache()

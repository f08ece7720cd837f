"""The Python layer from several host threads and on several streams at once.

The C ABI keeps nothing between calls; the Python layer caches an operator, its buffers and the backward workspaces, and these
tests hold that cache to the ABI's promise: the reference-named numpy functions from four threads, the autograd operators from
four threads on one stream, two streams released together by an event, and an operator used off the stream that allocated its
buffers.  Every result is compared bit for bit with an expectation computed before any thread starts: the oracle for the fill,
tests/near_ref.py, fill_grad_ref.py, gmc_grad_ref.py and loss_ref.py for the rest.  tests/test_concurrent_harness.py shows on the
CPU that the harness sees a shared staging buffer.

Sizes.  The numpy functions and the two-stream forwards run on [8,352,1216] (a pass stages 13.7 MB: the staging copy and the DMA
take long enough to overlap); the gradients on [4,128,640].  fill_grad_ref's cell sum is exact Python-integer arithmetic, a few
microseconds per non-zero term, so the upstream gradients here are non-zero on one pixel in 32 (as a loss masked by a sparse ground
truth is): every cell still receives terms from many strips and blocks, and the reference stays under a second per case.  The
backward wrappers of the two-stream test run on the same [4,128,640] cases for that reason: there the overlap comes from the
event that releases both streams, not from the size.
"""
import functools

import numpy as np
import pytest

import concurrency
import fill_grad_ref as G
import gmc_grad_ref as GM
import loss_ref as LR
import near_ref as N
from guarded import poison_op
from helpers import dt_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
WORKERS, ROUNDS = 4, 10
KITTI = (8, 352, 1216)
SMALL = (4, 128, 640)
PAYLOAD_BITS = np.array([0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def nan_bits_match(got, want):
    """Bit for bit, a NaN matching a NaN (the cell sum's NaN is the one quiet NaN of the contract)."""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan],
                                                                                             want.view(np.uint32)[~nan])


def frames(seed, shape, p, sky=0):
    """Seeded frames with a fraction p of depths in [1, 80) and `sky` empty rows on top."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(shape) < p, rng.uniform(1, 80, shape), 0).astype(F)
    x[:, :sky] = 0
    return x


def payload(seed, shape):
    """Seeded float32 channels with the bit patterns a copy must carry through."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-100, 100, shape).astype(F)
    flat = v.reshape(-1)
    flat[rng.permutation(flat.size)[:PAYLOAD_BITS.size]] = PAYLOAD_BITS.view(F)
    return v


def sparse_gradient(seed, shape):
    """fill_grad_ref.random_gradient (40 binades, planted zeros, subnormals, non-finite values, cancelling pairs) on one pixel in
    32 and wherever it is not finite, +0.0 elsewhere."""
    rng = np.random.default_rng(seed)
    g = G.random_gradient(rng, shape)
    return np.where((rng.random(shape) < 1 / 32) | ~np.isfinite(g), g, F(0)).astype(F)


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def torch_gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared cases are read-only)


def blocker(torch, stream, n=16):
    """A few milliseconds of plain torch work on `stream` (a chain of 4096 x 4096 float32 products), then an event."""
    with torch.cuda.stream(stream):
        a = torch.full((4096, 4096), 1.0 / 4096, device=DEV)
        b = a
        for _ in range(n):
            b = torch.mm(a, b)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev, b


_streams = []


def two_streams(torch):
    """Streams A and B of this module (the same two throughout: the product keeps an operator per stream)."""
    if not _streams:
        _streams.extend(torch.cuda.Stream(device=DEV) for _ in range(2))
    return _streams


def released_together(torch, on_a, on_b):
    """on_a() on stream A behind a blocker, on_b() on stream B behind the blocker's event: both are queued before either
    starts.  Returns (on_a's result, on_b's result) once the default stream has waited for both streams' events: the caller
    reads on the default stream, never through its implicit ordering."""
    A, B = two_streams(torch)
    for s, f in ((A, on_a), (B, on_b)):  # the per-stream operator, its workspace and the allocator's pools exist
        with torch.cuda.stream(s):
            f()
    torch.cuda.synchronize()
    ev, keep = blocker(torch, A)
    B.wait_event(ev)
    with torch.cuda.stream(A):
        ra = on_a()
        done_a = torch.cuda.Event()
        done_a.record(A)
    with torch.cuda.stream(B):
        rb = on_b()
        done_b = torch.cuda.Event()
        done_b.record(B)
    queued_first = not ev.query()
    here = torch.cuda.current_stream()
    here.wait_event(done_a)
    here.wait_event(done_b)
    assert queued_first, "the blocker ended before both passes were queued: nothing overlapped"
    return ra, rb, keep


# ---------------------------------------------------------------- 1: the numpy functions from threads, one shape

@functools.lru_cache(maxsize=None)
def kitti_case(k):
    """Thread k's frames [8,352,1216] and what the reference gives for every call of the round.  5 %, 1.2 %, 0.05 %, and 5 % under
    a 120-row sky: four different routes through the kernels, four different sets of flags in a workspace."""
    from oracle import oracle as O

    p, sky = ((0.05, 0), (0.012, 0), (0.0005, 0), (0.05, 120))[k]
    x = frames(100 + k, KITTI, p, sky)
    depth, dt, lbl, status = O.fill_batch(x)
    assert not status.any()
    c = dict(x=x, depth=depth[..., None], crop=O.depth_floor(depth[:, 96:], 0.9)[..., None], dt=dt, lbl=lbl)
    # the filter in front of the fill on two frames: another shape through the same operator
    c["removal"] = O.fill_batch(np.stack([O.outlier_removal(f) for f in x[:2]]).astype(F))[0][..., None]
    c["one"] = O.Distance_Transform(x[k + 1])  # eval_NYU.py's thresholds 0.001 / 0.1
    # a batch of two whose second frame has fewer values than sources under val_thr = 2.0: numpy's IndexError
    xm = x[:2].copy()
    xm[0][(xm[0] > 0) & (xm[0] <= 2.5)] = 3
    assert O.fill_batch(xm, 0.1, 2.0)[3].tolist() == [0, 1]
    c["misaligned"] = xm
    c["misaligned_depth0"] = O.fill_batch(xm[:1], 0.1, 2.0)[0][..., None]
    return frozen(c)


def test_numpy_functions_from_threads_one_shape(pkg, torch_gpu):
    """DT_complete_batch (plain, cropped and floored, with the outlier filter), nearest_point and Distance_Transform from four
    threads for ten rounds, every thread on frames of its own; thread 2 also owns the batch that raises IndexError."""
    cases = [kitti_case(k) for k in range(WORKERS)]
    op = pkg.device.default_op()
    pkg.DT_complete_batch(cases[0]["x"][..., None])  # the operator's buffers exist: poison_op has something to poison

    def work(k, r):
        c = cases[k]
        x4 = c["x"][..., None]
        with op._lock:  # (between two passes, not in the middle of another thread's)
            poison_op(op, 4 * r + k, kind=("zero", "ones")[(r + k) % 2])
        assert same_bits(pkg.DT_complete_batch(x4), c["depth"]), "DT_complete_batch"
        assert same_bits(pkg.DT_complete_batch(x4, first_row=96, floor=0.9), c["crop"]), "first_row, floor"
        dt, lbl = pkg.nearest_point(c["x"][k])
        assert same_bits(dt, c["dt"][k]) and same_bits(lbl, c["lbl"][k]), "nearest_point"
        assert same_bits(pkg.DT_complete_batch(x4[:2], if_removal=True), c["removal"]), "if_removal"
        assert same_bits(pkg.Distance_Transform(c["x"][k + 1]), c["one"]), "Distance_Transform"
        if k == 2:
            with pytest.raises(IndexError, match="frame 1"):
                pkg.DT_complete_batch(c["misaligned"][..., None], val_thr=2.0)
            assert same_bits(pkg.DT_complete_batch(c["misaligned"][:1, ..., None], val_thr=2.0), c["misaligned_depth0"])

    failures = concurrency.run_rounds(work, WORKERS, ROUNDS)
    assert not failures, concurrency.describe(failures)


# ---------------------------------------------------------------- 2: different shapes and metrics

@functools.lru_cache(maxsize=None)
def mixed_case(k):
    """Thread k's frames (4, 100 + 10 k, 300 + 7 k): k = 0, 1 for nearest_source(metric="l2") with three channels, k = 2, 3 for
    DT_complete_batch and device.fill(metric="l1_cv")."""
    from oracle import oracle as O

    shape = (4, 100 + 10 * k, 300 + 7 * k)
    x = frames(200 + k, shape, (0.05, 0.004, 0.05, 0.004)[k], sky=(0, 30, 0, 30)[k])
    if k < 2:
        _, dt, index, _ = O.fill_batch(x, metric="l2")
        values = payload(210 + k, (4, 3) + shape[1:])
        filled, pixel, status = N.gather(x, index, values)
        assert not status.any()
        return frozen(dict(x=x, values=values, dt=dt, pixel=pixel, filled=filled))
    depth, dt, index, status = O.fill_batch(x)
    return frozen(dict(x=x, depth=depth, dt=dt, index=index, status=status))


def test_numpy_functions_from_threads_shapes_and_metrics(pkg, torch_gpu):
    cases = [mixed_case(k) for k in range(WORKERS)]

    def work(k, r):
        c = cases[k]
        if k < 2:
            dt, pixel, filled = pkg.nearest_source(np.array(c["x"]), values=np.array(c["values"]), metric="l2")
            assert np.array_equal(dt_bits(dt), dt_bits(c["dt"])), "nearest_source: dt"
            assert same_bits(pixel, c["pixel"]), "nearest_source: pixel"
            assert same_bits(filled, c["filled"]), "nearest_source: filled"
        else:
            assert same_bits(pkg.DT_complete_batch(c["x"][..., None]), c["depth"][..., None]), "DT_complete_batch"
            got = pkg.device.fill(c["x"], metric="l1_cv")
            for name, key in (("depth", "depth"), ("dt", "dt"), ("index", "index")):
                assert same_bits(got[name], c[key]), "fill: " + name
            assert np.array_equal(got["status"] & 1, c["status"]), "fill: status"

    failures = concurrency.run_rounds(work, WORKERS, ROUNDS)
    assert not failures, concurrency.describe(failures)


# ---------------------------------------------------------------- 3: the autograd operators from threads, one stream

@functools.lru_cache(maxsize=None)
def fill_case(k):
    """autograd.fill on [4,128,640], input k: forward by the oracle in both metrics, gradient by fill_grad_ref (l2 for k = 0
    only)."""
    from oracle import oracle as O

    x = frames(300 + k, SMALL, (0.05, 0.01, 0.002, 0.05)[k], sky=(0, 0, 0, 40)[k])
    w = sparse_gradient(310 + k, SMALL)
    c = dict(x=x, w=w)
    for metric in ("l1_cv", "l2") if k == 0 else ("l1_cv",):
        depth, dt, index, status = O.fill_batch(x, metric=metric)
        assert not status.any()
        grad_x, st = G.backward(x, index, w)
        assert not st.any()
        c[metric] = frozen(dict(depth=depth, dt=dt, index=index, grad_x=grad_x))
    return frozen(c)


@functools.lru_cache(maxsize=None)
def values_case(C):
    """fill_values on [4,128,640] with C channels: near_ref's gather and backward on the oracle's labels."""
    from oracle import oracle as O

    x = frames(320 + C, SMALL, 0.02)
    _, dt, index, _ = O.fill_batch(x)
    values = payload(321 + C, (4, C) + SMALL[1:])
    w = sparse_gradient(322 + C, values.shape)
    filled, pixel, status = N.gather(x, index, values)
    grad_values, st = N.backward(x, index, w)
    assert not status.any() and not st.any()
    return frozen(dict(x=x, values=values, w=w, dt=dt, index=index, filled=filled, pixel=pixel, grad_values=grad_values))


@functools.lru_cache(maxsize=None)
def gmc_case(k):
    """generate_multi_channel (7, 4) on [4,128,640]: forward by the oracle (the device's own operations in the same order),
    gradient by gmc_grad_ref."""
    from oracle import oracle as O

    rng = np.random.default_rng(330 + k)
    data = frames(331 + k, SMALL, (0.05, 0.02)[k])
    mask = (data > F(0.1)).astype(F)
    outs = [np.asarray(o, F) for o in O.generate_multi_channel(data, mask, 7, 4)]
    gs = [rng.uniform(-2, 2, SMALL).astype(F) for _ in range(4)]
    grad = GM.backward(mask, outs[1], outs[2], 7, 4, gs)
    return frozen(dict(data=data, mask=mask, out2=outs[1], out3=outs[2], out4=outs[3], g1=gs[0], g2=gs[1], g3=gs[2], g4=gs[3],
                       grad=grad))


@functools.lru_cache(maxsize=None)
def loss_case():
    """train_loss with a correction (KITTI) on [4,128,640]: the gradients of main + aux depend on the exact counts alone, so
    they are the reference's bits; main and aux are sums in double, within (n + 2) 2^-53 of the reference's exact ones
    (tests/test_gpu_train_loss.py, check_stats) before their one rounding to float32."""
    rng = np.random.default_rng(340)
    pred, gt, lidar, corr = LR.make_case(rng, SMALL)
    stats, nterms = LR.forward(pred, gt, lidar, corr)
    grad_pred, grad_corr = LR.backward(pred, gt, stats, F(1), F(1), lidar, corr)
    return frozen(dict(pred=pred, gt=gt, lidar=lidar, corr=corr, stats=stats, nterms=nterms, grad_pred=grad_pred,
                       grad_corr=grad_corr))


def loss_value_ok(got, want, n):
    """A float32 `got` rounded from a double within (n + 2) 2^-53 relative of `want`."""
    got, want = float(got), float(want)
    return abs(got - want) <= (n + 2) * 2.0 ** -53 * abs(want) + 2.0 ** -24 * abs(got)


def fill_step(pkg, torch, c, metric):
    e = c[metric]
    x = dev(torch, c["x"]).requires_grad_(True)
    w = dev(torch, c["w"])
    depth, dt, index, status = pkg.autograd.fill(x, metric=metric)
    (depth * w).sum().backward()
    got = [t.detach().cpu().numpy() for t in (depth, dt, index, status, x.grad)]
    assert same_bits(got[0], e["depth"]), metric + ": depth"
    assert np.array_equal(dt_bits(got[1]), dt_bits(e["dt"])) and same_bits(got[2], e["index"]), metric + ": dt, index"
    assert not (got[3] & 1).any(), metric + ": status"
    assert nan_bits_match(got[4], e["grad_x"]), metric + ": x.grad"


def values_step(pkg, torch, c):
    x = dev(torch, c["x"])
    v = dev(torch, c["values"]).requires_grad_(True)
    w = dev(torch, c["w"])
    filled, dt, index, pixel, status = pkg.autograd.fill_values(x, v)
    (filled * w).sum().backward()
    got = [t.detach().cpu().numpy() for t in (filled, dt, index, pixel, status, v.grad)]
    assert same_bits(got[0], c["filled"]), "fill_values: filled"
    assert same_bits(got[1], c["dt"]) and same_bits(got[2], c["index"]) and same_bits(got[3], c["pixel"]), "fill_values: maps"
    assert not got[4].any(), "fill_values: status"
    assert nan_bits_match(got[5], c["grad_values"]), "fill_values: values.grad"


def gmc_step(pkg, torch, c):
    data = dev(torch, c["data"]).requires_grad_(True)
    lidar = pkg.autograd.generate_multi_channel(data, dev(torch, c["mask"]), 7, 4)
    sum((dev(torch, c["g%d" % (k + 1)]) * lidar[k]).sum() for k in range(4)).backward()
    for k, name in ((1, "out2"), (2, "out3"), (3, "out4")):
        assert same_bits(lidar[k].detach().cpu().numpy(), c[name]), "generate_multi_channel: lidar_%d" % (k + 1)
    GM.assert_same(data.grad.cpu().numpy(), c["grad"], "generate_multi_channel: data.grad")


def loss_step(pkg, torch, c):
    pred, gt, lidar, corr = (dev(torch, c[k]) for k in ("pred", "gt", "lidar", "corr"))
    pred.requires_grad_(True), corr.requires_grad_(True)
    main, aux = pkg.autograd.train_loss(pred, gt, lidar, corr)
    (main + aux).backward()
    assert loss_value_ok(main.item(), c["stats"][0], c["nterms"][0]), "train_loss: main"
    assert loss_value_ok(aux.item(), c["stats"][1], c["nterms"][1]), "train_loss: aux"
    assert same_bits(pred.grad.cpu().numpy(), c["grad_pred"]), "train_loss: pred.grad"
    assert same_bits(corr.grad.cpu().numpy(), c["grad_corr"]), "train_loss: correction.grad"


def test_autograd_operators_from_threads(pkg, torch_gpu):
    """fill (both metrics), fill_values (C = 3), generate_multi_channel (7, 4) and train_loss, each forward and backward, from
    four threads on the default stream."""
    torch = torch_gpu
    f, v, g, l = fill_case(0), values_case(3), gmc_case(0), loss_case()

    def work(k, r):
        if k == 0:
            fill_step(pkg, torch, f, "l1_cv")
            fill_step(pkg, torch, f, "l2")
        elif k == 1:
            values_step(pkg, torch, v)
        elif k == 2:
            gmc_step(pkg, torch, g)
        else:
            loss_step(pkg, torch, l)

    failures = concurrency.run_rounds(work, WORKERS, ROUNDS)
    assert not failures, concurrency.describe(failures)


def test_one_autograd_operator_from_four_threads(pkg, torch_gpu):
    """The worst case for a shared workspace: all four threads in autograd.fill, different inputs of one shape."""
    torch = torch_gpu
    cases = [fill_case(k) for k in range(WORKERS)]

    def work(k, r):
        fill_step(pkg, torch, cases[k], "l1_cv")

    failures = concurrency.run_rounds(work, WORKERS, ROUNDS)
    assert not failures, concurrency.describe(failures)


# ---------------------------------------------------------------- 4: two streams released together, one host thread

@functools.lru_cache(maxsize=None)
def stream_case(metric):
    """x1 dense, x2 sparse under a sky, [8,352,1216], and the oracle's outputs."""
    from oracle import oracle as O

    xs = frames(400, KITTI, 0.05), frames(401, KITTI, 0.0005, sky=120)
    return tuple(frozen(dict(x=x, out=O.fill_batch(x, metric=metric))) for x in xs)


@pytest.mark.parametrize("metric", ("l1_cv", "l2"))
def test_two_streams_fill(pkg, torch_gpu, metric):
    torch = torch_gpu
    c1, c2 = stream_case(metric)
    x1, x2 = dev(torch, c1["x"]), dev(torch, c2["x"])
    ra, rb, _ = released_together(torch, lambda: pkg.autograd.fill(x1, metric=metric), lambda: pkg.autograd.fill(x2, metric=metric))
    for got, c, what in ((ra, c1, "stream A"), (rb, c2, "stream B")):
        depth, dt, index, status = (t.cpu().numpy() for t in got)
        wd, wdt, wi, ws = c["out"]
        assert same_bits(depth, wd) and same_bits(index, wi), what
        assert np.array_equal(dt_bits(dt), dt_bits(wdt)) and np.array_equal(status & 1, ws), what
    torch.cuda.synchronize()


def test_two_streams_fill_values(pkg, torch_gpu):
    torch = torch_gpu
    cases = stream_case("l1_cv")
    vals = [payload(410 + k, (KITTI[0], 3) + KITTI[1:]) for k in range(2)]
    want = [N.gather(c["x"], c["out"][2], v) for c, v in zip(cases, vals)]
    xs = [dev(torch, c["x"]) for c in cases]
    vs = [dev(torch, v) for v in vals]
    ra, rb, _ = released_together(torch, lambda: pkg.autograd.fill_values(xs[0], vs[0]), lambda: pkg.autograd.fill_values(xs[1], vs[1]))
    for got, c, (filled, pixel, status), what in ((ra, cases[0], want[0], "stream A"), (rb, cases[1], want[1], "stream B")):
        g = [t.cpu().numpy() for t in got]
        assert same_bits(g[0], filled) and same_bits(g[3], pixel) and np.array_equal(g[4], status), what
        assert same_bits(g[1], c["out"][1]) and same_bits(g[2], c["out"][2]), what
    torch.cuda.synchronize()


def test_two_streams_backward_wrappers(pkg, torch_gpu):
    """fill_backward_device, nearest_gather_backward_device and generate_multi_channel_backward_device, each on two streams
    released together, on the [4,128,640] cases of the thread tests."""
    torch = torch_gpu
    D = pkg.device
    fa, fb = fill_case(0), fill_case(3)
    args = [[dev(torch, a) for a in (c["x"], c["l1_cv"]["index"], c["w"])] for c in (fa, fb)]
    ra, rb, _ = released_together(torch, lambda: D.fill_backward_device(*args[0]), lambda: D.fill_backward_device(*args[1]))
    for (gx, st), c, what in ((ra, fa, "fill A"), (rb, fb, "fill B")):
        assert nan_bits_match(gx.cpu().numpy(), c["l1_cv"]["grad_x"]) and not st.cpu().numpy().any(), what

    va, vb = values_case(3), values_case(1)
    args = [[dev(torch, a) for a in (c["x"], c["index"], c["w"])] for c in (va, vb)]
    ra, rb, _ = released_together(torch, lambda: D.nearest_gather_backward_device(*args[0]),
                                  lambda: D.nearest_gather_backward_device(*args[1]))
    for (gv, st), c, what in ((ra, va, "gather A"), (rb, vb, "gather B")):
        assert nan_bits_match(gv.cpu().numpy(), c["grad_values"]) and not st.cpu().numpy().any(), what

    ga, gb = gmc_case(0), gmc_case(1)
    args = [[dev(torch, c[k]) for k in ("mask", "out2", "out3", "g1", "g2", "g3", "g4")] for c in (ga, gb)]
    call = lambda a: D.generate_multi_channel_backward_device(a[0], a[1], a[2], a[3:], 7, 4)
    ra, rb, _ = released_together(torch, lambda: call(args[0]), lambda: call(args[1]))
    GM.assert_same(ra.cpu().numpy(), ga["grad"], "gmc A")
    GM.assert_same(rb.cpu().numpy(), gb["grad"], "gmc B")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5: an operator off its allocating stream

def test_operator_off_its_allocating_stream(pkg, torch_gpu):
    """A DtFill whose buffers were allocated under stream A runs under stream B behind a blocker and is dropped while that
    pass is queued; stream A at once allocates tensors of the workspace's and the outputs' sizes and keeps writing to them.
    B's results (in the test's own tensors, and the cropped depth, which is the operator's, copied on B) equal the oracle."""
    from oracle import oracle as O

    torch = torch_gpu
    c1, c2 = stream_case("l1_cv")
    x1, x2 = dev(torch, c1["x"]), dev(torch, c2["x"])
    A, B = two_streams(torch)
    out = dict(depth=torch.empty_like(x2), dt=torch.empty_like(x2), index=torch.empty_like(x2, dtype=torch.int32),
               status=torch.empty((KITTI[0],), dtype=torch.int32, device=DEV))
    out2 = dict(dt=torch.empty_like(x2), index=torch.empty_like(x2, dtype=torch.int32))
    op = pkg.device.DtFill(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        op.run(x1)  # every buffer of the operator is allocated under A
        op.run(x1, depth_rows_from=96, depth_floor=0.9)
        poison_op(op, 1, kind="ones")
    A.synchronize()
    sizes = [op._ws.numel()] + [t.numel() * t.element_size() for t in op._out.values()] + [op._crop.numel() * 4]
    ev, keep = blocker(torch, B)
    with torch.cuda.stream(B):
        op.run(x2, out=out)
        crop = op.run(x2, want=("depth", "dt", "index"), depth_rows_from=96, depth_floor=0.9, out=out2)["depth"].clone()
        done = torch.cuda.Event()
        done.record(B)
    del op
    with torch.cuda.stream(A):
        mine = [torch.empty(n, dtype=torch.uint8, device=DEV) for n in sizes]  # (the allocator decides here, on the host)
        A.wait_event(ev)  # released with B's passes: stream A writes while they run
        for k in range(24):
            for t in mine:
                t.fill_(0xFF if k % 2 else 0x00)
    queued_first = not ev.query()
    A.synchronize()
    B.synchronize()
    assert queued_first, "the blocker ended before stream A's writes were queued: nothing overlapped"
    wd, wdt, wi, ws = c2["out"]
    assert same_bits(out["depth"].cpu().numpy(), wd) and same_bits(out["index"].cpu().numpy(), wi)
    assert same_bits(out["dt"].cpu().numpy(), wdt) and np.array_equal(out["status"].cpu().numpy() & 1, ws)
    assert same_bits(crop.cpu().numpy(), O.depth_floor(wd[:, 96:], 0.9))
    assert same_bits(out2["index"].cpu().numpy(), wi) and same_bits(out2["dt"].cpu().numpy(), wdt)

"""dtfill_train_loss / dtfill_train_loss_backward (k_loss_part, k_loss_final, k_loss_bwd) on the device against the literal
reference of tests/loss_ref.py, and the autograd operator built on them.

Through the raw ABI every buffer is a guarded allocation; outputs, stats and the workspace are poisoned first and the inputs
must come back unchanged.  Every case runs with its payloads 4 bytes after a 256-byte boundary (the dword loads) and again on
the boundary (the 16-byte loads where B*H*W is a multiple of 4): include/dtfill.h makes the bits a function of the shape alone,
so the two must agree bit for bit.  The shapes: one pixel; 2 x 5 x 37 (odd, one partial chunk); 2 x 9 x 11 with the window
[2,7) x [3,10); 2 x 240 x 320 with the NYU window (150 chunks, one per block); 2 x 724 x 728 = 1024 * 1024 + 5568 elements:
1030 chunks of 1024 on 1024 blocks, so six blocks make a second trip and the last of them a partial one.
The inputs (loss_ref.make_case) make every term zero or a normal float32, so the device's float32 terms are numpy's."""
import numpy as np
import pytest

import loss_ref as R
from guarded import GuardedBuffer, is_poison, poison, poison_value, KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
G_MAIN, G_AUX = F(0.75), F(-1.5)
# name -> (shape, dataset, rows, cols)
CASES = {
    "1x1x1": ((1, 1, 1), "KITTI", None, None),
    "2x5x37": ((2, 5, 37), "KITTI", None, None),
    "2x9x11-window": ((2, 9, 11), "NYU", (2, 7), (3, 10)),
    "2x240x320-nyu": ((2, 240, 320), "NYU", None, None),
    "2x724x728-two-trips": ((2, 724, 728), "KITTI", None, None),
    "2x5x37-empty-mask": ((2, 5, 37), "NYU", (0, 5), (0, 37)),
}
_cache = {}


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def case(name):
    """The inputs and the reference's forward for one case, computed once and shared (nobody writes to them)."""
    if name in _cache:
        return _cache[name]
    shape, dataset, rows, cols = CASES[name]
    kind, gthr, ithr, prows, pcols = R.PRESETS[dataset]
    rows, cols = rows or prows, cols or pcols
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "1x1x1":
        pred, gt, lidar, corr = (np.full(shape, v, F) for v in (3, 2, 2, 2.5))
    else:
        pred, gt, lidar, corr = R.make_case(rng, shape, nyu=dataset == "NYU")
    if name.endswith("empty-mask"):
        gt[gt > 0] = 0
    if rows is not None and not name.endswith("empty-mask"):
        # gt-valid pixels outside the window: counted, not summed, and a non-finite prediction there leaves no trace
        gt[:, 0, 0], pred[:, 0, 0], lidar[:, 0, 0] = 10, np.inf, 0
        gt[0, -1, -1], pred[0, -1, -1], lidar[0, -1, -1] = 10, np.nan, 0
    c = dict(name=name, shape=shape, kind=kind, gthr=gthr, ithr=ithr, rows=rows, cols=cols, pred=pred, gt=gt, lidar=lidar, corr=corr)
    kw = dict(kind=kind, gt_thr=gthr, in_thr=ithr, rows=rows, cols=cols)
    c["kw"] = kw
    c["stats"], c["nterms"] = R.forward(pred, gt, lidar, corr, **kw)
    c["stats_main_only"], _ = R.forward(pred, gt, None, None, **kw)
    for a in (pred, gt, lidar, corr):
        a.setflags(write=False)
    _cache[name] = c
    return c


def _window(c):
    B, H, W = c["shape"]
    return (c["rows"] or (0, H)) + (c["cols"] or (0, W))


def _guarded(a, offset):
    import torch

    g = GuardedBuffer(a.nbytes, offset, DEV, frame_bytes=a[0].nbytes)
    g.view(torch.float32, a.shape).copy_(torch.from_numpy(np.array(a)))  # (a copy: the shared case is read-only)
    return g


class Device:
    """The four inputs of a case in guarded buffers at `offset`, and the two entry points on them."""

    def __init__(self, L, c, offset, aux=True):
        self.L, self.c, self.offset, self.aux = L, c, offset, aux
        self.names = ("pred", "corr", "gt", "lidar")
        self.bufs = {k: _guarded(c[k], offset) if (aux or k in ("pred", "gt")) else None for k in self.names}
        B, H, W = c["shape"]
        self.need = L.dtfill_train_loss_workspace_bytes(B, H, W)
        assert 0 < self.need <= 64 << 10
        self.ws = GuardedBuffer(self.need, 0, DEV, frame_bytes=H * W * 4)
        self.head = [None if self.bufs[k] is None else self.bufs[k].ptr for k in self.names] + [B, H, W, c["kind"], c["gthr"], c["ithr"], *_window(c)]
        self.guards = [b for b in self.bufs.values() if b is not None] + [self.ws]
        self.calls = 0

    def forward(self, stream=None):
        """One dtfill_train_loss call into a fresh, poisoned stats buffer; returns that GuardedBuffer (not yet synchronised)."""
        import torch

        stats = GuardedBuffer(6 * 8, 0, DEV)
        poison(stats.payload(), "ones")
        poison(self.ws.payload(), KINDS[self.calls % 3], 77 + self.calls)
        self.calls += 1
        torch.cuda.synchronize()  # the poison is in place before a call on another stream
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = self.L.dtfill_train_loss(*self.head, stats.ptr, self.ws.ptr, self.need, st)
        assert rc == 0, self.c["name"] + ": " + self.L.dtfill_strerror(rc).decode()
        self.guards.append(stats)
        return stats

    def backward(self, stats, g_main, g_aux, want_pred=True, want_corr=True):
        """One dtfill_train_loss_backward call; g_*: a float32 value or None (a NULL pointer).  Returns (grad_pred, grad_corr)
        as numpy, None for one not asked for, after checking that no poison is left."""
        import torch

        shape = self.c["shape"]
        B, H, W = shape
        gs = [None if g is None else torch.tensor([g], dtype=torch.float32, device=DEV) for g in (g_main, g_aux)]
        outs = [GuardedBuffer(B * H * W * 4, self.offset, DEV, frame_bytes=H * W * 4) if want else None for want in (want_pred, want_corr)]
        for o in outs:
            if o is not None:
                o.view(torch.int32, shape).fill_(int(poison_value("depth").view(np.int32)))
        rc = self.L.dtfill_train_loss_backward(*self.head, stats.ptr, *[None if g is None else g.data_ptr() for g in gs],
                                               *[None if o is None else o.ptr for o in outs], torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.c["name"] + ": " + self.L.dtfill_strerror(rc).decode()
        torch.cuda.synchronize()
        got = []
        for o in outs:
            if o is None:
                got.append(None)
                continue
            o.check(self.c["name"] + " gradient")
            got.append(o.view(torch.float32, shape).cpu().numpy())
            assert not is_poison(got[-1], "depth").any(), self.c["name"] + ": a gradient keeps poison"
        return got

    def finish(self):
        """Synchronise, check every guard, and that the inputs are what they were."""
        import torch

        torch.cuda.synchronize()
        for k, g in enumerate(self.guards):
            g.check("%s buffer %d" % (self.c["name"], k))
        for k in self.names:
            if self.bufs[k] is not None:
                now = self.bufs[k].view(torch.float32, self.c["shape"]).cpu().numpy()
                assert np.array_equal(now.view(np.uint32), self.c[k].view(np.uint32)), "%s: %s changed" % (self.c["name"], k)


def read_stats(buf):
    import torch

    return buf.view(torch.float64, (6,)).cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_stats(got, want, nterms, what):
    """n_gt and n_in exact; a sum of n non-negative float32 terms, added in double in any order, is within n * 2^-53 relative
    of their exact sum (fsum); main and aux carry a division and a root on top: (n + 2) * 2^-53."""
    print("%s: got %s want %s" % (what, got.tolist(), want.tolist()))
    assert got[2] == want[2] and got[3] == want[3], what + ": counts"
    for col, n, extra in ((4, nterms[0], 0), (5, nterms[1], 0), (0, nterms[0], 2), (1, nterms[1], 2)):
        if np.isnan(want[col]):
            assert np.isnan(got[col]), (what, R.COLUMNS[col])
        else:
            assert abs(got[col] - want[col]) <= (n + extra) * 2.0 ** -53 * abs(want[col]), (what, R.COLUMNS[col], got[col], want[col])
    assert not np.signbit(got[2:]).any()


@pytest.mark.parametrize("name", list(CASES))
def test_forward(L, name):
    import torch

    c = case(name)
    runs = []
    for offset in (4, 0):
        d = Device(L, c, offset)
        bufs = [d.forward(), d.forward()]  # two calls, the workspace poisoned differently in front of each
        torch.cuda.synchronize()
        bufs.append(d.forward(torch.cuda.Stream()))  # and one on a second stream
        d.finish()
        stats = [read_stats(b) for b in bufs]
        check_stats(stats[0], c["stats"], c["nterms"], "%s offset %d" % (name, offset))
        assert same_bits(stats[0], stats[1]) and same_bits(stats[0], stats[2]), name + ": two calls differ"
        runs.append(stats[0])
    assert same_bits(runs[0], runs[1]), name + ": alignment changes the bits"
    # without a correction: aux, n_in and S_aux are +0, and neither corr nor lidar exists to be read
    for offset in (4, 0):
        d = Device(L, c, offset, aux=False)
        buf = d.forward()
        d.finish()
        got = read_stats(buf)
        check_stats(got, c["stats_main_only"], (c["nterms"][0], 0), "%s main only offset %d" % (name, offset))
        assert not got[[1, 3, 5]].view(np.uint64).any()
        assert same_bits(got[[0, 2, 4]], runs[0][[0, 2, 4]])


@pytest.mark.parametrize("name", list(CASES))
def test_backward(L, name):
    """Bit for bit: k depends on the exact counts and g alone (KITTI), and for NYU on the main the forward wrote, which
    test_forward pins; the reference is evaluated with that main."""
    c = case(name)
    B, H, W = c["shape"]
    for offset in (4, 0):
        d = Device(L, c, offset)
        sbuf = d.forward()
        dstats = read_stats(sbuf)
        rstats = dstats if c["kind"] == R.NYU else c["stats"]
        ins = (c["pred"], c["gt"])
        variants = (  # g_main, g_aux, want_pred, want_corr
            (G_MAIN, G_AUX, True, True), (None, G_AUX, True, True), (G_MAIN, None, True, True), (G_MAIN, G_AUX, True, False),
            (G_MAIN, G_AUX, False, True), (None, None, True, True))
        for gm, ga, wp, wc in (variants if offset else variants[:1]):  # (the 16-byte path: both gradients once)
            got = d.backward(sbuf, gm, ga, wp, wc)
            want = R.backward(*ins, rstats, gm, ga, c["lidar"], c["corr"], **c["kw"])
            what = "%s offset %d g_main %s g_aux %s pred %s corr %s" % (name, offset, gm, ga, wp, wc)
            for g, w_, asked in zip(got, want, (wp, wc)):
                assert (g is not None) == asked
                if asked:
                    assert same_bits(g, w_), what + ": %d of %d differ" % ((g.view(np.uint32) != w_.view(np.uint32)).sum(), g.size)
        # unselected pixels are +0 by bit pattern (the reference's are; this says it of the device's own output)
        gp, gc = d.backward(sbuf, G_MAIN, G_AUX)
        m, mi = R.masks(c["gt"], c["lidar"], c["gthr"], c["ithr"])
        assert not gp[~(m & R.window_mask(c["shape"], c["rows"], c["cols"]))].view(np.uint32).any()
        assert not gc[~mi].view(np.uint32).any()
        # pred's gradient alone, from a forward without a correction (corr and lidar NULL)
        d2 = Device(L, c, offset, aux=False)
        s2 = d2.forward()
        got = d2.backward(s2, G_MAIN, None, True, False)[0]
        want = R.backward(*ins, read_stats(s2) if c["kind"] == R.NYU else c["stats_main_only"], G_MAIN, None, **c["kw"])[0]
        assert same_bits(got, want), name + ": main only"
        d.finish()
        d2.finish()


# ---------------------------------------------------------------- the device wrappers and the autograd operator

def _tensors(c, finite=False):
    import torch

    arrs = [np.array(c[k]) for k in ("pred", "gt", "lidar", "corr")]
    if finite:
        arrs = [np.nan_to_num(a, nan=0.0, posinf=1.0, neginf=1.0) for a in arrs]
        arrs[0] = np.where(np.abs(arrs[0]) > 1e30, F(1), arrs[0])
        arrs[3] = np.where(np.abs(arrs[3]) > 1e30, F(1), arrs[3])
    return [torch.from_numpy(np.ascontiguousarray(a, F)).to(DEV) for a in arrs]


def _dataset_kw(c):
    return dict(dataset="NYU" if c["kind"] == R.NYU else "KITTI", rows=c["rows"], cols=c["cols"])


@pytest.mark.parametrize("name", ("2x5x37", "2x9x11-window", "2x240x320-nyu"))
def test_autograd_matches_the_reference(pkg, L, name):
    import torch

    c = case(name)
    pred, gt, lidar, corr = _tensors(c)
    pred.requires_grad_(True), corr.requires_grad_(True), gt.requires_grad_(True), lidar.requires_grad_(True)
    kw = _dataset_kw(c)
    main, aux = pkg.autograd.train_loss(pred, gt, lidar, corr, **kw)
    assert main.dtype == torch.float32 and main.dim() == 0 and aux.dtype == torch.float32 and aux.dim() == 0
    dstats = pkg.device.train_loss_device(pred.detach(), gt.detach(), lidar.detach(), corr.detach(), **kw).cpu().numpy()
    check_stats(dstats, c["stats"], c["nterms"], name + " wrapper")
    assert main.item() == F(dstats[0]) and aux.item() == F(dstats[1])
    (3 * (main + aux)).backward()
    want = R.backward(c["pred"], c["gt"], dstats if c["kind"] == R.NYU else c["stats"], F(3), F(3), c["lidar"], c["corr"], **c["kw"])
    assert same_bits(pred.grad.cpu().numpy(), want[0]) and same_bits(corr.grad.cpu().numpy(), want[1])
    assert gt.grad is None and lidar.grad is None
    # aux unused: the correction gets no gradient, and pred's is the same
    p2, c2 = pred.detach().clone().requires_grad_(True), corr.detach().clone().requires_grad_(True)
    main2, aux2 = pkg.autograd.train_loss(p2, gt.detach(), lidar.detach(), c2, **kw)
    (3 * main2).backward()
    assert c2.grad is None and same_bits(p2.grad.cpu().numpy(), want[0])
    # main unused
    p3, c3 = pred.detach().clone().requires_grad_(True), corr.detach().clone().requires_grad_(True)
    (3 * pkg.autograd.train_loss(p3, gt.detach(), lidar.detach(), c3, **kw)[1]).backward()
    assert p3.grad is None and same_bits(c3.grad.cpu().numpy(), want[1])
    # without a correction: aux is None
    p4 = pred.detach().clone().requires_grad_(True)
    main4, aux4 = pkg.autograd.train_loss(p4, gt.detach(), **kw)
    assert aux4 is None and main4.item() == main.item()
    (3 * main4).backward()
    assert same_bits(p4.grad.cpu().numpy(), want[0])
    # only the correction asks for a gradient
    c5 = corr.detach().clone().requires_grad_(True)
    m5, a5 = pkg.autograd.train_loss(pred.detach(), gt.detach(), lidar.detach(), c5, **kw)
    (3 * (m5 + a5)).backward()
    assert same_bits(c5.grad.cpu().numpy(), want[1])


def test_wrapper_on_aligned_tensors_gives_the_abi_bits(pkg, L):
    """torch's allocations are 16-byte aligned: the 16-byte loads, two trips.  Same bits as the raw ABI 4 bytes off."""
    c = case("2x724x728-two-trips")
    pred, gt, lidar, corr = _tensors(c)
    d = Device(L, c, 4)
    sbuf = d.forward()
    want = read_stats(sbuf)
    stats = pkg.device.train_loss_device(pred, gt, lidar, corr)
    assert same_bits(stats.cpu().numpy(), want)
    import torch

    gm, ga = (torch.tensor(g, dtype=torch.float32, device=DEV) for g in (G_MAIN, G_AUX))
    gp, gc = pkg.device.train_loss_backward_device(pred, gt, stats, gm, ga, lidar, corr)
    wp, wc = d.backward(sbuf, G_MAIN, G_AUX)
    d.finish()
    assert same_bits(gp.cpu().numpy(), wp) and same_bits(gc.cpu().numpy(), wc)
    only = pkg.device.train_loss_backward_device(pred, gt, stats, gm, None, lidar, corr, want_correction=False)
    assert only[1] is None and same_bits(only[0].cpu().numpy(), wp)
    with pytest.raises(ValueError):
        pkg.device.train_loss_device(pred, gt, lidar)  # lidar without correction
    with pytest.raises(ValueError):
        pkg.device.train_loss_device(pred, gt, dataset="nyu")
    with pytest.raises(ValueError):
        pkg.device.train_loss_device(pred, gt[:, :-1].contiguous())
    with pytest.raises(ValueError):
        pkg.device.train_loss_device(pred, gt, rows=(4, 4))
    with pytest.raises(ValueError):
        pkg.device.train_loss_backward_device(pred, gt, stats, gm, ga, want_correction=True)


@pytest.mark.parametrize("dataset,shape", (("KITTI", (2, 9, 37)), ("NYU", (2, 240, 320))))
def test_autograd_against_the_eager_composition(pkg, L, dataset, shape):
    """train.py's expression in eager torch ops on the same device, in float64 (the exact value the bounds of
    test_train_loss.py's derivation speak of): the float64 values the operator's float32 results are rounded from within
    4 * 2^-24, every selected gradient within 2^-22, every unselected one +0."""
    import torch

    kind, gthr, ithr, rows, cols = R.PRESETS[dataset]
    rng = np.random.default_rng(23 + kind)
    arrs = R.make_case(rng, shape, nyu=kind == R.NYU, special=False, on_grid=False)
    arrs = [np.nan_to_num(a, nan=1.0 if k in (0, 3) else 0.0) for k, a in enumerate(arrs)]
    pred, gt, lidar, corr = (torch.from_numpy(a).to(DEV) for a in arrs)
    pred.requires_grad_(True), corr.requires_grad_(True)
    main, aux = pkg.autograd.train_loss(pred, gt, lidar, corr, dataset=dataset)
    (0.75 * main - 1.5 * aux).backward()
    p64, c64 = (t.detach().double().requires_grad_(True) for t in (pred, corr))
    g64 = gt.double()
    with_gt = gt > gthr_t(gthr)
    with_in = with_gt & (lidar > gthr_t(ithr))
    e = (p64 - g64) ** 2 * with_gt
    main_e = torch.sqrt(e[:, 6:228, 8:304].sum() / with_gt.sum()) if kind == R.NYU else e.sum() / with_gt.sum()
    aux_e = ((c64 - g64) ** 2 * with_in + (c64 - g64).abs() * with_in).sum() / with_in.sum()
    (0.75 * main_e - 1.5 * aux_e).backward()
    stats = pkg.device.train_loss_device(pred.detach(), gt, lidar, corr.detach(), dataset=dataset).cpu().numpy()
    for k, (nm, got, want) in enumerate((("main", main, main_e), ("aux", aux, aux_e))):
        rel = abs(stats[k] - want.item()) / abs(want.item())
        print("%s %s: fused %.17g eager %.17g rel %.3g" % (dataset, nm, stats[k], want.item(), rel))
        assert rel <= 4 * 2.0 ** -24 and got.item() == F(stats[k])
    sel_main = with_gt.clone()
    if kind == R.NYU:
        sel_main[:] = False
        sel_main[:, 6:228, 8:304] = with_gt[:, 6:228, 8:304]
    for nm, got, want, sel in (("grad_pred", pred.grad, p64.grad, sel_main), ("grad_corr", corr.grad, c64.grad, with_in)):
        got, want, sel = got.cpu().numpy(), want.cpu().numpy(), sel.cpu().numpy()
        assert not got[~sel].view(np.uint32).any() and not want[~sel].any()
        nz = sel & (want != 0)
        assert not got[sel & ~nz].any()
        err = np.abs(got[nz].astype(np.float64) - want[nz]) / np.abs(want[nz])
        print("%s %s: %d selected, max rel err %.3g" % (dataset, nm, nz.sum(), err.max()))
        assert nz.sum() > 20 and err.max() <= 2.0 ** -22


def gthr_t(v):
    """A threshold as the float32 the C ABI receives, for a compare with a float32 tensor."""
    return float(F(v))


def test_no_host_synchronisation(pkg, L):
    """Forward and backward under torch's synchronisation debug mode: any blocking call raises."""
    import torch

    c = case("2x9x11-window")
    kw = _dataset_kw(c)

    def step():
        pred, gt, lidar, corr = _tensors(c, finite=True)
        pred.requires_grad_(True), corr.requires_grad_(True)
        main, aux = pkg.autograd.train_loss(pred, gt, lidar, corr, **kw)
        (main + aux).backward()
        return main, aux, pred.grad, corr.grad

    _tensors(c)
    warm = step()  # the allocator's pools and the workspace exist
    torch.cuda.synchronize()
    pred, gt, lidar, corr = _tensors(c, finite=True)
    pred.requires_grad_(True), corr.requires_grad_(True)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        main, aux = pkg.autograd.train_loss(pred, gt, lidar, corr, **kw)
        (main + aux).backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert same_bits(pred.grad.cpu().numpy(), warm[2].cpu().numpy()) and main.item() == warm[0].item()

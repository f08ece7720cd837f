"""The training losses of train.py:215-251 without a GPU: the literal numpy statement of tests/loss_ref.py against torch's float64
autograd of the expression as train.py writes it, a hand case by value, the NYU window quirk, the edge cases, and the argument
checks of dtfill_train_loss / dtfill_train_loss_backward through ctypes (they come before any HIP call)."""
import numpy as np
import pytest

import loss_ref as R

F = np.float32
EPS = 2.0 ** -24  # the unit roundoff of float32


def train_py(pred, corr, gt, lidar, dataset):
    """train.py:215-249 as it reads, on float64 torch tensors [B,H,W] (the masks from the float32 frames, as the loader's
    numpy arrays give them).  Returns (main, aux)."""
    import torch

    if dataset == "KITTI":
        with_gt, with_input = gt > F(0.1), lidar > F(0.1)  # :215-216
    else:
        with_gt, with_input = gt > F(0.0001), lidar > F(0.001)  # :220-221
    total_value = np.sum(with_gt)  # :224
    with_input = np.logical_and(with_gt, with_input)  # :227
    total_value_input = np.sum(with_input)  # :228
    with_gt, with_input = torch.from_numpy(with_gt.astype(np.float64)), torch.from_numpy(with_input.astype(np.float64))
    gt = torch.from_numpy(gt.astype(np.float64))
    total_loss = (pred - gt) ** 2 * with_gt  # :240
    if dataset == "NYU":
        total_loss = torch.sqrt(torch.sum(total_loss[:, 6:228, 8:304]) / float(total_value))  # :242
    else:
        total_loss = torch.sum(total_loss) / float(total_value)  # :244
    auxi_loss = (corr - gt) ** 2 * with_input + torch.abs(corr - gt) * with_input  # :248
    return total_loss, torch.sum(auxi_loss) / float(total_value_input)  # :249


@pytest.mark.parametrize("dataset,shape", (("KITTI", (2, 9, 37)), ("NYU", (2, 240, 320))))
def test_numpy_statement_against_float64_autograd(dataset, shape):
    """The float32 statement against the exact (float64) value and gradient of train.py's expression.  u = 2^-24; fl(x) =
    x (1 + d), |d| <= u.
    Forward: e = fl(fl(p - g)^2) carries three roundings, a = fl(fl(fl(c - g)^2) + |fl(c - g)|) at most four, every term is
    non-negative, so the exact sum of the float32 terms (fsum, one more rounding of 2^-53) is within 4u relative of the exact
    sum, and so are main (KITTI) and aux after their double division.  The NYU root halves the relative error: 2u.
    Gradients: grad_pred = fl(fl(2 fl(p - g)) k): one rounding in t, none in 2t, one in k = fl32(g / n), one in the product:
    3u.  grad_corr = fl(fl(2u' + sgn u') k): one rounding in u', one in the sum -- 2u' and sgn u' share a sign, so nothing
    cancels and u's error is not amplified -- one in k, one in the product: 4u = 2^-22.  (For NYU k also carries main's own
    error, a weighted mean of signed per-term errors, far below its 1.5u worst case.)  Unselected pixels: +0 by bit pattern."""
    import torch

    kind, gthr, ithr, rows, cols = R.PRESETS[dataset]
    rng = np.random.default_rng(11 + kind)
    pred, gt, lidar, corr = R.make_case(rng, shape, nyu=kind == R.NYU, special=False, on_grid=False)
    # (x * mask would make a NaN of every non-finite input: train.py's expression is compared on finite frames, gt included)
    gt = np.nan_to_num(gt, nan=0.0)
    lidar = np.nan_to_num(lidar, nan=0.0)
    pred = np.nan_to_num(pred, nan=1.0)
    corr = np.nan_to_num(corr, nan=1.0)
    stats, _ = R.forward(pred, gt, lidar, corr, kind, gthr, ithr, rows, cols)
    p64 = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    c64 = torch.from_numpy(corr.astype(np.float64)).requires_grad_(True)
    main, aux = train_py(p64, c64, gt, lidar, dataset)
    g_main, g_aux = F(0.75), F(-1.5)
    (float(g_main) * main + float(g_aux) * aux).backward()
    rel = lambda got, want: abs(got - want) / abs(want)
    print("%s forward: main rel %.3g, aux rel %.3g" % (dataset, rel(stats[0], main.item()), rel(stats[1], aux.item())))
    assert rel(stats[0], main.item()) <= (2 if kind == R.NYU else 4) * EPS
    assert rel(stats[1], aux.item()) <= 4 * EPS
    m, mi = R.masks(gt, lidar, gthr, ithr)
    assert stats[2] == m.sum() > 0 and stats[3] == mi.sum() > 0
    gp, gc = R.backward(pred, gt, stats, g_main, g_aux, lidar, corr, kind, gthr, ithr, rows, cols)
    assert gp.dtype == F and gc.dtype == F
    for name, got, want, sel in (("grad_pred", gp, p64.grad.numpy(), m & R.window_mask(shape, rows, cols)),
                                 ("grad_corr", gc, c64.grad.numpy(), mi)):
        assert not got[~sel].view(np.uint32).any(), name + ": an unselected gradient is not +0"
        assert not want[~sel].any()
        nz = sel & (want != 0)
        assert np.array_equal(got[sel & ~nz], want[sel & ~nz])  # an exact prediction: 0 (of either sign) on both sides
        err = np.abs(got[nz].astype(np.float64) - want[nz]) / np.abs(want[nz])
        print("%s %s: %d selected, max rel err %.3g (bound %.3g)" % (dataset, name, nz.sum(), err.max(), 2.0 ** -22))
        assert nz.sum() > 20 and err.max() <= 2.0 ** -22, (name, err.max())


def test_hand_case_by_value():
    gt = np.array([2, 0, 4, 1], F).reshape(1, 1, 4)
    pred = np.array([3, 5, 2, 1], F).reshape(1, 1, 4)
    lidar = np.array([2, 0, 0, 1], F).reshape(1, 1, 4)
    corr = np.array([2.5, 9, 9, 0], F).reshape(1, 1, 4)
    stats, (nt_main, nt_aux) = R.forward(pred, gt, lidar, corr)
    assert stats[2] == 3 and stats[3] == 2 and (nt_main, nt_aux) == (3, 2)
    assert stats[4] == 5.0 and stats[5] == 2.75
    assert stats[0] == 5.0 / 3.0 and stats[1] == 1.375
    gp, gc = R.backward(pred, gt, stats, F(1), F(1), lidar, corr)
    third = F(1.0 / 3.0)
    assert np.array_equal(gp.reshape(-1), np.array([third * F(2), 0, -third * F(4), 0], F))
    assert np.array_equal(gc.reshape(-1), np.array([1, 0, 0, -1.5], F))
    assert not gp.reshape(-1)[[1, 3]].view(np.uint32).any() and not gc.reshape(-1)[[1, 2]].view(np.uint32).any()
    # NYU on the same frame: the root, and k_main = g / (2 main n_gt)
    s2, _ = R.forward(pred, gt, lidar, corr, R.NYU, 0.0001, 0.001, (0, 1), (0, 4))
    assert s2[0] == np.sqrt(5.0 / 3.0) and s2[2] == 3
    gp2, _ = R.backward(pred, gt, s2, F(1), None, lidar, corr, R.NYU, 0.0001, 0.001, (0, 1), (0, 4))
    k = F(1.0 / ((2.0 * np.sqrt(5.0 / 3.0)) * 3.0))
    assert np.array_equal(gp2.reshape(-1), np.array([F(2) * k, 0, F(-4) * k, 0], F))


def test_nyu_counts_the_frame_but_sums_the_window():
    """train.py:242 against :224: a gt-valid pixel with a large error outside [6,228) x [8,304) changes n_gt, and hence main;
    it does not change S_main, and its gradient is +0."""
    kind, gthr, ithr, rows, cols = R.PRESETS["NYU"]
    rng = np.random.default_rng(5)
    pred, gt, lidar, corr = R.make_case(rng, (1, 240, 320), nyu=True)
    outside = [(0, 0), (5, 100), (228, 100), (100, 7), (100, 304), (239, 319)]
    for i, j in outside:
        gt[0, i, j] = 0  # not valid: neither counted nor summed
    base, _ = R.forward(pred, gt, lidar, corr, kind, gthr, ithr, rows, cols)
    for i, j in outside:
        gt[0, i, j], pred[0, i, j] = 10, 1e6
    stats, _ = R.forward(pred, gt, lidar, corr, kind, gthr, ithr, rows, cols)
    assert stats[2] == base[2] + len(outside) and stats[4] == base[4]
    assert stats[0] == np.sqrt(base[4] / stats[2]) < base[0]
    gp, _ = R.backward(pred, gt, stats, F(1), None, lidar, corr, kind, gthr, ithr, rows, cols)
    for i, j in outside:
        assert gp[0, i, j].view(np.uint32) == 0
    # the same pixels inside the whole-frame window do count
    whole, _ = R.forward(pred, gt, lidar, corr, kind, gthr, ithr, None, None)
    assert whole[4] > stats[4] + 1e11
    # aux never sees the window
    assert stats[5] == whole[5] and stats[3] == whole[3]


def test_edge_cases():
    shape = (1, 3, 4)
    gt = np.zeros(shape, F)
    pred = np.ones(shape, F)
    # an empty mask: 0 / 0 = NaN, like the reference; every gradient +0
    stats, _ = R.forward(pred, gt, gt.copy(), pred.copy())
    assert np.isnan(stats[0]) and np.isnan(stats[1]) and not stats[2:].any()
    gp, gc = R.backward(pred, gt, stats, F(1), F(1), gt.copy(), pred.copy())
    assert not gp.view(np.uint32).any() and not gc.view(np.uint32).any()
    # corr = None: aux, n_in and S_aux are +0, no grad_corr
    gt[0, 1, 1], pred[0, 1, 1] = 2, 5
    stats, _ = R.forward(pred, gt)
    assert stats.tolist() == [9.0, 0.0, 1.0, 0.0, 9.0, 0.0] and not np.signbit(stats).any()
    gp, gc = R.backward(pred, gt, stats, F(1))
    assert gc is None and gp[0, 1, 1] == 6 and np.count_nonzero(gp) == 1
    # a threshold hit exactly is not selected, the next float above it is
    gt[0, 0, 0], gt[0, 0, 1] = F(0.1), np.nextafter(F(0.1), F(1))
    lidar = np.zeros(shape, F)
    lidar[0, 0, 1], lidar[0, 1, 1] = F(0.1), np.nextafter(F(0.1), F(1))
    m, mi = R.masks(gt, lidar, 0.1, 0.1)
    assert m.sum() == 2 and not m[0, 0, 0] and m[0, 0, 1] and mi.sum() == 1 and mi[0, 1, 1]
    # NaN or inf in pred / corr at an unselected pixel leaves no trace; a NaN gt or lidar is in no mask
    corr = pred.copy()
    clean = R.forward(pred, gt, lidar, corr)[0]
    pred2, corr2, gt2, lidar2 = pred.copy(), corr.copy(), gt.copy(), lidar.copy()
    pred2[0, 2, 0], pred2[0, 2, 1], corr2[0, 2, 2], corr2[0, 0, 1] = np.nan, np.inf, -np.inf, np.nan  # (0,0,1) is in m, not in mi
    gt2[0, 2, 3], lidar2[0, 2, 3] = np.nan, np.nan
    stats = R.forward(pred2, gt2, lidar2, corr2)[0]
    assert np.array_equal(stats, clean)
    gp, gc = R.backward(pred2, gt2, stats, F(2), F(2), lidar2, corr2)
    want = R.backward(pred, gt, clean, F(2), F(2), lidar, corr)
    assert np.array_equal(gp.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(gc.view(np.uint32), want[1].view(np.uint32))
    assert np.isfinite(gp).all() and np.isfinite(gc).all()
    # -0.0: an invalid gt; as a difference (pred == gt) it gives a zero term and a zero gradient of either sign
    gt3 = np.full(shape, F(-0.0))
    gt3[0, 0, 0] = 3
    pred3 = np.full(shape, F(-0.0))
    pred3[0, 0, 0] = 3
    stats = R.forward(pred3, gt3, gt3.copy(), pred3.copy())[0]
    assert stats.tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    gp, gc = R.backward(pred3, gt3, stats, F(1), F(1), gt3.copy(), pred3.copy())
    assert not gp.any() and not gc.any() and not gp.reshape(-1)[1:].view(np.uint32).any()  # sgn(0) = 0


# ---------------------------------------------------------------- the ABI without a GPU

NULL, SHAPE, WORKSPACE, METRIC = -1, -2, -3, -4
P = 256  # stands for a valid, aligned device pointer: no call below gets as far as using it


def _calls(L):
    ok = dict(pred=P, corr=P, gt=P, lidar=P, B=2, H=8, W=9, kind=0, gthr=0.1, ithr=0.1, r0=0, r1=8, c0=0, c1=9, stats=P, ws=P,
              nb=1 << 20, st=None, gm=P, ga=P, gp=P, gc=P)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.dtfill_train_loss(a["pred"], a["corr"], a["gt"], a["lidar"], a["B"], a["H"], a["W"], a["kind"], a["gthr"],
                                   a["ithr"], a["r0"], a["r1"], a["c0"], a["c1"], a["stats"], a["ws"], a["nb"], a["st"])

    def bwd(**kw):
        a = dict(ok, **kw)
        return L.dtfill_train_loss_backward(a["pred"], a["corr"], a["gt"], a["lidar"], a["B"], a["H"], a["W"], a["kind"],
                                            a["gthr"], a["ithr"], a["r0"], a["r1"], a["c0"], a["c1"], a["stats"], a["gm"],
                                            a["ga"], a["gp"], a["gc"], a["st"])

    return fwd, bwd


def test_argument_errors(pkg):
    """Every return code of include/dtfill.h's contract, each from one bad argument among good ones."""
    L = pkg.load()
    fwd, bwd = _calls(L)
    for f in (fwd, bwd):
        for k in ("pred", "gt", "stats"):
            assert f(**{k: None}) == NULL, k
        assert f(lidar=None) == NULL  # corr without lidar
        for k in ("B", "H", "W"):
            assert f(**{k: 0}) == SHAPE and f(**{k: -3}) == SHAPE, k
        assert f(B=1 << 15, H=1 << 8, W=1 << 8, r1=1 << 8, c1=1 << 8) == SHAPE  # B*H*W = 2^31
        M = 2 ** 31 - 1  # a product that does not fit 64 bits is rejected like any other
        assert f(B=M, H=M, W=M, r1=M, c1=M) == SHAPE and f(B=3, H=M, W=1, r1=M, c1=1) == SHAPE
        for win in (dict(r0=-1), dict(r1=9), dict(c0=-1), dict(c1=10), dict(r0=4, r1=4), dict(c0=5, c1=5), dict(r0=6, r1=2),
                    dict(c0=9, c1=9), dict(r0=8), dict(r1=0)):
            assert f(**win) == SHAPE, win
        for kind in (2, -1, 99):
            assert f(kind=kind) == METRIC, kind
    assert fwd(ws=None) == NULL
    need = L.dtfill_train_loss_workspace_bytes(2, 8, 9)
    assert need > 0
    assert fwd(nb=need - 1) == WORKSPACE and fwd(nb=0) == WORKSPACE
    assert fwd(ws=P + 4) == WORKSPACE and fwd(ws=P + 128) == WORKSPACE
    assert bwd(corr=None, lidar=None) == NULL  # grad_corr without corr
    assert bwd(gp=None, gc=None) == NULL  # no gradient asked for


def test_workspace_sizing(pkg):
    f = pkg.load().dtfill_train_loss_workspace_bytes
    sizes = [f(*s) for s in ((1, 1, 1), (2, 5, 37), (2, 256, 1216), (32, 256, 1216), (1, 1 << 15, (1 << 16) - 1))]
    assert all(0 < a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert sizes[-1] == sizes[-2] <= 64 << 10  # a fixed number of partials however large the batch
    M = 2 ** 31 - 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1 << 15, 1 << 8, 1 << 8), (M, M, M)):
        assert f(*bad) == 0, bad


def test_bindings_and_presets(pkg):
    """The Python layer's constants are the header's."""
    import re, os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtfill.h")).read()
    defs = dict(re.findall(r"#define (DTFILL_LOSS_[A-Z]+)\s+(\d+)", src))
    assert (int(defs["DTFILL_LOSS_KITTI"]), int(defs["DTFILL_LOSS_NYU"])) == (pkg._lib.LOSS_KITTI, pkg._lib.LOSS_NYU) == (R.KITTI, R.NYU)
    assert int(defs["DTFILL_LOSS_N"]) == len(pkg._lib.LOSS_COLUMNS) and pkg._lib.LOSS_COLUMNS == R.COLUMNS
    assert pkg.device.LOSS_PRESETS == R.PRESETS

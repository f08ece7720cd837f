"""Label -> source pixel without a GPU: the literal statement of tests/near_ref.py against its hand cases, against the
scipy-pinned `near` of tests/golden/l2_cases.npz and the oracle's depth on tests/golden/cases.npz, its backward against torch's
float64 autograd, and the argument checks of dtfill_nearest_gather / _backward through ctypes (they come before any HIP call)."""
import os
import re

import numpy as np
import pytest

import fill_grad_ref as G
import near_ref as R
from helpers import load_cases, load_l2_cases

F = np.float32


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_hand_cases_by_value():
    cases = R.hand_cases()
    assert len(cases) == 4
    for name, (x, index, vals, pixel, filled, status, grad_values) in cases.items():
        got_f, got_p, got_s = R.gather(x[None], index[None], vals[None, None])
        assert got_s[0] == status, name
        assert np.array_equal(got_p[0], pixel), (name, got_p[0])
        assert _same_bits(got_f[0, 0], filled), (name, got_f[0, 0])
        only_p = R.gather(x[None], index[None])
        assert only_p[0] is None and np.array_equal(only_p[1], got_p) and only_p[2][0] == status
        got_g, got_s = R.backward(x[None], index[None], R.hand_grad(x.shape)[None, None])
        assert got_s[0] == status and _same_bits(got_g[0, 0], grad_values), (name, got_g[0, 0])
    x, index = cases["survey 8c"][:2]
    at = {int(l): int(p) for l, p in zip(index.ravel(), cases["survey 8c"][3].ravel())}
    assert at == {1: 5, 2: 15, 3: 32}
    assert cases["a valued pixel that is no source"][6][0, 0].view(np.uint32) == 0  # +0.0 at the 0.5
    # the planted frame beside its neighbours: the rule is per pixel and per frame
    names = ("all zero", "planted labels", "a valued pixel that is no source")
    xs, idx = (np.stack([cases[n][k] for n in names]) for k in range(2))
    _, pixel, status = R.gather(xs, idx)
    assert status.tolist() == [R.NO_SOURCE, R.INDEX_ERROR, 0]
    assert all(np.array_equal(pixel[b], cases[n][3]) for b, n in enumerate(names))


def test_the_hand_frames_are_what_the_fill_gives(oracle):
    """The labels the hand cases assume are the oracle's (not the planted frame's: all of its labels are planted)."""
    cases = R.hand_cases()
    for name, c in cases.items():
        if name != "planted labels":
            assert np.array_equal(oracle.fill_batch(c[0][None])[2][0], c[1]), name


def test_l2_pixel_is_scipys_nearest(oracle):
    """Every case of l2_cases.npz: the reference's pixel map from the oracle's l2 labels is the stored scipy-pinned `near`
    (-1 everywhere and NO_SOURCE in a frame without sources)."""
    cases, _ = load_l2_cases()
    assert cases
    empty = 0
    for name, c in cases.items():
        x = np.ascontiguousarray(c["x"], F)[None]
        index = oracle.fill_batch(x, metric="l2")[2]
        _, pixel, status = R.gather(x, index)
        assert np.array_equal(pixel[0], c["near"].reshape(x.shape[1:])), name
        none = bool((c["near"] < 0).all())
        empty += none
        assert status[0] == (R.NO_SOURCE if none else 0), name
    assert empty  # the fixtures hold a frame without sources


def test_l1_pixel_reads_the_oracles_depth(oracle):
    """cases.npz: on frames whose two predicates agree (the value list is the source list) x.flat[pixel] is the oracle's depth."""
    cases, _ = load_cases()
    seen = 0
    for name, c in cases.items():
        x = np.ascontiguousarray(c["x"], F)
        x = x if x.ndim == 3 else x[None]
        src_thr, val_thr = (float(v) for v in np.ravel(c["thr"])[:2])
        index = np.asarray(c["lbl"], np.int32).reshape(x.shape)
        depth = np.asarray(c["depth"], F).reshape(x.shape)
        _, pixel, status = R.gather(x, index, src_thr=src_thr)
        for b in range(x.shape[0]):
            with np.errstate(invalid="ignore"):
                src, val = ~((F(1) - x[b]) > F(src_thr)), x[b] > F(val_thr)
            if not np.array_equal(src, val) or not src.any():
                continue
            seen += 1
            assert status[b] == 0 and (pixel[b] >= 0).all(), name
            assert _same_bits(x[b].reshape(-1)[pixel[b].reshape(-1)], depth[b].reshape(-1)), name
    assert seen >= 3


@pytest.mark.parametrize("seed,shape,C,p", ((1, (2, 12, 17), 3, 0.2), (2, (1, 24, 31), 1, 0.03), (3, (1, 9, 40), 2, 0.9)))
def test_backward_against_float64_autograd(oracle, seed, shape, C, p):
    """The oracle's labels on random frames; the gather as torch writes it, values.reshape(C, -1)[:, pix[L - 1]] in float64,
    and its autograd gradient for a finite upstream gradient spanning 40 binades, against backward() within the header's
    bound per cell: |S - exact| <= |C| 2^(E-38) + 2^-24 |exact| + 2^-149.  torch's float64 index_put sum adds |C| - 1 times,
    each within 2^-53 of a partial sum below |C| 2^(E+1), so |C|^2 2^(E+1-53) is added to the bound (tests/test_fill_backward.py
    argues the same way)."""
    import torch

    rng = np.random.default_rng(seed)
    B, H, W = shape
    x = np.where(rng.random(shape) < p, np.round(rng.uniform(1, 80, shape) * 256) / 256, 0).astype(F)
    x[0].reshape(-1)[rng.integers(0, H * W, 5)] = 0.5  # valued, not sources: never read
    index = oracle.fill_batch(x)[2]
    g = G.random_gradient(rng, (B, C, H, W), nonfinite=False)
    got, st = R.backward(x, index, g)
    assert not st.any() and got.dtype == F
    worst = 0.0
    for b in range(B):
        pix, k, _ = R.frame_ranks(x[b], index[b])
        assert (k >= 0).all()
        v64 = torch.zeros((C, H * W), dtype=torch.float64, requires_grad=True)
        out = v64[:, torch.from_numpy(pix[k])]
        out.backward(torch.from_numpy(g[b].reshape(C, -1).astype(np.float64)))
        want = v64.grad.numpy()
        gb = got[b].reshape(C, -1)
        rest = np.setdiff1d(np.arange(H * W), pix)
        assert not gb[:, rest].view(np.uint32).any() and not want[:, rest].any()
        for c in range(C):
            for j, s in enumerate(pix):
                terms = g[b, c].reshape(-1)[k == j]
                if terms.size == 0:
                    assert gb[c, s].view(np.uint32) == 0 and want[c, s] == 0
                    continue
                E = max((G.true_exponent(t) for t in terms if t != 0), default=None)  # (None: a cell of zeros, exact)
                bound = R.cell_bound(terms, want[c, s]) + (terms.size ** 2 * 2.0 ** (E + 1 - 53) if E is not None else 0.0)
                err = abs(float(gb[c, s]) - want[c, s])
                worst = max(worst, err / bound if bound else 0.0)
                assert err <= bound, (b, c, j, terms.size, gb[c, s], want[c, s], err, bound)
    print("seed %d: worst error %.3f of the bound" % (seed, worst))


def test_backward_nonfinite_cells_go_by_the_flags():
    """One source per label; the cells hold a NaN, both infinities, one infinity, and an overflowing pair."""
    H, W = 2, 8
    x = np.zeros((1, H, W), F)
    x[0, 0, :5] = 3.0  # sources 0 .. 4
    index = np.array([[[1, 2, 3, 4, 5, 1, 2, 3], [4, 5, 1, 2, 3, 4, 5, 0]]], np.int32)
    inf, nan = np.inf, np.nan
    g = np.array([[[[nan, inf, inf, -inf, 3e38, 1, -inf, 2], [-1, 3e38, 1, 5, 3, -2, 0, nan]]]], F)
    got, st = R.backward(x, index, g)
    want = np.zeros((1, 1, H, W), F)
    want[0, 0, 0, :5] = (nan, nan, inf, -inf, inf)  # the NaN at label 0 (the last pixel) goes nowhere
    assert not st.any() and np.array_equal(np.isnan(got), np.isnan(want))
    assert (got.view(np.uint32)[np.isnan(got)] == G.QNAN).all() and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ---------------------------------------------------------------- the ABI without a GPU

NULL, SHAPE, WORKSPACE, LAUNCH = -1, -2, -3, -5
P = 256  # stands for a valid, aligned device pointer: no call below that names a code gets as far as using it


def _fwd(L, **kw):
    a = dict(x=P, index=P, values=P, C=3, B=2, H=8, W=9, thr=0.1, out=P, pixel=P, status=P, ws=P, nb=1 << 20, st=None)
    a.update(kw)
    return L.dtfill_nearest_gather(a["x"], a["index"], a["values"], a["C"], a["B"], a["H"], a["W"], a["thr"], a["out"], a["pixel"],
                                   a["status"], a["ws"], a["nb"], a["st"])


def _bwd(L, **kw):
    a = dict(x=P, index=P, grad=P, C=3, B=2, H=8, W=9, thr=0.1, out=P, status=P, ws=P, nb=1 << 20, st=None)
    a.update(kw)
    return L.dtfill_nearest_gather_backward(a["x"], a["index"], a["grad"], a["C"], a["B"], a["H"], a["W"], a["thr"], a["out"],
                                            a["status"], a["ws"], a["nb"], a["st"])


def test_argument_errors(pkg):
    """Every return code of the contract that an argument can cause, each from one bad argument among good ones."""
    L = pkg.load()
    for call, ptrs in ((_fwd, ("x", "index", "ws")), (_bwd, ("x", "index", "grad", "out", "ws"))):
        for k in ptrs:
            assert call(L, **{k: None}) == NULL, k
        for k in ("B", "H", "W"):
            assert call(L, **{k: 0}) == SHAPE and call(L, **{k: -3}) == SHAPE, k
        assert call(L, B=70000, H=4, W=4) == SHAPE  # B is a grid dimension
        assert call(L, B=1, H=5000, W=5000) == SHAPE  # the forward's H + W - 2 < 8192
        assert call(L, B=1 << 15, H=1 << 8, W=1 << 8) == SHAPE  # B*H*W = 2^31
        assert call(L, C=-1) == SHAPE and call(L, C=65) == SHAPE
        assert call(L, nb=0) == WORKSPACE and call(L, ws=P + 4) == WORKSPACE and call(L, ws=P + 128) == WORKSPACE
        # the order of the checks: NULL before shape before workspace
        assert call(L, x=None, B=0, nb=0) == NULL and call(L, B=0, nb=0) == SHAPE
    assert _fwd(L, out=None, pixel=None) == NULL  # both outputs
    assert _fwd(L, values=None, pixel=None, out=None, C=0) == NULL
    assert _fwd(L, values=None) == NULL and _fwd(L, out=None) == NULL  # exactly one of values / out_values
    assert _fwd(L, C=0) == SHAPE  # C == 0 with values
    assert _bwd(L, C=0) == SHAPE
    need = L.dtfill_nearest_gather_workspace_bytes(2, 8, 9)
    assert need > 0 and _fwd(L, nb=need - 1) == WORKSPACE
    need = L.dtfill_nearest_gather_backward_workspace_bytes(2, 8, 9, 3)
    assert need > 0 and _bwd(L, nb=need - 1) == WORKSPACE
    assert _fwd(L, status=None, nb=0) == WORKSPACE and _bwd(L, status=None, nb=0) == WORKSPACE  # frame_status is nullable


def test_launch_failure_without_a_device(pkg):
    """Good arguments and no device to launch on: DTFILL_ERR_LAUNCH, the one code no argument causes.  (With a GPU present the
    stand-in pointers must not be launched on: the GPU module runs the good calls.)"""
    import torch

    if torch.cuda.is_available():
        return
    L = pkg.load()
    assert _fwd(L, nb=L.dtfill_nearest_gather_workspace_bytes(2, 8, 9)) == LAUNCH
    assert _fwd(L, values=None, out=None, C=0, nb=L.dtfill_nearest_gather_workspace_bytes(2, 8, 9)) == LAUNCH  # the pixel map alone
    assert _fwd(L, pixel=None, nb=L.dtfill_nearest_gather_workspace_bytes(2, 8, 9)) == LAUNCH
    assert _bwd(L, nb=L.dtfill_nearest_gather_backward_workspace_bytes(2, 8, 9, 3)) == LAUNCH


def test_workspace_sizing(pkg):
    L = pkg.load()
    f, fb = L.dtfill_nearest_gather_workspace_bytes, L.dtfill_nearest_gather_backward_workspace_bytes
    shapes = ((1, 1, 1), (2, 5, 37), (2, 240, 320), (32, 352, 1216))
    for size in (lambda *s: f(*s), lambda *s: fb(*s, 1), lambda *s: fb(*s, 64)):
        sizes = [size(*s) for s in shapes]
        assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    n = 32 * 352 * 1216
    assert 4 * n <= f(32, 352, 1216) <= 5 * n  # spix at 4 B/px and little else
    # the backward: non-decreasing in C, and for every C no larger than at C = 4 (the channels run in rounds)
    for s in shapes:
        per_c = [fb(*s, C) for C in range(1, 65)]
        assert all(a <= b for a, b in zip(per_c, per_c[1:])) and max(per_c) <= per_c[3], s
        assert per_c[0] >= 16 * s[0] * s[1] * s[2]
        assert fb(*s, 0) == 0 and fb(*s, 65) == 0 and fb(*s, -1) == 0
    # 0 on exactly the bad shapes of dtfill_workspace_bytes
    M = 2 ** 31 - 1
    for s in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 5000, 5000), (70000, 4, 4), (1 << 15, 1 << 8, 1 << 8), (M, M, M), (1, 1, 8192),
              (1, 8191, 1), (65535, 1, 1), (1, 4096, 4097), (1, 4097, 4097)) + shapes:
        bad = L.dtfill_workspace_bytes(*s, 0) == 0
        assert (f(*s) == 0) == bad and (fb(*s, 2) == 0) == bad, s


def test_bindings(pkg):
    """SYMBOLS against the header, the new names' place in both, and the constants."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dtfill.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dtfill_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(pkg._lib.SYMBOLS)
    new = {"dtfill_nearest_gather", "dtfill_nearest_gather_workspace_bytes", "dtfill_nearest_gather_backward",
           "dtfill_nearest_gather_backward_workspace_bytes"}
    assert new <= set(declared)
    L = pkg.load()
    assert len(L.dtfill_nearest_gather.argtypes) == 14 and len(L.dtfill_nearest_gather_backward.argtypes) == 13
    assert len(L.dtfill_nearest_gather_workspace_bytes.argtypes) == 3
    assert len(L.dtfill_nearest_gather_backward_workspace_bytes.argtypes) == 4
    assert re.search(r"#define DTFILL_ABI_VERSION 1\b", src) and L.dtfill_abi_version() == 1
    assert int(re.search(r"#define DTFILL_FRAME_NO_SOURCE\s+(\d+)", src).group(1)) == R.NO_SOURCE == pkg._lib.FRAME_NO_SOURCE == 4
    assert int(re.search(r"#define DTFILL_FRAME_INDEX_ERROR\s+(\d+)", src).group(1)) == R.INDEX_ERROR
    assert int(re.search(r"#define DTFILL_NEAR_MAX_C\s+(\d+)", src).group(1)) == 64
    for name in ("nearest_gather_device", "nearest_gather_backward_device"):
        assert hasattr(pkg.device, name)
    assert hasattr(pkg.autograd, "fill_values") and hasattr(pkg, "nearest_source")


def test_device_argument_checks_without_gpu(pkg):
    """The ValueErrors that need no device: dtype, rank, layout, shape, and host tensors where device tensors are asked for."""
    import torch

    x = torch.zeros((2, 4, 6))
    index = torch.zeros((2, 4, 6), dtype=torch.int32)
    values = torch.zeros((2, 3, 4, 6))
    fwd, bwd = pkg.device.nearest_gather_device, pkg.device.nearest_gather_backward_device
    for bad in (dict(x=x), dict(x=x.double()), dict(x=x[0]), dict(index=index.float()), dict(index=index[:, :-1]),
                dict(values=values.double()), dict(values=values[:, 0]), dict(values=values[:1]), dict(values=values[..., :-1])):
        a = dict(x=x, index=index, values=values)
        a.update(bad)
        with pytest.raises(ValueError):
            fwd(a["x"], a["index"], a["values"])
        with pytest.raises(ValueError):
            bwd(a["x"], a["index"], a["values"])
    with pytest.raises(ValueError):
        bwd(x, index, None)

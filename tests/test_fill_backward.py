"""The backward pass of the exact fill without a GPU: the literal statement of tests/fill_grad_ref.py against torch's float64
autograd of values[idx], the hand cases by value, the cell sum's own properties, and the argument checks of
dtfill_fill_backward through ctypes (they come before any HIP call)."""
import os
import re

import numpy as np
import pytest

import fill_grad_ref as R

F = np.float32


def _bits_match(got, want):
    """Bit for bit, a NaN matching a NaN."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("seed,shape,p", ((1, (2, 12, 17), 0.2), (2, (1, 24, 31), 0.03), (3, (1, 9, 40), 0.9)))
def test_statement_against_float64_autograd(oracle, seed, shape, p):
    """The oracle's labels (the reference's cv2 transform) on random frames, the gather as torch writes it -- values[idx] on the
    float64 value list -- and its autograd gradient for a random upstream gradient, against backward().

    The bound is the header's, |S - exact| <= |C| 2^(E-38) + 2^-24 |exact| + 2^-149, with `exact` torch's float64 index_put sum.
    That sum adds |C| - 1 times in float64: it is within (|C| - 1) 2^-53 sum|g| <= |C|^2 2^(E+1-53) of the exact sum, which is
    added to the bound (for |C| < 2^13, the largest cell a frame of these sizes can hold, it is below the first term).  The
    gradient spans 20 binades, so terms are rounded away (not every t is exact) and the first term is exercised."""
    import torch

    rng = np.random.default_rng(seed)
    B, H, W = shape
    x = np.where(rng.random(shape) < p, np.round(rng.uniform(1, 80, shape) * 256) / 256, 0).astype(F)
    x[0].reshape(-1)[rng.integers(0, H * W, 5)] = 0.5  # valued, not sources: the value list and the labels part ways
    depth, _, lbl, status = oracle.fill_batch(x)
    assert not status.any()
    assert np.array_equal(R.gather(x, lbl), depth)  # the gather this file transposes is the oracle's
    g = R.random_gradient(rng, shape, binades=20, special=False)
    got, st = R.backward(x, lbl, g)
    assert not st.any() and got.dtype == F
    worst = 0.0
    for b in range(B):
        valued, idx, ok = R.frame_cells(x[b], lbl[b], 0.1)
        x64 = torch.from_numpy(x[b].astype(np.float64)).requires_grad_(True)
        values = x64.reshape(-1)[torch.from_numpy(valued)]  # depth_list = x[with_value]
        out = values[torch.from_numpy(idx)]  # depth_list[lbl - 1]
        out.backward(torch.from_numpy(g[b].reshape(-1).astype(np.float64)))
        want = x64.grad.numpy().reshape(-1)
        gb = got[b].reshape(-1)
        not_valued = np.setdiff1d(np.arange(H * W), valued)
        assert not gb[not_valued].view(np.uint32).any() and not want[not_valued].any()
        for k, v in enumerate(valued):
            terms = g[b].reshape(-1)[idx == k]
            if terms.size == 0:
                assert gb[v].view(np.uint32) == 0 and want[v] == 0
                continue
            E = max(R.true_exponent(t) for t in terms)
            bound = R.cell_bound(terms, want[v]) + terms.size ** 2 * 2.0 ** (E + 1 - 53)
            err = abs(float(gb[v]) - want[v])
            worst = max(worst, err / bound)
            assert err <= bound, (b, k, terms.size, gb[v], want[v], err, bound)
    print("seed %d: worst error %.3f of the bound" % (seed, worst))
    assert worst > 0  # (some cell did round)


def test_hand_cases_by_value():
    cases = R.hand_cases()
    assert len(cases) == 7
    for name, (x, index, grad, want, status) in cases.items():
        got, st = R.backward(x[None], index[None], grad[None])
        assert st[0] == status, name
        assert _bits_match(got[0], want), (name, got[0], want)
        nan = np.isnan(got)
        assert (got.view(np.uint32)[nan] == R.QNAN).all(), name  # the one quiet NaN
    # the planted label n + 1 beside its neighbours: only that frame is zero and flagged
    names = ("valued pixels that are no sources", "a label n + 1", "a label -1")
    x, index, grad = (np.stack([cases[n][k] for n in names]) for k in range(3))
    got, st = R.backward(x, index, grad)
    assert st.tolist() == [0, 1, 0] and not got[1].view(np.uint32).any()
    assert _bits_match(got[0], cases[names[0]][3]) and _bits_match(got[2], cases[names[2]][3])


def test_the_hand_frames_are_what_the_fill_gives(oracle):
    """The labels the hand cases assume for their first three frames are the oracle's: no source under (0.1, 0.1)."""
    cases = R.hand_cases()
    for name in ("label 0 wraps to the last value", "all 0.5", "all zero"):
        x, index = cases[name][0], cases[name][1]
        depth, _, lbl, status = oracle.fill_batch(x[None])
        assert np.array_equal(lbl[0], index) and status[0] == cases[name][4], name
        if not status[0]:
            assert np.array_equal(R.gather(x[None], lbl), depth)


def test_cell_sum():
    S = R.cell_sum
    assert S([1e8, 1, -1e8]) == 1.0
    run = F(0)
    for g in (F(1e8), F(1), F(-1e8)):
        run = F(run + g)
    assert run == 0.0  # what a float32 running sum gives
    assert S([]).view(np.uint32) == 0 and S([-0.0]).view(np.uint32) == 0 and S([5.0, -5.0]).view(np.uint32) == 0
    assert S([np.nan, 1]).view(np.uint32) == R.QNAN and S([np.inf, -np.inf]).view(np.uint32) == R.QNAN
    assert S([np.inf, 1e38, 1e38]) == np.inf and S([-np.inf, -1]) == -np.inf
    assert S([3e38, 3e38]) == np.inf and S([-3e38, -3e38]) == -np.inf  # the scaling overflows, IEEE
    sub = F(2.0 ** -149)
    assert S([sub, sub, sub]) == F(3 * 2.0 ** -149) and S([sub, -sub]).view(np.uint32) == 0
    # a term 14 binades below the largest is exact, half a unit at 38 binades rounds to even
    assert S([2.0 ** 14, 1 + 2.0 ** -23, -2.0 ** 14]) == F(1 + 2.0 ** -23)
    assert S([2.0 ** 37, 0.5, -2.0 ** 37]) == 0 and S([2.0 ** 37, 1.5, -2.0 ** 37]) == 2
    # every order gives the same bits
    rng = np.random.default_rng(0)
    for _ in range(50):
        terms = R.random_gradient(rng, (int(rng.integers(2, 40)),), binades=60, special=False)
        want = S(terms)
        assert all(S(rng.permutation(terms)).view(np.uint32) == want.view(np.uint32) for _ in range(3))
    # the two roundings, in integers
    assert R.f32_of_int(2 ** 24 + 1) == (2 ** 23, 1) and R.f32_of_int(2 ** 24 + 3) == (2 ** 23 + 2, 1)  # ties to even
    assert R.f32_of_int(-(2 ** 60 + 2 ** 36)) == (-(2 ** 23), 37) and R.f32_of_int(2 ** 60 + 2 ** 36 + 1) == (2 ** 23 + 1, 37)
    assert R.ldexp_f32(3, -150) == F(2.0 ** -148) and R.ldexp_f32(1, -150) == 0 and R.ldexp_f32(2 ** 24 - 1, -173) == F(2.0 ** -149)


# ---------------------------------------------------------------- the ABI without a GPU

NULL, SHAPE, WORKSPACE, LAUNCH = -1, -2, -3, -5
P = 256  # stands for a valid, aligned device pointer: no call below that names a code gets as far as using it


def _call(L, **kw):
    a = dict(x=P, index=P, grad=P, B=2, H=8, W=9, thr=0.1, out=P, status=P, ws=P, nb=1 << 20, st=None)
    a.update(kw)
    return L.dtfill_fill_backward(a["x"], a["index"], a["grad"], a["B"], a["H"], a["W"], a["thr"], a["out"], a["status"], a["ws"],
                                  a["nb"], a["st"])


def test_argument_errors(pkg):
    """Every return code of the contract that an argument can cause, each from one bad argument among good ones."""
    L = pkg.load()
    for k in ("x", "index", "grad", "out", "ws"):
        assert _call(L, **{k: None}) == NULL, k
    for k in ("B", "H", "W"):
        assert _call(L, **{k: 0}) == SHAPE and _call(L, **{k: -3}) == SHAPE, k
    assert _call(L, B=70000, H=4, W=4) == SHAPE  # B is a grid dimension
    assert _call(L, B=1, H=5000, W=5000) == SHAPE  # the forward's H + W - 2 < 8192
    assert _call(L, B=1 << 15, H=1 << 8, W=1 << 8) == SHAPE  # B*H*W = 2^31
    need = L.dtfill_fill_backward_workspace_bytes(2, 8, 9)
    assert need > 0
    assert _call(L, nb=need - 1) == WORKSPACE and _call(L, nb=0) == WORKSPACE
    assert _call(L, ws=P + 4) == WORKSPACE and _call(L, ws=P + 128) == WORKSPACE
    # the order of the checks: NULL before shape before workspace
    assert _call(L, x=None, B=0, nb=0) == NULL and _call(L, B=0, nb=0) == SHAPE


def test_launch_failure_without_a_device(pkg):
    """Good arguments and no device to launch on: DTFILL_ERR_LAUNCH, the one code no argument causes.  (With a GPU present the
    stand-in pointers must not be launched on: the GPU module runs the good call.)"""
    import torch

    if torch.cuda.is_available():
        return
    L = pkg.load()
    assert _call(L, nb=L.dtfill_fill_backward_workspace_bytes(2, 8, 9)) == LAUNCH


def test_workspace_sizing(pkg):
    L = pkg.load()
    f = L.dtfill_fill_backward_workspace_bytes
    shapes = ((1, 1, 1), (2, 5, 37), (2, 240, 320), (32, 352, 1216))
    sizes = [f(*s) for s in shapes]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    # the accumulators (16 bytes per pixel) and little else
    assert 16 * 32 * 352 * 1216 <= sizes[-1] <= 17 * 32 * 352 * 1216
    # 0 on exactly the bad shapes of dtfill_workspace_bytes
    M = 2 ** 31 - 1
    for s in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 5000, 5000), (70000, 4, 4), (1 << 15, 1 << 8, 1 << 8), (M, M, M), (1, 1, 8192),
              (1, 8191, 1), (65535, 1, 1), (1, 4096, 4097), (1, 4097, 4097)) + shapes:
        assert (f(*s) == 0) == (L.dtfill_workspace_bytes(*s, 0) == 0), s


def test_bindings(pkg):
    """SYMBOLS against the header, and the new names' place in both."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dtfill.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dtfill_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(pkg._lib.SYMBOLS)
    assert {"dtfill_fill_backward", "dtfill_fill_backward_workspace_bytes"} <= set(declared)
    L = pkg.load()
    assert L.dtfill_fill_backward.restype is not None and len(L.dtfill_fill_backward.argtypes) == 12
    assert len(L.dtfill_fill_backward_workspace_bytes.argtypes) == 3
    assert re.search(r"#define DTFILL_ABI_VERSION 1\b", src) and L.dtfill_abi_version() == 1
    assert int(re.search(r"#define DTFILL_FRAME_INDEX_ERROR\s+(\d+)", src).group(1)) == R.INDEX_ERROR == pkg._lib.FRAME_INDEX_ERROR
    assert hasattr(pkg.device, "fill_backward_device") and hasattr(pkg.autograd, "fill")

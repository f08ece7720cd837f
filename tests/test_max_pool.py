"""The max-pool pyramid without a device: tests/pool_ref.py, the literal statement of both contracts of include/dtfill.h, held to
torch where torch is unambiguous (values without NaN, gradients without ties), to hand cases on one 8 x 8 window where it is
not (ties, +-0, NaN), and to the grouping of the backward's sum; and every return code of the two entry points, which are
host-side checks in front of any HIP call."""
import numpy as np
import pytest

import pool_ref as P

F = np.float32


@pytest.mark.parametrize("k", P.LEVELS)
def test_pool_ref_is_torch_max_pool2d_without_nan(k):
    import torch

    x = np.random.default_rng(k).standard_normal((2, 16, 24, 5)).astype(F)
    x[0, :4, :4] = np.round(x[0, :4, :4])  # ties in value: the value is the same whoever wins
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), k).permute(0, 2, 3, 1).numpy()
    got = P.max_pool(x, k)
    assert got.shape == (2, 16 // k, 24 // k, 5) and (got.view(np.uint32) == want.view(np.uint32)).all()


def test_backward_is_torch_autograd_without_ties():
    """Values drawn as a permutation, so that no two are equal: the winner is torch's, and every dx element is one of the
    three gradients or a sum of them in float64 within float32's rounding of the two adds."""
    import torch

    rng = np.random.default_rng(11)
    shape = (2, 16, 8, 4)
    x = rng.permutation(int(np.prod(shape))).reshape(shape).astype(F)
    dys = [rng.standard_normal((2, 16 // k, 8 // k, 4)).astype(F) for k in P.LEVELS]
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_()
    loss = sum((torch.nn.functional.max_pool2d(t, k) * torch.from_numpy(dy.astype(np.float64)).permute(0, 3, 1, 2)).sum()
               for k, dy in zip(P.LEVELS, dys))
    loss.backward()
    want = t.grad.permute(0, 2, 3, 1).numpy()
    got = P.backward(x, dys)
    scale = sum(np.abs(dy).max() for dy in dys)
    assert np.abs(got - want).max() <= 2 * 2.0 ** -24 * scale  # two rounded adds
    assert (got != 0).sum() == (want != 0).sum() >= x.size // 4  # every level-2 winner, a quarter of the pixels, has a gradient
    for drop in range(3):  # a level that is not asked for adds +0: the same bits as a gradient of zeros
        some = [None if n == drop else dy for n, dy in enumerate(dys)]
        zeroed = [np.zeros_like(dy) if n == drop else dy for n, dy in enumerate(dys)]
        assert (P.backward(x, some).view(np.uint32) == P.backward(x, zeroed).view(np.uint32)).all()
        assert (P.term(x, None, P.LEVELS[drop]).view(np.uint32) == 0).all()
    assert (P.backward(x, [None, None, None]).view(np.uint32) == 0).all()  # every dy NULL: all +0


@pytest.mark.parametrize("name,x,winners", P.hand_cases(), ids=[c[0] for c in P.hand_cases()])
def test_hand_cases_on_one_window(name, x, winners):
    for k in P.LEVELS:
        out, at = P.scan(x, k)
        i, j = winners[k]
        assert (at[0, 0, 0] == i * k + j).all(), (name, k, at[0, 0, 0])
        assert (out[0, 0, 0].view(np.uint32) == x[0, i, j].view(np.uint32)).all(), (name, k)  # the winner's own bits
        dy = np.full(out.shape, 3.0, F)
        t = P.term(x, dy, k)
        assert (t[0, i, j] == 3).all() and t[0, :k, :k].sum() == 3 * 4, (name, k)  # one winner per window and channel


def test_hand_cases_say_what_they_are_meant_to():
    cases = {c[0]: c for c in P.hand_cases()}
    x = cases["+0 before -0"][1]
    assert not np.signbit(P.max_pool(x, 8)).any() and np.signbit(P.max_pool(cases["-0 before +0"][1], 8)).all()
    nans = cases["two NaNs"][1]
    assert (P.max_pool(nans, 4)[0, 0, 0].view(np.uint32) == 0x7FC00123).all()
    assert (P.max_pool(nans, 8)[0, 0, 0].view(np.uint32) == 0x7FC00456).all()
    assert np.isnan(P.max_pool(cases["a NaN after a larger value"][1], 8)).all()


def sum_order_case():
    """(x, dys, the element): x[0,0] wins all three levels of its windows; dy2 = 1, dy4 = dy8 = 2^-24 there."""
    x = np.zeros((1, 8, 8, 4), F)
    x[0, 0, 0] = 1
    dys = [np.zeros((1, 8 // k, 8 // k, 4), F) for k in P.LEVELS]
    dys[0][0, 0, 0], dys[1][0, 0, 0], dys[2][0, 0, 0] = 1, 2.0 ** -24, 2.0 ** -24
    return x, dys


def test_the_sum_is_grouped_as_t2_plus_t4_then_t8():
    one, tiny = F(1), F(2.0 ** -24)
    assert F(F(one + tiny) + tiny) == 1 and F(one + F(tiny + tiny)) != 1  # the two groupings differ on this case
    x, dys = sum_order_case()
    dx = P.backward(x, dys)
    assert (dx[0, 0, 0] == 1).all() and dx.sum() == 4


def test_every_return_code_of_both_entry_points(pkg):
    """DTFILL_ERR_NULL and DTFILL_ERR_SHAPE are decided on the host before any HIP call; the pointers are never followed."""
    L = pkg.load()
    p = 4096  # any non-NULL address
    ok = dict(B=1, H=8, W=8, C=4, xc=4, xo=0, l2=(p, 4, 0), l4=(p, 4, 0), l8=(p, 4, 0))

    def forward(x=p, **kw):
        a = dict(ok, **kw)
        return L.dtfill_max_pool_pyramid(x, a["B"], a["H"], a["W"], a["C"], a["xc"], a["xo"], *a["l2"], *a["l4"], *a["l8"], None)

    def backward(x=p, dx=p, **kw):
        a = dict(ok, **kw)
        return L.dtfill_max_pool_pyramid_backward(x, a["B"], a["H"], a["W"], a["C"], a["xc"], a["xo"], *a["l2"], *a["l4"], *a["l8"], dx, None)

    none = (None, 0, 0)
    assert forward(x=None) == -1 and backward(x=None) == -1 and backward(dx=None) == -1
    assert forward(l2=none, l4=none, l8=none) == -1  # every out NULL; (in the backward every dy may be NULL: tests/test_gpu_max_pool.py)
    assert forward(x=None, B=0) == -1  # NULL is reported first
    shape_errors = [dict(B=0), dict(H=0), dict(W=0), dict(H=12), dict(W=4),  # not multiples of the largest requested level
                    dict(H=4, W=4, l8=none, l4=(p, 4, 0), l2=none, C=4, xc=4, B=-1),
                    dict(H=6, W=6, l8=none, l4=(p, 4, 0)),  # level 4 is the largest: 6 is no multiple of it
                    dict(H=6, W=6, l8=none, l4=none, C=6, xc=6), dict(C=0), dict(C=2, xc=2), dict(C=6, xc=8), dict(C=-4),
                    dict(xc=6), dict(xc=10, C=4, xo=2), dict(xo=4), dict(xc=8, xo=8), dict(xo=-4, xc=8),
                    dict(l2=(p, 6, 0)), dict(l4=(p, 8, 2)), dict(l8=(p, 8, 8)), dict(l2=(p, 8, -4)), dict(l4=(p, 0, 0)),
                    dict(C=8, xc=8, l8=(p, 4, 0)),  # the slice does not fit its tensor
                    dict(H=32768, W=32768),  # B H W x_channels = 2^32
                    dict(H=16384, W=16384, xc=8),  # 2^31
                    dict(H=8192, W=8192, l2=(p, 128, 0)),  # x has 2^28 floats, out2 2^24 pixels of 128: 2^31
                    dict(B=1 << 20, H=2048, W=2048)]  # beyond 64 bits if multiplied carelessly
    for kw in shape_errors:
        assert forward(**kw) == -2, kw
        assert backward(**kw) == -2, kw
    assert b"shape" in L.dtfill_strerror(-2)

"""dtfill_max_pool_pyramid and dtfill_max_pool_pyramid_backward on the device against tests/pool_ref.py, the literal statement of
their contracts, bit for bit (+0 == -0, a NaN matches a NaN; where the sign of a zero or a NaN's payload is the point, the bits
themselves), through the ABI on guarded buffers with poisoned outputs, in the manner of test_gpu_conv2d.py, whose helpers these
are; then the device functions, the numpy form, the autograd operator, and streams and threads."""
import itertools

import numpy as np
import pytest

import concurrency
import conv_ref as R
import pool_ref as P
import test_gpu_conv2d as fwd
from test_max_pool import sum_order_case

pytestmark = pytest.mark.gpu

DEV = fwd.DEV
F = np.float32
POISON = fwd.POISON
LEVELS = P.LEVELS
# one level-8 window and one float4; several windows, frames and blocks (2 x 6 windows of 16 quads: 768 threads); C no multiple of 16
SHAPES = ((1, 8, 8, 4), (2, 16, 24, 64), (1, 8, 16, 20))
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(LEVELS, n)]


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


def values(shape, seed):
    """Mixed magnitudes and signs, a few exact ties, -0 and +0."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 2.0 ** rng.integers(-3, 4, shape)).astype(F)
    x[rng.random(shape) < 0.1] = 0.0
    x[rng.random(shape) < 0.05] = -0.0
    x[rng.random(shape) < 0.1] = 1.5
    return x


def _wide(a, width, at):
    """a [..., C] as the channels at .. at + C - 1 of a tensor `width` wide, the others poison."""
    if width == a.shape[-1] and at == 0:
        return a
    out = np.full(a.shape[:-1] + (width,), POISON, np.uint32).view(F)
    out[..., at:at + a.shape[-1]] = a
    return out


def run_forward(L, x, levels=LEVELS, width=None, at=0, x_width=None, x_at=0, mis=0, stream=None):
    """One call of dtfill_max_pool_pyramid on guarded buffers: x the channels x_at .. of a tensor x_width wide, every out the
    channels at .. of a tensor `width` wide.  Returns {level: the whole out tensor, poison where the call wrote nothing}."""
    import torch

    B, H, W, C = x.shape
    width = C if width is None else width
    wx = _wide(x, C if x_width is None else x_width, x_at)
    gx = fwd._up(wx, mis)
    outs = {k: fwd._poisoned((B, H // k, W // k, width), mis) for k in levels}
    args = [v for k in LEVELS for v in ((outs[k].ptr, width, at) if k in outs else (None, 0, 0))]
    rc = L.dtfill_max_pool_pyramid(gx.ptr, B, H, W, C, wx.shape[3], x_at, *args, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    gx.check("x")
    assert (gx.view(torch.int32, wx.shape).cpu().numpy() == wx.view(np.int32)).all(), "x was written"
    for k, g in outs.items():
        g.check("out%d" % k)
    return {k: g.view(torch.float32, (B, H // k, W // k, width)).cpu().numpy() for k, g in outs.items()}


def run_backward(L, x, dys, width=None, at=0, x_width=None, x_at=0, mis=0, stream=None):
    """One call of dtfill_max_pool_pyramid_backward on guarded buffers; dys: (dy2, dy4, dy8), each an array or None, read as
    the channels at .. of tensors `width` wide.  Returns dx [B,H,W,C]."""
    import torch

    B, H, W, C = x.shape
    width = C if width is None else width
    wx = _wide(x, C if x_width is None else x_width, x_at)
    gx = fwd._up(wx, mis)
    wide = [None if dy is None else _wide(dy, width, at) for dy in dys]
    gdy = [None if w is None else fwd._up(w, mis) for w in wide]
    gdx = fwd._poisoned((B, H, W, C), mis)
    args = [v for g in gdy for v in ((g.ptr, width, at) if g else (None, 0, 0))]
    rc = L.dtfill_max_pool_pyramid_backward(gx.ptr, B, H, W, C, wx.shape[3], x_at, *args, gdx.ptr, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g, w, what in [(gx, wx, "x")] + [(g, w, "dy") for g, w in zip(gdy, wide) if g]:
        g.check(what)
        assert (g.view(torch.int32, w.shape).cpu().numpy() == w.view(np.int32)).all(), what + " was written"
    gdx.check("dx")
    return gdx.view(torch.float32, (B, H, W, C)).cpu().numpy()


def gradients(x, seed, levels=LEVELS):
    rng = np.random.default_rng(seed)
    B, H, W, C = x.shape
    return [(values((B, H // k, W // k, C), seed + k) + F(0.25 * rng.integers(1, 4))).astype(F) if k in levels else None for k in LEVELS]


_reference = {}


def reference(shape, seed):
    """(x, dys, pool_ref's three outputs, its dx), worked out once per case and shared."""
    if (shape, seed) not in _reference:
        x = values(shape, seed)
        dys = gradients(x, seed + 100)
        _reference[(shape, seed)] = x, dys, dict(zip(LEVELS, P.pyramid(x))), P.backward(x, dys)
    return _reference[(shape, seed)]


@pytest.mark.parametrize("shape", SHAPES)
def test_both_directions_at_every_shape(L, shape):
    x, dys, want, want_dx = reference(shape, 1)
    got = run_forward(L, x)
    for k in LEVELS:
        R.assert_same(got[k], want[k], "out%d at %s" % (k, shape))
        assert (got[k].view(np.uint32) == want[k].view(np.uint32)).all(), "the winner's own bits, the sign of a zero too"
    R.assert_same(run_backward(L, x, dys), want_dx, "dx at %s" % (shape,))


def test_offsets_keep_their_neighbours_and_a_pointer_off_by_one_float(L):
    shape = SHAPES[1]
    x, dys, want, want_dx = reference(shape, 1)
    got = run_forward(L, x, width=128, at=64, x_width=128, x_at=64)  # what the inference class does
    for k in LEVELS:
        R.assert_same(got[k][..., 64:], want[k], "out%d at offset 64 of 128" % k)
        assert (got[k][..., :64].view(np.uint32) == POISON).all(), "the other channels keep their poison"
    R.assert_same(run_backward(L, x, dys, width=128, at=64, x_width=128, x_at=64), want_dx, "dx, x and dy at offset 64 of 128")
    got = run_forward(L, x, width=96, at=4, x_width=80, x_at=12, mis=4)
    for k in LEVELS:
        R.assert_same(got[k][..., 4:68], want[k], "out%d, every pointer 4 bytes off a 16-byte boundary" % k)
        assert (np.delete(got[k], np.s_[4:68], axis=-1).view(np.uint32) == POISON).all()
    R.assert_same(run_backward(L, x, dys, width=96, at=4, x_width=80, x_at=12, mis=4), want_dx, "dx, every pointer 4 bytes off")
    small = SHAPES[2]
    x, dys, want, want_dx = reference(small, 1)
    got = run_forward(L, x, mis=4)
    for k in LEVELS:
        R.assert_same(got[k], want[k], "out%d of %s, 4 bytes off" % (k, small))
    R.assert_same(run_backward(L, x, dys, mis=4), want_dx, "dx of %s, 4 bytes off" % (small,))


@pytest.mark.parametrize("levels", SUBSETS, ids=["-".join(map(str, s)) for s in SUBSETS])
def test_every_subset_of_levels(L, levels):
    """A NULL out skips its level, a NULL dy adds +0, and the largest REQUESTED level decides the rule for H and W."""
    k = max(levels)
    shape = (2, 2 * k, 3 * k, 8)  # no multiple of the next level
    x = values(shape, 7)
    got = run_forward(L, x, levels)
    assert set(got) == set(levels)
    for lv in levels:
        R.assert_same(got[lv], P.max_pool(x, lv), "out%d alone with %s" % (lv, levels))
    dys = gradients(x, 8, levels)
    R.assert_same(run_backward(L, x, dys), P.backward(x, dys), "dx with the dys of %s" % (levels,))


def test_the_smallest_frames_and_a_backward_without_any_gradient(L):
    x = values((1, 4, 4, 4), 3)  # levels 2 and 4 only: 4 is no multiple of 8 and need not be
    got = run_forward(L, x, (2, 4))
    R.assert_same(got[2], P.max_pool(x, 2), "out2 of 4 x 4")
    R.assert_same(got[4], P.max_pool(x, 4), "out4 of 4 x 4")
    assert L.dtfill_max_pool_pyramid(4096, 1, 4, 4, 4, 4, 0, 4096, 4, 0, 4096, 4, 0, 4096, 4, 0, None) == -2
    x = values((2, 3, 5, 12), 4)  # every dy NULL: any frame, dx all +0, every element written
    dx = run_backward(L, x, [None, None, None])
    assert (dx.view(np.uint32) == 0).all()


def test_every_tie_pattern_of_a_4x4_window(L):
    """All 65 536 patterns of 0 and 1 in a 4 x 4 window, one per (frame, window, channel) of a [64,16,16,64] batch, 4 MB: levels 2
    and 4, both directions.  A merge of 2 x 2 winners that breaks ties by block order fails on every pattern whose first
    maximum in raster order is not the first in block order."""
    n = np.arange(65536).reshape(64, 4, 4, 64)  # (frame, window row, window column, channel) -> the pattern
    x = np.empty((64, 16, 16, 64), F)
    for i in range(4):
        for j in range(4):
            x[:, i::4, j::4, :] = (n >> (4 * i + j)) & 1
    want2, want4 = P.max_pool(x, 2), P.max_pool(x, 4)
    got = run_forward(L, x, (2, 4))
    R.assert_same(got[2], want2, "out2")
    R.assert_same(got[4], want4, "out4")
    dys = gradients(x, 5, (2, 4))
    assert all((dy != 0).all() for dy in dys[:2])
    want = P.backward(x, dys)
    dx = run_backward(L, x, dys)
    R.assert_same(dx, want, "dx")
    first = (n & 0b10111) == 0b10100  # maxima at (0,2) and (1,0), nothing before them: (0,2) wins, though (1,0) is in block 0
    assert first.any() and (P.scan(x, 4)[1][first] == 2).all() and (dx[:, 0::4, 2::4, :][first] != 0).all()


def test_ties_of_the_8x8_window_and_the_hand_cases(L):
    x = np.random.default_rng(6).integers(0, 3, (2, 16, 24, 8)).astype(F)  # nearly every window ties, at every level
    want = P.pyramid(x)
    got = run_forward(L, x)
    dys = gradients(x, 9)
    for k, w in zip(LEVELS, want):
        R.assert_same(got[k], w, "out%d" % k)
    R.assert_same(run_backward(L, x, dys), P.backward(x, dys), "dx")
    for name, x, winners in P.hand_cases():
        got = run_forward(L, x)
        dys = [np.full((1, 8 // k, 8 // k, 4), 2.0 ** n, F) for n, k in enumerate(LEVELS)]  # 1, 2, 4: the sum says who won what
        dx = run_backward(L, x, dys)
        R.assert_same(dx, P.backward(x, dys), "dx of " + name)
        for n, k in enumerate(LEVELS):
            i, j = winners[k]
            assert (got[k][0, 0, 0].view(np.uint32) == x[0, i, j].view(np.uint32)).all(), (name, k, "the winner's own bits")
            assert (dx[0, i, j].astype(int) & (1 << n)).all(), (name, k, "the gradient went elsewhere")
        assert dx.sum() == 4 * (16 * 1 + 4 * 2 + 4)


def test_the_sum_is_grouped_as_t2_plus_t4_then_t8(L):
    x, dys = sum_order_case()
    dx = run_backward(L, x, dys)
    assert (dx[0, 0, 0] == 1).all(), "(1 + 2^-24) + 2^-24 is 1; 1 + (2^-24 + 2^-24) is not"
    R.assert_same(dx, P.backward(x, dys), "dx")
    for drop in range(3):  # each dy NULL in turn
        some = [None if n == drop else dy for n, dy in enumerate(dys)]
        R.assert_same(run_backward(L, x, some), P.backward(x, some), "dy%d NULL" % LEVELS[drop])


def test_device_functions_numpy_form_and_autograd(pkg, L):
    import torch

    dev = pkg.device
    shape = SHAPES[1]
    x, dys, want, want_dx = reference(shape, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tx = t(x)
    outs = dev.max_pool_pyramid_device(tx)
    assert len(outs) == 3
    for k, o in zip(LEVELS, outs):
        R.assert_same(o.cpu().numpy(), want[k], "max_pool_pyramid_device, level %d" % k)
    (o4,) = dev.max_pool_pyramid_device(tx, (4,))
    R.assert_same(o4.cpu().numpy(), want[4], "one level")
    R.assert_same(pkg.max_pool(x, 8), want[8], "numpy max_pool")
    wide = torch.full((2, 8, 12, 128), float("nan"), device=DEV)
    got = dev.max_pool_pyramid_device(t(_wide(x, 128, 64)), (2,), 64, 64, [wide], [64])
    assert got[0] is wide and np.isnan(wide[..., :64].cpu().numpy()).all()
    R.assert_same(wide[..., 64:].cpu().numpy(), want[2], "x_offset, channels, outs, out_offsets")
    dx = dev.max_pool_pyramid_backward_device(tx, [t(dy) for dy in dys])
    R.assert_same(dx.cpu().numpy(), want_dx, "max_pool_pyramid_backward_device")
    dx = dev.max_pool_pyramid_backward_device(tx, [None, t(_wide(dys[1], 96, 32))], (2, 4), grad_offsets=[0, 32])
    R.assert_same(dx.cpu().numpy(), P.backward(x, [None, dys[1], None]), "a gradient at an offset, another None")
    # under the tape: level 2 concatenated behind 16 other channels (its gradient arrives as a slice), level 4 used as it is,
    # level 8 unused (a NULL dy)
    px = tx.clone().requires_grad_()
    p2, p4, p8 = pkg.autograd.max_pool_pyramid(px)
    R.assert_same(p8.detach().cpu().numpy(), want[8], "autograd forward")
    other = torch.zeros((2, 8, 12, 16), device=DEV)
    loss = (torch.cat([other, p2], dim=3) * torch.cat([other, t(dys[0])], dim=3)).sum() + (p4 * t(dys[1])).sum()
    loss.backward()
    R.assert_same(px.grad.cpu().numpy(), P.backward(x, [dys[0], dys[1], None]), "loss.backward()")
    for bad in (dict(levels=(3,)), dict(levels=(2, 2)), dict(levels=()), dict(outs=[wide]), dict(out_offsets=[4, 0, 0]),
                dict(levels=(2,), outs=[tx]), dict(levels=(2,), outs=[wide[:1].contiguous()])):
        with pytest.raises(ValueError):
            dev.max_pool_pyramid_device(**dict(dict(x=tx), **bad))
    with pytest.raises(ValueError):
        dev.max_pool_pyramid_device(tx.double())
    with pytest.raises(pkg.DtfillError):
        dev.max_pool_pyramid_device(tx[:, :12].contiguous())  # 12 rows: no multiple of 8
    with pytest.raises(pkg.DtfillError):
        dev.max_pool_pyramid_device(tx, x_offset=2)


def test_two_streams_and_four_threads(pkg, L):
    """The operator from four host threads on two streams at once, three rounds: every call's outputs and gradient are the
    reference's."""
    import torch

    dev = pkg.device
    shape = SHAPES[1]
    x, dys, want, want_dx = reference(shape, 1)
    tx = torch.from_numpy(x).to(DEV)
    tdy = [torch.from_numpy(dy).to(DEV) for dy in dys]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()

    def work(k, r):
        s = streams[k % 2]
        with torch.cuda.stream(s):
            outs = dev.max_pool_pyramid_device(tx)
            dx = dev.max_pool_pyramid_backward_device(tx, tdy)
        s.synchronize()
        for lv, o in zip(LEVELS, outs):
            R.assert_same(o.cpu().numpy(), want[lv], "thread %d round %d level %d" % (k, r, lv))
        R.assert_same(dx.cpu().numpy(), want_dx, "thread %d round %d dx" % (k, r))

    failures = concurrency.run_rounds(work, 4, 3)
    assert not failures, concurrency.describe(failures)

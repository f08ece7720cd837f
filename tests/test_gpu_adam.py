"""dtfill_adam_step on the device against tests/adam_ref.py bit for bit (any NaN equal to any NaN), through the ABI on guarded
buffers in the manner of test_gpu_max_pool.py: every parameter, both moment buffers with the padding floats between their
segments, the step record, and the guard bands of all of them.  Then the Python layer: adam_step_device, the numpy form, and
two optimizers on two streams.

No captured-graph test: lr and the pointer lists are launch arguments, so a replay would freeze them (optim.py says so)."""
import ctypes
import struct

import numpy as np
import pytest

import adam_ref as A
import test_gpu_conv2d as fwd
from guarded import GuardedBuffer
from test_gpu_reentrancy import released_together

pytestmark = pytest.mark.gpu

DEV = fwd.DEV
F = np.float32
POISON = fwd.POISON
EDGE = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e-20, -1e-20, 1e30, -1e30, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-7], F)


@pytest.fixture(scope="module")
def L(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg._lib.load()


@pytest.fixture(scope="module")
def CH(pkg):
    return pkg._lib.ADAM_CHUNK


def values(rng, n, edge=False):
    """n float32 values over a dozen binades, both signs; with `edge`, a fifth of them from EDGE."""
    x = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 5, n)).astype(F)
    if edge:
        at = rng.random(n) < 0.2
        x[at] = rng.choice(EDGE, int(at.sum()))
    return x


class Run:
    """Parameters, moments and a record on guarded buffers, and the reference's copy of them on the host.  mis_p[i]: bytes
    parameter i lies off a 16-byte boundary; mis_state: the same for m and v."""

    def __init__(self, L, params, mis_p=None, mis_state=0, stream=None):
        import torch

        self.L, self.stream, self.n = L, stream, len(params)
        self.counts = [p.size for p in params]
        self.offsets, self.floats = A.segment_offsets(self.counts)
        self.p = [np.array(p, F) for p in params]
        self.m = [np.zeros(c, F) for c in self.counts]
        self.v = [np.zeros(c, F) for c in self.counts]
        self.state = A.adam_state0()
        self.gp = [fwd._up(p, (mis_p or [0] * self.n)[i]) for i, p in enumerate(self.p)]
        start = np.full(self.floats, POISON, np.uint32).view(F)  # the padding floats: poison, and they stay poison
        for at, c in zip(self.offsets, self.counts):
            start[at:at + c] = 0
        self.gm, self.gv = fwd._up(start, mis_state), fwd._up(start, mis_state)
        self.grec = GuardedBuffer(24, 0, DEV)
        self.grads = []  # (guarded buffer, host array) of every step: alive until check(), and checked there
        assert L.dtfill_adam_record_bytes() == 24
        assert L.dtfill_adam_init(self.grec.ptr, self._handle()) == 0

    def _handle(self):
        import torch

        return None if self.stream is None else torch.cuda.current_stream().cuda_stream

    def upload(self, grads, mis_g=None):
        return [None if g is None else fwd._up(g, (mis_g or [0] * self.n)[i]) for i, g in enumerate(grads)]

    def step(self, grads, mis_g=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, up=None):
        """One call of dtfill_adam_step; grads[i] None: no gradient; up: upload()'s buffers of them, where the copy must not
        happen here.  Nothing is read back."""
        up = self.upload(grads, mis_g) if up is None else up
        self.grads += [(b, np.array(g, F)) for b, g in zip(up, grads) if b is not None]
        rc = self.L.dtfill_adam_step((ctypes.c_void_p * self.n)(*(b.ptr for b in self.gp)),
                                     (ctypes.c_void_p * self.n)(*(None if b is None else b.ptr for b in up)),
                                     (ctypes.c_longlong * self.n)(*self.counts), self.n, self.gm.ptr, self.gv.ptr, self.grec.ptr,
                                     lr, beta1, beta2, eps, self._handle())
        assert rc == 0, rc
        state = self.state
        for i, g in enumerate(grads):
            if g is not None:
                self.p[i], self.m[i], self.v[i], state = A.adam_step_ref(self.p[i], g, self.m[i], self.v[i], self.state, lr, beta1, beta2, eps)
        self.state = state

    def record(self):
        return struct.unpack("<qdd", self.grec.payload().cpu().numpy().tobytes())

    def check(self, what=""):
        import torch

        torch.cuda.synchronize()
        for i, b in enumerate(self.gp):
            b.check("%s p[%d]" % (what, i))
            A.assert_same(b.view(torch.float32, (self.counts[i],)).cpu().numpy(), self.p[i], "%s p[%d] of %d" % (what, i, self.counts[i]))
        for b, g in self.grads:
            b.check(what + " g")
            assert (b.view(torch.int32, g.shape).cpu().numpy() == g.view(np.int32)).all(), what + ": a gradient was written"
        for name, b, ref in (("m", self.gm, self.m), ("v", self.gv, self.v)):
            b.check("%s %s" % (what, name))
            got = b.view(torch.float32, (self.floats,)).cpu().numpy()
            pad = np.ones(self.floats, bool)
            for i, (at, c) in enumerate(zip(self.offsets, self.counts)):
                A.assert_same(got[at:at + c], ref[i], "%s %s[%d] of %d" % (what, name, i, c))
                pad[at:at + c] = False
            assert (got.view(np.uint32)[pad] == POISON).all(), "%s: a padding float of %s was written" % (what, name)
        self.grec.check(what + " record")
        assert struct.pack("<qdd", *self.record()) == struct.pack("<qdd", *self.state), (what, self.record(), self.state)
        self.grads = []


def test_chunk_seams_three_steps_and_the_record(L, CH):
    """Counts 1, 3, 4, 5 and one below, at, one above and 2 CH + 7 past the chunk size in ONE call; three steps with no host
    read in between; t, b1p and b2p afterwards are the reference's bit for bit."""
    rng = np.random.default_rng(11)
    counts = [1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7]
    run = Run(L, [values(rng, c) for c in counts])
    assert run.floats == L.dtfill_adam_state_floats((ctypes.c_longlong * 8)(*counts), 8)
    for lr in (1e-3, 1e-3, 5e-4):  # (the schedule halves lr between steps)
        run.step([values(rng, c) for c in counts], lr=lr)
    run.check("chunk seams")
    assert run.record()[0] == 3 and run.record()[1] == float(F(0.9)) * float(F(0.9)) * float(F(0.9))


def test_the_hand_case(L):
    import test_adam as T

    run = Run(L, [T.HAND_P])
    for step, (alpha, want_p, want_v) in enumerate(T.HAND, 1):
        run.step([T.HAND_G])
        run.check("hand case, step %d" % step)
        assert T.bits(run.p[0]) == want_p and T.bits(run.v[0]) == want_v


@pytest.mark.parametrize("n_off", (-1, 0, 1))
def test_group_seams(pkg, L, n_off):
    """One below, at and one above the variables a launch takes, tensors of 1 to 40 floats, two steps.  Every tensor has data
    of its own, so one of the second launch that read the first launch's table would show."""
    n = pkg._lib.ADAM_GROUP + n_off
    rng = np.random.default_rng(20 + n_off)
    counts = [int(c) for c in rng.integers(1, 41, n)]
    run = Run(L, [values(rng, c) for c in counts])
    for _ in range(2):
        run.step([values(rng, c) for c in counts])
    run.check("%d tensors" % n)


def test_misaligned_pointers_beside_aligned_ones(L, CH):
    """p and g off a 16-byte boundary by 0, 4, 8 and 12 bytes, independently: 16 tensors in one call, one of them longer than
    two chunks, only the (0, 0) ones on the 16-byte path.  Then m and v themselves 4 bytes off: every tensor on the dword path."""
    rng = np.random.default_rng(31)
    mis = [(a, b) for a in (0, 4, 8, 12) for b in (0, 4, 8, 12)]
    counts = [1000 + 37 * k for k in range(16)]
    counts[5], counts[0], counts[15] = 2 * CH + 7, CH + 5, 3
    run = Run(L, [values(rng, c) for c in counts], mis_p=[a for a, _ in mis])
    for _ in range(2):
        run.step([values(rng, c) for c in counts], mis_g=[b for _, b in mis])
    run.check("misaligned p and g")
    counts = [5, CH + 9, 64]
    run = Run(L, [values(rng, c) for c in counts], mis_state=4)
    for _ in range(2):
        run.step([values(rng, c) for c in counts])
    run.check("misaligned m and v")


def test_edge_values(L, CH):
    """+-0, denormals, 1e-20, 1e30, Inf and NaN in the parameters and in the gradients, on both paths, two steps (the second
    meets them in m and v too)."""
    rng = np.random.default_rng(41)
    counts = [EDGE.size, 2 * EDGE.size + 1, CH + 3, 777]
    params = [values(rng, c, edge=True) for c in counts]
    params[0] = np.array(EDGE)
    run = Run(L, params, mis_p=[0, 0, 0, 8])
    run.step([np.array(EDGE)[::-1].copy()] + [values(rng, c, edge=True) for c in counts[1:]])
    run.step([values(rng, c, edge=True) for c in counts])
    run.check("edge values")
    assert any(np.isnan(p).any() for p in run.p) and any(np.isinf(v).any() for v in run.v)
    # the denormal of the contract: g = 1e-20f, one step
    run = Run(L, [np.array([-2.0, 0.5, 3.0, 1.0], F)])
    run.step([np.array([1e-20, 1e-20, 0.0, 1.0], F)])
    run.check("denormal")
    assert run.v[0].view(np.uint32).tolist()[:2] == [0x47, 0x47]


def test_a_subset_keeps_the_other_segments(L, CH):
    """Step 2 has no gradient for tensors 1 and 4 (and step 3 for 0): their parameters and their segments of m and v stay as
    they are, and the others' segments stay where they were."""
    rng = np.random.default_rng(51)
    counts = [6, CH + 2, 17, 3, 40, 9]
    run = Run(L, [values(rng, c) for c in counts])
    run.step([values(rng, c) for c in counts])
    run.check("all six")
    before = [run.p[i].copy() for i in (1, 4)], [run.m[i].copy() for i in (1, 4)]
    run.step([None if i in (1, 4) else values(rng, c) for i, c in enumerate(counts)])
    run.check("without 1 and 4")
    assert all((a == b).all() for a, b in zip(before[0] + before[1], [run.p[1], run.p[4], run.m[1], run.m[4]]))
    run.step([None if i == 0 else values(rng, c) for i, c in enumerate(counts)])
    run.check("without 0")
    assert run.record()[0] == 3


def test_device_function_and_numpy_form(pkg):
    import torch

    O = pkg.optim
    rng = np.random.default_rng(61)
    counts = [(3, 3, 1, 16), (16,), (5, 7)]
    p = [values(rng, int(np.prod(c))).reshape(c) for c in counts]
    g = [values(rng, int(np.prod(c))).reshape(c) for c in counts]
    offsets, floats = A.segment_offsets([a.size for a in p])
    tp = [torch.from_numpy(a.copy()).to(DEV) for a in p]
    tg = [torch.from_numpy(a.copy()).to(DEV) for a in g]
    m, v = torch.zeros(floats, device=DEV), torch.zeros(floats, device=DEV)
    record = O.new_record(DEV)
    O.adam_step_device(tp, tg, m, v, record, 2e-3, 0.8, 0.99, 1e-6)
    O.adam_step_device(tp, [tg[0], None, tg[2]], m, v, record, 1e-3)
    state, want = A.adam_state0(), []
    for i in range(3):
        a, b, c, s1 = A.adam_step_ref(p[i], g[i], np.zeros_like(p[i]), np.zeros_like(p[i]), state, 2e-3, 0.8, 0.99, 1e-6)
        if i != 1:
            a, b, c, _ = A.adam_step_ref(a, g[i], b, c, s1, 1e-3)
        want.append((a, b, c))
    for i in range(3):
        A.assert_same(tp[i].cpu().numpy(), want[i][0], "adam_step_device p[%d]" % i)
        A.assert_same(m[offsets[i]:offsets[i] + p[i].size].cpu().numpy(), want[i][1].reshape(-1), "m[%d]" % i)
        A.assert_same(v[offsets[i]:offsets[i] + p[i].size].cpu().numpy(), want[i][2].reshape(-1), "v[%d]" % i)
    t, b1p, b2p = O.read_record(record)
    assert (t, b1p, b2p) == (2, float(F(0.8)) * float(F(0.9)), float(F(0.99)) * float(F(0.999)))
    # the numpy form, from the start
    np_p, np_m, np_v, np_state = O.adam_step(p, g, np.zeros(floats, F), np.zeros(floats, F), A.adam_state0(), 2e-3, 0.8, 0.99, 1e-6)
    for i in range(3):
        first = A.adam_step_ref(p[i], g[i], np.zeros_like(p[i]), np.zeros_like(p[i]), A.adam_state0(), 2e-3, 0.8, 0.99, 1e-6)
        A.assert_same(np_p[i], first[0], "adam_step p[%d]" % i)
        A.assert_same(np_m[offsets[i]:offsets[i] + p[i].size], first[1].reshape(-1), "adam_step m[%d]" % i)
    assert np_state == A.adam_advance(A.adam_state0(), 0.8, 0.99)
    for bad in (dict(grads=tg[:2]), dict(grads=[tg[0], tg[1], tg[2][:3].contiguous()]), dict(m=m[:-4]), dict(v=v.double()),
                dict(record=record[:2]), dict(lr=-1.0), dict(beta2=1.0), dict(grads=[None, None, None]),
                dict(params=[tp[0], tp[1], tp[2].t()])):
        with pytest.raises(ValueError):
            O.adam_step_device(**dict(dict(params=tp, grads=tg, m=m, v=v, record=record, lr=1e-3), **bad))
    with pytest.raises(pkg.DtfillError):
        O.adam_step_device(tp, [tg[0], tg[1], tp[2]], m, v, record, 1e-3)  # a gradient that is its parameter


def test_two_optimizers_on_two_streams(L, CH):
    """Two sets of variables, moments and records, stepped on two streams released together by an event."""
    import torch

    rng = np.random.default_rng(71)
    counts = ([40 * CH + 3, 5, 17 * CH], [33 * CH, CH - 1, 9, 8 * CH + 1])
    runs = [Run(L, [values(rng, c) for c in cs], stream=True) for cs in counts]
    grads = [[values(rng, c) for c in cs] for cs in counts]
    ups = [iter([run.upload(g), run.upload(g)]) for run, g in zip(runs, grads)]  # (a copy from the host would wait for the blocker)
    torch.cuda.synchronize()
    released_together(torch, lambda: runs[0].step(grads[0], up=next(ups[0])),
                      lambda: runs[1].step(grads[1], up=next(ups[1])))  # (each runs twice: two steps)
    for k, run in enumerate(runs):
        run.check("stream %d" % k)
        assert run.record()[0] == 2

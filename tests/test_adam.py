"""The Adam step's statement, tests/adam_ref.py, held to itself on the CPU: the hand case's bits, alpha against the closed form,
a float64 run of the same rule, the rule that tells Keras' epsilon from torch's, IEEE's edge values, the segment layout; then
the library's return codes and KerasAdam's argument checks, neither of which needs a GPU.  tests/test_gpu_adam.py holds the
kernel to adam_ref bit for bit."""
import ctypes
import math
import re

import numpy as np
import pytest

import adam_ref as A

F = np.float32
U = 2.0 ** -24  # float32's unit roundoff


def bits(a):
    return [int(x) for x in np.asarray(a, F).reshape(-1).view(np.uint32)]


HAND_P = np.array([0, 1, -2, 1e-30, 3], F)
HAND_G = np.array([1, -0.5, 1e-20, 1e-3, 0], F)
# lr = 1e-3, Keras' defaults otherwise, m = v = 0: alpha, p', v' after steps 1, 2 and 3, worked out once in numpy float32 and
# written down here, so that a change of adam_ref.py's own arithmetic shows
HAND = (
    (0x39A5CB17, [0xBA831253, 0x3F8020C5, 0xC0000000, 0xBA82A8A8, 0x40400000], [0x3A831200, 0x39831200, 0x00000047, 0x30896FEC, 0]),
    (0x3976BEEF, [0xBB031257, 0x3F80418A, 0xC0000000, 0xBB02B81A, 0x40400000], [0x3B030139, 0x3A030139, 0x0000008E, 0x31095E54, 0]),
    (0x3953D273, [0xBB449B86, 0x3F80624F, 0xC0000000, 0xBB4422BA, 0x40400000], [0x3B4468B0, 0x3A4468B0, 0x000000D5, 0x314DF320, 0]),
)


def test_the_hand_case_bit_for_bit():
    p, m, v, state = HAND_P, np.zeros(5, F), np.zeros(5, F), A.adam_state0()
    assert state == (0, 1.0, 1.0)
    for step, (alpha, want_p, want_v) in enumerate(HAND, 1):
        assert bits(A.adam_alpha(state, 1e-3)) == [alpha], step
        p, m, v, state = A.adam_step_ref(p, HAND_G, m, v, state, 1e-3)
        assert bits(p) == want_p and bits(v) == want_v, step
        assert state[0] == step
    assert bits(m[:2]) == [0x3E8AC085, 0xBE0AC085]
    assert state[1] == float(F(0.9)) * float(F(0.9)) * float(F(0.9)) and state[2] == float(F(0.999)) * float(F(0.999)) * float(F(0.999))
    # c1 and c2 are float32 subtractions, not 0.1f and 0.001f
    assert bits(F(1) - F(0.9)) == [0x3DCCCCD0] and bits(F(0.1)) == [0x3DCCCCCD]
    assert abs(float(F(1) - F(0.999)) - 0.0009999871) < 1e-10 and F(1) - F(0.999) != F(0.001)
    # lr is a float32 argument: as a double it would round alpha the other way at step 3
    t, b1p, b2p = A.adam_advance(A.adam_advance(A.adam_advance(A.adam_state0())))
    assert bits(F(1e-3 * math.sqrt(1.0 - b2p) / (1.0 - b1p))) == [0x3953D272]


def test_alpha_is_the_closed_form_rounded_once():
    """alpha against lr sqrt(1 - beta2^t) / (1 - beta1^t) in float64 with libm's pow, t = 1 .. 20 000.  The two differ by the
    running products' roundings (t - 1 of them, 2^-53 each, against pow's one) and a dozen float64 operations, and the powers'
    relative errors are magnified by b / (1 - b) where 1 - b cancels (halved under the square root):
        rel <= (t + 2) 2^-53 (b2^t / (1 - b2^t) / 2 + b1^t / (1 - b1^t)) + 16 2^-53
    on top of the half ulp of alpha's one rounding to float32."""
    lr, b1, b2 = float(F(1e-3)), float(F(0.9)), float(F(0.999))
    state, exact = A.adam_state0(), 0
    for t in range(1, 20001):
        alpha = A.adam_alpha(state, 1e-3)
        state = A.adam_advance(state)
        p1, p2 = math.pow(b1, t), math.pow(b2, t)
        closed = lr * math.sqrt(1.0 - p2) / (1.0 - p1)
        rel = (t + 2) * 2.0 ** -53 * (0.5 * p2 / (1.0 - p2) + p1 / (1.0 - p1)) + 16 * 2.0 ** -53
        assert abs(float(alpha) - closed) <= 0.5 * float(np.spacing(alpha)) + closed * rel, t
        exact += F(closed) == alpha
    assert state[0] == 20000 and exact > 19900  # (nearly always the closed form's own rounding)


def test_a_float64_run_of_the_same_rule_stays_within_the_derived_bound():
    """100 steps, 4096 elements, g = +-uniform(0.5, 1), p0 in (-1, 1), lr = 1e-3, against the same rule with the same float32
    scalars and float64 element arithmetic.  First order in u = 2^-24, with G = max |g| = 1, w_t = 1 - beta2^t:
      m: per step the roundings of g - m (<= 2 G u, then scaled by c1), of c1 * . (<= 2 G c1 u) and of the sum (<= G u) add
         (4 c1 + 1) G u = 1.4 u, and the old error shrinks by 1 - c1 = 0.9:            |dm| <= 14 u
      v: g g and g g - v (<= g g) round relative to g g <= 1 and are scaled by c2, c2 * . likewise, the sum rounds relative to
         v' >= w_t / 4 (every g g >= 1/4): relative to v' a step adds u (1 + 12 c2 / w_t) <= u (1 + 12 / t), and (1 - c2) v <=
         v' keeps the old relative error from growing:                                  |dv| / v <= u (100 + 12 H_100) < 163 u
      p: the step is D = alpha m' / (sqrt(v') + eps) with |m'| <= 1 - beta1^t and sqrt(v') >= sqrt(w_t) / 2, so |D| <= 2 lr;
         its error is alpha |dm| / sqrt(v') + |D| (163 u / 2 + 5 u) <= 28 lr u / (1 - beta1^t) + 173 lr u <= 453 lr u, and the
         subtraction rounds relative to |p| <= 1 + 100 * 2 lr = 1.2:                    |dp| <= 100 (453 lr + 1.2) u < 166 u"""
    rng = np.random.default_rng(7)
    n, steps, lr = 4096, 100, 1e-3
    p = rng.uniform(-1, 1, n).astype(F)
    m, v, state = np.zeros(n, F), np.zeros(n, F), A.adam_state0()
    p64, m64, v64 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    c1, c2, eps = float(F(1) - F(A.BETA1)), float(F(1) - F(A.BETA2)), float(F(A.EPS))
    for _ in range(steps):
        g = (rng.uniform(0.5, 1, n) * rng.choice([-1.0, 1.0], n)).astype(F)
        alpha = float(A.adam_alpha(state, lr))
        p, m, v, state = A.adam_step_ref(p, g, m, v, state, lr)
        g64 = g.astype(np.float64)
        m64 = m64 + c1 * (g64 - m64)
        v64 = v64 + c2 * (g64 * g64 - v64)
        p64 = p64 - (alpha * m64) / (np.sqrt(v64) + eps)
    assert np.abs(m - m64).max() <= 14 * U
    assert (np.abs(v - v64) / v64).max() <= 163 * U
    assert np.abs(p - p64).max() <= 166 * U
    assert np.abs(p - p64).max() > 0  # (float32 does round: the comparison is of two different computations)


def test_the_rule_is_keras_epsilon_hat_not_torchs():
    """Step 1, |g| of eps's size.  Keras: alpha m / (sqrt(v) + eps) = lr sqrt(c2) g / (sqrt(c2) g + eps), 0.0306 lr at g = eps.
    Torch divides sqrt(v) by sqrt(1 - beta2^t) first: lr g / (g + eps), 0.5 lr.  The statement's move equals the first within
    10 u (three roundings in m', three under the square root in v', halved; alpha's, the product, the root, the sum, the
    quotient) and is a factor 16 from torch's."""
    import torch

    lr, g = 1e-3, F(1e-7)
    p1, m1, v1, _ = A.adam_step_ref(np.zeros(1, F), np.array([g], F), np.zeros(1, F), np.zeros(1, F), A.adam_state0(), lr, eps=1e-7)
    move = -float(p1[0])
    b1, b2, c1, c2 = float(F(0.9)), float(F(0.999)), float(F(1) - F(0.9)), float(F(1) - F(0.999))
    alpha = float(F(lr)) * math.sqrt(1.0 - b2) / (1.0 - b1)
    closed = alpha * (c1 * float(g)) / (math.sqrt(c2 * float(g) ** 2) + float(F(1e-7)))
    assert abs(move - closed) <= 10 * U * closed
    assert 0.030 * lr < move < 0.031 * lr
    w = torch.zeros(1, dtype=torch.float32, requires_grad=True)
    w.grad = torch.tensor([float(g)], dtype=torch.float32)
    torch.optim.Adam([w], lr=lr, eps=1e-7).step()
    torch_move = -float(w.detach()[0])
    assert 0.49 * lr < torch_move < 0.51 * lr
    assert torch_move > 16 * move


def test_denormals_and_non_finite_gradients_go_where_ieee_sends_them():
    g = np.array([1e-20, np.nan, np.inf, -np.inf, 0.0, -0.0], F)
    p = np.array([-2, 1, 1, 1, -0.0, 5], F)
    p1, m1, v1, _ = A.adam_step_ref(p, g, np.zeros(6, F), np.zeros(6, F), A.adam_state0(), 1e-3)
    assert bits(v1[0]) == [0x00000047] and bits(p1[0]) == [0xC0000000] and 0 < m1[0] < 1e-20  # denormal v', kept
    assert np.isnan(p1[1]) and np.isnan(m1[1]) and np.isnan(v1[1])
    assert m1[2] == np.inf and v1[2] == np.inf and np.isnan(p1[2])  # inf / inf
    assert m1[3] == -np.inf and v1[3] == np.inf and np.isnan(p1[3])
    assert bits(p1[4:]) == [0x80000000, 0x40A00000] and not m1[4:].any() and not v1[4:].any()  # 0 / eps: nothing moves


def test_segment_offsets(pkg):
    assert A.segment_offsets([1, 3, 4, 5]) == ([0, 4, 8, 12], 20)
    assert A.segment_offsets([8]) == ([0], 8)
    L = pkg.load()
    for counts in ([1, 3, 4, 5], [8], [1], [4097, 2, 1 << 20]):
        arr = (ctypes.c_longlong * len(counts))(*counts)
        assert L.dtfill_adam_state_floats(arr, len(counts)) == A.segment_offsets(counts)[1], counts
    assert pkg.optim.segment_offsets([1, 3, 4, 5]) == ([0, 4, 8, 12], 20)


def test_constants_match_the_header(pkg):
    import os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtfill.h")).read()
    defines = dict(re.findall(r"^#define DTFILL_(ADAM_\w+)[ \t]+(\d+)\b", src, flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == {"ADAM_GROUP": pkg._lib.ADAM_GROUP, "ADAM_CHUNK": pkg._lib.ADAM_CHUNK}
    assert pkg.load().dtfill_adam_record_bytes() == 24 == 8 * pkg.optim.RECORD_WORDS
    # the launch's argument block: 28 bytes a variable and 48 of scalars, under HIP's 4096
    assert pkg._lib.ADAM_GROUP * 28 + 48 < 4096


def test_every_return_code_without_a_gpu(pkg):
    """Validation comes before any HIP call: made-up device addresses never reach a launch here."""
    L = pkg.load()
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    P, G, C = (vp * 2)(1 << 20, 2 << 20), (vp * 2)(3 << 20, 4 << 20), (ll * 2)(16, 5)
    M, V, R = 5 << 20, 6 << 20, 7 << 20
    step = lambda params=P, grads=G, counts=C, n=2, m=M, v=V, rec=R, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7: L.dtfill_adam_step(
        params, grads, counts, n, m, v, rec, lr, b1, b2, eps, None)
    for null in ("params", "grads", "counts", "m", "v", "rec"):
        assert step(**{null: None}) == -1, null
    assert step(n=0) == -2 and step(n=-3) == -2
    assert step(params=(vp * 2)(1 << 20, None)) == -1  # a NULL parameter, even where it has no gradient
    assert step(params=(vp * 2)(1 << 20, None), grads=(vp * 2)(3 << 20, None)) == -1
    assert step(grads=(vp * 2)(None, None)) == -1  # nothing to step
    for bad in (0, -1, 1 << 31, 1 << 40):
        assert step(counts=(ll * 2)(16, bad)) == -2, bad
    for name in ("lr", "eps"):
        for bad in (-1e-3, float("inf"), float("nan")):
            assert step(**{name: bad}) == -2, (name, bad)
    for name in ("b1", "b2"):
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            assert step(**{name: bad}) == -2, (name, bad)
    assert step(grads=(vp * 2)((1 << 20) + 60, 4 << 20)) == -2  # grads[0] starts inside params[0]'s 64 bytes
    assert step(grads=(vp * 2)((1 << 20) - 60, 4 << 20)) == -2  # and ends inside them
    assert step(params=(vp * 2)(1 << 20, 2 << 20), grads=(vp * 2)(3 << 20, 2 << 20)) == -2  # the same tensor
    # NULL comes before shape, arrays before elements
    assert step(m=None, n=0) == -1 and step(n=0, params=(vp * 2)(None, None)) == -2
    assert L.dtfill_adam_init(None, None) == -1
    S = L.dtfill_adam_state_floats
    assert S(None, 2) == 0 and S(C, 0) == 0 and S(C, -1) == 0
    assert S((ll * 2)(4, 0), 2) == 0 and S((ll * 2)(4, 1 << 31), 2) == 0 and S((ll * 2)(4, (1 << 31) - 1), 2) == 4 + (1 << 31)
    many = (ll * 9)(*([(1 << 31) - 4] * 9))  # 9 (2^31 - 4) > 2^34 - 4 floats: an offset would not fit its 32 bits of quads
    assert S(many, 8) == 8 * ((1 << 31) - 4) and S(many, 9) == 0
    assert b"shape" in L.dtfill_strerror(-2)


def test_keras_adam_argument_checks(pkg):
    import torch

    KerasAdam = pkg.optim.KerasAdam
    w = torch.zeros(4, requires_grad=True)
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=1e-3, beta_1=1.0), dict(lr=1e-3, beta_2=-0.1),
                dict(lr=1e-3, epsilon=-1e-7), dict(lr=1e-3, epsilon=float("inf"))):
        with pytest.raises(ValueError):
            KerasAdam([w], **bad)
    with pytest.raises(ValueError):
        KerasAdam([], lr=1e-3)
    with pytest.raises(ValueError, match="one group"):
        KerasAdam([dict(params=[w]), dict(params=[torch.zeros(2, requires_grad=True)])], lr=1e-3)
    with pytest.raises(ValueError, match="CUDA"):  # a CPU tensor: there is no CPU form of the optimizer
        KerasAdam([w], lr=1e-3)
    with pytest.raises(ValueError):
        KerasAdam([torch.zeros(4, dtype=torch.float64, requires_grad=True)], lr=1e-3)
    with pytest.raises(TypeError):
        KerasAdam([w])  # lr has no default: train.py always passes one
    for bad in (dict(lr=-1.0), dict(beta1=1.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            pkg.optim._check_scalars(**dict(dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7), **bad))

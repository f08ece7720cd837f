"""The Adam step of the reference's training loop, stated literally: numpy float32 scalars and Python floats, one rounding per
operation.  include/dtfill.h (dtfill_adam_step) states the same contract; csrc/dtfill_adam.hpp is held to this file bit for bit.

train.py:169 builds tf.keras.optimizers.Adam(lr=lr, beta_1=0.9): the "epsilon-hat" rule with eps = 1e-7,
    alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t);   m += (1 - beta1) (g - m);   v += (1 - beta2) (g g - v);
    var -= alpha m / (sqrt(v) + eps)
(restated from TensorFlow's ApplyAdam functor from memory; TensorFlow is not part of this project's tests).

Scalars, per step.  The state is (t, b1p, b2p): an integer and two Python floats (float64), (0, 1.0, 1.0) at the start.  A step
forms t' = t + 1, b1p' = b1p * float(float32(beta1)), b2p' = b2p * float(float32(beta2)): one float64 product each, no pow.
    alpha = float32( float(float32(lr)) * sqrt(1 - b2p') / (1 - b1p') )      float64, left to right, then ONE rounding to float32
    c1 = float32(1) - float32(beta1);  c2 = float32(1) - float32(beta2)      float32 subtractions
Elements, float32, one rounding per operation, nothing contracted, denormals kept, NaN and Inf wherever IEEE sends them:
    m' = m + c1 * (g - m)
    v' = v + c2 * (g * g - v)
    p' = p - (alpha * m') / (sqrt(v') + eps)

Segments.  m and v are two flat float32 buffers; tensor i's moments start at segment_offsets(counts)[i]: the prefix sum of the
counts, each rounded up to a multiple of 4.  The padding floats belong to nobody.
"""
import math

import numpy as np

F = np.float32
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-7  # tf.keras.optimizers.Adam's defaults (train.py passes lr and beta_1 = 0.9)


def adam_state0():
    """The state of an optimizer that has not stepped: (t, b1p, b2p)."""
    return (0, 1.0, 1.0)


def adam_advance(state, beta1=BETA1, beta2=BETA2):
    """The state after one more step."""
    t, b1p, b2p = state
    return (t + 1, b1p * float(F(beta1)), b2p * float(F(beta2)))


def adam_alpha(state, lr, beta1=BETA1, beta2=BETA2):
    """The float32 step size of the step that starts from `state` (it uses the ADVANCED powers)."""
    _, b1p, b2p = adam_advance(state, beta1, beta2)
    with np.errstate(all="ignore"):
        return F(np.float64(float(F(lr)) * math.sqrt(1.0 - b2p)) / np.float64(1.0 - b1p))  # (numpy: x / 0 is inf or nan, no raise)


def adam_step_ref(p, g, m, v, state, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One step on float32 arrays of one shape.  Returns (p', m', v', state'); nothing is changed in place."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    alpha = adam_alpha(state, lr, beta1, beta2)
    c1, c2, e = F(1) - F(beta1), F(1) - F(beta2), F(eps)
    with np.errstate(all="ignore"):
        m1 = (m + (c1 * (g - m)).astype(F)).astype(F)
        v1 = (v + (c2 * ((g * g).astype(F) - v).astype(F)).astype(F)).astype(F)
        p1 = (p - ((alpha * m1).astype(F) / (np.sqrt(v1).astype(F) + e).astype(F)).astype(F)).astype(F)
    return p1, m1, v1, adam_advance(state, beta1, beta2)


def segment_offsets(counts):
    """(per tensor the offset of its moments in m and in v, the floats each of m and v holds)."""
    offsets, at = [], 0
    for n in counts:
        offsets.append(at)
        at += (int(n) + 3) // 4 * 4
    return offsets, at


def same_bits(got, want):
    """Elementwise: the same float32 bits, any NaN equal to any NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what=""):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~same_bits(got, want))
    if bad.size:
        k = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r (%#x), want %r (%#x)" % (
            what, len(bad), got.size, k, got[k], got[k].view(np.uint32), want[k], want[k].view(np.uint32)))

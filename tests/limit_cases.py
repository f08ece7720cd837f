"""The cases of tests/test_gpu_pool_adam_limits.py (builders only: no tests, no fixtures, no torch at import), and what
tests/test_limit_cases.py asserts of them on the CPU.  The method is tests/conv_cases.py's part B: a batch is a tile of T = 3
frames repeated on the device, the reference (tests/pool_ref.py, tests/adam_ref.py) runs on the tile only, every period has an
odd factor, and the comparison is by bits on the device.

POOL: dtfill_max_pool_pyramid and its backward on [B, 8, 8, .] frames: x and dx past element 2^30 (byte offset 4 GiB), out2 and
      dy2 past it as the 16 channels at 16 of a 256-wide tensor, one case past 2 GiB, one at the largest B the shape rule admits
      for the 64-channel frame, and the calls that stand exactly at 2^31 elements.
ADAM: dtfill_adam_step with moments past float offsets 2^30, 2^31 and 2^32 of m and v (variables without a gradient occupy
      their segments and are never dereferenced), one variable of 2^31 - 1 floats, and the lists that are refused.
"""
import numpy as np

import adam_ref as A
import pool_ref as P
from conv_cases import POISON, T, widened  # noqa: F401 (POISON: for the tests)

F = np.float32
ERR_SHAPE = -2  # DTFILL_ERR_SHAPE
FRAME = 8  # H = W = 8: one window of the largest level a frame
LEVELS = P.LEVELS

# ---- the pool.  C channels read at xo of xc; widths / offsets: of out_k (forward) and of dy_k (backward), k = 2, 4, 8.
# levels: the levels the backward asks for (the forward asks for all three).
POOL = {
    "x and dx past 2 GiB": dict(B=2 ** 17 + T, C=64, xc=64, xo=0, widths=(64, 64, 64), offsets=(0, 0, 0), levels=(2, 4, 8), past=2 ** 29),
    "x and dx past 4 GiB": dict(B=2 ** 18 + T, C=64, xc=64, xo=0, widths=(64, 64, 64), offsets=(0, 0, 0), levels=(2, 4, 8), past=2 ** 30),
    "out2 and dy2 past 4 GiB at 16 of 256": dict(B=2 ** 18 + T, C=16, xc=16, xo=0, widths=(256, 16, 16), offsets=(16, 0, 0),
                                                 levels=(2, 4, 8), past=2 ** 30),
    "x and dx at the limit": dict(B=2 ** 19 - 1, C=64, xc=64, xo=0, widths=(64, 64, 64), offsets=(0, 0, 0), levels=(8,), past="limit"),
}

# (what is at 2^31, arguments): refused by either call
POOL_REFUSED = (
    ("B H W x_channels", dict(B=2 ** 19, C=64, xc=64, xo=0, widths=(64, 64, 64), offsets=(0, 0, 0))),
    ("B (H/2) (W/2) width_2", dict(B=2 ** 19, C=16, xc=16, xo=0, widths=(256, 16, 16), offsets=(16, 0, 0))),
    ("B (H/4) (W/4) width_4", dict(B=2 ** 19, C=16, xc=16, xo=0, widths=(16, 1024, 16), offsets=(0, 16, 0))),
    ("B (H/8) (W/8) width_8", dict(B=2 ** 19, C=16, xc=16, xo=0, widths=(16, 16, 4096), offsets=(0, 0, 16))),
)


def pool_elems(c):
    """The elements of x, dx and the three level tensors of case c."""
    n = c["B"] * FRAME * FRAME
    return dict(x=n * c["xc"], dx=n * c["C"], **{"l%d" % k: n // (k * k) * w for k, w in zip(LEVELS, c["widths"])})


def pool_device_bytes(c, backward, chunk):
    e = pool_elems(c)
    levels = sum(e["l%d" % k] for k in (c["levels"] if backward else LEVELS))
    return 4 * (e["x"] + levels + (e["dx"] if backward else 0)) + 4 * chunk


def pool_tile(c, seed=0):
    """x [T,8,8,xc] and per level the expected out_k and the dy_k (whole tensors, POISON beside the slice), and dx for the
    case's levels.  Values are the six integers -3 .. 3 without 0, so that every window has ties; frame 0 has a NaN, which wins
    its windows of every level; frame 1 has a -0 in a level-2 window of negative values, which it wins.  There is no +0, so no
    window ties the two zeros, the one pattern whose output bits the contract leaves to the order alone."""
    C, xc, xo = c["C"], c["xc"], c["xo"]
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-3, -2, -1, 1, 2, 3], F), (T, FRAME, FRAME, xc))
    x[0, 5, 2, xo + 1] = np.nan
    x[1, 2:4, 6:8, xo + 3] = -1
    x[1, 3, 6, xo + 3] = F(-0.0)
    xs = x[..., xo:xo + C]
    d = dict(x=x)
    dys = []
    for k, width, at in zip(LEVELS, c["widths"], c["offsets"]):
        d["out%d" % k] = widened(P.max_pool(xs, k), width, at)
        dy = rng.standard_normal((T, FRAME // k, FRAME // k, C)).astype(F)
        dys.append(dy if k in c["levels"] else None)
        d["dy%d" % k] = widened(dy, width, at) if k in c["levels"] else None
    d["dx"] = P.backward(xs, dys)
    return d


def pool_refused_count(a):
    n = a["B"] * FRAME * FRAME
    return max([n * a["xc"]] + [n // (k * k) * w for k, w in zip(LEVELS, a["widths"])])


# ---- Adam.  counts of the variables in order; LIVE: the ones that have a gradient.  The others are 2^30 floats each, have none,
# and are never dereferenced: they only put the live ones' segments past float offsets 2^30, 2^31 and 2^32 of m and v.
CHUNK = 4096  # DTFILL_ADAM_CHUNK
SKIP = 2 ** 30
ADAM_COUNTS = (300, SKIP, CHUNK + 5, SKIP, 2 * CHUNK + 7, SKIP, SKIP, 1001)
ADAM_LIVE = (0, 2, 4, 7)
ADAM_PARTS = {"past 4 and 8 GiB": 5, "past 16 GiB": 8}  # the variables of the call: the first 5 (m and v of 8 GiB each), all 8 (16 GiB)
ADAM_STEPS = 2

ONE_COUNT = 2 ** 31 - 1  # the largest count
ONE_ROW = 1365  # the tile's rows: 3 * 5 * 7 * 13 floats, T of them a period; a chunk of 4096 never lines up with it


def adam_values(rng, n):
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 5, n)).astype(F)


def adam_small_case(n_vars, seed=0):
    """-> (counts, offsets, floats, {i: (p0, [g of each step], p, m, v after ADAM_STEPS steps)} for the live i < n_vars, state)."""
    counts = ADAM_COUNTS[:n_vars]
    offsets, floats = A.segment_offsets(counts)
    live, state = {}, A.adam_state0()
    for i in ADAM_LIVE:
        if i >= n_vars:
            continue
        rng = np.random.default_rng(seed + i)
        p0 = adam_values(rng, counts[i])
        gs = [adam_values(rng, counts[i]) for _ in range(ADAM_STEPS)]
        p, m, v, s = p0, np.zeros(counts[i], F), np.zeros(counts[i], F), A.adam_state0()
        for g in gs:
            p, m, v, s = A.adam_step_ref(p, g, m, v, s)
        live[i], state = (p0, gs, p, m, v), s
    return counts, offsets, floats, live, state


def one_rows():
    """(rows, the floats of the last row that belong to the variable)"""
    rows = -(-ONE_COUNT // ONE_ROW)
    return rows, ONE_COUNT - (rows - 1) * ONE_ROW


def adam_one_tile(seed=0):
    """p, g, m, v [T, ONE_ROW] (v >= 0, as a second moment is) and p', m', v' after one step from the start state."""
    rng = np.random.default_rng(seed)
    p, g, m = (adam_values(rng, T * ONE_ROW).reshape(T, ONE_ROW) for _ in range(3))
    v = np.abs(adam_values(rng, T * ONE_ROW)).reshape(T, ONE_ROW)
    p1, m1, v1, state = A.adam_step_ref(p, g, m, v, A.adam_state0())
    return dict(p=p, g=g, m=m, v=v, p1=p1, m1=m1, v1=v1, state=state)


# lists dtfill_adam_step refuses and dtfill_adam_state_floats answers with 0, and the largest ones they take
ADAM_REFUSED = {
    "a count of 2^31": (2 ** 31,),
    "2^34 state floats": (2 ** 31 - 4,) * 8 + (32,),
}
ADAM_TAKEN = {
    "a count of 2^31 - 1": (2 ** 31 - 1,),
    "2^34 - 4 state floats": (2 ** 31 - 4,) * 8 + (28,),
}

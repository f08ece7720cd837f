"""dtfill_max_pool_pyramid, its backward and dtfill_adam_step past byte offset 4 GiB and at their rules' edges, by the method and
with the machinery of tests/test_gpu_conv2d_limits.py (tests/limit_cases.py has the cases, tests/test_limit_cases.py what they
are held to on the CPU).  Neither kernel has an item loop: the pool's grid is its windows, Adam's its chunks.

The pool computes size_t offsets into up to seven tensors from a deliberately 32-bit item index; k_adam places a variable's
moments at (size_t) seg4 * 4 + start, seg4 a 32-bit count of quads that the host fills.  Here x, dx, out2 and dy2 extend past
4 GiB, the batch stands at the shape rule's limit, and the moments of live variables begin just past float offsets 2^30, 2^31 and
2^32 of m and v, behind variables of 2^30 floats that have no gradient and are never dereferenced.

profiles/r33/limits.txt has every case's device bytes and duration on one MI355X.

Mutation check (each built once on a scratch copy and run once; in the same profile):
  pool_at kept to 32 bits of bytes         "out2 and dy2 past 4 GiB at 16 of 256" fails, forward (frames 0 .. 2 overwritten, 262144 ..
                                           262146 still poison) and backward; nothing else does.
  the pool's xp offset likewise            "x and dx past 4 GiB" fails forward and backward in frames 262144 .. 262146, "at the
                                           limit" from 262144 on; no test of test_gpu_max_pool.py fails in either build.
  k_adam's at as seg4 * 4 in 32 bits       "past 16 GiB" alone fails (the variable behind float offset 2^32).
  k_adam's at kept to 32 bits of bytes     "past 4 and 8 GiB", "past 16 GiB" (the variable just past 2^30) and the variable of
                                           2^31 - 1 floats (from row 786624, the first past 2^30 floats) fail; no test of
                                           test_gpu_adam.py fails in either build.
"""
import ctypes
import struct

import numpy as np
import pytest

import adam_ref as A
import large_cases as LC
import limit_cases as LM
from test_gpu_conv2d_limits import DEV, L, _release, _up, poisoned, tiled, unchanged  # noqa: F401 (L, _release: fixtures)
from test_gpu_large import need, no_mismatch

pytestmark = pytest.mark.gpu

F = np.float32
T = LM.T
N = LM.FRAME


def _ptr(t):
    return None if t is None else t.data_ptr()


_tiles = {}


def _pool_tile(name):
    if name not in _tiles:
        _tiles[name] = LM.pool_tile(LM.POOL[name])
        for a in _tiles[name].values():
            if a is not None:
                a.setflags(write=False)
    return _tiles[name]


def pool_args(c, tensors):
    """The nine level arguments of either call: pointer, width, offset of levels 2, 4, 8."""
    out = []
    for t, width, at in zip(tensors, c["widths"], c["offsets"]):
        out += [_ptr(t), width, at]
    return out


# ================================================================================================ the pool
@pytest.mark.parametrize("name", list(LM.POOL))
def test_pool_forward_past_2_gib_4_gib_and_at_the_limit(L, name):
    import torch

    c, d = LM.POOL[name], _pool_tile(name)
    B, C = c["B"], c["C"]
    for key in ("x", "out2", "out4", "out8"):
        LC.assert_alias_free(T, d[key].size // T)
    need(LM.pool_device_bytes(c, False, LC.CHUNK_BYTES), "pool forward, %s: B %d" % (name, B))
    x = tiled(d["x"], B)
    outs = [poisoned((B, N // k, N // k, w)) for k, w in zip(LM.LEVELS, c["widths"])]
    rc = L.dtfill_max_pool_pyramid(x.data_ptr(), B, N, N, C, c["xc"], c["xo"], *pool_args(c, outs), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, out in zip(LM.LEVELS, outs):  # the whole tensor of a period: the poison beside the slice must have survived
        no_mismatch(LC.mismatching_frames(out, _up(d["out%d" % k]), B), "%s: out%d" % (name, k))
    unchanged((("x", x, d["x"]),), B, name, LC.CHUNK_BYTES)


@pytest.mark.parametrize("name", list(LM.POOL))
def test_pool_backward_past_2_gib_4_gib_and_at_the_limit(L, name):
    import torch

    c, d = LM.POOL[name], _pool_tile(name)
    B, C = c["B"], c["C"]
    for key in ["x", "dx"] + ["dy%d" % k for k in c["levels"]]:
        LC.assert_alias_free(T, d[key].size // T)
    need(LM.pool_device_bytes(c, True, LC.CHUNK_BYTES), "pool backward, %s: B %d, levels %s" % (name, B, c["levels"]))
    x = tiled(d["x"], B)
    dys = [tiled(d["dy%d" % k], B) for k in LM.LEVELS]  # None for a level the case does not ask for
    dx = poisoned((B, N, N, C))
    rc = L.dtfill_max_pool_pyramid_backward(x.data_ptr(), B, N, N, C, c["xc"], c["xo"], *pool_args(c, dys), dx.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    no_mismatch(LC.mismatching_frames(dx, _up(d["dx"]), B), name + ": dx")
    unchanged([("x", x, d["x"])] + [("dy%d" % k, t, d["dy%d" % k]) for k, t in zip(LM.LEVELS, dys)], B, name, LC.CHUNK_BYTES)


def test_pool_calls_at_2_to_the_31_elements_are_refused(L):
    """Exactly 2^31 elements of x and of each level's tensor, forward and backward: DTFILL_ERR_SHAPE before any launch, so that
    small real buffers serve.  The calls just below the rule for x, which must run, are the "at the limit" cases above."""
    import torch

    bufs = [torch.zeros(4096, dtype=torch.float32, device=DEV) for _ in range(5)]
    x, dx, lv = bufs[0], bufs[1], bufs[2:]
    for what, a in LM.POOL_REFUSED:
        assert LM.pool_refused_count(a) == 2 ** 31
        head = (x.data_ptr(), a["B"], N, N, a["C"], a["xc"], a["xo"])
        assert L.dtfill_max_pool_pyramid(*head, *pool_args(a, lv), None) == LM.ERR_SHAPE, what
        assert L.dtfill_max_pool_pyramid_backward(*head, *pool_args(a, lv), dx.data_ptr(), None) == LM.ERR_SHAPE, what
    torch.cuda.synchronize()
    assert not any(t.any() for t in bufs)


# ================================================================================================ Adam
def _ll(counts):
    return (ctypes.c_longlong * len(counts))(*counts)


def _record(L):
    import torch

    rec = torch.zeros(3, dtype=torch.int64, device=DEV)
    assert L.dtfill_adam_record_bytes() == 24 and L.dtfill_adam_init(rec.data_ptr(), None) == 0
    return rec


def _all_poison(t, what, chunk=1 << 28):
    """Every 4 bytes of t are 0xFFFFFFFF, compared on the device in chunks."""
    import torch

    bits = t.view(torch.int32)
    for i in range(0, bits.numel(), chunk):
        bad = torch.nonzero(bits[i:i + chunk] != -1)
        assert not bad.numel(), "%s: float %d is no longer poison (%d in its chunk)" % (what, i + int(bad[0]), bad.numel())


@pytest.mark.parametrize("part", list(LM.ADAM_PARTS))
def test_adam_moments_past_4_8_and_16_gib(L, part):
    """Live variables (300 floats to two chunks and seven, one count no multiple of 4) before and behind variables of 2^30 floats
    that have no gradient: their moments begin just past float offsets 2^30 and 2^31 of m and v ("past 4 and 8 GiB": five
    variables, two buffers of 8 GiB) and 2^32 ("past 16 GiB": all eight, two buffers of 16 GiB, seg4 past 2^30).  Two steps.
    m and v are poisoned first; the live segments must be adam_ref's, and every other byte of m and v, the padding floats of the
    live segments included, must still be poison afterwards."""
    import torch

    n = LM.ADAM_PARTS[part]
    counts, offsets, floats, live, state = LM.adam_small_case(n)
    assert floats == L.dtfill_adam_state_floats(_ll(counts), n)
    need(2 * 4 * floats + 5 * (1 << 28), "adam, %s: %d variables, %d live, m and v of %d floats each" % (part, n, len(live), floats))
    m, v = (LC.poison_bits(torch.empty(floats, dtype=torch.float32, device=DEV)) for _ in range(2))
    assert m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
    for i in live:
        m[offsets[i]:offsets[i] + counts[i]] = 0
        v[offsets[i]:offsets[i] + counts[i]] = 0
    rec = _record(L)
    p = {i: _up(live[i][0]) for i in live}
    g = {i: [_up(a) for a in live[i][1]] for i in live}
    anyone = p[0].data_ptr()  # a skipped variable's parameter must not be NULL and is not dereferenced
    for step in range(LM.ADAM_STEPS):
        rc = L.dtfill_adam_step((ctypes.c_void_p * n)(*(p[i].data_ptr() if i in live else anyone for i in range(n))),
                                (ctypes.c_void_p * n)(*(g[i][step].data_ptr() if i in live else None for i in range(n))),
                                _ll(counts), n, m.data_ptr(), v.data_ptr(), rec.data_ptr(), A.LR, A.BETA1, A.BETA2, A.EPS, None)
        assert rc == 0, rc
    torch.cuda.synchronize()
    for i in live:
        at, c = offsets[i], counts[i]
        assert at >= (i // 2) * 2 ** 30 and (i < 7 or at >= 2 ** 32)
        A.assert_same(p[i].cpu().numpy(), live[i][2], "%s: p[%d]" % (part, i))
        A.assert_same(m[at:at + c].cpu().numpy(), live[i][3], "%s: m[%d] at float %d" % (part, i, at))
        A.assert_same(v[at:at + c].cpu().numpy(), live[i][4], "%s: v[%d] at float %d" % (part, i, at))
        for k, a in enumerate(live[i][1]):
            assert torch.equal(g[i][k], _up(a)), "a gradient was written"
        LC.poison_bits(m[at:at + c])
        LC.poison_bits(v[at:at + c])
    _all_poison(m, part + ": m outside the live segments")
    _all_poison(v, part + ": v outside the live segments")
    assert struct.unpack("<qdd", rec.cpu().numpy().tobytes()) == state


def test_adam_one_variable_of_2_to_the_31_minus_1_floats(L):
    """The largest count: p, g, m and v of 8 GiB each, 2^19 chunks, the last one a float short (1023 quads and three floats).
    The arrays are a tile of three rows of 1365 floats repeated, so a chunk never lines up with the period; one step; the
    floats behind the count, which complete the last row, must stay as they were."""
    import torch

    d = LM.adam_one_tile()
    rows, last = LM.one_rows()
    count = LM.ONE_COUNT
    LC.assert_alias_free(T, LM.ONE_ROW)
    assert L.dtfill_adam_state_floats(_ll([count]), 1) == count + 1
    need(4 * 4 * rows * LM.ONE_ROW + 4 * LC.CHUNK_BYTES, "adam, one variable of 2^31 - 1 floats")
    p, g, m, v = (tiled(d[k], rows) for k in ("p", "g", "m", "v"))
    rec = _record(L)
    rc = L.dtfill_adam_step((ctypes.c_void_p * 1)(p.data_ptr()), (ctypes.c_void_p * 1)(g.data_ptr()), _ll([count]), 1, m.data_ptr(),
                            v.data_ptr(), rec.data_ptr(), A.LR, A.BETA1, A.BETA2, A.EPS, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, t, before, after in (("p", p, d["p"], d["p1"]), ("m", m, d["m"], d["m1"]), ("v", v, d["v"], d["v1"])):
        no_mismatch(LC.mismatching_frames(t[:rows - 1], _up(after), rows - 1), "one variable: " + name)
        want = np.concatenate([after[(rows - 1) % T][:last], before[(rows - 1) % T][last:]])
        A.assert_same(t[rows - 1].cpu().numpy(), want, "one variable: the last row of " + name)
    unchanged((("g", g, d["g"]),), rows, "one variable", LC.CHUNK_BYTES)
    assert struct.unpack("<qdd", rec.cpu().numpy().tobytes()) == d["state"]


def test_adam_lists_past_the_rule_are_refused_without_an_allocation(L):
    """A count of 2^31 and a list of 2^34 state floats: DTFILL_ERR_SHAPE before any HIP call, so the pointers are never
    dereferenced and two floats serve for all of them.  The largest lists the rule takes are sized, not run, here."""
    import torch

    small = torch.zeros(8, dtype=torch.float32, device=DEV)
    rec = _record(L)
    for what, counts in LM.ADAM_REFUSED.items():
        n = len(counts)
        assert L.dtfill_adam_state_floats(_ll(counts), n) == 0, what
        rc = L.dtfill_adam_step((ctypes.c_void_p * n)(*[small.data_ptr()] * n), (ctypes.c_void_p * n)(*[small.data_ptr() + 16] * n), _ll(counts),
                                n, small.data_ptr(), small.data_ptr(), rec.data_ptr(), A.LR, A.BETA1, A.BETA2, A.EPS, None)
        assert rc == LM.ERR_SHAPE, (what, rc)
    for what, counts in LM.ADAM_TAKEN.items():
        assert L.dtfill_adam_state_floats(_ll(counts), len(counts)) == sum((c + 3) // 4 * 4 for c in counts), what
    torch.cuda.synchronize()
    assert not small.any() and struct.unpack("<qdd", rec.cpu().numpy().tobytes()) == A.adam_state0()

"""The cases of tests/limit_cases.py, held on the CPU to what tests/test_gpu_pool_adam_limits.py relies on: the thresholds each
case passes, the shape rules it stays within, the device bytes, the alias freedom of every tiled tensor, and that the tiles show
what they are for.  Conditions on the inputs, worked out from the references alone."""
import numpy as np
import pytest

import adam_ref as A
import large_cases as LC
import limit_cases as LM
import pool_ref as P

F = np.float32
T = LM.T


def test_pool_cases_pass_their_thresholds_within_the_rule():
    for name, c in LM.POOL.items():
        e = LM.pool_elems(c)
        assert all(n < 2 ** 31 for n in e.values()), name  # the shape rule
        assert c["xo"] + c["C"] <= c["xc"] and all(o + c["C"] <= w for o, w in zip(c["offsets"], c["widths"]))
        assert LM.pool_device_bytes(c, False, LC.CHUNK_BYTES) < 20e9 and LM.pool_device_bytes(c, True, LC.CHUNK_BYTES) < 20e9, name
        frame = {k: n // c["B"] for k, n in e.items()}
        if c["past"] == "limit":  # the largest B the rule admits for the frame
            assert e["x"] < 2 ** 31 <= e["x"] + frame["x"] and e["dx"] == e["x"], name
        else:  # the last T frames of the named tensors start at or beyond the threshold, and no batch smaller does that
            big = [k for k in e if (c["B"] - T) * frame[k] >= c["past"]]
            assert big and all((c["B"] - T - 1) * frame[k] < c["past"] for k in big), name
            assert set(big) == ({"l2"} if "out2" in name else {"x", "dx"}), (name, big)
    assert LM.POOL["x and dx past 4 GiB"]["B"] == 262147 and LM.POOL["x and dx at the limit"]["B"] == 524287
    sl = LM.POOL["out2 and dy2 past 4 GiB at 16 of 256"]
    assert sl["widths"][0] == 256 and sl["offsets"][0] == 16 and sl["C"] == 16 and 2 in sl["levels"]
    assert {c["past"] for c in LM.POOL.values()} == {2 ** 29, 2 ** 30, "limit"}


def test_pool_refused_calls_stand_exactly_at_the_limit():
    for what, a in LM.POOL_REFUSED:
        assert LM.pool_refused_count(a) == 2 ** 31, what
        e = LM.pool_elems(a)
        del e["dx"]  # (dense: never more than x)
        assert sorted(e.values())[-1] == 2 ** 31 and sorted(e.values())[-2] < 2 ** 31, what  # one tensor alone is at the limit
    assert len(LM.POOL_REFUSED) == 4  # x and each level


@pytest.mark.parametrize("name", list(LM.POOL))
def test_pool_tiles_show_what_they_are_for(name):
    c = LM.POOL[name]
    d = LM.pool_tile(c)
    for key, a in d.items():
        if a is not None:
            assert a.shape[0] == T
            LC.assert_alias_free(T, a.size // T)
    xs = d["x"][..., c["xo"]:c["xo"] + c["C"]]
    assert len({d["x"][t].tobytes() for t in range(T)}) == T
    assert not (xs.view(np.uint32) == 0).any() and (xs.view(np.uint32) == 0x80000000).sum() == 1  # one -0 and no +0: no tie of the zeros
    for k, at in zip(LM.LEVELS, c["offsets"]):
        out = d["out%d" % k][..., at:at + c["C"]]
        win = xs.reshape(T, 8 // k, k, 8 // k, k, c["C"]).transpose(0, 1, 3, 5, 2, 4).reshape(out.shape + (k * k,))
        with np.errstate(invalid="ignore"):
            ties = (win == out[..., None]).sum(-1) > 1
        assert ties.mean() > 0.25, (k, ties.mean())  # the raster-first rule decides a quarter of the level-2 windows and most above
        assert np.isnan(out).sum() == 1  # the NaN wins its window at every level
        rest = np.delete(d["out%d" % k], np.s_[at:at + c["C"]], axis=-1)
        assert (rest.view(np.uint32) == LM.POISON).all()
    assert (d["out2"].view(np.uint32) == 0x80000000).sum() == 1 and not (d["out4"].view(np.uint32) == 0x80000000).any()  # the -0 wins
    # dx: exactly one winner a window and level; the terms of a pixel that wins several levels do not cancel
    dx = d["dx"]
    assert not np.isnan(dx).any() and not (dx.view(np.uint32) == 0x80000000).any()
    per_frame = sum((8 // k) ** 2 for k in c["levels"]) * c["C"]
    assert 0.5 * per_frame * T < (dx != 0).sum() <= per_frame * T
    torch_free = P.backward(xs, [None if d["dy%d" % k] is None else d["dy%d" % k][..., at:at + c["C"]] for k, at in zip(LM.LEVELS, c["offsets"])])
    assert (torch_free.view(np.uint32) == dx.view(np.uint32)).all()


def test_adam_small_variables_lie_where_the_case_says():
    for part, n in LM.ADAM_PARTS.items():
        counts, offsets, floats, live, state = LM.adam_small_case(n)
        assert floats == sum((c + 3) // 4 * 4 for c in counts) and 2 * 4 * floats < (20e9 if n == 5 else 35e9)
        assert set(live) == {i for i in LM.ADAM_LIVE if i < n} and state[0] == LM.ADAM_STEPS
        for i, (p0, gs, p, m, v) in live.items():
            assert 300 <= counts[i] <= 3 * LM.CHUNK and p0.size == counts[i] and len(gs) == LM.ADAM_STEPS
            assert (p != p0).mean() > 0.9 and (m != 0).mean() > 0.9 and (v > 0).mean() > 0.9 and np.isfinite(p).all()
        assert all(counts[i] == LM.SKIP for i in range(n) if i not in live)
    counts, offsets, floats, live, _ = LM.adam_small_case(8)
    thresholds = {2: 2 ** 30, 4: 2 ** 31, 7: 2 ** 32}  # 4, 8 and 16 GiB of floats
    for i, least in thresholds.items():
        assert least <= offsets[i] < least + 2 ** 15, (i, offsets[i])  # just past it
    assert offsets[7] // 4 > 2 ** 30 and (offsets[7] // 4 * 4) % 2 ** 32 != offsets[7]  # seg4 * 4 does not fit 32 bits
    assert any(counts[i] % 4 for i in live) and any(counts[i] > 2 * LM.CHUNK for i in live) and any(counts[i] < LM.CHUNK for i in live)
    assert LM.ADAM_PARTS["past 4 and 8 GiB"] == 5 and offsets[4] + counts[4] < 2 ** 31 + 2 ** 15  # the first part stops behind 8 GiB


def test_adam_one_variable_is_a_tile_with_an_odd_period():
    rows, last = LM.one_rows()
    assert (rows - 1) * LM.ONE_ROW + last == LM.ONE_COUNT == 2 ** 31 - 1 and 0 < last < LM.ONE_ROW
    assert LM.ONE_ROW % 2 == 1 and np.gcd(T * LM.ONE_ROW, LM.CHUNK) == 1
    assert LM.ONE_COUNT % LM.CHUNK == LM.CHUNK - 1  # the last chunk is one float short: 1023 quads and three floats
    LC.assert_alias_free(T, LM.ONE_ROW)
    d = LM.adam_one_tile()
    assert (d["v"] >= 0).all() and all(d[k].shape == (T, LM.ONE_ROW) for k in ("p", "g", "m", "v", "p1", "m1", "v1"))
    for a, b in (("p", "p1"), ("m", "m1"), ("v", "v1")):
        assert (d[a] != d[b]).mean() > 0.9 and np.isfinite(d[b]).all()
    assert len({d["p"][t].tobytes() for t in range(T)}) == T and d["state"] == A.adam_advance(A.adam_state0())


def test_adam_refused_lists_stand_exactly_at_the_rule(pkg):
    import ctypes

    floats = lambda counts: sum((c + 3) // 4 * 4 for c in counts)  # noqa: E731
    assert LM.ADAM_REFUSED["a count of 2^31"] == (2 ** 31,) and LM.ADAM_TAKEN["a count of 2^31 - 1"] == (2 ** 31 - 1,)
    assert floats(LM.ADAM_REFUSED["2^34 state floats"]) == 2 ** 34 and floats(LM.ADAM_TAKEN["2^34 - 4 state floats"]) == 2 ** 34 - 4
    assert all(c < 2 ** 31 for c in LM.ADAM_REFUSED["2^34 state floats"])
    S = pkg._lib.load().dtfill_adam_state_floats  # the size function needs no GPU
    for counts in LM.ADAM_REFUSED.values():
        assert S((ctypes.c_longlong * len(counts))(*counts), len(counts)) == 0
    for counts in LM.ADAM_TAKEN.values():
        assert S((ctypes.c_longlong * len(counts))(*counts), len(counts)) == floats(counts)

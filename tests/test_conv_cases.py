"""The cases of tests/conv_cases.py, held on the CPU to what tests/test_gpu_conv2d_limits.py relies on: the item counts of part A,
the sizes and the alias freedom of every tiled case, references without a zero, and, for the value classes of part C, that the
reference itself shows what each class is for.  These are conditions on the inputs, worked out from the references alone."""
import numpy as np
import pytest

import conv_cases as CC
import conv_ref as R
import convb_ref as RB
import large_cases as LC

F = np.float32



def test_loop_cases_lie_just_past_the_grid_limit():
    """The table's item counts, recomputed from the tile constants: in (2^20, 2^20 + 2^10), so that most blocks take one item
    and some a second one; and the geometry the table asks for."""
    for name, c in CC.LOOP.items():
        n = CC.items(c)
        assert CC.MAX_BLOCKS < n < CC.MAX_BLOCKS + 2 ** 10, (name, n)
        assert 24 <= n - CC.MAX_BLOCKS, (name, n)  # "a few dozen to a few hundred"
        assert c["H"] * c["W"] <= CC.TILE_H * CC.TILE_W  # a handful of pixels up to one tile
    by_body = lambda key: [CC.tiles(c) for c in CC.LOOP.values() if c["body"].startswith(key)]  # noqa: E731
    for key in ("k_conv_mfma", "k_conv_wide"):
        assert any(ty > 1 for ty, _ in by_body(key)) and any(tx > 1 for _, tx in by_body(key)), key
        assert any(c.get("misaligned") for c in CC.LOOP.values() if c["body"].startswith(key)), key
    assert any(sx > 1 for _, sx in by_body("k_convb_dw"))
    # a second item that differs from the block's first in more than its frame: the items of a frame do not divide the grid
    for key in ("k_conv_mfma", "k_conv_wide", "k_convb_dw"):
        assert any(CC.MAX_BLOCKS % CC.items_per_frame(c) for c in CC.LOOP.values() if key in c["body"]), key
    assert {c["body"] for c in CC.LOOP.values()} >= {"k_conv_mfma<3,false>", "k_conv_mfma<7,true>", "k_conv_wide<ConvPlain<3,1>>",
                                                     "k_conv_wide<ConvPlain<3,2>>", "k_conv_wide<ConvTransposed>", "k_convb_dw<1,false>",
                                                     "k_convb_dw<3,true>"}
    wide = CC.LOOP["strided 3x3x16->128 residual"]
    assert wide["cout"] // CC.PASS_CHANNELS == 2 and wide["residual"]  # npass = 2
    assert CC.LOOP["dx 3x3x16->16"]["B"] == CC.LOOP["conv2d 3x3x16->16"]["B"]


def test_loop_cases_stay_under_3_gb():
    """Every case but two, which the backward's workspace rule keeps above it: either backward call asks for the larger of the
    data gradient's workspace (g, B H W Cout floats) and the weight gradient's (a row of ksize^2 Cin + 1 partials of Cout
    floats a segment), whichever gradient it computes.
      dw 3x3x1->16 with segs_x > 1: 2^20 segments, two a frame, are 2^19 frames of at least 65 pixels; dy is 2^19 * 65 * 16
                    floats = 2.18 GB and g's workspace the same again;
      dx 3x3x16->16 at the first row's B = 349559: a segment a frame, 145 * 16 floats each, are 3.24 GB of workspace.
    Their floors are worked out here, and each stays within 0.4 GB (x, the comparison's scratch) and 1.3 GB (dy, y and dx) of its."""
    floors = {"dw 3x3x1->16": (2 * 4 * 2 ** 19 * (CC.SEG_COLS + 1) * 16, 0.4e9), "dx 3x3x16->16": (4 * CC.LOOP["conv2d 3x3x16->16"]["B"] * (9 * 16 + 1) * 16, 1.3e9)}
    for name, c in CC.LOOP.items():
        if name in floors:
            floor, slack = floors[name]
            assert floor > 3e9 and CC.device_bytes(c) < floor + slack, (name, CC.device_bytes(c))
            assert CC.workspace_bytes(c) >= floor // (2 if name.startswith("dw") else 1)
        else:
            assert CC.device_bytes(c) <= 3e9, (name, CC.device_bytes(c))


def test_large_cases_pass_their_thresholds():
    for name, c in CC.LARGE.items():
        B, by = c["B"], c["by"]
        if c["past"] == "limit":
            assert 2 ** 31 - by <= B * by < 2 ** 31, name  # within one frame of 2^31
            assert 4 * B * by > 8e9
        else:
            assert (B - CC.T) * by >= c["past"] > (B - CC.T - 1) * by, name  # the last T frames start beyond the threshold
        n = B * c["H"] * c["W"]
        Ho, Wo = (c["H"], c["W"]) if c["entry"] in ("dx", "dw") else CC.out_frame(c)
        widest = max(c["cin"], c.get("width", 0)) if c["entry"] in ("dx", "dw") else c["cin"]
        assert n * widest < 2 ** 31 and B * Ho * Wo * max(c["cout"], c.get("out_channels", 0)) < 2 ** 31, name  # the shape rule
    past4 = lambda e: [c for c in CC.LARGE.values() if c["entry"] == e and c["past"] == 2 ** 30]  # noqa: E731
    assert all(past4(e) for e in ("conv2d", "strided", "transpose", "dx", "dw"))
    dx = past4("dx")[0]
    assert dx["by"] == dx["H"] * dx["W"] * dx["width"] == dx["H"] * dx["W"] * dx["cin"] and dx["at"] > 0  # dy, y and dx alike
    out = CC.LARGE["strided 1x1x16->64 at 16 of 80, out and residual past 4 GiB"]
    assert out["by"] == out["H"] * out["W"] * out["cout"] and out["out_offset"] > 0 and out["out_channels"] > out["cout"] + out["out_offset"] - 1
    for c in past4("dw"):  # dy and y as wide as x: they pass 4 GiB with it
        assert c["width"] * c["H"] * c["W"] == c["by"] and c["at"] > 0 and c["act"] == R.LEAKY
    lane = CC.LARGE["dw 3x3x16->1, x past 2 GiB, dy past 4 GiB"]
    assert lane["cout"] == 1 and (lane["B"] - CC.T) * lane["H"] * lane["W"] * lane["width"] >= 2 ** 30 and lane["at"] > 0
    limits = {n for n, c in CC.LARGE.items() if c["past"] == "limit"}
    assert len(limits) == 3  # x, out by out_channels, dy and y by their width: each rule has a call just below it that runs


def test_refused_calls_stand_exactly_at_the_limit():
    for entry, what, a in CC.REFUSED:
        assert CC.refused_count(entry, a) == 2 ** 31, (entry, what)
        assert a["B"] * a["H"] * a["W"] < 2 ** 31
    assert {(e, w.split()[-1]) for e, w, _ in CC.REFUSED} >= {("conv2d", "Cin"), ("strided", "Cout"), ("conv2d", "out_channels"),
                                                             ("dx", "dy_channels"), ("dw", "y_channels"), ("dx", "dx_channels")}


@pytest.fixture(scope="module", params=[("LOOP", n) for n in CC.LOOP] + [("LARGE", n) for n in CC.LARGE], ids=lambda p: "%s: %s" % p)
def tiled(request):
    table, name = request.param
    c = getattr(CC, table)[name]
    return c, CC.tile(c)


def test_tiles_are_alias_free_and_have_no_zero_output(tiled):
    c, d = tiled
    for what, period in CC.periods(c, d):
        assert period % CC.T == 0
        LC.assert_alias_free(CC.T, period // CC.T)
    want = d["want"]
    if c["entry"] == "dw":  # compared on the host, where a zero's sign is left open; the sums must still be sums of something
        dw, db = CC.split_dw(CC.level2(want, 4 * len(want)), c["ksize"], c["cin"])
        assert (dw[c["ksize"] // 2] != 0).mean() > 0.9 and (db != 0).all() and np.isfinite(dw).all()  # (H = 1: the middle row of taps)
    else:
        assert (want != 0).all() and not np.isnan(want[..., c.get("out_offset", 0):c.get("out_offset", 0) + c["cout"]]).any()
    for k in ("x", "dy", "y", "residual"):
        if d.get(k) is not None:
            assert d[k].shape[0] == CC.T and len({d[k][t].tobytes() for t in range(CC.T)}) == CC.T, k  # T distinct frames


def test_level2_is_dw_ref_on_the_tiled_batch():
    """level2 over a tile's partials repeated is convb_ref.dw_ref of the batch written out."""
    c = dict(CC.LOOP["dw 1x1x32->16"], B=7)
    d = CC.tile(c)
    reps = lambda a: np.concatenate([a] * 3)[:7]  # noqa: E731
    at, cout = d["at"], c["cout"]
    dw, db = RB.dw_ref(reps(d["x"]), reps(d["dy"])[..., at:at + cout], reps(d["y"])[..., at:at + cout], c["ksize"], c["act"], CC.ALPHA)
    got_dw, got_db = CC.split_dw(CC.level2(d["want"], 7), c["ksize"], c["cin"])
    assert (got_dw.view(np.uint32) == dw.view(np.uint32)).all() and (got_db.view(np.uint32) == db.view(np.uint32)).all()


# ---- part C: what each class is for, as a share of the reference's outputs

def _share(mask):
    return float(np.mean(mask))


RUNS = tuple(enumerate(CC.SMALL_SHAPES))  # (seed, shape) as tests/test_gpu_conv2d_limits.py runs them


@pytest.mark.parametrize("entry,ksize,cin,cout,stride", CC.FORWARD_LAYERS)
@pytest.mark.parametrize("name", list(CC.CLASSES))
def test_forward_classes_show_what_they_are_for(name, entry, ksize, cin, cout, stride):
    for seed, shape in RUNS:
        x, w, b = CC.class_case(name, ksize, cin, cout, shape, seed, entry)
        want = CC.forward_ref(entry, x, w, b, stride)
        assert not np.isnan(want).any()
        if name in ("subnormal x", "subnormal w"):
            sub = x if name == "subnormal x" else w
            assert _share(CC.is_subnormal(sub)) > 0.9
            other = CC.forward_ref(entry, CC.flushed(x), CC.flushed(w), b, stride)
            assert _share(CC.is_normal(want) & (want.view(np.uint32) != other.view(np.uint32))) >= 0.9  # normal, and from subnormals
        elif name == "straddling":
            assert _share(CC.is_subnormal(want)) >= 0.1 and _share(CC.is_normal(want)) >= 0.1, (seed, shape)
        elif name == "tiny":
            assert _share(CC.is_subnormal(want)) >= 0.9
        elif name == "huge":
            assert _share(np.isinf(want)) >= 0.1 and _share(np.isfinite(want)) >= 0.1, (seed, shape, _share(np.isinf(want)))
        else:  # leaky; one output channel is of one kind a run: the underflow under the even seed, the overflow under the odd one
            acc, y = CC.forward_ref(entry, x, w, None, stride, R.LINEAR), CC.forward_ref(entry, x, w, b, stride, R.LINEAR)
            under = _share(CC.is_subnormal(want) & CC.is_normal(y))  # y * alpha underflows
            over = _share(np.isinf(want) & np.isfinite(acc))  # the bias add overflows
            beside = _share(np.isfinite(want) & (np.abs(want) > 1e38))  # and does not, beside it
            if cout > 1:
                assert under >= 0.1 and over >= 0.1 and beside >= 0.1, (seed, shape, under, over, beside)
            elif seed % 2 == 0:
                assert under >= 0.1, (seed, shape, under)
            else:
                assert over >= 0.1 and beside >= 0.1, (seed, shape, over, beside)
    assert len(RUNS) == 2  # Cout == 1: both kinds are run


@pytest.mark.parametrize("name", ("straddling", "huge"))
def test_order_sensitive_classes_tell_the_orders_apart(name):
    """3x3x32->16, two groups: the contract's order against the tap-outermost one."""
    for seed, shape in RUNS:
        x, w, b = CC.class_case(name, 3, 32, 16, shape, seed)
        groups, taps = R.conv_ref(x, w, b, R.LEAKY, CC.ALPHA), R.conv_ref(x, w, b, R.LEAKY, CC.ALPHA, order="taps")
        assert _share(groups.view(np.uint32) != taps.view(np.uint32)) >= 0.1
        if name == "huge":
            assert _share(np.isfinite(groups) != np.isfinite(taps)) >= 0.02, (seed, shape)


@pytest.mark.parametrize("ksize,cin,cout", CC.BACKWARD_LAYERS)
@pytest.mark.parametrize("name", CC.BACKWARD_CLASSES)
def test_backward_classes_show_what_they_are_for(name, ksize, cin, cout):
    for seed, shape in RUNS:
        x, w, y, dy_dx, dy_dw = CC.backward_class_case(name, ksize, cin, cout, shape, seed)
        dx = RB.dx_ref(dy_dx, y, w, R.LEAKY, CC.ALPHA)
        dw, db = RB.dw_ref(x, dy_dw, y, ksize, R.LEAKY, CC.ALPHA)
        # (two frames of "huge": level 2 adds a partial of +inf to one of -inf, a NaN that the device must make too)
        assert not np.isnan(dx).any() and (not np.isnan(dw).any() or (name == "huge" and shape[0] > 1))
        assert 0.2 < _share(y > 0) < 0.8  # both branches of g
        if name in ("subnormal x", "subnormal w"):
            fdx = RB.dx_ref(CC.flushed(dy_dx), y, CC.flushed(w), R.LEAKY, CC.ALPHA)
            fdw, _ = RB.dw_ref(CC.flushed(x), CC.flushed(dy_dw), y, ksize, R.LEAKY, CC.ALPHA)
            for got, other in ((dx, fdx), (dw, fdw)):
                assert _share(CC.is_normal(got) & (got.view(np.uint32) != other.view(np.uint32))) >= 0.9
        elif name == "straddling":
            for got in (dx, dw):
                assert _share(CC.is_subnormal(got)) >= 0.1 and _share(CC.is_normal(got)) >= 0.1, (seed, shape)
        elif name == "tiny":
            assert _share(CC.is_subnormal(dx)) >= 0.9 and _share(CC.is_subnormal(dw)) >= 0.9
        else:
            for what, got in (("dx", dx), ("dw", dw)):
                assert _share(np.isinf(got)) >= 0.1 and _share(np.isfinite(got)) >= 0.1, (seed, shape, what, _share(np.isinf(got)))


# ================================================================================================ the bf16 calls
import conv_bf16_ref as HB  # noqa: E402


def test_bf16_loop_cases_lie_just_past_the_grid_limit():
    """As for LOOP: a hundred items past 2^20 on tiny frames; all five geometries at Cin = Cout = 16; a half group with two
    groups an item; two passes with a residual; a stride-2 and the transposed case again off the 16-byte path; and a frame
    whose items do not divide the grid in every geometry but the two-pass one."""
    for name, c in CC.HLOOP.items():
        n = CC.items(c)
        assert CC.MAX_BLOCKS + 24 <= n < CC.MAX_BLOCKS + 2 ** 10, (name, n)
        assert c["H"] * c["W"] <= CC.TILE_H * CC.TILE_W and c["bf16"]
        assert CC.device_bytes(c) <= 3e9, (name, CC.device_bytes(c))
    bodies = {c["body"] for c in CC.HLOOP.values()}
    assert bodies == {"k_convh_wide<ConvPlain<%s>>" % g for g in ("1,1", "3,1", "1,2", "3,2")} | {"k_convh_wide<ConvTransposed>"}
    for body in bodies:
        cases = [c for c in CC.HLOOP.values() if c["body"] == body]
        assert any(c["cin"] == 16 and c["cout"] == 16 for c in cases) or body == "k_convh_wide<ConvPlain<3,1>>", body
        assert any(CC.MAX_BLOCKS % CC.items_per_frame(c) for c in cases), body  # item k + 2^20 is another tile, parity or pass
    assert {CC.items_per_frame(c) for c in CC.HLOOP.values()} >= {3, 12}
    half = CC.HLOOP["bf16 3x3x48->16"]
    assert half["cin"] % HB.GROUP == 16 and -(-half["cin"] // HB.GROUP) == 2
    wide = CC.HLOOP["bf16 3x3x16->128 residual"]
    assert wide["cout"] // CC.PASS_CHANNELS == 2 and wide["residual"]
    off = [c for c in CC.HLOOP.values() if c.get("misaligned")]
    assert any(c.get("stride") == 2 for c in off) and any(c["entry"] == "transpose" for c in off)


def test_bf16_large_cases_pass_their_thresholds():
    for name, c in CC.HLARGE.items():
        B, by = c["B"], c["by"]
        if c["past"] == "limit":
            assert 2 ** 31 - by <= B * by < 2 ** 31 and 4 * B * by > 8e9, name
        else:
            assert (B - CC.T) * by >= c["past"] > (B - CC.T - 1) * by, name
        Ho, Wo = CC.out_frame(c)
        x_elems, out_elems = c["H"] * c["W"] * c["cin"], Ho * Wo * c.get("out_channels", c["cout"])
        assert by in (x_elems, out_elems, Ho * Wo * c["cout"]), name  # `by` is a frame of a tensor of the call
        assert B * x_elems < 2 ** 31 and B * out_elems < 2 ** 31, name  # the shape rule
        assert CC.device_bytes(c, LC.CHUNK_BYTES) < 20e9, (name, CC.device_bytes(c, LC.CHUNK_BYTES))
    for entry in ("strided", "transpose"):
        mine = {c["past"] for c in CC.HLARGE.values() if c["entry"] == entry}
        assert mine == {2 ** 29, 2 ** 30, "limit"}, entry
    past4 = lambda frame: [n for n, c in CC.HLARGE.items() if (c["B"] - CC.T) * frame(c) >= 2 ** 30]  # noqa: E731
    x4 = past4(lambda c: c["H"] * c["W"] * c["cin"])
    assert any("strided" in n for n in x4) and any("transpose" in n for n in x4)
    out4 = past4(lambda c: CC.out_frame(c)[0] * CC.out_frame(c)[1] * c["cout"])
    assert any("transpose" in n for n in out4)
    sl = CC.HLARGE["bf16 strided 1x1x16->64 at 16 of 80, out and residual past 4 GiB"]
    assert sl in [CC.HLARGE[n] for n in out4] and sl["residual"] and sl["out_offset"] == 16 and sl["out_channels"] == 80


def test_bf16_refused_calls_stand_exactly_at_the_limit():
    for entry, what, a in CC.HREFUSED:
        assert CC.refused_count(entry, a) == 2 ** 31, (entry, what)
        assert a["B"] * a["H"] * a["W"] < 2 ** 31 and a["cin"] % 16 == 0 and a["cout"] % 16 == 0 and a["ksize"] in (1, 3)
    assert {(e, w.split()[-1]) for e, w, _ in CC.HREFUSED} == {(e, t) for e in ("strided", "transpose") for t in ("Cin", "Cout", "out_channels")}


@pytest.fixture(scope="module", params=[("HLOOP", n) for n in CC.HLOOP] + [("HLARGE", n) for n in CC.HLARGE], ids=lambda p: "%s: %s" % p)
def htiled(request):
    table, name = request.param
    c = getattr(CC, table)[name]
    return c, CC.tile(c)


def test_bf16_tiles_are_exact_alias_free_and_have_no_zero_output(htiled):
    c, d = htiled
    for what, period in CC.periods(c, d):
        assert period % CC.T == 0
        LC.assert_alias_free(CC.T, period // CC.T)
    at, cout = c.get("out_offset", 0), c["cout"]
    want = d["want"][..., at:at + cout]
    assert (want != 0).all() and np.isfinite(want).all() and (want * 4 == np.rint(want * 4)).all()
    rest = np.delete(d["want"], np.s_[at:at + cout], axis=-1)
    assert (rest.view(np.uint32) == CC.POISON).all()
    for k in ("x", "w", "residual"):
        if d.get(k) is not None:
            assert (HB.bf16_round(d[k]) == d[k]).all() and (d[k] == np.rint(d[k])).all(), k  # integers that bf16 holds
    assert (d["bias"] * 2 % 2 == 1).all()  # odd multiples of 0.5: no sum is a zero
    # every partial sum in any order is an integer below 2^24 in magnitude: the contract's "exact" clause applies
    assert 8 * 4 * HB.bound_terms(c["ksize"], c["cin"]) + 9 + 9 < 2 ** 24
    for k in ("x", "residual"):
        if d.get(k) is not None:
            assert len({d[k][t].tobytes() for t in range(CC.T)}) == CC.T, k
    # and the tile's expectation is the statement's (the float64 sum, the float32 finish)
    ref = HB.conv2d_transpose_bf16_ref(d["x"], d["w"], d["bias"], R.LEAKY, CC.HALPHA)[0] if c["entry"] == "transpose" else \
        HB.conv2d_strided_bf16_ref(d["x"], d["w"], d["bias"], c["stride"], d["residual"], R.LEAKY, CC.HALPHA)[0]
    assert (ref.view(np.uint32) == want.view(np.uint32)).all()


# ---- part C of the bf16 calls: what each class is for
def _hsums(x, w, stride, transposed):
    xr, wr = HB.bf16_round(x), HB.bf16_round(w)
    if transposed:
        return HB.transpose_sum(xr, wr), HB.transpose_sum(np.abs(xr), np.abs(wr))
    return HB.strided_sum(xr, wr, stride), HB.strided_sum(np.abs(xr), np.abs(wr), stride)


@pytest.mark.parametrize("ksize,stride,transposed,cin,cout", CC.HLAYERS, ids=CC.HLAYER_IDS)
@pytest.mark.parametrize("name", list(CC.HCLASSES))
def test_bf16_classes_show_what_they_are_for(name, ksize, stride, transposed, cin, cout):
    n, fmax = HB.bound_terms(ksize, cin), CC.FLT_MAX
    for seed, shape in RUNS:
        x, w, b = CC.hclass_case(name, ksize, cin, cout, shape, seed, stride, transposed)
        total, S = _hsums(x, w, stride, transposed)
        if name == "near the top":  # S in its window; the rounding is left to the kernel, so some operands are no bf16 values
            assert fmax / 8 <= S.max() < fmax / 2, (seed, shape, S.max() / fmax)
            assert _share(HB.bf16_round(x) != x) > 0.9 and np.isfinite(HB.bf16_round(x)).all() and np.isfinite(HB.bf16_round(w)).all()
            assert np.abs(b).max() < fmax / 2 ** 10  # the finish cannot overflow either
            continue
        assert (HB.bf16_round(x) == x).all() and (HB.bf16_round(w) == w).all()  # the reference's operands are the kernel's
        if name == "over the top":  # one sign, and the exact sum beyond FLT_MAX by more than the bound, either sign of w
            assert (x > 0).all() and (w > 0).all() and (total == S).all()
            assert (S - HB.bound(ksize, cin, S) > 2.0 ** 128).all(), (seed, shape, S.min() / fmax)
            xn, wn, _ = CC.hclass_case(name, ksize, cin, cout, shape, seed, stride, transposed, -1)
            assert (xn == x).all() and (wn == -w).all()
        elif name in ("small products", "tiny products"):  # normal operands; a tenth of the products inexact in float32
            assert CC.is_normal(x).all() and CC.is_normal(w).all()
            p = x.reshape(-1, 1, cin, 1).astype(np.float64) * w.reshape(1, ksize * ksize, cin, cout).astype(np.float64)
            assert _share(p.astype(F).astype(np.float64) != p) >= 0.1, (seed, shape)
            if name == "small products":  # sums from 2^-149 to 2^-120, on either side of 2^-126
                assert _share((np.abs(total) >= 2.0 ** -149) & (np.abs(total) < 2.0 ** -120)) >= 0.9
                assert _share(np.abs(total) < 2.0 ** -126) >= 0.1 and _share(np.abs(total) >= 2.0 ** -126) >= 0.1
            else:  # no partial sum in any order reaches 2^-126, and the sums are no zeros
                assert S.max() < 2.0 ** -126 and b is None and _share(np.abs(total) >= 2.0 ** -149) >= 0.9
        else:  # subnormal operands that survive the rounding, and two references further apart than their bounds together
            sub = x if name == "subnormal x" else w
            assert _share(CC.is_subnormal(sub)) >= 0.5
            ftotal, fS = _hsums(CC.flushed(x), CC.flushed(w), stride, transposed)
            apart = np.abs(total - ftotal) > HB.bound(ksize, cin, S, b) + HB.bound(ksize, cin, fS, b)
            assert _share(apart) >= 0.1, (seed, shape, _share(apart))


# ================================================================================================ the newer backward kernels
def test_wide_loop_cases_reach_the_second_launch_and_the_second_item():
    wide = {n: c for n, c in CC.WLOOP.items() if c["entry"] == "dw_wide"}
    for name, c in wide.items():
        _, (Hs, Ws) = CC.wframes(c)
        assert (Hs, Ws) == (1, 129) and CC.wsegments(c) == 3 * c["B"] == 65637 == CC.GRID_Z + 102, name
        assert CC.GRID_Z % 3 == 0 and CC.GRID_Z // 3 == 21845  # segment 65535 is column 0 of frame 21845 ...
        assert (CC.wsegments(c) - CC.GRID_Z) == 102 and Ws % CC.SEG_COLS == 1  # ... and the last segment of a frame has one column
        assert c["cin"] in (16, 32) and c["cout"] == 32
    # one call for each instantiation dtfill.hip asks convb_dw_wide_launch for
    assert {(c["ksize"], c["stride"], c["transposed"]) for c in wide.values()} == {(1, 1, False), (3, 1, False), (5, 1, False), (7, 1, False),
                                                                                    (1, 2, False), (3, 2, False), (3, 2, True)}
    dx = {n: c for n, c in CC.WLOOP.items() if c["entry"] == "dx_wide"}
    assert {(c["ksize"], c["stride"], c["transposed"]) for c in dx.values()} == {(1, 2, False), (3, 2, True)}  # k_convb_spread; the transposed one
    image = {n: c for n, c in CC.WLOOP.items() if c["entry"] == "dw_image"}
    for name, c in image.items():
        assert CC.MAX_BLOCKS + 24 <= CC.witems(c) < CC.MAX_BLOCKS + 2 ** 10 and c["H"] * c["W"] <= 5, name
        assert CC.wsegments(c) == c["B"]  # one segment a frame
    assert {(c["ksize"], c["cin"], c["cout"]) for c in image.values()} == {(3, 3, 16), (7, 4, 16), (3, 3, 128)}
    two = image["dw image 3x3x3->128"]
    assert CC.witems(two) == 2 * two["B"] and CC.MAX_BLOCKS % 2 == 0  # item k + 2^20 is the same pass of another segment ...
    assert (7 * 7 * 4 + 16) // 16 == 13  # thirteen row tiles


def test_wide_loop_cases_stay_under_3_gb_or_at_their_floor():
    """Every case stays under 3 GB but six whose workspace the rule itself puts above it, at the smallest channels the issue's
    shapes allow: a row of ksize^2 Cin + 1 partials of Cout floats a segment (5x5 and 7x7 at Cin 16, Cout 32 over 65637 segments;
    the image layers over 2^20 segments at Cout 16 and 2^19 at Cout 128), and for the transposed layer g beside dy, both
    B 2H 2W Cout floats.  Each stays within 1 GB of its floor."""
    floors = {"dw wide 5x5x16->32": 4 * 65637 * (25 * 16 + 1) * 32, "dw wide 7x7x16->32": 4 * 65637 * (49 * 16 + 1) * 32,
              "dw wide transposed 16->32": 2 * 4 * 21879 * 2 * 258 * 32, "dx wide transposed 16->32": 2 * 4 * 21879 * 2 * 258 * 32,
              "dw image 7x7x4->16": 4 * (2 ** 20 + 101) * (49 * 4 + 1) * 16, "dw image 3x3x3->128": 4 * (2 ** 19 + 50) * 28 * 128}
    for name, c in CC.WLOOP.items():
        if name in floors:
            assert floors[name] > 2.8e9 and floors[name] <= CC.wdevice_bytes(c) < floors[name] + 1e9, (name, CC.wdevice_bytes(c))
        else:
            assert CC.wdevice_bytes(c) <= 3e9, (name, CC.wdevice_bytes(c))
        assert CC.wworkspace_bytes(c) % 256 == 0


@pytest.fixture(scope="module", params=list(CC.WLOOP))
def wtiled(request):
    c = CC.WLOOP[request.param]
    return c, CC.wtile(c)


def test_wide_loop_tiles_are_alias_free_and_their_sums_are_sums_of_something(wtiled):
    c, d = wtiled
    for key in ("x", "dy", "y"):
        assert d[key].shape[0] == CC.T and len({d[key][t].tobytes() for t in range(CC.T)}) == CC.T, key
        LC.assert_alias_free(CC.T, d[key].size // CC.T)
    want = d["want"]
    assert np.isfinite(want).all()
    if c["entry"] == "dx_wide":
        LC.assert_alias_free(CC.T, want.size // CC.T)
        on = want[:, ::2, ::2] if not c["transposed"] else want  # the 1x1 stride-2 layer: +0 off the even grid, by the contract
        assert (on != 0).all() and ((want == 0).mean() == (0.0 if c["transposed"] else 0.75))
        assert not (want.view(np.uint32) == 0x80000000).any()
    else:  # compared on the host, where a zero's sign is left open; H = 1: the middle row of taps is the one inside the frame
        per_frame = len(want) // CC.T
        assert per_frame == (1 if c["entry"] == "dw_image" else 3)
        dw, db = CC.split_dw(CC.level2(want, 4 * len(want)), c["ksize"], c["cin"])
        mid = dw[c["ksize"] // 2] if c["W"] > 1 else dw[c["ksize"] // 2, c["ksize"] // 2]
        # (a 1 x 1 frame: T products a sum, of values a third of which are zeros)
        assert (mid != 0).mean() > (0.9 if c["W"] > 1 else 0.5) and (db != 0).mean() > 0.9, (mid != 0).mean()
        assert len({p.tobytes() for p in want}) == len(want)  # every segment of the tile has partials of its own


def wsizes(c):
    """The elements of every tensor argument of a case of WLARGE, and its workspace bytes."""
    (Ho, Wo), _ = CC.wframes(c)
    n, no = c["B"] * c["H"] * c["W"], c["B"] * Ho * Wo
    e = {"dy": no * c["width"]}
    if c["act"] == R.LEAKY:
        e["y"] = no * c["width"]
    e["dx" if c["entry"] == "dx_wide" else "x"] = n * c["cin"]
    if c["dres"]:
        e["dresidual"] = no * c["cout"]
    return e


def test_backward_large_cases_pass_their_thresholds():
    past4 = {"wide": set(), "image": set()}
    for name, c in CC.WLARGE.items():
        group = "image" if c["entry"] == "dw_image" else "wide"
        e = wsizes(c)
        assert all(v < 2 ** 31 for v in e.values()), name  # the shape rule
        assert CC.wdevice_bytes(c, LC.CHUNK_BYTES) < 20e9, (name, CC.wdevice_bytes(c, LC.CHUNK_BYTES))
        frame = {k: v // c["B"] for k, v in e.items()}
        over = lambda least: {k for k in e if (c["B"] - CC.T) * frame[k] >= least}  # noqa: E731: the last T frames start beyond
        if "past 4 GiB" in name:
            named = {k for k in e if k in name.split(" past 4 GiB")[0].replace(",", " ").split()}
            assert named and named <= over(2 ** 30), (name, named, over(2 ** 30))
            past4[group] |= over(2 ** 30)
            assert "workspace" not in name or CC.wworkspace_bytes(c) > 2 ** 32, name  # g of a 64-channel dy for the whole batch
        elif "past 2 GiB" in name:
            assert over(2 ** 29) and not over(2 ** 30), name
        else:
            assert "at the limit" in name and any(2 ** 31 - frame[k] <= v < 2 ** 31 for k, v in e.items()), name
        assert c["at"] + c["cout"] <= c["width"]
    assert past4["wide"] == {"dy", "y", "dx", "dresidual", "x"} and past4["image"] == {"dy", "y"}
    for group in ("dx_wide", "dw_wide", "dw_image"):
        names = " ".join(n for n, c in CC.WLARGE.items() if c["entry"] == group)
        assert "past 4 GiB" in names and "at the limit" in names, group
    assert sum("past 2 GiB" in n for n in CC.WLARGE) == 2  # one for the wide calls, one for the image layer
    assert {(c["stride"], c["transposed"]) for c in CC.WLARGE.values() if c["entry"] == "dx_wide"} == {(1, False), (2, False), (2, True)}
    for name, c in CC.ILARGE.items():
        B, by = c["B"], c["by"]
        Ho, Wo = CC.out_frame(c)
        assert by == Ho * Wo * c.get("out_channels", c["cout"]) and c["cin"] in (3, 4), name
        assert B * by < 2 ** 31 and CC.device_bytes(c, LC.CHUNK_BYTES) < 20e9
        if c["past"] == "limit":
            assert 2 ** 31 - by <= B * by
        else:
            assert (B - CC.T) * by >= c["past"] > (B - CC.T - 1) * by, name
    assert {c["past"] for c in CC.ILARGE.values()} == {2 ** 29, 2 ** 30, "limit"}


def test_backward_refused_calls_stand_exactly_at_the_limit():
    for entry, what, a in CC.WREFUSED:
        assert CC.wrefused_count(entry, a) == 2 ** 31, (entry, what)
        n = a["B"] * a["H"] * a["W"]
        if entry == "image":
            counts = [n * a["cin"], n * a["cout"], n * a.get("out_channels", 0)]
        else:
            (Ho, Wo), _ = CC.wframes(dict(a, transposed=a.get("transposed", False), stride=a.get("stride", 1)))
            no = a["B"] * Ho * Wo
            counts = [n * a["cin"], n * a.get("dx_channels", 0), no * a["cout"], no * a.get("dy_channels", 0), no * a.get("y_channels", 0)]
        assert sorted(counts)[-1] == 2 ** 31 and sorted(counts)[-2] < 2 ** 31, (entry, what, counts)  # one count alone is at the limit
    has = {(e, w.split()[-1] if "(" not in w else "dx_channels") for e, w, _ in CC.WREFUSED}
    assert has >= {("image", "Cout"), ("image", "out_channels"), ("dw_image", "Cout"), ("dw_image", "dy_channels"), ("dw_image", "y_channels"),
                   ("dx_wide", "Cin"), ("dw_wide", "Cin"), ("dx_wide", "Cout"), ("dw_wide", "Cout"), ("dx_wide", "dy_channels"),
                   ("dw_wide", "y_channels"), ("dx_wide", "dx_channels")}
    assert {a.get("transposed", False) for e, _, a in CC.WREFUSED if e in ("dx_wide", "dw_wide")} == {False, True}


@pytest.fixture(scope="module", params=[("WLARGE", n) for n in CC.WLARGE] + [("ILARGE", n) for n in CC.ILARGE], ids=lambda p: "%s: %s" % p)
def blarge(request):
    table, name = request.param
    c = getattr(CC, table)[name]
    return table, c, (CC.wtile(c) if table == "WLARGE" else CC.tile(c))


def test_backward_large_tiles_are_alias_free_and_have_no_open_zero(blarge):
    table, c, d = blarge
    if table == "ILARGE":
        for _, period in CC.periods(c, d):
            LC.assert_alias_free(CC.T, period // CC.T)
        at = c.get("out_offset", 0)
        assert (d["want"][..., at:at + c["cout"]] != 0).all()
        return
    for key in ("x", "dy", "y"):
        assert len({d[key][t].tobytes() for t in range(CC.T)}) == CC.T, key
        LC.assert_alias_free(CC.T, d[key].size // CC.T)
    want = d["want"]
    assert np.isfinite(want).all()
    if c["entry"] == "dx_wide":
        LC.assert_alias_free(CC.T, want.size // CC.T)
        spread = not c["transposed"] and c["stride"] == 2 and c["ksize"] == 1
        assert ((want[:, ::2, ::2] if spread else want) != 0).all()  # off the even grid the 1x1 stride-2 layer writes +0, by the contract
        if c["dres"]:  # dresidual is g = dy here (LINEAR): a copy, zeros of dy included, bit for bit
            LC.assert_alias_free(CC.T, d["dres"].size // CC.T)
            assert c["act"] == R.LINEAR and (d["dres"].view(np.uint32) == d["dy"][..., c["at"]:c["at"] + c["cout"]].view(np.uint32)).all()
    else:
        dw, db = CC.split_dw(CC.level2(want, 4 * len(want)), c["ksize"], c["cin"])
        assert (dw != 0).mean() > 0.9 and (db != 0).all()


# ================================================================================================ the bf16 backward calls
def test_bf16_backward_loop_cases_reach_the_second_launch():
    wide = {n: c for n, c in CC.HBLOOP.items() if c["entry"] == "dw_wide"}
    for name, c in wide.items():
        _, (Hs, Ws) = CC.wframes(c)
        assert c["bf16"] and (Hs, Ws) == (1, 129) and CC.wsegments(c) == 3 * c["B"] == 65637 == CC.GRID_Z + 102, name
        assert CC.GRID_Z % 3 == 0  # segment 65535 is column 0 of frame 21845: the second launch begins on a frame boundary ...
        assert (CC.wsegments(c) - CC.GRID_Z) % 3 != 0 or Ws % CC.SEG_COLS == 1  # ... and its last frame ends with a segment of one column
        assert c["cin"] // 16 < CC.GRID_Z  # one launch along the group axis: gl0 stays 0 within the shape rule
    # one call for each instantiation convhb_weights_launch asks for, the 3x3 stride-1 one on both bodies
    assert sorted((c["ksize"], c["stride"], c["transposed"], c["mis"]) for c in wide.values()) == [
        (1, 1, False, 0), (1, 2, False, 0), (3, 1, False, 0), (3, 1, False, 4), (3, 2, False, 0), (3, 2, True, 0)]
    dx = {n: c for n, c in CC.HBLOOP.items() if c["entry"] == "dx_wide"}
    assert {(c["ksize"], c["stride"], c["transposed"]) for c in dx.values()} == {(1, 2, False), (3, 2, True)} and len(CC.HBLOOP) == 8
    for name, c in CC.HBLOOP.items():
        floor = 2 * 4 * 21879 * 2 * 258 * 32 if c["transposed"] else 0  # g beside dy, both B 2H 2W Cout floats
        assert max(floor, 0) <= CC.wdevice_bytes(c) < max(3e9, floor + 1e9), (name, CC.wdevice_bytes(c))
        assert CC.wworkspace_bytes(c) % 256 == 0 and CC.wworkspace_bytes(c) <= CC.wworkspace_bytes(dict(c, bf16=False))


@pytest.fixture(scope="module", params=[("HBLOOP", n) for n in CC.HBLOOP] + [("HBLARGE", n) for n in CC.HBLARGE], ids=lambda p: "%s: %s" % p)
def hbtiled(request):
    table, name = request.param
    c = getattr(CC, table)[name]
    return c, CC.wtile(c)  # asserts bf16 operands and partial sums below 2^24 quarter-units


def test_bf16_backward_tiles_are_exact_alias_free_and_have_no_open_zero(hbtiled):
    c, d = hbtiled
    for key in ("x", "dy", "y"):
        assert d[key].shape[0] == CC.T and len({d[key][t].tobytes() for t in range(CC.T)}) == CC.T, key
        LC.assert_alias_free(CC.T, d[key].size // CC.T)
    want = d["want"]
    assert np.isfinite(want).all() and np.array_equal(np.rint(want * 4), want * 4)
    if c["entry"] == "dx_wide":
        LC.assert_alias_free(CC.T, want.size // CC.T)
        spread = not c["transposed"] and c["stride"] == 2 and c["ksize"] == 1
        assert ((want[:, ::2, ::2] if spread else want) > 0).all() and not (want.view(np.uint32) == 0x80000000).any()
        assert not spread or (want == 0).mean() == 0.75  # +0 off the even grid, by the contract
        at = c["at"]
        dy, y = d["dy"][..., at:at + c["cout"]], d["y"][..., at:at + c["cout"]]
        x = CC.HBB.dx_sum(RB.g_ref(dy, y, c["act"], CC.HBALPHA), d["w"], c["stride"], c["transposed"])  # the float64 statement agrees
        assert np.array_equal(x, want.astype(np.float64))
        if c["dres"]:
            LC.assert_alias_free(CC.T, d["dres"].size // CC.T)
            assert (d["dres"] != 0).all()
    else:
        (_, _), (Hs, Ws) = CC.wframes(c)
        per_frame = -(-Hs // CC.SEG_ROWS) * -(-Ws // CC.SEG_COLS)
        assert len(want) == CC.T * per_frame and len({p.tobytes() for p in want}) == len(want)  # every segment has partials of its own
        # the partials of a frame add up to the statement over the whole frame
        at = c["at"]
        g = RB.g_ref(d["dy"][..., at:at + c["cout"]], d["y"][..., at:at + c["cout"]], c["act"], CC.HBALPHA)
        dw, db = CC.HBB.dw_sum(d["x"], g, c["ksize"], c["stride"], c["transposed"])
        total = want.astype(np.float64).sum(axis=0)
        assert np.array_equal(total[:-1].reshape(dw.shape), dw) and np.array_equal(total[-1], db)
        l2dw, l2db = CC.split_dw(CC.level2(want, 4 * len(want)), c["ksize"], c["cin"])
        assert (l2dw != 0).mean() > (0.25 if Hs == 1 and c["ksize"] == 3 else 0.9) and (l2db != 0).mean() > 0.9


def test_bf16_backward_large_cases_pass_their_thresholds():
    past4 = set()
    for name, c in CC.HBLARGE.items():
        e = wsizes(c)
        assert c["bf16"] and all(v < 2 ** 31 for v in e.values()), name  # the shape rule
        assert CC.wdevice_bytes(c, LC.CHUNK_BYTES) < 20e9, (name, CC.wdevice_bytes(c, LC.CHUNK_BYTES))
        frame = {k: v // c["B"] for k, v in e.items()}
        over = lambda least: {k for k in e if (c["B"] - CC.T) * frame[k] >= least}  # noqa: E731: the last T frames start beyond
        if "past 4 GiB" in name:
            named = {k for k in e if k in name.split(" past 4 GiB")[0].replace(",", " ").split()}
            assert named and named <= over(2 ** 30), (name, named, over(2 ** 30))
            past4 |= over(2 ** 30)
            if "workspace" in name:  # p.wt, the packed kernel, lies behind a g of more than 4 GiB
                (Ho, Wo), _ = CC.wframes(c)
                assert 4 * c["B"] * Ho * Wo * c["cout"] > 2 ** 32 and CC.wworkspace_bytes(c) > 2 ** 32, name
        elif "past 2 GiB" in name:
            assert over(2 ** 29) and not over(2 ** 30), name
        else:
            assert "at the limit" in name and any(2 ** 31 - frame[k] <= v < 2 ** 31 for k, v in e.items()), name
    assert past4 == {"dy", "y", "dx", "dresidual", "x"}
    shapes = sorted((c["entry"], c["ksize"], c["stride"], c["transposed"], c["cin"], c["cout"]) for c in CC.HBLARGE.values())
    assert shapes == [("dw_wide", 1, 1, False, 64, 16), ("dw_wide", 1, 1, False, 64, 16), ("dw_wide", 3, 2, False, 16, 16),
                      ("dw_wide", 3, 2, True, 64, 16), ("dx_wide", 1, 1, False, 64, 64), ("dx_wide", 1, 2, False, 64, 64),
                      ("dx_wide", 3, 2, True, 64, 16)]
    spread = [c for c in CC.HBLARGE.values() if c["entry"] == "dx_wide" and c["stride"] == 2 and not c["transposed"]]
    assert len(spread) == 1 and spread[0]["ksize"] == 1  # where p.tmp is in use


def test_bf16_backward_refused_calls_are_the_twins_wide_rows():
    assert len(CC.HBREFUSED) == 10 and all(a["ksize"] in (1, 3) for _, _, a in CC.HBREFUSED)  # the bf16 domain
    for entry, what, a in CC.HBREFUSED:
        assert CC.wrefused_count(entry, a) == 2 ** 31, (entry, what)
    assert {(e, a.get("transposed", False)) for e, _, a in CC.HBREFUSED} == {("dx_wide", False), ("dx_wide", True), ("dw_wide", False), ("dw_wide", True)}

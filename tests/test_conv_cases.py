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

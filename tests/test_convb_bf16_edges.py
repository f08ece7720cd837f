"""What the builders of tests/convb_bf16_edges.py are held to without a GPU: the one-term property and the table of A1, the
widths of A2 reaching every `left` from 1 to 31, the sentinels' reach, the exactness of A4, and that compare() and
subnormal_choice() do tell a truncating, a flushing and a mask-less kernel from the statement."""
import numpy as np
import pytest

import conv_bf16_ref as RH
import conv_ref as R
import convb_bf16_edges as E
import convb_bf16_ref as RHB

F = np.float32


def test_the_table_is_the_forwards_with_the_subnormal_range():
    import test_gpu_conv2d_bf16 as HT

    assert E.TABLE is HT.TABLE and E.TABLE.size == 22
    r = RH.bf16_round(E.SUBNORMALS).astype(np.float64)
    u = 2.0 ** -133
    assert np.array_equal(r / u, [64, 2, 2, 4, -5, 128, 1, 1, 0, 8])  # ties to even both ways, up to the normal 2^-126, down to 0
    assert (np.abs(E.SUBNORMALS[:-2]) >= u / 2).all() and abs(E.SUBNORMALS[8]) < u / 2 and E.is_subnormal(r).sum() == 8
    assert E.VALUES.size == E.CHANNELS
    trunc = (E.VALUES.view(np.uint32) & 0xFFFF0000).view(F)  # a truncating kernel differs on the ties up, the near-ties, FLT_MAX, ...
    differs = ~R.same_bits(trunc, RH.bf16_round(E.VALUES))
    assert differs.sum() >= 10


@pytest.mark.parametrize("lid,layer,site,tap", E.rounding_runs(), ids=lambda v: str(v).replace(" ", ""))
def test_rounding_cases_have_one_term_an_entry(lid, layer, site, tap):
    d = E.rounding_case(layer, site, tap)  # asserts the property, the diagonal and exactness
    n = E.VALUES.size
    assert np.isinf(d["dw"]).any() and np.isnan(d["dw"]).any() and E.is_subnormal(d["dw"]).sum() >= (4 if site == "g alpha" else 8)
    assert np.isnan(d["db"]).sum() == (0 if site == "x" else 3) and (d["y"] is None) == (site == "g linear")
    cols = {3 * k % E.ROUND_FRAME[1] for k in range(n)}
    assert len(cols) == n and any(c >= 32 for c in cols) and {c % 32 // 4 for c in cols if c < 32} == set(range(8))
    # the statement itself passes the comparison, the truncated table and a flushed one do not pass as they are
    E.compare(d["dw"].astype(F), d["dw"], "dw")
    assert E.subnormal_choice([(d["dw"].astype(F), d["dw"])]) == "kept"
    flushed = np.where(E.is_subnormal(d["dw"]), 0, d["dw"]).astype(F)
    assert E.subnormal_choice([(flushed, d["dw"])]) == "flushed"
    mixed = flushed.copy()
    k = tuple(np.argwhere(E.is_subnormal(d["dw"]))[0])
    mixed[k] = d["dw"][k]
    with pytest.raises(AssertionError):
        E.subnormal_choice([(mixed, d["dw"])])
    # a kernel that truncates where this site rounds: x, or g = g_ref(dy, y) (under y < 0 the float32 product, whose rounding to
    # bf16 is the second one), truncated to bf16 in place of bf16_round
    trunc = lambda a: (np.ascontiguousarray(a, F).view(np.uint32) & 0xFFFF0000).view(F)  # noqa: E731
    g = RHB.g_ref(d["dy"], d["y"], d["act"], d["alpha"])
    x, g = (trunc(d["x"]), RH.bf16_round(g)) if site == "x" else (RH.bf16_round(d["x"]), trunc(g))
    with np.errstate(over="ignore", invalid="ignore"):
        dw, db = RHB.dw_sum(x, g, layer[0], layer[1], layer[2])
    with pytest.raises(AssertionError):
        E.compare(dw.astype(F), d["dw"], "dw of a truncating kernel")
    if site != "x":
        with pytest.raises(AssertionError):
            E.compare(db.astype(F), d["db"], "db of a truncating kernel")


def test_the_sites_cover_every_layer_and_parity():
    runs = E.rounding_runs()
    assert {(l, s) for _, l, s, _ in runs} >= {(l, s) for l in E.STRIDED for s in E.SITES} | {(E.LAYERS[4], s) for s in E.SITES}
    assert {t for _, l, s, t in runs if l[2] and s == "g"} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_edge_widths_reach_every_left():
    """3x3 stride 1: every left from 1 to 31 with zero, one and (in the second segment) zero whole steps before it, i.e. at Ws =
    left, 32 + left and 64 + left; the other layers: every left behind a whole segment, and 1 and 31 in the first."""
    reach = {E.edge_left(w) for w in E.EDGE_WIDTHS[(3, 1, False)]} - {None}
    assert reach == {(left, whole, seg) for left in range(1, 32) for whole, seg in ((0, 0), (1, 0), (0, 1))}
    assert [w for w in E.EDGE_WIDTHS[(3, 1, False)] if E.edge_left(w) is None] == [32, 64, 96]
    for layer in E.LAYERS[1:]:
        reach = {E.edge_left(w) for w in E.EDGE_WIDTHS[layer]}
        assert reach == {(left, 0, 1) for left in range(1, 32)} | {(1, 0, 0), (31, 0, 0), (1, 1, 0), (31, 1, 0)}, layer
    # left > 16 is what the second half of chb_inside's index decides
    assert sum(1 for w in E.EDGE_WIDTHS[(3, 1, False)] if (E.edge_left(w) or (0,))[0] > 16) == 45


@pytest.mark.parametrize("layer", E.LAYERS, ids=E.IDS)
def test_edge_cases_put_the_sentinels_where_the_mask_matters(layer):
    ksize, stride, transposed = layer
    for Ws in (1, 2, 17, 31, 33, 65, 95):
        if Ws not in E.EDGE_WIDTHS[layer]:
            continue
        d = E.edge_case(layer, Ws)  # asserts exactness and that no inf meets a zero
        dw, db = d["dw"], d["db"]
        big = d["dy"] if transposed else d["x"]
        assert d["sentinel"][-1] == big.shape[2] - 1 and np.isinf(big[0, 0, d["sentinel"][-1], :8]).all() and np.isnan(big[0, 0, -1, 8:]).all()
        assert np.isfinite(np.delete(big, d["sentinel"], axis=2)).all() and np.isfinite(big[0, 1:]).all()
        if layer == (3, 1, False):
            # the contract: a position past the frame is +0 on both operands, so the last column of x never reaches tap column 0
            assert np.isfinite(dw[:, 0]).all() and np.isfinite(db).all()
            assert np.isinf(dw[:2, 1, :8]).all() and np.isnan(dw[:2, 1, 8:]).all() and np.isfinite(dw[2]).all()
            # without the mask the pixel v = Ws meets x[.., Ws - 1] * 0: NaN in tap column 0 (the statement over an extended g)
            wide = np.concatenate([d["dy"], np.zeros_like(d["dy"][:, :, :1])], axis=2)
            xw = np.concatenate([d["x"], np.zeros_like(d["x"][:, :, :1])], axis=2)
            with np.errstate(invalid="ignore"):
                unmasked, _ = RHB.dw_sum(xw, RHB.g_ref(wide, np.concatenate([d["y"], d["y"][:, :, :1]], axis=2), R.LEAKY, RHB.ALPHA_INT), 3, 1)
            assert np.isnan(unmasked[:2, 0]).all()
        elif layer == (1, 2, False):
            assert np.isfinite(dw).all()  # the last column of x is odd: the 1x1 stride-2 layer never reads it
        elif layer == (1, 1, False):
            assert not np.isfinite(dw).any() and np.isfinite(db).all()  # every input channel meets every entry: the plain case runs too
            assert np.isfinite(E.edge_case(layer, Ws, sentinels=False)["dw"]).all()
        else:
            assert np.isinf(dw).any() and np.isnan(dw).any() and np.isfinite(dw).any()
        if transposed:
            assert np.isinf(db[:8]).all() and np.isnan(db[8:]).all()
        held = dw if np.isfinite(dw).any() else db
        with pytest.raises(AssertionError):
            E.compare(np.where(np.isfinite(held), held + 0.25, held).astype(F), held, "a quarter off")
        E.compare(dw.astype(F), dw, "dw")


@pytest.mark.parametrize("lid,layer,channels", E.channel_runs(), ids=lambda v: str(v).replace(" ", ""))
def test_channel_cases_are_exact(lid, layer, channels):
    (x, w, dy, y), (dx, g, dw, db) = E.channel_case(layer, *channels)  # asserts integers below 2^24 quarter-units
    assert dw.shape == (layer[0], layer[0]) + channels and db.shape == channels[1:] and dx.shape == x.shape
    assert (dw != 0).mean() > 0.8 and np.abs(dx).max() > 4
    if channels == (32, 48):  # where int64 is cheap, it agrees
        want = RHB.integer_ref(x, w, dy, y, layer[1], R.LEAKY, layer[2])
        for a, b in zip((dx, g, dw, db), want):
            assert np.array_equal(a, b)


def test_channel_runs_are_the_networks():
    assert {c for _, l, c in E.channel_runs() if not l[2]} == {(16, 16), (16, 512), (512, 16), (64, 128), (256, 512), (512, 512), (32, 48)}
    assert {c for _, l, c in E.channel_runs() if l[2]} == {(512, 256), (128, 64), (16, 16), (16, 512)}
    assert len(E.channel_runs()) == 4 * 7 + 4

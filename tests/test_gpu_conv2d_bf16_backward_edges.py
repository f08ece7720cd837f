"""k_convhb_dw_wide and k_convhb_pack (csrc/dtfill_convhb.hpp) where tests/test_gpu_conv2d_bf16_backward.py cannot see a wrong
kernel, through the ABI with that file's machinery (run_data, run_weights: guarded buffers, poisoned outputs, a workspace of
NaNs).  tests/convb_bf16_edges.py builds the cases and tests/test_convb_bf16_edges.py holds the builders on the CPU.  Every
expectation is a numpy statement in float64 (or its float32 twin's own exact integers) and every comparison is exact: no
tolerance anywhere.

A1  the rounding of dw's operands.  A table (test_gpu_conv2d_bf16.py's, with the bf16 subnormal range) through each staging
    site: x and g of the strided layers (g under y > 0, under y < 0 with alpha 0.2 - a float32 product rounded a second time -
    and LINEAR with y NULL), x and g of the transposed layer, g there at each of the four parities of db's chains; aligned and 4
    bytes off (VEC = false).  Every entry of dw and db is a sum with at most one non-zero term, so the statement is exact.
    Subnormal bf16 operands are left open by the contract: kept or flushed to zero, one choice per call, printed.
    Measured on one MI355X: kept, in every call, as in the forward.
A2  every width of the edge k-step, with +inf and NaN in the large operand's last column: chb_inside at every `left`, and the
    contract's rule that a position past the frame is +0 on BOTH operands (3x3 stride 1: tap column 0 stays finite).
A3  the LINEAR path with y NULL through the ABI, bit for bit, the float32 twin beside it.
A4  the networks' channel counts, 16 to 512 either way: every tile, pass and group written once, with the right tap.

Seeded faults (each built once on a scratch copy and run once; profiles/r35/bf16_backward_edges.txt):
  chb_round truncates                 all 46 cases of A1 fail, every site; no test of test_gpu_conv2d_bf16_backward.py fails, the network
                                      test does (two dw layers at 59 and 62 times the bound).
  chb_inside: 8 + e for 12 + e        A2 fails at 3x3 stride 1, first at Ws = left = 16 (all of dw[:, 0] is NaN); no older test fails.
  b.y offset also under LINEAR        a no-op, not seeded: y is NULL there, y_channels is 0 and convb_g4 never reads it.
  k_convhb_pack without the flip      A3 and all seven channel pairs of A4 fail at 3x3 stride 1 (dx), as four cases of
                                      test_gpu_conv2d_bf16_backward.py and the network test do: the harness sees a wrong dx.
"""
import numpy as np
import pytest

import conv_ref as R
import convb_bf16_edges as E
import convb_bf16_ref as RHB
import test_gpu_conv2d_bf16_backward as bb
from test_gpu_conv2d_bf16_backward import L  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F = np.float32
POISON = bb.POISON


# ---- A1 ----------------------------------------------------------------------------------------------------------------------------
_rounding = {}


def _rounding_case(layer, site, tap):
    key = (layer, site, tap)
    if key not in _rounding:
        _rounding[key] = E.rounding_case(layer, site, tap)
    return _rounding[key]


@pytest.mark.parametrize("mis", (0, 4), ids=("aligned", "4 bytes off"))
@pytest.mark.parametrize("lid,layer,site,tap", E.rounding_runs(), ids=lambda v: str(v).replace(" ", ""))
def test_rounding_table_through_each_staging_site(L, lid, layer, site, tap, mis):
    ksize, stride, transposed = layer
    d = _rounding_case(layer, site, tap)
    dw, db = bb.run_weights(L, d["x"], d["dy"], d["y"], ksize, stride, transposed, alpha=d["alpha"], mis=mis, act=d["act"])
    choice = E.subnormal_choice([(dw, d["dw"]), (db, d["db"])])
    print("bf16 dw %s, table in %s%s%s: subnormal operands %s" % (lid, site, "" if tap is None else " at tap %s" % (tap,),
                                                                  ", 4 bytes off" if mis else "", choice))
    E.compare(dw, d["dw"], "dw")
    E.compare(db, d["db"], "db")
    assert choice in ("kept", "flushed")


# ---- A2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", E.LAYERS, ids=E.IDS)
def test_every_width_of_the_edge_k_step(L, layer):
    ksize, stride, transposed = layer
    for Ws in E.EDGE_WIDTHS[layer]:
        for sentinels in (True, False) if layer == (1, 1, False) else (True,):
            d = E.edge_case(layer, Ws, sentinels=sentinels)
            what = "Ws %d, left %s%s" % (Ws, E.edge_left(Ws), "" if sentinels else ", no sentinels")
            dw, db = bb.run_weights(L, d["x"], d["dy"], d["y"], ksize, stride, transposed)
            if layer == (3, 1, False):
                bad = np.argwhere(~np.isfinite(dw[:, 0]))
                assert not bad.size, ("%s: the last column of x reached tap column 0 through the position past the frame: %d entries of "
                                      "dw[:, 0], first %s" % (what, len(bad), tuple(bad[0])))
            E.compare(dw, d["dw"], "dw, " + what)
            E.compare(db, d["db"], "db, " + what)


# ---- A3 ----------------------------------------------------------------------------------------------------------------------------
_linear = {}


def linear_layer(ksize, stride, transposed):
    key = (ksize, stride, transposed)
    if key not in _linear:
        (x, w, dy, _), _ = bb.integer_layer(ksize, stride, transposed)
        _linear[key] = (x, w, dy), RHB.integer_ref(x, w, dy, None, stride, R.LINEAR, transposed)
    return _linear[key]


@pytest.mark.parametrize("ksize,stride,transposed", E.LAYERS, ids=E.IDS)
def test_the_linear_path_with_y_null(L, ksize, stride, transposed):
    (x, w, dy), (dx, g, dw, db) = linear_layer(ksize, stride, transposed)
    cin = x.shape[3]
    assert np.array_equal(g, dy)
    twin = {}
    for bf16 in (True, False):
        out = bb.run_data(L, dy, None, w, stride, transposed, dx_channels=cin + 24, dx_offset=8, residual=not transposed, bf16=bf16,
                          act=R.LINEAR)
        wide, res = out if not transposed else (out, None)
        R.assert_same(wide[..., 8:8 + cin], dx, "dx")
        assert (np.delete(wide, np.s_[8:8 + cin], axis=-1).view(np.uint32) == POISON).all(), "channels outside the dx slice"
        if res is not None:
            assert bb.same_bits(res, dy), "dresidual is dy, bit for bit"
        got_dw, got_db = bb.run_weights(L, x, dy, None, ksize, stride, transposed, bf16=bf16, act=R.LINEAR)
        R.assert_same(got_dw, dw, "dw")
        R.assert_same(got_db, db, "db")
        twin[bf16] = (wide, got_dw, got_db)
    for a, b, what in zip(twin[True], twin[False], ("dx", "dw", "db")):
        R.assert_same(a, b, what + " against the float32 twin")


# ---- A4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lid,layer,channels", E.channel_runs(), ids=lambda v: str(v).replace(" ", ""))
def test_the_networks_channel_counts(L, lid, layer, channels):
    ksize, stride, transposed = layer
    cin, cout = channels
    (x, w, dy, y), (dx, g, dw, db) = E.channel_case(layer, cin, cout)
    out = bb.run_data(L, dy, y, w, stride, transposed, dx_channels=cin + 24, dx_offset=8, residual=not transposed)
    wide, res = out if not transposed else (out, None)
    R.assert_same(wide[..., 8:8 + cin], dx, "dx")
    assert (np.delete(wide, np.s_[8:8 + cin], axis=-1).view(np.uint32) == POISON).all(), "channels outside the dx slice"
    if res is not None:
        R.assert_same(res, g, "dresidual")
    got_dw, got_db = bb.run_weights(L, x, dy, y, ksize, stride, transposed)
    R.assert_same(got_dw, dw, "dw")
    R.assert_same(got_db, db, "db")

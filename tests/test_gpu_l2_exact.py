"""The l2 mode held to its contract where float32 gives out and where a search stops: exact distances, near-ties beyond
d2 = 2^24, ties that sit exactly on a stop bound.  Inputs: tests/l2_exact_cases.py; what they hold is asserted without a GPU in
test_l2_exact.py; the reference is the brute force of tests/l2_ref.py (and the oracle, on the small frames, on every pixel).

Every pass goes through DtFill(metric="l2").run on poisoned outputs and workspace.  Bar: index exact, dt equal as uint32 bit
patterns (sqrtf is correctly rounded on both sides: out_dt must BE np.sqrt(float32(d2))), depth exact (every source has a value
of its own: a wrong winner shows there too), status bit 1 clear; and op.pass_stats() must show the kernel family the input is
meant for.

Which family can meet d2 >= 2^24: l2pts_tile, l2env_row and l2sky_row.  k_l2win stops at R^2 <= 225; k_l2far takes the far pixels
of rows with fewer than max(32, W / 8) of them, and such a pixel has a source within W / 8 + 15 columns or so: d2 < 1.1e6 at the
widest frame.  Those two are held to exactness by the bit-equal comparisons of the other l2 tests and by the bound ties here."""
import itertools

import numpy as np
import pytest

import l2_exact_cases as C
import l2_ref
from guarded import poison_op

pytestmark = pytest.mark.gpu
_POISON = itertools.count(9700)


@pytest.fixture(scope="module")
def op2(pkg, gpu_op):
    return pkg.device.DtFill(device="cuda:0", metric="l2")


def run(op, x, path):
    import torch

    xd = torch.from_numpy(x[None]).to("cuda:0")
    poison_op(op, next(_POISON), xd.shape, path=path)
    res = op.run(xd, path=path)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy()[0] for k, v in res.items()}
    return got, op.pass_stats()


def assert_reference(got, case, what):
    """The pass's outputs on every pixel set of the case against l2_ref."""
    assert got["status"] & 1 == 0, what
    for n, r in enumerate(case.refs):
        i, j = r.pix[:, 0], r.pix[:, 1]
        bad = got["index"][i, j] != r.label
        assert not bad.any(), "%s set %d: index differs at %d of %d px, first %s" % (what, n, bad.sum(), len(bad), r.pix[bad][:3].tolist())
        bad = l2_ref.bits(got["dt"][i, j]) != l2_ref.bits(r.dt)
        assert not bad.any(), "%s set %d: dt differs at %d of %d px, first %s" % (what, n, bad.sum(), len(bad), r.pix[bad][:3].tolist())
        assert np.array_equal(got["depth"][i, j], case.x.ravel()[r.near]), "%s set %d: depth differs" % (what, n)


def assert_oracle(got, want, what):
    depth, dt, idx, status = want
    assert np.array_equal(got["index"], idx[0]), "%s: index differs from the oracle at %d px" % (what, (got["index"] != idx[0]).sum())
    assert np.array_equal(l2_ref.bits(got["dt"]), l2_ref.bits(dt[0])), "%s: dt differs from the oracle" % what
    assert np.array_equal(got["depth"], depth[0]) and got["status"] & 1 == status[0] == 0, what


def owned_by(stats, family, sky_rows=None, W=None):
    """The pass statistics say that `family` took the frame: "points" (l2pts_tile), "rows" (every row to the row search:
    l2env_row), "window" (k_l2win, with exactly sky_rows rows redone whole by l2sky_row -- pass_stats counts whole rows)."""
    if family == "points":
        assert stats["points"] == stats["all"], stats
    elif family == "rows":
        assert stats["anydist"] == stats["all"] and stats["points"] == 0 and stats["window"] == 0, stats
    else:
        assert stats["points"] == 0 and stats["anydist"] == W * sky_rows and stats["window"] == stats["all"] - W * sky_rows, (stats, sky_rows)
        assert stats["colt"] == (stats["all"] if sky_rows else 0), stats


FAR = {"cluster500": (lambda o: C.cluster(500, o), "points"), "cluster1200": (lambda o: C.cluster(1200, o), "rows"),
       "edge": (C.edge, "window"), "line": (C.line, "points")}


@pytest.mark.parametrize("orient", (C.WIDE, C.TALL))
@pytest.mark.parametrize("name", sorted(FAR))
def test_near_ties_beyond_2_to_24(op2, name, orient):
    """120 x 8000 / 40 x 8100 and their transposes, every checked pixel of the first set at d2 >= 2^24 (up to 6.2e7):
      cluster500   500 sources in the 150 columns at one end: l2pts_tile; on the general path l2env_row
                   (40 000 sampled pixels: 525 collisions, 982 ties)
      cluster1200  1200 sources there: l2env_row on the default path (1065 collisions, 1330 ties)
      edge         30 % sources in columns < 3700, nothing beyond: k_l2win<10>'s frame, every row of the empty part redone by
                   l2sky_row (the 12 000 pixels of the last 300 columns: 600 collisions, 1800 ties); on the general path l2env_row
      line         a full column (wide) / row (tall) of sources: every far pixel's runner-up at d2 + 1, 78 % of them colliding;
                   l2pts_tile, and l2env_row on the general path
    A key compared or carried in float32, or packed a bit short, picks the wrong one of two sources at a collision; a tie rule
    other than the canonical one shows at a tie; a distance computed apart from the key shows in dt's bits."""
    case, family = FAR[name][0](orient), FAR[name][1]
    H, W = case.x.shape
    got, stats = run(op2, case.x, "auto")
    owned_by(stats, family, C.edge_sky_rows(orient) if name == "edge" else None, W)
    assert_reference(got, case, "%s %s auto" % (name, orient))
    if family != "rows":
        got, stats = run(op2, case.x, "general")
        owned_by(stats, "rows")
        assert_reference(got, case, "%s %s general" % (name, orient))


@pytest.mark.parametrize("name", [f.__name__ for f in C.SMALL])
def test_ties_on_a_stop_bound(op2, oracle, name):
    """Hand-built frames (tests/l2_exact_cases.py), every pixel against l2_ref and the oracle, on the default path (the window
    kernel's frame: its rows with 80 / 32 far pixels or more to l2sky_row, the other far pixels to k_l2far) and on the general
    path (l2env_row):
      ring17, ring33  l2sky_row's stop test `best >= gmin^2 + (R + 1)^2` with equality after the first and the second window: the
                      winner (smaller source row) is in the column just outside, on either side
      farpixel        l2far_pixel's `base^2 <= best` with equality at base = 32: the winner (straight above) is seen in that round
                      alone; k_l2win<10>'s split: d2 = 100 decided by the window, d2 = 101 handed on, both many-way ties
      rowcount        rows with 79, 80 and 81 far pixels, counted by several waves of three tiles: w2_row_t(640) = 80 sends the
                      first to the far list, the others to l2sky_row; pass_stats counts exactly the rows the reference counts
      win15           k_l2win<15>'s split: d2 = 225 against 226."""
    case = getattr(C, name)()
    H, W = case.x.shape
    want = oracle.fill_batch(case.x[None], metric="l2")
    sky_rows = int((case.far_rows(15 if name == "win15" else 10) >= l2_ref.row_threshold(W)).sum())
    for path in ("auto", "general"):
        got, stats = run(op2, case.x, path)
        if path == "auto":
            owned_by(stats, "window", sky_rows, W)
        else:
            owned_by(stats, "rows")
        for k, ((i, j), (wi, wj)) in case.planted.items():
            assert got["depth"][i, j] == case.x[wi, wj], "%s %s: pixel %s took the source at %s" % (
                name, path, k, np.argwhere(case.x == got["depth"][i, j]).tolist())
        assert_reference(got, case, "%s %s" % (name, path))
        assert_oracle(got, want, "%s %s" % (name, path))

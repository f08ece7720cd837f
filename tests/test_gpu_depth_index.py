"""depth_list[label - 1] (csrc/dtfill_index.hpp) at every kernel site that applies it, through every case of numpy's rule.

Sites: l1_cv -- the window kernel's epilogue (k_fused), fin_body (the any-distance kernels), pts_body (a handful of sources, its
plain pixels and its tie pixels), and chains handed on to k_tiesx (hand_on_append); l2 -- k_l2win<10>, k_l2win<15>, l2far_pixel
in k_l2far, l2sky_row, l2env_row, l2pts_tile.  Each site has a base frame F that takes its route (the shapes other tests of
this suite use for that route; the route is asserted with pass_stats() where it shows there).

Cases, from F (source values in (0.95, 10)) and the thresholds (source, value):
  (a) masks agree                    F                                  (0.1, 0.1)    status 0
  (b) more values than sources       F with F[5, :40] = 0.5             (0.1, 0.1)    status 0
  (c) fewer values than sources      F                                  (0.1, 5.0)    IndexError
  (c1) ONE value fewer than sources  F                                  (0.1, F's smallest value)  IndexError: only the last
       label is out of bounds, its index == nval exactly -- the case in which `<` typed as `<=` loses the status bit
  (d) sources, no value              F                                  (0.1, 100.0)  IndexError
  (e) no source, values              zeros, five values in row 3        (0.1, 0.1)    status 0, label 0, the LAST value everywhere
  (f) no source, no value            zeros                              (0.1, 0.1)    IndexError
(a), (b), (e), (f) run as ONE batch: only (f)'s frame may carry the status bit there, so a bit raised on the wrong frame shows.
The comparison is assert_equal_to_oracle's / assert_l2_equal_to_oracle's (test_gpu_parity.py): index and status exact on every
frame, dt exact (l2: sqrtf of the exact integer, bit for bit), depth on the frames with status 0, outputs and workspace poisoned first.

test_l2_output_subsets: the l2 sites' frames again, asked for every proper subset of the three outputs -- the `if (out_...)`
branches of the l2 bodies, with the route asserted."""
import itertools

import numpy as np
import pytest

from guarded import KINDS, is_poison, poison_op
from helpers import dt_bits

pytestmark = pytest.mark.gpu
_POISON = itertools.count(9300)
LAST_VALUE = np.float32(0.45)


def scattered(H, W, p, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p, rng.uniform(0.95, 10, (H, W)), 0).astype(np.float32)


def points(H, W, n, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros((H, W), np.float32)
    f.flat[rng.choice(H * W, n, replace=False)] = rng.uniform(0.95, 10, n)
    return f


def case_batch(F):
    """(a), (b), (e), (f) of base frame F as one batch"""
    x = np.zeros((4,) + F.shape, np.float32)
    x[0] = x[1] = F
    x[1, 5, :40] = 0.5
    x[2, 3, 4:9] = [0.5, 0.4, 0.3, 0.2, LAST_VALUE]
    return x


def compare(oracle, op, metric, x, st, vt, path, want_status):
    """One poisoned pass over x against the oracle; returns the pass's statistics.  path "fused" leaves the frames the window
    kernel cannot finish undefined and says which (status bit 2): those are compared on the other paths only."""
    import torch

    depth, dt, idx, status = oracle.fill_batch(x, st, vt, metric=metric)
    assert status.tolist() == want_status, "the oracle itself: %s" % status.tolist()
    xd = torch.from_numpy(x).to("cuda:0")
    poison_op(op, next(_POISON), xd.shape, path=path)
    res = op.run(xd, st, vt, path=path)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    done = (got["status"] & 2) == 0 if path == "fused" else np.ones(len(x), bool)
    what = "%s %s (%g, %g)" % (metric, path, st, vt)
    bad = got["index"][done] != idx[done]
    assert not bad.any(), "%s: index differs at %d px, first %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())
    assert np.array_equal(got["status"][done] & 1, status[done]), "%s: status %s, want %s" % (what, got["status"].tolist(), status.tolist())
    if metric == "l2":
        assert np.array_equal(dt_bits(got["dt"][done]), dt_bits(dt[done])), "%s: distance differs" % what
        assert np.array_equal(np.isinf(got["dt"][done]), np.isinf(dt[done])), what
    else:
        assert np.array_equal(got["dt"][done], dt[done]), "%s: distance map differs" % what
    ok = done & (status == 0)
    assert np.array_equal(got["depth"][ok], depth[ok], equal_nan=True), "%s: depth differs" % what
    return op.pass_stats(), done, (depth, idx)


def all_cases(oracle, op, metric, F, path, route):
    """Every case of base frame F on one path; route(stats) asserts, after a pass whose frames are all F's, that F took
    the kernels this site is about"""
    x = case_batch(F)
    _, done, (depth, idx) = compare(oracle, op, metric, x, 0.1, 0.1, path, [0, 0, 0, 1])
    assert done[0] and done[1]
    assert not idx[2].any() and np.all(depth[2] == LAST_VALUE)  # (e): the wrap, as the oracle gives it
    if path == "fused":  # the frames without a source are not the window kernel's: they are compared on the default path
        compare(oracle, op, metric, x, 0.1, 0.1, "auto", [0, 0, 0, 1])
    for vt in (float(F[F > 0].min()), 5.0, 100.0):  # (c1), (c), (d)
        stats, done, _ = compare(oracle, op, metric, F[None], 0.1, vt, path, [1])
        assert done[0]
        route(stats)


@pytest.fixture(scope="module")
def op2(pkg, gpu_op):
    return pkg.device.DtFill(device="cuda:0", metric="l2")


def test_l1_window_kernel(gpu_op, oracle):
    """k_fused's epilogue (the misaligned branch: depth_index_pos): 5 % at 64 x 96, the window kernel alone"""
    def route(stats):
        assert stats["window"] == stats["all"]
    all_cases(oracle, gpu_op, "l1_cv", scattered(64, 96, 0.05, 1), "fused", route)


def test_l1_any_distance_kernels(gpu_op, oracle):
    """fin_body (depth_index: it also owns the frames without a source): the same frame on the any-distance kernels"""
    def route(stats):
        assert stats["anydist"] == stats["all"]
    all_cases(oracle, gpu_op, "l1_cv", scattered(64, 96, 0.05, 1), "general", route)


def test_l1_handful_of_sources(gpu_op, oracle):
    """pts_body, both of its sites (the pixels with one nearest source, and the tie pixels behind their chains): 24 sources"""
    def route(stats):
        assert stats["points"] > 0
    all_cases(oracle, gpu_op, "l1_cv", points(64, 96, 24, 2), "auto", route)


@pytest.mark.parametrize("path", ("auto", "general"))
def test_l1_chains_handed_on(gpu_op, oracle, path):
    """Two sources on a diagonal at 90 x 130: every pixel of the band between them is a tie pixel, the chains cross the tiles'
    seams and go through hand_on_append to k_tiesx -- from pts_body (auto) and from fin_body (general).  The two values lie
    either side of (c)'s value threshold."""
    F = np.zeros((90, 130), np.float32)
    F[10, 10], F[50, 50] = 3.0, 7.0
    all_cases(oracle, gpu_op, "l1_cv", F, path, lambda stats: None)


def _window_all(stats):
    assert stats["window"] == stats["all"]


def _window_no_points(stats):
    assert stats["window"] > 0 and stats["points"] == 0


def _window_and_rows(stats):
    assert stats["window"] > 0 and stats["anydist"] > 0


def _rows_all(stats):
    assert stats["anydist"] == stats["all"]


def _points_all(stats):
    assert stats["points"] == stats["all"]


def _holed():
    F = scattered(160, 600, 0.06, 5)
    F[40:120, 200:420] = 0
    return F


# one frame per l2 site: (the frame, the path that sends it there, what pass_stats() must say after a pass over it alone)
L2_SITES = {
    "win10": (lambda: scattered(64, 256, 0.05, 3), "auto", _window_all),            # k_l2win<10>: 5 % at 64 x 256
    "win15": (lambda: scattered(130, 1216, 0.012, 4), "auto", _window_no_points),   # k_l2win<15>: 1.2 % at 130 x 1216
    "far_and_sky": (_holed, "auto", _window_and_rows),                              # k_l2far + l2sky_row: 6 % at 160 x 600 with a hole
    "row_search": (lambda: scattered(64, 256, 0.05, 3), "general", _rows_all),      # l2env_row: the general path
    "points": (lambda: points(128, 640, 60, 6), "auto", _points_all),               # l2pts_tile: 60 sources at 128 x 640
}


def test_l2_window_radius_10(op2, oracle):
    """k_l2win<10>: 5 % at 64 x 256"""
    F, path, route = L2_SITES["win10"]
    all_cases(oracle, op2, "l2", F(), path, route)


def test_l2_window_radius_15(op2, oracle):
    """k_l2win<15>: 1.2 % at 130 x 1216"""
    F, path, route = L2_SITES["win15"]
    all_cases(oracle, op2, "l2", F(), path, route)


def test_l2_far_list_and_sky_rows(op2, oracle):
    """l2far_pixel in k_l2far and l2sky_row: 6 % at 160 x 600 with the hole [40:120, 200:420].  A row with at least W / 8 pixels
    that have no source within the window's radius 10 is redone whole (l2sky_row: the hole's inner rows), the far pixels of the
    other rows go on the far list one by one (k_l2far: the hole's first and last rows).  That the frame has both kinds of row is
    checked here on the oracle's distances."""
    F, path, route = L2_SITES["far_and_sky"]
    F = F()
    far = (oracle.fill_batch(F[None], metric="l2")[1][0] > 10).sum(1)
    assert (far >= 600 // 8).any() and ((far > 0) & (far < 600 // 8)).any()
    all_cases(oracle, op2, "l2", F, path, route)


def test_l2_row_search(op2, oracle):
    """l2env_row (depth_index: it also owns the frames without a source): 5 % at 64 x 256 on the general path, which sends
    every frame to the row search (0.3 % at 200 x 640 has at most 512 sources and would be l2pts_tile's)"""
    F, path, route = L2_SITES["row_search"]
    all_cases(oracle, op2, "l2", F(), path, route)


def test_l2_handful_of_sources(op2, oracle):
    """l2pts_tile: 60 sources at 128 x 640"""
    F, path, route = L2_SITES["points"]
    all_cases(oracle, op2, "l2", F(), path, route)


@pytest.fixture(scope="module")
def l2_site_oracle(oracle):
    """site -> (the frame as a batch of one, the oracle's depth, dt, index): computed once per site, never written to"""
    cache = {}

    def get(site):
        if site not in cache:
            x = L2_SITES[site][0]()[None]
            depth, dt, idx, status = oracle.fill_batch(x, 0.1, 0.1, metric="l2")
            assert status.tolist() == [0]
            cache[site] = (x, {"depth": depth, "dt": dt, "index": idx})
        return cache[site]
    return get


OUTPUTS = ("depth", "dt", "index")
SUBSETS = [c for n in (1, 2) for c in itertools.combinations(OUTPUTS, n)]


@pytest.mark.parametrize("subset", SUBSETS, ids="+".join)
@pytest.mark.parametrize("site", list(L2_SITES))
def test_l2_output_subsets(op2, l2_site_oracle, site, subset):
    """Every l2 site asked for every proper, non-empty subset of (depth, dt, index): the wanted outputs equal the oracle's bit for
    bit, every buffer that was not asked for still holds its poison, and the frame took the route of its site."""
    import torch

    x, want = l2_site_oracle(site)
    _, path, route = L2_SITES[site]
    xd = torch.from_numpy(x).to("cuda:0")
    bufs = op2.run(xd, 0.1, 0.1, path=path)  # the operator's three output buffers: run() returns views of them
    seed = next(_POISON)
    kinds = [k for k in KINDS if k != "previous"]  # "previous" leaves values, not poison
    poison_op(op2, seed, xd.shape, kind=kinds[seed % len(kinds)], path=path)
    res = op2.run(xd, 0.1, 0.1, want=subset, path=path)
    torch.cuda.synchronize()
    what = "%s, want %s" % (site, "+".join(subset))
    assert sorted(res) == sorted(subset + ("status",)), what
    assert (res["status"].cpu().numpy() & 1).tolist() == [0], what  # (bit 2, "general path", is informational)
    for name in subset:
        got = res[name].cpu().numpy()
        if name == "dt":
            assert np.array_equal(dt_bits(got), dt_bits(want["dt"])), "%s: distance differs" % what
        else:
            assert np.array_equal(got, want[name]), "%s: %s differs" % (what, name)
    for name in OUTPUTS:
        if name not in subset:
            assert is_poison(bufs[name].cpu().numpy(), name).all(), "%s: %s was written" % (what, name)
    route(op2.pass_stats())

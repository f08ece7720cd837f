"""The routing rule and the tilings the kernels share (csrc/dtfill_route.hpp: the constants, route_decide, sky_possible, far_row,
window_tiling, tile_row_height, tile_row_culled, pts_tall, w2_row_t) are the ones tests/exhaustive_cases.py, tests/l2_ref.py and
tests/lidar_cases.py restate -- the restatement the GPU sweeps hold the device's pass_stats() to.  A host compiler reads the header
as it stands (tests/route_main.cpp answers cases from stdin), built with -fsanitize=undefined where the compiler has it, so a
changed constant, a `>=` typed as `>` or an overflow at the largest legal shapes fails here, without a GPU."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import exhaustive_cases as E
import l2_ref
import lidar_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distancetransform-depthcompletion_amd", "csrc")
MODES = (0, E.FM_GENERAL, E.FM_L2, E.FM_L2 | E.FM_GENERAL, E.FM_PREMARK | E.FM_PTS)
SUMMARY = ("H", "W", "mode", "nsrc", "dlb", "bandmax", "nfar16", "nfar32", "r0", "sky_ok")


class Header:
    """The compiled tests/route_main.cpp: consts (name -> value) and ask(lines) -> one answer line per case line."""

    def __init__(self, exe):
        self.exe = exe
        out = self.run("")
        self.consts = {k: int(v) for k, v in (ln.split() for ln in out[:out.index("end")])}

    def run(self, text):
        return subprocess.run([self.exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()

    def ask(self, lines):
        out = self.run("".join(ln + "\n" for ln in lines))
        out = out[out.index("end") + 1:]
        assert len(out) == len(lines)
        return out

    def routes(self, summaries):
        return [int(v) for v in self.ask(["route " + " ".join(str(int(s[k])) for k in SUMMARY) for s in summaries])]

    def tiles(self, cases):
        """(H, W, R, tbase) -> dict(TH, TW, tiles_x, nty, ntiles, trh, rows, cols)"""
        out = []
        for ln in self.ask(["tiles %d %d %d %d" % c for c in cases]):
            f = ln.split()
            at = f.index("cols")
            assert f[6] == "rows"
            d = dict(zip(("TH", "TW", "tiles_x", "nty", "ntiles", "trh"), map(int, f[:6])))
            d["rows"], d["cols"] = [int(v) for v in f[7:at]], [int(v) for v in f[at + 1:]]
            out.append(d)
        return out

    def culled(self, cases):
        return [bool(int(v)) for v in self.ask(["cull %d %d" % c for c in cases])]


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("route") / "route")
    cmd = [cxx, "-std=c++14", "-O1", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "route_main.cpp")]
    ubsan = ["-fsanitize=undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + ubsan, capture_output=True).returncode != 0:  # (a compiler without the UBSan runtime)
        subprocess.run(cmd, check=True)
    return Header(exe)


def test_constants(header):
    c = header.consts
    want = dict(F_WHM=E.F_WHM, F_WWM=E.F_WWM, L2_PTS_MAX=E.L2_PTS_MAX, W2_R16=E.W2_R[16], W2_R32=E.W2_R[32], PTS_BAND_MAX=E.PTS_BAND_MAX,
                PM16=E.PREMARK[16], PM32=E.PREMARK[32], SKY_MIN=E.SKY_MIN, SKY_MAX=E.SKY_MAX, ROUTE_POINTS=E.ROUTE_POINTS, ROUTE_PREMARK=0x100,
                W2_TH=E.W2_TH, W2_TW=E.W2_TW, PT_T=E.PT_T, PTS_WIDE_TH=E.PTS_TILES[False][0], PTS_WIDE_TW=E.PTS_TILES[False][1],
                PTS_TALL_TH=E.PTS_TILES[True][0], PTS_TALL_TW=E.PTS_TILES[True][1], DENSITY_LN_N=E.DENSITY_LN_N, FM_GENERAL=E.FM_GENERAL,
                FM_L2=E.FM_L2, FM_PREMARK=E.FM_PREMARK, FM_PTS=E.FM_PTS)
    assert c == want
    assert E.PTS_WAVE == (32, 64) and all(th % E.PTS_WAVE[0] == 0 and tw % E.PTS_WAVE[1] == 0 for th, tw in E.PTS_TILES.values())
    widths = list(range(1, 8192))
    rowt = [int(v) for v in header.ask(["rowt %d" % w for w in widths])]
    assert rowt == [l2_ref.row_threshold(w) for w in widths] == [E.w2_row_t(w) for w in widths]
    assert lidar_cases.L2_ROW_T == rowt[1216 - 1]


def density_edges(R):
    """(rest, W, nsrc) with nsrc * ball one below, at and one above DENSITY_LN_N * rest * W -- up to two of each kind with the
    smallest W, for a few heights"""
    ball = 2 * R * R + 2 * R + 1
    out = []
    for rest in (1, 7, 101, 352):  # (coprime to both balls, 545 and 2113)
        found = {-1: 0, 0: 0, 1: 0}
        for W in range(1, 4000):
            t = E.DENSITY_LN_N * rest * W
            for off in (-1, 0, 1):
                if (t + off) % ball == 0 and found[off] < 2:
                    found[off] += 1
                    out.append((rest, W, (t + off) // ball))
        assert min(found.values()) >= 1
    return out


def edge_summaries():
    out = []

    def add(H, W, nsrc, dlb, bandmax, nfar16, nfar32, r0, premark_sky=None):
        for mode in MODES:
            sky = E.sky_possible(mode == E.FM_PREMARK | E.FM_PTS, r0, H) if premark_sky is None else premark_sky
            out.append(dict(zip(SUMMARY, (H, W, mode, nsrc, dlb, bandmax, nfar16, nfar32, r0, sky))))

    # the density rule on the rows left to the window (the row flags) and on the whole frame (every other mode), dlb on its edge
    for R in (16, 32):
        for rest, W, nsrc in density_edges(R):
            for dlb in (0, R, R + 1):
                add(rest, W, nsrc, dlb, 97, 0, 0, 0)             # H = rest
                add(rest + 23, W, nsrc, dlb, 97, 3, 3, 20)       # 20 rows of sky, 3 far rows
                add(rest + 23, W, nsrc, dlb, 97, 3, 3, 20, premark_sky=False)
                add(rest + 5, W, nsrc, dlb, 97, 5 if R == 16 else 0, 5 if R == 32 else 0, 0)
    # the counts, the band, the first source row, the vertical reach, a window left with no row or one
    for H, W in ((352, 1216), (400, 300)):
        for nsrc, bandmax, r0, dlb in itertools.product((0, 1, 512, 513, 3000, 11000), (96, 97), (0, 8, 9, 320, 321, H - 1, H), (0, 16, 17, 32, 33)):
            sky = r0 if E.sky_possible(True, r0, H) else 0
            for n16, n32 in ((0, 0), (H - sky - 1, H - sky), (H - sky, H - sky - 1), (H - sky, H - sky), (H - 1, H)):
                add(H, W, nsrc, dlb, bandmax, n16, n32, r0)
    # the largest shapes the ABI takes
    for H, W in ((4096, 4097), (4097, 4096), (1, 8192), (8192, 1), (2, 8191), (8191, 2)):
        for nsrc, (n16, n32), r0 in itertools.product((0, 513, H * W - 1, H * W), ((0, 0), (H - 1, H - 1), (H, H)), (0, min(9, H - 1), H)):
            add(H, W, nsrc, 0, min(nsrc, 32 * W), n16, n32, r0)
            add(H, W, nsrc, H, min(nsrc, 32 * W), n16, n32, r0)
    return out


def test_decision_edges(header):
    cases = edge_summaries()
    got = header.routes(cases)
    seen = set()
    for s, r in zip(cases, got):
        assert r == E.decide(**s), s
        seen.add((s["mode"], r))
        if s["mode"] == E.FM_L2:
            ref = l2_ref.l2_route(s["nsrc"], s["H"], s["W"])
            assert (E.ROUTE_POINTS if ref == "points" else ref) == r, s
    # every mode met every route it can take
    for mode in MODES:
        want = {0} if mode & E.FM_GENERAL else {0, 16, 32} | ({E.ROUTE_POINTS} if mode else set())
        assert {r for m, r in seen if m == mode} == want, mode
    cull = [(keep, rows) for rows in (1, 3, 4, 5, 8, 40, 63, 64, 96) for keep in sorted({0, 1, rows // 4 - 1, rows // 4, rows // 4 + 1, rows} - {-1})]
    cull += [(10, 39), (10, 40), (10, 41), (24, 95), (24, 96), (24, 97)]
    assert header.culled(cull) == [E.tile_row_culled(*c) for c in cull]
    assert E.tile_row_culled(10, 40) and not E.tile_row_culled(10, 39) and not E.tile_row_culled(0, 40)
    sky = [(p, r0, H) for p in (0, 1) for H in (1, 9, 10, 321, 322, 352) for r0 in (0, 8, 9, 10, 320, 321, H - 1, H) if r0 >= 0]
    assert [bool(int(v)) for v in header.ask(["sky %d %d %d" % c for c in sky])] == [E.sky_possible(*c) for c in sky]
    far = list(itertools.product((0, 1), (16, 32), (4, 5, 6), (5,), (0, 8, 9, 10, 11, 15, 16, 17, 1 << 20)))
    assert [bool(int(v)) for v in header.ask(["far %d %d %d %d %d" % c for c in far])] == [bool(E.far_row(*c)) for c in far]


def test_tilings(header):
    cases = [(H, W, R, tbase) for R in (16, 32) for H in range(1, 301) for W in (1, 31, 32, 33, 159, 160, 161, 200, 640, 1216)
             for tbase in (0, 9, H // 3)]
    cases += [(352, 1216, R, 100) for R in (16, 32)] + [(H, W, R, 0) for R in (16, 32) for H, W in ((352, 1216), (480, 640), (2048, 2048))]
    for (H, W, R, tbase), t in zip(cases, header.tiles(cases)):
        rows, cols = E.window_tiles(H, W, R, tbase)
        assert t["rows"] == list(rows) and t["cols"] == list(cols), (H, W, R, tbase, t)
        assert t["trh"] == E.tile_row_height(H, tbase, t["nty"]) and t["TH"] == E.tile_row_height(H, 0, t["nty"])
        assert t["ntiles"] == t["tiles_x"] * t["nty"] and t["nty"] == -(-H // (E.F_WHM - 2 * R)) and t["tiles_x"] == -(-W // (E.F_WWM - 2 * R))
        # a tile and its halo fit the window; every row from tbase on and every column has a tile
        assert 0 < t["TH"] <= E.F_WHM - 2 * R and 0 < t["TW"] <= E.F_WWM - 2 * R and t["nty"] * t["TH"] >= H and t["tiles_x"] * t["TW"] >= W
    shapes = [(H, W) for H in range(1, 201) for W in range(1, 701, 7)] + [(480, 640)]
    for (H, W), ln in zip(shapes, header.ask(["pts %d %d" % s for s in shapes])):
        tall, tall2, tiles_x, ntiles = map(int, ln.split())
        th, tw = E.PTS_TILES[E.pts_tall(H, W)]
        assert (bool(tall), bool(tall2), tiles_x, ntiles) == (E.pts_tall(H, W), E.pts_tall(H, W), -(-W // tw), -(-W // tw) * -(-H // th)), (H, W)
    assert E.pts_tall(480, 640)


def frames_agree(header, frames):
    """frames: (source mask, metric, path).  The Python summary of each goes into the header's route_decide and must give the r
    of route(); the tile rows route() culls by, and its sky-off, redone with the header's tile_row_height / tile_row_culled, must
    give route()'s sky and far.  Returns the routes."""
    sums = [E.summarise(src, E.pass_mode(metric, path)) for src, metric, path in frames]
    want = [E.route(*f) for f in frames]
    got = header.routes(sums)
    assert got == [w["r"] for w in want]
    flagged = [k for k, s in enumerate(sums) if got[k] > 0 and s["mode"] & E.FM_PREMARK]
    tiles = header.tiles([(sums[k]["H"], sums[k]["W"], got[k], sums[k]["r0"] if sums[k]["sky_ok"] else 0) for k in flagged])
    spans, ask = [], []
    for k, t in zip(flagged, tiles):
        s, H = sums[k], sums[k]["H"]
        tbase = s["r0"] if s["sky_ok"] else 0
        assert t["rows"] == list(E.window_tiles(H, s["W"], got[k], tbase)[0])
        sp = [(tbase + ty * t["trh"], min(H, tbase + (ty + 1) * t["trh"])) for ty in range(t["nty"]) if tbase + ty * t["trh"] < H]
        assert [a for a, e in sp] == t["rows"] and sp[-1][1] == H
        spans.append(sp)
        ask += [(int((~s["far"][got[k]][a:e]).sum()), e - a) for a, e in sp]
    culled = header.culled(ask)
    assert [E.tile_row_culled(*c) for c in ask] == culled
    culled = iter(culled)
    for k, sp in zip(flagged, spans):
        s, f = sums[k], sums[k]["far"][got[k]].copy()
        for a, e in sp:
            if next(culled):
                f[a:e] = True
        r0, H = s["r0"], s["H"]
        sky = s["sky_ok"] and not f[r0] and not (r0 + 1 < H and f[r0 + 1])
        assert (r0 if sky else 0, int(f.sum()) + (r0 if s["sky_ok"] and not sky else 0)) == (want[k]["sky"], want[k]["far"]), frames[k][1:]
    return got


def test_random_masks(header):
    rng = np.random.default_rng(17)
    frames = []
    for k in range(2000):
        H, W = int(rng.integers(1, 97)), int(rng.integers(1, 321))
        src = rng.random((H, W)) < np.exp(rng.uniform(np.log(0.0005), np.log(0.3)))
        if k & 1:  # an empty top band, and an inner band emptied
            src[:int(rng.integers(0, 41))] = False
            a = int(rng.integers(0, H))
            src[a:a + int(rng.integers(0, 41))] = False
        frames += [(src, metric, path) for metric in ("l1_cv", "l2") for path in ("auto", "general")]
    got = frames_agree(header, frames)
    auto = [(f[1], r) for f, r in zip(frames, got) if f[2] == "auto"]
    assert {r for m, r in auto if m == "l1_cv"} == {0, 16, 32, E.ROUTE_POINTS} and {r for m, r in auto if m == "l2"} == {0, 16, 32, E.ROUTE_POINTS}
    skies = [E.route(*f)["sky"] for f, r in zip(frames, got) if f[1:] == ("l1_cv", "auto") and r > 0]
    assert sum(s > 0 for s in skies) > 20  # (the sky and the cull are met, not only passed by)


def test_sweeps(header):
    """mask 0 and mask all-ones of every GPU sweep"""
    frames = []
    for fam, anchor in E.sweep_names():
        x = E.sweep(fam, anchor)[0]
        frames += [(E.sources(x[k]), metric, path) for k in (0, len(x) - 1) for metric in ("l1_cv", "l2") for path in ("auto", "general")]
    got = frames_agree(header, frames)
    assert {0, 16, 32, E.ROUTE_POINTS} == set(got)

// dtfill_route.hpp -- which kernel family takes a frame and each of its rows, and the tilings of the kernels that share one:
// the ONE place where the routing rule, its constants and the window kernel's tile geometry are written down
// Part of libdtfill.so (included by dtfill_common.hpp).  Plain C++14, no HIP and no other header: a host compiler reads it as it
// stands (tests/test_route.py feeds tests/route_main.cpp cases and compares what it decides with tests/exhaustive_cases.py).
// frame_facts (dtfill_prepass.hpp) does everything that is parallel -- the scans over the row counts, the ballots, the bit words --
// and asks here for every scalar decision; the host (run_l1, run_l2) and fused_body take the tilings from here.
#pragma once

// ---- the constants ------------------------------------------------------------------------------------------------------
constexpr int F_WHM = 128;  // the window kernel's window: rows
constexpr int F_WWM = 192;  // ... and columns = 6 words
constexpr int ROUTE_POINTS = -1;  // route[b]: l2, at most L2_PTS_MAX sources in the frame (k_l2pts); l1_cv: k_pts's frame
constexpr int L2_PTS_MAX = 512;
constexpr int PTS_BAND_MAX = 96;  // l1_cv: ... and at most this many in any band of 32 rows
constexpr int W2_R16 = 10, W2_R32 = 15;  // l2: window radius of k_l2win for the frames k_frame routes 16 / 32
// route[b] | ROUTE_PREMARK (l1_cv): k_frame marked rows of the frame for the any-distance kernels up front (rows farther than
// PM16 / PM32 from every row that holds a source: the window kernel with halo 16 / 32 could not decide them, or only by running
// its level loop to the end for a handful of their pixels)
constexpr int ROUTE_PREMARK = 0x100;
constexpr int PM16 = 8, PM32 = 16;
constexpr int SKY_MIN = 9;  // rows above the first source row are k_sky's from this many on (fewer: within every window's reach)
constexpr int SKY_MAX = 320;  // ... and up to this many (k_sky's blocks stage r0 + 260 columns in LDS, in k_colT's launch)
constexpr int W2_TH = 32, W2_TW = 256;  // k_l2win's tile
constexpr int PT_T = 32;                // l2 points route: 32 x 32 tiles (l2pts_tile)
// k_pts's tile: 32 x 256 (k_fin's tile) or 64 x 128, see pts_tall()
constexpr int PTS_WIDE_TH = 32, PTS_WIDE_TW = 256, PTS_TALL_TH = 64, PTS_TALL_TW = 128;
// l2: a row with this many far pixels (an eighth of it: the empty sky of a LiDAR frame, not the scattered voids of a uniform one)
// is redone whole by k_l2env instead of pixel by pixel (k_l2far)
constexpr unsigned w2_row_t(int W) { return (unsigned)((W >> 3) > 32 ? (W >> 3) : 32); }

// the mode bits of a pass, as the host hands them to frame_facts
constexpr int FM_GENERAL = 1;  // every frame takes the any-distance kernels (tests)
constexpr int FM_L2 = 2;       // l2: the window kernel's cost does not grow with the distances it meets
constexpr int FM_PREMARK = 4;  // l1_cv without a depth epilogue: rows too far from every source row are handed on up front
constexpr int FM_PTS = 8;      // l1_cv: a frame with a handful of sources may go to k_pts

// ---- the tilings --------------------------------------------------------------------------------------------------------
// Geometry of one halo's tiling of the window kernel (the window is always F_WHM x F_WWM; FR = halo = largest distance the
// window can decide)
struct FusedTiles {
    int TH, TW, tiles_x, ntiles, nty;  // TH: the tile rows' height when they split the whole frame (the largest it gets)
};
constexpr FusedTiles window_tiling(int H, int W, int R) {
    const int THM = F_WHM - 2 * R, TWM = F_WWM - 2 * R;
    const int nty = (H + THM - 1) / THM, ntx = (W + TWM - 1) / TWM;
    FusedTiles t{};
    t.TH = (H + nty - 1) / nty;  // even split
    t.TW = (W + ntx - 1) / ntx;
    // columns in whole 128-byte lines when the window allows it: the runs of a tile row a wave stores are then whole lines
    if (((t.TW + 31) & ~31) <= TWM) t.TW = (t.TW + 31) & ~31;
    t.tiles_x = ntx;
    t.nty = nty;
    t.ntiles = ntx * nty;
    return t;
}
// the height of the window kernel's tile rows: nty of them split the rows from tbase on evenly -- tbase = the first source row
// when the rows above are the sky's, else 0 (FI_TR0).  frame_facts culls by it, fused_body stores by it.
constexpr int tile_row_height(int H, int tbase, int nty) { return (H - tbase + nty - 1) / nty; }
// a tile row of `rows` rows that is left with only `keep` of them (the others pre-marked) is not worth its windows: all of it
// goes to the any-distance kernels
constexpr bool tile_row_culled(int keep, int rows) { return keep != 0 && 4 * keep <= rows; }

// k_pts: 32 x 256 tiles or 64 x 128, whichever wastes fewer waves on the shape (640 columns are 2.5 tiles of 256 but 5 of 128)
struct PtsTiles {
    bool tall;
    int tiles_x, ntiles;
};
constexpr int pts_tiles_x(int W, bool tall) { return tall ? (W + PTS_TALL_TW - 1) / PTS_TALL_TW : (W + PTS_WIDE_TW - 1) / PTS_WIDE_TW; }
constexpr int pts_tiles_y(int H, bool tall) { return tall ? (H + PTS_TALL_TH - 1) / PTS_TALL_TH : (H + PTS_WIDE_TH - 1) / PTS_WIDE_TH; }
constexpr bool pts_tall(int H, int W) { return pts_tiles_x(W, true) * pts_tiles_y(H, true) < pts_tiles_x(W, false) * pts_tiles_y(H, false); }
constexpr PtsTiles pts_tiling(int H, int W) {
    return PtsTiles{pts_tall(H, W), pts_tiles_x(W, pts_tall(H, W)), pts_tiles_x(W, pts_tall(H, W)) * pts_tiles_y(H, pts_tall(H, W))};
}

// ---- the decision -------------------------------------------------------------------------------------------------------
// Row structure of the frame (l1_cv uses all of it, l2 only FI_DLB and the far rows):
//   r0     the first row that holds a source.  The rows above it -- the empty sky of a LiDAR frame -- need no search at all:
//          every source is below them, so cv2's backward sweep alone decides them, row by row from the two rows beneath
//          (k_sky).
//   vd(i)  vertical distance of row i to the nearest row with a source: every pixel of row i is at least that far from
//          every source.  A row at or below r0 with vd above a window kernel's reach (PM16 / PM32) cannot be decided by it: it
//          is handed to the any-distance kernels up front, and the window kernel takes the rest of the frame instead of nothing.
//          l2: the rows farther from every row with a source than the window kernel's radius (no pixel of them has a source in
//          its window).
// rows [0, r0) can be k_sky's
constexpr bool sky_possible(bool premark, int r0, int H) { return premark && r0 >= SKY_MIN && r0 <= SKY_MAX && r0 < H; }
// row i is out of reach of the window kernel of route R (16 / 32)
constexpr bool far_row(bool l2, int R, int i, int r0, int vd) {
    return l2 ? vd > (R == 16 ? W2_R16 : W2_R32) : (i >= r0 && vd > (R == 16 ? PM16 : PM32));
}

// what the scans over a frame's row counts produced
struct RouteIn {
    int H, W, mode;   // mode: FM_* bits
    int nsrc;         // sources in the frame
    int dlb;          // max vd: lower bound of the largest distance in the frame
    int bandmax;      // the most sources in a band of 32 rows (k_pts's tiles are that high)
    int nfar16, nfar32;  // rows with far_row(.., 16, ..) / far_row(.., 32, ..)
    int r0;
    bool sky_ok;      // sky_possible()
};

// Which kernel family takes the frame -- a speed heuristic, never a correctness condition (the window kernels hand on
// every row in which they meet a pixel they cannot decide).  With source density p the chance that a pixel has no
// source within L1 distance R is about (1-p)^(2 R^2 + 2 R + 1); if the frame is expected to hold such pixels all
// over (N (1-p)^ball > ~1, i.e. p * ball < ln N ~ 14), a window kernel with halo R would do its work for nothing.
// Runs of source-free rows do not say no (l1_cv): the density is judged on the rows that are left to the window.
// Without the row flags (a depth epilogue: a handed-on row costs the whole frame there, k_fused's kept depths being
// cropped / floored already; the forced paths of the tests) the old rule stays: a run of source-free rows that forces a
// distance above R sends the frame to the any-distance kernels.  The l2 window kernel counts its far pixels itself.
constexpr int DENSITY_LN_N = 14;
// (One return per mode, as frame_facts had it: folded into one comparison over "the rows the density is judged on", every
// window block of k_fused came out 80 instructions shorter and the headline 0.13 % slower in six alternating runs --
// profiles/r17/rejected_merged_fits_headline.txt.  The decision sits on that kernel's serial start-up.)
constexpr bool window_fits(const RouteIn &f, int R, int nfar) {
    const long long ball = 2 * R * R + 2 * R + 1;
    if (f.mode & FM_L2) return (long long)f.nsrc * ball >= (long long)DENSITY_LN_N * f.H * f.W;
    if (!(f.mode & FM_PREMARK)) return (long long)f.nsrc * ball >= (long long)DENSITY_LN_N * f.H * f.W && f.dlb <= R;
    const int rest = f.H - (f.sky_ok ? f.r0 : 0) - nfar;  // the rows left to the window
    return rest > 0 && (long long)f.nsrc * ball >= (long long)DENSITY_LN_N * rest * f.W;
}
// route: halo 16 if it fits, else halo 32 (three times the work per pixel, still cheaper than the any-distance
// kernels at a few percent density), else the any-distance kernels.  The route without ROUTE_PREMARK: 16, 32, 0 or ROUTE_POINTS
constexpr int route_decide(const RouteIn &f) {
    const bool l2 = f.mode & FM_L2, force_general = f.mode & FM_GENERAL;
    const bool handful = f.nsrc > 0 && f.nsrc <= L2_PTS_MAX;
    // l2, a handful of sources (the NYU sampling patterns): ROUTE_POINTS -- every 32 x 32 tile looks at the sources that can
    // own one of its pixels, found by distance from the tile's centre (l2pts_tile); the blocks of k_l2win's launch
    // write the list of sources
    const bool points = l2 && !force_general && handful;
    // l1_cv, a handful of sources and too thin for a window: k_pts (per tile, the sources whose cells reach it).  Not when they
    // crowd into one band of rows: its tiles would look at all of them for every pixel.
    const bool points1 = !l2 && (f.mode & FM_PTS) && handful && f.bandmax <= PTS_BAND_MAX;
    const int window = window_fits(f, 16, f.nfar16) ? 16 : window_fits(f, 32, f.nfar32) ? 32 : 0;
    return force_general ? 0 : points ? ROUTE_POINTS : window ? window : points1 ? ROUTE_POINTS : 0;
}

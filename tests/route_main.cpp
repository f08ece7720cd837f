// Prints what the kernels' routing header (csrc/dtfill_route.hpp) states and decides.  First its constants, one "NAME value" per
// line, then "end"; then one answer line per case line read from stdin:
//   route H W mode nsrc dlb bandmax nfar16 nfar32 r0 sky_ok   ->  route_decide of that summary
//   tiles H W R tbase   ->  TH TW tiles_x nty ntiles, tile_row_height, then the tile rows' and tile columns' origins inside the frame
//   pts H W             ->  pts_tall, and pts_tiling's tall, tiles_x and ntiles
//   rowt W              ->  w2_row_t
//   cull keep rows      ->  tile_row_culled
//   sky premark r0 H    ->  sky_possible
//   far l2 R i r0 vd    ->  far_row
// Host-only: tests/test_route.py compiles it with the host compiler (with -fsanitize=undefined where the compiler has it, so that
// an overflow at the largest legal shapes is a failure) and compares the lines with tests/exhaustive_cases.py.
#include <cstdio>
#include <cstring>

#include "dtfill_route.hpp"

// through compile-time constants, as the host's and the kernels' call sites may take them
static_assert(window_tiling(352, 1216, 16).ntiles == window_tiling(352, 1216, 16).tiles_x * window_tiling(352, 1216, 16).nty, "constexpr tiling");
static_assert(route_decide(RouteIn{1, 1, FM_GENERAL, 1, 0, 1, 0, 0, 0, false}) == 0, "constexpr decision");

#define CONST(name) std::printf(#name " %d\n", (int)(name))

int main() {
    CONST(F_WHM); CONST(F_WWM); CONST(L2_PTS_MAX); CONST(W2_R16); CONST(W2_R32); CONST(PTS_BAND_MAX); CONST(PM16); CONST(PM32);
    CONST(SKY_MIN); CONST(SKY_MAX); CONST(ROUTE_POINTS); CONST(ROUTE_PREMARK); CONST(W2_TH); CONST(W2_TW); CONST(PT_T);
    CONST(PTS_WIDE_TH); CONST(PTS_WIDE_TW); CONST(PTS_TALL_TH); CONST(PTS_TALL_TW); CONST(DENSITY_LN_N);
    CONST(FM_GENERAL); CONST(FM_L2); CONST(FM_PREMARK); CONST(FM_PTS);
    std::printf("end\n");
    char line[256], what[16];
    while (std::fgets(line, sizeof line, stdin)) {
        int a[10] = {0}, used = 0;
        if (std::sscanf(line, "%15s%n", what, &used) != 1) continue;
        const int n = std::sscanf(line + used, "%d %d %d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9);
        if (!std::strcmp(what, "route") && n == 10) {
            std::printf("%d\n", route_decide(RouteIn{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9] != 0}));
        } else if (!std::strcmp(what, "tiles") && n == 4) {
            const int H = a[0], W = a[1], tbase = a[3];
            const FusedTiles t = window_tiling(H, W, a[2]);
            const int TH = tile_row_height(H, tbase, t.nty);
            std::printf("%d %d %d %d %d %d rows", t.TH, t.TW, t.tiles_x, t.nty, t.ntiles, TH);
            for (int ty = 0; ty < t.nty; ++ty)
                if (tbase + ty * TH < H) std::printf(" %d", tbase + ty * TH);
            std::printf(" cols");
            for (int tx = 0; tx < t.tiles_x; ++tx)
                if (tx * t.TW < W) std::printf(" %d", tx * t.TW);
            std::printf("\n");
        } else if (!std::strcmp(what, "pts") && n == 2) {
            const PtsTiles p = pts_tiling(a[0], a[1]);
            std::printf("%d %d %d %d\n", (int)pts_tall(a[0], a[1]), (int)p.tall, p.tiles_x, p.ntiles);
        } else if (!std::strcmp(what, "rowt") && n == 1) {
            std::printf("%u\n", w2_row_t(a[0]));
        } else if (!std::strcmp(what, "cull") && n == 2) {
            std::printf("%d\n", (int)tile_row_culled(a[0], a[1]));
        } else if (!std::strcmp(what, "sky") && n == 3) {
            std::printf("%d\n", (int)sky_possible(a[0] != 0, a[1], a[2]));
        } else if (!std::strcmp(what, "far") && n == 5) {
            std::printf("%d\n", (int)far_row(a[0] != 0, a[1], a[2], a[3], a[4]));
        } else {
            std::printf("? %s", line);
            return 2;
        }
    }
    return 0;
}

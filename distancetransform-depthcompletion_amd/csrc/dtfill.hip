// dtfill.hip -- MI355X (gfx950) distance-transform + nearest-valid-depth fill.
//
// Replaces, for B frames at once, the reference's per-frame
//   nearest_point()      solution_DeepNet/tools.py:7-10   (cv2.distanceTransformWithLabels, L1, 5x5, LABEL_PIXEL)
//   DT_complete_batch()  solution_DeepNet/tools.py:13-35  (value-list compaction + depth_list[lbl-1] gather)
//   Distance_Transform() solution_DeepNet/eval_NYU.py:120-133
//
// The reference's arithmetic is OpenCV's two-pass 5x5 chamfer: two raster sweeps that are sequential
// in both image axes.  This file does NOT sweep.  It uses the following identity (derived in
// DESIGN.md section 2, checked bit-for-bit against the sequential restatement in oracle/):
//
//   d(q)      = exact L1 distance to the nearest source               (weights {1,2,3} == L1 norms of the taps)
//   live(q)   = "the forward sweep already reached the final value at q"
//             = some nearest source s of q lies in q's forward cone:  s above-or-left of q, or above-right
//               with (s.col - q.col) <= 2 (q.row - s.row)
//   parent(q) = live(q) ? first forward tap r (cv2 order) with live(r) and d(r)+w == d(q)
//                       : first backward tap r (cv2 order) with d(r)+w == d(q)
//   label(q)  = label(root of the parent chain) = 1 + raster rank of that source.
//
// Every hop lowers d by exactly the hop's L1 length, so a chain ends on a NEAREST source of its start pixel, and
// everything that decides label(q) lies inside the L1 ball of radius d(q) around q.
//
// Kernels of one l1_cv pass (six launches; seven with a k_frame launch of its own, see run_l1):
//   k_mask     source / value bit words + per-row prefix popcounts                    reads x once
//              (16-byte or dword row loads; with the outlier filter a second launch redoes the frames with a negative value);
//              clears the per-pass flags that later blocks only raise
//   k_frame    (frame_facts + frame_publish: block 0 of every frame in k_fused's launch, or a launch of its own)
//              per-frame row-count scan -> compaction ranks; frame facts; the row structure (first source row, rows too far
//              from every source row) and with it WHO takes which rows of the frame; value list when the source and value masks
//              of a frame differ; the source list of a frame that holds a handful
//   k_fused    every window block first works out the facts of its own frame from the row counts (frame_facts, the same
//              definition), so that it waits for no other block.  Dense frames (halo 16 or 32 per frame): one workgroup per (tile + halo) window, bit-sliced: the
//              level-synchronous form of the identity on bit planes held in registers, byte codes un-sliced into LDS,
//              lock-step chain walk, rank lookup, depth gather and the three output stores.  Hands a ROW on when one of its
//              pixels is farther than the halo from every source.
//   every other frame, and the handed-on rows (any distance, any density; dtfill_rows.hpp):
//   k_colT     per 32-row band and column: the band's source bits and the distances to the nearest source
//              above / below the band -- everything a row needs to know about its columns; and the label of
//              every source pixel, where k_fin can gather it
//              + k_sky's blocks (dtfill_sky.hpp) in the same launch: the rows above the first source row (the empty sky of a
//              LiDAR frame) in closed form from the two rows beneath
//   k_rows     packed-key min-plus row scans: d, the nearest source (smallest and largest column that reach d:
//              a pixel with ONE nearest source needs no chain), live; distance map + bit planes
//   k_fin      per tile: 5x5 parent rule bit-sliced for the remaining "tie" pixels, their chains (up to four hops through
//              the step bytes in LDS), label + depth of every pixel
//              + the tiles of the frames with a handful of sources ("k_pts", dtfill_pts.hpp) in the same launch: candidates
//              per wave box, dominance pruning, packed-key minima per pixel by one sweep down and one up, the same rule for
//              their tie pixels -- from the source list to the three outputs
//   k_tiesx    the few tie pixels whose chain crosses tiles or runs longer: follows the recorded links
// l2 pass (exact Euclidean, canonical tie-break; dtfill_l2.hpp): k_mask, k_frame, then
//   k_l2win<R> dense frames: (2R+1)^2 windows straight from the bit words, packed-key minimum over the window rows
//   k_l2far    the odd far pixel of a dense frame, half a wave each (l2far_list, l2far_pixel)
//   k_colT     vertical distances per column, for sparse frames and for rows of far pixels (the empty sky); its column words
//              are read through col_dist (dtfill_rows.hpp), by the l2 row searches as l2_column
//   k_l2env    sparse frames: lower envelope of parabolas searched by monotone bisection (l2env_row); rows of far pixels of a
//              dense frame (the sky): a window in the column distances (l2sky_row); frames with a handful of sources: tiles
//              over the source list (l2pts_tile)
//
// Where the routing rule and the tilings are written down: dtfill_route.hpp -- which kernel family takes a frame and each of its
// rows (route_decide, sky_possible, far_row, the mode bits a pass hands to frame_facts), the window kernel's tiling and its tile
// rows under a sky (window_tiling, tile_row_height, tile_row_culled), k_pts's and k_l2win's tiles.  frame_facts, fused_body and
// the host below call it; tests/test_route.py compiles it for the host and holds tests/exhaustive_cases.py to it.
//
// No MFMA in any of the above: this path is compare/min/index work (DESIGN.md "Roofline").  The matmul-shaped entry points are
// dtfill_conv2d (SparsityCNN's layers), dtfill_conv2d_strided and dtfill_conv2d_transpose (ResNet18's wide layers), all three
// dtfill_conv.hpp's, and their gradients dtfill_conv2d_backward_data and dtfill_conv2d_backward_weights (dtfill_conv2d's) and
// dtfill_conv2d_strided_backward_data / _weights and dtfill_conv2d_transpose_backward_data / _weights, all dtfill_convb.hpp's.
// dtfill_max_pool_pyramid and its backward (dtfill_pool.hpp) are compare-and-select work again, and memory-bound.
// dtfill_adam_step (dtfill_adam.hpp) is the training step's last line: Keras' Adam over every variable, one streaming pass.
// dtfill_conv2d_strided_bf16 and dtfill_conv2d_transpose_bf16 (dtfill_convh.hpp) are the wide layers on the bf16 matrix cores,
// the opt-in inference precision, over weights packed once by dtfill_conv2d_pack_bf16.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include "../../include/dtfill.h"

typedef uint16_t u16;
typedef uint8_t u8;
typedef unsigned long long u64;
typedef uint32_t u32;

namespace {

#include "dtfill_common.hpp"
#include "dtfill_prepass.hpp"
#include "dtfill_fused.hpp"
#include "dtfill_rows.hpp"
#include "dtfill_sky.hpp"
#include "dtfill_pts.hpp"
#include "dtfill_l2.hpp"
#include "dtfill_outlier.hpp"
#include "dtfill_gmc.hpp"
#include "dtfill_gmcv.hpp"
#include "dtfill_gmcb.hpp"
#include "dtfill_post.hpp"
#include "dtfill_loss.hpp"
#include "dtfill_lines.hpp"
#include "dtfill_read.hpp"
#include "dtfill_rgb.hpp"
#include "dtfill_nyu.hpp"
#include "dtfill_proj.hpp"
#include "dtfill_unproj.hpp"
#include "dtfill_fillb.hpp"
#include "dtfill_near.hpp"
#include "dtfill_conv.hpp"
#include "dtfill_convb.hpp"
#include "dtfill_pool.hpp"
#include "dtfill_adam.hpp"
#include "dtfill_convh.hpp"
#include "dtfill_convhb.hpp"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The workspace of a pass, 256-byte aligned pieces in this order; with ws = nullptr only the total is worked out
// (dtfill_workspace_bytes).  status is the workspace's frame status (make_pass puts the caller's in its place).
Pass carve(void *ws, int B, int H, int W, size_t *total = nullptr) {
    const size_t N = (size_t)B * H * W;
    const size_t Wd = (size_t)(W + 63) / 64;
    const size_t NW = (size_t)B * H * Wd;
    const size_t NR = (size_t)B * H;
    char *base = static_cast<char *>(ws);
    size_t off = 0;
    Pass c{};
    auto take = [&](size_t bytes) {
        char *r = base ? base + off : nullptr;
        off += align256(bytes);
        return r;
    };
    c.B = B;
    c.H = H;
    c.W = W;
    c.Wd = (int)Wd;
    c.Wp = (int)Wd * 8;
    c.srcbits = (u64 *)take(NW * 8);
    c.valbits = (u64 *)take(NW * 8);
    c.wpre_s = (u16 *)take(NW * 2);
    c.wpre_v = (u16 *)take(NW * 2);
    c.rowcnt_s = (u32 *)take(NR * 4);
    c.rowcnt_v = (u32 *)take(NR * 4);
    c.rowbase_s = (u32 *)take(NR * 4);
    c.rowbase_v = (u32 *)take(NR * 4);
    c.finfo = (int *)take((size_t)B * FI_STRIDE * 4);
    c.fflag2 = (int *)take((size_t)B * 4);
    c.rowfar = (u32 *)take(NR * 4);
    c.route = (int *)take((size_t)B * 4);
    c.status = (int *)take((size_t)B * 4);
    c.negflag = (int *)take((size_t)B * 4);
    // any-distance path (touched only for frames the fused kernel does not take)
    c.nb = (H + 31) / 32;
    c.ctp = ct_pitch(W);
    c.ct = (uint2 *)take((size_t)B * c.nb * c.ctp * sizeof(uint2));
    c.rec = (uint4 *)take(NW * sizeof(uint4));
    c.spix = (u32 *)take(N * 4);
    c.dscratch = (float *)take(N * 4);
    c.xlist = (u32 *)take(N * 4);
    c.xptr = (u32 *)take(N * 4);
    c.plane_bytes = align256(NW * 8);
    c.planes = (u8 *)take(PL_N * c.plane_bytes);
    c.vlist = (float *)take(N * 4);
    c.ptslist = (PtsSrc *)take((size_t)B * L2_PTS_MAX * sizeof(PtsSrc));
    if (total) *total = off;
    return c;
}

// the pass record of one call: the carved workspace, the input and the caller's outputs
Pass make_pass(const float *x, int B, int H, int W, float src_thr, float val_thr, float *out_depth, float *out_dt, int32_t *out_index,
               int32_t *frame_status, void *workspace, DepthEpilogue ep = DepthEpilogue{0, 0, 0.0f}) {
    Pass p = carve(workspace, B, H, W);
    p.x = x;
    p.src_thr = src_thr;
    p.val_thr = val_thr;
    p.out_depth = out_depth;
    p.out_dt = out_dt;
    p.out_index = out_index;
    if (frame_status) p.status = frame_status;
    p.ep = ep;
    if (!out_depth && !out_index) p.rec = nullptr, p.spix = nullptr;  // the distance map alone needs neither sources nor labels
    return p;
}

bool shape_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H + W - 2 < MAX_HW_SUM &&
           (long long)B * H * W < (1ll << 31);  // B is a grid dimension; pixel indices are 32-bit
}

// l1_cv: frames of up to DTFILL_FRAME_RIDE_MAX_H rows have their facts worked out inside k_fused's launch (run_l1)
static_assert(DTFILL_FRAME_RIDE_MAX_H <= F_RIDE_HMAX, "the facts of a riding frame lie in k_fused's ring memory");

// kernel_ms slots of dtfill_batch_timed, in launch order
enum { S1_MASK, S1_FRAME, S1_FUSED, S1_COLT, S1_ROWS, S1_FIN, S1_TIESX, NK_L1 };
const char *const kNamesL1[NK_L1] = {"k_mask", "k_frame", "k_fused", "k_colT", "k_rows", "k_fin", "k_tiesx"};
enum { S2_MASK, S2_FRAME, S2_WIN16, S2_WIN32, S2_FAR, S2_COLT, S2_ENV, NK_L2 };
const char *const kNamesL2[NK_L2] = {"k_mask", "k_frame", "k_l2win<10>", "k_l2win<15>", "k_l2far", "k_colT", "k_l2env"};

// Launch bookkeeping of a pass: ok after every launch; with events (dtfill_batch_timed) slot k's time runs from ev[k] to
// ev[k + 1].  at(k) records every boundary up to ev[k]: the slot of a kernel that does not run is left at 0 ms.
struct Marks {
    hipStream_t st;
    hipEvent_t *ev;
    int k = 0;
    bool ok = true;
    unsigned idle = 0;  // bit k: nothing was launched in slot k
    void at(int slot) {
        ok = ok && hipGetLastError() == hipSuccess;
        if (ev)
            for (; k <= slot; ++k) {
                if (k < slot) idle |= 1u << k;
                (void)hipEventRecord(ev[k], st);
            }
    }
};

// k_mask_plain; with DTFILL_FLAG_OUTLIER_REMOVAL the predicates see outlier_removal(x): k_mask<1, VEC>, VEC when the rows can be
// read 16 bytes at a time, then k_mask<2, VEC> redoes the frames that hold a negative value.
void launch_mask(const Pass &p, unsigned flags, hipStream_t st) {
    const bool vec = (p.W & 3) == 0 && (reinterpret_cast<uintptr_t>(p.x) & 15) == 0;
    const dim3 g(p.B, (p.H + 3) / 4);  // (frames along x)
    if (flags & DTFILL_FLAG_OUTLIER_REMOVAL) {
        // negflag ("this frame holds a negative value", raised by the first launch, read by the second) starts clear whatever
        // the workspace held before
        (void)hipMemsetAsync(p.negflag, 0, (size_t)p.B * sizeof(int), st);
        auto *const filter = vec ? k_mask<1, true> : k_mask<1, false>, *const redo = vec ? k_mask<2, true> : k_mask<2, false>;
        filter<<<g, 256, 0, st>>>(p);
        redo<<<g, 256, 0, st>>>(p);
    } else {
        // a wave takes the rows that fit one batch of words: one row of a KITTI frame, two of NYU's
        const int rows = max(1, MW_NW / p.Wd);
        k_mask_plain<<<dim3(p.B, (p.H + 4 * rows - 1) / (4 * rows)), 256, 0, st>>>(p);
    }
}

// waves per k_colT block: two iterations of two bands per wave (fewer, longer waves fit the CUs in one round)
int colT_waves(int nb) { return min(16, max(2, (nb + 3) / 4)); }

// k_colT, with k_sky's blocks behind the column blocks when sky.nblocks > 0; false if its LDS could not be granted
bool launch_colT(const Pass &p, const SkyArgs &sky, hipStream_t st) {
    int cw = colT_waves(p.nb);
    size_t lds = colT_lds(p.nb);
    if (sky.nblocks) {
        cw = SKY_NT / 64;
        lds = max(lds, sky_lds(sky_span_max(p.H, p.W)));
    }
    bool ok = true;
    if (lds > 48 * 1024)  // (set per call: the attribute belongs to the current device)
        ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_colT), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
    const int ncol = (p.ctp + 63) / 64;
    const int fx = cw <= 4;  // frames along grid x for frames of up to 512 rows (k_colT's comment)
    k_colT<<<fx ? dim3(p.B, ncol + sky.nblocks) : dim3(ncol + sky.nblocks, p.B), 64 * cw, lds, st>>>(p, ncol, sky, fx);
    return ok;
}

int run_l1(Pass p, unsigned flags, hipStream_t st, hipEvent_t *ev, unsigned *idle) {
    const int B = p.B, H = p.H, W = p.W;
    const bool general_only = flags & DTFILL_FLAG_GENERAL_ONLY;
    const bool fused_only = flags & DTFILL_FLAG_FUSED_ONLY;
    Marks m{st, ev};
    // The frame facts: every window block of k_fused works out its own frame's, and the first block of a frame publishes them
    // for the later launches (six launches).  A launch of its own (seven) where there is no window launch, on request, and for
    // tall frames: every window block scans all H row counts (DTFILL_FRAME_RIDE_MAX_H: DESIGN.md section 4).
    const bool ride = !general_only && !(flags & DTFILL_FLAG_SEPARATE_FRAME) && H <= DTFILL_FRAME_RIDE_MAX_H;
    p.ride = ride;
    m.at(S1_MASK);
    launch_mask(p, flags, st);
    // geometry of the window kernel's two tilings (k_frame pre-marks whole tile rows)
    const FusedTiles t16 = window_tiling(H, W, 16), t32 = window_tiling(H, W, 32);
    const bool epi = p.ep.row0 != 0 || p.ep.use_floor;
    // row flags (k_frame): the sky above the first source row goes to k_sky, rows too far from every source row to the
    // any-distance kernels, the rest of the frame to the window kernel.  Not with a depth epilogue (a handed-on row costs the
    // whole frame there) and not on the forced paths of the tests.
    const bool rowflags = !epi && !fused_only && !general_only;
    // k_sky takes the distances of its two base rows from the distance map: without one from the caller, the scratch frame
    float *const out_dt_caller = p.out_dt;
    if (rowflags && !p.out_dt) p.out_dt = p.dscratch;
    const int mode = (general_only ? FM_GENERAL : 0) | (rowflags ? FM_PREMARK | FM_PTS : 0);
    if (!ride) {
        m.at(S1_FRAME);  // (else the slot reads 0 ms)
        k_frame<<<B, 256, 0, st>>>(p, mode, t16.nty, t32.nty);
    }
    m.at(S1_FUSED);
    if (!general_only) {
        // dense frames: the window kernel, halo 16 or 32 per frame (k_frame's route).  It hands rows on (fflag2, rowfar) when a
        // tile pixel turns out to be farther than the halo from every source.
        // streaming stores only where every run of tile pixels a wave stores is whole 128-byte lines
        auto line = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 127) == 0; };
        const bool stream = (W & 31) == 0 && (t16.TW & 31) == 0 && (t32.TW & 31) == 0 && line(p.out_depth) && line(p.out_dt) &&
                            line(p.out_index);
        // frames along x: a frame's tiles beyond its own tiling (they exit) come last
        const dim3 fg(B, max(t16.ntiles, t32.ntiles));
        // the depth epilogue is a template parameter (no streaming stores with it): each instance holds two bodies, not four
        (epi ? k_fused<false, true> : stream ? k_fused<true, false> : k_fused<false, false>)<<<fg, F_NT, 0, st>>>(p.x, p.srcbits, p.wpre_s, p.rowbase_s, p.finfo, p.vlist, H, W, p.Wd, t16, t32,
                                                                      p.out_depth, p.out_dt, p.out_index, p.route, p.fflag2, p.rowfar, p.status, p.ep,
                                                                      frame_args(p, mode, t16.nty, t32.nty, ride, min(t16.ntiles, t32.ntiles)));
    }
    m.at(S1_COLT);
    if (!fused_only) {
        // every other frame: argmin scans, any distance (dtfill_rows.hpp)
        // k_sky's blocks (the rows above the first source row, dtfill_sky.hpp) ride behind the column blocks
        SkyArgs sky = {out_dt_caller, (W + SKY_SW - 1) / SKY_SW, 0};
        const bool sky_rides = rowflags && colT_waves(p.nb) <= SKY_NT / 64;  // (taller frames: a launch of its own, below)
        if (sky_rides) sky.nblocks = sky.nstrips * ((H + SKY_RG - 1) / SKY_RG);
        m.ok = launch_colT(p, sky, st) && m.ok;
        if (rowflags && !sky_rides)
            k_sky<<<dim3(sky.nstrips * ((H + SKY_RG - 1) / SKY_RG), B), SKY_NT, sky_lds(sky_span_max(H, W)), st>>>(p, sky);
        m.at(S1_ROWS);
        // columns per lane: 8 or 10, whichever leaves fewer idle lanes in the row's last wave
        const int nw8 = (W + 511) / 512, nw10 = (W + 639) / 640;
        const bool ten = nw10 * 640 < nw8 * 512;
        auto aligned = [](const void *q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; };
        const int nwv = ten ? nw10 : nw8;
        const bool fin = p.out_depth || p.out_index;  // the distance map alone needs neither sources nor tie-breaks
        const float *dt = p.out_dt;
        // bit 0: a lane's pixels can leave as vectors; bit 1: the distance map goes through LDS and leaves as whole lines
        const int ovec = (ten ? ((W & 1) == 0 && aligned(dt, 8)) : ((W & 3) == 0 && aligned(dt, 16))) |
                         (((W & 31) == 0 && dt && aligned(dt, 128)) ? 2 : 0);
        const size_t rlds = (ovec & 2) ? (size_t)W * sizeof(float) : 0;
        // rows per block: several where a row is one wave, or where there are very many rows (the exit of a frame that has none, or of
        // a row far from every handed-on row, costs a block dispatch per row)
        const int rpb = (nwv == 1 || (long long)H * B >= 16384) && nwv <= 4 ? R_RPB : 1;
        auto *const rows = rpb > 1   ? (ten ? k_rows<10, 256, true> : k_rows<8, 256, true>)
                                             : nwv <= 4 ? (ten ? k_rows<10, 256, false> : k_rows<8, 256, false>)
                                                        : (ten ? k_rows<10, 1024, false> : k_rows<8, 1024, false>);
        rows<<<dim3((H + rpb - 1) / rpb, B), 64 * nwv, rlds, st>>>(p.ct, p.ctp, p.fflag2, H, W, p.nb, p.Wp, p.planes, p.plane_bytes, p.out_dt, p.spix,
                                                                  ovec, p.rowfar, p.finfo, rpb);
        m.at(S1_FIN);
        // the frames with a handful of sources (k_frame: ROUTE_POINTS, fflag 3; only with the row flags) ride in k_fin's launch:
        // their tiles, from the source list to the outputs (dtfill_pts.hpp); k_tiesx finishes the chains that leave a tile
        PtsArgs pa;
        pa.ptslist = p.ptslist;
        pa.out_dt = p.out_dt;
        const PtsTiles pt = pts_tiling(H, W);  // 32 x 256 tiles or 64 x 128
        pa.tall = pt.tall;
        pa.tiles_x = pt.tiles_x;
        pa.ntiles = rowflags ? pt.ntiles : 0;
        const int ttx = (W + Q_TW - 1) / Q_TW;
        pa.fin_ntiles = fin ? ttx * ((H + Q_TH - 1) / Q_TH) : 0;
        if (fin || pa.ntiles) {
            const int vec = (W & 3) == 0 && aligned(p.out_depth, 16) && aligned(p.out_index, 16);
            k_fin<<<dim3(max(pa.fin_ntiles, pa.ntiles), B), Q_NT, 0, st>>>(p.planes, p.plane_bytes, p.Wp, p.fflag2, H, W, p.Wd, ttx, p.spix, p.x, p.rec,
                                                                           p.vlist, p.out_depth, p.out_index, p.status, p.finfo, p.xlist, p.xptr,
                                                                           p.planes + PL_UNRES * p.plane_bytes, vec, p.ep, p.dscratch, p.rowfar, pa);
            m.at(S1_TIESX);
            if (fin) k_tiesx<<<dim3(XL_BLOCKS, B), 256, 0, st>>>(p);
        }
    }
    m.at(NK_L1);
    if (idle) *idle = m.idle;
    return m.ok ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int run_l2(const Pass &p, unsigned flags, hipStream_t st, hipEvent_t *ev, unsigned *idle) {
    const int B = p.B, H = p.H, W = p.W;
    Marks m{st, ev};
    m.at(S2_MASK);
    launch_mask(p, flags, st);
    m.at(S2_FRAME);
    k_frame<<<B, 256, 0, st>>>(p, ((flags & DTFILL_FLAG_GENERAL_ONLY) ? FM_GENERAL : 0) | FM_L2, 0, 0);
    m.at(S2_WIN16);
    // dense frames (k_frame's route 16 / 32): windows of 21 x 21 / 31 x 31 around every pixel, the few pixels with no source
    // that near one by one
    const int ttx = (W + W2_TW - 1) / W2_TW, tty = (H + W2_TH - 1) / W2_TH;
    auto win = [&](auto radius, int want_route) {
        constexpr int R = decltype(radius)::value;
        k_l2win<R><<<dim3(ttx * tty, B), 256, L2Win<R>::LDS, st>>>(p.x, p.srcbits, p.wpre_s, p.rowbase_s, p.finfo, p.vlist, p.xlist, p.route, want_route,
                                                                   p.rowfar, p.fflag2, H, W, p.Wd, ttx, p.out_depth, p.out_dt, p.out_index, p.status);
    };
    win(std::integral_constant<int, W2_R16>{}, 16);
    m.at(S2_WIN32);
    win(std::integral_constant<int, W2_R32>{}, 32);
    m.at(S2_FAR);
    // one wave per listed pixel: enough blocks per frame for ~16 k waves in the batch
    k_l2far<<<dim3(min(256, max(16, 4096 / B)), B), 256, 0, st>>>(p);
    m.at(S2_COLT);
    // vertical distances per column (k_colT) for the frames that need them: route 0, or a row handed on by k_l2win
    m.ok = launch_colT(p, SkyArgs{}, st) && m.ok;
    m.at(S2_ENV);
    // the rows, one wave each; then the 32 x 32 tiles of the frames with a handful of sources, one wave each
    const size_t wave_lds = max(max(l2env_lds(W), (size_t)L2_PTS_MAX * 8), (size_t)(W + 2 * L2S_R) * 8);
    const int ntile = ((H + PT_T - 1) / PT_T) * ((W + PT_T - 1) / PT_T);
    auto env = [&](auto waves, int tpw) {  // waves per block, tiles per wave
        constexpr int WPB = decltype(waves)::value;
        const int nrowblk = (H + WPB - 1) / WPB;
        k_l2env<WPB><<<dim3(B, nrowblk + (ntile + WPB * tpw - 1) / (WPB * tpw)), 64 * WPB, WPB * wave_lds, st>>>(
            p.x, p.ct, p.ctp, p.nb, p.rec, p.Wd, p.finfo, p.vlist, p.route, p.rowfar, p.srclist(), H, W, nrowblk, wave_lds, tpw, p.out_depth,
            p.out_dt, p.out_index, p.status);
    };
    if (4 * wave_lds <= 64 * 1024) {
        env(std::integral_constant<int, 4>{}, 1);
    } else {
        if (wave_lds > 48 * 1024)  // rows wider than ~4900 pixels (set per call: the attribute belongs to the current device)
            m.ok = m.ok && hipFuncSetAttribute(reinterpret_cast<const void *>(k_l2env<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)l2env_lds(8192)) == hipSuccess;
        env(std::integral_constant<int, 1>{}, 8);
    }
    m.at(NK_L2);
    if (idle) *idle = m.idle;
    return m.ok ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// idle (with ev): bit k = slot k's kernel was not launched in this pass
int run(const Pass &p, int metric, unsigned flags, void *stream, hipEvent_t *ev, unsigned *idle = nullptr) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return metric == DTFILL_METRIC_L2 ? run_l2(p, flags, st, ev, idle) : run_l1(p, flags, st, ev, idle);
}

int check_args(const float *x, int B, int H, int W, int metric, float *out_depth, float *out_dt,
               int32_t *out_index, void *workspace, size_t ws_bytes, unsigned flags = 0u) {
    if (!x || !workspace || (!out_depth && !out_dt && !out_index)) return DTFILL_ERR_NULL;
    if (!shape_ok(B, H, W)) return DTFILL_ERR_SHAPE;
    if ((flags & DTFILL_FLAG_OUTLIER_REMOVAL) && (H < 4 || W < 4)) return DTFILL_ERR_SHAPE;  // the 7x7 filter's reflected border
    if (metric != DTFILL_METRIC_L1_CV && metric != DTFILL_METRIC_L2) return DTFILL_ERR_METRIC;
    if (ws_bytes < dtfill_workspace_bytes(B, H, W, metric) || ((uintptr_t)workspace & 255))
        return DTFILL_ERR_WORKSPACE;
    return DTFILL_OK;
}

}  // namespace

// dtfill_line_subsample: tiles of LS_TILE pixels per frame, split evenly over at most LS_MAXNB blocks per frame
struct LinesGrid {
    int tpb, nb;  // tiles per block, blocks per frame
};
inline LinesGrid lines_grid(int H, int W) {
    const int T = (int)(((long long)H * W + LS_TILE - 1) / LS_TILE);
    const int tpb = (T + LS_MAXNB - 1) / LS_MAXNB;
    return LinesGrid{tpb, (T + tpb - 1) / tpb};
}

namespace {
// dtfill_demo_multi_channel: out_1, then one launch per step (raws: the two workspace frames the raw steps alternate between)
template <int FORM>
void gmcv_launch(const float *lidar, const float *rgb, int C, int B, int H, int W, int ts, int scale_num, float sr,
                        float *const *outs, float *const *raws, hipStream_t st) {
    const size_t n = (size_t)B * H * W;
    const int tx = (W + GM_TW - 1) / GM_TW, ty = (H + GM_TH - 1) / GM_TH;
    const u32 ntiles = (u32)((size_t)tx * ty * B);  // (< 2^31: a tile holds a pixel)
    const u32 grid = min(ntiles, 1u << 22);
    k_gmcv_first<FORM><<<(unsigned)min((n + 255) / 256, (size_t)1 << 16), 256, 0, st>>>(lidar, rgb, C, n, sr, outs[0]);
    const float *src = lidar;
    for (int k = 1; k < scale_num; ++k) {
        float *raw = k + 1 < scale_num ? raws[(k - 1) & 1] : nullptr;  // stored only if a later step reads it
        if (ts == 7)
            k_gmcv7<FORM><<<grid, 256, 0, st>>>(src, rgb, C, H, W, tx, ty, ntiles, sr, raw, outs[k]);
        else
            k_gmcv<FORM><<<grid, 256, 0, st>>>(src, rgb, C, H, W, ts, tx, ty, ntiles, sr, raw, outs[k]);
        src = raw;
    }
}

// The workspace of dtfill_nearest_gather (nacc = 0: with spix) and of its backward (nacc = min(C, NG_CH) sets of accumulators),
// 256-byte aligned pieces; with ws = nullptr only the total is worked out.
NgWs ng_carve(void *ws, int B, int H, int W, int nacc, size_t *total) {
    const size_t N = (size_t)B * H * W, Wd = (size_t)(W + 63) / 64, NR = (size_t)B * H;
    char *base = static_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *r = base ? base + off : nullptr;
        off += align256(bytes);
        return r;
    };
    NgWs c{};
    c.Wd = (int)Wd;
    c.N = N;
    if (nacc) {
        c.tsum = (long long *)take(nacc * N * 8);
        c.ebias = (u32 *)take(nacc * N * 4);
        c.flags = (u32 *)take(nacc * N * 4);
    } else {
        c.spix = (u32 *)take(N * 4);
    }
    c.srcbits = (u64 *)take(NR * Wd * 8);
    c.rowcnt = (u32 *)take(NR * 4);
    c.rowbase = (u32 *)take(NR * 4);
    c.nsrc = (u32 *)take((size_t)B * 4);
    c.status = (int32_t *)take((size_t)B * 4);
    if (total) *total = off;
    return c;
}

template <int PX>
void ng_launch_gather(dim3 grid, hipStream_t st, const int32_t *index, const u32 *values, int C, size_t HW, const NgWs &ws,
                             u32 *out_values, int32_t *out_pixel, int32_t *status) {
    if (out_values && out_pixel)
        k_ng_gather<PX, true, true><<<grid, 256, 0, st>>>(index, values, C, HW, ws, out_values, out_pixel, status);
    else if (out_pixel)
        k_ng_gather<PX, true, false><<<grid, 256, 0, st>>>(index, values, C, HW, ws, out_values, out_pixel, status);
    else
        k_ng_gather<PX, false, true><<<grid, 256, 0, st>>>(index, values, C, HW, ws, out_values, out_pixel, status);
}

// One round of the backward: NC channels from channel c0 on.
template <int NC>
void ngb_round(hipStream_t st, const int32_t *index, const float *grad_out, float *grad_values, int C, int c0, int B, int H,
                      int W, const NgWs &ws, int32_t *status) {
    const size_t HW = (size_t)H * W, cp = (size_t)C * HW;
    const int sx = (W + 63) / 64, nstrips = sx * ((H + FB_TH - 1) / FB_TH);
    const dim3 strips((nstrips + 3) / 4, B), rows((H + 3) / 4, B);
    const float *g = grad_out + (size_t)c0 * HW;
    k_ngb_acc<0, NC><<<strips, 256, 0, st>>>(index, g, cp, H, W, sx, nstrips, c0 == 0, ws, status);
    k_ngb_acc<1, NC><<<strips, 256, 0, st>>>(index, g, cp, H, W, sx, nstrips, false, ws, status);
    k_ngb_out<NC><<<rows, 256, 0, st>>>(H, W, cp, c0 + NC < C, ws, grad_values + (size_t)c0 * HW);
}
}  // namespace

extern "C" {

int dtfill_abi_version(void) { return DTFILL_ABI_VERSION; }

const char *dtfill_strerror(int code) {
    switch (code) {
        case DTFILL_OK: return "ok";
        case DTFILL_ERR_NULL: return "null input, workspace, or no output requested";
        case DTFILL_ERR_SHAPE: return "bad shape: need 1 <= B <= 65535, H,W >= 1, H+W-2 < 8192 and B*H*W < 2^31";
        case DTFILL_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
        case DTFILL_ERR_METRIC: return "unknown metric";
        case DTFILL_ERR_LAUNCH: return "HIP kernel launch failed";
        case DTFILL_ERR_NO_DEVICE: return "no usable HIP device";
        default: return "unknown dtfill error code";
    }
}

size_t dtfill_workspace_bytes(int B, int H, int W, int metric) {
    if (!shape_ok(B, H, W)) return 0;
    if (metric != DTFILL_METRIC_L1_CV && metric != DTFILL_METRIC_L2) return 0;
    size_t total = 0;
    carve(nullptr, B, H, W, &total);
    return total;
}

int dtfill_batch_flags(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                       float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                       void *workspace, size_t ws_bytes, void *stream, unsigned flags) {
    int rc = check_args(x, B, H, W, metric, out_depth, out_dt, out_index, workspace, ws_bytes, flags);
    if (rc != DTFILL_OK) return rc;
    return run(make_pass(x, B, H, W, src_thr, val_thr, out_depth, out_dt, out_index, frame_status, workspace), metric, flags, stream,
               nullptr);
}

int dtfill_batch(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                 float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                 void *workspace, size_t ws_bytes, void *stream) {
    return dtfill_batch_flags(x, B, H, W, src_thr, val_thr, metric, out_depth, out_dt, out_index,
                              frame_status, workspace, ws_bytes, stream, 0u);
}

int dtfill_batch_epilogue(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                          float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                          void *workspace, size_t ws_bytes, void *stream, unsigned flags, int depth_row0, int use_floor,
                          float floor_) {
    int rc = check_args(x, B, H, W, metric, out_depth, out_dt, out_index, workspace, ws_bytes, flags);
    if (rc != DTFILL_OK) return rc;
    if (depth_row0 < 0 || depth_row0 >= H) return DTFILL_ERR_SHAPE;
    if (metric != DTFILL_METRIC_L1_CV) return (depth_row0 || use_floor) ? DTFILL_ERR_METRIC : dtfill_batch_flags(x, B, H, W, src_thr, val_thr, metric, out_depth, out_dt, out_index, frame_status, workspace, ws_bytes, stream, flags);
    return run(make_pass(x, B, H, W, src_thr, val_thr, out_depth, out_dt, out_index, frame_status, workspace,
                         DepthEpilogue{depth_row0, use_floor ? 1 : 0, floor_}),
               metric, flags, stream, nullptr);
}

int dtfill_outlier_removal(const float *x, int B, int H, int W, float *out, void *stream) {
    if (!x || !out) return DTFILL_ERR_NULL;
    if (B < 1 || H < 4 || W < 4 || (long long)B * H * W >= (1ll << 31) || B > 65535) return DTFILL_ERR_SHAPE;
    k_outlier<<<dim3((W + O_TW - 1) / O_TW, (H + O_TH - 1) / O_TH, B), 256, 0, static_cast<hipStream_t>(stream)>>>(
        x, H, W, out);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_generate_multi_channel(const float *data, const float *mask, int B, int H, int W, int table_size,
                                  int scale_num, float *out2, float *out3, float *out4, void *stream) {
    if (!data || !mask) return DTFILL_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31) || B > 65535) return DTFILL_ERR_SHAPE;
    if (table_size < 1 || (table_size & 1) == 0 || (table_size - 1) / 2 > GM_MAXHALF || scale_num < 1 || scale_num > 4)
        return DTFILL_ERR_SHAPE;
    float *outs[3] = {out2, out3, out4};
    for (int k = 0; k < scale_num - 1; ++k)
        if (!outs[k]) return DTFILL_ERR_NULL;
    const int half = (table_size - 1) / 2;
    const size_t lds = (size_t)2 * (GM_TH + 2 * half) * (GM_TW + 2 * half) * sizeof(float);
    const dim3 grid((W + GM_TW - 1) / GM_TW, (H + GM_TH - 1) / GM_TH, B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float *src = data, *msk = mask;
    for (int k = 0; k < scale_num - 1; ++k) {
        // (table size 7: a step also writes the later steps' values of the pixels that will pass their masks)
        float *n1 = k + 1 < scale_num - 1 ? outs[k + 1] : nullptr, *n2 = k + 2 < scale_num - 1 ? outs[k + 2] : nullptr;
        if (table_size == 7 && msk)
            k_gmc7<false><<<grid, 256, 0, st>>>(src, msk, H, W, outs[k], n1, n2);
        else if (table_size == 7)
            k_gmc7<true><<<grid, 256, 0, st>>>(src, nullptr, H, W, outs[k], n1, n2);
        else
            k_gmc<<<grid, 256, lds, st>>>(src, msk, H, W, table_size, outs[k]);
        src = outs[k];
        msk = nullptr;  // the next step's mask is (previous output > 0.001)
    }
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// B * H * W * ch < 2^31 for positive arguments, by division: the product itself may not fit 64 bits
static bool gmcv_count_ok(int B, int H, int W, int ch) {
    return B >= 1 && H >= 1 && W >= 1 && ch >= 1 && B <= 0x7fffffff / H / W / ch;
}

size_t dtfill_demo_multi_channel_workspace_bytes(int B, int H, int W, int scale_num) {
    if (!gmcv_count_ok(B, H, W, 1) || scale_num < 1 || scale_num > 4) return 0;
    // raw_k for the steps a later step reads (k = 2 .. scale_num - 1), at most two frames alive at a time
    return (size_t)min(2, max(0, scale_num - 2)) * align256((size_t)B * H * W * sizeof(float));
}

int dtfill_demo_multi_channel(const float *lidar, const float *rgb, int C, int B, int H, int W, int table_size, int scale_num,
                              float scale_range, float *out1, float *out2, float *out3, float *out4, void *workspace,
                              size_t ws_bytes, void *stream) {
    if (!lidar) return DTFILL_ERR_NULL;
    if (table_size < 1 || (table_size & 1) == 0 || (table_size - 1) / 2 > GM_MAXHALF || scale_num < 1 || scale_num > 4)
        return DTFILL_ERR_SHAPE;
    if (!(scale_range != 0.0f) || !isfinite(scale_range) || (rgb && C < 1) || B < 1 || H < 1 || W < 1) return DTFILL_ERR_SHAPE;
    if (!rgb) C = 0;
    if (C >= 0x7fffffff || !gmcv_count_ok(B, H, W, C + 1)) return DTFILL_ERR_SHAPE;
    float *outs[4] = {out1, out2, out3, out4};
    for (int k = 0; k < scale_num; ++k)
        if (!outs[k]) return DTFILL_ERR_NULL;
    const size_t need = dtfill_demo_multi_channel_workspace_bytes(B, H, W, scale_num);
    if (need && !workspace) return DTFILL_ERR_NULL;
    if (need && (ws_bytes < need || ((uintptr_t)workspace & 255))) return DTFILL_ERR_WORKSPACE;
    float *raws[2] = {nullptr, nullptr};  // raw_2 and raw_3, where a later step reads them
    if (need) raws[0] = static_cast<float *>(workspace);
    if (scale_num == 4) raws[1] = reinterpret_cast<float *>(static_cast<char *>(workspace) + need / 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool al16 = true;  // the one-store pixel of the three-channel image form needs 16-byte aligned outputs
    for (int k = 0; k < scale_num; ++k) al16 &= ((uintptr_t)outs[k] & 15) == 0;
    if (!rgb)
        gmcv_launch<GV_PLAIN>(lidar, nullptr, 0, B, H, W, table_size, scale_num, scale_range, outs, raws, st);
    else if (C == 3 && al16)
        gmcv_launch<GV_RGB3>(lidar, rgb, C, B, H, W, table_size, scale_num, scale_range, outs, raws, st);
    else
        gmcv_launch<GV_RGBC>(lidar, rgb, C, B, H, W, table_size, scale_num, scale_range, outs, raws, st);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_generate_multi_channel_backward_workspace_bytes(int B, int H, int W, int scale_num) {
    if (!gmcv_count_ok(B, H, W, 1) || scale_num < 1 || scale_num > 4) return 0;
    // G_k for the steps whose transpose feeds another one (k = 2 .. scale_num - 1)
    return (size_t)min(2, max(0, scale_num - 2)) * align256((size_t)B * H * W * sizeof(float));
}

int dtfill_generate_multi_channel_backward(const float *mask, const float *out2, const float *out3, int B, int H, int W,
                                           int table_size, int scale_num, const float *g1, const float *g2, const float *g3,
                                           const float *g4, float *grad_data, void *workspace, size_t ws_bytes, void *stream) {
    if (!mask || !grad_data) return DTFILL_ERR_NULL;
    if (table_size < 1 || (table_size & 1) == 0 || (table_size - 1) / 2 > GM_MAXHALF || scale_num < 1 || scale_num > 4)
        return DTFILL_ERR_SHAPE;
    if (!gmcv_count_ok(B, H, W, 1)) return DTFILL_ERR_SHAPE;
    if ((scale_num >= 3 && !out2) || (scale_num == 4 && !out3)) return DTFILL_ERR_NULL;
    const size_t need = dtfill_generate_multi_channel_backward_workspace_bytes(B, H, W, scale_num);
    if (need && !workspace) return DTFILL_ERR_NULL;
    if (need && (ws_bytes < need || ((uintptr_t)workspace & 255))) return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * H * W;
    const float *gs[4] = {g1, g2, g3, g4}, *fwds[3] = {nullptr, out2, out3};
    const int half = (table_size - 1) / 2;
    const size_t lds = ((size_t)2 * (GM_TH + 2 * half) * (GM_TW + 2 * half) + (size_t)(GM_TH + 4 * half) * (GM_TW + 4 * half)) * sizeof(float);
    const int tx = (W + GM_TW - 1) / GM_TW, ty = (H + GM_TH - 1) / GM_TH;
    const u32 ntiles = (u32)((size_t)tx * ty * B);  // (< 2^31: a tile holds a pixel)
    const u32 grid = min(ntiles, 1u << 22);
    // G_k = g_k + A_k^T G_(k+1), from the last step down; `up` is G_(k+1), NULL while it is all zero.  A zero G_(k+1) makes
    // the transpose sum +0 everywhere, so G_k = g_k + (+0): g_k itself but for its -0.0, which no later sum can tell from
    // +0.0 (a window's c_p enters only an addition to a sum that started from +0).  Such a step is not launched: the next
    // one reads g_k in place of G_k.  Only grad_data itself is written as g_1 + (+0).
    const float *up = gs[scale_num - 1];
    int frames = 0;
    for (int k = scale_num - 1; k >= 1; --k) {
        if (!up) {
            up = gs[k - 1];
            continue;
        }
        float *dst = k == 1 ? grad_data : reinterpret_cast<float *>(static_cast<char *>(workspace) + (size_t)(frames++ & 1) * (need / 2));
        const float *msk = k == 1 ? mask : nullptr;
        if (table_size == 7)
            k_gmcb<7><<<grid, 256, lds, st>>>(msk, fwds[k - 1], up, gs[k - 1], H, W, 7, tx, ty, ntiles, dst);
        else
            k_gmcb<0><<<grid, 256, lds, st>>>(msk, fwds[k - 1], up, gs[k - 1], H, W, table_size, tx, ty, ntiles, dst);
        up = dst;
    }
    if (up != grad_data)  // no step stored it: scale_num 1 (g_1 as it is), or every later gradient NULL (g_1 + (+0))
        k_gmcb_first<<<(unsigned)min((n + 255) / 256, (size_t)1 << 16), 256, 0, st>>>(up, n, scale_num > 1, grad_data);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// the checks the two loss entry points share; whether every pointer and the count allow the 16-byte loads
static int loss_check(const float *pred, const float *corr, const float *gt, const float *lidar, int B, int H, int W, int kind,
                      int r0, int r1, int c0, int c1) {
    if (!pred || !gt || (corr && !lidar)) return DTFILL_ERR_NULL;
    if (!gmcv_count_ok(B, H, W, 1)) return DTFILL_ERR_SHAPE;
    if (r0 < 0 || r1 > H || r0 >= r1 || c0 < 0 || c1 > W || c0 >= c1) return DTFILL_ERR_SHAPE;
    if (kind != DTFILL_LOSS_KITTI && kind != DTFILL_LOSS_NYU) return DTFILL_ERR_METRIC;
    return DTFILL_OK;
}
static bool loss_vec(size_t n, std::initializer_list<const void *> ptrs) {
    uintptr_t bits = (uintptr_t)(n & 3);
    for (const void *p : ptrs) bits |= (uintptr_t)p & 15;
    return bits == 0;
}

size_t dtfill_train_loss_workspace_bytes(int B, int H, int W) {
    if (!gmcv_count_ok(B, H, W, 1)) return 0;
    const size_t nb = (size_t)loss_blocks((size_t)B * H * W);
    return align256(nb * 2 * sizeof(double)) + align256(nb * 2 * sizeof(u32));
}

int dtfill_train_loss(const float *pred, const float *corr, const float *gt, const float *lidar, int B, int H, int W, int kind,
                      float gt_thr, float in_thr, int r0, int r1, int c0, int c1, double *stats, void *workspace,
                      size_t ws_bytes, void *stream) {
    if (!stats || !workspace) return DTFILL_ERR_NULL;
    const int rc = loss_check(pred, corr, gt, lidar, B, H, W, kind, r0, r1, c0, c1);
    if (rc != DTFILL_OK) return rc;
    if (ws_bytes < dtfill_train_loss_workspace_bytes(B, H, W) || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    const size_t n = (size_t)B * H * W;
    const int nb = loss_blocks(n);
    double *part_s = static_cast<double *>(workspace);
    u32 *part_n = reinterpret_cast<u32 *>(static_cast<char *>(workspace) + align256((size_t)nb * 2 * sizeof(double)));
    const LossWindow w{H, W, r0, r1, c0, c1};
    const bool win = r0 != 0 || r1 != H || c0 != 0 || c1 != W;
    const bool vec = loss_vec(n, {pred, corr, gt, corr ? lidar : nullptr});
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (aux, win, vec) -> the instantiation; lidar is not passed on without corr, so it is never read
    auto launch = [&](auto a, auto wn, auto v) {
        k_loss_part<decltype(a)::value, decltype(wn)::value, decltype(v)::value><<<nb, 256, 0, st>>>(
            pred, corr, gt, corr ? lidar : nullptr, n, w, gt_thr, in_thr, part_s, part_n);
    };
    auto pick_v = [&](auto a, auto wn) { vec ? launch(a, wn, std::true_type{}) : launch(a, wn, std::false_type{}); };
    auto pick_w = [&](auto a) { win ? pick_v(a, std::true_type{}) : pick_v(a, std::false_type{}); };
    corr ? pick_w(std::true_type{}) : pick_w(std::false_type{});
    k_loss_final<<<1, 64, 0, st>>>(part_s, part_n, nb, kind, corr ? 1 : 0, stats);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_train_loss_backward(const float *pred, const float *corr, const float *gt, const float *lidar, int B, int H, int W,
                               int kind, float gt_thr, float in_thr, int r0, int r1, int c0, int c1, const double *stats,
                               const float *g_main, const float *g_aux, float *grad_pred, float *grad_corr, void *stream) {
    if (!stats || (!grad_pred && !grad_corr) || (grad_corr && !corr)) return DTFILL_ERR_NULL;
    const int rc = loss_check(pred, corr, gt, lidar, B, H, W, kind, r0, r1, c0, c1);
    if (rc != DTFILL_OK) return rc;
    const size_t n = (size_t)B * H * W;
    const LossWindow w{H, W, r0, r1, c0, c1};
    const bool win = r0 != 0 || r1 != H || c0 != 0 || c1 != W;
    const bool vec = loss_vec(n, {pred, corr, gt, corr ? lidar : nullptr, grad_pred, grad_corr});
    const unsigned grid = (unsigned)min((n + L_CHUNK - 1) / L_CHUNK, (size_t)L_BWD_MAXB);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto wn, auto v) {
        k_loss_bwd<decltype(wn)::value, decltype(v)::value><<<grid, 256, 0, st>>>(
            pred, corr, gt, corr ? lidar : nullptr, n, w, kind, gt_thr, in_thr, stats, g_main, g_aux, grad_pred, grad_corr);
    };
    auto pick_v = [&](auto wn) { vec ? launch(wn, std::true_type{}) : launch(wn, std::false_type{}); };
    win ? pick_v(std::true_type{}) : pick_v(std::false_type{});
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_num_kernels(int metric) {
    return metric == DTFILL_METRIC_L1_CV ? NK_L1 : metric == DTFILL_METRIC_L2 ? NK_L2 : 0;
}

const char *dtfill_kernel_name(int metric, int k) {
    if (metric == DTFILL_METRIC_L1_CV && k >= 0 && k < NK_L1) return kNamesL1[k];
    if (metric == DTFILL_METRIC_L2 && k >= 0 && k < NK_L2) return kNamesL2[k];
    return "";
}

int dtfill_batch_timed(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                       float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                       void *workspace, size_t ws_bytes, void *stream, unsigned flags, float *kernel_ms) {
    int rc = check_args(x, B, H, W, metric, out_depth, out_dt, out_index, workspace, ws_bytes, flags);
    if (rc != DTFILL_OK) return rc;
    if (!kernel_ms) return DTFILL_ERR_NULL;
    const int nk = dtfill_num_kernels(metric);
    static_assert(NK_L2 <= NK_L1, "event array");
    hipEvent_t ev[NK_L1 + 1];
    for (int k = 0; k <= nk; ++k)
        if (hipEventCreate(&ev[k]) != hipSuccess) {
            while (k-- > 0) (void)hipEventDestroy(ev[k]);  // nothing created so far is left behind
            return DTFILL_ERR_NO_DEVICE;
        }
    unsigned idle = 0;
    rc = run(make_pass(x, B, H, W, src_thr, val_thr, out_depth, out_dt, out_index, frame_status, workspace), metric, flags, stream, ev, &idle);
    (void)hipEventSynchronize(ev[nk]);
    for (int k = 0; k < nk; ++k) {
        (void)hipEventElapsedTime(&kernel_ms[k], ev[k], ev[k + 1]);
        if (idle >> k & 1u) kernel_ms[k] = 0.0f;  // (two events back to back are still some microseconds apart)
    }
    for (int k = 0; k <= nk; ++k) (void)hipEventDestroy(ev[k]);
    return rc;
}

int dtfill_pass_stats(const void *workspace, size_t ws_bytes, int B, int H, int W, int metric, long long *out_px, void *stream) {
    if (!workspace || !out_px) return DTFILL_ERR_NULL;
    if (!shape_ok(B, H, W)) return DTFILL_ERR_SHAPE;
    if (metric != DTFILL_METRIC_L1_CV && metric != DTFILL_METRIC_L2) return DTFILL_ERR_METRIC;
    if (ws_bytes < dtfill_workspace_bytes(B, H, W, metric) || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out_px, 0, DTFILL_STATS_N * sizeof(long long), st) != hipSuccess) return DTFILL_ERR_LAUNCH;
    k_stats<<<B, 256, 0, st>>>(carve(const_cast<void *>(workspace), B, H, W), metric == DTFILL_METRIC_L2 ? 1 : 0, out_px);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_crop_floor(const float *x, int B, int H, int W, int r0, int r1, int c0, int c1, int use_floor, float floor_,
                      float *out, void *stream) {
    if (!x || !out) return DTFILL_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31) || B > 65535 || H > 65535) return DTFILL_ERR_SHAPE;
    if (r0 < 0 || r1 > H || r0 >= r1 || c0 < 0 || c1 > W || c0 >= c1) return DTFILL_ERR_SHAPE;
    const int OH = r1 - r0, OW = c1 - c0;
    k_crop_floor<<<dim3(min((OW + 255) / 256, 8), OH, B), 256, 0, static_cast<hipStream_t>(stream)>>>(
        x, H, W, r0, c0, OH, OW, use_floor, floor_, out);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_png16(const float *x, int B, int H, int W, int pad_top, int use_floor, float floor_, float lo, float hi,
                 float scale, uint16_t *out, void *stream) {
    if (!x || !out) return DTFILL_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || pad_top < 0 || (long long)B * ((long long)H + pad_top) * W >= (1ll << 31) || B > 65535 ||
        H + pad_top > 65535)
        return DTFILL_ERR_SHAPE;
    k_png16<<<dim3(min((W + 255) / 256, 8), H + pad_top, B), 256, 0, static_cast<hipStream_t>(stream)>>>(
        x, H, W, pad_top, use_floor, floor_, lo, hi, scale, out);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_line_subsample_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return align256((size_t)B * LS_REC * sizeof(double)) + align256((size_t)B * lines_grid(H, W).nb * sizeof(double2));
}

int dtfill_line_subsample(const float *x, int B, int H, int W, const double *K, const double *E, int n_bins, int keep_every,
                          float *out, int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream) {
    if (!x || !K || !E || !out || !frame_status || !workspace || n_bins < 1 || keep_every < 1) return DTFILL_ERR_NULL;
    const size_t need = dtfill_line_subsample_workspace_bytes(B, H, W);
    if (need == 0) return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    const LinesGrid g = lines_grid(H, W);
    const int HW = H * W;
    double *rec = static_cast<double *>(workspace);
    double2 *part = reinterpret_cast<double2 *>(static_cast<char *>(workspace) + align256((size_t)B * LS_REC * sizeof(double)));
    const bool vec = (HW & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid(g.nb, B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_lines_calib<<<B, 64, 0, st>>>(K, E, rec);
    if (vec) {
        k_lines_range<true><<<grid, 256, 0, st>>>(x, 0.1f, W, HW, g.tpb, rec, part);
        k_lines_keep<true><<<grid, 256, 0, st>>>(x, W, HW, n_bins, keep_every, g.tpb, rec, part, out, frame_status);
    } else {
        k_lines_range<false><<<grid, 256, 0, st>>>(x, 0.1f, W, HW, g.tpb, rec, part);
        k_lines_keep<false><<<grid, 256, 0, st>>>(x, W, HW, n_bins, keep_every, g.tpb, rec, part, out, frame_status);
    }
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_depth_read_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return align256((size_t)B * H * sizeof(int)) + align256((size_t)B * W * sizeof(int)) + align256((size_t)B * sizeof(u32));
}

int dtfill_depth_read(const uint16_t *raw, const int32_t *dims, int B, int hmax, int wmax, int H, int W, float *out,
                      int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream) {
    if (!raw || !out || !workspace) return DTFILL_ERR_NULL;
    const size_t need = dtfill_depth_read_workspace_bytes(B, H, W);
    if (need == 0 || hmax < 1 || wmax < 1 || (long long)B * hmax * wmax >= (1ll << 31)) return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    char *base = static_cast<char *>(workspace);
    int *ry = reinterpret_cast<int *>(base);
    int *rx = reinterpret_cast<int *>(base + align256((size_t)B * H * sizeof(int)));
    u32 *fw = reinterpret_cast<u32 *>(base + align256((size_t)B * H * sizeof(int)) + align256((size_t)B * W * sizeof(int)));
    const int rpb = max(DR_ROWS, (H + 65534) / 65535);
    const dim3 grid(B, (H + rpb - 1) / rpb);
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_read_maps<<<B, 128, 0, st>>>(dims, hmax, wmax, H, W, ry, rx, fw);
    if ((W & 3) == 0 && ((uintptr_t)out & 15) == 0)
        k_read_gather<true><<<grid, DR_THREADS, 0, st>>>(raw, dims, hmax, wmax, H, W, rpb, ry, rx, fw, out, frame_status);
    else
        k_read_gather<false><<<grid, DR_THREADS, 0, st>>>(raw, dims, hmax, wmax, H, W, rpb, ry, rx, fw, out, frame_status);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_rgb_read_workspace_bytes(int B, int H, int W) { return dtfill_depth_read_workspace_bytes(B, H, W); }

int dtfill_rgb_read(const uint8_t *raw, const int32_t *dims, int B, int hmax, int wmax, int C, int H, int W, int first_row,
                    int normalize, int layout, uint8_t *out_u8, float *out_f32, int32_t *frame_status, void *workspace,
                    size_t ws_bytes, void *stream) {
    if (!raw || !workspace || (!out_u8 && !out_f32)) return DTFILL_ERR_NULL;
    const size_t need = dtfill_rgb_read_workspace_bytes(B, H, W);
    if (need == 0 || hmax < 1 || wmax < 1 || C < 1 || C > 4 || first_row < 0 || first_row >= H ||
        (layout != DTFILL_RGB_NHWC && layout != DTFILL_RGB_NCHW))
        return DTFILL_ERR_SHAPE;
    const long long OH = H - first_row;
    if ((long long)hmax * wmax >= (1ll << 31) || (long long)B * hmax * wmax * C >= (1ll << 31) || B * OH * W * C >= (1ll << 31))
        return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    char *base = static_cast<char *>(workspace);
    int *ry = reinterpret_cast<int *>(base);
    int *rx = reinterpret_cast<int *>(base + align256((size_t)B * H * sizeof(int)));
    u32 *fw = reinterpret_cast<u32 *>(base + align256((size_t)B * H * sizeof(int)) + align256((size_t)B * W * sizeof(int)));
    const int rpb = max(RG_ROWS, (int)((OH + 65534) / 65535));
    const dim3 grid(B, (unsigned)((OH + rpb - 1) / rpb));
    const RgArgs a{raw, dims, hmax, wmax, H, W, first_row, rpb, normalize, layout, ry, rx, out_u8, out_f32, frame_status};
    // the LDS image holds a whole source row: rows that fit it, unless most of their bytes would go unsampled
#ifdef RGB_NO_STAGE  // the A/B build of scripts/bench_rgb_read.py: every pick from global memory
    const bool stage = false;
#else
    const bool stage = (long long)wmax * C <= RG_SPAN && wmax <= 2ll * W;
#endif
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_read_maps<<<B, 128, 0, st>>>(dims, hmax, wmax, H, W, ry, rx, fw);
    switch (C) {
        case 1: rgb_launch<1>(grid, st, stage, a); break;
        case 2: rgb_launch<2>(grid, st, stage, a); break;
        case 3: rgb_launch<3>(grid, st, stage, a); break;
        default: rgb_launch<4>(grid, st, stage, a); break;
    }
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_nyu_read_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return align256((size_t)B * (((size_t)H * W + 31) / 32) * sizeof(u32));  // one bit per output pixel
}

int dtfill_nyu_read(const uint8_t *rgb, const float *depth, int B, int C, int hin, int win, int H, int W, const double *wy,
                    int ry, const double *wx, int rx, const int32_t *samples, int n, int normalize, int layout,
                    float *out_rgb, float *out_gt, float *out_lidar, int32_t *frame_status, void *workspace, size_t ws_bytes,
                    void *stream) {
    if ((!rgb && !depth) || !workspace || !rgb != !out_rgb || (!depth && (out_gt || out_lidar)) ||
        (depth && !out_gt && !out_lidar))
        return DTFILL_ERR_NULL;
    const size_t need = dtfill_nyu_read_workspace_bytes(B, H, W);
    if (need == 0 || hin < 1 || win < 1 || H > hin || W > win || ry < 0 || ry > DTFILL_NYU_MAX_RADIUS || rx < 0 ||
        rx > DTFILL_NYU_MAX_RADIUS || !wy != (ry == 0) || !wx != (rx == 0) || n < 0 ||
        (rgb && (C < 1 || C > 4 || (layout != DTFILL_RGB_NHWC && layout != DTFILL_RGB_NCHW))))
        return DTFILL_ERR_SHAPE;
    const long long lim = 1ll << 31, src = (long long)B * hin * win;  // (hin * win <= src: B * H * W < 2^31 bounds neither)
    if ((long long)hin * win >= lim || src >= lim || (rgb && (src * C >= lim || (long long)B * H * W * C >= lim)) ||
        (long long)B * n * 2 >= lim)
        return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    NyArgs a{};
    a.y.f = (double)hin / H;
    a.x.f = (double)win / W;
    a.y.n_in = hin, a.y.n_out = H, a.y.r = ry;
    a.x.n_in = win, a.x.n_out = W, a.x.r = rx;
    for (int k = 0; k <= ry && wy; ++k) a.y.w[k] = wy[k];
    for (int k = 0; k <= rx && wx; ++k) a.x.w[k] = wx[k];
    a.normalize = normalize, a.layout = layout;
    a.words = ((size_t)H * W + 31) / 32;
    a.out_rgb = out_rgb, a.out_gt = out_gt, a.out_lidar = out_lidar;
    hipStream_t st = static_cast<hipStream_t>(stream);
    u32 *mask = samples && n > 0 ? static_cast<u32 *>(workspace) : nullptr;
    const size_t nclear = mask ? (size_t)B * a.words : (size_t)B;
    if (mask || frame_status)
        k_nyu_clear<<<(unsigned)((nclear + 255) / 256), 256, 0, st>>>(mask, mask ? nclear : 0, frame_status, B);
    if (mask)
        k_nyu_mark<<<(unsigned)(((size_t)B * n + 255) / 256), 256, 0, st>>>(samples, B, n, H, W, a.words, mask, frame_status);
    if (rgb) {
        a.src = rgb, a.C = C, a.mask = nullptr;
        nyu_launch<u8>(st, a, B);
    }
    if (depth) {
        a.src = depth, a.C = 1, a.mask = mask;
        nyu_launch<float>(st, a, B);
    }
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_project_points_workspace_bytes(int B, int N, int H, int W) {
    if (B < 1 || B > 65535 || N < 1 || H < 1 || W < 1 || (long long)B * N * 3 >= (1ll << 31) ||
        (long long)B * H * W >= (1ll << 31))  // (stride 3: the call checks its own)
        return 0;
    return align256((size_t)B * H * W * sizeof(u64)) + align256((size_t)B * PJ_ACC * sizeof(int));
}

int dtfill_project_points(const float *points, const int32_t *counts, int B, int N, int stride, int H, int W, const double *K,
                          const double *E, int mode, float min_z, float *out_f32, double *out_f64, int32_t *frame_status,
                          int32_t *frame_counts, void *workspace, size_t ws_bytes, void *stream) {
    if (!points || !K || !E || !workspace || (!out_f32 && !out_f64)) return DTFILL_ERR_NULL;
    const size_t need = dtfill_project_points_workspace_bytes(B, N, H, W);
    if (need == 0 || (stride != 3 && stride != 4) || (long long)B * N * stride >= (1ll << 31) ||
        (mode != DTFILL_PROJ_REFERENCE && mode != DTFILL_PROJ_ZBUFFER))
        return DTFILL_ERR_SHAPE;
    if (mode == DTFILL_PROJ_ZBUFFER && !(min_z >= 0.0f && min_z < __builtin_inff())) return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    int *acc = reinterpret_cast<int *>(static_cast<char *>(workspace) + align256((size_t)B * H * W * sizeof(u64)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == DTFILL_PROJ_REFERENCE)
        proj_launch<DTFILL_PROJ_REFERENCE>(st, points, counts, B, N, stride, H, W, K, E, min_z, out_f32, out_f64, frame_status,
                                           frame_counts, workspace, acc);
    else
        proj_launch<DTFILL_PROJ_ZBUFFER>(st, points, counts, B, N, stride, H, W, K, E, min_z, out_f32, out_f64, frame_status,
                                         frame_counts, workspace, acc);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_unproject_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return align256((size_t)B * LS_REC * sizeof(double)) + align256((size_t)B * lines_grid(H, W).nb * sizeof(double2)) +
           align256((size_t)B * up_tiles(H, W) * sizeof(int));
}

int dtfill_unproject(const float *x, const float *payload, int B, int H, int W, float val_thr, const double *K, const double *E,
                     int n_bins, int keep_every, int N, int stride, float *points, double *pitch, int32_t *pixel,
                     int32_t *counts, int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream) {
    if (!x || !K || !E || !points || !counts || !workspace) return DTFILL_ERR_NULL;
    const size_t need = dtfill_unproject_workspace_bytes(B, H, W);
    if (need == 0 || N < 1 || (stride != 3 && stride != 4) || (long long)B * N * stride >= (1ll << 31) || keep_every < 0 ||
        (keep_every >= 1 && n_bins < 1) || val_thr != val_thr)
        return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    const LinesGrid g = lines_grid(H, W);
    char *base = static_cast<char *>(workspace);
    UpWs ws;
    ws.rec = reinterpret_cast<double *>(base);
    ws.part = reinterpret_cast<double2 *>(base + align256((size_t)B * LS_REC * sizeof(double)));
    ws.tcnt = reinterpret_cast<int *>(base + align256((size_t)B * LS_REC * sizeof(double)) +
                                      align256((size_t)B * g.nb * sizeof(double2)));
    const bool vec = ((H * W) & 3) == 0 && ((uintptr_t)x & 15) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define DTFILL_UNPROJ_GO(VEC, KEEP)                                                                                              \
    unproj_launch<VEC, KEEP>(st, x, payload, B, H, W, val_thr, K, E, n_bins, keep_every, N, stride, points, pitch, pixel, counts, \
                             frame_status, ws, g.tpb, g.nb)
    if (keep_every >= 1) {
        if (vec) DTFILL_UNPROJ_GO(true, true); else DTFILL_UNPROJ_GO(false, true);
    } else {
        if (vec) DTFILL_UNPROJ_GO(true, false); else DTFILL_UNPROJ_GO(false, false);
    }
#undef DTFILL_UNPROJ_GO
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_unproject_backward_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return align256((size_t)B * LS_REC * sizeof(double)) + align256((size_t)B * sizeof(int));
}

int dtfill_unproject_backward(const float *grad_points, const int32_t *pixel, const int32_t *counts, int B, int N, int stride,
                              int H, int W, const double *K, const double *E, float *grad_x, float *grad_payload,
                              int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream) {
    if (!grad_points || !pixel || !counts || !K || !E || !grad_x || !workspace) return DTFILL_ERR_NULL;
    const size_t need = dtfill_unproject_backward_workspace_bytes(B, H, W);
    if (need == 0 || N < 1 || (stride != 3 && stride != 4) || (long long)B * N * stride >= (1ll << 31)) return DTFILL_ERR_SHAPE;
    if (ws_bytes < need || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    double *rec = static_cast<double *>(workspace);
    int *flags = reinterpret_cast<int *>(static_cast<char *>(workspace) + align256((size_t)B * LS_REC * sizeof(double)));
    const int HW = H * W;
    const size_t n = (size_t)B * HW;
    const dim3 recs((N + UB_BLOCK - 1) / UB_BLOCK, B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_lines_calib<<<B, 64, 0, st>>>(K, E, rec);
    k_unprojb_clear<<<(unsigned)min((n + 255) / 256, (size_t)1 << 16), 256, 0, st>>>(grad_x, grad_payload, n, flags, B);
    k_unprojb_check<<<recs, 256, 0, st>>>(pixel, counts, N, HW, flags);
    k_unprojb_scatter<<<recs, 256, 0, st>>>(grad_points, pixel, counts, N, stride, W, HW, rec, flags, grad_x, grad_payload,
                                            frame_status);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_metrics_workspace_bytes(int B) {
    if (B < 1 || B > 65535) return 0;
    return (size_t)B * M_NB * M_NS * sizeof(double);
}

int dtfill_metrics(const float *output, const float *target, int B, long long n, int kind, double *out, void *workspace,
                   size_t ws_bytes, void *stream) {
    if (!output || !target || !out || !workspace) return DTFILL_ERR_NULL;
    if (B < 1 || B > 65535 || n < 1 || n >= (1ll << 40)) return DTFILL_ERR_SHAPE;
    if (kind != DTFILL_METRICS_KITTI && kind != DTFILL_METRICS_NYU) return DTFILL_ERR_METRIC;
    if (ws_bytes < dtfill_metrics_workspace_bytes(B)) return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *part = static_cast<double *>(workspace);
    if (kind == DTFILL_METRICS_KITTI) {
        k_metrics_part<0><<<dim3(M_NB, B), 256, 0, st>>>(output, target, n, part);
        k_metrics_final<0><<<B, 64, 0, st>>>(part, M_NB, out);
    } else {
        k_metrics_part<1><<<dim3(M_NB, B), 256, 0, st>>>(output, target, n, part);
        k_metrics_final<1><<<B, 64, 0, st>>>(part, M_NB, out);
    }
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// The workspace of dtfill_fill_backward, 256-byte aligned pieces; with ws = nullptr only the total is worked out.
static FbWs fb_carve(void *ws, int B, int H, int W, size_t *total) {
    const size_t N = (size_t)B * H * W, Wd = (size_t)(W + 63) / 64, NR = (size_t)B * H;
    char *base = static_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *r = base ? base + off : nullptr;
        off += align256(bytes);
        return r;
    };
    FbWs c{};
    c.Wd = (int)Wd;
    c.tsum = (long long *)take(N * 8);
    c.ebias = (u32 *)take(N * 4);
    c.flags = (u32 *)take(N * 4);
    c.valbits = (u64 *)take(NR * Wd * 8);
    c.rowcnt = (u32 *)take(NR * 4);
    c.rowbase = (u32 *)take(NR * 4);
    c.nval = (u32 *)take((size_t)B * 4);
    c.err = (u32 *)take((size_t)B * 4);
    if (total) *total = off;
    return c;
}

size_t dtfill_fill_backward_workspace_bytes(int B, int H, int W) {
    if (!shape_ok(B, H, W)) return 0;
    size_t total = 0;
    fb_carve(nullptr, B, H, W, &total);
    return total;
}

int dtfill_fill_backward(const float *x, const int32_t *index, const float *grad_depth, int B, int H, int W, float val_thr,
                         float *grad_x, int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream) {
    if (!x || !index || !grad_depth || !grad_x || !workspace) return DTFILL_ERR_NULL;
    if (!shape_ok(B, H, W)) return DTFILL_ERR_SHAPE;
    if (ws_bytes < dtfill_fill_backward_workspace_bytes(B, H, W) || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FbWs ws = fb_carve(workspace, B, H, W, nullptr);
    const size_t HW = (size_t)H * W;
    const dim3 rows((H + 3) / 4, B);
    k_fb_count<<<rows, 256, 0, st>>>(x, H, W, val_thr, ws);
    // blocks that share a frame's clearing: one per 4096 pixels, at most 64
    k_fb_scan<<<dim3((unsigned)min((HW + 4095) / 4096, (size_t)64), B), 256, 0, st>>>(H, HW, ws);
    const int sx = (W + 63) / 64, nstrips = sx * ((H + FB_TH - 1) / FB_TH);
    const dim3 strips((nstrips + 3) / 4, B);
    k_fb_acc<0><<<strips, 256, 0, st>>>(index, grad_depth, H, W, sx, nstrips, ws);
    k_fb_acc<1><<<strips, 256, 0, st>>>(index, grad_depth, H, W, sx, nstrips, ws);
    k_fb_out<<<rows, 256, 0, st>>>(H, W, ws, grad_x, frame_status);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_nearest_gather_workspace_bytes(int B, int H, int W) {
    if (!shape_ok(B, H, W)) return 0;
    size_t total = 0;
    ng_carve(nullptr, B, H, W, 0, &total);
    return total;
}

int dtfill_nearest_gather(const float *x, const int32_t *index, const float *values, int C, int B, int H, int W, float src_thr,
                          float *out_values, int32_t *out_pixel, int32_t *frame_status, void *workspace, size_t ws_bytes,
                          void *stream) {
    if (!x || !index || !workspace || (!out_values && !out_pixel) || (!values != !out_values)) return DTFILL_ERR_NULL;
    if (!shape_ok(B, H, W) || C < 0 || C > DTFILL_NEAR_MAX_C || (C == 0 && values)) return DTFILL_ERR_SHAPE;
    if (ws_bytes < dtfill_nearest_gather_workspace_bytes(B, H, W) || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const NgWs ws = ng_carve(workspace, B, H, W, 0, nullptr);
    int32_t *status = frame_status ? frame_status : ws.status;
    const size_t HW = (size_t)H * W;
    const dim3 rows((H + 3) / 4, B);
    k_ng_count<<<rows, 256, 0, st>>>(x, H, W, src_thr, ws);
    k_ng_scan<0><<<dim3(1, B), 256, 0, st>>>(H, HW, 0, ws, status);
    k_ng_list<<<rows, 256, 0, st>>>(H, W, ws);
    const u32 *vin = reinterpret_cast<const u32 *>(values);  // the payload moves as bits
    u32 *vout = reinterpret_cast<u32 *>(out_values);
    const bool vec = (W & 3) == 0 && (((uintptr_t)index | (uintptr_t)out_values | (uintptr_t)out_pixel) & 15) == 0;
    if (vec)
        ng_launch_gather<4>(dim3((unsigned)((HW / 4 + 255) / 256), B), st, index, vin, C, HW, ws, vout, out_pixel, status);
    else
        ng_launch_gather<1>(dim3((unsigned)((HW + 255) / 256), B), st, index, vin, C, HW, ws, vout, out_pixel, status);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_nearest_gather_backward_workspace_bytes(int B, int H, int W, int C) {
    if (!shape_ok(B, H, W) || C < 1 || C > DTFILL_NEAR_MAX_C) return 0;
    size_t total = 0;
    ng_carve(nullptr, B, H, W, min(C, NG_CH), &total);
    return total;
}

int dtfill_nearest_gather_backward(const float *x, const int32_t *index, const float *grad_out, int C, int B, int H, int W,
                                   float src_thr, float *grad_values, int32_t *frame_status, void *workspace, size_t ws_bytes,
                                   void *stream) {
    if (!x || !index || !grad_out || !grad_values || !workspace) return DTFILL_ERR_NULL;
    if (!shape_ok(B, H, W) || C < 1 || C > DTFILL_NEAR_MAX_C) return DTFILL_ERR_SHAPE;
    if (ws_bytes < dtfill_nearest_gather_backward_workspace_bytes(B, H, W, C) || ((uintptr_t)workspace & 255))
        return DTFILL_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nacc = min(C, NG_CH);
    const NgWs ws = ng_carve(workspace, B, H, W, nacc, nullptr);
    int32_t *status = frame_status ? frame_status : ws.status;
    const size_t HW = (size_t)H * W;
    k_ng_count<<<dim3((H + 3) / 4, B), 256, 0, st>>>(x, H, W, src_thr, ws);
    // blocks that share a frame's clearing: one per 4096 pixels, at most 64
    k_ng_scan<1><<<dim3((unsigned)min((HW + 4095) / 4096, (size_t)64), B), 256, 0, st>>>(H, HW, nacc, ws, status);
    static_assert(NG_CH == 2, "the rounds below are of two channels and, for an odd C, a last one of one");
    int c0 = 0;
    for (; c0 + 2 <= C; c0 += 2) ngb_round<2>(st, index, grad_out, grad_values, C, c0, B, H, W, ws, status);
    if (c0 < C) ngb_round<1>(st, index, grad_out, grad_values, C, c0, B, H, W, ws, status);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// TensorFlow's 'same' rule for one axis: the output extent and the padding in front
static void conv2_same(int n, int ksize, int stride, int *out, int *front) {
    *out = (int)(((long long)n + stride - 1) / stride);
    const long long pad = (long long)(*out - 1) * stride + ksize - n;
    *front = pad > 0 ? (int)(pad / 2) : 0;
}

// what the three convolutions check alike; Ho, Wo: the output frame.  The channel counts an entry point takes are its own rule.
static int conv_check(const float *x, int B, int H, int W, int Cin, const float *w, int Cout, int act, float alpha, const float *out,
                      int out_channels, int out_offset, long long Ho, long long Wo) {
    if (!x || !w || !out) return DTFILL_ERR_NULL;
    if (out_offset < 0 || out_channels < 1 || (long long)out_offset + Cout > out_channels) return DTFILL_ERR_SHAPE;
    if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31) || B * Ho * Wo >= (1ll << 31)) return DTFILL_ERR_SHAPE;
    if ((long long)B * H * W * Cin >= (1ll << 31) || B * Ho * Wo * max(Cout, out_channels) >= (1ll << 31)) return DTFILL_ERR_SHAPE;
    if ((act != DTFILL_CONV_LINEAR && act != DTFILL_CONV_LEAKY) || !isfinite(alpha)) return DTFILL_ERR_SHAPE;
    return DTFILL_OK;
}

// the channel counts of the wide kernels: whole groups in, whole N-tiles out
static bool conv_wide_channels(int Cin, int Cout) { return Cin >= CV_G && Cin % CV_G == 0 && Cout >= 16 && Cout % 16 == 0; }

// the channel counts of the image layer: fewer than a k-step in, whole N-tiles out
static bool conv_image_channels(int Cin, int Cout) { return Cin >= 2 && Cin <= 4 && Cout >= 16 && Cout % 16 == 0; }

int dtfill_conv2d_image(const float *x, int B, int H, int W, int Cin, const float *w, const float *bias, int ksize, int Cout, int act,
                        float alpha, float *out, int out_channels, int out_offset, void *stream) {
    const int rc = conv_check(x, B, H, W, Cin, w, Cout, act, alpha, out, out_channels, out_offset, H, W);
    if (rc != DTFILL_OK) return rc;
    if ((ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7) || !conv_image_channels(Cin, Cout)) return DTFILL_ERR_SHAPE;
    const int r = (ksize - 1) / 2;
    const ConvArgs a{x, w, bias, nullptr, out, B, H, W, Cin, Cout, H, W, r, r, out_channels, out_offset, act, alpha};
    conv_image_launch(static_cast<hipStream_t>(stream), a, ksize);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_conv2d_strided(const float *x, int B, int H, int W, int Cin, const float *w, const float *bias, int ksize, int Cout,
                          int stride, const float *residual, int act, float alpha, float *out, int out_channels, int out_offset,
                          void *stream) {
    if (!x || !w || !out) return DTFILL_ERR_NULL;
    if (stride != 1 && stride != 2) return DTFILL_ERR_SHAPE;
    if (ksize != 1 && ksize != 3 && (stride == 2 || (ksize != 5 && ksize != 7))) return DTFILL_ERR_SHAPE;
    if (H < 1 || W < 1 || !conv_wide_channels(Cin, Cout)) return DTFILL_ERR_SHAPE;
    int Ho, Wo, pt, pl;
    conv2_same(H, ksize, stride, &Ho, &pt);
    conv2_same(W, ksize, stride, &Wo, &pl);
    const int rc = conv_check(x, B, H, W, Cin, w, Cout, act, alpha, out, out_channels, out_offset, Ho, Wo);
    if (rc != DTFILL_OK) return rc;
    const ConvArgs a{x, w, bias, residual, out, B, H, W, Cin, Cout, Ho, Wo, pt, pl, out_channels, out_offset, act, alpha};
    conv_strided_launch(static_cast<hipStream_t>(stream), a, ksize, stride);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_conv2d_transpose(const float *x, int B, int H, int W, int Cin, const float *w, const float *bias, int Cout, int act,
                            float alpha, float *out, int out_channels, int out_offset, void *stream) {
    const int rc = conv_check(x, B, H, W, Cin, w, Cout, act, alpha, out, out_channels, out_offset, 2ll * H, 2ll * W);
    if (rc != DTFILL_OK) return rc;
    if (!conv_wide_channels(Cin, Cout)) return DTFILL_ERR_SHAPE;
    const ConvArgs a{x, w, bias, nullptr, out, B, H, W, Cin, Cout, 2 * H, 2 * W, 0, 0, out_channels, out_offset, act, alpha};
    conv_transpose_launch(static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_conv2d(const float *x, int B, int H, int W, int Cin, const float *w, const float *bias, int ksize, int Cout, int act,
                  float alpha, float *out, int out_channels, int out_offset, void *stream) {
    const int rc = conv_check(x, B, H, W, Cin, w, Cout, act, alpha, out, out_channels, out_offset, H, W);
    if (rc != DTFILL_OK) return rc;
    if (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7) return DTFILL_ERR_SHAPE;
    if (Cin != 1 && (Cin < CV_G || Cin > 4 * CV_G || Cin % CV_G)) return DTFILL_ERR_SHAPE;
    if (Cout != 1 && Cout != 16) return DTFILL_ERR_SHAPE;
    const int r = (ksize - 1) / 2;
    const ConvArgs a{x, w, bias, nullptr, out, B, H, W, Cin, Cout, H, W, r, r, out_channels, out_offset, act, alpha};
    conv_launch(static_cast<hipStream_t>(stream), a, ksize);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// a slice of `channels` channels at `offset` of a [B,H,W,width] tensor
static bool convb_slice(int B, int H, int W, int channels, int width, int offset) {
    return offset >= 0 && width >= 1 && (long long)offset + channels <= width && (long long)B * H * W * width < (1ll << 31);
}

// The domain of the seven backward calls and everything they and the three size functions derive from a layer; false outside
// the domain.  The narrow rule is dtfill_conv2d's with B H W Cin < 2^31; the image rule is dtfill_conv2d_image's.  The wide rule: whole groups in, whole N-tiles out,
// the frame of dy [Ho,Wo] of a strided layer (stride 2: of an even frame) or [2H,2W] of the transposed one, and x, dy and a
// segment's partials each below 2^31 floats.
static bool convb_plan(const ConvBwLayer &l, ConvBwPlan *p) {
    const int B = l.B, H = l.H, W = l.W, Cin = l.Cin, ksize = l.ksize, Cout = l.Cout;
    const bool k1357 = ksize == 1 || ksize == 3 || ksize == 5 || ksize == 7;
    if (B < 1 || H < 1 || W < 1) return false;
    long long ho = H, wo = W;
    if (l.image) {
        if (!k1357 || l.stride != 1 || l.transposed || !conv_image_channels(Cin, Cout)) return false;
        if ((long long)B * H * W * max(Cin, Cout) >= (1ll << 31) || ((long long)ksize * ksize * Cin + 1) * Cout >= (1ll << 31)) return false;
    } else if (l.narrow) {
        if (!k1357 || l.stride != 1 || l.transposed) return false;
        if (Cin != 1 && (Cin < CV_G || Cin > 4 * CV_G || Cin % CV_G)) return false;
        if (Cout != 1 && Cout != 16) return false;
        if ((long long)B * H * W * Cin >= (1ll << 31)) return false;
    } else {
        if (!conv_wide_channels(Cin, Cout)) return false;
        if (l.transposed) {
            if (ksize != 3 || l.stride != 2) return false;
            ho = 2ll * H, wo = 2ll * W;
        } else if (l.stride == 2) {
            if ((ksize != 1 && ksize != 3) || H % 2 || W % 2) return false;
            ho = H / 2, wo = W / 2;
        } else if (l.stride != 1 || !k1357) {
            return false;
        }
        if (l.bf16 && ksize != 1 && ksize != 3) return false;  // dtfill_conv2d_strided_bf16's domain
        if ((long long)B * H * W * Cin >= (1ll << 31) || B * ho * wo * Cout >= (1ll << 31)) return false;
        if (((long long)ksize * ksize * Cin + 1) * Cout >= (1ll << 31)) return false;
    }
    p->Ho = (int)ho, p->Wo = (int)wo;
    // the weight sum: the segments lie over the output frame, over the input frame of the transposed layer
    p->Hs = l.transposed ? H : p->Ho, p->Ws = l.transposed ? W : p->Wo;
    p->HL = l.transposed ? p->Ho : H, p->WL = l.transposed ? p->Wo : W;
    p->segs_y = (p->Hs + CB_R - 1) / CB_R, p->segs_x = (p->Ws + CB_C - 1) / CB_C;
    const size_t taps = (size_t)ksize * ksize, pixels = (size_t)B * p->Ho * p->Wo;
    p->wt = align256(pixels * Cout * sizeof(float));
    // the kernel the data gradient runs under: float32 wT or wX, or their packed bf16 array (Cout in, Cin out)
    p->tmp = p->wt + align256(l.bf16 ? (size_t)convh_packed_quads(ksize, Cout, Cin) * sizeof(ch_b8) : taps * Cin * Cout * sizeof(float));
    const bool spread = !l.transposed && l.stride == 2 && ksize == 1;  // the chain's values before k_convb_spread
    const size_t data = l.image ? 0 : p->tmp + (spread ? align256(pixels * Cin * sizeof(float)) : 0);  // (the image layer has no dx)
    const size_t weights = align256((size_t)B * p->segs_y * p->segs_x * (taps * Cin + 1) * Cout * sizeof(float));
    p->bytes = data > weights ? data : weights;
    return true;
}

static size_t convb_workspace_bytes(const ConvBwLayer &l) {
    ConvBwPlan p;
    return convb_plan(l, &p) ? p.bytes : 0;
}

size_t dtfill_conv2d_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout) {
    return convb_workspace_bytes(ConvBwLayer{B, H, W, Cin, ksize, Cout, 1, false, true});
}

size_t dtfill_conv2d_wide_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout, int stride, int transposed) {
    return convb_workspace_bytes(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, transposed != 0, false});
}

// what the seven backward calls check alike, in the header's order; the layer's plan and the kernels' view of dy and y over the
// plan's small frame
static int convb_check(const ConvBwLayer &l, const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                       int y_offset, int act, float alpha, const void *workspace, size_t ws_bytes, ConvBwPlan *p, ConvBwArgs *a) {
    if (!dy || !workspace || (act == DTFILL_CONV_LEAKY && !y)) return DTFILL_ERR_NULL;
    if ((act != DTFILL_CONV_LINEAR && act != DTFILL_CONV_LEAKY) || !isfinite(alpha) || alpha < 0.0f) return DTFILL_ERR_SHAPE;
    if (act == DTFILL_CONV_LINEAR) y = nullptr;  // not read
    if (!convb_plan(l, p) || !convb_slice(l.B, p->Ho, p->Wo, l.Cout, dy_channels, dy_offset)) return DTFILL_ERR_SHAPE;
    if (y && !convb_slice(l.B, p->Ho, p->Wo, l.Cout, y_channels, y_offset)) return DTFILL_ERR_SHAPE;
    if (ws_bytes < p->bytes || ((uintptr_t)workspace & 255)) return DTFILL_ERR_WORKSPACE;
    const float *dys = dy + dy_offset, *ys = y ? y + y_offset : nullptr;
    const bool gvec = (((uintptr_t)dys | (uintptr_t)ys) & 15) == 0 && dy_channels % 4 == 0 && (!y || y_channels % 4 == 0);
    *a = ConvBwArgs{nullptr, dys, ys, dy_channels, y ? y_channels : 0, l.B, p->Hs, p->Ws, l.Cin, l.Cout, act, alpha,
                    p->segs_y, p->segs_x, false, gvec};
    return DTFILL_OK;
}

static int convb_data(const ConvBwLayer &l, const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                      int y_offset, const float *w, int act, float alpha, float *dx, int dx_channels, int dx_offset, float *dresidual,
                      void *workspace, size_t ws_bytes, void *stream, decltype(convb_data_launch) *launch = convb_data_launch) {
    if (!w || !dx) return DTFILL_ERR_NULL;
    ConvBwPlan p;
    ConvBwArgs a;
    const int rc = convb_check(l, dy, dy_channels, dy_offset, y, y_channels, y_offset, act, alpha, workspace, ws_bytes, &p, &a);
    if (rc != DTFILL_OK) return rc;
    if (!convb_slice(l.B, l.H, l.W, l.Cin, dx_channels, dx_offset)) return DTFILL_ERR_SHAPE;
    launch(static_cast<hipStream_t>(stream), l, p, a, w, dx, dx_channels, dx_offset, dresidual, workspace);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

static int convb_weights(const ConvBwLayer &l, const float *x, const float *dy, int dy_channels, int dy_offset, const float *y,
                         int y_channels, int y_offset, int act, float alpha, float *dw, float *db, void *workspace, size_t ws_bytes,
                         void *stream, decltype(convb_weights_launch) *launch = convb_weights_launch) {
    if (!x || !dw) return DTFILL_ERR_NULL;
    ConvBwPlan p;
    ConvBwWide a;
    const int rc = convb_check(l, dy, dy_channels, dy_offset, y, y_channels, y_offset, act, alpha, workspace, ws_bytes, &p, &a.b);
    if (rc != DTFILL_OK) return rc;
    a.b.x = x;
    a.b.xvec = ((uintptr_t)x & 15) == 0;  // (Cin is a multiple of 16 wherever 16-byte loads of x are used)
    a.HL = p.HL, a.WL = p.WL;
    launch(static_cast<hipStream_t>(stream), l, a, dw, db, workspace);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

size_t dtfill_conv2d_image_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout) {
    return convb_workspace_bytes(ConvBwLayer{B, H, W, Cin, ksize, Cout, 1, false, false, true});
}

int dtfill_conv2d_image_backward_weights(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                                         int y_offset, int B, int H, int W, int Cin, int ksize, int Cout, int act, float alpha,
                                         float *dw, float *db, void *workspace, size_t ws_bytes, void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, ksize, Cout, 1, false, false, true}, x, dy, dy_channels, dy_offset, y, y_channels,
                         y_offset, act, alpha, dw, db, workspace, ws_bytes, stream);
}

int dtfill_conv2d_backward_data(const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels, int y_offset,
                                const float *w, int B, int H, int W, int Cin, int ksize, int Cout, int act, float alpha, float *dx,
                                int dx_channels, int dx_offset, void *workspace, size_t ws_bytes, void *stream) {
    return convb_data(ConvBwLayer{B, H, W, Cin, ksize, Cout, 1, false, true}, dy, dy_channels, dy_offset, y, y_channels, y_offset, w,
                      act, alpha, dx, dx_channels, dx_offset, nullptr, workspace, ws_bytes, stream);
}

int dtfill_conv2d_backward_weights(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                                   int y_offset, int B, int H, int W, int Cin, int ksize, int Cout, int act, float alpha, float *dw,
                                   float *db, void *workspace, size_t ws_bytes, void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, ksize, Cout, 1, false, true}, x, dy, dy_channels, dy_offset, y, y_channels,
                         y_offset, act, alpha, dw, db, workspace, ws_bytes, stream);
}

int dtfill_conv2d_strided_backward_data(const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels, int y_offset,
                                        const float *w, int B, int H, int W, int Cin, int ksize, int Cout, int stride, int act,
                                        float alpha, float *dx, int dx_channels, int dx_offset, float *dresidual, void *workspace,
                                        size_t ws_bytes, void *stream) {
    return convb_data(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, false, false}, dy, dy_channels, dy_offset, y, y_channels,
                      y_offset, w, act, alpha, dx, dx_channels, dx_offset, dresidual, workspace, ws_bytes, stream);
}

int dtfill_conv2d_strided_backward_weights(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y,
                                           int y_channels, int y_offset, int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                           int act, float alpha, float *dw, float *db, void *workspace, size_t ws_bytes, void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, false, false}, x, dy, dy_channels, dy_offset, y, y_channels,
                         y_offset, act, alpha, dw, db, workspace, ws_bytes, stream);
}

int dtfill_conv2d_transpose_backward_data(const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels, int y_offset,
                                          const float *w, int B, int H, int W, int Cin, int Cout, int act, float alpha, float *dx,
                                          int dx_channels, int dx_offset, void *workspace, size_t ws_bytes, void *stream) {
    return convb_data(ConvBwLayer{B, H, W, Cin, 3, Cout, 2, true, false}, dy, dy_channels, dy_offset, y, y_channels, y_offset, w, act,
                      alpha, dx, dx_channels, dx_offset, nullptr, workspace, ws_bytes, stream);
}

int dtfill_conv2d_transpose_backward_weights(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y,
                                             int y_channels, int y_offset, int B, int H, int W, int Cin, int Cout, int act, float alpha,
                                             float *dw, float *db, void *workspace, size_t ws_bytes, void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, 3, Cout, 2, true, false}, x, dy, dy_channels, dy_offset, y, y_channels, y_offset,
                         act, alpha, dw, db, workspace, ws_bytes, stream);
}

// What the two pool entry points check alike; `lv`: the outs (forward) or the dys (backward) of levels 2, 4, 8, whose widths
// and offsets count only where the pointer is not NULL.  *K: the largest requested level, 1 if there is none.
static int pool_check(int B, int H, int W, int C, int x_channels, int x_offset, const void *const lv[3], const int lc[3],
                      const int lo[3], int *K) {
    *K = lv[2] ? 8 : lv[1] ? 4 : lv[0] ? 2 : 1;
    if (B < 1 || H < 1 || W < 1 || H % *K || W % *K) return DTFILL_ERR_SHAPE;
    if ((long long)B * H >= (1ll << 31) || (long long)B * H * W >= (1ll << 31)) return DTFILL_ERR_SHAPE;
    if (C < 4 || C % 4 || x_channels % 4 || x_offset % 4) return DTFILL_ERR_SHAPE;
    if (!convb_slice(B, H, W, C, x_channels, x_offset)) return DTFILL_ERR_SHAPE;
    for (int l = 0; l < 3; ++l) {
        const int k = 2 << l;
        if (lv[l] && (lc[l] % 4 || lo[l] % 4 || !convb_slice(B, H / k, W / k, C, lc[l], lo[l]))) return DTFILL_ERR_SHAPE;
    }
    return DTFILL_OK;
}

static bool pool_vec(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if ((uintptr_t)p & 15) return false;
    return true;
}

int dtfill_max_pool_pyramid(const float *x, int B, int H, int W, int C, int x_channels, int x_offset, float *out2, int out2_channels,
                            int out2_offset, float *out4, int out4_channels, int out4_offset, float *out8, int out8_channels,
                            int out8_offset, void *stream) {
    if (!x || (!out2 && !out4 && !out8)) return DTFILL_ERR_NULL;
    const void *const lv[3] = {out2, out4, out8};
    const int lc[3] = {out2_channels, out4_channels, out8_channels}, lo[3] = {out2_offset, out4_offset, out8_offset};
    int K;
    const int rc = pool_check(B, H, W, C, x_channels, x_offset, lv, lc, lo, &K);
    if (rc != DTFILL_OK) return rc;
    PoolArgs a{x, {nullptr, nullptr, nullptr}, {out2, out4, out8}, nullptr, B, H, W, C, x_channels, x_offset,
               {lc[0], lc[1], lc[2]}, {lo[0], lo[1], lo[2]}, (long long)B * (H / K) * (W / K) * (C / 4)};
    const bool vec = pool_vec({x, out2, out4, out8});
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (K == 8) pool_launch<8>(st, a, vec);
    else if (K == 4) pool_launch<4>(st, a, vec);
    else pool_launch<2>(st, a, vec);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_max_pool_pyramid_backward(const float *x, int B, int H, int W, int C, int x_channels, int x_offset, const float *dy2,
                                     int dy2_channels, int dy2_offset, const float *dy4, int dy4_channels, int dy4_offset,
                                     const float *dy8, int dy8_channels, int dy8_offset, float *dx, void *stream) {
    if (!x || !dx) return DTFILL_ERR_NULL;
    const void *const lv[3] = {dy2, dy4, dy8};
    const int lc[3] = {dy2_channels, dy4_channels, dy8_channels}, lo[3] = {dy2_offset, dy4_offset, dy8_offset};
    int K;
    const int rc = pool_check(B, H, W, C, x_channels, x_offset, lv, lc, lo, &K);
    if (rc != DTFILL_OK) return rc;
    PoolArgs a{x, {dy2, dy4, dy8}, {nullptr, nullptr, nullptr}, dx, B, H, W, C, x_channels, x_offset,
               {lc[0], lc[1], lc[2]}, {lo[0], lo[1], lo[2]}, (long long)B * (H / K) * (W / K) * (C / 4)};
    const bool vec = pool_vec({x, dy2, dy4, dy8, dx});
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (K == 8) pool_backward_launch<8>(st, a, vec);
    else if (K == 4) pool_backward_launch<4>(st, a, vec);
    else if (K == 2) pool_backward_launch<2>(st, a, vec);
    else pool_backward_launch<1>(st, a, vec);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// counts[0 .. n): every count in [1, 2^31); *total: the floats of m (and of v), each segment rounded up to 4 floats
static bool adam_layout(const long long *counts, int n, unsigned long long *total) {
    *total = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 1 || counts[i] >= (1ll << 31)) return false;
        *total += ((unsigned long long)counts[i] + 3) & ~3ull;
    }
    return *total / 4 <= 0xffffffffull;  // a segment's offset travels as a 32-bit count of quads
}

size_t dtfill_adam_state_floats(const long long *counts, int n) {
    unsigned long long total;
    return counts && n >= 1 && adam_layout(counts, n, &total) ? (size_t)total : 0;
}

size_t dtfill_adam_record_bytes(void) { return sizeof(AdamRecord); }

int dtfill_adam_init(void *record, void *stream) {
    if (!record) return DTFILL_ERR_NULL;
    k_adam_init<><<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(static_cast<AdamRecord *>(record));
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_adam_step(float *const *params, const float *const *grads, const long long *counts, int n, float *m, float *v,
                     void *record, float lr, float beta1, float beta2, float eps, void *stream) {
    if (!params || !grads || !counts || !m || !v || !record) return DTFILL_ERR_NULL;
    if (n < 1) return DTFILL_ERR_SHAPE;
    int stepped = 0;
    for (int i = 0; i < n; ++i) {
        if (!params[i]) return DTFILL_ERR_NULL;
        stepped += grads[i] != nullptr;
    }
    if (!stepped) return DTFILL_ERR_NULL;
    unsigned long long total;
    if (!adam_layout(counts, n, &total)) return DTFILL_ERR_SHAPE;
    if (!(lr >= 0.0f) || !isfinite(lr) || !(eps >= 0.0f) || !isfinite(eps)) return DTFILL_ERR_SHAPE;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) return DTFILL_ERR_SHAPE;
    for (int i = 0; i < n; ++i) {
        const uintptr_t p = (uintptr_t)params[i], g = (uintptr_t)grads[i], bytes = (uintptr_t)counts[i] * 4;
        if (g && p < g + bytes && g < p + bytes) return DTFILL_ERR_SHAPE;
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    AdamArgs a;
    a.m = m, a.v = v, a.rec = static_cast<const AdamRecord *>(record);
    a.lr = lr, a.b1 = beta1, a.b2 = beta2, a.eps = eps, a.n = 0, a.pad_ = 0;
    unsigned long long at = 0;
    u32 chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (grads[i]) {
            const int k = a.n++;
            a.p[k] = params[i], a.g[k] = grads[i], a.seg4[k] = (u32)(at / 4), a.count[k] = (u32)counts[i];
            a.end[k] = chunks += (u32)((counts[i] + ADAM_CHUNK - 1) / ADAM_CHUNK);  // <= 128 * 2^19 a launch
        }
        at += ((unsigned long long)counts[i] + 3) & ~3ull;
        if (a.n == ADAM_GROUP || (a.n && i == n - 1)) {
            k_adam<><<<chunks, ADAM_THREADS, 0, st>>>(a);
            a.n = 0, chunks = 0;
        }
    }
    k_adam_advance<><<<1, 64, 0, st>>>(static_cast<AdamRecord *>(record), beta1, beta2);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// The bf16 forms of the wide layers (dtfill_convh.hpp).  They stand last so that their kernels are asked for last.
static bool convh_channels(int ksize, int Cin, int Cout) {
    return (ksize == 1 || ksize == 3) && conv_wide_channels(Cin, Cout);
}

size_t dtfill_conv2d_bf16_packed_elems(int ksize, int Cin, int Cout) {
    if (!convh_channels(ksize, Cin, Cout) || (long long)Cin * Cout >= (1ll << 31)) return 0;
    const long long quads = convh_packed_quads(ksize, Cin, Cout);
    return quads * CH_Q < (1ll << 31) ? (size_t)quads * CH_Q : 0;
}

int dtfill_conv2d_pack_bf16(const float *w, int ksize, int Cin, int Cout, void *out, void *stream) {
    if (!w || !out) return DTFILL_ERR_NULL;
    if (!dtfill_conv2d_bf16_packed_elems(ksize, Cin, Cout) || ((uintptr_t)out & 15)) return DTFILL_ERR_SHAPE;
    const long long quads = convh_packed_quads(ksize, Cin, Cout);
    k_convh_pack<><<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(w, Cin, Cout, static_cast<ch_b8 *>(out), quads);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_conv2d_strided_bf16(const float *x, int B, int H, int W, int Cin, const void *w, const float *bias, int ksize, int Cout,
                               int stride, const float *residual, int act, float alpha, float *out, int out_channels,
                               int out_offset, void *stream) {
    if (!x || !w || !out) return DTFILL_ERR_NULL;
    if (stride != 1 && stride != 2) return DTFILL_ERR_SHAPE;
    if (H < 1 || W < 1 || !dtfill_conv2d_bf16_packed_elems(ksize, Cin, Cout) || ((uintptr_t)w & 15)) return DTFILL_ERR_SHAPE;
    int Ho, Wo, pt, pl;
    conv2_same(H, ksize, stride, &Ho, &pt);
    conv2_same(W, ksize, stride, &Wo, &pl);
    const float *wp = static_cast<const float *>(w);  // (ConvArgs carries the packed array as it carries a float32 one)
    const int rc = conv_check(x, B, H, W, Cin, wp, Cout, act, alpha, out, out_channels, out_offset, Ho, Wo);
    if (rc != DTFILL_OK) return rc;
    const ConvArgs a{x, wp, bias, residual, out, B, H, W, Cin, Cout, Ho, Wo, pt, pl, out_channels, out_offset, act, alpha};
    convh_strided_launch<>(static_cast<hipStream_t>(stream), a, ksize, stride);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

int dtfill_conv2d_transpose_bf16(const float *x, int B, int H, int W, int Cin, const void *w, const float *bias, int Cout, int act,
                                 float alpha, float *out, int out_channels, int out_offset, void *stream) {
    const float *wp = static_cast<const float *>(w);
    const int rc = conv_check(x, B, H, W, Cin, wp, Cout, act, alpha, out, out_channels, out_offset, 2ll * H, 2ll * W);
    if (rc != DTFILL_OK) return rc;
    if (!dtfill_conv2d_bf16_packed_elems(3, Cin, Cout) || ((uintptr_t)w & 15)) return DTFILL_ERR_SHAPE;
    const ConvArgs a{x, wp, bias, nullptr, out, B, H, W, Cin, Cout, 2 * H, 2 * W, 0, 0, out_channels, out_offset, act, alpha};
    convh_transpose_launch<>(static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? DTFILL_OK : DTFILL_ERR_LAUNCH;
}

// The bf16 forms of the wide layers' backward (dtfill_convhb.hpp): the float32 calls' checks and plan under ConvBwLayer::bf16, the
// launches handed in here so that their kernels are asked for behind every older one.
size_t dtfill_conv2d_wide_backward_bf16_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout, int stride, int transposed) {
    return convb_workspace_bytes(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, transposed != 0, false, false, true});
}

int dtfill_conv2d_strided_backward_data_bf16(const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                                             int y_offset, const float *w, int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                             int act, float alpha, float *dx, int dx_channels, int dx_offset, float *dresidual,
                                             void *workspace, size_t ws_bytes, void *stream) {
    return convb_data(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, false, false, false, true}, dy, dy_channels, dy_offset, y, y_channels,
                      y_offset, w, act, alpha, dx, dx_channels, dx_offset, dresidual, workspace, ws_bytes, stream, convhb_data_launch<>);
}

int dtfill_conv2d_strided_backward_weights_bf16(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y,
                                                int y_channels, int y_offset, int B, int H, int W, int Cin, int ksize, int Cout,
                                                int stride, int act, float alpha, float *dw, float *db, void *workspace, size_t ws_bytes,
                                                void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, ksize, Cout, stride, false, false, false, true}, x, dy, dy_channels, dy_offset, y,
                         y_channels, y_offset, act, alpha, dw, db, workspace, ws_bytes, stream, convhb_weights_launch<>);
}

int dtfill_conv2d_transpose_backward_data_bf16(const float *dy, int dy_channels, int dy_offset, const float *y, int y_channels,
                                               int y_offset, const float *w, int B, int H, int W, int Cin, int Cout, int act, float alpha,
                                               float *dx, int dx_channels, int dx_offset, void *workspace, size_t ws_bytes, void *stream) {
    return convb_data(ConvBwLayer{B, H, W, Cin, 3, Cout, 2, true, false, false, true}, dy, dy_channels, dy_offset, y, y_channels, y_offset,
                      w, act, alpha, dx, dx_channels, dx_offset, nullptr, workspace, ws_bytes, stream, convhb_data_launch<>);
}

int dtfill_conv2d_transpose_backward_weights_bf16(const float *x, const float *dy, int dy_channels, int dy_offset, const float *y,
                                                  int y_channels, int y_offset, int B, int H, int W, int Cin, int Cout, int act,
                                                  float alpha, float *dw, float *db, void *workspace, size_t ws_bytes, void *stream) {
    return convb_weights(ConvBwLayer{B, H, W, Cin, 3, Cout, 2, true, false, false, true}, x, dy, dy_channels, dy_offset, y, y_channels,
                         y_offset, act, alpha, dw, db, workspace, ws_bytes, stream, convhb_weights_launch<>);
}

}  // extern "C"

#ifdef FUSED_PROF
extern "C" int dtfill_fused_prof(unsigned long long *out16, int reset) {
    static unsigned long long h[F_PROF_SLOTS][16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fused_prof), sizeof(h)) != hipSuccess) return -1;
    for (int k = 0; k < 16; ++k) {
        out16[k] = 0;
        for (int i = 0; i < F_PROF_SLOTS; ++i) out16[k] += h[i][k];
    }
    if (reset) {
        for (auto &r : h)
            for (auto &v : r) v = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_fused_prof), h, sizeof(h)) != hipSuccess) return -1;
    }
    return 0;
}
// the timeline records (g_fused_tl) of the last pass(es) since a reset: F_TL_WAVES x F_TL_EV u64 into out
extern "C" int dtfill_fused_timeline(unsigned long long *out, int reset) {
    const size_t n = sizeof(unsigned long long) * F_TL_WAVES * F_TL_EV;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fused_tl), n) != hipSuccess) return -1;
    if (reset) {
        void *d = nullptr;
        if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_fused_tl)) != hipSuccess || hipMemset(d, 0, n) != hipSuccess) return -1;
        if (hipDeviceSynchronize() != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef PTS_PROF
extern "C" int dtfill_pts_prof(unsigned long long *out8, int reset) {
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_pts_prof), sizeof(z)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_pts_prof), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif

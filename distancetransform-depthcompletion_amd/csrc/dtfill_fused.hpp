// dtfill_fused.hpp -- k_fused<FR>: the bit-sliced LDS-window kernel of the l1_cv pass
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// k_fused: one workgroup (4 waves) per window = tile (<= 96 x 160) + halo FR, bit-sliced.
//
// Lane (r, half) owns half of window row r as three 32-bit words per bit plane (bit c%32 of word c/32 = window
// column c).  Level-synchronous form of the identity of DESIGN.md section 2 (checked in tests/parallel_model.py):
// with E_t = {d == t} and L_t = live pixels of E_t (E_0 = L_0 = sources),
//   E_t = dilate4(D_{t-1}) & ~D_{t-1} & in-image
//   forward tap T = (di,dj,w) offers   shift(L_{t-w}, di, dj)   to the pixels of E_t; L_t = those offered any
//   backward tap (negated offset)      candidates of level t-w for the pixels of E_t \ L_t
//   the FIRST tap in cv2 order wins (taken-mask chain); the winner is recorded in four "code planes"
//   holding the bits of its plane code (dtfill_taps.hpp): the parent code 0..15 itself; sources: CODE_SOURCE.
// The level loop runs the forward taps (they define L_t) and ORs E_t into three planes of d mod 8; the backward
// taps run ONCE after it for all levels, on those planes (bwd_tap).  A horizontal shift of a row is one
// v_alignbit per word; rows r-2..r+2 of the previous three levels come from a 4-slot LDS ring (one barrier per
// level).  Levels stop at FR, when a level is empty, or when every tile pixel is decided.
// Then every lane un-slices its row, 8 pixels per step, into the byte array s_par (2 * plane code; F_NONE =
// undecided), which reuses the ring's memory, and the tile pixels walk to their sources in lock-step:
// the byte is the byte offset of the step's s_par displacement in a 16-entry int16 table (s_tab), so a
// hop is two LDS reads and one add; d is |drow| + |dcol| to the root.
// LDS: 28.9 KB ring/s_par + 8 KB rank records.
// ------------------------------------------------------------------------------------------------
// (the window itself, F_WHM rows x F_WWM columns, is dtfill_route.hpp's: the tilings rest on it)
constexpr int F_NT = 256;   // lane = (row, half): waves 0-1 own words 0..2 of rows 0..127, waves 2-3 words 3..5
constexpr int F_P = 196;               // s_par row pitch: 49 dwords (odd) -> lane-per-row dword stores are conflict-free
constexpr int F_NWD = 6;               // 32-bit words per window row
constexpr int F_HW = 3;                // words per lane
constexpr int F_RS = 7;                // ring row stride in words: 6 + one zero pad (odd: conflict-free; the pad is
                                       // also the zero "word -1" of the next row and "word 6" of this one)
constexpr int F_RROWS = F_WHM + 4;     // ring rows: 2 zero rows above and below the window
constexpr int F_RPLANE = F_RROWS * F_RS;
constexpr int F_RING = 1 + 4 * 2 * F_RPLANE;  // one leading zero word, then [slot][plane E/L][row][7]
constexpr int F_NPLANES = 4;           // code planes: the bits of the plane code (dtfill_taps.hpp)
constexpr int F_EB = 8;                // tile pixels per lane walked in lock-step
// byte code of a decided pixel: 2 * plane code (a source: 2 * CODE_SOURCE = step (0,0))
constexpr int F_NONE = 2 * CODE_NONE;  // byte code of an undecided pixel: also step (0,0)
static_assert(CODE_SOURCE < (1 << F_NPLANES) && CODE_NONE < (1 << F_NPLANES) && !code_wins(CODE_SOURCE) && !code_wins(CODE_NONE), "the reserved codes fit the planes and never win");
static_assert(F_WWM == 32 * F_NWD, "window width must be six words");
static_assert(F_RING * 4 >= F_WHM * F_P + 256 * 8, "s_par and the un-slicing table must fit in the ring's memory");
static_assert((F_WHM * F_P) % 8 == 0 && F_WHM * F_P >= 4 * (1 + 4 * F_RPLANE), "the table is 8-byte aligned and lies behind the planes of P1b");

// One forward tap T (dtfill_taps.hpp) of the first-match chain.  src = the live pixels of the level BACK levels back, in the
// window row ROW below the lane's, with their neighbour words (src[1..3] = the lane's three words): what the call site loaded
// must be what the table says.  cand = shift(src, dj); the winners get the bits of the plane code in the code planes.
template <int T, int ROW, int BACK>
__device__ __forceinline__ void tap_step(const u32 (&src)[5], u32 (&taken)[F_HW], u32 (&C)[F_NPLANES][F_HW]) {
    static_assert(T >= 0 && T < 8 && ROW == code_di(T) && BACK == code_weight(T), "tap T reads row r + di of level t - weight");
    static_assert(code_wins(T), "a reserved code is no tap");
#pragma unroll
    for (int i = 0; i < F_HW; ++i) {
        const u32 cand = row_shift<code_dj(T)>(src + i);
        const u32 sel = cand & ~taken[i];
        taken[i] |= cand;
#pragma unroll
        for (int j = 0; j < F_NPLANES; ++j)
            if (plane_code(T) & (1 << j)) C[j][i] |= sel;
    }
}

// One BACKWARD tap (parent code T | 8), evaluated after the level loop for all levels at once: the candidate r = q + (ROW, dj)
// matches iff it is decided (dv) and d(r) + weight == d(q).  Only d mod 8 is kept (planes a0..a2 / b0..b2: dist_match).
template <int T, int ROW>
__device__ __forceinline__ void bwd_tap(const u32 (&a0)[5], const u32 (&a1)[5], const u32 (&a2)[5], const u32 (&dv)[5],
                                        const u32 (&b0)[F_HW], const u32 (&b1)[F_HW], const u32 (&b2)[F_HW],
                                        u32 (&taken)[F_HW], u32 (&C)[F_NPLANES][F_HW]) {
    constexpr int CODE = T | 8, DJ = code_dj(CODE);
    static_assert(T >= 0 && T < 8 && ROW == code_di(CODE), "backward tap T reads row r - di");
    static_assert(code_wins(CODE), "codes 13 and 14 never select (dtfill_taps.hpp): they mean source and undecided here");
#pragma unroll
    for (int i = 0; i < F_HW; ++i) {
        const u32 m = dist_match<code_weight(CODE)>(row_shift<DJ>(a0 + i), row_shift<DJ>(a1 + i), row_shift<DJ>(a2 + i), b0[i], b1[i], b2[i]) &
                      row_shift<DJ>(dv + i);
        const u32 sel = m & ~taken[i];
        taken[i] |= m;
#pragma unroll
        for (int j = 0; j < F_NPLANES; ++j)
            if (plane_code(CODE) & (1 << j)) C[j][i] |= sel;
    }
}

// 24-bit multiply the optimiser cannot see through: written as a plain product it folds the following shift
// into the constant, which then no longer fits 24 bits and becomes a quarter-rate v_mul_lo_u32
__device__ __forceinline__ u32 mul_u24_opaque(u32 a, u32 b) {
    u32 r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

#ifdef FUSED_PROF  // development probe (scripts/dev/fused_phase_probe.py): cycles per phase summed over the waves, and trip counts
// one record per wave slot (waves of the grid modulo F_PROF_SLOTS): no atomics contend for a line; the reader sums them
constexpr int F_PROF_SLOTS = 8192;
__device__ unsigned long long g_fused_prof[F_PROF_SLOTS][16];
// Timeline: per wave of the grid (up to F_TL_WAVES), its first F_TL_EV phase changes in order, each one u64
// = constant-clock time (s_memrealtime, 100 MHz) << 4 | the phase that ENDS there (15: the wave's start); 0 = no entry.
// The reader bins them into the share of working waves in each phase over time.
constexpr int F_TL_WAVES = 1 << 16, F_TL_EV = 32;
__device__ unsigned long long g_fused_tl[F_TL_WAVES][F_TL_EV];
__device__ __forceinline__ unsigned long long fprof_realtime() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
// per wave: t[k] cycles of phase k (P0 load, P1 levels, P1b backward taps, P2 un-slice, P3 hops, P3 epilogue + stores, tail),
// n[k] counts (waves, levels run, batches, walkers, -, hop trips (two hops each), -, -)
struct FusedProf {
    unsigned long long t[8] = {}, n[8] = {}, tprev = __builtin_readcyclecounter();
    int nev = 0;
    __device__ int wave() const { return (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); }
    __device__ void event(int k) {
        const unsigned long long rt = fprof_realtime();
        if ((threadIdx.x & 63) == 0 && wave() < F_TL_WAVES && nev < F_TL_EV) g_fused_tl[wave()][nev] = rt << 4 | (unsigned)k;
        ++nev;
    }
    __device__ FusedProf() { event(15); }
    __device__ void mark(int k) {
        const unsigned long long t_ = __builtin_readcyclecounter();
        t[k] += t_ - tprev;
        tprev = t_;
        event(k);
    }
    __device__ void flush() {
        const int slot = wave() % F_PROF_SLOTS;
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; ++k) {
                atomicAdd(&g_fused_prof[slot][k], t[k]);
                atomicAdd(&g_fused_prof[slot][8 + k], n[k]);
            }
    }
};
#define FPROF(...) __VA_ARGS__
#else
#define FPROF(...)
#endif

// the lane's three words of a ring row plus one neighbour word on each side (pads / other half)
__device__ __forceinline__ void ring_load5(const u32 *__restrict__ ring, int slot, int plane, int row, int wb,
                                           u32 (&a)[5]) {
    const u32 *p = ring + 1 + (slot * 2 + plane) * F_RPLANE + row * F_RS + wb - 1;
#pragma unroll
    for (int i = 0; i < 5; ++i) a[i] = p[i];
}
__device__ __forceinline__ void ring_store3(u32 *__restrict__ ring, int slot, int plane, int row, int wb,
                                            const u32 (&w)[F_HW]) {
    u32 *p = ring + 1 + (slot * 2 + plane) * F_RPLANE + row * F_RS + wb;
#pragma unroll
    for (int i = 0; i < F_HW; ++i) p[i] = w[i];
}

// P3 of the fused pass as a function of the staged window (s_par byte codes, s_rw rank half words): tile
// pixels walk to their sources in lock-step, d, rank -> label, gather, store.  Returns whether some tile pixel
// was undecided.  NT = threads of the calling block.
template <int FR, int NT, bool EPI, bool STREAM>
__device__ __forceinline__ bool fused_walk_epilogue(
    const u8 *__restrict__ s_par, const short *__restrict__ s_tab, const uint2 *__restrict__ s_rw, int b, int H,
    int W, int th, int tw, int r0, int c0, int wr0, int wc0, int sh, const float *__restrict__ x,
    const float *__restrict__ vlist,
    int *__restrict__ finfo, int nval, int misaligned, int sky0, float *__restrict__ out_depth, float *__restrict__ out_dt,
    int32_t *__restrict__ out_index, int *__restrict__ frame_status, const DepthEpilogue ep, u32 *__restrict__ rowflag
    FPROF(, FusedProf &prof)) {
    // ---- P3: tile pixels: walk to the source, d, rank -> label, gather, store.  Each lane walks F_EB
    // pixels in lock-step (their LDS reads are independent, so the hop latencies overlap) and then has
    // F_EB global gathers in flight together.
    // Frame bases are block-uniform (scalar registers); per pixel only 32-bit in-frame offsets are computed.
    const size_t fo = (size_t)b * H * W;
    // (nval, misaligned, sky0: the frame's FI_NVAL, FI_MISALIGNED, FI_SKY -- block-uniform)
    const float *gbase = misaligned ? vlist + fo : x + fo;
    // The outputs leave through buffer stores, one descriptor per frame and map (block-uniform): a store the pass does not
    // make -- an undecided pixel, a cropped row, a map the caller did not ask for (0 records) -- is a store whose offset the
    // range check drops.  So every batch issues the same stores, branch-free, and the compiler's vmcnt waits for a batch's
    // gathers are exact: they no longer wait for the label / distance stores issued behind them (in-order vmcnt; with
    // branches around the stores it has to assume the path without them and wait for all but seven).
    // A descriptor's records end with the tile's last row: a slot's rows below the tile (the last row group of a tile whose
    // height is no multiple of F_EB; still cells of the window, read and walked) are dropped the same way, without a compare.
    // the depth output may drop the first ep.row0 rows (then frames are H - row0 rows apart)
    // bytes of a frame's dropped rows; a pixel of them wraps past the records (the plain instances subtract nothing)
    const u32 dcrop = EPI ? (u32)(ep.row0 * W) << 2 : 0u;
    // r0 + th <= H: never past the frame.  (Block-uniform, but a premarked tile's span comes out of LDS: the record counts
    // are said to be uniform below, or every store is wrapped in a loop over the lanes' descriptors)
    const u32 tbytes = (u32)((r0 + th) * W) << 2;
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    const auto rs_d = __builtin_amdgcn_make_buffer_rsrc(out_depth ? out_depth + (size_t)b * (H - ep.row0) * W : nullptr, 0,
                                                        uni(out_depth && tbytes > dcrop ? (int)(tbytes - dcrop) : 0), 0x00020000);
    const auto rs_t = __builtin_amdgcn_make_buffer_rsrc(out_dt ? out_dt + fo : nullptr, 0, uni(out_dt ? (int)tbytes : 0), 0x00020000);
    const auto rs_i = __builtin_amdgcn_make_buffer_rsrc(out_index ? out_index + fo : nullptr, 0, uni(out_index ? (int)tbytes : 0), 0x00020000);
    constexpr u32 OFF_NONE = 0x80000000u;  // past every frame's records (a frame has < 2^26 pixels), with up to F_EB rows added too
    const char *tab = reinterpret_cast<const char *>(s_tab);
    auto step_of = [&](int c) { return (int)*reinterpret_cast<const short *>(tab + c); };
    const int src_base = wr0 * W + wc0;  // frame offset of window cell (0,0) (may be negative)
    const int wrest = W - F_P;           // frame offset of an s_par position: src_base + pos + row * wrest
    const u32 last_px = (u32)(H * W - 1);
    bool overflow = false;
    // STREAM (rows of whole 128-byte lines: W % 32 == 0, aligned outputs, tile columns in whole lines): a wave's run of
    // consecutive tile pixels is whole lines, and nothing of the outputs is read again in this pass -- streaming stores
    // (nt) keep them from pushing the inputs out of the caches.  Otherwise the L2 has to merge the partial lines: plain stores.
    auto put = [](__amdgpu_buffer_rsrc_t rs, u32 off, u32 v) { __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)off, 0, STREAM ? 2 : 0); };
    // A lane walks F_EB pixels of ONE column, rows 8 g .. 8 g + 7 of the tile: slot L = sb + tid is (row group g, column) =
    // divmod(L, tw), so the index arithmetic is done once per slot and the F_EB pixels differ by a row pitch each; a wave's store
    // is still a run of 64 consecutive pixels of a row (two runs where the slots wrap into the next group).
    // Software pipeline: the depth gathers of one batch stay in flight during the walk of the next batch (LDS only);
    // a batch's depth stores are issued just before the next batch's gathers.  Label and distance are stored at once.
    const int nslots = ((th + F_EB - 1) / F_EB) * tw;
    const float inv_tw = 1.0f / (float)tw;
    const u32 w4 = (u32)W << 2;
    float p_val[F_EB];  // the batch whose gathers are in flight
#pragma unroll
    for (int e = 0; e < F_EB; ++e) p_val[e] = 0.0f;
    // A batch's store offsets are computed once, at its head, and kept in registers: BYTE offsets (< 2^32: a frame has < 2^26
    // pixels; descriptor base + 32-bit vector offset), OFF_NONE for a pixel that is not stored.  p_o: those of the batch in flight.
    // OFF_NONE - dcrop is still past every frame's records.
    u32 p_o[F_EB];
#pragma unroll
    for (int e = 0; e < F_EB; ++e) p_o[e] = OFF_NONE;
    auto retire = [&]() {
#pragma unroll
        for (int e = 0; e < F_EB; ++e) put(rs_d, p_o[e] - dcrop, __float_as_uint(EPI ? depth_epilogue(p_val[e], ep) : p_val[e]));
    };
    for (int sb = 0; sb < nslots; sb += NT) {
        int pos[F_EB], step[F_EB], code[F_EB];  // pos = row * F_P + col: byte index in s_par
        u32 o[F_EB], home0;   // home0: window row << 16 | window column of the slot's first pixel
        FPROF(prof.mark(5); ++prof.n[2]);
        {
            const int L = sb + (int)threadIdx.x, Lc = min(L, nslots - 1);
            // L / tw: (L + 0.5) / tw is at least 0.5 / tw away from an integer, far above float rounding
            // for L < 2^14, tw < 2^8
            const int g = (int)(((float)Lc + 0.5f) * inv_tw);
            const int tc = Lc - __mul24(g, tw), trb = g * F_EB;
            home0 = (u32)(FR + trb) << 16 | (u32)(FR + tc);
            // byte offset; 24-bit multiplies are full rate (H, W < 8192).  A lane without a slot stores nothing
            u32 op = L < nslots ? (u32)(__mul24(r0 + trb, W) + c0 + tc) << 2 : OFF_NONE;
            const int pos0 = __mul24(FR + trb, F_P) + FR + tc;
            unsigned long long und = 0;  // lanes with an undecided cell among their eight
#pragma unroll
            for (int e = 0; e < F_EB; ++e) {
                pos[e] = pos0 + e * F_P;
                code[e] = s_par[pos[e]];
                und |= __ballot(code[e] == F_NONE);
                o[e] = code[e] != F_NONE ? op : OFF_NONE;  // (a row below the tile: past the records)
                // The offset is wanted HERE, in a register, and the next row's as a running add: left alone the compiler
                // sinks the select below the walk and keeps the eight code bytes and the compares' mask pairs alive instead,
                // and turns the adds into eight uniform multiples of the pitch (scalar registers the loop does not have).
                asm volatile("" : "+v"(o[e]), "+v"(op));
                op += w4;
            }
            // undecidable here: the any-distance kernels take the pixel's row (found again below, off the common path).
            // Wave-uniform and rare: only now does it matter whether the cell is one of the slot's rows inside the tile
            if (und) {
                const int nv = L < nslots ? th - trb : 0;
#pragma unroll
                for (int e = 0; e < F_EB; ++e) overflow |= e < nv && code[e] == F_NONE;
            }
        }
        // Unconditional hops: sources and undecided cells carry the step (0,0), so a walker that has
        // arrived just stays.  No selects, no divergent control flow -- the reads of the F_EB walkers
        // overlap.  Two hops between "everybody arrived?" checks.
        for (int hop = 0; hop < FR + 2; hop += 2) {
#pragma unroll
            for (int e = 0; e < F_EB; ++e) step[e] = step_of(code[e]);
            // everybody arrived? -- asked right after the (cheap, broadcast) table read, so the last trip
            // through the loop costs those 8 reads and not two more full hops
            int moving = 0;
#pragma unroll
            for (int e = 0; e < F_EB; ++e) moving |= step[e];
            if (!__any(moving != 0)) break;
            FPROF(++prof.n[5]);
#pragma unroll
            for (int e = 0; e < F_EB; ++e) pos[e] += step[e];
#pragma unroll
            for (int e = 0; e < F_EB; ++e) code[e] = s_par[pos[e]];
#pragma unroll
            for (int e = 0; e < F_EB; ++e) step[e] = step_of(code[e]);
#pragma unroll
            for (int e = 0; e < F_EB; ++e) pos[e] += step[e];
#pragma unroll
            for (int e = 0; e < F_EB; ++e) code[e] = s_par[pos[e]];
        }
        FPROF(prof.mark(4); for (int e = 0; e < F_EB; ++e) prof.n[3] += __popcll(__ballot(o[e] != OFF_NONE)));
        int pr[F_EB];
        u32 rc[F_EB], goff[F_EB];  // rc = row << 16 | column of the root in the window
        int lab[F_EB];
        // a decided chain ends on a source inside the in-image window.  F_RG pixels at a time: their rank records are read
        // together (independent LDS reads, one wait for the group) and the popcounts follow
        constexpr int F_RG = 4;
#pragma unroll
        for (int h = 0; h < F_EB; h += F_RG) {
            int bp[F_RG], ri[F_RG];
            uint2 rw[F_RG];
            // pos / F_P by a 24-bit multiply: 196 * 5350 / 2^20 = 1 + 2.3e-5, pos / 196 < 128, so the product is at most 0.003 above
            // the quotient, whose fraction is at most 195 / 196: same integer part (three full-rate instructions with the remainder;
            // the integer division is a quarter-rate v_mul_hi_u32)
            static_assert(F_P == 196 && F_WHM * F_P < (1 << 15), "the reciprocal below is F_P's");
#pragma unroll
            for (int k = 0; k < F_RG; ++k) {
                const int e = h + k;
                pr[e] = (int)(__umul24((u32)pos[e], 5350u) >> 20);
                rc[e] = __umul24((u32)pr[e], 65536u - F_P) + (u32)pos[e];  // pos = row * F_P + column: one multiply-add
                // bits 0..7: the bit index in the row's image-aligned bit string, from word w0 (sh + column < 256);
                // the row above them does not matter to the two bit-field extracts
                bp[k] = (int)(rc[e] + (u32)sh);
                ri[k] = pr[e] * 8 + (int)__builtin_amdgcn_ubfe((u32)bp[k], 5u, 3u);
            }
#pragma unroll
            for (int k = 0; k < F_RG; ++k) rw[k] = s_rw[ri[k]];  // {32 source bits, 1 + sources before them in the frame}
            // the bits below the pixel's: v_bfe_u32 takes the low five bits of its width operand
#pragma unroll
            for (int k = 0; k < F_RG; ++k) lab[h + k] = (int)rw[k].y + __popc(__builtin_amdgcn_ubfe(rw[k].x, 0u, (u32)bp[k]));
        }
        // depth_list[label - 1].  A decided pixel has label >= 1: depth_index_pos (dtfill_index.hpp).  Masks agree
        // (block-uniform): the label-th value is x at the source, and label <= nsrc = nval: nothing to test.
        // The min only makes sure that a logic error could never become a wild global access (an LDS index
        // out of range reads garbage at worst).
        if (!misaligned) {
#pragma unroll
            for (int e = 0; e < F_EB; ++e) {
                u32 t = (u32)(__mul24(pr[e], wrest) + pos[e]);
                asm("" : "+v"(t));  // one multiply-add, one add-shift: an instruction reads one scalar register, summed the other way round they are three
                goff[e] = min((t + (u32)src_base) << 2, last_px << 2);  // byte offset
            }
        } else {
            bool bad = false;
            const int nv = th + FR - (int)(home0 >> 16);  // the slot's rows inside the tile (a lane without a slot: no offsets at all)
#pragma unroll
            for (int e = 0; e < F_EB; ++e) {
                const DepthIndex di = depth_index_pos(lab[e], nval);
                bad |= o[e] != OFF_NONE && e < nv && !di.ok;
                goff[e] = (di.ok ? min((u32)di.idx, last_px) : 0u) << 2;
            }
            if (bad && out_depth) atomicOr(frame_status + b, DTFILL_FRAME_INDEX_ERROR);
        }
        retire();  // the previous batch: its gathers had the whole walk above to arrive
#pragma unroll
        for (int e = 0; e < F_EB; ++e) p_val[e] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(gbase) + goff[e]);
#pragma unroll
        for (int e = 0; e < F_EB; ++e) {
            p_o[e] = o[e];
            put(rs_i, o[e], (u32)lab[e]);
            // L1 distance to the nearest source IS d: |drow| + |dcol| of the two 16-bit halves in one instruction
            put(rs_t, o[e], __float_as_uint((float)__builtin_amdgcn_sad_u16(rc[e], home0 + ((u32)e << 16), 0u)));
        }
    }
    FPROF(prof.mark(5));
    retire();
    const bool any = __any(overflow);  // wave-uniform
    // The rows with an undecided pixel are redone by the any-distance kernels (every pixel of them; the decided ones get the
    // same values again).  With a depth epilogue the whole frame is (its chains may end on finished pixels whose stored
    // depth is already cropped / floored).  Rare, so a wave that met one looks for its rows only now (s_par is still there).
    if (any && !EPI) {
        for (int L = threadIdx.x; L < nslots; L += NT) {  // the slots this thread walked above
            const int g = L / tw, tc = L - g * tw;
            for (int tr = g * F_EB; tr < min(g * F_EB + F_EB, th); ++tr)
                if (s_par[__mul24(FR + tr, F_P) + FR + tc] == F_NONE) {
                    rowflag[(size_t)b * H + r0 + tr] = 1u;  // same-value race
                    // one of the two rows k_sky starts from: the any-distance kernels take the sky's rows as well (the sky is
                    // called off by a bit ORed into FI_SKY: the frame's publishing block may be ORing the rows into it in this very launch)
                    if (sky0 > 0 && (r0 + tr == sky0 || r0 + tr == sky0 + 1)) atomicOr(&finfo[b * FI_STRIDE + FI_SKY], SKY_OFF);
                }
        }
    }
    return any;
}

// FR = halo = largest distance the window can decide.  The geometry of a halo's tiling: FusedTiles, window_tiling (dtfill_route.hpp)
template <int FR, bool EPI, bool STREAM>
__device__ __forceinline__ void fused_body(int tile, bool premarked, int tbase, int nval, int misaligned, int sky0, const u32 *__restrict__ s_bs,
    const u32 *__restrict__ s_far,
    const float *__restrict__ x, const u64 *__restrict__ srcbits, const u16 *__restrict__ wpre_s,
    const u32 *__restrict__ rowbase_s, int *__restrict__ finfo, const float *__restrict__ vlist,
    int H, int W, int Wd, int nty, int TW, int tiles_x, float *__restrict__ out_depth,
    float *__restrict__ out_dt, int32_t *__restrict__ out_index,
    int *__restrict__ fflag, u32 *__restrict__ rowfar, int *__restrict__ frame_status, const DepthEpilogue ep, u32 *__restrict__ s_ring, uint2 *__restrict__ s_rw,
    short *__restrict__ s_tab, u32 (*__restrict__ s_any)[F_NT / 64]) {
    const int tid = threadIdx.x;
    // (frames along x, tiles along y: the tiles beyond a frame's own tiling, which exit, are dispatched after every working block)
    const int b = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    // the tile rows split the rows from tbase = FI_TR0 on evenly (frame_facts: 0, or the first source row under a sky): the
    // height frame_facts culled whole tile rows by
    // s_bs, s_far (LDS, inside the ring's memory; null when a k_frame launch went before): the frame's rank bases per row and
    // its pre-marked rows as bits, as this block's own frame_facts left them -- else rowbase_s and rowfar say the same
    const int TH = tile_row_height(H, tbase, nty);
    int r0 = tbase + ty * TH;
    const int c0 = tx * TW;
    int th = min(TH, H - r0);
    const int tw = min(TW, W - c0);
    if (th <= 0) return;  // block-uniform
    if (premarked) {
        // rows of this frame were handed to the any-distance kernels up front (the empty sky): the tile shrinks to the span
        // of its rows that are still this kernel's; a tile without any is done.  (A row another block marks meanwhile is
        // redone whole as well: whether this block still stores its part of it does not matter.)
        const u32 *rowflag = rowfar + (size_t)b * H;
        auto mine = [&](int i) { return s_far ? ((s_far[i >> 5] >> (i & 31)) & 1u) == 0u : rowflag[i] == 0u; };
        if (tid == 0) {
            s_any[0][0] = 0xFFFFFFFFu;
            s_any[0][1] = 0u;
        }
        __syncthreads();
        if (tid < th && mine(r0 + tid)) {
            atomicMin(&s_any[0][0], (u32)tid);
            atomicMax(&s_any[0][1], (u32)tid + 1u);
        }
        __syncthreads();
        const u32 lo = s_any[0][0], hi = s_any[0][1];
        if (hi == 0u) return;  // block-uniform
        r0 += (int)lo;
        th = (int)(hi - lo);
    }
    FPROF(FusedProf prof; prof.n[0] = 1);
    const int wr0 = r0 - FR, wc0 = c0 - FR;  // image coords of window cell (0,0)
    const int WH = th + 2 * FR, WW = tw + 2 * FR;
    const int ca = max(0, -wc0), cb = min(WW, W - wc0);  // in-image window columns [ca, cb)
    const int w0 = wc0 >> 6;                             // first image word column the window touches (-1 if wc0 < 0)
    const int sh = wc0 - 64 * w0;                        // window column 0 is bit sh of image word w0

    // ---- P0: this lane's half row: image-aligned words -> LDS (for the ranks), window-aligned planes -> registers
    const int r = tid & (F_WHM - 1);  // window row of this lane
    const int hf = tid >> 7;          // which half of the row (wave-uniform)
    const int wb = F_HW * hf;         // first of the lane's three words
    u32 M[F_HW], D[F_HW], TM[F_HW];  // in-image mask, decided pixels, tile pixels (of the lane's three words)
    {
        const int gi = wr0 + r;
        const bool rowin = r < WH && gi >= 0 && gi < H;
        // the lane's 96 window columns start at bit sh + 96 hf of the row's image-aligned bit string;
        // three image words (192 bits) starting at word (sh + 96 hf) / 64 cover them
        const int bit0 = sh + 96 * hf;
        const int kw = bit0 >> 6;  // wave-uniform
        u32 g[7];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int kk = kw + k;  // 0..3 relative to w0
            const int w = w0 + kk;
            u64 sb = 0;
            u32 rk = 0;
            if (rowin && kk < 4 && w >= 0 && w < Wd) {
                const size_t wi = ((size_t)b * H + gi) * Wd + w;
                sb = srcbits[wi];
                rk = (s_bs ? s_bs[gi] : rowbase_s[(size_t)b * H + gi]) + wpre_s[wi];
            }
            g[2 * k] = (u32)sb;
            g[2 * k + 1] = (u32)(sb >> 32);
            // each of the four image words of a row is stored once: half 0 stores its words kk = 0, 1 (and 2
            // if half 1 starts later), half 1 the rest
            const bool mine = hf == 0 ? kk < 2 : (kk >= 2 && kk < 4);
            if (mine) {
                s_rw[r * 8 + 2 * kk] = make_uint2((u32)sb, rk + 1u);
                s_rw[r * 8 + 2 * kk + 1] = make_uint2((u32)(sb >> 32), rk + 1u + (u32)__popc((u32)sb));
            }
        }
        g[6] = 0;
        const int s6 = bit0 & 63;
        const bool hi = s6 & 32;  // wave-uniform
        const int s5 = s6 & 31;
#pragma unroll
        for (int i = 0; i < F_HW; ++i) {
            const u32 lo_w = hi ? g[i + 1] : g[i], hi_w = hi ? g[i + 2] : g[i + 1];
            const u32 word = s5 ? __builtin_amdgcn_alignbit(hi_w, lo_w, s5) : lo_w;
            // in-image columns of window word wb + i: [max(ca, 32 (wb+i)), min(cb, 32 (wb+i) + 32))
            const int lo = max(ca - 32 * (wb + i), 0), up = min(cb - 32 * (wb + i), 32);
            u32 m = 0;
            if (rowin && up > lo) m = (up >= 32 ? 0xFFFFFFFFu : ((1u << up) - 1u)) & ~((1u << lo) - 1u);
            M[i] = m;
            D[i] = word & m;
            // tile columns of window word wb + i: [FR, FR + tw) -- rows [FR, FR + th)
            const int tlo = max(FR - 32 * (wb + i), 0), tup = min(FR + tw - 32 * (wb + i), 32);
            u32 tm = 0;
            if (r >= FR && r < FR + th && tup > tlo) tm = (tup >= 32 ? 0xFFFFFFFFu : ((1u << tup) - 1u)) & ~((1u << tlo) - 1u);
            TM[i] = tm;
        }
    }
    // level 0: E_0 = L_0 = sources; zero the rest of the ring (levels "-1,-2,-3", the guard rows, the pads)
    if (s_bs) __syncthreads();  // block-uniform: everybody has read the frame facts that lie in the ring's memory
    for (int k = tid; k < F_RING; k += F_NT) s_ring[k] = 0;
    if (tid < (1 << F_NPLANES)) {
        int di, dj;
        code_step(tid, di, dj);
        s_tab[tid] = (short)(di * F_P + dj);
    }
    __syncthreads();
    ring_store3(s_ring, 0, 0, r + 2, wb, D);
    ring_store3(s_ring, 0, 1, r + 2, wb, D);
    u32 C[F_NPLANES][F_HW];
    u32 Lv[F_HW];  // the live pixels so far: L_0 | .. | L_t (forward tap 0's plane code is 0, so the planes alone do not tell)
#pragma unroll
    for (int i = 0; i < F_HW; ++i) {
        Lv[i] = D[i];
#pragma unroll
        for (int j = 0; j < F_NPLANES; ++j) C[j][i] = ((CODE_SOURCE >> j) & 1) ? D[i] : 0u;  // sources
    }
    u32 Dup[F_HW], Ddn[F_HW];
    u32 Dl = 0, Dr = 0;  // D's neighbour words left / right of the lane's three (other half or nothing)
#pragma unroll
    for (int i = 0; i < F_HW; ++i) Dup[i] = Ddn[i] = 0;
    __syncthreads();
    FPROF(prof.mark(0));

    // ---- P1: levels.  Per level: E_t (dilation), L_t (forward taps, winners recorded), d mod 8 planes.
    u32 P0[F_HW], P1[F_HW], P2[F_HW];  // bits 0..2 of the level at which a pixel was decided (sources: 0)
#pragma unroll
    for (int i = 0; i < F_HW; ++i) P0[i] = P1[i] = P2[i] = 0;
    // (the level as a lambda that says whether to go on, the loop asking it in its condition: with the body written into the loop
    // and a break at its end the kernel came out with 20 bytes of scratch)
    auto level = [&](const int t) __attribute__((always_inline)) -> bool {
        FPROF(++prof.n[1]);
        const int s1 = (t - 1) & 3, s2 = (t - 2) & 3, s3 = (t - 3) & 3, sw = t & 3;
        u32 nb[5], e1[5], l1[5], taken[F_HW], Et[F_HW], Lt[F_HW];
        // dilation of D_{t-1}: left/right in registers (+ the neighbour words), up/down through E_{t-1}
        ring_load5(s_ring, s1, 0, r + 2, wb, e1);  // E_{t-1}, this row (also the last tap's source)
        Dl |= e1[0];
        Dr |= e1[4];
        ring_load5(s_ring, s1, 0, r + 1, wb, nb);  // E_{t-1}, row r-1
#pragma unroll
        for (int i = 0; i < F_HW; ++i) Dup[i] |= nb[i + 1];
        u32 e1d[5];
        ring_load5(s_ring, s1, 0, r + 3, wb, e1d);  // E_{t-1}, row r+1
        bool nonempty = false;
        {
            const u32 dd[5] = {Dl, D[0], D[1], D[2], Dr};
#pragma unroll
            for (int i = 0; i < F_HW; ++i) {
                Ddn[i] |= e1d[i + 1];
                const u32 dil = row_shift<1>(dd + i) | row_shift<-1>(dd + i) | Dup[i] | Ddn[i];
                Et[i] = dil & ~D[i] & M[i];
                taken[i] = ~Et[i];
                nonempty |= Et[i] != 0;
            }
        }
        // forward taps in cv2 order; the candidates are live pixels of levels t-3, t-2, t-1.  tap_step<T, row, levels back>: the
        // last two name what was loaded into its argument and are checked against the table
        ring_load5(s_ring, s3, 1, r + 0, wb, nb);  // L_{t-3}, row r-2
        tap_step<0, -2, 3>(nb, taken, C);
        tap_step<1, -2, 3>(nb, taken, C);
        {
            u32 l3[5], l2[5];
            ring_load5(s_ring, s3, 1, r + 1, wb, l3);  // L_{t-3}, row r-1
            ring_load5(s_ring, s2, 1, r + 1, wb, l2);  // L_{t-2}, row r-1
            ring_load5(s_ring, s1, 1, r + 1, wb, nb);  // L_{t-1}, row r-1
            tap_step<2, -1, 3>(l3, taken, C);
            tap_step<3, -1, 2>(l2, taken, C);
            tap_step<4, -1, 1>(nb, taken, C);
            tap_step<5, -1, 2>(l2, taken, C);
            tap_step<6, -1, 3>(l3, taken, C);
        }
        ring_load5(s_ring, s1, 1, r + 2, wb, l1);  // L_{t-1}, this row
        tap_step<7, 0, 1>(l1, taken, C);
        {
            const u32 m0 = (t & 1) ? 0xFFFFFFFFu : 0u, m1 = (t & 2) ? 0xFFFFFFFFu : 0u, m2 = (t & 4) ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int i = 0; i < F_HW; ++i) {
                Lt[i] = taken[i] & Et[i];
                Lv[i] |= Lt[i];
                P0[i] |= Et[i] & m0;
                P1[i] |= Et[i] & m1;
                P2[i] |= Et[i] & m2;
            }
        }
#pragma unroll
        for (int i = 0; i < F_HW; ++i) D[i] |= Et[i];
        ring_store3(s_ring, sw, 0, r + 2, wb, Et);
        ring_store3(s_ring, sw, 1, r + 2, wb, Lt);
        // Go on while level t produced something (else nothing farther exists either) AND some TILE pixel is
        // still undecided (a chain only runs through smaller distances, so the halo beyond that is not needed;
        // halo pixels near the window edge see fewer sources and would drag the loop towards FR).  One flag
        // word per wave, read after the level's only barrier (__syncthreads_or costs three); double-buffered
        // by level parity: a wave can be at most one level ahead.
        {
            bool open = false;
#pragma unroll
            for (int i = 0; i < F_HW; ++i) open |= (TM[i] & ~D[i]) != 0;
            const u32 flags = (__any(nonempty) ? 1u : 0u) | (__any(open) ? 2u : 0u);
            if ((tid & 63) == 0) s_any[t & 1][tid >> 6] = flags;
            __syncthreads();
            u32 any = 0;
#pragma unroll
            for (int w = 0; w < F_NT / 64; ++w) any |= s_any[t & 1][w];
            return any == 3u;
        }
    };
    for (int t = 1; t <= FR && level(t); ++t) {}
    FPROF(prof.mark(1));
    // ---- P1b: the backward taps of ALL levels in one pass (pixels that are decided but not live).  The d mod 8
    // planes and D go through the ring's memory (slots 0 and 1; its guard rows and pad words are still zero).
    __syncthreads();  // every wave is out of the level loop: the ring is dead
    // (for P2, in the ring's tail that neither the planes below nor s_par use: a byte of a bit plane -> its eight bits in the
    // low bits of eight bytes)
    uint2 *s_lut = reinterpret_cast<uint2 *>(reinterpret_cast<u8 *>(s_ring) + F_WHM * F_P);
    s_lut[tid] = make_uint2((((u32)tid & 15u) * 0x00204081u) & 0x01010101u, (((u32)tid >> 4) * 0x00204081u) & 0x01010101u);
    ring_store3(s_ring, 0, 0, r + 2, wb, P0);
    ring_store3(s_ring, 0, 1, r + 2, wb, P1);
    ring_store3(s_ring, 1, 0, r + 2, wb, P2);
    ring_store3(s_ring, 1, 1, r + 2, wb, D);
    __syncthreads();
    {
        u32 taken[F_HW], a0[5], a1[5], a2[5], dv[5];
#pragma unroll
        for (int i = 0; i < F_HW; ++i) taken[i] = ~(D[i] & ~Lv[i]);  // live = a source or offered by a forward tap
        auto row4 = [&](int row) {
            ring_load5(s_ring, 0, 0, row, wb, a0);
            ring_load5(s_ring, 0, 1, row, wb, a1);
            ring_load5(s_ring, 1, 0, row, wb, a2);
            ring_load5(s_ring, 1, 1, row, wb, dv);
        };
        // the negated cv2 taps, same order; bwd_tap<T, row>: the row that row4 loaded, checked against the table.  Taps 5 and 6
        // are not asked: they never select, and what they match tap 4 has matched before them, so tap 7 sees the same taken
        // mask without them (the proof stands in dtfill_taps.hpp, whose codes 13 and 14 mean source and undecided here).
        row4(r + 4);
        bwd_tap<0, 2>(a0, a1, a2, dv, P0, P1, P2, taken, C);
        bwd_tap<1, 2>(a0, a1, a2, dv, P0, P1, P2, taken, C);
        row4(r + 3);
        bwd_tap<2, 1>(a0, a1, a2, dv, P0, P1, P2, taken, C);
        bwd_tap<3, 1>(a0, a1, a2, dv, P0, P1, P2, taken, C);
        bwd_tap<4, 1>(a0, a1, a2, dv, P0, P1, P2, taken, C);
        row4(r + 2);
        bwd_tap<7, 0>(a0, a1, a2, dv, P0, P1, P2, taken, C);
    }

    // ---- P2: un-slice the code planes of this half row into bytes (2 * plane code), 8 pixels per step: a byte of a plane goes
    // through the table above (one 8-byte LDS read), two shift-ors put it into its bit of the eight bytes.  Undecided pixels
    // (not in D; no tap ever selected them, their planes are 0) get the plane bits of CODE_NONE: F_NONE.
    FPROF(prof.mark(2));
    u8 *s_par = reinterpret_cast<u8 *>(s_ring);
    __syncthreads();  // the ring is dead for everybody before its memory becomes s_par
    {
        u32 *prow = reinterpret_cast<u32 *>(s_par + r * F_P) + wb * 8;
#pragma unroll
        for (int i = 0; i < F_HW; ++i) {
            u32 cj[F_NPLANES];
#pragma unroll
            for (int j = 0; j < F_NPLANES; ++j) cj[j] = ((CODE_NONE >> j) & 1) ? C[j][i] | ~D[i] : C[j][i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u32 lo = 0, hi = 0;
#pragma unroll
                for (int j = 0; j < F_NPLANES; ++j) {
                    const uint2 sp = s_lut[(cj[j] >> (8 * q)) & 0xFFu];
                    lo |= sp.x << (j + 1);
                    hi |= sp.y << (j + 1);
                }
                prow[i * 8 + 2 * q] = lo;
                prow[i * 8 + 2 * q + 1] = hi;
            }
        }
    }
    __syncthreads();
    FPROF(prof.mark(3));

    const bool overflow = fused_walk_epilogue<FR, F_NT, EPI, STREAM>(s_par, s_tab, s_rw, b, H, W, th, tw, r0, c0, wr0, wc0, sh, x, vlist,
                                                        finfo, nval, misaligned, sky0, out_depth, out_dt, out_index, frame_status, ep, rowfar FPROF(, prof));
    if (overflow && (threadIdx.x & 63) == 0) {  // wave-uniform
        // 1: the rows marked in rowflag, 2: the whole frame.  Same-value race: every writer of a frame stores the same value,
        // the any-distance kernels read it after this kernel
        fflag[b] = EPI ? 2 : 1;
        atomicOr(frame_status + b, DTFILL_FRAME_GENERAL_PATH);
    }
    FPROF(prof.mark(6); prof.flush());
}

// k_fused: one launch for both halos.  route (frame_facts): 16 / 32 = the halo that is expected to decide every pixel of
// frame b (source density, runs of source-free rows), 0 = the any-distance kernels take the frame.  The grid is
// sized for the halo-32 tiling (more, smaller tiles); blocks beyond a frame's own tiling exit.  A tile pixel that turns out
// to be farther than the halo from every source is not stored: its ROW is handed to the any-distance kernels (rowflag,
// fflag = 1; frame_status), which redo exactly those rows -- the empty sky of a LiDAR frame, a hole in a dense one.
// fa.ride: no k_frame launch went before.  Every window block works out the facts of its frame itself (frame_facts: one round
// trip for the frame's row counts, then LDS), and the first block of every frame also publishes them for the later launches
// (frame_publish).  No block waits for another.  Else route, finfo, rowbase_s and rowfar are read as k_frame stored them.
// the block's LDS: one buffer, carved here
constexpr size_t F_OFF_RW = (sizeof(u32) * F_RING + 15) & ~(size_t)15, F_OFF_TAB = F_OFF_RW + sizeof(uint2) * F_WHM * 8, F_OFF_ANY = F_OFF_TAB + sizeof(short) * (1 << F_NPLANES),
                 F_LDS_OWN = F_OFF_ANY + sizeof(u32) * 2 * (F_NT / 64);
constexpr size_t F_LDS = F_LDS_OWN;
// frames of up to this many rows can ride: their facts (FrameScratch, then two rank bases per row) lie in the ring's memory
constexpr int F_RIDE_HMAX = (int)((sizeof(u32) * F_RING - sizeof(FrameScratch)) / (2 * sizeof(u32)));
static_assert(sizeof(FrameScratch) % 4 == 0 && F_NT == 256, "frame_facts runs on the window kernel's 256 threads");

template <bool STREAM, bool EPI>
__global__ __launch_bounds__(F_NT, 4) void k_fused(
    const float *__restrict__ x, const u64 *__restrict__ srcbits, const u16 *__restrict__ wpre_s,
    const u32 *__restrict__ rowbase_s, int *__restrict__ finfo, float *vlist /* written here in a frame whose masks differ */,
    int H, int W, int Wd, FusedTiles t16, FusedTiles t32, float *__restrict__ out_depth,
    float *__restrict__ out_dt, int32_t *__restrict__ out_index,
    int *__restrict__ route, int *__restrict__ fflag, u32 *__restrict__ rowfar, int *__restrict__ frame_status, const DepthEpilogue ep,
    const FrameArgs fa) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[F_LDS];
    u32 *s_ring = reinterpret_cast<u32 *>(s_raw);  // later: s_par bytes
    // per window row, the eight image-aligned 32-pixel half words it touches: {source bits, 1 + sources before them
    // in frame raster order} -- one 8-byte LDS read and a 32-bit popcount per rank lookup
    uint2 *s_rw = reinterpret_cast<uint2 *>(s_raw + F_OFF_RW);
    short *s_tab = reinterpret_cast<short *>(s_raw + F_OFF_TAB);  // s_par displacement of a plane code's step (0 for the two reserved codes)
    u32(*s_any)[F_NT / 64] = reinterpret_cast<u32(*)[F_NT / 64]>(s_raw + F_OFF_ANY);  // per wave: did level t produce anything (double-buffered by level parity)
    const int b = blockIdx.x, tile = blockIdx.y;
    int rt, tbase, nval, misaligned, sky0;  // block-uniform
    const u32 *s_bs = nullptr, *s_far = nullptr;
    if (fa.ride) {
        // A block beyond the tiling with fewer tiles (fa.ntmin of them) works only in a frame of the other tiling: most such
        // blocks exit.  They are dispatched long after the frame's first block, which has published the route by then (clear
        // since k_mask): a look at it saves them the facts.  Not seen yet (or not visible here): the facts say the same.
        // ONE look per block: the word changes during this launch, so every wave looking for itself could see something else,
        // and a block must stay or leave whole (thread 0 looks, everybody reads its answer behind a barrier; the slot is not
        // written again before the barriers of frame_facts)
        if (tile >= fa.ntmin) {  // block-uniform
            if (threadIdx.x == 0) s_any[0][0] = (u32)__hip_atomic_load(&route[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const int seen = (int)s_any[0][0];
            const int rs = seen > 0 ? (seen & 0xFF) : 0;
            if (seen != ROUTE_UNKNOWN && !((rs == 16 && tile < t16.ntiles) || (rs == 32 && tile < t32.ntiles))) return;  // block-uniform
        }
        FrameScratch &sc = *reinterpret_cast<FrameScratch *>(s_raw);
        u32 *bs = reinterpret_cast<u32 *>(s_raw + sizeof(FrameScratch)), *bv = bs + H;
        u32 *gs = fa.rowbase_s + (size_t)b * H, *gv = fa.rowbase_v + (size_t)b * H;
        const bool pub = tile == 0;  // the frame's first block also publishes the facts for the later launches
        const FrameFacts ff = frame_facts(fa.rowcnt_s + (size_t)b * H, fa.rowcnt_v + (size_t)b * H, H, W, fa.mode, fa.nty16, fa.nty32, sc, pub,
                                          [&](int i, u32 base_s, u32 base_v) {
                                              bs[i] = base_s;
                                              bv[i] = base_v;
                                              if (pub) {
                                                  gs[i] = base_s;
                                                  gv[i] = base_v;
                                              }
                                          });
        // The two masks of the frame differ somewhere (rare): its depths are gathered from the value list, which the
        // frame's first block writes in this very launch -- and no block waits for another.  So every working window
        // block of such a frame writes the whole list itself first (the same values from every writer).  Its own stores
        // are visible to its gathers: the barrier in front of the ring's zeroing lies between them.
        if (pub)
            frame_publish(ff, sc, b, fa.x, fa.valbits, fa.wpre_v, fa.srcbits, fa.wpre_s, fa.ptslist, H, W, Wd, gs, gv, finfo, vlist,
                          fflag, route, frame_status, fa.mode, fa.negflag, rowfar, true);
        else if (ff.misaligned && out_depth && ((ff.r == 16 && tile < t16.ntiles) || (ff.r == 32 && tile < t32.ntiles)))
            value_list(b, fa.x, fa.valbits, fa.wpre_v, H, W, Wd, vlist, [&](int i) { return bv[i]; });
        auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
        rt = uni(ff.route);
        tbase = uni(ff.tr0);
        nval = uni(ff.nval);
        misaligned = uni(ff.misaligned);
        sky0 = uni(ff.sky);
        s_bs = bs;
        s_far = sc.far[ff.plane];
    } else {
        rt = route[b];
        tbase = finfo[b * FI_STRIDE + FI_TR0];
        nval = finfo[b * FI_STRIDE + FI_NVAL];
        misaligned = finfo[b * FI_STRIDE + FI_MISALIGNED];
        sky0 = finfo[b * FI_STRIDE + FI_SKY] & ~SKY_OFF;  // (another block may have called the sky off already)
    }
    if (rt == ROUTE_POINTS) return;  // a frame with a handful of sources: k_pts's tiles ride in k_fin's launch (dtfill_pts.hpp)
    const int r = rt > 0 ? (rt & 0xFF) : 0;
    const bool pre = rt > 0 && (rt & ROUTE_PREMARK);
    // EPI (a depth epilogue: ep.row0 != 0 || ep.use_floor) is chosen on the host: the plain pass runs code compiled without it
#define FUSED_CALL(FR_, T_)                                                                                        \
    fused_body<FR_, EPI, STREAM>(tile, pre, tbase, nval, misaligned, sky0, s_bs, s_far, x, srcbits, wpre_s, rowbase_s, finfo, vlist, H, W, Wd, T_.nty, T_.TW, T_.tiles_x, out_depth, out_dt, \
                          out_index, fflag, rowfar, frame_status, ep, s_ring, s_rw, s_tab, s_any)
    if (r == 16 && tile < t16.ntiles)
        FUSED_CALL(16, t16);
    else if (r == 32 && tile < t32.ntiles)
        FUSED_CALL(32, t32);
#undef FUSED_CALL
}

// dtfill_prepass.hpp -- k_mask, k_frame: bit words, compaction ranks, frame facts (every pass starts with these)
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// k_mask: source predicate exactly as tools.py:8, mask = (1.0 - x) > thr (1 = fill, 0 = source); value predicate as
// tools.py:22, x > thr.  Per 64-pixel word: the two bit words and the row-local exclusive popcount; per row: totals (+ "masks
// differ" in bit 31), and the row's and the frame's per-pass flags cleared.
//   k_mask_plain (below mask_body): the pass without the outlier filter; a word is the lane mask of a compare.
//   k_mask<OM, VEC>, OM = 1, 2: outlier_removal() in front of the predicates, one wave per image row.  A row is read in chunks
//   of 256 pixels = four words, a batch of chunks in flight:
//     VEC (W % 4 == 0, 16-byte aligned frames): a lane reads 4 consecutive pixels in one load; its four predicate bits form a
//          nibble, and the 16 lanes of a DPP row combine theirs into one word.
//     !VEC: a lane reads pixel 64 q + lane of each of the chunk's four words q; word q is a ballot.
//   Either way the 16 lanes of group lane >> 4 hold word lane >> 4 of the chunk.
// ------------------------------------------------------------------------------------------------
constexpr int M4_NC = 8;  // 256-pixel chunks per batch (2048 pixels) with 16-byte loads
constexpr int M1_NC = 2;  // ... with dword loads

template <int CTRL>
__device__ __forceinline__ u32 dpp_or(u32 v) {  // v | v of the lane CTRL pairs it with (inside a row of 16)
    return v | (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// the 64-pixel word of this lane's 16-lane row from the lanes' nibbles (lane i of the row owns bits 4i..4i+3)
__device__ __forceinline__ u64 row_word(u32 nib, int lane) {
    u32 part = nib << (4 * (lane & 7));  // lanes 0-7 of the row build the low half, lanes 8-15 the high half
    part = dpp_or<0xB1>(part);           // quad_perm [1,0,3,2]
    part = dpp_or<0x4E>(part);           // quad_perm [2,3,0,1]
    part = dpp_or<0x141>(part);          // row_half_mirror: now every lane has its half-row's 32 bits
    const u32 other = (u32)__builtin_amdgcn_update_dpp(0, (int)part, 0x140, 0xF, 0xF, false);  // row_mirror
    return (lane & 8) ? ((u64)part << 32 | other) : ((u64)other << 32 | part);
}
// pixel q of the lane in a chunk, counted from the chunk's first pixel
template <bool VEC>
__device__ __forceinline__ int chunk_px(int q, int lane) { return VEC ? 4 * lane + q : 64 * q + lane; }
// word lane >> 4 of the chunk from the lanes' predicate bits (bit q: pixel chunk_px(q, lane))
template <bool VEC>
__device__ __forceinline__ u64 chunk_word(u32 nib, int lane) {
    if (VEC) return row_word(nib, lane);
    u64 w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u64 bq = __ballot((nib >> q) & 1u);
        w = (lane >> 4) == q ? bq : w;
    }
    return w;
}
// bit q: pixel chunk_px(q, lane) of the batch's chunk u is removed (s_drop: one bit per pixel of the batch)
template <bool VEC>
__device__ __forceinline__ u32 drop_bits(const u32 *s_drop, int u, int lane) {
    if (VEC) return s_drop[(u << 3) + (lane >> 3)] >> ((4 * lane) & 31);  // the lane's four pixels are adjacent bits of one word
    u32 d = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) d |= ((s_drop[(u << 3) + 2 * q + (lane >> 5)] >> (lane & 31)) & 1u) << q;
    return d;
}

// outlier_removal() (data_read.py:103-128) in front of the predicates, see dtfill_outlier.hpp: the candidates of the
// batch's pixels in registers (v > 1.0; every pixel when OM == 2) are listed in LDS, one lane each gathers a candidate's 25 taps,
// and the pixels it removes read as 0.0f below.  OM == 1 raises negflag[b] on a negative value, the OM == 2 launch redoes
// exactly those frames.
template <int OM, bool VEC>
__device__ __forceinline__ void mask_body(const float *__restrict__ x, int H, int W, int Wd, float src_thr, float val_thr,
                                          u64 *__restrict__ srcbits, u64 *__restrict__ valbits, u16 *__restrict__ wpre_s,
                                          u16 *__restrict__ wpre_v, u32 *__restrict__ rowcnt_s, u32 *__restrict__ rowcnt_v,
                                          int *__restrict__ negflag, u32 *__restrict__ rowfar, int *__restrict__ fflag2,
                                          int *__restrict__ frame_status, int *__restrict__ finfo, int *__restrict__ route, bool clear) {
    static_assert(OM == 1 || OM == 2, "the pass without the filter is k_mask_plain");
    __shared__ u16 s_list[4][M4_NC * 256];
    __shared__ u32 s_drop[4][M4_NC * 8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (frames along grid x: with a batch of a multiple of eight frames a frame's rows are one XCD's, where the window kernel's blocks of
    // that frame will look for its bit words)
    const int i = blockIdx.y * 4 + wave, b = blockIdx.x;
    if (i >= H) return;
    if (OM == 2 && !negflag[b]) return;
    bool neg = false;
    const int w_in_chunk = lane >> 4;  // which of the chunk's four words this lane's row builds
    const int nchunk = (W + 255) >> 8;
    constexpr int NC = VEC ? M4_NC : M1_NC;
    const float *row = x + ((size_t)b * H + i) * W;
    const size_t wrow = ((size_t)b * H + i) * Wd;
    u32 run_s = 0, run_v = 0, mis = 0;  // wave-uniform
    for (int c0 = 0; c0 < nchunk; c0 += NC) {
        float4 v[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int px = ((c0 + u) << 8) + chunk_px<VEC>(0, lane);
            if (VEC) {
                v[u] = (c0 + u < nchunk && px < W) ? reinterpret_cast<const float4 *>(row)[px >> 2] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {  // W % 4 != 0 may split a lane's pixels: every pixel is tested
                float f[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) f[q] = (c0 + u < nchunk && px + 64 * q < W) ? row[px + 64 * q] : 0.0f;
                v[u] = make_float4(f[0], f[1], f[2], f[3]);
            }
        }
        if (lane < M4_NC * 8) s_drop[wave][lane] = 0u;
        int n = 0;  // wave-uniform
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            if (c0 + u >= nchunk) break;
            const float f[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = ((c0 + u) << 8) + chunk_px<VEC>(VEC ? 0 : q, lane) < W;
                neg |= in && f[q] < 0.0f;
                const bool cand = in && (OM == 2 || f[q] > 1.0f);
                const u64 bal = __ballot(cand);
                if (cand) s_list[wave][n + (int)__builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u))] = (u16)((u << 8) + chunk_px<VEC>(q, lane));
                n += __popcll(bal);
            }
        }
        __builtin_amdgcn_wave_barrier();
        const float *xf = x + (size_t)b * H * W;
        for (int t = lane; t < n; t += 64) {
            const int jr = s_list[wave][t], j = (c0 << 8) + jr;
            const bool drop = is_outlier([&](int ti, int tj) {
                return xf[(size_t)reflect101(i + ti - 3, H) * W + reflect101(j + tj - 3, W)];  // neighbouring rows: cache hits
            });
            if (drop) atomicOr(&s_drop[wave][jr >> 5], 1u << (jr & 31));
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            if (c0 + u >= nchunk) break;  // wave-uniform
            float f[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            const u32 d = drop_bits<VEC>(s_drop[wave], u, lane);
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = ((d >> q) & 1u) ? 0.0f : f[q];
            u32 ns = 0, nv = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = ((c0 + u) << 8) + chunk_px<VEC>(VEC ? 0 : q, lane) < W;  // VEC: a lane's four pixels are inside or outside together
                ns |= (in && !((1.0f - f[q]) > src_thr)) ? (1u << q) : 0u;
                nv |= (in && (f[q] > val_thr)) ? (1u << q) : 0u;
            }
            const u64 ws = chunk_word<VEC>(ns, lane), wv = chunk_word<VEC>(nv, lane);
            const u32 cs = (u32)__popcll(ws), cv = (u32)__popcll(wv);
            // counts of the chunk's four words (every lane of a row holds its word's count)
            const u32 s0 = __builtin_amdgcn_readlane(cs, 0), s1 = __builtin_amdgcn_readlane(cs, 16),
                      s2 = __builtin_amdgcn_readlane(cs, 32), s3 = __builtin_amdgcn_readlane(cs, 48);
            const u32 v0 = __builtin_amdgcn_readlane(cv, 0), v1 = __builtin_amdgcn_readlane(cv, 16),
                      v2 = __builtin_amdgcn_readlane(cv, 32), v3 = __builtin_amdgcn_readlane(cv, 48);
            const u32 pre_s = run_s + (w_in_chunk > 0 ? s0 : 0u) + (w_in_chunk > 1 ? s1 : 0u) + (w_in_chunk > 2 ? s2 : 0u);
            const u32 pre_v = run_v + (w_in_chunk > 0 ? v0 : 0u) + (w_in_chunk > 1 ? v1 : 0u) + (w_in_chunk > 2 ? v2 : 0u);
            mis |= __any(ws != wv) ? 1u : 0u;
            const int k = ((c0 + u) << 2) + w_in_chunk;  // word index in the row
            if ((lane & 15) == 0 && k < Wd) {             // one lane per word: four adjacent words per store
                srcbits[wrow + k] = ws;
                valbits[wrow + k] = wv;
                wpre_s[wrow + k] = (u16)pre_s;
                wpre_v[wrow + k] = (u16)pre_v;
            }
            run_s += s0 + s1 + s2 + s3;
            run_v += v0 + v1 + v2 + v3;
        }
    }
    if (lane == 0) {
        rowcnt_s[(size_t)b * H + i] = run_s;
        rowcnt_v[(size_t)b * H + i] = run_v | (mis ? 0x80000000u : 0u);
        // clear (a pass whose frame facts are worked out in k_fused's launch): what the frame's publishing block
        // (frame_publish) and the window blocks both raise in that one launch starts clear here: the row flags, the frame's
        // any-distance flag, its status, "the sky is called off" and the route.  The raisers only ever set bits.  (With a
        // k_frame launch of its own that kernel stores all of them, as it always did.)
        if (clear) rowfar[(size_t)b * H + i] = 0u;
        if (clear && i == 0) {
            fflag2[b] = 0;
            frame_status[b] = DTFILL_FRAME_OK;
            finfo[b * FI_STRIDE + FI_SKY] = 0;
            route[b] = ROUTE_UNKNOWN;  // (k_fused's late blocks look at it before the facts are published)
        }
    }
    if (OM == 1 && __any(neg) && lane == 0) negflag[b] = 1;  // this frame is redone by the exhaustive launch
}
template <int OM, bool VEC>
__global__ __launch_bounds__(256) void k_mask(const Pass p) {
    mask_body<OM, VEC>(p.x, p.H, p.W, p.Wd, p.src_thr, p.val_thr, p.srcbits, p.valbits, p.wpre_s, p.wpre_v, p.rowcnt_s, p.rowcnt_v,
                       p.negflag, p.rowfar, p.fflag2, p.status, p.finfo, p.route, p.ride != 0);
}

// v with lane K's value replaced by the wave-uniform s
template <int K>
__device__ __forceinline__ u32 lane_set(u32 v, u32 s) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(K));
    return v;
}
// f(integral_constant<int, K>) for every K: the lane of lane_set is an immediate
template <class F, int... K>
__device__ __forceinline__ void for_words(std::integer_sequence<int, K...>, F f) {
    (f(std::integral_constant<int, K>{}), ...);
}
// The plain pass (no outlier filter): a lane reads pixel 64 k + lane of word k, so the compare's 64-bit result IS the bit word:
// the word's count is a scalar popcount, the row-local prefix a scalar sum, "the masks differ" a scalar xor.  Lane k of the
// wave collects word k of a batch of MW_NW words (the batch's loads are all in flight before the first compare) and stores it
// with its two prefixes: four stores per batch.  Any W, any alignment: the partial last word of a row is loaded and stored
// apart.  A frame's waves (4 gridDim.y of them) share its rows evenly, wave g takes the rows [g H / n, (g + 1) H / n):
// launch_mask gives a wave the rows that fill one batch.  (8 waves a SIMD are asked for: left alone the compiler keeps 101 SGPRs, 7 waves.)
constexpr int MW_NW = 20;  // 64-pixel words per batch (a KITTI row; 1280 pixels in flight)
__global__ __launch_bounds__(256, 8) void k_mask_plain(const Pass p) {
    const float *__restrict__ x = p.x;
    const int H = p.H, W = p.W, Wd = p.Wd;  // (Wd = nfull, + 1 with a partial last word)
    const float src_thr = p.src_thr, val_thr = p.val_thr;
    const bool clear = p.ride != 0;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (frames along grid x: see mask_body)
    const int b = blockIdx.x;
    const u32 nwave = gridDim.y * 4u, g = blockIdx.y * 4u + (u32)wave;  // (nwave <= H + 3 <= 2^13: the products fit)
    const int i1 = (int)((g + 1u) * (u32)H / nwave);
    const int nfull = W >> 6;
    const u64 tail = (1ull << (W & 63)) - 1ull;
    for (int i = (int)(g * (u32)H / nwave); i < i1; ++i) {
        const float *row = x + ((size_t)b * H + i) * W;
        const size_t wrow = ((size_t)b * H + i) * Wd;
        u32 run_s = 0, run_v = 0;  // wave-uniform
        u64 mis = 0;
        float vt = 0.0f;  // the partial last word of the row (word nfull), on its way with the first batch
        if (lane < (W & 63)) vt = row[(nfull << 6) + lane];
        for (int k0 = 0; k0 < nfull; k0 += MW_NW) {  // the full words
            float v[MW_NW];
#pragma unroll
            for (int k = 0; k < MW_NW; ++k)
                if (k0 + k < nfull) v[k] = row[((k0 + k) << 6) + lane];  // wave-uniform
            u32 s_lo = 0, s_hi = 0, v_lo = 0, v_hi = 0, pre_s = 0, pre_v = 0;  // lane k: word k0 + k
            for_words(std::make_integer_sequence<int, MW_NW>{}, [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if (k0 + k >= nfull) return;  // wave-uniform
                const u64 ws = __ballot(!((1.0f - v[k]) > src_thr)), wv = __ballot(v[k] > val_thr);
                s_lo = lane_set<k>(s_lo, (u32)ws);
                s_hi = lane_set<k>(s_hi, (u32)(ws >> 32));
                v_lo = lane_set<k>(v_lo, (u32)wv);
                v_hi = lane_set<k>(v_hi, (u32)(wv >> 32));
                pre_s = lane_set<k>(pre_s, run_s);
                pre_v = lane_set<k>(pre_v, run_v);
                run_s += (u32)__popcll(ws);
                run_v += (u32)__popcll(wv);
                mis |= ws ^ wv;
            });
            const int k = k0 + lane;
            if (lane < MW_NW && k < nfull) {
                p.srcbits[wrow + k] = (u64)s_hi << 32 | s_lo;
                p.valbits[wrow + k] = (u64)v_hi << 32 | v_lo;
                p.wpre_s[wrow + k] = (u16)pre_s;
                p.wpre_v[wrow + k] = (u16)pre_v;
            }
        }
        if (W & 63) {  // the pixels at or beyond W are no source and no value
            const u64 ws = __ballot(!((1.0f - vt) > src_thr)) & tail, wv = __ballot(vt > val_thr) & tail;
            if (lane == 0) {
                p.srcbits[wrow + nfull] = ws;
                p.valbits[wrow + nfull] = wv;
                p.wpre_s[wrow + nfull] = (u16)run_s;
                p.wpre_v[wrow + nfull] = (u16)run_v;
            }
            run_s += (u32)__popcll(ws);
            run_v += (u32)__popcll(wv);
            mis |= ws ^ wv;
        }
        if (lane == 0) {
            p.rowcnt_s[(size_t)b * H + i] = run_s;
            p.rowcnt_v[(size_t)b * H + i] = run_v | (mis ? 0x80000000u : 0u);
            // clear: as mask_body
            if (clear) p.rowfar[(size_t)b * H + i] = 0u;
            if (clear && i == 0) {
                p.fflag2[b] = 0;
                p.status[b] = DTFILL_FRAME_OK;
                p.finfo[b * FI_STRIDE + FI_SKY] = 0;
                p.route[b] = ROUTE_UNKNOWN;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The frame facts: everything a pass decides per frame, a pure function of the frame's row counts (k_mask), H, W, mode and
// the two tilings' tile rows.  Exclusive scan of the row counts = raster rank of the first source / value pixel of every row:
// cv2's label init (k=1; every zero pixel gets k++) and numpy's boolean compaction x[with_value] (tools.py:24).
//   frame_facts    works them out for a block of 256 threads and leaves the row structure in LDS (FrameScratch); every
//                  row's two rank bases go to the caller's sink.  Called by the block that publishes a frame (k_frame, or
//                  the first block of the frame in k_fused's launch) and by every window block of k_fused for its own frame: ONE
//                  definition, so a window block and the published state always agree.
//   frame_publish  stores what later launches read: finfo, route, the row flags, fflag2, the frame status, the source list
//                  of a k_pts frame, the value list when the two masks of a frame differ somewhere.  The row flags, fflag2,
//                  the status and FI_SKY start clear (k_mask) and are only raised here: the window blocks of the same
//                  launch raise them too.
// ------------------------------------------------------------------------------------------------
struct FrameScratch {
    u32 empty[256];   // bit i: row i holds no source (the rows past H count as empty)
    u32 far[2][256];  // bit i: row i >= r0 and vd(i) > PM16 / > PM32; after the tile-row culling: the chosen halo's pre-marked rows
    u16 ptrow[L2_PTS_MAX];  // rows that hold a source (for the source list of a k_pts frame)
    u32 ws[2][4], wv[2][4];  // the waves' totals of a batch of 256 rows, double-buffered by batch parity: one barrier per batch
    int mis, dlb, nfar[2], r0, bandmax, nrow;
};
struct FrameFacts {
    int r;           // the route without ROUTE_PREMARK: 16, 32, 0 or ROUTE_POINTS
    int route;       // ... as route[b] holds it
    int r0;          // the first row that holds a source (H: none)
    int sky;         // rows [0, sky) are k_sky's (0: none)
    int tr0;         // the first row of the window kernel's tiling
    int nsrc, nval, misaligned, dlb;
    int plane;       // which of FrameScratch::far holds the frame's pre-marked rows
    bool flags, sky_ok, any1, anygone;
    // the row flag of row i (l1_cv: 0 = the window kernel's, 1 = the any-distance kernels', 2 = k_sky's; l2: L2_ROW_GONE)
    __device__ __forceinline__ u32 rowflag(const FrameScratch &sc, int i, bool l2) const {
        const u32 farbit = (sc.far[plane][i >> 5] >> (i & 31)) & 1u;
        u32 f = 0u;
        if (flags && r > 0) f = i < r0 && sky_ok ? (sky ? 2u : 1u) : farbit;
        if (l2 && r > 0 && farbit) f = L2_ROW_GONE;  // (a frame without sources is not routed to a window)
        return f;
    }
};

// cs_, cv_: the frame's row counts; sink(i, bs, bv): the rank bases of row i < H; list: the rows that hold a source are wanted
// in sc.ptrow / sc.nrow (the publishing block's, for the source list of a k_pts frame)
template <class Sink>
__device__ __forceinline__ FrameFacts frame_facts(const u32 *__restrict__ cs_, const u32 *__restrict__ cv_, int H, int W, int mode,
                                                  int nty16, int nty32, FrameScratch &sc, bool list, Sink sink) {
    const bool l2 = mode & FM_L2, premark = mode & FM_PREMARK;  // (the mode bits: dtfill_route.hpp)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hp = (H + 63) & ~63;
    // the counts of the first 256 rows are on their way before anything else; every later batch while the one before is scanned
    u32 ncs = tid < H ? cs_[tid] : 0u, ncv = tid < H ? cv_[tid] : 0u;
    if (tid == 0) {
        sc.mis = 0;
        sc.dlb = 0;
        sc.r0 = H;
        sc.bandmax = 0;
        sc.nrow = 0;
    }
    if (tid < 2) sc.nfar[tid] = 0;
    for (int w = tid + (Hp >> 5); w < 256; w += 256) sc.empty[w] = 0xFFFFFFFFu;
    __syncthreads();
    u32 run_s = 0, run_v = 0;
    int mis = 0;
    for (int base = 0; base < Hp; base += 256) {
        const int i = base + tid;
        u32 cs = ncs, cv = ncv;
        ncs = i + 256 < H ? cs_[i + 256] : 0u;
        ncv = i + 256 < H ? cv_[i + 256] : 0u;
        mis |= (int)(cv >> 31);
        cv &= 0x7FFFFFFFu;
        {
            // the same pass over the row counts: "row has no source" as bits (a wave holds 64 consecutive rows: two whole words per
            // ballot, no atomics), the first row with a source, the most sources in a band of 32 rows (k_pts's tiles are that high)
            const u64 has = __ballot(cs != 0u), bal = ~has;
            if (lane == 0 && i < Hp) {
                sc.empty[i >> 5] = (u32)bal;
                sc.empty[(i >> 5) + 1] = (u32)(bal >> 32);
                if (has) atomicMin(&sc.r0, i + __ffsll((long long)has) - 1);
            }
            // ... and the rows that hold a source, listed (in any order; at most L2_PTS_MAX matter: a frame with more of them
            // is no k_pts frame)
            if (list) {  // block-uniform
                int at = 0;
                if (lane == 0 && has) at = atomicAdd(&sc.nrow, __popcll(has));
                at = __builtin_amdgcn_readfirstlane(at) + (int)__builtin_amdgcn_mbcnt_hi((u32)(has >> 32), __builtin_amdgcn_mbcnt_lo((u32)has, 0u));
                if (cs != 0u && at < L2_PTS_MAX) sc.ptrow[at] = (u16)i;
            }
        }
        u32 is = cs, iv = cv;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            u32 ts = __shfl_up(is, off), tv = __shfl_up(iv, off);
            if (lane >= off) {
                is += ts;
                iv += tv;
            }
        }
        {
            // the two bands of 32 rows a wave holds, off the inclusive scan: lanes 0..31 end in lane 31, the rest is the other band
            const u32 half = (u32)__shfl((int)is, 31);
            if (lane == 31 && is) atomicMax(&sc.bandmax, (int)is);
            if (lane == 63 && is != half) atomicMax(&sc.bandmax, (int)(is - half));
        }
        const int par = (base >> 8) & 1;
        if (lane == 63) {
            sc.ws[par][wave] = is;
            sc.wv[par][wave] = iv;
        }
        __syncthreads();
        u32 ps = 0, pv = 0, ts = 0, tv = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) {
                ps += sc.ws[par][k];
                pv += sc.wv[par][k];
            }
            ts += sc.ws[par][k];
            tv += sc.wv[par][k];
        }
        if (i < H) sink(i, run_s + ps + is - cs, run_v + pv + iv - cv);
        run_s += ts;
        run_v += tv;
    }
    if (mis) atomicOr(&sc.mis, 1);
    // Row structure of the frame (r0, vd(i), the far rows: dtfill_route.hpp says what they decide): the rows above r0 get
    // flag 2 when they are k_sky's, a far row flag 1; max vd = lower bound of the largest distance in the frame (FI_DLB).
    // "Row has no source" as bits in LDS (H <= 8191 -> 256 words); the rows past H count as empty.
    // (a frame in which every row holds a source -- the common dense one -- has vd = 0 everywhere: nothing to search)
    bool someempty = false;
    for (int w = tid; w <= (H - 1) >> 5; w += 256) someempty |= (sc.empty[w] & (w == (H - 1) >> 5 ? (2u << ((H - 1) & 31)) - 1u : 0xFFFFFFFFu)) != 0u;
    someempty = __syncthreads_or(someempty);
    if (!someempty) {
        sc.far[0][tid] = sc.far[1][tid] = 0u;
    } else {
        int dlb = 0;
        const int lastw = (H - 1) >> 5, r0 = sc.r0;
        for (int base = 0; base < Hp; base += 256) {
            const int i = base + tid;
            int vd = 0;
            if (i < H) {
                int up = BIG, dn = BIG;  // distance to the nearest row with a source at or above / at or below row i
                {
                    int w = i >> 5;
                    u32 m = ~sc.empty[w] & ((2u << (i & 31)) - 1u);
                    while (!m && w > 0) m = ~sc.empty[--w];
                    if (m) up = i - (w * 32 + 31 - __clz((int)m));
                }
                {
                    int w = i >> 5;
                    u32 m = ~sc.empty[w] & ~((1u << (i & 31)) - 1u);
                    while (!m && w < lastw) m = ~sc.empty[++w];
                    if (m) dn = w * 32 + __ffs((int)m) - 1 - i;
                }
                vd = min(up, dn);
                dlb = max(dlb, vd);
            }
            const u64 f16 = __ballot(i < H && far_row(l2, 16, i, r0, vd)), f32 = __ballot(i < H && far_row(l2, 32, i, r0, vd));
            if (lane == 0 && i < Hp) {
                sc.far[0][i >> 5] = (u32)f16;
                sc.far[0][(i >> 5) + 1] = (u32)(f16 >> 32);
                sc.far[1][i >> 5] = (u32)f32;
                sc.far[1][(i >> 5) + 1] = (u32)(f32 >> 32);
                if (f16) atomicAdd(&sc.nfar[0], __popcll(f16));
                if (f32) atomicAdd(&sc.nfar[1], __popcll(f32));
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) dlb = max(dlb, __shfl_xor(dlb, o));
        if (lane == 0 && dlb) atomicMax(&sc.dlb, dlb);
    }
    __syncthreads();
    FrameFacts ff;
    ff.misaligned = sc.mis;
    ff.dlb = sc.dlb;
    ff.nsrc = (int)run_s;
    ff.nval = (int)run_v;
    const int r0 = ff.r0 = sc.r0;
    const bool sky_ok = ff.sky_ok = sky_possible(premark, r0, H);
    // which kernel family takes the frame (every thread for itself, from what the barrier above made visible: no thread waits
    // for another's decision)
    const int r = ff.r = route_decide(RouteIn{H, W, mode, ff.nsrc, ff.dlb, sc.bandmax, sc.nfar[0], sc.nfar[1], r0, sky_ok});
    const bool flags = ff.flags = !l2 && premark && r >= 0;  // this frame's rows carry flags
    // k_sky starts from rows r0 and r0 + 1 as the window kernel leaves them (it runs beside the first any-distance kernel): a
    // frame that is not a window kernel's, or whose row r0 / r0 + 1 is handed on up front, keeps its sky with the other rows
    bool sky = sky_ok && r > 0;
    ff.plane = r == 32 ? 1 : 0;
    u32 *far = sc.far[ff.plane];
    ff.any1 = false;
    // (a frame in which every row holds a source has no far row, no sky and nothing to cull)
    if (someempty) {  // block-uniform
    if (flags && r > 0) {
        // a tile row of the window kernel that is left with only a few rows is not worth its windows: all of it goes to the
        // any-distance kernels.  One thread per tile row, whole words at a time.
        // the window kernel's tile rows: nty of them over the rows from the first source row on when the rows above are the
        // sky's, else over the whole frame (fused_body takes the same tile_row_height)
        const int nty = r == 16 ? nty16 : nty32, tbase = sky_ok ? r0 : 0;
        const int TH = tile_row_height(H, tbase, nty);
        auto bits = [&](int a, int e, int w) {  // the rows [a, e) as bits of word w
            const int lo = max(a - 32 * w, 0), hi = min(e - 32 * w, 32);
            return hi <= lo ? 0u : (hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
        };
        for (int t = tid; tbase + t * TH < H; t += 256) {
            const int a = tbase + t * TH, e = min(H, tbase + (t + 1) * TH);  // its rows (all below the sky)
            int keep = 0;
            for (int w = a >> 5; w <= (e - 1) >> 5 && a < e; ++w) keep += __popc(~far[w] & bits(a, e, w));
            if (tile_row_culled(keep, e - a))
                for (int w = a >> 5; w <= (e - 1) >> 5; ++w) atomicOr(&far[w], bits(a, e, w));
        }
    }
    __syncthreads();
    if (sky && (((far[r0 >> 5] >> (r0 & 31)) & 1u) || (r0 + 1 < H && ((far[(r0 + 1) >> 5] >> ((r0 + 1) & 31)) & 1u)))) sky = false;
    // some row carries flag 1: the rows above r0 when their sky is not k_sky's, or a pre-marked row (far holds no bit of a
    // row above r0 then, and none of a row past H ever)
    bool one = false;
    if (flags && r > 0) {
        one = sky_ok && !sky;
        for (int w = tid; w <= (H - 1) >> 5; w += 256) one |= far[w] != 0u;
    }
    ff.any1 = __syncthreads_or(one);
    }
    ff.sky = (flags && sky) ? r0 : 0;
    ff.tr0 = (flags && r > 0 && sky_ok) ? r0 : 0;
    ff.anygone = l2 && r > 0 && sc.nfar[ff.plane] > 0;  // l2: rows for k_colT + k_l2env from the start
    const bool marked = flags && r > 0 && (ff.sky > 0 || ff.any1);
    ff.route = marked ? (r | ROUTE_PREMARK) : r;
    return ff;
}

// The compacted value list of a frame whose two masks differ somewhere (rare): x at the value pixels, in raster order.
// bv(i): the rank base of row i's values.  One block of 256 threads writes the whole list.
template <class Base>
__device__ __forceinline__ void value_list(int b, const float *__restrict__ x, const u64 *__restrict__ valbits,
                                           const u16 *__restrict__ wpre_v, int H, int W, int Wd, float *__restrict__ vlist, Base bv) {
    const float *xf = x + (size_t)b * H * W;
    float *vl = vlist + (size_t)b * H * W;
    const int nwords = H * Wd;
    for (int w = threadIdx.x; w < nwords; w += 256) {
        u64 vb = valbits[(size_t)b * nwords + w];
        const int i = w / Wd, j0 = (w - i * Wd) * 64;
        u32 k = bv(i) + wpre_v[(size_t)b * nwords + w];
        while (vb) {
            const int bit = __ffsll((long long)vb) - 1;
            vb &= vb - 1;
            vl[k++] = xf[(size_t)i * W + j0 + bit];
        }
    }
}

// what the later launches read of frame b (bs_: the frame's rowbase_s, which this block's sink has stored before a barrier)
__device__ __forceinline__ void frame_publish(const FrameFacts &ff, const FrameScratch &sc, int b, const float *__restrict__ x,
                                              const u64 *__restrict__ valbits, const u16 *__restrict__ wpre_v,
                                              const u64 *__restrict__ srcbits, const u16 *__restrict__ wpre_s,
                                              PtsSrc *__restrict__ ptslist, int H, int W, int Wd, const u32 *bs_, const u32 *bv_,
                                              int *__restrict__ finfo, float *__restrict__ vlist, int *__restrict__ fflag2,
                                              int *__restrict__ route, int *__restrict__ frame_status, int mode,
                                              int *__restrict__ negflag, u32 *__restrict__ rowfar, bool raise) {
    // raise: the window blocks of this very launch raise rowfar, fflag2, the status and FI_SKY's SKY_OFF bit too (all clear since k_mask):
    // only what is non-zero is stored, flags by atomicOr.  Else (k_frame) every word is stored.
    const bool l2 = mode & FM_L2;
    const int tid = threadIdx.x, r = ff.r;
    // the route first: k_fused's late blocks look at it (they exit at once in a frame that is not their tiling's)
    if (tid == 0) __hip_atomic_store(&route[b], ff.route, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!l2 && r == ROUTE_POINTS) {
        // the frame's sources in raster order (index = label - 1), for k_pts
        PtsSrc *list = ptslist + (size_t)b * L2_PTS_MAX;
        const float *xf = x + (size_t)b * H * W;
        // an item = one 64-pixel word of a row that holds a source (the rows were listed above); a word's sources go to their
        // raster ranks.  Eight items per step, and everything an item needs before its depths is loaded at once (this block alone
        // works on the frame: the chain of dependent loads is what the step costs)
        constexpr int NQ = 8;
        const int nitems = min(sc.nrow, L2_PTS_MAX) * Wd;
        for (int it0 = tid; it0 < nitems; it0 += 256 * NQ) {
            u64 sb[NQ];
            u32 k[NQ];
            int row[NQ], w[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int it = min(it0 + 256 * q, nitems - 1);
                row[q] = sc.ptrow[it / Wd];
                w[q] = it % Wd;
                const size_t at = ((size_t)b * H + row[q]) * Wd + w[q];
                sb[q] = it0 + 256 * q < nitems ? srcbits[at] : 0ull;
                k[q] = bs_[row[q]] + wpre_s[at];  // (this block wrote bs_ before a barrier)
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                u64 m = sb[q];
                while (m) {
                    const int j = w[q] * 64 + __ffsll((long long)m) - 1;
                    m &= m - 1;
                    list[k[q]++] = PtsSrc{(u32)row[q] << 16 | (u32)j, xf[(size_t)row[q] * W + j]};  // ... with its depth
                }
            }
        }
    }
    // per row: l1_cv: 0 = the window kernel's, 1 = the any-distance kernels' (pre-marked here, or set by k_fused when it meets
    // a pixel farther than its halo), 2 = k_sky's; l2: far pixels k_l2win counted.  (Clear since k_mask.)
    for (int i = tid; i < H; i += 256) {
        const u32 f = ff.rowflag(sc, i, l2);
        if (f || !raise) rowfar[(size_t)b * H + i] = f;  // (1: the window kernel may store the same)
    }
    if (tid == 0) {
        finfo[b * FI_STRIDE + FI_NSRC] = ff.nsrc;
        finfo[b * FI_STRIDE + FI_NVAL] = ff.nval;
        finfo[b * FI_STRIDE + FI_MISALIGNED] = ff.misaligned;
        finfo[b * FI_STRIDE + FI_DLB] = ff.dlb;
        finfo[b * FI_STRIDE + FI_NUNRES] = 0;
        if (!raise)
            finfo[b * FI_STRIDE + FI_SKY] = ff.sky;
        else if (ff.sky)
            atomicOr(&finfo[b * FI_STRIDE + FI_SKY], ff.sky);
        finfo[b * FI_STRIDE + FI_TR0] = ff.tr0;
        negflag[b] = 0;  // k_mask's "this frame holds a negative value": consumed before this kernel, reset for the next pass
        const bool general = r == 0;
        // 2: the any-distance kernels take the whole frame; 1: the rows flagged 1 (pre-marked here, or by k_fused, or (l2) by
        // k_l2win when it hands a row of far pixels on); 0: nothing for them
        // 3 (l1_cv, ROUTE_POINTS): k_pts takes the frame, of the any-distance kernels only k_tiesx has something to do
        const int f2 = (!l2 && r == ROUTE_POINTS) ? 3 : general ? 2 : ((ff.flags && ff.any1) || ff.anygone) ? 1 : 0;
        const int st = (general || r == ROUTE_POINTS || (ff.route > 0 && (ff.route & ROUTE_PREMARK))) ? DTFILL_FRAME_GENERAL_PATH : DTFILL_FRAME_OK;
        if (!raise) {
            fflag2[b] = f2;
            frame_status[b] = st;
        } else {
            // k_fused stores fflag2 = 1 in a window frame whose rows carry flags, where f2 is 0 or 1, and 2 in a window frame
            // under a depth epilogue, where f2 is 0 (no row flags): the OR never mixes two different non-zero values
            if (f2) atomicOr(&fflag2[b], f2);
            if (st) atomicOr(&frame_status[b], st);
        }
    }
    // (this block wrote bv_ before a barrier)
    if (ff.misaligned) value_list(b, x, valbits, wpre_v, H, W, Wd, vlist, [&](int i) { return bv_[i]; });
}

// What the publishing block of a frame needs beside the pass's shape (k_frame unpacks the pass record into it, k_fused's
// launch carries it: its blocks read the row counts, mode and the two nty from it, a frame's first block all of it)
struct FrameArgs {
    const float *x;
    const u64 *valbits, *srcbits;
    const u16 *wpre_v, *wpre_s;
    PtsSrc *ptslist;
    const u32 *rowcnt_s, *rowcnt_v;
    u32 *rowbase_s, *rowbase_v;
    int *negflag;
    int mode, nty16, nty32;
    int ride;   // k_fused: its window blocks work the frame facts out themselves, block 0 of a frame publishes them
    int ntmin;  // ... the number of tiles of the tiling with fewer of them: the blocks from there on look at route[b] first
};
__host__ __device__ inline FrameArgs frame_args(const Pass &p, int mode, int nty16, int nty32, int ride, int ntmin) {
    return FrameArgs{p.x, p.valbits, p.srcbits, p.wpre_v, p.wpre_s, p.ptslist, p.rowcnt_s, p.rowcnt_v, p.rowbase_s, p.rowbase_v,
                     p.negflag, mode, nty16, nty32, ride, ntmin};
}

// one block of 256 threads: the facts of frame b, published
__device__ __forceinline__ void frame_body(int b, const float *__restrict__ x, const u64 *__restrict__ valbits,
                                           const u16 *__restrict__ wpre_v, const u64 *__restrict__ srcbits,
                                           const u16 *__restrict__ wpre_s, PtsSrc *__restrict__ ptslist,
                                           const u32 *__restrict__ rowcnt_s, const u32 *__restrict__ rowcnt_v, int H, int W, int Wd,
                                           u32 *__restrict__ rowbase_s, u32 *__restrict__ rowbase_v, int *__restrict__ finfo,
                                           float *__restrict__ vlist, int *__restrict__ fflag2, int *__restrict__ route,
                                           int *__restrict__ frame_status, int mode, int *__restrict__ negflag,
                                           u32 *__restrict__ rowfar, int nty16, int nty32, FrameScratch &sc) {
    u32 *bs_ = rowbase_s + (size_t)b * H, *bv_ = rowbase_v + (size_t)b * H;
    const FrameFacts ff = frame_facts(rowcnt_s + (size_t)b * H, rowcnt_v + (size_t)b * H, H, W, mode, nty16, nty32, sc, true,
                                      [&](int i, u32 bs, u32 bv) {
                                          bs_[i] = bs;
                                          bv_[i] = bv;
                                      });
    frame_publish(ff, sc, b, x, valbits, wpre_v, srcbits, wpre_s, ptslist, H, W, Wd, bs_, bv_, finfo, vlist, fflag2, route, frame_status,
                  mode, negflag, rowfar, false);
}
// k_frame: one workgroup per frame, in a launch of its own (the l2 pass, the forced any-distance path, frames taller than
// FRAME_RIDE_MAX_H, DTFILL_FLAG_SEPARATE_FRAME; else k_fused's blocks do the same in its launch)
__global__ __launch_bounds__(256) void k_frame(const Pass p, int mode, int nty16, int nty32) {
    __shared__ FrameScratch sc;
    frame_body(blockIdx.x, p.x, p.valbits, p.wpre_v, p.srcbits, p.wpre_s, p.ptslist, p.rowcnt_s, p.rowcnt_v, p.H, p.W, p.Wd, p.rowbase_s,
               p.rowbase_v, p.finfo, p.vlist, p.fflag2, p.route, p.status, mode, p.negflag, p.rowfar, nty16, nty32, sc);
}

// label of the source at (i, j): 1 + number of sources before it in raster order
__device__ __forceinline__ int source_rank(u32 base, u64 word, int j) {
    return (int)base + __popcll(word & ((1ull << (j & 63)) - 1ull)) + 1;
}

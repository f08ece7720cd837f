// dtfill_near.hpp -- label -> source pixel: any channels filled from the nearest source, and the backward of that gather.
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit), after dtfill_fillb.hpp,
// whose cell sum (fb_ebias, fb_term, fb_finish, fb_combine) the backward uses as it stands.  include/dtfill.h states the
// contract (dtfill_nearest_gather, dtfill_nearest_gather_backward); DESIGN.md section 14 says why it has this form.
#pragma once

// Per frame: the source list is the pixels with NOT((1.0f - x) > src_thr) in raster order (m of them, s_k the k-th, a NaN is a
// source); a label L = index[p] with 1 <= L <= m names s_{L-1}; L == 0 names nothing (-1 / +0.0); any other L names nothing
// and raises DTFILL_FRAME_INDEX_ERROR.  The rule is per pixel.
//
// Launches of the forward (dtfill_nearest_gather), what each reads and writes:
//   k_ng_count      x -> the source bit words (one u64 per 64 columns of a row) and the per-row counts
//   k_ng_scan<0>    row counts -> row bases, m, the frame's status word (NO_SOURCE or 0)
//   k_ng_list       bit words, row bases -> spix[k] = the pixel of the k-th source
//   k_ng_gather     index, spix, values -> out_pixel, out_values; ORs INDEX_ERROR into the status word
// and of the backward (dtfill_nearest_gather_backward), in rounds of up to NG_CH channels that share one set of accumulators:
//   k_ng_count, k_ng_scan<1> (also clears the accumulators of k < m), then per round
//   k_ngb_acc<0,NC> index, grad_out -> E and the flags per (channel, k); the first round ORs INDEX_ERROR into the status word
//   k_ngb_acc<1,NC> index, grad_out, E -> T per (channel, k)
//   k_ngb_out<NC>   bit words, row bases, E, flags, T -> every pixel of the round's channels of grad_values once; leaves the
//                   accumulators it read cleared for the next round
// The status word is the caller's frame_status[b], or a word of the workspace when that is NULL.
constexpr int NG_CH = 2;  // channels of a backward round

struct NgWs {
    u64 *srcbits;     // [B*H*Wd] bit j of word c of a row: pixel 64 c + j is a source
    u32 *rowcnt;      // [B*H] sources of the row
    u32 *rowbase;     // [B*H] sources of the frame in front of the row
    u32 *nsrc;        // [B] m
    int32_t *status;  // [B] the status word of a call without a frame_status
    u32 *spix;        // forward [B*H*W]: flat pixel of the k-th source of the frame
    u32 *ebias;       // backward [NG_CH][B*H*W] per (channel of the round, k): as FbWs
    u32 *flags;       // backward [NG_CH][B*H*W]
    long long *tsum;  // backward [NG_CH][B*H*W]
    size_t N;         // B*H*W: the accumulators' channel pitch
    int Wd;
};

// k = L - 1 for 1 <= L <= m, -1 otherwise; any 32-bit L (the subtraction is unsigned: INT32_MIN wraps to a huge k).
__device__ __forceinline__ int ng_rank(int32_t L, u32 m) {
    const u32 k = (u32)L - 1u;
    return k < m ? (int)k : -1;
}

// One wave per row: the source predicate as bit words, and the row's count.
__global__ __launch_bounds__(256) void k_ng_count(const float *__restrict__ x, int H, int W, float src_thr, NgWs ws) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= H) return;
    const size_t fr = (size_t)b * H + row;
    const float *__restrict__ xr = x + fr * W;
    u64 *__restrict__ bits = ws.srcbits + fr * ws.Wd;
    u32 cnt = 0;
    for (int c0 = 0; c0 < ws.Wd; c0 += 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = (c0 + u) * 64 + lane;
            v[u] = col < W ? xr[col] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = (c0 + u) * 64 + lane;
            const u64 word = __ballot(col < W && !((1.0f - v[u]) > src_thr));  // a NaN is a source, as in dtfill_batch
            if (c0 + u < ws.Wd && lane == 0) bits[c0 + u] = word;
            cnt += (u32)__popcll(word);
        }
    }
    if (lane == 0) ws.rowcnt[fr] = cnt;
}

// Every block scans its frame's row counts (H <= 8191 numbers) and so knows m; block 0 of the frame publishes the row bases, m
// and the status word.  ACC (the backward): all of the frame's blocks share the clearing of the accumulators of k < m, nacc
// channels of them.
template <int ACC>
__global__ __launch_bounds__(256) void k_ng_scan(int H, size_t HW, int nacc, NgWs ws, int32_t *__restrict__ status) {
    __shared__ u32 part[256];
    const int b = blockIdx.y, t = threadIdx.x;
    const u32 *__restrict__ rc = ws.rowcnt + (size_t)b * H;
    const int per = (H + 255) / 256, r0 = min(t * per, H), r1 = min(r0 + per, H);
    u32 s = 0;
    for (int r = r0; r < r1; ++r) s += rc[r];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const u32 v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const u32 m = part[255];
    if (blockIdx.x == 0) {
        u32 base = part[t] - s;
        for (int r = r0; r < r1; ++r) {
            ws.rowbase[(size_t)b * H + r] = base;
            base += rc[r];
        }
        if (t == 0) {
            ws.nsrc[b] = m;
            status[b] = m ? DTFILL_FRAME_OK : DTFILL_FRAME_NO_SOURCE;
        }
    }
    if (ACC) {
        const size_t f0 = (size_t)b * HW;
        for (int c = 0; c < nacc; ++c) {
            const size_t at = c * ws.N + f0;
            for (u32 k = blockIdx.x * 256u + t; k < m; k += gridDim.x * 256u) {
                ws.ebias[at + k] = 0u;
                ws.flags[at + k] = 0u;
                ws.tsum[at + k] = 0;
            }
        }
    }
}

// One wave per row: the rank of a source is its row's base plus the popcount of the row's bit words to its left.
__global__ __launch_bounds__(256) void k_ng_list(int H, int W, NgWs ws) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= H) return;
    const size_t fr = (size_t)b * H + row;
    const u64 *__restrict__ bits = ws.srcbits + fr * ws.Wd;
    u32 *__restrict__ spix = ws.spix + (size_t)b * H * W;
    u32 rank = ws.rowbase[fr];
    for (int c = 0; c < ws.Wd; ++c) {
        const u64 word = bits[c];  // (no bit at a column >= W)
        if (word >> lane & 1ull) spix[rank + (u32)__popcll(word & ((1ull << lane) - 1ull))] = (u32)(row * W + c * 64 + lane);
        rank += (u32)__popcll(word);
    }
}

// PX pixels per thread (4: 16-byte loads and stores, W % 4 == 0 and 16-byte aligned pointers; 1 otherwise).  The labels of
// neighbouring pixels are mostly equal, so the reads of spix and of a channel's gathered dword broadcast and stay in cache.
// The payload moves as bits.
template <int PX, bool PIX, bool VAL>
__global__ __launch_bounds__(256) void k_ng_gather(const int32_t *__restrict__ index, const u32 *__restrict__ values, int C,
                                                   size_t HW, NgWs ws, u32 *__restrict__ out_values,
                                                   int32_t *__restrict__ out_pixel, int32_t *__restrict__ status) {
    const int b = blockIdx.y;
    const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;  // HW % PX == 0
    const bool in = p < HW;
    const u32 m = ws.nsrc[b];
    const size_t f0 = (size_t)b * HW;
    const u32 *__restrict__ spix = ws.spix + f0;
    int32_t L[PX];
    int s[PX];
    bool bad = false;
    if (in) {
        if constexpr (PX == 4) {
            const int4 v = *reinterpret_cast<const int4 *>(index + f0 + p);
            L[0] = v.x, L[1] = v.y, L[2] = v.z, L[3] = v.w;
        } else {
            L[0] = index[f0 + p];
        }
#pragma unroll
        for (int u = 0; u < PX; ++u) {
            const int k = ng_rank(L[u], m);
            bad |= k < 0 && L[u] != 0;
            s[u] = k >= 0 ? (int)spix[k] : -1;
        }
        if (PIX) {
            if constexpr (PX == 4)
                *reinterpret_cast<int4 *>(out_pixel + f0 + p) = make_int4(s[0], s[1], s[2], s[3]);
            else
                out_pixel[f0 + p] = s[0];
        }
        if (VAL) {
            for (int c = 0; c < C; ++c) {
                const size_t plane = ((size_t)b * C + c) * HW;
                const u32 *__restrict__ vc = values + plane;
                u32 g[PX];
#pragma unroll
                for (int u = 0; u < PX; ++u) g[u] = s[u] >= 0 ? vc[s[u]] : 0u;
                if constexpr (PX == 4)
                    *reinterpret_cast<uint4 *>(out_values + plane + p) = make_uint4(g[0], g[1], g[2], g[3]);
                else
                    out_values[plane + p] = g[0];
            }
        }
    }
    const u64 anybad = __ballot(bad);
    if (anybad && (threadIdx.x & 63) == __builtin_ctzll(anybad)) atomicOr(&status[b], DTFILL_FRAME_INDEX_ERROR);
}

// k_fb_acc for NC channels at once, with the source list's label rule and no frame-wide gate.  PASS 0: E and the flags.
// PASS 1: T.  One wave per strip of 64 columns x FB_TH rows; grad points at channel c0 of frame 0, cp = C*H*W is a frame's pitch
// in it.  raise: this launch reports the bad labels (PASS 0 of the first round).
template <int PASS, int NC>
__global__ __launch_bounds__(256) void k_ngb_acc(const int32_t *__restrict__ index, const float *__restrict__ grad, size_t cp, int H,
                                                 int W, int sx, int nstrips, bool raise, NgWs ws, int32_t *__restrict__ status) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int strip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip >= nstrips) return;
    const int r0 = (strip / sx) * FB_TH, r1 = min(r0 + FB_TH, H);
    const int col = (strip % sx) * 64 + lane;
    const bool in = col < W;
    const size_t HW = (size_t)H * W, f0 = (size_t)b * HW;
    const float *__restrict__ gb = grad + (size_t)b * cp;
    const u32 m = ws.nsrc[b];
    int cur = -1;                  // the k the lane is adding for
    u32 emax[NC] = {}, fl[NC] = {};  // PASS 0: its partials
    long long acc[NC] = {};        // PASS 1: its partials ...
    int ecur[NC] = {};             // ... and the cells' E + 150
    bool bad = false;

    auto flush = [&](bool mine) {
        const int key = mine ? cur : -1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const size_t at = c * ws.N + f0;
            if (PASS == 0) {
                u32 e = mine ? emax[c] : 0u, f = mine ? fl[c] : 0u;
                const bool any_f = __ballot(f != 0u) != 0ull;
                const bool lead = fb_combine(key, e, [](u32 a, u32 d) { return max(a, d); });
                if (any_f) fb_combine(key, f, [](u32 a, u32 d) { return a | d; });
                if (lead && e) atomicMax(&ws.ebias[at + key], e);
                if (lead && f) atomicOr(&ws.flags[at + key], f);
            } else {
                long long a = mine ? acc[c] : 0;
                const bool lead = fb_combine(key, a, [](long long p, long long d) { return p + d; });
                if (lead && a) atomicAdd(reinterpret_cast<unsigned long long *>(ws.tsum + at + key), (unsigned long long)a);
            }
        }
    };

    for (int rb = r0; rb < r1; rb += FB_RB) {
        int32_t li[FB_RB];
        float g[NC][FB_RB];
#pragma unroll
        for (int u = 0; u < FB_RB; ++u) {
            const bool ok = in && rb + u < r1;
            const size_t at = (size_t)(rb + u) * W + col;
            li[u] = ok ? index[f0 + at] : 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) g[c][u] = ok ? gb[c * HW + at] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < FB_RB; ++u) {
            if (rb + u >= r1) break;  // (wave-uniform)
            const int k = in ? ng_rank(li[u], m) : -1;
            bad |= in && k < 0 && li[u] != 0;
            const bool change = k != cur;
            const bool mine = change && cur >= 0;
            if (__ballot(mine)) flush(mine);
            if (change) {
                cur = k;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    emax[c] = 0, fl[c] = 0, acc[c] = 0;
                    if (PASS == 1 && k >= 0) ecur[c] = (int)ws.ebias[c * ws.N + f0 + k];
                }
            }
            if (k >= 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (PASS == 0)
                        emax[c] = max(emax[c], fb_ebias(g[c][u], fl[c]));
                    else
                        acc[c] += fb_term(g[c][u], ecur[c]);
                }
            }
        }
    }
    flush(cur >= 0);
    if (PASS == 0 && raise) {
        const u64 anybad = __ballot(bad);
        if (anybad && lane == __builtin_ctzll(anybad)) atomicOr(&status[b], DTFILL_FRAME_INDEX_ERROR);
    }
}

// One wave per row: every pixel of the round's NC channels of grad_values once (out points at channel c0 of frame 0, cp as
// above).  A source's k is its row's base plus its rank within the row.  reset: another round follows, so the accumulators
// read here are left cleared for it (each k < m is read by exactly one lane of one wave).
template <int NC>
__global__ __launch_bounds__(256) void k_ngb_out(int H, int W, size_t cp, bool reset, NgWs ws, float *__restrict__ out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= H) return;
    const size_t fr = (size_t)b * H + row, HW = (size_t)H * W, f0 = (size_t)b * HW;
    const u64 *__restrict__ bits = ws.srcbits + fr * ws.Wd;
    float *__restrict__ orow = out + (size_t)b * cp + (size_t)row * W;
    u32 rank = ws.rowbase[fr];
    for (int w = 0; w < ws.Wd; ++w) {
        const u64 word = bits[w];
        const int col = w * 64 + lane;
        const bool src = word >> lane & 1ull;
        const size_t k = f0 + rank + (u32)__popcll(word & ((1ull << lane) - 1ull));
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float s = 0.0f;
            if (src) {
                const size_t at = c * ws.N + k;
                s = fb_finish(ws.ebias[at], ws.flags[at], ws.tsum[at]);
                if (reset) {
                    ws.ebias[at] = 0u;
                    ws.flags[at] = 0u;
                    ws.tsum[at] = 0;
                }
            }
            if (col < W) orow[c * HW + col] = s;
        }
        rank += (u32)__popcll(word);
    }
}

// dtfill_fillb.hpp -- the backward pass of the exact fill depth = depth_list[lbl - 1] (tools.py:24-26): the gradient of the
// filled depth gathered back onto the valued pixels.  Part of libdtfill.so; included by dtfill.hip inside its anonymous
// namespace (one translation unit).  include/dtfill.h states the contract (dtfill_fill_backward); DESIGN.md says why it has
// this form.
#pragma once

// Per frame: the value list is the pixels with x > val_thr in raster order (n of them, v_k the k-th); pixel p addresses
// idx(p) = index[p] - 1, + n when negative; grad_x[v_k] = S({grad_depth[p] : idx(p) = k}), +0.0 at every other pixel; a frame
// with an idx outside [0, n) is all +0.0 and carries DTFILL_FRAME_INDEX_ERROR.
//
// S(C) is defined through integers so that it does not depend on the order of the additions: E = the largest true binary
// exponent of the cell's finite non-zero terms, every term the integer t = rint(g * 2^-(E - 37)), T = sum t, S = T * 2^(E - 37)
// rounded once from the integer to float32 and scaled.  So the accumulators are integers and integer atomics suffice: a
// 32-bit max for E, a 32-bit OR for the NaN / +inf / -inf flags, a 64-bit add for T.  All three are associative and
// commutative: two calls give the same bits whatever order the blocks run in.
//
// Launches (dtfill_fill_backward), what each reads and writes:
//   k_fb_count  x -> the value bit words (one u64 per 64 columns of a row) and the per-row counts; clears the error flag
//   k_fb_scan   row counts -> row bases (exclusive scan within the frame) and n; clears the accumulators of k < n
//   k_fb_acc<0> index, grad_depth -> E and the flags per k; raises the frame's error flag
//   k_fb_acc<1> index, grad_depth, E -> T per k (not for a frame whose error flag is up)
//   k_fb_out    value bit words, row bases, E, flags, T, the error flag -> every pixel of grad_x once, frame_status
// index and grad_depth are read twice (E has to be final before a term can be rounded): 24 bytes per pixel with x's read
// and grad_x's store.
//
// k_fb_acc combines on chip before any atomic.  A wave owns a strip of 64 columns x FB_TH rows, a lane one column of it.  The
// lane walks down its column adding into a register while the label stays what it was (a cell is a run of rows in a column:
// the stripes under the first scan line of a LiDAR frame are a hundred rows high).  When the label changes the lane has one
// (k, partial) to flush; the flushing lanes of the wave then sum runs of neighbouring lanes that hold the same k into the
// run's first lane (fb_combine), which issues the one atomic.  A frame with one source so costs one atomic per strip,
// not one per pixel.
constexpr int FB_TH = 32;  // rows of a strip
constexpr int FB_RB = 8;   // rows a lane loads ahead of working on them
constexpr u32 FB_NAN = 1u, FB_PINF = 2u, FB_NINF = 4u;  // flag bits of a cell

struct FbWs {
    u64 *valbits;      // [B*H*Wd] bit j of word c of a row: pixel 64 c + j is valued
    u32 *rowcnt;       // [B*H] valued pixels of the row
    u32 *rowbase;      // [B*H] valued pixels of the frame in front of the row
    u32 *nval;         // [B] n
    u32 *err;          // [B] non-zero: some pixel of the frame addresses outside [0, n)
    u32 *ebias;        // [B*H*W] per k: E + 150 (1 .. 277), 0 = no finite non-zero term
    u32 *flags;        // [B*H*W] per k: FB_*
    long long *tsum;   // [B*H*W] per k: T
    int Wd;
};

// One wave per row: the value predicate as bit words, and the row's count.
__global__ __launch_bounds__(256) void k_fb_count(const float *__restrict__ x, int H, int W, float val_thr, FbWs ws) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.err[b] = 0u;
    if (row >= H) return;
    const size_t fr = (size_t)b * H + row;
    const float *__restrict__ xr = x + fr * W;
    u64 *__restrict__ bits = ws.valbits + fr * ws.Wd;
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
            const u64 word = __ballot(col < W && v[u] > val_thr);  // a NaN is not valued, as in numpy
            if (c0 + u < ws.Wd && lane == 0) bits[c0 + u] = word;
            cnt += (u32)__popcll(word);
        }
    }
    if (lane == 0) ws.rowcnt[fr] = cnt;
}

// Every block scans its frame's row counts (H <= 8191 numbers) and so knows n; block 0 of the frame publishes the row bases
// and n; all of the frame's blocks share the clearing of the accumulators of k < n.
__global__ __launch_bounds__(256) void k_fb_scan(int H, size_t HW, FbWs ws) {
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
    const u32 n = part[255];
    if (blockIdx.x == 0) {
        u32 base = part[t] - s;
        for (int r = r0; r < r1; ++r) {
            ws.rowbase[(size_t)b * H + r] = base;
            base += rc[r];
        }
        if (t == 0) ws.nval[b] = n;
    }
    const size_t f0 = (size_t)b * HW;
    for (u32 k = blockIdx.x * 256u + t; k < n; k += gridDim.x * 256u) {
        ws.ebias[f0 + k] = 0u;
        ws.flags[f0 + k] = 0u;
        ws.tsum[f0 + k] = 0;
    }
}

// E + 150 of one term (0: zero or not finite, which raises its flag instead).  Subnormals count by their true exponent.
__device__ __forceinline__ u32 fb_ebias(float g, u32 &fl) {
    const u32 u = __float_as_uint(g), ef = (u >> 23) & 0xFFu, fr = u & 0x7FFFFFu;
    if (ef == 0xFFu) {
        fl |= fr ? FB_NAN : (u >> 31) ? FB_NINF : FB_PINF;
        return 0u;
    }
    if (ef) return ef + 23u;
    return fr ? 32u - (u32)__clz(fr) : 0u;
}

// t = rint(g * 2^-(E - 37)), round half to even, in integers; ebc = E + 150 of the cell (>= the term's own).
// g = m * 2^(xf - 150) with xf = max(exponent field, 1), so t = m * 2^(xf + 37 - ebc); |t| < 2^38.
__device__ __forceinline__ long long fb_term(float g, int ebc) {
    const u32 u = __float_as_uint(g), ef = (u >> 23) & 0xFFu, fr = u & 0x7FFFFFu;
    if (ef == 0xFFu || (ef | fr) == 0u) return 0;
    const u32 m = ef ? fr | 0x800000u : fr;
    const int s = (int)(ef ? ef : 1u) + 37 - ebc;
    long long t;
    if (s >= 0) {
        t = (long long)m << min(s, 38);
    } else if (s <= -25) {
        t = 0;  // m < 2^24: below half a unit
    } else {
        const int r = -s;
        u32 q = m >> r;
        const u32 rem = m & ((1u << r) - 1u), half = 1u << (r - 1);
        if (rem > half || (rem == half && (q & 1u))) ++q;
        t = q;
    }
    return (u >> 31) ? -t : t;
}

// S of a finished cell.
__device__ __forceinline__ float fb_finish(u32 ebc, u32 fl, long long T) {
    if (fl) {
        if ((fl & FB_NAN) || (fl & (FB_PINF | FB_NINF)) == (FB_PINF | FB_NINF)) return __uint_as_float(0x7FC00000u);
        return __uint_as_float((fl & FB_PINF) ? 0x7F800000u : 0xFF800000u);
    }
    if (ebc == 0u || T == 0) return 0.0f;
    const int q = (int)ebc - 150 - 37;  // -186 .. 90
    const float f = (float)T;           // the one rounding of the integer
    // ldexpf(f, q): the product is exact in double, the conversion rounds once (into the subnormals, or to infinity)
    return (float)((double)f * __longlong_as_double((long long)(q + 1023) << 52));
}

// The flushing lanes of a wave hold (key >= 0, val), the others key = -1.  Runs of neighbouring lanes with one key are
// combined into the run's first lane; true for the lane that then holds a run's total.
template <class V, class Op>
__device__ __forceinline__ bool fb_combine(int key, V &val, Op op) {
    const int lane = threadIdx.x & 63;
    const int left = __shfl_up(key, 1);
    const bool head = lane == 0 || left != key;
    const u64 heads = __ballot(head);
    const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + __builtin_ctzll(above) : 63;  // the run's last lane
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_down(val, d);
        if (lane + d <= end) val = op(val, o);
    }
    return head && key >= 0;
}

// PASS 0: E and the flags.  PASS 1: T.  One wave per strip of 64 columns x FB_TH rows, nstrips = sx * ceil(H / FB_TH) per frame.
template <int PASS>
__global__ __launch_bounds__(256) void k_fb_acc(const int32_t *__restrict__ index, const float *__restrict__ grad, int H, int W,
                                                int sx, int nstrips, FbWs ws) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int strip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip >= nstrips) return;
    if (PASS == 1 && ws.err[b]) return;  // final: the launch before this one raised it
    const int r0 = (strip / sx) * FB_TH, r1 = min(r0 + FB_TH, H);
    const int col = (strip % sx) * 64 + lane;
    const bool in = col < W;
    const size_t f0 = (size_t)b * H * W;
    const int n = (int)ws.nval[b];  // < 2^24.001 (the shape rule)
    u32 *__restrict__ eb = ws.ebias + f0;
    u32 *__restrict__ fg = ws.flags + f0;
    unsigned long long *__restrict__ ts = reinterpret_cast<unsigned long long *>(ws.tsum + f0);
    int cur = -1;       // the k the lane is adding for
    u32 emax = 0, fl = 0;  // PASS 0: its partial
    long long acc = 0;  // PASS 1: its partial ...
    int ecur = 0;       // ... and the cell's E + 150
    bool bad = false;

    auto flush = [&](bool mine) {
        const int key = mine ? cur : -1;
        if (PASS == 0) {
            u32 e = mine ? emax : 0u, f = mine ? fl : 0u;
            const bool any_f = __ballot(f != 0u) != 0ull;
            const bool lead = fb_combine(key, e, [](u32 a, u32 c) { return max(a, c); });
            if (any_f) fb_combine(key, f, [](u32 a, u32 c) { return a | c; });
            if (lead && e) atomicMax(&eb[key], e);
            if (lead && f) atomicOr(&fg[key], f);
        } else {
            long long a = mine ? acc : 0;
            const bool lead = fb_combine(key, a, [](long long p, long long c) { return p + c; });
            if (lead && a) atomicAdd(&ts[key], (unsigned long long)a);
        }
    };

    for (int rb = r0; rb < r1; rb += FB_RB) {
        int32_t li[FB_RB];
        float g[FB_RB];
#pragma unroll
        for (int u = 0; u < FB_RB; ++u) {
            const bool ok = in && rb + u < r1;
            const size_t at = f0 + (size_t)(rb + u) * W + col;
            li[u] = ok ? index[at] : 0;
            g[u] = ok ? grad[at] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < FB_RB; ++u) {
            if (rb + u >= r1) break;  // (wave-uniform)
            int k = -1;
            if (in) {
                // numpy's rule (dtfill_index.hpp) for any 32-bit label; INT32_MIN - 1 is not computed
                const DepthIndex di = li[u] == INT32_MIN ? DepthIndex{0, false} : depth_index(li[u], n);
                if (di.ok)
                    k = di.idx;
                else
                    bad = true;
            }
            const bool change = k != cur;
            const bool mine = change && cur >= 0;
            if (__ballot(mine)) flush(mine);
            if (change) {
                cur = k;
                emax = 0, fl = 0, acc = 0;
                if (PASS == 1 && k >= 0) ecur = (int)eb[k];
            }
            if (k >= 0) {
                if (PASS == 0)
                    emax = max(emax, fb_ebias(g[u], fl));
                else
                    acc += fb_term(g[u], ecur);
            }
        }
    }
    flush(cur >= 0);
    if (PASS == 0) {
        const u64 anybad = __ballot(bad);
        if (anybad && lane == __builtin_ctzll(anybad)) atomicOr(&ws.err[b], 1u);
    }
}

// One wave per row: every pixel of grad_x once.  A valued pixel's k is its row's base plus its rank within the row.
__global__ __launch_bounds__(256) void k_fb_out(int H, int W, FbWs ws, float *__restrict__ grad_x, int32_t *__restrict__ status) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool err = ws.err[b] != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0 && status) status[b] = err ? DTFILL_FRAME_INDEX_ERROR : DTFILL_FRAME_OK;
    if (row >= H) return;
    const size_t fr = (size_t)b * H + row, f0 = (size_t)b * H * W;
    const u64 *__restrict__ bits = ws.valbits + fr * ws.Wd;
    float *__restrict__ out = grad_x + fr * W;
    u32 rank = ws.rowbase[fr];
    for (int c = 0; c < ws.Wd; ++c) {
        const u64 word = err ? 0ull : bits[c];
        const int col = c * 64 + lane;
        float s = 0.0f;
        if (word >> lane & 1ull) {
            const size_t k = f0 + rank + (u32)__popcll(word & ((1ull << lane) - 1ull));
            s = fb_finish(ws.ebias[k], ws.flags[k], ws.tsum[k]);
        }
        if (col < W) out[col] = s;
        rank += (u32)__popcll(word);
    }
}

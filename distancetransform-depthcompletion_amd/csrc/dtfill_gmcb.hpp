// dtfill_gmcb.hpp -- k_gmcb: the transpose of one step of generate_multi_channel(), net.py:83-122 (the backward of k_gmc)
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// tf.equal, tf.cast and tf.greater have no gradient, so the selection of a forward step and the re-masking between the steps
// are constants: a step is a fixed sparse linear map of its data, out_p = sum_t sel_p(t) d[p + t] / (1e-6 + cnt_p), and its
// backward is the transpose of that map.  It needs the step's mask, never its data (include/dtfill.h):
//   mx_p, cnt_p   the forward's window maximum of m[p + t] * w(t) over all ts^2 taps (padding taps: product 0; a NaN product
//                 is never selected) and the number of taps that reach it;
//   c_p           G_p / (1e-6f + cnt_p), one IEEE division per window;
//   out_q         g_q + (the float32 sum, from +0, of c_p over the in-image windows p around q that selected q,
//                 m[q] * w(q - p) == mx_p, in ascending raster order of p).
// A c_p is added only where it is selected, so a non-finite G_p stays inside the pixels its window selected.
// mask == nullptr: the mask is (fwd > 0.001f), fwd the forward output the step read (net.py:95-96), tested while staging.
//
// One block per 16 x 64 tile of q, the forward's tiling.  In LDS: the mask tile with a 2 * half halo (the windows of the centres
// that can select a q of the tile), then (mx_p, c_p) of the (16 + 2 half) x (64 + 2 half) centres around the tile, one float2
// each, computed once per block; a centre outside the image holds (NaN, 0): no product equals NaN, so it selects nothing.  Then
// every q gathers from its ts^2 centres in raster order.  No atomics: the order of the additions is the contract.  The tiles
// are numbered in one dimension (tile column fastest, then tile row, then frame) and a block strides over them, as k_gmcv.
// CTS: the compile-time table size (7: every model of the reference), or 0 for the `ts` argument.
template <int CTS>
__global__ __launch_bounds__(256) void k_gmcb(const float *__restrict__ mask, const float *__restrict__ fwd,
                                              const float *__restrict__ G, const float *__restrict__ gk, int H, int W, int ts,
                                              int tx, int ty, u32 ntiles, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float s_gb[];
    if (CTS) ts = CTS;
    constexpr int UNR = CTS ? CTS : 1;  // the tap loops of a compile-time table are unrolled whole
    const int half = (ts - 1) / 2;
    const int CW = GM_TW + 2 * half, CH = GM_TH + 2 * half;  // centres
    const int MW = GM_TW + 4 * half, MH = GM_TH + 4 * half;  // mask taps
    float2 *s_c = reinterpret_cast<float2 *>(s_gb);
    float *s_m = s_gb + 2 * CH * CW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (one round unless the grid was capped)
        const u32 tb = tile / (u32)tx;
        const int r0 = (int)(tb % (u32)ty) * GM_TH, c0 = (int)(tile % (u32)tx) * GM_TW;
        const size_t fo = (size_t)(tb / (u32)ty) * H * W;
        for (int k = threadIdx.x; k < MH * MW; k += 256) {
            const int r = k / MW, c = k - r * MW;
            const int gi = r0 + r - 2 * half, gj = c0 + c - 2 * half;
            float m = 0.0f;
            if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
                const size_t at = fo + (size_t)gi * W + gj;
                m = mask ? mask[at] : (fwd[at] > 0.001f ? 1.0f : 0.0f);
            }
            s_m[k] = m;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < CH * CW; k += 256) {
            const int r = k / CW, c = k - r * CW;
            const int gi = r0 + r - half, gj = c0 + c - half;
            const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W;
            const float Gp = in ? G[fo + (size_t)gi * W + gj] : 0.0f;
            // one pass over the taps: a new maximum restarts the count, an equal product extends it (mx starts at -inf: a
            // window of negative products selects its largest one; a NaN product is neither greater nor equal)
            float mx = -INFINITY, cnt = 0.0f;
            const float *mp = s_m + r * MW + c;
#pragma unroll UNR
            for (int i = 0; i < ts; ++i) {
#pragma unroll UNR
                for (int j = 0; j < ts; ++j) {
                    const float w = (float)(ts - abs(i - half) - abs(j - half));
                    const float sv = mp[i * MW + j] * w;
                    const bool gt = sv > mx, eq = sv == mx;
                    cnt = gt ? 1.0f : (eq ? cnt + 1.0f : cnt);
                    mx = gt ? sv : mx;
                }
            }
            s_c[k] = in ? make_float2(mx, __fdiv_rn(Gp, __fadd_rn(0.000001f, cnt))) : make_float2(NAN, 0.0f);
        }
        __syncthreads();
        for (int u = wave; u < GM_TH * GM_NCW; u += 4) {  // a wave per (row, column group), a lane per column
            const int r = u / GM_NCW, c = 64 * (u % GM_NCW) + lane;
            const int gi = r0 + r, gj = c0 + c;
            const bool in = gi < H && gj < W;
            const size_t at = fo + (size_t)gi * W + gj;
            const float gq = (gk && in) ? gk[at] : 0.0f;
            const float mq = s_m[(r + 2 * half) * MW + c + 2 * half];
            // p = q + (i - half, j - half) ascending in raster order; q is tap q - p of that window, of weight ts - |di| - |dj|
            float acc = 0.0f;
            const float2 *cp = s_c + r * CW + c;
#pragma unroll UNR
            for (int i = 0; i < ts; ++i) {
#pragma unroll UNR
                for (int j = 0; j < ts; ++j) {
                    const float w = (float)(ts - abs(i - half) - abs(j - half));
                    const float2 mc = cp[i * CW + j];
                    acc = mq * w == mc.x ? __fadd_rn(acc, mc.y) : acc;
                }
            }
            if (in) out[at] = gk ? __fadd_rn(gq, acc) : acc;
        }
        __syncthreads();  // the tile is read: the next round may stage
    }
}

// A chain that ends without a window step: out = g (scale_num 1), out = g + (+0) (every later gradient NULL: the transpose
// sums are all +0), or +0 everywhere for a NULL g.
__global__ __launch_bounds__(256) void k_gmcb_first(const float *__restrict__ g, size_t n, int plus0, float *__restrict__ out) {
    for (size_t at = (size_t)blockIdx.x * 256 + threadIdx.x; at < n; at += (size_t)gridDim.x * 256) {
        const float v = g ? g[at] : 0.0f;
        out[at] = plus0 ? __fadd_rn(v, 0.0f) : v;
    }
}

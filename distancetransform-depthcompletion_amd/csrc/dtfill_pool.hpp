// dtfill_pool.hpp -- the max-pool pyramid of ResNet18_NO_BN_l2_light_image (solution_DeepNet/net.py:4285, 4320, 4353): one
// tensor pooled by 2, 4 and 8 in one pass, and its backward (include/dtfill.h, dtfill_max_pool_pyramid and
// dtfill_max_pool_pyramid_backward).  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace.
//
// Both kernels are memory-bound: one read of x and 21/64 of it written forward; x, the dys and dx backward.  A thread owns
// one float4 of channels of one K x K window, K the largest requested level, and walks the window's pixels in raster order,
// two rows of K loads in flight at a time (the loop over the K / 2 row pairs is a real loop: unrolled, the compiler hoists all
// 64 loads of an 8 x 8 window and needs 256 VGPRs, or spills under a lower cap).  Adjacent threads own adjacent channel quads, then the next window to the right: the
// 64 channels of a pixel are 256 contiguous bytes, read by 16 lanes at once.  The grid is sized by windows times quads.
//
// Why no merge of block winners: the raster order of a window, restricted to any aligned sub-window, is that sub-window's own
// raster order.  So ONE scan of the K x K window feeds a running winner per level (one of level 8, two of level 4, four of
// level 2 are alive at a time), each by the contract's rule, and each level's winner is its raster-first one by construction.
// Nothing is built from the level below, no tie is ever broken by block order, and every pixel is loaded once.
//
// The backward runs the same scan with the winner's position beside each value, packed per channel: 2 bits for each of the 16
// level-2 windows in one word, 4 bits for each of the four level-4 windows and 6 bits for level 8 in another.  A second walk
// over the window's pixels, which reads only the dys, writes dx[p] = (t2 + t4) + t8, zeros included.  Windows are disjoint, so
// there are no atomics and no workspace.
#pragma once

struct PoolArgs {
    const float *x;
    const float *dy[3];  // backward: the gradients of levels 2, 4, 8 (NULL: +0)
    float *out[3];       // forward: the outputs of levels 2, 4, 8 (NULL: skipped)
    float *dx;           // backward: dense [B,H,W,C]
    int B, H, W, C, xc, xo;
    int lc[3], lo[3];  // width and offset of out_k (forward) or dy_k (backward)
    long long total;   // windows times channel quads
};

template <bool VEC>
__device__ __forceinline__ float4 pool_ld(const float *p) {
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool VEC>
__device__ __forceinline__ void pool_st(float *p, float4 v) {
    if (VEC) {
        *reinterpret_cast<float4 *>(p) = v;
    } else {
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    }
}

// the contract's step: best stays if it is NaN; else e takes over if it is larger or NaN.  (!(e <= b) is e > b or unordered.)
__device__ __forceinline__ bool pool_take(float e, float b) { return !(e <= b) && b == b; }

__device__ __forceinline__ void pool_scan(float4 &b, float4 e) {
    b.x = pool_take(e.x, b.x) ? e.x : b.x;
    b.y = pool_take(e.y, b.y) ? e.y : b.y;
    b.z = pool_take(e.z, b.z) ? e.z : b.z;
    b.w = pool_take(e.w, b.w) ? e.w : b.w;
}

// the same with the position `at` of e within its window
__device__ __forceinline__ void pool_scan_at(float4 &b, uint4 &p, float4 e, unsigned at) {
    const bool tx = pool_take(e.x, b.x), ty = pool_take(e.y, b.y), tz = pool_take(e.z, b.z), tw = pool_take(e.w, b.w);
    b.x = tx ? e.x : b.x, p.x = tx ? at : p.x;
    b.y = ty ? e.y : b.y, p.y = ty ? at : p.y;
    b.z = tz ? e.z : b.z, p.z = tz ? at : p.z;
    b.w = tw ? e.w : b.w, p.w = tw ? at : p.w;
}

__device__ __forceinline__ void pool_or(uint4 &w, uint4 p, int shift) {
    w.x |= p.x << shift, w.y |= p.y << shift, w.z |= p.z << shift, w.w |= p.w << shift;
}

// The thread's window: b, the window's row and column (in windows), the first channel of its quad.
template <int K>
__device__ __forceinline__ bool pool_item(const PoolArgs &a, int *b, int *wh, int *wv, int *c) {
    // 32-bit index arithmetic: total <= B H W C / 4 < 2^29 by the domain, and a 64-bit division is a long software routine
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)a.total) return false;
    const unsigned C4 = a.C >> 2, Wk = a.W / K, Hk = a.H / K;
    *c = (int)(t % C4) * 4;
    unsigned win = t / C4;
    *wv = (int)(win % Wk);
    win /= Wk;
    *wh = (int)(win % Hk);
    *b = (int)(win / Hk);
    return true;
}

// the element (b, h, v, channel c) of level l's tensor, [B, H / k, W / k, lc[l]] read or written at lo[l]
template <int LEVEL>
__device__ __forceinline__ size_t pool_at(const PoolArgs &a, int b, int h, int v, int c) {
    constexpr int k = 2 << LEVEL;
    return (((size_t)b * (a.H / k) + h) * (a.W / k) + v) * a.lc[LEVEL] + a.lo[LEVEL] + c;
}

template <int K, bool VEC>
__global__ __launch_bounds__(256) void k_pool_pyramid(const PoolArgs a) {
    int b, wh, wv, c;
    if (!pool_item<K>(a, &b, &wh, &wv, &c)) return;
    const float *xp = a.x + (((size_t)b * a.H + (size_t)wh * K) * a.W + (size_t)wv * K) * a.xc + a.xo + c;
    const size_t row = (size_t)a.W * a.xc;
    constexpr int N2 = K / 2, N4 = K >= 4 ? K / 4 : 1;
    const float4 zero = make_float4(0, 0, 0, 0);
    float4 b4[N4], b8 = zero;
#pragma unroll
    for (int n = 0; n < N4; ++n) b4[n] = zero;
#pragma unroll 1
    for (int band = 0; band < K / 2; ++band, xp += 2 * row) {  // the window's rows 2 band and 2 band + 1
        float4 v[2][K], b2[N2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) v[r][j] = pool_ld<VEC>(xp + r * row + (size_t)j * a.xc);
        const bool first4 = (band & 1) == 0, first8 = band == 0;  // this band opens its level-4 windows, the level-8 window
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float4 e = v[r][j];
                if (r == 0 && (j & 1) == 0) b2[j >> 1] = e;
                else pool_scan(b2[j >> 1], e);
                if (K >= 4) {
                    if (r == 0 && (j & 3) == 0 && first4) b4[j >> 2] = e;
                    else pool_scan(b4[j >> 2], e);
                }
                if (K >= 8) {
                    if (r == 0 && j == 0 && first8) b8 = e;
                    else pool_scan(b8, e);
                }
            }
        }
        if (a.out[0]) {
#pragma unroll
            for (int n = 0; n < N2; ++n) pool_st<VEC>(a.out[0] + pool_at<0>(a, b, wh * (K / 2) + band, wv * (K / 2) + n, c), b2[n]);
        }
        if (K >= 4 && !first4 && a.out[1]) {
#pragma unroll
            for (int n = 0; n < N4; ++n)
                pool_st<VEC>(a.out[1] + pool_at<1>(a, b, wh * (K / 4) + (band >> 1), wv * (K / 4) + n, c), b4[n]);
        }
    }
    if (K >= 8 && a.out[2]) pool_st<VEC>(a.out[2] + pool_at<2>(a, b, wh, wv, c), b8);
}

// d where the field `mask` of w at `shift` holds `at`, +0 elsewhere
__device__ __forceinline__ float4 pool_pick(uint4 w, int shift, unsigned mask, unsigned at, float4 d) {
    return make_float4(((w.x >> shift) & mask) == at ? d.x : 0.0f, ((w.y >> shift) & mask) == at ? d.y : 0.0f,
                       ((w.z >> shift) & mask) == at ? d.z : 0.0f, ((w.w >> shift) & mask) == at ? d.w : 0.0f);
}

// K = 1: no level is asked for, dx is all +0.
template <int K, bool VEC>
__global__ __launch_bounds__(256) void k_pool_pyramid_backward(const PoolArgs a) {
#pragma clang fp contract(off)
    int b, wh, wv, c;
    if (!pool_item<K>(a, &b, &wh, &wv, &c)) return;
    const float *xp = a.x + (((size_t)b * a.H + (size_t)wh * K) * a.W + (size_t)wv * K) * a.xc + a.xo + c;
    float *dxp = a.dx + (((size_t)b * a.H + (size_t)wh * K) * a.W + (size_t)wv * K) * a.C + c;
    const float4 zero = make_float4(0, 0, 0, 0);
    if (K == 1) {
        pool_st<VEC>(dxp, zero);
        return;
    }
    const size_t row = (size_t)a.W * a.xc, dx_row = (size_t)a.W * a.C;
    constexpr int N2 = K >= 2 ? K / 2 : 1, N4 = K >= 4 ? K / 4 : 1;
    const uint4 none = make_uint4(0, 0, 0, 0);
    uint4 w2 = none, w48 = none;  // the winners' positions: level 2, 2 bits a window; level 4, 4 bits a window, and level 8 from bit 16
    {
        float4 b4[N4], b8 = zero;
        uint4 p4[N4], p8 = none;
#pragma unroll
        for (int n = 0; n < N4; ++n) b4[n] = zero, p4[n] = none;
#pragma unroll 1
        for (int band = 0; band < K / 2; ++band, xp += 2 * row) {
            float4 v[2][K], b2[N2];
            uint4 p2[N2];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < K; ++j) v[r][j] = pool_ld<VEC>(xp + r * row + (size_t)j * a.xc);
            const bool first4 = (band & 1) == 0, first8 = band == 0;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float4 e = v[r][j];
                    if (r == 0 && (j & 1) == 0) b2[j >> 1] = e, p2[j >> 1] = none;
                    else pool_scan_at(b2[j >> 1], p2[j >> 1], e, r * 2 + (j & 1));
                    if (K >= 4) {
                        if (r == 0 && (j & 3) == 0 && first4) b4[j >> 2] = e, p4[j >> 2] = none;
                        else pool_scan_at(b4[j >> 2], p4[j >> 2], e, ((band & 1) * 2 + r) * 4 + (j & 3));
                    }
                    if (K >= 8) {
                        if (r == 0 && j == 0 && first8) b8 = e, p8 = none;
                        else pool_scan_at(b8, p8, e, (band * 2 + r) * 8 + j);
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < N2; ++n) pool_or(w2, p2[n], 2 * (band * 4 + n));
            if (K >= 4 && !first4) {
#pragma unroll
                for (int n = 0; n < N4; ++n) pool_or(w48, p4[n], 4 * ((band >> 1) * 2 + n));
            }
        }
        if (K >= 8) pool_or(w48, p8, 16);
    }
    // dx[p] = (t2 + t4) + t8, each +0 where p is not that level's winner; a level that is not asked for has a dy of +0
    const float4 d8 = K >= 8 && a.dy[2] ? pool_ld<VEC>(a.dy[2] + pool_at<2>(a, b, wh, wv, c)) : zero;
    float4 d4[N4];
#pragma unroll
    for (int n = 0; n < N4; ++n) d4[n] = zero;
#pragma unroll 1
    for (int band = 0; band < K / 2; ++band, dxp += 2 * dx_row) {
        float4 d2[N2];
        if (K >= 4 && (band & 1) == 0 && a.dy[1]) {
#pragma unroll
            for (int n = 0; n < N4; ++n) d4[n] = pool_ld<VEC>(a.dy[1] + pool_at<1>(a, b, wh * (K / 4) + (band >> 1), wv * (K / 4) + n, c));
        }
#pragma unroll
        for (int n = 0; n < N2; ++n)
            d2[n] = a.dy[0] ? pool_ld<VEC>(a.dy[0] + pool_at<0>(a, b, wh * (K / 2) + band, wv * (K / 2) + n, c)) : zero;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float4 t2 = pool_pick(w2, 2 * (band * 4 + (j >> 1)), 3u, r * 2 + (j & 1), d2[j >> 1]);
                float4 t4 = zero, t8 = zero;
                if (K >= 4) t4 = pool_pick(w48, 4 * ((band >> 1) * 2 + (j >> 2)), 15u, ((band & 1) * 2 + r) * 4 + (j & 3), d4[j >> 2]);
                if (K >= 8) t8 = pool_pick(w48, 16, 63u, (band * 2 + r) * 8 + j, d8);
                pool_st<VEC>(dxp + r * dx_row + (size_t)j * a.C,
                             make_float4((t2.x + t4.x) + t8.x, (t2.y + t4.y) + t8.y, (t2.z + t4.z) + t8.z, (t2.w + t4.w) + t8.w));
            }
        }
    }
}

// `vec`: every pointer of the call is 16-byte aligned (the channel counts and offsets are multiples of 4 by the domain)
template <int K>
static void pool_launch(hipStream_t st, const PoolArgs &a, bool vec) {
    const unsigned grid = (unsigned)((a.total + 255) / 256);
    (vec ? k_pool_pyramid<K, true> : k_pool_pyramid<K, false>)<<<grid, 256, 0, st>>>(a);
}

template <int K>
static void pool_backward_launch(hipStream_t st, const PoolArgs &a, bool vec) {
    const unsigned grid = (unsigned)((a.total + 255) / 256);
    (vec ? k_pool_pyramid_backward<K, true> : k_pool_pyramid_backward<K, false>)<<<grid, 256, 0, st>>>(a);
}

// dtfill_outlier.hpp -- outlier_removal() of data_read.py:103-128: stand-alone (k_outlier); k_mask<1>/<2> apply it in front of the predicates
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// outlier_removal() zeroes a pixel when (v - mean) > 1.0 with mean = sum / (count + 1e-5) over the 25 taps of the 7x7
// diamond (cv2.filter2D: reflect-101 border, float32 accumulation in kernel row-major order -- what OpenCV's direct
// filter does; mean, difference and test in float64 -- numpy's promotion).
// Only pixels with v > 1.0 can be zeroed as long as no tap is negative (then mean >= 0, or NaN and the test is false), so
// the 25 taps are only gathered for those (a few percent of a LiDAR frame).  A negative value anywhere switches to the
// exhaustive evaluation: per tile in k_outlier, per frame (a second launch) in k_mask.
// ------------------------------------------------------------------------------------------------
constexpr int O_TH = 16, O_TW = 128;

// k_outlier: one block per 16 x 128 tile staged in LDS with a 3-cell halo; candidates (v > 1.0, or every pixel when the
// staged tile holds a negative value) are compacted so that every lane evaluates one.
__global__ __launch_bounds__(256) void k_outlier(const float *__restrict__ x, int H, int W,
                                                 float *__restrict__ out) {
    __shared__ float s_t[(O_TH + 6) * (O_TW + 6)];
    __shared__ u16 s_list[O_TH * O_TW];
    __shared__ int s_n, s_neg;
    const int b = blockIdx.z, r0 = blockIdx.y * O_TH, c0 = blockIdx.x * O_TW;
    const float *xf = x + (size_t)b * H * W;
    if (threadIdx.x == 0) s_n = s_neg = 0;
    __syncthreads();
    bool neg = false;
    {
        // every load of the thread first (independent: one round trip instead of seven), then the tile
        constexpr int NIT = (O_TH + 6) * (O_TW + 6), PER = (NIT + 255) / 256;
        float lv[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int k = min((int)threadIdx.x + 256 * q, NIT - 1);
            const int r = k / (O_TW + 6), c = k - r * (O_TW + 6);
            const int gi = reflect101(min(r0 + r - 3, H + 2), H), gj = reflect101(min(c0 + c - 3, W + 2), W);
            lv[q] = xf[(size_t)gi * W + gj];
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int k = (int)threadIdx.x + 256 * q;
            if (k < NIT) {
                neg |= lv[q] < 0.0f;
                s_t[k] = lv[q];
            }
        }
    }
    if (__any(neg) && (threadIdx.x & 63) == 0) s_neg = 1;
    __syncthreads();
    const bool all = s_neg != 0;
    for (int k = threadIdx.x; k < O_TH * O_TW; k += 256) {  // the other pixels go out unchanged, candidates are listed
        const int r = k / O_TW, c = k - r * O_TW;
        const int gi = r0 + r, gj = c0 + c;
        const bool in = gi < H && gj < W;
        const float v = s_t[(r + 3) * (O_TW + 6) + c + 3];
        const bool cand = in && (all || v > 1.0f);
        if (in && !cand) out[(size_t)b * H * W + (size_t)gi * W + gj] = v;  // a candidate is stored by the lane that evaluates it
        const u64 bal = __ballot(cand);
        int base = 0;
        if ((threadIdx.x & 63) == 0 && bal) base = atomicAdd(&s_n, __popcll(bal));
        base = __builtin_amdgcn_readfirstlane(base);
        if (cand) s_list[base + (int)__builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u))] = (u16)k;
    }
    __syncthreads();
    const int n = s_n;
    for (int t = threadIdx.x; t < n; t += 256) {
        const int k = s_list[t], r = k / O_TW, c = k - r * O_TW;
        const bool drop = is_outlier([&](int ti, int tj) { return s_t[(r + ti) * (O_TW + 6) + c + tj]; });
        const float v = s_t[(r + 3) * (O_TW + 6) + c + 3];
        out[(size_t)b * H * W + (size_t)(r0 + r) * W + c0 + c] = drop ? v * 0.0f : v;  // data_read.py:128 multiplies by (1 - flag): a removed negative pixel is -0.0
    }
}

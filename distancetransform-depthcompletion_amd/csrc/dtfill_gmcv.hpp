// dtfill_gmcv.hpp -- k_gmcv7 / k_gmcv / k_gmcv_first: demo.py's value-weighted generate_multi_channel(), demo.py:108-198
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// One step of the demo driver's windowed fill (the contract is in include/dtfill.h, dtfill_demo_multi_channel): over the
// ts x ts window (zero padding), p = d * w with w = (float)10^(ts - |di| - |dj|) (demo.py:65-75); the selected taps are those
// whose p equals the window maximum (all ts^2 taps, padding included; a NaN product is skipped by the maximum and equals
// nothing); raw = (float32 sum of d over the selected taps in row-major order) / (1e-6 + count), count = the selected taps
// with d != 0.  A selected tap has d != 0 exactly when the maximum is not 0 (p = 0 needs d = 0: 10 * |d| does not underflow),
// so count = (mx != 0 ? selected taps : 0).  Unselected taps add +0 to the sum, which changes no value (a -0 sum becomes +0;
// the two compare equal, here and in every later step).
// Same 16 x 64 tile as k_gmc, the data tile alone with a (ts-1)/2 halo in LDS.  The tiles are numbered in one dimension
// (tile column fastest, then tile row, then frame) and a block takes tiles blockIdx.x, + gridDim.x, ...: no limit on B
// beyond B*H*W < 2^31, and the host may cap the grid.
//
// FORM: how a pixel goes out, fused into the step (GV_PLAIN: out[at] = raw / sr; GV_RGB3: rgb has 3 channels and out is
// 16-byte aligned, the pixel {rgb / sr, (raw / sr) / sr} is one 16-byte store; GV_RGBC: any channel count, dword stores).
// raw itself is stored (raw_out) only when a later step reads it.
enum { GV_PLAIN = 0, GV_RGB3 = 1, GV_RGBC = 2 };
constexpr u32 GV_WALK_MAX = 30;  // k_gmcv7 walks rings of up to this many taps in all, beyond that all 49 taps

// px: this pixel's C rgb values (memory or registers)
template <int FORM>
__device__ __forceinline__ void gmcv_emit(float raw, size_t at, const float *px, int C, float sr, float *__restrict__ raw_out,
                                          float *__restrict__ out) {
    if (raw_out) raw_out[at] = raw;
    const float v = __fdiv_rn(raw, sr);
    if (FORM == GV_PLAIN) {
        out[at] = v;
    } else if (FORM == GV_RGB3) {
        float4 o;
        o.x = __fdiv_rn(px[0], sr);
        o.y = __fdiv_rn(px[1], sr);
        o.z = __fdiv_rn(px[2], sr);
        o.w = __fdiv_rn(v, sr);  // demo.py:172-173 then :198: the lidar channel is divided twice
        *reinterpret_cast<float4 *>(out + at * 4) = o;
    } else {
        float *o = out + at * (size_t)(C + 1);
        for (int ch = 0; ch < C; ++ch) o[ch] = __fdiv_rn(px[ch], sr);
        o[C] = __fdiv_rn(v, sr);
    }
}

// (float)10^e, e = 0 .. 15: the decimal literal is rounded to float32 once, as (float)(double)10^e is (10^e is exact in double)
__device__ __forceinline__ float gmcv_pow10(int e) {
    constexpr float t[16] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f, 1e11f, 1e12f, 1e13f, 1e14f, 1e15f};
    return t[e];
}

// stage the PH x PW tile whose first pixel is (r0 - half, c0 - half) of frame `src`; outside the frame: +0
__device__ __forceinline__ void gmcv_stage(const float *__restrict__ src, int H, int W, int r0, int c0, int half, int PH, int PW,
                                           float *s_d) {
    for (int k = threadIdx.x; k < PH * PW; k += 256) {
        const int r = k / PW, c = k - r * PW;
        const int gi = r0 + r - half, gj = c0 + c - half;
        const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W;
        s_d[k] = in ? src[(size_t)gi * W + gj] : 0.0f;
    }
}

// table_size 7 (every model of the reference), compile-time unrolled.  A thread owns four vertically adjacent pixels (wave w:
// tile rows 4w .. 4w+3, a lane per column) and reads their 10 x 7 taps from LDS once.  Per pixel:
//   the maximum by rings: rounding is monotonic, so max over a ring of fl(d * w) = fl(w * max over the ring of d) -- 48 maxima
//   (three-operand) and 7 multiplies instead of 49 of each;
//   then in tap order: p = fl(d * w), selected iff p == mx, sum += selected ? d : 0, n += selected -- over the taps of the
//   rings that reach mx in some lane of the wave (on filled frames mostly the pixel itself and its four neighbours), or over
//   all 49 when a lane's maximum is reached in more than one ring.
template <int FORM>
__global__ __launch_bounds__(256) void k_gmcv7(const float *__restrict__ src, const float *__restrict__ rgb, int C, int H, int W,
                                               int tx, int ty, u32 ntiles, float sr, float *__restrict__ raw_out,
                                               float *__restrict__ out) {
    constexpr int half = 3, PW = GM_TW + 6, PH = GM_TH + 6, NQ = 4;
    static_assert(GM_TH == 16 && GM_TW == 64, "four waves, four rows each, a lane per column");
    __shared__ float s_d[PH * PW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (one round unless the grid was capped)
        const int bx = tile % (u32)tx, by = tile / (u32)tx % (u32)ty, b = tile / (u32)tx / (u32)ty;
        const int r0 = by * GM_TH, c0 = bx * GM_TW;
        const size_t fo = (size_t)b * H * W;
        const int gj = c0 + lane, gi0 = r0 + NQ * wave;
        gmcv_stage(src + fo, H, W, r0, c0, half, PH, PW, s_d);
        [[maybe_unused]] float px[FORM == GV_RGB3 ? NQ : 1][3] = {};  // the pixels' rgb, held only by the one-store form
        if constexpr (FORM == GV_RGB3) {  // issued before the barrier: back by the time the pixels go out
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (gi0 + q < H && gj < W) {
                    const float *p = rgb + (fo + (size_t)(gi0 + q) * W + gj) * 3;
                    px[q][0] = p[0];
                    px[q][1] = p[1];
                    px[q][2] = p[2];
                }
        }
        __syncthreads();
        float d[NQ + 6][7];
#pragma unroll
        for (int i = 0; i < NQ + 6; ++i)
#pragma unroll
            for (int j = 0; j < 7; ++j) d[i][j] = s_d[(NQ * wave + i) * PW + lane + j];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float ring[7];
#pragma unroll
            for (int s = 0; s < 7; ++s) ring[s] = -INFINITY;
#pragma unroll
            for (int i = 0; i < 7; ++i)
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const int s = (i < 3 ? 3 - i : i - 3) + (j < 3 ? 3 - j : j - 3);
                    ring[s] = fmaxf(ring[s], d[q + i][j]);  // (skips a NaN)
                }
            float rp[7], mx = -INFINITY;
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                rp[s] = __fmul_rn(ring[s], gmcv_pow10(7 - s));
                mx = fmaxf(mx, rp[s]);
            }
            // Which rings hold a selected tap, as lane masks (none for mx == 0: its result is 0 whatever is selected).  Where no lane
            // selects from two rings, only the rings some lane selects from need walking, each in tap order: what a lane adds
            // outside its own ring is +0, so its sum is still the one in tap order.  Worth it when those rings are few.
            const u64 nz = __ballot(mx != 0.0f);
            u64 seen = 0, twice = 0;
            u32 rings = 0, taps = 0;
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const u64 h = __ballot(rp[s] == mx) & nz;
                twice |= seen & h;
                seen |= h;
                if (h) {
                    rings |= 1u << s;
                    taps += s == 0 ? 1 : s < 4 ? 4 * s : 4 * (7 - s);  // (the ring's taps inside the 7 x 7 window)
                }
            }
            float acc = 0.0f;
            int n = 0;
            if (twice == 0 && taps <= GV_WALK_MAX) {  // wave-uniform
#pragma unroll
                for (int s = 0; s < 7; ++s) {
                    if (!(rings >> s & 1u)) continue;
#pragma unroll
                    for (int i = 0; i < 7; ++i)
#pragma unroll
                        for (int j = 0; j < 7; ++j) {
                            if ((i < 3 ? 3 - i : i - 3) + (j < 3 ? 3 - j : j - 3) != s) continue;
                            const float v = d[q + i][j];
                            const bool sel = __fmul_rn(v, gmcv_pow10(7 - s)) == mx;  // (never in a ring the lane does not select from)
                            acc = __fadd_rn(acc, sel ? v : 0.0f);
                            n += sel ? 1 : 0;
                        }
                }
            } else {
                // all 49 taps in order
#pragma unroll
                for (int i = 0; i < 7; ++i)
#pragma unroll
                    for (int j = 0; j < 7; ++j) {
                        const int s = (i < 3 ? 3 - i : i - 3) + (j < 3 ? 3 - j : j - 3);
                        const float v = d[q + i][j];
                        const bool sel = __fmul_rn(v, gmcv_pow10(7 - s)) == mx;
                        acc = __fadd_rn(acc, sel ? v : 0.0f);
                        n += sel ? 1 : 0;
                    }
            }
            const float cnt = mx != 0.0f ? (float)n : 0.0f;
            const float raw = __fdiv_rn(acc, __fadd_rn(0.000001f, cnt));
            if (gi0 + q < H && gj < W) {
                const size_t at = fo + (size_t)(gi0 + q) * W + gj;
                const float *pp = nullptr;  // GV_PLAIN reads no rgb
                if constexpr (FORM == GV_RGB3) pp = px[q];
                if constexpr (FORM == GV_RGBC) pp = rgb + at * (size_t)C;
                gmcv_emit<FORM>(raw, at, pp, C, sr, raw_out, out);
            }
        }
        __syncthreads();  // the tile is read: the next round may stage
    }
}

// any odd table size up to 15: the window maximum, then sum and count of the taps that reach it, from LDS
template <int FORM>
__global__ __launch_bounds__(256) void k_gmcv(const float *__restrict__ src, const float *__restrict__ rgb, int C, int H, int W,
                                              int ts, int tx, int ty, u32 ntiles, float sr, float *__restrict__ raw_out,
                                              float *__restrict__ out) {
    __shared__ float s_d[(GM_TH + 2 * GM_MAXHALF) * (GM_TW + 2 * GM_MAXHALF)];
    __shared__ float s_w[16];
    const int half = (ts - 1) / 2;
    const int PW = GM_TW + 2 * half, PH = GM_TH + 2 * half;
    if (threadIdx.x < 16) s_w[threadIdx.x] = gmcv_pow10(threadIdx.x);
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int bx = tile % (u32)tx, by = tile / (u32)tx % (u32)ty, b = tile / (u32)tx / (u32)ty;
        const int r0 = by * GM_TH, c0 = bx * GM_TW;
        const size_t fo = (size_t)b * H * W;
        gmcv_stage(src + fo, H, W, r0, c0, half, PH, PW, s_d);
        __syncthreads();
        for (int k = threadIdx.x; k < GM_TH * GM_TW; k += 256) {
            const int r = k / GM_TW, c = k - r * GM_TW;
            const int gi = r0 + r, gj = c0 + c;
            if (gi >= H || gj >= W) continue;
            float mx = -INFINITY;
            for (int i = 0; i < ts; ++i)
                for (int j = 0; j < ts; ++j)
                    mx = fmaxf(mx, __fmul_rn(s_d[(r + i) * PW + c + j], s_w[ts - abs(i - half) - abs(j - half)]));
            float acc = 0.0f;
            int n = 0;
            for (int i = 0; i < ts; ++i)
                for (int j = 0; j < ts; ++j) {
                    const float v = s_d[(r + i) * PW + c + j];
                    const bool sel = __fmul_rn(v, s_w[ts - abs(i - half) - abs(j - half)]) == mx;
                    acc = __fadd_rn(acc, sel ? v : 0.0f);
                    n += sel ? 1 : 0;
                }
            const float cnt = mx != 0.0f ? (float)n : 0.0f;
            const size_t at = fo + (size_t)gi * W + gj;
            gmcv_emit<FORM>(__fdiv_rn(acc, __fadd_rn(0.000001f, cnt)), at, FORM == GV_PLAIN ? nullptr : rgb + at * (size_t)C, C, sr,
                            raw_out, out);
        }
        __syncthreads();
    }
}

// out_1: raw_1 is the input itself, only the divided output goes out (demo.py:120,143 / :163-164,192)
template <int FORM>
__global__ __launch_bounds__(256) void k_gmcv_first(const float *__restrict__ src, const float *__restrict__ rgb, int C, size_t n,
                                                    float sr, float *__restrict__ out) {
    for (size_t at = (size_t)blockIdx.x * 256 + threadIdx.x; at < n; at += (size_t)gridDim.x * 256)
        gmcv_emit<FORM>(src[at], at, FORM == GV_PLAIN ? nullptr : rgb + at * (size_t)C, C, sr, nullptr, out);
}

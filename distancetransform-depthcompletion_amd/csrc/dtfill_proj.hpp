// dtfill_proj.hpp -- LiDAR point projection: point clouds in the Velodyne frame to sparse depth frames, the
// map_points_on_image() that subsample_Lidar_{train,val}.py end in, and its z-buffered form (include/dtfill.h has the
// contract).  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// Four launches; the launch boundaries are the only hand-offs between workgroups:
//   k_proj_clear    the per-pixel keys (REFERENCE: u32 0, ZBUFFER: u64 all ones) and the per-frame accumulators, 16 bytes a lane.
//   k_proj_scatter  one lane per point: a block copies its PJ_TILE records into LDS with coalesced dword loads (any stride, any
//                   element alignment, never a record beyond n_b), every lane projects its point in float64 and takes ONE
//                   integer atomic on its pixel's key:
//                     REFERENCE  max of i + 1 (u32): the last writer of numpy's in-order assignment;
//                     ZBUFFER    min of the bit pattern of z (u64): z > min_z >= 0, and positive doubles order as their bits.
//                                Points of equal z have equal bits, so the rule "largest i among them" picks the same value
//                                whichever of them is taken: no second key is kept.
//                   A block beyond its frame's n_b leaves at once.  The counters are summed per wave (ballot), then per block
//                   in LDS: the frame's accumulators see one atomic per block.
//   k_proj_resolve  one lane per pixel: REFERENCE projects the winner's record again (the same code, the same bits), ZBUFFER
//                   reads z out of the key; stores both outputs; counts the written pixels.  An index-error or bad-count frame
//                   is all +0.0: the flag is complete when this launch starts, so it reaches every pixel.
//   k_proj_finish   one lane per frame: status and the four counts.
// Integer max / min / add / or only: the result does not depend on the order in which the atomics arrive.
// ------------------------------------------------------------------------------------------------
constexpr int PJ_TILE = 256;             // points k_proj_scatter's block projects at a time (one per lane)
constexpr int PJ_BLOCK = 8 * PJ_TILE;    // ... and in all
constexpr int PJ_PIXELS = 16 * 256;      // pixels per block of k_proj_resolve
constexpr int PJ_ACC = 8;     // int32 per frame in the workspace: DTFILL_PROJ_* counts (4), the index-error flag
constexpr int PJ_ERR = 4;

// the calibration of one frame: K row-major (9), rows 0..2 of E (12); uniform loads, held in SGPRs
struct PjCal {
    double k[9], e[12];
};

__device__ __forceinline__ PjCal pj_cal(const double *__restrict__ K, const double *__restrict__ E, int b) {
    PjCal c;
#pragma unroll
    for (int j = 0; j < 9; ++j) c.k[j] = K[(size_t)b * 9 + j];
#pragma unroll
    for (int j = 0; j < 12; ++j) c.e[j] = E[(size_t)b * 16 + j];
    return c;
}

// h = K (E [X Y Z 1]^T)[0:3]: every operation rounded on its own, left to right as the contract writes them, so that the
// scatter and the resolve launches compute the same bits for the same record
__device__ __forceinline__ void pj_project(const PjCal &c, double X, double Y, double Z, double &z, double &u, double &v) {
#pragma clang fp contract(off)
    const double c0 = c.e[0] * X + c.e[1] * Y + c.e[2] * Z + c.e[3];
    const double c1 = c.e[4] * X + c.e[5] * Y + c.e[6] * Z + c.e[7];
    const double c2 = c.e[8] * X + c.e[9] * Y + c.e[10] * Z + c.e[11];
    const double h0 = c.k[0] * c0 + c.k[1] * c1 + c.k[2] * c2;
    const double h1 = c.k[3] * c0 + c.k[4] * c1 + c.k[5] * c2;
    z = c.k[6] * c0 + c.k[7] * c1 + c.k[8] * c2;
    u = rint(h0 / z);
    v = rint(h1 / z);
}

__device__ __forceinline__ bool pj_finite(double a) { return fabs(a) < __builtin_inf(); }  // false for a NaN

// frame b's record count: counts[b], or N without counts; -1 for a count outside [0, N]
__device__ __forceinline__ int pj_count(const int32_t *__restrict__ counts, int b, int N) {
    if (!counts) return N;
    const int n = counts[b];
    return n < 0 || n > N ? -1 : n;
}

// n16 16-byte words of keys = fill, and the B * PJ_ACC accumulators = 0
__global__ __launch_bounds__(256) void k_proj_clear(uint4 *__restrict__ keys, size_t n16, u32 fill, int *__restrict__ acc, int nacc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) keys[i] = make_uint4(fill, fill, fill, fill);
    if (i < (size_t)nacc) acc[i] = 0;
}

// points [blockIdx.x * PJ_BLOCK, +PJ_BLOCK) of frame blockIdx.y, a tile of PJ_TILE at a time.  What a block counts goes to
// the frame's accumulators once, at its end: one atomic per wave on the same few addresses was most of this kernel's time.
template <int MODE>
__global__ __launch_bounds__(PJ_TILE) void k_proj_scatter(const float *__restrict__ points, const int32_t *__restrict__ counts,
                                                          int N, int stride, int H, int W, const double *__restrict__ K,
                                                          const double *__restrict__ E, float min_z, void *__restrict__ keys,
                                                          int *__restrict__ acc) {
    __shared__ float s_rec[PJ_TILE * 4];
    __shared__ int s_cnt[4];  // REFERENCE: [0] a point outside the wrap range; ZBUFFER: inside, behind, outside
    const int t = threadIdx.x, b = blockIdx.y;
    const int nb = pj_count(counts, b, N);
    const int first = blockIdx.x * PJ_BLOCK;
    if (first >= nb) return;  // (a bad count too)
    const int last = min(nb, first + PJ_BLOCK);
    if (t < 4) s_cnt[t] = 0;  // (ordered before its first use by the barrier behind the first tile's copy)
    const PjCal c = pj_cal(K, E, b);
    const size_t HW = (size_t)H * W;
    for (int base = first; base < last; base += PJ_TILE) {
        const int cnt = min(PJ_TILE, last - base);
        const float *src = points + ((size_t)b * N + base) * stride;
        for (int k = t; k < cnt * stride; k += PJ_TILE) s_rec[k] = src[k];
        __syncthreads();
        const bool live = t < cnt;
        double z = 0.0, u = 0.0, v = 0.0;
        bool fin = false;
        if (live) {
            const double X = (double)s_rec[t * stride], Y = (double)s_rec[t * stride + 1], Z = (double)s_rec[t * stride + 2];
            fin = pj_finite(X) && pj_finite(Y) && pj_finite(Z);
            pj_project(c, X, Y, Z, z, u, v);
        }
        if (MODE == DTFILL_PROJ_REFERENCE) {
            const bool ok = pj_finite(u) && pj_finite(v) && u >= -(double)W && u < (double)W && v >= -(double)H && v < (double)H;
            if (live && ok) {
                int ui = (int)u, vi = (int)v;
                ui += ui < 0 ? W : 0;
                vi += vi < 0 ? H : 0;
                atomicMax(static_cast<u32 *>(keys) + (size_t)b * HW + (size_t)vi * W + ui, (u32)(base + t + 1));
            }
            if (__ballot(live && !ok) && (t & 63) == 0) atomicOr(&s_cnt[0], 1);
        } else {
            const bool front = live && fin && pj_finite(z) && z > (double)min_z;
            const bool in = front && pj_finite(u) && pj_finite(v) && u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H;
            if (in)
                atomicMin(static_cast<u64 *>(keys) + (size_t)b * HW + (size_t)(int)v * W + (int)u, (u64)__double_as_longlong(z));
            const int n_in = __popcll(__ballot(in)), n_behind = __popcll(__ballot(live && !front)),
                      n_out = __popcll(__ballot(front && !in));
            if ((t & 63) == 0) {
                if (n_in) atomicAdd(&s_cnt[0], n_in);
                if (n_behind) atomicAdd(&s_cnt[1], n_behind);
                if (n_out) atomicAdd(&s_cnt[2], n_out);
            }
        }
        __syncthreads();  // the records are rewritten by the next tile; the block's counts are complete behind the last one
    }
    if (MODE == DTFILL_PROJ_REFERENCE) {
        if (t == 0 && s_cnt[0]) atomicOr(acc + b * PJ_ACC + PJ_ERR, 1);
    } else {
        static_assert(DTFILL_PROJ_INSIDE == 1 && DTFILL_PROJ_BEHIND == 2 && DTFILL_PROJ_OUTSIDE == 3, "s_cnt[k] is column k + 1");
        if (t < 3 && s_cnt[t]) atomicAdd(acc + b * PJ_ACC + 1 + t, s_cnt[t]);
    }
}

// pixels [blockIdx.x * PJ_PIXELS, +PJ_PIXELS) of frame blockIdx.y, 256 at a time; the block's count of written pixels goes to
// the frame's accumulator once
template <int MODE>
__global__ __launch_bounds__(256) void k_proj_resolve(const float *__restrict__ points, const int32_t *__restrict__ counts, int N,
                                                      int stride, int HW, const double *__restrict__ K,
                                                      const double *__restrict__ E, const void *__restrict__ keys,
                                                      int *__restrict__ acc, float *__restrict__ out_f32,
                                                      double *__restrict__ out_f64) {
    __shared__ int s_hit;
    const int t = threadIdx.x, b = blockIdx.y;
    const bool dead = pj_count(counts, b, N) < 0 || (MODE == DTFILL_PROJ_REFERENCE && acc[b * PJ_ACC + PJ_ERR] != 0);
    const PjCal c = pj_cal(K, E, b);
    if (t == 0) s_hit = 0;
    __syncthreads();
    const int p0 = blockIdx.x * PJ_PIXELS, len = min(PJ_PIXELS, HW - p0);
    int n_hit = 0;  // of this lane's wave
    for (int off = t; off - t < len; off += 256) {  // (every lane takes every step: whole waves reach the ballot)
        const bool live = off < len;
        const int p = p0 + (live ? off : 0);
        double z = 0.0;
        bool hit = false;
        if (live && !dead) {
            if (MODE == DTFILL_PROJ_REFERENCE) {
                const u32 key = static_cast<const u32 *>(keys)[(size_t)b * HW + p];
                if (key) {
                    const float *r = points + ((size_t)b * N + (key - 1)) * stride;
                    double u, v;
                    pj_project(c, (double)r[0], (double)r[1], (double)r[2], z, u, v);
                    hit = true;
                }
            } else {
                const u64 key = static_cast<const u64 *>(keys)[(size_t)b * HW + p];
                if (key != ~0ull) {
                    z = __longlong_as_double((long long)key);
                    hit = true;
                }
            }
        }
        if (live) {
            if (out_f32) out_f32[(size_t)b * HW + p] = (float)z;
            if (out_f64) out_f64[(size_t)b * HW + p] = z;
        }
        n_hit += __popcll(__ballot(hit));
    }
    if (n_hit && (t & 63) == 0) atomicAdd(&s_hit, n_hit);
    __syncthreads();
    if (t == 0 && s_hit) atomicAdd(acc + b * PJ_ACC + DTFILL_PROJ_PIXELS, s_hit);
}

// frame t's status and counts
template <int MODE>
__global__ __launch_bounds__(256) void k_proj_finish(const int32_t *__restrict__ counts, int B, int N, const int *__restrict__ acc,
                                                     int32_t *__restrict__ frame_status, int32_t *__restrict__ frame_counts) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int nb = pj_count(counts, b, N);
    int c[DTFILL_PROJ_N] = {0, 0, 0, 0};
    int st = 0;
    if (nb < 0) {
        st = DTFILL_PROJ_BAD_COUNT;
    } else if (MODE == DTFILL_PROJ_REFERENCE && acc[b * PJ_ACC + PJ_ERR]) {
        st = DTFILL_PROJ_INDEX_ERROR;
    } else {
#pragma unroll
        for (int k = 0; k < DTFILL_PROJ_N; ++k) c[k] = acc[b * PJ_ACC + k];
        if (MODE == DTFILL_PROJ_REFERENCE) c[DTFILL_PROJ_INSIDE] = nb;  // every point of a valid frame lands
        if (c[DTFILL_PROJ_INSIDE] == 0) st = DTFILL_PROJ_NO_POINTS;
    }
    if (frame_status) frame_status[b] = st;
    if (frame_counts)
#pragma unroll
        for (int k = 0; k < DTFILL_PROJ_N; ++k) frame_counts[b * DTFILL_PROJ_N + k] = c[k];
}

// the four launches of one call; keys and acc: the two pieces of the workspace
template <int MODE>
void proj_launch(hipStream_t st, const float *points, const int32_t *counts, int B, int N, int stride, int H, int W,
                        const double *K, const double *E, float min_z, float *out_f32, double *out_f64, int32_t *frame_status,
                        int32_t *frame_counts, void *keys, int *acc) {
    const size_t HW = (size_t)H * W;
    const size_t n16 = (B * HW * (MODE == DTFILL_PROJ_REFERENCE ? sizeof(u32) : sizeof(u64)) + 15) / 16;
    const int nacc = B * PJ_ACC;
    k_proj_clear<<<(unsigned)((max(n16, (size_t)nacc) + 255) / 256), 256, 0, st>>>(
        static_cast<uint4 *>(keys), n16, MODE == DTFILL_PROJ_REFERENCE ? 0u : ~0u, acc, nacc);
    k_proj_scatter<MODE><<<dim3((N + PJ_BLOCK - 1) / PJ_BLOCK, B), PJ_TILE, 0, st>>>(points, counts, N, stride, H, W, K, E, min_z,
                                                                                  keys, acc);
    k_proj_resolve<MODE><<<dim3((unsigned)((HW + PJ_PIXELS - 1) / PJ_PIXELS), B), 256, 0, st>>>(points, counts, N, stride, (int)HW, K, E, keys, acc,
                                                                               out_f32, out_f64);
    if (frame_status || frame_counts)
        k_proj_finish<MODE><<<(B + 255) / 256, 256, 0, st>>>(counts, B, N, acc, frame_status, frame_counts);
}

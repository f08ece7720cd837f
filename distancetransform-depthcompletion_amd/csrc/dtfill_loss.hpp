// dtfill_loss.hpp -- the masked training losses of the reference's training step, solution_DeepNet/train.py:210-251, and their
// gradient.  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// train.py:215-251 on float32 [B,H,W] frames (include/dtfill.h states the contract):
//   m  = gt > gt_thr;  mi = m && lidar > in_thr          float32 compares, derived while the inputs are read, never stored
//   S_main = sum over m inside the window of (pred - gt)^2;   S_aux = sum over mi of (corr - gt)^2 + |corr - gt|
//   n_gt, n_in  the sizes of m and mi over the whole batch (the window does not apply to either)
// Per element float32, one rounding per operation, plain operators under fp contract(off) (dtfill_post.hpp says why the
// intrinsics do not suffice); a term is added only where it is selected, so a non-finite pred or corr at an unselected pixel
// leaves no trace.  The sums accumulate in float64, the counts in integers.
//
// The partition is a function of N = B*H*W alone: the batch is one run of N elements cut into chunks of L_CHUNK = 1024, chunk
// c goes to block c mod nb (nb = loss_blocks(N) <= L_MAXB), and lane t of the block owns elements 4t .. 4t+3 of the chunk.  A
// lane adds its terms in ascending element order, chunk after chunk; a block adds its lanes by the shuffle tree and its four
// waves in order; k_loss_final adds the blocks' partials, lane l those of blocks l, l + 64, .. in ascending order, then the
// same tree.  No atomics: two calls give the same bits, and the 16-byte loads (VEC: every pointer 16-byte aligned and N a
// multiple of 4) read the elements the dword loads read, so alignment does not change a bit either.
constexpr int L_CHUNK = 1024;  // elements per block and trip: 256 lanes x 4
constexpr int L_MAXB = 1024;   // blocks of the forward launch (four per CU), each striding over the chunks
constexpr int L_BWD_MAXB = 2048;  // blocks of the backward launch: no sum, so no order to keep

inline int loss_blocks(size_t n) { return (int)min((n + L_CHUNK - 1) / L_CHUNK, (size_t)L_MAXB); }

struct LossWindow {
    int H, W, r0, r1, c0, c1;
};

// The four elements a lane owns, as one 16-byte load or four dword loads of the same addresses; beyond n: zeros.
template <bool VEC>
__device__ __forceinline__ void loss_load4(const float *__restrict__ p, size_t at, size_t n, float v[4]) {
    if (VEC) {
        const float4 q = at < n ? *reinterpret_cast<const float4 *>(p + at) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = at + u < n ? p[at + u] : 0.0f;
    }
}

// Which of the lane's four elements lie inside the window of the main sum (bit u: element at + u).
__device__ __forceinline__ u32 loss_in_window(const LossWindow w, size_t at) {
    const u32 row = (u32)at / (u32)w.W;  // the row within the batch (at < 2^31: a 32-bit division)
    int j = (int)((u32)at - row * (u32)w.W), i = (int)(row % (u32)w.H);
    u32 bits = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        bits |= (i >= w.r0 && i < w.r1 && j >= w.c0 && j < w.c1) ? 1u << u : 0u;
        if (++j == w.W) {
            j = 0;
            if (++i == w.H) i = 0;
        }
    }
    return bits;
}

// Stage 1.  part_s: double [nb][2] (S_main, S_aux); part_n: u32 [nb][2] (n_gt, n_in), one row per block.
// AUX: corr and lidar are given; WIN: the window is not the whole frame.
template <bool AUX, bool WIN, bool VEC>
__global__ __launch_bounds__(256) void k_loss_part(const float *__restrict__ pred, const float *__restrict__ corr,
                                                   const float *__restrict__ gt, const float *__restrict__ lidar, size_t n,
                                                   const LossWindow w, float gt_thr, float in_thr,
                                                   double *__restrict__ part_s, u32 *__restrict__ part_n) {
#pragma clang fp contract(off)
    double sm = 0.0, sa = 0.0;
    u32 ng = 0, ni = 0;
    for (size_t base = (size_t)blockIdx.x * L_CHUNK; base < n; base += (size_t)gridDim.x * L_CHUNK) {
        const size_t at = base + 4 * threadIdx.x;
        float p[4], g[4], c[4], l[4];
        loss_load4<VEC>(pred, at, n, p);
        loss_load4<VEC>(gt, at, n, g);
        if (AUX) {
            loss_load4<VEC>(corr, at, n, c);
            loss_load4<VEC>(lidar, at, n, l);
        }
        const u32 win = WIN ? loss_in_window(w, at) : 0xFu;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool m = at + u < n && g[u] > gt_thr;  // train.py:215 / :220
            const float t = p[u] - g[u];
            const float e = t * t;  // :240
            sm += (m && (win >> u & 1u)) ? (double)e : 0.0;
            ng += m ? 1u : 0u;
            if (AUX) {
                const bool mi = m && l[u] > in_thr;  // :216 / :221, :227
                const float d = c[u] - g[u];
                const float a = d * d + fabsf(d);  // :248
                sa += mi ? (double)a : 0.0;
                ni += mi ? 1u : 0u;
            }
        }
    }
    // block sum in a fixed order: lanes (shuffle tree), then the four waves
    __shared__ double s_s[4][2];
    __shared__ u32 s_n[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sm += __shfl_down(sm, off);
        sa += __shfl_down(sa, off);
        ng += __shfl_down(ng, off);
        ni += __shfl_down(ni, off);
    }
    if (lane == 0) {
        s_s[wave][0] = sm, s_s[wave][1] = sa;
        s_n[wave][0] = ng, s_n[wave][1] = ni;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part_s[(size_t)blockIdx.x * 2 + k] = ((s_s[0][k] + s_s[1][k]) + s_s[2][k]) + s_s[3][k];
        part_n[(size_t)blockIdx.x * 2 + k] = s_n[0][k] + s_n[1][k] + s_n[2][k] + s_n[3][k];
    }
}

// Stage 2: one wave adds the nb partials in index order and writes the six columns of stats.
__global__ __launch_bounds__(64) void k_loss_final(const double *__restrict__ part_s, const u32 *__restrict__ part_n, int nb,
                                                   int kind, int aux, double *__restrict__ stats) {
    const int lane = threadIdx.x;
    double sm = 0.0, sa = 0.0;
    u32 ng = 0, ni = 0;  // (< 2^31 elements in all)
    for (int q = lane; q < nb; q += 64) {
        sm += part_s[2 * q], sa += part_s[2 * q + 1];
        ng += part_n[2 * q], ni += part_n[2 * q + 1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sm += __shfl_down(sm, off);
        sa += __shfl_down(sa, off);
        ng += __shfl_down(ng, off);
        ni += __shfl_down(ni, off);
    }
    if (lane == 0) {
        const double q = sm / (double)ng;  // an empty mask: 0 / 0 = NaN, like the reference
        stats[0] = kind == DTFILL_LOSS_NYU ? sqrt(q) : q;  // train.py:242 / :244
        stats[1] = aux ? sa / (double)ni : 0.0;            // :249
        stats[2] = (double)ng;
        stats[3] = aux ? (double)ni : 0.0;
        stats[4] = sm;
        stats[5] = aux ? sa : 0.0;
    }
}

// The four results of a lane, as one 16-byte store or dword stores of the same addresses.
template <bool VEC>
__device__ __forceinline__ void loss_store4(float *__restrict__ p, size_t at, size_t n, const float v[4]) {
    if (VEC) {
        if (at < n) *reinterpret_cast<float4 *>(p + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (at + u < n) p[at + u] = v[u];
    }
}

// Backward: grad_pred = (2 t) k_main where m inside the window, grad_corr = (2 u + sgn u) k_aux where mi, +0.0f elsewhere; both
// outputs (those that are given) fully overwritten.  k_main and k_aux come from stats and the device scalars g_main / g_aux:
// one double division each, rounded to float32 once.  A NULL g_* is a zero gradient: that output is all +0 and the inputs
// only it needs are not read.
template <bool WIN, bool VEC>
__global__ __launch_bounds__(256) void k_loss_bwd(const float *__restrict__ pred, const float *__restrict__ corr,
                                                  const float *__restrict__ gt, const float *__restrict__ lidar, size_t n,
                                                  const LossWindow w, int kind, float gt_thr, float in_thr,
                                                  const double *__restrict__ stats, const float *__restrict__ g_main,
                                                  const float *__restrict__ g_aux, float *__restrict__ grad_pred,
                                                  float *__restrict__ grad_corr) {
#pragma clang fp contract(off)
    const bool do_main = grad_pred && g_main, do_aux = grad_corr && g_aux;
    float k_main = 0.0f, k_aux = 0.0f;
    if (do_main) {
        const double ng = stats[2];
        k_main = kind == DTFILL_LOSS_NYU ? (float)((double)*g_main / ((2.0 * stats[0]) * ng)) : (float)((double)*g_main / ng);
    }
    if (do_aux) k_aux = (float)((double)*g_aux / stats[3]);
    for (size_t base = (size_t)blockIdx.x * L_CHUNK; base < n; base += (size_t)gridDim.x * L_CHUNK) {
        const size_t at = base + 4 * threadIdx.x;
        float g[4], x[4], l[4], out[4];
        if (do_main || do_aux) loss_load4<VEC>(gt, at, n, g);
        if (grad_pred) {
            if (do_main) {
                loss_load4<VEC>(pred, at, n, x);
                const u32 win = WIN ? loss_in_window(w, at) : 0xFu;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float t = x[u] - g[u];
                    out[u] = (g[u] > gt_thr && (win >> u & 1u)) ? (2.0f * t) * k_main : 0.0f;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) out[u] = 0.0f;
            }
            loss_store4<VEC>(grad_pred, at, n, out);
        }
        if (grad_corr) {
            if (do_aux) {
                loss_load4<VEC>(corr, at, n, x);
                loss_load4<VEC>(lidar, at, n, l);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d = x[u] - g[u];
                    const float s = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                    out[u] = (g[u] > gt_thr && l[u] > in_thr) ? (2.0f * d + s) * k_aux : 0.0f;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) out[u] = 0.0f;
            }
            loss_store4<VEC>(grad_corr, at, n, out);
        }
    }
}

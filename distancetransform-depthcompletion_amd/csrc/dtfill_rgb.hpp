// dtfill_rgb.hpp -- rgb_read() of the reference's loader (data_read.py:66-73: Pillow's NEAREST resize of the decoded uint8
// image) and the drivers' next two lines (rgb = img_batch[:, 96:] / 255.0 as float32; train.py:213-214 and its kin) on decoded
// uint8 images of 1..4 interleaved channels (include/dtfill.h has the contract).
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit), after dtfill_read.hpp.
#pragma once

// ------------------------------------------------------------------------------------------------
// Two launches:
//   k_read_maps    dtfill_read.hpp's, as it is: Pillow's running double sum -> ry [B,H] / rx [B,W] in the workspace.
//   k_rgb_gather   frames along grid x, bands of output rows along y.  A block takes RG_ROWS output rows at a time:
//                    STAGE   it copies the source row of each (its w * C bytes) into LDS, 16-byte loads between the first and
//                            last 16-byte boundary inside the row and single bytes before and after, so that no byte outside
//                            the row is read; the LDS image keeps the row's address mod 16.  The byte picks then hit LDS.
//                    !STAGE  the picks read global memory (rows too long for the LDS image, and downscales by more than two,
//                            where staging would read bytes nobody samples).
//                  Then it writes each row of each output that was asked for: 16-byte stores between the first and last
//                  16-byte boundary inside the OUTPUT row (16 bytes of out_u8, 4 floats of the flat W * C row for NHWC, 4
//                  pixels of a plane's row for NCHW), single elements before and after.  Nothing is shared between blocks.
// ------------------------------------------------------------------------------------------------
constexpr int RG_THREADS = 256;
constexpr int RG_ROWS = 4;        // output rows per step (and per block, unless H - first_row > 65535 * 4: grid y is 16 bits)
constexpr int RG_SPAN = 8192;     // longest source row in bytes that is staged: 4 * (8192 + 16) B of LDS a block
constexpr int RG_LROW = RG_SPAN + 16;

// v / 255 correctly rounded, the reference's float32(float64(v) / 255.0), for v = 0 .. 255: one Newton step on the
// product with the rounded reciprocal.  (v * (1 / 255.0f) alone is wrong for 126 of the 256 values; tests/test_rgb_read.py
// checks this form in float32 arithmetic on the host, tests/test_gpu_rgb_read.py its bits on the device.)
__device__ __forceinline__ float rg_unit(float v) {
    const float r = 1.0f / 255.0f;
    const float q = v * r;
    return fmaf(fmaf(-q, 255.0f, v), r, q);
}

__device__ __forceinline__ float rg_value(u8 v, bool normalize) { return normalize ? rg_unit((float)v) : (float)v; }

__device__ __forceinline__ void rg_store16(u8 *o, const u8 (&v)[16]) {
    u32 d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = v[4 * k] | (u32)v[4 * k + 1] << 8 | (u32)v[4 * k + 2] << 16 | (u32)v[4 * k + 3] << 24;
    *reinterpret_cast<uint4 *>(o) = make_uint4(d[0], d[1], d[2], d[3]);
}
__device__ __forceinline__ void rg_store16(float *o, const float (&v)[4]) {
    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
}

// One output row: o[e] = get(e) for e in [0, n), o element-aligned.
template <typename T, typename F>
__device__ __forceinline__ void rg_store_row(T *__restrict__ o, int n, int tid, F get) {
    constexpr int V = 16 / (int)sizeof(T);
    const int head = min(n, (int)(((16u - (u32)((uintptr_t)o & 15)) & 15u) / sizeof(T)));
    const int nv = (n - head) / V, tail0 = head + nv * V;
    for (int q = tid; q < nv; q += RG_THREADS) {
        const int e = head + q * V;
        T v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = get(e + k);
        rg_store16(o + e, v);
    }
    if (tid < head) o[tid] = get(tid);                       // head < V
    if (tid < n - tail0) o[tail0 + tid] = get(tail0 + tid);  // < V elements
}

// Row `io` of frame b's outputs from the source row at `row` (LDS or global): element (j, c) is row[rx[j] * C + c].
template <int C>
__device__ __forceinline__ void rg_write_row(const u8 *row, const int *__restrict__ rxb, int b, int io, int OH, int W,
                                             bool normalize, int layout, u8 *__restrict__ out_u8, float *__restrict__ out_f32,
                                             int tid) {
    const size_t flat = ((size_t)b * OH + io) * W * C;
    auto pick = [&](int e) {
        const int j = e / C;
        return row[rxb[j] * C + (e - j * C)];
    };
    if (out_u8) rg_store_row(out_u8 + flat, W * C, tid, pick);
    if (!out_f32) return;
    if (layout == DTFILL_RGB_NHWC) {
        rg_store_row(out_f32 + flat, W * C, tid, [&](int e) { return rg_value(pick(e), normalize); });
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c)
            rg_store_row(out_f32 + (((size_t)b * C + c) * OH + io) * W, W, tid,
                         [&](int j) { return rg_value(row[rxb[j] * C + c], normalize); });
    }
}

struct RgArgs {
    const u8 *raw;
    const int32_t *dims;  // nullable
    int hmax, wmax, H, W, first_row, rpb, normalize, layout;
    const int *ry, *rx;
    u8 *out_u8;      // nullable
    float *out_f32;  // nullable
    int32_t *frame_status;  // nullable
};

template <int C, bool STAGE>
__global__ __launch_bounds__(RG_THREADS) void k_rgb_gather(const RgArgs a) {
    const int hmax = a.hmax, wmax = a.wmax, H = a.H, W = a.W, first_row = a.first_row, rpb = a.rpb, layout = a.layout;
    const bool normalize = a.normalize != 0;
    const int32_t *__restrict__ dims = a.dims;
    u8 *__restrict__ out_u8 = a.out_u8;
    float *__restrict__ out_f32 = a.out_f32;
    int32_t *__restrict__ frame_status = a.frame_status;
    __shared__ __attribute__((aligned(16))) u8 stage[STAGE ? RG_ROWS : 1][STAGE ? RG_LROW : 16];
    const int b = blockIdx.x, tid = threadIdx.x, OH = H - first_row;
    const int i0 = blockIdx.y * rpb, i1 = min(OH, i0 + rpb);  // rows of the cropped output
    int h, w;
    const bool ok = dr_dims(dims, b, hmax, wmax, h, w);  // block-uniform
    if (frame_status && blockIdx.y == 0 && tid == 0) frame_status[b] = ok ? 0 : DTFILL_READ_BAD_DIMS;
    if (!ok) {  // k_read_maps wrote no map: zeros, element by element
        const int n = W * C;
        for (int io = i0; io < i1; ++io) {
            const size_t flat = ((size_t)b * OH + io) * n;
            for (int e = tid; e < n; e += RG_THREADS) {
                if (out_u8) out_u8[flat + e] = 0;
                // every element of the frame's [OH, W, C] or [C, OH, W] block once, whichever layout it has
                if (out_f32) out_f32[(size_t)b * OH * n + (size_t)(e / W) * OH * W + (size_t)io * W + e % W] = 0.0f;
            }
        }
        return;
    }
    const int *ryb = a.ry + (size_t)b * H + first_row;
    const int *rxb = a.rx + (size_t)b * W;
    const size_t pitch = (size_t)wmax * C;
    const u8 *src = a.raw + (size_t)b * hmax * pitch;
    const int nb = w * C;  // bytes of a source row; STAGE: <= RG_SPAN
    for (int ib = i0; ib < i1; ib += RG_ROWS) {
        const u8 *row[RG_ROWS];
#pragma unroll
        for (int u = 0; u < RG_ROWS; ++u) row[u] = src + (size_t)ryb[min(ib + u, i1 - 1)] * pitch;  // (the last row again)
        if (STAGE) {
            if (ib != i0) __syncthreads();  // the step before has read its rows
#pragma unroll
            for (int u = 0; u < RG_ROWS; ++u) {
                const u8 *p = row[u];
                const int al = (int)((uintptr_t)p & 15);
                u8 *d = &stage[u][al];  // d + head is 16-byte aligned wherever p + head is
                const int head = min(nb, (16 - al) & 15), nv = (nb - head) >> 4, tail0 = head + nv * 16;
                for (int k = tid; k < nv; k += RG_THREADS)
                    reinterpret_cast<uint4 *>(d + head)[k] = reinterpret_cast<const uint4 *>(p + head)[k];
                if (tid < head) d[tid] = p[tid];                        // < 16 bytes
                if (tid < nb - tail0) d[tail0 + tid] = p[tail0 + tid];  // < 16 bytes
                row[u] = d;
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < RG_ROWS; ++u)
            if (ib + u < i1) rg_write_row<C>(row[u], rxb, b, ib + u, OH, W, normalize, layout, out_u8, out_f32, tid);
    }
}

template <int C>
void rgb_launch(dim3 grid, hipStream_t st, bool stage, const RgArgs &a) {
    if (stage)
        k_rgb_gather<C, true><<<grid, RG_THREADS, 0, st>>>(a);
    else
        k_rgb_gather<C, false><<<grid, RG_THREADS, 0, st>>>(a);
}

// dtfill_adam.hpp -- the optimizer step of the reference's training loop, train.py:169 and :253-254: Keras' Adam for every
// variable of a network in one fused pass (include/dtfill.h, dtfill_adam_step, states the contract; tests/adam_ref.py is its
// numpy form).  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace.
//
// Memory-bound streaming: 28 bytes an element (p, g, m, v read; p, m, v written) and a dozen float32 operations.  What is
// particular is the shape of the work: some 80 tensors a step, most of them biases of 16 to 512 floats, a few of millions.
// One launch takes up to ADAM_GROUP of them.  Their pointers, counts, segment offsets and chunk prefix counts travel BY VALUE
// in the kernel's arguments: the gradients are new tensors every step, so a device table would want a copy per call and a
// buffer that outlives it; the argument block wants neither and keeps the entry point re-entrant.
//
// A block owns one chunk of ADAM_CHUNK consecutive elements of one tensor.  It finds the tensor by a binary search of the
// prefix counts (uniform across the block: scalar loads from the argument block, seven steps at most) and then runs one of
// two bodies, chosen per TENSOR: 16-byte accesses where p, g, m and v are all 16-byte aligned (the segment offsets are
// multiples of 4 floats, so m and v decide for every tensor alike), dword accesses of the same elements otherwise.  Either
// way a lane's four accesses to each of the four arrays are independent of one another and stated ahead of the arithmetic,
// so the compiler keeps several of them in flight before the first use (it issues 7 or 8 of the 16 up front in the 16-byte
// body and the rest between the elements' arithmetic; 78 VGPRs, 6 waves a SIMD).  A full chunk runs a branch-free form of
// that body.  A short chunk loads the clamped index instead of branching round the load -- a branch per load would make the
// compiler wait for each in turn -- and only its stores are predicated, so no padding float is read or written.
//
// The step record is read-only here: every block forms alpha from it (two float64 products, a square root, a divide), and
// k_adam_advance, one wave launched behind the last update launch on the same stream, writes t', b1p', b2p'.  Stream order is
// the only synchronisation; no block can see a half-advanced record.
#pragma once

constexpr int ADAM_GROUP = DTFILL_ADAM_GROUP;
constexpr int ADAM_CHUNK = DTFILL_ADAM_CHUNK;
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_U = 4;  // accesses per array a lane has in flight
static_assert(ADAM_CHUNK == ADAM_THREADS * ADAM_U * 4, "a chunk is one pass of the 16-byte body, four of the dword body");

struct AdamRecord {
    long long t;
    double b1p, b2p;  // beta1^t, beta2^t as running float64 products
};

// 28 bytes a tensor and 48 of scalars: 128 * 28 + 48 = 3632 bytes, under the 4096 a HIP launch carries.
struct AdamArgs {
    float *p[ADAM_GROUP];
    const float *g[ADAM_GROUP];
    u32 seg4[ADAM_GROUP];  // the tensor's offset in m and in v, in units of 4 floats
    u32 count[ADAM_GROUP];
    u32 end[ADAM_GROUP];  // chunks of the tensors 0 .. i of this launch
    float *m, *v;
    const AdamRecord *rec;
    float lr, b1, b2, eps;
    int n;
    int pad_;
};
static_assert(sizeof(AdamArgs) == 3632 && sizeof(AdamArgs) < 4096, "the argument block of k_adam");

struct AdamScalars {
    float alpha, c1, c2, eps;
};

__device__ __forceinline__ AdamScalars adam_scalars(const AdamArgs &a) {
#pragma clang fp contract(off)
    const double b1p = a.rec->b1p * (double)a.b1, b2p = a.rec->b2p * (double)a.b2;
    const double alpha = ((double)a.lr * sqrt(1.0 - b2p)) / (1.0 - b1p);
    return AdamScalars{(float)alpha, 1.0f - a.b1, 1.0f - a.b2, a.eps};
}

// the contract's three lines; one rounding each (hipcc contracts a * b + c by default)
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars s) {
#pragma clang fp contract(off)
    const float dm = g - m;
    const float sm = s.c1 * dm;
    m = m + sm;
    const float gg = g * g;
    const float dv = gg - v;
    const float sv = s.c2 * dv;
    v = v + sv;
    const float num = s.alpha * m;
    const float den = sqrtf(v) + s.eps;
    p = p - num / den;
}

// len elements from p, g, m, v (the chunk's first) in 16-byte accesses: len / 4 quads, then the 1 to 3 elements behind them.
// FULL: len == ADAM_CHUNK, nothing to clamp or predicate (nearly every block of a large tensor).
template <bool FULL>
__device__ __forceinline__ void adam_chunk_vec(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                               float *__restrict__ v, u32 len, const AdamScalars s) {
    const u32 nq = len >> 2, tid = threadIdx.x;
    if (nq) {
        float4 P[ADAM_U], G[ADAM_U], M[ADAM_U], V[ADAM_U];
#pragma unroll
        for (int k = 0; k < ADAM_U; ++k) {
            const u32 q = FULL ? tid + k * ADAM_THREADS : min(tid + k * ADAM_THREADS, nq - 1);
            P[k] = reinterpret_cast<const float4 *>(p)[q];
            G[k] = reinterpret_cast<const float4 *>(g)[q];
            M[k] = reinterpret_cast<const float4 *>(m)[q];
            V[k] = reinterpret_cast<const float4 *>(v)[q];
        }
#pragma unroll
        for (int k = 0; k < ADAM_U; ++k) {
            const u32 q = tid + k * ADAM_THREADS;
            adam_element(P[k].x, G[k].x, M[k].x, V[k].x, s);
            adam_element(P[k].y, G[k].y, M[k].y, V[k].y, s);
            adam_element(P[k].z, G[k].z, M[k].z, V[k].z, s);
            adam_element(P[k].w, G[k].w, M[k].w, V[k].w, s);
            if (FULL || q < nq) {
                reinterpret_cast<float4 *>(p)[q] = P[k];
                reinterpret_cast<float4 *>(m)[q] = M[k];
                reinterpret_cast<float4 *>(v)[q] = V[k];
            }
        }
    }
    const u32 e = 4 * nq + tid;
    if (!FULL && e < len) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_element(pe, g[e], me, ve, s);
        p[e] = pe, m[e] = me, v[e] = ve;
    }
}

// the same elements in dword accesses: passes of ADAM_THREADS * ADAM_U elements, lane t owning t, t + 256, ..
__device__ __forceinline__ void adam_chunk_dword(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                 float *__restrict__ v, u32 len, const AdamScalars s) {
    for (u32 base = 0; base < len; base += ADAM_THREADS * ADAM_U) {
        float P[ADAM_U], G[ADAM_U], M[ADAM_U], V[ADAM_U];
#pragma unroll
        for (int k = 0; k < ADAM_U; ++k) {
            const u32 e = min(base + threadIdx.x + k * ADAM_THREADS, len - 1);
            P[k] = p[e], G[k] = g[e], M[k] = m[e], V[k] = v[e];
        }
#pragma unroll
        for (int k = 0; k < ADAM_U; ++k) {
            const u32 e = base + threadIdx.x + k * ADAM_THREADS;
            adam_element(P[k], G[k], M[k], V[k], s);
            if (e < len) p[e] = P[k], m[e] = M[k], v[e] = V[k];
        }
    }
}

// The three kernels are templates for one reason: hipcc emits a translation unit's plain kernels first and its template
// instantiations behind them in the order they are asked for, and these are asked for last (dtfill.hip's last entry points).
// So they lie behind every older kernel in the code object and none of those moved when this file was added (a kernel's time
// shifts by up to a percent with its placement).
template <int = 0>
__global__ __launch_bounds__(ADAM_THREADS) void k_adam(const AdamArgs a) {
    // the first tensor whose chunks end behind this block's
    const u32 b = blockIdx.x;
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.end[mid] > b) hi = mid;
        else lo = mid + 1;
    }
    const u32 chunk = b - (lo ? a.end[lo - 1] : 0u);
    const u32 count = a.count[lo], start = chunk * (u32)ADAM_CHUNK;  // count < 2^31: start fits
    if (start >= count) return;                                       // (never: the grid is the chunks)
    const u32 len = min((u32)ADAM_CHUNK, count - start);
    float *p = a.p[lo];
    const float *g = a.g[lo];
    const size_t at = (size_t)a.seg4[lo] * 4 + start;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)a.m | (uintptr_t)a.v) & 15) == 0;
    const AdamScalars s = adam_scalars(a);
    if (vec && len == (u32)ADAM_CHUNK) adam_chunk_vec<true>(p + start, g + start, a.m + at, a.v + at, len, s);
    else if (vec) adam_chunk_vec<false>(p + start, g + start, a.m + at, a.v + at, len, s);
    else adam_chunk_dword(p + start, g + start, a.m + at, a.v + at, len, s);
}

// one wave behind the last k_adam of a step: the record of the next step
template <int = 0>
__global__ __launch_bounds__(64) void k_adam_advance(AdamRecord *rec, float b1, float b2) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0) {
        const AdamRecord r = *rec;
        rec->t = r.t + 1;
        rec->b1p = r.b1p * (double)b1;
        rec->b2p = r.b2p * (double)b2;
    }
}

template <int = 0>
__global__ __launch_bounds__(64) void k_adam_init(AdamRecord *rec) {
    if (threadIdx.x == 0) rec->t = 0, rec->b1p = 1.0, rec->b2p = 1.0;
}

// Fused cross-entropy for gfx950 (CDNA4): loss from raw logits [R, C] (fp32 or
// bf16) and integer class targets [R], and the gradient at the logits in
// their dtype.  No log-probability tensor is made: forward keeps, per row,
// the maximum m and log(sum exp(x - m)), and backward recomputes the softmax
// from those two floats.  Targets, ignore_index and the upstream gradient are
// read on the device; nothing goes through the host.
//
// Row mapping, one body (ROWS):
//   ROWS = 1  a 256-thread block owns one row (C > 1024)
//   ROWS = 4  each of the block's four waves owns a row; no LDS, no barrier
//             (C <= 1024)
//
// ce_fwd_kernel   the label is read first.  A row whose label is ignore_index
//                 writes loss +0.0 and reads no logits; a label outside
//                 [0, C) writes NaN and is never used as an index.  Otherwise
//                 every lane keeps an online pair (m, s): s = sum exp(x - m)
//                 over what it has seen.  Scalar loads peel up to the first
//                 16-byte boundary of THIS row (a bf16 row of C = 30522 starts
//                 4-byte aligned, an odd C 2-byte aligned), 16-byte loads
//                 (8 bf16 / 4 fp32) follow, CE_UNROLL of them in flight, and a
//                 scalar tail finishes the row.  A vector's own maximum is
//                 taken first, so s is rescaled at most once per load.  Pairs
//                 merge by __shfl_down over the wave; with ROWS = 1 the four
//                 wave pairs go through LDS and one thread combines them in
//                 ascending wave order.
//                   loss = log(s) - (x[label] - m)
//                 which is torch's (x - max) - log(sum) order: the term of
//                 the row maximum is exact.  (m, log s) are kept apart in
//                 stats [2, R]: their sum would round at |m|, and backward
//                 subtracts them one after the other, as forward does.
// ce_finalize_kernel  one block: fixed-order tree over the row losses in fp64
//                 and an integer count of the rows that are not ignored;
//                 writes the fp32 loss and the fp32 factor 1 / n (mean) or 1
//                 (sum).  mean over zero rows is 0 / 0 = NaN.
// ce_bwd_kernel   per row g = gout * factor, both read from the device (gout:
//                 the scalar, or the row's element without a reduction).  An
//                 ignored or out-of-range row writes zeros with 16-byte
//                 stores and reads nothing.  Any other row writes
//                 T(expf((x - m) - log s) * g); the thread that owns the
//                 label's element subtracts g before the one rounding (bf16:
//                 round to nearest even).  Head and tail peel as in forward,
//                 so every store stays inside the row.
//
// No float atomics, every sum in a fixed order: the same bits on every run and
// on every graph replay.  expf / logf, no fast-math.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cross_entropy.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int CE_UNROLL = 4;  // 16-byte loads in flight per lane
constexpr float NEG = -INFINITY;

__device__ __forceinline__ long long load_label(const void* p, long long i,
                                                int is64) {
    return is64 ? static_cast<const long long*>(p)[i]
                : static_cast<long long>(static_cast<const int*>(p)[i]);
}

// bf16 travels as its 16 bits
using bf16_t = uint16_t;

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t h) {
    return __uint_as_float(((uint32_t)h) << 16);
}

__device__ __forceinline__ void from_f32(float f, float& out) { out = f; }
// round to nearest even; a NaN stays a NaN (quiet bit set), as wire_f2bf
__device__ __forceinline__ void from_f32(float f, bf16_t& out) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        out = (bf16_t)((u >> 16) | 0x0040u);
        return;
    }
    u += 0x7fffu + ((u >> 16) & 1u);
    out = (bf16_t)(u >> 16);
}

template <typename T>
struct Vec {
    static constexpr int N = 16 / sizeof(T);
};

__device__ __forceinline__ void unpack(const uint4& q, float (&f)[4], float) {
    f[0] = __uint_as_float(q.x);
    f[1] = __uint_as_float(q.y);
    f[2] = __uint_as_float(q.z);
    f[3] = __uint_as_float(q.w);
}

__device__ __forceinline__ void unpack(const uint4& q, float (&f)[8], bf16_t) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

__device__ __forceinline__ uint4 pack(const float (&f)[4], float) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                      __float_as_uint(f[2]), __float_as_uint(f[3]));
}

__device__ __forceinline__ uint4 pack(const float (&f)[8], bf16_t) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bf16_t lo, hi;
        from_f32(f[2 * i], lo);
        from_f32(f[2 * i + 1], hi);
        w[i] = (uint32_t)lo | ((uint32_t)hi << 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// How a row [C] that starts at `row` splits into scalar head, 16-byte
// vectors and scalar tail.
template <typename T>
struct RowSplit {
    int head, nvec, tail0;
    __device__ __forceinline__ RowSplit(const T* row, int C) {
        constexpr int V = Vec<T>::N;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15u);
        int h = mis ? (16 - mis) / (int)sizeof(T) : 0;
        head = h < C ? h : C;
        nvec = (C - head) / V;
        tail0 = head + nvec * V;
    }
};

// one element into the online pair; -inf adds nothing
__device__ __forceinline__ void online_add(float& m, float& s, float x) {
    if (x > m) {
        s = s * expf(m - x) + 1.0f;  // m = -inf: s = 0 * 0 + 1
        m = x;
    } else if (x != NEG) {
        s += expf(x - m);
    }
}

// (m, s) <- (m, s) merged with (m2, s2), this pair's terms first
__device__ __forceinline__ void online_merge(float& m, float& s, float m2,
                                             float s2) {
    const float M = fmaxf(m, m2);
    if (M == NEG) return;  // both empty or all -inf: s stays 0
    s = s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
}

template <typename T, int ROWS>
__global__ void __launch_bounds__(THREADS) ce_fwd_kernel(CeArgs a) {
    constexpr int V = Vec<T>::N;
    constexpr int NTHR = ROWS == 1 ? THREADS : WAVE;  // threads on one row
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int t = ROWS == 1 ? tid : lane;
    const long long r = ROWS == 1 ? (long long)blockIdx.x
                                  : (long long)blockIdx.x * ROWS + wave;
    if (r >= a.R) return;  // ROWS = 4 only: wave-uniform, no barrier follows
    const int C = a.C;

    // block-uniform (ROWS = 1) or wave-uniform (ROWS = 4)
    const long long label = load_label(a.target, r, a.target_i64);
    if (label == a.ignore_index || label < 0 || label >= C) {
        if (t == 0) {
            a.row_loss[r] = label == a.ignore_index ? 0.0f : NAN;
            a.stats[r] = 0.0f;
            a.stats[a.R + r] = 0.0f;
        }
        return;
    }

    const T* row = static_cast<const T*>(a.logits) + (size_t)r * C;
    const RowSplit<T> sp(row, C);
    float m = NEG, s = 0.0f;
    for (int i = t; i < sp.head; i += NTHR) online_add(m, s, to_f32(row[i]));
    const uint4* vrow = reinterpret_cast<const uint4*>(row + sp.head);
    for (int v0 = t; v0 < sp.nvec; v0 += NTHR * CE_UNROLL) {
        uint4 q[CE_UNROLL];
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u)
            if (v0 + u * NTHR < sp.nvec) q[u] = vrow[v0 + u * NTHR];
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            if (v0 + u * NTHR < sp.nvec) {
                float f[V];
                unpack(q[u], f, T());
                float vm = f[0];
#pragma unroll
                for (int i = 1; i < V; ++i) vm = fmaxf(vm, f[i]);
                if (vm > m) {
                    s *= expf(m - vm);
                    m = vm;
                }
                if (m > NEG) {
                    float part = 0.0f;
#pragma unroll
                    for (int i = 0; i < V; ++i) part += expf(f[i] - m);
                    s += part;
                }
            }
        }
    }
    for (int i = sp.tail0 + t; i < C; i += NTHR) online_add(m, s, to_f32(row[i]));

#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const float m2 = __shfl_down(m, off), s2 = __shfl_down(s, off);
        online_merge(m, s, m2, s2);  // lanes past the wave's end merge junk
    }                                // that lane 0 never takes in
    if constexpr (ROWS == 1) {
        __shared__ float pm[WAVES], ps[WAVES];
        if (lane == 0) {
            pm[wave] = m;
            ps[wave] = s;
        }
        __syncthreads();
        if (tid != 0) return;
        for (int w = 1; w < WAVES; ++w) online_merge(m, s, pm[w], ps[w]);
    } else {
        if (lane != 0) return;
    }
    const float ls = logf(s);
    a.row_loss[r] = ls - (to_f32(row[label]) - m);
    a.stats[r] = m;
    a.stats[a.R + r] = ls;
}

// reduction: 1 mean, 2 sum.  out[0] = loss, out[1] = factor.
__global__ void __launch_bounds__(THREADS)
ce_finalize_kernel(const float* __restrict__ row_loss, const void* target,
                   int target_i64, long long ignore_index, long long R,
                   int reduction, float* __restrict__ out) {
    __shared__ double sum[THREADS];
    __shared__ long long cnt[THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    long long n = 0;
    for (long long r = tid; r < R; r += THREADS) {
        acc += (double)row_loss[r];
        n += load_label(target, r, target_i64) != ignore_index;
    }
    sum[tid] = acc;
    cnt[tid] = n;
    __syncthreads();
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half) {
            sum[tid] += sum[tid + half];
            cnt[tid] += cnt[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (reduction == 1) {
            out[0] = (float)(sum[0] / (double)cnt[0]);
            out[1] = 1.0f / (float)cnt[0];
        } else {
            out[0] = (float)sum[0];
            out[1] = 1.0f;
        }
    }
}

template <typename T, int ROWS>
__global__ void __launch_bounds__(THREADS) ce_bwd_kernel(CeBwdArgs a) {
    constexpr int V = Vec<T>::N;
    constexpr int NTHR = ROWS == 1 ? THREADS : WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int t = ROWS == 1 ? tid : lane;
    const long long r = ROWS == 1 ? (long long)blockIdx.x
                                  : (long long)blockIdx.x * ROWS + wave;
    if (r >= a.R) return;
    const int C = a.C;
    T* out = static_cast<T*>(a.grad) + (size_t)r * C;
    // the binding places grad at the logits' offset from a 16-byte boundary,
    // so one split serves the loads and the stores
    const RowSplit<T> sp(out, C);
    uint4* vout = reinterpret_cast<uint4*>(out + sp.head);

    const long long label = load_label(a.target, r, a.target_i64);
    if (label == a.ignore_index || label < 0 || label >= C) {
        T zero;
        from_f32(0.0f, zero);
        for (int i = t; i < sp.head; i += NTHR) out[i] = zero;
        for (int v = t; v < sp.nvec; v += NTHR) vout[v] = make_uint4(0, 0, 0, 0);
        for (int i = sp.tail0 + t; i < C; i += NTHR) out[i] = zero;
        return;
    }

    const T* row = static_cast<const T*>(a.logits) + (size_t)r * C;
    const uint4* vrow = reinterpret_cast<const uint4*>(row + sp.head);
    float g = a.gout[a.gout_per_row ? r : 0];
    if (a.factor != nullptr) g *= a.factor[0];
    const float m = a.stats[r], ls = a.stats[a.R + r];
    const int lab = (int)label;

    for (int i = t; i < sp.head; i += NTHR) {
        float v = expf((to_f32(row[i]) - m) - ls) * g;
        if (i == lab) v -= g;
        from_f32(v, out[i]);
    }
    for (int v0 = t; v0 < sp.nvec; v0 += NTHR * CE_UNROLL) {
        uint4 q[CE_UNROLL];
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u)
            if (v0 + u * NTHR < sp.nvec) q[u] = vrow[v0 + u * NTHR];
#pragma unroll
        for (int u = 0; u < CE_UNROLL; ++u) {
            const int v = v0 + u * NTHR;
            if (v < sp.nvec) {
                float f[V];
                unpack(q[u], f, T());
                const int base = sp.head + v * V;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    f[i] = expf((f[i] - m) - ls) * g;
                    if (base + i == lab) f[i] -= g;
                }
                vout[v] = pack(f, T());
            }
        }
    }
    for (int i = sp.tail0 + t; i < C; i += NTHR) {
        float v = expf((to_f32(row[i]) - m) - ls) * g;
        if (i == lab) v -= g;
        from_f32(v, out[i]);
    }
}

template <int ROWS>
dim3 row_grid(long long R) {
    return dim3((unsigned)((R + ROWS - 1) / ROWS));
}

}  // namespace

extern "C" {

void launch_ce_fwd(const CeArgs* a, hipStream_t s) {
    const bool wide = a->C > CE_WAVE_ROW_MAX_C;
    if (a->is_bf16) {
        if (wide)
            hipLaunchKernelGGL((ce_fwd_kernel<bf16_t, 1>), row_grid<1>(a->R),
                               dim3(THREADS), 0, s, *a);
        else
            hipLaunchKernelGGL((ce_fwd_kernel<bf16_t, 4>), row_grid<4>(a->R),
                               dim3(THREADS), 0, s, *a);
    } else {
        if (wide)
            hipLaunchKernelGGL((ce_fwd_kernel<float, 1>), row_grid<1>(a->R),
                               dim3(THREADS), 0, s, *a);
        else
            hipLaunchKernelGGL((ce_fwd_kernel<float, 4>), row_grid<4>(a->R),
                               dim3(THREADS), 0, s, *a);
    }
}

void launch_ce_finalize(const CeArgs* a, int reduction, float* out,
                        hipStream_t s) {
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(THREADS), 0, s,
                       a->row_loss, a->target, a->target_i64, a->ignore_index,
                       a->R, reduction, out);
}

void launch_ce_bwd(const CeBwdArgs* a, hipStream_t s) {
    const bool wide = a->C > CE_WAVE_ROW_MAX_C;
    if (a->is_bf16) {
        if (wide)
            hipLaunchKernelGGL((ce_bwd_kernel<bf16_t, 1>), row_grid<1>(a->R),
                               dim3(THREADS), 0, s, *a);
        else
            hipLaunchKernelGGL((ce_bwd_kernel<bf16_t, 4>), row_grid<4>(a->R),
                               dim3(THREADS), 0, s, *a);
    } else {
        if (wide)
            hipLaunchKernelGGL((ce_bwd_kernel<float, 1>), row_grid<1>(a->R),
                               dim3(THREADS), 0, s, *a);
        else
            hipLaunchKernelGGL((ce_bwd_kernel<float, 4>), row_grid<4>(a->R),
                               dim3(THREADS), 0, s, *a);
    }
}

}  // extern "C"

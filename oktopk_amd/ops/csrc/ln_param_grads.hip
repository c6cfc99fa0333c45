// Batched LayerNorm gamma / beta gradients: one launch for a table of
//   (gy bf16 [M, N], x bf16 [M, N], mean fp32 [M], rstd fp32 [M],
//    dst_gamma bf16 [N], dst_beta bf16 [N])
// entries.  Per column c
//   gg = bf16(sum_r (gy[r, c] * (x[r, c] - mean[r])) * rstd[r])
//   gb = bf16(sum_r gy[r, c])
//   dst_gamma[c] = bf16(float(dst_gamma[c]) + float(gg)), dst_beta likewise
// which is torch's native_layer_norm_backward(..., [False, True, True])
// followed by autograd's bf16 `slot += g`, with every bit theirs.  A backward
// pass of BERT-base has 26 such sites; torch runs two kernels for each and
// hands an fp32 workspace from the first to the second
// (profiles/README.md r21).
//
// The sums follow the association tree of torch's ROCm pair
// cuComputePartGradGammaBeta (block 64 x 4, grid ceil(N/64) x 64) and
// cuComputeGradGammaBeta (block 64 x 8), ATen/native/cuda/layer_norm_kernel.cu,
// for 128 <= M <= 1024, where every grid row of the first kernel owns one
// chunk of 16 rows (torch runs another kernel below 128 rows, and above 1024
// a grid row walks several chunks with an accumulate whose contraction has
// not been read from the binary):
//   t[r]  = gy[r]                      for beta
//         = (gy[r] * (x[r] - mean[r])) * rstd[r]     for gamma, no fma
//   A(j)  = (((0 + t[j]) + t[j+4]) + t[j+8]) + t[j+12]     j = 0..3, rows of
//           chunk p = rows 16p .. 16p+15; a row at or past M adds +0
//   P(p)  = (A(0) + A(2)) + (A(1) + A(3))                  p = 0..63
//   S(j)  = (((0 + P(8j)) + P(8j+1)) + ...) + P(8j+7)      j = 0..7
//   S(j) += S(j+4), j < 4;  S(j) += S(j+2), j < 2;  S(0) += S(1)
//   g     = bf16(S(0))
// No accumulator ever holds -0 (each starts from +0), so a skipped +0 leaves
// the bits alone.  The tree of a column does not depend on how columns are
// dealt to threads: a block owns a strip of 32 columns of one entry and all
// its rows, with the 64 chunk partials of the strip in LDS.  One launch, no
// workspace, no atomics, 2-byte stores bounded by N.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ln_param_grads.h"

// Scalar fp32 operations only and no contraction, as in residual_ln.hip: the
// order above is the whole contract of this file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#pragma clang fp contract(off)

namespace {

constexpr int LPG_THREADS = 256;
constexpr int LPG_STRIP = 32;    // columns per block
constexpr int LPG_PARTS = 64;    // grid rows of torch's first kernel
constexpr int LPG_CHUNK = 16;    // rows per grid row while M <= 1024
constexpr int LPG_BURST = 8;    // rows loaded before they are added (a multiple of 4)
constexpr int LPG_WARPS = 8;     // blockDim.y of torch's second kernel
constexpr int64_t LPG_MIN_ROWS = 128;
constexpr int64_t LPG_MAX_ROWS = (int64_t)LPG_PARTS * LPG_CHUNK;

struct LpgEntry {
    const uint16_t* gy;
    const uint16_t* x;
    const float* mean;
    const float* rstd;
    uint16_t* dst_gamma;
    uint16_t* dst_beta;
    int32_t M;
    int32_t N;
    int32_t vec;     // columns per thread and load: 4, 2 or 1
    int32_t pad;
};

struct LpgTable {
    int32_t n;
    uint32_t block_end[LN_GRAD_BATCH_CAPACITY];   // running sum of block counts
    LpgEntry e[LN_GRAD_BATCH_CAPACITY];
};
static_assert(sizeof(LpgTable) + 256 <= 4096, "table + hidden arguments: 4 KB");

__device__ __forceinline__ float lpg_b2f(uint32_t bits16) {
    return __builtin_bit_cast(float, bits16 << 16);
}

// c10::detail::round_to_nearest_even: NaN becomes 0x7fc0
__device__ __forceinline__ uint16_t lpg_f2b(float f) {
    if (f != f) return (uint16_t)0x7fc0u;
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// __syncthreads() from builtins: a header function built with other target
// features does not inline into these kernels
__device__ __forceinline__ void lpg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int VEC>
__device__ __forceinline__ void lpg_load(const uint16_t* __restrict__ p,
                                         float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        v[0] = lpg_b2f(w.x & 0xffffu); v[1] = lpg_b2f(w.x >> 16);
        v[2] = lpg_b2f(w.y & 0xffffu); v[3] = lpg_b2f(w.y >> 16);
    } else if constexpr (VEC == 2) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        v[0] = lpg_b2f(w & 0xffffu); v[1] = lpg_b2f(w >> 16);
    } else {
        v[0] = lpg_b2f(*p);
    }
}

// Strip number `blk` of one entry.  lds: P for gamma [64][32], P for beta
// [64][32], then S for gamma [8][32] and S for beta [8][32].
template <int VEC>
__device__ __forceinline__ void lpg_strip(const LpgEntry& e, int64_t blk,
                                          float* __restrict__ lds) {
    constexpr int TX = LPG_STRIP / VEC;       // threads along the strip
    constexpr int NY = LPG_THREADS / TX;      // chunks walked side by side
    constexpr int PSIZE = LPG_PARTS * LPG_STRIP;
    const int tid = (int)__builtin_amdgcn_workitem_id_x();
    const int tx = tid % TX, y = tid / TX;
    const int64_t M = e.M, N = e.N;
    const int64_t col0 = blk * LPG_STRIP + (int64_t)tx * VEC;
    const bool active = col0 < N;             // N % VEC == 0: whole vector in range

    for (int part = y; part < LPG_PARTS; part += NY) {
        float ag[4][VEC], ab[4][VEC];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) ag[j][v] = ab[j][v] = 0.f;
        }
        const int64_t r0 = (int64_t)part * LPG_CHUNK;
        if (active && r0 < M) {
            const uint16_t* gyp = e.gy + r0 * N + col0;
            const uint16_t* xp = e.x + r0 * N + col0;
            if (r0 + LPG_CHUNK <= M) {
                // a whole chunk, LPG_BURST rows at a time: their loads are
                // all issued before the first add
#pragma unroll
                for (int h = 0; h < LPG_CHUNK; h += LPG_BURST) {
                    float dy[LPG_BURST][VEC], xs[LPG_BURST][VEC];
                    float mu[LPG_BURST], rs[LPG_BURST];
#pragma unroll
                    for (int i = 0; i < LPG_BURST; ++i) {
                        lpg_load<VEC>(gyp + (h + i) * N, dy[i]);
                        lpg_load<VEC>(xp + (h + i) * N, xs[i]);
                        mu[i] = e.mean[r0 + h + i];
                        rs[i] = e.rstd[r0 + h + i];
                    }
#pragma unroll
                    for (int i = 0; i < LPG_BURST; ++i) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            ab[i & 3][v] = ab[i & 3][v] + dy[i][v];
                            ag[i & 3][v] = ag[i & 3][v] + (dy[i][v] * (xs[i][v] - mu[i])) * rs[i];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < LPG_CHUNK; ++i) {
                    if (r0 + i < M) {
                        float dy[VEC], xs[VEC];
                        lpg_load<VEC>(gyp + i * N, dy);
                        lpg_load<VEC>(xp + i * N, xs);
                        const float mu = e.mean[r0 + i], rs = e.rstd[r0 + i];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            ab[i & 3][v] = ab[i & 3][v] + dy[v];
                            ag[i & 3][v] = ag[i & 3][v] + (dy[v] * (xs[v] - mu)) * rs;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int at = part * LPG_STRIP + tx * VEC + v;
            lds[at] = (ag[0][v] + ag[2][v]) + (ag[1][v] + ag[3][v]);
            lds[PSIZE + at] = (ab[0][v] + ab[2][v]) + (ab[1][v] + ab[3][v]);
        }
    }
    lpg_sync();

    // torch's second kernel: thread (j, c) carries both sums of its column
    static_assert(LPG_THREADS == LPG_WARPS * LPG_STRIP, "one thread per (j, column)");
    constexpr int SSIZE = LPG_WARPS * LPG_STRIP;
    const int c = tid % LPG_STRIP, j = tid / LPG_STRIP;
    float* s = lds + 2 * PSIZE;
    float sg = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < LPG_PARTS / LPG_WARPS; ++i) {
        const int at = (j * (LPG_PARTS / LPG_WARPS) + i) * LPG_STRIP + c;
        sg = sg + lds[at];
        sb = sb + lds[PSIZE + at];
    }
#pragma unroll
    for (int off = LPG_WARPS / 2; off >= 1; off >>= 1) {
        if (j >= off && j < 2 * off) {
            s[j * LPG_STRIP + c] = sg;
            s[SSIZE + j * LPG_STRIP + c] = sb;
        }
        lpg_sync();
        if (j < off) {
            sg = sg + s[(j + off) * LPG_STRIP + c];
            sb = sb + s[SSIZE + (j + off) * LPG_STRIP + c];
        }
        lpg_sync();
    }
    const int64_t col = blk * LPG_STRIP + c;
    if (j == 0 && col < N) {
        const uint16_t gg = lpg_f2b(sg), gb = lpg_f2b(sb);
        e.dst_gamma[col] = lpg_f2b(lpg_b2f(e.dst_gamma[col]) + lpg_b2f(gg));
        e.dst_beta[col] = lpg_f2b(lpg_b2f(e.dst_beta[col]) + lpg_b2f(gb));
    }
}

__global__ __launch_bounds__(LPG_THREADS)
void ln_param_grads_kernel(const LpgTable t) {
    __shared__ float lds[2 * LPG_PARTS * LPG_STRIP + 2 * LPG_WARPS * LPG_STRIP];
    // first entry whose block_end exceeds the block's number (block-uniform)
    const uint32_t bid = __builtin_amdgcn_workgroup_id_x();
    int lo = 0, hi = t.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bid < t.block_end[mid]) hi = mid;
        else lo = mid + 1;
    }
    const int64_t blk = bid - (lo > 0 ? t.block_end[lo - 1] : 0u);
    const LpgEntry& e = t.e[lo];
    switch (e.vec) {
        case 4: lpg_strip<4>(e, blk, lds); break;
        case 2: lpg_strip<2>(e, blk, lds); break;
        default: lpg_strip<1>(e, blk, lds); break;
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int ln_param_grads_shape_ok(int64_t M, int64_t N) {
    return M >= LPG_MIN_ROWS && M <= LPG_MAX_ROWS && N >= 1 && N <= INT32_MAX / 2;
}

extern "C" int launch_ln_param_grads_bf16(const LnGradItem* items, int n,
                                          hipStream_t stream) {
    // plan everything first: nothing is launched unless every entry fits
    std::vector<LpgEntry> entries;
    std::vector<unsigned> blocks;
    uint64_t all_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const LnGradItem& it = items[i];
        if (!ln_param_grads_shape_ok(it.M, it.N)) return -1;
        LpgEntry e{};
        e.gy = (const uint16_t*)it.gy;
        e.x = (const uint16_t*)it.x;
        e.mean = it.mean;
        e.rstd = it.rstd;
        e.dst_gamma = (uint16_t*)it.dst_gamma;
        e.dst_beta = (uint16_t*)it.dst_beta;
        e.M = (int32_t)it.M;
        e.N = (int32_t)it.N;
        const uintptr_t a = (uintptr_t)it.gy | (uintptr_t)it.x;
        e.vec = (it.N % 4 == 0 && (a & 7) == 0) ? 4
              : (it.N % 2 == 0 && (a & 3) == 0) ? 2 : 1;
        entries.push_back(e);
        blocks.push_back((unsigned)((it.N + LPG_STRIP - 1) / LPG_STRIP));
        all_blocks += blocks.back();
        if (all_blocks > (uint64_t)INT32_MAX) return -1;   // grid limit
    }
    int launches = 0;
    for (int first = 0; first < n; first += LN_GRAD_BATCH_CAPACITY) {
        LpgTable t{};
        t.n = std::min(n - first, LN_GRAD_BATCH_CAPACITY);
        unsigned total = 0;
        for (int j = 0; j < t.n; ++j) {
            total += blocks[first + j];
            t.block_end[j] = total;
            t.e[j] = entries[first + j];
        }
        hipLaunchKernelGGL(ln_param_grads_kernel, dim3(total), dim3(LPG_THREADS),
                           0, stream, t);
        ++launches;
    }
    return launches;
}

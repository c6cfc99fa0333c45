// Bias-gradient column sum written straight into its gradient slot.
//
//   dst[c] = (accumulate ? dst[c] : 0) + sum_r gy[r, c]      gy bf16 [R, C]
//
// One launch, fp32 accumulation, no atomics and no workspace: every column
// is reduced by exactly one block in a fixed order, so two runs give the
// same bits, and the caller neither zeroes nor casts anything.  dst is
// written with 2-byte stores, so it may sit at any element offset of the
// flat gradient buffer.
//
// Tiling.  A 512-thread block owns a strip of TX*VEC columns.  Inside a
// wave, TX lanes lie along the strip (VEC bf16 each, one vector load) and
// 64/TX lanes along rows; the 8 waves stack further row groups, so a block
// walks TY = 8*64/TX rows per step.  Row groups are folded with xor
// shuffles inside the wave, then across the 8 waves through LDS.
//   C % 8 == 0, 16-B aligned : VEC 8, TX 4  -> 64-B row segments, 32-col
//       strips (24 / 96 blocks at C = 768 / 3072; R = 1024 is 8 loads per
//       thread, all in flight at once)
//   C % 2 == 0, 4-B aligned  : VEC 2, TX 32 -> 128-B row segments, 64-col
//       strips (477 blocks at C = 30522, a 62 MB stream)
//   otherwise                : VEC 1, TX 64 -> 128-B row segments
// Narrow outputs (C < strip) shrink TX so the lanes go to rows instead.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace {

constexpr int DG_THREADS = 512;
constexpr int DG_WAVES = DG_THREADS / 64;

__device__ __forceinline__ float dg_b2f(uint32_t bits16) {
    return __uint_as_float(bits16 << 16);
}

__device__ __forceinline__ uint16_t dg_f2b(float f) {
    // round-to-nearest-even, NaN kept quiet
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

template <int VEC>
__device__ __forceinline__ void dg_load_add(const uint16_t* __restrict__ p,
                                            float (&acc)[VEC]) {
    if constexpr (VEC == 8) {
        uint4 v = *reinterpret_cast<const uint4*>(p);
        acc[0] += dg_b2f(v.x & 0xffffu); acc[1] += dg_b2f(v.x >> 16);
        acc[2] += dg_b2f(v.y & 0xffffu); acc[3] += dg_b2f(v.y >> 16);
        acc[4] += dg_b2f(v.z & 0xffffu); acc[5] += dg_b2f(v.z >> 16);
        acc[6] += dg_b2f(v.w & 0xffffu); acc[7] += dg_b2f(v.w >> 16);
    } else if constexpr (VEC == 2) {
        uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        acc[0] += dg_b2f(v & 0xffffu); acc[1] += dg_b2f(v >> 16);
    } else {
        acc[0] += dg_b2f(*p);
    }
}

template <int VEC, int TX, int UNROLL>
__global__ __launch_bounds__(DG_THREADS)
void colsum_into_kernel(const uint16_t* __restrict__ gy, int64_t R, int64_t C,
                        uint16_t* __restrict__ dst, int accumulate) {
    constexpr int RY = 64 / TX;            // row groups inside a wave
    constexpr int TY = DG_WAVES * RY;      // rows per block step
    constexpr int STRIP = TX * VEC;        // columns per block
    __shared__ float part[DG_WAVES][STRIP];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tx = lane % TX;
    const int64_t col0 = ((int64_t)blockIdx.x * TX + tx) * VEC;
    const bool active = col0 < C;          // C % VEC == 0: whole vector in range

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;

    if (active) {
        const uint16_t* base = gy + col0;
        int64_t r = wave * RY + lane / TX;
        for (; r + (int64_t)(UNROLL - 1) * TY < R; r += (int64_t)UNROLL * TY) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                dg_load_add<VEC>(base + (r + (int64_t)u * TY) * C, acc);
        }
        for (; r < R; r += TY) dg_load_add<VEC>(base + r * C, acc);
    }

    // fold the wave's row groups (every lane takes part; idle lanes hold 0)
#pragma unroll
    for (int off = TX; off < 64; off <<= 1) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], off, 64);
    }
    if (lane < TX) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) part[wave][tx * VEC + v] = acc[v];
    }
    __syncthreads();

    if (threadIdx.x < STRIP) {
        const int64_t col = (int64_t)blockIdx.x * STRIP + threadIdx.x;
        if (col < C) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < DG_WAVES; ++w) s += part[w][threadIdx.x];
            if (accumulate) s += dg_b2f(dst[col]);
            dst[col] = dg_f2b(s);
        }
    }
}

template <int VEC, int TX, int UNROLL>
void dg_launch(const void* gy, int64_t R, int64_t C, void* dst, int accumulate,
               hipStream_t stream) {
    const int64_t strip = (int64_t)TX * VEC;
    const unsigned blocks = (unsigned)((C + strip - 1) / strip);
    hipLaunchKernelGGL((colsum_into_kernel<VEC, TX, UNROLL>), dim3(blocks),
                       dim3(DG_THREADS), 0, stream, (const uint16_t*)gy, R, C,
                       (uint16_t*)dst, accumulate);
}

}  // namespace

extern "C" void launch_colsum_into_bf16(const void* gy, int64_t R, int64_t C,
                                        void* dst, int accumulate,
                                        hipStream_t stream) {
    if (C <= 0) return;
    const uintptr_t a = (uintptr_t)gy;
    if (C % 8 == 0 && (a & 15) == 0) {
        if (C >= 32) dg_launch<8, 4, 4>(gy, R, C, dst, accumulate, stream);
        else         dg_launch<8, 1, 4>(gy, R, C, dst, accumulate, stream);
    } else if (C % 2 == 0 && (a & 3) == 0) {
        if (C >= 64) dg_launch<2, 32, 8>(gy, R, C, dst, accumulate, stream);
        else if (C >= 8) dg_launch<2, 4, 8>(gy, R, C, dst, accumulate, stream);
        else         dg_launch<2, 1, 8>(gy, R, C, dst, accumulate, stream);
    } else {
        if (C >= 64) dg_launch<1, 64, 8>(gy, R, C, dst, accumulate, stream);
        else         dg_launch<1, 8, 8>(gy, R, C, dst, accumulate, stream);
    }
}

// ---------------------------------------------------------------------------
// The same column sum with torch's association tree, so that it leaves the
// bits at::sum_out leaves (order: README.md here, "Bias-gradient column sum
// in torch's order"; configuration: colsum_exact_config.h).
//
// torch deals the rows of one column over L = bh * ctas logical lanes
// (threadIdx.y, blockIdx.y); lane l takes rows l, l + L, l + 2L, ... and
// adds row number k of its own into accumulator k mod 4.  So a column is
// 4L independent sequential chains: chain q (0 <= q < 4L) sums rows
// q, q + 4L, q + 8L, ... from +0.0f, and lane l owns chains l, l + L,
// l + 2L, l + 3L.  Here one block owns a strip of S = TX * VEC columns and
// all 4L chains of it: threads are (tx, y), y walks the chains, the chain
// sums go to LDS and are then combined in torch's order:
//   T(l)  = ((c[l] + c[l+L]) + c[l+2L]) + c[l+3L]
//   P(by) = tree over ty of T(ty + by*bh): T[ty] += T[ty+off], off = bh/2..1
//   G(ty) = ((0 + P(ty)) + P(ty+bh)) + ...         (only when ctas > 1)
//   out   = the same tree over G(ty); P(0) when ctas == 1
// One launch, no workspace, no atomics, 2-byte stores into dst.  Overwrite
// only: accumulating callers keep torch's sum + add_ (bindings.cpp says why).
// VEC is the load width only; torch's own vector size enters through bh.
// ---------------------------------------------------------------------------
namespace {

constexpr int DGX_MAX_THREADS = 512;
constexpr int DGX_MAX_LDS = 64 * 1024;

template <int VEC>
__device__ __forceinline__ void dgx_load(const uint16_t* __restrict__ p,
                                         float (&x)[VEC]) {
    if constexpr (VEC == 8) {
        uint4 v = *reinterpret_cast<const uint4*>(p);
        x[0] = dg_b2f(v.x & 0xffffu); x[1] = dg_b2f(v.x >> 16);
        x[2] = dg_b2f(v.y & 0xffffu); x[3] = dg_b2f(v.y >> 16);
        x[4] = dg_b2f(v.z & 0xffffu); x[5] = dg_b2f(v.z >> 16);
        x[6] = dg_b2f(v.w & 0xffffu); x[7] = dg_b2f(v.w >> 16);
    } else if constexpr (VEC == 4) {
        uint2 v = *reinterpret_cast<const uint2*>(p);
        x[0] = dg_b2f(v.x & 0xffffu); x[1] = dg_b2f(v.x >> 16);
        x[2] = dg_b2f(v.y & 0xffffu); x[3] = dg_b2f(v.y >> 16);
    } else if constexpr (VEC == 2) {
        uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        x[0] = dg_b2f(v & 0xffffu); x[1] = dg_b2f(v >> 16);
    } else {
        x[0] = dg_b2f(*p);
    }
}

__device__ __forceinline__ uint16_t dgx_f2b(float f) {
    // round-to-nearest-even; NaN becomes the canonical quiet NaN, as in
    // c10::BFloat16
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

template <int VEC>
__global__ __launch_bounds__(DGX_MAX_THREADS)
void colsum_exact_kernel(const uint16_t* __restrict__ gy, int64_t R, int64_t C,
                         uint16_t* __restrict__ dst, int tx_shift, int bh,
                         int ctas) {
    extern __shared__ float dgx_lds[];     // [4L][S]
    const int TX = 1 << tx_shift;
    const int s_shift = tx_shift + (VEC == 8 ? 3 : VEC == 4 ? 2 : VEC == 2 ? 1 : 0);
    const int S = 1 << s_shift;            // columns per block
    const int nthreads = blockDim.x;
    const int NY = nthreads >> tx_shift;
    const int tid = threadIdx.x;
    const int tx = tid & (TX - 1);
    const int y = tid >> tx_shift;
    const int L = bh * ctas;
    const int nchain = 4 * L;
    const int64_t col0 = ((int64_t)blockIdx.x * TX + tx) * VEC;
    const bool active = col0 < C;          // C % VEC == 0: whole vector in range
    const int64_t cstep = nchain;          // row stride inside a chain

    // chain sums
    for (int q = y; q < nchain; q += NY) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        if (active) {
            const uint16_t* base = gy + col0;
            int64_t r = q;
            for (; r + 3 * cstep < R; r += 4 * cstep) {
                float x[4][VEC];
#pragma unroll
                for (int u = 0; u < 4; ++u) dgx_load<VEC>(base + (r + u * cstep) * C, x[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + x[u][v];
                }
            }
            for (; r < R; r += cstep) {
                float x[VEC];
                dgx_load<VEC>(base + r * C, x);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + x[v];
            }
        }
        float* out = dgx_lds + ((size_t)q << s_shift) + tx * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) out[v] = acc[v];
    }
    __syncthreads();

    // T(l): the lane's four accumulators, left to right; stays in row l
    for (int i = tid; i < (L << s_shift); i += nthreads) {
        const int c = i & (S - 1);
        const int l = i >> s_shift;
        const float a0 = dgx_lds[((size_t)l << s_shift) + c];
        const float a1 = dgx_lds[((size_t)(l + L) << s_shift) + c];
        const float a2 = dgx_lds[((size_t)(l + 2 * L) << s_shift) + c];
        const float a3 = dgx_lds[((size_t)(l + 3 * L) << s_shift) + c];
        dgx_lds[((size_t)l << s_shift) + c] = ((a0 + a1) + a2) + a3;
    }
    __syncthreads();

    // P(by): block_y_reduce over the bh lanes of each logical block
    for (int off = bh >> 1; off > 0; off >>= 1) {
        const int items = (ctas * off) << s_shift;
        for (int i = tid; i < items; i += nthreads) {
            const int c = i & (S - 1);
            const int t = i >> s_shift;
            const int ty = t % off;
            const int by = t / off;
            const size_t row = (size_t)(by * bh + ty);
            dgx_lds[(row << s_shift) + c] =
                dgx_lds[(row << s_shift) + c] + dgx_lds[((row + off) << s_shift) + c];
        }
        __syncthreads();
    }

    int res_row = 0;
    if (ctas > 1) {
        // global_reduce: lane ty of the last block folds P(ty), P(ty+bh), ...
        // onto the identity, then block_y_reduce again.  Rows L .. L+bh-1
        // (dead chain sums) hold G.
        for (int i = tid; i < (bh << s_shift); i += nthreads) {
            const int c = i & (S - 1);
            const int ty = i >> s_shift;
            float g = 0.f;
            for (int j = ty; j < ctas; j += bh)
                g = g + dgx_lds[((size_t)(j * bh) << s_shift) + c];
            dgx_lds[((size_t)(L + ty) << s_shift) + c] = g;
        }
        __syncthreads();
        for (int off = bh >> 1; off > 0; off >>= 1) {
            for (int i = tid; i < (off << s_shift); i += nthreads) {
                const int c = i & (S - 1);
                const size_t row = (size_t)(L + (i >> s_shift));
                dgx_lds[(row << s_shift) + c] =
                    dgx_lds[(row << s_shift) + c] + dgx_lds[((row + off) << s_shift) + c];
            }
            __syncthreads();
        }
        res_row = L;
    }

    for (int c = tid; c < S; c += nthreads) {
        const int64_t col = ((int64_t)blockIdx.x << s_shift) + c;
        if (col < C) {
            dst[col] = dgx_f2b(dgx_lds[((size_t)res_row << s_shift) + c]);
        }
    }
}

inline int dgx_pow2_floor(int64_t n) {
    int p = 1;
    while ((int64_t)p * 2 <= n) p *= 2;
    return p;
}

template <int VEC>
bool dgx_launch(const void* gy, int64_t R, int64_t C, void* dst, int bh,
                int ctas, hipStream_t stream) {
    const int64_t nchain = 4 * (int64_t)bh * ctas;
    // 64-byte row segments; narrower when the output is
    int tx = 32 / VEC;
    while (tx > 1 && (int64_t)(tx / 2) * VEC >= C) tx /= 2;
    // a wide output has blocks to spare: 128-byte segments
    while (tx * VEC < 64 && C / (tx * VEC) > 512) tx *= 2;
    int ny = dgx_pow2_floor(std::min<int64_t>(nchain, DGX_MAX_THREADS / tx));
    // few chains (a long R per lane, ctas == 1): widen the strip instead
    while (tx * ny < 256 && (int64_t)tx * VEC < C) tx *= 2;
    // the chain sums of a strip must fit into LDS
    while (tx > 1 && nchain * tx * VEC * 4 > DGX_MAX_LDS) {
        tx /= 2;
        ny = dgx_pow2_floor(std::min<int64_t>(nchain, DGX_MAX_THREADS / tx));
    }
    const int64_t lds = nchain * tx * VEC * 4;
    if (lds > DGX_MAX_LDS) return false;
    int tx_shift = 0;
    while ((1 << tx_shift) < tx) ++tx_shift;
    const int64_t strip = (int64_t)tx * VEC;
    const unsigned blocks = (unsigned)((C + strip - 1) / strip);
    hipLaunchKernelGGL((colsum_exact_kernel<VEC>), dim3(blocks), dim3(tx * ny),
                       (size_t)lds, stream, (const uint16_t*)gy, R, C,
                       (uint16_t*)dst, tx_shift, bh, ctas);
    return true;
}

}  // namespace

// bh / ctas: torch's block height and blocks per output for this reduction
// (bh = 1, ctas = 1 when torch does not split the rows over threadIdx.y).
// Returns 0 when the configuration does not fit the kernel; nothing is
// launched then.
extern "C" int launch_colsum_exact_bf16(const void* gy, int64_t R, int64_t C,
                                        void* dst, int bh, int ctas,
                                        hipStream_t stream) {
    if (C <= 0 || R <= 0 || bh < 1 || ctas < 1 || (bh & (bh - 1)) != 0) return 0;
    const uintptr_t a = (uintptr_t)gy;
    if (C % 8 == 0 && (a & 15) == 0)
        return dgx_launch<8>(gy, R, C, dst, bh, ctas, stream);
    if (C % 4 == 0 && (a & 7) == 0)
        return dgx_launch<4>(gy, R, C, dst, bh, ctas, stream);
    if (C % 2 == 0 && (a & 3) == 0)
        return dgx_launch<2>(gy, R, C, dst, bh, ctas, stream);
    return dgx_launch<1>(gy, R, C, dst, bh, ctas, stream);
}

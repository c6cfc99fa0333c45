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

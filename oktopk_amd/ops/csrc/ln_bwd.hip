// LayerNorm backward with the gamma/beta gradients written into their
// gradient slots.  Two launches, no zeroing, no atomics:
//
//   1. ln_bwd_rows: one wave per row, fp32 math.  gx = rstd * (g - mean(g)
//      - xhat * mean(g * xhat)) with g = gy * gamma, xhat = (x - mean) *
//      rstd.  Each lane keeps its columns' gy*xhat and gy sums in registers
//      over the rows its wave visits; the block's 4 waves are folded through
//      LDS and one fp32 partial row [2, H] per block goes to the workspace.
//      The grid is rows / 4 blocks (256 at 1024 rows: every CU gets one).
//   2. ln_bwd_reduce: sums the per-block partials in a fixed order and
//      stores bf16 into the gamma and beta slots (overwrite or accumulate),
//      with 2-byte stores so the slots may sit at any element offset.
//
// H = 128 * NK, NK in {1, 2, 4, 6, 8}: lane l owns columns k*128 + 2l, +1
// (one 4-byte load per operand per k, 256 contiguous bytes per wave).
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr int LN_WAVES = 4;
constexpr int LN_THREADS = LN_WAVES * 64;

__device__ __forceinline__ float ln_b2f(uint32_t bits16) {
    return __uint_as_float(bits16 << 16);
}

__device__ __forceinline__ uint32_t ln_f2b(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

template <int NK>
__global__ __launch_bounds__(LN_THREADS)
void ln_bwd_rows_kernel(const uint16_t* __restrict__ gy,
                        const uint16_t* __restrict__ x,
                        const uint16_t* __restrict__ gamma,
                        const float* __restrict__ mean,
                        const float* __restrict__ rstd, int64_t rows,
                        uint16_t* __restrict__ gx, float* __restrict__ ws) {
    constexpr int H = NK * 128;
    __shared__ float part[LN_WAVES][2 * H];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    float gam[NK][2], dg[NK][2], db[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = k * 128 + 2 * lane;
        gam[k][0] = ln_b2f(gamma[c]);       // 2-byte loads: any alignment
        gam[k][1] = ln_b2f(gamma[c + 1]);
        dg[k][0] = dg[k][1] = db[k][0] = db[k][1] = 0.f;
    }

    for (int64_t row = (int64_t)blockIdx.x * LN_WAVES + wave; row < rows;
         row += (int64_t)gridDim.x * LN_WAVES) {
        const uint32_t* gyr = reinterpret_cast<const uint32_t*>(gy + row * H);
        const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + row * H);
        uint32_t gv[NK], xv[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            gv[k] = gyr[k * 64 + lane];
            xv[k] = xr[k * 64 + lane];
        }
        const float m = mean[row], rs = rstd[row];
        float xh[NK][2], g[NK][2];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float gy0 = ln_b2f(gv[k] & 0xffffu), gy1 = ln_b2f(gv[k] >> 16);
            xh[k][0] = (ln_b2f(xv[k] & 0xffffu) - m) * rs;
            xh[k][1] = (ln_b2f(xv[k] >> 16) - m) * rs;
            g[k][0] = gy0 * gam[k][0];
            g[k][1] = gy1 * gam[k][1];
            s1 += g[k][0] + g[k][1];
            s2 += g[k][0] * xh[k][0] + g[k][1] * xh[k][1];
            dg[k][0] += gy0 * xh[k][0];
            dg[k][1] += gy1 * xh[k][1];
            db[k][0] += gy0;
            db[k][1] += gy1;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
        }
        const float c1 = s1 * (1.0f / H), c2 = s2 * (1.0f / H);
        uint32_t* gxr = reinterpret_cast<uint32_t*>(gx + row * H);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float o0 = rs * (g[k][0] - c1 - xh[k][0] * c2);
            const float o1 = rs * (g[k][1] - c1 - xh[k][1] * c2);
            gxr[k * 64 + lane] = ln_f2b(o0) | (ln_f2b(o1) << 16);
        }
    }

#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = k * 128 + 2 * lane;
        part[wave][c] = dg[k][0];
        part[wave][c + 1] = dg[k][1];
        part[wave][H + c] = db[k][0];
        part[wave][H + c + 1] = db[k][1];
    }
    __syncthreads();
    float* out = ws + (int64_t)blockIdx.x * (2 * H);
    for (int i = threadIdx.x; i < 2 * H; i += LN_THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < LN_WAVES; ++w) s += part[w][i];
        out[i] = s;
    }
}

// partials fp32 [P, 2H] -> bf16 gamma slot [H], beta slot [H].  256 threads:
// 32 columns x 8 partial-row groups, folded through LDS.
__global__ __launch_bounds__(256)
void ln_bwd_reduce_kernel(const float* __restrict__ ws, int P, int H,
                          uint16_t* __restrict__ dgamma,
                          uint16_t* __restrict__ dbeta, int accumulate) {
    __shared__ float part[8][32];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + tx;   // 2H is a multiple of 32
    float s = 0.f;
    for (int p = ty; p < P; p += 8) s += ws[(int64_t)p * (2 * H) + col];
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += part[w][tx];
        uint16_t* dst = col < H ? dgamma + col : dbeta + (col - H);
        if (accumulate) t += ln_b2f(*dst);
        *dst = (uint16_t)ln_f2b(t);
    }
}

template <int NK>
void ln_rows_launch(const void* gy, const void* x, const void* gamma,
                    const float* mean, const float* rstd, int64_t rows,
                    void* gx, float* ws, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL((ln_bwd_rows_kernel<NK>), dim3(blocks), dim3(LN_THREADS),
                       0, stream, (const uint16_t*)gy, (const uint16_t*)x,
                       (const uint16_t*)gamma, mean, rstd, rows, (uint16_t*)gx,
                       ws);
}

}  // namespace

extern "C" bool ln_bwd_supported(int64_t H) {
    return H == 128 || H == 256 || H == 512 || H == 768 || H == 1024;
}

// blocks the row kernel uses (= partial rows the workspace must hold)
extern "C" int ln_bwd_blocks(int64_t rows) {
    int64_t b = (rows + LN_WAVES - 1) / LN_WAVES;
    if (b < 1) b = 1;
    if (b > 512) b = 512;
    return (int)b;
}

extern "C" void launch_ln_bwd_into(const void* gy, const void* x,
                                   const void* gamma, const float* mean,
                                   const float* rstd, int64_t rows, int64_t H,
                                   void* gx, float* ws, void* dgamma,
                                   void* dbeta, int accumulate,
                                   hipStream_t stream) {
    const int blocks = ln_bwd_blocks(rows);
    switch (H) {
        case 128:  ln_rows_launch<1>(gy, x, gamma, mean, rstd, rows, gx, ws, blocks, stream); break;
        case 256:  ln_rows_launch<2>(gy, x, gamma, mean, rstd, rows, gx, ws, blocks, stream); break;
        case 512:  ln_rows_launch<4>(gy, x, gamma, mean, rstd, rows, gx, ws, blocks, stream); break;
        case 768:  ln_rows_launch<6>(gy, x, gamma, mean, rstd, rows, gx, ws, blocks, stream); break;
        case 1024: ln_rows_launch<8>(gy, x, gamma, mean, rstd, rows, gx, ws, blocks, stream); break;
        default: return;
    }
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((unsigned)(2 * H / 32)),
                       dim3(256), 0, stream, ws, blocks, (int)H,
                       (uint16_t*)dgamma, (uint16_t*)dbeta, accumulate);
}

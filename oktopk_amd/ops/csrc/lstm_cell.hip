// Fused fp32 LSTM recurrent step for gfx950 (CDNA4), forward and backward.
//
// One launch per time step; launches on one stream are the only ordering
// between steps.  Both step kernels are the same shape of work: a skinny
// product D[m][n] = sum_k A[m][k] * B[n][k] with 16 rows of a weight matrix
// (A, read once per step over the whole grid) against the batch tile (B, 16
// rows of the previous step's state), followed by the cell's pointwise part
// for the hidden units the block owns.
//
//   forward   A = the four gate rows of FWD_UNITS hidden units of W_hh
//             [4H, H], B = h_{prev} [N, H], K = H
//   backward  A = BWD_UNITS rows of W_hh^T [H, 4H], B = dgates_{next}
//             [N, 4H], K = 4H
//
// The product runs on v_mfma_f32_16x16x4_f32.  A lane holds A[lane % 16][k]
// and B[lane % 16][k] with k picked by lane / 16, so a lane reads four
// consecutive k of one row (one 16-byte load when the row is aligned) and
// feeds them to four MFMAs with four independent accumulators: MFMA c of a
// 16-wide K chunk sums k = chunk + 4 * (lane / 16) + c over the four lane
// quads.  A and B use the same k for the same lane, which is all the
// instruction asks.  The block's waves take K chunks round robin, write
// their partial 16x16 tiles to LDS, and the pointwise threads add them in
// wave order: no atomics, the same bits on every run.
//
// Arithmetic contract (csrc/README.md, "Fused LSTM step"): fp32 throughout,
// sigmoid(x) = 1 / (1 + expf(-x)), tanhf, no fast-math.

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;    // MFMA M (weight rows) and N (batch rows)
constexpr int KCHUNK = 16;  // K of one group of four MFMAs
constexpr int WAVE = 64;
constexpr int DEPTH = 4;    // K chunks a wave loads before it multiplies

// Forward: 4 units x 4 gates fill M exactly; H / 4 blocks (200 at H = 800).
constexpr int FWD_UNITS = 4;
constexpr int FWD_WAVES = 8;
// Backward: 8 of the 16 MFMA rows are live.  A full tile gives H / 16 blocks
// (50 at H = 800, a fifth of the CUs); halving it doubles the blocks that
// pull W_hh^T, at the price of every block re-reading dgates_{next}.
constexpr int BWD_UNITS = 8;
constexpr int BWD_WAVES = 16;

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p) {
    if (VEC) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v;
    v.x = p[0];
    v.y = p[1];
    v.z = p[2];
    v.w = p[3];
    return v;
}

// This wave's share of the block's 16x16 tile.  a_row / b_row: the row this
// lane feeds (nullptr: a row of zeros, nothing is read).  K % 4 == 0, so a
// lane's four k are inside K together or not at all.  The loop bounds are
// wave-uniform and the loads reconverge before the MFMAs.
template <bool VEC, int WAVES>
__device__ __forceinline__ f32x4 wave_product(const float* a_row,
                                              const float* b_row, int K,
                                              int wave, int quad) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc0 = zero, acc1 = zero, acc2 = zero, acc3 = zero;
    // DEPTH chunks per trip, every load issued ahead of the MFMAs so that a
    // wave has 2 * DEPTH 16-byte loads in flight; a chunk past K adds zeros
    for (int k0 = wave * KCHUNK; k0 < K; k0 += DEPTH * WAVES * KCHUNK) {
        f32x4 a[DEPTH], b[DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int k = k0 + d * WAVES * KCHUNK + 4 * quad;
            a[d] = zero;
            b[d] = zero;
            if (k < K) {
                if (a_row != nullptr) a[d] = load4<VEC>(a_row + k);
                if (b_row != nullptr) b[d] = load4<VEC>(b_row + k);
            }
        }
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].x, b[d].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].y, b[d].y, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].z, b[d].z, acc2, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].w, b[d].w, acc3, 0, 0, 0);
        }
    }
    return (acc0 + acc1) + (acc2 + acc3);
}

// D[m][n] of the MFMA sits in lane n + 16 * (m / 4), register m % 4.
template <int WAVES>
__device__ __forceinline__ void store_partial(float (*part)[TILE][TILE + 1],
                                              f32x4 d, int wave, int quad,
                                              int col) {
    part[wave][4 * quad + 0][col] = d.x;
    part[wave][4 * quad + 1][col] = d.y;
    part[wave][4 * quad + 2][col] = d.z;
    part[wave][4 * quad + 3][col] = d.w;
}

template <int WAVES>
__device__ __forceinline__ float sum_partials(float (*part)[TILE][TILE + 1],
                                              int m, int n) {
    float s = part[0][m][n];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += part[w][m][n];
    return s;
}

__device__ __forceinline__ float sigmoidf(float x) {
    return 1.f / (1.f + expf(-x));
}

// gx_t [N, 4H]: pre-activations from the input projection in, activations
// (i, f, g, o) out.  h_prev / c_prev [N, H] are nullptr at the first step of
// the recurrence (zero state: no product).  grid = (H / 4, ceil(N / 16)).
template <bool VEC>
__global__ __launch_bounds__(FWD_WAVES* WAVE) void lstm_fwd_step(
    float* __restrict__ gx_t, const float* __restrict__ w_hh,
    const float* __restrict__ h_prev, const float* __restrict__ c_prev,
    float* __restrict__ y_t, float* __restrict__ c_t, int N, int H) {
    __shared__ float part[FWD_WAVES][TILE][TILE + 1];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * FWD_UNITS;
    const int nb = blockIdx.y * TILE;

    if (h_prev != nullptr) {
        const int lane = tid % WAVE, wave = tid / WAVE;
        const int col = lane % TILE, quad = lane / TILE;
        // MFMA row m = gate * 4 + unit
        const float* a_row =
            w_hh + ((size_t)(col / FWD_UNITS) * H + j0 + col % FWD_UNITS) * H;
        const float* b_row =
            nb + col < N ? h_prev + (size_t)(nb + col) * H : nullptr;
        f32x4 d = wave_product<VEC, FWD_WAVES>(a_row, b_row, H, wave, quad);
        store_partial<FWD_WAVES>(part, d, wave, quad, col);
        __syncthreads();
    }

    if (tid >= FWD_UNITS * TILE) return;
    const int u = tid % FWD_UNITS, n = tid / FWD_UNITS;
    if (nb + n >= N) return;
    const size_t row = (size_t)(nb + n);
    const int j = j0 + u;  // < H: H % 4 == 0 and gridDim.x == H / 4
    float* g = gx_t + row * 4 * H + j;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pre[q] = g[(size_t)q * H];
        if (h_prev != nullptr)
            pre[q] += sum_partials<FWD_WAVES>(part, q * FWD_UNITS + u, n);
    }
    const float ig = sigmoidf(pre[0]);
    const float fg = sigmoidf(pre[1]);
    const float gg = tanhf(pre[2]);
    const float og = sigmoidf(pre[3]);
    float c = ig * gg;
    if (c_prev != nullptr) c += fg * c_prev[row * H + j];
    g[0] = ig;
    g[(size_t)H] = fg;
    g[(size_t)2 * H] = gg;
    g[(size_t)3 * H] = og;
    c_t[row * H + j] = c;
    y_t[row * H + j] = og * tanhf(c);
}

// One backward step.  dg_next [N, 4H] is the step after this one in the
// recurrence (nullptr at its last step: no product and a zero carry);
// c_prev is nullptr at its first step.  dc_carry [N, H] is read and written
// by the one thread that owns the element.  grid = (ceil(H / 8), ceil(N / 16)).
template <bool VEC>
__global__ __launch_bounds__(BWD_WAVES* WAVE) void lstm_bwd_step(
    const float* __restrict__ gy_t, const float* __restrict__ act_t,
    const float* __restrict__ c_t, const float* __restrict__ c_prev,
    const float* __restrict__ w_hh_t, const float* __restrict__ dg_next,
    float* __restrict__ dc_carry, float* __restrict__ dg_t, int N, int H) {
    __shared__ float part[BWD_WAVES][TILE][TILE + 1];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * BWD_UNITS;
    const int nb = blockIdx.y * TILE;

    if (dg_next != nullptr) {
        const int lane = tid % WAVE, wave = tid / WAVE;
        const int col = lane % TILE, quad = lane / TILE;
        const float* a_row = (col < BWD_UNITS && j0 + col < H)
                                 ? w_hh_t + (size_t)(j0 + col) * 4 * H
                                 : nullptr;
        const float* b_row =
            nb + col < N ? dg_next + (size_t)(nb + col) * 4 * H : nullptr;
        f32x4 d = wave_product<VEC, BWD_WAVES>(a_row, b_row, 4 * H, wave, quad);
        store_partial<BWD_WAVES>(part, d, wave, quad, col);
        __syncthreads();
    }

    if (tid >= BWD_UNITS * TILE) return;
    const int u = tid % BWD_UNITS, n = tid / BWD_UNITS;
    const int j = j0 + u;
    if (j >= H || nb + n >= N) return;
    const size_t row = (size_t)(nb + n);
    const size_t e = row * H + j;
    const float* a = act_t + row * 4 * H + j;
    const float ig = a[0];
    const float fg = a[(size_t)H];
    const float gg = a[(size_t)2 * H];
    const float og = a[(size_t)3 * H];

    float dh = gy_t[e];
    float dc = 0.f;
    if (dg_next != nullptr) {
        dh += sum_partials<BWD_WAVES>(part, u, n);
        dc = dc_carry[e];
    }
    const float tc = tanhf(c_t[e]);
    dc += dh * og * (1.f - tc * tc);
    const float cp = c_prev != nullptr ? c_prev[e] : 0.f;
    dc_carry[e] = dc * fg;

    float* dg = dg_t + row * 4 * H + j;
    dg[0] = dc * gg * ig * (1.f - ig);
    dg[(size_t)H] = dc * cp * fg * (1.f - fg);
    dg[(size_t)2 * H] = dc * ig * (1.f - gg * gg);
    dg[(size_t)3 * H] = dh * tc * og * (1.f - og);
}

inline bool aligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

}  // namespace

// Step s of the recurrence is time t = s, or T - 1 - s when reversed; a
// step's neighbours in the recurrence are one time index away either side.
// Row strides (H and 4H floats, H % 4 == 0) keep every time slice as aligned
// as its base pointer, so one alignment decision holds for the whole call.

extern "C" void launch_lstm_fwd(float* gx, const float* w_hh, float* y,
                                float* c, int T, int N, int H, int reverse,
                                hipStream_t stream) {
    const dim3 grid(H / FWD_UNITS, (N + TILE - 1) / TILE);
    const dim3 block(FWD_WAVES * WAVE);
    const bool vec = aligned16(w_hh, y);
    const size_t nh = (size_t)N * H;
    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        const int tp = reverse ? t + 1 : t - 1;
        const float* h_prev = s > 0 ? y + tp * nh : nullptr;
        const float* c_prev = s > 0 ? c + tp * nh : nullptr;
        float* gx_t = gx + t * 4 * nh;
        if (vec)
            hipLaunchKernelGGL(lstm_fwd_step<true>, grid, block, 0, stream,
                               gx_t, w_hh, h_prev, c_prev, y + t * nh,
                               c + t * nh, N, H);
        else
            hipLaunchKernelGGL(lstm_fwd_step<false>, grid, block, 0, stream,
                               gx_t, w_hh, h_prev, c_prev, y + t * nh,
                               c + t * nh, N, H);
    }
}

extern "C" void launch_lstm_bwd(const float* gy, const float* act,
                                const float* c, const float* w_hh_t,
                                float* dc_carry, float* dgates, int T, int N,
                                int H, int reverse, hipStream_t stream) {
    const dim3 grid((H + BWD_UNITS - 1) / BWD_UNITS, (N + TILE - 1) / TILE);
    const dim3 block(BWD_WAVES * WAVE);
    const bool vec = aligned16(w_hh_t, dgates);
    const size_t nh = (size_t)N * H;
    for (int s = T - 1; s >= 0; --s) {
        const int t = reverse ? T - 1 - s : s;
        const int tp = reverse ? t + 1 : t - 1;  // step s - 1
        const int tn = reverse ? t - 1 : t + 1;  // step s + 1
        const float* c_prev = s > 0 ? c + tp * nh : nullptr;
        const float* dg_next = s < T - 1 ? dgates + tn * 4 * nh : nullptr;
        if (vec)
            hipLaunchKernelGGL(lstm_bwd_step<true>, grid, block, 0, stream,
                               gy + t * nh, act + t * 4 * nh, c + t * nh,
                               c_prev, w_hh_t, dg_next, dc_carry,
                               dgates + t * 4 * nh, N, H);
        else
            hipLaunchKernelGGL(lstm_bwd_step<false>, grid, block, 0, stream,
                               gy + t * nh, act + t * 4 * nh, c + t * nh,
                               c_prev, w_hh_t, dg_next, dc_carry,
                               dgates + t * 4 * nh, N, H);
    }
}

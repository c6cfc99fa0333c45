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
// A block owns NB = 1 or 2 batch tiles.  With NB = 2 a lane's A fragment is
// loaded once per K chunk and feeds two MFMAs, one per batch tile, into two
// accumulator sets of their own; each tile sees the chunks, and its partials
// the waves, in the order they have with NB = 1, so the bits are the same
// and the grid reads the weight matrix once per 32 batch rows instead of 16.
//
// State: the recurrence may start from (h0, c0) instead of zeros, the
// backward pass may take gradients at the final (h, c), and then gives the
// gradients at (h0, c0): dc0 is the carry after the last launch, dh0 one
// product-only launch after it.
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

// This wave's share of the block's NB 16x16 tiles, into out.  a_row /
// b_row[i]: the row this lane feeds (nullptr: a row of zeros, nothing is
// read).  K % 4 == 0, so a lane's four k are inside K together or not at all.
// The loop bounds are wave-uniform and the loads reconverge before the MFMAs.
template <bool VEC, int WAVES, int NB>
__device__ __forceinline__ void wave_product(const float* a_row,
                                             const float* const (&b_row)[NB],
                                             int K, int wave, int quad,
                                             f32x4 (&out)[NB]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i)
        acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = zero;
    // DEPTH chunks per trip, every load issued ahead of the MFMAs so that a
    // wave has (1 + NB) * DEPTH 16-byte loads in flight; a chunk past K adds
    // zeros
    for (int k0 = wave * KCHUNK; k0 < K; k0 += DEPTH * WAVES * KCHUNK) {
        f32x4 a[DEPTH], b[NB][DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int k = k0 + d * WAVES * KCHUNK + 4 * quad;
            a[d] = zero;
#pragma unroll
            for (int i = 0; i < NB; ++i) b[i][d] = zero;
            if (k < K) {
                if (a_row != nullptr) a[d] = load4<VEC>(a_row + k);
#pragma unroll
                for (int i = 0; i < NB; ++i)
                    if (b_row[i] != nullptr) b[i][d] = load4<VEC>(b_row[i] + k);
            }
        }
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].x, b[i][d].x, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].y, b[i][d].y, acc[i][1], 0, 0, 0);
                acc[i][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].z, b[i][d].z, acc[i][2], 0, 0, 0);
                acc[i][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d].w, b[i][d].w, acc[i][3], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
        out[i] = (acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]);
}

// D[m][n] of the MFMA sits in lane n + 16 * (m / 4), register m % 4.
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
// (i, f, g, o) out.  h_prev / c_prev [N, H] are the previous step's, or the
// initial state at the first step of the recurrence; nullptr there for a
// zero state (no product).  grid = (H / 4, ceil(N / (16 * NB))).
template <bool VEC, int NB>
__global__ __launch_bounds__(FWD_WAVES* WAVE) void lstm_fwd_step(
    float* __restrict__ gx_t, const float* __restrict__ w_hh,
    const float* __restrict__ h_prev, const float* __restrict__ c_prev,
    float* __restrict__ y_t, float* __restrict__ c_t, int N, int H) {
    __shared__ float part[NB][FWD_WAVES][TILE][TILE + 1];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * FWD_UNITS;
    const int nb = blockIdx.y * (NB * TILE);

    if (h_prev != nullptr) {
        const int lane = tid % WAVE, wave = tid / WAVE;
        const int col = lane % TILE, quad = lane / TILE;
        // MFMA row m = gate * 4 + unit
        const float* a_row =
            w_hh + ((size_t)(col / FWD_UNITS) * H + j0 + col % FWD_UNITS) * H;
        const float* b_row[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int r = nb + i * TILE + col;
            b_row[i] = r < N ? h_prev + (size_t)r * H : nullptr;
        }
        f32x4 d[NB];
        wave_product<VEC, FWD_WAVES, NB>(a_row, b_row, H, wave, quad, d);
#pragma unroll
        for (int i = 0; i < NB; ++i) store_partial(part[i], d[i], wave, quad, col);
        __syncthreads();
    }

    if (tid >= NB * FWD_UNITS * TILE) return;
    const int tile = tid / (FWD_UNITS * TILE);
    const int u = tid % FWD_UNITS, n = tid % (FWD_UNITS * TILE) / FWD_UNITS;
    if (nb + tile * TILE + n >= N) return;
    const size_t row = (size_t)(nb + tile * TILE + n);
    const int j = j0 + u;  // < H: H % 4 == 0 and gridDim.x == H / 4
    float* g = gx_t + row * 4 * H + j;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pre[q] = g[(size_t)q * H];
        if (h_prev != nullptr)
            pre[q] += sum_partials<FWD_WAVES>(part[tile], q * FWD_UNITS + u, n);
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

// The backward product of a block: partial tiles of dg [N, 4H] @ W_hh
// restricted to units j0 .. j0 + 7 and batch rows nb .. nb + 16 * NB - 1,
// left in part for sum_partials after the barrier.
template <bool VEC, int NB>
__device__ __forceinline__ void bwd_product(
    float (*part)[BWD_WAVES][TILE][TILE + 1], const float* w_hh_t,
    const float* dg, int j0, int nb, int N, int H) {
    const int tid = threadIdx.x;
    const int lane = tid % WAVE, wave = tid / WAVE;
    const int col = lane % TILE, quad = lane / TILE;
    const float* a_row = (col < BWD_UNITS && j0 + col < H)
                             ? w_hh_t + (size_t)(j0 + col) * 4 * H
                             : nullptr;
    const float* b_row[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int r = nb + i * TILE + col;
        b_row[i] = r < N ? dg + (size_t)r * 4 * H : nullptr;
    }
    f32x4 d[NB];
    wave_product<VEC, BWD_WAVES, NB>(a_row, b_row, 4 * H, wave, quad, d);
#pragma unroll
    for (int i = 0; i < NB; ++i) store_partial(part[i], d[i], wave, quad, col);
    __syncthreads();
}

// One backward step.  dg_next [N, 4H] is the step after this one in the
// recurrence (nullptr at its last step: no product and a zero carry); c_prev
// is the step before, c0 at the first step, nullptr for a zero state.
// dc_carry [N, H] is read and written by the one thread that owns the
// element.  FINAL is the last step of a recurrence whose final state has
// gradients: g_h / g_c [N, H] (either may be nullptr) join gy_t and stand in
// for the carry, and there is no product; every other step compiles without
// them.  grid = (ceil(H / 8), ceil(N / (16 * NB))).
template <bool VEC, int NB, bool FINAL>
__global__ __launch_bounds__(BWD_WAVES* WAVE) void lstm_bwd_step(
    const float* __restrict__ gy_t, const float* __restrict__ g_h,
    const float* __restrict__ g_c, const float* __restrict__ act_t,
    const float* __restrict__ c_t, const float* __restrict__ c_prev,
    const float* __restrict__ w_hh_t, const float* __restrict__ dg_next,
    float* __restrict__ dc_carry, float* __restrict__ dg_t, int N, int H) {
    __shared__ float part[FINAL ? 1 : NB][FINAL ? 1 : BWD_WAVES][TILE][TILE + 1];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * BWD_UNITS;
    const int nb = blockIdx.y * (NB * TILE);

    if constexpr (!FINAL) {
        if (dg_next != nullptr)
            bwd_product<VEC, NB>(part, w_hh_t, dg_next, j0, nb, N, H);
    }

    if (tid >= NB * BWD_UNITS * TILE) return;
    const int tile = tid / (BWD_UNITS * TILE);
    const int u = tid % BWD_UNITS, n = tid % (BWD_UNITS * TILE) / BWD_UNITS;
    const int j = j0 + u;
    if (j >= H || nb + tile * TILE + n >= N) return;
    const size_t row = (size_t)(nb + tile * TILE + n);
    const size_t e = row * H + j;
    const float* a = act_t + row * 4 * H + j;
    const float ig = a[0];
    const float fg = a[(size_t)H];
    const float gg = a[(size_t)2 * H];
    const float og = a[(size_t)3 * H];

    float dh = gy_t[e];
    float dc = 0.f;
    if constexpr (FINAL) {
        if (g_h != nullptr) dh += g_h[e];
        if (g_c != nullptr) dc = g_c[e];
    } else if (dg_next != nullptr) {
        dh += sum_partials<BWD_WAVES>(part[tile], u, n);
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

// dh0 [N, H] = dg_first [N, 4H] @ W_hh: the backward step's product on its
// own, for the gradient at the initial h.  Same grid as lstm_bwd_step.
template <bool VEC, int NB>
__global__ __launch_bounds__(BWD_WAVES* WAVE) void lstm_bwd_dh0(
    const float* __restrict__ w_hh_t, const float* __restrict__ dg_first,
    float* __restrict__ dh0, int N, int H) {
    __shared__ float part[NB][BWD_WAVES][TILE][TILE + 1];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * BWD_UNITS;
    const int nb = blockIdx.y * (NB * TILE);

    bwd_product<VEC, NB>(part, w_hh_t, dg_first, j0, nb, N, H);

    if (tid >= NB * BWD_UNITS * TILE) return;
    const int tile = tid / (BWD_UNITS * TILE);
    const int u = tid % BWD_UNITS, n = tid % (BWD_UNITS * TILE) / BWD_UNITS;
    const int j = j0 + u;
    if (j >= H || nb + tile * TILE + n >= N) return;
    const size_t row = (size_t)(nb + tile * TILE + n);
    dh0[row * H + j] = sum_partials<BWD_WAVES>(part[tile], u, n);
}

inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// batch_tiles 1 or 2 as asked.  0 (auto) is what was measured, at T = 35
// (profiles/README.md r18): the forward step is no faster with a pair at
// H = 1500 (+2 %), so it keeps single tiles.  The backward step gains 8 %
// there and loses 40 - 55 % at H = 800, where the pair halves a grid of 200
// blocks and the second read of the 10 MB W_hh^T is served by the L2s; it
// takes a pair when a second tile has rows to hold and W_hh^T (16 H^2 bytes)
// is larger than the eight 4 MB L2s together.
inline int pick_batch_tiles(int batch_tiles, int N, int H, bool backward) {
    if (batch_tiles == 1 || batch_tiles == 2) return batch_tiles;
    return backward && N > TILE && (size_t)16 * H * H > ((size_t)32 << 20) ? 2 : 1;
}

// Step s of the recurrence is time t = s, or T - 1 - s when reversed; a
// step's neighbours in the recurrence are one time index away either side.
// Row strides (H and 4H floats, H % 4 == 0) keep every time slice as aligned
// as its base pointer, so one alignment decision holds for the whole call.

template <bool VEC, int NB>
void lstm_fwd_loop(float* gx, const float* w_hh, const float* h0,
                   const float* c0, float* y, float* c, int T, int N, int H,
                   int reverse, hipStream_t stream) {
    const dim3 grid(H / FWD_UNITS, (N + NB * TILE - 1) / (NB * TILE));
    const dim3 block(FWD_WAVES * WAVE);
    const size_t nh = (size_t)N * H;
    for (int s = 0; s < T; ++s) {
        const int t = reverse ? T - 1 - s : s;
        const int tp = reverse ? t + 1 : t - 1;
        const float* h_prev = s > 0 ? y + tp * nh : h0;
        const float* c_prev = s > 0 ? c + tp * nh : c0;
        hipLaunchKernelGGL((lstm_fwd_step<VEC, NB>), grid, block, 0, stream,
                           gx + t * 4 * nh, w_hh, h_prev, c_prev, y + t * nh,
                           c + t * nh, N, H);
    }
}

template <bool VEC, int NB>
void lstm_bwd_loop(const float* gy, const float* g_hn, const float* g_cn,
                   const float* act, const float* c, const float* c0,
                   const float* w_hh_t, float* dc_carry, float* dgates,
                   float* dh0, int T, int N, int H, int reverse,
                   hipStream_t stream) {
    const dim3 grid((H + BWD_UNITS - 1) / BWD_UNITS,
                    (N + NB * TILE - 1) / (NB * TILE));
    const dim3 block(BWD_WAVES * WAVE);
    const size_t nh = (size_t)N * H;
    for (int s = T - 1; s >= 0; --s) {
        const int t = reverse ? T - 1 - s : s;
        const int tp = reverse ? t + 1 : t - 1;  // step s - 1
        const int tn = reverse ? t - 1 : t + 1;  // step s + 1
        const float* c_prev = s > 0 ? c + tp * nh : c0;
        const float* dg_next = s < T - 1 ? dgates + tn * 4 * nh : nullptr;
        if (s == T - 1 && (g_hn != nullptr || g_cn != nullptr))
            hipLaunchKernelGGL((lstm_bwd_step<VEC, NB, true>), grid, block, 0,
                               stream, gy + t * nh, g_hn, g_cn,
                               act + t * 4 * nh, c + t * nh, c_prev, w_hh_t,
                               nullptr, dc_carry, dgates + t * 4 * nh, N, H);
        else
            hipLaunchKernelGGL((lstm_bwd_step<VEC, NB, false>), grid, block, 0,
                               stream, gy + t * nh, nullptr, nullptr,
                               act + t * 4 * nh, c + t * nh, c_prev, w_hh_t,
                               dg_next, dc_carry, dgates + t * 4 * nh, N, H);
    }
    if (dh0 != nullptr) {
        const int t0 = reverse ? T - 1 : 0;
        hipLaunchKernelGGL((lstm_bwd_dh0<VEC, NB>), grid, block, 0, stream,
                           w_hh_t, dgates + t0 * 4 * nh, dh0, N, H);
    }
}

}  // namespace

// h0 / c0 [N, H]: the initial state, nullptr for zeros.
extern "C" void launch_lstm_fwd(float* gx, const float* w_hh, const float* h0,
                                const float* c0, float* y, float* c, int T,
                                int N, int H, int reverse, int batch_tiles,
                                hipStream_t stream) {
    const bool vec = aligned16(w_hh, y, h0);
    const bool pair = pick_batch_tiles(batch_tiles, N, H, false) == 2;
    auto loop = vec ? (pair ? lstm_fwd_loop<true, 2> : lstm_fwd_loop<true, 1>)
                    : (pair ? lstm_fwd_loop<false, 2> : lstm_fwd_loop<false, 1>);
    loop(gx, w_hh, h0, c0, y, c, T, N, H, reverse, stream);
}

// g_hn / g_cn [N, H]: gradients at the final state, nullptr for zeros.  c0:
// the initial cell state lstm_fwd ran from.  dc_carry ends as the gradient at
// c0; dh0, when not nullptr, receives the gradient at h0.
extern "C" void launch_lstm_bwd(const float* gy, const float* g_hn,
                                const float* g_cn, const float* act,
                                const float* c, const float* c0,
                                const float* w_hh_t, float* dc_carry,
                                float* dgates, float* dh0, int T, int N, int H,
                                int reverse, int batch_tiles,
                                hipStream_t stream) {
    const bool vec = aligned16(w_hh_t, dgates);
    const bool pair = pick_batch_tiles(batch_tiles, N, H, true) == 2;
    auto loop = vec ? (pair ? lstm_bwd_loop<true, 2> : lstm_bwd_loop<true, 1>)
                    : (pair ? lstm_bwd_loop<false, 2> : lstm_bwd_loop<false, 1>);
    loop(gy, g_hn, g_cn, act, c, c0, w_hh_t, dc_carry, dgates, dh0, T, N, H,
         reverse, stream);
}

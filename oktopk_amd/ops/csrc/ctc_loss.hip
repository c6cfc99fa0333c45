// Fused CTC loss for gfx950 (CDNA4): negative log-likelihood per utterance
// from the raw logits and, in the same launch, its gradient with respect to
// the raw logits.  The log-softmax is fused in and never materialised;
// lengths and targets are read on the device, nothing goes through the host.
//
// One block of 256 threads (4 waves) per utterance.  S = 2L + 1 states of
// the blank-extended target l'.
//
//   set-up   l' and, for the gradient, the chain "next odd state with the
//            same label" with its head flags, once per utterance, in LDS.
//   phase A  all waves: the row maximum and log(sum exp(x - max)) of
//            logits[t, n, :], one wave per row, lanes striding over C;
//            lp[t][s] = (logits[t, n, l'_s] - max) - log(sum) written into
//            BOTH lattices, where the recursions read it.
//   phase B  wave 0 walks alpha t = 0 -> len-1 while wave 1 walks beta t =
//            len-1 -> 0 (only alpha when no gradient is wanted).  A lane holds
//            K consecutive states in registers (K = 1, 2, 4: S <= 64 K); the
//            two neighbour states a lane lacks come from the lane next to it
//            by a wave shuffle, so the time loop has no barrier.  Each wave
//            reads lp[t] from its own lattice PF steps ahead and overwrites
//            that row with its result: two [T][S] lattices hold everything.
//              alpha_t(s): emission at t included
//              beta'_t(s): emission at t excluded,
//            so alpha_t(s) + beta'_t(s) + nll is the log posterior of state
//            s at time t and phase C needs no lp.
//   phase C  all waves, after one barrier: nll, then softmax(t, c) for every
//            t < len, coalesced along c; after one more barrier one wave per
//            row subtracts the posteriors: blank by a fixed-order wave
//            reduction over its states, each label by the lane that owns the
//            head of its chain, walking the chain in state order.  No float
//            atomics: the same bits on every run.  Rows t >= len are 0.
//
// The lattices and the two row statistics live in LDS (LAT_LDS) when
// T (2 Sst + 2) floats fit CTC_LDS_BUDGET, else in a global workspace
// [N][T (2 Sst + 2)] — the same code, templated on where the pointer goes.
// Sst is the row stride the host derives from shapes alone: 2 Lmax + 1 for
// padded targets, 255 for 1-D.
//
// An utterance whose S exceeds Sst (a target longer than the padded width, or
// than 127) gets NaN loss and a zero gradient.  A label outside [0, C) is an
// impossible emission (-inf) and is never used as an index.  All arithmetic
// is fp32 in log space with expf / logf, no fast-math; log-add of -inf
// operands is -inf, never NaN.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ctc_loss.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_S = 256;  // 64 lanes x K = 4 states
constexpr int PF = 4;       // lp rows in flight ahead of the recursion
constexpr float NEG = -INFINITY;

__device__ __forceinline__ long long load_int(const void* p, long long i,
                                              int is64) {
    return is64 ? static_cast<const long long*>(p)[i]
                : static_cast<long long>(static_cast<const int*>(p)[i]);
}

__device__ __forceinline__ float logadd3(float x, float y, float z) {
    const float m = fmaxf(fmaxf(x, y), z);
    if (m == NEG) return NEG;
    return m + logf(expf(x - m) + expf(y - m) + expf(z - m));
}

// Sum / max over the wave, every lane ending with the same bits (fp add and
// max commute, so both partners of a butterfly step compute the same value).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

template <int K>
__device__ __forceinline__ void load_row(const float* lat, int S, int s0,
                                         float (&v)[K]) {
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = s0 + i < S ? lat[s0 + i] : NEG;
}

template <int K>
__device__ __forceinline__ void store_row(float* lat, int S, int s0,
                                          const float (&v)[K]) {
#pragma unroll
    for (int i = 0; i < K; ++i)
        if (s0 + i < S) lat[s0 + i] = v[i];
}

// alpha, one wave: lat[t][s] holds lp on entry and alpha_t(s) on return.
template <int K>
__device__ __forceinline__ void alpha_walk(float* lat, const int* lab, int S,
                                           int Sst, int len, int blank,
                                           int lane) {
    const int s0 = lane * K;
    bool skip[K];
    float a[K], q[PF][K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int s = s0 + i;
        skip[i] = s >= 2 && s < S && lab[s] != blank && lab[s] != lab[s - 2];
    }
    load_row<K>(lat, S, s0, a);
#pragma unroll
    for (int i = 0; i < K; ++i)
        if (s0 + i >= 2) a[i] = NEG;
    store_row<K>(lat, S, s0, a);
#pragma unroll
    for (int p = 0; p < PF; ++p) {
#pragma unroll
        for (int i = 0; i < K; ++i) q[p][i] = NEG;
        if (1 + p < len) load_row<K>(lat + (size_t)(1 + p) * Sst, S, s0, q[p]);
    }
    for (int t = 1; t < len; t += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int tt = t + p;
            if (tt < len) {  // wave-uniform
                float cur[K], na[K];
#pragma unroll
                for (int i = 0; i < K; ++i) cur[i] = q[p][i];
                if (tt + PF < len)
                    load_row<K>(lat + (size_t)(tt + PF) * Sst, S, s0, q[p]);
                float up1 = __shfl_up(a[K - 1], 1);
                float up2 = K >= 2 ? __shfl_up(a[K >= 2 ? K - 2 : 0], 1)
                                   : __shfl_up(a[0], 2);
                if (lane == 0) up1 = up2 = NEG;
                if (K == 1 && lane == 1) up2 = NEG;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const float x1 = i >= 1 ? a[i >= 1 ? i - 1 : 0] : up1;
                    const float x2 = i >= 2 ? a[i >= 2 ? i - 2 : 0]
                                            : (i == 1 ? up1 : up2);
                    na[i] = cur[i] + logadd3(a[i], x1, skip[i] ? x2 : NEG);
                }
#pragma unroll
                for (int i = 0; i < K; ++i) a[i] = na[i];
                store_row<K>(lat + (size_t)tt * Sst, S, s0, a);
            }
        }
    }
}

// beta', one wave: lat[t][s] holds lp on entry and beta'_t(s) on return.
template <int K>
__device__ __forceinline__ void beta_walk(float* lat, const int* lab, int S,
                                          int Sst, int len, int blank,
                                          int lane) {
    const int s0 = lane * K;
    bool skip[K];
    float b[K], q[PF][K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int s = s0 + i;
        skip[i] = s + 2 < S && lab[s + 2] != blank && lab[s + 2] != lab[s];
        b[i] = (s < S && s >= S - 2) ? 0.0f : NEG;
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) {
#pragma unroll
        for (int i = 0; i < K; ++i) q[p][i] = NEG;
        if (len - 1 - p >= 0)
            load_row<K>(lat + (size_t)(len - 1 - p) * Sst, S, s0, q[p]);
    }
    for (int t = len - 1; t >= 0; t -= PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int tt = t - p;
            if (tt >= 0) {  // wave-uniform
                float x[K], nb[K];
#pragma unroll
                for (int i = 0; i < K; ++i) x[i] = q[p][i] + b[i];
                if (tt - PF >= 0)
                    load_row<K>(lat + (size_t)(tt - PF) * Sst, S, s0, q[p]);
                store_row<K>(lat + (size_t)tt * Sst, S, s0, b);
                if (tt > 0) {
                    float dn1 = __shfl_down(x[0], 1);
                    float dn2 = K >= 2 ? __shfl_down(x[K >= 2 ? 1 : 0], 1)
                                       : __shfl_down(x[0], 2);
                    if (lane == WAVE - 1) dn1 = dn2 = NEG;
                    if (K == 1 && lane == WAVE - 2) dn2 = NEG;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const float y1 = i + 1 < K ? x[i + 1 < K ? i + 1 : 0] : dn1;
                        const float y2 = i + 2 < K ? x[i + 2 < K ? i + 2 : 0]
                                                   : (i + 2 == K ? dn1 : dn2);
                        nb[i] = logadd3(x[i], y1, skip[i] ? y2 : NEG);
                    }
#pragma unroll
                    for (int i = 0; i < K; ++i) b[i] = nb[i];
                }
            }
        }
    }
}

template <int K, bool LAT_LDS>
__global__ void __launch_bounds__(THREADS) ctc_loss_kernel(CtcArgs a) {
    extern __shared__ float dyn_lds[];
    __shared__ int lab[MAX_S];
    __shared__ short nxt[MAX_S];           // next odd state, same label; 0: none
    __shared__ unsigned char head[MAX_S];  // first odd state with its label
    __shared__ long long red[WAVES];

    const int n = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int T = a.T, N = a.N, C = a.C, Sst = a.Sst, blank = a.blank;
    const bool want_grad = a.grad != nullptr;

    long long len64 = load_int(a.in_len, n, a.in_len_i64);
    const int len = (int)(len64 < 0 ? 0 : (len64 > T ? T : len64));
    long long L64 = load_int(a.tgt_len, n, a.tgt_len_i64);
    if (L64 < 0) L64 = 0;

    // where this utterance's labels start
    long long base, limit;
    if (a.tgt_stride >= 0) {
        base = (long long)n * a.tgt_stride;
        limit = base + a.tgt_stride;
    } else {
        long long part = 0;
        for (int i = tid; i < n; i += THREADS) {
            const long long v = load_int(a.tgt_len, i, a.tgt_len_i64);
            part += v < 0 ? 0 : v;
        }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) part += __shfl_xor(part, m);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        base = 0;
        for (int w = 0; w < WAVES; ++w) base += red[w];
        limit = a.tgt_numel;
    }

    float* grow = want_grad ? a.grad + (size_t)n * C : nullptr;  // + t N C
    const size_t gstep = (size_t)N * C;

    if (2 * L64 + 1 > Sst) {  // block-uniform: not served, see the header
        if (tid == 0) a.nll[n] = NAN;
        if (want_grad)
            for (long long i = tid; i < (long long)T * C; i += THREADS)
                grow[(size_t)(i / C) * gstep + i % C] = 0.0f;
        return;
    }
    const int L = (int)L64, S = 2 * L + 1;

    if (tid < S) {
        int v = blank;
        if (tid & 1) {
            const long long at = base + (tid >> 1);
            v = -1;
            if (at < limit) {
                const long long c = load_int(a.targets, at, a.targets_i64);
                if (c >= 0 && c < C) v = (int)c;
            }
        }
        lab[tid] = v;
    }
    __syncthreads();
    if (want_grad && tid < S && (tid & 1)) {
        const int v = lab[tid];
        int h = 1, nx = 0;
        for (int u = 1; u < tid; u += 2) h &= lab[u] != v;
        for (int u = tid + 2; u < S; u += 2)
            if (lab[u] == v) {
                nx = u;
                break;
            }
        head[tid] = (unsigned char)h;
        nxt[tid] = (short)nx;
    }

    const size_t lat_floats = ctc_lattice_floats(T, Sst);
    float* lat = LAT_LDS ? dyn_lds : a.ws + (size_t)n * lat_floats;
    float* alpha = lat;
    float* beta = lat + (size_t)T * Sst;
    // log-softmax as (x - max) - log(sum), torch's order: the row maximum's
    // own term is exact, where x - (max + log(sum)) would round at |x|
    float* rmax = lat + (size_t)2 * T * Sst;
    float* rlog = rmax + T;
    const float* xrow = a.logits + (size_t)n * C;  // + t N C

    // ---- phase A
    for (int t = wave; t < len; t += WAVES) {
        const float* row = xrow + (size_t)t * gstep;
        float m = NEG;
        for (int c = lane; c < C; c += WAVE) m = fmaxf(m, row[c]);
        m = wave_max(m);
        float sum = 0.0f;
        for (int c = lane; c < C; c += WAVE) sum += expf(row[c] - m);
        const float l = logf(wave_sum(sum));
        if (lane == 0) {
            rmax[t] = m;
            rlog[t] = l;
        }
        for (int s = lane; s < S; s += WAVE) {
            const int c = lab[s];
            const float v = c >= 0 ? (row[c] - m) - l : NEG;
            alpha[(size_t)t * Sst + s] = v;
            if (want_grad) beta[(size_t)t * Sst + s] = v;
        }
    }
    __syncthreads();

    // ---- phase B
    if (len > 0) {
        if (wave == 0)
            alpha_walk<K>(alpha, lab, S, Sst, len, blank, lane);
        else if (wave == 1 && want_grad)
            beta_walk<K>(beta, lab, S, Sst, len, blank, lane);
    }
    __syncthreads();

    // ---- phase C
    float nll;
    if (len > 0) {
        const float* last = alpha + (size_t)(len - 1) * Sst;
        nll = -logadd3(last[S - 1], S >= 2 ? last[S - 2] : NEG, NEG);
    } else {
        nll = L == 0 ? 0.0f : INFINITY;
    }
    const bool infeasible = nll == INFINITY;
    if (tid == 0) a.nll[n] = (infeasible && a.zero_infinity) ? 0.0f : nll;
    if (!want_grad) return;

    for (long long i = tid; i < (long long)(T - len) * C; i += THREADS)
        grow[(size_t)(len + i / C) * gstep + i % C] = 0.0f;
    if (infeasible) {
        const float fill = a.zero_infinity ? 0.0f : NAN;
        for (long long i = tid; i < (long long)len * C; i += THREADS)
            grow[(size_t)(i / C) * gstep + i % C] = fill;
        return;
    }
    for (long long i = tid; i < (long long)len * C; i += THREADS) {
        const int t = (int)(i / C), c = (int)(i % C);
        grow[(size_t)t * gstep + c] =
            expf((xrow[(size_t)t * gstep + c] - rmax[t]) - rlog[t]);
    }
    __syncthreads();  // the owners below overwrite what other threads wrote
    for (int t = wave; t < len; t += WAVES) {
        const float* row = xrow + (size_t)t * gstep;
        float* g = grow + (size_t)t * gstep;
        const float* al = alpha + (size_t)t * Sst;
        const float* be = beta + (size_t)t * Sst;
        const float m = rmax[t], l = rlog[t];
        float p = 0.0f;
        for (int s = lane; s < S; s += WAVE)
            if (lab[s] == blank) p += expf(al[s] + be[s] + nll);
        p = wave_sum(p);
        if (lane == 0) g[blank] = expf((row[blank] - m) - l) - p;
        for (int s = lane; s < S; s += WAVE) {
            const int c = lab[s];
            if ((s & 1) && c >= 0 && c != blank && head[s]) {
                float o = 0.0f;
                for (int u = s; u != 0; u = nxt[u]) o += expf(al[u] + be[u] + nll);
                g[c] = expf((row[c] - m) - l) - o;
            }
        }
    }
}

__global__ void __launch_bounds__(THREADS)
ctc_scale_grad_kernel(const float* __restrict__ g, const float* __restrict__ gout,
                      float* __restrict__ out, long long total, int N, int C) {
    const long long stride = (long long)gridDim.x * THREADS;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < total;
         i += stride)
        out[i] = g[i] * gout[(i / C) % N];
}

template <int K>
void launch_k(const CtcArgs& a, bool lds, size_t bytes, hipStream_t s) {
    if (lds)
        hipLaunchKernelGGL((ctc_loss_kernel<K, true>), dim3(a.N), dim3(THREADS),
                           bytes, s, a);
    else
        hipLaunchKernelGGL((ctc_loss_kernel<K, false>), dim3(a.N), dim3(THREADS),
                           0, s, a);
}

}  // namespace

extern "C" {

// a.ws == nullptr: the lattices go to LDS, and must fit CTC_LDS_BUDGET.
void launch_ctc_loss(const CtcArgs* a, hipStream_t s) {
    const bool lds = a->ws == nullptr;
    const size_t bytes = ctc_lattice_floats(a->T, a->Sst) * sizeof(float);
    if (a->Sst <= WAVE)
        launch_k<1>(*a, lds, bytes, s);
    else if (a->Sst <= 2 * WAVE)
        launch_k<2>(*a, lds, bytes, s);
    else
        launch_k<4>(*a, lds, bytes, s);
}

void launch_ctc_scale_grad(const float* g, const float* gout, float* out,
                           long long total, int N, int C, hipStream_t s) {
    long long blocks = (total + THREADS - 1) / THREADS;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(ctc_scale_grad_kernel, dim3((unsigned)blocks),
                       dim3(THREADS), 0, s, g, gout, out, total, N, C);
}

}  // extern "C"

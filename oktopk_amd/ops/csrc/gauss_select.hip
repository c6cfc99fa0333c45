// Device-resident Gaussian-k selection (gfx950, wave64).
//
// Replaces the host-side threshold pick of the gaussiank compressors
// (torch mean/std + scipy ppf + a count_gt-per-round refine loop, reference
// VGG/compression.py:220-266 and utils.py:136-138) with four launches and
// one 48-byte readback:
//
//   moments  one streaming pass: v = (float)g + r (or t + r), r = v, and
//            per-wave (n, mean, M2) partials of v — no atomics
//   finalize one block: fixed-order fp64 merge of the <= 8192 wave partials,
//            normal quantile, tau0 and the 10-entry candidate table
//   count    one read of r: |v| > cand[j] for all 10 candidates, thresholds
//            read from DEVICE memory, compact count layout [cand][block][wave]
//   decide   per-candidate totals + the 3-round refine tree in integers
//
// The compact write pass (kernels.hip) then runs on the chosen row.
//
// Numerics: a plain fp64 sum of x^2 loses ~(mean/std)^2 ulps when
// |mean| >> std, so each lane accumulates sum(x-p) and sum((x-p)^2) around
// a per-wave pivot p (the wave's first element), converts to (n, mean, M2)
// and every merge above the lane uses Chan's pairwise update.  Every merge
// order is fixed by the launch geometry alone, so tau is bitwise
// reproducible run to run.

#include <hip/hip_runtime.h>
#include <cstdint>

#define GS_BLOCK 256
#define GS_WAVES (GS_BLOCK / 64)
#define GS_NCAND 10
#define GS_FIN_THREADS 1024
#define GS_FIN_PER 8  // 1024 x 8 = 8192 wave partials max

typedef __attribute__((ext_vector_type(8))) short gs_bf16x8_t;

__device__ __forceinline__ float gs_b2f(short u) {
    return __uint_as_float(((uint32_t)(uint16_t)u) << 16);
}

__device__ __forceinline__ uint32_t gs_abs_bits(float x) {
    return __float_as_uint(x) & 0x7fffffffu;
}

// same comparison as kernels.hip sel_gt (strict >, NaN bit patterns sort
// above every finite threshold) so these counts match compact_write_kernel
__device__ __forceinline__ int gs_sel_gt(uint32_t abits, uint32_t tau_bits) {
    return (tau_bits == 0xFFFFFFFFu) | (abits > tau_bits);
}

// Chan et al. pairwise merge of (n, mean, M2): a <- a (+) b
__device__ __forceinline__ void gs_merge(double& na, double& ma, double& qa,
                                         double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb; ma = mb; qa = qb;
        return;
    }
    double nn = na + nb;
    double d = mb - ma;
    double w = nb / nn;
    ma = ma + d * w;
    qa = qa + qb + d * d * na * w;
    na = nn;
}

// ---------------------------------------------------------------------------
// pass A: EF restore (+bf16 upcast) + per-wave moments.  Same grid and wave
// subchunks as ef_count_kernel; VEC=false is the scalar-load variant for
// buffers that are not 16-byte aligned.
// ---------------------------------------------------------------------------
template <bool HAS_G, bool VEC>
__global__ void gauss_moments_kernel(const float* __restrict__ t,
                                     float* __restrict__ r,
                                     const short* __restrict__ g, int64_t n,
                                     int64_t chunk,
                                     double* __restrict__ partials) {
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t sub = chunk / GS_WAVES;  // multiple of 512
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > n) start = n;
    if (end > n) end = n;

    // pivot: this wave's first restored element (read before any lane of
    // the wave overwrites r[start]); non-finite pivots would poison every
    // difference, so they fall back to 0
    double p = 0.0;
    if (start < end) {
        float pv = (HAS_G ? gs_b2f(g[start]) : t[start]) + r[start];
        if (gs_abs_bits(pv) < 0x7f800000u) p = (double)pv;
    }
    double s1 = 0.0, s2 = 0.0;
    int cnt = 0;

    // lane `lane` owns the 8-element runs lane, lane+64, ... of the
    // subchunk in BOTH variants, so the scalar variant adds the same values
    // in the same order and returns bit-identical moments
    int64_t vend = start + ((end - start) & ~7LL);
    int64_t ng = (vend - start) >> 3;
    for (int64_t i = lane; i < ng; i += 64) {
        float v[8];
        if (VEC) {
            const float4* t4 = reinterpret_cast<const float4*>(t + start);
            float4* r4 = reinterpret_cast<float4*>(r + start);
            const gs_bf16x8_t* g8 =
                reinterpret_cast<const gs_bf16x8_t*>(g + start);
            float4 ra = r4[2 * i], rb = r4[2 * i + 1];
            float4 ta, tb;
            if (HAS_G) {
                gs_bf16x8_t gv = g8[i];
                ta.x = gs_b2f(gv[0]) + ra.x;
                ta.y = gs_b2f(gv[1]) + ra.y;
                ta.z = gs_b2f(gv[2]) + ra.z;
                ta.w = gs_b2f(gv[3]) + ra.w;
                tb.x = gs_b2f(gv[4]) + rb.x;
                tb.y = gs_b2f(gv[5]) + rb.y;
                tb.z = gs_b2f(gv[6]) + rb.z;
                tb.w = gs_b2f(gv[7]) + rb.w;
            } else {
                float4 ua = t4[2 * i], ub = t4[2 * i + 1];
                ta.x = ua.x + ra.x; ta.y = ua.y + ra.y;
                ta.z = ua.z + ra.z; ta.w = ua.w + ra.w;
                tb.x = ub.x + rb.x; tb.y = ub.y + rb.y;
                tb.z = ub.z + rb.z; tb.w = ub.w + rb.w;
            }
            // only the snapshot is written (compact_adaptive_ef contract):
            // t stays untouched, the write pass compacts from r
            r4[2 * i] = ta; r4[2 * i + 1] = tb;
            v[0] = ta.x; v[1] = ta.y; v[2] = ta.z; v[3] = ta.w;
            v[4] = tb.x; v[5] = tb.y; v[6] = tb.z; v[7] = tb.w;
        } else {
            int64_t base = start + 8 * i;
            #pragma unroll
            for (int j = 0; j < 8; ++j)
                v[j] = (HAS_G ? gs_b2f(g[base + j]) : t[base + j]) + r[base + j];
            #pragma unroll
            for (int j = 0; j < 8; ++j) r[base + j] = v[j];
        }
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            double d = (double)v[j] - p;
            s1 += d;
            s2 = fma(d, d, s2);
        }
        cnt += 8;
    }
    for (int64_t i = vend + lane; i < end; i += 64) {
        float v = (HAS_G ? gs_b2f(g[i]) : t[i]) + r[i];
        r[i] = v;
        double d = (double)v - p;
        s1 += d;
        s2 = fma(d, d, s2);
        cnt += 1;
    }

    // lane sums around the pivot -> (n, mean, M2)
    double na = (double)cnt, ma = 0.0, qa = 0.0;
    if (cnt > 0) {
        ma = p + s1 / na;
        qa = s2 - s1 * s1 / na;
        if (qa < 0.0) qa = 0.0;  // NaN stays NaN
    }
    for (int off = 32; off > 0; off >>= 1) {
        double nb = __shfl_down(na, off, 64);
        double mb = __shfl_down(ma, off, 64);
        double qb = __shfl_down(qa, off, 64);
        gs_merge(na, ma, qa, nb, mb, qb);
    }
    if (lane == 0) {
        int64_t w = (int64_t)blockIdx.x * GS_WAVES + wave;
        partials[3 * w + 0] = na;
        partials[3 * w + 1] = ma;
        partials[3 * w + 2] = qa;
    }
}

// ---------------------------------------------------------------------------
// upper-tail standard normal quantile: z with Q(z) = q, 0 < q <= 0.5.
// Rational approximations and coefficients of the Cephes Math Library's
// ndtri (S. L. Moshier; relative error ~1e-15 over the whole range).
// ---------------------------------------------------------------------------
__device__ double gs_polevl(double x, const double* c, int n) {
    double a = c[0];
    for (int i = 1; i <= n; ++i) a = a * x + c[i];
    return a;
}

__device__ double gs_ndtri_upper(double q) {
    // |q - 0.5| <= 3/8 region (q > exp(-2))
    const double P0[5] = {
        -5.99633501014107895267E1, 9.80010754185999661536E1,
        -5.66762857469070293439E1, 1.39312609387279679503E1,
        -1.23916583867381258016E0};
    const double Q0[9] = {
        1.00000000000000000000E0, 1.95448858338141759834E0,
        4.67627912898881538453E0, 8.63602421390890590575E1,
        -2.25462687854119370527E2, 2.00260212380060660359E2,
        -8.20372256168333339912E1, 1.59056225126211695515E1,
        -1.18331621121330003142E0};
    // x = sqrt(-2 log q) in [2, 8)
    const double P1[9] = {
        4.05544892305962419923E0, 3.15251094599893866154E1,
        5.71628192246421288162E1, 4.40805073893200834700E1,
        1.46849561928858024014E1, 2.18663306850790267539E0,
        -1.40256079171354495875E-1, -3.50424626827848203418E-2,
        -8.57456785154685413611E-4};
    const double Q1[9] = {
        1.00000000000000000000E0, 1.57799883256466749731E1,
        4.53907635128879210584E1, 4.13172038254672030440E1,
        1.50425385692907503408E1, 2.50464946208309415979E0,
        -1.42182922854787788574E-1, -3.80806407691578277194E-2,
        -9.33259480895457427372E-4};
    // x in [8, 64)
    const double P2[9] = {
        3.23774891776946035970E0, 6.91522889068984211695E0,
        3.93881025292474443415E0, 1.33303460815807542389E0,
        2.01485389549179081538E-1, 1.23716634817820021358E-2,
        3.01581553508235416007E-4, 2.65806974686737550832E-6,
        6.23974539184983293730E-9};
    const double Q2[9] = {
        1.00000000000000000000E0, 6.02427039364742014255E0,
        3.67983563856160859403E0, 1.37702099489081330271E0,
        2.16236993594496635890E-1, 1.34204006088543189037E-2,
        3.28014464682127739104E-4, 2.89247864745380683936E-6,
        6.79019408009981274425E-9};
    const double s2pi = 2.50662827463100050242E0;
    if (q > 0.13533528323661269189) {  // exp(-2)
        double y = q - 0.5;            // <= 0: the lower-tail quantile
        double y2 = y * y;
        double x = y + y * (y2 * gs_polevl(y2, P0, 4) / gs_polevl(y2, Q0, 8));
        return -(x * s2pi);
    }
    double x = sqrt(-2.0 * log(q));
    double x0 = x - log(x) / x;
    double z = 1.0 / x;
    double x1 = x < 8.0 ? z * gs_polevl(z, P1, 8) / gs_polevl(z, Q1, 8)
                        : z * gs_polevl(z, P2, 8) / gs_polevl(z, Q2, 8);
    return x0 - x1;
}

// record layout (6 doubles, the only host readback):
//   [0] chosen candidate  [1] count at chosen  [2] tau  [3] tau0
//   [4] mean  [5] std
__global__ void gauss_finalize_kernel(const double* __restrict__ partials,
                                      int nw, int64_t n, double q,
                                      float* __restrict__ cand,
                                      double* __restrict__ rec) {
    __shared__ double sn[GS_FIN_THREADS], sm[GS_FIN_THREADS], sq[GS_FIN_THREADS];
    int tid = threadIdx.x;
    double na = 0.0, ma = 0.0, qa = 0.0;
    #pragma unroll
    for (int j = 0; j < GS_FIN_PER; ++j) {
        int i = tid * GS_FIN_PER + j;
        if (i < nw)
            gs_merge(na, ma, qa, partials[3 * i], partials[3 * i + 1],
                     partials[3 * i + 2]);
    }
    sn[tid] = na; sm[tid] = ma; sq[tid] = qa;
    __syncthreads();
    for (int o = GS_FIN_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            gs_merge(na, ma, qa, sn[tid + o], sm[tid + o], sq[tid + o]);
            sn[tid] = na; sm[tid] = ma; sq[tid] = qa;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double mean = ma;
        double sd = n > 1 ? sqrt(qa / (double)(n - 1)) : 0.0;
        double tau0d;
        // degenerate (n < 2, constant or non-finite input): |mean| selects
        // nothing strictly above it, as the host _gaussian_threshold does
        if (n < 2 || !(sd > 0.0) || isinf(sd))
            tau0d = fabs(mean);
        else
            tau0d = fabs(mean + sd * gs_ndtri_upper(q));
        float tau0 = (float)tau0d;
        // every threshold the three-round refine loop can visit, level by
        // level: 0.5^(l-h) * 1.5^h at index l(l+1)/2 + h.  All factors are
        // exact in binary: one rounding per candidate.
        const double F[GS_NCAND] = {1.0,  0.5,   1.5,   0.25,  0.75,
                                    2.25, 0.125, 0.375, 1.125, 3.375};
        #pragma unroll
        for (int j = 0; j < GS_NCAND; ++j) cand[j] = (float)((double)tau0 * F[j]);
        rec[3] = (double)tau0;
        rec[4] = mean;
        rec[5] = sd;
    }
}

// ---------------------------------------------------------------------------
// pass B: one read of the restored snapshot counts all 10 candidates.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ void gauss_count_kernel(const float* __restrict__ r, int64_t n,
                                   const float* __restrict__ cand,
                                   int64_t chunk, int* __restrict__ wave_counts,
                                   int nblocks) {
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t sub = chunk / GS_WAVES;
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > n) start = n;
    if (end > n) end = n;
    uint32_t tb[GS_NCAND];
    int cnt[GS_NCAND];
    #pragma unroll
    for (int c = 0; c < GS_NCAND; ++c) {
        tb[c] = __float_as_uint(cand[c]) & 0x7fffffffu;  // cand >= 0 or NaN
        cnt[c] = 0;
    }
    int64_t vend = VEC ? start + ((end - start) & ~7LL) : start;
    if (VEC) {
        const float4* r4 = reinterpret_cast<const float4*>(r + start);
        int64_t ng = (vend - start) >> 3;
        for (int64_t i = lane; i < ng; i += 64) {
            float4 xa = r4[2 * i], xb = r4[2 * i + 1];
            uint32_t a[8] = {gs_abs_bits(xa.x), gs_abs_bits(xa.y),
                             gs_abs_bits(xa.z), gs_abs_bits(xa.w),
                             gs_abs_bits(xb.x), gs_abs_bits(xb.y),
                             gs_abs_bits(xb.z), gs_abs_bits(xb.w)};
            #pragma unroll
            for (int c = 0; c < GS_NCAND; ++c) {
                int s = 0;
                #pragma unroll
                for (int j = 0; j < 8; ++j) s += gs_sel_gt(a[j], tb[c]);
                cnt[c] += s;
            }
        }
    }
    for (int64_t i = vend + lane; i < end; i += 64) {
        uint32_t a = gs_abs_bits(r[i]);
        #pragma unroll
        for (int c = 0; c < GS_NCAND; ++c) cnt[c] += gs_sel_gt(a, tb[c]);
    }
    #pragma unroll
    for (int c = 0; c < GS_NCAND; ++c) {
        int v = cnt[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0)
            wave_counts[((int64_t)c * nblocks + blockIdx.x) * GS_WAVES + wave] = v;
    }
}

// ---------------------------------------------------------------------------
// decide: wave c totals candidate row c; thread 0 then walks the refine
// tree (3*cnt < 2k -> low child, 3*cnt > 4k -> high child, else stop; at
// most three counted rounds, the value reached after the third move is not
// re-tested — compression.py:236-255 in integers).
// ---------------------------------------------------------------------------
__global__ void gauss_decide_kernel(const int* __restrict__ wave_counts, int nw,
                                    int64_t k, const float* __restrict__ cand,
                                    double* __restrict__ rec) {
    __shared__ long long tot[GS_NCAND];
    int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long s = 0;
    for (int b = lane; b < nw; b += 64) s += wave_counts[(int64_t)c * nw + b];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) tot[c] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int l = 0, h = 0;
        for (int round = 0; round < 3; ++round) {
            long long cnt = tot[l * (l + 1) / 2 + h];
            if (3 * cnt < 2 * k) {
                ++l;
            } else if (3 * cnt > 4 * k) {
                ++l;
                ++h;
            } else {
                break;
            }
        }
        int j = l * (l + 1) / 2 + h;
        rec[0] = (double)j;
        rec[1] = (double)tot[j];
        rec[2] = (double)cand[j];
    }
}

extern "C" void launch_gauss_moments(const float* t, float* r, const void* g,
                                     int64_t n, int64_t chunk, int nblocks,
                                     double* partials, hipStream_t stream) {
    bool vec = ((((uintptr_t)t | (uintptr_t)r | (uintptr_t)g) & 15) == 0);
    const short* gs = (const short*)g;
#define GS_LAUNCH_A(HG, V)                                                    \
    hipLaunchKernelGGL((gauss_moments_kernel<HG, V>), dim3(nblocks),           \
                       dim3(GS_BLOCK), 0, stream, t, r, gs, n, chunk, partials)
    if (g != nullptr) {
        if (vec) GS_LAUNCH_A(true, true); else GS_LAUNCH_A(true, false);
    } else {
        if (vec) GS_LAUNCH_A(false, true); else GS_LAUNCH_A(false, false);
    }
#undef GS_LAUNCH_A
}

extern "C" void launch_gauss_finalize(const double* partials, int nw, int64_t n,
                                      double q, float* cand, double* rec,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(gauss_finalize_kernel, dim3(1), dim3(GS_FIN_THREADS), 0,
                       stream, partials, nw, n, q, cand, rec);
}

extern "C" void launch_gauss_count(const float* r, int64_t n, const float* cand,
                                   int64_t chunk, int nblocks, int* wave_counts,
                                   hipStream_t stream) {
    if (((uintptr_t)r & 15) == 0)
        hipLaunchKernelGGL((gauss_count_kernel<true>), dim3(nblocks),
                           dim3(GS_BLOCK), 0, stream, r, n, cand, chunk,
                           wave_counts, nblocks);
    else
        hipLaunchKernelGGL((gauss_count_kernel<false>), dim3(nblocks),
                           dim3(GS_BLOCK), 0, stream, r, n, cand, chunk,
                           wave_counts, nblocks);
}

extern "C" void launch_gauss_decide(const int* wave_counts, int nw, int64_t k,
                                    const float* cand, double* rec,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(gauss_decide_kernel, dim3(1), dim3(GS_NCAND * 64), 0,
                       stream, wave_counts, nw, k, cand, rec);
}

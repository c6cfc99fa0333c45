// Exact top-k selection and sparse top-k merge (gfx950, wave64).
//
// Replaces the torch.topk call-sites of the exact-top-k compressors
// (compress_org, reference VGG/compression.py:37-62, and the gTopK tree
// merge, VGG/allreducer.py:116-150) with a device-resident exact-k select:
//
//   hist x3  3-level radix histogram of the 32-bit key (11 + 11 + 10 bits);
//            level 1 is fused with the EF restore (+ bf16 upcast), later
//            levels read the restored snapshot and count only the keys
//            under the prefix chosen so far
//   pick x3  one block after each level: suffix-scan the bins from the top,
//            pick the bin holding the k-th key, update {prefix, remaining}
//            in DEVICE memory and clear the bins for the next level.  After
//            level 3 the prefix is tau and remaining is `need`: how many of
//            the keys equal to tau belong to the selection
//   count    per-wave (gt, eq) counts over contiguous wave sub-chunks (the
//            compact_count_multi_kernel layout, kernels.hip)
//   scan     exclusive scans of both rows (scan_offsets_kernel, kernels.hip)
//   write    position of a selected element = gt_before + min(eq_before,
//            need); a tie is selected iff eq_before < need.  Both are
//            monotone in the index, so the output is ascending with no
//            atomics and no sort; the same pass zeroes the residual there
//
// Nothing is read back until the selection is written: every launch takes
// tau/need from the 16-byte state record, and the output size is min(k, n)
// by definition.  All counting is in integers, so the result is bitwise
// reproducible.
//
// Keys.  SRC_F32: key = |x| bit pattern (nonnegative floats order as
// integers; NaN patterns sort above inf, as abs_bits does elsewhere).
// SRC_KEY: the array holds ready-made keys — sparse_merge_topk lays the two
// lists out in merged "slot" order, gives a live slot abs_bits(v) + 1 and
// the dead twin of a duplicated index 0, and runs the same select over the
// slots, so a dead slot can never outrank a live one.

#include <hip/hip_runtime.h>
#include <cstdint>

#define TK_BLOCK 256
#define TK_WAVES (TK_BLOCK / 64)
#define TK_VEC 8
#define TK_MAX_BINS 2048
#define TK_HIST_BLOCKS 1024
#define TK_PICK_THREADS 1024

enum { SRC_F32 = 0, SRC_KEY = 1 };

// state record (uint32[4]): [0] prefix value, [1] prefix mask,
// [2] remaining rank inside the prefix class, [3] unused
typedef __attribute__((ext_vector_type(8))) short tk_bf16x8_t;

__device__ __forceinline__ float tk_b2f(short u) {
    return __uint_as_float(((uint32_t)(uint16_t)u) << 16);
}

template <int SRC>
__device__ __forceinline__ uint32_t tk_key(uint32_t w) {
    return SRC == SRC_F32 ? (w & 0x7fffffffu) : w;
}

__device__ __forceinline__ void tk_hist_flush(const unsigned int* lhist,
                                              int nbins,
                                              unsigned int* __restrict__ ghist) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += TK_BLOCK)
        if (lhist[b]) atomicAdd(&ghist[b], lhist[b]);
}

// ---------------------------------------------------------------------------
// level 1, fused with the EF restore: v = (float)g + r (or t + r), r = v,
// bin = |v| bits >> 21.  Grid-stride over 8-element groups; n8 = 0 is the
// scalar variant for buffers that are not 16-byte aligned.
// ---------------------------------------------------------------------------
template <bool HAS_G>
__global__ void tk_ef_hist_kernel(const float* __restrict__ t,
                                  float* __restrict__ r,
                                  const short* __restrict__ g, int64_t n,
                                  int64_t n8, unsigned int* __restrict__ ghist) {
    __shared__ unsigned int lhist[TK_MAX_BINS];
    for (int b = threadIdx.x; b < TK_MAX_BINS; b += TK_BLOCK) lhist[b] = 0;
    __syncthreads();
    const float4* t4 = reinterpret_cast<const float4*>(t);
    float4* r4 = reinterpret_cast<float4*>(r);
    const tk_bf16x8_t* g8 = reinterpret_cast<const tk_bf16x8_t*>(g);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * TK_BLOCK;
    for (; i < n8; i += stride) {
        float4 ra = r4[2 * i], rb = r4[2 * i + 1];
        float4 ta, tb;
        if (HAS_G) {
            tk_bf16x8_t gv = g8[i];
            ta.x = tk_b2f(gv[0]) + ra.x; ta.y = tk_b2f(gv[1]) + ra.y;
            ta.z = tk_b2f(gv[2]) + ra.z; ta.w = tk_b2f(gv[3]) + ra.w;
            tb.x = tk_b2f(gv[4]) + rb.x; tb.y = tk_b2f(gv[5]) + rb.y;
            tb.z = tk_b2f(gv[6]) + rb.z; tb.w = tk_b2f(gv[7]) + rb.w;
        } else {
            float4 ua = t4[2 * i], ub = t4[2 * i + 1];
            ta.x = ua.x + ra.x; ta.y = ua.y + ra.y;
            ta.z = ua.z + ra.z; ta.w = ua.w + ra.w;
            tb.x = ub.x + rb.x; tb.y = ub.y + rb.y;
            tb.z = ub.z + rb.z; tb.w = ub.w + rb.w;
        }
        // only the snapshot is written: t stays untouched, every later
        // pass reads r
        r4[2 * i] = ta; r4[2 * i + 1] = tb;
        const float v[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            atomicAdd(&lhist[(__float_as_uint(v[j]) & 0x7fffffffu) >> 21], 1u);
    }
    for (i = n8 * 8 + (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x; i < n;
         i += stride) {
        float v = (HAS_G ? tk_b2f(g[i]) : t[i]) + r[i];
        r[i] = v;
        atomicAdd(&lhist[(__float_as_uint(v) & 0x7fffffffu) >> 21], 1u);
    }
    tk_hist_flush(lhist, TK_MAX_BINS, ghist);
}

// ---------------------------------------------------------------------------
// generic level: histogram of (key >> shift) & (nbins - 1) over the keys
// whose bits under the state's prefix mask equal its prefix value.  `first`
// (level 1 of the unfused callers) has no prefix and does not read state.
// ---------------------------------------------------------------------------
template <int SRC>
__global__ void tk_hist_kernel(const uint32_t* __restrict__ w, int64_t n,
                               int64_t n8, const uint32_t* __restrict__ state,
                               int first, int shift, int nbins,
                               unsigned int* __restrict__ ghist) {
    __shared__ unsigned int lhist[TK_MAX_BINS];
    for (int b = threadIdx.x; b < nbins; b += TK_BLOCK) lhist[b] = 0;
    __syncthreads();
    const uint32_t pval = first ? 0u : state[0];
    const uint32_t pmask = first ? 0u : state[1];
    const uint32_t bmask = (uint32_t)nbins - 1u;
    const uint4* w4 = reinterpret_cast<const uint4*>(w);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * TK_BLOCK;
    for (; i < n8; i += stride) {
        uint4 a = w4[2 * i], b = w4[2 * i + 1];
        const uint32_t u[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t key = tk_key<SRC>(u[j]);
            if ((key & pmask) == pval)
                atomicAdd(&lhist[(key >> shift) & bmask], 1u);
        }
    }
    for (i = n8 * 8 + (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x; i < n;
         i += stride) {
        uint32_t key = tk_key<SRC>(w[i]);
        if ((key & pmask) == pval)
            atomicAdd(&lhist[(key >> shift) & bmask], 1u);
    }
    tk_hist_flush(lhist, nbins, ghist);
}

// ---------------------------------------------------------------------------
// pick: one block.  Thread i owns bins nbins-1-2i and nbins-2-2i, so an
// inclusive scan over the threads is the count of keys in the bins above.
// The bin b with above(b) < remaining <= above(b) + hist[b] holds the
// wanted key; remaining becomes its rank inside b.  The total over the bins
// is never below `remaining` (level 1 counts all n >= k keys, a later level
// counts exactly the bin chosen before), so exactly one thread matches.
// ---------------------------------------------------------------------------
__global__ void tk_pick_kernel(unsigned int* __restrict__ hist, int nbins,
                               int shift, uint32_t* __restrict__ state,
                               uint32_t k_init, int first) {
    __shared__ uint32_t sh[TK_PICK_THREADS];
    const int tid = threadIdx.x;
    const uint32_t pval = first ? 0u : state[0];
    const uint32_t pmask = first ? 0u : state[1];
    const uint32_t remaining = first ? k_init : state[2];
    const int b0 = nbins - 1 - 2 * tid, b1 = b0 - 1;
    const uint32_t h0 = b0 >= 0 ? hist[b0] : 0u;
    const uint32_t h1 = b1 >= 0 ? hist[b1] : 0u;
    sh[tid] = h0 + h1;
    __syncthreads();
    for (int d = 1; d < TK_PICK_THREADS; d <<= 1) {  // Hillis-Steele
        uint32_t v = tid >= d ? sh[tid - d] : 0u;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    const uint32_t above0 = tid == 0 ? 0u : sh[tid - 1];
    const uint32_t above1 = above0 + h0;
    int b = -1;
    uint32_t rem = 0;
    if (h0 && above0 < remaining && remaining <= above0 + h0) {
        b = b0;
        rem = remaining - above0;
    } else if (h1 && above1 < remaining && remaining <= above1 + h1) {
        b = b1;
        rem = remaining - above1;
    }
    if (b >= 0) {
        state[0] = pval | ((uint32_t)b << shift);
        state[1] = pmask | (((uint32_t)nbins - 1u) << shift);
        state[2] = rem;
        state[3] = 0u;
    }
    if (b0 >= 0) hist[b0] = 0u;
    if (b1 >= 0) hist[b1] = 0u;
}

// eight keys of lane `lane`'s run at `my`; words past `end` read as key 0
// with ok = false.  `full` (wave-uniform) takes the two 16-byte loads.
template <int SRC>
__device__ __forceinline__ void tk_load8(const uint32_t* __restrict__ w,
                                         int64_t my, int64_t end, bool full,
                                         uint32_t (&u)[TK_VEC],
                                         bool (&ok)[TK_VEC]) {
    if (full) {
        const uint4* p = reinterpret_cast<const uint4*>(w + my);
        uint4 a = p[0], b = p[1];
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
        u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
        #pragma unroll
        for (int j = 0; j < TK_VEC; ++j) ok[j] = true;
    } else {
        #pragma unroll
        for (int j = 0; j < TK_VEC; ++j) {
            ok[j] = my + j < end;
            u[j] = ok[j] ? w[my + j] : 0u;
        }
    }
}

// ---------------------------------------------------------------------------
// count: per-wave (gt, eq) against tau = state[0].  Layout [2][block][wave].
// ---------------------------------------------------------------------------
template <int SRC>
__global__ void tk_count_kernel(const uint32_t* __restrict__ w, int64_t n,
                                int64_t chunk, int vec,
                                const uint32_t* __restrict__ state,
                                int* __restrict__ wave_counts, int nblocks) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sub = chunk / TK_WAVES;  // multiple of 512
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > n) start = n;
    if (end > n) end = n;
    const uint32_t tau = state[0];
    const int64_t step = 64 * TK_VEC;
    int gt = 0, eq = 0;
    for (int64_t base = start; base < end; base += step) {
        uint32_t u[TK_VEC];
        bool ok[TK_VEC];
        tk_load8<SRC>(w, base + (int64_t)lane * TK_VEC, end,
                      vec && base + step <= end, u, ok);
        #pragma unroll
        for (int j = 0; j < TK_VEC; ++j) {
            uint32_t key = tk_key<SRC>(u[j]);
            gt += ok[j] && key > tau;
            eq += ok[j] && key == tau;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        gt += __shfl_down(gt, off, 64);
        eq += __shfl_down(eq, off, 64);
    }
    if (lane == 0) {
        const int64_t nw = (int64_t)nblocks * TK_WAVES;
        const int64_t wi = (int64_t)blockIdx.x * TK_WAVES + wave;
        wave_counts[wi] = gt;
        wave_counts[nw + wi] = eq;
    }
}

// ---------------------------------------------------------------------------
// write: wave-autonomous, ascending by construction.  SRC_F32 emits (index,
// value) of the array itself and, with `zdst`, stores +0.0 there; SRC_KEY
// emits the slot's (uidx, uval).  `kout` bounds every store.
// ---------------------------------------------------------------------------
template <int SRC>
__global__ void tk_write_kernel(const uint32_t* __restrict__ w,
                                float* __restrict__ zdst, int64_t n,
                                int64_t chunk, int vec,
                                const uint32_t* __restrict__ state,
                                const int* __restrict__ offs_gt,
                                const int* __restrict__ offs_eq,
                                const int32_t* __restrict__ uidx,
                                const float* __restrict__ uval,
                                int32_t* __restrict__ out_idx,
                                float* __restrict__ out_val, int kout) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sub = chunk / TK_WAVES;
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > n) start = n;
    if (end > n) end = n;
    const uint32_t tau = state[0];
    const int need = (int)state[2];
    const uint64_t lt_mask = ((uint64_t)1 << lane) - 1;
    int gt_run = offs_gt[blockIdx.x * TK_WAVES + wave];
    int eq_run = offs_eq[blockIdx.x * TK_WAVES + wave];
    const int64_t step = 64 * TK_VEC;
    for (int64_t base = start; base < end; base += step) {
        const int64_t my = base + (int64_t)lane * TK_VEC;
        uint32_t u[TK_VEC];
        bool ok[TK_VEC];
        tk_load8<SRC>(w, my, end, vec && base + step <= end, u, ok);
        bool g[TK_VEC], e[TK_VEC];
        int gpre = 0, epre = 0, gtot = 0, etot = 0;
        #pragma unroll
        for (int j = 0; j < TK_VEC; ++j) {
            uint32_t key = tk_key<SRC>(u[j]);
            g[j] = ok[j] && key > tau;
            e[j] = ok[j] && key == tau;
            uint64_t bg = __ballot(g[j]), be = __ballot(e[j]);
            gpre += __popcll(bg & lt_mask);
            epre += __popcll(be & lt_mask);
            gtot += __popcll(bg);
            etot += __popcll(be);
        }
        // selected elements are rare: skip the store phase on iterations
        // that hold none (wave-uniform branch)
        if (gtot || (etot && eq_run < need)) {
            int gr = gt_run + gpre, er = eq_run + epre;
            #pragma unroll
            for (int j = 0; j < TK_VEC; ++j) {
                const bool take = g[j] || (e[j] && er < need);
                if (take) {
                    const int pos = gr + (er < need ? er : need);
                    if (pos < kout) {
                        if (SRC == SRC_F32) {
                            out_idx[pos] = (int32_t)(my + j);
                            out_val[pos] = __uint_as_float(u[j]);
                            if (zdst) zdst[my + j] = 0.f;
                        } else {
                            out_idx[pos] = uidx[my + j];
                            out_val[pos] = uval[my + j];
                        }
                    }
                }
                gr += g[j];
                er += e[j];
            }
        }
        gt_run += gtot;
        eq_run += etot;
    }
}

// ---------------------------------------------------------------------------
// sparse merge, slot layout.  a[i] sits at slot i + |{b < a[i]}|, b[j] at
// j + |{a <= b[j]}|: the merged order, an index held by both taking two
// adjacent slots.  The a slot carries a_val + b_val; the b twin is dead
// (key 0).  Live key = |v| bits + 1.  ndup counts the dead slots.
// ---------------------------------------------------------------------------
__global__ void tk_merge_slots_kernel(const int32_t* __restrict__ a_idx,
                                      const float* __restrict__ a_val, int na,
                                      const int32_t* __restrict__ b_idx,
                                      const float* __restrict__ b_val, int nb,
                                      uint32_t* __restrict__ ukey,
                                      int32_t* __restrict__ uidx,
                                      float* __restrict__ uval,
                                      int* __restrict__ ndup) {
    const int total = na + nb;
    int i = blockIdx.x * TK_BLOCK + threadIdx.x;
    const int stride = gridDim.x * TK_BLOCK;
    int dups = 0;
    for (; i < total; i += stride) {
        if (i < na) {
            const int32_t x = a_idx[i];
            int lo = 0, hi = nb;  // first b >= x
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (b_idx[mid] < x) lo = mid + 1; else hi = mid;
            }
            float v = a_val[i];
            if (lo < nb && b_idx[lo] == x) v = v + b_val[lo];
            const int s = i + lo;
            ukey[s] = (__float_as_uint(v) & 0x7fffffffu) + 1u;
            uidx[s] = x;
            uval[s] = v;
        } else {
            const int j = i - na;
            const int32_t x = b_idx[j];
            int lo = 0, hi = na;  // first a > x
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (a_idx[mid] <= x) lo = mid + 1; else hi = mid;
            }
            const bool dup = lo > 0 && a_idx[lo - 1] == x;
            const float v = b_val[j];
            const int s = j + lo;
            ukey[s] = dup ? 0u : (__float_as_uint(v) & 0x7fffffffu) + 1u;
            uidx[s] = x;
            uval[s] = v;
            dups += dup;
        }
    }
    for (int off = 32; off > 0; off >>= 1) dups += __shfl_down(dups, off, 64);
    if ((threadIdx.x & 63) == 0 && dups) atomicAdd(ndup, dups);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static inline int tk_hist_blocks(int64_t n) {
    int64_t b = (n + (int64_t)TK_BLOCK * TK_VEC - 1) / ((int64_t)TK_BLOCK * TK_VEC);
    if (b < 1) b = 1;
    if (b > TK_HIST_BLOCKS) b = TK_HIST_BLOCKS;
    return (int)b;
}

extern "C" void launch_tk_ef_hist(const float* t, float* r, const void* g,
                                  int64_t n, unsigned int* hist,
                                  hipStream_t stream) {
    bool vec = ((((uintptr_t)t | (uintptr_t)r | (uintptr_t)g) & 15) == 0);
    int64_t n8 = vec ? n / 8 : 0;
    if (g != nullptr)
        hipLaunchKernelGGL((tk_ef_hist_kernel<true>), dim3(tk_hist_blocks(n)),
                           dim3(TK_BLOCK), 0, stream, t, r, (const short*)g, n,
                           n8, hist);
    else
        hipLaunchKernelGGL((tk_ef_hist_kernel<false>), dim3(tk_hist_blocks(n)),
                           dim3(TK_BLOCK), 0, stream, t, r, (const short*)nullptr,
                           n, n8, hist);
}

extern "C" void launch_tk_hist(const void* words, int64_t n, int keymode,
                               const uint32_t* state, int first, int shift,
                               int nbins, unsigned int* hist,
                               hipStream_t stream) {
    const uint32_t* w = (const uint32_t*)words;
    int64_t n8 = ((uintptr_t)w & 15) == 0 ? n / 8 : 0;
    if (keymode)
        hipLaunchKernelGGL((tk_hist_kernel<SRC_KEY>), dim3(tk_hist_blocks(n)),
                           dim3(TK_BLOCK), 0, stream, w, n, n8, state, first,
                           shift, nbins, hist);
    else
        hipLaunchKernelGGL((tk_hist_kernel<SRC_F32>), dim3(tk_hist_blocks(n)),
                           dim3(TK_BLOCK), 0, stream, w, n, n8, state, first,
                           shift, nbins, hist);
}

extern "C" void launch_tk_pick(unsigned int* hist, int nbins, int shift,
                               uint32_t* state, uint32_t k_init, int first,
                               hipStream_t stream) {
    hipLaunchKernelGGL(tk_pick_kernel, dim3(1), dim3(TK_PICK_THREADS), 0, stream,
                       hist, nbins, shift, state, k_init, first);
}

extern "C" void launch_tk_count(const void* words, int64_t n, int keymode,
                                int64_t chunk, int nblocks,
                                const uint32_t* state, int* wave_counts,
                                hipStream_t stream) {
    const uint32_t* w = (const uint32_t*)words;
    int vec = ((uintptr_t)w & 15) == 0;
    if (keymode)
        hipLaunchKernelGGL((tk_count_kernel<SRC_KEY>), dim3(nblocks),
                           dim3(TK_BLOCK), 0, stream, w, n, chunk, vec, state,
                           wave_counts, nblocks);
    else
        hipLaunchKernelGGL((tk_count_kernel<SRC_F32>), dim3(nblocks),
                           dim3(TK_BLOCK), 0, stream, w, n, chunk, vec, state,
                           wave_counts, nblocks);
}

extern "C" void launch_tk_write(const void* words, float* zdst, int64_t n,
                                int keymode, int64_t chunk, int nblocks,
                                const uint32_t* state, const int* offs_gt,
                                const int* offs_eq, const int32_t* uidx,
                                const float* uval, int32_t* out_idx,
                                float* out_val, int kout, hipStream_t stream) {
    const uint32_t* w = (const uint32_t*)words;
    int vec = ((uintptr_t)w & 15) == 0;
    if (keymode)
        hipLaunchKernelGGL((tk_write_kernel<SRC_KEY>), dim3(nblocks),
                           dim3(TK_BLOCK), 0, stream, w, zdst, n, chunk, vec,
                           state, offs_gt, offs_eq, uidx, uval, out_idx,
                           out_val, kout);
    else
        hipLaunchKernelGGL((tk_write_kernel<SRC_F32>), dim3(nblocks),
                           dim3(TK_BLOCK), 0, stream, w, zdst, n, chunk, vec,
                           state, offs_gt, offs_eq, uidx, uval, out_idx,
                           out_val, kout);
}

extern "C" void launch_tk_merge_slots(const int32_t* a_idx, const float* a_val,
                                      int na, const int32_t* b_idx,
                                      const float* b_val, int nb,
                                      uint32_t* ukey, int32_t* uidx,
                                      float* uval, int* ndup,
                                      hipStream_t stream) {
    int total = na + nb;
    int blocks = (total + TK_BLOCK - 1) / TK_BLOCK;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(tk_merge_slots_kernel, dim3(blocks), dim3(TK_BLOCK), 0,
                       stream, a_idx, a_val, na, b_idx, b_val, nb, ukey, uidx,
                       uval, ndup);
}

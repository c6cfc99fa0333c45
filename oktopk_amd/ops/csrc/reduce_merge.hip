// Ok-Topk round-1 reduce at a region owner as an ordered sparse merge
// (gfx950, wave64).
//
// Replaces zeros(hi - lo) + scatter_add_ / unpack_scatter_add_ (float
// atomics) + compact_gt + "+ lo".  The payload an owner receives is P
// segments in rank order, each ascending and duplicate-free, so the reduce is
// a P-way merge of sorted runs: work proportional to the payload, no atomics,
// and the summation order fixed by construction — ((v_a + v_b) + v_c) ... in
// ascending segment order, which is the order index_add_ takes on the CPU.
// Nothing is allocated or touched at the region length.
//
//   rm_merge   stable merge by rank.  One thread per entry e = (x, v) at
//              position p of segment j; its slot in the merged scratch is
//                p + sum_{j'<j} upper_bound_{j'}(x) + sum_{j'>j} lower_bound_{j'}(x)
//              — a bijection onto [0, M) for ascending input, equal indices
//              adjacent and in segment order.  Every term is bounded by its
//              segment's count, so a slot is below M for ANY input (unsorted
//              segments included): no store can leave the scratch.  MODE
//              selects the source: 0 the (idx, val) pair form, 1 the fp32
//              wire, 2 the bf16 wire ([idx | val bits] per segment, decoded
//              as r2_wire_tail_kernel does; no unpacked copy is made).
//   rm_heads   an entry is a run head when its predecessor's index differs.
//              A head sums its run left to right (runs are at most P long),
//              then applies the range test base <= x < base + length and
//              compact_gt's predicate |s| > tau.  WRITE = false: per-wave
//              keep counts (geometry of compact_count: block b, wave w own
//              merged positions [b*chunk + w*sub, +sub), sub = chunk / 4).
//              WRITE = true: the same walk with the scanned offsets, so the
//              output is ascending with no atomics.  The run is summed again
//              in the write pass rather than kept in a third scratch array.
//   The count table is scanned by scan_offsets / count_totals (kernels.hip);
//   the total is the single readback, where compact_gt had one.
//
// Starting from +0.0 as the reference does changes nothing that survives:
// 0 + v == v bit for bit unless v is -0.0, and a sum of zeros is dropped by
// |s| > tau (tau >= 0), as is a NaN sum.
//
// Cost model: (P - 1) binary searches per entry, each inside the window of
// its segment that the block's 256 entries span (see rm_merge) — about
// log2(256) = 8 dependent 4-byte loads when the segments are equally dense,
// so roughly 8 * M * (P - 1) loads in all, from cache lines the whole block
// shares, plus 2 * P full-segment searches per block for the windows.
// Against three passes over n / P floats this wins while the region is large
// and P small, and loses at large P, where the region is short and the
// search count grows (measured: profiles/README.md r12); the device path is
// capped at RM_MAX_SEG segments, beyond which the ops layer runs the
// reference composition.
//
// Conventions follow wire_codec.hip / round2_tail.hip: block 256, at most
// 2048 blocks, grid-stride in rm_merge, segment tables ([element prefix |
// word prefix], P + 1 ints each, uploaded once) copied to LDS.  Only 4-byte
// alignment of the inputs is assumed (dword and 16-bit accesses only).

#include <hip/hip_runtime.h>
#include <cstdint>

#define RM_BLOCK 256
#define RM_WAVES (RM_BLOCK / 64)
#define RM_MAX_BLOCKS 2048
#define RM_MAX_SEG 64  // <= WIRE_MAX_SEG

// segment of element i: the j with tab[j] <= i < tab[j+1] (wire_find_seg)
__device__ __forceinline__ int rm_find_seg(const int* tab, int P, int i) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// number of a[0, c) below x (UPPER: not above x), searched inside [lo, hi]
template <bool UPPER>
__device__ __forceinline__ int rm_bound(const int32_t* __restrict__ a, int lo,
                                        int hi, int32_t x) {
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        const int32_t y = a[mid];
        if (UPPER ? y <= x : y < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// rm_merge.  `ibuf` holds the index lists: segment j's starts at word
// s_woff[j] (pair form: woff == eoff and ibuf is idx; wire form: ibuf is the
// wire buffer).  `val` is read in the pair form only.
//
// A block's 256 consecutive entries span [xmin, xmax]; thread q first finds
// segment q's window [lower_bound(xmin), upper_bound(xmax)], which holds
// every bound of every x in the span, so the per-entry searches run inside
// the windows (about as many entries as the block holds, and the same cache
// lines for the whole block) instead of whole segments.  Every bound stays
// within [0, count] whatever the input, so the slot stays below M.
// ---------------------------------------------------------------------------
template <int MODE>
__global__ void rm_merge_kernel(const int32_t* __restrict__ ibuf,
                                const float* __restrict__ val,
                                const int* __restrict__ meta, int P, int M,
                                int32_t* __restrict__ midx,
                                float* __restrict__ mval) {
    __shared__ int s_eoff[RM_MAX_SEG + 1];
    __shared__ int s_woff[RM_MAX_SEG + 1];
    __shared__ int s_wlo[RM_MAX_SEG];
    __shared__ int s_whi[RM_MAX_SEG];
    __shared__ int32_t s_min[RM_WAVES];
    __shared__ int32_t s_max[RM_WAVES];
    for (int j = threadIdx.x; j <= P; j += RM_BLOCK) {
        s_eoff[j] = meta[j];
        s_woff[j] = meta[P + 1 + j];
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * RM_BLOCK;
    // block-uniform trip count: every thread reaches both barriers
    for (int64_t tile = (int64_t)blockIdx.x * RM_BLOCK; tile < M; tile += stride) {
        const int64_t i = tile + threadIdx.x;
        const bool live = i < M;
        int j = 0, r = 0;
        int32_t x = 0;
        float v = 0.f;
        if (live) {
            j = rm_find_seg(s_eoff, P, (int)i);
            r = (int)i - s_eoff[j];
            const int c = s_eoff[j + 1] - s_eoff[j];
            const int32_t* seg = ibuf + s_woff[j];
            x = seg[r];
            if (MODE == 0)
                v = val[i];
            else if (MODE == 1)
                v = __uint_as_float((uint32_t)seg[c + r]);
            else
                v = __uint_as_float(
                    ((uint32_t)reinterpret_cast<const uint16_t*>(seg + c)[r]) << 16);
        }
        int32_t mn = live ? x : INT32_MAX, mx = live ? x : INT32_MIN;
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, __shfl_xor(mn, o));
            mx = max(mx, __shfl_xor(mx, o));
        }
        if ((threadIdx.x & 63) == 0) {
            s_min[threadIdx.x >> 6] = mn;
            s_max[threadIdx.x >> 6] = mx;
        }
        __syncthreads();
        if (threadIdx.x < P) {
            int32_t bmin = s_min[0], bmax = s_max[0];
            for (int w = 1; w < RM_WAVES; ++w) {
                bmin = min(bmin, s_min[w]);
                bmax = max(bmax, s_max[w]);
            }
            const int q = threadIdx.x;
            const int c = s_eoff[q + 1] - s_eoff[q];
            const int32_t* a = ibuf + s_woff[q];
            s_wlo[q] = rm_bound<false>(a, 0, c, bmin);
            s_whi[q] = rm_bound<true>(a, 0, c, bmax);
        }
        __syncthreads();
        if (live) {
            int slot = r;
            for (int q = 0; q < j; ++q)
                slot += rm_bound<true>(ibuf + s_woff[q], s_wlo[q], s_whi[q], x);
            for (int q = j + 1; q < P; ++q)
                slot += rm_bound<false>(ibuf + s_woff[q], s_wlo[q], s_whi[q], x);
            if (slot < M) {  // always true; keeps the store inside the scratch
                midx[slot] = x;
                mval[slot] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// rm_heads.  One merged position per lane per step, so lane order is position
// order.  `kout` bounds every output store.
// ---------------------------------------------------------------------------
template <bool WRITE>
__global__ void rm_heads_kernel(const int32_t* __restrict__ midx,
                                const float* __restrict__ mval, int M,
                                int chunk, int64_t base, int64_t length,
                                float tau, int* __restrict__ counts,
                                const int* __restrict__ offs,
                                int32_t* __restrict__ out_idx,
                                float* __restrict__ out_val, int kout) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sub = chunk / RM_WAVES;
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > M) start = M;
    if (end > M) end = M;
    const uint64_t lt_mask = ((uint64_t)1 << lane) - 1;
    int run = WRITE ? offs[blockIdx.x * RM_WAVES + wave] : 0;
    for (int64_t b = start; b < end; b += 64) {  // wave-uniform
        const int64_t i = b + lane;
        bool keep = false;
        int32_t x = 0;
        float s = 0.f;
        if (i < end) {
            x = midx[i];
            if (i == 0 || midx[i - 1] != x) {
                s = mval[i];
                for (int64_t t = i + 1; t < M && midx[t] == x; ++t) s += mval[t];
                const int64_t d = (int64_t)x - base;
                keep = d >= 0 && d < length && fabsf(s) > tau;
            }
        }
        const uint64_t bal = __ballot(keep);
        if (WRITE && keep) {
            const int pos = run + __popcll(bal & lt_mask);
            if (pos < kout) {
                out_idx[pos] = x;
                out_val[pos] = s;
            }
        }
        run += __popcll(bal);
    }
    if (!WRITE && lane == 0) counts[blockIdx.x * RM_WAVES + wave] = run;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
extern "C" int reduce_max_segments() { return RM_MAX_SEG; }

// heads geometry: chunk a multiple of RM_BLOCK, at most RM_MAX_BLOCKS blocks
extern "C" void rm_heads_geom(int M, int* chunk, int* nblocks) {
    int64_t nb = ((int64_t)M + RM_BLOCK - 1) / RM_BLOCK;
    if (nb < 1) nb = 1;
    if (nb > RM_MAX_BLOCKS) nb = RM_MAX_BLOCKS;
    int64_t ch = (((int64_t)M + nb - 1) / nb + RM_BLOCK - 1) / RM_BLOCK * RM_BLOCK;
    if (ch < RM_BLOCK) ch = RM_BLOCK;
    nb = ((int64_t)M + ch - 1) / ch;
    if (nb < 1) nb = 1;
    *chunk = (int)ch;
    *nblocks = (int)nb;
}

// mode: 0 pair form, 1 fp32 wire, 2 bf16 wire
extern "C" void launch_rm_merge(const int32_t* ibuf, const float* val,
                                const int* meta, int P, int M, int mode,
                                int32_t* midx, float* mval, hipStream_t stream) {
    int64_t nb = ((int64_t)M + RM_BLOCK - 1) / RM_BLOCK;
    if (nb < 1) nb = 1;
    if (nb > RM_MAX_BLOCKS) nb = RM_MAX_BLOCKS;
    const dim3 grid((unsigned)nb), block(RM_BLOCK);
    if (mode == 0)
        hipLaunchKernelGGL((rm_merge_kernel<0>), grid, block, 0, stream, ibuf,
                           val, meta, P, M, midx, mval);
    else if (mode == 1)
        hipLaunchKernelGGL((rm_merge_kernel<1>), grid, block, 0, stream, ibuf,
                           val, meta, P, M, midx, mval);
    else
        hipLaunchKernelGGL((rm_merge_kernel<2>), grid, block, 0, stream, ibuf,
                           val, meta, P, M, midx, mval);
}

// offs == nullptr: count pass into counts[nblocks * 4]; otherwise the write
// pass with the exclusive scan of those counts
extern "C" void launch_rm_heads(const int32_t* midx, const float* mval, int M,
                                int chunk, int nblocks, int64_t base,
                                int64_t length, float tau, int* counts,
                                const int* offs, int32_t* out_idx,
                                float* out_val, int kout, hipStream_t stream) {
    if (offs == nullptr)
        hipLaunchKernelGGL((rm_heads_kernel<false>), dim3(nblocks),
                           dim3(RM_BLOCK), 0, stream, midx, mval, M, chunk, base,
                           length, tau, counts, offs, out_idx, out_val, kout);
    else
        hipLaunchKernelGGL((rm_heads_kernel<true>), dim3(nblocks),
                           dim3(RM_BLOCK), 0, stream, midx, mval, M, chunk, base,
                           length, tau, counts, offs, out_idx, out_val, kout);
}

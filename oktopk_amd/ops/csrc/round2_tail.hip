// Ok-Topk round-2 tail (gfx950, wave64): the global selection over the
// gathered survivors and the residual credit, device-resident.
//
// Replaces, after the sparse allgather of round 2 (reference
// VGG/allreducer.py:833-845,1051-1052): abs + torch.topk + .item() + two
// gathers on an exact-recompute iteration, and on every iteration the
// credit through an n-element bool mask (two int64 index copies, two
// index_puts, zero_at_masked_).  Both index lists are ascending, so the
// credit is a binary search of the ~k-entry local selection per selected
// entry — the sorted intersection the reference takes with np.intersect1d.
// Nothing here is sized by the dense length n.
//
//   threshold iteration (every gathered entry is the selection): ONE launch
//     r2_credit       pair form: one thread per gathered entry, search +
//                     store of +0.0f into the residual on a hit
//     r2_wire_tail    wire form: the same thread first decodes its entry
//                     through the LDS segment tables (wire_codec.hip) and
//                     stores (idx, val)
//   exact iteration: the level / pick / count / scan kernels of
//   topk_select.hip over the gathered values, with
//     r2_wire_tail<HIST>  wire form: decode + store fused with radix level 1
//                     (bin = |v| bits >> 21), as tk_ef_hist fuses it into
//                     the EF restore
//     r2_write        the select's write pass over (all_idx, all_val): an
//                     entry's output slot is gt_before + min(eq_before,
//                     need), monotone in the position, so g_idx is ascending
//                     with no atomics; the credit lookup rides along
//
// Every launch takes tau / need from the 16-byte state record; that record
// is the only readback.  Only 4-byte alignment of the inputs is assumed
// (dword and 16-bit accesses only).  No float atomics: the one value ever
// written to the residual is +0.0f, by plain vector stores.

#include <hip/hip_runtime.h>
#include <cstdint>

#define R2_BLOCK 256
#define R2_WAVES (R2_BLOCK / 64)
#define R2_MAX_BLOCKS 2048
#define R2_MAX_SEG 1024  // == WIRE_MAX_SEG: the tables are built for both
#define R2_BINS 2048     // radix level 1: 11 bits, as topk_select.hip

static inline int r2_blocks(int64_t work) {
    int64_t b = (work + R2_BLOCK - 1) / R2_BLOCK;
    if (b < 1) b = 1;
    if (b > R2_MAX_BLOCKS) b = R2_MAX_BLOCKS;
    return (int)b;
}

// residual[x] = +0.0f when x is in the ascending local selection idx[0, m).
// x outside [0, n) is dropped, so no store can leave the residual.
__device__ __forceinline__ void r2_credit(int32_t x,
                                          const int32_t* __restrict__ idx,
                                          int m, float* __restrict__ residual,
                                          int64_t n) {
    int lo = 0, hi = m;  // first idx >= x
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (idx[mid] < x) lo = mid + 1; else hi = mid;
    }
    if (lo < m && idx[lo] == x && x >= 0 && (int64_t)x < n) residual[x] = 0.f;
}

// ---------------------------------------------------------------------------
// threshold iteration, pair form: the gathered lists are the result as they
// stand; only the credit runs.
// ---------------------------------------------------------------------------
__global__ void r2_credit_kernel(const int32_t* __restrict__ all_idx, int S,
                                 const int32_t* __restrict__ idx, int m,
                                 float* __restrict__ residual, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * R2_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * R2_BLOCK;
    for (; i < S; i += stride) r2_credit(all_idx[i], idx, m, residual, n);
}

// segment of element i: the j with tab[j] <= i < tab[j+1] (wire_find_seg)
__device__ __forceinline__ int r2_find_seg(const int* tab, int P, int i) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// wire form: one thread per gathered entry decodes it ([idx | val bits] per
// segment, meta = [element prefix | word prefix], both P+1 ints) and stores
// (idx, val).  HIST = false (threshold iteration): the credit lookup follows
// in the same thread.  HIST = true (exact iteration): the entry is counted
// into radix level 1 instead; the credit waits for the selection.
// ---------------------------------------------------------------------------
template <bool HIST>
__global__ void r2_wire_tail_kernel(const int32_t* __restrict__ buf,
                                    const int* __restrict__ meta, int P,
                                    int total, int bf16,
                                    int32_t* __restrict__ out_idx,
                                    float* __restrict__ out_val,
                                    const int32_t* __restrict__ idx, int m,
                                    float* __restrict__ residual, int64_t n,
                                    unsigned int* __restrict__ ghist) {
    __shared__ int s_eoff[R2_MAX_SEG + 1];
    __shared__ int s_woff[R2_MAX_SEG + 1];
    __shared__ unsigned int lhist[HIST ? R2_BINS : 1];
    for (int j = threadIdx.x; j <= P; j += R2_BLOCK) {
        s_eoff[j] = meta[j];
        s_woff[j] = meta[P + 1 + j];
    }
    if (HIST)
        for (int b = threadIdx.x; b < R2_BINS; b += R2_BLOCK) lhist[b] = 0;
    __syncthreads();
    int64_t i = (int64_t)blockIdx.x * R2_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * R2_BLOCK;
    for (; i < total; i += stride) {
        const int j = r2_find_seg(s_eoff, P, (int)i);
        const int r = (int)i - s_eoff[j];
        const int c = s_eoff[j + 1] - s_eoff[j];
        const int32_t* seg = buf + s_woff[j];
        const int32_t x = seg[r];
        uint32_t bits;
        if (bf16)
            bits = ((uint32_t)reinterpret_cast<const uint16_t*>(seg + c)[r]) << 16;
        else
            bits = (uint32_t)seg[c + r];
        out_idx[i] = x;
        out_val[i] = __uint_as_float(bits);
        if (HIST)
            atomicAdd(&lhist[(bits & 0x7fffffffu) >> 21], 1u);
        else if (m > 0)
            r2_credit(x, idx, m, residual, n);
    }
    if (HIST) {
        __syncthreads();
        for (int b = threadIdx.x; b < R2_BINS; b += R2_BLOCK)
            if (lhist[b]) atomicAdd(&ghist[b], lhist[b]);
    }
}

// ---------------------------------------------------------------------------
// exact iteration, write pass.  Geometry is tk_count_kernel's: block b, wave
// w own positions [b*chunk + w*sub, + sub), sub = chunk / 4, and offs_gt /
// offs_eq hold the exclusive scans of the per-wave (gt, eq) counts in that
// order.  One position per lane per step, so lane order is position order.
// `kout` bounds every output store.
// ---------------------------------------------------------------------------
__global__ void r2_write_kernel(const uint32_t* __restrict__ w,
                                const int32_t* __restrict__ all_idx, int64_t S,
                                int64_t chunk,
                                const uint32_t* __restrict__ state,
                                const int* __restrict__ offs_gt,
                                const int* __restrict__ offs_eq,
                                const int32_t* __restrict__ idx, int m,
                                float* __restrict__ residual, int64_t n,
                                int32_t* __restrict__ out_idx,
                                float* __restrict__ out_val, int kout) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t sub = chunk / R2_WAVES;
    int64_t start = (int64_t)blockIdx.x * chunk + (int64_t)wave * sub;
    int64_t end = start + sub;
    if (start > S) start = S;
    if (end > S) end = S;
    const uint32_t tau = state[0];
    const int need = (int)state[2];
    const uint64_t lt_mask = ((uint64_t)1 << lane) - 1;
    int gt_run = offs_gt[blockIdx.x * R2_WAVES + wave];
    int eq_run = offs_eq[blockIdx.x * R2_WAVES + wave];
    for (int64_t base = start; base < end; base += 64) {  // wave-uniform
        const int64_t i = base + lane;
        const bool ok = i < end;
        const uint32_t u = ok ? w[i] : 0u;
        const uint32_t key = u & 0x7fffffffu;
        const bool g = ok && key > tau;
        const bool e = ok && key == tau;
        const uint64_t bg = __ballot(g), be = __ballot(e);
        const int gr = gt_run + __popcll(bg & lt_mask);
        const int er = eq_run + __popcll(be & lt_mask);
        if (g || (e && er < need)) {
            const int pos = gr + (er < need ? er : need);
            if (pos < kout) {
                const int32_t x = all_idx[i];
                out_idx[pos] = x;
                out_val[pos] = __uint_as_float(u);
                if (m > 0) r2_credit(x, idx, m, residual, n);
            }
        }
        gt_run += __popcll(bg);
        eq_run += __popcll(be);
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
extern "C" void launch_r2_credit(const int32_t* all_idx, int S,
                                 const int32_t* idx, int m, float* residual,
                                 int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(r2_credit_kernel, dim3(r2_blocks(S)), dim3(R2_BLOCK), 0,
                       stream, all_idx, S, idx, m, residual, n);
}

// hist == nullptr: threshold iteration (decode + credit); otherwise decode +
// radix level 1 into hist[2048]
extern "C" void launch_r2_wire_tail(const int32_t* buf, const int* meta, int P,
                                    int total, int bf16, int32_t* out_idx,
                                    float* out_val, const int32_t* idx, int m,
                                    float* residual, int64_t n,
                                    unsigned int* hist, hipStream_t stream) {
    if (hist != nullptr)
        hipLaunchKernelGGL((r2_wire_tail_kernel<true>), dim3(r2_blocks(total)),
                           dim3(R2_BLOCK), 0, stream, buf, meta, P, total, bf16,
                           out_idx, out_val, idx, m, residual, n, hist);
    else
        hipLaunchKernelGGL((r2_wire_tail_kernel<false>), dim3(r2_blocks(total)),
                           dim3(R2_BLOCK), 0, stream, buf, meta, P, total, bf16,
                           out_idx, out_val, idx, m, residual, n, hist);
}

extern "C" void launch_r2_write(const void* words, const int32_t* all_idx,
                                int64_t S, int64_t chunk, int nblocks,
                                const uint32_t* state, const int* offs_gt,
                                const int* offs_eq, const int32_t* idx, int m,
                                float* residual, int64_t n, int32_t* out_idx,
                                float* out_val, int kout, hipStream_t stream) {
    hipLaunchKernelGGL(r2_write_kernel, dim3(nblocks), dim3(R2_BLOCK), 0, stream,
                       (const uint32_t*)words, all_idx, S, chunk, state, offs_gt,
                       offs_eq, idx, m, residual, n, out_idx, out_val, kout);
}

// Device-side sparse wire codec for the Ok-Topk engine (gfx950).
//
// Wire layout (AllReducer._pack / _unpack / _pack_ints — unchanged): segment
// j with c_j elements is c_j int32 indices followed by the values,
//   fp32 wire: c_j fp32 words
//   bf16 wire: ceil(c_j / 2) int32 words holding c_j bf16 values; when c_j
//              is odd the trailing half-word is ZERO
// and the segments are concatenated in destination / rank order.
//
//   wire_cuts    one binary search per interior region boundary over the
//                ascending selection -> cuts[P+1] (element offsets) and the
//                word-offset prefix woff[P+1], both left in device memory
//   wire_pack    one thread per element: index word, value (fp32 word or a
//                16-bit bf16 store) and the zero pad half-word
//   wire_unpack  gathers all segments into contiguous (idx, fp32 val)
//   wire_scatter_add   dest[idx - base] += val for every wire entry, never
//                materialising idx / val
//
// Every per-element kernel finds its segment by binary search over an LDS
// copy of the element-prefix table.  Conventions follow kernels.hip: wave64,
// BLOCK 256, grid-stride with <= 2048 blocks.  Only 4-byte alignment of the
// inputs is assumed (all loads/stores are dword or 16-bit).

#include <hip/hip_runtime.h>
#include <cstdint>

#define BLOCK 256
#define MAX_BLOCKS 2048
// tables are [WIRE_MAX_SEG + 1] ints each; two of them live in LDS (8.2 KB)
#define WIRE_MAX_SEG 1024

static inline int wire_blocks(int64_t work) {
    int64_t b = (work + BLOCK - 1) / BLOCK;
    if (b < 1) b = 1;
    if (b > MAX_BLOCKS) b = MAX_BLOCKS;
    return (int)b;
}

// fp32 -> bf16 bits, round-to-nearest-even; bit-equal to torch's
// .to(bfloat16) for every non-NaN input.  NaN stays a (quiet) NaN — the
// rounding add alone would carry some NaN payloads into the exponent.
__device__ __forceinline__ uint16_t wire_f2bf(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

__device__ __forceinline__ float wire_bf2f(uint16_t h) {
    return __uint_as_float(((uint32_t)h) << 16);
}

__device__ __forceinline__ int wire_val_words(int c, int bf16) {
    return bf16 ? (c + 1) >> 1 : c;
}

// segment of element i: the j with tab[j] <= i < tab[j+1] (empty segments,
// tab[j] == tab[j+1], are stepped over).  Requires tab[0] <= i < tab[P].
__device__ __forceinline__ int wire_find_seg(const int* tab, int P, int i) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (tab[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// wire_cuts: single block.  cuts[j] = lower_bound(idx, bounds[j]) for the
// interior boundaries (the searchsorted rule: an index equal to a boundary
// goes to the upper region), cuts[0] = 0, cuts[P] = m; then an exclusive
// scan of the per-segment word counts -> woff[P+1].  meta = [cuts | woff].
// ---------------------------------------------------------------------------
__global__ void wire_cuts_kernel(const int32_t* __restrict__ idx, int m,
                                 const int64_t* __restrict__ bounds, int P,
                                 int bf16, int* __restrict__ meta) {
    __shared__ int s_cuts[WIRE_MAX_SEG + 1];
    __shared__ int s_part[BLOCK];
    const int tid = threadIdx.x;
    for (int j = tid; j <= P; j += BLOCK) {
        int cut;
        if (j == 0) cut = 0;
        else if (j == P) cut = m;
        else {
            int64_t b = bounds[j];
            int lo = 0, hi = m;
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if ((int64_t)idx[mid] < b) lo = mid + 1; else hi = mid;
            }
            cut = lo;
        }
        s_cuts[j] = cut;
    }
    __syncthreads();
    // thread t owns segments [t*PER, t*PER + PER)
    const int PER = WIRE_MAX_SEG / BLOCK;
    int loc[PER];
    int s = 0;
    #pragma unroll
    for (int q = 0; q < PER; ++q) {
        int j = tid * PER + q;
        loc[q] = s;
        if (j < P) {
            int c = s_cuts[j + 1] - s_cuts[j];
            s += c + wire_val_words(c, bf16);
        }
    }
    s_part[tid] = s;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {  // Hillis-Steele over the partials
        int v = tid >= d ? s_part[tid - d] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int prefix = tid == 0 ? 0 : s_part[tid - 1];
    int* woff = meta + (P + 1);
    #pragma unroll
    for (int q = 0; q < PER; ++q) {
        int j = tid * PER + q;
        if (j < P) woff[j] = prefix + loc[q];
    }
    if (tid == BLOCK - 1) woff[P] = s_part[BLOCK - 1];
    for (int j = tid; j <= P; j += BLOCK) meta[j] = s_cuts[j];
}

// stage [eoff | woff] (2 * (P+1) ints) into LDS
__device__ __forceinline__ void wire_stage(const int* __restrict__ meta, int P,
                                           int* s_eoff, int* s_woff) {
    for (int j = threadIdx.x; j <= P; j += BLOCK) {
        s_eoff[j] = meta[j];
        s_woff[j] = meta[P + 1 + j];
    }
    __syncthreads();
}

__global__ void wire_pack_kernel(const int32_t* __restrict__ idx,
                                 const float* __restrict__ val, int m,
                                 const int* __restrict__ meta, int P, int bf16,
                                 int32_t* __restrict__ buf) {
    __shared__ int s_eoff[WIRE_MAX_SEG + 1];
    __shared__ int s_woff[WIRE_MAX_SEG + 1];
    wire_stage(meta, P, s_eoff, s_woff);
    int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (; i < m; i += stride) {
        int j = wire_find_seg(s_eoff, P, (int)i);
        int r = (int)i - s_eoff[j];
        int c = s_eoff[j + 1] - s_eoff[j];
        int32_t* seg = buf + s_woff[j];
        seg[r] = idx[i];
        if (bf16) {
            // neighbours share a word and belong to different lanes:
            // 16-bit stores, never read-modify-write
            uint16_t* hv = reinterpret_cast<uint16_t*>(seg + c);
            hv[r] = wire_f2bf(val[i]);
            if (r == c - 1 && (c & 1)) hv[c] = 0;
        } else {
            seg[c + r] = (int32_t)__float_as_uint(val[i]);
        }
    }
}

__global__ void wire_unpack_kernel(const int32_t* __restrict__ buf,
                                   const int* __restrict__ meta, int P,
                                   int total, int bf16,
                                   int32_t* __restrict__ out_idx,
                                   float* __restrict__ out_val) {
    __shared__ int s_eoff[WIRE_MAX_SEG + 1];
    __shared__ int s_woff[WIRE_MAX_SEG + 1];
    wire_stage(meta, P, s_eoff, s_woff);
    int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (; i < total; i += stride) {
        int j = wire_find_seg(s_eoff, P, (int)i);
        int r = (int)i - s_eoff[j];
        int c = s_eoff[j + 1] - s_eoff[j];
        const int32_t* seg = buf + s_woff[j];
        out_idx[i] = seg[r];
        if (bf16)
            out_val[i] = wire_bf2f(reinterpret_cast<const uint16_t*>(seg + c)[r]);
        else
            out_val[i] = __uint_as_float((uint32_t)seg[c + r]);
    }
}

// dest[idx - base] += val for every wire entry.  The caller guarantees
// base <= idx < base + n (scatter_add_'s contract); an entry outside that
// range is dropped rather than written out of bounds.
__global__ void wire_scatter_add_kernel(float* __restrict__ dest, int64_t n,
                                        const int32_t* __restrict__ buf,
                                        const int* __restrict__ meta, int P,
                                        int total, int64_t base, int bf16) {
    __shared__ int s_eoff[WIRE_MAX_SEG + 1];
    __shared__ int s_woff[WIRE_MAX_SEG + 1];
    wire_stage(meta, P, s_eoff, s_woff);
    int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (; i < total; i += stride) {
        int j = wire_find_seg(s_eoff, P, (int)i);
        int r = (int)i - s_eoff[j];
        int c = s_eoff[j + 1] - s_eoff[j];
        const int32_t* seg = buf + s_woff[j];
        int64_t d = (int64_t)seg[r] - base;
        float v = bf16 ? wire_bf2f(reinterpret_cast<const uint16_t*>(seg + c)[r])
                       : __uint_as_float((uint32_t)seg[c + r]);
        if (d >= 0 && d < n) atomicAdd(&dest[d], v);
    }
}

extern "C" int wire_max_segments() { return WIRE_MAX_SEG; }

extern "C" void launch_wire_cuts(const int32_t* idx, int m, const int64_t* bounds,
                                 int P, int bf16, int* meta, hipStream_t stream) {
    hipLaunchKernelGGL(wire_cuts_kernel, dim3(1), dim3(BLOCK), 0, stream, idx, m,
                       bounds, P, bf16, meta);
}

extern "C" void launch_wire_pack(const int32_t* idx, const float* val, int m,
                                 const int* meta, int P, int bf16, int32_t* buf,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(wire_pack_kernel, dim3(wire_blocks(m)), dim3(BLOCK), 0,
                       stream, idx, val, m, meta, P, bf16, buf);
}

extern "C" void launch_wire_unpack(const int32_t* buf, const int* meta, int P,
                                   int total, int bf16, int32_t* out_idx,
                                   float* out_val, hipStream_t stream) {
    hipLaunchKernelGGL(wire_unpack_kernel, dim3(wire_blocks(total)), dim3(BLOCK),
                       0, stream, buf, meta, P, total, bf16, out_idx, out_val);
}

extern "C" void launch_wire_scatter_add(float* dest, int64_t n, const int32_t* buf,
                                        const int* meta, int P, int total,
                                        int64_t base, int bf16,
                                        hipStream_t stream) {
    hipLaunchKernelGGL(wire_scatter_add_kernel, dim3(wire_blocks(total)),
                       dim3(BLOCK), 0, stream, dest, n, buf, meta, P, total, base,
                       bf16);
}

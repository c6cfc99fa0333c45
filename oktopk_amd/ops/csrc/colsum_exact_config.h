// Launch configuration torch picks for
//     at::sum_out(out_bf16[C], src_bf16[R, C] contiguous, {0})
// ported from setReduceConfig / ReduceConfig::set_block_dimension /
// get_output_vec_size in ATen/native/cuda/Reduce.cuh (torch 2.10, USE_ROCM
// branches included).  Only the association tree of the fp32 adds matters to
// colsum_exact_kernel, and that tree is fixed by (split, bh, ctas):
//   split : rows are dealt over threadIdx.y (input_mult[1] != 0)
//   bh    : block height
//   ctas  : blocks per output strip (ctas_per_output)
// V and bw are returned because they are part of the same derivation and the
// tests print them.  Anything this port does not cover is "unsupported"; the
// caller then runs torch's own reduction.
#pragma once
#include <algorithm>
#include <cstdint>

namespace colsum_exact {

struct Config {
    bool supported = false;
    int V = 1;       // output_vec_size
    int bw = 1;      // block width
    int bh = 1;      // block height
    bool split = false;
    int ctas = 1;    // ctas_per_output
};

inline int64_t last_pow2(int64_t n) {
    int64_t p = 1;
    while (p * 2 <= n) p *= 2;
    return p;
}

inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// src_addr: byte address of src[0, 0].  num_mp / max_threads_per_mp /
// warp_size: the device properties torch reads (multiProcessorCount,
// maxThreadsPerMultiProcessor, warpSize).
inline Config derive(int64_t R, int64_t C, uint64_t src_addr, int num_mp,
                     int max_threads_per_mp, int warp_size) {
    Config cfg;
    // R == 1 or C == 1 collapse the TensorIterator to one dimension (a copy,
    // or a reduction over the fastest dimension with block_x_reduce);
    // sub-iterators of a >32-bit problem are split differently.
    if (R < 2 || C < 2 || num_mp < 1 || warp_size < 1) return cfg;
    if (R > INT32_MAX / C) return cfg;            // numel within 32-bit indexing
    if (R * C * 2 > (int64_t)INT32_MAX) return cfg;  // byte offsets as well

    // get_output_vec_size: base address, output extent and row stride, all
    // in elements
    int V = 4;
    const uint64_t ns[3] = {src_addr / 2, (uint64_t)C, (uint64_t)C};
    for (uint64_t n : ns)
        while (n % (uint64_t)V != 0) V /= 2;

    // set_block_dimension(dim0 = C / V, dim1 = R)
    const int64_t dim0 = C / V, dim1 = R;
    const int max_nt = 512 / V;
    const int dim0_pow2 = dim0 < max_nt ? (int)last_pow2(dim0) : max_nt;
    const int dim1_pow2 = dim1 < max_nt ? (int)last_pow2(dim1) : max_nt;
    int bw = std::min(dim0_pow2, warp_size);
    const int bh = std::min(dim1_pow2, max_nt / bw);
    bw = std::min(dim0_pow2, max_nt / bh);
    const int num_threads = bw * bh;

    // output split across lanes; input split across warps when that leaves
    // enough values per thread
    int64_t step_output = bw, step_input = 1;
    const bool split = R >= std::min(bh * 16, 256);
    if (split) step_input *= bh;
    else step_output *= bh;

    const int64_t grid_x = div_up(C / V, step_output);
    // USE_ROCM: a 2-D iterator that does not fit one block counts 256
    // threads per CU
    const int tpm = grid_x == 1 ? max_threads_per_mp : 256;
    const int64_t target_grid = (int64_t)num_mp * (tpm / num_threads);
    const int64_t vpt = div_up(R, step_input);
    int64_t ctas = 1;
    if (split && vpt >= 256 && grid_x <= target_grid) {
        const int64_t c1 = div_up(target_grid, grid_x);
        const int64_t c2 = div_up(vpt, 16);
        const int64_t c3 = div_up(vpt, 256);
        ctas = std::max(std::min(c1, c2), c3);
        if (ctas > num_mp)
            ctas = num_mp < 128 ? (int64_t)num_mp * (ctas > 512 ? 4 : 2) : num_mp;
        else if (ctas > div_up(num_mp, 2))
            ctas = div_up(num_mp, 2);
        else if (ctas < 16)
            ctas = 1;
    }
    // every (threadIdx.y, blockIdx.y) must own at least one row: torch
    // leaves the value of a thread without rows uninitialised
    if (split && (int64_t)bh * ctas > R) return cfg;

    cfg.supported = true;
    cfg.V = V;
    cfg.bw = bw;
    cfg.bh = bh;
    cfg.split = split;
    cfg.ctas = (int)ctas;
    return cfg;
}

}  // namespace colsum_exact

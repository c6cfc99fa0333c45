// Host-side description of one batch of LayerNorm gamma / beta gradients
// (ln_param_grads.hip; README.md here, "Batched LayerNorm parameter
// gradients").
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

// Entries one launch carries.  The table travels by value in the kernel
// arguments (68 B per entry + 8), which HIP limits to 4 KB together with the
// hidden arguments.
constexpr int LN_GRAD_BATCH_CAPACITY = 48;

struct LnGradItem {
    const void* gy;     // bf16 [M, N] contiguous
    const void* x;      // bf16 [M, N] contiguous: the LayerNorm's input
    const float* mean;  // fp32 [M]
    const float* rstd;  // fp32 [M]
    void* dst_gamma;    // bf16 [N], any element offset; dst += gamma gradient
    void* dst_beta;     // bf16 [N], likewise
    int64_t M;
    int64_t N;
};

extern "C" {
// 1 for the row counts whose summation order the kernel reproduces
int ln_param_grads_shape_ok(int64_t M, int64_t N);
// Launches ceil(n / LN_GRAD_BATCH_CAPACITY) kernels on `stream`; returns that
// count, or -1 (nothing launched) when an entry does not fit the kernel.
// No two entries of one call may share a destination element.
int launch_ln_param_grads_bf16(const LnGradItem* items, int n, hipStream_t stream);
}

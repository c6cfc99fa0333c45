// Host-side description of one launch's worth of small gradient writes
// (direct_grad.hip, "Batched small-gradient writes"; README.md here).
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

// Entries one launch carries.  The table travels by value in the kernel
// arguments (36 B per entry + 8), which HIP limits to 4 KB together with the
// hidden arguments.
constexpr int GRAD_BATCH_CAPACITY = 96;

struct GradBatchItem {
    const void* src;   // colsum: gy bf16 [R, C] contiguous; add: g bf16 [C]
    void* dst;         // bf16 [C], any element offset
    int64_t R;         // rows of gy (unused by an add)
    int64_t C;
    int bh;            // colsum: torch's block height (1 when rows are not split)
    int ctas;          // colsum: torch's blocks per output
    int is_colsum;     // 0: dst[i] = bf16(float(dst[i]) + float(src[i]))
};

extern "C" {
// 1 when launch_colsum_exact_bf16 / a batched colsum entry can run this shape
int colsum_exact_plannable(const void* gy, int64_t R, int64_t C, int bh, int ctas);
// Launches ceil(n / GRAD_BATCH_CAPACITY) kernels on `stream`; returns that
// count, or -1 (nothing launched) when an entry does not fit the kernel.
// No two entries of one call may share a destination element.
int launch_grad_batch_bf16(const GradBatchItem* items, int n, hipStream_t stream);
}

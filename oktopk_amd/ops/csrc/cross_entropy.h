// Shared between cross_entropy.hip and bindings.cpp: the kernels' argument
// blocks.
#pragma once

// Up to this many classes a wave owns a row; above, a 256-thread block does.
constexpr int CE_WAVE_ROW_MAX_C = 1024;

struct CeArgs {
    const void* logits;      // [R, C] fp32 or bf16, contiguous
    const void* target;      // [R] int32 or int64
    float* row_loss;         // [R]; +0.0 where ignored, NaN where out of range
    float* stats;            // [2, R]: row maximum, then log(sum exp(x - max))
    long long ignore_index;
    long long R;
    int C;
    int is_bf16;
    int target_i64;
};

struct CeBwdArgs {
    const void* logits;      // [R, C]
    const void* target;      // [R]
    const float* stats;      // [2, R] of the forward
    const float* gout;       // [1], or [R] with gout_per_row
    const float* factor;     // [1] of the finalize kernel, or nullptr: 1
    void* grad;              // [R, C] in the logits' dtype
    long long ignore_index;
    long long R;
    int C;
    int is_bf16;
    int target_i64;
    int gout_per_row;
};

// Shared between ctc_loss.hip and bindings.cpp: the kernel's argument block
// and the sizes the binding needs to place the lattices.
#pragma once

#include <cstddef>

// Dynamic LDS the lattices may take; with the kernel's 1.8 KB of static LDS
// this stays under the 64 KB a launch gets without asking for more.
constexpr size_t CTC_LDS_BUDGET = 60 * 1024;
constexpr int CTC_MAX_L = 127;  // S = 2L + 1 <= 255 states, 4 per lane

#ifdef __HIPCC__
#define CTC_HOST_DEVICE __host__ __device__
#else
#define CTC_HOST_DEVICE
#endif

// alpha [T][Sst], beta' [T][Sst], row max [T], row log-sum [T]
CTC_HOST_DEVICE inline size_t ctc_lattice_floats(long long T, long long Sst) {
    return (size_t)T * (size_t)(2 * Sst + 2);
}

struct CtcArgs {
    const float* logits;    // [T, N, C]
    const void* targets;    // padded [N, tgt_stride] or 1-D (tgt_stride < 0)
    const void* in_len;     // [N]
    const void* tgt_len;    // [N]
    float* nll;             // [N]
    float* grad;            // [T, N, C], or nullptr: loss only
    float* ws;              // [N][T (2 Sst + 2)], or nullptr: lattices in LDS
    long long tgt_stride;   // padded width, or -1
    long long tgt_numel;    // bound of every label read
    int T, N, C;
    int blank;              // in [0, C)
    int Sst;                // lattice row stride, 1 .. 2 CTC_MAX_L + 1
    int targets_i64, in_len_i64, tgt_len_i64;
    int zero_infinity;
};

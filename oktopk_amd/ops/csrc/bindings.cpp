// PyTorch-ROCm bindings for the CDNA4 kernel library (kernels.hip).
// API mirrors oktopk_amd/ops/reference.py one-to-one so the dispatch layer
// can swap backends and the numerics tests can A/B them.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAGeneratorImpl.h>
#include <c10/cuda/CUDAGuard.h>

#include <cstdint>
#include <vector>

#include "colsum_exact_config.h"

// launchers from kernels.hip
extern "C" {
void launch_count_gt(const float*, int64_t, float, unsigned long long*, hipStream_t);
void launch_count_multi_gt(const float*, int64_t, const float*, int, unsigned long long*,
                           hipStream_t);
void launch_compact_count_multi(const float*, int64_t, const float*, int, int64_t,
                                int, int*, hipStream_t);
void launch_compact_write(const float*, int64_t, float, int64_t, int, const int*,
                          int32_t*, float*, hipStream_t);
void launch_hist(const float*, int64_t, uint32_t, uint32_t, int, int, unsigned int*,
                 hipStream_t);
void launch_scatter_add(float*, const int32_t*, const float*, int64_t, hipStream_t);
void launch_scatter_set_scaled(float*, const int32_t*, const float*, float, int64_t,
                               hipStream_t);
void launch_scatter_gt_credit(const int32_t*, const float*, int64_t, float,
                              float, float*, float*, unsigned long long*,
                              hipStream_t);
void launch_zero_at(float*, const int32_t*, int64_t, hipStream_t);
void launch_zero_at_masked(float*, const int32_t*, const bool*, int64_t, hipStream_t);
void launch_isin_sorted(const int32_t*, int64_t, const int32_t*, int64_t, bool*,
                        hipStream_t);
void launch_ef_restore(float*, float*, int64_t, hipStream_t);
void launch_ef_upcast(float*, float*, const void*, int64_t, hipStream_t);
void launch_ef_count(float*, float*, const void*, int64_t, const float*, int,
                     int64_t, int, int*, hipStream_t);
void launch_count_totals(const int*, int, int, int64_t*, hipStream_t);
void launch_scan_offsets(const int*, int, int*, hipStream_t);
void launch_sgd(float*, const float*, float*, int64_t, float, float, float, int,
                hipStream_t);
void launch_clip_scale(const double*, float, float*, hipStream_t);
void launch_adam(float*, const float*, float*, float*, void*, const float*, int64_t, float, float,
                 float, float, float, hipStream_t);
void launch_sumsq(const float*, int64_t, double*, hipStream_t);
void launch_sparse_sumsq(const float*, int64_t, float, float, double*, hipStream_t);
int64_t adam_sparse_ntiles(int64_t);
void launch_adam_sparse(float*, float*, float*, void*, const float*, int64_t,
                        const int32_t*, const float*, int64_t, int32_t*, int64_t,
                        float, float, float, float, float, float, float,
                        hipStream_t);
void launch_sgd_step(float*, const float*, float*, const float*, int64_t, float,
                     float, float, int, hipStream_t);
void launch_sgd_step_sparse(float*, float*, const float*, int64_t, const int32_t*,
                            const float*, int64_t, int32_t*, int64_t, float,
                            float, float, float, float, int, hipStream_t);
void launch_colsum_into_bf16(const void*, int64_t, int64_t, void*, int,
                             hipStream_t);
int launch_colsum_exact_bf16(const void*, int64_t, int64_t, void*, int, int,
                             hipStream_t);
bool ln_bwd_supported(int64_t H);
int ln_bwd_blocks(int64_t rows);
void launch_ln_bwd_into(const void* gy, const void* x, const void* gamma,
                        const float* mean, const float* rstd, int64_t rows,
                        int64_t H, void* gx, float* ws, void* dgamma,
                        void* dbeta, int accumulate, hipStream_t);
void launch_attn_rowdot(const void*, const void*, int64_t, int64_t, int64_t,
                        float*, hipStream_t);
void launch_linear_gelu(const void*, const void*, const float*, void*, void*, int,
                        int, int, int, hipStream_t);
void launch_add_ln_fwd(const void*, const void*, const void*, const void*, void*,
                       void*, float*, float*, int64_t, int, float, hipStream_t);
void launch_add_ln_bwd(const void*, const void*, const float*, const float*,
                       const void*, void*, float*, float*, int64_t, int,
                       hipStream_t);
void launch_attn_fwd(const void*, const void*, void*, void*, void*, int, int,
                     float, float, unsigned long long, unsigned long long,
                     const void*, const void*, unsigned int, int, int,
                     hipStream_t);
void launch_attn_fwd_fa(const void*, const void*, void*, void*, int, int, int,
                        float, float, unsigned long long, unsigned long long,
                        const void*, const void*, unsigned int, int, int,
                        hipStream_t);
void launch_dropout_mask_mul(void*, int64_t, int64_t, unsigned long long,
                             unsigned long long, const void*, const void*,
                             unsigned int, int, float, hipStream_t);
void launch_attn_bwd_fa(const void*, const void*, const void*, const void*,
                        const void*, void*, int, int, int, float, float,
                        unsigned long long, unsigned long long, const void*,
                        const void*, unsigned int, int, int, hipStream_t);
// launchers from wire_codec.hip
// gauss_select.hip
void launch_gauss_moments(const float*, float*, const void*, int64_t, int64_t,
                          int, double*, hipStream_t);
void launch_gauss_finalize(const double*, int, int64_t, double, float*, double*,
                           hipStream_t);
void launch_gauss_count(const float*, int64_t, const float*, int64_t, int, int*,
                        hipStream_t);
void launch_gauss_decide(const int*, int, int64_t, const float*, double*,
                         hipStream_t);
// topk_select.hip
void launch_tk_ef_hist(const float*, float*, const void*, int64_t, unsigned int*,
                       hipStream_t);
void launch_tk_hist(const void*, int64_t, int, const uint32_t*, int, int, int,
                    unsigned int*, hipStream_t);
void launch_tk_pick(unsigned int*, int, int, uint32_t*, uint32_t, int,
                    hipStream_t);
void launch_tk_count(const void*, int64_t, int, int64_t, int, const uint32_t*,
                     int*, hipStream_t);
void launch_tk_write(const void*, float*, int64_t, int, int64_t, int,
                     const uint32_t*, const int*, const int*, const int32_t*,
                     const float*, int32_t*, float*, int, hipStream_t);
void launch_tk_merge_slots(const int32_t*, const float*, int, const int32_t*,
                           const float*, int, uint32_t*, int32_t*, float*, int*,
                           hipStream_t);
int wire_max_segments();
void launch_wire_cuts(const int32_t*, int, const int64_t*, int, int, int*,
                      hipStream_t);
void launch_wire_pack(const int32_t*, const float*, int, const int*, int, int,
                      int32_t*, hipStream_t);
void launch_wire_unpack(const int32_t*, const int*, int, int, int, int32_t*,
                        float*, hipStream_t);
void launch_wire_scatter_add(float*, int64_t, const int32_t*, const int*, int,
                             int, int64_t, int, hipStream_t);
// round-2 tail (round2_tail.hip)
void launch_r2_credit(const int32_t*, int, const int32_t*, int, float*, int64_t,
                      hipStream_t);
void launch_r2_wire_tail(const int32_t*, const int*, int, int, int, int32_t*,
                         float*, const int32_t*, int, float*, int64_t,
                         unsigned int*, hipStream_t);
void launch_r2_write(const void*, const int32_t*, int64_t, int64_t, int,
                     const uint32_t*, const int*, const int*, const int32_t*,
                     int, float*, int64_t, int32_t*, float*, int, hipStream_t);
// round-1 reduce as an ordered merge (reduce_merge.hip)
int reduce_max_segments();
void rm_heads_geom(int, int*, int*);
void launch_rm_merge(const int32_t*, const float*, const int*, int, int, int,
                     int32_t*, float*, hipStream_t);
void launch_rm_heads(const int32_t*, const float*, int, int, int, int64_t,
                     int64_t, float, int*, const int*, int32_t*, float*, int,
                     hipStream_t);
}

namespace {

inline hipStream_t cur_stream() {
    return at::cuda::getCurrentCUDAStream().stream();
}

void check_f32_1d(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_i32_1d(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
    TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

}  // namespace

static int64_t count_gt(torch::Tensor t, double tau) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    auto out = torch::zeros({1}, t.options().dtype(torch::kInt64));
    launch_count_gt(t.data_ptr<float>(), t.numel(), (float)tau,
                    reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
                    cur_stream());
    return out.cpu().item<int64_t>();
}

static std::vector<int64_t> count_multi_gt(torch::Tensor t, std::vector<double> taus) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    TORCH_CHECK(taus.size() >= 1 && taus.size() <= 8, "1..8 thresholds");
    float tf[8];
    for (size_t j = 0; j < taus.size(); ++j) tf[j] = (float)taus[j];
    auto out = torch::zeros({(int64_t)taus.size()}, t.options().dtype(torch::kInt64));
    launch_count_multi_gt(t.data_ptr<float>(), t.numel(), tf, (int)taus.size(),
                          reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
                          cur_stream());
    auto cpu = out.cpu();
    std::vector<int64_t> res(taus.size());
    for (size_t j = 0; j < taus.size(); ++j) res[j] = cpu[j].item<int64_t>();
    return res;
}

struct CompactGeom {
    int64_t chunk;
    int nblocks;
};

static CompactGeom compact_geom(int64_t n) {
    // chunk per block: multiple of BLOCK*COMPACT_VEC (2048) covering n,
    // keeping <= 2048 blocks (G11 grid sizing)
    const int64_t unit = 2048;
    int64_t nchunks = (n + unit - 1) / unit;
    if (nchunks < 1) nchunks = 1;
    if (nchunks > 2048) nchunks = 2048;
    int64_t chunk = ((n + nchunks - 1) / nchunks + unit - 1) / unit * unit;
    int nblocks = (int)((n + chunk - 1) / chunk);
    if (nblocks < 1) nblocks = 1;
    return {chunk, nblocks};
}

// shared tail: given per-candidate per-wave counts (ntau x nblocks*4 on CPU)
// and the chosen candidate row, launch the write pass.
// Offsets stay on the GPU: a device reduction yields the per-candidate
// totals (the ONLY values the host needs — bump rule + output sizing, 8B
// each), and a single-block scan turns the chosen row into write offsets
// in place of the former 196 KB readback + CPU scan + 32 KB upload.
struct BumpResult { int chosen; int64_t total; };

static BumpResult bump_choose(torch::Tensor counts, int ntau, int nw,
                              int64_t hi_limit) {
    auto totals = torch::empty({ntau}, counts.options().dtype(torch::kInt64));
    launch_count_totals(counts.data_ptr<int>(), nw, ntau,
                        totals.data_ptr<int64_t>(), cur_stream());
    auto th = totals.cpu();
    const int64_t* tp = th.data_ptr<int64_t>();
    for (int c = 0; c < ntau; ++c)
        if (c == ntau - 1 || tp[c] <= hi_limit) return {c, tp[c]};
    return {ntau - 1, tp[ntau - 1]};
}

static std::vector<torch::Tensor> compact_finish(
    torch::Tensor t, double tau, const CompactGeom& g, torch::Tensor counts,
    int chosen, int64_t total) {
    const int nw = g.nblocks * 4;  // WAVES_PER_BLOCK
    auto idx = torch::empty({total}, t.options().dtype(torch::kInt32));
    auto val = torch::empty({total}, t.options());
    if (total > 0) {
        auto offs = torch::empty({nw}, t.options().dtype(torch::kInt32));
        launch_scan_offsets(counts.data_ptr<int>() + (int64_t)chosen * nw, nw,
                            offs.data_ptr<int>(), cur_stream());
        launch_compact_write(t.data_ptr<float>(), t.numel(), (float)tau, g.chunk,
                             g.nblocks, offs.data_ptr<int>(),
                             idx.data_ptr<int32_t>(), val.data_ptr<float>(),
                             cur_stream());
    }
    return {idx, val};
}

static std::vector<torch::Tensor> compact_gt(torch::Tensor t, double tau) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    int64_t n = t.numel();
    auto g = compact_geom(n);
    auto counts = torch::empty({g.nblocks * 4}, t.options().dtype(torch::kInt32));
    float tf = (float)tau;
    launch_compact_count_multi(t.data_ptr<float>(), n, &tf, 1, g.chunk, g.nblocks,
                               counts.data_ptr<int>(), cur_stream());
    auto b = bump_choose(counts, 1, g.nblocks * 4, n);
    return compact_finish(t, tau, g, counts, 0, b.total);
}

// Fused adaptive-threshold compaction: ONE pass counts all candidate taus
// per block; host applies the bump rule (smallest i with count <= hi_limit,
// reference add2residual VGG/compression.py:384-404); write pass extracts at
// the chosen tau.  Returns {idx, val, chosen_index, chosen_count}.
static std::vector<torch::Tensor> compact_adaptive(
    torch::Tensor t, std::vector<double> taus, int64_t hi_limit) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    TORCH_CHECK(taus.size() >= 1 && taus.size() <= 8, "1..8 thresholds");
    int ntau = (int)taus.size();
    int64_t n = t.numel();
    auto g = compact_geom(n);
    float tf[8];
    for (int j = 0; j < ntau; ++j) tf[j] = (float)taus[j];
    const int nw = g.nblocks * 4;
    auto counts = torch::empty({(int64_t)ntau * nw},
                               t.options().dtype(torch::kInt32));
    launch_compact_count_multi(t.data_ptr<float>(), n, tf, ntau, g.chunk, g.nblocks,
                               counts.data_ptr<int>(), cur_stream());
    auto b = bump_choose(counts, ntau, nw, hi_limit);
    auto out = compact_finish(t, taus[b.chosen], g, counts, b.chosen, b.total);
    out.push_back(torch::tensor((int64_t)b.chosen));
    out.push_back(torch::tensor(b.total));
    return out;
}

// fused EF restore + adaptive compaction: one streaming pass performs
//   t = float(grad_bf16) + residual (or t += residual), residual = t
// and counts every candidate tau (compact pass A layout); then the usual
// host bump rule + write pass.  Steady-state oktopk selection drops from
// three tensor-scale passes (EF, count, write) to two.
static std::vector<torch::Tensor> compact_adaptive_ef(
    torch::Tensor t, torch::Tensor residual, c10::optional<torch::Tensor> grad,
    std::vector<double> taus, int64_t hi_limit) {
    check_f32_1d(t, "t");
    check_f32_1d(residual, "residual");
    TORCH_CHECK(residual.numel() == t.numel(), "residual size mismatch");
    const at::cuda::CUDAGuard guard(t.device());
    TORCH_CHECK(taus.size() >= 1 && taus.size() <= 8, "1..8 thresholds");
    const void* gp = nullptr;
    if (grad.has_value()) {
        auto& gt = grad.value();
        TORCH_CHECK(gt.scalar_type() == torch::kBFloat16 && gt.is_contiguous() &&
                        gt.numel() == t.numel(),
                    "grad must be contiguous bf16 of same numel");
        gp = gt.data_ptr();
    }
    TORCH_CHECK((((uintptr_t)t.data_ptr() | (uintptr_t)residual.data_ptr() |
                  (uintptr_t)gp) & 15) == 0,
                "compact_adaptive_ef requires 16B-aligned buffers");
    int ntau = (int)taus.size();
    int64_t n = t.numel();
    auto g = compact_geom(n);
    float tf[8];
    for (int j = 0; j < ntau; ++j) tf[j] = (float)taus[j];
    const int nw = g.nblocks * 4;
    auto counts = torch::empty({(int64_t)ntau * nw},
                               t.options().dtype(torch::kInt32));
    launch_ef_count(t.data_ptr<float>(), residual.data_ptr<float>(), gp, n, tf,
                    ntau, g.chunk, g.nblocks, counts.data_ptr<int>(),
                    cur_stream());
    auto b = bump_choose(counts, ntau, nw, hi_limit);
    // pass B compacts from the residual SNAPSHOT (= the restored values);
    // t is left untouched — the callers densify into it afterwards anyway
    auto out = compact_finish(residual, taus[b.chosen], g, counts, b.chosen,
                              b.total);
    out.push_back(torch::tensor((int64_t)b.chosen));
    out.push_back(torch::tensor(b.total));
    return out;
}

// Device-resident Gaussian-k selection (gauss_select.hip): EF restore (+bf16
// upcast) with fused fp64 moments, on-device normal quantile + candidate
// table, one 10-candidate count pass, on-device refine-tree walk, then the
// usual compact write from the residual snapshot.  One 48-byte readback.
// Returns (idx, val, chosen, count, tau, tau0, mean, std).
static std::tuple<torch::Tensor, torch::Tensor, int64_t, int64_t, double,
                  double, double, double>
gaussian_select_ef(torch::Tensor t, torch::Tensor residual,
                   c10::optional<torch::Tensor> grad, double density,
                   int64_t k) {
    check_f32_1d(t, "t");
    check_f32_1d(residual, "residual");
    TORCH_CHECK(residual.numel() == t.numel(), "residual size mismatch");
    TORCH_CHECK(density > 0.0 && density <= 1.0, "density must be in (0, 1]");
    TORCH_CHECK(k >= 1, "k must be >= 1");
    int64_t n = t.numel();
    TORCH_CHECK(n >= 1, "gaussian_select_ef on empty tensor");
    TORCH_CHECK(n < ((int64_t)1 << 31), "gaussian_select_ef needs n < 2^31");
    const at::cuda::CUDAGuard guard(t.device());
    const void* gp = nullptr;
    if (grad.has_value()) {
        auto& gt = grad.value();
        TORCH_CHECK(gt.is_cuda() && gt.scalar_type() == torch::kBFloat16 &&
                        gt.is_contiguous() && gt.numel() == n,
                    "grad must be contiguous GPU bf16 of same numel");
        gp = gt.data_ptr();
    }
    auto g = compact_geom(n);
    const int nw = g.nblocks * 4;
    auto f64 = t.options().dtype(torch::kFloat64);
    auto partials = torch::empty({(int64_t)3 * nw}, f64);
    auto rec = torch::empty({6}, f64);
    auto cand = torch::empty({10}, t.options());
    auto counts = torch::empty({(int64_t)10 * nw},
                               t.options().dtype(torch::kInt32));
    // upper-tail mass of the quantile 1 - density/2, formed the way the
    // host path forms its ppf argument
    const double q = 1.0 - (1.0 - density / 2.0);
    auto stream = cur_stream();
    launch_gauss_moments(t.data_ptr<float>(), residual.data_ptr<float>(), gp, n,
                         g.chunk, g.nblocks, partials.data_ptr<double>(),
                         stream);
    launch_gauss_finalize(partials.data_ptr<double>(), nw, n, q,
                          cand.data_ptr<float>(), rec.data_ptr<double>(),
                          stream);
    launch_gauss_count(residual.data_ptr<float>(), n, cand.data_ptr<float>(),
                       g.chunk, g.nblocks, counts.data_ptr<int>(), stream);
    launch_gauss_decide(counts.data_ptr<int>(), nw, k, cand.data_ptr<float>(),
                        rec.data_ptr<double>(), stream);
    auto rh = rec.cpu();
    const double* rp = rh.data_ptr<double>();
    int chosen = (int)rp[0];
    int64_t total = (int64_t)rp[1];
    double tau = rp[2];
    auto out = compact_finish(residual, tau, g, counts, chosen, total);
    return std::make_tuple(out[0], out[1], (int64_t)chosen, total, tau, rp[3],
                           rp[4], rp[5]);
}

// Exact-k select over `len` 32-bit words (topk_select.hip): fp32 values
// keyed by |x| bits, or ready-made keys (keymode).  `hist` holds level 1's
// bins when the caller's fused pass already counted them (level1_done).
// Every launch reads tau / need from the device state record; nothing is
// read back here.  Fills out_idx / out_val (kout entries, ascending).
// With `r2` the write pass is the round-2 tail's (round2_tail.hip): it emits
// (all_idx[pos], words[pos]) and credits the residual at the entries that
// the local selection also holds.
struct R2Write {
    const int32_t* all_idx;
    const int32_t* idx;
    int m;
    float* residual;
    int64_t n;
};

static torch::Tensor tk_select_run(const void* words, int64_t len, int64_t kout,
                                   bool keymode, float* zero_dst,
                                   const int32_t* uidx, const float* uval,
                                   torch::Tensor hist, bool level1_done,
                                   torch::Tensor& out_idx,
                                   torch::Tensor& out_val,
                                   const R2Write* r2 = nullptr) {
    auto i32 = hist.options().dtype(torch::kInt32);
    auto state = torch::empty({4}, i32);
    auto* sp = reinterpret_cast<uint32_t*>(state.data_ptr<int>());
    auto* hp = reinterpret_cast<unsigned int*>(hist.data_ptr<int>());
    auto stream = cur_stream();
    const int shifts[3] = {21, 10, 0};
    const int nbins[3] = {2048, 2048, 1024};
    for (int lvl = 0; lvl < 3; ++lvl) {
        if (!(lvl == 0 && level1_done))
            launch_tk_hist(words, len, keymode, sp, lvl == 0, shifts[lvl],
                           nbins[lvl], hp, stream);
        launch_tk_pick(hp, nbins[lvl], shifts[lvl], sp, (uint32_t)kout,
                       lvl == 0, stream);
    }
    auto g = compact_geom(len);
    const int nw = g.nblocks * 4;
    auto counts = torch::empty({(int64_t)2 * nw}, i32);
    auto offs = torch::empty({(int64_t)2 * nw}, i32);
    launch_tk_count(words, len, keymode, g.chunk, g.nblocks, sp,
                    counts.data_ptr<int>(), stream);
    launch_scan_offsets(counts.data_ptr<int>(), nw, offs.data_ptr<int>(), stream);
    launch_scan_offsets(counts.data_ptr<int>() + nw, nw,
                        offs.data_ptr<int>() + nw, stream);
    if (r2 != nullptr)
        launch_r2_write(words, r2->all_idx, len, g.chunk, g.nblocks, sp,
                        offs.data_ptr<int>(), offs.data_ptr<int>() + nw,
                        r2->idx, r2->m, r2->residual, r2->n,
                        out_idx.data_ptr<int32_t>(), out_val.data_ptr<float>(),
                        (int)kout, stream);
    else
        launch_tk_write(words, zero_dst, len, keymode, g.chunk, g.nblocks, sp,
                        offs.data_ptr<int>(), offs.data_ptr<int>() + nw, uidx,
                        uval, out_idx.data_ptr<int32_t>(),
                        out_val.data_ptr<float>(), (int)kout, stream);
    return state;
}

static double tk_state_tau(const torch::Tensor& state) {
    auto sh = state.cpu();
    union { uint32_t u; float f; } c;
    c.u = (uint32_t)sh.data_ptr<int>()[0];
    return (double)c.f;
}

// Exact top-k by magnitude with the lowest-index tie rule; returns (idx
// int32 ascending, val, tau).  Writes nothing but its outputs.
static std::tuple<torch::Tensor, torch::Tensor, double> topk_select(
    torch::Tensor t, int64_t k) {
    check_f32_1d(t, "t");
    int64_t n = t.numel();
    TORCH_CHECK(k >= 1, "k must be >= 1");
    TORCH_CHECK(n >= 1, "topk_select on empty tensor");
    TORCH_CHECK(n < ((int64_t)1 << 31), "topk_select needs n < 2^31");
    const at::cuda::CUDAGuard guard(t.device());
    int64_t kout = k < n ? k : n;
    auto idx = torch::empty({kout}, t.options().dtype(torch::kInt32));
    auto val = torch::empty({kout}, t.options());
    auto hist = torch::zeros({2048}, t.options().dtype(torch::kInt32));
    auto state = tk_select_run(t.data_ptr<float>(), n, kout, false, nullptr,
                               nullptr, nullptr, hist, false, idx, val);
    return std::make_tuple(idx, val, tk_state_tau(state));
}

// topk_select over restored = float(grad) + residual (or t + residual),
// with the EF restore fused into the first histogram level and the residual
// zeroed at the selection by the write pass.  t is not written.
static std::tuple<torch::Tensor, torch::Tensor, double> topk_select_ef(
    torch::Tensor t, torch::Tensor residual, c10::optional<torch::Tensor> grad,
    int64_t k) {
    check_f32_1d(t, "t");
    check_f32_1d(residual, "residual");
    int64_t n = t.numel();
    TORCH_CHECK(residual.numel() == n, "residual size mismatch");
    TORCH_CHECK(residual.device() == t.device(), "residual device mismatch");
    TORCH_CHECK(k >= 1, "k must be >= 1");
    TORCH_CHECK(n >= 1, "topk_select_ef on empty tensor");
    TORCH_CHECK(n < ((int64_t)1 << 31), "topk_select_ef needs n < 2^31");
    const at::cuda::CUDAGuard guard(t.device());
    const void* gp = nullptr;
    if (grad.has_value()) {
        auto& gt = grad.value();
        TORCH_CHECK(gt.is_cuda() && gt.device() == t.device() &&
                        gt.scalar_type() == torch::kBFloat16 &&
                        gt.is_contiguous() && gt.numel() == n,
                    "grad must be contiguous GPU bf16 of same numel");
        gp = gt.data_ptr();
    }
    int64_t kout = k < n ? k : n;
    auto idx = torch::empty({kout}, t.options().dtype(torch::kInt32));
    auto val = torch::empty({kout}, t.options());
    auto hist = torch::zeros({2048}, t.options().dtype(torch::kInt32));
    float* rp = residual.data_ptr<float>();
    launch_tk_ef_hist(t.data_ptr<float>(), rp, gp, n,
                      reinterpret_cast<unsigned int*>(hist.data_ptr<int>()),
                      cur_stream());
    auto state = tk_select_run(rp, n, kout, false, rp, nullptr, nullptr, hist,
                               true, idx, val);
    return std::make_tuple(idx, val, tk_state_tau(state));
}

// Top-k of the sum of two sparse vectors (ascending unique indices): slot
// layout + the same exact-k select over the slot keys.  Sized by
// |a| + |b| only.  One 4-byte readback (the duplicate count), and none when
// one list alone already holds k entries.
static std::vector<torch::Tensor> sparse_merge_topk(
    torch::Tensor a_idx, torch::Tensor a_val, torch::Tensor b_idx,
    torch::Tensor b_val, int64_t k) {
    check_i32_1d(a_idx, "a_idx");
    check_f32_1d(a_val, "a_val");
    check_i32_1d(b_idx, "b_idx");
    check_f32_1d(b_val, "b_val");
    TORCH_CHECK(a_idx.numel() == a_val.numel() && b_idx.numel() == b_val.numel(),
                "idx / val length mismatch");
    TORCH_CHECK(a_idx.device() == a_val.device() &&
                    b_idx.device() == a_val.device() &&
                    b_val.device() == a_val.device(),
                "sparse_merge_topk: device mismatch");
    TORCH_CHECK(k >= 1, "k must be >= 1");
    int64_t na = a_idx.numel(), nb = b_idx.numel();
    int64_t total = na + nb;
    TORCH_CHECK(total < ((int64_t)1 << 31), "sparse_merge_topk: lists too long");
    const at::cuda::CUDAGuard guard(a_val.device());
    auto i32 = a_val.options().dtype(torch::kInt32);
    if (total == 0)
        return {torch::empty({0}, i32), torch::empty({0}, a_val.options())};
    auto ukey = torch::empty({total}, i32);
    auto uidx = torch::empty({total}, i32);
    auto uval = torch::empty({total}, a_val.options());
    // [0, 2048) histogram bins, [2048] duplicate count
    auto work = torch::zeros({2049}, i32);
    launch_tk_merge_slots(a_idx.data_ptr<int32_t>(), a_val.data_ptr<float>(),
                          (int)na, b_idx.data_ptr<int32_t>(),
                          b_val.data_ptr<float>(), (int)nb,
                          reinterpret_cast<uint32_t*>(ukey.data_ptr<int>()),
                          uidx.data_ptr<int32_t>(), uval.data_ptr<float>(),
                          work.data_ptr<int>() + 2048, cur_stream());
    int64_t kout = k;
    if (k > (na > nb ? na : nb)) {  // the union may be smaller than k
        int64_t m = total - work.narrow(0, 2048, 1).cpu().item<int>();
        kout = k < m ? k : m;
    }
    auto idx = torch::empty({kout}, i32);
    auto val = torch::empty({kout}, a_val.options());
    tk_select_run(ukey.data_ptr<int>(), total, kout, true, nullptr,
                  uidx.data_ptr<int32_t>(), uval.data_ptr<float>(),
                  work.narrow(0, 0, 2048), false, idx, val);
    return {idx, val};
}

static double kth_abs_value(torch::Tensor t, int64_t k) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    int64_t n = t.numel();
    TORCH_CHECK(n > 0, "kth_abs_value on empty tensor");
    if (k < 1) k = 1;
    if (k > n) k = n;
    // 3 histogram levels over |x| bits: 11 + 11 + 10
    const int shifts[3] = {21, 10, 0};
    const int bits[3] = {11, 11, 10};
    uint32_t prefix_mask = 0, prefix_val = 0;
    int64_t remaining = k;
    auto hist = torch::empty({2048}, t.options().dtype(torch::kInt32));
    for (int lvl = 0; lvl < 3; ++lvl) {
        int nbins = 1 << bits[lvl];
        hist.zero_();
        launch_hist(t.data_ptr<float>(), n, prefix_mask, prefix_val, shifts[lvl], nbins,
                    reinterpret_cast<unsigned int*>(hist.data_ptr<int>()), cur_stream());
        auto h = hist.narrow(0, 0, nbins).cpu();
        const int* hp = h.data_ptr<int>();
        int64_t b = nbins - 1;
        for (; b >= 0; --b) {
            if (remaining <= hp[b]) break;
            remaining -= hp[b];
        }
        if (b < 0) b = 0;  // fewer matching elements than k (ties/degenerate)
        prefix_val |= ((uint32_t)b) << shifts[lvl];
        prefix_mask |= ((uint32_t)(nbins - 1)) << shifts[lvl];
    }
    union { uint32_t u; float f; } c;
    c.u = prefix_val;
    return (double)c.f;
}

static torch::Tensor scatter_add_(torch::Tensor dest, torch::Tensor idx,
                                  torch::Tensor val) {
    check_f32_1d(dest, "dest");
    check_f32_1d(val, "val");
    check_i32_1d(idx, "idx");
    const at::cuda::CUDAGuard guard(dest.device());
    TORCH_CHECK(idx.numel() == val.numel(), "idx/val size mismatch");
    if (idx.numel())
        launch_scatter_add(dest.data_ptr<float>(), idx.data_ptr<int32_t>(),
                           val.data_ptr<float>(), idx.numel(), cur_stream());
    return dest;
}

static torch::Tensor zero_at_(torch::Tensor t, torch::Tensor idx) {
    check_f32_1d(t, "t");
    check_i32_1d(idx, "idx");
    const at::cuda::CUDAGuard guard(t.device());
    if (idx.numel())
        launch_zero_at(t.data_ptr<float>(), idx.data_ptr<int32_t>(), idx.numel(),
                       cur_stream());
    return t;
}

static torch::Tensor zero_at_masked_(torch::Tensor t, torch::Tensor idx,
                                     torch::Tensor mask) {
    check_f32_1d(t, "t");
    check_i32_1d(idx, "idx");
    TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kBool &&
                mask.is_contiguous(), "mask must be contiguous bool on GPU");
    const at::cuda::CUDAGuard guard(t.device());
    if (idx.numel())
        launch_zero_at_masked(t.data_ptr<float>(), idx.data_ptr<int32_t>(),
                              mask.data_ptr<bool>(), idx.numel(), cur_stream());
    return t;
}

static torch::Tensor fill_sparse_scaled_(torch::Tensor out, torch::Tensor idx,
                                         torch::Tensor val, double scale) {
    check_f32_1d(out, "out");
    check_i32_1d(idx, "idx");
    check_f32_1d(val, "val");
    const at::cuda::CUDAGuard guard(out.device());
    out.zero_();
    if (idx.numel())
        launch_scatter_set_scaled(out.data_ptr<float>(), idx.data_ptr<int32_t>(),
                                  val.data_ptr<float>(), (float)scale, idx.numel(),
                                  cur_stream());
    return out;
}

static torch::Tensor isin_sorted(torch::Tensor a, torch::Tensor b_sorted) {
    check_i32_1d(a, "a");
    check_i32_1d(b_sorted, "b_sorted");
    const at::cuda::CUDAGuard guard(a.device());
    auto out = torch::zeros({a.numel()}, a.options().dtype(torch::kBool));
    if (a.numel() && b_sorted.numel())
        launch_isin_sorted(a.data_ptr<int32_t>(), a.numel(),
                           b_sorted.data_ptr<int32_t>(), b_sorted.numel(),
                           out.data_ptr<bool>(), cur_stream());
    return out;
}

static torch::Tensor ef_restore_snapshot_(torch::Tensor t, torch::Tensor r) {
    check_f32_1d(t, "t");
    check_f32_1d(r, "r");
    const at::cuda::CUDAGuard guard(t.device());
    TORCH_CHECK(t.numel() == r.numel(), "t/r size mismatch");
    launch_ef_restore(t.data_ptr<float>(), r.data_ptr<float>(), t.numel(), cur_stream());
    return t;
}

static torch::Tensor ef_restore_upcast_(torch::Tensor t, torch::Tensor r,
                                        torch::Tensor g) {
    check_f32_1d(t, "t");
    check_f32_1d(r, "r");
    TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kBFloat16 && g.is_contiguous(),
                "g must be contiguous bf16 on GPU");
    TORCH_CHECK(t.numel() == r.numel() && t.numel() == g.numel());
    const at::cuda::CUDAGuard guard(t.device());
    launch_ef_upcast(t.data_ptr<float>(), r.data_ptr<float>(), g.data_ptr(),
                     t.numel(), cur_stream());
    return t;
}

static void fused_sgd_(torch::Tensor p, torch::Tensor g, torch::Tensor buf, double lr,
                       double momentum, double wd, bool nesterov) {
    check_f32_1d(p, "p");
    check_f32_1d(g, "g");
    check_f32_1d(buf, "buf");
    const at::cuda::CUDAGuard guard(p.device());
    launch_sgd(p.data_ptr<float>(), g.data_ptr<float>(), buf.data_ptr<float>(),
               p.numel(), (float)lr, (float)momentum, (float)wd, nesterov ? 1 : 0,
               cur_stream());
}

static const float* gscale_ptr(const c10::optional<torch::Tensor>& gs) {
    if (!gs.has_value() || !gs->defined() || gs->numel() == 0) return nullptr;
    TORCH_CHECK(gs->scalar_type() == torch::kFloat32 && gs->is_cuda() &&
                gs->numel() == 1, "gscale must be a 1-elem cuda float tensor");
    return gs->data_ptr<float>();
}

static void fused_adam_(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                        torch::Tensor v, double lr, double b1, double b2,
                        double eps, double wd,
                        c10::optional<torch::Tensor> gscale) {
    check_f32_1d(p, "p");
    check_f32_1d(g, "g");
    check_f32_1d(m, "m");
    check_f32_1d(v, "v");
    const at::cuda::CUDAGuard guard(p.device());
    launch_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                v.data_ptr<float>(), nullptr, gscale_ptr(gscale), p.numel(),
                (float)lr, (float)b1, (float)b2, (float)eps, (float)wd,
                cur_stream());
}

static void fused_adam_mirror_(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                               torch::Tensor v, torch::Tensor p_bf16, double lr,
                               double b1, double b2, double eps, double wd,
                               c10::optional<torch::Tensor> gscale) {
    check_f32_1d(p, "p");
    check_f32_1d(g, "g");
    check_f32_1d(m, "m");
    check_f32_1d(v, "v");
    TORCH_CHECK(p_bf16.scalar_type() == torch::kBFloat16 && p_bf16.is_contiguous() &&
                p_bf16.numel() == p.numel());
    const at::cuda::CUDAGuard guard(p.device());
    launch_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                v.data_ptr<float>(), p_bf16.data_ptr(), gscale_ptr(gscale),
                p.numel(), (float)lr, (float)b1, (float)b2, (float)eps,
                (float)wd, cur_stream());
}

static int64_t scatter_gt_credit_(torch::Tensor result,
                                  torch::Tensor residual, torch::Tensor idx,
                                  torch::Tensor val, double tau,
                                  double scale) {
    // result must arrive ZEROED; returns the number of scattered entries
    check_f32_1d(result, "result");
    check_f32_1d(residual, "residual");
    check_f32_1d(val, "val");
    TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous());
    const at::cuda::CUDAGuard guard(result.device());
    auto cnt = torch::zeros({1}, result.options().dtype(torch::kInt64));
    launch_scatter_gt_credit(idx.data_ptr<int32_t>(), val.data_ptr<float>(),
                             idx.numel(), (float)tau, (float)scale,
                             result.data_ptr<float>(),
                             residual.data_ptr<float>(),
                             (unsigned long long*)cnt.data_ptr<int64_t>(),
                             cur_stream());
    return cnt.cpu().item<int64_t>();
}

static torch::Tensor grad_clip_scale(torch::Tensor t, double max_norm) {
    // device-resident clip factor: scale = max/(||t||+1e-6) if ||t||>max
    // else 1 — no host sync (reference clips via a host norm check,
    // BERT/.../optimization.py:197)
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    auto ss = torch::zeros({1}, t.options().dtype(torch::kFloat64));
    launch_sumsq(t.data_ptr<float>(), t.numel(), ss.data_ptr<double>(),
                 cur_stream());
    auto out = torch::empty({1}, t.options());
    launch_clip_scale(ss.data_ptr<double>(), (float)max_norm,
                      out.data_ptr<float>(), cur_stream());
    return out;
}

// -- sparse optimizer tail (kernels.hip, "sparse optimizer tail") -----------

static void check_sparse_grad(const torch::Tensor& idx, const torch::Tensor& val) {
    check_i32_1d(idx, "idx");
    check_f32_1d(val, "val");
    TORCH_CHECK(idx.numel() == val.numel(), "idx / val length mismatch");
    TORCH_CHECK(idx.numel() < (int64_t)INT32_MAX, "selection too large");
}

static int64_t credit_gt_(torch::Tensor residual, torch::Tensor idx,
                          torch::Tensor val, double tau) {
    // scatter_gt_credit_ without the dense result: residual credit + count
    check_f32_1d(residual, "residual");
    check_sparse_grad(idx, val);
    const at::cuda::CUDAGuard guard(residual.device());
    auto cnt = torch::zeros({1}, residual.options().dtype(torch::kInt64));
    launch_scatter_gt_credit(idx.data_ptr<int32_t>(), val.data_ptr<float>(),
                             idx.numel(), (float)tau, 1.f, nullptr,
                             residual.data_ptr<float>(),
                             (unsigned long long*)cnt.data_ptr<int64_t>(),
                             cur_stream());
    return cnt.cpu().item<int64_t>();
}

static void sparse_sumsq_into_(torch::Tensor acc, torch::Tensor idx,
                               torch::Tensor val, double scale, double tau) {
    // sumsq_into_ of the dense gradient a sparse one stands for
    check_sparse_grad(idx, val);
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == torch::kFloat64 &&
                acc.numel() == 1 && acc.device() == val.device(),
                "acc must be a 1-elem fp64 tensor on val's device");
    const at::cuda::CUDAGuard guard(val.device());
    launch_sparse_sumsq(val.data_ptr<float>(), val.numel(), (float)scale,
                        (float)tau, acc.data_ptr<double>(), cur_stream());
}

static torch::Tensor grad_clip_scale_sparse(torch::Tensor idx, torch::Tensor val,
                                            double scale, double tau,
                                            double max_norm) {
    // grad_clip_scale of the dense gradient a sparse one stands for: fp64
    // sum over the kept entries, then the same clip_scale kernel; no sync
    check_sparse_grad(idx, val);
    const at::cuda::CUDAGuard guard(val.device());
    auto ss = torch::zeros({1}, val.options().dtype(torch::kFloat64));
    launch_sparse_sumsq(val.data_ptr<float>(), val.numel(), (float)scale,
                        (float)tau, ss.data_ptr<double>(), cur_stream());
    auto out = torch::empty({1}, val.options());
    launch_clip_scale(ss.data_ptr<double>(), (float)max_norm,
                      out.data_ptr<float>(), cur_stream());
    return out;
}

static void adam_sparse_impl(torch::Tensor& p, torch::Tensor& idx,
                             torch::Tensor& val, int64_t base, double scale,
                             double tau, torch::Tensor& m, torch::Tensor& v,
                             void* p_bf16, double lr, double b1, double b2,
                             double eps, double wd,
                             const c10::optional<torch::Tensor>& gscale) {
    check_f32_1d(p, "p");
    check_f32_1d(m, "m");
    check_f32_1d(v, "v");
    check_sparse_grad(idx, val);
    TORCH_CHECK(m.numel() == p.numel() && v.numel() == p.numel(),
                "p / m / v length mismatch");
    TORCH_CHECK(base >= 0, "base must be >= 0");
    const at::cuda::CUDAGuard guard(p.device());
    auto tile_start = torch::empty({adam_sparse_ntiles(p.numel()) + 1},
                                   idx.options());
    launch_adam_sparse(p.data_ptr<float>(), m.data_ptr<float>(),
                       v.data_ptr<float>(), p_bf16, gscale_ptr(gscale),
                       p.numel(), idx.data_ptr<int32_t>(), val.data_ptr<float>(),
                       idx.numel(), tile_start.data_ptr<int32_t>(), base,
                       (float)scale, (float)tau, (float)lr, (float)b1,
                       (float)b2, (float)eps, (float)wd, cur_stream());
}

static void fused_adam_sparse_(torch::Tensor p, torch::Tensor idx,
                               torch::Tensor val, int64_t base, double scale,
                               double tau, torch::Tensor m, torch::Tensor v,
                               double lr, double b1, double b2, double eps,
                               double wd, c10::optional<torch::Tensor> gscale) {
    adam_sparse_impl(p, idx, val, base, scale, tau, m, v, nullptr, lr, b1, b2,
                     eps, wd, gscale);
}

static void fused_adam_sparse_mirror_(torch::Tensor p, torch::Tensor idx,
                                      torch::Tensor val, int64_t base,
                                      double scale, double tau, torch::Tensor m,
                                      torch::Tensor v, torch::Tensor p_bf16,
                                      double lr, double b1, double b2,
                                      double eps, double wd,
                                      c10::optional<torch::Tensor> gscale) {
    TORCH_CHECK(p_bf16.is_cuda() && p_bf16.scalar_type() == torch::kBFloat16 &&
                p_bf16.is_contiguous() && p_bf16.numel() == p.numel(),
                "p_bf16: contiguous cuda bf16 of p's length");
    adam_sparse_impl(p, idx, val, base, scale, tau, m, v, p_bf16.data_ptr(), lr,
                     b1, b2, eps, wd, gscale);
}

// -- flat SGD (kernels.hip, "flat SGD") --------------------------------------

static float* sgd_buf_ptr(const torch::Tensor& p, const torch::Tensor& buf,
                          double momentum) {
    // buf is untouched without momentum and may then be empty
    if (momentum == 0.0) return nullptr;
    check_f32_1d(buf, "buf");
    TORCH_CHECK(buf.numel() == p.numel() && buf.device() == p.device(),
                "buf must have p's length and device");
    return buf.data_ptr<float>();
}

static void sgd_step_(torch::Tensor p, torch::Tensor g, torch::Tensor buf,
                      double lr, double momentum, double wd, bool nesterov,
                      c10::optional<torch::Tensor> gscale) {
    check_f32_1d(p, "p");
    check_f32_1d(g, "g");
    TORCH_CHECK(g.numel() == p.numel() && g.device() == p.device(),
                "g must have p's length and device");
    float* bp = sgd_buf_ptr(p, buf, momentum);
    const at::cuda::CUDAGuard guard(p.device());
    launch_sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), bp,
                    gscale_ptr(gscale), p.numel(), (float)lr, (float)momentum,
                    (float)wd, nesterov ? 1 : 0, cur_stream());
}

static void sgd_step_sparse_(torch::Tensor p, torch::Tensor idx,
                             torch::Tensor val, int64_t base, double scale,
                             double tau, torch::Tensor buf, double lr,
                             double momentum, double wd, bool nesterov,
                             c10::optional<torch::Tensor> gscale) {
    check_f32_1d(p, "p");
    check_sparse_grad(idx, val);
    TORCH_CHECK(idx.device() == p.device() && val.device() == p.device(),
                "idx / val must be on p's device");
    TORCH_CHECK(base >= 0, "base must be >= 0");
    float* bp = sgd_buf_ptr(p, buf, momentum);
    const at::cuda::CUDAGuard guard(p.device());
    auto tile_start = torch::empty({adam_sparse_ntiles(p.numel()) + 1},
                                   idx.options());
    launch_sgd_step_sparse(p.data_ptr<float>(), bp, gscale_ptr(gscale),
                           p.numel(), idx.data_ptr<int32_t>(),
                           val.data_ptr<float>(), idx.numel(),
                           tile_start.data_ptr<int32_t>(), base, (float)scale,
                           (float)tau, (float)lr, (float)momentum, (float)wd,
                           nesterov ? 1 : 0, cur_stream());
}

static torch::Tensor clip_scale_from_sumsq(torch::Tensor acc, double max_norm) {
    // the clip factor of grad_clip_scale from an already accumulated fp64
    // sum of squares (sumsq_into_ / sparse_sumsq_into_); no host sync
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == torch::kFloat64 &&
                acc.numel() == 1, "acc must be a 1-elem cuda fp64 tensor");
    const at::cuda::CUDAGuard guard(acc.device());
    auto out = torch::empty({1}, acc.options().dtype(torch::kFloat32));
    launch_clip_scale(acc.data_ptr<double>(), (float)max_norm,
                      out.data_ptr<float>(), cur_stream());
    return out;
}

static void colsum_bf16_into(torch::Tensor gy, torch::Tensor dst,
                             bool accumulate) {
    // bias gradient: dst[C] (=|+=) sum over all leading dims of a bf16
    // [..., C] tensor.  One launch; fp32 accumulation, no atomics; dst may
    // start at any element offset of a larger buffer.
    TORCH_CHECK(gy.is_cuda() && gy.scalar_type() == torch::kBFloat16 &&
                gy.is_contiguous() && gy.dim() >= 1, "gy: contiguous cuda bf16");
    TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kBFloat16 &&
                dst.is_contiguous() && dst.device() == gy.device(),
                "dst: contiguous cuda bf16 on gy's device");
    int64_t C = gy.size(-1);
    TORCH_CHECK(dst.numel() == C, "dst must hold gy.size(-1) elements");
    if (C == 0) return;
    int64_t R = gy.numel() / C;
    const at::cuda::CUDAGuard guard(gy.device());
    launch_colsum_into_bf16(gy.data_ptr(), R, C, dst.data_ptr(),
                            accumulate ? 1 : 0, cur_stream());
}

static py::object colsum_exact_config(int64_t R, int64_t C, int64_t src_addr,
                                      int64_t num_mp, int64_t max_threads_per_mp,
                                      int64_t warp_size) {
    // the port of torch's reduce configuration, for tests and tools:
    // (V, bw, bh, split, ctas), or None where it is unsupported
    auto cfg = colsum_exact::derive(R, C, (uint64_t)src_addr, (int)num_mp,
                                    (int)max_threads_per_mp, (int)warp_size);
    if (!cfg.supported) return py::none();
    return py::make_tuple(cfg.V, cfg.bw, cfg.bh, cfg.split, cfg.ctas);
}

static bool colsum_bf16_into_exact(torch::Tensor gy, torch::Tensor dst,
                                   bool accumulate) {
    // dst[C] = column sum of a contiguous bf16 [R, C], summed in the order
    // of at::sum_out(dst, gy, {0}) on this device, so it leaves the same
    // bits.  One launch.  False: this shape / address / device is outside
    // the ported family, and nothing was written.
    //
    // accumulate is always unsupported.  The form to match would be
    // dst.add_(at::sum(gy, {0}, false, kFloat)); the fp32 sum has the same
    // order, but torch's bf16 += fp32 add is not one function of its
    // operands: measured on MI355X (torch 2.10), [768 .. 15000] elements give
    // bf16(float(dst) + s), while [30520] and [30522] give
    // bf16(float(dst) + float(bf16(s))), 124 of 30522 elements apart.  That
    // switch lies in the elementwise kernels, not in the reduction, so the
    // accumulating caller keeps torch's two calls.  The captured fwd+bwd
    // only ever overwrites.
    TORCH_CHECK(gy.is_cuda() && gy.scalar_type() == torch::kBFloat16 &&
                gy.dim() == 2, "gy: cuda bf16 [R, C]");
    TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kBFloat16 &&
                dst.is_contiguous() && dst.device() == gy.device() &&
                dst.numel() == gy.size(1),
                "dst: contiguous cuda bf16 [C] on gy's device");
    if (accumulate || !gy.is_contiguous()) return false;
    const int64_t R = gy.size(0), C = gy.size(1);
    const at::cuda::CUDAGuard guard(gy.device());
    const auto* prop = at::cuda::getCurrentDeviceProperties();
    auto cfg = colsum_exact::derive(R, C, (uint64_t)(uintptr_t)gy.data_ptr(),
                                    prop->multiProcessorCount,
                                    prop->maxThreadsPerMultiProcessor,
                                    at::cuda::warp_size());
    if (!cfg.supported) return false;
    return launch_colsum_exact_bf16(gy.data_ptr(), R, C, dst.data_ptr(),
                                    cfg.split ? cfg.bh : 1, cfg.ctas,
                                    cur_stream()) != 0;
}

static torch::Tensor linear_bwd_into(torch::Tensor gy, torch::Tensor x,
                                     torch::Tensor w,
                                     c10::optional<torch::Tensor> gw_dst,
                                     c10::optional<torch::Tensor> gb_dst,
                                     bool accumulate, bool bias_kernel,
                                     bool bias_exact) {
    // backward of y = x W^T + b with the parameter gradients written
    // straight into their slots: gW is the GEMM's own output (beta = 0, or
    // beta = 1 when accumulating) and gb a column reduction whose output is
    // the slot, so neither needs a temporary plus an add.  Both leave
    // exactly the bits autograd's zero + accumulate left: bias_exact runs
    // the one-launch column sum that follows torch's summation order where
    // it is supported and torch's reduction elsewhere.  bias_kernel (wins
    // over bias_exact) selects the older one-launch column sum, whose order
    // is its own.  Returns gx.
    TORCH_CHECK(gy.is_cuda() && gy.scalar_type() == torch::kBFloat16 &&
                x.scalar_type() == torch::kBFloat16 &&
                w.scalar_type() == torch::kBFloat16 && w.dim() == 2,
                "linear_bwd_into: cuda bf16 operands");
    const int64_t N = w.size(0), K = w.size(1);
    TORCH_CHECK(gy.size(-1) == N && x.size(-1) == K &&
                gy.numel() / std::max<int64_t>(N, 1) ==
                    x.numel() / std::max<int64_t>(K, 1),
                "linear_bwd_into: shape mismatch");
    const at::cuda::CUDAGuard guard(gy.device());
    at::NoGradGuard no_grad;
    auto gy2 = gy.contiguous().view({-1, N});
    auto x2 = x.reshape({-1, K});
    auto gx = at::mm(gy2, w).view(x.sizes());
    if (gw_dst.has_value()) {
        auto& gw = *gw_dst;
        TORCH_CHECK(gw.is_cuda() && gw.scalar_type() == torch::kBFloat16 &&
                    gw.is_contiguous() && gw.dim() == 2 && gw.size(0) == N &&
                    gw.size(1) == K, "gw_dst: contiguous bf16 [N, K]");
        if (accumulate) gw.addmm_(gy2.t(), x2);
        else at::mm_out(gw, gy2.t(), x2);
    }
    if (gb_dst.has_value()) {
        auto& gb = *gb_dst;
        if (bias_kernel) {
            // one launch of ours; sums in another order than torch's
            // reduction, so a rare element rounds to the neighbouring bf16
            colsum_bf16_into(gy2, gb, accumulate);
        } else if (bias_exact && colsum_bf16_into_exact(gy2, gb, accumulate)) {
            // one launch of ours, torch's bits
        } else {
            // torch's own column reduction with the slot as its output:
            // the bits autograd's `0 + sum` left there, minus the add
            TORCH_CHECK(gb.is_cuda() && gb.scalar_type() == torch::kBFloat16 &&
                        gb.is_contiguous() && gb.numel() == N,
                        "gb_dst: contiguous bf16 [N]");
            // accumulating: fp32 sum added in fp32, one rounding into the slot
            if (accumulate) gb.add_(at::sum(gy2, {0}, false, at::kFloat));
            else at::sum_out(gb, gy2, {0});
        }
    }
    return gx;
}

static torch::Tensor attn_rowdot(torch::Tensor go, torch::Tensor out,
                                 int64_t num_heads) {
    // D[bh, s] = sum_d go[b,s,h,d]*out[b,s,h,d]  (head_dim 64)
    TORCH_CHECK(go.is_cuda() && go.scalar_type() == torch::kBFloat16 &&
                go.is_contiguous() && out.is_contiguous() &&
                out.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(go.dim() == 3 && go.sizes() == out.sizes());
    int64_t B = go.size(0), S = go.size(1);
    TORCH_CHECK(go.size(2) == num_heads * 64, "head_dim must be 64");
    const at::cuda::CUDAGuard guard(go.device());
    auto d = torch::empty({B * num_heads, S},
                          go.options().dtype(torch::kFloat32));
    launch_attn_rowdot(go.data_ptr(), out.data_ptr(), B, S, num_heads,
                       d.data_ptr<float>(), cur_stream());
    return d;
}

static void sumsq_into_(torch::Tensor acc, torch::Tensor t) {
    // accumulate sum(t^2) into acc (fp64[1], device) — launch_sumsq's
    // atomicAdd accumulates, so repeated calls over buckets build the
    // global norm without any host sync
    check_f32_1d(t, "t");
    TORCH_CHECK(acc.scalar_type() == torch::kFloat64 && acc.is_cuda() &&
                acc.numel() == 1);
    const at::cuda::CUDAGuard guard(t.device());
    launch_sumsq(t.data_ptr<float>(), t.numel(), acc.data_ptr<double>(),
                 cur_stream());
}

static double l2norm(torch::Tensor t) {
    check_f32_1d(t, "t");
    const at::cuda::CUDAGuard guard(t.device());
    auto out = torch::zeros({1}, t.options().dtype(torch::kFloat64));
    launch_sumsq(t.data_ptr<float>(), t.numel(), out.data_ptr<double>(), cur_stream());
    return std::sqrt(out.cpu().item<double>());
}

// ---------------------------------------------------------------------------
// sparse wire codec (wire_codec.hip): [idx int32 | val bits] per segment,
// fp32 or bf16 values, segments in destination / rank order
// ---------------------------------------------------------------------------
static int64_t wire_words(int64_t c, bool bf16) {
    return bf16 ? c + (c + 1) / 2 : 2 * c;
}

// [element prefix | word prefix] of `counts` as one device int32 tensor;
// total elements / words come back through the out-params
static torch::Tensor wire_tables(const std::vector<int64_t>& counts, bool bf16,
                                 const torch::Tensor& like, int64_t* total_elems,
                                 int64_t* total_words) {
    const int64_t P = (int64_t)counts.size();
    TORCH_CHECK(P <= wire_max_segments(), "wire codec: at most ",
                wire_max_segments(), " segments, got ", P);
    auto host = torch::empty({2 * (P + 1)}, torch::dtype(torch::kInt32));
    int32_t* h = host.data_ptr<int32_t>();
    int64_t e = 0, w = 0;
    for (int64_t j = 0; j < P; ++j) {
        TORCH_CHECK(counts[j] >= 0, "wire codec: negative segment count");
        h[j] = (int32_t)e;
        h[P + 1 + j] = (int32_t)w;
        e += counts[j];
        w += wire_words(counts[j], bf16);
        TORCH_CHECK(w <= INT32_MAX, "wire codec: word count overflows int32");
    }
    h[P] = (int32_t)e;
    h[2 * P + 1] = (int32_t)w;
    *total_elems = e;
    *total_words = w;
    return host.to(like.device());
}

static std::tuple<torch::Tensor, std::vector<int64_t>> pack_regions(
    torch::Tensor idx, torch::Tensor val, torch::Tensor bounds, bool wire_bf16) {
    check_i32_1d(idx, "idx");
    check_f32_1d(val, "val");
    TORCH_CHECK(idx.numel() == val.numel(), "idx/val size mismatch");
    TORCH_CHECK(bounds.device().is_cpu() && bounds.scalar_type() == torch::kInt64 &&
                bounds.dim() == 1 && bounds.numel() >= 2 && bounds.is_contiguous(),
                "bounds must be a contiguous int64 [P+1] CPU tensor");
    const int64_t P = bounds.numel() - 1;
    TORCH_CHECK(P <= wire_max_segments(), "wire codec: at most ",
                wire_max_segments(), " segments, got ", P);
    const int64_t* bp = bounds.data_ptr<int64_t>();
    for (int64_t j = 0; j < P; ++j)
        TORCH_CHECK(bp[j] <= bp[j + 1], "bounds must be non-decreasing");
    const int64_t m = idx.numel();
    // allocated before the counts are known: exact on the fp32 wire, the
    // bound m + (m+P)/2 on the bf16 wire (at most P odd segments)
    const int64_t cap = wire_bf16 ? m + (m + P) / 2 : 2 * m;
    TORCH_CHECK(cap <= INT32_MAX, "wire codec: word count overflows int32");
    const at::cuda::CUDAGuard guard(idx.device());
    std::vector<int64_t> counts(P, 0);
    if (m == 0)
        return {torch::empty({0}, idx.options()), counts};
    auto buf = torch::empty({cap}, idx.options());
    auto meta = torch::empty({2 * (P + 1)}, idx.options());
    torch::Tensor bdev;  // interior boundaries are only read when P > 1
    if (P > 1) bdev = bounds.to(idx.device());
    launch_wire_cuts(idx.data_ptr<int32_t>(), (int)m,
                     P > 1 ? bdev.data_ptr<int64_t>() : nullptr, (int)P,
                     wire_bf16 ? 1 : 0, meta.data_ptr<int>(), cur_stream());
    launch_wire_pack(idx.data_ptr<int32_t>(), val.data_ptr<float>(), (int)m,
                     meta.data_ptr<int>(), (int)P, wire_bf16 ? 1 : 0,
                     buf.data_ptr<int32_t>(), cur_stream());
    if (P == 1) {
        counts[0] = m;  // nothing to read back
    } else {
        // the one host sync, after both launches are queued
        auto ch = meta.narrow(0, 0, P + 1).cpu();
        const int32_t* cp = ch.data_ptr<int32_t>();
        for (int64_t j = 0; j < P; ++j) counts[j] = cp[j + 1] - cp[j];
    }
    int64_t words = 0;
    for (int64_t j = 0; j < P; ++j) words += wire_words(counts[j], wire_bf16);
    TORCH_CHECK(words <= cap, "wire codec: packed size exceeds its bound");
    return {buf.narrow(0, 0, words), counts};
}

static std::vector<torch::Tensor> unpack_segments(torch::Tensor buf,
                                                  std::vector<int64_t> counts,
                                                  bool wire_bf16) {
    check_i32_1d(buf, "buf");
    const at::cuda::CUDAGuard guard(buf.device());
    int64_t total = 0, words = 0;
    auto meta = wire_tables(counts, wire_bf16, buf, &total, &words);
    TORCH_CHECK(words <= buf.numel(), "wire codec: buf holds ", buf.numel(),
                " words, counts need ", words);
    auto out_idx = torch::empty({total}, buf.options());
    auto out_val = torch::empty({total}, buf.options().dtype(torch::kFloat32));
    if (total > 0)
        launch_wire_unpack(buf.data_ptr<int32_t>(), meta.data_ptr<int>(),
                           (int)counts.size(), (int)total, wire_bf16 ? 1 : 0,
                           out_idx.data_ptr<int32_t>(), out_val.data_ptr<float>(),
                           cur_stream());
    return {out_idx, out_val};
}

static torch::Tensor unpack_scatter_add_(torch::Tensor dest, torch::Tensor buf,
                                         std::vector<int64_t> counts,
                                         int64_t base, bool wire_bf16) {
    check_f32_1d(dest, "dest");
    check_i32_1d(buf, "buf");
    TORCH_CHECK(buf.device() == dest.device(), "buf must be on dest's device");
    const at::cuda::CUDAGuard guard(dest.device());
    int64_t total = 0, words = 0;
    for (int64_t c : counts) total += c;
    if (total == 0) return dest;
    auto meta = wire_tables(counts, wire_bf16, buf, &total, &words);
    TORCH_CHECK(words <= buf.numel(), "wire codec: buf holds ", buf.numel(),
                " words, counts need ", words);
    launch_wire_scatter_add(dest.data_ptr<float>(), dest.numel(),
                            buf.data_ptr<int32_t>(), meta.data_ptr<int>(),
                            (int)counts.size(), (int)total, base,
                            wire_bf16 ? 1 : 0, cur_stream());
    return dest;
}

// ---------------------------------------------------------------------------
// Ok-Topk round-2 tail (round2_tail.hip): global selection over the gathered
// survivors + residual credit.  tau is None on a threshold iteration (k not
// given) and when nothing was gathered.
// ---------------------------------------------------------------------------
static void check_round2_common(const torch::Tensor& residual,
                                const torch::Tensor& idx,
                                const c10::optional<int64_t>& k) {
    check_f32_1d(residual, "residual");
    check_i32_1d(idx, "idx");
    TORCH_CHECK(idx.device() == residual.device(), "idx must be on residual's device");
    TORCH_CHECK(idx.numel() <= INT32_MAX, "round2_tail: idx too long");
    TORCH_CHECK(!k.has_value() || k.value() >= 1, "k must be >= 1");
}

// exact iteration over (all_idx, all_val): the select of topk_select over
// all_val, written through launch_r2_write.  `hist` holds level 1 already
// when the wire decode counted it.
static std::tuple<torch::Tensor, torch::Tensor, py::object> round2_exact(
    torch::Tensor& residual, torch::Tensor& idx, torch::Tensor& all_idx,
    torch::Tensor& all_val, int64_t k, torch::Tensor hist, bool level1_done) {
    const int64_t S = all_idx.numel();
    const int64_t kout = k < S ? k : S;
    auto g_idx = torch::empty({kout}, all_idx.options());
    auto g_val = torch::empty({kout}, all_val.options());
    R2Write r2{all_idx.data_ptr<int32_t>(), idx.data_ptr<int32_t>(),
               (int)idx.numel(), residual.data_ptr<float>(), residual.numel()};
    auto state = tk_select_run(all_val.data_ptr<float>(), S, kout, false,
                               nullptr, nullptr, nullptr, hist, level1_done,
                               g_idx, g_val, &r2);
    return std::make_tuple(g_idx, g_val, py::cast(tk_state_tau(state)));
}

static std::tuple<torch::Tensor, torch::Tensor, py::object> round2_tail_(
    torch::Tensor residual, torch::Tensor idx, torch::Tensor all_idx,
    torch::Tensor all_val, c10::optional<int64_t> k) {
    check_round2_common(residual, idx, k);
    check_i32_1d(all_idx, "all_idx");
    check_f32_1d(all_val, "all_val");
    TORCH_CHECK(all_idx.numel() == all_val.numel(), "all_idx / all_val length mismatch");
    TORCH_CHECK(all_idx.device() == residual.device() &&
                    all_val.device() == residual.device(),
                "round2_tail_: device mismatch");
    const int64_t S = all_idx.numel();
    TORCH_CHECK(S <= INT32_MAX, "round2_tail_: gathered lists too long");
    const at::cuda::CUDAGuard guard(residual.device());
    if (!k.has_value() || S == 0) {
        // the gathered lists are the selection as they stand
        if (S > 0 && idx.numel() > 0)
            launch_r2_credit(all_idx.data_ptr<int32_t>(), (int)S,
                             idx.data_ptr<int32_t>(), (int)idx.numel(),
                             residual.data_ptr<float>(), residual.numel(),
                             cur_stream());
        return std::make_tuple(all_idx, all_val, py::object(py::none()));
    }
    auto hist = torch::zeros({2048}, all_idx.options());
    return round2_exact(residual, idx, all_idx, all_val, k.value(), hist, false);
}

static std::tuple<torch::Tensor, torch::Tensor, py::object> round2_tail_wire_(
    torch::Tensor residual, torch::Tensor idx, torch::Tensor buf,
    std::vector<int64_t> counts, bool wire_bf16, c10::optional<int64_t> k) {
    check_round2_common(residual, idx, k);
    check_i32_1d(buf, "buf");
    TORCH_CHECK(buf.device() == residual.device(), "buf must be on residual's device");
    const at::cuda::CUDAGuard guard(residual.device());
    int64_t S = 0, words = 0;
    auto meta = wire_tables(counts, wire_bf16, buf, &S, &words);
    TORCH_CHECK(words <= buf.numel(), "wire codec: buf holds ", buf.numel(),
                " words, counts need ", words);
    auto all_idx = torch::empty({S}, buf.options());
    auto all_val = torch::empty({S}, buf.options().dtype(torch::kFloat32));
    if (S == 0)
        return std::make_tuple(all_idx, all_val, py::object(py::none()));
    const bool exact = k.has_value();
    torch::Tensor hist;
    if (exact) hist = torch::zeros({2048}, buf.options());
    launch_r2_wire_tail(
        buf.data_ptr<int32_t>(), meta.data_ptr<int>(), (int)counts.size(), (int)S,
        wire_bf16 ? 1 : 0, all_idx.data_ptr<int32_t>(), all_val.data_ptr<float>(),
        idx.data_ptr<int32_t>(), (int)idx.numel(), residual.data_ptr<float>(),
        residual.numel(),
        exact ? reinterpret_cast<unsigned int*>(hist.data_ptr<int>()) : nullptr,
        cur_stream());
    if (!exact)
        return std::make_tuple(all_idx, all_val, py::object(py::none()));
    return round2_exact(residual, idx, all_idx, all_val, k.value(), hist, true);
}

// ---------------------------------------------------------------------------
// Ok-Topk round-1 reduce (reduce_merge.hip): the rank-ordered segments merged
// by index, equal indices summed in segment order, filtered to
// [base, base + length) and |sum| > tau.  mode: 0 pair form (ibuf = idx),
// 1 fp32 wire, 2 bf16 wire (ibuf = buf).  The kept count is the one readback.
// ---------------------------------------------------------------------------
static std::vector<torch::Tensor> reduce_run(
    const torch::Tensor& ibuf, const float* val,
    const std::vector<int64_t>& counts, int mode, int64_t base, int64_t length,
    double tau) {
    const int64_t P = (int64_t)counts.size();
    TORCH_CHECK(P <= reduce_max_segments(), "reduce_segments: at most ",
                reduce_max_segments(), " segments, got ", P);
    TORCH_CHECK(tau >= 0.0, "reduce_segments: tau must be >= 0");
    TORCH_CHECK(length >= 0, "reduce_segments: length must be >= 0");
    // [element prefix | index-list word prefix]; the pair form's index lists
    // are the element prefix itself
    auto host = torch::empty({2 * (P + 1)}, torch::dtype(torch::kInt32));
    int32_t* h = host.data_ptr<int32_t>();
    int64_t M = 0, w = 0;
    for (int64_t j = 0; j <= P; ++j) {
        h[j] = (int32_t)M;
        h[P + 1 + j] = (int32_t)(mode == 0 ? M : w);
        if (j == P) break;
        TORCH_CHECK(counts[j] >= 0, "reduce_segments: negative segment count");
        M += counts[j];
        w += wire_words(counts[j], mode == 2);
        TORCH_CHECK(w <= INT32_MAX, "reduce_segments: payload too long");
    }
    TORCH_CHECK((mode == 0 ? M : w) <= ibuf.numel(),
                "reduce_segments: counts need more than the buffer holds");
    auto iopt = ibuf.options();
    auto fopt = ibuf.options().dtype(torch::kFloat32);
    if (M == 0 || length == 0)
        return {torch::empty({0}, iopt), torch::empty({0}, fopt)};
    auto meta = host.to(ibuf.device());
    auto midx = torch::empty({M}, iopt);
    auto mval = torch::empty({M}, fopt);
    launch_rm_merge(ibuf.data_ptr<int32_t>(), val, meta.data_ptr<int>(), (int)P,
                    (int)M, mode, midx.data_ptr<int32_t>(),
                    mval.data_ptr<float>(), cur_stream());
    int chunk = 0, nblocks = 0;
    rm_heads_geom((int)M, &chunk, &nblocks);
    const int nw = nblocks * 4;
    auto cnt = torch::empty({nw}, iopt);
    launch_rm_heads(midx.data_ptr<int32_t>(), mval.data_ptr<float>(), (int)M,
                    chunk, nblocks, base, length, (float)tau,
                    cnt.data_ptr<int>(), nullptr, nullptr, nullptr, 0,
                    cur_stream());
    auto totals = torch::empty({1}, iopt.dtype(torch::kInt64));
    launch_count_totals(cnt.data_ptr<int>(), nw, 1, totals.data_ptr<int64_t>(),
                        cur_stream());
    const int64_t total = totals.cpu().item<int64_t>();
    TORCH_CHECK(total >= 0 && total <= M, "reduce_segments: bad kept count");
    auto g_idx = torch::empty({total}, iopt);
    auto g_val = torch::empty({total}, fopt);
    if (total > 0) {
        auto offs = torch::empty({nw}, iopt);
        launch_scan_offsets(cnt.data_ptr<int>(), nw, offs.data_ptr<int>(),
                            cur_stream());
        launch_rm_heads(midx.data_ptr<int32_t>(), mval.data_ptr<float>(),
                        (int)M, chunk, nblocks, base, length, (float)tau,
                        cnt.data_ptr<int>(), offs.data_ptr<int>(),
                        g_idx.data_ptr<int32_t>(), g_val.data_ptr<float>(),
                        (int)total, cur_stream());
    }
    return {g_idx, g_val};
}

static std::vector<torch::Tensor> reduce_segments(
    torch::Tensor idx, torch::Tensor val, std::vector<int64_t> counts,
    int64_t base, int64_t length, double tau) {
    check_i32_1d(idx, "idx");
    check_f32_1d(val, "val");
    TORCH_CHECK(idx.numel() == val.numel(), "idx / val length mismatch");
    TORCH_CHECK(val.device() == idx.device(), "val must be on idx's device");
    int64_t total = 0;
    for (int64_t c : counts) total += c;
    TORCH_CHECK(total == idx.numel(), "reduce_segments: counts sum to ", total,
                ", idx holds ", idx.numel());
    const at::cuda::CUDAGuard guard(idx.device());
    return reduce_run(idx, val.data_ptr<float>(), counts, 0, base, length, tau);
}

static std::vector<torch::Tensor> reduce_segments_wire(
    torch::Tensor buf, std::vector<int64_t> counts, bool wire_bf16,
    int64_t base, int64_t length, double tau) {
    check_i32_1d(buf, "buf");
    const at::cuda::CUDAGuard guard(buf.device());
    return reduce_run(buf, nullptr, counts, wire_bf16 ? 2 : 1, base, length, tau);
}

static std::vector<torch::Tensor> linear_gelu(torch::Tensor x, torch::Tensor w,
                                              torch::Tensor bias, bool apply_gelu,
                                              bool want_pre) {
    TORCH_CHECK(x.is_cuda() && w.is_cuda(), "GPU tensors required");
    TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && w.scalar_type() == torch::kBFloat16,
                "bf16 inputs required");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
                "x [M,K], w [N,K]");
    TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
    TORCH_CHECK(x.size(1) % 32 == 0, "K must be a multiple of 32");
    const at::cuda::CUDAGuard guard(x.device());
    int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    auto y = torch::empty({M, N}, x.options());
    torch::Tensor z;
    const float* bptr = nullptr;
    torch::Tensor bias_f;
    if (bias.defined() && bias.numel()) {
        bias_f = bias.to(torch::kFloat32).contiguous();
        bptr = bias_f.data_ptr<float>();
    }
    void* zptr = nullptr;
    if (want_pre) {
        z = torch::empty({M, N}, x.options());
        zptr = z.data_ptr();
    }
    launch_linear_gelu(x.data_ptr(), w.data_ptr(), bptr, y.data_ptr(), zptr,
                       (int)M, (int)N, (int)K, apply_gelu ? 1 : 0, cur_stream());
    if (want_pre) return {y, z};
    return {y};
}

static std::vector<torch::Tensor> add_ln_fwd(torch::Tensor x, torch::Tensor r,
                                             torch::Tensor gamma, torch::Tensor beta,
                                             double eps) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 && x.is_contiguous());
    TORCH_CHECK(r.sizes() == x.sizes() && r.is_contiguous());
    int H = (int)x.size(-1);
    TORCH_CHECK(H % 128 == 0 && H <= 2048, "H must be a multiple of 128, <= 2048");
    const at::cuda::CUDAGuard guard(x.device());
    int64_t rows = x.numel() / H;
    auto y = torch::empty_like(x);
    auto s = torch::empty_like(x);
    auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat32));
    auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat32));
    launch_add_ln_fwd(x.data_ptr(), r.data_ptr(), gamma.contiguous().data_ptr(),
                      beta.contiguous().data_ptr(), y.data_ptr(), s.data_ptr(),
                      mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, H,
                      (float)eps, cur_stream());
    return {y, s, mean, rstd};
}

static std::vector<torch::Tensor> add_ln_bwd(torch::Tensor gy, torch::Tensor s,
                                             torch::Tensor mean, torch::Tensor rstd,
                                             torch::Tensor gamma) {
    TORCH_CHECK(gy.is_cuda() && gy.scalar_type() == torch::kBFloat16);
    int H = (int)gy.size(-1);
    const at::cuda::CUDAGuard guard(gy.device());
    int64_t rows = gy.numel() / H;
    auto gyc = gy.contiguous();
    auto gx = torch::empty_like(gyc);
    auto dgamma = torch::zeros({H}, gy.options().dtype(torch::kFloat32));
    auto dbeta = torch::zeros({H}, gy.options().dtype(torch::kFloat32));
    launch_add_ln_bwd(gyc.data_ptr(), s.data_ptr(), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), gamma.contiguous().data_ptr(),
                      gx.data_ptr(), dgamma.data_ptr<float>(),
                      dbeta.data_ptr<float>(), rows, H, cur_stream());
    return {gx, dgamma, dbeta};
}

static bool ln_bwd_into_supported(int64_t H) { return ln_bwd_supported(H); }

static torch::Tensor ln_bwd_into(torch::Tensor gy, torch::Tensor x,
                                 torch::Tensor gamma, torch::Tensor mean,
                                 torch::Tensor rstd, torch::Tensor dgamma_dst,
                                 torch::Tensor dbeta_dst, bool accumulate) {
    // LayerNorm backward: returns gx; dgamma / dbeta are written (or
    // accumulated) into their gradient slots.  Two launches, no zeroing.
    TORCH_CHECK(gy.is_cuda() && gy.scalar_type() == torch::kBFloat16 &&
                x.scalar_type() == torch::kBFloat16 &&
                gamma.scalar_type() == torch::kBFloat16 &&
                gy.sizes() == x.sizes(), "ln_bwd_into: cuda bf16, same shapes");
    const int64_t H = x.size(-1);
    TORCH_CHECK(ln_bwd_supported(H), "ln_bwd_into: unsupported hidden size ", H);
    const int64_t rows = x.numel() / H;
    TORCH_CHECK(gamma.numel() == H && gamma.is_contiguous());
    for (auto* d : {&dgamma_dst, &dbeta_dst})
        TORCH_CHECK(d->is_cuda() && d->scalar_type() == torch::kBFloat16 &&
                    d->is_contiguous() && d->numel() == H,
                    "ln_bwd_into: slots must be contiguous bf16 [H]");
    TORCH_CHECK(mean.numel() == rows && rstd.numel() == rows);
    const at::cuda::CUDAGuard guard(gy.device());
    auto gyc = gy.contiguous();
    auto xc = x.contiguous();
    auto mf = mean.to(torch::kFloat32).contiguous();
    auto rf = rstd.to(torch::kFloat32).contiguous();
    TORCH_CHECK(((uintptr_t)gyc.data_ptr() & 3) == 0 &&
                ((uintptr_t)xc.data_ptr() & 3) == 0, "ln_bwd_into: 4-byte alignment");
    auto gx = torch::empty_like(xc);
    if (rows == 0) return gx;
    auto ws = torch::empty({(int64_t)ln_bwd_blocks(rows), 2 * H},
                           gy.options().dtype(torch::kFloat32));
    launch_ln_bwd_into(gyc.data_ptr(), xc.data_ptr(), gamma.data_ptr(),
                       mf.data_ptr<float>(), rf.data_ptr<float>(), rows, H,
                       gx.data_ptr(), ws.data_ptr<float>(),
                       dgamma_dst.data_ptr(), dbeta_dst.data_ptr(),
                       accumulate ? 1 : 0, cur_stream());
    return gx;
}

static std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, torch::Tensor mask,
                                           int64_t num_heads, double dropout_p,
                                           bool training, bool want_saved) {
    TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == torch::kBFloat16 &&
                qkv.is_contiguous());
    TORCH_CHECK(qkv.dim() == 3, "qkv must be [b, s, 3*h]");
    int64_t B = qkv.size(0), S = qkv.size(1);
    int64_t H3 = qkv.size(2);
    int64_t H = H3 / 3;
    int64_t HD = H / num_heads;
    TORCH_CHECK(S == 128 && HD == 64, "fused attention specialised for s=128, hd=64");
    const at::cuda::CUDAGuard guard(qkv.device());
    auto out = torch::empty({B, S, H}, qkv.options());
    torch::Tensor p_save, a_save;
    void* pptr = nullptr;
    void* aptr = nullptr;
    if (want_saved) {
        p_save = torch::empty({B * num_heads, S, S}, qkv.options());
        a_save = torch::empty({B * num_heads, S, S}, qkv.options());
        pptr = p_save.data_ptr();
        aptr = a_save.data_ptr();
    }
    const void* mptr = nullptr;
    torch::Tensor mask_c;
    if (mask.defined() && mask.numel()) {
        mask_c = mask.reshape({B, S}).to(torch::kBFloat16).contiguous();
        mptr = mask_c.data_ptr();
    }
    int apply_dropout = (training && dropout_p > 0.0) ? 1 : 0;
    unsigned long long seed = 0, offset = 0;
    const void* seed_ptr = nullptr;
    const void* offset_ptr = nullptr;
    unsigned int intragraph = 0;
    int captured = 0;
    if (apply_dropout) {
        auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
            c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator());
        at::PhiloxCudaState state;
        {
            std::lock_guard<std::mutex> lock(gen->mutex_);
            // one philox4x32 block covers 4 elements
            state = gen->philox_cuda_state((B * num_heads * S * S + 3) / 4 + 1);
        }
        if (state.captured_) {
            captured = 1;
            seed_ptr = state.seed_.ptr;
            offset_ptr = state.offset_.ptr;
            intragraph = state.offset_intragraph_;
        } else {
            seed = state.seed_.val;
            offset = state.offset_.val;
        }
    }
    float scale = 1.0f / std::sqrt((float)HD);
    launch_attn_fwd(qkv.data_ptr(), mptr, out.data_ptr(), pptr, aptr, (int)B,
                    (int)num_heads, scale, (float)(1.0 - dropout_p), seed, offset,
                    seed_ptr, offset_ptr, intragraph, captured, apply_dropout,
                    cur_stream());
    if (want_saved) return {out, p_save, a_save};
    return {out};
}

static std::vector<torch::Tensor> attn_fwd_fa(torch::Tensor qkv,
                                              torch::Tensor mask,
                                              int64_t num_heads,
                                              double dropout_p, bool training,
                                              bool want_lse) {
    TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == torch::kBFloat16 &&
                qkv.is_contiguous());
    TORCH_CHECK(qkv.dim() == 3, "qkv must be [b, s, 3*h]");
    int64_t B = qkv.size(0), S = qkv.size(1);
    int64_t H3 = qkv.size(2);
    int64_t H = H3 / 3;
    int64_t HD = H / num_heads;
    TORCH_CHECK(S % 128 == 0 && HD == 64,
                "flash attention needs seq % 128 == 0 and hd == 64");
    const at::cuda::CUDAGuard guard(qkv.device());
    auto out = torch::empty({B, S, H}, qkv.options());
    torch::Tensor lse;
    void* lse_ptr = nullptr;
    if (want_lse) {
        lse = torch::empty({B * num_heads, S},
                           qkv.options().dtype(torch::kFloat32));
        lse_ptr = lse.data_ptr();
    }
    const void* mptr = nullptr;
    torch::Tensor mask_c;
    if (mask.defined() && mask.numel()) {
        mask_c = mask.reshape({B, S}).to(torch::kBFloat16).contiguous();
        mptr = mask_c.data_ptr();
    }
    int apply_dropout = (training && dropout_p > 0.0) ? 1 : 0;
    unsigned long long seed = 0, offset = 0;
    const void* seed_ptr = nullptr;
    const void* offset_ptr = nullptr;
    unsigned int intragraph = 0;
    int captured = 0;
    if (apply_dropout) {
        auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
            c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator());
        at::PhiloxCudaState state;
        {
            std::lock_guard<std::mutex> lock(gen->mutex_);
            state = gen->philox_cuda_state((B * num_heads * S * S + 3) / 4 + 1);
        }
        if (state.captured_) {
            captured = 1;
            seed_ptr = state.seed_.ptr;
            offset_ptr = state.offset_.ptr;
            intragraph = state.offset_intragraph_;
        } else {
            seed = state.seed_.val;
            offset = state.offset_.val;
        }
    }
    float scale = 1.0f / std::sqrt((float)HD);
    launch_attn_fwd_fa(qkv.data_ptr(), mptr, out.data_ptr(), lse_ptr, (int)B,
                       (int)num_heads, (int)S, scale,
                       (float)(1.0 - dropout_p), seed, offset, seed_ptr,
                       offset_ptr, intragraph, captured, apply_dropout,
                       cur_stream());
    // philox state rides back as a CPU int64 tensor so the recompute
    // backward can regenerate the identical dropout mask (pointers are
    // round-tripped as ints; valid while the capture/graph lives)
    auto st = torch::tensor(
        {(int64_t)seed, (int64_t)offset, (int64_t)(uintptr_t)seed_ptr,
         (int64_t)(uintptr_t)offset_ptr, (int64_t)intragraph,
         (int64_t)captured},
        torch::TensorOptions().dtype(torch::kInt64));
    if (want_lse) return {out, lse, st};
    return {out, st};
}

static torch::Tensor attn_bwd_fa(torch::Tensor qkv, torch::Tensor go,
                                 torch::Tensor lse, torch::Tensor dvec,
                                 torch::Tensor mask, torch::Tensor philox_state,
                                 int64_t num_heads, double dropout_p,
                                 bool training) {
    TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == torch::kBFloat16 &&
                qkv.is_contiguous());
    TORCH_CHECK(go.scalar_type() == torch::kBFloat16 && go.is_contiguous());
    TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.is_contiguous());
    TORCH_CHECK(dvec.scalar_type() == torch::kFloat32 && dvec.is_contiguous());
    int64_t B = qkv.size(0), S = qkv.size(1);
    int64_t H = qkv.size(2) / 3;
    int64_t HD = H / num_heads;
    TORCH_CHECK(S % 128 == 0 && HD == 64,
                "flash attention bwd needs seq % 128 == 0 and hd == 64");
    const at::cuda::CUDAGuard guard(qkv.device());
    auto dqkv = torch::empty_like(qkv);
    const void* mptr = nullptr;
    torch::Tensor mask_c;
    if (mask.defined() && mask.numel()) {
        mask_c = mask.reshape({B, S}).to(torch::kBFloat16).contiguous();
        mptr = mask_c.data_ptr();
    }
    int apply_dropout = (training && dropout_p > 0.0) ? 1 : 0;
    TORCH_CHECK(philox_state.numel() == 6);
    auto st = philox_state.to(torch::kCPU);
    auto* p = st.data_ptr<int64_t>();
    float scale = 1.0f / std::sqrt((float)HD);
    launch_attn_bwd_fa(qkv.data_ptr(), go.data_ptr(), lse.data_ptr(),
                       dvec.data_ptr(), mptr, dqkv.data_ptr(), (int)B,
                       (int)num_heads, (int)S, scale,
                       (float)(1.0 - dropout_p), (unsigned long long)p[0],
                       (unsigned long long)p[1], (const void*)(uintptr_t)p[2],
                       (const void*)(uintptr_t)p[3], (unsigned int)p[4],
                       (int)p[5], apply_dropout, cur_stream());
    return dqkv;
}

static void dropout_mask_mul_(torch::Tensor a, torch::Tensor philox_state,
                              double dropout_p) {
    TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 &&
                a.is_contiguous());
    TORCH_CHECK(a.dim() == 3 && a.size(1) == a.size(2) &&
                a.size(1) % 4 == 0, "a must be [BH, S, S]");
    TORCH_CHECK(philox_state.numel() == 6);
    auto st = philox_state.to(torch::kCPU);
    auto* p = st.data_ptr<int64_t>();
    const at::cuda::CUDAGuard guard(a.device());
    // captured mode: the kernel reads the device-side seed/offset (same
    // graph/replay as the fwd), so the mask is identical per replay
    launch_dropout_mask_mul(
        a.data_ptr(), a.size(0), a.size(1), (unsigned long long)p[0],
        (unsigned long long)p[1], (const void*)(uintptr_t)p[2],
        (const void*)(uintptr_t)p[3], (unsigned int)p[4], (int)p[5],
        (float)(1.0 - dropout_p), cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "oktopk_amd CDNA4 HIP kernels (gfx950)";
    m.def("count_gt", &count_gt, "count |t| > tau");
    m.def("count_multi_gt", &count_multi_gt, "counts for up to 8 thresholds, one pass");
    m.def("compact_gt", &compact_gt, "ascending (idx,val) where |t| > tau");
    m.def("compact_adaptive", &compact_adaptive,
          "one-pass adaptive-threshold compaction: counts all candidate taus, "
          "applies the bump rule, extracts at the chosen tau");
    m.def("compact_adaptive_ef", &compact_adaptive_ef,
          "fused EF restore(+bf16 upcast) + adaptive-threshold compaction",
          py::arg("t"), py::arg("residual"), py::arg("grad"), py::arg("taus"),
          py::arg("hi_limit"));
    m.def("gaussian_select_ef", &gaussian_select_ef,
          "device-resident Gaussian-k selection: EF restore + fp64 moments, "
          "on-device ppf + refine tree, compact write; returns (idx, val, "
          "chosen, count, tau, tau0, mean, std)",
          py::arg("t"), py::arg("residual"), py::arg("grad"),
          py::arg("density"), py::arg("k"));
    m.def("topk_select", &topk_select,
          "exact top-k by |t| (lowest-index ties); returns (idx, val, tau)",
          py::arg("t"), py::arg("k"));
    m.def("topk_select_ef", &topk_select_ef,
          "fused EF restore(+bf16 upcast) + exact top-k; residual = restored "
          "with the selection zeroed; returns (idx, val, tau)",
          py::arg("t"), py::arg("residual"), py::arg("grad"), py::arg("k"));
    m.def("sparse_merge_topk", &sparse_merge_topk,
          "top-k of the sum of two ascending sparse vectors; returns (idx, val)",
          py::arg("a_idx"), py::arg("a_val"), py::arg("b_idx"),
          py::arg("b_val"), py::arg("k"));
    m.def("kth_abs_value", &kth_abs_value, "exact k-th largest |t| via radix select");
    m.def("scatter_add_", &scatter_add_, "dest[idx] += val");
    m.def("zero_at_", &zero_at_, "t[idx] = 0");
    m.def("zero_at_masked_", &zero_at_masked_, "t[idx[i]] = 0 where mask[idx[i]]");
    m.def("fill_sparse_scaled_", &fill_sparse_scaled_, "out=0; out[idx]=val*scale");
    m.def("isin_sorted", &isin_sorted, "membership of a in sorted b");
    m.def("ef_restore_snapshot_", &ef_restore_snapshot_, "t+=r; r=t (fused)");
    m.def("ef_restore_upcast_", &ef_restore_upcast_,
          "t = float(g_bf16) + r; r = t (fused upcast + EF restore)");
    m.def("fused_sgd_", &fused_sgd_, "fused SGD step");
    m.def("fused_adam_", &fused_adam_, "fused (Bert)Adam step",
          py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
          py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
          py::arg("wd"), py::arg("gscale") = py::none());
    m.def("fused_adam_mirror_", &fused_adam_mirror_,
          "fused Adam step + bf16 weight-mirror write",
          py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
          py::arg("p_bf16"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
          py::arg("eps"), py::arg("wd"), py::arg("gscale") = py::none());
    m.def("scatter_gt_credit_", &scatter_gt_credit_,
          "fused world-1 round-2 tail: result[idx]=val*scale and "
          "residual[idx]=0 where |val|>tau; returns the count");
    m.def("grad_clip_scale", &grad_clip_scale,
          "device-resident clip factor min(1, max/||t||) (no host sync)");
    m.def("credit_gt_", &credit_gt_,
          "residual[idx]=0 where |val|>tau; returns the count (no dense result)");
    m.def("sparse_sumsq_into_", &sparse_sumsq_into_,
          "acc (fp64[1]) += sum((val*scale)^2) over entries with |val|>tau");
    m.def("grad_clip_scale_sparse", &grad_clip_scale_sparse,
          "grad_clip_scale of a sparse gradient (idx, val, scale, tau)");
    m.def("fused_adam_sparse_", &fused_adam_sparse_,
          "fused Adam step, gradient given as (idx, val, base, scale, tau)",
          py::arg("p"), py::arg("idx"), py::arg("val"), py::arg("base"),
          py::arg("scale"), py::arg("tau"), py::arg("m"), py::arg("v"),
          py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
          py::arg("wd"), py::arg("gscale") = py::none());
    m.def("fused_adam_sparse_mirror_", &fused_adam_sparse_mirror_,
          "fused_adam_sparse_ + bf16 weight-mirror write",
          py::arg("p"), py::arg("idx"), py::arg("val"), py::arg("base"),
          py::arg("scale"), py::arg("tau"), py::arg("m"), py::arg("v"),
          py::arg("p_bf16"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
          py::arg("eps"), py::arg("wd"), py::arg("gscale") = py::none());
    m.def("sgd_step_", &sgd_step_,
          "flat SGD step (momentum / nesterov / weight decay), unfused "
          "roundings; buf untouched when momentum == 0",
          py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("lr"),
          py::arg("momentum"), py::arg("wd"), py::arg("nesterov"),
          py::arg("gscale") = py::none());
    m.def("sgd_step_sparse_", &sgd_step_sparse_,
          "sgd_step_, gradient given as (idx, val, base, scale, tau)",
          py::arg("p"), py::arg("idx"), py::arg("val"), py::arg("base"),
          py::arg("scale"), py::arg("tau"), py::arg("buf"), py::arg("lr"),
          py::arg("momentum"), py::arg("wd"), py::arg("nesterov"),
          py::arg("gscale") = py::none());
    m.def("clip_scale_from_sumsq", &clip_scale_from_sumsq,
          "clip factor min(1, max/(sqrt(acc)+1e-6)) from an fp64 sum of squares");
    m.def("l2norm", &l2norm, "L2 norm (fp64 accumulate)");
    m.def("colsum_bf16_into", &colsum_bf16_into,
          "bias grad: dst (=|+=) column sum of bf16 [R, C], one launch",
          py::arg("gy"), py::arg("dst"), py::arg("accumulate") = false);
    m.def("colsum_bf16_into_exact", &colsum_bf16_into_exact,
          "bias grad in torch's summation order (bit-equal to sum_out); "
          "False = unsupported (accumulate always is), nothing written",
          py::arg("gy"), py::arg("dst"), py::arg("accumulate") = false);
    m.def("colsum_exact_config", &colsum_exact_config,
          "torch's reduce configuration (V, bw, bh, split, ctas) for a "
          "dim-0 sum of a contiguous bf16 [R, C], or None",
          py::arg("R"), py::arg("C"), py::arg("src_addr"), py::arg("num_mp"),
          py::arg("max_threads_per_mp"), py::arg("warp_size"));
    m.def("ln_bwd_supported", &ln_bwd_into_supported,
          "hidden sizes ln_bwd_into handles");
    m.def("ln_bwd_into", &ln_bwd_into,
          "LayerNorm backward; dgamma/dbeta written into their gradient slots, returns gx",
          py::arg("gy"), py::arg("x"), py::arg("gamma"), py::arg("mean"),
          py::arg("rstd"), py::arg("dgamma_dst"), py::arg("dbeta_dst"),
          py::arg("accumulate") = false);
    m.def("linear_bwd_into", &linear_bwd_into,
          "Linear backward; gW/gb written into their gradient slots, returns gx",
          py::arg("gy"), py::arg("x"), py::arg("w"), py::arg("gw_dst"),
          py::arg("gb_dst"), py::arg("accumulate") = false,
          py::arg("bias_kernel") = false, py::arg("bias_exact") = false);
    m.def("attn_rowdot", &attn_rowdot,
          "flash-bwd D: per-(head,row) dot of gO and O (head_dim 64)");
    m.def("sumsq_into_", &sumsq_into_,
          "accumulate sum(t^2) into a device fp64[1] (no host sync)");
    m.def("attn_fwd", &attn_fwd,
          "fused self-attention forward: softmax(QK^T*scale+mask) dropout @ V "
          "(bf16 MFMA, seq=128/hd=64; returns ctx [+P, A for backward])");
    m.def("attn_fwd_fa", &attn_fwd_fa,
          "flash (online-softmax) attention forward: any seq % 128 == 0, "
          "hd=64 bf16; returns (ctx, lse, philox_state) — O(S) memory");
    m.def("attn_bwd_fa", &attn_bwd_fa,
          "flash attention backward: dQ/dK/dV from (qkv, gO, lse, D) with "
          "philox dropout-mask regeneration — nothing O(S^2) materialised");
    m.def("dropout_mask_mul_", &dropout_mask_mul_,
          "regenerate the forward's philox dropout mask in-place: "
          "a[i] = keep ? a[i]/keep_prob : 0");
    m.def("wire_max_segments", []() { return (int64_t)wire_max_segments(); },
          "largest segment count the wire codec kernels take");
    m.def("pack_regions", &pack_regions,
          "split an ascending (idx, val) selection at the region bounds and "
          "pack it into the wire layout; returns (buf, counts)",
          py::arg("idx"), py::arg("val"), py::arg("bounds"), py::arg("wire_bf16"));
    m.def("unpack_segments", &unpack_segments,
          "gather all wire segments into contiguous (idx int32, val fp32)",
          py::arg("buf"), py::arg("counts"), py::arg("wire_bf16"));
    m.def("unpack_scatter_add_", &unpack_scatter_add_,
          "dest[idx - base] += val for every wire entry (fused unpack-reduce)",
          py::arg("dest"), py::arg("buf"), py::arg("counts"), py::arg("base"),
          py::arg("wire_bf16"));
    m.def("round2_tail_", &round2_tail_,
          "Ok-Topk round-2 tail over gathered (all_idx, all_val): global "
          "selection (all entries, or exact top-k ascending) + residual "
          "credit; returns (g_idx, g_val, tau or None)",
          py::arg("residual"), py::arg("idx"), py::arg("all_idx"),
          py::arg("all_val"), py::arg("k") = py::none());
    m.def("round2_tail_wire_", &round2_tail_wire_,
          "round2_tail_ over the allgathered wire buffer (decode fused in)",
          py::arg("residual"), py::arg("idx"), py::arg("buf"), py::arg("counts"),
          py::arg("wire_bf16"), py::arg("k") = py::none());
    m.def("reduce_max_segments", []() { return (int64_t)reduce_max_segments(); },
          "segment limit of the ordered-merge reduce");
    m.def("reduce_segments", &reduce_segments,
          "ordered sparse reduce of rank-ordered ascending segments -> "
          "(g_idx ascending, g_val) with base <= idx < base + length, |sum| > tau",
          py::arg("idx"), py::arg("val"), py::arg("counts"), py::arg("base"),
          py::arg("length"), py::arg("tau"));
    m.def("reduce_segments_wire", &reduce_segments_wire,
          "reduce_segments over the packed wire buffer (decode fused in)",
          py::arg("buf"), py::arg("counts"), py::arg("wire_bf16"),
          py::arg("base"), py::arg("length"), py::arg("tau"));
    m.def("add_ln_fwd", &add_ln_fwd, "fused y=LN(x+r) forward (bf16)");
    m.def("add_ln_bwd", &add_ln_bwd, "fused add+LN backward (bf16, fp32 col sums)");
    m.def("linear_gelu", &linear_gelu,
          "fused y=gelu(x@W^T+b) bf16 MFMA kernel (optionally returns pre-act)");
}

// C-ABI of the loop-closure batch (included at the end of ndt2d_api.hip behind ndt_batch_host.hpp: one translation unit,
// so the kernels of ndt2d_kernels.hpp are defined once).  The context's plumbing is ndt_batch_host.hpp's; here are the
// 2D context, what is 2D's alone - the small variant and its marks, last_large, a level of overlapping grids - and
// the extern "C" shims.
#pragma once
#include <array>
#include <vector>

#include "ndt2d_batch.hpp"

struct ndt2d_batch : ndt::BatchContext<2, ndt2d_result, ndt2d_handle> {
  int* d_marks = nullptr;                // [n_pairs]: pairs the small variant left to the large one
  size_t marks_cap = 0;
  std::vector<int> h_marks;              // ... of the last host-pointer call, read back where the small variant ran
  bool use_small = true;                 // lidar-sized pairs run on the 256-thread variant first (ndt2d_batch_set_tuning)
  int64_t last_large = -1;               // pairs the last host-pointer call's final level ran on the large variant
};

static_assert(sizeof(ndt::ResultDev) == sizeof(ndt2d_result), "ResultDev mirrors ndt2d_result");
static_assert(offsetof(ndt::ResultDev, score) == offsetof(ndt2d_result, score), "ResultDev layout");
static_assert(offsetof(ndt::ResultDev, status) == offsetof(ndt2d_result, status), "ResultDev layout");

namespace {

template <> struct BatchTraits<ndt2d_batch> {
  using Result = ndt2d_result;
  using Handle = ndt2d_handle;
  using Args = ndt::BatchArgs;
  using Variant = ndt::BatchVariant<Args>;
  static constexpr int kDim = 2, kPose = 3;
  static constexpr size_t kSlabBytes = ndt::BatchGlobal::kTabBytes;
  static constexpr int kBlocksStart = ndt::kBatchGlobalBlocksStart, kBlocksFull = ndt::kBatchGlobalBlocks, kBlocksMax = ndt::kBatchGlobalBlocksMax;
  static constexpr const char* kTraceLaunch = "ndt2d_batch: grid build + Gauss-Newton loops on chip";
  static constexpr const char* kTraceGather = "ndt2d_multi: RCCL all-gather of the result rows";
  static constexpr Variant kSmall{{ndt::k_batch<0, ndt::BatchSmall>, ndt::k_batch<1, ndt::BatchSmall>}, ndt::BatchSmall::kThreads, ndt::BatchSmall::kLdsBytes};
  static constexpr Variant kLarge{{ndt::k_batch<0, ndt::BatchLarge>, ndt::k_batch<1, ndt::BatchLarge>}, ndt::kBatchThreads, ndt::kBatchLdsBytes};
  static constexpr Variant kGlobal{{ndt::k_batch_fallback<0>, ndt::k_batch_fallback<1>}, ndt::BatchGlobal::kThreads, ndt::BatchGlobal::kLdsBytes};
  static constexpr Variant kGlobal4{{ndt::k_batch_fallback<0, 4>, ndt::k_batch_fallback<1, 4>}, ndt::BatchGlobal::kThreads, ndt::BatchGlobal::kLdsBytes};
  static std::array<Variant, 4> variants() { return {kSmall, kLarge, kGlobal, kGlobal4}; }

  static int32_t create(const ndt2d_params* p, int device, Handle** out) { return ndt2d_create(p, device, out); }
  static int32_t set_target(Handle* f, const float* const* t, size_t n) { return ndt2d_set_target(f, t[0], t[1], n); }
  static int32_t align(Handle* f, const float* const* s, size_t n, const double* pose, Result* out) { return ndt2d_align(f, s[0], s[1], n, pose, out); }
  static void destroy(Handle* f) { ndt2d_destroy(f); }
  static int32_t create_context(const ndt2d_params* levels, int32_t n_levels, int32_t device_id, ndt2d_batch** out) {
    return ndt2d_batch_create_pyramid(levels, n_levels, device_id, out);
  }

  static int32_t create_own(ndt2d_batch* b) {
    // a level with overlapping grids runs EVERY pair on the global-table variant: one table slab per CU from the start
    for (const ndt2d_params& p : b->levels)
      if (p.overlap_grids == 4) b->global_blocks = b->n_cu < kBlocksFull ? b->n_cu : kBlocksFull;
    return NDT_OK;
  }
  static void free_own(ndt2d_batch* b) { if (b->d_marks) (void)hipFree(b->d_marks); }
  static int32_t bind_own(ndt2d_batch* b, Args& a, size_t n_pairs) {
    HIP_TRY(ndt::grow(&b->d_marks, &b->marks_cap, n_pairs, n_pairs + n_pairs / 4 + 64));
    a.slab = b->d_gslab;
    return NDT_OK;
  }
  static void set_clouds(Args& a, const float* const* t, const float* const* s) { a.tx = t[0]; a.ty = t[1]; a.sx = s[0]; a.sy = s[1]; }

  // The small variant takes every pair it can hold (lidar-sized scans) and marks the rest, the large variant then takes
  // exactly the marked ones, the global-table variant those whose grid does not fit on chip (handed over through fb_marks).
  static int32_t launch_level(ndt2d_batch* b, Args& a, const ndt2d_params& p, size_t n_pairs, hipStream_t st) {
    const bool newton = p.hessian_mode == NDT_HESSIAN_NEWTON;
    auto at_most = [&](size_t cap) { return (int)(n_pairs < cap ? n_pairs : cap); };
    const int blocks_fb = at_most((size_t)b->global_blocks);
    a.marks = nullptr;
    if (p.overlap_grids == 4) {
      // Biber's four overlapping grids: every pair of this level goes to the global-table variant (process_pair's NG),
      // so every pair is marked for it (any non-zero word is a mark)
      HIP_TRY(hipMemsetAsync(b->d_fb, 1, n_pairs * sizeof(int), st));
      a.queue = b->d_queue + 1;
      return launch_variant(kGlobal4, newton, blocks_fb, st, a);
    }
    HIP_TRY(hipMemsetAsync(b->d_queue, 0, 16, st));
    HIP_TRY(hipMemsetAsync(b->d_fb, 0, n_pairs * sizeof(int), st));
    if (b->use_small) {
      a.marks = b->d_marks;
      a.queue = b->d_queue;
      // the small variant keeps two workgroups resident per CU
      const int32_t ss = launch_variant(kSmall, newton, at_most(2 * (size_t)b->n_cu), st, a);
      if (ss != NDT_OK) return ss;
    }
    a.queue = b->d_queue + 1;                        // its own dequeue counter
    const int32_t ls = launch_variant(kLarge, newton, at_most((size_t)b->n_cu), st, a);
    return ls != NDT_OK ? ls : launch_variant(kGlobal, newton, blocks_fb, st, a);
  }

  static bool own_knob(int32_t knob) { return knob == NDT_TUNE_BATCH_SMALL_VARIANT; }
  static void tune_own(ndt2d_batch* b, int32_t, int64_t value) { b->use_small = value != 0; }

  // the small variant's marks tell how many pairs the final level ran on the large one
  // (an overlapping-grids level runs neither on-chip variant)
  static bool small_ran(const ndt2d_batch* b) { return b->use_small && b->levels.back().overlap_grids != 4; }
  static int32_t read_back(ndt2d_batch* b, size_t n_pairs, hipStream_t st) {
    b->h_marks.assign(small_ran(b) ? n_pairs : 0, 0);
    if (!b->h_marks.empty()) HIP_TRY(hipMemcpyAsync(b->h_marks.data(), b->d_marks, n_pairs * sizeof(int), hipMemcpyDeviceToHost, st));
    return NDT_OK;
  }
  static void host_done(ndt2d_batch* b, size_t n_pairs) {
    b->last_large = small_ran(b) ? 0 : (int64_t)n_pairs;
    for (int m : b->h_marks) b->last_large += m != 0;
  }
};

}  // namespace

extern "C" {

// The library's standard coarse-to-fine schedule: 4c and 2c cells with a
// stronger eigenvalue clamp, loose stops and a proportionally larger step limit, then `fine`.
int32_t ndt2d_default_pyramid(const ndt2d_params* fine, ndt2d_params levels[3]) {
  if (!fine || !levels) return NDT_ERR_INVALID_ARG;
  const double mult[2] = {4.0, 2.0}, ratio[2] = {0.1, 0.03};
  for (int i = 0; i < 2; ++i) {
    ndt2d_params p = *fine;
    p.cell_size = fine->cell_size * mult[i];
    p.eig_ratio = ratio[i];
    p.eps_trans = 1e-3; p.eps_rot = 1e-4;
    p.max_iterations = 30; p.fixed_iterations = 0;
    p.step_max_trans = fine->step_max_trans * mult[i];
    levels[i] = p;
  }
  levels[2] = *fine;
  return NDT_OK;
}

int32_t ndt2d_batch_create_pyramid(const ndt2d_params* levels, int32_t n_levels, int32_t device_id, ndt2d_batch** out) {
  if (!out) return NDT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!levels || n_levels < 1 || n_levels > 8) return NDT_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n_levels; ++i) {
    const int32_t st = check_params(&levels[i]);
    if (st != NDT_OK) return st;
  }
  return batch_create_pyramid(levels, n_levels, device_id, out);
}

int32_t ndt2d_batch_create(const ndt2d_params* p, int32_t device_id, ndt2d_batch** out) {
  if (!p) { if (out) *out = nullptr; return NDT_ERR_INVALID_ARG; }
  return ndt2d_batch_create_pyramid(p, 1, device_id, out);
}

int32_t ndt2d_batch_destroy(ndt2d_batch* b) { return batch_destroy(b); }

int64_t ndt2d_batch_last_large_count(const ndt2d_batch* b) { return b ? b->last_large : -1; }

void* ndt2d_batch_stream(ndt2d_batch* b) { return b ? (void*)b->stream : nullptr; }

int32_t ndt2d_batch_set_tuning(ndt2d_batch* b, int32_t knob, int64_t value) { return batch_set_tuning(b, knob, value); }

int32_t ndt2d_batch_wait_stream(ndt2d_batch* b, void* producer_stream) { return batch_wait_stream(b, producer_stream); }

int32_t ndt2d_batch_align_dev(ndt2d_batch* b, const float* d_tx, const float* d_ty, const uint64_t* d_toff,
                              const float* d_sx, const float* d_sy, const uint64_t* d_soff,
                              const double* d_init, size_t n_pairs, ndt2d_result* d_results, void* stream) {
  const float *const t[2] = {d_tx, d_ty}, *const s[2] = {d_sx, d_sy};
  return batch_align_dev(b, t, d_toff, s, d_soff, d_init, n_pairs, d_results, stream);
}

int32_t ndt2d_batch_align(ndt2d_batch* b, const float* tx, const float* ty, const uint64_t* toff,
                          const float* sx, const float* sy, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt2d_result* results) {
  const float *const t[2] = {tx, ty}, *const s[2] = {sx, sy};
  return batch_align(b, t, toff, s, soff, init, n_pairs, results);
}

}  // extern "C"

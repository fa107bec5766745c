// C-ABI of the 3D loop-closure batch (included at the end of ndt2d_api.hip behind ndt_batch_host.hpp: one translation
// unit).  The context's plumbing is ndt_batch_host.hpp's; here are the 3D context, its traits and the extern "C" shims.
#pragma once
#include <array>
#include <vector>

#include "ndt3d_batch.hpp"

struct ndt3d_batch : ndt::BatchContext<3, ndt3d_result, ndt3d_handle> {
  unsigned char* d_slab = nullptr;    // [n_cu][kB3SlabBytes]: what k_batch3 keeps of a pair beside its LDS carve
};

static_assert(sizeof(ndt::Result3Dev) == sizeof(ndt3d_result), "Result3Dev mirrors ndt3d_result");
static_assert(offsetof(ndt::Result3Dev, H) == offsetof(ndt3d_result, H), "Result3Dev layout");
static_assert(offsetof(ndt::Result3Dev, score) == offsetof(ndt3d_result, score), "Result3Dev layout");
static_assert(offsetof(ndt::Result3Dev, status) == offsetof(ndt3d_result, status), "Result3Dev layout");

namespace {

template <> struct BatchTraits<ndt3d_batch> {
  using Result = ndt3d_result;
  using Handle = ndt3d_handle;
  using Args = ndt::Batch3Args;
  using Variant = ndt::BatchVariant<Args>;
  static constexpr int kDim = 3, kPose = 6;
  static constexpr size_t kSlabBytes = ndt::kG3SlabBytes;
  static constexpr int kBlocksStart = ndt::kG3BlocksStart, kBlocksFull = ndt::kG3Blocks, kBlocksMax = ndt::kG3BlocksMax;
  static constexpr const char* kTraceLaunch = "ndt3d_batch: voxel grid build + Gauss-Newton loops on chip";
  static constexpr const char* kTraceGather = "ndt3d_multi: RCCL all-gather of the result rows";
  static constexpr Variant kOnChip{{ndt::k_batch3<0>, ndt::k_batch3<1>}, ndt::kB3Threads, ndt::kB3LdsBytes};
  static constexpr Variant kGlobal{{ndt::k_batch3_fallback<0>, ndt::k_batch3_fallback<1>}, ndt::kB3Threads, ndt::kB3LdsBytes};
  static std::array<Variant, 2> variants() { return {kOnChip, kGlobal}; }

  static int32_t create(const ndt3d_params* p, int device, Handle** out) { return ndt3d_create(p, device, out); }
  static int32_t set_target(Handle* f, const float* const* t, size_t n) { return ndt3d_set_target(f, t[0], t[1], t[2], n); }
  static int32_t align(Handle* f, const float* const* s, size_t n, const double* pose, Result* out) {
    return ndt3d_align(f, s[0], s[1], s[2], n, pose, out);
  }
  static void destroy(Handle* f) { ndt3d_destroy(f); }
  static int32_t create_context(const ndt3d_params* levels, int32_t n_levels, int32_t device_id, ndt3d_batch** out) {
    return ndt3d_batch_create_pyramid(levels, n_levels, device_id, out);
  }

  static int32_t create_own(ndt3d_batch* b) {
    return hipMalloc((void**)&b->d_slab, (size_t)b->n_cu * ndt::kB3SlabBytes) == hipSuccess ? NDT_OK : NDT_ERR_ALLOC;
  }
  static void free_own(ndt3d_batch* b) { if (b->d_slab) (void)hipFree(b->d_slab); }
  static int32_t bind_own(ndt3d_batch* b, Args& a, size_t) {
    a.slab = b->d_slab;
    a.gslab = b->d_gslab;
    return NDT_OK;
  }
  static void set_clouds(Args& a, const float* const* t, const float* const* s) {
    a.tx = t[0]; a.ty = t[1]; a.tz = t[2];
    a.sx = s[0]; a.sy = s[1]; a.sz = s[2];
  }

  // k_batch3 takes every pair; those whose voxel grid does not fit the LDS carve (handed over through fb_marks) have
  // their tables in global memory
  static int32_t launch_level(ndt3d_batch* b, Args& a, const ndt3d_params& p, size_t n_pairs, hipStream_t st) {
    const bool newton = p.hessian_mode == NDT_HESSIAN_NEWTON;
    const int blocks = (int)(n_pairs < (size_t)b->n_cu ? n_pairs : (size_t)b->n_cu);
    const int blocks_fb = (int)(n_pairs < (size_t)b->global_blocks ? n_pairs : (size_t)b->global_blocks);
    HIP_TRY(hipMemsetAsync(b->d_queue, 0, 16, st));
    HIP_TRY(hipMemsetAsync(b->d_fb, 0, n_pairs * sizeof(int), st));
    const int32_t ls = launch_variant(kOnChip, newton, blocks, st, a);
    return ls != NDT_OK ? ls : launch_variant(kGlobal, newton, blocks_fb, st, a);
  }

  static bool own_knob(int32_t) { return false; }
  static void tune_own(ndt3d_batch*, int32_t, int64_t) {}
  static int32_t read_back(ndt3d_batch*, size_t, hipStream_t) { return NDT_OK; }
  static void host_done(ndt3d_batch*, size_t) {}
};

}  // namespace

extern "C" {

int32_t ndt3d_batch_destroy(ndt3d_batch* b) { return batch_destroy(b); }

int32_t ndt3d_batch_create_pyramid(const ndt3d_params* levels, int32_t n_levels, int32_t device_id, ndt3d_batch** out) {
  if (!out) return NDT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!levels || n_levels < 1 || n_levels > 8) return NDT_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n_levels; ++i) {
    const int32_t st = check_params(&levels[i]);
    if (st != NDT_OK) return st;
    if (levels[i].overlap_grids == 4) { set_error("overlapping grids are a 2D option"); return NDT_ERR_INVALID_ARG; }
  }
  return batch_create_pyramid(levels, n_levels, device_id, out);
}

int32_t ndt3d_batch_create(const ndt3d_params* p, int32_t device_id, ndt3d_batch** out) {
  if (!p) { if (out) *out = nullptr; return NDT_ERR_INVALID_ARG; }
  return ndt3d_batch_create_pyramid(p, 1, device_id, out);
}

void* ndt3d_batch_stream(ndt3d_batch* b) { return b ? (void*)b->stream : nullptr; }

int32_t ndt3d_batch_set_tuning(ndt3d_batch* b, int32_t knob, int64_t value) { return batch_set_tuning(b, knob, value); }

int32_t ndt3d_batch_wait_stream(ndt3d_batch* b, void* producer_stream) { return batch_wait_stream(b, producer_stream); }

int32_t ndt3d_batch_align_dev(ndt3d_batch* b, const float* d_tx, const float* d_ty, const float* d_tz, const uint64_t* d_toff,
                              const float* d_sx, const float* d_sy, const float* d_sz, const uint64_t* d_soff,
                              const double* d_init, size_t n_pairs, ndt3d_result* d_results, void* stream) {
  const float *const t[3] = {d_tx, d_ty, d_tz}, *const s[3] = {d_sx, d_sy, d_sz};
  return batch_align_dev(b, t, d_toff, s, d_soff, d_init, n_pairs, d_results, stream);
}

int32_t ndt3d_batch_align(ndt3d_batch* b, const float* tx, const float* ty, const float* tz, const uint64_t* toff,
                          const float* sx, const float* sy, const float* sz, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt3d_result* results) {
  const float *const t[3] = {tx, ty, tz}, *const s[3] = {sx, sy, sz};
  return batch_align(b, t, toff, s, soff, init, n_pairs, results);
}

}  // extern "C"

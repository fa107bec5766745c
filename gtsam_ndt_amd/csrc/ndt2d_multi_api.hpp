// C-ABI of the multi-device loop-closure context (included at the end of ndt2d_api.hip behind ndt2d_batch_api.hpp), for
// a C++ host process that owns all GPUs of a node itself: ndt_batch_host.hpp's MultiContext over ndt2d_batch contexts
// (ndt2d_multi_align: host pointers, one host thread per device; ndt2d_multi_align_dev: device-resident shards and ONE
// grouped ncclAllGather of the result rows) and the extern "C" shims.
#pragma once

struct ndt2d_multi : ndt::MultiContext<ndt2d_batch> {};

int32_t ndt2d_multi_destroy(ndt2d_multi* m) { return multi_destroy(m); }

int32_t ndt2d_multi_create_pyramid(const ndt2d_params* levels, int32_t n_levels, const int32_t* device_ids,
                                   int32_t n_devices, ndt2d_multi** out) {
  return multi_create_pyramid(levels, n_levels, device_ids, n_devices, out);
}

int32_t ndt2d_multi_create(const ndt2d_params* p, const int32_t* device_ids, int32_t n_devices, ndt2d_multi** out) {
  if (!p) { if (out) *out = nullptr; return NDT_ERR_INVALID_ARG; }
  return ndt2d_multi_create_pyramid(p, 1, device_ids, n_devices, out);
}

int32_t ndt2d_multi_device_count(const ndt2d_multi* m) { return m ? static_cast<int32_t>(m->ctx.size()) : 0; }

// shard_begin[d] .. shard_begin[d+1] = the pairs device slot d would receive for these offsets
// (exposed so a caller can pre-place data, and so the split is testable without devices; the 3D contexts split alike)
int32_t ndt2d_multi_plan_hinted(int32_t n_shards, const uint64_t* toff, const uint64_t* soff, size_t n_pairs,
                                int32_t iterations_hint, const int32_t* pair_iterations, uint64_t* shard_begin) {
  if (n_shards <= 0 || !toff || !soff || !shard_begin) return NDT_ERR_INVALID_ARG;
  return ndt::plan_shards(n_shards, toff, soff, n_pairs, iterations_hint, pair_iterations, shard_begin) ? NDT_OK : NDT_ERR_INVALID_ARG;
}

int32_t ndt2d_multi_plan(int32_t n_shards, const uint64_t* toff, const uint64_t* soff, size_t n_pairs,
                         int32_t iterations_hint, uint64_t* shard_begin) {
  return ndt2d_multi_plan_hinted(n_shards, toff, soff, n_pairs, iterations_hint, nullptr, shard_begin);
}

int32_t ndt2d_multi_align(ndt2d_multi* m, const float* tx, const float* ty, const uint64_t* toff,
                          const float* sx, const float* sy, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt2d_result* results) {
  const float *const t[2] = {tx, ty}, *const s[2] = {sx, sy};
  return multi_align(m, t, toff, s, soff, init, n_pairs, results);
}

int32_t ndt2d_multi_align_dev(ndt2d_multi* m, const float* const* d_tx, const float* const* d_ty,
                              const uint64_t* const* d_toff, const float* const* d_sx, const float* const* d_sy,
                              const uint64_t* const* d_soff, const double* const* d_init, const size_t* n_pairs,
                              ndt2d_result** d_results_all, size_t* shard_stride, ndt2d_result* results) {
  const float *const *const t[2] = {d_tx, d_ty}, *const *const s[2] = {d_sx, d_sy};
  return multi_align_dev(m, t, d_toff, s, d_soff, d_init, n_pairs, d_results_all, shard_stride, results);
}

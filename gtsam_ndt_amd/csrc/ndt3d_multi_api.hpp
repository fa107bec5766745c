// C-ABI of the multi-device 3D loop-closure context (included at the end of ndt2d_api.hip behind ndt3d_batch_api.hpp):
// ndt_batch_host.hpp's MultiContext over ndt3d_batch contexts (one ndt3d_batch + one host thread per device; the
// device-resident form ends in ONE grouped ncclAllGather of the 408-byte result rows) and the extern "C" shims.
#pragma once

struct ndt3d_multi : ndt::MultiContext<ndt3d_batch> {};

int32_t ndt3d_multi_destroy(ndt3d_multi* m) { return multi_destroy(m); }

int32_t ndt3d_multi_create_pyramid(const ndt3d_params* levels, int32_t n_levels, const int32_t* device_ids,
                                   int32_t n_devices, ndt3d_multi** out) {
  return multi_create_pyramid(levels, n_levels, device_ids, n_devices, out);
}

int32_t ndt3d_multi_create(const ndt3d_params* p, const int32_t* device_ids, int32_t n_devices, ndt3d_multi** out) {
  if (!p) { if (out) *out = nullptr; return NDT_ERR_INVALID_ARG; }
  return ndt3d_multi_create_pyramid(p, 1, device_ids, n_devices, out);
}

int32_t ndt3d_multi_device_count(const ndt3d_multi* m) { return m ? static_cast<int32_t>(m->ctx.size()) : 0; }

int32_t ndt3d_multi_align(ndt3d_multi* m, const float* tx, const float* ty, const float* tz, const uint64_t* toff,
                          const float* sx, const float* sy, const float* sz, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt3d_result* results) {
  const float *const t[3] = {tx, ty, tz}, *const s[3] = {sx, sy, sz};
  return multi_align(m, t, toff, s, soff, init, n_pairs, results);
}

int32_t ndt3d_multi_align_dev(ndt3d_multi* m, const float* const* d_tx, const float* const* d_ty, const float* const* d_tz,
                              const uint64_t* const* d_toff, const float* const* d_sx, const float* const* d_sy,
                              const float* const* d_sz, const uint64_t* const* d_soff, const double* const* d_init,
                              const size_t* n_pairs, ndt3d_result** d_results_all, size_t* shard_stride,
                              ndt3d_result* results) {
  const float *const *const t[3] = {d_tx, d_ty, d_tz}, *const *const s[3] = {d_sx, d_sy, d_sz};
  return multi_align_dev(m, t, d_toff, s, d_soff, d_init, n_pairs, d_results_all, shard_stride, results);
}

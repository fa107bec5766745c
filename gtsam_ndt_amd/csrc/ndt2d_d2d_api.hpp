// Host side of map-to-map alignment, the 2D part (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt2d_d2d.hpp).  The two caches of a handle, the checks, the plan of a multi call and the entry points' bodies are
// ndt_map_host.hpp's, shared with the 3D handle.  The loop of one pair (align_map_pair there) is the launch chain of
// ndt2d_align_dev (ndt_chain_host.hpp: run_chain_tail, fetch_state) on the TARGET handle's stream, context and graph
// cache; the source handle only lends its component list.  Here: that chain's first launch and its kernel.
#pragma once

namespace {

const void* map_iter_kernel(const ndt2d_handle* h) {
  return h->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_iterate_d2d<1> : (const void*)&k_iterate_d2d<0>;
}

void launch_begin_map(ndt2d_handle* t, ndt2d_handle* s, int blocks, const double* pose, int fixed, IterState* host_state,
                      int* host_flag) {
  hipLaunchKernelGGL(k_begin_d2d, dim3(1), dim3(kBlock), 0, t->stream, t->d_map_call, t->d_dyn, (const float4*)s->d_comp,
                     (const float4*)t->d_cov, s->n_comp, blocks, pose[0], pose[1], pose[2], fixed, host_state, host_flag,
                     t->flight.call_seq);
}

int32_t run_map_multi_chain(ndt2d_handle* t, const StartPoses& sp, const StartMaps& sm, int m, int max_blocks, int fixed, int K) {
  const bool chunked = t->use_graph && fixed == 0;
  hipLaunchKernelGGL(k_begin_d2d_multi, dim3(kMaxStarts), dim3(kBlock), 0, t->stream, t->d_call, t->d_dyn_multi,
                     (const float4*)t->d_cov, sp, sm, m, fixed, chunked ? t->h_state_multi : (IterState*)nullptr,
                     chunked ? t->h_flag : (int*)nullptr, t->flight.call_seq);
  HIP_TRY(hipGetLastError());
  const void* solve = (const void*)&k_multi_solve;
  const void* body = t->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_multi_body_d2d<1> : (const void*)&k_multi_body_d2d<0>;
  if (t->use_graph)
    return run_map_multi_graph(t, solve, body, m, max_blocks, chunked ? t->check_every + (t->check_every & 1) : K + 1, chunked, K);
  // plain launches, in the graph's shapes; converged mode: the count of finished starts is polled every check_every
  // pairs, as run_chain_tail polls a single pair's state
  const dim3 gs(pow2_at_least(m)), gb(pow2_at_least(max_blocks), gs.x);
  int k = 0;
  for (; k <= K; ++k) {
    (void)launch_chain_kernel(solve, gs, dim3(kBlock), t->d_static, t->d_call, t->d_dyn_multi, k & 1, t->stream);
    (void)launch_chain_kernel(body, gb, dim3(kBlock), t->d_static, t->d_call, t->d_dyn_multi, k & 1, t->stream);
    if (fixed == 0 && k < K && (k % t->check_every) == t->check_every - 1) {
      int through = 0;
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&through, &t->d_dyn_multi->starts_done, sizeof through, hipMemcpyDeviceToHost, t->stream));
      HIP_TRY(hipStreamSynchronize(t->stream));
      if (through >= m) { ++k; break; }
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(t->h_state_multi, t->d_dyn_multi->state[(k - 1) & 1], kMaxStarts * sizeof(IterState),
                         hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_align_map_multi(ndt2d_handle* target, ndt2d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt2d_result* results) {
  return map_multi_entry(target, sources, init_poses, m, results);
}

int32_t ndt2d_evaluate_map(ndt2d_handle* target, ndt2d_handle* source, const double pose[3], ndt2d_eval* out) {
  return map_pair_entry(target, source, pose, /*fixed_override=*/1, out);
}

int32_t ndt2d_align_map(ndt2d_handle* target, ndt2d_handle* source, const double init_pose[3], ndt2d_result* out) {
  return map_pair_entry(target, source, init_pose, -1, out);
}

int32_t ndt2d_get_components(ndt2d_handle* h, float* mean_xy, float* cov_abc, int32_t* key, int32_t capacity, int32_t* n) {
  return get_components(h, mean_xy, cov_abc, key, capacity, n);
}

}  // extern "C"

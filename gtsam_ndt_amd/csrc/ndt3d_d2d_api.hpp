// Host side of map-to-map alignment, the 3D part (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt3d_d2d.hpp).  The two caches of a handle, the checks, the plan of a multi call and the entry points' bodies are
// ndt_map_host.hpp's, shared with the 2D handle.  The loop of one pair (align_map_pair there) is the launch chain of
// ndt3d_align_dev (ndt_chain_host.hpp: run_chain_tail, fetch_state) on the TARGET handle's stream, context and graph
// cache; the source handle only lends its component list.  Here: that chain's first launch and its kernel.
#pragma once

namespace {

// The template arguments of a 3D map-to-map kernel: f(MODE, NB) with the TARGET's Hessian and map neighbourhood (with_mode3
// for the setting map-to-map alignment has of its own)
template <class F>
auto with_map_mode3(const ndt3d_handle* t, F&& f) {
  return with_mode(t->prm, [&](auto M, auto) {
    return t->map_neighbourhood == 7 ? f(M, std::integral_constant<int, 7>{}) : f(M, std::integral_constant<int, 1>{});
  });
}

const void* map_iter_kernel(const ndt3d_handle* t) {
  return with_map_mode3(t, [](auto M, auto NB) { return (const void*)&ndt::k_iterate_d2d3<M, NB>; });
}

void launch_begin_map(ndt3d_handle* t, ndt3d_handle* s, int blocks, const double* pose, int fixed, ndt::IterState3* host_state,
                      int* host_flag) {
  hipLaunchKernelGGL(ndt::k_begin_d2d3, dim3(1), dim3(ndt::kBlock), 0, t->stream, t->d_map_call, t->d_dyn, (const float4*)s->d_comp,
                     (const float4*)t->d_cov, s->n_comp, blocks, pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], fixed,
                     host_state, host_flag, t->flight.call_seq);
}

// Two launches begin the chain: StartPoses3 plus StartMaps3 do not fit one kernel-argument block.  The solve is
// k_multi_solve3<0> in both Hessian modes: the body writes the 29 sums of the Gauss-Newton layout.
int32_t run_map_multi_chain(ndt3d_handle* t, const ndt::StartPoses3& sp, const ndt::StartMaps3& sm, int m, int max_blocks, int fixed, int K) {
  using namespace ndt;
  const bool converged_mode = fixed == 0;
  hipLaunchKernelGGL(k_begin_d2d_multi3_maps, dim3(kMaxStarts3), dim3(kBlock), 0, t->stream, t->d_dyn_multi, sm, m);
  hipLaunchKernelGGL(k_begin_d2d_multi3, dim3(1), dim3(64), 0, t->stream, t->d_call, t->d_dyn_multi, (const float4*)t->d_cov, sp,
                     m, fixed, converged_mode ? t->h_state_multi : (IterState3*)nullptr,
                     converged_mode ? t->h_flag : (int*)nullptr, t->flight.call_seq);
  HIP_TRY(hipGetLastError());
  const void* solve = (const void*)&k_multi_solve3<0>;
  const void* body = with_map_mode3(t, [](auto M, auto NB) { return (const void*)&k_multi_body_d2d3<M, NB>; });
  return run_map_multi_graph(t, solve, body, m, max_blocks, converged_mode ? t->check_every : K + 1, converged_mode, K);
}

}  // namespace

extern "C" {

int32_t ndt3d_align_map_multi(ndt3d_handle* target, ndt3d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt3d_result* results) {
  return map_multi_entry(target, sources, init_poses, m, results);
}

int32_t ndt3d_evaluate_map(ndt3d_handle* target, ndt3d_handle* source, const double pose[6], ndt3d_eval* out) {
  return map_pair_entry(target, source, pose, /*fixed_override=*/1, out);
}

int32_t ndt3d_align_map(ndt3d_handle* target, ndt3d_handle* source, const double init_pose[6], ndt3d_result* out) {
  return map_pair_entry(target, source, init_pose, -1, out);
}

int32_t ndt3d_get_components(ndt3d_handle* h, float* mean_xyz, float* cov6, int32_t* key, int32_t capacity, int32_t* n) {
  return get_components(h, mean_xyz, cov6, key, capacity, n);
}

}  // extern "C"

// Host side of map-to-map alignment, the 3D part (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt3d_d2d.hpp).  The two caches of a handle, the checks, the plan of a multi call and the entry points' bodies are
// ndt_map_host.hpp's, shared with the 2D handle.  The loop itself is the launch chain of ndt3d_align_dev (begin_align3 /
// finish_align3) on the TARGET handle's stream, context and graph cache; the source handle only lends its component list.
#pragma once

namespace {

// run_align3 with the source handle's component list in the place of a scan: the final state is in t->h_state on return.
int32_t align_map_pair(ndt3d_handle* t, ndt3d_handle* s, const double* pose, int fixed_override) {
  using namespace ndt;
  TraceRange range("ndt3d_align_map: Gauss-Newton loop");
  { const int32_t ps = prepare_map_pair(t, s, "alignment: both", pose); if (ps != NDT_OK) return ps; }
  if (s->n_comp < 1 || t->n_valid < 1) {
    *t->h_state = no_cell_state<IterState3>(pose);
    return NDT_OK;
  }
  if (!t->d_map_call) HIP_TRY(hipMalloc((void**)&t->d_map_call, sizeof(MapCall3)));
  const int fixed = fixed_override >= 0 ? fixed_override : t->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : t->prm.max_iterations;
  const int n = s->n_comp;
  const int blocks = capped_blocks(n, kBlock, kMaxBlocks);
  next_seq(&t->call_seq, t->h_flag);
  hipLaunchKernelGGL(k_begin_d2d3, dim3(1), dim3(kBlock), 0, t->stream, t->d_map_call, t->d_dyn, (const float4*)s->d_comp,
                     (const float4*)t->d_cov, n, blocks, pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], fixed,
                     fixed > 0 ? (IterState3*)nullptr : t->h_state, fixed > 0 ? (int*)nullptr : t->h_flag, t->call_seq);
  HIP_TRY(hipGetLastError());
  const void* func = with_mode(t->prm, [](auto M, auto) { return (const void*)&k_iterate_d2d3<M>; });
  const int launches = fixed > 0 ? K + 1 : 8;
  HIP_TRY(t->graphs.get(func, dim3(blocks), dim3(kBlock), (void*)t->d_static, (void*)t->d_map_call, (void*)t->d_dyn, launches,
                        kMapGraphKey | t->prm.hessian_mode, t->stream, &t->graph_exec));
  if (fixed > 0) {
    HIP_TRY(hipGraphLaunch(t->graph_exec, t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t->h_state, &t->d_dyn->state[K & 1], sizeof(IterState3), hipMemcpyDeviceToHost, t->stream));
    t->in_flight = 1;
  } else {
    t->chunk_run.drain = true;                          // the component list belongs to the other handle
    t->chunk_run.seq = t->call_seq;
    HIP_TRY(chunk_run_begin(t->chunk_run, t->graph_exec, t->stream, launches, K + 1));
    t->in_flight = 2;
  }
  return finish_align3(t);              // synchronous: nothing reads the source's list once this returns
}

// Two launches begin the chain: StartPoses3 plus StartMaps3 do not fit one kernel-argument block.  The solve is
// k_multi_solve3<0> in both Hessian modes: the body writes the 29 sums of the Gauss-Newton layout.
int32_t run_map_multi_chain(ndt3d_handle* t, const ndt::StartPoses3& sp, const ndt::StartMaps3& sm, int m, int max_blocks, int fixed, int K) {
  using namespace ndt;
  const bool converged_mode = fixed == 0;
  hipLaunchKernelGGL(k_begin_d2d_multi3_maps, dim3(kMaxStarts3), dim3(kBlock), 0, t->stream, t->d_dyn_multi, sm, m);
  hipLaunchKernelGGL(k_begin_d2d_multi3, dim3(1), dim3(64), 0, t->stream, t->d_call, t->d_dyn_multi, (const float4*)t->d_cov, sp,
                     m, fixed, converged_mode ? t->h_state_multi : (IterState3*)nullptr,
                     converged_mode ? t->h_flag : (int*)nullptr, t->call_seq);
  HIP_TRY(hipGetLastError());
  const int chunk = 8;
  const void* solve = (const void*)&k_multi_solve3<0>;
  const void* body = with_mode(t->prm, [](auto M, auto) { return (const void*)&k_multi_body_d2d3<M>; });
  return run_map_multi_graph(t, solve, body, m, max_blocks, converged_mode ? chunk : K + 1, converged_mode, K);
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

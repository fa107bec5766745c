// Host side of map-to-map alignment, the 2D part (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt2d_d2d.hpp).  The two caches of a handle, the checks, the plan of a multi call and the entry points' bodies are
// ndt_map_host.hpp's, shared with the 3D handle.  The loop itself is the launch chain of ndt2d_align_dev on the TARGET
// handle's stream, context and graph cache; the source handle only lends its component list.
#pragma once

namespace {

const void* map_iter_kernel(const ndt2d_handle* h) {
  return h->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_iterate_d2d<1> : (const void*)&k_iterate_d2d<0>;
}

// run_align with the source handle's component list in the place of a scan; the result is fetched as there
// (fetch_state / ndt2d_align_finish's state_to), from the target handle.
int32_t run_align_map(ndt2d_handle* t, ndt2d_handle* s, const double pose[3], int fixed_override) {
  TraceRange range("ndt2d_align_map: Gauss-Newton loop");
  const int check_every = t->check_every;             // (a fixed count is never polled)
  { const int32_t ps = prepare_map_pair(t, s, "alignment: both", pose); if (ps != NDT_OK) return ps; }
  if (s->n_comp < 1 || t->n_valid < 1) {
    t->pending = false;
    *t->h_state = no_cell_state<IterState>(pose);
    t->h_state->done = 2;               // marks "result already on the host"
    return NDT_OK;
  }
  if (!t->d_map_call) HIP_TRY(hipMalloc((void**)&t->d_map_call, sizeof(MapCall)));
  const int fixed = fixed_override >= 0 ? fixed_override : t->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : t->prm.max_iterations;
  const int n = s->n_comp;
  const int blocks = capped_blocks(n, kBlock, kMaxBlocks);
  const bool chunked = t->use_graph && check_every > 0 && fixed == 0;
  next_seq(&t->call_seq, t->h_flag);
  hipLaunchKernelGGL(k_begin_d2d, dim3(1), dim3(kBlock), 0, t->stream, t->d_map_call, t->d_dyn, (const float4*)s->d_comp,
                     (const float4*)t->d_cov, n, blocks, pose[0], pose[1], pose[2], fixed,
                     chunked ? t->h_state : (IterState*)nullptr, chunked ? t->h_flag : (int*)nullptr, t->call_seq);
  HIP_TRY(hipGetLastError());
  const void* func = map_iter_kernel(t);
  int k = 0;
  if (t->use_graph) {
    const int launches = chunked ? check_every + (check_every & 1) : K + 1;
    HIP_TRY(t->graphs.get(func, dim3(blocks), dim3(kBlock), (void*)t->d_static, (void*)t->d_map_call, (void*)t->d_dyn, launches,
                          kMapGraphKey | t->prm.hessian_mode, t->stream, &t->graph_exec));
    if (chunked) {
      t->chunk_run.drain = true;                        // the component list belongs to the other handle
      t->chunk_run.seq = t->call_seq;
      HIP_TRY(chunk_run_begin(t->chunk_run, t->graph_exec, t->stream, launches, K + 1));
      t->pending = false;
      return finish_chunk_run(t);
    }
    HIP_TRY(hipGraphLaunch(t->graph_exec, t->stream));
    k = K + 1;
  } else {
    for (; k <= K; ++k) {
      (void)launch_chain_kernel(func, dim3(blocks), dim3(kBlock), t->d_static, t->d_map_call, t->d_dyn, k & 1, t->stream);
      if (check_every > 0 && fixed == 0 && k < K && (k % check_every) == check_every - 1) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t->h_state, &t->d_dyn->state[k & 1], sizeof(IterState), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (t->h_state->done) { ++k; break; }
      }
    }
  }
  HIP_TRY(hipGetLastError());
  t->last_parity = (k - 1) & 1;
  t->h_state->done = 0;
  t->pending = true;
  return NDT_OK;
}

int32_t align_map_pair(ndt2d_handle* t, ndt2d_handle* s, const double* pose, int fixed_override) {
  const int32_t st = run_align_map(t, s, pose, fixed_override);
  return st != NDT_OK ? st : fetch_state(t);      // synchronises the target's stream: nothing reads the source's list any more
}

int32_t run_map_multi_chain(ndt2d_handle* t, const StartPoses& sp, const StartMaps& sm, int m, int max_blocks, int fixed, int K) {
  const bool chunked = t->use_graph && fixed == 0;
  hipLaunchKernelGGL(k_begin_d2d_multi, dim3(kMaxStarts), dim3(kBlock), 0, t->stream, t->d_call, t->d_dyn_multi,
                     (const float4*)t->d_cov, sp, sm, m, fixed, chunked ? t->h_state_multi : (IterState*)nullptr,
                     chunked ? t->h_flag : (int*)nullptr, t->call_seq);
  HIP_TRY(hipGetLastError());
  const void* solve = (const void*)&k_multi_solve;
  const void* body = t->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_multi_body_d2d<1> : (const void*)&k_multi_body_d2d<0>;
  if (t->use_graph)
    return run_map_multi_graph(t, solve, body, m, max_blocks, chunked ? t->check_every + (t->check_every & 1) : K + 1, chunked, K);
  // plain launches, in the graph's shapes; converged mode: the count of finished starts is polled every check_every
  // pairs, as run_align_map polls its state
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

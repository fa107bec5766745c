// Host side of map-to-map alignment (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt2d_d2d.hpp).  Two caches per handle, both derived from the exact per-cell sums and both dropped by everything that
// changes the grid (grid_changed): the covariance records (the handle as target, and the input of the compaction) and
// the component list (the handle as source).  The loop itself is the launch chain of ndt2d_align_dev on the TARGET
// handle's stream, context and graph cache; the source handle only lends its component list.
#pragma once

namespace {

constexpr int kMapGraphKey = 0x2000000;      // ChainGraphCache key of the k_iterate_d2d chains (| hessian_mode)
// ... and of the k_multi_solve + k_multi_body_d2d chains (| the body's grid width << 8 | hessian_mode; the solve's grid is
// the `blocks` of the key).  Bit 27: multi_align's keys reach bit 26 (64 starts << 20)
constexpr int kMapMultiGraphKey = 0x8000000;

int32_t ensure_cov_records(ndt2d_handle* h) {
  if (h->cov_valid) return NDT_OK;
  const size_t ncell = (size_t)h->grid.W * h->grid.H;
  const size_t nb = (ncell + kBlock - 1) / kBlock;
  HIP_TRY(grow(&h->d_cov, &h->cov_cap, 2 * ncell, 2 * (ncell + ncell / 8)));
  HIP_TRY(grow(&h->d_blk, &h->blk_cap, 2 * nb + 1, 2 * (nb + nb / 8) + 1));
  hipLaunchKernelGGL(k_cov_records, dim3((unsigned)nb), dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points,
                     h->prm.eig_ratio, h->d_cov, h->d_blk);
  HIP_TRY(hipGetLastError());
  h->cov_valid = true;
  h->comp_valid = false;
  return NDT_OK;
}

int32_t ensure_components(ndt2d_handle* h) {
  { const int32_t cs = ensure_cov_records(h); if (cs != NDT_OK) return cs; }
  if (h->comp_valid) return NDT_OK;
  TraceRange range("ndt2d: component list");
  const size_t ncell = (size_t)h->grid.W * h->grid.H;
  const unsigned int nb = (unsigned int)((ncell + kBlock - 1) / kBlock);
  unsigned int* counts = h->d_blk;
  unsigned int* offsets = h->d_blk + nb;
  unsigned int* total = h->d_blk + 2 * (size_t)nb;
  hipLaunchKernelGGL(k_comp_offsets, dim3(1), dim3(kScanThreads), 0, h->stream, (const unsigned int*)counts, nb, offsets, total);
  HIP_TRY(hipGetLastError());
  unsigned int n = 0;                                    // the one copy of the count: it sizes the list
  HIP_TRY(hipMemcpyAsync(&n, total, sizeof n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (n > 0) {
    HIP_TRY(grow(&h->d_comp, &h->comp_cap, 2 * (size_t)n, 2 * ((size_t)n + n / 8)));
    hipLaunchKernelGGL(k_components, dim3(nb), dim3(kBlock), 0, h->stream, (const float4*)h->d_cov, (unsigned int)ncell,
                       (const unsigned int*)offsets, h->d_comp, n);
    HIP_TRY(hipGetLastError());
  }
  h->n_comp = (int)n;
  h->comp_valid = true;
  return NDT_OK;
}

const void* map_iter_kernel(const ndt2d_handle* h) {
  return h->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_iterate_d2d<1> : (const void*)&k_iterate_d2d<0>;
}

// run_align with the source handle's component list in the place of a scan; the result is fetched as there
// (fetch_state / ndt2d_align_finish's state_to), from the target handle.
int32_t run_align_map(ndt2d_handle* t, ndt2d_handle* s, const double pose[3], int fixed_override, int check_every) {
  TraceRange range("ndt2d_align_map: Gauss-Newton loop");
  if (!t->has_target || !s->has_target) return NDT_ERR_NO_TARGET;
  if (t->device != s->device) { set_error("map-to-map alignment: both handles must live on one device"); return NDT_ERR_INVALID_ARG; }
  if (t->prm.overlap_grids == 4 || s->prm.overlap_grids == 4) {
    set_error("map-to-map alignment does not take overlapping grids");
    return NDT_ERR_INVALID_ARG;
  }
  if (!std::isfinite(pose[0]) || !std::isfinite(pose[1]) || !std::isfinite(pose[2])) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(t->device));
  { const int32_t fs = finish_chunk_run(t); if (fs != NDT_OK) return fs; }
  if (s != t) { const int32_t fs = finish_chunk_run(s); if (fs != NDT_OK) return fs; }
  { const int32_t cs = ensure_components(s); if (cs != NDT_OK) return cs; }
  { const int32_t cs = ensure_cov_records(t); if (cs != NDT_OK) return cs; }
  if (s->n_comp < 1 || t->n_valid < 1) {
    t->pending = false;
    *t->h_state = no_cell_state<IterState>(pose);
    t->h_state->done = 2;               // marks "result already on the host"
    return NDT_OK;
  }
  if (s != t) HIP_TRY(order_after(t->stream, s->stream, &s->map_ev));       // the list may still be in flight on s's stream
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

// m map-to-map alignments against t's grid, start k from sources[k]'s component list and init_poses[3k] (no entry of
// sources is null, 1 <= m <= kMaxStarts): the split chain of multi_align with k_multi_body_d2d as its evaluation, on t's
// stream, context and graph cache.  Everything is checked before anything is enqueued; returns once t's stream has
// drained or the chain has said that nothing reads a component list any more.
int32_t run_align_map_multi(ndt2d_handle* t, ndt2d_handle* const* sources, const double* init_poses, int32_t m, ndt2d_result* results) {
  TraceRange range("ndt2d_align_map_multi");
  ndt2d_handle* distinct[kMaxStarts];
  const int nd = distinct_pointers(sources, m, distinct);
  if (!t->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < nd; ++j) if (!distinct[j]->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < nd; ++j)
    if (distinct[j]->device != t->device) { set_error("map-to-map alignment: all handles must live on one device"); return NDT_ERR_INVALID_ARG; }
  bool four = t->prm.overlap_grids == 4;
  for (int j = 0; j < nd; ++j) four = four || distinct[j]->prm.overlap_grids == 4;
  if (four) { set_error("map-to-map alignment does not take overlapping grids"); return NDT_ERR_INVALID_ARG; }
  for (int k = 0; k < 3 * m; ++k) if (!std::isfinite(init_poses[k])) return NDT_ERR_INVALID_ARG;
  if (m < t->map_multi_from) {             // few starts: one single chain after the other costs less than the launch pairs
    for (int k = 0; k < m; ++k) {
      int32_t st = run_align_map(t, sources[k], &init_poses[3 * k], -1, t->check_every);
      if (st == NDT_OK) st = fetch_state(t);
      if (st != NDT_OK) return st;
      state_to(*t->h_state, &results[k]);
    }
    return NDT_OK;
  }
  HIP_TRY(hipSetDevice(t->device));
  { const int32_t fs = finish_chunk_run(t); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < nd; ++j)
    if (distinct[j] != t) { const int32_t fs = finish_chunk_run(distinct[j]); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < nd; ++j) { const int32_t cs = ensure_components(distinct[j]); if (cs != NDT_OK) return cs; }
  { const int32_t cs = ensure_cov_records(t); if (cs != NDT_OK) return cs; }
  // starts whose source has no component (all of them, if the target has no valid cell) are answered here
  StartPoses sp{};
  StartMaps sm{};
  int live = 0, max_blocks = 1;
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 3; ++j) sp.p[k][j] = init_poses[3 * k + j];
    const int n = t->n_valid < 1 ? 0 : sources[k]->n_comp;
    if (n < 1) { state_to(no_cell_state<IterState>(&init_poses[3 * k]), &results[k]); continue; }
    sm.comp[k] = sources[k]->d_comp;
    sm.n[k] = n;
    sm.blocks[k] = capped_blocks(n, kBlock, kMaxBlocks);
    max_blocks = sm.blocks[k] > max_blocks ? sm.blocks[k] : max_blocks;
    ++live;
  }
  if (live == 0) return NDT_OK;
  for (int j = 0; j < nd; ++j)             // a list may still be in flight on its handle's stream
    if (distinct[j] != t) HIP_TRY(order_after(t->stream, distinct[j]->stream, &distinct[j]->map_ev));
  HIP_TRY(ensure_multi_chain(&t->h_state_multi, kMaxStarts, &t->d_dyn_multi, t->stream));
  const int fixed = t->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : t->prm.max_iterations;
  const bool chunked = t->use_graph && fixed == 0;
  next_seq(&t->call_seq, t->h_flag);
  hipLaunchKernelGGL(k_begin_d2d_multi, dim3(kMaxStarts), dim3(kBlock), 0, t->stream, t->d_call, t->d_dyn_multi,
                     (const float4*)t->d_cov, sp, sm, (int)m, fixed, chunked ? t->h_state_multi : (IterState*)nullptr,
                     chunked ? t->h_flag : (int*)nullptr, t->call_seq);
  HIP_TRY(hipGetLastError());
  // launch shapes in powers of two (multi_align's reason): slots past m and workgroups past a start's blocks return at once
  const dim3 gs(pow2_at_least(m)), gb(pow2_at_least(max_blocks), gs.x);
  const void* solve = (const void*)&k_multi_solve;
  const void* body = t->prm.hessian_mode == NDT_HESSIAN_NEWTON ? (const void*)&k_multi_body_d2d<1> : (const void*)&k_multi_body_d2d<0>;
  if (t->use_graph) {
    const int launches = chunked ? t->check_every + (t->check_every & 1) : K + 1;
    hipGraphExec_t exec = nullptr;
    HIP_TRY(t->graphs.get2(solve, gs, dim3(kBlock), body, gb, dim3(kBlock), (void*)t->d_static, (void*)t->d_call, (void*)t->d_dyn_multi,
                           launches, kMapMultiGraphKey | ((int)gb.x << 8) | t->prm.hessian_mode, t->stream, &exec));
    bool seen = true;
    HIP_TRY(run_multi_chain(exec, t->stream, chunked ? t->h_flag : nullptr, launches, K + 1, t->call_seq, t->h_state_multi,
                            t->d_dyn_multi->state[K & 1], kMaxStarts * sizeof(IterState), &seen));
    if (!seen) { set_error("the map-to-map multi-start loop did not report its end"); return NDT_ERR_HIP; }
  } else {
    // plain launches; converged mode: the count of finished starts is polled every check_every pairs, as run_align_map
    // polls its state
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
  }
  for (int k = 0; k < m; ++k)
    if (sm.n[k] > 0) state_to(t->h_state_multi[k], &results[k]);
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_align_map_multi(ndt2d_handle* target, ndt2d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt2d_result* results) {
  if (!target || !sources || !init_poses || !results) return NDT_ERR_INVALID_ARG;
  if (m < 1 || m > kMaxStarts) return NDT_ERR_INVALID_ARG;
  for (int32_t k = 0; k < m; ++k) if (!sources[k]) return NDT_ERR_INVALID_ARG;
  return run_align_map_multi(target, sources, init_poses, m, results);
}

int32_t ndt2d_evaluate_map(ndt2d_handle* target, ndt2d_handle* source, const double pose[3], ndt2d_eval* out) {
  if (!target || !source || !pose || !out) return NDT_ERR_INVALID_ARG;
  int32_t st = run_align_map(target, source, pose, /*fixed_override=*/1, /*check_every=*/0);
  if (st != NDT_OK) return st;
  st = fetch_state(target);              // synchronises the target's stream: nothing reads the source's list any more
  if (st != NDT_OK) return st;
  state_to(*target->h_state, out);
  return NDT_OK;
}

int32_t ndt2d_align_map(ndt2d_handle* target, ndt2d_handle* source, const double init_pose[3], ndt2d_result* out) {
  if (!target || !source || !init_pose || !out) return NDT_ERR_INVALID_ARG;
  int32_t st = run_align_map(target, source, init_pose, -1, target->check_every);
  if (st != NDT_OK) return st;
  st = fetch_state(target);
  if (st != NDT_OK) return st;
  state_to(*target->h_state, out);
  return NDT_OK;
}

int32_t ndt2d_get_components(ndt2d_handle* h, float* mean_xy, float* cov_abc, int32_t* key, int32_t capacity, int32_t* n) {
  if (!h || capacity < 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  if (h->prm.overlap_grids == 4) { set_error("map-to-map alignment does not take overlapping grids"); return NDT_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish_chunk_run(h); if (fs != NDT_OK) return fs; }
  { const int32_t cs = ensure_components(h); if (cs != NDT_OK) return cs; }
  if (n) *n = h->n_comp;
  if (!mean_xy && !cov_abc && !key) return NDT_OK;
  if (capacity < h->n_comp) return NDT_ERR_CAPACITY;
  if (h->n_comp == 0) return NDT_OK;
  const size_t nc = (size_t)h->n_comp;
  float4* c = new (std::nothrow) float4[2 * nc];
  if (!c) return NDT_ERR_ALLOC;
  hipError_t e = hipMemcpyAsync(c, h->d_comp, 2 * nc * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { delete[] c; HIP_TRY(e); }
  for (size_t i = 0; i < nc; ++i) {
    const float4 a = c[2 * i], b = c[2 * i + 1];
    if (mean_xy) { mean_xy[2 * i] = a.x; mean_xy[2 * i + 1] = a.y; }
    if (cov_abc) { cov_abc[3 * i] = a.z; cov_abc[3 * i + 1] = a.w; cov_abc[3 * i + 2] = b.y; }
    if (key) { int32_t kk; std::memcpy(&kk, &b.z, sizeof kk); key[i] = kk; }
  }
  delete[] c;
  return NDT_OK;
}

}  // extern "C"

// Host side of 3D map-to-map alignment (included at the end of ndt2d_api.hip: one translation unit; kernels in
// ndt3d_d2d.hpp).  Two caches per handle, both derived from the exact per-voxel sums and both dropped by everything that
// changes the grid (grid_changed3): the covariance records (the handle as target, and the input of the compaction) and
// the component list (the handle as source).  The loop itself is the launch chain of ndt3d_align_dev (begin_align3 /
// finish_align3) on the TARGET handle's stream, context and graph cache; the source handle only lends its component list.
#pragma once

namespace {

constexpr int kMapGraphKey3 = 0x2000000;     // ChainGraphCache key of the k_iterate_d2d3 chains (| hessian_mode)
// ... and of the k_multi_solve3<0> + k_multi_body_d2d3 chains (| the body's grid width << 8 | hessian_mode; the solve's
// grid is the `blocks` of the key).  Bit 27: multi_align3's keys are 0x100000 | up to 64 << 8
constexpr int kMapMultiGraphKey3 = 0x8000000;

int32_t ensure_cov_records3(ndt3d_handle* h) {
  using namespace ndt;
  if (h->cov_valid) return NDT_OK;
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.D;
  const size_t nb = (ncell + kBlock - 1) / kBlock;
  // 48 bytes per voxel of the grid, valid or not: 6 GB at the 2^27-voxel limit of a handle
  if (grow(&h->d_cov, &h->cov_cap, 3 * ncell, 3 * (ncell + ncell / 8)) != hipSuccess ||
      grow(&h->d_blk, &h->blk_cap, 2 * nb + 1, 2 * (nb + nb / 8) + 1) != hipSuccess) {
    (void)hipGetLastError();
    set_error("map-to-map alignment: no device memory for the covariance records (48 bytes per voxel of the grid)");
    return NDT_ERR_ALLOC;
  }
  hipLaunchKernelGGL(k_cov_records3, dim3((unsigned)nb), dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points,
                     h->prm.eig_ratio, h->d_cov, h->d_blk);
  HIP_TRY(hipGetLastError());
  h->cov_valid = true;
  h->comp_valid = false;
  return NDT_OK;
}

int32_t ensure_components3(ndt3d_handle* h) {
  using namespace ndt;
  { const int32_t cs = ensure_cov_records3(h); if (cs != NDT_OK) return cs; }
  if (h->comp_valid) return NDT_OK;
  TraceRange range("ndt3d: component list");
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.D;
  const unsigned int nb = (unsigned int)((ncell + kBlock - 1) / kBlock);
  unsigned int* counts = h->d_blk;
  unsigned int* offsets = h->d_blk + nb;
  unsigned int* total = h->d_blk + 2 * (size_t)nb;
  hipLaunchKernelGGL(k_comp_offsets, dim3(1), dim3(kScanThreads), 0, h->stream, (const unsigned int*)counts, nb, offsets, total);
  HIP_TRY(hipGetLastError());
  unsigned int* hn = (unsigned int*)h->h_small;          // pinned; free between builds (their read-backs are consumed at once)
  HIP_TRY(hipMemcpyAsync(hn, total, sizeof *hn, hipMemcpyDeviceToHost, h->stream));      // the one copy of the count: it sizes the list
  HIP_TRY(hipStreamSynchronize(h->stream));
  const unsigned int n = *hn;                            // <= the voxel count <= 2^27, so it fits n_comp
  if (n > 0) {
    if (grow(&h->d_comp, &h->comp_cap, 3 * (size_t)n, 3 * ((size_t)n + n / 8)) != hipSuccess) {
      (void)hipGetLastError();
      set_error("map-to-map alignment: no device memory for the component list (48 bytes per valid voxel)");
      return NDT_ERR_ALLOC;
    }
    hipLaunchKernelGGL(k_components3, dim3(nb), dim3(kBlock), 0, h->stream, (const float4*)h->d_cov, (unsigned int)ncell,
                       (const unsigned int*)offsets, h->d_comp, n);
    HIP_TRY(hipGetLastError());
  }
  h->n_comp = (int)n;
  h->comp_valid = true;
  return NDT_OK;
}

// run_align3 with the source handle's component list in the place of a scan: the final state is in t->h_state on return.
int32_t run_align_map3(ndt3d_handle* t, ndt3d_handle* s, const double pose[6], int fixed_override) {
  using namespace ndt;
  TraceRange range("ndt3d_align_map: Gauss-Newton loop");
  if (!t->has_target || !s->has_target) return NDT_ERR_NO_TARGET;
  if (t->device != s->device) { set_error("map-to-map alignment: both handles must live on one device"); return NDT_ERR_INVALID_ARG; }
  for (int j = 0; j < 6; ++j) if (!std::isfinite(pose[j])) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(t->device));
  { const int32_t fs = finish_align3(t); if (fs != NDT_OK) return fs; }
  if (s != t) { const int32_t fs = finish_align3(s); if (fs != NDT_OK) return fs; }
  { const int32_t cs = ensure_components3(s); if (cs != NDT_OK) return cs; }
  { const int32_t cs = ensure_cov_records3(t); if (cs != NDT_OK) return cs; }
  if (s->n_comp < 1 || t->n_valid < 1) {
    *t->h_state = no_cell_state<IterState3>(pose);
    return NDT_OK;
  }
  if (s != t) HIP_TRY(order_after(t->stream, s->stream, &s->map_ev));       // the list may still be in flight on s's stream
  if (!t->d_map_call) HIP_TRY(hipMalloc((void**)&t->d_map_call, sizeof(MapCall3)));
  const int fixed = fixed_override >= 0 ? fixed_override : t->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : t->prm.max_iterations;
  const int n = s->n_comp;
  int blocks = (n + kBlock - 1) / kBlock;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  next_seq(&t->call_seq, t->h_flag);
  hipLaunchKernelGGL(k_begin_d2d3, dim3(1), dim3(kBlock), 0, t->stream, t->d_map_call, t->d_dyn, (const float4*)s->d_comp,
                     (const float4*)t->d_cov, n, blocks, pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], fixed,
                     fixed > 0 ? (IterState3*)nullptr : t->h_state, fixed > 0 ? (int*)nullptr : t->h_flag, t->call_seq);
  HIP_TRY(hipGetLastError());
  const void* func = with_mode(t->prm, [](auto M, auto) { return (const void*)&k_iterate_d2d3<M>; });
  const int launches = fixed > 0 ? K + 1 : 8;
  HIP_TRY(t->graphs.get(func, dim3(blocks), dim3(kBlock), (void*)t->d_static, (void*)t->d_map_call, (void*)t->d_dyn, launches,
                        kMapGraphKey3 | t->prm.hessian_mode, t->stream, &t->graph_exec));
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

// m map-to-map alignments against t's grid, start k from sources[k]'s component list and init_poses[6k] (no entry of
// sources is null, 1 <= m <= kMaxStarts3): the split chain of multi_align3 with k_multi_body_d2d3 as its evaluation, on
// t's stream, context and graph cache.  Everything is checked before anything is enqueued; returns once t's stream has
// drained or the chain has said that nothing reads a component list any more.
int32_t run_align_map_multi3(ndt3d_handle* t, ndt3d_handle* const* sources, const double* init_poses, int32_t m, ndt3d_result* results) {
  using namespace ndt;
  TraceRange range("ndt3d_align_map_multi");
  ndt3d_handle* distinct[kMaxStarts3];
  const int nd = distinct_pointers(sources, m, distinct);
  if (!t->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < nd; ++j) if (!distinct[j]->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < nd; ++j)
    if (distinct[j]->device != t->device) { set_error("map-to-map alignment: all handles must live on one device"); return NDT_ERR_INVALID_ARG; }
  for (int k = 0; k < 6 * m; ++k) if (!std::isfinite(init_poses[k])) return NDT_ERR_INVALID_ARG;
  if (m < t->map_multi_from) {             // few starts: one single chain after the other costs less than the launch pairs
    for (int k = 0; k < m; ++k) {
      const int32_t st = run_align_map3(t, sources[k], &init_poses[6 * k], -1);
      if (st != NDT_OK) return st;
      state3_to(*t->h_state, &results[k]);
    }
    return NDT_OK;
  }
  HIP_TRY(hipSetDevice(t->device));
  { const int32_t fs = finish_align3(t); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < nd; ++j)
    if (distinct[j] != t) { const int32_t fs = finish_align3(distinct[j]); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < nd; ++j) { const int32_t cs = ensure_components3(distinct[j]); if (cs != NDT_OK) return cs; }
  { const int32_t cs = ensure_cov_records3(t); if (cs != NDT_OK) return cs; }
  // starts whose source has no component (all of them, if the target has no valid voxel) are answered here
  StartPoses3 sp{};
  StartMaps3 sm{};
  int live = 0, max_blocks = 1;
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 6; ++j) sp.p[k][j] = init_poses[6 * k + j];
    const int n = t->n_valid < 1 ? 0 : sources[k]->n_comp;
    if (n < 1) { state3_to(no_cell_state<IterState3>(&init_poses[6 * k]), &results[k]); continue; }
    sm.comp[k] = sources[k]->d_comp;
    sm.n[k] = n;
    sm.blocks[k] = capped_blocks(n, kBlock, kMaxBlocks);
    max_blocks = sm.blocks[k] > max_blocks ? sm.blocks[k] : max_blocks;
    ++live;
  }
  if (live == 0) return NDT_OK;
  for (int j = 0; j < nd; ++j)             // a list may still be in flight on its handle's stream
    if (distinct[j] != t) HIP_TRY(order_after(t->stream, distinct[j]->stream, &distinct[j]->map_ev));
  HIP_TRY(ensure_multi_chain(&t->h_state_multi, kMaxStarts3, &t->d_dyn_multi, t->stream));
  const int fixed = t->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : t->prm.max_iterations;
  const bool converged_mode = fixed == 0;
  next_seq(&t->call_seq, t->h_flag);
  hipLaunchKernelGGL(k_begin_d2d_multi3_maps, dim3(kMaxStarts3), dim3(kBlock), 0, t->stream, t->d_dyn_multi, sm, (int)m);
  hipLaunchKernelGGL(k_begin_d2d_multi3, dim3(1), dim3(64), 0, t->stream, t->d_call, t->d_dyn_multi, (const float4*)t->d_cov, sp,
                     (int)m, fixed, converged_mode ? t->h_state_multi : (IterState3*)nullptr,
                     converged_mode ? t->h_flag : (int*)nullptr, t->call_seq);
  HIP_TRY(hipGetLastError());
  // launch shapes in powers of two (multi_align3's reason): slots past m and workgroups past a start's blocks return at
  // once.  The solve is k_multi_solve3<0> in both Hessian modes: the body writes the 29 sums of the Gauss-Newton layout
  const int chunk = 8;
  const int steps = converged_mode ? chunk : K + 1;
  const dim3 gs(pow2_at_least(m)), gb(pow2_at_least(max_blocks), gs.x);
  const void* solve = (const void*)&k_multi_solve3<0>;
  const void* body = with_mode(t->prm, [](auto M, auto) { return (const void*)&k_multi_body_d2d3<M>; });
  hipGraphExec_t exec = nullptr;
  HIP_TRY(t->graphs.get2(solve, gs, dim3(kBlock), body, gb, dim3(kBlock), (void*)t->d_static, (void*)t->d_call, (void*)t->d_dyn_multi,
                         steps, kMapMultiGraphKey3 | ((int)gb.x << 8) | t->prm.hessian_mode, t->stream, &exec));
  bool seen = true;
  HIP_TRY(run_multi_chain(exec, t->stream, converged_mode ? t->h_flag : nullptr, steps, K + 1, t->call_seq, t->h_state_multi,
                          t->d_dyn_multi->state[K & 1], kMaxStarts3 * sizeof(IterState3), &seen));
  if (!seen) { set_error("the 3D map-to-map multi-start loop did not report its end"); return NDT_ERR_HIP; }
  for (int k = 0; k < m; ++k)
    if (sm.n[k] > 0) state3_to(t->h_state_multi[k], &results[k]);
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt3d_align_map_multi(ndt3d_handle* target, ndt3d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt3d_result* results) {
  if (!target || !sources || !init_poses || !results) return NDT_ERR_INVALID_ARG;
  if (m < 1 || m > ndt::kMaxStarts3) return NDT_ERR_INVALID_ARG;
  for (int32_t k = 0; k < m; ++k) if (!sources[k]) return NDT_ERR_INVALID_ARG;
  return run_align_map_multi3(target, sources, init_poses, m, results);
}

int32_t ndt3d_evaluate_map(ndt3d_handle* target, ndt3d_handle* source, const double pose[6], ndt3d_eval* out) {
  if (!target || !source || !pose || !out) return NDT_ERR_INVALID_ARG;
  const int32_t st = run_align_map3(target, source, pose, /*fixed_override=*/1);
  if (st != NDT_OK) return st;
  state3_to(*target->h_state, out);
  return NDT_OK;
}

int32_t ndt3d_align_map(ndt3d_handle* target, ndt3d_handle* source, const double init_pose[6], ndt3d_result* out) {
  if (!target || !source || !init_pose || !out) return NDT_ERR_INVALID_ARG;
  const int32_t st = run_align_map3(target, source, init_pose, -1);
  if (st != NDT_OK) return st;
  state3_to(*target->h_state, out);
  return NDT_OK;
}

int32_t ndt3d_get_components(ndt3d_handle* h, float* mean_xyz, float* cov6, int32_t* key, int32_t capacity, int32_t* n) {
  if (!h || capacity < 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish_align3(h); if (fs != NDT_OK) return fs; }
  { const int32_t cs = ensure_components3(h); if (cs != NDT_OK) return cs; }
  if (n) *n = h->n_comp;
  if (!mean_xyz && !cov6 && !key) return NDT_OK;
  if (capacity < h->n_comp) return NDT_ERR_CAPACITY;
  if (h->n_comp == 0) return NDT_OK;
  const size_t nc = (size_t)h->n_comp;
  float4* c = new (std::nothrow) float4[3 * nc];
  if (!c) return NDT_ERR_ALLOC;
  hipError_t e = hipMemcpyAsync(c, h->d_comp, 3 * nc * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { delete[] c; HIP_TRY(e); }
  for (size_t i = 0; i < nc; ++i) {
    const float4 a = c[3 * i], b = c[3 * i + 1], d = c[3 * i + 2];
    if (mean_xyz) { mean_xyz[3 * i] = a.x; mean_xyz[3 * i + 1] = a.y; mean_xyz[3 * i + 2] = a.z; }
    if (cov6) { cov6[6 * i] = b.x; cov6[6 * i + 1] = b.y; cov6[6 * i + 2] = b.z; cov6[6 * i + 3] = b.w; cov6[6 * i + 4] = d.x; cov6[6 * i + 5] = d.y; }
    if (key) { int32_t kk; std::memcpy(&kk, &a.w, sizeof kk); key[i] = kk; }
  }
  delete[] c;
  return NDT_OK;
}

}  // extern "C"

// The host protocol of map-to-map alignment that the 2D and the 3D handle share (included behind ndt_coarsen.hpp and in
// front of ndt2d_d2d_api.hpp and ndt3d_d2d_api.hpp: one translation unit), as function templates over the handle type;
// what differs per dimension is HandleTraits<Handle>'s (next to each handle).  Two caches per handle, both derived from
// the exact per-cell sums and both dropped by everything that changes the grid (grid_changed, grid_changed3): the
// covariance records (the handle as target, and the input of the compaction) and the component list (the handle as
// source).  A call runs on the TARGET handle's stream, context and graph cache; a source handle only lends its list.
#pragma once

namespace {

// ChainGraphCache key of the k_iterate_d2d / k_iterate_d2d3 chains (| HandleTraits::map_graph_mode of the target: the
// Hessian mode in bit 0 and, 3D, the map neighbourhood in bit 4 - the cache compares keys, not kernels, and a handle
// switched between the neighbourhoods must never replay the other one's graph)
constexpr int kMapGraphKey = 0x2000000;
// ... and of the k_multi_solve + k_multi_body_d2d / k_multi_solve3<0> + k_multi_body_d2d3 chains (| the body's grid width
// << 8 | map_graph_mode; the solve's grid is the `blocks` of the key).  Bit 27: multi_align's keys reach bit 26 (64 starts
// << 20), multi_align3's are 0x100000 | up to 64 << 8
constexpr int kMapMultiGraphKey = 0x8000000;

// Per dimension (ndt2d_d2d_api.hpp, ndt3d_d2d_api.hpp).  The one launch of a single pair's chain that differs, its
// first (k_begin_d2d, k_begin_d2d3): s's component list against t's covariance records from `pose`, `blocks` workgroups
// per launch; and the kernel of the launches behind it.
void launch_begin_map(ndt2d_handle* t, ndt2d_handle* s, int blocks, const double* pose, int fixed, IterState* host_state, int* host_flag);
void launch_begin_map(ndt3d_handle* t, ndt3d_handle* s, int blocks, const double* pose, int fixed, IterState3* host_state, int* host_flag);
const void* map_iter_kernel(const ndt2d_handle* t);
const void* map_iter_kernel(const ndt3d_handle* t);
// The chain of a multi call whose plan is made: the first launch from sp and sm, then solve and body `K` + 1 times or
// until every start is through (fixed == 0); the final states are in t->h_state_multi on return.
int32_t run_map_multi_chain(ndt2d_handle* t, const StartPoses& sp, const StartMaps& sm, int m, int max_blocks, int fixed, int K);
int32_t run_map_multi_chain(ndt3d_handle* t, const StartPoses3& sp, const StartMaps3& sm, int m, int max_blocks, int fixed, int K);

// Out of device memory for one of the caches: the covariance records, or (list = true) the component list
template <class H>
int32_t map_alloc_failed(bool list) {
  using T = HandleTraits<H>;
  (void)hipGetLastError();
  last_error() = std::string("map-to-map alignment: no device memory for the ") + (list ? "component list (" : "covariance records (") +
                 std::to_string(16 * T::kRecord) + " bytes per " + (list ? "valid " : "") + T::kCell + (list ? ")" : " of the grid)");
  return NDT_ERR_ALLOC;
}

template <class H>
int32_t ensure_cov_records(H* h) {
  using T = HandleTraits<H>;
  if (h->cov_valid) return NDT_OK;
  const size_t ncell = T::cells(h);
  const size_t nb = (ncell + kBlock - 1) / kBlock;
  // a record per cell of the grid, valid or not: 6 GB at the 2^27-voxel limit of a 3D handle
  if (grow(&h->d_cov, &h->cov_cap, T::kRecord * ncell, T::kRecord * (ncell + ncell / 8)) != hipSuccess ||
      grow(&h->d_blk, &h->blk_cap, 2 * nb + 1, 2 * (nb + nb / 8) + 1) != hipSuccess)
    return map_alloc_failed<H>(false);
  T::launch_cov_records(h, (unsigned)nb);
  HIP_TRY(hipGetLastError());
  h->cov_valid = true;
  h->comp_valid = false;
  return NDT_OK;
}

template <class H>
int32_t ensure_components(H* h) {
  using T = HandleTraits<H>;
  { const int32_t cs = ensure_cov_records(h); if (cs != NDT_OK) return cs; }
  if (h->comp_valid) return NDT_OK;
  TraceRange range(T::kTraceComponents);
  const size_t ncell = T::cells(h);
  const unsigned int nb = (unsigned int)((ncell + kBlock - 1) / kBlock);
  unsigned int* counts = h->d_blk;
  unsigned int* offsets = h->d_blk + nb;
  unsigned int* total = h->d_blk + 2 * (size_t)nb;
  hipLaunchKernelGGL(k_comp_offsets, dim3(1), dim3(kScanThreads), 0, h->stream, (const unsigned int*)counts, nb, offsets, total);
  HIP_TRY(hipGetLastError());
  unsigned int* hn = (unsigned int*)h->h_small;          // pinned; free between builds (their read-backs are consumed at once)
  HIP_TRY(hipMemcpyAsync(hn, total, sizeof *hn, hipMemcpyDeviceToHost, h->stream));      // the one copy of the count: it sizes the list
  HIP_TRY(hipStreamSynchronize(h->stream));
  const unsigned int n = *hn;                            // <= the cell count <= 2^27, so it fits n_comp
  if (n > 0) {
    if (grow(&h->d_comp, &h->comp_cap, T::kRecord * (size_t)n, T::kRecord * ((size_t)n + n / 8)) != hipSuccess)
      return map_alloc_failed<H>(true);
    T::launch_components(h, nb, (unsigned int)ncell, (const unsigned int*)offsets, n);
    HIP_TRY(hipGetLastError());
  }
  h->n_comp = (int)n;
  h->comp_valid = true;
  return NDT_OK;
}

// What a map-to-map call refuses about its handles before it looks at anything else: the target t and the n source
// handles src (n = 0: t alone, as the source it is to ndt*_get_components).  who: "alignment: both", "search: both" ...
template <class H>
int32_t check_map_handles(const H* t, H* const* src, int n, const char* who) {
  if (!t->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < n; ++j) if (!src[j]->has_target) return NDT_ERR_NO_TARGET;
  for (int j = 0; j < n; ++j)
    if (src[j]->device != t->device) {
      last_error() = std::string("map-to-map ") + who + " handles must live on one device";
      return NDT_ERR_INVALID_ARG;
    }
  bool four = t->prm.overlap_grids == 4;                 // (ndt3d_create refuses them: never true of a 3D handle)
  for (int j = 0; j < n; ++j) four = four || src[j]->prm.overlap_grids == 4;
  if (four) { set_error("map-to-map alignment does not take overlapping grids"); return NDT_ERR_INVALID_ARG; }
  return NDT_OK;
}

// Finishes what is in flight on the target and on every source, then prepares each source's component list and the
// target's covariance records.  src[0 .. n): distinct handles, t may be among them.
template <class H>
int32_t prepare_map_handles(H* t, H* const* src, int n) {
  HIP_TRY(hipSetDevice(t->device));
  { const int32_t fs = finish(t); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < n; ++j)
    if (src[j] != t) { const int32_t fs = finish(src[j]); if (fs != NDT_OK) return fs; }
  for (int j = 0; j < n; ++j) { const int32_t cs = ensure_components(src[j]); if (cs != NDT_OK) return cs; }
  return ensure_cov_records(t);
}

// t's stream behind every source's: a list may still be in flight on its handle's stream
template <class H>
int32_t order_after_sources(H* t, H* const* src, int n) {
  for (int j = 0; j < n; ++j)
    if (src[j] != t) HIP_TRY(order_after(t->stream, src[j]->stream, &src[j]->map_ev));
  return NDT_OK;
}

// The head of every call on one pair: the checks, the finite-pose test (pose = null: the caller has none), then
// everything above.
template <class H>
int32_t prepare_map_pair(H* t, H* s, const char* who, const double* pose) {
  { const int32_t cs = check_map_handles(t, &s, 1, who); if (cs != NDT_OK) return cs; }
  for (int j = 0; pose && j < HandleTraits<H>::kPose; ++j) if (!std::isfinite(pose[j])) return NDT_ERR_INVALID_ARG;
  { const int32_t ps = prepare_map_handles(t, &s, 1); if (ps != NDT_OK) return ps; }
  return order_after_sources(t, &s, 1);
}

// The head of the calls whose kernels score a component against its own voxel only - the map-to-map searches and pose
// lists (who = "search", "pose list"), the _align forms through them.  The map neighbourhood 7 (ALGORITHM 2.26) is a
// scoring option of the alignment chains alone; these keep the single-voxel score their contracts name, so with 7 set
// on the target they refuse instead of answering another question (what single_voxel_only is to the point searches),
// before any device call.
template <class H>
int32_t prepare_single_voxel_map_pair(H* t, H* s, const char* who) {
  using T = HandleTraits<H>;
  if (T::map_neighbourhood(t) == 7) {
    last_error() = std::string("map-to-map ") + who + ": scores a component against its own voxel only; the target's map neighbourhood "
                   "is 7: call " + T::kMapNeighbourhoodSetter + "(target, 1) first - search with 1, refine with 7 (the map "
                   "neighbourhood is honoured by evaluate_map, align_map and align_map_multi)";
    return NDT_ERR_INVALID_ARG;
  }
  return prepare_map_pair(t, s, (std::string(who) + ": both").c_str(), nullptr);
}

// One alignment of s's component list against t's grid from `pose`, synchronous: the final state is in *t->h_state, and
// nothing reads s's list any more.  fixed_override: >= 0 replaces the handle's fixed_iterations.  The loop is the launch
// chain of ndt*_align_dev (ndt_chain_host.hpp) with the list in the place of a scan: launch 0 is the k_begin_d2d*, so the
// graph starts at parity 0; lane 0; drained, because the list belongs to the other handle.
template <class H>
int32_t align_map_pair(H* t, H* s, const double* pose, int fixed_override) {
  using T = HandleTraits<H>;
  using State = typename T::State;
  TraceRange range(T::kTraceMapPair);
  { const int32_t ps = prepare_map_pair(t, s, "alignment: both", pose); if (ps != NDT_OK) return ps; }
  if (s->n_comp < 1 || t->n_valid < 1) {
    t->flight.how = ChainFlight::kOnHost;
    *t->h_state = no_cell_state<State>(pose);
    return NDT_OK;
  }
  if (!t->d_map_call) HIP_TRY(hipMalloc((void**)&t->d_map_call, sizeof(*t->d_map_call)));
  const ChainPlan p = chain_plan(fixed_override, t->prm.fixed_iterations, t->prm.max_iterations, t->use_graph, t->check_every,
                                 /*first_in_front=*/false);
  const int blocks = capped_blocks(s->n_comp, kBlock, kMaxBlocks);
  next_seq(&t->flight.call_seq, t->h_flag);
  launch_begin_map(t, s, blocks, pose, p.fixed, p.chunked ? t->h_state : (State*)nullptr, p.chunked ? t->h_flag : (int*)nullptr);
  HIP_TRY(hipGetLastError());
  const ChainLaunch c{map_iter_kernel(t), dim3(blocks), dim3(kBlock), t->d_static, t->d_map_call, t->d_dyn};
  { const int32_t cs = run_chain_tail(t, c, kMapGraphKey | T::map_graph_mode(t), 0, t->stream, nullptr, p, /*drain=*/true);
    if (cs != NDT_OK) return cs; }
  return fetch_state(t);
}

// The k_multi_solve* + k_multi_body_d2d* chain of a multi call on t's graph cache: `launches` steps per replay, K + 1
// in all or, with converged = true, until the chain raises t's flag; the final states arrive in t->h_state_multi.
template <class H>
int32_t run_map_multi_graph(H* t, const void* solve, const void* body, int m, int max_blocks, int launches, bool converged, int K) {
  using T = HandleTraits<H>;
  // launch shapes in powers of two (multi_align's reason): slots past m and workgroups past a start's blocks return at once
  const dim3 gs(pow2_at_least(m)), gb(pow2_at_least(max_blocks), gs.x);
  hipGraphExec_t exec = nullptr;
  HIP_TRY(t->graphs.get2(solve, gs, dim3(kBlock), body, gb, dim3(kBlock), (void*)t->d_static, (void*)t->d_call, (void*)t->d_dyn_multi,
                         launches, kMapMultiGraphKey | ((int)gb.x << 8) | T::map_graph_mode(t), t->stream, &exec));
  bool seen = true;
  HIP_TRY(run_multi_chain(exec, t->stream, converged ? t->h_flag : nullptr, launches, K + 1, t->flight.call_seq, t->h_state_multi,
                          t->d_dyn_multi->state[K & 1], T::kMaxStarts * sizeof(typename T::State), &seen));
  if (!seen) { set_error(T::kMapMultiNoEnd); return NDT_ERR_HIP; }
  return NDT_OK;
}

// m map-to-map alignments against t's grid, start k from sources[k]'s component list and init_poses[kPose k] (no entry
// of sources is null, 1 <= m <= kMaxStarts): the split chain of multi_align / multi_align3 with k_multi_body_d2d* as its
// evaluation, on t's stream, context and graph cache.  Everything is checked before anything is enqueued; returns once
// t's stream has drained or the chain has said that nothing reads a component list any more.
template <class H>
int32_t run_align_map_multi(H* t, H* const* sources, const double* init_poses, int32_t m, typename HandleTraits<H>::Result* results) {
  using T = HandleTraits<H>;
  using State = typename T::State;
  TraceRange range(T::kTraceMapMulti);
  H* distinct[T::kMaxStarts];
  const int nd = distinct_pointers(sources, m, distinct);
  { const int32_t cs = check_map_handles(t, distinct, nd, "alignment: all"); if (cs != NDT_OK) return cs; }
  for (int k = 0; k < T::kPose * m; ++k) if (!std::isfinite(init_poses[k])) return NDT_ERR_INVALID_ARG;
  if (m < t->map_multi_from) {             // few starts: one single chain after the other costs less than the launch pairs
    for (int k = 0; k < m; ++k) {
      const int32_t st = align_map_pair(t, sources[k], &init_poses[T::kPose * k], -1);
      if (st != NDT_OK) return st;
      T::to(*t->h_state, &results[k]);
    }
    return NDT_OK;
  }
  { const int32_t ps = prepare_map_handles(t, distinct, nd); if (ps != NDT_OK) return ps; }
  // starts whose source has no component (all of them, if the target has no valid cell) are answered here
  typename T::Poses sp{};
  typename T::Maps sm{};
  int max_blocks = 1;
  const int live = plan_map_starts(sources, init_poses, m, t->n_valid >= 1, kBlock, kMaxBlocks, &sp, &sm, &max_blocks);
  for (int k = 0; k < m; ++k)
    if (sm.n[k] == 0) T::to(no_cell_state<State>(&init_poses[T::kPose * k]), &results[k]);
  if (live == 0) return NDT_OK;
  { const int32_t os = order_after_sources(t, distinct, nd); if (os != NDT_OK) return os; }
  HIP_TRY(ensure_multi_chain(&t->h_state_multi, T::kMaxStarts, &t->d_dyn_multi, t->stream));
  const int fixed = t->prm.fixed_iterations;
  next_seq(&t->flight.call_seq, t->h_flag);
  { const int32_t cs = run_map_multi_chain(t, sp, sm, (int)m, max_blocks, fixed, fixed > 0 ? fixed : t->prm.max_iterations);
    if (cs != NDT_OK) return cs; }
  for (int k = 0; k < m; ++k)
    if (sm.n[k] > 0) T::to(t->h_state_multi[k], &results[k]);
  return NDT_OK;
}

// ndt*_align_map (Out = the result, fixed_override = -1) and ndt*_evaluate_map (Out = the eval, fixed_override = 1)
template <class H, class Out>
int32_t map_pair_entry(H* target, H* source, const double* pose, int fixed_override, Out* out) {
  if (!target || !source || !pose || !out) return NDT_ERR_INVALID_ARG;
  const int32_t st = align_map_pair(target, source, pose, fixed_override);
  if (st != NDT_OK) return st;
  HandleTraits<H>::to(*target->h_state, out);
  return NDT_OK;
}

template <class H>
int32_t map_multi_entry(H* target, H* const* sources, const double* init_poses, int32_t m, typename HandleTraits<H>::Result* results) {
  if (!target || !sources || !init_poses || !results) return NDT_ERR_INVALID_ARG;
  if (m < 1 || m > HandleTraits<H>::kMaxStarts) return NDT_ERR_INVALID_ARG;
  for (int32_t k = 0; k < m; ++k) if (!sources[k]) return NDT_ERR_INVALID_ARG;
  return run_align_map_multi(target, sources, init_poses, m, results);
}

// ndt*_get_components: the count alone (mean, cov and key all null), or the list unpacked by the traits
template <class H>
int32_t get_components(H* h, float* mean, float* cov, int32_t* key, int32_t capacity, int32_t* n) {
  using T = HandleTraits<H>;
  if (!h || capacity < 0) return NDT_ERR_INVALID_ARG;
  { const int32_t cs = check_map_handles(h, (H* const*)nullptr, 0, ""); if (cs != NDT_OK) return cs; }
  { const int32_t ps = prepare_map_handles(h, &h, 1); if (ps != NDT_OK) return ps; }
  if (n) *n = h->n_comp;
  if (!mean && !cov && !key) return NDT_OK;
  if (capacity < h->n_comp) return NDT_ERR_CAPACITY;
  if (h->n_comp == 0) return NDT_OK;
  const size_t nc = (size_t)h->n_comp;
  float4* c = new (std::nothrow) float4[T::kRecord * nc];
  if (!c) return NDT_ERR_ALLOC;
  hipError_t e = hipMemcpyAsync(c, h->d_comp, T::kRecord * nc * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { delete[] c; HIP_TRY(e); }
  for (size_t i = 0; i < nc; ++i) T::unpack_component(c + T::kRecord * i, i, mean, cov, key);
  delete[] c;
  return NDT_OK;
}

}  // namespace

// C-ABI of the 3D SE(3) variant (included at the end of ndt2d_api.hip: one translation unit).
#pragma once
#include <vector>

#include "ndt3d_kernels.hpp"
#include "ndt3d_build.hpp"
#include "ndt3d_multi.hpp"
#include "ndt3d_d2d.hpp"
#include "ndt3d_d2d_multi.hpp"

// h_pub3, the pinned read-back of a single-sync build: the accumulator block's first 64 words, then the flag
constexpr int kPub3FlagWord = 64, kPub3Words = kPub3FlagWord + 16;

struct ndt3d_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  ndt3d_params prm{};
  ndt::Grid3Dev grid{};
  size_t cell_capacity = 0;
  bool has_target = false;
  int n_valid = 0;
  unsigned int* d_bounds = nullptr;   // [6]
  int* d_counters = nullptr;          // [kCountAlloc] counter shards of ndt3d_load_map's finalise and all counts of a merge (the builds keep theirs in d_tiles)
  int publish_seq = 0;                // the flag value of the read-back in flight (publish_and_wait)
  float* d_parts3 = nullptr;          // [256][8]: per-workgroup partial bounding boxes (k_bounds3_parts)
  void* h_small = nullptr;            // pinned kSmallBytes (counter shards at 0, the outside count at 128, a flag)
  float *d_t[3] = {nullptr, nullptr, nullptr}; size_t tcap = 0;
  float *d_b[3] = {nullptr, nullptr, nullptr}; size_t bcap = 0;      // binned build scratch
  unsigned int* d_tiles = nullptr; size_t tile_cap = 0;
  int last_ntile = 0;                 // tiles of the grid the handle holds (0: none): the launch bound of a single-sync build
  unsigned int* h_pub3 = nullptr;     // pinned [kPub3Words]: the accumulator block's first 64 words of a single-sync build, then the flag
  bool one_round_trip = true;
  size_t tiles_clean = 0;             // leading words of d_tiles known to be zero (the last build's publish cleared them)
  unsigned char* d_split3 = nullptr; size_t split3_cap = 0;   // shared tiles' hand-off (ndt3d_build.hpp Split3Bufs): the slab pool
  float *d_s[3] = {nullptr, nullptr, nullptr}; size_t scap = 0;
  ndt::AlignStatic3* d_static = nullptr;
  ndt::AlignCall3* d_call = nullptr;
  ndt::AlignDyn3* d_dyn = nullptr;
  ndt::AlignStatic3* h_static = nullptr;
  hipEvent_t upload_ev = nullptr;     // recorded after the last upload from h_static
  ndt::IterState3* h_state = nullptr;
  unsigned long long* d_outside = nullptr;   // [1] points of the last build / update outside the extent
  int* h_flag = nullptr;              // pinned: raised by the launch that ends a converged-mode loop
  ndt::ChainGraphCache graphs;
  ndt::ChainFlight flight;            // what the last single-pair alignment left in flight (ndt_chain_host.hpp)
  // To the shared chain code this is a handle with one lane that cannot be raised (ndt3d_set_tuning refuses the lane
  // knobs, no secondary stream exists), always on graphs, with chunks of 8 launches.
  ndt::LaneState lanes{1};
  static constexpr bool use_graph = true;
  static constexpr int check_every = 8;
  ndt::AlignDyn3* dyn_of(int) const { return d_dyn; }
  ndt::AlignDynMulti3* d_dyn_multi = nullptr;   // multi-scan / multi-start chains (ndt3d_multi.hpp), on first use
  ndt::IterState3* h_state_multi = nullptr;     // pinned [kMaxStarts3]
  ndt::SearchScratch srch;                      // exhaustive pose search scratch (ndt_search.hpp), allocated on first use
  ndt::PointFitScratch fit;                     // per-point fit and selection scratch (ndt_point_fit.hpp), allocated on first use
  ndt::VoxelFilterScratch vox;                  // voxel-grid scan filter scratch (ndt_voxel_filter.hpp), allocated on first use
  // map-to-map alignment (ndt_map_host.hpp, ndt3d_d2d_api.hpp), allocated on first use; both caches follow the grid (grid_changed3)
  float4* d_cov = nullptr; size_t cov_cap = 0;            // covariance records, 3 float4 per voxel (k_cov_records3)
  unsigned int* d_blk = nullptr; size_t blk_cap = 0;      // per-workgroup valid counts | their exclusive scan | the total
  float4* d_comp = nullptr; size_t comp_cap = 0;          // component list, 3 float4 per component (k_components3)
  int n_comp = 0;
  bool cov_valid = false, comp_valid = false;
  ndt::MapCall3* d_map_call = nullptr;
  int map_multi_from = 2;                                 // ndt3d_align_map_multi calls of this many starts use one chain (NDT_TUNE_MAP_MULTI_FROM)
  bool fused_begin = true;                                // NDT_TUNE_FUSED_BEGIN: launch 0 of a chain is k_iterate3_first (no k_begin3)
  hipEvent_t map_ev = nullptr;                            // orders a target handle's stream behind this handle's (order_after)
  int particle_team = 0;                                  // NDT_TUNE_PARTICLE_TEAM: lanes per pose of ndt3d_score_particles*, 0 = by the list's length
  int neighbourhood = 1;                                  // ndt3d_set_neighbourhood: voxels a point is scored against in the alignment chains (1 or 7)
  int map_neighbourhood = 1;                              // ndt3d_set_map_neighbourhood: voxels a source component is scored against, this handle as TARGET (1 or 7)
};

namespace {

template <> struct HandleTraits<ndt3d_handle>;   // (below; the shared chain code is used before it)

// everything that changes the voxel grid's sums or geometry drops what map-to-map alignment derived from them
void grid_changed3(ndt3d_handle* h) { h->cov_valid = false; h->comp_valid = false; }

int32_t upload_static3(ndt3d_handle* h) {
  // as upload_static in 2D: the copy is left in flight (whatever reads d_static is ordered behind it on the same
  // stream); the pinned source is only rewritten once the previous copy has left it
  HIP_TRY(hipEventSynchronize(h->upload_ev));
  ndt::AlignStatic3* c = h->h_static;
  c->grid = h->grid;
  set_solve_params(&c->prm, h->prm);
  HIP_TRY(hipMemcpyAsync(h->d_static, c, sizeof(ndt::AlignStatic3), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventRecord(h->upload_ev, h->stream));
  return NDT_OK;
}

// The device words and buffers of a binned build of n points over at most `ntile` tiles.
// One block of device words carries everything a build adds into, so that ONE fill clears it (round 2: four) and one
// publish brings the results back:  counter shards [32] | outside count (u64) | pad to 64 (the voxels a removal broke at word
// kCountUnder = 34, the arrival count of k_tile_count3's workgroups at word 41, a device-decided geometry from word kGeom3Word) | tile totals [ntile] | tickets of the shared tiles [ntile] |
// tile starts [ntile + 1] | scatter cursors [ntile] | number of (tile, share) workgroups [1] | their list [wg_bound]
struct Build3Bufs {
  int* d_cnt; unsigned long long* d_out;
  unsigned int *d_total, *d_ticket, *d_start, *d_cursor, *d_wgtotal, *d_wgmap;
  size_t wg_bound, zero_words;
  ndt::Split3Bufs sb;
};
int32_t ensure_build3_bufs(ndt3d_handle* h, size_t n, int ntile, bool binned, Build3Bufs* B) {
  using namespace ndt;
  B->wg_bound = (size_t)ntile + n / (size_t)kTile3SubMin + 1;
  const size_t tneed = 64 + 4 * (size_t)ntile + 4 + 1 + B->wg_bound;
  bool grew = false;
  HIP_TRY(grow(&h->d_tiles, &h->tile_cap, tneed, tneed, &grew));
  if (grew) h->tiles_clean = 0;
  B->d_cnt = reinterpret_cast<int*>(h->d_tiles);
  B->d_out = reinterpret_cast<unsigned long long*>(h->d_tiles + 32);
  B->d_total = h->d_tiles + 64;
  B->d_ticket = B->d_total + ntile;
  B->d_start = B->d_ticket + ntile;
  B->d_cursor = B->d_start + ntile + 1;
  B->d_wgtotal = B->d_cursor + ntile;
  B->d_wgmap = B->d_wgtotal + 1;
  B->zero_words = 64 + 2 * (size_t)ntile;
  B->sb = Split3Bufs{};
  if (!binned) return NDT_OK;
  HIP_TRY(grow({grow_buf(&h->d_b[0]), grow_buf(&h->d_b[1]), grow_buf(&h->d_b[2])}, &h->bcap, n, n + n / 4 + 1024));
  // the shared tiles' slabs: one per workgroup of the tile kernel's launch (only the shares of shared tiles use theirs)
  const size_t slabs = B->wg_bound;
  const size_t need = slabs * kSlabWords * sizeof(unsigned long long);
  HIP_TRY(grow(&h->d_split3, &h->split3_cap, need, need + need / 4));
  B->sb.pool = reinterpret_cast<unsigned long long*>(h->d_split3);
  B->sb.capacity = (unsigned int)(slabs > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : slabs);
  return NDT_OK;
}

// The binned build (ndt3d_build.hpp) of `tiles` tiles into the block of B: count (the scan runs in its last workgroup) ->
// scatter -> tile kernel, for a geometry the host knows (ga = {}: the grid of h->grid; merge = add to the cached sums, mv =
// the motion applied on the way in) or for one the count kernel's prologue decides into ga.out (set_target3_single_sync).
int32_t enqueue_binned_build3(ndt3d_handle* h, const float* dx, const float* dy, const float* dz, size_t n, int tiles,
                              const Build3Bufs& B, bool merge, const ndt::Move3Args& mv, const ndt::Geom3Args& ga, int sign = 1) {
  using namespace ndt;
  const Grid3Dev& g = h->grid;
  const GeomDev3* dg = ga.out;
  const int ntx = dg ? 0 : (g.W + (1 << kT3x) - 1) >> kT3x, nty = dg ? 0 : (g.H + (1 << kT3y) - 1) >> kT3y;
  const BinGeom3 bg = dg ? BinGeom3{} : BinGeom3{g.ox, g.oy, g.oz, g.inv_c, g.W, g.H, g.D, ntx, nty, tiles};
  size_t nb = (n + kBinThreads * 4 - 1) / (kBinThreads * 4);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_tile_count3, dim3((unsigned)nb), dim3(kBinThreads), tiles * sizeof(unsigned int), h->stream, dx, dy, dz, n,
                     bg, B.d_total, B.d_out, ga, Scan3Out{h->d_tiles + 41, B.d_start, B.d_cursor, B.d_wgtotal, B.d_wgmap}, mv);
  hipLaunchKernelGGL(k_tile_scatter3, dim3((unsigned)nb), dim3(kBinThreads), 2 * tiles * sizeof(unsigned int), h->stream, dx, dy, dz,
                     n, bg, B.d_cursor, h->d_b[0], h->d_b[1], h->d_b[2], dg, mv);
  // (no fill of the grid's sums: the workgroup that finishes a tile writes every voxel's sums, empty ones included)
  const auto tile_kernel = sign < 0 ? &k_tile_accumulate3<-1> : &k_tile_accumulate3<1>;       // sign = -1 (with merge): a removal
  hipLaunchKernelGGL(tile_kernel, dim3((unsigned)B.wg_bound), dim3(kBinThreads), 0, h->stream, h->d_b[0], h->d_b[1], h->d_b[2],
                     B.d_start, g, ntx, nty, merge ? 1 : 0, h->prm.min_points, h->prm.eig_ratio, B.d_cnt, B.d_ticket, B.sb,
                     (const unsigned int*)B.d_wgtotal, (const unsigned int*)B.d_wgmap, dg, (const Grid3Dev*)ga.grid);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// The read-back of a build's accumulator block (k_build_publish_clear3 through publish_and_wait): its first `nwords` words
// into pinned memory at h_dst, then `flag` raised; the kernel clears the block's first zero_words words behind it.  The
// kernel's own stores are the only copy, so a flag that has not come even after a synchronisation is an error.
int32_t read_back3(ndt3d_handle* h, unsigned int* h_dst, int nwords, int* flag, size_t zero_words) {
  bool seen = false;
  HIP_TRY(publish_and_wait(h->stream, &h->publish_seq, flag, [&](int seq) {
    hipLaunchKernelGGL(ndt::k_build_publish_clear3, dim3(1), dim3(256), 0, h->stream, h->d_tiles, h_dst, nwords, flag, seq, (int)zero_words);
  }, &seen));
  if (!seen) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!flag_raised(flag, h->publish_seq)) { set_error("the voxel-grid build did not report its end"); return NDT_ERR_HIP; }
  }
  h->tiles_clean = zero_words;
  return NDT_OK;
}

// a2 + a3 for n points into the grid whose geometry and storage are set: binned LDS build, or
// scattered global atomics for maps beyond the tile histogram.  merge = add to the cached sums
// (incremental submap update) instead of starting from zero; sign = -1 (with merge): take the points out of the cached
// sums again - the same kernels with the sign (NDT_ERR_INVALID_ARG when the points are not in the map).
int32_t accumulate3(ndt3d_handle* h, const float* dx, const float* dy, const float* dz, size_t n, bool merge,
                    unsigned long long* h_outside, const ndt::Rigid3F* move = nullptr, int sign = 1) {
  using namespace ndt;
  Grid3Dev& g = h->grid;
  const size_t ncell = (size_t)g.W * g.H * g.D;
  const int ntx = (g.W + (1 << kT3x) - 1) >> kT3x, nty = (g.H + (1 << kT3y) - 1) >> kT3y, ntz = (g.D + (1 << kT3z) - 1) >> kT3z;
  const long long ntile_ll = (long long)ntx * nty * ntz;
  const bool binned = ntile_ll <= kBinMaxTiles && n <= 0xFFFFFFFFull;
  const int ntile = binned ? (int)ntile_ll : 0;
  Build3Bufs B{};
  { const int32_t bs = ensure_build3_bufs(h, n, ntile, binned, &B); if (bs != NDT_OK) return bs; }
  // (the publish of the build before cleared the block, unless this one needs more of it or that one did not finish)
  const bool clean = h->tiles_clean >= B.zero_words;
  h->tiles_clean = 0;
  if (!clean) HIP_TRY(hipMemsetAsync(h->d_tiles, 0, B.zero_words * sizeof(unsigned int), h->stream));
  if (binned) {
    Move3Args mv{};
    if (move) { mv.T = *move; mv.use = 1; }
    { const int32_t bs = enqueue_binned_build3(h, dx, dy, dz, n, ntile, B, merge, mv, Geom3Args{}, sign); if (bs != NDT_OK) return bs; }
    h->last_ntile = ntile;
  } else {
    if (move) {                                      // this path takes the points as they are: move them first
      HIP_TRY(grow({grow_buf(&h->d_t[0]), grow_buf(&h->d_t[1]), grow_buf(&h->d_t[2])}, &h->tcap, n, n + n / 4 + 1024));
      hipLaunchKernelGGL(k_transform_points3, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, dx, dy, dz, n, *move,
                         h->d_t[0], h->d_t[1], h->d_t[2]);
      HIP_TRY(hipGetLastError());
      dx = h->d_t[0]; dy = h->d_t[1]; dz = h->d_t[2];
    }
    if (!merge) HIP_TRY(hipMemsetAsync(g.acc, 0, ncell * sizeof(CellAcc3), h->stream));
    const auto accumulate = sign < 0 ? &k_accumulate3<-1> : &k_accumulate3<1>;
    const auto finalise = sign < 0 ? &k_finalise3<-1> : &k_finalise3<1>;
    hipLaunchKernelGGL(accumulate, dim3(stream_blocks(n)), dim3(kBlock), 0, h->stream, dx, dy, dz, n, g, B.d_out);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(finalise, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, g,
                       h->prm.min_points, h->prm.eig_ratio, B.d_cnt);
    HIP_TRY(hipGetLastError());
  }
  // counter shards and outside count to the host through pinned memory and a flag (as the 2D build)
  int* hc = (int*)h->h_small;
  unsigned long long* ho = (unsigned long long*)((char*)h->h_small + 128);
  { const int32_t rs = read_back3(h, (unsigned int*)hc, kCountWords, small_flag(h->h_small), B.zero_words); if (rs != NDT_OK) return rs; }
  if (h_outside) *h_outside = *ho;
  int n_valid_sum = 0, n_over_sum = 0;
  sum_count_shards(hc, &n_valid_sum, &n_over_sum);
  h->n_valid = n_valid_sum;
  if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
  if (sign < 0 && hc[kCountUnder] > 0) {
    set_error("removed points are not in the target: a voxel's count fell below zero, or reached zero with sums left");
    return NDT_ERR_INVALID_ARG;
  }
  return NDT_OK;
}

// storage for ncell voxels: a 64-byte record (four float4) and the sums of each
int32_t ensure_cells3(ndt3d_handle* h, size_t ncell) {
  HIP_TRY(grow({grow_buf(&h->grid.rec, 4), grow_buf(&h->grid.acc)}, &h->cell_capacity, ncell, ncell + ncell / 8));
  return NDT_OK;
}

// Voxel-grid geometry for a bounding box (oracle/ndt3d.py grid_geometry3) and storage for its voxels.
int32_t setup_geometry3(ndt3d_handle* h, const float lo[3], const float hi[3]) {
  using namespace ndt;
  const double c = h->prm.cell_size;
  Grid3Dev& g = h->grid;
  g.cell = c;
  g.inv_c = lattice_inv_c(c);
  float o[3];
  int dims[3];
  double ncell_d = 1.0;
  for (int a = 0; a < 3; ++a) {
    const LatticeAxis A = lattice_axis(lo[a], hi[a], c);          // the rule the kernels call
    if (!(A.k >= 0.f) || A.k > 1e7f) { set_error("target extent too large for the cell size"); return NDT_ERR_CAPACITY; }
    o[a] = A.origin;
    dims[a] = (int)A.k + 2;
    ncell_d *= dims[a];
  }
  if (ncell_d > (double)kMaxCells) { set_error("3D target needs more than 2^27 cells"); return NDT_ERR_CAPACITY; }
  g.ox = o[0]; g.oy = o[1]; g.oz = o[2];
  g.W = dims[0]; g.H = dims[1]; g.D = dims[2]; g.pad = 0;
  g.fix_scale = std::ldexp(1.0, kFixShift) / c;
  const size_t ncell = (size_t)g.W * g.H * g.D;
  return ensure_cells3(h, ncell);
}

// ndt3d_set_target with ONE host round trip (the 3D twin of the 2D build's set_target_single_sync): a handle that already
// holds a grid enqueues the whole build at once - bounding-box partials (its workgroup 0 clears the accumulators), the count
// kernel whose prologue reduces the box and decides the grid (it must fit the handle's storage and a launch bound of twice
// the cached grid's tiles), scan, scatter, tile kernel with the geometry read from device memory - and one publish of the
// results AND the box.  If
// the grid does not fit, ok = 0 makes every kernel return and the caller builds the usual way with the box it now has.
// The host forms the geometry from the same box afterwards, by the function the kernel called (lattice_axis), and compares:
// the check guards the storage and the launch bound.
int32_t set_target3_single_sync(ndt3d_handle* h, const float* dx, const float* dy, const float* dz, size_t n, bool* done,
                                unsigned int* hb_out, bool* have_bounds) {
  using namespace ndt;
  *done = false; *have_bounds = false;
  if (!h->one_round_trip || h->cell_capacity == 0 || h->last_ntile <= 0 || n > 0xFFFFFFFFull || !h->grid.rec || !h->grid.acc) return NDT_OK;
  long long tb = 2ll * h->last_ntile + 16;
  if (tb > kBinMaxTiles) tb = kBinMaxTiles;
  const int tile_bound = (int)tb;
  if (!h->h_pub3) HIP_TRY(pinned_alloc(&h->h_pub3, kPub3Words * sizeof(unsigned int)));
  if (!h->d_parts3) HIP_TRY(hipMalloc((void**)&h->d_parts3, 256 * 8 * sizeof(float)));
  Build3Bufs B{};
  { const int32_t bs = ensure_build3_bufs(h, n, tile_bound, true, &B); if (bs != NDT_OK) return bs; }
  h->tiles_clean = 0;                                      // (k_bounds3_parts clears the block for this build)
  int sbk = stream_blocks(n);
  if (sbk > 256) sbk = 256;
  HIP_TRY(hipEventSynchronize(h->upload_ev));              // (an upload of d_static still in flight would overwrite the header)
  hipLaunchKernelGGL(k_bounds3_parts, dim3(sbk), dim3(kBlock), 0, h->stream, dx, dy, dz, n, h->d_parts3, h->d_tiles, (int)B.zero_words,
                     kGeom3Word, (int)(sizeof(GeomDev3) / 4));
  Geom3Args ga{};
  ga.parts = h->d_parts3; ga.nparts = sbk; ga.tile_bound = tile_bound; ga.cell = h->prm.cell_size;
  ga.cell_capacity = (unsigned long long)h->cell_capacity; ga.grid = &h->d_static->grid;
  ga.out = reinterpret_cast<GeomDev3*>(h->d_tiles + kGeom3Word);
  { const int32_t bs = enqueue_binned_build3(h, dx, dy, dz, n, tile_bound, B, false, Move3Args{}, ga); if (bs != NDT_OK) return bs; }
  unsigned int* hp = h->h_pub3;
  { const int32_t rs = read_back3(h, hp, 64, reinterpret_cast<int*>(hp + kPub3FlagWord), B.zero_words); if (rs != NDT_OK) return rs; }
  const GeomDev3* hg = reinterpret_cast<const GeomDev3*>(hp + kGeom3Word);
  for (int j = 0; j < 6; ++j) hb_out[j] = hg->bounds[j];
  *have_bounds = true;
  if (!hg->ok) return NDT_OK;                              // does not fit storage or bound (or no finite point): the usual way
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = ordered_to_float(hg->bounds[2 * a]); hi[a] = ordered_to_float(hg->bounds[2 * a + 1]); }
  // the host's view of the same geometry, from the same box; the storage is large enough, nothing is reallocated
  if (setup_geometry3(h, lo, hi) != NDT_OK) return NDT_OK;
  const Grid3Dev& g = h->grid;
  if (g.W != hg->bin.W || g.H != hg->bin.H || g.D != hg->bin.D || g.ox != hg->bin.ox || g.oy != hg->bin.oy || g.oz != hg->bin.oz) return NDT_OK;
  h->last_ntile = hg->bin.ntile;
  int n_valid_sum = 0, n_over_sum = 0;
  sum_count_shards(reinterpret_cast<const int*>(hp), &n_valid_sum, &n_over_sum);
  h->n_valid = n_valid_sum;
  if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
  *done = true;
  return NDT_OK;
}

int32_t set_target3_impl(ndt3d_handle* h, const float* dx, const float* dy, const float* dz, size_t n) {
  using namespace ndt;
  TraceRange range("ndt3d_set_target: voxel grid build");
  h->has_target = false;
  grid_changed3(h);
  unsigned int* hb = (unsigned int*)h->h_small;
  unsigned int fast_bounds[6];
  bool done = false, have_bounds = false;
  { const int32_t fs = set_target3_single_sync(h, dx, dy, dz, n, &done, fast_bounds, &have_bounds); if (fs != NDT_OK) return fs; }
  if (done) {
    h->has_target = true;
    return upload_static3(h);
  }
  if (have_bounds) {
    for (int j = 0; j < 6; ++j) hb[j] = fast_bounds[j];    // the single-sync attempt measured the box already
  } else {
    // bounding box: one partial per workgroup, then one wave reduces them into pinned host memory and raises a flag
    if (!h->d_parts3) HIP_TRY(hipMalloc((void**)&h->d_parts3, 256 * 8 * sizeof(float)));
    int sb = stream_blocks(n);
    if (sb > 256) sb = 256;
    int* flag = small_flag(h->h_small);
    hipLaunchKernelGGL(k_bounds3_parts, dim3(sb), dim3(kBlock), 0, h->stream, dx, dy, dz, n, h->d_parts3, (unsigned int*)nullptr, 0, 0, 0);
    bool seen = false;
    HIP_TRY(publish_and_wait(h->stream, &h->publish_seq, flag, [&](int seq) {
      hipLaunchKernelGGL(k_bounds3_publish, dim3(1), dim3(64), 0, h->stream, (const float*)h->d_parts3, sb, hb, flag, seq);
    }, &seen));
    if (!seen) {                                           // safety net: the atomic form with a copy each way
      for (int a = 0; a < 3; ++a) { hb[2 * a] = 0xFFFFFFFFu; hb[2 * a + 1] = 0u; }
      HIP_TRY(hipMemcpyAsync(h->d_bounds, hb, 24, hipMemcpyHostToDevice, h->stream));
      hipLaunchKernelGGL(k_bounds3, dim3(sb > kBoundsBlocks ? kBoundsBlocks : sb), dim3(kBlock), 0, h->stream, dx, dy, dz, n, h->d_bounds);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hb, h->d_bounds, 24, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
  }
  if (hb[0] == 0xFFFFFFFFu || hb[1] == 0u) { set_error("target has no finite point"); return NDT_ERR_INVALID_ARG; }
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = ordered_to_float(hb[2 * a]); hi[a] = ordered_to_float(hb[2 * a + 1]); }
  { const int32_t gs = setup_geometry3(h, lo, hi); if (gs != NDT_OK) return gs; }
  const int32_t as = accumulate3(h, dx, dy, dz, n, /*merge=*/false, nullptr);
  if (as != NDT_OK) return as;
  h->has_target = true;
  return upload_static3(h);
}

// The template arguments of a 3D alignment kernel: f(MODE, NB) with the handle's Hessian and neighbourhood (with_mode's
// second argument, the 2D grid count, is always 1 in 3D and unused).
template <class F>
auto with_mode3(const ndt3d_handle* h, F&& f) {
  return with_mode(h->prm, [&](auto M, auto) {
    return h->neighbourhood == 7 ? f(M, std::integral_constant<int, 7>{}) : f(M, std::integral_constant<int, 1>{});
  });
}
// Both enter the key a cached graph is found by (ChainGraphCache compares keys, not kernels): a handle switched between
// the neighbourhoods must never replay the other one's graph.
int graph_mode3(const ndt3d_handle* h) { return (h->neighbourhood == 7 ? 0x10 : 0) | h->prm.hessian_mode; }

// the k_iterate3 of the handle's Hessian and neighbourhood, for graphs and plain launches (scan_chain)
const void* iter3_kernel(const ndt3d_handle* h) {
  return with_mode3(h, [](auto M, auto NB) { return (const void*)&ndt::k_iterate3<M, NB>; });
}

// Neighbourhood 7 is a scoring option of the alignment chains alone.  The kernels behind every other entry point that
// scores points against the grid (the lattice search, the pose lists, the particle scores, the per-point fit) keep the
// single-voxel score their contracts name, so with 7 set they refuse instead of answering another question.
int32_t single_voxel_only(const ndt2d_handle*, const char* = nullptr) { return NDT_OK; }
int32_t single_voxel_only(const ndt3d_handle* h, const char* who = nullptr) {
  if (h->neighbourhood == 1) return NDT_OK;
  ndt::last_error() = std::string(who ? who : "this entry point") +
                      ": scores a point against its own voxel only; the handle's neighbourhood is 7: call "
                      "ndt3d_set_neighbourhood(h, 1) first (neighbourhood 7 is honoured by evaluate, align, align_trace "
                      "and the multi-start / multi-scan chains)";
  return NDT_ERR_INVALID_ARG;
}

// the k_iterate3 chain of a scan: one launch shape for every size, the handle's one lane
ChainLaunch scan_chain(const ndt3d_handle* h, size_t, int) {
  return {iter3_kernel(h), dim3(ndt::kMaxBlocks), dim3(ndt::kBlock), h->d_static, h->d_call, h->d_dyn};
}

// the first launch of the old protocol: launches 0 .. K follow
void launch_begin(ndt3d_handle* h, int, hipStream_t stream, const float* const* d_s, size_t n, const double* pose, int fixed,
                  ndt::IterState3* host_state, int* host_flag) {
  hipLaunchKernelGGL(ndt::k_begin3, dim3(1), dim3(64), 0, stream, h->d_call, h->d_dyn, d_s[0], d_s[1], d_s[2], (int)n, pose[0],
                     pose[1], pose[2], pose[3], pose[4], pose[5], fixed, host_state, host_flag, h->flight.call_seq);
}

// Enqueue the Gauss-Newton loop of ndt3d_evaluate* (fixed_override = 1) and ndt3d_align* (-1): the head of the chain
// (the 2D head's arguments; a 3D call has no lane to choose and always drains); everything behind launch 0 is
// run_chain_tail's.
int32_t begin_align(ndt3d_handle* h, const float* const* d_s, size_t n, const double* pose, int fixed_override, bool, bool) {
  using namespace ndt;
  TraceRange range("ndt3d_align: Gauss-Newton loop");
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  { const int32_t fs = finish_host_fed(h); if (fs != NDT_OK) return fs; }     // an unfinished asynchronous call
  if (n == 0 || n > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  if (h->n_valid < 1) {
    h->flight.how = ChainFlight::kOnHost;
    *h->h_state = no_cell_state<IterState3>(pose);
    return NDT_OK;
  }
  const ChainPlan p = chain_plan(fixed_override, h->prm.fixed_iterations, h->prm.max_iterations, h->use_graph, h->check_every,
                                 h->fused_begin);
  next_seq(&h->flight.call_seq, h->h_flag);
  // Launch 0.  Fused (the default): k_iterate3_first evaluates at the initial pose and writes the per-call context from
  // its arguments; launches 1 .. K follow.  Old protocol: k_begin3, then launches 0 .. K.
  IterState3* const host_state = p.chunked ? h->h_state : (IterState3*)nullptr;
  int* const host_flag = p.chunked ? h->h_flag : (int*)nullptr;
  if (p.first) {
    with_mode3(h, [&](auto M, auto NB) {
      hipLaunchKernelGGL((k_iterate3_first<M, NB>), dim3(kMaxBlocks), dim3(kBlock), 0, h->stream, (const AlignStatic3*)h->d_static,
                         h->d_call, h->d_dyn, d_s[0], d_s[1], d_s[2], (int)n, pose[0], pose[1], pose[2], pose[3], pose[4], pose[5],
                         p.fixed, host_state, host_flag, h->flight.call_seq);
      return 0;
    });
  } else {
    launch_begin(h, 0, h->stream, d_s, n, pose, p.fixed, host_state, host_flag);
  }
  return run_chain_tail(h, scan_chain(h, n, 0), graph_mode3(h), 0, h->stream, nullptr, p, /*drain=*/true);
}

void unpack_h21(const double* s, double* H) {
  H[0] = s[0]; H[1] = s[1]; H[2] = s[2]; H[7] = s[3]; H[8] = s[4]; H[14] = s[5];
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) H[6 * r + 3 + k] = s[6 + 3 * r + k];
  H[21] = s[15]; H[22] = s[16]; H[23] = s[17]; H[28] = s[18]; H[29] = s[19]; H[35] = s[20];
  for (int r = 0; r < 6; ++r) for (int c = 0; c < r; ++c) H[6 * r + c] = H[6 * c + r];
}

// IterState3 -> ndt3d_result, or -> ndt3d_eval (the fields it shares with the result)
template <class Out>
void state3_to(const ndt::IterState3& s, Out* out) {
  std::memset(out, 0, sizeof(*out));
  unpack_h21(s.H, out->H);
  for (int j = 0; j < 6; ++j) out->g[j] = s.g[j];
  out->score = s.score;
  out->n_hit = s.n_hit;
  if constexpr (std::is_same<Out, ndt3d_result>::value) {
    for (int j = 0; j < 6; ++j) out->pose[j] = s.pose[j];
    out->iterations = s.iter;
    out->status = s.status;
  }
}

// The 3D side of the host code both handles share (ndt_search.hpp, ndt_map_host.hpp)
template <> struct HandleTraits<ndt3d_handle> {
  using State = ndt::IterState3;
  using Result = ndt3d_result;
  using Window = ndt3d_search_window;
  using Hit = ndt3d_search_hit;
  using Poses = ndt::StartPoses3;
  using Maps = ndt::StartMaps3;
  static constexpr int kDim = 3, kPose = 6, kMaxStarts = ndt::kMaxStarts3;
  static constexpr int kRecord = 3;                        // float4 per covariance record and per component
  // The copy of a fixed chain's state is enqueued directly behind the chain, so that fetch_state is a stream synchronise
  // ("the whole chain and the fetch of its final state are enqueued", include/ndt_hip.h); 2D copies at fetch_state.
  static constexpr bool kQueuedFetch = true;
  static constexpr const char* kCell = "voxel";
  static constexpr const char* kTraceComponents = "ndt3d: component list";
  static constexpr const char* kTraceAlignTrace = "ndt3d_align_trace";
  static constexpr const char* kTraceMapPair = "ndt3d_align_map: Gauss-Newton loop";
  static constexpr const char* kTraceMapMulti = "ndt3d_align_map_multi";
  static constexpr const char* kMapMultiNoEnd = "the 3D map-to-map multi-start loop did not report its end";
  static size_t cells(const ndt3d_handle* h) { return (size_t)h->grid.W * h->grid.H * h->grid.D; }
  // the handle as a map-to-map TARGET: its map neighbourhood, and what of it (with the Hessian) enters a graph's key
  static int map_neighbourhood(const ndt3d_handle* h) { return h->map_neighbourhood; }
  static int map_graph_mode(const ndt3d_handle* h) { return (h->map_neighbourhood == 7 ? 0x10 : 0) | h->prm.hessian_mode; }
  static constexpr const char* kMapNeighbourhoodSetter = "ndt3d_set_map_neighbourhood";
  template <class... A> static int32_t begin(A... a) { return begin_align(a...); }
  template <class... A> static ChainLaunch scan_chain(A... a) { return ::scan_chain(a...); }
  template <class... A> static void launch_begin(A... a) { ::launch_begin(a...); }
  template <class Out> static void to(const ndt::IterState3& s, Out* out) { state3_to(s, out); }
  static void launch_cov_records(ndt3d_handle* h, unsigned nb) {
    hipLaunchKernelGGL(ndt::k_cov_records3, dim3(nb), dim3(ndt::kBlock), 0, h->stream, h->grid, h->prm.min_points,
                       h->prm.eig_ratio, h->d_cov, h->d_blk);
  }
  static void launch_components(ndt3d_handle* h, unsigned nb, unsigned ncell, const unsigned int* offsets, unsigned n) {
    hipLaunchKernelGGL(ndt::k_components3, dim3(nb), dim3(ndt::kBlock), 0, h->stream, (const float4*)h->d_cov, ncell, offsets,
                       h->d_comp, n);
  }
  // one component of the list as ndt3d_get_components hands it out
  static void unpack_component(const float4* c, size_t i, float* mean_xyz, float* cov6, int32_t* key) {
    const float4 a = c[0], b = c[1], d = c[2];
    if (mean_xyz) { mean_xyz[3 * i] = a.x; mean_xyz[3 * i + 1] = a.y; mean_xyz[3 * i + 2] = a.z; }
    if (cov6) { cov6[6 * i] = b.x; cov6[6 * i + 1] = b.y; cov6[6 * i + 2] = b.z; cov6[6 * i + 3] = b.w; cov6[6 * i + 4] = d.x; cov6[6 * i + 5] = d.y; }
    if (key) std::memcpy(&key[i], &a.w, sizeof(int32_t));
  }
  // the searched axes of a 3D window: x, y and yaw
  static SearchWindow window(const ndt3d_search_window& w) {
    SearchWindow v;
    const int src[3] = {0, 1, 5};
    for (int a = 0; a < 3; ++a) { v.center[a] = w.center[src[a]]; v.half_extent[a] = w.half_extent[a]; v.step[a] = w.step[a]; }
    v.min_sep_trans = w.min_sep_trans; v.min_sep_rot = w.min_sep_rot;
    return v;
  }
  // the peaks as the ABI's hits: the searched (x, y, yaw) from the peak, the pinned coordinates from the window's centre
  static void hits_out(const SearchPeak* peaks, int32_t n, const ndt3d_search_window& w3, ndt3d_search_hit* hits) {
    for (int32_t q = 0; q < n; ++q) {
      ndt3d_search_hit& hh = hits[q];
      std::memset(&hh, 0, sizeof(hh));
      hh.pose[0] = peaks[q].pose[0]; hh.pose[1] = peaks[q].pose[1]; hh.pose[5] = peaks[q].pose[2];
      for (int a = 2; a <= 4; ++a) hh.pose[a] = w3.center[a];
      hh.score = peaks[q].score;
      hh.index = peaks[q].index;
    }
  }
};

// m alignments against the cached voxel grid in one launch chain (ndt3d_multi.hpp)
int32_t multi_align3(ndt3d_handle* h, const float* const* sxs, const float* const* sys, const float* const* szs, const size_t* ns,
                     bool shared, const double* init_poses, int32_t m, ndt3d_result* results) {
  using namespace ndt;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  TraceRange range(shared ? "ndt3d_align_multi_start" : "ndt3d_align_multi_scan");
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (h->n_valid < 1) {
    for (int32_t k = 0; k < m; ++k) state3_to(no_cell_state<IterState3>(&init_poses[6 * k]), &results[k]);
    return NDT_OK;
  }
  HIP_TRY(ensure_multi_chain(&h->h_state_multi, kMaxStarts3, &h->d_dyn_multi, h->stream));
  const int fixed = h->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : h->prm.max_iterations;
  const bool converged_mode = fixed == 0;
  next_seq(&h->flight.call_seq, h->h_flag);
  StartPoses3 sp{};
  StartScans3 sc{};
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 6; ++j) sp.p[k][j] = init_poses[6 * k + j];
    const int q = shared ? 0 : k;
    sc.sx[k] = sxs[q]; sc.sy[k] = sys[q]; sc.sz[k] = szs[q]; sc.n[k] = (int)ns[q];
  }
  hipLaunchKernelGGL(k_begin_multi3_scans, dim3(1), dim3(64), 0, h->stream, h->d_dyn_multi, sc, (int)m);
  hipLaunchKernelGGL(k_begin_multi3, dim3(1), dim3(64), 0, h->stream, h->d_call, h->d_dyn_multi, sp, (int)m, fixed,
                     converged_mode ? h->h_state_multi : (IterState3*)nullptr, converged_mode ? h->h_flag : (int*)nullptr,
                     h->flight.call_seq);
  HIP_TRY(hipGetLastError());
  const int steps = converged_mode ? h->check_every : K + 1;
  hipGraphExec_t exec = nullptr;
  const void *fs = nullptr, *fb = nullptr;
  with_mode3(h, [&](auto M, auto NB) { fs = (const void*)&k_multi_solve3<M>; fb = (const void*)&k_multi_body3<M, NB>; return 0; });
  // launch shapes in powers of two (slots >= m are born finished: their workgroups return at once), so that a caller
  // whose m varies from call to call replays one of seven cached graphs instead of instantiating a new one each time
  int mg = 1;
  while (mg < m) mg <<= 1;
  HIP_TRY(h->graphs.get2(fs, dim3(mg), dim3(kBlock), fb, dim3(kMaxBlocks, mg), dim3(kBlock), (void*)h->d_static, (void*)h->d_call,
                         (void*)h->d_dyn_multi, steps, 0x100000 | (mg << 8) | graph_mode3(h), h->stream, &exec));
  bool seen = true;
  HIP_TRY(run_multi_chain(exec, h->stream, converged_mode ? h->h_flag : nullptr, steps, K + 1, h->flight.call_seq, h->h_state_multi,
                          h->d_dyn_multi->state[K & 1], kMaxStarts3 * sizeof(IterState3), &seen));
  if (!seen) { set_error("the 3D multi-scan loop did not report its end"); return NDT_ERR_HIP; }
  for (int k = 0; k < m; ++k) state3_to(h->h_state_multi[k], &results[k]);
  return NDT_OK;
}

}  // namespace

extern "C" {

void ndt3d_default_params(ndt3d_params* p) {
  if (!p) return;
  ndt2d_default_params(p);
  p->cell_size = 1.0;
  p->min_points = 5;
  p->step_max_trans = 1.0;
  p->min_hits = 6;
}

int32_t ndt3d_create(const ndt3d_params* p, int32_t device_id, ndt3d_handle** out) {
  if (!out) return NDT_ERR_INVALID_ARG;
  *out = nullptr;
  const int32_t st = check_params(p);
  if (st != NDT_OK) return st;
  if (p->overlap_grids == 4) { set_error("overlapping grids are a 2D option"); return NDT_ERR_INVALID_ARG; }
  const int ndev = ndt_device_count();
  if (ndev <= 0) { set_error("no HIP device visible: this library has no CPU fallback"); return NDT_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return NDT_ERR_INVALID_ARG;
  ndt3d_handle* h = new (std::nothrow) ndt3d_handle();
  if (!h) return NDT_ERR_ALLOC;
  h->device = device_id;
  h->prm = *p;
  auto fail = [&](int32_t code) { ndt3d_destroy(h); return code; };
  if (hipSetDevice(device_id) != hipSuccess) return fail(NDT_ERR_HIP);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(NDT_ERR_HIP);
  if (hipMalloc((void**)&h->d_bounds, 32) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_counters, ndt::kCountAlloc * sizeof(int)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_outside, sizeof(unsigned long long)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_static, sizeof(ndt::AlignStatic3)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_call, sizeof(ndt::AlignCall3)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_dyn, sizeof(ndt::AlignDyn3)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (ndt::pinned_alloc(&h->h_static, sizeof(ndt::AlignStatic3)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipEventCreateWithFlags(&h->upload_ev, hipEventDisableTiming) != hipSuccess) return fail(NDT_ERR_HIP);
  if (ndt::pinned_alloc(&h->h_state, sizeof(ndt::IterState3)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (ndt::pinned_alloc(&h->h_flag, 64) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (ndt::pinned_alloc(&h->h_small, ndt::kSmallBytes) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMemset(h->d_dyn, 0, sizeof(ndt::AlignDyn3)) != hipSuccess) return fail(NDT_ERR_HIP);
  *out = h;
  return NDT_OK;
}

int32_t ndt3d_destroy(ndt3d_handle* h) {
  if (!h) return NDT_OK;
  (void)hipSetDevice(h->device);
  (void)finish(h);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->graphs.clear();
  void* dev[] = {h->d_parts3, h->d_bounds, h->d_counters, h->d_outside, h->d_static, h->d_call, h->d_dyn, h->d_t[0], h->d_t[1], h->d_t[2],
                 h->d_s[0], h->d_s[1], h->d_s[2], h->d_b[0], h->d_b[1], h->d_b[2], h->d_tiles, h->d_split3, h->grid.rec, h->grid.acc, h->d_dyn_multi,
                 h->d_cov, h->d_blk, h->d_comp, h->d_map_call};
  for (void* p : dev) if (p) (void)hipFree(p);
  void* host[] = {h->h_static, h->h_state, h->h_small, h->h_flag, h->h_state_multi, h->h_pub3};
  for (void* p : host) if (p) (void)hipHostFree(p);
  h->srch.release();
  h->fit.release();
  h->vox.release();
  if (h->upload_ev) (void)hipEventDestroy(h->upload_ev);
  if (h->map_ev) (void)hipEventDestroy(h->map_ev);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return NDT_OK;
}

int32_t ndt3d_set_tuning(ndt3d_handle* h, int32_t knob, int64_t value) {
  if (!h) return NDT_ERR_INVALID_ARG;
  switch (knob) {
    case NDT_TUNE_SINGLE_SYNC_BUILD: h->one_round_trip = value != 0; return NDT_OK;
    case NDT_TUNE_MAP_MULTI_FROM: if (value < 1 || value > ndt::kMaxStarts3 + 1) return NDT_ERR_INVALID_ARG; h->map_multi_from = (int)value; return NDT_OK;
    // takes effect with the next alignment; an alignment in flight keeps the protocol it began with
    case NDT_TUNE_FUSED_BEGIN: if (value != 0 && value != 1) return NDT_ERR_INVALID_ARG; h->fused_begin = value != 0; return NDT_OK;
    case NDT_TUNE_PARTICLE_TEAM: if (value != 0 && value != 64 && value != 256) return NDT_ERR_INVALID_ARG; h->particle_team = (int)value; return NDT_OK;
    default: return NDT_ERR_INVALID_ARG;
  }
}

int32_t ndt3d_set_neighbourhood(ndt3d_handle* h, int32_t n) {
  if (!h) { ndt::set_error("ndt3d_set_neighbourhood: the handle is null"); return NDT_ERR_INVALID_ARG; }
  if (n != 1 && n != 7) {
    ndt::set_error("ndt3d_set_neighbourhood: the neighbourhood is 1 (own voxel) or 7 (own voxel and its six face neighbours)");
    return NDT_ERR_INVALID_ARG;
  }
  // an alignment in flight keeps the kernels it was enqueued with and is finished first, as the searches do
  if (h->flight.waits()) {
    HIP_TRY(hipSetDevice(h->device));
    const int32_t fs = finish(h);
    if (fs != NDT_OK) return fs;
  }
  h->neighbourhood = n;
  return NDT_OK;
}

int32_t ndt3d_neighbourhood(const ndt3d_handle* h) { return h ? h->neighbourhood : NDT_ERR_INVALID_ARG; }

// The map-to-map twin, a setting of its own: it selects kernels and graph keys of the calls this handle is the TARGET
// of, and rebuilds nothing (grid, sums, covariance records and component list do not depend on it).
int32_t ndt3d_set_map_neighbourhood(ndt3d_handle* h, int32_t n) {
  if (!h) { ndt::set_error("ndt3d_set_map_neighbourhood: the handle is null"); return NDT_ERR_INVALID_ARG; }
  if (n != 1 && n != 7) {
    ndt::set_error("ndt3d_set_map_neighbourhood: the map neighbourhood is 1 (own voxel) or 7 (own voxel and its six face neighbours)");
    return NDT_ERR_INVALID_ARG;
  }
  if (h->flight.waits()) {
    HIP_TRY(hipSetDevice(h->device));
    const int32_t fs = finish(h);
    if (fs != NDT_OK) return fs;
  }
  h->map_neighbourhood = n;
  return NDT_OK;
}

int32_t ndt3d_map_neighbourhood(const ndt3d_handle* h) {
  if (!h) { ndt::set_error("ndt3d_map_neighbourhood: the handle is null"); return NDT_ERR_INVALID_ARG; }
  return h->map_neighbourhood;
}

int32_t ndt3d_wait_stream(ndt3d_handle* h, void* producer_stream) {
  if (!h) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ndt::order_after(h->stream, (hipStream_t)producer_stream));
  return NDT_OK;
}

int32_t ndt3d_add_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, size_t* n_outside) {
  if (!h || !x || !y || !z || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[3] = {x, y, z};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt3d_add_target_points_dev(h, h->d_t[0], h->d_t[1], h->d_t[2], n, nullptr, n_outside, nullptr);
}

// the cos / sin table of a range image's rings (both conversions); false: an elevation is not finite
static bool ring_table(const double* elevations, int n_elev, ndt::RingTable* rings) {
  *rings = ndt::RingTable{};
  for (int e = 0; e < n_elev; ++e) {
    if (!std::isfinite(elevations[e])) return false;
    rings->cs[2 * e] = std::cos(elevations[e]); rings->cs[2 * e + 1] = std::sin(elevations[e]);
  }
  return true;
}

int32_t ndt3d_range_image_to_points_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim, const double* elevations,
                                        double azimuth0, double azimuth_inc, double range_min, double range_max, float* d_x,
                                        float* d_y, float* d_z, void* stream) {
  if (!d_ranges || !elevations || !d_x || !d_y || !d_z || n_elev < 1 || n_elev > ndt::kMaxRings || n_azim < 1 ||
      !std::isfinite(azimuth0) || !std::isfinite(azimuth_inc))
    return NDT_ERR_INVALID_ARG;
  ndt::RingTable rings;
  if (!ring_table(elevations, n_elev, &rings)) return NDT_ERR_INVALID_ARG;
  const size_t n = (size_t)n_elev * (size_t)n_azim;
  hipLaunchKernelGGL(ndt::k_range_image_to_points, dim3(stream_blocks(n)), dim3(ndt::kBlock), 0, (hipStream_t)stream, d_ranges,
                     n_elev, n_azim, rings, azimuth0, azimuth_inc, (float)range_min, (float)range_max, d_x, d_y, d_z);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

int32_t ndt3d_reserve_target(ndt3d_handle* h, const double lo[3], const double hi[3]) {
  if (!h || !lo || !hi) return NDT_ERR_INVALID_ARG;
  float l[3], u[3];
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) return NDT_ERR_INVALID_ARG;
    l[a] = (float)lo[a]; u[a] = (float)hi[a];
  }
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  h->has_target = false;
  grid_changed3(h);
  { const int32_t gs = setup_geometry3(h, l, u); if (gs != NDT_OK) return gs; }
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.D;
  HIP_TRY(hipMemsetAsync(h->grid.acc, 0, ncell * sizeof(ndt::CellAcc3), h->stream));
  HIP_TRY(hipMemsetAsync(h->grid.rec, 0, 4 * ncell * sizeof(float4), h->stream));
  h->n_valid = 0;
  h->has_target = true;
  return upload_static3(h);
}

// ndt3d_add_target_points_dev (sign = 1) and ndt3d_remove_target_points_dev (sign = -1): one submap update, with a sign
static int32_t update_target_points3_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                         const double pose[6], size_t* n_outside, void* stream, int sign) {
  if (!h || !d_x || !d_y || !d_z || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  // (a wrapped count is told from a full voxel by its size: removed_cell_broken, ndt2d_kernels.hpp)
  if (sign < 0 && n >= 0xFFF00000ull) { set_error("more points to remove than a call can take (2^32 - 2^20)"); return NDT_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (stream) HIP_TRY(ndt::order_after(h->stream, (hipStream_t)stream));
  const float* p[3] = {d_x, d_y, d_z};
  ndt::Rigid3F T;
  if (pose) {       // the points are moved on the way into the build (count and scatter passes), not by a kernel of their own
    double R[9];
    ndt::rot3_products(std::sin(pose[3]), std::cos(pose[3]), std::sin(pose[4]), std::cos(pose[4]), std::sin(pose[5]),
                       std::cos(pose[5]), R);
    for (int j = 0; j < 9; ++j) T.r[j] = (float)R[j];
    for (int j = 0; j < 3; ++j) T.t[j] = (float)pose[j];
  }
  unsigned long long outside = 0;
  grid_changed3(h);
  const int32_t fs = accumulate3(h, p[0], p[1], p[2], n, /*merge=*/true, &outside, pose ? &T : nullptr, sign);
  if (n_outside) *n_outside = (size_t)outside;
  if (fs != NDT_OK) { h->has_target = false; return fs; }
  return NDT_OK;          // geometry, storage and parameters are unchanged: the device context stays as it is
}

int32_t ndt3d_add_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                    const double pose[6], size_t* n_outside, void* stream) {
  return update_target_points3_dev(h, d_x, d_y, d_z, n, pose, n_outside, stream, 1);
}

int32_t ndt3d_remove_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                       const double pose[6], size_t* n_outside, void* stream) {
  return update_target_points3_dev(h, d_x, d_y, d_z, n, pose, n_outside, stream, -1);
}

int32_t ndt3d_remove_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, size_t* n_outside) {
  if (!h || !x || !y || !z || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[3] = {x, y, z};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt3d_remove_target_points_dev(h, h->d_t[0], h->d_t[1], h->d_t[2], n, nullptr, n_outside, nullptr);
}

int32_t ndt3d_set_target_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n, void* stream) {
  if (!h || !d_x || !d_y || !d_z || n == 0) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // producer of the device arrays
  return set_target3_impl(h, d_x, d_y, d_z, n);
}

int32_t ndt3d_set_target(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n) {
  if (!h || !x || !y || !z || n == 0) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[3] = {x, y, z};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt3d_set_target_dev(h, h->d_t[0], h->d_t[1], h->d_t[2], n, nullptr);
}

int32_t ndt3d_get_grid_info(ndt3d_handle* h, ndt3d_grid_info* info) {
  if (!h || !info) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  info->ox = h->grid.ox; info->oy = h->grid.oy; info->oz = h->grid.oz; info->inv_cell = h->grid.inv_c;
  info->width = h->grid.W; info->height = h->grid.H; info->depth = h->grid.D; info->n_valid = h->n_valid;
  return NDT_OK;
}

int32_t ndt3d_get_grid(ndt3d_handle* h, int32_t* count, float* mean_xyz, float* icov6) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nc = (size_t)h->grid.W * h->grid.H * h->grid.D;
  float4* rec = new (std::nothrow) float4[4 * nc];
  ndt::CellAcc3* acc = count ? new (std::nothrow) ndt::CellAcc3[nc] : nullptr;
  int32_t rc = (!rec || (count && !acc)) ? NDT_ERR_ALLOC : NDT_OK;
  if (rc == NDT_OK && hipMemcpyAsync(rec, h->grid.rec, 4 * nc * sizeof(float4), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK && acc && hipMemcpyAsync(acc, h->grid.acc, nc * sizeof(ndt::CellAcc3), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK) {
    for (size_t k = 0; k < nc; ++k) {
      const float4 a = rec[4 * k], b = rec[4 * k + 1], c = rec[4 * k + 2];
      const bool valid = a.w > 0.f;
      if (count) count[k] = (int32_t)acc[k].n;
      if (mean_xyz) { mean_xyz[3 * k] = valid ? a.x : 0.f; mean_xyz[3 * k + 1] = valid ? a.y : 0.f; mean_xyz[3 * k + 2] = valid ? a.z : 0.f; }
      if (icov6) {
        icov6[6 * k] = b.x; icov6[6 * k + 1] = b.y; icov6[6 * k + 2] = b.z; icov6[6 * k + 3] = b.w;
        icov6[6 * k + 4] = c.x; icov6[6 * k + 5] = c.y;
      }
    }
  }
  delete[] rec; delete[] acc;
  return rc;
}

int32_t ndt3d_evaluate(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                       const double pose[6], ndt3d_eval* out) {
  const float* const s[3] = {sx, sy, sz};
  return evaluate_host(h, s, n, pose, out);
}

int32_t ndt3d_evaluate_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                           const double pose[6], ndt3d_eval* out) {
  const float* const s[3] = {d_sx, d_sy, d_sz};
  return evaluate_dev(h, s, n, pose, out);
}

int32_t ndt3d_align_dev_async(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                              const double init_pose[6]) {
  const float* const s[3] = {d_sx, d_sy, d_sz};
  return align_dev_async(h, s, n, init_pose);
}

int32_t ndt3d_align_finish(ndt3d_handle* h, ndt3d_result* out) { return align_finish(h, out); }

int32_t ndt3d_align_trace(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                          const double init_pose[6], ndt3d_result* rows, int32_t capacity, int32_t* n_rows, ndt3d_result* out) {
  const float* const s[3] = {sx, sy, sz};
  return align_trace(h, s, n, init_pose, rows, capacity, n_rows, out);
}

int32_t ndt3d_align_multi_scan_dev(ndt3d_handle* h, const float* const* d_sx, const float* const* d_sy, const float* const* d_sz,
                                   const size_t* n, const double* init_poses, int32_t m, ndt3d_result* results) {
  if (!h || !d_sx || !d_sy || !d_sz || !n || !init_poses || !results || m < 1 || m > ndt::kMaxStarts3) return NDT_ERR_INVALID_ARG;
  for (int32_t k = 0; k < m; ++k)
    if (!d_sx[k] || !d_sy[k] || !d_sz[k] || n[k] == 0 || n[k] > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  return multi_align3(h, d_sx, d_sy, d_sz, n, /*shared=*/false, init_poses, m, results);
}

int32_t ndt3d_align_multi_start_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                    const double* init_poses, int32_t m, ndt3d_result* results) {
  if (!h || !d_sx || !d_sy || !d_sz || !init_poses || !results || m < 1 || m > ndt::kMaxStarts3) return NDT_ERR_INVALID_ARG;
  if (n == 0 || n > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  return multi_align3(h, &d_sx, &d_sy, &d_sz, &n, /*shared=*/true, init_poses, m, results);
}

void* ndt3d_stream(ndt3d_handle* h) { return h ? (void*)h->stream : nullptr; }

int32_t ndt3d_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                        const double init_pose[6], ndt3d_result* out) {
  const float* const s[3] = {d_sx, d_sy, d_sz};
  return align_dev(h, s, n, init_pose, out);
}

int32_t ndt3d_align(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                    const double init_pose[6], ndt3d_result* out) {
  const float* const s[3] = {sx, sy, sz};
  return align_host(h, s, n, init_pose, out);
}

}  // extern "C"

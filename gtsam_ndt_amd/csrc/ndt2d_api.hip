// C-ABI host side of the 2D NDT matcher (include/ndt_hip.h).  Owns device memory and one
// HIP stream per handle; every compute entry point launches the gfx950 kernels of
// ndt2d_kernels.hpp.  There is deliberately no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "../../include/ndt_hip.h"
#include "ndt2d_kernels.hpp"
#include "ndt2d_small.hpp"
#include "ndt2d_build.hpp"
#include "ndt2d_build_sorted.hpp"
#include "ndt2d_multi_start.hpp"
#include "ndt2d_d2d.hpp"
#include "ndt2d_d2d_multi.hpp"
#include "ndt_host.hpp"
#include "ndt_chain_host.hpp"
#include "ndt_search.hpp"

#include <atomic>

using namespace ndt;

struct ndt2d_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  ndt2d_params prm{};
  // target grid
  GridDev grid{};
  size_t cell_capacity = 0;
  bool has_target = false;
  int n_valid = 0;
  size_t n_points = 0;
  unsigned int* d_bounds = nullptr;        // [4]
  int* d_counters = nullptr;               // [kCountAlloc] shards of valid / overflowed cells, the cells a removal broke, a merge's counts
  unsigned long long* d_outside = nullptr; // [1]
  void* h_small = nullptr;                 // pinned scratch (kSmallBytes: counter shards at 0, the outside count at 128, a flag)
  // staging for host-pointer entry points
  float* d_t[2] = {nullptr, nullptr}; size_t tcap = 0;
  float* d_s[2] = {nullptr, nullptr}; size_t scap = 0;
  // alignment context (see ndt2d_kernels.hpp: who writes what)
  AlignStatic* d_static = nullptr;
  AlignCall* d_call = nullptr;
  AlignDyn* d_dyn = nullptr;
  AlignStatic* h_static = nullptr;         // pinned
  hipEvent_t upload_ev = nullptr;          // recorded after the last upload from h_static
  hipEvent_t wait_ev = nullptr;            // ndt2d_wait_stream's event
  IterState* h_state = nullptr;            // pinned
  int* h_flag = nullptr;                   // pinned: [0] raised by the launch that ends a converged-mode loop, [1] progress
  ChainFlight flight;                      // what the last single-pair alignment left in flight (ndt_chain_host.hpp)
  // the further launch chains of asynchronous fixed-iteration calls (ndt_host.hpp: AsyncLane), lane k at index k - 1;
  // lane 0 is stream / d_call / d_dyn
  AsyncLane lane[kMaxLanes - 1];
  AlignCall* d_call_lane[kMaxLanes - 1] = {};
  AlignDyn* d_dyn_lane[kMaxLanes - 1] = {};
  static constexpr int kDefaultLanes = 3;  // what a new handle runs (NDT_TUNE_ASYNC_CHAINS): the count DESIGN 7 measured best
  LaneState lanes;
  bool fork_every_pair = false;            // NDT_TUNE_LANE_FORK = 1: the secondary lanes fork from the handle's stream at every round
  AlignCall* call_of(int l) const { return l ? d_call_lane[l - 1] : d_call; }
  AlignDyn* dyn_of(int l) const { return l ? d_dyn_lane[l - 1] : d_dyn; }
  // binned grid build scratch (ndt2d_build.hpp)
  float* d_bx = nullptr; float* d_by = nullptr; size_t bcap = 0;
  unsigned int* d_tiles = nullptr; size_t tile_cap = 0;   // total[nt] | start[nt+1] | cursor[nt]
  ndt::GeomDev* d_geom = nullptr;          // geometry decided on the device (one-round-trip ndt2d_set_target)
  ndt::GeomDev* h_geom = nullptr;          // pinned: its read-back
  int last_ntile = 0;                      // tiles of the cached grid: the next build's launch bound follows it
  bool static_on_device = false;           // d_static holds this handle's parameters (some upload_static has run)
  bool one_round_trip = true;              // NDT_TUNE_SINGLE_SYNC_BUILD
  bool use_binned_build = true;
  int build_variant = 1;                   // NDT_TUNE_BINNED_BUILD: 1 chunk-sorted build (ndt2d_build_sorted.hpp), 2 the round-1 binned build
  float2* d_bxy = nullptr; size_t bxy_cap = 0;             // chunk-sorted copy of the cloud ([chunks][chunk points])
  unsigned int* d_table = nullptr; size_t table_cap = 0;   // [tiles][chunks]: start | len << 16 of every run
  float4* d_parts = nullptr;               // [kBoundsParts]: per-workgroup partial bounding boxes
  unsigned char* d_split = nullptr; size_t split_cap = 0;  // tickets | cursor | touched | parts | pool of the shared tiles (SplitBufs)
  unsigned int build_seq = 0;              // sorted builds so far on this handle (SplitBufs::seq; never 0 in a launch)
  // accumulators of the sorted build, ping-pong: half p = 256 bytes: int counters[kCountInts] | u64 outside at 128 | the cells
  // a removal broke (word kCountUnder).  A build adds to half acc_parity and clears the other one for the next build
  // (k_tile_gather), so no fill launch precedes it.
  unsigned char* d_acc2 = nullptr;
  int acc_parity = 0;
  bool acc_clean = false;                  // both halves known to be zero where the next build needs it
  int publish_seq = 0;                     // k_build_publish's flag value of the build in flight (small_flag(h_small))
  // hipGraph of the launch chain (launch-bound inner loop: one replay instead of K+1 launches)
  ChainGraphCache graphs;
  AlignDynMulti* d_dyn_multi = nullptr;    // multi-start chains (ndt2d_multi_start.hpp), allocated on first use
  IterState* h_state_multi = nullptr;      // pinned [kMaxStarts]
  int split_from = 12;                     // multi-start / multi-scan calls of this many starts use the split chain (NDT_TUNE_SPLIT_FROM)
  // execution strategy knobs (ndt2d_set_tuning; results do not depend on them beyond float32 summation order)
  bool use_small = true;                   // short scans run the whole loop in one workgroup (k_align_small)
  bool use_wide = true;                    // 1024-thread workgroups for large scans ...
  size_t wide_threshold = 300000;          // ... from this many source points
  bool use_graph = true;
  int check_every = 8;                     // converged mode: launches per chunk
  bool fused_begin = true;                 // NDT_TUNE_FUSED_BEGIN: launch 0 of a single-scan chain is k_iterate_first (no k_begin)
  int particle_team = 0;                   // NDT_TUNE_PARTICLE_TEAM: lanes per pose of ndt2d_score_particles*, 0 = by the list's length
  SearchScratch srch;                      // exhaustive pose search scratch (ndt_search.hpp), allocated on first use
  PointFitScratch fit;                     // per-point fit and selection scratch (ndt_point_fit.hpp), allocated on first use
  VoxelFilterScratch vox;                  // voxel-grid scan filter scratch (ndt_voxel_filter.hpp), allocated on first use
  // map-to-map alignment (ndt_map_host.hpp, ndt2d_d2d_api.hpp), allocated on first use; both caches follow the grid (grid_changed)
  float4* d_cov = nullptr; size_t cov_cap = 0;            // covariance records of the cached grid ([2 x cells], the layout of grid.rec)
  unsigned int* d_blk = nullptr; size_t blk_cap = 0;      // valid cells per workgroup of k_cov_records | their exclusive scan | the total
  float4* d_comp = nullptr; size_t comp_cap = 0;          // component list: this handle as the source of a map-to-map call
  int n_comp = 0;
  bool cov_valid = false, comp_valid = false;
  MapCall* d_map_call = nullptr;                          // per-call context of k_iterate_d2d (this handle as the target)
  hipEvent_t map_ev = nullptr;                            // orders a target handle's stream behind this handle's (order_after)
  int map_multi_from = 2;                                 // ndt2d_align_map_multi calls of this many starts use one chain (NDT_TUNE_MAP_MULTI_FROM)
};

namespace {

template <> struct HandleTraits<ndt2d_handle>;   // (below; the shared chain code is used before it)

constexpr size_t kMaxCells = (size_t)1 << 27;
#ifndef NDT_ITER_THREADS
#define NDT_ITER_THREADS 256
#endif
constexpr int kIterThreads = NDT_ITER_THREADS;   // workgroup size of k_iterate (256 workgroups always)
// Scans of a few hundred thousand points and more are no longer latency-bound per launch but short
// of loads in flight (15+ dependent gather rounds per thread at 256 threads): 1024-thread
// workgroups (four waves per SIMD) hide that latency.  Measured at 1M source points: see DESIGN 5.1.
constexpr int kIterThreadsWide = 1024;

int32_t check_params(const ndt2d_params* p) {
  if (!p) return NDT_ERR_INVALID_ARG;
  if (!(p->cell_size > 0.0) || !std::isfinite(p->cell_size)) return NDT_ERR_INVALID_ARG;
  if (p->min_points < 2 || p->max_iterations < 1 || p->fixed_iterations < 0) return NDT_ERR_INVALID_ARG;
  if (!(p->eig_ratio > 0.0) || !(p->eig_ratio <= 1.0)) return NDT_ERR_INVALID_ARG;
  if (p->hessian_mode != NDT_HESSIAN_GAUSS_NEWTON && p->hessian_mode != NDT_HESSIAN_NEWTON)
    return NDT_ERR_INVALID_ARG;
  if (!(p->step_max_trans > 0.0) || !(p->step_max_rot > 0.0)) return NDT_ERR_INVALID_ARG;
  if (!(p->d1 > 0.0) || !(p->d2 > 0.0) || !std::isfinite(p->d1) || !std::isfinite(p->d2)) return NDT_ERR_INVALID_ARG;
  if (p->overlap_grids != 0 && p->overlap_grids != 1 && p->overlap_grids != 4) return NDT_ERR_INVALID_ARG;
  if (p->line_search < 0 || p->line_search > 16) return NDT_ERR_INVALID_ARG;
  if (!(p->step_scale >= 0.0 && p->step_scale <= 8.0)) return NDT_ERR_INVALID_ARG;   // 0 means 1
  return NDT_OK;
}

int blocks_for(size_t) { return kMaxBlocks; }   // one workgroup per CU, always (see k_iterate)

// k_bounds ends in four same-address atomics per block (about 10 ns each, serialised): few blocks
#ifndef NDT_BOUNDS_BLOCKS
#define NDT_BOUNDS_BLOCKS 128
#endif
constexpr int kBoundsBlocks = NDT_BOUNDS_BLOCKS;
int stream_blocks(size_t n) {   // streaming kernels: up to 8 blocks per CU
  size_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int)b;
}

int32_t upload_static(ndt2d_handle* h);

// The cached grid is about to change (a new target, merged points, a reserved extent, a loaded map): what map-to-map
// alignment derived from it (ndt_map_host.hpp) is stale.
void grid_changed(ndt2d_handle* h) { h->cov_valid = false; h->comp_valid = false; }

// The words a removal adds to a failed call: what the kernels counted in kCountUnder means that points were removed that
// are not in the map.
int32_t check_removal(const int* hc) {
  if (hc[ndt::kCountUnder] > 0) {
    set_error("removed points are not in the target: a cell's count fell below zero, or reached zero with sums left");
    return NDT_ERR_INVALID_ARG;
  }
  return NDT_OK;
}

// sign = -1: the finalise behind a removal (accumulate_and_finalise), which also looks for the cells it broke
int32_t finalise_grid(ndt2d_handle* h, int sign = 1) {
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.ngrid;
  HIP_TRY(hipMemsetAsync(h->d_counters, 0, ndt::kCountWords * sizeof(int), h->stream));
  const dim3 blocks((unsigned)((ncell + kBlock - 1) / kBlock));
  if (sign < 0) hipLaunchKernelGGL((k_finalise<-1>), blocks, dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points, h->prm.eig_ratio, h->d_counters);
  else hipLaunchKernelGGL((k_finalise<1>), blocks, dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points, h->prm.eig_ratio, h->d_counters);
  HIP_TRY(hipGetLastError());
  int* hc = (int*)h->h_small;
  HIP_TRY(hipMemcpyAsync(hc, h->d_counters, ndt::kCountInts * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  // (on its own: the caller's outside count may be on its way into the two words between)
  HIP_TRY(hipMemcpyAsync(hc + ndt::kCountUnder, h->d_counters + ndt::kCountUnder, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  int n_valid_sum = 0, n_over_sum = 0;
  sum_count_shards(hc, &n_valid_sum, &n_over_sum);
  h->n_valid = n_valid_sum;
  if (sign < 0) { const int32_t rs = check_removal(hc); if (rs != NDT_OK) return rs; }
  if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
  return NDT_OK;
}

// ---- chunk-sorted build (ndt2d_build_sorted.hpp): host side -------------------------------------------------------
struct SortPlan { int P = 0, chunk = 0, nchunks = 0; };

// Points per thread of k_chunk_sort (chunk = 256 P points): small clouds take small chunks so that more CUs share
// the work (a 100k-point scan: 98 chunks of 1024), large ones the longest runs.  false: the table would exceed its
// bounds (tiles x chunks <= 2^20, chunks <= 4096) - the caller takes the round-1 path.
bool plan_sorted(size_t n, long long ntile, SortPlan* sp) {
  int P = n <= 131072 ? 4 : (n <= 524288 ? 8 : 16);
  for (;; P *= 2) {
    const size_t C = (size_t)kSortThreads * P, nch = (n + C - 1) / C;
    if (nch <= (size_t)kSortMaxChunks && nch * (size_t)ntile <= kSortMaxTable) { sp->P = P; sp->chunk = (int)C; sp->nchunks = (int)nch; return true; }
    if (P == 16) return false;
  }
}

// the chunk-sorted build's buffers for n points over `tiles` tiles: the sorted copy of the cloud, the run table and the
// buffers the workgroups that share a tile use (ndt2d_build_sorted.hpp: SplitBufs)
int32_t ensure_sorted_buffers(ndt2d_handle* h, const SortPlan& sp, size_t n, int tiles, SplitBufs* sb) {
  const size_t need_pts = (size_t)sp.nchunks * sp.chunk, need_tab = (size_t)tiles * sp.nchunks;
  HIP_TRY(grow(&h->d_bxy, &h->bxy_cap, need_pts, need_pts + need_pts / 4 + 4096));
  HIP_TRY(grow(&h->d_table, &h->table_cap, need_tab, need_tab + need_tab / 4 + 1024));
  const size_t pool_entries = n < (size_t)tiles * kGatherSplit * kTileCells ? n : (size_t)tiles * kGatherSplit * kTileCells;
  const size_t off_touched = ((size_t)tiles + 1) * sizeof(unsigned int);
  const size_t off_part = (off_touched + (size_t)tiles * sizeof(unsigned int) + 15) / 16 * 16;
  const size_t off_pool = off_part + (size_t)tiles * kGatherSplit * sizeof(uint2);
  const size_t need = off_pool + (pool_entries + 1) * sizeof(CellAcc);
  bool grew = false;
  HIP_TRY(grow(&h->d_split, &h->split_cap, need, need + need / 4, &grew));
  if (grew) h->build_seq = 0xFFFFFFFFu;                            // (the touched numbers must not start as garbage)
  if (h->build_seq == 0xFFFFFFFFu) {                               // new memory, or the numbers would wrap: start them over
    HIP_TRY(hipMemsetAsync(h->d_split, 0, h->split_cap, h->stream));
    h->build_seq = 0u;
  }
  ++h->build_seq;
  sb->ticket = reinterpret_cast<unsigned int*>(h->d_split);
  sb->touched = reinterpret_cast<unsigned int*>(h->d_split + off_touched);
  sb->part = reinterpret_cast<uint2*>(h->d_split + off_part);
  sb->pool = reinterpret_cast<CellAcc*>(h->d_split + off_pool);
  sb->tiles = tiles;
  sb->seq = h->build_seq;
  // a tile is shared so that no workgroup sums much more than a CU's share of the cloud; clouds too small to fill the
  // chip are cut finer, down to 1024 points per workgroup
  const size_t share = n / 200;
  sb->split_points = (int)(share < 1024 ? 1024 : (share > (size_t)1 << 24 ? (size_t)1 << 24 : share));
  return NDT_OK;
}

// Workgroups per tile (grid.y of k_tile_gather).  A cloud that fills most of the grid's tiles keeps most CUs busy with one
// workgroup per tile (169 tiles of a 1M-point submap: sharing them measured slower - the surplus workgroups cost more
// than the 87 idle CUs could give back); a cloud that lands on a few tiles (a 100k-point scan touches about 16) is
// where sharing pays: its tiles get up to kGatherSplit workgroups each.
int gather_split(size_t n, int tiles) {
  size_t touched = n / 6000 + 1;
  if (touched > (size_t)tiles) touched = (size_t)tiles;
  size_t s = 256 / touched;
  return (int)(s < 1 ? 1 : (s > (size_t)kGatherSplit ? (size_t)kGatherSplit : s));
}

void launch_chunk_sort(ndt2d_handle* h, const SortPlan& sp, const float* d_x, const float* d_y, size_t n, const BinGeom& bg,
                       int hist_tiles, const MoveArgs& mv, unsigned long long* d_outside, const GeomArgs& ga, const SplitBufs& sb) {
  const size_t lds = (size_t)sp.chunk * sizeof(float2) + (size_t)hist_tiles * sizeof(unsigned int);
#define NDT_SORT(PP) hipLaunchKernelGGL((k_chunk_sort<PP>), dim3((unsigned)sp.nchunks), dim3(kSortThreads), lds, h->stream, d_x, d_y, n, \
                                        bg, sp.nchunks, mv, h->d_bxy, h->d_table, d_outside, ga, sb.ticket, sb.tiles + 1, sb.touched, sb.seq)
  if (sp.P == 4) NDT_SORT(4); else if (sp.P == 8) NDT_SORT(8); else NDT_SORT(16);
#undef NDT_SORT
}

// the bounding box of a cloud as per-workgroup partials in h->d_parts; returns the number of partials
int launch_bounds_parts(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, GeomDev* zero = nullptr) {
  int nb = stream_blocks(n);
  if (nb > kBoundsParts) nb = kBoundsParts;
  const bool vec = (((uintptr_t)d_x | (uintptr_t)d_y) & 15u) == 0;
  if (vec) hipLaunchKernelGGL((k_bounds_parts<true>), dim3(nb), dim3(kBlock), 0, h->stream, d_x, d_y, n, h->d_parts, zero);
  else hipLaunchKernelGGL((k_bounds_parts<false>), dim3(nb), dim3(kBlock), 0, h->stream, d_x, d_y, n, h->d_parts, zero);
  return nb;
}

// The read-back of a sorted build: k_build_publish writes `nwords` words from device memory into pinned host memory and
// raises the flag in h_small (publish_and_wait).  If the flag does not come, a plain copy after a stream synchronisation
// is the safety net.
int32_t read_back(ndt2d_handle* h, const void* d_src, void* h_dst, int nwords) {
  int* flag = small_flag(h->h_small);
  bool seen = false;
  HIP_TRY(publish_and_wait(h->stream, &h->publish_seq, flag, [&](int seq) {
    hipLaunchKernelGGL(k_build_publish, dim3(1), dim3(64), 0, h->stream, (const unsigned int*)d_src, (unsigned int*)h_dst, nwords, flag, seq);
  }, &seen));
  if (!seen) {
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)nwords * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return NDT_OK;
}

// The two binned builds below enqueue the same launches for a geometry the host knows (the grids of h->grid) and for one
// the device decides in the same stream (set_target_single_sync); `tiles` is the grid's tile count or the launch bound.
// They add the counter shards and the outside count into d_cnt and d_out.

// Chunk-sorted build (ndt2d_build_sorted.hpp): sort every chunk of the cloud by tile, then one workgroup per tile gathers
// its runs.  Host geometry: ga = {} (merge = add to the cached sums, or with sign = -1 take the cloud out of them; the
// last grid's gather clears `clear_next`, the accumulator half of the next build).  Device geometry: ga, whose chunk sort prologue decides it into ga.out.
int32_t enqueue_sorted_build(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, const SortPlan& sp, const SplitBufs& sb,
                             int tiles, bool merge, const MoveArgs& mv, const GeomArgs& ga, int* d_cnt, unsigned long long* d_out,
                             unsigned int* clear_next, int sign = 1) {
  const GridDev& g = h->grid;
  const GeomDev* dg = ga.out;
  const int ngrid = dg ? 1 : g.ngrid;
  const int ntx = dg ? 0 : (g.W + kTile - 1) >> kTileShift;
  const int split = gather_split(n, tiles);
  for (int q = 0; q < ngrid; ++q) {
    const BinGeom bg = dg ? BinGeom{} : BinGeom{g.gx[q], g.gy[q], g.inv_c, g.W, g.H, ntx, tiles};
    launch_chunk_sort(h, sp, d_x, d_y, n, bg, tiles, mv, q == 0 ? d_out : (unsigned long long*)nullptr, ga, sb);
    const auto gather = sign < 0 ? &k_tile_gather<-1> : &k_tile_gather<1>;
    hipLaunchKernelGGL(gather, dim3(tiles, split), dim3(kGatherThreads), 0, h->stream, (const float2*)h->d_bxy,
                       (const unsigned int*)h->d_table, sp.nchunks, sp.chunk, g, q, ntx, merge ? 1 : 0, h->prm.min_points,
                       h->prm.eig_ratio, d_cnt, dg, (const GridDev*)ga.grid, sb, q == ngrid - 1 ? clear_next : (unsigned int*)nullptr);
    HIP_TRY(hipGetLastError());
  }
  return NDT_OK;
}

// the round-1 binned build's scratch for n points over `tiles` tiles: the binned cloud and the tile tables
int32_t ensure_binned_buffers(ndt2d_handle* h, size_t n, int tiles) {
  HIP_TRY(grow({grow_buf(&h->d_bx), grow_buf(&h->d_by)}, &h->bcap, n, n + n / 4 + 1024));
  const size_t tneed = 3 * (size_t)tiles + 4;
  HIP_TRY(grow(&h->d_tiles, &h->tile_cap, tneed, tneed));
  return NDT_OK;
}

// Round-1 binned build (ndt2d_build.hpp): per grid count -> scan -> scatter -> accumulate.  Host geometry: dg = null (merge =
// add to the cached sums).  Device geometry: dg and dgrid, decided by k_geometry behind the caller's k_build_init, which
// cleared the tile totals.
int32_t enqueue_binned_build(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, int tiles, bool merge, const GeomDev* dg,
                             const GridDev* dgrid, int* d_cnt, unsigned long long* d_out, int sign = 1) {
  const GridDev& g = h->grid;
  const int ngrid = dg ? 1 : g.ngrid;
  const int ntx = dg ? 0 : (g.W + kTile - 1) >> kTileShift;
  // tile tables laid out for `tiles`: total[tiles] | start[tiles + 1] | cursor[tiles]
  unsigned int* d_total = h->d_tiles;
  unsigned int* d_start = h->d_tiles + tiles;
  unsigned int* d_cursor = h->d_tiles + 2 * tiles + 1;
  const size_t chunk = (size_t)kBinThreads * kBinPerThread;
  size_t nb = (n + chunk - 1) / chunk;
  if (nb > 1024) nb = 1024;
  for (int q = 0; q < ngrid; ++q) {
    const BinGeom bg = dg ? BinGeom{} : BinGeom{g.gx[q], g.gy[q], g.inv_c, g.W, g.H, ntx, tiles};
    if (!dg) HIP_TRY(hipMemsetAsync(d_total, 0, tiles * sizeof(unsigned int), h->stream));
    hipLaunchKernelGGL(k_tile_count, dim3((unsigned)nb), dim3(kBinThreads), tiles * sizeof(unsigned int), h->stream,
                       d_x, d_y, n, bg, d_total, q == 0 ? d_out : (unsigned long long*)nullptr, dg);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(1024), 0, h->stream, d_total, d_start, d_cursor, dg ? 0 : tiles, dg);
    hipLaunchKernelGGL(k_tile_scatter, dim3((unsigned)nb), dim3(kBinThreads), 2 * tiles * sizeof(unsigned int),
                       h->stream, d_x, d_y, n, bg, d_cursor, h->d_bx, h->d_by, dg);
    const auto tile_kernel = sign < 0 ? &k_tile_accumulate<-1> : &k_tile_accumulate<1>;
    hipLaunchKernelGGL(tile_kernel, dim3(tiles), dim3(kBinThreads), 0, h->stream, h->d_bx, h->d_by, d_start, g, q,
                       ntx, merge ? 1 : 0, h->prm.min_points, h->prm.eig_ratio, d_cnt, dg, dgrid);
    HIP_TRY(hipGetLastError());
  }
  return NDT_OK;
}

// a2 + a3 for n points: binned LDS build when the tile histogram fits in LDS (always, below
// ~2.9 km x 2.9 km at 0.5 m cells), else scattered global atomics + k_finalise.  merge = add to
// the cached sums (incremental submap update) instead of starting from zero; sign = -1 (with merge): take the points
// out of the cached sums again - the same kernels on every path, with the sign (NDT_ERR_INVALID_ARG when the points are
// not in the map: check_removal).
int32_t accumulate_and_finalise(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, bool merge,
                                unsigned long long* h_outside, const MoveArgs* move = nullptr, int sign = 1) {
  TraceRange range(merge ? "ndt2d: submap update (moments + finalise)" : "ndt2d: moments + finalise");
  GridDev& g = h->grid;
  const size_t ncell1 = (size_t)g.W * g.H, ncell = ncell1 * g.ngrid;
  const int ntx = (g.W + kTile - 1) >> kTileShift, nty = (g.H + kTile - 1) >> kTileShift;
  const long long ntile_ll = (long long)ntx * nty;
  SortPlan sp;
  if (h->use_binned_build && h->build_variant == 1 && ntile_ll <= kBinMaxTiles && plan_sorted(n, ntile_ll, &sp)) {
    const int ntile = (int)ntile_ll;
    SplitBufs sb{};
    { const int32_t es = ensure_sorted_buffers(h, sp, n, ntile, &sb); if (es != NDT_OK) return es; }
    if (!h->acc_clean) HIP_TRY(hipMemsetAsync(h->d_acc2, 0, 512, h->stream));      // (first build, or one that failed half-way)
    h->acc_clean = false;
    unsigned char* cur = h->d_acc2 + 256 * h->acc_parity;
    unsigned char* nxt = h->d_acc2 + 256 * (1 - h->acc_parity);
    const MoveArgs none{1.f, 0.f, 0.f, 0.f, 0};
    { const int32_t bs = enqueue_sorted_build(h, d_x, d_y, n, sp, sb, ntile, merge, move ? *move : none, GeomArgs{},
                                              reinterpret_cast<int*>(cur), reinterpret_cast<unsigned long long*>(cur + 128),
                                              reinterpret_cast<unsigned int*>(nxt), sign);
      if (bs != NDT_OK) return bs; }
    h->last_ntile = ntile;
    int* hc = (int*)h->h_small;
    unsigned long long* ho = (unsigned long long*)((char*)h->h_small + 128);
    static_assert(ndt::kCountInts * sizeof(int) == 128, "the accumulator halves mirror h_small: counters at 0, outside at 128");
    { const int32_t ps = read_back(h, cur, hc, ndt::kCountWords); if (ps != NDT_OK) return ps; }   // counter shards, outside count, broken cells
    h->acc_parity ^= 1;
    h->acc_clean = true;
    int n_valid_sum = 0, n_over_sum = 0;
    sum_count_shards(hc, &n_valid_sum, &n_over_sum);
    h->n_valid = merge ? h->n_valid + n_valid_sum : n_valid_sum;       // merge: the gather kernel counts the change, tile by touched tile
    if (h_outside) *h_outside = *ho;
    if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
    return sign < 0 ? check_removal(hc) : NDT_OK;
  }
  // the other paths take the points as they are: move them into the map frame first
  if (move && move->use) {
    HIP_TRY(grow({grow_buf(&h->d_t[0]), grow_buf(&h->d_t[1])}, &h->tcap, n, n + n / 4 + 1024));
    hipLaunchKernelGGL(k_transform_points, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, d_x, d_y,
                       n, move->cs, move->sn, move->tx, move->ty, h->d_t[0], h->d_t[1]);
    HIP_TRY(hipGetLastError());
    d_x = h->d_t[0]; d_y = h->d_t[1];
  }
  HIP_TRY(hipMemsetAsync(h->d_outside, 0, sizeof(unsigned long long), h->stream));
  if (h->use_binned_build && ntile_ll <= kBinMaxTiles && n <= 0xFFFFFFFFull) {
    const int ntile = (int)ntile_ll;
    { const int32_t es = ensure_binned_buffers(h, n, ntile); if (es != NDT_OK) return es; }
    HIP_TRY(hipMemsetAsync(h->d_counters, 0, ndt::kCountWords * sizeof(int), h->stream));
    { const int32_t bs = enqueue_binned_build(h, d_x, d_y, n, ntile, merge, nullptr, nullptr, h->d_counters, h->d_outside, sign);
      if (bs != NDT_OK) return bs; }
    h->last_ntile = ntile;
    int* hc = (int*)h->h_small;
    unsigned long long* ho = (unsigned long long*)((char*)h->h_small + 128);
    HIP_TRY(hipMemcpyAsync(hc, h->d_counters, ndt::kCountWords * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(ho, h->d_outside, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));   // (over the two spare words)
    HIP_TRY(hipStreamSynchronize(h->stream));
    int n_valid_sum = 0, n_over_sum = 0;
    sum_count_shards(hc, &n_valid_sum, &n_over_sum);
    h->n_valid = n_valid_sum;
    if (h_outside) *h_outside = *ho;
    if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
    return sign < 0 ? check_removal(hc) : NDT_OK;
  }
  // fallback: scattered global atomics
  if (!merge) HIP_TRY(hipMemsetAsync(g.acc, 0, ncell * sizeof(CellAcc), h->stream));
  if (sign < 0) hipLaunchKernelGGL((k_accumulate<-1>), dim3(stream_blocks(n)), dim3(kBlock), 0, h->stream, d_x, d_y, n, g, h->d_outside);
  else hipLaunchKernelGGL((k_accumulate<1>), dim3(stream_blocks(n)), dim3(kBlock), 0, h->stream, d_x, d_y, n, g, h->d_outside);
  HIP_TRY(hipGetLastError());
  unsigned long long* ho = (unsigned long long*)((char*)h->h_small + 128);
  HIP_TRY(hipMemcpyAsync(ho, h->d_outside, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  const int32_t st = finalise_grid(h, sign);
  if (h_outside) *h_outside = *ho;
  return st;
}

// storage for ncell cells (all grids): a 32-byte record (two float4) and the sums of each
int32_t ensure_cells(ndt2d_handle* h, size_t ncell) {
  HIP_TRY(grow({grow_buf(&h->grid.rec, 2), grow_buf(&h->grid.acc)}, &h->cell_capacity, ncell, ncell + ncell / 8));
  return NDT_OK;
}

// Grid geometry for a bounding box (oracle/ndt2d.py grid_geometry) and storage for its cells.
int32_t setup_geometry(ndt2d_handle* h, float xmin, float xmax, float ymin, float ymax) {
  const double c = h->prm.cell_size;
  GridDev& g = h->grid;
  g.cell = c;
  g.cell32 = (float)c;
  g.inv_c = lattice_inv_c(c);
  const LatticeAxis X = lattice_axis(xmin, xmax, c), Y = lattice_axis(ymin, ymax, c);   // the rule the kernels call
  g.ox = X.origin;
  g.oy = Y.origin;
  const double kx = X.k, ky = Y.k;
  if (!(kx >= 0.0) || !(ky >= 0.0) || (kx + 2.0) * (ky + 2.0) > (double)kMaxCells) {
    set_error("target extent / cell_size needs more than 2^27 cells");
    return NDT_ERR_CAPACITY;
  }
  // overlapping grids: origins move down by half a cell, one extra column/row covers the maximum
  g.ngrid = h->prm.overlap_grids == 4 ? 4 : 1;
  g.pad = 0;
  const int extra = g.ngrid > 1 ? 1 : 0;
  g.W = (int)kx + 2 + extra;
  g.H = (int)ky + 2 + extra;
  for (int q = 0; q < kMaxGrids; ++q) {
    g.gx[q] = lattice_origin(X.base, overlap_shift(q, 0), c);
    g.gy[q] = lattice_origin(Y.base, overlap_shift(q, 1), c);
  }
  g.fix_scale = std::ldexp(1.0, kFixShift) / c;
  const size_t ncell = (size_t)g.W * g.H * g.ngrid;     // all grids, back to back
  if (ncell > kMaxCells) { set_error("target extent / cell_size needs more than 2^27 cells"); return NDT_ERR_CAPACITY; }
  return ensure_cells(h, ncell);
}

// ndt2d_set_target with ONE host round trip: bounds -> geometry (k_geometry, on the device, into d_static) ->
// binned build, enqueued back to back; the host learns the geometry together with the counters.  Possible
// when the handle already holds storage and parameters on the device (any earlier target) and the new grid
// fits them and the launch bound chosen here; otherwise *done = false (with the bounding box in hb_out when
// the device got that far) and the caller builds the usual way.
int32_t set_target_single_sync(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, bool* done, unsigned int* hb_out,
                               bool* have_bounds) {
  *done = false; *have_bounds = false;
  if (!h->one_round_trip || !h->use_binned_build || h->prm.overlap_grids == 4 || h->cell_capacity == 0 || !h->static_on_device ||
      h->last_ntile <= 0 || n > 0xFFFFFFFFull || !h->grid.rec || !h->grid.acc)
    return NDT_OK;
  long long tb = 2ll * h->last_ntile + 16;
  if (tb > kBinMaxTiles) tb = kBinMaxTiles;
  const int tile_bound = (int)tb;
  if (!h->d_geom) HIP_TRY(hipMalloc((void**)&h->d_geom, sizeof(GeomDev)));
  if (!h->h_geom) HIP_TRY(pinned_alloc(&h->h_geom, sizeof(GeomDev)));
  GeomDev* dg = h->d_geom;
  GridDev* dgrid = &h->d_static->grid;
  SortPlan sp;
  if (h->build_variant == 1 && plan_sorted(n, tile_bound, &sp)) {
    // chunk-sorted build: bounds partials -> chunk sort (reduce + geometry in its prologue) -> one workgroup per tile
    SplitBufs sb{};
    { const int32_t es = ensure_sorted_buffers(h, sp, n, tile_bound, &sb); if (es != NDT_OK) return es; }
    const int nparts = launch_bounds_parts(h, d_x, d_y, n, dg);
    GeomArgs ga{};
    ga.parts = h->d_parts; ga.nparts = nparts; ga.tile_bound = tile_bound; ga.cell = h->prm.cell_size;
    ga.cell_capacity = (unsigned long long)h->cell_capacity; ga.grid = dgrid; ga.out = dg;
    const MoveArgs stay{1.f, 0.f, 0.f, 0.f, 0};
    { const int32_t bs = enqueue_sorted_build(h, d_x, d_y, n, sp, sb, tile_bound, false, stay, ga, &dg->counters[0], &dg->n_outside,
                                              nullptr);
      if (bs != NDT_OK) return bs; }
  } else {
    // round-1 binned build: clear counters and tile totals -> bounds -> geometry -> count, scan, scatter, accumulate
    { const int32_t es = ensure_binned_buffers(h, n, tile_bound); if (es != NDT_OK) return es; }
    hipLaunchKernelGGL(k_build_init, dim3(1), dim3(1024), 0, h->stream, dg, h->d_tiles, tile_bound);
    hipLaunchKernelGGL(k_bounds, dim3(stream_blocks(n) > kBoundsBlocks ? kBoundsBlocks : stream_blocks(n)), dim3(kBlock), 0, h->stream,
                       d_x, d_y, n, &dg->bounds[0]);
    hipLaunchKernelGGL(k_geometry, dim3(1), dim3(64), 0, h->stream, h->prm.cell_size, (unsigned long long)h->cell_capacity, tile_bound,
                       dgrid, dg);
    { const int32_t bs = enqueue_binned_build(h, d_x, d_y, n, tile_bound, false, dg, dgrid, &dg->counters[0], &dg->n_outside);
      if (bs != NDT_OK) return bs; }
  }
  GeomDev* hg = h->h_geom;
  static_assert(sizeof(GeomDev) % 4 == 0, "GeomDev travels to the host word by word");
  { const int32_t ps = read_back(h, dg, hg, (int)(sizeof(GeomDev) / 4)); if (ps != NDT_OK) return ps; }
  const int* hc = hg->counters;
  for (int j = 0; j < 4; ++j) hb_out[j] = hg->bounds[j];
  *have_bounds = true;
  if (!hg->ok) return NDT_OK;                            // does not fit storage or bound (or no finite point): the usual way
  // the host's view of the same geometry, from the same bounds by the function the kernel called (lattice_axis): the
  // comparison guards the storage and the launch bound; storage is large enough, nothing is reallocated
  const int32_t gs = setup_geometry(h, ordered_to_float(hg->bounds[0]), ordered_to_float(hg->bounds[1]),
                                    ordered_to_float(hg->bounds[2]), ordered_to_float(hg->bounds[3]));
  if (gs != NDT_OK) return NDT_OK;
  if (h->grid.W != hg->bin.W || h->grid.H != hg->bin.H || h->grid.ox != hg->bin.ox || h->grid.oy != hg->bin.oy) return NDT_OK;
  h->h_static->grid = h->grid;                           // what d_static holds already
  h->last_ntile = hg->bin.ntile;
  int n_valid_sum = 0, n_over_sum = 0;
  sum_count_shards(hc, &n_valid_sum, &n_over_sum);
  h->n_valid = n_valid_sum;
  if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
  *done = true;
  return NDT_OK;
}

int32_t set_target_impl(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n) {
  TraceRange range("ndt2d_set_target: grid build");
  h->has_target = false;
  grid_changed(h);
  if (n == 0) return NDT_ERR_INVALID_ARG;
  unsigned int fast_bounds[4];
  bool done = false, have_bounds = false;
  { const int32_t fs = set_target_single_sync(h, d_x, d_y, n, &done, fast_bounds, &have_bounds); if (fs != NDT_OK) return fs; }
  if (done) {
    h->n_points = n;
    h->has_target = true;
    return NDT_OK;
  }
  // a1: bounding box on the device, geometry on the host (oracle/ndt2d.py grid_geometry)
  unsigned int init[4] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
  unsigned int* hb = (unsigned int*)h->h_small;
  if (have_bounds) {                                      // the single-sync attempt measured the box already
    std::memcpy(hb, fast_bounds, sizeof(init));
  } else {
    std::memcpy(hb, init, sizeof(init));
    {
      const int nparts = launch_bounds_parts(h, d_x, d_y, n);
      hipLaunchKernelGGL(k_bounds_reduce, dim3(1), dim3(64), 0, h->stream, (const float4*)h->d_parts, nparts, h->d_bounds);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hb, h->d_bounds, sizeof(init), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (hb[0] == 0xFFFFFFFFu || hb[1] == 0u) { set_error("target has no finite point"); return NDT_ERR_INVALID_ARG; }
  const int32_t gs = setup_geometry(h, ordered_to_float(hb[0]), ordered_to_float(hb[1]), ordered_to_float(hb[2]),
                                    ordered_to_float(hb[3]));
  if (gs != NDT_OK) return gs;
  // a2 + a3
  const int32_t st = accumulate_and_finalise(h, d_x, d_y, n, /*merge=*/false, nullptr);
  if (st != NDT_OK) return st;
  h->n_points = n;
  h->has_target = true;
  return upload_static(h);
}

// Static part of the device context: grid + solver parameters.  Uploaded (synchronously)
// whenever the target changes; the per-call part is written by the chain's first launch (k_iterate_first; k_begin under
// the old protocol) from kernel arguments, so no host buffer has to outlive an asynchronous call.
// the solver's part of the device context (2D and 3D: ndt3d_params is ndt2d_params)
void set_solve_params(SolveParams* p, const ndt2d_params& q) {
  p->d1 = (float)q.d1;
  p->d2 = (float)q.d2;
  p->hessian_mode = q.hessian_mode;
  p->max_iterations = q.max_iterations;
  p->min_hits = q.min_hits;
  p->line_search = q.line_search;
  p->eps_trans = q.eps_trans;
  p->eps_rot = q.eps_rot;
  p->step_max_trans = q.step_max_trans;
  p->step_max_rot = q.step_max_rot;
  p->step_scale = q.step_scale > 0.0 ? q.step_scale : 1.0;
}

int32_t upload_static(ndt2d_handle* h) {
  // The copy is left in flight (everything that reads d_static is ordered behind it on the same
  // stream); the pinned source is only rewritten once the previous copy has left it.
  HIP_TRY(hipEventSynchronize(h->upload_ev));
  AlignStatic* c = h->h_static;
  c->grid = h->grid;
  set_solve_params(&c->prm, h->prm);
  HIP_TRY(hipMemcpyAsync(h->d_static, c, sizeof(AlignStatic), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventRecord(h->upload_ev, h->stream));
  h->static_on_device = true;
  return NDT_OK;
}

// The parameters every alignment kernel is instantiated for, as template arguments: returns f(MODE, NG), called with
// std::integral_constant values of the Hessian (MODE 1: Newton) and the grid count (NG 4: overlapping grids).
template <class F>
auto with_mode(const ndt2d_params& p, F&& f) {
  using Zero = std::integral_constant<int, 0>;
  using One = std::integral_constant<int, 1>;
  using Four = std::integral_constant<int, 4>;
  if (p.hessian_mode == NDT_HESSIAN_NEWTON) return p.overlap_grids == 4 ? f(One{}, Four{}) : f(One{}, One{});
  return p.overlap_grids == 4 ? f(Zero{}, Four{}) : f(Zero{}, One{});
}

// the k_iterate of an alignment, for graphs and plain launches (scan_chain).  wide: 1024-thread
// workgroups - a property of the call (its scan size), calls in flight on different lanes may differ in it
const void* iter_kernel(const ndt2d_handle* h, bool wide) {
  return with_mode(h->prm, [&](auto M, auto NG) {
    return wide ? (const void*)&k_iterate<M, 0, kIterThreadsWide, NG> : (const void*)&k_iterate<M, 0, kIterThreads, NG>;
  });
}
// launch 0 of a chain with k_begin folded in: the same instances
const void* first_kernel(const ndt2d_handle* h, bool wide) {
  return with_mode(h->prm, [&](auto M, auto NG) {
    return wide ? (const void*)&k_iterate_first<M, kIterThreadsWide, NG> : (const void*)&k_iterate_first<M, kIterThreads, NG>;
  });
}
int iter_threads(bool wide) { return wide ? kIterThreadsWide : kIterThreads; }
bool is_wide(const ndt2d_handle* h, size_t n) { return h->use_wide && n >= h->wide_threshold; }

// The k_iterate chain of a scan of n points on `lane`: the kernels read everything (grid, source pointers, n, parameters,
// state) from device memory, so one graph of it serves every target and every source - of its lane: the per-call and
// dynamic contexts are baked into it.
ChainLaunch scan_chain(const ndt2d_handle* h, size_t n, int lane) {
  const bool wide = is_wide(h, n);
  return {iter_kernel(h, wide), dim3(blocks_for(n)), dim3(iter_threads(wide)), h->d_static, h->call_of(lane), h->dyn_of(lane)};
}

// the first launch of the old protocol, on `lane` and its stream: launches 0 .. K follow
void launch_begin(ndt2d_handle* h, int lane, hipStream_t stream, const float* const* d_s, size_t n, const double* pose, int fixed,
                  IterState* host_state, int* host_flag) {
  hipLaunchKernelGGL(k_begin, dim3(1), dim3(64), 0, stream, h->call_of(lane), h->dyn_of(lane), d_s[0], d_s[1], (int)n, pose[0],
                     pose[1], pose[2], fixed, host_state, host_flag, h->flight.call_seq);
}

// Enqueue the Gauss-Newton loop of ndt2d_evaluate* (fixed_override = 1) and ndt2d_align* (-1).  wait: the caller fetches
// the state next; own_source: the scan is in the handle's staging arrays.  The head of the chain: everything behind
// launch 0 is run_chain_tail's.
int32_t begin_align(ndt2d_handle* h, const float* const* d_s, size_t n, const double* pose, int fixed_override, bool wait,
                    bool own_source) {
  TraceRange range("ndt2d_align: Gauss-Newton loop");
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  { const int32_t fs = finish_host_fed(h); if (fs != NDT_OK) return fs; }     // an unfinished asynchronous call
  if (n == 0 || n > kMaxSourcePoints || !pose) { (void)lane_step(h->lanes, LaneEvent::kOther); return NDT_ERR_INVALID_ARG; }
  if (h->n_valid < 1) {
    (void)lane_step(h->lanes, LaneEvent::kOther);
    h->flight.how = ChainFlight::kOnHost;
    *h->h_state = no_cell_state<IterState>(pose);
    return NDT_OK;
  }
  const ChainPlan p = chain_plan(fixed_override, h->prm.fixed_iterations, h->prm.max_iterations, h->use_graph, h->check_every,
                                 h->fused_begin);
  const bool small = h->use_small && h->use_graph && n <= (size_t)kSmallMaxPoints;
  // Only a whole fixed-iteration chain that nobody waits for goes round the lanes; everything else runs on
  // lane 0 and starts the rotation over.
  const LanePlan plan = lane_step(h->lanes, p.fixed > 0 && h->use_graph && !small && !wait ? LaneEvent::kAsyncFixed : LaneEvent::kOther);
  next_seq(&h->flight.call_seq, h->h_flag);
  if (small) {
    // short scan: the whole loop in one launch of one workgroup (ndt2d_small.hpp)
    const bool lo = n <= (size_t)kSmallLoPoints;
    const void* func = with_mode(h->prm, [&](auto M, auto NG) {
      return lo ? (const void*)&k_align_small<M, NG, kSmallThreadsLo> : (const void*)&k_align_small<M, NG, kSmallThreadsHi>;
    });
    int ni = (int)n;
    IterState* dev_state = &h->d_dyn->state[0];
    void* args[] = {&h->d_static, (void*)&d_s[0], (void*)&d_s[1], &ni, (void*)&pose[0], (void*)&pose[1], (void*)&pose[2],
                    (void*)&p.fixed, &dev_state, &h->h_state, &h->h_flag};
    (void)hipLaunchKernel(func, dim3(1), dim3(lo ? kSmallThreadsLo : kSmallThreadsHi), args, 0, h->stream);
    HIP_TRY(hipGetLastError());
    h->flight.how = ChainFlight::kSmallRun;              // its last thread writes h_state, then raises the flag
    return NDT_OK;
  }
  hipStream_t stream = h->stream;
  // the fork: where non-chain work on the handle's stream may precede the round (or at every round, NDT_TUNE_LANE_FORK = 1),
  // one event per secondary lane in use
  // (a record that fails must not leave the state claiming a fork: the rule is kept across calls, so the lanes stay stale)
  if (h->fork_every_pair ? plan.record_fork : plan.mark) {
    for (int l = 1; l < h->lanes.lanes; ++l) {
      const hipError_t fe = h->lane[l - 1].mark_fork(h->stream);
      if (fe != hipSuccess) (void)lane_step(h->lanes, LaneEvent::kOther);
      HIP_TRY(fe);
    }
  }
  AsyncLane* const side = plan.lane ? &h->lane[plan.lane - 1] : nullptr;
  if (side) {
    if (h->fork_every_pair || plan.wait) {
      const hipError_t we = side->enter();
      if (we != hipSuccess) (void)lane_step(h->lanes, LaneEvent::kOther);
      HIP_TRY(we);
    }
    stream = side->stream;
  }
  // Launch 0.  Fused (the default): k_iterate_first, a plain launch that evaluates at the initial pose and writes the
  // per-call context from its arguments; launches 1 .. K follow.  Old protocol: k_begin, then launches 0 .. K.
  const bool wide = is_wide(h, n);
  const ChainLaunch c = scan_chain(h, n, plan.lane);
  IterState* const host_state = p.chunked ? h->h_state : (IterState*)nullptr;
  int* const host_flag = p.chunked ? h->h_flag : (int*)nullptr;
  if (p.first) {
    int ni = (int)n;
    void* args[] = {(void*)&c.a0, (void*)&c.a1, (void*)&c.a2, (void*)&d_s[0], (void*)&d_s[1], &ni, (void*)&pose[0], (void*)&pose[1],
                    (void*)&pose[2], (void*)&p.fixed, (void*)&host_state, (void*)&host_flag, &h->flight.call_seq};
    (void)hipLaunchKernel(first_kernel(h, wide), c.grid, c.block, args, 0, stream);
  } else {
    launch_begin(h, plan.lane, stream, d_s, n, pose, p.fixed, host_state, host_flag);
  }
  // (drain: the handle's own staging arrays outlive the call)
  return run_chain_tail(h, c, h->prm.hessian_mode | (wide ? 16 : 0), plan.lane, stream, side, p, !own_source);
}

void sym6_to_9(const double* s, double* H) {
  H[0] = s[0]; H[1] = s[1]; H[2] = s[3];
  H[3] = s[1]; H[4] = s[2]; H[5] = s[4];
  H[6] = s[3]; H[7] = s[4]; H[8] = s[5];
}

// IterState -> ndt2d_result, or -> ndt2d_eval (the fields it shares with the result)
template <class Out>
void state_to(const IterState& s, Out* out) {
  std::memset(out, 0, sizeof(*out));
  sym6_to_9(s.H, out->H);
  for (int j = 0; j < 3; ++j) out->g[j] = s.g[j];
  out->score = s.score;
  out->n_hit = s.n_hit;
  if constexpr (std::is_same<Out, ndt2d_result>::value) {
    for (int j = 0; j < 3; ++j) out->pose[j] = s.pose[j];
    out->iterations = s.iter;
    out->status = s.status;
  }
}

// The 2D side of the host code both handles share (ndt_chain_host.hpp, ndt_search.hpp, ndt_map_host.hpp)
template <> struct HandleTraits<ndt2d_handle> {
  using State = IterState;
  using Result = ndt2d_result;
  using Window = ndt2d_search_window;
  using Hit = ndt2d_search_hit;
  using Poses = StartPoses;
  using Maps = StartMaps;
  static constexpr int kDim = 2, kPose = 3, kMaxStarts = ndt::kMaxStarts;
  static constexpr int kRecord = 2;                        // float4 per covariance record and per component
  // the state of a fixed chain is copied at fetch_state, from the lane the chain ran on (3D: the copy is enqueued behind the chain)
  static constexpr bool kQueuedFetch = false;
  static constexpr const char* kCell = "cell";
  static constexpr const char* kTraceComponents = "ndt2d: component list";
  static constexpr const char* kTraceAlignTrace = "ndt2d_align_trace";
  static constexpr const char* kTraceMapPair = "ndt2d_align_map: Gauss-Newton loop";
  static constexpr const char* kTraceMapMulti = "ndt2d_align_map_multi";
  static constexpr const char* kMapMultiNoEnd = "the map-to-map multi-start loop did not report its end";
  static size_t cells(const ndt2d_handle* h) { return (size_t)h->grid.W * h->grid.H; }
  // a 2D target scores a component against its own cell only (the map neighbourhood is a 3D handle's setting)
  static int map_neighbourhood(const ndt2d_handle*) { return 1; }
  static int map_graph_mode(const ndt2d_handle* h) { return h->prm.hessian_mode; }
  static constexpr const char* kMapNeighbourhoodSetter = "";
  template <class... A> static int32_t begin(A... a) { return begin_align(a...); }
  template <class... A> static ChainLaunch scan_chain(A... a) { return ::scan_chain(a...); }
  template <class... A> static void launch_begin(A... a) { ::launch_begin(a...); }
  template <class Out> static void to(const IterState& s, Out* out) { state_to(s, out); }
  static void launch_cov_records(ndt2d_handle* h, unsigned nb) {
    hipLaunchKernelGGL(k_cov_records, dim3(nb), dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points, h->prm.eig_ratio,
                       h->d_cov, h->d_blk);
  }
  static void launch_components(ndt2d_handle* h, unsigned nb, unsigned ncell, const unsigned int* offsets, unsigned n) {
    hipLaunchKernelGGL(k_components, dim3(nb), dim3(kBlock), 0, h->stream, (const float4*)h->d_cov, ncell, offsets, h->d_comp, n);
  }
  // one component of the list as ndt2d_get_components hands it out
  static void unpack_component(const float4* c, size_t i, float* mean_xy, float* cov_abc, int32_t* key) {
    const float4 a = c[0], b = c[1];
    if (mean_xy) { mean_xy[2 * i] = a.x; mean_xy[2 * i + 1] = a.y; }
    if (cov_abc) { cov_abc[3 * i] = a.z; cov_abc[3 * i + 1] = a.w; cov_abc[3 * i + 2] = b.y; }
    if (key) std::memcpy(&key[i], &b.z, sizeof(int32_t));
  }
  static SearchWindow window(const ndt2d_search_window& w) {
    SearchWindow v;
    for (int a = 0; a < 3; ++a) { v.center[a] = w.center[a]; v.half_extent[a] = w.half_extent[a]; v.step[a] = w.step[a]; }
    v.min_sep_trans = w.min_sep_trans; v.min_sep_rot = w.min_sep_rot;
    return v;
  }
  // the walk's peaks as the ABI's hits
  static void hits_out(const SearchPeak* peaks, int32_t n, const ndt2d_search_window&, ndt2d_search_hit* hits) {
    for (int32_t q = 0; q < n; ++q) {
      ndt2d_search_hit& hh = hits[q];
      std::memset(&hh, 0, sizeof(hh));
      for (int a = 0; a < 3; ++a) hh.pose[a] = peaks[q].pose[a];
      hh.score = peaks[q].score;
      hh.index = peaks[q].index;
    }
  }
};

}  // namespace

// ------------------------------------------------------------------------------ C ABI
extern "C" {

int32_t ndt_abi_version(void) { return NDT_ABI_VERSION; }

const char* ndt_status_string(int32_t s) {
  switch (s) {
    case NDT_OK: return "ok";
    case NDT_NOT_CONVERGED: return "not converged (max_iterations reached)";
    case NDT_DEGENERATE_HESSIAN: return "degenerate Hessian";
    case NDT_TOO_FEW_HITS: return "too few source points in valid cells";
    case NDT_TOO_FEW_CELLS: return "target grid has no valid cell";
    case NDT_ERR_INVALID_ARG: return "invalid argument";
    case NDT_ERR_NO_TARGET: return "no target set";
    case NDT_ERR_HIP: return "HIP error";
    case NDT_ERR_NO_DEVICE: return "no HIP device";
    case NDT_ERR_CAPACITY: return "capacity limit exceeded";
    case NDT_ERR_ALLOC: return "allocation failed";
    case NDT_ERR_RCCL: return "RCCL error";
    default: return "unknown status";
  }
}

const char* ndt_last_error(void) { return last_error().c_str(); }

int32_t ndt_set_host_wait(int32_t mode) {
  if (mode != 0 && mode != 1) return NDT_ERR_INVALID_ARG;
  ndt::host_wait_mode().store(mode, std::memory_order_relaxed);
  return NDT_OK;
}

int32_t ndt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

int32_t ndt_magnusson_constants(double outlier_ratio, double cell_size, int32_t dim, double* d1, double* d2) {
  if (!d1 || !d2 || !(outlier_ratio > 0.0) || !(outlier_ratio < 1.0) || !(cell_size > 0.0) || (dim != 2 && dim != 3))
    return NDT_ERR_INVALID_ARG;
  const double c1 = 10.0 * (1.0 - outlier_ratio);
  const double c2 = outlier_ratio / std::pow(cell_size, (double)dim);
  const double d3 = -std::log(c2);
  const double md1 = -std::log(c1 + c2) - d3;                      // Magnusson's d1 (negative)
  const double md2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / md1);
  if (!std::isfinite(md1) || !std::isfinite(md2) || !(md1 < 0.0) || !(md2 > 0.0)) return NDT_ERR_INVALID_ARG;
  *d1 = -md1;
  *d2 = md2;
  return NDT_OK;
}

int32_t ndt2d_calibrated_covariance(const double H[9], int32_t hessian_mode, double cov[9]) {
  if (!H || !cov || (hessian_mode != NDT_HESSIAN_GAUSS_NEWTON && hessian_mode != NDT_HESSIAN_NEWTON)) return NDT_ERR_INVALID_ARG;
  for (int i = 0; i < 9; ++i) cov[i] = 0.0;
  // symmetric 3x3 inverse by cofactors, positive definiteness by the leading minors
  const double a = H[0], b = 0.5 * (H[1] + H[3]), c = 0.5 * (H[2] + H[6]), d = H[4], e = 0.5 * (H[5] + H[7]), f = H[8];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  if (!(a > 0.0) || !(a * d - b * b > 0.0) || !(det > 0.0) || !std::isfinite(det)) return NDT_DEGENERATE_HESSIAN;
  const bool newton = hessian_mode == NDT_HESSIAN_NEWTON;
  const double st = std::sqrt(newton ? NDT_COV_SCALE_NEWTON_TRANS : NDT_COV_SCALE_GN_TRANS);
  const double sr = std::sqrt(newton ? NDT_COV_SCALE_NEWTON_ROT : NDT_COV_SCALE_GN_ROT);
  const double S[3] = {st, st, sr};
  const double inv[9] = {c00 / det, c01 / det, c02 / det, c01 / det, (a * f - c * c) / det, (b * c - a * e) / det,
                         c02 / det, (b * c - a * e) / det, (a * d - b * b) / det};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) cov[3 * i + j] = S[i] * inv[3 * i + j] * S[j];
  return NDT_OK;
}

int32_t ndt2d_polar_to_points_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc,
                                  double range_min, double range_max, float* d_x, float* d_y, void* stream) {
  if (!d_ranges || !d_x || !d_y || n == 0 || !std::isfinite(angle_min) || !std::isfinite(angle_inc))
    return NDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_polar_to_points, dim3(stream_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, d_ranges, n,
                     angle_min, angle_inc, (float)range_min, (float)range_max, d_x, d_y);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

void ndt2d_default_params(ndt2d_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->cell_size = 0.5;
  p->min_points = 3;
  p->hessian_mode = NDT_HESSIAN_GAUSS_NEWTON;
  p->eig_ratio = 1e-3;
  p->d1 = 1.0;
  p->d2 = 1.0;
  p->max_iterations = 100;
  p->fixed_iterations = 0;
  p->eps_trans = 1e-5;
  p->eps_rot = 1e-5;
  p->step_max_trans = 0.5;
  p->step_max_rot = 0.2;
  p->min_hits = 3;
  p->step_scale = 1.0;
}

int32_t ndt2d_create(const ndt2d_params* p, int32_t device_id, ndt2d_handle** out) {
  if (!out) return NDT_ERR_INVALID_ARG;
  *out = nullptr;
  const int32_t st = check_params(p);
  if (st != NDT_OK) return st;
  const int ndev = ndt_device_count();
  if (ndev <= 0) { set_error("no HIP device visible: this library has no CPU fallback"); return NDT_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return NDT_ERR_INVALID_ARG;
  ndt2d_handle* h = new (std::nothrow) ndt2d_handle();
  if (!h) return NDT_ERR_ALLOC;
  h->device = device_id;
  h->prm = *p;
  auto fail = [&](int32_t code) { ndt2d_destroy(h); return code; };
  if (hipSetDevice(device_id) != hipSuccess) return fail(NDT_ERR_HIP);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(NDT_ERR_HIP);
  if (hipMalloc((void**)&h->d_bounds, 4 * sizeof(unsigned int)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_counters, ndt::kCountAlloc * sizeof(int)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_parts, kBoundsParts * sizeof(float4)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_acc2, 512) != hipSuccess) return fail(NDT_ERR_ALLOC);
  {   // k_chunk_sort: 32 KB of points + up to 32 KB of tile histogram, just over the 64 KB a kernel gets without asking
    const int lds = 4096 * (int)sizeof(float2) + kBinMaxTiles * (int)sizeof(unsigned int);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chunk_sort<4>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chunk_sort<8>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chunk_sort<16>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return fail(NDT_ERR_HIP);
  }
  if (hipMalloc((void**)&h->d_outside, sizeof(unsigned long long)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_static, sizeof(AlignStatic)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_call, sizeof(AlignCall)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMalloc((void**)&h->d_dyn, sizeof(AlignDyn)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (pinned_alloc(&h->h_static, sizeof(AlignStatic)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (pinned_alloc(&h->h_state, sizeof(IterState)) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (pinned_alloc(&h->h_flag, 64) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipEventCreateWithFlags(&h->upload_ev, hipEventDisableTiming) != hipSuccess) return fail(NDT_ERR_HIP);
  if (pinned_alloc(&h->h_small, kSmallBytes) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (hipMemset(h->d_dyn, 0, sizeof(AlignDyn)) != hipSuccess) return fail(NDT_ERR_HIP);
  // lanes 1 .. kMaxLanes - 1 of the asynchronous fixed-iteration calls: allocated here, never inside a call that may be timed
  for (int l = 0; l < kMaxLanes - 1; ++l) {
    if (h->lane[l].create() != hipSuccess) return fail(NDT_ERR_HIP);
    if (hipMalloc((void**)&h->d_call_lane[l], sizeof(AlignCall)) != hipSuccess) return fail(NDT_ERR_ALLOC);
    if (hipMalloc((void**)&h->d_dyn_lane[l], sizeof(AlignDyn)) != hipSuccess) return fail(NDT_ERR_ALLOC);
    if (hipMemset(h->d_dyn_lane[l], 0, sizeof(AlignDyn)) != hipSuccess) return fail(NDT_ERR_HIP);
    h->graphs.lane_stream[l] = h->lane[l].stream;
  }
  h->lanes.lanes = ndt2d_handle::kDefaultLanes;
  *out = h;
  return NDT_OK;
}

int32_t ndt2d_destroy(ndt2d_handle* h) {
  if (!h) return NDT_OK;
  (void)hipSetDevice(h->device);
  (void)finish(h);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (int l = 0; l < kMaxLanes - 1; ++l) {
    h->graphs.lane_stream[l] = nullptr;
    h->lane[l].destroy();                   // joins the lane first
  }
  h->graphs.clear();
  if (h->h_state_multi) (void)hipHostFree(h->h_state_multi);
  void* dev[] = {h->d_acc2, h->d_split, h->d_bxy, h->d_table, h->d_parts, h->d_geom, h->d_dyn_multi, h->d_bounds, h->d_counters, h->d_outside, h->d_static, h->d_call, h->d_dyn, h->d_call_lane[0], h->d_dyn_lane[0], h->d_call_lane[1], h->d_dyn_lane[1], h->d_call_lane[2], h->d_dyn_lane[2], h->d_bx, h->d_by, h->d_tiles, h->d_t[0], h->d_t[1], h->d_s[0], h->d_s[1],
                 h->grid.rec, h->grid.acc, h->d_cov, h->d_blk, h->d_comp, h->d_map_call};
  for (void* p : dev) if (p) (void)hipFree(p);
  void* host[] = {h->h_geom, h->h_static, h->h_state, h->h_small, h->h_flag};
  for (void* p : host) if (p) (void)hipHostFree(p);
  h->srch.release();
  h->fit.release();
  h->vox.release();
  if (h->upload_ev) (void)hipEventDestroy(h->upload_ev);
  if (h->wait_ev) (void)hipEventDestroy(h->wait_ev);
  if (h->map_ev) (void)hipEventDestroy(h->map_ev);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return NDT_OK;
}

void* ndt2d_stream(ndt2d_handle* h) { return h ? (void*)h->stream : nullptr; }

int32_t ndt2d_set_tuning(ndt2d_handle* h, int32_t knob, int64_t value) {
  if (!h) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  switch (knob) {
    case NDT_TUNE_LAUNCH_GRAPHS: h->use_graph = value != 0; return NDT_OK;
    case NDT_TUNE_WIDE_THRESHOLD: h->use_wide = value > 0; if (value > 0) h->wide_threshold = (size_t)value; return NDT_OK;
    case NDT_TUNE_SHORT_SCAN_KERNEL: h->use_small = value != 0; return NDT_OK;
    case NDT_TUNE_CHUNK_LAUNCHES: if (value < 2 || value > 128) return NDT_ERR_INVALID_ARG; h->check_every = (int)value; return NDT_OK;
    case NDT_TUNE_BINNED_BUILD:
      if (value < 0 || value > 2) return NDT_ERR_INVALID_ARG;
      h->use_binned_build = value != 0; if (value) h->build_variant = (int)value; return NDT_OK;
    case NDT_TUNE_SPLIT_FROM: if (value < 1 || value > 1000) return NDT_ERR_INVALID_ARG; h->split_from = (int)value; return NDT_OK;
    case NDT_TUNE_SINGLE_SYNC_BUILD: h->one_round_trip = value != 0; return NDT_OK;
    // (both set the number of launch chains; finish above has restarted the rotation and made the lanes stale)
    case NDT_TUNE_ASYNC_LANES: if (value < 1 || value > 2) return NDT_ERR_INVALID_ARG; h->lanes.lanes = (int)value; return NDT_OK;
    case NDT_TUNE_ASYNC_CHAINS: if (value < 1 || value > kMaxLanes) return NDT_ERR_INVALID_ARG; h->lanes.lanes = (int)value; return NDT_OK;
    case NDT_TUNE_MAP_MULTI_FROM: if (value < 1 || value > kMaxStarts + 1) return NDT_ERR_INVALID_ARG; h->map_multi_from = (int)value; return NDT_OK;
    // (the graphs of the two protocols have different first parities in the cache's key and never alias: nothing to drop)
    case NDT_TUNE_FUSED_BEGIN: if (value != 0 && value != 1) return NDT_ERR_INVALID_ARG; h->fused_begin = value != 0; return NDT_OK;
    // (finish above has made the lanes stale, so the first round under either protocol forks)
    case NDT_TUNE_LANE_FORK: if (value != 0 && value != 1) return NDT_ERR_INVALID_ARG; h->fork_every_pair = value != 0; return NDT_OK;
    case NDT_TUNE_PARTICLE_TEAM: if (value != 0 && value != 64 && value != 256) return NDT_ERR_INVALID_ARG; h->particle_team = (int)value; return NDT_OK;
    default: return NDT_ERR_INVALID_ARG;
  }
}

int32_t ndt2d_wait_stream(ndt2d_handle* h, void* producer_stream) {
  if (!h) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const bool own = (hipStream_t)producer_stream == h->stream;
  HIP_TRY(order_after(h->stream, (hipStream_t)producer_stream, &h->wait_ev));      // (nothing to do for the handle's own stream)
  // The next asynchronous call may run on a secondary lane, which is behind the handle's stream only up to its last fork -
  // taken before this wait, and in a run of asynchronous calls long ago.  So the lanes in use wait for the producer too;
  // where that is the handle's own stream (the caller's work on ndt2d_stream), for an event recorded there now.
  if (lane_step(h->lanes, LaneEvent::kWaitStream).both_wait) {
    if (own) {
      if (!h->wait_ev) HIP_TRY(hipEventCreateWithFlags(&h->wait_ev, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(h->wait_ev, h->stream));
    }
    for (int l = 1; l < h->lanes.lanes; ++l) HIP_TRY(hipStreamWaitEvent(h->lane[l - 1].stream, h->wait_ev, 0));
  }
  return NDT_OK;
}

int32_t ndt2d_set_target(ndt2d_handle* h, const float* x, const float* y, size_t n) {
  if (!h || !x || !y || n == 0) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[2] = {x, y};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt2d_set_target_dev(h, h->d_t[0], h->d_t[1], n, nullptr);
}

int32_t ndt2d_set_target_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, void* stream) {
  if (!h || !d_x || !d_y || n == 0) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // producer of d_x/d_y
  return set_target_impl(h, d_x, d_y, n);
}

int32_t ndt2d_reserve_target(ndt2d_handle* h, double xmin, double ymin, double xmax, double ymax) {
  if (!h || !(xmin <= xmax) || !(ymin <= ymax) || !std::isfinite(xmin) || !std::isfinite(xmax) || !std::isfinite(ymin) ||
      !std::isfinite(ymax))
    return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  h->has_target = false;
  grid_changed(h);
  const int32_t gs = setup_geometry(h, (float)xmin, (float)xmax, (float)ymin, (float)ymax);
  if (gs != NDT_OK) return gs;
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.ngrid;
  HIP_TRY(hipMemsetAsync(h->grid.acc, 0, ncell * sizeof(CellAcc), h->stream));
  HIP_TRY(hipMemsetAsync(h->grid.rec, 0, 2 * ncell * sizeof(float4), h->stream));
  h->n_valid = 0;
  h->n_points = 0;
  h->has_target = true;
  return upload_static(h);
}

namespace {

// ndt2d_add_target_points_dev (sign = 1) and ndt2d_remove_target_points_dev (sign = -1): one submap update, with a sign
int32_t update_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, const double pose[3],
                                 size_t* n_outside, void* stream, int sign) {
  if (!h || !d_x || !d_y || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  // (a wrapped count is told from a full cell by its size: removed_cell_broken, ndt2d_kernels.hpp)
  if (sign < 0 && n >= 0xFFF00000ull) { set_error("more points to remove than a call can take (2^32 - 2^20)"); return NDT_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  grid_changed(h);
  // order after the caller's producer stream, as ndt2d_set_target_dev does
  if (stream) HIP_TRY(order_after(h->stream, (hipStream_t)stream));
  // the scan is moved into the map frame inside the build's first kernel (k_chunk_sort; k_transform_points on the other paths)
  MoveArgs mv{1.f, 0.f, 0.f, 0.f, 0};
  if (pose) { mv.cs = (float)std::cos(pose[2]); mv.sn = (float)std::sin(pose[2]); mv.tx = (float)pose[0]; mv.ty = (float)pose[1]; mv.use = 1; }
  unsigned long long outside = 0;
  const int32_t fs = accumulate_and_finalise(h, d_x, d_y, n, /*merge=*/true, &outside, &mv, sign);
  if (n_outside) *n_outside = (size_t)outside;
  if (fs != NDT_OK) { h->has_target = false; return fs; }
  if (sign < 0) h->n_points -= n - (size_t)outside;
  else h->n_points += n - (size_t)outside;
  return NDT_OK;          // geometry, storage and parameters are unchanged: the device context stays as it is
}

}  // namespace

int32_t ndt2d_add_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n,
                                    const double pose[3], size_t* n_outside, void* stream) {
  return update_target_points_dev(h, d_x, d_y, n, pose, n_outside, stream, 1);
}

int32_t ndt2d_remove_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n,
                                       const double pose[3], size_t* n_outside, void* stream) {
  return update_target_points_dev(h, d_x, d_y, n, pose, n_outside, stream, -1);
}

int32_t ndt2d_remove_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n, size_t* n_outside) {
  if (!h || !x || !y || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[2] = {x, y};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt2d_remove_target_points_dev(h, h->d_t[0], h->d_t[1], n, nullptr, n_outside, nullptr);
}

int32_t ndt2d_add_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n, size_t* n_outside) {
  if (!h || !x || !y || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const t[2] = {x, y};
  { const int32_t ss = stage_target(h, t, n); if (ss != NDT_OK) return ss; }
  return ndt2d_add_target_points_dev(h, h->d_t[0], h->d_t[1], n, nullptr, n_outside, nullptr);
}

int32_t ndt2d_get_grid_info(ndt2d_handle* h, ndt2d_grid_info* info) {
  if (!h || !info) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  info->ox = h->grid.ox; info->oy = h->grid.oy;
  info->inv_cell = h->grid.inv_c; info->cell = h->grid.cell32;
  info->width = h->grid.W; info->height = h->grid.H;
  info->n_valid = h->n_valid; info->n_points = (int32_t)h->n_points;
  return NDT_OK;
}

int32_t ndt2d_get_grid(ndt2d_handle* h, int32_t* count, float* mean_xy, float* icov_abc) {
  if (!h) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const size_t ncell = (size_t)h->grid.W * h->grid.H;          // grid 0 (the unshifted one)
  float4* rec = new (std::nothrow) float4[2 * ncell];
  CellAcc* acc = count ? new (std::nothrow) CellAcc[ncell] : nullptr;
  int32_t rc = NDT_OK;
  if (!rec || (count && !acc)) rc = NDT_ERR_ALLOC;
  if (rc == NDT_OK && hipMemcpyAsync(rec, h->grid.rec, 2 * ncell * sizeof(float4), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK && acc && hipMemcpyAsync(acc, h->grid.acc, ncell * sizeof(CellAcc), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = NDT_ERR_HIP;
  if (rc == NDT_OK) {
    for (size_t k = 0; k < ncell; ++k) {
      const float4 a = rec[2 * k], b = rec[2 * k + 1];
      if (count) count[k] = (int32_t)acc[k].n;
      if (mean_xy) { mean_xy[2 * k] = a.x; mean_xy[2 * k + 1] = a.y; }
      if (icov_abc) {
        const bool valid = b.z > 0.f;
        icov_abc[3 * k] = valid ? a.z : 0.f;
        icov_abc[3 * k + 1] = valid ? a.w : 0.f;
        icov_abc[3 * k + 2] = valid ? b.y : 0.f;
      }
    }
  } else if (rc == NDT_ERR_HIP) {
    set_error(hipGetErrorString(hipGetLastError()));
  }
  delete[] rec; delete[] acc;
  return rc;
}

int32_t ndt2d_evaluate(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double pose[3],
                       ndt2d_eval* out) {
  const float* const s[2] = {sx, sy};
  return evaluate_host(h, s, n, pose, out);
}

int32_t ndt2d_evaluate_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3],
                           ndt2d_eval* out) {
  const float* const s[2] = {d_sx, d_sy};
  return evaluate_dev(h, s, n, pose, out);
}

int32_t ndt2d_align_trace(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double init_pose[3],
                          ndt2d_result* rows, int32_t capacity, int32_t* n_rows, ndt2d_result* out) {
  const float* const s[2] = {sx, sy};
  return align_trace(h, s, n, init_pose, rows, capacity, n_rows, out);
}

int32_t ndt2d_align_finish(ndt2d_handle* h, ndt2d_result* out) { return align_finish(h, out); }

int32_t ndt2d_align_dev_async(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                              const double init_pose[3]) {
  const float* const s[2] = {d_sx, d_sy};
  return align_dev_async(h, s, n, init_pose);
}

int32_t ndt2d_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                        const double init_pose[3], ndt2d_result* out) {
  const float* const s[2] = {d_sx, d_sy};
  return align_dev(h, s, n, init_pose, out);
}

int32_t ndt2d_align(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double init_pose[3],
                    ndt2d_result* out) {
  const float* const s[2] = {sx, sy};
  return align_host(h, s, n, init_pose, out);
}

}  // extern "C"


// ---- multi-start alignment (ndt2d_multi_start.hpp) ---------------------------------------------
namespace {

// The chain kernel of a multi-start call: the fused chain's k_iterate_multi (nh starts per workgroup), or split, the split
// chain's k_multi_body (one start per workgroup; k_multi_solve is the chain's other kernel)
template <int MODE, int NG, int THREADS, bool SHARED>
const void* multi_kernel_of(bool split, int nh) {
  if (split) return (const void*)&k_multi_body<MODE, 1, THREADS, SHARED, NG>;
  // overlapping grids: one start per workgroup; a 1024-thread workgroup fills its CU with one start
  if constexpr (NG == 1 && THREADS <= 256) {
    if (nh == 2) return (const void*)&k_iterate_multi<MODE, 2, THREADS, SHARED>;
    if (nh == 4) return (const void*)&k_iterate_multi<MODE, 4, THREADS, SHARED>;
  }
  return (const void*)&k_iterate_multi<MODE, 1, THREADS, SHARED, NG>;
}

const void* multi_kernel(const ndt2d_params& p, bool wide, bool shared, bool split, int nh) {
  return with_mode(p, [&](auto M, auto NG) {
    if (wide)
      return shared ? multi_kernel_of<M, NG, kIterThreadsWide, true>(split, nh) : multi_kernel_of<M, NG, kIterThreadsWide, false>(split, nh);
    return shared ? multi_kernel_of<M, NG, kIterThreads, true>(split, nh) : multi_kernel_of<M, NG, kIterThreads, false>(split, nh);
  });
}

// m alignments against the cached grid in one launch chain: of one scan from m initial poses (shared), or
// of m scans (each with its initial pose).  sxs / sys / ns have one entry when shared, m otherwise.
int32_t multi_align(ndt2d_handle* h, const float* const* sxs, const float* const* sys, const size_t* ns, bool shared,
                    const double* init_poses, int32_t m, ndt2d_result* results) {
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  TraceRange range(shared ? "ndt2d_align_multi_start" : "ndt2d_align_multi_scan");
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (h->n_valid < 1) {
    for (int32_t k = 0; k < m; ++k) state_to(no_cell_state<IterState>(&init_poses[3 * k]), &results[k]);
    return NDT_OK;
  }
  HIP_TRY(ensure_multi_chain(&h->h_state_multi, kMaxStarts, &h->d_dyn_multi, h->stream));
  size_t n_max = 0;
  for (int32_t k = 0; k < (shared ? 1 : m); ++k) n_max = ns[k] > n_max ? ns[k] : n_max;
  const bool wide = h->use_wide && n_max >= h->wide_threshold;
  const int fixed = h->prm.fixed_iterations;
  const int K = fixed > 0 ? fixed : h->prm.max_iterations;
  const bool converged_mode = fixed == 0;
  // grid = (256 workgroups) x (subsets of nh starts): up to six workgroups per CU carry one start
  // each, more starts double up inside the workgroups; a 1024-thread workgroup fills a CU alone
  const bool split = m >= h->split_from;
  // fused chain: six one-start workgroups fit a CU (78 VGPRs), more starts double up inside the workgroups;
  // split chain: one start per evaluation workgroup (measured best: 31.8 us per step at 64 starts, 33.0 with four)
  const bool four = h->prm.overlap_grids == 4;     // Biber's four overlapping grids: every point scores against all four (NG = 4)
  const int nh = (split || wide || m <= 6 || four) ? 1 : (m <= 12 ? 2 : 4);
  const int subsets = (m + nh - 1) / nh;
  // From kSplitFrom starts on the chain alternates two kernels per iteration (one workgroup per start solves,
  // then everybody evaluates): the 256-fold redundant prologues of the fused kernel cost more than the
  // second kernel boundary there.
  const void* func = multi_kernel(h->prm, wide, shared, split, nh);
  next_seq(&h->flight.call_seq, h->h_flag);
  StartPoses sp{};
  StartScans sc{};
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 3; ++j) sp.p[k][j] = init_poses[3 * k + j];
    sc.sx[k] = sxs[shared ? 0 : k]; sc.sy[k] = sys[shared ? 0 : k]; sc.n[k] = (int)ns[shared ? 0 : k];
  }
  // AlignCall.n doubles as the "armed" word of the chain: the scan size when shared, any non-zero value otherwise
  hipLaunchKernelGGL(k_begin_multi, dim3(1), dim3(64), 0, h->stream, h->d_call, h->d_dyn_multi, sxs[0], sys[0], (int)n_max, sp, sc,
                     (int)m, fixed, converged_mode ? h->h_state_multi : (IterState*)nullptr,
                     converged_mode ? h->h_flag : (int*)nullptr, h->flight.call_seq);
  HIP_TRY(hipGetLastError());
  const int launches = converged_mode ? h->check_every + (h->check_every & 1) : K + 1;
  hipGraphExec_t exec = nullptr;
  const int key = 0x10000 | (shared ? 0 : 0x20000) | (split ? 0x40000 : 0) | (nh << 5) | (subsets << 8) | h->prm.hessian_mode | (wide ? 16 : 0);
  if (!split)
    HIP_TRY(h->graphs.get(func, dim3(kMaxBlocks, subsets), dim3(wide ? kIterThreadsWide : kIterThreads), (void*)h->d_static,
                          (void*)h->d_call, (void*)h->d_dyn_multi, launches, key, h->stream, &exec));
  else {
    // launch shapes in powers of two (slots >= m are born finished: their workgroups return at once): a caller whose m
    // varies from call to call replays one of three cached graphs (16, 32, 64 starts) instead of instantiating new ones
    int mg = 1;
    while (mg < m) mg <<= 1;
    HIP_TRY(h->graphs.get2((const void*)&k_multi_solve, dim3(mg), dim3(kBlock), func, dim3(kMaxBlocks, mg),
                           dim3(wide ? kIterThreadsWide : kIterThreads), (void*)h->d_static, (void*)h->d_call,
                           (void*)h->d_dyn_multi, launches, (key & ~(0xff << 8)) | (mg << 8) | (mg << 20), h->stream, &exec));
  }
  bool seen = true;
  HIP_TRY(run_multi_chain(exec, h->stream, converged_mode ? h->h_flag : nullptr, launches, K + 1, h->flight.call_seq, h->h_state_multi,
                          h->d_dyn_multi->state[K & 1], kMaxStarts * sizeof(IterState), &seen));
  if (!seen) { set_error("the multi-start loop did not report its end"); return NDT_ERR_HIP; }
  for (int k = 0; k < m; ++k) state_to(h->h_state_multi[k], &results[k]);
  return NDT_OK;
}

}  // namespace

extern "C" int32_t ndt2d_align_multi_start_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                               const double* init_poses, int32_t m, ndt2d_result* results) {
  if (!h || !d_sx || !d_sy || !init_poses || !results || m < 1 || m > kMaxStarts) return NDT_ERR_INVALID_ARG;
  if (n == 0 || n > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  return multi_align(h, &d_sx, &d_sy, &n, /*shared=*/true, init_poses, m, results);
}

extern "C" int32_t ndt2d_align_multi_scan_dev(ndt2d_handle* h, const float* const* d_sx, const float* const* d_sy,
                                              const size_t* n, const double* init_poses, int32_t m, ndt2d_result* results) {
  if (!h || !d_sx || !d_sy || !n || !init_poses || !results || m < 1 || m > kMaxStarts) return NDT_ERR_INVALID_ARG;
  for (int32_t k = 0; k < m; ++k)
    if (!d_sx[k] || !d_sy[k] || n[k] == 0 || n[k] > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  return multi_align(h, d_sx, d_sy, n, /*shared=*/false, init_poses, m, results);
}

#include "ndt_batch_host.hpp"
#include "ndt2d_batch_api.hpp"
#include "ndt2d_multi_api.hpp"
#include "ndt3d_api.hpp"
#include "ndt3d_batch_api.hpp"
#include "ndt3d_multi_api.hpp"
#include "ndt_map_io.hpp"
#include "ndt_coarsen.hpp"
#include "ndt_merge.hpp"
#include "ndt_point_fit.hpp"
#include "ndt_map_host.hpp"
#include "ndt2d_search.hpp"
#include "ndt3d_search.hpp"
#include "ndt_score_poses.hpp"
#include "ndt_score_particles.hpp"
#include "ndt2d_d2d_api.hpp"
#include "ndt2d_d2d_search.hpp"
#include "ndt3d_d2d_api.hpp"
#include "ndt3d_d2d_search.hpp"
#include "ndt_score_map_poses.hpp"
#include "ndt_deskew.hpp"
#include "ndt_voxel_filter.hpp"

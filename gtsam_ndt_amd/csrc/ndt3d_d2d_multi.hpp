// Up to kMaxStarts3 3D map-to-map alignments against ONE target in one launch chain (ndt3d_align_map_multi), the SE(3)
// twin of ndt2d_d2d_multi.hpp: each start has its own source component list and initial pose; the same list m times is
// a multi-start.
//
// A 3D map-to-map iteration is one k_iterate_d2d3 launch of about a dozen workgroups (a submap has a few thousand voxel
// Gaussians), bound by the launch boundary and the float64 6x6 solve of its prologue: most of the chip idles through
// it.  Here one launch pair carries the iteration of every start - the split chain of ndt3d_multi.hpp with another
// evaluation kernel:
//   k_begin_d2d_multi3_maps, k_begin_d2d_multi3   per-call part of the context (the twins of k_begin_multi3_scans and
//                                                 k_begin_multi3; two launches: each argument block stays below 4 KB)
//   k_multi_solve3<0>    unchanged, in BOTH Hessian modes: k_iterate_d2d3 carries the same 29 sums and the Gauss-Newton
//                        form of the prologue in both (32 rows, store_state3<0>, no newton_rot_block3)
//   k_multi_body_d2d3    workgroup (b, h) does for start h what workgroup b of k_iterate_d2d3 does in its body and
//                        epilogue, by calling the same function: evaluate_components3 (ndt3d_d2d.hpp)
//
// Contract: start h's result is what ndt3d_align_map returns for (target, sources[h], init_poses[h]), bit for bit: the
// same component -> thread assignment (blocks[h] workgroups, the single call's grid, whatever the launch's width) handed
// to one evaluate_components3 - per-thread accumulation order and reduction trees are its own - and the same update
// (k_multi_solve3<0>); a finished start is frozen.
#pragma once
#include "ndt3d_d2d.hpp"
#include "ndt3d_multi.hpp"

namespace ndt {

struct StartMaps3 {                // 1 KB of kernel arguments
  const float4* comp[kMaxStarts3];
  int n[kMaxStarts3];              // 0: the start takes no part (its source has no component): born finished
  int blocks[kMaxStarts3];         // min(ceil(n / kBlock), kMaxBlocks)
};

// k_begin_d2d_multi3_maps clears the unused columns with one thread per column, and k_multi_solve3<0> folds kRowsMap3 rows
static_assert(kMaxBlocks <= kBlock && Acc3<0>::kRows == kRowsMap3, "the map-to-map chain folds k_multi_solve3<0>'s rows");

// One workgroup per slot: the slot's list, and the clearing of its partial columns.  k_multi_solve3<0> folds all
// kMaxBlocks columns of a start's kRowsMap3 rows; k_multi_body3 of a point-to-map chain on the handle leaves all of them
// dirty, and so does an earlier call of this chain with a wider start in the slot: columns blocks[h] .. kMaxBlocks - 1
// are cleared here, in both halves (adding a float64 zero is exact).
__global__ __launch_bounds__(kBlock) void k_begin_d2d_multi3_maps(AlignDynMulti3* __restrict__ dyn, StartMaps3 maps, int m) {
  const int h = blockIdx.x, tid = threadIdx.x;
  if (h >= kMaxStarts3) return;
  const int n = h < m ? maps.n[h] : 0;
  const int blocks = n > 0 ? maps.blocks[h] : 0;
  if (n > 0 && tid >= blocks && tid < kMaxBlocks) {
#pragma unroll
    for (int j = 0; j < kRowsMap3; ++j) { dyn->partials[0][h][j][tid] = 0.f; dyn->partials[1][h][j][tid] = 0.f; }
  }
  if (tid != 0) return;
  dyn->map[h].comp = n > 0 ? maps.comp[h] : nullptr;
  dyn->map[h].n = n;
  dyn->map[h].blocks = blocks;
}

// Behind k_begin_d2d_multi3_maps on the stream (it reads the counts that launch stored).  Slots >= m and starts without
// a component are born finished and never evaluated; starts_done begins at the number of the latter, so that the
// chain's end (starts_done == m) counts them.
__global__ void k_begin_d2d_multi3(AlignCall3* __restrict__ call, AlignDynMulti3* __restrict__ dyn, const float4* cov,
                                   StartPoses3 poses, int m, int fixed_iterations, IterState3* host_state, int* host_flag,
                                   int seq) {
  const int h = threadIdx.x;
  if (blockIdx.x != 0 || h >= kMaxStarts3) return;
  const bool live = dyn->map[h].n > 0;
  dyn->body[0][h].done = dyn->body[1][h].done = live ? 0 : 1;
  if (h == 0) {
    int born = 0;
    for (int k = 0; k < m; ++k) born += dyn->map[k].n > 0 ? 0 : 1;
    call->seq = seq;
    call->pad = m;
    call->sx = nullptr; call->sy = nullptr; call->sz = nullptr;
    call->n = 1;                                  // the "armed" word of the chain: 0 once the call is over
    call->fixed_iterations = fixed_iterations;
    call->host_state = host_state;
    call->host_flag = host_flag;
    dyn->launch[0] = 0; dyn->launch[1] = 0;
    dyn->starts_done = born;
    dyn->map_cov = cov;
  }
  IterState3 s = {};
  if (live) {
#pragma unroll
    for (int j = 0; j < 3; ++j) s.pose[j] = poses.p[h][j];
#pragma unroll
    for (int j = 3; j < 6; ++j) s.pose[j] = wrap_angle(poses.p[h][j]);
  } else {
    s.done = 1;
  }
  dyn->state[1][h] = s;                           // launch 0 has parity 0 and reads slot 1
  dyn->state[0][h] = IterState3{};
  dyn->ls[0][h] = LineSearch3{};
  dyn->ls[1][h] = LineSearch3{};
}

// Grid (>= max_h blocks[h], >= m), kBlock threads.  Reads body[parity][h] (k_multi_solve3's: the float64 pose), writes
// partials[parity][h][*][b]; workgroups past blocks[h] and those of finished or unused slots return without writing.
template <int MODE, int NB>
__global__ __launch_bounds__(kBlock) void k_multi_body_d2d3(const AlignStatic3* __restrict__ st, const AlignCall3* __restrict__ call,
                                                            AlignDynMulti3* __restrict__ dyn, int parity) {
  constexpr int NA = kNumAccMap3;
  __shared__ float s_wave[kBlock / 64][kRowsMap3];
  __shared__ float s_t[kBlock / 64][NA * kSum3RowStride];
  (void)call;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = blockIdx.x, h = blockIdx.y;

  // ---- batch 1 of loads: this start's pose, list and share of the launch (uniform), the static context
  const AlignDynMulti3::Body* bp = &dyn->body[parity][h];
  const int done = bp->done;
  double pose[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) pose[j] = bp->pose[j];
  const float4* __restrict__ comp = dyn->map[h].comp;
  const int n = dyn->map[h].n, blocks = dyn->map[h].blocks;
  const float4* __restrict__ cov = dyn->map_cov;
  const SolveParams prm = st->prm;
  const Grid3Dev G = st->grid;
  if (done || b >= blocks) return;       // uniform; a finished start's list may already be gone: nothing of it is loaded

  const int i = b * kBlock + tid;
  float4 ca = make_float4(0.f, 0.f, 0.f, 0.f), cb = ca, cc = ca;
  if (i < n) { ca = comp[3 * (size_t)i]; cb = comp[3 * (size_t)i + 1]; cc = comp[3 * (size_t)i + 2]; }

  // ---- body and epilogue: the function k_iterate_d2d3 calls
  MapPose3 T;
  make_map_pose3(pose, T);
  evaluate_components3<MODE, NB>(G, prm, T, comp, cov, n, i, blocks * kBlock, ca, cb, cc, s_wave, s_t[wave],
                             &dyn->partials[parity][h][0][b]);
}

}  // namespace ndt

// Up to kMaxStarts map-to-map alignments against ONE target in one launch chain (ndt2d_align_map_multi): each start has
// its own source component list and initial pose; the same list m times is a multi-start.
//
// A map-to-map iteration is one k_iterate_d2d launch of a few workgroups (a submap has a few thousand components), bound
// by the launch boundary and the prologue: most of the chip idles through it.  Here one launch pair carries the
// iteration of every start - the split chain of ndt2d_multi_start.hpp with another evaluation kernel:
//   k_begin_d2d_multi   per-call part of the context (the twin of k_begin_multi)
//   k_multi_solve       unchanged: one workgroup per start folds that start's partial rows and updates its state
//   k_multi_body_d2d    workgroup (b, h) does for start h what workgroup b of k_iterate_d2d does in its body and
//                       epilogue: the body is the same function, evaluate_components (ndt2d_d2d.hpp)
//
// Contract: start h's result is what ndt2d_align_map returns for (target, sources[h], init_poses[h]), bit for bit: the
// same component -> thread assignment (blocks[h] workgroups, the single call's grid, whatever the launch's width) handed
// to one evaluate_components - the per-thread accumulation order is its own -, the same reduction trees
// (wave_reduce11_lds, then the four waves in fixed order), the same update (k_multi_solve); a finished start is frozen.
#pragma once
#include "ndt2d_d2d.hpp"
#include "ndt2d_multi_start.hpp"

namespace ndt {

struct StartMaps {
  const float4* comp[kMaxStarts];
  int n[kMaxStarts];            // 0: the start takes no part (its source has no component): born finished
  int blocks[kMaxStarts];       // min(ceil(n / kBlock), kMaxBlocks)
};

// One workgroup per slot.  Slots >= m and starts without a component are born finished and never evaluated; starts_done
// begins at the number of the latter, so that the chain's end (starts_done == m) counts them.  k_multi_solve folds all
// kMaxBlocks rows of a start's partial table and the point-to-map chains of the handle leave them dirty: rows
// blocks[h] .. kMaxBlocks - 1 are cleared here, in both halves (adding a float64 zero is exact).
__global__ __launch_bounds__(kBlock) void k_begin_d2d_multi(AlignCall* __restrict__ call, AlignDynMulti* __restrict__ dyn,
                                                             const float4* cov, StartPoses poses, StartMaps maps, int m,
                                                             int fixed_iterations, IterState* host_state, int* host_flag, int seq) {
  const int h = blockIdx.x, tid = threadIdx.x;
  if (h >= kMaxStarts) return;
  const int n = h < m ? maps.n[h] : 0;
  const int blocks = n > 0 ? maps.blocks[h] : 0;
  if (n > 0 && tid >= blocks && tid < kMaxBlocks) {
#pragma unroll
    for (int j = 0; j < kNumAcc; ++j) { dyn->partials[0][h][j][tid] = 0.f; dyn->partials[1][h][j][tid] = 0.f; }
  }
  if (tid != 0) return;
  dyn->map[h].comp = maps.comp[h];
  dyn->map[h].n = n;
  dyn->map[h].blocks = blocks;
  dyn->posef[0][h].done = dyn->posef[1][h].done = n > 0 ? 0 : 1;
  if (h == 0) {
    int born = 0;
    for (int k = 0; k < m; ++k) born += maps.n[k] > 0 ? 0 : 1;
    call->seq = seq;
    call->pad = m;
    call->sx = nullptr;
    call->sy = nullptr;
    call->n = 1;                  // the "armed" word of the chain (multi_announce)
    call->fixed_iterations = fixed_iterations;
    call->host_state = host_state;
    call->host_flag = host_flag;
    dyn->launch[0] = 0; dyn->launch[1] = 0;
    dyn->subsets_done = 0;
    dyn->starts_done = born;
    dyn->map_cov = cov;
  }
  IterState s = {};
  if (n > 0) {
    s.pose[0] = poses.p[h][0]; s.pose[1] = poses.p[h][1]; s.pose[2] = wrap_angle(poses.p[h][2]);
  } else {
    s.done = 1;
  }
  dyn->state[1][h] = s;         // launch 0 has parity 0 and reads slot 1
  dyn->state[0][h] = IterState{};
  dyn->ls[0][h] = LineSearch{};
  dyn->ls[1][h] = LineSearch{};
}

// Grid (>= max_h blocks[h], mg), kBlock threads.  Reads posef[parity][h] (k_multi_solve's: the four floats k_iterate_d2d
// derives from its pose), writes partials[parity][h][*][b]; workgroups past blocks[h] and those of finished or unused
// slots return without writing.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_multi_body_d2d(const AlignStatic* __restrict__ st, const AlignCall* __restrict__ call,
                                                           AlignDynMulti* __restrict__ dyn, int parity) {
  __shared__ float s_wave[kBlock / 64][kNumAcc];
  __shared__ float s_t[kBlock / 64][(kNumAcc - 1) * kSumRowStride];
  (void)call;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, h = blockIdx.y;

  // ---- batch 1 of loads: this start's pose, list and share of the launch (uniform), the static context
  const AlignDynMulti::BodyPose* bp = &dyn->posef[parity][h];
  const float pcs = bp->cs, psn = bp->sn, ptx = bp->tx, pty = bp->ty;
  const int done = bp->done;
  const float4* __restrict__ comp = dyn->map[h].comp;
  const int n = dyn->map[h].n, blocks = dyn->map[h].blocks;
  const float4* __restrict__ cov = dyn->map_cov;
  const SolveParams prm = st->prm;
  const GridDev G = st->grid;
  if (done || b >= blocks) return;       // uniform; a finished start's list may already be gone: nothing of it is loaded

  const int stride = blocks * kBlock;
  int i = b * kBlock + tid;
  float4 ca = make_float4(0.f, 0.f, 0.f, 0.f), cb = ca;
  if (i < n) { ca = comp[2 * (size_t)i]; cb = comp[2 * (size_t)i + 1]; }

  // ---- body: the function k_iterate_d2d calls
  const PoseF P = make_pose(pcs, psn, ptx, pty, G.ox, G.oy, G.inv_c, G.W, G.H, prm.d1, prm.d2);
  float acc[kNumAcc];
  evaluate_components<MODE>(P, prm.d2, comp, cov, n, i, stride, ca, cb, acc);

  // ---- epilogue: wave tree -> LDS -> one partial column entry per sum (each chain kernel's own text: DESIGN 5.1)
  {
    const float r = wave_reduce11_lds(acc, s_t[wave], lane);
    if ((lane & 3) == 0 && lane < 4 * (kNumAcc - 1)) s_wave[wave][lane >> 2] = r;
  }
  __syncthreads();
  if (tid < kNumAcc) {
    float r = 0.f;
    if (tid < kNumAcc - 1) {
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) r += s_wave[w][tid];     // fixed order
    }
    dyn->partials[parity][h][tid][b] = r;
  }
}

}  // namespace ndt

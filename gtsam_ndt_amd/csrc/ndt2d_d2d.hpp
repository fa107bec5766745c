// Map-to-map alignment (distribution-to-distribution NDT; Stoyanov, Magnusson, Andreasson, Lilienthal, IJRR 2012):
// the source is the list of its own cell Gaussians, each scored against the target Gaussian of the cell its
// transformed mean falls in (docs/ALGORITHM.md section 2.13).  Everything comes from the exact per-cell sums both
// handles keep (CellAcc), so two submaps align without any of the points they were built from.
//
//   k_cov_records     target side: a second record array, the regularised covariance instead of its inverse
//   k_comp_offsets    source side: exclusive scan of the per-workgroup counts of valid cells ...
//   k_components      ... and the compaction of the valid cells into a dense list, in cell-key order
//   k_begin_d2d       per-call part of the context (the twin of k_begin)
//   k_iterate_d2d     one launch per Gauss-Newton iteration: the chain's shared prologue pieces and k_iterate's epilogue
//                     around a new body
#pragma once
#include "ndt2d_kernels.hpp"

namespace ndt {

// ---------------------------------------------------------------------------- covariance records
// The layout of GridDev::rec ({mx, my, Sxx, Sxy | Sxy, Syy, n, 0}; zero for an invalid cell), so image_point /
// image_key and the clamped lookup serve it as they are.  Sigma = l2c I + (l1 - l2c) e e^T: the matrix whose
// inverse finalise_sums stores, from the same eigen step (cell_eigen), float64 until the store.
__device__ __forceinline__ bool cov_record(int n, long long sx, long long sy, long long sxx, long long sxy, long long syy,
                                           double cx, double cy, double fix_scale, int min_points, double eig_ratio,
                                           float4& ra, float4& rb) {
  ra = make_float4(0.f, 0.f, 0.f, 0.f);
  rb = make_float4(0.f, 0.f, 0.f, 0.f);
  CellEig e;
  if (!cell_eigen(n, sx, sy, sxx, sxy, syy, cx, cy, fix_scale, min_points, eig_ratio, e)) return false;
  const double d = e.l1 - e.l2c;
  const float b32 = (float)(d * e.ex * e.ey);
  ra = make_float4((float)e.mx, (float)e.my, (float)fma(d * e.ex, e.ex, e.l2c), b32);
  rb = make_float4(b32, (float)fma(d * e.ey, e.ey, e.l2c), (float)n, 0.f);
  return true;
}

// One thread per cell of grid 0 (k_finalise's validity rule, its overflow rule included); block_valid[b] = the
// valid cells of workgroup b's kBlock cells, which is what the compaction below scans.
__global__ __launch_bounds__(kBlock) void k_cov_records(GridDev g, int min_points, double eig_ratio,
                                                         float4* __restrict__ cov, unsigned int* __restrict__ block_valid) {
  __shared__ unsigned int s_n[kBlock / 64];
  const unsigned int ncell = (unsigned int)g.W * (unsigned int)g.H;      // <= 2^27
  const unsigned int k = blockIdx.x * kBlock + threadIdx.x;
  bool ok = false;
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (k < ncell) {
    const CellAcc c = g.acc[k];
    if (c.n <= kMaxCellCount && (int)c.n >= min_points) {
      const int ix = (int)(k % (unsigned int)g.W), iy = (int)(k / (unsigned int)g.W);
      ok = cov_record((int)c.n, c.sx, c.sy, c.sxx, c.sxy, c.syy, cell_centre(g.gx[0], ix, g.cell),
                      cell_centre(g.gy[0], iy, g.cell), g.fix_scale, min_points, eig_ratio, ra, rb);
    }
    cov[2 * (size_t)k] = ra;
    cov[2 * (size_t)k + 1] = rb;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = (unsigned int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_valid[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

// Exclusive scan of nb counts by one workgroup: thread t owns a contiguous run of counts, the 1024 run totals are
// scanned in LDS, the total goes to *n_out.  Integer sums in a fixed assignment: no atomics, nothing depends on order.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_comp_offsets(const unsigned int* __restrict__ counts, unsigned int nb,
                                                                unsigned int* __restrict__ offsets,
                                                                unsigned int* __restrict__ n_out) {
  __shared__ unsigned int s_tot[kScanThreads];
  const unsigned int per = (nb + kScanThreads - 1) / kScanThreads;
  const unsigned int lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
  unsigned int sum = 0;
  for (unsigned int i = lo; i < hi; ++i) sum += counts[i];
  s_tot[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {                       // Hillis-Steele, inclusive
    const unsigned int v = threadIdx.x >= (unsigned)d ? s_tot[threadIdx.x - d] : 0u;
    __syncthreads();
    s_tot[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned int run = s_tot[threadIdx.x] - sum;
  for (unsigned int i = lo; i < hi; ++i) { offsets[i] = run; run += counts[i]; }
  if (threadIdx.x == kScanThreads - 1) *n_out = s_tot[kScanThreads - 1];
}

// The valid cells of the covariance records, dense and in cell-key order.  A component is 32 bytes, the record's
// own layout with the cell key where the record keeps its count: comp[2i] = (mx, my, Sxx, Sxy), comp[2i+1] =
// (Sxy, Syy, key bits, 0) - the two 16-byte loads per lane k_iterate_d2d issues, two components per 64-byte line.
__global__ __launch_bounds__(kBlock) void k_components(const float4* __restrict__ cov, unsigned int ncell,
                                                        const unsigned int* __restrict__ offsets,
                                                        float4* __restrict__ comp, unsigned int capacity) {
  __shared__ unsigned int s_n[kBlock / 64];
  const unsigned int k = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (k < ncell) { ra = cov[2 * (size_t)k]; rb = cov[2 * (size_t)k + 1]; }
  const bool ok = rb.z > 0.f;
  const unsigned long long m = __ballot(ok);
  if (lane == 0) s_n[wave] = (unsigned int)__popcll(m);
  __syncthreads();
  unsigned int at = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) at += s_n[w];
  at += (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
  if (ok && at < capacity) {
    comp[2 * (size_t)at] = ra;
    comp[2 * (size_t)at + 1] = make_float4(rb.x, rb.y, __int_as_float((int)k), 0.f);
  }
}

// ---------------------------------------------------------------------------- the iteration
// Per-call arguments of a map-to-map alignment (the twin of AlignCall), written by k_begin_d2d.
struct MapCall {
  const float4* comp;        // the source handle's component list
  const float4* cov;         // the target handle's covariance records
  int n;                     // components; the finishing launch of a converged-mode loop leaves 0 behind
  int fixed_iterations;
  IterState* host_state;     // converged mode: as AlignCall
  int* host_flag;
  int seq;
  int blocks;                // workgroups per launch (rows of the partial table in use)
};

// blocks <= kMaxBlocks workgroups write a partial row each; the prologue folds all kMaxBlocks rows in its fixed
// order, so the rows past `blocks` are cleared here, in both halves: adding a float64 zero is exact.
__global__ __launch_bounds__(kBlock) void k_begin_d2d(MapCall* __restrict__ call, AlignDyn* __restrict__ dyn, const float4* comp,
                                                       const float4* cov, int n, int blocks, double p0, double p1, double p2,
                                                       int fixed_iterations, IterState* host_state, int* host_flag, int seq) {
  const int tid = threadIdx.x;
  if (tid >= blocks && tid < kMaxBlocks) {
#pragma unroll
    for (int j = 0; j < kNumAcc; ++j) { dyn->rows[0][j][tid] = 0.f; dyn->rows[1][j][tid] = 0.f; }
  }
  if (tid != 0) return;
  call->comp = comp;
  call->cov = cov;
  call->n = n;
  call->fixed_iterations = fixed_iterations;
  call->host_state = host_state;
  call->host_flag = host_flag;
  call->seq = seq;
  call->blocks = blocks;
  IterState s = {};
  s.pose[0] = p0; s.pose[1] = p1; s.pose[2] = wrap_angle(p2);
  dyn->state[1] = s;            // launch 0 has parity 0 and reads slot 1
  dyn->state[0] = IterState{};
  dyn->ls[0] = LineSearch{};
  dyn->ls[1] = LineSearch{};
}

// What the body needs of the pose besides PoseF: the double angle, for S = R Sigma R^T through the half trace and
// the half difference of Sigma (Sxx = hm + u, Syy = hm - u, u = hd cos2t - b sin2t, Sxy = hd sin2t + b cos2t).
struct RotF { float c2t, s2t; };

// One source component against the target record its image fell on: the 10 sums + hit count of ALGORITHM 2.13.
// Written in the order tests/d2d_ref.py states in float32 (mirror32), so that restatement bounds this code's error.
template <int MODE>
__device__ __forceinline__ void accumulate_component(const PoseF& P, const RotF& R, const PointRec& r, float sa, float sb,
                                                     float sc, Acc2D& acc) {
  const bool hit = r.B.z > 0.f;
  const float hm = 0.5f * (sa + sc), hd = 0.5f * (sa - sc);
  const float u = fmaf(hd, R.c2t, -sb * R.s2t);
  const float sxy = fmaf(hd, R.s2t, sb * R.c2t);
  const float axx = (hm + u) + r.A.z, axy = sxy + r.A.w, ayy = (hm - u) + r.B.y;      // S + Sigma_j (S alone off the map: det > 0)
  const float rdet = __builtin_amdgcn_rcpf(fmaf(axx, ayy, -axy * axy));
  const float bxx = ayy * rdet, bxy = -axy * rdet, byy = axx * rdet;                   // B = (S + Sigma_j)^-1
  const float qx = r.px - r.A.x, qy = r.py - r.A.y;
  const float vx = fmaf(bxx, qx, bxy * qy), vy = fmaf(bxy, qx, byy * qy);
  const float m = fmaf(qx, vx, qy * vy);
  const float s = hit ? __builtin_amdgcn_exp2f(fmaf(P.nhd2, m, P.lg_d1)) : 0.f;
  const float jx = P.ty - r.py, jy = r.px - P.tx;                                       // K R mu
  const float zx = 2.f * fmaf(u, vy, -sxy * vx), zy = 2.f * fmaf(u, vx, sxy * vy);      // Z_theta v
  const float rx = jx - zx, ry = jy - zy;
  const float ct = fmaf(vx, jx, vy * jy) - 0.5f * fmaf(vx, zx, vy * zy);
  const float ux = fmaf(bxx, rx, bxy * ry), uy = fmaf(bxy, rx, byy * ry);               // B r_theta
  float hxx = bxx, hxy = bxy, hyy = byy, hxt = ux, hyt = uy, htt = fmaf(rx, ux, ry * uy);
  if (MODE == 1) {
    const float dvx = -P.d2 * vx, dvy = -P.d2 * vy, dct = -P.d2 * ct;
    hxx = fmaf(dvx, vx, hxx);
    hxy = fmaf(dvx, vy, hxy);
    hyy = fmaf(dvy, vy, hyy);
    hxt = fmaf(dct, vx, hxt);
    hyt = fmaf(dct, vy, hyt);
    // v' j_thth - 1/2 v' Z_thth v: j_thth = -R mu = t - p', Z_thth = -4 [[u, Sxy], [Sxy, -u]]
    htt = fmaf(dct, ct, htt) + fmaf(vx, P.tx - r.px, vy * (P.ty - r.py)) +
          2.f * fmaf(u, fmaf(vx, vx, -vy * vy), 2.f * sxy * vx * vy);
  }
  acc.h0 = fmaf(s, hxx, acc.h0); acc.h1 = fmaf(s, hxy, acc.h1); acc.h2 = fmaf(s, hyy, acc.h2);
  acc.h3 = fmaf(s, hxt, acc.h3); acc.h4 = fmaf(s, hyt, acc.h4); acc.h5 = fmaf(s, htt, acc.h5);
  acc.g0 = fmaf(s, vx, acc.g0);  acc.g1 = fmaf(s, vy, acc.g1);  acc.g2 = fmaf(s, ct, acc.g2);
  acc.s += s;
  acc.n_wave += (int)__popcll(__ballot(hit));
}

// Body of a map-to-map launch for one alignment, shared by k_iterate_d2d and the multi-start chain (k_multi_body_d2d):
// this workgroup's components (thread -> component assignment i, i + stride, ...; the first one already loaded into ca0,
// cb0) under the pose P, the thread's sums into acc[kNumAcc].  No __restrict__, the first component by const reference:
// the parameter shape that leaves both kernels the registers and instruction counts they had (Shared pieces).
template <int MODE>
__device__ __forceinline__ void evaluate_components(const PoseF& P, float d2, const float4* comp, const float4* cov, int n, int i,
                                                    int stride, const float4& ca0, const float4& cb0, float* acc) {
  float4 ca = ca0, cb = cb0;
  RotF R;
  R.c2t = P.cs * P.cs - P.sn * P.sn;
  R.s2t = 2.f * P.cs * P.sn;
  Acc2D A;
  acc_zero(A);
  while (i < n) {
    const int i2 = i + stride;
    float4 na = make_float4(0.f, 0.f, 0.f, 0.f), nb = na;
    if (i2 < n) { na = comp[2 * (size_t)i2]; nb = comp[2 * (size_t)i2 + 1]; }
    PointRec r;
    image_point(P, ca.x, ca.y, r);
    const int key = image_key(P, P.ox, P.oy, r, true);       // clamped onto the grid: every key is a cell of `cov`
    r.A = cov[2 * key];
    r.B = cov[2 * key + 1];
    accumulate_component<MODE>(P, R, r, ca.z, ca.w, cb.y, A);
    ca = na; cb = nb; i = i2;
  }
  acc_store(A, d2, acc);
  acc[11] = 0.f;
}

// Launch k (parity = k & 1) consumes state[parity^1] / partials[parity^1] of launch k-1 and produces state[parity] /
// partials[parity]: k_iterate's chain, state, flags and reduction (the shared pieces of ndt_chain.hpp and
// ndt2d_kernels.hpp), with call->blocks workgroups of kBlock threads
// (a component per lane; a few thousand components do not need a workgroup per CU).  Same two dependent memory
// round trips: previous state + partial rows + first component in one batch, then the record gather.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_iterate_d2d(const AlignStatic* __restrict__ st, const MapCall* __restrict__ call,
                                                        AlignDyn* __restrict__ dyn, int parity) {
  __shared__ double s_red[kNumAcc];
  __shared__ float s_wave[kBlock / 64][kNumAcc];
  __shared__ float s_t[kBlock / 64][(kNumAcc - 1) * kSumRowStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const IterState* prev = &dyn->state[parity ^ 1];
  IterState* cur = &dyn->state[parity];
  const bool writer = (blockIdx.x == 0) && (tid == 0);

  __builtin_amdgcn_sched_barrier(0);     // the four arguments stay one s_load batch above everything else
  // ---- batch 1 of loads: previous state (scalar), partial rows (vector), first component
  const double ps_pose0 = prev->pose[0], ps_pose1 = prev->pose[1], ps_pose2 = prev->pose[2];
  const int ps_iter = prev->iter, ps_done = prev->done, ps_have = prev->have_partials, ps_launch = prev->pad;
  const SolveParams prm = st->prm;
  const GridDev G = st->grid;
  const int n = call->n;
  const int fixed_iterations = call->fixed_iterations;
  const float4* __restrict__ comp = call->comp;
  const float4* __restrict__ cov = call->cov;
  IterState* const host_state = call->host_state;
  int* const host_flag = call->host_flag;
  float4 pv[3];
  {
    const float* part = &dyn->rows[parity ^ 1][0][0];     // this chain keeps the table as one row per sum
#pragma unroll
    for (int v = 0; v < 3; ++v)
      pv[v] = *reinterpret_cast<const float4*>(part + (wave * 3 + v) * kMaxBlocks + lane * 4);
  }
  const int stride = (int)gridDim.x * kBlock;
  int i = blockIdx.x * kBlock + tid;
  float4 ca = make_float4(0.f, 0.f, 0.f, 0.f), cb = ca;
  if (i < n) { ca = comp[2 * (size_t)i]; cb = comp[2 * (size_t)i + 1]; }

  if (ps_done) {                         // uniform: a finished alignment just carries its state
    if (writer) chain_carry_done(cur, prev, host_flag, call);     // nothing reads the component list any more
    return;
  }
  double pose[3] = {ps_pose0, ps_pose1, ps_pose2};
  int iter = ps_iter;
  if (ps_have) {
    // ---- prologue: fixed-order float64 fold of the kMaxBlocks partial columns (fold_rows12), then the solve
    double H[6], g[3], score = 0.0;
    int n_hit = 0, status = 0;
    fold_rows12(pv, reinterpret_cast<double*>(s_t[wave]), lane, &s_red[wave * 3]);
    __syncthreads();
    unpack_sums(s_red, H, g, score, n_hit);
    const bool done = gn_update(pose, H, g, n_hit, iter, status, prm, fixed_iterations, score, &dyn->ls[parity ^ 1],
                                &dyn->ls[parity], writer);
    if (writer) {
      auto store = [&](IterState* o) {
        pack_state(o, pose, H, g, score, n_hit, iter, status, done ? 1 : 0, ps_launch + 1);
      };
      store(cur);
      chain_announce(store, done, ps_launch + 1, host_state, host_flag, call);
    }
    if (done) return;                    // uniform
  } else if (writer) {
    copy_state(cur, prev, 1);
  }

  // ---- body: per-component terms at `pose` (evaluate_components)
  double sn_d, cs_d;
  sincos_wrapped(pose[2], &sn_d, &cs_d);
  const PoseF P = make_pose((float)cs_d, (float)sn_d, (float)pose[0], (float)pose[1], G.ox, G.oy, G.inv_c, G.W, G.H,
                            prm.d1, prm.d2);
  float acc[kNumAcc];
  evaluate_components<MODE>(P, prm.d2, comp, cov, n, i, stride, ca, cb, acc);

  // ---- epilogue: wave tree -> LDS -> one partial column entry per sum
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
    dyn->rows[parity][tid][blockIdx.x] = r;
  }
}

}  // namespace ndt

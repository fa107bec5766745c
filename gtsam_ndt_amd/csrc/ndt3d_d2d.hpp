// 3D map-to-map alignment (distribution-to-distribution NDT; docs/ALGORITHM.md section 2.14), the SE(3) twin of
// ndt2d_d2d.hpp: the source is the list of its own voxel Gaussians, each scored against the target Gaussian of the voxel
// its transformed mean falls in (and, with the target's map neighbourhood 7, against those of that voxel's six face
// neighbours: section 2.26).  Everything comes from the exact per-voxel sums both handles keep (CellAcc3).
//
//   k_cov_records3    target side: a second record array, the regularised covariance instead of its inverse
//   k_comp_offsets    (ndt2d_d2d.hpp, dimension-free) exclusive scan of the per-workgroup counts of valid voxels ...
//   k_components3     ... and the compaction of the valid voxels into a dense list, in voxel-key order
//   k_begin_d2d3      per-call part of the context (the twin of k_begin3)
//   k_iterate_d2d3    one launch per iteration: k_iterate3's prologue and epilogue around a new per-component body
//                     (<MODE, NB>: the Hessian form and the map neighbourhood, 1 or 7)
#pragma once
#include "ndt2d_d2d.hpp"
#include "ndt3d_kernels.hpp"

namespace ndt {

// ---------------------------------------------------------------------------- covariance records
// 48 bytes per voxel, three float4: cov[3k] = (mean_x, mean_y, mean_z, n; 0 = invalid), cov[3k+1] = Sigma (xx xy xz yy),
// cov[3k+2] = (yz zz 0 0); all zero for an invalid voxel.  Sigma = sum_k max(l_k, eig_ratio lmax) v_k v_k^T: the matrix
// whose inverse finalise_sums3 stores, from the same eigen step (cell_eigen3), float64 until the store.
__device__ __forceinline__ bool cov_record3(const CellAcc3& c, double cx, double cy, double cz, double fix_scale, int min_points,
                                            double eig_ratio, float4& ra, float4& rb, float4& rc) {
  return cell_eigen3(c, cx, cy, cz, fix_scale, min_points, eig_ratio,
                     [&](int n, double mx, double my, double mz, double axx, double ayy, double azz, double lim,
                         const double* v0, const double* v1, const double* v2) {
    const double l0 = fmax(axx, lim), l1 = fmax(ayy, lim), l2 = fmax(azz, lim);
    const double sxx = l0 * v0[0] * v0[0] + l1 * v1[0] * v1[0] + l2 * v2[0] * v2[0];
    const double sxy = l0 * v0[0] * v0[1] + l1 * v1[0] * v1[1] + l2 * v2[0] * v2[1];
    const double sxz = l0 * v0[0] * v0[2] + l1 * v1[0] * v1[2] + l2 * v2[0] * v2[2];
    const double syy = l0 * v0[1] * v0[1] + l1 * v1[1] * v1[1] + l2 * v2[1] * v2[1];
    const double syz = l0 * v0[1] * v0[2] + l1 * v1[1] * v1[2] + l2 * v2[1] * v2[2];
    const double szz = l0 * v0[2] * v0[2] + l1 * v1[2] * v1[2] + l2 * v2[2] * v2[2];
    ra = make_float4((float)mx, (float)my, (float)mz, (float)n);
    rb = make_float4((float)sxx, (float)sxy, (float)sxz, (float)syy);
    rc = make_float4((float)syz, (float)szz, 0.f, 0.f);
  });
}

// One thread per voxel (k_finalise3's validity rule, its overflow rule included); block_valid[b] = the valid voxels of
// workgroup b's kBlock voxels, which is what the compaction below scans.
__global__ __launch_bounds__(kBlock) void k_cov_records3(Grid3Dev g, int min_points, double eig_ratio, float4* __restrict__ cov,
                                                          unsigned int* __restrict__ block_valid) {
  __shared__ unsigned int s_n[kBlock / 64];
  const unsigned int ncell = (unsigned int)g.W * (unsigned int)g.H * (unsigned int)g.D;      // <= 2^27
  const unsigned int k = blockIdx.x * kBlock + threadIdx.x;
  bool ok = false;
  if (k < ncell) {
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
    const CellAcc3 c = g.acc[k];
    if (c.n <= kMaxCellCount && (int)c.n >= min_points) {
      const unsigned int w32 = (unsigned int)g.W, h32 = (unsigned int)g.H;
      const int ix = (int)(k % w32), iy = (int)((k / w32) % h32), iz = (int)(k / (w32 * h32));
      ok = cov_record3(c, cell_centre(g.ox, ix, g.cell), cell_centre(g.oy, iy, g.cell), cell_centre(g.oz, iz, g.cell),
                       g.fix_scale, min_points, eig_ratio, ra, rb, rc);
      if (!ok) { ra = make_float4(0.f, 0.f, 0.f, 0.f); rb = ra; rc = ra; }
    }
    cov[3 * (size_t)k] = ra;
    cov[3 * (size_t)k + 1] = rb;
    cov[3 * (size_t)k + 2] = rc;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = (unsigned int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_valid[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

// The valid voxels of the covariance records, dense and in voxel-key order.  A component is the record's own 48 bytes
// with the voxel key where the record keeps its count: comp[3i] = (mx, my, mz, key bits), comp[3i+1] = (xx xy xz yy),
// comp[3i+2] = (yz zz 0 0) - three 16-byte loads per lane in k_iterate_d2d3, four components per three 64-byte lines.
__global__ __launch_bounds__(kBlock) void k_components3(const float4* __restrict__ cov, unsigned int ncell,
                                                         const unsigned int* __restrict__ offsets, float4* __restrict__ comp,
                                                         unsigned int capacity) {
  __shared__ unsigned int s_n[kBlock / 64];
  const unsigned int k = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
  if (k < ncell) { ra = cov[3 * (size_t)k]; rb = cov[3 * (size_t)k + 1]; rc = cov[3 * (size_t)k + 2]; }
  const bool ok = ra.w > 0.f;
  const unsigned long long m = __ballot(ok);
  if (lane == 0) s_n[wave] = (unsigned int)__popcll(m);
  __syncthreads();
  unsigned int at = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) at += s_n[w];
  at += (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
  if (ok && at < capacity) {
    comp[3 * (size_t)at] = make_float4(ra.x, ra.y, ra.z, __int_as_float((int)k));
    comp[3 * (size_t)at + 1] = rb;
    comp[3 * (size_t)at + 2] = rc;
  }
}

// ---------------------------------------------------------------------------- the iteration
// Per-call arguments of a map-to-map alignment (the twin of AlignCall3), written by k_begin_d2d3.
struct MapCall3 {
  const float4* comp;        // the source handle's component list
  const float4* cov;         // the target handle's covariance records
  int n;                     // components; the finishing launch of a converged-mode loop leaves 0 behind
  int fixed_iterations;
  IterState3* host_state;    // converged mode: as AlignCall3
  int* host_flag;
  int seq;
  int blocks;                // workgroups per launch (columns of the partial table in use)
};

constexpr int kNumAccMap3 = 29;      // Htt(6) Htr(9) Hrr(6) g(6) score n_hit, in both Hessian modes
constexpr int kRowsMap3 = 32;        // partial rows the prologue folds (k_iterate3<0>'s 8 per wave)
// k_begin_d2d3 clears the unused columns from one workgroup of kBlock threads, and the fold reads a row as 64 lanes x float4
static_assert(kMaxBlocks <= kBlock && kMaxBlocks == 256, "k_begin_d2d3 and the fold of k_iterate_d2d3 assume 256 partial columns");
static_assert(kRowsMap3 <= kNumAcc3 && kNumAccMap3 <= kRowsMap3 && kRowsMap3 % 4 == 0, "AlignDyn3::partials holds the folded rows");

// blocks <= kMaxBlocks workgroups write a partial column each; the prologue folds all kMaxBlocks columns in its fixed
// order, so the columns past `blocks` are cleared here, in both halves: adding a float64 zero is exact.
__global__ __launch_bounds__(kBlock) void k_begin_d2d3(MapCall3* __restrict__ call, AlignDyn3* __restrict__ dyn, const float4* comp,
                                                        const float4* cov, int n, int blocks, double p0, double p1, double p2,
                                                        double p3, double p4, double p5, int fixed_iterations,
                                                        IterState3* host_state, int* host_flag, int seq) {
  const int tid = threadIdx.x;
  if (tid >= blocks && tid < kMaxBlocks) {
#pragma unroll
    for (int j = 0; j < kRowsMap3; ++j) { dyn->partials[0][j][tid] = 0.f; dyn->partials[1][j][tid] = 0.f; }
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
  IterState3 s = {};
  s.pose[0] = p0; s.pose[1] = p1; s.pose[2] = p2;
  s.pose[3] = wrap_angle(p3); s.pose[4] = wrap_angle(p4); s.pose[5] = wrap_angle(p5);
  dyn->state[1] = s;            // launch 0 has parity 0 and reads slot 1
  dyn->state[0] = IterState3{};
  dyn->ls[0] = LineSearch3{};
  dyn->ls[1] = LineSearch3{};
}

// What the body needs of the pose: R and t in float32 (rounded from float64, as make_rot3), and the axes of the map-frame
// form of the derivatives, dR/da_k = [a_k]x R: a_roll = R[:, 0] (read from R), a_pitch = (-sin yaw, cos yaw, 0),
// a_yaw = e_z.  d2R/da_k da_l = [a_l]x [a_k]x R for k <= l.
struct MapPose3 {
  float R[9];
  float tx, ty, tz;
  float bx, by;              // a_pitch
};
__device__ __forceinline__ void make_map_pose3(const double* pose, MapPose3& T) {
  // (its own text of ndt_pose.hpp's rot3_products, as make_rot3: through make_rt3 k_score_map_poses3, which reads R and t
  // from here, measured outside the run-to-run spread)
  double sa, ca, sb, cb, sg, cg;
  sincos_wrapped(pose[3], &sa, &ca);
  sincos_wrapped(pose[4], &sb, &cb);
  sincos_wrapped(pose[5], &sg, &cg);
  T.R[0] = (float)(cg * cb); T.R[1] = (float)(cg * sb * sa - sg * ca); T.R[2] = (float)(cg * sb * ca + sg * sa);
  T.R[3] = (float)(sg * cb); T.R[4] = (float)(sg * sb * sa + cg * ca); T.R[5] = (float)(sg * sb * ca - cg * sa);
  T.R[6] = (float)(-sb);     T.R[7] = (float)(cb * sa);                T.R[8] = (float)(cb * ca);
  T.tx = (float)pose[0]; T.ty = (float)pose[1]; T.tz = (float)pose[2];
  T.bx = (float)(-sg); T.by = (float)cg;
}

__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
  return fmaf(a0, b0, fmaf(a1, b1, a2 * b2));
}
__device__ __forceinline__ float dot3(const V3& a, const V3& b) { return dot3(a.x, b.x, a.y, b.y, a.z, b.z); }
// S x for a symmetric S = (xx xy xz yy yz zz)
__device__ __forceinline__ V3 symv(const float* S, const V3& x) {
  return V3{dot3(S[0], x.x, S[1], x.y, S[2], x.z), dot3(S[1], x.x, S[3], x.y, S[4], x.z), dot3(S[2], x.x, S[4], x.y, S[5], x.z)};
}
// S = (R Sg) R' for a symmetric Sg: a source covariance under the pose's rotation (the body, and the staging of the search)
__device__ __forceinline__ void rotate_cov3(const float* R, const float* Sg, float* S) {
  float Tm[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Tm[3 * r] = dot3(R[3 * r], Sg[0], R[3 * r + 1], Sg[1], R[3 * r + 2], Sg[2]);
    Tm[3 * r + 1] = dot3(R[3 * r], Sg[1], R[3 * r + 1], Sg[3], R[3 * r + 2], Sg[4]);
    Tm[3 * r + 2] = dot3(R[3 * r], Sg[2], R[3 * r + 1], Sg[4], R[3 * r + 2], Sg[5]);
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) S[q++] = dot3(Tm[3 * i], R[3 * j], Tm[3 * i + 1], R[3 * j + 1], Tm[3 * i + 2], R[3 * j + 2]);
}
// m = q' B q with B = (S + Sigma_j)^-1 by cofactors (the sum's six entries xx xy xz yy yz zz), and v = B q
__device__ __forceinline__ float mahalanobis_sum3(float axx, float axy, float axz, float ayy, float ayz, float azz, const V3& q,
                                                  float* B, V3& v) {
  const float c00 = fmaf(ayy, azz, -ayz * ayz), c01 = fmaf(axz, ayz, -axy * azz), c02 = fmaf(axy, ayz, -axz * ayy);
  const float c11 = fmaf(axx, azz, -axz * axz), c12 = fmaf(axy, axz, -axx * ayz), c22 = fmaf(axx, ayy, -axy * axy);
  const float rdet = 1.0f / dot3(axx, c00, axy, c01, axz, c02);
  B[0] = c00 * rdet; B[1] = c01 * rdet; B[2] = c02 * rdet; B[3] = c11 * rdet; B[4] = c12 * rdet; B[5] = c22 * rdet;
  v = symv(B, q);
  return dot3(q, v);
}
// a_k x b for the three axes
template <int K>
__device__ __forceinline__ V3 axis_cross(const MapPose3& T, const V3& b) {
  if (K == 0) {
    const float ax = T.R[0], ay = T.R[3], az = T.R[6];
    return V3{fmaf(ay, b.z, -az * b.y), fmaf(az, b.x, -ax * b.z), fmaf(ax, b.y, -ay * b.x)};
  }
  if (K == 1) return V3{T.by * b.z, -(T.bx * b.z), fmaf(T.bx, b.y, -T.by * b.x)};
  return V3{-b.y, b.x, 0.f};
}

// The terms of one rotation parameter (ALGORITHM 2.14): j = a x (R mu), p = a x v, e = a x (S v), f = S p,
// Z v = e - f, r = j - Z v, c = v'(j - Z v / 2), U = B r.
struct RotTerms3 { V3 j, p, e, f, r, U; float c; };
template <int K>
__device__ __forceinline__ void rot_terms3(const MapPose3& T, const float* S, const float* B, const V3& pr, const V3& v,
                                           const V3& Sv, RotTerms3& o) {
  o.j = axis_cross<K>(T, pr);
  o.p = axis_cross<K>(T, v);
  o.e = axis_cross<K>(T, Sv);
  o.f = symv(S, o.p);
  const V3 z{o.e.x - o.f.x, o.e.y - o.f.y, o.e.z - o.f.z};
  o.r = V3{o.j.x - z.x, o.j.y - z.y, o.j.z - z.z};
  o.c = dot3(v, o.j) - 0.5f * dot3(v, z);
  o.U = symv(B, o.r);
}

// One source component (mean -> image p, covariance Sg) against the target record its image fell on: the 29 sums of
// ALGORITHM 2.14.  Written in the order tests/d2d3_ref.py states in float32 (mirror32), so that restatement bounds this
// code's error.  A miss takes the unit matrix for the target covariance, so that every term stays finite, and weighs 0.
template <int MODE>
__device__ __forceinline__ void accumulate_component3(const MapPose3& T, const float* Sg, float px, float py, float pz, bool in,
                                                      const float4& A4, const float4& B4, const float4& C2, float d1, float d2,
                                                      float nhd2, float* acc) {
  const bool hit = in & (A4.w > 0.f);
  float S[6];
  rotate_cov3(T.R, Sg, S);
  const float axx = S[0] + (hit ? B4.x : 1.f), axy = S[1] + (hit ? B4.y : 0.f), axz = S[2] + (hit ? B4.z : 0.f);
  const float ayy = S[3] + (hit ? B4.w : 1.f), ayz = S[4] + (hit ? C2.x : 0.f), azz = S[5] + (hit ? C2.y : 1.f);
  float B[6];
  V3 v;
  const float m = mahalanobis_sum3(axx, axy, axz, ayy, ayz, azz, V3{px - A4.x, py - A4.y, pz - A4.z}, B, v);
  const float s = hit ? d1 * __builtin_amdgcn_exp2f(nhd2 * m) : 0.f;
  const float w = s * d2;
  const V3 Sv = symv(S, v);
  const V3 pr{px - T.tx, py - T.ty, pz - T.tz};
  RotTerms3 t[3];
  rot_terms3<0>(T, S, B, pr, v, Sv, t[0]);
  rot_terms3<1>(T, S, B, pr, v, Sv, t[1]);
  rot_terms3<2>(T, S, B, pr, v, Sv, t[2]);
  const float v3[3] = {v.x, v.y, v.z};
  {
    int qq = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        float h = B[qq];
        if (MODE == 1) h = h - d2 * v3[i] * v3[j];
        acc[qq] = fmaf(w, h, acc[qq]);
        ++qq;
      }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u3[3] = {t[k].U.x, t[k].U.y, t[k].U.z};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float h = u3[r];
      if (MODE == 1) h = h - d2 * v3[r] * t[k].c;
      acc[6 + 3 * r + k] = fmaf(w, h, acc[6 + 3 * r + k]);
    }
  }
  {
    int qq = 15;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = k; l < 3; ++l) {
        float h = dot3(t[k].r, t[l].U);
        if (MODE == 1) {       // - d2 c_k c_l + v' j_kl - v' Z_kl v / 2, the last two = p_l . (e_k - j_k) - p_k . f_l
          const V3 ej{t[k].e.x - t[k].j.x, t[k].e.y - t[k].j.y, t[k].e.z - t[k].j.z};
          h = (h - d2 * t[k].c * t[l].c) + (dot3(t[l].p, ej) - dot3(t[k].p, t[l].f));
        }
        acc[qq] = fmaf(w, h, acc[qq]);
        ++qq;
      }
  }
  acc[21] = fmaf(w, v.x, acc[21]); acc[22] = fmaf(w, v.y, acc[22]); acc[23] = fmaf(w, v.z, acc[23]);
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[24 + k] = fmaf(w, t[k].c, acc[24 + k]);
  acc[27] += s;
  acc[28] += hit ? 1.f : 0.f;
}

// ---- map neighbourhood 7 (ALGORITHM 2.26): the same terms with a component's work split in two.  The NB = 1 kernels keep
// the text above untouched, and with it the instructions they compiled to before the option existed;
// what follows is accumulate_component3's operations on the same operands in the same order, so the own voxel's term is
// bit for bit that function's.
// What does not depend on the target voxel (mean -> image p, covariance Sg) - S = R Sg R', R mu = p - t and the three
// a_k x (R mu) - is formed once per component ...
struct ComponentFrame3 { float S[6]; V3 j[3]; };
__device__ __forceinline__ void component_frame3(const MapPose3& T, const float* Sg, float px, float py, float pz, ComponentFrame3& F) {
  rotate_cov3(T.R, Sg, F.S);
  const V3 pr{px - T.tx, py - T.ty, pz - T.tz};
  F.j[0] = axis_cross<0>(T, pr);
  F.j[1] = axis_cross<1>(T, pr);
  F.j[2] = axis_cross<2>(T, pr);
}
// (rot_terms3 with j = a_k x (R mu) from the frame)
template <int K>
__device__ __forceinline__ void rot_terms_of3(const MapPose3& T, const float* S, const float* B, const V3& j, const V3& v,
                                              const V3& Sv, RotTerms3& o) {
  o.j = j;
  o.p = axis_cross<K>(T, v);
  o.e = axis_cross<K>(T, Sv);
  o.f = symv(S, o.p);
  const V3 z{o.e.x - o.f.x, o.e.y - o.f.y, o.e.z - o.f.z};
  o.r = V3{o.j.x - z.x, o.j.y - z.y, o.j.z - z.z};
  o.c = dot3(v, o.j) - 0.5f * dot3(v, z);
  o.U = symv(B, o.r);
}
// ... and the rest once per candidate voxel (A4 = its mean and count, B4 and tyz, tzz = its covariance; hit = the
// candidate is in the grid and its record valid): S + Sigma_j, the cofactor inverse and its one division, v, S v, the
// rotation terms, the 29 sums.  A miss takes the unit matrix and weighs 0, as above.
template <int MODE>
__device__ __forceinline__ void accumulate_pair3(const MapPose3& T, const ComponentFrame3& F, float px, float py, float pz, bool hit,
                                                 const float4& A4, const float4& B4, float tyz, float tzz, float d1, float d2,
                                                 float nhd2, float* acc) {
  const float* S = F.S;
  const float axx = S[0] + (hit ? B4.x : 1.f), axy = S[1] + (hit ? B4.y : 0.f), axz = S[2] + (hit ? B4.z : 0.f);
  const float ayy = S[3] + (hit ? B4.w : 1.f), ayz = S[4] + (hit ? tyz : 0.f), azz = S[5] + (hit ? tzz : 1.f);
  float B[6];
  V3 v;
  const float m = mahalanobis_sum3(axx, axy, axz, ayy, ayz, azz, V3{px - A4.x, py - A4.y, pz - A4.z}, B, v);
  const float s = hit ? d1 * __builtin_amdgcn_exp2f(nhd2 * m) : 0.f;
  const float w = s * d2;
  const V3 Sv = symv(S, v);
  RotTerms3 t[3];
  rot_terms_of3<0>(T, S, B, F.j[0], v, Sv, t[0]);
  rot_terms_of3<1>(T, S, B, F.j[1], v, Sv, t[1]);
  rot_terms_of3<2>(T, S, B, F.j[2], v, Sv, t[2]);
  const float v3[3] = {v.x, v.y, v.z};
  {
    int qq = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        float h = B[qq];
        if (MODE == 1) h = h - d2 * v3[i] * v3[j];
        acc[qq] = fmaf(w, h, acc[qq]);
        ++qq;
      }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u3[3] = {t[k].U.x, t[k].U.y, t[k].U.z};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float h = u3[r];
      if (MODE == 1) h = h - d2 * v3[r] * t[k].c;
      acc[6 + 3 * r + k] = fmaf(w, h, acc[6 + 3 * r + k]);
    }
  }
  {
    int qq = 15;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = k; l < 3; ++l) {
        float h = dot3(t[k].r, t[l].U);
        if (MODE == 1) {       // - d2 c_k c_l + v' j_kl - v' Z_kl v / 2, the last two = p_l . (e_k - j_k) - p_k . f_l
          const V3 ej{t[k].e.x - t[k].j.x, t[k].e.y - t[k].j.y, t[k].e.z - t[k].j.z};
          h = (h - d2 * t[k].c * t[l].c) + (dot3(t[l].p, ej) - dot3(t[k].p, t[l].f));
        }
        acc[qq] = fmaf(w, h, acc[qq]);
        ++qq;
      }
  }
  acc[21] = fmaf(w, v.x, acc[21]); acc[22] = fmaf(w, v.y, acc[22]); acc[23] = fmaf(w, v.z, acc[23]);
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[24 + k] = fmaf(w, t[k].c, acc[24 + k]);
  acc[27] += s;
  acc[28] += hit ? 1.f : 0.f;
}

// Body and epilogue of a map-to-map launch for one alignment, shared by k_iterate_d2d3 and the multi-start chain
// (k_multi_body_d2d3), in the shape of evaluate_block3: this workgroup's components (i, i + stride, ...; the first one
// already loaded into ca, cb, cc) under the pose T, each mean looked up as a point is (a voxel of `cov` either way),
// per-thread sums, the wave's sums through LDS, one partial row entry per sum at partial_col[row * kMaxBlocks].
// NB = the target's map neighbourhood (ndt3d_set_map_neighbourhood, ALGORITHM 2.26): 1 = the voxel the image of the mean
// falls into, 7 = and its six face neighbours.
template <int MODE, int NB>
__device__ __forceinline__ void evaluate_components3(const Grid3Dev& G, const SolveParams& prm, const MapPose3& T,
                                                     const float4* __restrict__ comp, const float4* __restrict__ cov, int n, int i,
                                                     int stride, float4 ca, float4 cb, float4 cc, float (*s_wave)[kRowsMap3],
                                                     float* s_t_wave, float* __restrict__ partial_col) {
  constexpr int NA = kNumAccMap3;
  const Extent3F E = extent3(G);
  const float d1 = prm.d1, d2 = prm.d2;
  const float nhd2 = nhd2_of(d2);
  float acc[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) acc[j] = 0.f;
  static_assert(NB == 1 || NB == 7, "the map neighbourhood is the own voxel, or the own voxel and its six face neighbours");
  if constexpr (NB == 1) {
  while (i < n) {
    const int i2 = i + stride;
    float4 na = make_float4(0.f, 0.f, 0.f, 0.f), nb = na, nc = na;
    if (i2 < n) { na = comp[3 * (size_t)i2]; nb = comp[3 * (size_t)i2 + 1]; nc = comp[3 * (size_t)i2 + 2]; }
    const V3 p = image3(T.R, T.tx, T.ty, T.tz, ca.x, ca.y, ca.z);
    const Voxel3 vox = voxel_of3(G, E, p.x, p.y, p.z);
    const int key = vox.key;
    const float4 A4 = cov[3 * (size_t)key];
    const float4 B4 = cov[3 * (size_t)key + 1];
    const float4 C2 = cov[3 * (size_t)key + 2];
    const float Sg[6] = {cb.x, cb.y, cb.z, cb.w, cc.x, cc.y};
    accumulate_component3<MODE>(T, Sg, p.x, p.y, p.z, vox.in, A4, B4, C2, d1, d2, nhd2, acc);
    ca = na; cb = nb; cc = nc; i = i2;
  }
  } else {
  // Own voxel and its six face neighbours, in evaluate_block3<MODE, 7>'s order and by its rule: a candidate is taken by
  // index, and one that leaves the grid loads the own record (an address inside the array) and has no vote.  All seven
  // records (10 of a record's 12 words each) are requested in front of the first term; a candidate that is off the grid
  // or empty adds a term of weight zero (no branch: the lanes of a wave disagree on which candidates count).  The frame
  // - S, R mu and its three cross products - is formed once, under the loads.
  const int WH = G.W * G.H;
  while (i < n) {
    const int i2 = i + stride;
    float4 na = make_float4(0.f, 0.f, 0.f, 0.f), nb = na, nc = na;
    if (i2 < n) { na = comp[3 * (size_t)i2]; nb = comp[3 * (size_t)i2 + 1]; nc = comp[3 * (size_t)i2 + 2]; }
    const V3 p = image3(T.R, T.tx, T.ty, T.tz, ca.x, ca.y, ca.z);
    const VoxelIndex3 vox = voxel_index3(G, E, p.x, p.y, p.z);
    const bool in = vox.in;
    const bool ok[NB] = {in, in && vox.ix > 0, in && vox.ix + 1 < G.W, in && vox.iy > 0, in && vox.iy + 1 < G.H,
                         in && vox.iz > 0, in && vox.iz + 1 < G.D};
    const int dk[NB] = {0, -1, 1, -G.W, G.W, -WH, WH};
    float4 A4[NB], B4[NB];
    float2 C2[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const float4* r = cov + 3 * (size_t)(unsigned int)(vox.key + (ok[c] ? dk[c] : 0));
      A4[c] = r[0];
      B4[c] = r[1];
      C2[c] = *reinterpret_cast<const float2*>(r + 2);
    }
    // (left alone, the scheduler sinks the records of four candidates next to their terms to save registers: four more
    // exposed gather latencies in a launch of one wave per SIMD, which has nothing to hide them under)
    __builtin_amdgcn_sched_barrier(0);
    const float Sg[6] = {cb.x, cb.y, cb.z, cb.w, cc.x, cc.y};
    ComponentFrame3 F;
    component_frame3(T, Sg, p.x, p.y, p.z, F);
#pragma unroll
    for (int c = 0; c < NB; ++c)
      accumulate_pair3<MODE>(T, F, p.x, p.y, p.z, ok[c] & (A4[c].w > 0.f), A4[c], B4[c], C2[c].x, C2[c].y, d1, d2, nhd2, acc);
    ca = na; cb = nb; cc = nc; i = i2;
  }
  }
  block_reduce3_store<NA, kRowsMap3>(acc, s_t_wave, s_wave, partial_col);
}

// Launch k (parity = k & 1) consumes state[parity^1] / partials[parity^1] of launch k-1 and produces state[parity] /
// partials[parity]: k_iterate3<0>'s chain, state, flags, fold and reduction (the shared pieces of ndt_chain.hpp and
// ndt3d_kernels.hpp), with call->blocks workgroups of kBlock threads, a component per lane.  Both Hessian modes carry
// the same 29 sums:
// in the map-frame form the second-derivative terms are per-component, there is no M to contract in the prologue.
// NB (evaluate_components3) changes the body alone: the sums, their fold and the update are the same.
template <int MODE, int NB>
__global__ __launch_bounds__(kBlock) void k_iterate_d2d3(const AlignStatic3* __restrict__ st, const MapCall3* __restrict__ call,
                                                         AlignDyn3* __restrict__ dyn, int parity) {
  constexpr int NA = kNumAccMap3, RPW = kRowsMap3 / 4;
  __shared__ double s_red[kRowsMap3];
  __shared__ float s_wave[kBlock / 64][kRowsMap3];
  __shared__ float s_t[kBlock / 64][NA * kSum3RowStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const IterState3* prev = &dyn->state[parity ^ 1];
  IterState3* cur = &dyn->state[parity];
  const bool writer = (blockIdx.x == 0) && (tid == 0);

  // ---- batch 1 of loads: previous state (scalar), partial rows (vector), first component
  double pose[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) pose[j] = prev->pose[j];
  const int ps_iter = prev->iter, ps_done = prev->done, ps_have = prev->have_partials, ps_launch = prev->pad;
  const SolveParams prm = st->prm;
  const Grid3Dev G = st->grid;
  const int n = call->n;
  const int fixed_iterations = call->fixed_iterations;
  const float4* __restrict__ comp = call->comp;
  const float4* __restrict__ cov = call->cov;
  IterState3* const host_state = call->host_state;
  int* const host_flag = call->host_flag;
  float4 pv[RPW];
  {
    const float* part = &dyn->partials[parity ^ 1][0][0];
#pragma unroll
    for (int v = 0; v < RPW; ++v)
      pv[v] = *reinterpret_cast<const float4*>(part + (wave * RPW + v) * kMaxBlocks + lane * 4);
  }
  const int stride = (int)gridDim.x * kBlock;
  int i = blockIdx.x * kBlock + tid;
  float4 ca = make_float4(0.f, 0.f, 0.f, 0.f), cb = ca, cc = ca;
  if (i < n) { ca = comp[3 * (size_t)i]; cb = comp[3 * (size_t)i + 1]; cc = comp[3 * (size_t)i + 2]; }

  if (ps_done) {                         // uniform: a finished alignment just carries its state
    if (writer) chain_carry_done(cur, prev, host_flag, call);     // nothing reads the component list any more
    return;
  }
  int iter = ps_iter;
  if (ps_have) {
    // ---- prologue: fixed-order float64 fold of the kMaxBlocks partial columns (k_iterate3<0>'s: one round of 8 rows),
    // then the solve
    {
      double* t = reinterpret_cast<double*>(s_t[wave]);
#pragma unroll
      for (int v = 0; v < RPW; ++v)
        t[v * kSum3RowStride + lane] = (((double)pv[v].x + (double)pv[v].y) + (double)pv[v].z) + (double)pv[v].w;
      __builtin_amdgcn_wave_barrier();
      {
        const int v = lane >> 3;
        const double* row = t + v * kSum3RowStride + (lane & 7);
        double a = ((row[0] + row[8]) + (row[16] + row[24])) + ((row[32] + row[40]) + (row[48] + row[56]));
        a += dpp_mov<0xB1, 0xf>(a);
        a += dpp_mov<0x4E, 0xf>(a);
        a += dpp_mov<0x124, 0xf>(a);                             // row_ror:4 moves data up: lane 8v+4 gets lane 8v
        if ((lane & 7) == 4) s_red[wave * RPW + v] = a;
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // 6x6 from the 21 packed sums: Htt(6) Htr(9) Hrr(6)
    double A[36], g[6];
    A[0] = s_red[0]; A[1] = s_red[1]; A[2] = s_red[2]; A[7] = s_red[3]; A[8] = s_red[4]; A[14] = s_red[5];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) A[6 * r + 3 + k] = s_red[6 + 3 * r + k];
    A[21] = s_red[15]; A[22] = s_red[16]; A[23] = s_red[17]; A[28] = s_red[18]; A[29] = s_red[19]; A[35] = s_red[20];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < r; ++c) A[6 * r + c] = A[6 * c + r];
#pragma unroll
    for (int j = 0; j < 6; ++j) g[j] = s_red[21 + j];
    const double score = s_red[27];
    const int n_hit = (int)(s_red[28] + 0.5);
    int status = 0;
    const bool done = gn_update3(pose, A, g, n_hit, iter, status, prm, fixed_iterations, score, &dyn->ls[parity ^ 1],
                                 &dyn->ls[parity], writer);
    if (writer) {
      auto store = [&](IterState3* o) {          // the Gauss-Newton form in both modes: s_red holds the whole Hessian
        store_state3<0>(o, pose, g, s_red, A, score, n_hit, iter, status, done ? 1 : 0, ps_launch + 1);
      };
      store(cur);
      chain_announce(store, done, ps_launch + 1, host_state, host_flag, call);
    }
    if (done) return;                    // uniform
  } else if (writer) {
    copy_state(cur, prev, 1);
  }

  // ---- body and epilogue: per-component terms at `pose`
  MapPose3 T;
  make_map_pose3(pose, T);
  evaluate_components3<MODE, NB>(G, prm, T, comp, cov, n, i, stride, ca, cb, cc, s_wave, s_t[wave],
                             &dyn->partials[parity][0][blockIdx.x]);
}

}  // namespace ndt

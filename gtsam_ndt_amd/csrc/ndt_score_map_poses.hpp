// The map-to-map score of a source map at every pose of a LIST, against the target's cached grid (docs/ALGORITHM.md
// "Scoring a map at a list of poses"): what a loop closure between two submaps of unknown relative height and tilt, a
// submap-level particle filter or a caller's own sampler needs between ndt*_evaluate_map (one pose per call) and the
// (x, y, theta | yaw) lattice of ndt*_search_map.  Included at the end of ndt2d_api.hip, behind ndt_score_poses.hpp and
// the two *_d2d_search.hpp: the score kernels of both dimensions, the host template and the C ABI.
//
//   k_score_map_poses    in the shape of k_score_poses*: 256 consecutive list entries per workgroup, ONE LANE PER POSE.
//   k_score_map_poses3   The source's RAW components are staged through LDS a round of the lattice kernels' at a time
//                        (kMapSearchChunk / kMapSearch3Chunk; 5 floats in 2D, 9 in 3D) and read back as broadcasts.
//                        What k_search_score_d2d* hoist per heading is done per lane here: every lane rotates Sigma_i
//                        with its own R (2D: the five operations of the lattice kernel's staging; 3D: rotate_cov3),
//                        forms the image of the mean (2D: image_point's fma order; 3D: image_row3 for all three rows,
//                        layer_key3 and voxel_clamped3), gathers its own covariance records - those of four
//                        components are issued before the first is consumed, and the rotations run under their
//                        latency - and keeps a private float sum in the lattice kernels' order (two chains over the
//                        even and odd components of a round, then total += s0 + s1) and a private hit count.  A list
//                        that spells a search lattice gives ndt*_search_map_scores' volume bit for bit; a pose's
//                        score and count depend on nothing but the two grids and that pose.  No cross-lane
//                        reduction, no atomics.  Per component the arithmetic is search_component_score /
//                        search_component_score3.  A pose that is not finite, or whose float32 form is not, scores
//                        exactly +0 with count 0.
//   The keys, the shortlist and the gather of a best-poses call are ndt_score_poses.hpp's (best_poses_select).
#pragma once

#include "ndt2d_d2d_search.hpp"
#include "ndt3d_d2d_search.hpp"
#include "ndt_score_poses.hpp"

namespace ndt {

// cov = the target's covariance records, comp[2n] = the source's component list, both as kernel arguments (global, not
// flat, loads).  poses[m][3] = (x, y, theta) in double.  Lanes past m compute the last entry and store nothing.  n_hit may
// be null.
__global__ __launch_bounds__(kPoseThreads) void k_score_map_poses(const AlignStatic* __restrict__ st, const float4* __restrict__ cov,
                                                                  float d1, float d2, const float4* __restrict__ comp, int n,
                                                                  const double* __restrict__ poses, unsigned int m,
                                                                  float* __restrict__ out, unsigned int* __restrict__ n_hit) {
  __shared__ float4 s_ms[kMapSearchChunk];                   // mu_x, mu_y, and Sigma_i's xx, xy as the list has them
  __shared__ float4 s_yy4[kMapSearchChunk / 4];              // Sigma_i's yy of four components
  float* s_yy = reinterpret_cast<float*>(s_yy4);
  const GridDev G = st->grid;
  const int tid = threadIdx.x;
  const unsigned int i = blockIdx.x * (unsigned int)kPoseThreads + tid;
  const bool live = i < m;
  double p[3];
  bool ok;
  load_pose<3>(poses, min(i, m - 1u), p, &ok);
  double sn_d, cs_d;
  sincos_wrapped(wrap_angle(p[2]), &sn_d, &cs_d);
  const PoseF P = make_pose((float)cs_d, (float)sn_d, (float)p[0], (float)p[1], G.ox, G.oy, G.inv_c, G.W, G.H, d1, d2);
  ok = ok && isfinite(P.cs) && isfinite(P.sn) && isfinite(P.tx) && isfinite(P.ty);
  RotF R;                                                    // as k_search_score_d2d
  R.c2t = P.cs * P.cs - P.sn * P.sn;
  R.s2t = 2.f * P.cs * P.sn;
  float total = 0.f;
  unsigned int count = 0u;
  for (int base = 0; base < n; base += kMapSearchChunk) {
    const int mc = min(kMapSearchChunk, n - base);
    const int m4 = (mc + 3) & ~3;
    __syncthreads();                                         // the previous round has been read by every wave
    for (int k = tid; k < m4; k += kPoseThreads) {
      // image_point's clamp once per component; the round is padded to a multiple of four as k_search_score_d2d pads it
      // (the mean at the clamp bound: the grid's empty outer ring, exactly 0 and no hit; the unit matrix for Sigma)
      float4 ms = make_float4(1e15f, 1e15f, 1.f, 0.f);
      float syy = 1.f;
      if (k < mc) {
        const float4 ca = comp[2 * (size_t)(base + k)], cb = comp[2 * (size_t)(base + k) + 1];
        ms = make_float4(clamp_coord(ca.x), clamp_coord(ca.y), ca.z, ca.w);
        syy = cb.y;
      }
      s_ms[k] = ms;
      s_yy[k] = syy;
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < m4; k += 4) {
      const float4 yy = s_yy4[k >> 2];                       // broadcast reads: components k .. k + 3
      const float sc[4] = {yy.x, yy.y, yy.z, yy.w};
      float4 c[4];
      PointRec r[4];
      // all four gathers in flight before the first is consumed
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c[u] = s_ms[k + u];
        image_clamped(P, c[u].x, c[u].y, r[u]);
        const int key = image_key(P, P.ox, P.oy, r[u], true);          // clamped onto the grid: a cell of `cov`
        r[u].A = cov[2 * key];
        r[u].B = cov[2 * key + 1];
      }
      // S = R Sigma_i R^T with the lane's own heading: the five operations of k_search_score_d2d's staging
      float sxx[4], sxy[4], syy[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float sa = c[u].z, sb = c[u].w;
        const float hm = 0.5f * (sa + sc[u]), hd = 0.5f * (sa - sc[u]);
        const float w = fmaf(hd, R.c2t, -sb * R.s2t);
        sxx[u] = hm + w;
        sxy[u] = fmaf(hd, R.s2t, sb * R.c2t);
        syy[u] = hm - w;
      }
      s0 += search_component_score(P, r[0], sxx[0], sxy[0], syy[0]);
      s1 += search_component_score(P, r[1], sxx[1], sxy[1], syy[1]);
      s0 += search_component_score(P, r[2], sxx[2], sxy[2], syy[2]);
      s1 += search_component_score(P, r[3], sxx[3], sxy[3], syy[3]);
#pragma unroll
      for (int u = 0; u < 4; ++u) count += r[u].B.z > 0.f ? 1u : 0u;   // search_component_score's hit
    }
    total += s0 + s1;
  }
  if (live) {
    out[i] = ok ? total : 0.f;
    if (n_hit) n_hit[i] = ok ? count : 0u;
  }
}

// comp[3n] = the source's component list.  poses[m][6] = (tx, ty, tz, roll, pitch, yaw) in double.  Lanes past m compute
// the last entry and store nothing.  n_hit may be null.  U = 2 or 4: the components whose gathers are in flight together
// (DESIGN.md section 5.18); the sums take the same order either way.
template <int U>
__global__ __launch_bounds__(kPoseThreads) void k_score_map_poses3(const AlignStatic3* __restrict__ st, const float4* __restrict__ cov,
                                                                   float d1, float d2, const float4* __restrict__ comp, int n,
                                                                   const double* __restrict__ poses, unsigned int m,
                                                                   float* __restrict__ out, unsigned int* __restrict__ n_hit) {
  __shared__ float4 s_mu[kMapSearch3Chunk];                  // mu and Sigma_i's xx
  __shared__ float4 s_sg[kMapSearch3Chunk];                  // Sigma_i's xy xz yy yz
  __shared__ float4 s_zz4[kMapSearch3Chunk / 4];             // Sigma_i's zz of four components
  float* s_zz = reinterpret_cast<float*>(s_zz4);
  const Grid3Dev G = st->grid;
  const int tid = threadIdx.x;
  const unsigned int i = blockIdx.x * (unsigned int)kPoseThreads + tid;
  const bool live = i < m;
  const Extent3F E = extent3(G);
  const float nhd2 = nhd2_of(d2);
  const unsigned int layer = (unsigned int)(G.W * G.H);
  const unsigned int last_cell = layer * (unsigned int)G.D - 1u;
  float R[9], tx, ty, tz;
  bool ok;
  {
    double p[6];
    load_pose<6>(poses, min(i, m - 1u), p, &ok);
    for (int a = 3; a < 6; ++a) p[a] = wrap_angle(p[a]);
    MapPose3 T;
    make_map_pose3(p, T);                                    // R and t; the axes of the derivatives are not used
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = T.R[q];
    tx = T.tx; ty = T.ty; tz = T.tz;
    ok = ok && isfinite(tx) && isfinite(ty) && isfinite(tz);
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && isfinite(R[q]);
  }
  float total = 0.f;
  unsigned int count = 0u;
  for (int base = 0; base < n; base += kMapSearch3Chunk) {
    const int mc = min(kMapSearch3Chunk, n - base);
    const int m4 = (mc + 3) & ~3;
    __syncthreads();                                         // the previous round has been read by every wave
    for (int k = tid; k < m4; k += kPoseThreads) {
      // The round is padded to a multiple of four with components whose mean is NaN (their image fails the inside test:
      // exactly 0 and no hit) and whose Sigma is the unit matrix (S + Sigma_j keeps a positive determinant).
      const float nan = __builtin_nanf("");
      float4 mu = make_float4(nan, nan, nan, 1.f), sg = make_float4(0.f, 0.f, 1.f, 0.f);
      float szz = 1.f;
      if (k < mc) {
        const float4 ca = comp[3 * (size_t)(base + k)], cb = comp[3 * (size_t)(base + k) + 1],
                     cc = comp[3 * (size_t)(base + k) + 2];
        mu = make_float4(ca.x, ca.y, ca.z, cb.x);
        sg = make_float4(cb.y, cb.z, cb.w, cc.x);
        szz = cc.y;
      }
      s_mu[k] = mu;
      s_sg[k] = sg;
      s_zz[k] = szz;
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < m4; k += 4) {
      const float4 zz4 = s_zz4[k >> 2];                      // (broadcast reads: every lane reads the same components)
      const float zz[4] = {zz4.x, zz4.y, zz4.z, zz4.w};
      float term[4];
#pragma unroll
      for (int h = 0; h < 4; h += U) {
        float px[U], py[U], pz[U], sxx[U];
        bool in[U];
        float4 A[U], B[U];
        float2 Cc[U];
        // all U gathers in flight before the first is consumed
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float4 q = s_mu[k + h + u];
          px[u] = image_row3(R, tx, q.x, q.y, q.z);
          py[u] = image_row3(R + 3, ty, q.x, q.y, q.z);
          pz[u] = image_row3(R + 6, tz, q.x, q.y, q.z);      // (layer_key3 per lane here: the rotation is the lane's)
          sxx[u] = q.w;
          const Voxel3 vox = voxel_clamped3(G, E, layer_key3(G, E, pz[u], layer), px[u], py[u], last_cell);
          in[u] = vox.in;
          const float4* r = cov + 3 * (size_t)(unsigned int)vox.key;
          A[u] = r[0];
          B[u] = r[1];
          Cc[u] = *reinterpret_cast<const float2*>(r + 2);
        }
        __builtin_amdgcn_sched_barrier(0);                   // no wait moves up between the loads
        // the rotations run behind the gathers, under their latency
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float4 g = s_sg[k + h + u];
          const float Sg[6] = {sxx[u], g.x, g.y, g.z, g.w, zz[h + u]};
          float S[6];
          rotate_cov3(R, Sg, S);
          term[h + u] = search_component_score3(px[u], py[u], pz[u], in[u], make_float4(S[0], S[1], S[2], S[3]), S[4], S[5],
                                                A[u], B[u], Cc[u], d1, nhd2);
          count += (in[u] & (A[u].w > 0.f)) ? 1u : 0u;       // search_component_score3's hit
        }
      }
      s0 += term[0];
      s1 += term[1];
      s0 += term[2];
      s1 += term[3];
    }
    total += s0 + s1;
  }
  if (live) {
    out[i] = ok ? total : 0.f;
    if (n_hit) n_hit[i] = ok ? count : 0u;
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

constexpr int kMapPoses3InFlight = 4;                        // k_score_map_poses3's U

// ---- what differs per dimension: the score launch on t's stream
void launch_score_map_poses(ndt2d_handle* t, ndt2d_handle* s, unsigned blocks, const double* d_poses, size_t m, float* d_scores,
                            uint32_t* d_n_hit) {
  using namespace ndt;
  hipLaunchKernelGGL(k_score_map_poses, dim3(blocks), dim3(kPoseThreads), 0, t->stream, t->d_static, (const float4*)t->d_cov,
                     (float)t->prm.d1, (float)t->prm.d2, (const float4*)s->d_comp, s->n_comp, d_poses, (unsigned)m, d_scores, d_n_hit);
}
void launch_score_map_poses(ndt3d_handle* t, ndt3d_handle* s, unsigned blocks, const double* d_poses, size_t m, float* d_scores,
                            uint32_t* d_n_hit) {
  using namespace ndt;
  hipLaunchKernelGGL(k_score_map_poses3<kMapPoses3InFlight>, dim3(blocks), dim3(kPoseThreads), 0, t->stream, t->d_static,
                     (const float4*)t->d_cov, (float)t->prm.d1, (float)t->prm.d2, (const float4*)s->d_comp, s->n_comp, d_poses,
                     (unsigned)m, d_scores, d_n_hit);
}

// The argument checks of every entry point, before any device call.  sel: a best-poses call (k, the separations and the
// hit outputs count).  *n_hits is 0 wherever it can be written.
template <class H>
int32_t score_map_poses_check(const H* t, const H* s, const void* poses, size_t m, const void* out, bool sel, double min_sep_trans,
                              double min_sep_rot, int32_t k, int32_t* n_hits) {
  if (n_hits) *n_hits = 0;
  if (!t || !s || !poses || !out || m == 0) return NDT_ERR_INVALID_ARG;
  if (sel) {
    if (!n_hits || k < 1 || k > HandleTraits<H>::kMaxStarts) return NDT_ERR_INVALID_ARG;
    if (!std::isfinite(min_sep_trans) || !std::isfinite(min_sep_rot) || min_sep_trans < 0.0 || min_sep_rot < 0.0)
      return NDT_ERR_INVALID_ARG;
  }
  if (m > (size_t)ndt::kSearchMaxPoses) {
    ndt::set_error("the pose list holds more than 2^25 poses");
    return NDT_ERR_CAPACITY;
  }
  return NDT_OK;
}

// Every entry point prepares the pair as ndt*_search_map does (prepare_single_voxel_map_pair: the refusal of a target
// at map neighbourhood 7, then prepare_map_pair: the handle errors before any device
// call, the alignment in flight finished, the derived data, t's stream behind s's); then the score launch on t's stream.
template <class H>
int32_t score_map_poses_enqueue(H* t, H* s, const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  launch_score_map_poses(t, s, (unsigned)((m + ndt::kPoseThreads - 1) / ndt::kPoseThreads), d_poses, m, d_scores, d_n_hit);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// ndt*_score_map_poses_dev
template <class H>
int32_t score_map_poses_dev(H* t, H* s, const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  { const int32_t cs = score_map_poses_check(t, s, d_poses, m, d_scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  { const int32_t ps = prepare_single_voxel_map_pair(t, s, "pose list"); if (ps != NDT_OK) return ps; }
  { const int32_t es = score_map_poses_enqueue(t, s, d_poses, m, d_scores, d_n_hit); if (es != NDT_OK) return es; }
  HIP_TRY(hipStreamSynchronize(t->stream));
  return NDT_OK;
}

// ndt*_score_map_poses: the list, the scores and the counts through the target's search scratch, as score_poses_host
template <class H>
int32_t score_map_poses_host(H* t, H* s, const double* poses, size_t m, float* scores, uint32_t* n_hit) {
  using namespace ndt;
  constexpr int P = HandleTraits<H>::kPose;
  { const int32_t cs = score_map_poses_check(t, s, poses, m, scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  { const int32_t ps = prepare_single_voxel_map_pair(t, s, "pose list"); if (ps != NDT_OK) return ps; }
  SearchScratch& S = t->srch;
  HIP_TRY(grow(&S.d_list, &S.list_cap, m * P, m * P + m * P / 4));
  HIP_TRY(grow(&S.d_vol, &S.vol_cap, m, m + m / 4));
  if (n_hit) HIP_TRY(grow(&S.d_cnt, &S.cnt_cap, m, m + m / 4));
  HIP_TRY(hipMemcpyAsync(S.d_list, poses, m * P * sizeof(double), hipMemcpyHostToDevice, t->stream));
  { const int32_t es = score_map_poses_enqueue(t, s, S.d_list, m, S.d_vol, n_hit ? S.d_cnt : nullptr); if (es != NDT_OK) return es; }
  HIP_TRY(hipMemcpyAsync(scores, S.d_vol, m * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  if (n_hit) HIP_TRY(hipMemcpyAsync(n_hit, S.d_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return NDT_OK;
}

// ndt*_best_map_poses_dev: scores into the target's scratch, then the tail of every best-poses call
template <class H>
int32_t best_map_poses_dev(H* t, H* s, const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                           typename HandleTraits<H>::Hit* hits, int32_t* n_hits) {
  using namespace ndt;
  { const int32_t cs = score_map_poses_check(t, s, d_poses, m, hits, true, min_sep_trans, min_sep_rot, k, n_hits); if (cs != NDT_OK) return cs; }
  { const int32_t ps = prepare_single_voxel_map_pair(t, s, "pose list"); if (ps != NDT_OK) return ps; }
  SearchScratch& S = t->srch;
  HIP_TRY(grow(&S.d_vol, &S.vol_cap, m, m + m / 4));
  { const int32_t es = score_map_poses_enqueue(t, s, d_poses, m, S.d_vol, nullptr); if (es != NDT_OK) return es; }
  return best_poses_select<H>(S, t->stream, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}

// ndt*_best_map_poses_align_dev: the hits, then every hit as a start of one map-to-map chain (nothing for zero hits)
template <class H>
int32_t best_map_poses_align_dev(H* t, H* s, const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                                 typename HandleTraits<H>::Hit* hits, typename HandleTraits<H>::Result* results, int32_t* n_hits) {
  if (n_hits) *n_hits = 0;
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = best_map_poses_dev(t, s, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
  if (st != NDT_OK || *n_hits < 1) return st;
  return search_hits_align<H>(hits, *n_hits, [&](const double* init) {
    H* sources[HandleTraits<H>::kMaxStarts];
    std::fill_n(sources, *n_hits, s);
    return map_multi_entry(t, sources, init, *n_hits, results);    // ndt*_align_map_multi
  });
}

}  // namespace

extern "C" {

int32_t ndt2d_score_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m, float* d_scores,
                                  uint32_t* d_n_hit) {
  TraceRange range("ndt2d_score_map_poses");
  return score_map_poses_dev(target, source, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt2d_score_map_poses(ndt2d_handle* target, ndt2d_handle* source, const double* poses, size_t m, float* scores,
                              uint32_t* n_hit) {
  TraceRange range("ndt2d_score_map_poses");
  return score_map_poses_host(target, source, poses, m, scores, n_hit);
}
int32_t ndt2d_best_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m, double min_sep_trans,
                                 double min_sep_rot, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits) {
  TraceRange range("ndt2d_best_map_poses");
  return best_map_poses_dev(target, source, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}
int32_t ndt2d_best_map_poses_align_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                       ndt2d_result* results, int32_t* n_hits) {
  TraceRange range("ndt2d_best_map_poses_align");
  return best_map_poses_align_dev(target, source, d_poses, m, min_sep_trans, min_sep_rot, k, hits, results, n_hits);
}

int32_t ndt3d_score_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m, float* d_scores,
                                  uint32_t* d_n_hit) {
  TraceRange range("ndt3d_score_map_poses");
  return score_map_poses_dev(target, source, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt3d_score_map_poses(ndt3d_handle* target, ndt3d_handle* source, const double* poses, size_t m, float* scores,
                              uint32_t* n_hit) {
  TraceRange range("ndt3d_score_map_poses");
  return score_map_poses_host(target, source, poses, m, scores, n_hit);
}
int32_t ndt3d_best_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m, double min_sep_trans,
                                 double min_sep_rot, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits) {
  TraceRange range("ndt3d_best_map_poses");
  return best_map_poses_dev(target, source, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}
int32_t ndt3d_best_map_poses_align_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt3d_search_hit* hits,
                                       ndt3d_result* results, int32_t* n_hits) {
  TraceRange range("ndt3d_best_map_poses_align");
  return best_map_poses_align_dev(target, source, d_poses, m, min_sep_trans, min_sep_rot, k, hits, results, n_hits);
}

}  // extern "C"

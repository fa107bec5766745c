// The NDT score of a scan at every pose of a SHORT list, with the count of lookups that hit a valid cell
// (docs/ALGORITHM.md "Scoring particles: a team of lanes per pose"): the particles of a particle filter, a few hundred
// to a few thousand poses, for which the one-lane-per-pose kernels of ndt_score_poses.hpp leave the device almost empty
// (below 65 536 poses every SIMD holds at most one wave, and that wave walks the whole scan; DESIGN 5.19 has the
// times).  Included at the end of ndt2d_api.hip, behind ndt_score_poses.hpp: the kernels of both dimensions, the host
// template and the C ABI.
//
//   k_score_particles<NG, TEAM>   2D and 3D: a TEAM of 64 or 256 lanes per pose, the scan's points dealt round the team.
//   k_score_particles3<TEAM>      The pose is formed as k_score_poses forms it (load_pose, wrap_angle, sincos_wrapped /
//                                 make_rot3, the float of the doubles, +0 with count 0 for a pose that is not finite in
//                                 double or in float32) and is uniform over the team, so it lives in scalar registers.
//                                 Per point the arithmetic is the list kernels' device functions unchanged (image_key,
//                                 search_point_score and the fmed3 clamp; image3, layer_key3, voxel_clamped3,
//                                 search_point_score3): every term has the list kernel's bits.  Only the order of the
//                                 sum differs, and it is defined over 256 VIRTUAL lanes, so the bits do not depend on
//                                 TEAM: point j belongs to virtual lane v = j mod 256; p[v] sums, from +0 and in
//                                 ascending j, the terms of its points (overlap_grids = 4: grids 0, 1, 2, 3 of a point
//                                 one at a time); q[l] = (p[l] + p[l+64]) + (p[l+128] + p[l+192]) for l < 64; then
//                                 q[l] = q[l] + q[l ^ s] for s = 32, 16, 8, 4, 2, 1; the score is q[0].
//                                 TEAM = 64: one wave per pose, four poses per workgroup; lane l owns the partials l,
//                                 l+64, l+128, l+192: a round of 256 points is four coalesced point loads and four
//                                 independent gathers in flight per lane, held together by a scheduling barrier as in
//                                 k_score_poses.  No LDS, no barrier.
//                                 TEAM = 256: one workgroup per pose; thread t owns p[t] and keeps four gathers in
//                                 flight over four of its points (2D with overlap_grids = 4: over one point's four
//                                 grids, because the point's terms are added grid by grid); the q step crosses the
//                                 waves through 1 KB of LDS and the butterfly runs in wave 0.
//                                 Points are read straight from global memory (each is read by one lane per pose); the
//                                 next round's points are loaded ahead of this round's gathers.  No atomics.
//                                 The hit count is the number of (point, grid) lookups that hit a valid cell - what
//                                 ndt*_evaluate_dev reports as n_hit at that pose - counted per wave on the scalar unit
//                                 from the compare mask (as accumulate_point does) and written only where the output
//                                 pointer is not null.
#pragma once

#include "ndt_score_poses.hpp"

namespace ndt {

constexpr int kParticleLanes = 256;             // virtual lanes of the summation order, and threads per workgroup
// Lists shorter than this run 256-lane teams by default.  Derived: 256 CUs x 4 SIMDs = 1024, below which one wave per pose
// leaves SIMDs empty.  Measured (kernel times): at 1024 poses the wide team is still ahead (2D 6.5 against
// 7.1 us, 3D 45 against 66 us), at 2048 the narrow one is ahead in 2D (8.3 against 9.8 us) and level in 3D (88 against 87),
// from 4096 on it is ahead or level everywhere: so the switch sits at 2048.
constexpr size_t kParticleWideBelow = 2048;

__device__ __forceinline__ int particle_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// q[l] = q[l] + q[l ^ s], s = 32 .. 1: every lane ends with the same bits (float addition commutes)
__device__ __forceinline__ float particle_butterfly(float q) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) q = q + __shfl_xor(q, s, 64);
  return q;
}

// The tail of both kernels.  TEAM = 64: p[4] are lane l's partials l, l+64, l+128, l+192 and hits the wave's count.
// TEAM = 256: p[0] is thread t's partial t and hits its wave's count; s_p[256], s_cnt[4] are the workgroup's LDS.
template <int TEAM>
__device__ __forceinline__ void particle_finish(const float* p, unsigned int hits, bool ok, unsigned int i, float* __restrict__ out,
                                                uint32_t* __restrict__ n_hit, float* s_p, unsigned int* s_cnt) {
  const int tid = threadIdx.x, lane = tid & 63;
  float q;
  if constexpr (TEAM == 64) {
    q = (p[0] + p[1]) + (p[2] + p[3]);
  } else {
    s_p[tid] = p[0];
    if (lane == 0) s_cnt[tid >> 6] = hits;
    __syncthreads();
    if (tid >= 64) return;
    q = (s_p[lane] + s_p[lane + 64]) + (s_p[lane + 128] + s_p[lane + 192]);
    hits = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
  }
  q = particle_butterfly(q);
  if (lane == 0) {
    out[i] = ok ? q : 0.f;
    if (n_hit) n_hit[i] = ok ? hits : 0u;
  }
}

// rec = st->grid.rec, as a kernel argument (global, not flat, gathers).  poses[m][3] = (x, y, theta) in double.
// TEAM = 64: (m + 3) / 4 workgroups, wave w of workgroup b scores entry 4 b + w; TEAM = 256: m workgroups.
template <int NG, int TEAM>
__global__ __launch_bounds__(kParticleLanes) void k_score_particles(const AlignStatic* __restrict__ st, const float4* __restrict__ rec,
                                                                    float d1, float d2, const float* __restrict__ sx,
                                                                    const float* __restrict__ sy, int n,
                                                                    const double* __restrict__ poses, unsigned int m,
                                                                    float* __restrict__ out, uint32_t* __restrict__ n_hit) {
  static_assert(TEAM == 64 || TEAM == 256, "a team is one wave or one workgroup");
  const GridDev G = st->grid;
  const int tid = threadIdx.x;
  const int t = TEAM == 64 ? (tid & 63) : tid;                      // the lane's place in its team
  const unsigned int i = TEAM == 64 ? blockIdx.x * 4u + (unsigned int)particle_uniform(tid >> 6) : blockIdx.x;
  if (i >= m) return;                                               // (TEAM = 64: a whole wave, and no barrier follows)
  double p3[3];
  bool ok;
  load_pose<3>(poses, i, p3, &ok);
  double sn_d, cs_d;
  sincos_wrapped(wrap_angle(p3[2]), &sn_d, &cs_d);
  // uniform over the team: the pose's four floats in scalar registers
  const PoseF P = make_pose(search_uniform((float)cs_d), search_uniform((float)sn_d), search_uniform((float)p3[0]),
                            search_uniform((float)p3[1]), G.ox, G.oy, G.inv_c, G.W, G.H, d1, d2);
  ok = ok && isfinite(P.cs) && isfinite(P.sn) && isfinite(P.tx) && isfinite(P.ty);
  const int ncell = G.W * G.H;
  // A round's points are loaded one round ahead, unconditionally (past n: the last point again), so that no wait sits
  // between the loads and the gathers issued behind them; place() then gives the point its value.  Points past n sit at
  // the clamp bound, on the grid's empty outer ring, as k_search_score pads its chunks: they add exactly +0 and hit
  // nothing.  (image_point's clamp once per point, here.)
  auto load_point = [&](int j, float& x, float& y) {
    const int jj = min(j, n - 1);
    x = sx[jj]; y = sy[jj];
  };
  auto place = [&](int j, float& x, float& y) {
    x = j < n ? clamp_coord(x) : 1e15f;
    y = j < n ? clamp_coord(y) : 1e15f;
  };
  unsigned int hits = 0;
  if constexpr (TEAM == 256 && NG == 4) {
    // one point per round; its four grids' gathers in flight, its four terms added grid by grid
    float p = 0.f;
    float x, y;
    load_point(t, x, y);
    for (int base = 0; base < n; base += TEAM) {
      float xn, yn;
      load_point(base + TEAM + t, xn, yn);                          // the next round's point, ahead of the gathers
      place(base + t, x, y);
      PointRec r[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        image_clamped(P, x, y, r[g]);
        const int key = g * ncell + image_key(P, G.gx[g], G.gy[g], r[g], true);
        r[g].A = rec[2 * key];
        r[g].B = rec[2 * key + 1];
      }
      __builtin_amdgcn_sched_barrier(0);                            // no wait moves up between the eight loads
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        p += search_point_score(P, r[g]);
        hits += (unsigned int)__popcll(__ballot(r[g].B.z > 0.f));
      }
      x = xn; y = yn;
    }
    __shared__ float s_p[kParticleLanes];
    __shared__ unsigned int s_cnt[4];
    particle_finish<TEAM>(&p, hits, ok, i, out, n_hit, s_p, s_cnt);
  } else {
    // four points per round, STRIDE apart: TEAM = 64 four virtual lanes' next points (four sums), TEAM = 256 the
    // thread's next four points (one sum, added in ascending j)
    constexpr int STRIDE = TEAM == 64 ? 64 : kParticleLanes, NP = TEAM == 64 ? 4 : 1;
    float p[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) p[u] = 0.f;
    float x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load_point(STRIDE * u + t, x[u], y[u]);
    for (int base = 0; base < n; base += 4 * STRIDE) {
      float xn[4], yn[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) load_point(base + 4 * STRIDE + STRIDE * u + t, xn[u], yn[u]);
      PointRec r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        place(base + STRIDE * u + t, x[u], y[u]);
        image_clamped(P, x[u], y[u], r[u]);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const float ox = NG == 1 ? G.ox : G.gx[g], oy = NG == 1 ? G.oy : G.gy[g];
        // all four gathers in flight before the first is consumed
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int key = g * ncell + image_key(P, ox, oy, r[u], true);
          r[u].A = rec[2 * key];
          r[u].B = rec[2 * key + 1];
        }
        __builtin_amdgcn_sched_barrier(0);                          // no wait moves up between the eight loads
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          p[NP == 4 ? u : 0] += search_point_score(P, r[u]);
          hits += (unsigned int)__popcll(__ballot(r[u].B.z > 0.f));
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) { x[u] = xn[u]; y[u] = yn[u]; }
    }
    if constexpr (TEAM == 256) {
      __shared__ float s_p[kParticleLanes];
      __shared__ unsigned int s_cnt[4];
      particle_finish<TEAM>(p, hits, ok, i, out, n_hit, s_p, s_cnt);
    } else {
      particle_finish<TEAM>(p, hits, ok, i, out, n_hit, nullptr, nullptr);
    }
  }
}

// poses[m][6] = (tx, ty, tz, roll, pitch, yaw) in double.  Workgroups and teams as k_score_particles.
template <int TEAM>
__global__ __launch_bounds__(kParticleLanes) void k_score_particles3(const AlignStatic3* __restrict__ st, const float4* __restrict__ rec,
                                                                     float d1, float d2, const float* __restrict__ sx,
                                                                     const float* __restrict__ sy, const float* __restrict__ sz, int n,
                                                                     const double* __restrict__ poses, unsigned int m,
                                                                     float* __restrict__ out, uint32_t* __restrict__ n_hit) {
  static_assert(TEAM == 64 || TEAM == 256, "a team is one wave or one workgroup");
  const Grid3Dev G = st->grid;
  const int tid = threadIdx.x;
  const int t = TEAM == 64 ? (tid & 63) : tid;
  const unsigned int i = TEAM == 64 ? blockIdx.x * 4u + (unsigned int)particle_uniform(tid >> 6) : blockIdx.x;
  if (i >= m) return;                                               // (TEAM = 64: a whole wave, and no barrier follows)
  const Extent3F E = extent3(G);
  const float nhd2 = nhd2_of(d2);
  const unsigned int layer = (unsigned int)(G.W * G.H);
  const unsigned int last_cell = layer * (unsigned int)G.D - 1u;
  float R[9], tx, ty, tz;
  bool ok;
  {
    double p6[6];
    load_pose<6>(poses, i, p6, &ok);
    for (int a = 3; a < 6; ++a) p6[a] = wrap_angle(p6[a]);
    Rot3F T;
    make_rot3(p6, T);                                               // R and t; the derivative matrices are not used
    // uniform over the team: in scalar registers
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = search_uniform(T.R[q]);
    tx = search_uniform(T.tx); ty = search_uniform(T.ty); tz = search_uniform(T.tz);
    ok = ok && isfinite(tx) && isfinite(ty) && isfinite(tz);
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && isfinite(R[q]);
  }
  // A round's points are loaded one round ahead, unconditionally (past n: the last point again), so that no wait sits
  // between the loads and the gathers issued behind them; place() then gives the point its value.  Points past n are
  // NaN points: their image fails the inside test, as a NaN point of the scan does, and they add exactly +0 and hit
  // nothing.
  auto load_point = [&](int j, float& x, float& y, float& z) {
    const int jj = min(j, n - 1);
    x = sx[jj]; y = sy[jj]; z = sz[jj];
  };
  auto place = [&](int j, float& x, float& y, float& z) {
    const float nan = __builtin_nanf("");
    x = j < n ? x : nan; y = j < n ? y : nan; z = j < n ? z : nan;
  };
  // four points per round, STRIDE apart: TEAM = 64 four virtual lanes' next points (four sums), TEAM = 256 the thread's
  // next four points (one sum, added in ascending j)
  constexpr int STRIDE = TEAM == 64 ? 64 : kParticleLanes, NP = TEAM == 64 ? 4 : 1;
  float p[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) p[u] = 0.f;
  unsigned int hits = 0;
  float x[4], y[4], z[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) load_point(STRIDE * u + t, x[u], y[u], z[u]);
  for (int base = 0; base < n; base += 4 * STRIDE) {
    float xn[4], yn[4], zn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load_point(base + 4 * STRIDE + STRIDE * u + t, xn[u], yn[u], zn[u]);
    float px[4], py[4], pz[4];
    bool in[4];
    float4 A[4], B[4];
    float2 C[4];
    // all four gathers in flight before the first is consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      place(base + STRIDE * u + t, x[u], y[u], z[u]);
      const V3 q = image3(R, tx, ty, tz, x[u], y[u], z[u]);
      px[u] = q.x; py[u] = q.y; pz[u] = q.z;
      const Voxel3 vox = voxel_clamped3(G, E, layer_key3(G, E, q.z, layer), q.x, q.y, last_cell);
      in[u] = vox.in;
      const float4* r = rec + 4 * (size_t)(unsigned int)vox.key;
      A[u] = r[0];
      B[u] = r[1];
      C[u] = *reinterpret_cast<const float2*>(r + 2);
    }
    __builtin_amdgcn_sched_barrier(0);                              // no wait moves up between the twelve loads
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      p[NP == 4 ? u : 0] += search_point_score3(px[u], py[u], pz[u], in[u], A[u], B[u], C[u], d1, nhd2);
      hits += (unsigned int)__popcll(__ballot(in[u] & (A[u].w > 0.f)));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { x[u] = xn[u]; y[u] = yn[u]; z[u] = zn[u]; }
  }
  if constexpr (TEAM == 256) {
    __shared__ float s_p[kParticleLanes];
    __shared__ unsigned int s_cnt[4];
    particle_finish<TEAM>(p, hits, ok, i, out, n_hit, s_p, s_cnt);
  } else {
    particle_finish<TEAM>(p, hits, ok, i, out, n_hit, nullptr, nullptr);
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// ---- what differs per dimension ----
template <int TEAM>
void launch_score_particles(ndt2d_handle* h, unsigned blocks, const float* const* d_s, size_t n, const double* d_poses, size_t m,
                            float* d_scores, uint32_t* d_n_hit) {
  using namespace ndt;
  const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;          // as upload_static
  if (h->prm.overlap_grids == 4)
    hipLaunchKernelGGL((k_score_particles<4, TEAM>), dim3(blocks), dim3(kParticleLanes), 0, h->stream, h->d_static,
                       (const float4*)h->grid.rec, d1, d2, d_s[0], d_s[1], (int)n, d_poses, (unsigned)m, d_scores, d_n_hit);
  else
    hipLaunchKernelGGL((k_score_particles<1, TEAM>), dim3(blocks), dim3(kParticleLanes), 0, h->stream, h->d_static,
                       (const float4*)h->grid.rec, d1, d2, d_s[0], d_s[1], (int)n, d_poses, (unsigned)m, d_scores, d_n_hit);
}
template <int TEAM>
void launch_score_particles(ndt3d_handle* h, unsigned blocks, const float* const* d_s, size_t n, const double* d_poses, size_t m,
                            float* d_scores, uint32_t* d_n_hit) {
  using namespace ndt;
  const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;          // as upload_static3
  hipLaunchKernelGGL(k_score_particles3<TEAM>, dim3(blocks), dim3(kParticleLanes), 0, h->stream, h->d_static,
                     (const float4*)h->grid.rec, d1, d2, d_s[0], d_s[1], d_s[2], (int)n, d_poses, (unsigned)m, d_scores, d_n_hit);
}

// the launch on h's stream, behind the alignment in flight (arguments checked); the team width is NDT_TUNE_PARTICLE_TEAM's,
// or by the list's length
template <class H>
int32_t score_particles_enqueue(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, float* d_scores,
                                uint32_t* d_n_hit) {
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  const int team = h->particle_team ? h->particle_team : (m < ndt::kParticleWideBelow ? 256 : 64);
  if (team == 256) launch_score_particles<256>(h, (unsigned)m, d_s, n, d_poses, m, d_scores, d_n_hit);
  else launch_score_particles<64>(h, (unsigned)((m + 3) / 4), d_s, n, d_poses, m, d_scores, d_n_hit);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// ndt*_score_particles_dev (sync) and ndt*_score_particles_async: the checks of ndt*_score_poses_dev, the launch, and for
// the first the wait
template <class H>
int32_t score_particles_dev(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, float* d_scores,
                            uint32_t* d_n_hit, bool sync) {
  { const int32_t cs = score_poses_check(h, d_s, n, d_poses, m, d_scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  { const int32_t es = score_particles_enqueue(h, d_s, n, d_poses, m, d_scores, d_n_hit); if (es != NDT_OK) return es; }
  if (sync) HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// ndt*_score_particles: the scan, the list, the scores and the counts through the search scratch, as score_poses_host
template <class H>
int32_t score_particles_host(H* h, const float* const* s, size_t n, const double* poses, size_t m, float* scores, uint32_t* n_hit) {
  using namespace ndt;
  constexpr int P = HandleTraits<H>::kPose;
  { const int32_t cs = score_poses_check(h, s, n, poses, m, scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  HIP_TRY(hipSetDevice(h->device));
  const float* d_s[3];
  { const int32_t ss = fit_stage(h, s, n, d_s); if (ss != NDT_OK) return ss; }
  SearchScratch& S = h->srch;
  HIP_TRY(grow(&S.d_list, &S.list_cap, m * P, m * P + m * P / 4));
  HIP_TRY(grow(&S.d_vol, &S.vol_cap, m, m + m / 4));
  if (n_hit) HIP_TRY(grow(&S.d_cnt, &S.cnt_cap, m, m + m / 4));
  HIP_TRY(hipMemcpyAsync(S.d_list, poses, m * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  { const int32_t es = score_particles_enqueue(h, d_s, n, S.d_list, m, S.d_vol, n_hit ? S.d_cnt : nullptr); if (es != NDT_OK) return es; }
  HIP_TRY(hipMemcpyAsync(scores, S.d_vol, m * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (n_hit) HIP_TRY(hipMemcpyAsync(n_hit, S.d_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_score_particles_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                  float* d_scores, uint32_t* d_n_hit) {
  TraceRange range("ndt2d_score_particles");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return score_particles_dev(h, s, n, d_poses, m, d_scores, d_n_hit, true);
}
int32_t ndt2d_score_particles_async(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                    float* d_scores, uint32_t* d_n_hit) {
  TraceRange range("ndt2d_score_particles_async");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return score_particles_dev(h, s, n, d_poses, m, d_scores, d_n_hit, false);
}
int32_t ndt2d_score_particles(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double* poses, size_t m,
                              float* scores, uint32_t* n_hit) {
  TraceRange range("ndt2d_score_particles");
  const float* s[3] = {sx, sy, nullptr};
  return score_particles_host(h, s, n, poses, m, scores, n_hit);
}

int32_t ndt3d_score_particles_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                  const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  TraceRange range("ndt3d_score_particles");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return score_particles_dev(h, s, n, d_poses, m, d_scores, d_n_hit, true);
}
int32_t ndt3d_score_particles_async(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                    const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  TraceRange range("ndt3d_score_particles_async");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return score_particles_dev(h, s, n, d_poses, m, d_scores, d_n_hit, false);
}
int32_t ndt3d_score_particles(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const double* poses,
                              size_t m, float* scores, uint32_t* n_hit) {
  TraceRange range("ndt3d_score_particles");
  const float* s[3] = {sx, sy, sz};
  return score_particles_host(h, s, n, poses, m, scores, n_hit);
}

}  // extern "C"

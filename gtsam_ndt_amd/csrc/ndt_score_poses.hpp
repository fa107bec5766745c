// The NDT score of a scan at every pose of a LIST, against the cached grid (docs/ALGORITHM.md "Scoring a list of poses"):
// what a particle filter, a relocaliser with outside hypotheses or a caller's own sampler needs between the single-pose
// evaluation and the lattice of an exhaustive search.  Included at the end of ndt2d_api.hip, behind the search headers:
// the score kernels of both dimensions, the key and gather kernels, the host template and the C ABI.
//
//   k_score_poses<NG>   2D, in the shape of k_search_score (ndt2d_search.hpp): 256 consecutive list entries per workgroup,
//   k_score_poses3      ONE LANE PER POSE.  The scan is staged through LDS in the search kernels' chunks and read back as
//                       broadcasts; each lane gathers its own records - the loads of four points are all issued before the
//                       first is waited for, which a scheduling barrier behind the gathers holds the compiler to (left
//                       alone it interleaves loads and waits to save registers) - and keeps a private float
//                       sum in the search kernels' order (two chains over the even and odd points of a chunk, then
//                       total += s0 + s1): a list that spells a search lattice gives the search's volume bit for bit, and
//                       a pose's score depends on nothing but the grid, the scan and that pose.  No cross-lane reduction,
//                       no atomics.  The per-point arithmetic is the search kernels' device functions (image_key and
//                       search_point_score; image3, layer_key3, voxel_clamped3 and search_point_score3).
//                       3D: the rotation is per lane, so layer_key3, which k_search_score3 calls once per point and
//                       workgroup at staging, is called per lane.
//                       A pose with a non-finite coordinate scores exactly +0, and so does a finite one whose float32
//                       form is not finite (a translation beyond float32, an angle whose wrap leaves no finite sine and
//                       cosine): no pose of the list gives a NaN score.
//   k_pose_keys         one 64-bit key (score bits << 32 | ~index) per pose with a positive score, appended per wave as
//                       k_search_peaks does; k_search_sel_* / k_search_collect / k_search_sort (ndt_search.hpp) then
//                       shortlist the best 4096 unchanged.
//   k_pose_gather       the shortlisted poses into one buffer, fetched with the shortlist in one synchronisation; the
//                       separation walk runs on the host.
#pragma once

#include "ndt2d_search.hpp"
#include "ndt3d_search.hpp"

namespace ndt {

constexpr int kPoseThreads = 256;               // list entries per workgroup

// P coordinates of list entry i; *ok = all finite (else the entry is the zero pose, whose score the caller discards)
template <int P>
__device__ __forceinline__ void load_pose(const double* __restrict__ poses, unsigned int i, double* p, bool* ok) {
  bool fin = true;
#pragma unroll
  for (int a = 0; a < P; ++a) {
    p[a] = poses[(size_t)P * i + a];
    fin = fin && isfinite(p[a]);
  }
#pragma unroll
  for (int a = 0; a < P; ++a) p[a] = fin ? p[a] : 0.0;
  *ok = fin;
}

// rec = st->grid.rec, as a kernel argument (global, not flat, gathers).  poses[m][3] = (x, y, theta) in double.  Lanes past
// m compute the last entry and store nothing.  The chunk loop is k_search_score's text (a list that spells a lattice
// gives the search's volume bit for bit only while the two stay in step): as one function for both kernels it measured
// outside the run-to-run spread at 65 536 poses.
template <int NG>
__global__ __launch_bounds__(kPoseThreads) void k_score_poses(const AlignStatic* __restrict__ st, const float4* __restrict__ rec,
                                                              float d1, float d2, const float* __restrict__ sx,
                                                              const float* __restrict__ sy, int n,
                                                              const double* __restrict__ poses, unsigned int m,
                                                              float* __restrict__ out) {
  __shared__ float4 s_pt4[kSearchChunk / 2];
  float2* s_pt = reinterpret_cast<float2*>(s_pt4);
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
  const int ncell = G.W * G.H;
  float total = 0.f;
  for (int base = 0; base < n; base += kSearchChunk) {
    const int mc = min(kSearchChunk, n - base);
    const int m4 = (mc + 3) & ~3;
    __syncthreads();                                     // the previous chunk has been read by every wave
    for (int k = tid; k < m4; k += kPoseThreads) {
      // image_point's clamp once per point, and the padding onto the grid's empty outer ring, as k_search_score
      float x = 1e15f, y = 1e15f;
      if (k < mc) {
        x = clamp_coord(sx[base + k]);
        y = clamp_coord(sy[base + k]);
      }
      s_pt[k] = make_float2(x, y);
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < m4; k += 4) {
      const float4 q01 = s_pt4[k >> 1], q23 = s_pt4[(k >> 1) + 1];   // points k .. k + 3 (a broadcast read)
      const float qx[4] = {q01.x, q01.z, q23.x, q23.z}, qy[4] = {q01.y, q01.w, q23.y, q23.w};
      PointRec r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) image_clamped(P, qx[u], qy[u], r[u]);
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
        // NG = 4: no wait moves up between a grid's eight loads (left alone the compiler serialises the last grids').  One
        // grid needs no barrier - its eight loads stay together - and is 7 % slower with one (2.01 against 1.87 ms on the
        // 1.34M-pose lattice of DESIGN 5.17)
        if (NG > 1) __builtin_amdgcn_sched_barrier(0);
        s0 += search_point_score(P, r[0]);
        s1 += search_point_score(P, r[1]);
        s0 += search_point_score(P, r[2]);
        s1 += search_point_score(P, r[3]);
      }
    }
    total += s0 + s1;
  }
  if (live) out[i] = ok ? total : 0.f;
}

// poses[m][6] = (tx, ty, tz, roll, pitch, yaw) in double.  Lanes past m compute the last entry and store nothing.
// amdgpu_waves_per_eu(1, 5): twelve loads in flight need 94 VGPRs, five waves per SIMD; aiming at eight waves the
// compiler keeps 63 and serialises the gathers into four round trips per four points instead (a target of six gives the
// same 94, of four 98).
__global__ __launch_bounds__(kPoseThreads) __attribute__((amdgpu_waves_per_eu(1, 5))) void k_score_poses3(const AlignStatic3* __restrict__ st, const float4* __restrict__ rec,
                                                               float d1, float d2, const float* __restrict__ sx,
                                                               const float* __restrict__ sy, const float* __restrict__ sz, int n,
                                                               const double* __restrict__ poses, unsigned int m,
                                                               float* __restrict__ out) {
  __shared__ float4 s_pt[kSearch3Chunk];                     // x, y, z
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
    Rot3F T;
    make_rot3(p, T);                                         // R and t; the derivative matrices are not used
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = T.R[q];
    tx = T.tx; ty = T.ty; tz = T.tz;
    ok = ok && isfinite(tx) && isfinite(ty) && isfinite(tz);
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && isfinite(R[q]);
  }
  float total = 0.f;
  for (int base = 0; base < n; base += kSearch3Chunk) {
    const int mc = min(kSearch3Chunk, n - base);
    const int m4 = (mc + 3) & ~3;
    __syncthreads();                                         // the previous chunk has been read by every wave
    for (int k = tid; k < m4; k += kPoseThreads) {
      // The chunk is padded to a multiple of four with NaN points: their image fails the inside test, as a NaN point of
      // the scan does, and they add exactly 0.
      float x = __builtin_nanf(""), y = x, z = x;
      if (k < mc) { x = sx[base + k]; y = sy[base + k]; z = sz[base + k]; }
      s_pt[k] = make_float4(x, y, z, 0.f);
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < m4; k += 4) {
      float px[4], py[4], pz[4];
      bool in[4];
      float4 A[4], B[4];
      float2 C[4];
      // all four gathers in flight before the first is consumed
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 q = s_pt[k + u];                        // (a broadcast read: every lane reads the same point)
        const V3 p = image3(R, tx, ty, tz, q.x, q.y, q.z);
        px[u] = p.x; py[u] = p.y; pz[u] = p.z;           // (layer_key3 per lane here: the rotation is the lane's)
        const Voxel3 vox = voxel_clamped3(G, E, layer_key3(G, E, p.z, layer), p.x, p.y, last_cell);
        in[u] = vox.in;
        gather_rec3(rec, vox.key, A[u], B[u], C[u]);
      }
      __builtin_amdgcn_sched_barrier(0);                     // no wait moves up between the twelve loads
      s0 += search_point_score3(px[0], py[0], pz[0], in[0], A[0], B[0], C[0], d1, nhd2);
      s1 += search_point_score3(px[1], py[1], pz[1], in[1], A[1], B[1], C[1], d1, nhd2);
      s0 += search_point_score3(px[2], py[2], pz[2], in[2], A[2], B[2], C[2], d1, nhd2);
      s1 += search_point_score3(px[3], py[3], pz[3], in[3], A[3], B[3], C[3], d1, nhd2);
    }
    total += s0 + s1;
  }
  if (live) out[i] = ok ? total : 0.f;
}

// One key per pose with a positive score, in the key format of k_search_peaks; one append per wave.
__global__ __launch_bounds__(256) void k_pose_keys(const float* __restrict__ scores, unsigned int m,
                                                   unsigned long long* __restrict__ keys, unsigned int cap,
                                                   SearchSel* __restrict__ sel) {
  const unsigned int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const float s = idx < m ? scores[idx] : 0.f;
  const bool cand = s > 0.f;
  const unsigned long long mask = __ballot(cand);
  if (mask == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  unsigned int base = 0;
  if (lane == leader) base = atomicAdd(&sel->count, (unsigned int)__popcll(mask));
  base = (unsigned int)__shfl((int)base, leader, 64);
  if (cand) {
    const unsigned int slot = base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
    if (slot < cap)                     // cap = m: never false, kept as a bounds check
      keys[slot] = ((unsigned long long)__float_as_uint(s) << 32) | (0xFFFFFFFFull - (unsigned long long)idx);
  }
}

// picked[c][P] = the list's pose behind shortlist entry c, c < n_out (behind k_search_sort)
template <int P>
__global__ __launch_bounds__(256) void k_pose_gather(const SearchSel* __restrict__ sel, const double* __restrict__ poses,
                                                     unsigned int m, double* __restrict__ picked) {
  const unsigned int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= min(sel->n_out, (unsigned int)kSearchShortlist)) return;
  const unsigned int idx = min(0xFFFFFFFFu - (unsigned int)(sel->keys[c] & 0xFFFFFFFFull), m - 1u);   // (a bounds check)
#pragma unroll
  for (int a = 0; a < P; ++a) picked[(size_t)P * c + a] = poses[(size_t)P * idx + a];
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// ---- what differs per dimension ----
void launch_score_poses(ndt2d_handle* h, unsigned blocks, const float* const* d_s, size_t n, const double* d_poses, size_t m,
                        float* d_scores) {
  using namespace ndt;
  const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;          // as upload_static
  if (h->prm.overlap_grids == 4)
    hipLaunchKernelGGL(k_score_poses<4>, dim3(blocks), dim3(kPoseThreads), 0, h->stream, h->d_static, (const float4*)h->grid.rec, d1,
                       d2, d_s[0], d_s[1], (int)n, d_poses, (unsigned)m, d_scores);
  else
    hipLaunchKernelGGL(k_score_poses<1>, dim3(blocks), dim3(kPoseThreads), 0, h->stream, h->d_static, (const float4*)h->grid.rec, d1,
                       d2, d_s[0], d_s[1], (int)n, d_poses, (unsigned)m, d_scores);
}
void launch_score_poses(ndt3d_handle* h, unsigned blocks, const float* const* d_s, size_t n, const double* d_poses, size_t m,
                        float* d_scores) {
  using namespace ndt;
  const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;          // as upload_static3
  hipLaunchKernelGGL(k_score_poses3, dim3(blocks), dim3(kPoseThreads), 0, h->stream, h->d_static, (const float4*)h->grid.rec, d1, d2,
                     d_s[0], d_s[1], d_s[2], (int)n, d_poses, (unsigned)m, d_scores);
}
int32_t pose_multi_start(ndt2d_handle* h, const float* const* d_s, size_t n, const double* init, int32_t m, ndt2d_result* results) {
  return ndt2d_align_multi_start_dev(h, d_s[0], d_s[1], n, init, m, results);
}
int32_t pose_multi_start(ndt3d_handle* h, const float* const* d_s, size_t n, const double* init, int32_t m, ndt3d_result* results) {
  return ndt3d_align_multi_start_dev(h, d_s[0], d_s[1], d_s[2], n, init, m, results);
}

// The argument checks of every entry point, before any device call.  sel: a best-poses call (k and the separations count).
template <class H>
int32_t score_poses_check(const H* h, const float* const* s, size_t n, const void* poses, size_t m, const void* out, bool sel,
                          double min_sep_trans, double min_sep_rot, int32_t k, const void* n_hits) {
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  if (!h || !poses || !out) return NDT_ERR_INVALID_ARG;
  for (int a = 0; a < DIM; ++a) if (!s[a]) return NDT_ERR_INVALID_ARG;
  if (n == 0 || n > kMaxSourcePoints || m == 0) return NDT_ERR_INVALID_ARG;
  if (sel) {
    if (!n_hits || k < 1 || k > HandleTraits<H>::kMaxStarts) return NDT_ERR_INVALID_ARG;
    if (!std::isfinite(min_sep_trans) || !std::isfinite(min_sep_rot) || min_sep_trans < 0.0 || min_sep_rot < 0.0)
      return NDT_ERR_INVALID_ARG;
  }
  if (m > (size_t)ndt::kSearchMaxPoses) {
    ndt::set_error("the pose list holds more than 2^25 poses");
    return NDT_ERR_CAPACITY;
  }
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  return single_voxel_only(h);
}

// the score launch on h's stream, behind the alignment in flight (arguments checked)
template <class H>
int32_t score_poses_enqueue(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, float* d_scores) {
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  launch_score_poses(h, (unsigned)((m + ndt::kPoseThreads - 1) / ndt::kPoseThreads), d_s, n, d_poses, m, d_scores);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// ndt*_score_poses_dev
template <class H>
int32_t score_poses_dev(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, float* d_scores) {
  { const int32_t cs = score_poses_check(h, d_s, n, d_poses, m, d_scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  { const int32_t es = score_poses_enqueue(h, d_s, n, d_poses, m, d_scores); if (es != NDT_OK) return es; }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// ndt*_score_poses: the scan staged as ndt*_search stages it, the list and the scores through the search scratch
template <class H>
int32_t score_poses_host(H* h, const float* const* s, size_t n, const double* poses, size_t m, float* scores) {
  using namespace ndt;
  constexpr int P = HandleTraits<H>::kPose;
  { const int32_t cs = score_poses_check(h, s, n, poses, m, scores, false, 0.0, 0.0, 1, nullptr); if (cs != NDT_OK) return cs; }
  HIP_TRY(hipSetDevice(h->device));
  const float* d_s[3];
  { const int32_t ss = fit_stage(h, s, n, d_s); if (ss != NDT_OK) return ss; }
  SearchScratch& S = h->srch;
  HIP_TRY(grow(&S.d_list, &S.list_cap, m * P, m * P + m * P / 4));
  HIP_TRY(grow(&S.d_vol, &S.vol_cap, m, m + m / 4));
  HIP_TRY(hipMemcpyAsync(S.d_list, poses, m * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  { const int32_t es = score_poses_enqueue(h, d_s, n, S.d_list, m, S.d_vol); if (es != NDT_OK) return es; }
  HIP_TRY(hipMemcpyAsync(scores, S.d_vol, m * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

// The greedy separation walk over the sorted shortlist and its poses picked[c][P] (gtsam_ndt_amd/search.py select_best):
// translation distance over x, y (and z), rotation distance the largest wrapped difference of the angles.
template <class H>
int32_t pose_walk(const ndt::SearchSel& sel, const double* picked, double min_sep_trans, double min_sep_rot, int32_t k,
                  typename HandleTraits<H>::Hit* hits) {
#pragma clang fp contract(off)
  constexpr int P = HandleTraits<H>::kPose, NT = P == 3 ? 2 : 3;
  int32_t m = 0;
  const double st2 = min_sep_trans * min_sep_trans, sr = min_sep_rot;
  for (unsigned int c = 0; c < sel.n_out && m < k; ++c) {
    const unsigned long long key = sel.keys[c];
    const unsigned int bits = (unsigned int)(key >> 32);
    const double* p = picked + (size_t)P * c;
    bool keep = true;
    for (int32_t q = 0; q < m && keep; ++q) {
      double d2 = 0.0, dr = 0.0;
      for (int a = 0; a < NT; ++a) { const double d = p[a] - hits[q].pose[a]; d2 = d2 + d * d; }
      for (int a = NT; a < P; ++a) dr = std::max(dr, std::fabs(ndt::wrap_angle(p[a] - hits[q].pose[a])));
      if (d2 < st2 && dr < sr) keep = false;
    }
    if (!keep) continue;
    typename HandleTraits<H>::Hit& hh = hits[m++];
    std::memset(&hh, 0, sizeof(hh));
    for (int a = 0; a < P; ++a) hh.pose[a] = p[a];
    std::memcpy(&hh.score, &bits, 4);
    hh.index = (int32_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
  }
  return m;
}

// The tail of every best-poses call, of a scan's list and of a map's (ndt_score_map_poses.hpp): the list's scores are
// enqueued into S.d_vol on `stream`; keys, shortlist, the shortlisted poses, the host's walk.  Synchronous.
template <class H>
int32_t best_poses_select(ndt::SearchScratch& S, hipStream_t stream, const double* d_poses, size_t m, double min_sep_trans,
                          double min_sep_rot, int32_t k, typename HandleTraits<H>::Hit* hits, int32_t* n_hits) {
  using namespace ndt;
  constexpr int P = HandleTraits<H>::kPose;
  constexpr size_t pick_bytes = (size_t)kSearchShortlist * 6 * sizeof(double);     // room for either dimension
  if (!S.d_pick) HIP_TRY(hipMalloc((void**)&S.d_pick, pick_bytes));
  if (!S.h_pick) HIP_TRY(pinned_alloc(&S.h_pick, pick_bytes));
  { const int32_t bs = search_keys_begin(S, stream, m); if (bs != NDT_OK) return bs; }      // every pose can be a candidate
  SearchSel* sel = S.d_sel;
  hipLaunchKernelGGL(k_pose_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const float*)S.d_vol, (unsigned)m, S.d_keys,
                     (unsigned)m, sel);
  search_keys_shortlist(S, stream, m);
  hipLaunchKernelGGL(k_pose_gather<P>, dim3(kSearchShortlist / 256), dim3(256), 0, stream, (const SearchSel*)sel, d_poses, (unsigned)m,
                     S.d_pick);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(S.h_sel, sel, sizeof(SearchSel), hipMemcpyDeviceToHost, stream));
  // (all kSearchShortlist rows, at most 196 KB: how many are filled is known only behind this same synchronisation;
  // the walk reads the first n_out)
  HIP_TRY(hipMemcpyAsync(S.h_pick, S.d_pick, (size_t)kSearchShortlist * P * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *n_hits = pose_walk<H>(*S.h_sel, S.h_pick, min_sep_trans, min_sep_rot, k, hits);
  return NDT_OK;
}

// ndt*_best_poses_dev: scores into the scratch, then the tail above
template <class H>
int32_t best_poses_dev(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, double min_sep_trans,
                       double min_sep_rot, int32_t k, typename HandleTraits<H>::Hit* hits, int32_t* n_hits) {
  using namespace ndt;
  { const int32_t cs = score_poses_check(h, d_s, n, d_poses, m, hits, true, min_sep_trans, min_sep_rot, k, n_hits); if (cs != NDT_OK) return cs; }
  *n_hits = 0;
  HIP_TRY(hipSetDevice(h->device));
  SearchScratch& S = h->srch;
  HIP_TRY(grow(&S.d_vol, &S.vol_cap, m, m + m / 4));
  { const int32_t es = score_poses_enqueue(h, d_s, n, d_poses, m, S.d_vol); if (es != NDT_OK) return es; }
  return best_poses_select<H>(S, h->stream, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}

// ndt*_best_poses_align_dev: the hits, then one multi-start call from their poses (nothing for zero hits)
template <class H>
int32_t best_poses_align_dev(H* h, const float* const* d_s, size_t n, const double* d_poses, size_t m, double min_sep_trans,
                             double min_sep_rot, int32_t k, typename HandleTraits<H>::Hit* hits,
                             typename HandleTraits<H>::Result* results, int32_t* n_hits) {
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = best_poses_dev(h, d_s, n, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
  if (st != NDT_OK || *n_hits == 0) return st;
  return search_hits_align<H>(hits, *n_hits, [&](const double* init) { return pose_multi_start(h, d_s, n, init, *n_hits, results); });
}

}  // namespace

extern "C" {

int32_t ndt2d_score_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                              float* d_scores) {
  TraceRange range("ndt2d_score_poses");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return score_poses_dev(h, s, n, d_poses, m, d_scores);
}
int32_t ndt2d_score_poses(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double* poses, size_t m, float* scores) {
  TraceRange range("ndt2d_score_poses");
  const float* s[3] = {sx, sy, nullptr};
  return score_poses_host(h, s, n, poses, m, scores);
}
int32_t ndt2d_best_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                             double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits) {
  TraceRange range("ndt2d_best_poses");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return best_poses_dev(h, s, n, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}
int32_t ndt2d_best_poses_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                   double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                   ndt2d_result* results, int32_t* n_hits) {
  TraceRange range("ndt2d_best_poses_align");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return best_poses_align_dev(h, s, n, d_poses, m, min_sep_trans, min_sep_rot, k, hits, results, n_hits);
}

int32_t ndt3d_score_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                              const double* d_poses, size_t m, float* d_scores) {
  TraceRange range("ndt3d_score_poses");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return score_poses_dev(h, s, n, d_poses, m, d_scores);
}
int32_t ndt3d_score_poses(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const double* poses,
                          size_t m, float* scores) {
  TraceRange range("ndt3d_score_poses");
  const float* s[3] = {sx, sy, sz};
  return score_poses_host(h, s, n, poses, m, scores);
}
int32_t ndt3d_best_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                             const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                             ndt3d_search_hit* hits, int32_t* n_hits) {
  TraceRange range("ndt3d_best_poses");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return best_poses_dev(h, s, n, d_poses, m, min_sep_trans, min_sep_rot, k, hits, n_hits);
}
int32_t ndt3d_best_poses_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                   const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                                   ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits) {
  TraceRange range("ndt3d_best_poses_align");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return best_poses_align_dev(h, s, n, d_poses, m, min_sep_trans, min_sep_rot, k, hits, results, n_hits);
}

}  // extern "C"

// Exhaustive pose search for 3D map-to-map alignment (docs/ALGORITHM.md section 2.16): the map-to-map score of
// ndt3d_evaluate_map at every pose of an (x, y, yaw) lattice, z, roll and pitch pinned to the window centre's, from the
// source handle's component list and the target handle's covariance records - no points.  Included at the end of
// ndt2d_api.hip, after ndt3d_search.hpp and ndt3d_d2d_api.hpp: the lattice, the peak selection, the scratch, the
// separation walk and the host run are ndt_search.hpp's, the 3D window and hit HandleTraits<ndt3d_handle>'s, the component
// list and the covariance records ndt_map_host.hpp's.
//
//   k_search_score_d2d3  the score volume, in the shape of k_search_score3 / k_search_score_d2d: one workgroup = one yaw x
//                        a 16 x 16 tile of translations, ONE LANE PER TRANSLATION, a wave an 8 x 8 block.  R is uniform
//                        over the workgroup (scalar registers).  What does not depend on the translation in x and y is
//                        done once per component and workgroup while the chunk is staged into LDS: S = (R Sigma_i) R^T
//                        (rotate_cov3, 27 dot3 products), the image's z, its inside test and the voxel layer's key
//                        (layer_key3).  A lane reads the component back as broadcasts, forms the image's x and y with
//                        its own translation (image_row3, which evaluate_components3 calls through image3: the voxel
//                        key is the contract's, in the clamped form voxel_clamped3), gathers its own covariance
//                        record and keeps a private float sum in component order.  No cross-lane reduction and no
//                        atomics: the volume is the same bit for bit on every call.  Per component the float32
//                        arithmetic is the score part of accumulate_component3; only the summation order differs.
#pragma once

#include "ndt3d_d2d.hpp"
#include "ndt_search.hpp"

namespace ndt {

// Source components staged in LDS per round: 11 words each, 22,528 bytes per workgroup, so LDS allows seven workgroups
// per CU (160 KiB) where the registers allow four or five: it never limits occupancy.  (1024 components would be 45,056
// bytes: three workgroups per CU.)  Four components are eleven broadcast ds_read_b128:
//   s_mu[k]  = (mu_x, mu_y, mu_z, image z)     s_sa[k] = (Sxx, Sxy, Sxz, Syy)
//   s_sb[3 (k / 4) + 0 .. 2] = Syz, Szz and the layer key of components k .. k + 3
constexpr int kMapSearch3Chunk = 512;

// The score part of accumulate_component3 (ndt3d_d2d.hpp) with S already rotated: its mahalanobis_sum3 and exponent.
// A miss keeps whatever record the clamped key named (all zero for an invalid voxel): S is positive definite on its own,
// and the term is deselected.
__device__ __forceinline__ float search_component_score3(float px, float py, float pz, bool in, const float4& sa, float syz,
                                                         float szz, const float4& A4, const float4& B4, const float2& C2,
                                                         float d1, float nhd2) {
  const bool hit = in & (A4.w > 0.f);
  float B[6];
  V3 v;
  const float m = mahalanobis_sum3(sa.x + B4.x, sa.y + B4.y, sa.z + B4.z, sa.w + B4.w, syz + C2.x, szz + C2.y,
                                   V3{px - A4.x, py - A4.y, pz - A4.z}, B, v);
  return hit ? d1 * __builtin_amdgcn_exp2f(nhd2 * m) : 0.f;
}

// One lattice pose per lane.  cov = the target handle's covariance records, as a kernel argument: the gathers are
// global (not flat) loads.  st = the target's static context (its grid geometry); comp[3n] = the source's component
// list.  Axes, pinned coordinates, tasks and the store: as k_search_score3.
__global__ __launch_bounds__(kSearchThreads, 4) void k_search_score_d2d3(const AlignStatic3* __restrict__ st,
                                                                      const float4* __restrict__ cov, float d1, float d2,
                                                                      const float4* __restrict__ comp, int n,
                                                                      const float* __restrict__ ax, const float* __restrict__ ay,
                                                                      const double* __restrict__ ayaw, double cz, double croll,
                                                                      double cpitch, int nx, int ny, int nt,
                                                                      float* __restrict__ out) {
  __shared__ float4 s_mu[kMapSearch3Chunk];                  // mu and the image's z
  __shared__ float4 s_sa[kMapSearch3Chunk];                  // Sxx Sxy Sxz Syy
  __shared__ float4 s_sb[3 * (kMapSearch3Chunk / 4)];        // per four components: Syz x 4, Szz x 4, layer key x 4
  float* s_sbf = reinterpret_cast<float*>(s_sb);
  const Grid3Dev G = st->grid;
  const int tiles_x = (nx + kSearchTile - 1) / kSearchTile, tiles_y = (ny + kSearchTile - 1) / kSearchTile;
  const long long nblocks = (long long)tiles_x * tiles_y * nt;
  const int tid = threadIdx.x;
  const Extent3F E = extent3(G);
  const float nhd2 = nhd2_of(d2);
  const int layer = G.W * G.H;
  const unsigned last_cell = (unsigned)(layer * G.D - 1);
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const SearchTask task = search_task(b, tiles_x, tiles_y, nx, ny);      // (its `live` is formed again below)
    const int j = task.j, tile_x = task.tile_x, tile_y = task.tile_y, ix = task.ix, iy = task.iy;
    const double pose[6] = {0.0, 0.0, cz, croll, cpitch, ayaw[j]};
    const PoseRt3 T = make_rt3(pose);                        // R and tz
    float R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = search_uniform(T.R[q]);
    const float tz = search_uniform(T.tz);
    const float tx = ax[min(ix, nx - 1)], ty = ay[min(iy, ny - 1)];   // the float of the double, as make_rt3's tx
    float total = 0.f;
    for (int base = 0; base < n; base += kMapSearch3Chunk) {
      const int m = min(kMapSearch3Chunk, n - base);
      const int m4 = (m + 3) & ~3;
      __syncthreads();                                       // the previous chunk (or task) has been read by every wave
      for (int k = tid; k < m4; k += kSearchThreads) {
        // The chunk is padded to a multiple of four with components that fail the inside test (layer -1: they add
        // exactly 0) and carry the unit matrix (S + Sigma_j keeps a positive determinant), so the loop below needs no tail.
        float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), sa = make_float4(1.f, 0.f, 0.f, 1.f);
        float syz = 0.f, szz = 1.f;
        int lk = -1;
        if (k < m) {
          const float4 ca = comp[3 * (size_t)(base + k)], cb = comp[3 * (size_t)(base + k) + 1],
                       cc = comp[3 * (size_t)(base + k) + 2];
          const float pz = image_row3(R + 6, tz, ca.x, ca.y, ca.z);
          const Voxel3 L = layer_key3(G, E, pz, (unsigned)layer);
          if (L.in) lk = L.key;
          mu = make_float4(ca.x, ca.y, ca.z, pz);
          const float Sg[6] = {cb.x, cb.y, cb.z, cb.w, cc.x, cc.y};
          float S[6];
          rotate_cov3(R, Sg, S);
          sa = make_float4(S[0], S[1], S[2], S[3]);
          syz = S[4];
          szz = S[5];
        }
        s_mu[k] = mu;
        s_sa[k] = sa;
        const int g = 12 * (k >> 2) + (k & 3);
        s_sbf[g] = syz;
        s_sbf[g + 4] = szz;
        s_sbf[g + 8] = __int_as_float(lk);
      }
      __syncthreads();
      // two partial sums (even / odd components) per chunk: two independent chains, and short ones for accuracy
      float s0 = 0.f, s1 = 0.f;
      for (int k = 0; k < m4; k += 4) {
        const float4 l4 = s_sb[3 * (k >> 2) + 2];              // (broadcast reads: every lane reads the same components)
        const int lk[4] = {__float_as_int(l4.x), __float_as_int(l4.y), __float_as_int(l4.z), __float_as_int(l4.w)};
        float px[4], py[4], pz[4];
        bool in[4];
        float4 A[4], B[4];
        float2 Cc[4];
        // all four gathers in flight before the first is consumed
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 p = s_mu[k + u];
          px[u] = image_row3(R, tx, p.x, p.y, p.z);
          py[u] = image_row3(R + 3, ty, p.x, p.y, p.z);
          pz[u] = p.w;
          const Voxel3 vox = voxel_clamped3(G, E, Voxel3{lk[u], lk[u] >= 0}, px[u], py[u], last_cell);
          in[u] = vox.in;
          gather_cov3(cov, vox.key, A[u], B[u], Cc[u]);
        }
        // S is read behind the gathers: its LDS latency hides under theirs, and 24 registers fewer are live across them
        const float4 yz4 = s_sb[3 * (k >> 2)], zz4 = s_sb[3 * (k >> 2) + 1];
        const float syz[4] = {yz4.x, yz4.y, yz4.z, yz4.w}, szz[4] = {zz4.x, zz4.y, zz4.z, zz4.w};
        const float4 sa[4] = {s_sa[k], s_sa[k + 1], s_sa[k + 2], s_sa[k + 3]};
        s0 += search_component_score3(px[0], py[0], pz[0], in[0], sa[0], syz[0], szz[0], A[0], B[0], Cc[0], d1, nhd2);
        s1 += search_component_score3(px[1], py[1], pz[1], in[1], sa[1], syz[1], szz[1], A[1], B[1], Cc[1], d1, nhd2);
        s0 += search_component_score3(px[2], py[2], pz[2], in[2], sa[2], syz[2], szz[2], A[2], B[2], Cc[2], d1, nhd2);
        s1 += search_component_score3(px[3], py[3], pz[3], in[3], sa[3], syz[3], szz[3], A[3], B[3], Cc[3], d1, nhd2);
      }
      total += s0 + s1;
    }
    {
      // the lane's pose index again, from the thread index behind an opaque move: carried across the loops above, ix
      // and iy cost the two registers that stand between this kernel and four waves per SIMD
      int tl = tid;
      asm volatile("" : "+v"(tl));
      const int ox = tile_x + ((tl >> 6) & 1) * 8 + (tl & 7), oy = tile_y + (tl >> 7) * 8 + ((tl & 63) >> 3);
      if (ox < nx && oy < ny) out[((size_t)j * ny + oy) * nx + ox] = total;
    }
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// The whole map-to-map search (search_host_run) on the TARGET handle's stream and search scratch; the source handle lends
// its component list.  Here: the score launch, with the pinned coordinates.
int32_t search_map_run3(ndt3d_handle* t, ndt3d_handle* s, const ndt3d_search_window* w3, int32_t k, ndt3d_search_hit* hits,
                        int32_t* n_hits, float* d_scores) {
  using namespace ndt;
  TraceRange range(d_scores ? "ndt3d_search_map_scores" : "ndt3d_search_map");
  return search_host_run(t, s, w3, k, hits, n_hits, d_scores, [&](const SearchPlan& plan, unsigned grid, float* vol) {
    hipLaunchKernelGGL(k_search_score_d2d3, dim3(grid), dim3(kSearchThreads), 0, t->stream, t->d_static, (const float4*)t->d_cov,
                       (float)t->prm.d1, (float)t->prm.d2, (const float4*)s->d_comp, s->n_comp, plan.d_x, plan.d_y, plan.d_rot,
                       w3->center[2], w3->center[3], w3->center[4], plan.L.nx, plan.L.ny, plan.L.nt, vol);
  });
}

}  // namespace

extern "C" {

int32_t ndt3d_search_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, int32_t k,
                         ndt3d_search_hit* hits, int32_t* n_hits) {
  if (!target || !source || !w || !hits || !n_hits) return NDT_ERR_INVALID_ARG;
  if (k < 1 || k > ndt::kMaxStarts3) return NDT_ERR_INVALID_ARG;
  *n_hits = 0;
  return search_map_run3(target, source, w, k, hits, n_hits, nullptr);
}

int32_t ndt3d_search_map_scores(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, float* d_scores) {
  if (!target || !source || !w || !d_scores) return NDT_ERR_INVALID_ARG;
  return search_map_run3(target, source, w, 1, nullptr, nullptr, d_scores);
}

int32_t ndt3d_search_align_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, int32_t k,
                               ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits) {
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = ndt3d_search_map(target, source, w, k, hits, n_hits);
  if (st != NDT_OK || *n_hits < 1) return st;
  // every hit is a start of one map-to-map chain (ndt3d_align_map_multi: bit for bit ndt3d_align_map from each pose)
  return search_hits_align<ndt3d_handle>(hits, *n_hits, [&](const double* poses) {
    ndt3d_handle* sources[ndt::kMaxStarts3];
    std::fill_n(sources, *n_hits, source);
    return ndt3d_align_map_multi(target, sources, poses, *n_hits, results);
  });
}

}  // extern "C"

// Exhaustive pose search for 2D map-to-map alignment (docs/ALGORITHM.md section 2.15): the map-to-map score of
// ndt2d_evaluate_map at every pose of an (x, y, theta) lattice, from the source handle's component list and the target
// handle's covariance records - no points.  Included at the end of ndt2d_api.hip, after ndt2d_search.hpp and
// ndt2d_d2d_api.hpp: the lattice, the peak selection, the scratch, the separation walk and the host run are
// ndt_search.hpp's, the component list and the covariance records ndt_map_host.hpp's.
//
//   k_search_score_d2d  the score volume, in the shape of k_search_score: one workgroup = one heading x a 16 x 16 tile
//                       of translations, ONE LANE PER TRANSLATION, a wave an 8 x 8 block.  What a heading makes uniform
//                       is done once per component while the chunk is staged into LDS: S = R Sigma_i R^T (cos 2t and
//                       sin 2t are the workgroup's).  A lane reads (mu, S) back as a broadcast, forms the image of the
//                       mean with its own translation (image_point's fmaf order: the cell key is the contract's),
//                       gathers its own target record and keeps a private float sum in component order.  No cross-lane
//                       reduction and no atomics: the volume is the same bit for bit on every call.  Per component the
//                       float32 arithmetic is the score part of accumulate_component; only the summation order differs.
#pragma once

#include "ndt2d_d2d.hpp"
#include "ndt_search.hpp"

namespace ndt {

// Source components staged in LDS per round: 20 bytes each ((mu_x, mu_y, Sxx, Sxy) as one float4 and Syy in an array
// of its own, so four components are five broadcast ds_read_b128), 20 KiB per workgroup: eight workgroups per CU by
// LDS (160 KiB), which is the CU's 32 waves.
constexpr int kMapSearchChunk = 1024;

// The score part of accumulate_component (ndt2d_d2d.hpp) with S = (sxx, sxy, syy) already rotated: the same float32
// operations in the same order.
__device__ __forceinline__ float search_component_score(const PoseF& P, const PointRec& r, float sxx, float sxy, float syy) {
  const bool hit = r.B.z > 0.f;
  const float axx = sxx + r.A.z, axy = sxy + r.A.w, ayy = syy + r.B.y;                 // S + Sigma_j (S alone off the map: det > 0)
  const float rdet = __builtin_amdgcn_rcpf(fmaf(axx, ayy, -axy * axy));
  const float bxx = ayy * rdet, bxy = -axy * rdet, byy = axx * rdet;                   // B = (S + Sigma_j)^-1
  const float qx = r.px - r.A.x, qy = r.py - r.A.y;
  const float vx = fmaf(bxx, qx, bxy * qy), vy = fmaf(bxy, qx, byy * qy);
  const float m = fmaf(qx, vx, qy * vy);
  return hit ? __builtin_amdgcn_exp2f(fmaf(P.nhd2, m, P.lg_d1)) : 0.f;
}

// One lattice pose per lane.  cov = the target handle's covariance records, as a kernel argument: the compiler then
// knows it for a global pointer and gathers with global (not flat) loads.  st = the target's static context (its grid
// geometry); comp[2n] = the source's component list.  Axes, tasks and the store: as k_search_score.
__global__ __launch_bounds__(kSearchThreads) void k_search_score_d2d(const AlignStatic* __restrict__ st,
                                                                     const float4* __restrict__ cov, float d1, float d2,
                                                                     const float4* __restrict__ comp, int n,
                                                                     const float* __restrict__ ax, const float* __restrict__ ay,
                                                                     const double* __restrict__ ath, int nx, int ny, int nt,
                                                                     float* __restrict__ out) {
  __shared__ float4 s_ms[kMapSearchChunk];                   // mu_x, mu_y, Sxx, Sxy
  __shared__ float4 s_yy4[kMapSearchChunk / 4];              // Syy of four components
  float* s_yy = reinterpret_cast<float*>(s_yy4);
  const GridDev G = st->grid;
  const int tiles_x = (nx + kSearchTile - 1) / kSearchTile, tiles_y = (ny + kSearchTile - 1) / kSearchTile;
  const long long nblocks = (long long)tiles_x * tiles_y * nt;
  const int tid = threadIdx.x;
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const SearchTask task = search_task(b, tiles_x, tiles_y, nx, ny);
    const int j = task.j, ix = task.ix, iy = task.iy;
    const bool live = task.live;
    double sn_d, cs_d;
    sincos_wrapped(ath[j], &sn_d, &cs_d);
    const PoseF P = make_pose((float)cs_d, (float)sn_d, ax[min(ix, nx - 1)], ay[min(iy, ny - 1)], G.ox, G.oy, G.inv_c, G.W,
                              G.H, d1, d2);
    RotF R;                                                  // as k_iterate_d2d
    R.c2t = P.cs * P.cs - P.sn * P.sn;
    R.s2t = 2.f * P.cs * P.sn;
    float total = 0.f;
    for (int base = 0; base < n; base += kMapSearchChunk) {
      const int m = min(kMapSearchChunk, n - base);
      const int m4 = (m + 3) & ~3;
      __syncthreads();                                   // the previous chunk (or task) has been read by every wave
      for (int k = tid; k < m4; k += kSearchThreads) {
        // image_point's clamp and the rotation of Sigma_i, once per component and heading.  The chunk is padded to a
        // multiple of four with components whose mean sits at the clamp bound (they land on the grid's empty outer
        // ring and score exactly 0) and whose Sigma is the unit matrix (S + 0 keeps a positive determinant), so the
        // loop below needs no tail
        float4 ms = make_float4(1e15f, 1e15f, 1.f, 0.f);
        float syy = 1.f;
        if (k < m) {
          const float4 ca = comp[2 * (size_t)(base + k)], cb = comp[2 * (size_t)(base + k) + 1];
          const float sa = ca.z, sb = ca.w, sc = cb.y;
          const float hm = 0.5f * (sa + sc), hd = 0.5f * (sa - sc);
          const float u = fmaf(hd, R.c2t, -sb * R.s2t);
          ms.x = clamp_coord(ca.x);
          ms.y = clamp_coord(ca.y);
          ms.z = hm + u;
          ms.w = fmaf(hd, R.s2t, sb * R.c2t);
          syy = hm - u;
        }
        s_ms[k] = ms;
        s_yy[k] = syy;
      }
      __syncthreads();
      // two partial sums (even / odd components) per chunk: two independent chains, and short ones for accuracy
      float s0 = 0.f, s1 = 0.f;
      for (int k = 0; k < m4; k += 4) {
        const float4 yy = s_yy4[k >> 2];                                 // broadcast reads: components k .. k + 3
        const float syy[4] = {yy.x, yy.y, yy.z, yy.w};
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
        s0 += search_component_score(P, r[0], c[0].z, c[0].w, syy[0]);
        s1 += search_component_score(P, r[1], c[1].z, c[1].w, syy[1]);
        s0 += search_component_score(P, r[2], c[2].z, c[2].w, syy[2]);
        s1 += search_component_score(P, r[3], c[3].z, c[3].w, syy[3]);
      }
      total += s0 + s1;
    }
    if (live) out[((size_t)j * ny + iy) * nx + ix] = total;
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// The whole map-to-map search (search_host_run) on the TARGET handle's stream and search scratch; the source handle lends
// its component list.  Here: the score launch.
int32_t search_map_run(ndt2d_handle* t, ndt2d_handle* s, const ndt2d_search_window* w, int32_t k, ndt2d_search_hit* hits,
                       int32_t* n_hits, float* d_scores) {
  TraceRange range(d_scores ? "ndt2d_search_map_scores" : "ndt2d_search_map");
  return search_host_run(t, s, w, k, hits, n_hits, d_scores, [&](const SearchPlan& plan, unsigned grid, float* vol) {
    hipLaunchKernelGGL(k_search_score_d2d, dim3(grid), dim3(kSearchThreads), 0, t->stream, t->d_static, (const float4*)t->d_cov,
                       (float)t->prm.d1, (float)t->prm.d2, (const float4*)s->d_comp, s->n_comp, plan.d_x, plan.d_y, plan.d_rot,
                       plan.L.nx, plan.L.ny, plan.L.nt, vol);
  });
}

}  // namespace

extern "C" {

int32_t ndt2d_search_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, int32_t k,
                         ndt2d_search_hit* hits, int32_t* n_hits) {
  if (!target || !source || !w || !hits || !n_hits) return NDT_ERR_INVALID_ARG;
  if (k < 1 || k > kMaxStarts) return NDT_ERR_INVALID_ARG;
  *n_hits = 0;
  return search_map_run(target, source, w, k, hits, n_hits, nullptr);
}

int32_t ndt2d_search_map_scores(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, float* d_scores) {
  if (!target || !source || !w || !d_scores) return NDT_ERR_INVALID_ARG;
  return search_map_run(target, source, w, 1, nullptr, nullptr, d_scores);
}

int32_t ndt2d_search_align_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, int32_t k,
                               ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits) {
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = ndt2d_search_map(target, source, w, k, hits, n_hits);
  if (st != NDT_OK || *n_hits < 1) return st;
  // every hit is a start of one map-to-map chain (ndt2d_align_map_multi: bit for bit ndt2d_align_map from each pose)
  return search_hits_align<ndt2d_handle>(hits, *n_hits, [&](const double* poses) {
    ndt2d_handle* sources[kMaxStarts];
    std::fill_n(sources, *n_hits, source);
    return ndt2d_align_map_multi(target, sources, poses, *n_hits, results);
  });
}

}  // extern "C"

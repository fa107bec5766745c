// Exhaustive 2D pose search over an (x, y, theta) lattice against the cached target grid (docs/ALGORITHM.md
// "Exhaustive pose search").  Included at the end of ndt2d_api.hip: the score kernel and the C ABI.  The lattice, the peak
// selection, the scratch and the separation walk are ndt_search.hpp's, shared with the 3D search.
//
//   k_search_score<NG>  the score volume: one workgroup = one heading x a 16 x 16 tile of translations, ONE LANE PER
//                       TRANSLATION.  The scan is staged through LDS in chunks and read back as a broadcast (every lane
//                       of the wave reads the same point); each lane gathers its own cell record and keeps a private
//                       float sum in point order.  No cross-lane reduction and no atomics: the volume is the same bit
//                       for bit on every call.  Per point the float32 arithmetic is the single-pose path's
//                       (image_point, image_key, the score term of accumulate_point); only the summation order differs.
#pragma once

#include "ndt_search.hpp"

namespace ndt {

constexpr int kSearchChunk = 2048;              // source points staged in LDS per round (16 KB)

// The score term of accumulate_point (ndt2d_kernels.hpp), alone: its hit rule and exponent around the shared mahalanobis2.
__device__ __forceinline__ float search_point_score(const PoseF& P, const PointRec& r) {
  const bool hit = r.B.z > 0.f;
  const float m = mahalanobis2(r);
  return hit ? __builtin_amdgcn_exp2f(fmaf(P.nhd2, m, P.lg_d1)) : 0.f;
}

// One lattice pose per lane.  rec = st->grid.rec, as a kernel argument: the compiler then knows it for a global pointer
// and gathers with global (not flat) loads.  ax[nx], ay[ny]: the translations as float32; ath[nt]: the (wrapped) headings in double.
// Workgroup b covers heading b / tiles and translation tile b % tiles; lanes past the window's edge compute a clamped
// pose and store nothing.
template <int NG>
__global__ __launch_bounds__(kSearchThreads) void k_search_score(const AlignStatic* __restrict__ st, const float4* __restrict__ rec,
                                                                 float d1, float d2,
                                                                 const float* __restrict__ sx, const float* __restrict__ sy,
                                                                 int n, const float* __restrict__ ax,
                                                                 const float* __restrict__ ay, const double* __restrict__ ath,
                                                                 int nx, int ny, int nt, float* __restrict__ out) {
  __shared__ float4 s_pt4[kSearchChunk / 2];                 // kSearchChunk is a multiple of four
  float2* s_pt = reinterpret_cast<float2*>(s_pt4);
  const GridDev G = st->grid;
  const int tiles_x = (nx + kSearchTile - 1) / kSearchTile, tiles_y = (ny + kSearchTile - 1) / kSearchTile;
  const long long nblocks = (long long)tiles_x * tiles_y * nt;
  const int tid = threadIdx.x;
  // (a grid-stride loop over the workgroups' tasks: a lattice of few translations and many headings can need more
  // workgroups than one launch may have threads)
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const SearchTask task = search_task(b, tiles_x, tiles_y, nx, ny);
    const int j = task.j, ix = task.ix, iy = task.iy;
    const bool live = task.live;
    double sn_d, cs_d;
    sincos_wrapped(ath[j], &sn_d, &cs_d);
    const PoseF P = make_pose((float)cs_d, (float)sn_d, ax[min(ix, nx - 1)], ay[min(iy, ny - 1)], G.ox, G.oy, G.inv_c, G.W,
                              G.H, d1, d2);
    const int ncell = G.W * G.H;
    float total = 0.f;
    for (int base = 0; base < n; base += kSearchChunk) {
      const int m = min(kSearchChunk, n - base);
      const int m4 = (m + 3) & ~3;
      __syncthreads();                                   // the previous chunk (or task) has been read by every wave
      for (int k = tid; k < m4; k += kSearchThreads) {
        // image_point's clamp, done once per point here (fmed3 of a clamped value is the value).  The chunk is padded
        // to a multiple of four with points at the clamp bound: they land on the grid's empty outer ring and score
        // exactly 0, so the loop below needs no tail
        float x = 1e15f, y = 1e15f;
        if (k < m) {
          x = clamp_coord(sx[base + k]);
          y = clamp_coord(sy[base + k]);
        }
        s_pt[k] = make_float2(x, y);
      }
      __syncthreads();
      // two partial sums (even / odd points) per chunk: two independent chains, and short ones for accuracy
      float s0 = 0.f, s1 = 0.f;
      for (int k = 0; k < m4; k += 4) {
        const float4 q01 = s_pt4[k >> 1], q23 = s_pt4[(k >> 1) + 1];   // points k .. k + 3 (a broadcast read)
        const float qx[4] = {q01.x, q01.z, q23.x, q23.z}, qy[4] = {q01.y, q01.w, q23.y, q23.w};
        PointRec r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) image_clamped(P, qx[u], qy[u], r[u]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const float ox = NG == 1 ? G.ox : G.gx[g], oy = NG == 1 ? G.oy : G.gy[g];   // as k_iterate<NG>
          // all four gathers in flight before the first is consumed
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int key = g * ncell + image_key(P, ox, oy, r[u], true);
            r[u].A = rec[2 * key];
            r[u].B = rec[2 * key + 1];
          }
          s0 += search_point_score(P, r[0]);
          s1 += search_point_score(P, r[1]);
          s0 += search_point_score(P, r[2]);
          s1 += search_point_score(P, r[3]);
        }
      }
      total += s0 + s1;
    }
    if (live) out[((size_t)j * ny + iy) * nx + ix] = total;
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// The whole search on the handle's stream (search_host_run): the score launch.
int32_t search_run(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w,
                   int32_t k, ndt2d_search_hit* hits, int32_t* n_hits, float* d_scores) {
  TraceRange range(d_scores ? "ndt2d_search_scores" : "ndt2d_search");
  return search_host_run(h, (ndt2d_handle*)nullptr, w, k, hits, n_hits, d_scores, [&](const SearchPlan& plan, unsigned grid, float* vol) {
    const SearchLattice& L = plan.L;
    const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;        // as upload_static
    if (h->prm.overlap_grids == 4)
      hipLaunchKernelGGL(k_search_score<4>, dim3(grid), dim3(kSearchThreads), 0, h->stream, h->d_static,
                         (const float4*)h->grid.rec, d1, d2, d_sx, d_sy, (int)n, plan.d_x, plan.d_y, plan.d_rot, L.nx, L.ny, L.nt, vol);
    else
      hipLaunchKernelGGL(k_search_score<1>, dim3(grid), dim3(kSearchThreads), 0, h->stream, h->d_static,
                         (const float4*)h->grid.rec, d1, d2, d_sx, d_sy, (int)n, plan.d_x, plan.d_y, plan.d_rot, L.nx, L.ny, L.nt, vol);
  });
}

int32_t search_args(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const ndt2d_search_window* w, int32_t k,
                    const void* hits, const int32_t* n_hits) {
  if (!h || !sx || !sy || !w || !hits || !n_hits) return NDT_ERR_INVALID_ARG;
  if (n == 0 || n > kMaxSourcePoints || k < 1 || k > kMaxStarts) return NDT_ERR_INVALID_ARG;
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_search_lattice_size(const ndt2d_search_window* w, int32_t dims[3]) {
  if (!w || !dims) return NDT_ERR_INVALID_ARG;
  SearchWindow v;
  SearchLattice L;
  const int32_t st = search_lattice_of<ndt2d_handle>(w, &v, &L);
  if (st != NDT_OK) return st;
  dims[0] = L.nt; dims[1] = L.ny; dims[2] = L.nx;
  return NDT_OK;
}

int32_t ndt2d_search_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w,
                         int32_t k, ndt2d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = search_args(h, d_sx, d_sy, n, w, k, hits, n_hits);
  if (st != NDT_OK) return st;
  *n_hits = 0;
  return search_run(h, d_sx, d_sy, n, w, k, hits, n_hits, nullptr);
}

int32_t ndt2d_search(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const ndt2d_search_window* w, int32_t k,
                     ndt2d_search_hit* hits, int32_t* n_hits) {
  int32_t st = search_args(h, sx, sy, n, w, k, hits, n_hits);
  if (st != NDT_OK) return st;
  *n_hits = 0;
  { SearchWindow v; SearchLattice L; st = search_lattice_of<ndt2d_handle>(w, &v, &L); if (st != NDT_OK) return st; }
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const s[2] = {sx, sy};
  { const int32_t ss = stage_source(h, s, n); if (ss != NDT_OK) return ss; }
  return ndt2d_search_dev(h, h->d_s[0], h->d_s[1], n, w, k, hits, n_hits);
}

int32_t ndt2d_search_scores_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                const ndt2d_search_window* w, float* d_scores) {
  if (!h || !d_sx || !d_sy || !w || !d_scores || n == 0 || n > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  return search_run(h, d_sx, d_sy, n, w, 1, nullptr, nullptr, d_scores);
}

int32_t ndt2d_search_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w,
                               int32_t k, ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits) {
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = ndt2d_search_dev(h, d_sx, d_sy, n, w, k, hits, n_hits);
  if (st != NDT_OK || *n_hits == 0) return st;
  return search_hits_align<ndt2d_handle>(hits, *n_hits, [&](const double* init) {
    return ndt2d_align_multi_start_dev(h, d_sx, d_sy, n, init, *n_hits, results);
  });
}

}  // extern "C"
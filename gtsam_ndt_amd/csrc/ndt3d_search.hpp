// Exhaustive 3D pose search over an (x, y, yaw) lattice against the cached voxel grid (docs/ALGORITHM.md "Exhaustive 3D
// pose search"); z, roll and pitch are pinned to the window centre's.  Included at the end of ndt2d_api.hip: the score
// kernel and the C ABI.  The lattice, the peak selection, the scratch and the separation walk are ndt_search.hpp's.
//
//   k_search_score3     the score volume, in the shape of k_search_score (ndt2d_search.hpp): one workgroup = one yaw x a
//                       16 x 16 tile of translations, ONE LANE PER TRANSLATION, each wave an 8 x 8 block.  R is uniform
//                       over the workgroup.  The scan is staged through LDS in chunks and read back as broadcasts; each
//                       lane gathers its own voxel record (40 of its 64 bytes) and keeps a private float sum in point
//                       order: no cross-lane reduction, no atomics, the same bits on every call.  Per point the float32
//                       arithmetic is the single-scan chain's, through the functions it calls (image_row3,
//                       mahalanobis3, nhd2_of; ndt3d_kernels.hpp); only the summation order differs, and the voxel key
//                       takes the clamped form (voxel_clamped3) where evaluate_block3 takes voxel_of3's select.
//                       What does not depend on the translation in x and y - the image's z, its inside test in z and
//                       the voxel layer's key (layer_key3) - is computed once per point and workgroup while the chunk
//                       is staged.
#pragma once

#include "ndt_search.hpp"

namespace ndt {

constexpr int kSearch3Chunk = 1024;             // source points staged in LDS per round (16 KB of points + 4 KB of layer keys)

// The score term of accumulate_point3 (ndt3d_kernels.hpp), alone: its hit rule and exponent around the shared mahalanobis3.
__device__ __forceinline__ float search_point_score3(float px, float py, float pz, bool in, const float4& A4, const float4& B4,
                                                     const float2& C2, float d1, float nhd2) {
  const bool hit = in & (A4.w > 0.f);
  const float m = mahalanobis3(px, py, pz, A4, B4, C2);
  return hit ? d1 * __builtin_amdgcn_exp2f(nhd2 * m) : 0.f;
}

__device__ __forceinline__ float search_uniform(float v) {      // a workgroup-uniform float, held in a scalar register
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// One lattice pose per lane.  rec = st->grid.rec, as a kernel argument: the gathers are global (not flat) loads.
// ax[nx], ay[ny]: the translations as float32; ayaw[nt]: the (wrapped) yaws in double; cz, croll, cpitch: the pinned
// coordinates.  Workgroup b covers yaw b / tiles and translation tile b % tiles; lanes past the window's edge compute a
// clamped pose and store nothing.
__global__ __launch_bounds__(kSearchThreads) void k_search_score3(const AlignStatic3* __restrict__ st, const float4* __restrict__ rec,
                                                                  float d1, float d2,
                                                                  const float* __restrict__ sx, const float* __restrict__ sy,
                                                                  const float* __restrict__ sz, int n,
                                                                  const float* __restrict__ ax, const float* __restrict__ ay,
                                                                  const double* __restrict__ ayaw, double cz, double croll,
                                                                  double cpitch, int nx, int ny, int nt, float* __restrict__ out) {
  __shared__ float4 s_pt[kSearch3Chunk];                     // x, y, z and the image's z
  __shared__ int4 s_layer4[kSearch3Chunk / 4];               // key of the image's voxel layer, or -1: outside in z
  int* s_layer = reinterpret_cast<int*>(s_layer4);
  const Grid3Dev G = st->grid;
  const int tiles_x = (nx + kSearchTile - 1) / kSearchTile, tiles_y = (ny + kSearchTile - 1) / kSearchTile;
  const long long nblocks = (long long)tiles_x * tiles_y * nt;
  const int tid = threadIdx.x;
  const Extent3F E = extent3(G);
  const float nhd2 = nhd2_of(d2);
  const int layer = G.W * G.H;
  const unsigned last_cell = (unsigned)(layer * G.D - 1);
  // (a grid-stride loop over the workgroups' tasks, as k_search_score)
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const SearchTask task = search_task(b, tiles_x, tiles_y, nx, ny);
    const int j = task.j, ix = task.ix, iy = task.iy;
    const bool live = task.live;
    const double pose[6] = {0.0, 0.0, cz, croll, cpitch, ayaw[j]};
    const PoseRt3 T = make_rt3(pose);                        // R and tz
    float R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = search_uniform(T.R[q]);
    const float tz = search_uniform(T.tz);
    const float tx = ax[min(ix, nx - 1)], ty = ay[min(iy, ny - 1)];   // the float of the double, as make_rt3's tx
    float total = 0.f;
    for (int base = 0; base < n; base += kSearch3Chunk) {
      const int m = min(kSearch3Chunk, n - base);
      const int m4 = (m + 3) & ~3;
      __syncthreads();                                       // the previous chunk (or task) has been read by every wave
      for (int k = tid; k < m4; k += kSearchThreads) {
        // The chunk is padded to a multiple of four with points that fail the inside test (layer -1): they add exactly 0.
        float x = 0.f, y = 0.f, z = 0.f, pz = 0.f;
        int lk = -1;
        if (k < m) {
          x = sx[base + k]; y = sy[base + k]; z = sz[base + k];
          pz = image_row3(R + 6, tz, x, y, z);
          const Voxel3 L = layer_key3(G, E, pz, (unsigned)layer);
          if (L.in) lk = L.key;
        }
        s_pt[k] = make_float4(x, y, z, pz);
        s_layer[k] = lk;
      }
      __syncthreads();
      // two partial sums (even / odd points) per chunk: two independent chains, and short ones for accuracy
      float s0 = 0.f, s1 = 0.f;
      for (int k = 0; k < m4; k += 4) {
        const int4 l4 = s_layer4[k >> 2];                    // (broadcast reads: every lane reads the same points)
        const int lk[4] = {l4.x, l4.y, l4.z, l4.w};
        float px[4], py[4], pz[4];
        bool in[4];
        float4 A[4], B[4];
        float2 C[4];
        // all four gathers in flight before the first is consumed
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 p = s_pt[k + u];
          px[u] = image_row3(R, tx, p.x, p.y, p.z);
          py[u] = image_row3(R + 3, ty, p.x, p.y, p.z);
          pz[u] = p.w;
          const Voxel3 vox = voxel_clamped3(G, E, Voxel3{lk[u], lk[u] >= 0}, px[u], py[u], last_cell);
          in[u] = vox.in;
          gather_rec3(rec, vox.key, A[u], B[u], C[u]);
        }
        s0 += search_point_score3(px[0], py[0], pz[0], in[0], A[0], B[0], C[0], d1, nhd2);
        s1 += search_point_score3(px[1], py[1], pz[1], in[1], A[1], B[1], C[1], d1, nhd2);
        s0 += search_point_score3(px[2], py[2], pz[2], in[2], A[2], B[2], C[2], d1, nhd2);
        s1 += search_point_score3(px[3], py[3], pz[3], in[3], A[3], B[3], C[3], d1, nhd2);
      }
      total += s0 + s1;
    }
    if (live) out[((size_t)j * ny + iy) * nx + ix] = total;
  }
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

// The whole search on the handle's stream (search_host_run): the score launch, with the pinned coordinates.
int32_t search_run3(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                    const ndt3d_search_window* w3, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits, float* d_scores) {
  using namespace ndt;
  TraceRange range(d_scores ? "ndt3d_search_scores" : "ndt3d_search");
  return search_host_run(h, (ndt3d_handle*)nullptr, w3, k, hits, n_hits, d_scores, [&](const SearchPlan& plan, unsigned grid, float* vol) {
    const SearchLattice& L = plan.L;
    const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;        // as upload_static3
    hipLaunchKernelGGL(k_search_score3, dim3(grid), dim3(kSearchThreads), 0, h->stream, h->d_static, (const float4*)h->grid.rec, d1, d2,
                       d_sx, d_sy, d_sz, (int)n, plan.d_x, plan.d_y, plan.d_rot, w3->center[2], w3->center[3], w3->center[4], L.nx,
                       L.ny, L.nt, vol);
  });
}

int32_t search_args3(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const ndt3d_search_window* w,
                     int32_t k, const void* hits, const int32_t* n_hits) {
  if (!h || !sx || !sy || !sz || !w || !hits || !n_hits) return NDT_ERR_INVALID_ARG;
  if (n == 0 || n > kMaxSourcePoints || k < 1 || k > ndt::kMaxStarts3) return NDT_ERR_INVALID_ARG;
  return single_voxel_only(h);
}

}  // namespace

extern "C" {

int32_t ndt3d_search_lattice_size(const ndt3d_search_window* w, int32_t dims[3]) {
  if (!w || !dims) return NDT_ERR_INVALID_ARG;
  SearchWindow v;
  SearchLattice L;
  const int32_t st = search_lattice_of<ndt3d_handle>(w, &v, &L);
  if (st != NDT_OK) return st;
  dims[0] = L.nt; dims[1] = L.ny; dims[2] = L.nx;
  return NDT_OK;
}

int32_t ndt3d_search_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                         const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = search_args3(h, d_sx, d_sy, d_sz, n, w, k, hits, n_hits);
  if (st != NDT_OK) return st;
  *n_hits = 0;
  return search_run3(h, d_sx, d_sy, d_sz, n, w, k, hits, n_hits, nullptr);
}

int32_t ndt3d_search(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const ndt3d_search_window* w,
                     int32_t k, ndt3d_search_hit* hits, int32_t* n_hits) {
  int32_t st = search_args3(h, sx, sy, sz, n, w, k, hits, n_hits);
  if (st != NDT_OK) return st;
  *n_hits = 0;
  { SearchWindow v; SearchLattice L; st = search_lattice_of<ndt3d_handle>(w, &v, &L); if (st != NDT_OK) return st; }
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  const float* const s[3] = {sx, sy, sz};
  { const int32_t ss = stage_source(h, s, n); if (ss != NDT_OK) return ss; }
  return ndt3d_search_dev(h, h->d_s[0], h->d_s[1], h->d_s[2], n, w, k, hits, n_hits);
}

int32_t ndt3d_search_scores_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                const ndt3d_search_window* w, float* d_scores) {
  if (!h || !d_sx || !d_sy || !d_sz || !w || !d_scores || n == 0 || n > kMaxSourcePoints) return NDT_ERR_INVALID_ARG;
  { const int32_t ns = single_voxel_only(h); if (ns != NDT_OK) return ns; }
  return search_run3(h, d_sx, d_sy, d_sz, n, w, 1, nullptr, nullptr, d_scores);
}

int32_t ndt3d_search_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                               const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, ndt3d_result* results,
                               int32_t* n_hits) {
  if (!results) return NDT_ERR_INVALID_ARG;
  const int32_t st = ndt3d_search_dev(h, d_sx, d_sy, d_sz, n, w, k, hits, n_hits);
  if (st != NDT_OK || *n_hits == 0) return st;
  return search_hits_align<ndt3d_handle>(hits, *n_hits, [&](const double* init) {
    return ndt3d_align_multi_start_dev(h, d_sx, d_sy, d_sz, n, init, *n_hits, results);
  });
}

}  // extern "C"

// Exhaustive 2D pose search over an (x, y, theta) lattice against the cached target grid (docs/ALGORITHM.md
// "Exhaustive pose search").  Included at the end of ndt2d_api.hip: the kernels, the host-side lattice and the C ABI.
//
//   k_search_score<NG>  the score volume: one workgroup = one heading x a 16 x 16 tile of translations, ONE LANE PER
//                       TRANSLATION.  The scan is staged through LDS in chunks and read back as a broadcast (every lane
//                       of the wave reads the same point); each lane gathers its own cell record and keeps a private
//                       float sum in point order.  No cross-lane reduction and no atomics: the volume is the same bit
//                       for bit on every call.  Per point the float32 arithmetic is the single-pose path's
//                       (image_point, image_key, the score term of accumulate_point); only the summation order differs.
//   k_search_peaks      strict 3x3x3 local maxima (ties broken by the lower flat index) -> 64-bit keys
//                       (score bits << 32 | ~index), appended in any order: the selection below is exact on the keys,
//                       so the order of the appends does not matter.
//   k_search_sel_*      radix select of the 4096th largest key, eight passes of eight bits (an LDS histogram per
//                       workgroup, one pick per pass in one workgroup), then the keys at or above it are collected and
//                       sorted (bitonic, one workgroup).  The greedy separation walk runs on the host over the sorted
//                       shortlist (at most 4096 entries).
#pragma once

#include <algorithm>
#include <vector>

namespace ndt {

constexpr int kSearchTile = 16;                 // translations per workgroup edge (16 x 16 = 256 lanes)
constexpr int kSearchThreads = kSearchTile * kSearchTile;
constexpr int kSearchChunk = 2048;              // source points staged in LDS per round (16 KB)
constexpr long long kSearchMaxPoses = 1ll << 25;
constexpr int kSearchShortlist = 4096;
constexpr int kSearchSortThreads = 1024;

// selection state of one search (device memory; the host copies it back whole once the sort is done)
struct SearchSel {
  unsigned long long prefix;        // digits of the threshold key chosen so far
  unsigned long long thresh;        // the shortlist is every key >= thresh
  unsigned int count;               // peaks found (appended by k_search_peaks)
  unsigned int need;                // rank still to find inside the current prefix (0: take every peak)
  unsigned int n_out;               // keys in the shortlist
  unsigned int pad;
  unsigned int hist[256];
  unsigned long long keys[kSearchShortlist];   // the shortlist, sorted descending by k_search_sort
};

// The score term of accumulate_point (ndt2d_kernels.hpp), alone: the same float32 operations in the same order.
__device__ __forceinline__ float search_point_score(const PoseF& P, float px, float py, const float4& A, const float4& B) {
  const bool hit = B.z > 0.f;
  const float a = A.z, b = A.w, c = B.y;
  const float qx = px - A.x, qy = py - A.y;
  const float vx = fmaf(a, qx, b * qy), vy = fmaf(b, qx, c * qy);
  const float m = fmaf(qx, vx, qy * vy);
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
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // (a grid-stride loop over the workgroups' tasks: a lattice of few translations and many headings can need more
  // workgroups than one launch may have threads)
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int j = (int)(b / (tiles_x * tiles_y));
    const int t = (int)(b - (long long)j * tiles_x * tiles_y);
    // a wave is an 8 x 8 block of translations: its lanes look up neighbouring cells
    const int ix = (t % tiles_x) * kSearchTile + (wave & 1) * 8 + (lane & 7);
    const int iy = (t / tiles_x) * kSearchTile + (wave >> 1) * 8 + (lane >> 3);
    const bool live = ix < nx && iy < ny;
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
          x = __builtin_amdgcn_fmed3f(sx[base + k], -1e15f, 1e15f);
          y = __builtin_amdgcn_fmed3f(sy[base + k], -1e15f, 1e15f);
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
        for (int u = 0; u < 4; ++u) {                                  // image_point
          r[u].px = fmaf(P.cs, qx[u], fmaf(-P.sn, qy[u], P.tx));
          r[u].py = fmaf(P.sn, qx[u], fmaf(P.cs, qy[u], P.ty));
        }
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
          s0 += search_point_score(P, r[0].px, r[0].py, r[0].A, r[0].B);
          s1 += search_point_score(P, r[1].px, r[1].py, r[1].A, r[1].B);
          s0 += search_point_score(P, r[2].px, r[2].py, r[2].A, r[2].B);
          s1 += search_point_score(P, r[3].px, r[3].py, r[3].A, r[3].B);
        }
      }
      total += s0 + s1;
    }
    if (live) out[((size_t)j * ny + iy) * nx + ix] = total;
  }
}

// Peaks of the volume: score > 0 and beating every distinct in-window neighbour of the 3x3x3 block (a higher score,
// or the same score and a lower flat index); theta neighbours wrap on a cyclic axis only.  Key = score bits << 32 |
// (0xFFFFFFFF - index): for scores >= 0 its order is (score descending, index ascending).
__global__ __launch_bounds__(256) void k_search_peaks(const float* __restrict__ vol, int nx, int ny, int nt, int cyclic,
                                                      unsigned long long* __restrict__ keys, unsigned int cap,
                                                      SearchSel* __restrict__ sel) {
  const long long N = (long long)nx * ny * nt;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool peak = false;
  float s = 0.f;
  if (idx < N) {
    s = vol[idx];
    peak = s > 0.f;
    const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), j = (int)(idx / ((long long)nx * ny));
    for (int dj = -1; dj <= 1 && peak; ++dj) {
      int jj = j + dj;
      if (cyclic) jj = (jj + nt) % nt;
      else if (jj < 0 || jj >= nt) continue;
      for (int dy = -1; dy <= 1 && peak; ++dy) {
        const int yy = iy + dy;
        if (yy < 0 || yy >= ny) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = ix + dx;
          if (xx < 0 || xx >= nx) continue;
          const long long q = ((long long)jj * ny + yy) * nx + xx;
          if (q == idx) continue;
          const float v = vol[q];
          if (v > s || (v == s && q < idx)) { peak = false; break; }
        }
      }
    }
  }
  // one append per wave: lanes take consecutive slots after the wave's base
  const unsigned long long mask = __ballot(peak);
  if (mask == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  unsigned int base = 0;
  if (lane == leader) base = atomicAdd(&sel->count, (unsigned int)__popcll(mask));
  base = (unsigned int)__shfl((int)base, leader, 64);
  if (peak) {
    const unsigned int slot = base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
    if (slot < cap)                     // cap bounds the peaks of the lattice: never false, kept as a bounds check
      keys[slot] = ((unsigned long long)__float_as_uint(s) << 32) | (0xFFFFFFFFull - (unsigned long long)idx);
  }
}

// before the peaks: zero the count and the histogram
__global__ void k_search_sel_clear(SearchSel* sel) {
  for (int b = threadIdx.x; b < 256; b += blockDim.x) sel->hist[b] = 0u;
  if (threadIdx.x == 0) { sel->count = 0u; sel->n_out = 0u; sel->prefix = 0ull; sel->thresh = 0ull; sel->need = 0u; }
}

// after the peaks: at most kSearchShortlist peaks -> take them all (thresh 0), else find the kSearchShortlist-th key
__global__ void k_search_sel_begin(SearchSel* sel, unsigned int cap) {
  if (threadIdx.x != 0) return;
  const unsigned int c = min(sel->count, cap);
  sel->count = c;
  sel->need = c <= (unsigned int)kSearchShortlist ? 0u : (unsigned int)kSearchShortlist;
}

// pass p: histogram of digit p (bits 56 - 8p .. 63 - 8p) of the keys whose higher digits equal the prefix
__global__ __launch_bounds__(256) void k_search_sel_hist(const unsigned long long* __restrict__ keys, SearchSel* sel, int p) {
  __shared__ unsigned int s_hist[256];
  const unsigned int need = sel->need;
  if (need == 0u) return;                                       // uniform
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned int c = sel->count;
  const int shift = 56 - 8 * p;
  const unsigned long long prefix = sel->prefix;
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < c; i += gridDim.x * blockDim.x) {
    const unsigned long long k = keys[i];
    if (p == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  const unsigned int v = s_hist[threadIdx.x];
  if (v) atomicAdd(&sel->hist[threadIdx.x], v);
}

// pass p: the digit that holds the need-th largest key; the last pass fixes the threshold
__global__ void k_search_sel_pick(SearchSel* sel, int p) {
  if (sel->need == 0u) return;                                  // uniform
  if (threadIdx.x == 0) {
    unsigned int need = sel->need;
    int b = 255;
    for (; b > 0; --b) {
      const unsigned int h = sel->hist[b];
      if (need <= h) break;
      need -= h;
    }
    sel->prefix = (sel->prefix << 8) | (unsigned long long)b;
    if (p == 7) {
      sel->thresh = sel->prefix;
      sel->need = 0u;
    } else {
      sel->need = need;
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 256; b += blockDim.x) sel->hist[b] = 0u;
}

// every key >= thresh into the shortlist (exactly min(count, kSearchShortlist) of them: the keys are distinct)
__global__ __launch_bounds__(256) void k_search_collect(const unsigned long long* __restrict__ keys, SearchSel* sel) {
  const unsigned int c = sel->count;
  const unsigned long long thresh = sel->thresh;
  for (unsigned int i0 = blockIdx.x * blockDim.x; i0 < c; i0 += gridDim.x * blockDim.x) {
    const unsigned int i = i0 + threadIdx.x;
    const unsigned long long k = i < c ? keys[i] : 0ull;
    const bool take = i < c && k >= thresh;
    const unsigned long long mask = __ballot(take);
    if (mask == 0ull) continue;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(&sel->n_out, (unsigned int)__popcll(mask));
    base = (unsigned int)__shfl((int)base, leader, 64);
    if (take) {
      const unsigned int slot = base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
      if (slot < (unsigned int)kSearchShortlist) sel->keys[slot] = k;
    }
  }
}

// the shortlist sorted descending (bitonic over 4096 slots in LDS; empty slots hold 0 and sort last)
__global__ __launch_bounds__(kSearchSortThreads) void k_search_sort(SearchSel* sel) {
  __shared__ unsigned long long s_k[kSearchShortlist];
  const unsigned int n = min(sel->n_out, (unsigned int)kSearchShortlist);
  for (int i = threadIdx.x; i < kSearchShortlist; i += kSearchSortThreads) s_k[i] = (unsigned int)i < n ? sel->keys[i] : 0ull;
  __syncthreads();
  for (int size = 2; size <= kSearchShortlist; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < kSearchShortlist; i += kSearchSortThreads) {
        const int partner = i ^ stride;
        if (partner > i) {
          const bool desc = (i & size) == 0;
          const unsigned long long a = s_k[i], b = s_k[partner];
          if (desc ? (a < b) : (a > b)) { s_k[i] = b; s_k[partner] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < kSearchShortlist; i += kSearchSortThreads) sel->keys[i] = s_k[i];
  if (threadIdx.x == 0) sel->n_out = n;
}

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

constexpr double kSearchPi = 3.141592653589793;

// the lattice of a window (docs/ALGORITHM.md "Exhaustive pose search"); mirrored by gtsam_ndt_amd/search.py lattice()
struct SearchLattice {
  int nx = 0, ny = 0, nt = 0;
  bool cyclic = false;
};

int32_t search_lattice(const ndt2d_search_window* w, SearchLattice* L) {
  if (!w) return NDT_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(w->center[a]) || !std::isfinite(w->half_extent[a]) || !std::isfinite(w->step[a]))
      return NDT_ERR_INVALID_ARG;
    if (!(w->half_extent[a] >= 0.0) || !(w->step[a] > 0.0)) return NDT_ERR_INVALID_ARG;
  }
  if (!std::isfinite(w->min_sep_trans) || !std::isfinite(w->min_sep_rot) || w->min_sep_trans < 0.0 || w->min_sep_rot < 0.0)
    return NDT_ERR_INVALID_ARG;
  double n[3];
  for (int a = 0; a < 3; ++a) n[a] = 2.0 * std::floor(w->half_extent[a] / w->step[a] + 1e-9) + 1.0;
  L->cyclic = w->half_extent[2] >= kSearchPi;
  if (L->cyclic) n[2] = std::max(1.0, std::floor(2.0 * kSearchPi / w->step[2] + 0.5));
  const double lim = (double)kSearchMaxPoses;
  if (n[0] > lim || n[1] > lim || n[2] > lim || n[0] * n[1] * n[2] > lim) {
    set_error("the search window holds more than 2^25 lattice poses");
    return NDT_ERR_CAPACITY;
  }
  L->nx = (int)n[0]; L->ny = (int)n[1]; L->nt = (int)n[2];
  return NDT_OK;
}

// wrap_angle (ndt2d_kernels.hpp) on the host, without contraction: what search.py computes in numpy
double search_wrap(double t) {
#pragma clang fp contract(off)
  if (t > kSearchPi || t <= -kSearchPi) {
    t = t - 2.0 * kSearchPi * std::floor((t + kSearchPi) / (2.0 * kSearchPi));
    if (t <= -kSearchPi) t += 2.0 * kSearchPi;
  }
  return t;
}

// the axes in double: x, y, and the wrapped headings
void search_axes(const ndt2d_search_window* w, const SearchLattice& L, std::vector<double>* ax) {
#pragma clang fp contract(off)
  const int n[3] = {L.nx, L.ny, L.nt};
  for (int a = 0; a < 3; ++a) {
    ax[a].resize(n[a]);
    const int h = (n[a] - 1) / 2;
    for (int i = 0; i < n[a]; ++i) {
      double v;
      if (a == 2 && L.cyclic) v = w->center[2] + (double)i * (2.0 * kSearchPi / (double)n[2]);
      else v = w->center[a] + (double)(i - h) * w->step[a];
      ax[a][i] = a == 2 ? search_wrap(v) : v;
    }
  }
}

// the greedy separation walk over the sorted shortlist
int32_t search_walk(const SearchSel& sel, const std::vector<double>* ax, const SearchLattice& L,
                    const ndt2d_search_window* w, int32_t k, ndt2d_search_hit* hits) {
#pragma clang fp contract(off)
  int32_t m = 0;
  const double st2 = w->min_sep_trans * w->min_sep_trans, sr = w->min_sep_rot;
  for (unsigned int c = 0; c < sel.n_out && m < k; ++c) {
    const unsigned long long key = sel.keys[c];
    const unsigned int bits = (unsigned int)(key >> 32);
    const long long idx = (long long)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    const int ix = (int)(idx % L.nx), iy = (int)((idx / L.nx) % L.ny), j = (int)(idx / ((long long)L.nx * L.ny));
    const double p[3] = {ax[0][ix], ax[1][iy], ax[2][j]};
    bool keep = true;
    for (int32_t q = 0; q < m && keep; ++q) {
      const double dx = p[0] - hits[q].pose[0], dy = p[1] - hits[q].pose[1];
      const double dt = std::fabs(search_wrap(p[2] - hits[q].pose[2]));
      if (dx * dx + dy * dy < st2 && dt < sr) keep = false;
    }
    if (!keep) continue;
    ndt2d_search_hit& hh = hits[m++];
    std::memset(&hh, 0, sizeof(hh));
    for (int a = 0; a < 3; ++a) hh.pose[a] = p[a];
    std::memcpy(&hh.score, &bits, 4);
    hh.index = (int32_t)idx;
  }
  return m;
}

// The whole search on the handle's stream.  d_scores != null: only the volume, into the caller's buffer; else the hits.
int32_t search_run(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w,
                   int32_t k, ndt2d_search_hit* hits, int32_t* n_hits, float* d_scores) {
  TraceRange range(d_scores ? "ndt2d_search_scores" : "ndt2d_search");
  SearchLattice L;
  { const int32_t ls = search_lattice(w, &L); if (ls != NDT_OK) return ls; }
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish_chunk_run(h); if (fs != NDT_OK) return fs; }
  std::vector<double> ax[3];
  search_axes(w, L, ax);
  const size_t N = (size_t)L.nx * L.ny * L.nt;
  // axes on the device: headings (double) | x (float) | y (float)
  const size_t axes_bytes = 8 * (size_t)L.nt + 4 * ((size_t)L.nx + L.ny);
  HIP_TRY(grow(&h->d_srch_axes, &h->srch_axes_cap, axes_bytes, axes_bytes + axes_bytes / 4));
  HIP_TRY(hipStreamSynchronize(h->stream));          // the pinned buffer's last copy has left it
  HIP_TRY(grow({grow_buf(&h->h_srch_axes)}, &h->h_srch_axes_cap, axes_bytes, axes_bytes + axes_bytes / 4, nullptr, /*pinned=*/true));
  double* hth = reinterpret_cast<double*>(h->h_srch_axes);
  float* hx = reinterpret_cast<float*>(hth + L.nt);
  float* hy = hx + L.nx;
  for (int j = 0; j < L.nt; ++j) hth[j] = ax[2][j];
  for (int i = 0; i < L.nx; ++i) hx[i] = (float)ax[0][i];          // translation: the float of the double, as k_begin
  for (int i = 0; i < L.ny; ++i) hy[i] = (float)ax[1][i];
  HIP_TRY(hipMemcpyAsync(h->d_srch_axes, h->h_srch_axes, axes_bytes, hipMemcpyHostToDevice, h->stream));
  const double* dth = reinterpret_cast<const double*>(h->d_srch_axes);
  const float* dx = reinterpret_cast<const float*>(dth + L.nt);
  const float* dy = dx + L.nx;

  float* vol = d_scores;
  if (!vol) {
    HIP_TRY(grow(&h->d_srch_vol, &h->srch_vol_cap, N, N + N / 4));
    vol = h->d_srch_vol;
  }
  const long long tiles = (long long)((L.nx + kSearchTile - 1) / kSearchTile) * ((L.ny + kSearchTile - 1) / kSearchTile);
  const long long tasks = tiles * L.nt;
  const unsigned grid = (unsigned)std::min<long long>(tasks, 1ll << 20);
  const float d1 = (float)h->prm.d1, d2 = (float)h->prm.d2;        // as upload_static
  if (h->prm.overlap_grids == 4)
    hipLaunchKernelGGL(k_search_score<4>, dim3(grid), dim3(kSearchThreads), 0, h->stream, h->d_static,
                       (const float4*)h->grid.rec, d1, d2, d_sx, d_sy, (int)n, dx, dy, dth, L.nx, L.ny, L.nt, vol);
  else
    hipLaunchKernelGGL(k_search_score<1>, dim3(grid), dim3(kSearchThreads), 0, h->stream, h->d_static,
                       (const float4*)h->grid.rec, d1, d2, d_sx, d_sy, (int)n, dx, dy, dth, L.nx, L.ny, L.nt, vol);
  HIP_TRY(hipGetLastError());
  if (d_scores) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return NDT_OK;
  }

  // peaks: at most one in every 2 x 2 x 2 block of the lattice (two neighbours cannot both beat each other)
  const size_t cap = (size_t)((L.nx + 1) / 2) * ((L.ny + 1) / 2) * ((L.nt + 1) / 2);
  HIP_TRY(grow(&h->d_srch_keys, &h->srch_keys_cap, cap, cap + cap / 4));
  if (!h->d_srch_sel) HIP_TRY(hipMalloc((void**)&h->d_srch_sel, sizeof(SearchSel)));
  if (!h->h_srch_sel) HIP_TRY(pinned_alloc(&h->h_srch_sel, sizeof(SearchSel)));
  SearchSel* sel = h->d_srch_sel;
  const unsigned hb = (unsigned)std::min<size_t>(std::max<size_t>((cap + 255) / 256, 1), 1024);
  hipLaunchKernelGGL(k_search_sel_clear, dim3(1), dim3(256), 0, h->stream, sel);
  hipLaunchKernelGGL(k_search_peaks, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (const float*)vol, L.nx, L.ny,
                     L.nt, L.cyclic ? 1 : 0, h->d_srch_keys, (unsigned)cap, sel);
  hipLaunchKernelGGL(k_search_sel_begin, dim3(1), dim3(64), 0, h->stream, sel, (unsigned)cap);
  for (int p = 0; p < 8; ++p) {
    hipLaunchKernelGGL(k_search_sel_hist, dim3(hb), dim3(256), 0, h->stream, (const unsigned long long*)h->d_srch_keys, sel, p);
    hipLaunchKernelGGL(k_search_sel_pick, dim3(1), dim3(64), 0, h->stream, sel, p);
  }
  hipLaunchKernelGGL(k_search_collect, dim3(hb), dim3(256), 0, h->stream, (const unsigned long long*)h->d_srch_keys, sel);
  hipLaunchKernelGGL(k_search_sort, dim3(1), dim3(kSearchSortThreads), 0, h->stream, sel);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_srch_sel, sel, sizeof(SearchSel), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *n_hits = search_walk(*h->h_srch_sel, ax, L, w, k, hits);
  return NDT_OK;
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
  SearchLattice L;
  const int32_t st = search_lattice(w, &L);
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
  { SearchLattice L; st = search_lattice(w, &L); if (st != NDT_OK) return st; }
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t ss = stage_source(h, sx, sy, n); if (ss != NDT_OK) return ss; }
  return ndt2d_search_dev(h, h->d_sx, h->d_sy, n, w, k, hits, n_hits);
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
  std::vector<double> init(3 * (size_t)*n_hits);
  for (int32_t q = 0; q < *n_hits; ++q)
    for (int a = 0; a < 3; ++a) init[3 * q + a] = hits[q].pose[a];
  return ndt2d_align_multi_start_dev(h, d_sx, d_sy, n, init.data(), *n_hits, results);
}

}  // extern "C"

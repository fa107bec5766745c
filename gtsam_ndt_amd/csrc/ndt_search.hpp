// What the exhaustive pose searches of the 2D and the 3D handle share (docs/ALGORITHM.md "Exhaustive pose search"):
// the window's lattice, peak selection on a score volume [n_rot][n_y][n_x], the scratch a handle keeps for a search and
// the host's separation walk.  The score kernels are per dimension (ndt2d_search.hpp, ndt3d_search.hpp); everything
// here works on any volume of that layout.
//
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

#include "ndt_chain_host.hpp"

namespace ndt {

constexpr int kSearchTile = 16;                 // translations per workgroup edge (16 x 16 = 256 lanes)
constexpr int kSearchThreads = kSearchTile * kSearchTile;
constexpr long long kSearchMaxPoses = 1ll << 25;
constexpr int kSearchShortlist = 4096;
constexpr int kSearchSortThreads = 1024;

// The lattice pose of a lane of the score kernels.  Workgroup task b covers rotation j = b / tiles and translation tile
// b % tiles (tiles = tiles_x tiles_y); a wave is an 8 x 8 block of translations, so that its lanes look up neighbouring
// cells.  A lane past the window's edge is not live: it computes a clamped pose and stores nothing.
struct SearchTask {
  int j, tile_x, tile_y;            // uniform over the workgroup: the rotation and the tile's first translation
  int ix, iy;                       // the lane's translation
  bool live;
};
__device__ __forceinline__ SearchTask search_task(long long b, int tiles_x, int tiles_y, int nx, int ny) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long tiles = (long long)tiles_x * tiles_y;
  const int j = (int)(b / tiles);
  const int t = (int)(b - j * tiles);
  const int tile_x = (t % tiles_x) * kSearchTile, tile_y = (t / tiles_x) * kSearchTile;
  const int ix = tile_x + (wave & 1) * 8 + (lane & 7);
  const int iy = tile_y + (wave >> 1) * 8 + (lane >> 3);
  return SearchTask{j, tile_x, tile_y, ix, iy, ix < nx && iy < ny};
}

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

// The search scratch of a handle, allocated on first use and grown on demand; release() in the handle's destroy.
struct SearchScratch {
  float* d_vol = nullptr; size_t vol_cap = 0;                      // the score volume
  unsigned long long* d_keys = nullptr; size_t keys_cap = 0;      // peak keys
  unsigned char* d_axes = nullptr; size_t axes_cap = 0;           // the lattice's axes
  SearchSel* d_sel = nullptr;                                     // selection state and shortlist
  unsigned char* h_axes = nullptr; size_t h_axes_cap = 0;         // pinned: the axes' upload
  SearchSel* h_sel = nullptr;                                     // pinned: the shortlist's read-back
  // a pose list (ndt_score_poses.hpp): d_vol holds its scores, d_keys its candidates' keys
  double* d_list = nullptr; size_t list_cap = 0;                  // a host list's upload (doubles)
  double* d_pick = nullptr;                                       // the shortlisted poses [kSearchShortlist][6]
  double* h_pick = nullptr;                                       // pinned: their read-back
  unsigned int* d_cnt = nullptr; size_t cnt_cap = 0;              // a host list's hit counts (ndt_score_map_poses.hpp)
  void release() {
    void* dev[] = {d_vol, d_keys, d_axes, d_sel, d_list, d_pick, d_cnt};
    for (void* p : dev) if (p) (void)hipFree(p);
    void* host[] = {h_axes, h_sel, h_pick};
    for (void* p : host) if (p) (void)hipHostFree(p);
    *this = SearchScratch{};
  }
};

}  // namespace ndt

// ------------------------------------------------------------------------------ host side
namespace {

constexpr double kSearchPi = 3.141592653589793;

// A window over the three searched axes (x, y, rotation): the 2D window as it is, the 3D window's x, y and yaw.
struct SearchWindow {
  double center[3], half_extent[3], step[3];
  double min_sep_trans, min_sep_rot;
};

// the lattice of a window (docs/ALGORITHM.md "Exhaustive pose search"); mirrored by gtsam_ndt_amd/search.py lattice()
struct SearchLattice {
  int nx = 0, ny = 0, nt = 0;
  bool cyclic = false;
};

// one hit of the separation walk: the searched axes' values, the lattice score and the flat index
struct SearchPeak {
  double pose[3];
  float score;
  int32_t index;
};

int32_t search_lattice(const SearchWindow& w, SearchLattice* L) {
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(w.center[a]) || !std::isfinite(w.half_extent[a]) || !std::isfinite(w.step[a]))
      return NDT_ERR_INVALID_ARG;
    if (!(w.half_extent[a] >= 0.0) || !(w.step[a] > 0.0)) return NDT_ERR_INVALID_ARG;
  }
  if (!std::isfinite(w.min_sep_trans) || !std::isfinite(w.min_sep_rot) || w.min_sep_trans < 0.0 || w.min_sep_rot < 0.0)
    return NDT_ERR_INVALID_ARG;
  double n[3];
  for (int a = 0; a < 3; ++a) n[a] = 2.0 * std::floor(w.half_extent[a] / w.step[a] + 1e-9) + 1.0;
  L->cyclic = w.half_extent[2] >= kSearchPi;
  if (L->cyclic) n[2] = std::max(1.0, std::floor(2.0 * kSearchPi / w.step[2] + 0.5));
  const double lim = (double)ndt::kSearchMaxPoses;
  if (n[0] > lim || n[1] > lim || n[2] > lim || n[0] * n[1] * n[2] > lim) {
    ndt::set_error("the search window holds more than 2^25 lattice poses");
    return NDT_ERR_CAPACITY;
  }
  L->nx = (int)n[0]; L->ny = (int)n[1]; L->nt = (int)n[2];
  return NDT_OK;
}

// the axes in double: x, y, and the wrapped rotations (ndt_pose.hpp's wrap_angle, on the host without contraction: what
// search.py computes in numpy)
void search_axes(const SearchWindow& w, const SearchLattice& L, std::vector<double>* ax) {
#pragma clang fp contract(off)
  const int n[3] = {L.nx, L.ny, L.nt};
  for (int a = 0; a < 3; ++a) {
    ax[a].resize(n[a]);
    const int h = (n[a] - 1) / 2;
    for (int i = 0; i < n[a]; ++i) {
      double v;
      if (a == 2 && L.cyclic) v = w.center[2] + (double)i * (2.0 * kSearchPi / (double)n[2]);
      else v = w.center[a] + (double)(i - h) * w.step[a];
      ax[a][i] = a == 2 ? ndt::wrap_angle(v) : v;
    }
  }
}

// the greedy separation walk over the sorted shortlist
int32_t search_walk(const ndt::SearchSel& sel, const std::vector<double>* ax, const SearchLattice& L, const SearchWindow& w,
                    int32_t k, SearchPeak* hits) {
#pragma clang fp contract(off)
  int32_t m = 0;
  const double st2 = w.min_sep_trans * w.min_sep_trans, sr = w.min_sep_rot;
  for (unsigned int c = 0; c < sel.n_out && m < k; ++c) {
    const unsigned long long key = sel.keys[c];
    const unsigned int bits = (unsigned int)(key >> 32);
    const long long idx = (long long)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    const int ix = (int)(idx % L.nx), iy = (int)((idx / L.nx) % L.ny), j = (int)(idx / ((long long)L.nx * L.ny));
    const double p[3] = {ax[0][ix], ax[1][iy], ax[2][j]};
    bool keep = true;
    for (int32_t q = 0; q < m && keep; ++q) {
      const double dx = p[0] - hits[q].pose[0], dy = p[1] - hits[q].pose[1];
      const double dt = std::fabs(ndt::wrap_angle(p[2] - hits[q].pose[2]));
      if (dx * dx + dy * dy < st2 && dt < sr) keep = false;
    }
    if (!keep) continue;
    SearchPeak& hh = hits[m++];
    for (int a = 0; a < 3; ++a) hh.pose[a] = p[a];
    std::memcpy(&hh.score, &bits, 4);
    hh.index = (int32_t)idx;
  }
  return m;
}

// The lattice of a search on a stream: its axes on the host (double) and on the device, where the score kernel reads them
// (rotations in double, translations as the float of the double, as k_begin / k_begin3 round a pose's translation).
struct SearchPlan {
  SearchLattice L;
  std::vector<double> ax[3];
  const double* d_rot = nullptr;
  const float *d_x = nullptr, *d_y = nullptr;
  size_t poses() const { return (size_t)L.nx * L.ny * L.nt; }
  long long tasks() const {     // workgroups' tasks of a score kernel: one rotation x one tile of translations each
    return (long long)((L.nx + ndt::kSearchTile - 1) / ndt::kSearchTile) * ((L.ny + ndt::kSearchTile - 1) / ndt::kSearchTile) * L.nt;
  }
};

// the axes of plan->L to the device (enqueued on `stream`; plan->L is set)
int32_t search_upload_axes(ndt::SearchScratch& s, hipStream_t stream, const SearchWindow& w, SearchPlan* plan) {
  using namespace ndt;
  const SearchLattice& L = plan->L;
  search_axes(w, L, plan->ax);
  // axes on the device: rotations (double) | x (float) | y (float)
  const size_t axes_bytes = 8 * (size_t)L.nt + 4 * ((size_t)L.nx + L.ny);
  HIP_TRY(grow(&s.d_axes, &s.axes_cap, axes_bytes, axes_bytes + axes_bytes / 4));
  HIP_TRY(hipStreamSynchronize(stream));          // the pinned buffer's last copy has left it
  HIP_TRY(grow({grow_buf(&s.h_axes)}, &s.h_axes_cap, axes_bytes, axes_bytes + axes_bytes / 4, nullptr, /*pinned=*/true));
  double* hth = reinterpret_cast<double*>(s.h_axes);
  float* hx = reinterpret_cast<float*>(hth + L.nt);
  float* hy = hx + L.nx;
  for (int j = 0; j < L.nt; ++j) hth[j] = plan->ax[2][j];
  for (int i = 0; i < L.nx; ++i) hx[i] = (float)plan->ax[0][i];
  for (int i = 0; i < L.ny; ++i) hy[i] = (float)plan->ax[1][i];
  HIP_TRY(hipMemcpyAsync(s.d_axes, s.h_axes, axes_bytes, hipMemcpyHostToDevice, stream));
  plan->d_rot = reinterpret_cast<const double*>(s.d_axes);
  plan->d_x = reinterpret_cast<const float*>(plan->d_rot + L.nt);
  plan->d_y = plan->d_x + L.nx;
  return NDT_OK;
}

// where a score kernel writes the volume: the caller's buffer, else the scratch's (grown to hold it)
int32_t search_volume(ndt::SearchScratch& s, size_t N, float* d_scores, float** vol) {
  *vol = d_scores;
  if (d_scores) return NDT_OK;
  HIP_TRY(ndt::grow(&s.d_vol, &s.vol_cap, N, N + N / 4));
  *vol = s.d_vol;
  return NDT_OK;
}

// The selection of a search or of a pose list (ndt_score_poses.hpp) in two halves round the caller's key kernel.
// First: room for `cap` keys and the selection state, cleared (enqueued on `stream`).
int32_t search_keys_begin(ndt::SearchScratch& s, hipStream_t stream, size_t cap) {
  using namespace ndt;
  HIP_TRY(grow(&s.d_keys, &s.keys_cap, cap, cap + cap / 4));
  if (!s.d_sel) HIP_TRY(hipMalloc((void**)&s.d_sel, sizeof(SearchSel)));
  if (!s.h_sel) HIP_TRY(pinned_alloc(&s.h_sel, sizeof(SearchSel)));
  hipLaunchKernelGGL(k_search_sel_clear, dim3(1), dim3(256), 0, stream, s.d_sel);
  return NDT_OK;
}

// Then: the keys appended since (at most cap) -> the shortlist in s.d_sel, sorted (enqueued on `stream`).
void search_keys_shortlist(ndt::SearchScratch& s, hipStream_t stream, size_t cap) {
  using namespace ndt;
  SearchSel* sel = s.d_sel;
  const unsigned hb = (unsigned)std::min<size_t>(std::max<size_t>((cap + 255) / 256, 1), 1024);
  hipLaunchKernelGGL(k_search_sel_begin, dim3(1), dim3(64), 0, stream, sel, (unsigned)cap);
  for (int p = 0; p < 8; ++p) {
    hipLaunchKernelGGL(k_search_sel_hist, dim3(hb), dim3(256), 0, stream, (const unsigned long long*)s.d_keys, sel, p);
    hipLaunchKernelGGL(k_search_sel_pick, dim3(1), dim3(64), 0, stream, sel, p);
  }
  hipLaunchKernelGGL(k_search_collect, dim3(hb), dim3(256), 0, stream, (const unsigned long long*)s.d_keys, sel);
  hipLaunchKernelGGL(k_search_sort, dim3(1), dim3(kSearchSortThreads), 0, stream, sel);
}

// Peaks of the volume -> shortlist -> the host's walk: hits[0 .. *n_hits), best first.  Synchronous.
int32_t search_select(ndt::SearchScratch& s, hipStream_t stream, const float* vol, const SearchPlan& plan, const SearchWindow& w,
                      int32_t k, SearchPeak* hits, int32_t* n_hits) {
  using namespace ndt;
  const SearchLattice& L = plan.L;
  const size_t N = plan.poses();
  // peaks: at most one in every 2 x 2 x 2 block of the lattice (two neighbours cannot both beat each other)
  const size_t cap = (size_t)((L.nx + 1) / 2) * ((L.ny + 1) / 2) * ((L.nt + 1) / 2);
  { const int32_t bs = search_keys_begin(s, stream, cap); if (bs != NDT_OK) return bs; }
  SearchSel* sel = s.d_sel;
  hipLaunchKernelGGL(k_search_peaks, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, vol, L.nx, L.ny, L.nt, L.cyclic ? 1 : 0,
                     s.d_keys, (unsigned)cap, sel);
  search_keys_shortlist(s, stream, cap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s.h_sel, sel, sizeof(SearchSel), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *n_hits = search_walk(*s.h_sel, plan.ax, L, w, k, hits);
  return NDT_OK;
}

// What differs between the dimensions in the host code both handles share, specialised next to each handle
// (ndt2d_api.hip, ndt3d_api.hpp).  Here: Window and Hit (the ABI's), kPose, kMaxStarts, window (the searched axes of a
// Window) and hits_out (the walk's peaks as the ABI's hits).  Declared in ndt_chain_host.hpp, with finish (waits for the
// alignment in flight).

// (ndt_map_host.hpp) what a map-to-map call refuses and prepares before it enqueues anything
template <class H> int32_t prepare_single_voxel_map_pair(H* t, H* s, const char* who);

// The lattice of an ABI window; *w = its searched axes.  Every centre coordinate has to be finite, the pinned ones too.
template <class H>
int32_t search_lattice_of(const typename HandleTraits<H>::Window* win, SearchWindow* w, SearchLattice* L) {
  if (!win) return NDT_ERR_INVALID_ARG;
  for (int a = 0; a < HandleTraits<H>::kPose; ++a)
    if (!std::isfinite(win->center[a])) return NDT_ERR_INVALID_ARG;
  *w = HandleTraits<H>::window(*win);
  return search_lattice(*w, L);
}

// The whole search on t's stream and search scratch.  s = null: of a scan; else of s's component list (a map-to-map
// search: s lends the list, and nothing reads it any more on return).  launch(plan, grid, vol) enqueues the score kernel
// on t's stream: `grid` workgroups, the volume into vol.  d_scores != null: only the volume, into the caller's buffer;
// else the hits.
template <class H, class Launch>
int32_t search_host_run(H* t, H* s, const typename HandleTraits<H>::Window* win, int32_t k,
                        typename HandleTraits<H>::Hit* hits, int32_t* n_hits, float* d_scores, Launch&& launch) {
  using T = HandleTraits<H>;
  SearchWindow w;
  SearchPlan plan;
  { const int32_t ls = search_lattice_of<H>(win, &w, &plan.L); if (ls != NDT_OK) return ls; }
  if (s) {
    const int32_t ps = prepare_single_voxel_map_pair(t, s, "search");
    if (ps != NDT_OK) return ps;
  } else {
    if (!t->has_target) return NDT_ERR_NO_TARGET;
    HIP_TRY(hipSetDevice(t->device));
    { const int32_t fs = finish(t); if (fs != NDT_OK) return fs; }
  }
  { const int32_t us = search_upload_axes(t->srch, t->stream, w, &plan); if (us != NDT_OK) return us; }
  float* vol = nullptr;
  { const int32_t vs = search_volume(t->srch, plan.poses(), d_scores, &vol); if (vs != NDT_OK) return vs; }
  launch(plan, (unsigned)std::min<long long>(plan.tasks(), 1ll << 20), vol);
  HIP_TRY(hipGetLastError());
  if (d_scores) {
    HIP_TRY(hipStreamSynchronize(t->stream));
    return NDT_OK;
  }
  SearchPeak peaks[T::kMaxStarts];
  { const int32_t ss = search_select(t->srch, t->stream, vol, plan, w, k, peaks, n_hits); if (ss != NDT_OK) return ss; }
  T::hits_out(peaks, *n_hits, *win, hits);
  return NDT_OK;
}

// The hits of a search as the start poses of one multi call: align(poses) gets them as [n_hits][kPose].
template <class H, class Align>
int32_t search_hits_align(const typename HandleTraits<H>::Hit* hits, int32_t n_hits, Align&& align) {
  constexpr int P = HandleTraits<H>::kPose;
  double poses[HandleTraits<H>::kMaxStarts][P];
  for (int32_t q = 0; q < n_hits; ++q)
    for (int j = 0; j < P; ++j) poses[q][j] = hits[q].pose[j];
  return align(&poses[0][0]);
}

}  // namespace

// A scan's points scored one by one against the cached grid, and those that fit kept (included behind ndt_merge.hpp: one
// translation unit; docs/ALGORITHM.md section 2.19).  Every other entry point returns sums over the scan;
// these write what the sums are made of - m_i = q' Sigma^-1 q of point i in its cell, with the float32 operations of the
// single-scan alignment by calling its device functions (image_point / image_key / mahalanobis2 in 2D; make_rot3,
// image3, voxel_of3 and mahalanobis3 in 3D) -
// and a class per point, and copy the points of the wanted classes to the front of an output cloud in their order.
//
// Three kernels, ordered by their boundaries alone (the rule of ndt2d_kernels.hpp for the chain: no tickets, no atomics
// that decide a position, no fences):
//   k_point_fit     tile t = points [t kFitTile, (t + 1) kFitTile): m, class, and the tile's four class counts as one
//                   plain 16-byte store into table[t]
//   k_point_scan    one workgroup: base[t] = kept points in the tiles before t, in tile order
//   k_point_select  tile t again: ranks its kept points (ballot + mbcnt in the wave, wave counts through LDS, a running
//                   base per round of 256) and copies coordinates and indices to base[t] + rank
// All of it is integer bookkeeping on per-point results, so every output is the same to the bit from run to run.
#pragma once
#include <type_traits>

namespace ndt {

constexpr int kFitRounds = 4;                       // rounds of kBlock points per workgroup
constexpr int kFitTile = kBlock * kFitRounds;       // 1024 points per tile

enum : unsigned int { kPointInvalid = 0, kPointMiss = 1, kPointMisfit = 2, kPointFit = 3 };

template <int DIM> struct FitGrid { using type = GridDev; };
template <> struct FitGrid<3> { using type = Grid3Dev; };

// By value: every field is read with a constant index and stays in scalar registers.
template <int DIM>
struct FitArgs {
  typename FitGrid<DIM>::type grid;
  const float* s[3];               // the scan (s[2] is null in 2D)
  double pose[DIM == 2 ? 3 : 6];
  unsigned int n;                  // <= kMaxSourcePoints < 2^31
  float max_m;
  float* m;                        // [n] or null
  unsigned char* cls;              // [n]
  uint4* table;                    // [tiles]: (n_invalid, n_miss, n_misfit, n_fit) of each tile
};

template <int DIM>
struct SelectArgs {
  const unsigned int* s[3];        // the scan's words: coordinates are copied as bits
  unsigned int* o[3];
  unsigned int* index;             // [n] or null
  const unsigned char* cls;
  const unsigned int* base;        // [tiles]
  unsigned int n, keep;
};

// 2D: hit and m of one image point over the NG grids - the lookup of the chain's body (ndt2d_iterate_text.hpp) and
// accumulate_point's mahalanobis2; the least m of the grids whose cell is valid.
template <int NG>
__device__ __forceinline__ bool fit_point2(const PoseF& P, const GridDev& G, float x, float y, float& m_out) {
  PointRec r;
  image_point(P, x, y, r);
  const int ncell = G.W * G.H;
  bool hit = false;
  float best = INFINITY;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const int key = q * ncell + image_key(P, G.gx[q], G.gy[q], r, true);
    r.A = G.rec[2 * key];
    r.B = G.rec[2 * key + 1];
    const bool valid = r.B.z > 0.f;
    const float m = mahalanobis2(r);
    if (valid && (!hit || m < best)) best = m;
    hit |= valid;
  }
  m_out = best;
  return hit;
}

// 3D: hit and m of one point through the chain's functions: image3, voxel_of3, the record loads, mahalanobis3
__device__ __forceinline__ bool fit_point3(const Rot3F& T, const Grid3Dev& G, float x, float y, float z, float& m_out) {
  const V3 p = image3(T.R, T.tx, T.ty, T.tz, x, y, z);
  const Voxel3 vox = voxel_of3(G, extent3(G), p.x, p.y, p.z);
  const int key = vox.key;
  const float4 A4 = G.rec[4 * key];
  const float4 B4 = G.rec[4 * key + 1];
  const float4 C2 = G.rec[4 * key + 2];
  m_out = mahalanobis3(p.x, p.y, p.z, A4, B4, C2);
  return vox.in & (A4.w > 0.f);
}

template <int DIM, int NG>
__global__ __launch_bounds__(kBlock) void k_point_fit(FitArgs<DIM> a) {
  __shared__ unsigned int s_cnt[kBlock / 64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int first = blockIdx.x * (unsigned int)kFitTile + tid;       // < 2^31 + kFitTile: no wrap
  // the tile's coordinates, all requested before anything waits: round r of a wave is 64 consecutive floats per axis
  float x[kFitRounds], y[kFitRounds], z[kFitRounds];
#pragma unroll
  for (int r = 0; r < kFitRounds; ++r) {
    const unsigned int i = first + r * kBlock;
    const bool live = i < a.n;
    x[r] = live ? a.s[0][i] : 0.f;
    y[r] = live ? a.s[1][i] : 0.f;
    z[r] = (DIM == 3 && live) ? a.s[2][i] : 0.f;
  }
  // the pose as the chain forms it: angles wrapped (k_begin*), then float32 of the float64 sincos
  PoseF P;
  Rot3F T;
  if constexpr (DIM == 2) {
    double sn_d, cs_d;
    sincos_wrapped(wrap_angle(a.pose[2]), &sn_d, &cs_d);
    P = make_pose((float)cs_d, (float)sn_d, (float)a.pose[0], (float)a.pose[1], a.grid.ox, a.grid.oy, a.grid.inv_c, a.grid.W,
                  a.grid.H, 1.f, 1.f);
  } else {
    const double pose[6] = {a.pose[0], a.pose[1], a.pose[2], wrap_angle(a.pose[3]), wrap_angle(a.pose[4]), wrap_angle(a.pose[5])};
    make_rot3(pose, T);
  }
  unsigned int cnt[4] = {0u, 0u, 0u, 0u};             // of the wave, the same in every lane
#pragma unroll
  for (int r = 0; r < kFitRounds; ++r) {
    const unsigned int i = first + r * kBlock;
    const bool live = i < a.n;
    // (a dead lane carries the origin through the same code: its key is clamped or tested like any other)
    bool finite, hit;
    float m;
    if constexpr (DIM == 2) {
      finite = isfinite(x[r]) && isfinite(y[r]);
      hit = fit_point2<NG>(P, a.grid, x[r], y[r], m);
    } else {
      finite = isfinite(x[r]) && isfinite(y[r]) && isfinite(z[r]);
      hit = fit_point3(T, a.grid, x[r], y[r], z[r], m);
    }
    unsigned int c = kPointInvalid;
    if (finite) c = !hit ? kPointMiss : (m <= a.max_m ? kPointFit : kPointMisfit);
    if (live) {
      if (a.m) a.m[i] = c >= kPointMisfit ? m : (c == kPointMiss ? INFINITY : NAN);
      a.cls[i] = (unsigned char)c;
    }
#pragma unroll
    for (unsigned int k = 0; k < 4; ++k) cnt[k] += (unsigned int)__popcll(__ballot(live & (c == k)));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cnt[wave][k] = cnt[k];
  }
  __syncthreads();
  if (tid == 0) {
    uint4 t;
    t.x = ((s_cnt[0][0] + s_cnt[1][0]) + s_cnt[2][0]) + s_cnt[3][0];
    t.y = ((s_cnt[0][1] + s_cnt[1][1]) + s_cnt[2][1]) + s_cnt[3][1];
    t.z = ((s_cnt[0][2] + s_cnt[1][2]) + s_cnt[2][2]) + s_cnt[3][2];
    t.w = ((s_cnt[0][3] + s_cnt[1][3]) + s_cnt[2][3]) + s_cnt[3][3];
    a.table[blockIdx.x] = t;
  }
}

// the kept points of a tile under a mask of 1 << class
__device__ __forceinline__ unsigned int kept_of(const uint4& t, unsigned int keep) {
  return ((keep & 1u) ? t.x : 0u) + ((keep & 2u) ? t.y : 0u) + ((keep & 4u) ? t.z : 0u) + ((keep & 8u) ? t.w : 0u);
}

// One workgroup walks the table in tile order, kBlock tiles a trip: an inclusive scan in each wave (six shuffle steps),
// the waves' totals through LDS, a running base.  2M tiles (a scan of 2^31 points) are 8k trips.
__global__ __launch_bounds__(kBlock) void k_point_scan(const uint4* __restrict__ table, unsigned int tiles, unsigned int keep,
                                                        unsigned int* __restrict__ base) {
  __shared__ unsigned int s_w[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned int run = 0u;
  for (unsigned int t0 = 0u; t0 < tiles; t0 += kBlock) {          // (the same in every lane)
    const unsigned int t = t0 + tid;
    const unsigned int v = t < tiles ? kept_of(table[t], keep) : 0u;
    unsigned int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned int u = (unsigned int)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned int off = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const unsigned int c = s_w[w];
      off += w < wave ? c : 0u;
      total += c;
    }
    if (t < tiles) base[t] = run + off + (inc - v);
    run += total;
    __syncthreads();                                              // s_w is rewritten by the next trip
  }
}

template <int DIM>
__global__ __launch_bounds__(kBlock) void k_point_select(SelectArgs<DIM> a) {
  __shared__ unsigned int s_w[kFitRounds][kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int first = blockIdx.x * (unsigned int)kFitTile + tid;
  unsigned int c[kFitRounds];
#pragma unroll
  for (int r = 0; r < kFitRounds; ++r) {
    const unsigned int i = first + r * kBlock;
    c[r] = i < a.n ? (unsigned int)a.cls[i] : 4u;                 // class 4: a dead lane, in no mask
  }
  unsigned int run = a.base[blockIdx.x];
  unsigned int rank[kFitRounds];
#pragma unroll
  for (int r = 0; r < kFitRounds; ++r) {
    const bool kept = (a.keep >> c[r]) & 1u;
    const unsigned long long mask = __ballot(kept);
    rank[r] = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    if (lane == 0) s_w[r][wave] = (unsigned int)__popcll(mask);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kFitRounds; ++r) {
    unsigned int off = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const unsigned int n_w = s_w[r][w];
      off += w < wave ? n_w : 0u;
      total += n_w;
    }
    if ((a.keep >> c[r]) & 1u) {                                  // (a live lane: i < n, and pos <= i)
      const unsigned int i = first + r * kBlock;
      const unsigned int pos = run + off + rank[r];
#pragma unroll
      for (int d = 0; d < DIM; ++d) a.o[d][pos] = a.s[d][i];
      if (a.index) a.index[pos] = i;
    }
    run += total;
  }
}

}  // namespace ndt

namespace {

// ---- what differs per dimension ----
void fit_grid(const ndt2d_handle* h, ndt::FitArgs<2>* a) { a->grid = h->grid; }
void fit_grid(const ndt3d_handle* h, ndt::FitArgs<3>* a) { a->grid = h->grid; }
void launch_point_fit(ndt2d_handle* h, unsigned tiles, const ndt::FitArgs<2>& a) {
  if (h->grid.ngrid == 4) hipLaunchKernelGGL((ndt::k_point_fit<2, 4>), dim3(tiles), dim3(kBlock), 0, h->stream, a);
  else hipLaunchKernelGGL((ndt::k_point_fit<2, 1>), dim3(tiles), dim3(kBlock), 0, h->stream, a);
}
void launch_point_fit(ndt3d_handle* h, unsigned tiles, const ndt::FitArgs<3>& a) {
  hipLaunchKernelGGL((ndt::k_point_fit<3, 1>), dim3(tiles), dim3(ndt::kBlock), 0, h->stream, a);
}
// a host scan into the handle's staging arrays (as ndt*_evaluate stages its scan)
template <class H>
int32_t fit_stage(H* h, const float* const* s, size_t n, const float** d) {
  const int32_t ss = stage_source(h, s, n);
  for (int a = 0; a < 3; ++a) d[a] = a < HandleTraits<H>::kDim ? h->d_s[a] : nullptr;
  return ss;
}

// The argument checks of every entry point, in the order the header lists them.  d_o: the output cloud of a selection
// (null: a fit call, which takes no mask).
template <class H>
int32_t point_fit_check(const H* h, const char* who, const float* const* s, size_t n, const double* pose, float max_m,
                        uint32_t keep, float* const* d_o, const ndt_point_fit* fit) {
  using T = HandleTraits<H>;
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  auto bad = [&](const char* what) { ndt::last_error() = std::string(who) + ": " + what; return NDT_ERR_INVALID_ARG; };
  if (!h) return bad("the handle is null");
  for (int a = 0; a < DIM; ++a) if (!s[a]) return bad("a coordinate array of the scan is null");
  if (!pose) return bad("the pose is null");
  if (!fit) return bad("fit is null");
  if (n == 0) return bad("the scan is empty");
  if (n > kMaxSourcePoints) return bad("the scan holds more points than an alignment takes");
  for (int i = 0; i < T::kPose; ++i) if (!std::isfinite(pose[i])) return bad("the pose is not finite");
  if (!(max_m >= 0.f)) return bad("max_m is NaN or negative");
  if (d_o) {
    if (keep == 0 || keep > 15) return bad("keep is not a mask of 1 << class (1 .. 15)");
    for (int a = 0; a < DIM; ++a) if (!d_o[a]) return bad("a coordinate array of the output is null");
  }
  if (!h->has_target) { ndt::last_error() = std::string(who) + ": the handle holds no target"; return NDT_ERR_NO_TARGET; }
  return single_voxel_only(h, who);
}

// ndt*_fit_points_dev (d_o null) and ndt*_select_points_dev
template <class H>
int32_t point_fit_impl(H* h, const char* who, const float* const* d_s, size_t n, const double* pose, float max_m, uint32_t keep,
                       float* d_m, uint8_t* d_class, float* const* d_o, uint32_t* d_index, ndt_point_fit* fit) {
  using namespace ndt;
  using T = HandleTraits<H>;
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  { const int32_t cs = point_fit_check(h, who, d_s, n, pose, max_m, keep, d_o, fit); if (cs != NDT_OK) return cs; }
  std::memset(fit, 0, sizeof(*fit));
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  PointFitScratch& S = h->fit;
  const size_t tiles = (n + kFitTile - 1) / kFitTile;
  auto no_memory = [&]() {
    (void)hipGetLastError();
    last_error() = std::string(who) + ": the scratch cannot grow";
    return NDT_ERR_ALLOC;
  };
  if (!d_class) {
    if (grow(&S.d_cls, &S.cls_cap, n, n + n / 4 + 1024) != hipSuccess) return no_memory();
    d_class = S.d_cls;
  }
  if (grow({grow_buf(&S.d_table), grow_buf(&S.d_base)}, &S.tile_cap, tiles, tiles + tiles / 4 + 64) != hipSuccess) return no_memory();
  {
    bool grew = false;
    if (grow({grow_buf(&S.h_table)}, &S.h_cap, tiles, tiles + tiles / 4 + 64, &grew, /*pinned=*/true) != hipSuccess) return no_memory();
    if (grew) std::memset(S.h_table, 0, S.h_cap * sizeof(uint4));
  }
  FitArgs<DIM> a{};
  fit_grid(h, &a);
  for (int d = 0; d < DIM; ++d) a.s[d] = d_s[d];
  for (int i = 0; i < T::kPose; ++i) a.pose[i] = pose[i];
  a.n = (unsigned int)n;
  a.max_m = max_m;
  a.m = d_m;
  a.cls = d_class;
  a.table = S.d_table;
  launch_point_fit(h, (unsigned)tiles, a);
  HIP_TRY(hipGetLastError());
  if (d_o) {
    hipLaunchKernelGGL(k_point_scan, dim3(1), dim3(kBlock), 0, h->stream, (const uint4*)S.d_table, (unsigned)tiles, keep, S.d_base);
    HIP_TRY(hipGetLastError());
    SelectArgs<DIM> b{};
    for (int d = 0; d < DIM; ++d) {
      b.s[d] = reinterpret_cast<const unsigned int*>(d_s[d]);
      b.o[d] = reinterpret_cast<unsigned int*>(d_o[d]);
    }
    b.index = d_index;
    b.cls = d_class;
    b.base = S.d_base;
    b.n = (unsigned int)n;
    b.keep = keep;
    hipLaunchKernelGGL((k_point_select<DIM>), dim3((unsigned)tiles), dim3(kBlock), 0, h->stream, b);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(S.h_table, S.d_table, tiles * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (size_t t = 0; t < tiles; ++t) {
    const uint4 e = S.h_table[t];
    fit->n_invalid += e.x; fit->n_miss += e.y; fit->n_misfit += e.z; fit->n_fit += e.w;
  }
  if (d_o)
    fit->n_selected = ((keep & 1u) ? fit->n_invalid : 0) + ((keep & 2u) ? fit->n_miss : 0) + ((keep & 4u) ? fit->n_misfit : 0) +
                      ((keep & 8u) ? fit->n_fit : 0);
  return NDT_OK;
}

// ndt*_fit_points: host arrays in and out
template <class H>
int32_t point_fit_host(H* h, const char* who, const float* const* s, size_t n, const double* pose, float max_m, float* m,
                       uint8_t* cls, ndt_point_fit* fit) {
  using namespace ndt;
  { const int32_t cs = point_fit_check(h, who, s, n, pose, max_m, 0, nullptr, fit); if (cs != NDT_OK) return cs; }
  HIP_TRY(hipSetDevice(h->device));
  const float* d_s[3];
  { const int32_t ss = fit_stage(h, s, n, d_s); if (ss != NDT_OK) return ss; }
  PointFitScratch& S = h->fit;
  if (m && grow(&S.d_m, &S.m_cap, n, n + n / 4 + 1024) != hipSuccess) {
    (void)hipGetLastError();
    last_error() = std::string(who) + ": the scratch cannot grow";
    return NDT_ERR_ALLOC;
  }
  const int32_t st = point_fit_impl(h, who, d_s, n, pose, max_m, 0, m ? S.d_m : nullptr, nullptr, nullptr, nullptr, fit);
  if (st != NDT_OK) return st;
  if (m) HIP_TRY(hipMemcpyAsync(m, S.d_m, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (cls) HIP_TRY(hipMemcpyAsync(cls, S.d_cls, n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_fit_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3], float max_m,
                             float* d_m, uint8_t* d_class, ndt_point_fit* fit) {
  TraceRange range("ndt2d_fit_points");
  const float* s[3] = {d_sx, d_sy, nullptr};
  return point_fit_impl(h, "ndt2d_fit_points_dev", s, n, pose, max_m, 0, d_m, d_class, nullptr, nullptr, fit);
}
int32_t ndt2d_fit_points(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double pose[3], float max_m, float* m,
                         uint8_t* cls, ndt_point_fit* fit) {
  TraceRange range("ndt2d_fit_points");
  const float* s[3] = {sx, sy, nullptr};
  return point_fit_host(h, "ndt2d_fit_points", s, n, pose, max_m, m, cls, fit);
}
int32_t ndt2d_select_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3], float max_m,
                                uint32_t keep, float* d_ox, float* d_oy, uint32_t* d_index, ndt_point_fit* fit) {
  TraceRange range("ndt2d_select_points");
  const float* s[3] = {d_sx, d_sy, nullptr};
  float* o[3] = {d_ox, d_oy, nullptr};
  return point_fit_impl(h, "ndt2d_select_points_dev", s, n, pose, max_m, keep, nullptr, nullptr, o, d_index, fit);
}
int32_t ndt3d_fit_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double pose[6],
                             float max_m, float* d_m, uint8_t* d_class, ndt_point_fit* fit) {
  TraceRange range("ndt3d_fit_points");
  const float* s[3] = {d_sx, d_sy, d_sz};
  return point_fit_impl(h, "ndt3d_fit_points_dev", s, n, pose, max_m, 0, d_m, d_class, nullptr, nullptr, fit);
}
int32_t ndt3d_fit_points(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const double pose[6],
                         float max_m, float* m, uint8_t* cls, ndt_point_fit* fit) {
  TraceRange range("ndt3d_fit_points");
  const float* s[3] = {sx, sy, sz};
  return point_fit_host(h, "ndt3d_fit_points", s, n, pose, max_m, m, cls, fit);
}
int32_t ndt3d_select_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                const double pose[6], float max_m, uint32_t keep, float* d_ox, float* d_oy, float* d_oz,
                                uint32_t* d_index, ndt_point_fit* fit) {
  TraceRange range("ndt3d_select_points");
  const float* s[3] = {d_sx, d_sy, d_sz};
  float* o[3] = {d_ox, d_oy, d_oz};
  return point_fit_impl(h, "ndt3d_select_points_dev", s, n, pose, max_m, keep, nullptr, nullptr, o, d_index, fit);
}

}  // extern "C"

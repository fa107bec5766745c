// One submap folded into another at a pose, from the per-cell sums alone (included behind ndt_coarsen.hpp: one translation
// unit; docs/ALGORITHM.md section 2.18).  All points of a source cell are moved rigidly and filed as a block under the
// destination cell of their mean: an exact identity on the raw moments, evaluated in float64 in ONE fixed operation order
// (no contraction) and rounded to integers once per sum, so the contribution is a pure function of (source sums, pose,
// destination geometry).  Adding it with integer atomics commutes bit for bit, and subtracting it (SIGN = -1) with the same
// arguments is the exact inverse whatever happened to the destination in between.  What global-map assembly from submaps
// that came back from ndt*_load_map needs: such a map has no points to add.
#pragma once
#include <type_traits>

namespace ndt {

// Both geometries, the pose and its rotation, by value: every field is read with a constant index, so the block stays in
// scalar registers.
struct MergeArgs {
  const void* src;             // sums of src's grid 0 [sD][sH][sW]
  void* dst;                   // sums of dst's grid [dD][dH][dW]
  unsigned long long* counts;  // [0] += the points dropped outside dst, [1] += the points filed
  int sW, sH, sD, ring;        // ring = 1: dst's outermost ring of cells counts as outside (2D)
  int dW, dH, dD;
  int chunk;                   // cells per thread of the compaction, 1 .. kMergeChunk
  float s_org[3], d_org[3];
  float d_inv_c, padf;
  double s_cell, d_cell, s_fix, d_fix;   // cell sizes and 2^22 / cell size
  double k, kk;                // c_s / c_d and its square: src units -> dst units
  double R[9], t[3];           // row-major with stride 3 (2D: the third row and column are zero)
};

constexpr int kMergeThreads = 256;
constexpr int kMergeChunk = 8;          // most cells per thread of the compaction: a workgroup scans up to 2048 cells at a time

// ((R[r][0] v0 + R[r][1] v1) [+ R[r][2] v2]), every operation rounded separately
template <int DIM>
__device__ __forceinline__ double merge_row(const double* R, int r, double v0, double v1, double v2) {
#pragma clang fp contract(off)
  double acc = R[3 * r] * v0 + R[3 * r + 1] * v1;
  if (DIM == 3) acc = acc + R[3 * r + 2] * v2;
  return acc;
}

// Steps 1-3 of section 2.18 for one source cell c at grid index idx: false when the block lands outside dst, else the
// destination cell and the integers to add.
template <int DIM>
__device__ __forceinline__ bool merge_contribution(const MergeArgs& a, const CoarsenSums<DIM>& c, const int* idx, size_t* cell,
                                                   long long* dS, long long* dSS) {
#pragma clang fp contract(off)
  const double dn = (double)c.n;
  double e[3] = {0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    e[i] = cell_centre(a.s_org[i], idx[i], a.s_cell);
    S[i] = (double)c.s[i];
    mu[i] = e[i] + S[i] / (dn * a.s_fix);
  }
  // 1. the mean's image and its cell under dst's own float32 binning rule
  int j[3] = {0, 0, 0};
  bool in = true;
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    const float p = (float)(merge_row<DIM>(a.R, r, mu[0], mu[1], mu[2]) + a.t[r]);
    const float f = (p - a.d_org[r]) * a.d_inv_c;
    const int ext = r == 0 ? a.dW : (r == 1 ? a.dH : a.dD);
    const float lo = a.ring ? 1.f : 0.f, hi = (float)(ext - a.ring);
    in = in & (f >= lo) & (f < hi);                 // (a NaN fails both)
    j[r] = (int)f;
  }
  if (!in) return false;
  *cell = ((size_t)j[2] * a.dH + j[1]) * a.dW + j[0];
  // 2. the source centre's image from the destination cell's centre, and the sums turned into dst's frame and units
  double av[3] = {0.0, 0.0, 0.0}, rv[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    const double re = merge_row<DIM>(a.R, r, e[0], e[1], e[2]) + a.t[r];
    av[r] = (re - cell_centre(a.d_org[r], j[r], a.d_cell)) * a.d_fix;
    rv[r] = a.k * merge_row<DIM>(a.R, r, S[0], S[1], S[2]);
  }
  double M[3][3] = {};
  {
    int p = 0;
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int m = i; m < DIM; ++m, ++p) { M[i][m] = (double)c.ss[p]; M[m][i] = M[i][m]; }
  }
  double T[3][3] = {};                              // R SS
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int m = 0; m < DIM; ++m) T[r][m] = merge_row<DIM>(a.R, r, M[0][m], M[1][m], M[2][m]);
  // 3. the contribution, rounded half to even
  int p = 0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    dS[i] = llrint(dn * av[i] + rv[i]);
#pragma unroll
    for (int m = i; m < DIM; ++m, ++p) {
      const double q = a.kk * merge_row<DIM>(a.R, m, T[i][0], T[i][1], T[i][2]);     // k^2 (R SS R^T)[i][m]
      dSS[p] = llrint((((dn * av[i]) * av[m] + av[i] * rv[m]) + av[m] * rv[i]) + q);
    }
  }
  // the roundings can leave n dSS_aa < dS_a^2, which no point set has: the least dSS_aa that has it (as k_coarsen)
  p = 0;
#pragma unroll
  for (int i = 0; i < DIM; p += DIM - i, ++i) {
    const __int128 sq = (__int128)dS[i] * dS[i];
    if ((__int128)c.n * dSS[p] < sq) dSS[p] = ceil_div_u128((unsigned __int128)sq, c.n);
  }
  return true;
}

// One thread per cell of src's grid 0, grid-stride.  Most cells of a submap are empty (nine in ten of the config-3 map's), and the
// float64 work of a block is some 1 500 instructions whatever the number of live lanes, so a workgroup first compacts the
// occupied cells of a.chunk x 256 consecutive cells into a list in LDS (empty cells leave there, after one 4-byte
// load) and then works the list off with dense waves (the host picks the chunk so that a large grid still
// spreads over the chip and a small one is not left to a handful of workgroups).  The
// block's sums go to the destination cell with the atomics k_accumulate issues per point (one count and five or nine
// 64-bit sums), here per source cell: collisions are the normal case when src is finer than dst, and integer adds make
// their order - and the order of the list - irrelevant.  The dropped and the filed point counts are summed per wave and
// added by one lane.
template <int DIM, int SIGN>
__global__ __launch_bounds__(kMergeThreads) void k_merge(MergeArgs a) {
  using Cell = CoarsenSums<DIM>;
  constexpr int NP = DIM * (DIM + 1) / 2;
  __shared__ unsigned int s_list[kMergeThreads * kMergeChunk];
  const unsigned int kPer = kMergeThreads * (unsigned int)a.chunk;
  __shared__ unsigned int s_count;
  const unsigned int total = (unsigned int)a.sW * (unsigned int)a.sH * (unsigned int)a.sD;     // <= 2^27
  const Cell* const src = static_cast<const Cell*>(a.src);
  Cell* const dst = static_cast<Cell*>(a.dst);
  unsigned long long outside = 0ull, filed = 0ull;
  for (unsigned int base = blockIdx.x * kPer; base < total; base += gridDim.x * kPer) {        // (the same in every lane of the workgroup)
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    unsigned int nn[kMergeChunk];
#pragma unroll
    for (int u = 0; u < kMergeChunk; ++u) {
      const unsigned int k = base + u * kMergeThreads + threadIdx.x;
      nn[u] = (u < a.chunk && k < total) ? src[k].n : 0u;       // (constant indices: nn stays in registers)
    }
#pragma unroll
    for (int u = 0; u < kMergeChunk; ++u)
      if (nn[u] != 0u && nn[u] <= kMaxCellCount) s_list[atomicAdd(&s_count, 1u)] = base + u * kMergeThreads + threadIdx.x;   // < kPer entries
    __syncthreads();
    const unsigned int count = s_count;
    for (unsigned int i = threadIdx.x; i < count; i += kMergeThreads) {
      const unsigned int k = s_list[i];
      const Cell c = src[k];
      const unsigned int n = c.n;
      const unsigned int w = (unsigned int)a.sW, h = (unsigned int)a.sH;
      const int idx[3] = {(int)(k % w), (int)((k / w) % h), (int)(k / (w * h))};
      size_t cell = 0;
      long long dS[DIM], dSS[NP];
      if (!merge_contribution<DIM>(a, c, idx, &cell, dS, dSS)) { outside += n; continue; }
      filed += n;
      Cell* d = dst + cell;
      atomicAdd(&d->n, SIGN > 0 ? n : 0u - n);
#pragma unroll
      for (int q = 0; q < DIM; ++q) atomicAdd((unsigned long long*)&d->s[q], signed_term<SIGN>((unsigned long long)dS[q]));
#pragma unroll
      for (int p = 0; p < NP; ++p) atomicAdd((unsigned long long*)&d->ss[p], signed_term<SIGN>((unsigned long long)dSS[p]));
    }
    __syncthreads();                                       // the list has been read
  }
  // (every lane comes here: the loops have no early return)
  if (__ballot(outside != 0ull)) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) outside += __shfl_xor(outside, m);
    if ((threadIdx.x & 63) == 0) atomicAdd(&a.counts[0], outside);
  }
  if (__ballot(filed != 0ull)) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) filed += __shfl_xor(filed, m);
    if ((threadIdx.x & 63) == 0) atomicAdd(&a.counts[1], filed);
  }
}

}  // namespace ndt

namespace {

// The rotation and translation of a pose in float64, formed here and handed to the kernel by value so that there is one
// right answer: cos / sin from libm, then in 3D the nine products of R = Rz Ry Rx in the host form of ndt_pose.hpp, every
// operation rounded separately.
template <int DIM>
void merge_rotation(const double* pose, double* R, double* t) {
  for (int i = 0; i < 9; ++i) R[i] = 0.0;
  if (DIM == 2) {
    const double c = std::cos(pose[2]), s = std::sin(pose[2]);
    R[0] = c; R[1] = -s; R[3] = s; R[4] = c;
    t[0] = pose[0]; t[1] = pose[1]; t[2] = 0.0;
  } else {
    ndt::rot3_products(std::sin(pose[3]), std::cos(pose[3]), std::sin(pose[4]), std::cos(pose[4]), std::sin(pose[5]),
                       std::cos(pose[5]), R);
    t[0] = pose[0]; t[1] = pose[1]; t[2] = pose[2];
  }
}

// ---- what differs per dimension ----
void merge_geometry(const ndt2d_handle* s, const ndt2d_handle* d, ndt::MergeArgs* a) {
  const GridDev &gs = s->grid, &gd = d->grid;
  a->src = gs.acc; a->dst = gd.acc;
  a->sW = gs.W; a->sH = gs.H; a->sD = 1; a->ring = 1;
  a->dW = gd.W; a->dH = gd.H; a->dD = 1;
  a->s_org[0] = gs.gx[0]; a->s_org[1] = gs.gy[0]; a->s_org[2] = 0.f;
  a->d_org[0] = gd.gx[0]; a->d_org[1] = gd.gy[0]; a->d_org[2] = 0.f;
  a->d_inv_c = gd.inv_c;
  a->s_cell = gs.cell; a->d_cell = gd.cell; a->s_fix = gs.fix_scale; a->d_fix = gd.fix_scale;
}
void merge_geometry(const ndt3d_handle* s, const ndt3d_handle* d, ndt::MergeArgs* a) {
  const ndt::Grid3Dev &gs = s->grid, &gd = d->grid;
  a->src = gs.acc; a->dst = gd.acc;
  a->sW = gs.W; a->sH = gs.H; a->sD = gs.D; a->ring = 0;
  a->dW = gd.W; a->dH = gd.H; a->dD = gd.D;
  a->s_org[0] = gs.ox; a->s_org[1] = gs.oy; a->s_org[2] = gs.oz;
  a->d_org[0] = gd.ox; a->d_org[1] = gd.oy; a->d_org[2] = gd.oz;
  a->d_inv_c = gd.inv_c;
  a->s_cell = gs.cell; a->d_cell = gd.cell; a->s_fix = gs.fix_scale; a->d_fix = gd.fix_scale;
}
void merge_grid_changed(ndt2d_handle* h) { grid_changed(h); }
void merge_grid_changed(ndt3d_handle* h) { grid_changed3(h); }
// the signed finalise of every cell of the grid, counting into h->d_counters (k_finalise / k_finalise3, as finalise_grid launches them)
void launch_merge_finalise(ndt2d_handle* h, int sign) {
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.ngrid;
  const dim3 blocks((unsigned)((ncell + kBlock - 1) / kBlock));
  if (sign < 0) hipLaunchKernelGGL((k_finalise<-1>), blocks, dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points, h->prm.eig_ratio, h->d_counters);
  else hipLaunchKernelGGL((k_finalise<1>), blocks, dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points, h->prm.eig_ratio, h->d_counters);
}
void launch_merge_finalise(ndt3d_handle* h, int sign) {
  using namespace ndt;
  const size_t ncell = (size_t)h->grid.W * h->grid.H * h->grid.D;
  const auto finalise = sign < 0 ? &k_finalise3<-1> : &k_finalise3<1>;
  hipLaunchKernelGGL(finalise, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->grid, h->prm.min_points,
                     h->prm.eig_ratio, h->d_counters);
}
void merge_count_points(ndt2d_handle* h, unsigned long long filed, int sign) {
  if (sign < 0) h->n_points -= (size_t)filed; else h->n_points += (size_t)filed;
}
void merge_count_points(ndt3d_handle*, unsigned long long, int) {}          // (not tracked in 3D)
int32_t merge_upload(ndt2d_handle* h) { return upload_static(h); }
int32_t merge_upload(ndt3d_handle* h) { return upload_static3(h); }

// ndt*_merge_map (sign = 1) and ndt*_unmerge_map (sign = -1)
template <class H>
int32_t merge_map_impl(H* dst, H* src, const double* pose, size_t* n_outside, int sign) {
  using namespace ndt;
  using T = HandleTraits<H>;
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  const char* who = sign < 0 ? "unmerge_map" : "merge_map";
  if (n_outside) *n_outside = 0;
  if (!dst || !src || !pose) { last_error() = std::string(who) + ": a handle or the pose is null"; return NDT_ERR_INVALID_ARG; }
  if (src == dst) { last_error() = std::string(who) + ": source and destination are one handle"; return NDT_ERR_INVALID_ARG; }
  if (src->device != dst->device) { last_error() = std::string(who) + ": both handles must live on one device"; return NDT_ERR_INVALID_ARG; }
  if (src->prm.overlap_grids == 4 || dst->prm.overlap_grids == 4) {
    last_error() = std::string(who) + " does not take overlapping grids";
    return NDT_ERR_INVALID_ARG;
  }
  if (src->prm.cell_size > dst->prm.cell_size) {
    last_error() = std::string(who) + ": the source's cell_size exceeds the destination's (a wider Gaussian cannot be filed under one cell)";
    return NDT_ERR_INVALID_ARG;
  }
  for (int i = 0; i < T::kPose; ++i)
    if (!std::isfinite(pose[i])) { last_error() = std::string(who) + ": the pose is not finite"; return NDT_ERR_INVALID_ARG; }
  if (!src->has_target || !dst->has_target) { last_error() = std::string(who) + ": a handle holds no target"; return NDT_ERR_NO_TARGET; }
  HIP_TRY(hipSetDevice(dst->device));
  { const int32_t fs = finish(src); if (fs != NDT_OK) return fs; }
  { const int32_t fs = finish(dst); if (fs != NDT_OK) return fs; }
  merge_grid_changed(dst);
  MergeArgs a{};
  merge_geometry(src, dst, &a);
  a.k = a.s_cell / a.d_cell;
  a.kk = a.k * a.k;
  merge_rotation<DIM>(pose, a.R, a.t);
  // one fill, the merge, the signed finalise of every cell, one copy: the counter shards, the broken-cell word and the
  // merge's two counts travel together
  a.counts = reinterpret_cast<unsigned long long*>(dst->d_counters + kCountMerge);
  static_assert(kCountMerge % 2 == 0 && kCountAlloc * sizeof(int) <= kSmallFlagByte, "64-bit counts; the read-back stays in front of the flag");
  HIP_TRY(order_after(dst->stream, src->stream, &src->map_ev));             // src's sums may still be in flight on its stream
  HIP_TRY(hipMemsetAsync(dst->d_counters, 0, kCountAlloc * sizeof(int), dst->stream));
  const size_t total = (size_t)a.sW * a.sH * a.sD;
  a.chunk = 1;                                                              // two workgroups per CU before the lists get longer
  while (a.chunk < kMergeChunk && total / ((size_t)kMergeThreads * a.chunk) > 512) a.chunk *= 2;
  size_t blocks = (total + (size_t)kMergeThreads * a.chunk - 1) / ((size_t)kMergeThreads * a.chunk);
  if (blocks > 2048) blocks = 2048;
  if (sign < 0) hipLaunchKernelGGL((k_merge<DIM, -1>), dim3((unsigned)blocks), dim3(kMergeThreads), 0, dst->stream, a);
  else hipLaunchKernelGGL((k_merge<DIM, 1>), dim3((unsigned)blocks), dim3(kMergeThreads), 0, dst->stream, a);
  HIP_TRY(hipGetLastError());
  launch_merge_finalise(dst, sign);
  HIP_TRY(hipGetLastError());
  int* hc = static_cast<int*>(dst->h_small);
  dst->has_target = false;                                                  // until the counts say that all is well
  HIP_TRY(hipMemcpyAsync(hc, dst->d_counters, kCountAlloc * sizeof(int), hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));                               // src is free on return
  const unsigned long long* hcnt = reinterpret_cast<const unsigned long long*>(hc + kCountMerge);
  if (n_outside) *n_outside = (size_t)hcnt[0];
  int n_valid_sum = 0, n_over_sum = 0;
  sum_count_shards(hc, &n_valid_sum, &n_over_sum);
  dst->n_valid = n_valid_sum;
  if (sign < 0 && hc[kCountUnder] > 0) {
    set_error("unmerge_map: the source map at this pose is not in the destination: a cell's count fell below zero, or reached zero with sums left");
    return NDT_ERR_INVALID_ARG;
  }
  if (n_over_sum > 0) { set_error("a target cell holds more than 2^20 points"); return NDT_ERR_CAPACITY; }
  dst->has_target = true;
  merge_count_points(dst, hcnt[1], sign);
  return merge_upload(dst);
}

}  // namespace

extern "C" {

int32_t ndt2d_merge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside) {
  TraceRange range("ndt2d_merge_map");
  return merge_map_impl(dst, src, pose, n_outside, 1);
}
int32_t ndt2d_unmerge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside) {
  TraceRange range("ndt2d_unmerge_map");
  return merge_map_impl(dst, src, pose, n_outside, -1);
}
int32_t ndt3d_merge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside) {
  TraceRange range("ndt3d_merge_map");
  return merge_map_impl(dst, src, pose, n_outside, 1);
}
int32_t ndt3d_unmerge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside) {
  TraceRange range("ndt3d_unmerge_map");
  return merge_map_impl(dst, src, pose, n_outside, -1);
}

}  // extern "C"

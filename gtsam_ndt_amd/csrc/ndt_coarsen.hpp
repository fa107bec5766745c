// A coarser submap from a submap's exact sums (included behind ndt_map_io.hpp: one translation unit): the cells of
// dst's grid are unions of f x f (x f) cells of src's, f = 2 or 4, and their fixed-point sums follow from the children's
// by integer arithmetic alone (docs/ALGORITHM.md section 2.17) - no points, deterministic to the bit.  What a pyramid
// level of a submap that came back from ndt*_load_map needs.
#pragma once
#include "ndt_coarsen_geom.hpp"

namespace ndt {

// CellAcc (DIM = 2: sx sy | sxx sxy syy) and CellAcc3 (DIM = 3: s[3] | xx xy xz yy yz zz) under one name
template <int DIM> struct CoarsenSums {
  long long s[DIM];
  long long ss[DIM * (DIM + 1) / 2];
  unsigned int n, pad;
};
static_assert(sizeof(CoarsenSums<2>) == sizeof(CellAcc) && sizeof(CoarsenSums<3>) == sizeof(CellAcc3), "views of the cell blocks");
static_assert(offsetof(CellAcc, sxx) == offsetof(CoarsenSums<2>, ss) && offsetof(CellAcc, n) == offsetof(CoarsenSums<2>, n), "");
static_assert(offsetof(CellAcc3, ss) == offsetof(CoarsenSums<3>, ss) && offsetof(CellAcc3, n) == offsetof(CoarsenSums<3>, n), "");

struct CoarsenArgs {
  const void* src;       // fine sums [D][H][W]
  void* dst;             // coarse sums [Dc][Hc][Wc]: every one is written, empty ones as zero
  int W, H, D;           // fine extents (D = 1 in 2D)
  int Wc, Hc, Dc;
  int off[3];            // CoarsenAxis::off per axis (off[2] unused in 2D)
};

constexpr int kCoarsenThreads = 256;   // = child columns per workgroup

__device__ __forceinline__ __int128 shfl_xor_i128(__int128 v, int mask) {
  const unsigned long long lo = __shfl_xor((unsigned long long)v, mask);
  const long long hi = __shfl_xor((long long)(v >> 64), mask);
  return ((__int128)hi << 64) | (__int128)lo;
}

// ceil(sq / n) for 0 <= sq < 2^96, 0 < n <= 2^20, by long division in 32-bit digits (no 128-bit division on the device);
// the quotients this file asks for fit 64 bits (sq <= n^2 2^46)
__device__ __forceinline__ long long ceil_div_u128(unsigned __int128 sq, unsigned int n) {
  unsigned long long rem = (unsigned long long)(sq >> 64) % n;     // (the digit above contributes nothing below 2^64 n)
  unsigned long long q = 0;
  const unsigned long long lo = (unsigned long long)sq;
#pragma unroll
  for (int d = 1; d >= 0; --d) {
    const unsigned long long cur = (rem << 32) | ((lo >> (32 * d)) & 0xFFFFFFFFull);   // rem < 2^20: no overflow
    q = (q << 32) | (cur / n);
    rem = cur % n;
  }
  return (long long)(q + (rem ? 1ull : 0ull));
}

// One workgroup per run of kCoarsenThreads child columns of one coarse row: for each of the F (F x F in 3D) fine rows
// under it the run is ONE contiguous piece of src (kCoarsenThreads cells), fetched into LDS in 16-byte pieces, lane j
// piece j, j + 256, ... - fully coalesced whatever the cell size - then lane t takes child column t out of LDS and adds it,
// moved to the parent's centre, to its own partial sums; after the last row the F lanes of a parent add theirs across
// lanes and the first of them rounds and stores.  Children outside the fine grid count as empty.
template <int DIM, int F>
__global__ __launch_bounds__(kCoarsenThreads) void k_coarsen(CoarsenArgs a) {
  using Cell = CoarsenSums<DIM>;
  constexpr int kPieces = (int)sizeof(Cell) / 16;
  constexpr int NP = DIM * (DIM + 1) / 2;
  constexpr int kLog = F == 2 ? 1 : 2;
  constexpr int kParents = kCoarsenThreads / F;
  static_assert(sizeof(Cell) % 16 == 0 && (F == 2 || F == 4), "");
  __shared__ uint4 s_row[kCoarsenThreads * kPieces];
  const int t = threadIdx.x;
  const int kx = t & (F - 1);                              // the workgroup's first column is a parent's first
  const long long nbx = (a.Wc + kParents - 1) / kParents;
  const long long total = nbx * a.Hc * a.Dc;
  for (long long rb = blockIdx.x; rb < total; rb += gridDim.x) {
    const int bx = (int)(rb % nbx);
    const long long yz = rb / nbx;
    const int Y = (int)(yz % a.Hc), Z = (int)(yz / a.Hc);
    const int X0 = bx * kParents;
    const int ix0 = X0 * F - a.off[0];                     // fine column of lane 0 (may lie left of the grid)
    const int lo = ix0 < 0 ? 0 : ix0, hi = ix0 + kCoarsenThreads < a.W ? ix0 + kCoarsenThreads : a.W;
    unsigned int n = 0;
    long long N1[DIM] = {};
    __int128 N2[NP] = {};
    for (int kz = 0; kz < (DIM == 3 ? F : 1); ++kz) {
      const int iz = DIM == 3 ? Z * F + kz - a.off[2] : 0;
      if (iz < 0 || iz >= a.D) continue;                   // (the same in every lane of the workgroup, as the next two)
      for (int ky = 0; ky < F; ++ky) {
        const int iy = Y * F + ky - a.off[1];
        if (iy < 0 || iy >= a.H || lo >= hi) continue;
        const uint4* row = static_cast<const uint4*>(a.src) + ((size_t)iz * a.H + iy) * a.W * kPieces;
        __syncthreads();                                   // the row before has been read
        for (int j = t; j < kCoarsenThreads * kPieces; j += kCoarsenThreads) {
          const int cix = ix0 + j / kPieces;
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (cix >= lo && cix < hi) v = row[(long long)ix0 * kPieces + j];
          s_row[j] = v;
        }
        __syncthreads();
        const Cell c = *reinterpret_cast<const Cell*>(&s_row[t * kPieces]);
        if (c.n != 0u) {                                   // (empty children hold zero sums)
          const int d[3] = {2 * kx - F + 1, 2 * ky - F + 1, 2 * kz - F + 1};   // child centre - parent centre, in 2^21 fine units
          n += c.n;
          int p = 0;
#pragma unroll
          for (int i = 0; i < DIM; ++i) {
            N1[i] += c.s[i] + (long long)c.n * d[i] * 2097152ll;
#pragma unroll
            for (int k = i; k < DIM; ++k, ++p) {
              const long long cross = d[i] * c.s[k] + d[k] * c.s[i];            // |s| <= 2^42
              N2[p] += (__int128)c.ss[p] + (__int128)cross * 2097152ll + (__int128)((long long)c.n * d[i] * d[k]) * 4398046511104ll;
            }
          }
        }
      }
    }
    // the F lanes of a parent are neighbours in one wave
#pragma unroll
    for (int m = 1; m < F; m <<= 1) {
      n += __shfl_xor(n, m);
#pragma unroll
      for (int i = 0; i < DIM; ++i) N1[i] += __shfl_xor(N1[i], m);
#pragma unroll
      for (int p = 0; p < NP; ++p) N2[p] += shfl_xor_i128(N2[p], m);
    }
    const int X = X0 + t / F;
    if (kx == 0 && X < a.Wc) {
      Cell out;
      out.n = n; out.pad = 0u;
#pragma unroll
      for (int i = 0; i < DIM; ++i) out.s[i] = (N1[i] + F / 2) >> kLog;          // floor
#pragma unroll
      for (int p = 0; p < NP; ++p) out.ss[p] = (long long)((N2[p] + F * F / 2) >> (2 * kLog));
      // the two roundings can leave a nearly degenerate cell with n ss_aa < s_a^2, which no point set has and
      // ndt*_load_map refuses: the least ss_aa that has it
      if (n > 0u && n <= kMaxCellCount) {
        int p = 0;
#pragma unroll
        for (int i = 0; i < DIM; p += DIM - i, ++i) {
          const __int128 sq = (__int128)out.s[i] * out.s[i];
          if ((__int128)n * out.ss[p] < sq) out.ss[p] = ceil_div_u128((unsigned __int128)sq, n);
        }
      }
      static_cast<Cell*>(a.dst)[((size_t)Z * a.Hc + Y) * a.Wc + X] = out;
    }
  }
}

}  // namespace ndt

namespace {

template <int DIM>
int32_t launch_coarsen(const ndt::CoarsenArgs& a, int f, hipStream_t stream) {
  using namespace ndt;
  const long long nbx = (a.Wc + kCoarsenThreads / f - 1) / (kCoarsenThreads / f);
  const long long total = nbx * a.Hc * a.Dc;
  const unsigned blocks = (unsigned)(total < (1ll << 20) ? total : (1ll << 20));
  if (f == 2) hipLaunchKernelGGL((k_coarsen<DIM, 2>), dim3(blocks), dim3(kCoarsenThreads), 0, stream, a);
  else hipLaunchKernelGGL((k_coarsen<DIM, 4>), dim3(blocks), dim3(kCoarsenThreads), 0, stream, a);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// what both entry points refuse before they look at a grid; *f = the factor
template <class Handle>
int32_t check_coarsen_args(const Handle* src, const Handle* dst, int* f) {
  if (!src || !dst) { set_error("coarsen_map: a handle is null"); return NDT_ERR_INVALID_ARG; }
  if (src == dst) { set_error("coarsen_map: source and destination are one handle"); return NDT_ERR_INVALID_ARG; }
  if (src->device != dst->device) { set_error("coarsen_map: both handles must live on one device"); return NDT_ERR_INVALID_ARG; }
  if (src->prm.overlap_grids == 4 || dst->prm.overlap_grids == 4) {
    set_error("coarsen_map does not take overlapping grids");
    return NDT_ERR_INVALID_ARG;
  }
  *f = ndt::coarsen_factor(src->prm.cell_size, dst->prm.cell_size);
  if (*f == 0) { set_error("coarsen_map: the destination's cell_size must be exactly 2 or 4 times the source's"); return NDT_ERR_INVALID_ARG; }
  if (!src->has_target) { set_error("coarsen_map: the source handle holds no target"); return NDT_ERR_NO_TARGET; }
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_coarsen_map(ndt2d_handle* src, ndt2d_handle* dst) {
  TraceRange range("ndt2d_coarsen_map");
  int f = 0;
  { const int32_t cs = check_coarsen_args(src, dst, &f); if (cs != NDT_OK) return cs; }
  HIP_TRY(hipSetDevice(dst->device));
  { const int32_t fs = finish(src); if (fs != NDT_OK) return fs; }
  { const int32_t fs = finish(dst); if (fs != NDT_OK) return fs; }
  dst->has_target = false;
  grid_changed(dst);
  const GridDev& s = src->grid;
  CoarsenAxis ax, ay;
  if (!coarsen_axis(s.ox, s.cell, s.W, f, &ax) || !coarsen_axis(s.oy, s.cell, s.H, f, &ay)) {
    set_error("coarsen_map: the source grid's origin is no lattice point the library can index");
    return NDT_ERR_INVALID_ARG;
  }
  GridDev& g = dst->grid;
  const double c = dst->prm.cell_size;
  g.cell = c; g.cell32 = (float)c; g.inv_c = (float)(1.0 / c);
  g.W = ax.extent; g.H = ay.extent; g.ngrid = 1; g.pad = 0;
  static const double kShift[4][2] = {{0.0, 0.0}, {0.5, 0.0}, {0.0, 0.5}, {0.5, 0.5}};   // as setup_geometry: also with one grid
  for (int q = 0; q < kMaxGrids; ++q) {
    g.gx[q] = (float)(((double)ax.K0 - kShift[q][0] * f) * s.cell);
    g.gy[q] = (float)(((double)ay.K0 - kShift[q][1] * f) * s.cell);
  }
  g.ox = g.gx[0]; g.oy = g.gy[0];
  g.fix_scale = std::ldexp(1.0, kFixShift) / c;
  const size_t ncell = (size_t)g.W * g.H;
  if (ncell > kMaxCells) { set_error("target extent / cell_size needs more than 2^27 cells"); return NDT_ERR_CAPACITY; }
  { const int32_t es = ensure_cells(dst, ncell); if (es != NDT_OK) return es; }
  HIP_TRY(order_after(dst->stream, src->stream, &src->map_ev));     // src's sums may still be in flight on its stream
  const CoarsenArgs a{s.acc, g.acc, s.W, s.H, 1, g.W, g.H, 1, {ax.off, ay.off, 0}};
  { const int32_t ls = launch_coarsen<2>(a, f, dst->stream); if (ls != NDT_OK) return ls; }
  { const int32_t fs = finalise_grid(dst); if (fs != NDT_OK) return fs; }   // synchronises: src is free on return
  dst->n_points = src->n_points;
  dst->last_ntile = 0;               // as ndt2d_load_map
  dst->has_target = true;
  return upload_static(dst);
}

int32_t ndt3d_coarsen_map(ndt3d_handle* src, ndt3d_handle* dst) {
  using namespace ndt;
  TraceRange range("ndt3d_coarsen_map");
  int f = 0;
  { const int32_t cs = check_coarsen_args(src, dst, &f); if (cs != NDT_OK) return cs; }
  HIP_TRY(hipSetDevice(dst->device));
  { const int32_t fs = finish(src); if (fs != NDT_OK) return fs; }
  { const int32_t fs = finish(dst); if (fs != NDT_OK) return fs; }
  dst->has_target = false;
  grid_changed3(dst);
  const Grid3Dev& s = src->grid;
  CoarsenAxis ax[3];
  if (!coarsen_axis(s.ox, s.cell, s.W, f, &ax[0]) || !coarsen_axis(s.oy, s.cell, s.H, f, &ax[1]) ||
      !coarsen_axis(s.oz, s.cell, s.D, f, &ax[2])) {
    set_error("coarsen_map: the source grid's origin is no lattice point the library can index");
    return NDT_ERR_INVALID_ARG;
  }
  Grid3Dev& g = dst->grid;
  const double c = dst->prm.cell_size;
  g.cell = c; g.inv_c = (float)(1.0 / c);
  g.ox = ax[0].origin; g.oy = ax[1].origin; g.oz = ax[2].origin;
  g.W = ax[0].extent; g.H = ax[1].extent; g.D = ax[2].extent; g.pad = 0;
  g.fix_scale = std::ldexp(1.0, kFixShift) / c;
  const double ncell_d = (double)g.W * g.H * g.D;
  if (ncell_d > (double)kMaxCells) { set_error("3D target needs more than 2^27 cells"); return NDT_ERR_CAPACITY; }
  { const int32_t es = ensure_cells3(dst, (size_t)ncell_d); if (es != NDT_OK) return es; }
  HIP_TRY(order_after(dst->stream, src->stream, &src->map_ev));
  const CoarsenArgs a{s.acc, g.acc, s.W, s.H, s.D, g.W, g.H, g.D, {ax[0].off, ax[1].off, ax[2].off}};
  { const int32_t ls = launch_coarsen<3>(a, f, dst->stream); if (ls != NDT_OK) return ls; }
  { const int32_t fs = finalise_grid3(dst); if (fs != NDT_OK) return fs; }  // synchronises: src is free on return
  dst->has_target = true;
  return upload_static3(dst);
}

}  // extern "C"

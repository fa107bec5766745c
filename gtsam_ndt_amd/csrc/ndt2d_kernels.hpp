// 2D NDT kernels for gfx950 (MI355X).  Hand-written HIP; wave64, DPP reductions, no MFMA
// (point-wise gather + reduction, HBM/latency bound - BASELINE.json north_star).
//
// Stage map (the reference has no source to cite,
// /root/reference/README.md:1 is its only line):
//   k_bounds        a1  bounding box of the target cloud
//   k_accumulate    a1+a2  cell key + exact fixed-point per-cell sums (n, Su, Suu')
//   k_finalise      a3  sums -> Welford form (n, mean, M2) -> Sigma -> clamp -> Sigma^-1 record
//   k_iterate<MODE> a4-a8  one launch per Gauss-Newton iteration:
//                       prologue  = fixed-order reduction of the previous launch's block
//                                   partials + 3x3 solve + pose update (every block, redundantly)
//                       body      = transform, lookup, score, Jacobian, per-thread sums
//                       epilogue  = wave DPP tree -> LDS -> the block's sums as three 16-byte entries
#pragma once
#include "ndt_device.hpp"
#include "ndt_chain.hpp"
#include "ndt_lattice.hpp"
#include "ndt_pose.hpp"

namespace ndt {

constexpr int kBlock = 256;        // threads per workgroup (4 waves)
constexpr int kMaxBlocks = 256;    // one workgroup per CU; also rows in the partials table
constexpr int kNumAcc = 12;        // Hxx Hxy Hyy Hxt Hyt Htt gx gy gt score nhit (pad)
constexpr int kFixShift = 22;      // fixed-point: U = rint(u * 2^22 / c), |U| <= 2^21
constexpr unsigned kMaxCellCount = 1u << 20;  // n*U^2 < 2^63 needs n <= 2^20 per cell

// ---- per-cell exact sums (48 B) -----------------------------------------------------
struct CellAcc {
  long long sx, sy, sxx, sxy, syy;
  unsigned int n;
  unsigned int pad;
};

constexpr int kMaxGrids = 4;       // Biber's four half-cell-shifted grids (params.overlap_grids = 4)

struct GridDev {
  float ox, oy, inv_c, cell32;   // origin of grid 0
  int W, H;
  int ngrid, pad;                // 1 or 4; grid g's cells are [g*W*H, (g+1)*W*H) of rec / acc
  float gx[kMaxGrids], gy[kMaxGrids];   // origin of grid g (gx[0] = ox, gy[0] = oy)
  double cell;       // params.cell_size
  double fix_scale;  // 2^kFixShift / cell
  float4* rec;       // one 32-byte record per cell = two float4: rec[2k] = (mean_x, mean_y, a, b),
                     // rec[2k+1] = (b, c, n as float, 0); both halves share one 64-byte line
  CellAcc* acc;
};

struct SolveParams {
  float d1, d2;
  int hessian_mode;
  int max_iterations;
  int min_hits;
  int line_search;   // > 0: backtracking line search, at most this many halvings per step
  double eps_trans, eps_rot, step_max_trans, step_max_rot;
  double step_scale;   // over-relaxation factor on the solved step (1 = plain)
};

// Backtracking line-search state (oracle/ndt2d.py gn_update): the pose the current step
// started from, its score, the clamped step and how far along it the trial pose sits.
struct LineSearch {
  double base[3];
  double step[3];
  double score;
  double alpha;
  int trials;
  int valid;
};
constexpr double kLineSearchTol = 1e-3;   // oracle/ndt2d.py LS_TOL

// State handed from launch k-1 to launch k through HBM (kernel boundary = the only
// inter-workgroup synchronisation; no in-launch hand-off, no atomics).
struct IterState {
  double pose[3];
  double H[6];   // xx xy yy xt yt tt of the last evaluation
  double g[3];
  double score;
  int n_hit;
  int iter;
  int status;
  int done;
  int have_partials;
  int pad;           // index of the launch that wrote this state (what the host sees as progress)
};

// Device context, split by who writes it so that the read-only parts can be fetched with
// scalar loads in one batch at kernel entry:
//   AlignStatic  grid + solver parameters; uploaded by the host when the target changes
//   AlignCall    per-alignment arguments; written by the first launch of a single-scan chain (k_iterate_first, from its
//                kernel arguments) or, under the old protocol (NDT_TUNE_FUSED_BEGIN = 0, ndt2d_align_trace), by k_begin
//   AlignDyn     iteration state and block partials; written by k_iterate_first / k_begin and k_iterate
struct AlignStatic {
  GridDev grid;
  SolveParams prm;
};
struct AlignCall {
  const float* sx;
  const float* sy;
  int n;
  int fixed_iterations;
  // converged mode: pinned host memory the finishing launch writes the final state and a flag
  // into, so the host sees the end of the loop without a copy or a stream sync (null = off)
  IterState* host_state;
  int* host_flag;
  int seq;                   // this call's number: what the first launch past the end reports in host_flag[2]
  int pad;
};
// partials: what a launch hands to the next, 12 KB per parity.  The single-scan chain (k_iterate, k_iterate_first) keeps
// it packed by workgroup: entry [g][partial_slot(b)] holds sums 4g .. 4g+3 of workgroup b (sum 11 is the zero pad), so
// that a workgroup leaves its 11 sums as three 16-byte stores and the fold reads four 16-byte entries per lane.
// partial_slot puts the eight workgroups that share a 128-byte line on one XCD (consecutive workgroups go round the
// eight XCDs): a line is merged in one L2 instead of being written in parts from all eight.  Only the speed depends on
// where the workgroups really run.  The map-to-map chain (k_begin_d2d, k_iterate_d2d) keeps the same bytes as one row of
// kMaxBlocks entries per sum (rows).  A chain never reads what another chain wrote: its first launch reads no partials.
__host__ __device__ constexpr int partial_slot(int b) { return (b & 7) * (kMaxBlocks / 8) + (b >> 3); }
struct AlignDyn {
  IterState state[2];
  union {
    float4 partials[2][kNumAcc / 4][kMaxBlocks];
    float rows[2][kNumAcc][kMaxBlocks];
  };
  LineSearch ls[2];       // ping-pong like state; touched only when prm.line_search > 0
};
static_assert(kNumAcc % 4 == 0 && sizeof(AlignDyn::partials) == sizeof(AlignDyn::rows) &&
              offsetof(AlignDyn, partials) % 16 == 0, "the partials table: 24 KB, 16-byte aligned, in either view");

// A scan moved into the map frame with the pose an alignment returned, before it is merged into
// the submap (ndt2d_add_target_points_dev): float32 products and sums in a fixed order (no
// contraction), so that a host restatement reproduces the points bit for bit.
__global__ __launch_bounds__(kBlock) void k_transform_points(const float* __restrict__ x, const float* __restrict__ y,
                                                              size_t n, float cs, float sn, float tx, float ty,
                                                              float* __restrict__ ox, float* __restrict__ oy) {
#pragma clang fp contract(off)      // hipcc's __fmul_rn is a plain `*` and would be fused into an fma
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float px = x[i], py = y[i];
  const float a = cs * px, b = sn * py, c = sn * px, d = cs * py;
  ox[i] = (a - b) + tx;
  oy[i] = (c + d) + ty;
}

// ---------------------------------------------------------------------------- a1 bounds
__global__ __launch_bounds__(kBlock) void k_bounds(const float* __restrict__ x,
                                                    const float* __restrict__ y, size_t n,
                                                    unsigned int* __restrict__ out /*[4]*/) {
  float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  // 8 points in flight per thread: a one-point loop pays the memory latency per trip
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += 8 * stride) {
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t ii = i + u * stride;
      a[u] = ii < n ? x[ii] : NAN;
      b[u] = ii < n ? y[ii] : NAN;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (isfinite(a[u]) && isfinite(b[u])) {
        xmin = fminf(xmin, a[u]); xmax = fmaxf(xmax, a[u]);
        ymin = fminf(ymin, b[u]); ymax = fmaxf(ymax, b[u]);
      }
    }
  }
  xmin = wave_min(xmin); xmax = wave_max(xmax);
  ymin = wave_min(ymin); ymax = wave_max(ymax);
  __shared__ float s_b[kBlock / 64][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_b[wave][0] = xmin; s_b[wave][1] = xmax; s_b[wave][2] = ymin; s_b[wave][3] = ymax; }
  __syncthreads();
  if (threadIdx.x == 0) {   // one atomic per block and bound: the four words are contended
    for (int w = 1; w < kBlock / 64; ++w) {
      xmin = fminf(xmin, s_b[w][0]); xmax = fmaxf(xmax, s_b[w][1]);
      ymin = fminf(ymin, s_b[w][2]); ymax = fmaxf(ymax, s_b[w][3]);
    }
    atomicMin(&out[0], float_to_ordered(xmin));
    atomicMax(&out[1], float_to_ordered(xmax));
    atomicMin(&out[2], float_to_ordered(ymin));
    atomicMax(&out[3], float_to_ordered(ymax));
  }
}

// The grid's outermost ring of cells never receives a target point: the source-side lookup clamps
// keys onto the grid instead of testing them (image_key below), so every out-of-range, NaN or
// dead-lane lookup lands on a ring cell, which must therefore stay invalid.  ndt2d_set_target's
// geometry leaves the ring empty by construction (one guard cell either side) except for a
// boundary point that float32 rounding of (x - ox) * inv_c puts into cell 0 with a cell size that
// is not a power of two; ndt2d_reserve_target + ndt2d_add_target_points can put points anywhere.
// Both are handled by the one rule every build path calls, cell_of<kRing2> (ndt_lattice.hpp): a point
// whose cell lies on the ring counts as outside the grid (oracle/ndt2d.py cell_keys32(interior=True)
// states the same rule).  cell_centre, fix_coord and the terms of a point come from the same header,
// so the global-memory path, the binned builds and the LDS-resident batch kernels build
// bit-identical cell records from the same points.
constexpr int kRing2 = 1;
using Limit2 = LatticeLimit<kRing2>;

// a3 (1/2): exact sums -> Welford form (n, mean, M2) -> Sigma = M2/(n-1) -> eigenvalues, clamp, unit eigenvector of
// the large one.  float64 scalar code in the order of oracle/ndt2d.py finalise_cell().  Shared by the Sigma^-1
// records (finalise_sums) and the covariance records of map-to-map alignment (ndt2d_d2d.hpp: cov_record).
// Returns false when the cell is not usable.
struct CellEig {
  double mx, my;     // mean
  double l1, l2c;    // large eigenvalue, clamped small one
  double ex, ey;     // unit eigenvector of l1
};
__device__ __forceinline__ bool cell_eigen(int n, long long sx, long long sy, long long sxx, long long sxy, long long syy,
                                           double cx, double cy, double fix_scale, int min_points, double eig_ratio,
                                           CellEig& e) {
  if (n < min_points || n < 2) return false;
  // one reciprocal per cell: r = 1 / (n S); mean = centre + Su r; 1 / (n S^2) = r^2 n.  (A reciprocal of
  // fix_scale alone would be loop-invariant in every caller and cost a register pair held across the
  // whole build: the 1024-thread batch kernel spilled it.)
  const double dn = (double)n;
  const double r = 1.0 / (dn * fix_scale);
  e.mx = fma((double)sx, r, cx);
  e.my = fma((double)sy, r, cy);
  // M2 = (n*Suu - Su*Su) / (n * S^2), numerator exact in 128-bit
  const double den = r * r * dn;
  const double m2xx = to_double(sub128(mul_s64(n, sxx), mul_s64(sx, sx))) * den;
  const double m2xy = to_double(sub128(mul_s64(n, sxy), mul_s64(sx, sy))) * den;
  const double m2yy = to_double(sub128(mul_s64(n, syy), mul_s64(sy, sy))) * den;
  const double vxx = m2xx / (dn - 1.0), vxy = m2xy / (dn - 1.0), vyy = m2yy / (dn - 1.0);
  const double half_tr = 0.5 * (vxx + vyy);
  const double half_df = 0.5 * (vxx - vyy);
  const double disc = sqrt(fma(half_df, half_df, vxy * vxy));
  e.l1 = half_tr + disc;
  const double l2 = half_tr - disc;
  if (!(e.l1 > 0.0)) return false;
  e.l2c = fmax(l2, eig_ratio * e.l1);
  double ex, ey;
  if (half_df >= 0.0) { ex = half_df + disc; ey = vxy; }
  else                { ex = vxy; ey = disc - half_df; }
  const double nrm = sqrt(fma(ex, ex, ey * ey));
  if (nrm > 0.0) { ex /= nrm; ey /= nrm; } else { ex = 1.0; ey = 0.0; }
  e.ex = ex; e.ey = ey;
  return true;
}

// a3 (2/2): -> Sigma^-1 record.  Returns false (record zeroed) when the cell is not usable.
__device__ __forceinline__ bool finalise_sums(int n, long long sx, long long sy, long long sxx, long long sxy,
                                              long long syy, double cx, double cy, double fix_scale,
                                              int min_points, double eig_ratio, float4& ra, float4& rb) {
  ra = make_float4(0.f, 0.f, 0.f, 0.f);
  rb = make_float4(0.f, 0.f, 0.f, 0.f);
  CellEig e;
  if (!cell_eigen(n, sx, sy, sxx, sxy, syy, cx, cy, fix_scale, min_points, eig_ratio, e)) return false;
  const double ex = e.ex, ey = e.ey;
  const double i1 = 1.0 / e.l1, i2 = 1.0 / e.l2c, d = i1 - i2;
  const float b32 = (float)(d * ex * ey);
  ra = make_float4((float)e.mx, (float)e.my, (float)fma(d * ex, ex, i2), b32);
  rb = make_float4(b32, (float)fma(d * ey, ey, i2), (float)n, 0.f);
  return true;
}

// What a removal (SIGN = -1 of the build kernels) must not leave in a cell: a count that went below zero - it wrapped, and
// a cell of a usable grid never holds more than kMaxCellCount points, so anything above that is a wrap as long as the
// removed cloud has fewer than 2^32 - 2^20 points (the entry points see to that) - or a count of zero with a sum left.
// Either shows that points were removed that are not in the map.  any_sum = the cell's sums or-ed together.
__device__ __forceinline__ bool removed_cell_broken(unsigned int n, unsigned long long any_sum) {
  return n > kMaxCellCount || (n == 0u && any_sum != 0ull);
}

// ------------------------------------------------------------------ a1+a2 accumulate
// Exact, order-independent per-cell sufficient statistics: cell-centred coordinates
// quantised to c*2^-22 and summed with 64-bit integer atomics.  Integer addition is
// associative, so the sums (and everything derived from them) are bitwise identical from
// run to run and under any point order; merging two clouds' sums is the exact form of the
// Chan/Welford pairwise update.
// SIGN = -1: the points' contributions are taken out of the sums (ndt_device.hpp, "a build with a sign").
template <int SIGN>
__global__ __launch_bounds__(kBlock) void k_accumulate(const float* __restrict__ x,
                                                        const float* __restrict__ y, size_t n,
                                                        GridDev g,
                                                        unsigned long long* __restrict__ n_outside) {
  unsigned int outside = 0;
  const size_t ncell = (size_t)g.W * g.H;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const float px = x[i], py = y[i];
    bool any = false;
    for (int q = 0; q < g.ngrid; ++q) {
      const float ox = g.gx[q], oy = g.gy[q];
      int ix, iy;
      if (cell_of(px, py, ox, oy, g.inv_c, Limit2(g.W), Limit2(g.H), ix, iy)) {
        any = true;
        CellAcc* c = g.acc + (q * ncell + (size_t)iy * g.W + ix);
        atomicAdd(&c->n, signed_one<SIGN>());
        point_terms(px, py, ox, oy, ix, iy, g.cell, g.fix_scale, [&](int j, unsigned long long t) {
          atomicAdd((unsigned long long*)&c->sx + j, signed_term<SIGN>(t));
        });
      }
    }
    if (!any) outside++;
  }
  if (n_outside && outside) atomicAdd(n_outside, (unsigned long long)outside);
}

// ------------------------------------------------------------------------- a3 finalise
// One thread per cell.  SIGN = -1 (behind a removal): a cell the removal broke is counted in counters[kCountUnder].
template <int SIGN>
__global__ __launch_bounds__(kBlock) void k_finalise(GridDev g, int min_points, double eig_ratio,
                                                      int* __restrict__ counters /*[kCountShards][2]: valid, overflow*/) {
  int* const under = counters + kCountUnder;
  counters = count_shard(counters);
  const size_t ncell = (size_t)g.W * g.H;
  const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= ncell * g.ngrid) return;
  const CellAcc c = g.acc[k];
  float4 ra, rb;
  bool ok = false;
  if (SIGN < 0 && removed_cell_broken(c.n, (unsigned long long)(c.sx | c.sy | c.sxx | c.sxy | c.syy))) {
    atomicAdd(under, 1);                           // (only a removal of points that are not in the map comes here)
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    rb = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if (c.n > kMaxCellCount) {
    atomicAdd(&counters[1], 1);
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    rb = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if ((int)c.n >= min_points) {             // empty cells (the vast majority) skip everything
    const unsigned int w32 = (unsigned int)g.W, nc32 = (unsigned int)ncell;   // <= 2^27 cells: 32-bit div
    const unsigned int q = (unsigned int)k / nc32, k32 = (unsigned int)k - q * nc32;
    const int ix = (int)(k32 % w32), iy = (int)(k32 / w32);
    ok = finalise_sums((int)c.n, c.sx, c.sy, c.sxx, c.sxy, c.syy, cell_centre(g.gx[q], ix, g.cell),
                       cell_centre(g.gy[q], iy, g.cell), g.fix_scale, min_points, eig_ratio, ra, rb);
  } else {
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    rb = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // one atomic per wave, not one per valid cell (18.7k same-address atomics cost ~190 us)
  const unsigned long long valid_mask = __ballot(ok);
  if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(valid_mask | (1ull << 63)) && valid_mask)
    atomicAdd(&counters[0], (int)__popcll(valid_mask));
  g.rec[2 * k] = ra;
  g.rec[2 * k + 1] = rb;
}

// ---------------------------------------------------------------------- a8 solve/update
// Scalar float64 on the critical path of every iteration (each workgroup runs it
// redundantly in its prologue), so it is written for latency: LDL^T with three reciprocals
// (v_rcp_f64 + two Newton steps) instead of divisions and square roots, squared norms
// instead of sqrt, and a branch-free sincos for |t| <= pi.  Same algorithm and pivot tests as
// oracle/ndt2d.py solve3()/gn_update().
__device__ __forceinline__ double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

__device__ __forceinline__ bool solve3(const double* H /*xx xy yy xt yt tt*/, const double* g,
                                       double* d) {
  const double h00 = H[0], h01 = H[1], h11 = H[2], h02 = H[3], h12 = H[4], h22 = H[5];
  const double d0 = fmax(fabs(h00), 1e-12), d1 = fmax(fabs(h11), 1e-12), d2 = fmax(fabs(h22), 1e-12);
  double lam = 0.0;
  for (int attempt = 0; attempt < 12; ++attempt) {
    const double a00 = h00 + lam * d0, a11 = h11 + lam * d1, a22 = h22 + lam * d2;
    if (a00 > 1e-12 * d0) {
      const double r0 = fast_rcp(a00);
      const double l10 = h01 * r0, l20 = h02 * r0;
      const double p1 = a11 - l10 * h01;
      if (p1 > 1e-12 * d1) {
        const double r1 = fast_rcp(p1);
        const double t = h12 - l20 * h01;
        const double l21 = t * r1;
        const double p2 = a22 - l20 * h02 - l21 * t;
        if (p2 > 1e-12 * d2) {
          const double r2 = fast_rcp(p2);
          const double z0 = -g[0];
          const double z1 = -g[1] - l10 * z0;
          const double z2 = -g[2] - l20 * z0 - l21 * z1;
          const double x2 = z2 * r2;
          const double x1 = z1 * r1 - l21 * x2;
          const double x0 = z0 * r0 - l10 * x1 - l20 * x2;
          if (isfinite(x0) && isfinite(x1) && isfinite(x2)) {
            d[0] = x0; d[1] = x1; d[2] = x2;
            return true;
          }
        }
      }
    }
    lam = (lam == 0.0) ? 1e-6 : lam * 10.0;
  }
  return false;
}

// sin/cos for |t| <= ~pi (poses are wrapped): quadrant reduction + the classic fdlibm
// minimax kernels on [-pi/4, pi/4]; error < 1 ulp, no table, no slow path.
__device__ __forceinline__ void sincos_wrapped(double t, double* sn, double* cs) {
  const double k = rint(t * 0.63661977236758134308);            // 2/pi
  double r = fma(-k, 1.57079632679489655800e+00, t);             // pi/2 hi
  r = fma(-k, 6.12323399573676603587e-17, r);                    // pi/2 lo
  const double z = r * r;
  const double ps = fma(fma(fma(fma(fma(1.58969099521155010221e-10, z, -2.50507602534068634195e-08), z,
                                    2.75573137070700676789e-06), z, -1.98412698298579493134e-04), z,
                            8.33333333332248946124e-03), z, -1.66666666666666324348e-01);
  const double s = fma(r * z, ps, r);
  const double pc = fma(fma(fma(fma(fma(-1.13596475577881948265e-11, z, 2.08757232129817482790e-09), z,
                                    -2.75573143513906633035e-07), z, 2.48015872894767294178e-05), z,
                            -1.38888888888741095749e-03), z, 4.16666666666666019037e-02);
  const double c = fma(z * z, pc, fma(-0.5, z, 1.0));
  const int q = ((int)k) & 3;
  const double s1 = (q & 1) ? c : s;
  const double c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}

// returns done; updates pose/iter/status in place
// ls_in / ls_out: line-search state before / after this step (the same object, or the two
// ping-pong slots); touched only when p.line_search > 0; `write` selects the one storing thread.
__device__ __forceinline__ bool gn_update(double* pose, const double* H, const double* g, int n_hit,
                                          int& iter, int& status, const SolveParams& p, int fixed_iterations,
                                          double score, const LineSearch* ls_in, LineSearch* ls_out, bool write) {
  if (p.line_search > 0 && ls_in->valid && ls_in->trials < p.line_search &&
      (n_hit < p.min_hits || score < ls_in->score - kLineSearchTol * fabs(ls_in->score))) {
    // the evaluation was a trial of the previous step and it scored worse: halve and retry
    LineSearch ls = *ls_in;
    ls.alpha *= 0.5;
    ls.trials += 1;
    pose[0] = ls.base[0] + ls.alpha * ls.step[0];
    pose[1] = ls.base[1] + ls.alpha * ls.step[1];
    pose[2] = wrap_angle(ls.base[2] + ls.alpha * ls.step[2]);
    if (write) *ls_out = ls;
    iter += 1;
    status = 0;
    if (fixed_iterations > 0) return iter >= fixed_iterations;
    if (iter >= p.max_iterations) { status = 1; return true; }
    return false;
  }
  if (n_hit < p.min_hits) { status = 3; return true; }
  double d[3];
  if (!solve3(H, g, d)) { status = 2; return true; }
  d[0] *= p.step_scale; d[1] *= p.step_scale; d[2] *= p.step_scale;
  const double nt2 = d[0] * d[0] + d[1] * d[1];
  const double nr = fabs(d[2]);
  double alpha = 1.0;
  if (nt2 > p.step_max_trans * p.step_max_trans) alpha = p.step_max_trans / sqrt(nt2);
  if (nr * alpha > p.step_max_rot) alpha = p.step_max_rot / nr;
  if (p.line_search > 0 && write) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { ls_out->base[j] = pose[j]; ls_out->step[j] = d[j] * alpha; }
    ls_out->score = score; ls_out->alpha = 1.0; ls_out->trials = 0; ls_out->valid = 1;
  }
  pose[0] += d[0] * alpha;
  pose[1] += d[1] * alpha;
  pose[2] = wrap_angle(pose[2] + d[2] * alpha);
  iter += 1;
  status = 0;
  if (fixed_iterations > 0) return iter >= fixed_iterations;
  if (nt2 * alpha * alpha < p.eps_trans * p.eps_trans && nr * alpha < p.eps_rot) return true;
  if (iter >= p.max_iterations) { status = 1; return true; }
  return false;
}

// Per-call part of the context, written from kernel arguments (no host buffer lifetime).
__global__ void k_begin(AlignCall* __restrict__ call, AlignDyn* __restrict__ dyn, const float* sx,
                        const float* sy, int n, double p0, double p1, double p2, int fixed_iterations,
                        IterState* host_state, int* host_flag, int seq) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  call->seq = seq;
  call->pad = 0;
  call->sx = sx;
  call->sy = sy;
  call->n = n;
  call->fixed_iterations = fixed_iterations;
  call->host_state = host_state;
  call->host_flag = host_flag;
  IterState s = {};
  s.pose[0] = p0; s.pose[1] = p1; s.pose[2] = wrap_angle(p2);
  dyn->state[1] = s;            // launch 0 has parity 0 and reads slot 1
  dyn->state[0] = IterState{};
  dyn->ls[0] = LineSearch{};
  dyn->ls[1] = LineSearch{};
}

// ---- per-point pieces of the body (rows a4-a6) ------------------------------------------
// The loop-closure kernel is VALU-issue bound, so this code is written
// for instructions per point: clamped keys instead of an in-grid compare chain, one-instruction
// floor, 24-bit multiply, d1 folded into the exponent and d2 applied once to the finished sums,
// the SE(2) Jacobian read off the image point, hits counted on the scalar unit.  (Writing the
// (x,y) math on register pairs for v_pk_*_f32 was measured: no gain, gfx950 issues packed f32
// at half rate.)
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct PoseF {
  float cs, sn, tx, ty, ox, oy, inv_c;
  int W, wm1, hm1;
  float lg_d1;   // log2(d1):  d1*exp(-d2/2 m) = exp2(nhd2*m + lg_d1)
  float nhd2;    // -d2/2 * log2(e)
  float d2;
};
// -d2/2 * log2(e), the scale of every score's exponent: d1 exp(-d2/2 m) = d1 exp2(nhd2_of(d2) m)
__device__ __forceinline__ float nhd2_of(float d2) { return -0.5f * d2 * 1.44269504088896340736f; }
__device__ __forceinline__ PoseF make_pose(float cs, float sn, float tx, float ty, float ox, float oy, float inv_c,
                                           int W, int H, float d1, float d2) {
  PoseF P;
  P.cs = cs; P.sn = sn; P.tx = tx; P.ty = ty; P.ox = ox; P.oy = oy; P.inv_c = inv_c;
  P.W = W; P.wm1 = W - 1; P.hm1 = H - 1;
  P.lg_d1 = __builtin_amdgcn_logf(d1);                 // v_log_f32 = log2
  P.nhd2 = nhd2_of(d2);
  P.d2 = d2;
  return P;
}

// floor(f) as int32 in ONE instruction (v_cvt_flr_i32_f32: saturating, NaN -> 0); the
// portable spelling costs v_floor_f32 + v_cvt_i32_f32 per coordinate in the hottest loop.
__device__ __forceinline__ int floor_to_int(float f) {
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(f));
  return r;
}

// clamp(i, 0, hi) in one instruction (v_med3_i32); min(max()) with a runtime bound is two
__device__ __forceinline__ int clamp_index(int i, int hi) {
  int r;
  asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(i), "s"(hi));
  return r;
}

struct PointRec {
  float px, py;   // image R p + t of the source point (non-finite coordinates clamped to +-1e15)
  float4 A;       // mean_x, mean_y, a, b
  float4 B;       // b, c, n, 0
};

// a4 (1/2): transform and cell key.  No in-grid compare chain: the key is clamped onto the grid,
// whose outermost ring of cells is empty by construction (one guard cell below the minimum,
// one above the maximum), so every out-of-range, infinite or NaN point lands on an invalid
// cell.  NaN/inf never reach the sums: coordinates are clamped to +-1e15 first (v_med3_f32
// returns the finite bound for a NaN), which keeps every later product finite.
// In two halves, for the kernels that clamp a point once where they stage it and take its image per pose.
__device__ __forceinline__ float clamp_coord(float v) { return __builtin_amdgcn_fmed3f(v, -1e15f, 1e15f); }
__device__ __forceinline__ void image_clamped(const PoseF& P, float x, float y, PointRec& r) {
  r.px = fmaf(P.cs, x, fmaf(-P.sn, y, P.tx));
  r.py = fmaf(P.sn, x, fmaf(P.cs, y, P.ty));
}
__device__ __forceinline__ void image_point(const PoseF& P, float x, float y, PointRec& r) {
  image_clamped(P, clamp_coord(x), clamp_coord(y), r);
}
__device__ __forceinline__ int image_key(const PoseF& P, float ox, float oy, const PointRec& r, bool live) {
  int ix = floor_to_int((r.px - ox) * P.inv_c), iy = floor_to_int((r.py - oy) * P.inv_c);
  ix = clamp_index(ix, P.wm1);
  iy = clamp_index(iy, P.hm1);
  return live ? __mul24(iy, P.W) + ix : 0;                        // cell 0 is a guard cell; W, iy < 2^24
}
__device__ __forceinline__ int point_key(const PoseF& P, float x, float y, bool live, PointRec& r) {
  image_point(P, x, y, r);
  return image_key(P, P.ox, P.oy, r, live);
}

// a4 (2/2), global-memory grid: one 32-byte record per cell
__device__ __forceinline__ void lookup_point(const PoseF& P, const float4* __restrict__ rec, float x, float y,
                                             bool live, PointRec& r) {
  const int key = point_key(P, x, y, live, r);
  r.A = rec[2 * key];
  r.B = rec[2 * key + 1];
}

// m = q' Sigma^-1 q of an image point in the cell whose record it carries, and v = Sigma^-1 q
__device__ __forceinline__ float mahalanobis2(const PointRec& r, float& vx, float& vy) {
  const float a = r.A.z, b = r.A.w, c = r.B.y;
  const float qx = r.px - r.A.x, qy = r.py - r.A.y;
  vx = fmaf(a, qx, b * qy); vy = fmaf(b, qx, c * qy);
  return fmaf(qx, vx, qy * vy);
}
__device__ __forceinline__ float mahalanobis2(const PointRec& r) { float vx, vy; return mahalanobis2(r, vx, vy); }

struct Acc2D {            // the running sums of one thread (unscaled: d2 is applied in acc_store)
  float h0, h1, h2, h3, h4, h5;   // Hxx Hxy Hyy Hxt Hyt Htt
  float g0, g1, g2, s;            // gx gy gt score
  int n_wave;                     // hits of the whole wave, kept on the scalar unit
};
__device__ __forceinline__ void acc_zero(Acc2D& a) {
  a.h0 = a.h1 = a.h2 = a.h3 = a.h4 = a.h5 = a.g0 = a.g1 = a.g2 = a.s = 0.f;
  a.n_wave = 0;
}
__device__ __forceinline__ void acc_store(const Acc2D& a, float d2, float* out /*[11]*/) {
  out[0] = a.h0 * d2; out[1] = a.h1 * d2; out[2] = a.h2 * d2; out[3] = a.h3 * d2; out[4] = a.h4 * d2;
  out[5] = a.h5 * d2; out[6] = a.g0 * d2; out[7] = a.g1 * d2; out[8] = a.g2 * d2; out[9] = a.s;
  out[10] = (threadIdx.x & 63) == 0 ? (float)a.n_wave : 0.f;     // the wave's hits, once
}

// a5+a6: Mahalanobis score, SE(2) Jacobian, gradient / Hessian terms into the thread's sums
template <int MODE>
__device__ __forceinline__ void accumulate_point(const PoseF& P, const PointRec& r, Acc2D& acc) {
  const bool hit = r.B.z > 0.f;                                   // n > 0: a finalised cell
  const float a = r.A.z, b = r.A.w, c = r.B.y;
  float vx, vy;                                                   // Sigma^-1 q
  const float m = mahalanobis2(r, vx, vy);
#if defined(NDT_BATCH_ABLATE) && (NDT_BATCH_ABLATE & 4)      // tools only: no transcendental
  const float s = hit ? fmaf(P.nhd2, m, 1.f) : 0.f;
#else
  const float s = hit ? __builtin_amdgcn_exp2f(fmaf(P.nhd2, m, P.lg_d1)) : 0.f;
#endif
  const float jx = P.ty - r.py, jy = r.px - P.tx;                  // dR/dtheta p = perp(p' - t)
  const float vt = fmaf(vx, jx, vy * jy);
  const float ux = fmaf(a, jx, b * jy), uy = fmaf(b, jx, c * jy);   // Sigma^-1 j
  float hxx = a, hxy = b, hyy = c, hxt = ux, hyt = uy, htt = fmaf(jx, ux, jy * uy);
  if (MODE == 1) {   // full Newton Hessian (Biber / Magnusson)
    const float dvx = -P.d2 * vx, dvy = -P.d2 * vy, dvt = -P.d2 * vt;
    hxx = fmaf(dvx, vx, hxx);
    hxy = fmaf(dvx, vy, hxy);
    hyy = fmaf(dvy, vy, hyy);
    hxt = fmaf(dvt, vx, hxt);
    hyt = fmaf(dvt, vy, hyt);
    htt = fmaf(dvt, vt, htt) + fmaf(vy, jx, -vx * jy);
  }
  acc.h0 = fmaf(s, hxx, acc.h0); acc.h1 = fmaf(s, hxy, acc.h1); acc.h2 = fmaf(s, hyy, acc.h2);
  acc.h3 = fmaf(s, hxt, acc.h3); acc.h4 = fmaf(s, hyt, acc.h4); acc.h5 = fmaf(s, htt, acc.h5);
  acc.g0 = fmaf(s, vx, acc.g0);  acc.g1 = fmaf(s, vy, acc.g1);  acc.g2 = fmaf(s, vt, acc.g2);
  acc.s += s;
  acc.n_wave += (int)__popcll(__ballot(hit));                     // s_bcnt1 on the compare mask: no VALU
}

// 128-byte state copy without a struct temporary (a by-value IterState lands in scratch)
__device__ __forceinline__ void copy_state(IterState* dst, const IterState* src, int have_partials) {
  static_assert(sizeof(IterState) == 128, "IterState is copied as 8 x 16 bytes");
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int j = 0; j < 8; ++j) d4[j] = s4[j];
  if (have_partials >= 0) dst->have_partials = have_partials;
}

// The 11 sums of a wave through LDS instead of 11 DPP trees (66 dependent steps): every lane
// parks its 11 values ([j][lane], row stride 68 floats: at most 2-way bank conflicts on the way
// back), then lane 4j+q adds the 16 values of accumulator j whose lane index is q mod 4 (two
// independent chains), and the quad folds with two DPP steps.  Same wave throughout: LDS runs a
// wave's operations in order, so no barrier.  Returns accumulator (lane >> 2)'s total, valid in
// lanes < 44; a fixed order, so sums stay reproducible.
constexpr int kSumRowStride = 68;
__device__ __forceinline__ float wave_reduce11_lds(const float* acc, float* s_t, int lane) {
#pragma unroll
  for (int j = 0; j < kNumAcc - 1; ++j) s_t[j * kSumRowStride + lane] = acc[j];
  __builtin_amdgcn_wave_barrier();
  const int j = lane >> 2, q = lane & 3;
  float a = 0.f, b = 0.f;
  if (lane < 4 * (kNumAcc - 1)) {
    const float* row = s_t + j * kSumRowStride + q;
#pragma unroll
    for (int k = 0; k < 16; k += 2) { a += row[4 * k]; b += row[4 * k + 4]; }
  }
  float v = a + b;
  v += dpp_mov<0xB1, 0xf>(v);
  v += dpp_mov<0x4E, 0xf>(v);
  __builtin_amdgcn_wave_barrier();                     // s_t is rewritten by this wave next iteration
  return v;
}

// Prologue of a chain launch, a wave's share: three partial rows of 256 block entries (pv[v]: this lane's four of row v)
// -> their totals in out[0..2], in a fixed order.  Each lane folds its 4 blocks per row in float64 and parks the 3
// values in LDS (t: 3 x 66 doubles, [row][lane]); lane 16v+q adds the 4 values of row v whose lane index is q mod 16,
// four DPP steps fold the 16 lanes - instead of three 6-step float64 DPP trees on the critical path.  Four waves
// (rows 3w .. 3w+2 into s_red + 3w) and a __syncthreads make the 12 sums of an alignment.
__device__ __forceinline__ void fold_rows12(const float4* pv, double* t, int lane, double* out) {
#pragma unroll
  for (int v = 0; v < 3; ++v)
    t[v * 66 + lane] = (((double)pv[v].x + (double)pv[v].y) + (double)pv[v].z) + (double)pv[v].w;
  __builtin_amdgcn_wave_barrier();
  double a = 0.0;
  if (lane < 48) {
    const double* row = t + (lane >> 4) * 66 + (lane & 15);
    a = (row[0] + row[16]) + (row[32] + row[48]);
  }
  a += dpp_mov<0xB1, 0xf>(a);
  a += dpp_mov<0x4E, 0xf>(a);
  a += dpp_mov<0x124, 0xf>(a);
  a += dpp_mov<0x128, 0xf>(a);                           // every lane of the 16-lane row holds its total
  if ((lane & 15) == 0 && lane < 48) out[lane >> 4] = a;
  __builtin_amdgcn_wave_barrier();                       // where t is the epilogue's buffer, this wave rewrites it
}

// The same fold over the packed table of the single-scan chain (AlignDyn::partials), a wave's share: group g of four sums.
// pv[j] = group g's entry of workgroup 4 lane + j, i.e. its sums 4g .. 4g+3, so component r of pv[0..3] is what
// fold_rows12 finds in one float4 of row 4g + r.  Per sum the operands, the operations and their order are those of
// fold_rows12; with four rows all 64 lanes take part in the second step.  t: 4 x 66 doubles.  Three waves (sums
// 4w .. 4w+3 into s_red + 4w) and a __syncthreads make the 12 sums.
__device__ __forceinline__ void fold_packed4(const float4* pv, double* t, int lane, double* out) {
  t[0 * 66 + lane] = (((double)pv[0].x + (double)pv[1].x) + (double)pv[2].x) + (double)pv[3].x;
  t[1 * 66 + lane] = (((double)pv[0].y + (double)pv[1].y) + (double)pv[2].y) + (double)pv[3].y;
  t[2 * 66 + lane] = (((double)pv[0].z + (double)pv[1].z) + (double)pv[2].z) + (double)pv[3].z;
  t[3 * 66 + lane] = (((double)pv[0].w + (double)pv[1].w) + (double)pv[2].w) + (double)pv[3].w;
  __builtin_amdgcn_wave_barrier();
  const double* row = t + (lane >> 4) * 66 + (lane & 15);
  double a = (row[0] + row[16]) + (row[32] + row[48]);
  a += dpp_mov<0xB1, 0xf>(a);
  a += dpp_mov<0x4E, 0xf>(a);
  a += dpp_mov<0x124, 0xf>(a);
  a += dpp_mov<0x128, 0xf>(a);                           // every lane of the 16-lane row holds its total
  if ((lane & 15) == 0) out[lane >> 4] = a;
  __builtin_amdgcn_wave_barrier();                       // t is the epilogue's buffer: this wave rewrites it
}

// the folded sums -> what gn_update takes
__device__ __forceinline__ void unpack_sums(const double* s_red, double* H, double* g, double& score, int& n_hit) {
#pragma unroll
  for (int j = 0; j < 6; ++j) H[j] = s_red[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) g[j] = s_red[6 + j];
  score = s_red[9];
  n_hit = (int)(s_red[10] + 0.5);
}

// The state a launch leaves behind, field by field into *o (no struct temporary: see copy_state); pad = this launch's
// index.
__device__ __forceinline__ void pack_state(IterState* o, const double* pose, const double* H, const double* g,
                                           double score, int n_hit, int iter, int status, int done, int launch) {
  o->pose[0] = pose[0]; o->pose[1] = pose[1]; o->pose[2] = pose[2];
#pragma unroll
  for (int j = 0; j < 6; ++j) o->H[j] = H[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) o->g[j] = g[j];
  o->score = score;
  o->n_hit = n_hit;
  o->iter = iter;
  o->status = status;
  o->done = done;
  o->have_partials = 1;
  o->pad = launch;
}

// The per-call arguments of a chain, as its first launch takes them (k_begin's)
struct BeginArgs {
  const float* sx;
  const float* sy;
  int n;
  double p0, p1, p2;
  int fixed_iterations;
  IterState* host_state;
  int* host_flag;
  int seq;
};

// What the one writing thread of k_iterate_first leaves for launch 1, field by field (no struct temporary: see
// copy_state): AlignCall as k_begin writes it; state[0] as the old launch 0 left it (the initial state with
// have_partials = 1, pad = launch 0); state[1] as k_begin left it (have_partials = 0); both line-search slots cleared.
// pose: the initial pose with its angle wrapped.
__device__ __forceinline__ void begin_state(IterState* o, const double* pose, int have_partials) {
  o->pose[0] = pose[0]; o->pose[1] = pose[1]; o->pose[2] = pose[2];
#pragma unroll
  for (int j = 0; j < 6; ++j) o->H[j] = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) o->g[j] = 0.0;
  o->score = 0.0;
  o->n_hit = 0;
  o->iter = 0;
  o->status = 0;
  o->done = 0;
  o->have_partials = have_partials;
  o->pad = 0;
}
__device__ __forceinline__ void clear_line_search(LineSearch* o) {
#pragma unroll
  for (int j = 0; j < 3; ++j) { o->base[j] = 0.0; o->step[j] = 0.0; }
  o->score = 0.0; o->alpha = 0.0; o->trials = 0; o->valid = 0;
}
__device__ __forceinline__ void begin_chain(AlignCall* call, AlignDyn* dyn, const BeginArgs& b, const double* pose) {
  call->seq = b.seq;
  call->pad = 0;
  call->sx = b.sx;
  call->sy = b.sy;
  call->n = b.n;
  call->fixed_iterations = b.fixed_iterations;
  call->host_state = b.host_state;
  call->host_flag = b.host_flag;
  begin_state(&dyn->state[0], pose, 1);
  begin_state(&dyn->state[1], pose, 0);
  clear_line_search(&dyn->ls[0]);
  clear_line_search(&dyn->ls[1]);
}

// ---------------------------------------------------------------- a4-a8 iterate kernel
// Launch k (parity = k & 1) consumes state[parity^1] and partials[parity^1] written by
// launch k-1 and produces state[parity], partials[parity].  Always kMaxBlocks workgroups
// (one per CU); a workgroup without points contributes a zero partial row.
//
// The iteration is a serial dependence chain (reduce -> solve -> transform -> gather ->
// reduce), so the kernel is written to keep the number of dependent memory round trips behind
// the argument load at two: the partial rows, then the previous state with the read-only
// scalars in one s_load batch, then the first source points are all requested before anything
// waits for the rows; the cell-record gather is the second.
// EXP is an ablation mask for tools/exp_iter.hip only (1: no reduce/solve, 2: no body,
// 4: no epilogue tree, 8: empty) and tools/exp_tail.hip (16: the row-per-sum table with twelve 4-byte stores per
// workgroup, as it was before the table was packed; 32: packed, but slot = workgroup); the library instantiates EXP = 0.
//
// The text of the launch is ndt2d_iterate_text.hpp, shared with k_iterate_first (launch 0 of a chain, FIRST = 1).
template <int MODE, int EXP = 0, int THREADS = kBlock, int NG = 1>
__global__ __launch_bounds__(THREADS) void k_iterate(const AlignStatic* __restrict__ st,
                                                    const AlignCall* __restrict__ call,
                                                    AlignDyn* __restrict__ dyn, int parity) {
  constexpr int FIRST = 0;
  const BeginArgs b{};
#include "ndt2d_iterate_text.hpp"
}

// Launch 0 of a single-scan chain with k_begin folded in: evaluates at the initial pose (partials[0]) straight from its
// arguments, and its workgroup 0 writes the per-call context and both state slots for launch 1 (parity 1) to find
// across the kernel boundary.  No workgroup of this launch reads any of them.  The same text as k_iterate.
template <int MODE, int THREADS = kBlock, int NG = 1>
__global__ __launch_bounds__(THREADS) void k_iterate_first(const AlignStatic* __restrict__ st, AlignCall* __restrict__ call,
                                                          AlignDyn* __restrict__ dyn, const float* sx0, const float* sy0, int n0,
                                                          double p0, double p1, double p2, int fixed0, IterState* host_state0,
                                                          int* host_flag0, int seq) {
  constexpr int FIRST = 1, EXP = 0, parity = 0;
  const BeginArgs b{sx0, sy0, n0, p0, p1, p2, fixed0, host_state0, host_flag0, seq};
#include "ndt2d_iterate_text.hpp"
}

// ------------------------------------------------------------- scan format (section 8f rank 4)
// Range/bearing -> Cartesian SoA.  One sincos per beam from the beam index (no accumulated
// angle error); invalid returns become NaN points, which every kernel above ignores.
__global__ __launch_bounds__(kBlock) void k_polar_to_points(const float* __restrict__ r, size_t n, double angle_min,
                                                             double angle_inc, float range_min, float range_max,
                                                             float* __restrict__ x, float* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const float ri = r[i];
    double s, c;
    sincos(fma((double)i, angle_inc, angle_min), &s, &c);
    const bool ok = isfinite(ri) & (ri >= range_min) & (ri <= range_max);
    x[i] = ok ? (float)((double)ri * c) : NAN;
    y[i] = ok ? (float)((double)ri * s) : NAN;
  }
}

}  // namespace ndt

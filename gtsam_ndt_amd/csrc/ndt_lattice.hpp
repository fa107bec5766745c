// The target-side lattice rule, stated once for host and device (docs/ALGORITHM.md sections 2.2, 2.6, 2.19): the grid of
// a cloud, the cell of a target point, and what the point adds to its cell's exact sums.  Plain C++, no HIP types and no
// handle: every build path and the host geometry call these functions, and tests/cpp/lattice_main.cpp runs them under
// the host sanitizers.  (The source side is stated elsewhere: how a pose becomes a rotation in ndt_pose.hpp, and the
// lookups, which clamp instead of testing, in image_point / image_key of ndt2d_kernels.hpp and voxel_of3 / voxel_clamped3 of
// ndt3d_kernels.hpp.)
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define NDT_LATTICE_FN __host__ __device__ __forceinline__
#else
#define NDT_LATTICE_FN inline
#endif

namespace ndt {

// ---------------------------------------------------------------- 1. the lattice of a cloud, one axis
// (oracle/ndt2d.py grid_geometry, oracle/ndt3d.py grid_geometry3.)  The limits on k differ between the callers (storage,
// launch bounds, the LDS carve) and stay with them: k may be negative, huge or not a number, so a caller compares it
// before it converts it.  An axis with an accepted k has k + 2 cells: one guard cell either side.
struct LatticeAxis {
  double base;     // floor(min / c)
  float origin;    // lattice_origin(base, 0, c)
  float k;         // floor((max - origin) * inv_c), in float32 as the kernels place a point
};
NDT_LATTICE_FN float lattice_inv_c(double c) { return (float)(1.0 / c); }
// the origin `shift` cells further down; grid q of the four overlapping ones is shifted by half a cell along x (axis 0)
// when q is odd and along y (axis 1) when q >= 2
NDT_LATTICE_FN float lattice_origin(double base, double shift, double c) { return (float)((base - 1.0 - shift) * c); }
NDT_LATTICE_FN double overlap_shift(int q, int axis) { return 0.5 * (double)((q >> axis) & 1); }
NDT_LATTICE_FN LatticeAxis lattice_axis(float mn, float mx, double c) {
  LatticeAxis a;
  a.base = std::floor((double)mn / c);
  a.origin = lattice_origin(a.base, 0.0, c);
  a.k = std::floor((mx - a.origin) * lattice_inv_c(c));
  return a;
}

// ---------------------------------------------------------------- 2. the cell of a target point
// f = (p - o) * inv_c in float32; inside when RING <= f < extent - RING; the index is (int)f.  RING = 1 in 2D: the
// source-side lookup clamps keys onto the grid, so every out-of-range, NaN or dead-lane lookup lands on a cell of the
// outermost ring, which must therefore never receive a target point (ndt2d_kernels.hpp).  RING = 0 in 3D.
NDT_LATTICE_FN float lattice_coord(float p, float o, float inv_c) { return (p - o) * inv_c; }
// the upper limit of an axis as the float32 the test compares with (a type of its own: an extent cannot pass for it)
template <int RING>
struct LatticeLimit {
  float v;
  NDT_LATTICE_FN explicit LatticeLimit(int extent) : v((float)(extent - RING)) {}
};
// the index of a point that is known to be inside (it was binned by cell_of)
NDT_LATTICE_FN int lattice_index(float p, float o, float inv_c) { return (int)lattice_coord(p, o, inv_c); }

// The indices are valid only when the result is true (a NaN, an infinity or a far point converts to no integer).
template <int RING>
NDT_LATTICE_FN bool cell_of(float px, float py, float ox, float oy, float inv_c, LatticeLimit<RING> hx, LatticeLimit<RING> hy,
                            int& ix, int& iy) {
  const float fx = lattice_coord(px, ox, inv_c), fy = lattice_coord(py, oy, inv_c);
  const bool in = (fx >= (float)RING) & (fx < hx.v) & (fy >= (float)RING) & (fy < hy.v);
  ix = in ? (int)fx : -1;
  iy = in ? (int)fy : -1;
  return in;
}
template <int RING>
NDT_LATTICE_FN bool cell_of(float px, float py, float pz, float ox, float oy, float oz, float inv_c, LatticeLimit<RING> hx,
                            LatticeLimit<RING> hy, LatticeLimit<RING> hz, int& ix, int& iy, int& iz) {
  const float fx = lattice_coord(px, ox, inv_c), fy = lattice_coord(py, oy, inv_c), fz = lattice_coord(pz, oz, inv_c);
  const bool in = (fx >= (float)RING) & (fx < hx.v) & (fy >= (float)RING) & (fy < hy.v) & (fz >= (float)RING) & (fz < hz.v);
  ix = in ? (int)fx : -1;
  iy = in ? (int)fy : -1;
  iz = in ? (int)fz : -1;
  return in;
}

// ---------------------------------------------------------------- 3. what a point adds to its cell's exact sums
// Cell-centred coordinates quantised to c * 2^-22 (fix_scale = 2^22 / c).  The centre is rounded once.
NDT_LATTICE_FN double cell_centre(float o, int i, double cell) { return __builtin_fma((double)i + 0.5, cell, (double)o); }
// |U| <= 2^21 for a point inside its cell, so the conversion is the single-instruction
// v_cvt_i32_f64 (an f64 -> i64 conversion is emulated) and products are 32 x 32 -> 64 bit.
NDT_LATTICE_FN int fix_coord(float p, double centre, double fix_scale) {
  return (int)__builtin_rint(((double)p - centre) * fix_scale);
}
NDT_LATTICE_FN unsigned long long prod64(int a, int b) { return (unsigned long long)((long long)a * (long long)b); }
NDT_LATTICE_FN unsigned long long term64(int u) { return (unsigned long long)(long long)u; }

// add(j, term) for the cell's sums in storage order: 2D x y xx xy yy, 3D x y z xx xy xz yy yz zz.  The callable holds
// the destination and the sign only.
template <class Add>
NDT_LATTICE_FN void point_terms(float px, float py, float ox, float oy, int ix, int iy, double cell, double fix_scale,
                                Add&& add) {
  const int ux = fix_coord(px, cell_centre(ox, ix, cell), fix_scale);
  const int uy = fix_coord(py, cell_centre(oy, iy, cell), fix_scale);
  add(0, term64(ux)); add(1, term64(uy));
  add(2, prod64(ux, ux)); add(3, prod64(ux, uy)); add(4, prod64(uy, uy));
}
template <class Add>
NDT_LATTICE_FN void point_terms(float px, float py, float pz, float ox, float oy, float oz, int ix, int iy, int iz,
                                double cell, double fix_scale, Add&& add) {
  const int ux = fix_coord(px, cell_centre(ox, ix, cell), fix_scale);
  const int uy = fix_coord(py, cell_centre(oy, iy, cell), fix_scale);
  const int uz = fix_coord(pz, cell_centre(oz, iz, cell), fix_scale);
  add(0, term64(ux)); add(1, term64(uy)); add(2, term64(uz));
  add(3, prod64(ux, ux)); add(4, prod64(ux, uy)); add(5, prod64(ux, uz));
  add(6, prod64(uy, uy)); add(7, prod64(uy, uz)); add(8, prod64(uz, uz));
}

}  // namespace ndt

// Stand-alone driver of the target-side lattice rule (gtsam_ndt_amd/csrc/ndt_lattice.hpp) for tests/test_lattice_host.py,
// which builds it with -fsanitize=address,undefined: the functions the build kernels and the host geometry call, on the
// CPU.  float32 values travel as their bit patterns, the cell size as a decimal that reads back exactly.
//   G dim c  (min max) per axis      -> "none" (no finite point), "capacity" (an extent beyond this caller's limits), or
//                                        "ok" and (origin bits, extent) per axis
//   P dim c  (origin extent p) per axis -> "out", or "in", the indices, the residuals and the 5 / 9 terms (signed)
// The ring is the library's: 1 in 2D, 0 in 3D.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ndt_lattice.hpp"

namespace {

float from_bits(std::uint32_t b) { float f; std::memcpy(&f, &b, sizeof f); return f; }
std::uint32_t to_bits(float f) { std::uint32_t b; std::memcpy(&b, &f, sizeof b); return b; }

// the limits of ndt3d_set_target on the host: 1e7 cells per axis, 2^27 cells in all
bool geometry(int dim, double c) {
  float mn[3], mx[3];
  for (int a = 0; a < dim; ++a) {
    std::uint32_t lo, hi;
    if (std::scanf("%" SCNu32 " %" SCNu32, &lo, &hi) != 2) return false;
    mn[a] = from_bits(lo); mx[a] = from_bits(hi);
  }
  std::uint32_t origin[3];
  int ext[3];
  double ncell = 1.0;
  for (int a = 0; a < dim; ++a) {
    if (!(mn[a] <= mx[a])) { std::puts("none"); return true; }
    const ndt::LatticeAxis A = ndt::lattice_axis(mn[a], mx[a], c);
    if (!(A.k >= 0.f) || A.k > 1e7f) { std::puts("capacity"); return true; }
    origin[a] = to_bits(A.origin);
    ext[a] = (int)A.k + 2;
    ncell *= ext[a];
  }
  if (ncell > 134217728.0) { std::puts("capacity"); return true; }
  std::printf("ok");
  for (int a = 0; a < dim; ++a) std::printf(" %" PRIu32 " %d", origin[a], ext[a]);
  std::printf("\n");
  return true;
}

template <int DIM, int RING>
bool point(double c) {
  float o[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
  int ext[3] = {1, 1, 1}, i[3] = {0, 0, 0};
  for (int a = 0; a < DIM; ++a) {
    std::uint32_t ob, pb;
    if (std::scanf("%" SCNu32 " %d %" SCNu32, &ob, &ext[a], &pb) != 3) return false;
    o[a] = from_bits(ob); p[a] = from_bits(pb);
  }
  const float inv_c = ndt::lattice_inv_c(c);
  const double fix_scale = 4194304.0 / c;
  using Limit = ndt::LatticeLimit<RING>;
  bool in;
  if (DIM == 2) in = ndt::cell_of(p[0], p[1], o[0], o[1], inv_c, Limit(ext[0]), Limit(ext[1]), i[0], i[1]);
  else in = ndt::cell_of(p[0], p[1], p[2], o[0], o[1], o[2], inv_c, Limit(ext[0]), Limit(ext[1]), Limit(ext[2]), i[0], i[1], i[2]);
  if (!in) { std::puts("out"); return true; }
  long long t[9];
  auto add = [&](int j, unsigned long long v) { t[j] = (long long)v; };
  if (DIM == 2) ndt::point_terms(p[0], p[1], o[0], o[1], i[0], i[1], c, fix_scale, add);
  else ndt::point_terms(p[0], p[1], p[2], o[0], o[1], o[2], i[0], i[1], i[2], c, fix_scale, add);
  std::printf("in");
  for (int a = 0; a < DIM; ++a) std::printf(" %d", i[a]);
  for (int a = 0; a < DIM; ++a) std::printf(" %d", ndt::fix_coord(p[a], ndt::cell_centre(o[a], i[a], c), fix_scale));
  for (int j = 0; j < (DIM == 2 ? 5 : 9); ++j) std::printf(" %lld", t[j]);
  std::printf("\n");
  return true;
}

}  // namespace

int main() {
  char cmd;
  int dim;
  double c;
  while (std::scanf(" %c %d %lf", &cmd, &dim, &c) == 3) {
    if ((dim != 2 && dim != 3) || !(c > 0.0)) return 2;
    bool ok = false;
    if (cmd == 'G') ok = geometry(dim, c);
    else if (cmd == 'P') ok = dim == 2 ? point<2, 1>(c) : point<3, 0>(c);
    if (!ok) return 2;
  }
  return 0;
}

// The lattice of a coarsened submap, one axis at a time (docs/ALGORITHM.md section 2.17): host arithmetic only, no HIP, so
// that tests/cpp/coarsen_geom_main.cpp runs it under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

namespace ndt {

struct CoarsenAxis {
  long long k0;    // fine origin in fine cells: rint(o / c)
  long long K0;    // coarse origin in fine cells: f * floor((k0 + 1 - f) / f), a multiple of f
  int off;         // k0 - K0, in [f - 1, 2f - 2]: fine cell ix lies in coarse cell (off + ix) / f at position (off + ix) % f
  int extent;      // coarse cells: (off + W - 2) / f + 2
  float origin;    // (float)(K0 * c)
};

// Origins beyond 2^40 cells are no grid of this library (2^27 cells at most, float32 coordinates).
constexpr double kCoarsenMaxOriginCells = 1099511627776.0;

// false: f is not 2 or 4, W < 1, or the origin is not finite / too far out in cells for the integers here.
inline bool coarsen_axis(float o, double c, int W, int f, CoarsenAxis* out) {
  if ((f != 2 && f != 4) || W < 1 || !(c > 0.0)) return false;
  const double q = (double)o / c;
  if (!(std::fabs(q) <= kCoarsenMaxOriginCells)) return false;
  const long long k0 = std::llrint(q);
  const long long a = k0 + 1 - f;
  const long long fl = a >= 0 ? a / f : -((-a + f - 1) / f);   // floor division
  const long long K0 = fl * f;
  out->k0 = k0;
  out->K0 = K0;
  out->off = (int)(k0 - K0);
  out->extent = (int)(((long long)out->off + W - 2) / f) + 2;    // off + W - 2 >= f - 2 >= 0
  out->origin = (float)((double)K0 * c);
  return true;
}

// The factor between two cell sizes: 2 or 4 when coarse == f * fine exactly (in double), else 0.
inline int coarsen_factor(double fine, double coarse) {
  if (coarse == 2.0 * fine) return 2;
  if (coarse == 4.0 * fine) return 4;
  return 0;
}

}  // namespace ndt

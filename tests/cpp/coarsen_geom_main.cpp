// Stand-alone driver of the host arithmetic of submap coarsening (gtsam_ndt_amd/csrc/ndt_coarsen_geom.hpp) for
// tests/test_coarsen_geom_sanitize.py, which builds it with -fsanitize=address,undefined.
// Reads lines "origin cell W f" from stdin; prints "ok k0 K0 off extent origin" (origin as its float32 bit pattern) or "refused".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ndt_coarsen_geom.hpp"

int main() {
  double origin, cell;
  int W, f;
  while (std::scanf("%lf %lf %d %d", &origin, &cell, &W, &f) == 4) {
    ndt::CoarsenAxis ax;
    if (!ndt::coarsen_axis((float)origin, cell, W, f, &ax)) { std::puts("refused"); continue; }
    std::uint32_t bits;
    std::memcpy(&bits, &ax.origin, sizeof bits);
    std::printf("ok %lld %lld %d %d %" PRIu32 "\n", ax.k0, ax.K0, ax.off, ax.extent, bits);
  }
  std::printf("factors %d %d %d %d %d\n", ndt::coarsen_factor(0.5, 1.0), ndt::coarsen_factor(0.5, 2.0), ndt::coarsen_factor(0.5, 1.5),
              ndt::coarsen_factor(0.5, 0.5), ndt::coarsen_factor(0.1, 0.2));
  return 0;
}

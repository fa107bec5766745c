// Stand-alone driver of the source-side pose rule (gtsam_ndt_amd/csrc/ndt_pose.hpp) for tests/test_pose_host.py, which
// builds it with -fsanitize=address,undefined and -ffp-contract=off: the functions every kernel and host site calls, on
// the CPU in their host form.  float64 values travel as their bit patterns.
//   R sa ca sb cb sg cg  -> the nine entries of R = Rz Ry Rx, then the nine of dR/dpitch
//   W t                  -> wrap_angle(t)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ndt_pose.hpp"

namespace {

double from_bits(std::uint64_t b) { double d; std::memcpy(&d, &b, sizeof d); return d; }
std::uint64_t to_bits(double d) { std::uint64_t b; std::memcpy(&b, &d, sizeof b); return b; }

bool read(double* v, int n) {
  for (int i = 0; i < n; ++i) {
    std::uint64_t b;
    if (std::scanf("%" SCNu64, &b) != 1) return false;
    v[i] = from_bits(b);
  }
  return true;
}

}  // namespace

int main() {
  char cmd;
  while (std::scanf(" %c", &cmd) == 1) {
    if (cmd == 'R') {
      double v[6], R[9], Rb[9];
      if (!read(v, 6)) return 2;
      ndt::rot3_products(v[0], v[1], v[2], v[3], v[4], v[5], R);
      ndt::rot3_pitch_products(v[0], v[1], v[2], v[3], v[4], v[5], Rb);
      for (int i = 0; i < 9; ++i) std::printf("%" PRIu64 " ", to_bits(R[i]));
      for (int i = 0; i < 9; ++i) std::printf("%" PRIu64 "%c", to_bits(Rb[i]), i == 8 ? '\n' : ' ');
    } else if (cmd == 'W') {
      double t;
      if (!read(&t, 1)) return 2;
      std::printf("%" PRIu64 "\n", to_bits(ndt::wrap_angle(t)));
    } else {
      return 2;
    }
  }
  return 0;
}

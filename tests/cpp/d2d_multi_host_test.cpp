// Host-only check of the plan of an ndt2d_align_map_multi call (csrc/ndt_host.hpp: distinct_pointers, capped_blocks,
// pow2_at_least).  No GPU, no HIP call.  Prints "ok" and returns 0, or says which expectation failed.
#include <cstdio>
#include <vector>

#include "ndt_host.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) { std::printf("failed: %s\n", what); ++failures; }
}

}  // namespace

int main() {
  // blocks of a map-to-map launch: one component per lane of 256-thread workgroups, at most 256 of them
  expect(ndt::capped_blocks(1, 256, 256) == 1, "1 component -> 1 workgroup");
  expect(ndt::capped_blocks(256, 256, 256) == 1, "256 components -> 1 workgroup");
  expect(ndt::capped_blocks(257, 256, 256) == 2, "257 components -> 2 workgroups");
  expect(ndt::capped_blocks(65536, 256, 256) == 256, "65536 components -> 256 workgroups");
  expect(ndt::capped_blocks(65537, 256, 256) == 256, "65537 components: capped");
  expect(ndt::capped_blocks(1ll << 27, 256, 256) == 256, "2^27 components: capped");
  expect(ndt::capped_blocks(0x7fffffffll, 256, 256) == 256, "2^31 - 1 components: no overflow");
  for (int v = 1; v <= 256; ++v) {
    const int p = ndt::pow2_at_least(v);
    expect(p >= v && p < 2 * v && (p & (p - 1)) == 0, "pow2_at_least");
  }
  // distinct handles, first occurrence first; the heap copies put every access under the address sanitizer
  int a = 0, b = 0, c = 0;
  {
    std::vector<int*> in = {&a, &b, &a, &c, &b, &a}, out(in.size(), nullptr);
    const int n = ndt::distinct_pointers(in.data(), (int)in.size(), out.data());
    expect(n == 3 && out[0] == &a && out[1] == &b && out[2] == &c, "three distinct of six");
  }
  {
    std::vector<int*> in(64, &b), out(64, nullptr);
    expect(ndt::distinct_pointers(in.data(), 64, out.data()) == 1 && out[0] == &b, "a multi-start names one handle");
  }
  {
    std::vector<int> v(64);
    std::vector<int*> in, out(64, nullptr);
    for (int& x : v) in.push_back(&x);
    expect(ndt::distinct_pointers(in.data(), 64, out.data()) == 64 && out[63] == &v[63], "64 different handles");
  }
  {
    std::vector<int*> in = {&c}, out(1, nullptr);
    expect(ndt::distinct_pointers(in.data(), 1, out.data()) == 1 && out[0] == &c, "one start");
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}

// Host-only check of the plan of an ndt2d_align_map_multi / ndt3d_align_map_multi call (csrc/ndt_host.hpp:
// distinct_pointers, capped_blocks, pow2_at_least, plan_map_starts).  No GPU, no HIP call.  Prints "ok" and returns 0, or
// says which expectation failed.
#include <cstdio>
#include <memory>
#include <vector>

#include "ndt_host.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) { std::printf("failed: %s\n", what); ++failures; }
}

// stand-ins for StartPoses / StartPoses3, StartMaps / StartMaps3 and a source handle
constexpr int kSlots = 64;
template <int P> struct Poses { double p[kSlots][P]; };
struct Maps { const float* comp[kSlots]; int n[kSlots]; int blocks[kSlots]; };
struct Source { const float* d_comp; int n_comp; };

// One call of plan_map_starts with pose length P: start k from src[k], pose entries 100 k + j.  Checks what every plan
// promises (poses copied, slots of m and beyond untouched, a start is live exactly if its source has a component and the
// target a cell, its blocks, the maximum) and returns the number of live starts.
template <int P>
int walk_plan(const std::vector<Source*>& src, bool target_has_cells, int want_max_blocks, const char* what) {
  const int m = (int)src.size();
  std::vector<double> init((size_t)P * m);                 // exactly P m values: a read past them is the sanitizer's
  for (int k = 0; k < m; ++k) for (int j = 0; j < P; ++j) init[P * k + j] = 100.0 * k + j;
  auto sp = std::make_unique<Poses<P>>();
  auto sm = std::make_unique<Maps>();
  for (int k = 0; k < kSlots; ++k) {
    for (int j = 0; j < P; ++j) sp->p[k][j] = -1.0;
    sm->comp[k] = nullptr; sm->n[k] = 0; sm->blocks[k] = 0;
  }
  int max_blocks = -7;
  const int live = ndt::plan_map_starts(src.data(), init.data(), m, target_has_cells, 256, 256, sp.get(), sm.get(), &max_blocks);
  int want_live = 0;
  bool ok = true;
  for (int k = 0; k < kSlots; ++k) {
    for (int j = 0; j < P; ++j) ok = ok && sp->p[k][j] == (k < m ? 100.0 * k + j : -1.0);
    const int n = k < m && target_has_cells ? src[k]->n_comp : 0;
    if (n > 0) {
      ++want_live;
      ok = ok && sm->comp[k] == src[k]->d_comp && sm->n[k] == n && sm->blocks[k] == ndt::capped_blocks(n, 256, 256);
    } else {
      ok = ok && sm->comp[k] == nullptr && sm->n[k] == 0 && sm->blocks[k] == 0;      // answered on the spot
    }
  }
  expect(ok, what);
  expect(live == want_live, what);
  expect(max_blocks == want_max_blocks, what);
  return live;
}

template <int P>
void plan_cases() {
  const float list[4] = {};
  Source one{list, 1}, small{list + 1, 300}, big{list + 2, 65536}, over{list + 3, 65537}, empty{nullptr, 0};
  expect(walk_plan<P>({&small}, true, 2, "m = 1") == 1, "m = 1: live");
  expect(walk_plan<P>({&one, &small, &one}, true, 2, "m = 3") == 3, "m = 3: all live");
  {
    std::vector<Source> v(64);
    std::vector<Source*> in;
    for (int k = 0; k < 64; ++k) { v[k] = Source{list, 256 * k + 1}; in.push_back(&v[k]); }   // 1 .. 64 workgroups
    expect(walk_plan<P>(in, true, 64, "m = 64, 64 sources") == 64, "m = 64: all live");
  }
  expect(walk_plan<P>(std::vector<Source*>(64, &small), true, 2, "one source named 64 times") == 64, "a multi-start: all live");
  expect(walk_plan<P>({&small, &empty, &one, &empty, &big}, true, 256, "sources without a component among live ones") == 3,
         "two of five answered on the spot");
  expect(walk_plan<P>({&empty, &empty}, true, 1, "no source has a component") == 0, "no live start");
  expect(walk_plan<P>({&small, &big, &one}, false, 1, "a target without a valid cell") == 0, "every start answered");
  expect(walk_plan<P>({&over}, true, 256, "65537 components: kMaxBlocks workgroups") == 1, "capped start is live");
  expect(walk_plan<P>({&one, &over, &small}, true, 256, "max_blocks of a capped set") == 3, "capped set: all live");
  expect(walk_plan<P>({&one, &small, &one, &empty}, true, 2, "max_blocks of a mixed set") == 3, "mixed set");
  expect(walk_plan<P>({&one, &one}, true, 1, "max_blocks of single-workgroup starts") == 2, "two small starts");
}

}  // namespace

int main() {
  plan_cases<3>();
  plan_cases<6>();
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

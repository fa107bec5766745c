// Host-only check of the device-free half of the batch and multi-device contexts (csrc/ndt_host.hpp: pair_offsets_ok,
// plan_shards, rebase_shard, gather_layout, ungather).  No GPU, no HIP call.  Every array has exactly the size its
// function may read or write, so that an access past it is the sanitizer's to find.  Prints "ok" and returns 0, or says
// which expectation failed.
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ndt_host.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) { std::printf("failed: %s\n", what); ++failures; }
}

constexpr uint64_t kBatchMaxCloud = 1ull << 29;      // csrc/ndt2d_batch.hpp's

// offsets of clouds of the given sizes: sizes.size() + 1 entries
std::vector<uint64_t> offsets(const std::vector<uint64_t>& sizes) {
  std::vector<uint64_t> off(sizes.size() + 1, 0);
  std::partial_sum(sizes.begin(), sizes.end(), off.begin() + 1);
  return off;
}

// ragged pairs, every seventh target and every fifth source empty
std::vector<uint64_t> ragged(size_t n, uint64_t mul, size_t empty_every) {
  std::vector<uint64_t> s(n);
  for (size_t k = 0; k < n; ++k) s[k] = k % empty_every == empty_every - 1 ? 0 : 100 + mul * (k % 13);
  return s;
}

// what every plan promises: it begins at 0, ends at n_pairs and never steps back
bool plan_is_a_split(const std::vector<uint64_t>& begin, size_t n_pairs) {
  bool ok = begin.front() == 0 && begin.back() == n_pairs;
  for (size_t d = 0; d + 1 < begin.size(); ++d) ok = ok && begin[d] <= begin[d + 1];
  return ok;
}

void offsets_and_plan(size_t n_pairs) {
  const std::vector<uint64_t> toff = offsets(ragged(n_pairs, 37, 7)), soff = offsets(ragged(n_pairs, 11, 5));
  expect(ndt::pair_offsets_ok(toff.data(), soff.data(), n_pairs, kBatchMaxCloud), "ragged offsets with empty pairs are accepted");
  for (int shards : {1, 2, 3, 8, 300}) {                 // 300: more shards than pairs at every n_pairs here
    std::vector<uint64_t> begin(shards + 1, ~0ull), hinted(shards + 1, ~0ull);
    expect(ndt::plan_shards(shards, toff.data(), soff.data(), n_pairs, 30, nullptr, begin.data()), "a plan is made");
    expect(plan_is_a_split(begin, n_pairs), "the plan is a split of the pairs");
    if (shards > (int)n_pairs) {
      size_t used = 0;
      for (int d = 0; d < shards; ++d) used += begin[d + 1] > begin[d];
      expect(used <= n_pairs, "more shards than pairs: the others are empty");
    }
    const std::vector<int32_t> zero(n_pairs, 0);         // no per-pair hint anywhere: the un-hinted plan
    expect(ndt::plan_shards(shards, toff.data(), soff.data(), n_pairs, 30, zero.data(), hinted.data()) && hinted == begin,
           "per-pair hints that are all zero give the un-hinted plan");
    std::vector<int32_t> slow(n_pairs, 0);
    slow[0] = 3000;                                      // the first pair takes 100 times the iterations
    expect(ndt::plan_shards(shards, toff.data(), soff.data(), n_pairs, 30, slow.data(), hinted.data()) &&
           plan_is_a_split(hinted, n_pairs), "a hinted plan is a split");
    if (shards == 2 && n_pairs >= 3) expect(hinted[1] <= begin[1], "a slow first pair shortens the first shard");
  }
  // rebasing the shard k0 .. k1: both ends, one in the middle, and empty shards at either end
  const size_t mid = n_pairs / 2;
  const size_t cases[][2] = {{0, n_pairs}, {0, mid}, {mid, n_pairs}, {0, 0}, {n_pairs, n_pairs}, {mid, mid}};
  for (const auto& c : cases) {
    const size_t k0 = c[0], k1 = c[1];
    std::vector<uint64_t> out(k1 - k0 + 1, ~0ull);
    ndt::rebase_shard(toff.data(), k0, k1, out.data());
    bool ok = out[0] == 0;
    for (size_t k = k0; k < k1; ++k) ok = ok && out[k - k0 + 1] - out[k - k0] == toff[k + 1] - toff[k];
    expect(ok, "a rebased shard starts at 0 and keeps its clouds' sizes");
    expect(ndt::pair_offsets_ok(out.data(), out.data(), k1 - k0, kBatchMaxCloud), "a rebased shard is a valid batch");
  }
  // a decreasing offset, in the target's or the source's array, first or last
  for (size_t at : {(size_t)0, n_pairs - 1}) {
    std::vector<uint64_t> bad = toff;
    for (size_t k = at + 1; k <= n_pairs; ++k) bad[k] += 5;       // room to step back without wrapping
    bad[at] = bad[at + 1] + 1;
    std::vector<uint64_t> begin(3, 77);
    expect(!ndt::pair_offsets_ok(bad.data(), soff.data(), n_pairs, kBatchMaxCloud), "a decreasing target offset is rejected");
    expect(!ndt::pair_offsets_ok(toff.data(), bad.data(), n_pairs, kBatchMaxCloud), "a decreasing source offset is rejected");
    expect(!ndt::plan_shards(2, bad.data(), soff.data(), n_pairs, 30, nullptr, begin.data()) && begin[0] == 77 && begin[2] == 77,
           "no plan for a decreasing offset, nothing written");
  }
  // a cloud of kBatchMaxCloud + 1 points (offsets only: nobody looks at a point)
  for (size_t at : {(size_t)0, n_pairs - 1}) {
    std::vector<uint64_t> sizes = ragged(n_pairs, 37, 7);
    sizes[at] = kBatchMaxCloud;
    const std::vector<uint64_t> full = offsets(sizes);
    expect(ndt::pair_offsets_ok(full.data(), soff.data(), n_pairs, kBatchMaxCloud), "a cloud of kBatchMaxCloud points is accepted");
    sizes[at] = kBatchMaxCloud + 1;
    const std::vector<uint64_t> over = offsets(sizes);
    expect(!ndt::pair_offsets_ok(over.data(), soff.data(), n_pairs, kBatchMaxCloud), "a target of kBatchMaxCloud + 1 points is rejected");
    expect(!ndt::pair_offsets_ok(soff.data(), over.data(), n_pairs, kBatchMaxCloud), "a source of kBatchMaxCloud + 1 points is rejected");
  }
}

// The gather of shards of 3, 0 and 5 pairs with rows of row_bytes: layout, then the way of a row from its shard's send
// buffer through the receive buffer into the caller's array
void gather(size_t row_bytes) {
  const std::vector<size_t> n = {3, 0, 5};
  const ndt::GatherLayout g = ndt::gather_layout(n.data(), (int)n.size(), row_bytes);
  expect(g.stride == 5 && g.total == 8, "the stride is the longest shard, the total every pair");
  expect(g.count == 5 * row_bytes / 8, "the count is in doubles");
  const size_t w = row_bytes / 8;                      // doubles per row
  std::vector<double> recv(n.size() * g.count, 0.0);   // what an all-gather of `count` doubles per shard leaves
  for (size_t d = 0; d < n.size(); ++d)
    for (size_t r = 0; r < n[d]; ++r)
      for (size_t j = 0; j < w; ++j) recv[(d * g.stride + r) * w + j] = 1000.0 * (d + 1) + 10.0 * r + 0.001 * j;
  std::vector<double> out(g.total * w, -1.0);
  int copies = 0;
  const int st = ndt::ungather(n.data(), (int)n.size(), g.stride, 0, [&](size_t to, size_t from, size_t rows) {
    for (size_t j = 0; j < rows * w; ++j) out[to * w + j] = recv[from * w + j];
    ++copies;
    return 0;
  });
  expect(st == 0 && copies == 2, "one copy per shard that has rows");
  bool ok = true;
  size_t k = 0;
  for (size_t d = 0; d < n.size(); ++d)
    for (size_t r = 0; r < n[d]; ++r, ++k)
      for (size_t j = 0; j < w; ++j) ok = ok && out[k * w + j] == 1000.0 * (d + 1) + 10.0 * r + 0.001 * j;
  expect(ok && k == g.total, "global pair order, padding dropped");
  const int failed = ndt::ungather(n.data(), (int)n.size(), g.stride, 0, [&](size_t, size_t from, size_t) { return from == 0 ? 7 : 0; });
  expect(failed == 7, "the first failing copy's status comes back");
  const std::vector<size_t> none = {0, 0};
  expect(ndt::gather_layout(none.data(), 2, row_bytes).total == 0, "no pair anywhere");
}

}  // namespace

int main() {
  offsets_and_plan(1);
  offsets_and_plan(3);
  offsets_and_plan(257);
  {   // every pair empty: offsets all zero
    const std::vector<uint64_t> zero(4, 0);
    std::vector<uint64_t> begin(3, ~0ull);
    expect(ndt::pair_offsets_ok(zero.data(), zero.data(), 3, kBatchMaxCloud), "three empty pairs are accepted");
    expect(ndt::plan_shards(2, zero.data(), zero.data(), 3, 0, nullptr, begin.data()) && plan_is_a_split(begin, 3), "and split");
  }
  gather(136);      // ndt2d_result
  gather(408);      // ndt3d_result
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}

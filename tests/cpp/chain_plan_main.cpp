// Host-only check of the plan of a single-pair launch chain (csrc/ndt_host.hpp: chain_plan).  No GPU, no HIP call: the
// plan is a pure function of the override, the parameters, the two tuning knobs and whether launch 0 stands in front of
// the graph.  It is compared, over every combination of the values below, with a verbatim restatement of the four
// computations it replaced (the 2D and the 3D scan chain, the 2D and the 3D map-to-map chain), each on the rows that
// caller can reach.  Prints "ok" and returns 0, or says which expectation failed.
#include <cstdio>

#include "ndt_host.hpp"

using ndt::ChainPlan;

namespace {

int failures = 0;

struct Old {
  int fixed, K, first;
  bool chunked;      // the first launch gets the host state and flag pointers; chunk_run_begin follows
  int launches;      // of the graph fetched (only where graphs are on)
  int chunk;         // passed to chunk_run_begin (only where chunked)
};

// ---- the four computations before there was one, verbatim ----------------------------------------------------------------
// run_align (2D scan chain)
Old old_scan2d(int fixed_override, int fixed_iterations, int max_iterations, bool use_graph, int check_every, bool fused_begin) {
  const int fixed = fixed_override >= 0 ? fixed_override : fixed_iterations;
  const int K = fixed > 0 ? fixed : max_iterations;
  const bool chunked = use_graph && check_every > 0 && fixed == 0;
  const int first = fused_begin ? 1 : 0;
  const int chunk = check_every + (check_every & 1);
  return {fixed, K, first, chunked, chunked ? chunk : K + 1 - first, chunk};
}

// run_align_map (2D map-to-map chain)
Old old_map2d(int fixed_override, int fixed_iterations, int max_iterations, bool use_graph, int check_every) {
  const int fixed = fixed_override >= 0 ? fixed_override : fixed_iterations;
  const int K = fixed > 0 ? fixed : max_iterations;
  const bool chunked = use_graph && check_every > 0 && fixed == 0;
  const int launches = chunked ? check_every + (check_every & 1) : K + 1;
  return {fixed, K, 0, chunked, launches, launches};
}

// begin_align3 (3D scan chain): graphs always, chunks of 8
Old old_scan3d(int fixed_override, int fixed_iterations, int max_iterations, bool fused_begin) {
  const int fixed = fixed_override >= 0 ? fixed_override : fixed_iterations;
  const int first = fused_begin ? 1 : 0;
  const int K = fixed > 0 ? fixed : max_iterations;
  const int chunk = 8;
  return {fixed, K, first, !(fixed > 0), fixed > 0 ? K + 1 - first : chunk, chunk};
}

// align_map_pair(ndt3d_handle*, ...) (3D map-to-map chain)
Old old_map3d(int fixed_override, int fixed_iterations, int max_iterations) {
  const int fixed = fixed_override >= 0 ? fixed_override : fixed_iterations;
  const int K = fixed > 0 ? fixed : max_iterations;
  const int launches = fixed > 0 ? K + 1 : 8;
  return {fixed, K, 0, !(fixed > 0), launches, launches};
}

// the plain-launch loop's poll of run_align and run_align_map: after launch k, fetch the state and look at `done`
bool old_polls(int check_every, int fixed, int K, int k) {
  return check_every > 0 && fixed == 0 && k < K && (k % check_every) == check_every - 1;
}

void compare(const char* who, const ChainPlan& p, const Old& o, bool use_graph, const int* row) {
  bool same = p.fixed == o.fixed && p.K == o.K && p.first == o.first && p.chunked == o.chunked && p.graph == use_graph;
  if (use_graph) same = same && p.launches == o.launches;
  if (o.chunked) same = same && p.chunk == o.chunk;
  if (same) return;
  std::printf("%s: row (%d, %d, %d, %d, %d, %d): fixed %d K %d first %d chunked %d chunk %d launches %d, expected %d %d %d %d %d %d\n",
              who, row[0], row[1], row[2], row[3], row[4], row[5], p.fixed, p.K, p.first, (int)p.chunked, p.chunk, p.launches,
              o.fixed, o.K, o.first, (int)o.chunked, o.chunk, o.launches);
  ++failures;
}

}  // namespace

int main() {
  const int overrides[] = {-1, 0, 1, 5}, fixed_its[] = {0, 3, 30}, max_its[] = {1, 30}, checks[] = {0, 1, 7, 8};
  long rows = 0;
  for (int fo : overrides) for (int fi : fixed_its) for (int mi : max_its) for (int ug = 0; ug < 2; ++ug)
    for (int ce : checks) for (int fused = 0; fused < 2; ++fused) {
      const int row[6] = {fo, fi, mi, ug, ce, fused};
      const ChainPlan p = ndt::chain_plan(fo, fi, mi, ug != 0, ce, fused != 0);
      ++rows;
      compare("2D scan", p, old_scan2d(fo, fi, mi, ug != 0, ce, fused != 0), ug != 0, row);
      if (!fused) compare("2D map", p, old_map2d(fo, fi, mi, ug != 0, ce), ug != 0, row);
      if (ug && ce == 8) {                                  // what a 3D handle passes
        compare("3D scan", p, old_scan3d(fo, fi, mi, fused != 0), true, row);
        if (!fused) compare("3D map", p, old_map3d(fo, fi, mi), true, row);
      }
      // chunks are even, so that replays of one graph keep alternating the parity
      if (p.chunk & 1) { std::printf("row %ld: odd chunk %d\n", rows, p.chunk); ++failures; }
      // a chain that is not chunked runs launches 0 .. K, `first` of them in front of the graph
      if (!p.chunked && p.first + p.launches != p.K + 1) {
        std::printf("row %ld: first %d + launches %d != K + 1 = %d\n", rows, p.first, p.launches, p.K + 1);
        ++failures;
      }
      // a fixed chain (an evaluation among them) is the same whatever the chunk length: never chunked, never polled
      if (p.fixed > 0 && (p.chunked || p.poll != 0)) { std::printf("row %ld: a fixed chain is chunked or polled\n", rows); ++failures; }
      // the plain-launch loop polls where the old loops polled
      for (int k = p.first; !ug && k <= p.K; ++k) {
        const bool polls = p.poll > 0 && k < p.K && (k % p.poll) == p.poll - 1;
        if (polls != old_polls(ce, p.fixed, p.K, k)) { std::printf("row %ld: poll differs at launch %d\n", rows, k); ++failures; }
      }
      if (ug && p.poll != 0) { std::printf("row %ld: a graph chain polls\n", rows); ++failures; }
    }
  if (rows != 4 * 3 * 2 * 2 * 4 * 2) { std::printf("walked %ld rows\n", rows); ++failures; }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}

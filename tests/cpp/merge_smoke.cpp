// Submap merging through the C++ adapter: loads two saved maps (files written by the pytest driver) into
// ndt::NdtMatcherHip / ndt::NdtMatcherHip3, folds the second into the first at a pose (mergeMap), writes the result,
// takes it out again (unmergeMap) and writes that too.  The driver compares both files with the restatement's bytes.
//   merge_smoke <2|3> dst.map src.map merged.map back.map pose...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ndt_matcher_hip.hpp"

static std::vector<unsigned char> load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> v(n);
  if (std::fread(v.data(), 1, n, f) != (size_t)n) std::exit(2);
  std::fclose(f);
  return v;
}

static void store(const char* path, const std::vector<unsigned char>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), 1, v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
  std::fclose(f);
}

static double cell_size_of(const std::vector<unsigned char>& blob) {
  ndt_map_header h;
  if (blob.size() < sizeof h) std::exit(2);
  std::memcpy(&h, blob.data(), sizeof h);
  return h.cell_size;
}

template <class Matcher, class Params, class Pose>
static int run(Params pd, Params ps, const std::vector<unsigned char>& dst_blob, const std::vector<unsigned char>& src_blob,
               const Pose& pose, char** out) {
  pd.cell_size = cell_size_of(dst_blob);
  ps.cell_size = cell_size_of(src_blob);
  Matcher dst(pd), src(ps);
  dst.loadMap(dst_blob);
  src.loadMap(src_blob);
  const size_t outside = dst.mergeMap(src, pose);
  store(out[0], dst.saveMap());
  const size_t outside_back = dst.unmergeMap(src, pose);
  store(out[1], dst.saveMap());
  std::printf("outside %zu %zu\n", outside, outside_back);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: 2|3 dst.map src.map merged.map back.map pose...\n"); return 2; }
  const int dim = std::atoi(argv[1]);
  if ((dim != 2 && dim != 3) || argc != 6 + (dim == 2 ? 3 : 6)) { std::fprintf(stderr, "a 2D pose has 3 numbers, a 3D pose 6\n"); return 2; }
  const auto dst_blob = load(argv[2]), src_blob = load(argv[3]);
  double p[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < (dim == 2 ? 3 : 6); ++i) p[i] = std::strtod(argv[6 + i], nullptr);
  try {
    if (dim == 2)
      return run<ndt::NdtMatcherHip>(ndt::NdtMatcherHip::defaultParams(), ndt::NdtMatcherHip::defaultParams(), dst_blob, src_blob,
                                     ndt::Pose2{p[0], p[1], p[2]}, argv + 4);
    return run<ndt::NdtMatcherHip3>(ndt::NdtMatcherHip3::defaultParams(), ndt::NdtMatcherHip3::defaultParams(), dst_blob, src_blob,
                                    ndt::Pose3{p[0], p[1], p[2], p[3], p[4], p[5]}, argv + 4);
  } catch (const ndt::NdtError& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
}

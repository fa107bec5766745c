// The voxel-grid scan filter through the C++ adapter: loads a cloud (a file written by the pytest driver), makes one
// call of NdtMatcherHip::voxelFilterDev (or the 3D twin) on a matcher without a target and compares the count and the
// first and last output point, as float32 bit patterns, with what the driver passes in.
//   voxel_filter_smoke <2|3> cloud.f32 n leaf min_points n_out first[dim] last[dim]      (points as hex words)
// Exit 0: all equal; 1: something differs (printed); 3: the library reported an error (printed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ndt_matcher_hip.hpp"

// Only the C API of the HIP runtime is needed for the device buffers (no device code: plain g++).
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device, 2 = device to host
}

static std::vector<float> load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> v(n / sizeof(float));
  if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}
static float* device(size_t n, const float* from = nullptr) {
  void* d = nullptr;
  if (hipMalloc(&d, n * sizeof(float)) != 0 || (from && hipMemcpy(d, from, n * sizeof(float), 1) != 0)) {
    std::fprintf(stderr, "device buffer failed\n");
    std::exit(2);
  }
  return static_cast<float*>(d);
}
static uint32_t word_at(const float* d, size_t i) {
  uint32_t w = 0;
  if (hipMemcpy(&w, d + i, sizeof w, 2) != 0) { std::fprintf(stderr, "download failed\n"); std::exit(2); }
  return w;
}

int main(int argc, char** argv) {
  const int dim = argc > 1 ? std::atoi(argv[1]) : 0;
  if ((dim != 2 && dim != 3) || argc != 7 + 2 * dim) { std::fprintf(stderr, "usage: 2|3 cloud n leaf min_points n_out first... last...\n"); return 2; }
  const auto cloud = load(argv[2]);
  const size_t n = std::strtoull(argv[3], nullptr, 10);
  const double leaf = std::strtod(argv[4], nullptr);
  const uint32_t min_points = (uint32_t)std::strtoul(argv[5], nullptr, 10);
  const unsigned long long want_out = std::strtoull(argv[6], nullptr, 10);
  if (cloud.size() != n * (size_t)dim) { std::fprintf(stderr, "the cloud file holds %zu floats\n", cloud.size()); return 2; }
  try {
    const float* s[3] = {nullptr, nullptr, nullptr};
    float* o[3] = {nullptr, nullptr, nullptr};
    auto buffers = [&]() {                   // behind the matcher's constructor: without a device that one reports it
      for (int a = 0; a < dim; ++a) { s[a] = device(n, cloud.data() + a * n); o[a] = device(n); }
    };
    ndt_voxel_filter_info info;
    if (dim == 2) {
      ndt::NdtMatcherHip m(ndt::NdtMatcherHip::defaultParams());
      buffers();
      info = m.voxelFilterDev(s[0], s[1], n, leaf, o[0], o[1], n, min_points);
    } else {
      ndt::NdtMatcherHip3 m(ndt::NdtMatcherHip3::defaultParams());
      buffers();
      info = m.voxelFilterDev(s[0], s[1], s[2], n, leaf, o[0], o[1], o[2], n, min_points);
    }
    std::printf("info %llu %llu %llu\n", (unsigned long long)info.n_invalid, (unsigned long long)info.n_voxels,
                (unsigned long long)info.n_out);
    int bad = info.n_out != want_out || info.n_out == 0;
    for (int a = 0; a < dim && !bad; ++a) {
      const uint32_t first = word_at(o[a], 0), last = word_at(o[a], (size_t)info.n_out - 1);
      const uint32_t want_first = (uint32_t)std::strtoul(argv[7 + a], nullptr, 16);
      const uint32_t want_last = (uint32_t)std::strtoul(argv[7 + dim + a], nullptr, 16);
      std::printf("axis %d first %08x (%08x) last %08x (%08x)\n", a, first, want_first, last, want_last);
      bad |= first != want_first || last != want_last;
    }
    return bad;
  } catch (const ndt::NdtError& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
}

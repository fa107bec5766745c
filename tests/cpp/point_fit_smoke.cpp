// Per-point fit and selection through the C++ adapter: loads a saved map and a scan (files written by the pytest
// driver), runs NdtMatcherHip::fitPointsDev / selectPointsDev (or the 3D twins) and the C calls on a second handle of
// the same map, prints both summaries and writes the wrapper's classes and selected indices for the driver to compare.
//   point_fit_smoke <2|3> map.blob scan.f32 n max_m keep classes.u8 index.u32 pose...
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

template <class T>
static std::vector<T> load(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}
template <class T>
static void store(const char* path, const std::vector<T>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
  std::fclose(f);
}
template <class T>
static T* device(size_t n, const T* from = nullptr) {
  void* d = nullptr;
  if (hipMalloc(&d, n * sizeof(T)) != 0 || (from && hipMemcpy(d, from, n * sizeof(T), 1) != 0)) { std::fprintf(stderr, "device buffer failed\n"); std::exit(2); }
  return static_cast<T*>(d);
}
template <class T>
static std::vector<T> host(const T* d, size_t n) {
  std::vector<T> v(n);
  if (n && hipMemcpy(v.data(), d, n * sizeof(T), 2) != 0) { std::fprintf(stderr, "download failed\n"); std::exit(2); }
  return v;
}
static void print(const char* who, const ndt_point_fit& f) {
  std::printf("%s %llu %llu %llu %llu %llu\n", who, (unsigned long long)f.n_invalid, (unsigned long long)f.n_miss,
              (unsigned long long)f.n_misfit, (unsigned long long)f.n_fit, (unsigned long long)f.n_selected);
}
static double cell_size_of(const std::vector<unsigned char>& blob) {
  ndt_map_header h;
  if (blob.size() < sizeof h) std::exit(2);
  std::memcpy(&h, blob.data(), sizeof h);
  return h.cell_size;
}

int main(int argc, char** argv) {
  if (argc < 9) { std::fprintf(stderr, "usage: 2|3 map scan n max_m keep classes index pose...\n"); return 2; }
  const int dim = std::atoi(argv[1]);
  if ((dim != 2 && dim != 3) || argc != 9 + (dim == 2 ? 3 : 6)) { std::fprintf(stderr, "a 2D pose has 3 numbers, a 3D pose 6\n"); return 2; }
  const auto blob = load<unsigned char>(argv[2]);
  const auto scan = load<float>(argv[3]);
  const size_t n = std::strtoull(argv[4], nullptr, 10);
  const float max_m = std::strtof(argv[5], nullptr);
  const uint32_t keep = (uint32_t)std::strtoul(argv[6], nullptr, 10);
  if (scan.size() != n * (size_t)dim) { std::fprintf(stderr, "the scan file holds %zu floats\n", scan.size()); return 2; }
  double p[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < (dim == 2 ? 3 : 6); ++i) p[i] = std::strtod(argv[9 + i], nullptr);
  try {
    const float* s[3] = {nullptr, nullptr, nullptr};
    float* o[3] = {nullptr, nullptr, nullptr};
    float* d_m = nullptr;
    uint8_t* d_class = nullptr;
    uint32_t* d_index = nullptr;
    auto buffers = [&]() {                   // behind the matcher's constructor: without a device that one reports it
      for (int a = 0; a < dim; ++a) { s[a] = device(n, scan.data() + a * n); o[a] = device<float>(n); }
      d_m = device<float>(n);
      d_class = device<uint8_t>(n);
      d_index = device<uint32_t>(n);
    };
    ndt_point_fit fw, sw, fc, sc;
    if (dim == 2) {
      auto prm = ndt::NdtMatcherHip::defaultParams();
      prm.cell_size = cell_size_of(blob);
      ndt::NdtMatcherHip m(prm);
      buffers();
      m.loadMap(blob);
      const ndt::Pose2 at{p[0], p[1], p[2]};
      fw = m.fitPointsDev(s[0], s[1], n, at, max_m, d_m, d_class);
      sw = m.selectPointsDev(s[0], s[1], n, at, max_m, keep, o[0], o[1], d_index);
      ndt2d_handle* h = nullptr;
      if (ndt2d_create(&prm, 0, &h) != NDT_OK || ndt2d_load_map(h, blob.data(), blob.size()) != NDT_OK) return 4;
      if (ndt2d_fit_points(h, scan.data(), scan.data() + n, n, p, max_m, nullptr, nullptr, &fc) != NDT_OK) return 4;
      if (ndt2d_select_points_dev(h, s[0], s[1], n, p, max_m, keep, o[0], o[1], nullptr, &sc) != NDT_OK) return 4;
      ndt2d_destroy(h);
    } else {
      auto prm = ndt::NdtMatcherHip3::defaultParams();
      prm.cell_size = cell_size_of(blob);
      ndt::NdtMatcherHip3 m(prm);
      buffers();
      m.loadMap(blob);
      const ndt::Pose3 at{p[0], p[1], p[2], p[3], p[4], p[5]};
      fw = m.fitPointsDev(s[0], s[1], s[2], n, at, max_m, d_m, d_class);
      sw = m.selectPointsDev(s[0], s[1], s[2], n, at, max_m, keep, o[0], o[1], o[2], d_index);
      ndt3d_handle* h = nullptr;
      if (ndt3d_create(&prm, 0, &h) != NDT_OK || ndt3d_load_map(h, blob.data(), blob.size()) != NDT_OK) return 4;
      if (ndt3d_fit_points(h, scan.data(), scan.data() + n, scan.data() + 2 * n, n, p, max_m, nullptr, nullptr, &fc) != NDT_OK) return 4;
      if (ndt3d_select_points_dev(h, s[0], s[1], s[2], n, p, max_m, keep, o[0], o[1], o[2], nullptr, &sc) != NDT_OK) return 4;
      ndt3d_destroy(h);
    }
    print("wrapper_fit", fw);
    print("wrapper_select", sw);
    print("c_fit", fc);
    print("c_select", sc);
    store(argv[7], host(d_class, n));
    store(argv[8], host(d_index, (size_t)sw.n_selected));
    return 0;
  } catch (const ndt::NdtError& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
}

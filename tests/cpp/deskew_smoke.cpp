// Sweep de-skewing through the C++ adapter (include/ndt_matcher_hip.hpp), driven by tests/test_cpp_deskew.py.
//   deskew_smoke host p0 .. p5 c0 .. c5
//       sweepMotion of the two 3D poses, and of their (x, y, yaw) as 2D poses; needs no device.  Prints every double in
//       hexadecimal.
//   deskew_smoke dev ranges2.f32 frac2.f32 n ranges3.f32 frac3.f32 elevations.f64 n_elev n_azim out.f32
//       the de-skewing conversions of an n-beam scan and an n_elev x n_azim image (beam i / column j at bearing
//       -pi + (i + 1/2) 2 pi / n, fraction -0.25 + i 1.5 / n, ref_frac 0.5, ranges in [0.05, 100]), then deskewPointsDev
//       of what they returned with the fractions of the files and ref_frac 1.  Writes x y | x' y' | x y z | x' y' z'.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ndt_matcher_hip.hpp"

// Only the C API of the HIP runtime is needed for the device buffers (no device code: plain g++).
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device, 2 = device to host
int hipDeviceSynchronize(void);
}

static const ndt::Pose2 kMotion2 = [] { ndt::Pose2 p; p.x = 0.25; p.y = 0.05; p.theta = 0.08; return p; }();
static const ndt::Pose3 kMotion3 = [] { ndt::Pose3 p; p.x = 0.5; p.y = 0.1; p.z = 0.02; p.roll = 0.01; p.pitch = -0.01; p.yaw = 0.12; return p; }();

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
static float* device(size_t n, const float* from = nullptr) {
  void* d = nullptr;
  if (hipMalloc(&d, n * sizeof(float)) != 0 || (from && hipMemcpy(d, from, n * sizeof(float), 1) != 0)) {
    std::printf("error no device buffer: no CPU fallback\n");
    std::exit(3);
  }
  return static_cast<float*>(d);
}

static int host(char** v) {
  double a[12];
  for (int i = 0; i < 12; ++i) a[i] = std::strtod(v[i], nullptr);
  ndt::Pose3 p, c;
  p.x = a[0]; p.y = a[1]; p.z = a[2]; p.roll = a[3]; p.pitch = a[4]; p.yaw = a[5];
  c.x = a[6]; c.y = a[7]; c.z = a[8]; c.roll = a[9]; c.pitch = a[10]; c.yaw = a[11];
  const ndt::Pose3 d3 = ndt::NdtMatcherHip3::sweepMotion(p, c);
  std::printf("sweep3 %a %a %a %a %a %a\n", d3.x, d3.y, d3.z, d3.roll, d3.pitch, d3.yaw);
  ndt::Pose2 p2, c2;
  p2.x = a[0]; p2.y = a[1]; p2.theta = a[5];
  c2.x = a[6]; c2.y = a[7]; c2.theta = a[11];
  const ndt::Pose2 d2 = ndt::NdtMatcherHip::sweepMotion(p2, c2);
  std::printf("sweep2 %a %a %a\n", d2.x, d2.y, d2.theta);
  try {
    p.x = std::nan("");
    ndt::NdtMatcherHip3::sweepMotion(p, c);
    return 1;
  } catch (const ndt::NdtError& e) {
    std::printf("refused %d\n", e.code());
  }
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 14 && std::string(argv[1]) == "host") return host(argv + 2);
    if (argc != 11 || std::string(argv[1]) != "dev") { std::fprintf(stderr, "usage: see the head of deskew_smoke.cpp\n"); return 2; }
    const auto r2 = load<float>(argv[2]), f2 = load<float>(argv[3]);
    const size_t n = std::strtoull(argv[4], nullptr, 10);
    const auto r3 = load<float>(argv[5]), f3 = load<float>(argv[6]);
    const auto el = load<double>(argv[7]);
    const int ne = std::atoi(argv[8]), na = std::atoi(argv[9]);
    const size_t n3 = (size_t)ne * na;
    if (r2.size() != n || f2.size() != n || r3.size() != n3 || f3.size() != n3 || el.size() != (size_t)ne) return 2;
    const double pi = 3.141592653589793;
    std::vector<float> out(4 * n + 6 * n3);
    {
      const float* d_r = device(n, r2.data());
      const float* d_f = device(n, f2.data());
      float* d[4];
      for (float*& q : d) q = device(n);
      const double inc = 2.0 * pi / (double)n;
      ndt::NdtMatcherHip::polarToPointsDev(d_r, n, -pi + 0.5 * inc, inc, 0.05, 100.0, d[2], d[3], nullptr);     // overwritten below
      ndt::NdtMatcherHip::polarToPointsDev(d_r, n, -pi + 0.5 * inc, inc, 0.05, 100.0, kMotion2, -0.25, 1.5 / (double)n, 0.5,
                                           d[0], d[1], nullptr);
      ndt::NdtMatcherHip::deskewPointsDev(d[0], d[1], d_f, n, kMotion2, 1.0, d[2], d[3], nullptr);
      if (hipDeviceSynchronize() != 0) return 2;
      for (int k = 0; k < 4; ++k)
        if (hipMemcpy(out.data() + k * n, d[k], n * sizeof(float), 2) != 0) return 2;
    }
    {
      const float* d_r = device(n3, r3.data());
      const float* d_f = device(n3, f3.data());
      float* d[6];
      for (float*& q : d) q = device(n3);
      const double inc = 2.0 * pi / (double)na;
      ndt::NdtMatcherHip3::rangeImageToPointsDev(d_r, ne, na, el.data(), -pi + 0.5 * inc, inc, 0.05, 100.0, d[3], d[4], d[5],
                                                 nullptr);
      ndt::NdtMatcherHip3::rangeImageToPointsDev(d_r, ne, na, el.data(), -pi + 0.5 * inc, inc, 0.05, 100.0, kMotion3, -0.25,
                                                 1.5 / (double)na, 0.5, d[0], d[1], d[2], nullptr);
      ndt::NdtMatcherHip3::deskewPointsDev(d[0], d[1], d[2], d_f, n3, kMotion3, 1.0, d[3], d[4], d[5], nullptr);
      if (hipDeviceSynchronize() != 0) return 2;
      for (int k = 0; k < 6; ++k)
        if (hipMemcpy(out.data() + 4 * n + k * n3, d[k], n3 * sizeof(float), 2) != 0) return 2;
    }
    FILE* f = std::fopen(argv[10], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { std::perror(argv[10]); return 2; }
    std::fclose(f);
    std::printf("ok %zu %zu\n", n, n3);
    return 0;
  } catch (const ndt::NdtError& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
}

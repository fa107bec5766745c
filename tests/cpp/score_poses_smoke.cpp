// Scoring a list of poses through the C++ adapter: loads a saved map, a scan and a pose list (files written by the pytest
// driver), runs NdtMatcherHip::scorePosesDev / bestPosesDev / bestPosesAlignDev (or the 3D twins), writes the scores and
// prints the hits and the refined results with every double in hexadecimal, for the driver to compare bit for bit.
//   score_poses_smoke <2|3> map.blob scan.f32 n poses.f64 m k min_sep_trans min_sep_rot scores.f32
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
static T* device(size_t n, const T* from = nullptr) {
  void* d = nullptr;
  if (hipMalloc(&d, n * sizeof(T)) != 0 || (from && hipMemcpy(d, from, n * sizeof(T), 1) != 0)) { std::fprintf(stderr, "device buffer failed\n"); std::exit(2); }
  return static_cast<T*>(d);
}
static double cell_size_of(const std::vector<unsigned char>& blob) {
  ndt_map_header h;
  if (blob.size() < sizeof h) std::exit(2);
  std::memcpy(&h, blob.data(), sizeof h);
  return h.cell_size;
}
static void row(const char* who, int32_t index, float score, const double* pose, int np) {
  std::printf("%s %d %a", who, (int)index, (double)score);
  for (int a = 0; a < np; ++a) std::printf(" %a", pose[a]);
  std::printf("\n");
}
static void result(const double* pose, int np, double score, int iterations, int n_hit, int status) {
  std::printf("result %d %d %d %a", iterations, n_hit, status, score);
  for (int a = 0; a < np; ++a) std::printf(" %a", pose[a]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 11) { std::fprintf(stderr, "usage: 2|3 map scan n poses m k min_sep_trans min_sep_rot scores\n"); return 2; }
  const int dim = std::atoi(argv[1]);
  if (dim != 2 && dim != 3) return 2;
  const int np = dim == 2 ? 3 : 6;
  const auto blob = load<unsigned char>(argv[2]);
  const auto scan = load<float>(argv[3]);
  const size_t n = std::strtoull(argv[4], nullptr, 10);
  const auto poses = load<double>(argv[5]);
  const size_t m = std::strtoull(argv[6], nullptr, 10);
  const int k = std::atoi(argv[7]);
  const double sep_t = std::strtod(argv[8], nullptr), sep_r = std::strtod(argv[9], nullptr);
  if (scan.size() != n * (size_t)dim || poses.size() != m * (size_t)np) { std::fprintf(stderr, "the files do not hold n points and m poses\n"); return 2; }
  try {
    const float* s[3] = {nullptr, nullptr, nullptr};
    const double* d_poses = nullptr;
    float* d_scores = nullptr;
    auto buffers = [&]() {                   // behind the matcher's constructor: without a device that one reports it
      for (int a = 0; a < dim; ++a) s[a] = device(n, scan.data() + a * n);
      d_poses = device(poses.size(), poses.data());
      d_scores = device<float>(m);
    };
    if (dim == 2) {
      auto prm = ndt::NdtMatcherHip::defaultParams();
      prm.cell_size = cell_size_of(blob);
      ndt::NdtMatcherHip mt(prm);
      buffers();
      mt.loadMap(blob);
      mt.scorePosesDev(s[0], s[1], n, d_poses, m, d_scores, nullptr);
      for (const auto& h : mt.bestPosesDev(s[0], s[1], n, d_poses, m, k, sep_t, sep_r, nullptr)) {
        const double p[3] = {h.pose.x, h.pose.y, h.pose.theta};
        row("hit", h.index, h.score, p, np);
      }
      for (const auto& q : mt.bestPosesAlignDev(s[0], s[1], n, d_poses, m, k, sep_t, sep_r, nullptr, /*complete=*/true)) {
        const double p[3] = {q.hit.pose.x, q.hit.pose.y, q.hit.pose.theta};
        row("match", q.hit.index, q.hit.score, p, np);
        const double r[3] = {q.result.pose.x, q.result.pose.y, q.result.pose.theta};
        result(r, np, q.result.score, q.result.iterations, q.result.n_hit, q.result.status);
      }
    } else {
      auto prm = ndt::NdtMatcherHip3::defaultParams();
      prm.cell_size = cell_size_of(blob);
      ndt::NdtMatcherHip3 mt(prm);
      buffers();
      mt.loadMap(blob);
      mt.scorePosesDev(s[0], s[1], s[2], n, d_poses, m, d_scores, nullptr);
      for (const auto& h : mt.bestPosesDev(s[0], s[1], s[2], n, d_poses, m, k, sep_t, sep_r, nullptr)) {
        const double p[6] = {h.pose.x, h.pose.y, h.pose.z, h.pose.roll, h.pose.pitch, h.pose.yaw};
        row("hit", h.index, h.score, p, np);
      }
      for (const auto& q : mt.bestPosesAlignDev(s[0], s[1], s[2], n, d_poses, m, k, sep_t, sep_r, nullptr, /*complete=*/true)) {
        const double p[6] = {q.hit.pose.x, q.hit.pose.y, q.hit.pose.z, q.hit.pose.roll, q.hit.pose.pitch, q.hit.pose.yaw};
        row("match", q.hit.index, q.hit.score, p, np);
        const double r[6] = {q.result.pose.x, q.result.pose.y, q.result.pose.z, q.result.pose.roll, q.result.pose.pitch, q.result.pose.yaw};
        result(r, np, q.result.score, q.result.iterations, q.result.n_hit, q.result.status);
      }
    }
    std::vector<float> sc(m);
    if (hipMemcpy(sc.data(), d_scores, m * sizeof(float), 2) != 0) { std::fprintf(stderr, "download failed\n"); return 2; }
    FILE* f = std::fopen(argv[10], "wb");
    if (!f || std::fwrite(sc.data(), sizeof(float), m, f) != m) { std::perror(argv[10]); return 2; }
    std::fclose(f);
    return 0;
  } catch (const ndt::NdtError& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
}

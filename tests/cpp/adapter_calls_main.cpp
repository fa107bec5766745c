// The call record of include/ndt_matcher_hip.hpp (tests/test_adapter_calls.py): every public member and free function of
// the adapter once per dimension, linked against the recording stand-in tests/cpp/adapter_stub.cpp instead of the
// library.  A section "== Class.method [mode]" holds the C calls the stand-in saw (lines "  C ...") and what the adapter
// returned, every field at full precision; every section runs with the stand-in answering NDT_OK [ok], failing every call
// [fail], and failing every call but ndt*_wait_stream [fail-after-wait].  Members of a class template are only
// type-checked where they are instantiated: a method added to the adapter gets its section here.
//
// The sizes are the smallest that tell a mistake: 5 points per scan, pose lists of 2, k = 3 where the stand-in reports 2
// hits, batch pairs of 3 and 5 points, 2 shards.  This file compiles unchanged against any version of the header that
// keeps its interface; tests/golden/adapter_calls.txt is its output with the header as it was before the 2D and the 3D
// classes were merged.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "ndt_matcher_hip.hpp"

extern "C" void stub_arena(const void* base, size_t bytes);
extern "C" void stub_mode(int mode);
extern "C" void stub_section(const char* title);

namespace {
using namespace ndt;

constexpr size_t N = 5;         // points per scan
constexpr size_t M = 2;         // poses per list

// everything the adapter only passes through lives here, so that the record holds offsets, not addresses
struct Arena {
  float x[N], y[N], z[N], x2[N], y2[N], z2[N], ox[N], oy[N], oz[N], frac[N], ranges[N], m[N], scores[N];
  double poses[6 * M], elevations[2], init[12];
  uint64_t toff[3], soff[3];
  uint32_t n_hit[N], index[N], count[N];
  uint8_t cls[N];
  ndt2d_search_window w2;
  ndt3d_search_window w3;
  ndt3d_result results[2];
  char producer, other_stream;
} A;

void nums(const char* label, const double* v, size_t n) {
  printf("    %s", label);
  for (size_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}
void show(const Pose2& p) { printf("    pose x=%.17g y=%.17g theta=%.17g\n", p.x, p.y, p.theta); }
void show(const Pose3& p) {
  printf("    pose x=%.17g y=%.17g z=%.17g roll=%.17g pitch=%.17g yaw=%.17g\n", p.x, p.y, p.z, p.roll, p.pitch, p.yaw);
}
template <class R>
void show_result(const R& r) {
  show(r.pose);
  nums("information", r.information.data(), r.information.size());
  nums("covariance", r.covariance.data(), r.covariance.size());
  printf("    score=%.17g iterations=%d n_hit=%d status=%d converged=%d\n", r.score, r.iterations, r.n_hit, r.status,
         (int)r.converged());
}
void show(const MatchResult& r) { show_result(r); }
void show(const MatchResult3& r) { show_result(r); }
template <class Hit>
void show_hit(const Hit& h) {
  show(h.pose);
  printf("    hit score=%.9g index=%d\n", (double)h.score, (int)h.index);
}
void show(const NdtMatcherHip::SearchHit& h) { show_hit(h); }
void show(const NdtMatcherHip3::SearchHit& h) { show_hit(h); }
void show(const NdtMatcherHip::SearchMatch& s) { show_hit(s.hit); show_result(s.result); }
void show(const NdtMatcherHip3::SearchMatch& s) { show_hit(s.hit); show_result(s.result); }
template <class T>
void show(const std::vector<T>& v) {
  printf("    size=%zu\n", v.size());
  for (size_t i = 0; i < v.size(); ++i) { printf("   [%zu]\n", i); show(v[i]); }
}
template <class E>
void show_eval(const E& e, size_t n) {
  nums("H", e.H, n * n);
  nums("g", e.g, n);
  printf("    score=%.17g n_hit=%d\n", e.score, e.n_hit);
}
void show(const ndt2d_eval& e) { show_eval(e, 3); }
void show(const ndt3d_eval& e) { show_eval(e, 6); }
void show(const ndt2d_grid_info& g) {
  printf("    grid ox=%.9g oy=%.9g inv_cell=%.9g cell=%.9g width=%d height=%d n_valid=%d n_points=%d\n", (double)g.ox, (double)g.oy,
         (double)g.inv_cell, (double)g.cell, g.width, g.height, g.n_valid, g.n_points);
}
void show(const ndt3d_grid_info& g) {
  printf("    grid ox=%.9g oy=%.9g oz=%.9g inv_cell=%.9g width=%d height=%d depth=%d n_valid=%d\n", (double)g.ox, (double)g.oy,
         (double)g.oz, (double)g.inv_cell, g.width, g.height, g.depth, g.n_valid);
}
void show(const ndt_point_fit& f) {
  printf("    fit n_invalid=%lu n_miss=%lu n_misfit=%lu n_fit=%lu n_selected=%lu\n", (unsigned long)f.n_invalid,
         (unsigned long)f.n_miss, (unsigned long)f.n_misfit, (unsigned long)f.n_fit, (unsigned long)f.n_selected);
}
void show(const ndt_voxel_filter_info& v) {
  printf("    info n_invalid=%lu n_voxels=%lu n_out=%lu\n", (unsigned long)v.n_invalid, (unsigned long)v.n_voxels,
         (unsigned long)v.n_out);
}
void show(size_t v) { printf("    value=%zu\n", v); }
void show(const ndt2d_params& p) {
  printf("    params %.17g %d %d %.17g %.17g %.17g %d %d %.17g %.17g %.17g %.17g %d %d %d %.17g\n", p.cell_size, p.min_points,
         p.hessian_mode, p.eig_ratio, p.d1, p.d2, p.max_iterations, p.fixed_iterations, p.eps_trans, p.eps_rot, p.step_max_trans,
         p.step_max_rot, p.min_hits, p.overlap_grids, p.line_search, p.step_scale);
}
void show_ptr(const void* p) { printf("    pointer=%#zx\n", reinterpret_cast<size_t>(p)); }

// one section per mode; a throw ends the section with the error's code and its text, which begins with `where`
template <class F>
void section(const std::string& name, F&& body, int modes = 3) {
  static const char* const tag[3] = {"ok", "fail", "fail-after-wait"};
  for (int mode = 0; mode < modes; ++mode) {
    stub_mode(mode);
    stub_section((name + " [" + tag[mode] + "]").c_str());
    try {
      body();
    } catch (const NdtError& e) {
      printf("  throws code=%d what=%s\n", (int)e.code(), e.what());
    }
  }
  stub_mode(0);
}

// ---- what differs between the dimensions, for the sections that are the same text in both ------------------------------
struct D2 {
  using Matcher = NdtMatcherHip;
  using Pose = Pose2;
  using Window = ndt2d_search_window;
  static constexpr const char* name = "NdtMatcherHip";
  static Pose pose(double b) { Pose p; p.x = b + 0.1; p.y = b + 0.2; p.theta = b + 0.3; return p; }
  static Window& window() { return A.w2; }
};
struct D3 {
  using Matcher = NdtMatcherHip3;
  using Pose = Pose3;
  using Window = ndt3d_search_window;
  static constexpr const char* name = "NdtMatcherHip3";
  static Pose pose(double b) {
    Pose p;
    p.x = b + 0.1; p.y = b + 0.2; p.z = b + 0.3; p.roll = b + 0.4; p.pitch = b + 0.5; p.yaw = b + 0.6;
    return p;
  }
  static Window& window() { return A.w3; }
};

// the members that take no coordinate arrays: the same calls on either matcher
template <class D>
void shared_sections(typename D::Matcher& a, typename D::Matcher& b) {
  using Mt = typename D::Matcher;
  using Pose = typename D::Pose;
  const std::string c = std::string(D::name) + ".";
  void* const producer = &A.producer;
  section(c + "defaultParams", [&] { show(Mt::defaultParams()); });
  section(c + "gridInfo", [&] { const Mt& ca = a; show(ca.gridInfo()); });
  section(c + "saveMap", [&] {
    const Mt& ca = a;
    const std::vector<unsigned char> buf = ca.saveMap();
    printf("    bytes");
    for (unsigned char v : buf) printf(" %d", (int)v);
    printf("\n");
  });
  section(c + "loadMap", [&] { a.loadMap(std::vector<unsigned char>{1, 2, 3}); });
  section(c + "coarsenInto", [&] { a.coarsenInto(b); });
  section(c + "mergeMap", [&] { show(a.mergeMap(b, D::pose(1))); });
  section(c + "unmergeMap", [&] { show(a.unmergeMap(b, D::pose(2))); });
  section(c + "alignMap", [&] {
    show(a.alignMap(b));
    show(a.alignMap(b, D::pose(3)));
    show(a.alignMap(a, D::pose(4)));
  });
  section(c + "alignMapMulti", [&] {
    show(a.alignMapMulti(std::vector<Mt*>{&b, &a}, std::vector<Pose>{D::pose(1), D::pose(2)}));
    show(a.alignMapMulti({&b, nullptr}, {D::pose(3), D::pose(4)}));
    show(a.alignMapMulti({}, {}));
    show(a.alignMapMulti({&b, &a}, {D::pose(5)}));
  });
  section(c + "evaluateMap", [&] { show(a.evaluateMap(b, D::pose(5))); });
  section(c + "searchMap", [&] { for (int k : {3, 0, -1}) show(a.searchMap(b, D::window(), k)); });
  section(c + "searchMapScores", [&] { a.searchMapScores(b, D::window(), A.scores); });
  section(c + "searchAlignMap", [&] { for (int k : {3, 0, -1}) show(a.searchAlignMap(b, D::window(), k)); });
  section(c + "scoreMapPosesDev", [&] {
    a.scoreMapPosesDev(b, A.poses, M, A.scores, A.n_hit, producer);
    a.scoreMapPosesDev(b, A.poses, M, A.scores, nullptr, nullptr, true);
  });
  section(c + "bestMapPosesDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestMapPosesDev(b, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestMapPosesDev(b, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "bestMapPosesAlignDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestMapPosesAlignDev(b, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestMapPosesAlignDev(b, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "sweepMotion", [&] { show(Mt::sweepMotion(D::pose(1), D::pose(2))); });
  section(c + "stream", [&] { show_ptr(a.stream()); });
  section(c + "raw", [&] { show_ptr(a.raw()); show_ptr(b.raw()); });
}

// ---- free functions ---------------------------------------------------------------------------------------------------
void free_function_sections() {
  section("invert3", [] {
    const double H[9] = {4, 1, 0.5, 1, 3, 0.25, 0.5, 0.25, 2}, Z[9] = {0};
    double C[9];
    printf("    ok=%d\n", (int)invert3(H, C));
    nums("C", C, 9);
    printf("    ok=%d\n", (int)invert3(Z, C));
    nums("C", C, 9);
  }, 1);
  section("invert6", [] {
    double H[36], Z[36] = {0}, C[36];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) H[6 * i + j] = (i == j ? 10.0 + i : 0.0) + 0.125 * (i < j ? 6 * i + j : 6 * j + i);
    printf("    ok=%d\n", (int)invert6(H, C));
    nums("C", C, 36);
    printf("    ok=%d\n", (int)invert6(Z, C));
    nums("C", C, 36);
  }, 1);
  section("to_match_result", [] {
    ndt2d_result r{};
    for (int i = 0; i < 3; ++i) { r.pose[i] = 1.5 + i; r.g[i] = 9.0; }
    for (int i = 0; i < 9; ++i) r.H[i] = 20.0 + i;
    r.score = 12.5; r.iterations = 7; r.n_hit = 33; r.status = NDT_NOT_CONVERGED;
    show(to_match_result(r));
    show(to_match_result(r, NDT_HESSIAN_NEWTON));
  });
  section("covarianceInLocalFrame", [] {
    MatchResult m;
    m.pose = D2::pose(0.25);
    for (int i = 0; i < 9; ++i) m.covariance[i] = 1.0 + 0.5 * i;
    nums("C_local", covarianceInLocalFrame(m).data(), 9);
  }, 1);
  section("rotationOf", [] { nums("R", rotationOf(D3::pose(0.25)).data(), 9); }, 1);
  section("covarianceInLocalFrame3", [] {
    std::array<double, 36> cov{};
    for (int i = 0; i < 36; ++i) cov[i] = 1.0 + 0.5 * i;
    nums("C_local", covarianceInLocalFrame3(D3::pose(0.25), cov).data(), 36);
  }, 1);
}

// ---- NdtMatcherHip: the members that take (x, y) -------------------------------------------------------------------------
void matcher2_sections(NdtMatcherHip& a) {
  const std::string c = "NdtMatcherHip.";
  void* const producer = &A.producer;
  const std::vector<float> vx(A.x, A.x + N), vy(A.y, A.y + N);
  section(c + "setTarget", [&] { a.setTarget(A.x, A.y, N); a.setTarget(vx, vy); });
  section(c + "reserveTarget", [&] { a.reserveTarget(-1.5, -2.5, 3.5, 4.5); });
  section(c + "addTargetPoints", [&] { show(a.addTargetPoints(A.x, A.y, N)); });
  section(c + "addTargetPointsDev", [&] {
    const Pose2 p = D2::pose(1);
    show(a.addTargetPointsDev(A.x, A.y, N));
    show(a.addTargetPointsDev(A.x, A.y, N, &p, producer));
  });
  section(c + "removeTargetPoints", [&] { show(a.removeTargetPoints(A.x, A.y, N)); });
  section(c + "removeTargetPointsDev", [&] {
    const Pose2 p = D2::pose(2);
    show(a.removeTargetPointsDev(A.x, A.y, N));
    show(a.removeTargetPointsDev(A.x, A.y, N, &p, producer));
  });
  section(c + "align", [&] {
    show(a.align(A.x, A.y, N));
    show(a.align(A.x, A.y, N, D2::pose(1)));
    show(a.align(vx, vy));
    show(a.align(vx, vy, D2::pose(2)));
  });
  section(c + "alignDev", [&] {
    show(a.alignDev(A.x, A.y, N, D2::pose(1), producer));
    show(a.alignDev(A.x, A.y, N, D2::pose(2), nullptr, true));
  });
  section(c + "alignMultiStartDev", [&] {
    show(a.alignMultiStartDev(A.x, A.y, N, {D2::pose(1), D2::pose(2)}, producer));
    show(a.alignMultiStartDev(A.x, A.y, N, {D2::pose(3)}, nullptr, true));
  });
  section(c + "alignMultiScanDev", [&] {
    const std::vector<NdtMatcherHip::DeviceScan> scans = {NdtMatcherHip::DeviceScan{A.x, A.y, N}, NdtMatcherHip::DeviceScan{A.x2, A.y2, 3}};
    show(a.alignMultiScanDev(scans, {D2::pose(1), D2::pose(2)}, producer));
    show(a.alignMultiScanDev(scans, {D2::pose(3), D2::pose(4)}, nullptr, true));
  });
  section(c + "alignMultiScanDev/mismatch", [&] {
    a.alignMultiScanDev({NdtMatcherHip::DeviceScan{A.x, A.y, N}}, {D2::pose(1), D2::pose(2)}, producer);
  });
  section(c + "alignMultiScanDev/empty", [&] { a.alignMultiScanDev({}, {}, producer); });
  section(c + "searchDev", [&] {
    for (int k : {3, 0, -1}) show(a.searchDev(A.x, A.y, N, A.w2, k, producer));
    show(a.searchDev(A.x, A.y, N, A.w2, 3, nullptr, true));
  });
  section(c + "searchAlignDev", [&] {
    for (int k : {3, 0, -1}) show(a.searchAlignDev(A.x, A.y, N, A.w2, k, producer));
    show(a.searchAlignDev(A.x, A.y, N, A.w2, 3, nullptr, true));
  });
  section(c + "scorePosesDev", [&] {
    a.scorePosesDev(A.x, A.y, N, A.poses, M, A.scores, producer);
    a.scorePosesDev(A.x, A.y, N, A.poses, M, A.scores, nullptr, true);
  });
  section(c + "polarToPointsDev", [&] {
    NdtMatcherHip::polarToPointsDev(A.ranges, N, -1.5, 0.25, 0.1, 30.0, A.ox, A.oy, &A.other_stream);
  });
  // (the overloads have a section each: a section ends at its first throw, and both `where` strings are to be seen)
  section(c + "polarToPointsDev/deskew", [&] {
    NdtMatcherHip::polarToPointsDev(A.ranges, N, -1.5, 0.25, 0.1, 30.0, D2::pose(1), 0.125, 0.0625, 0.75, A.ox, A.oy, &A.other_stream);
  });
  section(c + "deskewPointsDev", [&] {
    NdtMatcherHip::deskewPointsDev(A.x, A.y, A.frac, N, D2::pose(1), 0.75, A.ox, A.oy, &A.other_stream);
  });
  section(c + "scoreParticlesDev", [&] {
    a.scoreParticlesDev(A.x, A.y, N, A.poses, M, A.scores, A.n_hit, producer);
    a.scoreParticlesDev(A.x, A.y, N, A.poses, M, A.scores, nullptr, nullptr, true);
  });
  section(c + "scoreParticlesAsync", [&] {
    a.scoreParticlesAsync(A.x, A.y, N, A.poses, M, A.scores, A.n_hit, producer);
    a.scoreParticlesAsync(A.x, A.y, N, A.poses, M, A.scores, nullptr, nullptr, true);
  });
  section(c + "scoreParticles", [&] { a.scoreParticles(A.x, A.y, N, A.poses, M, A.scores, A.n_hit); });
  section(c + "bestPosesDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestPosesDev(A.x, A.y, N, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestPosesDev(A.x, A.y, N, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "bestPosesAlignDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestPosesAlignDev(A.x, A.y, N, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestPosesAlignDev(A.x, A.y, N, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "to_search_hit", [&] {
    ndt2d_search_hit h{};
    for (int i = 0; i < 3; ++i) h.pose[i] = 2.5 + i;
    h.score = 1.75f; h.index = 42;
    show(NdtMatcherHip::to_search_hit(h));
  }, 1);
  section(c + "evaluate", [&] { show(a.evaluate(A.x, A.y, N, D2::pose(1))); });
  section(c + "fitPointsDev", [&] {
    show(a.fitPointsDev(A.x, A.y, N, D2::pose(1), 9.5f));
    show(a.fitPointsDev(A.x, A.y, N, D2::pose(2), 9.5f, A.m, A.cls));
  });
  section(c + "selectPointsDev", [&] {
    show(a.selectPointsDev(A.x, A.y, N, D2::pose(1), 9.5f, 12u, A.ox, A.oy));
    show(a.selectPointsDev(A.x, A.y, N, D2::pose(2), 9.5f, 12u, A.ox, A.oy, A.index));
  });
  section(c + "voxelFilterDev", [&] {
    show(a.voxelFilterDev(A.x, A.y, N, 0.25, A.ox, A.oy, N));
    show(a.voxelFilterDev(A.x, A.y, N, 0.25, A.ox, A.oy, N, 2u, A.count));
  });
}

// ---- NdtMatcherHip3: the members that take (x, y, z) ---------------------------------------------------------------------
void matcher3_sections(NdtMatcherHip3& a) {
  const std::string c = "NdtMatcherHip3.";
  void* const producer = &A.producer;
  section(c + "setTarget", [&] { a.setTarget(A.x, A.y, A.z, N); });
  section(c + "setTuning", [&] { a.setTuning(3, 4); });
  section(c + "setNeighbourhood", [&] { a.setNeighbourhood(7); });
  section(c + "neighbourhood", [&] { const NdtMatcherHip3& ca = a; show((size_t)ca.neighbourhood()); });
  section(c + "addTargetPoints", [&] { show(a.addTargetPoints(A.x, A.y, A.z, N)); });
  section(c + "reserveTarget", [&] { a.reserveTarget({-1.5, -2.5, -3.5}, {1.5, 2.5, 3.5}); });
  section(c + "addTargetPointsDev", [&] {
    const Pose3 p = D3::pose(1);
    show(a.addTargetPointsDev(A.x, A.y, A.z, N));
    show(a.addTargetPointsDev(A.x, A.y, A.z, N, &p, producer));
  });
  section(c + "removeTargetPoints", [&] { show(a.removeTargetPoints(A.x, A.y, A.z, N)); });
  section(c + "removeTargetPointsDev", [&] {
    const Pose3 p = D3::pose(2);
    show(a.removeTargetPointsDev(A.x, A.y, A.z, N));
    show(a.removeTargetPointsDev(A.x, A.y, A.z, N, &p, producer));
  });
  section(c + "fitPointsDev", [&] {
    show(a.fitPointsDev(A.x, A.y, A.z, N, D3::pose(1), 9.5f));
    show(a.fitPointsDev(A.x, A.y, A.z, N, D3::pose(2), 9.5f, A.m, A.cls));
  });
  section(c + "selectPointsDev", [&] {
    show(a.selectPointsDev(A.x, A.y, A.z, N, D3::pose(1), 9.5f, 12u, A.ox, A.oy, A.oz));
    show(a.selectPointsDev(A.x, A.y, A.z, N, D3::pose(2), 9.5f, 12u, A.ox, A.oy, A.oz, A.index));
  });
  section(c + "voxelFilterDev", [&] {
    show(a.voxelFilterDev(A.x, A.y, A.z, N, 0.25, A.ox, A.oy, A.oz, N));
    show(a.voxelFilterDev(A.x, A.y, A.z, N, 0.25, A.ox, A.oy, A.oz, N, 2u, A.count));
  });
  section(c + "alignDev", [&] {
    show(a.alignDev(A.x, A.y, A.z, N));
    show(a.alignDev(A.x, A.y, A.z, N, D3::pose(1)));
  });
  section(c + "alignMultiScanDev", [&] {
    const std::vector<NdtMatcherHip3::DeviceScan3> scans = {NdtMatcherHip3::DeviceScan3{A.x, A.y, A.z, N},
                                                            NdtMatcherHip3::DeviceScan3{A.x2, A.y2, A.z2, 3}};
    show(a.alignMultiScanDev(scans, {D3::pose(1), D3::pose(2)}));
  });
  section(c + "alignMultiScanDev/mismatch", [&] {
    a.alignMultiScanDev({NdtMatcherHip3::DeviceScan3{A.x, A.y, A.z, N}}, {D3::pose(1), D3::pose(2)});
  });
  section(c + "alignMultiScanDev/empty", [&] { a.alignMultiScanDev({}, {}); });
  section(c + "alignMultiStartDev", [&] { show(a.alignMultiStartDev(A.x, A.y, A.z, N, {D3::pose(1), D3::pose(2)})); });
  section(c + "alignMultiStartDev/empty", [&] { a.alignMultiStartDev(A.x, A.y, A.z, N, {}); });
  section(c + "searchDev", [&] {
    for (int k : {3, 0, -1}) show(a.searchDev(A.x, A.y, A.z, N, A.w3, k, producer));
    show(a.searchDev(A.x, A.y, A.z, N, A.w3, 3, nullptr, true));
  });
  section(c + "searchAlignDev", [&] {
    for (int k : {3, 0, -1}) show(a.searchAlignDev(A.x, A.y, A.z, N, A.w3, k, producer));
    show(a.searchAlignDev(A.x, A.y, A.z, N, A.w3, 3, nullptr, true));
  });
  section(c + "scorePosesDev", [&] {
    a.scorePosesDev(A.x, A.y, A.z, N, A.poses, M, A.scores, producer);
    a.scorePosesDev(A.x, A.y, A.z, N, A.poses, M, A.scores, nullptr, true);
  });
  section(c + "rangeImageToPointsDev", [&] {
    NdtMatcherHip3::rangeImageToPointsDev(A.ranges, 2, 2, A.elevations, -1.5, 0.25, 0.1, 30.0, A.ox, A.oy, A.oz, &A.other_stream);
  });
  section(c + "rangeImageToPointsDev/deskew", [&] {
    NdtMatcherHip3::rangeImageToPointsDev(A.ranges, 2, 2, A.elevations, -1.5, 0.25, 0.1, 30.0, D3::pose(1), 0.125, 0.0625, 0.75, A.ox,
                                          A.oy, A.oz, &A.other_stream);
  });
  section(c + "deskewPointsDev", [&] {
    NdtMatcherHip3::deskewPointsDev(A.x, A.y, A.z, A.frac, N, D3::pose(1), 0.75, A.ox, A.oy, A.oz, &A.other_stream);
  });
  section(c + "scoreParticlesDev", [&] {
    a.scoreParticlesDev(A.x, A.y, A.z, N, A.poses, M, A.scores, A.n_hit, producer);
    a.scoreParticlesDev(A.x, A.y, A.z, N, A.poses, M, A.scores, nullptr, nullptr, true);
  });
  section(c + "scoreParticlesAsync", [&] {
    a.scoreParticlesAsync(A.x, A.y, A.z, N, A.poses, M, A.scores, A.n_hit, producer);
    a.scoreParticlesAsync(A.x, A.y, A.z, N, A.poses, M, A.scores, nullptr, nullptr, true);
  });
  section(c + "scoreParticles", [&] { a.scoreParticles(A.x, A.y, A.z, N, A.poses, M, A.scores, A.n_hit); });
  section(c + "bestPosesDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestPosesDev(A.x, A.y, A.z, N, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestPosesDev(A.x, A.y, A.z, N, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "bestPosesAlignDev", [&] {
    for (int k : {3, 0, -1}) show(a.bestPosesAlignDev(A.x, A.y, A.z, N, A.poses, M, k, 0.5, 0.25, producer));
    show(a.bestPosesAlignDev(A.x, A.y, A.z, N, A.poses, M, 3, 0.5, 0.25, nullptr, true));
  });
  section(c + "toSearchHit", [&] {
    ndt3d_search_hit h{};
    for (int i = 0; i < 6; ++i) h.pose[i] = 2.5 + i;
    h.score = 1.75f; h.index = 42;
    show(NdtMatcherHip3::toSearchHit(h));
  }, 1);
  section(c + "align", [&] {
    show(a.align(A.x, A.y, A.z, N));
    show(a.align(A.x, A.y, A.z, N, D3::pose(1)));
  });
  section(c + "toMatchResult", [&] {
    ndt3d_result r{};
    for (int i = 0; i < 6; ++i) { r.pose[i] = 1.5 + i; r.g[i] = 9.0; }
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) r.H[6 * i + j] = (i == j ? 10.0 + i : 0.0) + 0.125 * (i < j ? 6 * i + j : 6 * j + i);
    r.score = 12.5; r.iterations = 7; r.n_hit = 33; r.status = NDT_NOT_CONVERGED;
    show(NdtMatcherHip3::toMatchResult(r));
  }, 1);
}

// ---- pyramid, batch, multi-device -------------------------------------------------------------------------------------
std::vector<Pose2> poses2(size_t n) { std::vector<Pose2> v; for (size_t k = 0; k < n; ++k) v.push_back(D2::pose(1.0 + k)); return v; }
std::vector<Pose3> poses3(size_t n) { std::vector<Pose3> v; for (size_t k = 0; k < n; ++k) v.push_back(D3::pose(1.0 + k)); return v; }

void pyramid_sections() {
  std::unique_ptr<NdtPyramidHip> p;
  section("NdtPyramidHip.NdtPyramidHip", [&] {
    p.reset(new NdtPyramidHip());
    NdtPyramidHip custom(NdtMatcherHip::defaultParams(), 1, {NdtPyramidHip::Level{8.0, 0.2}});
  });
  section("NdtPyramidHip.setTarget", [&] { p->setTarget(A.x, A.y, N); });
  section("NdtPyramidHip.align", [&] { show(p->align(A.x, A.y, N)); show(p->align(A.x, A.y, N, D2::pose(1))); });
  section("NdtPyramidHip.~NdtPyramidHip", [&] { p.reset(); }, 1);
}

template <class Batch, class Poses>
void batch_align_sections(const std::string& c, Batch& b, Batch& b0, const std::vector<typename Batch::Cloud>& t,
                          const std::vector<typename Batch::Cloud>& s, Poses poses) {
  section(c + "align", [&] { show(b.align(t, s, poses(2))); show(b0.align(t, s, poses(2))); });
  section(c + "align/mismatch", [&] { b.align(t, {s[0]}, poses(2)); });
  section(c + "align/guesses", [&] { b.align(t, s, poses(1)); });
  section(c + "align/empty", [&] { b.align({}, {}, {}); });
}

void batch_sections() {
  std::unique_ptr<NdtBatchHip> b, bp, b0;
  section("NdtBatchHip.standardPyramid", [] {
    for (const ndt2d_params& p : NdtBatchHip::standardPyramid()) show(p);
    ndt2d_params fine = NdtMatcherHip::defaultParams();
    fine.cell_size = 0.125;
    for (const ndt2d_params& p : NdtBatchHip::standardPyramid(fine)) show(p);
  });
  section("NdtBatchHip.NdtBatchHip", [&] {
    NdtBatchHip d;
    b.reset(new NdtBatchHip(NdtMatcherHip::defaultParams(), 1));
  });
  section("NdtBatchHip.NdtBatchHip/levels", [&] {
    b0.reset(new NdtBatchHip(std::vector<ndt2d_params>{}, 0));
    bp.reset(new NdtBatchHip(NdtBatchHip::standardPyramid(), 1));
  });
  section("NdtBatchHip.setTuning", [&] { b->setTuning(5, 6); });
  const std::vector<NdtBatchHip::Cloud> t = {NdtBatchHip::Cloud{A.x, A.y, 3}, NdtBatchHip::Cloud{A.x2, A.y2, 5}};
  const std::vector<NdtBatchHip::Cloud> s = {NdtBatchHip::Cloud{A.ox, A.oy, 5}, NdtBatchHip::Cloud{A.x, A.y, 3}};
  batch_align_sections("NdtBatchHip.", *b, *b0, t, s, poses2);
  section("NdtBatchHip.~NdtBatchHip", [&] { b.reset(); bp.reset(); b0.reset(); }, 1);

  std::unique_ptr<NdtBatchHip3> c, c0;
  section("NdtBatchHip3.NdtBatchHip3", [&] {
    NdtBatchHip3 d;
    c.reset(new NdtBatchHip3(NdtMatcherHip3::defaultParams(), 1));
  });
  section("NdtBatchHip3.NdtBatchHip3/levels", [&] {
    c0.reset(new NdtBatchHip3(std::vector<ndt3d_params>{}, 0));
    NdtBatchHip3 two(std::vector<ndt3d_params>(2, NdtMatcherHip3::defaultParams()), 1);
  });
  section("NdtBatchHip3.setTuning", [&] { c->setTuning(5, 6); });
  const std::vector<NdtBatchHip3::Cloud> t3 = {NdtBatchHip3::Cloud{A.x, A.y, A.z, 3}, NdtBatchHip3::Cloud{A.x2, A.y2, A.z2, 5}};
  const std::vector<NdtBatchHip3::Cloud> s3 = {NdtBatchHip3::Cloud{A.ox, A.oy, A.oz, 5}, NdtBatchHip3::Cloud{A.x, A.y, A.z, 3}};
  batch_align_sections("NdtBatchHip3.", *c, *c0, t3, s3, poses3);
  section("NdtBatchHip3.alignDev", [&] {
    c->alignDev(A.x, A.y, A.z, A.toff, A.x2, A.y2, A.z2, A.soff, A.init, 2, A.results);
    c->alignDev(A.x, A.y, A.z, A.toff, A.x2, A.y2, A.z2, A.soff, A.init, 2, A.results, &A.other_stream);
  });
  section("NdtBatchHip3.stream", [&] { show_ptr(c->stream()); });
  section("NdtBatchHip3.~NdtBatchHip3", [&] { c.reset(); c0.reset(); }, 1);
}

void multi_sections() {
  std::unique_ptr<NdtMultiHip> m, m0;
  section("NdtMultiHip.NdtMultiHip", [&] {
    NdtMultiHip d;
    m.reset(new NdtMultiHip(NdtMatcherHip::defaultParams(), {1, 0}));
  });
  section("NdtMultiHip.NdtMultiHip/levels", [&] {
    m0.reset(new NdtMultiHip(std::vector<ndt2d_params>{}, {1}));
    NdtMultiHip pyr(NdtBatchHip::standardPyramid(), {});
  });
  section("NdtMultiHip.deviceCount", [&] { const NdtMultiHip& cm = *m; show((size_t)cm.deviceCount()); });
  const std::vector<NdtMultiHip::Cloud> t = {NdtMultiHip::Cloud{A.x, A.y, 3}, NdtMultiHip::Cloud{A.x2, A.y2, 5}};
  const std::vector<NdtMultiHip::Cloud> s = {NdtMultiHip::Cloud{A.ox, A.oy, 5}, NdtMultiHip::Cloud{A.x, A.y, 3}};
  batch_align_sections("NdtMultiHip.", *m, *m0, t, s, poses2);
  NdtMultiHip::DeviceShard s0, s1;
  s0.tx = A.x; s0.ty = A.y; s0.toff = A.toff; s0.sx = A.ox; s0.sy = A.oy; s0.soff = A.soff; s0.init = A.init; s0.n_pairs = 2;
  s1.tx = A.x2; s1.ty = A.y2; s1.toff = A.toff + 1; s1.sx = A.x; s1.sy = A.y; s1.soff = A.soff + 1; s1.init = A.init + 6; s1.n_pairs = 1;
  section("NdtMultiHip.alignDev", [&] { show(m->alignDev({s0, s1})); show(m0->alignDev({s1, s0})); });
  section("NdtMultiHip.alignDev/one-shard", [&] { m->alignDev({s0}); });
  section("NdtMultiHip.~NdtMultiHip", [&] { m.reset(); m0.reset(); }, 1);

  std::unique_ptr<NdtMultiHip3> m3;
  section("NdtMultiHip3.NdtMultiHip3", [&] {
    NdtMultiHip3 d;
    m3.reset(new NdtMultiHip3(NdtMatcherHip3::defaultParams(), {1, 0}));
  });
  section("NdtMultiHip3.deviceCount", [&] { const NdtMultiHip3& cm = *m3; show((size_t)cm.deviceCount()); });
  section("NdtMultiHip3.raw", [&] { show_ptr(m3->raw()); });
  section("NdtMultiHip3.~NdtMultiHip3", [&] { m3.reset(); }, 1);
}

template <class D>
void matcher_life(void (*own)(typename D::Matcher&)) {
  using Mt = typename D::Matcher;
  const std::string c = std::string(D::name) + ".";
  std::unique_ptr<Mt> a, b;
  section(c + D::name, [&] {
    a.reset(new Mt());
    auto p = Mt::defaultParams();
    p.hessian_mode = NDT_HESSIAN_GAUSS_NEWTON;
    p.cell_size = 4.0;
    b.reset(new Mt(p, 1));
  });
  own(*a);
  shared_sections<D>(*a, *b);
  section(c + "~" + D::name, [&] { a.reset(); b.reset(); }, 1);
}
}  // namespace

int main() {
  for (size_t i = 0; i < N; ++i) {
    A.x[i] = 1.0f + i; A.y[i] = 11.0f + i; A.z[i] = 21.0f + i; A.x2[i] = 31.0f + i; A.y2[i] = 41.0f + i; A.z2[i] = 51.0f + i;
    A.ox[i] = 61.0f + i; A.oy[i] = 71.0f + i; A.oz[i] = 81.0f + i;
  }
  stub_arena(&A, sizeof(A));
  free_function_sections();
  matcher_life<D2>(matcher2_sections);
  matcher_life<D3>(matcher3_sections);
  pyramid_sections();
  batch_sections();
  multi_sections();
  return 0;
}

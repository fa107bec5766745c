// ndt_matcher_hip.hpp - header-only C++ adapter over the C ABI (ndt_hip.h).
//
// This is the host-side mirror of the scan-matcher interface named by BASELINE.json's
// north_star ("the repo's existing scan-matcher -> GTSAM-factor interface").  The reference
// checkout shows no such interface (/root/reference/README.md:1 is its only line), so the
// class below is this repo's proposal of the smallest one a SLAM front end needs:
//   setTarget(scan or submap)  ->  align(scan, initial guess)  ->  pose + information.
// INTEGRATION.md shows how a maintainer maps it onto the real interface.
//
// No GPU code here: everything goes through extern "C" entry points of libndt_hip.so.
#ifndef NDT_MATCHER_HIP_HPP_
#define NDT_MATCHER_HIP_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "ndt_hip.h"

namespace ndt {

struct Pose2 {           // tx, ty, theta: maps source-frame points into the target frame
  double x = 0.0, y = 0.0, theta = 0.0;
};

struct MatchResult {
  Pose2 pose;
  std::array<double, 9> information{};   // row-major 3x3 Hessian of -score at the last evaluation
  std::array<double, 9> covariance{};    // calibrated pose covariance S H^-1 S (ndt2d_calibrated_covariance;
                                         // zero if the Hessian is not positive definite)
  double score = 0.0;
  int iterations = 0;
  int n_hit = 0;
  int status = NDT_OK;                   // NDT_OK / NDT_NOT_CONVERGED / ...
  bool converged() const { return status == NDT_OK; }
};

class NdtError : public std::runtime_error {
 public:
  NdtError(int32_t code, const std::string& where)
      : std::runtime_error(where + ": " + ndt_status_string(code) + " (" + std::to_string(code) + ") " +
                           ndt_last_error()),
        code_(code) {}
  int32_t code() const { return code_; }

 private:
  int32_t code_;
};

inline bool invert3(const double* H, double* C) {
  const double a = H[0], b = H[1], c = H[2], d = H[4], e = H[5], f = H[8];   // symmetric
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  if (!(det > 0.0) && !(det < 0.0)) { for (int i = 0; i < 9; ++i) C[i] = 0.0; return false; }
  const double id = 1.0 / det;
  C[0] = c00 * id; C[1] = c01 * id; C[2] = c02 * id;
  C[3] = C[1];     C[4] = (a * f - c * c) * id; C[5] = (b * c - a * e) * id;
  C[6] = C[2];     C[7] = C[5];                 C[8] = (a * d - b * b) * id;
  return true;
}

inline MatchResult to_match_result(const ndt2d_result& r, int32_t hessian_mode = NDT_HESSIAN_GAUSS_NEWTON) {
  MatchResult m;
  m.pose = {r.pose[0], r.pose[1], r.pose[2]};
  for (int i = 0; i < 9; ++i) m.information[i] = r.H[i];
  (void)ndt2d_calibrated_covariance(r.H, hessian_mode, m.covariance.data());
  m.score = r.score; m.iterations = r.iterations; m.n_hit = r.n_hit; m.status = r.status;
  return m;
}

// The calibrated covariance in the tangent frame of the measured pose, which is what a
// gtsam::BetweenFactor<Pose2> noise model expects (its error is Logmap(measured^-1 * predicted), i.e.
// translation errors expressed in the measured pose's own axes): C_local = A C A' with
// A = diag(R(theta)', 1).  MatchResult::covariance itself is for additive errors on (tx, ty, theta)
// in the target frame.
inline std::array<double, 9> covarianceInLocalFrame(const MatchResult& m) {
  const double c = std::cos(m.pose.theta), s = std::sin(m.pose.theta);
  const double A[9] = {c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0};
  double T[9];
  std::array<double, 9> out{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      T[3 * i + j] = 0.0;
      for (int k = 0; k < 3; ++k) T[3 * i + j] += A[3 * i + k] * m.covariance[3 * k + j];
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) out[3 * i + j] += T[3 * i + k] * A[3 * j + k];
  return out;
}

// One matcher = one device stream + one cached target grid.  Not thread-safe; use one
// instance per thread (distinct instances are independent).
class NdtMatcherHip {
 public:
  static ndt2d_params defaultParams() { ndt2d_params p; ndt2d_default_params(&p); return p; }

  explicit NdtMatcherHip(const ndt2d_params& params = defaultParams(), int device = 0) : mode_(params.hessian_mode) {
    const int32_t st = ndt2d_create(&params, device, &h_);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_create");
  }
  ~NdtMatcherHip() { ndt2d_destroy(h_); }
  NdtMatcherHip(const NdtMatcherHip&) = delete;
  NdtMatcherHip& operator=(const NdtMatcherHip&) = delete;

  // (i) target grid from SoA float arrays
  void setTarget(const float* x, const float* y, size_t n) { check(ndt2d_set_target(h_, x, y, n), "ndt2d_set_target"); }
  void setTarget(const std::vector<float>& x, const std::vector<float>& y) { setTarget(x.data(), y.data(), x.size()); }
  // empty grid over the extent the submap may grow into; fill with addTargetPoints(Dev)
  void reserveTarget(double xmin, double ymin, double xmax, double ymax) {
    check(ndt2d_reserve_target(h_, xmin, ymin, xmax, ymax), "ndt2d_reserve_target");
  }
  // incremental submap update: returns the number of points outside the cached extent
  size_t addTargetPoints(const float* x, const float* y, size_t n) {
    size_t outside = 0;
    check(ndt2d_add_target_points(h_, x, y, n, &outside), "ndt2d_add_target_points");
    return outside;
  }
  // points already on the device, moved into the map frame by `pose` first (nullptr: as they are)
  size_t addTargetPointsDev(const float* d_x, const float* d_y, size_t n, const Pose2* pose = nullptr,
                            void* producer_stream = nullptr) {
    size_t outside = 0;
    const double p[3] = {pose ? pose->x : 0.0, pose ? pose->y : 0.0, pose ? pose->theta : 0.0};
    check(ndt2d_add_target_points_dev(h_, d_x, d_y, n, pose ? p : nullptr, &outside, producer_stream),
          "ndt2d_add_target_points_dev");
    return outside;
  }
  // the exact inverse of addTargetPoints(Dev): the points leave the cached grid's sums (throws when they are not in the
  // map); removing a scan at its old pose and adding it at a new one re-anchors it after a loop closure
  size_t removeTargetPoints(const float* x, const float* y, size_t n) {
    size_t outside = 0;
    check(ndt2d_remove_target_points(h_, x, y, n, &outside), "ndt2d_remove_target_points");
    return outside;
  }
  size_t removeTargetPointsDev(const float* d_x, const float* d_y, size_t n, const Pose2* pose = nullptr,
                               void* producer_stream = nullptr) {
    size_t outside = 0;
    const double p[3] = {pose ? pose->x : 0.0, pose ? pose->y : 0.0, pose ? pose->theta : 0.0};
    check(ndt2d_remove_target_points_dev(h_, d_x, d_y, n, pose ? p : nullptr, &outside, producer_stream),
          "ndt2d_remove_target_points_dev");
    return outside;
  }
  ndt2d_grid_info gridInfo() const { ndt2d_grid_info g; check(ndt2d_get_grid_info(h_, &g), "ndt2d_get_grid_info"); return g; }
  // submap persistence: the cached grid as a flat buffer (ndt_map_header + exact per-cell sums), and back - bit for
  // bit the same grid when the loading matcher has the saving one's parameters; it goes on taking points
  std::vector<unsigned char> saveMap() const {
    std::vector<unsigned char> buf(ndt2d_map_size(h_));
    check(ndt2d_save_map(h_, buf.data(), buf.size(), nullptr), "ndt2d_save_map");
    return buf;
  }
  void loadMap(const std::vector<unsigned char>& buf) { check(ndt2d_load_map(h_, buf.data(), buf.size()), "ndt2d_load_map"); }
  // dst (cell_size exactly 2 or 4 times this matcher's) receives the grid whose cells are unions of this grid's, from the
  // exact per-cell sums alone (ndt2d_coarsen_map): a pyramid level for a submap that holds no points
  void coarsenInto(NdtMatcherHip& dst) { check(ndt2d_coarsen_map(h_, dst.h_), "ndt2d_coarsen_map"); }

  // (ii)+(iii)+solve: full alignment from an initial guess
  MatchResult align(const float* sx, const float* sy, size_t n, const Pose2& guess = Pose2()) {
    const double init[3] = {guess.x, guess.y, guess.theta};
    ndt2d_result r;
    check(ndt2d_align(h_, sx, sy, n, init, &r), "ndt2d_align");
    return to_match_result(r, mode_);
  }
  MatchResult align(const std::vector<float>& sx, const std::vector<float>& sy, const Pose2& guess = Pose2()) {
    return align(sx.data(), sy.data(), sx.size(), guess);
  }
  // Source scan already on the device (e.g. from ndt2d_polar_to_points_dev).  producer_stream is
  // the stream that wrote d_sx / d_sy: the handle's own stream is ordered behind it first
  // (ndt2d_wait_stream; nullptr = the legacy default stream); complete = true when those arrays are
  // known to be complete (the producer was synchronised), which skips the ordering.  The same holds for arrays
  // written on the handle's own stream (ndt2d_stream): pass that stream as producer_stream, it is not implied.
  MatchResult alignDev(const float* d_sx, const float* d_sy, size_t n, const Pose2& guess, void* producer_stream,
                       bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    const double init[3] = {guess.x, guess.y, guess.theta};
    ndt2d_result r;
    check(ndt2d_align_dev(h_, d_sx, d_sy, n, init, &r), "ndt2d_align_dev");
    return to_match_result(r, mode_);
  }
  // Several starts around a poor guess in one launch chain (ndt2d_align_multi_start_dev, at most 64):
  // result k is what alignDev(guesses[k]) returns; pick e.g. the best score among the converged ones.
  std::vector<MatchResult> alignMultiStartDev(const float* d_sx, const float* d_sy, size_t n, const std::vector<Pose2>& guesses,
                                              void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<double> init(3 * guesses.size());
    for (size_t k = 0; k < guesses.size(); ++k) { init[3 * k] = guesses[k].x; init[3 * k + 1] = guesses[k].y; init[3 * k + 2] = guesses[k].theta; }
    std::vector<ndt2d_result> r(guesses.size());
    check(ndt2d_align_multi_start_dev(h_, d_sx, d_sy, n, init.data(), (int32_t)guesses.size(), r.data()),
          "ndt2d_align_multi_start_dev");
    std::vector<MatchResult> out;
    for (const ndt2d_result& q : r) out.push_back(to_match_result(q, mode_));
    return out;
  }
  // Several different device scans against the cached grid in one launch chain (ndt2d_align_multi_scan_dev,
  // at most 64): scans[k] = {d_x, d_y, n}; result k is what alignDev(scans[k], guesses[k]) returns.
  struct DeviceScan { const float* x; const float* y; size_t n; };
  std::vector<MatchResult> alignMultiScanDev(const std::vector<DeviceScan>& scans, const std::vector<Pose2>& guesses,
                                             void* producer_stream, bool complete = false) {
    if (scans.size() != guesses.size() || scans.empty()) throw NdtError(NDT_ERR_INVALID_ARG, "alignMultiScanDev");
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    const size_t m = scans.size();
    std::vector<const float*> px(m), py(m);
    std::vector<size_t> n(m);
    std::vector<double> init(3 * m);
    for (size_t k = 0; k < m; ++k) {
      px[k] = scans[k].x; py[k] = scans[k].y; n[k] = scans[k].n;
      init[3 * k] = guesses[k].x; init[3 * k + 1] = guesses[k].y; init[3 * k + 2] = guesses[k].theta;
    }
    std::vector<ndt2d_result> r(m);
    check(ndt2d_align_multi_scan_dev(h_, px.data(), py.data(), n.data(), init.data(), (int32_t)m, r.data()),
          "ndt2d_align_multi_scan_dev");
    std::vector<MatchResult> out;
    for (const ndt2d_result& q : r) out.push_back(to_match_result(q, mode_));
    return out;
  }
  // Exhaustive pose search over an (x, y, theta) window against the cached grid (ndt2d_search_dev; lattice, peaks and
  // separation: ndt_hip.h): the best k (1..64) well-separated lattice poses, best first.  For a loop-closure candidate
  // or a relocalisation whose guess is metres and tens of degrees off, where alignDev's basin (about one cell) is too
  // narrow.  producer_stream as in alignMultiStartDev.
  struct SearchHit {
    Pose2 pose;            // the lattice pose, theta wrapped to (-pi, pi]
    float score = 0.f;     // the lattice score
    int32_t index = 0;     // flat lattice index
  };
  struct SearchMatch {
    SearchHit hit;
    MatchResult result;    // alignMultiStartDev's result from hit.pose
  };
  std::vector<SearchHit> searchDev(const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window& window, int k,
                                   void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt2d_search_dev(h_, d_sx, d_sy, n, &window, (int32_t)k, hits.data(), &n_hits), "ndt2d_search_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(to_search_hit(hits[i]));
    return out;
  }
  // searchDev, then one alignment from every hit in one launch chain (ndt2d_search_align_dev): result i is bit for bit
  // what alignMultiStartDev returns from the hits' poses.  The best match is usually the converged result of highest
  // score.
  std::vector<SearchMatch> searchAlignDev(const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window& window,
                                          int k, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt2d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt2d_search_align_dev(h_, d_sx, d_sy, n, &window, (int32_t)k, hits.data(), r.data(), &n_hits),
          "ndt2d_search_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{to_search_hit(hits[i]), to_match_result(r[i], mode_)});
    return out;
  }
  // The score at every pose of a list in one launch (ndt2d_score_poses_dev; contract: ndt_hip.h): d_poses is [m][3] =
  // (x, y, theta) in double, d_scores [m] floats, both device memory - the weights of a particle filter's particles.  A
  // non-finite pose scores 0.  producer_stream: the stream that wrote the scan and the list.
  void scorePosesDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                     void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    check(ndt2d_score_poses_dev(h_, d_sx, d_sy, n, d_poses, m, d_scores), "ndt2d_score_poses_dev");
  }
  // the handle's stream (hipStream_t as void*): what scoreParticlesAsync's outputs are ordered on
  void* stream() { return ndt2d_stream(h_); }
  // The driver side of the boundary, on the caller's stream (no handle involved; all pointers are device pointers):
  // ranges -> points (ndt2d_polar_to_points_dev) and, with the sensor's motion within the sweep, the same de-skewed
  // (ndt2d_polar_to_points_deskew_dev): `motion` is the sensor's pose at the end of the sweep in its frame at the start,
  // beam i was fired at sweep fraction frac0 + i * frac_inc, the points come out in the sensor frame at ref_frac.
  static void polarToPointsDev(const float* d_ranges, size_t n, double angle_min, double angle_inc, double range_min,
                               double range_max, float* d_x, float* d_y, void* stream) {
    check(ndt2d_polar_to_points_dev(d_ranges, n, angle_min, angle_inc, range_min, range_max, d_x, d_y, stream),
          "ndt2d_polar_to_points_dev");
  }
  static void polarToPointsDev(const float* d_ranges, size_t n, double angle_min, double angle_inc, double range_min,
                               double range_max, const Pose2& motion, double frac0, double frac_inc, double ref_frac,
                               float* d_x, float* d_y, void* stream) {
    const double delta[3] = {motion.x, motion.y, motion.theta};
    check(ndt2d_polar_to_points_deskew_dev(d_ranges, n, angle_min, angle_inc, range_min, range_max, delta, frac0, frac_inc,
                                           ref_frac, d_x, d_y, stream), "ndt2d_polar_to_points_deskew_dev");
  }
  // prev^-1 o cur: the motion between the last two estimates, the constant-velocity guess of the next sweep's motion
  static Pose2 sweepMotion(const Pose2& prev, const Pose2& cur) {
    const double p[3] = {prev.x, prev.y, prev.theta}, c[3] = {cur.x, cur.y, cur.theta};
    double d[3];
    check(ndt2d_sweep_motion(p, c, d), "ndt2d_sweep_motion");
    Pose2 out;
    out.x = d[0]; out.y = d[1]; out.theta = d[2];
    return out;
  }
  // Device points with a sweep fraction each -> the sensor frame at ref_frac (ndt2d_deskew_points_dev); the outputs may
  // be the inputs
  static void deskewPointsDev(const float* d_x, const float* d_y, const float* d_frac, size_t n, const Pose2& motion,
                              double ref_frac, float* d_ox, float* d_oy, void* stream) {
    const double delta[3] = {motion.x, motion.y, motion.theta};
    check(ndt2d_deskew_points_dev(d_x, d_y, d_frac, n, delta, ref_frac, d_ox, d_oy, stream), "ndt2d_deskew_points_dev");
  }
  // scorePosesDev for SHORT lists (a particle filter's particles; the faster call at every size measured): a team of lanes per pose
  // (ndt2d_score_particles_dev; contract: ndt_hip.h).  d_n_hit [m] (may be null): the lookups that hit a valid cell,
  // evaluate's n_hit at that pose.  The scores differ from scorePosesDev's only by the order of the float32 sum.
  void scoreParticlesDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                         uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    check(ndt2d_score_particles_dev(h_, d_sx, d_sy, n, d_poses, m, d_scores, d_n_hit), "ndt2d_score_particles_dev");
  }
  // the same, returning after the enqueue (ndt2d_score_particles_async): the outputs are complete in stream order on
  // stream() (ndt2d_stream); the scan, the list and the outputs stay alive until then
  void scoreParticlesAsync(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                           uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    check(ndt2d_score_particles_async(h_, d_sx, d_sy, n, d_poses, m, d_scores, d_n_hit), "ndt2d_score_particles_async");
  }
  // the same with host arrays (ndt2d_score_particles); n_hit may be null
  void scoreParticles(const float* sx, const float* sy, size_t n, const double* poses, size_t m, float* scores, uint32_t* n_hit) {
    check(ndt2d_score_particles(h_, sx, sy, n, poses, m, scores, n_hit), "ndt2d_score_particles");
  }
  // the best k (1..64) well-separated poses of the list, best first (ndt2d_best_poses_dev): hit.index is the position in
  // the list, hit.pose the list's pose as it stands there
  std::vector<SearchHit> bestPosesDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, int k,
                                      double min_sep_trans, double min_sep_rot, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt2d_best_poses_dev(h_, d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), &n_hits),
          "ndt2d_best_poses_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(to_search_hit(hits[i]));
    return out;
  }
  // bestPosesDev, then one alignment from every hit in one launch chain (ndt2d_best_poses_align_dev)
  std::vector<SearchMatch> bestPosesAlignDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                             int k, double min_sep_trans, double min_sep_rot, void* producer_stream,
                                             bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt2d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt2d_best_poses_align_dev(h_, d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), r.data(),
                                     &n_hits), "ndt2d_best_poses_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{to_search_hit(hits[i]), to_match_result(r[i], mode_)});
    return out;
  }
  static SearchHit to_search_hit(const ndt2d_search_hit& h) {
    SearchHit s;
    s.pose = {h.pose[0], h.pose[1], h.pose[2]};
    s.score = h.score;
    s.index = h.index;
    return s;
  }
  // one evaluation at a fixed pose, for callers with their own optimiser
  ndt2d_eval evaluate(const float* sx, const float* sy, size_t n, const Pose2& at) {
    const double p[3] = {at.x, at.y, at.theta};
    ndt2d_eval e;
    check(ndt2d_evaluate(h_, sx, sy, n, p, &e), "ndt2d_evaluate");
    return e;
  }
  // Per-point fit of a device scan at a pose (ndt2d_fit_points_dev): m = q' Sigma^-1 q of every point in its cell into
  // d_m and its class byte (NDT_POINT_*) into d_class - either may be null - and the class counts, which count points.
  // The scan must be complete on the device, or the handle ordered behind its producer (ndt2d_wait_stream), as for
  // ndt2d_evaluate_dev.
  ndt_point_fit fitPointsDev(const float* d_sx, const float* d_sy, size_t n, const Pose2& at, float max_m, float* d_m = nullptr,
                             uint8_t* d_class = nullptr) {
    const double p[3] = {at.x, at.y, at.theta};
    ndt_point_fit f;
    check(ndt2d_fit_points_dev(h_, d_sx, d_sy, n, p, max_m, d_m, d_class, &f), "ndt2d_fit_points_dev");
    return f;
  }
  // The points whose class is in `keep` (a mask of 1 << NDT_POINT_*), copied to the front of d_ox / d_oy in the source
  // frame, bit for bit and in their order, their scan indices into d_index (may be null): what addTargetPointsDev(...,
  // &pose) and removeTargetPointsDev take.  The count is the summary's n_selected.
  ndt_point_fit selectPointsDev(const float* d_sx, const float* d_sy, size_t n, const Pose2& at, float max_m, uint32_t keep,
                                float* d_ox, float* d_oy, uint32_t* d_index = nullptr) {
    const double p[3] = {at.x, at.y, at.theta};
    ndt_point_fit f;
    check(ndt2d_select_points_dev(h_, d_sx, d_sy, n, p, max_m, keep, d_ox, d_oy, d_index, &f), "ndt2d_select_points_dev");
    return f;
  }
  // Voxel-grid filter of a device cloud (ndt2d_voxel_filter_dev; docs/ALGORITHM.md 2.24): the centroid of every voxel of the
  // absolute lattice floor(x / leaf) that holds at least min_points points, into d_ox / d_oy[0 .. n_out) in ascending
  // lattice order (iy, ix) - the same bits for every order of the input - and the points per voxel into d_count (may be
  // null).  The outputs hold `capacity` elements (n is always enough) and must not overlap the inputs.  Needs no
  // target; the cloud must be complete on the device, or the handle ordered behind its producer (ndt2d_wait_stream).
  ndt_voxel_filter_info voxelFilterDev(const float* d_x, const float* d_y, size_t n, double leaf, float* d_ox, float* d_oy,
                                       size_t capacity, uint32_t min_points = 1, uint32_t* d_count = nullptr) {
    ndt_voxel_filter_info info;
    check(ndt2d_voxel_filter_dev(h_, d_x, d_y, n, leaf, min_points, d_ox, d_oy, d_count, capacity, &info), "ndt2d_voxel_filter_dev");
    return info;
  }
  // Map-to-map alignment (ndt2d_align_map): `source`'s cached grid against this matcher's, no points involved - the
  // loop closure between two submaps, or between a reloaded map and the current one.  guess and the result map the
  // source map's frame into this map's frame; this matcher's parameters drive the solve; source may be *this.
  // The result's covariance carries the point-to-map calibration factors, which are NOT calibrated for this
  // objective: build a noise model from result.information with factors of your own.
  // Folds `source`'s submap into this matcher's at `pose` (source's frame in this one's: what alignMap(source) returns), from
  // source's exact per-cell sums alone (ndt2d_merge_map: no points, so a map that came back from loadMap merges too);
  // source's cell_size is at most this one's.  Returns the points that fell outside this grid.  unmergeMap with the same
  // arguments takes exactly that out again, whatever was added or removed in between.
  size_t mergeMap(NdtMatcherHip& source, const Pose2& pose) {
    size_t outside = 0;
    const double p[3] = {pose.x, pose.y, pose.theta};
    check(ndt2d_merge_map(h_, source.h_, p, &outside), "ndt2d_merge_map");
    return outside;
  }
  size_t unmergeMap(NdtMatcherHip& source, const Pose2& pose) {
    size_t outside = 0;
    const double p[3] = {pose.x, pose.y, pose.theta};
    check(ndt2d_unmerge_map(h_, source.h_, p, &outside), "ndt2d_unmerge_map");
    return outside;
  }
  MatchResult alignMap(NdtMatcherHip& source, const Pose2& guess = Pose2()) {
    const double init[3] = {guess.x, guess.y, guess.theta};
    ndt2d_result r;
    check(ndt2d_align_map(h_, source.h_, init, &r), "ndt2d_align_map");
    return to_match_result(r, mode_);
  }
  // Up to 64 map-to-map alignments against this matcher's grid in one launch chain (ndt2d_align_map_multi): start k
  // aligns *sources[k] from guesses[k].  The same matcher in every entry is a multi-start; an entry may be this matcher.
  // Result k is bit for bit what alignMap(*sources[k], guesses[k]) returns.
  std::vector<MatchResult> alignMapMulti(const std::vector<NdtMatcherHip*>& sources, const std::vector<Pose2>& guesses) {
    if (sources.size() != guesses.size()) throw NdtError(NDT_ERR_INVALID_ARG, "alignMapMulti: one guess per source");
    std::vector<ndt2d_handle*> hs;
    std::vector<double> init;
    for (size_t k = 0; k < sources.size(); ++k) {
      hs.push_back(sources[k] ? sources[k]->h_ : nullptr);
      init.insert(init.end(), {guesses[k].x, guesses[k].y, guesses[k].theta});
    }
    std::vector<ndt2d_result> r(hs.size());
    check(ndt2d_align_map_multi(h_, hs.data(), init.data(), (int32_t)hs.size(), r.data()), "ndt2d_align_map_multi");
    std::vector<MatchResult> out;
    for (const ndt2d_result& x : r) out.push_back(to_match_result(x, mode_));
    return out;
  }
  ndt2d_eval evaluateMap(NdtMatcherHip& source, const Pose2& at) {
    const double p[3] = {at.x, at.y, at.theta};
    ndt2d_eval e;
    check(ndt2d_evaluate_map(h_, source.h_, p, &e), "ndt2d_evaluate_map");
    return e;
  }
  // The exhaustive search for this objective (ndt2d_search_map / ndt2d_search_align_map): the map-to-map score at every
  // pose of the window's lattice, the best k well-separated peaks, and one alignMap run from each - a submap-to-submap
  // loop closure whose guess is metres off and has no heading.  Window, hits and k as in searchDev.
  std::vector<SearchHit> searchMap(NdtMatcherHip& source, const ndt2d_search_window& window, int k) {
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt2d_search_map(h_, source.h_, &window, (int32_t)k, hits.data(), &n_hits), "ndt2d_search_map");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(to_search_hit(hits[i]));
    return out;
  }
  // the score volume [n_theta][n_y][n_x] itself, into device memory (ndt2d_search_map_scores)
  void searchMapScores(NdtMatcherHip& source, const ndt2d_search_window& window, float* d_scores) {
    check(ndt2d_search_map_scores(h_, source.h_, &window, d_scores), "ndt2d_search_map_scores");
  }
  // result i is bit for bit what alignMap returns from hit i's pose
  std::vector<SearchMatch> searchAlignMap(NdtMatcherHip& source, const ndt2d_search_window& window, int k) {
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt2d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt2d_search_align_map(h_, source.h_, &window, (int32_t)k, hits.data(), r.data(), &n_hits), "ndt2d_search_align_map");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{to_search_hit(hits[i]), to_match_result(r[i], mode_)});
    return out;
  }
  // evaluateMap's score at every pose of a list in one launch (ndt2d_score_map_poses_dev; contract: ndt_hip.h): d_poses is
  // [m][3] = (x, y, theta) in double, d_scores [m] floats, d_n_hit [m] counts of components that fell in a valid cell (may
  // be null), all device memory - the particles of a submap-level filter, samples round a place-recognition hypothesis.
  // A non-finite pose scores 0.  producer_stream: the stream that wrote the list.
  void scoreMapPosesDev(NdtMatcherHip& source, const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit,
                        void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    check(ndt2d_score_map_poses_dev(h_, source.h_, d_poses, m, d_scores, d_n_hit), "ndt2d_score_map_poses_dev");
  }
  // the best k (1..64) well-separated poses of the list, best first (ndt2d_best_map_poses_dev): hit.index is the position
  // in the list, hit.pose the list's pose as it stands there
  std::vector<SearchHit> bestMapPosesDev(NdtMatcherHip& source, const double* d_poses, size_t m, int k, double min_sep_trans,
                                         double min_sep_rot, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt2d_best_map_poses_dev(h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), &n_hits),
          "ndt2d_best_map_poses_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(to_search_hit(hits[i]));
    return out;
  }
  // bestMapPosesDev, then alignMap from every hit in one launch chain (ndt2d_best_map_poses_align_dev): result i is bit
  // for bit what alignMap returns from hit i's pose
  std::vector<SearchMatch> bestMapPosesAlignDev(NdtMatcherHip& source, const double* d_poses, size_t m, int k,
                                                double min_sep_trans, double min_sep_rot, void* producer_stream,
                                                bool complete = false) {
    if (!complete) check(ndt2d_wait_stream(h_, producer_stream), "ndt2d_wait_stream");
    std::vector<ndt2d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt2d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt2d_best_map_poses_align_dev(h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), r.data(),
                                         &n_hits), "ndt2d_best_map_poses_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{to_search_hit(hits[i]), to_match_result(r[i], mode_)});
    return out;
  }
  ndt2d_handle* raw() { return h_; }

 private:
  static void check(int32_t st, const char* where) { if (st < 0) throw NdtError(st, where); }
  ndt2d_handle* h_ = nullptr;
  int32_t mode_ = NDT_HESSIAN_GAUSS_NEWTON;   // the form of the Hessian the results carry (covariance calibration)
};

// Coarse-to-fine alignment: levels of (cell multiplier, eig_ratio)
// above the caller's finest grid widen the convergence basin; each level starts from the
// previous level's pose and the last level runs with the caller's parameters.
class NdtPyramidHip {
 public:
  struct Level { double cell_mult, eig_ratio; };
  explicit NdtPyramidHip(const ndt2d_params& fine = NdtMatcherHip::defaultParams(), int device = 0,
                         std::vector<Level> coarse = {{4.0, 0.1}, {2.0, 0.03}}) {
    for (const Level& l : coarse) {
      ndt2d_params p = fine;
      p.cell_size = fine.cell_size * l.cell_mult;
      p.eig_ratio = l.eig_ratio;
      p.eps_trans = 1e-3; p.eps_rot = 1e-4; p.max_iterations = 30; p.fixed_iterations = 0;
      p.step_max_trans = fine.step_max_trans * l.cell_mult;
      levels_.emplace_back(new NdtMatcherHip(p, device));
    }
    levels_.emplace_back(new NdtMatcherHip(fine, device));
  }
  ~NdtPyramidHip() { for (NdtMatcherHip* m : levels_) delete m; }
  NdtPyramidHip(const NdtPyramidHip&) = delete;
  NdtPyramidHip& operator=(const NdtPyramidHip&) = delete;

  void setTarget(const float* x, const float* y, size_t n) { for (NdtMatcherHip* m : levels_) m->setTarget(x, y, n); }
  MatchResult align(const float* sx, const float* sy, size_t n, const Pose2& guess = Pose2()) {
    Pose2 pose = guess;
    MatchResult r;
    int total = 0;
    for (NdtMatcherHip* m : levels_) {
      r = m->align(sx, sy, n, pose);
      total += r.iterations;
      if (r.status != NDT_OK && r.status != NDT_NOT_CONVERGED) break;
      pose = r.pose;
    }
    r.iterations = total;
    return r;
  }

 private:
  std::vector<NdtMatcherHip*> levels_;
};

namespace detail {
struct CloudView { const float* x; const float* y; size_t n; };

// concatenates the pairs into the SoA + offsets form of ndt2d_batch_align / ndt2d_multi_align
template <class Clouds, class Call>
std::vector<MatchResult> align_pairs(const Clouds& targets, const Clouds& sources, const std::vector<Pose2>& guesses,
                                     const char* what, int32_t hessian_mode, Call&& call) {
  const size_t n = targets.size();
  if (sources.size() != n || guesses.size() != n || n == 0) throw NdtError(NDT_ERR_INVALID_ARG, what);
  std::vector<uint64_t> toff(n + 1, 0), soff(n + 1, 0);
  for (size_t k = 0; k < n; ++k) { toff[k + 1] = toff[k] + targets[k].n; soff[k + 1] = soff[k] + sources[k].n; }
  std::vector<float> tx(toff[n]), ty(toff[n]), sx(soff[n]), sy(soff[n]);
  std::vector<double> init(3 * n);
  for (size_t k = 0; k < n; ++k) {
    std::copy(targets[k].x, targets[k].x + targets[k].n, tx.begin() + toff[k]);
    std::copy(targets[k].y, targets[k].y + targets[k].n, ty.begin() + toff[k]);
    std::copy(sources[k].x, sources[k].x + sources[k].n, sx.begin() + soff[k]);
    std::copy(sources[k].y, sources[k].y + sources[k].n, sy.begin() + soff[k]);
    init[3 * k] = guesses[k].x; init[3 * k + 1] = guesses[k].y; init[3 * k + 2] = guesses[k].theta;
  }
  std::vector<ndt2d_result> res(n);
  const int32_t st = call(tx.data(), ty.data(), toff.data(), sx.data(), sy.data(), soff.data(), init.data(), n, res.data());
  if (st < 0) throw NdtError(st, what);
  std::vector<MatchResult> out;
  out.reserve(n);
  for (const auto& r : res) out.push_back(to_match_result(r, hessian_mode));
  return out;
}
}  // namespace detail

// Loop-closure candidates: many independent pairs in one call.
class NdtBatchHip {
 public:
  struct Cloud { const float* x; const float* y; size_t n; };

  explicit NdtBatchHip(const ndt2d_params& params = NdtMatcherHip::defaultParams(), int device = 0)
      : mode_(params.hessian_mode) {
    const int32_t st = ndt2d_batch_create(&params, device, &b_);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_batch_create");
  }
  // coarse-to-fine: `levels` ordered coarse to fine (see standardPyramid)
  NdtBatchHip(const std::vector<ndt2d_params>& levels, int device)
      : mode_(levels.empty() ? NDT_HESSIAN_GAUSS_NEWTON : levels.back().hessian_mode) {
    const int32_t st = ndt2d_batch_create_pyramid(levels.data(), static_cast<int32_t>(levels.size()), device, &b_);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_batch_create_pyramid");
  }
  // the library's 3-level schedule (4c, 2c, c) around `fine`
  static std::vector<ndt2d_params> standardPyramid(const ndt2d_params& fine = NdtMatcherHip::defaultParams()) {
    std::vector<ndt2d_params> lv(3);
    const int32_t st = ndt2d_default_pyramid(&fine, lv.data());
    if (st != NDT_OK) throw NdtError(st, "ndt2d_default_pyramid");
    return lv;
  }
  ~NdtBatchHip() { ndt2d_batch_destroy(b_); }
  // NDT_TUNE_BATCH_SMALL_VARIANT / NDT_TUNE_BATCH_GLOBAL_WORKGROUPS (memory of the global-table variant against its rate)
  void setTuning(int32_t knob, int64_t value) {
    const int32_t st = ndt2d_batch_set_tuning(b_, knob, value);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_batch_set_tuning");
  }
  NdtBatchHip(const NdtBatchHip&) = delete;
  NdtBatchHip& operator=(const NdtBatchHip&) = delete;

  std::vector<MatchResult> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                 const std::vector<Pose2>& guesses) {
    return detail::align_pairs(targets, sources, guesses, "ndt2d_batch_align", mode_,
                               [&](const float* tx, const float* ty, const uint64_t* toff, const float* sx, const float* sy,
                                   const uint64_t* soff, const double* init, size_t n, ndt2d_result* res) {
                                 return ndt2d_batch_align(b_, tx, ty, toff, sx, sy, soff, init, n, res);
                               });
  }

 private:
  ndt2d_batch* b_ = nullptr;
  int32_t mode_ = NDT_HESSIAN_GAUSS_NEWTON;
};

// The same over several GPUs owned by this process: pairs are split into contiguous
// work-balanced shards, one host thread and one batch context per device.
class NdtMultiHip {
 public:
  using Cloud = NdtBatchHip::Cloud;

  // devices empty = every visible device
  explicit NdtMultiHip(const ndt2d_params& params = NdtMatcherHip::defaultParams(), const std::vector<int32_t>& devices = {})
      : mode_(params.hessian_mode) {
    const int32_t st = ndt2d_multi_create(&params, devices.empty() ? nullptr : devices.data(),
                                          static_cast<int32_t>(devices.size()), &m_);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_multi_create");
  }
  NdtMultiHip(const std::vector<ndt2d_params>& levels, const std::vector<int32_t>& devices)
      : mode_(levels.empty() ? NDT_HESSIAN_GAUSS_NEWTON : levels.back().hessian_mode) {
    const int32_t st = ndt2d_multi_create_pyramid(levels.data(), static_cast<int32_t>(levels.size()),
                                                  devices.empty() ? nullptr : devices.data(),
                                                  static_cast<int32_t>(devices.size()), &m_);
    if (st != NDT_OK) throw NdtError(st, "ndt2d_multi_create_pyramid");
  }
  ~NdtMultiHip() { ndt2d_multi_destroy(m_); }
  NdtMultiHip(const NdtMultiHip&) = delete;
  NdtMultiHip& operator=(const NdtMultiHip&) = delete;

  int deviceCount() const { return ndt2d_multi_device_count(m_); }

  std::vector<MatchResult> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                 const std::vector<Pose2>& guesses) {
    return detail::align_pairs(targets, sources, guesses, "ndt2d_multi_align", mode_,
                               [&](const float* tx, const float* ty, const uint64_t* toff, const float* sx, const float* sy,
                                   const uint64_t* soff, const double* init, size_t n, ndt2d_result* res) {
                                 return ndt2d_multi_align(m_, tx, ty, toff, sx, sy, soff, init, n, res);
                               });
  }

  // Shards already resident on their devices (one DeviceShard per context, in context order; the
  // pointers are device pointers laid out as ndt2d_batch_align_dev takes them).  Every context aligns
  // its shard, the result rows are exchanged with one RCCL all-gather on the contexts' streams
  // (ndt2d_multi_align_dev), and the rows come back in global pair order.
  struct DeviceShard {
    const float* tx = nullptr; const float* ty = nullptr; const uint64_t* toff = nullptr;
    const float* sx = nullptr; const float* sy = nullptr; const uint64_t* soff = nullptr;
    const double* init = nullptr;
    size_t n_pairs = 0;
  };
  std::vector<MatchResult> alignDev(const std::vector<DeviceShard>& shards) {
    const size_t nd = shards.size();
    std::vector<const float*> tx(nd), ty(nd), sx(nd), sy(nd);
    std::vector<const uint64_t*> toff(nd), soff(nd);
    std::vector<const double*> init(nd);
    std::vector<size_t> n(nd);
    size_t total = 0;
    for (size_t d = 0; d < nd; ++d) {
      tx[d] = shards[d].tx; ty[d] = shards[d].ty; toff[d] = shards[d].toff; sx[d] = shards[d].sx; sy[d] = shards[d].sy;
      soff[d] = shards[d].soff; init[d] = shards[d].init; n[d] = shards[d].n_pairs;
      total += n[d];
    }
    if (static_cast<int>(nd) != deviceCount()) throw NdtError(NDT_ERR_INVALID_ARG, "NdtMultiHip::alignDev: one shard per device");
    std::vector<ndt2d_result> rows(total);
    const int32_t st = ndt2d_multi_align_dev(m_, tx.data(), ty.data(), toff.data(), sx.data(), sy.data(), soff.data(),
                                             init.data(), n.data(), nullptr, nullptr, rows.data());
    if (st < 0) throw NdtError(st, "ndt2d_multi_align_dev");
    std::vector<MatchResult> out;
    out.reserve(total);
    for (const ndt2d_result& r : rows) out.push_back(to_match_result(r, mode_));
    return out;
  }

 private:
  ndt2d_multi* m_ = nullptr;
  int32_t mode_ = NDT_HESSIAN_GAUSS_NEWTON;
};

// ---- 3D (SE(3), BASELINE config 5): the same shape over the ndt3d_* entry points ----------------
struct Pose3 {           // translation and roll/pitch/yaw of R = Rz(yaw) Ry(pitch) Rx(roll)
  double x = 0.0, y = 0.0, z = 0.0, roll = 0.0, pitch = 0.0, yaw = 0.0;
};

struct MatchResult3 {
  Pose3 pose;
  std::array<double, 36> information{};  // row-major 6x6 Gauss-Newton Hessian of -score (tx ty tz roll pitch yaw)
  std::array<double, 36> covariance{};   // its inverse (zero if singular)
  double score = 0.0;
  int iterations = 0, n_hit = 0, status = NDT_OK;
  bool converged() const { return status == NDT_OK; }
};

// symmetric positive definite 6x6 inverse by Gauss-Jordan with partial pivoting; false if singular
inline bool invert6(const double* H, double* C) {
  double a[6][12];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) { a[i][j] = H[6 * i + j]; a[i][6 + j] = i == j ? 1.0 : 0.0; }
  for (int c = 0; c < 6; ++c) {
    int p = c;
    for (int r = c + 1; r < 6; ++r) if (std::abs(a[r][c]) > std::abs(a[p][c])) p = r;
    if (!(std::abs(a[p][c]) > 0.0)) { for (int i = 0; i < 36; ++i) C[i] = 0.0; return false; }
    if (p != c) for (int j = 0; j < 12; ++j) std::swap(a[p][j], a[c][j]);
    const double inv = 1.0 / a[c][c];
    for (int j = 0; j < 12; ++j) a[c][j] *= inv;
    for (int r = 0; r < 6; ++r) {
      if (r == c) continue;
      const double f = a[r][c];
      if (f != 0.0) for (int j = 0; j < 12; ++j) a[r][j] -= f * a[c][j];
    }
  }
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) C[6 * i + j] = a[i][6 + j];
  return true;
}

// R = Rz(yaw) Ry(pitch) Rx(roll), row-major
inline std::array<double, 9> rotationOf(const Pose3& p) {
  const double ca = std::cos(p.roll), sa = std::sin(p.roll), cb = std::cos(p.pitch), sb = std::sin(p.pitch),
               cg = std::cos(p.yaw), sg = std::sin(p.yaw);
  return {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
          sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
          -sb, cb * sa, cb * ca};
}

// MatchResult3::covariance is for additive errors on (tx, ty, tz, roll, pitch, yaw).  A factor on SE(3) (e.g.
// gtsam::BetweenFactor<gtsam::Pose3>, whose tangent vector is (rotation; translation) in the measured pose's own
// frame) wants C_local = J C J' with, to first order, omega_body = E (d roll, d pitch, d yaw)',
// E = [[1, 0, -sin pitch], [0, cos roll, sin roll cos pitch], [0, -sin roll, cos roll cos pitch]], and rho = R' dt.
// Returned row-major 6x6 in the order (omega_x, omega_y, omega_z, rho_x, rho_y, rho_z).
inline std::array<double, 36> covarianceInLocalFrame3(const Pose3& pose, const std::array<double, 36>& cov) {
  const std::array<double, 9> R = rotationOf(pose);
  const double ca = std::cos(pose.roll), sa = std::sin(pose.roll), cb = std::cos(pose.pitch), sb = std::sin(pose.pitch);
  double J[36] = {0};
  const double E[9] = {1.0, 0.0, -sb, 0.0, ca, sa * cb, 0.0, -sa, ca * cb};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      J[6 * i + 3 + j] = E[3 * i + j];            // omega <- euler increments
      J[6 * (3 + i) + j] = R[3 * j + i];          // rho <- R' dt
    }
  double T[36];
  std::array<double, 36> out{};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      T[6 * i + j] = 0.0;
      for (int k = 0; k < 6; ++k) T[6 * i + j] += J[6 * i + k] * cov[6 * k + j];
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
      for (int k = 0; k < 6; ++k) out[6 * i + j] += T[6 * i + k] * J[6 * j + k];
  return out;
}

class NdtMatcherHip3 {
 public:
  static ndt3d_params defaultParams() { ndt3d_params p; ndt3d_default_params(&p); return p; }

  explicit NdtMatcherHip3(const ndt3d_params& params = defaultParams(), int device = 0) {
    const int32_t st = ndt3d_create(&params, device, &h_);
    if (st != NDT_OK) throw NdtError(st, "ndt3d_create");
  }
  ~NdtMatcherHip3() { ndt3d_destroy(h_); }
  NdtMatcherHip3(const NdtMatcherHip3&) = delete;
  NdtMatcherHip3& operator=(const NdtMatcherHip3&) = delete;

  void setTarget(const float* x, const float* y, const float* z, size_t n) { check(ndt3d_set_target(h_, x, y, z, n), "ndt3d_set_target"); }
  // execution-strategy knobs of a 3D handle (NDT_TUNE_SINGLE_SYNC_BUILD)
  void setTuning(int32_t knob, int64_t value) { check(ndt3d_set_tuning(h_, knob, value), "ndt3d_set_tuning"); }
  // 1: a point is scored against its own voxel; 7: and against the six face neighbours (ndt3d_set_neighbourhood).  The
  // alignments honour it; the searches, pose lists, particle scores and point fits throw while 7 is set.
  void setNeighbourhood(int32_t n) { check(ndt3d_set_neighbourhood(h_, n), "ndt3d_set_neighbourhood"); }
  int32_t neighbourhood() const { return ndt3d_neighbourhood(h_); }
  // incremental voxel-grid update: returns the number of points outside the cached extent
  size_t addTargetPoints(const float* x, const float* y, const float* z, size_t n) {
    size_t outside = 0;
    check(ndt3d_add_target_points(h_, x, y, z, n, &outside), "ndt3d_add_target_points");
    return outside;
  }
  // empty voxel grid over a chosen box (a submap that grows scan by scan)
  void reserveTarget(const std::array<double, 3>& lo, const std::array<double, 3>& hi) {
    check(ndt3d_reserve_target(h_, lo.data(), hi.data()), "ndt3d_reserve_target");
  }
  // submap persistence, as NdtMatcherHip::saveMap / loadMap
  std::vector<unsigned char> saveMap() const {
    std::vector<unsigned char> buf(ndt3d_map_size(h_));
    check(ndt3d_save_map(h_, buf.data(), buf.size(), nullptr), "ndt3d_save_map");
    return buf;
  }
  void loadMap(const std::vector<unsigned char>& buf) { check(ndt3d_load_map(h_, buf.data(), buf.size()), "ndt3d_load_map"); }
  // as NdtMatcherHip::coarsenInto, for voxel grids (ndt3d_coarsen_map)
  void coarsenInto(NdtMatcherHip3& dst) { check(ndt3d_coarsen_map(h_, dst.h_), "ndt3d_coarsen_map"); }
  // device points, optionally moved into the map frame by `pose` first (the pose an alignment returned);
  // producer_stream = the stream that wrote them (nullptr: complete)
  size_t addTargetPointsDev(const float* d_x, const float* d_y, const float* d_z, size_t n, const Pose3* pose = nullptr,
                            void* producer_stream = nullptr) {
    size_t outside = 0;
    double p[6] = {0, 0, 0, 0, 0, 0};
    if (pose) { p[0] = pose->x; p[1] = pose->y; p[2] = pose->z; p[3] = pose->roll; p[4] = pose->pitch; p[5] = pose->yaw; }
    check(ndt3d_add_target_points_dev(h_, d_x, d_y, d_z, n, pose ? p : nullptr, &outside, producer_stream), "ndt3d_add_target_points_dev");
    return outside;
  }
  // the exact inverse of addTargetPoints(Dev), as NdtMatcherHip::removeTargetPoints(Dev)
  size_t removeTargetPoints(const float* x, const float* y, const float* z, size_t n) {
    size_t outside = 0;
    check(ndt3d_remove_target_points(h_, x, y, z, n, &outside), "ndt3d_remove_target_points");
    return outside;
  }
  size_t removeTargetPointsDev(const float* d_x, const float* d_y, const float* d_z, size_t n, const Pose3* pose = nullptr,
                               void* producer_stream = nullptr) {
    size_t outside = 0;
    double p[6] = {0, 0, 0, 0, 0, 0};
    if (pose) { p[0] = pose->x; p[1] = pose->y; p[2] = pose->z; p[3] = pose->roll; p[4] = pose->pitch; p[5] = pose->yaw; }
    check(ndt3d_remove_target_points_dev(h_, d_x, d_y, d_z, n, pose ? p : nullptr, &outside, producer_stream), "ndt3d_remove_target_points_dev");
    return outside;
  }
  // per-point fit and selection against the voxel grid, as NdtMatcherHip::fitPointsDev / selectPointsDev
  ndt_point_fit fitPointsDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& at, float max_m,
                             float* d_m = nullptr, uint8_t* d_class = nullptr) {
    const double p[6] = {at.x, at.y, at.z, at.roll, at.pitch, at.yaw};
    ndt_point_fit f;
    check(ndt3d_fit_points_dev(h_, d_sx, d_sy, d_sz, n, p, max_m, d_m, d_class, &f), "ndt3d_fit_points_dev");
    return f;
  }
  ndt_point_fit selectPointsDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& at, float max_m,
                                uint32_t keep, float* d_ox, float* d_oy, float* d_oz, uint32_t* d_index = nullptr) {
    const double p[6] = {at.x, at.y, at.z, at.roll, at.pitch, at.yaw};
    ndt_point_fit f;
    check(ndt3d_select_points_dev(h_, d_sx, d_sy, d_sz, n, p, max_m, keep, d_ox, d_oy, d_oz, d_index, &f), "ndt3d_select_points_dev");
    return f;
  }
  // voxel-grid filter of a device cloud in order (iz, iy, ix) (ndt3d_voxel_filter_dev), as NdtMatcherHip::voxelFilterDev
  ndt_voxel_filter_info voxelFilterDev(const float* d_x, const float* d_y, const float* d_z, size_t n, double leaf, float* d_ox,
                                       float* d_oy, float* d_oz, size_t capacity, uint32_t min_points = 1,
                                       uint32_t* d_count = nullptr) {
    ndt_voxel_filter_info info;
    check(ndt3d_voxel_filter_dev(h_, d_x, d_y, d_z, n, leaf, min_points, d_ox, d_oy, d_oz, d_count, capacity, &info),
          "ndt3d_voxel_filter_dev");
    return info;
  }
  MatchResult3 alignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& guess = Pose3()) {
    const double init[6] = {guess.x, guess.y, guess.z, guess.roll, guess.pitch, guess.yaw};
    ndt3d_result r;
    check(ndt3d_align_dev(h_, d_sx, d_sy, d_sz, n, init, &r), "ndt3d_align_dev");
    return toMatchResult(r);
  }
  // up to 64 different device scans against the cached voxel grid in one launch chain; result k is bit for bit
  // what alignDev returns for scan k and guesses[k]
  struct DeviceScan3 { const float* x; const float* y; const float* z; size_t n; };
  std::vector<MatchResult3> alignMultiScanDev(const std::vector<DeviceScan3>& scans, const std::vector<Pose3>& guesses) {
    const size_t m = scans.size();
    if (m == 0 || guesses.size() != m) throw NdtError(NDT_ERR_INVALID_ARG, "ndt3d_align_multi_scan_dev");
    std::vector<const float*> px(m), py(m), pz(m);
    std::vector<size_t> ns(m);
    std::vector<double> init(6 * m);
    for (size_t k = 0; k < m; ++k) {
      px[k] = scans[k].x; py[k] = scans[k].y; pz[k] = scans[k].z; ns[k] = scans[k].n;
      const Pose3& g = guesses[k];
      const double p[6] = {g.x, g.y, g.z, g.roll, g.pitch, g.yaw};
      std::copy(p, p + 6, init.begin() + 6 * k);
    }
    std::vector<ndt3d_result> res(m);
    check(ndt3d_align_multi_scan_dev(h_, px.data(), py.data(), pz.data(), ns.data(), init.data(), static_cast<int32_t>(m), res.data()),
          "ndt3d_align_multi_scan_dev");
    std::vector<MatchResult3> out;
    out.reserve(m);
    for (const auto& r : res) out.push_back(toMatchResult(r));
    return out;
  }
  // one device scan from several initial poses (a lattice of hypotheses around a poor guess)
  std::vector<MatchResult3> alignMultiStartDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                               const std::vector<Pose3>& guesses) {
    std::vector<DeviceScan3> scans(guesses.size(), DeviceScan3{d_sx, d_sy, d_sz, n});
    return alignMultiScanDev(scans, guesses);
  }
  // Exhaustive pose search over an (x, y, yaw) window against the cached voxel grid (ndt3d_search_dev; lattice, peaks
  // and separation: ndt_hip.h), as NdtMatcherHip::searchDev: the best k (1..64) well-separated lattice poses, best
  // first; z, roll and pitch are the window centre's.  producer_stream: the stream that wrote the device arrays
  // (complete = true: they are known to be complete, no ordering needed).
  struct SearchHit {
    Pose3 pose;            // the lattice pose, yaw wrapped to (-pi, pi]
    float score = 0.f;     // the lattice score
    int32_t index = 0;     // flat lattice index
  };
  struct SearchMatch {
    SearchHit hit;
    MatchResult3 result;   // alignMultiStartDev's result from hit.pose (searchAlignMap: alignMap's)
  };
  std::vector<SearchHit> searchDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                   const ndt3d_search_window& window, int k, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt3d_search_dev(h_, d_sx, d_sy, d_sz, n, &window, (int32_t)k, hits.data(), &n_hits), "ndt3d_search_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(toSearchHit(hits[i]));
    return out;
  }
  // searchDev, then one alignment from every hit in one launch chain (ndt3d_search_align_dev): result i is bit for bit
  // what alignMultiStartDev returns from the hits' poses.  Search with a subsampled scan (voxelFilterDev, or every 8th
  // point) and refine with the full one when the lattice is large.
  std::vector<SearchMatch> searchAlignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                          const ndt3d_search_window& window, int k, void* producer_stream,
                                          bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt3d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt3d_search_align_dev(h_, d_sx, d_sy, d_sz, n, &window, (int32_t)k, hits.data(), r.data(), &n_hits),
          "ndt3d_search_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{toSearchHit(hits[i]), toMatchResult(r[i])});
    return out;
  }
  // The score at every pose of a list in one launch (ndt3d_score_poses_dev), as NdtMatcherHip::scorePosesDev: d_poses is
  // [m][6] = (tx, ty, tz, roll, pitch, yaw) in double, all six free - a search over z, roll or pitch is a list.
  void scorePosesDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                     float* d_scores, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    check(ndt3d_score_poses_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, d_scores), "ndt3d_score_poses_dev");
  }
  void* stream() { return ndt3d_stream(h_); }
  // The driver side of the 3D boundary, on the caller's stream (no handle involved; d_* are device pointers, elevations
  // a host array of n_elev angles): range image -> points (ndt3d_range_image_to_points_dev) and, with the sensor's
  // motion within the sweep, the same de-skewed (ndt3d_range_image_to_points_deskew_dev): azimuth column j was fired at
  // sweep fraction frac0 + j * frac_inc, the points come out in the sensor frame at ref_frac.
  static void rangeImageToPointsDev(const float* d_ranges, int n_elev, int n_azim, const double* elevations, double azimuth0,
                                    double azimuth_inc, double range_min, double range_max, float* d_x, float* d_y,
                                    float* d_z, void* stream) {
    check(ndt3d_range_image_to_points_dev(d_ranges, n_elev, n_azim, elevations, azimuth0, azimuth_inc, range_min, range_max,
                                          d_x, d_y, d_z, stream), "ndt3d_range_image_to_points_dev");
  }
  static void rangeImageToPointsDev(const float* d_ranges, int n_elev, int n_azim, const double* elevations, double azimuth0,
                                    double azimuth_inc, double range_min, double range_max, const Pose3& motion,
                                    double frac0, double frac_inc, double ref_frac, float* d_x, float* d_y, float* d_z,
                                    void* stream) {
    const double delta[6] = {motion.x, motion.y, motion.z, motion.roll, motion.pitch, motion.yaw};
    check(ndt3d_range_image_to_points_deskew_dev(d_ranges, n_elev, n_azim, elevations, azimuth0, azimuth_inc, range_min,
                                                 range_max, delta, frac0, frac_inc, ref_frac, d_x, d_y, d_z, stream),
          "ndt3d_range_image_to_points_deskew_dev");
  }
  // prev^-1 o cur, as NdtMatcherHip::sweepMotion
  static Pose3 sweepMotion(const Pose3& prev, const Pose3& cur) {
    const double p[6] = {prev.x, prev.y, prev.z, prev.roll, prev.pitch, prev.yaw};
    const double c[6] = {cur.x, cur.y, cur.z, cur.roll, cur.pitch, cur.yaw};
    double d[6];
    check(ndt3d_sweep_motion(p, c, d), "ndt3d_sweep_motion");
    Pose3 out;
    out.x = d[0]; out.y = d[1]; out.z = d[2]; out.roll = d[3]; out.pitch = d[4]; out.yaw = d[5];
    return out;
  }
  // Device points with a sweep fraction each -> the sensor frame at ref_frac (ndt3d_deskew_points_dev); the outputs may
  // be the inputs
  static void deskewPointsDev(const float* d_x, const float* d_y, const float* d_z, const float* d_frac, size_t n,
                              const Pose3& motion, double ref_frac, float* d_ox, float* d_oy, float* d_oz, void* stream) {
    const double delta[6] = {motion.x, motion.y, motion.z, motion.roll, motion.pitch, motion.yaw};
    check(ndt3d_deskew_points_dev(d_x, d_y, d_z, d_frac, n, delta, ref_frac, d_ox, d_oy, d_oz, stream),
          "ndt3d_deskew_points_dev");
  }
  // scorePosesDev for SHORT lists, a team of lanes per pose, with the hit counts (ndt3d_score_particles_dev), as
  // NdtMatcherHip::scoreParticlesDev; d_n_hit may be null
  void scoreParticlesDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                         float* d_scores, uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    check(ndt3d_score_particles_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, d_scores, d_n_hit), "ndt3d_score_particles_dev");
  }
  // the same, returning after the enqueue (ndt3d_score_particles_async): complete in stream order on stream() (ndt3d_stream)
  void scoreParticlesAsync(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                           float* d_scores, uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    check(ndt3d_score_particles_async(h_, d_sx, d_sy, d_sz, n, d_poses, m, d_scores, d_n_hit), "ndt3d_score_particles_async");
  }
  // the same with host arrays (ndt3d_score_particles); n_hit may be null
  void scoreParticles(const float* sx, const float* sy, const float* sz, size_t n, const double* poses, size_t m, float* scores,
                      uint32_t* n_hit) {
    check(ndt3d_score_particles(h_, sx, sy, sz, n, poses, m, scores, n_hit), "ndt3d_score_particles");
  }
  // the best k (1..64) well-separated poses of the list (ndt3d_best_poses_dev): translation distance over (x, y, z),
  // rotation distance the largest wrapped difference of roll, pitch and yaw
  std::vector<SearchHit> bestPosesDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses,
                                      size_t m, int k, double min_sep_trans, double min_sep_rot, void* producer_stream,
                                      bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt3d_best_poses_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), &n_hits),
          "ndt3d_best_poses_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(toSearchHit(hits[i]));
    return out;
  }
  // bestPosesDev, then one alignment from every hit in one launch chain (ndt3d_best_poses_align_dev)
  std::vector<SearchMatch> bestPosesAlignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                             const double* d_poses, size_t m, int k, double min_sep_trans, double min_sep_rot,
                                             void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt3d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt3d_best_poses_align_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(),
                                     r.data(), &n_hits), "ndt3d_best_poses_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{toSearchHit(hits[i]), toMatchResult(r[i])});
    return out;
  }
  static SearchHit toSearchHit(const ndt3d_search_hit& h) {
    SearchHit s;
    s.pose = {h.pose[0], h.pose[1], h.pose[2], h.pose[3], h.pose[4], h.pose[5]};
    s.score = h.score;
    s.index = h.index;
    return s;
  }
  ndt3d_grid_info gridInfo() const { ndt3d_grid_info g; check(ndt3d_get_grid_info(h_, &g), "ndt3d_get_grid_info"); return g; }

  MatchResult3 align(const float* sx, const float* sy, const float* sz, size_t n, const Pose3& guess = Pose3()) {
    const double init[6] = {guess.x, guess.y, guess.z, guess.roll, guess.pitch, guess.yaw};
    ndt3d_result r;
    check(ndt3d_align(h_, sx, sy, sz, n, init, &r), "ndt3d_align");
    return toMatchResult(r);
  }
  // Map-to-map alignment (ndt3d_align_map): source's cached voxel grid against this matcher's, no points; the pose maps
  // the source map's frame into this map's frame; this matcher's parameters drive the solve; source may be *this.
  // result.covariance is the plain inverse of the map-to-map Hessian: no calibration exists for this objective.
  // as NdtMatcherHip::mergeMap / unmergeMap, for voxel grids (ndt3d_merge_map, ndt3d_unmerge_map)
  size_t mergeMap(NdtMatcherHip3& source, const Pose3& pose) {
    size_t outside = 0;
    const double p[6] = {pose.x, pose.y, pose.z, pose.roll, pose.pitch, pose.yaw};
    check(ndt3d_merge_map(h_, source.h_, p, &outside), "ndt3d_merge_map");
    return outside;
  }
  size_t unmergeMap(NdtMatcherHip3& source, const Pose3& pose) {
    size_t outside = 0;
    const double p[6] = {pose.x, pose.y, pose.z, pose.roll, pose.pitch, pose.yaw};
    check(ndt3d_unmerge_map(h_, source.h_, p, &outside), "ndt3d_unmerge_map");
    return outside;
  }
  MatchResult3 alignMap(NdtMatcherHip3& source, const Pose3& guess = Pose3()) {
    const double init[6] = {guess.x, guess.y, guess.z, guess.roll, guess.pitch, guess.yaw};
    ndt3d_result r;
    check(ndt3d_align_map(h_, source.h_, init, &r), "ndt3d_align_map");
    return toMatchResult(r);
  }
  // Up to 64 map-to-map alignments against this matcher's voxel grid in one launch chain (ndt3d_align_map_multi): start
  // k aligns *sources[k] from guesses[k].  The same matcher in every entry is a multi-start; an entry may be this
  // matcher.  Result k is bit for bit what alignMap(*sources[k], guesses[k]) returns.
  std::vector<MatchResult3> alignMapMulti(const std::vector<NdtMatcherHip3*>& sources, const std::vector<Pose3>& guesses) {
    if (sources.size() != guesses.size()) throw NdtError(NDT_ERR_INVALID_ARG, "alignMapMulti: one guess per source");
    std::vector<ndt3d_handle*> hs;
    std::vector<double> init;
    for (size_t k = 0; k < sources.size(); ++k) {
      hs.push_back(sources[k] ? sources[k]->h_ : nullptr);
      init.insert(init.end(), {guesses[k].x, guesses[k].y, guesses[k].z, guesses[k].roll, guesses[k].pitch, guesses[k].yaw});
    }
    std::vector<ndt3d_result> r(hs.size());
    check(ndt3d_align_map_multi(h_, hs.data(), init.data(), (int32_t)hs.size(), r.data()), "ndt3d_align_map_multi");
    std::vector<MatchResult3> out;
    for (const ndt3d_result& x : r) out.push_back(toMatchResult(x));
    return out;
  }
  ndt3d_eval evaluateMap(NdtMatcherHip3& source, const Pose3& at) {
    const double p[6] = {at.x, at.y, at.z, at.roll, at.pitch, at.yaw};
    ndt3d_eval e;
    check(ndt3d_evaluate_map(h_, source.h_, p, &e), "ndt3d_evaluate_map");
    return e;
  }
  // The exhaustive search for this objective (ndt3d_search_map / ndt3d_search_align_map): the map-to-map score at every
  // pose of the window's (x, y, yaw) lattice, z, roll and pitch the window centre's, the best k well-separated peaks,
  // and one alignMap run from each - a loop closure between two 3D submaps whose guess is metres off and has no
  // heading.  Window, hits and k as in searchDev.
  std::vector<SearchHit> searchMap(NdtMatcherHip3& source, const ndt3d_search_window& window, int k) {
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt3d_search_map(h_, source.h_, &window, (int32_t)k, hits.data(), &n_hits), "ndt3d_search_map");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(toSearchHit(hits[i]));
    return out;
  }
  // the score volume [n_yaw][n_y][n_x] itself, into device memory (ndt3d_search_map_scores)
  void searchMapScores(NdtMatcherHip3& source, const ndt3d_search_window& window, float* d_scores) {
    check(ndt3d_search_map_scores(h_, source.h_, &window, d_scores), "ndt3d_search_map_scores");
  }
  // result i is bit for bit what alignMap returns from hit i's pose
  std::vector<SearchMatch> searchAlignMap(NdtMatcherHip3& source, const ndt3d_search_window& window, int k) {
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt3d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt3d_search_align_map(h_, source.h_, &window, (int32_t)k, hits.data(), r.data(), &n_hits), "ndt3d_search_align_map");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{toSearchHit(hits[i]), toMatchResult(r[i])});
    return out;
  }
  // evaluateMap's score at every pose of a list in one launch (ndt3d_score_map_poses_dev), as
  // NdtMatcherHip::scoreMapPosesDev: d_poses is [m][6] = (tx, ty, tz, roll, pitch, yaw) in double - z, roll and pitch are
  // free here, where searchMap pins them: two submaps of unknown relative height and tilt.
  void scoreMapPosesDev(NdtMatcherHip3& source, const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit,
                        void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    check(ndt3d_score_map_poses_dev(h_, source.h_, d_poses, m, d_scores, d_n_hit), "ndt3d_score_map_poses_dev");
  }
  // the best k (1..64) well-separated poses of the list, best first (ndt3d_best_map_poses_dev)
  std::vector<SearchHit> bestMapPosesDev(NdtMatcherHip3& source, const double* d_poses, size_t m, int k, double min_sep_trans,
                                         double min_sep_rot, void* producer_stream, bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    check(ndt3d_best_map_poses_dev(h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), &n_hits),
          "ndt3d_best_map_poses_dev");
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(toSearchHit(hits[i]));
    return out;
  }
  // bestMapPosesDev, then alignMap from every hit in one launch chain (ndt3d_best_map_poses_align_dev)
  std::vector<SearchMatch> bestMapPosesAlignDev(NdtMatcherHip3& source, const double* d_poses, size_t m, int k,
                                                double min_sep_trans, double min_sep_rot, void* producer_stream,
                                                bool complete = false) {
    if (!complete) check(ndt3d_wait_stream(h_, producer_stream), "ndt3d_wait_stream");
    std::vector<ndt3d_search_hit> hits(k > 0 ? (size_t)k : 1);
    std::vector<ndt3d_result> r(hits.size());
    int32_t n_hits = 0;
    check(ndt3d_best_map_poses_align_dev(h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, (int32_t)k, hits.data(), r.data(),
                                         &n_hits), "ndt3d_best_map_poses_align_dev");
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{toSearchHit(hits[i]), toMatchResult(r[i])});
    return out;
  }
  ndt3d_handle* raw() { return h_; }
  static MatchResult3 toMatchResult(const ndt3d_result& r) {
    MatchResult3 m;
    m.pose = {r.pose[0], r.pose[1], r.pose[2], r.pose[3], r.pose[4], r.pose[5]};
    for (int i = 0; i < 36; ++i) m.information[i] = r.H[i];
    invert6(r.H, m.covariance.data());
    m.score = r.score; m.iterations = r.iterations; m.n_hit = r.n_hit; m.status = r.status;
    return m;
  }

 private:
  static void check(int32_t st, const char* where) { if (st < 0) throw NdtError(st, where); }
  ndt3d_handle* h_ = nullptr;
};

// 3D loop-closure candidates: many independent 3D pairs in one call (ndt3d_batch_*; the pair's voxel grid
// lives in LDS for its whole alignment).  `levels` coarse to fine for a pyramid, one entry otherwise.
class NdtBatchHip3 {
 public:
  struct Cloud { const float* x; const float* y; const float* z; size_t n; };

  explicit NdtBatchHip3(const ndt3d_params& params = NdtMatcherHip3::defaultParams(), int device = 0) {
    const int32_t st = ndt3d_batch_create(&params, device, &b_);
    if (st != NDT_OK) throw NdtError(st, "ndt3d_batch_create");
  }
  NdtBatchHip3(const std::vector<ndt3d_params>& levels, int device) {
    const int32_t st = ndt3d_batch_create_pyramid(levels.data(), static_cast<int32_t>(levels.size()), device, &b_);
    if (st != NDT_OK) throw NdtError(st, "ndt3d_batch_create_pyramid");
  }
  ~NdtBatchHip3() { ndt3d_batch_destroy(b_); }
  // NDT_TUNE_BATCH_GLOBAL_WORKGROUPS: 1..256 table slabs of 7.9 MB for the pairs whose voxel grid does not fit on chip
  void setTuning(int32_t knob, int64_t value) {
    const int32_t st = ndt3d_batch_set_tuning(b_, knob, value);
    if (st != NDT_OK) throw NdtError(st, "ndt3d_batch_set_tuning");
  }
  NdtBatchHip3(const NdtBatchHip3&) = delete;
  NdtBatchHip3& operator=(const NdtBatchHip3&) = delete;

  std::vector<MatchResult3> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                  const std::vector<Pose3>& guesses) {
    const size_t n = targets.size();
    if (sources.size() != n || guesses.size() != n || n == 0) throw NdtError(NDT_ERR_INVALID_ARG, "ndt3d_batch_align");
    std::vector<uint64_t> toff(n + 1, 0), soff(n + 1, 0);
    for (size_t k = 0; k < n; ++k) { toff[k + 1] = toff[k] + targets[k].n; soff[k + 1] = soff[k] + sources[k].n; }
    std::vector<float> t[3], s[3];
    for (int c = 0; c < 3; ++c) { t[c].resize(toff[n]); s[c].resize(soff[n]); }
    std::vector<double> init(6 * n);
    for (size_t k = 0; k < n; ++k) {
      const float* tc[3] = {targets[k].x, targets[k].y, targets[k].z};
      const float* sc[3] = {sources[k].x, sources[k].y, sources[k].z};
      for (int c = 0; c < 3; ++c) {
        std::copy(tc[c], tc[c] + targets[k].n, t[c].begin() + toff[k]);
        std::copy(sc[c], sc[c] + sources[k].n, s[c].begin() + soff[k]);
      }
      const Pose3& g = guesses[k];
      const double p[6] = {g.x, g.y, g.z, g.roll, g.pitch, g.yaw};
      std::copy(p, p + 6, init.begin() + 6 * k);
    }
    std::vector<ndt3d_result> res(n);
    const int32_t st = ndt3d_batch_align(b_, t[0].data(), t[1].data(), t[2].data(), toff.data(), s[0].data(), s[1].data(),
                                         s[2].data(), soff.data(), init.data(), n, res.data());
    if (st < 0) throw NdtError(st, "ndt3d_batch_align");
    std::vector<MatchResult3> out;
    out.reserve(n);
    for (const auto& r : res) out.push_back(NdtMatcherHip3::toMatchResult(r));
    return out;
  }
  // device arrays laid out as ndt3d_batch_align_dev takes them; asynchronous on `stream` (nullptr: the context's own)
  void alignDev(const float* d_tx, const float* d_ty, const float* d_tz, const uint64_t* d_toff, const float* d_sx,
                const float* d_sy, const float* d_sz, const uint64_t* d_soff, const double* d_init, size_t n_pairs,
                ndt3d_result* d_results, void* stream = nullptr) {
    const int32_t st = ndt3d_batch_align_dev(b_, d_tx, d_ty, d_tz, d_toff, d_sx, d_sy, d_sz, d_soff, d_init, n_pairs, d_results, stream);
    if (st < 0) throw NdtError(st, "ndt3d_batch_align_dev");
  }
  void* stream() { return ndt3d_batch_stream(b_); }

 private:
  ndt3d_batch* b_ = nullptr;
};

// The 3D candidates over several GPUs owned by this process (ndt3d_multi_*): host pairs split into contiguous
// work-balanced shards, one context and one host thread per device.
class NdtMultiHip3 {
 public:
  explicit NdtMultiHip3(const ndt3d_params& params = NdtMatcherHip3::defaultParams(), const std::vector<int32_t>& devices = {}) {
    const int32_t st = ndt3d_multi_create(&params, devices.empty() ? nullptr : devices.data(), static_cast<int32_t>(devices.size()), &m_);
    if (st != NDT_OK) throw NdtError(st, "ndt3d_multi_create");
  }
  ~NdtMultiHip3() { ndt3d_multi_destroy(m_); }
  NdtMultiHip3(const NdtMultiHip3&) = delete;
  NdtMultiHip3& operator=(const NdtMultiHip3&) = delete;
  int deviceCount() const { return ndt3d_multi_device_count(m_); }
  ndt3d_multi* raw() { return m_; }     // ndt3d_multi_align / ndt3d_multi_align_dev (RCCL gather) take it

 private:
  ndt3d_multi* m_ = nullptr;
};

}  // namespace ndt
#endif  // NDT_MATCHER_HIP_HPP_

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
//
// The 2D and the 3D classes share their text: what differs between ndt2d_* and ndt3d_* is stated once per dimension in
// detail::Dim<2> / Dim<3>, and every member that takes no coordinate arrays exists once, in detail::MatcherCore,
// BatchCore and MultiCore.  Members of a class template are type-checked only where they are instantiated:
// tests/cpp/adapter_calls_main.cpp instantiates and calls every one of them (tests/test_adapter_calls.py pins what they
// pass to the library and return), so a member added here gets its section there.
#ifndef NDT_MATCHER_HIP_HPP_
#define NDT_MATCHER_HIP_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
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

namespace detail {
inline void check(int32_t st, const char* where) { if (st < 0) throw NdtError(st, where); }
inline void require_ok(int32_t st, const char* where) { if (st != NDT_OK) throw NdtError(st, where); }

// an entry point together with the name NdtError reports for it
template <class F>
struct Entry { F fn; const char* name; };
template <class F, class... A>
void call(const Entry<F>& e, A&&... a) { check(e.fn(std::forward<A>(a)...), e.name); }

// the entry points whose signatures differ between the dimensions only in the types below, as Dim<D>::name
#define NDT_ENTRY(D, name) static constexpr Entry<decltype(&ndt##D##d_##name)> name{&ndt##D##d_##name, "ndt" #D "d_" #name};
#define NDT_ENTRIES(D)                                                                                                      \
  NDT_ENTRY(D, default_params) NDT_ENTRY(D, create) NDT_ENTRY(D, destroy) NDT_ENTRY(D, stream) NDT_ENTRY(D, wait_stream)        \
  NDT_ENTRY(D, get_grid_info) NDT_ENTRY(D, map_size) NDT_ENTRY(D, save_map) NDT_ENTRY(D, load_map) NDT_ENTRY(D, coarsen_map)    \
  NDT_ENTRY(D, merge_map) NDT_ENTRY(D, unmerge_map) NDT_ENTRY(D, align_map) NDT_ENTRY(D, align_map_multi)                       \
  NDT_ENTRY(D, evaluate_map) NDT_ENTRY(D, search_map) NDT_ENTRY(D, search_map_scores) NDT_ENTRY(D, search_align_map)            \
  NDT_ENTRY(D, score_map_poses_dev) NDT_ENTRY(D, best_map_poses_dev) NDT_ENTRY(D, best_map_poses_align_dev)                     \
  NDT_ENTRY(D, sweep_motion) NDT_ENTRY(D, batch_create) NDT_ENTRY(D, batch_create_pyramid) NDT_ENTRY(D, batch_destroy)          \
  NDT_ENTRY(D, batch_set_tuning) NDT_ENTRY(D, multi_create) NDT_ENTRY(D, multi_destroy) NDT_ENTRY(D, multi_device_count)

template <int D>
struct Dim;
template <>
struct Dim<2> {
  using Handle = ndt2d_handle; using Batch = ndt2d_batch; using Multi = ndt2d_multi; using Params = ndt2d_params;
  using Result = ndt2d_result; using Eval = ndt2d_eval; using GridInfo = ndt2d_grid_info;
  using Window = ndt2d_search_window; using Hit = ndt2d_search_hit;
  using Pose = Pose2; using Match = MatchResult;
  static constexpr int kPose = 3;        // doubles per pose
  static std::array<double, 3> pack(const Pose2& p) { return {p.x, p.y, p.theta}; }
  static Pose2 unpack(const double* v) { Pose2 p; p.x = v[0]; p.y = v[1]; p.theta = v[2]; return p; }
  NDT_ENTRIES(2)
  NDT_ENTRY(2, multi_create_pyramid)     // (the 3D library has none)
};
template <>
struct Dim<3> {
  using Handle = ndt3d_handle; using Batch = ndt3d_batch; using Multi = ndt3d_multi; using Params = ndt3d_params;
  using Result = ndt3d_result; using Eval = ndt3d_eval; using GridInfo = ndt3d_grid_info;
  using Window = ndt3d_search_window; using Hit = ndt3d_search_hit;
  using Pose = Pose3; using Match = MatchResult3;
  static constexpr int kPose = 6;
  static std::array<double, 6> pack(const Pose3& p) { return {p.x, p.y, p.z, p.roll, p.pitch, p.yaw}; }
  static Pose3 unpack(const double* v) {
    Pose3 p;
    p.x = v[0]; p.y = v[1]; p.z = v[2]; p.roll = v[3]; p.pitch = v[4]; p.yaw = v[5];
    return p;
  }
  NDT_ENTRIES(3)
};
#undef NDT_ENTRIES
#undef NDT_ENTRY

// the poses of a list back to back, as the C calls take m of them
template <int D>
std::vector<double> pack_all(const std::vector<typename Dim<D>::Pose>& poses) {
  std::vector<double> out;
  for (const auto& g : poses) { const auto p = Dim<D>::pack(g); out.insert(out.end(), p.begin(), p.end()); }
  return out;
}

// a result row without its covariance, which the dimensions derive differently (to_match_result, NdtMatcherHip3::toMatchResult)
template <int D>
typename Dim<D>::Match result_row(const typename Dim<D>::Result& r) {
  typename Dim<D>::Match m;
  m.pose = Dim<D>::unpack(r.pose);
  std::copy(r.H, r.H + Dim<D>::kPose * Dim<D>::kPose, m.information.begin());
  m.score = r.score; m.iterations = r.iterations; m.n_hit = r.n_hit; m.status = r.status;
  return m;
}
}  // namespace detail

inline MatchResult to_match_result(const ndt2d_result& r, int32_t hessian_mode = NDT_HESSIAN_GAUSS_NEWTON) {
  MatchResult m = detail::result_row<2>(r);
  (void)ndt2d_calibrated_covariance(r.H, hessian_mode, m.covariance.data());
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

namespace detail {
// What NdtMatcherHip (D = 2) and NdtMatcherHip3 (D = 3) share: the handle's life, and every member that takes no
// coordinate arrays.  Derived is the matcher itself, so that `source` parameters and lists of sources have its type; it
// supplies result(row), the conversion of a result row (2D: calibrated by its Hessian mode; 3D: the plain inverse).
template <int D, class Derived>
class MatcherCore {
 protected:
  using Dm = Dim<D>;
  using Pose = typename Dm::Pose;
  using Match = typename Dm::Match;

 public:
  static typename Dm::Params defaultParams() { typename Dm::Params p; Dm::default_params.fn(&p); return p; }

  MatcherCore(const MatcherCore&) = delete;
  MatcherCore& operator=(const MatcherCore&) = delete;

  typename Dm::GridInfo gridInfo() const { typename Dm::GridInfo g; call(Dm::get_grid_info, h_, &g); return g; }
  // submap persistence: the cached grid as a flat buffer (ndt_map_header + exact per-cell sums), and back - bit for
  // bit the same grid when the loading matcher has the saving one's parameters; it goes on taking points
  std::vector<unsigned char> saveMap() const {
    std::vector<unsigned char> buf(Dm::map_size.fn(h_));
    call(Dm::save_map, h_, buf.data(), buf.size(), nullptr);
    return buf;
  }
  void loadMap(const std::vector<unsigned char>& buf) { call(Dm::load_map, h_, buf.data(), buf.size()); }
  // dst (cell_size exactly 2 or 4 times this matcher's) receives the grid whose cells are unions of this grid's, from the
  // exact per-cell sums alone (ndt2d_coarsen_map, ndt3d_coarsen_map): a pyramid level for a submap that holds no points
  void coarsenInto(Derived& dst) { call(Dm::coarsen_map, h_, dst.h_); }

  // The best k (1..64) well-separated poses of a search or of a list, best first.
  struct SearchHit {
    Pose pose;             // the lattice pose (the list's pose as it stands there), theta / yaw wrapped to (-pi, pi]
    float score = 0.f;     // the lattice score
    int32_t index = 0;     // flat lattice index (position in the list)
  };
  struct SearchMatch {
    SearchHit hit;
    Match result;          // alignMultiStartDev's result from hit.pose (the map searches: alignMap's)
  };
  static SearchHit toSearchHit(const typename Dm::Hit& h) {
    SearchHit s;
    s.pose = Dm::unpack(h.pose);
    s.score = h.score;
    s.index = h.index;
    return s;
  }
  // the handle's stream (hipStream_t as void*): what scoreParticlesAsync's outputs are ordered on
  void* stream() { return Dm::stream.fn(h_); }
  // prev^-1 o cur: the motion between the last two estimates, the constant-velocity guess of the next sweep's motion
  static Pose sweepMotion(const Pose& prev, const Pose& cur) {
    double d[Dm::kPose];
    call(Dm::sweep_motion, Dm::pack(prev).data(), Dm::pack(cur).data(), d);
    return Dm::unpack(d);
  }

  // Folds `source`'s submap into this matcher's at `pose` (source's frame in this one's: what alignMap(source) returns), from
  // source's exact per-cell sums alone (ndt2d_merge_map, ndt3d_merge_map: no points, so a map that came back from loadMap
  // merges too); source's cell_size is at most this one's.  Returns the points that fell outside this grid.  unmergeMap
  // with the same arguments takes exactly that out again, whatever was added or removed in between.
  size_t mergeMap(Derived& source, const Pose& pose) {
    size_t outside = 0;
    call(Dm::merge_map, h_, source.h_, Dm::pack(pose).data(), &outside);
    return outside;
  }
  size_t unmergeMap(Derived& source, const Pose& pose) {
    size_t outside = 0;
    call(Dm::unmerge_map, h_, source.h_, Dm::pack(pose).data(), &outside);
    return outside;
  }
  // Map-to-map alignment (ndt2d_align_map, ndt3d_align_map): `source`'s cached grid against this matcher's, no points
  // involved - the loop closure between two submaps, or between a reloaded map and the current one.  guess and the result
  // map the source map's frame into this map's frame; this matcher's parameters drive the solve; source may be *this.
  // The 2D result's covariance carries the point-to-map calibration factors, which are NOT calibrated for this
  // objective: build a noise model from result.information with factors of your own.  The 3D one is the plain inverse
  // of the map-to-map Hessian: no calibration exists for this objective.
  Match alignMap(Derived& source, const Pose& guess = Pose()) {
    typename Dm::Result r;
    call(Dm::align_map, h_, source.h_, Dm::pack(guess).data(), &r);
    return self().result(r);
  }
  // Up to 64 map-to-map alignments against this matcher's grid in one launch chain (ndt2d_align_map_multi,
  // ndt3d_align_map_multi): start k aligns *sources[k] from guesses[k].  The same matcher in every entry is a
  // multi-start; an entry may be this matcher.  Result k is bit for bit what alignMap(*sources[k], guesses[k]) returns.
  std::vector<Match> alignMapMulti(const std::vector<Derived*>& sources, const std::vector<Pose>& guesses) {
    if (sources.size() != guesses.size()) throw NdtError(NDT_ERR_INVALID_ARG, "alignMapMulti: one guess per source");
    std::vector<typename Dm::Handle*> hs;
    for (Derived* s : sources) hs.push_back(s ? s->h_ : nullptr);
    const std::vector<double> init = pack_all<D>(guesses);
    std::vector<typename Dm::Result> r(hs.size());
    call(Dm::align_map_multi, h_, hs.data(), init.data(), (int32_t)hs.size(), r.data());
    return results(r);
  }
  typename Dm::Eval evaluateMap(Derived& source, const Pose& at) {
    typename Dm::Eval e;
    call(Dm::evaluate_map, h_, source.h_, Dm::pack(at).data(), &e);
    return e;
  }
  // The exhaustive search for this objective (ndt2d_search_map / ndt2d_search_align_map and their ndt3d twins): the
  // map-to-map score at every pose of the window's lattice - (x, y, theta); in 3D (x, y, yaw), with z, roll and pitch the
  // window centre's - the best k well-separated peaks, and one alignMap run from each: a submap-to-submap loop closure
  // whose guess is metres off and has no heading.  Window, hits and k as in searchDev.
  std::vector<SearchHit> searchMap(Derived& source, const typename Dm::Window& window, int k) {
    return hits(k, [&](int32_t kk, typename Dm::Hit* h, int32_t* n) { call(Dm::search_map, h_, source.h_, &window, kk, h, n); });
  }
  // the score volume [n_theta][n_y][n_x] itself, into device memory (ndt2d_search_map_scores, ndt3d_search_map_scores)
  void searchMapScores(Derived& source, const typename Dm::Window& window, float* d_scores) {
    call(Dm::search_map_scores, h_, source.h_, &window, d_scores);
  }
  // result i is bit for bit what alignMap returns from hit i's pose
  std::vector<SearchMatch> searchAlignMap(Derived& source, const typename Dm::Window& window, int k) {
    return matches(k, [&](int32_t kk, typename Dm::Hit* h, typename Dm::Result* r, int32_t* n) {
      call(Dm::search_align_map, h_, source.h_, &window, kk, h, r, n);
    });
  }
  // evaluateMap's score at every pose of a list in one launch (ndt2d_score_map_poses_dev, ndt3d_score_map_poses_dev;
  // contract: ndt_hip.h): d_poses is [m][3] = (x, y, theta) or [m][6] = (tx, ty, tz, roll, pitch, yaw) in double, d_scores
  // [m] floats, d_n_hit [m] counts of components that fell in a valid cell (may be null), all device memory - the particles
  // of a submap-level filter, samples round a place-recognition hypothesis; in 3D z, roll and pitch are free here, where
  // searchMap pins them.  A non-finite pose scores 0.  producer_stream: the stream that wrote the list.
  void scoreMapPosesDev(Derived& source, const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit,
                        void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    call(Dm::score_map_poses_dev, h_, source.h_, d_poses, m, d_scores, d_n_hit);
  }
  // the best k (1..64) well-separated poses of the list, best first (ndt2d_best_map_poses_dev, ndt3d_best_map_poses_dev):
  // hit.index is the position in the list, hit.pose the list's pose as it stands there
  std::vector<SearchHit> bestMapPosesDev(Derived& source, const double* d_poses, size_t m, int k, double min_sep_trans,
                                         double min_sep_rot, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    return hits(k, [&](int32_t kk, typename Dm::Hit* h, int32_t* n) {
      call(Dm::best_map_poses_dev, h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, kk, h, n);
    });
  }
  // bestMapPosesDev, then alignMap from every hit in one launch chain (ndt2d_best_map_poses_align_dev and its ndt3d
  // twin): result i is bit for bit what alignMap returns from hit i's pose
  std::vector<SearchMatch> bestMapPosesAlignDev(Derived& source, const double* d_poses, size_t m, int k,
                                                double min_sep_trans, double min_sep_rot, void* producer_stream,
                                                bool complete = false) {
    wait(producer_stream, complete);
    return matches(k, [&](int32_t kk, typename Dm::Hit* h, typename Dm::Result* r, int32_t* n) {
      call(Dm::best_map_poses_align_dev, h_, source.h_, d_poses, m, min_sep_trans, min_sep_rot, kk, h, r, n);
    });
  }
  typename Dm::Handle* raw() { return h_; }

 protected:
  MatcherCore(const typename Dm::Params& params, int device) { require_ok(Dm::create.fn(&params, device, &h_), Dm::create.name); }
  ~MatcherCore() { Dm::destroy.fn(h_); }

  static void check(int32_t st, const char* where) { detail::check(st, where); }
  // orders the handle's stream behind the producer of device arrays, unless they are known to be complete
  void wait(void* producer_stream, bool complete) { if (!complete) call(Dm::wait_stream, h_, producer_stream); }
  // run(k, hits, n_hits) fills a buffer of k hits (one when k is not positive: the library refuses such a k itself)
  template <class Run>
  std::vector<SearchHit> hits(int k, Run&& run) {
    std::vector<typename Dm::Hit> h(k > 0 ? (size_t)k : 1);
    int32_t n_hits = 0;
    run((int32_t)k, h.data(), &n_hits);
    std::vector<SearchHit> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(toSearchHit(h[i]));
    return out;
  }
  // the same with a result row per hit: run(k, hits, results, n_hits)
  template <class Run>
  std::vector<SearchMatch> matches(int k, Run&& run) {
    std::vector<typename Dm::Hit> h(k > 0 ? (size_t)k : 1);
    std::vector<typename Dm::Result> r(h.size());
    int32_t n_hits = 0;
    run((int32_t)k, h.data(), r.data(), &n_hits);
    std::vector<SearchMatch> out;
    for (int32_t i = 0; i < n_hits; ++i) out.push_back(SearchMatch{toSearchHit(h[i]), self().result(r[i])});
    return out;
  }
  std::vector<Match> results(const std::vector<typename Dm::Result>& rows) {
    std::vector<Match> out;
    out.reserve(rows.size());
    for (const auto& r : rows) out.push_back(self().result(r));
    return out;
  }
  const Derived& self() const { return static_cast<const Derived&>(*this); }

  typename Dm::Handle* h_ = nullptr;
};
}  // namespace detail

// One matcher = one device stream + one cached target grid.  Not thread-safe; use one
// instance per thread (distinct instances are independent).  The members that take no scan - the map's life, map-to-map
// alignment and search, sweepMotion, stream, raw - are detail::MatcherCore's.
class NdtMatcherHip : public detail::MatcherCore<2, NdtMatcherHip> {
 public:
  explicit NdtMatcherHip(const ndt2d_params& params = defaultParams(), int device = 0)
      : MatcherCore(params, device), mode_(params.hessian_mode) {}

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
    const auto p = Dm::pack(pose ? *pose : Pose2());
    check(ndt2d_add_target_points_dev(h_, d_x, d_y, n, pose ? p.data() : nullptr, &outside, producer_stream),
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
    const auto p = Dm::pack(pose ? *pose : Pose2());
    check(ndt2d_remove_target_points_dev(h_, d_x, d_y, n, pose ? p.data() : nullptr, &outside, producer_stream),
          "ndt2d_remove_target_points_dev");
    return outside;
  }

  // (ii)+(iii)+solve: full alignment from an initial guess
  MatchResult align(const float* sx, const float* sy, size_t n, const Pose2& guess = Pose2()) {
    ndt2d_result r;
    check(ndt2d_align(h_, sx, sy, n, Dm::pack(guess).data(), &r), "ndt2d_align");
    return result(r);
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
    wait(producer_stream, complete);
    ndt2d_result r;
    check(ndt2d_align_dev(h_, d_sx, d_sy, n, Dm::pack(guess).data(), &r), "ndt2d_align_dev");
    return result(r);
  }
  // Several starts around a poor guess in one launch chain (ndt2d_align_multi_start_dev, at most 64):
  // result k is what alignDev(guesses[k]) returns; pick e.g. the best score among the converged ones.
  std::vector<MatchResult> alignMultiStartDev(const float* d_sx, const float* d_sy, size_t n, const std::vector<Pose2>& guesses,
                                              void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    const std::vector<double> init = detail::pack_all<2>(guesses);
    std::vector<ndt2d_result> r(guesses.size());
    check(ndt2d_align_multi_start_dev(h_, d_sx, d_sy, n, init.data(), (int32_t)guesses.size(), r.data()),
          "ndt2d_align_multi_start_dev");
    return results(r);
  }
  // Several different device scans against the cached grid in one launch chain (ndt2d_align_multi_scan_dev,
  // at most 64): scans[k] = {d_x, d_y, n}; result k is what alignDev(scans[k], guesses[k]) returns.
  struct DeviceScan { const float* x; const float* y; size_t n; };
  std::vector<MatchResult> alignMultiScanDev(const std::vector<DeviceScan>& scans, const std::vector<Pose2>& guesses,
                                             void* producer_stream, bool complete = false) {
    if (scans.size() != guesses.size() || scans.empty()) throw NdtError(NDT_ERR_INVALID_ARG, "alignMultiScanDev");
    wait(producer_stream, complete);
    const size_t m = scans.size();
    std::vector<const float*> px(m), py(m);
    std::vector<size_t> n(m);
    for (size_t k = 0; k < m; ++k) { px[k] = scans[k].x; py[k] = scans[k].y; n[k] = scans[k].n; }
    const std::vector<double> init = detail::pack_all<2>(guesses);
    std::vector<ndt2d_result> r(m);
    check(ndt2d_align_multi_scan_dev(h_, px.data(), py.data(), n.data(), init.data(), (int32_t)m, r.data()),
          "ndt2d_align_multi_scan_dev");
    return results(r);
  }
  // Exhaustive pose search over an (x, y, theta) window against the cached grid (ndt2d_search_dev; lattice, peaks and
  // separation: ndt_hip.h): the best k (1..64) well-separated lattice poses, best first.  For a loop-closure candidate
  // or a relocalisation whose guess is metres and tens of degrees off, where alignDev's basin (about one cell) is too
  // narrow.  producer_stream as in alignMultiStartDev.
  std::vector<SearchHit> searchDev(const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window& window, int k,
                                   void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    return hits(k, [&](int32_t kk, ndt2d_search_hit* h, int32_t* n_hits) {
      check(ndt2d_search_dev(h_, d_sx, d_sy, n, &window, kk, h, n_hits), "ndt2d_search_dev");
    });
  }
  // searchDev, then one alignment from every hit in one launch chain (ndt2d_search_align_dev): result i is bit for bit
  // what alignMultiStartDev returns from the hits' poses.  The best match is usually the converged result of highest
  // score.
  std::vector<SearchMatch> searchAlignDev(const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window& window,
                                          int k, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    return matches(k, [&](int32_t kk, ndt2d_search_hit* h, ndt2d_result* r, int32_t* n_hits) {
      check(ndt2d_search_align_dev(h_, d_sx, d_sy, n, &window, kk, h, r, n_hits), "ndt2d_search_align_dev");
    });
  }
  // The score at every pose of a list in one launch (ndt2d_score_poses_dev; contract: ndt_hip.h): d_poses is [m][3] =
  // (x, y, theta) in double, d_scores [m] floats, both device memory - the weights of a particle filter's particles.  A
  // non-finite pose scores 0.  producer_stream: the stream that wrote the scan and the list.
  void scorePosesDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                     void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    check(ndt2d_score_poses_dev(h_, d_sx, d_sy, n, d_poses, m, d_scores), "ndt2d_score_poses_dev");
  }
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
    check(ndt2d_polar_to_points_deskew_dev(d_ranges, n, angle_min, angle_inc, range_min, range_max, Dm::pack(motion).data(),
                                           frac0, frac_inc, ref_frac, d_x, d_y, stream), "ndt2d_polar_to_points_deskew_dev");
  }
  // Device points with a sweep fraction each -> the sensor frame at ref_frac (ndt2d_deskew_points_dev); the outputs may
  // be the inputs
  static void deskewPointsDev(const float* d_x, const float* d_y, const float* d_frac, size_t n, const Pose2& motion,
                              double ref_frac, float* d_ox, float* d_oy, void* stream) {
    check(ndt2d_deskew_points_dev(d_x, d_y, d_frac, n, Dm::pack(motion).data(), ref_frac, d_ox, d_oy, stream),
          "ndt2d_deskew_points_dev");
  }
  // scorePosesDev for SHORT lists (a particle filter's particles; the faster call at every size measured): a team of lanes per pose
  // (ndt2d_score_particles_dev; contract: ndt_hip.h).  d_n_hit [m] (may be null): the lookups that hit a valid cell,
  // evaluate's n_hit at that pose.  The scores differ from scorePosesDev's only by the order of the float32 sum.
  void scoreParticlesDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                         uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    check(ndt2d_score_particles_dev(h_, d_sx, d_sy, n, d_poses, m, d_scores, d_n_hit), "ndt2d_score_particles_dev");
  }
  // the same, returning after the enqueue (ndt2d_score_particles_async): the outputs are complete in stream order on
  // stream() (ndt2d_stream); the scan, the list and the outputs stay alive until then
  void scoreParticlesAsync(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m, float* d_scores,
                           uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
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
    wait(producer_stream, complete);
    return hits(k, [&](int32_t kk, ndt2d_search_hit* h, int32_t* n_hits) {
      check(ndt2d_best_poses_dev(h_, d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, kk, h, n_hits), "ndt2d_best_poses_dev");
    });
  }
  // bestPosesDev, then one alignment from every hit in one launch chain (ndt2d_best_poses_align_dev)
  std::vector<SearchMatch> bestPosesAlignDev(const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                             int k, double min_sep_trans, double min_sep_rot, void* producer_stream,
                                             bool complete = false) {
    wait(producer_stream, complete);
    return matches(k, [&](int32_t kk, ndt2d_search_hit* h, ndt2d_result* r, int32_t* n_hits) {
      check(ndt2d_best_poses_align_dev(h_, d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, kk, h, r, n_hits),
            "ndt2d_best_poses_align_dev");
    });
  }
  static SearchHit to_search_hit(const ndt2d_search_hit& h) { return toSearchHit(h); }
  // one evaluation at a fixed pose, for callers with their own optimiser
  ndt2d_eval evaluate(const float* sx, const float* sy, size_t n, const Pose2& at) {
    ndt2d_eval e;
    check(ndt2d_evaluate(h_, sx, sy, n, Dm::pack(at).data(), &e), "ndt2d_evaluate");
    return e;
  }
  // Per-point fit of a device scan at a pose (ndt2d_fit_points_dev): m = q' Sigma^-1 q of every point in its cell into
  // d_m and its class byte (NDT_POINT_*) into d_class - either may be null - and the class counts, which count points.
  // The scan must be complete on the device, or the handle ordered behind its producer (ndt2d_wait_stream), as for
  // ndt2d_evaluate_dev.
  ndt_point_fit fitPointsDev(const float* d_sx, const float* d_sy, size_t n, const Pose2& at, float max_m, float* d_m = nullptr,
                             uint8_t* d_class = nullptr) {
    ndt_point_fit f;
    check(ndt2d_fit_points_dev(h_, d_sx, d_sy, n, Dm::pack(at).data(), max_m, d_m, d_class, &f), "ndt2d_fit_points_dev");
    return f;
  }
  // The points whose class is in `keep` (a mask of 1 << NDT_POINT_*), copied to the front of d_ox / d_oy in the source
  // frame, bit for bit and in their order, their scan indices into d_index (may be null): what addTargetPointsDev(...,
  // &pose) and removeTargetPointsDev take.  The count is the summary's n_selected.
  ndt_point_fit selectPointsDev(const float* d_sx, const float* d_sy, size_t n, const Pose2& at, float max_m, uint32_t keep,
                                float* d_ox, float* d_oy, uint32_t* d_index = nullptr) {
    ndt_point_fit f;
    check(ndt2d_select_points_dev(h_, d_sx, d_sy, n, Dm::pack(at).data(), max_m, keep, d_ox, d_oy, d_index, &f),
          "ndt2d_select_points_dev");
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

 private:
  friend class detail::MatcherCore<2, NdtMatcherHip>;
  MatchResult result(const ndt2d_result& r) const { return to_match_result(r, mode_); }
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

// The 3D matcher: the same shape over the ndt3d_* entry points, with detail::MatcherCore's members beside these.
class NdtMatcherHip3 : public detail::MatcherCore<3, NdtMatcherHip3> {
 public:
  explicit NdtMatcherHip3(const ndt3d_params& params = defaultParams(), int device = 0) : MatcherCore(params, device) {}

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
  // device points, optionally moved into the map frame by `pose` first (the pose an alignment returned);
  // producer_stream = the stream that wrote them (nullptr: complete)
  size_t addTargetPointsDev(const float* d_x, const float* d_y, const float* d_z, size_t n, const Pose3* pose = nullptr,
                            void* producer_stream = nullptr) {
    size_t outside = 0;
    const auto p = Dm::pack(pose ? *pose : Pose3());
    check(ndt3d_add_target_points_dev(h_, d_x, d_y, d_z, n, pose ? p.data() : nullptr, &outside, producer_stream),
          "ndt3d_add_target_points_dev");
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
    const auto p = Dm::pack(pose ? *pose : Pose3());
    check(ndt3d_remove_target_points_dev(h_, d_x, d_y, d_z, n, pose ? p.data() : nullptr, &outside, producer_stream),
          "ndt3d_remove_target_points_dev");
    return outside;
  }
  // per-point fit and selection against the voxel grid, as NdtMatcherHip::fitPointsDev / selectPointsDev
  ndt_point_fit fitPointsDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& at, float max_m,
                             float* d_m = nullptr, uint8_t* d_class = nullptr) {
    ndt_point_fit f;
    check(ndt3d_fit_points_dev(h_, d_sx, d_sy, d_sz, n, Dm::pack(at).data(), max_m, d_m, d_class, &f), "ndt3d_fit_points_dev");
    return f;
  }
  ndt_point_fit selectPointsDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& at, float max_m,
                                uint32_t keep, float* d_ox, float* d_oy, float* d_oz, uint32_t* d_index = nullptr) {
    ndt_point_fit f;
    check(ndt3d_select_points_dev(h_, d_sx, d_sy, d_sz, n, Dm::pack(at).data(), max_m, keep, d_ox, d_oy, d_oz, d_index, &f),
          "ndt3d_select_points_dev");
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
  MatchResult3 align(const float* sx, const float* sy, const float* sz, size_t n, const Pose3& guess = Pose3()) {
    ndt3d_result r;
    check(ndt3d_align(h_, sx, sy, sz, n, Dm::pack(guess).data(), &r), "ndt3d_align");
    return toMatchResult(r);
  }
  MatchResult3 alignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const Pose3& guess = Pose3()) {
    ndt3d_result r;
    check(ndt3d_align_dev(h_, d_sx, d_sy, d_sz, n, Dm::pack(guess).data(), &r), "ndt3d_align_dev");
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
    for (size_t k = 0; k < m; ++k) { px[k] = scans[k].x; py[k] = scans[k].y; pz[k] = scans[k].z; ns[k] = scans[k].n; }
    const std::vector<double> init = detail::pack_all<3>(guesses);
    std::vector<ndt3d_result> res(m);
    check(ndt3d_align_multi_scan_dev(h_, px.data(), py.data(), pz.data(), ns.data(), init.data(), static_cast<int32_t>(m), res.data()),
          "ndt3d_align_multi_scan_dev");
    return results(res);
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
  std::vector<SearchHit> searchDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                   const ndt3d_search_window& window, int k, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    return hits(k, [&](int32_t kk, ndt3d_search_hit* h, int32_t* n_hits) {
      check(ndt3d_search_dev(h_, d_sx, d_sy, d_sz, n, &window, kk, h, n_hits), "ndt3d_search_dev");
    });
  }
  // searchDev, then one alignment from every hit in one launch chain (ndt3d_search_align_dev): result i is bit for bit
  // what alignMultiStartDev returns from the hits' poses.  Search with a subsampled scan (voxelFilterDev, or every 8th
  // point) and refine with the full one when the lattice is large.
  std::vector<SearchMatch> searchAlignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                          const ndt3d_search_window& window, int k, void* producer_stream,
                                          bool complete = false) {
    wait(producer_stream, complete);
    return matches(k, [&](int32_t kk, ndt3d_search_hit* h, ndt3d_result* r, int32_t* n_hits) {
      check(ndt3d_search_align_dev(h_, d_sx, d_sy, d_sz, n, &window, kk, h, r, n_hits), "ndt3d_search_align_dev");
    });
  }
  // The score at every pose of a list in one launch (ndt3d_score_poses_dev), as NdtMatcherHip::scorePosesDev: d_poses is
  // [m][6] = (tx, ty, tz, roll, pitch, yaw) in double, all six free - a search over z, roll or pitch is a list.
  void scorePosesDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                     float* d_scores, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    check(ndt3d_score_poses_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, d_scores), "ndt3d_score_poses_dev");
  }
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
    check(ndt3d_range_image_to_points_deskew_dev(d_ranges, n_elev, n_azim, elevations, azimuth0, azimuth_inc, range_min,
                                                 range_max, Dm::pack(motion).data(), frac0, frac_inc, ref_frac, d_x, d_y, d_z,
                                                 stream), "ndt3d_range_image_to_points_deskew_dev");
  }
  // Device points with a sweep fraction each -> the sensor frame at ref_frac (ndt3d_deskew_points_dev); the outputs may
  // be the inputs
  static void deskewPointsDev(const float* d_x, const float* d_y, const float* d_z, const float* d_frac, size_t n,
                              const Pose3& motion, double ref_frac, float* d_ox, float* d_oy, float* d_oz, void* stream) {
    check(ndt3d_deskew_points_dev(d_x, d_y, d_z, d_frac, n, Dm::pack(motion).data(), ref_frac, d_ox, d_oy, d_oz, stream),
          "ndt3d_deskew_points_dev");
  }
  // scorePosesDev for SHORT lists, a team of lanes per pose, with the hit counts (ndt3d_score_particles_dev), as
  // NdtMatcherHip::scoreParticlesDev; d_n_hit may be null
  void scoreParticlesDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                         float* d_scores, uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    check(ndt3d_score_particles_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, d_scores, d_n_hit), "ndt3d_score_particles_dev");
  }
  // the same, returning after the enqueue (ndt3d_score_particles_async): complete in stream order on stream() (ndt3d_stream)
  void scoreParticlesAsync(const float* d_sx, const float* d_sy, const float* d_sz, size_t n, const double* d_poses, size_t m,
                           float* d_scores, uint32_t* d_n_hit, void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
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
    wait(producer_stream, complete);
    return hits(k, [&](int32_t kk, ndt3d_search_hit* h, int32_t* n_hits) {
      check(ndt3d_best_poses_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, kk, h, n_hits),
            "ndt3d_best_poses_dev");
    });
  }
  // bestPosesDev, then one alignment from every hit in one launch chain (ndt3d_best_poses_align_dev)
  std::vector<SearchMatch> bestPosesAlignDev(const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                             const double* d_poses, size_t m, int k, double min_sep_trans, double min_sep_rot,
                                             void* producer_stream, bool complete = false) {
    wait(producer_stream, complete);
    return matches(k, [&](int32_t kk, ndt3d_search_hit* h, ndt3d_result* r, int32_t* n_hits) {
      check(ndt3d_best_poses_align_dev(h_, d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, kk, h, r, n_hits),
            "ndt3d_best_poses_align_dev");
    });
  }
  // a result row with the plain inverse of its Hessian as the covariance
  static MatchResult3 toMatchResult(const ndt3d_result& r) {
    MatchResult3 m = detail::result_row<3>(r);
    invert6(r.H, m.covariance.data());
    return m;
  }

 private:
  friend class detail::MatcherCore<3, NdtMatcherHip3>;
  MatchResult3 result(const ndt3d_result& r) const { return toMatchResult(r); }
};

namespace detail {
// concatenates the pairs into the SoA + offsets form of ndt2d_batch_align / ndt2d_multi_align / ndt3d_batch_align: a
// Cloud is {x, y, n} or {x, y, z, n}; run(t, toff, s, soff, init, n, rows) gets the D coordinate arrays of either side
template <int D, class Clouds, class Convert, class Run>
std::vector<typename Dim<D>::Match> align_pairs(const Clouds& targets, const Clouds& sources,
                                                const std::vector<typename Dim<D>::Pose>& guesses, const char* what,
                                                Convert&& convert, Run&& run) {
  const size_t n = targets.size();
  if (sources.size() != n || guesses.size() != n || n == 0) throw NdtError(NDT_ERR_INVALID_ARG, what);
  std::vector<uint64_t> toff(n + 1, 0), soff(n + 1, 0);
  for (size_t k = 0; k < n; ++k) { toff[k + 1] = toff[k] + targets[k].n; soff[k + 1] = soff[k] + sources[k].n; }
  std::vector<float> t[D], s[D];
  for (int c = 0; c < D; ++c) { t[c].resize(toff[n]); s[c].resize(soff[n]); }
  for (size_t k = 0; k < n; ++k) {
    const float* tc[3] = {targets[k].x, targets[k].y, nullptr};
    const float* sc[3] = {sources[k].x, sources[k].y, nullptr};
    if constexpr (D == 3) { tc[2] = targets[k].z; sc[2] = sources[k].z; }
    for (int c = 0; c < D; ++c) {
      std::copy(tc[c], tc[c] + targets[k].n, t[c].begin() + toff[k]);
      std::copy(sc[c], sc[c] + sources[k].n, s[c].begin() + soff[k]);
    }
  }
  const std::vector<double> init = pack_all<D>(guesses);
  std::vector<typename Dim<D>::Result> res(n);
  check(run(t, toff.data(), s, soff.data(), init.data(), n, res.data()), what);
  std::vector<typename Dim<D>::Match> out;
  out.reserve(n);
  for (const auto& r : res) out.push_back(convert(r));
  return out;
}

// the life of a batch context (ndt2d_batch_*, ndt3d_batch_*)
template <int D>
class BatchCore {
 public:
  BatchCore(const BatchCore&) = delete;
  BatchCore& operator=(const BatchCore&) = delete;
  // NDT_TUNE_BATCH_SMALL_VARIANT (2D) / NDT_TUNE_BATCH_GLOBAL_WORKGROUPS: the slabs of the global-table variant, for the
  // pairs whose grid does not fit on chip (memory against rate; 3D: 1..256 slabs of 7.9 MB)
  void setTuning(int32_t knob, int64_t value) { require_ok(Dim<D>::batch_set_tuning.fn(b_, knob, value), Dim<D>::batch_set_tuning.name); }

 protected:
  BatchCore(const typename Dim<D>::Params& params, int device) {
    require_ok(Dim<D>::batch_create.fn(&params, device, &b_), Dim<D>::batch_create.name);
  }
  // coarse-to-fine: `levels` ordered coarse to fine, one entry for a single level
  BatchCore(const std::vector<typename Dim<D>::Params>& levels, int device) {
    require_ok(Dim<D>::batch_create_pyramid.fn(levels.data(), static_cast<int32_t>(levels.size()), device, &b_),
               Dim<D>::batch_create_pyramid.name);
  }
  ~BatchCore() { Dim<D>::batch_destroy.fn(b_); }
  typename Dim<D>::Batch* b_ = nullptr;
};

// the life of a multi-device context (ndt2d_multi_*, ndt3d_multi_*); devices empty = every visible device
template <int D>
class MultiCore {
 public:
  MultiCore(const MultiCore&) = delete;
  MultiCore& operator=(const MultiCore&) = delete;
  int deviceCount() const { return Dim<D>::multi_device_count.fn(m_); }

 protected:
  MultiCore(const typename Dim<D>::Params& params, const std::vector<int32_t>& devices) {
    require_ok(Dim<D>::multi_create.fn(&params, devices.empty() ? nullptr : devices.data(), static_cast<int32_t>(devices.size()), &m_),
               Dim<D>::multi_create.name);
  }
  // 2D only.  It is here, not in NdtMultiHip, because a constructor there would run after this class's: a failed
  // create would then be followed by ~MultiCore's destroy.
  MultiCore(const std::vector<typename Dim<D>::Params>& levels, const std::vector<int32_t>& devices) {
    static_assert(D == 2, "the 3D library has no ndt3d_multi_create_pyramid");
    require_ok(Dim<D>::multi_create_pyramid.fn(levels.data(), static_cast<int32_t>(levels.size()),
                                               devices.empty() ? nullptr : devices.data(), static_cast<int32_t>(devices.size()), &m_),
               Dim<D>::multi_create_pyramid.name);
  }
  ~MultiCore() { Dim<D>::multi_destroy.fn(m_); }
  typename Dim<D>::Multi* m_ = nullptr;
};

// the Hessian mode a pyramid's results carry: its finest level's
inline int32_t mode_of(const std::vector<ndt2d_params>& levels) {
  return levels.empty() ? NDT_HESSIAN_GAUSS_NEWTON : levels.back().hessian_mode;
}
}  // namespace detail

// Loop-closure candidates: many independent pairs in one call.
class NdtBatchHip : public detail::BatchCore<2> {
 public:
  struct Cloud { const float* x; const float* y; size_t n; };

  explicit NdtBatchHip(const ndt2d_params& params = NdtMatcherHip::defaultParams(), int device = 0)
      : BatchCore(params, device), mode_(params.hessian_mode) {}
  // coarse-to-fine: `levels` ordered coarse to fine (see standardPyramid)
  NdtBatchHip(const std::vector<ndt2d_params>& levels, int device) : BatchCore(levels, device), mode_(detail::mode_of(levels)) {}
  // the library's 3-level schedule (4c, 2c, c) around `fine`
  static std::vector<ndt2d_params> standardPyramid(const ndt2d_params& fine = NdtMatcherHip::defaultParams()) {
    std::vector<ndt2d_params> lv(3);
    detail::require_ok(ndt2d_default_pyramid(&fine, lv.data()), "ndt2d_default_pyramid");
    return lv;
  }

  std::vector<MatchResult> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                 const std::vector<Pose2>& guesses) {
    return detail::align_pairs<2>(targets, sources, guesses, "ndt2d_batch_align",
                                  [&](const ndt2d_result& r) { return to_match_result(r, mode_); },
                                  [&](const std::vector<float>* t, const uint64_t* toff, const std::vector<float>* s,
                                      const uint64_t* soff, const double* init, size_t n, ndt2d_result* res) {
                                    return ndt2d_batch_align(b_, t[0].data(), t[1].data(), toff, s[0].data(), s[1].data(), soff,
                                                             init, n, res);
                                  });
  }

 private:
  int32_t mode_ = NDT_HESSIAN_GAUSS_NEWTON;
};

// The same over several GPUs owned by this process: pairs are split into contiguous
// work-balanced shards, one host thread and one batch context per device.
class NdtMultiHip : public detail::MultiCore<2> {
 public:
  using Cloud = NdtBatchHip::Cloud;

  // devices empty = every visible device
  explicit NdtMultiHip(const ndt2d_params& params = NdtMatcherHip::defaultParams(), const std::vector<int32_t>& devices = {})
      : MultiCore(params, devices), mode_(params.hessian_mode) {}
  NdtMultiHip(const std::vector<ndt2d_params>& levels, const std::vector<int32_t>& devices)
      : MultiCore(levels, devices), mode_(detail::mode_of(levels)) {}

  std::vector<MatchResult> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                 const std::vector<Pose2>& guesses) {
    return detail::align_pairs<2>(targets, sources, guesses, "ndt2d_multi_align",
                                  [&](const ndt2d_result& r) { return to_match_result(r, mode_); },
                                  [&](const std::vector<float>* t, const uint64_t* toff, const std::vector<float>* s,
                                      const uint64_t* soff, const double* init, size_t n, ndt2d_result* res) {
                                    return ndt2d_multi_align(m_, t[0].data(), t[1].data(), toff, s[0].data(), s[1].data(), soff,
                                                             init, n, res);
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
    detail::check(ndt2d_multi_align_dev(m_, tx.data(), ty.data(), toff.data(), sx.data(), sy.data(), soff.data(), init.data(),
                                        n.data(), nullptr, nullptr, rows.data()), "ndt2d_multi_align_dev");
    std::vector<MatchResult> out;
    out.reserve(total);
    for (const ndt2d_result& r : rows) out.push_back(to_match_result(r, mode_));
    return out;
  }

 private:
  int32_t mode_ = NDT_HESSIAN_GAUSS_NEWTON;
};

// 3D loop-closure candidates: many independent 3D pairs in one call (ndt3d_batch_*; the pair's voxel grid
// lives in LDS for its whole alignment).  `levels` coarse to fine for a pyramid, one entry otherwise.
class NdtBatchHip3 : public detail::BatchCore<3> {
 public:
  struct Cloud { const float* x; const float* y; const float* z; size_t n; };

  explicit NdtBatchHip3(const ndt3d_params& params = NdtMatcherHip3::defaultParams(), int device = 0) : BatchCore(params, device) {}
  NdtBatchHip3(const std::vector<ndt3d_params>& levels, int device) : BatchCore(levels, device) {}

  std::vector<MatchResult3> align(const std::vector<Cloud>& targets, const std::vector<Cloud>& sources,
                                  const std::vector<Pose3>& guesses) {
    return detail::align_pairs<3>(targets, sources, guesses, "ndt3d_batch_align", NdtMatcherHip3::toMatchResult,
                                  [&](const std::vector<float>* t, const uint64_t* toff, const std::vector<float>* s,
                                      const uint64_t* soff, const double* init, size_t n, ndt3d_result* res) {
                                    return ndt3d_batch_align(b_, t[0].data(), t[1].data(), t[2].data(), toff, s[0].data(),
                                                             s[1].data(), s[2].data(), soff, init, n, res);
                                  });
  }
  // device arrays laid out as ndt3d_batch_align_dev takes them; asynchronous on `stream` (nullptr: the context's own)
  void alignDev(const float* d_tx, const float* d_ty, const float* d_tz, const uint64_t* d_toff, const float* d_sx,
                const float* d_sy, const float* d_sz, const uint64_t* d_soff, const double* d_init, size_t n_pairs,
                ndt3d_result* d_results, void* stream = nullptr) {
    detail::check(ndt3d_batch_align_dev(b_, d_tx, d_ty, d_tz, d_toff, d_sx, d_sy, d_sz, d_soff, d_init, n_pairs, d_results, stream),
                  "ndt3d_batch_align_dev");
  }
  void* stream() { return ndt3d_batch_stream(b_); }
};

// The 3D candidates over several GPUs owned by this process (ndt3d_multi_*): host pairs split into contiguous
// work-balanced shards, one context and one host thread per device.
class NdtMultiHip3 : public detail::MultiCore<3> {
 public:
  explicit NdtMultiHip3(const ndt3d_params& params = NdtMatcherHip3::defaultParams(), const std::vector<int32_t>& devices = {})
      : MultiCore(params, devices) {}
  ndt3d_multi* raw() { return m_; }     // ndt3d_multi_align / ndt3d_multi_align_dev (RCCL gather) take it
};

}  // namespace ndt
#endif  // NDT_MATCHER_HIP_HPP_

// Sensor motion within a lidar sweep, undone on the device (included at the end of ndt2d_api.hip: one translation unit).
// The motion is one constant twist xi = Log(delta), delta the sensor's pose at the end of the sweep in its frame at the
// start; a point measured at sweep fraction s moves to the sensor frame at fraction s_ref with
// p' = Exp((s - s_ref) xi) p  (docs/ALGORITHM.md section 2.23).  The host takes the logarithm once in double
// (ndt2d_motion_twist / ndt3d_motion_twist) and hands the twist to the kernels by value; every point is worked in
// float64 and rounded to float32 once, at the store.
#pragma once

namespace ndt {

// |angle| below which sin a / a and its kin come from their power series (the terms left out are below 1e-17)
constexpr double kDeskewSmallAngle = 1e-4;
// a 3D delta that turns by this much or more is refused: the logarithm is ill-conditioned near pi
constexpr double kDeskewMaxAngle3 = 3.1;

template <int DIM> struct SweepTwist {
  double v[DIM];                       // rho: the translational part
  double w[DIM == 2 ? 1 : 3];          // omega | phi
  double ref;                          // s_ref
  int zero;                            // xi is exactly zero: every point comes out untouched
};

// sin h / h, by its series below kDeskewSmallAngle (sh = sin h)
__host__ __device__ inline double deskew_sinc(double h, double sh) {
  return fabs(h) < kDeskewSmallAngle ? 1.0 - h * h * (1.0 / 6.0) : sh / h;
}

// p <- Exp(u xi) p.
// SE(2): V(a) = sinc(a/2) R(a/2), so with h = u omega / 2 the translation is u sinc(h) R(h) v and the rotation is the
// double angle of the same sine and cosine: one sincos, nothing that cancels.
// SE(3): with w = u phi, alpha = |w|, h = alpha / 2:  R = I + A [w]x + B [w]x^2,  V = I + B [w]x + C [w]x^2,
// A = sin alpha / alpha = sinc(h) cos h, B = (1 - cos alpha) / alpha^2 = sinc(h)^2 / 2, C = (1 - A) / alpha^2.
template <int DIM>
__device__ __forceinline__ void exp_apply(const SweepTwist<DIM>& xi, double u, double* p) {
  if constexpr (DIM == 2) {
    const double h = 0.5 * (u * xi.w[0]);
    double sh, ch;
    sincos(h, &sh, &ch);
    const double k = u * deskew_sinc(h, sh);
    const double s = 2.0 * sh * ch, c = 1.0 - 2.0 * sh * sh;
    const double tx = k * (ch * xi.v[0] - sh * xi.v[1]), ty = k * (sh * xi.v[0] + ch * xi.v[1]);
    const double x = p[0], y = p[1];
    p[0] = (c * x - s * y) + tx;
    p[1] = (s * x + c * y) + ty;
  } else {
    const double w[3] = {u * xi.w[0], u * xi.w[1], u * xi.w[2]};
    const double r[3] = {u * xi.v[0], u * xi.v[1], u * xi.v[2]};
    const double a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double al = sqrt(a2);
    double A, B, Cc;
    if (al < kDeskewSmallAngle) {
      A = 1.0 - a2 * (1.0 / 6.0); B = 0.5 - a2 * (1.0 / 24.0); Cc = 1.0 / 6.0 - a2 * (1.0 / 120.0);
    } else {
      const double h = 0.5 * al;
      double sh, ch;
      sincos(h, &sh, &ch);
      const double k = sh / h;
      A = k * ch; B = 0.5 * k * k; Cc = (1.0 - A) / a2;
    }
    auto cross = [&](const double* q, double* o) {
      o[0] = w[1] * q[2] - w[2] * q[1]; o[1] = w[2] * q[0] - w[0] * q[2]; o[2] = w[0] * q[1] - w[1] * q[0];
    };
    double wp[3], wwp[3], wr[3], wwr[3];
    cross(p, wp); cross(wp, wwp); cross(r, wr); cross(wr, wwr);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (p[a] + A * wp[a] + B * wwp[a]) + (r[a] + B * wr[a] + Cc * wwr[a]);
  }
}

// What the three kernels do with a point in double: u = 0 and xi = 0 leave it as it is (the identities the contract
// pins bit for bit do not rest on -0.0 + 0.0 or on what a product does to a NaN's payload), anything else goes
// through exp_apply.  Returns whether the point moved.
template <int DIM>
__device__ __forceinline__ bool deskew_point(const SweepTwist<DIM>& xi, double s, double* p) {
  const double u = s - xi.ref;
  if (xi.zero || u == 0.0) return false;
  exp_apply<DIM>(xi, u, p);
  return true;
}

// k_polar_to_points with the beam's sweep fraction frac0 + i frac_inc: the same bearing sincos and validity rule, the
// unrounded products (double)r c, (double)r s go through the motion.
__global__ __launch_bounds__(kBlock) void k_polar_to_points_deskew(const float* __restrict__ r, size_t n, double angle_min,
                                                                    double angle_inc, float range_min, float range_max,
                                                                    SweepTwist<2> xi, double frac0, double frac_inc,
                                                                    float* __restrict__ x, float* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const float ri = r[i];
    double s, c;
    sincos(fma((double)i, angle_inc, angle_min), &s, &c);
    const bool ok = isfinite(ri) & (ri >= range_min) & (ri <= range_max);
    double p[2] = {(double)ri * c, (double)ri * s};
    deskew_point<2>(xi, fma((double)i, frac_inc, frac0), p);
    x[i] = ok ? (float)p[0] : NAN;
    y[i] = ok ? (float)p[1] : NAN;
  }
}

// k_range_image_to_points with azimuth column j fired at fraction frac0 + j frac_inc (every ring of a column at once)
__global__ __launch_bounds__(kBlock) void k_range_image_to_points_deskew(const float* __restrict__ r, int n_elev, int n_azim,
                                                                          RingTable rings, double az0, double az_inc,
                                                                          float range_min, float range_max, SweepTwist<3> xi,
                                                                          double frac0, double frac_inc,
                                                                          float* __restrict__ x, float* __restrict__ y,
                                                                          float* __restrict__ z) {
  const size_t n = (size_t)n_elev * n_azim;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const int e = (int)(i / (size_t)n_azim), j = (int)(i - (size_t)e * n_azim);
    const float ri = r[i];
    double s, c;
    sincos(fma((double)j, az_inc, az0), &s, &c);
    const double ce = rings.cs[2 * e], se = rings.cs[2 * e + 1];
    const bool ok = isfinite(ri) & (ri >= range_min) & (ri <= range_max);
    double p[3] = {(double)ri * (ce * c), (double)ri * (ce * s), (double)ri * se};
    deskew_point<3>(xi, fma((double)j, frac_inc, frac0), p);
    x[i] = ok ? (float)p[0] : NAN;
    y[i] = ok ? (float)p[1] : NAN;
    z[i] = ok ? (float)p[2] : NAN;
  }
}

struct DeskewPtrs { const float* in[3]; float* out[3]; };

// Cartesian points with a fraction each.  A point reads all its coordinates before it stores any, and no thread
// touches another's point, so the outputs may be the inputs.  (No __restrict__: they may alias.)
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_deskew_points(DeskewPtrs a, const float* frac, size_t n, SweepTwist<DIM> xi) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    float q[DIM];
    double p[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) { q[d] = a.in[d][i]; p[d] = (double)q[d]; }
    const float f = frac[i];
    const bool moved = deskew_point<DIM>(xi, (double)f, p);
#pragma unroll
    for (int d = 0; d < DIM; ++d) a.out[d][i] = !isfinite(f) ? NAN : moved ? (float)p[d] : q[d];
  }
}

}  // namespace ndt

namespace {

bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

void euler_to_matrix(const double* e, double R[9]) {        // R = Rz(yaw) Ry(pitch) Rx(roll)
  ndt::rot3_products(std::sin(e[0]), std::cos(e[0]), std::sin(e[1]), std::cos(e[1]), std::sin(e[2]), std::cos(e[2]), R);
}

template <int DIM>
int32_t make_twist(const double* delta, double ref_frac, ndt::SweepTwist<DIM>* out) {
  double xi[DIM == 2 ? 3 : 6];
  const int32_t st = DIM == 2 ? ndt2d_motion_twist(delta, xi) : ndt3d_motion_twist(delta, xi);
  if (st != NDT_OK) return st;
  if (!std::isfinite(ref_frac)) return NDT_ERR_INVALID_ARG;
  out->zero = 1;
  for (int i = 0; i < DIM; ++i) { out->v[i] = xi[i]; out->zero &= xi[i] == 0.0; }
  for (int i = 0; i < (DIM == 2 ? 1 : 3); ++i) { out->w[i] = xi[DIM + i]; out->zero &= xi[DIM + i] == 0.0; }
  out->ref = ref_frac;
  return NDT_OK;
}

template <int DIM>
int32_t deskew_points_dev(const float* const* in, const float* d_frac, size_t n, const double* delta, double ref_frac,
                          float* const* out, void* stream) {
  if (!d_frac || !delta || n == 0) return NDT_ERR_INVALID_ARG;
  ndt::DeskewPtrs a{};
  for (int d = 0; d < DIM; ++d) {
    if (!in[d] || !out[d]) return NDT_ERR_INVALID_ARG;
    a.in[d] = in[d]; a.out[d] = out[d];
  }
  ndt::SweepTwist<DIM> xi;
  { const int32_t ts = make_twist<DIM>(delta, ref_frac, &xi); if (ts != NDT_OK) return ts; }
  hipLaunchKernelGGL((ndt::k_deskew_points<DIM>), dim3(stream_blocks(n)), dim3(ndt::kBlock), 0, (hipStream_t)stream, a, d_frac,
                     n, xi);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_sweep_motion(const double prev[3], const double cur[3], double delta[3]) {
  if (!prev || !cur || !delta || !all_finite(prev, 3) || !all_finite(cur, 3)) return NDT_ERR_INVALID_ARG;
  const double c = std::cos(prev[2]), s = std::sin(prev[2]);
  const double dx = cur[0] - prev[0], dy = cur[1] - prev[1];
  delta[0] = c * dx + s * dy;
  delta[1] = c * dy - s * dx;
  delta[2] = ndt::wrap_angle(cur[2] - prev[2]);
  return NDT_OK;
}

int32_t ndt3d_sweep_motion(const double prev[6], const double cur[6], double delta[6]) {
  if (!prev || !cur || !delta || !all_finite(prev, 6) || !all_finite(cur, 6)) return NDT_ERR_INVALID_ARG;
  bool same = true;
  for (int i = 0; i < 6; ++i) same &= prev[i] == cur[i];
  if (same) {                                               // Rp' Rp is the identity only to rounding: no motion is exactly zero
    for (int i = 0; i < 6; ++i) delta[i] = 0.0;
    return NDT_OK;
  }
  double Rp[9], Rc[9], R[9];
  euler_to_matrix(prev + 3, Rp);
  euler_to_matrix(cur + 3, Rc);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rp[i] * Rc[j] + Rp[3 + i] * Rc[3 + j] + Rp[6 + i] * Rc[6 + j];   // Rp' Rc
    delta[i] = Rp[i] * (cur[0] - prev[0]) + Rp[3 + i] * (cur[1] - prev[1]) + Rp[6 + i] * (cur[2] - prev[2]);
  }
  const double sb = -R[6] < -1.0 ? -1.0 : -R[6] > 1.0 ? 1.0 : -R[6];
  delta[4] = std::asin(sb);
  if (std::fabs(std::cos(delta[4])) < 1e-12) {              // gimbal lock: roll and yaw turn about one axis, roll = 0 by choice
    delta[3] = 0.0;
    delta[5] = std::atan2(-R[1], R[4]);
  } else {
    delta[3] = std::atan2(R[7], R[8]);
    delta[5] = std::atan2(R[3], R[0]);
  }
  return NDT_OK;
}

int32_t ndt2d_motion_twist(const double delta[3], double xi[3]) {
  if (!delta || !xi || !all_finite(delta, 3)) return NDT_ERR_INVALID_ARG;
  const double w = ndt::wrap_angle(delta[2]), h = 0.5 * w;
  const double sh = std::sin(h), ch = std::cos(h), k = ndt::deskew_sinc(h, sh);
  xi[0] = (ch * delta[0] + sh * delta[1]) / k;              // V(w)^-1 = R(-h) / sinc(h)
  xi[1] = (ch * delta[1] - sh * delta[0]) / k;
  xi[2] = w;
  return NDT_OK;
}

int32_t ndt3d_motion_twist(const double delta[6], double xi[6]) {
  if (!delta || !xi || !all_finite(delta, 6)) return NDT_ERR_INVALID_ARG;
  // the rotation as a unit quaternion q = qz qy qx = (qw, v), straight from the half angles: theta = 2 atan2(|v|, qw)
  // is well conditioned at every angle, which the trace of R is not
  const double ca = std::cos(0.5 * delta[3]), sa = std::sin(0.5 * delta[3]), cb = std::cos(0.5 * delta[4]);
  const double sb = std::sin(0.5 * delta[4]), cg = std::cos(0.5 * delta[5]), sg = std::sin(0.5 * delta[5]);
  double qw = cg * cb * ca + sg * sb * sa;
  double v[3] = {cg * cb * sa - sg * sb * ca, cg * sb * ca + sg * cb * sa, sg * cb * ca - cg * sb * sa};
  if (qw < 0.0) { qw = -qw; for (int i = 0; i < 3; ++i) v[i] = -v[i]; }
  const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double half = std::atan2(vn, qw), theta = 2.0 * half;
  if (theta >= ndt::kDeskewMaxAngle3) {
    set_error("the sweep's rotation is 3.1 rad or more: its logarithm is ill-conditioned");
    return NDT_ERR_INVALID_ARG;
  }
  const double scale = vn < ndt::kDeskewSmallAngle ? 2.0 + vn * vn * (1.0 / 3.0) : theta / vn;     // theta / sin(theta / 2)
  const double p[3] = {scale * v[0], scale * v[1], scale * v[2]};
  // rho = V^-1 t,  V^-1 = I - [phi]x / 2 + D [phi]x^2,  D = (1 - (theta / 2) cot(theta / 2)) / theta^2
  const double t2 = theta * theta;
  const double D = theta < ndt::kDeskewSmallAngle ? 1.0 / 12.0 + t2 * (1.0 / 720.0)
                                                  : (1.0 - half * std::cos(half) / std::sin(half)) / t2;
  const double* t = delta;
  const double pt[3] = {p[1] * t[2] - p[2] * t[1], p[2] * t[0] - p[0] * t[2], p[0] * t[1] - p[1] * t[0]};
  const double ppt[3] = {p[1] * pt[2] - p[2] * pt[1], p[2] * pt[0] - p[0] * pt[2], p[0] * pt[1] - p[1] * pt[0]};
  for (int i = 0; i < 3; ++i) {
    xi[i] = t[i] - 0.5 * pt[i] + D * ppt[i];
    xi[3 + i] = p[i];
  }
  return NDT_OK;
}

int32_t ndt2d_polar_to_points_deskew_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc, double range_min,
                                         double range_max, const double delta[3], double frac0, double frac_inc,
                                         double ref_frac, float* d_x, float* d_y, void* stream) {
  if (!d_ranges || !d_x || !d_y || !delta || n == 0 || !std::isfinite(angle_min) || !std::isfinite(angle_inc) ||
      !std::isfinite(frac0) || !std::isfinite(frac_inc))
    return NDT_ERR_INVALID_ARG;
  ndt::SweepTwist<2> xi;
  { const int32_t ts = make_twist<2>(delta, ref_frac, &xi); if (ts != NDT_OK) return ts; }
  hipLaunchKernelGGL(ndt::k_polar_to_points_deskew, dim3(stream_blocks(n)), dim3(ndt::kBlock), 0, (hipStream_t)stream, d_ranges,
                     n, angle_min, angle_inc, (float)range_min, (float)range_max, xi, frac0, frac_inc, d_x, d_y);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

int32_t ndt3d_range_image_to_points_deskew_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim, const double* elevations,
                                               double azimuth0, double azimuth_inc, double range_min, double range_max,
                                               const double delta[6], double frac0, double frac_inc, double ref_frac,
                                               float* d_x, float* d_y, float* d_z, void* stream) {
  if (!d_ranges || !elevations || !d_x || !d_y || !d_z || !delta || n_elev < 1 || n_elev > ndt::kMaxRings || n_azim < 1 ||
      !std::isfinite(azimuth0) || !std::isfinite(azimuth_inc) || !std::isfinite(frac0) || !std::isfinite(frac_inc))
    return NDT_ERR_INVALID_ARG;
  ndt::SweepTwist<3> xi;
  { const int32_t ts = make_twist<3>(delta, ref_frac, &xi); if (ts != NDT_OK) return ts; }
  ndt::RingTable rings;
  if (!ring_table(elevations, n_elev, &rings)) return NDT_ERR_INVALID_ARG;
  const size_t n = (size_t)n_elev * (size_t)n_azim;
  hipLaunchKernelGGL(ndt::k_range_image_to_points_deskew, dim3(stream_blocks(n)), dim3(ndt::kBlock), 0, (hipStream_t)stream,
                     d_ranges, n_elev, n_azim, rings, azimuth0, azimuth_inc, (float)range_min, (float)range_max, xi, frac0,
                     frac_inc, d_x, d_y, d_z);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

int32_t ndt2d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_frac, size_t n, const double delta[3],
                                double ref_frac, float* d_ox, float* d_oy, void* stream) {
  const float* in[2] = {d_x, d_y};
  float* out[2] = {d_ox, d_oy};
  return deskew_points_dev<2>(in, d_frac, n, delta, ref_frac, out, stream);
}

int32_t ndt3d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_z, const float* d_frac, size_t n,
                                const double delta[6], double ref_frac, float* d_ox, float* d_oy, float* d_oz, void* stream) {
  const float* in[3] = {d_x, d_y, d_z};
  float* out[3] = {d_ox, d_oy, d_oz};
  return deskew_points_dev<3>(in, d_frac, n, delta, ref_frac, out, stream);
}

}  // extern "C"

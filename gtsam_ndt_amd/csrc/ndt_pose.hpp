// The source-side pose rule, stated once for host and device (docs/ALGORITHM.md sections 2.5 and 2.6): the wrap of an
// angle onto (-pi, pi] and the products of the 3D rotation R = Rz(yaw) Ry(pitch) Rx(roll) and of its pitch derivative.
// Plain C++, no HIP types and no handle, in the manner of ndt_lattice.hpp.  Every host site that turns a 3D pose into a
// matrix calls these functions, and on the device newton_rot_block3, map_sums_to_pose_frame and make_rt3 (the 3D search
// kernels); make_rot3 calls the pitch derivative only.  NOT through this header: the nine products of R in make_rot3 and
// make_map_pose3, which spell the same expressions themselves (DESIGN.md section 5.1 has the measurements), so the R of
// the alignment chains, the batch kernels and the 3D list kernels is not what tests/cpp/pose_main.cpp runs under the
// host sanitizers; tests/test_gpu_tilted3d.py and tests/test_gpu_seams.py hold those on the device.
//
// The sines and cosines stay with the caller (sincos_wrapped on the device, libm on the host); nothing here wraps an
// angle on the caller's behalf or calls a sine.
//
// Host and device are told apart by the compilation pass.  On the host every operation is rounded separately: the
// contraction pragma below is limited to the host pass of clang, and a compiler that does not know it (the test's g++)
// is given -ffp-contract=off.  tests/seam_ref.rot3d_entries states that form.  On the device the same text is compiled
// under the library's flags, which may fuse a product into the sum behind it; tools/codeobj_diff.py against the parent
// commit decides that the kernels are unchanged.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define NDT_POSE_FN __host__ __device__ __forceinline__
#else
#define NDT_POSE_FN inline
#endif
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#define NDT_POSE_ROUND_EACH _Pragma("clang fp contract(off)")
#else
#define NDT_POSE_ROUND_EACH
#endif

namespace ndt {

// (-pi, pi]: -pi itself goes to +pi
NDT_POSE_FN double wrap_angle(double t) {
  NDT_POSE_ROUND_EACH
  const double pi = 3.141592653589793;
  if (t > pi || t <= -pi) {
    t = t - 2.0 * pi * std::floor((t + pi) / (2.0 * pi));
    if (t <= -pi) t += 2.0 * pi;
  }
  return t;
}

// R = Rz Ry Rx, row-major, from the sines and cosines of roll (a), pitch (b) and yaw (g)
NDT_POSE_FN void rot3_products(double sa, double ca, double sb, double cb, double sg, double cg, double* R) {
  NDT_POSE_ROUND_EACH
  R[0] = cg * cb; R[1] = cg * sb * sa - sg * ca; R[2] = cg * sb * ca + sg * sa;
  R[3] = sg * cb; R[4] = sg * sb * sa + cg * ca; R[5] = sg * sb * ca - cg * sa;
  R[6] = -sb;     R[7] = cb * sa;                R[8] = cb * ca;
}
// dR/dpitch = Rz dRy Rx.  (The roll and yaw derivatives are permutations of R and stay with their callers: a roll
// derivative maps columns (1, 2) -> (col 2, -col 1), a yaw derivative rows (0, 1) -> (-row 1, row 0).)
NDT_POSE_FN void rot3_pitch_products(double sa, double ca, double sb, double cb, double sg, double cg, double* Rb) {
  NDT_POSE_ROUND_EACH
  Rb[0] = -cg * sb; Rb[1] = cg * cb * sa; Rb[2] = cg * cb * ca;
  Rb[3] = -sg * sb; Rb[4] = sg * cb * sa; Rb[5] = sg * cb * ca;
  Rb[6] = -cb;      Rb[7] = -sb * sa;     Rb[8] = -sb * ca;
}

}  // namespace ndt

// What the hand-off of a k_iterate launch's sums costs (scratch tool, not part of the library or the bench): the launch
// chain of tools/exp_iter.hip - a 1M-point wall scene, a 100k-point scan, 31 launches per alignment, the shape of
// config 3 - with three forms of the table between two launches, body and solve the same:
//   rows    EXP = 16: float[12][256], one row per sum; a workgroup leaves twelve 4-byte stores, four waves fold three
//           rows each (the kernel before the table was packed)
//   packed  EXP = 32: float4[3][256], slot = workgroup; three 16-byte stores per workgroup, three waves fold four sums
//           each; every 128-byte line still has writers on all eight XCDs
//   xcd     EXP = 0:  packed, slot (b % 8) * 32 + b / 8, so that the eight writers of a 128-byte line sit on one XCD
//           (the library)
// Per form: us per launch, in aggregate, of N = 1, 2, 3, 4, 6, 8 chains on N non-blocking streams (alignments enqueued
// round-robin from one host thread), host clock over CALLS alignments, REPEATS samples with the forms alternating inside
// every sample so that drift hits all alike; median (min - max).  The xcd column at N chains is the ceiling of a handle
// with N launch chains.  The final state of every form is printed as bits: they must be the same.
//   hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -std=c++17 -Iinclude -Igtsam_ndt_amd/csrc -o tools/bin/exp_tail tools/exp_tail.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gtsam_ndt_amd/csrc/ndt2d_kernels.hpp"
using namespace ndt;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

#ifndef THR
#define THR 256
#endif
constexpr int K = 30, CALLS = 100, REPEATS = 7, NFORM = 3, NCOUNT = 6, kMaxChains = 8;
constexpr int kChains[NCOUNT] = {1, 2, 3, 4, 6, 8};
static const char* const kFormName[NFORM] = {"rows", "packed", "xcd"};

struct Chain {
  hipStream_t st;
  AlignCall* call;
  AlignDyn* dyn;
  hipGraphExec_t ge[NFORM];
};

template <int EXP>
hipGraphExec_t capture(const Chain& c, const AlignStatic* d_st) {
  hipGraph_t g; hipGraphExec_t ge;
  CK(hipStreamBeginCapture(c.st, hipStreamCaptureModeRelaxed));
  for (int k = 0; k <= K; ++k) hipLaunchKernelGGL((k_iterate<0, EXP, THR>), dim3(kMaxBlocks), dim3(THR), 0, c.st, d_st, c.call, c.dyn, k & 1);
  CK(hipStreamEndCapture(c.st, &g));
  CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  CK(hipGraphDestroy(g));
  return ge;
}

// CALLS alignments over `lanes` chains, round-robin; us per launch in aggregate
double sample(Chain* ch, int lanes, int form, const float* sx, const float* sy, int n) {
  for (int l = 0; l < lanes; ++l) CK(hipStreamSynchronize(ch[l].st));
  const auto t0 = std::chrono::steady_clock::now();
  for (int c = 0; c < CALLS; ++c) {
    Chain& x = ch[c % lanes];
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(64), 0, x.st, x.call, x.dyn, sx, sy, n, 0.1, -0.08, 0.01, K, (IterState*)nullptr, (int*)nullptr, 0);
    CK(hipGraphLaunch(x.ge[form], x.st));
  }
  for (int l = 0; l < lanes; ++l) CK(hipStreamSynchronize(ch[l].st));
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  return us / (CALLS * (K + 1));
}

int main(int argc, char** argv) {
  const int n_t = 1000000, n_s = argc > 1 ? atoi(argv[1]) : 100000;
  std::vector<float> tx(n_t), ty(n_t), sx(n_s), sy(n_s);
  unsigned long long z = 88172645463325252ull;
  auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0; };
  // walls of a 4x4 block of 50 m rooms + noise (the scene of exp_iter.hip)
  for (int i = 0; i < n_t; ++i) {
    const int w = (int)(rnd() * 10); const double t = rnd() * 200 - 100, e = (rnd() + rnd() + rnd() + rnd() - 2) * 0.05;
    if (w < 5) { tx[i] = (float)t; ty[i] = (float)(-100 + 50 * w + e); } else { ty[i] = (float)t; tx[i] = (float)(-100 + 50 * (w - 5) + e); }
  }
  for (int i = 0; i < n_s; ++i) {
    const int w = (int)(rnd() * 4); const double t = rnd() * 50, e = (rnd() + rnd() + rnd() + rnd() - 2) * 0.05;
    double X, Y;
    if (w == 0) { X = t; Y = -50 + e; } else if (w == 1) { X = t; Y = 0 + e; } else if (w == 2) { X = 0 + e; Y = t - 50; } else { X = 50 + e; Y = t - 50; }
    sx[i] = (float)(X - 0.1); sy[i] = (float)(Y + 0.08);
  }
  float *dtx, *dty, *dsx, *dsy;
  CK(hipMalloc(&dtx, n_t * 4)); CK(hipMalloc(&dty, n_t * 4)); CK(hipMalloc(&dsx, n_s * 4)); CK(hipMalloc(&dsy, n_s * 4));
  CK(hipMemcpy(dtx, tx.data(), n_t * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dty, ty.data(), n_t * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsx, sx.data(), n_s * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dsy, sy.data(), n_s * 4, hipMemcpyHostToDevice));
  GridDev g{};
  g.cell = 0.5; g.cell32 = 0.5f; g.inv_c = 2.f; g.ox = -101.f; g.oy = -101.f; g.W = 404; g.H = 404;
  g.ngrid = 1; g.gx[0] = g.ox; g.gy[0] = g.oy;
  g.fix_scale = std::ldexp(1.0, kFixShift) / 0.5;
  const size_t nc = (size_t)g.W * g.H;
  CK(hipMalloc(&g.rec, 2 * nc * sizeof(float4))); CK(hipMalloc(&g.acc, nc * sizeof(CellAcc)));
  CK(hipMemset(g.acc, 0, nc * sizeof(CellAcc)));
  int* d_cnt; CK(hipMalloc(&d_cnt, 8)); CK(hipMemset(d_cnt, 0, 8));
  Chain ch[kMaxChains];
  for (Chain& c : ch) {
    CK(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    CK(hipMalloc(&c.call, sizeof(AlignCall))); CK(hipMalloc(&c.dyn, sizeof(AlignDyn)));
    CK(hipMemset(c.dyn, 0, sizeof(AlignDyn)));
  }
  hipStream_t st = ch[0].st;
  hipLaunchKernelGGL((k_accumulate<1>), dim3(2048), dim3(kBlock), 0, st, dtx, dty, (size_t)n_t, g, (unsigned long long*)nullptr);
  hipLaunchKernelGGL((k_finalise<1>), dim3((unsigned)((nc + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, g, 3, 1e-3, d_cnt);
  int cnt[2]; CK(hipMemcpyAsync(cnt, d_cnt, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
  printf("valid cells %d\n", cnt[0]);
  AlignStatic* d_st;
  CK(hipMalloc(&d_st, sizeof(AlignStatic)));
  AlignStatic hs{};
  hs.grid = g;
  hs.prm.d1 = 1.f; hs.prm.d2 = 1.f; hs.prm.max_iterations = 100; hs.prm.min_hits = 3;
  hs.prm.eps_trans = 1e-5; hs.prm.eps_rot = 1e-5; hs.prm.step_max_trans = 0.5; hs.prm.step_max_rot = 0.2;
  CK(hipMemcpy(d_st, &hs, sizeof(hs), hipMemcpyHostToDevice));
  for (Chain& c : ch) {
    c.ge[0] = capture<16>(c, d_st);
    c.ge[1] = capture<32>(c, d_st);
    c.ge[2] = capture<0>(c, d_st);
  }
  std::vector<double> us[NCOUNT][NFORM];
  for (int rep = 0; rep <= REPEATS; ++rep)            // sample 0 is the warm-up
    for (int c = 0; c < NCOUNT; ++c)
      for (int f = 0; f < NFORM; ++f) {
        const double v = sample(ch, kChains[c], f, dsx, dsy, n_s);
        if (rep) us[c][f].push_back(v);
      }
  for (int c = 0; c < NCOUNT; ++c) {
    const int lanes = kChains[c];
    printf("thr %d n_src %d  %d chain%s, us per launch, median (min - max) of %d samples of %d alignments:", THR, n_s, lanes,
           lanes > 1 ? "s" : "", REPEATS, CALLS);
    for (int f = 0; f < NFORM; ++f) {
      std::vector<double>& a = us[c][f];
      std::sort(a.begin(), a.end());
      printf("  %s %.3f (%.3f - %.3f)", kFormName[f], a[a.size() / 2], a.front(), a.back());
    }
    printf("\n");
  }
  // the result of every form, bit for bit
  for (int f = 0; f < NFORM; ++f) {
    sample(ch, 1, f, dsx, dsy, n_s);
    IterState s; CK(hipMemcpy(&s, &ch[0].dyn->state[K & 1], sizeof(s), hipMemcpyDeviceToHost));
    unsigned long long b[4]; memcpy(b, s.pose, 24); memcpy(b + 3, &s.score, 8);
    printf("%-6s pose %.9f %.9f %.9f iter %d nhit %d  bits %016llx %016llx %016llx score %016llx\n", kFormName[f], s.pose[0], s.pose[1],
           s.pose[2], s.iter, s.n_hit, b[0], b[1], b[2], b[3]);
  }
  return 0;
}

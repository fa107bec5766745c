// The text of a launch of the 2D single-scan chain, included into the bodies of k_iterate and k_iterate_first
// (ndt2d_kernels.hpp) - not a header of its own.  It expects, in scope: the template parameters MODE, EXP, THREADS, NG;
// st, call, dyn, parity; a constexpr int FIRST and a BeginArgs b.
//
// Why an include and not a function: the two kernels must run the same body and epilogue, and k_iterate's code object
// must not change (Shared pieces).  As a __forceinline__ function template called from both kernels the
// text came out differently in every k_iterate instance (the sx / sy loads swapped, another exit structure, 2 to 4
// instructions fewer, and one VGPR more in <0, 0, 1024, 4>; tools/codeobj_diff.py), with the LDS arrays declared in the
// function or passed in by reference, with or without __restrict__ on its parameters.  Included, every k_iterate
// instance is identical text to what it was.
//
// FIRST = 1 is launch 0 of a chain with k_begin folded in: the same text with another head.  Its pose, scan and n are
// the kernel arguments b, so nothing in its head waits for `dyn` or `call`; there is no prologue; workgroup 0's thread 0
// writes what k_begin and the old launch 0 left behind between them (begin_chain).  FIRST = 0 never looks at b.
  __shared__ double s_red[kNumAcc];
  __shared__ float s_wave[THREADS / 64][kNumAcc];
  __shared__ float s_t[THREADS / 64][(kNumAcc - 1) * kSumRowStride];
  if (EXP & 8) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Where this lane's share of the previous launch's table lies, as one unsigned 32-bit byte offset (the loads keep the
  // scalar-base form), worked out up here, while the kernel arguments are still on their way.  Waves 0..2 own the three
  // groups of four sums: the entries of the lane's workgroups 4 lane .. 4 lane + 3, which lie partial_slot's 32 entries
  // = 512 bytes apart (EXP & 32, tools/exp_tail.hip: slot = workgroup, 64 contiguous bytes).  The other waves read the
  // entries of workgroups 0..3 of group 0 instead and never look at them.
  static_assert(partial_slot(4 * 5 + 3) == partial_slot(4 * 5) + 3 * (kMaxBlocks / 8), "entries of a lane's four workgroups");
  const unsigned wv = __builtin_amdgcn_readfirstlane(wave);     // uniform: the selects below are scalar
  const unsigned pv_ln = lane & (wv < kNumAcc / 4 ? 63u : 0u);
  const unsigned pv_off = 16u * ((wv < kNumAcc / 4 ? wv * kMaxBlocks : 0u) +
                                 ((EXP & 32) ? 4u * pv_ln : (unsigned)partial_slot(4 * (int)pv_ln)));
  __builtin_amdgcn_sched_barrier(0);     // ... and stays above the wait for them
  const IterState* prev = &dyn->state[parity ^ 1];
  IterState* cur = &dyn->state[parity];
  const bool writer = (blockIdx.x == 0) && (tid == 0);

  // ---- batch 1 of loads.  The partial rows go first: the previous launch wrote them from every XCD, so they come
  // from beyond this XCD's L2 and are the only thing the fold waits for.  They are requested before ps_done and
  // ps_have are known - the table always exists, so the loads are harmless on every path - but pv[] holds nothing
  // meaningful when ps_done is set or ps_have is clear and must not be used there.
  __builtin_amdgcn_sched_barrier(0);     // the four arguments stay one s_load batch above everything else
  float4 pv[4];
  if (!FIRST && !(EXP & 1)) {
    // No exec branch around the loads: hipcc puts the phi copies of the join, and with them a wait for the rows, at the
    // end of such a branch.
    if (EXP & 16) {                      // the row-per-sum table: waves 0..3, three rows each (tools/exp_tail.hip)
      const float* part = &dyn->rows[parity ^ 1][0][0];
      const int off = (THREADS / 64 <= 4 || wave < 4) ? wave * 3 * kMaxBlocks + lane * 4 : 0;
#pragma unroll
      for (int v = 0; v < 3; ++v) pv[v] = *reinterpret_cast<const float4*>(part + off + v * kMaxBlocks);
    } else {
      const char* part = reinterpret_cast<const char*>(&dyn->partials[parity ^ 1][0][0]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pv[j] = *reinterpret_cast<const float4*>(part + pv_off + 16u * ((EXP & 32) ? j : j * (kMaxBlocks / 8)));
    }
  }
  // previous state, static and call part: scalar loads, all in ONE batch behind the row loads, one scalar wait
  // (FIRST: the static part alone; the rest are kernel arguments)
  const double ps_pose0 = FIRST ? b.p0 : prev->pose[0], ps_pose1 = FIRST ? b.p1 : prev->pose[1];
  const double ps_pose2 = FIRST ? b.p2 : prev->pose[2];     // (FIRST: not wrapped yet)
  const int ps_iter = FIRST ? 0 : prev->iter, ps_done = FIRST ? 0 : prev->done, ps_have = FIRST ? 0 : prev->have_partials;
  const int ps_launch = FIRST ? 0 : prev->pad;
  const SolveParams prm = st->prm;
  const GridDev G = st->grid;
  const int n = FIRST ? b.n : call->n;
  const int fixed_iterations = FIRST ? b.fixed_iterations : call->fixed_iterations;
  const float* __restrict__ sx = FIRST ? b.sx : call->sx;
  const float* __restrict__ sy = FIRST ? b.sy : call->sy;
  IterState* const host_state = FIRST ? b.host_state : call->host_state;
  int* const host_flag = FIRST ? b.host_flag : call->host_flag;
  // Pin the read-only scalars here: without this hipcc sinks their s_loads below the
  // `done` branch and they become a third dependent round trip.
  if (FIRST) {     // what comes from memory only: an "s" operand on a kernel argument turns the scalar loads into vector loads
    asm volatile("" ::"s"(G.ox), "s"(G.oy), "s"(G.inv_c), "s"(G.W), "s"(G.H), "s"(G.rec), "s"(prm.d1), "s"(prm.d2));
  } else {
    asm volatile("" ::"s"(G.ox), "s"(G.oy), "s"(G.inv_c), "s"(G.W), "s"(G.H), "s"(G.rec),
                 "s"(prm.d1), "s"(prm.d2), "s"(prm.hessian_mode), "s"(prm.min_hits), "s"(prm.max_iterations), "s"(prm.eps_trans),
                 "s"(prm.eps_rot), "s"(prm.step_max_trans), "s"(prm.step_max_rot), "s"(prm.step_scale), "s"(prm.line_search), "s"(ps_pose0),
                 "s"(ps_pose1), "s"(ps_pose2), "s"(ps_iter), "s"(ps_done), "s"(ps_have), "s"(ps_launch), "s"(fixed_iterations),
                 "s"(host_state), "s"(host_flag));
  }
  const int stride = kMaxBlocks * THREADS;
  int i = blockIdx.x * THREADS + tid;
  float x = 0.f, y = 0.f, x1 = 0.f, y1 = 0.f;
  if (i < n) { x = sx[i]; y = sy[i]; }
  if (i + stride < n) { x1 = sx[i + stride]; y1 = sy[i + stride]; }

  if (ps_done) {                         // uniform: a finished alignment just carries its state
    if (writer) chain_carry_done(cur, prev, host_flag, call);
    return;
  }
  // FIRST: the initial angle is wrapped here, behind the point loads - wrap_angle's branch at the top would split the
  // head's block and with it the argument loads into two batches
  double pose[3] = {ps_pose0, ps_pose1, FIRST ? wrap_angle(ps_pose2) : ps_pose2};
  int iter = ps_iter;
  if (ps_have) {
    double H[6], g[3], score = 0.0;
    int n_hit = 0, status = 0;
    bool done = false;
    if (!(EXP & 1)) {
      // ---- prologue: fixed-order reduction (wave w < 3 owns sums 4w..4w+3), then the solve
      // Keep the rows opaque until here: hipcc otherwise hoists the fold's float64 conversions, and with them the
      // wait for the rows, up to the row loads - in front of the scalar batch and the point loads.
      if ((EXP & 16) ? wave < 4 : wave < kNumAcc / 4) {        // 4 x 66 doubles fit in the epilogue's buffer
#pragma unroll
        for (int v = 0; v < ((EXP & 16) ? 3 : 4); ++v) {
          v4f r = {pv[v].x, pv[v].y, pv[v].z, pv[v].w};
          asm volatile("" : "+v"(r));
          pv[v] = make_float4(r.x, r.y, r.z, r.w);
        }
        if (EXP & 16) fold_rows12(pv, reinterpret_cast<double*>(s_t[wave]), lane, &s_red[wave * 3]);
        else fold_packed4(pv, reinterpret_cast<double*>(s_t[wave]), lane, &s_red[wave * 4]);
      }
      __syncthreads();
      unpack_sums(s_red, H, g, score, n_hit);
      done = gn_update(pose, H, g, n_hit, iter, status, prm, fixed_iterations, score, &dyn->ls[parity ^ 1],
                       &dyn->ls[parity], writer);
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) H[j] = 0.0;
      g[0] = g[1] = g[2] = 0.0;
      iter += 1;
      done = iter >= fixed_iterations;
    }
    if (writer) {
      auto store = [&](IterState* o) {
        pack_state(o, pose, H, g, score, n_hit, iter, status, done ? 1 : 0, ps_launch + 1);
      };
      store(cur);
      chain_announce(store, done, ps_launch + 1, host_state, host_flag, call);
    }
    if (done) return;                    // uniform
  } else if (FIRST) {
    if (writer) begin_chain(const_cast<AlignCall*>(call), dyn, b, pose);
  } else if (writer) {
    copy_state(cur, prev, 1);
  }

  // ---- body: per-point terms at `pose`
  double sn_d, cs_d;
  sincos_wrapped(pose[2], &sn_d, &cs_d);
  const float4* __restrict__ rec = G.rec;
  const PoseF P = make_pose((float)cs_d, (float)sn_d, (float)pose[0], (float)pose[1], G.ox, G.oy, G.inv_c, G.W,
                            G.H, prm.d1, prm.d2);
  Acc2D A;
  acc_zero(A);

  // two points in flight per thread: both gathers are issued before either is consumed
  while (!(EXP & 2) && i < n) {
    const int i2 = i + 2 * stride;
    float xn0 = 0.f, yn0 = 0.f, xn1 = 0.f, yn1 = 0.f;
    if (i2 < n) { xn0 = sx[i2]; yn0 = sy[i2]; }
    if (i2 + stride < n) { xn1 = sx[i2 + stride]; yn1 = sy[i2 + stride]; }
    PointRec r0, r1;
    const bool two = (i + stride) < n;
    if (NG == 1) {
      lookup_point(P, rec, x, y, true, r0);
      lookup_point(P, rec, x1, y1, two, r1);
      accumulate_point<MODE>(P, r0, A);
      accumulate_point<MODE>(P, r1, A);
    } else {
      // overlapping grids (Biber): the same image point scores against every grid
      image_point(P, x, y, r0);
      image_point(P, x1, y1, r1);
      const int ncell = G.W * G.H;
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const int k0 = q * ncell + image_key(P, G.gx[q], G.gy[q], r0, true);
        const int k1 = q * ncell + image_key(P, G.gx[q], G.gy[q], r1, two);
        r0.A = rec[2 * k0]; r0.B = rec[2 * k0 + 1];
        r1.A = rec[2 * k1]; r1.B = rec[2 * k1 + 1];
        accumulate_point<MODE>(P, r0, A);
        accumulate_point<MODE>(P, r1, A);
      }
    }
    x = xn0; y = yn0; x1 = xn1; y1 = yn1; i = i2;
  }
  float acc[kNumAcc];
  acc_store(A, prm.d2, acc);
  acc[11] = 0.f;

  // ---- epilogue: wave tree -> LDS -> this block's entry of the three groups, one 16-byte store each
  // (EXP & 32, tools/exp_tail.hip: slot = workgroup, so that every 128-byte line has writers on all eight XCDs)
  const int slot = (EXP & 32) ? (int)blockIdx.x : partial_slot(blockIdx.x);
  if (EXP & 4) {
    if (tid < kNumAcc / 4) dyn->partials[parity][tid][slot] = make_float4(acc[0], acc[1], acc[0], acc[1]);
    return;
  }
  {
    const float r = wave_reduce11_lds(acc, s_t[wave], lane);
    if ((lane & 3) == 0 && lane < 4 * (kNumAcc - 1)) s_wave[wave][lane >> 2] = r;
  }
  // where lane 4g's entry goes, worked out in front of the barrier (pinned: hipcc otherwise sinks the address
  // arithmetic, a dozen instructions, to the store - the last thing the launch waits for)
  unsigned out_off = 16u * (((unsigned)parity * (kNumAcc / 4) + (unsigned)(tid >> 2)) * kMaxBlocks + (unsigned)slot);
  if (!(EXP & 16)) asm volatile("" : "+v"(out_off));
  __syncthreads();
  if (tid < kNumAcc) {
    float r = 0.f;
    if (tid < kNumAcc - 1) {
#pragma unroll
      for (int w = 0; w < THREADS / 64; ++w) r += s_wave[w][tid];     // fixed order
    }
    if (EXP & 16) {
      dyn->rows[parity][tid][blockIdx.x] = r;
    } else {
      // lanes 0..11 hold one sum each: every quad hands its four to its first lane (quad_perm broadcasts, all twelve
      // lanes still active), and lanes 0, 4 and 8 store 16 bytes each
      const float4 q = make_float4(dpp_mov<0x00, 0xf>(r), dpp_mov<0x55, 0xf>(r), dpp_mov<0xAA, 0xf>(r), dpp_mov<0xFF, 0xf>(r));
      if ((tid & 3) == 0) *reinterpret_cast<float4*>(reinterpret_cast<char*>(&dyn->partials[0][0][0]) + out_off) = q;
    }
  }

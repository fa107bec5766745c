// The host half of the launch-chain protocol for ONE alignment, stated once for the 2D and the 3D handle and for scans and
// map-to-map chains (the device half is ndt_chain.hpp; the plan and the in-flight record are ndt_host.hpp's ChainPlan and
// ChainFlight).  Included behind the kernels and ndt_hip.h, in front of everything that calls finish (one translation
// unit).  A handle here has: stream, h_state, h_flag, graphs, flight, lanes, dyn_of(lane), d_s / d_t with scap / tcap,
// use_graph and check_every.  A 3D handle is one whose lane count is 1 and stays 1, whose use_graph is constantly true and
// whose check_every is constantly 8.  What differs per dimension is HandleTraits<Handle>'s, next to each handle:
//   begin        the head of a chain: the checks, the no-cell result, (2D) the lane fork and the short-scan launch, launch 0
//   scan_chain   the k_iterate* of a scan of n points, its launch shape and lane's context
//   launch_begin the old-protocol first launch (k_begin / k_begin3)
//   kQueuedFetch how a fixed chain's state comes home (run_chain_tail)
#pragma once

#include "ndt_host.hpp"

namespace {

template <class Handle> struct HandleTraits;

// k_iterate* index points with int and look three strides (of up to 256 x 1024 threads) ahead
constexpr size_t kMaxSourcePoints = 0x7fffffffull - 4ull * ndt::kMaxBlocks * 1024ull;

// A chain's kernel, its launch shape, and the three context pointers every launch takes in front of its parity
struct ChainLaunch { const void* func; dim3 grid, block; void *a0, *a1, *a2; };

// The result of an alignment against a grid with no valid cell (IterState or IterState3): the initial pose, NDT_TOO_FEW_CELLS
template <class State>
State no_cell_state(const double* pose) {
  State s;
  std::memset(&s, 0, sizeof(s));
  for (size_t j = 0; j < sizeof(s.pose) / sizeof(s.pose[0]); ++j) s.pose[j] = pose[j];
  s.status = NDT_TOO_FEW_CELLS;
  return s;
}

// Waits for what the host has to keep fed or listen for (a short-scan launch, a converged-mode loop); both run on lane 0.
// The head of the next alignment calls this and nothing more: a fixed chain still in flight is simply followed on the
// stream (the caller gave up its result by not fetching it).
template <class H>
int32_t finish_host_fed(H* h) {
  ndt::ChainFlight& f = h->flight;
  const ndt::ChainFlight::How how = f.how;
  if (!f.host_fed()) return NDT_OK;
  f.how = ndt::ChainFlight::kOnHost;
  bool seen = false;
  if (how == ndt::ChainFlight::kSmallRun) {
    // No stream sync once the flag is up: the kernel read the scan into registers at its start and raises the flag as
    // its last action, after writing the state next to it, so the result is on the host and the source buffers are free.
    HIP_TRY(ndt::spin_until(h->stream, [&]() { return __atomic_load_n(&h->h_flag[0], __ATOMIC_ACQUIRE) != 0; }, &seen));
    HIP_TRY(hipGetLastError());
    // not seen after real syncs: the kernel has ended anyway, fetch_state copies lane 0's state[0]
    if (!seen) { f.how = ndt::ChainFlight::kFetch; f.lane = 0; f.parity = 0; }
    return NDT_OK;
  }
  HIP_TRY(ndt::chunk_run_finish(f.chunk_run, h->stream, h->h_flag, &seen));
  HIP_TRY(hipGetLastError());
  if (!seen) { ndt::set_error("the Gauss-Newton loop did not report its end"); return NDT_ERR_HIP; }
  return NDT_OK;                                          // the finishing launch wrote the result into h_state
}

// The head of every entry point that is about to use the handle's stream for something else than a rotating
// asynchronous alignment.  The secondary lanes need no wait here: the handle's stream was ordered behind their chains when
// those were enqueued (AsyncLane::leave).  The rotation starts over and the secondary lanes are stale from here on
// (lane_step: kOther): the next asynchronous call records fresh fork events behind this entry point's work, and the
// calls that follow it on lanes 1 .. N-1 wait for theirs.  A queued copy into h_state is waited for too: the entry point
// may write h_state from the host.
template <class H>
int32_t finish(H* h) {
  (void)ndt::lane_step(h->lanes, ndt::LaneEvent::kOther);
  if (h->flight.how == ndt::ChainFlight::kQueued) {
    h->flight.how = ndt::ChainFlight::kOnHost;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return finish_host_fed(h);
}

// The state of the last alignment into h_state, from the lane it ran on (the handle's stream is behind every lane's chains)
template <class H>
int32_t fetch_state(H* h) {
  ndt::ChainFlight& f = h->flight;
  { const int32_t fs = finish_host_fed(h); if (fs != NDT_OK) return fs; }
  (void)ndt::lane_step(h->lanes, ndt::LaneEvent::kFinish);
  if (f.how == ndt::ChainFlight::kFetch)
    HIP_TRY(hipMemcpyAsync(h->h_state, &h->dyn_of(f.lane)->state[f.parity], sizeof(*h->h_state), hipMemcpyDeviceToHost, h->stream));
  if (f.how != ndt::ChainFlight::kOnHost) HIP_TRY(hipStreamSynchronize(h->stream));      // kFetch, or kQueued: the copy
  f.how = ndt::ChainFlight::kOnHost;
  return NDT_OK;
}

// Everything behind the first launch of a chain (launch p.first - 1, or a k_begin*): launches p.first .. p.K of kernel c
// on `stream` (lane `lane`; side: that lane if it is a secondary one), and the record of how the state arrives.
//   chunked       the first two chunks on the handle's stream; finish_host_fed keeps the loop fed.  drain: before that
//                 returns, wait until nothing reads the source arrays any more (a caller that owns them may skip it)
//   fixed, graph  one replay; a secondary lane then orders the handle's stream behind itself
//   plain         launches one by one, in converged mode with a state fetch every p.poll launches
// key: the graph's mode in the cache, next to (p.launches, c.grid.x, lane, p.first).
template <class H>
int32_t run_chain_tail(H* h, const ChainLaunch& c, int key, int lane, hipStream_t stream, ndt::AsyncLane* side,
                       const ndt::ChainPlan& p, bool drain) {
  ndt::ChainFlight& f = h->flight;
  const auto* dyn = h->dyn_of(lane);
  int k = p.first;
  if (p.graph) {
    // (a secondary-lane call that fails here leaves its lane behind the fork event at most and nothing else: harmless)
    hipGraphExec_t exec = nullptr;
    HIP_TRY(h->graphs.get(c.func, c.grid, c.block, c.a0, c.a1, c.a2, p.launches, key, h->stream, &exec, lane, p.first));
    if (p.chunked) {
      f.chunk_run.drain = drain;
      f.chunk_run.seq = f.call_seq;
      f.how = ndt::ChainFlight::kChunkRun;               // (also where the second replay fails: the first is in flight)
      HIP_TRY(ndt::chunk_run_begin(f.chunk_run, exec, h->stream, p.chunk, p.K + 1, p.first));
      return NDT_OK;
    }
    HIP_TRY(hipGraphLaunch(exec, stream));
    if (side) HIP_TRY(side->leave(h->stream));
    k = p.K + 1;
  } else {
    for (; k <= p.K; ++k) {
      (void)ndt::launch_chain_kernel(c.func, c.grid, c.block, c.a0, c.a1, c.a2, k & 1, stream);
      if (p.poll > 0 && k < p.K && (k % p.poll) == p.poll - 1) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h->h_state, &dyn->state[k & 1], sizeof(*h->h_state), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h->h_state->done) { ++k; break; }
      }
    }
  }
  HIP_TRY(hipGetLastError());
  f.how = ndt::ChainFlight::kFetch;
  f.lane = lane;
  f.parity = (k - 1) & 1;
  if (HandleTraits<H>::kQueuedFetch) {
    HIP_TRY(hipMemcpyAsync(h->h_state, &dyn->state[f.parity], sizeof(*h->h_state), hipMemcpyDeviceToHost, h->stream));
    f.how = ndt::ChainFlight::kQueued;
  }
  return NDT_OK;
}

// A host cloud into the handle's staging arrays d (capacity *cap), behind the alignment in flight
template <class H, size_t D>
int32_t stage_cloud(H* h, float* (&d)[D], size_t* cap, const float* const* src, size_t n) {
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  ndt::GrowBuf bufs[D];
  for (size_t a = 0; a < D; ++a) bufs[a] = ndt::grow_buf(&d[a]);
  HIP_TRY(ndt::grow(bufs, D, cap, n, n + n / 4 + 1024));
  for (size_t a = 0; a < D; ++a) HIP_TRY(hipMemcpyAsync(d[a], src[a], n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  return NDT_OK;
}
template <class H> int32_t stage_source(H* h, const float* const* s, size_t n) { return stage_cloud(h, h->d_s, &h->scap, s, n); }
template <class H> int32_t stage_target(H* h, const float* const* t, size_t n) { return stage_cloud(h, h->d_t, &h->tcap, t, n); }

// ---- the single-pair entry points (the extern "C" functions pack their coordinate arrays into s) -----------------------

template <class H>
bool scan_set(const float* const* s) {
  for (int a = 0; a < HandleTraits<H>::kDim; ++a) if (!s[a]) return false;
  return true;
}

// ndt*_align_finish
template <class H>
int32_t align_finish(H* h, typename HandleTraits<H>::Result* out) {
  if (!h || !out) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t st = fetch_state(h); if (st != NDT_OK) return st; }
  HandleTraits<H>::to(*h->h_state, out);
  return NDT_OK;
}

// ndt*_align_dev_async: the chain is enqueued (converged mode: its first two chunks; ndt*_align_finish keeps the loop fed)
template <class H>
int32_t align_dev_async(H* h, const float* const* d_s, size_t n, const double* init_pose) {
  if (!h || !scan_set<H>(d_s) || !init_pose) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  return HandleTraits<H>::begin(h, d_s, n, init_pose, -1, /*wait=*/false, /*own_source=*/false);
}

// ndt*_align_dev; own_source: the scan is in the handle's staging arrays, which outlive the call (ndt*_align)
template <class H>
int32_t align_dev(H* h, const float* const* d_s, size_t n, const double* init_pose, typename HandleTraits<H>::Result* out,
                  bool own_source = false) {
  if (!h || !scan_set<H>(d_s) || !init_pose || !out) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const int32_t st = HandleTraits<H>::begin(h, d_s, n, init_pose, -1, /*wait=*/true, own_source);
  return st != NDT_OK ? st : align_finish(h, out);
}

// ndt*_align
template <class H>
int32_t align_host(H* h, const float* const* s, size_t n, const double* init_pose, typename HandleTraits<H>::Result* out) {
  if (!h || !scan_set<H>(s) || !init_pose || !out || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t ss = stage_source(h, s, n); if (ss != NDT_OK) return ss; }
  return align_dev(h, h->d_s, n, init_pose, out, /*own_source=*/true);
}

// ndt*_evaluate_dev (order the handle behind the scan's producer with ndt*_wait_stream first): a chain of one iteration
template <class H, class Eval>
int32_t evaluate_dev(H* h, const float* const* d_s, size_t n, const double* pose, Eval* out) {
  if (!h || !scan_set<H>(d_s) || !pose || !out || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t st = HandleTraits<H>::begin(h, d_s, n, pose, /*fixed_override=*/1, /*wait=*/true, false); if (st != NDT_OK) return st; }
  { const int32_t st = fetch_state(h); if (st != NDT_OK) return st; }
  HandleTraits<H>::to(*h->h_state, out);
  return NDT_OK;
}

// ndt*_evaluate
template <class H, class Eval>
int32_t evaluate_host(H* h, const float* const* s, size_t n, const double* pose, Eval* out) {
  if (!h || !scan_set<H>(s) || !pose || !out || n == 0) return NDT_ERR_INVALID_ARG;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t ss = stage_source(h, s, n); if (ss != NDT_OK) return ss; }
  return evaluate_dev(h, h->d_s, n, pose, out);
}

// ndt*_align_trace: the launch-per-iteration kernels behind a k_begin*, one plain launch and one state fetch per
// iteration; no flag, and the final state stays on the host.
template <class H>
int32_t align_trace(H* h, const float* const* s, size_t n, const double* init_pose, typename HandleTraits<H>::Result* rows,
                    int32_t capacity, int32_t* n_rows, typename HandleTraits<H>::Result* out) {
  using T = HandleTraits<H>;
  if (!h || !scan_set<H>(s) || !init_pose || !rows || capacity < 1 || !n_rows || n == 0 || n > kMaxSourcePoints)
    return NDT_ERR_INVALID_ARG;
  *n_rows = 0;
  if (!h->has_target) return NDT_ERR_NO_TARGET;
  ndt::TraceRange range(T::kTraceAlignTrace);
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  if (h->n_valid < 1) {
    T::to(no_cell_state<typename T::State>(init_pose), &rows[0]);
    if (out) *out = rows[0];
    return NDT_OK;
  }
  { const int32_t ss = stage_source(h, s, n); if (ss != NDT_OK) return ss; }
  const ndt::ChainPlan p = ndt::chain_plan(-1, h->prm.fixed_iterations, h->prm.max_iterations, false, 0, false);
  ndt::next_seq(&h->flight.call_seq);
  T::launch_begin(h, 0, h->stream, h->d_s, n, init_pose, p.fixed, nullptr, nullptr);
  const ChainLaunch c = T::scan_chain(h, n, 0);
  for (int k = 0; k <= p.K; ++k) {
    (void)ndt::launch_chain_kernel(c.func, c.grid, c.block, c.a0, c.a1, c.a2, k & 1, h->stream);
    HIP_TRY(hipGetLastError());
    if (k == 0) continue;                                  // launch 0 only evaluates
    HIP_TRY(hipMemcpyAsync(h->h_state, &h->dyn_of(0)->state[k & 1], sizeof(*h->h_state), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (*n_rows < capacity) T::to(*h->h_state, &rows[(*n_rows)++]);
    if (h->h_state->done) break;
  }
  h->flight.how = ndt::ChainFlight::kOnHost;               // the final state is in h_state
  if (out) T::to(*h->h_state, out);
  return NDT_OK;
}

}  // namespace

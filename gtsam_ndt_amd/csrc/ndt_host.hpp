// Host-side helpers shared by the C-ABI translation units: per-thread error text, the HIP_TRY
// macro that turns a hipError_t into NDT_ERR_HIP without throwing, buffer growth and pinned
// allocation, launch-chain graphs and their cache, the launch chains ("lanes") of asynchronous
// alignments, the plan of a single-pair chain and the record of what it leaves in flight (their users
// are ndt_chain_host.hpp's), and the host half of the converged-mode and build read-back protocols
// (flags in pinned host memory).
#pragma once
#include <hip/hip_runtime.h>

#include <sched.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>

#include "ndt_dyn.hpp"

namespace ndt {

inline std::string& last_error() {
  thread_local std::string e;
  return e;
}
inline void set_error(const char* msg) { last_error() = msg ? msg : ""; }

// One buffer of a group that grows together (grow below): `unit` bytes per element of the group's capacity.
struct GrowBuf { void** p; size_t unit; };
template <class T>
inline GrowBuf grow_buf(T** p, size_t per = 1) { return {reinterpret_cast<void**>(p), per * sizeof(T)}; }

// Makes the buffers of a group, which share the capacity *cap (in elements), hold `need` elements.  If they hold fewer,
// each is freed and allocated again with `want` elements (the caller's slack rule; want >= need): the contents are lost.
// On failure *cap is 0 and the buffers not allocated yet are null, so the next call tries again.
// *grew (optional): the group was reallocated.  pinned: host memory (hipHostMalloc) instead of device memory.
inline hipError_t grow(const GrowBuf* bufs, size_t nbufs, size_t* cap, size_t need, size_t want, bool* grew = nullptr,
                       bool pinned = false) {
  if (grew) *grew = false;
  if (need <= *cap) return hipSuccess;
  *cap = 0;
  for (size_t k = 0; k < nbufs; ++k) {
    const GrowBuf& b = bufs[k];
    if (*b.p) (void)(pinned ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
  }
  for (size_t k = 0; k < nbufs; ++k) {
    const GrowBuf& b = bufs[k];
    const hipError_t e = pinned ? hipHostMalloc(b.p, want * b.unit, hipHostMallocDefault) : hipMalloc(b.p, want * b.unit);
    if (e != hipSuccess) return e;
  }
  *cap = want;
  if (grew) *grew = true;
  return hipSuccess;
}
inline hipError_t grow(std::initializer_list<GrowBuf> bufs, size_t* cap, size_t need, size_t want, bool* grew = nullptr,
                       bool pinned = false) {
  return grow(bufs.begin(), bufs.size(), cap, need, want, grew, pinned);
}
template <class T>
inline hipError_t grow(T** p, size_t* cap, size_t need, size_t want, bool* grew = nullptr) {
  return grow({grow_buf(p)}, cap, need, want, grew);
}

// Pinned host memory of a fixed size, zeroed: a word the host compares with a sequence number (publish_and_wait) must not
// start out equal to one.
template <class T>
inline hipError_t pinned_alloc(T** p, size_t bytes) {
  const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocDefault);
  if (e == hipSuccess) std::memset(*p, 0, bytes);
  return e;
}

}  // namespace ndt

namespace ndt {

// the sharded build counters (ndt_device.hpp: kCountShards pairs of valid / overflowed cells) read back -> their totals
inline void sum_count_shards(const int* hc, int* valid, int* over) {
  int v = 0, o = 0;
  for (int k = 0; k < 16; ++k) { v += hc[2 * k]; o += hc[2 * k + 1]; }
  *valid = v; *over = o;
}

// roctx range over an API call (SURVEY.md section 5 "tracing"): shows up in rocprofv3 --marker-trace around
// the kernels the call enqueues; a few nanoseconds when no profiler is attached, nothing at all when the marker
// library is not on the machine (ndt_dyn.hpp).
struct TraceRange {
  explicit TraceRange(const char* name) { if (roctx().RangePushA) (void)roctx().RangePushA(name); }
  ~TraceRange() { if (roctx().RangePop) (void)roctx().RangePop(); }
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;
};

// Orders everything enqueued on `consumer` from now on behind the work that is in `producer` now
// (event record + stream wait; the host does not block).
// `cached` (optional): an event the caller keeps for this purpose, created on first use - a wait that
// is already enqueued refers to the record that preceded it, so re-recording the event is safe.
inline hipError_t order_after(hipStream_t consumer, hipStream_t producer, hipEvent_t* cached = nullptr) {
  if (producer == consumer) return hipSuccess;
  hipEvent_t ev = cached ? *cached : nullptr;
  hipError_t e = hipSuccess;
  if (!ev) {
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    if (cached) *cached = ev;
  }
  e = hipEventRecord(ev, producer);
  if (e == hipSuccess) e = hipStreamWaitEvent(consumer, ev, 0);
  if (!cached) (void)hipEventDestroy(ev);            // released by the runtime once the wait has been satisfied
  return e;
}

// A linear chain of `launches` launches of one kernel whose last argument is the launch parity
// (k & 1), built with explicit graph nodes.  No stream capture: capture state is process-wide
// in the HIP runtime and this library's handles may be driven from several threads at once.
// first_parity: the parity of the graph's first launch - 1 where launch 0 of the chain is enqueued outside the graph
// (a first launch that carries the per-call arguments, k_iterate_first).
inline hipError_t build_chain_graph(const void* func, dim3 grid, dim3 block, void* a0, void* a1, void* a2,
                                    int launches, hipGraph_t* graph_out, hipGraphExec_t* exec_out, int first_parity = 0) {
  hipGraph_t g = nullptr;
  hipError_t e = hipGraphCreate(&g, 0);
  if (e != hipSuccess) return e;
  hipGraphNode_t prev = nullptr;
  for (int k = 0; k < launches && e == hipSuccess; ++k) {
    int parity = (k + first_parity) & 1;
    void* args[4] = {&a0, &a1, &a2, &parity};
    hipKernelNodeParams p{};
    p.func = const_cast<void*>(func);
    p.gridDim = grid;
    p.blockDim = block;
    p.sharedMemBytes = 0;
    p.kernelParams = args;
    p.extra = nullptr;
    hipGraphNode_t node = nullptr;
    e = hipGraphAddKernelNode(&node, g, prev ? &prev : nullptr, prev ? 1 : 0, &p);
    prev = node;
  }
  if (e == hipSuccess) e = hipGraphInstantiate(exec_out, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); return e; }
  *graph_out = g;
  return hipSuccess;
}

// One plain launch of a kernel of such a chain, with the chain's arguments
inline hipError_t launch_chain_kernel(const void* func, dim3 grid, dim3 block, void* a0, void* a1, void* a2, int parity,
                                      hipStream_t stream) {
  void* args[4] = {&a0, &a1, &a2, &parity};
  return hipLaunchKernel(func, grid, block, args, 0, stream);
}

// The same for chains that alternate two kernels per step (A then B, both taking the step's parity).
inline hipError_t build_chain_graph2(const void* fa, dim3 ga, dim3 ba, const void* fb, dim3 gb, dim3 bb, void* a0, void* a1,
                                     void* a2, int steps, hipGraph_t* graph_out, hipGraphExec_t* exec_out) {
  hipGraph_t g = nullptr;
  hipError_t e = hipGraphCreate(&g, 0);
  if (e != hipSuccess) return e;
  hipGraphNode_t prev = nullptr;
  for (int k = 0; k < 2 * steps && e == hipSuccess; ++k) {
    int parity = (k >> 1) & 1;
    void* args[4] = {&a0, &a1, &a2, &parity};
    hipKernelNodeParams p{};
    p.func = const_cast<void*>((k & 1) ? fb : fa);
    p.gridDim = (k & 1) ? gb : ga;
    p.blockDim = (k & 1) ? bb : ba;
    p.sharedMemBytes = 0;
    p.kernelParams = args;
    p.extra = nullptr;
    hipGraphNode_t node = nullptr;
    e = hipGraphAddKernelNode(&node, g, prev ? &prev : nullptr, prev ? 1 : 0, &p);
    prev = node;
  }
  if (e == hipSuccess) e = hipGraphInstantiate(exec_out, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); return e; }
  *graph_out = g;
  return hipSuccess;
}

// A handle alternates between a few chain lengths (the converged-mode chunk, the fixed-K chain of a
// timing run, the 2-launch chain of an evaluation): keep the last few instantiated graphs instead
// of rebuilding one on every change.
struct ChainGraphCache {
  static constexpr int kSlots = 16;
  struct Slot { int launches = 0, blocks = 0, mode = -1, lane = 0, first_parity = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; unsigned long stamp = 0; };
  Slot slot[kSlots];
  unsigned long clock = 0;
  hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};   // the owner's secondary launch chains (AsyncLane below): replays of their graphs are queued there

  // lane: a graph bakes the AlignCall / AlignDyn pointers of its launches, so each launch chain of a handle has its own.
  // first_parity: and the parities of its launches, so a chain that starts at launch 1 never gets one that starts at launch 0
  hipGraphExec_t find(int launches, int blocks, int mode, int lane = 0, int first_parity = 0) {
    for (Slot& s : slot)
      if (s.exec && s.launches == launches && s.blocks == blocks && s.mode == mode && s.lane == lane &&
          s.first_parity == first_parity) { s.stamp = ++clock; return s.exec; }
    return nullptr;
  }
  // the slot to build into: an empty one, else the least recently used (destroyed first).  Replays
  // of the evicted exec may still be queued (a converged-mode loop leaves up to two chunks of no-op
  // launches behind): the owner's stream (and its secondary lanes) is drained before the exec is destroyed.
  Slot* victim(hipStream_t stream) {
    Slot* v = &slot[0];
    for (Slot& s : slot) {
      if (!s.exec) { v = &s; break; }
      if (s.stamp < v->stamp) v = &s;
    }
    if (v->exec) (void)hipStreamSynchronize(stream);
    if (v->exec) for (hipStream_t l : lane_stream) if (l) (void)hipStreamSynchronize(l);
    release(*v);
    return v;
  }
  void release(Slot& s) {
    if (s.exec) (void)hipGraphExecDestroy(s.exec);
    if (s.graph) (void)hipGraphDestroy(s.graph);
    s = Slot{};
  }
  void clear() { for (Slot& s : slot) release(s); }
  hipError_t get(const void* func, dim3 grid, dim3 block, void* a0, void* a1, void* a2, int launches, int mode,
                 hipStream_t stream, hipGraphExec_t* out, int lane = 0, int first_parity = 0) {
    if (hipGraphExec_t e = find(launches, (int)grid.x, mode, lane, first_parity)) { *out = e; return hipSuccess; }
    Slot* s = victim(stream);
    const hipError_t err = build_chain_graph(func, grid, block, a0, a1, a2, launches, &s->graph, &s->exec, first_parity);
    if (err != hipSuccess) { *s = Slot{}; return err; }
    s->launches = launches; s->blocks = (int)grid.x; s->mode = mode; s->lane = lane; s->first_parity = first_parity;
    s->stamp = ++clock;
    *out = s->exec;
    return hipSuccess;
  }
  // two-kernel chains (build_chain_graph2); `blocks` of the key is the first kernel's grid
  hipError_t get2(const void* fa, dim3 ga, dim3 ba, const void* fb, dim3 gb, dim3 bb, void* a0, void* a1, void* a2, int steps,
                  int mode, hipStream_t stream, hipGraphExec_t* out) {
    if (hipGraphExec_t e = find(steps, (int)ga.x, mode)) { *out = e; return hipSuccess; }
    Slot* s = victim(stream);
    const hipError_t err = build_chain_graph2(fa, ga, ba, fb, gb, bb, a0, a1, a2, steps, &s->graph, &s->exec);
    if (err != hipSuccess) { *s = Slot{}; return err; }
    s->launches = steps; s->blocks = (int)ga.x; s->mode = mode; s->stamp = ++clock;
    *out = s->exec;
    return hipSuccess;
  }
};

// ---- up to four launch chains per handle ---------------------------------------------------------------------------
// Successive asynchronous fixed-iteration alignments on a handle are independent of one another (own scan, own initial
// pose, the same read-only grid), and one launch chain leaves the chip idle for most of every launch.  So
// such calls go round N "lanes" (1 <= N <= kMaxLanes): lane 0 is the handle's stream and device context, lanes 1 .. N-1
// ("secondary") are streams with a context of their own.  The handle's stream stays ordered behind all of them:
//   lane-0 call  enqueue the chain on the handle's stream
//   lane-k call  enqueue the chain on lane k, record its `done` there, the handle's stream waits for `done`
// A secondary lane in turn has to be behind everything on the handle's stream that is NOT a rotating chain (a build, an
// update, a synchronous or converged call, a tuning change: `kOther`) - and behind nothing else: its own previous chain
// is ordered by its stream, and the other lanes' chains share nothing writable with it (own AlignCall / AlignDyn /
// graphs, read-only AlignStatic, grid and scans).  So the fork is taken only when such work may precede the round:
//   lane-0 call  if the secondary lanes are `stale` (a kOther since the last fork; a new handle): record every secondary
//                lane's `fork` on the handle's stream in front of the chain (`mark`); a fork is then pending for each
//                of them (`fork_live`, one bit per lane)
//   lane-k call  if its bit of `fork_live` is set: lane k waits for its fork (`wait`) - everything before the lane-0
//                call that recorded it, not that call's chain - and clears the bit
// In a run of back-to-back asynchronous calls the first round forks and every secondary lane then runs its chains back
// to back: a wait for a fork at every round would put two cross-queue hops (lane k ends -> handle's stream records the
// fork -> lane k starts) between a lane's chains for nothing.  NDT_TUNE_LANE_FORK = 1 forks at every round all the same
// (`record_fork`), to compare the two in one process.
// Anything else that happens on the handle in between starts the rotation over at lane 0, so a lane-k call only ever
// follows calls on lanes 0 .. k-1 directly, and the lane-0 one has recorded the fork if one is due.  ndt*_wait_stream
// is the exception: it orders every lane behind the producer and keeps the rotation.

constexpr int kMaxLanes = 4;

enum class LaneEvent {
  kAsyncFixed,   // an asynchronous call on the fixed-iteration graph path: the kind that rotates
  kWaitStream,   // ndt*_wait_stream
  kOther,        // any other entry point that uses the handle's stream (synchronous calls, converged mode, builds, tuning)
  kFinish        // ndt*_align_finish: every lane idle afterwards
};

struct LaneState {
  int lanes = 2;           // NDT_TUNE_ASYNC_CHAINS / NDT_TUNE_ASYNC_LANES: 1 = everything on lane 0, as a handle without lanes
  int next = 0;            // the lane of the next rotating call
  bool stale = true;       // the secondary lanes are not known to be behind the non-chain work on the handle's stream
  unsigned fork_live = 0;  // bit k: a fork has been recorded since lane k last waited
};

struct LanePlan {
  int lane = 0;              // where this call's chain goes
  bool record_fork = false;  // lane-0 call that may get partners (where every round forks: NDT_TUNE_LANE_FORK = 1)
  bool both_wait = false;    // kWaitStream: the secondary lanes wait for the producer too
  bool mark = false;         // lane-0 call: record the fork events at its head, the secondary lanes are stale
  bool wait = false;         // lane-k call: wait for the fork event, one was recorded since the last wait
};

// What an event on the handle does, and the state after it.  Pure: the only place the rotation and fork rule lives.
inline LanePlan lane_step(LaneState& s, LaneEvent ev) {
  LanePlan p;
  if (s.lanes < 2) { s.next = 0; s.stale = true; s.fork_live = 0; return p; }
  const int lanes = s.lanes < kMaxLanes ? s.lanes : kMaxLanes;
  switch (ev) {
    case LaneEvent::kAsyncFixed:
      if (s.next >= lanes) s.next = 0;
      p.lane = s.next;
      p.record_fork = s.next == 0;
      if (s.next == 0) {
        p.mark = s.stale;
        if (s.stale) { s.fork_live = (1u << lanes) - 2u; s.stale = false; }
      } else {
        p.wait = (s.fork_live >> s.next) & 1u;
        s.fork_live &= ~(1u << s.next);
      }
      s.next = s.next + 1 < lanes ? s.next + 1 : 0;
      break;
    case LaneEvent::kWaitStream:
      p.both_wait = true;
      break;
    case LaneEvent::kOther:
      s.stale = true;
      s.fork_live = 0;
      s.next = 0;
      break;
    case LaneEvent::kFinish:
      s.next = 0;
      break;
  }
  return p;
}

// ---- the plan of one alignment's launch chain -------------------------------------------------------------------------
// The numbers every single-pair chain takes (scan or map-to-map, 2D or 3D; the device half is ndt_chain.hpp): launches
// 0 .. K evaluate, launch k >= 1 solves first.  Launch 0 either stands in front of the graph (`first` = 1: a
// k_iterate*_first, which carries the per-call arguments) or is the graph's first launch behind a k_begin* (`first` = 0).
struct ChainPlan {
  int fixed = 0;         // iterations of a fixed chain, 0: converged mode
  int K = 0;             // the last launch index: fixed, or max_iterations
  int first = 0;         // launches enqueued in front of the graph, and so the parity of the graph's first launch
  bool graph = true;     // one graph replay per chain or chunk; false: plain launches (NDT_TUNE_LAUNCH_GRAPHS = 0)
  bool chunked = false;  // converged mode on graphs: chunks of launches until the finishing launch raises the host flag
                         // (chunk_run_begin below) - the only chains whose first launch gets the host state and flag pointers
  int chunk = 0;         // launches per chunk: even, so that replays keep alternating the parity
  int launches = 0;      // length of the graph to fetch
  int poll = 0;          // plain launches in converged mode: fetch the state every `poll` launches (0: never)
};

// Pure: the only place these decisions live.  fixed_override >= 0 replaces the parameters' fixed_iterations (1: an
// evaluation); first_in_front: launch 0 is enqueued in front of the graph (map-to-map chains never: theirs is k_begin_d2d*).
inline ChainPlan chain_plan(int fixed_override, int fixed_iterations, int max_iterations, bool use_graph, int check_every,
                            bool first_in_front) {
  ChainPlan p;
  p.fixed = fixed_override >= 0 ? fixed_override : fixed_iterations;
  p.K = p.fixed > 0 ? p.fixed : max_iterations;
  p.first = first_in_front ? 1 : 0;
  p.graph = use_graph;
  p.chunked = use_graph && check_every > 0 && p.fixed == 0;
  p.chunk = check_every + (check_every & 1);
  p.launches = p.chunked ? p.chunk : p.K + 1 - p.first;
  p.poll = !use_graph && p.fixed == 0 && check_every > 0 ? check_every : 0;
  return p;
}

// The stream and events of a secondary lane (created with the handle, never inside a call that may be timed)
struct AsyncLane {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, done = nullptr;
  hipError_t create() {
    hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
    return e;
  }
  void destroy() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (fork) (void)hipEventDestroy(fork);
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
    *this = AsyncLane{};
  }
  // head of a lane-0 call (LanePlan::mark), once per secondary lane in use
  hipError_t mark_fork(hipStream_t main) { return hipEventRecord(fork, main); }
  // head of this lane's call (LanePlan::wait): behind everything that preceded the lane-0 call that recorded the fork
  hipError_t enter() { return hipStreamWaitEvent(stream, fork, 0); }
  // tail of this lane's call: the handle's stream is ordered behind this chain
  hipError_t leave(hipStream_t main) {
    const hipError_t e = hipEventRecord(done, stream);
    return e == hipSuccess ? hipStreamWaitEvent(main, done, 0) : e;
  }
};

// Converged mode of the launch-chain paths: replay `exec` (an even-length chunk of launches),
// always one chunk ahead of the one being waited for, until the finishing launch raises flag[0]
// in pinned host memory (it has written its state next to it first).  Nothing but kernel
// launches goes into the stream: no copy, no event, no sync inside the loop; launches enqueued
// past the end exit on the `done` state (about 1.7 us each).
//   flag[0]  raised by the finishing launch
//   flag[1]  index of the last launch that ran its prologue (the host's view of progress)
//   flag[2]  call number, written by the first launch past the end: the source arrays are free
// Launch indices count from the chain's launch 0.  Where that launch was enqueued in front of the chunks (a first launch
// that carries the per-call arguments), chunk w holds launches first + w * chunk .. first + (w + 1) * chunk - 1 with
// first = 1, and its graph starts at parity 1; chunks have even length, so replays keep alternating.
struct ChunkRun {          // a converged-mode loop in flight (begin ... finish)
  hipGraphExec_t exec = nullptr;
  int chunk = 0, max_launches = 0, launched = 0;
  int first = 0;           // index of the first launch of chunk 0: the launches enqueued in front of the chunks
  bool active = false;
  int seq = 0;             // number of this call: flag[2] == seq means "nothing reads the sources any more"
  bool drain = true;       // before returning, wait until nothing reads the source arrays any more (the
                           // first launch past the end says so); a caller that owns those arrays may skip it
};

// Enqueue the first two chunks and return: the asynchronous half.
inline hipError_t chunk_run_begin(ChunkRun& r, hipGraphExec_t exec, hipStream_t stream, int chunk, int max_launches,
                                  int first = 0) {
  r.exec = exec; r.chunk = chunk; r.max_launches = max_launches; r.launched = 0; r.first = first; r.active = true;
  hipError_t e = hipGraphLaunch(exec, stream);
  ++r.launched;
  if (e == hipSuccess) { e = hipGraphLaunch(exec, stream); ++r.launched; }
  return e;
}

// Spin on pinned host memory until `ready()`; the stream is only consulted for errors and, after a
// long time without progress, for a real synchronisation.  (hipStreamQuery is NOT used to decide
// that the stream has drained: with graph replays in flight it was seen to report hipSuccess in
// the middle of an alignment, which made an earlier version of this loop return a state a few
// chunks short of convergence - about one alignment in a hundred with eight busy host threads,
// tools/soak_threads.py.)  Returns hipSuccess with *ok = ready(), or the stream's error.
// How a host thread waits for a flag in pinned memory (ndt_set_host_wait): 0 = spin on the core (default: an
// alignment takes 60-300 us, shorter than a sleep's granularity), 1 = spin for the first ~20 us of a wait, then give the
// core away between polls (sched_yield) - for a SLAM process that drives several handles from several threads on
// fewer cores than threads.  Process-wide; results do not depend on it.
inline std::atomic<int>& host_wait_mode() {
  static std::atomic<int> mode{0};
  return mode;
}

template <class Ready>
inline hipError_t spin_until(hipStream_t stream, Ready&& ready, bool* ok) {
  unsigned long spins = 0;
  int syncs = 0;
  const bool yielding = host_wait_mode().load(std::memory_order_relaxed) == 1;
  for (;;) {
    if (ready()) { *ok = true; return hipSuccess; }
    if (yielding && spins > 2048) sched_yield();
    else __builtin_ia32_pause();                         // a polite spin: yields the core's issue slots to its sibling thread
    if ((++spins & 0xfffff) != 0) continue;
    const hipError_t q = hipStreamQuery(stream);
    if (q != hipSuccess && q != hipErrorNotReady) { *ok = false; return q; }
    if ((spins >> 20) % 48 == 0) {                      // roughly every second of (paused) spinning: a real sync
      const hipError_t es = hipStreamSynchronize(stream);
      if (es != hipSuccess) { *ok = false; return es; }
      if (ready()) { *ok = true; return hipSuccess; }
      if (++syncs >= 2) { *ok = false; return hipSuccess; }   // everything enqueued has run and it is still not ready
    }
  }
}

// Keep one chunk ahead until the flag is raised, then wait until the source arrays are free.
// *seen = true on success; a loop that does not report its end is an error, never a result.
inline hipError_t chunk_run_finish(ChunkRun& r, hipStream_t stream, int* flag, bool* seen) {
  auto raised = [&]() { return __atomic_load_n(&flag[0], __ATOMIC_ACQUIRE) != 0; };
  int waited = 0;
  hipError_t e = hipSuccess;
  *seen = false;
  while (e == hipSuccess) {
    const int need = r.first + (waited + 1) * r.chunk - 1;   // chunk `waited` is through when progress reaches this
    bool ok = false;
    e = spin_until(stream, [&]() { return raised() || __atomic_load_n(&flag[1], __ATOMIC_ACQUIRE) >= need; }, &ok);
    if (e != hipSuccess || raised()) break;
    // ok == false: the stream is idle and the progress counter did not move - feed it anyway; the
    // launch cap below ends a loop that can never finish
    ++waited;
    if (r.first + (r.launched - 1) * r.chunk > r.max_launches + 2 * r.chunk) { e = hipErrorLaunchFailure; break; }
    e = hipGraphLaunch(r.exec, stream);
    ++r.launched;
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(stream);
  } else if (r.drain) {
    // flag[2]: raised by the first launch past the end - the finishing launch (whose other workgroups
    // may still have had point loads in flight when the flag went up) is complete by then, and it left
    // n = 0 behind, so no later launch touches the source arrays.
    // flag[1] now holds the finishing launch's index: if it was the last launch enqueued there is
    // nothing behind it to raise flag[2], and the stream's end is what to wait for.
    const int last = __atomic_load_n(&flag[1], __ATOMIC_ACQUIRE);
    if (r.first + r.launched * r.chunk - 1 > last) {
      bool ok = false;
      e = spin_until(stream, [&]() { return __atomic_load_n(&flag[2], __ATOMIC_ACQUIRE) == r.seq; }, &ok);
      if (e == hipSuccess && !ok) e = hipStreamSynchronize(stream);
    } else {
      e = hipStreamSynchronize(stream);
    }
  }
  *seen = e == hipSuccess && raised();
  r.active = false;
  return e;
}

inline hipError_t run_chunks_until_flag(hipGraphExec_t exec, hipStream_t stream, int* flag, int chunk, int max_launches,
                                        int seq, bool* seen) {
  ChunkRun r;
  r.seq = seq;
  const hipError_t e = chunk_run_begin(r, exec, stream, chunk, max_launches);
  if (e != hipSuccess) { *seen = false; (void)hipStreamSynchronize(stream); return e; }
  return chunk_run_finish(r, stream, flag, seen);
}

// What a handle's last single-pair alignment left in flight, and so how its final state reaches h_state (2D and 3D:
// ndt_chain_host.hpp's run_chain_tail records it, finish and fetch_state consume it).
struct ChainFlight {
  enum How {
    kOnHost,    // nothing in flight: h_state holds the result (or no alignment has run)
    kFetch,     // a chain on `lane` (run, or at least enqueued): fetch_state copies state[parity] of that lane's context
    kQueued,    // a chain with the copy of its final state enqueued behind it: a stream synchronise brings it
    kChunkRun,  // a converged-mode loop the host has to keep fed (chunk_run); its finishing launch writes h_state
    kSmallRun   // a k_align_small launch: it writes h_state, then raises flag[0]
  };
  How how = kOnHost;
  int lane = 0, parity = 0;
  ChunkRun chunk_run;
  int call_seq = 0;        // alignments enqueued so far (never 0 once one has run)
  bool host_fed() const { return how == kChunkRun || how == kSmallRun; }
  bool waits() const { return host_fed() || how == kQueued; }    // finish has something to wait for
};

// The buffers of a handle's multi-start chains, allocated on first use: pinned room for `starts` final states and the
// chains' device context (zeroed on `stream`).
template <class State, class Dyn>
inline hipError_t ensure_multi_chain(State** h_states, int starts, Dyn** d_dyn, hipStream_t stream) {
  hipError_t e = *h_states ? hipSuccess : pinned_alloc(h_states, starts * sizeof(State));
  if (e == hipSuccess && !*d_dyn) {
    e = hipMalloc(reinterpret_cast<void**>(d_dyn), sizeof(Dyn));
    if (e == hipSuccess) e = hipMemsetAsync(*d_dyn, 0, sizeof(Dyn), stream);
  }
  return e;
}

// Runs a multi-start chain whose first launch (k_begin_multi*) is enqueued, until its final states are in h_states.
// Converged mode (flag != null): chunks of `launches` until the finishing launch, which writes the states there itself,
// raises flag[0]; *seen = false: it did not.  Fixed mode: one replay of the whole chain, then a copy of `bytes` from d_states.
inline hipError_t run_multi_chain(hipGraphExec_t exec, hipStream_t stream, int* flag, int launches, int max_launches, int seq,
                                  void* h_states, const void* d_states, size_t bytes, bool* seen) {
  *seen = true;
  if (flag) {
    const hipError_t e = run_chunks_until_flag(exec, stream, flag, launches, max_launches, seq, seen);
    return e != hipSuccess ? e : hipGetLastError();
  }
  hipError_t e = hipGraphLaunch(exec, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h_states, d_states, bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return e;
}

// ---- the plan of a call that carries several map-to-map alignments (ndt2d_align_map_multi, ndt3d_align_map_multi) ---
// Pure host functions: tests/cpp/d2d_multi_host_test.cpp walks them without a device.  The rest of the plan, which
// makes HIP calls, is ndt_map_host.hpp's run_align_map_multi.

// Workgroups of `threads` threads for n items, at most `cap` (a map-to-map launch: one component per lane, kMaxBlocks rows)
inline int capped_blocks(long long n, int threads, int cap) {
  const long long b = (n + threads - 1) / threads;
  return (int)(b < cap ? b : cap);
}

// The smallest power of two >= v (v >= 1): launch shapes in powers of two keep the number of cached graphs small
inline int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// The distinct pointers of in[0 .. m), in the order of their first occurrence, into out (room for m); returns their number.
// A caller's list of source handles may name one handle many times (a multi-start): its derived data is prepared once.
template <class T>
inline int distinct_pointers(T* const* in, int m, T** out) {
  int n = 0;
  for (int k = 0; k < m; ++k) {
    bool seen = false;
    for (int j = 0; j < n && !seen; ++j) seen = out[j] == in[k];
    if (!seen) out[n++] = in[k];
  }
  return n;
}

// The kernel arguments of such a call's first launch, from start k's pose init_poses[P k .. P k + P) (P = the pose length
// of Poses: StartPoses / StartPoses3) and the component list sources[k] has prepared (d_comp, n_comp): sp->p[k], and in
// *sm (StartMaps / StartMaps3, zeroed by the caller) the list, its length and its workgroups (capped_blocks).  A start
// whose source has no component - every start, if the target has no valid cell - keeps n = 0 in its slot: the caller
// answers it on the spot.  Returns the number of the others; *max_blocks = the most workgroups any of them takes (>= 1).
template <class Poses, class Maps, class Source>
inline int plan_map_starts(Source* const* sources, const double* init_poses, int m, bool target_has_cells, int threads,
                           int cap, Poses* sp, Maps* sm, int* max_blocks) {
  constexpr int P = (int)(sizeof(sp->p[0]) / sizeof(sp->p[0][0]));
  int live = 0;
  *max_blocks = 1;
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < P; ++j) sp->p[k][j] = init_poses[P * k + j];
    const int n = target_has_cells ? sources[k]->n_comp : 0;
    if (n < 1) { sm->n[k] = 0; continue; }
    sm->comp[k] = sources[k]->d_comp;
    sm->n[k] = n;
    sm->blocks[k] = capped_blocks(n, threads, cap);
    *max_blocks = sm->blocks[k] > *max_blocks ? sm->blocks[k] : *max_blocks;
    ++live;
  }
  return live;
}

// ---- the device-free half of the batch and multi-device contexts (ndt_batch_host.hpp) -------------------------------
// Pure host functions: tests/cpp/batch_host_test.cpp walks them without a device.  Offsets are CSR style: pair k's
// cloud is points off[k] .. off[k + 1] of the concatenated arrays, so an offset array has n_pairs + 1 entries.

// What a batch call accepts of its offsets: none decreases, and no cloud has more than max_cloud points (kBatchMaxCloud:
// a cloud of a pair is indexed with 32-bit byte offsets on the device)
inline bool pair_offsets_ok(const uint64_t* toff, const uint64_t* soff, size_t n_pairs, uint64_t max_cloud) {
  for (size_t k = 0; k < n_pairs; ++k)
    if (toff[k + 1] < toff[k] || soff[k + 1] < soff[k] || toff[k + 1] - toff[k] > max_cloud || soff[k + 1] - soff[k] > max_cloud)
      return false;
  return true;
}

// The split of n_pairs pairs into n_shards contiguous, work-balanced shards (ndt2d_multi_plan_hinted): shard d gets
// pairs shard_begin[d] .. shard_begin[d + 1].  false, with shard_begin untouched: an offset decreases.
inline bool plan_shards(int n_shards, const uint64_t* toff, const uint64_t* soff, size_t n_pairs, int iterations_hint,
                        const int32_t* pair_iterations, uint64_t* shard_begin) {
  const double kk = iterations_hint > 0 ? iterations_hint : 30;
  // work of a pair = its target points once (grid build: three passes) + its source points per iteration; the
  // iterations from the caller's per-pair hint where it gives one (converged-mode batches: what the candidate took at
  // the coarser level, or last time), else the common hint
  auto work = [&](size_t k) {
    const double it = pair_iterations && pair_iterations[k] > 0 ? (double)pair_iterations[k] : kk;
    return 3.0 * double(toff[k + 1] - toff[k]) + it * double(soff[k + 1] - soff[k]) + 1.0;
  };
  double total = 0;
  for (size_t k = 0; k < n_pairs; ++k) {
    if (toff[k + 1] < toff[k] || soff[k + 1] < soff[k]) return false;
    total += work(k);
  }
  size_t k = 0;
  double acc = 0;
  shard_begin[0] = 0;
  for (int d = 1; d <= n_shards; ++d) {
    const double goal = total * d / n_shards;
    // a pair goes to the shard in which its midpoint falls: contiguous, deterministic, balanced
    while (k < n_pairs && acc + 0.5 * work(k) <= goal) acc += work(k++);
    shard_begin[d] = d == n_shards ? n_pairs : k;
  }
  return true;
}

// The offsets of the shard of pairs k0 .. k1 rebased to its first point, so that only its own points are uploaded:
// out[0 .. k1 - k0] (k1 - k0 + 1 entries, out[0] = 0)
inline void rebase_shard(const uint64_t* off, size_t k0, size_t k1, uint64_t* out) {
  for (size_t k = k0; k <= k1; ++k) out[k - k0] = off[k] - off[k0];
}

// The layout of the all-gather of result rows (multi_align_dev): every shard sends `stride` rows, the longest shard's
// number (its own, then zeroed padding), as `count` doubles; shard d's rows sit at row d * stride of every receive buffer.
struct GatherLayout { size_t stride = 0, count = 0, total = 0; };    // total: the pairs of all shards
inline GatherLayout gather_layout(const size_t* n_pairs, int n_shards, size_t row_bytes) {
  GatherLayout g;
  for (int d = 0; d < n_shards; ++d) {
    g.stride = n_pairs[d] > g.stride ? n_pairs[d] : g.stride;
    g.total += n_pairs[d];
  }
  g.count = g.stride * (row_bytes / sizeof(double));
  return g;
}

// Global pair order out of a receive buffer, padding dropped: copy(to, from, rows) for every shard that has rows, in
// rows of the caller's array (to) and of the receive buffer (from).  Returns the first result of copy that is not `ok`.
template <class Status, class Copy>
inline Status ungather(const size_t* n_pairs, int n_shards, size_t stride, Status ok, Copy&& copy) {
  size_t k = 0;
  for (int d = 0; d < n_shards; ++d) {
    if (n_pairs[d] > 0) { const Status st = copy(k, (size_t)d * stride, n_pairs[d]); if (st != ok) return st; }
    k += n_pairs[d];
  }
  return ok;
}

// The pinned 256-byte block of a handle (h_small): counter shards at 0, the outside count at 128, the cells a removal broke
// behind it (word kCountUnder of ndt_device.hpp), the flag of a build's read-back (publish_and_wait) at byte kSmallFlagByte.
constexpr size_t kSmallBytes = 256, kSmallFlagByte = 192;
inline int* small_flag(void* h_small) { return reinterpret_cast<int*>(static_cast<char*>(h_small) + kSmallFlagByte); }

inline bool flag_raised(const int* flag, int seq) { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq; }

// Advances a sequence number the device echoes into pinned memory (1 .. 2^31 - 1, never 0: pinned blocks start zeroed) and
// returns it: a build's read-back (publish_and_wait below) or an alignment call (ChunkRun::seq, the number k_begin* hands to
// the chain).  flag: the converged-mode flags of an alignment call (ChunkRun), whose flag[0] and flag[1] are cleared first.
inline int next_seq(int* seq, int* flag = nullptr) {
  if (flag) {
    __atomic_store_n(&flag[0], 0, __ATOMIC_RELAXED);
    __atomic_store_n(&flag[1], 0, __ATOMIC_RELAXED);
  }
  return *seq = *seq == 0x7fffffff ? 1 : *seq + 1;
}

// The read-back of a build through pinned memory: advances *seq (next_seq) and calls launch(seq), which enqueues the publish
// kernel (k_build_publish, k_build_publish_clear3 or k_bounds3_publish): it writes its words into pinned memory, then raises
// *flag to seq.  The host spins on the flag.  *seen = false: it did not come (a stream error, or a second of silence) - the
// caller's fallback decides what that means.
template <class Launch>
inline hipError_t publish_and_wait(hipStream_t stream, int* seq, const int* flag, Launch&& launch, bool* seen) {
  const int want = next_seq(seq);
  *seen = false;
  launch(want);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return spin_until(stream, [&]() { return flag_raised(flag, want); }, seen);
}

// Scratch of ndt*_fit_points* / ndt*_select_points* (ndt_point_fit.hpp), grown on first use and freed with the handle.
struct PointFitScratch {
  unsigned char* d_cls = nullptr; size_t cls_cap = 0;     // a class per point, where the caller gives no array
  float* d_m = nullptr; size_t m_cap = 0;                 // m per point on its way to a host array
  uint4* d_table = nullptr;                               // per tile: the four class counts
  unsigned int* d_base = nullptr; size_t tile_cap = 0;    // per tile: the kept points in front of it
  uint4* h_table = nullptr; size_t h_cap = 0;             // pinned (zeroed when it grows): the table's read-back
  void release() {
    void* dev[] = {d_cls, d_m, d_table, d_base};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (h_table) (void)hipHostFree(h_table);
    *this = PointFitScratch{};
  }
};

// What the kernels of ndt*_voxel_filter* (ndt_voxel_filter.hpp) hand to the host and to each other: the occupied box as
// unsigned maxima (0: no valid point yet, so a memset starts a call), and three counts.
struct VoxHeader {
  unsigned int hi[3];        // max over the valid points of i + 2^30 (>= 1)
  unsigned int lo[3];        // max of 2^30 - i (>= 1)
  unsigned int n_invalid, n_voxels, n_out, pad;
};

// Scratch of ndt*_voxel_filter* (ndt_voxel_filter.hpp), grown to need and freed with the handle.
struct VoxelFilterScratch {
  VoxHeader* d_hdr = nullptr;
  VoxHeader* h_hdr = nullptr;                             // pinned: the header's read-back
  uint2* d_words = nullptr; size_t word_cap = 0;          // per 32 voxels of the box: (occupancy bits, occupied voxels in front)
  unsigned int* d_chunk_sum = nullptr;                    // per chunk of words: its occupied voxels
  unsigned int* d_chunk_base = nullptr; size_t chunk_cap = 0;   // ... and those of the chunks in front of it
  unsigned int* d_cnt = nullptr;                          // per occupied voxel, in the contract's order: n
  unsigned int* d_key = nullptr;                          // ... its index in the box
  unsigned long long* d_sum = nullptr; size_t vox_cap = 0;      // ... and the sums of U, [3][vox_cap]
  unsigned int* d_tile_cnt = nullptr;                     // per tile of voxels: those with n >= min_points
  unsigned int* d_tile_base = nullptr; size_t tile_cap = 0;     // ... and those of the tiles in front of it
  float* d_out = nullptr;                                 // the host entry's outputs, [3][out_cap]
  unsigned int* d_ocnt = nullptr; size_t out_cap = 0;
  void release() {
    void* dev[] = {d_hdr, d_words, d_chunk_sum, d_chunk_base, d_cnt, d_key, d_sum, d_tile_cnt, d_tile_base, d_out, d_ocnt};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (h_hdr) (void)hipHostFree(h_hdr);
    *this = VoxelFilterScratch{};
  }
};

}  // namespace ndt

#define HIP_TRY(expr)                                                           \
  do {                                                                           \
    const hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                      \
      ::ndt::last_error() = std::string(#expr) + ": " + hipGetErrorString(_e);   \
      (void)hipGetLastError();                                                   \
      return NDT_ERR_HIP;                                                        \
    }                                                                            \
  } while (0)

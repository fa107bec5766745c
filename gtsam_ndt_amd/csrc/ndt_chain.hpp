// Device half of the launch-chain protocol: how the one thread of a launch that talks to the host does it.
// The words are those of ChunkRun in ndt_host.hpp (flag[0] raised by the finishing launch, flag[1] the index of the last
// launch that ran its prologue, flag[2] the call number once nothing reads the sources any more); the host half is
// feed_chunks there.  Dimension-free: templated on the state and call types of the chain.
#pragma once
#include <hip/hip_runtime.h>

namespace ndt {

// A single chain's launch has updated its state (`store(p)` writes that state to *p).  Finishing launch: the final state
// and this launch's number first, then n = 0 so that the launches enqueued past the end load nothing, a system fence,
// and only then the flag, with release - the host reads the state as soon as it sees flag[0].  Any other launch: progress.
template <class Store, class State, class Call>
__device__ __forceinline__ void chain_announce(Store&& store, bool done, int launch, State* host_state, int* host_flag,
                                               const Call* call) {
  if (!host_flag) return;
  if (done) {
    store(host_state);
    __hip_atomic_store(host_flag + 1, launch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const_cast<Call*>(call)->n = 0;
    __threadfence_system();
    __hip_atomic_store(host_flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    __hip_atomic_store(host_flag + 1, launch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// A launch past the end of a single chain carries the finished state.  The launch that finished the loop is complete
// (this one started after it) and left n = 0 behind: nothing reads the source arrays any more - the host may hand them back.
// copy_state(State*, const State*, int) of the chain's state type must be visible where a kernel calls this
// (ndt2d_kernels.hpp, ndt3d_kernels.hpp): it is looked up at instantiation.
template <class State, class Call>
__device__ __forceinline__ void chain_carry_done(State* cur, const State* prev, int* host_flag, const Call* call) {
  copy_state(cur, prev, -1);
  if (host_flag) __hip_atomic_store(host_flag + 2, call->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The herald of a chain that carries several alignments (every final state went to the host, fenced, when its start
// finished).  While anything runs: progress.  Not from the launches past the end: they may execute after the host has
// reset the flags for its NEXT call, and a stale progress number there makes that call's feeding loop run ahead of its
// own chain (found by tools/soak_round2.py).  First launch after every start has finished (`armed`: call->n as this
// launch read it): stop the launches behind it from loading points, then raise the flag.  The ones after it: the first
// is complete, the sources are free.  host_flag is not null (a call without host flags announces nothing).
template <class Call>
__device__ __forceinline__ void multi_announce(bool running, int launch, int armed, int* host_flag, const Call* call) {
  if (running) {
    __hip_atomic_store(host_flag + 1, launch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else if (armed != 0) {
    const_cast<Call*>(call)->n = 0;
    __threadfence_system();
    __hip_atomic_store(host_flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    __hip_atomic_store(host_flag + 2, call->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace ndt

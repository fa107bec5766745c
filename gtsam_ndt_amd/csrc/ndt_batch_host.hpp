// The host plumbing that the 2D and the 3D loop-closure batch context share, and the multi-device context built on it
// (included in front of ndt2d_batch_api.hpp and ndt3d_batch_api.hpp: one translation unit), as function templates over
// the context type; what differs per dimension is BatchTraits<Ctx>'s (next to each context).  The device-free parts -
// offset validation, shard split, shard rebasing, gather layout - are ndt_host.hpp's.
//   batch context         one device: staging for host pointers, the table slabs of the global-table variant (a few to
//                         begin with, one per CU on demand), single-pair handles for what no batch variant holds
//   multi-device context  one batch context per device, in two forms:
//     multi_align      host pointers: one host thread per device, pairs split into contiguous, work-balanced shards
//                      (plan_shards), results written straight into the caller's array - no collective, the host
//                      array is the meeting point;
//     multi_align_dev  device-resident shards: every context aligns its shard on its own stream and the result rows
//                      are exchanged with ONE grouped ncclAllGather (RCCL over xGMI) on those streams - north_star's
//                      "final RCCL gather".  RCCL is loaded on first use (ndt_dyn.hpp).
// Pairs are independent, so there is no exchange step during the alignments in either form.  The
// one-process-per-GPU deployment (torch.distributed, backend "nccl" = RCCL) lives in gtsam_ndt_amd/dist.py / bench.py.
#pragma once

#include <thread>
#include <vector>

#include "ndt2d_batch.hpp"      // kBatchMaxCloud

// What the shared code needs of a context type Ctx (ndt2d_batch_api.hpp, ndt3d_batch_api.hpp):
//   Result, Handle, Args                  the result row, the single-pair handle, the kernels' argument struct
//   kDim, kPose                           coordinates per point (2, 3), pose length (3, 6)
//   kSlabBytes, kBlocksStart / Full / Max the global-table variant's slab per workgroup, and how many a context begins
//                                         with / grows to / may be told to have
//   kTraceLaunch, kTraceGather            names of the marker ranges
//   create / set_target / align / destroy of the single-pair handle; create_context (ndt*_batch_create_pyramid)
//   variants()                            every kernel variant (BatchVariant: the LDS opt-in of create)
//   create_own, free_own, bind_own        what the context holds beside the common fields: made, freed, put into Args
//   set_clouds                            the coordinate pointers of Args
//   launch_level                          one resolution level: the only code that names kernels
//   own_knob, tune_own                    the knobs beside NDT_TUNE_BATCH_GLOBAL_WORKGROUPS: is it one, set it
//   read_back, host_done                  beside the result rows of a host-pointer call: enqueued, and once they are there
namespace { template <class Ctx> struct BatchTraits; }

namespace ndt {

// The fields both batch contexts have
template <int kDim, class Result, class Handle>
struct BatchContext {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<ndt2d_params> levels;   // coarse to fine; one entry unless created as a pyramid
  int n_cu = 0;
  unsigned int* d_queue = nullptr;
  // staging for the host-pointer entry point
  // (one capacity per buffer: a failed allocation of one must not leave its sibling's capacity standing)
  float *d_t[kDim] = {}, *d_s[kDim] = {};
  size_t cap_t[kDim] = {}, cap_s[kDim] = {};
  uint64_t *d_toff = nullptr, *d_soff = nullptr;
  double* d_init = nullptr;
  Result* d_out = nullptr;
  size_t cap_toff = 0, cap_soff = 0, cap_init = 0, cap_out = 0;
  std::vector<Handle*> fallback;      // single-pair path (one handle per level) for pairs no batch variant holds
  int* d_fb = nullptr;                // [n_pairs]: marks of the pairs the on-chip variant left to the global-table one
  size_t fb_cap = 0;
  unsigned char* d_gslab = nullptr;   // [global_blocks][kSlabBytes]: tables of the global-table variant
  int global_blocks = 0;              // its workgroups (and slabs): a few to begin with, one per CU once a call has used them
  bool global_pinned = false;         // ... unless NDT_TUNE_BATCH_GLOBAL_WORKGROUPS fixed the number
  unsigned int* h_fb_seen = nullptr;  // pinned host word the global-table variant counts its pairs in
};

// One kernel variant in its two instantiations (fn[1]: full Newton Hessian) with its workgroup shape
template <class Args>
struct BatchVariant { void (*fn[2])(Args); int threads, lds_bytes; };

// One batch context per device (BatchTraits<Ctx>::Result: complete where a multi-device context is defined)
template <class Ctx>
struct MultiContext {
  using Batch = Ctx;
  std::vector<Ctx*> ctx;
  int32_t iterations_hint = 30;      // expected evaluations per pair over all levels (shard balancing)
  // device-resident form (multi_align_dev): one RCCL communicator per context, created on first use
  std::vector<ncclComm_t> comms;
  std::vector<typename BatchTraits<Ctx>::Result*> d_send;  // [ctx]: this device's rows, padded to the longest shard
  std::vector<typename BatchTraits<Ctx>::Result*> d_recv;  // [ctx]: every device's rows after the all-gather
  size_t gather_cap = 0;                                   // rows per shard the buffers hold
};

}  // namespace ndt

namespace {

template <class Args>
int32_t launch_variant(const BatchVariant<Args>& v, bool newton, int blocks, hipStream_t st, const Args& a) {
  hipLaunchKernelGGL(v.fn[newton ? 1 : 0], dim3(blocks), dim3(v.threads), v.lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

inline size_t batch_slack(size_t k) { return k + k / 4 + 64; }   // the staging buffers' room to grow

// The global-table variant's slabs (3.7 MB / 7.9 MB per workgroup in 2D / 3D) are most of a context's memory and most
// batches never touch them, so a context is created with a few and gets one per CU only when a previous call has
// handed pairs to that variant (counted by the kernel in a pinned host word - no synchronisation to learn it).  The
// call that first meets such pairs runs them on the starting set: slower for that call, the same results.
template <class Ctx>
void grow_global_slabs(Ctx* b, hipStream_t st) {
  using T = BatchTraits<Ctx>;
  const int full = b->n_cu < T::kBlocksFull ? b->n_cu : T::kBlocksFull;
  if (b->global_pinned || b->global_blocks >= full || !b->h_fb_seen) return;
  if (__atomic_load_n(b->h_fb_seen, __ATOMIC_RELAXED) == 0) return;
  // earlier launches on either stream may still be using the present slabs
  if (hipStreamSynchronize(st) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) { (void)hipGetLastError(); return; }
  unsigned char* bigger = nullptr;
  if (hipMalloc((void**)&bigger, (size_t)full * T::kSlabBytes) != hipSuccess) {
    (void)hipGetLastError();
    b->global_pinned = true;            // not enough memory for the full set: stay with what there is
    return;
  }
  (void)hipFree(b->d_gslab);
  b->d_gslab = bigger;
  b->global_blocks = full;
}

// What a level's launches take from its parameters
template <class Args>
void fill_level(Args& a, const ndt2d_params& p, bool chained) {
  a.chain = chained ? 1 : 0;
  a.min_points = p.min_points;
  a.fixed_iterations = p.fixed_iterations;
  a.cell = p.cell_size;
  a.eig_ratio = p.eig_ratio;
  a.prm.d1 = (float)p.d1; a.prm.d2 = (float)p.d2;
  a.prm.hessian_mode = p.hessian_mode;
  a.prm.max_iterations = p.max_iterations;
  a.prm.min_hits = p.min_hits;
  a.prm.line_search = p.line_search;
  a.prm.eps_trans = p.eps_trans; a.prm.eps_rot = p.eps_rot;
  a.prm.step_max_trans = p.step_max_trans; a.prm.step_max_rot = p.step_max_rot;
  a.prm.step_scale = p.step_scale > 0.0 ? p.step_scale : 1.0;
}

// Every level of the context on n_pairs device-resident pairs, enqueued on st.  A later level starts every pair from
// the pose the previous one left in d_out; stream order is the only synchronisation between launches.
template <class Ctx>
int32_t batch_launch(Ctx* b, const float* const* d_t, const uint64_t* d_toff, const float* const* d_s, const uint64_t* d_soff,
                     const double* d_init, size_t n_pairs, typename BatchTraits<Ctx>::Result* d_out, hipStream_t st) {
  using T = BatchTraits<Ctx>;
  TraceRange range(T::kTraceLaunch);
  typename T::Args a{};
  T::set_clouds(a, d_t, d_s);
  a.toff = reinterpret_cast<const unsigned long long*>(d_toff);
  a.soff = reinterpret_cast<const unsigned long long*>(d_soff);
  a.init = d_init;
  a.out = reinterpret_cast<decltype(a.out)>(d_out);
  a.queue = b->d_queue;
  a.n_pairs = (int)n_pairs;
  HIP_TRY(grow(&b->d_fb, &b->fb_cap, n_pairs, batch_slack(n_pairs)));
  grow_global_slabs(b, st);
  a.fb_marks = b->d_fb;
  a.fb_seen = b->h_fb_seen;
  { const int32_t os = T::bind_own(b, a, n_pairs); if (os != NDT_OK) return os; }
  for (size_t lv = 0; lv < b->levels.size(); ++lv) {
    fill_level(a, b->levels[lv], lv > 0);
    const int32_t ls = T::launch_level(b, a, b->levels[lv], n_pairs, st);
    if (ls != NDT_OK) return ls;
  }
  return NDT_OK;
}

template <class Ctx>
int32_t batch_destroy(Ctx* b) {
  using T = BatchTraits<Ctx>;
  if (!b) return NDT_OK;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  T::free_own(b);
  void* dev[] = {b->d_gslab, b->d_fb, b->d_queue, b->d_toff, b->d_soff, b->d_init, b->d_out};
  for (void* p : dev) if (p) (void)hipFree(p);
  for (int c = 0; c < T::kDim; ++c) {
    if (b->d_t[c]) (void)hipFree(b->d_t[c]);
    if (b->d_s[c]) (void)hipFree(b->d_s[c]);
  }
  if (b->h_fb_seen) (void)hipHostFree(b->h_fb_seen);
  for (typename T::Handle* f : b->fallback) T::destroy(f);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return NDT_OK;
}

// ndt*_batch_create_pyramid behind its checks of the levels
template <class Ctx>
int32_t batch_create_pyramid(const ndt2d_params* levels, int32_t n_levels, int32_t device_id, Ctx** out) {
  using T = BatchTraits<Ctx>;
  const int ndev = ndt_device_count();
  if (ndev <= 0) { set_error("no HIP device visible: this library has no CPU fallback"); return NDT_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return NDT_ERR_INVALID_ARG;
  Ctx* b = new (std::nothrow) Ctx();
  if (!b) return NDT_ERR_ALLOC;
  b->device = device_id;
  b->levels.assign(levels, levels + n_levels);
  b->global_blocks = T::kBlocksStart;
  auto fail = [&](int32_t code) { batch_destroy(b); return code; };
  if (hipSetDevice(device_id) != hipSuccess) return fail(NDT_ERR_HIP);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return fail(NDT_ERR_HIP);
  b->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return fail(NDT_ERR_HIP);
  if (hipMalloc((void**)&b->d_queue, 16) != hipSuccess) return fail(NDT_ERR_ALLOC);
  { const int32_t os = T::create_own(b); if (os != NDT_OK) return fail(os); }
  if (hipMalloc((void**)&b->d_gslab, (size_t)b->global_blocks * T::kSlabBytes) != hipSuccess) return fail(NDT_ERR_ALLOC);
  if (pinned_alloc(&b->h_fb_seen, 64) != hipSuccess) return fail(NDT_ERR_ALLOC);
  // more than 64 KiB of dynamic LDS needs an explicit opt-in per kernel
  for (const BatchVariant<typename T::Args>& v : T::variants())
    for (auto fn : v.fn)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, v.lds_bytes) != hipSuccess)
        return fail(NDT_ERR_HIP);
  *out = b;
  return NDT_OK;
}

template <class Ctx>
int32_t batch_set_tuning(Ctx* b, int32_t knob, int64_t value) {
  using T = BatchTraits<Ctx>;
  if (!b) return NDT_ERR_INVALID_ARG;
  const bool global = knob == NDT_TUNE_BATCH_GLOBAL_WORKGROUPS;
  if (global ? value < 1 || value > T::kBlocksMax : !T::own_knob(knob)) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (!global) { T::tune_own(b, knob, value); return NDT_OK; }
  if ((int)value != b->global_blocks) {                // one table slab per workgroup: re-allocate
    unsigned char* slab = nullptr;
    if (hipMalloc((void**)&slab, (size_t)value * T::kSlabBytes) != hipSuccess) { (void)hipGetLastError(); return NDT_ERR_ALLOC; }
    (void)hipFree(b->d_gslab);
    b->d_gslab = slab;
    b->global_blocks = (int)value;
  }
  b->global_pinned = true;                             // the caller's number stands: no growth on demand
  return NDT_OK;
}

template <class Ctx>
int32_t batch_wait_stream(Ctx* b, void* producer_stream) {
  if (!b) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(order_after(b->stream, (hipStream_t)producer_stream));
  return NDT_OK;
}

// t[c], s[c]: coordinate c of the concatenated target and source clouds
template <class Ctx>
int32_t batch_align_dev(Ctx* b, const float* const* d_t, const uint64_t* d_toff, const float* const* d_s, const uint64_t* d_soff,
                        const double* d_init, size_t n_pairs, typename BatchTraits<Ctx>::Result* d_results, void* stream) {
  if (!b || !d_toff || !d_soff || !d_init || !d_results) return NDT_ERR_INVALID_ARG;
  for (int c = 0; c < BatchTraits<Ctx>::kDim; ++c) if (!d_t[c] || !d_s[c]) return NDT_ERR_INVALID_ARG;
  if (n_pairs == 0 || n_pairs > 0x7fffffffull) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(b->device));
  return batch_launch(b, d_t, d_toff, d_s, d_soff, d_init, n_pairs, d_results, stream ? (hipStream_t)stream : b->stream);
}

template <class Ctx>
int32_t batch_align(Ctx* b, const float* const* t, const uint64_t* toff, const float* const* s, const uint64_t* soff,
                    const double* init, size_t n_pairs, typename BatchTraits<Ctx>::Result* results) {
  using T = BatchTraits<Ctx>;
  constexpr int D = T::kDim, P = T::kPose;
  if (!b || !toff || !soff || !init || !results || n_pairs == 0 || n_pairs > 0x7fffffffull) return NDT_ERR_INVALID_ARG;
  for (int c = 0; c < D; ++c) if (!t[c] || !s[c]) return NDT_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(b->device));
  if (!pair_offsets_ok(toff, soff, n_pairs, (uint64_t)kBatchMaxCloud)) return NDT_ERR_INVALID_ARG;
  const size_t nt = toff[n_pairs], ns = soff[n_pairs];
  hipStream_t st = b->stream;
  for (int c = 0; c < D; ++c) {
    HIP_TRY(grow(&b->d_t[c], &b->cap_t[c], nt, batch_slack(nt)));
    HIP_TRY(grow(&b->d_s[c], &b->cap_s[c], ns, batch_slack(ns)));
  }
  HIP_TRY(grow(&b->d_toff, &b->cap_toff, n_pairs + 1, batch_slack(n_pairs + 1)));
  HIP_TRY(grow(&b->d_soff, &b->cap_soff, n_pairs + 1, batch_slack(n_pairs + 1)));
  HIP_TRY(grow(&b->d_init, &b->cap_init, P * (n_pairs + 1), batch_slack(P * (n_pairs + 1))));
  HIP_TRY(grow(&b->d_out, &b->cap_out, n_pairs + 1, batch_slack(n_pairs + 1)));
  for (int c = 0; c < D; ++c) {
    HIP_TRY(hipMemcpyAsync(b->d_t[c], t[c], nt * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_s[c], s[c], ns * sizeof(float), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(b->d_toff, toff, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_soff, soff, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_init, init, P * n_pairs * sizeof(double), hipMemcpyHostToDevice, st));
  int32_t rc = batch_launch(b, b->d_t, b->d_toff, b->d_s, b->d_soff, b->d_init, n_pairs, b->d_out, st);
  if (rc != NDT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(results, b->d_out, n_pairs * sizeof(*results), hipMemcpyDeviceToHost, st));
  { const int32_t rs = T::read_back(b, n_pairs, st); if (rs != NDT_OK) return rs; }
  HIP_TRY(hipStreamSynchronize(st));
  T::host_done(b, n_pairs);
  // pairs no batch variant holds go level by level through the single-pair path
  for (size_t k = 0; k < n_pairs; ++k) {
    if (results[k].status != NDT_ERR_CAPACITY) continue;
    if (b->fallback.empty()) {
      for (const ndt2d_params& lp : b->levels) {
        typename T::Handle* f = nullptr;
        rc = T::create(&lp, b->device, &f);
        if (rc != NDT_OK) return rc;
        b->fallback.push_back(f);
      }
    }
    const float *tk[D], *sk[D];
    for (int c = 0; c < D; ++c) { tk[c] = t[c] + toff[k]; sk[c] = s[c] + soff[k]; }
    double pose[P];
    for (int j = 0; j < P; ++j) pose[j] = init[P * k + j];
    int total = 0;
    for (typename T::Handle* f : b->fallback) {
      rc = T::set_target(f, tk, toff[k + 1] - toff[k]);
      if (rc == NDT_OK) rc = T::align(f, sk, soff[k + 1] - soff[k], pose, &results[k]);
      if (rc < 0) break;
      total += results[k].iterations;
      results[k].iterations = total;
      if (results[k].status != NDT_OK && results[k].status != NDT_NOT_CONVERGED) break;
      for (int j = 0; j < P; ++j) pose[j] = results[k].pose[j];
    }
    if (rc < 0) return rc;
  }
  return NDT_OK;
}

// ---------------------------------------------------------------------------------------- the multi-device context

// Result-row buffers of the gather: d_send[d] holds `rows` rows on device d, d_recv[d] holds rows * n_devices.
// Grows to `want` rows by allocating EVERY new buffer first and swapping afterwards: a failed allocation leaves the
// old buffers, and the capacity that describes them, exactly as they were (a later call that fits them still works).
template <class Ctx, typename Row>
int32_t grow_gather_buffers(const std::vector<Ctx*>& ctx, std::vector<Row*>& d_send, std::vector<Row*>& d_recv,
                            size_t* cap, size_t want) {
  const int nd = static_cast<int>(ctx.size());
  std::vector<Row*> ns(nd, nullptr), nr(nd, nullptr);
  hipError_t err = hipSuccess;
  for (int d = 0; d < nd && err == hipSuccess; ++d) {
    err = hipSetDevice(ctx[d]->device);
    if (err == hipSuccess) err = hipMalloc((void**)&ns[d], want * sizeof(Row));
    if (err == hipSuccess) err = hipMalloc((void**)&nr[d], want * nd * sizeof(Row));
  }
  if (err == hipSuccess)
    for (int d = 0; d < nd && err == hipSuccess; ++d) {      // the old buffers may still be in use by the last call
      err = hipSetDevice(ctx[d]->device);
      if (err == hipSuccess) err = hipStreamSynchronize(ctx[d]->stream);
    }
  if (err != hipSuccess) {
    for (int d = 0; d < nd; ++d) {
      (void)hipSetDevice(ctx[d]->device);
      if (ns[d]) (void)hipFree(ns[d]);
      if (nr[d]) (void)hipFree(nr[d]);
    }
    last_error() = std::string("gather buffers: ") + hipGetErrorString(err);
    (void)hipGetLastError();
    return err == hipErrorOutOfMemory ? NDT_ERR_ALLOC : NDT_ERR_HIP;
  }
  d_send.resize(nd, nullptr);
  d_recv.resize(nd, nullptr);
  for (int d = 0; d < nd; ++d) {
    (void)hipSetDevice(ctx[d]->device);
    if (d_send[d]) (void)hipFree(d_send[d]);
    if (d_recv[d]) (void)hipFree(d_recv[d]);
    d_send[d] = ns[d];
    d_recv[d] = nr[d];
  }
  *cap = want;
  return NDT_OK;
}

inline int32_t require_rccl() {
  if (rccl().ok) return NDT_OK;
  set_error("librccl.so.1 could not be loaded: the device-resident multi-GPU gather needs RCCL (everything else does not)");
  return NDT_ERR_RCCL;
}

#define RCCL_TRY(expr)                                                                    \
  do {                                                                                    \
    const ncclResult_t _r = (expr);                                                       \
    if (_r != ncclSuccess) {                                                              \
      ::ndt::last_error() = std::string(#expr) + ": " + ndt::rccl().GetErrorString(_r);           \
      return NDT_ERR_RCCL;                                                                \
    }                                                                                     \
  } while (0)

template <class M>
int32_t multi_destroy(M* m) {
  if (!m) return NDT_OK;
  for (size_t d = 0; d < m->ctx.size(); ++d) {
    (void)hipSetDevice(m->ctx[d]->device);
    if (d < m->d_send.size() && m->d_send[d]) (void)hipFree(m->d_send[d]);
    if (d < m->d_recv.size() && m->d_recv[d]) (void)hipFree(m->d_recv[d]);
  }
  for (ncclComm_t c : m->comms) if (c && rccl().ok) (void)rccl().CommDestroy(c);
  for (auto* b : m->ctx) batch_destroy(b);
  delete m;
  return NDT_OK;
}

// One batch context per listed device (n_devices = 0: per visible device)
template <class M>
int32_t multi_create_pyramid(const ndt2d_params* levels, int32_t n_levels, const int32_t* device_ids,
                             int32_t n_devices, M** out) {
  using Ctx = typename M::Batch;
  if (!out) return NDT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!levels || n_levels < 1 || n_devices < 0 || (n_devices > 0 && !device_ids)) return NDT_ERR_INVALID_ARG;
  const int visible = ndt_device_count();
  if (visible <= 0) { set_error("no HIP device visible: this library has no CPU fallback"); return NDT_ERR_NO_DEVICE; }
  M* m = new (std::nothrow) M();
  if (!m) return NDT_ERR_ALLOC;
  m->iterations_hint = 0;
  for (int32_t i = 0; i < n_levels; ++i)
    m->iterations_hint += levels[i].fixed_iterations > 0 ? levels[i].fixed_iterations : 30;
  const int n = n_devices > 0 ? n_devices : visible;
  for (int i = 0; i < n; ++i) {
    Ctx* b = nullptr;
    const int32_t st = BatchTraits<Ctx>::create_context(levels, n_levels, n_devices > 0 ? device_ids[i] : i, &b);
    if (st != NDT_OK) { multi_destroy(m); return st; }
    m->ctx.push_back(b);
  }
  *out = m;
  return NDT_OK;
}

template <class Ctx>
int32_t multi_align(MultiContext<Ctx>* m, const float* const* t, const uint64_t* toff, const float* const* s, const uint64_t* soff,
                    const double* init, size_t n_pairs, typename BatchTraits<Ctx>::Result* results) {
  using T = BatchTraits<Ctx>;
  constexpr int D = T::kDim;
  if (!m || m->ctx.empty() || !toff || !soff || !init || !results || n_pairs == 0) return NDT_ERR_INVALID_ARG;
  for (int c = 0; c < D; ++c) if (!t[c] || !s[c]) return NDT_ERR_INVALID_ARG;
  const int nd = static_cast<int>(m->ctx.size());
  std::vector<uint64_t> begin(nd + 1);
  if (!plan_shards(nd, toff, soff, n_pairs, m->iterations_hint, nullptr, begin.data())) return NDT_ERR_INVALID_ARG;
  std::vector<int32_t> status(nd, NDT_OK);
  std::vector<std::string> message(nd);
  auto run = [&](int d) {
    const size_t k0 = begin[d], k1 = begin[d + 1];
    if (k1 == k0) return;
    std::vector<uint64_t> to(k1 - k0 + 1), so(k1 - k0 + 1);
    rebase_shard(toff, k0, k1, to.data());
    rebase_shard(soff, k0, k1, so.data());
    const float *td[D], *sd[D];
    for (int c = 0; c < D; ++c) { td[c] = t[c] + toff[k0]; sd[c] = s[c] + soff[k0]; }
    status[d] = batch_align(m->ctx[d], td, to.data(), sd, so.data(), init + T::kPose * k0, k1 - k0, results + k0);
    if (status[d] != NDT_OK) message[d] = ndt_last_error();   // last_error is per thread
  };
  std::vector<std::thread> workers;
  for (int d = 1; d < nd; ++d) workers.emplace_back(run, d);
  run(0);
  for (std::thread& w : workers) w.join();
  for (int d = 0; d < nd; ++d)
    if (status[d] != NDT_OK) { set_error(message[d].c_str()); return status[d]; }
  return NDT_OK;
}

// Device-resident form with the RCCL gather (BASELINE.json north_star: "shards scan pairs across the 8
// GPUs of one node with a final RCCL gather over xGMI").  One host thread enqueues everything: the
// batch kernels on every context's stream, then one grouped ncclAllGather of the padded result rows
// on the same streams - no host copy of a result, no host synchronisation between alignment and gather.
// d_t[c][d], d_s[c][d]: coordinate c of device d's clouds.
template <class Ctx>
int32_t multi_align_dev(MultiContext<Ctx>* m, const float* const* const* d_t, const uint64_t* const* d_toff,
                        const float* const* const* d_s, const uint64_t* const* d_soff, const double* const* d_init,
                        const size_t* n_pairs, typename BatchTraits<Ctx>::Result** d_results_all, size_t* shard_stride,
                        typename BatchTraits<Ctx>::Result* results) {
  using T = BatchTraits<Ctx>;
  using Row = typename T::Result;
  constexpr int D = T::kDim;
  if (!m || m->ctx.empty() || !d_toff || !d_soff || !d_init || !n_pairs) return NDT_ERR_INVALID_ARG;
  for (int c = 0; c < D; ++c) if (!d_t[c] || !d_s[c]) return NDT_ERR_INVALID_ARG;
  const int nd = static_cast<int>(m->ctx.size());
  for (int d = 0; d < nd; ++d) {
    if (n_pairs[d] > 0x7fffffffull) return NDT_ERR_INVALID_ARG;
    if (n_pairs[d] == 0) continue;
    if (!d_toff[d] || !d_soff[d] || !d_init[d]) return NDT_ERR_INVALID_ARG;
    for (int c = 0; c < D; ++c) if (!d_t[c][d] || !d_s[c][d]) return NDT_ERR_INVALID_ARG;
  }
  static_assert(sizeof(Row) % sizeof(double) == 0, "rows travel as doubles");
  // the gather moves `stride` rows per shard: the longest shard (padding rows are zero)
  const GatherLayout g = gather_layout(n_pairs, nd, sizeof(Row));
  if (g.total == 0) return NDT_ERR_INVALID_ARG;
  { const int32_t rs = require_rccl(); if (rs != NDT_OK) return rs; }
  if (m->comms.empty()) {
    // one communicator per context, all in this process (ncclCommInitAll); a device listed twice
    // cannot take part in a collective with itself
    std::vector<int> devs(nd);
    for (int d = 0; d < nd; ++d) {
      devs[d] = m->ctx[d]->device;
      for (int e = 0; e < d; ++e)
        if (devs[e] == devs[d]) { set_error("the RCCL gather needs distinct devices"); return NDT_ERR_INVALID_ARG; }
    }
    m->comms.assign(nd, nullptr);
    const ncclResult_t r = rccl().CommInitAll(m->comms.data(), nd, devs.data());
    if (r != ncclSuccess) {
      m->comms.clear();
      last_error() = std::string("ncclCommInitAll: ") + rccl().GetErrorString(r);
      return NDT_ERR_RCCL;
    }
  }
  if (g.stride > m->gather_cap) {
    const int32_t gs = grow_gather_buffers(m->ctx, m->d_send, m->d_recv, &m->gather_cap, g.stride + g.stride / 4 + 16);
    if (gs != NDT_OK) return gs;
  }
  for (int d = 0; d < nd; ++d) {
    HIP_TRY(hipSetDevice(m->ctx[d]->device));
    hipStream_t st = m->ctx[d]->stream;
    if (n_pairs[d] < g.stride)
      HIP_TRY(hipMemsetAsync(m->d_send[d] + n_pairs[d], 0, (g.stride - n_pairs[d]) * sizeof(Row), st));
    if (n_pairs[d] > 0) {
      const float *td[D], *sd[D];
      for (int c = 0; c < D; ++c) { td[c] = d_t[c][d]; sd[c] = d_s[c][d]; }
      const int32_t bs = batch_launch(m->ctx[d], td, d_toff[d], sd, d_soff[d], d_init[d], n_pairs[d], m->d_send[d], st);
      if (bs != NDT_OK) return bs;
    }
  }
  TraceRange range(T::kTraceGather);
  RCCL_TRY(rccl().GroupStart());
  for (int d = 0; d < nd; ++d) {
    const ncclResult_t r = rccl().AllGather(m->d_send[d], m->d_recv[d], g.count, ncclDouble, m->comms[d], m->ctx[d]->stream);
    if (r != ncclSuccess) {
      (void)rccl().GroupEnd();
      last_error() = std::string("ncclAllGather: ") + rccl().GetErrorString(r);
      return NDT_ERR_RCCL;
    }
  }
  RCCL_TRY(rccl().GroupEnd());
  if (results) {     // global pair order, padding dropped, from the first device's copy of the gather
    HIP_TRY(hipSetDevice(m->ctx[0]->device));
    const hipError_t read_back = ungather(n_pairs, nd, g.stride, hipSuccess, [&](size_t to, size_t from, size_t rows) {
      return hipMemcpyAsync(results + to, m->d_recv[0] + from, rows * sizeof(Row), hipMemcpyDeviceToHost, m->ctx[0]->stream);
    });
    HIP_TRY(read_back);
  }
  for (int d = 0; d < nd; ++d) {
    HIP_TRY(hipSetDevice(m->ctx[d]->device));
    HIP_TRY(hipStreamSynchronize(m->ctx[d]->stream));
    if (d_results_all) d_results_all[d] = m->d_recv[d];
  }
  if (shard_stride) *shard_stride = g.stride;
  return NDT_OK;
}

}  // namespace

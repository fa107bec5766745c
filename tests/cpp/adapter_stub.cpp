// A recording stand-in for libndt_hip.so, for tests/cpp/adapter_calls_main.cpp (tests/test_adapter_calls.py): exactly the
// extern "C" entry points that include/ndt_matcher_hip.hpp names - one the header names and this file lacks fails the link.
// Every stand-in prints one line "  C name arg ... -> status" (no status where the entry point returns none) and, when it
// returns NDT_OK, fills its outputs with values that differ per call (by the call's number within the section), per row
// and per field.
//   scalars                     by value
//   handles                     as the value ndt*_create handed out (h0x100, h0x200, ...)
//   pointers passed through     @offset into the arena the driver registered, `null`, or `local` (the adapter's own memory)
//   arrays the adapter packs    by their contents, at the length the C contract gives them: [a b c]
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "ndt_hip.h"

// ---- control (not part of the ABI; declared again in the driver) ---------------------------------------------------
extern "C" void stub_arena(const void* base, size_t bytes);
extern "C" void stub_mode(int mode);              // 0: NDT_OK; 1: every call fails; 2: every call but ndt*_wait_stream fails
extern "C" void stub_section(const char* title);  // prints the header, restarts the call numbers

namespace {
const char* g_base = nullptr;
size_t g_bytes = 0;
int g_mode = 0, g_c = 0;
uintptr_t g_handles = 0;
constexpr int kDevices = 2;                       // what ndt*_multi_device_count answers

void put(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
}

struct Hnd { const void* p; };                    // a handle, batch or multi context
struct Vals { const double* p; size_t n; };       // doubles the adapter packed
struct U64s { const uint64_t* p; size_t n; };
struct F32s { const float* p; size_t n; };
struct I32s { const int32_t* p; int n; };
struct Ptrs { const void* const* p; size_t n; };  // a table of pass-through pointers
struct Hnds { const void* const* p; size_t n; };  // a table of handles
struct Prm { const ndt2d_params* p; int n; };

template <class T> Hnd H(T* h) { return Hnd{h}; }
template <class T> Ptrs PT(T* const* p, size_t n) { return Ptrs{reinterpret_cast<const void* const*>(p), n}; }

void ptr(const void* p) {
  const char* c = static_cast<const char*>(p);
  if (!p) put(" null");
  else if (g_base && c >= g_base && c < g_base + g_bytes) put(" @%zu", static_cast<size_t>(c - g_base));
  else put(" local");
}
void arg(const void* p) { ptr(p); }
void arg(Hnd h) { if (h.p) put(" h%#zx", reinterpret_cast<size_t>(h.p)); else put(" hnull"); }
void arg(int v) { put(" %d", v); }
void arg(unsigned v) { put(" %u", v); }
void arg(long v) { put(" %ld", v); }
void arg(unsigned long v) { put(" %lu", v); }
void arg(float v) { put(" %.9g", static_cast<double>(v)); }
void arg(double v) { put(" %.17g", v); }
void arg(Vals v) {
  if (!v.p) { put(" null"); return; }
  for (size_t i = 0; i < v.n; ++i) put("%s%.17g", i ? " " : " [", v.p[i]);
  put(v.n ? "]" : " []");
}
void arg(U64s v) {
  for (size_t i = 0; i < v.n; ++i) put("%s%lu", i ? " " : " [", static_cast<unsigned long>(v.p[i]));
  put(v.n ? "]" : " []");
}
void arg(F32s v) {
  for (size_t i = 0; i < v.n; ++i) put("%s%.9g", i ? " " : " [", static_cast<double>(v.p[i]));
  put(v.n ? "]" : " []");
}
void arg(I32s v) {
  if (!v.p) { put(" null"); return; }
  for (int i = 0; i < v.n; ++i) put("%s%d", i ? " " : " [", v.p[i]);
  put(v.n ? "]" : " []");
}
void arg(Ptrs v) {
  put(" [");
  for (size_t i = 0; i < v.n; ++i) ptr(v.p[i]);
  put(" ]");
}
void arg(Hnds v) {
  put(" [");
  for (size_t i = 0; i < v.n; ++i) arg(Hnd{v.p[i]});
  put(" ]");
}
void arg(Prm v) {
  if (!v.p) { put(" null"); return; }
  for (int i = 0; i < v.n; ++i) {
    const ndt2d_params& p = v.p[i];
    put(" {%.17g %d %d %.17g %.17g %.17g %d %d %.17g %.17g %.17g %.17g %d %d %d %.17g}", p.cell_size, p.min_points,
        p.hessian_mode, p.eig_ratio, p.d1, p.d2, p.max_iterations, p.fixed_iterations, p.eps_trans, p.eps_rot,
        p.step_max_trans, p.step_max_rot, p.min_hits, p.overlap_grids, p.line_search, p.step_scale);
  }
  if (v.n == 0) put(" {}");
}
void arg(const ndt2d_search_window* w) { ptr(w); }
void arg(const ndt3d_search_window* w) { ptr(w); }

int32_t status_of(const char* name) {
  const size_t n = strlen(name);
  const bool wait = n >= 11 && strcmp(name + n - 11, "wait_stream") == 0;
  return g_mode == 0 || (g_mode == 2 && wait) ? NDT_OK : NDT_ERR_INVALID_ARG;
}

// prints the call, returns its status
template <class... A>
int32_t call(const char* name, A... a) {
  ++g_c;
  put("  C %s", name);
  (arg(a), ...);
  const int32_t st = status_of(name);
  put(" -> %d\n", st);
  return st;
}
// the same for an entry point that returns no status
template <class... A>
void seen(const char* name, A... a) {
  ++g_c;
  put("  C %s", name);
  (arg(a), ...);
  put("\n");
}

// ---- outputs -------------------------------------------------------------------------------------------------------
template <int N, class R>
void fill_result(R* r, int i) {
  const double id = 10.0 * g_c + i;
  for (int j = 0; j < N; ++j) { r->pose[j] = id + 0.01 * (j + 1); r->g[j] = -(id + j); }
  for (int a = 0; a < N; ++a)
    for (int b = 0; b < N; ++b) r->H[N * a + b] = (a == b ? 50.0 + a : 0.0) + 0.01 * (N * a + b) + 0.001 * id;
  r->score = 100.0 * g_c + i + 0.5;
  r->iterations = 3 + g_c + i;
  r->n_hit = 40 + g_c + i;
  r->status = i == 1 ? NDT_NOT_CONVERGED : NDT_OK;
  r->reserved = 0;
}
template <int N, class E>
void fill_eval(E* e) {
  for (int j = 0; j < N * N; ++j) e->H[j] = 7.0 + g_c + 0.01 * j;
  for (int j = 0; j < N; ++j) e->g[j] = -(1.0 + g_c + 0.1 * j);
  e->score = 200.0 + g_c;
  e->n_hit = 60 + g_c;
  e->reserved = 0;
}
template <int N, class Hit>
void fill_hit(Hit* h, int i) {
  const double id = 10.0 * g_c + i;
  for (int j = 0; j < N; ++j) h->pose[j] = -(id + 0.01 * (j + 1));
  h->score = 0.25f * (i + 1) + g_c;
  h->index = 7 * g_c + i;
}
int n_hits_of(int32_t k) { return k < 0 ? 0 : (k < 2 ? k : 2); }
template <int N, class Hit, class R>
void fill_hits(int32_t k, Hit* hits, R* results, int32_t* n_hits) {
  *n_hits = k < 2 ? k : 2;                                      // min(k, 2), as it stands for k <= 0 too
  for (int i = 0; i < n_hits_of(k); ++i) {
    fill_hit<N>(hits + i, i);
    if (results) fill_result<N>(results + i, i);
  }
}
void fill_fit(ndt_point_fit* f) {
  f->n_invalid = 1 + g_c; f->n_miss = 20 + g_c; f->n_misfit = 300 + g_c; f->n_fit = 4000 + g_c; f->n_selected = 50000 + g_c;
}
void fill_info(ndt_voxel_filter_info* v) { v->n_invalid = 2 + g_c; v->n_voxels = 30 + g_c; v->n_out = 400 + g_c; }
template <class T>
int32_t create(int32_t st, T** out) {
  if (st == NDT_OK) { g_handles += 0x100; *out = reinterpret_cast<T*>(g_handles); }
  return st;
}
int32_t outside(int32_t st, size_t* n_outside) {
  if (st == NDT_OK) *n_outside = 1000 + g_c;
  return st;
}
void default_params(ndt2d_params* p, int dim) {
  *p = ndt2d_params{0.5 * dim, 2 + dim, NDT_HESSIAN_NEWTON, 0.01 * dim, 1.0 + dim, 0.5 + dim, 20 + dim, 0, 1e-4 * dim,
                    1e-5 * dim, 0.25 * dim, 0.1 * dim, 5 + dim, 1, 0, 0, 1.0};
}
}  // namespace

extern "C" {
void stub_arena(const void* base, size_t bytes) { g_base = static_cast<const char*>(base); g_bytes = bytes; }
void stub_mode(int mode) { g_mode = mode; }
void stub_section(const char* title) { g_c = 0; put("== %s\n", title); }

const char* ndt_last_error(void) { return "stub"; }
const char* ndt_status_string(int32_t status) { return status == NDT_ERR_INVALID_ARG ? "invalid argument" : "status"; }

int32_t ndt2d_calibrated_covariance(const double Hm[9], int32_t hessian_mode, double cov[9]) {
  const int32_t st = call("ndt2d_calibrated_covariance", Vals{Hm, 9}, hessian_mode, static_cast<const void*>(cov));
  if (st == NDT_OK) for (int i = 0; i < 9; ++i) cov[i] = Hm[i] + hessian_mode;
  return st;
}

// ---- life cycle, grid, maps ----------------------------------------------------------------------------------------
void ndt2d_default_params(ndt2d_params* p) { seen("ndt2d_default_params", static_cast<const void*>(p)); default_params(p, 2); }
void ndt3d_default_params(ndt3d_params* p) { seen("ndt3d_default_params", static_cast<const void*>(p)); default_params(p, 3); }
int32_t ndt2d_default_pyramid(const ndt2d_params* fine, ndt2d_params levels[3]) {
  const int32_t st = call("ndt2d_default_pyramid", Prm{fine, 1}, static_cast<const void*>(levels));
  if (st == NDT_OK) for (int i = 0; i < 3; ++i) { levels[i] = *fine; levels[i].cell_size = fine->cell_size * (4 >> i); }
  return st;
}
int32_t ndt2d_create(const ndt2d_params* p, int32_t device_id, ndt2d_handle** out) {
  return create(call("ndt2d_create", Prm{p, 1}, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt3d_create(const ndt3d_params* p, int32_t device_id, ndt3d_handle** out) {
  return create(call("ndt3d_create", Prm{p, 1}, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt2d_destroy(ndt2d_handle* h) { return call("ndt2d_destroy", H(h)); }
int32_t ndt3d_destroy(ndt3d_handle* h) { return call("ndt3d_destroy", H(h)); }
void* ndt2d_stream(ndt2d_handle* h) { seen("ndt2d_stream", H(h)); return reinterpret_cast<char*>(h) + 0x5000; }
void* ndt3d_stream(ndt3d_handle* h) { seen("ndt3d_stream", H(h)); return reinterpret_cast<char*>(h) + 0x6000; }
int32_t ndt2d_wait_stream(ndt2d_handle* h, void* producer_stream) { return call("ndt2d_wait_stream", H(h), producer_stream); }
int32_t ndt3d_wait_stream(ndt3d_handle* h, void* producer_stream) { return call("ndt3d_wait_stream", H(h), producer_stream); }
int32_t ndt3d_set_tuning(ndt3d_handle* h, int32_t knob, int64_t value) { return call("ndt3d_set_tuning", H(h), knob, value); }
int32_t ndt3d_set_neighbourhood(ndt3d_handle* h, int32_t n) { return call("ndt3d_set_neighbourhood", H(h), n); }
int32_t ndt3d_neighbourhood(const ndt3d_handle* h) { seen("ndt3d_neighbourhood", H(h)); return 7; }

int32_t ndt2d_set_target(ndt2d_handle* h, const float* x, const float* y, size_t n) { return call("ndt2d_set_target", H(h), x, y, n); }
int32_t ndt3d_set_target(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n) {
  return call("ndt3d_set_target", H(h), x, y, z, n);
}
int32_t ndt2d_reserve_target(ndt2d_handle* h, double xmin, double ymin, double xmax, double ymax) {
  return call("ndt2d_reserve_target", H(h), xmin, ymin, xmax, ymax);
}
int32_t ndt3d_reserve_target(ndt3d_handle* h, const double lo[3], const double hi[3]) {
  return call("ndt3d_reserve_target", H(h), Vals{lo, 3}, Vals{hi, 3});
}
int32_t ndt2d_add_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n, size_t* n_outside) {
  return outside(call("ndt2d_add_target_points", H(h), x, y, n, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt3d_add_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, size_t* n_outside) {
  return outside(call("ndt3d_add_target_points", H(h), x, y, z, n, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt2d_remove_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n, size_t* n_outside) {
  return outside(call("ndt2d_remove_target_points", H(h), x, y, n, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt3d_remove_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, size_t* n_outside) {
  return outside(call("ndt3d_remove_target_points", H(h), x, y, z, n, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt2d_add_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, const double pose[3],
                                    size_t* n_outside, void* stream) {
  return outside(call("ndt2d_add_target_points_dev", H(h), d_x, d_y, n, Vals{pose, 3}, static_cast<const void*>(n_outside), stream), n_outside);
}
int32_t ndt3d_add_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                    const double pose[6], size_t* n_outside, void* stream) {
  return outside(call("ndt3d_add_target_points_dev", H(h), d_x, d_y, d_z, n, Vals{pose, 6}, static_cast<const void*>(n_outside), stream), n_outside);
}
int32_t ndt2d_remove_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, const double pose[3],
                                       size_t* n_outside, void* stream) {
  return outside(call("ndt2d_remove_target_points_dev", H(h), d_x, d_y, n, Vals{pose, 3}, static_cast<const void*>(n_outside), stream), n_outside);
}
int32_t ndt3d_remove_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                       const double pose[6], size_t* n_outside, void* stream) {
  return outside(call("ndt3d_remove_target_points_dev", H(h), d_x, d_y, d_z, n, Vals{pose, 6}, static_cast<const void*>(n_outside), stream), n_outside);
}
int32_t ndt2d_get_grid_info(ndt2d_handle* h, ndt2d_grid_info* info) {
  const int32_t st = call("ndt2d_get_grid_info", H(h), static_cast<const void*>(info));
  if (st == NDT_OK) *info = ndt2d_grid_info{-1.5f, -2.5f, 4.0f, 0.25f, 11, 12, 13, 14};
  return st;
}
int32_t ndt3d_get_grid_info(ndt3d_handle* h, ndt3d_grid_info* info) {
  const int32_t st = call("ndt3d_get_grid_info", H(h), static_cast<const void*>(info));
  if (st == NDT_OK) *info = ndt3d_grid_info{-1.5f, -2.5f, -3.5f, 2.0f, 21, 22, 23, 24};
  return st;
}
size_t ndt2d_map_size(const ndt2d_handle* h) { seen("ndt2d_map_size", H(h)); return 6; }
size_t ndt3d_map_size(const ndt3d_handle* h) { seen("ndt3d_map_size", H(h)); return 7; }
static int32_t save(int32_t st, void* buf, size_t capacity, int first) {
  if (st == NDT_OK) for (size_t i = 0; i < capacity; ++i) static_cast<unsigned char*>(buf)[i] = static_cast<unsigned char>(first + i);
  return st;
}
int32_t ndt2d_save_map(ndt2d_handle* h, void* buf, size_t capacity, size_t* written) {
  return save(call("ndt2d_save_map", H(h), static_cast<const void*>(buf), capacity, static_cast<const void*>(written)), buf, capacity, 20);
}
int32_t ndt3d_save_map(ndt3d_handle* h, void* buf, size_t capacity, size_t* written) {
  return save(call("ndt3d_save_map", H(h), static_cast<const void*>(buf), capacity, static_cast<const void*>(written)), buf, capacity, 30);
}
int32_t ndt2d_load_map(ndt2d_handle* h, const void* buf, size_t bytes) { return call("ndt2d_load_map", H(h), buf, bytes); }
int32_t ndt3d_load_map(ndt3d_handle* h, const void* buf, size_t bytes) { return call("ndt3d_load_map", H(h), buf, bytes); }
int32_t ndt2d_coarsen_map(ndt2d_handle* src, ndt2d_handle* dst) { return call("ndt2d_coarsen_map", H(src), H(dst)); }
int32_t ndt3d_coarsen_map(ndt3d_handle* src, ndt3d_handle* dst) { return call("ndt3d_coarsen_map", H(src), H(dst)); }
int32_t ndt2d_merge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside) {
  return outside(call("ndt2d_merge_map", H(dst), H(src), Vals{pose, 3}, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt3d_merge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside) {
  return outside(call("ndt3d_merge_map", H(dst), H(src), Vals{pose, 6}, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt2d_unmerge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside) {
  return outside(call("ndt2d_unmerge_map", H(dst), H(src), Vals{pose, 3}, static_cast<const void*>(n_outside)), n_outside);
}
int32_t ndt3d_unmerge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside) {
  return outside(call("ndt3d_unmerge_map", H(dst), H(src), Vals{pose, 6}, static_cast<const void*>(n_outside)), n_outside);
}

// ---- alignment of scans --------------------------------------------------------------------------------------------
int32_t ndt2d_align(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double init_pose[3], ndt2d_result* out) {
  const int32_t st = call("ndt2d_align", H(h), sx, sy, n, Vals{init_pose, 3}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<3>(out, 0);
  return st;
}
int32_t ndt3d_align(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const double init_pose[6],
                    ndt3d_result* out) {
  const int32_t st = call("ndt3d_align", H(h), sx, sy, sz, n, Vals{init_pose, 6}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<6>(out, 0);
  return st;
}
int32_t ndt2d_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double init_pose[3], ndt2d_result* out) {
  const int32_t st = call("ndt2d_align_dev", H(h), d_sx, d_sy, n, Vals{init_pose, 3}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<3>(out, 0);
  return st;
}
int32_t ndt3d_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                        const double init_pose[6], ndt3d_result* out) {
  const int32_t st = call("ndt3d_align_dev", H(h), d_sx, d_sy, d_sz, n, Vals{init_pose, 6}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<6>(out, 0);
  return st;
}
int32_t ndt2d_align_multi_start_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* init_poses,
                                    int32_t m, ndt2d_result* results) {
  const int32_t st = call("ndt2d_align_multi_start_dev", H(h), d_sx, d_sy, n, Vals{init_poses, 3 * static_cast<size_t>(m)}, m,
                          static_cast<const void*>(results));
  if (st == NDT_OK) for (int i = 0; i < m; ++i) fill_result<3>(results + i, i);
  return st;
}
int32_t ndt2d_align_multi_scan_dev(ndt2d_handle* h, const float* const* d_sx, const float* const* d_sy, const size_t* n,
                                   const double* init_poses, int32_t m, ndt2d_result* results) {
  const size_t um = static_cast<size_t>(m);
  const int32_t st = call("ndt2d_align_multi_scan_dev", H(h), PT(d_sx, um), PT(d_sy, um),
                          U64s{reinterpret_cast<const uint64_t*>(n), um}, Vals{init_poses, 3 * um}, m, static_cast<const void*>(results));
  if (st == NDT_OK) for (int i = 0; i < m; ++i) fill_result<3>(results + i, i);
  return st;
}
int32_t ndt3d_align_multi_scan_dev(ndt3d_handle* h, const float* const* d_sx, const float* const* d_sy, const float* const* d_sz,
                                   const size_t* n, const double* init_poses, int32_t m, ndt3d_result* results) {
  const size_t um = static_cast<size_t>(m);
  const int32_t st = call("ndt3d_align_multi_scan_dev", H(h), PT(d_sx, um), PT(d_sy, um), PT(d_sz, um),
                          U64s{reinterpret_cast<const uint64_t*>(n), um}, Vals{init_poses, 6 * um}, m, static_cast<const void*>(results));
  if (st == NDT_OK) for (int i = 0; i < m; ++i) fill_result<6>(results + i, i);
  return st;
}
int32_t ndt2d_evaluate(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double pose[3], ndt2d_eval* out) {
  const int32_t st = call("ndt2d_evaluate", H(h), sx, sy, n, Vals{pose, 3}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_eval<3>(out);
  return st;
}

// ---- searches, pose lists, particles -------------------------------------------------------------------------------
int32_t ndt2d_search_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w, int32_t k,
                         ndt2d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt2d_search_dev", H(h), d_sx, d_sy, n, w, k, static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, static_cast<ndt2d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt3d_search_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                         const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt3d_search_dev", H(h), d_sx, d_sy, d_sz, n, w, k, static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, static_cast<ndt3d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt2d_search_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const ndt2d_search_window* w,
                               int32_t k, ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt2d_search_align_dev", H(h), d_sx, d_sy, n, w, k, static_cast<const void*>(hits),
                          static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, results, n_hits);
  return st;
}
int32_t ndt3d_search_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                               const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, ndt3d_result* results,
                               int32_t* n_hits) {
  const int32_t st = call("ndt3d_search_align_dev", H(h), d_sx, d_sy, d_sz, n, w, k, static_cast<const void*>(hits),
                          static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, results, n_hits);
  return st;
}
int32_t ndt2d_score_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                              float* d_scores) {
  return call("ndt2d_score_poses_dev", H(h), d_sx, d_sy, n, d_poses, m, d_scores);
}
int32_t ndt3d_score_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                              const double* d_poses, size_t m, float* d_scores) {
  return call("ndt3d_score_poses_dev", H(h), d_sx, d_sy, d_sz, n, d_poses, m, d_scores);
}
int32_t ndt2d_score_particles_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                                  float* d_scores, uint32_t* d_n_hit) {
  return call("ndt2d_score_particles_dev", H(h), d_sx, d_sy, n, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt3d_score_particles_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                  const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  return call("ndt3d_score_particles_dev", H(h), d_sx, d_sy, d_sz, n, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt2d_score_particles_async(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses,
                                    size_t m, float* d_scores, uint32_t* d_n_hit) {
  return call("ndt2d_score_particles_async", H(h), d_sx, d_sy, n, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt3d_score_particles_async(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                    const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit) {
  return call("ndt3d_score_particles_async", H(h), d_sx, d_sy, d_sz, n, d_poses, m, d_scores, d_n_hit);
}
int32_t ndt2d_score_particles(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double* poses, size_t m,
                              float* scores, uint32_t* n_hit) {
  return call("ndt2d_score_particles", H(h), sx, sy, n, poses, m, scores, n_hit);
}
int32_t ndt3d_score_particles(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n, const double* poses,
                              size_t m, float* scores, uint32_t* n_hit) {
  return call("ndt3d_score_particles", H(h), sx, sy, sz, n, poses, m, scores, n_hit);
}
int32_t ndt2d_best_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses, size_t m,
                             double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt2d_best_poses_dev", H(h), d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, static_cast<ndt2d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt3d_best_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                             const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                             ndt3d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt3d_best_poses_dev", H(h), d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, static_cast<ndt3d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt2d_best_poses_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses,
                                   size_t m, double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                   ndt2d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt2d_best_poses_align_dev", H(h), d_sx, d_sy, n, d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, results, n_hits);
  return st;
}
int32_t ndt3d_best_poses_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                   const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                                   ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt3d_best_poses_align_dev", H(h), d_sx, d_sy, d_sz, n, d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, results, n_hits);
  return st;
}

// ---- the driver side of the boundary, point fits, the voxel filter ---------------------------------------------------
int32_t ndt2d_polar_to_points_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc, double range_min,
                                  double range_max, float* d_x, float* d_y, void* stream) {
  return call("ndt2d_polar_to_points_dev", d_ranges, n, angle_min, angle_inc, range_min, range_max, d_x, d_y, stream);
}
int32_t ndt2d_polar_to_points_deskew_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc, double range_min,
                                         double range_max, const double delta[3], double frac0, double frac_inc, double ref_frac,
                                         float* d_x, float* d_y, void* stream) {
  return call("ndt2d_polar_to_points_deskew_dev", d_ranges, n, angle_min, angle_inc, range_min, range_max, Vals{delta, 3}, frac0,
              frac_inc, ref_frac, d_x, d_y, stream);
}
int32_t ndt3d_range_image_to_points_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim, const double* elevations,
                                        double azimuth0, double azimuth_inc, double range_min, double range_max, float* d_x,
                                        float* d_y, float* d_z, void* stream) {
  return call("ndt3d_range_image_to_points_dev", d_ranges, n_elev, n_azim, elevations, azimuth0, azimuth_inc, range_min, range_max,
              d_x, d_y, d_z, stream);
}
int32_t ndt3d_range_image_to_points_deskew_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim, const double* elevations,
                                               double azimuth0, double azimuth_inc, double range_min, double range_max,
                                               const double delta[6], double frac0, double frac_inc, double ref_frac, float* d_x,
                                               float* d_y, float* d_z, void* stream) {
  return call("ndt3d_range_image_to_points_deskew_dev", d_ranges, n_elev, n_azim, elevations, azimuth0, azimuth_inc, range_min,
              range_max, Vals{delta, 6}, frac0, frac_inc, ref_frac, d_x, d_y, d_z, stream);
}
int32_t ndt2d_sweep_motion(const double prev[3], const double cur[3], double delta[3]) {
  const int32_t st = call("ndt2d_sweep_motion", Vals{prev, 3}, Vals{cur, 3}, static_cast<const void*>(delta));
  if (st == NDT_OK) for (int j = 0; j < 3; ++j) delta[j] = 0.5 + j;
  return st;
}
int32_t ndt3d_sweep_motion(const double prev[6], const double cur[6], double delta[6]) {
  const int32_t st = call("ndt3d_sweep_motion", Vals{prev, 6}, Vals{cur, 6}, static_cast<const void*>(delta));
  if (st == NDT_OK) for (int j = 0; j < 6; ++j) delta[j] = 0.5 + j;
  return st;
}
int32_t ndt2d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_frac, size_t n, const double delta[3],
                                double ref_frac, float* d_ox, float* d_oy, void* stream) {
  return call("ndt2d_deskew_points_dev", d_x, d_y, d_frac, n, Vals{delta, 3}, ref_frac, d_ox, d_oy, stream);
}
int32_t ndt3d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_z, const float* d_frac, size_t n,
                                const double delta[6], double ref_frac, float* d_ox, float* d_oy, float* d_oz, void* stream) {
  return call("ndt3d_deskew_points_dev", d_x, d_y, d_z, d_frac, n, Vals{delta, 6}, ref_frac, d_ox, d_oy, d_oz, stream);
}
int32_t ndt2d_fit_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3], float max_m,
                             float* d_m, uint8_t* d_class, ndt_point_fit* fit) {
  const int32_t st = call("ndt2d_fit_points_dev", H(h), d_sx, d_sy, n, Vals{pose, 3}, max_m, d_m, d_class, static_cast<const void*>(fit));
  if (st == NDT_OK) fill_fit(fit);
  return st;
}
int32_t ndt3d_fit_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                             const double pose[6], float max_m, float* d_m, uint8_t* d_class, ndt_point_fit* fit) {
  const int32_t st = call("ndt3d_fit_points_dev", H(h), d_sx, d_sy, d_sz, n, Vals{pose, 6}, max_m, d_m, d_class, static_cast<const void*>(fit));
  if (st == NDT_OK) fill_fit(fit);
  return st;
}
int32_t ndt2d_select_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3], float max_m,
                                uint32_t keep, float* d_ox, float* d_oy, uint32_t* d_index, ndt_point_fit* fit) {
  const int32_t st = call("ndt2d_select_points_dev", H(h), d_sx, d_sy, n, Vals{pose, 3}, max_m, keep, d_ox, d_oy, d_index,
                          static_cast<const void*>(fit));
  if (st == NDT_OK) fill_fit(fit);
  return st;
}
int32_t ndt3d_select_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                const double pose[6], float max_m, uint32_t keep, float* d_ox, float* d_oy, float* d_oz,
                                uint32_t* d_index, ndt_point_fit* fit) {
  const int32_t st = call("ndt3d_select_points_dev", H(h), d_sx, d_sy, d_sz, n, Vals{pose, 6}, max_m, keep, d_ox, d_oy, d_oz, d_index,
                          static_cast<const void*>(fit));
  if (st == NDT_OK) fill_fit(fit);
  return st;
}
int32_t ndt2d_voxel_filter_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, double leaf, uint32_t min_points,
                               float* d_ox, float* d_oy, uint32_t* d_count, size_t capacity, ndt_voxel_filter_info* info) {
  const int32_t st = call("ndt2d_voxel_filter_dev", H(h), d_x, d_y, n, leaf, min_points, d_ox, d_oy, d_count, capacity,
                          static_cast<const void*>(info));
  if (st == NDT_OK) fill_info(info);
  return st;
}
int32_t ndt3d_voxel_filter_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n, double leaf,
                               uint32_t min_points, float* d_ox, float* d_oy, float* d_oz, uint32_t* d_count, size_t capacity,
                               ndt_voxel_filter_info* info) {
  const int32_t st = call("ndt3d_voxel_filter_dev", H(h), d_x, d_y, d_z, n, leaf, min_points, d_ox, d_oy, d_oz, d_count, capacity,
                          static_cast<const void*>(info));
  if (st == NDT_OK) fill_info(info);
  return st;
}

// ---- map to map ------------------------------------------------------------------------------------------------------
int32_t ndt2d_align_map(ndt2d_handle* target, ndt2d_handle* source, const double init_pose[3], ndt2d_result* out) {
  const int32_t st = call("ndt2d_align_map", H(target), H(source), Vals{init_pose, 3}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<3>(out, 0);
  return st;
}
int32_t ndt3d_align_map(ndt3d_handle* target, ndt3d_handle* source, const double init_pose[6], ndt3d_result* out) {
  const int32_t st = call("ndt3d_align_map", H(target), H(source), Vals{init_pose, 6}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_result<6>(out, 0);
  return st;
}
int32_t ndt2d_align_map_multi(ndt2d_handle* target, ndt2d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt2d_result* results) {
  const size_t um = static_cast<size_t>(m);
  const int32_t st = call("ndt2d_align_map_multi", H(target), Hnds{reinterpret_cast<const void* const*>(sources), um},
                          Vals{init_poses, 3 * um}, m, static_cast<const void*>(results));
  if (st == NDT_OK) for (int i = 0; i < m; ++i) fill_result<3>(results + i, i);
  return st;
}
int32_t ndt3d_align_map_multi(ndt3d_handle* target, ndt3d_handle* const* sources, const double* init_poses, int32_t m,
                              ndt3d_result* results) {
  const size_t um = static_cast<size_t>(m);
  const int32_t st = call("ndt3d_align_map_multi", H(target), Hnds{reinterpret_cast<const void* const*>(sources), um},
                          Vals{init_poses, 6 * um}, m, static_cast<const void*>(results));
  if (st == NDT_OK) for (int i = 0; i < m; ++i) fill_result<6>(results + i, i);
  return st;
}
int32_t ndt2d_evaluate_map(ndt2d_handle* target, ndt2d_handle* source, const double pose[3], ndt2d_eval* out) {
  const int32_t st = call("ndt2d_evaluate_map", H(target), H(source), Vals{pose, 3}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_eval<3>(out);
  return st;
}
int32_t ndt3d_evaluate_map(ndt3d_handle* target, ndt3d_handle* source, const double pose[6], ndt3d_eval* out) {
  const int32_t st = call("ndt3d_evaluate_map", H(target), H(source), Vals{pose, 6}, static_cast<const void*>(out));
  if (st == NDT_OK) fill_eval<6>(out);
  return st;
}
int32_t ndt2d_search_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, int32_t k,
                         ndt2d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt2d_search_map", H(target), H(source), w, k, static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, static_cast<ndt2d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt3d_search_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, int32_t k,
                         ndt3d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt3d_search_map", H(target), H(source), w, k, static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, static_cast<ndt3d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt2d_search_map_scores(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, float* d_scores) {
  return call("ndt2d_search_map_scores", H(target), H(source), w, d_scores);
}
int32_t ndt3d_search_map_scores(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, float* d_scores) {
  return call("ndt3d_search_map_scores", H(target), H(source), w, d_scores);
}
int32_t ndt2d_search_align_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w, int32_t k,
                               ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt2d_search_align_map", H(target), H(source), w, k, static_cast<const void*>(hits),
                          static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, results, n_hits);
  return st;
}
int32_t ndt3d_search_align_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w, int32_t k,
                               ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt3d_search_align_map", H(target), H(source), w, k, static_cast<const void*>(hits),
                          static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, results, n_hits);
  return st;
}
int32_t ndt2d_score_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m, float* d_scores,
                                  uint32_t* d_n_hit) {
  return call("ndt2d_score_map_poses_dev", H(target), H(source), d_poses, m, d_scores, d_n_hit);
}
int32_t ndt3d_score_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m, float* d_scores,
                                  uint32_t* d_n_hit) {
  return call("ndt3d_score_map_poses_dev", H(target), H(source), d_poses, m, d_scores, d_n_hit);
}
int32_t ndt2d_best_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m, double min_sep_trans,
                                 double min_sep_rot, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt2d_best_map_poses_dev", H(target), H(source), d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, static_cast<ndt2d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt3d_best_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m, double min_sep_trans,
                                 double min_sep_rot, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits) {
  const int32_t st = call("ndt3d_best_map_poses_dev", H(target), H(source), d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, static_cast<ndt3d_result*>(nullptr), n_hits);
  return st;
}
int32_t ndt2d_best_map_poses_align_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                       ndt2d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt2d_best_map_poses_align_dev", H(target), H(source), d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<3>(k, hits, results, n_hits);
  return st;
}
int32_t ndt3d_best_map_poses_align_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt3d_search_hit* hits,
                                       ndt3d_result* results, int32_t* n_hits) {
  const int32_t st = call("ndt3d_best_map_poses_align_dev", H(target), H(source), d_poses, m, min_sep_trans, min_sep_rot, k,
                          static_cast<const void*>(hits), static_cast<const void*>(results), static_cast<const void*>(n_hits));
  if (st == NDT_OK) fill_hits<6>(k, hits, results, n_hits);
  return st;
}

// ---- batch and multi-device contexts -----------------------------------------------------------------------------------
int32_t ndt2d_batch_create(const ndt2d_params* p, int32_t device_id, ndt2d_batch** out) {
  return create(call("ndt2d_batch_create", Prm{p, 1}, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt3d_batch_create(const ndt3d_params* p, int32_t device_id, ndt3d_batch** out) {
  return create(call("ndt3d_batch_create", Prm{p, 1}, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt2d_batch_create_pyramid(const ndt2d_params* levels, int32_t n_levels, int32_t device_id, ndt2d_batch** out) {
  return create(call("ndt2d_batch_create_pyramid", Prm{levels, n_levels}, n_levels, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt3d_batch_create_pyramid(const ndt3d_params* levels, int32_t n_levels, int32_t device_id, ndt3d_batch** out) {
  return create(call("ndt3d_batch_create_pyramid", Prm{levels, n_levels}, n_levels, device_id, static_cast<const void*>(out)), out);
}
int32_t ndt2d_batch_destroy(ndt2d_batch* b) { return call("ndt2d_batch_destroy", H(b)); }
int32_t ndt3d_batch_destroy(ndt3d_batch* b) { return call("ndt3d_batch_destroy", H(b)); }
int32_t ndt2d_batch_set_tuning(ndt2d_batch* b, int32_t knob, int64_t value) { return call("ndt2d_batch_set_tuning", H(b), knob, value); }
int32_t ndt3d_batch_set_tuning(ndt3d_batch* b, int32_t knob, int64_t value) { return call("ndt3d_batch_set_tuning", H(b), knob, value); }
void* ndt3d_batch_stream(ndt3d_batch* b) { seen("ndt3d_batch_stream", H(b)); return reinterpret_cast<char*>(b) + 0x7000; }
int32_t ndt2d_batch_align(ndt2d_batch* b, const float* tx, const float* ty, const uint64_t* toff, const float* sx, const float* sy,
                          const uint64_t* soff, const double* init, size_t n_pairs, ndt2d_result* results) {
  const int32_t st = call("ndt2d_batch_align", H(b), F32s{tx, toff[n_pairs]}, F32s{ty, toff[n_pairs]}, U64s{toff, n_pairs + 1},
                          F32s{sx, soff[n_pairs]}, F32s{sy, soff[n_pairs]}, U64s{soff, n_pairs + 1}, Vals{init, 3 * n_pairs}, n_pairs,
                          static_cast<const void*>(results));
  if (st == NDT_OK) for (size_t i = 0; i < n_pairs; ++i) fill_result<3>(results + i, static_cast<int>(i));
  return st;
}
int32_t ndt3d_batch_align(ndt3d_batch* b, const float* tx, const float* ty, const float* tz, const uint64_t* toff, const float* sx,
                          const float* sy, const float* sz, const uint64_t* soff, const double* init, size_t n_pairs,
                          ndt3d_result* results) {
  const int32_t st = call("ndt3d_batch_align", H(b), F32s{tx, toff[n_pairs]}, F32s{ty, toff[n_pairs]}, F32s{tz, toff[n_pairs]},
                          U64s{toff, n_pairs + 1}, F32s{sx, soff[n_pairs]}, F32s{sy, soff[n_pairs]}, F32s{sz, soff[n_pairs]},
                          U64s{soff, n_pairs + 1}, Vals{init, 6 * n_pairs}, n_pairs, static_cast<const void*>(results));
  if (st == NDT_OK) for (size_t i = 0; i < n_pairs; ++i) fill_result<6>(results + i, static_cast<int>(i));
  return st;
}
int32_t ndt3d_batch_align_dev(ndt3d_batch* b, const float* d_tx, const float* d_ty, const float* d_tz, const uint64_t* d_toff,
                              const float* d_sx, const float* d_sy, const float* d_sz, const uint64_t* d_soff, const double* d_init,
                              size_t n_pairs, ndt3d_result* d_results, void* stream) {
  return call("ndt3d_batch_align_dev", H(b), d_tx, d_ty, d_tz, d_toff, d_sx, d_sy, d_sz, d_soff, d_init, n_pairs,
              static_cast<const void*>(d_results), stream);
}
int32_t ndt2d_multi_create(const ndt2d_params* p, const int32_t* device_ids, int32_t n_devices, ndt2d_multi** out) {
  return create(call("ndt2d_multi_create", Prm{p, 1}, I32s{device_ids, n_devices}, n_devices, static_cast<const void*>(out)), out);
}
int32_t ndt3d_multi_create(const ndt3d_params* p, const int32_t* device_ids, int32_t n_devices, ndt3d_multi** out) {
  return create(call("ndt3d_multi_create", Prm{p, 1}, I32s{device_ids, n_devices}, n_devices, static_cast<const void*>(out)), out);
}
int32_t ndt2d_multi_create_pyramid(const ndt2d_params* levels, int32_t n_levels, const int32_t* device_ids, int32_t n_devices,
                                   ndt2d_multi** out) {
  return create(call("ndt2d_multi_create_pyramid", Prm{levels, n_levels}, n_levels, I32s{device_ids, n_devices}, n_devices,
                     static_cast<const void*>(out)), out);
}
int32_t ndt2d_multi_destroy(ndt2d_multi* m) { return call("ndt2d_multi_destroy", H(m)); }
int32_t ndt3d_multi_destroy(ndt3d_multi* m) { return call("ndt3d_multi_destroy", H(m)); }
int32_t ndt2d_multi_device_count(const ndt2d_multi* m) { seen("ndt2d_multi_device_count", H(m)); return kDevices; }
int32_t ndt3d_multi_device_count(const ndt3d_multi* m) { seen("ndt3d_multi_device_count", H(m)); return kDevices; }
int32_t ndt2d_multi_align(ndt2d_multi* m, const float* tx, const float* ty, const uint64_t* toff, const float* sx, const float* sy,
                          const uint64_t* soff, const double* init, size_t n_pairs, ndt2d_result* results) {
  const int32_t st = call("ndt2d_multi_align", H(m), F32s{tx, toff[n_pairs]}, F32s{ty, toff[n_pairs]}, U64s{toff, n_pairs + 1},
                          F32s{sx, soff[n_pairs]}, F32s{sy, soff[n_pairs]}, U64s{soff, n_pairs + 1}, Vals{init, 3 * n_pairs}, n_pairs,
                          static_cast<const void*>(results));
  if (st == NDT_OK) for (size_t i = 0; i < n_pairs; ++i) fill_result<3>(results + i, static_cast<int>(i));
  return st;
}
int32_t ndt2d_multi_align_dev(ndt2d_multi* m, const float* const* d_tx, const float* const* d_ty, const uint64_t* const* d_toff,
                              const float* const* d_sx, const float* const* d_sy, const uint64_t* const* d_soff,
                              const double* const* d_init, const size_t* n_pairs, ndt2d_result** d_results_all, size_t* shard_stride,
                              ndt2d_result* results) {
  const int32_t st = call("ndt2d_multi_align_dev", H(m), PT(d_tx, kDevices), PT(d_ty, kDevices), PT(d_toff, kDevices),
                          PT(d_sx, kDevices), PT(d_sy, kDevices), PT(d_soff, kDevices), PT(d_init, kDevices),
                          U64s{reinterpret_cast<const uint64_t*>(n_pairs), kDevices}, static_cast<const void*>(d_results_all),
                          static_cast<const void*>(shard_stride), static_cast<const void*>(results));
  if (st == NDT_OK) for (size_t i = 0; i < n_pairs[0] + n_pairs[1]; ++i) fill_result<3>(results + i, static_cast<int>(i));
  return st;
}
}  // extern "C"

// Voxel-grid scan filter with exact centroids (included at the end of ndt2d_api.hip: one translation unit;
// docs/ALGORITHM.md section 2.24).  A cloud goes in, one point per occupied voxel of the absolute lattice
// i = floor(x / leaf) comes out: the voxel's centroid from integer sums, in ascending lattice order.  It is the submap's
// way of summing (section 2.2: offsets from the cell centre in units of leaf 2^-22, added as 64-bit integers), so the
// output - coordinates, counts, order - is the same to the bit for every order of the input and for every launch.
//
// An ordered compaction without a sort.  Every pass is its own launch, ordered by the launch boundaries alone; the only
// atomics are integer max / or / add, none of which decides a position:
//   k_vox_bounds      per axis min / max of i over the valid points, and the invalid points counted      -> host
//   k_vox_mark        one bit per voxel of the box (ix fastest), atomicOr
//   k_vox_chunk_sums  occupied voxels per chunk of kVoxChunk bitmap words
//   k_vox_scan        one workgroup: the chunks (later: the tiles) in front of each, and the total        -> host
//   k_vox_rank        per word the occupied voxels in front of it
//   k_vox_accumulate  each point finds its voxel's rank - its place in the contract's order: the word's base + the
//                     popcount of the bits below - adds (1, U) there and notes the voxel's index in the box
//   k_vox_keep        min_points > 1 only: voxels with n >= min_points per tile, then k_vox_scan again
//   k_vox_emit        mu = fma(sum U, leaf / (n 2^22), centre) per voxel, to rank (min_points = 1) or to the tile's
//                     base + the rank among the kept (ballot + mbcnt, as k_point_select)
// The host reads the header twice on the way (the box decides the bitmap's size, the voxel count the sums' size) and
// once at the end.
#pragma once
#include <type_traits>

namespace ndt {

constexpr int kVoxWordsPerThread = 8;
constexpr int kVoxChunk = kBlock * kVoxWordsPerThread;       // 2048 bitmap words = 65536 voxels per workgroup of the rank passes
constexpr unsigned int kVoxBias = 1u << 30;                  // |i| < 2^30
constexpr unsigned long long kVoxMaxBox = 1ull << 30;        // voxels of the occupied box
constexpr int kVoxMaxBlocks = 2048;                          // workgroups of the three passes over the points

// By value: every field is read with a constant index and stays in scalar registers.
template <int DIM>
struct VoxArgs {
  const float* s[3];               // the cloud (s[2] is null in 2D)
  unsigned int n;                  // <= kMaxSourcePoints < 2^31
  double leaf, scale;              // scale = 2^22 / leaf, one division on the host
  int lo[3];                       // the box's least index per axis
  unsigned int ext[3];             // its extent per axis (1 in z for 2D); ext[0] ext[1] ext[2] <= 2^30
  unsigned int n_voxels;           // occupied voxels (k_vox_accumulate)
  VoxHeader* hdr;
  uint2* words;
  unsigned int* cnt;
  unsigned int* key;
  unsigned long long* sum[3];
};

// i = floor(x / leaf) as one IEEE division; false: x is not finite or |i| >= 2^30
__device__ __forceinline__ bool vox_index(float x, double leaf, int* i) {
  const double f = floor((double)x / leaf);
  const bool ok = isfinite(x) && fabs(f) < 1073741824.0;
  *i = ok ? (int)f : 0;
  return ok;
}
// centre = (i + 0.5) leaf, one rounded product (i + 0.5 is exact)
__device__ __forceinline__ double vox_centre(int i, double leaf) {
#pragma clang fp contract(off)
  return ((double)i + 0.5) * leaf;
}
// U = llrint((x - centre) (2^22 / leaf)): a rounded difference, a rounded product, to nearest even
__device__ __forceinline__ long long vox_offset(float x, double centre, double scale) {
#pragma clang fp contract(off)
  const double d = (double)x - centre;
  return llrint(d * scale);
}

template <int DIM>
__device__ __forceinline__ bool vox_load(const VoxArgs<DIM>& a, unsigned int p, float* x, int* i) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    x[d] = a.s[d][p];
    ok &= vox_index(x[d], a.leaf, &i[d]);
  }
  return ok;
}
// The voxel's index in the box, ix fastest (< 2^30).  false: outside the box - the cloud is not the one k_vox_bounds
// saw (a caller that writes it during the call); such a point is dropped rather than indexed with.
template <int DIM>
__device__ __forceinline__ bool vox_linear(const VoxArgs<DIM>& a, const int* i, unsigned int* L_out) {
  unsigned int L = 0u;
  bool in = true;
#pragma unroll
  for (int d = DIM - 1; d >= 0; --d) {
    const unsigned int r = (unsigned int)(i[d] - a.lo[d]);
    in &= r < a.ext[d];
    L = L * a.ext[d] + r;
  }
  *L_out = L;
  return in;
}

template <int DIM>
__global__ __launch_bounds__(kBlock) void k_vox_bounds(VoxArgs<DIM> a) {
  __shared__ unsigned int s_red[kBlock / 64][2 * DIM + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned int hi[DIM], lo[DIM], bad = 0u;
#pragma unroll
  for (int d = 0; d < DIM; ++d) hi[d] = lo[d] = 0u;
  for (unsigned int p = blockIdx.x * kBlock + tid; p < a.n; p += gridDim.x * kBlock) {   // (p < 2^31 + 2^19: no wrap)
    float x[DIM];
    int i[DIM];
    if (vox_load<DIM>(a, p, x, i)) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        hi[d] = max(hi[d], kVoxBias + (unsigned int)i[d]);
        lo[d] = max(lo[d], kVoxBias - (unsigned int)i[d]);
      }
    } else {
      ++bad;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      hi[d] = max(hi[d], (unsigned int)__shfl_xor((int)hi[d], m, 64));
      lo[d] = max(lo[d], (unsigned int)__shfl_xor((int)lo[d], m, 64));
    }
    bad += (unsigned int)__shfl_xor((int)bad, m, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) { s_red[wave][d] = hi[d]; s_red[wave][DIM + d] = lo[d]; }
    s_red[wave][2 * DIM] = bad;
  }
  __syncthreads();
  if (tid < 2 * DIM + 1) {
    unsigned int v = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) v = tid < 2 * DIM ? max(v, s_red[w][tid]) : v + s_red[w][tid];
    if (tid < DIM) { if (v) atomicMax(&a.hdr->hi[tid], v); }
    else if (tid < 2 * DIM) { if (v) atomicMax(&a.hdr->lo[tid - DIM], v); }
    else if (v) atomicAdd(&a.hdr->n_invalid, v);
  }
}

// Same-address atomics serialise, and a bearing-ordered scan sends whole waves to one voxel: a lane whose neighbour below
// has the same voxel leaves the atomic to it, and a lane that already reads the bit as set issues none.  (The plain load
// may be older than another workgroup's atomic - then the bit is set twice, which is what atomicOr is for; it cannot be
// newer than the clear, which a launch boundary orders.)
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_vox_mark(VoxArgs<DIM> a) {
  const unsigned int lane = threadIdx.x & 63u;
  for (unsigned int p0 = blockIdx.x * kBlock + (threadIdx.x & ~63u); p0 < a.n; p0 += gridDim.x * kBlock) {   // (a wave walks together)
    const unsigned int p = p0 + lane;
    float x[DIM];
    int i[DIM];
    unsigned int L;
    if (!(p < a.n && vox_load<DIM>(a, p, x, i) && vox_linear<DIM>(a, i, &L))) L = 0xffffffffu;      // no voxel
    const unsigned int before = (unsigned int)__shfl_up((int)L, 1, 64);
    if (L != 0xffffffffu && (lane == 0u || before != L)) {
      unsigned int* word = reinterpret_cast<unsigned int*>(a.words) + 2u * (L >> 5);             // (.x of the word)
      const unsigned int bit = 1u << (L & 31u);
      if (!(*word & bit)) atomicOr(word, bit);
    }
  }
}

// the sum of v over the workgroup, in every thread (s_w: kBlock / 64 words, free again after the call)
__device__ __forceinline__ unsigned int vox_block_sum(unsigned int v, unsigned int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (unsigned int)__shfl_xor((int)v, m, 64);
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  unsigned int t = 0u;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) t += s_w[w];
  __syncthreads();
  return t;
}
// the sum of v over the threads in front of this one (exclusive scan over the workgroup)
__device__ __forceinline__ unsigned int vox_block_scan(unsigned int v, unsigned int* s_w, unsigned int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int u = (unsigned int)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  unsigned int off = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const unsigned int c = s_w[w];
    off += w < wave ? c : 0u;
    all += c;
  }
  __syncthreads();
  *total = all;
  return off + (inc - v);
}

// chunk b = words [b kVoxChunk, (b + 1) kVoxChunk) (the array is allocated and cleared in whole chunks); thread t has
// eight consecutive words, 64 bytes
__global__ __launch_bounds__(kBlock) void k_vox_chunk_sums(const uint2* __restrict__ words, unsigned int* __restrict__ chunk_sum) {
  __shared__ unsigned int s_w[kBlock / 64];
  const uint4* w4 = reinterpret_cast<const uint4*>(words + ((size_t)blockIdx.x * kVoxChunk + threadIdx.x * kVoxWordsPerThread));
  unsigned int c = 0u;
#pragma unroll
  for (int k = 0; k < kVoxWordsPerThread / 2; ++k) {
    const uint4 e = w4[k];
    c += (unsigned int)(__popc(e.x) + __popc(e.z));
  }
  const unsigned int t = vox_block_sum(c, s_w);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = t;
}

// One workgroup walks v[0 .. count) in order, kBlock a trip (k_point_scan on plain counts): base[k] = the sum in front
// of k; *total = the sum of all.
__global__ __launch_bounds__(kBlock) void k_vox_scan(const unsigned int* __restrict__ v, unsigned int count,
                                                      unsigned int* __restrict__ base, unsigned int* __restrict__ total) {
  __shared__ unsigned int s_w[kBlock / 64];
  unsigned int run = 0u;
  for (unsigned int k0 = 0u; k0 < count; k0 += kBlock) {            // (the same in every lane)
    const unsigned int k = k0 + threadIdx.x;
    unsigned int all;
    const unsigned int ex = vox_block_scan(k < count ? v[k] : 0u, s_w, &all);
    if (k < count) base[k] = run + ex;
    run += all;
  }
  if (threadIdx.x == 0) *total = run;
}

// per word the occupied voxels in front of it, into .y (the words of a thread without a voxel keep theirs: never read)
__global__ __launch_bounds__(kBlock) void k_vox_rank(uint2* __restrict__ words, const unsigned int* __restrict__ chunk_base) {
  __shared__ unsigned int s_w[kBlock / 64];
  uint4* w4 = reinterpret_cast<uint4*>(words + ((size_t)blockIdx.x * kVoxChunk + threadIdx.x * kVoxWordsPerThread));
  uint4 e[kVoxWordsPerThread / 2];
  unsigned int c = 0u;
#pragma unroll
  for (int k = 0; k < kVoxWordsPerThread / 2; ++k) {
    e[k] = w4[k];
    c += (unsigned int)(__popc(e[k].x) + __popc(e[k].z));
  }
  unsigned int all;
  unsigned int run = chunk_base[blockIdx.x] + vox_block_scan(c, s_w, &all);
  if (c == 0u) return;                                              // (behind the workgroup's barriers)
#pragma unroll
  for (int k = 0; k < kVoxWordsPerThread / 2; ++k) {
    e[k].y = run;
    run += (unsigned int)__popc(e[k].x);
    e[k].w = run;
    run += (unsigned int)__popc(e[k].z);
    w4[k] = e[k];
  }
}

// NDT_VOX_MERGE (default 1): neighbouring lanes of a wave that hit the same voxel - a lidar delivers its returns in
// bearing order, so runs of one voxel fill whole waves - add their (1, U) in registers first (a segmented scan over the
// runs, six shuffle steps), and the last lane of each run issues the atomics.  Integer sums: the result is the same to
// the bit either way (DESIGN 5.21 has what it is worth).
#ifndef NDT_VOX_MERGE
#define NDT_VOX_MERGE 1
#endif

template <int DIM>
__global__ __launch_bounds__(kBlock) void k_vox_accumulate(VoxArgs<DIM> a) {
  const unsigned int lane = threadIdx.x & 63u;
  // a wave walks the loop together (p0 is the same in its lanes): the shuffles below need all of them
  for (unsigned int p0 = blockIdx.x * kBlock + (threadIdx.x & ~63u); p0 < a.n; p0 += gridDim.x * kBlock) {
    const unsigned int p = p0 + lane;
    float x[DIM];
    int i[DIM];
    unsigned int L, rank = 0xffffffffu;
    long long U[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) U[d] = 0;
    if (p < a.n && vox_load<DIM>(a, p, x, i) && vox_linear<DIM>(a, i, &L)) {
      const uint2 w = a.words[L >> 5];
      const unsigned int r = w.y + (unsigned int)__popc(w.x & ((1u << (L & 31u)) - 1u));
      if (r < a.n_voxels) {                                        // (always, for the cloud that was marked)
        rank = r;
#pragma unroll
        for (int d = 0; d < DIM; ++d) U[d] = vox_offset(x[d], vox_centre(i[d], a.leaf), a.scale);
      }
    }
    const bool ok = rank != 0xffffffffu;
    unsigned int c = ok ? 1u : 0u;
    bool last = true;
#if NDT_VOX_MERGE
    const unsigned int before = (unsigned int)__shfl_up((int)rank, 1, 64);
    const unsigned long long heads = __ballot(lane == 0u || before != rank);
    // the run this lane is in: the heads at or below it (runs are contiguous, so equal numbers mean one run)
    const unsigned int run = __builtin_amdgcn_mbcnt_hi((unsigned int)(heads >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)heads, 0u)) +
                             (unsigned int)((heads >> lane) & 1ull);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const unsigned int run_up = (unsigned int)__shfl_up((int)run, s, 64);
      const unsigned int c_up = (unsigned int)__shfl_up((int)c, s, 64);
      const bool same = lane >= (unsigned int)s && run_up == run;
      c += same ? c_up : 0u;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const long long u_up = __shfl_up(U[d], s, 64);
        U[d] += same ? u_up : 0ll;
      }
    }
    last = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
#endif
    if (ok && last) {
      a.key[rank] = L;                                             // (every lane that stores here stores the same L)
      atomicAdd(&a.cnt[rank], c);
#pragma unroll
      for (int d = 0; d < DIM; ++d) atomicAdd(&a.sum[d][rank], (unsigned long long)U[d]);   // two's complement: the sum of the signed U
    }
  }
}

// tile t = voxels [t kBlock, (t + 1) kBlock)
__global__ __launch_bounds__(kBlock) void k_vox_keep(const unsigned int* __restrict__ cnt, unsigned int n_voxels,
                                                      unsigned int min_points, unsigned int* __restrict__ tile_cnt) {
  __shared__ unsigned int s_w[kBlock / 64];
  const unsigned int v = blockIdx.x * kBlock + threadIdx.x;
  const unsigned int t = vox_block_sum((v < n_voxels && cnt[v] >= min_points) ? 1u : 0u, s_w);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t;
}

template <int DIM>
struct VoxEmitArgs {
  double leaf;
  int lo[3];
  unsigned int ext[3];
  const unsigned int* cnt;
  const unsigned int* key;
  const unsigned long long* sum[3];
  const unsigned int* tile_base;   // COMPACT only
  unsigned int n_voxels, min_points;
  float* o[3];
  unsigned int* ocnt;              // or null
  unsigned long long capacity;
};

template <int DIM, bool COMPACT>
__global__ __launch_bounds__(kBlock) void k_vox_emit(VoxEmitArgs<DIM> a) {
  __shared__ unsigned int s_w[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned int v = blockIdx.x * kBlock + threadIdx.x;
  const unsigned int n = v < a.n_voxels ? a.cnt[v] : 0u;
  const bool kept = n >= a.min_points;                              // (min_points >= 1: a dead lane is not kept)
  unsigned long long pos = v;
  if constexpr (COMPACT) {
    const unsigned long long mask = __ballot(kept);
    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    if (lane == 0) s_w[wave] = (unsigned int)__popcll(mask);
    __syncthreads();
    unsigned int off = 0u;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) off += w < wave ? s_w[w] : 0u;
    pos = (unsigned long long)a.tile_base[blockIdx.x] + off + rank;
  }
  if (!kept || pos >= a.capacity) return;
  unsigned int L = a.key[v];
  const double step = a.leaf / ((double)n * 4194304.0);             // (n 2^22 is exact)
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const unsigned int q = d + 1 < DIM ? L / a.ext[d] : 0u;
    const int i = a.lo[d] + (int)(d + 1 < DIM ? L - q * a.ext[d] : L);
    L = q;
    const double mu = fma((double)(long long)a.sum[d][v], step, vox_centre(i, a.leaf));
    a.o[d][pos] = (float)mu;
  }
  if (a.ocnt) a.ocnt[pos] = n;
}

}  // namespace ndt

namespace {

unsigned vox_point_blocks(size_t n) {
  const size_t b = (n + ndt::kBlock - 1) / ndt::kBlock;
  return (unsigned)(b < (size_t)ndt::kVoxMaxBlocks ? b : (size_t)ndt::kVoxMaxBlocks);
}

// k_vox_bounds ends in seven atomics per workgroup on the same seven words, which serialise: four points per thread and
// at most 256 workgroups
unsigned vox_bounds_blocks(size_t n) {
  const size_t b = (n + 4 * ndt::kBlock - 1) / (4 * ndt::kBlock);
  return (unsigned)(b < 256 ? b : 256);
}

// the argument checks of both entry points, in the order the header lists them
template <int DIM>
int32_t voxel_filter_check(const void* h, const char* who, const float* const* s, size_t n, double leaf, uint32_t min_points,
                           float* const* o, const uint32_t* count, size_t capacity, const ndt_voxel_filter_info* info) {
  auto bad = [&](const char* what) { ndt::last_error() = std::string(who) + ": " + what; return NDT_ERR_INVALID_ARG; };
  if (!h) return bad("the handle is null");
  for (int a = 0; a < DIM; ++a) if (!s[a]) return bad("a coordinate array of the input is null");
  for (int a = 0; a < DIM; ++a) if (!o[a]) return bad("a coordinate array of the output is null");
  if (!info) return bad("info is null");
  if (n == 0) return bad("the cloud is empty");
  if (n > kMaxSourcePoints) return bad("the cloud holds more points than an alignment takes");
  if (!std::isfinite(leaf) || !(leaf > 0.0)) return bad("leaf is not finite and positive");
  if (min_points == 0) return bad("min_points is 0");
  auto overlaps = [](const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
  };
  for (int a = 0; a < DIM; ++a) {
    for (int b = 0; b < DIM; ++b)
      if (overlaps(s[a], n * sizeof(float), o[b], capacity * sizeof(float))) return bad("an output array overlaps an input array");
    if (count && overlaps(s[a], n * sizeof(float), count, capacity * sizeof(uint32_t))) return bad("the count array overlaps an input array");
  }
  return NDT_OK;
}

int32_t voxel_no_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    ndt::last_error() = std::string(who) + ": no HIP device visible: this library has no CPU fallback";
    return NDT_ERR_NO_DEVICE;
  }
  return NDT_OK;
}

// ndt*_voxel_filter_dev: device arrays in and out
template <class H>
int32_t voxel_filter_impl(H* h, const char* who, const float* const* d_s, size_t n, double leaf, uint32_t min_points,
                          float* const* d_o, uint32_t* d_count, size_t capacity, ndt_voxel_filter_info* info) {
  using namespace ndt;
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  { const int32_t cs = voxel_filter_check<DIM>(h, who, d_s, n, leaf, min_points, d_o, d_count, capacity, info); if (cs != NDT_OK) return cs; }
  std::memset(info, 0, sizeof(*info));
  { const int32_t ds = voxel_no_device(who); if (ds != NDT_OK) return ds; }
  HIP_TRY(hipSetDevice(h->device));
  { const int32_t fs = finish(h); if (fs != NDT_OK) return fs; }
  VoxelFilterScratch& S = h->vox;
  auto no_memory = [&]() {
    (void)hipGetLastError();
    last_error() = std::string(who) + ": the scratch cannot grow";
    return NDT_ERR_ALLOC;
  };
  if (!S.d_hdr && hipMalloc(&S.d_hdr, sizeof(VoxHeader)) != hipSuccess) return no_memory();
  if (!S.h_hdr && pinned_alloc(&S.h_hdr, sizeof(VoxHeader)) != hipSuccess) return no_memory();
  auto read_header = [&]() -> hipError_t {
    const hipError_t e = hipMemcpyAsync(S.h_hdr, S.d_hdr, sizeof(VoxHeader), hipMemcpyDeviceToHost, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
  };
  const unsigned blocks = vox_point_blocks(n);

  // 1. the occupied box
  VoxArgs<DIM> a{};
  for (int d = 0; d < DIM; ++d) a.s[d] = d_s[d];
  a.n = (unsigned int)n;
  a.leaf = leaf;
  a.scale = 4194304.0 / leaf;
  a.hdr = S.d_hdr;
  HIP_TRY(hipMemsetAsync(S.d_hdr, 0, sizeof(VoxHeader), h->stream));
  hipLaunchKernelGGL((k_vox_bounds<DIM>), dim3(vox_bounds_blocks(n)), dim3(kBlock), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(read_header());
  info->n_invalid = S.h_hdr->n_invalid;
  if (S.h_hdr->hi[0] == 0u) return NDT_OK;                          // every point is invalid
  unsigned long long box = 1ull;
  a.ext[2] = 1u;
  for (int d = 0; d < DIM; ++d) {
    const long long hi = (long long)S.h_hdr->hi[d] - (long long)kVoxBias, lo = (long long)kVoxBias - (long long)S.h_hdr->lo[d];
    a.lo[d] = (int)lo;
    a.ext[d] = (unsigned int)(hi - lo + 1);                         // < 2^31
    box = box <= kVoxMaxBox ? box * a.ext[d] : box;                 // (2^30 2^31 fits)
  }
  if (box > kVoxMaxBox) {
    last_error() = std::string(who) + ": the lattice box of the occupied voxels holds more than 2^30 voxels (a smaller cloud or a larger leaf)";
    return NDT_ERR_CAPACITY;
  }

  // 2. occupancy, 3. rank
  const size_t chunks = ((size_t)((box + 31ull) >> 5) + kVoxChunk - 1) / kVoxChunk;     // <= 2^14
  const size_t nword = chunks * kVoxChunk;
  if (grow({grow_buf(&S.d_words)}, &S.word_cap, nword, nword + (nword / 4 / kVoxChunk) * kVoxChunk) != hipSuccess) return no_memory();
  if (grow({grow_buf(&S.d_chunk_sum), grow_buf(&S.d_chunk_base)}, &S.chunk_cap, chunks, chunks + chunks / 4 + 64) != hipSuccess) return no_memory();
  a.words = S.d_words;
  HIP_TRY(hipMemsetAsync(S.d_words, 0, nword * sizeof(uint2), h->stream));
  hipLaunchKernelGGL((k_vox_mark<DIM>), dim3(blocks), dim3(kBlock), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vox_chunk_sums, dim3((unsigned)chunks), dim3(kBlock), 0, h->stream, (const uint2*)S.d_words, S.d_chunk_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(kBlock), 0, h->stream, (const unsigned int*)S.d_chunk_sum, (unsigned)chunks,
                     S.d_chunk_base, &S.d_hdr->n_voxels);
  HIP_TRY(hipGetLastError());
  HIP_TRY(read_header());
  const size_t nvox = S.h_hdr->n_voxels;                            // 1 .. min(n, box)
  info->n_voxels = nvox;
  if (nvox == 0) return NDT_OK;
  a.n_voxels = (unsigned int)nvox;
  const size_t tiles = (nvox + kBlock - 1) / kBlock;
  if (grow({grow_buf(&S.d_cnt), grow_buf(&S.d_key), grow_buf(&S.d_sum, 3)}, &S.vox_cap, nvox, nvox + nvox / 4 + 1024) != hipSuccess)
    return no_memory();
  for (int d = 0; d < DIM; ++d) a.sum[d] = S.d_sum + (size_t)d * S.vox_cap;
  a.cnt = S.d_cnt;
  a.key = S.d_key;
  HIP_TRY(hipMemsetAsync(S.d_cnt, 0, nvox * sizeof(unsigned int), h->stream));
  for (int d = 0; d < DIM; ++d) HIP_TRY(hipMemsetAsync(a.sum[d], 0, nvox * sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(k_vox_rank, dim3((unsigned)chunks), dim3(kBlock), 0, h->stream, S.d_words, (const unsigned int*)S.d_chunk_base);
  HIP_TRY(hipGetLastError());

  // 4. accumulate
  hipLaunchKernelGGL((k_vox_accumulate<DIM>), dim3(blocks), dim3(kBlock), 0, h->stream, a);
  HIP_TRY(hipGetLastError());

  // 5. finalise
  VoxEmitArgs<DIM> e{};
  e.leaf = leaf;
  for (int d = 0; d < 3; ++d) { e.lo[d] = a.lo[d]; e.ext[d] = a.ext[d]; }
  e.cnt = S.d_cnt;
  e.key = S.d_key;
  for (int d = 0; d < DIM; ++d) { e.sum[d] = a.sum[d]; e.o[d] = d_o[d]; }
  e.n_voxels = (unsigned)nvox;
  e.min_points = min_points;
  e.ocnt = d_count;
  e.capacity = capacity;
  if (min_points > 1) {
    if (grow({grow_buf(&S.d_tile_cnt), grow_buf(&S.d_tile_base)}, &S.tile_cap, tiles, tiles + tiles / 4 + 64) != hipSuccess) return no_memory();
    hipLaunchKernelGGL(k_vox_keep, dim3((unsigned)tiles), dim3(kBlock), 0, h->stream, (const unsigned int*)S.d_cnt, (unsigned)nvox,
                       min_points, S.d_tile_cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(kBlock), 0, h->stream, (const unsigned int*)S.d_tile_cnt, (unsigned)tiles,
                       S.d_tile_base, &S.d_hdr->n_out);
    HIP_TRY(hipGetLastError());
    e.tile_base = S.d_tile_base;
    hipLaunchKernelGGL((k_vox_emit<DIM, true>), dim3((unsigned)tiles), dim3(kBlock), 0, h->stream, e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(read_header());
    info->n_out = S.h_hdr->n_out;
  } else {
    hipLaunchKernelGGL((k_vox_emit<DIM, false>), dim3((unsigned)tiles), dim3(kBlock), 0, h->stream, e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    info->n_out = nvox;
  }
  if (info->n_out > capacity) {
    last_error() = std::string(who) + ": the outputs hold fewer than info->n_out elements";
    return NDT_ERR_CAPACITY;
  }
  return NDT_OK;
}

// ndt*_voxel_filter: host arrays in and out, staged as ndt*_fit_points stages its scan
template <class H>
int32_t voxel_filter_host(H* h, const char* who, const float* const* s, size_t n, double leaf, uint32_t min_points,
                          float* const* o, uint32_t* count, size_t capacity, ndt_voxel_filter_info* info) {
  using namespace ndt;
  constexpr int DIM = std::is_same<H, ndt2d_handle>::value ? 2 : 3;
  { const int32_t cs = voxel_filter_check<DIM>(h, who, s, n, leaf, min_points, o, count, capacity, info); if (cs != NDT_OK) return cs; }
  std::memset(info, 0, sizeof(*info));
  { const int32_t ds = voxel_no_device(who); if (ds != NDT_OK) return ds; }
  HIP_TRY(hipSetDevice(h->device));
  const float* d_s[3];
  { const int32_t ss = fit_stage(h, s, n, d_s); if (ss != NDT_OK) return ss; }
  VoxelFilterScratch& S = h->vox;
  const size_t cap = capacity < n ? capacity : n;                   // (n_out <= n)
  if (grow({grow_buf(&S.d_out, 3), grow_buf(&S.d_ocnt)}, &S.out_cap, cap, cap + cap / 4 + 1024) != hipSuccess) {
    (void)hipGetLastError();
    last_error() = std::string(who) + ": the scratch cannot grow";
    return NDT_ERR_ALLOC;
  }
  float* d_o[3] = {S.d_out, S.d_out + S.out_cap, DIM == 3 ? S.d_out + 2 * S.out_cap : nullptr};
  const int32_t st = voxel_filter_impl(h, who, d_s, n, leaf, min_points, d_o, count ? S.d_ocnt : nullptr, cap, info);
  if (st != NDT_OK) return st;
  const size_t m = (size_t)info->n_out;
  if (m == 0) return NDT_OK;
  for (int d = 0; d < DIM; ++d) HIP_TRY(hipMemcpyAsync(o[d], d_o[d], m * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (count) HIP_TRY(hipMemcpyAsync(count, S.d_ocnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

}  // namespace

extern "C" {

int32_t ndt2d_voxel_filter_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, double leaf, uint32_t min_points,
                               float* d_ox, float* d_oy, uint32_t* d_count, size_t capacity, ndt_voxel_filter_info* info) {
  TraceRange range("ndt2d_voxel_filter");
  const float* s[3] = {d_x, d_y, nullptr};
  float* o[3] = {d_ox, d_oy, nullptr};
  return voxel_filter_impl(h, "ndt2d_voxel_filter_dev", s, n, leaf, min_points, o, d_count, capacity, info);
}
int32_t ndt2d_voxel_filter(ndt2d_handle* h, const float* x, const float* y, size_t n, double leaf, uint32_t min_points, float* ox,
                           float* oy, uint32_t* count, size_t capacity, ndt_voxel_filter_info* info) {
  TraceRange range("ndt2d_voxel_filter");
  const float* s[3] = {x, y, nullptr};
  float* o[3] = {ox, oy, nullptr};
  return voxel_filter_host(h, "ndt2d_voxel_filter", s, n, leaf, min_points, o, count, capacity, info);
}
int32_t ndt3d_voxel_filter_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n, double leaf,
                               uint32_t min_points, float* d_ox, float* d_oy, float* d_oz, uint32_t* d_count, size_t capacity,
                               ndt_voxel_filter_info* info) {
  TraceRange range("ndt3d_voxel_filter");
  const float* s[3] = {d_x, d_y, d_z};
  float* o[3] = {d_ox, d_oy, d_oz};
  return voxel_filter_impl(h, "ndt3d_voxel_filter_dev", s, n, leaf, min_points, o, d_count, capacity, info);
}
int32_t ndt3d_voxel_filter(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, double leaf,
                           uint32_t min_points, float* ox, float* oy, float* oz, uint32_t* count, size_t capacity,
                           ndt_voxel_filter_info* info) {
  TraceRange range("ndt3d_voxel_filter");
  const float* s[3] = {x, y, z};
  float* o[3] = {ox, oy, oz};
  return voxel_filter_host(h, "ndt3d_voxel_filter", s, n, leaf, min_points, o, count, capacity, info);
}

}  // extern "C"

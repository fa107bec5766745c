/*
 * ndt_hip.h - C ABI of the MI355X (gfx950) NDT scan matcher.
 *
 * Drop-in boundary.  BASELINE.json's north_star names the interface
 * this library sits behind - "the repo's existing scan-matcher -> GTSAM-factor interface" -
 * but the reference checkout contains no header, class or signature for it:
 * /root/reference/README.md:1 ("# GTSAM-NDT") is the only line of the only file.  Each
 * entry point below therefore cites the SURVEY.md section 8 row it implements instead of a
 * reference file:line; INTEGRATION.md shows the adapter a maintainer of the reference
 * would write against this header once the real interface is visible.
 *
 * Conventions
 *   - extern "C", opaque handles, plain pointers and sizes, POD structs.  No C++ or torch
 *     types cross this boundary.
 *   - Every function returns an int32 status: 0 = NDT_OK; > 0 = numerical outcome of an
 *     alignment (also stored in ndt2d_result.status); < 0 = usage / HIP error.  No
 *     exception crosses the ABI; HIP errors are captured and returned.
 *   - Host-pointer entry points borrow the caller's buffers for the duration of the call
 *     and are synchronous.  "_dev" entry points take device pointers (any allocator:
 *     hipMalloc, torch) and enqueue on the given hipStream_t (passed as void*); results
 *     written to device memory are valid after that stream is synchronised.
 *   - A handle is single-threaded; distinct handles may be used from distinct threads.  A map-to-map call
 *     (ndt2d_align_map / ndt2d_evaluate_map, ndt3d_align_map / ndt3d_evaluate_map) uses BOTH its handles for its
 *     duration: no other thread may touch either.
 *   - Points are SoA float32 arrays (x[], y[]); poses are double (tx, ty, theta).
 *   - There is NO CPU fallback: every entry point that computes needs a gfx950 device.
 */
#ifndef NDT_HIP_H_
#define NDT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDT_ABI_VERSION 1

/* ---- status codes -------------------------------------------------------------- */
enum {
  NDT_OK = 0,
  NDT_NOT_CONVERGED = 1,      /* max_iterations reached                              */
  NDT_DEGENERATE_HESSIAN = 2, /* H + lambda*diag(H) never became positive definite    */
  NDT_TOO_FEW_HITS = 3,       /* fewer than min_hits source points fell in valid cells */
  NDT_TOO_FEW_CELLS = 4,      /* target grid has no valid cell                        */
  NDT_ERR_INVALID_ARG = -1,
  NDT_ERR_NO_TARGET = -2,
  NDT_ERR_HIP = -3,
  NDT_ERR_NO_DEVICE = -4,
  NDT_ERR_CAPACITY = -5,      /* a per-cell or per-grid capacity limit was exceeded   */
  NDT_ERR_ALLOC = -6,
  NDT_ERR_RCCL = -7           /* an RCCL call of the multi-device gather failed (ndt_last_error has its text) */
};

enum { NDT_HESSIAN_GAUSS_NEWTON = 0, NDT_HESSIAN_NEWTON = 1 };

/* ---- parameters (SURVEY.md section 5 "Config/flags": one POD at handle creation) -- */
typedef struct ndt2d_params {
  double cell_size;        /* c, metres                                   (row a1) */
  int32_t min_points;      /* a cell is valid iff n >= min_points          (row a3) */
  int32_t hessian_mode;    /* NDT_HESSIAN_*                                (row a6) */
  double eig_ratio;        /* lambda_min clamped to eig_ratio*lambda_max   (row a3) */
  double d1, d2;           /* score = sum d1*exp(-d2/2 * q' S^-1 q)        (row a5) */
  int32_t max_iterations;  /* cap on Gauss-Newton updates                  (row a8) */
  int32_t fixed_iterations;/* > 0: run exactly this many updates, no convergence test */
  double eps_trans;        /* converged when |dt| < eps_trans and ...      (row a8) */
  double eps_rot;          /* ... |dtheta| < eps_rot                               */
  double step_max_trans;   /* step is scaled so |dt| <= step_max_trans     (row a8) */
  double step_max_rot;     /* ... and |dtheta| <= step_max_rot                     */
  int32_t min_hits;        /* fewer hits than this => NDT_TOO_FEW_HITS             */
  int32_t overlap_grids;   /* 0 or 1: one grid; 4: Biber's four grids shifted by half a cell, every
                              point scores against all four (every 2D entry point: ndt2d_align*, the multi-start /
                              multi-scan chains, ndt2d_batch_*, ndt2d_multi_*)  */
  int32_t line_search;     /* 0: plain Gauss-Newton steps.  n in 1..16: backtracking line search - an
                              evaluation that scores worse than the pose its step started from (or
                              leaves the map) halves the step and retries from that pose, at most n
                              times per step; every trial is one evaluation and counts as one
                              iteration; convergence is tested on accepted evaluations only */
  int32_t reserved;
  double step_scale;       /* over-relaxation: the solved step is multiplied by this before the step
                              limits and the convergence test.  1 = plain Gauss-Newton/Newton.  The
                              Gauss-Newton Hessian of this score overestimates the true curvature
                              about 3x, so 2..3 cuts the iterations to
                              convergence 2..3x; keep 1 with NDT_HESSIAN_NEWTON.  0 means 1;
                              valid range (0, 8] */
} ndt2d_params;

/* ---- result (row a9) ------------------------------------------------------------ */
typedef struct ndt2d_result {
  double pose[3];     /* tx, ty, theta: maps source-frame points into the target frame */
  double H[9];        /* row-major 3x3 Hessian of -score at the last evaluated pose     */
  double g[3];        /* gradient of -score at the last evaluated pose                  */
  double score;       /* sum of per-point scores at the last evaluated pose             */
  int32_t iterations; /* Gauss-Newton updates applied                                   */
  int32_t n_hit;      /* source points that fell in a valid cell at the last evaluation */
  int32_t status;     /* NDT_OK / NDT_NOT_CONVERGED / ...                               */
  int32_t reserved;
} ndt2d_result;

/* one evaluation at a fixed pose (rows a4-a7), for stage parity tests and callers that
 * run their own optimiser */
typedef struct ndt2d_eval {
  double H[9];
  double g[3];
  double score;
  int32_t n_hit;
  int32_t reserved;
} ndt2d_eval;

/* geometry of the cached target grid (rows a1-a3) */
typedef struct ndt2d_grid_info {
  float ox, oy;       /* origin (lower-left corner of cell 0)  */
  float inv_cell;     /* float32(1/cell_size)                  */
  float cell;
  int32_t width, height;
  int32_t n_valid;    /* cells with n >= min_points and a usable covariance */
  int32_t n_points;   /* target points binned                                */
} ndt2d_grid_info;

typedef struct ndt2d_handle ndt2d_handle;

/* ---- lifecycle -------------------------------------------------------------------- */
int32_t ndt_abi_version(void);
const char* ndt_status_string(int32_t status);
/* last HIP error text captured on this thread ("" if none) */
const char* ndt_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int32_t ndt_device_count(void);
/* How a host thread waits for an alignment's end flag (pinned host memory).  0 (default): it spins on its core - a
 * call takes 60-300 us, less than a sleep's granularity.  1: it spins for the first ~20 us of a wait and then gives the
 * core away between polls (sched_yield) - for a process that drives several handles from more threads than it has
 * cores.  Process-wide, takes effect at the next wait; results do not depend on it. */
int32_t ndt_set_host_wait(int32_t mode);

void ndt2d_default_params(ndt2d_params* p);
int32_t ndt2d_create(const ndt2d_params* p, int32_t device_id, ndt2d_handle** out);
int32_t ndt2d_destroy(ndt2d_handle* h);

/* ---- (i) target voxel grid: rows a1-a3 ---------------------------------------------- */
/* Builds and caches the NDT grid of a target cloud. */
int32_t ndt2d_set_target(ndt2d_handle* h, const float* x, const float* y, size_t n);
int32_t ndt2d_set_target_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n,
                             void* stream);
/* An empty grid over a caller-chosen extent (the region a submap is allowed to grow into),
 * filled afterwards with ndt2d_add_target_points(_dev).  The geometry is what ndt2d_set_target
 * derives from a cloud whose bounding box is [xmin, xmax] x [ymin, ymax] (as float32), so
 * reserve + add of a cloud's own bounding box gives bit for bit the grid of ndt2d_set_target.
 * Aligning against it before any cell is valid returns NDT_TOO_FEW_CELLS. */
int32_t ndt2d_reserve_target(ndt2d_handle* h, double xmin, double ymin, double xmax, double ymax);
/* Incremental submap update: bins n more points into the
 * cached grid's exact per-cell sums and re-finalises.  Points outside the cached extent
 * are counted in *n_outside (may be NULL) and ignored; so are points whose cell lies on the grid's
 * outermost ring (within one cell of the extent's border): the ring stays empty by contract,
 * because alignments clamp out-of-range lookups onto it. */
int32_t ndt2d_add_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n,
                                size_t* n_outside);
/* The same with the points already on the device, optionally moved into the map frame first:
 * pose != NULL applies p' = R(theta) p + t in float32 (x' = (cs*x - sn*y) + tx, y' = (sn*x + cs*y)
 * + ty with cs, sn = (float)cos/sin(theta), every operation rounded separately) - the pose an
 * alignment of that scan returned - so a scan goes ranges -> points -> align -> submap without
 * leaving the GPU.  NaN points (no return) are ignored.  `stream` is the stream that produced
 * d_x/d_y (NULL: already complete); the call returns when the grid is updated. */
int32_t ndt2d_add_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n,
                                    const double pose[3], size_t* n_outside, void* stream);
/* The exact inverse of ndt2d_add_target_points: takes n points out of the cached grid's per-cell sums and
 * re-finalises the cells they lie in.  The points are binned by the float32 operations of the add (outside and
 * ring points are counted in *n_outside and nothing is subtracted for them; with overlap_grids = 4 a point leaves
 * all four grids), and the sums are exact integers, so if the points are - as float32 values - points that were
 * added before, the grid is bit for bit the one the handle would hold had they never been added, whatever was
 * added or removed in between: sums (ndt2d_save_map), records, n_valid, n_points and every alignment.  A cell that
 * falls below min_points becomes invalid (zero record); geometry and storage never change, and a grid with
 * everything removed equals a fresh ndt2d_reserve_target of its extent.
 * Points that are not in the map are detected where the integers show it - a cell's count would go below zero, or
 * reaches zero while one of its sums does not: NDT_ERR_INVALID_ARG (ndt_last_error() says so), and the handle has
 * no target afterwards, as after a failed add.  One call takes fewer than 2^32 - 2^20 points. */
int32_t ndt2d_remove_target_points(ndt2d_handle* h, const float* x, const float* y, size_t n,
                                   size_t* n_outside);
/* The same with the points on the device: pose, NaN points, `stream` and the return are those of
 * ndt2d_add_target_points_dev.  Removing a scan with the pose it was added with and adding it again with another
 * re-anchors it in the submap (a loop closure moved it) at the cost of two scans, not of the submap. */
int32_t ndt2d_remove_target_points_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n,
                                       const double pose[3], size_t* n_outside, void* stream);
/* ---- submap persistence -------------------------------------------------------------------
 * The cached grid as a flat buffer: this header, then n_cells per-cell blocks of the EXACT fixed-point sums the
 * build keeps (2D, 48 B: int64 sx, sy, sxx, sxy, syy; uint32 n, pad.  3D, 80 B: int64 s[3], ss[6] (xx xy xz yy yz
 * zz); uint32 n, pad.  Coordinates are relative to the cell centre, in units of cell_size / 2^22).  Loading
 * re-finalises the sums with the LOADING handle's min_points / eig_ratio: with the saving handle's parameters the
 * grid is bit for bit the one that was saved, it goes on taking points (ndt2d_add_target_points*), and a map can be
 * re-finalised under other validity rules without the raw points.  cell_size (and overlap_grids) must match the
 * handle's (NDT_ERR_INVALID_ARG otherwise, as for a buffer that is not a map or is cut short); sums found in the
 * outermost ring of a 2D map, which the builders keep empty, are dropped on load.  The format is
 * little-endian, as the machines this library runs on. */
#define NDT_MAP_MAGIC 0x4d54444eu   /* "NDTM" */
typedef struct ndt_map_header {
  uint32_t magic, version;         /* NDT_MAP_MAGIC, 1 */
  int32_t dims, ngrid;             /* 2 or 3; 1, or 4 for the 2D overlapping grids (stored back to back) */
  int32_t width, height, depth;    /* cells per axis (depth 1 in 2D); x fastest, then y, then z */
  uint32_t cell_bytes;             /* 48 or 80 */
  double cell_size;
  uint64_t n_cells;                /* width * height * depth * ngrid */
  uint64_t n_points;               /* points binned so far (2D; 0 in 3D) */
  float origin[4][3];              /* lower corner of grid g */
} ndt_map_header;
/* bytes ndt2d_save_map writes for the cached grid (0 without one) */
size_t ndt2d_map_size(const ndt2d_handle* h);
/* *written (may be NULL) = the bytes needed, also when capacity is too small (NDT_ERR_CAPACITY) */
int32_t ndt2d_save_map(ndt2d_handle* h, void* buf, size_t capacity, size_t* written);
int32_t ndt2d_load_map(ndt2d_handle* h, const void* buf, size_t bytes);
/* ---- a coarser submap from a submap's sums ------------------------------------------------
 * dst receives a target grid whose cells are unions of f x f cells of src's cached grid, f = dst's cell_size / src's,
 * which must be exactly 2 or 4 (tested as dst_cell == f * src_cell in double).  No points are needed: the exact
 * per-cell sums of the children give the parent's by integer arithmetic alone (docs/ALGORITHM.md section 2.17), on the
 * device, deterministic to the bit.  This is what a pyramid level of a submap needs that came back from
 * ndt2d_load_map and never saw a point.
 * Lattice, per axis: with k0 = rint(origin / c) the fine origin in fine cells, the coarse cells are those of the
 * lattice of multiples of f c; the coarse origin is (float)(K0 c) with K0 = f floor((k0 + 1 - f) / f), fine cell ix
 * lies in coarse cell (k0 + ix - K0) / f, and the coarse extent is (k0 + W - 2 - K0) / f + 2.  For a src that
 * ndt2d_set_target built from a cloud these are the origin and extents ndt2d_set_target derives from the same cloud
 * at cell f c; the outermost ring of dst is empty, as the 2D contract asks.  The float32 rounding of the coarse origin
 * shifts the lattice by less than an ulp of the origin, as the fine origin's own rounding does; it is zero where
 * K0 c is a float32 value (dyadic cell sizes at ordinary coordinates).
 * Sums: a child at position k of f along an axis has its centre (2k - f + 1) 2^21 fine units from the parent's; the
 * children's sums are moved there and added exactly (up to 67 bits), then brought to the parent's unit (f fine
 * units) by S' = floor((N + f/2) / f) and SS' = floor((NN + f^2/2) / f^2) - the only roundings.  Where they leave
 * n' SS'_aa < S'_a^2 (a nearly degenerate cell), SS'_aa is raised to ceil(S'_a^2 / n'), so that every coarse map
 * passes ndt2d_load_map.  n_points carries over.
 * The coarse sums are finalised with DST's min_points / eig_ratio, as ndt2d_load_map does, and dst then is what a handle
 * is after ndt2d_load_map: it aligns, serves ndt2d_align_map* / ndt2d_search_*map* on either side, takes
 * ndt2d_add_target_points* / ndt2d_remove_target_points*, and saves.  src is unchanged.  Pending asynchronous
 * alignments of both handles are finished first; the call returns when dst is ready.
 * NDT_ERR_INVALID_ARG: a null handle, src == dst, handles on different devices, a ratio that is not 2 or 4, or
 * overlap_grids = 4 on either side (out of scope: four fine grids shifted by half a FINE cell do not coarsen into
 * grids shifted by half a COARSE cell).  NDT_ERR_NO_TARGET: src holds no grid.  NDT_ERR_CAPACITY: the coarse grid
 * exceeds 2^27 cells, or a coarse cell would hold more than 2^20 points; dst has no target afterwards, as after a
 * failed load.  ndt_last_error() says which. */
int32_t ndt2d_coarsen_map(ndt2d_handle* src, ndt2d_handle* dst);

/* Folds the submap of src into the submap of dst at `pose` (x, y, yaw: src's frame in dst's, what ndt2d_align_map(dst,
 * src) returns), from src's exact per-cell sums alone (docs/ALGORITHM.md section 2.18) - no points, so it works on maps
 * that came back from ndt2d_load_map.  ndt2d_unmerge_map takes the same contribution out again.
 * Per cell of src's grid with 0 < n <= 2^20, centre e, sums S, SS (src units c_s 2^-22), k = c_s / c_d, all float64 in a
 * fixed operation order without contraction, R = (cos, -sin; sin, cos) from libm on the host:
 *   1. mu = e + S / (n 2^22 / c_s); mu' = (R0 mu_x + R1 mu_y) + t per row; the destination cell is the one dst's own
 *      float32 binning rule gives (float)mu'.  A block that lands outside dst's interior (the ring counts as outside) is
 *      dropped whole and its n added to *n_outside (may be NULL).
 *   2. a = ((R e + t) - centre_dst) 2^22 / c_d;  r = k (R S);  Q = k^2 (R SS R^T).
 *   3. dn = n, dS_a = llrint(n a_a + r_a), dSS_ab = llrint(n a_a a_b + a_a r_b + a_b r_a + Q_ab) (half to even); where
 *      n dSS_aa < dS_a^2 (exact), dSS_aa is raised to ceil(dS_a^2 / n), the rule of ndt2d_coarsen_map, so every
 *      contribution - and by Cauchy-Schwarz every sum of them - passes ndt2d_load_map.
 *   4. dst's sums += (merge) or -= (unmerge) the contribution by integer atomics: merges commute bit for bit and unmerge
 *      with the same (src, pose) is the exact inverse whatever was added to or removed from dst in between.
 *   5. dst's cells are finalised again with dst's min_points / eig_ratio, n_points changes by the merged n, and what
 *      map-to-map alignment derived from dst is dropped.  src is unchanged; the call returns when dst is ready.
 * A source cell goes wholly to the cell of its mean, so the result is not the map a rebuild from the points would give;
 * total count and (within the roundings) the global first and second moments are conserved.
 * NDT_ERR_INVALID_ARG: a null handle or pose, src == dst, handles on different devices, overlap_grids = 4 on either
 * side, src's cell_size above dst's, a pose that is not finite; for ndt2d_unmerge_map also content that is not in dst (a
 * cell's count fell below zero, or reached zero with sums left) - dst then has no target, as after a failed
 * ndt2d_remove_target_points.  NDT_ERR_NO_TARGET: either handle holds no grid (a reserved one counts).
 * NDT_ERR_CAPACITY: a destination cell would exceed 2^20 points; dst has no target afterwards. */
int32_t ndt2d_merge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside);
int32_t ndt2d_unmerge_map(ndt2d_handle* dst, ndt2d_handle* src, const double pose[3], size_t* n_outside);

int32_t ndt2d_get_grid_info(ndt2d_handle* h, ndt2d_grid_info* info);
/* Copies the finalised cell records to host arrays of width*height entries each
 * (any pointer may be NULL): count, mean (x,y interleaved), icov (a,b,c interleaved). */
int32_t ndt2d_get_grid(ndt2d_handle* h, int32_t* count, float* mean_xy, float* icov_abc);

/* ---- (ii)+(iii) evaluation at a fixed pose: rows a4-a7 ------------------------------- */
int32_t ndt2d_evaluate(ndt2d_handle* h, const float* sx, const float* sy, size_t n,
                       const double pose[3], ndt2d_eval* out);

/* the scan already on the device (ndt2d_wait_stream orders the handle behind its producer) */
int32_t ndt2d_evaluate_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3],
                           ndt2d_eval* out);

/* ---- per-point fit and selection (docs/ALGORITHM.md section 2.19) ---------------------- */
/* The class of a source point at a pose, one byte per point. */
enum {
  NDT_POINT_INVALID = 0,   /* a coordinate is NaN or +-inf (tested on the input, before anything is clamped)        */
  NDT_POINT_MISS = 1,      /* finite, but no valid cell: outside the grid, on its ring, a cell with n < min_points  */
  NDT_POINT_MISFIT = 2,    /* in a valid cell, m > max_m                                                            */
  NDT_POINT_FIT = 3        /* in a valid cell, m <= max_m (a float32 compare)                                       */
};
/* What a fit or a selection counted.  The four class counts add up to n.  n_miss + n_misfit + n_fit and
 * n_misfit + n_fit count POINTS: with overlap_grids = 4 a point in valid cells of several grids is one hit here, where
 * ndt2d_eval::n_hit counts it once per grid.  n_selected: the points a selection copied (0 after a fit call). */
typedef struct ndt_point_fit {
  uint64_t n_invalid, n_miss, n_misfit, n_fit, n_selected;
} ndt_point_fit;

/* Scores every point of a scan against the cached grid at `pose`.  Image point, cell and m_i = q' Sigma^-1 q are the
 * float32 operations of the single-scan alignment (the angle wrapped, cos / sin rounded from float64, the fma image, the
 * key clamped onto the ring; q, Sigma^-1 q, m as three fmas and two multiplies), m_i is not clamped at zero, and with
 * overlap_grids = 4 it is the least m over the grids whose cell is valid (a hit = any grid's cell valid).
 *   d_class[i] (may be NULL): the class above.   d_m[i] (may be NULL): m_i for classes 2 and 3, +inf for 1, NaN for 0.
 * Runs on the handle's stream under the stream contract of ndt2d_evaluate_dev (ndt2d_wait_stream for producers), finishes
 * a pending asynchronous alignment first (its result stays fetchable) and returns when the outputs and *fit are complete.
 * Every output is deterministic to the bit.  A grid without a valid cell (a reserved one) is no error: every finite
 * point is a MISS.
 * NDT_ERR_INVALID_ARG (ndt_last_error says which): a null handle, scan, pose or fit; n = 0 or above what an alignment
 * takes; a pose that is not finite; max_m NaN or negative (+inf is legal: every hit fits).  NDT_ERR_NO_TARGET: no grid.
 * NDT_ERR_ALLOC: the handle's scratch (a byte per point where d_class is NULL, 20 bytes per 1024 points) cannot grow. */
int32_t ndt2d_fit_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3],
                             float max_m, float* d_m, uint8_t* d_class, ndt_point_fit* fit);
/* the same with host arrays in and out, the scan staged as ndt2d_evaluate stages it */
int32_t ndt2d_fit_points(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double pose[3], float max_m,
                         float* m, uint8_t* cls, ndt_point_fit* fit);
/* Fits as above and copies the points whose class is in `keep` (a mask of 1 << class, 1 .. 15) to d_ox / d_oy[0 ..
 * fit->n_selected): in the SOURCE frame, bit for bit, in ascending index order - what ndt2d_add_target_points_dev(...,
 * pose) and ndt2d_remove_target_points_dev take.  d_index (may be NULL) receives their indices in the scan.  Elements
 * past n_selected are not written; the outputs hold n elements and must not overlap the inputs.
 * NDT_ERR_INVALID_ARG also for keep = 0 or above 15 and for a null d_ox / d_oy. */
int32_t ndt2d_select_points_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double pose[3],
                                float max_m, uint32_t keep, float* d_ox, float* d_oy, uint32_t* d_index,
                                ndt_point_fit* fit);

/* ---- voxel-grid scan filter, exact centroids (docs/ALGORITHM.md section 2.24) ---------- */
/* What a filter call counted: the points skipped, the occupied voxels, and those with n >= min_points (the outputs). */
typedef struct ndt_voxel_filter_info {
  uint64_t n_invalid, n_voxels, n_out;
} ndt_voxel_filter_info;

/* Downsamples a cloud to one point per occupied voxel of the ABSOLUTE lattice i = floor(x / leaf) per axis (independent
 * of the cloud's bounding box: a world point lands in the same voxel in every call): the voxel's centroid.  Per point,
 * in float64 on the float32 input, every operation rounded once: i = floor(x / leaf); centre = (i + 0.5) leaf;
 * U = llrint((x - centre) (2^22 / leaf)).  A point is invalid - skipped and counted - if a coordinate is not finite or
 * an |i| >= 2^30.  Per occupied voxel n and the sum of U per axis are integers (uint32, int64), so they do not depend on
 * the order of the points; the output coordinate is fma((double) sum U, leaf / (n 2^22), centre) rounded to float32 once.
 * A voxel is emitted iff n >= min_points (1: every occupied voxel; 2 or 3 drop isolated returns), in ascending lattice
 * order (iy, ix), ix fastest.  d_count (may be NULL) receives n per emitted voxel.  Outputs and *info are the same to the
 * bit for every permutation of the input and for every launch.
 * Runs on the handle's stream under the stream contract of ndt2d_fit_points_dev (ndt2d_wait_stream for producers),
 * finishes a pending asynchronous alignment first (its result stays fetchable) and returns when the outputs and *info
 * are complete.  It needs no target and leaves a cached grid untouched.  The outputs hold `capacity` elements (n is
 * always enough) and are never written past info->n_out or capacity.
 * NDT_ERR_CAPACITY with *info filled: n_out > capacity (retry with n_out).  NDT_ERR_CAPACITY with n_voxels = 0: the
 * lattice box of the occupied voxels (max - min + 1 per axis) holds more than 2^30 voxels; ndt_last_error says which.
 * NDT_ERR_INVALID_ARG (ndt_last_error says which): a null handle, input, output or info; n = 0 or above what an
 * alignment takes; leaf not finite or <= 0; min_points = 0; an output that overlaps an input (pointer ranges).
 * NDT_ERR_ALLOC: the handle's scratch (32 bytes per occupied voxel, 8 bytes per 32 voxels of the box) cannot grow.
 * Every point invalid: NDT_OK with n_out = 0. */
int32_t ndt2d_voxel_filter_dev(ndt2d_handle* h, const float* d_x, const float* d_y, size_t n, double leaf,
                               uint32_t min_points, float* d_ox, float* d_oy, uint32_t* d_count, size_t capacity,
                               ndt_voxel_filter_info* info);
/* the same with host arrays in and out, the cloud staged as ndt2d_fit_points stages its scan */
int32_t ndt2d_voxel_filter(ndt2d_handle* h, const float* x, const float* y, size_t n, double leaf, uint32_t min_points,
                           float* ox, float* oy, uint32_t* count, size_t capacity, ndt_voxel_filter_info* info);

/* ---- full alignment: rows a4-a9 ------------------------------------------------------ */
int32_t ndt2d_align(ndt2d_handle* h, const float* sx, const float* sy, size_t n,
                    const double init_pose[3], ndt2d_result* out);
/* Source already on the device.  Synchronous in the result (out is host memory). */
int32_t ndt2d_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                        const double init_pose[3], ndt2d_result* out);
/* Asynchronous form for timing and pipelining: returns as soon as the loop is under way on the
 * handle's stream; ndt2d_align_finish() waits and fetches.  With fixed_iterations > 0 the whole
 * loop is enqueued here; in converged mode the first launches are enqueued here and
 * ndt2d_align_finish() keeps the loop fed until it converges, so the d_sx / d_sy buffers must
 * stay valid until it returns (any other call on the handle finishes a loop in flight first).
 * Pipelining: consecutive fixed-iteration calls (scans above the short-scan limit, launch graphs on) may run
 * concurrently, up to four at a time: the handle sends them round its launch chains, so that every call fills the
 * launch gaps of the others (NDT_TUNE_ASYNC_CHAINS, three by default; 1 = one chain, calls run one after the other).
 * Each alignment stays what it is - own scan, own initial pose, bit-identical result; ndt2d_align_finish returns
 * the last call's result.  Every call's source arrays must stay valid until ndt2d_align_finish returns.
 * Stream contract: when this function returns, ndt2d_stream(h) is ordered behind this alignment and all earlier
 * ones, so an event recorded there afterwards covers them. */
int32_t ndt2d_align_dev_async(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                              const double init_pose[3]);
int32_t ndt2d_align_finish(ndt2d_handle* h, ndt2d_result* out);
/* Multi-scan: m (1..64) DIFFERENT scans against the cached grid, each from its own initial pose, in one
 * launch chain - several robots', or several recent, scans relocalised in one submap.  d_sx / d_sy / n
 * are host arrays of m device pointers / sizes; results[k] is bit for bit what ndt2d_align_dev returns for
 * scan k on the launch-per-iteration path.  This is the call that takes the 1M-point-target configuration
 * off the launch-latency floor with distinct data: 64 scans of 100k points move 64 x 3.2 MB of algorithmic
 * traffic per launch. */
int32_t ndt2d_align_multi_scan_dev(ndt2d_handle* h, const float* const* d_sx, const float* const* d_sy, const size_t* n,
                                   const double* init_poses, int32_t m, ndt2d_result* results);
/* Per-iteration trace, for debugging and stage-by-stage parity checks ("optional
 * per-iteration trace ... copied back on request"; never on a timed path: one plain launch and one state
 * fetch per iteration, always through the launch-per-iteration kernels).  rows[j], j < *n_rows <= capacity,
 * is the state after j + 1 updates: pose after them, H / g / score / n_hit of the evaluation that
 * produced the (j+1)-th update (taken at rows[j-1].pose, the initial pose for j = 0), iterations = j + 1,
 * status.  out (may be NULL) receives the final result, as ndt2d_align returns it.  Host arrays. */
int32_t ndt2d_align_trace(ndt2d_handle* h, const float* sx, const float* sy, size_t n, const double init_pose[3],
                          ndt2d_result* rows, int32_t capacity, int32_t* n_rows, ndt2d_result* out);
/* Multi-start: m (1..64) independent alignments of the SAME scan against the cached grid from m
 * initial poses (init_poses is [m][3], host memory), carried by ONE launch chain - the source points
 * are read once per launch and every point scores against every live pose, so m alignments cost little
 * more than one (the single alignment is bound by launch latency, DESIGN.md section 5.1: 8 starts cost
 * 1.9x one, 64 starts 6x).  For a loop-closure candidate with a poor guess: a grid of starts around
 * it, keep the best score.
 * results[k] is bit for bit what ndt2d_align_dev returns for init_poses[k] on the
 * launch-per-iteration path; a start that has finished is frozen while the others go on.
 * Synchronous in the results (host memory).  overlap_grids = 4: the same chain with four lookups per point (one start per
 * workgroup), every start still bit for bit its single alignment with the option. */
int32_t ndt2d_align_multi_start_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                    const double* init_poses, int32_t m, ndt2d_result* results);
/* Exhaustive pose search (docs/ALGORITHM.md "Exhaustive pose search"): the NDT score of the scan at every pose of an
 * (x, y, theta) lattice around a poor guess, against the cached grid, then the best well-separated peaks - for a
 * loop-closure candidate whose odometry has drifted by metres, or a robot relocalising in a map.
 * Lattice: n_x = 2 floor(hx/sx + 1e-9) + 1 poses at cx + i sx, i = -(n_x-1)/2 .. (n_x-1)/2, the same for y and for
 * theta when h_theta < pi; h_theta >= pi is a full turn: n_theta = max(1, floor(2 pi/s_theta + 0.5)) headings c_theta + j 2pi/n_theta,
 * j = 0 .. n_theta-1, a cyclic axis.  Headings are wrapped to (-pi, pi].  Flat index ((j n_y) + iy) n_x + ix; at most
 * 2^25 poses (NDT_ERR_CAPACITY above).  The score at a pose is the score ndt2d_evaluate_dev reports there (the same
 * float32 terms per point, summed in another order; overlap_grids honoured).
 * Peaks: score > 0 and beating every in-window neighbour of the 3x3x3 block (higher score, or equal score and lower
 * index; theta wraps on a cyclic axis only).  Hits: the best min(#peaks, 4096) peaks by (score desc, index asc),
 * walked in that order; a peak is dropped when an accepted hit lies closer than min_sep_trans in translation AND
 * closer than min_sep_rot in wrapped heading; at most k (1..64) hits.  Deterministic: the same inputs give the same
 * volume and hits bit for bit.  A window that misses the map returns NDT_OK with *n_hits = 0. */
typedef struct ndt2d_search_window {
  double center[3];       /* x, y, theta of the lattice's middle pose */
  double half_extent[3];  /* metres, metres, radians (>= 0; 0 pins the axis); theta >= pi: a full turn */
  double step[3];         /* lattice step per axis, > 0 */
  double min_sep_trans;   /* hits closer than this in translation ... */
  double min_sep_rot;     /* ... AND in rotation than an accepted hit are dropped (both >= 0) */
} ndt2d_search_window;

typedef struct ndt2d_search_hit {
  double pose[3];         /* lattice pose, theta wrapped to (-pi, pi] */
  float score;            /* the lattice score (float32, as in the volume) */
  int32_t index;          /* flat lattice index */
} ndt2d_search_hit;

/* dims = n_theta, n_y, n_x of the window's lattice (CPU only; the same validation as the searches) */
int32_t ndt2d_search_lattice_size(const ndt2d_search_window* w, int32_t dims[3]);
/* hits[0 .. *n_hits) (hits has room for k), best first.  Synchronous in the hits (host memory). */
int32_t ndt2d_search_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                         const ndt2d_search_window* w, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits);
/* the same with a host scan */
int32_t ndt2d_search(ndt2d_handle* h, const float* sx, const float* sy, size_t n,
                     const ndt2d_search_window* w, int32_t k, ndt2d_search_hit* hits, int32_t* n_hits);
/* the score volume itself into d_scores (device memory, n_theta x n_y x n_x floats, flat index order); returns once
 * it is written */
int32_t ndt2d_search_scores_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                const ndt2d_search_window* w, float* d_scores);
/* ndt2d_search_dev, then ndt2d_align_multi_start_dev from the hits' poses: results[i] is bit for bit what
 * ndt2d_align_multi_start_dev returns for those poses (results has room for k) */
int32_t ndt2d_search_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                               const ndt2d_search_window* w, int32_t k, ndt2d_search_hit* hits,
                               ndt2d_result* results, int32_t* n_hits);
/* Scoring a list of poses (docs/ALGORITHM.md "Scoring a list of poses"): the NDT score of the scan at every pose of a
 * list of any shape, in one launch - the weights of a particle filter's particles (NDT-MCL), relocalisation from outside
 * hypotheses, the samples of a caller's own search.  poses is [m][3] = (x, y, theta) in double; theta need not be wrapped.
 * Score: scores[i] is the score ndt2d_evaluate_dev reports for the scan at poses[3i .. 3i+2] - per point the float32
 * operations of the single-pose path, summed in another order, the contract of ndt2d_search_scores_dev: the heading is
 * wrapped, its cos / sin taken in double and rounded to float32, the translation is the float of the double, the cell
 * key is clamped onto the grid's empty ring, and overlap_grids = 4 is honoured (four lookups per point).  NaN points of
 * the scan add nothing.  A pose with a non-finite coordinate scores exactly +0.0f (a device list cannot be validated on
 * the host, and 0 is the weight a particle filter wants for it) and never becomes a hit.  So does a finite pose whose
 * float32 form is not finite: a translation beyond float32's range, an angle so large that wrapping leaves no finite sine
 * and cosine (in 3D: a non-finite entry of R).  No pose of a list gives a NaN score.
 * Bitwise: a pose's score depends on nothing but the handle's grid, the scan and that pose - not on its position in the
 * list, nor on the rest of the list - and two calls give the same bits.  A list that holds the lattice of a search window
 * in flat index order, with the axes' doubles of that lattice, gives the volume of ndt2d_search_scores_dev bit for bit
 * (every pose is summed in the search kernel's order).
 * Best poses: candidates are the poses with score > 0; the best min(#candidates, 4096) by (score descending, index
 * ascending) are walked in that order; a candidate is dropped when an accepted hit lies closer than min_sep_trans in
 * translation (Euclidean over x, y) AND closer than min_sep_rot in rotation (|wrap(dtheta)|), both strictly; at most k
 * (1..64) hits.  hits[q].pose is the list's pose at hits[q].index bit for bit (not wrapped), hits[q].score its float32
 * score.  Deterministic to the bit.  A list without a positive score gives NDT_OK and *n_hits = 0.
 * ndt2d_best_poses_align_dev then refines the hits in one ndt2d_align_multi_start_dev call: results[q] is bit for bit
 * what that call returns for the hits' poses; nothing is launched for zero hits.
 * Streams and state: as ndt2d_search_scores_dev - on the handle's stream, behind an asynchronous alignment in flight
 * (which is finished first), returning once the outputs are complete; producers of the scan and of the list are ordered
 * by ndt2d_wait_stream.  The handle's grid, parameters and later alignments are untouched.
 * Errors, found before any device call: a null handle, scan, list or output, n = 0 or above what an alignment takes,
 * m = 0, k outside 1..64, a separation that is NaN, infinite or negative: NDT_ERR_INVALID_ARG; m > 2^25:
 * NDT_ERR_CAPACITY (the search's cap: index and key share 32 bits); no grid: NDT_ERR_NO_TARGET.  A grid without a valid
 * cell is no error: every score is 0. */
int32_t ndt2d_score_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                              const double* d_poses /* device, [m][3] */, size_t m, float* d_scores /* device, [m] */);
/* the same with a host scan, a host list and host scores (staged through the handle's scratch) */
int32_t ndt2d_score_poses(ndt2d_handle* h, const float* sx, const float* sy, size_t n,
                          const double* poses, size_t m, float* scores);
/* hits[0 .. *n_hits) (hits has room for k), best first.  Synchronous in the hits (host memory). */
int32_t ndt2d_best_poses_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n, const double* d_poses,
                             size_t m, double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                             int32_t* n_hits);
/* ndt2d_best_poses_dev, then ndt2d_align_multi_start_dev from the hits' poses (results has room for k) */
int32_t ndt2d_best_poses_align_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                   const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                                   ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits);
/* Scoring particles (docs/ALGORITHM.md "Scoring particles: a team of lanes per pose"): ndt2d_score_poses_dev for SHORT
 * lists - the few hundred to few thousand particles of a particle filter - with the hit count beside the score and an
 * asynchronous form.  Where ndt2d_score_poses_dev gives every pose one lane, which walks the whole scan, these give every
 * pose a team of 64 or 256 lanes, which share the scan's points between them.
 * Score: the pose is formed as ndt2d_score_poses_dev forms it, and every point's term is that call's bit for bit (NaN
 * points add nothing, a non-finite pose or one whose float32 form is not finite scores exactly +0.0f with count 0, no
 * score is NaN).  scores[i] differs from ndt2d_score_poses_dev's ONLY by the order of the float32 summation, which is
 * the one ALGORITHM states over 256 virtual lanes (per-lane sums in point order, a fixed pairing of the four quarters, a
 * xor butterfly over 64 lanes).  Both sums add the same n * overlap_grids non-negative terms, so they agree to within
 * 2 * n * overlap_grids * 2^-24 relative, and bit for bit for n <= 2.
 * n_hit[i] (d_n_hit may be NULL: not written) is the number of (point, grid) lookups that hit a valid cell: exactly what
 * ndt2d_evaluate_dev reports as n_hit at that pose - what tells a good fit from a small overlap.
 * Bitwise: a score and a count depend on nothing but the handle's grid, the scan and that pose - not on the pose's
 * position in the list, not on the list's length, not on the team width (NDT_TUNE_PARTICLE_TEAM) - and two calls give the
 * same bits.
 * Which call: ndt2d_score_particles* for every list that does not need ndt2d_score_poses_dev's bits.  Measured (DESIGN
 * 5.19, MI355X, host to host) it is the faster call at every list size from 256 to 1 048 576 poses, in 2D and in 3D: 4096
 * particles take 0.05 ms against 0.22 ms (2D, 1440 points) and 0.20 ms against 3.5 ms (3D, 16 384 points); from 65 536
 * poses on, where one lane per pose fills the device too, it keeps an edge of 1.3x to 1.5x.  No list size was found from
 * which ndt2d_score_poses_dev is faster.  That call remains the one whose scores are the search volume's bit for bit, and
 * the one ndt2d_best_poses* select from.
 * _dev: on the handle's stream, behind an asynchronous alignment in flight (which is finished first); returns when the
 * outputs are complete.  Argument checks and error codes are those of ndt2d_score_poses_dev.
 * _async: the same checks and the same launch, returning after the enqueue: the outputs are complete in stream order on
 * ndt2d_stream(h), and the scan, the list and the outputs must stay alive until then.  Producers on other streams are
 * ordered with ndt2d_wait_stream, as for every device entry point.
 * ndt2d_score_particles: host scan, host list, host scores and counts (staged through the handle's scratch). */
int32_t ndt2d_score_particles_dev(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                  const double* d_poses /* device, [m][3] */, size_t m, float* d_scores /* device, [m] */,
                                  uint32_t* d_n_hit /* device, [m], may be NULL */);
int32_t ndt2d_score_particles_async(ndt2d_handle* h, const float* d_sx, const float* d_sy, size_t n,
                                    const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit);
int32_t ndt2d_score_particles(ndt2d_handle* h, const float* sx, const float* sy, size_t n,
                              const double* poses, size_t m, float* scores, uint32_t* n_hit /* may be NULL */);
/* ---- map-to-map alignment (distribution-to-distribution NDT; docs/ALGORITHM.md section 2.13) ----------------
 * Aligns the cached grid of `source` to the cached grid of `target` without any of the points either was built from:
 * what a handle keeps after ndt2d_add_target_points_dev, and all that ndt2d_save_map / ndt2d_load_map persist, is
 * enough.  The source is the list of its valid cells' Gaussians (mean, regularised covariance: its *components*, in
 * cell-key order), each scored against the target Gaussian of the cell its transformed mean falls in, with the combined
 * covariance R S_i R^T + S_j; every hit weighs the same.  pose = (tx, ty, theta) maps the source map's frame into the
 * target map's frame.
 *   - The TARGET handle's parameters drive the solve (d1, d2, hessian_mode, the limits and stops, step_scale,
 *     line_search, its tuning knobs, its stream); the source handle's min_points / eig_ratio decide only its
 *     components.  The cell sizes may differ.  step_scale: the Gauss-Newton Hessian of this objective is close to
 *     the true one, so factors much above 1.5 over-relax and do not converge.
 *   - target == source is legal (a map against itself: the identity is a fixed point).
 *   - Both handles must live on the same device and neither may have overlap_grids = 4: NDT_ERR_INVALID_ARG.
 *     No grid on either handle: NDT_ERR_NO_TARGET.  A non-finite pose: NDT_ERR_INVALID_ARG.  A source without a
 *     component or a target without a valid cell: NDT_OK with status NDT_TOO_FEW_CELLS and the initial pose
 *     (ndt2d_evaluate_map: all zeros).
 *   - Both calls are synchronous; the target's stream is ordered behind the source's by the library.  The derived
 *     per-handle data (covariance records, component list) is built on a handle's first such call and again after
 *     anything that changes its grid.  Results are bit for bit reproducible from call to call.
 *   - ndt2d_result / ndt2d_eval are those of ndt2d_align / ndt2d_evaluate (n_hit counts components that hit a valid
 *     target cell).  ndt2d_calibrated_covariance accepts the H returned here, but its factors were calibrated for
 *     the point-to-distribution objective: they are NOT calibrated for this one. */
int32_t ndt2d_evaluate_map(ndt2d_handle* target, ndt2d_handle* source, const double pose[3], ndt2d_eval* out);
int32_t ndt2d_align_map(ndt2d_handle* target, ndt2d_handle* source, const double init_pose[3], ndt2d_result* out);
/* m (1..64) map-to-map alignments against ONE target in one launch chain: start k aligns sources[k] from
 * init_poses[3k .. 3k+2].  The same handle m times is a multi-start (a loop closure with a poor guess); different
 * handles are several submaps relocalised against one older submap; sources[k] may be `target`.
 *   - results[k] is bit for bit what ndt2d_align_map(target, sources[k], &init_poses[3k], ...) returns, whatever
 *     hessian_mode, fixed or converged mode, max_iterations, step_scale, line_search and the tuning knobs are; a start
 *     that has finished is frozen while the others go on.
 *   - The target handle's parameters, stream and tuning drive the call, as for ndt2d_align_map.  Synchronous: it
 *     returns once nothing reads any source's component list any more.
 *   - Errors of the whole call, found before anything is enqueued (the handles stay usable): a null pointer, a null
 *     entry of sources, m outside 1..64 (these three before any device call), a non-finite pose, overlap_grids = 4 on
 *     any handle, handles on different devices: NDT_ERR_INVALID_ARG; a handle without a grid: NDT_ERR_NO_TARGET.
 *   - Inside an NDT_OK call: a source without a component gives ITS start status NDT_TOO_FEW_CELLS and its initial
 *     pose while the others run; a target without a valid cell gives that to every start.
 * Pairs with different targets are not covered (one call per target).  The 3D twin is ndt3d_align_map_multi. */
int32_t ndt2d_align_map_multi(ndt2d_handle* target, ndt2d_handle* const* sources, const double* init_poses /* [m][3] */,
                              int32_t m, ndt2d_result* results /* [m] */);
/* Exhaustive pose search for map-to-map alignment (docs/ALGORITHM.md section 2.17): the score ndt2d_evaluate_map
 * reports (the same float32 terms per component, summed in another order) at every pose of the window's lattice, then
 * the best well-separated peaks - a loop closure between two submaps whose relative pose is known to metres and not at
 * all in heading.  Window, lattice, hits, k in 1..64, the window errors and bitwise determinism are those of
 * ndt2d_search above; handles, devices, overlap_grids and target == source are as for ndt2d_align_map (d1, d2: the
 * target handle's).  A source without a component or a target without a valid cell gives an all-zero volume and no
 * hit.  All three are synchronous: they return once nothing reads the source's component list any more.
 * ndt2d_search_map_scores writes the volume [n_theta][n_y][n_x] into device memory.  ndt2d_search_align_map refines
 * all hits in one ndt2d_align_map_multi call (nothing is launched for zero hits): results[q] is bit for bit what
 * ndt2d_align_map(target, source, hits[q].pose) returns (hits and results have room for k). */
int32_t ndt2d_search_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w,
                         int32_t k, ndt2d_search_hit* hits, int32_t* n_hits);
int32_t ndt2d_search_map_scores(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w,
                                float* d_scores);
int32_t ndt2d_search_align_map(ndt2d_handle* target, ndt2d_handle* source, const ndt2d_search_window* w,
                               int32_t k, ndt2d_search_hit* hits, ndt2d_result* results, int32_t* n_hits);
/* Scoring a map at a list of poses (docs/ALGORITHM.md section 2.21): the map-to-map score of `source` against `target`
 * at every pose of a list of any shape, in one launch - the particles of a submap-level filter, a caller's own samples
 * round a place-recognition hypothesis, a search over axes the lattice of ndt2d_search_map does not have.  poses is
 * [m][3] = (x, y, theta) in double; theta need not be wrapped.
 * Score: scores[i] is the score ndt2d_evaluate_map(target, source, poses[3i .. 3i+2]) reports - the same float32 terms per
 * component, summed in another order; the arithmetic per component is that of ndt2d_search_map_scores with the heading's
 * share done per pose: the angle is wrapped, its cos / sin taken in double and rounded to float32, the translation is
 * the float of the double.  d1 and d2 are the target handle's.
 * Hit count: n_hit[i] (may be NULL) is the number of source components whose image falls in a valid target cell: exactly
 * ndt2d_evaluate_map's n_hit at that pose.  It tells a high score from a large overlap; its ratio to the component count
 * (ndt2d_get_components) is the gate a loop closure wants.  Asking for it changes no score bit.
 * A pose with a non-finite coordinate scores exactly +0.0f with n_hit 0 and never becomes a hit; so does a finite pose
 * whose float32 form is not finite (a translation beyond float32, an angle whose wrap leaves no finite sine and cosine).
 * No pose of a list gives a NaN.
 * Bitwise: a pose's score and count depend on nothing but the two grids and that pose - not on its position in the list,
 * nor on the rest of the list - and two calls give the same bits.  A list that holds the lattice of a search window in
 * flat index order, with the axes' doubles of that lattice (angles in (-pi, pi]), gives the volume of
 * ndt2d_search_map_scores bit for bit.
 * Best poses: the rule of ndt2d_best_poses_dev - candidates have score > 0, the best min(#candidates, 4096) by (score
 * descending, index ascending) are walked, a candidate is dropped when an accepted hit lies closer than min_sep_trans
 * AND closer than min_sep_rot (both strictly), at most k (1..64) hits; hits[q].pose is the list's row bit for bit.
 * ndt2d_best_map_poses_align_dev then refines all hits in one ndt2d_align_map_multi call: results[q] is bit for bit what
 * ndt2d_align_map(target, source, hits[q].pose) returns; nothing is launched for zero hits.
 * Handles, streams and state: as ndt2d_search_map - the derived data of both handles is ensured, target == source is
 * legal, everything runs on the target's stream, behind the source's and behind an alignment in flight (which is
 * finished first); a call returns once the outputs are complete and nothing reads the source's component list any more.
 * The list's producer is ordered by ndt2d_wait_stream(target, ...).  Grids, parameters and later calls are untouched.
 * Errors, found before any device call: a null handle, list or score output, m = 0, k outside 1..64, a null hits,
 * n_hits or results, a separation that is NaN, infinite or negative: NDT_ERR_INVALID_ARG; m > 2^25: NDT_ERR_CAPACITY;
 * no grid on either handle: NDT_ERR_NO_TARGET; overlap_grids = 4 on either handle or handles on different devices:
 * NDT_ERR_INVALID_ARG.  A source without a component or a target without a valid cell is no error: every score is 0 and
 * there are no hits.  *n_hits is 0 wherever it could be written. */
int32_t ndt2d_score_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses /* device, [m][3] */,
                                  size_t m, float* d_scores /* device, [m] */, uint32_t* d_n_hit /* device, [m]; may be NULL */);
/* the same with a host list and host outputs (staged through the target's scratch) */
int32_t ndt2d_score_map_poses(ndt2d_handle* target, ndt2d_handle* source, const double* poses, size_t m,
                              float* scores, uint32_t* n_hit /* may be NULL */);
/* hits[0 .. *n_hits) (hits has room for k), best first.  Synchronous in the hits (host memory). */
int32_t ndt2d_best_map_poses_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m,
                                 double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                 int32_t* n_hits);
/* ndt2d_best_map_poses_dev, then ndt2d_align_map_multi from the hits' poses (results has room for k) */
int32_t ndt2d_best_map_poses_align_dev(ndt2d_handle* target, ndt2d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt2d_search_hit* hits,
                                       ndt2d_result* results, int32_t* n_hits);
/* The components of a handle's cached grid, as host copies: mean_xy [2n], cov_abc [3n] = (Sxx, Sxy, Syy), key [n] =
 * iy * width + ix, ascending.  Any pointer may be NULL; *n (if given) is the count, also when capacity is too small
 * for the arrays asked for (NDT_ERR_CAPACITY). */
int32_t ndt2d_get_components(ndt2d_handle* h, float* mean_xy, float* cov_abc, int32_t* key, int32_t capacity, int32_t* n);

/* Execution-strategy knobs of a handle.  They choose between kernels that compute the same alignment
 * (results agree up to float32 summation order; the tests pin each pair of choices against each other
 * and against the oracle); the defaults are the measured best, nothing reads the environment.
 *   NDT_TUNE_LAUNCH_GRAPHS      1 (default): launch chains are hipGraph replays; 0: plain launches
 *   NDT_TUNE_WIDE_THRESHOLD     source points from which k_iterate runs on 1024-thread workgroups
 *                               (default 300000); 0: never
 *   NDT_TUNE_SHORT_SCAN_KERNEL  1 (default): scans of <= 4096 points run the whole loop in one workgroup
 *   NDT_TUNE_CHUNK_LAUNCHES     converged mode: launches per graph replay, 2..128 (default 8)
 *   NDT_TUNE_BINNED_BUILD       1 (default): LDS-binned grid build; 0: scattered global atomics
 *   NDT_TUNE_SPLIT_FROM         multi-start / multi-scan calls of at least this many starts run two kernels per
 *                               iteration (one workgroup per start solves, then everybody evaluates) instead of
 *                               the fused kernel whose every workgroup repeats its starts' solves (default 12)
 *   NDT_TUNE_SINGLE_SYNC_BUILD  1 (default): ndt2d_set_target on a handle that already holds a grid decides the new grid's
 *                               geometry on the device and enqueues the whole build at once (one host round trip;
 *                               it falls back by itself when the new grid does not fit the cached storage).
 *                               0: bounding box to the host first, then the build (two round trips)
 *   NDT_TUNE_ASYNC_CHAINS       the number of launch chains (streams of the handle) that consecutive fixed-iteration
 *                               ndt2d_align_dev_async calls go round, 1..4 (default 3): that many of them overlap.
 *                               1: one stream, one call after the other (for a caller that shares the GPU and wants
 *                               one queue).  Other values: NDT_ERR_INVALID_ARG.  Results are bit-identical whatever
 *                               the count.  ndt2d_set_tuning only
 *   NDT_TUNE_ASYNC_LANES        the same count under its earlier name, 1 or 2 only: 2: such calls overlap in pairs on
 *                               two streams of the handle; 1: one stream.  Other values: NDT_ERR_INVALID_ARG (a count
 *                               of 3 or 4 is set with NDT_TUNE_ASYNC_CHAINS)
 *   NDT_TUNE_MAP_MULTI_FROM     ndt2d_align_map_multi calls of at least this many starts run one launch chain for all
 *                               starts; smaller calls run one ndt2d_align_map chain per start (default 2; 1..65, 65:
 *                               never the shared chain).  Results are bit-identical either way.  The same knob, range
 *                               and default on ndt3d_set_tuning for ndt3d_align_map_multi
 *   NDT_TUNE_FUSED_BEGIN        1 (default): the first launch of a single-scan alignment takes the call's arguments and
 *                               evaluates at the initial pose itself (K + 1 launches for K iterations); 0: a small
 *                               kernel writes the arguments into the device context first (K + 2 launches, the protocol
 *                               ndt2d_align_trace always runs).  Other values: NDT_ERR_INVALID_ARG.  Results are
 *                               bit-identical either way.  The same knob on ndt3d_set_tuning
 *   NDT_TUNE_LANE_FORK          0 (default): the further streams of NDT_TUNE_ASYNC_CHAINS >= 2 wait for the handle's stream
 *                               only where something other than such an alignment (a build, an update, a synchronous or
 *                               converged call, a tuning change) precedes a round of them, and run their alignments back
 *                               to back otherwise; 1: each waits for the head of the round's first call at every round.  Other values:
 *                               NDT_ERR_INVALID_ARG.  Results are bit-identical either way.  ndt2d_set_tuning only
 *   NDT_TUNE_PARTICLE_TEAM      lanes per pose of ndt2d_score_particles*: 0 (default): 256 (one workgroup per pose) for lists
 *                               of fewer than 2048 poses and 64 (one wave per pose) from there on - below 256 CUs x 4
 *                               SIMDs = 1024 poses one wave per pose leaves SIMDs empty, and the wide team was measured
 *                               ahead up to 1024 and behind from 2048; 64 or 256: that width for every list.
 *                               Other values: NDT_ERR_INVALID_ARG.  Scores and counts are bit-identical either way.  The
 *                               same knob on ndt3d_set_tuning for ndt3d_score_particles*
 *   NDT_TUNE_BATCH_SMALL_VARIANT (batch contexts) 1 (default): lidar-sized pairs run on the 256-thread
 *                               variant of the batch kernel first; 0: every pair on the 1024-thread one
 *   NDT_TUNE_BATCH_GLOBAL_WORKGROUPS (batch contexts, 2D and 3D) workgroups of the global-table variant, each with its own
 *                               table slab in device memory (3.7 MB in 2D, 7.9 MB in 3D): 1..256.  Unset, a context starts
 *                               with 8 (30 MB / 63 MB) and grows ONCE to one per CU (0.95 GB / 2.0 GB) at the start of the
 *                               first call after one in which a pair needed that variant - a context whose pairs all fit
 *                               on chip never pays for it; the call that first meets over-capacity pairs runs them on the
 *                               8.  Setting the knob fixes the number (64: a batch of over-capacity pairs about 2.8x
 *                               slower than on 256).  Results do not depend on it */
enum {
  NDT_TUNE_LAUNCH_GRAPHS = 1,
  NDT_TUNE_WIDE_THRESHOLD = 2,
  NDT_TUNE_SHORT_SCAN_KERNEL = 3,
  NDT_TUNE_CHUNK_LAUNCHES = 4,
  NDT_TUNE_BINNED_BUILD = 5,
  NDT_TUNE_BATCH_SMALL_VARIANT = 6,
  /* 7: was the one-XCD team kernel of round 2 (measured slower than the default, moved to tools/experiments) */
  NDT_TUNE_SPLIT_FROM = 8,
  NDT_TUNE_SINGLE_SYNC_BUILD = 9,
  NDT_TUNE_BATCH_GLOBAL_WORKGROUPS = 10,
  NDT_TUNE_ASYNC_LANES = 11,
  NDT_TUNE_MAP_MULTI_FROM = 12,
  NDT_TUNE_FUSED_BEGIN = 13,
  NDT_TUNE_LANE_FORK = 14,
  NDT_TUNE_ASYNC_CHAINS = 15,
  NDT_TUNE_PARTICLE_TEAM = 16
};
int32_t ndt2d_set_tuning(ndt2d_handle* h, int32_t knob, int64_t value);
/* hipStream_t the handle enqueues on (as void*), for event timing by the caller */
void* ndt2d_stream(ndt2d_handle* h);
/* Stream ordering of the device-pointer entry points.  A handle enqueues on its own non-blocking
 * stream, which is NOT ordered against the stream that produced the caller's device arrays (torch's
 * current stream, a driver's stream, the stream given to ndt2d_polar_to_points_dev).
 * ndt2d_wait_stream orders everything the handle enqueues after this call behind the work that is
 * in producer_stream now (event record + stream wait: the host does not block; NULL = the legacy
 * default stream).  Call it before ndt2d_align_dev / ndt2d_align_dev_async whenever the source
 * arrays were written on a stream that has not been synchronised - ANY stream, the handle's own
 * (ndt2d_stream) included: an asynchronous fixed-iteration alignment may run on one of the handle's further
 * streams (NDT_TUNE_ASYNC_CHAINS), which is ordered behind the caller's work on ndt2d_stream only by
 * ndt2d_wait_stream(h, ndt2d_stream(h)).
 * (ndt2d_set_target_dev and ndt2d_add_target_points_dev take the producer stream themselves.) */
int32_t ndt2d_wait_stream(ndt2d_handle* h, void* producer_stream);

/* ---- either side of the path --------------------------- */
/* Magnusson's outlier-mixture score constants (PhD thesis 2009, eq. 6.8-6.10) expressed as the
 * d1, d2 of ndt2d_params: with c1 = 10(1 - p_o), c2 = p_o / cell^dim, d3 = -ln c2,
 * d1 = -ln(c1 + c2) - d3, d2 = -2 ln((-ln(c1 e^-1/2 + c2) - d3) / d1).  The library maximises
 * sum d1' exp(-d2/2 m) with d1' = -d1 > 0, which is what is returned in *d1.  dim is 2 or 3. */
int32_t ndt_magnusson_constants(double outlier_ratio, double cell_size, int32_t dim, double* d1, double* d2);

/* Pose covariance for a factor-graph noise model from the Hessian an
 * alignment returned: cov = S H^-1 S with S = diag(s_t, s_t, s_r).  H^-1 itself is NOT the covariance
 * of the estimate: the score is a robust sum over cells, not a likelihood of independent points, and
 * its piecewise-smooth surface makes the fixed point of the iteration several times more sensitive to
 * the sampling of both scans than the local curvature says.  The factors are calibrated by Monte-Carlo
 * over noise realisations of both scans (tests/test_gpu_covariance.py):
 *   Gauss-Newton Hessian:  s_t^2 = 10,  s_r^2 = 18        Newton Hessian:  s_t^2 = 3.9,  s_r^2 = 7.5
 * and put the calibrated covariance within a factor 2.5 of the empirical one (every eigenvalue of
 * C_empirical C_calibrated^-1 in [0.4, 2.5]; the test asserts a factor 3) on scans with some 20 or more
 * points per occupied cell; the excess over H^-1 is discretisation noise and grows as the scans get
 * sparser (up to 5.5x off at 7 points per cell: inflate further there).  Needs no device.
 * The factors are those of point-to-map alignment; for the H of ndt2d_align_map they are not calibrated.
 * Returns NDT_DEGENERATE_HESSIAN (cov zeroed) when H is not positive definite. */
#define NDT_COV_SCALE_GN_TRANS 10.0
#define NDT_COV_SCALE_GN_ROT 18.0
#define NDT_COV_SCALE_NEWTON_TRANS 3.9
#define NDT_COV_SCALE_NEWTON_ROT 7.5
int32_t ndt2d_calibrated_covariance(const double H[9], int32_t hessian_mode, double cov[9]);

/* Range/bearing scan -> SoA Cartesian points on the device (the driver side of the boundary):
 * x[i] = r[i] cos(angle_min + i*angle_inc), y likewise; ranges outside [range_min, range_max]
 * or non-finite become NaN points, which every entry point of this library ignores.
 * All pointers are device pointers; asynchronous on `stream` (NULL = default stream). */
int32_t ndt2d_polar_to_points_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc,
                                  double range_min, double range_max, float* d_x, float* d_y, void* stream);

/* ---- loop-closure candidate batch (BASELINE config 4) -------------- */
/* Independent scan pairs, aligned concurrently: one persistent workgroup per CU pulls pairs
 * from a queue, builds the pair's target grid in LDS and runs its whole Gauss-Newton loop on
 * chip.  Clouds are concatenated SoA arrays; pair k owns target points [toff[k], toff[k+1])
 * and source points [soff[k], soff[k+1]); init is [n_pairs][3]; results is [n_pairs].
 * A pair whose grid exceeds the on-chip capacity (more than 20480 cells or 2559 occupied cells, e.g. a
 * scan against a submap wider than 71 m at 0.5 m cells) is handed, on the device and within the same
 * call, to a third variant of the kernel that keeps the pair's tables in global memory (up to 512 x 512
 * cells, 32767 occupied: 256 m x 256 m at 0.5 m cells).  Beyond that a pair gets status
 * NDT_ERR_CAPACITY from the _dev entry point, and the host-pointer entry point re-runs it through the
 * single-pair path transparently.
 * A cell that more than 2^20 target points of a pair fall into: where ndt2d_set_target answers
 * NDT_ERR_CAPACITY for the whole cloud, the batch kernels (2D and 3D, every variant) make that one cell invalid -
 * a source point in it is a miss - and align the pair on the other cells; the pair's status says nothing about it
 * (tests/test_gpu_batch_records.py).
 * overlap_grids = 4: every pair of such a level runs on that third variant (four grids on chip would quarter
 * the capacity to 71 x 71 cells), its four grids back to back in the tables: 256 x 256 cells per grid
 * (128 m x 128 m at 0.5 m cells), 32767 occupied cells over the four; the context then holds one table slab
 * per CU from creation (0.95 GB).  Results equal ndt2d_align's with the same option up to float32 summation
 * order (tests/test_gpu_batch_overlap.py). */
typedef struct ndt2d_batch ndt2d_batch;
int32_t ndt2d_batch_create(const ndt2d_params* p, int32_t device_id, ndt2d_batch** out);
/* Coarse-to-fine over the batch (loop-closure candidates start from poor guesses): levels[0..n)
 * ordered coarse to fine, at most 8; every pair runs level 0 from its init and each later level
 * from the pose the previous one reached; a level that ends with a status other than NDT_OK /
 * NDT_NOT_CONVERGED ends the pair with that status; iterations are summed over levels and
 * H, g, score, n_hit are those of the last level run.  One kernel launch per level, the clouds
 * stay where they are.  ndt2d_default_pyramid fills the standard 3-level schedule (4c, 2c, c). */
int32_t ndt2d_default_pyramid(const ndt2d_params* fine, ndt2d_params levels[3]);
int32_t ndt2d_batch_create_pyramid(const ndt2d_params* levels, int32_t n_levels, int32_t device_id, ndt2d_batch** out);
int32_t ndt2d_batch_destroy(ndt2d_batch* b);
int32_t ndt2d_batch_align(ndt2d_batch* b, const float* tx, const float* ty, const uint64_t* toff,
                          const float* sx, const float* sy, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt2d_result* results);
/* All pointers are device pointers (results too).  Asynchronous on `stream` (NULL = the
 * context's own stream): the results are valid once that stream is synchronised.  Calls on one
 * context share its dequeue counters and pair marks, so they must be ordered with respect to each
 * other (the same stream, or synchronised streams); use one context per concurrent stream. */
int32_t ndt2d_batch_align_dev(ndt2d_batch* b, const float* d_tx, const float* d_ty, const uint64_t* d_toff,
                              const float* d_sx, const float* d_sy, const uint64_t* d_soff,
                              const double* d_init, size_t n_pairs, ndt2d_result* d_results, void* stream);
void* ndt2d_batch_stream(ndt2d_batch* b);
int32_t ndt2d_batch_set_tuning(ndt2d_batch* b, int32_t knob, int64_t value);   /* NDT_TUNE_BATCH_SMALL_VARIANT, _GLOBAL_WORKGROUPS */
/* as ndt2d_wait_stream, for calls that run on the context's own stream (stream == NULL above) */
int32_t ndt2d_batch_wait_stream(ndt2d_batch* b, void* producer_stream);
/* Of the pairs of the last ndt2d_batch_align() call, how many ran on the 1024-thread variant of
 * the kernel (the rest fitted the 256-thread variant for lidar-sized scans: clouds of at most 8192
 * points, at most 767 occupied cells); -1 before the first call.  Diagnostic. */
int64_t ndt2d_batch_last_large_count(const ndt2d_batch* b);

/* The same batch over several devices from ONE host process (a C++ SLAM back end that owns the
 * node's GPUs itself): one batch context and one host thread per device, pairs split into
 * contiguous work-balanced shards, results written into the caller's array.  Pairs are
 * independent, so no data moves between devices.  device_ids == NULL with n_devices == 0 means
 * every visible device; an id may be listed more than once (two contexts on that device; not with
 * the RCCL gather of ndt2d_multi_align_dev).  (The one-process-per-GPU deployment is
 * gtsam_ndt_amd/dist.py: the same sharding, the gather through torch.distributed's RCCL backend.) */
typedef struct ndt2d_multi ndt2d_multi;
int32_t ndt2d_multi_create(const ndt2d_params* p, const int32_t* device_ids, int32_t n_devices, ndt2d_multi** out);
int32_t ndt2d_multi_create_pyramid(const ndt2d_params* levels, int32_t n_levels, const int32_t* device_ids,
                                   int32_t n_devices, ndt2d_multi** out);
int32_t ndt2d_multi_destroy(ndt2d_multi* m);
int32_t ndt2d_multi_device_count(const ndt2d_multi* m);
/* Arguments as ndt2d_batch_align (host pointers).  Returns the first failing shard's status. */
int32_t ndt2d_multi_align(ndt2d_multi* m, const float* tx, const float* ty, const uint64_t* toff,
                          const float* sx, const float* sy, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt2d_result* results);
/* Device-resident form with the RCCL gather: shard d's clouds are already on device d (arrays of
 * n_devices device pointers, each laid out as ndt2d_batch_align_dev takes it; n_pairs[d] pairs on
 * device d, 0 allowed).  Every context aligns its shard on its own stream and the result rows of all
 * shards are exchanged with ONE ncclAllGather over those streams (xGMI on a multi-GPU node), so that
 * every device ends up holding every row - no result passes through host memory on the way.
 * Layout of a gathered copy: row k of shard d at index d * (*shard_stride) + k, *shard_stride = the
 * longest shard (shorter shards are zero-padded).  d_results_all[d] (may be NULL) receives device d's
 * copy - owned by the context, valid until its next call; results (may be NULL, host memory,
 * sum of n_pairs rows) receives the rows in global pair order without padding.  Synchronous.
 * The communicators are created on the first call (ncclCommInitAll: one process, one rank per
 * context, distinct devices required); RCCL failures return NDT_ERR_RCCL. */
int32_t ndt2d_multi_align_dev(ndt2d_multi* m, const float* const* d_tx, const float* const* d_ty,
                              const uint64_t* const* d_toff, const float* const* d_sx, const float* const* d_sy,
                              const uint64_t* const* d_soff, const double* const* d_init, const size_t* n_pairs,
                              ndt2d_result** d_results_all, size_t* shard_stride, ndt2d_result* results);
/* The split ndt2d_multi_align uses: shard d owns pairs [shard_begin[d], shard_begin[d+1]);
 * shard_begin has n_shards + 1 entries.  Work of a pair = 3 x target points + iterations_hint x
 * source points (iterations_hint <= 0: 30).  Needs no device. */
int32_t ndt2d_multi_plan(int32_t n_shards, const uint64_t* toff, const uint64_t* soff, size_t n_pairs,
                         int32_t iterations_hint, uint64_t* shard_begin);
/* The same split with a per-pair work hint (pairs of a converged-mode batch need different numbers
 * of iterations - 14 to 53 in this repository's tests): pair_iterations[k] > 0 replaces iterations_hint for pair k
 * (NULL: ndt2d_multi_plan).  For callers that place device-resident shards themselves (ndt2d_multi_align_dev). */
int32_t ndt2d_multi_plan_hinted(int32_t n_shards, const uint64_t* toff, const uint64_t* soff, size_t n_pairs,
                                int32_t iterations_hint, const int32_t* pair_iterations, uint64_t* shard_begin);

/* ---- 3D NDT, SE(3) (BASELINE config 5) ----------------------- */
/* Same pipeline in 3D: dense voxel grid with per-cell mean / 3x3 covariance (eigenvalue clamp
 * by a fixed-sweep Jacobi), pose = (tx, ty, tz, roll, pitch, yaw) with R = Rz(yaw) Ry(pitch)
 * Rx(roll), 6x6 Hessian (Gauss-Newton, or the full Newton form of Magnusson 2009 eq. 6.13 with
 * hessian_mode = NDT_HESSIAN_NEWTON), 6-vector gradient.  ndt3d_params has the layout and
 * meaning of ndt2d_params (overlap_grids is a 2D option). */
typedef ndt2d_params ndt3d_params;

typedef struct ndt3d_result {
  double pose[6];     /* tx ty tz roll pitch yaw                                  */
  double H[36];       /* row-major 6x6 Hessian (the form hessian_mode selects) at the last evaluation */
  double g[6];
  double score;
  int32_t iterations, n_hit, status, reserved;
} ndt3d_result;

typedef struct ndt3d_eval {
  double H[36];
  double g[6];
  double score;
  int32_t n_hit, reserved;
} ndt3d_eval;

typedef struct ndt3d_grid_info {
  float ox, oy, oz, inv_cell;
  int32_t width, height, depth;
  int32_t n_valid;
} ndt3d_grid_info;

typedef struct ndt3d_handle ndt3d_handle;
void ndt3d_default_params(ndt3d_params* p);   /* cell 1.0 m, min_points 5, step_max_trans 1.0, min_hits 6 */
int32_t ndt3d_create(const ndt3d_params* p, int32_t device_id, ndt3d_handle** out);
int32_t ndt3d_destroy(ndt3d_handle* h);
int32_t ndt3d_set_target(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n);
/* Incremental submap update, as ndt2d_add_target_points: bins n more points into the cached voxel
 * grid's exact sums and re-finalises; points outside the cached extent are counted and ignored. */
int32_t ndt3d_add_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n,
                                size_t* n_outside);
/* Range image of a spinning multi-beam lidar -> SoA Cartesian points on the device (the driver side of the 3D
 * boundary, as ndt2d_polar_to_points_dev): d_ranges is [n_elev][n_azim] row-major, n_elev <= 128; ring e looks up
 * at elevations[e] (host array, radians), column j at azimuth0 + j * azimuth_inc;
 * p = r (cos e cos a, cos e sin a, sin e).  Ranges outside [range_min, range_max] or non-finite become NaN points,
 * which every entry point of this library ignores.  d_* are device pointers; asynchronous on `stream`
 * (NULL = default stream). */
int32_t ndt3d_range_image_to_points_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim, const double* elevations,
                                        double azimuth0, double azimuth_inc, double range_min, double range_max, float* d_x,
                                        float* d_y, float* d_z, void* stream);

/* ---- sensor motion within a sweep (docs/ALGORITHM.md section 2.23) ---------------------------- */
/* A spinning lidar takes its returns one after another while the platform moves: `delta` is the sensor's pose at the end
 * of the sweep in the sensor frame at its start ((dx, dy, dtheta) | (tx, ty, tz, roll, pitch, yaw), R = Rz Ry Rx), the
 * motion in between is one constant twist xi = Log(delta), and a point p measured at sweep fraction s (0 = start,
 * 1 = end) is expressed in the sensor frame at fraction ref_frac by p' = Exp((s - ref_frac) xi) p.  s and ref_frac
 * are not clamped.  Every point is worked in float64 and rounded to float32 once.  With delta all zero, and for a
 * point whose s equals ref_frac, the result is bit for bit what the entry point without the motion gives (the range
 * entries) or the input (the point entries).  2D: dtheta is wrapped to (-pi, pi].  3D: a delta that turns by 3.1 rad
 * or more is NDT_ERR_INVALID_ARG, as is a non-finite delta, ref_frac, frac0 or frac_inc.
 *
 * The four helpers need no device.  *_sweep_motion: delta = prev^-1 o cur of two poses in one frame - the motion
 * between the last two estimates is the constant-velocity guess of the motion within this sweep (pitch =
 * asin(clamp(-R20)); where |cos pitch| < 1e-12 roll and yaw share an axis and roll = 0 is returned; cur == prev gives
 * exact zeros).  *_motion_twist: xi = Log(delta), (vx, vy, omega) | (rho[3], phi[3]). */
int32_t ndt2d_sweep_motion(const double prev[3], const double cur[3], double delta[3]);
int32_t ndt3d_sweep_motion(const double prev[6], const double cur[6], double delta[6]);
int32_t ndt2d_motion_twist(const double delta[3], double xi[3]);
int32_t ndt3d_motion_twist(const double delta[6], double xi[6]);
/* ndt2d_polar_to_points_dev / ndt3d_range_image_to_points_dev with the motion undone: beam i / azimuth column j (every
 * ring of it) was fired at fraction frac0 + i * frac_inc.  The unrounded float64 products of the plain conversions go
 * through the motion; invalid returns become NaN points as there.  Asynchronous on `stream`. */
int32_t ndt2d_polar_to_points_deskew_dev(const float* d_ranges, size_t n, double angle_min, double angle_inc,
                                         double range_min, double range_max, const double delta[3], double frac0,
                                         double frac_inc, double ref_frac, float* d_x, float* d_y, void* stream);
int32_t ndt3d_range_image_to_points_deskew_dev(const float* d_ranges, int32_t n_elev, int32_t n_azim,
                                               const double* elevations, double azimuth0, double azimuth_inc,
                                               double range_min, double range_max, const double delta[6], double frac0,
                                               double frac_inc, double ref_frac, float* d_x, float* d_y, float* d_z,
                                               void* stream);
/* Cartesian device points with a fraction each (drivers that deliver x, y, z, t; non-repetitive scanners).  A point
 * whose fraction is not finite becomes a NaN point, whatever delta is.  The outputs may be the inputs.  Asynchronous
 * on `stream`. */
int32_t ndt2d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_frac, size_t n, const double delta[3],
                                double ref_frac, float* d_ox, float* d_oy, void* stream);
int32_t ndt3d_deskew_points_dev(const float* d_x, const float* d_y, const float* d_z, const float* d_frac, size_t n,
                                const double delta[6], double ref_frac, float* d_ox, float* d_oy, float* d_oz,
                                void* stream);

/* Empty voxel grid over a chosen extent (lo / hi = min / max corner, x y z), to be filled with
 * ndt3d_add_target_points(_dev): a submap that grows scan by scan, as ndt2d_reserve_target. */
int32_t ndt3d_reserve_target(ndt3d_handle* h, const double lo[3], const double hi[3]);
/* ndt3d_add_target_points with the points already on the device, optionally moved into the map frame first:
 * pose != NULL applies p' = R p + t in float32 (R = Rz(yaw) Ry(pitch) Rx(roll) formed in float64 and rounded to
 * float32; each row ((r0 x + r1 y) + r2 z) + t with every operation rounded separately) - the pose an alignment
 * of that scan returned - so a 3D scan goes align -> submap without leaving the GPU.  `stream` is the stream that
 * produced the arrays (NULL: already complete); the call returns when the grid is updated. */
int32_t ndt3d_add_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                    const double pose[6], size_t* n_outside, void* stream);
/* The exact inverse of ndt3d_add_target_points(_dev), as ndt2d_remove_target_points(_dev): the points leave the voxels'
 * exact sums, binned (and moved, with a pose) by the float32 operations of the add; removing points that were added
 * leaves bit for bit the grid without them; points that are not in the map (a voxel's count below zero, or zero with
 * a sum left) give NDT_ERR_INVALID_ARG and a handle without a target. */
int32_t ndt3d_remove_target_points(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n,
                                   size_t* n_outside);
int32_t ndt3d_remove_target_points_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                                       const double pose[6], size_t* n_outside, void* stream);
/* device arrays; `stream` = the stream that produced them (NULL: already complete) */
int32_t ndt3d_set_target_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n,
                             void* stream);
/* submap persistence, as ndt2d_save_map / ndt2d_load_map (dims = 3, 80-byte cell blocks) */
size_t ndt3d_map_size(const ndt3d_handle* h);
int32_t ndt3d_save_map(ndt3d_handle* h, void* buf, size_t capacity, size_t* written);
int32_t ndt3d_load_map(ndt3d_handle* h, const void* buf, size_t bytes);
/* ndt2d_coarsen_map for voxel grids: dst's voxels are unions of f x f x f voxels of src's, f = 2 or 4; lattice, sums,
 * roundings, finalisation with dst's parameters and return values as there (no overlap_grids in 3D).  A 3D grid has
 * no empty-ring contract - ndt3d_add_target_points* bins a point into a ring voxel of a reserved extent like into any
 * other - so sums found in src's ring are kept: they go to the coarse voxel their place on the lattice names. */
int32_t ndt3d_coarsen_map(ndt3d_handle* src, ndt3d_handle* dst);
/* ndt2d_merge_map / ndt2d_unmerge_map for voxel grids: pose = (x, y, z, roll, pitch, yaw), R = Rz Ry Rx as the nine
 * products of the alignment kernels in their order (float64, host), rows ((R0 x + R1 y) + R2 z) + t, Q a symmetric 3 x 3;
 * a block is inside where 0 <= f < extent on every axis (no ring in 3D).  Steps, roundings and return values as there. */
int32_t ndt3d_merge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside);
int32_t ndt3d_unmerge_map(ndt3d_handle* dst, ndt3d_handle* src, const double pose[6], size_t* n_outside);
int32_t ndt3d_get_grid_info(ndt3d_handle* h, ndt3d_grid_info* info);
/* count [cells], mean [cells][3], icov [cells][6] (xx xy xz yy yz zz); any pointer may be NULL */
int32_t ndt3d_get_grid(ndt3d_handle* h, int32_t* count, float* mean_xyz, float* icov6);
int32_t ndt3d_evaluate(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                       const double pose[6], ndt3d_eval* out);
int32_t ndt3d_evaluate_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                           const double pose[6], ndt3d_eval* out);
/* ndt2d_fit_points* / ndt2d_select_points_dev for voxel grids: the image is the nested fma of the 3D alignment under
 * R = Rz Ry Rx (angles wrapped, the nine products in float64, rounded to float32), a point is in the grid where
 * 0 <= f < extent on every axis (no ring in 3D), m_i is its three-by-three form.  Classes, outputs, stream behaviour and
 * return values as there. */
int32_t ndt3d_fit_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                             const double pose[6], float max_m, float* d_m, uint8_t* d_class, ndt_point_fit* fit);
int32_t ndt3d_fit_points(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                         const double pose[6], float max_m, float* m, uint8_t* cls, ndt_point_fit* fit);
int32_t ndt3d_select_points_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                const double pose[6], float max_m, uint32_t keep, float* d_ox, float* d_oy, float* d_oz,
                                uint32_t* d_index, ndt_point_fit* fit);
/* ndt2d_voxel_filter* for three coordinates: the same per-axis arithmetic, order (iz, iy, ix) with ix fastest. */
int32_t ndt3d_voxel_filter_dev(ndt3d_handle* h, const float* d_x, const float* d_y, const float* d_z, size_t n, double leaf,
                               uint32_t min_points, float* d_ox, float* d_oy, float* d_oz, uint32_t* d_count,
                               size_t capacity, ndt_voxel_filter_info* info);
int32_t ndt3d_voxel_filter(ndt3d_handle* h, const float* x, const float* y, const float* z, size_t n, double leaf,
                           uint32_t min_points, float* ox, float* oy, float* oz, uint32_t* count, size_t capacity,
                           ndt_voxel_filter_info* info);
int32_t ndt3d_align(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                    const double init_pose[6], ndt3d_result* out);
int32_t ndt3d_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                        const double init_pose[6], ndt3d_result* out);
/* Asynchronous form, as ndt2d_align_dev_async / ndt2d_align_finish: returns once the loop is under way
 * on the handle's stream (with fixed_iterations > 0 the whole chain and the fetch of its final state
 * are enqueued, so back-to-back calls keep the GPU busy without a host round trip per alignment);
 * the d_s* arrays must stay valid until ndt3d_align_finish returns.  Any other call on the handle
 * finishes an alignment in flight first. */
int32_t ndt3d_align_dev_async(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                              const double init_pose[6]);
int32_t ndt3d_align_finish(ndt3d_handle* h, ndt3d_result* out);
/* Many alignments against the cached voxel grid in ONE launch chain, as ndt2d_align_multi_scan_dev /
 * ndt2d_align_multi_start_dev: m (1..64) different scans, each from its own initial pose (d_sx / d_sy / d_sz / n:
 * host arrays of m device pointers / sizes; init_poses [m][6]) - or one scan from m initial poses.  Per
 * iteration the chain runs two kernels (one workgroup per start reduces and solves, then 256 x m workgroups
 * evaluate), so the launch boundary and the 6 x 6 solve are paid once per iteration for all starts.
 * results[k] is bit for bit what ndt3d_align_dev returns for scan k and init_poses[k]; a start that has
 * finished is frozen while the others go on.  Synchronous in the results (host memory). */
int32_t ndt3d_align_multi_scan_dev(ndt3d_handle* h, const float* const* d_sx, const float* const* d_sy, const float* const* d_sz,
                                   const size_t* n, const double* init_poses, int32_t m, ndt3d_result* results);
int32_t ndt3d_align_multi_start_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                    const double* init_poses, int32_t m, ndt3d_result* results);
/* The neighbourhood a source point is scored against (docs/ALGORITHM.md 2.25): n = 1 (a new handle) is the voxel its
 * image lies in; n = 7 adds that voxel's six face neighbours (the "DIRECT7" of PCL's ndt_omp and Autoware), which
 * makes the score continuous across a voxel face and widens the basin.  The own voxel is found as with 1 (an image
 * outside the grid or not finite contributes nothing, whatever lies next to it); candidates in the order own, -x, +x,
 * -y, +y, -z, +z, one that leaves the grid skipped by index; every candidate with a valid record adds one term to the
 * score, g, H (both Hessian modes) and one to n_hit, which min_hits is compared with.  A scoring option only: the
 * voxel grid and its records are the same, so the switch costs nothing and nothing is rebuilt; bit for bit
 * reproducible; with 1 every result is bit for bit what it was before the option existed.
 *   Honoured by ndt3d_evaluate*, ndt3d_align*, ndt3d_align_dev_async / ndt3d_align_finish, ndt3d_align_trace,
 *     ndt3d_align_multi_start_dev and ndt3d_align_multi_scan_dev (results[k] bit for bit the single call with 7).
 *   Refused with 7 set (NDT_ERR_INVALID_ARG, ndt_last_error names the option): ndt3d_search*, ndt3d_score_poses*,
 *     ndt3d_best_poses*, ndt3d_score_particles*, ndt3d_fit_points* and ndt3d_select_points_dev - their kernels keep the
 *     single-voxel score their contracts name.  To search with 1 and refine with 7, call the setter in between.
 *   Unaffected: builds and updates, save / load, coarsen, merge, every map-to-map entry point (components, not
 *     points), ndt3d_voxel_filter*, and the ndt3d_batch_* / ndt3d_multi_* contexts, which have no such option.
 * ndt3d_set_neighbourhood: n other than 1 or 7, or a null handle: NDT_ERR_INVALID_ARG (the setting stays).  An
 * alignment in flight on the handle is finished first; no target is needed and no other device work is done.
 * ndt3d_neighbourhood returns 1 or 7 (a null handle: NDT_ERR_INVALID_ARG). */
int32_t ndt3d_set_neighbourhood(ndt3d_handle* h, int32_t n);
int32_t ndt3d_neighbourhood(const ndt3d_handle* h);
/* The map neighbourhood: the target voxels a source COMPONENT is scored against in 3D map-to-map alignment
 * (docs/ALGORITHM.md 2.26; Stoyanov et al. 2012 pair a source Gaussian with neighbouring target Gaussians).  n = 1 (a
 * new handle) is the voxel the image of the component's mean falls into, the objective of 2.14; n = 7 adds that voxel's
 * six face neighbours, which takes the jumps at the voxel faces out of the score and with them the pull towards the
 * identity that two maps on one lattice show.  A setting of its own, not ndt3d_set_neighbourhood (points), and the
 * TARGET handle's, like d1, d2 and the Hessian mode: a source handle's value is ignored.
 *   The own voxel is found as with 1 (the float32 image of the mean; outside the grid or not finite: the component
 *   contributes nothing, whatever lies next to it).  Candidates in the order own, -x, +x, -y, +y, -z, +z; one that
 *   leaves [0, W) x [0, H) x [0, D) is skipped by index (key - 1 from ix = 0 is a voxel of the grid and not a
 *   neighbour).  Every candidate with a valid covariance record adds one full term of 2.14 with that voxel's mean and
 *   covariance to the score, g and H (both Hessian modes), in candidate order, and one to n_hit: n_hit counts
 *   component-voxel pairs, and min_hits is compared with that count.  With target == source and 7 the identity is a
 *   stationary point up to float32 rounding only (the pairs i->j and j->i cancel in exact arithmetic).
 *   Honoured by ndt3d_evaluate_map, ndt3d_align_map and ndt3d_align_map_multi (on both sides of
 *     NDT_TUNE_MAP_MULTI_FROM; results[k] stays bit for bit the single call's).
 *   Refused while the target's setting is 7 (NDT_ERR_INVALID_ARG, ndt_last_error names ndt3d_set_map_neighbourhood):
 *     ndt3d_search_map, ndt3d_search_map_scores, ndt3d_search_align_map, ndt3d_score_map_poses*, ndt3d_best_map_poses* -
 *     their kernels keep the single-voxel score their contracts name.  Search with 1, refine with 7.
 *   Unaffected: everything that scores points, builds, updates, save / load, coarsen, merge, ndt3d_get_components.
 * Bit for bit reproducible; with 1 every result is bit for bit what it was before the option existed.
 * ndt3d_set_map_neighbourhood: n other than 1 or 7, or a null handle: NDT_ERR_INVALID_ARG, ndt_last_error names the
 * function (the setting stays).  An alignment in flight on the handle is finished first; nothing is rebuilt (grid, sums,
 * covariance records and component list do not depend on the setting) and no target is needed.
 * ndt3d_map_neighbourhood returns 1 or 7 (a null handle: NDT_ERR_INVALID_ARG). */
int32_t ndt3d_set_map_neighbourhood(ndt3d_handle* h, int32_t n);
int32_t ndt3d_map_neighbourhood(const ndt3d_handle* h);
/* Exhaustive 3D pose search (docs/ALGORITHM.md "Exhaustive 3D pose search"), the twin of ndt2d_search*: the NDT score of
 * the scan at every pose of an (x, y, yaw) lattice against the cached voxel grid, then the best well-separated peaks - a
 * ground vehicle's relocalisation or loop closure whose guess is metres and tens of degrees off.  z, roll and pitch are
 * pinned to center[2], center[3], center[4] at every lattice pose (the refinement that follows frees all six).
 * The window's axes are (x, y, yaw): half_extent[a] and step[a] go with center[0], center[1], center[5].  Validation,
 * axis lengths, the cyclic yaw axis for half_extent[2] >= pi, wrapping to (-pi, pi], the flat index
 * ((j n_y) + iy) n_x + ix, the 2^25-pose cap, peaks, the 4096-peak shortlist, the separation walk (dx, dy and wrapped
 * yaw), k in 1..64 and bitwise determinism are those of ndt2d_search_window above; non-finite center[2..4] is
 * NDT_ERR_INVALID_ARG too.  The score at a lattice pose is the score ndt3d_evaluate_dev reports at
 * (x, y, center[2], center[3], center[4], yaw): the same float32 terms per point, summed in another order.  A window
 * that misses the map returns NDT_OK with *n_hits = 0.  Any alignment in flight on the handle is finished first. */
typedef struct ndt3d_search_window {
  double center[6];       /* tx ty tz roll pitch yaw of the lattice's middle pose; tz, roll and pitch are pinned */
  double half_extent[3];  /* x, y (metres), yaw (radians); >= 0, 0 pins the axis; yaw >= pi: a full turn */
  double step[3];         /* lattice step per axis (x, y, yaw), > 0 */
  double min_sep_trans;   /* hits closer than this in (x, y) ... */
  double min_sep_rot;     /* ... AND in wrapped yaw than an accepted hit are dropped (both >= 0) */
} ndt3d_search_window;

typedef struct ndt3d_search_hit {
  double pose[6];         /* lattice pose: x, y, center[2..4], yaw wrapped to (-pi, pi] */
  float score;            /* the lattice score (float32, as in the volume) */
  int32_t index;          /* flat lattice index */
} ndt3d_search_hit;

/* dims = n_yaw, n_y, n_x of the window's lattice (CPU only; the same validation as the searches) */
int32_t ndt3d_search_lattice_size(const ndt3d_search_window* w, int32_t dims[3]);
/* hits[0 .. *n_hits) (hits has room for k), best first.  Synchronous in the hits (host memory). */
int32_t ndt3d_search_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                         const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits);
/* the same with a host scan */
int32_t ndt3d_search(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                     const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits, int32_t* n_hits);
/* the score volume itself into d_scores (device memory, n_yaw x n_y x n_x floats, flat index order); returns once it
 * is written */
int32_t ndt3d_search_scores_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                const ndt3d_search_window* w, float* d_scores);
/* ndt3d_search_dev, then ndt3d_align_multi_start_dev from the hits' poses: results[i] is bit for bit what
 * ndt3d_align_multi_start_dev returns for those poses (results has room for k) */
int32_t ndt3d_search_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                               const ndt3d_search_window* w, int32_t k, ndt3d_search_hit* hits,
                               ndt3d_result* results, int32_t* n_hits);
/* Scoring a list of 3D poses (docs/ALGORITHM.md "Scoring a list of poses"), the twin of ndt2d_score_poses*: poses is
 * [m][6] = (tx, ty, tz, roll, pitch, yaw) in double, so the list also covers what the lattice pins - a search over z,
 * roll or pitch is a list.  scores[i] is the score ndt3d_evaluate_dev reports at poses[6i .. 6i+5]: the three angles
 * wrapped, the nine products of the rotation in double and rounded to float32, the nested-fma image, the inside test
 * 0 <= f < extent and the score term of the single-pose path, summed in another order.  NaN points add nothing; a
 * non-finite pose scores exactly +0.0f and never becomes a hit.  The bitwise properties are those of the 2D calls; the
 * lattice of an ndt3d_search_window is the list (x, y, center[2], center[3], center[4], yaw) in flat index order, and
 * then the scores are the volume of ndt3d_search_scores_dev bit for bit.  Best poses: as in 2D, with the translation
 * distance Euclidean over (x, y, z) and the rotation distance the largest of the wrapped |droll|, |dpitch|, |dyaw|.
 * ndt3d_best_poses_align_dev refines the hits in one ndt3d_align_multi_start_dev call.  Streams, state and errors are
 * those of the 2D calls (ndt3d_wait_stream orders the producers). */
int32_t ndt3d_score_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                              const double* d_poses /* device, [m][6] */, size_t m, float* d_scores /* device, [m] */);
int32_t ndt3d_score_poses(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                          const double* poses, size_t m, float* scores);
int32_t ndt3d_best_poses_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                             const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                             ndt3d_search_hit* hits, int32_t* n_hits);
int32_t ndt3d_best_poses_align_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                   const double* d_poses, size_t m, double min_sep_trans, double min_sep_rot, int32_t k,
                                   ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits);
/* Scoring 3D particles (docs/ALGORITHM.md "Scoring particles: a team of lanes per pose"), the twin of
 * ndt2d_score_particles*: a team of 64 or 256 lanes per pose of a short list, the hit count beside the score, an
 * asynchronous form.  poses is [m][6] = (tx, ty, tz, roll, pitch, yaw) in double.  The pose and every point's term are
 * ndt3d_score_poses_dev's bit for bit; the score differs from that call's only by the summation order, which is the one
 * ALGORITHM states over 256 virtual lanes; n_hit[i] is what ndt3d_evaluate_dev reports as n_hit at that pose.  A score and
 * a count depend on nothing but the grid, the scan and the pose - not on the position in the list, the list's length or
 * the team width - and two calls give the same bits.  They are the faster calls at every list size measured (DESIGN
 * 5.19); ndt3d_score_poses_dev remains for the search volume's bits and for ndt3d_best_poses*.  Streams, the asynchronous form's contract and the errors are those of the 2D calls
 * (ndt3d_stream, ndt3d_wait_stream). */
int32_t ndt3d_score_particles_dev(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                  const double* d_poses /* device, [m][6] */, size_t m, float* d_scores /* device, [m] */,
                                  uint32_t* d_n_hit /* device, [m], may be NULL */);
int32_t ndt3d_score_particles_async(ndt3d_handle* h, const float* d_sx, const float* d_sy, const float* d_sz, size_t n,
                                    const double* d_poses, size_t m, float* d_scores, uint32_t* d_n_hit);
int32_t ndt3d_score_particles(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                              const double* poses, size_t m, float* scores, uint32_t* n_hit /* may be NULL */);
/* Per-iteration trace, as ndt2d_align_trace (debugging and stage-by-stage parity checks; never on a timed path):
 * rows[j], j < *n_rows <= capacity, is the state after j + 1 updates - the pose after them, H / g / score / n_hit
 * of the evaluation that produced the (j+1)-th update.  out (may be NULL): the final result.  Host arrays. */
int32_t ndt3d_align_trace(ndt3d_handle* h, const float* sx, const float* sy, const float* sz, size_t n,
                          const double init_pose[6], ndt3d_result* rows, int32_t capacity, int32_t* n_rows, ndt3d_result* out);
/* ---- 3D map-to-map alignment (distribution-to-distribution NDT; docs/ALGORITHM.md section 2.14) ---------------
 * The SE(3) twin of ndt2d_align_map: aligns the cached voxel grid of `source` to the cached voxel grid of `target` from the
 * per-voxel sums alone - what a handle keeps after ndt3d_add_target_points_dev, and all that ndt3d_save_map /
 * ndt3d_load_map persist, is enough; no point of either map is needed.  The source is the list of its valid voxels'
 * Gaussians (mean, regularised covariance: its *components*, in voxel-key order), each scored against the target Gaussian
 * of the one voxel its transformed mean falls in, with the combined covariance R S_i R^T + S_j; every hit weighs the same.
 * pose = (tx, ty, tz, roll, pitch, yaw) maps the source map's frame into the target map's frame.
 *   - The TARGET handle's parameters drive the solve (d1, d2, hessian_mode, the limits and stops, step_scale,
 *     line_search, its stream); the source handle's min_points / eig_ratio decide only its components.  The cell sizes
 *     may differ.  step_scale much above 1 over-relaxes this objective, as in 2D.
 *   - target == source is legal (a map against itself: the identity is a fixed point).
 *   - Both handles must live on the same device: NDT_ERR_INVALID_ARG.  No grid on either handle: NDT_ERR_NO_TARGET.
 *     A non-finite pose: NDT_ERR_INVALID_ARG.  A source without a component or a target without a valid voxel: NDT_OK
 *     with status NDT_TOO_FEW_CELLS and the initial pose (ndt3d_evaluate_map: all zeros).
 *   - Both calls are synchronous and finish an alignment in flight on either handle first; the target's stream is ordered
 *     behind the source's by the library.  The derived per-handle data (covariance records, component list) is built on
 *     a handle's first such call and again after anything that changes its grid.  Results are bit for bit reproducible.
 *   - Two maps of one scene on the same voxel lattice pull towards the identity (measured at 1 m voxels: an
 *     offset of 0.10 m / 10 mrad is recovered from the zero guess, 0.30 m / 30 mrad ends in a local optimum): from a guess
 *     more than about a tenth of a voxel off, align a coarse pair of handles first and the fine pair from its result
 *     (DESIGN.md section 5.9).
 *   - ndt3d_result / ndt3d_eval are those of ndt3d_align / ndt3d_evaluate (n_hit counts components that hit a valid
 *     target voxel).  No covariance calibration exists for this objective.  Not offered: pairing with neighbouring
 *     voxels.  Several alignments against one target: ndt3d_align_map_multi below. */
int32_t ndt3d_evaluate_map(ndt3d_handle* target, ndt3d_handle* source, const double pose[6], ndt3d_eval* out);
int32_t ndt3d_align_map(ndt3d_handle* target, ndt3d_handle* source, const double init_pose[6], ndt3d_result* out);
/* m (1..64) 3D map-to-map alignments against ONE target in one launch chain (the twin of ndt2d_align_map_multi): start
 * k aligns sources[k] from init_poses[6k .. 6k+5].  The same handle m times is a multi-start (the peaks of
 * ndt3d_search_map); different handles are several submaps relocalised against one older submap; sources[k] may be
 * `target`.
 *   - results[k] is bit for bit what ndt3d_align_map(target, sources[k], &init_poses[6k], ...) returns, whatever
 *     hessian_mode, fixed or converged mode, max_iterations, step_scale, line_search and NDT_TUNE_MAP_MULTI_FROM are; a
 *     start that has finished is frozen while the others go on.
 *   - The target handle's parameters, stream and graph cache drive the call, as for ndt3d_align_map.  Synchronous: it
 *     returns once nothing reads any source's component list any more.
 *   - Errors of the whole call, found before anything is enqueued (the handles stay usable): a null pointer, a null
 *     entry of sources, m outside 1..64 (these three before any device call), a non-finite pose, handles on different
 *     devices: NDT_ERR_INVALID_ARG; a handle without a grid: NDT_ERR_NO_TARGET.
 *   - Inside an NDT_OK call: a source without a component gives ITS start status NDT_TOO_FEW_CELLS and its initial
 *     pose while the others run; a target without a valid voxel gives that to every start; nothing is launched if no
 *     start is live.
 * Pairs with different targets are not covered (one call per target). */
int32_t ndt3d_align_map_multi(ndt3d_handle* target, ndt3d_handle* const* sources, const double* init_poses /* [m][6] */,
                              int32_t m, ndt3d_result* results /* [m] */);
/* Exhaustive pose search for 3D map-to-map alignment (docs/ALGORITHM.md section 2.16): the score ndt3d_evaluate_map
 * reports (the same float32 terms per component, summed in another order) at every pose of the window's (x, y, yaw)
 * lattice, z, roll and pitch pinned to center[2..4], then the best well-separated peaks - a loop closure between two
 * 3D submaps whose relative pose is known to metres and not at all in heading.  Window, lattice, hits (6-vector
 * poses), k in 1..64, the window errors and bitwise determinism are those of ndt3d_search above; handles, devices and
 * target == source are as for ndt3d_align_map (d1, d2: the target handle's).  A source without a component or a target
 * without a valid voxel gives an all-zero volume and no hit.  All three are synchronous: they return once nothing reads
 * the source's component list any more.  ndt3d_search_map_scores writes the volume [n_yaw][n_y][n_x] into device
 * memory.  ndt3d_search_align_map refines all hits in one ndt3d_align_map_multi call (nothing is launched for zero
 * hits): results[q] is bit for bit what ndt3d_align_map(target, source, hits[q].pose) returns (hits and results have
 * room for k). */
int32_t ndt3d_search_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w,
                         int32_t k, ndt3d_search_hit* hits, int32_t* n_hits);
int32_t ndt3d_search_map_scores(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w,
                                float* d_scores);
int32_t ndt3d_search_align_map(ndt3d_handle* target, ndt3d_handle* source, const ndt3d_search_window* w,
                               int32_t k, ndt3d_search_hit* hits, ndt3d_result* results, int32_t* n_hits);
/* Scoring a 3D map at a list of poses (docs/ALGORITHM.md section 2.21), the twin of ndt2d_score_map_poses*: poses is
 * [m][6] = (tx, ty, tz, roll, pitch, yaw) in double, angles not necessarily wrapped - z, roll and pitch are free here,
 * where ndt3d_search_map pins them: the loop closure between two submaps of unknown relative height and tilt.
 * scores[i] is the score and n_hit[i] the n_hit ndt3d_evaluate_map reports at poses[6i .. 6i+5]; a non-finite pose, a
 * translation beyond float32 or a non-finite entry of R scores exactly +0.0f with n_hit 0.  A list that holds the lattice
 * of an ndt3d_search_map window in flat index order, rows (x, y, center[2], center[3], center[4], yaw) with the axes'
 * doubles, gives the volume of ndt3d_search_map_scores bit for bit.  The separation of the best poses is Euclidean over
 * x, y, z and the largest wrapped difference of the three angles, as for ndt3d_best_poses_dev.
 * ndt3d_best_map_poses_align_dev refines the hits in one ndt3d_align_map_multi call.  Handles, streams, state and errors:
 * as ndt2d_score_map_poses*. */
int32_t ndt3d_score_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses /* device, [m][6] */,
                                  size_t m, float* d_scores /* device, [m] */, uint32_t* d_n_hit /* device, [m]; may be NULL */);
int32_t ndt3d_score_map_poses(ndt3d_handle* target, ndt3d_handle* source, const double* poses, size_t m,
                              float* scores, uint32_t* n_hit /* may be NULL */);
int32_t ndt3d_best_map_poses_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m,
                                 double min_sep_trans, double min_sep_rot, int32_t k, ndt3d_search_hit* hits,
                                 int32_t* n_hits);
int32_t ndt3d_best_map_poses_align_dev(ndt3d_handle* target, ndt3d_handle* source, const double* d_poses, size_t m,
                                       double min_sep_trans, double min_sep_rot, int32_t k, ndt3d_search_hit* hits,
                                       ndt3d_result* results, int32_t* n_hits);
/* The components of a handle's cached voxel grid, as host copies: mean_xyz [3n], cov6 [6n] = (xx xy xz yy yz zz) of the
 * regularised covariance, key [n] = (iz * height + iy) * width + ix, ascending.  Any pointer may be NULL; *n (if given) is
 * the count, also when capacity is too small for the arrays asked for (NDT_ERR_CAPACITY). */
int32_t ndt3d_get_components(ndt3d_handle* h, float* mean_xyz, float* cov6, int32_t* key, int32_t capacity, int32_t* n);
void* ndt3d_stream(ndt3d_handle* h);
/* as ndt2d_wait_stream: order the handle's stream behind the producer of the device arrays */
int32_t ndt3d_wait_stream(ndt3d_handle* h, void* producer_stream);
/* Execution-strategy knobs of a 3D handle (as ndt2d_set_tuning: they choose between code paths that build the same grid).
 *   NDT_TUNE_SINGLE_SYNC_BUILD  1 (default): ndt3d_set_target on a handle that already holds a grid decides the new grid's
 *                               geometry on the device and pays one host round trip; 0: the bounding box comes to the host
 *                               first (two round trips)
 *   NDT_TUNE_MAP_MULTI_FROM     ndt3d_align_map_multi calls of at least this many starts run one launch chain for all
 *                               starts; smaller calls run one ndt3d_align_map chain per start (default 2; 1..65, 65:
 *                               never the shared chain; other values NDT_ERR_INVALID_ARG).  Results are bit-identical
 *                               either way.
 *   NDT_TUNE_FUSED_BEGIN        as on ndt2d_set_tuning, for ndt3d_align* (k_iterate3_first against k_begin3; default 1)
 *   NDT_TUNE_PARTICLE_TEAM      as on ndt2d_set_tuning, for ndt3d_score_particles* (0, 64 or 256; default 0)
 * Other knobs: NDT_ERR_INVALID_ARG. */
int32_t ndt3d_set_tuning(ndt3d_handle* h, int32_t knob, int64_t value);

/* ---- 3D loop-closure candidate batch ------------------------------------------------------------ */
/* The 3D twin of ndt2d_batch: independent 3D scan pairs aligned concurrently, one persistent
 * 1024-thread workgroup per CU, the pair's voxel grid (u16 voxel -> slot table + 36-byte records) in
 * LDS for the whole Gauss-Newton / Newton loop.  Clouds are concatenated SoA arrays; pair k owns
 * target points [toff[k], toff[k+1]) and source points [soff[k], soff[k+1]); init is [n_pairs][6];
 * results is [n_pairs].  Every pair's result equals the single-pair path's (ndt3d_set_target +
 * ndt3d_align) up to float32 summation order: same records bit for bit, same per-point arithmetic.
 * On-chip capacity per pair: 2 B per voxel + 36 B per occupied voxel <= 157 KB and 6 B per voxel
 * <= 157 KB during the build (BASELINE config 5: 17 424 voxels, 2 706 occupied = 132 KB; that grid holds up to
 * 3 494 occupied voxels).  A pair
 * beyond it is handed, on the device and within the same call, to a second variant of the kernel that
 * keeps the pair's voxel table in global memory and its first 4 461 records on chip (up to 2^20 voxels - e.g.
 * 256 x 256 x 16 - and 32 767 occupied; a pair that only has a few more occupied voxels than fit stays on the first
 * variant with its last records in global memory).
 * Beyond that a pair gets status NDT_ERR_CAPACITY from the _dev entry point, and the host-pointer entry
 * point re-runs it through the single-pair path transparently.  Stream semantics as ndt2d_batch_align_dev.
 * A context holds about 0.2 GB of device memory (per-workgroup slabs of the build, 8 slabs of the global-memory variant)
 * and 2.1 GB once a call has needed the global-memory variant (NDT_TUNE_BATCH_GLOBAL_WORKGROUPS).
 * Results do not depend on the order of a cloud's points beyond float32 summation order (the grid not at all);
 * the grid build is fastest on scans left in the order a 64-beam driver delivers them (all beams of one bearing, then
 * the next bearing): it walks a cloud in rows of 64 points and combines a lane's consecutive rows in registers. */
typedef struct ndt3d_batch ndt3d_batch;
int32_t ndt3d_batch_create(const ndt3d_params* p, int32_t device_id, ndt3d_batch** out);
/* coarse-to-fine over the batch, as ndt2d_batch_create_pyramid (levels coarse to fine, at most 8) */
int32_t ndt3d_batch_create_pyramid(const ndt3d_params* levels, int32_t n_levels, int32_t device_id, ndt3d_batch** out);
int32_t ndt3d_batch_destroy(ndt3d_batch* b);
int32_t ndt3d_batch_align(ndt3d_batch* b, const float* tx, const float* ty, const float* tz, const uint64_t* toff,
                          const float* sx, const float* sy, const float* sz, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt3d_result* results);
int32_t ndt3d_batch_align_dev(ndt3d_batch* b, const float* d_tx, const float* d_ty, const float* d_tz, const uint64_t* d_toff,
                              const float* d_sx, const float* d_sy, const float* d_sz, const uint64_t* d_soff,
                              const double* d_init, size_t n_pairs, ndt3d_result* d_results, void* stream);
void* ndt3d_batch_stream(ndt3d_batch* b);
int32_t ndt3d_batch_wait_stream(ndt3d_batch* b, void* producer_stream);
int32_t ndt3d_batch_set_tuning(ndt3d_batch* b, int32_t knob, int64_t value);   /* NDT_TUNE_BATCH_GLOBAL_WORKGROUPS */

/* The 3D batch over several devices from ONE host process: ndt2d_multi_* for ndt3d_batch contexts (one context and one
 * host thread per device, contiguous work-balanced shards by ndt2d_multi_plan's rule).  ndt3d_multi_align takes host
 * pointers laid out as ndt3d_batch_align; ndt3d_multi_align_dev takes per-device device pointers (arrays of n_devices
 * pointers, shard d on device d, n_pairs[d] pairs, 0 allowed), aligns every shard on its context's stream and
 * exchanges the 408-byte result rows with ONE grouped ncclAllGather - layout, ownership and error codes as
 * ndt2d_multi_align_dev. */
typedef struct ndt3d_multi ndt3d_multi;
int32_t ndt3d_multi_create(const ndt3d_params* p, const int32_t* device_ids, int32_t n_devices, ndt3d_multi** out);
int32_t ndt3d_multi_create_pyramid(const ndt3d_params* levels, int32_t n_levels, const int32_t* device_ids,
                                   int32_t n_devices, ndt3d_multi** out);
int32_t ndt3d_multi_destroy(ndt3d_multi* m);
int32_t ndt3d_multi_device_count(const ndt3d_multi* m);
int32_t ndt3d_multi_align(ndt3d_multi* m, const float* tx, const float* ty, const float* tz, const uint64_t* toff,
                          const float* sx, const float* sy, const float* sz, const uint64_t* soff, const double* init,
                          size_t n_pairs, ndt3d_result* results);
int32_t ndt3d_multi_align_dev(ndt3d_multi* m, const float* const* d_tx, const float* const* d_ty, const float* const* d_tz,
                              const uint64_t* const* d_toff, const float* const* d_sx, const float* const* d_sy,
                              const float* const* d_sz, const uint64_t* const* d_soff, const double* const* d_init,
                              const size_t* n_pairs, ndt3d_result** d_results_all, size_t* shard_stride,
                              ndt3d_result* results);

#ifdef __cplusplus
}
#endif
#endif /* NDT_HIP_H_ */

// CLEAR MOD matching on the GPU for gfx950: the per-frame loop of the reference's
// evaluation/pyeval/CLEAR_MOD_HUN.py:58-91 (cost matrix, scipy's linear_sum_assignment, the
// d < td count) as one launch over F frames, one workgroup per frame.
//
// The assignment is scipy's algorithm (rectangular_lsap: shortest augmenting paths after
// Jonker-Volgenant, fp64 duals), rows = the smaller side, columns = the larger.  Nothing of size
// n x m exists: a cost is evaluated where it is read, d = sqrt(dx^2 + dy^2) in fp64 with each
// product and the sum rounded on its own (no fma) and a correctly rounded sqrt, priced 1e6 unless
// d <= td.  The state is O(n + m): row duals and the rows' columns in LDS (n <= 1024), the column
// state (dual, tentative distance, predecessor, owner row) in LDS up to kEvLdsCols columns and in
// the caller's workspace beyond.  The parallel part is the column scan of one Dijkstra step: lanes
// stride over the columns, relax them against the current row and min-reduce (value, column) with
// ties to the lowest column, so a result never depends on timing.
//
// Loop bounds (all known at kernel entry): rows cur < n; Dijkstra steps per row <= cur + 1 (each
// step closes one column, and only the <= cur assigned columns are not sinks); the augmentation
// walks <= cur + 1 predecessors; every scan is a strided loop over m.  !(d <= td) prices NaN / inf
// distances as 1e6, so every reduced cost is finite and the min-reduction always finds a column;
// should it not, the frame is given up (matched = -1) rather than retried.
#include "common.h"

#include <limits.h>

namespace mvbev {

constexpr int kEvThreads = 256;
constexpr int kEvWaves = kEvThreads / kWave;
constexpr int kEvMaxRows = MVBEV_CLEAR_MOD_MAX_SMALL;
constexpr int kEvLdsCols = 2048;
constexpr int64_t kEvMaxCols = MVBEV_CLEAR_MOD_MAX_LARGE;
constexpr double kEvBeyond = 1e6;  // CLEAR_MOD_HUN.py:70

struct EvPoints {
  const void* p;
  int f64;
  int64_t base;  // the frame's first point
};

__device__ __forceinline__ void ev_load(const EvPoints& s, int i, double& x, double& y) {
  const int64_t k = 2 * (s.base + i);
  if (s.f64) {
    x = static_cast<const double*>(s.p)[k];
    y = static_cast<const double*>(s.p)[k + 1];
  } else {
    x = (double)static_cast<const float*>(s.p)[k];
    y = (double)static_cast<const float*>(s.p)[k + 1];
  }
}

// getDistance (CLEAR_MOD_HUN.py:6-7): the products and the sum are separate roundings
__device__ __forceinline__ double ev_dist(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
  const double dx = ax - bx, dy = ay - by;
  const double xx = dx * dx, yy = dy * dy;
  return __dsqrt_rn(xx + yy);
}

__device__ __forceinline__ double ev_price(double d, double td) { return !(d <= td) ? kEvBeyond : d; }

struct EvCols {
  double* v;    // column dual
  double* sp;   // shortest tentative path cost to the column in this row's search
  int* path;    // predecessor row; ~row once the column is closed (in the tree)
  int* r4c;     // the row assigned to the column, or -1
};

// (value, column) minimum over the workgroup, ties to the lowest column; red_* hold kEvWaves entries
__device__ __forceinline__ void ev_min(double& bv, int& bi, double* red_v, int* red_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (ov < bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    red_v[threadIdx.x >> 6] = bv;
    red_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = red_v[0];
  bi = red_i[0];
#pragma unroll
  for (int w = 1; w < kEvWaves; ++w) {
    const double ov = red_v[w];
    const int oi = red_i[w];
    if (ov < bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
}

// scipy's rectangular_lsap over n rows and m >= n columns; c4r[i] = the column of row i.
// Returns false if a search found no column (cannot happen with finite prices).
__device__ __forceinline__ bool ev_assign(const EvCols c, double* u, int* c4r, int n, int m, const EvPoints rows,
                                          const EvPoints cols, double td, double (*red_v)[kEvWaves],
                                          int (*red_i)[kEvWaves]) {
  const int tid = threadIdx.x;
  for (int j = tid; j < m; j += kEvThreads) {
    c.v[j] = 0.0;
    c.r4c[j] = -1;
  }
  for (int i = tid; i < n; i += kEvThreads) {
    u[i] = 0.0;
    c4r[i] = -1;
  }
  __syncthreads();
  int par = 0;
  for (int cur = 0; cur < n; ++cur) {
    for (int j = tid; j < m; j += kEvThreads) {  // sp / path are touched by a column's own thread until the duals
      c.sp[j] = INFINITY;
      c.path[j] = 0;
    }
    double min_val = 0.0;
    int i = cur, sink = -1;
    for (int step = 0; step <= cur && sink < 0; ++step) {
      double rx, ry;
      ev_load(rows, i, rx, ry);
      const double ui = u[i];
      double bv = INFINITY;
      int bi = INT_MAX;
      for (int j = tid; j < m; j += kEvThreads) {
        if (c.path[j] < 0) continue;  // closed
        double cx, cy;
        ev_load(cols, j, cx, cy);
        const double r = min_val + ev_price(ev_dist(rx, ry, cx, cy), td) - ui - c.v[j];
        double s = c.sp[j];
        if (r < s) {
          s = r;
          c.sp[j] = r;
          c.path[j] = i;
        }
        if (s < bv) {  // j ascends per thread: the lowest column of equal values stays
          bv = s;
          bi = j;
        }
      }
      ev_min(bv, bi, red_v[par], red_i[par]);  // the two buffers alternate: one barrier per step
      par ^= 1;
      if (bi == INT_MAX) return false;
      min_val = bv;
      if (bi % kEvThreads == tid) c.path[bi] = ~c.path[bi];  // its owner closes it
      const int r = c.r4c[bi];
      if (r < 0) sink = bi;
      else i = r;
    }
    if (sink < 0) return false;
    // the duals: every closed column j, and the row that owns it (the search tree's rows but cur)
    if (tid == 0) u[cur] += min_val;
    for (int j = tid; j < m; j += kEvThreads) {
      if (c.path[j] >= 0) continue;
      const double delta = min_val - c.sp[j];
      c.v[j] -= delta;
      const int r = c.r4c[j];
      if (r >= 0) u[r] += delta;
    }
    __syncthreads();
    if (tid == 0) {  // augment along the predecessors, sink back to cur
      int j = sink;
      for (int k = 0; k <= cur; ++k) {
        const int r = ~c.path[j];
        c.r4c[j] = r;
        const int t = c4r[r];
        c4r[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();  // the next row's reset must not overtake the walk
  }
  return true;
}

struct EvArgs {
  const void *gt, *det;
  int gt_f64, det_f64;
  const int32_t *gt_off, *det_off;
  int64_t Ng, Nd;
  double td;
  int32_t *n_gt, *n_det, *matched;
  double *modp_sum, *cost;
  int32_t* match;
  EvCols ws;           // SoA over ws_entries entries; frame f owns [gt_off[f] + det_off[f], + m)
  int64_t ws_entries;
};

__global__ __launch_bounds__(kEvThreads) void clear_mod_kernel(EvArgs a) {
  __shared__ double s_u[kEvMaxRows];
  __shared__ int s_c4r[kEvMaxRows];
  __shared__ double s_v[kEvLdsCols];
  __shared__ double s_sp[kEvLdsCols];
  __shared__ int s_path[kEvLdsCols];
  __shared__ int s_r4c[kEvLdsCols];
  __shared__ double red_v[2][kEvWaves];
  __shared__ int red_i[2][kEvWaves];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int64_t g0 = a.gt_off[f], g1 = a.gt_off[f + 1], d0 = a.det_off[f], d1 = a.det_off[f + 1];
  const bool in_range = g0 >= 0 && g0 <= g1 && g1 <= a.Ng && d0 >= 0 && d0 <= d1 && d1 <= a.Nd;
  const int64_t ng64 = g1 - g0, nd64 = d1 - d0;
  const int64_t n64 = ng64 < nd64 ? ng64 : nd64, m64 = ng64 < nd64 ? nd64 : ng64;
  const bool in_ws = m64 > kEvLdsCols;
  // a frame the call cannot hold (sizes past the limits, a workspace that does not cover it) is
  // reported, never run: nothing below indexes past what was checked here
  const bool ok = in_range && n64 <= kEvMaxRows && m64 <= kEvMaxCols && (!in_ws || g0 + d0 + m64 <= a.ws_entries);
  if (!ok) {
    if (tid == 0) {
      a.n_gt[f] = in_range ? (int32_t)ng64 : -1;
      a.n_det[f] = in_range ? (int32_t)nd64 : -1;
      a.matched[f] = -1;
      a.modp_sum[f] = 0.0;
      a.cost[f] = 0.0;
    }
    if (a.match && in_range)
      for (int64_t i = tid; i < ng64; i += kEvThreads) a.match[g0 + i] = -1;
    return;
  }
  const int ng = (int)ng64, nd = (int)nd64, n = (int)n64, m = (int)m64;
  const bool gt_rows = ng <= nd;  // scipy transposes when there are more rows than columns
  const EvPoints gtp{a.gt, a.gt_f64, g0}, detp{a.det, a.det_f64, d0};
  const EvPoints rows = gt_rows ? gtp : detp, cols = gt_rows ? detp : gtp;
  bool solved;
  if (in_ws) {
    const int64_t e0 = g0 + d0;
    solved = ev_assign(EvCols{a.ws.v + e0, a.ws.sp + e0, a.ws.path + e0, a.ws.r4c + e0}, s_u, s_c4r, n, m, rows,
                       cols, a.td, red_v, red_i);
  } else {
    solved = ev_assign(EvCols{s_v, s_sp, s_path, s_r4c}, s_u, s_c4r, n, m, rows, cols, a.td, red_v, red_i);
  }
  // the matching is done: the LDS column arrays are free.  Per row: its MODP term (0 unless counted),
  // its price, and the GT index it counts for (-1: d >= td, CLEAR_MOD_HUN.py:73).
  __syncthreads();
  double* term = s_v;                 // [kEvMaxRows]
  double* price = s_v + kEvMaxRows;   // [kEvMaxRows]  (kEvLdsCols == 2 kEvMaxRows)
  double* ordered = s_sp;             // the counted terms in GT index order
  int* key = s_path;
  static_assert(kEvLdsCols >= 2 * kEvMaxRows, "the epilogue's arrays live in the column arrays");
  if (a.match)
    for (int i = tid; i < ng; i += kEvThreads) a.match[g0 + i] = -1;
  for (int i = tid; i < n; i += kEvThreads) {
    const int j = solved ? s_c4r[i] : -1;
    double d = INFINITY;
    if (j >= 0 && j < m) {
      double rx, ry, cx, cy;
      ev_load(rows, i, rx, ry);
      ev_load(cols, j, cx, cy);
      d = ev_dist(rx, ry, cx, cy);
    }
    const bool counted = d < a.td;
    term[i] = counted ? 1.0 - d / a.td : 0.0;
    price[i] = ev_price(d, a.td);
    key[i] = counted ? (gt_rows ? i : j) : -1;
  }
  __syncthreads();  // also orders the -1 fill of match before the matched entries below
  for (int i = tid; i < n; i += kEvThreads) {
    const int k = key[i];
    if (k < 0) continue;
    if (a.match) a.match[g0 + k] = gt_rows ? s_c4r[i] : i;
    int rank = 0;  // among the counted rows, by GT index
    for (int q = 0; q < n; ++q) rank += (key[q] >= 0 && key[q] < k);
    ordered[rank] = term[i];
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += key[i] >= 0;
    double modp = 0.0, total = 0.0;
    for (int i = 0; i < c; ++i) modp += ordered[i];
    for (int i = 0; i < n; ++i) total += price[i];
    a.n_gt[f] = ng;
    a.n_det[f] = nd;
    a.matched[f] = solved ? c : -1;
    a.modp_sum[f] = modp;
    a.cost[f] = total;
  }
}

}  // namespace mvbev

extern "C" {

size_t mvbev_clear_mod_workspace_bytes(int64_t Ng, int64_t Nd, int64_t max_large) {
  using namespace mvbev;
  if (Ng < 0 || Nd < 0 || max_large <= kEvLdsCols) return 0;
  return (size_t)(Ng + Nd) * (2 * sizeof(double) + 2 * sizeof(int));
}

int mvbev_clear_mod_frames(const void* gt, const void* det, int dtype, const int32_t* gt_off, const int32_t* det_off,
                           int64_t F, int64_t Ng, int64_t Nd, int64_t max_small, int64_t max_large, double td,
                           int32_t* n_gt, int32_t* n_det, int32_t* matched, double* modp_sum, double* cost,
                           int32_t* match, void* workspace, size_t ws_bytes, void* stream) {
  using namespace mvbev;
  if (!gt_off || !det_off || !n_gt || !n_det || !matched || !modp_sum || !cost) return MVBEV_ERR_NULL;
  if ((Ng > 0 && !gt) || (Nd > 0 && !det)) return MVBEV_ERR_NULL;
  if (F <= 0 || Ng < 0 || Nd < 0 || max_small < 0 || max_large < 0) return MVBEV_ERR_RANK;
  if (dtype != MVBEV_EVAL_F32 && dtype != MVBEV_EVAL_F64 && dtype != MVBEV_EVAL_GT_F64_DET_F32) return MVBEV_ERR_SHAPE;
  if (max_small > kEvMaxRows || max_large > kEvMaxCols || max_small > max_large) return MVBEV_ERR_SHAPE;
  if (F > INT32_MAX || Ng + Nd > INT32_MAX) return MVBEV_ERR_SHAPE;
  const size_t need = mvbev_clear_mod_workspace_bytes(Ng, Nd, max_large);
  if (need) {
    if (!workspace) return MVBEV_ERR_NULL;
    if (ws_bytes < need) return MVBEV_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return MVBEV_ERR_ALIGN;
  }
  EvArgs a;
  a.gt = gt;
  a.det = det;
  a.gt_f64 = dtype != MVBEV_EVAL_F32;
  a.det_f64 = dtype == MVBEV_EVAL_F64;
  a.gt_off = gt_off;
  a.det_off = det_off;
  a.Ng = Ng;
  a.Nd = Nd;
  a.td = td;
  a.n_gt = n_gt;
  a.n_det = n_det;
  a.matched = matched;
  a.modp_sum = modp_sum;
  a.cost = cost;
  a.match = match;
  const int64_t T = need ? Ng + Nd : 0;
  double* wd = static_cast<double*>(need ? workspace : nullptr);
  a.ws.v = wd;
  a.ws.sp = wd + T;
  a.ws.path = reinterpret_cast<int*>(wd + 2 * T);
  a.ws.r4c = a.ws.path + T;
  a.ws_entries = T;
  hipLaunchKernelGGL(clear_mod_kernel, dim3((unsigned)F), dim3(kEvThreads), 0, as_stream(stream), a);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

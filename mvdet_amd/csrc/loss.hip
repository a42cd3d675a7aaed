// The training criterion on the GPU for gfx950: multiview_detector/loss/gaussian_mse.py:7-20
//   target = F.adaptive_max_pool2d(target, x.shape[2:])                 -> adaptive_max_pool_kernel
//   target = F.conv2d(target, kernel, padding=(k - 1) / 2)              -> gaussian_mse_kernel
//   F.mse_loss(x, target)                                               -> its partials + loss_finalize_kernel
// applied once to the map and once per view (trainer.py:43-47), with the per-batch counts of
// trainer.py:51-54 from the same pass, and the backward grad_x = g w 2/numel (x - t).
// An item's target is the dense tensor or the list of its non-zero cells (mvbev_loss_points): the
// conv kernel then scatters the cells into its tile itself and the item needs no pooling launch.
//
// One launch covers every item of a step (the mvbev_warp_view idiom: a by-value argument pack of
// at most kLossMaxItems items, workgroups numbered through the items).  Nothing here uses float
// atomics: every sum has a fixed order (lane, wave shuffle tree, waves in order, workgroups in
// order in fp64), so results repeat bitwise.
#include "common.h"

namespace mvbev {

constexpr int kLossMaxItems = 16;
constexpr int kLossMaxC = 8;      // slice_mask is 64 bits
constexpr int kLossThreads = 256;
constexpr int kLossTH = 16;       // output tile: 16 rows x 64 columns, 4 adjacent columns per lane
constexpr int kLossTW = 64;
constexpr int kLossLdsBytes = 64 * 1024;
constexpr int kPoolTJ = 256;      // outputs of one row per pooling workgroup
constexpr int kPoolSpan = 1024;   // source columns whose column maxima fit the workgroup's LDS

// LDS row pitch of the staged tile: the 16 lanes of a row read columns 4 apart, the 4 rows of a
// wave are one pitch apart, so pitch % 4 == 1 spreads a wave's 64 reads over 64 banks.
__host__ __device__ inline int loss_pitch(int k) {
  const int cols = kLossTW + k - 1;
  return cols + ((5 - (cols & 3)) & 3);
}

// torch's update rule (AdaptiveMaxPoolKernel: val > max || isnan(val)): NaN wins a window.
__device__ inline float pool_max(float m, float v) { return (v > m || isnan(v)) ? v : m; }

struct PoolItem {
  const float* t;
  int64_t ts[4];
  float* out;
  int32_t C, h, w, Ht, Wt, chunks, blk0;
};
struct PoolArgs {
  PoolItem it[kLossMaxItems];
  int32_t n;
};

// One workgroup per (item, b, c, output row, chunk of kPoolTJ output columns).  The source rows
// of the window are read along the row (coalesced) into per-column maxima in LDS, then each
// output takes the maximum over its column window: one write per output.  A chunk whose source
// span exceeds kPoolSpan columns (reduction factors above 4) walks its windows directly.
__global__ __launch_bounds__(kLossThreads) void adaptive_max_pool_kernel(PoolArgs a) {
  __shared__ __attribute__((aligned(16))) float colmax[kPoolSpan];
  const int tid = threadIdx.x, bid = blockIdx.x;
  int ii = 0;
  for (int i = 1; i < a.n; ++i)
    if (bid >= a.it[i].blk0) ii = i;
  const PoolItem& it = a.it[ii];
  const int local = bid - it.blk0;
  const int chunk = local % it.chunks;
  const int rest = local / it.chunks;
  const int i = rest % it.h, plane = rest / it.h;
  const int b = plane / it.C, c = plane % it.C;
  const int64_t Ht = it.Ht, Wt = it.Wt, h = it.h, w = it.w;
  const int r0 = (int)((i * Ht) / h), r1 = (int)(((i + 1) * Ht + h - 1) / h);
  const int j0 = chunk * kPoolTJ, j1 = min(j0 + kPoolTJ, it.w);
  const int c0 = (int)((j0 * Wt) / w), c1 = (int)((j1 * Wt + w - 1) / w);
  const int span = c1 - c0;
  const float* src = it.t + b * it.ts[0] + c * it.ts[1];
  float* dst = it.out + ((int64_t)plane * h + i) * w;
  if (span <= kPoolSpan) {
    // 16-byte loads where the rows allow them (unit column stride, every row of the span aligned)
    const bool vec = it.ts[3] == 1 && (it.ts[2] & 3) == 0 && (((reinterpret_cast<uintptr_t>(src) >> 2) + c0) & 3) == 0;
    const int nvec = vec ? span >> 2 : 0;
    for (int v = tid; v < nvec; v += kLossThreads) {
      float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      for (int rr = r0; rr < r1; ++rr) {
        const float4 x = *reinterpret_cast<const float4*>(src + rr * it.ts[2] + c0 + 4 * v);
        m.x = pool_max(m.x, x.x);
        m.y = pool_max(m.y, x.y);
        m.z = pool_max(m.z, x.z);
        m.w = pool_max(m.w, x.w);
      }
      *reinterpret_cast<float4*>(colmax + 4 * v) = m;
    }
    for (int cc = 4 * nvec + tid; cc < span; cc += kLossThreads) {
      float m = -INFINITY;
      for (int rr = r0; rr < r1; ++rr) m = pool_max(m, src[rr * it.ts[2] + (c0 + cc) * it.ts[3]]);
      colmax[cc] = m;
    }
    __syncthreads();
    for (int j = j0 + tid; j < j1; j += kLossThreads) {
      const int cs = (int)((j * Wt) / w) - c0, ce = (int)(((j + 1) * Wt + w - 1) / w) - c0;
      float m = -INFINITY;
      for (int cc = cs; cc < ce; ++cc) m = pool_max(m, colmax[cc]);
      dst[j] = m;
    }
  } else {
    for (int j = j0 + tid; j < j1; j += kLossThreads) {
      const int cs = (int)((j * Wt) / w), ce = (int)(((j + 1) * Wt + w - 1) / w);
      float m = -INFINITY;
      for (int rr = r0; rr < r1; ++rr)
        for (int cc = cs; cc < ce; ++cc) m = pool_max(m, src[rr * it.ts[2] + cc * it.ts[3]]);
      dst[j] = m;
    }
  }
}

struct MseItem {
  const float* x;
  int64_t xs[4];
  const float* src;  // the pooled target, or the target itself when the sizes are equal
  int64_t ss[4];
  const float* wk;
  float* t_out;
  float* diff;
  uint64_t slices;
  int32_t C, h, w, k, tiles_x, tiles_y, blk0, finite;
};
// A point item's target: the non-zero cells of the logical [B][C][Ht][Wt] target (mvbev_loss_points).
// cells == nullptr: a dense item, staged from MseItem::src.
struct MsePoints {
  const int32_t* cells;  // [n][3]: channel, row, column; batch item b owns [offs[b], offs[b + 1])
  const float* vals;     // [n], >= 0
  const int32_t* offs;   // [B + 1]
  int32_t Ht, Wt;
};
struct MseArgs {
  MseItem it[kLossMaxItems];
  MsePoints pt[kLossMaxItems];
  int32_t n, stats_item;
  float thres;
};

// The pooled positions whose adaptive_max_pool2d window [floor(i in / out), ceil((i + 1) in / out))
// holds source position p: floor(p out / in) .. ceil((p + 1) out / in) - 1 (one position when in is
// a multiple of out, up to two for uneven windows, a run of ceil(out / in) + 1 at most when in < out).
__host__ __device__ inline void pooled_range(int64_t p, int64_t in, int64_t out, int& first, int& last) {
  first = (int)((p * out) / in);
  last = (int)(((p + 1) * out + in - 1) / in) - 1;
}

// The kernel's taps are read through the constant address space: nothing writes them while the
// kernel runs, and only there can the compiler turn a load at a wave-uniform address into a scalar
// load (through a plain pointer it cannot rule out that the t_out / diff / partials stores alias
// the taps, and emits one vector load per lane).
typedef const float __attribute__((address_space(4))) * TapPtr;
__device__ __forceinline__ TapPtr as_taps(const float* p) { return (TapPtr)(uintptr_t)p; }

// The k x k taps of one (co, ci) slice for a lane's 4 adjacent outputs: along a kernel row the lane
// keeps the last three target values in registers and reads one new value from LDS per tap.  K > 0:
// the row loop unrolls, so a row's taps arrive in a few wide scalar loads and its LDS reads issue
// together; K == 0: any k, taps loaded as the loop goes.
template <int K>
__device__ __forceinline__ void conv_rows(const float* __restrict__ tb, TapPtr wp, int k, int pitch,
                                          float (&acc)[4]) {
  const int kk = K > 0 ? K : k;
  constexpr int kUnroll = K > 0 ? K : 4;
  for (int ky = 0; ky < kk; ++ky) {
    const float* tr = tb + ky * pitch;
    const TapPtr wr = wp + ky * kk;
    float v0 = tr[0], v1 = tr[1], v2 = tr[2];
#pragma unroll kUnroll
    for (int kx = 0; kx < kk; ++kx) {
      const float v3 = tr[kx + 3];
      const float wv = wr[kx];
      acc[0] = fmaf(wv, v0, acc[0]);
      acc[1] = fmaf(wv, v1, acc[1]);
      acc[2] = fmaf(wv, v2, acc[2]);
      acc[3] = fmaf(wv, v3, acc[3]);
      v0 = v1;
      v1 = v2;
      v2 = v3;
    }
  }
}

// One workgroup per (item, b, 16 x 64 output tile), all output channels.  Lane (ly, lx) owns the
// 4 adjacent outputs (ly, 4 lx .. 4 lx + 3): along a kernel row it keeps the last three target
// values in registers and reads one new value from LDS per tap (4 FMAs per LDS read).  The tap
// index is wave-uniform, so the taps come through scalar loads, once per wave.
__global__ __launch_bounds__(kLossThreads) void gaussian_mse_kernel(MseArgs a, double* __restrict__ partials) {
  extern __shared__ float tile[];
  __shared__ unsigned nz_mask;
  __shared__ double red_d[2][kLossThreads / kWave];
  __shared__ int red_i[2][kLossThreads / kWave];
  const int tid = threadIdx.x, bid = blockIdx.x;
  int ii = 0;
  for (int i = 1; i < a.n; ++i)
    if (bid >= a.it[i].blk0) ii = i;
  const MseItem& it = a.it[ii];
  const int local = bid - it.blk0;
  const int tile_x = local % it.tiles_x;
  const int rest = local / it.tiles_x;
  const int tile_y = rest % it.tiles_y, b = rest / it.tiles_y;
  const int C = it.C, h = it.h, w = it.w, k = it.k, r = k >> 1;
  const int rows = kLossTH + k - 1, cols = kLossTW + k - 1, pitch = loss_pitch(k);
  const int plane = rows * pitch;
  const int y0 = tile_y * kLossTH, x0 = tile_x * kLossTW;

  // stage the target tile and its halo, zeros outside the image; note which channels hold a non-zero
  if (tid == 0) nz_mask = 0;
  __syncthreads();
  unsigned nz = 0;
  const MsePoints& pt = a.pt[ii];
  if (pt.cells) {
    // a point item: zero the tile, then raise every pooled cell whose window holds a point to the
    // point's value.  Values are >= 0, where the integer order of the bits is the float order, and a
    // maximum does not depend on the order of arrival: the tile is what the dense path stages from
    // the pooled dense target, word for word.
    for (int i = tid; i < C * plane; i += kLossThreads) tile[i] = 0.f;
    __syncthreads();
    const int p1 = pt.offs[b + 1];
    for (int p = pt.offs[b] + tid; p < p1; p += kLossThreads) {
      const int ci = pt.cells[3 * (int64_t)p];
      const float v = pt.vals[p];
      if ((unsigned)ci >= (unsigned)C || !(v > 0.f)) continue;
      int i0, i1, j0, j1;
      pooled_range(pt.cells[3 * (int64_t)p + 1], pt.Ht, h, i0, i1);
      pooled_range(pt.cells[3 * (int64_t)p + 2], pt.Wt, w, j0, j1);
      // clip to the image, then to the tile plus its halo
      const int ry0 = max(max(i0, 0) - (y0 - r), 0), ry1 = min(min(i1, h - 1) - (y0 - r), rows - 1);
      const int rx0 = max(max(j0, 0) - (x0 - r), 0), rx1 = min(min(j1, w - 1) - (x0 - r), cols - 1);
      if (ry0 > ry1 || rx0 > rx1) continue;
      nz |= 1u << ci;
      int* tp = reinterpret_cast<int*>(tile + ci * plane);
      for (int ry = ry0; ry <= ry1; ++ry)
        for (int rx = rx0; rx <= rx1; ++rx) atomicMax(tp + ry * pitch + rx, __float_as_int(v));
    }
  } else {
    for (int ci = 0; ci < C; ++ci) {
      const float* sp = it.src + b * it.ss[0] + ci * it.ss[1];
      float* tp = tile + ci * plane;
      for (int ry = tid >> 6; ry < rows; ry += kLossThreads / 64) {
        const int gy = y0 - r + ry;
        const bool iny = gy >= 0 && gy < h;
        for (int rx = tid & 63; rx < cols; rx += 64) {
          const int gx = x0 - r + rx;
          float v = 0.f;
          if (iny && gx >= 0 && gx < w) v = sp[gy * it.ss[2] + gx * it.ss[3]];
          tp[ry * pitch + rx] = v;
          if (v != 0.f) nz |= 1u << ci;  // NaN counts as non-zero
        }
      }
    }
  }
  if (nz) atomicOr(&nz_mask, nz);
  __syncthreads();
  nz = nz_mask;

  const int ly = tid >> 4, lx = (tid & 15) * 4;
  const int gy = y0 + ly, gx = x0 + lx;
  const bool skips = it.finite != 0;
  const bool stats = ii == a.stats_item;
  float sse = 0.f, gt_sum = 0.f;
  int tp_n = 0, pred_n = 0;
  for (int co = 0; co < C; ++co) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ci = 0; ci < C; ++ci) {
      // exact skips (finite kernels only): an all-zero slice, an all-zero staged channel
      if (skips && (!((it.slices >> (co * C + ci)) & 1) || !((nz >> ci) & 1))) continue;
      const TapPtr wp = as_taps(it.wk) + (int64_t)(co * C + ci) * k * k;
      const float* tb = tile + ci * plane + ly * pitch + lx;
      if (!skips) {
        // a non-finite kernel: torch's conv never multiplies the padding, so a NaN / Inf tap reaches
        // an output only through a target cell inside the image (0 * NaN there, nothing outside)
        for (int ky = 0; ky < k; ++ky) {
          const float* tr = tb + ky * pitch;
          const TapPtr wr = wp + ky * k;
          const int sy = gy + ky - r;
          if (sy < 0 || sy >= h) continue;
          for (int kx = 0; kx < k; ++kx) {
            const float wv = wr[kx];
            const int sx = gx + kx - r;
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (sx + q >= 0 && sx + q < w) acc[q] = fmaf(wv, tr[kx + q], acc[q]);
          }
        }
        continue;
      }
      // the reference's two kernel sizes get compile-time loops; any other odd k the generic one
      switch (k) {
        case 21: conv_rows<21>(tb, wp, k, pitch, acc); break;
        case 41: conv_rows<41>(tb, wp, k, pitch, acc); break;
        default: conv_rows<0>(tb, wp, k, pitch, acc); break;
      }
    }
    if (gy < h) {
      const int64_t o = (((int64_t)b * C + co) * h + gy) * w + gx;
      const float* xp = it.x ? it.x + b * it.xs[0] + co * it.xs[1] + gy * it.xs[2] : nullptr;
      const float* gp = tile + co * plane + (ly + r) * pitch + lx + r;  // the raw target under this lane
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (gx + q >= w) continue;
        const float t = acc[q];
        if (it.t_out) it.t_out[o + q] = t;
        if (xp) {
          const float xv = xp[(gx + q) * it.xs[3]];
          const float d = xv - t;
          if (it.diff) it.diff[o + q] = d;
          sse += d * d;
          if (stats) {
            const float gt = gp[q];
            const bool p = xv > a.thres;  // NaN compares false
            pred_n += p;
            tp_n += p && gt == 1.f;
            gt_sum += gt;
          }
        }
      }
    }
  }

  // workgroup sums in a fixed order: shuffle tree per wave, then the waves in order
  double s0 = sse, s1 = gt_sum;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off);
    s1 += __shfl_down(s1, off);
    tp_n += __shfl_down(tp_n, off);
    pred_n += __shfl_down(pred_n, off);
  }
  if ((tid & (kWave - 1)) == 0) {
    red_d[0][tid >> 6] = s0;
    red_d[1][tid >> 6] = s1;
    red_i[0][tid >> 6] = tp_n;
    red_i[1][tid >> 6] = pred_n;
  }
  __syncthreads();
  if (tid == 0) {
    double p0 = 0, p3 = 0;
    int p1 = 0, p2 = 0;
    for (int wv = 0; wv < kLossThreads / kWave; ++wv) {
      p0 += red_d[0][wv];
      p3 += red_d[1][wv];
      p1 += red_i[0][wv];
      p2 += red_i[1][wv];
    }
    double* pp = partials + (int64_t)bid * 4;
    pp[0] = p0;
    pp[1] = p1;
    pp[2] = p2;
    pp[3] = p3;
  }
}

struct FinItem {
  int32_t blk0, nblk;
  double scale;  // weight / numel
};
struct FinArgs {
  FinItem it[kLossMaxItems];
  int32_t n, stats_item;
};

// sum of column col of rows [r0, r0 + nr) of the partials: thread t takes rows t, t + 256, ...
// in order, then a fixed tree over the workgroup; every thread returns the total
__device__ double partial_sum(const double* __restrict__ partials, int r0, int nr, int col, double* red) {
  const int tid = threadIdx.x;
  double s = 0;
  for (int g = tid; g < nr; g += kLossThreads) s += partials[(int64_t)(r0 + g) * 4 + col];
  __syncthreads();  // red is reused from call to call
  red[tid] = s;
  __syncthreads();
  for (int off = kLossThreads / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kLossThreads) void loss_finalize_kernel(FinArgs a, const double* __restrict__ partials,
                                                                     float* __restrict__ loss,
                                                                     double* __restrict__ stats) {
  __shared__ double red[kLossThreads];
  double total = 0;
  for (int i = 0; i < a.n; ++i) total += a.it[i].scale * partial_sum(partials, a.it[i].blk0, a.it[i].nblk, 0, red);
  if (threadIdx.x == 0) *loss = (float)total;
  if (stats && a.stats_item >= 0) {
    const FinItem it = a.it[a.stats_item];
    const double tp = partial_sum(partials, it.blk0, it.nblk, 1, red);
    const double pred = partial_sum(partials, it.blk0, it.nblk, 2, red);
    const double gt = partial_sum(partials, it.blk0, it.nblk, 3, red);
    if (threadIdx.x == 0) {
      stats[0] = tp;
      stats[1] = pred - tp;
      stats[2] = gt - tp;
    }
  }
}

struct BwdItem {
  const float* diff;
  float* grad;
  int64_t numel;
  int32_t blk0;
  float weight;
};
struct BwdArgs {
  BwdItem it[kLossMaxItems];
  int32_t n;
};

__global__ __launch_bounds__(kLossThreads) void gaussian_mse_backward_kernel(BwdArgs a,
                                                                             const float* __restrict__ grad_out) {
  const int bid = blockIdx.x;
  int ii = 0;
  for (int i = 1; i < a.n; ++i)
    if (bid >= a.it[i].blk0) ii = i;
  const BwdItem& it = a.it[ii];
  const float scale = (float)((double)*grad_out * (double)it.weight * 2.0 / (double)it.numel);
  const int64_t e = (int64_t)(bid - it.blk0) * kLossThreads + threadIdx.x;
  if (e < it.numel) it.grad[e] = scale * it.diff[e];
}

// the checks every entry point shares; the per-item workgroup counts of the conv kernel
static int loss_check_items(const mvbev_loss_item* items, int n, int64_t B) {
  if (!items) return MVBEV_ERR_NULL;
  if (n <= 0 || B <= 0) return MVBEV_ERR_RANK;
  if (n > kLossMaxItems) return MVBEV_ERR_SHAPE;
  for (int i = 0; i < n; ++i) {
    const mvbev_loss_item& it = items[i];
    if (it.C <= 0 || it.h <= 0 || it.w <= 0 || it.Ht <= 0 || it.Wt <= 0) return MVBEV_ERR_RANK;
    if (it.C > kLossMaxC || B * it.C * it.h * it.w > INT32_MAX || B * it.C * it.Ht * it.Wt > INT32_MAX * (int64_t)64)
      return MVBEV_ERR_SHAPE;
    for (int d = 0; d < 4; ++d)
      if (it.x_strides[d] < 0 || it.t_strides[d] < 0) return MVBEV_ERR_STRIDE;
  }
  return MVBEV_OK;
}

static int64_t loss_item_blocks(const mvbev_loss_item& it, int64_t B) {
  return B * ceil_div(it.h, (int64_t)kLossTH) * ceil_div(it.w, (int64_t)kLossTW);
}

// mvbev_gaussian_mse_f32 (points == nullptr) and mvbev_gaussian_mse_points_f32
static int launch_gaussian_mse(const mvbev_loss_item* items, const mvbev_loss_points* points, int n, int64_t B,
                               const mvbev_loss_kernel* kernels, int nkernels, float cls_thres, int stats_item,
                               double* partials, int64_t npartials, void* stream) {
  const int st = loss_check_items(items, n, B);
  if (st != MVBEV_OK) return st;
  if (!kernels || !partials) return MVBEV_ERR_NULL;
  if (nkernels <= 0) return MVBEV_ERR_RANK;
  if (stats_item < -1 || stats_item >= n) return MVBEV_ERR_SHAPE;
  MseArgs a = {};
  a.n = n, a.stats_item = stats_item, a.thres = cls_thres;
  int64_t blocks = 0, lds = 0;
  for (int i = 0; i < n; ++i) {
    const mvbev_loss_item& it = items[i];
    if (it.kernel_id < 0 || it.kernel_id >= nkernels) return MVBEV_ERR_SHAPE;
    const mvbev_loss_kernel& kn = kernels[it.kernel_id];
    if (kn.k <= 0) return MVBEV_ERR_RANK;
    if (kn.k % 2 == 0 || kn.C != it.C || kn.k > 1023) return MVBEV_ERR_SHAPE;
    const int k = (int)kn.k;
    const int64_t bytes = it.C * (kLossTH + k - 1) * (int64_t)loss_pitch(k) * (int64_t)sizeof(float);
    if (bytes > kLossLdsBytes - 256) return MVBEV_ERR_SHAPE;  // 256 B: the kernel's static LDS
    const bool same = it.Ht == it.h && it.Wt == it.w;
    if (i == stats_item && (!same || !it.x)) return MVBEV_ERR_SHAPE;
    // a point record: all three pointers or none (none: a dense item), the item's own Ht x Wt
    const mvbev_loss_points* rec = points ? points + i : nullptr;
    const bool pts = rec && (rec->cells || rec->values || rec->offsets);
    if (pts) {
      if (!rec->cells || !rec->values || !rec->offsets) return MVBEV_ERR_NULL;
      if (rec->Ht != it.Ht || rec->Wt != it.Wt || it.Ht > INT32_MAX || it.Wt > INT32_MAX) return MVBEV_ERR_SHAPE;
      if (!kn.w || (!it.x && !it.t_out)) return MVBEV_ERR_NULL;
    } else if (!kn.w || !it.target || (!same && !it.pooled) || (!it.x && !it.t_out)) {
      return MVBEV_ERR_NULL;
    }
    if (!it.x && it.diff) return MVBEV_ERR_NULL;
    lds = std::max(lds, bytes);
    MseItem& m = a.it[i];
    m.x = it.x;
    m.src = same ? it.target : it.pooled;
    const int64_t contiguous[4] = {it.C * it.h * it.w, it.h * it.w, it.w, 1};
    for (int d = 0; d < 4; ++d) {
      m.xs[d] = it.x_strides[d];
      m.ss[d] = same ? it.t_strides[d] : contiguous[d];
    }
    m.wk = kn.w, m.t_out = it.t_out, m.diff = it.diff, m.slices = kn.slice_mask;
    m.C = (int32_t)it.C, m.h = (int32_t)it.h, m.w = (int32_t)it.w, m.k = k, m.finite = kn.finite;
    m.tiles_x = (int32_t)ceil_div(it.w, (int64_t)kLossTW);
    m.tiles_y = (int32_t)ceil_div(it.h, (int64_t)kLossTH);
    if (pts) {
      MsePoints& q = a.pt[i];
      q.cells = rec->cells, q.vals = rec->values, q.offs = rec->offsets;
      q.Ht = (int32_t)it.Ht, q.Wt = (int32_t)it.Wt;
      m.src = nullptr;
    }
    m.blk0 = (int32_t)blocks;
    blocks += loss_item_blocks(it, B);
    if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  }
  if (npartials < 4 * blocks) return MVBEV_ERR_SHAPE;
  hipLaunchKernelGGL(gaussian_mse_kernel, dim3((unsigned)blocks), dim3(kLossThreads), (size_t)lds, as_stream(stream),
                     a, partials);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // namespace mvbev

extern "C" {

int mvbev_adaptive_max_pool_f32(const mvbev_loss_item* items, int n, int64_t B, void* stream) {
  using namespace mvbev;
  const int st = loss_check_items(items, n, B);
  if (st != MVBEV_OK) return st;
  PoolArgs a = {};
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    const mvbev_loss_item& it = items[i];
    if (it.Ht == it.h && it.Wt == it.w) continue;
    if (!it.target || !it.pooled) return MVBEV_ERR_NULL;
    PoolItem& p = a.it[a.n++];
    p.t = it.target;
    for (int d = 0; d < 4; ++d) p.ts[d] = it.t_strides[d];
    p.out = it.pooled;
    p.C = (int32_t)it.C, p.h = (int32_t)it.h, p.w = (int32_t)it.w, p.Ht = (int32_t)it.Ht, p.Wt = (int32_t)it.Wt;
    p.chunks = (int32_t)ceil_div(it.w, (int64_t)kPoolTJ);
    p.blk0 = (int32_t)blocks;
    blocks += B * it.C * it.h * p.chunks;
    if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  }
  if (a.n == 0) return MVBEV_OK;
  hipLaunchKernelGGL(adaptive_max_pool_kernel, dim3((unsigned)blocks), dim3(kLossThreads), 0, as_stream(stream), a);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int64_t mvbev_gaussian_mse_blocks(const mvbev_loss_item* items, int n, int64_t B) {
  using namespace mvbev;
  if (loss_check_items(items, n, B) != MVBEV_OK) return 0;
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) blocks += loss_item_blocks(items[i], B);
  return blocks <= INT32_MAX ? blocks : 0;
}

int mvbev_gaussian_mse_f32(const mvbev_loss_item* items, int n, int64_t B, const mvbev_loss_kernel* kernels,
                           int nkernels, float cls_thres, int stats_item, double* partials, int64_t npartials,
                           void* stream) {
  return mvbev::launch_gaussian_mse(items, nullptr, n, B, kernels, nkernels, cls_thres, stats_item, partials,
                                    npartials, stream);
}

int mvbev_gaussian_mse_points_f32(const mvbev_loss_item* items, const mvbev_loss_points* points, int n, int64_t B,
                                  const mvbev_loss_kernel* kernels, int nkernels, float cls_thres, int stats_item,
                                  double* partials, int64_t npartials, void* stream) {
  if (!points) return MVBEV_ERR_NULL;
  return mvbev::launch_gaussian_mse(items, points, n, B, kernels, nkernels, cls_thres, stats_item, partials,
                                    npartials, stream);
}

int mvbev_loss_finalize_f32(const mvbev_loss_item* items, int n, int64_t B, const double* partials,
                            int64_t npartials, int stats_item, float* loss, double* stats, void* stream) {
  using namespace mvbev;
  const int st = loss_check_items(items, n, B);
  if (st != MVBEV_OK) return st;
  if (!partials || !loss) return MVBEV_ERR_NULL;
  if (stats_item < -1 || stats_item >= n) return MVBEV_ERR_SHAPE;
  FinArgs a = {};
  a.n = n, a.stats_item = stats_item;
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t nb = loss_item_blocks(items[i], B);
    a.it[i].blk0 = (int32_t)blocks;
    a.it[i].nblk = (int32_t)nb;
    a.it[i].scale = (double)items[i].weight / (double)(B * items[i].C * items[i].h * items[i].w);
    blocks += nb;
    if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  }
  if (npartials < 4 * blocks) return MVBEV_ERR_SHAPE;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kLossThreads), 0, as_stream(stream), a, partials, loss,
                     stats);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_gaussian_mse_backward_f32(const mvbev_loss_item* items, int n, int64_t B, const float* grad_out,
                                    float* const* grads, void* stream) {
  using namespace mvbev;
  const int st = loss_check_items(items, n, B);
  if (st != MVBEV_OK) return st;
  if (!grad_out || !grads) return MVBEV_ERR_NULL;
  BwdArgs a = {};
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (!grads[i]) continue;  // no gradient wanted for this item
    if (!items[i].diff) return MVBEV_ERR_NULL;
    BwdItem& b = a.it[a.n++];
    b.diff = items[i].diff, b.grad = grads[i];
    b.numel = B * items[i].C * items[i].h * items[i].w;
    b.weight = items[i].weight;
    b.blk0 = (int32_t)blocks;
    blocks += ceil_div(b.numel, (int64_t)kLossThreads);
  }
  if (a.n == 0) return MVBEV_OK;
  hipLaunchKernelGGL(gaussian_mse_backward_kernel, dim3((unsigned)blocks), dim3(kLossThreads), 0, as_stream(stream),
                     a, grad_out);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

// The first conv of the "late fusion" ablation's ground-plane head (res_proj_variant.py:53, :70-82), fused with
// everything in front of it, for gfx950:
//   x[b][c]   = kornia warp of view c's single (foot) plane, c < N;  x[b][N], x[b][N + 1] = the coord map
//   y1[b][co] = relu(b1[co] + sum_c sum_t w1[co][c][t] * x[b][c][p + s_t])        (3x3, padding 1)
// The input has N + 2 channels (9 at config 2, K = 81): the cost of this conv is the write of y1, so it is a plain
// fp32 VALU kernel.  Neither the warped planes nor the concatenated tensor are written in inference.
//
// Forward thread mapping.  A block owns an 8 x 32 pixel tile of one batch item and 64 output channels.  Phase 1
// stages the N + 2 channels of the tile grown by one pixel in LDS: one warp sample (warp_common.h's warp_coord, the
// blend of warp_tile_kernel, corner loads through L1 / L2) or coord value per (channel, halo pixel), zero outside
// the grid.  A view none of whose staged samples is inside its source (or non-finite) is marked dead: geometry
// only, and it adds exact zeros — unless its w1 columns hold a NaN / inf (bit v of the device word w_mask,
// thin_conv1_weight_mask_kernel, once per weight version): 0 * NaN is NaN in the reference, so such a view is
// evaluated over every tile.  Phase 2: one thread per pixel, 8 output channels per pass; the weights are
// wave-uniform and come through scalar loads, every tap is multiplied (a NaN sample reaches its 3 x 3
// neighbourhood in every channel), the sum runs in a fixed order: per output channel three partial sums over the
// input channels in order — taps (0, 2, 4, 6) from the bias, taps (1, 3, 5, 7), tap 8 — added at the end (two
// neighbouring weights are one 64-bit scalar operand of a packed FMA).
// Split-bf16 output: the pass's 8 channels are one 32-B entry (store_split8).
//
// Backward (dpre = the gradient of the pre-activation, masked by the caller):
//   thin_conv1_dx_kernel   dxw[b][v][p] = sum_co sum_t w1[co][v][t] dpre[b][co][p - s_t]: a block owns 4 x 32
//                          pixels, its two thread halves take alternate 8-channel runs of dpre (staged with a halo
//                          in LDS) and are added in a fixed order at the end.
//   thin_conv1_dw_kernel   per (pixel tile, 256 output channels, 4 views): thread = output channel; the tile's
//                          rows of dpre pass through LDS transposed, the warped planes' taps are LDS broadcasts.
//                          Leaves partials[tile][co][v][t]; thin_conv1_dw_reduce_kernel adds the tiles in order in
//                          fp64.
// No float atomics: results repeat bitwise.
#include "warp_common.h"

namespace mvbev {

constexpr int kTcTH = 8, kTcTW = 32;              // forward / dw pixel tile
constexpr int kTcThreads = kTcTH * kTcTW;         // one thread per pixel
constexpr int kTcHH = kTcTH + 2, kTcHW = kTcTW + 2;  // the staged tile with its halo
constexpr int kTcMaxCh = kWarpMaxViews + 2;
// output channels per forward block.  cfg2 (7 planes, 120 x 360, Cout 512; interleaved A/B, 4 rounds of 30 launches):
// 256 131.6-134.5 us, 128 83.2-87.7, 64 78.0-82.9 — the launch is 180 pixel tiles, so the slices are what fills the
// 256 CUs (5.6 workgroups each at 64), and the scalar weight loads' latency needs the waves to hide behind
#ifndef MVBEV_TC_COUT_BLOCK
#define MVBEV_TC_COUT_BLOCK 64
#endif
constexpr int kTcCoutBlock = MVBEV_TC_COUT_BLOCK;  // output channels per forward block
constexpr int kTcDxTH = 4;                        // dx tile rows (x kTcTW columns, two thread halves)
constexpr int kTcDxChunk = 16;                    // dpre channels staged per step (8 per half)
constexpr int kTcDwViews = 4;                     // views per dw block
constexpr int kTcDwPitch = 36;                    // staged plane row pitch of the dw kernel (16-B aligned rows)

struct TcArgs {
  WarpArgs w;  // views (src = the planes, sC unused), H, W, Ho, Wo, B, nviews, tiles_x, tiles (per item), nwg
  int Cout, cslices, split;
};

// mvbev_warp_perspective_f32's sample of plane `base` (row stride sH, column stride 1) at output pixel (u, v)
__device__ inline float tc_sample(const float* __restrict__ base, int64_t sH, const float (&m)[9], int u, int v, int Ho,
                                  int Wo, int H, int W, bool& live) {
  const WarpCoord wc = warp_coord(m, u, v, Ho, Wo, H, W);
  if (!wc.finite) {
    live = true;
    return __builtin_nanf("");
  }
  if (!wc.inside) return 0.f;
  live = true;
  const float ix = wc.ix, iy = wc.iy;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  const float w_nw = (fx1 - ix) * (fy1 - iy), w_ne = (ix - fx0) * (fy1 - iy);
  const float w_sw = (fx1 - ix) * (iy - fy0), w_se = (ix - fx0) * (iy - fy0);
  const bool vx0 = x0 >= 0, vx1 = x0 + 1 <= W - 1, vy0 = y0 >= 0, vy1 = y0 + 1 <= H - 1;
  const int cx0 = max(x0, 0), cy0 = max(y0, 0), cx1 = min(x0 + 1, W - 1), cy1 = min(y0 + 1, H - 1);
  const float* r0 = base + cy0 * sH;
  const float* r1 = base + cy1 * sH;
  const float vnw = r0[cx0], vne = r0[cx1], vsw = r1[cx0], vse = r1[cx1];
  float acc = 0.f;  // invalid corners are replaced by 0 (a select, not a zero weight), as warp_tile_kernel
  acc += (vx0 && vy0 ? vnw : 0.f) * w_nw;
  acc += (vx1 && vy0 ? vne : 0.f) * w_ne;
  acc += (vx0 && vy1 ? vsw : 0.f) * w_sw;
  acc += (vx1 && vy1 ? vse : 0.f) * w_se;
  return acc;
}

// (the weights and the bias are parameters of their own, __restrict__: with the stores to y1 known not to alias them
// their wave-uniform loads become scalar loads)
__global__ __launch_bounds__(kTcThreads) void thin_conv1_fwd_kernel(const TcArgs ta, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1,
                                                                   void* __restrict__ y1, float* __restrict__ xwp,
                                                                   const int32_t* __restrict__ w_mask) {
  __shared__ float xs[kTcMaxCh][kTcHH][kTcHW];
  __shared__ int live[kTcMaxCh];
  const WarpArgs& a = ta.w;
  const int tid = threadIdx.x;
  const int N = a.nviews, nch = N + 2, Ho = a.Ho, Wo = a.Wo;
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int cs = lb % ta.cslices;  // the Cout slices of a tile are neighbours: they share the planes' lines
  const int rest = lb / ta.cslices;
  const int tile = rest % a.tiles, b = rest / a.tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r0 = ty * kTcTH, u0 = tx * kTcTW;

  // the coord channels always count, and a view whose weights are non-finite (0 * NaN = NaN)
  if (tid < kTcMaxCh) live[tid] = tid >= N || (w_mask && ((*w_mask >> tid) & 1));
  __syncthreads();
  // phase 1
  for (int it = tid; it < nch * (kTcHH * kTcHW); it += kTcThreads) {
    const int c = it / (kTcHH * kTcHW), q = it - c * (kTcHH * kTcHW);
    const int hr = q / kTcHW, hc = q - hr * kTcHW;
    const int r = r0 + hr - 1, u = u0 + hc - 1;
    float val = 0.f;  // nn.Conv2d's zero padding, coord channels included
    if (r >= 0 && r < Ho && u >= 0 && u < Wo) {
      if (c < N) {
        const WarpView& vw = a.v[c];
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = vw.m[k];
        bool lv = false;
        val = tc_sample(static_cast<const float*>(vw.src) + (int64_t)b * vw.sB, vw.sH, m, u, r, Ho, Wo, a.H, a.W, lv);
        if (lv) live[c] = 1;  // (every writer stores the same value)
        if (xwp && cs == 0 && hr >= 1 && hr <= kTcTH && hc >= 1 && hc <= kTcTW)
          xwp[(((int64_t)b * N + c) * Ho + r) * Wo + u] = val;
      } else if (c == N) {  // mvbev_fill_coord_map_f32's values
        val = coord_value(u, Wo);
      } else {
        val = coord_value(r, Ho);
      }
    }
    xs[c][hr][hc] = val;
  }
  __syncthreads();

  // phase 2
  const int pr = tid / kTcTW, pc = tid - pr * kTcTW;
  const int r = r0 + pr, u = u0 + pc;
  const bool pix = r < Ho && u < Wo;
  const int K = nch * 9;
  const int co_begin = cs * kTcCoutBlock, co_end = min(ta.Cout, co_begin + kTcCoutBlock);
  const int64_t npix = (int64_t)Ho * Wo;
  for (int co0 = co_begin; co0 < co_end; co0 += 8) {
    // per output channel: a pair of sums over the taps (0, 1), (2, 3), (4, 5), (6, 7) of every channel — the two
    // weights of a pair are neighbours in w1, so one packed FMA takes them as one 64-bit scalar operand — and a
    // third over tap 8; the bias starts the first
    f32x2_t acc2[8];
    float acc1[8], acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc2[j] = f32x2_t{b1 ? b1[co0 + j] : 0.f, 0.f}, acc1[j] = 0.f;
    for (int c = 0; c < nch; ++c) {
      if (!live[c]) continue;  // uniform over the block
      float x[9];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) x[3 * kh + kw] = xs[c][pr + kh][pc + kw];
      const float* __restrict__ wp = w1 + (int64_t)co0 * K + c * 9;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int t = 0; t < 8; t += 2)
          acc2[j] = __builtin_elementwise_fma(f32x2_t{wp[j * K + t], wp[j * K + t + 1]}, f32x2_t{x[t], x[t + 1]}, acc2[j]);
        acc1[j] = fmaf(wp[j * K + 8], x[8], acc1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = (acc2[j].x + acc2[j].y) + acc1[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = relu_nan(acc[j]);
    if (!pix) continue;
    if (ta.split) {
      u32x4_t* out = static_cast<u32x4_t*>(y1) + 2 * (((int64_t)b * (ta.Cout / 8) + co0 / 8) * npix + (int64_t)r * Wo + u);
      store_split8(out, acc);
    } else {
      float* out = static_cast<float*>(y1) + ((int64_t)b * ta.Cout + co0) * npix + (int64_t)r * Wo + u;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j * npix] = acc[j];
    }
  }
}

// bit v of *mask = w1[:, v] (v < N) holds a NaN / inf.  One workgroup: the word is written whole by every launch.
__global__ __launch_bounds__(1024) void thin_conv1_weight_mask_kernel(const float* __restrict__ w1, int N, int64_t n,
                                                                      int32_t* __restrict__ mask) {
  __shared__ int m;
  if (threadIdx.x == 0) m = 0;
  __syncthreads();
  int mine = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const int c = (int)((i / 9) % (N + 2));
    if (c < N && !isfinite(w1[i])) mine |= 1 << c;
  }
  if (mine) atomicOr(&m, mine);
  __syncthreads();
  if (threadIdx.x == 0) *mask = m;
}

struct TcBwdArgs {
  const float* dpre;
  const float* w1;
  const float* xw;
  float* dxw;
  float* partials;
  int N, B, Cout, Ho, Wo, tiles_x, tiles, nwg;
};

// (w1 and dxw as __restrict__ parameters of their own: scalar weight loads, as in the forward)
__global__ __launch_bounds__(256) void thin_conv1_dx_kernel(const TcBwdArgs a, const float* __restrict__ w1,
                                                            float* __restrict__ dxw) {
  constexpr int HH = kTcDxTH + 2, NPX = kTcDxTH * kTcTW;  // 6 x 34 staged pixels per channel, 128 pixels
  __shared__ float ds[kTcDxChunk][HH][kTcHW];
  __shared__ float red[kWarpMaxViews][NPX];
  const int tid = threadIdx.x;
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int tile = lb % a.tiles, b = lb / a.tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r0 = ty * kTcDxTH, u0 = tx * kTcTW;
  const int px = tid & (NPX - 1);
  const int half = __builtin_amdgcn_readfirstlane(tid >> 7);  // a half is two whole waves: uniform, scalar weight loads
  const int pr = px / kTcTW, pc = px - pr * kTcTW;
  const int N = a.N, Ho = a.Ho, Wo = a.Wo, K = (N + 2) * 9;
  const int64_t npix = (int64_t)Ho * Wo;
  float acc[kWarpMaxViews];
#pragma unroll
  for (int v = 0; v < kWarpMaxViews; ++v) acc[v] = 0.f;
  for (int c0 = 0; c0 < a.Cout; c0 += kTcDxChunk) {
    __syncthreads();  // the previous chunk's readers
    for (int it = tid; it < kTcDxChunk * HH * kTcHW; it += 256) {
      const int cc = it / (HH * kTcHW), q = it - cc * (HH * kTcHW);
      const int hr = q / kTcHW, hc = q - hr * kTcHW;
      const int r = r0 + hr - 1, u = u0 + hc - 1, co = c0 + cc;
      float val = 0.f;
      if (co < a.Cout && r >= 0 && r < Ho && u >= 0 && u < Wo) val = a.dpre[((int64_t)b * a.Cout + co) * npix + (int64_t)r * Wo + u];
      ds[cc][hr][hc] = val;
    }
    __syncthreads();
    for (int j = 0; j < 8; ++j) {
      const int cc = 8 * half + j, co = c0 + cc;
      if (co >= a.Cout) break;  // uniform over the wave
      float d[9];  // d[t] = dpre[p - s_t]: tap (kh, kw) reads the pixel at (-(kh - 1), -(kw - 1))
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) d[3 * kh + kw] = ds[cc][pr + 2 - kh][pc + 2 - kw];
      const float* __restrict__ wp = w1 + (int64_t)co * K;
#pragma unroll
      for (int v = 0; v < kWarpMaxViews; ++v) {
        if (v < N) {
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[v] = fmaf(wp[v * 9 + t], d[t], acc[v]);
        }
      }
    }
  }
  if (half == 1) {
#pragma unroll
    for (int v = 0; v < kWarpMaxViews; ++v) red[v][px] = acc[v];
  }
  __syncthreads();
  if (half == 0) {
    const int r = r0 + pr, u = u0 + pc;
    if (r < Ho && u < Wo) {
#pragma unroll
      for (int v = 0; v < kWarpMaxViews; ++v)
        if (v < N) dxw[((int64_t)b * N + v) * npix + (int64_t)r * Wo + u] = acc[v] + red[v][px];
    }
  }
}

// grid (pixel tiles of all items, Cout / 256, N / 4): thread = output channel
__global__ __launch_bounds__(256) void thin_conv1_dw_kernel(const TcBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kTcDwViews][kTcHH][kTcDwPitch];
  __shared__ float dl[256][kTcTW + 1];
  const int tid = threadIdx.x;
  const int blk = blockIdx.x, tile = blk % a.tiles, b = blk / a.tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r0 = ty * kTcTH, u0 = tx * kTcTW;
  const int co0 = blockIdx.y * 256, v0 = blockIdx.z * kTcDwViews;
  const int N = a.N, Ho = a.Ho, Wo = a.Wo;
  const int64_t npix = (int64_t)Ho * Wo;
  for (int it = tid; it < kTcDwViews * kTcHH * kTcDwPitch; it += 256) {
    const int vi = it / (kTcHH * kTcDwPitch), q = it - vi * (kTcHH * kTcDwPitch);
    const int hr = q / kTcDwPitch, hc = q - hr * kTcDwPitch;
    const int r = r0 + hr - 1, u = u0 + hc - 1, v = v0 + vi;
    float val = 0.f;
    if (v < N && hc < kTcHW && r >= 0 && r < Ho && u >= 0 && u < Wo) val = a.xw[((int64_t)b * N + v) * npix + (int64_t)r * Wo + u];
    xs[vi][hr][hc] = val;
  }
  float acc[kTcDwViews][9];
#pragma unroll
  for (int vi = 0; vi < kTcDwViews; ++vi)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[vi][t] = 0.f;
  for (int rr = 0; rr < kTcTH; ++rr) {
    const int r = r0 + rr;
    if (r >= Ho) break;
    __syncthreads();  // the previous row's readers (and, first, the planes' writers)
    for (int it = tid; it < 256 * kTcTW; it += 256) {
      const int cl = it / kTcTW, p = it - cl * kTcTW;
      const int co = co0 + cl, u = u0 + p;
      dl[cl][p] = (co < a.Cout && u < Wo) ? a.dpre[((int64_t)b * a.Cout + co) * npix + (int64_t)r * Wo + u] : 0.f;
    }
    __syncthreads();
    float d[kTcTW];
#pragma unroll
    for (int p = 0; p < kTcTW; ++p) d[p] = dl[tid][p];
#pragma unroll
    for (int vi = 0; vi < kTcDwViews; ++vi) {
      if (v0 + vi >= N) continue;  // uniform
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        float x[kTcDwPitch];
#pragma unroll
        for (int q = 0; q < kTcDwPitch / 4; ++q) {
          const f32x4a_t t = *reinterpret_cast<const f32x4a_t*>(&xs[vi][rr + kh][4 * q]);  // a broadcast
          x[4 * q] = t[0], x[4 * q + 1] = t[1], x[4 * q + 2] = t[2], x[4 * q + 3] = t[3];
        }
#pragma unroll
        for (int p = 0; p < kTcTW; ++p)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) acc[vi][3 * kh + kw] = fmaf(d[p], x[p + kw], acc[vi][3 * kh + kw]);
      }
    }
  }
  const int co = co0 + tid;
  if (co >= a.Cout) return;
  float* out = a.partials + (((int64_t)blk * a.Cout + co) * N + v0) * 9;
#pragma unroll
  for (int vi = 0; vi < kTcDwViews; ++vi) {
    if (v0 + vi >= N) continue;
#pragma unroll
    for (int t = 0; t < 9; ++t) out[vi * 9 + t] = acc[vi][t];
  }
}

// dw[co][v][t] (v < N of the N + 2 input channels) = sum over the tiles, in order, in fp64
__global__ __launch_bounds__(256) void thin_conv1_dw_reduce_kernel(const float* __restrict__ partials, int nblk, int N,
                                                                  int Cout, float* __restrict__ dw) {
  const int per = N * 9;
  const int64_t n = (int64_t)Cout * per;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int k = 0; k < nblk; ++k) s += (double)partials[(int64_t)k * n + i];
  const int64_t co = i / per;
  dw[co * (int64_t)(per + 18) + (i - co * per)] = (float)s;
}

static int tc_check_sizes(int64_t nviews, int64_t B, int64_t Cout, int64_t Ho, int64_t Wo) {
  if (nviews <= 0 || B <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0) return MVBEV_ERR_RANK;
  if (nviews > kWarpMaxViews || Cout % 8 != 0 || Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || Ho * Wo > INT32_MAX / 2 ||
      B > INT32_MAX / (Ho * Wo) || B * Ho * Wo > (int64_t)INT32_MAX / Cout)
    return MVBEV_ERR_SHAPE;  // every tensor below 2^31 elements
  return MVBEV_OK;
}

}  // namespace mvbev

extern "C" {

int mvbev_thin_conv1_forward_f32_ex(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W,
                                    int64_t Ho, int64_t Wo, const float* w1, const float* b1, int64_t Cout, void* y1,
                                    int y1_layout, float* xw, const int32_t* w_mask, void* stream);

int mvbev_thin_conv1_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W, int64_t Ho,
                                 int64_t Wo, const float* w1, const float* b1, int64_t Cout, void* y1, int y1_layout,
                                 float* xw, void* stream) {
  return mvbev_thin_conv1_forward_f32_ex(views, nviews, B, H, W, Ho, Wo, w1, b1, Cout, y1, y1_layout, xw, nullptr,
                                         stream);
}

int mvbev_thin_conv1_weight_mask(const float* w1, int nviews, int64_t Cout, int32_t* mask, void* stream) {
  using namespace mvbev;
  if (!w1 || !mask) return MVBEV_ERR_NULL;
  if (nviews <= 0 || Cout <= 0) return MVBEV_ERR_RANK;
  if (nviews > kWarpMaxViews || Cout > INT32_MAX / (9 * (kWarpMaxViews + 2))) return MVBEV_ERR_SHAPE;
  hipLaunchKernelGGL(thin_conv1_weight_mask_kernel, dim3(1), dim3(1024), 0, as_stream(stream), w1, nviews,
                     Cout * (nviews + 2) * 9, mask);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_thin_conv1_forward_f32_ex(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W,
                                    int64_t Ho, int64_t Wo, const float* w1, const float* b1, int64_t Cout, void* y1,
                                    int y1_layout, float* xw, const int32_t* w_mask, void* stream) {
  using namespace mvbev;
  if (!views || !w1 || !y1) return MVBEV_ERR_NULL;
  if (H <= 0 || W <= 0) return MVBEV_ERR_RANK;
  const int st = tc_check_sizes(nviews, B, Cout, Ho, Wo);
  if (st != MVBEV_OK) return st;
  if (H > INT32_MAX / 2 || W > INT32_MAX / 2 || H * W > INT32_MAX / 2 || B > INT32_MAX / (H * W)) return MVBEV_ERR_SHAPE;
  if (y1_layout != MVBEV_LAYOUT_F32 && y1_layout != MVBEV_LAYOUT_SPLIT_BF16) return MVBEV_ERR_SHAPE;
  if (y1_layout == MVBEV_LAYOUT_SPLIT_BF16 && (reinterpret_cast<uintptr_t>(y1) & 15) != 0) return MVBEV_ERR_ALIGN;
  TcArgs ta = {};
  WarpArgs& a = ta.w;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_warp_view& s = views[i];
    if (!s.src) return MVBEV_ERR_NULL;
    if (s.src_strides[3] != 1 || s.src_strides[0] < 0 || s.src_strides[2] < 0) return MVBEV_ERR_STRIDE;
    WarpView& d = a.v[i];
    unpack_view(s, d, false);  // (sW == 1: checked above)
    d.sC = 0;
  }
  const int64_t tiles_x = ceil_div(Wo, (int64_t)kTcTW), tiles_y = ceil_div(Ho, (int64_t)kTcTH);
  const int64_t cslices = ceil_div(Cout, (int64_t)kTcCoutBlock);
  if (B * tiles_x * tiles_y * cslices > INT32_MAX) return MVBEV_ERR_SHAPE;
  a.nviews = nviews;
  a.B = (int)B; a.C = 1; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)(tiles_x * tiles_y);
  a.nwg = (int)(B * tiles_x * tiles_y * cslices);
  ta.Cout = (int)Cout, ta.cslices = (int)cslices, ta.split = y1_layout == MVBEV_LAYOUT_SPLIT_BF16;
  hipLaunchKernelGGL(thin_conv1_fwd_kernel, dim3((unsigned)a.nwg), dim3(kTcThreads), 0, as_stream(stream), ta, w1, b1, y1,
                     xw, w_mask);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int64_t mvbev_thin_conv1_backward_blocks(int64_t B, int64_t Ho, int64_t Wo) {
  using namespace mvbev;
  if (tc_check_sizes(1, B, 8, Ho, Wo) != MVBEV_OK) return 0;
  return B * ceil_div(Ho, (int64_t)kTcTH) * ceil_div(Wo, (int64_t)kTcTW);
}

int mvbev_thin_conv1_backward_f32(const float* dpre, const float* w1, const float* xw, int nviews, int64_t B,
                                  int64_t Cout, int64_t Ho, int64_t Wo, float* dxw, float* partials, int64_t npartials,
                                  void* stream) {
  using namespace mvbev;
  if (!dpre || (dxw && !w1) || (partials && !xw)) return MVBEV_ERR_NULL;
  const int st = tc_check_sizes(nviews, B, Cout, Ho, Wo);
  if (st != MVBEV_OK) return st;
  TcBwdArgs a = {};
  a.dpre = dpre, a.w1 = w1, a.xw = xw, a.dxw = dxw, a.partials = partials;
  a.N = nviews, a.B = (int)B, a.Cout = (int)Cout, a.Ho = (int)Ho, a.Wo = (int)Wo;
  a.tiles_x = (int)ceil_div(Wo, (int64_t)kTcTW);
  if (partials) {
    const int64_t blocks = B * ceil_div(Ho, (int64_t)kTcTH) * a.tiles_x;
    if (blocks > INT32_MAX || ceil_div(Cout, (int64_t)256) > 65535) return MVBEV_ERR_SHAPE;
    if (npartials < blocks * Cout * nviews * 9) return MVBEV_ERR_SHAPE;
  }
  if (dxw) {
    a.tiles = (int)(a.tiles_x * ceil_div(Ho, (int64_t)kTcDxTH));
    if (B * a.tiles > INT32_MAX) return MVBEV_ERR_SHAPE;
    a.nwg = (int)(B * a.tiles);
    hipLaunchKernelGGL(thin_conv1_dx_kernel, dim3((unsigned)a.nwg), dim3(256), 0, as_stream(stream), a, w1, dxw);
    MVBEV_CHECK_LAUNCH();
  }
  if (partials) {
    a.tiles = (int)(a.tiles_x * ceil_div(Ho, (int64_t)kTcTH));
    a.nwg = (int)(B * a.tiles);
    const dim3 grid((unsigned)a.nwg, (unsigned)ceil_div(Cout, (int64_t)256),
                    (unsigned)ceil_div((int64_t)nviews, (int64_t)kTcDwViews));
    hipLaunchKernelGGL(thin_conv1_dw_kernel, grid, dim3(256), 0, as_stream(stream), a);
    MVBEV_CHECK_LAUNCH();
  }
  return MVBEV_OK;
}

int mvbev_thin_conv1_grad_weight_f32(const float* partials, int64_t nblocks, int nviews, int64_t Cout, float* dw,
                                     void* stream) {
  using namespace mvbev;
  if (!partials || !dw) return MVBEV_ERR_NULL;
  if (nblocks <= 0 || nviews <= 0 || Cout <= 0) return MVBEV_ERR_RANK;
  if (nviews > kWarpMaxViews || Cout % 8 != 0 || nblocks > INT32_MAX || Cout * nviews * 9 > INT32_MAX / 2 ||
      nblocks > INT64_MAX / (Cout * nviews * 9))
    return MVBEV_ERR_SHAPE;
  const int64_t n = Cout * nviews * 9;
  hipLaunchKernelGGL(thin_conv1_dw_reduce_kernel, dim3((unsigned)ceil_div(n, (int64_t)256)), dim3(256), 0,
                     as_stream(stream), partials, (int)nblocks, nviews, (int)Cout, dw);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

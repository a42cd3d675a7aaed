// The per-view image head after its first 1x1 conv, for gfx950 (persp_trans_detector.py:65-66 with the
// first conv moved in front of the upsample, detector.py):
//   out = conv1x1(relu(F.interpolate(g, (Hu, Wu), mode="bilinear")), W)      -> img_head_fwd_kernel
// and its backward from g alone (the upsampled pre-activation is recomputed, never stored):
//   grad_g = U^T(mask * (W^T grad_out)),  grad_W = sum grad_out * relu(pre)  -> img_head_bwd_kernel
//                                                                               + img_head_wgrad_kernel
//
// One launch covers every view and the whole batch (the mvbev_loss_item idiom: a by-value pack of at
// most kIhMaxViews items, workgroups numbered through the views).  Both kernels stage the box of g
// their tile taps in LDS, channel-innermost, with a pixel pitch of cc + 4 floats: lanes on adjacent
// pixels read their float4 of channels from different banks.  Channels go through the box in chunks
// of cc (a multiple of 4 the host picks so that the box fits), so any Cm <= 256 and any ratio >= 1
// fit.  Nothing here uses float atomics: every sum has a fixed order, so results repeat bitwise.
#include "common.h"
#include "warp_common.h"

namespace mvbev {

constexpr int kIhMaxViews = 16;
constexpr int kIhMaxCm = 256;
constexpr int kIhMaxCo = 4;
constexpr int kIhThreads = 256;
constexpr int kIhTH = 8;    // forward: output tile, one lane per output pixel (a wave is 2 rows of 32)
constexpr int kIhTW = 32;
constexpr int kIhSH = 4;    // backward: tile of backbone pixels (gather form)
constexpr int kIhSW = 16;
constexpr int kIhPad = 4;   // floats added to the box's pixel pitch (keeps float4 alignment)
constexpr int kIhBoxBytes = 40 * 1024;

struct IhFwdItem {
  const float* g;
  int64_t gs[4];
  float* out;
  int64_t os[4];
};
struct IhFwdArgs {
  IhFwdItem it[kIhMaxViews];
  int32_t B, Cm, h, w, Hu, Wu, tiles_x, tiles_y, brows, bcols, cc;
  float sy, sx;
};

struct IhBwdItem {
  const float* g;
  int64_t gs[4];
  const float* go;
  int64_t gos[4];
  float* gg;  // may be null: no grad_g wanted for this view
  int64_t ggs[4];
};
struct IhBwdArgs {
  IhBwdItem it[kIhMaxViews];
  int32_t B, Cm, h, w, Hu, Wu, tiles_x, tiles_y, cc, nwg;
  float sy, sx;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The upsampled pre-activation from its four taps, with the roundings of torch's GPU upsample
// (UpSampleBilinear2d.cu): h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d) as the device compiler fuses it
// there, written out with fmaf so that no compiler choice can move a rounding.  torch has two kernels and
// they round the top row differently: the NCHW kernel forms fma(w0, a, w1 * b), the channels-last kernel
// (ih_torch_nhwc below says when torch takes it) fma(w1, b, w0 * a).  Every tap is multiplied, zero weights
// included (0 * inf and 0 * NaN give NaN, as the reference's upsample does).
__device__ __forceinline__ float up_pre(bool nhwc, float a, float b, float c, float d, float l0y, float l1y,
                                        float l0x, float l1x) {
#pragma clang fp contract(off)
  const float top = nhwc ? fmaf(l1x, b, l0x * a) : fmaf(l0x, a, l1x * b);
  const float bottom = fmaf(l0x, c, l1x * d);
  return fmaf(l0y, top, l1y * bottom);
}

// Whether F.interpolate runs its channels-last kernel on a g of these strides: a dense channels-last
// tensor of at least 16 channels (anything else goes through the NCHW kernel's arithmetic).
__device__ __forceinline__ bool ih_torch_nhwc(const int64_t (&gs)[4], int B, int Cm, int h, int w) {
  return Cm >= 16 && h * w > 1 && gs[1] == 1 && gs[3] == Cm && gs[2] == (int64_t)w * Cm &&
         (B == 1 || gs[0] == (int64_t)h * w * Cm);
}

// The bilinear taps of upsampled index X as torch's GPU upsample computes them (UpSampleBilinear2d.cu:
// area_pixel_compute_source_index, whose scale * (X + 0.5) - 0.5 the device compiler fuses into one
// multiply-add), not warp_common.h's up_taps (the CPU kernel's two roundings): together with up_pre above
// the pre-activation has the bits of F.interpolate on this GPU, so the ReLU falls as it did in the
// torch ops this kernel replaces and as the mask tests replay from F.interpolate.
__device__ inline UpTaps ih_taps(int X, float scale, int n) {
#pragma clang fp contract(off)
  UpTaps t;
  float s = fmaf(scale, (float)X + 0.5f, -0.5f);
  s = s < 0.f ? 0.f : s;
  t.i0 = min((int)s, n - 1);
  t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
  t.l1 = s - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// Stages channels [c0, c0 + cc) of the brows x bcols box of g whose first pixel is (ry0, rx0) into
// box[(ry * bcols + rx) * pitch + c].  Box pixels past the map repeat its border pixel (always a valid
// read; the taps never reach them), channels >= Cm are zeros.  gp already points at the batch item.
__device__ inline void ih_stage_box(float* __restrict__ box, const float* __restrict__ gp, const int64_t (&gs)[4],
                                    int c0, int cc, int Cm, int ry0, int rx0, int brows, int bcols, int h, int w) {
  const int tid = threadIdx.x, pitch = cc + kIhPad, npx = brows * bcols;
  const bool chan_inner = gs[1] < gs[3];  // channels-last (or a slice of it): channels are the close axis
  const bool vec = gs[1] == 1 && ((gs[0] | gs[2] | gs[3] | Cm) & 3) == 0 && (reinterpret_cast<uintptr_t>(gp) & 15) == 0;
  if (vec) {
    const int q = cc >> 2;
    for (int i = tid; i < npx * q; i += kIhThreads) {
      const int px = i / q, c = (i - px * q) * 4;
      const int ry = px / bcols, rx = px - ry * bcols;
      const int yy = min(max(ry0 + ry, 0), h - 1), xx = min(max(rx0 + rx, 0), w - 1);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + c < Cm) v = ld4(gp + yy * gs[2] + xx * gs[3] + (c0 + c));
      *reinterpret_cast<float4*>(box + px * pitch + c) = v;
    }
  } else if (chan_inner) {
    for (int i = tid; i < npx * cc; i += kIhThreads) {
      const int px = i / cc, c = i - px * cc;
      const int ry = px / bcols, rx = px - ry * bcols;
      const int yy = min(max(ry0 + ry, 0), h - 1), xx = min(max(rx0 + rx, 0), w - 1);
      box[px * pitch + c] = c0 + c < Cm ? gp[(c0 + c) * gs[1] + yy * gs[2] + xx * gs[3]] : 0.f;
    }
  } else {
    for (int i = tid; i < npx * cc; i += kIhThreads) {
      const int c = i / npx, px = i - c * npx;
      const int ry = px / bcols, rx = px - ry * bcols;
      const int yy = min(max(ry0 + ry, 0), h - 1), xx = min(max(rx0 + rx, 0), w - 1);
      box[px * pitch + c] = c0 + c < Cm ? gp[(c0 + c) * gs[1] + yy * gs[2] + xx * gs[3]] : 0.f;
    }
  }
}

// One workgroup per (view, b, 8 x 32 output tile), one lane per output pixel, all CO outputs.  W sits
// in LDS padded with zeros to a multiple of 4 channels and is read at a wave-uniform address.
template <int CO>
__global__ __launch_bounds__(kIhThreads) void img_head_fwd_kernel(IhFwdArgs a, const float* __restrict__ W) {
  extern __shared__ __attribute__((aligned(16))) float ih_lds[];
  const int tid = threadIdx.x;
  const int Cm = a.Cm, Cmp = (Cm + 3) & ~3, cc = a.cc, pitch = cc + kIhPad;
  float* wl = ih_lds;             // [CO][Cmp]
  float* box = ih_lds + CO * Cmp;  // [brows * bcols][pitch]
  int bid = blockIdx.x;
  const int tile_x = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int tile_y = bid % a.tiles_y;
  bid /= a.tiles_y;
  const int b = bid % a.B, v = bid / a.B;
  const IhFwdItem& it = a.it[v];
  for (int i = tid; i < CO * Cmp; i += kIhThreads) {
    const int o = i / Cmp, c = i - o * Cmp;
    wl[i] = c < Cm ? W[o * Cm + c] : 0.f;
  }
  const int Y0 = tile_y * kIhTH, X0 = tile_x * kIhTW;
  const int Y = Y0 + (tid >> 5), X = X0 + (tid & 31);
  const int by0 = ih_taps(Y0, a.sy, a.h).i0, bx0 = ih_taps(X0, a.sx, a.w).i0;
  // lanes past the image take the last pixel's taps (valid addresses) and store nothing
  const UpTaps ty = ih_taps(min(Y, a.Hu - 1), a.sy, a.h), tx = ih_taps(min(X, a.Wu - 1), a.sx, a.w);
  const int p00 = ((ty.i0 - by0) * a.bcols + (tx.i0 - bx0)) * pitch;
  const int p01 = ((ty.i0 - by0) * a.bcols + (tx.i1 - bx0)) * pitch;
  const int p10 = ((ty.i1 - by0) * a.bcols + (tx.i0 - bx0)) * pitch;
  const int p11 = ((ty.i1 - by0) * a.bcols + (tx.i1 - bx0)) * pitch;
  const float* gp = it.g + b * it.gs[0];
  const bool nhwc = ih_torch_nhwc(it.gs, a.B, Cm, a.h, a.w);
  float acc[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) acc[o] = 0.f;
  for (int c0 = 0; c0 < Cmp; c0 += cc) {
    const int n = min(cc, Cmp - c0);
    __syncthreads();  // the previous chunk is consumed
    ih_stage_box(box, gp, it.gs, c0, cc, Cm, by0, bx0, a.brows, a.bcols, a.h, a.w);
    __syncthreads();
    for (int c = 0; c < n; c += 4) {
      const float4 A = ld4(box + p00 + c), Bq = ld4(box + p01 + c), Cq = ld4(box + p10 + c), D = ld4(box + p11 + c);
      float r[4];
      r[0] = relu_nan(up_pre(nhwc, A.x, Bq.x, Cq.x, D.x, ty.l0, ty.l1, tx.l0, tx.l1));
      r[1] = relu_nan(up_pre(nhwc, A.y, Bq.y, Cq.y, D.y, ty.l0, ty.l1, tx.l0, tx.l1));
      r[2] = relu_nan(up_pre(nhwc, A.z, Bq.z, Cq.z, D.z, ty.l0, ty.l1, tx.l0, tx.l1));
      r[3] = relu_nan(up_pre(nhwc, A.w, Bq.w, Cq.w, D.w, ty.l0, ty.l1, tx.l0, tx.l1));
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        const float4 wv = ld4(wl + o * Cmp + c0 + c);
        acc[o] = fmaf(wv.x, r[0], acc[o]);
        acc[o] = fmaf(wv.y, r[1], acc[o]);
        acc[o] = fmaf(wv.z, r[2], acc[o]);
        acc[o] = fmaf(wv.w, r[3], acc[o]);
      }
    }
  }
  if (Y < a.Hu && X < a.Wu) {
    float* op = it.out + b * it.os[0] + Y * it.os[2] + X * it.os[3];
#pragma unroll
    for (int o = 0; o < CO; ++o) op[o * it.os[1]] = acc[o];
  }
}

// The upsampled indices whose taps reach backbone index y along an axis of n -> N pixels: [lo, hi],
// empty when lo > hi.  i0 and i1 never decrease with the upsampled index, so the set {Y: i0(Y) == y or
// i1(Y) == y} is the run from the first Y with i1(Y) >= y to the last with i0(Y) <= y; both ends are
// found with the tap rule itself from an estimate (nothing assumes the ratio).
__device__ inline void ih_reach(int y, float scale, int n, int N, int& lo, int& hi) {
  // (source coordinates are clamped at 0, so rows 0 and 1 are reached from the first upsampled row on)
  int e = y <= 1 ? 0 : (int)floorf(((float)y - 0.5f) / scale - 0.5f);
  e = min(max(e, 0), N - 1);
  while (e > 0 && ih_taps(e - 1, scale, n).i1 >= y) --e;
  while (e < N && ih_taps(e, scale, n).i1 < y) ++e;
  lo = e;
  e = (int)floorf(((float)y + 1.5f) / scale - 0.5f);
  e = min(max(e, 0), N - 1);
  while (e < N - 1 && ih_taps(e + 1, scale, n).i0 <= y) ++e;
  while (e >= 0 && ih_taps(e, scale, n).i0 > y) --e;
  hi = e;
}

// One workgroup per (view with a grad_out, b, 4 x 16 tile of backbone pixels).  A thread owns four
// channels (c4 = tid % (cc / 4)) of the backbone pixels px = slot, slot + slots, ... of the tile and
// gathers, in a fixed order, every output pixel whose taps reach its pixel: pre is recomputed from
// the staged box (the tile plus a ring of one pixel), d = mask * (W^T grad_out), grad_g += wy wx d
// (both taps count where a clamped border makes i1 == i0).  An output pixel's term of grad_W is added
// by the thread whose pixel is the output's (i0y, i0x) tap, once; the threads' sums are added over the
// slots in order and written as column blockIdx.x of partials[Co * Cm][nwg].
template <int CO>
__global__ __launch_bounds__(kIhThreads) void img_head_bwd_kernel(IhBwdArgs a, const float* __restrict__ W,
                                                                  float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float ih_lds[];
  float* box = ih_lds;
  const int tid = threadIdx.x;
  const int Cm = a.Cm, Cmp = (Cm + 3) & ~3, cc = a.cc, pitch = cc + kIhPad;
  constexpr int brows = kIhSH + 2, bcols = kIhSW + 2;
  int bid = blockIdx.x;
  const int tile_x = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int tile_y = bid % a.tiles_y;
  bid /= a.tiles_y;
  const int b = bid % a.B, v = bid / a.B;
  const IhBwdItem& it = a.it[v];
  const int y0 = tile_y * kIhSH, x0 = tile_x * kIhSW;
  const float* gp = it.g + b * it.gs[0];
  const float* gop = it.go + b * it.gos[0];
  const bool nhwc = ih_torch_nhwc(it.gs, a.B, Cm, a.h, a.w);
  const int q = cc >> 2, slots = kIhThreads / q;
  const int c4 = tid % q, slot = tid / q;
  const bool active = slot < slots;
  const bool gg_vec = it.gg && it.ggs[1] == 1 && ((it.ggs[0] | it.ggs[2] | it.ggs[3] | Cm) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(it.gg) & 15) == 0;

  for (int c0 = 0; c0 < Cmp; c0 += cc) {
    __syncthreads();  // the previous chunk's box / sums are consumed
    ih_stage_box(box, gp, it.gs, c0, cc, Cm, y0 - 1, x0 - 1, brows, bcols, a.h, a.w);
    __syncthreads();
    const int cb = c0 + 4 * c4;  // this thread's first channel
    const bool chan_ok = active && cb < Cmp;
    float wr[CO][4], gw[CO][4];
#pragma unroll
    for (int o = 0; o < CO; ++o)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wr[o][j] = chan_ok && cb + j < Cm ? W[o * Cm + cb + j] : 0.f;
        gw[o][j] = 0.f;
      }
    if (chan_ok) {
      for (int px = slot; px < kIhSH * kIhSW; px += slots) {
        const int y = y0 + px / kIhSW, x = x0 + px % kIhSW;
        if (y >= a.h || x >= a.w) continue;
        int Ylo, Yhi, Xlo, Xhi;
        ih_reach(y, a.sy, a.h, a.Hu, Ylo, Yhi);
        ih_reach(x, a.sx, a.w, a.Wu, Xlo, Xhi);
        if (Xlo > Xhi) Yhi = Ylo - 1;  // no output pixel reaches this one (never for Hu >= h, Wu >= w): no loads
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int Y = Ylo; Y <= Yhi; ++Y) {
          const UpTaps ty = ih_taps(Y, a.sy, a.h);
          const float wy = (ty.i0 == y ? ty.l0 : 0.f) + (ty.i1 == y ? ty.l1 : 0.f);
          const float* r0 = box + (ty.i0 - (y0 - 1)) * bcols * pitch + 4 * c4;
          const float* r1 = box + (ty.i1 - (y0 - 1)) * bcols * pitch + 4 * c4;
          // grad_out of the next output pixel is loaded one iteration ahead of its use
          const float* gor = gop + Y * it.gos[2];
          float gon[CO];
#pragma unroll
          for (int o = 0; o < CO; ++o) gon[o] = gor[o * it.gos[1] + min(Xlo, Xhi) * it.gos[3]];
          for (int X = Xlo; X <= Xhi; ++X) {
            float go[CO];
            const int64_t xn = min(X + 1, Xhi) * it.gos[3];
#pragma unroll
            for (int o = 0; o < CO; ++o) {
              go[o] = gon[o];
              gon[o] = gor[o * it.gos[1] + xn];
            }
            const UpTaps tx = ih_taps(X, a.sx, a.w);
            const float wgt = wy * ((tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f));
            const int o0 = (tx.i0 - (x0 - 1)) * pitch, o1 = (tx.i1 - (x0 - 1)) * pitch;
            const float4 A = ld4(r0 + o0), Bq = ld4(r0 + o1), Cq = ld4(r1 + o0), D = ld4(r1 + o1);
            float pre[4];
            pre[0] = up_pre(nhwc, A.x, Bq.x, Cq.x, D.x, ty.l0, ty.l1, tx.l0, tx.l1);
            pre[1] = up_pre(nhwc, A.y, Bq.y, Cq.y, D.y, ty.l0, ty.l1, tx.l0, tx.l1);
            pre[2] = up_pre(nhwc, A.z, Bq.z, Cq.z, D.z, ty.l0, ty.l1, tx.l0, tx.l1);
            pre[3] = up_pre(nhwc, A.w, Bq.w, Cq.w, D.w, ty.l0, ty.l1, tx.l0, tx.l1);
            const bool own = partials && ty.i0 == y && tx.i0 == x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float t = 0.f;
#pragma unroll
              for (int o = 0; o < CO; ++o) t = fmaf(wr[o][j], go[o], t);
              // threshold_backward's mask: the gradient passes where pre is NaN
              const float d = pre[j] <= 0.f ? 0.f : t;
              acc[j] = fmaf(wgt, d, acc[j]);
              if (own) {
                const float r = relu_nan(pre[j]);
#pragma unroll
                for (int o = 0; o < CO; ++o) gw[o][j] = fmaf(go[o], r, gw[o][j]);
              }
            }
          }
        }
        if (it.gg) {
          float* dp = it.gg + b * it.ggs[0] + y * it.ggs[2] + x * it.ggs[3];
          if (gg_vec) {
            *reinterpret_cast<float4*>(dp + cb) = make_float4(acc[0], acc[1], acc[2], acc[3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (cb + j < Cm) dp[(cb + j) * it.ggs[1]] = acc[j];
          }
        }
      }
    }
    if (partials) {
      // the threads' grad_W sums: red[slot][o][cc], then the slots in order
      __syncthreads();
      float* red = ih_lds;
      if (active) {
#pragma unroll
        for (int o = 0; o < CO; ++o)
#pragma unroll
          for (int j = 0; j < 4; ++j) red[(slot * CO + o) * cc + 4 * c4 + j] = gw[o][j];
      }
      __syncthreads();
      for (int i = tid; i < CO * cc; i += kIhThreads) {
        const int o = i / cc, c = i - o * cc;
        if (c0 + c >= Cm) continue;
        float s = 0.f;
        for (int sl = 0; sl < slots; ++sl) s += red[(sl * CO + o) * cc + c];
        partials[(int64_t)(o * Cm + c0 + c) * a.nwg + blockIdx.x] = s;
      }
    }
  }
}

// grad_W[row] = the sum of row `row` of partials[rows][nwg]: thread t takes columns t, t + 256, ... in
// order in fp64, then a fixed tree over the workgroup.
__global__ __launch_bounds__(kIhThreads) void img_head_wgrad_kernel(const float* __restrict__ partials, int nwg,
                                                                    float* __restrict__ grad_w) {
  __shared__ double red[kIhThreads];
  const int tid = threadIdx.x;
  const float* row = partials + (int64_t)blockIdx.x * nwg;
  double s = 0;
  for (int i = tid; i < nwg; i += kIhThreads) s += (double)row[i];
  red[tid] = s;
  __syncthreads();
  for (int off = kIhThreads / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) grad_w[blockIdx.x] = (float)red[0];
}

static int ih_check_dims(int n, int64_t B, int64_t Cm, int64_t h, int64_t w, int64_t Co, int64_t Hu, int64_t Wu) {
  if (n <= 0 || B <= 0 || Cm <= 0 || h <= 0 || w <= 0 || Co <= 0 || Hu <= 0 || Wu <= 0) return MVBEV_ERR_RANK;
  if (n > kIhMaxViews || Cm > kIhMaxCm || Co > kIhMaxCo || Hu < h || Wu < w) return MVBEV_ERR_SHAPE;
  if (B * Cm * h * w > INT32_MAX || B * Co * Hu * Wu > INT32_MAX) return MVBEV_ERR_SHAPE;
  return MVBEV_OK;
}

// the largest channel chunk (a multiple of 4, at most Cm rounded up) whose box of npx pixels fits
static int ih_chunk(int64_t Cm, int64_t npx) {
  const int64_t Cmp = round_up(Cm, 4);
  int64_t cc = kIhBoxBytes / (int64_t)sizeof(float) / npx - kIhPad;
  cc = std::min(Cmp, cc & ~(int64_t)3);
  return (int)std::max<int64_t>(cc, 4);
}

// rows (columns) of g that the taps of T adjacent upsampled rows span at most: their source
// coordinates lie within (T - 1) * scale of each other, so i0 takes at most floor((T - 1) * scale) + 2
// values and i1 adds one more
static int ih_box_extent(int T, float scale, int64_t n) {
  return (int)std::min<int64_t>(n, (int64_t)((float)(T - 1) * scale + 1e-3f) + 3);
}

static int64_t ih_bwd_tiles(int64_t B, int64_t h, int64_t w) {
  return B * ceil_div(h, (int64_t)kIhSH) * ceil_div(w, (int64_t)kIhSW);
}

static int ih_active_views(const mvbev_img_head_item* items, int n) {
  int k = 0;
  for (int i = 0; i < n; ++i) k += items[i].grad_out != nullptr;
  return k;
}

}  // namespace mvbev

extern "C" {

int mvbev_img_head_forward_f32(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h, int64_t w,
                               int64_t Co, int64_t Hu, int64_t Wu, const float* weight, void* stream) {
  using namespace mvbev;
  if (!items || !weight) return MVBEV_ERR_NULL;
  const int st = ih_check_dims(n, B, Cm, h, w, Co, Hu, Wu);
  if (st != MVBEV_OK) return st;
  IhFwdArgs a = {};
  for (int i = 0; i < n; ++i) {
    if (!items[i].g || !items[i].out) return MVBEV_ERR_NULL;
    a.it[i].g = items[i].g, a.it[i].out = items[i].out;
    for (int d = 0; d < 4; ++d) {
      if (items[i].g_strides[d] < 0 || items[i].out_strides[d] < 0) return MVBEV_ERR_STRIDE;
      a.it[i].gs[d] = items[i].g_strides[d], a.it[i].os[d] = items[i].out_strides[d];
    }
  }
  a.B = (int32_t)B, a.Cm = (int32_t)Cm, a.h = (int32_t)h, a.w = (int32_t)w, a.Hu = (int32_t)Hu, a.Wu = (int32_t)Wu;
  a.sy = (float)h / (float)Hu;  // area_pixel_compute_scale(align_corners=false), as warp_up_kernel
  a.sx = (float)w / (float)Wu;
  a.tiles_x = (int32_t)ceil_div(Wu, (int64_t)kIhTW);
  a.tiles_y = (int32_t)ceil_div(Hu, (int64_t)kIhTH);
  a.brows = ih_box_extent(kIhTH, a.sy, h);
  a.bcols = ih_box_extent(kIhTW, a.sx, w);
  a.cc = ih_chunk(Cm, (int64_t)a.brows * a.bcols);
  const int64_t blocks = (int64_t)n * B * a.tiles_x * a.tiles_y;
  if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  const size_t lds = ((size_t)Co * round_up(Cm, 4) + (size_t)a.brows * a.bcols * (a.cc + kIhPad)) * sizeof(float);
  const dim3 grid((unsigned)blocks), block(kIhThreads);
  hipStream_t s = as_stream(stream);
  switch (Co) {
    case 1: hipLaunchKernelGGL(img_head_fwd_kernel<1>, grid, block, lds, s, a, weight); break;
    case 2: hipLaunchKernelGGL(img_head_fwd_kernel<2>, grid, block, lds, s, a, weight); break;
    case 3: hipLaunchKernelGGL(img_head_fwd_kernel<3>, grid, block, lds, s, a, weight); break;
    default: hipLaunchKernelGGL(img_head_fwd_kernel<4>, grid, block, lds, s, a, weight); break;
  }
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int64_t mvbev_img_head_backward_blocks(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h,
                                       int64_t w, int64_t Co, int64_t Hu, int64_t Wu) {
  using namespace mvbev;
  if (!items || ih_check_dims(n, B, Cm, h, w, Co, Hu, Wu) != MVBEV_OK) return 0;
  const int64_t blocks = ih_active_views(items, n) * ih_bwd_tiles(B, h, w);
  return blocks <= INT32_MAX ? blocks : 0;
}

int mvbev_img_head_backward_f32(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h, int64_t w,
                                int64_t Co, int64_t Hu, int64_t Wu, const float* weight, float* partials,
                                int64_t npartials, void* stream) {
  using namespace mvbev;
  if (!items || !weight) return MVBEV_ERR_NULL;
  const int st = ih_check_dims(n, B, Cm, h, w, Co, Hu, Wu);
  if (st != MVBEV_OK) return st;
  IhBwdArgs a = {};
  int k = 0;
  bool any_gg = false;
  for (int i = 0; i < n; ++i) {
    const mvbev_img_head_item& src = items[i];
    if (!src.grad_out) continue;  // this view's output took no part in the loss
    if (!src.g) return MVBEV_ERR_NULL;
    IhBwdItem& it = a.it[k++];
    it.g = src.g, it.go = src.grad_out, it.gg = src.grad_g;
    any_gg = any_gg || src.grad_g;
    for (int d = 0; d < 4; ++d) {
      if (src.g_strides[d] < 0 || src.grad_out_strides[d] < 0 || (src.grad_g && src.grad_g_strides[d] < 0))
        return MVBEV_ERR_STRIDE;
      it.gs[d] = src.g_strides[d], it.gos[d] = src.grad_out_strides[d], it.ggs[d] = src.grad_g_strides[d];
    }
  }
  if (k == 0 || (!any_gg && !partials)) return MVBEV_OK;  // nothing is wanted
  const int64_t blocks = k * ih_bwd_tiles(B, h, w);
  if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  if (partials && npartials < Co * Cm * blocks) return MVBEV_ERR_SHAPE;
  a.B = (int32_t)B, a.Cm = (int32_t)Cm, a.h = (int32_t)h, a.w = (int32_t)w, a.Hu = (int32_t)Hu, a.Wu = (int32_t)Wu;
  a.sy = (float)h / (float)Hu;
  a.sx = (float)w / (float)Wu;
  a.tiles_x = (int32_t)ceil_div(w, (int64_t)kIhSW);
  a.tiles_y = (int32_t)ceil_div(h, (int64_t)kIhSH);
  constexpr int npx = (kIhSH + 2) * (kIhSW + 2);
  a.cc = ih_chunk(Cm, npx);
  a.nwg = (int32_t)blocks;
  // the box, reused for the threads' grad_W sums: (256 / (cc / 4)) slots x Co x cc floats
  const size_t box = (size_t)npx * (a.cc + kIhPad) * sizeof(float);
  const size_t red = (size_t)(kIhThreads / (a.cc / 4)) * Co * a.cc * sizeof(float);
  const size_t lds = std::max(box, red);
  const dim3 grid((unsigned)blocks), block(kIhThreads);
  hipStream_t s = as_stream(stream);
  switch (Co) {
    case 1: hipLaunchKernelGGL(img_head_bwd_kernel<1>, grid, block, lds, s, a, weight, partials); break;
    case 2: hipLaunchKernelGGL(img_head_bwd_kernel<2>, grid, block, lds, s, a, weight, partials); break;
    case 3: hipLaunchKernelGGL(img_head_bwd_kernel<3>, grid, block, lds, s, a, weight, partials); break;
    default: hipLaunchKernelGGL(img_head_bwd_kernel<4>, grid, block, lds, s, a, weight, partials); break;
  }
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_img_head_grad_weight_f32(const float* partials, int64_t nblocks, int64_t Cm, int64_t Co, float* grad_w,
                                   void* stream) {
  using namespace mvbev;
  if (!partials || !grad_w) return MVBEV_ERR_NULL;
  if (nblocks <= 0 || Cm <= 0 || Co <= 0) return MVBEV_ERR_RANK;
  if (Cm > kIhMaxCm || Co > kIhMaxCo || nblocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  hipLaunchKernelGGL(img_head_wgrad_kernel, dim3((unsigned)(Co * Cm)), dim3(kIhThreads), 0, as_stream(stream),
                     partials, (int)nblocks, grad_w);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

// The front and the closing upsample of the reference's ImageProjVariant ("early fusion",
// multiview_detector/models/image_proj_variant.py) for gfx950.
//
// img_proj_kernel replaces, in ONE launch, the camera loop of :64-86 and the cat of :88:
//   F.interpolate(imgs[:, cam], upsample_shape, 'bilinear')            (:67, a DOWNsample in the Wildtrack set-up)
//   kornia.warp_perspective(img_res, proj_mat, reducedgrid_shape)      (:69)
//   torch.cat(projected_imgs + [coord_map.repeat(B)], dim=1)           (:88)
// Per grid pixel and view the kornia sample coordinates (warp_coord: the one contraction-free definition of
// warp_common.h; non-finite coordinates give NaN, coordinates outside the resized image give 0) pick up to four
// corners of the RESIZED image; each in-bounds corner is evaluated from the full-resolution image with PyTorch's
// align_corners=False taps (up_taps: scale * (dst + 0.5) - 0.5 clamped at 0, the second tap clamped at the edge,
// the product rounded before the subtraction) in PyTorch's order l0y (l0x a + l1x b) + l1y (l0x c + l1x d); the
// four corner values are blended as warp_tile_kernel blends them (invalid corners selected to 0, not multiplied).
// At most 16 taps per sample and channel; the resized images are never written.  The two coord channels
// (coord_value: mvbev_fill_coord_map_f32's values) are written by the same launch.  The output is addressed by
// element strides, so NCHW and channels-last outputs hold bitwise-equal values.
//
// A latency-bound gather (config 2: 302 k (pixel, view) items, 4 MB written): two thread mappings are built, one
// thread per (pixel, view) over 16 x 16 tiles of one view, and one thread per pixel that walks the views
// (MVBEV_IMG_PROJ_PER_PIXEL); tools/img_proj_bench.py measures both.
//
// upsample_map_kernel / upsample_map_bwd_kernel: the closing F.interpolate(map, reducedgrid_shape, 'bilinear')
// of :92 (a real ~8x upsample here) on a one-channel map, and its adjoint as a fixed-order gather: one wave per
// low-resolution pixel sums the output pixels whose taps touch it (lane-strided partial sums, then a shuffle
// tree: the same order every run, no float atomics).
#include "warp_common.h"

namespace mvbev {

constexpr int kIpTile = 16;  // the block's square tile: 256 threads, a wave = 4 rows x 16 columns

struct IpView {
  const float* src;
  int64_t sB, sC, sH;  // element strides (column stride 1)
  float m[9];
};

struct IpArgs {
  IpView v[kWarpMaxViews];
  int nviews, B, H, W, Hr, Wr, Ho, Wo, tiles_x, tiles;
  float sy, sx;  // H / Hr, W / Wr (fp32 quotients: PyTorch's area_pixel_compute_scale)
  int64_t oB, oC, oH, oW;
};

// the three channels of view vw at grid pixel (u, v) of batch item b
__device__ __forceinline__ void ip_sample(const IpArgs& a, const IpView& vw, int b, int u, int v, float (&r)[3]) {
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = vw.m[k];
  const WarpCoord wc = warp_coord(m, u, v, a.Ho, a.Wo, a.Hr, a.Wr);
  if (!wc.inside) {
    const float fill = wc.finite ? 0.f : __builtin_nanf("");
    r[0] = r[1] = r[2] = fill;
    return;
  }
  const float ix = wc.ix, iy = wc.iy;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  const float w_nw = (fx1 - ix) * (fy1 - iy), w_ne = (ix - fx0) * (fy1 - iy);
  const float w_sw = (fx1 - ix) * (iy - fy0), w_se = (ix - fx0) * (iy - fy0);
  const bool vx0 = x0 >= 0, vx1 = x0 + 1 <= a.Wr - 1, vy0 = y0 >= 0, vy1 = y0 + 1 <= a.Hr - 1;
  // an invalid corner evaluates a safe in-bounds pixel of the resized image and is replaced by 0
  UpTaps tx[2], ty[2];
  tx[0] = up_taps(max(x0, 0), a.sx, a.W);
  tx[1] = up_taps(min(x0 + 1, a.Wr - 1), a.sx, a.W);
  ty[0] = up_taps(max(y0, 0), a.sy, a.H);
  ty[1] = up_taps(min(y0 + 1, a.Hr - 1), a.sy, a.H);
  const float* base = vw.src + (int64_t)b * vw.sB;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pc = base + (int64_t)c * vw.sC;
    float rv[2][2];
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
      const float* r0 = pc + (int64_t)ty[ky].i0 * vw.sH;
      const float* r1 = pc + (int64_t)ty[ky].i1 * vw.sH;
#pragma unroll
      for (int kx = 0; kx < 2; ++kx)
        rv[ky][kx] = ty[ky].l0 * (tx[kx].l0 * r0[tx[kx].i0] + tx[kx].l1 * r0[tx[kx].i1]) +
                     ty[ky].l1 * (tx[kx].l0 * r1[tx[kx].i0] + tx[kx].l1 * r1[tx[kx].i1]);
    }
    float acc = 0.f;
    acc += (vx0 && vy0 ? rv[0][0] : 0.f) * w_nw;
    acc += (vx1 && vy0 ? rv[0][1] : 0.f) * w_ne;
    acc += (vx0 && vy1 ? rv[1][0] : 0.f) * w_sw;
    acc += (vx1 && vy1 ? rv[1][1] : 0.f) * w_se;
    r[c] = acc;
  }
}

// PER_PIXEL false: block = (b, view, 16 x 16 tile), view 0's threads also write the coord channels;
// true: block = (b, tile), each thread walks the views
template <bool PER_PIXEL>
__global__ __launch_bounds__(kIpTile* kIpTile) void img_proj_kernel(const IpArgs a, float* __restrict__ out) {
  const int lb = blockIdx.x;
  const int tile = lb % a.tiles;
  const int q = lb / a.tiles;
  const int view = PER_PIXEL ? 0 : q % a.nviews;
  const int b = PER_PIXEL ? q : q / a.nviews;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int v = ty * kIpTile + (int)(threadIdx.x / kIpTile);
  const int u = tx * kIpTile + (int)(threadIdx.x % kIpTile);
  if (v >= a.Ho || u >= a.Wo) return;
  float* o = out + (int64_t)b * a.oB + (int64_t)v * a.oH + (int64_t)u * a.oW;
  if (view == 0) {
    o[(int64_t)(3 * a.nviews) * a.oC] = coord_value(u, a.Wo);
    o[(int64_t)(3 * a.nviews + 1) * a.oC] = coord_value(v, a.Ho);
  }
  if constexpr (PER_PIXEL) {
    for (int k = 0; k < a.nviews; ++k) {
      float r[3];
      ip_sample(a, a.v[k], b, u, v, r);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[(int64_t)(3 * k + c) * a.oC] = r[c];
    }
  } else {
    float r[3];
    ip_sample(a, a.v[view], b, u, v, r);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(int64_t)(3 * view + c) * a.oC] = r[c];
  }
}

__global__ __launch_bounds__(256) void upsample_map_kernel(const float* __restrict__ x, float* __restrict__ y, int B,
                                                           int h, int w, int Ho, int Wo, float sy, float sx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * Ho * Wo) return;
  const int X = (int)(i % Wo), Y = (int)((i / Wo) % Ho), b = (int)(i / ((int64_t)Wo * Ho));
  const UpTaps ty = up_taps(Y, sy, h), tx = up_taps(X, sx, w);
  const float* p = x + (int64_t)b * h * w;
  const float* r0 = p + (int64_t)ty.i0 * w;
  const float* r1 = p + (int64_t)ty.i1 * w;
  y[i] = ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
}

// the output indices X whose taps can touch source index i: their source coordinate scale (X + 0.5) - 0.5 lies in
// (i - 1, i + 1) (clamped coordinates belong to i = 0), one index of margin on both sides for the rounding
__device__ __forceinline__ void up_adjoint_range(int i, float scale, int N, int& lo, int& hi) {
  lo = max(0, (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1);
  hi = min(N - 1, (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1);
}
__device__ __forceinline__ float up_adjoint_weight(const UpTaps& t, int i) {
  return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);  // (the edge: both taps on the last index)
}

__global__ __launch_bounds__(256) void upsample_map_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                               int B, int h, int w, int Ho, int Wo, float sy,
                                                               float sx) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per low-resolution pixel
  const int lane = threadIdx.x & 63;
  if (wid >= (int64_t)B * h * w) return;
  const int x = (int)(wid % w), y = (int)((wid / w) % h), b = (int)(wid / ((int64_t)w * h));
  int ylo, yhi, xlo, xhi;
  up_adjoint_range(y, sy, Ho, ylo, yhi);
  up_adjoint_range(x, sx, Wo, xlo, xhi);
  const int nx = xhi - xlo + 1, n = (yhi - ylo + 1) * nx;
  const float* g = dy + (int64_t)b * Ho * Wo;
  float sum = 0.f;
  for (int k = lane; k < n; k += 64) {
    const int Y = ylo + k / nx, X = xlo + k % nx;
    const float wy = up_adjoint_weight(up_taps(Y, sy, h), y), wx = up_adjoint_weight(up_taps(X, sx, w), x);
    sum += wy * wx * g[(int64_t)Y * Wo + X];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  if (lane == 0) dx[wid] = sum;
}

static int um_check(int64_t B, int64_t h, int64_t w, int64_t Ho, int64_t Wo) {
  if (B <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0) return MVBEV_ERR_RANK;
  if (Ho < h || Wo < w || Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || Ho * Wo > INT32_MAX / 2 ||
      B > INT32_MAX / 2 / (Ho * Wo))
    return MVBEV_ERR_SHAPE;
  return MVBEV_OK;
}

}  // namespace mvbev

extern "C" {

int mvbev_img_proj_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W, int64_t Hr,
                               int64_t Wr, int64_t Ho, int64_t Wo, float* out, const int64_t out_strides[4], int flags,
                               void* stream) {
  using namespace mvbev;
  if (!views || !out || !out_strides) return MVBEV_ERR_NULL;
  if (nviews <= 0 || B <= 0 || H <= 0 || W <= 0 || Hr <= 0 || Wr <= 0 || Ho <= 0 || Wo <= 0) return MVBEV_ERR_RANK;
  if (nviews > kWarpMaxViews || (flags & ~MVBEV_IMG_PROJ_PER_PIXEL)) return MVBEV_ERR_SHAPE;
  const int64_t lim = INT32_MAX / 2;
  if (H > lim || W > lim || H * W > lim || B > lim / (H * W) || Hr > lim || Wr > lim || Hr * Wr > lim || Ho > lim ||
      Wo > lim || Ho * Wo > lim || B * (3 * nviews + 2) > lim / (Ho * Wo))
    return MVBEV_ERR_SHAPE;  // every tensor below 2^31 elements
  for (int k = 0; k < 4; ++k)
    if (out_strides[k] < 0) return MVBEV_ERR_STRIDE;
  IpArgs a = {};
  for (int i = 0; i < nviews; ++i) {
    const mvbev_warp_view& s = views[i];
    if (!s.src) return MVBEV_ERR_NULL;
    if (s.src_strides[3] != 1 || s.src_strides[0] < 0 || s.src_strides[1] < 0 || s.src_strides[2] < 0)
      return MVBEV_ERR_STRIDE;
    IpView& d = a.v[i];
    d.src = static_cast<const float*>(s.src);
    d.sB = s.src_strides[0], d.sC = s.src_strides[1], d.sH = s.src_strides[2];
    for (int k = 0; k < 9; ++k) d.m[k] = s.m[k];
  }
  a.nviews = nviews;
  a.B = (int)B, a.H = (int)H, a.W = (int)W, a.Hr = (int)Hr, a.Wr = (int)Wr, a.Ho = (int)Ho, a.Wo = (int)Wo;
  a.sy = (float)H / (float)Hr, a.sx = (float)W / (float)Wr;
  a.oB = out_strides[0], a.oC = out_strides[1], a.oH = out_strides[2], a.oW = out_strides[3];
  a.tiles_x = (int)ceil_div(Wo, (int64_t)kIpTile);
  a.tiles = (int)(a.tiles_x * ceil_div(Ho, (int64_t)kIpTile));
  const bool per_pixel = (flags & MVBEV_IMG_PROJ_PER_PIXEL) != 0;
  const int64_t nwg = B * a.tiles * (per_pixel ? 1 : nviews);
  if (nwg > INT32_MAX) return MVBEV_ERR_SHAPE;
  if (per_pixel)
    hipLaunchKernelGGL(img_proj_kernel<true>, dim3((unsigned)nwg), dim3(kIpTile * kIpTile), 0, as_stream(stream), a, out);
  else
    hipLaunchKernelGGL(img_proj_kernel<false>, dim3((unsigned)nwg), dim3(kIpTile * kIpTile), 0, as_stream(stream), a, out);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_upsample_map_f32(const float* x, int64_t B, int64_t h, int64_t w, int64_t Ho, int64_t Wo, float* y,
                           void* stream) {
  using namespace mvbev;
  if (!x || !y) return MVBEV_ERR_NULL;
  const int st = um_check(B, h, w, Ho, Wo);
  if (st != MVBEV_OK) return st;
  hipLaunchKernelGGL(upsample_map_kernel, dim3((unsigned)ceil_div(B * Ho * Wo, (int64_t)256)), dim3(256), 0,
                     as_stream(stream), x, y, (int)B, (int)h, (int)w, (int)Ho, (int)Wo, (float)h / (float)Ho,
                     (float)w / (float)Wo);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_upsample_map_backward_f32(const float* dy, int64_t B, int64_t h, int64_t w, int64_t Ho, int64_t Wo,
                                    float* dx, void* stream) {
  using namespace mvbev;
  if (!dy || !dx) return MVBEV_ERR_NULL;
  const int st = um_check(B, h, w, Ho, Wo);
  if (st != MVBEV_OK) return st;
  hipLaunchKernelGGL(upsample_map_bwd_kernel, dim3((unsigned)ceil_div(B * h * w, (int64_t)4)), dim3(256), 0,
                     as_stream(stream), dy, dx, (int)B, (int)h, (int)w, (int)Ho, (int)Wo, (float)h / (float)Ho,
                     (float)w / (float)Wo);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

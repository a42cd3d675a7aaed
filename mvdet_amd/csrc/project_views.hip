// The projection as a standalone op on plain channels-last tensors (mvdet_amd.ProjectViews), gfx950:
//   world = cat([warp(upsample(feat_v)) for v] + [coord_map])          persp_trans_detector.py:65, :69, :77
// forward (project_views_cl_kernel) and its adjoint (project_views_cl_adjoint_kernel), fp32 / fp16 / bf16
// storage, fp32 math.
//
// Channels-last makes both sides lines: a source pixel is C contiguous elements, an output pixel's view
// slice is C contiguous elements at offset v * C of a Ctot-element pixel.  Mapping (both kernels): a block
// is 32 pixels x 8 lanes, a lane owns one 16-B unit of consecutive channels (4 fp32 / 8 16-bit) and steps
// through its pixel's channel chunk 8 units at a time, so the 8 lanes of a pixel touch one 128-B piece of a
// line per access (as warp_wino_cl_kernel).  The sample geometry (warp_coord / up_window, the shared code of
// every warp) is computed once per lane and reused by every unit of the chunk.
//
// Access widths are chosen on the host, never assumed: with the coord channels Ctot = N C + 2, so a pixel
// is only 8-B (fp32) or 4-B (16-bit) aligned.  A unit moves as 16-B, 8-B, 4-B or element accesses — the
// widest that divides the base address, every stride and the view offset v * C in bytes; the last
// C % unit channels go element by element.
#include "project_common.h"

namespace mvbev {
namespace pv {

struct FwdArgs {
  WarpArgs w;     // views (src, strides, matrix), sizes of the warp's source in w.H / w.W, grid, tiling
  int h, sw;      // the views' own height and width (h <= H, sw <= W)
  float sy, sx;   // upsample scales h / H, w / W as PyTorch computes them
  void* out;      // [B][Ho][Wo][Ctot]
  int64_t Ctot;
  int coord;      // write the two coord channels at N * C
  int lw, stw;    // access widths in bytes of the source loads and of the stores
};

// One block: 32 output pixels (4 x 8) of one (batch item, view, channel chunk).  TAPS = 9: the fused
// upsample's 3x3 window (up_window, warp_up_kernel's sum order); TAPS = 4: the bilinear corners (nw, ne, sw,
// se; an out-of-bounds corner contributes 0 * weight, as GridSampler.h).
template <typename T, typename TO, bool UP>
__global__ __launch_bounds__(kThreads) void project_views_cl_kernel(const FwdArgs fa) {
  constexpr int N = Unit<T>::N, TAPS = UP ? 9 : 4;
  const WarpArgs& a = fa.w;
  const WarpBlock wb = warp_block_index(a);
  const WarpView& vw = a.v[wb.view];
  const int pix = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  const int v = wb.k * kTH + pix / kTW, u = wb.tx * kTW + pix % kTW;
  if (v >= a.Ho || u >= a.Wo) return;
  const int H = a.H, W = a.W;
  float m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = vw.m[i];
  bool finite, inside;
  int64_t off[TAPS];
  float wt[UP ? 6 : 4];  // UP: the window's row weights ay[3] then its column weights ax[3]; else the 4 corners'
  if constexpr (UP) {
    const UpWindow uw = up_window(m, u, v, a.Ho, a.Wo, H, W, fa.h, fa.sw, fa.sy, fa.sx);
    finite = uw.finite, inside = uw.inside;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      wt[i] = uw.ay[i], wt[3 + i] = uw.ax[i];
#pragma unroll
      for (int j = 0; j < 3; ++j)  // rows / columns past the map carry weight 0: clamp their address
        off[3 * i + j] = (int64_t)min(uw.rb + i, fa.h - 1) * vw.sH + (int64_t)min(uw.cb + j, fa.sw - 1) * vw.sW;
    }
  } else {
    const WarpCoord wc = warp_coord(m, u, v, a.Ho, a.Wo, H, W);
    finite = wc.finite, inside = wc.inside;
    const float ix = wc.ix, iy = wc.iy;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = inside ? (int)fx0 : 0, y0 = inside ? (int)fy0 : 0;
    const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
    const float cw[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0),
                         (ix - fx0) * (iy - fy0)};
    const bool vx[2] = {x0 >= 0, x0 + 1 <= W - 1}, vy[2] = {y0 >= 0, y0 + 1 <= H - 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cx = min(max(x0 + (k & 1), 0), W - 1), cy = min(max(y0 + (k >> 1), 0), H - 1);
      off[k] = (int64_t)cy * vw.sH + (int64_t)cx * vw.sW;
      wt[k] = cw[k];
    }
    // an out-of-bounds corner: its (clamped, finite-weight) value is replaced by 0 below
    if (!(vx[0] && vy[0])) off[0] = -1;
    if (!(vx[1] && vy[0])) off[1] = -1;
    if (!(vx[0] && vy[1])) off[2] = -1;
    if (!(vx[1] && vy[1])) off[3] = -1;
  }
  const float fill = finite ? 0.f : __builtin_nanf("");
  const T* src = static_cast<const T*>(vw.src) + (int64_t)wb.b * vw.sB;
  TO* out = static_cast<TO*>(fa.out) + (((int64_t)wb.b * a.Ho + v) * a.Wo + u) * fa.Ctot;
  TO* dst = out + (int64_t)wb.view * a.C;
  const int c_begin = wb.chunk * kCPB, c_end = min(a.C, c_begin + kCPB);

  // the sample of N channels from x[tap][], in warp_up_kernel's / the exact warp's order; explicit fmas: contraction
  // is the compiler's choice per call site, and the unit path, the element tail and every instantiation (fp32 and
  // 16-bit maps) must give the same bits
  auto combine = [&](const float (&x)[TAPS][N], float (&r)[N]) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
      float acc = 0.f;
      if constexpr (UP) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float row = 0.f;
#pragma unroll
          for (int j = 0; j < 3; ++j) row = __builtin_fmaf(wt[3 + j], x[3 * i + j][e], row);
          acc = __builtin_fmaf(wt[i], row, acc);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(off[k] >= 0 ? x[k][e] : 0.f, wt[k], acc);
      }
      r[e] = acc;
    }
  };

  for (int c = c_begin + lane * N; c < c_end; c += kLanes * N) {
    float r[N];
    if (c + N <= c_end) {
      if (inside) {
        float x[TAPS][N];
#pragma unroll
        for (int t = 0; t < TAPS; ++t) load_unit<T>(src + (off[t] < 0 ? 0 : off[t]) + c, fa.lw, x[t]);
        combine(x, r);
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) r[e] = fill;
      }
      if constexpr (std::is_same<T, TO>::value) {
        store_unit<TO>(dst + c, fa.stw, r);
      } else {  // 16-bit maps, fp32 out: two 16-B units
        float lo[4], hi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = r[e], hi[e] = r[4 + e];
        store_unit<TO>(dst + c, fa.stw, lo);
        store_unit<TO>(dst + c + 4, fa.stw, hi);
      }
    } else {  // the last C % N channels, element by element
      for (int cc = c; cc < c_end; ++cc) {
        float acc = fill;
        if (inside) {
          float x[TAPS][N] = {};
#pragma unroll
          for (int t = 0; t < TAPS; ++t) x[t][0] = to_f32<T>(src[(off[t] < 0 ? 0 : off[t]) + cc]);
          float rr[N];
          combine(x, rr);
          acc = rr[0];
        }
        dst[cc] = cvt_out<TO>(acc);
      }
    }
  }
  if (fa.coord && wb.view == 0 && wb.chunk == 0 && lane == 0) {  // mvbev_fill_coord_map_f32's values
    TO* cc = out + (int64_t)a.nviews * a.C;
    cc[0] = cvt_out<TO>(coord_value(u, a.Wo));
    cc[1] = cvt_out<TO>(coord_value(v, a.Ho));
  }
}

struct AdjView {
  const int32_t* rp;
  const int32_t* col;
  const float* val;
  void* gs;          // [B][h][w][C]
  int64_t sB, sP;    // batch and pixel strides of gs in elements
  int64_t c_off;     // the view's first channel in a grad_out pixel
};
struct AdjArgs {
  AdjView v[kWarpMaxViews];
  const void* go;    // [B][Ho][Wo][Ctot]
  int64_t Ctot, gB;  // pixel and batch strides of go in elements
  int nviews, B, C, P, pblocks, chunks, nwg;
  int lw, stw;       // access widths in bytes of the grad_out loads and the grad_src stores
};

// grad_src[b][p][c] = sum_e val[e] * grad_out[b][col[e]][c_off + c] over row p of the view's plan, in CSR
// order, one fma per entry: the per-(pixel, channel) sum of warp_adjoint_kernel (the fp32 NCHW gather), in its
// order.  One block: 32 source pixels of one (batch item, view, channel chunk); an empty row stores zeros.
template <typename TG, typename TS>
__global__ __launch_bounds__(kThreads) void project_views_cl_adjoint_kernel(const AdjArgs a) {
  constexpr int N = Unit<TS>::N;  // channels per lane and step: a 16-B unit of grad_src
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int pb = lb % a.pblocks;
  int r = lb / a.pblocks;
  const int chunk = r % a.chunks;
  r /= a.chunks;
  const int view = r % a.nviews, b = r / a.nviews;
  const int p = pb * kPix + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (p >= a.P) return;
  const AdjView& vw = a.v[view];
  const int e0 = vw.rp[p], e1 = vw.rp[p + 1];
  const TG* go = static_cast<const TG*>(a.go) + (int64_t)b * a.gB + vw.c_off;
  TS* gs = static_cast<TS*>(vw.gs) + (int64_t)b * vw.sB + (int64_t)p * vw.sP;
  const int c_begin = chunk * kCPB, c_end = min(a.C, c_begin + kCPB);
  for (int c = c_begin + lane * N; c < c_end; c += kLanes * N) {
    if (c + N <= c_end) {
      float acc[N];
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] = 0.f;
      for (int e = e0; e < e1; ++e) {
        const float w = vw.val[e];
        const TG* g = go + (int64_t)vw.col[e] * a.Ctot + c;
        if constexpr (std::is_same<TG, TS>::value) {
          float x[N];
          load_unit<TG>(g, a.lw, x);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] = __builtin_fmaf(w, x[i], acc[i]);
        } else {  // fp32 grad_out, 16-bit grad_src: two 16-B units
          float x[2][4];
          load_unit<TG>(g, a.lw, x[0]);
          load_unit<TG>(g + 4, a.lw, x[1]);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] = __builtin_fmaf(w, x[i >> 2][i & 3], acc[i]);
        }
      }
      store_unit<TS>(gs + c, a.stw, acc);
    } else {
      for (int cc = c; cc < c_end; ++cc) {
        float acc = 0.f;
        for (int e = e0; e < e1; ++e)
          acc = __builtin_fmaf(vw.val[e], to_f32<TG>(go[(int64_t)vw.col[e] * a.Ctot + cc]), acc);
        gs[cc] = cvt_out<TS>(acc);
      }
    }
  }
}

}  // namespace pv
}  // namespace mvbev

extern "C" int mvbev_project_views_cl_forward(const mvbev_warp_view* views, int nviews, int src_kind, int64_t B,
                                              int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int64_t Ho,
                                              int64_t Wo, void* out, int out_kind, int64_t Ctot, int coord_channels,
                                              void* stream) {
  using namespace mvbev;
  if (!views || !out) return MVBEV_ERR_NULL;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || nviews <= 0)
    return MVBEV_ERR_RANK;
  if (src_kind < 0 || src_kind > 2 || (out_kind != src_kind && out_kind != 0)) return MVBEV_ERR_SHAPE;
  const int64_t tiles_x = ceil_div(Wo, pv::kTW), tiles = tiles_x * ceil_div(Ho, pv::kTH);
  const int64_t chunks = ceil_div(C, pv::kCPB);
  if (nviews > kWarpMaxViews || B * nviews > 65535 || C > INT32_MAX / 2 || H > INT32_MAX / 2 || W > INT32_MAX / 2 ||
      Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || H < h || W < w || Ctot < nviews * C + (coord_channels ? 2 : 0) ||
      (coord_channels && (Ho < 2 || Wo < 2)) || tiles * chunks * B * nviews > INT32_MAX)
    return MVBEV_ERR_SHAPE;  // upsampling only (the 3x3 window bound); a grid side of 1 has no coord map
  pv::FwdArgs fa = {};
  WarpArgs& a = fa.w;
  const int es = pv::kind_size(src_kind), eo = pv::kind_size(out_kind);
  uint64_t src_bits = 0;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_warp_view& s = views[i];
    if (!s.src) return MVBEV_ERR_NULL;
    if (s.src_strides[1] != 1 && C > 1) return MVBEV_ERR_STRIDE;  // channels-last lines
    if (s.src_strides[0] < 0 || s.src_strides[2] < 0 || s.src_strides[3] < 0) return MVBEV_ERR_STRIDE;
    unpack_view(s, a.v[i], false);
    src_bits |= reinterpret_cast<uintptr_t>(s.src) | (uint64_t)s.src_strides[0] * es | (uint64_t)s.src_strides[2] * es |
                (uint64_t)s.src_strides[3] * es;
  }
  a.nviews = nviews;
  a.B = (int)B; a.C = (int)C; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)tiles;
  a.chunks = (int)chunks;
  a.nwg = (int)(tiles * chunks * B * nviews);
  set_fastdiv(a);
  fa.h = (int)h; fa.sw = (int)w;
  fa.sy = (float)h / (float)H;  // area_pixel_compute_scale(align_corners=false), as warp_up_kernel
  fa.sx = (float)w / (float)W;
  fa.out = out;
  fa.Ctot = Ctot;
  fa.coord = coord_channels ? 1 : 0;
  // a unit of channels starts at a multiple of 16 B inside its line, so the line starts decide: the source pixel
  // (base and strides), the output pixel (Ctot) and the view's offset inside it (v * C)
  fa.lw = pv::access_width(es, {src_bits});
  fa.stw = pv::access_width(eo, {reinterpret_cast<uintptr_t>(out), (uint64_t)Ctot * eo, (uint64_t)C * eo});
  const bool up = !(h == H && w == W);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)a.nwg), block(pv::kThreads);
#define MVBEV_PV_LAUNCH(T, TO)                                                                          \
  do {                                                                                                  \
    if (up) hipLaunchKernelGGL((pv::project_views_cl_kernel<T, TO, true>), grid, block, 0, st, fa);     \
    else hipLaunchKernelGGL((pv::project_views_cl_kernel<T, TO, false>), grid, block, 0, st, fa);       \
  } while (0)
  if (src_kind == 0) MVBEV_PV_LAUNCH(float, float);
  else if (src_kind == 1 && out_kind == 1) MVBEV_PV_LAUNCH(__half, __half);
  else if (src_kind == 1) MVBEV_PV_LAUNCH(__half, float);
  else if (out_kind == 2) MVBEV_PV_LAUNCH(__bf16, __bf16);
  else MVBEV_PV_LAUNCH(__bf16, float);
#undef MVBEV_PV_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

extern "C" int mvbev_project_views_cl_backward(const void* grad_out, int grad_out_kind, int64_t Ctot,
                                               const mvbev_project_views_grad* views, int nviews, int grad_src_kind,
                                               int64_t B, int64_t C, int64_t h, int64_t w, int64_t Ho, int64_t Wo,
                                               void* stream) {
  using namespace mvbev;
  if (!grad_out || !views) return MVBEV_ERR_NULL;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || nviews <= 0) return MVBEV_ERR_RANK;
  if (grad_src_kind < 0 || grad_src_kind > 2 || (grad_out_kind != grad_src_kind && grad_out_kind != 0))
    return MVBEV_ERR_SHAPE;
  if (nviews > kWarpMaxViews || h * w >= INT32_MAX || 9 * Ho * Wo >= INT32_MAX || C > INT32_MAX / 2 ||
      Ctot < nviews * C)
    return MVBEV_ERR_SHAPE;
  pv::AdjArgs a = {};
  const int eg = pv::kind_size(grad_out_kind), es = pv::kind_size(grad_src_kind);
  uint64_t go_bits = reinterpret_cast<uintptr_t>(grad_out) | (uint64_t)Ctot * eg | (uint64_t)C * eg;
  uint64_t gs_bits = 0;
  int n = 0;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_project_views_grad& v = views[i];
    if (!v.grad_src) continue;  // this view needs no gradient
    if (!v.row_ptr || !v.col || !v.val) return MVBEV_ERR_NULL;
    // channels-last lines, dense rows (the plan indexes source pixels linearly)
    if ((v.grad_src_strides[1] != 1 && C > 1) || v.grad_src_strides[3] < C ||
        v.grad_src_strides[2] != w * v.grad_src_strides[3] || v.grad_src_strides[0] < 0)
      return MVBEV_ERR_STRIDE;
    a.v[n++] = pv::AdjView{v.row_ptr, v.col, v.val, v.grad_src, v.grad_src_strides[0], v.grad_src_strides[3],
                           (int64_t)i * C};
    gs_bits |= reinterpret_cast<uintptr_t>(v.grad_src) | (uint64_t)v.grad_src_strides[0] * es |
               (uint64_t)v.grad_src_strides[3] * es;
  }
  if (n == 0) return MVBEV_OK;
  a.go = grad_out;
  a.Ctot = Ctot;
  a.gB = Ho * Wo * Ctot;
  a.nviews = n;
  a.B = (int)B; a.C = (int)C; a.P = (int)(h * w);
  a.pblocks = (int)ceil_div(h * w, pv::kPix);
  a.chunks = (int)ceil_div(C, pv::kCPB);
  const int64_t nwg = (int64_t)a.pblocks * a.chunks * n * B;
  if (nwg > INT32_MAX) return MVBEV_ERR_SHAPE;
  a.nwg = (int)nwg;
  a.lw = pv::access_width(eg, {go_bits});
  a.stw = pv::access_width(es, {gs_bits});
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)nwg), block(pv::kThreads);
#define MVBEV_PV_LAUNCH(TG, TS) hipLaunchKernelGGL((pv::project_views_cl_adjoint_kernel<TG, TS>), grid, block, 0, st, a)
  if (grad_src_kind == 0) MVBEV_PV_LAUNCH(float, float);
  else if (grad_src_kind == 1 && grad_out_kind == 1) MVBEV_PV_LAUNCH(__half, __half);
  else if (grad_src_kind == 1) MVBEV_PV_LAUNCH(float, __half);
  else if (grad_out_kind == 2) MVBEV_PV_LAUNCH(__bf16, __bf16);
  else MVBEV_PV_LAUNCH(float, __bf16);
#undef MVBEV_PV_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

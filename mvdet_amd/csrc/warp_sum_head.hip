// The ground-plane head of the "no joint spatial reasoning" ablation (no_joint_conv_variant.py:51-53,64-81)
// after its first 1x1 conv has been moved in front of the upsample and the warp, for gfx950:
//   hidden[p, :] = relu(bias + W_c coord(p) + sum_v warp_v(upsample(z_v))[p, :]),  z_v = W_v feat_v
//   map[p]       = w2 . hidden[p, :]
// A 1x1 conv is a per-pixel linear map over channels, the bilinear upsample (:64) and the zero-padded
// bilinear warp (:68) are per-channel linear maps over pixels, so they commute: z_v is a GEMM at backbone
// resolution (torch's), and everything after it is warp_sum_head_fwd_kernel.  Neither the upsampled maps
// (265 MB per view at config 2), nor the concatenated slab (620 MB), nor — in inference — anything of
// [B,Cm,Ho,Wo] is written.
//
// Forward thread mapping.  One wave per block; a block owns 16 consecutive pixels of one grid row, in four
// groups of four.  Per group the 64 lanes first compute the geometry, lane = (pixel of the group, view): the
// folded 3x3 backbone window of warp_common.h's up_window (the window of warp_up_kernel and of the adjoint
// plan, so forward and backward describe the same sparse matrix).  Then, pixel by pixel and view by view, the
// window is broadcast with v_readlane (scalar registers: a view that does not reach the pixel costs one
// scalar branch and no load) and the lanes turn into channels: lane l owns channels 4 l .. 4 l + 3 and
// 256 + 4 l .. 256 + 4 l + 3 of the channels-last line, one 16-B load per tap and half (a wave reads the 2-KB
// line of a tap contiguously).  Taps of weight 0 are not loaded (the plan has no entry for them either).
// The sum over views stays in registers, then bias, the coord term and ReLU, and the dot with w2 is a
// butterfly over the wave.  Training keeps the post-ReLU values: they pass through LDS ([pixel][channel],
// conflict-free both ways) so that a lane stores the group's four pixels of one channel plane as 16 bytes.
//
// Backward: warp_sum_head_bwd_kernel turns dmap into the gradient of the pre-activation, in place over
// hidden if asked, and leaves per-block sums for w2, bias and the coord weights; a second kernel adds them
// in a fixed order.  The gradient to z_v is the existing adjoint of the fused upsample + warp
// (mvbev_warp_views_adjoint with the upsampled plans).  No float atomics anywhere: results repeat bitwise.
#include "warp_common.h"

namespace mvbev {

constexpr int kShMaxCm = 512;     // 2 halves x 64 lanes x 4 channels
constexpr int kShCols = 16;       // pixels per block (one grid row segment)
constexpr int kShGroup = 4;       // pixels per geometry pass / per 16-B hidden store
constexpr int kShBoxRows = 12;    // grid rows per tile of mvbev_warp_upsampled_wino_boxes
constexpr int kShBwdThreads = 256;
constexpr int kShBwdChunk = 4096;  // pixels of one channel plane per backward block

struct ShArgs {
  WarpArgs w;    // views (src = z_v, channel stride 1), sizes of the UPSAMPLED image in w.H / w.W, C = Cm,
                 // tiles_x = blocks per grid row, tiles = box tiles per view
  int h, sw;     // backbone-resolution height and width (the fields of warp_up.hip's UpArgs)
  float sy, sx;  // upsample source scales in / out as PyTorch computes them
  const int32_t* boxes;  // mvbev_warp_upsampled_wino_boxes' [nviews][tiles][4], or null
  const float* bias;
  const float* w_coord;
  const float* w2;
  float* map;
  float* hidden;      // null: inference
  uint32_t vec_mask;  // bit v: view v's lines take 16-B loads (Cm, strides and base multiples of 4 floats)
  int hidden_vec;     // 16-B hidden stores (Wo % 4 == 0, aligned base)
};

__device__ __forceinline__ float sh_lanef(float x, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}

__global__ __launch_bounds__(kWave) void warp_sum_head_fwd_kernel(const ShArgs sa) {
  __shared__ __attribute__((aligned(16))) float hbuf[kShGroup * kShMaxCm];  // [pixel of the group][channel]
  const ShArgs& ua = sa;
  const WarpArgs& a = sa.w;
  const int lane = threadIdx.x;
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int tx = lb % a.tiles_x;
  const int rest = lb / a.tiles_x;
  const int v = rest % a.Ho, b = rest / a.Ho;
  const int u0 = tx * kShCols;
  const int Cm = a.C, Ho = a.Ho, Wo = a.Wo, h = ua.h, w = ua.sw;

  // this lane's channels and their parameters
  float pb[2][4], pw[2][4], pc0[2][4], pc1[2][4];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 256 * k + 4 * lane + j;
      const bool ok = c < Cm;
      pb[k][j] = ok ? sa.bias[c] : 0.f;
      pw[k][j] = ok ? sa.w2[c] : 0.f;
      pc0[k][j] = ok ? sa.w_coord[2 * c] : 0.f;
      pc1[k][j] = ok ? sa.w_coord[2 * c + 1] : 0.f;
    }
  const float cy = coord_value(v, Ho);  // mvbev_fill_coord_map_f32's values

  // geometry role of this lane: view gview of the group's pixel gpx
  const int gview = lane & 15, gpx = lane >> 4;
  const bool vlane = gview < a.nviews;
  float m[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) m[q] = a.v[vlane ? gview : 0].m[q];
  bool reach = vlane;  // geometry only: whether the view reaches this block's box tile at all
  if (vlane && ua.boxes) {
    const int tile = (v / kShBoxRows) * a.tiles_x + tx;
    const int32_t* bx = ua.boxes + 4 * ((int64_t)gview * a.tiles + tile);
    reach = bx[1] >= 0 || (bx[3] >> 30) != 0;
  }

  for (int g = 0; g < kShCols / kShGroup; ++g) {
    const int ug = u0 + kShGroup * g;
    if (ug >= Wo) break;
    // flag: 0 the view adds exactly 0 to this pixel, 1 a window to sample, 2 non-finite coordinates (NaN)
    int flag = 0;
    UpWindow uw;
    uw.rb = 0, uw.cb = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) uw.ay[q] = 0.f, uw.ax[q] = 0.f;
    if (reach && ug + gpx < Wo) {
      uw = up_window(m, ug + gpx, v, Ho, Wo, a.H, a.W, h, w, ua.sy, ua.sx);
      flag = uw.inside ? 1 : (uw.finite ? 0 : 2);
    }
    for (int px = 0; px < kShGroup; ++px) {
      const int u = ug + px;
      if (u >= Wo) break;
      float acc[2][4];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
      bool nan = false;
      for (int vi = 0; vi < a.nviews; ++vi) {
        const int src = px * 16 + vi;
        const int fl = __builtin_amdgcn_readlane(flag, src);
        if (fl == 0) continue;
        if (fl == 2) {
          nan = true;
          continue;
        }
        const int rb = __builtin_amdgcn_readlane(uw.rb, src), cb = __builtin_amdgcn_readlane(uw.cb, src);
        float ay[3], ax[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) ay[q] = sh_lanef(uw.ay[q], src), ax[q] = sh_lanef(uw.ax[q], src);
        const WarpView& vw = a.v[vi];
        const float* base = static_cast<const float*>(vw.src) + (int64_t)b * vw.sB;
        const bool vec = (sa.vec_mask >> vi) & 1u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float* prow = base + (int64_t)min(rb + i, h - 1) * vw.sH;  // (a row past the map has weight 0)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const float wt = ay[i] * ax[j];
            if (wt == 0.f) continue;  // uniform; no entry in the adjoint plan either
            const float* p = prow + (int64_t)min(cb + j, w - 1) * vw.sW;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const int c = 256 * k + 4 * lane;
              if (c >= Cm) continue;
              float4 q;
              if (vec) {
                q = *reinterpret_cast<const float4*>(p + c);
              } else {
                q.x = p[c];
                q.y = c + 1 < Cm ? p[c + 1] : 0.f;
                q.z = c + 2 < Cm ? p[c + 2] : 0.f;
                q.w = c + 3 < Cm ? p[c + 3] : 0.f;
              }
              acc[k][0] = fmaf(wt, q.x, acc[k][0]);
              acc[k][1] = fmaf(wt, q.y, acc[k][1]);
              acc[k][2] = fmaf(wt, q.z, acc[k][2]);
              acc[k][3] = fmaf(wt, q.w, acc[k][3]);
            }
          }
        }
      }
      const float cx = coord_value(u, Wo);
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float hv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float pre = acc[k][j] + fmaf(pc1[k][j], cy, fmaf(pc0[k][j], cx, pb[k][j]));
          if (nan) pre = __builtin_nanf("");
          hv[j] = relu_nan(pre);
          part = fmaf(hv[j], pw[k][j], part);  // (channels >= Cm: all-zero parameters, hv = 0)
        }
        if (sa.hidden)
          *reinterpret_cast<float4*>(&hbuf[px * kShMaxCm + 256 * k + 4 * lane]) = make_float4(hv[0], hv[1], hv[2], hv[3]);
      }
      if (nan) part = __builtin_nanf("");  // (Cm < 4 lanes' worth: every lane, not only those with a channel)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
      // no_joint_conv_variant.py:81 interpolates the map to its own size: the identity, except that torch's lerp
      // x + 0 * (x' - x) turns +-inf (a non-finite w2, bias or coord weight) into NaN at that pixel
      if (lane == 0) sa.map[((int64_t)b * Ho + v) * Wo + u] = isinf(part) ? __builtin_nanf("") : part;
    }
    if (sa.hidden) {
      __syncthreads();  // one wave: orders the LDS stores above before the transposed reads
      const int npx = min(kShGroup, Wo - ug);
      for (int c = lane; c < Cm; c += kWave) {
        float* hp = sa.hidden + (((int64_t)b * Cm + c) * Ho + v) * Wo + ug;
        const float h0 = hbuf[c], h1 = hbuf[kShMaxCm + c], h2 = hbuf[2 * kShMaxCm + c], h3 = hbuf[3 * kShMaxCm + c];
        if (sa.hidden_vec) {
          *reinterpret_cast<float4*>(hp) = make_float4(h0, h1, h2, h3);
        } else {
          hp[0] = h0;
          if (npx > 1) hp[1] = h1;
          if (npx > 2) hp[2] = h2;
          if (npx > 3) hp[3] = h3;
        }
      }
      __syncthreads();  // the next group overwrites hbuf
    }
  }
}

struct ShBwdArgs {
  const float* dmap;
  const float* hidden;
  const float* w2;
  float* dhidden;   // may be null, may alias hidden
  float* partials;  // may be null; [4][Cm][nblk]: rows dmap * hidden, dhidden, dhidden * x, dhidden * y
  int B, Cm, Ho, Wo, pchunks, nblk, vec;
};

// One block per (channel c, batch item b, chunk of kShBwdChunk pixels of the plane): dhidden = hidden <= 0 ? 0 :
// dmap * w2[c] (mvbev_relu_backward_f32's rule: the gradient passes where hidden is NaN), and the block's four
// sums by a fixed tree.
__global__ __launch_bounds__(kShBwdThreads) void warp_sum_head_bwd_kernel(const ShBwdArgs a) {
  __shared__ float red[4][kShBwdThreads];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int blk = blockIdx.y, b = blk / a.pchunks, pc = blk - b * a.pchunks;
  const int npix = a.Ho * a.Wo;
  const int p0 = pc * kShBwdChunk, p1 = min(npix, p0 + kShBwdChunk);
  const float wc = a.w2[c];
  const float* dm = a.dmap + (int64_t)b * npix;
  const int64_t plane = ((int64_t)b * a.Cm + c) * npix;
  const float* hd = a.hidden + plane;
  float* dh = a.dhidden ? a.dhidden + plane : nullptr;
  const double ix = 1.0 / (double)(a.Wo - 1), iy = 1.0 / (double)(a.Ho - 1);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  auto one = [&](int p, float hv, float g) __attribute__((always_inline)) {
    const float d = hv <= 0.f ? 0.f : g * wc;
    const int y = p / a.Wo, x = p - y * a.Wo;
    // (not coord_value: the reciprocal multiply can round differently, and changing it changes the gradients)
    const float cx = (float)((double)x * ix * 2.0 - 1.0), cy = (float)((double)y * iy * 2.0 - 1.0);
    s[0] = fmaf(g, hv, s[0]);
    s[1] += d;
    s[2] = fmaf(d, cx, s[2]);
    s[3] = fmaf(d, cy, s[3]);
    return d;
  };
  if (a.vec) {  // npix % 4 == 0 and 16-B aligned bases
    for (int p = p0 + 4 * tid; p < p1; p += 4 * kShBwdThreads) {
      const float4 hv = *reinterpret_cast<const float4*>(hd + p);
      const float4 g = *reinterpret_cast<const float4*>(dm + p);
      float4 d;
      d.x = one(p, hv.x, g.x);
      d.y = one(p + 1, hv.y, g.y);
      d.z = one(p + 2, hv.z, g.z);
      d.w = one(p + 3, hv.w, g.w);
      if (dh) *reinterpret_cast<float4*>(dh + p) = d;
    }
  } else {
    for (int p = p0 + tid; p < p1; p += kShBwdThreads) {
      const float d = one(p, hd[p], dm[p]);
      if (dh) dh[p] = d;
    }
  }
  if (!a.partials) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q][tid] = s[q];
  __syncthreads();
  for (int off = kShBwdThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + off];
    }
    __syncthreads();
  }
  if (tid < 4) a.partials[((int64_t)tid * a.Cm + c) * a.nblk + blk] = red[tid][0];
}

// Row r = q * Cm + c of partials[4 * Cm][nblk] -> grad_w2[c] (q = 0), grad_bias[c] (1), grad_w_coord[c][q - 2]:
// thread t adds columns t, t + 256, ... in order in fp64, then a fixed tree.
__global__ __launch_bounds__(kShBwdThreads) void warp_sum_head_params_kernel(const float* __restrict__ partials, int nblk,
                                                                            int Cm, float* gw2, float* gb, float* gwc) {
  __shared__ double red[kShBwdThreads];
  const int tid = threadIdx.x;
  const int q = blockIdx.x / Cm, c = blockIdx.x - q * Cm;
  float* out = q == 0 ? (gw2 ? gw2 + c : nullptr) : q == 1 ? (gb ? gb + c : nullptr) : (gwc ? gwc + 2 * c + (q - 2) : nullptr);
  if (!out) return;  // uniform over the block
  const float* row = partials + (int64_t)blockIdx.x * nblk;
  double s = 0;
  for (int i = tid; i < nblk; i += kShBwdThreads) s += (double)row[i];
  red[tid] = s;
  __syncthreads();
  for (int off = kShBwdThreads / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) *out = (float)red[0];
}

static int sh_check_plane(int64_t B, int64_t Cm, int64_t Ho, int64_t Wo) {
  if (B <= 0 || Cm <= 0 || Ho <= 0 || Wo <= 0) return MVBEV_ERR_RANK;
  if (Cm > kShMaxCm || Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || Ho * Wo > INT32_MAX - 4 * kShBwdThreads ||
      B * ceil_div(Ho * Wo, (int64_t)kShBwdChunk) > 65535)
    return MVBEV_ERR_SHAPE;
  return MVBEV_OK;
}

}  // namespace mvbev

extern "C" {

int mvbev_warp_sum_head_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t Cm, int64_t h,
                                    int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, const float* bias,
                                    const float* w_coord, const float* w2, float* map, float* hidden,
                                    const int32_t* boxes, void* stream) {
  using namespace mvbev;
  if (!views || !bias || !w_coord || !w2 || !map) return MVBEV_ERR_NULL;
  if (nviews <= 0 || B <= 0 || Cm <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
    return MVBEV_ERR_RANK;
  const int64_t tiles_x = ceil_div(Wo, (int64_t)kShCols);
  if (nviews > kWarpMaxViews || Cm > kShMaxCm || H < h || W < w || H > INT32_MAX / 2 || W > INT32_MAX / 2 ||
      Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || B * Ho * tiles_x > INT32_MAX)
    return MVBEV_ERR_SHAPE;
  ShArgs sa = {};
  ShArgs& ua = sa;
  WarpArgs& a = sa.w;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_warp_view& s = views[i];
    if (!s.src) return MVBEV_ERR_NULL;
    if (s.src_strides[1] != 1 || s.src_strides[0] < 0 || s.src_strides[2] < 0 || s.src_strides[3] < 0)
      return MVBEV_ERR_STRIDE;  // channels-last lines
    WarpView& d = a.v[i];
    unpack_view(s, d, false);  // (sC == 1: checked above)
    if (Cm % 4 == 0 && d.sB % 4 == 0 && d.sH % 4 == 0 && d.sW % 4 == 0 && (reinterpret_cast<uintptr_t>(d.src) & 15) == 0)
      sa.vec_mask |= 1u << i;
  }
  a.nviews = nviews;
  a.B = (int)B; a.C = (int)Cm; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.tiles_x = (int)tiles_x;
  a.tiles = (int)(tiles_x * ceil_div(Ho, (int64_t)kShBoxRows));  // the box tiles of one view
  a.nwg = (int)(B * Ho * tiles_x);
  ua.h = (int)h; ua.sw = (int)w;
  ua.sy = (float)h / (float)H;  // area_pixel_compute_scale(align_corners=false), as warp_up_kernel
  ua.sx = (float)w / (float)W;
  ua.boxes = boxes;
  sa.bias = bias, sa.w_coord = w_coord, sa.w2 = w2, sa.map = map, sa.hidden = hidden;
  sa.hidden_vec = hidden && Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(hidden) & 15) == 0;
  hipLaunchKernelGGL(warp_sum_head_fwd_kernel, dim3((unsigned)a.nwg), dim3(kWave), 0, as_stream(stream), sa);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int64_t mvbev_warp_sum_head_backward_blocks(int64_t B, int64_t Cm, int64_t Ho, int64_t Wo) {
  using namespace mvbev;
  if (sh_check_plane(B, Cm, Ho, Wo) != MVBEV_OK) return 0;
  return B * ceil_div(Ho * Wo, (int64_t)kShBwdChunk);
}

int mvbev_warp_sum_head_backward_f32(const float* dmap, const float* hidden, const float* w2, int64_t B, int64_t Cm,
                                     int64_t Ho, int64_t Wo, float* dhidden, float* partials, void* stream) {
  using namespace mvbev;
  if (!dmap || !hidden || !w2) return MVBEV_ERR_NULL;
  const int st = sh_check_plane(B, Cm, Ho, Wo);
  if (st != MVBEV_OK) return st;
  if (!dhidden && !partials) return MVBEV_OK;  // nothing is wanted
  ShBwdArgs a = {};
  a.dmap = dmap, a.hidden = hidden, a.w2 = w2, a.dhidden = dhidden, a.partials = partials;
  a.B = (int)B, a.Cm = (int)Cm, a.Ho = (int)Ho, a.Wo = (int)Wo;
  a.pchunks = (int)ceil_div(Ho * Wo, (int64_t)kShBwdChunk);
  a.nblk = (int)(B * a.pchunks);
  a.vec = (Ho * Wo) % 4 == 0 && ((reinterpret_cast<uintptr_t>(dmap) | reinterpret_cast<uintptr_t>(hidden) |
                                  reinterpret_cast<uintptr_t>(dhidden)) & 15) == 0;
  hipLaunchKernelGGL(warp_sum_head_bwd_kernel, dim3((unsigned)Cm, (unsigned)a.nblk), dim3(kShBwdThreads), 0,
                     as_stream(stream), a);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

int mvbev_warp_sum_head_grad_params_f32(const float* partials, int64_t nblocks, int64_t Cm, float* grad_w2,
                                        float* grad_bias, float* grad_w_coord, void* stream) {
  using namespace mvbev;
  if (!partials) return MVBEV_ERR_NULL;
  if (nblocks <= 0 || Cm <= 0) return MVBEV_ERR_RANK;
  if (Cm > kShMaxCm || nblocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  if (!grad_w2 && !grad_bias && !grad_w_coord) return MVBEV_OK;
  hipLaunchKernelGGL(warp_sum_head_params_kernel, dim3((unsigned)(4 * Cm)), dim3(kShBwdThreads), 0, as_stream(stream),
                     partials, (int)nblocks, (int)Cm, grad_w2, grad_bias, grad_w_coord);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

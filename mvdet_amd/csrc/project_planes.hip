// The weighted multi-plane projection on plain channels-last tensors (mvdet_amd.ProjectPlanes), gfx950:
//   world_v = sum_d warp_{v,d}(upsample(w_v[:, d] * feat_v)),   world = cat([world_v for v] + [coord_map])
// forward (project_planes_cl_kernel) and backward (project_planes_cl_adjoint_kernel), fp32 / fp16 / bf16 maps, fp32
// weights, fp32 math.  The sum over planes commutes with the gather, so neither the D products nor the D warped
// maps are ever written: a block reads feat_v and the D weight planes in place and writes its N C channels once.
//
// Mapping: project_views.hip's (project_common.h) — a block is 32 pixels x 8 lanes, a lane owns one 16-B unit of
// consecutive channels and steps through its pixel's channel chunk 8 units at a time.
//
// Forward.  A pixel has up to 8 planes x 9 (offset, coefficient) pairs, which do not stay in registers: lane d of a
// pixel computes plane d's sample geometry (warp_coord / up_window), multiplies each tap's coefficient by the
// weight plane's value at that tap and parks the pairs in LDS ([plane][tap][pixel], so a wave's 8 pixels read 8
// consecutive 8-B entries and a pixel's 8 lanes one broadcast address).  The channel loop then runs over planes
// and taps from LDS: per tap the term is (a_t * w[b, d, q_t]) * f[b, c, q_t] with a_t the coefficient
// project_views_cl_kernel uses (the window's column weight ax[j], rows combined by ay[i]; or the corner weight),
// one fp32 accumulator through the planes d = 0 .. D - 1.  With D = 1 and weights of exactly 1.0 these are
// project_views_cl_kernel's operations and bits.
//
// Backward.  grad_feat[b][q][c] = sum_d w[b][d][q] G_d[c],  grad_weight[b][d][q] = sum_c f[b][q][c] G_d[c], with
// G_d[c] = sum_e val_e grad_out[b][col_e][c_off + c] over row q of plane d's CSR adjoint plan (the sum and order of
// project_views_cl_adjoint_kernel).  A block is 32 source pixels x 8 lanes of one (batch item, view) and walks
// every channel, so the sum over C never leaves the block: each lane keeps its D partial sums (channel units in
// ascending order) in its own LDS slots, and the 8 lanes of a pixel are reduced by a xor butterfly (1, 2, 4).  One
// launch, no atomics, bitwise repeatable.
#include "project_common.h"

namespace mvbev {
namespace pp {

using pv::kCPB;
using pv::kLanes;
using pv::kPix;
using pv::kTH;
using pv::kThreads;
using pv::kTW;
using pv::Unit;

constexpr int kMaxPlanes = 8;
static_assert(kMaxPlanes <= kLanes, "lane d of a pixel prepares plane d");

struct FwdView {
  const void* src;   // [B][h][w][C]
  const float* wgt;  // [B][D][h][w] dense
  int64_t sB;
  int sH, sW;        // row and pixel strides of src in elements (a batch item's map spans < 2^31 elements)
};
struct FwdArgs {
  FwdView v[kWarpMaxViews];
  const float* mats;  // device [nviews][D][9]: src_norm <- dst_norm of the H x W source
  void* out;          // [B][Ho][Wo][Ctot]
  int64_t Ctot;
  int nviews, D, B, C, H, W, Ho, Wo, h, sw;
  float sy, sx;
  int tiles_x, tiles, chunks, nwg;
  int coord, lw, stw;
};

// the LDS of a forward block, per plane: pair[TAPS][32] {offset, coefficient}, ay[3][32] (UP), status[32]
template <int TAPS> struct FwdLds {
  static constexpr int kPlaneWords = (2 * TAPS + 3 + 1) * kPix;
  __device__ static uint2* pair(unsigned* base, int d, int t) {
    return reinterpret_cast<uint2*>(base + d * kPlaneWords) + t * kPix;
  }
  __device__ static float* ay(unsigned* base, int d, int i) {
    return reinterpret_cast<float*>(base + d * kPlaneWords + 2 * TAPS * kPix) + i * kPix;
  }
  __device__ static int* status(unsigned* base, int d) {
    return reinterpret_cast<int*>(base + d * kPlaneWords + (2 * TAPS + 3) * kPix);
  }
};
enum : int { kSkip = 0, kInside = 1, kNan = 2 };

// One block: 32 output pixels (4 x 8) of one (batch item, view, channel chunk), all planes.
template <typename T, typename TO, bool UP>
__global__ __launch_bounds__(kThreads) void project_planes_cl_kernel(const FwdArgs a) {
  constexpr int N = Unit<T>::N, TAPS = UP ? 9 : 4;
  using L = FwdLds<TAPS>;
  extern __shared__ __attribute__((aligned(16))) unsigned lds[];
  // lb = ((b * nviews + view) * chunks + chunk) * tiles + tile, tile = k * tiles_x + tx
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int tile = lb % a.tiles;
  int r = lb / a.tiles;
  const int chunk = r % a.chunks;
  r /= a.chunks;
  const int view = r % a.nviews, b = r / a.nviews;
  const int k = tile / a.tiles_x, tx = tile - k * a.tiles_x;
  const FwdView& vw = a.v[view];
  const int pix = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  const int v = k * kTH + pix / kTW, u = tx * kTW + pix % kTW;
  const bool live = v < a.Ho && u < a.Wo;
  const int H = a.H, W = a.W, D = a.D;

  if (live && lane < D) {  // plane `lane` of this pixel
    const int d = lane;
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = a.mats[((int64_t)view * D + d) * 9 + i];
    const float* wp = vw.wgt + ((int64_t)b * D + d) * a.h * a.sw;
    int st;
    if constexpr (UP) {
      const UpWindow uw = up_window(m, u, v, a.Ho, a.Wo, H, W, a.h, a.sw, a.sy, a.sx);
      st = uw.inside ? kInside : (uw.finite ? kSkip : kNan);
      if (uw.inside) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          L::ay(lds, d, i)[pix] = uw.ay[i];
#pragma unroll
          for (int j = 0; j < 3; ++j) {  // rows / columns past the map carry weight 0: clamp their address
            const int rr = min(uw.rb + i, a.h - 1), cc = min(uw.cb + j, a.sw - 1);
            const float cf = uw.ax[j] * wp[rr * a.sw + cc];
            L::pair(lds, d, 3 * i + j)[pix] = make_uint2((unsigned)(rr * vw.sH + cc * vw.sW), __float_as_uint(cf));
          }
        }
      }
    } else {
      const WarpCoord wc = warp_coord(m, u, v, a.Ho, a.Wo, H, W);
      st = wc.inside ? kInside : (wc.finite ? kSkip : kNan);
      if (wc.inside) {
        const float ix = wc.ix, iy = wc.iy;
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
        const float cw[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0),
                             (ix - fx0) * (iy - fy0)};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int x = x0 + (t & 1), y = y0 + (t >> 1);
          const bool ok = x >= 0 && x <= W - 1 && y >= 0 && y <= H - 1;
          const int cx = min(max(x, 0), W - 1), cy = min(max(y, 0), H - 1);
          // an out-of-bounds corner contributes 0 (GridSampler.h): a zero coefficient on a clamped address
          const float cf = ok ? cw[t] * wp[cy * a.sw + cx] : 0.f;
          L::pair(lds, d, t)[pix] = make_uint2((unsigned)(cy * vw.sH + cx * vw.sW), __float_as_uint(cf));
        }
      }
    }
    L::status(lds, d)[pix] = st;
  }
  __syncthreads();
  if (!live) return;

  bool nan = false, any = false;
  for (int d = 0; d < D; ++d) {
    const int st = L::status(lds, d)[pix];
    nan |= st == kNan;
    any |= st == kInside;
  }
  const T* src = static_cast<const T*>(vw.src) + (int64_t)b * vw.sB;
  TO* out = static_cast<TO*>(a.out) + (((int64_t)b * a.Ho + v) * a.Wo + u) * a.Ctot;
  TO* dst = out + (int64_t)view * a.C;
  const int c_begin = chunk * kCPB, c_end = min(a.C, c_begin + kCPB);
  const float fill = nan ? __builtin_nanf("") : 0.f;
  const bool sample = any && !nan;

  // acc += plane d's sample of N channels from x[tap][]: explicit fmas in project_views_cl_kernel's order
  // (contraction is the compiler's choice per call site; every path and instantiation must give the same bits)
  auto combine = [&](int d, const float (&cf)[TAPS], const float (&x)[TAPS][N], float (&acc)[N])
                     __attribute__((always_inline)) {
    if constexpr (UP) {
      float ay[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) ay[i] = L::ay(lds, d, i)[pix];
#pragma unroll
      for (int e = 0; e < N; ++e) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float row = 0.f;
#pragma unroll
          for (int j = 0; j < 3; ++j) row = __builtin_fmaf(cf[3 * i + j], x[3 * i + j][e], row);
          acc[e] = __builtin_fmaf(ay[i], row, acc[e]);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[e] = __builtin_fmaf(x[t][e], cf[t], acc[e]);
    }
  };

  for (int c = c_begin + lane * N; c < c_end; c += kLanes * N) {
    if (c + N <= c_end) {
      float acc[N];
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = fill;
      if (sample) {
        for (int d = 0; d < D; ++d) {
          if (L::status(lds, d)[pix] != kInside) continue;
          float cf[TAPS], x[TAPS][N];
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const uint2 oc = L::pair(lds, d, t)[pix];
            cf[t] = __uint_as_float(oc.y);
            pv::load_unit<T>(src + oc.x + c, a.lw, x[t]);
          }
          combine(d, cf, x, acc);
        }
      }
      if constexpr (std::is_same<T, TO>::value) {
        pv::store_unit<TO>(dst + c, a.stw, acc);
      } else {  // 16-bit maps, fp32 out: two 16-B units
        float lo[4], hi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = acc[e], hi[e] = acc[4 + e];
        pv::store_unit<TO>(dst + c, a.stw, lo);
        pv::store_unit<TO>(dst + c + 4, a.stw, hi);
      }
    } else {  // the last C % N channels, element by element
      for (int cc = c; cc < c_end; ++cc) {
        float acc[N] = {};
        acc[0] = fill;
        if (sample) {
          for (int d = 0; d < D; ++d) {
            if (L::status(lds, d)[pix] != kInside) continue;
            float cf[TAPS], x[TAPS][N] = {};
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
              const uint2 oc = L::pair(lds, d, t)[pix];
              cf[t] = __uint_as_float(oc.y);
              x[t][0] = to_f32<T>(src[oc.x + cc]);
            }
            combine(d, cf, x, acc);
          }
        }
        dst[cc] = pv::cvt_out<TO>(acc[0]);
      }
    }
  }
  if (a.coord && view == 0 && chunk == 0 && lane == 0) {  // mvbev_fill_coord_map_f32's values
    TO* cc = out + (int64_t)a.nviews * a.C;
    cc[0] = pv::cvt_out<TO>(coord_value(u, a.Wo));
    cc[1] = pv::cvt_out<TO>(coord_value(v, a.Ho));
  }
}

struct AdjView {
  const int32_t* rp;  // [D][P + 1]: plane d's row pointers into col / val
  const int32_t* col;
  const float* val;
  const void* f;      // [B][h][w][C] (read for grad_weight)
  const float* wgt;   // [B][D][h][w] (read for grad_feat)
  void* gf;           // [B][h][w][C] or NULL
  float* gw;          // [B][D][h][w] or NULL
  int64_t fB, fP;     // batch and pixel strides of f in elements
  int64_t gB, gP;     // ... of gf
  int64_t c_off;      // the view's first channel in a grad_out pixel
};
struct AdjArgs {
  AdjView v[kWarpMaxViews];
  const void* go;    // [B][Ho][Wo][Ctot]
  int64_t Ctot, oB;  // pixel and batch strides of go in elements
  int nviews, D, B, C, P, pblocks, nwg;
  int lw, fw, stw;   // access widths in bytes of the grad_out loads, the map loads and the grad_feat stores
};

// One block: 32 source pixels of one (batch item, view): every plane, every channel.
template <typename TG, typename TS>
__global__ __launch_bounds__(kThreads) void project_planes_cl_adjoint_kernel(const AdjArgs a) {
  constexpr int N = Unit<TS>::N;  // channels per lane and step: a 16-B unit of the maps
  __shared__ float gws[kMaxPlanes][kThreads];  // a lane's partial sums over its channels, one slot per plane
  const int lb = xcd_remap(blockIdx.x, a.nwg);
  const int pb = lb % a.pblocks;
  const int r = lb / a.pblocks;
  const int view = r % a.nviews, b = r / a.nviews;
  const int tid = threadIdx.x, lane = tid % kLanes;
  const int p = pb * kPix + tid / kLanes;
  if (p >= a.P) return;  // (no barrier below: a lane reads and writes its own LDS slots only)
  const AdjView& vw = a.v[view];
  const int D = a.D, C = a.C, P = a.P;
  const bool want_f = vw.gf != nullptr, want_w = vw.gw != nullptr;
  const TG* go = static_cast<const TG*>(a.go) + (int64_t)b * a.oB + vw.c_off;
  const TS* f = static_cast<const TS*>(vw.f) + (int64_t)b * vw.fB + (int64_t)p * vw.fP;
  TS* gf = static_cast<TS*>(vw.gf) + (int64_t)b * vw.gB + (int64_t)p * vw.gP;
  const float* wq = vw.wgt + (int64_t)b * D * P + p;  // + d P
  for (int d = 0; d < D; ++d) gws[d][tid] = 0.f;

  for (int c = lane * N; c < C; c += kLanes * N) {
    if (c + N <= C) {
      float acc[N], fx[N];
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] = 0.f, fx[i] = 0.f;
      if (want_w) pv::load_unit<TS>(f + c, a.fw, fx);
      for (int d = 0; d < D; ++d) {
        const int e0 = vw.rp[d * (P + 1) + p], e1 = vw.rp[d * (P + 1) + p + 1];
        if (e0 == e1) continue;  // G_d = 0: nothing to add (an empty row)
        float G[N];
#pragma unroll
        for (int i = 0; i < N; ++i) G[i] = 0.f;
        for (int e = e0; e < e1; ++e) {
          const float w = vw.val[e];
          const TG* g = go + (int64_t)vw.col[e] * a.Ctot + c;
          if constexpr (std::is_same<TG, TS>::value) {
            float x[N];
            pv::load_unit<TG>(g, a.lw, x);
#pragma unroll
            for (int i = 0; i < N; ++i) G[i] = __builtin_fmaf(w, x[i], G[i]);
          } else {  // fp32 grad_out, 16-bit maps: two 16-B units
            float x[2][4];
            pv::load_unit<TG>(g, a.lw, x[0]);
            pv::load_unit<TG>(g + 4, a.lw, x[1]);
#pragma unroll
            for (int i = 0; i < N; ++i) G[i] = __builtin_fmaf(w, x[i >> 2][i & 3], G[i]);
          }
        }
        if (want_f) {
          const float w = wq[(int64_t)d * P];
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] = __builtin_fmaf(w, G[i], acc[i]);
        }
        if (want_w) {
          float s = gws[d][tid];
#pragma unroll
          for (int i = 0; i < N; ++i) s = __builtin_fmaf(fx[i], G[i], s);
          gws[d][tid] = s;
        }
      }
      if (want_f) pv::store_unit<TS>(gf + c, a.stw, acc);
    } else {  // the last C % N channels, element by element
      for (int cc = c; cc < C; ++cc) {
        float acc = 0.f;
        const float fx = want_w ? to_f32<TS>(f[cc]) : 0.f;
        for (int d = 0; d < D; ++d) {
          const int e0 = vw.rp[d * (P + 1) + p], e1 = vw.rp[d * (P + 1) + p + 1];
          if (e0 == e1) continue;
          float G = 0.f;
          for (int e = e0; e < e1; ++e)
            G = __builtin_fmaf(vw.val[e], to_f32<TG>(go[(int64_t)vw.col[e] * a.Ctot + cc]), G);
          if (want_f) acc = __builtin_fmaf(wq[(int64_t)d * P], G, acc);
          if (want_w) gws[d][tid] = __builtin_fmaf(fx, G, gws[d][tid]);
        }
        if (want_f) gf[cc] = pv::cvt_out<TS>(acc);
      }
    }
  }
  if (want_w) {
    for (int d = 0; d < D; ++d) {  // the 8 lanes of a pixel: xor butterfly, the same sum in every lane
      float s = gws[d][tid];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      if (lane == 0) vw.gw[((int64_t)b * D + d) * P + p] = s;
    }
  }
}

}  // namespace pp
}  // namespace mvbev

extern "C" int mvbev_project_planes_cl_forward(const mvbev_project_planes_view* views, int nviews, int nplanes,
                                               const float* mats, int src_kind, int64_t B, int64_t C, int64_t h,
                                               int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* out,
                                               int out_kind, int64_t Ctot, int coord_channels, void* stream) {
  using namespace mvbev;
  if (!views || !out || !mats) return MVBEV_ERR_NULL;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || nviews <= 0 || nplanes <= 0)
    return MVBEV_ERR_RANK;
  if (src_kind < 0 || src_kind > 2 || (out_kind != src_kind && out_kind != 0)) return MVBEV_ERR_SHAPE;
  const int64_t tiles_x = ceil_div(Wo, pv::kTW), tiles = tiles_x * ceil_div(Ho, pv::kTH);
  const int64_t chunks = ceil_div(C, pv::kCPB);
  if (nviews > kWarpMaxViews || nplanes > pp::kMaxPlanes || C > INT32_MAX / 2 || H > INT32_MAX / 2 ||
      W > INT32_MAX / 2 || Ho > INT32_MAX / 2 || Wo > INT32_MAX / 2 || H < h || W < w || Ho < 2 || Wo < 2 ||
      Ctot < nviews * C + (coord_channels ? 2 : 0) ||
      B * nplanes * h * w > INT32_MAX || tiles * chunks * B * nviews > INT32_MAX)
    return MVBEV_ERR_SHAPE;  // upsampling only (the 3x3 window bound); a grid side of 1 has no normalised grid
  pp::FwdArgs a = {};
  const int es = pv::kind_size(src_kind), eo = pv::kind_size(out_kind);
  uint64_t src_bits = 0;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_project_planes_view& s = views[i];
    if (!s.feat || !s.weight) return MVBEV_ERR_NULL;
    if (s.feat_strides[1] != 1 && C > 1) return MVBEV_ERR_STRIDE;  // channels-last lines
    if (s.feat_strides[0] < 0 || s.feat_strides[2] < 0 || s.feat_strides[3] < C ||
        s.feat_strides[2] * (h - 1) + s.feat_strides[3] * (w - 1) + C > INT32_MAX)
      return MVBEV_ERR_STRIDE;  // a batch item's map is addressed with 32-bit element offsets
    a.v[i] = pp::FwdView{s.feat, s.weight, s.feat_strides[0], (int)s.feat_strides[2], (int)s.feat_strides[3]};
    src_bits |= reinterpret_cast<uintptr_t>(s.feat) | (uint64_t)s.feat_strides[0] * es |
                (uint64_t)s.feat_strides[2] * es | (uint64_t)s.feat_strides[3] * es;
  }
  a.mats = mats;
  a.out = out;
  a.Ctot = Ctot;
  a.nviews = nviews; a.D = nplanes;
  a.B = (int)B; a.C = (int)C; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.h = (int)h; a.sw = (int)w;
  a.sy = (float)h / (float)H;  // area_pixel_compute_scale(align_corners=false), as warp_up_kernel
  a.sx = (float)w / (float)W;
  a.tiles_x = (int)tiles_x; a.tiles = (int)tiles; a.chunks = (int)chunks;
  a.nwg = (int)(tiles * chunks * B * nviews);
  a.coord = coord_channels ? 1 : 0;
  a.lw = pv::access_width(es, {src_bits});
  a.stw = pv::access_width(eo, {reinterpret_cast<uintptr_t>(out), (uint64_t)Ctot * eo, (uint64_t)C * eo});
  const bool up = !(h == H && w == W);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)a.nwg), block(pv::kThreads);
  const size_t lds = (size_t)nplanes * (up ? pp::FwdLds<9>::kPlaneWords : pp::FwdLds<4>::kPlaneWords) * 4;
#define MVBEV_PP_LAUNCH(T, TO)                                                                            \
  do {                                                                                                    \
    if (up) hipLaunchKernelGGL((pp::project_planes_cl_kernel<T, TO, true>), grid, block, lds, st, a);     \
    else hipLaunchKernelGGL((pp::project_planes_cl_kernel<T, TO, false>), grid, block, lds, st, a);       \
  } while (0)
  if (src_kind == 0) MVBEV_PP_LAUNCH(float, float);
  else if (src_kind == 1 && out_kind == 1) MVBEV_PP_LAUNCH(__half, __half);
  else if (src_kind == 1) MVBEV_PP_LAUNCH(__half, float);
  else if (out_kind == 2) MVBEV_PP_LAUNCH(__bf16, __bf16);
  else MVBEV_PP_LAUNCH(__bf16, float);
#undef MVBEV_PP_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

extern "C" int mvbev_project_planes_cl_backward(const void* grad_out, int grad_out_kind, int64_t Ctot,
                                                const mvbev_project_planes_grad* views, int nviews, int nplanes,
                                                int map_kind, int64_t B, int64_t C, int64_t h, int64_t w, int64_t Ho,
                                                int64_t Wo, void* stream) {
  using namespace mvbev;
  if (!grad_out || !views) return MVBEV_ERR_NULL;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || nviews <= 0 || nplanes <= 0)
    return MVBEV_ERR_RANK;
  if (map_kind < 0 || map_kind > 2 || (grad_out_kind != map_kind && grad_out_kind != 0)) return MVBEV_ERR_SHAPE;
  if (nviews > kWarpMaxViews || nplanes > pp::kMaxPlanes || nplanes * (h * w + 1) >= INT32_MAX ||
      9 * nplanes * Ho * Wo >= INT32_MAX || C > INT32_MAX / 2 || Ctot < nviews * C)
    return MVBEV_ERR_SHAPE;
  pp::AdjArgs a = {};
  const int eg = pv::kind_size(grad_out_kind), es = pv::kind_size(map_kind);
  const uint64_t go_bits = reinterpret_cast<uintptr_t>(grad_out) | (uint64_t)Ctot * eg | (uint64_t)C * eg;
  uint64_t gf_bits = 0, f_bits = 0;
  int n = 0;
  for (int i = 0; i < nviews; ++i) {
    const mvbev_project_planes_grad& v = views[i];
    if (!v.grad_feat && !v.grad_weight) continue;  // this view needs no gradient
    if (!v.row_ptr || !v.col || !v.val) return MVBEV_ERR_NULL;
    if ((v.grad_feat && !v.weight) || (v.grad_weight && !v.feat)) return MVBEV_ERR_NULL;
    // channels-last lines, dense rows (the plans index source pixels linearly)
    if (v.grad_feat && ((v.grad_feat_strides[1] != 1 && C > 1) || v.grad_feat_strides[3] < C ||
                        v.grad_feat_strides[2] != w * v.grad_feat_strides[3] || v.grad_feat_strides[0] < 0))
      return MVBEV_ERR_STRIDE;
    if (v.grad_weight && ((v.feat_strides[1] != 1 && C > 1) || v.feat_strides[3] < C ||
                          v.feat_strides[2] != w * v.feat_strides[3] || v.feat_strides[0] < 0))
      return MVBEV_ERR_STRIDE;
    a.v[n++] = pp::AdjView{v.row_ptr, v.col, v.val, v.feat, v.weight, v.grad_feat, v.grad_weight,
                           v.feat_strides[0], v.feat_strides[3], v.grad_feat_strides[0], v.grad_feat_strides[3],
                           (int64_t)i * C};
    if (v.grad_feat)
      gf_bits |= reinterpret_cast<uintptr_t>(v.grad_feat) | (uint64_t)v.grad_feat_strides[0] * es |
                 (uint64_t)v.grad_feat_strides[3] * es;
    if (v.grad_weight)
      f_bits |= reinterpret_cast<uintptr_t>(v.feat) | (uint64_t)v.feat_strides[0] * es |
                (uint64_t)v.feat_strides[3] * es;
  }
  if (n == 0) return MVBEV_OK;
  a.go = grad_out;
  a.Ctot = Ctot;
  a.oB = Ho * Wo * Ctot;
  a.nviews = n; a.D = nplanes;
  a.B = (int)B; a.C = (int)C; a.P = (int)(h * w);
  a.pblocks = (int)ceil_div(h * w, pv::kPix);
  const int64_t nwg = (int64_t)a.pblocks * n * B;
  if (nwg > INT32_MAX) return MVBEV_ERR_SHAPE;
  a.nwg = (int)nwg;
  a.lw = pv::access_width(eg, {go_bits});
  a.fw = pv::access_width(es, {f_bits});
  a.stw = pv::access_width(es, {gf_bits});
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)nwg), block(pv::kThreads);
#define MVBEV_PP_LAUNCH(TG, TS) \
  hipLaunchKernelGGL((pp::project_planes_cl_adjoint_kernel<TG, TS>), grid, block, 0, st, a)
  if (map_kind == 0) MVBEV_PP_LAUNCH(float, float);
  else if (map_kind == 1 && grad_out_kind == 1) MVBEV_PP_LAUNCH(__half, __half);
  else if (map_kind == 1) MVBEV_PP_LAUNCH(float, __half);
  else if (grad_out_kind == 2) MVBEV_PP_LAUNCH(__bf16, __bf16);
  else MVBEV_PP_LAUNCH(float, __bf16);
#undef MVBEV_PP_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

// Layout and epilogue passes of the inference residual tail (mvdet_amd.ResidualTail: ResNet-18's layer4,
// multiview_detector/models/resnet.py:43-75, with eval-mode BatchNorm folded into the 3xbf16 convs).
//
// The 3x3 convs are conv_bf16x3.hip's LDS-DMA ring kernel, which reads and writes the split-bf16 blocked layout
// [item][C / 8][rows][cols][hi8, lo8]; the backbone's maps are fp32 channels-last.  What the convs do not have:
//   * cl_to_split_kernel: channels-last (fp32 / fp16 / bf16) -> split-bf16 blocked, plain or as the four
//     2 x 2 polyphase sub-grids x_pq[r][c] = x[2r + p][2c + q] on which a dilation-4 conv is a dilation-2 conv
//     (RingGeo<4> would need 176 KiB of LDS);
//   * res_close_kernel: out = relu(y + identity) from the conv's split-bf16 y (plain or polyphase) and the fp32
//     channels-last identity, to fp32 channels-last, and in the same pass the next block's conv1 input;
//   * poly_to_plain_kernel: the four sub-grids of a dilation-4 conv's output back onto the full grid.
// All three are element-wise over (pixel, 8-channel group) units of 32 B: no LDS, no atomics, vector stores only.
//
// Thread mapping (cdna_hip_programming.md, global memory coalescing).  Channels are the fast axis of a
// channels-last pixel, pixels the fast axis of a blocked plane, so neither side alone can own the lane index.
// A wave takes 16 consecutive pixels x 4 consecutive channel groups, lane = 4 * pixel + group: a pixel's four
// lanes touch 128 contiguous channels-last bytes (one cache line), and a group's 16 lanes touch 512 contiguous
// blocked bytes.  (Pixel-fastest lanes would read 32 B per 4 C-byte pixel pitch; group-fastest lanes would
// store 32-B pieces one plane apart.)
#include "common.h"

namespace mvbev {
namespace rt {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

constexpr int kMaxViews = 16;
constexpr int kPix = 16;  // pixels per wave
constexpr int kGrp = 4;   // 8-channel groups per wave

struct Views {
  const void* p[kMaxViews];
  int64_t sB[kMaxViews], sH[kMaxViews], sW[kMaxViews];  // element strides (the channel stride is 1)
};

struct Args {
  Views v;         // cl_to_split: the sources; res_close: the identity
  const u32x4* y;  // res_close / poly_to_plain: split-bf16 input
  float* out;      // res_close: fp32 [M][h][w][C]
  u32x4* next;     // split-bf16 output (res_close: optional)
  int B, M, G, h, w, h2, w2;
  int dh, dw;      // the pixel domain the threads walk
  int gq, pb;      // ceil(G / kGrp), ceil(dh * dw / kPix)
  int items;       // items of the domain
};

// The (item, group, row, column) of this thread in the launch's domain; false: nothing to do.
__device__ inline bool unit(const Args& a, int& item, int& g, int& r, int& c) {
  const int lane = threadIdx.x & 63;
  int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int pb = (int)(wv % a.pb);
  wv /= a.pb;
  const int gq = (int)(wv % a.gq);
  wv /= a.gq;
  if (wv >= a.items) return false;
  item = (int)wv;
  g = gq * kGrp + (lane & (kGrp - 1));
  const int px = pb * kPix + (lane >> 2);
  if (g >= a.G || px >= a.dh * a.dw) return false;
  r = px / a.dw;
  c = px - r * a.dw;
  return true;
}

// 8 fp32 values as the blocked layout's 16-B hi and 16-B lo pieces: hi = bf16(x) (nearest even), lo = bf16(x - hi)
__device__ inline void split8(const float (&x)[8], u32x4& hi, u32x4& lo) {
  unsigned int hw[4], lw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const __bf16 h0 = (__bf16)x[2 * j], h1 = (__bf16)x[2 * j + 1];
    const __bf16 l0 = (__bf16)(x[2 * j] - (float)h0), l1 = (__bf16)(x[2 * j + 1] - (float)h1);
    hw[j] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
    lw[j] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
  }
  hi = u32x4{hw[0], hw[1], hw[2], hw[3]};
  lo = u32x4{lw[0], lw[1], lw[2], lw[3]};
}

// hi + lo of one blocked unit, in fp32 (a bf16 is the upper half of its fp32)
__device__ inline void join8(const u32x4& hi, const u32x4& lo, float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = __builtin_bit_cast(float, hi[j] << 16) + __builtin_bit_cast(float, lo[j] << 16);
    x[2 * j + 1] = __builtin_bit_cast(float, hi[j] & 0xFFFF0000u) + __builtin_bit_cast(float, lo[j] & 0xFFFF0000u);
  }
}

template <int KIND> __device__ inline void load8(const void* base, int64_t off, float (&x)[8]);
template <> __device__ inline void load8<0>(const void* base, int64_t off, float (&x)[8]) {
  const floatx4* p = reinterpret_cast<const floatx4*>(static_cast<const float*>(base) + off);
  const floatx4 q0 = p[0], q1 = p[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = q0[j], x[4 + j] = q1[j];
}
template <> __device__ inline void load8<1>(const void* base, int64_t off, float (&x)[8]) {  // fp16
  const halfx8 q = *reinterpret_cast<const halfx8*>(static_cast<const _Float16*>(base) + off);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = (float)q[j];
}
template <> __device__ inline void load8<2>(const void* base, int64_t off, float (&x)[8]) {  // bf16
  const u16x8 q = *reinterpret_cast<const u16x8*>(static_cast<const unsigned short*>(base) + off);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = __builtin_bit_cast(float, (unsigned)q[j] << 16);
}

// The blocked unit index of full-grid pixel (r, c) of item m in the polyphase layout [4 M][G][h2][w2]
__device__ inline int64_t poly_unit(const Args& a, int m, int g, int r, int c) {
  const int item = 4 * m + 2 * (r & 1) + (c & 1);
  return (((int64_t)item * a.G + g) * a.h2 + (r >> 1)) * a.w2 + (c >> 1);
}
__device__ inline int64_t plain_unit(const Args& a, int m, int g, int r, int c) {
  return (((int64_t)m * a.G + g) * a.h + r) * a.w + c;
}

// Domain: the OUTPUT items ([M] plain over h x w, [4 M] polyphase over h2 x w2); a polyphase unit whose source
// pixel lies past an odd h or w is an exact zero, written here (the buffer is never memset).
template <int KIND, bool POLY>
__global__ __launch_bounds__(256) void cl_to_split_kernel(const Args a) {
  int item, g, r, c;
  if (!unit(a, item, g, r, c)) return;
  const int m = POLY ? item >> 2 : item;
  const int sr = POLY ? 2 * r + ((item >> 1) & 1) : r, sc = POLY ? 2 * c + (item & 1) : c;
  u32x4 hi = u32x4{0u, 0u, 0u, 0u}, lo = hi;
  if (sr < a.h && sc < a.w) {
    const int v = m / a.B, b = m - v * a.B;
    float x[8];
    load8<KIND>(a.v.p[v], (int64_t)b * a.v.sB[v] + (int64_t)sr * a.v.sH[v] + (int64_t)sc * a.v.sW[v] + 8 * g, x);
    split8(x, hi, lo);
  }
  u32x4* d = a.next + 2 * ((((int64_t)item * a.G + g) * a.dh + r) * a.dw + c);
  d[0] = hi;
  d[1] = lo;
}

// Domain: the full grid of the M items, h x w, or with a polyphase `next` the padded 2 h2 x 2 w2 (the units past
// h or w only store next's zero pads).  ReLU as torch's clamp_min(0): NaN stays NaN.
template <bool YPOLY, int NEXT>
__global__ __launch_bounds__(256) void res_close_kernel(const Args a) {
  int m, g, r, c;
  if (!unit(a, m, g, r, c)) return;
  if (NEXT == 2 && (r >= a.h || c >= a.w)) {
    u32x4* d = a.next + 2 * poly_unit(a, m, g, r, c);
    d[0] = u32x4{0u, 0u, 0u, 0u};
    d[1] = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const u32x4* yp = a.y + 2 * (YPOLY ? poly_unit(a, m, g, r, c) : plain_unit(a, m, g, r, c));
  float s[8], id[8];
  join8(yp[0], yp[1], s);
  const int v = m / a.B, b = m - v * a.B;
  load8<0>(a.v.p[v], (int64_t)b * a.v.sB[v] + (int64_t)r * a.v.sH[v] + (int64_t)c * a.v.sW[v] + 8 * g, id);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = s[j] + id[j];
    s[j] = t != t ? t : fmaxf(t, 0.f);
  }
  floatx4* o = reinterpret_cast<floatx4*>(a.out + (((int64_t)m * a.h + r) * a.w + c) * (8 * (int64_t)a.G) + 8 * g);
  o[0] = floatx4{s[0], s[1], s[2], s[3]};
  o[1] = floatx4{s[4], s[5], s[6], s[7]};
  if (NEXT != 0) {
    u32x4 hi, lo;
    split8(s, hi, lo);
    u32x4* d = a.next + 2 * (NEXT == 2 ? poly_unit(a, m, g, r, c) : plain_unit(a, m, g, r, c));
    d[0] = hi;
    d[1] = lo;
  }
}

// Domain: the full grid of the M items; a permutation copy of 32-B units.
__global__ __launch_bounds__(256) void poly_to_plain_kernel(const Args a) {
  int m, g, r, c;
  if (!unit(a, m, g, r, c)) return;
  const u32x4* s = a.y + 2 * poly_unit(a, m, g, r, c);
  u32x4* d = a.next + 2 * plain_unit(a, m, g, r, c);
  const u32x4 hi = s[0], lo = s[1];
  d[0] = hi;
  d[1] = lo;
}

// Sizes, domain and grid; the kernels index pixels and items in int32, addresses in int64.
static int plan(Args& a, int64_t B, int64_t M, int64_t C, int64_t h, int64_t w, bool poly_domain, bool poly_items,
                unsigned& nblk) {
  if (B <= 0 || M <= 0 || C <= 0 || h <= 0 || w <= 0) return MVBEV_ERR_RANK;
  if (C % 8 != 0 || M % B != 0) return MVBEV_ERR_SHAPE;
  const int64_t h2 = (h + 1) / 2, w2 = (w + 1) / 2;
  if (C > INT32_MAX || 4 * h2 * w2 > INT32_MAX - 64 || 4 * M > INT32_MAX) return MVBEV_ERR_SHAPE;
  a.B = (int)B; a.M = (int)M; a.G = (int)(C / 8); a.h = (int)h; a.w = (int)w; a.h2 = (int)h2; a.w2 = (int)w2;
  if (poly_items) {
    a.items = (int)(4 * M); a.dh = a.h2; a.dw = a.w2;
  } else if (poly_domain) {
    a.items = (int)M; a.dh = 2 * a.h2; a.dw = 2 * a.w2;
  } else {
    a.items = (int)M; a.dh = a.h; a.dw = a.w;
  }
  a.gq = (int)ceil_div(a.G, kGrp);
  a.pb = (int)ceil_div((int64_t)a.dh * a.dw, kPix);
  const int64_t waves = (int64_t)a.items * a.gq * a.pb;
  const int64_t blocks = ceil_div(waves, 4);
  if (blocks > INT32_MAX) return MVBEV_ERR_SHAPE;
  nblk = (unsigned)blocks;
  return MVBEV_OK;
}

// The channels-last views of a table: unit channel stride, 16-B aligned units
static int take_views(Views& t, const mvbev_warp_view* views, int nviews, int64_t C, int elem_size) {
  if (!views) return MVBEV_ERR_NULL;
  if (nviews <= 0 || nviews > kMaxViews) return MVBEV_ERR_SHAPE;
  const int64_t ea = 16 / elem_size;  // elements per 16 B
  for (int i = 0; i < nviews; ++i) {
    if (!views[i].src) return MVBEV_ERR_NULL;
    const int64_t* s = views[i].src_strides;
    if (s[1] != 1 || s[3] < C || s[2] < 0 || s[0] < 0) return MVBEV_ERR_STRIDE;
    if (s[0] % ea != 0 || s[2] % ea != 0 || s[3] % ea != 0) return MVBEV_ERR_STRIDE;
    if ((reinterpret_cast<uintptr_t>(views[i].src) & 15) != 0) return MVBEV_ERR_ALIGN;
    t.p[i] = views[i].src;
    t.sB[i] = s[0]; t.sH[i] = s[2]; t.sW[i] = s[3];
  }
  return MVBEV_OK;
}

}  // namespace rt
}  // namespace mvbev

extern "C" int mvbev_cl_to_split_bf16(const mvbev_warp_view* views, int nviews, int src_kind, int64_t B, int64_t C,
                                      int64_t h, int64_t w, int polyphase, void* dst, void* stream) {
  using namespace mvbev;
  using namespace mvbev::rt;
  if (!dst) return MVBEV_ERR_NULL;
  if (src_kind < 0 || src_kind > 2) return MVBEV_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) != 0) return MVBEV_ERR_ALIGN;
  Args a = {};
  int st = take_views(a.v, views, nviews, C, src_kind == 0 ? 4 : 2);
  if (st != MVBEV_OK) return st;
  unsigned nblk = 0;
  st = plan(a, B, (int64_t)nviews * B, C, h, w, false, polyphase != 0, nblk);
  if (st != MVBEV_OK) return st;
  a.next = static_cast<u32x4*>(dst);
  hipStream_t s = as_stream(stream);
#define MVBEV_RT_LAUNCH(K)                                                                          \
  do {                                                                                              \
    if (polyphase) hipLaunchKernelGGL((cl_to_split_kernel<K, true>), dim3(nblk), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((cl_to_split_kernel<K, false>), dim3(nblk), dim3(256), 0, s, a);        \
  } while (0)
  if (src_kind == 0) MVBEV_RT_LAUNCH(0);
  else if (src_kind == 1) MVBEV_RT_LAUNCH(1);
  else MVBEV_RT_LAUNCH(2);
#undef MVBEV_RT_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

extern "C" int mvbev_res_close_f32(const void* y, int y_polyphase, const mvbev_warp_view* identity, int nviews,
                                   int64_t B, int64_t C, int64_t h, int64_t w, float* out, void* next,
                                   int next_polyphase, void* stream) {
  using namespace mvbev;
  using namespace mvbev::rt;
  if (!y || !out) return MVBEV_ERR_NULL;
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(next)) & 15) != 0)
    return MVBEV_ERR_ALIGN;
  Args a = {};
  int st = take_views(a.v, identity, nviews, C, 4);
  if (st != MVBEV_OK) return st;
  const bool npoly = next && next_polyphase;
  unsigned nblk = 0;
  st = plan(a, B, (int64_t)nviews * B, C, h, w, npoly, false, nblk);
  if (st != MVBEV_OK) return st;
  a.y = static_cast<const u32x4*>(y);
  a.out = out;
  a.next = static_cast<u32x4*>(next);
  hipStream_t s = as_stream(stream);
#define MVBEV_RT_LAUNCH(YP)                                                                               \
  do {                                                                                                    \
    if (!next) hipLaunchKernelGGL((res_close_kernel<YP, 0>), dim3(nblk), dim3(256), 0, s, a);             \
    else if (!npoly) hipLaunchKernelGGL((res_close_kernel<YP, 1>), dim3(nblk), dim3(256), 0, s, a);       \
    else hipLaunchKernelGGL((res_close_kernel<YP, 2>), dim3(nblk), dim3(256), 0, s, a);                   \
  } while (0)
  if (y_polyphase) MVBEV_RT_LAUNCH(true); else MVBEV_RT_LAUNCH(false);
#undef MVBEV_RT_LAUNCH
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

extern "C" int mvbev_split_polyphase_to_plain(const void* src, int64_t M, int64_t C, int64_t h, int64_t w, void* dst,
                                              void* stream) {
  using namespace mvbev;
  using namespace mvbev::rt;
  if (!src || !dst) return MVBEV_ERR_NULL;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) != 0) return MVBEV_ERR_ALIGN;
  Args a = {};
  unsigned nblk = 0;
  const int st = plan(a, M, M, C, h, w, false, false, nblk);
  if (st != MVBEV_OK) return st;
  a.y = static_cast<const u32x4*>(src);
  a.next = static_cast<u32x4*>(dst);
  hipLaunchKernelGGL(poly_to_plain_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), a);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

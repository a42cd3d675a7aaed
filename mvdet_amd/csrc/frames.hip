// The camera-frame front for gfx950: decoded uint8 frames to the normalized fp32 views the detectors take, i.e. the
// reference's T.Compose([T.Resize(size), T.ToTensor(), normalize]) (main.py:38-40, applied per camera by
// frameDataset.__getitem__, frameDataset.py:127-133) for every view and batch item in ONE launch.
//
// T.Resize of a PIL image is Pillow's Image.resize(..., BILINEAR): two separable passes over 8-bit data with 22-bit
// fixed-point coefficients, horizontal first, rounded and clipped to uint8 after EACH pass
//   acc = 1 << 21;  acc += px * coef (the taps);  out = clamp(acc >> 22, 0, 255)          (int32)
// and ToTensor + Normalize map each of a channel's 256 byte values to one fp32 value.  The coefficient tables
// (mvdet_amd.frames.resample_table restates Pillow's precompute_coeffs / normalize_coeffs_8bpc in float64) and the
// [3][256] value table are built on the host, so the result is bit for bit what the CPU transform gives.
//
// frames_kernel: a workgroup of 256 threads owns a TH x TW output tile of one (batch item, view).
//   0. the value table, and the tile's bounds and coefficients, go to LDS.  Bounds are clamped to the staged box
//      there, so a corrupt table gives wrong values, never an access outside the box.
//   1. the input box the tile needs is staged as bytes in LDS.  It is fetched as ALIGNED dwords: a row's bytes start
//      at (address & 3) inside its first dword, which is kept in LDS, so rows of any byte stride are read with
//      coalesced dword loads and nothing is shifted.  (An aligned dword that holds one byte of the box lies on that
//      byte's page; the bytes of it outside the box are never used.)
//   2. the horizontal pass writes a second uint8 LDS array, one plane per channel [3][box rows][TW].  A pixel's three
//      bytes are cut out of two LDS dwords with a funnel shift (LDS bytes are read a dword at a time throughout).
//   3. the vertical pass reads it a dword (four columns) at a time, maps the bytes through the table and stores
//      fp32: a thread holds four columns of a row in all three channels, i.e. twelve consecutive floats of a
//      channels-last view (3 TW floats per tile row and wave) or four consecutive floats of each NCHW channel row,
//      written as float4 when the output is 16-byte aligned (scalar stores otherwise: the same values).
// An axis of equal input and output size, which Pillow skips, runs with the formula's own table for that case: one
// tap of weight 1 << 22 (and a second of weight 0), an exact copy.
//
// The tile is the first of 16 x 64, 8 x 64, 8 x 32 whose LDS need is below 64 KB (frames_pick); 8 x 32 holds
// downscales up to 7x on both axes.  No register array is indexed by the tap count (no scratch).
#include "common.h"

namespace mvbev {

constexpr int kFrThreads = 256;
constexpr int kFrMaxViews = 16;
constexpr int kFrMaxTaps = 64;           // ksize per axis accepted by the entry point
constexpr int64_t kFrLdsLimit = 65536;   // dynamic LDS a launch may ask for without a function attribute

struct FrArgs {
  const uint8_t* src[kFrMaxViews];
  int64_t sB[kFrMaxViews], sH[kFrMaxViews];  // bytes
  const int32_t *bx, *cx, *by, *cy;          // bounds [out][2], coef [out][ks]
  const float* lut;                          // [3][256]
  float* out;
  int64_t oB, oV, oC, oH, oW;                // elements
  int nviews, H, W, h, w, ksx, ksy;
  int capW, capH;                            // the staged box's capacity in pixels / rows
  int tiles_x, tiles_y;
  int vec;  // float4 stores: 1 a 16-byte aligned channels-last view, 2 16-byte aligned NCHW rows, 0 neither
};

// pixels an axis' staged box can span for `tile` outputs: first >= c0 - s - 0.5 and end <= c1 + s + 0.5 with
// c1 - c0 = (tile - 1) scale, so the span is below (tile - 1) scale + 2 s + 1; s = (ks - 1) / 2 >= the support
static int64_t fr_cap(int64_t in, int64_t out, int ks, int tile) {
  const double span = (double)(tile - 1) * ((double)in / (double)out) + (double)(ks - 1) + 1.0;
  return std::min<int64_t>(in, (int64_t)span + 2);
}

struct FrLayout {
  int capW, capH;
  int64_t pitchA;  // bytes per staged row (a dword multiple, 3 bytes of misalignment included)
  int64_t bytes;
};

static FrLayout fr_layout(int64_t H, int64_t W, int64_t h, int64_t w, int ksx, int ksy, int TH, int TW) {
  FrLayout l;
  l.capW = (int)fr_cap(W, w, ksx, TW);
  l.capH = (int)fr_cap(H, h, ksy, TH);
  l.pitchA = ((int64_t)l.capW * 3 + 3 + 3) / 4 * 4;
  l.bytes = 3 * 256 * 4 + (int64_t)TW * (ksx + 2) * 4 + (int64_t)TH * (ksy + 2) * 4 + l.capH * l.pitchA +
            (int64_t)l.capH * TW * 3;
  return l;
}

// the tile (0: 16 x 64, 1: 8 x 64, 2: 8 x 32) or -1 when none fits
static int frames_pick(int64_t H, int64_t W, int64_t h, int64_t w, int ksx, int ksy, FrLayout* l) {
  const int th[3] = {16, 8, 8}, tw[3] = {64, 64, 32};
  for (int i = 0; i < 3; ++i) {
    *l = fr_layout(H, W, h, w, ksx, ksy, th[i], tw[i]);
    if (l->bytes <= kFrLdsLimit) return i;
  }
  return -1;
}

__device__ __forceinline__ int fr_clip8(int acc) { return min(max(acc >> 22, 0), 255); }

template <int TH, int TW>
__global__ __launch_bounds__(kFrThreads) void frames_kernel(const FrArgs a) {
  extern __shared__ __align__(16) unsigned char fr_lds[];
  float* lut = reinterpret_cast<float*>(fr_lds);            // [3][256]
  int* cxs = reinterpret_cast<int*>(lut + 3 * 256);         // [TW][ksx]
  int* bxs = cxs + TW * a.ksx;                              // [TW][2]: first relative to the box, count
  int* cys = bxs + TW * 2;                                  // [TH][ksy]
  int* bys = cys + TH * a.ksy;                              // [TH][2]
  unsigned char* A = reinterpret_cast<unsigned char*>(bys + TH * 2);  // [capH][pitchA]
  const int pitchA = (a.capW * 3 + 3 + 3) / 4 * 4;
  unsigned char* Bm = A + (size_t)a.capH * pitchA;          // [3][capH][TW]

  const int tid = threadIdx.x;
  int q = blockIdx.x;
  const int tx = q % a.tiles_x;
  q /= a.tiles_x;
  const int ty = q % a.tiles_y;
  q /= a.tiles_y;
  const int view = q % a.nviews;
  const int b = q / a.nviews;
  const int ox0 = tx * TW, oy0 = ty * TH;
  const int nx = min(TW, a.w - ox0), ny = min(TH, a.h - oy0);

  // the box: [x_lo, x_end) x [y_lo, y_end), inside the image and inside the staged capacity
  const int x_lo = min(max(a.bx[2 * ox0], 0), a.W - 1);
  const int y_lo = min(max(a.by[2 * oy0], 0), a.H - 1);
  const int xl = ox0 + nx - 1, yl = oy0 + ny - 1;
  const int x_end = min(max(a.bx[2 * xl] + a.bx[2 * xl + 1], x_lo + 1), min(a.W, x_lo + a.capW));
  const int y_end = min(max(a.by[2 * yl] + a.by[2 * yl + 1], y_lo + 1), min(a.H, y_lo + a.capH));
  const int boxW = x_end - x_lo, boxH = y_end - y_lo;

  // 0. tables
  for (int i = tid; i < 3 * 256; i += kFrThreads) lut[i] = a.lut[i];
  for (int i = tid; i < nx * a.ksx; i += kFrThreads) cxs[i] = a.cx[(int64_t)ox0 * a.ksx + i];
  for (int i = tid; i < ny * a.ksy; i += kFrThreads) cys[i] = a.cy[(int64_t)oy0 * a.ksy + i];
  if (tid < nx) {
    const int f = min(max(a.bx[2 * (ox0 + tid)], x_lo), x_end - 1);
    bxs[2 * tid] = f - x_lo;
    bxs[2 * tid + 1] = min(max(a.bx[2 * (ox0 + tid) + 1], 0), min(a.ksx, x_end - f));
  } else if (tid >= 64 && tid - 64 < ny) {
    const int r = tid - 64;
    const int f = min(max(a.by[2 * (oy0 + r)], y_lo), y_end - 1);
    bys[2 * r] = f - y_lo;
    bys[2 * r + 1] = min(max(a.by[2 * (oy0 + r) + 1], 0), min(a.ksy, y_end - f));
  }

  // 1. stage the box as aligned dwords
  const int64_t sH = a.sH[view];
  const uint8_t* g0 = a.src[view] + (int64_t)b * a.sB[view] + (int64_t)y_lo * sH + (int64_t)x_lo * 3;
  const unsigned mis0 = (unsigned)(reinterpret_cast<uintptr_t>(g0) & 3);
  const unsigned misH = (unsigned)(sH & 3);
  const int dpr = pitchA >> 2;
  {
    const int step_r = kFrThreads / dpr, step_d = kFrThreads % dpr;
    int r = tid / dpr, d = tid % dpr;
    uint32_t* A32w = reinterpret_cast<uint32_t*>(A);
    while (r < boxH) {
      const unsigned mis = (mis0 + (unsigned)r * misH) & 3;
      const int ndw = (int)(mis + (unsigned)boxW * 3 + 3) >> 2;
      if (d < ndw) {
        const uint8_t* g = g0 + (int64_t)r * sH - mis;
        A32w[r * dpr + d] = reinterpret_cast<const uint32_t*>(g)[d];
      }
      r += step_r, d += step_d;
      if (d >= dpr) d -= dpr, ++r;
    }
  }
  __syncthreads();

  // 2. horizontal pass into the planes Bm[c][r][ox].  A thread keeps its column (kFrThreads is a multiple of TW) and
  // walks the rows; a pixel's three bytes come out of two dwords (any byte offset) with one funnel shift.
  const uint32_t* A32 = reinterpret_cast<const uint32_t*>(A);
  const int plane = a.capH * TW;
  {
    const int ox = tid % TW;
    if (ox < nx) {
      const int n = bxs[2 * ox + 1];
      const unsigned o0 = (unsigned)bxs[2 * ox] * 3;
      const int* cf = cxs + ox * a.ksx;
      for (int r = tid / TW; r < boxH; r += kFrThreads / TW) {
        const unsigned o = ((mis0 + (unsigned)r * misH) & 3) + o0;
        const uint32_t* row = A32 + r * dpr;
        int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
        for (int k = 0; k < n; ++k) {
          const unsigned bo = o + 3 * k;
          // (the second dword may lie past the row's bytes, never past the LDS allocation: Bm follows A)
          const uint64_t two = ((uint64_t)row[(bo >> 2) + 1] << 32) | row[bo >> 2];
          const uint32_t px = (uint32_t)(two >> (8 * (bo & 3)));
          const int c = cf[k];
          acc0 += (int)(px & 255) * c;
          acc1 += (int)((px >> 8) & 255) * c;
          acc2 += (int)((px >> 16) & 255) * c;
        }
        unsigned char* o3 = Bm + r * TW + ox;
        o3[0] = (unsigned char)fr_clip8(acc0);
        o3[plane] = (unsigned char)fr_clip8(acc1);
        o3[2 * plane] = (unsigned char)fr_clip8(acc2);
      }
    }
  }
  __syncthreads();

  // 3. vertical pass, value table, store: a thread owns four consecutive columns of one row in all three channels
  // (one dword per plane and tap) and stores them as float4 where the output allows it
  const uint32_t* B32 = reinterpret_cast<const uint32_t*>(Bm);
  float* ob = a.out + (int64_t)b * a.oB + (int64_t)view * a.oV;
  constexpr int G = TW / 4;
  for (int i = tid; i < TH * G; i += kFrThreads) {
    const int r = i / G, g = i % G, ox = 4 * g;
    if (r >= ny || ox >= nx) continue;
    const int n = bys[2 * r + 1];
    const uint32_t* p = B32 + bys[2 * r] * G + g;
    const int* cf = cys + r * a.ksy;
    int acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c][j] = 1 << 21;
    for (int k = 0; k < n; ++k) {
      const int w = cf[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t d = p[(c * a.capH + k) * G];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[c][j] += (int)((d >> (8 * j)) & 255) * w;
      }
    }
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = lut[c * 256 + fr_clip8(acc[c][j])];
    float* o = ob + (int64_t)(oy0 + r) * a.oH + (int64_t)(ox0 + ox) * a.oW;
    const bool full = ox + 4 <= nx;
    if (a.vec == 1 && full) {  // a channels-last view: twelve consecutive floats
      float4* o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(v[0][0], v[1][0], v[2][0], v[0][1]);
      o4[1] = make_float4(v[1][1], v[2][1], v[0][2], v[1][2]);
      o4[2] = make_float4(v[2][2], v[0][3], v[1][3], v[2][3]);
    } else if (a.vec == 2 && full) {  // NCHW: four consecutive floats per channel
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o + (int64_t)c * a.oC) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ox + j < nx) o[(int64_t)c * a.oC + (int64_t)j * a.oW] = v[c][j];
    }
  }
}

}  // namespace mvbev

extern "C" {

int mvbev_frames_resize_normalize_u8(const mvbev_frame_view* views, int nviews, int64_t B, int64_t H, int64_t W,
                                     int64_t h, int64_t w, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                                     const int32_t* bounds_y, const int32_t* coef_y, int ksy, const float* lut,
                                     float* out, const int64_t out_strides[5], void* stream) {
  using namespace mvbev;
  if (!views || !bounds_x || !coef_x || !bounds_y || !coef_y || !lut || !out || !out_strides) return MVBEV_ERR_NULL;
  if (nviews <= 0 || B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || ksx <= 0 || ksy <= 0) return MVBEV_ERR_RANK;
  if (nviews > kFrMaxViews || ksx > kFrMaxTaps || ksy > kFrMaxTaps) return MVBEV_ERR_SHAPE;
  const int64_t lim = INT32_MAX / 2;
  if (H > lim || W > lim / 3 || h > lim || w > lim || h * w > lim / 3 || B * nviews > lim / (3 * h * w))
    return MVBEV_ERR_SHAPE;  // the output below 2^31 elements, a row below 2^31 bytes
  for (int k = 0; k < 5; ++k)
    if (out_strides[k] < 0) return MVBEV_ERR_STRIDE;
  FrLayout l;
  const int tile = frames_pick(H, W, h, w, ksx, ksy, &l);
  if (tile < 0) return MVBEV_ERR_SHAPE;  // the staged box does not fit LDS (mvdet_amd.frames.supported)
  FrArgs a = {};
  for (int i = 0; i < nviews; ++i) {
    if (!views[i].src) return MVBEV_ERR_NULL;
    if (views[i].batch_stride < 0 || views[i].row_stride < 0) return MVBEV_ERR_STRIDE;
    a.src[i] = static_cast<const uint8_t*>(views[i].src);
    a.sB[i] = views[i].batch_stride, a.sH[i] = views[i].row_stride;
  }
  a.bx = bounds_x, a.cx = coef_x, a.by = bounds_y, a.cy = coef_y, a.lut = lut, a.out = out;
  a.oB = out_strides[0], a.oV = out_strides[1], a.oC = out_strides[2], a.oH = out_strides[3], a.oW = out_strides[4];
  a.nviews = nviews, a.H = (int)H, a.W = (int)W, a.h = (int)h, a.w = (int)w, a.ksx = ksx, a.ksy = ksy;
  a.capW = l.capW, a.capH = l.capH;
  const bool al = reinterpret_cast<uintptr_t>(out) % 16 == 0 && a.oB % 4 == 0 && a.oV % 4 == 0 && a.oH % 4 == 0;
  a.vec = al && a.oC == 1 && a.oW == 3 ? 1 : al && a.oW == 1 && a.oC % 4 == 0 ? 2 : 0;
  const int th[3] = {16, 8, 8}, tw[3] = {64, 64, 32};
  a.tiles_x = (int)ceil_div(w, (int64_t)tw[tile]);
  a.tiles_y = (int)ceil_div(h, (int64_t)th[tile]);
  const int64_t nwg = B * nviews * a.tiles_x * a.tiles_y;
  if (nwg > INT32_MAX) return MVBEV_ERR_SHAPE;
  const dim3 grid((unsigned)nwg), block(kFrThreads);
  const size_t lds = (size_t)l.bytes;
  if (tile == 0)
    hipLaunchKernelGGL((frames_kernel<16, 64>), grid, block, lds, as_stream(stream), a);
  else if (tile == 1)
    hipLaunchKernelGGL((frames_kernel<8, 64>), grid, block, lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL((frames_kernel<8, 32>), grid, block, lds, as_stream(stream), a);
  MVBEV_CHECK_LAUNCH();
  return MVBEV_OK;
}

}  // extern "C"

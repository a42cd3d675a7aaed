// What the channels-last projection ops (project_views.hip, project_planes.hip) share: the 32-pixel x 8-lane line
// mapping's constants, the 16-B unit moved as host-chosen access widths, and the choice of those widths.
#pragma once

#include <initializer_list>

#include "warp_common.h"

namespace mvbev {
namespace pv {

constexpr int kPix = 32, kLanes = 8, kThreads = kPix * kLanes;
constexpr int kTH = 4, kTW = 8;  // output pixels of a forward block: 4 rows x 8 columns
#ifndef MVBEV_PV_CPB
#define MVBEV_PV_CPB 256  // channels per block: the geometry (~150 VALU instructions) is paid once per chunk
#endif
constexpr int kCPB = MVBEV_PV_CPB;
static_assert(kTH * kTW == kPix && kCPB % (kLanes * 8) == 0, "a chunk is whole rounds of the 8 lanes' units");

template <typename T> struct Unit { static constexpr int N = 16 / (int)sizeof(T); };  // elements per 16-B unit

template <typename T> __device__ inline T cvt_out(float v);
template <> __device__ inline float cvt_out<float>(float v) { return v; }
template <> __device__ inline __half cvt_out<__half>(float v) { return __float2half(v); }  // round to nearest even
template <> __device__ inline __bf16 cvt_out<__bf16>(float v) { return (__bf16)v; }        // round to nearest even

// N elements at p as accesses of `width` bytes (a uniform value: 16, 8, 4 or sizeof(T)) -> fp32
template <typename T>
__device__ inline void load_unit(const T* __restrict__ p, int width, float (&x)[Unit<T>::N]) {
  constexpr int N = Unit<T>::N;
  union { u32x4_t q; uint2 d[2]; unsigned s[4]; T e[N]; } u;
  if (width == 16) {
    u.q = *reinterpret_cast<const u32x4_t*>(p);
  } else if (width == 8) {
    u.d[0] = reinterpret_cast<const uint2*>(p)[0];
    u.d[1] = reinterpret_cast<const uint2*>(p)[1];
  } else if (sizeof(T) == 4 || width == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) u.s[i] = reinterpret_cast<const unsigned*>(p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) u.e[i] = p[i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = to_f32<T>(u.e[i]);
}

// N fp32 values rounded once to T and stored at p as accesses of `width` bytes
template <typename T>
__device__ inline void store_unit(T* __restrict__ p, int width, const float (&x)[Unit<T>::N]) {
  constexpr int N = Unit<T>::N;
  union { u32x4_t q; uint2 d[2]; unsigned s[4]; T e[N]; } u;
#pragma unroll
  for (int i = 0; i < N; ++i) u.e[i] = cvt_out<T>(x[i]);
  if (width == 16) {
    *reinterpret_cast<u32x4_t*>(p) = u.q;
  } else if (width == 8) {
    reinterpret_cast<uint2*>(p)[0] = u.d[0];
    reinterpret_cast<uint2*>(p)[1] = u.d[1];
  } else if (sizeof(T) == 4 || width == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<unsigned*>(p)[i] = u.s[i];
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = u.e[i];
  }
}

// the widest of 16, 8, 4 (and esize) bytes that divides every one of the byte quantities in q
inline int access_width(int esize, std::initializer_list<uint64_t> q) {
  uint64_t any = 0;
  for (uint64_t x : q) any |= x;
  for (int wd = 16; wd > esize; wd >>= 1)
    if (any % (uint64_t)wd == 0) return wd;
  return esize;
}

inline int kind_size(int kind) { return kind == 0 ? 4 : 2; }

}  // namespace pv
}  // namespace mvbev

// mx_common.h — the MX (OCP Microscaling) device helpers shared by mx.hip (the
// block-scaled sum) and mx_quant.hip (quantise, wide-output fold): the format
// table, the scale, the dequantising add, the requantising narrow in its two
// rounding modes and a source's request.  Moved textually out of mx.hip; the arithmetic and the
// GLOO_MX_SCALED_CVT switch are described at the head of that file.
// Internal: device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "buffer_rsrc.h"
#include "gloo_amd.h"

// a scale multiply followed by an add is what the compiler would otherwise fuse
#pragma clang fp contract(off)

#ifndef GLOO_MX_SCALED_CVT
#define GLOO_MX_SCALED_CVT 3
#endif

namespace gloo_amd {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

constexpr int kMxBlock = 512;  // lanes per workgroup, as the k-source folds
constexpr bool kScaledWiden = (GLOO_MX_SCALED_CVT & 1) != 0;
constexpr bool kScaledNarrow = (GLOO_MX_SCALED_CVT & 2) != 0;

template <int FMT>
struct MxFmt {
  static constexpr bool kFp4 = FMT == GLOO_HIP_MXFP4_E2M1;
  static constexpr bool kE5M2 = FMT == GLOO_HIP_MXFP8_E5M2;
  static constexpr int kAcc = kFp4 ? 32 : 16;          // elements (f32 accumulators) per 16-byte packet
  static constexpr int kLanesPerBlock = kFp4 ? 1 : 2;  // packets per block of 32 elements
  static constexpr int kUnroll = kFp4 ? 1 : 2;         // packets per lane per tile
  static constexpr int kEmax = kFp4 ? 2 : kE5M2 ? 15 : 8;
  static constexpr float kMax = kFp4 ? 6.0f : kE5M2 ? 57344.0f : 448.0f;
  static constexpr uint32_t kNanFill = kFp4 ? 0u : 0x7F7F7F7Fu;  // e2m1 has no NaN: the scale byte alone carries it
  static constexpr uint32_t kTileBlocks = (uint32_t)kMxBlock * kUnroll / kLanesPerBlock;
  static constexpr uint32_t kTileBytes = (uint32_t)kMxBlock * kUnroll * 16;
  static constexpr uint32_t kBlkStep = kMxBlock / kLanesPerBlock;  // blocks between a lane's consecutive packets
};

struct MxSrcList {
  const void* e[GLOO_HIP_MAX_SRCS];
  const uint8_t* s[GLOO_HIP_MAX_SRCS];
};

// 2^(X - 127) as binary32; X = 255 gives +inf (see the head of mx.hip)
__device__ __forceinline__ float mx_scale(uint32_t X) {
  return __builtin_bit_cast(float, X ? X << 23 : 0x00400000u);
}

// the two elements of `w` that `SEL` names, times sc: FP8 the low (0) or high
// (1) half of the dword, FP4 the two nibbles of byte SEL (low nibble first)
template <int FMT, int SEL>
__device__ __forceinline__ f32x2 mx_widen2(uint32_t w, float sc) {
  using F = MxFmt<FMT>;
  f32x2 v;
  if constexpr (F::kFp4) {
    // gfx950 has no unscaled e2m1 convert: scale 1.0 gives the table values
    v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, kScaledWiden ? sc : 1.0f, SEL);
  } else if constexpr (kScaledWiden) {
    if constexpr (F::kE5M2) v = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(w, sc, SEL != 0);
    else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc, SEL != 0);
  } else {
    if constexpr (F::kE5M2) v = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, SEL != 0);
    else v = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, SEL != 0);
  }
  if constexpr (!kScaledWiden) {
    v.x = v.x * sc;
    v.y = v.y * sc;
  }
  return v;
}

// One packet dequantised with its block's scale byte into (FIRST) or added
// onto the packet's accumulators, in element order.
template <int FMT, bool FIRST>
__device__ __forceinline__ void mx_add_packet(u32x4 p, uint32_t X, float (&a)[MxFmt<FMT>::kAcc]) {
  using F = MxFmt<FMT>;
  constexpr int kPerDword = F::kAcc / 4;
  const float sc = mx_scale(X);
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int d = 0; d < 4; d++) {
    float v[kPerDword];
    if constexpr (F::kFp4) {
      const f32x2 b0 = mx_widen2<FMT, 0>(w[d], sc), b1 = mx_widen2<FMT, 1>(w[d], sc);
      const f32x2 b2 = mx_widen2<FMT, 2>(w[d], sc), b3 = mx_widen2<FMT, 3>(w[d], sc);
      v[0] = b0.x, v[1] = b0.y, v[2] = b1.x, v[3] = b1.y, v[4] = b2.x, v[5] = b2.y, v[6] = b3.x, v[7] = b3.y;
    } else {
      const f32x2 lo = mx_widen2<FMT, 0>(w[d], sc), hi = mx_widen2<FMT, 1>(w[d], sc);
      v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
    }
#pragma unroll
    for (int e = 0; e < kPerDword; e++) a[kPerDword * d + e] = FIRST ? v[e] : a[kPerDword * d + e] + v[e];
  }
}

// e2m1 code of a (clamped, |a * inv| <= 6) accumulator: the magnitude's code
// is rint of a map that is exact in every piece (0.5 steps below 2, 1 up to
// 4, 2 above), and an even code is an even mantissa, so rint's ties are the
// format's; the sign is the accumulator's, also on a zero.
__device__ __forceinline__ uint32_t fp4_code(float q) {
  const float m = __builtin_fabsf(q);
  const float t = m < 2.0f ? m * 2.0f : m < 4.0f ? m : m * 0.5f;
  const uint32_t off = m < 2.0f ? 0u : m < 4.0f ? 2u : 4u;
  return ((uint32_t)__builtin_rintf(t) + off) | ((__builtin_bit_cast(uint32_t, q) >> 28) & 8u);
}

// One dword of elements from its kPerDword values: divided by sc on the way
// where the converts are the scaled ones (sc is ignored otherwise).
template <int FMT>
__device__ __forceinline__ uint32_t mx_convert_dword(const float (&q)[MxFmt<FMT>::kAcc / 4], float sc) {
  using F = MxFmt<FMT>;
  constexpr int kPerDword = F::kAcc / 4;
  if constexpr (kScaledNarrow) {
    if constexpr (F::kFp4) {
      uint32_t r = 0;
      r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[0], q[1], sc, 0);
      r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[2], q[3], sc, 1);
      r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[4], q[5], sc, 2);
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[6], q[7], sc, 3);
    } else {
      i16x2 r = {0, 0};
      if constexpr (F::kE5M2) {
        r = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(r, q[0], q[1], sc, false);
        r = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(r, q[2], q[3], sc, true);
      } else {
        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, q[0], q[1], sc, false);
        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, q[2], q[3], sc, true);
      }
      return __builtin_bit_cast(uint32_t, r);
    }
  } else if constexpr (F::kFp4) {
    uint32_t r = 0;
#pragma unroll
    for (int e = 0; e < kPerDword; e++) r |= fp4_code(q[e]) << (4 * e);
    return r;
  } else if constexpr (F::kE5M2) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(q[2], q[3], __builtin_amdgcn_cvt_pk_bf8_f32(q[0], q[1], 0, false), true);
  } else {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false), true);
  }
}

// The accumulators of one packet requantised with the block's X_out.
template <int FMT>
__device__ __forceinline__ u32x4 mx_narrow_packet(const float (&a)[MxFmt<FMT>::kAcc], uint32_t Xout) {
  using F = MxFmt<FMT>;
  constexpr int kPerDword = F::kAcc / 4;
  // 2^(127 - X_out): the field 254 - X_out is never below the element emax
  const float inv = __builtin_bit_cast(float, (254u - Xout) << 23);
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    float q[kPerDword];
    if constexpr (kScaledNarrow) {
      // the convert divides by its scale operand; the clamp moves in front of it
      const float lim = F::kMax * mx_scale(Xout);
#pragma unroll
      for (int e = 0; e < kPerDword; e++) q[e] = __builtin_amdgcn_fmed3f(a[kPerDword * d + e], -lim, lim);
    } else {
#pragma unroll
      for (int e = 0; e < kPerDword; e++)
        q[e] = __builtin_amdgcn_fmed3f(a[kPerDword * d + e] * inv, -F::kMax, F::kMax);
    }
    w[d] = mx_convert_dword<FMT>(q, mx_scale(Xout));
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// MurmurHash3's finaliser
__host__ __device__ __forceinline__ uint32_t mx_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ h >> 16;
}

// K of a call's seed, computed once on the host
inline uint32_t mxSeedKey(uint64_t seed) { return mx_fmix32((uint32_t)seed) ^ (uint32_t)(seed >> 32); }

// The stochastic elements step (include/gloo_amd.h "MX stochastic rounding")
// on the binary32 bits of one clamped q: the on-grid value it stores.  The
// significand, implicit bit in front, is shifted down until 16 bits stay below
// the element's grid unit: 7 - M bits from the element's smallest normal
// binade up, one more per binade below it, and for 24 or more nothing is left
// (an f32 denormal's false implicit bit included).  What stays is the
// truncated magnitude t in grid units above frac16, so the 16 random bits
// added to it carry into t exactly when frac16 + R16 >= 2^16, and t times the
// unit is exact: t = 2^(M + 1) is the next binade's first value.
template <int FMT>
__device__ __forceinline__ float mx_sr_element(float q, uint32_t r16) {
  using F = MxFmt<FMT>;
  constexpr uint32_t M = F::kFp4 ? 1 : F::kE5M2 ? 2 : 3;                 // mantissa bits
  constexpr uint32_t kMinNormal = F::kFp4 ? 127 : F::kE5M2 ? 113 : 121;  // f32 exponent field of the smallest normal
  const uint32_t bits = __builtin_bit_cast(uint32_t, q), E = (bits >> 23) & 0xFFu;
  const uint32_t binade = E > kMinNormal ? E : kMinNormal;
  const uint32_t shift = binade - E + (7 - M);
  const uint32_t sig = (bits & 0x007FFFFFu) | 0x00800000u;
  const uint32_t t = ((sig >> (shift < 24 ? shift : 24)) + r16) >> 16;
  const float mag = (float)t * __builtin_bit_cast(float, (binade - M) << 23);
  return __builtin_copysignf(mag, q);
}

// mx_narrow_packet with stochastic rounding: `first` is the global index of
// a[0], a multiple of the number of accumulators in use (8 or the packet's),
// so the packet's pairs share the high word of their index; key is the host's
// K.  One hash serves two neighbouring elements.  The values handed to the
// converts are on the element grid already: scale 1, and no rounding is left.
template <int FMT>
__device__ __forceinline__ u32x4 mx_narrow_packet_sr(const float (&a)[MxFmt<FMT>::kAcc], uint32_t Xout, size_t first,
                                                     uint32_t key) {
  using F = MxFmt<FMT>;
  constexpr int kPerDword = F::kAcc / 4;
  const float inv = __builtin_bit_cast(float, (254u - Xout) << 23);
  const uint32_t pair0 = (uint32_t)(first >> 1), high = 0x9E3779B9u * (uint32_t)(first >> 33);
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    float q[kPerDword];
#pragma unroll
    for (int e = 0; e < kPerDword; e += 2) {
      const uint32_t W = mx_fmix32(((pair0 + (uint32_t)(kPerDword * d + e) / 2) ^ key) + high);
      q[e] = mx_sr_element<FMT>(__builtin_amdgcn_fmed3f(a[kPerDword * d + e] * inv, -F::kMax, F::kMax), W & 0xFFFFu);
      q[e + 1] = mx_sr_element<FMT>(__builtin_amdgcn_fmed3f(a[kPerDword * d + e + 1] * inv, -F::kMax, F::kMax), W >> 16);
    }
    w[d] = mx_convert_dword<FMT>(q, 1.0f);
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// One source's packets of the tile and their blocks' scale bytes, requested.
template <int FMT>
__device__ __forceinline__ void mx_request(const void* elems, const uint8_t* scales, size_t base, uint32_t bytes,
                                           size_t block0, uint32_t blocks, u32x4 (&v)[MxFmt<FMT>::kUnroll],
                                           uint32_t (&x)[MxFmt<FMT>::kUnroll]) {
  using F = MxFmt<FMT>;
  const auto re = make_rsrc(static_cast<const char*>(elems) + base, bytes);
  const auto rs = make_rsrc(scales + block0, blocks);
  const uint32_t lane_off = threadIdx.x * 16u, lane_blk = threadIdx.x / F::kLanesPerBlock;
#pragma unroll
  for (int u = 0; u < F::kUnroll; u++) v[u] = bload<kAuxNT>(re, lane_off + u * kMxBlock * 16);
#pragma unroll
  for (int u = 0; u < F::kUnroll; u++) x[u] = __builtin_amdgcn_raw_buffer_load_b8(rs, lane_blk + u * F::kBlkStep, 0, 0);
}

}  // namespace
}  // namespace gloo_amd

// mx.hip — block-scaled (OCP Microscaling) k-source sum for gfx950.
//
// dst = requantise(sum_j dequantise(src_j)) over k <= 8 sources of MXFP8
// (e4m3 / e5m2 elements) or MXFP4 (e2m1, two per byte), every block of 32
// elements carrying one E8M0 scale byte; the contract is include/gloo_amd.h
// "MX block-scaled sum".  One pass: every source byte is read once, every
// result byte written once, nothing is staged in a wider type in memory.
//
// Work split.  A workgroup owns one tile of kMxBlock lanes x UNROLL 16-byte
// packets, as the k-source folds of reduce.hip do; packet u of lane t sits at
// (t + u * kMxBlock) * 16 bytes into the tile, so a wave instruction covers
// 1 KiB contiguous, and the last tile is clipped by the descriptors' byte
// bounds (loads return 0, stores are dropped), never by a lane branch.
//   MXFP8: a block is two packets, so lanes 2m and 2m + 1 hold block m of the
//     tile (16 f32 accumulators per packet each) and meet once, after the last
//     source, to agree on the block's amax: one DPP quad permute, no LDS.
//   MXFP4: a block is one packet, so a lane holds a whole block (32 f32
//     accumulators per packet) and needs no cross-lane step; UNROLL is 1
//     there, which keeps the accumulators of ONE packet live per lane.
// Source j + 1's packets and scale bytes are requested before source j's are
// dequantised and added (wide_tile's order): two sources in flight per lane.
//
// Arithmetic.  The model is one v_mul_f32 by the block scale 2^(X - 127) per
// element, one v_add_f32 per source, and after the last source amax, X_out,
// one v_mul_f32 by 2^(127 - X_out), a clamp and the narrowing; contraction is
// off for the whole file, packed f32 arithmetic for the kernel.  gfx950's
// scaled converts carry both multiplies (GLOO_MX_SCALED_CVT, a build-time bit
// mask, default 3): bit 0 dequantises with v_cvt_scalef32_pk_f32_{fp8,bf8,fp4}
// (the scale operand is 2^(X - 127) built from the scale byte's bits; X = 0:
// the denormal 0x00400000; X = 255: +inf, so that every element of such a
// source is inf or NaN and the block is found non-finite below); bit 1
// requantises with v_cvt_scalef32_pk_{fp8,bf8,fp4}_f32, which divide by their
// scale operand, behind a v_med3_f32 clamp to +-max normal * 2^(X_out - 127)
// (the converts' own overflow behaviour is never relied on).  Each bit was
// compared with the plain form (bit clear: unscaled convert, v_mul_f32, clamp,
// unscaled narrowing; e2m1 narrowed by fp4_code) and with the model on an
// MI355X over the whole scale range, denormal products, scale 0 and f32
// overflow included: the same bytes.  amax is the unsigned
// maximum of the accumulators' magnitude bits, so one compare against
// 0x7F800000 finds any inf or NaN of the block.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <string>

#include "buffer_rsrc.h"
#include "gloo_amd.h"
#include "gloo_amd/errors.h"

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

// 2^(X - 127) as binary32; X = 255 gives +inf (see the head of the file)
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
      const float sc = mx_scale(Xout);
      if constexpr (F::kFp4) {
        uint32_t r = 0;
        r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[0], q[1], sc, 0);
        r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[2], q[3], sc, 1);
        r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[4], q[5], sc, 2);
        w[d] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, q[6], q[7], sc, 3);
      } else {
        i16x2 r = {0, 0};
        if constexpr (F::kE5M2) {
          r = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(r, q[0], q[1], sc, false);
          r = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(r, q[2], q[3], sc, true);
        } else {
          r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, q[0], q[1], sc, false);
          r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, q[2], q[3], sc, true);
        }
        w[d] = __builtin_bit_cast(uint32_t, r);
      }
    } else {
#pragma unroll
      for (int e = 0; e < kPerDword; e++)
        q[e] = __builtin_amdgcn_fmed3f(a[kPerDword * d + e] * inv, -F::kMax, F::kMax);
      if constexpr (F::kFp4) {
        uint32_t r = 0;
#pragma unroll
        for (int e = 0; e < kPerDword; e++) r |= fp4_code(q[e]) << (4 * e);
        w[d] = r;
      } else if constexpr (F::kE5M2) {
        w[d] = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(q[2], q[3], __builtin_amdgcn_cvt_pk_bf8_f32(q[0], q[1], 0, false),
                                                         true);
      } else {
        w[d] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false),
                                                         true);
      }
    }
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

template <int FMT>
__global__ __launch_bounds__(kMxBlock) GLOO_WIDE_KERNEL void mx_fold_kernel(void* dstE, uint8_t* dstS, MxSrcList srcs,
                                                                             int k, size_t nblocks) {
  using F = MxFmt<FMT>;
  constexpr int U = F::kUnroll;
  const size_t block0 = (size_t)blockIdx.x * F::kTileBlocks;
  if (block0 >= nblocks) return;
  const uint32_t blocks = (uint32_t)((nblocks - block0) < F::kTileBlocks ? (nblocks - block0) : F::kTileBlocks);
  const uint32_t bytes = blocks * (16u * F::kLanesPerBlock);
  const size_t base = (size_t)blockIdx.x * F::kTileBytes;
  const uint32_t lane_off = threadIdx.x * 16u;
  const uint32_t lane_blk = threadIdx.x / F::kLanesPerBlock;  // the lane's block of the tile, packet 0
  constexpr uint32_t kBlkStep = MxFmt<FMT>::kBlkStep;          // ... and its step per packet

  float a[U][F::kAcc];
  u32x4 cur[U], nxt[U];
  uint32_t curX[U], nxtX[U];
  mx_request<FMT>(srcs.e[0], srcs.s[0], base, bytes, block0, blocks, cur, curX);
  if (k > 1) mx_request<FMT>(srcs.e[1], srcs.s[1], base, bytes, block0, blocks, nxt, nxtX);
#pragma unroll
  for (int u = 0; u < U; u++) mx_add_packet<FMT, true>(cur[u], curX[u], a[u]);
  for (int j = 1; j < k; j++) {
#pragma unroll
    for (int u = 0; u < U; u++) cur[u] = nxt[u], curX[u] = nxtX[u];
    if (j + 1 < k)  // in flight while source j is dequantised and added
      mx_request<FMT>(srcs.e[j + 1], srcs.s[j + 1], base, bytes, block0, blocks, nxt, nxtX);
#pragma unroll
    for (int u = 0; u < U; u++) mx_add_packet<FMT, false>(cur[u], curX[u], a[u]);
  }

  const auto rd = make_rsrc(static_cast<const char*>(dstE) + base, bytes);
  const auto rx = make_rsrc(dstS + block0, blocks);
#pragma unroll
  for (int u = 0; u < U; u++) {
    // amax on the magnitude bits: an inf or NaN accumulator is the maximum
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < F::kAcc; i++) {
      const uint32_t mag = __builtin_bit_cast(uint32_t, a[u][i]) & 0x7FFFFFFFu;
      m = mag > m ? mag : m;
    }
    if constexpr (F::kLanesPerBlock == 2) {
      // the block's other half sits in lane ^ 1: quad_perm [1, 0, 3, 2]
      const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);
      m = o > m ? o : m;
    }
    const bool finite = m < 0x7F800000u;
    const uint32_t f = m >> 23;  // 0 for zero and denormals
    const uint32_t Xfin = f > (uint32_t)F::kEmax ? f - (uint32_t)F::kEmax : 0u;
    u32x4 out = mx_narrow_packet<FMT>(a[u], finite ? Xfin : 0u);
    if (!finite) out = u32x4{F::kNanFill, F::kNanFill, F::kNanFill, F::kNanFill};
    bstore<kAuxNT>(rd, lane_off + u * kMxBlock * 16, out);
    if (F::kLanesPerBlock == 1 || (threadIdx.x & 1) == 0)
      __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(finite ? Xfin : 255u), rx, lane_blk + u * kBlkStep, 0, 0);
  }
}

int mxError(int code, const std::string& msg) { return setError(code, "reduce_mx: " + msg); }

std::string hex(const void* p) {
  char buf[32];
  snprintf(buf, sizeof(buf), "%p", p);
  return buf;
}

struct Range {
  uintptr_t lo, hi;
  std::string name;
};
bool overlap(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }

template <int FMT>
int launchMx(void* dstE, uint8_t* dstS, const MxSrcList& list, int k, size_t nblocks, hipStream_t s) {
  const size_t grid = (nblocks + MxFmt<FMT>::kTileBlocks - 1) / MxFmt<FMT>::kTileBlocks;
  if (grid > 0x7FFFFFFFu) return mxError(GLOO_HIP_EINVAL_ARG, "nblocks " + std::to_string(nblocks) + " is too large for one launch");
  mx_fold_kernel<FMT><<<dim3((unsigned)grid), dim3(kMxBlock), 0, s>>>(dstE, dstS, list, k, nblocks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return setError((int)e, std::string("mx_fold_kernel: ") + hipGetErrorString(e));
  return GLOO_HIP_OK;
}

}  // namespace
}  // namespace gloo_amd

extern "C" {

int gloo_hip_mx_supported(int fmt) { return fmt >= GLOO_HIP_MXFP8_E4M3 && fmt <= GLOO_HIP_MXFP4_E2M1 ? 1 : 0; }

size_t gloo_hip_mx_tile_blocks(int fmt) {
  switch (fmt) {
    case GLOO_HIP_MXFP8_E4M3: return gloo_amd::MxFmt<GLOO_HIP_MXFP8_E4M3>::kTileBlocks;
    case GLOO_HIP_MXFP8_E5M2: return gloo_amd::MxFmt<GLOO_HIP_MXFP8_E5M2>::kTileBlocks;
    case GLOO_HIP_MXFP4_E2M1: return gloo_amd::MxFmt<GLOO_HIP_MXFP4_E2M1>::kTileBlocks;
    default: return 0;
  }
}

int gloo_hip_reduce_mx(int fmt, void* dst_elems, uint8_t* dst_scales, const void* const* src_elems,
                       const uint8_t* const* src_scales, int k, size_t nblocks, gloo_hip_stream_t stream) {
  using namespace gloo_amd;
  if (!gloo_hip_mx_supported(fmt)) return mxError(GLOO_HIP_EINVAL_DTYPE, "unknown MX format " + std::to_string(fmt));
  if (k < 1 || k > GLOO_HIP_MAX_SRCS)
    return mxError(GLOO_HIP_EINVAL_ARG, "source count " + std::to_string(k) + " is outside 1.." + std::to_string(GLOO_HIP_MAX_SRCS));
  if (nblocks == 0) return GLOO_HIP_OK;
  if (!dst_elems) return mxError(GLOO_HIP_EINVAL_PTR, "dst_elems is null");
  if (!dst_scales) return mxError(GLOO_HIP_EINVAL_PTR, "dst_scales is null");
  if (!src_elems) return mxError(GLOO_HIP_EINVAL_PTR, "src_elems is null");
  if (!src_scales) return mxError(GLOO_HIP_EINVAL_PTR, "src_scales is null");
  if ((uintptr_t)dst_elems % 16) return mxError(GLOO_HIP_EINVAL_PTR, "dst_elems " + hex(dst_elems) + " is not 16-byte aligned");
  const size_t ebytes = nblocks * (fmt == GLOO_HIP_MXFP4_E2M1 ? 16 : 32);
  MxSrcList list = {};
  for (int j = 0; j < k; j++) {
    const std::string ej = "src_elems[" + std::to_string(j) + "]", sj = "src_scales[" + std::to_string(j) + "]";
    if (!src_elems[j]) return mxError(GLOO_HIP_EINVAL_PTR, ej + " is null");
    if (!src_scales[j]) return mxError(GLOO_HIP_EINVAL_PTR, sj + " is null");
    if ((uintptr_t)src_elems[j] % 16) return mxError(GLOO_HIP_EINVAL_PTR, ej + " " + hex(src_elems[j]) + " is not 16-byte aligned");
    list.e[j] = src_elems[j];
    list.s[j] = src_scales[j];
  }
  // the destination arrays may BE source 0's (in place); any other shared byte is refused
  const Range dst[2] = {{(uintptr_t)dst_elems, (uintptr_t)dst_elems + ebytes, "dst_elems"},
                        {(uintptr_t)dst_scales, (uintptr_t)dst_scales + nblocks, "dst_scales"}};
  if (overlap(dst[0], dst[1])) return mxError(GLOO_HIP_EINVAL_ARG, "dst_elems " + hex(dst_elems) + " overlaps dst_scales");
  for (int j = 0; j < k; j++) {
    const Range src[2] = {{(uintptr_t)src_elems[j], (uintptr_t)src_elems[j] + ebytes, "src_elems[" + std::to_string(j) + "]"},
                          {(uintptr_t)src_scales[j], (uintptr_t)src_scales[j] + nblocks, "src_scales[" + std::to_string(j) + "]"}};
    for (int d = 0; d < 2; d++)
      for (int t = 0; t < 2; t++) {
        const bool inPlace = j == 0 && d == t && dst[d].lo == src[t].lo;
        if (!inPlace && overlap(dst[d], src[t]))
          return mxError(GLOO_HIP_EINVAL_ARG, dst[d].name + " " + hex((const void*)dst[d].lo) + " overlaps " + src[t].name);
      }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (fmt) {
    case GLOO_HIP_MXFP8_E4M3: return launchMx<GLOO_HIP_MXFP8_E4M3>(dst_elems, dst_scales, list, k, nblocks, s);
    case GLOO_HIP_MXFP8_E5M2: return launchMx<GLOO_HIP_MXFP8_E5M2>(dst_elems, dst_scales, list, k, nblocks, s);
    default: return launchMx<GLOO_HIP_MXFP4_E2M1>(dst_elems, dst_scales, list, k, nblocks, s);
  }
}

}  // extern "C"

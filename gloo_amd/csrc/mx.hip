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
//
// Rounding mode.  mx_fold_kernel<FMT, SR>: SR = false is the above; SR = true
// (gloo_hip_reduce_mx_sr, "MX stochastic rounding") narrows with
// mx_narrow_packet_sr of mx_common.h from the packet's first element index and
// the seed's key, the one argument only that instantiation reads.  Everything
// in front of the narrowing is shared.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <string>

#include "buffer_rsrc.h"
#include "gloo_amd.h"
#include "gloo_amd/errors.h"
#include "mx_common.h"

#pragma clang fp contract(off)

namespace gloo_amd {
namespace {

template <int FMT, bool SR>
__global__ __launch_bounds__(kMxBlock) GLOO_WIDE_KERNEL void mx_fold_kernel(void* dstE, uint8_t* dstS, MxSrcList srcs,
                                                                             int k, size_t nblocks, uint32_t key) {
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
    u32x4 out;
    if constexpr (SR) {  // key is read here only; the packet's first element of the whole tensor
      const size_t pkt = (size_t)blockIdx.x * (kMxBlock * U) + threadIdx.x + u * kMxBlock;
      out = mx_narrow_packet_sr<FMT>(a[u], finite ? Xfin : 0u, pkt * F::kAcc, key);
    } else {
      out = mx_narrow_packet<FMT>(a[u], finite ? Xfin : 0u);
    }
    if (!finite) out = u32x4{F::kNanFill, F::kNanFill, F::kNanFill, F::kNanFill};
    bstore<kAuxNT>(rd, lane_off + u * kMxBlock * 16, out);
    if (F::kLanesPerBlock == 1 || (threadIdx.x & 1) == 0)
      __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(finite ? Xfin : 255u), rx, lane_blk + u * kBlkStep, 0, 0);
  }
}


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
int launchMx(const std::string& fn, void* dstE, uint8_t* dstS, const MxSrcList& list, int k, size_t nblocks, const uint64_t* seed,
             hipStream_t s) {
  const size_t grid = (nblocks + MxFmt<FMT>::kTileBlocks - 1) / MxFmt<FMT>::kTileBlocks;
  if (grid > 0x7FFFFFFFu)
    return setError(GLOO_HIP_EINVAL_ARG, fn + ": nblocks " + std::to_string(nblocks) + " is too large for one launch");
  const dim3 g((unsigned)grid), b(kMxBlock);
  if (seed) mx_fold_kernel<FMT, true><<<g, b, 0, s>>>(dstE, dstS, list, k, nblocks, mxSeedKey(*seed));
  else mx_fold_kernel<FMT, false><<<g, b, 0, s>>>(dstE, dstS, list, k, nblocks, 0u);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return setError((int)e, std::string("mx_fold_kernel: ") + hipGetErrorString(e));
  return GLOO_HIP_OK;
}

// both rounding modes of the sum: `seed` is null for round to nearest even
int reduceMx(const std::string& fn, int fmt, void* dst_elems, uint8_t* dst_scales, const void* const* src_elems,
             const uint8_t* const* src_scales, int k, size_t nblocks, const uint64_t* seed, gloo_hip_stream_t stream) {
  auto mxError = [&](int code, const std::string& msg) { return setError(code, fn + ": " + msg); };
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
    case GLOO_HIP_MXFP8_E4M3: return launchMx<GLOO_HIP_MXFP8_E4M3>(fn, dst_elems, dst_scales, list, k, nblocks, seed, s);
    case GLOO_HIP_MXFP8_E5M2: return launchMx<GLOO_HIP_MXFP8_E5M2>(fn, dst_elems, dst_scales, list, k, nblocks, seed, s);
    default: return launchMx<GLOO_HIP_MXFP4_E2M1>(fn, dst_elems, dst_scales, list, k, nblocks, seed, s);
  }
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
  return gloo_amd::reduceMx("reduce_mx", fmt, dst_elems, dst_scales, src_elems, src_scales, k, nblocks, nullptr, stream);
}

int gloo_hip_reduce_mx_sr(int fmt, void* dst_elems, uint8_t* dst_scales, const void* const* src_elems,
                          const uint8_t* const* src_scales, int k, size_t nblocks, uint64_t seed, gloo_hip_stream_t stream) {
  return gloo_amd::reduceMx("reduce_mx_sr", fmt, dst_elems, dst_scales, src_elems, src_scales, k, nblocks, &seed, stream);
}

}  // extern "C"

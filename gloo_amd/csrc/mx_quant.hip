// mx_quant.hip — the two ends of the MX (OCP Microscaling) path for gfx950:
// a wide-to-MX quantise and a wide-output MX fold, for f32, f16 and bf16.  The
// contract is include/gloo_amd.h "MX quantise and wide-output fold"; formats,
// blocks, scales and nibble order are the MX block-scaled sum's (mx.hip), and
// so are the device helpers of mx_common.h.
//
// mx_quantise_kernel<FMT, DTYPE, SR>: (elements, E8M0 scales) = quantise(wide src).
//   Traffic per block: 128 (f32) or 64 bytes read, 32 (FP8) or 16 (FP4) + 1
//   written.  A lane owns 8 consecutive elements of a row: one b128 load for
//   f16 / bf16, two adjacent ones for f32.  Four lanes are a block, and blocks
//   coincide with DPP quads, so the block's amax, taken on magnitude bits as
//   in mx.hip (one compare finds inf or NaN), is two quad permutes and no LDS.
//   Each lane narrows its 8 values with mx_narrow_packet's arithmetic (the
//   scaled converts behind the v_med3_f32 clamp) and stores 8 (FP8) or 4 (FP4)
//   bytes: a wave's store is 512 or 256 contiguous bytes; lane 0 of the quad
//   stores the scale byte.  A workgroup owns a tile of kQRows rows of kMxBlock
//   lanes, row r of lane t at element (t + r * kMxBlock) * 8; all rows are
//   loaded before the first is consumed.  The last tile is clipped by the
//   descriptors' byte bounds (whole blocks), never by a lane branch.
//   The widening goes through f32 for every dtype (exact: bits, a shift, or
//   v_cvt_f32_f16, denormals included); gfx950's direct
//   v_cvt_scalef32_pk_{fp8,bf8,fp4}_{f16,bf16} converts are not used.
//   The third template parameter is the rounding mode: SR = true
//   (gloo_hip_quantise_mx_sr) narrows with mx_narrow_packet_sr from the row's
//   first element index and the seed's key, which only it reads.
//
// mx_fold_wide_kernel<FMT, DTYPE>: dst = narrow_dtype(sum_j dequantise(src_j)).
//   The source side is mx_fold_kernel's: the same tile, packets, accumulator
//   layout and request order (source j + 1 in flight while source j is
//   dequantised and added).  No amax, no cross-lane arithmetic.  A scale byte
//   of 255 is carried as a flag per packet, because element * inf is inf, not
//   NaN, for non-zero elements.  A lane's 16 (FP8) or 32 (FP4) accumulators
//   are 32 to 128 contiguous bytes of the wide dtype, so per-lane b128 stores
//   would put a wave instruction's lanes 32 to 128 bytes apart.  Instead each
//   wave turns its quads through LDS (2 to 8 KiB per wave and packet; no
//   workgroup barrier: the exchange never leaves the wave), so that every b128
//   store instruction covers 1 KiB contiguous.  The per-lane form was measured
//   beside this one and is 1.1x to 7x slower.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <type_traits>

#include "buffer_rsrc.h"
#include "gloo_amd.h"
#include "gloo_amd/errors.h"
#include "mx_common.h"

#pragma clang fp contract(off)

namespace gloo_amd {
namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kQRows = 4;                                      // rows of 8 elements per lane and tile
constexpr uint32_t kQTileBlocks = kMxBlock * kQRows / 4;       // four lanes per block
constexpr uint32_t kQuietNaN = 0x7FC00000u;

template <int DTYPE>
struct MxWide {
  static constexpr bool kF32 = DTYPE == GLOO_HIP_F32;
  static constexpr uint32_t kSize = kF32 ? 4 : 2;
  static constexpr int kLoads = kF32 ? 2 : 1;  // b128 loads per 8 elements

  // element e (0 or 1) of a dword of two 16-bit elements, widened exactly
  __device__ static __forceinline__ float widen16(uint32_t w, int e) {
    if constexpr (DTYPE == GLOO_HIP_BF16) return __builtin_bit_cast(float, e ? w & 0xFFFF0000u : w << 16);
    else return (float)__builtin_bit_cast(_Float16, (uint16_t)(e ? w >> 16 : w));
  }
  // the contract's single narrowing; every NaN becomes the dtype's canonical quiet NaN
  __device__ static __forceinline__ uint32_t narrow(float a) {
    if constexpr (kF32) return a != a ? kQuietNaN : __builtin_bit_cast(uint32_t, a);
    else if constexpr (DTYPE == GLOO_HIP_BF16) return a != a ? 0x7FC0u : __builtin_bit_cast(uint16_t, (__bf16)a);
    else return a != a ? 0x7E00u : __builtin_bit_cast(uint16_t, (_Float16)a);
  }
};

template <int FMT, int DTYPE, bool SR>
__global__ __launch_bounds__(kMxBlock) GLOO_WIDE_KERNEL void mx_quantise_kernel(void* dstE, uint8_t* dstS, const void* src,
                                                                                 size_t nblocks, uint32_t key) {
  using F = MxFmt<FMT>;
  using W = MxWide<DTYPE>;
  constexpr uint32_t kOut = F::kFp4 ? 4 : 8;      // element bytes a lane stores per row
  constexpr uint32_t kIn = 8 * W::kSize;          // wide bytes a lane loads per row
  const size_t block0 = (size_t)blockIdx.x * kQTileBlocks;
  if (block0 >= nblocks) return;
  const uint32_t blocks = (uint32_t)((nblocks - block0) < kQTileBlocks ? (nblocks - block0) : kQTileBlocks);
  const auto rs = make_rsrc(static_cast<const char*>(src) + block0 * (4 * kIn), blocks * (4 * kIn));
  const auto rd = make_rsrc(static_cast<char*>(dstE) + block0 * (4 * kOut), blocks * (4 * kOut));
  const auto rx = make_rsrc(dstS + block0, blocks);

  u32x4 v[kQRows][W::kLoads];
#pragma unroll
  for (int r = 0; r < kQRows; r++)
#pragma unroll
    for (int h = 0; h < W::kLoads; h++) v[r][h] = bload<kAuxNT>(rs, (threadIdx.x + r * kMxBlock) * kIn + h * 16);

#pragma unroll
  for (int r = 0; r < kQRows; r++) {
    float q[F::kAcc] = {};  // the lane's 8 values in front of a packet of zeros: the unused dwords fold away
    if constexpr (W::kF32) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t w[4] = {v[r][h].x, v[r][h].y, v[r][h].z, v[r][h].w};
#pragma unroll
        for (int d = 0; d < 4; d++) q[4 * h + d] = __builtin_bit_cast(float, w[d]);
      }
    } else {
      const uint32_t w[4] = {v[r][0].x, v[r][0].y, v[r][0].z, v[r][0].w};
#pragma unroll
      for (int d = 0; d < 4; d++) q[2 * d] = W::widen16(w[d], 0), q[2 * d + 1] = W::widen16(w[d], 1);
    }
    // amax on the magnitude bits, then across the quad: [1, 0, 3, 2] and [2, 3, 0, 1]
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t mag = __builtin_bit_cast(uint32_t, q[i]) & 0x7FFFFFFFu;
      m = mag > m ? mag : m;
    }
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);
    m = o > m ? o : m;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true);
    m = o > m ? o : m;
    const bool finite = m < 0x7F800000u;
    const uint32_t f = m >> 23;  // 0 for zero and denormals
    const uint32_t Xfin = f > (uint32_t)F::kEmax ? f - (uint32_t)F::kEmax : 0u;
    u32x4 out;
    if constexpr (SR)  // key is read here only; the row's first element of the whole tensor
      out = mx_narrow_packet_sr<FMT>(q, finite ? Xfin : 0u, (block0 * 4 + threadIdx.x + r * kMxBlock) * 8, key);
    else out = mx_narrow_packet<FMT>(q, finite ? Xfin : 0u);
    if (!finite) out.x = F::kNanFill, out.y = F::kNanFill;
    const uint32_t row = threadIdx.x + r * kMxBlock;
    if constexpr (F::kFp4) __builtin_amdgcn_raw_buffer_store_b32(out.x, rd, row * kOut, 0, kAuxNT);
    else __builtin_amdgcn_raw_buffer_store_b64(u32x2{out.x, out.y}, rd, row * kOut, 0, kAuxNT);
    if ((threadIdx.x & 3) == 0) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(finite ? Xfin : 255u), rx, row >> 2, 0, 0);
  }
}

template <int FMT, int DTYPE>
__global__ __launch_bounds__(kMxBlock) GLOO_WIDE_KERNEL void mx_fold_wide_kernel(void* dst, MxSrcList srcs, int k,
                                                                                  size_t nblocks) {
  using F = MxFmt<FMT>;
  using W = MxWide<DTYPE>;
  constexpr int U = F::kUnroll;
  constexpr int kQuads = F::kAcc * (int)W::kSize / 16;  // b128 stores per packet: 2, 4 or 8
  const size_t block0 = (size_t)blockIdx.x * F::kTileBlocks;
  if (block0 >= nblocks) return;
  const uint32_t blocks = (uint32_t)((nblocks - block0) < F::kTileBlocks ? (nblocks - block0) : F::kTileBlocks);
  const uint32_t bytes = blocks * (16u * F::kLanesPerBlock);
  const size_t base = (size_t)blockIdx.x * F::kTileBytes;

  float a[U][F::kAcc];
  u32x4 cur[U], nxt[U];
  uint32_t curX[U], nxtX[U];
  bool nan[U];  // some source's scale byte for the packet's block was 255
  mx_request<FMT>(srcs.e[0], srcs.s[0], base, bytes, block0, blocks, cur, curX);
  if (k > 1) mx_request<FMT>(srcs.e[1], srcs.s[1], base, bytes, block0, blocks, nxt, nxtX);
#pragma unroll
  for (int u = 0; u < U; u++) mx_add_packet<FMT, true>(cur[u], curX[u], a[u]), nan[u] = curX[u] == 255u;
  for (int j = 1; j < k; j++) {
#pragma unroll
    for (int u = 0; u < U; u++) cur[u] = nxt[u], curX[u] = nxtX[u];
    if (j + 1 < k)  // in flight while source j is dequantised and added
      mx_request<FMT>(srcs.e[j + 1], srcs.s[j + 1], base, bytes, block0, blocks, nxt, nxtX);
#pragma unroll
    for (int u = 0; u < U; u++) mx_add_packet<FMT, false>(cur[u], curX[u], a[u]), nan[u] |= curX[u] == 255u;
  }

  const auto rd = make_rsrc(static_cast<char*>(dst) + block0 * (32 * W::kSize), blocks * (32 * W::kSize));
  __shared__ u32x4 turn[kMxBlock / 64][64 * kQuads];  // per wave: one packet of each lane
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int u = 0; u < U; u++) {
    u32x4 out[kQuads];
#pragma unroll
    for (int e = 0; e < F::kAcc; e++) a[u][e] = nan[u] ? __builtin_bit_cast(float, kQuietNaN) : a[u][e];
#pragma unroll
    for (int i = 0; i < kQuads; i++) {
      uint32_t w[4];
#pragma unroll
      for (int d = 0; d < 4; d++) {
        if constexpr (W::kF32) w[d] = W::narrow(a[u][4 * i + d]);
        else w[d] = W::narrow(a[u][8 * i + 2 * d]) | W::narrow(a[u][8 * i + 2 * d + 1]) << 16;
      }
      out[i] = u32x4{w[0], w[1], w[2], w[3]};
    }
    const uint32_t pkt = threadIdx.x + u * kMxBlock;  // the lane's packet of the tile: kQuads * 16 wide bytes
    // lane l's quads i sit at l * kQuads + i; quad q of the wave's packets goes out from lane q % 64
    if (u > 0) __builtin_amdgcn_wave_barrier();  // packet u - 1 has been read back
#pragma unroll
    for (int i = 0; i < kQuads; i++) turn[wave][lane * kQuads + i] = out[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < kQuads; i++)
      bstore<kAuxNT>(rd, ((pkt - lane) * kQuads + i * 64 + lane) * 16, turn[wave][i * 64 + lane]);
  }
}

std::string hex(const void* p) {
  char buf[32];
  snprintf(buf, sizeof(buf), "%p", p);
  return buf;
}

struct Range {
  const char* name;
  std::string index;  // "[j]" for a source of a list
  const void* p;
  size_t bytes;
  bool wide;  // element and wide arrays are 16-byte aligned, scale arrays start anywhere
};

// The checks both entry points share, in gloo_hip_reduce_mx's order: nulls,
// alignment, then any byte shared between a destination and a source array.
int checkRanges(const std::string& fn, const Range* dst, int ndst, const Range* src, int nsrc) {
  auto fail = [&](int code, const std::string& msg) { return setError(code, fn + ": " + msg); };
  for (const Range* set : {dst, src})
    for (int i = 0; i < (set == dst ? ndst : nsrc); i++) {
      const Range& r = set[i];
      if (!r.p) return fail(GLOO_HIP_EINVAL_PTR, r.name + r.index + " is null");
      if (r.wide && (uintptr_t)r.p % 16) return fail(GLOO_HIP_EINVAL_PTR, r.name + r.index + " " + hex(r.p) + " is not 16-byte aligned");
    }
  auto overlap = [](const Range& x, const Range& y) {
    return (uintptr_t)x.p < (uintptr_t)y.p + y.bytes && (uintptr_t)y.p < (uintptr_t)x.p + x.bytes;
  };
  for (int d = 0; d < ndst; d++) {
    for (int e = d + 1; e < ndst; e++)
      if (overlap(dst[d], dst[e])) return fail(GLOO_HIP_EINVAL_ARG, std::string(dst[d].name) + " " + hex(dst[d].p) + " overlaps " + dst[e].name);
    for (int s = 0; s < nsrc; s++)
      if (overlap(dst[d], src[s]))
        return fail(GLOO_HIP_EINVAL_ARG, std::string(dst[d].name) + " " + hex(dst[d].p) + " overlaps " + src[s].name + src[s].index);
  }
  return GLOO_HIP_OK;
}

bool wideDtype(int dtype) { return dtype == GLOO_HIP_F32 || dtype == GLOO_HIP_F16 || dtype == GLOO_HIP_BF16; }

// f(format, dtype) with both as compile-time constants; the caller has checked them
template <typename Fn>
int withFormatAndDtype(int fmt, int dtype, Fn&& f) {
  auto withDtype = [&](auto F) {
    switch (dtype) {
      case GLOO_HIP_F32: return f(F, std::integral_constant<int, GLOO_HIP_F32>{});
      case GLOO_HIP_F16: return f(F, std::integral_constant<int, GLOO_HIP_F16>{});
      default: return f(F, std::integral_constant<int, GLOO_HIP_BF16>{});
    }
  };
  switch (fmt) {
    case GLOO_HIP_MXFP8_E4M3: return withDtype(std::integral_constant<int, GLOO_HIP_MXFP8_E4M3>{});
    case GLOO_HIP_MXFP8_E5M2: return withDtype(std::integral_constant<int, GLOO_HIP_MXFP8_E5M2>{});
    default: return withDtype(std::integral_constant<int, GLOO_HIP_MXFP4_E2M1>{});
  }
}

int checkFormatAndDtype(const std::string& fn, int fmt, int dtype) {
  if (!gloo_hip_mx_supported(fmt)) return setError(GLOO_HIP_EINVAL_DTYPE, fn + ": unknown MX format " + std::to_string(fmt));
  if (!wideDtype(dtype)) return setError(GLOO_HIP_EINVAL_DTYPE, fn + ": dtype " + std::to_string(dtype) + " is not f32, f16 or bf16");
  return GLOO_HIP_OK;
}

int checkGrid(const std::string& fn, size_t grid, size_t nblocks) {
  if (grid <= 0x7FFFFFFFu) return GLOO_HIP_OK;
  return setError(GLOO_HIP_EINVAL_ARG, fn + ": nblocks " + std::to_string(nblocks) + " is too large for one launch");
}

int launchStatus(const char* kernel) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? GLOO_HIP_OK : setError((int)e, std::string(kernel) + ": " + hipGetErrorString(e));
}

// both rounding modes of the quantise: `seed` is null for round to nearest even
int quantiseMx(const std::string& fn, int fmt, int dtype, void* dst_elems, uint8_t* dst_scales, const void* src, size_t nblocks,
               const uint64_t* seed, gloo_hip_stream_t stream) {
  if (const int rc = checkFormatAndDtype(fn, fmt, dtype)) return rc;
  if (nblocks == 0) return GLOO_HIP_OK;
  const size_t ebytes = nblocks * (fmt == GLOO_HIP_MXFP4_E2M1 ? 16 : 32), wbytes = nblocks * 32 * (dtype == GLOO_HIP_F32 ? 4 : 2);
  const Range dst[2] = {{"dst_elems", "", dst_elems, ebytes, true}, {"dst_scales", "", dst_scales, nblocks, false}};
  const Range from = {"src", "", src, wbytes, true};
  if (const int rc = checkRanges(fn, dst, 2, &from, 1)) return rc;
  const size_t grid = (nblocks + kQTileBlocks - 1) / kQTileBlocks;
  if (const int rc = checkGrid(fn, grid, nblocks)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return withFormatAndDtype(fmt, dtype, [&](auto F, auto D) {
    const dim3 g((unsigned)grid), b(kMxBlock);
    if (seed) mx_quantise_kernel<F(), D(), true><<<g, b, 0, s>>>(dst_elems, dst_scales, src, nblocks, mxSeedKey(*seed));
    else mx_quantise_kernel<F(), D(), false><<<g, b, 0, s>>>(dst_elems, dst_scales, src, nblocks, 0u);
    return launchStatus("mx_quantise_kernel");
  });
}

}  // namespace
}  // namespace gloo_amd

extern "C" {

size_t gloo_hip_mx_quantise_tile_blocks(int fmt, int dtype) {
  return gloo_hip_mx_supported(fmt) && gloo_amd::wideDtype(dtype) ? gloo_amd::kQTileBlocks : 0;
}

size_t gloo_hip_mx_wide_tile_blocks(int fmt, int dtype) { return gloo_amd::wideDtype(dtype) ? gloo_hip_mx_tile_blocks(fmt) : 0; }

int gloo_hip_quantise_mx(int fmt, int dtype, void* dst_elems, uint8_t* dst_scales, const void* src, size_t nblocks,
                         gloo_hip_stream_t stream) {
  return gloo_amd::quantiseMx("quantise_mx", fmt, dtype, dst_elems, dst_scales, src, nblocks, nullptr, stream);
}

int gloo_hip_quantise_mx_sr(int fmt, int dtype, void* dst_elems, uint8_t* dst_scales, const void* src, size_t nblocks,
                            uint64_t seed, gloo_hip_stream_t stream) {
  return gloo_amd::quantiseMx("quantise_mx_sr", fmt, dtype, dst_elems, dst_scales, src, nblocks, &seed, stream);
}

int gloo_hip_reduce_mx_wide(int fmt, int dtype, void* dst, const void* const* src_elems, const uint8_t* const* src_scales, int k,
                            size_t nblocks, gloo_hip_stream_t stream) {
  using namespace gloo_amd;
  const std::string fn = "reduce_mx_wide";
  if (const int rc = checkFormatAndDtype(fn, fmt, dtype)) return rc;
  if (k < 1 || k > GLOO_HIP_MAX_SRCS)
    return setError(GLOO_HIP_EINVAL_ARG, fn + ": source count " + std::to_string(k) + " is outside 1.." + std::to_string(GLOO_HIP_MAX_SRCS));
  if (nblocks == 0) return GLOO_HIP_OK;
  if (!src_elems) return setError(GLOO_HIP_EINVAL_PTR, fn + ": src_elems is null");
  if (!src_scales) return setError(GLOO_HIP_EINVAL_PTR, fn + ": src_scales is null");
  const size_t ebytes = nblocks * (fmt == GLOO_HIP_MXFP4_E2M1 ? 16 : 32), wbytes = nblocks * 32 * (dtype == GLOO_HIP_F32 ? 4 : 2);
  const Range to = {"dst", "", dst, wbytes, true};
  Range from[2 * GLOO_HIP_MAX_SRCS];
  MxSrcList list = {};
  for (int j = 0; j < k; j++) {
    const std::string index = "[" + std::to_string(j) + "]";
    from[2 * j] = {"src_elems", index, src_elems[j], ebytes, true};
    from[2 * j + 1] = {"src_scales", index, src_scales[j], nblocks, false};
    list.e[j] = src_elems[j];
    list.s[j] = src_scales[j];
  }
  if (const int rc = checkRanges(fn, &to, 1, from, 2 * k)) return rc;
  const size_t grid = (nblocks + gloo_hip_mx_tile_blocks(fmt) - 1) / gloo_hip_mx_tile_blocks(fmt);
  if (const int rc = checkGrid(fn, grid, nblocks)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return withFormatAndDtype(fmt, dtype, [&](auto F, auto D) {
    mx_fold_wide_kernel<F(), D()><<<dim3((unsigned)grid), dim3(kMxBlock), 0, s>>>(dst, list, k, nblocks);
    return launchStatus("mx_fold_wide_kernel");
  });
}

}  // extern "C"

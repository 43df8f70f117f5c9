// buffer_rsrc.h — raw buffer loads / stores of 16-byte packets, shared by the
// kernel translation units (reduce.hip, mx.hip, mx_quant.hip). Internal: device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace gloo_amd {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Buffer resources.  Each workgroup builds descriptors whose base is its own
// tile (wave-uniform, SGPRs) and whose range is the bytes left in the body, so
// 32-bit lane offsets suffice for any chunk size and the hardware range check
// drops the out-of-range packets of a ragged last tile (loads return 0, stores
// are discarded) without per-lane branches.
constexpr int kRsrcFlags = 0x00020000;  // gfx950 raw-buffer word 3
constexpr int kAuxNT = 2;               // cache policy `nt`: streamed once
constexpr int kAuxWT = 1 | 2 | 16;      // `sc0 nt sc1`: streamed once, written through (not held in L2)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, kRsrcFlags);
}
template <int AUX>
__device__ __forceinline__ u32x4 bload(__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t soff = 0) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, AUX);
}
template <int AUX>
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, uint32_t off, u32x4 v, uint32_t soff = 0) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, soff, AUX);
}

}  // namespace
}  // namespace gloo_amd

// Kernels whose f32 arithmetic is the contract's (the wide sum, the MX sum):
// built with packed f32 arithmetic off, so every add and multiply is one
// single-element IEEE binary32 instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define GLOO_WIDE_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define GLOO_WIDE_KERNEL
#endif

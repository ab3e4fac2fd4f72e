// Device helpers shared by the implicit-GEMM gather kernels (igemm.hip: bf16 / fp32, igemm_fp8.hip: fp8 operands with bf16
// output).  Their argument block, the choice of a build and the launch plans are host code: conv_plan.h.
#pragma once
#include "common.h"
#include "conv_plan.h"

// 16-byte chunk with the elements whose mask bit is clear set to zero (bit e = element e; bf16: two elements per word)
template <typename T> __device__ __forceinline__ uint4 keep_masked(uint4 q, unsigned mb) {
  unsigned w[4] = {q.x, q.y, q.z, q.w};
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] &= ((0u - ((mb >> (2 * i)) & 1u)) & 0x0000ffffu) | ((0u - ((mb >> (2 * i + 1)) & 1u)) & 0xffff0000u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] &= 0u - ((mb >> i) & 1u);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// swizzled byte offset of 16-byte chunk `c` (0..7) in 128-byte row `r`
__device__ __forceinline__ int swz128(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// XCD-aware bijective remap of the linear block id (blocks b and b+8 share an XCD / L2).
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  int q = nblk >> 3, r = nblk & 7, x = bid & 7, i = bid >> 3;
  int start = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return start + i;
}

// 16-byte load through a buffer descriptor: out-of-range offsets (>= num_records) return zeros, so halo / tail
// handling needs no branch and no zero-initialised destination.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
#define OOB_OFF ((int)0x80000000)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t rs, int byte_off) {
  u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ unsigned buf_load4(__amdgpu_buffer_rsrc_t rs, int byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b32(rs, byte_off, 0, 0);
}


// Launchers of a chosen build (conv_plan.h: choose_conv / choose_fp8).  `a` is filled as for the gather kernel; the fp8 one also
// checks it (element = byte; mx_sa / mx_sb set: the block-scaled MX build, the per-tensor scale2 / scale3 then null).
int launch_pgemm_build(GatherArgs& a, ConvBuild b, hipStream_t st);      // pgemm.hip
int dispatch_gather_fp8(GatherArgs& a, hipStream_t st);                  // igemm_fp8.hip

// out[i] (+)= sum over S fp32 slabs of n elements, `stride` elements apart (igemm.hip; also used by wgrad_fp8.hip)
void launch_slab_reduce(const float* ws, float* dw, long n, int S, long stride, int accumulate, hipStream_t st);

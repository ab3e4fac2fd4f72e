// What the row kernels over heat-maps share (heatmap.hip, occlude.hip): the arg-max order, the register-resident map geometry and
// the dispatch between the forms.  rows = B*K maps of H*W fp32.
#pragma once
#include "common.h"
#include <stdlib.h>

struct ArgBest { float v; int i; };
__device__ __forceinline__ bool arg_better(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && !bn) || (an && bn && ai < bi);
  return av > bv || (av == bv && ai < bi);
}

// ---------------------------------------------------------------------------------------- register-resident row kernels
// The loop-form row kernels walk a map two to four times with 4-byte loads and a block reduction between the walks: at one
// 16-KB map per workgroup they are latency-bound (arg-max 1.8 TB/s, soft-arg-max and KL 1.3 - 2 TB/s of the 22-MB heat-map
// tensors by counters, round 2).  These forms fetch a map ONCE with 16-byte loads, all of them in flight together, and keep it
// in registers for every pass:
//   WPM = false: one 256-thread workgroup per map of 1024 * NV floats (64 x 64 maps: NV = 4), block reductions through LDS;
//   WPM = true : one WAVE per map of 256 * NV floats (16 x 16: NV = 1, 32 x 32: NV = 4), four maps per workgroup, reductions by
//                wave shuffles only -- no LDS, no barrier.
// Same arithmetic per element as the loop kernels; sums are folded in a different (fixed) order.
template <int NV, bool WPM> struct RowGeom {
  static constexpr int kThreads = WPM ? 64 : 256;                         // threads per map
  __device__ static int map() { return WPM ? (int)(blockIdx.x * 4 + (threadIdx.x >> 6)) : (int)blockIdx.x; }
  __device__ static int tid() { return WPM ? (int)(threadIdx.x & 63) : (int)threadIdx.x; }
  __device__ static float sum(float v, float* red) { if constexpr (WPM) return wave_sum(v); else return block_sum<4>(v, red); }
  __device__ static float max(float v, float* red) { if constexpr (WPM) return wave_max(v); else return block_max<4>(v, red); }
  // three sums with ONE exchange through LDS (red3: 12 floats) instead of three barrier pairs
  __device__ static void sum3(float& a, float& b, float& c, float* red3) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if constexpr (!WPM) {
      __syncthreads();
      if ((threadIdx.x & 63) == 0) { float* q = red3 + 3 * (threadIdx.x >> 6); q[0] = a; q[1] = b; q[2] = c; }
      __syncthreads();
      a = (red3[0] + red3[3]) + (red3[6] + red3[9]); b = (red3[1] + red3[4]) + (red3[7] + red3[10]); c = (red3[2] + red3[5]) + (red3[8] + red3[11]);
    }
  }
};
template <int NV, bool WPM>
__device__ __forceinline__ void row_load(const float* __restrict__ row, float (&v)[4 * NV]) {
  using G = RowGeom<NV, WPM>;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float4 q = reinterpret_cast<const float4*>(row)[G::tid() + G::kThreads * j];
    v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
  }
}
// element index of register slot (j, e) of this thread
template <int NV, bool WPM> __device__ __forceinline__ int row_index(int j, int e) { return 4 * (RowGeom<NV, WPM>::tid() + RowGeom<NV, WPM>::kThreads * j) + e; }

// row-kernel dispatch (one definition, in api.hip, so that every translation unit reads the MI355_ROW_REG switch once and alike):
// 0 = no register form for this map size (or unaligned pointers): the loop kernels; 1 = 4096 pixels, block per map; 2 = 1024 and
// 3 = 256 pixels, wave per map
int row_form(int HW, const void* a, const void* b = nullptr, const void* c = nullptr);

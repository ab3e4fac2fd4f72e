// fp8 helpers shared by the quantisation kernels (igemm_fp8.hip) and the producers that write fp8 copies on the side (bn.hip).
#pragma once
#include "common.h"

// state[0] = scale (x_q = x * scale), state[1] = descale = 1 / scale, state[2] = amax seen since the last update (bits),
// state[3] = the descale of the COPY most recently made with this record (weight packs: the packed copy outlives the scale
// refresh that follows its optimizer step, so its consumers read [3], not [1]).  Activation copies carry their own 16-byte
// record {scale, descale, 0, 0} behind their data instead (mi355_fp8_quantize, write = 2): several copies of one stream are
// alive at once (a forward shared by two backward passes with an optimizer step -- and its scale refresh -- in between).
__device__ __forceinline__ float clamp_fp8(float v, float lim) {   // saturate; NaN stays NaN
  return v != v ? v : fminf(fmaxf(v, -lim), lim);
}
template <bool BF8>
__device__ __forceinline__ unsigned pack4_fp8(float a, float b, float c, float d) {
  constexpr float LIM = BF8 ? 57344.f : 448.f;
  int w = 0;
  if constexpr (BF8) {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(clamp_fp8(a, LIM), clamp_fp8(b, LIM), w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(clamp_fp8(c, LIM), clamp_fp8(d, LIM), w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_fp8(a, LIM), clamp_fp8(b, LIM), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_fp8(c, LIM), clamp_fp8(d, LIM), w, true);
  }
  return (unsigned)w;
}

// One step of a thread's running max of |v| over the non-NaN elements (Inf counts).  A compare and a select, not fmaxf: that
// becomes v_max_f32 on the raw inputs, which answers a SIGNALLING NaN (any bf16 pattern 0x7f81..0x7fbf widened by a shift is
// one) with a quiet NaN; the next element then replaces that NaN and the maximum seen so far, an Inf included, is forgotten.
__device__ __forceinline__ float fp8_amax_step(float amax, float v) {
  const float a = fabsf(v);
  return a > amax ? a : amax;
}
// The scale exponent of the per-tensor rule: the largest k with amax * 2^margin * 2^k <= 1.75 * 2^max_exp (e4m3: 448 =
// 1.75 * 2^8, e5m2: 57344 = 1.75 * 2^15), clamped to [-126, 126] so that 2^k and 2^-k are both normal floats.  For a finite
// amax > 0, from its bits (exact for every float, subnormals included; as mx_exp below).
__device__ __forceinline__ int fp8_scale_exp(float amax, int max_exp, int margin) {
  const unsigned b = __float_as_uint(amax);
  int ex = (int)(b >> 23);
  unsigned frac = b & 0x7fffffu;
  if (ex == 0) {                                   // subnormal: bring the leading one to bit 23
    const int sh = __clz((int)frac) - 8;
    frac = (frac << sh) & 0x7fffffu;
    ex = 1 - sh;
  }
  const int k = max_exp - (ex - 127) - margin - (frac > 0x600000u ? 1 : 0);      // (mantissa > 1.75: one power less)
  return k < -126 ? -126 : (k > 126 ? 126 : k);
}

// amax of a block into state[2]: ONE integer atomic per block (exact and order-independent).  `seen` = state[2] as loaded at the
// START of the kernel (a plain load whose latency hides behind the main loop): blocks that cannot raise it skip the atomic, and
// the atomic itself is issued without a return value, so no block waits for memory at its end -- a dependent load + atomic in
// the tail of every block doubled the time of the short BatchNorm launches, and per-WAVE atomics on one address serialise at
// ~12 ns each (8192 of them made the first quantisation kernel take 100 us whatever the tensor size).
// Every thread of the 256-thread block must call it.
__device__ __forceinline__ unsigned fp8_amax_seen(const float* state) { return reinterpret_cast<const unsigned*>(state)[2]; }
__device__ __forceinline__ void fp8_record_amax(float amax, float* state, unsigned seen) {
  __shared__ float fp8_red_[4];
  amax = block_max<4>(amax, fp8_red_);
  if (threadIdx.x == 0) {
    const unsigned bits = __float_as_uint(amax);
    if (amax > 0.f && bits > seen) (void)atomicMax(reinterpret_cast<unsigned*>(state) + 2, bits);
  }
}
// 8 values * scale -> 8 fp8 bytes
template <bool BF8>
__device__ __forceinline__ uint2 pack8_fp8(const float (&v)[8], float scale) {
  uint2 o;
  o.x = pack4_fp8<BF8>(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
  o.y = pack4_fp8<BF8>(v[4] * scale, v[5] * scale, v[6] * scale, v[7] * scale);
  return o;
}

// ---- MX (block-scaled e4m3, one E8M0 byte per 32 elements): the scale rule, stated in mx_fp8.hip.  The ONE copy: mx_quantize_kernel,
// the weight packs and the fused copy of the gather kernel's act epilogue (igemm_fp8.hip) all call these.
// exponent e of the rule for a finite amax >= 0 (bit arithmetic: exact for every float, subnormals included)
__device__ __forceinline__ int mx_exp(float amax) {
  const unsigned b = __float_as_uint(amax);
  const int e = (int)(b >> 23) - 127 - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);     // (m > 1.75: fraction bits > 0.75)
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// 2^-e as a float (e <= 120 for every finite amax, so the exponent field 127 - e stays in [7, 254])
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }
// |v| when finite, else 0 (and the non-finite flag set)
__device__ __forceinline__ float mx_finite_abs(float v, bool& bad) {
  const float a = fabsf(v);
  const bool fin = a <= 3.40282347e38f;      // false for NaN and Inf
  bad = bad || !fin;
  return fin ? a : 0.f;
}

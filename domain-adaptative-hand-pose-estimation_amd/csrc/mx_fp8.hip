// MX (OCP microscaling) fp8 operands of the gather GEMM's block-scaled build (gather_fp8_kernel<..., MX> in igemm_fp8.hip;
// 'mxfp8' compute mode): e4m3 elements with one E8M0 scale byte per block of 32 consecutive elements along the axis the
// GEMM contracts.  No state: every copy carries its own scales, nothing is recorded for a later scale update.
//
// Scale rule.  amax = max |x| over the block (exact, from the bf16 / fp32 source), amax = m * 2^E with m in [1, 2):
//   e = E - 8 + (m > 1.75 ? 1 : 0)      the smallest e with amax / 2^e <= 448 (the largest finite e4m3 value),
//   e clamped to [-127, 127], scale byte = e + 127, element = RNE-to-e4m3(x * 2^-e).
// This deliberately departs from OCP MX v1.0's e = floor(log2 amax) - emax(= 8), which puts the top of a block above 448
// where it saturates: here the scale is rounded up so that no finite value saturates.
//   all-zero block (and any amax below 2^-126, where the clamp bites): byte 0x00, elements x * 2^127 (zeros stay +-0);
//   a block holding a NaN or an Inf: byte 0xFF (the E8M0 NaN: its products are NaN, as the bf16 path's would be); its
//     elements are quantised with the e of its finite values (Inf saturates to +-448, NaN stays NaN).
// Halo / out-of-bounds rows need nothing: the kernel's OOB loads return zero data and a zero scale byte (2^-127 * 0 = 0).
//
// Layouts ([rows][C] NHWC activations / gradients; conv-form weights [O][T][I]):
//   activation / gradient   e4m3 [rows][C]   scales [rows][C/32]
//   forward weight pack     e4m3 [O][T][I]   scales [O][T][I/32]
//   input-gradient pack     e4m3 [I][T][O]   scales [I][T][O/32]    (blocks along O; quantised from the fp32 master too)
// i.e. the scale array is the element array with its contiguous axis divided by 32, which is how the GEMM finds the scale
// dword of a 128-element K tile: (byte offset of the tile's first element) / 32.
#include "igemm_common.h"
#include "fp8_common.h"

// (mx_exp / mx_inv_scale / mx_finite_abs, the one copy of the rule above: fp8_common.h -- the fused copy of the act epilogue in
// igemm_fp8.hip uses them too)

// ------------------------------------------------------------------------------------ activations / gradients
// 16 elements per thread-iteration; the two lanes of a pair (2k, 2k + 1) hold one 32-element block and exchange their partial
// amax.  n16 is even and the grid stride is even, so both lanes of a pair always run the same iterations.  HBM-bound:
// 2 (bf16) or 4 (fp32) bytes read and 1 + 1/32 written per element, plain vector stores.
template <typename T>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const T* __restrict__ x, unsigned char* __restrict__ q,
                                                          unsigned char* __restrict__ s, long n16) {
  constexpr int PER = Chunk<T>::N, NC = 16 / PER;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
    float v[16];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float w[PER]; Chunk<T>::load(x + i * 16 + c * PER, w);
#pragma unroll
      for (int e = 0; e < PER; ++e) v[c * PER + e] = w[e];
    }
    float amax = 0.f; bool bad = false;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, mx_finite_abs(v[e], bad));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    bad = (__shfl_xor((int)bad, 1, 64) | (int)bad) != 0;
    const int ex = mx_exp(amax);
    const float sc = mx_inv_scale(ex);
    uint4 o;
    o.x = pack4_fp8<false>(v[0] * sc, v[1] * sc, v[2] * sc, v[3] * sc);
    o.y = pack4_fp8<false>(v[4] * sc, v[5] * sc, v[6] * sc, v[7] * sc);
    o.z = pack4_fp8<false>(v[8] * sc, v[9] * sc, v[10] * sc, v[11] * sc);
    o.w = pack4_fp8<false>(v[12] * sc, v[13] * sc, v[14] * sc, v[15] * sc);
    reinterpret_cast<uint4*>(q)[i] = o;
    if (!(i & 1)) s[i >> 1] = bad ? (unsigned char)0xFF : (unsigned char)(ex + 127);
  }
}

extern "C" int mi355_mx_quantize(const void* x, void* q, void* scales, long rows, int C, int src_dtype, void* stream) {
  if (!x || !q || !scales) MI_FAIL(MI355_EINVAL, "mx_quantize: null source, element or scale pointer");
  if (rows < 1 || C < 32 || C % 32) MI_FAIL(MI355_EINVAL, "mx_quantize: rows=%ld, C=%d must be a positive multiple of 32", rows, C);
  if (src_dtype != MI355_BF16 && src_dtype != MI355_F32) MI_FAIL(MI355_EINVAL, "mx_quantize: source dtype %d", src_dtype);
  if (((uintptr_t)x | (uintptr_t)q) % 16) MI_FAIL(MI355_EINVAL, "mx_quantize: source and element buffers must be 16-byte aligned");
  const long n16 = rows * (long)C / 16;
  int grid = (int)((n16 + 255) / 256); if (grid > 2048) grid = 2048;
  hipStream_t st = as_stream(stream);
  unsigned char* o = reinterpret_cast<unsigned char*>(q);
  unsigned char* s = reinterpret_cast<unsigned char*>(scales);
  if (src_dtype == MI355_BF16) hipLaunchKernelGGL(mx_quantize_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, o, s, n16);
  else hipLaunchKernelGGL(mx_quantize_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, o, s, n16);
  MI_CHECK_LAUNCH("mx_quantize");
  return MI355_OK;
}

// ------------------------------------------------------------------------------------ weight packs
// 4 values of a 32-element block held by the 8 aligned lanes of a group -> 4 e4m3 bytes; returns the block's scale byte.
__device__ __forceinline__ unsigned char mx_quant4_group8(const float (&v)[4], unsigned& word) {
  float amax = 0.f; bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) amax = fmaxf(amax, mx_finite_abs(v[e], bad));
  int b = bad ? 1 : 0;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) { amax = fmaxf(amax, __shfl_xor(amax, o, 64)); b |= __shfl_xor(b, o, 64); }
  const int ex = mx_exp(amax);
  const float sc = mx_inv_scale(ex);
  word = pack4_fp8<false>(v[0] * sc, v[1] * sc, v[2] * sc, v[3] * sc);
  return b ? (unsigned char)0xFF : (unsigned char)(ex + 127);
}

// fp32 master [O][T][I] -> wf [O][T][I] + sf [O][T][I/32] and wt [I][T][O] + st [I][T][O/32], one 32 x 32 (o, i) tile of one
// tap per 256-thread block: row o of the tile is one forward block, column i one input-gradient block, both from the master.
__device__ __forceinline__ void pack_mx_block(const float* __restrict__ w, unsigned char* __restrict__ wf, unsigned char* __restrict__ sf,
                                              unsigned char* __restrict__ wt, unsigned char* __restrict__ st, int O, int T, int I, int b) {
  __shared__ float tile[32][33];
  const int tiles_i = I / 32, tiles_o = O / 32;
  const int tap = b / (tiles_i * tiles_o), r = b % (tiles_i * tiles_o);
  const int o0 = (r / tiles_i) * 32, i0 = (r % tiles_i) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8
#pragma unroll
  for (int k = 0; k < 4; ++k) tile[ty + 8 * k][tx] = w[((size_t)(o0 + ty + 8 * k) * T + tap) * I + i0 + tx];
  __syncthreads();
  const int row = threadIdx.x >> 3, g = threadIdx.x & 7;             // 8 lanes per 32-element block
  {   // wf: 4 consecutive i of row o
    const float v[4] = {tile[row][4 * g], tile[row][4 * g + 1], tile[row][4 * g + 2], tile[row][4 * g + 3]};
    unsigned word;
    const unsigned char sb = mx_quant4_group8(v, word);
    const size_t rr = (size_t)(o0 + row) * T + tap;
    *reinterpret_cast<unsigned*>(wf + rr * I + i0 + 4 * g) = word;
    if (g == 0) sf[rr * (I / 32) + i0 / 32] = sb;
  }
  {   // wt: 4 consecutive o of column i
    const float v[4] = {tile[4 * g][row], tile[4 * g + 1][row], tile[4 * g + 2][row], tile[4 * g + 3][row]};
    unsigned word;
    const unsigned char sb = mx_quant4_group8(v, word);
    const size_t rr = (size_t)(i0 + row) * T + tap;
    *reinterpret_cast<unsigned*>(wt + rr * O + o0 + 4 * g) = word;
    if (g == 0) st[rr * (O / 32) + o0 / 32] = sb;
  }
}
__global__ __launch_bounds__(256) void pack_weights_mx_kernel(const float* __restrict__ w, unsigned char* __restrict__ wf,
                                                              unsigned char* __restrict__ sf, unsigned char* __restrict__ wt,
                                                              unsigned char* __restrict__ st, int O, int T, int I) {
  pack_mx_block(w, wf, sf, wt, st, O, T, I, blockIdx.x);
}
// every MX conv weight of an optimizer group in ONE launch: items in device memory, block -> item by binary search over the
// first-block prefix (as pack_weights_fp8_batched_kernel)
__global__ __launch_bounds__(256) void pack_weights_mx_batched_kernel(const mi355_packmx_item* __restrict__ items, int nitems) {
  int lo = 0, hi = nitems - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  const mi355_packmx_item it = items[lo];
  pack_mx_block(it.w, (unsigned char*)it.wf, (unsigned char*)it.sf, (unsigned char*)it.wt, (unsigned char*)it.st, it.O, it.T, it.I,
                b - it.blk0);
}

extern "C" int mi355_pack_weights_mx(const float* w_master, void* wf, void* sf, void* wt, void* st, int O, int T, int I, void* stream) {
  if (!w_master || !wf || !sf || !wt || !st) MI_FAIL(MI355_EINVAL, "pack_weights_mx: null master, pack or scale pointer");
  if (O < 32 || I < 32 || O % 32 || I % 32 || T < 1) MI_FAIL(MI355_EINVAL, "pack_weights_mx: O=%d I=%d must be multiples of 32 (T=%d)", O, I, T);
  if ((long)O * T * I >= (1L << 31)) MI_FAIL(MI355_EINVAL, "pack_weights_mx: weight too large");
  hipLaunchKernelGGL(pack_weights_mx_kernel, dim3((O / 32) * (I / 32) * T), dim3(256), 0, as_stream(stream), w_master,
                     (unsigned char*)wf, (unsigned char*)sf, (unsigned char*)wt, (unsigned char*)st, O, T, I);
  MI_CHECK_LAUNCH("pack_weights_mx");
  return MI355_OK;
}

extern "C" int mi355_pack_weights_mx_batched(const mi355_packmx_item* items_dev, int nitems, int total_blocks, void* stream) {
  if (!items_dev || nitems < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "pack_weights_mx_batched: bad args");
  hipLaunchKernelGGL(pack_weights_mx_batched_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, nitems);
  MI_CHECK_LAUNCH("pack_weights_mx_batched");
  return MI355_OK;
}

// What the per-joint losses of jfa.hip (loss1 / loss3) and proto.hip (lossx / lossx3) share: the window of a key point, the pooling
// kernel and its backward written as a gather (each with a small policy for the one step in which the two losses differ), the
// check of the geometry arguments, the host code that launches the two kernels, and the fp64 wave sum of the KL kernels.
#pragma once
#include <math.h>
#include "common.h"

#define JOINT_T 256                   // threads of a block
#define JOINT_CT 256                  // channels of a block's channel tile: at most 32 bf16 / 64 fp32 chunks of 16 bytes
#define JOINT_STRIP 256               // joint_gather: pixels of a block's strip

struct joint_win { int r0, r1, q0, q1; };        // rows [r0, r1) x columns [q0, q1); empty when r1 <= r0 or q1 <= q0

// The reference's window (loss1): r0 = int(max(cr - radius, 0)), r1 = int(min(cr + radius, H - 1)) and the same for the columns
// with W - 1 -- fp32 arithmetic, truncation towards zero as .int() does, the half-open slice r0:r1.  `rows_by_x`: the reference
// slices the row axis by x and the column axis by y; 0 is the geometric indexing.  A coordinate outside the map leaves r1 <= r0
// (the reference falls into negative-index slicing there): an empty window.  A NaN coordinate gives an empty window as well.
// The bounds are brought into [0, H] and [-1, H - 1] as floats before the conversion, so that an infinity or a value past 2^31
// never reaches the cast; for every other value this changes nothing (a lower bound above H and an upper bound below 0 are
// empty windows either way).
__device__ __forceinline__ joint_win joint_window(const float* __restrict__ xy, int radius, int rows_by_x, int H, int W) {
  const float x = xy[0], y = xy[1], rad = (float)radius;
  const float cr = rows_by_x ? x : y, cc = rows_by_x ? y : x;
  joint_win w;
  if (cr != cr || cc != cc) { w.r0 = 0; w.r1 = 0; w.q0 = 0; w.q1 = 0; return w; }
  w.r0 = (int)fminf(fmaxf(cr - rad, 0.f), (float)H);
  w.r1 = (int)fmaxf(fminf(cr + rad, (float)(H - 1)), -1.f);
  w.q0 = (int)fminf(fmaxf(cc - rad, 0.f), (float)W);
  w.q1 = (int)fmaxf(fminf(cc + rad, (float)(W - 1)), -1.f);
  return w;
}

// The xor butterfly in fp64, the same in every lane: every wave sum of the two KL kernels.
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- pooling
// One block per (b, j) and channel tile.  Thread t owns chunk t % CW of the tile and pixel group g = t / CW: it adds the window's
// pixels g, g + G, g + 2 G, ... (row-major inside the window) in that order, the G partial sums meet in LDS and the threads of
// group 0 add them in ascending g, divide once and store.  The policy D says by what: D::zero(w) -- store zeros, divide by
// nothing -- and D::of(w), the divisor of every element of the window otherwise.
template <typename T, typename D>
__global__ __launch_bounds__(JOINT_T) void joint_pool_kernel(const T* __restrict__ f, const float* __restrict__ xy, float* __restrict__ desc,
                                                              int K, int C, int H, int W, int radius, int rows_by_x, D by) {
  constexpr int N = Chunk<T>::N;
  __shared__ __attribute__((aligned(16))) float part[JOINT_T][N];
  const int t = threadIdx.x, bj = blockIdx.x, b = bj / K;
  const int c0 = blockIdx.y * JOINT_CT;
  const int CW = min(C - c0, JOINT_CT) / N, G = JOINT_T / CW;
  const int ch = t % CW, g = t / CW;
  const joint_win w = joint_window(xy + 2L * bj, radius, rows_by_x, H, W);
  const int nr = max(w.r1 - w.r0, 0), nq = max(w.q1 - w.q0, 0), np = nr * nq;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  if (g < G) {
    const T* __restrict__ fb = f + (long)b * H * W * C + c0 + ch * N;
    for (int p = g; p < np; p += G) {
      const int r = w.r0 + p / nq, q = w.q0 + p % nq;
      float v[N];
      Chunk<T>::load(fb + ((long)r * W + q) * C, v);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) part[t][e] = acc[e];
  __syncthreads();
  if (g == 0) {
    for (int gg = 1; gg < G; ++gg)
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += part[gg * CW + ch][e];
    float* __restrict__ d = desc + (long)bj * C + c0 + ch * N;
    const bool zero = by.zero(w);
    const float div = zero ? 1.f : by.of(w);
#pragma unroll
    for (int e4 = 0; e4 < N; e4 += 4)
      *reinterpret_cast<float4*>(d + e4) = zero ? make_float4(0.f, 0.f, 0.f, 0.f)
                                                : make_float4(acc[e4] / div, acc[e4 + 1] / div, acc[e4 + 2] / div, acc[e4 + 3] / div);
  }
}

// ---------------------------------------------------------------- backward of the pooling, as a gather
// One block per strip of JOINT_STRIP pixels of one image and channel tile.  The image's K windows and the table gd[j][c], the
// gradient that every pixel of window j receives in channel c0 + c, sit in LDS; the policy S forms the table once per (b, j, c)
// in S::fill (which sees the finished windows of its own thread, win[t] for t < K, and ends before the block's barrier).
// Thread t owns chunk t % CW of every pixel gp, gp + G, ... of the strip: it adds gd[j] over the joints whose window holds the
// pixel, j ascending, in fp32.  Write mode stores the sum rounded to T (+0 where no window covers); accumulate mode leaves an
// uncovered pixel alone and stores RNE(old + sum) on a covered one.
template <typename T, bool ACC, typename S>
__global__ __launch_bounds__(JOINT_T) void joint_gather_kernel(const float* __restrict__ xy, T* __restrict__ out, int K, int C, int H, int W,
                                                                int radius, int rows_by_x, S src) {
  constexpr int N = Chunk<T>::N;
  __shared__ __attribute__((aligned(16))) float gd[MI355_JFA_MAX_JOINTS * JOINT_CT];
  __shared__ joint_win win[MI355_JFA_MAX_JOINTS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int c0 = blockIdx.z * JOINT_CT;
  const int CT = min(C - c0, JOINT_CT), CW = CT / N, G = JOINT_T / CW;
  if (t < K) win[t] = joint_window(xy + 2L * (b * K + t), radius, rows_by_x, H, W);
  src.fill(gd, win, b, K, C, c0, CT);
  __syncthreads();
  const int ch = t % CW, gp = t / CW;
  if (gp >= G) return;
  const int p0 = blockIdx.x * JOINT_STRIP, p1 = min(p0 + JOINT_STRIP, H * W);
  T* __restrict__ ob = out + (long)b * H * W * C + c0 + ch * N;
  // The walk below is bound by instruction issue, and its time moves by 4 % with where its loops fall in the 64-byte fetch lines:
  // before this padding the same loop took 100 us under one policy and 104 us under the other (write mode, workload shape),
  // only because their S::fill code differs in length by 16 bytes.  The padding fixes the position for every policy; the three
  // no-ops put the pixel loop's head 32 bytes into a line with today's compiler, the faster of the placements measured for
  // write mode, which is the mode a step with one term runs ("Joint feature alignment", Measured).
  asm volatile(".p2align 6\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0");
  for (int p = p0 + gp; p < p1; p += G) {
    const int r = p / W, q = p - r * W;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    bool covered = false;
    for (int j = 0; j < K; ++j) {
      const joint_win w = win[j];
      if (r < w.r0 || r >= w.r1 || q < w.q0 || q >= w.q1) continue;
      covered = true;
      const float* __restrict__ s = gd + j * JOINT_CT + ch * N;
#pragma unroll
      for (int e4 = 0; e4 < N; e4 += 4) {
        const float4 v = *reinterpret_cast<const float4*>(s + e4);
        acc[e4] += v.x; acc[e4 + 1] += v.y; acc[e4 + 2] += v.z; acc[e4 + 3] += v.w;
      }
    }
    T* __restrict__ o = ob + (long)p * C;
    if (ACC) {
      if (!covered) continue;
      float old[N];
      Chunk<T>::load(o, old);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = old[e] + acc[e];
    }
    Chunk<T>::store(o, acc);
  }
}

// ---------------------------------------------------------------- host
// nullptr, or what is wrong with the geometry
static const char* joint_geometry(const char* who, int B, int K, int C, int H, int W, int radius, int dtype) {
  static thread_local char msg[160];
  msg[0] = 0;
  if (dtype != MI355_F32 && dtype != MI355_BF16) snprintf(msg, sizeof(msg), "%s: dtype=%d (fp32 or bf16 features)", who, dtype);
  else if (B < 1 || B > 65535) snprintf(msg, sizeof(msg), "%s: B=%d (1 .. 65535)", who, B);
  else if (K < 1 || K > MI355_JFA_MAX_JOINTS) snprintf(msg, sizeof(msg), "%s: K=%d (1 .. %d joints)", who, K, MI355_JFA_MAX_JOINTS);
  else if (C < 8 || C % 8) snprintf(msg, sizeof(msg), "%s: C=%d (a multiple of 8, at least 8)", who, C);
  else if (H < 1 || W < 1 || (long)H * W > (1L << 24)) snprintf(msg, sizeof(msg), "%s: H=%d W=%d (at least 1, H W <= 2^24)", who, H, W);
  else if (radius < 1 || radius > (1 << 20)) snprintf(msg, sizeof(msg), "%s: radius=%d (at least 1)", who, radius);
  else if (cdiv(C, JOINT_CT) > 65535) snprintf(msg, sizeof(msg), "%s: C=%d too large (at most 65535 channel tiles of %d)", who, C, JOINT_CT);
  return msg[0] ? msg : nullptr;
}

// The body of a pooling entry point `who`: the checks, the label and the launch with the divisor policy `by`; `more` is a check
// of the entry's own that comes after the geometry's (nullptr, or its message).
template <typename D>
static int joint_pool_launch(const char* who, const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius,
                             int rows_by_x, int dtype, void* stream, D by, const char* more = nullptr) {
  if (!feature || !xy || !desc) MI_FAIL(MI355_EINVAL, "%s: null pointer", who);
  if (((uintptr_t)feature | (uintptr_t)desc) & 15) MI_FAIL(MI355_EINVAL, "%s: feature and desc must be 16-byte aligned", who);
  if ((uintptr_t)xy & 3) MI_FAIL(MI355_EINVAL, "%s: xy must be 4-byte aligned", who);
  if (const char* m = joint_geometry(who, B, K, C, H, W, radius, dtype)) MI_FAIL(MI355_EINVAL, "%s", m);
  if (more) MI_FAIL(MI355_EINVAL, "%s", more);
  hipStream_t s = as_stream(stream);
  const int esz = dtype == MI355_BF16 ? 2 : 4;
  const int side = 2 * radius < (H > W ? H : W) ? 2 * radius : (H > W ? H : W);
  char lab[96];
  snprintf(lab, sizeof(lab), "%s B%d K%d C%d %dx%d r%d %s%s", who, B, K, C, H, W, radius, rows_by_x ? "ref" : "xy", esz == 2 ? "" : " f32");
  ProfScope ps(s, 0.0, (double)B * K * C * ((double)side * side * esz + 4.0), 2, lab);
  const dim3 grid(B * K, cdiv(C, JOINT_CT));
  if (esz == 2) hipLaunchKernelGGL((joint_pool_kernel<bf16_t, D>), grid, dim3(JOINT_T), 0, s, (const bf16_t*)feature, xy, desc, K, C, H, W, radius, rows_by_x ? 1 : 0, by);
  else hipLaunchKernelGGL((joint_pool_kernel<float, D>), grid, dim3(JOINT_T), 0, s, (const float*)feature, xy, desc, K, C, H, W, radius, rows_by_x ? 1 : 0, by);
  MI_CHECK_LAUNCH(who);
  return MI355_OK;
}

// The body of a gather entry point `who`.  `src` is the table policy; it names its gradient operand (S::GRAD, src.g) and, where it
// has one, its record in device memory (src.blend, else nullptr).
template <typename S>
static int joint_gather_launch(const char* who, const float* xy, void* grad_feature, int accumulate, int B, int K, int C, int H, int W, int radius,
                               int rows_by_x, int dtype, void* stream, S src, const char* more = nullptr) {
  if (!src.g || !xy || (S::BLEND && !src.blend) || !grad_feature) MI_FAIL(MI355_EINVAL, "%s: null pointer", who);
  if (((uintptr_t)src.g | (uintptr_t)grad_feature) & 15) MI_FAIL(MI355_EINVAL, "%s: %s and grad_feature must be 16-byte aligned", who, S::GRAD);
  if (((uintptr_t)xy | (uintptr_t)src.blend) & 3) MI_FAIL(MI355_EINVAL, "%s: %s must be 4-byte aligned", who, S::BLEND ? "xy and blend" : "xy");
  if (const char* m = joint_geometry(who, B, K, C, H, W, radius, dtype)) MI_FAIL(MI355_EINVAL, "%s", m);
  if (more) MI_FAIL(MI355_EINVAL, "%s", more);
  hipStream_t s = as_stream(stream);
  const int esz = dtype == MI355_BF16 ? 2 : 4;
  char lab[96];
  snprintf(lab, sizeof(lab), "%s B%d K%d C%d %dx%d r%d %s %s%s", who, B, K, C, H, W, radius, rows_by_x ? "ref" : "xy", accumulate ? "acc" : "write",
           esz == 2 ? "" : " f32");
  ProfScope ps(s, 0.0, (double)B * H * W * C * esz * (accumulate ? 2.0 : 1.0), 2, lab);
  const dim3 grid(cdiv((long)H * W, JOINT_STRIP), B, cdiv(C, JOINT_CT));
#define JOINT_GATHER(T, ACC) hipLaunchKernelGGL((joint_gather_kernel<T, ACC, S>), grid, dim3(JOINT_T), 0, s, xy, (T*)grad_feature, K, C, H, W, radius, rows_by_x ? 1 : 0, src)
  if (esz == 2) { if (accumulate) JOINT_GATHER(bf16_t, true); else JOINT_GATHER(bf16_t, false); }
  else { if (accumulate) JOINT_GATHER(float, true); else JOINT_GATHER(float, false); }
#undef JOINT_GATHER
  MI_CHECK_LAUNCH(who);
  return MI355_OK;
}

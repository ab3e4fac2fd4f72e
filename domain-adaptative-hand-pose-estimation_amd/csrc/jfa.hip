// Per-joint feature alignment (uda/model/loss.py:331-378, loss1 / loss3): the box sum of a window of the feature map around each
// key point into one descriptor per joint, the KL divergence between the channel distributions of two sets of descriptors with
// both gradients, and the backward of the pooling written as a gather.  Features are channels-last ([B][H][W][C], bf16 or fp32):
// the C channels of one pixel are contiguous and every access along them is one 16-byte chunk per lane.  No atomics; every sum
// runs in a fixed order, so two runs give the same bits.
#include <math.h>
#include "common.h"
#include "jfa_common.h"

#define JFA_T 256                     // threads of a block
#define JFA_CT 256                    // channels of a block's channel tile: at most 32 bf16 / 64 fp32 chunks of 16 bytes
#define JFA_STRIP 256                 // jfa_scatter: pixels of a block's strip

// ---------------------------------------------------------------- pooling
// One block per (b, j) and channel tile.  Thread t owns chunk t % CW of the tile and pixel group g = t / CW: it adds the window's
// pixels g, g + G, g + 2 G, ... (row-major inside the window) in that order, the G partial sums meet in LDS and the threads of
// group 0 add them in ascending g, divide once and store.
template <typename T>
__global__ __launch_bounds__(JFA_T) void jfa_pool_kernel(const T* __restrict__ f, const float* __restrict__ xy, float* __restrict__ desc,
                                                          int K, int C, int H, int W, int radius, float divisor, int rows_by_x) {
  constexpr int N = Chunk<T>::N;
  __shared__ __attribute__((aligned(16))) float part[JFA_T][N];
  const int t = threadIdx.x, bj = blockIdx.x, b = bj / K;
  const int c0 = blockIdx.y * JFA_CT;
  const int CW = min(C - c0, JFA_CT) / N, G = JFA_T / CW;
  const int ch = t % CW, g = t / CW;
  const jfa_win w = jfa_window(xy + 2L * bj, radius, rows_by_x, H, W);
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
#pragma unroll
    for (int e4 = 0; e4 < N; e4 += 4)
      *reinterpret_cast<float4*>(d + e4) = make_float4(acc[e4] / divisor, acc[e4 + 1] / divisor, acc[e4 + 2] / divisor, acc[e4 + 3] / divisor);
  }
}

// ---------------------------------------------------------------- KL between the channel distributions
// One wave per row (b, j) of a, b [rows][C]: lp = log_softmax(a), q = (b + 1e-6) / S with S = sum_c (b_c + 1e-6),
// row = sum_c q_c (log q_c - lp_c);  ga = coef (softmax(a) - q),  gb = coef ((log q - lp) - row) / S.  Lane l owns the 16-byte
// chunks l, l + 64, ...; every wave sum is the xor butterfly, the same in every lane.
// The arithmetic behind the fp32 operands is fp64: log q and lp are both near -log C and their difference is what is summed -- a
// row is a few 1e-3 where each term is a few units, so fp32 logarithms (1 ulp of 2 .. 5) leave the loss with 1e-4 relative, more
// than the reference's own fp32 run.  The rows are small (B K C elements, 0.3 M at the workload shape); fp64 costs nothing here.
__device__ inline double jfa_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(JFA_T) void jfa_kl_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ rows,
                                                        float* __restrict__ ga, float* __restrict__ gb, int nrows, int C, float coef) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * (JFA_T / WAVE) + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const float* __restrict__ ar = a + (long)row * C;
  const float* __restrict__ br = b + (long)row * C;
  const double eps = 1e-6;
  float m = -INFINITY;
  double s = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    m = fmaxf(fmaxf(fmaxf(m, va.x), fmaxf(va.y, va.z)), va.w);
    s += (((double)vb.x + eps) + ((double)vb.y + eps)) + (((double)vb.z + eps) + ((double)vb.w + eps));
  }
  m = wave_max(m);
  const double S = jfa_wave_sum(s), md = (double)m;
  double z = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c);
    z += (exp((double)va.x - md) + exp((double)va.y - md)) + (exp((double)va.z - md) + exp((double)va.w - md));
  }
  const double lse = log(jfa_wave_sum(z));
  double kl = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    const float x[4] = {va.x, va.y, va.z, va.w}, y[4] = {vb.x, vb.y, vb.z, vb.w};
    double e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double q = ((double)y[i] + eps) / S;
      e[i] = q * (log(q) - (((double)x[i] - md) - lse));
    }
    kl += (e[0] + e[1]) + (e[2] + e[3]);
  }
  kl = jfa_wave_sum(kl);
  if (lane == 0) rows[row] = (float)kl;
  if (!ga && !gb) return;
  const double cf = (double)coef;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    const float x[4] = {va.x, va.y, va.z, va.w}, y[4] = {vb.x, vb.y, vb.z, vb.w};
    float da[4], db[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double q = ((double)y[i] + eps) / S, lp = ((double)x[i] - md) - lse;
      da[i] = (float)(cf * (exp(lp) - q));
      db[i] = (float)(cf * (((log(q) - lp) - kl) / S));
    }
    if (ga) *reinterpret_cast<float4*>(ga + (long)row * C + c) = make_float4(da[0], da[1], da[2], da[3]);
    if (gb) *reinterpret_cast<float4*>(gb + (long)row * C + c) = make_float4(db[0], db[1], db[2], db[3]);
  }
}

// ---------------------------------------------------------------- backward of the pooling, as a gather
// One block per strip of JFA_STRIP pixels of one image and channel tile.  The image's K windows and gd[j][c] = g[b][j][c] /
// divisor (formed once per (b, j, c)) sit in LDS.  Thread t owns chunk t % CW of every pixel g, g + G, ... of the strip: it adds
// gd[j] over the joints whose window holds the pixel, j ascending, in fp32.  Write mode stores the sum rounded to T (+0 where no
// window covers); accumulate mode leaves an uncovered pixel alone and stores RNE(old + sum) on a covered one.
template <typename T, bool ACC>
__global__ __launch_bounds__(JFA_T) void jfa_scatter_kernel(const float* __restrict__ g, const float* __restrict__ xy, T* __restrict__ out,
                                                             int K, int C, int H, int W, int radius, float divisor, int rows_by_x) {
  constexpr int N = Chunk<T>::N;
  __shared__ __attribute__((aligned(16))) float gd[MI355_JFA_MAX_JOINTS * JFA_CT];
  __shared__ jfa_win win[MI355_JFA_MAX_JOINTS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int c0 = blockIdx.z * JFA_CT;
  const int CT = min(C - c0, JFA_CT), CW = CT / N, G = JFA_T / CW;
  if (t < K) win[t] = jfa_window(xy + 2L * (b * K + t), radius, rows_by_x, H, W);
  for (int e = t; e < K * CT; e += JFA_T) {
    const int j = e / CT, c = e - j * CT;
    gd[j * JFA_CT + c] = g[((long)b * K + j) * C + c0 + c] / divisor;
  }
  __syncthreads();
  const int ch = t % CW, gp = t / CW;
  if (gp >= G) return;
  const int p0 = blockIdx.x * JFA_STRIP, p1 = min(p0 + JFA_STRIP, H * W);
  T* __restrict__ ob = out + (long)b * H * W * C + c0 + ch * N;
  for (int p = p0 + gp; p < p1; p += G) {
    const int r = p / W, q = p - r * W;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    bool covered = false;
    for (int j = 0; j < K; ++j) {
      const jfa_win w = win[j];
      if (r < w.r0 || r >= w.r1 || q < w.q0 || q >= w.q1) continue;
      covered = true;
      const float* __restrict__ s = gd + j * JFA_CT + ch * N;
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
extern "C" int mi355_jfa_pool(const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius,
                              float divisor, int rows_by_x, int dtype, void* stream) {
  if (!feature || !xy || !desc) MI_FAIL(MI355_EINVAL, "jfa_pool: null pointer");
  if (((uintptr_t)feature | (uintptr_t)desc) & 15) MI_FAIL(MI355_EINVAL, "jfa_pool: feature and desc must be 16-byte aligned");
  if ((uintptr_t)xy & 3) MI_FAIL(MI355_EINVAL, "jfa_pool: xy must be 4-byte aligned");
  if (const char* m = jfa_geometry("jfa_pool", B, K, C, H, W, radius, divisor, dtype, JFA_CT)) MI_FAIL(MI355_EINVAL, "%s", m);
  hipStream_t s = as_stream(stream);
  const int esz = dtype == MI355_BF16 ? 2 : 4;
  const int side = 2 * radius < (H > W ? H : W) ? 2 * radius : (H > W ? H : W);
  char lab[96];
  snprintf(lab, sizeof(lab), "jfa_pool B%d K%d C%d %dx%d r%d %s%s", B, K, C, H, W, radius, rows_by_x ? "ref" : "xy", esz == 2 ? "" : " f32");
  ProfScope ps(s, 0.0, (double)B * K * C * ((double)side * side * esz + 4.0), 2, lab);
  const dim3 grid(B * K, cdiv(C, JFA_CT));
  if (esz == 2) hipLaunchKernelGGL(jfa_pool_kernel<bf16_t>, grid, dim3(JFA_T), 0, s, (const bf16_t*)feature, xy, desc, K, C, H, W, radius, divisor, rows_by_x ? 1 : 0);
  else hipLaunchKernelGGL(jfa_pool_kernel<float>, grid, dim3(JFA_T), 0, s, (const float*)feature, xy, desc, K, C, H, W, radius, divisor, rows_by_x ? 1 : 0);
  MI_CHECK_LAUNCH("jfa_pool");
  return MI355_OK;
}

extern "C" int mi355_jfa_kl(const float* a, const float* b, float* rows, float* grad_a, float* grad_b, int nrows, int C, float coef,
                            void* stream) {
  if (!a || !b || !rows) MI_FAIL(MI355_EINVAL, "jfa_kl: null pointer");
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad_a | (uintptr_t)grad_b) & 15) MI_FAIL(MI355_EINVAL, "jfa_kl: a, b and the gradients must be 16-byte aligned");
  if ((uintptr_t)rows & 3) MI_FAIL(MI355_EINVAL, "jfa_kl: rows must be 4-byte aligned");
  if (nrows < 1) MI_FAIL(MI355_EINVAL, "jfa_kl: nrows=%d", nrows);
  if (C < 8 || C % 8) MI_FAIL(MI355_EINVAL, "jfa_kl: C=%d (a multiple of 8, at least 8)", C);
  if (!isfinite(coef)) MI_FAIL(MI355_EINVAL, "jfa_kl: coef=%g must be finite", (double)coef);
  hipStream_t s = as_stream(stream);
  char lab[96];
  snprintf(lab, sizeof(lab), "jfa_kl rows%d C%d grads%d%d", nrows, C, grad_a ? 1 : 0, grad_b ? 1 : 0);
  ProfScope ps(s, 0.0, 4.0 * nrows * C * (2.0 + (grad_a ? 1 : 0) + (grad_b ? 1 : 0)), 2, lab);
  hipLaunchKernelGGL(jfa_kl_kernel, dim3(cdiv(nrows, JFA_T / WAVE)), dim3(JFA_T), 0, s, a, b, rows, grad_a, grad_b, nrows, C, coef);
  MI_CHECK_LAUNCH("jfa_kl");
  return MI355_OK;
}

extern "C" int mi355_jfa_scatter(const float* grad_desc, const float* xy, void* grad_feature, int accumulate, int B, int K, int C, int H,
                                 int W, int radius, float divisor, int rows_by_x, int dtype, void* stream) {
  if (!grad_desc || !xy || !grad_feature) MI_FAIL(MI355_EINVAL, "jfa_scatter: null pointer");
  if (((uintptr_t)grad_desc | (uintptr_t)grad_feature) & 15) MI_FAIL(MI355_EINVAL, "jfa_scatter: grad_desc and grad_feature must be 16-byte aligned");
  if ((uintptr_t)xy & 3) MI_FAIL(MI355_EINVAL, "jfa_scatter: xy must be 4-byte aligned");
  if (const char* m = jfa_geometry("jfa_scatter", B, K, C, H, W, radius, divisor, dtype, JFA_CT)) MI_FAIL(MI355_EINVAL, "%s", m);
  hipStream_t s = as_stream(stream);
  const int esz = dtype == MI355_BF16 ? 2 : 4;
  char lab[96];
  snprintf(lab, sizeof(lab), "jfa_scatter B%d K%d C%d %dx%d r%d %s %s%s", B, K, C, H, W, radius, rows_by_x ? "ref" : "xy", accumulate ? "acc" : "write",
           esz == 2 ? "" : " f32");
  ProfScope ps(s, 0.0, (double)B * H * W * C * esz * (accumulate ? 2.0 : 1.0), 2, lab);
  const dim3 grid(cdiv((long)H * W, JFA_STRIP), B, cdiv(C, JFA_CT));
#define JFA_SCATTER(T, ACC) hipLaunchKernelGGL((jfa_scatter_kernel<T, ACC>), grid, dim3(JFA_T), 0, s, grad_desc, xy, (T*)grad_feature, K, C, H, W, radius, divisor, rows_by_x ? 1 : 0)
  if (esz == 2) { if (accumulate) JFA_SCATTER(bf16_t, true); else JFA_SCATTER(bf16_t, false); }
  else { if (accumulate) JFA_SCATTER(float, true); else JFA_SCATTER(float, false); }
#undef JFA_SCATTER
  MI_CHECK_LAUNCH("jfa_scatter");
  return MI355_OK;
}

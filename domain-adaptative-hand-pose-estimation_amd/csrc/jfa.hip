// Per-joint feature alignment (uda/model/loss.py:331-378, loss1 / loss3): the box sum of a window of the feature map around each
// key point into one descriptor per joint, the KL divergence between the channel distributions of two sets of descriptors with
// both gradients, and the backward of the pooling written as a gather.  Features are channels-last ([B][H][W][C], bf16 or fp32):
// the C channels of one pixel are contiguous and every access along them is one 16-byte chunk per lane.  No atomics; every sum
// runs in a fixed order, so two runs give the same bits.
#include <math.h>
#include "common.h"
#include "joint_pool.h"

// The pooling divides every window's sum by the launch's one divisor, an empty window's zeros included.
struct jfa_divisor {
  float divisor;
  __device__ bool zero(const joint_win&) const { return false; }
  __device__ float of(const joint_win&) const { return divisor; }
};

// The gather's table: gd[j][c] = g[b][j][c] / divisor.
struct jfa_grad {
  static constexpr const char* GRAD = "grad_desc";
  static constexpr bool BLEND = false;
  static constexpr const float* blend = nullptr;
  const float* g;                     // [B][K][C]
  float divisor;
  __device__ void fill(float* gd, const joint_win*, int b, int K, int C, int c0, int CT) const {
    for (int e = threadIdx.x; e < K * CT; e += JOINT_T) {
      const int j = e / CT, c = e - j * CT;
      gd[j * JOINT_CT + c] = g[((long)b * K + j) * C + c0 + c] / divisor;
    }
  }
};

// nullptr, or the complaint about a divisor that is not a positive finite number
static const char* jfa_divisor_check(const char* who, float divisor) {
  static thread_local char msg[96];
  if (divisor > 0.f && isfinite(divisor)) return nullptr;
  snprintf(msg, sizeof(msg), "%s: divisor=%g must be positive", who, (double)divisor);
  return msg;
}

// ---------------------------------------------------------------- KL between the channel distributions
// One wave per row (b, j) of a, b [rows][C]: lp = log_softmax(a), q = (b + 1e-6) / S with S = sum_c (b_c + 1e-6),
// row = sum_c q_c (log q_c - lp_c);  ga = coef (softmax(a) - q),  gb = coef ((log q - lp) - row) / S.  Lane l owns the 16-byte
// chunks l, l + 64, ...; every wave sum is the xor butterfly, the same in every lane.
// The arithmetic behind the fp32 operands is fp64: log q and lp are both near -log C and their difference is what is summed -- a
// row is a few 1e-3 where each term is a few units, so fp32 logarithms (1 ulp of 2 .. 5) leave the loss with 1e-4 relative, more
// than the reference's own fp32 run.  The rows are small (B K C elements, 0.3 M at the workload shape); fp64 costs nothing here.
__global__ __launch_bounds__(JOINT_T) void jfa_kl_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ rows,
                                                        float* __restrict__ ga, float* __restrict__ gb, int nrows, int C, float coef) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * (JOINT_T / WAVE) + (threadIdx.x >> 6);
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
  const double S = wave_sum(s), md = (double)m;
  double z = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c);
    z += (exp((double)va.x - md) + exp((double)va.y - md)) + (exp((double)va.z - md) + exp((double)va.w - md));
  }
  const double lse = log(wave_sum(z));
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
  kl = wave_sum(kl);
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

// ---------------------------------------------------------------- host
extern "C" int mi355_jfa_pool(const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius,
                              float divisor, int rows_by_x, int dtype, void* stream) {
  return joint_pool_launch("jfa_pool", feature, xy, desc, B, K, C, H, W, radius, rows_by_x, dtype, stream, jfa_divisor{divisor},
                           jfa_divisor_check("jfa_pool", divisor));
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
  hipLaunchKernelGGL(jfa_kl_kernel, dim3(cdiv(nrows, JOINT_T / WAVE)), dim3(JOINT_T), 0, s, a, b, rows, grad_a, grad_b, nrows, C, coef);
  MI_CHECK_LAUNCH("jfa_kl");
  return MI355_OK;
}

extern "C" int mi355_jfa_scatter(const float* grad_desc, const float* xy, void* grad_feature, int accumulate, int B, int K, int C, int H,
                                 int W, int radius, float divisor, int rows_by_x, int dtype, void* stream) {
  return joint_gather_launch("jfa_scatter", xy, grad_feature, accumulate, B, K, C, H, W, radius, rows_by_x, dtype, stream,
                             jfa_grad{grad_desc, divisor}, jfa_divisor_check("jfa_scatter", divisor));
}

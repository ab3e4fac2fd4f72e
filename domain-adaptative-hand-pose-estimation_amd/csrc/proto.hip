// Per-joint prototype alignment with running memory (uda/model/loss.py:381-466 and :560-652, lossx / lossx3): the box mean of a
// window of the feature map around each key point, divided by the window's own s_row * s_col; the batch mean of those descriptors
// blended with a memory kept from call to call into one prototype per joint; the KL divergence between the channel distributions
// of two sets of prototypes with both gradients; and the backward of pooling + batch mean + blend written as one gather.
// Features are channels-last ([B][H][W][C], bf16 or fp32), as in jfa.hip.  No atomics; every sum runs in a fixed order, so two
// runs give the same bits.  Nothing here reads device memory on the host or allocates: all of it can be captured into a graph.
#include <math.h>
#include "common.h"
#include "joint_pool.h"

#define PROTO_UNROLL 8                // proto_update: images whose descriptors are loaded before they are added

// The reference's divisor s1 * s2 (:418-419, :425): s = hi - lo + 1 on either axis, ONE MORE than the pixels the half-open slice
// lo:hi sums.  Only asked for a window that is not empty, so both factors are at least 2.
__device__ __forceinline__ float proto_divisor(const joint_win& w) { return (float)((w.r1 - w.r0 + 1) * (w.q1 - w.q0 + 1)); }
__device__ __forceinline__ bool proto_empty(const joint_win& w) { return w.r1 <= w.r0 || w.q1 <= w.q0; }

// The pooling divides by the window's own divisor; an empty window stores zeros (and divides by nothing).
struct proto_window_divisor {
  __device__ bool zero(const joint_win& w) const { return proto_empty(w); }
  __device__ float of(const joint_win& w) const { return proto_divisor(w); }
};

// The gather's table: gd[j][c] = (g[j][c] * (m / B)) / divisor(b, j) -- the prototype gradient [K][C], the same for every image,
// times d P / d desc = m / B, over the window's own divisor (1 for an empty window, which covers no pixel).  m is blend[0] in
// device memory, as in proto_update.
struct proto_grad {
  static constexpr const char* GRAD = "grad_proto";
  static constexpr bool BLEND = true;
  const float* g;                     // [K][C]
  const float* blend;
  int B;
  __device__ void fill(float* gd, const joint_win* win, int, int K, int C, int c0, int CT) const {
    __shared__ float dv[MI355_JFA_MAX_JOINTS];
    const int t = threadIdx.x;
    if (t < K) dv[t] = proto_empty(win[t]) ? 1.f : proto_divisor(win[t]);
    __syncthreads();
    const float fac = blend[0] / (float)B;
    for (int e = t; e < K * CT; e += JOINT_T) {
      const int j = e / CT, c = e - j * CT;
      gd[j * JOINT_CT + c] = (g[(long)j * C + c0 + c] * fac) / dv[j];
    }
  }
};

// ---------------------------------------------------------------- batch mean, blend with the memory, memory update
// One thread per 4 channels of one joint: pbar = (sum_b desc[b][j][c]) / B with b ascending in fp32, P = m pbar + (1 - m) M as two
// products and one sum (:436-437, :448), stored to `proto` and to the memory itself.  blend = {m, 1 - m} sits in device memory
// (the host rounds each of the two once, as the reference's Python floats are rounded where they meet the tensor), so a captured
// graph follows a changed value.  The work is a few thousand threads of load latency: one wave a block spreads them over the CUs,
// and each thread has the loads of PROTO_UNROLL images in flight before it adds them.
__global__ __launch_bounds__(WAVE) void proto_update_kernel(const float* __restrict__ desc, float* __restrict__ mem, const float* __restrict__ blend,
                                                            float* __restrict__ proto, int B, int KC) {
  const int i = 4 * (blockIdx.x * WAVE + threadIdx.x);
  if (i >= KC) return;
  float4 s = *reinterpret_cast<const float4*>(desc + i);
  int b = 1;
  for (; b + PROTO_UNROLL <= B; b += PROTO_UNROLL) {          // the loads of a group are in flight together; the sum stays b ascending
    float4 v[PROTO_UNROLL];
#pragma unroll
    for (int u = 0; u < PROTO_UNROLL; ++u) v[u] = *reinterpret_cast<const float4*>(desc + (long)(b + u) * KC + i);
#pragma unroll
    for (int u = 0; u < PROTO_UNROLL; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
  }
  for (; b < B; ++b) {
    const float4 v = *reinterpret_cast<const float4*>(desc + (long)b * KC + i);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float n = (float)B, m = blend[0], om = blend[1];
  const float4 o = *reinterpret_cast<const float4*>(mem + i);
  const float4 p = make_float4(m * (s.x / n) + om * o.x, m * (s.y / n) + om * o.y, m * (s.z / n) + om * o.z, m * (s.w / n) + om * o.w);
  *reinterpret_cast<float4*>(proto + i) = p;
  *reinterpret_cast<float4*>(mem + i) = p;
}

// ---------------------------------------------------------------- KL between the channel distributions of the prototypes
// One wave per joint of pt, ps [K][C]: lp = log_softmax(pt);  mode 0 (`kl`, lossx :455-466): q = ps / S, S = sum_c ps_c;  mode 1
// (`softkl`, lossx3 :645): q = softmax(ps).  row = sum_c q_c (log q_c - lp_c), an element with q_c = 0 adding nothing (as
// KLDivLoss's xlogy).  gt = coef (softmax(pt) - q);  gs = coef ((log q - lp) - row) / S in mode 0 (0 for an element with
// q_c = 0, where the reference's autograd gives -inf) and coef q ((log q - lp) - row) in mode 1.  Mode 0, S <= 0 or NaN: row 0
// and zero gradients (the reference returns NaN for an all-zero source prototype).  fp64 behind the fp32 operands, as jfa_kl:
// the row is a small difference of large logarithms.
__global__ __launch_bounds__(JOINT_T) void proto_kl_kernel(const float* __restrict__ pt, const float* __restrict__ ps, float* __restrict__ rows,
                                                            float* __restrict__ gt, float* __restrict__ gs, int K, int C, int mode, float coef) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * (JOINT_T / WAVE) + (threadIdx.x >> 6);
  if (row >= K) return;
  const float* __restrict__ ar = pt + (long)row * C;
  const float* __restrict__ br = ps + (long)row * C;
  float ma = -INFINITY, mb = -INFINITY;
  double s = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    ma = fmaxf(fmaxf(fmaxf(ma, va.x), fmaxf(va.y, va.z)), va.w);
    mb = fmaxf(fmaxf(fmaxf(mb, vb.x), fmaxf(vb.y, vb.z)), vb.w);
    s += ((double)vb.x + (double)vb.y) + ((double)vb.z + (double)vb.w);
  }
  ma = wave_max(ma);
  mb = wave_max(mb);
  const double mad = (double)ma, mbd = (double)mb;
  double S = wave_sum(s), za = 0.0, zb = 0.0;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    za += (exp((double)va.x - mad) + exp((double)va.y - mad)) + (exp((double)va.z - mad) + exp((double)va.w - mad));
    if (mode) zb += (exp((double)vb.x - mbd) + exp((double)vb.y - mbd)) + (exp((double)vb.z - mbd) + exp((double)vb.w - mbd));
  }
  const double lsa = log(wave_sum(za)), lsb = mode ? log(wave_sum(zb)) : 0.0;
  const bool dead = !mode && !(S > 0.0);            // (also a NaN sum)
  double kl = 0.0;
  for (int c = 4 * lane; c < C && !dead; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    const float x[4] = {va.x, va.y, va.z, va.w}, y[4] = {vb.x, vb.y, vb.z, vb.w};
    double e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double lp = ((double)x[i] - mad) - lsa;
      const double lq = mode ? ((double)y[i] - mbd) - lsb : log((double)y[i] / S);
      const double q = mode ? exp(lq) : (double)y[i] / S;
      e[i] = q == 0.0 ? 0.0 : q * (lq - lp);
    }
    kl += (e[0] + e[1]) + (e[2] + e[3]);
  }
  kl = wave_sum(kl);
  if (lane == 0) rows[row] = (float)kl;
  if (!gt && !gs) return;
  const double cf = (double)coef;
  for (int c = 4 * lane; c < C; c += 4 * WAVE) {
    const float4 va = *reinterpret_cast<const float4*>(ar + c), vb = *reinterpret_cast<const float4*>(br + c);
    const float x[4] = {va.x, va.y, va.z, va.w}, y[4] = {vb.x, vb.y, vb.z, vb.w};
    float da[4], db[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (dead) { da[i] = 0.f; db[i] = 0.f; continue; }
      const double lp = ((double)x[i] - mad) - lsa;
      const double lq = mode ? ((double)y[i] - mbd) - lsb : log((double)y[i] / S);
      const double q = mode ? exp(lq) : (double)y[i] / S;
      da[i] = (float)(cf * (exp(lp) - q));
      db[i] = q == 0.0 ? 0.f : (float)(mode ? cf * (q * ((lq - lp) - kl)) : cf * (((lq - lp) - kl) / S));
    }
    if (gt) *reinterpret_cast<float4*>(gt + (long)row * C + c) = make_float4(da[0], da[1], da[2], da[3]);
    if (gs) *reinterpret_cast<float4*>(gs + (long)row * C + c) = make_float4(db[0], db[1], db[2], db[3]);
  }
}

// ---------------------------------------------------------------- host
extern "C" int mi355_proto_pool(const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius,
                                int rows_by_x, int dtype, void* stream) {
  return joint_pool_launch("proto_pool", feature, xy, desc, B, K, C, H, W, radius, rows_by_x, dtype, stream, proto_window_divisor{});
}

extern "C" int mi355_proto_update(const float* desc, float* memory, const float* blend, float* proto, int B, int K, int C, void* stream) {
  if (!desc || !memory || !blend || !proto) MI_FAIL(MI355_EINVAL, "proto_update: null pointer");
  if (((uintptr_t)desc | (uintptr_t)memory | (uintptr_t)proto) & 15) MI_FAIL(MI355_EINVAL, "proto_update: desc, memory and proto must be 16-byte aligned");
  if ((uintptr_t)blend & 3) MI_FAIL(MI355_EINVAL, "proto_update: blend must be 4-byte aligned");
  if (B < 1 || B > 65535) MI_FAIL(MI355_EINVAL, "proto_update: B=%d (1 .. 65535)", B);
  if (K < 1 || K > MI355_JFA_MAX_JOINTS) MI_FAIL(MI355_EINVAL, "proto_update: K=%d (1 .. %d joints)", K, MI355_JFA_MAX_JOINTS);
  if (C < 8 || C % 8 || C > (1 << 24)) MI_FAIL(MI355_EINVAL, "proto_update: C=%d (a multiple of 8, 8 .. 2^24)", C);
  if (memory == proto) MI_FAIL(MI355_EINVAL, "proto_update: proto must not be the memory itself");
  hipStream_t s = as_stream(stream);
  char lab[96];
  snprintf(lab, sizeof(lab), "proto_update B%d K%d C%d", B, K, C);
  ProfScope ps(s, 0.0, 4.0 * K * C * (B + 3.0), 2, lab);
  hipLaunchKernelGGL(proto_update_kernel, dim3(cdiv((long)K * C / 4, WAVE)), dim3(WAVE), 0, s, desc, memory, blend, proto, B, K * C);
  MI_CHECK_LAUNCH("proto_update");
  return MI355_OK;
}

extern "C" int mi355_proto_kl(const float* proto_t, const float* proto_s, float* rows, float* grad_t, float* grad_s, int K, int C, int mode,
                              float coef, void* stream) {
  if (!proto_t || !proto_s || !rows) MI_FAIL(MI355_EINVAL, "proto_kl: null pointer");
  if (((uintptr_t)proto_t | (uintptr_t)proto_s | (uintptr_t)grad_t | (uintptr_t)grad_s) & 15)
    MI_FAIL(MI355_EINVAL, "proto_kl: the prototypes and the gradients must be 16-byte aligned");
  if ((uintptr_t)rows & 3) MI_FAIL(MI355_EINVAL, "proto_kl: rows must be 4-byte aligned");
  if (K < 1) MI_FAIL(MI355_EINVAL, "proto_kl: K=%d", K);
  if (C < 8 || C % 8) MI_FAIL(MI355_EINVAL, "proto_kl: C=%d (a multiple of 8, at least 8)", C);
  if (mode != MI355_PROTO_KL && mode != MI355_PROTO_SOFTKL) MI_FAIL(MI355_EINVAL, "proto_kl: mode=%d (0 kl, 1 softkl)", mode);
  if (!isfinite(coef)) MI_FAIL(MI355_EINVAL, "proto_kl: coef=%g must be finite", (double)coef);
  hipStream_t s = as_stream(stream);
  char lab[96];
  snprintf(lab, sizeof(lab), "proto_kl K%d C%d %s grads%d%d", K, C, mode ? "softkl" : "kl", grad_t ? 1 : 0, grad_s ? 1 : 0);
  ProfScope ps(s, 0.0, 4.0 * K * C * (2.0 + (grad_t ? 1 : 0) + (grad_s ? 1 : 0)), 2, lab);
  hipLaunchKernelGGL(proto_kl_kernel, dim3(cdiv(K, JOINT_T / WAVE)), dim3(JOINT_T), 0, s, proto_t, proto_s, rows, grad_t, grad_s, K, C, mode, coef);
  MI_CHECK_LAUNCH("proto_kl");
  return MI355_OK;
}

extern "C" int mi355_proto_scatter(const float* grad_proto, const float* xy, const float* blend, void* grad_feature, int accumulate, int B, int K,
                                   int C, int H, int W, int radius, int rows_by_x, int dtype, void* stream) {
  return joint_gather_launch("proto_scatter", xy, grad_feature, accumulate, B, K, C, H, W, radius, rows_by_x, dtype, stream,
                             proto_grad{grad_proto, blend, B});
}

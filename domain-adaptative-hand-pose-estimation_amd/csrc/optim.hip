// SGD (momentum, weight decay, Nesterov) over a flat fp32 range + the low-precision parameter copy,
// and the plain cast kernel.  Pure streaming: float4 per lane.
#include "common.h"

// torch.optim.SGD semantics (train1.py:141-148): g' = g + wd*p; buf = mu*buf + g' (buf starts at 0, which equals
// torch's "first step: buf = g'"); p -= lr * (nesterov ? g' + mu*buf : buf)
template <typename L>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                   const float* __restrict__ lr_dev, float mu, float wd, int nesterov, L* __restrict__ lowp) {
  const float lr = *lr_dev;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv = reinterpret_cast<float4*>(buf)[i];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w}; const float gg[4] = {gv.x, gv.y, gv.z, gv.w}; float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = gg[e] + wd * pp[e];
      bb[e] = mu * bb[e] + d;
      pp[e] -= lr * (nesterov ? d + mu * bb[e] : bb[e]);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(buf)[i] = make_float4(bb[0], bb[1], bb[2], bb[3]);
    if (lowp) {
#pragma unroll
      for (int e = 0; e < 4; ++e) lowp[4 * i + e] = (L)pp[e];
    }
  }
  // tail
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = g[i] + wd * p[i];
    const float b = mu * buf[i] + d; buf[i] = b;
    const float np = p[i] - lr * (nesterov ? d + mu * b : b); p[i] = np;
    if (lowp) lowp[i] = (L)np;
  }
}

extern "C" int mi355_sgd_nesterov(float* p, const float* g, float* buf, long n, const float* lr_dev, float momentum, float wd,
                                  int nesterov, void* p_lowp, void* stream) {
  if (!p || !g || !buf || !lr_dev || n < 1) MI_FAIL(MI355_EINVAL, "sgd: bad args");
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) MI_FAIL(MI355_EINVAL, "sgd: pointers must be 16-byte aligned");
  int grid = (int)((n / 4 + 255) / 256); if (grid < 1) grid = 1; if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(sgd_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(stream), p, g, buf, n, lr_dev, momentum, wd, nesterov, (bf16_t*)p_lowp);
  MI_CHECK_LAUNCH("sgd");
  return MI355_OK;
}

template <typename T>
__global__ void cast_kernel(const float* __restrict__ in, T* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (T)in[i];
}
extern "C" int mi355_cast_f32(const float* in, void* out, long n, int dtype, void* stream) {
  if (!in || !out || n < 1) MI_FAIL(MI355_EINVAL, "cast: bad args");
  int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096;
  if (dtype == MI355_BF16) hipLaunchKernelGGL(cast_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(stream), in, (bf16_t*)out, n);
  else if (dtype == MI355_F32) hipLaunchKernelGGL(cast_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream), in, (float*)out, n);
  else MI_FAIL(MI355_EINVAL, "cast: bad dtype");
  MI_CHECK_LAUNCH("cast");
  return MI355_OK;
}

// EMA ("mean teacher") update of uda/model/loss.py:252-261 (update_ema_variables5; train1.py:461):
//   v_ema = v_ema * m + (1. - m) * v_main        -- three fp32 roundings: a = fl(e*k), b = fl(p*c), e' = fl(a + b)
// k = float32(m) and c = float32(1.0 - m) are read from coef_dev[0..1] (a replayed graph sees the warm-up schedule).  An FMA
// form differs from torch in about a quarter of the elements, so the multiplies and the add never contract, whatever the
// build's flags say.
__device__ __forceinline__ float ema1(float e, float p, float k, float c) {
#pragma clang fp contract(off)
  const float a = e * k;
  const float b = p * c;
  return a + b;
}

// Flat range (the mirror of one FusedSGD group): pure stream, float4 per lane, grid-stride, scalar tail.  p is only read.
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ e, const float* __restrict__ p, long n,
                                                   const float* __restrict__ coef_dev) {
  const float k = coef_dev[0], c = coef_dev[1];
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 ev = reinterpret_cast<float4*>(e)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    reinterpret_cast<float4*>(e)[i] = make_float4(ema1(ev.x, pv.x, k, c), ema1(ev.y, pv.y, k, c), ema1(ev.z, pv.z, k, c),
                                                  ema1(ev.w, pv.w, k, c));
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) e[i] = ema1(e[i], p[i], k, c);
}

extern "C" int mi355_ema_update(float* e, const float* p, long n, const float* coef_dev, void* stream) {
  if (!e || !p || !coef_dev || n < 1) MI_FAIL(MI355_EINVAL, "ema_update: bad args");
  if (((uintptr_t)e | (uintptr_t)p) & 15) MI_FAIL(MI355_EINVAL, "ema_update: pointers must be 16-byte aligned");
  int grid = (int)((n / 4 + 255) / 256); if (grid < 1) grid = 1; if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(ema_kernel, dim3(grid), dim3(256), 0, as_stream(stream), e, p, n, coef_dev);
  MI_CHECK_LAUNCH("ema_update");
  return MI355_OK;
}

// Everything that is not in flat storage (BatchNorm running statistics, parameters FusedSGD never laid out, the
// num_batches_tracked counters) in ONE launch: records live in device memory, block b finds its record by binary search over
// the records' first-block prefix (as mi355_pack_weights_batched) and handles MI355_EMA_CHUNK of its elements.
__global__ __launch_bounds__(256) void ema_batched_kernel(const mi355_ema_item* __restrict__ items, int nitems,
                                                           const float* __restrict__ coef_dev) {
  int lo = 0, hi = nitems - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  const mi355_ema_item it = items[lo];
  const long i0 = (long)(b - it.blk0) * MI355_EMA_CHUNK;
  const long i1 = i0 + MI355_EMA_CHUNK < it.n ? i0 + MI355_EMA_CHUNK : it.n;
  if (it.kind == MI355_EMA_COPY64) {
    const long long* __restrict__ s = reinterpret_cast<const long long*>(it.src);
    long long* __restrict__ d = reinterpret_cast<long long*>(it.dst);
    for (long i = i0 + threadIdx.x; i < i1; i += 256) d[i] = s[i];
  } else {
    const float k = coef_dev[0], c = coef_dev[1];
    const float* __restrict__ s = reinterpret_cast<const float*>(it.src);
    float* __restrict__ d = reinterpret_cast<float*>(it.dst);
    for (long i = i0 + threadIdx.x; i < i1; i += 256) d[i] = ema1(d[i], s[i], k, c);
  }
}

extern "C" int mi355_ema_update_batched(const mi355_ema_item* items_dev, int count, int total_blocks, const float* coef_dev,
                                        void* stream) {
  if (!items_dev || !coef_dev || count < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "ema_update_batched: bad args");
  hipLaunchKernelGGL(ema_batched_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, count, coef_dev);
  MI_CHECK_LAUNCH("ema_update_batched");
  return MI355_OK;
}

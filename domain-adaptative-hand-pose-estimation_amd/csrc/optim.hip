// SGD (momentum, weight decay, Nesterov) over a flat fp32 range + the low-precision parameter copy,
// Adam / AdamW over a table of parameters, the gradient norm, the EMA update and the plain cast kernel.  Pure streaming: float4 per lane.
#include "common.h"
#include "adam_slice.h"

// torch.optim.SGD semantics (train1.py:141-148): g' = g + wd*p; buf = mu*buf + g' (buf starts at 0, which equals
// torch's "first step: buf = g'"); p -= lr * (nesterov ? g' + mu*buf : buf)
// CLIP (mi355_sgd_nesterov_clipped): the same step on g_c = fl32(g * coef), coef and skip read once per block from the record
// mi355_grad_clip_coef wrote; with skip set the block returns before its first store.
__device__ __forceinline__ float clip1(float g, float coef) {
#pragma clang fp contract(off)
  const float gc = g * coef;          // rounded on its own: never contracted into gc + wd * p
  return gc;
}

template <typename L, bool CLIP>
__device__ __forceinline__ void sgd_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                         const float* __restrict__ lr_dev, float mu, float wd, int nesterov, L* __restrict__ lowp,
                                         const mi355_clip_rec* __restrict__ rec) {
  float coef = 1.f;
  if constexpr (CLIP) {
    if (rec->skip) return;
    coef = rec->coef;
  }
  const float lr = *lr_dev;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv = reinterpret_cast<float4*>(buf)[i];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w}; float gg[4] = {gv.x, gv.y, gv.z, gv.w}; float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (CLIP) gg[e] = clip1(gg[e], coef);
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
    const float gi = CLIP ? clip1(g[i], coef) : g[i];
    const float d = gi + wd * p[i];
    const float b = mu * buf[i] + d; buf[i] = b;
    const float np = p[i] - lr * (nesterov ? d + mu * b : b); p[i] = np;
    if (lowp) lowp[i] = (L)np;
  }
}

template <typename L>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                   const float* __restrict__ lr_dev, float mu, float wd, int nesterov, L* __restrict__ lowp) {
  sgd_body<L, false>(p, g, buf, n, lr_dev, mu, wd, nesterov, lowp, nullptr);
}

template <typename L>
__global__ __launch_bounds__(256) void sgd_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                           const float* __restrict__ lr_dev, float mu, float wd, int nesterov,
                                                           L* __restrict__ lowp, const mi355_clip_rec* __restrict__ rec) {
  sgd_body<L, true>(p, g, buf, n, lr_dev, mu, wd, nesterov, lowp, rec);
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

extern "C" int mi355_sgd_nesterov_clipped(float* p, const float* g, float* buf, long n, const float* lr_dev, const mi355_clip_rec* rec_dev,
                                          float momentum, float wd, int nesterov, void* p_lowp, void* stream) {
  if (!p || !g || !buf || !lr_dev || !rec_dev) MI_FAIL(MI355_EINVAL, "sgd_clipped: null pointer");
  if (n < 1) MI_FAIL(MI355_EINVAL, "sgd_clipped: n=%ld", n);
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) MI_FAIL(MI355_EINVAL, "sgd_clipped: pointers must be 16-byte aligned");
  if ((uintptr_t)rec_dev & 7) MI_FAIL(MI355_EINVAL, "sgd_clipped: the record must be 8-byte aligned");
  int grid = (int)((n / 4 + 255) / 256); if (grid < 1) grid = 1; if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(sgd_clipped_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(stream), p, g, buf, n, lr_dev, momentum, wd, nesterov,
                     (bf16_t*)p_lowp, rec_dev);
  MI_CHECK_LAUNCH("sgd_clipped");
  return MI355_OK;
}

// ---- global gradient norm (mi355pose.h: mi355_grad_sumsq_batched / mi355_grad_clip_coef) ---------------------------------------
// wave_sum of common.h on doubles: the same fixed xor tree, so every lane ends with the same bits.
__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// 4 waves; the result is valid in thread 0 only (the one that stores it): waves are added in wave order.
__device__ inline double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Block b finds its item by binary search over blk0 (as ema_batched_kernel) and owns elements [i0, i0 + len) of it, at most
// MI355_GN_CHUNK: GN_V float4 per lane, lane-interleaved (float4 number j * 256 + lane of the slice), ALL issued before the first
// use -- 64 KB in flight per block -- then squared and added in fp64 in index order (the square of an fp32 value is exact in
// fp64, so a contracted and an uncontracted build give the same bits).  The up to three floats behind the last whole quad go to
// lanes 0..2.
#define GN_V (MI355_GN_CHUNK / 4 / 256)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const mi355_gn_item* __restrict__ items, int nitems, double* __restrict__ partials) {
  __shared__ double red[4];
  int lo = 0, hi = nitems - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  const mi355_gn_item it = items[lo];
  const long i0 = (long)(b - it.blk0) * MI355_GN_CHUNK;
  const long len = it.n - i0 < MI355_GN_CHUNK ? it.n - i0 : MI355_GN_CHUNK;      // (<= 0 only for a malformed table: nothing is read)
  const float* __restrict__ g = it.g + i0;
  const int n4 = len > 0 ? (int)(len >> 2) : 0;
  float4 v[GN_V];
  if (n4 > 0) {
    // a quad past the slice's end re-reads the slice's last whole quad (a clamped address, no branch: the loads stay
    // back to back) and is zeroed below
#pragma unroll
    for (int j = 0; j < GN_V; ++j) {
      const int q = j * 256 + threadIdx.x;
      v[j] = reinterpret_cast<const float4*>(g)[q < n4 ? q : n4 - 1];
    }
  }
  const int t = (n4 << 2) + threadIdx.x;
  const float tail = (threadIdx.x < 3 && t < len) ? g[t] : 0.f;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < GN_V; ++j) {
    if (j * 256 + (int)threadIdx.x >= n4) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    acc += (double)v[j].x * (double)v[j].x; acc += (double)v[j].y * (double)v[j].y;
    acc += (double)v[j].z * (double)v[j].z; acc += (double)v[j].w * (double)v[j].w;
  }
  acc += (double)tail * (double)tail;
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) partials[b] = s;
}

extern "C" int mi355_grad_sumsq_batched(const mi355_gn_item* items_dev, int count, int total_blocks, double* partials_dev, void* stream) {
  if (!items_dev || !partials_dev) MI_FAIL(MI355_EINVAL, "grad_sumsq_batched: null pointer");
  if (count < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "grad_sumsq_batched: count=%d total_blocks=%d", count, total_blocks);
  if (total_blocks < count) MI_FAIL(MI355_EINVAL, "grad_sumsq_batched: total_blocks=%d for count=%d items (each owns a block)", total_blocks, count);
  if (((uintptr_t)items_dev | (uintptr_t)partials_dev) & 7) MI_FAIL(MI355_EINVAL, "grad_sumsq_batched: items and partials must be 8-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, count, partials_dev);
  MI_CHECK_LAUNCH("grad_sumsq_batched");
  return MI355_OK;
}

// One block: lane t adds partials[t], partials[t + 256], ... in that order, then the tree; thread 0 fills the record.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ partials, int nblocks, mi355_clip_rec* __restrict__ rec) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) acc += partials[i];
  const double sumsq = block_sum_f64(acc, red);
  if (threadIdx.x != 0) return;
  rec->sumsq = sumsq;
  if (!isfinite(sumsq)) {
    rec->norm = (float)sumsq;          // inf or NaN, as torch's total_norm would be
    rec->coef = 0.f;
    rec->skip = 1;
    rec->n_skipped = rec->n_skipped + 1;
  } else {
    const float norm = (float)__dsqrt_rn(sumsq);
    rec->norm = norm;
    rec->coef = fminf(1.0f, __fdiv_rn(rec->max_norm, norm + 1e-6f));
    rec->skip = 0;
  }
}

extern "C" int mi355_grad_clip_coef(const double* partials_dev, int total_blocks, mi355_clip_rec* rec_dev, void* stream) {
  if (!partials_dev || !rec_dev) MI_FAIL(MI355_EINVAL, "grad_clip_coef: null pointer");
  if (total_blocks < 1) MI_FAIL(MI355_EINVAL, "grad_clip_coef: total_blocks=%d", total_blocks);
  if (((uintptr_t)partials_dev | (uintptr_t)rec_dev) & 7) MI_FAIL(MI355_EINVAL, "grad_clip_coef: partials and the record must be 8-byte aligned");
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials_dev, total_blocks, rec_dev);
  MI_CHECK_LAUNCH("grad_clip_coef");
  return MI355_OK;
}

// ---- Adam / AdamW (mi355pose.h: mi355_adam_step_batched / mi355_adam_tick_batched) ---------------------------------------------
// The per-block scalars of one item; every fp32 operation of adam1 is rounded on its own, whatever the build's flags say.  sqrtf
// and `/` are the correctly rounded forms under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (__fsqrt_rn is the
// hardware's 1-ulp root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, which this build does not do).
struct adam_consts { float coef, wd, decay, omb1, beta2, omb2, step_size, bc2s, eps; int clip, l2, decoupled; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const adam_consts& c) {
#pragma clang fp contract(off)
  float gc = c.clip ? g * c.coef : g;
  float pp = p;
  if (c.decoupled) pp = pp * c.decay;
  else if (c.l2) { const float t = c.wd * pp; gc = gc + t; }
  const float d = gc - m;
  const float e = c.omb1 * d;
  const float mm = m + e;
  const float a = c.beta2 * v;
  const float s = c.omb2 * gc;
  const float q = s * gc;
  const float vv = a + q;
  const float den = sqrtf(vv) / c.bc2s + c.eps;
  const float u = c.step_size * (mm / den);
  p = pp - u; m = mm; v = vv;
}

// x^t for a whole t >= 1 by squaring in fp64: exact where the powers are (t = 1, dyadic x), otherwise within a few dozen fp64 ulps
// of pow() -- far below the fp32 rounding of the values derived from it -- and the same bits on every lane and in every launch.
__device__ __forceinline__ double ipow64(double x, unsigned t) {
  double r = 1.0;
  while (t) { if (t & 1u) r *= x; x *= x; t >>= 1; }
  return r;
}

// Block b owns elements [i0, i0 + len) of its item (adam_slice.h), len <= MI355_ADAM_CHUNK: float4 number j * 256 + lane of the
// slice per pass, then the up to three floats behind the last whole quad in lanes 0..2.  step and lr are only read.  The four
// streams' addresses come out of the table, so they are told to be global memory (address space 1): global_load / global_store
// instead of flat ones, which would count against the LDS counter as well.
typedef float adam_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) adam_v4 adam_gv4;
typedef __attribute__((address_space(1))) float adam_gf;
__global__ __launch_bounds__(256) void adam_step_kernel(const mi355_adam_item* __restrict__ items, int nitems,
                                                         const mi355_clip_rec* __restrict__ rec) {
  adam_consts c;
  c.clip = rec != nullptr; c.coef = 1.f;
  if (rec) {
    if (rec->skip) return;
    c.coef = rec->coef;
  }
  const adam_slice sl = adam_block_slice(items, nitems, blockIdx.x);
  if (sl.len <= 0) return;               // (only for a malformed table: nothing is touched)
  const mi355_adam_item it = items[sl.item];
  const long i0 = sl.i0;
  const int len = sl.len;
  {
    const unsigned t = (unsigned)*it.step + 1u;
    const double lr = (double)*it.lr;
    const double bc1 = 1.0 - ipow64(it.beta1, t);
    const double bc2 = 1.0 - ipow64(it.beta2, t);
    c.step_size = (float)(lr / bc1);
    c.bc2s = (float)sqrt(bc2);
    c.decay = (float)(1.0 - lr * (double)it.wd);
    c.omb1 = (float)(1.0 - it.beta1);
    c.omb2 = (float)(1.0 - it.beta2);
    c.beta2 = (float)it.beta2; c.eps = it.eps; c.wd = it.wd;
    c.decoupled = it.decoupled != 0;
    c.l2 = !c.decoupled && it.wd != 0.f;
  }
  adam_gf* __restrict__ p = (adam_gf*)(it.p + i0);
  const adam_gf* __restrict__ g = (const adam_gf*)(it.g + i0);
  adam_gf* __restrict__ m = (adam_gf*)(it.m + i0);
  adam_gf* __restrict__ v = (adam_gf*)(it.v + i0);
  const int n4 = len >> 2;
  for (int q = threadIdx.x; q < n4; q += 256) {
    adam_v4 pv = ((const adam_gv4*)p)[q];
    const adam_v4 gv = ((const adam_gv4*)g)[q];
    adam_v4 mv = ((const adam_gv4*)m)[q];
    adam_v4 vv = ((const adam_gv4*)v)[q];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w}; const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float mm[4] = {mv.x, mv.y, mv.z, mv.w}; float ww[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) adam1(pp[e], gg[e], mm[e], ww[e], c);
    pv.x = pp[0]; pv.y = pp[1]; pv.z = pp[2]; pv.w = pp[3];
    mv.x = mm[0]; mv.y = mm[1]; mv.z = mm[2]; mv.w = mm[3];
    vv.x = ww[0]; vv.y = ww[1]; vv.z = ww[2]; vv.w = ww[3];
    ((adam_gv4*)p)[q] = pv; ((adam_gv4*)m)[q] = mv; ((adam_gv4*)v)[q] = vv;
  }
  const int t = (n4 << 2) + threadIdx.x;
  if (threadIdx.x < 3 && t < len) {
    float pt = p[t], mt = m[t], vt = v[t];
    adam1(pt, g[t], mt, vt, c);
    p[t] = pt; m[t] = mt; v[t] = vt;
  }
}

// One thread per item: *step += 1 (fp32: exact up to 2^24), behind the step launch on the same stream.
__global__ __launch_bounds__(256) void adam_tick_kernel(const mi355_adam_item* __restrict__ items, int nitems,
                                                         const mi355_clip_rec* __restrict__ rec) {
  if (rec && rec->skip) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nitems) { float* s = items[i].step; *s = *s + 1.0f; }
}

extern "C" int mi355_adam_step_batched(const mi355_adam_item* items_dev, int count, int total_blocks, const mi355_clip_rec* rec_dev,
                                       void* stream) {
  if (!items_dev) MI_FAIL(MI355_EINVAL, "adam_step_batched: null table");
  if (count < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "adam_step_batched: count=%d total_blocks=%d", count, total_blocks);
  if (total_blocks < count) MI_FAIL(MI355_EINVAL, "adam_step_batched: total_blocks=%d for count=%d items (each owns a block)", total_blocks, count);
  if ((uintptr_t)items_dev & 7) MI_FAIL(MI355_EINVAL, "adam_step_batched: the table must be 8-byte aligned");
  if ((uintptr_t)rec_dev & 7) MI_FAIL(MI355_EINVAL, "adam_step_batched: the record must be 8-byte aligned");
  hipLaunchKernelGGL(adam_step_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, count, rec_dev);
  MI_CHECK_LAUNCH("adam_step_batched");
  return MI355_OK;
}

extern "C" int mi355_adam_tick_batched(const mi355_adam_item* items_dev, int count, const mi355_clip_rec* rec_dev, void* stream) {
  if (!items_dev) MI_FAIL(MI355_EINVAL, "adam_tick_batched: null table");
  if (count < 1) MI_FAIL(MI355_EINVAL, "adam_tick_batched: count=%d", count);
  if ((uintptr_t)items_dev & 7) MI_FAIL(MI355_EINVAL, "adam_tick_batched: the table must be 8-byte aligned");
  if ((uintptr_t)rec_dev & 7) MI_FAIL(MI355_EINVAL, "adam_tick_batched: the record must be 8-byte aligned");
  hipLaunchKernelGGL(adam_tick_kernel, dim3((unsigned)(((long)count + 255) / 256)), dim3(256), 0, as_stream(stream), items_dev, count, rec_dev);
  MI_CHECK_LAUNCH("adam_tick_batched");
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

// Mean-teacher consistency (train1.py:351-364, uda/model/loss.py:265-297): the device-side BatchNorm fold that keeps the
// teacher's one-launch eval convs fed at fixed addresses, and the masked MSE heat-map loss with its gradient.
// Both are pure streams: 16-byte accesses where the addresses allow, scalar otherwise.
#include "common.h"

// ---------------------------------------------------------------- BatchNorm fold
// torch's `gamma / torch.sqrt(var + eps)` rounding for rounding: one add, a correctly rounded square root and divide.
__device__ __forceinline__ float fold_scale(const mi355_fold_item& it, int c) {
  return it.gamma[c] / sqrtf(it.var[c] + it.eps);
}
// `w * scale`, `beta - mean * scale (+ cbias * scale)`: every product and sum rounded on its own, whatever the build's flags say
__device__ __forceinline__ float fold_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fold_shift(float beta, float mean, float scale, const float* cbias, int c) {
#pragma clang fp contract(off)
  const float ms = mean * scale;
  float sh = beta - ms;
  if (cbias) { const float bs = cbias[c] * scale; sh = sh + bs; }
  return sh;
}

// Block b finds its item by binary search over the first-block prefix (as mi355_pack_weights_batched) and folds
// MI355_FOLD_CHUNK of its elements.  The scales the chunk needs are computed once per block into LDS: the channels
// [c_lo, c_hi] the chunk spans (axis 0; at most one per element), all I of them (axis 1, I <= MI355_FOLD_CHUNK), or -- axis 1
// with more channels than that -- per element.  The first block of an item also writes its bias.
__global__ __launch_bounds__(256) void bn_fold_batched_kernel(const mi355_fold_item* __restrict__ items, int nitems) {
  __shared__ float sc[MI355_FOLD_CHUNK];
  int lo = 0, hi = nitems - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  const mi355_fold_item it = items[lo];
  const int t = threadIdx.x;
  const long TI = (long)it.T * it.I;
  const long n = (long)it.O * TI;
  const long i0 = (long)(b - it.blk0) * MI355_FOLD_CHUNK;
  const long i1 = i0 + MI355_FOLD_CHUNK < n ? i0 + MI355_FOLD_CHUNK : n;
  const int C = it.axis == 0 ? it.O : it.I;
  if (b == it.blk0)
    for (int c = t; c < C; c += 256) it.out_bias[c] = fold_shift(it.beta[c], it.mean[c], fold_scale(it, c), it.conv_bias, c);
  if (i0 >= n) return;                                      // (cannot happen with a consistent table; checked on the host)
  int c_lo = 0, cached;                                      // sc[c - c_lo] for c_lo <= c < c_lo + cached
  if (it.axis == 0) { c_lo = (int)(i0 / TI); cached = (int)((i1 - 1) / TI) - c_lo + 1; }
  else cached = it.I <= MI355_FOLD_CHUNK ? it.I : 0;
  for (int c = t; c < cached; c += 256) sc[c] = fold_scale(it, c_lo + c);
  __syncthreads();
  const float* __restrict__ w = it.w;
  float* __restrict__ o = it.out_w;
  const int ax = it.axis, I = it.I;
  auto scale_at = [&](long e) -> float {
    const int c = ax == 0 ? (int)(e / TI) : (int)(e % I);
    return cached ? sc[c - c_lo] : fold_scale(it, c);
  };
  // i0 is a multiple of the chunk, so 16-byte alignment of the chunk is that of the two base pointers
  if ((((uintptr_t)w | (uintptr_t)o) & 15) == 0) {
    const long v1 = i0 + ((i1 - i0) & ~3L);
    for (long e = i0 + 4 * t; e < v1; e += 1024) {
      const float4 q = *reinterpret_cast<const float4*>(w + e);
      *reinterpret_cast<float4*>(o + e) = make_float4(fold_mul(q.x, scale_at(e)), fold_mul(q.y, scale_at(e + 1)),
                                                      fold_mul(q.z, scale_at(e + 2)), fold_mul(q.w, scale_at(e + 3)));
    }
    for (long e = v1 + t; e < i1; e += 256) o[e] = fold_mul(w[e], scale_at(e));
  } else {
    for (long e = i0 + t; e < i1; e += 256) o[e] = fold_mul(w[e], scale_at(e));
  }
}

extern "C" int mi355_bn_fold_batched(const mi355_fold_item* items_host, const mi355_fold_item* items_dev, int count,
                                     int total_blocks, void* stream) {
  if (!items_host || !items_dev || count < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "bn_fold_batched: bad args");
  long blk = 0;
  for (int i = 0; i < count; ++i) {
    const mi355_fold_item& it = items_host[i];
    if (!it.w || !it.gamma || !it.beta || !it.mean || !it.var || !it.out_w || !it.out_bias)
      MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d has a null pointer", i);
    if (it.O < 1 || it.T < 1 || it.I < 1) MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d: O=%d T=%d I=%d", i, it.O, it.T, it.I);
    if (it.axis != 0 && it.axis != 1) MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d: axis %d is neither 0 nor 1", i, it.axis);
    if (((uintptr_t)it.w | (uintptr_t)it.gamma | (uintptr_t)it.beta | (uintptr_t)it.mean | (uintptr_t)it.var |
         (uintptr_t)it.conv_bias | (uintptr_t)it.out_w | (uintptr_t)it.out_bias) & 3)
      MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d: pointers must be 4-byte aligned", i);
    const long n = (long)it.O * it.T * it.I;
    if (n > (1L << 40)) MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d too large", i);
    if (it.blk0 != blk) MI_FAIL(MI355_EINVAL, "bn_fold_batched: item %d starts at block %d, the items before it end at %ld", i, it.blk0, blk);
    blk += (n + MI355_FOLD_CHUNK - 1) / MI355_FOLD_CHUNK;
  }
  if (blk != total_blocks) MI_FAIL(MI355_EINVAL, "bn_fold_batched: the table holds %ld blocks, total_blocks is %d", blk, total_blocks);
  char lab[64];
  snprintf(lab, sizeof(lab), "bn_fold items%d blocks%d", count, total_blocks);
  ProfScope ps(as_stream(stream), 0.0, 8.0 * MI355_FOLD_CHUNK * total_blocks, 2, lab);
  hipLaunchKernelGGL(bn_fold_batched_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, count);
  MI_CHECK_LAUNCH("bn_fold_batched");
  return MI355_OK;
}

// ---------------------------------------------------------------- masked MSE over heat-map rows
// One block per row r = b * K + k.  Each lane sums its elements in index order, the block sum is a fixed shuffle tree: the
// same bits on every run.  A row outside the joint mask is written as zeros (sum and gradient) without reading pred / target.
template <bool VEC>
__global__ __launch_bounds__(256) void mse_heatmap_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const mi355_mse_rec* __restrict__ rec, float* __restrict__ rows,
                                                           float* __restrict__ grad, int K, int HW) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const unsigned mask = (unsigned)rec->joint_mask;
  const float gs = rec->grad_scale;
  const bool on = (mask >> (r % K)) & 1u;
  const long base = (long)r * HW;
  const float* __restrict__ p = pred + base;
  const float* __restrict__ q = target + base;
  float* __restrict__ g = grad ? grad + base : nullptr;
  float s = 0.f;
  if (!on) {
    if (g) {
      if (VEC) for (int j = 4 * t; j < HW; j += 1024) *reinterpret_cast<float4*>(g + j) = make_float4(0.f, 0.f, 0.f, 0.f);
      else for (int j = t; j < HW; j += 256) g[j] = 0.f;
    }
  } else if (VEC) {
    for (int j = 4 * t; j < HW; j += 1024) {
      const float4 a = *reinterpret_cast<const float4*>(p + j), c = *reinterpret_cast<const float4*>(q + j);
      const float d0 = a.x - c.x, d1 = a.y - c.y, d2 = a.z - c.z, d3 = a.w - c.w;
      const float e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2, e3 = d3 * d3;
      s = s + e0; s = s + e1; s = s + e2; s = s + e3;
      if (g) *reinterpret_cast<float4*>(g + j) = make_float4(d0 * gs, d1 * gs, d2 * gs, d3 * gs);
    }
  } else {
    for (int j = t; j < HW; j += 256) {
      const float d = p[j] - q[j];
      const float e = d * d;
      s = s + e;
      if (g) g[j] = d * gs;
    }
  }
  s = block_sum<4>(s, red);
  if (t == 0) rows[r] = on ? s : 0.f;
}

extern "C" int mi355_mse_heatmap(const float* pred, const float* target, const mi355_mse_rec* rec_dev, float* rows, float* unit_grad,
                                 int B, int K, int HW, void* stream) {
  if (!pred || !target || !rec_dev || !rows) MI_FAIL(MI355_EINVAL, "mse_heatmap: null pointer");
  if (B < 1 || K < 1 || K > 32) MI_FAIL(MI355_EINVAL, "mse_heatmap: B=%d K=%d (1 <= K <= 32)", B, K);
  if (HW < 1) MI_FAIL(MI355_EINVAL, "mse_heatmap: HW=%d", HW);
  if ((long)B * K > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "mse_heatmap: too many rows");
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)rec_dev | (uintptr_t)rows | (uintptr_t)unit_grad) & 3)
    MI_FAIL(MI355_EINVAL, "mse_heatmap: pointers must be 4-byte aligned");
  char lab[64];
  snprintf(lab, sizeof(lab), "mse_heatmap rows%d HW%d%s", B * K, HW, unit_grad ? " +grad" : "");
  ProfScope ps(as_stream(stream), 0.0, (unit_grad ? 12.0 : 8.0) * B * K * HW, 2, lab);
  const bool vec = HW % 4 == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)unit_grad) & 15) == 0;
  if (vec) hipLaunchKernelGGL(mse_heatmap_kernel<true>, dim3(B * K), dim3(256), 0, as_stream(stream), pred, target, rec_dev, rows, unit_grad, K, HW);
  else hipLaunchKernelGGL(mse_heatmap_kernel<false>, dim3(B * K), dim3(256), 0, as_stream(stream), pred, target, rec_dev, rows, unit_grad, K, HW);
  MI_CHECK_LAUNCH("mse_heatmap");
  return MI355_OK;
}

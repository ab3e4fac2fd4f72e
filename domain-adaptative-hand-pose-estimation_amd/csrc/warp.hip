// Geometric teacher view: the per-sample affine warp of an image batch, the back-warp of the teacher's heat-maps with the
// "peak was inside the teacher's frame" flag, and the MSE over heat-map rows with a per-map weight.  Forward only (the teacher is
// detached).  The arithmetic of both warps is stated in include/mi355pose.h and restated in numpy by tests/warp_ref.py:
// every product and sum rounded on its own, whatever the build's flags say, and no tap read whose weight is exactly 0.
#include "common.h"

static_assert(sizeof(mi355_view_rec) == 72, "mi355_view_rec is three 2 x 3 fp32 matrices");

// fl(fl(fl(a * j) + fl(b * i)) + c)
__device__ __forceinline__ float warp_coord(float a, float b, float c, float j, float i) {
#pragma clang fp contract(off)
  const float p = a * j;
  const float q = b * i;
  const float s = p + q;
  return s + c;
}
__device__ __forceinline__ float warp_blend(float v0, float v1, float f) {
#pragma clang fp contract(off)
  const float om = 1.0f - f;
  const float p = v0 * om;
  const float q = v1 * f;
  return p + q;
}

// One bilinear sample of an H x W plane at (xs, ys); ld(offset) reads element y * W + x of it.  The range test comes before any
// conversion to an integer: a NaN or infinite coordinate gives +0 and nothing is converted out of range.  Inside it x0, y0 lie in
// [-1, W) x [-1, H); a tap at -1 or at W / H has the value +0 and is not read.
template <typename Ld>
__device__ __forceinline__ float warp_sample(const Ld& ld, float xs, float ys, int H, int W) {
#pragma clang fp contract(off)
  if (!(xs > -1.0f && xs < (float)W && ys > -1.0f && ys < (float)H)) return 0.0f;
  const float xf = floorf(xs), yf = floorf(ys);
  const float fx = xs - xf, fy = ys - yf;
  const int x0 = (int)xf, y0 = (int)yf;
  auto row = [&](int y) -> float {
    if (y < 0 || y >= H) return 0.0f;
    const int o = y * W + x0;
    const float v0 = x0 >= 0 ? ld(o) : 0.0f;
    if (fx == 0.0f) return v0;
    const float v1 = x0 + 1 < W ? ld(o + 1) : 0.0f;
    return warp_blend(v0, v1, fx);
  };
  const float r0 = row(y0);
  if (fy == 0.0f) return r0;
  return warp_blend(r0, row(y0 + 1), fy);
}

// ---------------------------------------------------------------- images
// A streaming kernel: every output pixel written once, the taps gathered through the caches (a 256 x 256 plane is 256 KB: L2, not
// LDS).  One block owns a TW x 16 tile of output pixels of one sample, so that its taps come from a compact patch of the input
// whatever the angle, and walks the C planes with the coordinates computed once.  VEC: four columns per lane and one 16-byte
// store (host: W % 4 == 0 and out 16-byte aligned, so every row of every plane is); otherwise one column per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void affine_warp_kernel(const float* __restrict__ x, const mi355_view_rec* __restrict__ recs,
                                                           float* __restrict__ out, int C, int H, int W, int tiles_x, int tiles_y) {
  constexpr int PX = VEC ? 4 : 1, TW = 16 * PX;
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int i = ty * 16 + (threadIdx.x >> 4), j0 = tx * TW + (threadIdx.x & 15) * PX;
  if (i >= H || j0 >= W) return;                         // (VEC: W % 4 == 0, a quad is inside the row or outside it)
  const float* __restrict__ m = recs[b].img;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  float xs[PX], ys[PX];
#pragma unroll
  for (int q = 0; q < PX; ++q) {
    xs[q] = warp_coord(m00, m01, m02, (float)(j0 + q), (float)i);
    ys[q] = warp_coord(m10, m11, m12, (float)(j0 + q), (float)i);
  }
  const long plane = (long)H * W;
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ src = x + ((long)b * C + c) * plane;
    float* __restrict__ dst = out + ((long)b * C + c) * plane + (long)i * W + j0;
    auto ld = [&](int o) -> float { return src[o]; };
    float v[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) v[q] = warp_sample(ld, xs[q], ys[q], H, W);
    if constexpr (VEC) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
  }
}

static bool warp_overlap(const void* p, long np, const void* q, long nq) {     // [p, p + np) and [q, q + nq), in bytes
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

extern "C" int mi355_affine_warp_images(const float* x, const mi355_view_rec* recs, float* out, int B, int C, int H, int W,
                                        void* stream) {
  if (!x || !recs || !out) MI_FAIL(MI355_EINVAL, "affine_warp_images: null pointer (x %p, recs %p, out %p)", (const void*)x, (const void*)recs, (void*)out);
  if (B < 1 || C < 1) MI_FAIL(MI355_EINVAL, "affine_warp_images: B=%d C=%d (each at least 1)", B, C);
  if (H < 1 || W < 1 || H > MI355_WARP_MAX_SIDE || W > MI355_WARP_MAX_SIDE)
    MI_FAIL(MI355_EINVAL, "affine_warp_images: H=%d W=%d outside 1..%d", H, W, MI355_WARP_MAX_SIDE);
  if (((uintptr_t)x | (uintptr_t)recs | (uintptr_t)out) & 3) MI_FAIL(MI355_EINVAL, "affine_warp_images: pointers must be 4-byte aligned");
  if ((long)B * C > (1L << 40) / ((long)H * W)) MI_FAIL(MI355_EINVAL, "affine_warp_images: too large (B=%d C=%d H=%d W=%d)", B, C, H, W);
  const long n = (long)B * C * H * W;
  if (warp_overlap(out, 4 * n, x, 4 * n)) MI_FAIL(MI355_EINVAL, "affine_warp_images: out and x overlap");
  if (warp_overlap(out, 4 * n, recs, (long)sizeof(mi355_view_rec) * B)) MI_FAIL(MI355_EINVAL, "affine_warp_images: out and recs overlap");
  const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const int tw = vec ? 64 : 16;
  const int tiles_x = cdiv(W, tw), tiles_y = cdiv(H, 16);
  const long blocks = (long)B * tiles_x * tiles_y;
  if (blocks > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "affine_warp_images: %ld blocks are beyond the grid", blocks);
  char lab[96];
  snprintf(lab, sizeof(lab), "affine_warp %dx%dx%dx%d%s", B, C, H, W, vec ? "" : " scalar");
  ProfScope ps(as_stream(stream), 0.0, 8.0 * n + (double)sizeof(mi355_view_rec) * B, 2, lab);
  if (vec) hipLaunchKernelGGL(affine_warp_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, recs, out, C, H, W, tiles_x, tiles_y);
  else hipLaunchKernelGGL(affine_warp_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, recs, out, C, H, W, tiles_x, tiles_y);
  MI_CHECK_LAUNCH("affine_warp_images");
  return MI355_OK;
}

// ---------------------------------------------------------------- heat-maps
// mi355_argmax2d's order (heatmap.hip): NaN counts as maximum, on equal values the lower index wins.
__device__ __forceinline__ bool warp_better(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && !bn) || (an && bn && ai < bi);
  return av > bv || (av == bv && ai < bi);
}

constexpr int WU_SCRATCH = 32;                            // floats in front of the staged map: [0,16) wave values, [16,32) wave indices

// One workgroup per map r = b * K + k, flip_decode_kernel's layout: 256 threads, 1024 for maps above 32 KB.  Pass 1 walks the
// teacher's map once: it stages it in LDS (LDS = true: up to 64 KB) and keeps a running (value, index) per thread, folded over
// lanes and waves in mi355_argmax2d's order.  Pass 2 writes every pixel of the back-warped map, its taps read from LDS -- or, LDS =
// false, from global memory through the caches: the same operations, the same bits.  Thread 0 writes the flag and the weight.
template <bool LDS>
__global__ __launch_bounds__(1024) void affine_unwarp_kernel(const float* __restrict__ y, const mi355_view_rec* __restrict__ recs,
                                                              float margin, const float* __restrict__ w_in, float* __restrict__ out,
                                                              float* __restrict__ valid, float* __restrict__ w_out, int K, int h, int w) {
  extern __shared__ __align__(16) float wu_smem[];
  float* sv = wu_smem; int* si = reinterpret_cast<int*>(wu_smem) + 16;
  float* smap = wu_smem + WU_SCRATCH;
  const int hw = h * w, NT = blockDim.x, r = blockIdx.x;
  const float* __restrict__ src = y + (size_t)r * hw;
  float* __restrict__ dst = out + (size_t)r * hw;
  const mi355_view_rec* __restrict__ rec = recs + r / K;
  float bv = -INFINITY; int bi = 0x7fffffff;               // "nothing yet": loses against every real candidate
  for (int i = threadIdx.x; i < hw; i += NT) {
    const float v = src[i];
    if (LDS) smap[i] = v;
    if (warp_better(v, i, bv, bi)) { bv = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (warp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();                                       // the wave results and the staged map
  const float* __restrict__ m = rec->hm;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  auto ld = [&](int o) -> float { return LDS ? smap[o] : src[o]; };
  for (int i = threadIdx.x; i < hw; i += NT) {
    const int py = i / w, px = i - py * w;
    const float xs = warp_coord(m00, m01, m02, (float)px, (float)py);
    const float ys = warp_coord(m10, m11, m12, (float)px, (float)py);
    dst[i] = warp_sample(ld, xs, ys, h, w);
  }
  if (threadIdx.x == 0) {
    bv = sv[0]; bi = si[0];
    for (int q = 1; q < (NT >> 6); ++q) if (warp_better(sv[q], si[q], bv, bi)) { bv = sv[q]; bi = si[q]; }
    // (hw >= 1: bi is a real index.)  The flag is about the location alone.
    const int uy = bi / w, ux = bi - uy * w;
    const float fux = (float)ux, fuy = (float)uy;
    bool ok = fux >= margin && fux <= (float)(w - 1) - margin && fuy >= margin && fuy <= (float)(h - 1) - margin;
    if (ok) {
      const float* __restrict__ v = rec->hm_inv;
      const float qx = warp_coord(v[0], v[1], v[2], fux, fuy);
      const float qy = warp_coord(v[3], v[4], v[5], fux, fuy);
      ok = qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1);
    }
    const float f = ok ? 1.0f : 0.0f;
    valid[r] = f;
    if (w_out) w_out[r] = w_in[r] * f;
  }
}

extern "C" int mi355_affine_unwarp_heatmaps(const float* y, const mi355_view_rec* recs, float margin, const float* w_in, float* out,
                                            float* valid, float* w_out, int B, int K, int h, int w, void* stream) {
  if (!y || !recs || !out || !valid)
    MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: null pointer (y %p, recs %p, out %p, valid %p)", (const void*)y, (const void*)recs, (void*)out, (void*)valid);
  if ((w_in == nullptr) != (w_out == nullptr)) MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: w_in and w_out go together (both or neither)");
  if (B < 1 || K < 1) MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: B=%d K=%d (each at least 1)", B, K);
  if (h < 1 || w < 1 || h > MI355_WARP_MAX_SIDE || w > MI355_WARP_MAX_SIDE)
    MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: h=%d w=%d outside 1..%d", h, w, MI355_WARP_MAX_SIDE);
  if (!(margin >= 0.0f) || margin > 3.0e38f) MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: margin=%g must be finite and >= 0", (double)margin);
  if ((long)B * K > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: too many maps (B=%d K=%d)", B, K);
  if (((uintptr_t)y | (uintptr_t)recs | (uintptr_t)out | (uintptr_t)valid | (uintptr_t)w_in | (uintptr_t)w_out) & 3)
    MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: pointers must be 4-byte aligned");
  const long rows = (long)B * K, hw = (long)h * w, n = rows * hw;
  if (n > (1L << 40)) MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: too large (B=%d K=%d h=%d w=%d)", B, K, h, w);
  const void* in[3] = {y, recs, w_in};
  const long in_bytes[3] = {4 * n, (long)sizeof(mi355_view_rec) * B, w_in ? 4 * rows : 0};
  const void* outs[3] = {out, valid, w_out};
  const long out_bytes[3] = {4 * n, 4 * rows, w_out ? 4 * rows : 0};
  static const char* const in_name[3] = {"y", "recs", "w_in"};
  static const char* const out_name[3] = {"out", "valid", "w_out"};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 3; ++i)
      if (in[i] && warp_overlap(outs[o], out_bytes[o], in[i], in_bytes[i]))
        MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: %s and %s overlap", out_name[o], in_name[i]);
    for (int p = o + 1; p < 3; ++p)
      if (outs[p] && warp_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]))
        MI_FAIL(MI355_EINVAL, "affine_unwarp_heatmaps: %s and %s overlap", out_name[o], out_name[p]);
  }
  hipStream_t st = as_stream(stream);
  const bool lds = hw * 4 <= 65536;
  const size_t smem = (size_t)WU_SCRATCH * 4 + (lds ? (size_t)hw * 4 : 0);
  static size_t cap = 64 * 1024;                           // per process and unguarded, as flip_decode's
  if (smem > cap) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(affine_unwarp_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
      MI_FAIL(MI355_ELAUNCH, "affine_unwarp_heatmaps: cannot raise the dynamic LDS limit to %zu bytes", smem);
    cap = smem;
  }
  char lab[96];
  snprintf(lab, sizeof(lab), "affine_unwarp rows%ld %dx%d%s%s", rows, h, w, lds ? "" : " global", w_out ? " +w" : "");
  ProfScope ps(st, 0.0, 8.0 * n + (double)sizeof(mi355_view_rec) * B + (w_out ? 12.0 : 4.0) * rows, 2, lab);
  if (lds)
    hipLaunchKernelGGL(affine_unwarp_kernel<true>, dim3((unsigned)rows), dim3(hw * 4 > 32768 ? 1024 : 256), smem, st, y, recs, margin, w_in, out,
                       valid, w_out, K, h, w);
  else
    hipLaunchKernelGGL(affine_unwarp_kernel<false>, dim3((unsigned)rows), dim3(256), smem, st, y, recs, margin, w_in, out, valid, w_out, K, h, w);
  MI_CHECK_LAUNCH("affine_unwarp_heatmaps");
  return MI355_OK;
}

// ---------------------------------------------------------------- masked, weighted MSE over heat-map rows
// mse_heatmap_kernel (teacher.hip) with a per-map weight from device memory: the same lane sums and the same shuffle tree, then
// rows[r] = fl(s * w) and grad = fl(fl(d * gs) * w).  A row with w == 0 or outside the joint mask is written as zeros without
// reading pred / target.
template <bool VEC>
__global__ __launch_bounds__(256) void mse_heatmap_w_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const mi355_mse_rec* __restrict__ rec, const float* __restrict__ wmap,
                                                             float* __restrict__ rows, float* __restrict__ grad, int K, int HW) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const unsigned mask = (unsigned)rec->joint_mask;
  const float gs = rec->grad_scale;
  const float wt = wmap[r];
  const bool on = ((mask >> (r % K)) & 1u) && !(wt == 0.0f);
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
      if (g) {
        const float g0 = d0 * gs, g1 = d1 * gs, g2 = d2 * gs, g3 = d3 * gs;
        *reinterpret_cast<float4*>(g + j) = make_float4(g0 * wt, g1 * wt, g2 * wt, g3 * wt);
      }
    }
  } else {
    for (int j = t; j < HW; j += 256) {
      const float d = p[j] - q[j];
      const float e = d * d;
      s = s + e;
      if (g) { const float u = d * gs; g[j] = u * wt; }
    }
  }
  s = block_sum<4>(s, red);
  if (t == 0) rows[r] = on ? s * wt : 0.f;
}

extern "C" int mi355_mse_heatmap_w(const float* pred, const float* target, const mi355_mse_rec* rec_dev, const float* wmap, float* rows,
                                   float* unit_grad, int B, int K, int HW, void* stream) {
  if (!pred || !target || !rec_dev || !wmap || !rows) MI_FAIL(MI355_EINVAL, "mse_heatmap_w: null pointer");
  if (B < 1 || K < 1 || K > 32) MI_FAIL(MI355_EINVAL, "mse_heatmap_w: B=%d K=%d (1 <= K <= 32)", B, K);
  if (HW < 1) MI_FAIL(MI355_EINVAL, "mse_heatmap_w: HW=%d", HW);
  if ((long)B * K > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "mse_heatmap_w: too many rows");
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)rec_dev | (uintptr_t)wmap | (uintptr_t)rows | (uintptr_t)unit_grad) & 3)
    MI_FAIL(MI355_EINVAL, "mse_heatmap_w: pointers must be 4-byte aligned");
  char lab[64];
  snprintf(lab, sizeof(lab), "mse_heatmap_w rows%d HW%d%s", B * K, HW, unit_grad ? " +grad" : "");
  ProfScope ps(as_stream(stream), 0.0, (unit_grad ? 12.0 : 8.0) * B * K * HW + 4.0 * B * K, 2, lab);
  const bool vec = HW % 4 == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)unit_grad) & 15) == 0;
  if (vec) hipLaunchKernelGGL(mse_heatmap_w_kernel<true>, dim3(B * K), dim3(256), 0, as_stream(stream), pred, target, rec_dev, wmap, rows, unit_grad, K, HW);
  else hipLaunchKernelGGL(mse_heatmap_w_kernel<false>, dim3(B * K), dim3(256), 0, as_stream(stream), pred, target, rec_dev, wmap, rows, unit_grad, K, HW);
  MI_CHECK_LAUNCH("mse_heatmap_w");
  return MI355_OK;
}

// Evaluation at image resolution: the decode of utils/keypoint_detection.py:172-205 (compute_uv_from_heatmaps2: bilinear
// up-sampling of the heat-maps to the image size, then arg-max) as ONE kernel that never writes the up-sampled maps, and the
// accumulation of the end-point error and the thresholded hit counts behind EPE / PCK curve / AUC (:95-136).  Not in the reference:
// the flip test (the batch with its mirror images for one forward; the two sets of heat-maps averaged) and the quarter-pixel and
// second-order (DARK) sub-pixel decodes of Simple Baselines / HRNet / mmpose, average + arg-max + refinement in one launch.
#include "common.h"

// mi355_argmax2d's order (heatmap.hip): NaN counts as maximum, on equal values the lower index wins
__device__ __forceinline__ bool up_better(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && !bn) || (an && bn && ai < bi);
  return av > bv || (av == bv && ai < bi);
}

// One workgroup per map: 256 threads, 1024 for maps above 32 KB (at 64 KB two workgroups fit the LDS of a CU; 2 x 4 waves
// would leave its SIMDs idle).  The h x w input map is staged in LDS once (LDS = true: up to 64 KB, 16-byte loads where
// the addresses allow) or read in place through the caches (LDS = false: larger maps); the H x W outputs exist in registers only.
// The threads form a TY x TX grid, TX = the power of two >= min(W, 256), TY = threads / TX: a thread owns the columns ox = tx, tx + TX, ... and
// walks the rows oy = ty, ty + TY, ... of each, so the column's indices and weights are computed once per column, no
// division per output.  Index and weight rule and the expression order are bilinear_up_kernel's (ATen upsample_bilinear2d,
// align_corners = False); nothing is contracted into an FMA.  Every thread keeps a running (value, index); the fold over lanes
// and waves compares indices on equal values, so the result is the first maximum in row-major order whatever the walk order.
template <bool LDS>
__global__ __launch_bounds__(1024) void upsample_argmax_kernel(const float* __restrict__ hm, int* __restrict__ idx, float* __restrict__ xy,
                                                               float* __restrict__ maxval, int h, int w, int H, int W, int tx_log2, int vec) {
  extern __shared__ __align__(16) float smap[];           // the map, then (after the walk) the results of up to 16 waves: >= 128 bytes
  const int hw = h * w, NT = blockDim.x;
  const float* __restrict__ src = hm + (size_t)blockIdx.x * hw;
  if (LDS) {
    if (vec) {          // (host: hw % 4 == 0 and hm 16-byte aligned, so every map is)
      for (int i = threadIdx.x; i < (hw >> 2); i += NT) reinterpret_cast<float4*>(smap)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
      for (int i = threadIdx.x; i < hw; i += NT) smap[i] = src[i];
    }
    __syncthreads();
  }
  const float* __restrict__ m = LDS ? smap : src;
  const int TX = 1 << tx_log2, TY = NT >> tx_log2;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log2;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  // "nothing yet" is -inf at an index past the grid: every real candidate replaces it (a real -inf by its lower index), and a
  // thread without an output (tx >= W or ty >= H) hands it on to lose every comparison of the fold
  float bv = -INFINITY; int bi = 0x7fffffff;
  for (int ox = tx; ox < W; ox += TX) {
    float fx = sx * ((float)ox + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
    const int x0 = min((int)fx, w - 1);                  // (fx < w in exact arithmetic; the clamp keeps a rounding slip in bounds)
    const int x1 = x0 + ((x0 < w - 1) ? 1 : 0);
    const float lx = fx - (float)x0, hx = 1.f - lx;
    int py0 = -1; float top = 0.f, bot = 0.f;            // the two row terms of the column, kept while y0 stays (up-sampling: H / h outputs)
    for (int oy = ty; oy < H; oy += TY) {
      float fy = sy * ((float)oy + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
      const int y0 = min((int)fy, h - 1);
      const float ly = fy - (float)y0, hy = 1.f - ly;
      if (y0 != py0) {
        const int y1 = y0 + ((y0 < h - 1) ? 1 : 0);
        top = hx * m[y0 * w + x0] + lx * m[y0 * w + x1];
        bot = hx * m[y1 * w + x0] + lx * m[y1 * w + x1];
        py0 = y0;
      }
      const float v = hy * top + ly * bot;
      const int i = oy * W + ox;
      if (up_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (up_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  float* sv = smap; int* si = reinterpret_cast<int*>(smap) + 16;
  __syncthreads();                                     // every thread is done with the map
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < (NT >> 6); ++q) if (up_better(sv[q], si[q], bv, bi)) { bv = sv[q]; bi = si[q]; }
    const bool pos = bv > 0.0f;                        // torch.greater(maxvals, 0.0): NaN -> False
    if (idx) idx[blockIdx.x] = bi;
    if (maxval) maxval[blockIdx.x] = bv;
    if (xy) { xy[2 * blockIdx.x] = pos ? (float)(bi % W) : 0.f; xy[2 * blockIdx.x + 1] = pos ? (float)(bi / W) : 0.f; }
  }
}

extern "C" int mi355_upsample_argmax(const float* hm, int32_t* idx, float* xy, float* maxval, int rows, int h, int w, int H, int W,
                                     void* stream) {
  if (!hm || rows < 1 || h < 1 || w < 1 || H < 1 || W < 1) MI_FAIL(MI355_EINVAL, "upsample_argmax: bad args");
  if ((long)h * w > 0x7fffffffL || (long)H * W >= 0x7fffffffL)
    MI_FAIL(MI355_EINVAL, "upsample_argmax: map of %d x %d -> %d x %d is beyond 32-bit indices", h, w, H, W);
  if (((uintptr_t)hm | (uintptr_t)idx | (uintptr_t)xy | (uintptr_t)maxval) & 3) MI_FAIL(MI355_EINVAL, "upsample_argmax: pointers must be 4-byte aligned");
  // the maps at their own size: every weight is 1 or 0, the virtual map is the input -- mi355_argmax2d's kernels and bits
  if (H == h && W == w) return mi355_argmax2d(hm, idx, xy, maxval, rows, H, W, stream);
  hipStream_t st = as_stream(stream);
  int tx_log2 = 0;
  while (tx_log2 < 8 && (1 << tx_log2) < W) ++tx_log2;
  const long hw = (long)h * w;
  const int vec = (hw % 4 == 0 && ((uintptr_t)hm & 15) == 0) ? 1 : 0;
  char lab[64];
  snprintf(lab, sizeof(lab), "upsample_argmax rows%d %dx%d>%dx%d", rows, h, w, H, W);
  ProfScope ps(st, 10.0 * rows * H * W, 4.0 * rows * hw, 2, lab);
  if (hw * 4 <= 65536)
    hipLaunchKernelGGL(upsample_argmax_kernel<true>, dim3(rows), dim3(hw * 4 > 32768 ? 1024 : 256), (size_t)(hw * 4 < 128 ? 128 : hw * 4), st, hm, idx, xy, maxval, h, w, H, W, tx_log2, vec);
  else
    hipLaunchKernelGGL(upsample_argmax_kernel<false>, dim3(rows), dim3(256), 128, st, hm, idx, xy, maxval, h, w, H, W, tx_log2, 0);
  MI_CHECK_LAUNCH("upsample_argmax");
  return MI355_OK;
}

// Thread (k, t) walks b = 0 .. B-1 in order for joint k and threshold t; the threads with t = 0 also carry the joint's error
// sum and count.  float64 arithmetic from the fp32 inputs as pck_dists_kernel; the sum is sequential in b, so a data set gives
// the same accumulator bits in one batch or in many.  Invisible joints are skipped before their coordinates are touched.
__global__ __launch_bounds__(256) void pose_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ vis,
                                                            const float* __restrict__ thr, int T, int B, int K, double* __restrict__ sum_err,
                                                            int* __restrict__ count, int* __restrict__ hits) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= K * T) return;
  const int k = id / T, t = id % T;
  const double th = (double)thr[t];
  double s = t == 0 ? sum_err[k] : 0.0;
  int c = 0, hit = 0;
  for (int b = 0; b < B; ++b) {
    const int r = b * K + k;
    if (!(vis[r] > 0.f)) continue;
    const double dx = (double)pred[2 * r] - (double)gt[2 * r];
    const double dy = (double)pred[2 * r + 1] - (double)gt[2 * r + 1];
    const double e = sqrt(dx * dx + dy * dy);
    s += e; ++c;
    hit += (e < th) ? 1 : 0;                           // strict, as accuracy_3d's `joint_est_error < joint_threshold`
  }
  hits[id] += hit;
  if (t == 0) { sum_err[k] = s; count[k] += c; }
}

extern "C" int mi355_pose_metrics(const float* pred_xy, const float* gt_xy, const float* vis, const float* thr, int T, int B, int K,
                                  double* sum_err, int32_t* count, int32_t* hits, void* stream) {
  if (!pred_xy || !gt_xy || !vis || !thr || !sum_err || !count || !hits) MI_FAIL(MI355_EINVAL, "pose_metrics: null pointer");
  if (T < 1 || B < 1 || K < 1 || (long)K * T > (1L << 24) || (long)B * K > (1L << 30))
    MI_FAIL(MI355_EINVAL, "pose_metrics: T=%d B=%d K=%d", T, B, K);
  if ((((uintptr_t)pred_xy | (uintptr_t)gt_xy | (uintptr_t)vis | (uintptr_t)thr | (uintptr_t)count | (uintptr_t)hits) & 3) || ((uintptr_t)sum_err & 7))
    MI_FAIL(MI355_EINVAL, "pose_metrics: pointers must be aligned to their element");
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(cdiv((long)K * T, 256)), dim3(256), 0, as_stream(stream), pred_xy, gt_xy, vis, thr, T, B, K,
                     sum_err, count, hits);
  MI_CHECK_LAUNCH("pose_metrics");
  return MI355_OK;
}

// ------------------------------------------------------------------------------------------------ flip test, sub-pixel decode
// The input batch followed by its mirror images along W, for one forward of 2B images: item i of x goes to out[i] and to
// out[n + row * W + (W - 1 - col)].  VEC: four columns per thread, the mirrored quad stored reversed at column W - 4 - col
// (host: W % 4 == 0, both pointers 16-byte aligned, so every quad of either half is); otherwise one element per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void mirror_batch_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int W) {
  const long step = (long)gridDim.x * 256;
  if (VEC) {
    const int W4 = W >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += step) {
      const long row = i / W4; const int c4 = (int)(i - row * W4);
      const float4 q = reinterpret_cast<const float4*>(x)[i];
      reinterpret_cast<float4*>(out)[i] = q;
      reinterpret_cast<float4*>(out + n)[row * W4 + (W4 - 1 - c4)] = make_float4(q.w, q.z, q.y, q.x);
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
      const long row = i / W; const int c = (int)(i - row * W);
      const float v = x[i];
      out[i] = v;
      out[n + row * W + (W - 1 - c)] = v;
    }
  }
}

extern "C" int mi355_mirror_batch(const float* x, float* out, int B, int C, int H, int W, void* stream) {
  if (!x || !out) MI_FAIL(MI355_EINVAL, "mirror_batch: null pointer (x %p, out %p)", (const void*)x, (void*)out);
  if (B < 1 || C < 1 || H < 1 || W < 1) MI_FAIL(MI355_EINVAL, "mirror_batch: B=%d C=%d H=%d W=%d", B, C, H, W);
  if (((uintptr_t)x | (uintptr_t)out) & 3) MI_FAIL(MI355_EINVAL, "mirror_batch: pointers must be 4-byte aligned");
  const long n = (long)B * C * H * W;
  hipStream_t st = as_stream(stream);
  const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  char lab[64];
  snprintf(lab, sizeof(lab), "mirror_batch %dx%dx%dx%d", B, C, H, W);
  ProfScope ps(st, 0.0, 12.0 * n, 2, lab);
  const long items = vec ? n >> 2 : n;
  const int blocks = (int)(cdiv(items, 256) < (1L << 16) ? cdiv(items, 256) : (1L << 16));
  if (vec) hipLaunchKernelGGL(mirror_batch_kernel<true>, dim3(blocks), dim3(256), 0, st, x, out, n, W);
  else hipLaunchKernelGGL(mirror_batch_kernel<false>, dim3(blocks), dim3(256), 0, st, x, out, n, W);
  MI_CHECK_LAUNCH("mirror_batch");
  return MI355_OK;
}

// The thirteen points of the second-order refinement around the arg-max: the centre, (+-1, 0), (+-2, 0), (0, +-1), (0, +-2) and
// the four diagonals, in the order the differences below name them.
constexpr int FD_POINTS = 13, FD_RMAX = 16, FD_ROWS = FD_POINTS * (2 * FD_RMAX + 1);
constexpr int FD_SCRATCH = (32 + FD_ROWS + FD_POINTS + 3) & ~3;     // floats in front of the staged map: keeps the map 16-byte aligned
__device__ const signed char FD_DX[FD_POINTS] = {0, 1, -1, 2, -2, 0, 0, 0, 0, 1, -1, 1, -1};
__device__ const signed char FD_DY[FD_POINTS] = {0, 0, 0, 0, 0, 1, -1, 2, -2, 1, 1, -1, -1};

// The working map m of one row: hm itself, or 0.5f * (hm + hm_flip mirrored back), the sum and the product rounded separately.
// shift = 1 reads the mirrored map one column to the right (Simple Baselines' SHIFT_HEATMAP); column 0 keeps its unshifted value.
struct FlipMap {
  const float* __restrict__ a; const float* __restrict__ f; int w, shift;
  __device__ __forceinline__ int src_col(int x) const { return shift ? (x ? w - x : w - 1) : w - 1 - x; }
  __device__ __forceinline__ float at(int row_off, int x) const {
    const float v = a[row_off + x];
    return f ? 0.5f * (v + f[row_off + src_col(x)]) : v;
  }
};

// One workgroup per map, upsample_argmax_kernel's layout: 256 threads, 1024 for maps above 32 KB.  One pass forms the working
// map (FlipMap), stages it in LDS (LDS = true: up to 64 KB) and writes it to avg_out where asked, and keeps a running
// (value, index) per thread; the fold over lanes and waves is mi355_argmax2d's (first maximum in row-major order, NaN counts as
// maximum).  LDS = false re-forms a value from hm / hm_flip through the caches wherever the refinement needs one: the same two
// operations, the same bits.  mode 1: a quarter pixel towards the higher neighbour.  mode 2: the Taylor ("DARK") step on the
// log of the map smoothed by the separable taps, zero padded -- the 13 x (2 radius + 1) row sums one per thread, then the 13
// column sums, both fp32 in ascending tap order with every product and sum rounded on its own, then float64 in thread 0.  No
// renormalisation to the original maximum: a constant added to every log cancels in all five differences.
template <bool LDS>
__global__ __launch_bounds__(1024) void flip_decode_kernel(const float* __restrict__ hm, const float* __restrict__ hm_flip, int shift,
                                                           float* __restrict__ avg_out, int mode, const float* __restrict__ taps, int radius,
                                                           float scale_x, float scale_y, int* __restrict__ idx, float* __restrict__ xy,
                                                           float* __restrict__ maxval, int h, int w, int vec) {
  extern __shared__ __align__(16) float smem[];            // [0,16) wave values, [16,32) wave indices, row sums, column sums, the map
  float* sv = smem; int* si = reinterpret_cast<int*>(smem) + 16;
  float* rowsum = smem + 32; float* colsum = rowsum + FD_ROWS;
  float* smap = smem + FD_SCRATCH;
  const int hw = h * w, NT = blockDim.x;
  const size_t base = (size_t)blockIdx.x * hw;
  const FlipMap fm{hm + base, hm_flip ? hm_flip + base : nullptr, w, shift};
  float* __restrict__ avg = avg_out ? avg_out + base : nullptr;
  float bv = -INFINITY; int bi = 0x7fffffff;               // "nothing yet": loses against every real candidate (upsample_argmax_kernel)
  if (vec) {            // (host: w % 4 == 0, hm and avg_out 16-byte aligned: a quad stays inside one row of the map)
    for (int q = threadIdx.x; q < (hw >> 2); q += NT) {
      const int i = q << 2, y = i / w, x = i - y * w;
      float4 v = reinterpret_cast<const float4*>(fm.a)[q];
      if (fm.f) {
        const float* __restrict__ fr = fm.f + (i - x);
        v.x = 0.5f * (v.x + fr[fm.src_col(x)]);     v.y = 0.5f * (v.y + fr[fm.src_col(x + 1)]);
        v.z = 0.5f * (v.z + fr[fm.src_col(x + 2)]); v.w = 0.5f * (v.w + fr[fm.src_col(x + 3)]);
      }
      if (LDS) reinterpret_cast<float4*>(smap)[q] = v;
      if (avg) reinterpret_cast<float4*>(avg)[q] = v;
      if (up_better(v.x, i, bv, bi)) { bv = v.x; bi = i; }
      if (up_better(v.y, i + 1, bv, bi)) { bv = v.y; bi = i + 1; }
      if (up_better(v.z, i + 2, bv, bi)) { bv = v.z; bi = i + 2; }
      if (up_better(v.w, i + 3, bv, bi)) { bv = v.w; bi = i + 3; }
    }
  } else {
    for (int i = threadIdx.x; i < hw; i += NT) {
      const int y = i / w, x = i - y * w;
      const float v = fm.at(i - x, x);
      if (LDS) smap[i] = v;
      if (avg) avg[i] = v;
      if (up_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (up_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();                                       // the wave results and the staged map
  bv = sv[0]; bi = si[0];                                // every thread folds the waves: the winner is known block-wide
  for (int q = 1; q < (NT >> 6); ++q) if (up_better(sv[q], si[q], bv, bi)) { bv = sv[q]; bi = si[q]; }
  const bool pos = bv > 0.0f;                            // torch.greater(maxvals, 0.0): NaN -> False
  const int py = bi / w, px = bi - py * w;
  auto m = [&](int y, int x) -> float { return LDS ? smap[y * w + x] : fm.at(y * w, x); };
  double ox = 0.0, oy = 0.0;
  // (pos, mode, px, py are the same in every thread of the block: the barriers below are reached by all or by none)
  if (pos && mode == 1 && threadIdx.x == 0) {
    if (px >= 1 && px <= w - 2) { const float d = m(py, px + 1) - m(py, px - 1); ox = d > 0.f ? 0.25 : (d < 0.f ? -0.25 : 0.0); }
    if (py >= 1 && py <= h - 2) { const float d = m(py + 1, px) - m(py - 1, px); oy = d > 0.f ? 0.25 : (d < 0.f ? -0.25 : 0.0); }
  }
  if (pos && mode == 2 && px >= 2 && px <= w - 3 && py >= 2 && py <= h - 3) {
    const int nt = 2 * radius + 1;
    for (int t = threadIdx.x; t < FD_POINTS * nt; t += NT) {
      const int p = t / nt, yy = py + FD_DY[p] + (t - p * nt) - radius, x0 = px + FD_DX[p] - radius;
      const bool yin = yy >= 0 && yy < h;
      float row = 0.f;
      for (int j = 0; j < nt; ++j) {
        const int xx = x0 + j;
        const float v = (yin && xx >= 0 && xx < w) ? m(yy, xx) : 0.f;
        row = row + taps[j] * v;
      }
      rowsum[t] = row;
    }
    __syncthreads();
    if (threadIdx.x < FD_POINTS) {
      float tot = 0.f;
      for (int j = 0; j < nt; ++j) tot = tot + taps[j] * rowsum[threadIdx.x * nt + j];
      colsum[threadIdx.x] = tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double L[FD_POINTS];
#pragma unroll
      for (int p = 0; p < FD_POINTS; ++p) { const double t = (double)colsum[p]; L[p] = log(t > 1e-10 ? t : 1e-10); }
      const double gx = .5 * (L[1] - L[2]), gy = .5 * (L[5] - L[6]);
      const double dxx = .25 * (L[3] - 2. * L[0] + L[4]), dyy = .25 * (L[7] - 2. * L[0] + L[8]);
      const double dxy = .25 * (L[9] - L[10] - L[11] + L[12]);
      const double det = dxx * dyy - dxy * dxy;
      if (det != 0.0) {
        const double tx = -(dyy * gx - dxy * gy) / det, ty = -(dxx * gy - dxy * gx) / det;
        if (isfinite(tx) && isfinite(ty)) { ox = tx; oy = ty; }
      }
    }
  }
  if (threadIdx.x == 0) {
    if (idx) idx[blockIdx.x] = bi;
    if (maxval) maxval[blockIdx.x] = bv;
    if (xy) {
      xy[2 * blockIdx.x] = pos ? (float)((double)px + ox) * scale_x : 0.f;
      xy[2 * blockIdx.x + 1] = pos ? (float)((double)py + oy) * scale_y : 0.f;
    }
  }
}

extern "C" int mi355_flip_decode(const float* hm, const float* hm_flip, int shift, float* avg_out, int mode, const float* taps, int radius,
                                 float scale_x, float scale_y, int32_t* idx, float* xy, float* maxval, int rows, int h, int w, void* stream) {
  if (!hm) MI_FAIL(MI355_EINVAL, "flip_decode: hm is null");
  if (rows < 1 || h < 1 || w < 1) MI_FAIL(MI355_EINVAL, "flip_decode: rows=%d h=%d w=%d", rows, h, w);
  if ((long)h * w > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "flip_decode: map of h=%d x w=%d is beyond 32-bit indices", h, w);
  if (((uintptr_t)hm | (uintptr_t)hm_flip | (uintptr_t)avg_out | (uintptr_t)taps | (uintptr_t)idx | (uintptr_t)xy | (uintptr_t)maxval) & 3)
    MI_FAIL(MI355_EINVAL, "flip_decode: pointers (hm, hm_flip, avg_out, taps, idx, xy, maxval) must be 4-byte aligned");
  if (mode < 0 || mode > 2) MI_FAIL(MI355_EINVAL, "flip_decode: mode=%d is none of 0 (argmax), 1 (quarter), 2 (taylor)", mode);
  if (mode == 2 && !taps) MI_FAIL(MI355_EINVAL, "flip_decode: mode 2 needs taps");
  if (mode == 2 && (radius < 1 || radius > FD_RMAX)) MI_FAIL(MI355_EINVAL, "flip_decode: radius=%d outside 1..%d", radius, FD_RMAX);
  if (shift != 0 && shift != 1) MI_FAIL(MI355_EINVAL, "flip_decode: shift=%d is neither 0 nor 1", shift);
  hipStream_t st = as_stream(stream);
  const long hw = (long)h * w;
  const int vec = (hw % 4 == 0 && (!hm_flip || w % 4 == 0) && (((uintptr_t)hm | (uintptr_t)avg_out) & 15) == 0) ? 1 : 0;
  const bool lds = hw * 4 <= 65536;
  const size_t smem = (size_t)FD_SCRATCH * 4 + (lds ? (size_t)hw * 4 : 0);
  static size_t cap = 64 * 1024;                           // per process and unguarded, as the attribute flags of augment.hip
  if (smem > cap) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(flip_decode_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
      MI_FAIL(MI355_ELAUNCH, "flip_decode: cannot raise the dynamic LDS limit to %zu bytes", smem);
    cap = smem;
  }
  char lab[64];
  snprintf(lab, sizeof(lab), "flip_decode rows%d %dx%d m%d f%d", rows, h, w, mode, hm_flip ? 1 + shift : 0);
  ProfScope ps(st, (hm_flip ? 4.0 : 2.0) * rows * hw, (hm_flip ? 8.0 : 4.0) * rows * hw + (avg_out ? 4.0 * rows * hw : 0.0), 2, lab);
  if (lds)
    hipLaunchKernelGGL(flip_decode_kernel<true>, dim3(rows), dim3(hw * 4 > 32768 ? 1024 : 256), smem, st, hm, hm_flip, shift, avg_out, mode, taps,
                       radius, scale_x, scale_y, idx, xy, maxval, h, w, vec);
  else
    hipLaunchKernelGGL(flip_decode_kernel<false>, dim3(rows), dim3(256), smem, st, hm, hm_flip, shift, avg_out, mode, taps, radius, scale_x,
                       scale_y, idx, xy, maxval, h, w, vec);
  MI_CHECK_LAUNCH("flip_decode");
  return MI355_OK;
}

// Evaluation at image resolution: the decode of utils/keypoint_detection.py:172-205 (compute_uv_from_heatmaps2: bilinear
// up-sampling of the heat-maps to the image size, then arg-max) as ONE kernel that never writes the up-sampled maps, and the
// accumulation of the end-point error and the thresholded hit counts behind EPE / PCK curve / AUC (:95-136).
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

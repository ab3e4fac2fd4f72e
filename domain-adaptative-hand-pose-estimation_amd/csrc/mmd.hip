// Multi-kernel MMD between a batch of source and a batch of target heat-maps, per joint (uda/model/loss.py:1061-1104 MMD_loss3,
// :1107-1196 MMD_loss / mmd_rbf): three launches -- pairwise squared distances in the difference form, the bandwidths with the
// Gaussian kernels' coefficients and the per-joint loss, and the gradient as an (n x n) by (n x HW) product per joint -- without
// the reference's n x n x HW temporaries.  Rows are read where they are, through two pointers: row i < B is source[i][k], row
// i >= B is target[i - B][k].  No atomics; every sum runs in a fixed order, so two runs give the same bits.
#include <math.h>
#include "common.h"

#define MMD_DT 32                     // mmd_dist: a block owns a DT x DT tile of row pairs (upper triangle of tiles) of one joint
#define MMD_DCH 64                    // ... and walks HW in chunks of DCH floats staged in LDS
#define MMD_DLD (MMD_DCH + 4)         // LDS row stride: 16-byte reads of 16 different rows hit 16 different 16-byte slots
#define MMD_GR 16                     // mmd_grad: a block owns GR rows ...
#define MMD_GC 1024                   // ... by GC columns (4 per thread) of one joint

struct mmd_params {
  float div;                          // kernel_mul ^ (kernel_num / 2)
  float mulpow[MI355_MMD_MAX_KERNELS];   // kernel_mul ^ m
  float bwfix[MI355_MMD_MAX_KERNELS];    // the bandwidths when fix_sigma is given (formed in double on the host)
  float coef;                         // scale / (B^2 K)
  int num, fixed;
};

__device__ __forceinline__ const float* mmd_row(const float* __restrict__ src, const float* __restrict__ tgt, int i, int k, int B,
                                                int K, int HW) {
  return i < B ? src + ((long)i * K + k) * HW : tgt + ((long)(i - B) * K + k) * HW;
}

// ---------------------------------------------------------------- distances
// D[k][i][j] = sum_p (x_i[p] - x_j[p])^2.  Thread (ty, tx) of the 16 x 16 block owns the pairs (ty | ty + 16) x (tx | tx + 16) of
// the tile.  Per chunk every pair sums its 64 squares into four interleaved partial sums (p mod 4), these are added pairwise and the
// chunk's sum goes into a compensated running total: the error stays near one rounding at HW = 4096, where a plain running sum
// would drift by sqrt(HW) of them.  The two staging paths (float4 / scalar loads) fill the same LDS image: the same bits.
// A pair is computed once (i < j; in a diagonal tile the lower half idles) and written to D[i][j] and D[j][i]; D[i][i] = 0.
template <bool VEC>
__global__ __launch_bounds__(256) void mmd_dist_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                        float* __restrict__ D, int B, int K, int HW, int ntile) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sa[2][MMD_DT][MMD_DLD];
  const int t = threadIdx.x, k = blockIdx.y, n = 2 * B;
  int ti = 0, r = blockIdx.x;
  while (r >= ntile - ti) { r -= ntile - ti; ++ti; }
  const int tj = ti + r;
  const int ty = t >> 4, tx = t & 15;
  float tot[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, comp[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int p0 = 0; p0 < HW; p0 += MMD_DCH) {
    if (VEC) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int q = t + 256 * s, half = q >> 9, row = (q & 511) >> 4, c4 = q & 15;
        const int g = (half ? tj : ti) * MMD_DT + row, p = p0 + 4 * c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < n && p < HW) v = *reinterpret_cast<const float4*>(mmd_row(src, tgt, g, k, B, K, HW) + p);
        *reinterpret_cast<float4*>(&sa[half][row][4 * c4]) = v;
      }
    } else {
#pragma unroll 4
      for (int s = 0; s < 16; ++s) {
        const int q = t + 256 * s, half = q >> 11, row = (q & 2047) >> 6, c = q & 63;
        const int g = (half ? tj : ti) * MMD_DT + row, p = p0 + c;
        sa[half][row][c] = (g < n && p < HW) ? mmd_row(src, tgt, g, k, B, K, HW)[p] : 0.f;
      }
    }
    __syncthreads();
    float4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int c4 = 0; c4 < MMD_DCH / 4; ++c4) {
      float4 xa[2], xb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        xa[a] = *reinterpret_cast<const float4*>(&sa[0][ty + 16 * a][4 * c4]);
        xb[a] = *reinterpret_cast<const float4*>(&sa[1][tx + 16 * a][4 * c4]);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float d0 = xa[a].x - xb[b].x, d1 = xa[a].y - xb[b].y, d2 = xa[a].z - xb[b].z, d3 = xa[a].w - xb[b].w;
          acc[a][b].x = fmaf(d0, d0, acc[a][b].x); acc[a][b].y = fmaf(d1, d1, acc[a][b].y);
          acc[a][b].z = fmaf(d2, d2, acc[a][b].z); acc[a][b].w = fmaf(d3, d3, acc[a][b].w);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float chunk = (acc[a][b].x + acc[a][b].y) + (acc[a][b].z + acc[a][b].w);
        const float y = chunk - comp[a][b];
        const float s = tot[a][b] + y;
        comp[a][b] = (s - tot[a][b]) - y;
        tot[a][b] = s;
      }
    __syncthreads();
  }
  float* __restrict__ Dk = D + (long)k * n * n;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gi = ti * MMD_DT + ty + 16 * a, gj = tj * MMD_DT + tx + 16 * b;
      if (gi >= n || gj >= n) continue;
      if (gi < gj) { Dk[gi * n + gj] = tot[a][b]; Dk[gj * n + gi] = tot[a][b]; }
      else if (gi == gj) Dk[gi * n + gi] = 0.f;
    }
}

// ---------------------------------------------------------------- bandwidths, coefficients, loss
// Kmat = sum_m exp(-d / bw_m) and sum_m (-1 / bw_m) exp(-d / bw_m) of one distance
__device__ __forceinline__ void mmd_pair(float d, const float* bw, const float* nib, int num, float& kv, float& cv) {
#pragma clang fp contract(off)
  kv = 0.f; cv = 0.f;
#pragma unroll
  for (int m = 0; m < MI355_MMD_MAX_KERNELS; ++m)          // (unrolled with a predicate: bw[] and nib[] stay in registers)
    if (m < num) {
      const float e = expf(-d / bw[m]);
      kv = kv + e;
      cv = cv + nib[m] * e;
    }
}

// One block per joint.  The sum of D: every thread a compensated sum of its strided elements, then the fixed shuffle tree.  Thread q
// then owns the four entries (a, b), (B + a, B + b), (a, B + b), (B + a, b) of quad q = a * B + b: it replaces each distance by its
// coefficient c in place and adds ((XX + YY) - XY) - YX, the reference's element, to its partial loss -- exactly 0 for a quad whose
// four distances are the same bits.  A joint whose distances are all zero has no bandwidth (the reference divides 0 by 0): its
// coefficients and its loss are written as zeros.
__global__ __launch_bounds__(256) void mmd_coef_kernel(float* __restrict__ D, float* __restrict__ loss_rows, mmd_params P, int B) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int t = threadIdx.x, k = blockIdx.x, n = 2 * B, nn = n * n;
  float* __restrict__ Dk = D + (long)k * nn;
  float bw[MI355_MMD_MAX_KERNELS], nib[MI355_MMD_MAX_KERNELS];
  bool live = true;
  if (P.fixed) {
#pragma unroll
    for (int m = 0; m < MI355_MMD_MAX_KERNELS; ++m) bw[m] = P.bwfix[m];
  } else {
    float s = 0.f, c = 0.f;
    for (int e = t; e < nn; e += 256) {
      const float y = Dk[e] - c;
      const float u = s + y;
      c = (u - s) - y;
      s = u;
    }
    const float S = block_sum<4>(s, red);
    live = S != 0.f;
    const float b0 = (S / (float)(nn - n)) / P.div;
#pragma unroll
    for (int m = 0; m < MI355_MMD_MAX_KERNELS; ++m) bw[m] = b0 * P.mulpow[m];
  }
#pragma unroll
  for (int m = 0; m < MI355_MMD_MAX_KERNELS; ++m) nib[m] = -1.f / bw[m];
  float part = 0.f;
  for (int q = t; q < B * B; q += 256) {
    const int a = q / B, b = q - a * B;
    const int ss = a * n + b, tt = (B + a) * n + B + b, st = a * n + B + b, ts = (B + a) * n + b;
    if (!live) { Dk[ss] = 0.f; Dk[tt] = 0.f; Dk[st] = 0.f; Dk[ts] = 0.f; continue; }
    float kss, ktt, kst, kts, css, ctt, cst, cts;
    mmd_pair(Dk[ss], bw, nib, P.num, kss, css);
    mmd_pair(Dk[tt], bw, nib, P.num, ktt, ctt);
    mmd_pair(Dk[st], bw, nib, P.num, kst, cst);
    mmd_pair(Dk[ts], bw, nib, P.num, kts, cts);
    part = part + (((kss + ktt) - kst) - kts);
    Dk[ss] = P.coef * css; Dk[tt] = P.coef * ctt; Dk[st] = -(P.coef * cst); Dk[ts] = -(P.coef * cts);
  }
  const float total = block_sum<4>(part, red);
  if (t == 0) loss_rows[k] = live ? total / (float)(B * B) : 0.f;
}

// ---------------------------------------------------------------- gradient
// g_i[p] = 4 sum_j c_ij (x_i[p] - x_j[p]) for rows row_lo <= i < row_lo + nrows: x_i sum_j c_ij - sum_j c_ij x_j with the difference
// taken first, as in the distances -- rows that are close to one another do not cancel.  The block's GR x n coefficients sit in LDS
// (j-major: one j is four 16-byte broadcast reads); a thread keeps its 4 columns of the GR rows and of their sums in registers and
// streams the n rows x_j past them, j ascending: a fixed order.
template <bool VEC>
__global__ __launch_bounds__(256) void mmd_grad_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                        const float* __restrict__ C, float* __restrict__ gsrc, float* __restrict__ gtgt,
                                                        int B, int K, int HW, int row_lo, int nrows) {
  __shared__ __attribute__((aligned(16))) float cs[MI355_MMD_MAX_ROWS][MMD_GR];
  const int t = threadIdx.x, k = blockIdx.z, n = 2 * B;
  const int i0 = row_lo + blockIdx.y * MMD_GR, iend = row_lo + nrows;
  const float* __restrict__ Ck = C + (long)k * n * n;
  for (int e = t; e < MMD_GR * n; e += 256) {
    const int r = e / n, j = e - r * n;
    cs[j][r] = i0 + r < iend ? Ck[(i0 + r) * n + j] : 0.f;
  }
  __syncthreads();
  int p[4];
  bool in[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    p[v] = blockIdx.x * MMD_GC + (VEC ? 4 * t + v : t + 256 * v);
    in[v] = p[v] < HW;
  }
  auto load = [&](const float* row, float (&x)[4]) {
    if (VEC) {
      const float4 q = in[0] ? *reinterpret_cast<const float4*>(row + p[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) x[v] = in[v] ? row[p[v]] : 0.f;
    }
  };
  float xi[MMD_GR][4], acc[MMD_GR][4];
#pragma unroll
  for (int r = 0; r < MMD_GR; ++r) {
    if (i0 + r < iend) load(mmd_row(src, tgt, i0 + r, k, B, K, HW), xi[r]);
    else { xi[r][0] = 0.f; xi[r][1] = 0.f; xi[r][2] = 0.f; xi[r][3] = 0.f; }
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[r][v] = 0.f;
  }
  for (int j = 0; j < n; ++j) {
    float xj[4], c[MMD_GR];
    load(mmd_row(src, tgt, j, k, B, K, HW), xj);
#pragma unroll
    for (int r4 = 0; r4 < MMD_GR / 4; ++r4) {
      const float4 q = *reinterpret_cast<const float4*>(&cs[j][4 * r4]);
      c[4 * r4] = q.x; c[4 * r4 + 1] = q.y; c[4 * r4 + 2] = q.z; c[4 * r4 + 3] = q.w;
    }
#pragma unroll
    for (int r = 0; r < MMD_GR; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[r][v] = fmaf(c[r], xi[r][v] - xj[v], acc[r][v]);
  }
#pragma unroll
  for (int r = 0; r < MMD_GR; ++r) {
    const int i = i0 + r;
    if (i >= iend) continue;
    float* __restrict__ g = i < B ? gsrc + ((long)i * K + k) * HW : gtgt + ((long)(i - B) * K + k) * HW;
    if (VEC) {
      if (in[0]) *reinterpret_cast<float4*>(g + p[0]) = make_float4(4.f * acc[r][0], 4.f * acc[r][1], 4.f * acc[r][2], 4.f * acc[r][3]);
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) if (in[v]) g[p[v]] = 4.f * acc[r][v];
    }
  }
}

// ---------------------------------------------------------------- host
extern "C" size_t mi355_mmd_workspace(int B, int K) {
  if (B < 1 || K < 1 || 2L * B > MI355_MMD_MAX_ROWS) return 0;
  return (size_t)K * (2 * B) * (2 * B) * sizeof(float);
}

extern "C" int mi355_mmd_heatmap(const float* source, const float* target, float* work, size_t work_bytes, float* loss_rows,
                                 float* grad_source, float* grad_target, int B, int K, int HW, float kernel_mul, int kernel_num,
                                 float fix_sigma, float scale, void* stream) {
  if (!source || !target || !work || !loss_rows) MI_FAIL(MI355_EINVAL, "mmd_heatmap: null pointer");
  if (B < 1 || K < 1 || HW < 1) MI_FAIL(MI355_EINVAL, "mmd_heatmap: B=%d K=%d HW=%d", B, K, HW);
  if (2L * B > MI355_MMD_MAX_ROWS) MI_FAIL(MI355_EINVAL, "mmd_heatmap: n = 2 B = %ld rows, at most %d", 2L * B, MI355_MMD_MAX_ROWS);
  if (K > 65535) MI_FAIL(MI355_EINVAL, "mmd_heatmap: K=%d (at most 65535)", K);
  if (kernel_num < 1 || kernel_num > MI355_MMD_MAX_KERNELS)
    MI_FAIL(MI355_EINVAL, "mmd_heatmap: kernel_num=%d (1 <= kernel_num <= %d)", kernel_num, MI355_MMD_MAX_KERNELS);
  if (!(kernel_mul > 0.f) || !isfinite(kernel_mul)) MI_FAIL(MI355_EINVAL, "mmd_heatmap: kernel_mul=%g must be positive", (double)kernel_mul);
  if (!isfinite(scale) || !isfinite(fix_sigma)) MI_FAIL(MI355_EINVAL, "mmd_heatmap: scale=%g fix_sigma=%g must be finite", (double)scale, (double)fix_sigma);
  if (((uintptr_t)source | (uintptr_t)target | (uintptr_t)work | (uintptr_t)loss_rows | (uintptr_t)grad_source | (uintptr_t)grad_target) & 3)
    MI_FAIL(MI355_EINVAL, "mmd_heatmap: pointers must be 4-byte aligned");
  if (HW > (1 << 30)) MI_FAIL(MI355_EINVAL, "mmd_heatmap: HW=%d (at most 2^30)", HW);
  const size_t need = mi355_mmd_workspace(B, K);
  if (work_bytes < need) MI_FAIL(MI355_EINVAL, "mmd_heatmap: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int n = 2 * B;
  mmd_params P;
  memset(&P, 0, sizeof(P));
  const double div = pow((double)kernel_mul, kernel_num / 2);
  P.div = (float)div;
  for (int m = 0; m < MI355_MMD_MAX_KERNELS; ++m) {
    const int mm = m < kernel_num ? m : kernel_num - 1;          // (slots past kernel_num are never read: keep them finite)
    P.mulpow[m] = (float)pow((double)kernel_mul, mm);
    P.bwfix[m] = fix_sigma > 0.f ? (float)((double)fix_sigma / div * pow((double)kernel_mul, mm)) : 1.f;
  }
  P.coef = (float)((double)scale / ((double)B * B * K));
  P.num = kernel_num;
  P.fixed = fix_sigma > 0.f;
  hipStream_t s = as_stream(stream);
  char lab[96];
  {
    const int ntile = cdiv(n, MMD_DT);
    const bool vec = HW % 4 == 0 && (((uintptr_t)source | (uintptr_t)target) & 15) == 0;
    snprintf(lab, sizeof(lab), "mmd_dist n%d K%d HW%d%s", n, K, HW, vec ? "" : " scalar");
    ProfScope ps(s, 1.5 * n * n * (double)K * HW, 4.0 * n * (double)K * HW + 4.0 * n * n * K, 2, lab);
    const dim3 grid(ntile * (ntile + 1) / 2, K);
    if (vec) hipLaunchKernelGGL(mmd_dist_kernel<true>, grid, dim3(256), 0, s, source, target, work, B, K, HW, ntile);
    else hipLaunchKernelGGL(mmd_dist_kernel<false>, grid, dim3(256), 0, s, source, target, work, B, K, HW, ntile);
    MI_CHECK_LAUNCH("mmd_dist");
  }
  {
    snprintf(lab, sizeof(lab), "mmd_coef n%d K%d kernels%d%s", n, K, kernel_num, P.fixed ? " fixed" : "");
    ProfScope ps(s, 0.0, 8.0 * n * n * K, 2, lab);
    hipLaunchKernelGGL(mmd_coef_kernel, dim3(K), dim3(256), 0, s, work, loss_rows, P, B);
    MI_CHECK_LAUNCH("mmd_coef");
  }
  if (grad_source || grad_target) {
    const int row_lo = grad_source ? 0 : B, nrows = (grad_source && grad_target) ? n : B;
    const bool vec = HW % 4 == 0 && (((uintptr_t)source | (uintptr_t)target | (uintptr_t)grad_source | (uintptr_t)grad_target) & 15) == 0;
    snprintf(lab, sizeof(lab), "mmd_grad n%d K%d HW%d rows%d+%d%s", n, K, HW, row_lo, nrows, vec ? "" : " scalar");
    ProfScope ps(s, 3.0 * nrows * n * (double)K * HW, 4.0 * (n + nrows) * (double)K * HW, 2, lab);
    const dim3 grid(cdiv(HW, MMD_GC), cdiv(nrows, MMD_GR), K);
    if (vec) hipLaunchKernelGGL(mmd_grad_kernel<true>, grid, dim3(256), 0, s, source, target, work, grad_source, grad_target, B, K, HW, row_lo, nrows);
    else hipLaunchKernelGGL(mmd_grad_kernel<false>, grid, dim3(256), 0, s, source, target, work, grad_source, grad_target, B, K, HW, row_lo, nrows);
    MI_CHECK_LAUNCH("mmd_grad");
  }
  return MI355_OK;
}

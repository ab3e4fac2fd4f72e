// Adaptive key-point occlusion of the student's target input and the teacher's per-map confidence (see mi355pose.h; Kim et al.,
// ECCV 2022 -- not in the reference: PAPERS.md).  Three launches: the peak of softmax(beta * y) per teacher map beside its arg-max
// (a row kernel in the forms of heatmap.hip), the gate and the boxes per sample (one thread per sample, integer arithmetic), and
// the copy of the target batch with the boxes blanked (a pure stream).
#include "common.h"
#include "heatmap_rows.h"

// ---------------------------------------------------------------------------------------- peak_prob
// The sum of the softmax's denominator is taken in fp64 on the fp32 operands -- exp((double)v * beta - (double)max * beta), summed in
// a fixed order, one rounding to fp32 at the store -- as the bone kernels do their arithmetic: p is then the float64 value rounded
// once, whatever the map holds (an fp32 sum of fp32 expf is a few ulp off and, at a large beta, the rounding of v * beta alone costs
// more).  16 fp64 exponentials per thread at 64 x 64: far below the launch's memory time.
// what thread 0 of a map stores: arg-max by mi355_argmax2d's rules and p = 1 / s
__device__ __forceinline__ void peak_store(int m, float bv, int bi, double s, int W, int* __restrict__ idx, float* __restrict__ xy,
                                           float* __restrict__ p) {
  const bool pos = bv > 0.0f;                                // np.greater(maxvals, 0.0): NaN -> False
  idx[m] = bi;
  xy[2 * m] = pos ? (float)(bi % W) : 0.f; xy[2 * m + 1] = pos ? (float)(bi / W) : 0.f;
  p[m] = (float)(1.0 / s);
}
__device__ __forceinline__ bool peak_bad(float v) { return !(fabsf(v) < INFINITY); }      // NaN or +-inf
__device__ __forceinline__ double peak_term(float v, double beta, double mx) { return exp((double)v * beta - mx); }
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// block of four waves; the result is valid in thread 0 (the only reader).  `red` = shared double[4].
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Loop form (any size, any alignment): the arg-max walk, then the sum; the second walk is served by the caches.
__global__ __launch_bounds__(256) void peak_prob_kernel(const float* __restrict__ hm, float beta, int* __restrict__ idx, float* __restrict__ xy,
                                                         float* __restrict__ p, unsigned HW, int W) {
  __shared__ float sv[4]; __shared__ int si[4];
  __shared__ double red[4];
  const float* row = hm + (size_t)blockIdx.x * HW;
  float bv = row[0]; int bi = 0;
  if (threadIdx.x < HW) { bv = row[threadIdx.x]; bi = threadIdx.x; }
  for (unsigned i = threadIdx.x + 256; i < HW; i += 256) { const float v = row[i]; if (arg_better(v, (int)i, bv, bi)) { bv = v; bi = (int)i; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = sv[0]; bi = si[0];                                    // (every thread: the maximum feeds the sum)
  for (int w = 1; w < 4; ++w) if (arg_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
  const double b64 = (double)beta, mx = (double)bv * b64;   // beta > 0: the maximum of v * beta
  double s = 0.0; bool bad = false;
  for (unsigned i = threadIdx.x; i < HW; i += 256) { const float v = row[i]; bad |= peak_bad(v); s += peak_term(v, b64, mx); }
  s = block_sum_f64(bad ? (double)NAN : s, red);
  if (threadIdx.x == 0) peak_store(blockIdx.x, bv, bi, s, W, idx, xy, p);
}

template <int NV, bool WPM>
__global__ __launch_bounds__(256) void peak_prob_reg_kernel(const float* __restrict__ hm, float beta, int* __restrict__ idx, float* __restrict__ xy,
                                                             float* __restrict__ p, int rows, int W) {
  using G = RowGeom<NV, WPM>;
  constexpr int HW = 4 * NV * G::kThreads;
  __shared__ float sv[4]; __shared__ int si[4];
  __shared__ double red[4];
  const int m = G::map();
  if (WPM && m >= rows) return;                              // (wave-uniform: a whole wave owns a map)
  float v[4 * NV];
  row_load<NV, WPM>(hm + (size_t)m * HW, v);
  float bv = v[0]; int bi = row_index<NV, WPM>(0, 0);
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = row_index<NV, WPM>(j, e);
      bad |= peak_bad(v[4 * j + e]);
      if (arg_better(v[4 * j + e], i, bv, bi)) { bv = v[4 * j + e]; bi = i; }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if constexpr (!WPM) {
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bv = sv[0]; bi = si[0];
    for (int w = 1; w < 4; ++w) if (arg_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
  }
  const double b64 = (double)beta, mx = (double)bv * b64;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4 * NV; ++k) s += peak_term(v[k], b64, mx);
  if (bad) s = (double)NAN;
  if constexpr (WPM) s = wave_sum_f64(s); else s = block_sum_f64(s, red);
  if (G::tid() == 0) peak_store(m, bv, bi, s, W, idx, xy, p);
}

// ---------------------------------------------------------------------------------------- teacher_select
// One workgroup; thread b (strided) owns sample b.  Behind the comparison with tau and the two float products of a draw
// everything is integer arithmetic.  The candidates of a sample are the set bits of one 64-bit word (K <= 64), in ascending joint
// order: the j-th of them is found by clearing j low bits, and taking it out clears its bit -- no list in memory.  The two sums
// of the statistics are integer sums, so their order does not matter.
__global__ __launch_bounds__(256) void teacher_select_kernel(const float* __restrict__ p, const float* __restrict__ xy, const float* __restrict__ gate_in,
                                                              const float* __restrict__ w_in, const float* __restrict__ u, float tau, float prob,
                                                              int N, int lo, int hi, int S, int H, int W, float* __restrict__ conf,
                                                              float* __restrict__ w_out, int* __restrict__ boxes, int* __restrict__ count,
                                                              float* __restrict__ stats, int B, int K) {
  __shared__ int sred[8];
  int n_pass = 0, n_box = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    unsigned long long cand = 0ull;
    for (int k = 0; k < K; ++k) {
      const size_t r = (size_t)b * K + k;
      const bool pass = p[r] >= tau && (!gate_in || gate_in[r] > 0.f);
      conf[r] = pass ? 1.0f : 0.0f;
      bool cand_ok = pass;
      if (w_in) { const float w = w_in[r]; w_out[r] = w * (pass ? 1.0f : 0.0f); cand_ok = pass && w > 0.f; }
      if (cand_ok) cand |= 1ull << k;
      n_pass += pass ? 1 : 0;
    }
    if (N < 1) continue;
    int* bx = boxes + (size_t)b * N * 4;
    const float* ub = u + (size_t)b * (1 + 2 * N);
    int c = 0;
    const int m = __popcll(cand);
    if (!(ub[0] >= prob)) {
      const int take = m < N ? m : N;
      const int sx = S / W, sy = S / H;
      for (; c < take; ++c) {
        const int mm = m - c;                                // candidates left
        float t = ub[1 + 2 * c] * (float)mm;
        t = fminf(fmaxf(t, 0.f), (float)(mm - 1));           // (a draw outside [0, 1) stays inside the list; NaN -> 0)
        const int j = (int)t;
        unsigned long long rest = cand;
        for (int q = 0; q < j; ++q) rest &= rest - 1;          // (j < mm set bits: never empties the word)
        const int k = __builtin_ctzll(rest);
        cand &= ~(1ull << k);
        float ts = ub[2 + 2 * c] * (float)(hi - lo + 1);
        ts = fminf(fmaxf(ts, 0.f), (float)(hi - lo));
        const int side = lo + (int)ts;
        const size_t r = (size_t)b * K + k;
        const float fx = fminf(fmaxf(xy[2 * r], 0.f), (float)(W - 1)), fy = fminf(fmaxf(xy[2 * r + 1], 0.f), (float)(H - 1));
        const int cx = (int)fx * sx + sx / 2, cy = (int)fy * sy + sy / 2;
        int x0 = cx - side / 2, y0 = cy - side / 2;
        int x1 = x0 + side, y1 = y0 + side;
        x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > S ? S : x1; y1 = y1 > S ? S : y1;
        bx[4 * c] = x0; bx[4 * c + 1] = y0; bx[4 * c + 2] = x1; bx[4 * c + 3] = y1;
      }
    }
    for (int q = c; q < N; ++q) { bx[4 * q] = 0; bx[4 * q + 1] = 0; bx[4 * q + 2] = 0; bx[4 * q + 3] = 0; }
    count[b] = c;
    n_box += c;
  }
  if (!stats) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { n_pass += __shfl_xor(n_pass, o, 64); n_box += __shfl_xor(n_box, o, 64); }
  if ((threadIdx.x & 63) == 0) { sred[threadIdx.x >> 6] = n_pass; sred[4 + (threadIdx.x >> 6)] = n_box; }
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[0] = (float)(sred[4] + sred[5] + sred[6] + sred[7]) / (float)B;                   // mean boxes per sample
    stats[1] = (float)(sred[0] + sred[1] + sred[2] + sred[3]) / ((float)B * (float)K);      // share of confident maps
  }
}

// ---------------------------------------------------------------------------------------- occlude_images
// blockIdx.y = sample; its box records go through LDS once per block and sit in registers for the block's share of the sample.
// VEC: one 16-byte vector per thread and step, four columns of one row (host: W % 4 == 0, both bases 16-byte aligned); otherwise
// one word.  Words move as integers: every bit pattern survives.  A blanked word is +0.0.
template <bool VEC>
__global__ __launch_bounds__(256) void occlude_images_kernel(const unsigned* __restrict__ x, const int* __restrict__ boxes, int N,
                                                              unsigned* __restrict__ out, unsigned plane, unsigned HW, unsigned W) {
  __shared__ int sb[4 * MI355_OCC_MAX_BOXES];
  const unsigned b = blockIdx.y;
  if ((int)threadIdx.x < 4 * N) sb[threadIdx.x] = boxes[(size_t)b * 4 * N + threadIdx.x];
  __syncthreads();
  int bx0[MI355_OCC_MAX_BOXES], by0[MI355_OCC_MAX_BOXES], bx1[MI355_OCC_MAX_BOXES], by1[MI355_OCC_MAX_BOXES];
#pragma unroll
  for (int i = 0; i < MI355_OCC_MAX_BOXES; ++i) {
    const bool on = i < N;                                   // an unused slot is the empty box
    bx0[i] = on ? sb[4 * i] : 0; by0[i] = on ? sb[4 * i + 1] : 0; bx1[i] = on ? sb[4 * i + 2] : 0; by1[i] = on ? sb[4 * i + 3] : 0;
  }
  const size_t base = (size_t)b * plane;
  const unsigned step = gridDim.x * 256;
  if (VEC) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(x + base);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(out + base);
    for (unsigned v = blockIdx.x * 256 + threadIdx.x; v < (plane >> 2); v += step) {
      uint4 q = src[v];
      const unsigned pix = (v << 2) % HW;
      const int y = (int)(pix / W), c = (int)(pix % W);
      bool h0 = false, h1 = false, h2 = false, h3 = false;
#pragma unroll
      for (int i = 0; i < MI355_OCC_MAX_BOXES; ++i) {
        const bool row = y >= by0[i] && y < by1[i];
        h0 |= row && c >= bx0[i] && c < bx1[i];
        h1 |= row && c + 1 >= bx0[i] && c + 1 < bx1[i];
        h2 |= row && c + 2 >= bx0[i] && c + 2 < bx1[i];
        h3 |= row && c + 3 >= bx0[i] && c + 3 < bx1[i];
      }
      q.x = h0 ? 0u : q.x; q.y = h1 ? 0u : q.y; q.z = h2 ? 0u : q.z; q.w = h3 ? 0u : q.w;
      dst[v] = q;
    }
  } else {
    for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < plane; e += step) {
      const unsigned pix = e % HW;
      const int y = (int)(pix / W), c = (int)(pix % W);
      bool h = false;
#pragma unroll
      for (int i = 0; i < MI355_OCC_MAX_BOXES; ++i) h |= y >= by0[i] && y < by1[i] && c >= bx0[i] && c < bx1[i];
      out[base + e] = h ? 0u : x[base + e];
    }
  }
}

// ---------------------------------------------------------------------------------------- host
static bool occ_overlap(const void* p, long np, const void* q, long nq) {      // [p, p + np) and [q, q + nq), in bytes
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

extern "C" int mi355_peak_prob(const float* hm, float beta, int32_t* idx, float* xy, float* p, int rows, int H, int W, void* stream) {
  if (!hm) MI_FAIL(MI355_EINVAL, "peak_prob: null hm");
  if (!idx) MI_FAIL(MI355_EINVAL, "peak_prob: null idx");
  if (!xy) MI_FAIL(MI355_EINVAL, "peak_prob: null xy");
  if (!p) MI_FAIL(MI355_EINVAL, "peak_prob: null p");
  if (rows < 1 || H < 1 || W < 1) MI_FAIL(MI355_EINVAL, "peak_prob: bad shape (rows=%d H=%d W=%d)", rows, H, W);
  if ((long)H * (long)W >= (1L << 31)) MI_FAIL(MI355_EINVAL, "peak_prob: map too large (H=%d W=%d: H*W must be below 2^31)", H, W);
  if (((uintptr_t)hm | (uintptr_t)idx | (uintptr_t)xy | (uintptr_t)p) & 3) MI_FAIL(MI355_EINVAL, "peak_prob: hm, idx, xy and p must be 4-byte aligned");
  if (!__builtin_isfinite(beta) || !(beta > 0.f)) MI_FAIL(MI355_EINVAL, "peak_prob: beta must be finite and positive, got %g", (double)beta);
  hipStream_t st = as_stream(stream);
  const int HW = H * W;
  const int form = row_form(HW, hm);
  char lab[80];
  if (prof_on()) snprintf(lab, sizeof(lab), "peak_prob rows%d %dx%d form%d", rows, H, W, form);
  ProfScope ps(st, 0.0, 4.0 * rows * HW + 16.0 * rows, 2, prof_on() ? lab : nullptr);
  switch (form) {
    case 1: hipLaunchKernelGGL((peak_prob_reg_kernel<4, false>), dim3(rows), dim3(256), 0, st, hm, beta, idx, xy, p, rows, W); break;
    case 2: hipLaunchKernelGGL((peak_prob_reg_kernel<4, true>), dim3(cdiv(rows, 4)), dim3(256), 0, st, hm, beta, idx, xy, p, rows, W); break;
    case 3: hipLaunchKernelGGL((peak_prob_reg_kernel<1, true>), dim3(cdiv(rows, 4)), dim3(256), 0, st, hm, beta, idx, xy, p, rows, W); break;
    default: hipLaunchKernelGGL(peak_prob_kernel, dim3(rows), dim3(256), 0, st, hm, beta, idx, xy, p, (unsigned)HW, W);
  }
  MI_CHECK_LAUNCH("peak_prob");
  return MI355_OK;
}

extern "C" int mi355_teacher_select(const float* p, const float* xy, const float* gate_in, const float* w_in, const float* u, float tau,
                                    float prob, int N, int lo, int hi, int S, int H, int W, float* conf, float* w_out, int32_t* boxes,
                                    int32_t* count, float* stats, int B, int K, void* stream) {
  if (!p) MI_FAIL(MI355_EINVAL, "teacher_select: null p");
  if (!conf) MI_FAIL(MI355_EINVAL, "teacher_select: null conf");
  if ((w_in == nullptr) != (w_out == nullptr)) MI_FAIL(MI355_EINVAL, "teacher_select: w_in and w_out go together (both or neither)");
  if (B < 1 || B > MI355_OCC_MAX_BATCH) MI_FAIL(MI355_EINVAL, "teacher_select: bad batch (B=%d, 1..%d)", B, MI355_OCC_MAX_BATCH);
  if (K < 1 || K > MI355_OCC_MAX_JOINTS) MI_FAIL(MI355_EINVAL, "teacher_select: bad joint count (K=%d, 1..%d)", K, MI355_OCC_MAX_JOINTS);
  if (N < 0 || N > MI355_OCC_MAX_BOXES) MI_FAIL(MI355_EINVAL, "teacher_select: N=%d boxes per sample, 0..%d", N, MI355_OCC_MAX_BOXES);
  if (!__builtin_isfinite(tau)) MI_FAIL(MI355_EINVAL, "teacher_select: tau must be finite, got %g", (double)tau);
  if (!(prob >= 0.f && prob <= 1.f)) MI_FAIL(MI355_EINVAL, "teacher_select: prob must lie in [0, 1], got %g", (double)prob);
  if (N > 0) {
    if (!xy) MI_FAIL(MI355_EINVAL, "teacher_select: null xy");
    if (!u) MI_FAIL(MI355_EINVAL, "teacher_select: null u");
    if (!boxes) MI_FAIL(MI355_EINVAL, "teacher_select: null boxes");
    if (!count) MI_FAIL(MI355_EINVAL, "teacher_select: null count");
    if (S < 1 || S > MI355_OCC_MAX_SIDE || H < 1 || W < 1 || S % H != 0 || S % W != 0)
      MI_FAIL(MI355_EINVAL, "teacher_select: the image side S=%d (1..%d) must be a multiple of the heat-map sides H=%d and W=%d", S, MI355_OCC_MAX_SIDE, H, W);
    if (lo < 1) MI_FAIL(MI355_EINVAL, "teacher_select: lo=%d must be at least 1", lo);
    if (lo > hi) MI_FAIL(MI355_EINVAL, "teacher_select: lo=%d above hi=%d", lo, hi);
    if (hi > S) MI_FAIL(MI355_EINVAL, "teacher_select: hi=%d above the image side S=%d", hi, S);
  }
  if (((uintptr_t)p | (uintptr_t)xy | (uintptr_t)gate_in | (uintptr_t)w_in | (uintptr_t)u | (uintptr_t)conf | (uintptr_t)w_out |
       (uintptr_t)boxes | (uintptr_t)count | (uintptr_t)stats) & 3)
    MI_FAIL(MI355_EINVAL, "teacher_select: pointers must be 4-byte aligned");
  char lab[64];
  if (prof_on()) snprintf(lab, sizeof(lab), "teacher_select B%d K%d N%d", B, K, N);
  ProfScope ps(as_stream(stream), 0.0, 24.0 * B * K + 20.0 * B * N, 2, prof_on() ? lab : nullptr);
  hipLaunchKernelGGL(teacher_select_kernel, dim3(1), dim3(256), 0, as_stream(stream), p, xy, gate_in, w_in, u, tau, prob, N, lo, hi, S, H, W,
                     conf, w_out, boxes, count, stats, B, K);
  MI_CHECK_LAUNCH("teacher_select");
  return MI355_OK;
}

extern "C" int mi355_occlude_images(const float* x, const int32_t* boxes, int N, float* out, int B, int C, int H, int W, void* stream) {
  if (!x) MI_FAIL(MI355_EINVAL, "occlude_images: null x");
  if (!out) MI_FAIL(MI355_EINVAL, "occlude_images: null out");
  if (N < 0 || N > MI355_OCC_MAX_BOXES) MI_FAIL(MI355_EINVAL, "occlude_images: N=%d boxes per sample, 0..%d", N, MI355_OCC_MAX_BOXES);
  if (N > 0 && !boxes) MI_FAIL(MI355_EINVAL, "occlude_images: null boxes");
  if (B < 1 || B > MI355_OCC_MAX_BATCH || C < 1 || H < 1 || W < 1 || H > MI355_OCC_MAX_SIDE || W > MI355_OCC_MAX_SIDE)
    MI_FAIL(MI355_EINVAL, "occlude_images: bad shape (B=%d C=%d H=%d W=%d; B up to %d, sides up to %d)", B, C, H, W, MI355_OCC_MAX_BATCH, MI355_OCC_MAX_SIDE);
  const long plane = (long)C * H * W;
  if (plane >= (1L << 31)) MI_FAIL(MI355_EINVAL, "occlude_images: a sample of C*H*W=%ld words, must be below 2^31", plane);
  if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)boxes) & 3) MI_FAIL(MI355_EINVAL, "occlude_images: x, out and boxes must be 4-byte aligned");
  if (occ_overlap(x, 4L * B * plane, out, 4L * B * plane)) MI_FAIL(MI355_EINVAL, "occlude_images: x and out overlap");
  if (N > 0 && occ_overlap(boxes, 16L * B * N, out, 4L * B * plane)) MI_FAIL(MI355_EINVAL, "occlude_images: boxes and out overlap");
  hipStream_t st = as_stream(stream);
  const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const long items = vec ? plane >> 2 : plane;
  // about 2048 blocks over the batch (at least one per sample), each walking its share of one sample
  long per = 2048 / B; if (per < 1) per = 1;
  long gx = cdiv(items, 256); if (gx > per) gx = per; if (gx < 1) gx = 1;
  char lab[80];
  if (prof_on()) snprintf(lab, sizeof(lab), "occlude_images %dx%dx%dx%d N%d%s", B, C, H, W, N, vec ? "" : " scalar");
  ProfScope ps(st, 0.0, 8.0 * B * plane + 16.0 * B * N, 2, prof_on() ? lab : nullptr);
  if (vec) hipLaunchKernelGGL(occlude_images_kernel<true>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, (const unsigned*)x, boxes, N,
                              (unsigned*)out, (unsigned)plane, (unsigned)(H * W), (unsigned)W);
  else hipLaunchKernelGGL(occlude_images_kernel<false>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, (const unsigned*)x, boxes, N,
                          (unsigned*)out, (unsigned)plane, (unsigned)(H * W), (unsigned)W);
  MI_CHECK_LAUNCH("occlude_images");
  return MI355_OK;
}

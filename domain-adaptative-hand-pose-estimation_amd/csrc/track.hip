// Hand tracking: the crop of a hand's square out of a uint8 frame (resize, mirror, normalise) and the per-hand update that maps
// the decoded key points back to the frame and writes the next frame's box -- both driven by 32-byte records in device memory
// that the host never reads.  Forward only.  The arithmetic is stated in include/mi355pose.h and restated in numpy by
// tests/track_ref.py: fp32, every operation rounded on its own whatever the build's flags say; with fx == 0 the second tap is not read.
#include "common.h"
#include <cmath>

static_assert(sizeof(mi355_track_rec) == 32, "mi355_track_rec is eight words");
static_assert(sizeof(mi355_track_params) == 40, "mi355_track_params is ten words");

constexpr int TK_TILE = 32;                   // a workgroup writes a 32 x 32 tile: 256 threads, 4 adjacent pixels each

struct TkNorm { float mean[3], stdv[3]; };

__device__ __forceinline__ bool tk_bounded(float v) { return fabsf(v) <= MI355_TRACK_MAX_COORD; }            // false for NaN, inf
// live, position and size of a record (header: USABLE, without the frame test): float comparisons only
__device__ __forceinline__ bool tk_usable(int live, float x0, float y0, float side, float four_s) {
  return live != 0 && tk_bounded(x0) && tk_bounded(y0) && side >= 1.0f && side <= four_s;
}
__device__ __forceinline__ float tk_blend(float v0, float v1, float f) {
#pragma clang fp contract(off)
  const float om = 1.0f - f;
  const float p = v0 * om;
  const float q = v1 * f;
  return p + q;
}
// fl(fl(o + fl(fl(j + off) * step)) - 0.5f)
__device__ __forceinline__ float tk_coord(float o, float j, float off, float step) {
#pragma clang fp contract(off)
  const float u = j + off;
  const float p = u * step;
  const float s = o + p;
  return s - 0.5f;
}

// One bilinear sample of the three channels of a Hf x Wf RGB frame at (xs, ys), the bytes looked up in the table T[3][256].  The
// range test comes before any conversion to an integer; inside it x0, y0 lie in [-1, Wf) x [-1, Hf), so every byte offset formed
// below is inside the frame.  A tap outside the frame is +0 and is not read, nor is the second tap of a pair when fx (fy) == 0.
__device__ __forceinline__ void tk_sample(const unsigned char* __restrict__ fr, const float (*T)[256], float xs, float ys, int Hf, int Wf,
                                          float* v) {
#pragma clang fp contract(off)
  if (!(xs > -1.0f && xs < (float)Wf && ys > -1.0f && ys < (float)Hf)) { v[0] = v[1] = v[2] = 0.0f; return; }
  const float xf = floorf(xs), yf = floorf(ys);
  const float fx = xs - xf, fy = ys - yf;
  const int x0 = (int)xf, y0 = (int)yf;
  auto row = [&](int y, float* r) {
    if (y < 0 || y >= Hf) { r[0] = r[1] = r[2] = 0.0f; return; }
    const unsigned char* __restrict__ line = fr + (long)y * Wf * 3;      // pixel x of this row: line + 3 x, formed for 0 <= x < Wf only
    float a[3] = {0.0f, 0.0f, 0.0f};
    if (x0 >= 0) { const unsigned char* p = line + 3 * x0; a[0] = T[0][p[0]]; a[1] = T[1][p[1]]; a[2] = T[2][p[2]]; }
    if (fx == 0.0f) { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; return; }
    float b[3] = {0.0f, 0.0f, 0.0f};
    if (x0 + 1 < Wf) { const unsigned char* p = line + 3 * (x0 + 1); b[0] = T[0][p[0]]; b[1] = T[1][p[1]]; b[2] = T[2][p[2]]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = tk_blend(a[c], b[c], fx);
  };
  float r0[3];
  row(y0, r0);
  if (fy == 0.0f) { v[0] = r0[0]; v[1] = r0[1]; v[2] = r0[2]; return; }
  float r1[3];
  row(y0 + 1, r1);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = tk_blend(r0[c], r1[c], fy);
}

// ---------------------------------------------------------------- crop, resize, mirror, normalise
// A streaming kernel: every output pixel written once, the taps gathered through the caches.  The eight words of the record go
// through LDS (one read per workgroup) next to the 3 x 256 table of normalised byte values, so the inner loop holds no division
// but the one by n * n.  VEC: one 16-byte store per thread and channel (host: out 16-byte aligned; S % 16 == 0 does the rest).
template <bool VEC>
__global__ __launch_bounds__(256) void roi_crop_kernel(const unsigned char* __restrict__ frames, int F, int Hf, int Wf,
                                                        const mi355_track_rec* __restrict__ recs, int S, int tiles_x, TkNorm nm,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float s_T[3][256];
  __shared__ int s_rec[8];
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_x;
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  if (tid < 8) s_rec[tid] = reinterpret_cast<const int*>(recs + b)[tid];
#pragma unroll
  for (int c = 0; c < 3; ++c) s_T[c][tid] = ((float)tid / 255.0f - nm.mean[c]) / nm.stdv[c];
  __syncthreads();
  const int i = ty * TK_TILE + (tid >> 3), j0 = tx * TK_TILE + (tid & 7) * 4;
  if (i >= S || j0 >= S) return;                             // (S % 16 == 0: a quad is inside the row or outside it)
  const int frame = s_rec[0], mirror = s_rec[4], live = s_rec[5];
  const float x0 = __int_as_float(s_rec[1]), y0 = __int_as_float(s_rec[2]), side = __int_as_float(s_rec[3]);
  const float Sf = (float)S;
  const long plane = (long)S * S;
  float* __restrict__ dst = out + (long)b * 3 * plane + (long)i * S + j0;
  float px[3][4];
  if (!(tk_usable(live, x0, y0, side, 4.0f * Sf) && frame >= 0 && frame < F)) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) px[c][q] = 0.0f;
  } else {
    const unsigned char* __restrict__ fr = frames + (long)frame * Hf * Wf * 3;
    const float step = side / Sf;
    const int n = side <= Sf ? 1 : (side <= 2.0f * Sf ? 2 : (side <= 3.0f * Sf ? 3 : 4));
    const float nf = (float)n, nn = (float)(n * n);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + q;
      const float fj = (float)(mirror ? S - 1 - j : j), fi = (float)i;
      float acc[3] = {0.0f, 0.0f, 0.0f};
      for (int ay = 0; ay < n; ++ay) {
        const float ys = tk_coord(y0, fi, ((float)ay + 0.5f) / nf, step);
        for (int ax = 0; ax < n; ++ax) {
          const float xs = tk_coord(x0, fj, ((float)ax + 0.5f) / nf, step);
          float v[3];
          tk_sample(fr, s_T, xs, ys, Hf, Wf, v);
          if (ay == 0 && ax == 0) { acc[0] = v[0]; acc[1] = v[1]; acc[2] = v[2]; }
          else { acc[0] = acc[0] + v[0]; acc[1] = acc[1] + v[1]; acc[2] = acc[2] + v[2]; }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c][q] = acc[c] / nn;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (VEC) *reinterpret_cast<float4*>(dst + c * plane) = make_float4(px[c][0], px[c][1], px[c][2], px[c][3]);
    else {
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[c * plane + q] = px[c][q];
    }
  }
}

static bool track_overlap(const void* p, long np, const void* q, long nq) {    // [p, p + np) and [q, q + nq), in bytes
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
static bool track_side_ok(int S) { return S >= 16 && S <= MI355_TRACK_MAX_SIDE && S % 16 == 0; }
static bool track_finite(float v) { return std::fabs(v) <= 3.4028234663852886e38f; }    // false for NaN, inf

extern "C" int mi355_roi_crop_normalize(const unsigned char* frames, int F, int Hf, int Wf, const mi355_track_rec* recs, int N, int S,
                                        const float* norm, float* out, void* stream) {
  if (!frames) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: frames is null");
  if (!recs) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: recs is null");
  if (!norm) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: norm is null");
  if (!out) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: out is null");
  if (F < 1) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: F=%d (at least 1)", F);
  if (Hf < 1 || Hf > MI355_TRACK_MAX_FRAME) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: Hf=%d outside 1..%d", Hf, MI355_TRACK_MAX_FRAME);
  if (Wf < 1 || Wf > MI355_TRACK_MAX_FRAME) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: Wf=%d outside 1..%d", Wf, MI355_TRACK_MAX_FRAME);
  if (N < 1) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: N=%d (at least 1)", N);
  if (!track_side_ok(S)) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: S=%d is not a multiple of 16 from 16 to %d", S, MI355_TRACK_MAX_SIDE);
  for (int c = 0; c < 3; ++c) {
    if (!track_finite(norm[c])) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: norm mean[%d]=%g is not finite", c, (double)norm[c]);
    if (!(norm[3 + c] > 0.0f) || !track_finite(norm[3 + c]))
      MI_FAIL(MI355_EINVAL, "roi_crop_normalize: norm std[%d]=%g must be finite and > 0", c, (double)norm[3 + c]);
  }
  if ((uintptr_t)recs & 3) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: recs must be 4-byte aligned");
  if ((uintptr_t)out & 3) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: out must be 4-byte aligned");
  const long frame_bytes = 3L * Hf * Wf;
  if ((long)F > (1L << 40) / frame_bytes) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: too large (F=%d Hf=%d Wf=%d)", F, Hf, Wf);
  const int tiles_x = cdiv(S, TK_TILE);
  const long tiles = (long)tiles_x * tiles_x;
  if ((long)N > 0x7fffffffL / tiles) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: too large (N=%d S=%d: the blocks are beyond the grid)", N, S);
  const long nout = 12L * N * S * S, nrec = (long)sizeof(mi355_track_rec) * N, nfr = frame_bytes * F;
  if (track_overlap(out, nout, frames, nfr)) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: out and frames overlap");
  if (track_overlap(out, nout, recs, nrec)) MI_FAIL(MI355_EINVAL, "roi_crop_normalize: out and recs overlap");
  TkNorm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = norm[c]; nm.stdv[c] = norm[3 + c]; }
  const bool vec = ((uintptr_t)out & 15) == 0;
  char lab[96];
  snprintf(lab, sizeof(lab), "roi_crop %dx3x%dx%d from %dx%dx%d%s", N, S, S, F, Hf, Wf, vec ? "" : " scalar");
  ProfScope ps(as_stream(stream), 0.0, (double)nout + (double)nrec, 2, lab);
  const dim3 grid((unsigned)(N * tiles));
  if (vec) hipLaunchKernelGGL(roi_crop_kernel<true>, grid, dim3(256), 0, as_stream(stream), frames, F, Hf, Wf, recs, S, tiles_x, nm, out);
  else hipLaunchKernelGGL(roi_crop_kernel<false>, grid, dim3(256), 0, as_stream(stream), frames, F, Hf, Wf, recs, S, tiles_x, nm, out);
  MI_CHECK_LAUNCH("roi_crop_normalize");
  return MI355_OK;
}

// ---------------------------------------------------------------- key points back to the frame, the next box
// One thread per hand: K <= 64 joints walked twice in ascending order (the map-back with the visibility and the score, then
// nothing but registers).  The record is read completely before anything is written, so rec_out may be rec_in.
// (No __restrict__ on the record pointers: rec_out may be rec_in.)
__global__ __launch_bounds__(64) void track_update_kernel(const mi355_track_rec* rec_in, const float* __restrict__ xy,
                                                           const float* __restrict__ conf, mi355_track_params P, float* __restrict__ kp,
                                                           float* __restrict__ vis, float* __restrict__ score,
                                                           mi355_track_rec* rec_out, int N, int K) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  const mi355_track_rec r = rec_in[b];
  const float Sf = (float)P.S, Wff = (float)P.Wf, Hff = (float)P.Hf;
  const float four_s = 4.0f * Sf;
  float* __restrict__ kpb = kp + (long)b * K * 2;
  float* __restrict__ visb = vis + (long)b * K;
  mi355_track_rec o = r;
  if (!tk_usable(r.live, r.x0, r.y0, r.side, four_s)) {
    for (int k = 0; k < K; ++k) { kpb[2 * k] = 0.0f; kpb[2 * k + 1] = 0.0f; visb[k] = 0.0f; }
    score[b] = 0.0f;
    o.live = 0;                                              // "rec_in with live = 0": nothing else changes
    rec_out[b] = o;
    return;
  }
  o.reserved = 0;
  const float* __restrict__ xyb = xy + (long)b * K * 2;
  const float* __restrict__ cb = conf + (long)b * K;
  const float st = r.side / Sf;
  const float sm1 = Sf - 1.0f;
  int m = 0;
  float sum = 0.0f, lx = 0.0f, ux = 0.0f, ly = 0.0f, uy = 0.0f;
  for (int k = 0; k < K; ++k) {
    const float x = xyb[2 * k], y = xyb[2 * k + 1], c = cb[k];
    const float xm = r.mirror ? sm1 - x : x;
    const float px = xm * st, py = y * st;
    const float kx = r.x0 + px, ky = r.y0 + py;
    const bool fin = fabsf(kx) < INFINITY && fabsf(ky) < INFINITY;        // false for NaN, inf
    const bool v = fin && c >= P.tau;
    kpb[2 * k] = fin ? kx : 0.0f;
    kpb[2 * k + 1] = fin ? ky : 0.0f;
    visb[k] = v ? 1.0f : 0.0f;
    if (v) {
      sum = sum + c;
      if (m == 0) { lx = ux = kx; ly = uy = ky; }
      else {
        lx = kx < lx ? kx : lx; ux = kx > ux ? kx : ux;
        ly = ky < ly ? ky : ly; uy = ky > uy ? ky : uy;
      }
      ++m;
    }
  }
  score[b] = m > 0 ? sum / (float)m : 0.0f;
  float cap = Wff < Hff ? Wff : Hff;
  cap = four_s < cap ? four_s : cap;
  auto clamp = [&](float s) { const float t = s < P.min_side ? P.min_side : s; return t > cap ? cap : t; };
  const float hx = r.side * 0.5f;
  float cx = r.x0 + hx, cy = r.y0 + hx, side = r.side;
  bool dead = false;
  if (m >= P.min_joints) {
    const float w = ux - lx, h = uy - ly;
    const float e = w > h ? w : h;
    const float sn = clamp(P.scale * e);
    const float sx = lx + ux, sy = ly + uy;
    const float nx = sx * 0.5f, ny = sy * 0.5f;
    const float dx = nx - cx, dy = ny - cy, ds = sn - side;
    const float ax = P.alpha * dx, ay = P.alpha * dy, as = P.alpha * ds;
    cx = cx + ax; cy = cy + ay;
    side = clamp(side + as);
    o.lost = 0;
  } else {
    o.lost = r.lost < 0 ? 1 : (r.lost >= P.max_lost ? P.max_lost + 1 : r.lost + 1);
    if (o.lost > P.max_lost) dead = true;
    else { const float t = side * P.grow; side = t > cap ? cap : t; }
  }
  if (dead) o.live = 0;
  else {
    const float h2 = side * 0.5f;
    auto shift = [&](float v, float L) { const float t = v < 0.0f ? 0.0f : v; const float hi = L - side; return t > hi ? hi : t; };
    o.x0 = shift(cx - h2, Wff);
    o.y0 = shift(cy - h2, Hff);
    o.side = side;
    o.live = 1;
  }
  rec_out[b] = o;
}

extern "C" int mi355_track_update(const mi355_track_rec* rec_in, const float* xy, const float* conf, mi355_track_params P, float* kp,
                                  float* vis, float* score, mi355_track_rec* rec_out, int N, int K, void* stream) {
  const struct { const char* name; const void* p; } ptrs[7] = {{"rec_in", rec_in}, {"xy", xy}, {"conf", conf}, {"kp", kp}, {"vis", vis},
                                                                {"score", score}, {"rec_out", rec_out}};
  for (const auto& a : ptrs) if (!a.p) MI_FAIL(MI355_EINVAL, "track_update: %s is null", a.name);
  if (N < 1) MI_FAIL(MI355_EINVAL, "track_update: N=%d (at least 1)", N);
  if (K < 1 || K > MI355_TRACK_MAX_JOINTS) MI_FAIL(MI355_EINVAL, "track_update: K=%d outside 1..%d", K, MI355_TRACK_MAX_JOINTS);
  if (!track_finite(P.tau)) MI_FAIL(MI355_EINVAL, "track_update: tau=%g is not finite", (double)P.tau);
  if (P.min_joints < 1 || P.min_joints > K) MI_FAIL(MI355_EINVAL, "track_update: min_joints=%d outside 1..K=%d", P.min_joints, K);
  if (!(P.scale > 0.0f) || !track_finite(P.scale)) MI_FAIL(MI355_EINVAL, "track_update: scale=%g must be finite and > 0", (double)P.scale);
  if (!(P.alpha >= 0.0f && P.alpha <= 1.0f)) MI_FAIL(MI355_EINVAL, "track_update: alpha=%g outside [0, 1]", (double)P.alpha);
  if (!(P.grow >= 1.0f) || !track_finite(P.grow)) MI_FAIL(MI355_EINVAL, "track_update: grow=%g must be finite and >= 1", (double)P.grow);
  if (P.max_lost < 0 || P.max_lost > (1 << 30)) MI_FAIL(MI355_EINVAL, "track_update: max_lost=%d outside 0..2^30", P.max_lost);
  if (!(P.min_side >= 1.0f) || !track_finite(P.min_side)) MI_FAIL(MI355_EINVAL, "track_update: min_side=%g must be finite and >= 1", (double)P.min_side);
  if (P.Wf < 1 || P.Wf > MI355_TRACK_MAX_FRAME) MI_FAIL(MI355_EINVAL, "track_update: Wf=%d outside 1..%d", P.Wf, MI355_TRACK_MAX_FRAME);
  if (P.Hf < 1 || P.Hf > MI355_TRACK_MAX_FRAME) MI_FAIL(MI355_EINVAL, "track_update: Hf=%d outside 1..%d", P.Hf, MI355_TRACK_MAX_FRAME);
  if (!track_side_ok(P.S)) MI_FAIL(MI355_EINVAL, "track_update: S=%d is not a multiple of 16 from 16 to %d", P.S, MI355_TRACK_MAX_SIDE);
  for (const auto& a : ptrs) if ((uintptr_t)a.p & 3) MI_FAIL(MI355_EINVAL, "track_update: %s must be 4-byte aligned", a.name);
  const long nk = (long)N * K, nrec = (long)sizeof(mi355_track_rec) * N;
  const long bytes[7] = {nrec, 8 * nk, 4 * nk, 8 * nk, 4 * nk, 4L * N, nrec};
  for (int o = 3; o < 7; ++o) {
    for (int i = 0; i < 3; ++i) {
      if (o == 6 && i == 0 && rec_out == rec_in) continue;                       // in place
      if (track_overlap(ptrs[o].p, bytes[o], ptrs[i].p, bytes[i])) MI_FAIL(MI355_EINVAL, "track_update: %s and %s overlap", ptrs[o].name, ptrs[i].name);
    }
    for (int p = o + 1; p < 7; ++p)
      if (track_overlap(ptrs[o].p, bytes[o], ptrs[p].p, bytes[p])) MI_FAIL(MI355_EINVAL, "track_update: %s and %s overlap", ptrs[o].name, ptrs[p].name);
  }
  char lab[64];
  snprintf(lab, sizeof(lab), "track_update N%d K%d", N, K);
  ProfScope ps(as_stream(stream), 0.0, 24.0 * nk + 2.0 * nrec + 4.0 * N, 2, lab);
  hipLaunchKernelGGL(track_update_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, as_stream(stream), rec_in, xy, conf, P, kp, vis, score,
                     rec_out, N, K);
  MI_CHECK_LAUNCH("track_update");
  return MI355_OK;
}

// Fourier-domain source stylisation (Yang and Soatto, "FDA: Fourier Domain Adaptation for Semantic Segmentation", CVPR 2020; not
// in the reference): the low-frequency amplitude of every source plane replaced by that of the target plane of the same index,
// the source phase kept.  Only the (2b+1)^2 lowest frequencies are touched, so no FFT is taken: the window of both spectra is a
// partial DFT (launch 1, per stripe of 32 rows, partial sums to the workspace) and the change to the image is the inverse partial
// DFT of the amplitude difference (launch 2).  Twiddles, sums, magnitudes and the inverse sum are fp64 on fp32 operands with ONE
// rounding to fp32 at the store.  No atomics, fixed summation orders: the same bits on every run.  Semantics: include/mi355pose.h.
#include "common.h"
#include <math.h>

#define FDA_ROWS 32                      // rows of one spectrum stripe: lane = (row, slot), 256 / 32 = 8 slots
#define FDA_SLOTS 8
#define FDA_KMAX 5                       // frequencies one slot may own: ceil((MI355_FDA_MAX_B + 1) / FDA_SLOTS)
#define FDA_RPT 4                        // apply: rows (of four pixels each) one lane accumulates at a time
#define FDA_MAX_RG 4                     // apply: at most this many row groups of FDA_RPT rows in one pass

struct FdaNorm { float mean[4], std[4]; };

// e^{+2 pi i k / N} for k = 0 .. N/2 (the other half is its mirror image: fda_tw).  sincospi is exact at k = 0 and 2k = N.
__device__ __forceinline__ void fda_build_tw(double2* __restrict__ tab, int N) {
  for (int k = threadIdx.x; k <= N / 2; k += 256) {
    double s, c;
    sincospi(2.0 * (double)k / (double)N, &s, &c);
    tab[k] = make_double2(c, s);
  }
}
__device__ __forceinline__ double2 fda_tw(const double2* __restrict__ tab, int k, int N) {      // 0 <= k < N
  const bool hi = 2 * k > N;
  const double2 t = tab[hi ? N - k : k];
  return make_double2(t.x, hi ? -t.y : t.y);
}
__device__ __forceinline__ int fda_wrap(int i, int N) { return i >= N ? i - N : i; }             // i < 2N
// The spectrum launch reads a twiddle per (v, x) and four FMAs: it keeps all N of e^{-2 pi i k / N}, so a lookup is one LDS read.
__device__ __forceinline__ void fda_build_conj(double2* __restrict__ tab, int N) {
  for (int k = threadIdx.x; k < N; k += 256) {
    double s, c;
    sincospi(2.0 * (double)(2 * k > N ? N - k : k) / (double)N, &s, &c);      // (the mirror image takes the same argument)
    tab[k] = make_double2(c, 2 * k > N ? s : -s);
  }
}
// Frequency slots of the row transform: the fewest (a power of two) whose FDA_KMAX frequencies each cover nv; the other slots split
// the columns, so that a pixel is loaded by as few lanes as possible.
__host__ __device__ __forceinline__ int fda_nvs(int nv) {
  int nvs = 1;
  while (nvs * FDA_KMAX < nv) nvs <<= 1;
  return nvs;
}

// Launch 1.  Block = one stripe of 32 rows of one plane, of x_s and of x_t.  Stage 1: lane (row, slot) forms the row transform
// R[row, v] = sum_x p[row, x] e^{-2 pi i v x / W} of both images for the frequencies v and the share of the columns its slot owns
// (nvs frequency slots x xs column shares = 8, fda_nvs; the twiddle of a (v, x) is read once for both images).  Stage 2: the column
// twiddles: F[u, v] = sum_row R[row, v] e^{-2 pi i u y / H}, u in [-b, b], v in [0, b], written to ws[plane][stripe][image].
// E = 4: rows read as float4 (x_s, x_t 16-byte aligned, W % 4 == 0); E = 1: float by float.
template <int E>
__global__ __launch_bounds__(256) void fda_spectrum_kernel(const float* __restrict__ x_s, const float* __restrict__ x_t,
                                                            double2* __restrict__ ws, int H, int W, int b, int S) {
  extern __shared__ double2 fda_lds[];
  const int nv = b + 1, n = 2 * b + 1, tid = threadIdx.x;
  double2* __restrict__ tw = fda_lds;
  double2* __restrict__ R = fda_lds + (H > W ? H : W);                      // [image][column share][row][nv]
  const int stripe = blockIdx.x % S;
  const long plane = blockIdx.x / S;
  const int row = tid & (FDA_ROWS - 1), slot = tid >> 5;
  const int nvs = fda_nvs(nv), sh = __ffs(nvs) - 1;
  const int xs = FDA_SLOTS / nvs, jv = slot & (nvs - 1), jx = slot >> sh;
  const int y0 = stripe * FDA_ROWS, y = y0 + row;
  const bool live = y < H;
  fda_build_conj(tw, W);
  __syncthreads();

  double sr[FDA_KMAX], si[FDA_KMAX], tr[FDA_KMAX], ti[FDA_KMAX];
  int idx[FDA_KMAX], jump[FDA_KMAX];
#pragma unroll
  for (int k = 0; k < FDA_KMAX; ++k) {
    const int v = jv + nvs * k;
    sr[k] = si[k] = tr[k] = ti[k] = 0.0;
    idx[k] = (v * E * jx) % W;
    jump[k] = (v * E * (xs - 1)) % W;
  }
  if (live) {
    const float* __restrict__ ps = x_s + (plane * H + y) * W;
    const float* __restrict__ pt = x_t + (plane * H + y) * W;
    const int nchunk = W / E;
    for (int c = jx; c < nchunk; c += xs) {
      float a[E], q[E];
      if constexpr (E == 4) {
        const float4 fa = reinterpret_cast<const float4*>(ps)[c], fq = reinterpret_cast<const float4*>(pt)[c];
        a[0] = fa.x; a[1] = fa.y; a[2] = fa.z; a[3] = fa.w;
        q[0] = fq.x; q[1] = fq.y; q[2] = fq.z; q[3] = fq.w;
      } else {
        a[0] = ps[c]; q[0] = pt[c];
      }
#pragma unroll
      for (int k = 0; k < FDA_KMAX; ++k) {
        const int v = jv + nvs * k;
        if (v < nv) {
          int i = idx[k];
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const double2 w = tw[i];
            const double da = (double)a[e], dq = (double)q[e];
            sr[k] = fma(da, w.x, sr[k]); si[k] = fma(da, w.y, si[k]);
            tr[k] = fma(dq, w.x, tr[k]); ti[k] = fma(dq, w.y, ti[k]);
            i = fda_wrap(i + v, W);
          }
          idx[k] = fda_wrap(i + jump[k], W);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < FDA_KMAX; ++k) {
    const int v = jv + nvs * k;
    if (v < nv) {
      R[((0 * xs + jx) * FDA_ROWS + row) * nv + v] = make_double2(sr[k], si[k]);
      R[((1 * xs + jx) * FDA_ROWS + row) * nv + v] = make_double2(tr[k], ti[k]);
    }
  }
  __syncthreads();
  if (xs > 1) {                                        // the column shares of a row, in their order, into share 0
    for (int i = tid; i < 2 * FDA_ROWS * nv; i += 256) {
      const int img = i / (FDA_ROWS * nv), rest = i - img * (FDA_ROWS * nv);
      double2 acc = R[(img * xs) * FDA_ROWS * nv + rest];
      for (int j = 1; j < xs; ++j) {
        const double2 p = R[(img * xs + j) * FDA_ROWS * nv + rest];
        acc.x += p.x; acc.y += p.y;
      }
      R[(img * xs) * FDA_ROWS * nv + rest] = acc;
    }
  }
  if (H != W) fda_build_conj(tw, H);                   // (every lane is past its last read of the row twiddles)
  __syncthreads();

  const int rows = (H - y0 < FDA_ROWS) ? H - y0 : FDA_ROWS;
  const double2* __restrict__ Rs = R;
  const double2* __restrict__ Rt = R + xs * FDA_ROWS * nv;
  double2* __restrict__ dst = ws + ((plane * S + stripe) * 2) * (long)(n * nv);
  for (int o = tid; o < n * nv; o += 256) {
    const int ui = o / nv, v = o - ui * nv;
    const int um = (ui < b) ? ui - b + H : ui - b;     // u mod H
    int i = (um * y0) % H;
    double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double2 w = tw[i];                         // e^{-2 pi i u y / H}
      const double2 p = Rs[r * nv + v], q = Rt[r * nv + v];
      ar = fma(p.x, w.x, fma(-p.y, w.y, ar)); ai = fma(p.y, w.x, fma(p.x, w.y, ai));
      br = fma(q.x, w.x, fma(-q.y, w.y, br)); bi = fma(q.y, w.x, fma(q.x, w.y, bi));
      i = fda_wrap(i + um, H);
    }
    dst[o] = make_double2(ar, ai);
    dst[n * nv + o] = make_double2(br, bi);
  }
}

// Launch 2.  Block = `rpb` rows (a multiple of 32) of one plane.  Folds the plane's S stripe partials in stripe order, folds the
// de-normalisation into them (times std; plus mean H W at DC), forms D[u, v] = (|Ft| - |Fs|) Fs / |Fs| (phase factor 1 where
// |Fs| == 0) scaled by 1 / (H W std) and doubled for v > 0 (D is Hermitian: the v < 0 half is the conjugate), then per pass of
// up to 16 rows G[y, v] = sum_u D[u, v] e^{2 pi i u y / H} (v = 0: from u >= 0 alone, real by construction) and
// out[y, x] = fl32(x_s[y, x] + sum_v Re(G[y, v] e^{2 pi i v x / W})).  Lane = four consecutive pixels of FDA_RPT rows.
template <int E>
__global__ __launch_bounds__(256) void fda_apply_kernel(const float* __restrict__ x_s, float* __restrict__ out,
                                                         const double2* __restrict__ ws, FdaNorm nm, int C, int H, int W, int b,
                                                         int S, int SA, int rpb) {
  extern __shared__ double2 fda_lds[];
  const int nv = b + 1, n = 2 * b + 1, nn = n * nv, tid = threadIdx.x;
  double2* __restrict__ twW = fda_lds;
  double2* __restrict__ twH = twW + (W / 2 + 1);
  double2* __restrict__ D = twH + (H / 2 + 1);
  double2* __restrict__ G = D + nn;                                          // [FDA_MAX_RG * FDA_RPT][nv]
  const int sa = blockIdx.x % SA;
  const long plane = blockIdx.x / SA;
  const int ch = (int)(plane % C);
  fda_build_tw(twW, W);
  fda_build_tw(twH, H);
  {
    const double sd = (double)nm.std[ch], dc = (double)nm.mean[ch] * (double)H * (double)W;
    const double inv = 1.0 / ((double)H * (double)W * sd);
    const double2* __restrict__ src = ws + (plane * S * 2) * (long)nn;
    for (int o = tid; o < nn; o += 256) {
      double fr = 0.0, fi = 0.0, gr = 0.0, gi = 0.0;
      for (int st = 0; st < S; ++st) {
        const double2 p = src[(long)(2 * st) * nn + o], q = src[(long)(2 * st + 1) * nn + o];
        fr += p.x; fi += p.y; gr += q.x; gi += q.y;
      }
      fr *= sd; fi *= sd; gr *= sd; gi *= sd;
      if (o == b * nv) { fr += dc; gr += dc; }
      const double as = sqrt(fr * fr + fi * fi), at = sqrt(gr * gr + gi * gi);
      const double d = at - as;
      const double k = ((o % nv) ? 2.0 : 1.0) * inv;
      double dr, di;
      if (as == 0.0) { dr = d; di = 0.0; }
      else { dr = d * (fr / as); di = d * (fi / as); }
      D[o] = make_double2(dr * k, di * k);
    }
  }
  __syncthreads();

  const int W4 = (W + 3) >> 2;                                              // lanes a row takes (<= 256)
  int nrg = 256 / W4;
  if (nrg > FDA_MAX_RG) nrg = FDA_MAX_RG;
  const int GR = nrg * FDA_RPT;
  const int rg = tid / W4, c4 = tid - rg * W4;
  const bool active = rg < nrg;
  const int y0 = sa * rpb, yend = (y0 + rpb < H) ? y0 + rpb : H;
  int xe[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) xe[e] = (4 * c4 + e < W) ? 4 * c4 + e : 0;     // (a column past the row: computed, never stored)

  for (int g0 = y0; g0 < yend; g0 += GR) {
    for (int i = tid; i < GR * nv; i += 256) {
      const int r = i / nv, v = i - r * nv, y = g0 + r;
      double gr = 0.0, gi = 0.0;
      if (y < yend) {
        if (v == 0) {
          int j = 0;
          double acc = 0.0;
          for (int u = 1; u <= b; ++u) {
            j = fda_wrap(j + y, H);
            const double2 w = fda_tw(twH, j, H), d = D[(b + u) * nv];
            acc = fma(d.x, w.x, fma(-d.y, w.y, acc));
          }
          gr = D[b * nv].x + acc;                     // (D[u > 0, 0] carries no factor 2: the u < 0 half is added here)
          gr += acc;
        } else {
          int j = (b * y) % H;
          j = j ? H - j : 0;                           // (-b y) mod H
          for (int ui = 0; ui < n; ++ui) {
            const double2 w = fda_tw(twH, j, H), d = D[ui * nv + v];
            gr = fma(d.x, w.x, fma(-d.y, w.y, gr));
            gi = fma(d.x, w.y, fma(d.y, w.x, gi));
            j = fda_wrap(j + y, H);
          }
        }
      }
      G[i] = make_double2(gr, gi);
    }
    __syncthreads();
    if (active) {
      double acc[FDA_RPT][4];
#pragma unroll
      for (int rr = 0; rr < FDA_RPT; ++rr)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[rr][e] = 0.0;
      int j[4] = {0, 0, 0, 0};
      const double2* __restrict__ Gr = G + rg * FDA_RPT * nv;
      for (int v = 0; v < nv; ++v) {
        double2 w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { w[e] = fda_tw(twW, j[e], W); j[e] = fda_wrap(j[e] + xe[e], W); }
#pragma unroll
        for (int rr = 0; rr < FDA_RPT; ++rr) {
          const double2 g = Gr[rr * nv + v];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[rr][e] = fma(g.x, w[e].x, fma(-g.y, w[e].y, acc[rr][e]));
        }
      }
#pragma unroll
      for (int rr = 0; rr < FDA_RPT; ++rr) {
        const int y = g0 + rg * FDA_RPT + rr;
        if (y < yend) {
          const long base = (plane * H + y) * W;
          if constexpr (E == 4) {
            const float4 p = reinterpret_cast<const float4*>(x_s + base)[c4];
            reinterpret_cast<float4*>(out + base)[c4] = make_float4((float)((double)p.x + acc[rr][0]), (float)((double)p.y + acc[rr][1]),
                                                                    (float)((double)p.z + acc[rr][2]), (float)((double)p.w + acc[rr][3]));
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (4 * c4 + e < W) out[base + 4 * c4 + e] = (float)((double)x_s[base + 4 * c4 + e] + acc[rr][e]);
          }
        }
      }
    }
    __syncthreads();
  }
}

static bool fda_overlap(const void* p, long np, const void* q, long nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

static int fda_check_shape(const char* who, int B, int C, int H, int W, int b) {
  if (B < 1) MI_FAIL(MI355_EINVAL, "%s: B=%d (at least 1)", who, B);
  if (C < 1 || C > 4) MI_FAIL(MI355_EINVAL, "%s: C=%d (1 .. 4)", who, C);
  if (H < 1 || H > 1024) MI_FAIL(MI355_EINVAL, "%s: H=%d (1 .. 1024)", who, H);
  if (W < 1 || W > 1024) MI_FAIL(MI355_EINVAL, "%s: W=%d (1 .. 1024)", who, W);
  if (b < 0 || b > MI355_FDA_MAX_B) MI_FAIL(MI355_EINVAL, "%s: b=%d (0 .. MI355_FDA_MAX_B = %d)", who, b, MI355_FDA_MAX_B);
  if (2 * b + 1 > (H < W ? H : W)) MI_FAIL(MI355_EINVAL, "%s: b=%d: the window 2b+1 = %d is wider than min(H, W) = %d", who, b, 2 * b + 1, H < W ? H : W);
  if ((long)B * C * cdiv(H, FDA_ROWS) > 0x7fffffffL) MI_FAIL(MI355_EINVAL, "%s: B=%d too large for one launch (C=%d H=%d)", who, B, C, H);
  return MI355_OK;
}

static long fda_ws_bytes(int B, int C, int H, int W, int b) {
  return (long)B * C * cdiv(H, FDA_ROWS) * 2 * (2 * b + 1) * (b + 1) * (long)sizeof(double2);
}

extern "C" long mi355_fda_workspace_bytes(int B, int C, int H, int W, int b) {
  if (fda_check_shape("fda_workspace_bytes", B, C, H, W, b) != MI355_OK) return -1;
  return fda_ws_bytes(B, C, H, W, b);
}

extern "C" int mi355_fda_transfer(const float* x_s, const float* x_t, float* out, const float* mean, const float* std, int B, int C,
                                  int H, int W, int b, void* ws, long ws_bytes, void* stream) {
  const char* who = "fda_transfer";
  if (!x_s) MI_FAIL(MI355_EINVAL, "%s: x_s is null", who);
  if (!x_t) MI_FAIL(MI355_EINVAL, "%s: x_t is null", who);
  if (!out) MI_FAIL(MI355_EINVAL, "%s: out is null", who);
  if (!mean) MI_FAIL(MI355_EINVAL, "%s: mean is null", who);
  if (!std) MI_FAIL(MI355_EINVAL, "%s: std is null", who);
  if (!ws) MI_FAIL(MI355_EINVAL, "%s: ws is null", who);
  const int rc = fda_check_shape(who, B, C, H, W, b);
  if (rc != MI355_OK) return rc;
  FdaNorm nm;
  for (int c = 0; c < 4; ++c) { nm.mean[c] = 0.f; nm.std[c] = 1.f; }
  for (int c = 0; c < C; ++c) {
    if (!(std[c] > 0.f) || !isfinite(std[c])) MI_FAIL(MI355_EINVAL, "%s: std[%d]=%g (positive and finite)", who, c, (double)std[c]);
    if (!isfinite(mean[c])) MI_FAIL(MI355_EINVAL, "%s: mean[%d]=%g (finite)", who, c, (double)mean[c]);
    nm.mean[c] = mean[c]; nm.std[c] = std[c];
  }
  if ((uintptr_t)x_s & 3) MI_FAIL(MI355_EINVAL, "%s: x_s must be 4-byte aligned", who);
  if ((uintptr_t)x_t & 3) MI_FAIL(MI355_EINVAL, "%s: x_t must be 4-byte aligned", who);
  if ((uintptr_t)out & 3) MI_FAIL(MI355_EINVAL, "%s: out must be 4-byte aligned", who);
  if ((uintptr_t)ws & 15) MI_FAIL(MI355_EINVAL, "%s: ws must be 16-byte aligned", who);
  const long need = fda_ws_bytes(B, C, H, W, b), nx = 4L * B * C * H * W;
  if (ws_bytes < need) MI_FAIL(MI355_EINVAL, "%s: ws_bytes=%ld is too small (mi355_fda_workspace_bytes: %ld)", who, ws_bytes, need);
  if (fda_overlap(out, nx, x_s, nx)) MI_FAIL(MI355_EINVAL, "%s: out and x_s overlap", who);
  if (fda_overlap(out, nx, x_t, nx)) MI_FAIL(MI355_EINVAL, "%s: out and x_t overlap", who);
  if (fda_overlap(ws, need, x_s, nx)) MI_FAIL(MI355_EINVAL, "%s: ws and x_s overlap", who);
  if (fda_overlap(ws, need, x_t, nx)) MI_FAIL(MI355_EINVAL, "%s: ws and x_t overlap", who);
  if (fda_overlap(ws, need, out, nx)) MI_FAIL(MI355_EINVAL, "%s: ws and out overlap", who);

  const int nv = b + 1, n = 2 * b + 1, S = cdiv(H, FDA_ROWS);
  const long planes = (long)B * C;
  const double px = (double)planes * H * W;
  hipStream_t st = as_stream(stream);
  {
    const int xs = FDA_SLOTS / fda_nvs(nv);
    const size_t lds = sizeof(double2) * ((size_t)(H > W ? H : W) + 2 * (size_t)xs * FDA_ROWS * nv);        // at most 57 KB
    const bool vec = (W % 4 == 0) && ((((uintptr_t)x_s | (uintptr_t)x_t) & 15) == 0);
    char lab[96];
    snprintf(lab, sizeof(lab), "fda spectrum B%d C%d %dx%d b%d%s", B, C, H, W, b, vec ? "" : " scalar");
    // fp64 FMAs: two per pixel, image and frequency in the row transform, four per row, image and coefficient in the column one
    ProfScope ps(st, 2.0 * (4.0 * px * nv + 8.0 * (double)planes * H * n * nv), 8.0 * px + 2.0 * (double)need, 2, lab);
    if (vec) hipLaunchKernelGGL(fda_spectrum_kernel<4>, dim3((unsigned)(planes * S)), dim3(256), lds, st, x_s, x_t, (double2*)ws, H, W, b, S);
    else hipLaunchKernelGGL(fda_spectrum_kernel<1>, dim3((unsigned)(planes * S)), dim3(256), lds, st, x_s, x_t, (double2*)ws, H, W, b, S);
    MI_CHECK_LAUNCH("fda_transfer (spectrum)");
  }
  {
    const int sub = b <= 8 ? 1 : 2;                    // more rows per block where the fold of the partials is long
    const int rpb = FDA_ROWS * sub, SA = cdiv(H, rpb);
    const size_t lds = sizeof(double2) * ((size_t)(W / 2 + 1) + (size_t)(H / 2 + 1) + (size_t)n * nv + (size_t)FDA_MAX_RG * FDA_RPT * nv);
    const bool vec = (W % 4 == 0) && ((((uintptr_t)x_s | (uintptr_t)out) & 15) == 0);
    char lab[96];
    snprintf(lab, sizeof(lab), "fda apply B%d C%d %dx%d b%d%s", B, C, H, W, b, vec ? "" : " scalar");
    ProfScope ps(st, 2.0 * (2.0 * px * nv + 4.0 * (double)planes * H * n * nv), 8.0 * px + (double)need * SA, 2, lab);
    if (vec) hipLaunchKernelGGL(fda_apply_kernel<4>, dim3((unsigned)(planes * SA)), dim3(256), lds, st, x_s, out, (const double2*)ws, nm, C, H, W, b, S, SA, rpb);
    else hipLaunchKernelGGL(fda_apply_kernel<1>, dim3((unsigned)(planes * SA)), dim3(256), lds, st, x_s, out, (const double2*)ws, nm, C, H, W, b, S, SA, rpb);
    MI_CHECK_LAUNCH("fda_transfer (apply)");
  }
  return MI355_OK;
}

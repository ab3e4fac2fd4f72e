// Cross-domain mixup (uda/model/loss.py:13-24): the source-dominant and the target-dominant blend of two batches of images, of
// their heat-maps and the element-wise maximum of their joint weights, in ONE launch.  A pure stream: every input element is
// read once and feeds both blends; 16-byte accesses where the addresses allow, scalar otherwise.
#include "common.h"

// torch's `a * mix + b * (1. - mix)` rounding for rounding: om = fl(1 - lam) once per sample, then two products and one sum,
// each rounded on its own, whatever the build's flags say.
__device__ __forceinline__ float mix_om(float lam) {
#pragma clang fp contract(off)
  return 1.0f - lam;
}
__device__ __forceinline__ float mix1(float a, float b, float lam, float om) {
#pragma clang fp contract(off)
  const float p = a * lam;
  const float q = b * om;
  return p + q;
}

// One flat range of B samples of `plane` floats: lo = out[0, n) the source-dominant blend, hi = out[n, 2n) the target-dominant
// one, n = B * plane.  I is the index type of an element: unsigned where 2n fits 31 bits (one 32-bit division per vector), long
// otherwise.  A 16-byte vector straddles two samples whenever plane % 4 != 0: the coefficient is looked up per element then.
// `hi` is 16-byte aligned only when n % 4 == 0 (HI_VEC); its four floats go out one by one otherwise.
template <typename I, bool HI_VEC>
__device__ __forceinline__ void mix_range_vec(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ lo,
                                              const float* __restrict__ lam, long n, long plane) {
  float* __restrict__ hi = lo + n;
  const I n4 = (I)(n >> 2), P = (I)plane;
  const I stride = (I)gridDim.x * 256;
  for (I v = (I)blockIdx.x * 256 + threadIdx.x; v < n4; v += stride) {
    const I e = v * 4;
    const float4 x = reinterpret_cast<const float4*>(a)[v];
    const float4 y = reinterpret_cast<const float4*>(b)[v];
    const I s0 = e / P;
    const I left = (s0 + 1) * P - e;                  // elements of this vector's first sample from e on (>= 1)
    const float l0 = lam[s0], o0 = mix_om(l0);
    float l[4] = {l0, l0, l0, l0}, o[4] = {o0, o0, o0, o0};
    if (left < 4) {                                    // (plane may be shorter than a vector: up to four samples in one)
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        const I sj = (e + j) / P;
        l[j] = lam[sj]; o[j] = mix_om(l[j]);
      }
    }
    reinterpret_cast<float4*>(lo)[v] = make_float4(mix1(x.x, y.x, l[0], o[0]), mix1(x.y, y.y, l[1], o[1]),
                                                   mix1(x.z, y.z, l[2], o[2]), mix1(x.w, y.w, l[3], o[3]));
    const float4 t = make_float4(mix1(y.x, x.x, l[0], o[0]), mix1(y.y, x.y, l[1], o[1]),
                                 mix1(y.z, x.z, l[2], o[2]), mix1(y.w, x.w, l[3], o[3]));
    if (HI_VEC) reinterpret_cast<float4*>(hi)[v] = t;
    else { hi[e] = t.x; hi[e + 1] = t.y; hi[e + 2] = t.z; hi[e + 3] = t.w; }
  }
  for (long e = ((long)n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {   // n % 4 elements
    const float l0 = lam[e / plane], o0 = mix_om(l0);
    lo[e] = mix1(a[e], b[e], l0, o0);
    hi[e] = mix1(b[e], a[e], l0, o0);
  }
}

__device__ __forceinline__ void mix_range_scalar(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ lo,
                                                 const float* __restrict__ lam, long n, long plane) {
  float* __restrict__ hi = lo + n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const float l0 = lam[e / plane], o0 = mix_om(l0);
    const float x = a[e], y = b[e];
    lo[e] = mix1(x, y, l0, o0);
    hi[e] = mix1(y, x, l0, o0);
  }
}

struct MixRange { const float* a; const float* b; float* out; long n, plane; int vec, hi_vec, wide; };

__device__ __forceinline__ void mix_range(const MixRange& r, const float* __restrict__ lam) {
  if (!r.vec) mix_range_scalar(r.a, r.b, r.out, lam, r.n, r.plane);
  else if (r.wide) { if (r.hi_vec) mix_range_vec<long, true>(r.a, r.b, r.out, lam, r.n, r.plane);
                     else mix_range_vec<long, false>(r.a, r.b, r.out, lam, r.n, r.plane); }
  else { if (r.hi_vec) mix_range_vec<unsigned, true>(r.a, r.b, r.out, lam, r.n, r.plane);
         else mix_range_vec<unsigned, false>(r.a, r.b, r.out, lam, r.n, r.plane); }
}

// Capped grid, grid-stride: every block walks its share of the images, then of the heat-maps, then of the B * K weights.
__global__ __launch_bounds__(256) void mixup_pairs_kernel(MixRange img, MixRange hm, const float* __restrict__ w_s,
                                                           const float* __restrict__ w_t, float* __restrict__ w_mix, long nw,
                                                           const float* __restrict__ lam) {
  mix_range(img, lam);
  mix_range(hm, lam);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nw; e += (long)gridDim.x * 256) {
    const float m = fmaxf(w_s[e], w_t[e]);
    w_mix[e] = m;
    w_mix[nw + e] = m;
  }
}

static bool mix_overlap(const void* p, long np, const void* q, long nq) {      // [p, p + np) and [q, q + nq), in bytes
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

static MixRange mix_make_range(const float* a, const float* b, float* out, long n, long plane) {
  MixRange r;
  r.a = a; r.b = b; r.out = out; r.n = n; r.plane = plane;
  r.vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0) ? 1 : 0;
  r.hi_vec = (n % 4 == 0) ? 1 : 0;
  r.wide = (2 * n > 0x7fffffffL) ? 1 : 0;
  return r;
}

extern "C" int mi355_mixup_pairs(const float* x_s, const float* x_t, const float* hm_s, const float* hm_t, const float* w_s,
                                 const float* w_t, const float* lam, float* x_mix, float* hm_mix, float* w_mix, int B,
                                 long img_plane, long hm_plane, int K, void* stream) {
  if (!x_s || !x_t || !hm_s || !hm_t || !w_s || !w_t || !lam || !x_mix || !hm_mix || !w_mix)
    MI_FAIL(MI355_EINVAL, "mixup_pairs: null pointer");
  if (B < 1) MI_FAIL(MI355_EINVAL, "mixup_pairs: B=%d", B);
  if (img_plane < 1 || hm_plane < 1 || K < 1)
    MI_FAIL(MI355_EINVAL, "mixup_pairs: img_plane=%ld hm_plane=%ld K=%d (each at least 1)", img_plane, hm_plane, K);
  if (img_plane > (1L << 40) / B || hm_plane > (1L << 40) / B) MI_FAIL(MI355_EINVAL, "mixup_pairs: too large (B=%d img_plane=%ld hm_plane=%ld)", B, img_plane, hm_plane);
  if (((uintptr_t)x_s | (uintptr_t)x_t | (uintptr_t)hm_s | (uintptr_t)hm_t | (uintptr_t)w_s | (uintptr_t)w_t | (uintptr_t)lam |
       (uintptr_t)x_mix | (uintptr_t)hm_mix | (uintptr_t)w_mix) & 3)
    MI_FAIL(MI355_EINVAL, "mixup_pairs: pointers must be 4-byte aligned");
  const long nx = (long)B * img_plane, nh = (long)B * hm_plane, nw = (long)B * K;
  const void* in[7] = {x_s, x_t, hm_s, hm_t, w_s, w_t, lam};
  const long in_bytes[7] = {4 * nx, 4 * nx, 4 * nh, 4 * nh, 4 * nw, 4 * nw, 4L * B};
  const void* out[3] = {x_mix, hm_mix, w_mix};
  const long out_bytes[3] = {8 * nx, 8 * nh, 8 * nw};
  static const char* const in_name[7] = {"x_s", "x_t", "hm_s", "hm_t", "w_s", "w_t", "lam"};
  static const char* const out_name[3] = {"x_mix", "hm_mix", "w_mix"};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 7; ++i)
      if (mix_overlap(out[o], out_bytes[o], in[i], in_bytes[i]))
        MI_FAIL(MI355_EINVAL, "mixup_pairs: %s and %s overlap", out_name[o], in_name[i]);
    for (int p = o + 1; p < 3; ++p)
      if (mix_overlap(out[o], out_bytes[o], out[p], out_bytes[p]))
        MI_FAIL(MI355_EINVAL, "mixup_pairs: %s and %s overlap", out_name[o], out_name[p]);
  }
  const MixRange img = mix_make_range(x_s, x_t, x_mix, nx, img_plane), hm = mix_make_range(hm_s, hm_t, hm_mix, nh, hm_plane);
  const long most = nx > nh ? nx : nh;
  long grid = ((img.vec && hm.vec ? most / 4 : most) + 255) / 256;
  if (grid < 1) grid = 1;
  if (grid > MI355_MIXUP_MAX_BLOCKS) grid = MI355_MIXUP_MAX_BLOCKS;
  char lab[96];
  snprintf(lab, sizeof(lab), "mixup B%d img%ld hm%ld K%d%s", B, img_plane, hm_plane, K, img.vec && hm.vec ? "" : " scalar");
  ProfScope ps(as_stream(stream), 0.0, 16.0 * (nx + nh + nw) + 4.0 * B, 2, lab);
  hipLaunchKernelGGL(mixup_pairs_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), img, hm, w_s, w_t, w_mix, nw, lam);
  MI_CHECK_LAUNCH("mixup_pairs");
  return MI355_OK;
}

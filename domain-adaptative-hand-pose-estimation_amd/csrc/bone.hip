// Bone-ratio skeleton prior (see mi355pose.h; not in the reference: in the family of the bone-length-ratio constraint of Zhou et
// al., ICCV 2017 -- PAPERS.md).  The bone lengths of a predicted hand, divided by their mean, are held to running statistics of
// the same ratios in the source annotations.  Two tiny kernels, fp64 arithmetic on fp32 operands, every sum in ascending bone /
// sample order, one rounding to fp32 at each store; the build's -ffp-contract=off keeps every product and sum rounded on its own.
#include "common.h"
#include <stdio.h>

// length of bone e of one sample and whether it is present; returns the number n of present bones, S = their summed length
__device__ __forceinline__ int bone_lengths(const float* __restrict__ uv, const float* __restrict__ w, const int* __restrict__ bones,
                                            const int* __restrict__ seen, int K, int E, double* l, double* dx, double* dy, unsigned& present,
                                            double& S) {
  int n = 0;
  S = 0.0; present = 0u;
  for (int e = 0; e < E; ++e) {
    const int p = bones[2 * e], c = bones[2 * e + 1];
    if ((unsigned)p >= (unsigned)K || (unsigned)c >= (unsigned)K) { l[e] = 0.0; if (dx) { dx[e] = 0.0; dy[e] = 0.0; } continue; }   // (a table entry outside the joints is no bone)
    const bool on = (!w || (w[p] > 0.f && w[c] > 0.f)) && (!seen || seen[e] != 0);
    const double x = (double)uv[2 * c] - (double)uv[2 * p], y = (double)uv[2 * c + 1] - (double)uv[2 * p + 1];
    const double len = sqrt(x * x + y * y);
    l[e] = len;
    if (dx) { dx[e] = x; dy[e] = y; }
    if (on) { present |= 1u << e; ++n; S += len; }
  }
  return n;
}

// one thread per sample: at most 32 bones of serial fp64 work, and the per-joint sums sit in the thread's own memory
__global__ __launch_bounds__(64) void bone_prior_kernel(const float* __restrict__ uv, const float* __restrict__ weight,
                                                         const int* __restrict__ bones, const float* __restrict__ mean,
                                                         const float* __restrict__ var, const int* __restrict__ seen, float margin,
                                                         float eps, float coef, float* __restrict__ loss_rows, float* __restrict__ g_uv,
                                                         int B, int K, int E) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float* p_uv = uv + (size_t)b * K * 2;
  const float* p_w = weight ? weight + (size_t)b * K : nullptr;
  float* g = g_uv ? g_uv + (size_t)b * K * 2 : nullptr;
  double l[MI355_BONE_MAX_BONES], dx[MI355_BONE_MAX_BONES], dy[MI355_BONE_MAX_BONES], q[MI355_BONE_MAX_BONES];
  double acc[2 * MI355_BONE_MAX_JOINTS];
  unsigned present; double S;
  const int n = bone_lengths(p_uv, p_w, bones, seen, K, E, l, dx, dy, present, S);
  for (int j = 0; j < 2 * K; ++j) acc[j] = 0.0;
  if (n < 2 || S == 0.0) {                                   // skipped by selection (a NaN sum is not 0: it goes on)
    loss_rows[b] = 0.f;
    if (g) for (int j = 0; j < 2 * K; ++j) g[j] = 0.f;
    return;
  }
  const double dn = (double)n, lbar = S / dn;
  double loss = 0.0, Qs = 0.0;
  for (int e = 0; e < E; ++e) {
    q[e] = 0.0;
    if (!(present >> e & 1u)) continue;
    const double r = l[e] / lbar;
    const double sd = sqrt((double)var[e] + (double)eps);
    const double z = (r - (double)mean[e]) / sd;
    const double a = fabs(z) - (double)margin;
    const double h = a > 0.0 ? a : (a == a ? 0.0 : a);       // max(a, 0) that keeps a NaN
    const double sg = z > 0.0 ? 1.0 : (z < 0.0 ? -1.0 : z);  // sign(z): 0 for +-0, NaN for NaN
    loss += 0.5 * (h * h);
    q[e] = h * sg / (dn * sd);
    Qs += q[e] * r;
  }
  loss_rows[b] = (float)(loss / dn);
  if (!g) return;
  const double Q = Qs / dn;
  for (int e = 0; e < E; ++e) {
    if (!(present >> e & 1u) || l[e] == 0.0) continue;       // a bone of length 0 has no direction: it contributes nothing
    const double k = (double)coef * ((q[e] - Q) / lbar) / l[e];
    const double tx = k * dx[e], ty = k * dy[e];
    const int p = bones[2 * e], c = bones[2 * e + 1];
    acc[2 * c] += tx; acc[2 * c + 1] += ty;
    acc[2 * p] -= tx; acc[2 * p + 1] -= ty;
  }
  for (int j = 0; j < 2 * K; ++j) g[j] = (float)acc[j];
}

// One workgroup.  Pass 1: thread b (strided) leaves lbar of sample b in LDS, -1 for a skipped sample.  Pass 2: thread e owns bone
// e and walks the samples in ascending order twice (mean, then the biased variance about it).
__global__ __launch_bounds__(256) void bone_stats_kernel(const float* __restrict__ kp, const float* __restrict__ weight,
                                                          const int* __restrict__ bones, float* __restrict__ mean, float* __restrict__ var,
                                                          int* __restrict__ seen, float rho, int B, int K, int E) {
  extern __shared__ double lbar_s[];
  for (int b = threadIdx.x; b < B; b += 256) {
    double l[MI355_BONE_MAX_BONES];
    unsigned present; double S;
    const int n = bone_lengths(kp + (size_t)b * K * 2, weight ? weight + (size_t)b * K : nullptr, bones, nullptr, K, E, l, nullptr, nullptr,
                               present, S);
    lbar_s[b] = (n < 2 || S == 0.0) ? -1.0 : S / (double)n;
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e >= E) return;
  const int p = bones[2 * e], c = bones[2 * e + 1];
  if ((unsigned)p >= (unsigned)K || (unsigned)c >= (unsigned)K) return;
  double m = 0.0, v = 0.0;
  int cnt = 0;
  for (int pass = 0; pass < 2; ++pass) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      const double lb = lbar_s[b];
      if (lb < 0.0) continue;
      const float* u = kp + (size_t)b * K * 2;
      if (weight && !(weight[(size_t)b * K + p] > 0.f && weight[(size_t)b * K + c] > 0.f)) continue;
      const double x = (double)u[2 * c] - (double)u[2 * p], y = (double)u[2 * c + 1] - (double)u[2 * p + 1];
      const double r = sqrt(x * x + y * y) / lb;
      if (pass == 0) { s += r; ++cnt; } else { s += (r - m) * (r - m); }
    }
    if (cnt == 0) return;                                    // no sample shows this bone: not touched
    if (pass == 0) m = s / (double)cnt; else v = s / (double)cnt;
  }
  if (seen[e] == 0) {
    mean[e] = (float)m; var[e] = (float)v; seen[e] = 1;
  } else {
    const double k = (double)rho;
    mean[e] = (float)((1.0 - k) * (double)mean[e] + k * m);
    var[e] = (float)((1.0 - k) * (double)var[e] + k * v);
  }
}

static int bone_shape_check(const char* who, const void* bones, int B, int K, int E) {
  if (!bones) MI_FAIL(MI355_EINVAL, "%s: null bone table", who);
  if (B < 1 || B > MI355_BONE_MAX_BATCH) MI_FAIL(MI355_EINVAL, "%s: bad batch (B=%d, at most %d)", who, B, MI355_BONE_MAX_BATCH);
  if (K < 2 || K > MI355_BONE_MAX_JOINTS) MI_FAIL(MI355_EINVAL, "%s: bad joint count (K=%d, 2..%d)", who, K, MI355_BONE_MAX_JOINTS);
  if (E < 1 || E > MI355_BONE_MAX_BONES) MI_FAIL(MI355_EINVAL, "%s: bad bone count (E=%d, 1..%d)", who, E, MI355_BONE_MAX_BONES);
  return MI355_OK;
}

extern "C" int mi355_bone_prior(const float* uv, const float* weight, const int* bones, const float* mean, const float* var, const int* seen,
                                float margin, float eps, float coef, float* loss_rows, float* g_uv, int B, int K, int E, void* stream) {
  if (!uv || !mean || !var || !seen || !loss_rows) MI_FAIL(MI355_EINVAL, "bone_prior: null uv, mean, var, seen or loss_rows");
  if (int rc = bone_shape_check("bone_prior", bones, B, K, E)) return rc;
  if (!__builtin_isfinite(margin) || margin < 0.f) MI_FAIL(MI355_EINVAL, "bone_prior: margin must be finite and not negative, got %g", (double)margin);
  if (!__builtin_isfinite(eps) || !(eps > 0.f)) MI_FAIL(MI355_EINVAL, "bone_prior: eps must be finite and positive, got %g", (double)eps);
  if (!__builtin_isfinite(coef)) MI_FAIL(MI355_EINVAL, "bone_prior: coef must be finite, got %g", (double)coef);
  char lab[64];
  if (prof_on()) snprintf(lab, sizeof(lab), "bone_prior B%d K%d E%d%s", B, K, E, g_uv ? " +grad" : "");
  ProfScope ps(as_stream(stream), 0.0, (g_uv ? 16.0 : 8.0) * B * K + 4.0 * B, 2, prof_on() ? lab : nullptr);
  hipLaunchKernelGGL(bone_prior_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), uv, weight, bones, mean, var, seen, margin, eps,
                     coef, loss_rows, g_uv, B, K, E);
  MI_CHECK_LAUNCH("bone_prior");
  return MI355_OK;
}

extern "C" int mi355_bone_stats_update(const float* kp, const float* weight, const int* bones, float* mean, float* var, int* seen, float rho,
                                       int B, int K, int E, void* stream) {
  if (!kp || !mean || !var || !seen) MI_FAIL(MI355_EINVAL, "bone_stats_update: null kp, mean, var or seen");
  if (int rc = bone_shape_check("bone_stats_update", bones, B, K, E)) return rc;
  if (!(rho >= 0.f && rho <= 1.f)) MI_FAIL(MI355_EINVAL, "bone_stats_update: rho must lie in [0, 1], got %g", (double)rho);
  char lab[64];
  if (prof_on()) snprintf(lab, sizeof(lab), "bone_stats_update B%d K%d E%d", B, K, E);
  ProfScope ps(as_stream(stream), 0.0, 12.0 * B * K + 24.0 * E, 2, prof_on() ? lab : nullptr);
  hipLaunchKernelGGL(bone_stats_kernel, dim3(1), dim3(256), sizeof(double) * (size_t)B, as_stream(stream), kp, weight, bones, mean, var,
                     seen, rho, B, K, E);
  MI_CHECK_LAUNCH("bone_stats_update");
  return MI355_OK;
}

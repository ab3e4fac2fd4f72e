// Rendered hands: a batch of S x S images drawn from one 480-byte record per sample -- 20 bone capsules, one optional occluder
// capsule, a gradient + value-noise background, Lambert shading, sensor noise, photometric gain / bias -- with the "geometry-only"
// teacher image and the per-pixel primitive ids from the same launch.  The arithmetic is stated in include/mi355pose.h and restated
// in numpy by tests/render_ref.py: fp32, + - * / sqrt only, every operation rounded on its own whatever the build's flags say.
#include "common.h"
#include <cmath>

static_assert(sizeof(mi355_hand_rec) == 480 && sizeof(mi355_hand_rec) % 16 == 0, "mi355_hand_rec is 120 words");

constexpr int RH_TILE = 32;                   // a workgroup draws a 32 x 32 tile: 256 threads, 4 adjacent pixels each
constexpr int RH_PRIMS = 21;                  // 20 bones and the occluder
constexpr int RH_PW = 12;                     // words per staged primitive: ax ay az ex ey ez ee r r2 index (2 spare)
constexpr float RH_CULL_MARGIN = 4.0f;        // pixels.  With every coordinate and radius <= 2^20 in magnitude the rounding of the
                                              // coverage test moves a capsule's edge by less than a pixel (one ulp of 2^21 is
                                              // 0.25) and the rounding of the box below by as much: 4 keeps the culling conservative.

__device__ __forceinline__ float rh_hash01(uint32_t s, uint32_t a, uint32_t b) {
  uint32_t h = s ^ (a * 0x9E3779B1u);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= b * 0xC2B2AE35u;
  h ^= h >> 13;
  h *= 0x27D4EB2Fu;
  h ^= h >> 16;
  return (float)(h >> 8) * 5.9604644775390625e-08f;       // 2^-24: exact
}
__device__ __forceinline__ float rh_clamp01(float q) { return q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q); }   // a NaN stays a NaN
__device__ __forceinline__ bool rh_bounded(float v) { return fabsf(v) <= MI355_RENDER_MAX_COORD; }         // false for NaN, inf

struct RhHit { float depth, wx, wy, d2; int slot; };

// The front-most staged primitive at (px, py): slot -1 when nothing covers it.  The list is in ascending primitive order and the
// comparison is strict, so the lower index wins a tie.
__device__ __forceinline__ RhHit rh_trace(const float (*prim)[RH_PW], int n, float px, float py) {
#pragma clang fp contract(off)
  RhHit h;
  h.depth = INFINITY; h.slot = -1; h.wx = h.wy = h.d2 = 0.0f;
  for (int s = 0; s < n; ++s) {
    const float* P = prim[s];
    const float ax = P[0], ay = P[1], az = P[2], ex = P[3], ey = P[4], ez = P[5], ee = P[6], r2 = P[8];
    const float dx = px - ax, dy = py - ay;
    const float de = dx * ex + dy * ey;
    const float q = ee > 0.0f ? de / ee : 0.0f;
    const float t = rh_clamp01(q);
    const float cx = ax + t * ex, cy = ay + t * ey;
    const float wx = px - cx, wy = py - cy;
    const float d2 = wx * wx + wy * wy;
    if (d2 <= r2) {
      const float depth = (az + t * ez) - sqrtf(r2 - d2);
      if (depth < h.depth) { h.depth = depth; h.slot = s; h.wx = wx; h.wy = wy; h.d2 = d2; }
    }
  }
  return h;
}

// Colour of one sub-sample, added to acc[3] (the caller adds the four in the stated order).
__device__ __forceinline__ void rh_shade(const float (*prim)[RH_PW], int n, const mi355_hand_rec* R, bool noisy, float px, float py,
                                         float* acc, bool first) {
#pragma clang fp contract(off)
  const RhHit h = rh_trace(prim, n, px, py);
  float col[3];
  if (h.slot >= 0) {
    const float* P = prim[h.slot];
    const float r = P[7], r2 = P[8];
    const bool occ = __float_as_int(P[9]) == RH_PRIMS - 1;
    const float nx = h.wx / r, ny = h.wy / r, nz = sqrtf(1.0f - h.d2 / r2);
    const float dot = nx * R->light[0] + ny * R->light[1] + nz * R->light[2];
    const float lam = dot > 0.0f ? dot : 0.0f;
    const float shade = R->ambient + (1.0f - R->ambient) * lam;
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = (occ ? R->occ_col[c] : R->skin[c]) * shade;
  } else {
    const float g = rh_clamp01((px * R->grad[0] + py * R->grad[1]) + R->grad_off);
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = R->bg0[c] + g * (R->bg1[c] - R->bg0[c]);
    if (noisy) {                                            // inv_cell in (0, 1], px, py in [-0.25, 512.25]: u, v in [0, 514)
      const float u = (px + 1.0f) * R->noise_inv_cell, v = (py + 1.0f) * R->noise_inv_cell;
      const float fu = floorf(u), fv = floorf(v);
      const uint32_t ix = (uint32_t)(int)fu, iy = (uint32_t)(int)fv, sd = R->noise_seed;
      const float fx = u - fu, fy = v - fv;
      const float sx = (fx * fx) * (3.0f - 2.0f * fx), sy = (fy * fy) * (3.0f - 2.0f * fy);
      const float l00 = rh_hash01(sd, ix, iy), l10 = rh_hash01(sd, ix + 1u, iy);
      const float l01 = rh_hash01(sd, ix, iy + 1u), l11 = rh_hash01(sd, ix + 1u, iy + 1u);
      const float top = l00 + sx * (l10 - l00), bot = l01 + sx * (l11 - l01);
      const float val = top + sy * (bot - top);
      const float add = R->noise_amp * (val - 0.5f);
#pragma unroll
      for (int c = 0; c < 3; ++c) col[c] = col[c] + add;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] = first ? col[c] : acc[c] + col[c];
}

struct RhNorm { float mean[3], inv_std[3]; };

__global__ __launch_bounds__(256) void render_hands_kernel(const mi355_hand_rec* __restrict__ recs, float* __restrict__ out,
                                                            float* __restrict__ out_ema, unsigned char* __restrict__ ids, int S,
                                                            int tiles_x, RhNorm norm) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint32_t s_words[sizeof(mi355_hand_rec) / 4];
  __shared__ float s_prim[RH_PRIMS][RH_PW];
  __shared__ int s_n;
  const int tiles = tiles_x * tiles_x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int tid = threadIdx.x;
  if (tid < (int)(sizeof(mi355_hand_rec) / 4)) s_words[tid] = reinterpret_cast<const uint32_t*>(recs + b)[tid];
  __syncthreads();
  const mi355_hand_rec* R = reinterpret_cast<const mi355_hand_rec*>(s_words);
  const int X0 = tx * RH_TILE, Y0 = ty * RH_TILE;
  if (tid < 64) {                                            // the first wave: lane k builds, tests and files primitive k
    bool keep = false;
    float ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0, r = 0;
    if (tid < RH_PRIMS) {
      if (tid < RH_PRIMS - 1) {
        const int ja = (tid & 3) == 0 ? 0 : tid, jb = tid + 1;
        ax = R->jx[ja]; ay = R->jy[ja]; az = R->jz[ja]; bx = R->jx[jb]; by = R->jy[jb]; bz = R->jz[jb]; r = R->radius[tid];
      } else {
        ax = R->occ_a[0]; ay = R->occ_a[1]; bx = R->occ_b[0]; by = R->occ_b[1]; az = bz = R->occ_z; r = R->occ_r;
      }
      const bool valid = rh_bounded(ax) && rh_bounded(ay) && rh_bounded(az) && rh_bounded(bx) && rh_bounded(by) && rh_bounded(bz) &&
                         rh_bounded(r) && r > 0.0f;
      // float comparisons only: the tile's sub-samples and pixel centres lie in [X0 - 0.25, X0 + 31.25] x [Y0 - 0.25, Y0 + 31.25]
      const float xlo = (float)X0 - 0.25f - RH_CULL_MARGIN, xhi = (float)(X0 + RH_TILE - 1) + 0.25f + RH_CULL_MARGIN;
      const float ylo = (float)Y0 - 0.25f - RH_CULL_MARGIN, yhi = (float)(Y0 + RH_TILE - 1) + 0.25f + RH_CULL_MARGIN;
      keep = valid && fminf(ax, bx) - r <= xhi && fmaxf(ax, bx) + r >= xlo && fminf(ay, by) - r <= yhi && fmaxf(ay, by) + r >= ylo;
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int slot = __popcll(mask & ((1ull << tid) - 1ull));
      float* P = s_prim[slot];
      const float ex = bx - ax, ey = by - ay;
      P[0] = ax; P[1] = ay; P[2] = az; P[3] = ex; P[4] = ey; P[5] = bz - az; P[6] = ex * ex + ey * ey; P[7] = r; P[8] = r * r;
      P[9] = __int_as_float(tid);
    }
    if (tid == 0) s_n = __popcll(mask);
  }
  __syncthreads();
  const int n = s_n;
  const int i = Y0 + (tid >> 3), j0 = X0 + (tid & 7) * 4;
  if (i >= S || j0 >= S) return;                             // (S % 16 == 0: a quad is inside the row or outside it)
  const bool noisy = R->noise_amp > 0.0f && R->noise_inv_cell > 0.0f && R->noise_inv_cell <= 1.0f;
  const bool sensor = R->sensor_sigma > 0.0f;
  float m[4][3];
  unsigned char id[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float fj = (float)(j0 + q), fi = (float)i;
    float acc[3];
    rh_shade(s_prim, n, R, noisy, fj - 0.25f, fi - 0.25f, acc, true);
    rh_shade(s_prim, n, R, noisy, fj + 0.25f, fi - 0.25f, acc, false);
    rh_shade(s_prim, n, R, noisy, fj - 0.25f, fi + 0.25f, acc, false);
    rh_shade(s_prim, n, R, noisy, fj + 0.25f, fi + 0.25f, acc, false);
#pragma unroll
    for (int c = 0; c < 3; ++c) m[q][c] = 0.25f * acc[c];
    if (ids) {
      const RhHit h = rh_trace(s_prim, n, fj, fi);
      id[q] = h.slot >= 0 ? (unsigned char)(__float_as_int(s_prim[h.slot][9]) + 1) : (unsigned char)0;
    }
  }
  const long plane = (long)S * S, at = (long)i * S + j0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float mean = norm.mean[c], inv_std = norm.inv_std[c], gain = R->gain[c], bias = R->bias[c];
    float v[4], e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      e[q] = (m[q][c] - mean) * inv_std;
      float w = m[q][c] * gain + bias;
      if (sensor) {
        const uint32_t sd = R->sensor_seed ^ ((uint32_t)(4 * c + 1) * 0x632BE5ABu);
        const uint32_t ui = (uint32_t)i, uj = (uint32_t)(j0 + q);
        float u = rh_hash01(sd, ui, uj);
        u = u + rh_hash01(R->sensor_seed ^ ((uint32_t)(4 * c + 2) * 0x632BE5ABu), ui, uj);
        u = u + rh_hash01(R->sensor_seed ^ ((uint32_t)(4 * c + 3) * 0x632BE5ABu), ui, uj);
        u = u + rh_hash01(R->sensor_seed ^ ((uint32_t)(4 * c + 4) * 0x632BE5ABu), ui, uj);
        w = w + R->sensor_sigma * (u - 2.0f);
      }
      v[q] = (w - mean) * inv_std;
    }
    const long o = ((long)b * 3 + c) * plane + at;
    *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
    if (out_ema) *reinterpret_cast<float4*>(out_ema + o) = make_float4(e[0], e[1], e[2], e[3]);
  }
  if (ids) *reinterpret_cast<uchar4*>(ids + (long)b * plane + at) = make_uchar4(id[0], id[1], id[2], id[3]);
}

static bool render_overlap(const void* p, long np, const void* q, long nq) {   // [p, p + np) and [q, q + nq), in bytes
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

extern "C" size_t mi355_hand_rec_size(void) { return sizeof(mi355_hand_rec); }

extern "C" int mi355_render_hands(const mi355_hand_rec* recs, float* out, float* out_ema, unsigned char* ids, int B, int S,
                                  const float* mean3, const float* inv_std3, void* stream) {
  if (!recs) MI_FAIL(MI355_EINVAL, "render_hands: recs is null");
  if (!out) MI_FAIL(MI355_EINVAL, "render_hands: out is null");
  if (!mean3 || !inv_std3) MI_FAIL(MI355_EINVAL, "render_hands: mean3 / inv_std3 is null (mean3 %p, inv_std3 %p)", (const void*)mean3, (const void*)inv_std3);
  if (B < 1) MI_FAIL(MI355_EINVAL, "render_hands: B=%d (at least 1)", B);
  if (S < 16 || S > MI355_RENDER_MAX_SIDE || S % 16 != 0) MI_FAIL(MI355_EINVAL, "render_hands: S=%d is not a multiple of 16 from 16 to %d", S, MI355_RENDER_MAX_SIDE);
  if ((uintptr_t)recs & 15) MI_FAIL(MI355_EINVAL, "render_hands: recs must be 16-byte aligned");
  if ((uintptr_t)out & 15) MI_FAIL(MI355_EINVAL, "render_hands: out must be 16-byte aligned");
  if ((uintptr_t)out_ema & 15) MI_FAIL(MI355_EINVAL, "render_hands: out_ema must be 16-byte aligned");
  if ((uintptr_t)ids & 3) MI_FAIL(MI355_EINVAL, "render_hands: ids must be 4-byte aligned");
  const int tiles_x = cdiv(S, RH_TILE);
  const long tiles = (long)tiles_x * tiles_x;
  if ((long)B > 0x7fffffffL / tiles) MI_FAIL(MI355_EINVAL, "render_hands: too large (B=%d S=%d: the blocks are beyond the grid)", B, S);
  const long px = (long)B * S * S, nrec = (long)sizeof(mi355_hand_rec) * B;
  const struct { const char* name; const void* p; long bytes; } bufs[4] = {
      {"recs", recs, nrec}, {"out", out, 12 * px}, {"out_ema", out_ema, 12 * px}, {"ids", ids, px}};
  for (int u = 0; u < 4; ++u)
    for (int v = u + 1; v < 4; ++v)
      if (bufs[u].p && bufs[v].p && render_overlap(bufs[u].p, bufs[u].bytes, bufs[v].p, bufs[v].bytes))
        MI_FAIL(MI355_EINVAL, "render_hands: %s and %s overlap", bufs[u].name, bufs[v].name);
  RhNorm norm;
  for (int c = 0; c < 3; ++c) { norm.mean[c] = mean3[c]; norm.inv_std[c] = inv_std3[c]; }
  char lab[96];
  snprintf(lab, sizeof(lab), "render_hands %dx3x%dx%d%s%s", B, S, S, out_ema ? " +ema" : "", ids ? " +ids" : "");
  ProfScope ps(as_stream(stream), 0.0, (out_ema ? 24.0 : 12.0) * px + (ids ? 1.0 : 0.0) * px + (double)nrec, 2, lab);
  hipLaunchKernelGGL(render_hands_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, as_stream(stream), recs, out, out_ema, ids, S,
                     tiles_x, norm);
  MI_CHECK_LAUNCH("render_hands");
  return MI355_OK;
}

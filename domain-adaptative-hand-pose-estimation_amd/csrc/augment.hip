// Training augmentation on the device (include/mi355pose.h, "training augmentation"): the reference's per-sample Pillow
// chain -- rotate, resized crop, colour jitter, Gaussian blur, to_tensor + Normalize, and the image_ema copy -- for a batch
// of ragged uint8 RGB sources, in Pillow's own integer / float32 / float64 arithmetic so that the result is bit-identical.
//
// Launch 1 (aug_geometry): one block per band of BAND output rows of one image.  The rotated pixel is computed on the fly
// from the fixed-point closed form (no rotated image is stored); the horizontal BILINEAR pass writes the band's rows of
// the uint8 intermediate to LDS, the vertical pass reads them.  Writes the uint8 geometry image to the workspace, the
// optional normalised image_ema, and the integer luminance sum of the image as it stands right before contrast.
// mi355_resize_normalize is this launch alone, instantiated without the uint8 image and the luminance sum (FULL = false):
// the normalised geometry image is its output.
// Launch 2 (aug_photometric): one block per tile of TILE output rows with a 3-row halo: jitter recomputed pointwise,
// the 3 + 3 box-blur passes in LDS (ping-pong, edge clamp), then the normalisation to fp32 NCHW.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;           // threads per block
constexpr int BAND = 8;           // output rows per geometry block
constexpr int KMAX = 9;           // BILINEAR taps for crop side <= 4 * S (support 4)
constexpr int TMAX = 9 * 4 + 5;   // intermediate rows per band: <= (BAND - 1) * scale + 2 * support + 2 at scale 4
constexpr int TILE = 16;          // output rows per photometric block
constexpr int HALO = 3;           // one row per vertical box pass
constexpr int SMAX = 512;          // dynamic LDS at SMAX: 85 504 B (geometry), 67 584 B (photometric); the cap is raised on demand
constexpr int PREC = 22;          // Resample.c PRECISION_BITS for 8-bit images

struct Norm { float mean[3], stdv[3]; };

__device__ inline void rot_pixel(const uint8_t* __restrict__ img, const mi355_aug_rec& r, int y, int x, int (&px)[3]) {
  // pixel (y, x) of Image.rotate's result (same canvas, fill 0); (y, x) lies inside the h x w canvas
  int ys, xs;
  switch (r.rot) {
    case 1: ys = y; xs = x; break;
    case 2: ys = r.h - 1 - y; xs = r.w - 1 - x; break;
    case 3: ys = x; xs = r.w - 1 - y; break;                  // Transpose.ROTATE_90 (square)
    case 4: ys = r.h - 1 - x; xs = y; break;                  // Transpose.ROTATE_270 (square)
    default: {
      const int xx = r.a[2] + y * r.a[1] + x * r.a[0];        // int32, checked on the host not to overflow
      const int yy = r.a[5] + y * r.a[4] + x * r.a[3];
      xs = xx >> 16; ys = yy >> 16;                           // arithmetic shift: floor
      if (xs < 0 || xs >= r.w || ys < 0 || ys >= r.h) { px[0] = px[1] = px[2] = 0; return; }
    }
  }
  const uint8_t* p = img + (ys * r.w + xs) * 3;
  px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
}

__device__ inline int luminance(const int (&px)[3]) {
  return (19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 0x8000) >> 16;
}

// Blend.c: in1 + alpha * (in2 - in1) in float32; truncated inside [0, 1], clipped outside
__device__ inline int blend(int deg, int v, float alpha) {
  const float t = (float)deg + alpha * (float)(v - deg);
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (int)t;
}

__device__ inline void apply_op(int op, float f, int mean, int (&px)[3]) {
  int deg[3];
  if (op == 0) { deg[0] = deg[1] = deg[2] = 0; }
  else if (op == 1) { deg[0] = deg[1] = deg[2] = mean; }
  else { const int l = luminance(px); deg[0] = deg[1] = deg[2] = l; }
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = blend(deg[c], px[c], f);
}

__device__ inline int clip8(int v) {       // Resample.c clip8 on a 22-bit fixed-point sum
  if (v >= (1 << PREC << 8)) return 255;
  if (v <= 0) return 0;
  return v >> PREC;
}

// Resample.c precompute_coeffs / normalize_coeffs_8bpc for one output index of a side -> S BILINEAR resize
__device__ inline void bilinear_coeffs(int side, int S, int i, int* xmin_out, int* n_out, int* k_out) {
  const double scale = (double)side / S;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = (i + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > side) xmax = side;
  xmax -= xmin;
  if (xmax > KMAX) xmax = KMAX;             // (cannot happen for side <= 4 S; keeps the LDS table in bounds)
  double w[KMAX], ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = (x + xmin - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    w[x] = t < 1.0 ? 1.0 - t : 0.0;
    ww += w[x];
  }
  for (int x = 0; x < xmax; ++x) {
    double v = w[x];
    if (ww != 0.0) v /= ww;
    k_out[x] = v < 0 ? (int)(-0.5 + v * (1 << PREC)) : (int)(0.5 + v * (1 << PREC));
  }
  *xmin_out = xmin; *n_out = xmax;
}

// FULL: the first launch of mi355_augment.  !FULL: mi355_resize_normalize -- `ema` is the output, geo / lsum are not touched
template <bool FULL>
__global__ __launch_bounds__(NT) void aug_geometry(const uint8_t* __restrict__ src, const mi355_aug_rec* __restrict__ recs,
                                                   int S, uint8_t* __restrict__ geo, float* __restrict__ ema, Norm nm,
                                                   unsigned long long* __restrict__ lsum) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* kx = reinterpret_cast<int*>(smem);            // [S] first tap
  int* kn = kx + S;                                  // [S] taps
  int* kk = kn + S;                                  // [S][KMAX] coefficients
  uint8_t* tmp = reinterpret_cast<uint8_t*>(kk + S * KMAX);   // [TMAX][S][3] horizontal pass of this band
  __shared__ unsigned long long red;

  const int b = blockIdx.y, y0 = blockIdx.x * BAND, tid = threadIdx.x;
  const mi355_aug_rec r = recs[b];
  const uint8_t* img = src + r.offset;
  const bool resize = r.side != S;
  if (FULL && tid == 0) red = 0;

  int rmin = 0, nrows = BAND;
  if (resize) {
    for (int i = tid; i < S; i += NT) bilinear_coeffs(r.side, S, i, &kx[i], &kn[i], &kk[i * KMAX]);
    __syncthreads();
    rmin = kx[y0];
    nrows = kx[y0 + BAND - 1] + kn[y0 + BAND - 1] - rmin;
    if (nrows > TMAX) return;                        // uniform; cannot happen for side <= 4 S (host check)
    for (int e = tid; e < nrows * S; e += NT) {      // horizontal pass: rows rmin.. of the crop, all S columns
      const int row = e / S, xx = e - row * S;
      int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
      const int x0 = kx[xx], n = kn[xx];
      for (int k = 0; k < n; ++k) {
        int px[3];
        rot_pixel(img, r, r.top + rmin + row, r.left + x0 + k, px);
        const int c = kk[xx * KMAX + k];
        acc[0] += px[0] * c; acc[1] += px[1] * c; acc[2] += px[2] * c;
      }
      uint8_t* t = tmp + (row * S + xx) * 3;
      t[0] = (uint8_t)clip8(acc[0]); t[1] = (uint8_t)clip8(acc[1]); t[2] = (uint8_t)clip8(acc[2]);
    }
  } else {
    for (int e = tid; e < BAND * S; e += NT) {       // crop only (Image.resize is skipped at the target size)
      const int row = e / S, xx = e - row * S;
      int px[3];
      rot_pixel(img, r, r.top + y0 + row, r.left + xx, px);
      uint8_t* t = tmp + (row * S + xx) * 3;
      t[0] = (uint8_t)px[0]; t[1] = (uint8_t)px[1]; t[2] = (uint8_t)px[2];
    }
  }
  __syncthreads();

  bool contrast = false;
  if (FULL)
    for (int j = 0; j < 3; ++j) contrast |= r.order[j] == 1;
  unsigned lum = 0;
  const size_t plane = (size_t)S * S;
  for (int e = tid; e < BAND * S; e += NT) {         // vertical pass, outputs, pre-contrast jitter
    const int row = e / S, xx = e - row * S, yy = y0 + row;
    int px[3];
    if (resize) {
      int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
      const int t0 = kx[yy] - rmin, n = kn[yy];
      for (int k = 0; k < n; ++k) {
        const uint8_t* t = tmp + ((t0 + k) * S + xx) * 3;
        const int c = kk[yy * KMAX + k];
        acc[0] += t[0] * c; acc[1] += t[1] * c; acc[2] += t[2] * c;
      }
      px[0] = clip8(acc[0]); px[1] = clip8(acc[1]); px[2] = clip8(acc[2]);
    } else {
      const uint8_t* t = tmp + (row * S + xx) * 3;
      px[0] = t[0]; px[1] = t[1]; px[2] = t[2];
    }
    const size_t pix = (size_t)yy * S + xx;
    if (FULL) {
      uint8_t* g = geo + ((size_t)b * plane + pix) * 3;
      g[0] = (uint8_t)px[0]; g[1] = (uint8_t)px[1]; g[2] = (uint8_t)px[2];
    }
    if (ema) {
      float* o = ema + (size_t)b * 3 * plane + pix;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = ((float)px[c] / 255.0f - nm.mean[c]) / nm.stdv[c];
    }
    if (contrast) {
      for (int j = 0; j < 3 && r.order[j] != 1; ++j)
        if (r.order[j] >= 0) apply_op(r.order[j], r.factor[r.order[j]], 0, px);
      lum += (unsigned)luminance(px);
    }
  }
  if (contrast) {                                    // exact integer sum: order-independent, deterministic
    for (int o = WAVE / 2; o > 0; o >>= 1) lum += __shfl_down(lum, o, WAVE);
    if ((tid & (WAVE - 1)) == 0) atomicAdd(&red, (unsigned long long)lum);
    __syncthreads();
    if (tid == 0) atomicAdd(&lsum[b], red);
  }
}

__global__ __launch_bounds__(NT) void aug_photometric(const uint8_t* __restrict__ geo, const mi355_aug_rec* __restrict__ recs,
                                                      int S, const unsigned long long* __restrict__ lsum, Norm nm,
                                                      float* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int rows = TILE + 2 * HALO;
  uint8_t* buf[2] = {smem, smem + rows * S * 3};     // [rows][S][3] each; LDS row j holds image row y0 - HALO + j

  const int b = blockIdx.y, y0 = blockIdx.x * TILE, tid = threadIdx.x;
  const mi355_aug_rec r = recs[b];
  const size_t plane = (size_t)S * S;
  // ImageStat: mean = sum / count in double, ImageEnhance.Contrast: int(mean + 0.5)
  const int mean = (int)((double)lsum[b] / (double)plane + 0.5);
  const int lo = max(0, y0 - HALO), hi = min(S, y0 + TILE + HALO);
  auto at = [&](int k, int y, int x) { return buf[k] + ((y - (y0 - HALO)) * S + x) * 3; };

  for (int e = tid; e < (hi - lo) * S; e += NT) {    // jitter, every op in the drawn order
    const int y = lo + e / S, x = e % S;
    const uint8_t* g = geo + ((size_t)b * plane + (size_t)y * S + x) * 3;
    int px[3] = {g[0], g[1], g[2]};
    for (int j = 0; j < 3; ++j)
      if (r.order[j] >= 0) apply_op(r.order[j], r.factor[r.order[j]], mean, px);
    uint8_t* d = at(0, y, x);
    d[0] = (uint8_t)px[0]; d[1] = (uint8_t)px[1]; d[2] = (uint8_t)px[2];
  }
  int cur = 0;
  if (r.blur) {
    const unsigned ww = r.ww, fw = r.fw;
    auto box = [&](const uint8_t* c, const uint8_t* m, const uint8_t* p, uint8_t* d) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const unsigned bulk = (unsigned)c[ch] * ww + ((unsigned)m[ch] + (unsigned)p[ch]) * fw;
        d[ch] = (uint8_t)((bulk + (1u << 23)) >> 24);
      }
    };
    for (int pass = 0; pass < 3; ++pass) {           // horizontal passes over every row held
      __syncthreads();
      for (int e = tid; e < (hi - lo) * S; e += NT) {
        const int y = lo + e / S, x = e % S;
        box(at(cur, y, x), at(cur, y, max(x - 1, 0)), at(cur, y, min(x + 1, S - 1)), at(cur ^ 1, y, x));
      }
      cur ^= 1;
    }
    for (int pass = 1; pass <= 3; ++pass) {          // vertical passes: the valid rows shrink by one per pass
      __syncthreads();
      const int plo = max(0, y0 - HALO + pass), phi = min(S, y0 + TILE + HALO - pass);
      for (int e = tid; e < (phi - plo) * S; e += NT) {
        const int y = plo + e / S, x = e % S;
        box(at(cur, y, x), at(cur, max(y - 1, 0), x), at(cur, min(y + 1, S - 1), x), at(cur ^ 1, y, x));
      }
      cur ^= 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < TILE * S; e += NT) {         // to_tensor + Normalize, fp32 NCHW
    const int y = y0 + e / S, x = e % S;
    const uint8_t* s = at(cur, y, x);
    float* o = out + (size_t)b * 3 * plane + (size_t)y * S + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = ((float)s[c] / 255.0f - nm.mean[c]) / nm.stdv[c];
  }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t mi355_augment_workspace(int B, int S) {
  if (B < 1 || S < 1) return 0;
  return align256((size_t)B * sizeof(unsigned long long)) + (size_t)B * S * S * 3;
}

static int check_rec(const mi355_aug_rec& r, int i, int64_t src_bytes, int S) {
  if (r.h < 1 || r.w < 1 || r.h > 4096 || r.w > 4096)
    MI_FAIL(MI355_EINVAL, "augment: image %d: size %dx%d outside 1..4096", i, r.h, r.w);
  const int64_t bytes = (int64_t)r.h * r.w * 3;    // < 2^31: the kernels index inside an image with 32-bit ints
  if (r.offset < 0 || r.offset > src_bytes || bytes > src_bytes - r.offset)
    MI_FAIL(MI355_EINVAL, "augment: image %d: bytes [%lld, %lld) outside the packed buffer of %lld", i, (long long)r.offset,
            (long long)(r.offset + bytes), (long long)src_bytes);
  if (r.rot < 0 || r.rot > 4) MI_FAIL(MI355_EINVAL, "augment: image %d: rotation mode %d", i, r.rot);
  if ((r.rot == 3 || r.rot == 4) && r.h != r.w) MI_FAIL(MI355_EINVAL, "augment: image %d: 90 / 270 shortcut needs a square image", i);
  if (r.rot == 0) {
    // |a0|, |a1|, |a3|, |a4| <= 1.0 in 16.16 and |a2|, |a5| bounded: a2 + y*a1 + x*a0 stays inside int32
    for (int k : {0, 1, 3, 4})
      if (r.a[k] < -65536 || r.a[k] > 65536) MI_FAIL(MI355_EINVAL, "augment: image %d: a%d = %d is not a rotation coefficient", i, k, r.a[k]);
    for (int k : {2, 5})
      if (r.a[k] < -(1 << 29) || r.a[k] > (1 << 29)) MI_FAIL(MI355_EINVAL, "augment: image %d: offset a%d = %d out of range", i, k, r.a[k]);
  }
  if (r.side < 1 || r.top < 0 || r.left < 0 || r.top > r.h - r.side || r.left > r.w - r.side)
    MI_FAIL(MI355_EINVAL, "augment: image %d: crop (%d, %d, side %d) outside %dx%d", i, r.top, r.left, r.side, r.h, r.w);
  if (r.side > 4 * S) MI_FAIL(MI355_EINVAL, "augment: image %d: crop side %d > 4 x %d (BILINEAR taps)", i, r.side, S);
  int seen = 0;
  for (int j = 0; j < 3; ++j) {
    const int op = r.order[j];
    if (op < -1 || op > 2 || (op >= 0 && (seen >> op) & 1)) MI_FAIL(MI355_EINVAL, "augment: image %d: op order", i);
    if (op >= 0) {
      seen |= 1 << op;
      const float f = r.factor[op];
      if (!(f >= 0.0f && f <= 1e6f)) MI_FAIL(MI355_EINVAL, "augment: image %d: factor %g", i, (double)f);
    }
  }
  if (r.blur != 0 && r.blur != 1) MI_FAIL(MI355_EINVAL, "augment: image %d: blur %d", i, r.blur);
  if (r.blur && ((uint64_t)r.ww + 2ull * r.fw > (1ull << 24) || r.ww == 0))
    MI_FAIL(MI355_EINVAL, "augment: image %d: box weights %u, %u", i, r.ww, r.fw);
  return MI355_OK;
}

// argument checks shared by mi355_augment (ws_needed: its workspace) and mi355_resize_normalize, all before anything is enqueued
static int check_batch(const uint8_t* src, int64_t src_bytes, const mi355_aug_rec* rec_host, const mi355_aug_rec* rec_dev, int B, int S,
                       const float* norm, const float* out, bool ws_needed, const void* ws, size_t ws_bytes, Norm* nm) {
  if (B < 1 || B > 65535) MI_FAIL(MI355_EINVAL, "augment: batch %d outside 1..65535", B);
  if (S < TILE || S > SMAX || S % TILE) MI_FAIL(MI355_EINVAL, "augment: output side %d (multiple of %d, at most %d)", S, TILE, SMAX);
  if (!src || src_bytes < 3 || !rec_host || !rec_dev || !norm || !out || (ws_needed && !ws)) MI_FAIL(MI355_EINVAL, "augment: null argument");
  if ((size_t)B * 3 * S * S > (size_t)INT32_MAX) MI_FAIL(MI355_EINVAL, "augment: output exceeds the 32-bit index range");
  // names the two arguments the requirement follows from: a workspace sized for side 256 is refused at 512 by this message
  if (ws_needed && ws_bytes < mi355_augment_workspace(B, S))
    MI_FAIL(MI355_EWORKSPACE, "augment: workspace %zu < %zu for batch %d, output side %d", ws_bytes, mi355_augment_workspace(B, S), B, S);
  for (int c = 0; c < 3; ++c) {
    nm->mean[c] = norm[c]; nm->stdv[c] = norm[3 + c];
    if (!(nm->stdv[c] != 0.0f)) MI_FAIL(MI355_EINVAL, "augment: std[%d] = 0", c);
  }
  for (int i = 0; i < B; ++i) {
    const int rc = check_rec(rec_host[i], i, src_bytes, S);
    if (rc) return rc;
  }
  return MI355_OK;
}

// dynamic LDS above the 64 KB default (S > 384 geometry, S > 496 photometric): raise the kernel's cap, once per size reached.
// The caps the callers keep are per process and unguarded, like the attribute flags of igemm.hip / pgemm.hip: one GPU and one
// calling thread per process (train1.py starts one rank per GPU).
template <typename K>
static int raise_lds(K kern, size_t lds, size_t* cap, const char* what) {
  if (lds <= *cap) return MI355_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    MI_FAIL(MI355_ELAUNCH, "augment: cannot raise the dynamic LDS limit of the %s kernel to %zu bytes", what, lds);
  *cap = lds;
  return MI355_OK;
}
constexpr size_t LDS_DEFAULT = 64 * 1024;
static size_t geometry_lds(int S) { return (size_t)S * (2 + KMAX) * sizeof(int) + (size_t)TMAX * S * 3; }

extern "C" int mi355_augment(const uint8_t* src, int64_t src_bytes, const mi355_aug_rec* rec_host, const mi355_aug_rec* rec_dev,
                             int B, int S, const float* norm, float* out, float* ema, void* ws, size_t ws_bytes, void* stream) {
  Norm nm;
  int rc = check_batch(src, src_bytes, rec_host, rec_dev, B, S, norm, out, true, ws, ws_bytes, &nm);
  if (rc) return rc;
  const size_t lds_a = geometry_lds(S), lds_b = 2 * (size_t)(TILE + 2 * HALO) * S * 3;
  static size_t cap_a = LDS_DEFAULT, cap_b = LDS_DEFAULT;
  if ((rc = raise_lds(aug_geometry<true>, lds_a, &cap_a, "geometry")) || (rc = raise_lds(aug_photometric, lds_b, &cap_b, "photometric"))) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long* lsum = reinterpret_cast<unsigned long long*>(ws);
  uint8_t* geo = reinterpret_cast<uint8_t*>(ws) + align256((size_t)B * sizeof(unsigned long long));
  if (hipMemsetAsync(lsum, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess)
    MI_FAIL(MI355_ELAUNCH, "augment: memset failed");
  hipLaunchKernelGGL(aug_geometry<true>, dim3(S / BAND, B), dim3(NT), lds_a, st, src, rec_dev, S, geo, ema, nm, lsum);
  MI_CHECK_LAUNCH("augment geometry");
  hipLaunchKernelGGL(aug_photometric, dim3(S / TILE, B), dim3(NT), lds_b, st, geo, rec_dev, S, lsum, nm, out);
  MI_CHECK_LAUNCH("augment photometric");
  return MI355_OK;
}

extern "C" int mi355_resize_normalize(const uint8_t* src, int64_t src_bytes, const mi355_aug_rec* rec_host, const mi355_aug_rec* rec_dev,
                                      int B, int S, const float* norm, float* out, void* stream) {
  Norm nm;
  int rc = check_batch(src, src_bytes, rec_host, rec_dev, B, S, norm, out, false, nullptr, 0, &nm);
  if (rc) return rc;
  const size_t lds = geometry_lds(S);
  static size_t cap = LDS_DEFAULT;
  if ((rc = raise_lds(aug_geometry<false>, lds, &cap, "resize")) != MI355_OK) return rc;
  hipLaunchKernelGGL(aug_geometry<false>, dim3(S / BAND, B), dim3(NT), lds, as_stream(stream), src, rec_dev, S,
                     (uint8_t*)nullptr, out, nm, (unsigned long long*)nullptr);
  MI_CHECK_LAUNCH("resize_normalize");
  return MI355_OK;
}

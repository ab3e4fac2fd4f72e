// Host-side exerciser of the geometric-view entry points (mi355_affine_warp_images, mi355_affine_unwarp_heatmaps,
// mi355_mse_heatmap_w) for the CPU-box sanitizer job (tests/test_host_warp.py): built like fda_driver.cpp -- the HOST pass of every
// .hip file with -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers are fake,
// well-aligned addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code under
// test has run.  The job passes when no sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL,
// naming what is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static char* fp(size_t i, size_t off = 0) { return reinterpret_cast<char*>(static_cast<uintptr_t>(0x100000000ull + (i << 44))) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

struct Warp { char *x, *recs, *out; int B, C, H, W; };
static Warp warp_ok(int B = 2, int C = 3, int H = 16, int W = 20, size_t in_off = 0, size_t out_off = 0) {
  return Warp{fp(1, in_off), fp(2, in_off), fp(3, out_off), B, C, H, W};
}
static int run(const Warp& a) {
  return mi355_affine_warp_images((const float*)a.x, (const mi355_view_rec*)a.recs, (float*)a.out, a.B, a.C, a.H, a.W, nullptr);
}

struct Unwarp { char *y, *recs, *w_in, *out, *valid, *w_out; float margin; int B, K, h, w; };
static Unwarp unwarp_ok(int B = 2, int K = 21, int h = 16, int w = 16, size_t in_off = 0, size_t out_off = 0, bool weights = true) {
  return Unwarp{fp(1, in_off), fp(2, in_off), weights ? fp(3, in_off) : nullptr, fp(4, out_off), fp(5, out_off), weights ? fp(6, out_off) : nullptr,
                2.0f, B, K, h, w};
}
static int run(const Unwarp& a) {
  return mi355_affine_unwarp_heatmaps((const float*)a.y, (const mi355_view_rec*)a.recs, a.margin, (const float*)a.w_in, (float*)a.out,
                                      (float*)a.valid, (float*)a.w_out, a.B, a.K, a.h, a.w, nullptr);
}

struct Mse { char *pred, *target, *rec, *wmap, *rows, *grad; int B, K, HW; };
static Mse mse_ok(int B = 2, int K = 21, int HW = 64, size_t off = 0, bool grad = true) {
  return Mse{fp(1, off), fp(2, off), fp(3), fp(4, off), fp(5, off), grad ? fp(6, off) : nullptr, B, K, HW};
}
static int run(const Mse& a) {
  return mi355_mse_heatmap_w((const float*)a.pred, (const float*)a.target, (const mi355_mse_rec*)a.rec, (const float*)a.wmap, (float*)a.rows,
                             (float*)a.grad, a.B, a.K, a.HW, nullptr);
}

int main() {
  static_assert(sizeof(mi355_view_rec) == 72, "three 2 x 3 fp32 matrices");
  // ---- the shapes of tests/test_gpu_warp.py, aligned and 4 bytes off (inputs, outputs, both), and the largest extents
  struct { int B, C, H, W; } images[] = {{1, 3, 16, 16}, {3, 3, 17, 19}, {2, 1, 24, 40}, {2, 3, 64, 64}, {2, 3, 256, 256}, {64, 3, 256, 256},
                                         {1, 1, 1, 1}, {2, 3, MI355_WARP_MAX_SIDE, MI355_WARP_MAX_SIDE}};
  for (auto& s : images)
    for (size_t in_off : {(size_t)0, (size_t)4})
      for (size_t out_off : {(size_t)0, (size_t)4})
        EXPECT(ran(run(warp_ok(s.B, s.C, s.H, s.W, in_off, out_off))));
  struct { int B, K, h, w; } maps[] = {{1, 1, 4, 4}, {3, 21, 16, 16}, {2, 5, 17, 19}, {2, 21, 64, 64}, {1, 3, 128, 128}, {1, 2, 130, 127},
                                       {64, 21, 64, 64}, {1, 1, 1, 1}, {1, 1, MI355_WARP_MAX_SIDE, MI355_WARP_MAX_SIDE}};
  for (auto& s : maps)
    for (size_t in_off : {(size_t)0, (size_t)4})
      for (size_t out_off : {(size_t)0, (size_t)4})
        for (bool weights : {true, false}) {
          EXPECT(ran(run(unwarp_ok(s.B, s.K, s.h, s.w, in_off, out_off, weights))));
          if (s.K <= 32 && (long)s.h * s.w <= 0x7fffffffL) EXPECT(ran(run(mse_ok(s.B, s.K, s.h * s.w, in_off, weights))));
        }
  for (float m : {0.0f, 0.5f, 2.0f, 1.0e30f}) { Unwarp a = unwarp_ok(); a.margin = m; EXPECT(ran(run(a))); }
  const long nx = 4L * 2 * 3 * 16 * 20, ny = 4L * 2 * 21 * 16 * 16, nr = 4L * 2 * 21;
  { Warp a = warp_ok(); a.out = a.x + nx; EXPECT(ran(run(a))); }                                    // touching is not overlapping
  { Warp a = warp_ok(); a.x = a.out + nx; EXPECT(ran(run(a))); }
  { Warp a = warp_ok(); a.recs = a.out + nx; EXPECT(ran(run(a))); }
  { Unwarp a = unwarp_ok(); a.out = a.y + ny; EXPECT(ran(run(a))); }
  { Unwarp a = unwarp_ok(); a.valid = a.out + ny; a.w_out = a.valid + nr; EXPECT(ran(run(a))); }

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  { Warp a = warp_ok(); a.x = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Warp a = warp_ok(); a.recs = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Warp a = warp_ok(); a.out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  EXPECT(run(warp_ok(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(warp_ok(-3)) == MI355_EINVAL && says("B=-3"));
  EXPECT(run(warp_ok(2, 0)) == MI355_EINVAL && says("C=0"));
  EXPECT(run(warp_ok(2, 3, 0, 20)) == MI355_EINVAL && says("H=0"));
  EXPECT(run(warp_ok(2, 3, 16, 0)) == MI355_EINVAL && says("W=0"));
  EXPECT(run(warp_ok(2, 3, MI355_WARP_MAX_SIDE + 1, 20)) == MI355_EINVAL && says("H=4097"));
  EXPECT(run(warp_ok(2, 3, 16, MI355_WARP_MAX_SIDE + 1)) == MI355_EINVAL && says("W=4097"));
  EXPECT(run(warp_ok(0x7fffffff, 0x7fffffff, MI355_WARP_MAX_SIDE, MI355_WARP_MAX_SIDE)) == MI355_EINVAL && says("too large"));
  { Warp a = warp_ok(); a.x += 2; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Warp a = warp_ok(); a.recs += 1; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Warp a = warp_ok(); a.out += 3; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Warp a = warp_ok(); a.out = a.x; EXPECT(run(a) == MI355_EINVAL && says("out and x overlap")); }                  // in place
  { Warp a = warp_ok(); a.out = a.x + nx - 4; EXPECT(run(a) == MI355_EINVAL && says("out and x overlap")); }         // by one float
  { Warp a = warp_ok(); a.recs = a.out + nx - 4; EXPECT(run(a) == MI355_EINVAL && says("out and recs overlap")); }

  { Unwarp a = unwarp_ok(); a.y = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Unwarp a = unwarp_ok(); a.recs = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Unwarp a = unwarp_ok(); a.out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Unwarp a = unwarp_ok(); a.valid = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Unwarp a = unwarp_ok(); a.w_in = nullptr; EXPECT(run(a) == MI355_EINVAL && says("go together")); }
  { Unwarp a = unwarp_ok(); a.w_out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("go together")); }
  EXPECT(run(unwarp_ok(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(unwarp_ok(2, 0)) == MI355_EINVAL && says("K=0"));
  EXPECT(run(unwarp_ok(2, -1)) == MI355_EINVAL && says("K=-1"));
  EXPECT(run(unwarp_ok(2, 21, 0, 16)) == MI355_EINVAL && says("h=0"));
  EXPECT(run(unwarp_ok(2, 21, 16, 0)) == MI355_EINVAL && says("w=0"));
  EXPECT(run(unwarp_ok(2, 21, MI355_WARP_MAX_SIDE + 1, 16)) == MI355_EINVAL && says("h=4097"));
  EXPECT(run(unwarp_ok(2, 21, 16, MI355_WARP_MAX_SIDE + 1)) == MI355_EINVAL && says("w=4097"));
  EXPECT(run(unwarp_ok(0x7fffffff, 0x7fffffff)) == MI355_EINVAL && says("too many maps"));
  EXPECT(run(unwarp_ok(0x7fffffff, 1, MI355_WARP_MAX_SIDE, MI355_WARP_MAX_SIDE)) == MI355_EINVAL && says("too large"));
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float bad : {-1.0f, -0.0001f, inf, -inf, nan}) { Unwarp a = unwarp_ok(); a.margin = bad; EXPECT(run(a) == MI355_EINVAL && says("margin")); }
  { Unwarp a = unwarp_ok(); a.y += 2; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Unwarp a = unwarp_ok(); a.w_in += 1; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Unwarp a = unwarp_ok(); a.valid += 3; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Unwarp a = unwarp_ok(); a.w_out += 2; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Unwarp a = unwarp_ok(); a.out = a.y; EXPECT(run(a) == MI355_EINVAL && says("out and y overlap")); }
  { Unwarp a = unwarp_ok(); a.out = a.y + ny - 4; EXPECT(run(a) == MI355_EINVAL && says("out and y overlap")); }
  { Unwarp a = unwarp_ok(); a.valid = a.y + 64; EXPECT(run(a) == MI355_EINVAL && says("valid and y overlap")); }
  { Unwarp a = unwarp_ok(); a.w_out = a.w_in; EXPECT(run(a) == MI355_EINVAL && says("w_out and w_in overlap")); }
  { Unwarp a = unwarp_ok(); a.w_out = a.recs + 8; EXPECT(run(a) == MI355_EINVAL && says("w_out and recs overlap")); }
  { Unwarp a = unwarp_ok(); a.valid = a.out + ny - 4; EXPECT(run(a) == MI355_EINVAL && says("out and valid overlap")); }
  { Unwarp a = unwarp_ok(); a.w_out = a.valid + nr - 4; EXPECT(run(a) == MI355_EINVAL && says("valid and w_out overlap")); }

  { Mse a = mse_ok(); a.pred = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Mse a = mse_ok(); a.target = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Mse a = mse_ok(); a.rec = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Mse a = mse_ok(); a.wmap = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  { Mse a = mse_ok(); a.rows = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null pointer")); }
  EXPECT(ran(run(mse_ok(2, 21, 64, 0, false))));                                                      // the gradient is optional
  EXPECT(run(mse_ok(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(mse_ok(2, 0)) == MI355_EINVAL && says("K=0"));
  EXPECT(run(mse_ok(2, 33)) == MI355_EINVAL && says("K=33"));
  EXPECT(run(mse_ok(2, 21, 0)) == MI355_EINVAL && says("HW=0"));
  EXPECT(run(mse_ok(0x7fffffff, 32)) == MI355_EINVAL && says("too many rows"));
  { Mse a = mse_ok(); a.wmap += 2; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  { Mse a = mse_ok(); a.grad += 1; EXPECT(run(a) == MI355_EINVAL && says("4-byte aligned")); }
  std::printf("warp driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

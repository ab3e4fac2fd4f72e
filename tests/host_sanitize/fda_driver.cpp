// Host-side exerciser of the Fourier-domain stylisation entry points (mi355_fda_workspace_bytes, mi355_fda_transfer) for the
// CPU-box sanitizer job (tests/test_host_fda.py): built like mixup_driver.cpp -- the HOST pass of every .hip file with
// -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned
// addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run.
// The job passes when no sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL (-1 bytes),
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

struct Args { char *x_s, *x_t, *out, *ws; float mean[4], std[4]; const float *pm, *ps; int B, C, H, W, b; long ws_bytes; };
static Args ok_args(int B = 2, int C = 3, int H = 16, int W = 20, int b = 2, size_t off = 0) {
  Args a;
  a.x_s = fp(1, off); a.x_t = fp(2, off); a.out = fp(3, off); a.ws = fp(4);
  const float m[4] = {0.485f, 0.456f, 0.406f, 0.5f}, s[4] = {0.229f, 0.224f, 0.225f, 0.25f};
  std::memcpy(a.mean, m, sizeof(m)); std::memcpy(a.std, s, sizeof(s));
  a.pm = nullptr; a.ps = nullptr;
  a.B = B; a.C = C; a.H = H; a.W = W; a.b = b;
  a.ws_bytes = mi355_fda_workspace_bytes(B, C, H, W, b);
  return a;
}
static int run(const Args& a, bool null_mean = false, bool null_std = false) {
  return mi355_fda_transfer((const float*)a.x_s, (const float*)a.x_t, (float*)a.out, null_mean ? nullptr : a.mean, null_std ? nullptr : a.std,
                            a.B, a.C, a.H, a.W, a.b, a.ws, a.ws_bytes, nullptr);
}

int main() {
  // ---- the shapes of tests/test_gpu_fda.py, aligned and 4 bytes off, and the largest extents
  struct { int C, H, W, b; } shapes[] = {{3, 16, 16, 0}, {3, 16, 16, 1}, {3, 16, 16, 7}, {3, 16, 32, 2}, {3, 48, 16, 2}, {3, 17, 19, 2},
                                         {1, 24, 40, 3}, {3, 64, 64, 5}, {3, 128, 128, 32}, {3, 256, 256, 2}, {4, 1024, 1024, 32}, {1, 1, 1, 0}};
  for (auto& s : shapes)
    for (int B : {1, 2, 3, 64})
      for (size_t off : {(size_t)0, (size_t)4}) {
        const long need = mi355_fda_workspace_bytes(B, s.C, s.H, s.W, s.b);
        EXPECT(need == (long)B * s.C * ((s.H + 31) / 32) * 2 * (2 * s.b + 1) * (s.b + 1) * 16);
        EXPECT(ran(run(ok_args(B, s.C, s.H, s.W, s.b, off))));
      }
  { Args a = ok_args(); a.ws_bytes += 100; EXPECT(ran(run(a))); }                                   // a larger workspace is fine
  const long nx = 4L * 2 * 3 * 16 * 20;
  { Args a = ok_args(); a.out = a.x_s + nx; EXPECT(ran(run(a))); }                                  // touching is not overlapping
  { Args a = ok_args(); a.x_t = a.out + nx; EXPECT(ran(run(a))); }
  { Args a = ok_args(); a.ws = a.x_s + nx; EXPECT(ran(run(a))); }
  { Args a = ok_args(); a.out = a.ws + a.ws_bytes; EXPECT(ran(run(a))); }

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(mi355_fda_workspace_bytes(2, 3, 16, 20, -1) == -1 && says("b=-1"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 256, 256, 33) == -1 && says("b=33") && says("MI355_FDA_MAX_B"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 16, 20, 8) == -1 && says("b=8") && says("min(H, W)"));
  EXPECT(mi355_fda_workspace_bytes(2, 0, 16, 20, 2) == -1 && says("C=0"));
  EXPECT(mi355_fda_workspace_bytes(2, 5, 16, 20, 2) == -1 && says("C=5"));
  EXPECT(mi355_fda_workspace_bytes(0, 3, 16, 20, 2) == -1 && says("B=0"));
  EXPECT(mi355_fda_workspace_bytes(-7, 3, 16, 20, 2) == -1 && says("B=-7"));
  EXPECT(mi355_fda_workspace_bytes(0x7fffffff, 4, 1024, 1024, 32) == -1 && says("B=2147483647"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 0, 20, 0) == -1 && says("H=0"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 1025, 20, 2) == -1 && says("H=1025"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 16, 0, 0) == -1 && says("W=0"));
  EXPECT(mi355_fda_workspace_bytes(2, 3, 16, 1025, 2) == -1 && says("W=1025"));
  EXPECT(run(ok_args(2, 3, 16, 20, -1)) == MI355_EINVAL && says("b=-1"));
  EXPECT(run(ok_args(2, 3, 256, 256, 33)) == MI355_EINVAL && says("b=33"));
  EXPECT(run(ok_args(2, 3, 16, 20, 8)) == MI355_EINVAL && says("b=8"));
  EXPECT(run(ok_args(2, 0)) == MI355_EINVAL && says("C=0"));
  EXPECT(run(ok_args(2, 5)) == MI355_EINVAL && says("C=5"));
  EXPECT(run(ok_args(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(ok_args(-1)) == MI355_EINVAL && says("B=-1"));
  EXPECT(run(ok_args(2, 3, 0, 20, 0)) == MI355_EINVAL && says("H=0"));
  EXPECT(run(ok_args(2, 3, 2000, 20, 2)) == MI355_EINVAL && says("H=2000"));
  EXPECT(run(ok_args(2, 3, 16, 0, 0)) == MI355_EINVAL && says("W=0"));
  EXPECT(run(ok_args(2, 3, 16, 1025, 2)) == MI355_EINVAL && says("W=1025"));
  { Args a = ok_args(); a.x_s = nullptr; EXPECT(run(a) == MI355_EINVAL && says("x_s is null")); }
  { Args a = ok_args(); a.x_t = nullptr; EXPECT(run(a) == MI355_EINVAL && says("x_t is null")); }
  { Args a = ok_args(); a.out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("out is null")); }
  { Args a = ok_args(); a.ws = nullptr; EXPECT(run(a) == MI355_EINVAL && says("ws is null")); }
  EXPECT(run(ok_args(), true) == MI355_EINVAL && says("mean is null"));
  EXPECT(run(ok_args(), false, true) == MI355_EINVAL && says("std is null"));
  { Args a = ok_args(); a.x_s += 2; EXPECT(run(a) == MI355_EINVAL && says("x_s must be 4-byte aligned")); }
  { Args a = ok_args(); a.x_t += 1; EXPECT(run(a) == MI355_EINVAL && says("x_t must be 4-byte aligned")); }
  { Args a = ok_args(); a.out += 3; EXPECT(run(a) == MI355_EINVAL && says("out must be 4-byte aligned")); }
  { Args a = ok_args(); a.ws += 8; EXPECT(run(a) == MI355_EINVAL && says("ws must be 16-byte aligned")); }
  { Args a = ok_args(); a.ws_bytes -= 1; EXPECT(run(a) == MI355_EINVAL && says("ws_bytes") && says("too small")); }
  { Args a = ok_args(); a.ws_bytes = -1; EXPECT(run(a) == MI355_EINVAL && says("ws_bytes=-1")); }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float bad : {0.0f, -0.5f, inf, nan}) { Args a = ok_args(); a.std[2] = bad; EXPECT(run(a) == MI355_EINVAL && says("std[2]")); }
  for (float bad : {inf, -inf, nan}) { Args a = ok_args(); a.mean[0] = bad; EXPECT(run(a) == MI355_EINVAL && says("mean[0]")); }
  { Args a = ok_args(2, 1); a.std[2] = nan; a.mean[3] = inf; EXPECT(ran(run(a))); }                 // (only the first C values are read)
  { Args a = ok_args(); a.out = a.x_s; EXPECT(run(a) == MI355_EINVAL && says("out and x_s overlap")); }               // in place
  { Args a = ok_args(); a.out = a.x_s + nx - 4; EXPECT(run(a) == MI355_EINVAL && says("out and x_s overlap")); }      // by one float
  { Args a = ok_args(); a.x_t = a.out + nx - 4; EXPECT(run(a) == MI355_EINVAL && says("out and x_t overlap")); }
  { Args a = ok_args(); a.ws = a.x_s + 16; EXPECT(run(a) == MI355_EINVAL && says("ws and x_s overlap")); }
  { Args a = ok_args(); a.x_t = a.ws + a.ws_bytes - 4; EXPECT(run(a) == MI355_EINVAL && says("ws and x_t overlap")); }
  { Args a = ok_args(); a.ws = a.out + nx - 16; EXPECT(run(a) == MI355_EINVAL && says("ws and out overlap")); }
  std::printf("fda driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

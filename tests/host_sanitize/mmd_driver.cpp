// Host-side exerciser of the MMD entry points (mi355_mmd_workspace / mi355_mmd_heatmap) for the CPU-box sanitizer job
// (tests/test_host_mmd.py): built like teacher_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined,
// linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned addresses that the host never
// dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run.  The job passes when no
// sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL, naming what is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static void* fake(size_t i) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + (i << 28))); }
static float* ff(size_t i, size_t off = 0) { return reinterpret_cast<float*>(fake(i)) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static int run(int B, int K, int HW, float mul = 2.f, int num = 5, float fix = 0.f, float scale = 1.f, int grads = 3, size_t off = 0) {
  return mi355_mmd_heatmap(ff(1, off), ff(2, off), ff(3), mi355_mmd_workspace(B, K), ff(4), (grads & 1) ? ff(5, off) : nullptr,
                           (grads & 2) ? ff(6, off) : nullptr, B, K, HW, mul, num, fix, scale, nullptr);
}

int main() {
  // ---- workspace sizes
  EXPECT(mi355_mmd_workspace(1, 1) == 16 && mi355_mmd_workspace(2, 21) == 21u * 16 * 4 && mi355_mmd_workspace(64, 21) == 21u * 128 * 128 * 4);
  EXPECT(mi355_mmd_workspace(128, 3) == 3u * 256 * 256 * 4 && mi355_mmd_workspace(128, 65535) == (size_t)65535 * 256 * 256 * 4);
  EXPECT(mi355_mmd_workspace(129, 1) == 0 && mi355_mmd_workspace(0, 1) == 0 && mi355_mmd_workspace(1, 0) == 0 && mi355_mmd_workspace(-3, -3) == 0);
  EXPECT(mi355_mmd_workspace(0x7fffffff, 1) == 0 && mi355_mmd_workspace(1, 0x7fffffff) == (size_t)0x7fffffff * 16);

  // ---- the shapes of tests/test_gpu_mmd.py: every batch size and row length, aligned and not, every gradient request
  for (int B : {1, 2, 3, 4, 5, 7, 9, 15, 17, 64, 128})
    for (int hw : {1, 35, 56, 64, 68, 70, 1028, 4096})
      for (int grads = 0; grads < 4; ++grads)
        for (size_t off = 0; off <= 1; ++off)
          EXPECT(ran(run(B, B > 17 ? 3 : 21, hw, 2.f, 5, 0.f, 1.f, grads, off)));
  EXPECT(ran(run(2, 1, 64)));
  for (int num = 1; num <= MI355_MMD_MAX_KERNELS; ++num) EXPECT(ran(run(2, 21, 64, 2.f, num)));
  EXPECT(ran(run(2, 21, 64, 1.5f, 8, 3.f, 0.1f)));
  EXPECT(ran(run(2, 21, 64, 1e-3f, 8)) && ran(run(2, 21, 64, 1e3f, 8)) && ran(run(2, 21, 64, 2.f, 5, -1.f)) && ran(run(2, 21, 64, 2.f, 5, 0.f, 0.f)));
  EXPECT(ran(run(128, 65535, 1)) && ran(run(1, 1, 1 << 30)));

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  const size_t ws = mi355_mmd_workspace(2, 21);
  EXPECT(mi355_mmd_heatmap(nullptr, ff(2), ff(3), ws, ff(4), ff(5), ff(6), 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mmd_heatmap(ff(1), nullptr, ff(3), ws, ff(4), ff(5), ff(6), 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mmd_heatmap(ff(1), ff(2), nullptr, ws, ff(4), ff(5), ff(6), 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mmd_heatmap(ff(1), ff(2), ff(3), ws, nullptr, ff(5), ff(6), 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("null"));
  for (int which = 0; which < 6; ++which) {          // a pointer that is not even 4-byte aligned, each in turn
    float* p[6] = {ff(1), ff(2), ff(3), ff(4), ff(5), ff(6)};
    p[which] = (float*)((char*)p[which] + 2);
    EXPECT(mi355_mmd_heatmap(p[0], p[1], p[2], ws, p[3], p[4], p[5], 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
  }
  EXPECT(run(0, 21, 64) == MI355_EINVAL && says("B=0"));
  EXPECT(run(-1, 21, 64) == MI355_EINVAL && says("B=-1"));
  EXPECT(run(2, 0, 64) == MI355_EINVAL && says("K=0"));
  EXPECT(run(2, 21, 0) == MI355_EINVAL && says("HW=0"));
  EXPECT(run(2, 21, -5) == MI355_EINVAL && says("HW=-5"));
  EXPECT(run(129, 1, 64) == MI355_EINVAL && says("258 rows"));
  EXPECT(run(0x7fffffff, 1, 64) == MI355_EINVAL && says("rows"));
  EXPECT(run(2, 65536, 64) == MI355_EINVAL && says("K=65536"));
  EXPECT(run(2, 21, (1 << 30) + 1) == MI355_EINVAL && says("HW="));
  EXPECT(run(2, 21, 64, 2.f, 0) == MI355_EINVAL && says("kernel_num=0"));
  EXPECT(run(2, 21, 64, 2.f, 9) == MI355_EINVAL && says("kernel_num=9"));
  EXPECT(run(2, 21, 64, 2.f, -1) == MI355_EINVAL && says("kernel_num=-1"));
  EXPECT(run(2, 21, 64, 0.f) == MI355_EINVAL && says("kernel_mul"));
  EXPECT(run(2, 21, 64, -2.f) == MI355_EINVAL && says("kernel_mul"));
  EXPECT(run(2, 21, 64, NAN) == MI355_EINVAL && says("kernel_mul"));
  EXPECT(run(2, 21, 64, INFINITY) == MI355_EINVAL && says("kernel_mul"));
  EXPECT(run(2, 21, 64, 2.f, 5, NAN) == MI355_EINVAL && says("fix_sigma"));
  EXPECT(run(2, 21, 64, 2.f, 5, 0.f, INFINITY) == MI355_EINVAL && says("scale"));
  EXPECT(mi355_mmd_heatmap(ff(1), ff(2), ff(3), ws - 1, ff(4), ff(5), ff(6), 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("workspace"));
  EXPECT(mi355_mmd_heatmap(ff(1), ff(2), ff(3), 0, ff(4), nullptr, nullptr, 2, 21, 64, 2.f, 5, 0.f, 1.f, nullptr) == MI355_EINVAL && says("workspace"));
  std::printf("mmd driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

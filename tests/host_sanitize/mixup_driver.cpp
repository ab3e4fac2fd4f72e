// Host-side exerciser of the cross-domain mixup entry point (mi355_mixup_pairs) for the CPU-box sanitizer job
// (tests/test_host_mixup.py): built like mmd_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined,
// linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned addresses that the host never
// dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run.  The job passes when no
// sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL, naming what is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static float* ff(size_t i, size_t off = 0) { return reinterpret_cast<float*>(static_cast<uintptr_t>(0x100000000ull + (i << 44))) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

struct Args { float* p[10]; int B; long img, hm; int K; };
static Args ok_args(int B = 3, long img = 105, long hm = 735, int K = 21, size_t off = 0) {
  Args a;
  for (int i = 0; i < 10; ++i) a.p[i] = ff(i + 1, off);
  a.B = B; a.img = img; a.hm = hm; a.K = K;
  return a;
}
static int run(const Args& a) {
  return mi355_mixup_pairs(a.p[0], a.p[1], a.p[2], a.p[3], a.p[4], a.p[5], a.p[6], a.p[7], a.p[8], a.p[9], a.B, a.img, a.hm, a.K, nullptr);
}

int main() {
  // ---- the shapes of tests/test_gpu_mixup.py: every batch size, image and heat-map plane, aligned and 4 bytes off
  for (int B : {1, 3, 5, 64})
    for (long img : {12L, 105L, 768L, 3L * 512 * 512, 3L * 256 * 256})
      for (long hm : {21L, 735L, 1344L, 21L * 64 * 64})
        for (size_t off = 0; off <= 1; ++off)
          EXPECT(ran(run(ok_args(B, img, hm, 21, off))));
  EXPECT(ran(run(ok_args(1, 1, 1, 1))));
  EXPECT(ran(run(ok_args(2, (1L << 31) + 3, 7, 1))));                 // 2 n above 2^31: the wide index build
  EXPECT(ran(run(ok_args(1, 1L << 40, 1L << 40, 1))));               // the largest extent that is accepted
  { Args a = ok_args(); a.p[1] = a.p[7] + 2 * 3 * 105; EXPECT(ran(run(a))); }      // x_t right behind x_mix: touching is not overlapping
  { Args a = ok_args(); a.p[7] = a.p[0] + 3 * 105; EXPECT(ran(run(a))); }          // x_mix right behind x_s

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  for (int i = 0; i < 10; ++i) { Args a = ok_args(); a.p[i] = nullptr; EXPECT(run(a) == MI355_EINVAL && says("null")); }
  for (int i = 0; i < 10; ++i) {                                      // a pointer that is not even 4-byte aligned, each in turn
    Args a = ok_args(); a.p[i] = (float*)((char*)a.p[i] + 2); EXPECT(run(a) == MI355_EINVAL && says("aligned"));
  }
  EXPECT(run(ok_args(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(ok_args(-1)) == MI355_EINVAL && says("B=-1"));
  EXPECT(run(ok_args(3, 0)) == MI355_EINVAL && says("img_plane=0"));
  EXPECT(run(ok_args(3, -7)) == MI355_EINVAL && says("img_plane=-7"));
  EXPECT(run(ok_args(3, 105, 0)) == MI355_EINVAL && says("hm_plane=0"));
  EXPECT(run(ok_args(3, 105, 735, 0)) == MI355_EINVAL && says("K=0"));
  EXPECT(run(ok_args(3, 105, 735, -21)) == MI355_EINVAL && says("K=-21"));
  EXPECT(run(ok_args(2, 1L << 40, 7)) == MI355_EINVAL && says("too large"));
  EXPECT(run(ok_args(0x7fffffff, 105, 1L << 40)) == MI355_EINVAL && says("too large"));
  EXPECT(run(ok_args(3, 0x7fffffffffffffffL, 7)) == MI355_EINVAL && says("too large"));
  { Args a = ok_args(); a.p[7] = a.p[0]; EXPECT(run(a) == MI355_EINVAL && says("x_mix and x_s overlap")); }                 // in place
  { Args a = ok_args(); a.p[7] = a.p[0] + 3 * 105 - 1; EXPECT(run(a) == MI355_EINVAL && says("x_mix and x_s overlap")); }   // by one float
  { Args a = ok_args(); a.p[1] = a.p[7] + 2 * 3 * 105 - 1; EXPECT(run(a) == MI355_EINVAL && says("x_mix and x_t overlap")); }
  { Args a = ok_args(); a.p[8] = a.p[2] + 5; EXPECT(run(a) == MI355_EINVAL && says("hm_mix and hm_s overlap")); }
  { Args a = ok_args(); a.p[8] = a.p[3]; EXPECT(run(a) == MI355_EINVAL && says("hm_mix and hm_t overlap")); }
  { Args a = ok_args(); a.p[9] = a.p[4] + 1; EXPECT(run(a) == MI355_EINVAL && says("w_mix and w_s overlap")); }
  { Args a = ok_args(); a.p[5] = a.p[9] + 2 * 3 * 21 - 1; EXPECT(run(a) == MI355_EINVAL && says("w_mix and w_t overlap")); }
  { Args a = ok_args(); a.p[6] = a.p[8] + 100; EXPECT(run(a) == MI355_EINVAL && says("hm_mix and lam overlap")); }
  { Args a = ok_args(); a.p[8] = a.p[7] + 3 * 105; EXPECT(run(a) == MI355_EINVAL && says("x_mix and hm_mix overlap")); }    // in the second half
  { Args a = ok_args(); a.p[9] = a.p[8]; EXPECT(run(a) == MI355_EINVAL && says("hm_mix and w_mix overlap")); }
  std::printf("mixup driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

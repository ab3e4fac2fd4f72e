// Host-side exerciser of mi355_peak_prob, mi355_teacher_select and mi355_occlude_images for the CPU-box sanitizer job
// (tests/test_host_occlude.py): built like bone_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined,
// linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned addresses that the host never
// dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run.  The job passes when no
// sanitizer report aborts the process, every accepted shape reaches the launch and every refused argument comes back as
// MI355_EINVAL with a message that names what is wrong.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
template <typename T = float> static T* fake(size_t i, size_t off = 0) { return reinterpret_cast<T*>(static_cast<uintptr_t>(0x100000000ull + (i << 28) + off)); }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static int peak(const float* hm, float beta, int32_t* idx, float* xy, float* p, int rows, int H, int W) {
  return mi355_peak_prob(hm, beta, idx, xy, p, rows, H, W, nullptr);
}

struct Sel {
  const float *p = fake(4), *xy = fake(5), *gate = nullptr, *w_in = nullptr, *u = fake(6);
  float tau = 0.02f, prob = 0.5f;
  int N = 1, lo = 20, hi = 41, S = 256, H = 64, W = 64;
  float *conf = fake(7), *w_out = nullptr;
  int32_t *boxes = fake<int32_t>(8), *count = fake<int32_t>(9);
  float* stats = fake(10);
  int B = 3, K = 21;
  int call() const { return mi355_teacher_select(p, xy, gate, w_in, u, tau, prob, N, lo, hi, S, H, W, conf, w_out, boxes, count, stats, B, K, nullptr); }
};

static int occ(const float* x, const int32_t* boxes, int N, float* out, int B, int C, int H, int W) {
  return mi355_occlude_images(x, boxes, N, out, B, C, H, W, nullptr);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");

  // ---- peak_prob: the sides and row counts of tests/test_gpu_occlude.py, aligned and one float past a 16-byte boundary
  float *hm = fake(1), *xy = fake(2), *p = fake(3);
  int32_t* idx = fake<int32_t>(11);
  const int sides[][2] = {{64, 64}, {32, 32}, {16, 16}, {24, 40}, {1, 1}, {1, 3}, {63, 65}, {128, 128}};
  for (const auto& s : sides)
    for (int n : {1, 4, 5, 21, 1344})
      for (float beta : {1.f, 3.f}) {
        EXPECT(ran(peak(hm, beta, idx, xy, p, n, s[0], s[1])));
        EXPECT(ran(peak(fake(1, 4), beta, fake<int32_t>(11, 4), fake(2, 4), fake(3, 4), n, s[0], s[1])));
      }
  EXPECT(ran(peak(hm, 1.f, idx, xy, p, 1, 46340, 46340)));                                          // H*W just below 2^31
  EXPECT(ran(peak(hm, 1e-30f, idx, xy, p, 0x7fffffff, 1, 1)));
  EXPECT(peak(nullptr, 1.f, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("null hm"));
  EXPECT(peak(hm, 1.f, nullptr, xy, p, 4, 16, 16) == MI355_EINVAL && says("null idx"));
  EXPECT(peak(hm, 1.f, idx, nullptr, p, 4, 16, 16) == MI355_EINVAL && says("null xy"));
  EXPECT(peak(hm, 1.f, idx, xy, nullptr, 4, 16, 16) == MI355_EINVAL && says("null p"));
  EXPECT(peak(hm, 1.f, idx, xy, p, 0, 16, 16) == MI355_EINVAL && says("rows=0"));
  EXPECT(peak(hm, 1.f, idx, xy, p, -3, 16, 16) == MI355_EINVAL && says("rows=-3"));
  EXPECT(peak(hm, 1.f, idx, xy, p, 4, 0, 16) == MI355_EINVAL && says("H=0"));
  EXPECT(peak(hm, 1.f, idx, xy, p, 4, 16, -1) == MI355_EINVAL && says("W=-1"));
  EXPECT(peak(hm, 1.f, idx, xy, p, 1, 46341, 46341) == MI355_EINVAL && says("2^31"));
  EXPECT(peak(hm, 1.f, idx, xy, p, 1, 0x7fffffff, 0x7fffffff) == MI355_EINVAL && says("2^31"));
  EXPECT(peak(fake(1, 2), 1.f, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("aligned"));
  EXPECT(peak(hm, 0.f, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(peak(hm, -1.f, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(peak(hm, inf, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(peak(hm, nan, idx, xy, p, 4, 16, 16) == MI355_EINVAL && says("beta"));

  // ---- teacher_select: batches, joint counts, box counts and sides of the GPU tests, and the limits
  const int ssides[][2] = {{256, 64}, {64, 16}, {16, 16}, {4096, 1}};
  for (int B : {1, 3, 64, 300, MI355_OCC_MAX_BATCH})
    for (int K : {1, 21, MI355_OCC_MAX_JOINTS})
      for (int N : {0, 1, MI355_OCC_MAX_BOXES})
        for (const auto& s : ssides) {
          Sel a; a.B = B; a.K = K; a.N = N; a.S = s[0]; a.H = a.W = s[1]; a.lo = 1; a.hi = s[0];
          EXPECT(ran(a.call()));
          a.gate = fake(12); a.w_in = fake(13); a.w_out = fake(14); a.lo = a.hi = 3; a.stats = nullptr;
          EXPECT(ran(a.call()));
        }
  { Sel a; a.N = 0; a.xy = nullptr; a.u = nullptr; a.boxes = nullptr; a.count = nullptr; a.lo = 7; a.hi = 2; a.S = 0; EXPECT(ran(a.call())); }   // the gate alone reads no box argument
  { Sel a; a.prob = 0.f; EXPECT(ran(a.call())); a.prob = 1.f; EXPECT(ran(a.call())); a.tau = -1.f; EXPECT(ran(a.call())); }
  { Sel a; a.S = 256; a.H = 32; a.W = 64; EXPECT(ran(a.call())); }
  { Sel a; a.p = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null p")); }
  { Sel a; a.conf = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null conf")); }
  { Sel a; a.xy = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null xy")); }
  { Sel a; a.u = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null u")); }
  { Sel a; a.boxes = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null boxes")); }
  { Sel a; a.count = nullptr; EXPECT(a.call() == MI355_EINVAL && says("null count")); }
  { Sel a; a.w_in = fake(13); EXPECT(a.call() == MI355_EINVAL && says("w_in and w_out")); }
  { Sel a; a.w_out = fake(14); EXPECT(a.call() == MI355_EINVAL && says("w_in and w_out")); }
  { Sel a; a.B = 0; EXPECT(a.call() == MI355_EINVAL && says("B=0")); }
  { Sel a; a.B = MI355_OCC_MAX_BATCH + 1; EXPECT(a.call() == MI355_EINVAL && says("B=")); }
  { Sel a; a.K = 0; EXPECT(a.call() == MI355_EINVAL && says("K=0")); }
  { Sel a; a.K = MI355_OCC_MAX_JOINTS + 1; EXPECT(a.call() == MI355_EINVAL && says("K=65")); }
  { Sel a; a.N = -1; EXPECT(a.call() == MI355_EINVAL && says("N=-1")); }
  { Sel a; a.N = MI355_OCC_MAX_BOXES + 1; EXPECT(a.call() == MI355_EINVAL && says("N=9")); }
  { Sel a; a.N = 0x7fffffff; EXPECT(a.call() == MI355_EINVAL && says("N=")); }
  { Sel a; a.lo = 42; EXPECT(a.call() == MI355_EINVAL && says("lo=42")); }
  { Sel a; a.lo = 0; EXPECT(a.call() == MI355_EINVAL && says("lo=0")); }
  { Sel a; a.lo = -5; EXPECT(a.call() == MI355_EINVAL && says("lo=-5")); }
  { Sel a; a.hi = 257; EXPECT(a.call() == MI355_EINVAL && says("hi=257")); }
  { Sel a; a.hi = 0x7fffffff; EXPECT(a.call() == MI355_EINVAL && says("hi=")); }
  { Sel a; a.prob = -0.1f; EXPECT(a.call() == MI355_EINVAL && says("prob")); }
  { Sel a; a.prob = 1.5f; EXPECT(a.call() == MI355_EINVAL && says("prob")); }
  { Sel a; a.prob = nan; EXPECT(a.call() == MI355_EINVAL && says("prob")); }
  { Sel a; a.tau = nan; EXPECT(a.call() == MI355_EINVAL && says("tau")); }
  { Sel a; a.tau = inf; EXPECT(a.call() == MI355_EINVAL && says("tau")); }
  { Sel a; a.tau = -inf; EXPECT(a.call() == MI355_EINVAL && says("tau")); }
  { Sel a; a.S = 250; EXPECT(a.call() == MI355_EINVAL && says("multiple")); }
  { Sel a; a.H = 48; EXPECT(a.call() == MI355_EINVAL && says("multiple")); }
  { Sel a; a.W = 0; EXPECT(a.call() == MI355_EINVAL && says("multiple")); }
  { Sel a; a.H = -4; EXPECT(a.call() == MI355_EINVAL && says("multiple")); }
  { Sel a; a.S = 0; EXPECT(a.call() == MI355_EINVAL && says("S=0")); }
  { Sel a; a.S = MI355_OCC_MAX_SIDE * 2; a.hi = 41; EXPECT(a.call() == MI355_EINVAL && says("S=")); }
  { Sel a; a.p = fake(4, 2); EXPECT(a.call() == MI355_EINVAL && says("aligned")); }

  // ---- occlude_images: the shapes of the GPU tests, the flagship shape, each operand one float past a 16-byte boundary
  float *x = fake(15), *out = fake(17);
  int32_t* boxes = fake<int32_t>(16);
  const int shapes[][4] = {{1, 3, 16, 16}, {3, 3, 48, 48}, {2, 1, 16, 20}, {64, 3, 256, 256}, {1, 1, 1, 1}, {5, 3, 64, 64},
                           {MI355_OCC_MAX_BATCH, 1, 1, 3}, {1, 1, MI355_OCC_MAX_SIDE, MI355_OCC_MAX_SIDE}};
  for (const auto& s : shapes)
    for (int N : {0, 1, MI355_OCC_MAX_BOXES}) {
      EXPECT(ran(occ(x, boxes, N, out, s[0], s[1], s[2], s[3])));
      EXPECT(ran(occ(fake(15, 4), boxes, N, out, s[0], s[1], s[2], s[3])));
      EXPECT(ran(occ(x, fake<int32_t>(16, 4), N, fake(17, 4), s[0], s[1], s[2], s[3])));
    }
  EXPECT(ran(occ(x, nullptr, 0, out, 2, 3, 8, 8)));                                                  // no boxes: a copy
  EXPECT(occ(nullptr, boxes, 1, out, 2, 3, 8, 8) == MI355_EINVAL && says("null x"));
  EXPECT(occ(x, boxes, 1, nullptr, 2, 3, 8, 8) == MI355_EINVAL && says("null out"));
  EXPECT(occ(x, nullptr, 1, out, 2, 3, 8, 8) == MI355_EINVAL && says("null boxes"));
  EXPECT(occ(x, boxes, -1, out, 2, 3, 8, 8) == MI355_EINVAL && says("N=-1"));
  EXPECT(occ(x, boxes, 9, out, 2, 3, 8, 8) == MI355_EINVAL && says("N=9"));
  EXPECT(occ(x, boxes, 1, out, 0, 3, 8, 8) == MI355_EINVAL && says("B=0"));
  EXPECT(occ(x, boxes, 1, out, MI355_OCC_MAX_BATCH + 1, 3, 8, 8) == MI355_EINVAL && says("B="));
  EXPECT(occ(x, boxes, 1, out, 2, 0, 8, 8) == MI355_EINVAL && says("C=0"));
  EXPECT(occ(x, boxes, 1, out, 2, 3, -8, 8) == MI355_EINVAL && says("H=-8"));
  EXPECT(occ(x, boxes, 1, out, 2, 3, 8, 0) == MI355_EINVAL && says("W=0"));
  EXPECT(occ(x, boxes, 1, out, 2, 3, MI355_OCC_MAX_SIDE + 1, 8) == MI355_EINVAL && says("H=4097"));
  EXPECT(occ(x, boxes, 1, out, 1, 0x7fffffff, 4096, 4096) == MI355_EINVAL && says("2^31"));
  EXPECT(occ(x, boxes, 1, out, 1, 128, 4096, 4096) == MI355_EINVAL && says("2^31"));
  EXPECT(occ(fake(15, 2), boxes, 1, out, 2, 3, 8, 8) == MI355_EINVAL && says("aligned"));
  EXPECT(occ(x, boxes, 1, x, 2, 3, 8, 8) == MI355_EINVAL && says("x and out overlap"));
  EXPECT(occ(x, boxes, 1, fake(15, 1024), 2, 3, 8, 8) == MI355_EINVAL && says("x and out overlap"));
  EXPECT(occ(x, fake<int32_t>(17, 64), 1, out, 2, 3, 8, 8) == MI355_EINVAL && says("boxes and out overlap"));
  std::printf("occlude driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

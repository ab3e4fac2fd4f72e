// Host-side exerciser of mi355_softargmax_backward, mi355_bone_prior and mi355_bone_stats_update for the CPU-box sanitizer job
// (tests/test_host_bone.py): built like coord_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined,
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

static int bwd(const float* pred, const float* g_uv, float beta, float* grad, int n, int H, int W) {
  return mi355_softargmax_backward(pred, g_uv, beta, grad, n, H, W, nullptr);
}
static int prior(const float* uv, const float* w, const int* bones, const float* mean, const float* var, const int* seen, float margin,
                 float eps, float coef, float* rows, float* g, int B, int K, int E) {
  return mi355_bone_prior(uv, w, bones, mean, var, seen, margin, eps, coef, rows, g, B, K, E, nullptr);
}
static int stats(const float* kp, const float* w, const int* bones, float* mean, float* var, int* seen, float rho, int B, int K, int E) {
  return mi355_bone_stats_update(kp, w, bones, mean, var, seen, rho, B, K, E, nullptr);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  float *pred = fake(1), *guv = fake(2), *grad = fake(3);

  // ---- soft-arg-max backward: the sides and row counts of tests/test_gpu_bone.py, aligned pointers and pointers one float past a
  //      16-byte boundary, both betas
  const int sides[][2] = {{16, 16}, {32, 32}, {64, 64}, {24, 20}, {6, 10}, {1, 1}, {1, 3}, {63, 65}, {128, 128}};
  for (const auto& s : sides)
    for (int n : {1, 4, 5, 1344})
      for (float beta : {1.f, 100.f}) {
        EXPECT(ran(bwd(pred, guv, beta, grad, n, s[0], s[1])));
        EXPECT(ran(bwd(fake(1, 4), guv, beta, grad, n, s[0], s[1])));
        EXPECT(ran(bwd(pred, fake(2, 4), beta, fake(3, 4), n, s[0], s[1])));
      }
  EXPECT(ran(bwd(pred, guv, 1.f, grad, 1, 46340, 46340)));                                        // H*W just below 2^31
  EXPECT(ran(bwd(pred, guv, 1e-30f, grad, 0x7fffffff, 1, 1)));
  EXPECT(bwd(nullptr, guv, 1.f, grad, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(bwd(pred, nullptr, 1.f, grad, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(bwd(pred, guv, 1.f, nullptr, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(bwd(pred, guv, 1.f, grad, 0, 16, 16) == MI355_EINVAL && says("rows=0"));
  EXPECT(bwd(pred, guv, 1.f, grad, -3, 16, 16) == MI355_EINVAL && says("rows=-3"));
  EXPECT(bwd(pred, guv, 1.f, grad, 4, 0, 16) == MI355_EINVAL && says("H=0"));
  EXPECT(bwd(pred, guv, 1.f, grad, 4, 16, -1) == MI355_EINVAL && says("W=-1"));
  EXPECT(bwd(pred, guv, 1.f, grad, 1, 46341, 46341) == MI355_EINVAL && says("2^31"));
  EXPECT(bwd(pred, guv, 1.f, grad, 1, 0x7fffffff, 0x7fffffff) == MI355_EINVAL && says("2^31"));
  EXPECT(bwd(pred, guv, 0.f, grad, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(bwd(pred, guv, -1.f, grad, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(bwd(pred, guv, inf, grad, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(bwd(pred, guv, nan, grad, 4, 16, 16) == MI355_EINVAL && says("beta"));

  // ---- bone prior and statistics: the batches and tables of the GPU tests and the limits
  float *uv = fake(4), *w = fake(5), *mean = fake(7), *var = fake(8), *rows = fake(10), *g = fake(11);
  int *bones = fake<int>(6), *seen = fake<int>(9);
  const int shapes[][3] = {{1, 21, 20}, {3, 21, 20}, {5, 21, 20}, {64, 21, 20}, {1, 4, 3}, {3, 4, 3}, {5, 4, 3}, {1, 2, 1},
                           {MI355_BONE_MAX_BATCH, MI355_BONE_MAX_JOINTS, MI355_BONE_MAX_BONES}};
  for (const auto& s : shapes)
    for (float margin : {0.f, 1.f}) {
      EXPECT(ran(prior(uv, w, bones, mean, var, seen, margin, 1e-4f, 1.f / s[0], rows, g, s[0], s[1], s[2])));
      EXPECT(ran(prior(uv, nullptr, bones, mean, var, seen, margin, 1e-4f, 0.f, rows, nullptr, s[0], s[1], s[2])));
      EXPECT(ran(prior(fake(4, 4), fake(5, 4), fake<int>(6, 4), fake(7, 4), fake(8, 4), fake<int>(9, 4), margin, 1e-4f, -2.f, fake(10, 4),
                       fake(11, 4), s[0], s[1], s[2])));
      EXPECT(ran(stats(uv, w, bones, mean, var, seen, 0.01f, s[0], s[1], s[2])));
      EXPECT(ran(stats(uv, nullptr, bones, mean, var, seen, margin, s[0], s[1], s[2])));            // rho 0 and 1
    }
  EXPECT(prior(nullptr, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, nullptr, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, bones, nullptr, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, bones, mean, nullptr, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, bones, mean, var, nullptr, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, nullptr, g, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 0, 21, 20) == MI355_EINVAL && says("B=0"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, -1, 21, 20) == MI355_EINVAL && says("B=-1"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, MI355_BONE_MAX_BATCH + 1, 21, 20) == MI355_EINVAL && says("B="));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 1, 20) == MI355_EINVAL && says("K=1"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 33, 20) == MI355_EINVAL && says("K=33"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 0) == MI355_EINVAL && says("E=0"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 21, 33) == MI355_EINVAL && says("E=33"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, 1.f, rows, g, 3, 0x7fffffff, 0x7fffffff) == MI355_EINVAL);
  EXPECT(prior(uv, w, bones, mean, var, seen, -1.f, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("margin"));
  EXPECT(prior(uv, w, bones, mean, var, seen, inf, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("margin"));
  EXPECT(prior(uv, w, bones, mean, var, seen, nan, 1e-4f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("margin"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 0.f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("eps"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, -1.f, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("eps"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, inf, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("eps"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, nan, 1.f, rows, g, 3, 21, 20) == MI355_EINVAL && says("eps"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, inf, rows, g, 3, 21, 20) == MI355_EINVAL && says("coef"));
  EXPECT(prior(uv, w, bones, mean, var, seen, 1.f, 1e-4f, nan, rows, g, 3, 21, 20) == MI355_EINVAL && says("coef"));

  EXPECT(stats(nullptr, w, bones, mean, var, seen, 0.01f, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(stats(uv, w, nullptr, mean, var, seen, 0.01f, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(stats(uv, w, bones, nullptr, var, seen, 0.01f, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(stats(uv, w, bones, mean, nullptr, seen, 0.01f, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(stats(uv, w, bones, mean, var, nullptr, 0.01f, 3, 21, 20) == MI355_EINVAL && says("null"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, 0, 21, 20) == MI355_EINVAL && says("B=0"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, MI355_BONE_MAX_BATCH + 1, 21, 20) == MI355_EINVAL && says("B="));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, 3, 1, 20) == MI355_EINVAL && says("K=1"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, 3, 33, 20) == MI355_EINVAL && says("K=33"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, 3, 21, 0) == MI355_EINVAL && says("E=0"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 0.01f, 3, 21, 33) == MI355_EINVAL && says("E=33"));
  EXPECT(stats(uv, w, bones, mean, var, seen, -0.1f, 3, 21, 20) == MI355_EINVAL && says("rho"));
  EXPECT(stats(uv, w, bones, mean, var, seen, 1.5f, 3, 21, 20) == MI355_EINVAL && says("rho"));
  EXPECT(stats(uv, w, bones, mean, var, seen, nan, 3, 21, 20) == MI355_EINVAL && says("rho"));
  std::printf("bone driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

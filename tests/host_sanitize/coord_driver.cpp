// Host-side exerciser of mi355_coord_heatmap for the CPU-box sanitizer job (tests/test_host_coord.py): built like adam_driver.cpp --
// the HOST pass of every .hip file with -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device
// pointers are fake, well-aligned addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the
// host code under test has run.  The job passes when no sanitizer report aborts the process, every accepted shape reaches the
// launch and every refused argument comes back as MI355_EINVAL with a message that names what is wrong.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static float* fake(size_t i, size_t off = 0) { return reinterpret_cast<float*>(static_cast<uintptr_t>(0x100000000ull + (i << 28) + off)); }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static int go(const float* pred, const float* coord, const float* weight, float beta, float delta, float coef, float* rows, float* grad,
              float* uv, int n, int H, int W) {
  return mi355_coord_heatmap(pred, coord, weight, beta, delta, coef, rows, grad, uv, n, H, W, nullptr);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  float *pred = fake(1), *coord = fake(2), *weight = fake(3), *rows = fake(4), *grad = fake(5), *uv = fake(6);

  // ---- accepted shapes: the sides and row counts of tests/test_gpu_coord.py, every nullable operand present and absent, aligned
  //      pointers and pointers one float past a 16-byte boundary, both deltas and betas
  const int sides[][2] = {{16, 16}, {32, 32}, {64, 64}, {24, 20}, {6, 10}, {4, 8}, {1, 1}, {1, 3}, {63, 65}, {128, 128}};
  for (const auto& s : sides)
    for (int n : {1, 4, 5, 1344})
      for (float delta : {0.f, 1.f})
        for (float beta : {1.f, 100.f}) {
          EXPECT(ran(go(pred, coord, weight, beta, delta, 1.f / n, rows, grad, uv, n, s[0], s[1])));
          EXPECT(ran(go(pred, coord, nullptr, beta, delta, 1.f / n, rows, nullptr, uv, n, s[0], s[1])));
          EXPECT(ran(go(pred, coord, weight, beta, delta, 1.f / n, rows, grad, nullptr, n, s[0], s[1])));
          EXPECT(ran(go(pred, coord, nullptr, beta, delta, 0.f, rows, nullptr, nullptr, n, s[0], s[1])));
          EXPECT(ran(go(fake(1, 4), coord, weight, beta, delta, -2.f, rows, grad, uv, n, s[0], s[1])));
          EXPECT(ran(go(pred, fake(2, 4), fake(3, 4), beta, delta, 1.f, fake(4, 4), fake(5, 4), fake(6, 4), n, s[0], s[1])));
        }
  EXPECT(ran(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 1, 46340, 46340)));          // H*W just below 2^31
  EXPECT(ran(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 1, 1, 0x7fffffff)));
  EXPECT(ran(go(pred, coord, weight, 1e-30f, 1e30f, 1e30f, rows, grad, uv, 0x7fffffff, 1, 1)));

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(go(nullptr, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(go(pred, nullptr, weight, 1.f, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, nullptr, grad, uv, 4, 16, 16) == MI355_EINVAL && says("null"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 0, 16, 16) == MI355_EINVAL && says("rows=0"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, -3, 16, 16) == MI355_EINVAL && says("rows=-3"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 4, 0, 16) == MI355_EINVAL && says("H=0"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 4, 16, -1) == MI355_EINVAL && says("W=-1"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 1, 46341, 46341) == MI355_EINVAL && says("2^31"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 1, 65536, 32768) == MI355_EINVAL && says("2^31"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, 1.f, rows, grad, uv, 1, 0x7fffffff, 0x7fffffff) == MI355_EINVAL && says("2^31"));
  EXPECT(go(pred, coord, weight, 0.f, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(go(pred, coord, weight, -1.f, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(go(pred, coord, weight, inf, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(go(pred, coord, weight, nan, 1.f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("beta"));
  EXPECT(go(pred, coord, weight, 1.f, -0.5f, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("delta"));
  EXPECT(go(pred, coord, weight, 1.f, inf, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("delta"));
  EXPECT(go(pred, coord, weight, 1.f, nan, 1.f, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("delta"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, inf, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("coef"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, -inf, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("coef"));
  EXPECT(go(pred, coord, weight, 1.f, 1.f, nan, rows, grad, uv, 4, 16, 16) == MI355_EINVAL && says("coef"));
  std::printf("coord driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

// Host-side exerciser of the MX inference entry points (mi355_conv_fwd_mx_act / mi355_conv_dgrad_mx_act) for the CPU-box
// sanitizer job (tests/test_host_mx_act.py): built like driver.cpp -- the HOST pass of every .hip file with
// -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned
// addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run
// (argument checks, phase / tap tables of the transposed conv, build choice, tile grid, label).  The job passes when no
// sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static void* fake(size_t i) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + (i << 28))); }

static mi355_conv_desc desc(int N, int H, int W, int Ci, int Co, int k, int s, int p) {
  mi355_conv_desc d; std::memset(&d, 0, sizeof(d));
  d.N = N; d.Hi = H; d.Wi = W; d.Ci = Ci; d.Co = Co; d.kh = d.kw = k; d.stride = s; d.pad = p; d.dtype = MI355_FP8;
  d.Ho = (H + 2 * p - k) / s + 1; d.Wo = (W + 2 * p - k) / s + 1;
  return d;
}
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }

int main() {
  // ---- the case geometries of tests/test_gpu_mx_eval.py and the neck / head layers of the pose network at B = 64
  struct G { int N, H, W, Ci, Co, k, s, p; };
  const G geo[] = {{2, 8, 8, 128, 128, 3, 1, 1}, {3, 9, 11, 128, 64, 3, 1, 1}, {2, 8, 8, 256, 128, 3, 2, 1}, {1, 8, 8, 128, 128, 4, 2, 1},
                   {5, 60, 60, 128, 128, 3, 1, 1}, {10, 60, 58, 128, 256, 3, 1, 1}, {64, 64, 64, 256, 256, 3, 1, 1},
                   {64, 16, 16, 256, 2048, 4, 2, 1}, {64, 32, 32, 256, 256, 4, 2, 1}, {64, 64, 64, 256, 256, 4, 2, 1}};
  for (const G& g : geo) {
    const mi355_conv_desc d = desc(g.N, g.H, g.W, g.Ci, g.Co, g.k, g.s, g.p);
    for (int relu = 0; relu <= 1; ++relu)
      for (int res = 0; res <= 1; ++res)
        for (int copy = 0; copy <= 1; ++copy) {
          if (copy && g.Co % 32) continue;
          const int rc = mi355_conv_fwd_mx_act(&d, fake(1), fake(2), fake(3), fake(4), (const float*)fake(5), res ? fake(6) : nullptr, relu,
                                               fake(7), copy ? fake(8) : nullptr, copy ? fake(9) : nullptr, nullptr);
          EXPECT(ran(rc));
        }
    if (g.Co % 128 == 0 && (g.Co & (g.Co - 1)) == 0) {      // dgrad form: Co is the contracted axis
      for (int relu = 0; relu <= 1; ++relu)
        for (int copy = 0; copy <= 1; ++copy) {
          const int rc = mi355_conv_dgrad_mx_act(&d, fake(7), fake(9), fake(3), fake(4), relu ? (const float*)fake(5) : nullptr, relu, fake(1),
                                                 copy ? fake(8) : nullptr, copy ? fake(2) : nullptr, nullptr);
          EXPECT(ran(rc));
        }
    }
  }
  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  {
    const mi355_conv_desc d = desc(2, 8, 8, 128, 128, 3, 1, 1);
    const float* bias = (const float*)fake(5);
    EXPECT(mi355_conv_fwd_mx_act(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 1, fake(7), fake(8), nullptr, nullptr) == MI355_EINVAL);   // y8 without sy
    EXPECT(mi355_conv_fwd_mx_act(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 1, fake(7), nullptr, fake(9), nullptr) == MI355_EINVAL);   // sy without y8
    EXPECT(mi355_conv_fwd_mx_act(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 1, nullptr, nullptr, nullptr, nullptr) == MI355_EINVAL);   // null y
    EXPECT(mi355_conv_fwd_mx_act(&d, fake(1), nullptr, fake(3), fake(4), bias, nullptr, 1, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);   // null sx
    EXPECT(mi355_conv_fwd_mx_act(nullptr, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 1, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);
    EXPECT(mi355_conv_fwd_mx_act(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 1, fake(7), (char*)fake(8) + 4, fake(9), nullptr) == MI355_EINVAL);   // misaligned y8
    mi355_conv_desc b = desc(2, 8, 8, 128, 72, 3, 1, 1);                 // Co = 72: fine without a copy, refused with one
    EXPECT(ran(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr)));
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), fake(8), fake(9), nullptr) == MI355_EINVAL);
    b = desc(2, 8, 8, 128, 68, 3, 1, 1);                                  // Co not a multiple of 8
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);
    b = desc(2, 8, 8, 64, 128, 3, 1, 1);                                  // contracted channels below one K tile
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);
    b = desc(2, 8, 8, 384, 128, 3, 1, 1);                                 // ... not a power of two
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);
    b = d; b.dtype = MI355_BF16;
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);
    b = d; b.Ho += 1;
    EXPECT(mi355_conv_fwd_mx_act(&b, fake(1), fake(2), fake(3), fake(4), bias, nullptr, 0, fake(7), nullptr, nullptr, nullptr) == MI355_EINVAL);

    const mi355_conv_desc t = desc(1, 8, 8, 128, 128, 4, 2, 1);
    EXPECT(mi355_conv_dgrad_mx_act(&t, fake(7), fake(9), fake(3), fake(4), bias, 1, fake(1), fake(8), nullptr, nullptr) == MI355_EINVAL);          // dx8 without sdx
    EXPECT(mi355_conv_dgrad_mx_act(&t, fake(7), fake(9), fake(3), fake(4), bias, 1, nullptr, nullptr, nullptr, nullptr) == MI355_EINVAL);          // null dx
    EXPECT(mi355_conv_dgrad_mx_act(&t, fake(7), fake(9), nullptr, fake(4), bias, 1, fake(1), nullptr, nullptr, nullptr) == MI355_EINVAL);          // null pack
    b = desc(1, 8, 8, 72, 128, 4, 2, 1);                                  // Ci = 72 output channels: no copy
    EXPECT(ran(mi355_conv_dgrad_mx_act(&b, fake(7), fake(9), fake(3), fake(4), bias, 1, fake(1), nullptr, nullptr, nullptr)));
    EXPECT(mi355_conv_dgrad_mx_act(&b, fake(7), fake(9), fake(3), fake(4), bias, 1, fake(1), fake(8), fake(2), nullptr) == MI355_EINVAL);
    b = desc(1, 8, 8, 128, 192, 4, 2, 1);                                 // contracted Co not a power of two
    EXPECT(mi355_conv_dgrad_mx_act(&b, fake(7), fake(9), fake(3), fake(4), bias, 1, fake(1), nullptr, nullptr, nullptr) == MI355_EINVAL);
    b = desc(2, 8, 8, 128, 128, 1, 2, 0);                                 // 1x1 / stride 2: three of four output parities have no tap
    EXPECT(mi355_conv_dgrad_mx_act(&b, fake(7), fake(9), fake(3), fake(4), bias, 1, fake(1), nullptr, nullptr, nullptr) == MI355_EINVAL);
    // the statistics-carrying MX entries still refuse what they refused, and take no ReLU
    int ns = -1;
    EXPECT(mi355_conv_fwd_mx(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, fake(7), (float*)fake(10), 1 << 20, nullptr, nullptr) == MI355_EINVAL);
    EXPECT(ran(mi355_conv_fwd_mx(&d, fake(1), fake(2), fake(3), fake(4), bias, nullptr, fake(7), (float*)fake(10), 1 << 20, &ns, nullptr)));
  }
  std::printf("mx act driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

// Host-side exerciser of the prototype-alignment entry points (mi355_proto_pool / mi355_proto_update / mi355_proto_kl /
// mi355_proto_scatter) for the CPU-box sanitizer job (tests/test_host_proto.py): built like jfa_driver.cpp -- the HOST pass of
// every .hip file with -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers are
// fake, well-aligned addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code
// under test has run.  The job passes when no sanitizer report aborts the process and every invalid call is refused with
// MI355_EINVAL, naming what is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static void* fake(size_t i, size_t off = 0) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + (i << 28) + off)); }
static float* ff(size_t i, size_t off = 0) { return reinterpret_cast<float*>(fake(i, off)); }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static int pool(int B, int K, int C, int H, int W, int r = 6, int ref = 1, int dt = MI355_BF16) {
  return mi355_proto_pool(fake(1), ff(2), ff(3), B, K, C, H, W, r, ref, dt, nullptr);
}
static int upd(int B, int K, int C) { return mi355_proto_update(ff(1), ff(2), ff(3), ff(4), B, K, C, nullptr); }
static int kl(int K, int C, int mode = MI355_PROTO_KL, float coef = 1.f, int grads = 3) {
  return mi355_proto_kl(ff(1), ff(2), ff(3), (grads & 1) ? ff(4) : nullptr, (grads & 2) ? ff(5) : nullptr, K, C, mode, coef, nullptr);
}
static int scat(int acc, int B, int K, int C, int H, int W, int r = 6, int ref = 0, int dt = MI355_BF16) {
  return mi355_proto_scatter(ff(1), ff(2), ff(3), fake(4), acc, B, K, C, H, W, r, ref, dt, nullptr);
}

int main() {
  // ---- the shapes of tests/test_gpu_proto.py and the workload's: every dtype, indexing and mode
  for (int dt : {MI355_F32, MI355_BF16})
    for (int ref = 0; ref < 2; ++ref)
      for (int C : {8, 24, 256, 264, 2048})
        for (int K : {1, 21, 32})
          for (int B : {1, 2, 3, 64}) {
            EXPECT(ran(pool(B, K, C, 64, 64, 6, ref, dt)) && ran(pool(B, K, C, 16, 16, 16, ref, dt)) && ran(pool(B, K, C, 32, 48, 1, ref, dt)));
            for (int acc = 0; acc < 2; ++acc)
              EXPECT(ran(scat(acc, B, K, C, 64, 64, 6, ref, dt)) && ran(scat(acc, B, K, C, 16, 16, 16, ref, dt)) && ran(scat(acc, B, K, C, 32, 48, 1, ref, dt)));
          }
  for (int C : {8, 24, 256, 264, 2048})
    for (int K : {1, 3, 4, 5, 21, 32}) {
      for (int B : {1, 2, 3, 64, 65535}) EXPECT(ran(upd(B, K, C)));
      for (int mode : {MI355_PROTO_KL, MI355_PROTO_SOFTKL})
        for (int grads = 0; grads < 4; ++grads) EXPECT(ran(kl(K, C, mode, 0.5f / K, grads)));
    }
  EXPECT(ran(pool(65535, 32, 8, 1, 1)) && ran(pool(1, 1, 8, 4096, 4096)) && ran(scat(1, 1, 1, 8, 4096, 4096)) && ran(kl(0x7fffffff, 8)));
  EXPECT(ran(pool(2, 21, 256, 64, 64, 1 << 20)) && ran(kl(21, 256, MI355_PROTO_SOFTKL, 0.f)) && ran(kl(21, 256, MI355_PROTO_KL, -1.f)));
  EXPECT(ran(upd(2, 32, 1 << 24)));

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(mi355_proto_pool(nullptr, ff(2), ff(3), 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_pool(fake(1), nullptr, ff(3), 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_pool(fake(1), ff(2), nullptr, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_scatter(nullptr, ff(2), ff(3), fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_scatter(ff(1), nullptr, ff(3), fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_scatter(ff(1), ff(2), nullptr, fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_scatter(ff(1), ff(2), ff(3), nullptr, 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_update(nullptr, ff(2), ff(3), ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_update(ff(1), nullptr, ff(3), ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_update(ff(1), ff(2), nullptr, ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_update(ff(1), ff(2), ff(3), nullptr, 2, 21, 256, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_update(ff(1), ff(2), ff(3), ff(2), 2, 21, 256, nullptr) == MI355_EINVAL && says("memory itself"));
  EXPECT(mi355_proto_kl(nullptr, ff(2), ff(3), ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_kl(ff(1), nullptr, ff(3), ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_proto_kl(ff(1), ff(2), nullptr, ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("null"));
  for (size_t off : {2, 4, 8}) {          // one element (and less) off a 16-byte boundary
    EXPECT(mi355_proto_pool(fake(1, off), ff(2), ff(3), 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_pool(fake(1), ff(2), ff(3, off), 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_scatter(ff(1, off), ff(2), ff(3), fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_scatter(ff(1), ff(2), ff(3), fake(4, off), 1, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_update(ff(1, off), ff(2), ff(3), ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_update(ff(1), ff(2, off), ff(3), ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_update(ff(1), ff(2), ff(3), ff(4, off), 2, 21, 256, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_kl(ff(1, off), ff(2), ff(3), ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_kl(ff(1), ff(2, off), ff(3), ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_kl(ff(1), ff(2), ff(3), ff(4, off), ff(5), 21, 256, 1, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
    EXPECT(mi355_proto_kl(ff(1), ff(2), ff(3), ff(4), ff(5, off), 21, 256, 1, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
  }
  EXPECT(mi355_proto_pool(fake(1), ff(2, 2), ff(3), 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_proto_scatter(ff(1), ff(2, 2), ff(3), fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_proto_scatter(ff(1), ff(2), ff(3, 2), fake(4), 0, 2, 21, 256, 64, 64, 6, 1, 1, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_proto_update(ff(1), ff(2), ff(3, 2), ff(4), 2, 21, 256, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_proto_kl(ff(1), ff(2), ff(3, 2), ff(4), ff(5), 21, 256, 0, 1.f, nullptr) == MI355_EINVAL && says("aligned"));
  for (int which = 0; which < 2; ++which) {
    auto call = [&](int B, int K, int C, int H, int W, int r = 6, int dt = MI355_BF16) {
      return which ? scat(1, B, K, C, H, W, r, 0, dt) : pool(B, K, C, H, W, r, 1, dt);
    };
    EXPECT(call(0, 21, 256, 64, 64) == MI355_EINVAL && says("B=0"));
    EXPECT(call(-2, 21, 256, 64, 64) == MI355_EINVAL && says("B=-2"));
    EXPECT(call(65536, 21, 256, 64, 64) == MI355_EINVAL && says("B=65536"));
    EXPECT(call(2, 0, 256, 64, 64) == MI355_EINVAL && says("K=0"));
    EXPECT(call(2, 33, 256, 64, 64) == MI355_EINVAL && says("K=33"));
    EXPECT(call(2, -1, 256, 64, 64) == MI355_EINVAL && says("K=-1"));
    EXPECT(call(2, 21, 0, 64, 64) == MI355_EINVAL && says("C=0"));
    EXPECT(call(2, 21, 4, 64, 64) == MI355_EINVAL && says("C=4"));
    EXPECT(call(2, 21, 12, 64, 64) == MI355_EINVAL && says("C=12"));
    EXPECT(call(2, 21, -8, 64, 64) == MI355_EINVAL && says("C=-8"));
    EXPECT(call(2, 21, 0x7ffffff8, 64, 64) == MI355_EINVAL && says("too large"));
    EXPECT(call(2, 21, 256, 0, 64) == MI355_EINVAL && says("H=0"));
    EXPECT(call(2, 21, 256, 64, 0) == MI355_EINVAL && says("W=0"));
    EXPECT(call(2, 21, 256, -64, 64) == MI355_EINVAL && says("H=-64"));
    EXPECT(call(2, 21, 256, 65536, 65536) == MI355_EINVAL && says("H=65536"));
    EXPECT(call(2, 21, 256, 0x7fffffff, 0x7fffffff) == MI355_EINVAL && says("W="));
    EXPECT(call(2, 21, 256, 64, 64, 0) == MI355_EINVAL && says("radius=0"));
    EXPECT(call(2, 21, 256, 64, 64, -6) == MI355_EINVAL && says("radius=-6"));
    EXPECT(call(2, 21, 256, 64, 64, 0x7fffffff) == MI355_EINVAL && says("radius="));
    EXPECT(call(2, 21, 256, 64, 64, 6, MI355_FP8) == MI355_EINVAL && says("dtype=2"));
    EXPECT(call(2, 21, 256, 64, 64, 6, -1) == MI355_EINVAL && says("dtype=-1"));
  }
  EXPECT(upd(0, 21, 256) == MI355_EINVAL && says("B=0"));
  EXPECT(upd(65536, 21, 256) == MI355_EINVAL && says("B=65536"));
  EXPECT(upd(2, 0, 256) == MI355_EINVAL && says("K=0"));
  EXPECT(upd(2, 33, 256) == MI355_EINVAL && says("K=33"));
  EXPECT(upd(2, 21, 12) == MI355_EINVAL && says("C=12"));
  EXPECT(upd(2, 21, 0) == MI355_EINVAL && says("C=0"));
  EXPECT(upd(2, 21, 0x7ffffff8) == MI355_EINVAL && says("C="));
  EXPECT(kl(0, 256) == MI355_EINVAL && says("K=0"));
  EXPECT(kl(-21, 256) == MI355_EINVAL && says("K=-21"));
  EXPECT(kl(21, 0) == MI355_EINVAL && says("C=0"));
  EXPECT(kl(21, 12) == MI355_EINVAL && says("C=12"));
  EXPECT(kl(21, 260) == MI355_EINVAL && says("C=260"));
  EXPECT(kl(21, 256, 2) == MI355_EINVAL && says("mode=2"));
  EXPECT(kl(21, 256, -1) == MI355_EINVAL && says("mode=-1"));
  EXPECT(kl(21, 256, 0, NAN) == MI355_EINVAL && says("coef"));
  EXPECT(kl(21, 256, 1, INFINITY) == MI355_EINVAL && says("coef"));
  std::printf("proto driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

// Host-side exerciser of the gradient-norm clipping entry points (mi355_grad_sumsq_batched / mi355_grad_clip_coef /
// mi355_sgd_nesterov_clipped) for the CPU-box sanitizer job (tests/test_host_gradclip.py): built like proto_driver.cpp -- the HOST
// pass of every .hip file with -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers
// are fake, well-aligned addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code
// under test has run.  The job passes when no sanitizer report aborts the process and every invalid call is refused with
// MI355_EINVAL, naming what is wrong.
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

static int sumsq(int count, int blocks) {
  return mi355_grad_sumsq_batched(reinterpret_cast<const mi355_gn_item*>(fake(1)), count, blocks, reinterpret_cast<double*>(fake(2)), nullptr);
}
static int coef(int blocks) {
  return mi355_grad_clip_coef(reinterpret_cast<const double*>(fake(2)), blocks, reinterpret_cast<mi355_clip_rec*>(fake(3)), nullptr);
}
static int sgd(long n, int nesterov = 1, float wd = 1e-4f, bool lowp = false) {
  return mi355_sgd_nesterov_clipped(ff(1), ff(2), ff(3), n, ff(4), reinterpret_cast<const mi355_clip_rec*>(fake(5)), 0.9f, wd, nesterov,
                                    lowp ? fake(6) : nullptr, nullptr);
}
static int blocks_of(long n) { return (int)((n + MI355_GN_CHUNK - 1) / MI355_GN_CHUNK); }

int main() {
  static_assert(sizeof(mi355_gn_item) == 24 && sizeof(mi355_clip_rec) == 32, "record layouts of mi355/ops.py");
  // ---- the shapes of tests/test_gpu_gradclip.py and the workload's
  const long C = MI355_GN_CHUNK;
  const long lens[] = {1, 3, 4, 5, C - 4, C, C + 4, 2 * C + 8};
  int all = 0;
  for (long n : lens) { EXPECT(ran(sumsq(1, blocks_of(n))) && ran(coef(blocks_of(n)))); all += blocks_of(n); }
  EXPECT(all == 11 &&ran(sumsq(8, all)) && ran(coef(all)));
  EXPECT(ran(sumsq(3, blocks_of(100000) + blocks_of(150001) + blocks_of(50003))) && ran(coef(19)));
  EXPECT(ran(sumsq(170, 1700)) && ran(coef(1700)) && ran(sumsq(1, 1)) && ran(coef(1)) && ran(sumsq(1, 0x7fffffff)) && ran(coef(0x7fffffff)));
  for (long n : {4L, 5L, 1023L, 4100L, 1L, 25000000L, 1L << 32})
    for (int nesterov = 0; nesterov < 2; ++nesterov)
      for (float wd : {0.f, 1e-4f})
        for (int lowp = 0; lowp < 2; ++lowp) EXPECT(ran(sgd(n, nesterov, wd, lowp != 0)));

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(mi355_grad_sumsq_batched(nullptr, 1, 1, reinterpret_cast<double*>(fake(2)), nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_grad_sumsq_batched(reinterpret_cast<const mi355_gn_item*>(fake(1)), 1, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(sumsq(0, 1) == MI355_EINVAL && says("count=0"));
  EXPECT(sumsq(-1, 1) == MI355_EINVAL && says("count=-1"));
  EXPECT(sumsq(1, 0) == MI355_EINVAL && says("total_blocks=0"));
  EXPECT(sumsq(1, -7) == MI355_EINVAL && says("total_blocks=-7"));
  EXPECT(sumsq(9, 8) == MI355_EINVAL && says("total_blocks=8"));
  EXPECT(mi355_grad_sumsq_batched(reinterpret_cast<const mi355_gn_item*>(fake(1, 4)), 1, 1, reinterpret_cast<double*>(fake(2)), nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_grad_sumsq_batched(reinterpret_cast<const mi355_gn_item*>(fake(1)), 1, 1, reinterpret_cast<double*>(fake(2, 4)), nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_grad_clip_coef(nullptr, 1, reinterpret_cast<mi355_clip_rec*>(fake(3)), nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_grad_clip_coef(reinterpret_cast<const double*>(fake(2)), 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(coef(0) == MI355_EINVAL && says("total_blocks=0"));
  EXPECT(coef(-1) == MI355_EINVAL && says("total_blocks=-1"));
  EXPECT(mi355_grad_clip_coef(reinterpret_cast<const double*>(fake(2, 4)), 1, reinterpret_cast<mi355_clip_rec*>(fake(3)), nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_grad_clip_coef(reinterpret_cast<const double*>(fake(2)), 1, reinterpret_cast<mi355_clip_rec*>(fake(3, 4)), nullptr) == MI355_EINVAL && says("aligned"));
  const mi355_clip_rec* rec = reinterpret_cast<const mi355_clip_rec*>(fake(5));
  EXPECT(mi355_sgd_nesterov_clipped(nullptr, ff(2), ff(3), 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_sgd_nesterov_clipped(ff(1), nullptr, ff(3), 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2), nullptr, 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2), ff(3), 8, nullptr, rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2), ff(3), 8, ff(4), nullptr, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(sgd(0) == MI355_EINVAL && says("n=0"));
  EXPECT(sgd(-4) == MI355_EINVAL && says("n=-4"));
  for (size_t off : {4, 8, 12}) {          // one element (and more) off a 16-byte boundary
    EXPECT(mi355_sgd_nesterov_clipped(ff(1, off), ff(2), ff(3), 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("16-byte aligned"));
    EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2, off), ff(3), 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("16-byte aligned"));
    EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2), ff(3, off), 8, ff(4), rec, 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("16-byte aligned"));
  }
  EXPECT(mi355_sgd_nesterov_clipped(ff(1), ff(2), ff(3), 8, ff(4), reinterpret_cast<const mi355_clip_rec*>(fake(5, 4)), 0.9f, 0.f, 1, nullptr, nullptr) == MI355_EINVAL && says("8-byte aligned"));
  std::printf("gradclip driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

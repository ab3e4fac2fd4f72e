// Host-side exerciser of mi355_render_hands and mi355_hand_rec_size for the CPU-box sanitizer job (tests/test_host_render.py): built
// like warp_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined, linked with this program.  No GPU is
// needed or used: device pointers are fake, well-aligned addresses that the host never dereferences (mean3 / inv_std3 are real host
// arrays: the entry point reads them), and every launch fails in the HIP runtime AFTER the host code under test has run.  The job
// passes when no sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL, naming the argument.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static char* fp(size_t i, size_t off = 0) { return reinterpret_cast<char*>(static_cast<uintptr_t>(0x100000000ull + (i << 44))) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static const float g_mean[3] = {0.485f, 0.456f, 0.406f}, g_inv_std[3] = {4.3668122f, 4.4642859f, 4.4444447f};

struct Render { char *recs, *out, *ema, *ids; int B, S; const float *mean, *inv_std; };
static Render ok(int B = 3, int S = 32, bool ema = true, bool ids = true) {
  return Render{fp(1), fp(2), ema ? fp(3) : nullptr, ids ? fp(4) : nullptr, B, S, g_mean, g_inv_std};
}
static int run(const Render& a) {
  return mi355_render_hands((const mi355_hand_rec*)a.recs, (float*)a.out, (float*)a.ema, (unsigned char*)a.ids, a.B, a.S, a.mean, a.inv_std, nullptr);
}

int main() {
  static_assert(sizeof(mi355_hand_rec) == 480 && sizeof(mi355_hand_rec) % 16 == 0, "120 words");
  EXPECT(mi355_hand_rec_size() == sizeof(mi355_hand_rec));
  // ---- the shapes of tests/test_gpu_render.py, the flagship batch and the extremes, with each nullable output absent in turn
  struct { int B, S; } shapes[] = {{3, 16}, {3, 32}, {3, 48}, {3, 64}, {64, 256}, {1, 16}, {1, MI355_RENDER_MAX_SIDE}, {4096, MI355_RENDER_MAX_SIDE}};
  for (auto& s : shapes)
    for (bool ema : {true, false})
      for (bool ids : {true, false})
        EXPECT(ran(run(ok(s.B, s.S, ema, ids))));
  for (int S = 16; S <= MI355_RENDER_MAX_SIDE; S += 16) EXPECT(ran(run(ok(2, S))));
  const long px = 3L * 32 * 32, nout = 12 * px, nrec = 480L * 3;
  { Render a = ok(); a.out = a.recs + nrec; a.ema = a.out + nout; a.ids = a.ema + nout; EXPECT(ran(run(a))); }       // touching is not overlapping
  { Render a = ok(); a.recs = a.ids + px + 16; EXPECT(ran(run(a))); }

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  { Render a = ok(); a.recs = nullptr; EXPECT(run(a) == MI355_EINVAL && says("recs is null")); }
  { Render a = ok(); a.out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("out is null")); }
  { Render a = ok(); a.mean = nullptr; EXPECT(run(a) == MI355_EINVAL && says("mean3")); }
  { Render a = ok(); a.inv_std = nullptr; EXPECT(run(a) == MI355_EINVAL && says("inv_std3")); }
  EXPECT(run(ok(0)) == MI355_EINVAL && says("B=0"));
  EXPECT(run(ok(-2)) == MI355_EINVAL && says("B=-2"));
  for (int S : {0, -16, 8, 15, 17, 24, 100, 520, 528, 1024, 0x7fffffff}) {
    char want[32];
    std::snprintf(want, sizeof(want), "S=%d", S);
    EXPECT(run(ok(3, S)) == MI355_EINVAL && says(want));
  }
  EXPECT(run(ok(0x7fffffff, MI355_RENDER_MAX_SIDE)) == MI355_EINVAL && says("too large"));
  EXPECT(run(ok(0x7fffffff / 256 + 1, MI355_RENDER_MAX_SIDE)) == MI355_EINVAL && says("too large"));
  EXPECT(ran(run(ok(0x7fffffff / 256, MI355_RENDER_MAX_SIDE, false, false))));                                          // the largest grid
  EXPECT(ran(run(ok(0x7fffffff, 16))));
  for (size_t off : {(size_t)1, (size_t)4, (size_t)8}) {
    { Render a = ok(); a.recs += off; EXPECT(run(a) == MI355_EINVAL && says("recs must be 16-byte aligned")); }
    { Render a = ok(); a.out += off; EXPECT(run(a) == MI355_EINVAL && says("out must be 16-byte aligned")); }
    { Render a = ok(); a.ema += off; EXPECT(run(a) == MI355_EINVAL && says("out_ema must be 16-byte aligned")); }
  }
  for (size_t off : {(size_t)1, (size_t)2, (size_t)3}) { Render a = ok(); a.ids += off; EXPECT(run(a) == MI355_EINVAL && says("ids must be 4-byte aligned")); }
  { Render a = ok(); a.ids += 4; EXPECT(ran(run(a))); }
  { Render a = ok(); a.out = a.recs; EXPECT(run(a) == MI355_EINVAL && says("recs and out overlap")); }
  { Render a = ok(); a.out = a.recs + nrec - 16; EXPECT(run(a) == MI355_EINVAL && says("recs and out overlap")); }
  { Render a = ok(); a.recs = a.ema + nout - 16; EXPECT(run(a) == MI355_EINVAL && says("recs and out_ema overlap")); }
  { Render a = ok(); a.recs = a.ids + px - 16; EXPECT(run(a) == MI355_EINVAL && says("recs and ids overlap")); }
  { Render a = ok(); a.ema = a.out; EXPECT(run(a) == MI355_EINVAL && says("out and out_ema overlap")); }
  { Render a = ok(); a.ema = a.out + nout - 16; EXPECT(run(a) == MI355_EINVAL && says("out and out_ema overlap")); }
  { Render a = ok(); a.ids = a.out + nout - 4; EXPECT(run(a) == MI355_EINVAL && says("out and ids overlap")); }
  { Render a = ok(); a.ids = a.ema; EXPECT(run(a) == MI355_EINVAL && says("out_ema and ids overlap")); }
  { Render a = ok(3, 32, false, true); a.ids = a.out + 64; EXPECT(run(a) == MI355_EINVAL && says("out and ids overlap")); }
  std::printf("render driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

// Host-side exerciser of the mean-teacher entry points (mi355_bn_fold_batched / mi355_mse_heatmap) for the CPU-box sanitizer
// job (tests/test_host_teacher.py): built like driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined,
// linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned addresses that the host never
// dereferences (the host copy of the record table is real memory: that is what the argument checks read), and every launch fails
// in the HIP runtime AFTER the host code under test has run.  The job passes when no sanitizer report aborts the process and
// every invalid call is refused with MI355_EINVAL, naming what is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static void* fake(size_t i) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + (i << 28))); }
static float* ff(size_t i, size_t off = 0) { return reinterpret_cast<float*>(fake(i)) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static mi355_fold_item item(size_t slot, int O, int T, int I, int axis, bool bias, int blk0) {
  mi355_fold_item it; std::memset(&it, 0, sizeof(it));
  it.w = ff(slot); it.gamma = ff(slot, 1 << 20); it.beta = ff(slot, 2 << 20); it.mean = ff(slot, 3 << 20); it.var = ff(slot, 4 << 20);
  it.conv_bias = bias ? ff(slot, 5 << 20) : nullptr;
  it.out_w = ff(slot, 6 << 20); it.out_bias = ff(slot, 7 << 20);
  it.eps = 1e-5f; it.O = O; it.T = T; it.I = I; it.axis = axis; it.blk0 = blk0;
  return it;
}
static int blocks(const mi355_fold_item& it) { return (int)(((long)it.O * it.T * it.I + MI355_FOLD_CHUNK - 1) / MI355_FOLD_CHUNK); }

int main() {
  // ---- the table of tests/test_gpu_mt.py, then the layers of a ResNet-50 pose teacher
  struct S { int O, T, I, axis; bool bias; };
  const S small[] = {{1, 1, 1, 0, false}, {5, 9, 3, 0, true}, {4, 16, 7, 1, false}, {64, 1, 64, 0, true}, {33, 31, 1, 0, false},
                     {41, 5, 5, 1, true}, {64, 49, 3, 0, false}, {2048, 16, 256, 1, false}, {512, 9, 512, 0, false}};
  std::vector<mi355_fold_item> tab;
  int blk = 0;
  for (size_t i = 0; i < sizeof(small) / sizeof(small[0]); ++i) {
    tab.push_back(item(i + 1, small[i].O, small[i].T, small[i].I, small[i].axis, small[i].bias, blk));
    blk += blocks(tab.back());
  }
  const mi355_fold_item* dev = (const mi355_fold_item*)fake(40);
  EXPECT(ran(mi355_bn_fold_batched(tab.data(), dev, (int)tab.size(), blk, nullptr)));
  EXPECT(ran(mi355_bn_fold_batched(tab.data(), dev, 1, blocks(tab[0]), nullptr)));
  {   // 4-byte-aligned, not 16-byte-aligned views are fine
    std::vector<mi355_fold_item> t2(tab.begin(), tab.begin() + 2);
    t2[1].w = ff(2, 1); t2[1].out_w = ff(2, (6 << 20) + 3); t2[1].out_bias = ff(2, (7 << 20) + 1);
    EXPECT(ran(mi355_bn_fold_batched(t2.data(), dev, 2, blocks(t2[0]) + blocks(t2[1]), nullptr)));
  }
  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(mi355_bn_fold_batched(nullptr, dev, 1, 1, nullptr) == MI355_EINVAL);
  EXPECT(mi355_bn_fold_batched(tab.data(), nullptr, 1, 1, nullptr) == MI355_EINVAL);
  EXPECT(mi355_bn_fold_batched(tab.data(), dev, 0, 1, nullptr) == MI355_EINVAL);
  EXPECT(mi355_bn_fold_batched(tab.data(), dev, 1, 0, nullptr) == MI355_EINVAL);
  EXPECT(mi355_bn_fold_batched(tab.data(), dev, (int)tab.size(), blk + 1, nullptr) == MI355_EINVAL && says("total_blocks"));
  EXPECT(mi355_bn_fold_batched(tab.data(), dev, (int)tab.size(), blk - 1, nullptr) == MI355_EINVAL && says("total_blocks"));
  for (int field = 0; field < 7; ++field) {          // every required pointer
    std::vector<mi355_fold_item> t2(tab.begin(), tab.begin() + 3);
    mi355_fold_item& it = t2[1];
    switch (field) {
      case 0: it.w = nullptr; break;       case 1: it.gamma = nullptr; break;  case 2: it.beta = nullptr; break;
      case 3: it.mean = nullptr; break;    case 4: it.var = nullptr; break;    case 5: it.out_w = nullptr; break;
      default: it.out_bias = nullptr; break;
    }
    EXPECT(mi355_bn_fold_batched(t2.data(), dev, 3, blocks(t2[0]) + blocks(t2[1]) + blocks(t2[2]), nullptr) == MI355_EINVAL && says("null"));
  }
  for (int axis : {-1, 2, 7}) {
    std::vector<mi355_fold_item> t2(tab.begin(), tab.begin() + 2);
    t2[1].axis = axis;
    EXPECT(mi355_bn_fold_batched(t2.data(), dev, 2, blocks(t2[0]) + blocks(t2[1]), nullptr) == MI355_EINVAL && says("axis"));
  }
  {
    std::vector<mi355_fold_item> t2(tab.begin(), tab.begin() + 4);
    const int total = blocks(t2[0]) + blocks(t2[1]) + blocks(t2[2]) + blocks(t2[3]);
    t2[2].blk0 += 1;                                  // a first block that disagrees with the items before it
    EXPECT(mi355_bn_fold_batched(t2.data(), dev, 4, total, nullptr) == MI355_EINVAL && says("block"));
    t2[2].blk0 -= 1; t2[3].I = 0;
    EXPECT(mi355_bn_fold_batched(t2.data(), dev, 4, total, nullptr) == MI355_EINVAL);
    t2[3].I = 64; t2[3].out_w = (float*)((char*)t2[3].out_w + 2);      // not even 4-byte aligned
    EXPECT(mi355_bn_fold_batched(t2.data(), dev, 4, total, nullptr) == MI355_EINVAL && says("aligned"));
  }

  // ---- mi355_mse_heatmap: the shapes of the GPU test, aligned and not, with and without the gradient
  const mi355_mse_rec* rec = (const mi355_mse_rec*)fake(50);
  const int hws[] = {1, 35, 64, 4096};
  for (int B : {1, 3, 64})
    for (int hw : hws)
      for (int grad = 0; grad <= 1; ++grad)
        for (int off = 0; off <= 1; ++off)
          EXPECT(ran(mi355_mse_heatmap(ff(51, off), ff(52), rec, ff(53), grad ? ff(54) : nullptr, B, 21, hw, nullptr)));
  EXPECT(ran(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 32, 64, nullptr)));
  EXPECT(ran(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 1, 64, nullptr)));
  EXPECT(mi355_mse_heatmap(nullptr, ff(52), rec, ff(53), ff(54), 2, 21, 64, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mse_heatmap(ff(51), nullptr, rec, ff(53), ff(54), 2, 21, 64, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), nullptr, ff(53), ff(54), 2, 21, 64, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, nullptr, ff(54), 2, 21, 64, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 33, 64, nullptr) == MI355_EINVAL && says("K=33"));
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 0, 64, nullptr) == MI355_EINVAL);
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 0, 21, 64, nullptr) == MI355_EINVAL);
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 21, 0, nullptr) == MI355_EINVAL && says("HW=0"));
  EXPECT(mi355_mse_heatmap(ff(51), ff(52), rec, ff(53), ff(54), 2, 21, -5, nullptr) == MI355_EINVAL && says("HW=-5"));
  EXPECT(mi355_mse_heatmap((const float*)((const char*)ff(51) + 1), ff(52), rec, ff(53), ff(54), 2, 21, 64, nullptr) == MI355_EINVAL);
  std::printf("teacher driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

// Host-side exerciser of the Adam / AdamW entry points (mi355_adam_step_batched / mi355_adam_tick_batched) for the CPU-box
// sanitizer job (tests/test_host_adam.py): built like gradclip_driver.cpp -- the HOST pass of every .hip file with
// -fsanitize=address,undefined, linked with this program.  No GPU is needed or used: device pointers are fake, well-aligned
// addresses that the host never dereferences, and every launch fails in the HIP runtime AFTER the host code under test has run.
// The job passes when no sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL, naming what is
// wrong.  The table walk below runs the kernel's own block-to-slice function (csrc/adam_slice.h, __host__ __device__) on host
// tables: every block of a well-formed table lands in one item, inside [0, n), on a 16-byte boundary, and a block behind the end of a
// malformed table gets an empty slice.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/mi355pose.h"
#include "../../domain-adaptative-hand-pose-estimation_amd/csrc/adam_slice.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static void* fake(size_t i, size_t off = 0) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + (i << 28) + off)); }
static const mi355_adam_item* tab(size_t off = 0) { return reinterpret_cast<const mi355_adam_item*>(fake(1, off)); }
static const mi355_clip_rec* rec(size_t off = 0) { return reinterpret_cast<const mi355_clip_rec*>(fake(2, off)); }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }
static int blocks_of(long n) { return (int)((n + MI355_ADAM_CHUNK - 1) / MI355_ADAM_CHUNK); }

int main() {
  static_assert(sizeof(mi355_adam_item) == 88, "record layout of mi355/ops.py");
  static_assert(offsetof(mi355_adam_item, step) == 32 && offsetof(mi355_adam_item, lr) == 40 && offsetof(mi355_adam_item, n) == 48 &&
                offsetof(mi355_adam_item, beta1) == 56 && offsetof(mi355_adam_item, beta2) == 64 && offsetof(mi355_adam_item, eps) == 72 &&
                offsetof(mi355_adam_item, wd) == 76 && offsetof(mi355_adam_item, decoupled) == 80 && offsetof(mi355_adam_item, blk0) == 84, "field offsets of mi355/ops.py");
  static_assert(MI355_ADAM_CHUNK % (4 * 256) == 0, "a chunk is whole float4 passes of 256 lanes");

  // ---- a table of the lengths of tests/test_gpu_adam.py: every block maps into its item
  const long C = MI355_ADAM_CHUNK;
  const long lens[] = {1, 3, 4, 5, 255, 1024, C, C + 1, 2 * C + 7, 25000000};
  std::vector<mi355_adam_item> items;
  int total = 0;
  for (long n : lens) {
    mi355_adam_item it;
    std::memset(&it, 0, sizeof it);
    it.n = n; it.blk0 = total; it.beta1 = 0.9; it.beta2 = 0.999; it.eps = 1e-8f;
    items.push_back(it);
    total += blocks_of(n);
  }
  std::vector<long> covered(items.size(), 0);
  for (int b = 0; b < total; ++b) {
    const adam_slice s = adam_block_slice(items.data(), (int)items.size(), b);
    EXPECT(s.item >= 0 && s.item < (int)items.size() && b >= items[s.item].blk0);
    EXPECT(s.len > 0 && s.len <= C && s.i0 % C == 0 && s.i0 >= 0 && s.i0 + s.len <= items[s.item].n);
    EXPECT(s.i0 + s.len == items[s.item].n || s.len == C);
    covered[s.item] += s.len;
  }
  for (size_t i = 0; i < items.size(); ++i) EXPECT(covered[i] == items[i].n);
  for (int b = total; b < total + 3; ++b) {            // more blocks than the table has slices: nothing to touch
    const adam_slice s = adam_block_slice(items.data(), (int)items.size(), b);
    EXPECT(s.item == (int)items.size() - 1 && s.len == 0);
  }
  EXPECT(adam_block_slice(items.data(), 1, 0).len == 1 && adam_block_slice(items.data(), 1, 1).len == 0);

  // ---- accepted shapes
  for (long n : lens) EXPECT(ran(mi355_adam_step_batched(tab(), 1, blocks_of(n), nullptr, nullptr)) && ran(mi355_adam_step_batched(tab(), 1, blocks_of(n), rec(), nullptr)));
  EXPECT(ran(mi355_adam_step_batched(tab(), (int)items.size(), total, rec(), nullptr)));
  EXPECT(ran(mi355_adam_step_batched(tab(), 170, 2500, nullptr, nullptr)) && ran(mi355_adam_step_batched(tab(), 1, 0x7fffffff, nullptr, nullptr)));
  for (int count : {1, 3, 255, 256, 257, 170, 100000})
    EXPECT(ran(mi355_adam_tick_batched(tab(), count, nullptr, nullptr)) && ran(mi355_adam_tick_batched(tab(), count, rec(), nullptr)));
  EXPECT(ran(mi355_adam_tick_batched(tab(), 0x7fffffff, nullptr, nullptr)));          // (the grid size must not overflow)

  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  EXPECT(mi355_adam_step_batched(nullptr, 1, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_adam_step_batched(nullptr, 1, 1, rec(), nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_adam_step_batched(tab(), 0, 1, nullptr, nullptr) == MI355_EINVAL && says("count=0"));
  EXPECT(mi355_adam_step_batched(tab(), -1, 1, nullptr, nullptr) == MI355_EINVAL && says("count=-1"));
  EXPECT(mi355_adam_step_batched(tab(), 1, 0, nullptr, nullptr) == MI355_EINVAL && says("total_blocks=0"));
  EXPECT(mi355_adam_step_batched(tab(), 1, -7, nullptr, nullptr) == MI355_EINVAL && says("total_blocks=-7"));
  EXPECT(mi355_adam_step_batched(tab(), 9, 8, nullptr, nullptr) == MI355_EINVAL && says("total_blocks=8"));
  EXPECT(mi355_adam_step_batched(tab(4), 1, 1, nullptr, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_adam_step_batched(tab(), 1, 1, rec(4), nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_adam_tick_batched(nullptr, 1, nullptr, nullptr) == MI355_EINVAL && says("null"));
  EXPECT(mi355_adam_tick_batched(tab(), 0, nullptr, nullptr) == MI355_EINVAL && says("count=0"));
  EXPECT(mi355_adam_tick_batched(tab(), -5, rec(), nullptr) == MI355_EINVAL && says("count=-5"));
  EXPECT(mi355_adam_tick_batched(tab(4), 1, nullptr, nullptr) == MI355_EINVAL && says("aligned"));
  EXPECT(mi355_adam_tick_batched(tab(), 1, rec(4), nullptr) == MI355_EINVAL && says("aligned"));
  std::printf("adam driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

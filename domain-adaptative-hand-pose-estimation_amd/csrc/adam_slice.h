// Which part of which item of an mi355_adam_item table block b owns: shared by adam_step_kernel (csrc/optim.hip) and by the host
// program that walks tables under the sanitizers (tests/host_sanitize/adam_driver.cpp), so both run the same code.
#pragma once
#include "../../include/mi355pose.h"

struct adam_slice { int item; long i0; int len; };          // elements [i0, i0 + len) of items[item]; len <= 0: nothing

// The last item whose blk0 <= b (binary search, as grad_sumsq_kernel), and the MI355_ADAM_CHUNK slice of it that block b - blk0
// is.  i0 is a multiple of the chunk, so a 16-byte aligned item keeps its quads aligned.  A block behind the last slice of its item
// (a malformed table) gets len <= 0.
__host__ __device__ inline adam_slice adam_block_slice(const mi355_adam_item* items, int nitems, int b) {
  int lo = 0, hi = nitems - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  adam_slice s;
  s.item = lo;
  s.i0 = (long)(b - items[lo].blk0) * MI355_ADAM_CHUNK;
  const long left = items[lo].n - s.i0;
  s.len = left <= 0 ? 0 : (left < MI355_ADAM_CHUNK ? (int)left : MI355_ADAM_CHUNK);
  return s;
}

// What the per-joint pooling kernels of jfa.hip (loss1 / loss3) and proto.hip (lossx / lossx3) share: the window of a key point and
// the check of the geometry arguments.
#pragma once
#include <math.h>
#include "common.h"

struct jfa_win { int r0, r1, q0, q1; };          // rows [r0, r1) x columns [q0, q1); empty when r1 <= r0 or q1 <= q0

// The reference's window (loss1): r0 = int(max(cr - radius, 0)), r1 = int(min(cr + radius, H - 1)) and the same for the columns
// with W - 1 -- fp32 arithmetic, truncation towards zero as .int() does, the half-open slice r0:r1.  `rows_by_x`: the reference
// slices the row axis by x and the column axis by y; 0 is the geometric indexing.  A coordinate outside the map leaves r1 <= r0
// (the reference falls into negative-index slicing there): an empty window.  A NaN coordinate gives an empty window as well.
// The bounds are brought into [0, H] and [-1, H - 1] as floats before the conversion, so that an infinity or a value past 2^31
// never reaches the cast; for every other value this changes nothing (a lower bound above H and an upper bound below 0 are
// empty windows either way).
__device__ __forceinline__ jfa_win jfa_window(const float* __restrict__ xy, int radius, int rows_by_x, int H, int W) {
  const float x = xy[0], y = xy[1], rad = (float)radius;
  const float cr = rows_by_x ? x : y, cc = rows_by_x ? y : x;
  jfa_win w;
  if (cr != cr || cc != cc) { w.r0 = 0; w.r1 = 0; w.q0 = 0; w.q1 = 0; return w; }
  w.r0 = (int)fminf(fmaxf(cr - rad, 0.f), (float)H);
  w.r1 = (int)fmaxf(fminf(cr + rad, (float)(H - 1)), -1.f);
  w.q0 = (int)fminf(fmaxf(cc - rad, 0.f), (float)W);
  w.q1 = (int)fmaxf(fminf(cc + rad, (float)(W - 1)), -1.f);
  return w;
}

// nullptr, or what is wrong with the geometry (`tile`: the channels of a block's channel tile)
static const char* jfa_geometry(const char* who, int B, int K, int C, int H, int W, int radius, float divisor, int dtype, int tile) {
  static thread_local char msg[160];
  msg[0] = 0;
  if (dtype != MI355_F32 && dtype != MI355_BF16) snprintf(msg, sizeof(msg), "%s: dtype=%d (fp32 or bf16 features)", who, dtype);
  else if (B < 1 || B > 65535) snprintf(msg, sizeof(msg), "%s: B=%d (1 .. 65535)", who, B);
  else if (K < 1 || K > MI355_JFA_MAX_JOINTS) snprintf(msg, sizeof(msg), "%s: K=%d (1 .. %d joints)", who, K, MI355_JFA_MAX_JOINTS);
  else if (C < 8 || C % 8) snprintf(msg, sizeof(msg), "%s: C=%d (a multiple of 8, at least 8)", who, C);
  else if (H < 1 || W < 1 || (long)H * W > (1L << 24)) snprintf(msg, sizeof(msg), "%s: H=%d W=%d (at least 1, H W <= 2^24)", who, H, W);
  else if (radius < 1 || radius > (1 << 20)) snprintf(msg, sizeof(msg), "%s: radius=%d (at least 1)", who, radius);
  else if (!(divisor > 0.f) || !isfinite(divisor)) snprintf(msg, sizeof(msg), "%s: divisor=%g must be positive", who, (double)divisor);
  else if (cdiv(C, tile) > 65535) snprintf(msg, sizeof(msg), "%s: C=%d too large (at most 65535 channel tiles of %d)", who, C, tile);
  return msg[0] ? msg : nullptr;
}

// Host-side plan of the conv-family launches in plain C++17 -- no HIP header, so tests/conv_dispatch_probe.cpp prints the choices
// without a GPU.  Describe: mi355_conv_desc -> the shape half of GatherArgs.  Choose: GatherArgs + element size + ConvKnobs ->
// ConvBuild, the value that names the kernel build and from which the launch-log label is printed.  (Launch: one table per kernel
// in igemm.hip / pgemm.hip / igemm_fp8.hip maps a ConvBuild to its instantiation.)  Also the one copy of the tile grid with its
// statistics-slice admission and of the weight-gradient split rule.
#pragma once
#include <stdlib.h>
#include "common.h"

#define MAX_TAPS 52
struct Tap { int8_t dy, dx; int16_t widx; };

// One launch covers up to 4 independent sub-problems ("phases") that share A, B, D and the tile shape: the stride^2
// output phases of a strided dgrad / ConvTranspose forward, each a unit-stride gather over its own tap subset.
// Logical tile id = tile_in_phase * nphase + phase, so every XCD gets the same mix of light and heavy phases.
struct Phase { int OHp, OWp, out_oy, out_ox, M, ntaps, tap0, ntm; };
struct GatherArgs {
  const void* A; const void* B; void* D;
  const float* bias; const void* residual; const float* scale;
  int Hi, Wi, Ci;
  int in_sy, in_sx;
  int Ho, Wo;
  int out_sy, out_sx;
  int Nout, ldb, ldd;
  int cshift;
  int accumulate;
  int nphase, ntn, ntiles;     // ntiles = nphase * max_phase(ntm) * ntn
  int hw;                      // heat-map output mode: pixels per image
  int lw;                      // KW3: log2(min(W, 128))
  unsigned a_bytes, b_bytes;
  size_t stat_bytes;           // (host) capacity of stat_partial
  int stat_slices;             // (host) slices the launch writes: nphase * ntm, 0 when the statistics were not fused
  // BatchNorm BACKWARD reduction fused into the epilogue: this launch produces dy of a BatchNorm whose input was bnb_x
  // (same shape as D); per m-tile slice and channel it leaves (sum dy_eff, sum dy_eff * xhat) in bnb_partial[slice][Nout][2].
  // bnb_relu: 0 none, 1 mask from bnb_y > 0, 2 mask recomputed from bnb_x (see bn.hip).
  const void* bnb_x; const void* bnb_y;
  const float* bnb_mean; const float* bnb_invstd; const float* bnb_gamma; const float* bnb_beta;
  float* bnb_partial; int bnb_relu;
  float* stat_partial;         // BatchNorm statistics of the OUTPUT fused into the epilogue: [m-tile slice][Nout][n, mean, M2]
  Phase ph[4];
  Tap taps[MAX_TAPS];
  const float* scale2;         // fp8 path: further device scalars multiplied into the output (operand descales)
  const float* scale3;
  int a_fmt;                   // fp8 path: format of the gathered operand, 0 = e4m3, 1 = e5m2
  // accumulate = 1 only: the value already in D is kept where its bit is set ([rows][ldd / chunk] bytes, bit e = channel
  // chunk * chunk_size + e: the ReLU bit mask of BatchNorm's forward) -- D + this launch's result = masked fork gradient
  const unsigned char* acc_mask;
  int relu;                    // max(0, .) on the finished value (inference: conv + folded BatchNorm + ReLU in one launch)
  // Concatenated-K forward (CAT builds of the gather kernel): D += A2 * B2^T as ONE more K tile behind the conv's own taps --
  // A2 [M][c2] lives at the OUTPUT resolution (row m = output pixel m: single phase, unit output stride), B2 [Nout][c2],
  // c2 <= one K tile.  `heatmap_conv(y) + feature_conv(f)` of the multiscale-fusion heads as one GEMM (regda_7.py:4573-4581).
  // MX build of the fp8 gather kernel (igemm_fp8.hip, mx_fp8.hip), which has no CAT form and shares these slots: the E8M0 scale
  // arrays of A and B (one byte per 32 contracted elements, laid out like the operand with its contiguous axis divided by 32 --
  // the scale dword of a 128-channel K tile sits at (byte offset of the tile's first element) / 32) and their sizes.
  union { const void* A2; const void* mx_sa; };
  union { const void* B2; const void* mx_sb; };
  const float* bias2;
  int c2;
  union { unsigned a2_bytes; unsigned mx_sa_bytes; };
  union { unsigned b2_bytes; unsigned mx_sb_bytes; };
  int pg_nadd;                 // (pgemm.hip, ADD build) slots of the addend ring
  // MX build, inference epilogue (EPI 3 of gather_fp8_kernel): D = act(acc + bias + residual) with `relu` as above, no statistics,
  // no accumulate, no scale.  mx_y8 / mx_sy (both or neither; Nout % 32 == 0): the MX copy of the bf16 values stored to D -- e4m3
  // laid out like D, one E8M0 byte per 32 output channels of a pixel at (element offset in D) / 32.
  int mx_act;
  void* mx_y8; void* mx_sy;
};

// ------------------------------------------------------------------------------------ knobs
inline long conv_knob(const char* name, long dflt, bool* set = nullptr) {
  const char* v = getenv(name);
  if (set) *set = v != nullptr;
  return v ? atol(v) : dflt;
}
inline bool conv_knob_set(const char* name) { bool set; (void)conv_knob(name, 0, &set); return set; }
// Every MI355_* switch the conv family reads, read once per process (conv_knobs).  A/B and experiment switches unless said otherwise.
struct ConvKnobs {
  int tile = (int)conv_knob("MI355_TILE", -1);            // force a register-staged tile (0: 128x128, 1: 64x128, 2: 128x64, 3: 64x64)
  int dma = (int)conv_knob("MI355_DMA", 1);               // LDS-DMA ring; 0 disables, 2 forces (tests)
  int cat_tile = (int)conv_knob("MI355_CAT_TILE", 0);     // force a concat-K tile (1: 128x128, 2: 128x128 dma, 3: 64x128)
  // 256 x 256 LDS-DMA tiles.  1: launches of ONE round of tiles (30.41 / 30.42 -> 30.15 / 30.18 ms; with 128 .. 191 tiles too:
  // slower); 2 (default): also up to four full rounds, the phases of strided input gradients / transposed convs, the concat-K forward
  int t256d = (int)conv_knob("MI355_T256D", 2);
  long t256d_min = conv_knob("MI355_T256D_MIN", 192);     // fewest 256 x 256 tiles of a (last) round
  long t256d_kmin = conv_knob("MI355_T256D_KMIN", 32);    // shortest K taken, in 16-byte chunks
  bool t256 = conv_knob_set("MI355_T256");                // (set at all) the register-staged 256 x 256 tile
  int kw3 = (int)conv_knob("MI355_KW3", 1);               // shared-A-tile builds; 2: wherever the shape allows (tests), 4: without the 256x128 macro tile
  int kw3_n64 = (int)conv_knob("MI355_KW3_N64", 1);       // the shared-A-tile variant for 64 output channels
  int splitk = (int)conv_knob("MI355_SPLITK", 2);         // two K groups per workgroup (1: 128 x 128 tiles only)
  long splitk_min = conv_knob("MI355_SPLITK_MIN", 128), splitk_max = conv_knob("MI355_SPLITK_MAX", 320);      // tile counts taken
  long splitk_kmin = conv_knob("MI355_SPLITK_KMIN", 128); // shortest K taken, in 16-byte chunks (128: the 1x1 convs with K = 1024 at 16x16 too, 30.88 / 30.81 -> 30.76 / 30.76 ms)
  bool stats256 = conv_knob("MI355_STATS_256", 1) != 0;   // statistics epilogue on the 256-row tiles
  int phases = (int)conv_knob("MI355_PHASES", 1);         // 0: one launch per phase of a strided input gradient
  int wg_blocks = (int)conv_knob("MI355_WG_BLOCKS", 768); // blocks a weight gradient aims at (3 per CU)
  int wgrad_kw = (int)conv_knob("MI355_WGRAD_KW", 1);     // the kw-shared 3x3 / stride-1 weight-gradient kernel
  int wgrad_kw2 = (int)conv_knob("MI355_WGRAD_KW2", 1);   // the parity-image 3x3 / 4x4 stride-2 weight-gradient kernel
  bool wgrad_group256 = conv_knob("MI355_WGRAD_GROUP256", 1) != 0;      // the 256 x 256-tile grouped weight-gradient kernel
  bool wgrad_kw_group = conv_knob("MI355_WGRAD_KW_GROUP", 1) != 0;      // grouped launches of the 3x3 / stride-1 kernel
  int wg_group_blocks = (int)conv_knob("MI355_WG_GROUP_BLOCKS", 512);   // (768 -> 512: -0.09 ms / iteration, three same-box pairs)
  int wg_group256_blocks = (int)conv_knob("MI355_WG_GROUP256_BLOCKS", 256);
  int wg_kw_group_blocks = (int)conv_knob("MI355_WG_KW_GROUP_BLOCKS", 512);      // (512 / 768 / 1024: 32.47 / 32.55 / 32.64 ms per iteration, same box)
  // The persistent GEMM.  0: never; 1: where it measured faster than the gather kernel; 2: wherever the launch fits the kernel
  // (tests, A/B runs).  pgemm_set >= 0 (mi355_set_pgemm) overrides the environment at run time.
  int pgemm = (int)conv_knob("MI355_PGEMM", 1), pgemm_set = -1;
  int pg_add_maxk = (int)conv_knob("MI355_PG_ADD", 1) * 64;      // largest K the addend ring takes (0 = none)
  long pg_min_rows = conv_knob("MI355_PG_MIN_ROWS", 32768);
  int pg_ring = (int)conv_knob("MI355_PG_RING", 0), pg_bm = (int)conv_knob("MI355_PG_BM", 64);
  int pg_per_cu = (int)conv_knob("MI355_PG_PER_CU", 2);   // blocks of the persistent grid per CU, at most
  int fp8_tile = (int)conv_knob("MI355_FP8_TILE", -1);    // force an fp8 / MX tile (0: 128x128, 1: 64x128)
  // fewest 128x128 tiles for the fp8 shared-A-tile build (0 off); fp8_kw3_set >= 0 (mi355_set_fp8_kw3) overrides the environment
  long fp8_kw3 = conv_knob("MI355_FP8_KW3", 1024), fp8_kw3_set = -1;
};
// the process's knobs (one object for every translation unit of the library: the run-time setters write it)
inline ConvKnobs& conv_knobs() { static ConvKnobs k; return k; }

// ------------------------------------------------------------------------------------ describe
// forward: one phase, every tap of the window
static inline void describe_fwd(GatherArgs& a, const mi355_conv_desc* d) {
  a.Hi = d->Hi; a.Wi = d->Wi; a.Ci = d->Ci; a.in_sy = a.in_sx = d->stride;
  a.Ho = d->Ho; a.Wo = d->Wo; a.out_sy = a.out_sx = 1;
  a.Nout = d->Co; a.ldd = d->Co; a.ldb = d->kh * d->kw * d->Ci;
  a.nphase = 1; a.ph[0].OHp = d->Ho; a.ph[0].OWp = d->Wo; a.ph[0].M = d->N * d->Ho * d->Wo; a.ph[0].ntaps = d->kh * d->kw;
  for (int i = 0; i < d->kh; ++i)
    for (int j = 0; j < d->kw; ++j) { Tap& t = a.taps[i * d->kw + j]; t.dy = (int8_t)(i - d->pad); t.dx = (int8_t)(j - d->pad); t.widx = (int16_t)(i * d->kw + j); }
}
// conv-form dgrad: dx[n][iy][ix][ci] = sum_{kh,kw,co} dy[n][(iy+p-kh)/s][(ix+p-kw)/s][co] * w[co][kh][kw][ci]
// decomposed into stride^2 phases (iy%s, ix%s), each a unit-stride gather over its own tap subset.  A phase without taps is
// left out (a.nphase may end up 0); returns whether there is one, i.e. whether dx has pixels no phase writes.
static inline bool describe_dgrad(GatherArgs& a, const mi355_conv_desc* d) {
  const int s = d->stride;
  auto parity_without_tap = [&](int k) {      // along one axis of the k-wide window
    for (int p = 0; p < s; ++p) { int cnt = 0; for (int i = 0; i < k; ++i) if ((p + d->pad - i) % s == 0) ++cnt; if (!cnt) return true; }
    return false;
  };
  const bool need_zero = parity_without_tap(d->kh) || parity_without_tap(d->kw);
  a.Hi = d->Ho; a.Wi = d->Wo; a.Ci = d->Co;
  a.in_sy = a.in_sx = 1; a.Ho = d->Hi; a.Wo = d->Wi; a.out_sy = a.out_sx = s;
  a.Nout = d->Ci; a.ldd = d->Ci; a.ldb = d->kh * d->kw * d->Co;
  a.nphase = 0;
  int nt = 0;
  for (int py = 0; py < s; ++py)
    for (int px = 0; px < s; ++px) {
      Phase& P = a.ph[a.nphase];
      P.OHp = (d->Hi - py + s - 1) / s; P.OWp = (d->Wi - px + s - 1) / s;
      if (P.OHp <= 0 || P.OWp <= 0) continue;
      P.out_oy = py; P.out_ox = px; P.M = d->N * P.OHp * P.OWp; P.tap0 = nt;
      for (int kh = 0; kh < d->kh; ++kh) {
        if ((py + d->pad - kh) % s != 0) continue;
        for (int kw = 0; kw < d->kw; ++kw) {
          if ((px + d->pad - kw) % s != 0) continue;
          Tap& t = a.taps[nt++]; t.dy = (int8_t)((py + d->pad - kh) / s); t.dx = (int8_t)((px + d->pad - kw) / s);
          t.widx = (int16_t)(kh * d->kw + kw);
        }
      }
      P.ntaps = nt - P.tap0;
      if (P.ntaps == 0) continue;   // region already zeroed (or left untouched when accumulating)
      ++a.nphase;
    }
  return need_zero;
}
// statistics of dx only when every output pixel is produced by this launch (no zero-filled or empty phase)
static inline bool dgrad_fuses_stats(const GatherArgs& a, int stride, bool need_zero) { return !need_zero && a.nphase == stride * stride; }
// capacity that always suffices for the fused statistics of a conv output / deconv output (smallest tile = 64 rows)
static inline size_t conv_stats_bytes(long rows, int C) { return (size_t)(rows / 64 + 8) * C * 3 * sizeof(float); }

// ------------------------------------------------------------------------------------ the build of a launch
enum ConvFamily { CONV_GATHER = 0, CONV_PGEMM, CONV_FP8, CONV_MX };
struct ConvBuild {
  int family = CONV_GATHER;
  int bm = 64, bn = 64;      // tile
  bool f32 = false;          // fp32 build (bf16 otherwise)
  bool small_c = false;      // small-channel tile (fewer than 8 chunks of input channels)
  bool hm = false;           // heat-map output (mi355_conv1x1_heatmap only)
  bool dma = false;          // LDS-DMA ring
  bool kw3 = false;          // shared A tile
  bool cat = false;          // concat-K
  int kg = 1;                // K groups per workgroup (1 or 2)
  int ns = 0; bool add = false;      // persistent GEMM: ring depth, addend ring
  bool bf8 = false;          // fp8: e5m2 gathered operand
  int epi = 0;               // 0 plain, 1 statistics, 2 BatchNorm-backward: known once the launcher has admitted the slices; 3 MX inference (mx_act)
};
// What the launch log shows in brackets (common.h, "profiling"): printed from the value the launch table is indexed with.
static inline void conv_build_text(const ConvBuild& b, char* out, size_t n) {
  char epi[8] = "";
  if (b.epi) snprintf(epi, sizeof(epi), " epi%d", b.epi);
  if (b.family == CONV_PGEMM) snprintf(out, n, "pgemm bm%d bn%d ns%d%s%s", b.bm, b.bn, b.ns, epi, b.add ? " add" : "");
  else if (b.family == CONV_GATHER)
    snprintf(out, n, "%sg%dx%d%s%s%s%s%s%s%s", b.cat ? "cat " : "", b.bm, b.bn, b.f32 ? " f32" : "", b.small_c ? " small" : "", b.hm ? " hm" : "",
             b.dma ? " dma" : "", b.kw3 ? " kw3" : "", b.kg == 2 ? " kg2" : "", epi);
  else snprintf(out, n, "%s g%dx%d%s%s%s", b.family == CONV_MX ? "mx" : "f8", b.bm, b.bn, b.kw3 ? " kw3" : "", b.bf8 ? " bf8" : "", epi);
}

// ------------------------------------------------------------------------------------ choose
// 3x3 / unit stride / same-size maps of a power-of-two width in [8, 128], taps in row-major order: the shape the shared-A-tile
// ("kw3") builds take.  The bf16 and the fp8 chooser add their own conditions.
static inline bool kw3_shape(const GatherArgs& a) {
  if (!(a.nphase == 1 && a.ph[0].ntaps == 9 && a.in_sx == 1 && a.in_sy == 1 && a.out_sx == 1 && a.out_sy == 1 &&
        a.ph[0].OWp == a.Wi && a.ph[0].OHp == a.Hi && a.Wo == a.Wi && a.Ho == a.Hi && a.Wi >= 8 && a.Wi <= 128 && ilog2_exact(a.Wi) >= 0))
    return false;
  for (int g = 0; g < 3; ++g) {
    const Tap* tp = a.taps + a.ph[0].tap0 + 3 * g;
    int seen = 0;
    for (int k = 0; k < 3; ++k) { if (tp[k].dy != tp[0].dy || tp[k].dx < -1 || tp[k].dx > 1) return false; seen |= 1 << (tp[k].dx + 1); }
    if (seen != 7 || tp[0].dy < -1 || tp[0].dy > 1) return false;
  }
  return true;
}

// Do the 256 x 256 tiles of this launch fill whole rounds of 256 CUs (one 8-wave block per CU)?  mode 1: exactly one round of
// >= tmin tiles; mode 2 (experiment): up to four rounds, the last one with >= tmin tiles, phases of a strided launch counted separately.
static inline bool t256_fits(const GatherArgs& a, int mode, long tmin) {
  long t = 0;
  for (int i = 0; i < a.nphase; ++i) t += cdiv(a.ph[i].M, 256L) * (a.Nout / 256);
  if (mode < 2) return t >= tmin && t <= 256;
  const long rem = t % 256;
  return t >= tmin && t <= 1024 && (rem == 0 || rem >= tmin);
}

// what the ladders below look at
struct GatherWork {
  long Mtot = 0;
  long kavg;             // K in 16-byte chunks, averaged over the phases (those of a strided dgrad differ in length)
  long t128, t64;        // tiles of 128 x 128 / 64 x 128
  bool small;            // fewer than 8 chunks of input channels
};
static inline GatherWork gather_work(const GatherArgs& a, int elem_size) {
  GatherWork w; long ntaps_tot = 0;
  for (int i = 0; i < a.nphase; ++i) { w.Mtot += a.ph[i].M; ntaps_tot += a.ph[i].ntaps; }
  const int chunks = a.Ci / (16 / elem_size);
  w.small = chunks < 8;
  w.kavg = ntaps_tot * chunks / a.nphase;
  w.t128 = (long)cdiv(w.Mtot, 128L) * cdiv(a.Nout, 128);
  w.t64 = (long)cdiv(w.Mtot, 64L) * cdiv(a.Nout, 128);
  return w;
}

// The rungs the plain and the concat-K ladder end with (more than 64 output columns; b arrives as a 64 x 64 tile).
static inline ConvBuild choose_by_tile_count(ConvBuild b, const GatherWork& w, const ConvKnobs& k) {
  // LDS-DMA ring for K-heavy layers (>= 16 K-tiles): +9..12 % on the 3x3 / 4x4 convs, but -15 % on short-K 1x1 convs
  // (2 blocks/CU instead of 3), so those keep the register-staged form.  MI355_DMA=0 disables, =2 forces (tests).
  // (measured: 334 -> 310 us forward, 324 -> 312 us dgrad on 256->256 @64x64; at 1024 tiles the LDS-DMA ring still wins)
  // (also the K-heavy mid-size layers, 256 .. 511 tiles with K >= 2048: 3x3 256->256 @16x16 36.2 -> 32.7 us; a 3-stage ring with
  //  two tiles in flight and counted vmcnt measured 33.5 us there: the per-CU fill rate, not latency, bounds these layers)
  if (k.dma == 2 || (k.dma == 1 && ((w.t128 >= 512 && w.kavg >= 128) || (w.t128 >= 256 && w.kavg >= 256)))) { b.bm = 128; b.bn = 128; b.dma = true; }
  // short-K 1x1 convs at large M are all prologue / epilogue and HBM-bound: more, smaller blocks in flight win
  // (64->256 @64x64: 54.5 -> 47.0 us, 256->256: 79.6 -> 68.9 us)
  else if (w.t128 >= 512 && w.kavg <= 32 && !b.f32) { b.bm = 64; b.bn = 128; }
  else if (w.t128 >= 512) { b.bm = 128; b.bn = 128; }   // (128x256 tile with 8 waves measured slower: 687 vs 755 TFLOP/s)
  else if (w.t64 >= 512) { b.bm = 64; b.bn = 128; }
  return b;
}

// concatenated-K forward: the tile choices of the plain path that matter for the two layers that use it (1x1 and 3x3 / stride 2,
// 256 -> 256 channels), register-staged or LDS-DMA ring
static inline ConvBuild choose_cat(const GatherArgs& a, int elem_size, const ConvKnobs& k) {
  const GatherWork w = gather_work(a, elem_size);
  ConvBuild b;
  b.f32 = elem_size == 4; b.cat = true;
  if (k.t256d >= 2 && !b.f32 && a.Nout % 256 == 0 && k.dma == 1 && t256_fits(a, k.t256d, k.t256d_min)) { b.bm = 256; b.bn = 256; b.dma = true; }
  else if (k.cat_tile == 1 && a.Nout > 64) { b.bm = 128; b.bn = 128; }
  else if (k.cat_tile == 2 && a.Nout > 64) { b.bm = 128; b.bn = 128; b.dma = true; }
  else if (k.cat_tile == 3 && a.Nout > 64) { b.bm = 64; b.bn = 128; }
  else if (a.Nout > 64) b = choose_by_tile_count(b, w, k);
  return b;
}

// column tile of the persistent GEMM: the widest whose weight slice [BN][K] stays within 64 KB
static inline int pg_bn(const GatherArgs& a) {
  if (a.Nout > 64 && (long)a.Ci * 128 * 2 <= 64 * 1024) return 128;
  if ((long)a.Ci * 64 * 2 <= 64 * 1024) return 64;
  return 0;
}
// LDS of a persistent-GEMM block (PgSmem of pgemm.hip) plus `nadd` addend-ring slots (tile + mask bytes each)
static inline int pgemm_smem(int bm, int bn, int ns, int nk, int nadd) {
  return nk * bn * 128 + ns * bm * 128 + bm * bn * 2 + nadd * (bm * bn * 2 + bm * bn / 8);
}
static inline int pgemm_nadd(int ns, int nk, bool add) { return add ? (ns - 1) / nk + 2 : 0; }      // addend-ring slots (kernel comment)
// Does the launch described by `a` fit the persistent GEMM (pgemm.hip)?  1x1, unit stride both ways (GEMM rows =
// NHWC pixels in order), bf16, whole 64-channel K steps, a weight slice of one column tile that fits LDS beside the ring, no
// BatchNorm-backward epilogue, no heat-map output, no concatenated second operand.
static inline bool pgemm_eligible(const GatherArgs& a, int elem_size, const ConvKnobs& k) {
  const int mode = k.pgemm_set >= 0 ? k.pgemm_set : k.pgemm;
  if (!mode || elem_size != 2) return false;
  if (a.nphase != 1 || a.ph[0].ntaps != 1 || a.A2) return false;
  const Tap& tp = a.taps[a.ph[0].tap0];
  if (tp.dy != 0 || tp.dx != 0 || tp.widx != 0) return false;
  if (a.in_sx != 1 || a.in_sy != 1 || a.out_sx != 1 || a.out_sy != 1) return false;
  if (a.ph[0].OHp != a.Hi || a.ph[0].OWp != a.Wi || a.Ho != a.Hi || a.Wo != a.Wi || a.ph[0].out_oy || a.ph[0].out_ox) return false;
  if (a.Ci % 64 || a.ldb != a.Ci || a.ldd != a.Nout || a.Nout % 8) return false;
  if (a.bnb_partial || a.hw) return false;
  const long Mrows = a.ph[0].M;
  if (Mrows * a.Ci * 2 >= (1L << 31) || Mrows * a.Nout * 2 >= (1L << 31)) return false;
  if (Mrows < 256 || !pg_bn(a)) return false;
  if (a.residual && a.accumulate) return false;               // (one addend tensor per tile in the addend ring)
  if (a.acc_mask && (a.Nout % 32 || !a.accumulate)) return false;      // mask bytes travel as dwords
  if (mode >= 2) return true;
  // residual / accumulate epilogues (addend ring): one block per CU carries ring, addend slots and a heavier epilogue -- measured
  // 87 -> 74 us on 64 -> 256 @64x64 + residual (eval), 44 -> 46 us on 128 -> 512 @32x32 + residual: worth it for one K step per tile only
  if ((a.residual || a.accumulate) && a.Ci > k.pg_add_maxk) return false;
  // Where it wins against the gather kernel (profiles/r04_pgemm_layers.txt: per layer, operands from HBM): the large maps
  // (>= 32 K rows), with a short K (<= 128: wide outputs stream at 5 TB/s) or a narrow output (K = 256 -> 64 / 128 columns).
  // K = 256 -> 256 columns needs two column tiles, i.e. the activations twice (no gain), K = 512 leaves room for 64-wide
  // column tiles only (slower).
  return Mrows >= k.pg_min_rows && (a.Ci <= 128 || (a.Ci <= 256 && a.Nout <= 128));
}
static inline ConvBuild choose_pgemm(const GatherArgs& a, const ConvKnobs& k) {
  ConvBuild b;
  b.family = CONV_PGEMM; b.bm = k.pg_bm == 128 ? 128 : 64; b.bn = pg_bn(a);
  const int nk = a.Ci >> 6;
  b.add = a.residual || a.accumulate;
  // ring depth: the deepest ring with which TWO blocks still share a CU (each hides the other's epilogue), else the deepest that fits
  int ring = k.pg_ring;
  if (!ring) {
    auto bytes = [&](int ns) { return pgemm_smem(64, b.bn, ns, nk, pgemm_nadd(ns, nk, b.add)); };
    if (!b.add) for (int ns : {8, 6, 5, 4}) if (!ring && bytes(ns) <= 80 * 1024) ring = ns;      // two blocks per CU
    for (int ns : {8, 6, 5, 4}) if (!ring && bytes(ns) <= 160 * 1024) ring = ns;
  }
  b.ns = (b.bm == 64 && (ring == 8 || ring == 6 || ring == 5)) ? ring : 4;      // (the 128-row tile exists with a ring of 4 only)
  return b;
}
// Tile grid of a persistent-GEMM launch, its addend ring and the admission of the statistics epilogue (b.epi).  Returns the
// dynamic LDS of a block, 0 when the weight slice does not fit.
static inline int pgemm_plan_grid(GatherArgs& a, ConvBuild& b) {
  const int nk = a.Ci >> 6;
  a.pg_nadd = pgemm_nadd(b.ns, nk, b.add);
  const int smem = pgemm_smem(b.bm, b.bn, b.ns, nk, a.pg_nadd);
  if (smem > 160 * 1024) return 0;
  const int ntm = a.ph[0].ntm = cdiv(a.ph[0].M, b.bm);
  a.ntn = cdiv(a.Nout, b.bn);
  a.ntiles = ntm * a.ntn; a.stat_slices = 0;
  if (a.stat_partial && (b.add || (size_t)ntm * a.Nout * 3 * sizeof(float) > a.stat_bytes)) a.stat_partial = nullptr;
  b.epi = a.stat_partial ? 1 : 0;
  return smem;
}

// The bf16 / fp32 launch described by `a` (cshift excepted, which the chooser does not read) -> its build.  The ORDER of the
// rungs is the behaviour.
static inline ConvBuild choose_conv(const GatherArgs& a, int elem_size, const ConvKnobs& k) {
  if (a.A2) return choose_cat(a, elem_size, k);
  const bool bf16 = elem_size == 2;
  if (bf16 && pgemm_eligible(a, 2, k)) return choose_pgemm(a, k);       // 1x1 / unit stride: the persistent pipelined GEMM (pgemm.hip)
  const GatherWork w = gather_work(a, elem_size);
  ConvBuild b;
  b.f32 = !bf16;
  if (w.small) { b.bm = 128; b.small_c = true; return b; }
  if (k.tile >= 0 && k.tile <= 3) {
    static const int forced[4][2] = {{128, 128}, {64, 128}, {128, 64}, {64, 64}};
    b.bm = forced[k.tile][0]; b.bn = forced[k.tile][1];
    return b;
  }
  // 3x3 / unit stride / same-size maps of a power-of-two width <= 128: the A-tile-sharing variant (see KW3 in igemm.hip)
  const bool kw3 = k.kw3 && bf16 && kw3_shape(a) && (a.Nout > 64 || (k.kw3_n64 && a.Nout == 64)) && a.Ci % 64 == 0 && !a.bnb_partial;
  const long rows128 = cdiv(w.Mtot, 128L);
  if (a.Nout <= 64) {
    // 3x3 64 -> 64 on the large maps (layer1 of the ResNets: 2048 tiles of 128 x 64): the shared-A-tile variant here too -- two
    // thirds of what a 128 x 64 tile stages per tap is the A tile
    if (kw3 && (rows128 >= 2048 || k.kw3 == 2)) { b.bm = 128; b.kw3 = true; }
    else if (rows128 >= 512) b.bm = 128;
  }
  else if (bf16 && k.t256 && a.Nout % 256 == 0 && (long)cdiv(w.Mtot, 256L) * (a.Nout / 256) >= 256) { b.bm = 256; b.bn = 256; }
  // one 256 x 256 tile per CU on the LDS-DMA ring (8 waves, 128 accumulators each): half the bytes through L1 per MFMA of the 128 x 128
  // tiles, for launches that offer one round of such tiles
  // (not the accumulating epilogues: their read-modify-write of a 128-KB tile has no second block on the CU to hide behind --
  //  1x1 1024 -> 256 @16x16 input gradient + masked accumulate 20.8 -> 25.2 us, 256 -> 256 @64x64 + accumulate 93 -> 112 us)
  else if (k.t256d && bf16 && (a.nphase == 1 || k.t256d >= 2) && a.Nout % 256 == 0 && k.dma == 1 && !a.bnb_partial && !a.accumulate &&
           t256_fits(a, k.t256d, k.t256d_min) && w.kavg >= k.t256d_kmin && !(kw3 && w.t128 >= 2048)) {      // (the big 3x3 layers keep the shared-A-tile kernels: 309.7 vs 312.7 us)
    b.bm = 256; b.bn = 256; b.dma = true;
  }
  // 256x128 macro tile (128 accumulators per wave, 2 blocks/CU, 0.21 KB of L1 traffic per MFMA): 313 -> 302 us on the 64x64 layers
  else if (kw3 && w.t128 >= 4096 && k.kw3 != 2 && k.kw3 != 4) { b.bm = 256; b.bn = 128; b.kw3 = true; }
  else if (kw3 && (w.t128 >= 2048 || k.kw3 == 2)) { b.bm = 128; b.bn = 128; b.kw3 = true; }
  // one 128 x 128 tile per CU or fewer and a long K: two K groups per workgroup (KG in igemm.hip) -- 3x3 256 -> 256 @16x16 and kin
  // fewer 128 x 128 tiles than CUs (the 8x8 maps: 128 of them would leave half the chip idle): 64-row tiles, two K groups each
  else if (k.splitk >= 2 && k.dma == 1 && w.t128 < 256 && w.t64 >= k.splitk_min && w.t64 <= 384 && w.kavg >= k.splitk_kmin && !a.bnb_partial) { b.bm = 64; b.bn = 128; b.dma = true; b.kg = 2; }
  else if (k.splitk && k.dma == 1 && w.t128 >= k.splitk_min && w.t128 <= k.splitk_max && w.kavg >= k.splitk_kmin && !a.bnb_partial) { b.bm = 128; b.bn = 128; b.dma = true; b.kg = 2; }
  else b = choose_by_tile_count(b, w, k);
  return b;
}

// fp8 / MX operands (igemm_fp8.hip; element = byte)
static inline ConvBuild choose_fp8(const GatherArgs& a, const ConvKnobs& k) {
  const bool mx = a.mx_sa != nullptr;
  long Mtot = 0;
  for (int i = 0; i < a.nphase; ++i) Mtot += a.ph[i].M;
  const long t128 = (long)cdiv(Mtot, 128L) * cdiv(a.Nout, 128);
  ConvBuild b;
  b.family = mx ? CONV_MX : CONV_FP8; b.bf8 = a.a_fmt != 0;
  // the shared-A-tile variant (kw3_shape) from 1024 128x128 tiles on (MI355_FP8_KW3 / mi355_set_fp8_kw3: 0 off, n = smallest tile count).
  // B=64: 3x3 256->256 @64x64 183 -> 168 us, @32x32 53.5 -> 48.4; below 1024 tiles neutral to slower (@16x16 18.9 -> 21.0).
  // Iteration: ResNet-101 512x512 76.45 / 76.60 -> 76.24 / 76.05 ms, ResNet-50 32.11 / 32.06 -> 31.92 / 32.04.
  const long kw3_min = k.fp8_kw3_set >= 0 ? k.fp8_kw3_set : k.fp8_kw3;
  if (!mx && kw3_min > 0 && t128 >= kw3_min && a.Nout > 64 && kw3_shape(a)) { b.bm = 128; b.bn = 128; b.kw3 = true; }      // (no MX build of it)
  else if (k.fp8_tile == 0 || (k.fp8_tile < 0 && t128 >= 512 && a.Nout > 64)) { b.bm = 128; b.bn = 128; }
  else if (k.fp8_tile == 1 || (k.fp8_tile < 0 && a.Nout > 64 && (long)cdiv(Mtot, 64L) * cdiv(a.Nout, 128) >= 256)) b.bn = 128;
  return b;
}

// ------------------------------------------------------------------------------------ tile grid and epilogue admission
// Tile grid of a gather launch (bf16 / fp32 / fp8) and the admission of its per-slice epilogue output: the statistics or
// BatchNorm-backward partials are dropped (pointer nulled) when the phases have unequal tile counts, which would leave
// unwritten slices, or when the caller's buffer is too small.
static inline void plan_tile_grid(GatherArgs& a, int bm, int bn, bool hm_out) {
  a.ntn = cdiv(a.Nout, bn);
  int mx = 0;
  for (int i = 0; i < a.nphase; ++i) { a.ph[i].ntm = cdiv(a.ph[i].M, bm); if (a.ph[i].ntm > mx) mx = a.ph[i].ntm; }
  a.ntiles = a.nphase * mx * a.ntn;
  a.stat_slices = 0;
  bool even = !hm_out;
  for (int i = 0; i < a.nphase; ++i) even = even && a.ph[i].ntm == mx;
  if (a.stat_partial) {
    if (even && !a.residual && !a.accumulate && (size_t)a.nphase * mx * a.Nout * 3 * sizeof(float) <= a.stat_bytes) a.stat_slices = a.nphase * mx;
    else a.stat_partial = nullptr;
  }
  if (a.bnb_partial) {
    if (even && !a.stat_partial && (size_t)a.nphase * mx * a.Nout * 2 * sizeof(float) <= a.stat_bytes) a.stat_slices = a.nphase * mx;
    else a.bnb_partial = nullptr;
  }
}
// Which gather builds have which epilogue: the BatchNorm-backward one (EPI 2) exists for the regular tiles only, the statistics
// one (EPI 1) also for the 256x128 macro tile and the 256x256 LDS-DMA build.
constexpr bool gather_has_bnb(int bm, bool hm, bool kw3, bool cat, int kg) { return !hm && bm <= 128 && !kw3 && !cat && kg == 1; }
constexpr bool gather_has_stats(int bm, int bn, bool hm, bool dma) { return !hm && (bm <= 128 || (bm == 256 && bn == 128) || (bm == 256 && bn == 256 && dma)); }
// the epilogue a gather launch runs, after plan_tile_grid: partials the build cannot write are dropped
static inline int gather_epilogue(GatherArgs& a, const ConvBuild& b, const ConvKnobs& k) {
  if (!gather_has_bnb(b.bm, b.hm, b.kw3, b.cat, b.kg)) a.bnb_partial = nullptr;
  if (!gather_has_stats(b.bm, b.bn, b.hm, b.dma) || (b.bm == 256 && !k.stats256)) a.stat_partial = nullptr;
  if (!a.stat_partial && !a.bnb_partial) a.stat_slices = 0;
  return a.bnb_partial ? 2 : a.stat_partial ? 1 : 0;
}

// What the gather and the fp8 launcher do before they start the kernel of build `b`: tile grid, epilogue (b.epi), KW3 width.
static inline void plan_gather_launch(GatherArgs& a, ConvBuild& b, const ConvKnobs& k) {
  plan_tile_grid(a, b.bm, b.bn, b.hm);
  b.epi = b.family == CONV_GATHER ? gather_epilogue(a, b, k) : (b.family == CONV_MX && a.mx_act) ? 3 : (a.stat_partial ? 1 : 0);
  if (b.kw3) a.lw = ilog2_exact(a.Wi);
}

// ------------------------------------------------------------------------------------ weight-gradient plans
// The split rule: S splits of the M reduction rows, each a whole number of K steps, none empty.
struct WgradSplit { int S, rows; };
static inline WgradSplit wgrad_split(long M, int kstep, long want) {
  const long ksteps = (M + kstep - 1) / kstep;
  long S = want > ksteps ? ksteps : want;
  if (S < 1) S = 1;
  long rps = (M + S - 1) / S; rps = ((rps + kstep - 1) / kstep) * kstep;
  WgradSplit r; r.S = (int)((M + rps - 1) / rps); r.rows = (int)rps;
  return r;
}
// split count of a launch on its own: fill the chip (3 blocks per CU), but keep >= 16 reduction steps per block while at least
// one block per CU remains -- short blocks are all prologue / epilogue and every split costs a full fp32 slab write + read.
// (measured per layer, B=64 @256x256: see DESIGN.md)
static inline WgradSplit wgrad_split_alone(long M, int kstep, long tiles, const ConvKnobs& k) {
  const long ksteps = (M + kstep - 1) / kstep;
  long S = (k.wg_blocks + tiles - 1) / tiles;
  const long S16 = ksteps / 16, S256 = (256 + tiles - 1) / tiles, lo = S16 > S256 ? S16 : S256;
  if (S > lo) S = lo;
  if (tiles >= 384) S = 1;                       // enough tiles on their own: direct write, no slab pass
  return wgrad_split(M, kstep, S);
}

struct WgradPlan { int S, rows_per_split, nto, nti, ldw, kw3, mt, kw2; };
static inline WgradPlan plan_wgrad(const mi355_conv_desc* d, const ConvKnobs& k) {
  WgradPlan w; w.ldw = d->kh * d->kw * d->Ci;
  const int bkm = d->dtype == MI355_BF16 ? 64 : 32;
  const long M = (long)d->N * d->Ho * d->Wo;
  // 3x3 / stride 1 / pad 1 in bf16 with a power-of-two width: the kw-shared kernel (see wgrad_kw_kernel)
  w.kw3 = k.wgrad_kw && d->dtype == MI355_BF16 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 &&
          d->Ho == d->Hi && d->Wo == d->Wi &&              // (not a cropped output: the shifted-row trick needs same-size maps)
          d->Wi >= 8 && ilog2_exact(d->Wi) >= 0;
  w.mt = d->Co <= 64 ? 1 : 2;
  // 3x3 / 4x4, stride 2, pad 1 in bf16, output width a power of two in [8, 64]: the parity-image kernel (wgrad_kw2_kernel)
  w.kw2 = k.wgrad_kw2 && d->dtype == MI355_BF16 && d->kh == d->kw && (d->kh == 3 || d->kh == 4) && d->stride == 2 && d->pad == 1 &&
          d->Hi % 2 == 0 && d->Wi % 2 == 0 && d->Ho == d->Hi / 2 && d->Wo == d->Wi / 2 && d->Wo >= 8 && d->Wo <= 64 &&
          ilog2_exact(d->Wo) >= 0;
  long tiles;
  if (w.kw2) { w.nto = cdiv(d->Co, 64 * w.mt); w.nti = cdiv(d->Ci, 64); tiles = (long)w.nto * d->kh * w.nti; }
  else if (w.kw3) { w.nto = cdiv(d->Co, 64 * w.mt); w.nti = cdiv(d->Ci, 64); tiles = (long)w.nto * 3 * w.nti; }
  else { w.nto = cdiv(d->Co, 128); w.nti = cdiv(w.ldw, 128); tiles = (long)w.nto * w.nti; }
  const WgradSplit s = wgrad_split_alone(M, bkm, tiles, k);
  w.S = s.S; w.rows_per_split = s.rows;
  return w;
}
// the kernel a single weight-gradient launch runs, as the launch log names it
static inline const char* wgrad_kernel_name(const WgradPlan& w) { return w.kw2 ? "wgrad_kw2" : w.kw3 ? "wgrad_kw" : "wgrad"; }

// ------------------------------------------------------------------------------------ grouped weight-gradient plans
// mi355_conv_wgrad_grouped: which items share a launch (walk_wgrad_groups) and the split counts and slab offsets of one grouped
// launch (group_plan).  igemm.hip launches from these; tests/conv_dispatch_probe.cpp prints them without a GPU.
#define WG_MAX 24        // items of one launch of the generic / the 256 x 256-tile grouped kernel
#define WGK_MAX 16       // items of one launch of the grouped 3x3 / stride-1 kernel
static inline bool group_eligible(const mi355_conv_desc* d, const WgradPlan& w) {
  return !w.kw2 && !w.kw3 && (long)w.nto * w.nti < 384;
}
// ... and of those, the ones the 256 x 256-tile kernel takes (wgrad_group256_kernel): bf16, whole 256-wide tiles both ways
static inline bool group256_eligible(const mi355_conv_desc* d, const WgradPlan& w) {
  return conv_knobs().wgrad_group256 && d->dtype == MI355_BF16 && d->kh == 1 && d->kw == 1 && d->pad == 0 && d->Co % 256 == 0 && d->Ci % 256 == 0;
}
// 3x3 / stride-1 problems (wgrad_kw_kernel) small enough to share a launch: fewer than 24 K steps per block at 768 blocks
static inline bool kw_group_eligible(const mi355_conv_desc* d, const WgradPlan& w) {
  if (!conv_knobs().wgrad_kw_group || !w.kw3) return false;
  const long M = (long)d->N * d->Ho * d->Wo, ksteps = (M + 63) / 64;
  return (long)w.nto * 3 * w.nti * ksteps < 768L * 24;
}
static inline long group_tiles(int kind, const mi355_conv_desc* d, const WgradPlan& w) {
  return kind == 3 ? (long)(d->Co / 256) * (w.ldw / 256) : kind == 2 ? (long)w.nto * 3 * w.nti : (long)w.nto * w.nti;
}
struct GroupPlan { int S, rps; size_t ws_off; };
// Split counts and slab offsets of the items of one grouped launch of `kind`; returns its blocks.
static inline long group_plan(const mi355_wgrad_item* items, const int* idx, int n, GroupPlan* gp, size_t* ws_bytes, int kind) {
  const ConvKnobs& kn = conv_knobs();
  const int target = kind == 3 ? kn.wg_group256_blocks : kind == 2 ? kn.wg_kw_group_blocks : kn.wg_group_blocks;
  auto rows = [](const mi355_conv_desc* d) { return (long)d->N * d->Ho * d->Wo; };
  auto kstep = [](const mi355_conv_desc* d) { return d->dtype == MI355_BF16 ? 64 : 32; };
  // equal work per block: block-steps W = sum tiles_i * ksteps_i; aim at 3 blocks per CU, never fewer than 16 K-steps per block
  // (256-wide tiles: one 8-wave block per CU)
  double W = 0;
  for (int k = 0; k < n; ++k) {
    const mi355_conv_desc* d = &items[idx[k]].d;
    W += (double)group_tiles(kind, d, plan_wgrad(d, kn)) * ((rows(d) + kstep(d) - 1) / kstep(d));
  }
  long per = (long)(W / target) + 1; if (per < 16) per = 16;
  auto plan_at = [&](long per, GroupPlan* out, size_t* ws_end) {      // blocks of the group when every block runs `per` K steps
    long blocks = 0; size_t off = 0;
    for (int k = 0; k < n; ++k) {
      const mi355_wgrad_item& it = items[idx[k]]; const mi355_conv_desc* d = &it.d; const WgradPlan w = plan_wgrad(d, kn);
      const WgradSplit s = wgrad_split(rows(d), kstep(d), ((rows(d) + kstep(d) - 1) / kstep(d) + per - 1) / per);
      if (out) { out[k].S = s.S; out[k].rps = s.rows; out[k].ws_off = off; }
      if (s.S > 1 || it.accumulate) off += (size_t)s.S * d->Co * w.ldw * sizeof(float);
      blocks += group_tiles(kind, d, w) * s.S;
    }
    if (ws_end) *ws_end = off;
    return blocks;
  };
  // 256-wide tiles run one block per CU: a grid of 294 blocks on 256 CUs would take two rounds, the second nearly empty -- lengthen
  // the blocks until the group fits the target (rounding the split counts up is what overshoots it)
  for (int trial = 0; kind == 3 && trial < 64; ++trial) {
    if (plan_at(per, nullptr, nullptr) <= target) break;
    per += per / 16 + 1;
  }
  return plan_at(per, gp, ws_bytes);
}
// The launches mi355_conv_wgrad_grouped makes of `items`, in order, handed to `fn(kind, idx, m)`: kind 0 = one item through
// mi355_conv_wgrad, 1 = a group of the generic kernel, 2 = a group of the 3x3 / stride-1 kernel, 3 = a group of the 256 x 256-tile kernel.  One walk for the launcher and
// for the workspace size, so the two cannot disagree.  Two items that write the same dw (one conv used twice in a backward:
// overwrite, then accumulate) must neither share a launch -- the overwrite and the read-modify-write would race -- nor change
// their order: whatever is pending goes first.
template <typename F>
static inline int walk_wgrad_groups(const mi355_wgrad_item* items, int n, F&& fn) {
  int gi[WG_MAX], ki[WGK_MAX], bi[WG_MAX]; int gm = 0, km = 0, bm = 0;
  auto flush_g = [&]() -> int { if (!gm) return 0; int e = fn(1, gi, gm); gm = 0; return e; };
  auto flush_k = [&]() -> int { if (!km) return 0; int e = fn(2, ki, km); km = 0; return e; };
  auto flush_b = [&]() -> int { if (!bm) return 0; int e = fn(3, bi, bm); bm = 0; return e; };
  for (int i = 0; i < n; ++i) {
    const mi355_wgrad_item& it = items[i];
    WgradPlan w = plan_wgrad(&it.d, conv_knobs());
    bool shares = false;
    for (int k = 0; k < gm; ++k) shares = shares || items[gi[k]].dw == it.dw;
    for (int k = 0; k < km; ++k) shares = shares || items[ki[k]].dw == it.dw;
    for (int k = 0; k < bm; ++k) shares = shares || items[bi[k]].dw == it.dw;
    if (shares) { if (int e = flush_g()) return e; if (int e = flush_k()) return e; if (int e = flush_b()) return e; }
    if (kw_group_eligible(&it.d, w)) {
      if (km && (km == WGK_MAX || plan_wgrad(&items[ki[0]].d, conv_knobs()).mt != w.mt)) { if (int e = flush_k()) return e; }
      ki[km++] = i;
    } else if (group_eligible(&it.d, w) && group256_eligible(&it.d, w)) {
      if (bm == WG_MAX) { if (int e = flush_b()) return e; }
      bi[bm++] = i;
    } else if (group_eligible(&it.d, w)) {
      if (gm && (gm == WG_MAX || items[gi[0]].d.dtype != it.d.dtype)) { if (int e = flush_g()) return e; }
      gi[gm++] = i;
    } else {
      int one = i;
      if (int e = fn(0, &one, 1)) return e;
    }
  }
  if (int e = flush_g()) return e;
  if (int e = flush_b()) return e;
  return flush_k();
}

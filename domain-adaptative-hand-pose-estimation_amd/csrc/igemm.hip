// Implicit-GEMM convolution family on MFMA (gfx950):
//   gather-GEMM  : D[m][n] = sum_{tap} sum_c A[pix(m)+off(tap)][c] * B[n][tap][c]
//                  -> conv-form forward, and (per stride phase) conv-form dgrad / ConvTranspose fwd
//   wgrad-GEMM   : dW[o][tap][c] = sum_m DY[m][o] * X[pix(m)+off(tap)][c]   (split over m, slab reduce)
// Layout: activations NHWC, K (channels) contiguous, 16-byte chunks; tiles staged through LDS in
// 128-byte rows with an XOR swizzle so that ds_read_b128 fragment reads are conflict-free.
// bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulate.  f32: v_mfma_f32_32x32x2_f32 (exact fp32, parity path).
#include "common.h"
#include <stdlib.h>

#include "igemm_common.h"

template <typename T> struct MmaTraits;
template <> struct MmaTraits<bf16_t> { static constexpr int BK = 64; static constexpr int CH = 8; };
template <> struct MmaTraits<float> { static constexpr int BK = 32; static constexpr int CH = 4; };

#define GATHER_STAGES 1     // one LDS stage: the pipeline depth lives in registers (see the K loop)
template <typename T, int BM, int BN, int STAGES = 1, bool KW3 = false>
struct GatherSmem {
  static constexpr int kARows = KW3 ? BM + 4 * (BM / 8) + 4 : BM;        // KW3: segmented A image with spare rows (see the kernel)
  static constexpr int kStage = (kARows + BN) * 128;
  static constexpr int kOutStride = BN * (int)sizeof(T) + 16;
  static constexpr int kOut = BM * kOutStride;
  static constexpr int kBytes = (STAGES * kStage > kOut ? STAGES * kStage : kOut) + BM * 4;
};

// WGM x WGN waves per workgroup (64 lanes each); every wave owns a (BM/WGM) x (BN/WGN) sub-tile.
// HM_OUT: the result is written as NCHW fp32 heat-maps [image][Nout][hw] (the 1x1 conv to the K=21 key-point maps).
// DMA: K-tiles travel global -> LDS directly (buffer_load ... lds, 1 KiB per wave-instruction, out-of-range lanes deliver
//      zeros) into a 2-stage ring: no staging registers, no ds_write, one barrier per K-tile.
// EPI: epilogue extras, compiled separately so the plain kernel keeps its register budget (3 blocks per CU):
//      0 plain, 1 + BatchNorm statistics of the output, 2 + BatchNorm-backward reduction of the output.
// KW3: 3x3 / unit-stride convs (forward and input gradient).  The three taps of a kernel row read the same pixels shifted by
//      -1 / 0 / +1, so ONE staged A tile per (kernel row, 64-channel chunk) serves three K sub-steps (three B tiles): a third
//      fewer bytes through L1 and LDS per MFMA.  The LDS A image keeps every run of min(W,128) pixels in a segment of its
//      own with spare zero rows between segments, so a shifted fragment read sees zeros exactly at the image border
//      (same construction as wgrad_kw_kernel).
// CAT: one more K tile behind the conv's own taps, gathered from a second operand pair (A2 [M][c2] at the output resolution,
//      B2 [Nout][c2]; channels c2 .. BK-1 of that tile are out-of-range lanes = zeros): y = conv(x, w) + A2 * B2^T as ONE GEMM.
// KG: K groups inside the workgroup (intra-workgroup split-K; LDS-DMA builds).  A launch that offers one tile per CU or fewer runs
//      one wave per SIMD, and its K loop is a chain of exposed load latencies (one tile in flight per CU).  With KG = 2 the block has
//      2 x WGM x WGN waves: group g multiplies its half of the K tiles out of a ring of its own (two tiles in flight per CU, two
//      waves per SIMD), group 1 then hands its accumulators to group 0 through LDS (fp32, its own ring's space) and group 0 runs
//      the usual epilogue -- streamed out by all the block's threads.  No fp32 partials in HBM.
template <typename T, int BM, int BN, bool SMALL_C, int WGM = 2, int WGN = 2, bool HM_OUT = false, bool DMA = false, int EPI = 0,
          bool KW3 = false, bool CAT = false, int KG = 1>
__global__ __launch_bounds__(64 * WGM * WGN * KG, (KW3 && BM == 256) ? 2 : 1) void gather_gemm_kernel(const GatherArgs p) {
  constexpr int CH = MmaTraits<T>::CH;
  constexpr int GTHR = 64 * WGM * WGN;                          // threads of one K group (= the whole block unless KG > 1)
  constexpr int NTHR = GTHR * KG, RPP = GTHR / 8;               // rows staged per pass (8 lanes = one 128-byte row)
  constexpr int WM = BM / WGM, WN = BN / WGN, MT = WM / 32, NT = WN / 32;
  constexpr int RA = BM / RPP, RB = BN / RPP;
  using SM = GatherSmem<T, BM, BN, DMA ? 2 : 1, KW3>;
  static_assert(!KW3 || (!DMA && !SMALL_C && !HM_OUT && sizeof(T) == 2), "KW3 is a bf16 variant of the plain large-channel kernel");
  static_assert(!DMA || !SMALL_C, "the LDS-DMA pipeline is built for the large-channel path");
  static_assert(!CAT || (!SMALL_C && !HM_OUT && !KW3 && EPI != 2), "CAT: plain large-channel forward (register-staged or LDS-DMA)");
  static_assert(KG == 1 || (KG == 2 && DMA && !CAT && !HM_OUT && EPI != 2 && BM * BN * 4 <= 2 * SM::kStage), "KG: two K groups on the LDS-DMA ring");
  constexpr int kRing = 2 * SM::kStage;                         // (KG > 1) LDS of one K group's ring; group g's ring starts at g * kRing
  constexpr int kTotal = SM::kBytes + (KG - 1) * kRing;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* row_off = reinterpret_cast<int*>(smem + kTotal - BM * 4);

  const int t = threadIdx.x, lane = t & 63;
  const int tg = KG > 1 ? t % GTHR : t, grp = KG > 1 ? __builtin_amdgcn_readfirstlane(t / GTHR) : 0;      // thread in its K group, K group
  const int wave = tg >> 6, wave_blk = t >> 6;                  // wave in its K group (sub-tile, staging), wave in the block (statistics fold)
  const int tile_g = xcd_remap(blockIdx.x, p.ntiles);
  const int phi = tile_g % p.nphase, tile = tile_g / p.nphase;
  const Phase& P = p.ph[phi];
  if (tile >= P.ntm * p.ntn) return;                 // phases of unequal size (odd extents): block-uniform exit
  const int pM = P.M, pOHp = P.OHp, pOWp = P.OWp, pkchunks = P.ntaps << p.cshift;
  const Tap* __restrict__ ptaps = p.taps + P.tap0;
  const int m0 = (tile / p.ntn) * BM, n0 = (tile % p.ntn) * BN;
  const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
  const int lc = tg & 7, lr = tg >> 3;

  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A, p.a_bytes), rsB = make_rsrc(p.B, p.b_bytes);
  const __amdgpu_buffer_rsrc_t rsA2 = make_rsrc(CAT ? p.A2 : p.A, CAT ? p.a2_bytes : 0u), rsB2 = make_rsrc(CAT ? p.B2 : p.B, CAT ? p.b2_bytes : 0u);
  const int nk_main = (pkchunks + 7) >> 3;            // K tiles of the conv's own taps; the CAT tile is K tile number nk_main

  // decode this thread's A rows once
  int iy0[RA], ix0[RA], abase[RA];
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    int m = m0 + lr + RPP * i;
    if (m < pM) {
      int ox = m % pOWp, r = m / pOWp, oy = r % pOHp, n = r / pOHp;
      iy0[i] = oy * p.in_sy; ix0[i] = ox * p.in_sx; abase[i] = n * p.Hi * p.Wi;
    } else { iy0[i] = -(1 << 20); ix0[i] = 0; abase[i] = 0; }
  }
  if (t < BM) {  // output pixel offset (elements) of every tile row, -1 when out of range
    int m = m0 + t, off = -1;
    if (m < pM) {
      int ox = m % pOWp, r = m / pOWp, oy = r % pOHp, n = r / pOHp;
      off = ((n * p.Ho + oy * p.out_sy + P.out_oy) * p.Wo + ox * p.out_sx + P.out_ox) * p.ldd;
    }
    row_off[t] = off;
  }

  // Register-staged software pipeline over ONE LDS stage (35 KB per block -> 4 blocks = 16 waves per CU): tile kt+1
  // travels HBM -> registers while tile kt is multiplied out of LDS; the other resident blocks cover the rest of the
  // latency.  Measured alternatives (3x3 256->256 @64x64, B=64, fwd): LDS double buffer at 2 blocks/CU 649 TFLOP/s,
  // this form 723, prefetch distance 2 with two register sets (184 VGPRs -> 2 blocks/CU) 616.
  uint4 ra0[RA], rb0[RB];
  const int cmask = (1 << p.cshift) - 1;
  // element offset of every row's window origin: the per-tap part of an A address is then one scalar (dy*Wi+dx)*Ci --
  // no per-row integer multiplies inside the K loop (v_mul_lo_u32 is quarter rate)
  int pix0[RA];
#pragma unroll
  for (int i = 0; i < RA; ++i) pix0[i] = iy0[i] >= 0 ? (abase[i] + iy0[i] * p.Wi + ix0[i]) * p.Ci : 0;
  auto tap_of = [&](int kt) -> Tap { return ptaps[((CAT && kt >= nk_main ? nk_main - 1 : kt) * 8) >> p.cshift]; };     // (large-channel path: one tap per K-tile)
  auto load_tile = [&](int kt, const Tap tpu, uint4 (&ra)[RA], uint4 (&rb)[RB]) {
    if constexpr (CAT) {
      if (kt == nk_main) {              // block-uniform: the second operand pair, chunk lc of row m / output channel n
        const bool okc = lc * CH < p.c2;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
          const int m = m0 + lr + RPP * i;
          ra[i] = buf_load16(rsA2, (okc && m < pM) ? (m * p.c2 + lc * CH) * (int)sizeof(T) : OOB_OFF);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int n = n0 + lr + RPP * i;
          rb[i] = buf_load16(rsB2, (okc && n < p.Nout) ? (n * p.c2 + lc * CH) * (int)sizeof(T) : OOB_OFF);
        }
        return;
      }
    }
    if constexpr (SMALL_C) {
      const int q = kt * 8 + lc; const bool okq = q < pkchunks; const int tap = okq ? (q >> p.cshift) : 0; const int cc = (q & cmask) * CH;
      const Tap tp = ptaps[tap];
      const int koff = (int)tp.widx * p.Ci + cc;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        int iy = iy0[i] + tp.dy, ix = ix0[i] + tp.dx;
        bool ok = okq && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        ra[i] = buf_load16(rsA, ok ? ((abase[i] + iy * p.Wi + ix) * p.Ci + cc) * (int)sizeof(T) : OOB_OFF);
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        int n = n0 + lr + RPP * i;
        rb[i] = buf_load16(rsB, (okq && n < p.Nout) ? (n * p.ldb + koff) * (int)sizeof(T) : OOB_OFF);
      }
    } else {
      const int cc = (((kt * 8) & cmask) + lc) * CH;
      const int toff = ((int)tpu.dy * p.Wi + (int)tpu.dx) * p.Ci + cc;
      const int koff = (int)tpu.widx * p.Ci + cc;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const int iy = iy0[i] + tpu.dy, ix = ix0[i] + tpu.dx;
        const bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        ra[i] = buf_load16(rsA, ok ? (pix0[i] + toff) * (int)sizeof(T) : OOB_OFF);
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        int n = n0 + lr + RPP * i;
        rb[i] = buf_load16(rsB, n < p.Nout ? (n * p.ldb + koff) * (int)sizeof(T) : OOB_OFF);
      }
    }
  };
  // LDS-DMA issue of K-tile kt into ring stage `stage`: lane (row lr, physical chunk lc) fetches the logical chunk
  // lc ^ ((row>>1)&7), so the linear 1-KiB image each wave-instruction writes IS the swizzled tile (swizzle on the source)
  const int lcs = lc ^ ((lr >> 1) & 7);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  auto dma_tile = [&](int kt, int stage) {
    const bool cat = CAT && kt == nk_main;            // block-uniform
    const int q0 = (cat ? 0 : kt) * 8, tap = q0 >> p.cshift;
    const int cc = ((q0 & cmask) + lcs) * CH;
    const Tap tp = ptaps[tap];
    const int koff = (int)tp.widx * p.Ci + cc;
    const int toff = ((int)tp.dy * p.Wi + (int)tp.dx) * p.Ci + cc;
    (void)koff; (void)toff; (void)wave_u;   // (only used in the device pass below)
#if defined(__HIP_DEVICE_COMPILE__)    // (the host pass must still be able to emit the kernel stub)
    typedef __attribute__((address_space(3))) void* ldsp;
    char* sa = smem + grp * kRing + stage * SM::kStage + wave_u * 1024;
    char* sb = sa + BM * 128;
    if constexpr (CAT) {
      if (cat) {                                      // logical chunk lcs of row m / output channel n of the second operand pair
        const bool okc = lcs * CH < p.c2;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
          const int m = m0 + lr + RPP * i;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA2, (ldsp)(sa + i * RPP * 128), 16,
                                                   (okc && m < pM) ? (m * p.c2 + lcs * CH) * (int)sizeof(T) : OOB_OFF, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const int n = n0 + lr + RPP * i;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB2, (ldsp)(sb + i * RPP * 128), 16,
                                                   (okc && n < p.Nout) ? (n * p.c2 + lcs * CH) * (int)sizeof(T) : OOB_OFF, 0, 0, 0);
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      int iy = iy0[i] + tp.dy, ix = ix0[i] + tp.dx;
      bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (ldsp)(sa + i * RPP * 128), 16,
                                               ok ? (pix0[i] + toff) * (int)sizeof(T) : OOB_OFF, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      int n = n0 + lr + RPP * i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (ldsp)(sb + i * RPP * 128), 16,
                                               n < p.Nout ? (n * p.ldb + koff) * (int)sizeof(T) : OOB_OFF, 0, 0, 0);
    }
#endif
  };
  char* as = smem;
  char* bs = smem + SM::kARows * 128;
  auto store_tile = [&](const uint4 (&ra)[RA], const uint4 (&rb)[RB]) {
#pragma unroll
    for (int i = 0; i < RA; ++i) *reinterpret_cast<uint4*>(as + swz128(lr + RPP * i, lc)) = ra[i];
#pragma unroll
    for (int i = 0; i < RB; ++i) *reinterpret_cast<uint4*>(bs + swz128(lr + RPP * i, lc)) = rb[i];
  };

  f32x16_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int r31 = lane & 31, hi = lane >> 5;
  auto compute = [&]() {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8_t a[MT], b[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(as + swz128(wm0 + i * 32 + r31, 2 * s + hi));
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(bs + swz128(wn0 + j * 32 + r31, 2 * s + hi));
        // operands swapped: acc holds D^T (lane = m row, registers = 4-wide runs of n) for a wide epilogue
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int e = 2 * s + hi;
        float a[MT], b[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const float*>(as + swz128(wm0 + i * 32 + r31, e >> 2) + (e & 3) * 4);
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const float*>(bs + swz128(wn0 + j * 32 + r31, e >> 2) + (e & 3) * 4);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    }
  };

  const int nk = nk_main + (CAT ? 1 : 0);
  if constexpr (KW3) {
    // sub-step ks = (group g, kw), group g = (kernel row kh, channel chunk): tap index kh*3 + kw, channels chunk*64 ..
    const int nchunk = p.Ci >> 6, nsub = 9 * nchunk;
    for (int i = t; i < SM::kARows * 8; i += NTHR) reinterpret_cast<uint4*>(as)[i] = make_uint4(0, 0, 0, 0);
    int simg[RA];                                         // LDS byte offset of this thread's A rows in the segmented image
#pragma unroll
    for (int i = 0; i < RA; ++i) { const int r = lr + RPP * i; simg[i] = swz128(r + 2 + 4 * (r >> p.lw), lc); }
    int rimg[MT];                                         // image row of this lane's fragment rows
#pragma unroll
    for (int i = 0; i < MT; ++i) { const int q = wm0 + i * 32 + r31; rimg[i] = q + 2 + 4 * (q >> p.lw); }
    auto load_a = [&](int g, uint4 (&ra)[RA]) {
      const int kh = g / nchunk, chunk = g - kh * nchunk;
      const int dyv = ptaps[kh * 3].dy;
      const int toff = dyv * p.Wi * p.Ci + chunk * 64 + lc * CH;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const bool ok = (unsigned)(iy0[i] + dyv) < (unsigned)p.Hi;
        ra[i] = buf_load16(rsA, ok ? (pix0[i] + toff) * (int)sizeof(T) : OOB_OFF);
      }
    };
    auto load_b = [&](int ks, uint4 (&rb)[RB]) {
      const int g = ks / 3, kw = ks - g * 3;
      const int kh = g / nchunk, chunk = g - kh * nchunk;
      const int koff = (int)ptaps[kh * 3 + kw].widx * p.Ci + chunk * 64 + lc * CH;
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int n = n0 + lr + RPP * i;
        rb[i] = buf_load16(rsB, n < p.Nout ? (n * p.ldb + koff) * (int)sizeof(T) : OOB_OFF);
      }
    };
    auto compute_kw = [&](int dxv) {
      int arow[MT], axor[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) { const int r = rimg[i] + dxv; arow[i] = r * 128; axor[i] = (r >> 1) & 7; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8_t a[MT], b[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(as + arow[i] + (((2 * s + hi) ^ axor[i]) << 4));
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(bs + swz128(wn0 + j * 32 + r31, 2 * s + hi));
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    };
    load_a(0, ra0);
    load_b(0, rb0);
    int kw = 0, g = 0;
    for (int ks = 0; ks < nsub; ++ks) {
      const int dxv = ptaps[(g / nchunk) * 3 + kw].dx;
      __syncthreads();                                    // sub-step ks-1 fully multiplied
      if (kw == 0) {
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<uint4*>(as + simg[i]) = ra0[i];
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) *reinterpret_cast<uint4*>(bs + swz128(lr + RPP * i, lc)) = rb0[i];
      __syncthreads();
      if (ks + 1 < nsub) {
        load_b(ks + 1, rb0);
        if (kw == 2) load_a(g + 1, ra0);                  // the next group's A tile travels during this group's last sub-step
      }
      __builtin_amdgcn_s_setprio(1);
      compute_kw(dxv);
      __builtin_amdgcn_s_setprio(0);
      if (++kw == 3) { kw = 0; ++g; }
    }
  } else if constexpr (DMA && KG > 1) {
    // K group g multiplies K tiles [kbeg, kend) out of its own ring; the barriers are the block's, so both groups make nk0 trips
    const int nk0 = (nk + 1) >> 1;
    const int kbeg = grp ? nk0 : 0, kend = grp ? nk : nk0;
    char* ring = smem + grp * kRing;
    if (kbeg < kend) dma_tile(kbeg, 0);
    for (int i = 0; i < nk0; ++i) {
      const int kt = kbeg + i;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      __syncthreads();
      if (kt + 1 < kend) dma_tile(kt + 1, (i + 1) & 1);
      as = ring + (i & 1) * SM::kStage; bs = as + BM * 128;
      if (kt < kend) {
        __builtin_amdgcn_s_setprio(1);
        compute();
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // group 1's partial sums travel to group 0 through group 1's ring space: [wave][accumulator quad][lane] float4, written and
    // read by the same (wave, lane) pair of each group -- conflict-free, no index arithmetic beyond a constant stride
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem + kRing) + wave * (MT * NT * 4 * 64) + lane;
    if (grp == 1) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            red[((i * NT + j) * 4 + q) * 64] = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
    }
    __syncthreads();
    if (grp == 0) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 v = red[((i * NT + j) * 4 + q) * 64];
            acc[i][j][4 * q] += v.x; acc[i][j][4 * q + 1] += v.y; acc[i][j][4 * q + 2] += v.z; acc[i][j][4 * q + 3] += v.w;
          }
    }
  } else if constexpr (DMA) {
    dma_tile(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of tile kt have landed in LDS
#endif
      __syncthreads();                                      // everyone's have; stage (kt+1)&1 is no longer being read
      if (kt + 1 < nk) dma_tile(kt + 1, (kt + 1) & 1);
      as = smem + (kt & 1) * SM::kStage; bs = as + BM * 128;
      __builtin_amdgcn_s_setprio(1);
      compute();
      __builtin_amdgcn_s_setprio(0);
    }
  } else {
    // (two K-tiles in flight for the small tiles -- 64x128 and below have the registers -- measured: no gain on the
    //  latency-bound mid-size layers, occupancy 5 -> 3; per-K-step issue cost, not prefetch depth, bounds them)
    load_tile(0, tap_of(0), ra0, rb0);
    Tap tpn = tap_of(nk > 1 ? 1 : 0);                      // the tap word of tile kt+1 is fetched one iteration early
    for (int kt = 0; kt < nk; ++kt) {
      const Tap tpu = tpn;
      if (kt + 2 < nk) tpn = tap_of(kt + 2);
      __syncthreads(); store_tile(ra0, rb0); __syncthreads();
      if (kt + 1 < nk) load_tile(kt + 1, tpu, ra0, rb0);
      __builtin_amdgcn_s_setprio(1);
      compute();
      __builtin_amdgcn_s_setprio(0);
    }
  }
  __syncthreads();

  char* outs = smem;
  if constexpr (HM_OUT) {
    // ---- heat-map epilogue: acc + bias -> fp32 LDS tile -> per key-point runs of BM consecutive pixels (512-byte rows)
    constexpr int HS = BN * 4 + 16;
    static_assert(BM * HS <= SM::kBytes - BM * 4, "fp32 staging tile must fit");
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ml = wm0 + i * 32 + r31, nl = wn0 + j * 32 + 8 * g + 4 * hi;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e] + ((p.bias && (nl + e) < p.Nout) ? p.bias[nl + e] : 0.f);
          *reinterpret_cast<float4*>(outs + ml * HS + nl * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
    __syncthreads();
    float* __restrict__ Y = reinterpret_cast<float*>(p.D);
    for (int id = t; id < p.Nout * BM; id += NTHR) {
      const int k = id / BM, r = id % BM;
      const int gp = row_off[r];                       // global pixel index (ldd == 1)
      if (gp < 0) continue;
      const int img = gp / p.hw, pp = gp - img * p.hw;
      Y[((size_t)img * p.Nout + k) * p.hw + pp] = *reinterpret_cast<const float*>(outs + r * HS + k * 4);
    }
    return;
  }
  // ---- epilogue: (acc + bias) * scale -> T -> LDS tile -> coalesced 16-byte rows (+residual / +dx)
  const float scale = p.scale ? *p.scale : 1.0f;
  if (KG == 1 || grp == 0)       // (KG > 1: K group 0 holds the sums; every thread of the block then streams rows out)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ml = wm0 + i * 32 + r31;
        const int nl = wn0 + j * 32 + 8 * g + 4 * hi;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float b = (p.bias && (n0 + nl + e) < p.Nout) ? p.bias[n0 + nl + e] : 0.f;
          if constexpr (CAT) { if (p.bias2 && (n0 + nl + e) < p.Nout) b += p.bias2[n0 + nl + e]; }
          v[e] = (acc[i][j][4 * g + e] + b) * scale;
        }
        char* dst = outs + ml * SM::kOutStride + nl * (int)sizeof(T);
        if constexpr (sizeof(T) == 2) {
          union { bf16_t h[4]; uint2 q; } u;
#pragma unroll
          for (int e = 0; e < 4; ++e) u.h[e] = (bf16_t)v[e];
          *reinterpret_cast<uint2*>(dst) = u.q;
        } else {
          *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
  __syncthreads();
  constexpr int CPR = BN / CH;  // 16-byte chunks per tile row
  T* __restrict__ D = reinterpret_cast<T*>(p.D);
  const T* __restrict__ R = reinterpret_cast<const T*>(p.residual);
  // Optional fused BatchNorm statistics of the tile just produced (per output channel over the tile's valid rows, Welford):
  // every thread already holds the rounded values it streams out, so the statistics cost no extra LDS or HBM reads.
  constexpr bool stats = EPI == 1, bnb = EPI == 2;
  float sn = 0.f, smean[CH], sm2[CH];      // bnb mode reuses smean / sm2 as the two running sums
  float bmu[CH], bis[CH], bsc[CH], bsh[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { smean[e] = 0.f; sm2[e] = 0.f; bmu[e] = 0.f; bis[e] = 0.f; bsc[e] = 0.f; bsh[e] = 0.f; }
  const T* __restrict__ BX = reinterpret_cast<const T*>(p.bnb_x);
  const T* __restrict__ BY = reinterpret_cast<const T*>(p.bnb_y);
  if (bnb) {
    const int n = n0 + (t % CPR) * CH;
    if (n < p.Nout) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        bmu[e] = p.bnb_mean[n + e]; bis[e] = p.bnb_invstd[n + e];
        if (p.bnb_relu == 2) { bsc[e] = p.bnb_gamma[n + e] * bis[e]; bsh[e] = p.bnb_beta[n + e] - bmu[e] * bsc[e]; }
      }
    }
  }
  if constexpr (!bnb) {
    // rows streamed one at a time, loads interleaved with the stores (measured faster than fetching all rows' addends
    // up front: 44 vs 49 us on the 256->64 1x1 dgrad @64x64)
    for (int id = t; id < BM * CPR; id += NTHR) {
      const int r = id / CPR, c = id % CPR;
      const int off = row_off[r];
      const int n = n0 + c * CH;
      if (off < 0 || n >= p.Nout) continue;
      float v[CH];
      Chunk<T>::load(reinterpret_cast<const T*>(outs + r * SM::kOutStride + c * 16), v);
      const size_t g = (size_t)off + n;
      if (stats) {
        // (Welford per row.  A cheaper form -- running sums of deviations from the thread's first row, 3 VALU per element instead
        //  of 6 + a division per row -- is as accurate (1e-8 of float64, both) and halves this epilogue's VALU work in isolation,
        //  but measured no gain in the iteration: 33.27 / 33.34 vs 33.26 / 33.13 ms, same box; other resident blocks hide it)
        sn += 1.f; const float inv = 1.f / sn;
#pragma unroll
        for (int e = 0; e < CH; ++e) { const float d = v[e] - smean[e]; smean[e] += d * inv; sm2[e] += d * (v[e] - smean[e]); }
      }
      if (R) { float w[CH]; Chunk<T>::load(R + g, w);
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] += w[e]; }
      if (p.accumulate) {
        // the optional bit mask is applied to the packed words BEFORE unpacking: selecting per unpacked float made the
        // compiler permute the registers and feed v_pk_add_f32 through op_sel, and those adds dropped an addend now and
        // then (lanes 48-63 only, run-to-run different: 40 - 240 of 8.4 M elements on the 32x64x64x64 dgrad) on gfx950
        uint4 q = *reinterpret_cast<const uint4*>(D + g);
        if (p.acc_mask) q = keep_masked<T>(q, p.acc_mask[g / CH]);
        float w[CH]; Chunk<T>::unpack(q, w);
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] += w[e]; }
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] = v[e] < 0.f ? 0.f : v[e]; }      // (keeps NaN, like ATen relu)
      Chunk<T>::store(D + g, v);
    }
  } else {
    // EPI == 2 (own register budget, 2 blocks per CU): every global operand of the epilogue -- the addend and the
    // BatchNorm's x / y -- is fetched for all of this thread's rows before any is used: one latency instead of one per row
    constexpr int IT = BM * CPR / NTHR;
    static_assert(BM * CPR % NTHR == 0, "whole passes only");
    const int ec = t % CPR, er0 = t / CPR;
    const int en = n0 + ec * CH;
    const bool ecok = en < p.Nout;
    int eoff[IT];
    uint4 qa[IT], qx[IT], qy[IT];
    const T* __restrict__ ADD = R ? R : (p.accumulate ? D : nullptr);
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int off = row_off[er0 + k * (NTHR / CPR)];
      eoff[k] = (off >= 0 && ecok) ? off + en : -1;
      if (eoff[k] >= 0) {
        if (ADD) qa[k] = *reinterpret_cast<const uint4*>(ADD + (size_t)eoff[k]);
        qx[k] = *reinterpret_cast<const uint4*>(BX + (size_t)eoff[k]);
        if (p.bnb_relu == 1) qy[k] = *reinterpret_cast<const uint4*>(BY + (size_t)eoff[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      if (eoff[k] < 0) continue;
      const int r = er0 + k * (NTHR / CPR);
      float v[CH];
      Chunk<T>::load(reinterpret_cast<const T*>(outs + r * SM::kOutStride + ec * 16), v);
      const size_t g = (size_t)eoff[k];
      if (ADD) { float w[CH]; Chunk<T>::unpack(qa[k], w);
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] += w[e]; }
      if (R && p.accumulate) { float w[CH]; Chunk<T>::load(D + g, w);      // (both at once: not used by this model)
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] += w[e]; }
      Chunk<T>::store(D + g, v);
      // same arithmetic as bn_bwd_reduce_kernel, on the value as stored (rounded to T)
      float xv[CH], gq[CH]; Chunk<T>::unpack(qx[k], xv);
#pragma unroll
      for (int e = 0; e < CH; ++e) gq[e] = (float)(T)v[e];
      if (p.bnb_relu == 1) { float yv[CH]; Chunk<T>::unpack(qy[k], yv);
#pragma unroll
        for (int e = 0; e < CH; ++e) gq[e] = yv[e] <= 0.f ? 0.f : gq[e]; }
      else if (p.bnb_relu == 2) {
#pragma unroll
        for (int e = 0; e < CH; ++e) gq[e] = (xv[e] * bsc[e] + bsh[e]) <= 0.f ? 0.f : gq[e]; }
#pragma unroll
      for (int e = 0; e < CH; ++e) { smean[e] += gq[e]; sm2[e] += gq[e] * ((xv[e] - bmu[e]) * bis[e]); }
    }
  }
  if (bnb) {
    constexpr int NW = NTHR / 64;
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < CH; ++e) { smean[e] += __shfl_down(smean[e], o, 64); sm2[e] += __shfl_down(sm2[e], o, 64); }
    }
    __syncthreads();
    float* sp = reinterpret_cast<float*>(smem);        // [NW][BN][2]
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float* q = sp + ((size_t)wave_blk * BN + (t % CPR) * CH + e) * 2;
        q[0] = smean[e]; q[1] = sm2[e];
      }
    }
    __syncthreads();
    if (t < BN && n0 + t < p.Nout) {
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) { a1 += sp[((size_t)w * BN + t) * 2]; a2 += sp[((size_t)w * BN + t) * 2 + 1]; }
      const int slice = (tile / p.ntn) * p.nphase + phi;
      float* out = p.bnb_partial + ((size_t)slice * p.Nout + n0 + t) * 2;
      out[0] = a1; out[1] = a2;
    }
    return;
  }
  if (stats) {
    // thread t owns chunk column t % CPR and the rows t / CPR + k * (NTHR / CPR).  Fold the row lanes: inside a wave by
    // shuffle-down (lower lane = left operand), across the waves through LDS in wave order (fixed order: reproducible).
    constexpr int NW = NTHR / 64;
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
      const float nb = __shfl_down(sn, o, 64);
      const float nt = sn + nb, f = nt > 0.f ? nb / nt : 0.f;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const float mb = __shfl_down(smean[e], o, 64), vb = __shfl_down(sm2[e], o, 64);
        const float d = mb - smean[e];
        smean[e] += d * f; sm2[e] += vb + d * d * sn * f;
      }
      sn = nt;
    }
    __syncthreads();                                   // everyone is done reading the staged tile
    float* sp = reinterpret_cast<float*>(smem);        // [NW][BN][3]
    static_assert(NW * BN * 3 * 4 <= SM::kBytes - BM * 4, "statistics scratch must fit in the tile staging area");
    if (lane < CPR && lane < 64) {
      const int c = t % CPR;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float* q = sp + ((size_t)wave_blk * BN + c * CH + e) * 3;
        q[0] = sn; q[1] = smean[e]; q[2] = sm2[e];
      }
    }
    __syncthreads();
    if (t < BN && n0 + t < p.Nout) {
      float n = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float* q = sp + ((size_t)w * BN + t) * 3;
        const float nb = q[0];
        if (nb > 0.f) { const float nt = n + nb, f = nb / nt, d = q[1] - mean; mean += d * f; m2 += q[2] + d * d * n * f; n = nt; }
      }
      const int slice = (tile / p.ntn) * p.nphase + phi;
      float* out = p.stat_partial + ((size_t)slice * p.Nout + n0 + t) * 3;
      out[0] = n; out[1] = mean; out[2] = m2;
    }
  }
}

// ------------------------------------------------------------------------------------ wgrad
struct WgradArgs {
  const void* X; const void* DY; float* out;
  int Hi, Wi, Ci, Ho, Wo, Co;
  int kw, stride, pad, cshift;
  int M, rows_per_split, ldw;
  long slab_stride;
  int nto, nti;
  unsigned x_bytes, dy_bytes;
  FastDiv dWo, dHo;
};

// tr16-read friendly swizzle of a [rows][256 B] bf16 image (guide T10, image (b))
__device__ __forceinline__ int swz256(int r, int ch) { return r * 256 + ((ch ^ (((r & 3) << 2) | ((r >> 2) & 3))) << 4); }

template <typename T> struct WgradSmem {
  static constexpr int BKM = (sizeof(T) == 2) ? 64 : 32;
  static constexpr int kBytes = 2 * BKM * 128 * (int)sizeof(T) + 2 * BKM * 8;
};
// body shared by the single-problem kernel and the grouped one (`bid` of `nblk` blocks work on problem p)
template <typename T>
__device__ __forceinline__ void wgrad_gemm_body(const WgradArgs& p, const int bid, const int nblk, char* smem) {
  constexpr int CH = MmaTraits<T>::CH;
  constexpr int BKM = (sizeof(T) == 2) ? 64 : 32;   // reduction rows per LDS tile
  constexpr int CPR = 128 / CH;                      // chunks per 128-wide tile row
  constexpr int RPT = BKM * CPR / 256;               // rows per thread per operand
  constexpr int ROWB = 128 * (int)sizeof(T);         // LDS row bytes
  char* ys = smem;                 // DY tile [BKM][128 o]
  char* xs = smem + BKM * ROWB;    // X  tile [BKM][128 cols]
  // pixel decode of the reduction rows, shared by the 16/32 lanes that stage one row: one thread per row decodes
  // (n, oy, ox) for the NEXT tile while this one is multiplied -> {pixel index of the window origin, (iy0<<16)|ix0}
  int2* rowinfo = reinterpret_cast<int2*>(smem + 2 * BKM * ROWB);   // [2][BKM]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // XCD-aware order: all tiles of one pixel range (split) are neighbours in the remapped id, i.e. share an XCD / L2,
  // so the DY and X rows of that range are fetched into one L2 instead of eight
  const int ntile = p.nto * p.nti;
  const int lid = xcd_remap(bid, nblk);
  const int split = lid / ntile, tile = lid - split * ntile;
  const int o0 = (tile / p.nti) * 128, c0 = (tile % p.nti) * 128;  // c0: flattened (tap, ci) column
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  const int lc = t % CPR, lr = t / CPR;

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.X, p.x_bytes), rsY = make_rsrc(p.DY, p.dy_bytes);

  // this thread's fixed column chunk -> (tap, ci)
  const int col = c0 + lc * CH;
  const bool colok = col < p.ldw;
  const int qc = col / CH;
  const int tap = colok ? (qc >> p.cshift) : 0;
  const int ci = (qc & ((1 << p.cshift) - 1)) * CH;
  const int tdy = tap / p.kw - p.pad, tdx = tap % p.kw - p.pad;
  const bool ook = (o0 + lc * CH) < p.Co;

  const int mbeg = split * p.rows_per_split;
  const int mend = min(p.M, mbeg + p.rows_per_split);

  uint4 rx[RPT], ry[RPT];
  const int toff = tdy * p.Wi + tdx;                       // this thread's tap as a pixel-index offset
  auto decode_rows = [&](int mt0, int buf) {               // threads 0..BKM-1, one reduction row each
    if (t < BKM) {
      const unsigned m = (unsigned)(mt0 + t);
      unsigned r = fd_div(m, p.dWo); int ox = (int)(m - r * p.Wo);
      unsigned n = fd_div(r, p.dHo); int oy = (int)(r - n * p.Ho);
      const int iy0 = oy * p.stride, ix0 = ox * p.stride;
      rowinfo[buf * BKM + t] = make_int2(((int)n * p.Hi + iy0) * p.Wi + ix0, (iy0 << 16) | ix0);
    }
  };
  auto load_tile = [&](int mt0, int buf) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int rr = lr + (256 / CPR) * i;
      const int m = mt0 + rr;
      const bool mok = m < mend;
      ry[i] = buf_load16(rsY, (mok && ook) ? (m * p.Co + o0 + lc * CH) * (int)sizeof(T) : OOB_OFF);
      const int2 ri = rowinfo[buf * BKM + rr];
      const int iy = (ri.y >> 16) + tdy, ix = (ri.y & 0xffff) + tdx;
      const bool xok = mok && colok && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
      rx[i] = buf_load16(rsX, xok ? ((ri.x + toff) * p.Ci + ci) * (int)sizeof(T) : OOB_OFF);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = lr + (256 / CPR) * i;
      int off;
      if constexpr (sizeof(T) == 2) off = swz256(r, lc); else off = r * ROWB + lc * 16;
      *reinterpret_cast<uint4*>(ys + off) = ry[i];
      *reinterpret_cast<uint4*>(xs + off) = rx[i];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int r31 = lane & 31, hi = lane >> 5;
  // tr16 lane roles: 16-lane group g reads a 4-row x 16-col block; lane 4q+p supplies row q, cols 4p..4p+3
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  int trA[2][2], trB[2][2];     // LDS byte addresses of the tr16 reads of k-step 0: [sub-tile i][rows +0 / +4]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 8 * (tg >> 1) + tq + 4 * u;
      trA[i][u] = swz256(row, (wm0 + i * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
      trB[i][u] = swz256(row, (wn0 + i * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
    }
  decode_rows(mbeg, 0);
  __syncthreads();
  if (mbeg < mend) load_tile(mbeg, 0);
  int buf = 0;
  for (int mt0 = mbeg; mt0 < mend; mt0 += BKM, buf ^= 1) {
    __syncthreads();   // previous tile's LDS reads done
    store_tile();
    decode_rows(mt0 + BKM, buf ^ 1);
    __syncthreads();
    if (mt0 + BKM < mend) load_tile(mt0 + BKM, buf ^ 1);
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < BKM / 16; ++s) {
        bf16x8_t a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          typedef __attribute__((address_space(3))) bf16x4_t* lds4;
          // the swizzle term of swz256 does not depend on s (16 rows = 4096 B per k-step): base + immediate offset
          bf16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][0] + s * 4096));
          bf16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][1] + s * 4096));
          bf16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xs + trB[i][0] + s * 4096));
          bf16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xs + trB[i][1] + s * 4096));
          a[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
          b[i] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < BKM / 2; ++s) {
        const int row = 2 * s + hi;
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const float*>(ys + row * ROWB + (wm0 + i * 32 + r31) * 4);
          b[i] = *reinterpret_cast<const float*>(xs + row * ROWB + (wn0 + i * 32 + r31) * 4);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  float* out = p.out + (size_t)split * p.slab_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int c = c0 + wn0 + j * 32 + r31;
        if (o < p.Co && c < p.ldw) out[(size_t)o * p.ldw + c] = acc[i][j][r];
      }
}

template <typename T>
__global__ __launch_bounds__(256, 3) void wgrad_gemm_kernel(const WgradArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[WgradSmem<T>::kBytes];
  wgrad_gemm_body<T>(p, blockIdx.x, gridDim.x, smem);
}

// Several independent weight-gradient problems in ONE launch (the small layers of a ResNet stage: each alone offers
// 16 .. 64 output tiles, far too few for 256 CUs, so the single-problem launch splits its pixel range 16 .. 48 ways and
// pays for it with as many fp32 slabs plus a reduce launch).  Grouped, the tiles of all problems fill the chip together:
// 2 .. 4 splits per problem, long K loops, one launch + one grouped slab reduce for the whole stage.  The argument blocks
// travel by value in the kernel-argument segment (graph-capturable, no device table).
struct WgradGroupArgs { WgradArgs p[WG_MAX]; int bstart[WG_MAX + 1]; int n; };
template <typename T>
__global__ __launch_bounds__(256, 3) void wgrad_group_kernel(const WgradGroupArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[WgradSmem<T>::kBytes];
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.bstart[i + 1]) ++i;         // block-uniform scan of <= 24 entries
  wgrad_gemm_body<T>(g.p[i], (int)blockIdx.x - g.bstart[i], g.bstart[i + 1] - g.bstart[i], smem);
}

// 256 x 256 output tiles for the grouped 1x1 weight gradients with >= 256 channels on both sides (bf16; layer3 / layer4 of the
// ResNets).  By counters the 128 x 128 form fetches 2 - 7x its operands from beyond L2 (the sibling tiles of a pixel range do not find
// each other's lines in the 4-MB L2s: the layer4 group moved 0.94 GB through L1 for 0.15 GB of x + dy), i.e. those launches are
// bound by L2-miss bandwidth.  Here a block of 8 waves owns 256 output channels x 256 input channels: per 64-pixel step four
// [64][128] images (two DY halves, two X halves; same tr16 swizzle and fragment reads as the 128 x 128 body) = 64 KB for 256 MFMAs
// -- half the bytes per MFMA -- travel global -> LDS by LDS-DMA into a two-stage ring (the swizzle applied on the per-lane source
// address, out-of-range lanes deliver zeros; one barrier per step, no staging registers: a register-staged form of this tile, one
// block per CU with two barriers per step, measured SLOWER than the 128 x 128 kernel: 265 vs 223 us on the layer3 group), and every
// wave multiplies a 128 x 64 sub-tile (128 accumulators).  1x1 convs only (stride 1 or 2): a column is an input channel.
#define WG256_IMG (64 * 256)
template <int OFF> __device__ __forceinline__ bf16x4_t wg256_tr(unsigned a) {
  bf16x4_t v; asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF)); return v;
}
// one 16-pixel sub-step of a wave's 128 x 64 sub-tile: 12 transposed fragment reads (asm), one counted wait that names them, 8 MFMAs
template <int OFF> __device__ __forceinline__ void wg256_step(unsigned st, const int (&trA)[4][2], const int (&trB)[2][2], f32x16_t (&acc)[4][2]) {
  bf16x4_t a0[4], a1[4], b0[2], b1[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) { a0[i] = wg256_tr<OFF>(st + (unsigned)trA[i][0]); a1[i] = wg256_tr<OFF>(st + (unsigned)trA[i][1]); }
#pragma unroll
  for (int j = 0; j < 2; ++j) { b0[j] = wg256_tr<OFF>(st + (unsigned)trB[j][0]); b1[j] = wg256_tr<OFF>(st + (unsigned)trB[j][1]); }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0[0]), "+v"(a0[1]), "+v"(a0[2]), "+v"(a0[3]), "+v"(a1[0]), "+v"(a1[1]), "+v"(a1[2]), "+v"(a1[3]),
               "+v"(b0[0]), "+v"(b0[1]), "+v"(b1[0]), "+v"(b1[1]));
  bf16x8_t a[4], b[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = __builtin_shufflevector(a0[i], a1[i], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = __builtin_shufflevector(b0[j], b1[j], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
}
#define WG256_SMEM (2 * 4 * WG256_IMG + 2 * 64 * 4)
__device__ __forceinline__ void wgrad_gemm256_body(const WgradArgs& p, const int bid, const int nblk, char* smem) {
  constexpr int BKM = 64, IMG = WG256_IMG, STAGE = 4 * IMG;
  int* rowpix = reinterpret_cast<int*>(smem + 2 * STAGE);      // [2][BKM]: input pixel index of every reduction row
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ntile = p.nto * p.nti;                   // (in 256 x 256 tiles)
  const int lid = xcd_remap(bid, nblk);
  const int split = lid / ntile, tile = lid - split * ntile;
  const int o0 = (tile / p.nti) * 256, c0 = (tile % p.nti) * 256;
  const int wo = wave >> 2, wc = wave & 3;           // multiply: DY image wo (128 output channels), X image wc >> 1, columns (wc & 1) * 64 ..
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.X, p.x_bytes), rsY = make_rsrc(p.DY, p.dy_bytes);
  const int mbeg = split * p.rows_per_split;
  const int mend = min(p.M, mbeg + p.rows_per_split);
  // staging: wave w fills image w >> 1 (0, 1: DY halves, 2, 3: X halves), row groups (w & 1) * 8 + j, j = 0 .. 7, of four rows each;
  // lane -> row (lane >> 4) of the group, physical chunk lane & 15, which holds the logical chunk pc ^ (((r & 3) << 2) | ((r >> 2) & 3))
  const int img = wave >> 1, half = img & 1;
  const bool isx = img >= 2;
  const int rsub = lane >> 4, pc = lane & 15;
  int colb[4];                                       // byte offset of this lane's column for row groups with (group & 3) == q
#pragma unroll
  for (int q = 0; q < 4; ++q) colb[q] = ((isx ? c0 : o0) + half * 128 + ((pc ^ ((rsub << 2) | q)) << 3)) * 2;
  const int ld2 = (isx ? p.Ci : p.Co) * 2;           // row pitch in bytes
  auto decode_rows = [&](int mt0, int buf) {
    if (t < BKM) {
      const unsigned m = (unsigned)(mt0 + t);
      unsigned r = fd_div(m, p.dWo); int ox = (int)(m - r * p.Wo);
      unsigned n = fd_div(r, p.dHo); int oy = (int)(r - n * p.Ho);
      rowpix[buf * BKM + t] = ((int)n * p.Hi + oy * p.stride) * p.Wi + ox * p.stride;
    }
  };
  auto dma_tile = [&](int mt0, int stage, int buf) {
    (void)mt0; (void)stage; (void)buf;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) void* ldsp;
    char* dst = smem + stage * STAGE + img * IMG + (wave & 1) * 8 * 1024;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = ((wave & 1) * 8 + j) * 4 + rsub, m = mt0 + r;
      const int row = isx ? rowpix[buf * BKM + r] : m;
      const int off = m < mend ? row * ld2 + colb[j & 3] : OOB_OFF;
      if (isx) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (ldsp)(dst + j * 1024), 16, off, 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (ldsp)(dst + j * 1024), 16, off, 0, 0, 0);
    }
#endif
  };
  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int r31 = lane & 31, hi = lane >> 5;
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;      // tr16 lane roles (as in wgrad_gemm_body)
  const int wn0 = (wc & 1) * 64;
  int trA[4][2], trB[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = 8 * (tg >> 1) + tq + 4 * u;
#pragma unroll
    for (int i = 0; i < 4; ++i) trA[i][u] = wo * IMG + swz256(row, (i * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) trB[j][u] = (2 + (wc >> 1)) * IMG + swz256(row, (wn0 + j * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
  }
  typedef __attribute__((address_space(3))) char* lds_cptr256;
  const unsigned smem_lds = (unsigned)(uintptr_t)(lds_cptr256)smem;
  decode_rows(mbeg, 0);
  decode_rows(mbeg + BKM, 1);
  __syncthreads();
  if (mbeg < mend) dma_tile(mbeg, 0, 0);
  int it = 0;
  for (int mt0 = mbeg; mt0 < mend; mt0 += BKM, ++it) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's pieces of tile `it` have landed
#endif
    __syncthreads();                                         // everyone's have; stage (it + 1) & 1 is no longer being read
    if (mt0 + BKM < mend) dma_tile(mt0 + BKM, (it + 1) & 1, (it + 1) & 1);
    decode_rows(mt0 + 2 * BKM, it & 1);                      // (row buffer it & 1 was consumed by the DMA issued one trip ago)
    // The fragment reads are inline asm: hipcc guards every LDS read it can see behind an LDS-DMA with `s_waitcnt vmcnt(0)`, i.e. it
    // would wait for the tile issued a few lines up before multiplying this one (seen in the disassembly of the builtin form).
    const unsigned st = smem_lds + (unsigned)((it & 1) * STAGE);
    __builtin_amdgcn_s_setprio(1);
    wg256_step<0>(st, trA, trB, acc); wg256_step<4096>(st, trA, trB, acc); wg256_step<8192>(st, trA, trB, acc); wg256_step<12288>(st, trA, trB, acc);
    __builtin_amdgcn_s_setprio(0);
  }
  float* out = p.out + (size_t)split * p.slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + wo * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int c = c0 + (wc >> 1) * 128 + wn0 + j * 32 + r31;
        if (o < p.Co && c < p.ldw) out[(size_t)o * p.ldw + c] = acc[i][j][r];
      }
}
__global__ __launch_bounds__(512, 1) void wgrad_group256_kernel(const WgradGroupArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem256[];
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.bstart[i + 1]) ++i;
  wgrad_gemm256_body(g.p[i], (int)blockIdx.x - g.bstart[i], g.bstart[i + 1] - g.bstart[i], smem256);
}

// grouped fixed-order slab reduction: out_i (=|+=) sum over the S_i slabs of problem i, one float4 column per thread
struct SlabItem { const float* slabs; float* out; long n4, stride; int S, accumulate; };
struct SlabGroupArgs { SlabItem it[WG_MAX]; int bstart[WG_MAX + 1]; int n; };
__global__ __launch_bounds__(256) void slab_reduce_group_kernel(const SlabGroupArgs g) {
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.bstart[i + 1]) ++i;
  const SlabItem& q = g.it[i];
  const long c = (long)((int)blockIdx.x - g.bstart[i]) * 256 + threadIdx.x;
  if (c >= q.n4) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < q.S; ++s) {
    const float4 a = reinterpret_cast<const float4*>(q.slabs + (size_t)s * q.stride)[c];
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
  }
  if (q.accumulate) { const float4 o = reinterpret_cast<const float4*>(q.out)[c]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
  reinterpret_cast<float4*>(q.out)[c] = v;
}

// ------------------------------------------------------------------------------------ wgrad, 3x3 stride 1 (bf16)
// The three horizontal taps of one kernel row share ONE staged X tile: with unit stride the tap (kh, kw) operand of
// output pixel m is the input pixel m + (kh-1)*W + (kw-1), i.e. the kw taps are the same rows shifted by -1 / 0 / +1.
// A block owns (128|64 output channels) x (64 input channels) x (kh; kw = 0,1,2): per 64-pixel step it stages one DY
// tile and one X tile (the X tile once instead of three times) and issues 3x the MFMAs of the generic kernel's step.
// Row shifts must not leak across image rows: the LDS X image keeps every run of min(W,64) pixels in its own segment
// with 4 spare rows between segments (the row before / after a segment is the halo: zero at the image border, the
// neighbouring pixel when W > 64), so a shifted tr16 read picks up zeros exactly where the padding is.
struct WgradKwArgs {
  const void* X; const void* DY; float* out;
  int H, W, Ci, Co;
  int lw, lwf, halo;            // log2(min(W,64)), log2(W), W > 64
  int M, rows_per_split, ldw;
  long slab_stride;
  int nto, nci;
  unsigned x_bytes, dy_bytes;
  FastDiv dH;
};
// 128-byte rows, tr16-read friendly for any 4 consecutive rows (shifted reads included)
__device__ __forceinline__ int swzx(int r, int ch) { return r * 128 + ((ch ^ (((r >> 1) & 1) << 2)) << 4); }

template <int MT> struct WgradKwSmem { static constexpr int kBytes = 64 * 256 + (64 + 4 * 8 + 4) * 128 + 2 * 64 * 4; };
// body shared by the single-problem kernel and the grouped one (`bid` of `nblk` blocks work on problem p)
template <int MT>
__device__ __forceinline__ void wgrad_kw_body(const WgradKwArgs& p, const int bid, const int nblk, char* smem) {
  constexpr int BO = 64 * MT, BKM = 64;
  constexpr int CPRY = BO / 8, RPY = 256 / CPRY, NPY = BKM / RPY;
  constexpr int XROWS = 64 + 4 * 8 + 4;
  char* ys = smem;
  char* xs = smem + BKM * 256;
  int* rowinfo = reinterpret_cast<int*>(smem + BKM * 256 + XROWS * 128);   // [2][BKM]: image row oy of each pixel

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ntile = p.nto * 3 * p.nci;
  const int lid = xcd_remap(bid, nblk);
  const int split = lid / ntile;
  int tile = lid - split * ntile;
  const int ot = tile / (3 * p.nci); tile -= ot * 3 * p.nci;
  const int kh = tile / p.nci, cit = tile - kh * p.nci;
  const int o0 = ot * BO, ci0 = cit * 64, tdy = kh - 1;
  const int wm0 = (wave >> 1) * (32 * MT), wn0 = (wave & 1) * 32;

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.X, p.x_bytes), rsY = make_rsrc(p.DY, p.dy_bytes);
  const int lcy = t % CPRY, lry = t / CPRY;
  const int lcx = t & 7, lrx = t >> 3;
  const bool ook = (o0 + lcy * 8) < p.Co;
  const bool cok = (ci0 + lcx * 8) < p.Ci;
  const int mbeg = split * p.rows_per_split;
  const int mend = min(p.M, mbeg + p.rows_per_split);

  for (int i = t; i < XROWS * 8; i += 256) reinterpret_cast<uint4*>(xs)[i] = make_uint4(0, 0, 0, 0);

  uint4 ry[NPY], rx[2], rh = make_uint4(0, 0, 0, 0);
  auto decode_rows = [&](int mt0, int buf) {
    if (t < BKM) {
      const unsigned m = (unsigned)(mt0 + t);
      const unsigned r = m >> p.lwf;
      const unsigned n = fd_div(r, p.dH);
      rowinfo[buf * BKM + t] = (m < (unsigned)p.M) ? (int)(r - n * p.H) : -(1 << 20);
    }
  };
  auto load_tile = [&](int mt0, int buf) {
#pragma unroll
    for (int i = 0; i < NPY; ++i) {
      const int m = mt0 + lry + RPY * i;
      ry[i] = buf_load16(rsY, (m < mend && ook) ? (m * p.Co + o0 + lcy * 8) * 2 : OOB_OFF);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rr = lrx + 32 * i, m = mt0 + rr;
      const int oy = rowinfo[buf * BKM + rr];
      const bool ok = cok && (unsigned)(oy + tdy) < (unsigned)p.H;
      rx[i] = buf_load16(rsX, ok ? ((m + tdy * p.W) * p.Ci + ci0 + lcx * 8) * 2 : OOB_OFF);
    }
    if (p.halo && t < 16) {     // W > 64: the tile is a 64-pixel piece of one image row; fetch its two neighbours
      const int side = t >> 3, ox0 = mt0 & (p.W - 1);
      const int oy = rowinfo[buf * BKM];
      const bool ok = (side ? (ox0 + 64 < p.W) : (ox0 > 0)) && (unsigned)(oy + tdy) < (unsigned)p.H && (ci0 + (t & 7) * 8) < p.Ci;
      const int m = mt0 + (side ? 64 : -1);
      rh = buf_load16(rsX, ok ? ((m + tdy * p.W) * p.Ci + ci0 + (t & 7) * 8) * 2 : OOB_OFF);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NPY; ++i) *reinterpret_cast<uint4*>(ys + swz256(lry + RPY * i, lcy)) = ry[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = lrx + 32 * i;
      *reinterpret_cast<uint4*>(xs + swzx(r + 2 + 4 * (r >> p.lw), lcx)) = rx[i];
    }
    if (p.halo && t < 16) *reinterpret_cast<uint4*>(xs + swzx((t >> 3) ? 66 : 1, t & 7)) = rh;
  };

  f32x16_t acc[3][MT];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][i][r] = 0.f;

  const int r31 = lane & 31, hi = lane >> 5;
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  int trA[MT][2], trB[3][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = 8 * (tg >> 1) + tq + 4 * u;                 // reduction row inside a 16-row k-step
#pragma unroll
    for (int i = 0; i < MT; ++i) trA[i][u] = swz256(row, (wm0 + i * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
    const int R0 = row + 2 + 4 * (row >> p.lw);
#pragma unroll
    for (int a = 0; a < 3; ++a) trB[a][u] = swzx(R0 + a - 1, wn0 / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
  }
  decode_rows(mbeg, 0);
  __syncthreads();
  if (mbeg < mend) load_tile(mbeg, 0);
  int buf = 0;
  for (int mt0 = mbeg; mt0 < mend; mt0 += BKM, buf ^= 1) {
    __syncthreads();
    store_tile();
    decode_rows(mt0 + BKM, buf ^ 1);
    __syncthreads();
    if (mt0 + BKM < mend) load_tile(mt0 + BKM, buf ^ 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      typedef __attribute__((address_space(3))) bf16x4_t* lds4;
      const int eoff = (16 * s + 4 * ((16 * s) >> p.lw)) * 128;       // image-row offset of k-step s (uniform)
      bf16x8_t a[MT], b[3];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        bf16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][0] + s * 4096));
        bf16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][1] + s * 4096));
        a[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        bf16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xs + trB[k][0] + eoff));
        bf16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xs + trB[k][1] + eoff));
        b[k] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[k][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[k], acc[k][i], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }
  float* out = p.out + (size_t)split * p.slab_stride;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int c = ci0 + wn0 + r31;
        if (o < p.Co && c < p.Ci) out[(size_t)o * p.ldw + (kh * 3 + k) * p.Ci + c] = acc[k][i][r];
      }
}
template <int MT>
__global__ __launch_bounds__(256, 3) void wgrad_kw_kernel(const WgradKwArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[WgradKwSmem<MT>::kBytes];
  wgrad_kw_body<MT>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}
// The 3x3 / stride-1 weight gradients of one ResNet stage in ONE launch (bf16).  Alone, such a layer offers 24 .. 48 output tiles:
// it splits its pixel range 16 .. 256 ways to reach a few hundred blocks, which then sit unevenly on the 256 CUs (384 blocks:
// half the CUs carry two), run 8 .. 16 K steps each (mostly prologue and fp32 slab stores) and leave 16 .. 256 slabs to a reduce
// launch of their own.  Grouped, the tiles of all the stage's layers fill the chip together with a few long splits per layer and
// one grouped slab reduction.  Argument blocks by value in the kernel-argument segment (graph-capturable), as wgrad_group_kernel.
struct WgradKwGroupArgs { WgradKwArgs p[WGK_MAX]; int bstart[WGK_MAX + 1]; int n; };
template <int MT>
__global__ __launch_bounds__(256, 3) void wgrad_kw_group_kernel(const WgradKwGroupArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[WgradKwSmem<MT>::kBytes];
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.bstart[i + 1]) ++i;         // block-uniform scan of <= 16 entries
  wgrad_kw_body<MT>(g.p[i], (int)blockIdx.x - g.bstart[i], g.bstart[i + 1] - g.bstart[i], smem);
}

// ------------------------------------------------------------------------------------ wgrad, 3x3 / 4x4 stride 2 pad 1 (bf16)
// Same idea for stride 2 (the strided convs of the backbone / adversarial heads and the conv-form of the 4x4 transposed
// convs): tap kw of output pixel ox reads input column 2*ox + kw - 1, so the taps fall on TWO column-parity images of the
// input row -- E[j] = x[2j], O[j] = x[2j+1] -- as shifted reads: kw0 = O[ox-1], kw1 = E[ox], kw2 = O[ox], kw3 = E[ox+1].
// Per 64-pixel step a block stages one DY tile and the two parity tiles (as much X data as ONE tap of the generic kernel)
// and multiplies 3 (4) taps out of them.
struct WgradKw2Args {
  const void* X; const void* DY; float* out;
  int H, W, Ho, Ci, Co;
  int lw, lwo;                  // log2(min(Wo,64)), log2(Wo)
  int M, rows_per_split, ldw;
  long slab_stride;
  int nto, nci;
  unsigned x_bytes, dy_bytes;
  FastDiv dHo;
};

template <int MT, int KW>
__global__ __launch_bounds__(256, KW == 4 ? 2 : 3) void wgrad_kw2_kernel(const WgradKw2Args p) {
  constexpr int BO = 64 * MT, BKM = 64;
  constexpr int CPRY = BO / 8, RPY = 256 / CPRY, NPY = BKM / RPY;
  constexpr int XROWS = 64 + 4 * 8 + 4;
  __shared__ __attribute__((aligned(16))) char smem[BKM * 256 + 2 * XROWS * 128 + 2 * BKM * 8];
  char* ys = smem;
  char* xe = smem + BKM * 256;                 // even input columns
  char* xo = xe + XROWS * 128;                 // odd input columns
  int2* rowinfo = reinterpret_cast<int2*>(smem + BKM * 256 + 2 * XROWS * 128);   // [2][BKM]: {input pixel of (2oy, 2ox), oy}

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ntile = p.nto * KW * p.nci;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lid / ntile;
  int tile = lid - split * ntile;
  const int ot = tile / (KW * p.nci); tile -= ot * KW * p.nci;
  const int kh = tile / p.nci, cit = tile - kh * p.nci;
  const int o0 = ot * BO, ci0 = cit * 64, tdy = kh - 1;
  const int wm0 = (wave >> 1) * (32 * MT), wn0 = (wave & 1) * 32;

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.X, p.x_bytes), rsY = make_rsrc(p.DY, p.dy_bytes);
  const int lcy = t % CPRY, lry = t / CPRY;
  const int lcx = t & 7, lrx = t >> 3;
  const bool ook = (o0 + lcy * 8) < p.Co;
  const bool cok = (ci0 + lcx * 8) < p.Ci;
  const int mbeg = split * p.rows_per_split;
  const int mend = min(p.M, mbeg + p.rows_per_split);

  for (int i = t; i < 2 * XROWS * 8; i += 256) reinterpret_cast<uint4*>(xe)[i] = make_uint4(0, 0, 0, 0);

  uint4 ry[NPY], re[2], ro[2];
  auto decode_rows = [&](int mt0, int buf) {
    if (t < BKM) {
      const unsigned m = (unsigned)(mt0 + t);
      const unsigned q = m >> p.lwo, ox = m & ((1u << p.lwo) - 1);
      const unsigned n = fd_div(q, p.dHo);
      const int oy = (int)(q - n * p.Ho);
      rowinfo[buf * BKM + t] = (m < (unsigned)p.M) ? make_int2(((int)n * p.H + 2 * oy) * p.W + 2 * (int)ox, oy) : make_int2(0, -(1 << 20));
    }
  };
  auto load_tile = [&](int mt0, int buf) {
#pragma unroll
    for (int i = 0; i < NPY; ++i) {
      const int m = mt0 + lry + RPY * i;
      ry[i] = buf_load16(rsY, (m < mend && ook) ? (m * p.Co + o0 + lcy * 8) * 2 : OOB_OFF);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int2 ri = rowinfo[buf * BKM + lrx + 32 * i];
      const bool ok = cok && (unsigned)(2 * ri.y + tdy) < (unsigned)p.H;
      const int off = ((ri.x + tdy * p.W) * p.Ci + ci0 + lcx * 8) * 2;
      re[i] = buf_load16(rsX, ok ? off : OOB_OFF);
      ro[i] = buf_load16(rsX, ok ? off + p.Ci * 2 : OOB_OFF);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NPY; ++i) *reinterpret_cast<uint4*>(ys + swz256(lry + RPY * i, lcy)) = ry[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = lrx + 32 * i;
      const int a = swzx(r + 2 + 4 * (r >> p.lw), lcx);
      *reinterpret_cast<uint4*>(xe + a) = re[i];
      *reinterpret_cast<uint4*>(xo + a) = ro[i];
    }
  };

  f32x16_t acc[KW][MT];
#pragma unroll
  for (int a = 0; a < KW; ++a)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][i][r] = 0.f;

  const int r31 = lane & 31, hi = lane >> 5;
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  int trA[MT][2], trB[KW][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = 8 * (tg >> 1) + tq + 4 * u;
#pragma unroll
    for (int i = 0; i < MT; ++i) trA[i][u] = swz256(row, (wm0 + i * 32) / 8 + 2 * (tg & 1) + (tp >> 1)) + 8 * (tp & 1);
    const int R0 = row + 2 + 4 * (row >> p.lw);
    const int ch = wn0 / 8 + 2 * (tg & 1) + (tp >> 1);
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      // kw0 = O[ox-1], kw1 = E[ox], kw2 = O[ox], kw3 = E[ox+1]   (offsets relative to the even image)
      const int shift = k == 0 ? -1 : (k == 3 ? 1 : 0);
      trB[k][u] = swzx(R0 + shift, ch) + 8 * (tp & 1) + ((k & 1) ? 0 : XROWS * 128);
    }
  }
  decode_rows(mbeg, 0);
  __syncthreads();
  if (mbeg < mend) load_tile(mbeg, 0);
  int buf = 0;
  for (int mt0 = mbeg; mt0 < mend; mt0 += BKM, buf ^= 1) {
    __syncthreads();
    store_tile();
    decode_rows(mt0 + BKM, buf ^ 1);
    __syncthreads();
    if (mt0 + BKM < mend) load_tile(mt0 + BKM, buf ^ 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      typedef __attribute__((address_space(3))) bf16x4_t* lds4;
      const int eoff = (16 * s + 4 * ((16 * s) >> p.lw)) * 128;
      bf16x8_t a[MT], b[KW];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        bf16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][0] + s * 4096));
        bf16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ys + trA[i][1] + s * 4096));
        a[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        bf16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xe + trB[k][0] + eoff));
        bf16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(xe + trB[k][1] + eoff));
        b[k] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[k][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[k], acc[k][i], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }
  float* out = p.out + (size_t)split * p.slab_stride;
#pragma unroll
  for (int k = 0; k < KW; ++k)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int c = ci0 + wn0 + r31;
        if (o < p.Co && c < p.Ci) out[(size_t)o * p.ldw + (kh * KW + k) * p.Ci + c] = acc[k][i][r];
      }
}

// Fixed-order slab reduction.  SL "slab lanes" share each float4 column: lane j sums slabs j, j+SL, ... (4 loads in
// flight), the SL partial sums are then added in lane order -- the order depends only on (S, SL), never on timing.
template <int SL>
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, long n, int S,
                                                           long stride, int accumulate) {
  constexpr int COLS = 256 / SL;
  __shared__ float4 part[SL > 1 ? 256 : 1];
  const long n4 = n >> 2;
  const int col = threadIdx.x % COLS, sl = threadIdx.x / COLS;
  for (long i0 = (long)blockIdx.x * COLS; i0 < n4; i0 += (long)gridDim.x * COLS) {
    const long i = i0 + col;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) {
      int s = sl;
      for (; s + 3 * SL < S; s += 4 * SL) {
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = reinterpret_cast<const float4*>(slabs + (size_t)(s + u * SL) * stride)[i];
#pragma unroll
        for (int u = 0; u < 4; ++u) { v.x += a[u].x; v.y += a[u].y; v.z += a[u].z; v.w += a[u].w; }
      }
      for (; s < S; s += SL) { const float4 a = reinterpret_cast<const float4*>(slabs + (size_t)s * stride)[i]; v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
    }
    if constexpr (SL > 1) {
      __syncthreads();
      part[threadIdx.x] = v;
      __syncthreads();
      if (sl == 0 && i < n4) {
        float4 r = accumulate ? reinterpret_cast<const float4*>(out)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < SL; ++j) { const float4 q = part[j * COLS + col]; r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w; }
        reinterpret_cast<float4*>(out)[i] = r;
      }
    } else {
      if (i < n4) {
        if (accumulate) { const float4 o = reinterpret_cast<const float4*>(out)[i]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        reinterpret_cast<float4*>(out)[i] = v;
      }
    }
  }
}
void launch_slab_reduce(const float* ws, float* dw, long n, int S, long stride, int accumulate, hipStream_t st) {
  const long n4 = n / 4;
  // enough slab lanes that ~64K threads stream, but never more lanes than slabs
  int SL = 1;
  while (SL < 16 && n4 * SL < 65536 && SL * 2 <= S) SL *= 2;
  const int cols = 256 / SL;
  dim3 grid(cdiv(n4, cols));
  char lab[64];
  if (prof_on()) snprintf(lab, sizeof(lab), "slab_reduce n%ld S%d", n, S);
  ProfScope ps(st, 0.0, 4.0 * n * (S + 1), 2, prof_on() ? lab : nullptr);
  if (SL == 1) hipLaunchKernelGGL(slab_reduce_kernel<1>, grid, dim3(256), 0, st, ws, dw, n, S, stride, accumulate);
  else if (SL == 2) hipLaunchKernelGGL(slab_reduce_kernel<2>, grid, dim3(256), 0, st, ws, dw, n, S, stride, accumulate);
  else if (SL == 4) hipLaunchKernelGGL(slab_reduce_kernel<4>, grid, dim3(256), 0, st, ws, dw, n, S, stride, accumulate);
  else if (SL == 8) hipLaunchKernelGGL(slab_reduce_kernel<8>, grid, dim3(256), 0, st, ws, dw, n, S, stride, accumulate);
  else hipLaunchKernelGGL(slab_reduce_kernel<16>, grid, dim3(256), 0, st, ws, dw, n, S, stride, accumulate);
}

// plain zero-fill (own kernel rather than hipMemsetAsync: a kernel node replays identically inside HIP graphs)
__global__ void zero_fill_kernel(uint4* __restrict__ p, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------ host side
// describe, choose, launch: the first two are conv_plan.h; what follows maps a chosen ConvBuild to its instantiation.
template <typename T, int BM, int BN, bool SMALL_C, int WGM, int WGN, bool HM_OUT, bool DMA, int EPI, bool KW3 = false, bool CAT = false, int KG = 1>
static void launch_gather_epi(const GatherArgs& a, const ConvBuild& b, hipStream_t st) {
  using SM = GatherSmem<T, BM, BN, DMA ? 2 : 1, KW3>;
  constexpr int smem = SM::kBytes + (KG - 1) * 2 * SM::kStage;
  auto kern = gather_gemm_kernel<T, BM, BN, SMALL_C, WGM, WGN, HM_OUT, DMA, EPI, KW3, CAT, KG>;
  static bool attr_set = false;   // raise the dynamic-LDS cap once per instantiation
  if (!attr_set) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem); attr_set = true; }
  if (prof_on()) { char text[64]; conv_build_text(b, text, sizeof(text)); prof_amend_label("[%s]", text); }
  hipLaunchKernelGGL(kern, dim3(a.ntiles), dim3(64 * WGM * WGN * KG), smem, st, a);
}

// `b` names this instantiation (launch_gather_build, heatmap_conv): its tile grid and epilogue, then the launch
template <typename T, int BM, int BN, bool SMALL_C, int WGM = 2, int WGN = 2, bool HM_OUT = false, bool DMA = false, bool KW3 = false, bool CAT = false, int KG = 1>
static void launch_gather(GatherArgs& a, ConvBuild b, hipStream_t st) {
  plan_gather_launch(a, b, conv_knobs());
  if constexpr (gather_has_bnb(BM, HM_OUT, KW3, CAT, KG)) {
    if (b.epi == 2) { launch_gather_epi<T, BM, BN, SMALL_C, WGM, WGN, HM_OUT, DMA, 2>(a, b, st); return; }
  }
  if constexpr (gather_has_stats(BM, BN, HM_OUT, DMA)) {
    if (b.epi == 1) { launch_gather_epi<T, BM, BN, SMALL_C, WGM, WGN, HM_OUT, DMA, 1, KW3, CAT, KG>(a, b, st); return; }
  }
  launch_gather_epi<T, BM, BN, SMALL_C, WGM, WGN, HM_OUT, DMA, 0, KW3, CAT, KG>(a, b, st);
}

// Every build of the gather kernel the chooser can name (the heat-map build has its own entry point, heatmap_conv):
//   BM, BN, small-channel, waves along M, waves along N, LDS-DMA, shared A tile, concat-K, K groups, bf16 only
#define GATHER_BUILDS(X) \
  X(128,  64, true,  2, 2, false, false, false, 1, false) \
  X(128, 128, false, 2, 2, false, false, false, 1, false) \
  X( 64, 128, false, 2, 2, false, false, false, 1, false) \
  X(128,  64, false, 2, 2, false, false, false, 1, false) \
  X( 64,  64, false, 2, 2, false, false, false, 1, false) \
  X(128, 128, false, 2, 2, true,  false, false, 1, false) \
  X( 64, 128, false, 2, 2, true,  false, false, 2, false) \
  X(128, 128, false, 2, 2, true,  false, false, 2, false) \
  X(256, 256, false, 2, 4, false, false, false, 1, false) \
  X(256, 256, false, 2, 4, true,  false, false, 1, true)  \
  X(128,  64, false, 2, 2, false, true,  false, 1, true)  \
  X(128, 128, false, 2, 2, false, true,  false, 1, true)  \
  X(256, 128, false, 2, 2, false, true,  false, 1, true)  \
  X( 64,  64, false, 2, 2, false, false, true,  1, false) \
  X( 64, 128, false, 2, 2, false, false, true,  1, false) \
  X(128, 128, false, 2, 2, false, false, true,  1, false) \
  X(128, 128, false, 2, 2, true,  false, true,  1, false) \
  X(256, 256, false, 2, 4, true,  false, true,  1, true)
template <typename T>
static bool launch_gather_build(GatherArgs& a, const ConvBuild& b, hipStream_t st) {
#define X(BM, BN, SMALL_C, WGM, WGN, DMA, KW3, CAT, KG, BF16_ONLY) \
  if (b.bm == BM && b.bn == BN && b.small_c == SMALL_C && b.dma == DMA && b.kw3 == KW3 && b.cat == CAT && b.kg == KG) { \
    if constexpr (!BF16_ONLY || sizeof(T) == 2) { launch_gather<T, BM, BN, SMALL_C, WGM, WGN, false, DMA, KW3, CAT, KG>(a, b, st); return true; } \
  }
  GATHER_BUILDS(X)
#undef X
  return false;
}

template <typename T>
static int dispatch_gather(GatherArgs& a, hipStream_t st) {
  constexpr int CH = MmaTraits<T>::CH;
  if (a.Ci % CH) MI_FAIL(MI355_EINVAL, "gather: Ci=%d not a multiple of %d", a.Ci, CH);
  a.cshift = ilog2_exact(a.Ci / CH);
  if (a.cshift < 0) MI_FAIL(MI355_EINVAL, "gather: Ci/%d must be a power of two (Ci=%d)", CH, a.Ci);
  if (a.Nout % CH) MI_FAIL(MI355_EINVAL, "gather: Nout=%d not a multiple of %d", a.Nout, CH);
  if (a.nphase < 1 || a.nphase > 4) MI_FAIL(MI355_EINVAL, "gather: nphase=%d", a.nphase);
  long Mtot = 0, ntaps_tot = 0; double flops = 0.0;
  for (int i = 0; i < a.nphase; ++i) {
    Mtot += a.ph[i].M; ntaps_tot += a.ph[i].ntaps;
    flops += 2.0 * a.ph[i].M * (double)a.Nout * a.ph[i].ntaps * a.Ci;
  }
  {
    // A spans [images][Hi][Wi][Ci]; images = M / (OHp*OWp)
    const long imgs = a.ph[0].M / ((long)a.ph[0].OHp * a.ph[0].OWp);
    a.a_bytes = (unsigned)(imgs * a.Hi * a.Wi * a.Ci * (long)sizeof(T));
    a.b_bytes = (unsigned)((long)a.Nout * a.ldb * (long)sizeof(T));
  }
  // algorithmic bytes: every input element, weight and output element once
  if (a.A2) flops += 2.0 * Mtot * (double)a.Nout * a.c2;
  ProfScope ps(st, flops, (double)a.a_bytes + (double)a.b_bytes * ntaps_tot / (a.ldb / a.Ci) + (double)Mtot * a.Nout * sizeof(T) +
                              (a.A2 ? (double)a.a2_bytes + a.b2_bytes : 0.0));
  if (a.A2) {
    if ((a.Ci / CH) < 8 || a.nphase != 1 || a.out_sx != 1 || a.out_sy != 1 || a.bnb_partial || a.residual || a.accumulate)
      MI_FAIL(MI355_EINVAL, "concat-K forward: plain single-phase forward conv with >= 8 input chunks only");
    if (a.c2 < CH || a.c2 % CH || a.c2 > MmaTraits<T>::BK) MI_FAIL(MI355_EINVAL, "concat-K forward: c2=%d must be a multiple of %d and <= %d", a.c2, CH, MmaTraits<T>::BK);
  }
  const ConvBuild b = choose_conv(a, (int)sizeof(T), conv_knobs());
  if (b.family == CONV_PGEMM) return launch_pgemm_build(a, b, st);
  if (!launch_gather_build<T>(a, b, st)) MI_FAIL(MI355_EINVAL, "gather: no such build (%dx%d)", b.bm, b.bn);
  MI_CHECK_LAUNCH(b.cat ? "gather_gemm_cat" : "gather_gemm");
  return MI355_OK;
}

// crop_ok: the entry point also takes a CROPPED output -- the top-left Ho x Wo outputs of a unit-stride conv (forward and weight
// gradient only).  That is how the 7x7 / stride-2 stem runs as a 4x4 conv over the space-to-depth image (window rows -2 .. +1:
// pad 2, the 129th output row / column never computed).
static int check_desc(const mi355_conv_desc* d, bool crop_ok = false) {
  if (!d) MI_FAIL(MI355_EINVAL, "null conv desc");
  if (d->dtype != MI355_F32 && d->dtype != MI355_BF16 && d->dtype != MI355_FP8) MI_FAIL(MI355_EINVAL, "bad dtype %d", d->dtype);
  if (d->kh * d->kw > MAX_TAPS || d->kh < 1 || d->kw < 1) MI_FAIL(MI355_EINVAL, "unsupported kernel %dx%d", d->kh, d->kw);
  if (d->stride < 1 || d->stride > 2) MI_FAIL(MI355_EINVAL, "unsupported stride %d", d->stride);
  const int fho = (d->Hi + 2 * d->pad - d->kh) / d->stride + 1, fwo = (d->Wi + 2 * d->pad - d->kw) / d->stride + 1;
  const bool cropped = crop_ok && d->stride == 1 && d->kh > 1 && d->dtype != MI355_FP8 && d->Ho >= 1 && d->Wo >= 1 && d->Ho <= fho && d->Wo <= fwo;
  if (!cropped && (d->Ho != fho || d->Wo != fwo))
    MI_FAIL(MI355_EINVAL, "conv desc: output size %dx%d inconsistent with input %dx%d k%d s%d p%d", d->Ho, d->Wo, d->Hi, d->Wi, d->kh, d->stride, d->pad);
  // the kernels form signed 32-bit BYTE offsets and 32-bit buffer-resource sizes: bound bytes, not elements
  const long esz = d->dtype == MI355_F32 ? 4 : 2;      // (fp8 operands, bf16 results: bound by the wider side)
  if ((long)d->N * d->Hi * d->Wi * d->Ci * esz >= (1L << 31) || (long)d->N * d->Ho * d->Wo * d->Co * esz >= (1L << 31))
    MI_FAIL(MI355_EINVAL, "tensor too large for 32-bit byte offsets (%ld / %ld bytes): split the batch",
            (long)d->N * d->Hi * d->Wi * d->Ci * esz, (long)d->N * d->Ho * d->Wo * d->Co * esz);
  return MI355_OK;
}

static void set_bnb(GatherArgs& a, const mi355_bn_bwd_src* bn, float* partial, size_t partial_bytes) {
  a.bnb_x = bn->x; a.bnb_y = bn->relu ? bn->y : nullptr;
  a.bnb_mean = bn->save_mean; a.bnb_invstd = bn->save_invstd; a.bnb_gamma = bn->gamma; a.bnb_beta = bn->beta;
  a.bnb_relu = bn->relu ? (bn->y ? 1 : 2) : 0;
  a.bnb_partial = partial; a.stat_bytes = partial_bytes;
}
static int check_bnb(const mi355_bn_bwd_src* bn, const float* partial, const int* nslices) {
  if (!bn || !partial || !nslices || !bn->x || !bn->save_mean || !bn->save_invstd)
    MI_FAIL(MI355_EINVAL, "bnbwd fusion: bn source / partial / nslices must be given");
  if (bn->relu && !bn->y && (!bn->gamma || !bn->beta)) MI_FAIL(MI355_EINVAL, "bnbwd fusion: relu without y needs gamma and beta");
  return MI355_OK;
}
// fp8 operand launches: device scalars undoing the operand scales, and the format of the gathered operand
// (MX: block scales sa / sb instead of the descales, e4m3 operands; mx_fp8.hip)
// act: the MX inference epilogue (bias, residual, ReLU; no statistics), y8 / sy its optional MX copy of the output
struct Fp8Extra { const float* descale_a; const float* descale_b; int a_fmt; const void* sa = nullptr; const void* sb = nullptr;
                  bool act = false; void* y8 = nullptr; void* sy = nullptr; };
struct CatExtra { const void* x2; const void* w2; const float* bias2; int c2; };
static int dispatch_conv(GatherArgs& a, const mi355_conv_desc* d, const Fp8Extra* f8, hipStream_t st) {
  if (f8) { a.scale2 = f8->descale_a; a.scale3 = f8->descale_b; a.a_fmt = f8->a_fmt; a.mx_sa = f8->sa; a.mx_sb = f8->sb;
            a.mx_act = f8->act ? 1 : 0; a.mx_y8 = f8->y8; a.mx_sy = f8->sy; return dispatch_gather_fp8(a, st); }
  return d->dtype == MI355_BF16 ? dispatch_gather<bf16_t>(a, st) : dispatch_gather<float>(a, st);
}
static int conv_fwd_impl(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, const void* residual, void* y,
                         float* partial, size_t partial_bytes, int* nslices, void* stream, const mi355_bn_bwd_src* bn = nullptr,
                         const Fp8Extra* f8 = nullptr, int relu = 0, const CatExtra* cat = nullptr) {
  if (int e = check_desc(d, true)) return e;
  if ((d->dtype == MI355_FP8) != (f8 != nullptr)) MI_FAIL(MI355_EINVAL, "fp8 descriptors go through the *_fp8 entry points (and only they)");
  if (relu && (bn || (f8 && !f8->act) || partial)) MI_FAIL(MI355_EINVAL, "conv_fwd: the fused ReLU is an inference epilogue (no statistics / BatchNorm-backward / fp8 variant)");
  GatherArgs a; memset(&a, 0, sizeof(a));
  if (prof_on()) prof_set_tag("fwd%s k%ds%d %d>%d @%dx%d n%d%s%s%s", f8 ? (f8->sa ? (f8->y8 ? "mx+q" : "mx") : "8") : "", d->kh, d->stride, d->Ci, d->Co, d->Hi, d->Wi, d->N, partial ? " +stats" : "",
                              residual ? " +res" : "", cat ? " +cat" : "");
  a.relu = relu ? 1 : 0;
  a.A = x; a.B = w; a.D = y; a.bias = bias; a.residual = residual; a.scale = nullptr; a.accumulate = 0;
  describe_fwd(a, d);
  if (bn) set_bnb(a, bn, partial, partial_bytes);
  else { a.stat_partial = partial; a.stat_bytes = partial_bytes; }
  if (cat) {
    const long esz = d->dtype == MI355_F32 ? 4 : 2;
    a.A2 = cat->x2; a.B2 = cat->w2; a.bias2 = cat->bias2; a.c2 = cat->c2;
    a.a2_bytes = (unsigned)((long)d->N * d->Ho * d->Wo * cat->c2 * esz); a.b2_bytes = (unsigned)((long)d->Co * cat->c2 * esz);
  }
  const int e = dispatch_conv(a, d, f8, as_stream(stream));
  if (nslices) *nslices = a.stat_slices;
  return e;
}
extern "C" int mi355_conv_fwd_fp8(const mi355_conv_desc* d, const void* x8, int x_fmt, const void* w8, const float* descale_x,
                                  const float* descale_w, const float* bias, const void* residual, void* y, float* partial,
                                  size_t partial_bytes, int* nslices, void* stream) {
  if (!descale_x || !descale_w || (x_fmt != 0 && x_fmt != 1)) MI_FAIL(MI355_EINVAL, "conv_fwd_fp8: descale scalars / format missing");
  if (nslices) *nslices = 0;
  Fp8Extra f8{descale_x, descale_w, x_fmt};
  return conv_fwd_impl(d, x8, w8, bias, residual, y, partial, partial_bytes, nslices, stream, nullptr, &f8);
}
// MX operands (mx_fp8.hip): e4m3 x8 [N][Hi][Wi][Ci] with scales sx [N][Hi][Wi][Ci/32], w8 [Co][T][Ci] with sw [Co][T][Ci/32]
extern "C" int mi355_conv_fwd_mx(const mi355_conv_desc* d, const void* x8, const void* sx, const void* w8, const void* sw,
                                 const float* bias, const void* residual, void* y, float* partial, size_t partial_bytes,
                                 int* nslices, void* stream) {
  if (nslices) *nslices = 0;
  if (!d || !x8 || !sx || !w8 || !sw || !y) MI_FAIL(MI355_EINVAL, "conv_fwd_mx: null descriptor, operand, scale or output");
  if (d->dtype != MI355_FP8) MI_FAIL(MI355_EINVAL, "conv_fwd_mx: the descriptor's dtype must be MI355_FP8");
  if (d->Ci < 128 || d->Ci % 128 || (d->Ci & (d->Ci - 1))) MI_FAIL(MI355_EINVAL, "conv_fwd_mx: Ci=%d (contracted) must be a power-of-two multiple of 128", d->Ci);
  if (d->Co < 8 || d->Co % 8) MI_FAIL(MI355_EINVAL, "conv_fwd_mx: Co=%d must be a multiple of 8", d->Co);
  if ((partial == nullptr) != (nslices == nullptr)) MI_FAIL(MI355_EINVAL, "conv_fwd_mx: partial and nslices go together");
  Fp8Extra f8{nullptr, nullptr, 0, sx, sw};
  return conv_fwd_impl(d, x8, w8, bias, residual, y, partial, partial_bytes, nslices, stream, nullptr, &f8);
}
// the MX copy an act launch writes beside its bf16 output of `C` channels: both pointers or neither, whole 32-channel blocks
static int check_mx_copy(const char* who, const void* y8, const void* sy, int C) {
  if ((y8 == nullptr) != (sy == nullptr)) MI_FAIL(MI355_EINVAL, "%s: the MX copy of the output takes both its elements and its scales", who);
  if (y8 && C % 32) MI_FAIL(MI355_EINVAL, "%s: an MX copy of the output needs a multiple of 32 output channels (%d)", who, C);
  if (y8 && (uintptr_t)y8 % 8) MI_FAIL(MI355_EINVAL, "%s: the element buffer of the MX copy must be 8-byte aligned", who);
  return MI355_OK;
}
// inference on MX operands: y = act(conv(x8, w8) + bias + residual) with the BatchNorm that follows folded into w8 / bias by the
// caller (as mi355_conv_fwd_act), and optionally the MX copy (y8, sy) of that y for the next MX layer
extern "C" int mi355_conv_fwd_mx_act(const mi355_conv_desc* d, const void* x8, const void* sx, const void* w8, const void* sw,
                                     const float* bias, const void* residual, int relu, void* y, void* y8, void* sy, void* stream) {
  if (!d || !x8 || !sx || !w8 || !sw || !y) MI_FAIL(MI355_EINVAL, "conv_fwd_mx_act: null descriptor, operand, scale or output");
  if (d->dtype != MI355_FP8) MI_FAIL(MI355_EINVAL, "conv_fwd_mx_act: the descriptor's dtype must be MI355_FP8");
  if (d->Ci < 128 || d->Ci % 128 || (d->Ci & (d->Ci - 1))) MI_FAIL(MI355_EINVAL, "conv_fwd_mx_act: Ci=%d (contracted) must be a power-of-two multiple of 128", d->Ci);
  if (d->Co < 8 || d->Co % 8) MI_FAIL(MI355_EINVAL, "conv_fwd_mx_act: Co=%d must be a multiple of 8", d->Co);
  if (int e = check_mx_copy("conv_fwd_mx_act", y8, sy, d->Co)) return e;
  Fp8Extra f8{nullptr, nullptr, 0, sx, sw, true, y8, sy};
  return conv_fwd_impl(d, x8, w8, bias, residual, y, nullptr, 0, nullptr, stream, nullptr, &f8, relu);
}
extern "C" int mi355_conv_fwd(const mi355_conv_desc* d, const void* x, const void* w, const float* bias,
                              const void* residual, void* y, void* stream) {
  return conv_fwd_impl(d, x, w, bias, residual, y, nullptr, 0, nullptr, stream);
}
// inference: y = act(conv(x) + bias + residual) -- with the BatchNorm that follows folded into w / bias by the caller
extern "C" int mi355_conv_fwd_act(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, const void* residual,
                                  int relu, void* y, void* stream) {
  return conv_fwd_impl(d, x, w, bias, residual, y, nullptr, 0, nullptr, stream, nullptr, nullptr, relu);
}
extern "C" int mi355_conv_fwd_stats(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                                    float* partial, size_t partial_bytes, int* nslices, void* stream) {
  if (!partial || !nslices) MI_FAIL(MI355_EINVAL, "conv_fwd_stats: partial / nslices must be given");
  return conv_fwd_impl(d, x, w, bias, nullptr, y, partial, partial_bytes, nslices, stream);
}
// y = conv(x, w) + x2 * w2^T + bias + bias2 as ONE implicit GEMM (K = kh*kw*Ci + c2): x2 [N*Ho*Wo][c2] at the OUTPUT resolution,
// w2 [Co][c2], both in the descriptor's dtype, c2 a multiple of the 16-byte chunk and <= one K tile (64 bf16 / 32 fp32).
// partial / nslices: nullable pair, BatchNorm statistics of y from the epilogue as in mi355_conv_fwd_stats.
extern "C" int mi355_conv_fwd_cat(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, const void* x2,
                                  const void* w2, const float* bias2, int c2, void* y, float* partial, size_t partial_bytes,
                                  int* nslices, void* stream) {
  if (!x2 || !w2 || c2 < 1) MI_FAIL(MI355_EINVAL, "conv_fwd_cat: second operand pair missing");
  if ((partial == nullptr) != (nslices == nullptr)) MI_FAIL(MI355_EINVAL, "conv_fwd_cat: partial and nslices go together");
  if (d && d->dtype == MI355_FP8) MI_FAIL(MI355_EINVAL, "conv_fwd_cat: bf16 / fp32 descriptors only");
  if (nslices) *nslices = 0;
  CatExtra cat{x2, w2, bias2, c2};
  return conv_fwd_impl(d, x, w, bias, nullptr, y, partial, partial_bytes, nslices, stream, nullptr, nullptr, 0, &cat);
}
// ConvTranspose2d input gradient (= conv-form forward) producing the dy of a BatchNorm: its backward reduction in the epilogue
extern "C" int mi355_conv_fwd_bnbwd(const mi355_conv_desc* d, const void* x, const void* w, void* y, const mi355_bn_bwd_src* bn,
                                    float* partial, size_t partial_bytes, int* nslices, void* stream) {
  if (int e = check_bnb(bn, partial, nslices)) return e;
  return conv_fwd_impl(d, x, w, nullptr, nullptr, y, partial, partial_bytes, nslices, stream, bn);
}
// capacity that always suffices for the fused statistics of a conv output / deconv output (smallest tile = 64 rows)
extern "C" size_t mi355_conv_stats_bytes(long rows, int C) { return conv_stats_bytes(rows, C); }

// 1x1 conv C -> K (K <= 32) written as NCHW fp32 heat-maps: y[n][k][p] = bias[k] + sum_c x[n*HW+p][c] * w[k][c]
template <typename T>
static int heatmap_conv(const void* x, const void* w, const float* bias, float* y, int N, int HW, int C, int K, hipStream_t st) {
  constexpr int CH = MmaTraits<T>::CH;
  GatherArgs a; memset(&a, 0, sizeof(a));
  a.A = x; a.B = w; a.D = y; a.bias = bias;
  a.Hi = 1; a.Wi = HW; a.Ci = C; a.in_sy = a.in_sx = 1;
  a.Ho = 1; a.Wo = HW; a.out_sy = a.out_sx = 1; a.ldd = 1; a.hw = HW;
  a.Nout = K; a.ldb = C;
  a.nphase = 1; a.ph[0].OHp = 1; a.ph[0].OWp = HW; a.ph[0].M = N * HW; a.ph[0].ntaps = 1;
  if (C % CH) MI_FAIL(MI355_EINVAL, "conv1x1_heatmap: C=%d not a multiple of %d", C, CH);
  a.cshift = ilog2_exact(C / CH);
  if (a.cshift < 3) MI_FAIL(MI355_EINVAL, "conv1x1_heatmap: C/%d must be a power of two >= 8 (C=%d)", CH, C);
  a.a_bytes = (unsigned)((long)N * HW * C * (long)sizeof(T));
  a.b_bytes = (unsigned)((long)K * C * (long)sizeof(T));
  if (prof_on()) prof_set_tag("hm1x1 %d>%d hw%d n%d", C, K, HW, N);
  ProfScope ps(st, 2.0 * N * HW * (double)K * C, (double)a.a_bytes + a.b_bytes + 4.0 * N * HW * K);
  ConvBuild b;
  b.bm = 128; b.bn = 32; b.f32 = sizeof(T) == 4; b.hm = true;
  launch_gather<T, 128, 32, false, 4, 1, true>(a, b, st);
  MI_CHECK_LAUNCH("conv1x1_heatmap");
  return MI355_OK;
}
extern "C" int mi355_conv1x1_heatmap(const void* x, const void* w, const float* bias, float* y, int N, int HW, int C, int K,
                                     int dtype, void* stream) {
  if (!x || !w || !y || N < 1 || HW < 1 || K < 1 || K > 32) MI_FAIL(MI355_EINVAL, "conv1x1_heatmap: bad args");
  if ((long)N * HW * C >= (1L << 31)) MI_FAIL(MI355_EINVAL, "conv1x1_heatmap: tensor too large");
  return dtype == MI355_BF16 ? heatmap_conv<bf16_t>(x, w, bias, y, N, HW, C, K, as_stream(stream))
       : dtype == MI355_F32 ? heatmap_conv<float>(x, w, bias, y, N, HW, C, K, as_stream(stream))
       : (mi355_set_error("bad dtype"), MI355_EINVAL);
}

// conv-form dgrad (describe_dgrad): stride^2 phases in one launch
static int conv_dgrad_impl(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias, const float* scale_dev,
                           int accumulate, void* dx, float* partial, size_t partial_bytes, int* nslices, void* stream,
                           const mi355_bn_bwd_src* bn = nullptr, const Fp8Extra* f8 = nullptr, const void* acc_mask = nullptr,
                           int relu = 0);
extern "C" int mi355_conv_dgrad_fp8(const mi355_conv_desc* d, const void* dy8, int dy_fmt, const void* wT8, const float* descale_dy,
                                    const float* descale_w, const float* scale_dev, int accumulate, void* dx, float* partial,
                                    size_t partial_bytes, int* nslices, void* stream) {
  if (!descale_dy || !descale_w || (dy_fmt != 0 && dy_fmt != 1)) MI_FAIL(MI355_EINVAL, "conv_dgrad_fp8: descale scalars / format missing");
  Fp8Extra f8{descale_dy, descale_w, dy_fmt};
  return conv_dgrad_impl(d, dy8, wT8, nullptr, scale_dev, accumulate, dx, partial, partial_bytes, nslices, stream, nullptr, &f8);
}
// MX operands: e4m3 dy8 [N][Ho][Wo][Co] with sdy [N][Ho][Wo][Co/32], wT8 [Ci][T][Co] with swT [Ci][T][Co/32]
extern "C" int mi355_conv_dgrad_mx(const mi355_conv_desc* d, const void* dy8, const void* sdy, const void* wT8, const void* swT,
                                   const float* scale_dev, int accumulate, void* dx, float* partial, size_t partial_bytes,
                                   int* nslices, void* stream) {
  if (nslices) *nslices = 0;
  if (!d || !dy8 || !sdy || !wT8 || !swT || !dx) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: null descriptor, operand, scale or output");
  if (d->dtype != MI355_FP8) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: the descriptor's dtype must be MI355_FP8");
  if (d->Co < 128 || d->Co % 128 || (d->Co & (d->Co - 1))) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: Co=%d (contracted) must be a power-of-two multiple of 128", d->Co);
  if (d->Ci < 8 || d->Ci % 8) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: Ci=%d must be a multiple of 8", d->Ci);
  if ((partial == nullptr) != (nslices == nullptr)) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: partial and nslices go together");
  if (accumulate != 0 && accumulate != 1) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx: accumulate %d", accumulate);
  if (int e = check_desc(d)) return e;       // (before the zero fill of a phase without taps)
  Fp8Extra f8{nullptr, nullptr, 0, sdy, swT};
  return conv_dgrad_impl(d, dy8, wT8, nullptr, scale_dev, accumulate, dx, partial, partial_bytes, nslices, stream, nullptr, &f8);
}
// inference ConvTranspose2d forward on MX operands: dx = act(dgrad(dy8) + bias), optionally with the MX copy (dx8, sdx) of dx
extern "C" int mi355_conv_dgrad_mx_act(const mi355_conv_desc* d, const void* dy8, const void* sdy, const void* wT8, const void* swT,
                                       const float* bias, int relu, void* dx, void* dx8, void* sdx, void* stream) {
  if (!d || !dy8 || !sdy || !wT8 || !swT || !dx) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx_act: null descriptor, operand, scale or output");
  if (d->dtype != MI355_FP8) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx_act: the descriptor's dtype must be MI355_FP8");
  if (d->Co < 128 || d->Co % 128 || (d->Co & (d->Co - 1))) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx_act: Co=%d (contracted) must be a power-of-two multiple of 128", d->Co);
  if (d->Ci < 8 || d->Ci % 8) MI_FAIL(MI355_EINVAL, "conv_dgrad_mx_act: Ci=%d must be a multiple of 8", d->Ci);
  if (int e = check_mx_copy("conv_dgrad_mx_act", dx8, sdx, d->Ci)) return e;
  if (int e = check_desc(d)) return e;
  {   // every output pixel must come out of the launch: a zero-filled parity would carry neither the bias nor a copy
    GatherArgs probe; memset(&probe, 0, sizeof(probe));
    if (describe_dgrad(probe, d) || probe.nphase != d->stride * d->stride)
      MI_FAIL(MI355_EINVAL, "conv_dgrad_mx_act: k%d s%d p%d leaves output pixels without a tap", d->kh, d->stride, d->pad);
  }
  Fp8Extra f8{nullptr, nullptr, 0, sdy, swT, true, dx8, sdx};
  return conv_dgrad_impl(d, dy8, wT8, bias, nullptr, 0, dx, nullptr, 0, nullptr, stream, nullptr, &f8, nullptr, relu);
}
// conv input gradient that is the dy of a BatchNorm: that BatchNorm's backward reduction in the epilogue
extern "C" int mi355_conv_dgrad_bnbwd(const mi355_conv_desc* d, const void* dy, const void* wT, const float* scale_dev, int accumulate,
                                      void* dx, const mi355_bn_bwd_src* bn, float* partial, size_t partial_bytes, int* nslices,
                                      void* stream) {
  if (int e = check_bnb(bn, partial, nslices)) return e;
  return conv_dgrad_impl(d, dy, wT, nullptr, scale_dev, accumulate, dx, partial, partial_bytes, nslices, stream, bn);
}
extern "C" int mi355_conv_dgrad(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias,
                                const float* scale_dev, int accumulate, void* dx, void* stream) {
  return conv_dgrad_impl(d, dy, wT, bias, scale_dev, accumulate, dx, nullptr, 0, nullptr, stream);
}
// dx <- dgrad + (bit of acc_mask set ? dx : 0): the fork of a residual block whose other branch's gradient is still the
// UNMASKED dy of the block's final ReLU -- BatchNorm's backward then need not write the masked copy (mi355_bn_bwd dresidual)
extern "C" int mi355_conv_dgrad_masked_acc(const mi355_conv_desc* d, const void* dy, const void* wT, const float* scale_dev, void* dx,
                                           const void* acc_mask, void* stream) {
  if (!acc_mask) MI_FAIL(MI355_EINVAL, "conv_dgrad_masked_acc: acc_mask is null");
  return conv_dgrad_impl(d, dy, wT, nullptr, scale_dev, 1, dx, nullptr, 0, nullptr, stream, nullptr, nullptr, acc_mask);
}
// inference ConvTranspose2d forward: dx = act(dgrad(dy) + bias) with the following BatchNorm folded into wT / bias
extern "C" int mi355_conv_dgrad_act(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias, int relu, void* dx,
                                    void* stream) {
  return conv_dgrad_impl(d, dy, wT, bias, nullptr, 0, dx, nullptr, 0, nullptr, stream, nullptr, nullptr, nullptr, relu);
}
// ConvTranspose2d forward (= conv-form dgrad) with the BatchNorm statistics of its output fused into the epilogue
extern "C" int mi355_conv_dgrad_stats(const mi355_conv_desc* d, const void* dy, const void* wT, void* dx, float* partial,
                                      size_t partial_bytes, int* nslices, void* stream) {
  if (!partial || !nslices) MI_FAIL(MI355_EINVAL, "conv_dgrad_stats: partial / nslices must be given");
  return conv_dgrad_impl(d, dy, wT, nullptr, nullptr, 0, dx, partial, partial_bytes, nslices, stream);
}
static int conv_dgrad_impl(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias, const float* scale_dev,
                           int accumulate, void* dx, float* partial, size_t partial_bytes, int* nslices, void* stream,
                           const mi355_bn_bwd_src* bn, const Fp8Extra* f8, const void* acc_mask, int relu) {
  if (nslices) *nslices = 0;
  if (relu && (bn || (f8 && !f8->act) || partial || accumulate)) MI_FAIL(MI355_EINVAL, "conv_dgrad: the fused ReLU is an inference epilogue of the transposed conv");
  if (acc_mask && (!accumulate || bn || f8)) MI_FAIL(MI355_EINVAL, "conv_dgrad: acc_mask goes with accumulate = 1 on the plain bf16 / fp32 path only");
  if (int e = check_desc(d)) return e;
  if ((d->dtype == MI355_FP8) != (f8 != nullptr)) MI_FAIL(MI355_EINVAL, "fp8 descriptors go through the *_fp8 entry points (and only they)");
  if (f8 && bn) MI_FAIL(MI355_EINVAL, "fp8 dgrad: no BatchNorm-backward epilogue");
  hipStream_t st = as_stream(stream);
  const int s = d->stride;
  GatherArgs a; memset(&a, 0, sizeof(a));
  const bool need_zero = describe_dgrad(a, d);
  if (need_zero && !accumulate) {
    const size_t esz = d->dtype == MI355_F32 ? 4 : 2;        // dx element size (bf16 for fp8 operands)
    const size_t n16 = (size_t)d->N * d->Hi * d->Wi * d->Ci * esz / 16;   // Ci*esz is a multiple of 16
    int grid = (int)((n16 + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(zero_fill_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<uint4*>(dx), n16);
    MI_CHECK_LAUNCH("zero_fill");
  }
  auto tag = [&]() {      // (a launch consumes the pending tag: the per-phase launches below set it once each)
    if (prof_on()) prof_set_tag("dgrad%s k%ds%d %d>%d @%dx%d n%d%s%s%s", f8 ? (f8->sa ? (f8->y8 ? "mx+q" : "mx") : "8") : "", d->kh, d->stride, d->Ci, d->Co, d->Hi, d->Wi, d->N, partial ? " +stats" : "",
                                accumulate ? (acc_mask ? " +macc" : " +acc") : "", bn ? " +bnb" : "");
  };
  tag();
  a.A = dy; a.B = wT; a.D = dx; a.bias = bias; a.residual = nullptr; a.scale = scale_dev;
  a.accumulate = accumulate ? 1 : 0;
  a.acc_mask = reinterpret_cast<const unsigned char*>(acc_mask);
  a.relu = relu ? 1 : 0;
  if (a.nphase == 0) return MI355_OK;
  if (conv_knobs().phases || a.nphase == 1) {      // (MI355_PHASES=0: one launch per phase, A/B)
    if (bn) set_bnb(a, bn, partial, partial_bytes);   // (zero-filled phases carry dy = 0: they add nothing to the sums)
    else if (partial && dgrad_fuses_stats(a, s, need_zero)) { a.stat_partial = partial; a.stat_bytes = partial_bytes; }
    const int e = dispatch_conv(a, d, f8, st);
    if (nslices) *nslices = a.stat_slices;
    return e;
  }
  if (f8) MI_FAIL(MI355_EINVAL, "fp8 dgrad: MI355_PHASES=0 is a bf16 / fp32 experiment switch");
  const int np = a.nphase;
  for (int i = 0; i < np; ++i) {
    GatherArgs b = a; b.nphase = 1; b.ph[0] = a.ph[i];
    if (i) tag();
    if (int e = dispatch_conv(b, d, nullptr, st)) return e;
  }
  return MI355_OK;
}

// argument blocks of the three weight-gradient kernels: `out` is dw or the item's slabs, `rows` the rows per split
template <typename Args>
static void fill_wgrad_common(Args& a, const mi355_conv_desc* d, const WgradPlan& w, const void* x, const void* dy, float* out, int rows) {
  memset(&a, 0, sizeof(a));
  a.X = x; a.DY = dy; a.out = out; a.Ci = d->Ci; a.Co = d->Co;
  a.M = d->N * d->Ho * d->Wo; a.rows_per_split = rows; a.ldw = w.ldw; a.slab_stride = (long)d->Co * w.ldw; a.nto = w.nto;
  const long esz = d->dtype == MI355_BF16 ? 2 : 4;
  a.x_bytes = (unsigned)((long)d->N * d->Hi * d->Wi * d->Ci * esz); a.dy_bytes = (unsigned)((long)a.M * d->Co * esz);
}
static void fill_wgrad_args(WgradArgs& a, const mi355_conv_desc* d, const WgradPlan& w, const void* x, const void* dy, float* out, int rows) {
  fill_wgrad_common(a, d, w, x, dy, out, rows);
  a.Hi = d->Hi; a.Wi = d->Wi; a.Ho = d->Ho; a.Wo = d->Wo; a.nti = w.nti;
  a.kw = d->kw; a.stride = d->stride; a.pad = d->pad; a.cshift = ilog2_exact(d->Ci / (d->dtype == MI355_BF16 ? 8 : 4));
  a.dWo = make_fastdiv(d->Wo); a.dHo = make_fastdiv(d->Ho);
}
static void fill_wgrad_args(WgradKwArgs& k, const mi355_conv_desc* d, const WgradPlan& w, const void* x, const void* dy, float* out, int rows) {
  fill_wgrad_common(k, d, w, x, dy, out, rows);
  k.H = d->Hi; k.W = d->Wi; k.nci = w.nti;
  k.lwf = ilog2_exact(d->Wi); k.lw = k.lwf > 6 ? 6 : k.lwf; k.halo = d->Wi > 64;
  k.dH = make_fastdiv(d->Hi);
}
static void fill_wgrad_args(WgradKw2Args& k, const mi355_conv_desc* d, const WgradPlan& w, const void* x, const void* dy, float* out, int rows) {
  fill_wgrad_common(k, d, w, x, dy, out, rows);
  k.H = d->Hi; k.W = d->Wi; k.Ho = d->Ho; k.nci = w.nti;
  k.lwo = ilog2_exact(d->Wo); k.lw = k.lwo > 6 ? 6 : k.lwo;
  k.dHo = make_fastdiv(d->Ho);
}
static int check_wgrad_channels(const mi355_conv_desc* d) {
  const int CH = d->dtype == MI355_BF16 ? 8 : 4;
  if (d->Ci % CH || d->Co % CH) MI_FAIL(MI355_EINVAL, "wgrad: channels must be multiples of %d", CH);
  if (ilog2_exact(d->Ci / CH) < 0) MI_FAIL(MI355_EINVAL, "wgrad: Ci/%d must be a power of two", CH);
  return MI355_OK;
}

extern "C" size_t mi355_conv_wgrad_workspace(const mi355_conv_desc* d) {
  WgradPlan w = plan_wgrad(d, conv_knobs());
  return (size_t)w.S * d->Co * w.ldw * sizeof(float);
}

extern "C" int mi355_conv_wgrad(const mi355_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                                void* ws, size_t ws_bytes, void* stream) {
  if (int e = check_desc(d, true)) return e;
  hipStream_t st = as_stream(stream);
  if (int e = check_wgrad_channels(d)) return e;
  const WgradPlan w = plan_wgrad(d, conv_knobs());
  const size_t need = (size_t)w.S * d->Co * w.ldw * sizeof(float);
  const bool direct = (w.S == 1 && !accumulate);
  if (!direct && (ws == nullptr || ws_bytes < need)) MI_FAIL(MI355_EWORKSPACE, "wgrad workspace %zu < %zu", ws_bytes, need);
  float* out = direct ? dw : reinterpret_cast<float*>(ws);
  const long M = (long)d->N * d->Ho * d->Wo, slab = (long)d->Co * w.ldw, esz = d->dtype == MI355_BF16 ? 2 : 4;
  const unsigned x_bytes = (unsigned)((long)d->N * d->Hi * d->Wi * d->Ci * esz), dy_bytes = (unsigned)(M * d->Co * esz);
  {
    if (prof_on()) prof_set_tag("%s k%ds%d %d>%d @%dx%d n%d S%d", wgrad_kernel_name(w), d->kh, d->stride, d->Ci, d->Co, d->Hi, d->Wi, d->N, w.S);
    ProfScope ps(st, 2.0 * M * (double)d->Co * w.ldw, (double)x_bytes + (double)dy_bytes + 4.0 * d->Co * w.ldw);
    if (w.kw2) {
      WgradKw2Args k; fill_wgrad_args(k, d, w, x, dy, out, w.rows_per_split);
      dim3 grid(w.nto * d->kh * w.nti * w.S);
      if (d->kh == 3) { if (w.mt == 1) hipLaunchKernelGGL((wgrad_kw2_kernel<1, 3>), grid, dim3(256), 0, st, k); else hipLaunchKernelGGL((wgrad_kw2_kernel<2, 3>), grid, dim3(256), 0, st, k); }
      else { if (w.mt == 1) hipLaunchKernelGGL((wgrad_kw2_kernel<1, 4>), grid, dim3(256), 0, st, k); else hipLaunchKernelGGL((wgrad_kw2_kernel<2, 4>), grid, dim3(256), 0, st, k); }
    } else if (w.kw3) {
      WgradKwArgs k; fill_wgrad_args(k, d, w, x, dy, out, w.rows_per_split);
      dim3 grid(w.nto * 3 * w.nti * w.S);
      if (w.mt == 1) hipLaunchKernelGGL(wgrad_kw_kernel<1>, grid, dim3(256), 0, st, k);
      else hipLaunchKernelGGL(wgrad_kw_kernel<2>, grid, dim3(256), 0, st, k);
    } else {
      WgradArgs a; fill_wgrad_args(a, d, w, x, dy, out, w.rows_per_split);
      dim3 grid(w.nto * w.nti * w.S);
      if (d->dtype == MI355_BF16) hipLaunchKernelGGL(wgrad_gemm_kernel<bf16_t>, grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(wgrad_gemm_kernel<float>, grid, dim3(256), 0, st, a);
    }
    MI_CHECK_LAUNCH(wgrad_kernel_name(w));
  }
  if (!direct) {
    launch_slab_reduce(reinterpret_cast<const float*>(ws), dw, slab, w.S, slab, accumulate, st);
    MI_CHECK_LAUNCH("slab_reduce");
  }
  return MI355_OK;
}


// ------------------------------------------------------------------------------------ grouped weight gradients
// items: HOST array.  Problems the specialised kernels take (3x3 stride 1 -> wgrad_kw, 3x3 / 4x4 stride 2 -> wgrad_kw2), and
// any problem that fills the chip on its own, run through mi355_conv_wgrad one by one; the rest -- the generic kernel's
// small problems -- are launched in groups of up to WG_MAX with a split count chosen for the GROUP.
// Which items share a launch (walk_wgrad_groups, whose launch kinds are the `kind` below) and the split counts and slab offsets of
// a group (group_plan) are in conv_plan.h.
// The slab reductions of a grouped launch, one launch for all of them.
static void slab_group_add(SlabGroupArgs& sg, int& nblocks, const float* slabs, float* out, long slab_stride, int S, int accumulate) {
  SlabItem& q = sg.it[sg.n];
  q.slabs = slabs; q.out = out; q.n4 = slab_stride / 4; q.stride = slab_stride; q.S = S; q.accumulate = accumulate;
  sg.bstart[sg.n] = nblocks; nblocks += cdiv(q.n4, 256); ++sg.n;
}
static int launch_slab_reduce_group(SlabGroupArgs& sg, int nblocks, hipStream_t st) {
  sg.bstart[sg.n] = nblocks;
  if (!sg.n) return MI355_OK;
  double sb = 0; for (int k = 0; k < sg.n; ++k) sb += 16.0 * sg.it[k].n4 * (sg.it[k].S + 1);
  char lab[64];
  if (prof_on()) snprintf(lab, sizeof(lab), "slab_reduce_group x%d", sg.n);
  ProfScope ps(st, 0.0, sb, 2, prof_on() ? lab : nullptr);
  hipLaunchKernelGGL(slab_reduce_group_kernel, dim3(nblocks), dim3(256), 0, st, sg); MI_CHECK_LAUNCH("slab_reduce_group");
  return MI355_OK;
}
extern "C" size_t mi355_conv_wgrad_grouped_workspace(const mi355_wgrad_item* items, int n) {
  if (!items || n < 1) return 0;
  size_t need = 0;
  (void)walk_wgrad_groups(items, n, [&](int kind, const int* idx, int m) -> int {
    size_t b = 0;
    if (kind == 0) b = mi355_conv_wgrad_workspace(&items[idx[0]].d);
    else { static_assert(WGK_MAX <= WG_MAX, "one plan array for every kind"); GroupPlan gp[WG_MAX]; group_plan(items, idx, m, gp, &b, kind); }
    if (b > need) need = b;
    return 0;
  });
  return need;
}
// the kernel of a grouped launch of `kind`, d0 its first item
static void launch_group_kernel(const WgradGroupArgs& g, int nb, int kind, const mi355_conv_desc* d0, hipStream_t st) {
  if (kind == 3) {
    static bool attr_set = false;
    if (!attr_set) { (void)hipFuncSetAttribute((const void*)wgrad_group256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WG256_SMEM); attr_set = true; }
    hipLaunchKernelGGL(wgrad_group256_kernel, dim3(nb), dim3(512), WG256_SMEM, st, g);
  }
  else if (d0->dtype == MI355_BF16) hipLaunchKernelGGL(wgrad_group_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(wgrad_group_kernel<float>, dim3(nb), dim3(256), 0, st, g);
}
static void launch_group_kernel(const WgradKwGroupArgs& g, int nb, int, const mi355_conv_desc* d0, hipStream_t st) {
  if (plan_wgrad(d0, conv_knobs()).mt == 1) hipLaunchKernelGGL(wgrad_kw_group_kernel<1>, dim3(nb), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(wgrad_kw_group_kernel<2>, dim3(nb), dim3(256), 0, st, g);
}
// One grouped launch (Group = WgradKwGroupArgs for kind 2, WgradGroupArgs for kinds 1 and 3) and the slab reductions of its items.
template <typename Group>
static int launch_wgrad_group(const mi355_wgrad_item* items, const int* idx, int n, void* ws, size_t ws_bytes, hipStream_t st, int kind) {
  const char* name = kind == 3 ? "wgrad_group256" : kind == 2 ? "wgrad_kw_group" : "wgrad_group";
  GroupPlan gp[WG_MAX]; size_t need = 0;
  group_plan(items, idx, n, gp, &need, kind);
  if (need && (!ws || ws_bytes < need)) MI_FAIL(MI355_EWORKSPACE, "%s workspace %zu < %zu", name, ws_bytes, need);
  Group g; memset(&g, 0, sizeof(g));
  SlabGroupArgs sg; memset(&sg, 0, sizeof(sg));
  int nb = 0, nsb = 0;
  double flops = 0, bytes = 0;
  for (int k = 0; k < n; ++k) {
    const mi355_wgrad_item& it = items[idx[k]]; const mi355_conv_desc* d = &it.d;
    if (kind != 2) { if (int e = check_wgrad_channels(d)) return e; }
    WgradPlan w = plan_wgrad(d, conv_knobs());
    if (kind == 3) { w.nto = d->Co / 256; w.nti = w.ldw / 256; }
    const bool direct = gp[k].S == 1 && !it.accumulate;
    auto& a = g.p[k];
    fill_wgrad_args(a, d, w, it.x, it.dy, direct ? it.dw : reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + gp[k].ws_off), gp[k].rps);
    g.bstart[k] = nb; nb += (int)group_tiles(kind, d, w) * gp[k].S;
    flops += 2.0 * a.M * (double)d->Co * w.ldw; bytes += (double)a.x_bytes + a.dy_bytes + 4.0 * d->Co * w.ldw;
    if (!direct) slab_group_add(sg, nsb, a.out, it.dw, a.slab_stride, gp[k].S, it.accumulate);
  }
  g.bstart[n] = nb; g.n = n;
  {
    const mi355_conv_desc* d0 = &items[idx[0]].d;
    if (prof_on()) prof_set_tag("%s x%d blocks%d first k%ds%d %d>%d @%dx%d", name, n, nb, d0->kh, d0->stride, d0->Ci, d0->Co, d0->Hi, d0->Wi);
    ProfScope ps(st, flops, bytes);
    launch_group_kernel(g, nb, kind, d0, st);
    MI_CHECK_LAUNCH(name);
  }
  return launch_slab_reduce_group(sg, nsb, st);
}
extern "C" int mi355_conv_wgrad_grouped(const mi355_wgrad_item* items, int n, void* ws, size_t ws_bytes, void* stream) {
  if (!items || n < 1) MI_FAIL(MI355_EINVAL, "wgrad_grouped: no items");
  hipStream_t st = as_stream(stream);
  for (int i = 0; i < n; ++i) {
    if (int e = check_desc(&items[i].d)) return e;
    if (!items[i].x || !items[i].dy || !items[i].dw) MI_FAIL(MI355_EINVAL, "wgrad_grouped: item %d has a null operand", i);
  }
  return walk_wgrad_groups(items, n, [&](int kind, const int* idx, int m) -> int {
    if (kind == 0) { const mi355_wgrad_item& it = items[idx[0]]; return mi355_conv_wgrad(&it.d, it.x, it.dy, it.dw, it.accumulate, ws, ws_bytes, stream); }
    if (kind == 2) return launch_wgrad_group<WgradKwGroupArgs>(items, idx, m, ws, ws_bytes, st, kind);
    return launch_wgrad_group<WgradGroupArgs>(items, idx, m, ws, ws_bytes, st, kind);
  });
}

// ------------------------------------------------------------------------------------ weight packing
template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wt, int O, int Tt, int I, int Ipad) {
  // tile 32(o) x 32(i) per tap through LDS so both the read ([O][T][I]) and the transposed write ([Ipad][T][O]) coalesce;
  // channels I..Ipad-1 of the packed copies are zero (stem: 3 -> 8)
  __shared__ float tile[32][33];
  const int tap = blockIdx.z, o0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    int o = o0 + r, i = i0 + tx;
    float v = (o < O && i < I) ? w[((size_t)o * Tt + tap) * I + i] : 0.f;
    tile[r][tx] = v;
    if (wf && o < O && i < Ipad) Elem<T>::st(wf + ((size_t)o * Tt + tap) * Ipad + i, v);
  }
  __syncthreads();
  if (wt)
    for (int r = ty; r < 32; r += 8) {
      int i = i0 + r, o = o0 + tx;
      if (o < O && i < Ipad) Elem<T>::st(wt + ((size_t)i * Tt + tap) * O + o, tile[tx][r]);
    }
}

// All conv weights of one optimizer group in ONE launch (after the optimizer step): items live in device memory,
// block b finds its item by binary search over the items' first-block prefix.
template <typename T>
__global__ void pack_weights_batched_kernel(const mi355_pack_item* __restrict__ items, int nitems) {
  __shared__ float tile[32][33];
  int lo = 0, hi = nitems - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  const mi355_pack_item it = items[lo];
  const int O = it.O, Tt = it.T, I = it.I, Ipad = it.Ipad;
  const int nbi = (Ipad + 31) / 32, nbo = (O + 31) / 32;
  int q = b - it.blk0;
  const int bi = q % nbi; q /= nbi;
  const int bo = q % nbo; const int tap = q / nbo;
  const float* __restrict__ w = it.w;
  T* __restrict__ wf = reinterpret_cast<T*>(it.wf);
  T* __restrict__ wt = reinterpret_cast<T*>(it.wt);
  const int o0 = bo * 32, i0 = bi * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    int o = o0 + r, i = i0 + tx;
    float v = (o < O && i < I) ? w[((size_t)o * Tt + tap) * I + i] : 0.f;
    tile[r][tx] = v;
    if (wf && o < O && i < Ipad) Elem<T>::st(wf + ((size_t)o * Tt + tap) * Ipad + i, v);
  }
  __syncthreads();
  if (wt)
    for (int r = ty; r < 32; r += 8) {
      int i = i0 + r, o = o0 + tx;
      if (o < O && i < Ipad) Elem<T>::st(wt + ((size_t)i * Tt + tap) * O + o, tile[tx][r]);
    }
}
extern "C" int mi355_pack_weights_batched(const mi355_pack_item* items_dev, int nitems, int total_blocks, int dtype, void* stream) {
  if (!items_dev || nitems < 1 || total_blocks < 1) MI_FAIL(MI355_EINVAL, "pack_weights_batched: bad args");
  if (dtype == MI355_BF16) hipLaunchKernelGGL(pack_weights_batched_kernel<bf16_t>, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, nitems);
  else if (dtype == MI355_F32) hipLaunchKernelGGL(pack_weights_batched_kernel<float>, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, nitems);
  else MI_FAIL(MI355_EINVAL, "bad dtype");
  MI_CHECK_LAUNCH("pack_weights_batched");
  return MI355_OK;
}

extern "C" int mi355_pack_weights(const float* w, void* wf, void* wt, int O, int Tt, int I, int Ipad, int dtype, void* stream) {
  if (!w || O < 1 || Tt < 1 || I < 1 || Ipad < I) MI_FAIL(MI355_EINVAL, "pack_weights: bad args");
  dim3 grid(cdiv(Ipad, 32), cdiv(O, 32), Tt);
  if (dtype == MI355_BF16) hipLaunchKernelGGL(pack_weights_kernel<bf16_t>, grid, dim3(256), 0, as_stream(stream), w, (bf16_t*)wf, (bf16_t*)wt, O, Tt, I, Ipad);
  else if (dtype == MI355_F32) hipLaunchKernelGGL(pack_weights_kernel<float>, grid, dim3(256), 0, as_stream(stream), w, (float*)wf, (float*)wt, O, Tt, I, Ipad);
  else MI_FAIL(MI355_EINVAL, "bad dtype");
  MI_CHECK_LAUNCH("pack_weights");
  return MI355_OK;
}

// Host-side exerciser of mi355_roi_crop_normalize and mi355_track_update for the CPU-box sanitizer job (tests/test_host_track.py):
// built like render_driver.cpp -- the HOST pass of every .hip file with -fsanitize=address,undefined, linked with this program.  No
// GPU is needed or used: device pointers are fake, well-aligned addresses that the host never dereferences (norm is a real host
// array: the entry point reads it), and every launch fails in the HIP runtime AFTER the host code under test has run.  The job
// passes when no sanitizer report aborts the process and every invalid call is refused with MI355_EINVAL, naming the argument.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../../include/mi355pose.h"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d  %s  (last error: %s)\n", __FILE__, __LINE__, #cond, mi355_last_error()); ++g_fail; } } while (0)
static char* fp(size_t i, size_t off = 0) { return reinterpret_cast<char*>(static_cast<uintptr_t>(0x100000000ull + (i << 44))) + off; }
static bool ran(int rc) { return rc == MI355_ELAUNCH || rc == MI355_OK; }
static bool says(const char* what) { return std::strstr(mi355_last_error(), what) != nullptr; }

static const float g_norm[6] = {0.485f, 0.456f, 0.406f, 0.229f, 0.224f, 0.225f};

struct Crop { char *frames, *recs, *out; int F, Hf, Wf, N, S; const float* norm; };
static Crop crop(int N = 3, int S = 32, int Hf = 40, int Wf = 56, int F = 2) { return Crop{fp(1), fp(2), fp(3), F, Hf, Wf, N, S, g_norm}; }
static int run(const Crop& a) {
  return mi355_roi_crop_normalize((const unsigned char*)a.frames, a.F, a.Hf, a.Wf, (const mi355_track_rec*)a.recs, a.N, a.S, a.norm,
                                  (float*)a.out, nullptr);
}

struct Upd { char *rec_in, *xy, *conf, *kp, *vis, *score, *rec_out; mi355_track_params P; int N, K; };
static Upd upd(int N = 3, int K = 21, int S = 32, int Hf = 40, int Wf = 56) {
  mi355_track_params P = {0.02f, 8, 1.5f, 1.0f, 1.25f, 5, 16.0f, Wf, Hf, S};
  return Upd{fp(1), fp(2), fp(3), fp(4), fp(5), fp(6), fp(7), P, N, K};
}
static int run(const Upd& a) {
  return mi355_track_update((const mi355_track_rec*)a.rec_in, (const float*)a.xy, (const float*)a.conf, a.P, (float*)a.kp, (float*)a.vis,
                            (float*)a.score, (mi355_track_rec*)a.rec_out, a.N, a.K, nullptr);
}

int main() {
  static_assert(sizeof(mi355_track_rec) == 32 && sizeof(mi355_track_params) == 40, "eight and ten words");
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

  // ================================================================ roi_crop_normalize
  // ---- the shapes of tests/test_gpu_track.py, the flagship crop and the extremes, out 16-byte aligned and off by 4 bytes
  for (int S : {16, 32, 64})
    for (int N : {1, 3, 5})
      for (size_t off : {(size_t)0, (size_t)4}) {
        { Crop a = crop(N, S, 40, 56); a.out += off; EXPECT(ran(run(a))); }
        { Crop a = crop(N, S, 33, 57); a.out += off; EXPECT(ran(run(a))); }
      }
  for (int S = 16; S <= MI355_TRACK_MAX_SIDE; S += 16) EXPECT(ran(run(crop(2, S))));
  EXPECT(ran(run(crop(64, 256, 480, 640, 1))));
  EXPECT(ran(run(crop(1, 16, 1, 1, 1))));
  EXPECT(ran(run(crop(1, MI355_TRACK_MAX_SIDE, MI355_TRACK_MAX_FRAME, MI355_TRACK_MAX_FRAME, 4))));
  EXPECT(ran(run(crop(0x7fffffff, 16))));                                                                              // the largest grid
  EXPECT(ran(run(crop(0x7fffffff / 256, MI355_TRACK_MAX_SIDE))));
  { Crop a = crop(); a.frames += 1; EXPECT(ran(run(a))); }                                                             // frames: any alignment
  const long nout = 12L * 3 * 32 * 32, nrec = 32L * 3, nfr = 3L * 40 * 56 * 2;
  { Crop a = crop(); a.recs = a.out + nout; a.frames = a.recs + nrec; EXPECT(ran(run(a))); }                            // touching is not overlapping
  { Crop a = crop(); a.out = a.frames + nfr; EXPECT(ran(run(a))); }
  // ---- refused arguments: each fails with MI355_EINVAL before any launch
  { Crop a = crop(); a.frames = nullptr; EXPECT(run(a) == MI355_EINVAL && says("frames is null")); }
  { Crop a = crop(); a.recs = nullptr; EXPECT(run(a) == MI355_EINVAL && says("recs is null")); }
  { Crop a = crop(); a.norm = nullptr; EXPECT(run(a) == MI355_EINVAL && says("norm is null")); }
  { Crop a = crop(); a.out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("out is null")); }
  for (int F : {0, -1}) { char w[32]; std::snprintf(w, sizeof(w), "F=%d", F); Crop a = crop(); a.F = F; EXPECT(run(a) == MI355_EINVAL && says(w)); }
  for (int v : {0, -3, MI355_TRACK_MAX_FRAME + 1, 0x7fffffff}) {
    char w[32];
    std::snprintf(w, sizeof(w), "Hf=%d", v);
    { Crop a = crop(); a.Hf = v; EXPECT(run(a) == MI355_EINVAL && says(w)); }
    std::snprintf(w, sizeof(w), "Wf=%d", v);
    { Crop a = crop(); a.Wf = v; EXPECT(run(a) == MI355_EINVAL && says(w)); }
  }
  for (int N : {0, -2}) { char w[32]; std::snprintf(w, sizeof(w), "N=%d", N); EXPECT(run(crop(N)) == MI355_EINVAL && says(w)); }
  for (int S : {0, -16, 8, 15, 17, 24, 100, 520, 528, 1024, 0x7fffffff}) {
    char w[32];
    std::snprintf(w, sizeof(w), "S=%d", S);
    EXPECT(run(crop(3, S)) == MI355_EINVAL && says(w));
  }
  for (int c = 0; c < 3; ++c) {
    float nm[6];
    for (float bad : {nan, inf, -inf}) {
      std::memcpy(nm, g_norm, sizeof(nm)); nm[c] = bad;
      { Crop a = crop(); a.norm = nm; EXPECT(run(a) == MI355_EINVAL && says("norm mean")); }
    }
    for (float bad : {nan, inf, 0.0f, -1.0f}) {
      std::memcpy(nm, g_norm, sizeof(nm)); nm[3 + c] = bad;
      { Crop a = crop(); a.norm = nm; EXPECT(run(a) == MI355_EINVAL && says("norm std")); }
    }
  }
  for (size_t off : {(size_t)1, (size_t)2, (size_t)3}) {
    { Crop a = crop(); a.recs += off; EXPECT(run(a) == MI355_EINVAL && says("recs must be 4-byte aligned")); }
    { Crop a = crop(); a.out += off; EXPECT(run(a) == MI355_EINVAL && says("out must be 4-byte aligned")); }
  }
  { Crop a = crop(); a.F = 0x7fffffff; a.Hf = a.Wf = MI355_TRACK_MAX_FRAME; EXPECT(run(a) == MI355_EINVAL && says("too large (F=")); }
  EXPECT(run(crop(0x7fffffff / 256 + 1, MI355_TRACK_MAX_SIDE)) == MI355_EINVAL && says("too large (N="));
  EXPECT(run(crop(0x7fffffff, 48)) == MI355_EINVAL && says("too large (N="));
  { Crop a = crop(); a.out = a.frames; EXPECT(run(a) == MI355_EINVAL && says("out and frames overlap")); }
  { Crop a = crop(); a.out = a.frames + nfr - 4; EXPECT(run(a) == MI355_EINVAL && says("out and frames overlap")); }
  { Crop a = crop(); a.frames = a.out + nout - 1; EXPECT(run(a) == MI355_EINVAL && says("out and frames overlap")); }
  { Crop a = crop(); a.recs = a.out + 64; EXPECT(run(a) == MI355_EINVAL && says("out and recs overlap")); }
  { Crop a = crop(); a.out = a.recs + nrec - 4; EXPECT(run(a) == MI355_EINVAL && says("out and recs overlap")); }

  // ================================================================ track_update
  for (int N : {1, 3, 5, 64, 65, 4096})
    for (int K : {1, 21, MI355_TRACK_MAX_JOINTS}) {
      Upd a = upd(N, K); a.P.min_joints = K < 8 ? K : 8;
      EXPECT(ran(run(a)));
      a.rec_out = a.rec_in; EXPECT(ran(run(a)));                                                                       // in place
    }
  EXPECT(ran(run(upd(0x7fffffff, MI355_TRACK_MAX_JOINTS))));
  { Upd a = upd(); a.P.alpha = 0.0f; a.P.grow = 1.0f; a.P.max_lost = 0; a.P.min_side = 1.0f; a.P.min_joints = 21; a.P.tau = -3.0e38f; EXPECT(ran(run(a))); }
  { Upd a = upd(); a.P.max_lost = 1 << 30; a.P.Wf = a.P.Hf = MI355_TRACK_MAX_FRAME; a.P.S = MI355_TRACK_MAX_SIDE; EXPECT(ran(run(a))); }
  const long nk = 3L * 21;
  { Upd a = upd(); a.xy = a.rec_in + nrec; a.conf = a.xy + 8 * nk; a.kp = a.conf + 4 * nk; a.vis = a.kp + 8 * nk; a.score = a.vis + 4 * nk;
    a.rec_out = a.score + 12; EXPECT(ran(run(a))); }                                                                   // touching is not overlapping
  // ---- refused arguments
  { Upd a = upd(); a.rec_in = nullptr; EXPECT(run(a) == MI355_EINVAL && says("rec_in is null")); }
  { Upd a = upd(); a.xy = nullptr; EXPECT(run(a) == MI355_EINVAL && says("xy is null")); }
  { Upd a = upd(); a.conf = nullptr; EXPECT(run(a) == MI355_EINVAL && says("conf is null")); }
  { Upd a = upd(); a.kp = nullptr; EXPECT(run(a) == MI355_EINVAL && says("kp is null")); }
  { Upd a = upd(); a.vis = nullptr; EXPECT(run(a) == MI355_EINVAL && says("vis is null")); }
  { Upd a = upd(); a.score = nullptr; EXPECT(run(a) == MI355_EINVAL && says("score is null")); }
  { Upd a = upd(); a.rec_out = nullptr; EXPECT(run(a) == MI355_EINVAL && says("rec_out is null")); }
  for (int N : {0, -1}) { char w[32]; std::snprintf(w, sizeof(w), "N=%d", N); EXPECT(run(upd(N)) == MI355_EINVAL && says(w)); }
  for (int K : {0, -1, MI355_TRACK_MAX_JOINTS + 1, 0x7fffffff}) { char w[32]; std::snprintf(w, sizeof(w), "K=%d", K); EXPECT(run(upd(3, K)) == MI355_EINVAL && says(w)); }
  for (float bad : {nan, inf, -inf}) { Upd a = upd(); a.P.tau = bad; EXPECT(run(a) == MI355_EINVAL && says("tau=")); }
  for (int bad : {0, -1, 22, 0x7fffffff}) { Upd a = upd(); a.P.min_joints = bad; EXPECT(run(a) == MI355_EINVAL && says("min_joints=")); }
  for (float bad : {nan, inf, 0.0f, -1.5f}) { Upd a = upd(); a.P.scale = bad; EXPECT(run(a) == MI355_EINVAL && says("scale=")); }
  for (float bad : {nan, inf, -0.25f, 1.5f}) { Upd a = upd(); a.P.alpha = bad; EXPECT(run(a) == MI355_EINVAL && says("alpha=")); }
  for (float bad : {nan, inf, 0.5f, -2.0f}) { Upd a = upd(); a.P.grow = bad; EXPECT(run(a) == MI355_EINVAL && says("grow=")); }
  for (int bad : {-1, (1 << 30) + 1, 0x7fffffff}) { Upd a = upd(); a.P.max_lost = bad; EXPECT(run(a) == MI355_EINVAL && says("max_lost=")); }
  for (float bad : {nan, inf, 0.5f, -4.0f}) { Upd a = upd(); a.P.min_side = bad; EXPECT(run(a) == MI355_EINVAL && says("min_side=")); }
  for (int bad : {0, -1, MI355_TRACK_MAX_FRAME + 1}) {
    { Upd a = upd(); a.P.Wf = bad; EXPECT(run(a) == MI355_EINVAL && says("Wf=")); }
    { Upd a = upd(); a.P.Hf = bad; EXPECT(run(a) == MI355_EINVAL && says("Hf=")); }
  }
  for (int bad : {0, 8, 24, 520, -16}) { Upd a = upd(); a.P.S = bad; EXPECT(run(a) == MI355_EINVAL && says("S=")); }
  for (size_t off : {(size_t)1, (size_t)2, (size_t)3}) {
    { Upd a = upd(); a.rec_in += off; EXPECT(run(a) == MI355_EINVAL && says("rec_in must be 4-byte aligned")); }
    { Upd a = upd(); a.xy += off; EXPECT(run(a) == MI355_EINVAL && says("xy must be 4-byte aligned")); }
    { Upd a = upd(); a.conf += off; EXPECT(run(a) == MI355_EINVAL && says("conf must be 4-byte aligned")); }
    { Upd a = upd(); a.kp += off; EXPECT(run(a) == MI355_EINVAL && says("kp must be 4-byte aligned")); }
    { Upd a = upd(); a.vis += off; EXPECT(run(a) == MI355_EINVAL && says("vis must be 4-byte aligned")); }
    { Upd a = upd(); a.score += off; EXPECT(run(a) == MI355_EINVAL && says("score must be 4-byte aligned")); }
    { Upd a = upd(); a.rec_out += off; EXPECT(run(a) == MI355_EINVAL && says("rec_out must be 4-byte aligned")); }
  }
  { Upd a = upd(); a.rec_out = a.rec_in + 32; EXPECT(run(a) == MI355_EINVAL && says("rec_out and rec_in overlap")); }     // shifted by one record
  { Upd a = upd(); a.kp = a.xy; EXPECT(run(a) == MI355_EINVAL && says("kp and xy overlap")); }
  { Upd a = upd(); a.vis = a.conf + 4 * nk - 4; EXPECT(run(a) == MI355_EINVAL && says("vis and conf overlap")); }
  { Upd a = upd(); a.score = a.rec_in + 4; EXPECT(run(a) == MI355_EINVAL && says("score and rec_in overlap")); }
  { Upd a = upd(); a.vis = a.kp + 8; EXPECT(run(a) == MI355_EINVAL && says("kp and vis overlap")); }
  { Upd a = upd(); a.score = a.vis; EXPECT(run(a) == MI355_EINVAL && says("vis and score overlap")); }
  { Upd a = upd(); a.rec_out = a.score; EXPECT(run(a) == MI355_EINVAL && says("score and rec_out overlap")); }
  { Upd a = upd(); a.rec_out = a.rec_in; a.kp = a.rec_in + 8; EXPECT(run(a) == MI355_EINVAL && says("kp and rec_in overlap")); }
  std::printf("track driver: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}

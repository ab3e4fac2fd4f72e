// The kernel build the library would choose for a convolution, without a GPU: csrc/conv_plan.h (describe, choose, plan) driven
// the way conv_fwd_impl / conv_dgrad_impl / mi355_conv_wgrad drive it.  Knobs come from the environment as in the library.
//
// stdin, one case per line:   op dtype N H W Ci Co k stride pad Ho Wo [flag=value ...]
//   op     fwd | dgrad | wgrad | cat | fp8 | mx | pgemm (= fwd under mi355_set_pgemm(2) unless pgemm= says otherwise);
//          fp8, mx and pgemm take ":dgrad" for the input gradient (fp8:dgrad gathers e5m2, as the training step does)
//   dtype  bf16 | f32 (fp8 / mx: ignored, the operands are bytes and the results bf16)
//          wplan = the split of a weight gradient in full; gitem = one item of a grouped weight-gradient call (held back
//          until a line "gplan" asks for the launches mi355_conv_wgrad_grouped would make of the items so far)
//   flags  stats=1 res=1 acc=1 (2: masked accumulate) bnb=1 c2=<channels of the second operand> pgemm=<mode> kw3min=<tiles>
//          slices=1 (with stats=1 / bnb=1: append the slices the launch writes and the slices its buffer holds)
//          dw=<n> (gitem: items with the same n write the same gradient)
// stdout:  "<line number>\t<text>" per launch, the text being what the launch log shows in brackets; input gradients under
//          MI355_PHASES=0 give one line per phase, weight gradients "<kernel> S<splits>".
//          wplan: "<kernel> S<splits> rows<rows per split> M<reduction rows> ws<workspace bytes>"
//          gplan: one line per launch, "kind<0 single | 1 generic | 2 3x3 | 3 256-tile> ws<bytes>" and per item
//                 " | item<index> S<splits> rows<rows per split> M<rows> slab<1: slab-reduced, 0: written directly>"
#include <cstdio>
#include <cstring>
#include <string>
#include <sstream>
#include <iostream>
#include <vector>
#include "../domain-adaptative-hand-pose-estimation_amd/csrc/conv_plan.h"
#include "../include/mi355pose.h"

static float g_dummy[4];      // stands for every operand the chooser only tests for presence

static float g_dw[64];        // stands for the gradients of grouped items: items with the same index share one

static void print_launch(int line, GatherArgs a, bool fp8, bool slices = false) {
  const ConvKnobs& k = conv_knobs();
  ConvBuild b = fp8 ? choose_fp8(a, k) : choose_conv(a, a.cshift, k);     // (cshift holds the element size here)
  char text[64];
  if (b.family == CONV_PGEMM) { if (!pgemm_plan_grid(a, b)) { printf("%d\tpgemm: the weight slice does not fit\n", line); return; } }
  else plan_gather_launch(a, b, k);
  conv_build_text(b, text, sizeof(text));
  if (slices) printf("%d\t%s slices=%d/%zu\n", line, text, a.stat_slices, a.stat_bytes / ((size_t)a.Nout * (b.epi == 2 ? 2 : 3) * sizeof(float)));
  else printf("%d\t%s\n", line, text);
}

// the launches of one grouped weight-gradient call, as mi355_conv_wgrad_grouped walks them
static void print_group_plan(int line, const std::vector<mi355_wgrad_item>& items) {
  (void)walk_wgrad_groups(items.data(), (int)items.size(), [&](int kind, const int* idx, int m) -> int {
    GroupPlan gp[WG_MAX]; size_t ws = 0;
    if (kind == 0) {
      const mi355_wgrad_item& it = items[idx[0]];
      const WgradPlan w = plan_wgrad(&it.d, conv_knobs());
      gp[0].S = w.S; gp[0].rps = w.rows_per_split; ws = (size_t)w.S * it.d.Co * w.ldw * sizeof(float);
    } else group_plan(items.data(), idx, m, gp, &ws, kind);
    printf("%d\tkind%d ws%zu", line, kind, ws);
    for (int k = 0; k < m; ++k) {
      const mi355_wgrad_item& it = items[idx[k]];
      printf(" | item%d S%d rows%d M%ld slab%d", idx[k], gp[k].S, gp[k].rps, (long)it.d.N * it.d.Ho * it.d.Wo, (gp[k].S > 1 || it.accumulate) ? 1 : 0);
    }
    printf("\n");
    return 0;
  });
}

int main() {
  std::string row;
  std::vector<mi355_wgrad_item> group;
  for (int line = 1; std::getline(std::cin, row); ++line) {
    if (row.compare(0, 5, "gplan") == 0) { if (!group.empty()) print_group_plan(line, group); group.clear(); continue; }
    std::istringstream in(row);
    std::string op, dt, flag;
    mi355_conv_desc d; memset(&d, 0, sizeof(d));
    if (!(in >> op >> dt >> d.N >> d.Hi >> d.Wi >> d.Ci >> d.Co >> d.kh >> d.stride >> d.pad >> d.Ho >> d.Wo)) {
      if (row.find_first_not_of(" \t\r") == std::string::npos) continue;
      fprintf(stderr, "line %d: cannot parse '%s'\n", line, row.c_str()); return 2;
    }
    d.kw = d.kh;
    int stats = 0, res = 0, acc = 0, bnb = 0, c2 = 0, pgemm = -1, slices = 0, dw = -1; long kw3min = -1;
    while (in >> flag) {
      const size_t eq = flag.find('=');
      const std::string key = flag.substr(0, eq); const long v = eq == std::string::npos ? 1 : atol(flag.c_str() + eq + 1);
      if (key == "stats") stats = (int)v; else if (key == "res") res = (int)v; else if (key == "acc") acc = (int)v;
      else if (key == "bnb") bnb = (int)v; else if (key == "c2") c2 = (int)v; else if (key == "pgemm") pgemm = (int)v;
      else if (key == "kw3min") kw3min = v; else if (key == "slices") slices = (int)v; else if (key == "dw") dw = (int)v;
      else { fprintf(stderr, "line %d: unknown flag '%s'\n", line, flag.c_str()); return 2; }
    }
    const bool dgrad = op == "dgrad" || op.find(":dgrad") != std::string::npos;
    const std::string kind = op.substr(0, op.find(':'));
    const bool fp8 = kind == "fp8" || kind == "mx";
    if (kind == "pgemm" && pgemm < 0) pgemm = 2;
    d.dtype = fp8 ? MI355_FP8 : dt == "f32" ? MI355_F32 : MI355_BF16;
    conv_knobs().pgemm_set = pgemm < 0 ? -1 : pgemm;        // what mi355_set_pgemm / mi355_set_fp8_kw3 do
    conv_knobs().fp8_kw3_set = kw3min < 0 ? -1 : kw3min;

    if (kind == "wgrad" || kind == "wplan") {
      const WgradPlan w = plan_wgrad(&d, conv_knobs());
      if (kind == "wgrad") printf("%d\t%s S%d\n", line, wgrad_kernel_name(w), w.S);
      else printf("%d\t%s S%d rows%d M%ld ws%zu\n", line, wgrad_kernel_name(w), w.S, w.rows_per_split, (long)d.N * d.Ho * d.Wo, (size_t)w.S * d.Co * w.ldw * sizeof(float));
      continue;
    }
    if (kind == "gitem") {
      if (dw < 0 || dw >= 64 || group.size() >= 64) { fprintf(stderr, "line %d: gitem needs dw=0..63\n", line); return 2; }
      mi355_wgrad_item it; memset(&it, 0, sizeof(it));
      it.d = d; it.x = g_dummy; it.dy = g_dummy; it.dw = &g_dw[dw]; it.accumulate = acc ? 1 : 0;
      group.push_back(it);
      continue;
    }
    GatherArgs a; memset(&a, 0, sizeof(a));
    a.cshift = fp8 ? 1 : d.dtype == MI355_F32 ? 4 : 2;
    a.A = a.B = a.D = g_dummy;
    if (kind == "mx") { a.mx_sa = g_dummy; a.mx_sb = g_dummy; }
    if (!dgrad) {
      describe_fwd(a, &d);
      if (res) a.residual = g_dummy;
      a.stat_bytes = conv_stats_bytes((long)d.N * d.Ho * d.Wo, d.Co);
      if (bnb) a.bnb_partial = g_dummy; else if (stats) a.stat_partial = g_dummy;
      if (kind == "cat") { a.A2 = a.B2 = g_dummy; a.c2 = c2; }
      print_launch(line, a, fp8, slices != 0);
      continue;
    }
    const bool need_zero = describe_dgrad(a, &d);
    a.accumulate = acc ? 1 : 0;
    if (acc == 2) a.acc_mask = reinterpret_cast<const unsigned char*>(g_dummy);
    if (kind == "fp8") a.a_fmt = 1;
    if (a.nphase == 0) continue;
    if (conv_knobs().phases || a.nphase == 1) {
      a.stat_bytes = conv_stats_bytes((long)d.N * d.Hi * d.Wi, d.Ci);
      if (bnb) a.bnb_partial = g_dummy;
      else if (stats && dgrad_fuses_stats(a, d.stride, need_zero)) a.stat_partial = g_dummy;
      print_launch(line, a, fp8, slices != 0);
      continue;
    }
    for (int i = 0; i < a.nphase; ++i) { GatherArgs p = a; p.nphase = 1; p.ph[0] = a.ph[i]; print_launch(line, p, fp8); }
  }
  return 0;
}

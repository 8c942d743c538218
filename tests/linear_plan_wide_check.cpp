// CPU walk of the wide plan (LinearEnv::wide_rows, plan_wide of zonos_amd/csrc/zn_linear_plan.h): see tests/test_linear_plan_wide.py.
#include "zn_linear_plan.h"

#include <cstring>
#include <string>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::string describe(const LinearPlan& p) {
  char b[240];
  if (p.err) { snprintf(b, sizeof b, "ERR %d", p.err); return b; }
  const char* ln = p.ln_launch ? " ln_launch" : "";
  const char* st = p.writes_ln_stats ? " writes_stats" : p.reads_ln_stats ? " reads_stats" : "";
  switch (p.kernel) {
    case LinearPlan::GEMV: snprintf(b, sizeof b, "GEMV per%d tiles%d", p.rows_per_launch, p.row_tiles); break;
    case LinearPlan::GEMM16: snprintf(b, sizeof b, "GEMM16 nw%d blocks%d per%d tiles%d%s", p.nw, p.blocks, p.rows_per_launch, p.row_tiles, ln); break;
    case LinearPlan::GEMM16S:
      snprintf(b, sizeof b, "GEMM16S nwv%d groups%d ksplit%d lnp%d w8%d per%d tiles%d wide_groups%d%s%s", p.nwv, p.groups, p.ksplit, (int)p.lnp, (int)p.w8, p.rows_per_launch, p.row_tiles,
               p.groups_wide, ln, st);
      break;
    case LinearPlan::GEMM16K: snprintf(b, sizeof b, "GEMM16K nch%d ln_pro%d epi%d per%d tiles%d%s%s", p.nch, (int)p.ln_pro, p.epi, p.rows_per_launch, p.row_tiles, ln, st); break;
    default: snprintf(b, sizeof b, "kernel %d per%d tiles%d", (int)p.kernel, p.rows_per_launch, p.row_tiles); break;
  }
  return b;
}

// every field but the three the wide plan may change
static bool same_but_rows(const LinearPlan& a, const LinearPlan& b) {
  return a.kernel == b.kernel && a.epi == b.epi && a.ln_launch == b.ln_launch && a.writes_ln_stats == b.writes_ln_stats && a.reads_ln_stats == b.reads_ln_stats && a.ks == b.ks &&
         a.nch == b.nch && a.units == b.units && a.upw == b.upw && a.blocks == b.blocks && a.full == b.full && a.nw == b.nw && a.tile8 == b.tile8 && a.nwv == b.nwv &&
         a.groups == b.groups && a.ksplit == b.ksplit && a.lnp == b.lnp && a.ln_pro == b.ln_pro && a.w8 == b.w8 && a.err == b.err && !strcmp(a.msg, b.msg);
}
static bool same(const LinearPlan& a, const LinearPlan& b) {
  return same_but_rows(a, b) && a.rows_per_launch == b.rows_per_launch && a.row_tiles == b.row_tiles && a.groups_wide == b.groups_wide;
}

static long long g_plans = 0, g_wide16s = 0, g_wide16k = 0, g_fallback = 0, g_fallback_1mib = 0, g_stay = 0, g_w8wide = 0, g_lnpwide = 0;

// the wide plan pw of a decode call of `rows` > 16 rows against the 16-row plan p16 of the same call
static void check_wide(const LinearEnv& e, const LinearPlan& pw, const LinearPlan& p16, int pro, int epi, int rows, int N, int K, bool one_mib) {
  ++g_plans;
  CHECK(same_but_rows(pw, p16), "rows %d pro %d epi %d N %d K %d: %s vs the 16-row plan %s", rows, pro, epi, N, K, describe(pw).c_str(), describe(p16).c_str());
  if (pw.err) { CHECK(pw.row_tiles == 1, "error plan with row tiles"); return; }
  CHECK(linear_plan_launchable(pw, pro, pw.epi), "pro %d epi %d rows %d N %d K %d: %s", pro, epi, rows, N, K, describe(pw).c_str());
  const int tiles = ((rows < 64 ? rows : 64) + 15) / 16;
  const bool k_wide = p16.kernel == LinearPlan::GEMM16K && epi != EPI_MAMBA;
  const bool s_form = p16.kernel == LinearPlan::GEMM16S && ((epi == EPI_RESID && pro == PRO_NONE) || (epi == EPI_SILU && (pro == PRO_NONE || pro == PRO_LN)));
  if (k_wide) {
    ++g_wide16k;
    CHECK(pw.row_tiles == tiles && pw.rows_per_launch == 64 && pw.groups_wide == 0, "%s at %d rows", describe(pw).c_str(), rows);
  } else if (s_form) {
    const int wrows = epi == EPI_SILU ? N / 2 : N, per = epi == EPI_SILU ? 32 : 64, groups = (wrows + per - 1) / per;
    const bool fits = (size_t)p16.ksplit * 16 * tiles * groups * 64 * sizeof(float) <= e.g16_part_bytes;
    if (fits) {
      ++g_wide16s; g_w8wide += pw.w8; g_lnpwide += pw.lnp;
      CHECK(pw.row_tiles == tiles && pw.rows_per_launch == 64, "%s at %d rows", describe(pw).c_str(), rows);
      CHECK(pw.groups_wide == groups && (long long)pw.groups_wide * per >= wrows && (long long)(pw.groups_wide - 1) * per < wrows, "%s: grid does not cover %d rows", describe(pw).c_str(), wrows);
      CHECK(pw.groups_wide <= ZN_G16_MAX_GROUPS && K % (pw.ksplit * ZN_G16_KC) == 0, "%s", describe(pw).c_str());
    } else {
      ++g_fallback; g_fallback_1mib += one_mib;
      CHECK(same(pw, p16), "partial tiles do not fit: %s must be the 16-row plan %s", describe(pw).c_str(), describe(p16).c_str());
    }
  } else {
    ++g_stay;      // direct fragments, the Mamba2 projections, STORE, F32 and LayerNorm x residual on the LDS-staged kernel
    CHECK(same(pw, p16) && pw.row_tiles == 1 && pw.rows_per_launch == 16, "%s stays per 16 (%s)", describe(pw).c_str(), describe(p16).c_str());
  }
  CHECK(pro != PRO_LN || (pw.ln_launch + pw.ln_pro + pw.reads_ln_stats == 1), "LayerNorm applied once: %s", describe(pw).c_str());
}

struct Pinned { const char* what; int rows; const char* plan; };

int main(int argc, char** argv) {
  const bool print = argc > 1 && !strcmp(argv[1], "--print");
  const int rows_all[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 64};
  const int rows_wide[] = {17, 24, 32, 33, 48, 64};
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {2048, 8192}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws)
        for (int w8 = 0; w8 < 2; ++w8) {
          LinearEnv e;
          e.small_m_lds = (tune & 1) ? 1 : 2; e.no_split_small_m = (tune & 2) ? 2 : 0; e.fc1_ln_launch = (tune & 4) ? 2 : 0; e.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
          e.gemm16k_max_tiles = mt; e.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; e.has_g16_part = true; e.has_ln_part = ws != 1;
          e.w8_offered = w8 != 0;
          LinearEnv ew = e;
          ew.wide_rows = true;
          for (const auto& nk : shapes) {
            // 1. rows <= 16, and prefill at any row count: the wide setting changes nothing
            for (int rows : rows_all)
              for (int prefill = 0; prefill < 2; ++prefill) {
                if (!prefill && rows > 16) continue;
                for (int pro = 0; pro < ZN_NPRO; ++pro)
                  for (int epi = 0; epi < ZN_NEPI; ++epi)
                    for (int target : {256, 1024})
                      for (int hand = 0; hand < 4; ++hand) {
                        const LinearPlan a = plan_linear(e, pro, epi, rows, nk[0], nk[1], target, prefill != 0, (hand & 1) != 0, (hand & 2) != 0);
                        const LinearPlan b = plan_linear(ew, pro, epi, rows, nk[0], nk[1], target, prefill != 0, (hand & 1) != 0, (hand & 2) != 0);
                        CHECK(same(a, b) && b.row_tiles == 1, "rows %d prefill %d pro %d epi %d: %s vs %s", rows, prefill, pro, epi, describe(b).c_str(), describe(a).c_str());
                      }
              }
            // 2. decode, more than 16 rows
            for (int rows : rows_wide) {
              for (int pro = 0; pro < ZN_NPRO; ++pro)
                for (int epi = 0; epi < ZN_NEPI; ++epi)
                  for (int target : {256, 1024})
                    for (int hand = 0; hand < 4; ++hand) {
                      // the 16-row plan of the same call: what the wide setting off returns (an error plan's message names the row count)
                      const LinearPlan p16 = plan_linear(e, pro, epi, rows, nk[0], nk[1], target, false, (hand & 1) != 0, (hand & 2) != 0);
                      const LinearPlan at16 = plan_linear(e, pro, epi, 16, nk[0], nk[1], target, false, (hand & 1) != 0, (hand & 2) != 0);
                      CHECK(p16.err == at16.err && (p16.err || same(p16, at16)), "wide off at %d rows: %s is not the plan at 16 rows %s", rows, describe(p16).c_str(), describe(at16).c_str());
                      CHECK(p16.err || (p16.rows_per_launch == 16 && p16.row_tiles == 1), "wide off: %s", describe(p16).c_str());
                      check_wide(ew, plan_linear(ew, pro, epi, rows, nk[0], nk[1], target, false, (hand & 1) != 0, (hand & 2) != 0), p16, pro, epi, rows, nk[0], nk[1], ws == 2);
                    }
              // the pair of plan_post_attention: fc1 reads statistics only if out_proj writes them, wide as grouped
              const LinearPlan out = plan_linear(ew, PRO_NONE, EPI_RESID, rows, nk[0], nk[1], 512, false, true, false);
              for (int F2 : {16384, 4096, 512}) {
                const LinearPlan fc1 = plan_linear(ew, PRO_LN, EPI_SILU, rows, F2, nk[0], 512, false, false, out.writes_ln_stats);
                CHECK(!fc1.reads_ln_stats || out.writes_ln_stats, "fc1 reads statistics out_proj does not write: %s / %s", describe(out).c_str(), describe(fc1).c_str());
                CHECK(!plan_linear(ew, PRO_LN, EPI_SILU, rows, F2, nk[0], 512, false, false, false).reads_ln_stats, "fc1 reads statistics nobody offered");
                CHECK(fc1.err || (fc1.reads_ln_stats + fc1.ln_launch == 1), "fc1's LayerNorm: %s", describe(fc1).c_str());
              }
            }
          }
        }
  // 3. the plans at the production shapes (Zonos-v0.1), default tune values and workspace, the wide setting on; fc1 / fc2 also with the FP8 stream offered
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true; e.wide_rows = true;
  static const Pinned pinned[] = {
    {"in_proj", 32, "GEMM16K nch2 ln_pro1 epi3 per64 tiles2"},
    {"out_proj", 32, "GEMM16K nch2 ln_pro0 epi1 per64 tiles2 writes_stats"},
    {"fc1", 32, "GEMM16S nwv2 groups512 ksplit1 lnp1 w80 per64 tiles2 wide_groups256 reads_stats"},
    {"fc2", 32, "GEMM16S nwv2 groups64 ksplit8 lnp0 w80 per64 tiles2 wide_groups32"},
    {"heads", 32, "GEMM16K nch2 ln_pro0 epi4 per64 tiles2 ln_launch"},
    {"fc1.fp8", 32, "GEMM16S nwv2 groups512 ksplit1 lnp1 w81 per64 tiles2 wide_groups256 reads_stats"},
    {"fc2.fp8", 32, "GEMM16S nwv2 groups64 ksplit8 lnp0 w81 per64 tiles2 wide_groups32"},
    {"in_proj", 64, "GEMM16K nch2 ln_pro1 epi3 per64 tiles4"},
    {"out_proj", 64, "GEMM16K nch2 ln_pro0 epi1 per64 tiles4 writes_stats"},
    {"fc1", 64, "GEMM16S nwv2 groups512 ksplit1 lnp1 w80 per64 tiles4 wide_groups256 reads_stats"},
    {"fc2", 64, "GEMM16S nwv2 groups64 ksplit8 lnp0 w80 per64 tiles4 wide_groups32"},
    {"heads", 64, "GEMM16K nch2 ln_pro0 epi4 per64 tiles4 ln_launch"},
    {"fc1.fp8", 64, "GEMM16S nwv2 groups512 ksplit1 lnp1 w81 per64 tiles4 wide_groups256 reads_stats"},
    {"fc2.fp8", 64, "GEMM16S nwv2 groups64 ksplit8 lnp0 w81 per64 tiles4 wide_groups32"},
  };
  size_t np = 0;
  for (int rows : {32, 64}) {
    LinearEnv e8 = e;
    e8.w8_offered = true;
    const LinearPlan in = plan_linear(e, PRO_LN, EPI_ROPE_KV, rows, 3072, 2048, 256, false, false, false);
    const LinearPlan out = plan_linear(e, PRO_NONE, EPI_RESID, rows, 2048, 2048, 512, false, true, false);
    const LinearPlan fc1 = plan_linear(e, PRO_LN, EPI_SILU, rows, 16384, 2048, 512, false, false, out.writes_ln_stats);
    const LinearPlan fc2 = plan_linear(e, PRO_NONE, EPI_RESID, rows, 2048, 8192, 1024, false, false, false);
    const LinearPlan heads = plan_linear(e, PRO_LN, EPI_F32, rows, 9225, 2048, 512, false, false, false);
    const LinearPlan fc1q = plan_linear(e8, PRO_LN, EPI_SILU, rows, 16384, 2048, 512, false, false, out.writes_ln_stats);
    const LinearPlan fc2q = plan_linear(e8, PRO_NONE, EPI_RESID, rows, 2048, 8192, 1024, false, false, false);
    const LinearPlan* ps[] = {&in, &out, &fc1, &fc2, &heads, &fc1q, &fc2q};
    const char* names[] = {"in_proj", "out_proj", "fc1", "fc2", "heads", "fc1.fp8", "fc2.fp8"};
    for (int k = 0; k < 7; ++k, ++np) {
      if (print) { printf("    {\"%s\", %d, \"%s\"},\n", names[k], rows, describe(*ps[k]).c_str()); continue; }
      CHECK(np < sizeof pinned / sizeof pinned[0] && !strcmp(pinned[np].what, names[k]) && pinned[np].rows == rows && describe(*ps[k]) == pinned[np].plan,
            "%s at %d rows: %s", names[k], rows, describe(*ps[k]).c_str());
    }
  }
  if (print) return 0;
  CHECK(np == sizeof pinned / sizeof pinned[0], "pinned table: %zu entries walked", np);
  printf("wide plans %lld: GEMM16S wide %lld (FP8 %lld, statistics %lld), GEMM16K wide %lld, back to 16 rows for the partial tiles %lld (1 MiB workspace %lld), per 16 %lld\n", g_plans,
         g_wide16s, g_w8wide, g_lnpwide, g_wide16k, g_fallback, g_fallback_1mib, g_stay);
  CHECK(g_wide16s > 0 && g_w8wide > 0 && g_lnpwide > 0 && g_wide16k > 0 && g_stay > 0, "a branch of the wide plan was never walked");
  CHECK(g_fallback_1mib > 0, "the 1 MiB workspace never showed the fallback");
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

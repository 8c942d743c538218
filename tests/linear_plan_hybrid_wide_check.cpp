// CPU walk of the Mamba2 in_proj's wide forms (LinearEnv::wide_hybrid, plan_wide of zonos_amd/csrc/zn_linear_plan.h): see tests/test_linear_plan_hybrid_wide.py.
#include "zn_linear_plan.h"

#include <cstring>
#include <string>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::string describe(const LinearPlan& p) {
  char b[240];
  if (p.err) { snprintf(b, sizeof b, "ERR %d", p.err); return b; }
  static const char* names[] = {"GEMV", "GEMM16", "GEMM16S", "GEMM16K", "GEMM64S", "GEMM_TILED"};
  snprintf(b, sizeof b, "%s nch%d ln_pro%d epi%d nwv%d groups%d ksplit%d per%d tiles%d wide_groups%d loop%d", names[p.kernel], p.nch, (int)p.ln_pro, p.epi, p.nwv, p.groups, p.ksplit,
           p.rows_per_launch, p.row_tiles, p.groups_wide, (int)p.row_loop);
  return b;
}

// every field but the three the Mamba2 in_proj's wide forms may change
static bool same_but_rows(const LinearPlan& a, const LinearPlan& b) {
  return a.kernel == b.kernel && a.epi == b.epi && a.groups_wide == b.groups_wide && a.ln_launch == b.ln_launch && a.writes_ln_stats == b.writes_ln_stats &&
         a.reads_ln_stats == b.reads_ln_stats && a.ks == b.ks && a.nch == b.nch && a.units == b.units && a.upw == b.upw && a.blocks == b.blocks && a.full == b.full && a.nw == b.nw &&
         a.tile8 == b.tile8 && a.nwv == b.nwv && a.groups == b.groups && a.ksplit == b.ksplit && a.lnp == b.lnp && a.ln_pro == b.ln_pro && a.w8 == b.w8 && a.err == b.err &&
         !strcmp(a.msg, b.msg);
}
static bool same(const LinearPlan& a, const LinearPlan& b) { return same_but_rows(a, b) && a.rows_per_launch == b.rows_per_launch && a.row_tiles == b.row_tiles && a.row_loop == b.row_loop; }

static long long g_plans = 0, g_grid = 0, g_loop = 0, g_loop_as_grid = 0, g_same = 0;

struct Pinned { const char* what; int form, rows; const char* plan; };

int main(int argc, char** argv) {
  const bool print = argc > 1 && !strcmp(argv[1], "--print");
  const int rows_all[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 32, 33, 48, 64, 80};
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {8384, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {8512, 4096}, {2048, 8192}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws)
        for (int w8 = 0; w8 < 2; ++w8)
          for (int wide = 0; wide < 2; ++wide) {
            LinearEnv e;      // wide_hybrid left at its default: the env every other walk and every caller before the field builds
            e.small_m_lds = (tune & 1) ? 1 : 2; e.no_split_small_m = (tune & 2) ? 2 : 0; e.fc1_ln_launch = (tune & 4) ? 2 : 0; e.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
            e.gemm16k_max_tiles = mt; e.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; e.has_g16_part = true; e.has_ln_part = ws != 1;
            e.w8_offered = w8 != 0; e.wide_rows = wide != 0;
            CHECK(e.wide_hybrid == 0, "the default of LinearEnv::wide_hybrid is 0");
            for (const auto& nk : shapes)
              for (int rows : rows_all)
                for (int prefill = 0; prefill < 2; ++prefill)
                  for (int pro = 0; pro < ZN_NPRO; ++pro)
                    for (int epi = 0; epi < ZN_NEPI; ++epi)
                      for (int hand = 0; hand < 4; hand += 3) {
                        const int target = rows <= 4 && (hand & 1) ? 1024 : 256;     // (the GEMV's grid: nothing above 4 rows reads it)
                        const LinearPlan a = plan_linear(e, pro, epi, rows, nk[0], nk[1], target, prefill != 0, (hand & 1) != 0, (hand & 2) != 0);
                        for (int form = wide ? 0 : 3; form <= (wide ? 4 : 3); ++form) {      // without wide_rows: one value of the field is enough to show it is not read
                            LinearEnv eh = e;
                            eh.wide_hybrid = form;
                            const LinearPlan b = plan_linear(eh, pro, epi, rows, nk[0], nk[1], target, prefill != 0, (hand & 1) != 0, (hand & 2) != 0);
                            ++g_plans;
                            CHECK(!a.row_loop, "no loop form without the field: %s", describe(a).c_str());
                            const bool may = wide && !prefill && rows > 16 && !a.err && a.kernel == LinearPlan::GEMM16K && epi == EPI_MAMBA && form >= 2;
                            if (!may) {
                              ++g_same;
                              CHECK(same(a, b), "form %d wide %d rows %d prefill %d pro %d epi %d N %d K %d: %s vs %s", form, wide, rows, prefill, pro, epi, nk[0], nk[1], describe(b).c_str(),
                                    describe(a).c_str());
                              continue;
                            }
                            // the Mamba2 in_proj on gemm16k_kernel, decode, more than 16 rows, a wide form asked for
                            const int tiles = ((rows < 64 ? rows : 64) + 15) / 16;
                            CHECK(a.rows_per_launch == 16 && a.row_tiles == 1, "without the field the Mamba2 in_proj stays per 16: %s", describe(a).c_str());
                            CHECK(same_but_rows(a, b), "form %d rows %d pro %d N %d K %d: %s vs %s", form, rows, pro, nk[0], nk[1], describe(b).c_str(), describe(a).c_str());
                            CHECK(b.rows_per_launch == 64 && b.row_tiles == tiles, "form %d rows %d: %s", form, rows, describe(b).c_str());
                            CHECK(linear_plan_launchable(b, pro, b.epi), "form %d rows %d pro %d N %d K %d: %s", form, rows, pro, nk[0], nk[1], describe(b).c_str());
                            const bool loop_exists = pro == PRO_NONE && b.nch == 2 && !b.ln_pro;     // the one instantiation: what production launches
                            const int picked = form == 4 ? wide_hybrid_form(rows < 64 ? rows : 64) : form;
                            CHECK(picked == 2 || picked == 3, "the default form at %d rows is a wide one here: %d", rows, picked);
                            CHECK(b.row_loop == (picked == 3 && loop_exists), "form %d rows %d pro %d N %d K %d: %s", form, rows, pro, nk[0], nk[1], describe(b).c_str());
                            if (b.row_loop) ++g_loop; else if (picked == 3) ++g_loop_as_grid; else ++g_grid;
                        }
                      }
          }
  // the plans at the production shapes (Zonos-v0.1-hybrid: d_state 128 -> N = 8512; d_state 64, two groups -> N = 8384), default tune values and workspace
  static const Pinned pinned[] = {
    {"mamba_in_proj.8512", 0, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 0, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 0, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 0, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 1, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 1, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 1, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 1, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 2, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 2, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 2, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 2, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop0"},
    {"mamba_in_proj.8512", 3, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop1"},
    {"mamba_in_proj.8512", 3, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop1"},
    {"mamba_in_proj.8512", 3, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop1"},
    {"mamba_in_proj.8512", 3, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop1"},
    {"mamba_in_proj.8384", 0, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 0, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 0, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 0, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 1, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 1, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 1, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 1, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per16 tiles1 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 2, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 2, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 2, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 2, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop0"},
    {"mamba_in_proj.8384", 3, 17, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop1"},
    {"mamba_in_proj.8384", 3, 32, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles2 wide_groups0 loop1"},
    {"mamba_in_proj.8384", 3, 64, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop1"},
    {"mamba_in_proj.8384", 3, 80, "GEMM16K nch2 ln_pro0 epi5 nwv0 groups0 ksplit0 per64 tiles4 wide_groups0 loop1"},
  };
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true; e.wide_rows = true;
  size_t np = 0;
  for (int N : {8512, 8384})
    for (int form = 0; form <= 3; ++form)
      for (int rows : {17, 32, 64, 80}) {
        LinearEnv eh = e;
        eh.wide_hybrid = form;
        const LinearPlan p = plan_linear(eh, PRO_NONE, EPI_MAMBA, rows, N, 2048, (N / 2 + 3) / 4, false, false, false);
        const std::string what = "mamba_in_proj." + std::to_string(N);
        if (print) { printf("    {\"%s\", %d, %d, \"%s\"},\n", what.c_str(), form, rows, describe(p).c_str()); ++np; continue; }
        CHECK(np < sizeof pinned / sizeof pinned[0] && what == pinned[np].what && pinned[np].form == form && pinned[np].rows == rows && describe(p) == pinned[np].plan,
              "%s form %d at %d rows: %s", what.c_str(), form, rows, describe(p).c_str());
        ++np;
      }
  if (print) return 0;
  CHECK(np == sizeof pinned / sizeof pinned[0], "pinned table: %zu entries walked", np);
  // the Mamba2 out_proj (2048 x 4096, no prologue from 5 rows on, store): wide with and without the field
  for (int form = 0; form <= 4; ++form)
    for (int rows : {17, 32, 64, 80}) {
      LinearEnv eh = e;
      eh.wide_hybrid = form;
      const LinearPlan p = plan_linear(eh, PRO_NONE, EPI_STORE, rows, 2048, 4096, 1024, false, false, false);
      CHECK(describe(p) == std::string("GEMM16K nch4 ln_pro0 epi0 nwv0 groups0 ksplit0 per64 tiles") + std::to_string(rows >= 64 ? 4 : (rows + 15) / 16) + " wide_groups0 loop0",
            "Mamba2 out_proj form %d at %d rows: %s", form, rows, describe(p).c_str());
    }
  printf("plans %lld: equal to the plan without the field %lld, row groups on grid y %lld, the row-tile loop %lld, loop asked for where only the grid form exists %lld\n", g_plans, g_same, g_grid,
         g_loop, g_loop_as_grid);
  CHECK(g_same > 0 && g_grid > 0 && g_loop > 0 && g_loop_as_grid > 0, "a branch was never walked");
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

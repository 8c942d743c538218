// CPU walk of plan_linear's FP8 offer for the Mamba2 projections (zonos_amd/csrc/zn_linear_plan.h: LinearEnv::w8k_offered -> LinearPlan::w8 of a GEMM16K
// plan): see tests/test_linear_plan_mamba_fp8.py.
#include "zn_linear_plan.h"

#include <cstring>
#include <initializer_list>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// every field of a plan but w8
static bool same_but_w8(const LinearPlan& a, const LinearPlan& b) {
  return a.kernel == b.kernel && a.epi == b.epi && a.rows_per_launch == b.rows_per_launch && a.row_tiles == b.row_tiles && a.groups_wide == b.groups_wide && a.row_loop == b.row_loop &&
         a.ln_launch == b.ln_launch && a.writes_ln_stats == b.writes_ln_stats && a.reads_ln_stats == b.reads_ln_stats && a.ks == b.ks && a.nch == b.nch && a.units == b.units &&
         a.upw == b.upw && a.blocks == b.blocks && a.full == b.full && a.nw == b.nw && a.tile8 == b.tile8 && a.nwv == b.nwv && a.groups == b.groups && a.ksplit == b.ksplit &&
         a.lnp == b.lnp && a.ln_pro == b.ln_pro && a.err == b.err && !memcmp(a.msg, b.msg, sizeof a.msg);
}

int main() {
  // the production (N, K) pairs of both stacks: attention in_proj / out_proj, fc1, fc2, the heads; the Mamba2 in_proj (d_state 128; d_state 64 with two groups) and
  // out_proj; and shapes off the kernels' grids
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {8384, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {8512, 4096}, {2048, 8192}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  long long plans = 0, n_in = 0, n_out = 0, n_in_loop = 0, n_in_grid = 0, n_out_grid = 0, n_small = 0;
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws)
        for (int w8 = 0; w8 < 2; ++w8)
          for (int wide = 0; wide < 2; ++wide) {
              LinearEnv off;
              off.small_m_lds = (tune & 1) ? 1 : 2; off.no_split_small_m = (tune & 2) ? 2 : 0; off.fc1_ln_launch = (tune & 4) ? 2 : 0; off.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
              off.gemm16k_max_tiles = mt; off.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; off.has_g16_part = true; off.has_ln_part = ws != 1;
              off.w8_offered = w8 != 0; off.wide_rows = wide != 0;
              CHECK(!off.w8k_offered, "the default of LinearEnv::w8k_offered is false");
              for (const auto& nk : shapes)
                for (int rows = 1; rows <= 80; ++rows)
                  for (int prefill = 0; prefill < 2; ++prefill)
                    for (int pro = 0; pro < ZN_NPRO; ++pro)
                      for (int epi = 0; epi < ZN_NEPI; ++epi)
                      // wide_hybrid 0 .. 4 where it is read (the Mamba2 epilogue under wide_rows); elsewhere one value is enough
                      for (int form = wide && epi == EPI_MAMBA ? 0 : 4; form <= 4; ++form) {
                        off.wide_hybrid = form;
                        LinearEnv on = off;
                        on.w8k_offered = true;
                        const bool pf = prefill != 0;
                        const int target = rows <= 4 ? 1024 : 256;
                        const LinearPlan a = plan_linear(off, pro, epi, rows, nk[0], nk[1], target, pf, false, false);
                        const LinearPlan b = plan_linear(on, pro, epi, rows, nk[0], nk[1], target, pf, false, false);
                        ++plans;
                        // the offer changes no other field: kernel, row_tiles, row_loop, grid
                        CHECK(same_but_w8(a, b), "the offer changes a plan: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                        // w8_offered alone leaves every GEMM16K plan unmarked
                        CHECK(!(a.w8 && a.kernel == LinearPlan::GEMM16K), "w8_offered marks a GEMM16K plan: pro %d epi %d rows %d N %d K %d", pro, epi, rows, nk[0], nk[1]);
                        // where the offer is not read, w8 is what w8_offered made it
                        const bool inst = pro == PRO_NONE && !b.ln_pro && ((b.epi == EPI_MAMBA && b.nch == 2) || (b.epi == EPI_STORE && b.nch == 4));     // the FP8 instantiations
                        const bool mine = !pf && !b.err && b.kernel == LinearPlan::GEMM16K && inst;
                        CHECK(b.w8 == (mine || a.w8), "w8 %d, expected %d: pro %d epi %d rows %d N %d K %d prefill %d kernel %d nch %d", (int)b.w8, (int)(mine || a.w8), pro, epi, rows, nk[0],
                              nk[1], prefill, (int)b.kernel, b.nch);
                        if (b.w8 && b.kernel == LinearPlan::GEMM16K) {
                          CHECK(!pf && rows > 4 && pro == PRO_NONE && (epi == EPI_MAMBA || epi == EPI_STORE), "w8 outside its plans: pro %d epi %d rows %d prefill %d", pro, epi, rows, prefill);
                          CHECK(nk[1] == (epi == EPI_MAMBA ? 2048 : 4096), "w8 outside its widths: epi %d K %d", epi, nk[1]);
                          (epi == EPI_MAMBA ? n_in : n_out)++;
                          if (b.row_tiles > 1) (epi == EPI_STORE ? n_out_grid : b.row_loop ? n_in_loop : n_in_grid)++;
                          else ++n_small;
                        }
                        if (pf || rows <= 4 || epi == EPI_ROPE_KV || epi == EPI_RESID || epi == EPI_F32)
                          CHECK(!(b.w8 && !a.w8), "the offer is read where it must not be: pro %d epi %d rows %d prefill %d", pro, epi, rows, prefill);
                        if (!b.err) CHECK(linear_plan_launchable(b, pro, b.epi), "not launchable under the offer: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                        // a w8 flag on a GEMM16K plan without an FP8 instantiation is never launchable
                        if (!b.err && b.kernel == LinearPlan::GEMM16K && !inst) {
                          LinearPlan forced = b;
                          forced.w8 = true;
                          CHECK(!linear_plan_launchable(forced, pro, b.epi), "forced w8 launchable: pro %d epi %d nch %d ln_pro %d", pro, b.epi, b.nch, (int)b.ln_pro);
                        }
                      }
            }
  // the production plans, default settings, as a generation step makes them (wide from 17 rows on, the form the plan picks)
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true; e.wide_rows = true; e.wide_hybrid = 4; e.w8k_offered = true;
  for (int rows = 1; rows <= 80; ++rows) {
    const bool big = rows > 4;
    for (int N : {8512, 8384}) CHECK(plan_linear(e, PRO_NONE, EPI_MAMBA, rows, N, 2048, (N / 2 + 3) / 4, false, false, false).w8 == big, "Mamba2 in_proj %d at %d rows", N, rows);
    CHECK(plan_linear(e, big ? PRO_NONE : PRO_GATED, EPI_STORE, rows, 2048, 4096, 1024, false, false, false).w8 == big, "Mamba2 out_proj at %d rows", rows);
    CHECK(!plan_linear(e, PRO_NONE, EPI_STORE, rows, 2048, 2048, 512, false, false, false).w8, "attention out_proj (K = 2048) at %d rows", rows);
    CHECK(!plan_linear(e, PRO_NONE, EPI_ROPE_KV, rows, 3072, 2048, 256, false, false, false).w8, "attention in_proj at %d rows", rows);
    CHECK(!plan_linear(e, PRO_NONE, EPI_F32, rows, 9225, 2048, 512, false, false, false).w8, "heads at %d rows", rows);
    CHECK(!plan_linear(e, PRO_NONE, EPI_MAMBA, rows, 8512, 2048, 0, true, false, false).w8 && !plan_linear(e, PRO_NONE, EPI_STORE, rows, 2048, 4096, 0, true, false, false).w8,
          "prefill reads bf16 at %d rows", rows);
  }
  printf("plans %lld; reading FP8 under the offer: in_proj %lld, out_proj %lld (16 rows per pass %lld, in_proj row-tile loop %lld, in_proj grid y %lld, out_proj grid y %lld)\n", plans, n_in,
         n_out, n_small, n_in_loop, n_in_grid, n_out_grid);
  CHECK(n_in > 0 && n_out > 0 && n_small > 0 && n_in_loop > 0 && n_in_grid > 0 && n_out_grid > 0, "a form was never planned with FP8");
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

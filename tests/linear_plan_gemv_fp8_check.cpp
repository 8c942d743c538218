// CPU walk of plan_linear's FP8 offer for the GEMV of 1..4 decode rows (zonos_amd/csrc/zn_linear_plan.h: LinearEnv::w8v_offered -> LinearPlan::w8 of a GEMV
// plan): see tests/test_linear_plan_gemv_fp8.py.
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
// the table of the instantiations, written out a second time: (prologue, epilogue, K slices, chunks per slice) of fc1, fc2, the Mamba2 in_proj and out_proj
static bool table(int pro, int epi, int ks, int nch) {
  if (pro == PRO_LN && epi == EPI_SILU) return ks == 1 && nch == 4;
  if (pro == PRO_NONE && epi == EPI_RESID) return ks == 4 && nch == 4;
  if (pro == PRO_NONE && epi == EPI_MAMBA) return ks == 1 && nch == 4;
  if ((pro == PRO_GATED || pro == PRO_NONE) && epi == EPI_STORE) return ks == 4 && nch == 2;
  return false;
}

int main() {
  const int rows_v[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 24, 33, 64, 65, 80};
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {8384, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {2047, 4096}, {8512, 4096}, {2048, 8192}, {2047, 8192},
                           {2004, 2048}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  long long plans = 0, marked = 0, n_proj[5] = {};
  { LinearEnv d; CHECK(!d.w8v_offered && !d.w8_offered && !d.w8k_offered, "the default of LinearEnv::w8v_offered is false"); }
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws)
        for (int offers = 0; offers < 4; ++offers)
          for (int wide = 0; wide < 2; ++wide) {
            LinearEnv e;
            e.small_m_lds = (tune & 1) ? 1 : 2; e.no_split_small_m = (tune & 2) ? 2 : 0; e.fc1_ln_launch = (tune & 4) ? 2 : 0; e.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
            e.gemm16k_max_tiles = mt; e.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; e.has_g16_part = true; e.has_ln_part = ws != 1;
            e.wide_rows = wide != 0; e.wide_hybrid = 4;
            LinearEnv none = e;                                  // no offer at all: every GEMV plan of the two existing offers must equal this one's
            e.w8_offered = (offers & 1) != 0; e.w8k_offered = (offers & 2) != 0;
            LinearEnv off = e, on = e;
            off.w8v_offered = false; on.w8v_offered = true;
            for (int rows : rows_v)
              for (const auto& nk : shapes)
                for (int prefill = 0; prefill < 2; ++prefill)
                  for (int pro = 0; pro < ZN_NPRO; ++pro)
                    for (int epi = 0; epi < ZN_NEPI; ++epi)
                      for (int target : {64, 256, 1024}) {
                        const bool pf = prefill != 0;
                        const LinearPlan d = plan_linear(e, pro, epi, rows, nk[0], nk[1], target, pf, false, false);       // w8v_offered left at its default
                        const LinearPlan a = plan_linear(off, pro, epi, rows, nk[0], nk[1], target, pf, false, false);
                        const LinearPlan b = plan_linear(on, pro, epi, rows, nk[0], nk[1], target, pf, false, false);
                        const LinearPlan n = plan_linear(none, pro, epi, rows, nk[0], nk[1], target, pf, false, false);
                        ++plans;
                        // with the offer false every plan is today's, w8 included; the two existing offers leave every GEMV plan unmarked
                        CHECK(d.w8 == a.w8 && same_but_w8(d, a), "offer off changes a plan: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                        CHECK(!(a.w8 && a.kernel == LinearPlan::GEMV) && !n.w8 && same_but_w8(n, a), "an existing offer marks a GEMV plan or changes a field: pro %d epi %d rows %d N %d K %d", pro, epi, rows, nk[0], nk[1]);
                        // with it true every plan equals the un-offered one in every field but w8
                        CHECK(same_but_w8(a, b), "the offer changes a plan: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                        const bool inst = table(pro, b.epi, b.ks, b.nch);
                        CHECK(inst == lin_has_w8v(pro, b.epi, b.ks, b.nch), "lin_has_w8v is not the table: pro %d epi %d ks %d nch %d", pro, b.epi, b.ks, b.nch);
                        const bool mine = !pf && !b.err && rows <= 4 && b.kernel == LinearPlan::GEMV && inst;
                        CHECK(b.w8 == (mine || a.w8), "w8 %d, expected %d: pro %d epi %d rows %d N %d K %d prefill %d kernel %d ks %d nch %d", (int)b.w8, (int)(mine || a.w8), pro, epi, rows,
                              nk[0], nk[1], prefill, (int)b.kernel, b.ks, b.nch);
                        if (rows > 4 || pf || b.err) CHECK(b.w8 == a.w8, "the offer is read where it must not be: pro %d epi %d rows %d prefill %d err %d", pro, epi, rows, prefill, b.err);
                        if (!pf && !b.err && rows <= 4) CHECK(b.kernel == LinearPlan::GEMV, "a decode plan of %d rows that is no GEMV", rows);
                        if (b.w8 && b.kernel == LinearPlan::GEMV) {
                          ++marked;
                          n_proj[epi == EPI_SILU ? 0 : epi == EPI_RESID ? 1 : epi == EPI_MAMBA ? 2 : pro == PRO_GATED ? 3 : 4]++;
                          CHECK(b.rows_per_launch == 4 && nk[1] == (epi == EPI_RESID ? 8192 : epi == EPI_STORE ? 4096 : 2048), "w8 outside its widths: epi %d K %d", epi, nk[1]);
                        }
                        if (!b.err) CHECK(linear_plan_launchable(b, pro, b.epi), "not launchable under the offer: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                        // a w8 flag on a GEMV plan without an instantiation is never launchable
                        if (!b.err && b.kernel == LinearPlan::GEMV && !inst) {
                          LinearPlan forced = b;
                          forced.w8 = true;
                          CHECK(!linear_plan_launchable(forced, pro, b.epi), "forced w8 launchable: pro %d epi %d ks %d nch %d", pro, b.epi, b.ks, b.nch);
                        }
                      }
          }
  // the production plans at default settings as a generation step makes them: the stream at 1, 2, 3, 4 rows under the offer and not without it; 5 rows: no GEMV, unchanged
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true; e.wide_rows = true; e.wide_hybrid = 4;
  LinearEnv v = e;
  v.w8v_offered = true;
  struct Prod { const char* name; int pro, epi, N, K, target, ks, nch; };
  const Prod prod[] = {{"fc1", PRO_LN, EPI_SILU, 16384, 2048, 512, 1, 4},          {"fc2", PRO_NONE, EPI_RESID, 2048, 8192, 1024, 4, 4},
                       {"in_proj 8512", PRO_NONE, EPI_MAMBA, 8512, 2048, (8512 / 2 + 3) / 4, 1, 4}, {"in_proj 8384", PRO_NONE, EPI_MAMBA, 8384, 2048, (8384 / 2 + 3) / 4, 1, 4},
                       {"out_proj gated", PRO_GATED, EPI_STORE, 2048, 4096, 1024, 4, 2}, {"out_proj", PRO_NONE, EPI_STORE, 2048, 4096, 1024, 4, 2}};
  for (const Prod& q : prod)
    for (int rows = 1; rows <= 5; ++rows) {
      if (rows == 5 && q.pro == PRO_GATED) continue;                  // (the gated prologue serves at most 4 rows)
      const LinearPlan a = plan_linear(e, q.pro, q.epi, rows, q.N, q.K, q.target, false, false, false), b = plan_linear(v, q.pro, q.epi, rows, q.N, q.K, q.target, false, false, false);
      CHECK(!a.err && !a.w8 && same_but_w8(a, b), "%s at %d rows: the offer changes the plan", q.name, rows);
      if (rows <= 4) {
        CHECK(b.w8 && b.kernel == LinearPlan::GEMV && b.ks == q.ks && b.nch == q.nch && b.full && b.rows_per_launch == 4, "%s at %d rows: kernel %d ks %d nch %d full %d w8 %d", q.name, rows,
              (int)b.kernel, b.ks, b.nch, (int)b.full, (int)b.w8);
        CHECK(linear_plan_launchable(b, q.pro, q.epi), "%s at %d rows not launchable", q.name, rows);
      } else CHECK(!b.w8 && b.kernel != LinearPlan::GEMV, "%s at 5 rows: kernel %d w8 %d", q.name, (int)b.kernel, (int)b.w8);
    }
  // what the step does not offer stays unmarked under the offer: attention in_proj / out_proj and the heads have no instantiation
  for (int rows = 1; rows <= 4; ++rows) {
    CHECK(!plan_linear(v, PRO_LN, EPI_ROPE_KV, rows, 3072, 2048, 256, false, false, false).w8, "attention in_proj at %d rows", rows);
    CHECK(!plan_linear(v, PRO_NONE, EPI_RESID, rows, 2048, 2048, 512, false, false, false).w8, "attention out_proj at %d rows", rows);
    CHECK(!plan_linear(v, PRO_LN, EPI_F32, rows, 9225, 2048, 512, false, false, false).w8, "heads at %d rows", rows);
    CHECK(!plan_linear(v, PRO_NONE, EPI_MAMBA, rows, 8512, 2048, 0, true, false, false).w8, "prefill reads bf16 at %d rows", rows);
  }
  printf("plans %lld; GEMV plans reading FP8 under the offer %lld (fc1 %lld, fc2 %lld, in_proj %lld, out_proj gated %lld, out_proj %lld)\n", plans, marked, n_proj[0], n_proj[1], n_proj[2],
         n_proj[3], n_proj[4]);
  for (int k = 0; k < 5; ++k) CHECK(n_proj[k] > 0, "projection %d never planned with FP8", k);
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

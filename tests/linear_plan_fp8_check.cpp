// CPU walk of plan_linear's FP8 offer (zonos_amd/csrc/zn_linear_plan.h: LinearEnv::w8_offered -> LinearPlan::w8) over the grid that
// tests/linear_plan_check.cpp walks: see tests/test_fp8_cpu.py.
#include "zn_linear_plan.h"

#include <cstring>
#include <initializer_list>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// every field of a plan but w8
static bool same_but_w8(LinearPlan a, LinearPlan b) {
  a.w8 = b.w8 = false;
  return a.kernel == b.kernel && a.epi == b.epi && a.rows_per_launch == b.rows_per_launch && a.ln_launch == b.ln_launch && a.writes_ln_stats == b.writes_ln_stats &&
         a.reads_ln_stats == b.reads_ln_stats && a.ks == b.ks && a.nch == b.nch && a.units == b.units && a.upw == b.upw && a.blocks == b.blocks && a.full == b.full &&
         a.nw == b.nw && a.tile8 == b.tile8 && a.nwv == b.nwv && a.groups == b.groups && a.ksplit == b.ksplit && a.lnp == b.lnp && a.ln_pro == b.ln_pro && a.err == b.err &&
         !memcmp(a.msg, b.msg, sizeof a.msg);
}

int main() {
  const int rows_v[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 64};
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {2048, 8192}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  long long plans = 0, w8_plans = 0, w8_pair[3] = {};
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws) {
        LinearEnv e;
        e.small_m_lds = (tune & 1) ? 1 : 2; e.no_split_small_m = (tune & 2) ? 2 : 0; e.fc1_ln_launch = (tune & 4) ? 2 : 0; e.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
        e.gemm16k_max_tiles = mt; e.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; e.has_g16_part = true; e.has_ln_part = ws != 1;
        LinearEnv off = e, on = e;
        off.w8_offered = false; on.w8_offered = true;
        for (int rows : rows_v)
          for (const auto& nk : shapes)
            for (int prefill = 0; prefill < 2; ++prefill)
              for (int pro = 0; pro < ZN_NPRO; ++pro)
                for (int epi = 0; epi < ZN_NEPI; ++epi)
                  for (int target : {256, 1024})
                    for (int hand = 0; hand < 4; ++hand) {
                      const bool pf = prefill != 0, want = (hand & 1) != 0, have = (hand & 2) != 0;
                      const LinearPlan d = plan_linear(e, pro, epi, rows, nk[0], nk[1], target, pf, want, have);          // the default env: no offer
                      const LinearPlan a = plan_linear(off, pro, epi, rows, nk[0], nk[1], target, pf, want, have);
                      const LinearPlan b = plan_linear(on, pro, epi, rows, nk[0], nk[1], target, pf, want, have);
                      ++plans;
                      // with the offer off, every plan is the default-env plan, w8 included
                      CHECK(!d.w8 && !a.w8 && same_but_w8(d, a), "offer off changes a plan: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                      // offering never changes any other field
                      CHECK(same_but_w8(a, b), "the offer changes a plan: pro %d epi %d rows %d N %d K %d prefill %d", pro, epi, rows, nk[0], nk[1], prefill);
                      // w8 exactly for decode GEMM16S plans of the two MLP projections
                      const bool fc1 = epi == EPI_SILU && (pro == PRO_NONE || pro == PRO_LN), fc2 = epi == EPI_RESID && pro == PRO_NONE;
                      const bool expect = !pf && !b.err && b.kernel == LinearPlan::GEMM16S && (fc1 || fc2);
                      CHECK(b.w8 == expect, "w8 %d, expected %d: pro %d epi %d rows %d N %d K %d prefill %d kernel %d", (int)b.w8, (int)expect, pro, epi, rows, nk[0], nk[1], prefill, (int)b.kernel);
                      if (b.w8) {
                        ++w8_plans;
                        w8_pair[fc2 ? 2 : pro == PRO_LN ? 1 : 0]++;
                        CHECK(rows > 4 && nk[1] % ZN_G16_KC == 0 && lin_has_w8(pro, epi), "w8 outside its shapes: rows %d K %d", rows, nk[1]);
                        CHECK(linear_plan_launchable(b, pro, b.epi), "w8 plan not launchable: pro %d epi %d", pro, epi);
                      }
                      // a w8 flag on a pair without an FP8 instantiation is never launchable
                      if (!b.err && b.kernel == LinearPlan::GEMM16S && !lin_has_w8(pro, b.epi)) {
                        LinearPlan forced = b;
                        forced.w8 = true;
                        CHECK(!linear_plan_launchable(forced, pro, b.epi), "forced w8 launchable: pro %d epi %d", pro, b.epi);
                      }
                    }
      }
  // the production shapes, default settings: fc1 (with and without handed-over statistics) and fc2 at 6 and 16 rows read the stream, 2 and 4 rows do not
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true; e.w8_offered = true;
  for (int rows : {2, 4, 6, 16}) {
    const bool big = rows > 4;
    CHECK(plan_linear(e, PRO_LN, EPI_SILU, rows, 16384, 2048, 512, false, false, true).w8 == big, "fc1 (statistics) at %d rows", rows);
    CHECK(plan_linear(e, PRO_LN, EPI_SILU, rows, 16384, 2048, 512, false, false, false).w8 == big, "fc1 (LayerNorm launch) at %d rows", rows);
    CHECK(plan_linear(e, PRO_NONE, EPI_RESID, rows, 2048, 8192, 1024, false, false, false).w8 == big, "fc2 at %d rows", rows);
    CHECK(!plan_linear(e, PRO_NONE, EPI_RESID, rows, 2048, 2048, 512, false, true, false).w8, "out_proj (gemm16k) at %d rows", rows);
    CHECK(!plan_linear(e, PRO_LN, EPI_ROPE_KV, rows, 3072, 2048, 256, false, false, false).w8, "in_proj at %d rows", rows);
    CHECK(!plan_linear(e, PRO_LN, EPI_F32, rows, 9225, 2048, 512, false, false, false).w8, "heads at %d rows", rows);
  }
  CHECK(!plan_linear(e, PRO_NONE, EPI_SILU, 48, 16384, 2048, 0, true, false, false).w8 && !plan_linear(e, PRO_NONE, EPI_RESID, 48, 2048, 8192, 0, true, false, false).w8, "prefill reads bf16");
  printf("plans %lld, reading FP8 when offered %lld (none x SiLU %lld, LayerNorm x SiLU %lld, none x residual %lld)\n", plans, w8_plans, w8_pair[0], w8_pair[1], w8_pair[2]);
  for (int k = 0; k < 3; ++k) CHECK(w8_pair[k] > 0, "pair %d never planned with FP8", k);
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

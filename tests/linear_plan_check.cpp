// CPU walk of plan_linear (zonos_amd/csrc/zn_linear_plan.h, the header the launchers of zn_api.hip follow): see tests/test_linear_plan.py.
#include "zn_linear_plan.h"

#include <cstring>
#include <string>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::string describe(const LinearPlan& p) {
  char b[200];
  if (p.err) { snprintf(b, sizeof b, "ERR %d", p.err); return b; }
  const char* ln = p.ln_launch ? " ln_launch" : "";
  const char* st = p.writes_ln_stats ? " writes_stats" : p.reads_ln_stats ? " reads_stats" : "";
  switch (p.kernel) {
    case LinearPlan::GEMV: snprintf(b, sizeof b, "GEMV ks%d nch%d upw%d blocks%d full%d per%d", p.ks, p.nch, p.upw, p.blocks, (int)p.full, p.rows_per_launch); break;
    case LinearPlan::GEMM16: snprintf(b, sizeof b, "GEMM16 nw%d tile%d blocks%d per%d%s", p.nw, p.tile8 ? 8 : 16, p.blocks, p.rows_per_launch, ln); break;
    case LinearPlan::GEMM16S: snprintf(b, sizeof b, "GEMM16S nwv%d groups%d ksplit%d lnp%d per%d%s%s", p.nwv, p.groups, p.ksplit, (int)p.lnp, p.rows_per_launch, ln, st); break;
    case LinearPlan::GEMM16K: snprintf(b, sizeof b, "GEMM16K nch%d ln_pro%d epi%d per%d%s%s", p.nch, (int)p.ln_pro, p.epi, p.rows_per_launch, ln, st); break;
    case LinearPlan::GEMM64S: snprintf(b, sizeof b, "GEMM64S groups%d ksplit%d per%d", p.groups, p.ksplit, p.rows_per_launch); break;
    case LinearPlan::GEMM_TILED: snprintf(b, sizeof b, "GEMM_TILED epi%d per%d", p.epi, p.rows_per_launch); break;
  }
  return b;
}

static long long g_plans = 0, g_errs = 0, g_kind[6] = {};

static void check_plan(const LinearEnv& e, const LinearPlan& p, int pro, int epi, int rows, int N, int K, int target, bool prefill) {
  ++g_plans;
  if (p.err) { ++g_errs; CHECK(p.err < 0 && p.msg[0] != 0, "error plan without code or message"); return; }
  g_kind[(int)p.kernel]++;
  // 1. a kernel launch_linear<pro, epi> holds (the table of the header, which its `if constexpr` guards read too); prefill may turn EPI_ROPE_KV into EPI_STORE
  CHECK(p.epi == epi || (prefill && epi == EPI_ROPE_KV && p.epi == EPI_STORE), "epi %d -> %d", epi, p.epi);
  CHECK(linear_plan_launchable(p, pro, p.epi), "pro %d epi %d rows %d N %d K %d prefill %d: %s", pro, epi, rows, N, K, (int)prefill, describe(p).c_str());
  CHECK(prefill ? p.rows_per_launch == 0 : p.rows_per_launch == (rows <= 4 ? 4 : 16), "rows per launch %d at %d rows", p.rows_per_launch, rows);
  CHECK(prefill || (p.kernel == LinearPlan::GEMV) == (rows <= 4), "rows %d: %s", rows, describe(p).c_str());
  CHECK(!p.ln_launch || (pro == PRO_LN && !prefill && rows > 4 && !p.ln_pro && !p.reads_ln_stats), "LayerNorm launch: %s", describe(p).c_str());
  CHECK(pro != PRO_LN || prefill || rows <= 4 || (p.ln_launch + p.ln_pro + p.reads_ln_stats == 1), "LayerNorm applied once: %s", describe(p).c_str());
  // 2. the hand-off (the half a single plan shows)
  if (p.writes_ln_stats) CHECK(p.kernel == LinearPlan::GEMM16K && p.epi == EPI_RESID && N == 16 * ZN_G16_LNT && e.has_ln_part && e.fc1_ln_launch != 2, "writes: %s N %d", describe(p).c_str(), N);
  if (p.reads_ln_stats) CHECK(p.kernel == LinearPlan::GEMM16S && p.lnp && K == 16 * ZN_G16_LNT, "reads: %s K %d", describe(p).c_str(), K);
  CHECK(p.lnp == p.reads_ln_stats, "lnp %d reads %d", (int)p.lnp, (int)p.reads_ln_stats);
  // 3. split-K plans fit their scratch buffer and ticket array
  if (p.kernel == LinearPlan::GEMM16S || p.kernel == LinearPlan::GEMM64S) {
    const size_t tile = p.kernel == LinearPlan::GEMM64S ? (size_t)64 * 64 * 4 : (size_t)16 * p.nwv * 16 * 4;
    CHECK(p.ksplit >= 1 && (size_t)p.ksplit * tile * p.groups <= e.g16_part_bytes, "%s: partial tiles exceed %zu bytes", describe(p).c_str(), e.g16_part_bytes);
    CHECK(p.groups >= 1 && p.groups <= ZN_G16_MAX_GROUPS, "%s: groups", describe(p).c_str());
    CHECK(K % (p.ksplit * ZN_G16_KC) == 0, "%s: K %d", describe(p).c_str(), K);
    const int wrows = p.epi == EPI_SILU ? N / 2 : N, per = (p.epi == EPI_SILU ? 8 : 16) * p.nwv;      // weight rows per workgroup
    CHECK((long long)p.groups * per >= wrows && (long long)(p.groups - 1) * per < wrows, "%s: grid does not cover %d rows", describe(p).c_str(), wrows);
  } else CHECK(p.ksplit == 0, "%s: ksplit", describe(p).c_str());
  // 4. the GEMV's grid covers its units; the mask-free form only when everything divides
  if (p.kernel == LinearPlan::GEMV) {
    const int lanes_units = p.ks == 1 ? 4 : 1;
    CHECK(p.units == (epi == EPI_SILU ? N / 2 : (N + 1) / 2) && p.upw >= 1 && p.blocks >= 1, "%s", describe(p).c_str());
    CHECK((long long)p.blocks * lanes_units * p.upw >= p.units, "%s: units %d", describe(p).c_str(), p.units);
    CHECK(p.ks * p.nch * 512 >= K, "%s: K %d", describe(p).c_str(), K);
    CHECK(p.full == (p.ks * p.nch * 512 == K && N % 2 == 0 && (long long)p.blocks * lanes_units * p.upw == p.units), "%s: full", describe(p).c_str());
  }
  if (p.kernel == LinearPlan::GEMM16K) CHECK(K == ZN_G16K_NKW * ZN_G16K_KCH * p.nch && (!prefill || rows <= 64), "%s: K %d rows %d", describe(p).c_str(), K, rows);
  if (p.kernel == LinearPlan::GEMM16) CHECK(K % (p.nw * 32) == 0 && p.blocks == (p.tile8 ? N / 8 : (epi == EPI_SILU ? N / 2 / 16 : (N + 15) / 16)), "%s", describe(p).c_str());
  if (p.kernel == LinearPlan::GEMM_TILED) CHECK(prefill && K % 32 == 0, "%s: K %d (the tiled kernel walks whole 32-wide fragments)", describe(p).c_str(), K);
  (void)target;
}

struct Pinned { const char* what; int rows; const char* plan; };

int main(int argc, char** argv) {
  const bool print = argc > 1 && !strcmp(argv[1], "--print");
  const int rows_v[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 64};
  const int shapes[][2] = {{2048, 2048}, {3072, 2048}, {8512, 2048}, {9225, 2048}, {16384, 2048}, {2048, 4096}, {2048, 8192}, {1000, 512}, {72, 256}, {200, 136}};
  const int tiles_v[] = {0, 64, 200};
  for (int tune = 0; tune < 16; ++tune)
    for (int mt : tiles_v)
      for (int ws = 0; ws < 3; ++ws) {      // the handle's workspace: all of it (zn_create), no statistics buffer, a partial-tile buffer of 1 MiB
        LinearEnv e;
        e.small_m_lds = (tune & 1) ? 1 : 2; e.no_split_small_m = (tune & 2) ? 2 : 0; e.fc1_ln_launch = (tune & 4) ? 2 : 0; e.no_prefill_gemm16k = (tune & 8) ? 2 : 0;
        e.gemm16k_max_tiles = mt; e.g16_part_bytes = ws == 2 ? (size_t)1 << 20 : (size_t)8 << 20; e.has_g16_part = true; e.has_ln_part = ws != 1;
        for (int rows : rows_v)
          for (const auto& nk : shapes)
            for (int prefill = 0; prefill < 2; ++prefill) {
              for (int pro = 0; pro < ZN_NPRO; ++pro)
                for (int epi = 0; epi < ZN_NEPI; ++epi)
                  for (int target : {256, 1024})
                    for (int hand = 0; hand < 4; ++hand)
                      check_plan(e, plan_linear(e, pro, epi, rows, nk[0], nk[1], target, prefill != 0, (hand & 1) != 0, (hand & 2) != 0), pro, epi, rows, nk[0], nk[1], target, prefill != 0);
              // 2. the pair layer_post_attention and zn_bench_kernel make (plan_post_attention): out_proj [N][K], then fc1 over its N columns
              if (prefill) continue;
              const LinearPlan out = plan_linear(e, PRO_NONE, EPI_RESID, rows, nk[0], nk[1], 512, false, true, false);
              for (int F2 : {16384, 4096, 512}) {
                const LinearPlan fc1 = plan_linear(e, PRO_LN, EPI_SILU, rows, F2, nk[0], 512, false, false, out.writes_ln_stats);
                CHECK(!fc1.reads_ln_stats || out.writes_ln_stats, "fc1 reads statistics out_proj does not write: %s / %s", describe(out).c_str(), describe(fc1).c_str());
                CHECK(!plan_linear(e, PRO_LN, EPI_SILU, rows, F2, nk[0], 512, false, false, false).reads_ln_stats, "fc1 reads statistics nobody offered");
                CHECK(fc1.err || fc1.reads_ln_stats || rows <= 4 || fc1.ln_launch, "fc1 without LayerNorm: %s", describe(fc1).c_str());
              }
            }
      }
  // 5. the plans at the production shapes (Zonos-v0.1: d 2048, 16 / 4 heads of 128, d_ff 8192, 9 x 1025 logits), default tune values and workspace
  LinearEnv e;
  e.g16_part_bytes = (size_t)8 << 20; e.has_g16_part = e.has_ln_part = true;
  static const Pinned pinned[] = {
    {"in_proj", 2, "GEMV ks1 nch4 upw2 blocks192 full1 per4"},
    {"out_proj", 2, "GEMV ks1 nch4 upw1 blocks256 full1 per4"},
    {"fc1", 2, "GEMV ks1 nch4 upw4 blocks512 full1 per4"},
    {"fc2", 2, "GEMV ks4 nch4 upw1 blocks1024 full1 per4"},
    {"heads", 2, "GEMV ks1 nch4 upw3 blocks385 full0 per4"},
    {"in_proj", 4, "GEMV ks1 nch4 upw2 blocks192 full1 per4"},
    {"out_proj", 4, "GEMV ks1 nch4 upw1 blocks256 full1 per4"},
    {"fc1", 4, "GEMV ks1 nch4 upw4 blocks512 full1 per4"},
    {"fc2", 4, "GEMV ks4 nch4 upw1 blocks1024 full1 per4"},
    {"heads", 4, "GEMV ks1 nch4 upw3 blocks385 full0 per4"},
    {"in_proj", 6, "GEMM16K nch2 ln_pro1 epi3 per16"},
    {"out_proj", 6, "GEMM16K nch2 ln_pro0 epi1 per16 writes_stats"},
    {"fc1", 6, "GEMM16S nwv2 groups512 ksplit1 lnp1 per16 reads_stats"},
    {"fc2", 6, "GEMM16S nwv2 groups64 ksplit8 lnp0 per16"},
    {"heads", 6, "GEMM16K nch2 ln_pro0 epi4 per16 ln_launch"},
    {"in_proj", 16, "GEMM16K nch2 ln_pro1 epi3 per16"},
    {"out_proj", 16, "GEMM16K nch2 ln_pro0 epi1 per16 writes_stats"},
    {"fc1", 16, "GEMM16S nwv2 groups512 ksplit1 lnp1 per16 reads_stats"},
    {"fc2", 16, "GEMM16S nwv2 groups64 ksplit8 lnp0 per16"},
    {"heads", 16, "GEMM16K nch2 ln_pro0 epi4 per16 ln_launch"},
    {"in_proj", 48, "GEMM16K nch2 ln_pro0 epi3 per0"},
    {"out_proj", 48, "GEMM16K nch2 ln_pro0 epi1 per0"},
    {"fc1", 48, "GEMM64S groups256 ksplit1 per0"},
    {"fc2", 48, "GEMM64S groups32 ksplit8 per0"},
    {"heads", 48, "GEMV ks1 nch4 upw3 blocks385 full0 per4"},
  };
  size_t np = 0;
  for (int rows : {2, 4, 6, 16, 48}) {
    const bool pf = rows == 48;
    LinearEnv e64 = e;
    e64.no_prefill_gemm16k = 2;          // prefill fc1 / fc2: the 64-row kernel only (prefill_linear)
    const LinearPlan in = pf ? plan_linear(e, PRO_NONE, EPI_ROPE_KV, rows, 3072, 2048, 0, true, false, false) : plan_linear(e, PRO_LN, EPI_ROPE_KV, rows, 3072, 2048, 256, false, false, false);
    const LinearPlan out = plan_linear(e, PRO_NONE, EPI_RESID, rows, 2048, 2048, pf ? 0 : 512, pf, !pf, false);
    const LinearPlan fc1 = pf ? plan_linear(e64, PRO_NONE, EPI_SILU, rows, 16384, 2048, 0, true, false, false) : plan_linear(e, PRO_LN, EPI_SILU, rows, 16384, 2048, 512, false, false, out.writes_ln_stats);
    const LinearPlan fc2 = plan_linear(pf ? e64 : e, PRO_NONE, EPI_RESID, rows, 2048, 8192, pf ? 0 : 1024, pf, false, false);
    const LinearPlan heads = plan_linear(e, PRO_LN, EPI_F32, pf ? 2 : rows, 9225, 2048, 512, false, false, false);   // after a prefill: the last position of the two rows
    const LinearPlan* ps[] = {&in, &out, &fc1, &fc2, &heads};
    const char* names[] = {"in_proj", "out_proj", "fc1", "fc2", "heads"};
    for (int k = 0; k < 5; ++k, ++np) {
      if (print) { printf("    {\"%s\", %d, \"%s\"},\n", names[k], rows, describe(*ps[k]).c_str()); continue; }
      CHECK(np < sizeof pinned / sizeof pinned[0] && !strcmp(pinned[np].what, names[k]) && pinned[np].rows == rows && describe(*ps[k]) == pinned[np].plan,
            "%s at %d rows: %s", names[k], rows, describe(*ps[k]).c_str());
    }
  }
  if (print) return 0;
  CHECK(np == sizeof pinned / sizeof pinned[0], "pinned table: %zu entries walked", np);
  printf("plans %lld (errors %lld): GEMV %lld GEMM16 %lld GEMM16S %lld GEMM16K %lld GEMM64S %lld GEMM_TILED %lld\n", g_plans, g_errs, g_kind[0], g_kind[1], g_kind[2],
         g_kind[3], g_kind[4], g_kind[5]);
  for (int k = 0; k < 6; ++k) CHECK(g_kind[k] > 0, "kernel family %d never planned", k);
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

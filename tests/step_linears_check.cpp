// CPU walk of the decode step's table of linears (zonos_amd/csrc/zn_step_linears.h) against the literals the call sites of zn_api.hip carried before the table
// existed: see tests/test_step_linears.py.  The literals below are that frozen behaviour, typed in per model width; nothing here is computed by the table.
#include "zn_step_linears.h"

#include <cstring>
#include <initializer_list>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static bool same_plan(const LinearPlan& a, const LinearPlan& b) {
  return a.kernel == b.kernel && a.epi == b.epi && a.rows_per_launch == b.rows_per_launch && a.row_tiles == b.row_tiles && a.groups_wide == b.groups_wide && a.row_loop == b.row_loop &&
         a.ln_launch == b.ln_launch && a.writes_ln_stats == b.writes_ln_stats && a.reads_ln_stats == b.reads_ln_stats && a.ks == b.ks && a.nch == b.nch && a.units == b.units &&
         a.upw == b.upw && a.blocks == b.blocks && a.full == b.full && a.nw == b.nw && a.tile8 == b.tile8 && a.nwv == b.nwv && a.groups == b.groups && a.ksplit == b.ksplit &&
         a.lnp == b.lnp && a.ln_pro == b.ln_pro && a.w8 == b.w8 && a.err == b.err && !memcmp(a.msg, b.msg, sizeof a.msg);
}

// one linear as its call site wrote it: plan_linear(env, pro, epi, rows, N, K, target, false, want, <stats>); pro_small: the prologue at 1..4 rows where it differs
enum { OFF_NONE, OFF_MLP, OFF_MAMBA };
struct Lit { int lin, pro_small, pro, epi, N, K, target; bool want; int offer; };
struct Model { const char* name; zn_config c; bool in_proj_bias; Lit lits[7]; int n; };

static zn_config transformer(int d, int H, int Hkv, int F, int dbl) {
  zn_config c{};
  c.d_model = d; c.n_layer = 2; c.n_heads = H; c.n_heads_kv = Hkv; c.d_ff = F; c.n_codebooks = 9; c.vocab_head = 1025; c.vocab_embed = 1032; c.double_out_proj = dbl;
  return c;
}
static zn_config hybrid(int d, int H, int Hkv, int F, int d_inner, int d_state, int ngroups, int rope_mode) {
  zn_config c = transformer(d, H, Hkv, F, 0);
  c.arch = 1; c.m_d_inner = d_inner; c.m_headdim = 64; c.m_d_state = d_state; c.m_ngroups = ngroups; c.m_d_conv = 4; c.rope_mode = rope_mode;
  return c;
}
// the targets zn_create sets: in_proj 256, out_proj 512, fc1 512, fc2 1024 (the Mamba2 out_proj too), heads 512
#define TRANSFORMER_LITS(d, nqkv, nq, F)                                                                                                      \
  {{SL_IN_PROJ, PRO_LN, PRO_LN, EPI_ROPE_KV, nqkv, d, 256, false, OFF_NONE}, {SL_OUT_PROJ_FIRST, PRO_NONE, PRO_NONE, EPI_STORE, d, nq, 512, false, OFF_NONE},      \
   {SL_OUT_PROJ, PRO_NONE, PRO_NONE, EPI_RESID, d, nq, 512, true, OFF_NONE}, {SL_FC1, PRO_LN, PRO_LN, EPI_SILU, 2 * F, d, 512, false, OFF_MLP},                 \
   {SL_FC2, PRO_NONE, PRO_NONE, EPI_RESID, d, F, 1024, false, OFF_MLP}, {SL_HEADS, PRO_LN, PRO_LN, EPI_F32, 9225, d, 512, false, OFF_NONE}}
// in_target: (d_in_proj / 2 + 3) / 4; out_small: the out_proj's prologue at 1..4 rows; in_epi: the attention in_proj's epilogue
#define HYBRID_LITS(d, d_in_proj, in_target, d_inner, out_small, in_epi, nqkv, nq, F)                                                         \
  {{SL_M_IN_PROJ, PRO_NONE, PRO_NONE, EPI_MAMBA, d_in_proj, d, in_target, false, OFF_MAMBA}, {SL_M_OUT_PROJ, out_small, PRO_NONE, EPI_STORE, d, d_inner, 1024, false, OFF_MAMBA}, \
   {SL_H_IN_PROJ, PRO_NONE, PRO_NONE, in_epi, nqkv, d, 256, false, OFF_NONE}, {SL_H_OUT_PROJ, PRO_NONE, PRO_NONE, EPI_STORE, d, nq, 512, false, OFF_NONE},          \
   {SL_H_FC1, PRO_NONE, PRO_NONE, EPI_SILU, 2 * F, d, 512, false, OFF_NONE}, {SL_H_FC2, PRO_NONE, PRO_NONE, EPI_STORE, d, F, 1024, false, OFF_NONE},            \
   {SL_H_HEADS, PRO_NONE, PRO_NONE, EPI_F32, 9225, d, 512, false, OFF_NONE}}

static const Model MODELS[] = {
    // synth.FULL_CFG (Zonos-v0.1: 16 heads of 128, 4 KV heads; out_proj applied twice), CHAIN_CFG, TINY_CFG
    {"full", transformer(2048, 16, 4, 8192, 1), false, TRANSFORMER_LITS(2048, 3072, 2048, 8192), 6},
    {"chain", transformer(512, 4, 2, 2048, 1), false, TRANSFORMER_LITS(512, 1024, 512, 2048), 6},
    {"tiny", transformer(128, 4, 2, 256, 0), false, TRANSFORMER_LITS(128, 256, 128, 256), 6},
    // synth.HYBRID_FULL_CFG (d_inner 4096, d_state 128: in_proj 8192 + 256 + 64 rows), HYBRID_TINY_CFG (d_inner 256, d_state 64: 512 + 128 + 4 rows)
    {"hybrid_full", hybrid(2048, 16, 4, 8192, 4096, 128, 1, 0), false, HYBRID_LITS(2048, 8512, 1064, 4096, PRO_GATED, EPI_ROPE_KV, 3072, 2048, 8192), 7},
    {"hybrid_tiny", hybrid(128, 4, 2, 256, 256, 64, 1, 0), false, HYBRID_LITS(128, 644, 81, 256, PRO_GATED, EPI_ROPE_KV, 256, 128, 256), 7},
    // two norm groups (d_state 64: 8192 + 256 + 64 rows): the gated norm is a launch at every row count
    {"hybrid_groups", hybrid(2048, 16, 4, 8192, 4096, 64, 2, 0), false, HYBRID_LITS(2048, 8512, 1064, 4096, PRO_NONE, EPI_ROPE_KV, 3072, 2048, 8192), 7},
    // half-split rotary (the checkpoint's attn_cfg), and interleaved rotary with a qkv bias: the in_proj stores, rotation and KV append follow as a launch
    {"hybrid_half_split", hybrid(2048, 16, 4, 8192, 4096, 128, 1, 1), false, HYBRID_LITS(2048, 8512, 1064, 4096, PRO_GATED, EPI_STORE, 3072, 2048, 8192), 7},
    {"hybrid_qkv_bias", hybrid(2048, 16, 4, 8192, 4096, 128, 1, 0), true, HYBRID_LITS(2048, 8512, 1064, 4096, PRO_GATED, EPI_STORE, 3072, 2048, 8192), 7},
};

int main() {
  long long plans = 0, n_w8 = 0, n_wide = 0, n_stats = 0, n_gated = 0;
  bool seen[SL_COUNT] = {};
  for (const Model& m : MODELS)
    for (int small_rows : {0, 2, 3})
      for (int wide_rows : {0, 1})
        for (int wide_hybrid : {0, 1, 2, 3})
          for (int fc1_ln : {0, 2})
            for (int ws = 0; ws < 2; ++ws) {
              int tune[ZN_TUNE_NKEYS] = {};      // zn_create's defaults, then the keys of this walk
              tune[ZN_TUNE_WG_IN_PROJ] = 256; tune[ZN_TUNE_WG_OUT_PROJ] = 512; tune[ZN_TUNE_WG_FC1] = 512; tune[ZN_TUNE_WG_FC2] = 1024; tune[ZN_TUNE_WG_HEADS] = 512;
              tune[ZN_TUNE_SMALL_M_LDS] = 2; tune[ZN_TUNE_FP8_SMALL_ROWS] = small_rows; tune[ZN_TUNE_WIDE_ROWS] = wide_rows; tune[ZN_TUNE_WIDE_HYBRID] = wide_hybrid;
              tune[ZN_TUNE_FC1_LN_LAUNCH] = fc1_ln;
              LinearEnv base;      // as a generation step's env: wide from 17 rows on unless ZN_TUNE_WIDE_ROWS = 1; the Mamba2 in_proj's form, unset = 4
              base.small_m_lds = 2; base.fc1_ln_launch = fc1_ln; base.wide_rows = wide_rows != 1; base.wide_hybrid = wide_hybrid ? wide_hybrid : 4;
              base.has_g16_part = base.has_ln_part = ws != 0; base.g16_part_bytes = ws ? (size_t)8 << 20 : 0;
              for (int offered = 0; offered < 2; ++offered)
                for (int rows = 1; rows <= 80; ++rows)
                  for (int k = 0; k < m.n; ++k) {
                    const Lit& l = m.lits[k];
                    LinearEnv e = base;      // the offer as the call sites made it (plan_post_attention's em, mamba_env)
                    if (offered && l.offer == OFF_MLP) { e.w8_offered = true; e.w8v_offered = small_rows == 2 || small_rows == 3; }
                    if (offered && l.offer == OFF_MAMBA) { e.w8k_offered = true; e.w8v_offered = small_rows == 2 || small_rows == 3; }
                    const int pro = rows <= 4 ? l.pro_small : l.pro;
                    for (int stats = 0; stats < (l.lin == SL_FC1 ? 2 : 1); ++stats) {
                      const LinearPlan want = plan_linear(e, pro, l.epi, rows, l.N, l.K, l.target, false, l.want, stats != 0);
                      const LinearPlan got = plan_step_linear(base, m.c, tune, l.lin, rows, offered != 0, stats != 0, m.in_proj_bias);
                      ++plans; seen[l.lin] = true;
                      CHECK(same_plan(want, got), "%s linear %d rows %d offered %d stats %d small_rows %d wide_rows %d wide_hybrid %d fc1_ln %d ws %d: kernel %d / %d w8 %d / %d rows_per_launch %d / %d",
                            m.name, l.lin, rows, offered, stats, small_rows, wide_rows, wide_hybrid, fc1_ln, ws, (int)want.kernel, (int)got.kernel, (int)want.w8, (int)got.w8,
                            want.rows_per_launch, got.rows_per_launch);
                      CHECK(!got.err && linear_plan_launchable(got, pro, l.epi), "%s linear %d rows %d: not launchable for <%d, %d> (err %d %s)", m.name, l.lin, rows, pro, l.epi, got.err, got.msg);
                      const StepLinearDesc d = step_linear_desc(m.c, tune, l.lin, rows, m.in_proj_bias);
                      CHECK(d.pro == pro && d.epi == l.epi && d.N == l.N && d.K == l.K && d.target == l.target && d.want_ln_stats == l.want && d.offer == l.offer,
                            "%s linear %d rows %d: the description <%d, %d> %d x %d target %d", m.name, l.lin, rows, d.pro, d.epi, d.N, d.K, d.target);
                      n_w8 += got.w8; n_wide += got.row_tiles > 1; n_stats += got.writes_ln_stats; n_gated += pro == PRO_GATED;
                    }
                  }
            }
  for (int lin = 0; lin < SL_COUNT; ++lin) CHECK(seen[lin], "linear %d of the table was never walked", lin);
  printf("plans %lld: reading FP8 %lld, wide %lld, leaving LayerNorm statistics %lld, gated prologue %lld\n", plans, n_w8, n_wide, n_stats, n_gated);
  CHECK(n_w8 > 0 && n_wide > 0 && n_stats > 0 && n_gated > 0, "a form was never planned");
  printf(g_fail ? "FAIL: %d checks\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}

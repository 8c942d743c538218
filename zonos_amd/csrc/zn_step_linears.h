// Plain C++ (no HIP): the linears of a decode step on the launches path, as ONE table.  What each of them is - prologue, epilogue, shape, GEMV target, statistics
// hand-off, FP8 offer - is said here and nowhere else: the launches of zn_api.hip (launch_step_linear<PRO, EPI>), its plan queries and zn_bench_kernel all plan through
// plan_step_linear, and tests/test_step_linears.py (tests/step_linears_check.cpp, g++) holds the table to the literals the call sites carried before it existed.
#pragma once
#include "../../include/zonos_hip.h"
#include "zn_linear_plan.h"

enum StepLinear {
  // transformer block (_torch.py TransformerBlock) and the heads
  SL_IN_PROJ, SL_OUT_PROJ_FIRST /* double_out_proj: the first of the two calls */, SL_OUT_PROJ, SL_FC1, SL_FC2, SL_HEADS,
  // hybrid stack (mamba_ssm Block): the Mamba2 mixer, the attention layers, the heads
  SL_M_IN_PROJ, SL_M_OUT_PROJ, SL_H_IN_PROJ, SL_H_OUT_PROJ, SL_H_FC1, SL_H_FC2, SL_H_HEADS,
  SL_COUNT
};
enum StepOffer { SO_NONE, SO_MLP /* zn_set_mlp_fp8: w8_offered */, SO_MAMBA /* zn_set_mamba_fp8: w8k_offered */ };   // both: w8v_offered under ZN_TUNE_FP8_SMALL_ROWS = 2, 3

struct StepLinearDesc {
  int pro, epi, N, K;
  int target;            // the GEMV's grid
  bool want_ln_stats;    // asks to leave LayerNorm statistics for its consumer (fc1)
  int offer;             // StepOffer (step_linear_offer)
};

// ZN_TUNE_FP8_SMALL_ROWS: the GEMV launches (1..4 rows) of a projection whose FP8 stream is offered read it (LinearEnv::w8v_offered); 3 = with a ring of two units ahead
inline bool fp8_small_rows_on(const int* tune) { return tune[ZN_TUNE_FP8_SMALL_ROWS] == 2 || tune[ZN_TUNE_FP8_SMALL_ROWS] == 3; }
inline int step_linear_offer(int lin) { return lin == SL_FC1 || lin == SL_FC2 ? SO_MLP : lin == SL_M_IN_PROJ || lin == SL_M_OUT_PROJ ? SO_MAMBA : SO_NONE; }
// RMSNormGated as the prologue of the Mamba2 out_proj: one norm group, up to 4 rows (the GEMV, whose waves hold whole rows); else a launch of its own
inline bool mamba_gated_pro(const zn_config& c, int rows) { return c.m_ngroups == 1 && c.m_d_inner % 8 == 0 && rows <= 4 && c.m_d_inner <= 4096; }

// in_proj_bias: the attention layer of a hybrid stack has a qkv bias (read for SL_H_IN_PROJ only)
inline StepLinearDesc step_linear_desc(const zn_config& c, const int* tune, int lin, int rows, bool in_proj_bias = false) {
  const int d = c.d_model, hd = c.n_heads > 0 ? d / c.n_heads : 0, nq = c.n_heads * hd, nqkv = (c.n_heads + 2 * c.n_heads_kv) * hd, nhead = c.n_codebooks * c.vocab_head;
  const int m_d_in_proj = 2 * c.m_d_inner + 2 * c.m_ngroups * c.m_d_state + (c.m_headdim > 0 ? c.m_d_inner / c.m_headdim : 0);
  const int t_in = tune[ZN_TUNE_WG_IN_PROJ], t_out = tune[ZN_TUNE_WG_OUT_PROJ], t_fc1 = tune[ZN_TUNE_WG_FC1], t_fc2 = tune[ZN_TUNE_WG_FC2], t_hd = tune[ZN_TUNE_WG_HEADS];
  StepLinearDesc r = {-1, -1, 0, 0, 0, false, step_linear_offer(lin)};
  switch (lin) {
    case SL_IN_PROJ:        r = {PRO_LN, EPI_ROPE_KV, nqkv, d, t_in, false, r.offer}; break;
    case SL_OUT_PROJ_FIRST: r = {PRO_NONE, EPI_STORE, d, nq, t_out, false, r.offer}; break;
    case SL_OUT_PROJ:       r = {PRO_NONE, EPI_RESID, d, nq, t_out, true, r.offer}; break;
    case SL_FC1:            r = {PRO_LN, EPI_SILU, 2 * c.d_ff, d, t_fc1, false, r.offer}; break;
    case SL_FC2:            r = {PRO_NONE, EPI_RESID, d, c.d_ff, t_fc2, false, r.offer}; break;
    case SL_HEADS:          r = {PRO_LN, EPI_F32, nhead, d, t_hd, false, r.offer}; break;
    case SL_M_IN_PROJ:      r = {PRO_NONE, EPI_MAMBA, m_d_in_proj, d, (m_d_in_proj / 2 + 3) / 4, false, r.offer}; break;
    case SL_M_OUT_PROJ:     r = {mamba_gated_pro(c, rows) ? PRO_GATED : PRO_NONE, EPI_STORE, d, c.m_d_inner, t_fc2, false, r.offer}; break;
    // MHA: split, interleaved RoPE and the KV append in the epilogue; the other attn_cfg forms (half-split or no rotary, qkv bias) store and a launch follows
    case SL_H_IN_PROJ:      r = {PRO_NONE, c.rope_mode == 0 && !in_proj_bias ? EPI_ROPE_KV : EPI_STORE, nqkv, d, t_in, false, r.offer}; break;
    case SL_H_OUT_PROJ:     r = {PRO_NONE, EPI_STORE, d, nq, t_out, false, r.offer}; break;
    case SL_H_FC1:          r = {PRO_NONE, EPI_SILU, 2 * c.d_ff, d, t_fc1, false, r.offer}; break;
    case SL_H_FC2:          r = {PRO_NONE, EPI_STORE, d, c.d_ff, t_fc2, false, r.offer}; break;
    case SL_H_HEADS:        r = {PRO_NONE, EPI_F32, nhead, d, t_hd, false, r.offer}; break;
  }
  return r;
}

// The plan of linear `lin` over `rows` rows of a generation step: ONE call of plan_linear.  base: the tune values and workspace facts with no offer set; offered: the
// layer's FP8 stream (of the kind the table names for the linear) is attached and not switched off; stats_in: the producer of the rows left LayerNorm statistics
// (writes_ln_stats of its plan: SL_OUT_PROJ -> SL_FC1, the one such pair).
inline LinearPlan plan_step_linear(const LinearEnv& base, const int* tune, const StepLinearDesc& d, int rows, bool offered, bool stats_in) {
  LinearEnv e = base;
  if (offered && d.offer != SO_NONE) {
    (d.offer == SO_MLP ? e.w8_offered : e.w8k_offered) = true;
    e.w8v_offered = fp8_small_rows_on(tune);      // the GEMV launches of 1..4 rows: an offer of its own
  }
  return plan_linear(e, d.pro, d.epi, rows, d.N, d.K, d.target, false, d.want_ln_stats, stats_in);
}
inline LinearPlan plan_step_linear(const LinearEnv& base, const zn_config& c, const int* tune, int lin, int rows, bool offered, bool stats_in, bool in_proj_bias = false) {
  return plan_step_linear(base, tune, step_linear_desc(c, tune, lin, rows, in_proj_bias), rows, offered, stats_in);
}

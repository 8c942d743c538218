// Plain C++ (no HIP): which kernel serves a linear of 1 .. 64 activation rows, decided as a VALUE (plan_linear -> LinearPlan) that the
// launchers of zn_api.hip only follow (launch_linear) and that tests/test_linear_plan.py (tests/linear_plan_check.cpp, g++) walks on the CPU.
#pragma once
#include <cstddef>
#include <cstdio>

enum { PRO_NONE = 0, PRO_LN = 1, PRO_GATED = 2, ZN_NPRO = 3 };
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SILU = 2, EPI_ROPE_KV = 3, EPI_F32 = 4, EPI_MAMBA = 5, ZN_NEPI = 6 };

#define ZN_G16_KC 256          // gemm16s_kernel / gemm64s_kernel: K chunk staged in LDS
#define ZN_G16_LNT 128         // 16-column tiles per row of the LayerNorm statistics (GemvArgs::ln_part_out / ln_part_in)
#define ZN_G16_MAX_GROUPS 1024 // arrival tickets of the split-K combine
#define ZN_G16K_NKW 8          // gemm16k_kernel: waves per workgroup ...
#define ZN_G16K_KCH 128        // ... and K chunk per wave: K = 8 * 128 * {2, 4}

// What a decision may depend on, and nothing else: the tune values (zn_debug_tune; 0 = never set) and the workspace of the handle.
struct LinearEnv {
  int small_m_lds = 2, no_split_small_m = 0, gemm16k_max_tiles = 0, fc1_ln_launch = 0, no_prefill_gemm16k = 0;
  size_t g16_part_bytes = 0;      // split-K partial tiles
  bool has_g16_part = false, has_ln_part = false;
  bool w8_offered = false;        // the caller holds the weights as an FP8 stream as well (zn_fp8_kernels.h) and has not switched it off
  bool w8k_offered = false;       // the same for a GEMM16K projection (the Mamba2 in_proj / out_proj: zn_mamba_fp8_kernels.h); an offer of its own: w8_offered never marks a GEMM16K plan
  bool w8v_offered = false;       // the same for the GEMV of 1..4 decode rows (zn_gemv_fp8_kernels.h; ZN_TUNE_FP8_SMALL_ROWS = 2); an offer of its own: w8_offered and w8k_offered never mark a GEMV plan
  bool wide_rows = false;         // decode steps of more than 16 rows: up to 64 rows per weight pass (plan_linear) instead of groups of 16
  int wide_hybrid = 0;            // under wide_rows, the Mamba2 in_proj (GEMM16K x EPI_MAMBA): 0 / 1 groups of 16, 2 row groups on grid y, 3 the row-tile loop
                                  // (gemm16k_rows_kernel), 4 = the form wide_hybrid_form picks for the row count (ZN_TUNE_WIDE_HYBRID unset)
};

struct LinearPlan {
  enum Kernel { GEMV, GEMM16, GEMM16S, GEMM16K, GEMM64S, GEMM_TILED } kernel = GEMV;
  int epi = 0;                // the epilogue the kernel carries: the one asked for, or (prefill, EPI_ROPE_KV not served) EPI_STORE: rope_kv_rows_kernel follows
  int rows_per_launch = 0;    // 4 (GEMV), 16 (decode MFMA kernels), 64 (the wide plan), 0 = all rows in one launch (prefill)
  int row_tiles = 1;          // 16-row activation blocks per weight pass: 1, or (the wide plan of 17..64 decode rows) 2 .. 4.  GEMM16K: grid y;
                              // GEMM16S: gemm16w_kernel<., ., RB = row_tiles>, whose 64-row workgroups (groups_wide of them) keep ksplit and the
                              // statistics order of nwv
  int groups_wide = 0;
  bool row_loop = false;      // GEMM16K x EPI_MAMBA with row_tiles > 1: gemm16k_rows_kernel (grid y = 1: the workgroup keeps its weight tile as B fragments and walks
                              // the row tiles) instead of gemm16k_kernel's row groups on grid y
  bool ln_launch = false;     // a layernorm_kernel launch over the rows of each group runs first (into nbuf)
  bool writes_ln_stats = false, reads_ln_stats = false;   // LayerNorm statistics per 16-column tile: left by this launch / normalised from
  // GEMV: K slices per row pair, 512-wide chunks per slice, units (weight-row pairs) and units per wave (ks 1) or block (ks 4), grid, mask-free
  int ks = 0, nch = 0, units = 0, upw = 0, blocks = 0;
  bool full = false;
  int nw = 0; bool tile8 = false;                  // GEMM16 (direct fragments): waves per workgroup, 8-row instead of 16-row weight tiles
  int nwv = 0, groups = 0, ksplit = 0; bool lnp = false;   // GEMM16S / GEMM64S: 16-row tiles per workgroup, grid x, grid y; LayerNorm from handed-over statistics
  bool ln_pro = false;        // GEMM16K (nch = 128-wide chunks per wave): LayerNorm as its prologue
  bool w8 = false;            // GEMM16S, decode: the launch reads the FP8 stream (gemm16s_kernel<., NWV | ZN_G16S_W8>) instead of the bf16 weights;
                              // GEMM16K, decode (LinearEnv::w8k_offered): gemm16k8_kernel / gemm16k8_rows_kernel in place of gemm16k_kernel / gemm16k_rows_kernel;
                              // GEMV, decode (LinearEnv::w8v_offered): gemv8_kernel in place of gemv_kernel
  int err = 0;                // shapes nobody serves: a ZN_ERR_* code (-4 = ZN_ERR_UNSUPPORTED) and its message
  char msg[96] = {};
};

// ---------------------------------------------------------------------------- the instantiations launch_linear<PRO, EPI> holds: one table for
// its `if constexpr` guards and for the CPU walk
constexpr bool lin_has_gemv_ks4(int pro) { return pro == PRO_NONE || pro == PRO_GATED; }
constexpr bool lin_has_gemm16(int pro) { return pro != PRO_GATED; }                         // GEMM16, GEMM16S, GEMM16K: no gated-norm prologue
constexpr bool lin_has_tile8(int epi) { return epi != EPI_SILU; }
constexpr bool lin_has_lnp(int pro, int epi) { return pro == PRO_LN && epi == EPI_SILU; }
constexpr bool lin_has_gemm16k(int pro, int epi) { return lin_has_gemm16(pro) && epi != EPI_SILU; }   // row-pair epilogues only
constexpr bool lin_has_gemm16k_ln(int pro, int nch) { return pro == PRO_LN && nch == 2; }  // (the LayerNorm prologue at K = 4096 would not fit the register file)
constexpr bool lin_has_gemm16k_rows(int pro, int epi, int nch) { return pro == PRO_NONE && epi == EPI_MAMBA && nch == 2; }   // gemm16k_rows_kernel: the Mamba2 in_proj at K = 2048, what production launches
// gemm16s_kernel<., NWV | ZN_G16S_W8>: fc1 (SiLU gate; its LayerNorm is a launch in front or comes from handed-over statistics, so the kernel's prologue is none
// either way) and fc2 (no prologue, residual)
constexpr bool lin_has_w8(int pro, int epi) { return (epi == EPI_SILU && (pro == PRO_NONE || pro == PRO_LN)) || (epi == EPI_RESID && pro == PRO_NONE); }
// gemm16k8_kernel<EPI, NCH> / gemm16k8_rows_kernel<2> (zn_mamba_fp8_kernels.h): the Mamba2 in_proj (no prologue, K = 2048) and out_proj (no prologue, store, K = 4096)
constexpr bool lin_has_w8k(int pro, int epi, int nch) { return pro == PRO_NONE && ((epi == EPI_MAMBA && nch == 2) || (epi == EPI_STORE && nch == 4)); }
// gemv8_kernel<R, NCH, KS, PRO, EPI, ., .> (zn_gemv_fp8_kernels.h), R = 2 and 4: what production launches at 1..4 rows - the transformer's fc1 (LayerNorm, SiLU gate, K = 2048)
// and fc2 (residual, K = 8192 in four quarters), the Mamba2 in_proj (K = 2048) and out_proj (K = 4096 in four quarters; gated-norm prologue with one norm group, else none)
constexpr bool lin_has_w8v(int pro, int epi, int ks, int nch) {
  return (pro == PRO_LN && epi == EPI_SILU && ks == 1 && nch == 4) || (pro == PRO_NONE && epi == EPI_RESID && ks == 4 && nch == 4) ||
         (pro == PRO_NONE && epi == EPI_MAMBA && ks == 1 && nch == 4) || ((pro == PRO_GATED || pro == PRO_NONE) && epi == EPI_STORE && ks == 4 && nch == 2);
}
// gemm16w_kernel (zn_wide_kernels.h), decode steps of 17..64 rows: fc1 (SiLU gate; LayerNorm none, from a launch, or from handed-over statistics) and fc2 (residual)
constexpr bool lin_has_wide16s(int pro, int epi) { return (epi == EPI_SILU && (pro == PRO_NONE || pro == PRO_LN)) || (epi == EPI_RESID && pro == PRO_NONE); }
constexpr bool lin_has_prefill(int pro, int epi) { return pro == PRO_NONE && (epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SILU); }   // GEMM64S, GEMM_TILED
inline bool linear_plan_launchable(const LinearPlan& p, int pro, int epi) {
  switch (p.kernel) {
    case LinearPlan::GEMV: return (p.ks == 1 || (p.ks == 4 && lin_has_gemv_ks4(pro))) && (p.nch == 1 || p.nch == 2 || p.nch == 4 || p.nch == 8) &&
                                  (!p.w8 || lin_has_w8v(pro, epi, p.ks, p.nch));
    case LinearPlan::GEMM16: return lin_has_gemm16(pro) && (p.nw == 4 || p.nw == 8 || p.nw == 16) && (!p.tile8 || lin_has_tile8(epi));
    case LinearPlan::GEMM16S: return lin_has_gemm16(pro) && (p.nwv == 2 || p.nwv == 4) && (!p.lnp || lin_has_lnp(pro, epi)) && (!p.w8 || lin_has_w8(pro, epi)) &&
                                     (p.row_tiles == 1 || (p.row_tiles >= 2 && p.row_tiles <= 4 && lin_has_wide16s(pro, epi)));
    case LinearPlan::GEMM16K: return (p.row_tiles >= 1 && p.row_tiles <= 4) && lin_has_gemm16k(pro, epi) && (p.nch == 2 || p.nch == 4) && (!p.ln_pro || lin_has_gemm16k_ln(pro, p.nch)) &&
                                     (!p.row_loop || (p.row_tiles >= 2 && !p.ln_pro && lin_has_gemm16k_rows(pro, epi, p.nch))) &&
                                     (!p.w8 || (!p.ln_pro && lin_has_w8k(pro, epi, p.nch)));
    case LinearPlan::GEMM64S: case LinearPlan::GEMM_TILED: return !p.w8 && lin_has_prefill(pro, epi);
  }
  return false;
}

// ---------------------------------------------------------------------------- the decisions
// rows in (4, 16] (and short prompts up to 64), K = 8 waves x 128 x {2, 4} and few weight rows (the LDS-staged kernel would have to split K over
// workgroups): one 16-row tile per workgroup, K split over its waves, no cross-workgroup combine.  ZN_TUNE_NO_SPLIT_SMALL_M = 2 disables.
inline bool gemm16k_fits(const LinearEnv& e, int epi, int N, int K) {
  if (epi == EPI_SILU || e.small_m_lds <= 1 || e.no_split_small_m == 2) return false;
  const int per = ZN_G16K_NKW * ZN_G16K_KCH, nch = K / per;
  if (K % per || (nch != 2 && nch != 4)) return false;
  return (N + 15) / 16 < (e.gemm16k_max_tiles > 0 ? e.gemm16k_max_tiles : 1024);     // many rows: the 64-row workgroups fill the chip without a split (ZN_TUNE_GEMM16K_MAX_TILES: the tile count from which they take over)
}

// rows in (4, 16], K a multiple of 256: the LDS-staged kernel (coalesced weight stream); K is split over workgroups until the grid has
// >= 512 of them, the partial tiles meet in a scratch buffer.  false = shape not served.
inline bool plan_gemm16s(const LinearEnv& e, int epi, int N, int K, bool lnp, LinearPlan& p) {
  if (K % ZN_G16_KC || !e.has_g16_part) return false;
  if (lnp && K != 16 * ZN_G16_LNT) return false;
  const int nrows_w = (epi == EPI_SILU) ? N / 2 : N;          // weight rows that define the grid
  const int per64 = (epi == EPI_SILU) ? 32 : 64;
  // 64-row workgroups when that already gives >= 512 of them, else 32-row ones, else split K as well
  int nwv = 4, groups = (nrows_w + per64 - 1) / per64;
  if (groups < 512) { nwv = 2; groups = (nrows_w + per64 / 2 - 1) / (per64 / 2); }
  if (groups > ZN_G16_MAX_GROUPS) return false;
  int ks = 1;
  while (groups * ks < 448 && ks < 16 && K % (2 * ks * ZN_G16_KC) == 0) ks *= 2;
  // (fc2 at 16 rows, K = 8192 over 64 groups: 8 slices; 4: 1.690, 8: 1.681, 16: 1.746 ms per batch-8 step)
  // (the Mamba2 in_proj, N = 8512 over 266 groups: 1 / 2 (default) / 4 slices: 1.933 / 1.937 / 1.945 ms per batch-8 hybrid step)
  if (ks > 1 && K / ks < 512) {
    // short slices: the combine costs more than the direct-fragment kernel's access pattern, unless a shallower split
    // still fills the chip (in_proj, N = 3072: 96 groups x 4 slices of 512)
    ks /= 2;
    if (ks < 2 || K / ks < 512 || groups * ks < 320) return false;
  }
  if ((size_t)ks * 16 * groups * nwv * 16 * sizeof(float) > e.g16_part_bytes) return false;
  p.kernel = LinearPlan::GEMM16S; p.nwv = nwv; p.groups = groups; p.ksplit = ks; p.lnp = lnp;
  return true;
}

// Projection of a short prompt (17..64 rows) through the weight-streaming 64-row kernel; false = shape not served.
inline bool plan_gemm64s(const LinearEnv& e, int epi, int rows, int N, int K, LinearPlan& p) {
  if (rows > 64 || K % 256 || (epi == EPI_SILU && (N / 2) % 32) || e.small_m_lds <= 1) return false;
  const int groups = (epi == EPI_SILU) ? (N / 2 + 31) / 32 : (N + 63) / 64;
  if (groups > ZN_G16_MAX_GROUPS) return false;
  int ks = 1;
  while (groups * ks < 256 && ks < 16 && K % (2 * ks * 256) == 0) ks *= 2;
  // (fc2, K = 8192: the split this picks, 8, against 4 / 16 / 2 forced: prefill 2.71 vs 2.90 / 2.77 / 3.13 ms)
  if ((size_t)ks * 64 * groups * 64 * sizeof(float) > e.g16_part_bytes) return false;
  p.kernel = LinearPlan::GEMM64S; p.nwv = 4; p.groups = groups; p.ksplit = ks;
  return true;
}

// The plan of out [rows][N] = epi(pro(x [rows][K]) W^T).  Decode (prefill = false): rows <= 4 the fused GEMV (groups of <= 4 rows per launch),
// rows in (4, 16] per group one weight pass on the matrix cores.  prefill = true: the rows of a prompt in one launch, normalised by the caller.
// want_ln_stats_out: the caller would hand LayerNorm statistics of this projection's output to its consumer; have_ln_stats_in: the producer of
// x left them (writes_ln_stats of its plan).  target_blocks: the GEMV's grid (ZN_TUNE_WG_*).
inline LinearPlan plan_linear_bf16(const LinearEnv& e, int pro, int epi, int rows, int N, int K, int target_blocks, bool prefill, bool want_ln_stats_out,
                                   bool have_ln_stats_in) {
  LinearPlan p;
  p.epi = epi;
#define ZN_PLAN_FAIL(...) do { p.err = -4; snprintf(p.msg, sizeof p.msg, __VA_ARGS__); return p; } while (0)
  if (prefill) {
    if (pro != PRO_NONE || !(lin_has_prefill(pro, epi) || epi == EPI_ROPE_KV)) ZN_PLAN_FAIL("prefill linear: prologue %d / epilogue %d not served", pro, epi);
    // Short prompts (<= 64 rows), contractions of 2048 or 4096 with few weight rows (in_proj, both out_proj calls): the decode side's gemm16k_kernel
    // over ceil(rows / 16) row groups in ONE launch, instead of gemm64s_kernel's 8-way split-K with a ticketed combine (14.4 us for 8-13 MB).
    // in_proj at K = 2048: split, RoPE and the KV append in its epilogue, as in a decode step; else they follow as a launch.
    const bool k16 = rows <= 64 && gemm16k_fits(e, epi, N, K) && e.no_prefill_gemm16k != 2;
    if (epi == EPI_ROPE_KV && !(k16 && K / (ZN_G16K_NKW * ZN_G16K_KCH) == 2)) p.epi = epi = EPI_STORE;
    if (k16) { p.kernel = LinearPlan::GEMM16K; p.nch = K / (ZN_G16K_NKW * ZN_G16K_KCH); return p; }
    if (!plan_gemm64s(e, epi, rows, N, K, p)) {
      // gemm_bf16_kernel walks K in whole 32-wide fragments: a shorter tail would read into the next row
      if (K % 32) ZN_PLAN_FAIL("tiled gemm: K=%d not a multiple of 32", K);
      p.kernel = LinearPlan::GEMM_TILED;
    }
    return p;
  }
  if (rows <= 4) {
    p.kernel = LinearPlan::GEMV; p.rows_per_launch = 4;
    p.ks = ((pro == PRO_NONE || pro == PRO_GATED) && K >= 4096 && K % 2048 == 0) ? 4 : 1;
    const int kw = K / p.ks, nch = (kw + 511) / 512;
    p.nch = nch <= 1 ? 1 : nch <= 2 ? 2 : nch <= 4 ? 4 : nch <= 8 ? 8 : 99;
    if (p.nch > 8) ZN_PLAN_FAIL("gemv: K=%d too large for the register-resident activation path", K);
    p.units = (epi == EPI_SILU) ? N / 2 : (N + 1) / 2;
    const int lanes_units = (p.ks == 1) ? 4 : 1;  // units in flight per block
    p.upw = (p.units + target_blocks * lanes_units - 1) / (target_blocks * lanes_units);
    if (p.upw < 1) p.upw = 1;
    p.blocks = (p.units + p.upw * lanes_units - 1) / (p.upw * lanes_units);
    p.full = (kw == p.nch * 512) && (N % 2 == 0) && (p.units == p.blocks * lanes_units * p.upw);
    return p;
  }
  // rows in (4, 16]: LayerNorm, when fused in the GEMV, is a row-wise launch here (amortised over the batch) unless a kernel below takes it in
  if (pro == PRO_GATED) ZN_PLAN_FAIL("gated-norm prologue: at most 4 rows (got %d)", rows);
  p.rows_per_launch = 16;
  // few weight-row tiles (N = d_model: 128 workgroups) -> more waves per workgroup so that every CU still keeps enough loads in flight
  const int tiles = (epi == EPI_SILU) ? (N / 2) / 16 : (N + 15) / 16;
  p.nw = 4;
  if (tiles <= 256 && K % 256 == 0) p.nw = 8;
  if (tiles <= 256 && K >= 8192 && K % 512 == 0) p.nw = 16;
  if (K % (p.nw * 32)) ZN_PLAN_FAIL("gemm16: K=%d not a multiple of %d", K, p.nw * 32);
  if (epi == EPI_SILU && (N / 2) % 16) ZN_PLAN_FAIL("gemm16: d_ff must be a multiple of 16");
  const bool k16 = gemm16k_fits(e, epi, N, K);
  // the producer of these rows left LayerNorm statistics per 16-column tile (plan_post_attention): fc1 normalises while it stages
  if (lin_has_lnp(pro, epi) && have_ln_stats_in && !k16 && e.small_m_lds > 1 && plan_gemm16s(e, epi, N, K, true, p)) { p.reads_ln_stats = true; return p; }
  // gemm16k normalises its rows itself when at most one workgroup per CU repeats the statistics (in_proj: 8.7 us vs 4.8 + 6.2; the heads' 577
  // tiles: 21.8 vs 5.0 + 11.9)
  p.ln_pro = k16 && pro == PRO_LN && tiles <= 256 && K == 2 * ZN_G16K_NKW * ZN_G16K_KCH;
  p.ln_launch = pro == PRO_LN && !p.ln_pro;
  if (k16) {
    // rows 5..16: the projection that completes the residual stream leaves LayerNorm statistics per 16-column tile and fc1 normalises its
    // activation chunks from them - no LayerNorm launch in between.  ZN_TUNE_FC1_LN_LAUNCH = 2: the launch.
    p.writes_ln_stats = want_ln_stats_out && e.fc1_ln_launch != 2 && e.has_ln_part && epi == EPI_RESID && N == 16 * ZN_G16_LNT;
    p.kernel = LinearPlan::GEMM16K; p.nch = K / (ZN_G16K_NKW * ZN_G16K_KCH);
    return p;
  }
  if (e.small_m_lds > 1 && plan_gemm16s(e, epi, N, K, false, p)) return p;
  p.kernel = LinearPlan::GEMM16;
  p.tile8 = lin_has_tile8(epi) && tiles <= 192 && N % 8 == 0;   // N = d_model: 8-row tiles so that every CU gets a workgroup
  p.blocks = p.tile8 ? N / 8 : tiles;
  return p;
#undef ZN_PLAN_FAIL
}

#define ZN_WIDE_ROWS 64       // activation rows per weight pass of the wide plan
// The form of the Mamba2 in_proj (GEMM16K x EPI_MAMBA) over a group of `rows` rows (17..64) when ZN_TUNE_WIDE_HYBRID is unset: 1 groups of 16, 2 row groups on
// grid y, 3 the row-tile loop.  The loop at EVERY row count: measured (tools/hybridwidebench.py, profiles/hybridwidebench.txt; Zonos-v0.1-hybrid shapes, in_proj
// 8512 x 2048, medians of 20 alternated repetitions, us per in_proj, groups of 16 / grid y / loop) 18 rows 21.58 / 17.23 / 15.25, 32 rows 23.77 / 19.64 / 18.70,
// 48 rows 34.93 / 26.33 / 24.08, 64 rows 46.10 / 33.22 / 29.76 (the repetitions spread by <= 0.27 us); ms per decode step of the 46-layer stack 18 rows 2.581 /
// 2.379 / 2.300, 32 rows 2.886 / 2.691 / 2.654, 48 rows 4.009 / 3.632 / 3.514, 64 rows 4.878 / 4.316 / 4.136 (spread <= 0.074 ms)
inline int wide_hybrid_form(int rows) { (void)rows; return 3; }
// The wide form of a 16-row decode plan p16 for a group of `rows` rows (17..64; more rows run in groups of 64, the last group planned by its own
// size): what fixes an output bit - the kernel family, ksplit (slice boundaries, in-order addition), the order of the tile statistics (nwv), every
// LayerNorm decision - stays p16's; the activation rows of one weight pass grow to 16 * row_tiles.  Returns p16 itself where no wide form exists.
inline LinearPlan plan_wide(const LinearEnv& e, const LinearPlan& p16, int pro, int epi, int rows, int N) {
  if (p16.err || rows <= 16) return p16;
  LinearPlan p = p16;
  const int tiles = ((rows < ZN_WIDE_ROWS ? rows : ZN_WIDE_ROWS) + 15) / 16;
  if (p16.kernel == LinearPlan::GEMM16K) {
    // one launch, grid y = row tiles: the tile's weights come from HBM once and from the XCD's L2 for the other row groups, as in a short prefill
    // (us per projection at 32 / 64 rows, groups of 16 -> one launch: in_proj 16.4 -> 14.9 / 32.4 -> 22.0, out_proj 10.4 -> 5.4 / 20.4 -> 7.9, heads 25.8 -> 20.0 / 51.1 -> 35.8).
    if (epi == EPI_MAMBA) {
      // The Mamba2 in_proj (8512 x 2048 at the hybrid checkpoint's sizes): LinearEnv::wide_hybrid picks groups of 16, the row groups on grid y above (conv
      // window and xBC of row group y: the kernel's blockIdx.y block), or the row-tile loop, which requests the weight tile once and keeps it as B fragments
      // while it walks the row tiles - no re-read through L2 per 16 rows.  The loop exists for what production launches (lin_has_gemm16k_rows); elsewhere
      // form 3 is form 2.
      const int form = e.wide_hybrid == 4 ? wide_hybrid_form(rows < ZN_WIDE_ROWS ? rows : ZN_WIDE_ROWS) : e.wide_hybrid;
      if (form != 2 && form != 3) return p16;
      p.row_loop = form == 3 && !p16.ln_pro && lin_has_gemm16k_rows(pro, epi, p16.nch);
    }
    p.rows_per_launch = ZN_WIDE_ROWS; p.row_tiles = tiles;
    return p;
  }
  if (p16.kernel != LinearPlan::GEMM16S || !lin_has_wide16s(pro, epi)) return p16;   // GEMM16 direct fragments, the Mamba2 projections, STORE, F32
  const int nrows_w = (epi == EPI_SILU) ? N / 2 : N, per = (epi == EPI_SILU) ? 32 : 64;
  const int groups = (nrows_w + per - 1) / per;      // (fc1 at 32 / 64 rows: 31.6 -> 19.6 / 62.9 -> 22.5 us, fc2 23.9 -> 13.0 / 47.3 -> 18.3; other workgroup sizes not measured)
  if ((size_t)p16.ksplit * 16 * tiles * groups * 64 * sizeof(float) > e.g16_part_bytes) return p16;   // partial tiles [ksplit][16 row_tiles][64 groups] fp32
  p.rows_per_launch = ZN_WIDE_ROWS; p.row_tiles = tiles; p.groups_wide = groups;
  return p;
}

// The plan, and on top of it the one thing an offered FP8 stream changes: a decode launch of gemm16s_kernel for fc1 or fc2 reads the stream.
// Kernel, grid, split, statistics hand-over - everything else is decided without looking at the offer.
inline LinearPlan plan_linear(const LinearEnv& e, int pro, int epi, int rows, int N, int K, int target_blocks, bool prefill, bool want_ln_stats_out,
                              bool have_ln_stats_in) {
  LinearPlan p = plan_linear_bf16(e, pro, epi, rows, N, K, target_blocks, prefill, want_ln_stats_out, have_ln_stats_in);
  p.w8 = e.w8_offered && !prefill && !p.err && p.kernel == LinearPlan::GEMM16S && lin_has_w8(pro, epi);
  // ... and a decode launch of gemm16k_kernel / gemm16k_rows_kernel for the Mamba2 in_proj or out_proj reads its stream (w8k_offered), at EVERY row count from 5 on:
  // measured (tools/hybridfp8bench.py, profiles/hybridfp8bench.txt; Zonos-v0.1-hybrid shapes, one quantised model, the stream against the bf16 copy under
  // ZN_TUNE_MAMBA_FP8 = 2, medians of 20 alternated repetitions, FP8 / bf16) us per in_proj (8512 x 2048) 8 rows 7.57 / 10.67, 16 rows 9.76 / 12.35, 18 rows
  // 12.43 / 15.25, 32 rows 15.59 / 18.73, 48 rows 21.34 / 24.17, 64 rows 27.13 / 29.91; us per out_proj (2048 x 4096) 5.87 / 6.56, 7.23 / 7.79, 7.31 / 7.92,
  // 7.25 / 7.75, 11.45 / 12.93, 11.43 / 12.82 (the repetitions spread by <= 0.18 us); ms per decode step of the 46-layer stack 8 rows 1.519 / 1.664, 16 rows
  // 1.864 / 1.988, 18 rows 2.176 / 2.323, 32 rows 2.522 / 2.691, 48 rows 3.348 / 3.545, 64 rows 3.973 / 4.175 (spread <= 0.08 ms, 0.20 at 64 rows): no band
  // of row counts in which the stream is slower, so none is declined
  if (e.w8k_offered && !prefill && !p.err && p.kernel == LinearPlan::GEMM16K && !p.ln_pro && lin_has_w8k(pro, epi, p.nch)) p.w8 = true;
  // ... and a decode GEMV launch (1..4 rows) of fc1, fc2 or a Mamba2 projection reads its stream (w8v_offered) where gemv8_kernel has the instantiation.
  // At EVERY (projection, row count): measured (tools/smallrowsbench.py, profiles/smallrowsbench.txt; Zonos-v0.1 and Zonos-v0.1-hybrid shapes, one quantised model, the
  // stream against the bf16 GEMV with ZN_TUNE_FP8_SMALL_ROWS unset, medians of 20 alternated repetitions, us per launch at 1 / 2 / 3 / 4 rows, FP8 : bf16) fc1
  // 11.57 : 14.78, 9.78 : 13.49, 20.20 : 22.59, 12.09 : 14.84; fc2 5.63 : 7.61, 6.34 : 8.15, 7.32 : 9.91, 7.95 : 9.32; in_proj (8512 x 2048) 7.38 : 9.57, 6.83 : 8.78,
  // 9.06 : 10.62, 8.48 : 10.47; out_proj with the gated norm 5.66 : 6.30, 5.64 : 6.70, 8.13 : 8.56, 7.88 : 8.64; out_proj without it 4.27 : 5.01, 4.08 : 5.22,
  // 4.84 : 5.64, 5.23 : 6.16 (the repetitions spread by <= 0.36 us, 0.70 for the gated out_proj at 2 rows: below every difference); ms per decode step of the
  // 46-layer hybrid stack 1.078 : 1.202 (1 guided utterance), 1.271 : 1.389 (2), 1.053 : 1.170 (1 unguided), 1.305 : 1.396 (3), of the 26-layer transformer
  // 1.148 : 1.245 (2 guided utterances), 0.978 : 1.120 (a one-slot session) (spread <= 0.05 ms): no (projection, row count) where the stream is slower, so none
  // is declined
  if (e.w8v_offered && !prefill && !p.err && p.kernel == LinearPlan::GEMV && rows <= 4 && lin_has_w8v(pro, epi, p.ks, p.nch)) p.w8 = true;
  // LinearEnv::wide_rows, decode, more than 16 rows: the same plan over up to 64 rows per weight pass (plan_wide).  Wide at EVERY row count from 17 on:
  // measured (tools/widebench.py, profiles/widebench.txt; Zonos-v0.1 shapes, medians of 20, ms per decode step, groups of 16 -> wide) 18 rows 2.630 -> 1.771,
  // 32 rows 2.723 -> 1.822, 48 rows 4.178 -> 2.400, 64 rows 5.495 -> 2.585 (FP8 stream: 2.490 -> 1.633 ... 5.186 -> 2.445); the repetitions spread by <= 0.04 ms
  if (e.wide_rows && !prefill && rows > 16) return plan_wide(e, p, pro, epi, rows, N);
  return p;
}

// libzonos_hip.so — C ABI (include/zonos_hip.h) over the gfx950 kernels.  Host logic only: argument checks,
// workspace, launch geometry, hipGraph capture of one decode step.
#include "../../include/zonos_hip.h"
#include "zn_decode_kernels.h"
#include "zn_attn_fp8_kernels.h"
#include "zn_wide_kernels.h"
#include "zn_mamba_fp8_kernels.h"
#include "zn_gemv_fp8_kernels.h"
#include "zn_chain_kernel.h"
#include "zn_step_kernel.h"
#include "zn_prefill_kernels.h"
#include "zn_prefill_attn_fp8_kernels.h"
#include "zn_cond_kernels.h"
#include "zn_mamba_kernels.h"
#include "zn_step_linears.h"
#include "zn_gen_state.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

static thread_local std::string g_create_err;
#define ZN_GRAPH_STEPS 8
#define ZN_G16_PART_BYTES ((size_t)8 << 20)
#define ZN_REARM_AFTER 4

// How the next decode steps run (plan_steps): the one record zn_decode_steps, enqueue_step and decode_blocks agree through.
struct StepPlan {
  enum Path { LAUNCHES, CHAIN, STACK } path = LAUNCHES;   // one launch per op; one chain launch per block; the whole-step kernel
  int nbk = 0;              // STACK: key blocks (rows * Hkv attention workgroups each) of the launch
  int attn_fused = 0;       // LAUNCHES, CHAIN: shape of the attention launches (attn_fused_for)
  int run = 1;              // steps enqueued together: 1, or ZN_GRAPH_STEPS (one graph)
  bool fused_tail = false;  // the step reads its embedding from x_emb and its sampler launch leaves the next step's
  int graph_slot = 0;       // index into graph_exec (graph_slot_for)
};

struct zn_handle_s {
  zn_config cfg;
  int max_rows = 0, hd = 0, G = 0;
  std::vector<zn_layer_weights> layers;
  // optional FP8 stream of a layer's fc1 / fc2 (zn_set_mlp_fp8): E4M3 codes [N][K] and a scale exponent per weight row; the layer's bf16 fc1 / fc2
  // hold the dequantised values, and every kernel but gemm16s_kernel<., NWV | ZN_G16S_W8> reads those
  struct MlpFp8 { const uint8_t *fc1_q = nullptr, *fc2_q = nullptr; const int8_t *fc1_exp = nullptr, *fc2_exp = nullptr; };
  std::vector<MlpFp8> mlp_fp8;
  // the same for a Mamba2 layer's in_proj / out_proj (zn_set_mamba_fp8); read by gemm16k8_kernel / gemm16k8_rows_kernel only
  struct MambaFp8 { const uint8_t *in_q = nullptr, *out_q = nullptr; const int8_t *in_exp = nullptr, *out_exp = nullptr; };
  std::vector<MambaFp8> mamba_fp8;
  // FP8 KV cache (zn_set_kv_fp8): the mode and the code cache of the per-op entry points (this generation's code caches: gen.kv8_layers)
  bool kv_fp8 = false;
  bool kv_fp8_only = false;          // zn_set_kv_fp8_only: where the FP8 KV cache is in effect, the code caches are the only KV storage (no bf16 cache)
  uint8_t* op_kv8 = nullptr;
  const void* heads = nullptr;
  const void *norm_f_w = nullptr, *norm_f_b = nullptr;
  const float* rope = nullptr;
  const bf16_t** emb_tables_dev = nullptr;
  bool has_io = false;  // embeddings + heads bound (false: backbone-only handle)
  // workspace (device)
  bf16_t *x = nullptr, *q = nullptr, *o1 = nullptr, *mbuf = nullptr, *nbuf = nullptr;
  // hybrid backbone (arch 1): residual stream, normalised activations, Mamba2 intermediates
  bf16_t *res = nullptr, *hn = nullptr, *m_zx = nullptr, *m_xbc = nullptr, *m_y = nullptr, *m_g = nullptr;
  float* m_vg = nullptr;            // [rows][m_d_inner] fp32 y * silu(z) (mamba_ssm_kernel -> out_proj prologue)
  int m_nheads = 0, m_conv_dim = 0, m_d_in_proj = 0;
  // persistent post-attention chain (zn_chain_kernel.h): granule buffers of the four in-launch hand-offs ([rows][len / 2] x 8 B),
  // the launch epoch (tag), the second residual-stream buffer (blocks alternate h->x / ch_x2)
  unsigned long long *ch_gy1 = nullptr, *ch_gx1 = nullptr, *ch_gx2 = nullptr, *ch_gm = nullptr;
  unsigned long long *ch_gqkv = nullptr, *ch_ga = nullptr;   // whole-step kernel: q | k | v of the next block, attention output
  unsigned long long *ch_gbmax = nullptr, *ch_gpart = nullptr;   // key-block attention role: per-block score maxima and P.V partials (zn_step_kernel.h)
  bool stackv_ok[4] = {};                    // whole-step kernel instantiations 1 .. 3 that fit this model and device (stack_variant_ok)
  bool stackv1_ok[4] = {};                   // the same for the one-row kernel (step_r1_kernel: generations without guidance)
  StackLayer* stack_layers = nullptr;        // device table [n_layer], rebuilt by zn_gen_begin (it holds the KV cache pointers)
  bool stack_ok = false, stack1_ok = false, stack_checked = false;   // two rows / one row: the whole-step kernel fits (stack_shapes_ok, asked once)
  unsigned* ch_epoch = nullptr;
  unsigned long long epoch_bound = 1;        // host-side upper bound of the device epoch (tags advance by one per block of every decode step enqueued)
  unsigned* ch_diag = nullptr;               // [16] words: [0..7] the first hand-off wait that timed out describes itself (sweep_granules); [8] the longest hand-off wait a whole-step launch measured (10 ns ticks), [9] waits beyond 0.2 ms (StepPacer::report)
  unsigned diag_host[8] = {};
  bf16_t* ch_x2 = nullptr;
  bf16_t* dbg_trace = nullptr;               // diagnostic: [n_layer][2][rows * d] copies of (x after the block, attention output) per decode step
  bf16_t* x_emb = nullptr;                  // [max_rows][d] embedding of the column the next decode step consumes (written by the step's tail)
  int* tail_ticket = nullptr;               // arrival ticket of the sampler launch whose last workgroup runs the step's tail
  unsigned long long* ch_stamps = nullptr;   // diagnostic: [n_layer][32] timeline stamps of workgroup 0 (zn_debug_chain_stamps)
  int device = 0;              // the HIP device the handle was created on
  // hand-off timeouts (zn_get_counters): a reported timeout demotes the handle to the launches path (no in-launch hand-offs) until ZN_REARM_AFTER
  // generations in a row have completed there cleanly, or zn_debug_tune(ZN_TUNE_PERSISTENT, 1) re-arms it at once
  bool demoted = false;
  int clean_since_demotion = 0;
  long long n_timeouts = 0, n_generations = 0, n_fallback_generations = 0, n_rearms = 0;
  hipStream_t gen_stream = nullptr;   // the stream the generation's steps were last enqueued on (handoff_timeout drains it)
  int ch_variant = 0;          // 0 = shapes do not fit (launches path), 1 = <4,1,8,4,2> (Zonos-v0.1 dims), 2 = <1,1,2,1,1> (d_model 512)
  float* g16_part = nullptr;   // gemm16s_kernel: split-K partial tiles
  int* g16_tickets = nullptr;
  size_t g16_part_bytes = 0;
  float* ln_part = nullptr;    // LayerNorm statistics per (row, 16-column tile) handed from out_proj's epilogue to fc1 (rows 5..16): [max_rows][ZN_G16_LNT][2]
  float *logits_raw = nullptr, *last_logits = nullptr;
  int* tok_raw = nullptr;
  float *scores = nullptr, *cmax = nullptr;
  float* pv_part = nullptr;    // split P.V pass: partials per (row, kv head, block)
  int* pv_tickets = nullptr;
  bf16_t *pf_x = nullptr, *pf_n = nullptr, *pf_qkv = nullptr, *pf_a = nullptr, *pf_u = nullptr, *pf_m = nullptr;   // batched-prefill workspace
  // hybrid batched prefill: residual stream (bf16, or fp32 with residual_in_fp32), in_proj output, conv output, scan output, gated-normalised
  bf16_t *pf_res = nullptr, *pf_zx = nullptr, *pf_xbc = nullptr, *pf_y = nullptr, *pf_g = nullptr;
  size_t pf_rows = 0;
  int* fw_lengths = nullptr;   // [max_rows] positions of zn_op_backbone_forward's rows
  int* row_len = nullptr;      // [max_rows] valid positions per row of a right-padded prefill (zn_prefill_rows)
  std::vector<int> row_len_host;   // source of the copy into row_len (kept until the next zn_gen_begin has drained the stream)
  bf16_t* qkv_tmp = nullptr;   // [rows][(H + 2 Hkv) hd]: in_proj output of an attention layer whose RoPE / bias form the fused epilogue does not cover
  int prefill_mode = 1;     // 1 = batched (MFMA GEMMs + tiled attention), 0 = position by position through the decode kernels
  int lcap = 0;
  GenState* st = nullptr;
  int *remaining = nullptr, *stopping = nullptr;
  zn_row_params* row_tab = nullptr;   // [max_rows] per-utterance settings of this generation (zn_gen_set_rows)
  int* prefix_shift = nullptr;        // [max_rows] column shift per utterance of this generation (zn_gen_set_prefix_rows: <= 0; zn_gen_admit: either sign)
  // slotted session (zn_gen_open_slots): requests join the running generation slot by slot
  int* step0 = nullptr;               // [max_rows] device: session step at which slot b's request was admitted, -1 = idle
  void* adm_cache = nullptr;          // scratch cache of an admission's prefill: n_layer buffers of adm_layer_bytes
  size_t adm_layer_bytes = 0;
  int adm_cap_S = 0;                  // positions per row the scratch cache holds (max_rows rows)
  AdmitLayer* adm_layers = nullptr;   // device table [n_layer] (scratch buffer, session buffer, kind) of admit_rows_kernel
  std::vector<const void*> adm_caches;
  char* adm_stage = nullptr;          // pinned: an admission's slots, prefixes, remaining steps, row lengths ([max_rows] ints each) and parameter entries
  char* adm_dev = nullptr;            // its device copy
  hipEvent_t adm_event = nullptr;     // the copy of adm_stage has been consumed
  bool adm_pending = false;
  int* done_host = nullptr;  // pinned: [0..3] synchronous stop check, [4..7] asynchronous one
  hipEvent_t stop_event = nullptr;
  GenHost gen;                      // this generation's host record (zn_gen_state.h): zn_gen_begin starts it afresh
  int force_eos_step = -1;
  float eos_bias = 0.f;
  int tune[ZN_TUNE_NKEYS] = {};     // settings of zn_debug_tune by enum zn_tune_key (include/zonos_hip.h); defaults: zn_create.  0 = never set
  int pending_hook = 0;             // zn_debug_tune(ZN_TUNE_HOOK, v): the one-shot test hook the next zn_gen_begin consumes (enum zn_tune_hook)
  const int* tok_override = nullptr;
  int tok_override_calls = 0;
  hipStream_t cap_stream = nullptr;
  // captured decode steps, one slot per launch shape and run length (graph_slot_for).  A slot's graph is captured once per generation and
  // kept to its end: no graph is destroyed while launches of it may still be queued.
#define ZN_NGRAPHS (8 + 2 * (ZN_SK_KB_MAXNB + 1))
  hipGraphExec_t graph_exec[ZN_NGRAPHS] = {};
  hipGraph_t graph[ZN_NGRAPHS] = {};
  bool graph_tried[ZN_NGRAPHS] = {};
  StepPlan last_plan;        // of the decode steps enqueued last (zn_decode_path_detail)
  std::string err;
};

#define ZN_FAIL(h, code, ...)                                   \
  do {                                                          \
    char _b[1024]; snprintf(_b, sizeof _b, __VA_ARGS__);         \
    if (h) (h)->err = _b; else g_create_err = _b;               \
    return (code);                                              \
  } while (0)
#define HIPCHK(h, call)                                                                       \
  do {                                                                                        \
    hipError_t _e = (call);                                                                   \
    if (_e != hipSuccess) ZN_FAIL(h, ZN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)
// A check of zn_gen_state.h: its code and message are the call's.
#define ZN_GEN_CHECK(h, check)                                  \
  do {                                                          \
    const GenErr _g = (check);                                  \
    if (_g.code) ZN_FAIL(h, _g.code, "%s", _g.msg);             \
  } while (0)

extern "C" int zn_abi_version(void) { return ZN_ABI_VERSION; }

extern "C" const char* zn_last_error(zn_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" size_t zn_kv_bytes_per_layer(const zn_config* c, int32_t rows, int32_t max_len) {
  if (!c || c->n_heads <= 0) return 0;
  const size_t hd = (size_t)c->d_model / c->n_heads;
  return (size_t)rows * max_len * 2 * c->n_heads_kv * hd * 2;
}

extern "C" size_t zn_mamba_state_bytes_per_layer(const zn_config* c, int32_t rows, size_t* conv_bytes) {
  if (conv_bytes) *conv_bytes = 0;
  if (!c || c->arch != 1 || c->m_headdim <= 0 || rows < 0) return 0;
  const size_t conv_dim = (size_t)c->m_d_inner + 2 * (size_t)c->m_ngroups * c->m_d_state;
  const size_t cb = (size_t)rows * conv_dim * c->m_d_conv * 2;
  if (conv_bytes) *conv_bytes = cb;
  return cb + (size_t)rows * c->m_d_inner * c->m_d_state * 2;   // nheads * headdim = d_inner
}

static void free_graph(zn_handle h) {
  for (int k = 0; k < ZN_NGRAPHS; ++k) {
    if (h->graph_exec[k]) { (void)hipGraphExecDestroy(h->graph_exec[k]); h->graph_exec[k] = nullptr; }
    if (h->graph[k]) { (void)hipGraphDestroy(h->graph[k]); h->graph[k] = nullptr; }
    h->graph_tried[k] = false;
  }
}

// The persistent kernels' hand-offs wait on EVERY workgroup of their grid, one per CU: two such launches on one device at the same time
// (two handles generating concurrently, on any streams) could each hold part of the CUs and wait for the rest until the bounded
// waits give up.  One generation per device owns the persistent kernels; a generation that begins while another handle's is active
// on the same device runs the launches path (same results, no in-launch hand-offs).  Single-tenant per PROCESS: other processes
// sharing the GPU are outside this library's reach.
static std::mutex g_tenant_mu;
static const void* g_tenant[64] = {};
extern "C" int zn_tenant_try_claim(int32_t device, const void* owner) {
  if (device < 0 || device >= 64 || !owner) return 0;
  std::lock_guard<std::mutex> lk(g_tenant_mu);
  if (g_tenant[device] && g_tenant[device] != owner) return 0;
  g_tenant[device] = owner;
  return 1;
}
extern "C" int zn_tenant_release(int32_t device, const void* owner) {
  if (device < 0 || device >= 64) return 0;
  std::lock_guard<std::mutex> lk(g_tenant_mu);
  if (g_tenant[device] != owner) return 0;
  g_tenant[device] = nullptr;
  return 1;
}
// While ANY thread of the process captures a stream (thread-local capture mode included) HIP refuses hipMemcpy / hipMemset on the null stream (hipErrorStreamCaptureImplicit): a handle
// holds this lock from hipStreamBeginCapture to hipStreamEndCapture, and each such call that another handle's thread may make beside that generation holds it for the call alone.
static std::mutex g_capture_mu;
#define ZN_NOT_IN_CAPTURE(call) [&] { std::lock_guard<std::mutex> lk(g_capture_mu); return (call); }()

extern "C" int zn_destroy(zn_handle h) {
  if (!h) return ZN_OK;
  (void)zn_tenant_release(h->device, h);
  free_graph(h);
  void* ptrs[] = {h->emb_tables_dev, h->x, h->q, h->o1, h->mbuf, h->nbuf, h->logits_raw, h->last_logits, h->tok_raw, h->scores, h->cmax, h->pv_part, h->pv_tickets, h->pf_x, h->pf_n, h->pf_qkv, h->pf_a, h->pf_u, h->pf_m, h->pf_res, h->pf_zx, h->pf_xbc, h->pf_y, h->pf_g, h->qkv_tmp, h->fw_lengths, h->row_len, h->st, h->remaining, h->stopping, h->row_tab, h->prefix_shift, h->step0, h->adm_cache, h->adm_layers, h->adm_dev, h->res, h->hn, h->m_zx, h->m_xbc, h->m_y, h->m_g, h->m_vg, h->g16_part, h->g16_tickets, h->ln_part, h->ch_gy1, h->ch_gx1, h->ch_gx2, h->ch_gm, h->ch_epoch, h->ch_x2, h->x_emb, h->tail_ticket, h->ch_gqkv, h->ch_ga, h->ch_gbmax, h->ch_gpart, h->stack_layers, h->ch_diag};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (h->done_host) (void)hipHostFree(h->done_host);
  if (h->adm_stage) (void)hipHostFree(h->adm_stage);
  if (h->adm_event) (void)hipEventDestroy(h->adm_event);
  if (h->stop_event) (void)hipEventDestroy(h->stop_event);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  delete h;
  return ZN_OK;
}

// ------------------------------------------------------------------------------------------------ persistent chain
#define ZN_CH_GRID 256
#define ZN_CH_DYN_LDS (64 * 1024)     // unused dynamic LDS on top of the static 33 KB: never two workgroups on one CU
template <int NCH, int T_OUT, int T_FC1, int T_FC2, int T_IN>
static bool chain_resident(int n_cus) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chain_kernel<NCH, T_OUT, T_FC1, T_FC2, T_IN>, ZN_CH_THREADS, ZN_CH_DYN_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return per_cu >= 1 && n_cus >= ZN_CH_GRID;       // every workgroup of the grid is resident at once (the hand-offs wait on all of them)
}
// Which instantiation of chain_kernel serves this model at batch 1 (0 = none: the launches path).
static int chain_variant_for(const zn_config& c) {
  if (c.arch != 0 || !c.double_out_proj || c.d_ff != 4 * c.d_model) return 0;
  int dev = 0, n_cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  const int G = ZN_CH_GRID, hd = c.d_model / c.n_heads, nqkv = (c.n_heads + 2 * c.n_heads_kv) * hd;
  if ((c.d_model / 2) % G || c.d_ff % G || (nqkv / 2) % G || nqkv % 2) return 0;
  const int p_out = c.d_model / 2 / G, p_fc1 = c.d_ff / G, p_in = nqkv / 2 / G;
  if (p_fc1 * 2 > 64 || p_out * 2 > 64 || p_in * 2 > 64) return 0;                 // one communication-wave lane per (unit, row)
  auto fits = [&](int t_out, int t_fc1, int t_fc2, int t_in) {
    return p_out <= ZN_CH_CWAVES * t_out && p_fc1 <= ZN_CH_CWAVES * t_fc1 && p_out <= (ZN_CH_CWAVES / 4) * t_fc2 && p_in <= ZN_CH_CWAVES * t_in;
  };
  // the last block's launch ends with the fused heads (T_IN = 5 / 3 tiles per wave) when they fit its lanes, else after fc2 (T_IN = 0)
  if (c.d_model == 2048 && fits(1, 8, 4, 2) && chain_resident<4, 1, 8, 4, 2>(n_cus) && chain_resident<4, 1, 8, 4, 0>(n_cus) && chain_resident<4, 1, 8, 4, 5>(n_cus)) return 1;
  if (c.d_model == 512 && fits(1, 2, 1, 1) && chain_resident<1, 1, 2, 1, 1>(n_cus) && chain_resident<1, 1, 2, 1, 0>(n_cus) && chain_resident<1, 1, 2, 1, 5>(n_cus)) return 2;
  return 0;
}

extern "C" int zn_create(const zn_config* cfg, const zn_weights* w, int32_t max_rows, zn_handle* out) {
  if (!cfg || !w || !out) ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "zn_create: null argument");
  *out = nullptr;
  const zn_config& c = *cfg;
  if (c.d_model <= 0 || c.n_layer <= 0 || c.n_heads <= 0 || c.n_heads_kv <= 0 || c.d_ff <= 0 || c.n_codebooks <= 0)
    ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "zn_create: non-positive dimension");
  if (c.d_model % c.n_heads || c.n_heads % c.n_heads_kv) ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "zn_create: heads do not divide");
  const int hd = c.d_model / c.n_heads, G = c.n_heads / c.n_heads_kv;
  if (hd != 32 && hd != 64 && hd != 128) ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "head_dim %d not in {32,64,128}", hd);
  if (G != 1 && G != 2 && G != 4 && G != 8) ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "GQA group %d not in {1,2,4,8}", G);
  if (c.d_model % 8 || c.d_ff % 8 || c.d_model > 4096) ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "d_model/d_ff must be multiples of 8, d_model <= 4096");
  if (c.n_codebooks > ZN_FRAME_MAXQ) ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "n_codebooks > %d", ZN_FRAME_MAXQ);
  if (c.vocab_head > ZN_SAMPLE_MAXV) ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "vocab_head > %d", ZN_SAMPLE_MAXV);
  if (max_rows < 2 || max_rows % 2) ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "max_rows must be even and >= 2");
  if (c.arch != 0 && c.arch != 1) ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "zn_create: arch must be 0 (transformer) or 1 (hybrid)");
  if (c.arch == 1) {
    if (c.m_headdim != 64 || (c.m_d_state != 64 && c.m_d_state != 128) || c.m_d_conv != 4)
      ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "Mamba2: headdim %d / d_state %d / d_conv %d not in {64} x {64,128} x {4}", c.m_headdim, c.m_d_state, c.m_d_conv);
    if (c.m_d_inner <= 0 || c.m_d_inner % 64 || c.m_ngroups < 1 || (c.m_d_inner / 64) % c.m_ngroups || (c.m_d_inner / c.m_ngroups) % 8 ||
        c.m_d_inner / c.m_ngroups > 8192)
      ZN_FAIL((zn_handle) nullptr, ZN_ERR_UNSUPPORTED, "Mamba2: d_inner %d / ngroups %d not supported", c.m_d_inner, c.m_ngroups);
  }
  if (c.rope_mode < 0 || c.rope_mode > 2) ZN_FAIL((zn_handle) nullptr, ZN_ERR_ARG, "zn_create: rope_mode must be 0, 1 or 2");
  zn_handle h = new zn_handle_s();
  h->cfg = c; h->max_rows = max_rows; h->hd = hd; h->G = G;
  h->tune[ZN_TUNE_WG_IN_PROJ] = 256; h->tune[ZN_TUNE_WG_OUT_PROJ] = 512; h->tune[ZN_TUNE_WG_FC1] = 512; h->tune[ZN_TUNE_WG_FC2] = 1024; h->tune[ZN_TUNE_WG_HEADS] = 512;
  h->tune[ZN_TUNE_ATTN_FUSED_MAX_KEYS] = 512; h->tune[ZN_TUNE_GRAPH_RUNS] = 2; h->tune[ZN_TUNE_SMALL_M_LDS] = 2;      // every other key: unset
  if (hipGetDevice(&h->device) != hipSuccess) { (void)hipGetLastError(); h->device = 0; }
  if (c.arch == 1) {
    h->m_nheads = c.m_d_inner / c.m_headdim;
    h->m_conv_dim = c.m_d_inner + 2 * c.m_ngroups * c.m_d_state;
    h->m_d_in_proj = 2 * c.m_d_inner + 2 * c.m_ngroups * c.m_d_state + h->m_nheads;
  }
  if (const char* e = getenv("ZN_PREFILL_MODE")) h->prefill_mode = atoi(e);
  h->layers.assign(w->layers, w->layers + c.n_layer);
  h->mlp_fp8.assign(c.n_layer, zn_handle_s::MlpFp8{});
  h->mamba_fp8.assign(c.n_layer, zn_handle_s::MambaFp8{});
  h->heads = w->heads; h->norm_f_w = w->norm_f_w; h->norm_f_b = w->norm_f_b; h->rope = w->rope_table;
#define ZC(call) do { hipError_t _e = ZN_NOT_IN_CAPTURE(call); if (_e != hipSuccess) { g_create_err = std::string(#call) + ": " + hipGetErrorString(_e); zn_destroy(h); return ZN_ERR_HIP; } } while (0)
  ZC(hipMalloc(&h->emb_tables_dev, sizeof(void*) * c.n_codebooks));
  if (w->embeddings) ZC(hipMemcpy(h->emb_tables_dev, w->embeddings, sizeof(void*) * c.n_codebooks, hipMemcpyHostToDevice));
  h->has_io = (w->embeddings != nullptr && w->heads != nullptr);
  const size_t R = max_rows;
  ZC(hipMalloc(&h->x, R * c.d_model * 2));
  ZC(hipMalloc(&h->q, R * c.d_model * 2));
  ZC(hipMalloc(&h->o1, R * c.d_model * 2));
  ZC(hipMalloc(&h->mbuf, R * c.d_ff * 2));
  ZC(hipMalloc(&h->nbuf, R * c.d_model * 2));
  ZC(hipMalloc(&h->logits_raw, R * c.n_codebooks * c.vocab_head * sizeof(float)));
  // per-utterance buffers: up to R utterances (one row each) when generating without guidance, R / 2 with it
  ZC(hipMalloc(&h->last_logits, R * c.n_codebooks * c.vocab_head * sizeof(float)));
  ZC(hipMalloc(&h->tok_raw, R * c.n_codebooks * sizeof(int)));
  ZC(hipMalloc(&h->fw_lengths, R * sizeof(int)));
  ZC(hipMalloc(&h->row_len, R * sizeof(int)));
  ZC(hipMalloc(&h->st, sizeof(GenState)));
  ZC(hipMemset(h->st, 0, sizeof(GenState)));
  ZC(hipMalloc(&h->remaining, R * sizeof(int)));
  ZC(hipMalloc(&h->stopping, R * sizeof(int)));
  ZC(hipMalloc(&h->row_tab, R * sizeof(zn_row_params)));
  ZC(hipMalloc(&h->prefix_shift, R * sizeof(int)));
  ZC(hipHostMalloc(&h->done_host, sizeof(int) * 8));
  ZC(hipEventCreateWithFlags(&h->stop_event, hipEventDisableTiming));
  for (unsigned long long** g : {&h->ch_gy1, &h->ch_gx1, &h->ch_gx2}) {
    ZC(hipMalloc(g, R * (c.d_model / 2) * 8));
    ZC(hipMemset(*g, 0, R * (c.d_model / 2) * 8));             // tag 0 is never a launch's epoch
  }
  { const size_t nqkv = (size_t)(c.n_heads + 2 * c.n_heads_kv) * hd;
    ZC(hipMalloc(&h->ch_gqkv, R * (nqkv / 2 + 1) * 8)); ZC(hipMemset(h->ch_gqkv, 0, R * (nqkv / 2 + 1) * 8));
    ZC(hipMalloc(&h->ch_ga, R * (c.d_model / 2) * 8)); ZC(hipMemset(h->ch_ga, 0, R * (c.d_model / 2) * 8));
    { const size_t nbm = (size_t)2 * c.n_heads_kv * ZN_SK_KB_MAXNB * 4 * 8, npt = (size_t)2 * c.n_heads_kv * ZN_SK_KB_MAXNB * ZN_SK_KB_PSZ * 8;
      ZC(hipMalloc(&h->ch_gbmax, nbm)); ZC(hipMemset(h->ch_gbmax, 0, nbm));
      ZC(hipMalloc(&h->ch_gpart, npt)); ZC(hipMemset(h->ch_gpart, 0, npt)); }
    ZC(hipMalloc(&h->stack_layers, (size_t)c.n_layer * sizeof(StackLayer))); }
  ZC(hipMalloc(&h->ch_gm, R * (c.d_ff / 2 + 1) * 8));
  ZC(hipMemset(h->ch_gm, 0, R * (c.d_ff / 2 + 1) * 8));
  ZC(hipMalloc(&h->ch_epoch, 64));
  ZC(hipMalloc(&h->ch_diag, 64));
  ZC(hipMemset(h->ch_diag, 0, 64));
  { const unsigned one = 1; ZC(hipMemcpy(h->ch_epoch, &one, sizeof one, hipMemcpyHostToDevice)); }
  ZC(hipMalloc(&h->ch_x2, R * c.d_model * 2));
  h->ch_variant = chain_variant_for(c);
  if (const char* e = getenv("ZN_CHAIN")) if (atoi(e) == 0) h->tune[ZN_TUNE_PERSISTENT] = 2;
  if (const char* e = getenv("ZN_STACK")) if (atoi(e) == 0) h->tune[ZN_TUNE_WHOLE_STEP] = 2;
  {   // split-K partial tiles + tickets of the small-M projections (batches of 3..8 utterances; short-prompt prefill at any batch)
    ZC(hipMalloc(&h->x_emb, R * c.d_model * 2));
    ZC(hipMalloc(&h->tail_ticket, sizeof(int)));
    ZC(hipMemset(h->tail_ticket, 0, sizeof(int)));
    ZC(hipMalloc(&h->g16_part, ZN_G16_PART_BYTES));
    ZC(hipMalloc(&h->g16_tickets, ZN_G16_MAX_GROUPS * sizeof(int)));
    ZC(hipMemset(h->g16_tickets, 0, ZN_G16_MAX_GROUPS * sizeof(int)));
    h->g16_part_bytes = ZN_G16_PART_BYTES;
    ZC(hipMalloc(&h->ln_part, R * ZN_G16_LNT * 2 * sizeof(float)));
  }
  if (c.arch == 1) {
    ZC(hipMalloc(&h->res, R * c.d_model * 4));     // bf16, or fp32 with residual_in_fp32
    ZC(hipMalloc(&h->qkv_tmp, R * (size_t)(c.n_heads + 2 * c.n_heads_kv) * hd * 2));
    ZC(hipMalloc(&h->hn, R * c.d_model * 2));
    ZC(hipMalloc(&h->m_zx, R * h->m_d_in_proj * 2));
    ZC(hipMalloc(&h->m_xbc, R * h->m_conv_dim * 2));
    ZC(hipMalloc(&h->m_y, R * c.m_d_inner * 2));
    ZC(hipMalloc(&h->m_vg, R * c.m_d_inner * sizeof(float)));
    ZC(hipMalloc(&h->m_g, R * c.m_d_inner * 2));
  }
#undef ZC
  *out = h;
  return ZN_OK;
}

// ------------------------------------------------------------------------------------------------ launches
template <int R, int NCH, int KS, int PRO, int EPI>
static void launch_gemv_t(const GemvArgs& a, int blocks, bool full, hipStream_t s) {
  if (full) hipLaunchKernelGGL((gemv_kernel<R, NCH, KS, PRO, EPI, true>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemv_kernel<R, NCH, KS, PRO, EPI, false>), dim3(blocks), dim3(256), 0, s, a);
}
template <int R, int KS, int PRO, int EPI>
static int launch_gemv_nch(const GemvArgs& a, int nch, int blocks, bool full, hipStream_t s) {
  switch (nch) {
    case 1: launch_gemv_t<R, 1, KS, PRO, EPI>(a, blocks, full, s); return 0;
    case 2: launch_gemv_t<R, 2, KS, PRO, EPI>(a, blocks, full, s); return 0;
    case 4: launch_gemv_t<R, 4, KS, PRO, EPI>(a, blocks, full, s); return 0;
    case 8: launch_gemv_t<R, 8, KS, PRO, EPI>(a, blocks, full, s); return 0;
  }
  return -1;
}
template <int PRO, int EPI>
static int launch_gemv_rows(const GemvArgs& a, int rgroup, int ks, int nch, int blocks, bool full, hipStream_t s) {
  if (ks == 1) {
    if (rgroup <= 2) return launch_gemv_nch<2, 1, PRO, EPI>(a, nch, blocks, full && rgroup == 2, s);
    return launch_gemv_nch<4, 1, PRO, EPI>(a, nch, blocks, full && rgroup == 4, s);
  }
  if constexpr (PRO == PRO_NONE || PRO == PRO_GATED) {
    if (rgroup <= 2) return launch_gemv_nch<2, 4, PRO, EPI>(a, nch, blocks, full && rgroup == 2, s);
    return launch_gemv_nch<4, 4, PRO, EPI>(a, nch, blocks, full && rgroup == 4, s);
  }
  return -1;
}
// the same launch reading the FP8 stream (p.w8 on a GEMV plan; gemv8_kernel): the instantiations of lin_has_w8v - one (KS, NCH) per (PRO, EPI) - each for
// R = 2 and 4, FULL, and one or two units requested ahead (depth: ZN_TUNE_FP8_SMALL_ROWS = 2 / 3)
template <int R, int NCH, int KS, int PRO, int EPI>
static void launch_gemv8_t(const GemvArgs& a, int blocks, bool full, int depth, hipStream_t s) {
  if (depth == 1) {
    if (full) hipLaunchKernelGGL((gemv8_kernel<R, NCH, KS, PRO, EPI, true, 1>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gemv8_kernel<R, NCH, KS, PRO, EPI, false, 1>), dim3(blocks), dim3(256), 0, s, a);
  } else {
    if (full) hipLaunchKernelGGL((gemv8_kernel<R, NCH, KS, PRO, EPI, true, 2>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gemv8_kernel<R, NCH, KS, PRO, EPI, false, 2>), dim3(blocks), dim3(256), 0, s, a);
  }
}
template <int PRO, int EPI>
static int launch_gemv8_rows(const GemvArgs& a, int rgroup, int ks, int nch, int blocks, bool full, int depth, hipStream_t s) {
  constexpr int KS = (EPI == EPI_SILU || EPI == EPI_MAMBA) ? 1 : 4, NCH = EPI == EPI_STORE ? 2 : 4;
  if constexpr (lin_has_w8v(PRO, EPI, KS, NCH)) {
    if (ks != KS || nch != NCH) return -1;
    if (rgroup <= 2) launch_gemv8_t<2, NCH, KS, PRO, EPI>(a, blocks, full && rgroup == 2, depth, s);
    else launch_gemv8_t<4, NCH, KS, PRO, EPI>(a, blocks, full && rgroup == 4, depth, s);
    return 0;
  }
  return -1;
}

static void launch_gemm(const bf16_t* A, int lda, const bf16_t* W, bf16_t* out, int ldo, const bf16_t* resid, int M, int N, int K, hipStream_t s,
                        const bf16_t* bias = nullptr) {
  GemmArgs g{A, W, out, resid, M, N, K, lda, ldo, bias};
  dim3 grid((N + 127) / 128, (M + 127) / 128);
  if (M >= 256 && K % ZN_PG_KC == 0 && lda % 8 == 0) {   // long prompts: LDS-staged panels (coalesced row pieces)
    if (resid) hipLaunchKernelGGL((gemm_bf16s_kernel<1>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16s_kernel<0>), grid, dim3(256), 0, s, g);
    return;
  }
  if (resid) hipLaunchKernelGGL((gemm_bf16_kernel<1>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm_bf16_kernel<0>), grid, dim3(256), 0, s, g);
}
template <int NW, int EPI>
static void launch_gemm16_t(const GemvArgs& g, int blocks, bool tile8, hipStream_t s) {
  if constexpr (lin_has_tile8(EPI)) if (tile8) { hipLaunchKernelGGL((gemm16_kernel<NW, EPI, 8>), dim3(blocks), dim3(NW * 64), 0, s, g); return; }
  hipLaunchKernelGGL((gemm16_kernel<NW, EPI>), dim3(blocks), dim3(NW * 64), 0, s, g);
}
template <int EPI, bool LNP>
static void launch_gemm16s_t(const GemvArgs& g, const LinearPlan& p, hipStream_t s) {
  if (p.nwv == 4) hipLaunchKernelGGL((gemm16s_kernel<EPI, 4, LNP>), dim3(p.groups, p.ksplit), dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm16s_kernel<EPI, 2, LNP>), dim3(p.groups, p.ksplit), dim3(128), 0, s, g);
}
// the same launch reading the FP8 stream (p.w8): fc1 <EPI_SILU, ., {false, true}> and fc2 <EPI_RESID, ., false> only (lin_has_w8)
template <int EPI, bool LNP>
static void launch_gemm16s_w8_t(const GemvArgs& g, const LinearPlan& p, hipStream_t s) {
  if (p.nwv == 4) hipLaunchKernelGGL((gemm16s_kernel<EPI, 4 | ZN_G16S_W8, LNP>), dim3(p.groups, p.ksplit), dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm16s_kernel<EPI, 2 | ZN_G16S_W8, LNP>), dim3(p.groups, p.ksplit), dim3(128), 0, s, g);
}

// gemm16w_kernel over nr = 17..64 rows of a plan with row_tiles > 1: RB = ceil(nr / 16) activation blocks per staged weight chunk
template <int EPI, bool W8>
static void launch_gemm16w_t(const GemvArgs& g, const LinearPlan& p, int nr, hipStream_t s) {
  const dim3 grid(p.groups_wide, p.ksplit), block(256);
  const int rb = (nr + 15) / 16;
  if (rb == 2) hipLaunchKernelGGL((gemm16w_kernel<EPI, W8, 2>), grid, block, 0, s, g);
  else if (rb == 3) hipLaunchKernelGGL((gemm16w_kernel<EPI, W8, 3>), grid, block, 0, s, g);
  else hipLaunchKernelGGL((gemm16w_kernel<EPI, W8, 4>), grid, block, 0, s, g);
}

// Every decision about a linear of 1 .. 64 rows is plan_linear's (zn_linear_plan.h); what it may depend on:
// step: the plan of a generation step (wide from 17 rows on unless ZN_TUNE_WIDE_ROWS = 1); else of a per-op entry point (wide only under = 2).
static LinearEnv linear_env(zn_handle h, bool step = true) {
  LinearEnv e;
  e.wide_rows = h->tune[ZN_TUNE_WIDE_ROWS] == 2 || (step && h->tune[ZN_TUNE_WIDE_ROWS] != 1);
  // the Mamba2 in_proj of a generation step (mamba_mixer, zn_op_mamba_step included): ZN_TUNE_WIDE_HYBRID, unset = the form plan_wide picks for the row count
  e.wide_hybrid = !step ? 0 : h->tune[ZN_TUNE_WIDE_HYBRID] ? h->tune[ZN_TUNE_WIDE_HYBRID] : 4;
  e.small_m_lds = h->tune[ZN_TUNE_SMALL_M_LDS]; e.no_split_small_m = h->tune[ZN_TUNE_NO_SPLIT_SMALL_M]; e.gemm16k_max_tiles = h->tune[ZN_TUNE_GEMM16K_MAX_TILES];
  e.fc1_ln_launch = h->tune[ZN_TUNE_FC1_LN_LAUNCH]; e.no_prefill_gemm16k = h->tune[ZN_TUNE_NO_PREFILL_GEMM16K];
  e.g16_part_bytes = h->g16_part_bytes; e.has_g16_part = h->g16_part != nullptr; e.has_ln_part = h->ln_part != nullptr;
  return e;
}
// g serves the row group [r0, r0 + nr) of the rows it described: every per-row pointer moves there.
static void advance_rows(GemvArgs& g, int r0, int nr, int out_cols) {
  g.nrows = nr;
  if (g.x) g.x += (size_t)r0 * g.K;
  if (g.gv) g.gv += (size_t)r0 * g.K;
  if (g.out) g.out += (size_t)r0 * out_cols;
  if (g.resid) g.resid += (size_t)r0 * g.N;
  if (g.out_f32) g.out_f32 += (size_t)r0 * g.N;
  if (g.lengths) g.lengths += r0;
  if (g.q_out) g.q_out += (size_t)r0 * g.n_heads * g.hd;
  if (g.kv) g.kv += (size_t)r0 * g.max_len * 2 * g.n_heads_kv * g.hd;
  if (g.kv8) g.kv8 += (size_t)r0 * g.max_len * 2 * g.n_heads_kv * g.hd;
  if (g.conv_state) { g.conv_state += (size_t)r0 * g.conv_dim * 4; g.xbc += (size_t)r0 * g.conv_dim; }
  if (g.ln_part_out) g.ln_part_out += (size_t)r0 * ZN_G16_LNT * 2;
  if (g.ln_part_in) g.ln_part_in += (size_t)r0 * ZN_G16_LNT * 2;
}
// Launches what the plan says over `rows` activation rows, group by group of rows_per_launch (weights are re-streamed per group: 16 rows, or 64 under the wide
// plan, whose last group follows its own size: 16 rows or fewer are the 16-row plan's launch): the template switches, and nothing that decides.
template <int PRO, int EPI>
static int launch_linear(zn_handle h, const LinearPlan& p, GemvArgs a, int rows, hipStream_t s) {
  if (p.err) ZN_FAIL(h, p.err, "%s", p.msg);
  if (!linear_plan_launchable(p, PRO, EPI)) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "linear: no kernel %d for prologue %d / epilogue %d (ks=%d nch=%d)", (int)p.kernel, PRO, EPI, p.ks, p.nch);
  if ((p.reads_ln_stats && !a.ln_part_in) || (p.writes_ln_stats && !a.ln_part_out)) ZN_FAIL(h, ZN_ERR_STATE, "linear: the plan hands over LayerNorm statistics, the call has no buffer for them");
  if (p.w8 && (!a.W8q || !a.W8exp)) ZN_FAIL(h, ZN_ERR_STATE, "linear: the plan reads an FP8 weight stream, the call has none");
  if (!p.writes_ln_stats) a.ln_part_out = nullptr;
  a.units = p.units; a.upw = p.upw;
  if (p.ksplit) { a.part = h->g16_part; a.tickets = h->g16_tickets; a.ksplit = p.ksplit; }
  const int per = p.rows_per_launch ? p.rows_per_launch : rows;
  for (int r0 = 0; r0 < rows; r0 += per) {
    GemvArgs g = a;
    const int nr = rows - r0 < per ? rows - r0 : per;
    advance_rows(g, r0, nr, EPI == EPI_SILU ? a.N / 2 : a.N);
    if (p.ln_launch) {
      hipLaunchKernelGGL(layernorm_kernel, dim3(nr), dim3(64), 0, s, g.x, a.ln_w, a.ln_b, h->nbuf, a.K, a.eps);
      g.x = h->nbuf;
    }
    switch (p.kernel) {
      case LinearPlan::GEMV:
        if (p.w8) {      // (launchable: lin_has_w8v holds this (PRO, EPI, ks, nch))
          (void)launch_gemv8_rows<PRO, EPI>(g, nr, p.ks, p.nch, p.blocks, p.full, h->tune[ZN_TUNE_FP8_SMALL_ROWS] == 3 ? 2 : 1, s);
          break;
        }
        (void)launch_gemv_rows<PRO, EPI>(g, nr, p.ks, p.nch, p.blocks, p.full, s);      // (its instantiations: linear_plan_launchable)
        break;
      case LinearPlan::GEMM16:
        if constexpr (lin_has_gemm16(PRO)) {
          if (p.nw == 16) launch_gemm16_t<16, EPI>(g, p.blocks, p.tile8, s);
          else if (p.nw == 8) launch_gemm16_t<8, EPI>(g, p.blocks, p.tile8, s);
          else launch_gemm16_t<4, EPI>(g, p.blocks, p.tile8, s);
        }
        break;
      case LinearPlan::GEMM16S:
        if constexpr (lin_has_wide16s(PRO, EPI)) if (p.row_tiles > 1 && nr > 16) {
          if constexpr (lin_has_lnp(PRO, EPI)) if (p.lnp) {      // LayerNorm from the handed-over statistics, in the 16-row plan's order, as one launch
            if (p.nwv == 4) hipLaunchKernelGGL((ln_from_stats_kernel<16>), dim3(nr), dim3(64), 0, s, g.x, g.ln_part_in, a.ln_w, a.ln_b, h->nbuf, a.eps);
            else hipLaunchKernelGGL((ln_from_stats_kernel<8>), dim3(nr), dim3(64), 0, s, g.x, g.ln_part_in, a.ln_w, a.ln_b, h->nbuf, a.eps);
            g.x = h->nbuf;
          }
          if (p.w8) launch_gemm16w_t<EPI, true>(g, p, nr, s);
          else launch_gemm16w_t<EPI, false>(g, p, nr, s);
          break;
        }
        if constexpr (lin_has_w8(PRO, EPI)) if (p.w8) {
          if constexpr (lin_has_lnp(PRO, EPI)) if (p.lnp) { launch_gemm16s_w8_t<EPI, true>(g, p, s); break; }
          launch_gemm16s_w8_t<EPI, false>(g, p, s);
          break;
        }
        if constexpr (lin_has_lnp(PRO, EPI)) if (p.lnp) { launch_gemm16s_t<EPI, true>(g, p, s); break; }
        if constexpr (lin_has_gemm16(PRO)) launch_gemm16s_t<EPI, false>(g, p, s);
        break;
      case LinearPlan::GEMM16K:   // decode: one 16-row group per launch (the wide plan: up to four); prefill: ceil(rows / 16) of them
        if constexpr (lin_has_gemm16k(PRO, EPI)) {
          const dim3 grid((a.N + 15) / 16, (nr + 15) / 16), block(ZN_G16K_NKW * 64);
          // the same launches reading the FP8 stream (p.w8: the Mamba2 in_proj at nch 2, out_proj at nch 4; lin_has_w8k)
          if constexpr (lin_has_w8k(PRO, EPI, EPI == EPI_MAMBA ? 2 : 4)) if (p.w8) {
            if constexpr (EPI == EPI_MAMBA) {
              if (p.row_loop && nr > 16) hipLaunchKernelGGL((gemm16k8_rows_kernel<2>), dim3(grid.x), block, 0, s, g);
              else hipLaunchKernelGGL((gemm16k8_kernel<EPI_MAMBA, 2>), grid, block, 0, s, g);
            } else hipLaunchKernelGGL((gemm16k8_kernel<EPI_STORE, 4>), grid, block, 0, s, g);
            break;
          }
          if constexpr (lin_has_gemm16k_rows(PRO, EPI, 2)) if (p.row_loop && nr > 16) {    // the row-tile loop: one workgroup per weight tile walks the row tiles
            hipLaunchKernelGGL((gemm16k_rows_kernel<2>), dim3(grid.x), block, 0, s, g);
            break;
          }
          if constexpr (lin_has_gemm16k_ln(PRO, 2)) if (p.ln_pro) { hipLaunchKernelGGL((gemm16k_kernel<EPI, 2, PRO_LN>), grid, block, 0, s, g); break; }
          if (p.nch == 2) hipLaunchKernelGGL((gemm16k_kernel<EPI, 2, PRO_NONE>), grid, block, 0, s, g);
          else hipLaunchKernelGGL((gemm16k_kernel<EPI, 4, PRO_NONE>), grid, block, 0, s, g);
        }
        break;
      case LinearPlan::GEMM64S:
        if constexpr (lin_has_prefill(PRO, EPI)) hipLaunchKernelGGL((gemm64s_kernel<EPI>), dim3(p.groups, p.ksplit), dim3(256), 0, s, g);
        break;
      case LinearPlan::GEMM_TILED:
        if constexpr (lin_has_prefill(PRO, EPI) && EPI == EPI_SILU) {
          launch_gemm(g.x, a.K, a.W, h->pf_u, a.N, nullptr, nr, a.N, a.K, s);
          hipLaunchKernelGGL(silu_mul_rows_kernel, dim3(nr), dim3(256), 0, s, h->pf_u, g.out, a.N / 2);
        } else if constexpr (lin_has_prefill(PRO, EPI)) launch_gemm(g.x, a.K, a.W, g.out, a.N, g.resid, nr, a.N, a.K, s);
        break;
    }
  }
  return ZN_OK;
}
template <int PRO, int EPI>
static int run_gemv(zn_handle h, const GemvArgs& a, int rows, int target_blocks, hipStream_t s, bool step = true) {
  return launch_linear<PRO, EPI>(h, plan_linear(linear_env(h, step), PRO, EPI, rows, a.N, a.K, target_blocks, false, false, false), a, rows, s);
}
// A projection over the M rows of a batched prefill (x normalised by the caller): the small-M kernels up to 64 rows, else the tiled GEMM.
// with_gemm16k = false: fc1 / fc2, which were measured on the 64-row kernel only.  EPI_ROPE_KV (in_proj): *rope_done tells whether split, RoPE and
// the KV append ran in the epilogue (q compact [M][Hq * hd] in q_out) or rope_kv_rows_kernel still has to follow on out [M][N].
template <int EPI>
static int prefill_linear(zn_handle h, const GemvArgs& g, int M, hipStream_t s, bool with_gemm16k = true, bool* rope_done = nullptr) {
  LinearEnv e = linear_env(h);
  if (!with_gemm16k) e.no_prefill_gemm16k = 2;
  const LinearPlan p = plan_linear(e, PRO_NONE, EPI, M, g.N, g.K, 0, true, false, false);
  if constexpr (EPI == EPI_ROPE_KV) {
    if (!(*rope_done = p.epi == EPI_ROPE_KV)) return launch_linear<PRO_NONE, EPI_STORE>(h, p, g, M, s);
  }
  return launch_linear<PRO_NONE, EPI>(h, p, g, M, s);
}

// ONE arithmetic for the decode attention on every path (launches, per-block chain, whole-step kernels): scores on the matrix cores in
// one summation order, P.V per 512-key block (the reference's block size) on the matrix cores in one order, the blocks' unnormalised partials
// combined by the reference's recurrence acc = acc * f_j + pv_j in block order (attn_block_probs / attn_block_pv, shared by the launches and
// by the attention role of zn_step_kernel.h).  The fused launch (scores + pass 2 + normalisation in one launch) serves contexts of one block:
// ZN_TUNE_ATTN_FUSED_MAX_KEYS may lower that limit (tests), never raise it.
#define ZN_AFUSED_LIMIT 512
// Launch shape of the decode attention for contexts of at most keys_upper_bound keys: 1 = the one-launch shape (one block), 0 = scores launch +
// block launch.
static bool attn_split_cols(zn_handle h, int rows) { return h->tune[ZN_TUNE_ATTN_SPLIT_COLS] == 2 || (h->tune[ZN_TUNE_ATTN_SPLIT_COLS] != 1 && rows > 4); }
static int attn_fused_for(zn_handle h, int keys_upper_bound) {
  const int lim = h->tune[ZN_TUNE_ATTN_FUSED_MAX_KEYS] < ZN_AFUSED_LIMIT ? h->tune[ZN_TUNE_ATTN_FUSED_MAX_KEYS] : ZN_AFUSED_LIMIT;
  return keys_upper_bound <= lim ? 1 : 0;
}

#ifndef ZN_ATTN_DSF
#define ZN_ATTN_DSF 4
#endif
#ifndef ZN_ATTN_DSS
#define ZN_ATTN_DSS 2
#endif
// FP8: the same launches reading the code cache a.kv8 (zn_attn_fp8_kernels.h) - the form the caller's plan chose by leaving a code cache in the arguments (run_attention).
#define ZN_ATTN_LAUNCH(FP8, BF16, grid_, block_) do { if (a.kv8) hipLaunchKernelGGL(FP8, grid_, block_, 0, s, a); else hipLaunchKernelGGL(BF16, grid_, block_, 0, s, a); } while (0)
template <int HD>
static int launch_attn_g(const AttnArgs& a, int G, dim3 grid, int fused, bool split_cols, hipStream_t s) {
  constexpr int DS = HD == 128 ? ZN_ATTN_DSS : 1;       // value-column parts per (row, kv head[, block]) when split_cols (attn_block_kernel)
  constexpr int DSF = HD == 128 ? ZN_ATTN_DSF : 1;      // ... of the one-launch shape
  switch (G) {
#define ZN_ATTN_CASE(GG) case GG: \
    if (fused) { \
      if (split_cols && DSF > 1) ZN_ATTN_LAUNCH((attn_block_fp8_kernel<HD, GG, true, DSF>), (attn_block_kernel<HD, GG, true, DSF>), dim3(grid.y * grid.z * DSF), dim3(512)); \
      else ZN_ATTN_LAUNCH((attn_block_fp8_kernel<HD, GG, true>), (attn_block_kernel<HD, GG, true>), dim3(grid.y * grid.z), dim3(512)); \
      return 0; \
    } \
    ZN_ATTN_LAUNCH((attn_scores_fp8_kernel<HD, GG>), (attn_scores_kernel<HD, GG>), grid, dim3(256)); \
    if (split_cols && DS > 1) ZN_ATTN_LAUNCH((attn_block_fp8_kernel<HD, GG, false, DS>), (attn_block_kernel<HD, GG, false, DS>), dim3(grid.y * DS, grid.z * a.nbcap), dim3(512)); \
    else ZN_ATTN_LAUNCH((attn_block_fp8_kernel<HD, GG, false>), (attn_block_kernel<HD, GG, false>), dim3(grid.y, grid.z * a.nbcap), dim3(512)); \
    return 0;
    ZN_ATTN_CASE(1) ZN_ATTN_CASE(2) ZN_ATTN_CASE(4) ZN_ATTN_CASE(8)
#undef ZN_ATTN_CASE
  }
  return -1;
}
#undef ZN_ATTN_LAUNCH

// ---- FP8 KV cache (zn_set_kv_fp8).  In effect: a generation of 5 rows or more on a transformer handle with the mode on - always the launches path
// (the persistent kernels serve one or two rows).  Then every KV append rounds to the E4M3 grid and writes both caches.
#define ZN_KV_FP8_MIN_ROWS 5
static bool kv_fp8_rows(zn_handle h, int rows) { return h->cfg.arch == 0 && rows >= ZN_KV_FP8_MIN_ROWS; }
static bool kv_fp8_gen(zn_handle h) { return h->kv_fp8 && kv_fp8_rows(h, h->gen.rows); }
static uint8_t* kv8_of(zn_handle h, int li) { return kv_fp8_gen(h) && !h->gen.kv8_layers.empty() ? (uint8_t*)const_cast<void*>(h->gen.kv8_layers[li]) : nullptr; }
// The decode attention's side of the plan, in one place: does an attention launch over `rows` rows that has a code cache read it?  ZN_TUNE_KV_FP8 = 2: never (the bf16
// cache holds the dequantised codes: the same bits).  No row count is declined: the FP8 reads have not been measured against the bf16 reads yet (tools/kvfp8bench.py).
// codes_only: there is no bf16 cache to read instead (a codes-only generation, a per-op call without one): the key is ignored.
static bool kv_fp8_attn_reads(zn_handle h, int rows, bool codes_only = false) { return (codes_only || h->tune[ZN_TUNE_KV_FP8] != 2) && kv_fp8_rows(h, rows); }
// Codes only (zn_set_kv_fp8_only): a generation in which the FP8 KV cache is in effect on a handle with the second flag on keeps no bf16 cache - the
// appends write the codes alone, the decode and the prefill attention read them, an admission's scratch cache holds codes.
static bool kv_codes_only_rows(zn_handle h, int rows) { return h->kv_fp8 && h->kv_fp8_only && kv_fp8_rows(h, rows); }
static bool kv_codes_only_gen(zn_handle h) { return kv_codes_only_rows(h, h->gen.rows); }
static int kv_fp8_bound(zn_handle h, const char* who) {
  if (kv_fp8_gen(h) && h->gen.kv8_layers.empty()) ZN_FAIL(h, ZN_ERR_STATE, "%s: the FP8 KV cache is in effect (zn_set_kv_fp8, %d rows) and no code caches are bound (zn_gen_bind_kv_fp8)", who, h->gen.rows);
  return ZN_OK;
}

static int ensure_attn_ws(zn_handle h, int max_len) {
  const int lcap = ((max_len + 511) / 512) * 512;
  if (lcap <= h->lcap) return ZN_OK;
  free_graph(h);
  for (float** p : {&h->scores, &h->cmax, &h->pv_part}) if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (h->pv_tickets) { (void)hipFree(h->pv_tickets); h->pv_tickets = nullptr; }
  const size_t RH = (size_t)h->max_rows * h->cfg.n_heads;
  const int nc = lcap / ZN_ACHUNK;
  HIPCHK(h, hipMalloc(&h->scores, RH * lcap * sizeof(float)));
  HIPCHK(h, hipMalloc(&h->cmax, RH * nc * sizeof(float)));
  { const size_t groups = (size_t)h->max_rows * h->cfg.n_heads_kv;
    HIPCHK(h, hipMalloc(&h->pv_part, groups * (lcap / 512) * (size_t)(h->G * h->hd + 4 * h->G) * sizeof(float)));     // (up to four column parts, each with its e sums)
    HIPCHK(h, hipMalloc(&h->pv_tickets, 4 * groups * sizeof(int)));
    HIPCHK(h, ZN_NOT_IN_CAPTURE(hipMemset(h->pv_tickets, 0, 4 * groups * sizeof(int)))); }
  h->lcap = lcap;
  return ZN_OK;
}

static int run_attention(zn_handle h, const bf16_t* q, const bf16_t* kv, int max_len, const int* lengths, const int* ext, int ext_scalar,
                         bf16_t* out, int rows, int fused, hipStream_t s, unsigned long long* stamps = nullptr, const uint8_t* kv8 = nullptr) {
  const zn_config& c = h->cfg;
  if (max_len > h->lcap || rows > h->max_rows) ZN_FAIL(h, ZN_ERR_STATE, "attention workspace too small (max_len %d rows %d)", max_len, rows);
  AttnArgs a{};
  a.q = q; a.kv = kv; a.lengths = lengths; a.ext = ext; a.ext_scalar = ext_scalar; a.max_len = max_len;
  a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv; a.lcap = h->lcap; a.scale = (float)(1.0 / std::sqrt((double)h->hd));
  a.scores = h->scores; a.cmax = h->cmax; a.out = out; a.rows = rows; a.stamps = stamps;
  a.kv8 = kv8 && kv_fp8_attn_reads(h, rows, kv == nullptr) ? kv8 : nullptr;      // kv8: the code cache of `kv` (the FP8 KV cache in effect), or NULL; kv == NULL: codes only
  if (!a.kv8 && !kv) ZN_FAIL(h, ZN_ERR_STATE, "attention: neither a bf16 cache nor a code cache it may read (%d rows)", rows);
  const int hd = h->hd;
  dim3 grid((max_len + ZN_ACHUNK - 1) / ZN_ACHUNK, c.n_heads_kv, rows);
  // fused: one launch for contexts of one 512-key block (the caller bounds the context: attn_fused_for); else: scores, then the P.V pass
  // with one workgroup per (slice, kv head, row, 512-key block) and the ticketed in-order combine
  a.part = h->pv_part; a.tickets = h->pv_tickets; a.nbcap = (max_len + 511) / 512;
  if (a.nbcap > 32) ZN_FAIL(h, ZN_ERR_ARG, "attention: %d keys of capacity exceed the 32 blocks the split pass combines", max_len);
  // batches of 3..8 utterances: two workgroups per (row, kv head[, block]), each with half of the value columns (ZN_TUNE_ATTN_SPLIT_COLS = 1: never, 2: always)
  const bool sc = attn_split_cols(h, rows);
  int r2 = hd == 128 ? launch_attn_g<128>(a, h->G, grid, fused, sc, s) : hd == 64 ? launch_attn_g<64>(a, h->G, grid, fused, sc, s)
                                                                                 : launch_attn_g<32>(a, h->G, grid, fused, sc, s);
  if (r2) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "attention: unsupported group %d", h->G);
  return ZN_OK;
}

// ---- The linears of a decode step: what each is, is zn_step_linears.h's table; here, the handle's side of it (which layer offers a stream, the W8 pointers, the
// arguments) and the ONE launcher every step linear goes through.
static bool mlp_fp8_offered(zn_handle h, int li) { return li >= 0 && h->mlp_fp8[li].fc1_q != nullptr && h->tune[ZN_TUNE_MLP_FP8] != 2; }
static bool mamba_fp8_offered(zn_handle h, int li) { return li >= 0 && h->mamba_fp8[li].in_q != nullptr && h->tune[ZN_TUNE_MAMBA_FP8] != 2; }
// layer li offers linear `lin` the FP8 stream the table names for it
static bool stream_offered(zn_handle h, int lin, int li) {
  const int offer = step_linear_offer(lin);
  return offer == SO_MLP ? mlp_fp8_offered(h, li) : offer == SO_MAMBA ? mamba_fp8_offered(h, li) : false;
}
// ... and so does EVERY layer that has the linear (the plan queries: a handle with streams on some layers only reports none)
static bool every_layer_offers(zn_handle h, int lin) {
  const int offer = step_linear_offer(lin);
  if (offer == SO_NONE || h->cfg.arch != (offer == SO_MAMBA ? 1 : 0)) return false;
  int n = 0;
  for (int li = 0; li < h->cfg.n_layer; ++li)
    if (offer == SO_MLP || h->layers[li].kind == 1) { ++n; if (!stream_offered(h, lin, li)) return false; }
  return n > 0;
}
static void attach_w8(zn_handle h, int lin, int li, GemvArgs& a) {
  if (li < 0) return;
  const zn_handle_s::MlpFp8& f = h->mlp_fp8[li];
  const zn_handle_s::MambaFp8& m = h->mamba_fp8[li];
  switch (lin) {
    case SL_FC1: a.W8q = f.fc1_q; a.W8exp = f.fc1_exp; break;
    case SL_FC2: a.W8q = f.fc2_q; a.W8exp = f.fc2_exp; break;
    case SL_M_IN_PROJ: a.W8q = m.in_q; a.W8exp = m.in_exp; break;
    case SL_M_OUT_PROJ: a.W8q = m.out_q; a.W8exp = m.out_exp; break;
  }
}
// li: the layer (its qkv bias decides the hybrid in_proj's epilogue), -1 = none
static bool step_in_proj_bias(zn_handle h, int lin, int li) { return lin == SL_H_IN_PROJ && li >= 0 && h->layers[li].in_proj_bias != nullptr; }
static LinearPlan step_plan(zn_handle h, int lin, int li, int rows, bool offered, bool stats_in = false) {
  return plan_step_linear(linear_env(h), h->cfg, h->tune, lin, rows, offered, stats_in, step_in_proj_bias(h, lin, li));
}
static GemvArgs linear_args(zn_handle h, const void* W, int N, int K, const bf16_t* x, bf16_t* out, const bf16_t* resid = nullptr) {
  GemvArgs a{};
  a.W = (const bf16_t*)W; a.N = N; a.K = K; a.x = x; a.out = out; a.resid = resid; a.eps = h->cfg.norm_eps;
  return a;
}
// the arguments of a step linear; N and K are the table's: launch_step_linear fills them
static GemvArgs step_args(zn_handle h, const void* W, const bf16_t* x, bf16_t* out, const bf16_t* resid = nullptr) { return linear_args(h, W, 0, 0, x, out, resid); }
// Launches step linear `lin` of layer li as plan p says.  The call site names the kernel pair; the table decides it: a pair that is not the table's launches nothing.
// d: the table's description, when the caller has it already
template <int PRO, int EPI>
static int launch_step_linear(zn_handle h, int lin, int li, const LinearPlan& p, GemvArgs a, int rows, hipStream_t s, const StepLinearDesc* known = nullptr) {
  const StepLinearDesc d = known ? *known : step_linear_desc(h->cfg, h->tune, lin, rows, step_in_proj_bias(h, lin, li));
  if (d.pro != PRO || d.epi != EPI) ZN_FAIL(h, ZN_ERR_STATE, "step linear %d: the call launches <%d, %d>, the table says <%d, %d>", lin, PRO, EPI, d.pro, d.epi);
  a.N = d.N; a.K = d.K;
  attach_w8(h, lin, li, a);
  return launch_linear<PRO, EPI>(h, p, a, rows, s);
}
template <int PRO, int EPI>
static int run_step_linear(zn_handle h, int lin, int li, const GemvArgs& a, int rows, hipStream_t s) {
  const StepLinearDesc d = step_linear_desc(h->cfg, h->tune, lin, rows, step_in_proj_bias(h, lin, li));
  return launch_step_linear<PRO, EPI>(h, lin, li, plan_step_linear(linear_env(h), h->tune, d, rows, stream_offered(h, lin, li), false), a, rows, s, &d);
}
static GemvArgs in_proj_args(zn_handle h, const zn_layer_weights& lw, const bf16_t* x, bf16_t* kv, int max_len, const int* lengths, uint8_t* kv8 = nullptr, bool kv_round = false) {
  const zn_config& c = h->cfg;
  GemvArgs a = step_args(h, lw.in_proj, x, nullptr);
  a.ln_w = (const bf16_t*)lw.norm_w; a.ln_b = (const bf16_t*)lw.norm_b; a.lengths = lengths; a.hd = h->hd; a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv;
  a.q_out = h->q; a.kv = kv; a.rope = h->rope; a.max_len = max_len; a.rope_positions = c.rope_positions;
  a.kv8 = kv8; a.kv_round = kv_round ? 1 : 0;
  return a;
}
static GemvArgs fc1_args(zn_handle h, const zn_layer_weights& lw, const bf16_t* x, const float* ln_stats) {   // ln_stats: left by x's producer, or null
  GemvArgs a = step_args(h, lw.fc1, x, h->mbuf);
  a.ln_w = (const bf16_t*)lw.norm2_w; a.ln_b = (const bf16_t*)lw.norm2_b; a.ln_part_in = ln_stats;
  return a;
}
// The projection that completes the residual stream (the second out_proj call under double_out_proj, else the single one) and fc1, planned
// together: fc1 normalises from handed-over LayerNorm statistics exactly when that projection's plan writes them (rows 5..16).
// mlp_w8: the layer's fc1 / fc2 are offered as an FP8 stream too (mlp_fp8_offered).
struct PostAttnPlans { LinearPlan out, fc1, fc2; };
static PostAttnPlans plan_post_attention(zn_handle h, int rows, bool mlp_w8 = false) {
  PostAttnPlans pp;
  pp.out = step_plan(h, SL_OUT_PROJ, -1, rows, false);
  pp.fc1 = step_plan(h, SL_FC1, -1, rows, mlp_w8, pp.out.writes_ln_stats);
  pp.fc2 = step_plan(h, SL_FC2, -1, rows, mlp_w8);
  return pp;
}

// LayerNorm -> in_proj -> split -> RoPE(q,k) -> KV append of block `li` (q in h->q, k/v in the cache row lengths[r])
static int layer_in_proj(zn_handle h, int li, bf16_t* x, bf16_t* kv, int max_len, const int* lengths, int rows, hipStream_t s, uint8_t* kv8 = nullptr, bool kv_round = false) {
  return run_step_linear<PRO_LN, EPI_ROPE_KV>(h, SL_IN_PROJ, li, in_proj_args(h, h->layers[li], x, kv, max_len, lengths, kv8, kv_round), rows, s);
}

// out_proj (-> out_proj again, _torch.py:419-420) -> residual -> LayerNorm -> fc1 -> y * silu(gate) -> fc2 -> residual
// pp: the plans, when the caller made them already (zn_bench_kernel); which: all three launches, or one of SL_OUT_PROJ / SL_FC1 / SL_FC2 alone
static int layer_post_attention(zn_handle h, int li, bf16_t* x, int rows, hipStream_t s, bf16_t* x1_copy = nullptr, const PostAttnPlans* planned = nullptr, int which = -1) {
  const zn_layer_weights& lw = h->layers[li];
  const PostAttnPlans pp = planned ? *planned : plan_post_attention(h, rows, mlp_fp8_offered(h, li));
  int rc;
  if (which < 0 || which == SL_OUT_PROJ) {
    GemvArgs o = step_args(h, lw.out_proj, h->o1, x, x);
    o.ln_part_out = h->ln_part;
    if (h->cfg.double_out_proj && which < 0) {   // q is dead after attention: reuse it for the intermediate projection
      if ((rc = run_step_linear<PRO_NONE, EPI_STORE>(h, SL_OUT_PROJ_FIRST, li, step_args(h, lw.out_proj, h->o1, h->q), rows, s))) return rc;
      o.x = h->q;
    }
    if ((rc = launch_step_linear<PRO_NONE, EPI_RESID>(h, SL_OUT_PROJ, li, pp.out, o, rows, s))) return rc;
    if (x1_copy) (void)hipMemcpyAsync(x1_copy, x, (size_t)rows * h->cfg.d_model * 2, hipMemcpyDeviceToDevice, s);      // diagnostic trace
  }
  if ((which < 0 || which == SL_FC1) && (rc = launch_step_linear<PRO_LN, EPI_SILU>(h, SL_FC1, li, pp.fc1, fc1_args(h, lw, x, pp.out.writes_ln_stats ? h->ln_part : nullptr), rows, s))) return rc;
  if (which < 0 || which == SL_FC2) return launch_step_linear<PRO_NONE, EPI_RESID>(h, SL_FC2, li, pp.fc2, step_args(h, lw.fc2, h->mbuf, x, x), rows, s);
  return ZN_OK;
}

// One decode step of block `li` on x [rows][d] in place (_torch.py:307-328), as launches.
static int layer_decode(zn_handle h, int li, bf16_t* x, bf16_t* kv, int max_len, const int* lengths, const int* ext,
                        int ext_scalar, int rows, int attn_fused, hipStream_t s) {
  int rc;
  if ((rc = layer_in_proj(h, li, x, kv, max_len, lengths, rows, s))) return rc;
  // KV-cached GQA attention over keys [0, lengths+1) (_torch.py:413-417) -> attention output in h->o1
  if ((rc = run_attention(h, h->q, kv, max_len, lengths, ext, ext_scalar, h->o1, rows, attn_fused, s))) return rc;
  return layer_post_attention(h, li, x, rows, s);
}

// The chain never updates the residual stream in place (zn_chain_kernel.h): block li reads it from one buffer and leaves it
// in the other.
static bf16_t* chain_x(zn_handle h, int li) { return (li & 1) ? h->ch_x2 : h->x; }

// Post-attention chain of block `li` plus the in_proj of block li + 1 in ONE launch (zn_chain_kernel.h); x = h->x, the
// attention output in h->o1, the next block's q in h->q.
// Heads matrix rows per workgroup fit the chain's op-4 schedule (5 tiles per compute wave, one epilogue lane per (pair, row))?
static bool chain_heads_fit(zn_handle h) {
  const int units = (h->cfg.n_codebooks * h->cfg.vocab_head + 1) / 2, ppw = (units + ZN_CH_GRID - 1) / ZN_CH_GRID;
  return ppw <= ZN_CH_CWAVES * 5 && ppw * 2 <= 64;
}

// with_heads: the last block's launch also applies norm_f + the fused heads (fp32 logits into h->logits_raw)
static int launch_chain(zn_handle h, int li, const std::vector<const void*>& kv_layers, int max_len, const int* lengths, hipStream_t s,
                        const bf16_t* xin = nullptr, bool with_heads = false) {
  const zn_config& c = h->cfg;
  const zn_layer_weights& lw = h->layers[li];
  const bool last = li + 1 >= c.n_layer;
  ChainArgs a{};
  a.W_out = (const bf16_t*)lw.out_proj; a.W_fc1 = (const bf16_t*)lw.fc1; a.W_fc2 = (const bf16_t*)lw.fc2;
  a.ln2_w = (const bf16_t*)lw.norm2_w; a.ln2_b = (const bf16_t*)lw.norm2_b; a.eps = c.norm_eps; a.F = c.d_ff;
  a.a = h->o1; a.xin = xin ? xin : chain_x(h, li); a.xout = chain_x(h, li + 1);
  a.g_y1 = h->ch_gy1; a.g_x1 = h->ch_gx1; a.g_x2 = h->ch_gx2; a.g_m = h->ch_gm;
  a.epoch = h->ch_epoch; a.tmo = &h->st->pad[0]; a.diag = h->ch_diag;
  a.dbg_pause = h->gen.dbg_pause; a.stamp_layer = li;
  a.stamps = h->ch_stamps ? h->ch_stamps + (size_t)li * 32 : nullptr;
  if (!last) {
    const zn_layer_weights& nx = h->layers[li + 1];
    a.W_in = (const bf16_t*)nx.in_proj; a.lnn_w = (const bf16_t*)nx.norm_w; a.lnn_b = (const bf16_t*)nx.norm_b;
    a.nqkv = (c.n_heads + 2 * c.n_heads_kv) * h->hd;
    a.q_out = h->q; a.kv = (bf16_t*)kv_layers[li + 1]; a.rope = h->rope; a.lengths = lengths;
    a.max_len = max_len; a.hd = h->hd; a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv; a.rope_positions = c.rope_positions;
  }
  const bool heads = last && with_heads;
  if (heads) {
    a.W_in = (const bf16_t*)h->heads; a.lnn_w = (const bf16_t*)h->norm_f_w; a.lnn_b = (const bf16_t*)h->norm_f_b;
    a.nqkv = c.n_codebooks * c.vocab_head; a.heads_out = h->logits_raw;
  }
  const dim3 grid(ZN_CH_GRID), block(ZN_CH_THREADS);
  if (h->ch_variant == 1) {
    if (heads) hipLaunchKernelGGL((chain_kernel<4, 1, 8, 4, 5>), grid, block, ZN_CH_DYN_LDS, s, a);
    else if (last) hipLaunchKernelGGL((chain_kernel<4, 1, 8, 4, 0>), grid, block, ZN_CH_DYN_LDS, s, a);
    else hipLaunchKernelGGL((chain_kernel<4, 1, 8, 4, 2>), grid, block, ZN_CH_DYN_LDS, s, a);
  } else {
    if (heads) hipLaunchKernelGGL((chain_kernel<1, 1, 2, 1, 5>), grid, block, ZN_CH_DYN_LDS, s, a);
    else if (last) hipLaunchKernelGGL((chain_kernel<1, 1, 2, 1, 0>), grid, block, ZN_CH_DYN_LDS, s, a);
    else hipLaunchKernelGGL((chain_kernel<1, 1, 2, 1, 1>), grid, block, ZN_CH_DYN_LDS, s, a);
  }
  return ZN_OK;
}

// Whole-step kernel (zn_step_kernel.h): batch 1 at the Zonos-v0.1 shapes: in_proj(0) + ONE launch per decode step.  The default at batch 1;
// zn_debug_tune(ZN_TUNE_WHOLE_STEP, 2) or ZN_STACK=0 in the environment at zn_create selects one chain launch per block.  Instantiations (static tile schedules
// for the streaming workgroups the attention role leaves):
//   variant 1  <4, 2, 10, 5, 6, 6>   1 .. 6 key blocks  (8 .. 48 attention workgroups: contexts up to 3072 keys)
//   variant 2  <4, 2, 11, 6, 7, 8>   7 .. 8 blocks   (up to 4096 keys)
//   variant 3  <4, 2, 13, 7, 8, 12>  9 .. 12 blocks  (up to 6144 keys); longer contexts take the per-block path
// One row (step_r1_kernel, cfg_scale == 1) uses the same three instantiations with Hkv * NBK attention workgroups: the streaming workgroups
// grow from 256 - 8 NBK to 256 - 4 NBK, and their fullest share of every matrix never exceeds the two-row launch's.
// The T_* are tiles per compute wave, so they follow ZN_SK_CW.  With 208 / 192 / 160 streaming workgroups the fullest workgroup has 5 / 6 / 7 row pairs
// of out_proj (four K-quarter tiles each in fc2), 40 / 44 / 52 rows of fc1, 8 / 8 / 10 row pairs of in_proj and 23 / 25 / 29 of the heads; six compute
// waves (-DZN_SK_CW=6) cover them with
//   variant 1  <4, 1, 7, 4, 4, 6>    variant 2  <4, 1, 8, 4, 5, 8>    variant 3  <4, 2, 9, 5, 5, 12>
#if ZN_SK_CW == 6
#define ZN_SK_T1 4, 1, 7, 4, 4, 6
#define ZN_SK_T2 4, 1, 8, 4, 5, 8
#define ZN_SK_T3 4, 2, 9, 5, 5, 12
#else
#define ZN_SK_T1 4, 2, 10, 5, 6, 6
#define ZN_SK_T2 4, 2, 11, 6, 7, 8
#define ZN_SK_T3 4, 2, 13, 7, 8, 12
#endif
static int stack_variant_of(int mode) { return mode <= 6 ? 1 : mode <= 8 ? 2 : 3; }
template <int R, int NCH, int T_OUT, int T_FC1, int T_FC2, int T_IN, int NBV>
static bool stack_variant_ok(zn_handle h, int natt) {
  const zn_config& c = h->cfg;
  const int nsw = ZN_CH_GRID - natt;
  if (nsw < 64) return false;
  auto most = [&](int units) { return (units + nsw - 1) / nsw; };                     // units of the fullest streaming workgroup
  const int nqkv = (c.n_heads + 2 * c.n_heads_kv) * h->hd;
  const int p_out = most(c.d_model / 2), p_fc1 = 2 * most(c.d_ff / 2), p_qkv = most((nqkv + 1) / 2), p_hd = most((c.n_codebooks * c.vocab_head + 1) / 2);
  if (p_out > ZN_SK_CW * T_OUT || 4 * p_out > ZN_SK_CW * T_FC2 || p_fc1 > ZN_SK_CW * T_FC1 || p_qkv > ZN_SK_CW * T_IN || p_hd > ZN_SK_CW * T_IN) return false;   // the static schedule
  if (p_qkv > 10) return false;                                                                                                   // the pre-block: five row pairs per helper wave, or two per compute wave when there are six
  if (p_out * 2 > 64 || p_out * 4 > 64 || p_fc1 > 64 || p_qkv * 2 > 64 || p_hd * 2 > 64 || nqkv % 2) return false;              // one epilogue lane per (unit, row); s_res slots
  // every workgroup of the grid must be resident at once (the hand-offs wait on all of them): one per CU by its LDS, no scratch
  const void* fn = R == 1 ? (const void*)step_r1_kernel<NCH, T_OUT, T_FC1, T_FC2, T_IN, NBV> : (const void*)step_kernel<NCH, T_OUT, T_FC1, T_FC2, T_IN, NBV>;
  int dev = 0, n_cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, ZN_SK_DYN_LDS) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, ZN_SK_THREADS, ZN_SK_DYN_LDS) != hipSuccess) { (void)hipGetLastError(); return false; }
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return false; }
  return per_cu >= 1 && n_cus >= ZN_CH_GRID && fa.localSizeBytes == 0;
}
static bool stack_shapes_ok(zn_handle h) {
  const zn_config& c = h->cfg;
  if (h->ch_variant != 1 || h->hd != 128 || c.n_heads_kv < 1 || c.n_heads != 4 * c.n_heads_kv) return false;
  const int npairs = 2 * c.n_heads_kv, nkvh = c.n_heads_kv;
  h->stackv_ok[1] = stack_variant_ok<2, ZN_SK_T1>(h, npairs * 6);
  h->stackv_ok[2] = stack_variant_ok<2, ZN_SK_T2>(h, npairs * 8);
  h->stackv_ok[3] = stack_variant_ok<2, ZN_SK_T3>(h, npairs * ZN_SK_KB_MAXNB);
  h->stackv1_ok[1] = stack_variant_ok<1, ZN_SK_T1>(h, nkvh * 6);
  h->stackv1_ok[2] = stack_variant_ok<1, ZN_SK_T2>(h, nkvh * 8);
  h->stackv1_ok[3] = stack_variant_ok<1, ZN_SK_T3>(h, nkvh * ZN_SK_KB_MAXNB);
  h->stack1_ok = h->stackv1_ok[1];
  return h->stackv_ok[1];
}
// ------------------------------------------------------------------------------------------------ step plan: which kernels serve a decode step
// The persistent kernels are allowed for this generation: not switched off (zn_debug_tune(ZN_TUNE_PERSISTENT, 2), or ZN_CHAIN=0 in the environment at zn_create), the handle not demoted by
// a hand-off timeout, the device's tenancy held, and no two unguided rows of different lengths (zn_prefill_rows): the two-row persistent kernels read lengths[r] per row, but their hand-off
// schedules, key-block counts and graph slots were built and measured for the guided pair, whose rows advance in lockstep; such rows run the launches path, bit-identical by construction.
// Nor a column shift per utterance (zn_gen_set_prefix_rows): the fused tail's sampler and sample1_kernel do not read it, so two unguided rows whose audio prefixes differ run the launches
// path even when their lengths advance in lockstep.
// Nor a slotted session (zn_gen_open_slots): its samplers read the row table, the shifts and the slots' step origins.
// The handle's half is here; the generation's half is GenHost::persist_eligible.
static bool persist_allowed(zn_handle h) { return h->tune[ZN_TUNE_PERSISTENT] != 2 && !h->demoted && h->gen.persist_eligible(); }
// Row counts a persistent kernel can serve on this model: two (the per-block chain and step_kernel) or one (step_r1_kernel, the whole-step
// kernel only: one row beyond its 6144-key bound, or with it switched off, runs the launches path).
static bool persist_shape(zn_handle h, int rows) { return h->ch_variant != 0 && (rows == 2 || (rows == 1 && h->ch_variant == 1)); }
static bool persist_active(zn_handle h, int rows) { return persist_shape(h, rows) && persist_allowed(h); }
// The key blocks a whole-step launch covering `keys_upper_bound` keys needs: -1 = the whole-step kernel does not serve the step (the
// per-block path does at two rows, the launches path at one), n >= 1 = rows * Hkv * n attention workgroups.  For rows that are persist_active.
static int stack_blocks_for(zn_handle h, int rows, int keys_upper_bound) {
  if (h->tune[ZN_TUNE_WHOLE_STEP] == 2 || !(rows == 1 ? h->stack1_ok : h->stack_ok)) return -1;
  const int nb = keys_upper_bound <= 512 ? 1 : (keys_upper_bound + 511) / 512;
  return nb <= ZN_SK_KB_MAXNB && (rows == 1 ? h->stackv1_ok : h->stackv_ok)[stack_variant_of(nb)] ? nb : -1;
}
// Launches path and chain path: slots 0..2 (one step) and 4..6 (a run), by attention launch shape.  Whole-step kernel: one slot per key-block
// count of the attention role, 8 + nbk (one step) and 8 + (ZN_SK_KB_MAXNB + 1) + nbk (a run).
static int graph_slot_for(const StepPlan& p) { return p.path == StepPlan::STACK ? 8 + (p.run > 1 ? ZN_SK_KB_MAXNB + 1 : 0) + p.nbk : p.attn_fused + (p.run > 1 ? 4 : 0); }
// The per-block persistent chain serves two rows when the model fits an instantiation: 1.07 vs 1.16 ms per decode step at the Zonos-v0.1 dimensions.
static bool chain_allowed(zn_handle h, int rows) { return h->ch_variant != 0 && rows == 2 && persist_allowed(h); }
// One step of `rows` rows over at most `keys` keys off the whole-step kernel (a step of plan_steps, or of the position-by-position prefill).
static StepPlan plan_blocks(zn_handle h, int rows, int keys) {
  StepPlan p;
  p.path = chain_allowed(h, rows) ? StepPlan::CHAIN : StepPlan::LAUNCHES; p.attn_fused = attn_fused_for(h, keys);
  return p;
}
// The next decode steps of the generation, `steps_left` of them still asked for.  A step appends one key per row; a run of ZN_GRAPH_STEPS steps with one launch shape replays the long graph.
// The whole-step kernel serves every step whose context fits one of its instantiations; a run takes the attention role its LAST step needs (workgroups of key blocks past a step's context leave
// at once).  Fused tail: at batch 1 on a persistent kernel the step's tail (bookkeeping + next step's embedding) runs in the sampler launch's last workgroup.  Larger batches keep three launches
// (one workgroup embedding 8 utterances in turn cost 31 us per step at batch 8), and so does the launches path (its first op reads h->x): one row has the fused tail only on whole-step steps.
static StepPlan plan_steps(zn_handle h, int steps_left) {
  const int rows = h->gen.rows, keys = h->gen.len_hi + 1, keys_run = h->gen.len_hi + ZN_GRAPH_STEPS;
  const bool want_run = steps_left >= ZN_GRAPH_STEPS && h->tune[ZN_TUNE_GRAPH_RUNS] > 1;
  const bool tail_ok = h->cfg.arch == 0 && persist_active(h, rows) && h->gen.batch <= 2;
  const int nb_run = tail_ok && want_run ? stack_blocks_for(h, rows, keys_run) : -1;
  const int nb_one = tail_ok ? stack_blocks_for(h, rows, keys) : -1;
  StepPlan p = plan_blocks(h, rows, keys);
  if (nb_run >= 0 || nb_one >= 0) {
    p.path = StepPlan::STACK; p.nbk = nb_run >= 0 ? nb_run : nb_one; p.run = nb_run >= 0 ? ZN_GRAPH_STEPS : 1;
  } else if (want_run && attn_fused_for(h, keys_run) == p.attn_fused) p.run = ZN_GRAPH_STEPS;
  p.fused_tail = tail_ok && p.path != StepPlan::LAUNCHES;
  p.graph_slot = graph_slot_for(p);
  return p;
}
static bool stack_pre(zn_handle h) { return h->tune[ZN_TUNE_STACK_PRE] != 2; }
static int launch_stack(zn_handle h, hipStream_t s, int rows, int nbk) {
  const zn_config& c = h->cfg;
  ChainArgs a{};
  a.eps = c.norm_eps; a.F = c.d_ff; a.nqkv = (c.n_heads + 2 * c.n_heads_kv) * h->hd;
  a.xin = h->x_emb; a.xout = h->x;
  a.g_y1 = h->ch_gy1; a.g_x1 = h->ch_gx1; a.g_x2 = h->ch_gx2; a.g_m = h->ch_gm; a.g_qkv = h->ch_gqkv; a.g_a = h->ch_ga;
  a.g_bmax = h->ch_gbmax; a.g_part = h->ch_gpart;
  a.epoch = h->ch_epoch; a.tmo = &h->st->pad[0]; a.diag = h->ch_diag;
  a.dbg_pause = h->gen.dbg_pause;
  a.stamps = h->ch_stamps; a.stamp_layer = c.n_layer / 2;
  a.rope = h->rope; a.lengths = h->gen.lengths; a.max_len = h->gen.max_len; a.hd = h->hd; a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv;
  a.rope_positions = c.rope_positions;
  a.layers = h->stack_layers; a.n_layer = c.n_layer; a.q0 = h->q; a.scale = (float)(1.0 / std::sqrt((double)h->hd));
  a.heads_rows = c.n_codebooks * c.vocab_head; a.heads_out = h->logits_raw; a.trace = h->dbg_trace;
  const int mode = nbk, npairs = rows * c.n_heads_kv;
  a.natt = npairs * (mode < 1 ? 1 : mode);
  if (stack_pre(h)) {       // block 0's LayerNorm + in_proj + RoPE + KV append inside the launch (ZN_TUNE_STACK_PRE = 2: as a launch before it)
    a.pre_W = (const bf16_t*)h->layers[0].in_proj; a.pre_ln_w = (const bf16_t*)h->layers[0].norm_w; a.pre_ln_b = (const bf16_t*)h->layers[0].norm_b;
    a.pre_kv = (bf16_t*)h->gen.kv_layers[0];
  }
  const dim3 grid(ZN_CH_GRID), block(ZN_SK_THREADS);
  if (rows == 1) {
    switch (stack_variant_of(mode)) {
      case 1: hipLaunchKernelGGL((step_r1_kernel<ZN_SK_T1>), grid, block, ZN_SK_DYN_LDS, s, a); break;
      case 2: hipLaunchKernelGGL((step_r1_kernel<ZN_SK_T2>), grid, block, ZN_SK_DYN_LDS, s, a); break;
      default: hipLaunchKernelGGL((step_r1_kernel<ZN_SK_T3>), grid, block, ZN_SK_DYN_LDS, s, a); break;
    }
    return ZN_OK;
  }
  if (rows != 2) ZN_FAIL(h, ZN_ERR_STATE, "launch_stack: %d rows (the whole-step kernel serves one or two)", rows);
  switch (stack_variant_of(mode)) {
    case 1: hipLaunchKernelGGL((step_kernel<ZN_SK_T1>), grid, block, ZN_SK_DYN_LDS, s, a); break;
    case 2: hipLaunchKernelGGL((step_kernel<ZN_SK_T2>), grid, block, ZN_SK_DYN_LDS, s, a); break;
    default: hipLaunchKernelGGL((step_kernel<ZN_SK_T3>), grid, block, ZN_SK_DYN_LDS, s, a); break;
  }
  return ZN_OK;
}
// device table of the whole-step kernel (KV cache pointers of this generation)
static int build_stack_table(zn_handle h) {
  const zn_config& c = h->cfg;
  std::vector<StackLayer> t(c.n_layer);
  for (int li = 0; li < c.n_layer; ++li) {
    const zn_layer_weights& lw = h->layers[li];
    const bool last = li + 1 == c.n_layer;
    StackLayer& L = t[li];
    L.W_out = (const bf16_t*)lw.out_proj; L.W_fc1 = (const bf16_t*)lw.fc1; L.W_fc2 = (const bf16_t*)lw.fc2;
    L.ln2_w = (const bf16_t*)lw.norm2_w; L.ln2_b = (const bf16_t*)lw.norm2_b;
    L.kv = (const bf16_t*)h->gen.kv_layers[li];
    if (last) { L.W_in = (const bf16_t*)h->heads; L.lnn_w = (const bf16_t*)h->norm_f_w; L.lnn_b = (const bf16_t*)h->norm_f_b; L.kv_next = nullptr; }
    else {
      const zn_layer_weights& nx = h->layers[li + 1];
      L.W_in = (const bf16_t*)nx.in_proj; L.lnn_w = (const bf16_t*)nx.norm_w; L.lnn_b = (const bf16_t*)nx.norm_b; L.kv_next = (bf16_t*)h->gen.kv_layers[li + 1];
    }
  }
  HIPCHK(h, ZN_NOT_IN_CAPTURE(hipMemcpy(h->stack_layers, t.data(), t.size() * sizeof(StackLayer), hipMemcpyHostToDevice)));
  return ZN_OK;
}

// All blocks of one decode step on h->x (transformer): launches per op, or in_proj(0) + (attention, chain) per block, as the plan says.
// x0 != NULL: the residual stream enters the first block from there (the decode step's embedding buffer) instead of h->x.
// heads_done != NULL: the caller wants the logits too; set when the last block's chain launch has produced them.
static int decode_blocks(zn_handle h, const StepPlan& p, const int* ext, int ext_scalar, hipStream_t s, const bf16_t* x0 = nullptr, bool* heads_done = nullptr) {
  const zn_config& c = h->cfg;
  int rc;
  const size_t tb = (size_t)h->gen.rows * c.d_model * 2;
  const bool chain = p.path == StepPlan::CHAIN;
  if (x0 && !chain) ZN_FAIL(h, ZN_ERR_STATE, "decode_blocks: a separate input buffer is the chain path's");
  auto trace = [&](int li) {        // slots per block: x after the block, attention output, q, m (first d values per row pair), x after the attention half
    if (!h->dbg_trace) return;
    (void)hipMemcpyAsync((char*)h->dbg_trace + (size_t)(8 * li) * tb, chain ? chain_x(h, li + 1) : h->x, tb, hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync((char*)h->dbg_trace + (size_t)(8 * li + 1) * tb, h->o1, tb, hipMemcpyDeviceToDevice, s);
    if (!chain) (void)hipMemcpyAsync((char*)h->dbg_trace + (size_t)(8 * li + 3) * tb, h->mbuf, (size_t)h->gen.rows * c.d_ff * 2 <= 4 * tb ? (size_t)h->gen.rows * c.d_ff * 2 : 4 * tb, hipMemcpyDeviceToDevice, s);
  };
  auto trace_q = [&](int li) {      // q of block li, as the attention launch reads it
    if (h->dbg_trace) (void)hipMemcpyAsync((char*)h->dbg_trace + (size_t)(8 * li + 2) * tb, h->q, tb, hipMemcpyDeviceToDevice, s);
  };
  if (!chain) {
    for (int li = 0; li < c.n_layer; ++li) {
      // (the FP8 KV cache in effect - 5 rows or more, so never the chain below: the append rounds and writes both caches, the attention reads what its plan says)
      if ((rc = layer_in_proj(h, li, h->x, (bf16_t*)h->gen.kv_layers[li], h->gen.max_len, h->gen.lengths, h->gen.rows, s, kv8_of(h, li), kv_fp8_gen(h)))) return rc;
      trace_q(li);
      if ((rc = run_attention(h, h->q, (bf16_t*)h->gen.kv_layers[li], h->gen.max_len, h->gen.lengths, ext, ext_scalar, h->o1, h->gen.rows, p.attn_fused, s, nullptr, kv8_of(h, li)))) return rc;
      if ((rc = layer_post_attention(h, li, h->x, h->gen.rows, s, h->dbg_trace ? (bf16_t*)((char*)h->dbg_trace + (size_t)(8 * li + 7) * tb) : nullptr))) return rc;
      trace(li);
    }
    return ZN_OK;
  }
  if ((rc = layer_in_proj(h, 0, x0 ? const_cast<bf16_t*>(x0) : h->x, (bf16_t*)h->gen.kv_layers[0], h->gen.max_len, h->gen.lengths, h->gen.rows, s))) return rc;
  h->epoch_bound += c.n_layer;                             // one tag per chain launch (counted again by zn_decode_steps: the bound stays an upper bound)
  for (int li = 0; li < c.n_layer; ++li) {
    trace_q(li);
    if ((rc = run_attention(h, h->q, (bf16_t*)h->gen.kv_layers[li], h->gen.max_len, h->gen.lengths, ext, ext_scalar, h->o1, h->gen.rows, p.attn_fused, s,
                            h->ch_stamps ? h->ch_stamps + (size_t)(c.n_layer + li) * 32 : nullptr))) return rc;
    const bool wh = heads_done && li + 1 == c.n_layer && chain_heads_fit(h);
    if ((rc = launch_chain(h, li, h->gen.kv_layers, h->gen.max_len, h->gen.lengths, s, li == 0 ? x0 : nullptr, wh))) return rc;
    if (wh) *heads_done = true;
    trace(li);
  }
  if (c.n_layer & 1) HIPCHK(h, hipMemcpyAsync(h->x, h->ch_x2, tb, hipMemcpyDeviceToDevice, s));   // odd depth: the stream ends in the second buffer
  return ZN_OK;
}

static int heads_logits(zn_handle h, const bf16_t* x, int rows, hipStream_t s) {
  GemvArgs a = step_args(h, h->heads, x, nullptr);
  a.ln_w = (const bf16_t*)h->norm_f_w; a.ln_b = (const bf16_t*)h->norm_f_b; a.out_f32 = h->logits_raw;
  return run_step_linear<PRO_LN, EPI_F32>(h, SL_HEADS, -1, a, rows, s);
}

// ------------------------------------------------------------------------------------------------ hybrid backbone
// fused residual add + norm of the mamba_ssm Block over `rows` rows; the norm kind and the residual's type follow the config
static void launch_add_ln(zn_handle h, const bf16_t* hid, bf16_t* res, int has_res, int write_res, const void* w, const void* b, bf16_t* out, int rows,
                          hipStream_t s) {
  AddLnArgs a{};
  a.h = hid; a.res = res; a.w = (const bf16_t*)w; a.b = (const bf16_t*)b; a.out = out; a.d = h->cfg.d_model; a.has_res = has_res; a.write_res = write_res;
  a.eps = h->cfg.norm_eps; a.rms = h->cfg.rms_norm; a.res32 = h->cfg.residual_in_fp32;
  hipLaunchKernelGGL(add_ln_kernel, dim3(rows), dim3(256), 0, s, a);
}

// The Mamba2 in_proj with the conv window update + SiLU of its xBC rows in the epilogue (causal_conv1d_update; one launch less): n [rows][d] -> m_zx, m_xbc
static int mamba_in_proj(zn_handle h, int li, const bf16_t* n, void* conv_state, int rows, hipStream_t s) {
  const zn_config& c = h->cfg;
  const zn_layer_weights& lw = h->layers[li];
  GemvArgs a = step_args(h, lw.m_in_proj, n, h->m_zx);
  a.conv_state = (bf16_t*)conv_state; a.conv_w = (const bf16_t*)lw.m_conv_w; a.conv_b = (const bf16_t*)lw.m_conv_b; a.xbc = h->m_xbc;
  a.d_inner = c.m_d_inner; a.conv_dim = h->m_conv_dim;
  return run_step_linear<PRO_NONE, EPI_MAMBA>(h, SL_M_IN_PROJ, li, a, rows, s);
}

// The Mamba2 out_proj without a prologue (more than 4 rows, or several norm groups: g [rows][d_inner] is the gated norm's output) -> out [rows][d]
static int mamba_out_proj(zn_handle h, int li, const bf16_t* g, bf16_t* out, int rows, hipStream_t s) {
  return run_step_linear<PRO_NONE, EPI_STORE>(h, SL_M_OUT_PROJ, li, step_args(h, h->layers[li].m_out_proj, g, out), rows, s);
}

// The Mamba2 out_proj of up to 4 rows with RMSNormGated (one group) as its prologue: m_vg [rows][d_inner] fp32 gated values -> out [rows][d].  With the default
// settings this is the plan of a plain GEMV, under ZN_TUNE_FP8_SMALL_ROWS it reads the stream.
static int mamba_out_proj_gated(zn_handle h, int li, bf16_t* out, int rows, hipStream_t s) {
  GemvArgs o = step_args(h, h->layers[li].m_out_proj, nullptr, out);
  o.gv = h->m_vg; o.ln_w = (const bf16_t*)h->layers[li].m_norm_w;
  return run_step_linear<PRO_GATED, EPI_STORE>(h, SL_M_OUT_PROJ, li, o, rows, s);
}

// One token through the Mamba2 mixer of layer li (mamba_ssm Mamba2.step): n [rows][d] normalised -> out [rows][d]
static int mamba_mixer(zn_handle h, int li, const bf16_t* n, void* state, bf16_t* out, int rows, hipStream_t s) {
  const zn_config& c = h->cfg;
  const zn_layer_weights& lw = h->layers[li];
  int rc;
  if ((rc = mamba_in_proj(h, li, n, state, rows, s))) return rc;
  size_t conv_bytes = 0;   // the state buffer is laid out for exactly `rows` rows (zn_mamba_state_bytes_per_layer)
  (void)zn_mamba_state_bytes_per_layer(&c, rows, &conv_bytes);
  MambaArgs m{};
  m.zx = h->m_zx; m.conv_state = (bf16_t*)state; m.ssm_state = (bf16_t*)((char*)state + conv_bytes);
  m.conv_w = (const bf16_t*)lw.m_conv_w; m.conv_b = (const bf16_t*)lw.m_conv_b;
  m.dt_bias = (const bf16_t*)lw.m_dt_bias; m.A_log = (const bf16_t*)lw.m_A_log; m.D = (const bf16_t*)lw.m_D;
  m.norm_w = (const bf16_t*)lw.m_norm_w; m.xbc = h->m_xbc; m.y = h->m_y; m.g = h->m_g;
  m.d_inner = c.m_d_inner; m.conv_dim = h->m_conv_dim; m.nheads = h->m_nheads; m.d_state = c.m_d_state; m.ngroups = c.m_ngroups;
  m.d_in_proj = h->m_d_in_proj; m.eps = c.norm_eps;
  m.rows = rows;
  // RMSNormGated: up to 4 rows (the GEMV, whose waves hold whole rows) the gate product leaves the state-update kernel
  // in fp32 and the row statistic + weight run as the prologue of out_proj (one launch less; batch-1 step 1.28 -> 1.17 ms);
  // more rows, or several norm groups: a launch of its own (at 16 rows the prologue's fp32 fragment loads in each of the
  // 128 workgroups cost more than the launch: 1.92 -> 2.14 ms, measured)
  const bool gated_pro = mamba_gated_pro(c, rows);
  m.vg = gated_pro ? h->m_vg : nullptr;
  if (c.m_d_state == 128) hipLaunchKernelGGL((mamba_ssm_kernel<128, 2>), dim3(h->m_nheads, (rows + 1) / 2), dim3(256), 0, s, m);
  else hipLaunchKernelGGL((mamba_ssm_kernel<64, 2>), dim3(h->m_nheads, (rows + 1) / 2), dim3(256), 0, s, m);
  if (gated_pro) return mamba_out_proj_gated(h, li, out, rows, s);
  hipLaunchKernelGGL(mamba_gated_norm_kernel, dim3(c.m_ngroups, rows), dim3(256), 0, s, m);
  return mamba_out_proj(h, li, h->m_g, out, rows, s);
}

// One token through hybrid layer li (mamba_ssm Block, fused_add_norm): hidden h->x / residual h->res in, same out.
static int hybrid_layer(zn_handle h, int li, void* cache, int max_len, const int* lengths, int rows, int attn_fused, hipStream_t s) {
  const zn_config& c = h->cfg;
  const zn_layer_weights& lw = h->layers[li];
  int rc;
  // (the add + LayerNorm as a prologue of the GEMV that consumes it - every workgroup repeating it, the residual
  // ping-ponging between two buffers - was measured slower than this launch: batch-1 step 1.17 -> 1.24 ms)
  launch_add_ln(h, h->x, h->res, li > 0, 1, lw.norm_w, lw.norm_b, h->hn, rows, s);
  if (lw.kind == 1) return mamba_mixer(h, li, h->hn, cache, h->x, rows, s);
  if (step_linear_desc(c, h->tune, SL_H_IN_PROJ, rows, step_in_proj_bias(h, SL_H_IN_PROJ, li)).epi == EPI_ROPE_KV) {  // MHA: in_proj -> split -> interleaved RoPE(q,k) -> KV append, one launch
    GemvArgs a = step_args(h, lw.in_proj, h->hn, nullptr);
    a.lengths = lengths; a.hd = h->hd; a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv;
    a.q_out = h->q; a.kv = (bf16_t*)cache; a.rope = h->rope; a.max_len = max_len; a.rope_positions = c.rope_positions;
    if ((rc = run_step_linear<PRO_NONE, EPI_ROPE_KV>(h, SL_H_IN_PROJ, li, a, rows, s))) return rc;
  } else {   // the other attn_cfg forms (half-split or no rotary, qkv bias): projection (+ bias), then rotation + KV append
    GemvArgs a = step_args(h, lw.in_proj, h->hn, h->qkv_tmp);
    a.bias = (const bf16_t*)lw.in_proj_bias;
    if ((rc = run_step_linear<PRO_NONE, EPI_STORE>(h, SL_H_IN_PROJ, li, a, rows, s))) return rc;
    hipLaunchKernelGGL(rope_kv_any_kernel, dim3(1, rows), dim3(256), 0, s, h->qkv_tmp, h->q, c.n_heads * h->hd, (bf16_t*)cache, h->rope, 1, 0, lengths, max_len,
                       c.n_heads, c.n_heads_kv, h->hd, c.rope_positions, c.rope_mode);
  }
  if ((rc = run_attention(h, h->q, (const bf16_t*)cache, max_len, lengths, nullptr, 0, h->o1, rows, attn_fused, s))) return rc;
  GemvArgs o = step_args(h, lw.out_proj, h->o1, h->x);
  o.bias = (const bf16_t*)lw.out_proj_bias;
  if ((rc = run_step_linear<PRO_NONE, EPI_STORE>(h, SL_H_OUT_PROJ, li, o, rows, s))) return rc;
  launch_add_ln(h, h->x, h->res, 1, 1, lw.norm2_w, lw.norm2_b, h->hn, rows, s);
  if ((rc = run_step_linear<PRO_NONE, EPI_SILU>(h, SL_H_FC1, li, step_args(h, lw.fc1, h->hn, h->mbuf), rows, s))) return rc;
  return run_step_linear<PRO_NONE, EPI_STORE>(h, SL_H_FC2, li, step_args(h, lw.fc2, h->mbuf, h->x), rows, s);
}

// final add + norm (_mamba_ssm.py:111-119) of the token in h->x / h->res, then the heads
static int hybrid_heads(zn_handle h, hipStream_t s) {
  launch_add_ln(h, h->x, h->res, 1, 0, h->norm_f_w, h->norm_f_b, h->hn, h->gen.rows, s);
  GemvArgs a = step_args(h, h->heads, h->hn, nullptr);
  a.out_f32 = h->logits_raw;
  return run_step_linear<PRO_NONE, EPI_F32>(h, SL_H_HEADS, -1, a, h->gen.rows, s);
}

// All layers for the token in h->x, then the final add + LayerNorm and the heads.
static int hybrid_token(zn_handle h, bool want_logits, int attn_fused, hipStream_t s) {
  const zn_config& c = h->cfg;
  int rc;
  for (int li = 0; li < c.n_layer; ++li)
    if ((rc = hybrid_layer(h, li, (void*)h->gen.kv_layers[li], h->gen.max_len, h->gen.lengths, h->gen.rows, attn_fused, s))) return rc;
  if (!want_logits) return ZN_OK;
  return hybrid_heads(h, s);
}

static SampleArgs make_sample_args(zn_handle h, const zn_sampling& sp) {
  SampleArgs a{};
  const zn_config& c = h->cfg;
  a.n_q = c.n_codebooks; a.V = c.vocab_head; a.eos_id = c.eos_id;
  a.temperature = sp.temperature; a.top_p = sp.top_p; a.top_k = sp.top_k; a.min_p = sp.min_p;
  a.linear = sp.linear; a.conf = sp.conf; a.quad = sp.quad;
  a.penalty = sp.repetition_penalty; a.pen_window = sp.repetition_penalty_window;
  a.seed = sp.seed;
  return a;
}
static_assert(sizeof(zn_row_params) == ZN_ROW_PARAMS_BYTES, "zn_row_params is one 64-byte entry per utterance");

static bool guided(zn_handle h) { return h->gen.guided(); }

static EmbedArgs make_embed_args(zn_handle h) {
  const zn_config& c = h->cfg;
  EmbedArgs e{};
  e.tables = h->emb_tables_dev; e.codes = h->gen.codes; e.col_dev = &h->st->offset; e.sb = c.n_codebooks * h->gen.t_total; e.si = h->gen.t_total;
  e.col = 0; e.n_q = c.n_codebooks; e.d = c.d_model; e.batch = h->gen.batch; e.vocab_embed = c.vocab_embed; e.out = h->x_emb; e.dup = guided(h) ? 1 : 0;
  e.shift = h->gen.prefix_set ? h->prefix_shift : nullptr;
  e.step0 = h->gen.slots_open ? h->step0 : nullptr;
  return e;
}

// The sampler arguments of this generation's launches (first frame, decode steps of every path): the call-wide parameters, and the
// per-utterance table once zn_gen_set_rows has filled it, the column shifts once zn_gen_set_prefix_rows has.
static SampleArgs gen_sample_args(zn_handle h) {
  SampleArgs a = make_sample_args(h, h->gen.sp);
  a.cfg_scale = h->gen.cfg_scale; a.ctx = h->gen.max_new < 100 ? h->gen.max_new : 100;
  a.rows = h->gen.rows_set ? h->row_tab : nullptr;
  a.pairs = h->gen.pairs_set ? 1 : 0;
  a.shift = h->gen.prefix_set ? h->prefix_shift : nullptr;
  a.step0 = h->gen.slots_open ? h->step0 : nullptr;
  return a;
}
// The sampler launch over the heads' logits: of a decode step (the logit bias, the penalty over the codes, a draw), or of a first frame (the mix alone).
static SampleArgs make_frame_sampler(zn_handle h, bool step) {
  SampleArgs a = gen_sample_args(h);
  a.raw = h->logits_raw; a.mix = guided(h) ? 1 : 0; a.apply_bias = step ? 1 : 0; a.batch = h->gen.batch;
  if (step) { a.codes = h->gen.codes; a.t_total = h->gen.t_total; }
  a.use_penalty = step && (h->gen.rows_set || (h->gen.sp.repetition_penalty != 1.0f)); a.st = h->st; a.logits_out = h->last_logits; a.tokens = h->tok_raw;
  a.draw = step ? 1 : 0;
  return a;
}
// The bookkeeping that follows the sampler launch `a` (frame_update_kernel, or the tail in that launch's last workgroup).  slot >= 0: that slot of a session alone
// (an admission), which the test hook's token override leaves alone.
static FrameArgs make_frame_args(zn_handle h, const SampleArgs& a, int first, int slot) {
  const zn_config& c = h->cfg;
  FrameArgs f{};
  f.st = h->st; f.codes = h->gen.codes; f.t_total = h->gen.t_total; f.batch = h->gen.batch; f.n_q = c.n_codebooks; f.eos_id = c.eos_id;
  f.mask_id = c.mask_id; f.tokens = h->tok_raw; f.remaining = h->remaining; f.stopping = h->stopping; f.lengths = h->gen.lengths;
  f.rows = h->gen.rows; f.first = first; f.shift = a.shift; f.step0 = a.step0;
  if (slot >= 0) { f.slot_base = slot; f.slot_count = 1; }
  else { f.override = h->tok_override; f.override_calls = h->tok_override_calls; }
  return f;
}
// The first frame after a prefill: of every utterance (slot < 0: zn_sample_first), or of one admitted slot.
static void launch_first_frame(zn_handle h, int slot, hipStream_t s) {
  SampleArgs a = make_frame_sampler(h, false);
  if (slot >= 0) a.slot_base = slot;
  hipLaunchKernelGGL(sample_kernel, dim3(h->cfg.n_codebooks, slot >= 0 ? 1 : h->gen.batch), dim3(256), 0, s, a);
  hipLaunchKernelGGL(frame_update_kernel, dim3(1), dim3(256), 0, s, make_frame_args(h, a, 1, slot));
}

// One iteration of model.py:467-502: embed -> 26 blocks -> heads -> CFG/bias/penalty/sample -> bookkeeping.  With the fused tail the
// embedding of the current column is already in h->x_emb when the step starts (zn_decode_steps launches embed_kernel before the
// first step of a run; every step's sampler launch leaves the next one's, SampleArgs::ticket).
static int enqueue_step(zn_handle h, const StepPlan& p, hipStream_t s) {
  const zn_config& c = h->cfg;
  int rc;
  const bool fused = p.fused_tail;
  if (!fused) {
    EmbedArgs e = make_embed_args(h);
    e.out = h->x;
    hipLaunchKernelGGL(embed_kernel, dim3(h->gen.batch), dim3(256), 0, s, e);
  }
  if (c.arch == 1) {
    if ((rc = hybrid_token(h, true, p.attn_fused, s))) return rc;
  } else {
    bool heads_done = false;
    if (p.path == StepPlan::STACK) {                                 // every block + the heads in one launch (in_proj of block 0 inside it, or as a launch before it)
      if (!stack_pre(h) && (rc = layer_in_proj(h, 0, h->x_emb, (bf16_t*)h->gen.kv_layers[0], h->gen.max_len, h->gen.lengths, h->gen.rows, s))) return rc;
      if ((rc = launch_stack(h, s, h->gen.rows, p.nbk))) return rc;
      heads_done = true;
    } else if ((rc = decode_blocks(h, p, nullptr, 0, s, fused ? h->x_emb : nullptr, &heads_done))) return rc;
    if (!heads_done && (rc = heads_logits(h, h->x, h->gen.rows, s))) return rc;
  }
  SampleArgs a = make_frame_sampler(h, true);
  const FrameArgs f = a.fr = make_frame_args(h, a, 0, -1);
  if (fused) { a.ticket = h->tail_ticket; a.em = make_embed_args(h); }
  // batch 1, greedy decoding: sampling, bookkeeping and the next embedding in one workgroup (sample1_kernel: 0.8337 -> 0.8312 ms per step).  With a
  // temperature its one wave per codebook carries 17 exp / log / hash evaluations per lane and the nine ticketed workgroups are ahead again (0.8396 vs
  // 0.8415): they keep those steps.  ZN_TUNE_SAMPLER = 2: always the ticketed kernel; 3: the one-workgroup kernel for every parameter set it implements (tests).
  const bool one_wg = fused && h->gen.batch == 1 && !h->gen.rows_set && h->tune[ZN_TUNE_SAMPLER] != 2 && (h->tune[ZN_TUNE_SAMPLER] == 3 || !(h->gen.sp.temperature > 0.f)) && c.vocab_head <= 64 * ZN_S1_IT &&
                      c.n_codebooks <= 16 && !(h->gen.sp.top_p > 0.f) && h->gen.sp.top_k <= 0 && !(h->gen.sp.linear > 0.f) &&
                      (!a.use_penalty || h->gen.sp.repetition_penalty_window <= 16) && h->gen.rows <= 1024;
  if (one_wg) { hipLaunchKernelGGL(sample1_kernel, dim3(1), dim3(1024), 0, s, a); return ZN_OK; }
  hipLaunchKernelGGL(sample_kernel, dim3(c.n_codebooks, h->gen.batch), dim3(256), 0, s, a);
  if (!fused) hipLaunchKernelGGL(frame_update_kernel, dim3(1), dim3(256), 0, s, f);
  return ZN_OK;
}

// ------------------------------------------------------------------------------------------------ generation
extern "C" int zn_gen_begin(zn_handle h, int32_t batch, const void* const* kv_layers_dev, int32_t max_len, int32_t* lengths_dev,
                            int32_t* delayed_codes_dev, int32_t t_total, int32_t offset0, int32_t max_new_tokens, float cfg_scale,
                            const zn_sampling* sp, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!lengths_dev || !delayed_codes_dev || !sp) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_begin: null argument");
  if (!h->has_io) ZN_FAIL(h, ZN_ERR_STATE, "zn_gen_begin: handle was created without embeddings/heads");
  // cfg_scale == 1: no guidance, one row per utterance (the reference's _compute_logits skips the mix, model.py:230); else [cond ‖ uncond]
  const int rows = cfg_scale == 1.0f ? batch : 2 * batch;
  if (batch < 1 || rows > h->max_rows) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_begin: batch %d needs %d rows, max_rows is %d", batch, rows, h->max_rows);
  // a codes-only generation (zn_set_kv_fp8_only) has no bf16 caches: the argument may be NULL, and what it holds is never read or written
  const bool codes_only = kv_codes_only_rows(h, rows);
  if (!codes_only && !kv_layers_dev) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_begin: null argument");
  if (max_len < 1 || t_total < 1 || offset0 < 1 || offset0 >= t_total) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_begin: bad lengths");
  if (max_len > h->cfg.rope_positions)
    ZN_FAIL(h, ZN_ERR_ARG, "sequence length %d exceeds the %d-position RoPE table (zonos/backbone/_torch.py:206)", max_len, h->cfg.rope_positions);
  if (sp->repetition_penalty_window < 0 || sp->repetition_penalty_window > 64) ZN_FAIL(h, ZN_ERR_ARG, "repetition_penalty_window out of range");
  hipStream_t s = (hipStream_t)stream;
  int rc = ensure_attn_ws(h, max_len);
  if (rc) return rc;
  free_graph(h);
  h->gen.begin(batch, rows, max_len, t_total, offset0, max_new_tokens, cfg_scale, *sp, lengths_dev, delayed_codes_dev);   // = GenHost{} and these: every flag of the last generation is gone
  if (codes_only) h->gen.kv_layers.assign(h->cfg.n_layer, nullptr);
  else h->gen.kv_layers.assign(kv_layers_dev, kv_layers_dev + h->cfg.n_layer);
  // The hand-off tags are 32-bit and advance by n_layer per decode step (~41 hours of continuous batch-1 decoding): long before they
  // can wrap, between two generations, the epoch restarts at 1 over zeroed granule buffers (tag 0 is never a launch's epoch).
  if (h->pending_hook == ZN_HOOK_TAG_WRAP) { h->epoch_bound = 0x70000001ull; h->pending_hook = 0; }   // test hook: behave as if the tags were about to wrap
  if (h->epoch_bound > 0x70000000ull) {
    const size_t R = h->max_rows, nqkv = (size_t)(h->cfg.n_heads + 2 * h->cfg.n_heads_kv) * h->hd;
    for (unsigned long long* g : {h->ch_gy1, h->ch_gx1, h->ch_gx2, h->ch_ga}) HIPCHK(h, hipMemsetAsync(g, 0, R * (h->cfg.d_model / 2) * 8, s));
    HIPCHK(h, hipMemsetAsync(h->ch_gqkv, 0, R * (nqkv / 2 + 1) * 8, s));
    HIPCHK(h, hipMemsetAsync(h->ch_gm, 0, R * (h->cfg.d_ff / 2 + 1) * 8, s));
    HIPCHK(h, hipMemsetAsync(h->ch_gbmax, 0, (size_t)2 * h->cfg.n_heads_kv * ZN_SK_KB_MAXNB * 4 * 8, s));
    HIPCHK(h, hipMemsetAsync(h->ch_gpart, 0, (size_t)2 * h->cfg.n_heads_kv * ZN_SK_KB_MAXNB * ZN_SK_KB_PSZ * 8, s));
    const unsigned one = 1;
    HIPCHK(h, hipMemcpyAsync(h->ch_epoch, &one, sizeof one, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    h->epoch_bound = 1;
  }
  // A handle demoted by a reported hand-off timeout goes back to the persistent kernels after ZN_REARM_AFTER generations in a row
  // that completed on the launches path (a pause of the device is transient; a demotion for the handle's whole life would cost 25 % of
  // every later utterance on a say-so of one event).
  h->n_generations++;
  if (h->demoted && h->clean_since_demotion >= ZN_REARM_AFTER) { h->demoted = false; h->clean_since_demotion = 0; h->n_rearms++; }
  const bool persist_rows = h->cfg.arch == 0 && persist_shape(h, rows);
  if (h->demoted && persist_rows && h->tune[ZN_TUNE_PERSISTENT] != 2) h->n_fallback_generations++;
  // one or two rows on a model the persistent kernels serve: claim the device for them, or run this generation on the launches path
  h->gen.persist_ok = !persist_rows || zn_tenant_try_claim(h->device, h) != 0;
  if (h->cfg.arch == 0 && h->ch_variant == 1) {
    if (!h->stack_checked) { h->stack_ok = stack_shapes_ok(h); h->stack_checked = true; }
    if (h->stack_ok) { int rc = build_stack_table(h); if (rc) return rc; }
  }
  GenState st{};
  st.offset = offset0; st.step = 0; st.all_done = 0; st.force_eos_step = h->force_eos_step; st.eos_bias = h->eos_bias;
  if (h->pending_hook == ZN_HOOK_PAUSE) { h->gen.dbg_pause = 3000000u; h->pending_hook = 0; }   // test hook: every launch of this generation pauses all its waves for 30 ms in block 2
  if (h->pending_hook == ZN_HOOK_TIMEOUT_WORD) { st.pad[0] = 1; h->pending_hook = 0; }   // test hook: this generation's hand-off waits find the timeout word set
  HIPCHK(h, hipMemcpyAsync(h->st, &st, sizeof st, hipMemcpyHostToDevice, s));
  std::vector<int> rem(batch, t_total - offset0), stop(batch, 0);   // model.py:439-441
  HIPCHK(h, hipMemcpyAsync(h->remaining, rem.data(), batch * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->stopping, stop.data(), batch * sizeof(int), hipMemcpyHostToDevice, s));
  std::vector<int> len0(rows, 0);
  HIPCHK(h, hipMemcpyAsync(len0.data(), lengths_dev, rows * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));  // host vectors go out of scope
  for (int v : len0) if (v > h->gen.len_hi) h->gen.len_hi = v;
  h->gen.gen_active = true;
  h->gen_stream = s;
  return ZN_OK;
}

static int ensure_prefill_ws(zn_handle h, size_t M) {
  if (M <= h->pf_rows) return ZN_OK;
  const zn_config& c = h->cfg;
  for (bf16_t** p : {&h->pf_x, &h->pf_n, &h->pf_qkv, &h->pf_a, &h->pf_u, &h->pf_m, &h->pf_res, &h->pf_zx, &h->pf_xbc, &h->pf_y, &h->pf_g})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  h->pf_rows = 0;
  const size_t nqkv = (size_t)(c.n_heads + 2 * c.n_heads_kv) * h->hd;
  HIPCHK(h, hipMalloc(&h->pf_x, M * c.d_model * 2));
  HIPCHK(h, hipMalloc(&h->pf_n, M * c.d_model * 2));
  HIPCHK(h, hipMalloc(&h->pf_qkv, M * nqkv * 2));
  HIPCHK(h, hipMalloc(&h->pf_a, M * (size_t)c.n_heads * h->hd * 2));
  HIPCHK(h, hipMalloc(&h->pf_u, M * 2 * (size_t)c.d_ff * 2));
  HIPCHK(h, hipMalloc(&h->pf_m, M * (size_t)c.d_ff * 2));
  if (c.arch == 1) {
    HIPCHK(h, hipMalloc(&h->pf_res, M * c.d_model * 4));
    HIPCHK(h, hipMalloc(&h->pf_zx, M * (size_t)h->m_d_in_proj * 2));
    HIPCHK(h, hipMalloc(&h->pf_xbc, M * (size_t)h->m_conv_dim * 2));
    HIPCHK(h, hipMalloc(&h->pf_y, M * (size_t)c.m_d_inner * 2));
    HIPCHK(h, hipMalloc(&h->pf_g, M * (size_t)c.m_d_inner * 2));
  }
  h->pf_rows = M;
  return ZN_OK;
}

// FP8: the same launches reading the code cache a.kv8 (zn_prefill_attn_fp8_kernels.h) - the form prefill_attention chose by leaving a code cache in the arguments.
#define ZN_PA_LAUNCH(FP8, BF16, grid_) do { if (a.kv8) hipLaunchKernelGGL(FP8, grid_, dim3(256), 0, s, a); else hipLaunchKernelGGL(BF16, grid_, dim3(256), 0, s, a); } while (0)
template <int HD>
static int launch_prefill_attn(const PrefillAttnArgs& a, int G, int R, bool mfma, hipStream_t s) {
  if constexpr (HD == 128) {
    if (mfma) {   // both contractions on the matrix cores (same row semantics)
      dim3 grid((a.S + 64 / G - 1) / (64 / G), a.n_heads_kv, R);
      switch (G) {
        case 1: ZN_PA_LAUNCH((attn_prefill_mfma_fp8_kernel<1>), (attn_prefill_mfma_kernel<1>), grid); return 0;
        case 2: ZN_PA_LAUNCH((attn_prefill_mfma_fp8_kernel<2>), (attn_prefill_mfma_kernel<2>), grid); return 0;
        case 4: ZN_PA_LAUNCH((attn_prefill_mfma_fp8_kernel<4>), (attn_prefill_mfma_kernel<4>), grid); return 0;
        case 8: ZN_PA_LAUNCH((attn_prefill_mfma_fp8_kernel<8>), (attn_prefill_mfma_kernel<8>), grid); return 0;
      }
    }
  }
  switch (G) {
#define ZN_PA(GG) case GG: ZN_PA_LAUNCH((attn_prefill_fp8_kernel<HD, GG>), (attn_prefill_kernel<HD, GG>), dim3((a.S + 64 / GG - 1) / (64 / GG), a.n_heads_kv, R)); return 0;
    ZN_PA(1) ZN_PA(2) ZN_PA(4) ZN_PA(8)
#undef ZN_PA
  }
  return -1;
}
#undef ZN_PA_LAUNCH

static int qsplit(int S) { return S >= 768 ? 256 : S >= 192 ? 64 : 32; }   // query split of the CPU flash kernel

// All S positions at once: row-wise kernels over M = R*S rows, MFMA GEMMs, tiled exact causal attention.
// causal attention of S prefill positions over the keys already written for them (SDPA is_causal=True, _torch.py:415)
// row_len (device, [R]): right-padded rows, row r holds row_len[r] <= S positions; each row then takes the query split and key extents of its own length
// kv8: the code cache of `kv`, or NULL.  The form is chosen here: the FP8 kernels read kv8 exactly where there is no bf16 cache (kv == NULL: a codes-only generation,
// an admission's scratch cache of codes, zn_op_attn_prefill_rows_fp8); with both caches the bf16 kernels read kv, as before the codes-only mode existed.
static int prefill_attention(zn_handle h, const bf16_t* q, int ldq, const bf16_t* kv, int max_len, bf16_t* out, int ldo, int S, int R,
                             hipStream_t s, int base = 0, const int* row_len = nullptr, const uint8_t* kv8 = nullptr) {
  const zn_config& c = h->cfg;
  const int hd = h->hd;
  if (!kv && !kv8) ZN_FAIL(h, ZN_ERR_STATE, "prefill attention: neither a bf16 cache nor a code cache");
  PrefillAttnArgs pa{};
  pa.q = q; pa.ldq = ldq; pa.kv = kv; pa.kv8 = kv ? nullptr : kv8; pa.out = out; pa.ldo = ldo; pa.S = S; pa.base = base; pa.max_len = max_len;
  pa.n_heads = c.n_heads; pa.n_heads_kv = c.n_heads_kv; pa.qsplit = qsplit(S); pa.scale = (float)(1.0 / std::sqrt((double)hd));
  pa.row_len = row_len;
  const bool mfma = h->tune[ZN_TUNE_PREFILL_ATTN_VALU] != 2;   // 2: the VALU kernel at every head size
  int r2 = hd == 128 ? launch_prefill_attn<128>(pa, h->G, R, mfma, s) : hd == 64 ? launch_prefill_attn<64>(pa, h->G, R, mfma, s) : launch_prefill_attn<32>(pa, h->G, R, mfma, s);
  if (r2) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "prefill attention: unsupported group %d", h->G);
  return ZN_OK;
}

// Transformer blocks over all S positions of R rows (hidden [R][S][d]) with `base` keys already cached per row: the
// residual stream of every position ends in h->pf_x.  row_len (device, [R]; base 0 only): right-padded rows.  The row-wise kernels and the
// projections run over all R * S positions (pad rows are computed and dropped: no op mixes positions except the attention, which bounds
// every row by row_len[r]); RoPE and the KV append run over the pad positions too - cache slots at or past row_len[r], which the row's own
// decode steps overwrite, one per step, before the attention's extent reaches them.
// kv_round: the FP8 KV cache is in effect for these appends (rounded K/V into kv_layers); kv8_layers (may be NULL: an admission's scratch cache) receive the codes.
// kv_layers NULL or NULL entries (codes only): the appends write kv8_layers alone and the attention reads them.
static int transformer_prefill_core(zn_handle h, const bf16_t* hidden, int S, int R, const void* const* kv_layers, int max_len, int base, hipStream_t s,
                                    const int* row_len = nullptr, const void* const* kv8_layers = nullptr, bool kv_round = false) {
  const zn_config& c = h->cfg;
  const int M = R * S, d = c.d_model, hd = h->hd, nq = c.n_heads * hd, nkv = c.n_heads_kv * hd, nqkv = nq + 2 * nkv, F = c.d_ff;
  int rc = ensure_prefill_ws(h, (size_t)M);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->pf_x, hidden, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s));
  for (int li = 0; li < c.n_layer; ++li) {
    const zn_layer_weights& lw = h->layers[li];
    bf16_t* kv = kv_layers ? (bf16_t*)kv_layers[li] : nullptr;
    // short prompts (<= 64 rows): every projection streams its weights through a small-M kernel (10.7 -> ~2.5 ms per prefill); prefill_linear
    // (LayerNorm as gemm16k's prologue over four row groups: 22.0 us against 4.7 + 9 for the launch pair: 768 workgroups repeat the statistics)
    hipLaunchKernelGGL(layernorm_kernel, dim3(M), dim3(64), 0, s, h->pf_x, (const bf16_t*)lw.norm_w, (const bf16_t*)lw.norm_b, h->pf_n, d, c.norm_eps);
    GemvArgs g = linear_args(h, lw.in_proj, nqkv, d, h->pf_n, h->pf_qkv, nullptr);
    g.hd = hd; g.n_heads = c.n_heads; g.n_heads_kv = c.n_heads_kv; g.q_out = h->pf_qkv; g.kv = kv; g.rope = h->rope; g.max_len = max_len;
    g.rope_positions = c.rope_positions; g.pf_S = S; g.pf_base = base;
    g.kv8 = kv8_layers ? (uint8_t*)const_cast<void*>(kv8_layers[li]) : nullptr; g.kv_round = kv_round ? 1 : 0;
    bool rope_done = false;
    if ((rc = prefill_linear<EPI_ROPE_KV>(h, g, M, s, true, &rope_done))) return rc;
    if (!rope_done) hipLaunchKernelGGL(rope_kv_rows_kernel, dim3(S, R), dim3(256), 0, s, h->pf_qkv, kv, h->rope, S, base, max_len, c.n_heads, c.n_heads_kv, hd, c.rope_positions, g.kv8, g.kv_round);
    rc = prefill_attention(h, h->pf_qkv, rope_done ? nq : nqkv, kv, max_len, h->pf_a, nq, S, R, s, base, row_len, g.kv8);
    if (rc) return rc;
    if (c.double_out_proj && (rc = prefill_linear<EPI_STORE>(h, linear_args(h, lw.out_proj, d, nq, h->pf_a, h->pf_n, nullptr), M, s))) return rc;
    if ((rc = prefill_linear<EPI_RESID>(h, linear_args(h, lw.out_proj, d, nq, c.double_out_proj ? h->pf_n : h->pf_a, h->pf_x, h->pf_x), M, s))) return rc;
    hipLaunchKernelGGL(layernorm_kernel, dim3(M), dim3(64), 0, s, h->pf_x, (const bf16_t*)lw.norm2_w, (const bf16_t*)lw.norm2_b, h->pf_n, d, c.norm_eps);
    if ((rc = prefill_linear<EPI_SILU>(h, linear_args(h, lw.fc1, 2 * F, d, h->pf_n, h->pf_m, nullptr), M, s, false))) return rc;
    if ((rc = prefill_linear<EPI_RESID>(h, linear_args(h, lw.fc2, d, F, h->pf_m, h->pf_x, h->pf_x), M, s, false))) return rc;
  }
  return ZN_OK;
}

static int prefill_batched(zn_handle h, const bf16_t* hidden, int S, hipStream_t s, const int* row_len) {
  const zn_config& c = h->cfg;
  const int R = h->gen.rows, d = c.d_model;
  int rc = transformer_prefill_core(h, hidden, S, R, h->gen.kv_layers.data(), h->gen.max_len, 0, s, row_len, kv_fp8_gen(h) ? h->gen.kv8_layers.data() : nullptr, kv_fp8_gen(h));
  if (rc) return rc;
  hipLaunchKernelGGL(gather_last_kernel, dim3(R), dim3(256), 0, s, h->pf_x, h->x, S, d, row_len);
  hipLaunchKernelGGL(add_lengths_kernel, dim3(1), dim3(64 > R ? 64 : R), 0, s, h->gen.lengths, R, S, row_len);
  return ZN_OK;
}

// A projection over M rows of the hybrid prefill: out [M][N] = A [M][K] W^T (+ bias).  exact: row by row through the decode
// step's GEMV (same summation order as a single step: lets tests compare a prefill with single steps bit for bit).
static int proj_rows(zn_handle h, const bf16_t* A, int lda, const void* W, const void* bias, bf16_t* out, int ldo, int M, int N, int K, bool exact,
                     hipStream_t s) {
  if (exact) {
    for (int m = 0; m < M; ++m) {
      GemvArgs g{};
      g.W = (const bf16_t*)W; g.N = N; g.K = K; g.x = A + (size_t)m * lda; g.out = out + (size_t)m * ldo; g.bias = (const bf16_t*)bias;
      int rc = run_gemv<PRO_NONE, EPI_STORE>(h, g, 1, h->tune[ZN_TUNE_WG_OUT_PROJ], s);
      if (rc) return rc;
    }
    return ZN_OK;
  }
  launch_gemm(A, lda, (const bf16_t*)W, out, ldo, nullptr, M, N, K, s, (const bf16_t*)bias);
  return ZN_OK;
}

// Hybrid blocks over all S positions of R rows (mamba_ssm Block semantics): Mamba2 layers run the sequence conv and the
// selective scan (zn_mamba_kernels.h), attention layers the batched projections + tiled causal attention.  The mixer
// output of every position ends in h->pf_x, the residual stream in h->pf_res; caches advance by S positions.
// row_len (device, [R]; base 0 only): right-padded rows - the sequence conv and the scan stop at row_len[r], the attention bounds row r by it.
static int hybrid_prefill_core(zn_handle h, const bf16_t* hidden, int S, int R, const void* const* caches, int max_len, int base, bool exact,
                               hipStream_t s, const int* row_len = nullptr) {
  const zn_config& c = h->cfg;
  const int M = R * S, d = c.d_model, hd = h->hd, nq = c.n_heads * hd, nkv = c.n_heads_kv * hd, nqkv = nq + 2 * nkv, F = c.d_ff;
  int rc = ensure_prefill_ws(h, (size_t)M);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->pf_x, hidden, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s));
  for (int li = 0; li < c.n_layer; ++li) {
    const zn_layer_weights& lw = h->layers[li];
    launch_add_ln(h, h->pf_x, h->pf_res, li > 0, 1, lw.norm_w, lw.norm_b, h->pf_n, M, s);
    if (lw.kind == 1) {
      if ((rc = proj_rows(h, h->pf_n, d, lw.m_in_proj, nullptr, h->pf_zx, h->m_d_in_proj, M, h->m_d_in_proj, d, exact, s))) return rc;
      size_t conv_bytes = 0;
      (void)zn_mamba_state_bytes_per_layer(&c, R, &conv_bytes);
      MambaArgs m{};
      m.zx = h->pf_zx; m.conv_state = (bf16_t*)caches[li]; m.ssm_state = (bf16_t*)((char*)caches[li] + conv_bytes);
      m.conv_w = (const bf16_t*)lw.m_conv_w; m.conv_b = (const bf16_t*)lw.m_conv_b;
      m.dt_bias = (const bf16_t*)lw.m_dt_bias; m.A_log = (const bf16_t*)lw.m_A_log; m.D = (const bf16_t*)lw.m_D;
      m.norm_w = (const bf16_t*)lw.m_norm_w; m.xbc = h->pf_xbc; m.y = h->pf_y; m.g = h->pf_g; m.vg = nullptr;
      m.d_inner = c.m_d_inner; m.conv_dim = h->m_conv_dim; m.nheads = h->m_nheads; m.d_state = c.m_d_state; m.ngroups = c.m_ngroups;
      m.d_in_proj = h->m_d_in_proj; m.eps = c.norm_eps; m.rows = R;
      hipLaunchKernelGGL(mamba_conv_seq_kernel, dim3((h->m_conv_dim + 255) / 256, R), dim3(256), 0, s, m, S, row_len);
      if (c.m_d_state == 128) hipLaunchKernelGGL((mamba_scan_kernel<128>), dim3(h->m_nheads, R), dim3(256), 0, s, m, S, row_len);
      else hipLaunchKernelGGL((mamba_scan_kernel<64>), dim3(h->m_nheads, R), dim3(256), 0, s, m, S, row_len);
      m.rows = M;
      hipLaunchKernelGGL(mamba_gated_norm_kernel, dim3(c.m_ngroups, M), dim3(256), 0, s, m);
      if ((rc = proj_rows(h, h->pf_g, c.m_d_inner, lw.m_out_proj, nullptr, h->pf_x, d, M, d, c.m_d_inner, exact, s))) return rc;
      continue;
    }
    bf16_t* kv = (bf16_t*)caches[li];
    if ((rc = proj_rows(h, h->pf_n, d, lw.in_proj, lw.in_proj_bias, h->pf_qkv, nqkv, M, nqkv, d, exact, s))) return rc;
    hipLaunchKernelGGL(rope_kv_any_kernel, dim3(S, R), dim3(256), 0, s, h->pf_qkv, h->pf_qkv, nqkv, kv, h->rope, S, base, (const int*)nullptr, max_len,
                       c.n_heads, c.n_heads_kv, hd, c.rope_positions, c.rope_mode);
    if ((rc = prefill_attention(h, h->pf_qkv, nqkv, kv, max_len, h->pf_a, nq, S, R, s, base, row_len))) return rc;
    if ((rc = proj_rows(h, h->pf_a, nq, lw.out_proj, lw.out_proj_bias, h->pf_x, d, M, d, nq, exact, s))) return rc;
    launch_add_ln(h, h->pf_x, h->pf_res, 1, 1, lw.norm2_w, lw.norm2_b, h->pf_n, M, s);
    if ((rc = proj_rows(h, h->pf_n, d, lw.fc1, nullptr, h->pf_u, 2 * F, M, 2 * F, d, exact, s))) return rc;
    hipLaunchKernelGGL(silu_mul_rows_kernel, dim3(M), dim3(256), 0, s, h->pf_u, h->pf_m, F);
    if ((rc = proj_rows(h, h->pf_m, F, lw.fc2, nullptr, h->pf_x, d, M, d, F, exact, s))) return rc;
  }
  return ZN_OK;
}

extern "C" int zn_debug_prefill_mode(zn_handle h, int32_t mode) { if (!h) return ZN_ERR_ARG; h->prefill_mode = mode; return ZN_OK; }

// All S positions at once (true), or position by position through the decode kernels (prefill_mode 0, S = 1, dimensions the batched kernels do not tile)?
static bool prefill_all_at_once(zn_handle h, int S) {
  const zn_config& c = h->cfg;
  if (S <= 1 || c.d_model % 32 || c.d_ff % 32) return false;
  return c.arch == 1 ? (h->prefill_mode >= 1 && c.m_d_inner % 32 == 0) : h->prefill_mode == 1;
}

// The prefill of S positions per row; row_len (device, [rows]) != nullptr: right-padded rows of row_len[r] <= S valid positions (batched prefill only).
static int prefill_impl(zn_handle h, const void* hidden_dev, int32_t S, const int* row_len, hipStream_t s) {
  const zn_config& c = h->cfg;
  int rc;
  const bool at_once = prefill_all_at_once(h, S);
  if (c.arch == 1 && at_once) {
    // all positions at once (mode 2: projections row by row through the step's GEMV: bit-comparable with single steps)
    if ((rc = hybrid_prefill_core(h, (const bf16_t*)hidden_dev, S, h->gen.rows, h->gen.kv_layers.data(), h->gen.max_len, 0, h->prefill_mode == 2, s, row_len))) return rc;
    hipLaunchKernelGGL(gather_last_kernel, dim3(h->gen.rows), dim3(256), 0, s, h->pf_x, h->x, S, c.d_model, row_len);
    hipLaunchKernelGGL(gather_last_bytes_kernel, dim3(h->gen.rows), dim3(256), 0, s, (const void*)h->pf_res, (void*)h->res, S, c.d_model * (c.residual_in_fp32 ? 4 : 2), row_len);
    hipLaunchKernelGGL(add_lengths_kernel, dim3(1), dim3(64 > h->gen.rows ? 64 : h->gen.rows), 0, s, h->gen.lengths, h->gen.rows, S, row_len);
    h->gen.len_hi += S;
    if ((rc = hybrid_heads(h, s))) return rc;
  } else if (c.arch == 0 && at_once) {
    if ((rc = prefill_batched(h, (const bf16_t*)hidden_dev, S, s, row_len))) return rc;
    h->gen.len_hi += S;
  } else {
    // Position by position through the decode kernels.  Row-wise ops are independent of S; attention reproduces the
    // reference's causal flash-attention blocking through `ext` = keys spanned by the query block of this position.
    const int qb = qsplit(S);
    for (int p = 0; p < S; ++p) {
      hipLaunchKernelGGL(gather_pos_kernel, dim3(h->gen.rows), dim3(256), 0, s, (const bf16_t*)hidden_dev, h->x, S, p, c.d_model);
      int ext = (p / qb) * qb + qb; if (ext > S) ext = S;
      const StepPlan plan = plan_blocks(h, h->gen.rows, ++h->gen.len_hi);
      if ((rc = c.arch == 1 ? hybrid_token(h, p == S - 1, plan.attn_fused, s) : decode_blocks(h, plan, nullptr, ext, s))) return rc;
      hipLaunchKernelGGL(add_lengths_kernel, dim3(1), dim3(64 > h->gen.rows ? 64 : h->gen.rows), 0, s, h->gen.lengths, h->gen.rows, 1);
    }
  }
  if (c.arch == 0 && (rc = heads_logits(h, h->x, h->gen.rows, s))) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_prefill(zn_handle h, const void* hidden_dev, int32_t S, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_PREFILL));
  if (!hidden_dev || S < 1 || S > h->gen.max_len) ZN_FAIL(h, ZN_ERR_ARG, "zn_prefill: bad S=%d (max_len %d)", S, h->gen.max_len);
  if (int rc = kv_fp8_bound(h, "zn_prefill")) return rc;
  h->gen.gen_prefilled = true;
  return prefill_impl(h, hidden_dev, S, nullptr, (hipStream_t)stream);
}

extern "C" int zn_prefill_rows(zn_handle h, const void* hidden_dev, int32_t S, const int32_t* row_len, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_PREFILL_ROWS));
  if (!hidden_dev || !row_len || S < 1 || S > h->gen.max_len) ZN_FAIL(h, ZN_ERR_ARG, "zn_prefill_rows: null argument or bad S=%d (max_len %d)", S, h->gen.max_len);
  if (int rc = kv_fp8_bound(h, "zn_prefill_rows")) return rc;
  const int R = h->gen.rows;
  bool uniform, unequal2;
  ZN_GEN_CHECK(h, gen_check_prefill_rows(h->gen, row_len, S, &uniform, &unequal2));
  hipStream_t s = (hipStream_t)stream;
  h->gen.gen_prefilled = true;
  if (uniform) return prefill_impl(h, hidden_dev, S, nullptr, s);          // zn_prefill: the same launches, the same bits
  if (!prefill_all_at_once(h, S))
    ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_prefill_rows: rows of different lengths need the batched prefill; this handle prefills position by position "
            "(zn_debug_prefill_mode 0, S = 1, or dimensions that are not multiples of 32)");
  h->row_len_host.assign(row_len, row_len + R);
  HIPCHK(h, hipMemcpyAsync(h->row_len, h->row_len_host.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
  h->gen.rows_unequal2 = unequal2;
  return prefill_impl(h, hidden_dev, S, h->row_len, s);                     // len_hi += S: the bound of the longest row
}

extern "C" int zn_gen_set_rows(zn_handle h, const zn_row_params* rows_host, int32_t n) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_ROWS));
  std::vector<int> rem;
  bool pairs;
  ZN_GEN_CHECK(h, gen_check_set_rows(h->gen, h->cfg.n_codebooks, rows_host, n, &rem, &pairs));
  hipStream_t s = h->gen_stream;
  HIPCHK(h, hipMemcpyAsync(h->row_tab, rows_host, (size_t)n * sizeof(zn_row_params), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->remaining, rem.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));  // the host arrays are the caller's / go out of scope
  h->gen.rows_set = true;
  h->gen.pairs_set = pairs;
  return ZN_OK;
}

extern "C" int zn_gen_set_prefix_rows(zn_handle h, const int32_t* prefix_len_host, int32_t n) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_PREFIX_ROWS));
  std::vector<int> shift;
  bool any;
  ZN_GEN_CHECK(h, gen_check_prefix_rows(h->gen, prefix_len_host, n, &shift, &any));
  if (any) {
    hipStream_t s = h->gen_stream;
    HIPCHK(h, hipMemcpyAsync(h->prefix_shift, shift.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));  // the host vector goes out of scope
  }
  h->gen.prefix_set = any;                  // every shift 0: the kernels keep their NULL branch (the same launches, the same bits)
  return ZN_OK;
}

// ------------------------------------------------------------------------------------------------ slotted session
static int handoff_timeout(zn_handle h, int count);

extern "C" int zn_gen_open_slots(zn_handle h, int32_t slack) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_OPEN_SLOTS));
  ZN_GEN_CHECK(h, gen_check_open_slots(h->gen, slack));
  const size_t R = h->max_rows;
  if (!h->step0) HIPCHK(h, hipMalloc(&h->step0, R * sizeof(int)));
  if (!h->adm_stage) HIPCHK(h, hipHostMalloc(&h->adm_stage, R * (4 * sizeof(int) + sizeof(zn_row_params))));
  if (!h->adm_dev) HIPCHK(h, hipMalloc(&h->adm_dev, R * (4 * sizeof(int) + sizeof(zn_row_params))));
  if (!h->adm_layers) HIPCHK(h, hipMalloc(&h->adm_layers, (size_t)h->cfg.n_layer * sizeof(AdmitLayer)));
  if (!h->adm_event) HIPCHK(h, hipEventCreateWithFlags(&h->adm_event, hipEventDisableTiming));
  hipStream_t s = h->gen_stream;
  const int B = h->gen.batch;
  HIPCHK(h, hipMemsetAsync(h->remaining, 0, B * sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->stopping, 0, B * sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->prefix_shift, 0, B * sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->step0, 0xFF, B * sizeof(int), s));                     // -1: idle
  HIPCHK(h, hipMemsetAsync(h->row_tab, 0, (size_t)B * sizeof(zn_row_params), s));    // an idle slot samples greedily, without a penalty
  h->adm_cap_S = 0;                        // the pointer table names this generation's caches: rebuilt by the first admission
  h->gen.open_slots(slack);
  return ZN_OK;
}

// The scratch cache of an admission: n_layer buffers for max_rows rows of S positions (attention) or of Mamba2 state, and the table that pairs
// each with the session's buffer.  Grows with S; the stream is drained before a buffer an earlier admission may still read is freed.
static int ensure_admit_cache(zn_handle h, int S, hipStream_t s) {
  if (S <= h->adm_cap_S) return ZN_OK;
  const zn_config& c = h->cfg;
  const int cap = ((S + 63) / 64) * 64;
  const bool codes_only = kv_codes_only_gen(h);      // the scratch cache holds codes: half the bytes
  const size_t attn = codes_only ? zn_kv_fp8_bytes_per_layer(&c, h->max_rows, cap) : zn_kv_bytes_per_layer(&c, h->max_rows, cap), mamba = zn_mamba_state_bytes_per_layer(&c, h->max_rows, nullptr);
  const size_t per = ((attn > mamba ? attn : mamba) + 255) / 256 * 256;
  if (per > h->adm_layer_bytes) {
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->adm_cache) { (void)hipFree(h->adm_cache); h->adm_cache = nullptr; h->adm_layer_bytes = 0; }
    HIPCHK(h, hipMalloc(&h->adm_cache, per * c.n_layer));
    h->adm_layer_bytes = per;
  }
  std::vector<AdmitLayer> tab(c.n_layer);
  h->adm_caches.resize(c.n_layer);
  for (int li = 0; li < c.n_layer; ++li) {
    h->adm_caches[li] = (char*)h->adm_cache + (size_t)li * h->adm_layer_bytes;
    tab[li] = AdmitLayer{h->adm_caches[li], const_cast<void*>(h->gen.kv_layers[li]), (c.arch == 1 && h->layers[li].kind == 1) ? 1 : 0, codes_only ? 1 : 0, kv8_of(h, li)};
  }
  HIPCHK(h, hipMemcpyAsync(h->adm_layers, tab.data(), tab.size() * sizeof(AdmitLayer), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));      // the host vector goes out of scope
  h->adm_cap_S = cap;
  return ZN_OK;
}

extern "C" int zn_gen_admit(zn_handle h, const zn_admit* a, int32_t n, const void* hidden_dev, int32_t S, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_ADMIT));
  const zn_config& c = h->cfg;
  const int B = h->gen.batch, halves = guided(h) ? 2 : 1, nq = c.n_codebooks, MR = h->max_rows;
  ZN_GEN_CHECK(h, gen_check_admit_call(h->gen, a && hidden_dev, n, S));
  if (int rc = kv_fp8_bound(h, "zn_gen_admit")) return rc;
  bool uniform;
  ZN_GEN_CHECK(h, gen_check_admit(h->gen, nq, a, n, S, &uniform));
  if (!prefill_all_at_once(h, S))
    ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_gen_admit needs the batched prefill; this handle prefills position by position (zn_debug_prefill_mode 0, S = 1, or dimensions that are not multiples of 32)");
  hipStream_t s = (hipStream_t)stream;
  h->gen_stream = s;
  int rc = ensure_admit_cache(h, S, s);
  if (rc) return rc;
  // stage the admission's arguments: one pinned buffer, one copy
  if (h->adm_pending) { HIPCHK(h, hipEventSynchronize(h->adm_event)); h->adm_pending = false; }
  const int Rs = n * halves;
  int* w = (int*)h->adm_stage;
  zn_row_params* pw = (zn_row_params*)(h->adm_stage + (size_t)MR * 4 * sizeof(int));
  for (int j = 0; j < n; ++j) {
    w[j] = a[j].slot; w[MR + j] = a[j].prefix_len; w[2 * MR + j] = a[j].params.max_new_tokens + nq - 1;
    for (int hf = 0; hf < halves; ++hf) w[3 * MR + hf * n + j] = a[j].row_len;
    pw[j] = a[j].params;
  }
  HIPCHK(h, hipMemcpyAsync(h->adm_dev, h->adm_stage, (size_t)MR * (4 * sizeof(int) + sizeof(zn_row_params)), hipMemcpyHostToDevice, s));
  const int* dv = (const int*)h->adm_dev;
  const int* row_len_dev = uniform ? nullptr : dv + 3 * MR;           // every length S: zn_prefill's launches, as zn_prefill_rows makes them
  h->gen.gen_prefilled = true;
  size_t conv_src = 0, conv_dst = 0;
  if (c.arch == 1) {
    (void)zn_mamba_state_bytes_per_layer(&c, Rs, &conv_src);
    const size_t state = zn_mamba_state_bytes_per_layer(&c, h->gen.rows, &conv_dst);
    (void)state;
    const size_t zb = zn_mamba_state_bytes_per_layer(&c, Rs, nullptr);
    for (int li = 0; li < c.n_layer; ++li)                               // a prefill continues the state it finds: the scratch rows begin at zero
      if (h->layers[li].kind == 1) HIPCHK(h, hipMemsetAsync(const_cast<void*>(h->adm_caches[li]), 0, zb, s));
    if ((rc = hybrid_prefill_core(h, (const bf16_t*)hidden_dev, S, Rs, h->adm_caches.data(), S, 0, h->prefill_mode == 2, s, row_len_dev))) return rc;
  } else if (kv_codes_only_gen(h)) {       // codes only: the scratch cache holds codes, which admit_rows_kernel copies as they are
    if ((rc = transformer_prefill_core(h, (const bf16_t*)hidden_dev, S, Rs, nullptr, S, 0, s, row_len_dev, h->adm_caches.data(), true))) return rc;
  } else if ((rc = transformer_prefill_core(h, (const bf16_t*)hidden_dev, S, Rs, h->adm_caches.data(), S, 0, s, row_len_dev, nullptr, kv_fp8_gen(h)))) return rc;   // (FP8 KV cache: the scratch rows are rounded, admit_rows_kernel writes their codes)
  AdmitArgs m{};
  m.layers = h->adm_layers; m.n_layer = c.n_layer; m.n = n; m.halves = halves; m.B = B; m.S = S; m.max_len = h->gen.max_len;
  m.kv_row_bytes = 2 * c.n_heads_kv * h->hd * 2;
  if (c.arch == 1) {
    m.conv_row_bytes = h->m_conv_dim * c.m_d_conv * 2; m.ssm_row_bytes = c.m_d_inner * c.m_d_state * 2; m.ssm_off_src = conv_src; m.ssm_off_dst = conv_dst;
    m.pf_res = h->pf_res; m.res = h->res; m.res_row_bytes = c.d_model * (c.residual_in_fp32 ? 4 : 2);
  }
  m.slot = dv; m.prefix = dv + MR; m.rem = dv + 2 * MR; m.row_len = dv + 3 * MR; m.params = (const zn_row_params*)(h->adm_dev + (size_t)MR * 4 * sizeof(int));
  m.pf_x = h->pf_x; m.x = h->x; m.d = c.d_model; m.st = h->st;
  m.lengths = h->gen.lengths; m.remaining = h->remaining; m.stopping = h->stopping; m.shift = h->prefix_shift; m.step0 = h->step0; m.rows = h->row_tab;
  hipLaunchKernelGGL(admit_rows_kernel, dim3(Rs, c.n_layer + 1, ZN_ADMIT_PARTS), dim3(256), 0, s, m);
  HIPCHK(h, hipEventRecord(h->adm_event, s));
  h->adm_pending = true;
  // the heads over every row of h->x, as a prefill of the whole batch runs them (the logits of the rows not admitted are workspace: the next
  // step's heads rewrite them before any sampler reads them), then the first frame of each admitted slot alone
  if ((rc = c.arch == 1 ? hybrid_heads(h, s) : heads_logits(h, h->x, h->gen.rows, s))) return rc;
  for (int j = 0; j < n; ++j) launch_first_frame(h, a[j].slot, s);
  h->gen.slots_admitted(a, n);
  h->gen.emb_valid = false;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_gen_retire(zn_handle h, int32_t slot) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_RETIRE));
  ZN_GEN_CHECK(h, gen_check_retire(h->gen, slot));
  hipStream_t s = h->gen_stream;
  HIPCHK(h, hipMemsetAsync(h->gen.lengths + slot, 0, sizeof(int), s));
  if (guided(h)) HIPCHK(h, hipMemsetAsync(h->gen.lengths + h->gen.batch + slot, 0, sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->remaining + slot, 0, sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->step0 + slot, 0xFF, sizeof(int), s));
  h->gen.slot_retired(slot);
  return ZN_OK;
}

extern "C" int zn_gen_row_state(zn_handle h, int32_t* remaining_host, int32_t* steps_host, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_ROW_STATE));
  hipStream_t s = (hipStream_t)stream;
  const int B = h->gen.batch;
  std::vector<int> rem(B), s0(B);
  GenState st{};
  HIPCHK(h, hipMemcpyAsync(rem.data(), h->remaining, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(s0.data(), h->step0, B * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&st, h->st, sizeof st, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b) {
    if (remaining_host) remaining_host[b] = rem[b];
    if (steps_host) steps_host[b] = s0[b] < 0 ? -1 : st.step - s0[b];
  }
  if (st.pad[0] != 0) return handoff_timeout(h, st.pad[0]);
  return ZN_OK;
}

extern "C" int zn_sample_first(zn_handle h, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SAMPLE_FIRST));
  launch_first_frame(h, -1, (hipStream_t)stream);
  h->gen.emb_valid = false;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_decode_steps(zn_handle h, int32_t n, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_DECODE_STEPS));
  if (n < 0) ZN_FAIL(h, ZN_ERR_ARG, "n < 0");
  hipStream_t s = (hipStream_t)stream;
  h->gen_stream = s;
  if (int rc = kv_fp8_bound(h, "zn_decode_steps")) return rc;
  ZN_GEN_CHECK(h, gen_check_steps(h->gen, n));
  for (int i = 0; i < n;) {
    const StepPlan p = h->last_plan = plan_steps(h, n - i);
    const int k = p.graph_slot, run = p.run;
    // steps with the fused tail read the embedding their predecessor's tail left: the first of them gets it from embed_kernel; steps
    // without it (one row off the whole-step kernel) embed into h->x themselves and leave x_emb stale
    if (p.fused_tail && !h->gen.emb_valid) hipLaunchKernelGGL(embed_kernel, dim3(h->gen.batch), dim3(256), 0, s, make_embed_args(h));
    h->gen.emb_valid = p.fused_tail;
    if (!h->graph_exec[k] && !h->graph_tried[k] && n > 1) {
      // capture; every step-varying quantity (column, positions) is read from device memory
      h->graph_tried[k] = true;
      // capture on an internal stream: the caller's stream may be the legacy null stream, which cannot be captured
      if (!h->cap_stream) (void)hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
      hipStream_t cs = h->cap_stream; std::unique_lock<std::mutex> capturing(g_capture_mu);
      if (cs && hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        int rc = ZN_OK;
        for (int j = 0; j < run && rc == ZN_OK; ++j) rc = enqueue_step(h, p, cs);
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(cs, &g); capturing.unlock();
        if (rc == ZN_OK && e == hipSuccess && g && hipGraphInstantiate(&h->graph_exec[k], g, nullptr, nullptr, 0) == hipSuccess) h->graph[k] = g;
        else { if (g) (void)hipGraphDestroy(g); h->graph_exec[k] = nullptr; (void)hipGetLastError(); }
      } else (void)hipGetLastError();
    }
    if (h->graph_exec[k]) HIPCHK(h, hipGraphLaunch(h->graph_exec[k], s));
    else for (int j = 0; j < run; ++j) { int rc = enqueue_step(h, p, s); if (rc) return rc; }
    i += run; h->gen.len_hi += run; h->epoch_bound += (unsigned long long)run * (h->cfg.n_layer + 1);
  }
  if (h->gen.slots_open) h->gen.slots_advance(n);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_gen_end(zn_handle h) {
  if (!h) return ZN_ERR_ARG;
  (void)zn_tenant_release(h->device, h);
  if (h->gen.gen_active && !h->gen.gen_ended && h->demoted && !h->gen.gen_timed_out) h->clean_since_demotion++;
  h->gen.gen_ended = true;
  return ZN_OK;
}

// [0] hand-off timeouts reported on this handle, [1] generations begun, [2] of those, batch-1 generations that ran the launches path because an
// earlier timeout had demoted the handle, [3] 1 while demoted, [4] times the handle was re-armed, [5] clean generations since the demotion,
// [6] the longest in-kernel hand-off wait any whole-step launch of this handle measured, in microseconds (0: none beyond 0.1 ms), [7] waits
// beyond 0.2 ms (a pause of the device shows up as one such wait per waiting wave).  Reading [6], [7] synchronises with the device.
extern "C" int zn_get_counters(zn_handle h, int64_t* out, int32_t n) {
  if (!h || !out || n < 0) return ZN_ERR_ARG;
  unsigned w[2] = {0, 0};
  if (n > 6 && h->ch_diag) HIPCHK(h, ZN_NOT_IN_CAPTURE(hipMemcpy(w, h->ch_diag + 8, sizeof w, hipMemcpyDeviceToHost)));
  const long long v[8] = {h->n_timeouts, h->n_generations, h->n_fallback_generations, h->demoted ? 1 : 0, h->n_rearms, h->clean_since_demotion, (long long)(w[0] / 100u), (long long)w[1]};
  for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
  return ZN_OK;
}

extern "C" int zn_decode_path_detail(zn_handle h) {
  if (!h || !h->gen.gen_active || h->cfg.arch != 0 || !persist_active(h, h->gen.rows)) return 0;
  // which persistent kernel: the last plan's; whether one is still allowed: asked now (a timeout reported since demotes at once).  One row: 2 or 0
  return h->last_plan.path == StepPlan::STACK ? 2 : chain_allowed(h, h->gen.rows) ? 1 : 0;
}
extern "C" int zn_decode_path(zn_handle h) { return zn_decode_path_detail(h) != 0 ? 1 : 0; }
extern "C" int zn_graph_active(zn_handle h) {
  if (!h) return 0;
  for (int k = 0; k < ZN_NGRAPHS; ++k) if (h->graph_exec[k]) return 1;
  return 0;
}

// A bounded hand-off wait of the persistent kernels gave up (sweep_granules): the generation's results are void.  The message names the
// wait (stage: 1 y1, 2 x1, 3 m, 4 x2, 5 q|k|v, 6 attention output, 7 block maxima and 8 partials of the key-block attention role; block; workgroup; wave; the tag waited for and the first stale granule),
// the handle falls back to one launch per op (no in-launch hand-offs) for its later generations, and the sticky word is cleared so
// that a new generation can run.
static int handoff_timeout(zn_handle h, int count) {
  // zn_all_stopped_end only waited for the stop event: in deferred mode up to 16 further steps (graph launches) may still be queued behind
  // it.  Drain the generation's stream before the diagnostic words are read and cleared and before the graphs those steps run from are
  // destroyed (on a non-blocking stream the null-stream copies below would not wait for them).
  if (h->gen_stream) (void)hipStreamSynchronize(h->gen_stream);
  (void)ZN_NOT_IN_CAPTURE(hipMemcpy(h->diag_host, h->ch_diag, sizeof h->diag_host, hipMemcpyDeviceToHost));
  (void)ZN_NOT_IN_CAPTURE(hipMemset(h->ch_diag, 0, 32));                   // (the wait statistics in words 8, 9 stay)
  (void)ZN_NOT_IN_CAPTURE(hipMemset(&h->st->pad[0], 0, sizeof(int)));
  h->demoted = true; h->clean_since_demotion = 0; h->n_timeouts++; h->gen.gen_timed_out = true;
  free_graph(h);
  const unsigned* d = h->diag_host;
  ZN_FAIL(h, ZN_ERR_HIP, "decode chain: %d hand-off wait(s) timed out - the results of this generation are invalid. First: stage %u of block %u, workgroup %u wave %u lane %u "
          "waited for tag %u, granule at byte %u carried tag %u after %u passes. This handle runs the launches path for its next %d generations (zn_debug_tune(8, 1) re-arms the persistent kernels at once; zn_get_counters)",
          count, d[0] >> 8, d[0] & 255u, d[1], d[2], d[6], d[3], d[4], d[5], d[7], ZN_REARM_AFTER);
}

extern "C" int zn_all_stopped(zn_handle h, int32_t* out, zn_stream stream) {
  if (!h || !out) return ZN_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // all_done, force_eos_step, eos_bias, pad[0] = the persistent chain's sticky timeout word: one 16-byte copy
  HIPCHK(h, hipMemcpyAsync(h->done_host, &h->st->all_done, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  *out = h->done_host[0];
  if (h->done_host[3] != 0) return handoff_timeout(h, h->done_host[3]);
  return ZN_OK;
}

// The stop check without a host round trip on the critical path: *_begin queues the copy of the loop state behind the steps
// enqueued so far, the caller enqueues the next steps, *_end (one batch later) waits for the copy - long done by then.
extern "C" int zn_all_stopped_begin(zn_handle h, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, hipMemcpyAsync(h->done_host + 4, &h->st->all_done, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipEventRecord(h->stop_event, s));
  h->gen.stop_pending = true;
  return ZN_OK;
}
extern "C" int zn_all_stopped_end(zn_handle h, int32_t* out) {
  if (!h || !out) return ZN_ERR_ARG;
  if (!h->gen.stop_pending) ZN_FAIL(h, ZN_ERR_STATE, "zn_all_stopped_end without zn_all_stopped_begin");
  HIPCHK(h, hipEventSynchronize(h->stop_event));
  h->gen.stop_pending = false;
  *out = h->done_host[4];
  if (h->done_host[7] != 0) return handoff_timeout(h, h->done_host[7]);
  return ZN_OK;
}

extern "C" int zn_get_step_outputs(zn_handle h, float* logits_dev, int32_t* tokens_dev, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const zn_config& c = h->cfg;
  if (logits_dev) HIPCHK(h, hipMemcpyAsync(logits_dev, h->last_logits, (size_t)h->gen.batch * c.n_codebooks * c.vocab_head * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (tokens_dev) HIPCHK(h, hipMemcpyAsync(tokens_dev, h->tok_raw, (size_t)h->gen.batch * c.n_codebooks * sizeof(int), hipMemcpyDeviceToDevice, s));
  return ZN_OK;
}

extern "C" int zn_codes_changed(zn_handle h) { if (!h) return ZN_ERR_ARG; h->gen.emb_valid = false; return ZN_OK; }
extern "C" int zn_debug_force_eos(zn_handle h, int32_t step) { if (!h) return ZN_ERR_ARG; h->force_eos_step = step; return ZN_OK; }
extern "C" int zn_debug_token_override(zn_handle h, const int32_t* tokens_dev, int32_t calls) {
  if (!h) return ZN_ERR_ARG;
  h->tok_override = tokens_dev; h->tok_override_calls = tokens_dev ? calls : 0;
  free_graph(h);
  return ZN_OK;
}
extern "C" int zn_debug_tune(zn_handle h, int32_t key, int32_t value) {
  if (!h || key < 0 || key >= ZN_TUNE_NKEYS || value < 1) return ZN_ERR_ARG;
  if (key == ZN_TUNE_HOOK && value == ZN_HOOK_RESET_WAIT_STATS) {   // observation hook: forget the wait statistics (zn_get_counters [6], [7]) gathered so far
    if (h->ch_diag) { (void)hipDeviceSynchronize(); (void)ZN_NOT_IN_CAPTURE(hipMemset(h->ch_diag + 8, 0, 2 * sizeof(unsigned))); }
    return ZN_OK;
  }
  (key == ZN_TUNE_HOOK ? h->pending_hook : h->tune[key]) = value; free_graph(h); h->gen.emb_valid = false;      // (a hook waits for zn_gen_begin)
  if (key == ZN_TUNE_PERSISTENT && value == 1 && h->demoted) { h->demoted = false; h->clean_since_demotion = 0; h->n_rearms++; }
  return ZN_OK;
}
extern "C" int zn_debug_trace(zn_handle h, void* trace_dev) {
  if (!h) return ZN_ERR_ARG;
  h->dbg_trace = (bf16_t*)trace_dev; free_graph(h);
  return ZN_OK;
}
extern "C" int zn_debug_chain_stamps(zn_handle h, uint64_t* stamps_dev) {
  if (!h) return ZN_ERR_ARG;
  h->ch_stamps = (unsigned long long*)stamps_dev; free_graph(h);
  return ZN_OK;
}
extern "C" int zn_debug_eos_bias(zn_handle h, float bias) { if (!h) return ZN_ERR_ARG; h->eos_bias = bias; return ZN_OK; }

// ------------------------------------------------------------------------------------------------ measurement
// Launches one of the step's weight-streaming kernels `iters` times on `stream`, cycling over the layers so that
// every launch streams its weights from HBM (26 x 67 MB >> the 256 MiB Infinity Cache), bracketed by HIP events on
// that stream.  which: 0 = LayerNorm+fc1+SiLU-gate, 1 = fc2+residual, 2 = out_proj+residual, 3 = LayerNorm+heads.
extern "C" int zn_bench_kernel(zn_handle h, int32_t which, int32_t rows, int32_t iters, float* ms_per_launch, double* bytes_per_launch,
                               zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!ms_per_launch || !bytes_per_launch || iters < 1 || (rows & 0xff) < 1 || (rows & 0xff) > h->max_rows || which < 0 || which > 8)
    ZN_FAIL(h, ZN_ERR_ARG, "zn_bench_kernel: bad argument");
  h->gen_stream = (hipStream_t)stream;
  const bool same_layer = (rows & 0x100) != 0;   // measurement variant: keep hitting layer 0 (weights stay in the Infinity Cache)
  const int ctx_arg = (rows >> 16) & 0x7fff;     // which == 6: keys already in the cache (0 = 450, the mean context of a 10 s utterance)
  rows &= 0xff;
  hipStream_t s = (hipStream_t)stream;
  const zn_config& c = h->cfg;
  const int d = c.d_model;
  HIPCHK(h, hipMemsetAsync(h->x, 0, (size_t)rows * d * 2, s));
  HIPCHK(h, hipMemsetAsync(h->mbuf, 0, (size_t)rows * c.d_ff * 2, s));
  HIPCHK(h, hipMemsetAsync(h->o1, 0, (size_t)rows * d * 2, s));
  const int hd = h->hd, nq = c.n_heads * hd, nkv = c.n_heads_kv * hd;
  bf16_t* tkv = nullptr; int* tlen = nullptr; int stack_nbk = -1;   // which == 4, 5: a scratch cache of 8 positions per row, all rows at position 0; which == 6: key blocks of the launch
  if (which == 5 && !chain_allowed(h, rows)) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_bench_kernel: the persistent chain serves batch 1 (2 rows) of the transformer only");
  if (which == 4 || which == 5) {
    HIPCHK(h, hipMalloc(&tkv, (size_t)rows * 8 * 2 * nkv * 2));
    HIPCHK(h, hipMalloc(&tlen, (size_t)rows * sizeof(int)));
    HIPCHK(h, hipMemsetAsync(tlen, 0, (size_t)rows * sizeof(int), s));
  }
  // which == 6: the whole-step kernel (every block of a decode step + the heads in ONE launch) on a scratch cache of its own per layer,
  // all rows at position ctx; the handle's generation state is put back afterwards
  std::vector<void*> skv;
  GenHost saved_gen;
  const int ctx = ctx_arg > 0 ? ctx_arg : 450;
  if (which == 6) {
    saved_gen = h->gen;
    if (!persist_active(h, rows)) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_bench_kernel: the whole-step kernel serves one or two rows of the transformer only");
    if (!h->stack_checked) { h->stack_ok = stack_shapes_ok(h); h->stack_checked = true; }
    if ((stack_nbk = stack_blocks_for(h, rows, ctx + 1)) < 0) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_bench_kernel: the whole-step kernel does not serve this model / context");
    const int cap = ctx + 8;
    std::vector<int> lens(rows, ctx);
    HIPCHK(h, hipMalloc(&tlen, (size_t)rows * sizeof(int)));
    HIPCHK(h, ZN_NOT_IN_CAPTURE(hipMemcpy(tlen, lens.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice)));
    skv.assign(c.n_layer, nullptr);
    h->gen.kv_layers.assign(c.n_layer, nullptr);
    for (int li = 0; li < c.n_layer; ++li) {
      HIPCHK(h, hipMalloc(&skv[li], (size_t)rows * cap * 2 * nkv * 2));
      HIPCHK(h, hipMemsetAsync(skv[li], 0, (size_t)rows * cap * 2 * nkv * 2, s));
      h->gen.kv_layers[li] = skv[li];
    }
    h->gen.max_len = cap; h->gen.lengths = tlen;
    HIPCHK(h, hipMemsetAsync(h->x_emb, 0, (size_t)rows * d * 2, s));
    HIPCHK(h, hipMemsetAsync(h->q, 0, (size_t)rows * d * 2, s));
    int rcb = build_stack_table(h);
    if (rcb) return rcb;
  }
  // which == 7: the Mamba2 in_proj (conv-window epilogue included) on a scratch window, cycling through the Mamba2 layers
  std::vector<int> mamba_layers;
  bf16_t* tconv = nullptr;
  // which == 8: the Mamba2 out_proj; up to 4 rows with one norm group it carries the gated norm as its prologue, as in a step (on zeroed gated values)
  const bool out_gated = which == 8 && c.arch == 1 && mamba_gated_pro(c, rows);
  if (which == 7 || which == 8) {
    for (int li = 0; li < c.n_layer; ++li) if (c.arch == 1 && h->layers[li].kind == 1) mamba_layers.push_back(li);
    if (mamba_layers.empty()) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_bench_kernel: the handle has no Mamba2 layer");
    if (which == 8) {
      HIPCHK(h, hipMemsetAsync(h->m_g, 0, (size_t)rows * c.m_d_inner * 2, s));
      if (out_gated) HIPCHK(h, hipMemsetAsync(h->m_vg, 0, (size_t)rows * c.m_d_inner * sizeof(float), s));
    } else {
      HIPCHK(h, hipMalloc(&tconv, (size_t)rows * h->m_conv_dim * 4 * 2));
      HIPCHK(h, hipMemsetAsync(tconv, 0, (size_t)rows * h->m_conv_dim * 4 * 2, s));
    }
  }
  hipEvent_t e0, e1;
  HIPCHK(h, hipEventCreate(&e0));
  HIPCHK(h, hipEventCreate(&e1));
  int rc = ZN_OK;
  // which 0, 1, 2: one launch of layer_post_attention, which 3, 4, 7, 8: heads_logits, layer_in_proj and the Mamba2 projections - the step's own code, so what is priced is what runs.
  // which == 0 at 5..16 rows: fc1 normalises from the statistics its producer left; the producer runs once, outside the timed loop, on the zeroed rows.
  // Up to 4 rows fc1 / fc2 are planned as for a block whose FP8 stream is offered (the GEMV reads it under ZN_TUNE_FP8_SMALL_ROWS = 2) when every block has one;
  // from 5 rows on, the plans of the bf16 weights
  const PostAttnPlans pp = plan_post_attention(h, rows, rows <= 4 && every_layer_offers(h, SL_FC1));
  if (which == 0 && pp.out.writes_ln_stats) rc = layer_post_attention(h, 0, h->x, rows, s, nullptr, &pp, SL_OUT_PROJ);
  for (int pass = 0; pass < 2 && rc == ZN_OK; ++pass) {   // pass 0 = warm-up
    if (pass == 1) HIPCHK(h, hipEventRecord(e0, s));
    for (int i = 0; i < (pass ? iters : (iters < 8 ? iters : 8)) && rc == ZN_OK; ++i) {
      const int li = same_layer ? 0 : i % c.n_layer;
      if (which <= 2) rc = layer_post_attention(h, li, h->x, rows, s, nullptr, &pp, which == 0 ? SL_FC1 : which == 1 ? SL_FC2 : SL_OUT_PROJ);
      else if (which == 6) rc = launch_stack(h, s, rows, stack_nbk);
      else if (which == 7) rc = mamba_in_proj(h, mamba_layers[same_layer ? 0 : i % mamba_layers.size()], h->x, tconv, rows, s);
      else if (which == 8 && out_gated) rc = mamba_out_proj_gated(h, mamba_layers[same_layer ? 0 : i % mamba_layers.size()], h->x, rows, s);
      else if (which == 8) rc = mamba_out_proj(h, mamba_layers[same_layer ? 0 : i % mamba_layers.size()], h->m_g, h->x, rows, s);
      else if (which == 5) {
        if (i % c.n_layer == c.n_layer - 1) continue;       // the last block's launch has no in_proj: not the launch being priced
        rc = launch_chain(h, i % c.n_layer, std::vector<const void*>(c.n_layer, tkv), 8, tlen, s);
      } else if (which == 4) rc = layer_in_proj(h, li, h->x, tkv, 8, tlen, rows, s);
      else rc = heads_logits(h, h->x, rows, s);
    }
  }
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(e1, s));
  HIPCHK(h, hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (tkv) (void)hipFree(tkv);
  if (tlen) (void)hipFree(tlen);
  if (tconv) (void)hipFree(tconv);
  if (which == 6) {
    for (void* p : skv) if (p) (void)hipFree(p);
    h->gen = saved_gen;
    if (h->gen.gen_active && (int)h->gen.kv_layers.size() == c.n_layer) { int rcb = build_stack_table(h); if (rcb) return rcb; }
    int tmo = 0;
    HIPCHK(h, ZN_NOT_IN_CAPTURE(hipMemcpy(&tmo, &h->st->pad[0], sizeof(int), hipMemcpyDeviceToHost)));
    if (tmo != 0) return handoff_timeout(h, tmo);
  }
  if (which == 5 || which == 6) h->epoch_bound += (unsigned long long)(iters + 8) * (c.n_layer + 1);
  int launches = iters;
  if (which == 5) { launches = 0; for (int i = 0; i < iters; ++i) launches += (i % c.n_layer != c.n_layer - 1); }
  *ms_per_launch = ms / launches;
  // chain launch: out_proj (read once, applied twice), fc1, fc2 of the block and in_proj of the next one
  const double wbytes = which == 5 ? ((double)d * nq + 3.0 * c.d_ff * d + (double)(nq + 2 * nkv) * d) * 2 : which == 0 ? 2.0 * c.d_ff * d * 2 : which == 1 ? (double)d * c.d_ff * 2 : which == 2 ? (double)d * c.n_heads * h->hd * 2
                        : which == 4 ? (double)(nq + 2 * nkv) * d * 2 : (double)c.n_codebooks * c.vocab_head * d * 2;
  *bytes_per_launch = which == 7 ? (double)h->m_d_in_proj * d * 2 : which == 8 ? (double)d * c.m_d_inner * 2 : wbytes;   // algorithmic bytes = the weight matrix, read once (activations are KBs)
  if (which == 6) {             // every block's out_proj (once), fc1, fc2, in_proj; the heads; K and V of `ctx` keys read, one row written
    const double per_block = ((double)d * nq + 3.0 * c.d_ff * d) * 2, inp = (double)(nq + 2 * nkv) * d * 2, kvpos = 2.0 * nkv * 2;
    const int nin = stack_pre(h) ? c.n_layer : c.n_layer - 1;      // in_proj of block 0 inside the launch (the pre-block) or before it
    *bytes_per_launch = c.n_layer * per_block + nin * inp + (double)c.n_codebooks * c.vocab_head * d * 2 +
                        (double)rows * c.n_layer * kvpos * ctx + (double)rows * nin * kvpos;
  }
  return ZN_OK;
}

// ------------------------------------------------------------------------------------------------ single ops
// A plan's LayerNorm launch normalises the rows of one launch group into nbuf [max_rows][d_model]: a caller-chosen K may not outrun it.
static int check_ln_launch_fits(zn_handle h, const LinearPlan& p, int rows, int K, const char* who) {
  if (p.err || !(p.ln_launch || (p.lnp && p.row_tiles > 1))) return ZN_OK;      // (the wide plan normalises from handed-over statistics into nbuf too)
  const int per = p.rows_per_launch && p.rows_per_launch < rows ? p.rows_per_launch : rows;
  if ((size_t)per * K > (size_t)h->max_rows * h->cfg.d_model)
    ZN_FAIL(h, ZN_ERR_ARG, "%s: the LayerNorm launch over %d rows of K = %d exceeds the handle's buffer of %d x %d", who, per, K, h->max_rows, h->cfg.d_model);
  return ZN_OK;
}

template <int PRO, int EPI>
static int linear_fused_go(zn_handle h, const LinearPlan& p, const GemvArgs& a, int rows, hipStream_t s) {
  return launch_linear<PRO, EPI>(h, p, a, rows, s);
}

// zn_op_linear_fused, and (W_q != null) zn_op_linear_fp8: the same op with the weights offered as an FP8 stream as well
static int linear_fused_impl(zn_handle h, zn_linear_op* op, const void* W_q, const void* W_exp, bool fp8, zn_stream stream) {
  if (!h || !op) return ZN_ERR_ARG;
  for (int i = 0; i < ZN_LP_NFIELDS; ++i) op->plan[i] = 0;
  op->plan[ZN_LP_ERR] = ZN_ERR_ARG;
  const zn_config& c = h->cfg;
  const int pro = op->pro, epi = op->epi, rows = op->rows, N = op->N, K = op->K;
  const bool prefill = op->prefill != 0;
  if (pro < 0 || pro >= ZN_NPRO || epi < 0 || epi >= ZN_NEPI || (op->prefill != 0 && op->prefill != 1) || (op->ln_stats_in != 0 && op->ln_stats_in != 1))
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: bad prologue / epilogue / flag");
  if (epi == EPI_MAMBA || (pro == PRO_GATED && epi != EPI_STORE)) { op->plan[ZN_LP_ERR] = ZN_ERR_UNSUPPORTED; ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_op_linear_fused: prologue %d with epilogue %d is not a production pair", pro, epi); }
  if (!op->W || rows < 1 || N < 1 || K < 8 || K % 8 || op->target_blocks < 0) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: bad shape or weights");
  if ((pro == PRO_GATED ? !op->gv : !op->x) || (pro != PRO_NONE && !op->ln_w) || (pro == PRO_LN && !op->ln_b))
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: an operand of the prologue is missing");
  if (pro == PRO_LN && K > 4096) { op->plan[ZN_LP_ERR] = ZN_ERR_UNSUPPORTED; ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_op_linear_fused: fused LayerNorm needs K <= 4096"); }
  if (((epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SILU || (epi == EPI_ROPE_KV && prefill)) && !op->out) || (epi == EPI_RESID && !op->resid) ||
      (epi == EPI_F32 && !op->out_f32) || (epi == EPI_SILU && N % 2) || (op->bias && (epi != EPI_STORE || prefill)))
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: an operand of the epilogue is missing or not served");
  if (epi == EPI_ROPE_KV) {
    if ((!op->kv && !h->op_kv8) || !op->q_out || op->max_len < 1 || N != (c.n_heads + 2 * c.n_heads_kv) * h->hd) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: RoPE + KV append needs kv, q_out, max_len and N = (Hq + 2 Hkv) hd");
    if (prefill ? (op->pf_S < 1 || rows % op->pf_S || op->pf_base < 0 || op->pf_base + op->pf_S > op->max_len) : !op->lengths)
      ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_fused: RoPE + KV append needs lengths (decode) or pf_S dividing rows with pf_base + pf_S <= max_len (prefill)");
  }
  LinearEnv env = linear_env(h, false);
  if (fp8) {
#define ZN_F8_REFUSE(code, ...) do { op->plan[ZN_LP_ERR] = code; ZN_FAIL(h, code, __VA_ARGS__); } while (0)
    if (!W_q || !W_exp) ZN_F8_REFUSE(ZN_ERR_ARG, "zn_op_linear_fp8: codes or exponents missing");
    if (!lin_has_w8(pro, epi)) ZN_F8_REFUSE(ZN_ERR_UNSUPPORTED, "zn_op_linear_fp8: prologue %d with epilogue %d has no FP8 kernel (fc1: none or LayerNorm x SiLU gate; fc2: none x residual)", pro, epi);
    if (prefill) ZN_F8_REFUSE(ZN_ERR_UNSUPPORTED, "zn_op_linear_fp8: the prefill kernels read bf16 weights");
    if (K % ZN_G16_KC) ZN_F8_REFUSE(ZN_ERR_UNSUPPORTED, "zn_op_linear_fp8: K=%d is no multiple of %d", K, ZN_G16_KC);
    env.w8_offered = h->tune[ZN_TUNE_MLP_FP8] != 2;
    env.w8v_offered = env.w8_offered && fp8_small_rows_on(h->tune);
  }
  LinearPlan p = plan_linear(env, pro, epi, rows, N, K, op->target_blocks > 0 ? op->target_blocks : 1, prefill, op->want_ln_stats_out != 0, op->ln_stats_in != 0);
  int* o = op->plan;
  o[ZN_LP_W8] = p.w8;
  o[ZN_LP_KERNEL] = (int)p.kernel; o[ZN_LP_EPI] = p.epi; o[ZN_LP_KS] = p.ks; o[ZN_LP_NCH] = p.nch; o[ZN_LP_UPW] = p.upw; o[ZN_LP_BLOCKS] = p.blocks; o[ZN_LP_FULL] = p.full;
  o[ZN_LP_NW] = p.nw; o[ZN_LP_TILE8] = p.tile8; o[ZN_LP_NWV] = p.nwv; o[ZN_LP_GROUPS] = p.groups; o[ZN_LP_KSPLIT] = p.ksplit; o[ZN_LP_LNP] = p.lnp; o[ZN_LP_LN_PRO] = p.ln_pro;
  o[ZN_LP_LN_LAUNCH] = p.ln_launch; o[ZN_LP_WRITES_LN_STATS] = p.writes_ln_stats; o[ZN_LP_READS_LN_STATS] = p.reads_ln_stats; o[ZN_LP_ERR] = p.err;
  o[ZN_LP_ROPE_DONE] = epi == EPI_ROPE_KV && p.epi == EPI_ROPE_KV && !p.err; o[ZN_LP_ROWS_PER_LAUNCH] = p.rows_per_launch;
  o[ZN_LP_ROW_TILES] = p.row_tiles;
  if (p.err) ZN_FAIL(h, p.err, "%s", p.msg);
  if (fp8 && !p.w8) ZN_F8_REFUSE(ZN_ERR_UNSUPPORTED, "zn_op_linear_fp8: this op's plan (kernel %d) would not read the FP8 stream", (int)p.kernel);
#undef ZN_F8_REFUSE
  int rc;
#define ZN_LF_REFUSE(...) do { o[ZN_LP_ERR] = ZN_ERR_ARG; ZN_FAIL(h, ZN_ERR_ARG, __VA_ARGS__); } while (0)
  if ((rc = check_ln_launch_fits(h, p, rows, K, "zn_op_linear_fused"))) { o[ZN_LP_ERR] = rc; return rc; }
  if ((p.writes_ln_stats || p.reads_ln_stats) && rows > h->max_rows) ZN_LF_REFUSE("zn_op_linear_fused: LayerNorm statistics of %d rows exceed the handle's %d", rows, h->max_rows);
  if (op->ln_stats_in && !h->ln_part) ZN_LF_REFUSE("zn_op_linear_fused: the handle has no statistics buffer");
  if (p.kernel == LinearPlan::GEMM_TILED && p.epi == EPI_SILU) {   // the tiled SiLU gate goes through pf_u [pf_rows][2 d_ff]
    if (N % 4) ZN_LF_REFUSE("zn_op_linear_fused: the row-wise SiLU gate takes column pairs (N = %d is no multiple of 4)", N);
    const size_t per = (size_t)2 * c.d_ff, need = ((size_t)rows * N + per - 1) / per;
    if ((rc = ensure_prefill_ws(h, need))) { o[ZN_LP_ERR] = rc; return rc; }
  }
#undef ZN_LF_REFUSE
  GemvArgs a = linear_args(h, op->W, N, K, (const bf16_t*)op->x, (bf16_t*)op->out, (const bf16_t*)op->resid);
  a.ln_w = (const bf16_t*)op->ln_w; a.ln_b = (const bf16_t*)op->ln_b; a.gv = (const float*)op->gv; a.bias = (const bf16_t*)op->bias; a.out_f32 = (float*)op->out_f32;
  a.ln_part_out = op->want_ln_stats_out ? h->ln_part : nullptr;
  a.ln_part_in = op->ln_stats_in ? h->ln_part : nullptr;
  a.W8q = (const uint8_t*)W_q; a.W8exp = (const int8_t*)W_exp;
  if (epi == EPI_ROPE_KV) {
    a.lengths = op->lengths; a.hd = h->hd; a.n_heads = c.n_heads; a.n_heads_kv = c.n_heads_kv; a.q_out = (bf16_t*)op->q_out; a.kv = (bf16_t*)op->kv;
    a.rope = h->rope; a.max_len = op->max_len; a.rope_positions = c.rope_positions;
    a.kv8 = h->op_kv8; a.kv_round = h->op_kv8 != nullptr;      // zn_op_bind_kv_fp8
    if (prefill) { a.pf_S = op->pf_S; a.pf_base = op->pf_base; }
  }
  hipStream_t s = (hipStream_t)stream;
  rc = ZN_ERR_UNSUPPORTED;
  const int e = p.epi;       // (prefill: EPI_ROPE_KV not served in the epilogue arrives here as EPI_STORE, as in prefill_linear)
  if (pro == PRO_NONE) {
    if (e == EPI_STORE) rc = linear_fused_go<PRO_NONE, EPI_STORE>(h, p, a, rows, s);
    else if (e == EPI_RESID) rc = linear_fused_go<PRO_NONE, EPI_RESID>(h, p, a, rows, s);
    else if (e == EPI_SILU) rc = linear_fused_go<PRO_NONE, EPI_SILU>(h, p, a, rows, s);
    else if (e == EPI_F32) rc = linear_fused_go<PRO_NONE, EPI_F32>(h, p, a, rows, s);
    else if (e == EPI_ROPE_KV) rc = linear_fused_go<PRO_NONE, EPI_ROPE_KV>(h, p, a, rows, s);
  } else if (pro == PRO_LN) {
    if (e == EPI_STORE) rc = linear_fused_go<PRO_LN, EPI_STORE>(h, p, a, rows, s);
    else if (e == EPI_RESID) rc = linear_fused_go<PRO_LN, EPI_RESID>(h, p, a, rows, s);
    else if (e == EPI_SILU) rc = linear_fused_go<PRO_LN, EPI_SILU>(h, p, a, rows, s);
    else if (e == EPI_F32) rc = linear_fused_go<PRO_LN, EPI_F32>(h, p, a, rows, s);
    else if (e == EPI_ROPE_KV) rc = linear_fused_go<PRO_LN, EPI_ROPE_KV>(h, p, a, rows, s);
  } else if (e == EPI_STORE) rc = linear_fused_go<PRO_GATED, EPI_STORE>(h, p, a, rows, s);
  if (rc) { o[ZN_LP_ERR] = rc; return rc; }
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}
extern "C" int zn_op_linear_fused(zn_handle h, zn_linear_op* op, zn_stream stream) { return linear_fused_impl(h, op, nullptr, nullptr, false, stream); }
extern "C" int zn_op_linear_fp8(zn_handle h, zn_linear_op* op, const void* W_q, const void* W_exp, zn_stream stream) {
  return linear_fused_impl(h, op, W_q, W_exp, true, stream);
}

extern "C" int zn_op_fp8_quantize_rows(zn_handle h, const void* W_dev, int32_t N, int32_t K, void* q_dev, void* exp_dev, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!W_dev || !q_dev || !exp_dev || N < 1 || K < 8 || K % 8) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_fp8_quantize_rows: bad argument (K a multiple of 8)");
  hipLaunchKernelGGL(fp8_quantize_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W_dev, K, (uint8_t*)q_dev, (int8_t*)exp_dev);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}
extern "C" int zn_op_fp8_dequant_rows(zn_handle h, const void* q_dev, const void* exp_dev, int32_t N, int32_t K, void* W_out_dev, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!q_dev || !exp_dev || !W_out_dev || N < 1 || K < 8 || K % 8) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_fp8_dequant_rows: bad argument (K a multiple of 8)");
  hipLaunchKernelGGL(fp8_dequant_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)q_dev, (const int8_t*)exp_dev, K, (bf16_t*)W_out_dev);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}
// ZN_FP8_VERIFY: 8-element pieces of W [N][K] that differ from the dequantised stream (< 0: a HIP error)
static long long fp8_mismatches(const void* q, const void* e, const void* W, int N, int K) {
  unsigned* cnt = nullptr;
  unsigned host = 0;
  if (ZN_NOT_IN_CAPTURE(hipMalloc(&cnt, sizeof(unsigned))) != hipSuccess) return -1;
  bool ok = ZN_NOT_IN_CAPTURE(hipMemset(cnt, 0, sizeof(unsigned))) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(fp8_compare_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)0, (const uint8_t*)q, (const int8_t*)e, K, (const bf16_t*)W, cnt);
    ok = hipGetLastError() == hipSuccess && ZN_NOT_IN_CAPTURE(hipMemcpy(&host, cnt, sizeof(unsigned), hipMemcpyDeviceToHost)) == hipSuccess;
  }
  (void)hipFree(cnt);
  return ok ? (long long)host : -1;
}
// What zn_set_mlp_fp8 and zn_set_mamba_fp8 share once their own refusals have passed: all four pointers or none, the ZN_FP8_VERIFY comparison of both matrices, the graph drop.
struct Fp8Stream { const char* name; const void *q, *exp, *W; int N, K; };
static int attach_fp8_pair(zn_handle h, const char* who, int layer, const Fp8Stream& a, const Fp8Stream& b) {
  const int n_set = (a.q != nullptr) + (a.exp != nullptr) + (b.q != nullptr) + (b.exp != nullptr);
  if (n_set != 0 && n_set != 4) ZN_FAIL(h, ZN_ERR_ARG, "%s: all four pointers, or none", who);
  const char* v = getenv("ZN_FP8_VERIFY");
  if (n_set == 4 && v && atoi(v) == 1) {
    const long long b1 = fp8_mismatches(a.q, a.exp, a.W, a.N, a.K);
    const long long b2 = b1 < 0 ? -1 : fp8_mismatches(b.q, b.exp, b.W, b.N, b.K);
    if (b1 < 0 || b2 < 0) ZN_FAIL(h, ZN_ERR_HIP, "%s: the verification could not run", who);
    if (b1 || b2) ZN_FAIL(h, ZN_ERR_ARG, "%s: layer %d's bf16 weights are not the dequantised stream (%s: %lld, %s: %lld pieces of 8 differ)", who, layer, a.name, b1, b.name, b2);
  }
  free_graph(h); h->gen.emb_valid = false;
  return ZN_OK;
}
extern "C" int zn_set_mlp_fp8(zn_handle h, int32_t layer, const void* fc1_q, const void* fc1_exp, const void* fc2_q, const void* fc2_exp) {
  if (!h) return ZN_ERR_ARG;
  const zn_config& c = h->cfg;
  if (c.arch == 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mlp_fp8: the hybrid stack has no FP8 path");
  if (layer < 0 || layer >= c.n_layer) ZN_FAIL(h, ZN_ERR_ARG, "zn_set_mlp_fp8: layer %d out of range", layer);
  if (h->layers[layer].kind != 0) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mlp_fp8: layer %d is a Mamba2 layer", layer);
  if (c.d_model % ZN_G16_KC || c.d_ff % ZN_G16_KC) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mlp_fp8: d_model %d / d_ff %d must be multiples of %d", c.d_model, c.d_ff, ZN_G16_KC);
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_MLP_FP8));
  if (int rc = attach_fp8_pair(h, "zn_set_mlp_fp8", layer, {"fc1", fc1_q, fc1_exp, h->layers[layer].fc1, 2 * c.d_ff, c.d_model}, {"fc2", fc2_q, fc2_exp, h->layers[layer].fc2, c.d_model, c.d_ff})) return rc;
  zn_handle_s::MlpFp8& f = h->mlp_fp8[layer];
  f.fc1_q = (const uint8_t*)fc1_q; f.fc1_exp = (const int8_t*)fc1_exp; f.fc2_q = (const uint8_t*)fc2_q; f.fc2_exp = (const int8_t*)fc2_exp;
  return ZN_OK;
}
extern "C" int zn_set_kv_fp8(zn_handle h, int32_t on) {
  if (!h) return ZN_ERR_ARG;
  if (h->cfg.arch == 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_kv_fp8: the hybrid stack's attention layers keep a bf16 KV cache");
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_KV_FP8));
  h->kv_fp8 = on != 0;
  free_graph(h); h->gen.emb_valid = false;
  return ZN_OK;
}
extern "C" int zn_set_kv_fp8_only(zn_handle h, int32_t on) {
  if (!h) return ZN_ERR_ARG;
  if (h->cfg.arch == 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_kv_fp8_only: the hybrid stack's attention layers keep a bf16 KV cache");
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_KV_FP8_ONLY));
  h->kv_fp8_only = on != 0;
  free_graph(h); h->gen.emb_valid = false;
  return ZN_OK;
}
extern "C" size_t zn_kv_fp8_bytes_per_layer(const zn_config* c, int32_t rows, int32_t max_len) { return zn_kv_bytes_per_layer(c, rows, max_len) / 2; }
extern "C" int zn_gen_bind_kv_fp8(zn_handle h, const void* const* codes_layers_dev) {
  if (!h) return ZN_ERR_ARG;
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_BIND_KV_FP8));
  if (!codes_layers_dev) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_bind_kv_fp8: null argument");
  for (int li = 0; li < h->cfg.n_layer; ++li)
    if (!codes_layers_dev[li] && h->layers[li].kind == 0) ZN_FAIL(h, ZN_ERR_ARG, "zn_gen_bind_kv_fp8: layer %d has no code cache", li);
  h->gen.kv8_layers.assign(codes_layers_dev, codes_layers_dev + h->cfg.n_layer);
  h->adm_cap_S = 0;          // a session's admission table names the code caches: rebuilt by the next admission
  return ZN_OK;
}
extern "C" int zn_kv_cache_plan(zn_handle h, int32_t rows, int32_t out[3]) {
  if (!h || !out || rows < 1) return ZN_ERR_ARG;
  const bool codes_only = kv_codes_only_rows(h, rows);
  out[0] = h->kv_fp8 && kv_fp8_rows(h, rows);
  out[1] = out[0] && kv_fp8_attn_reads(h, rows, codes_only);
  out[2] = !codes_only;
  return ZN_OK;
}
extern "C" int zn_kv_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]) {
  int32_t o[3];
  if (!out || zn_kv_cache_plan(h, rows, o) != ZN_OK) return ZN_ERR_ARG;
  out[0] = o[0]; out[1] = o[1];
  return ZN_OK;
}
extern "C" int zn_op_bind_kv_fp8(zn_handle h, void* codes_dev) {
  if (!h) return ZN_ERR_ARG;
  if (h->cfg.arch == 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_op_bind_kv_fp8: the hybrid stack's attention layers keep a bf16 KV cache");
  h->op_kv8 = (uint8_t*)codes_dev;
  return ZN_OK;
}
extern "C" int zn_op_rope_kv_rows(zn_handle h, void* qkv_dev, void* kv_dev, int32_t max_len, int32_t S, int32_t base, int32_t rows, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  const zn_config& c = h->cfg;
  if (!qkv_dev || (!kv_dev && !h->op_kv8) || max_len < 1 || S < 1 || base < 0 || rows < 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_rope_kv_rows: bad argument");
  if (c.arch != 0) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_op_rope_kv_rows: the transformer prefill's kernel (interleaved pairs)");
  hipLaunchKernelGGL(rope_kv_rows_kernel, dim3(S, rows), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv_dev, (bf16_t*)kv_dev, h->rope, S, base, max_len, c.n_heads, c.n_heads_kv,
                     h->hd, c.rope_positions, h->op_kv8, h->op_kv8 != nullptr ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}
extern "C" int zn_set_mamba_fp8(zn_handle h, int32_t layer, const void* in_q, const void* in_exp, const void* out_q, const void* out_exp) {
  if (!h) return ZN_ERR_ARG;
  const zn_config& c = h->cfg;
  if (c.arch != 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mamba_fp8: a transformer handle has no Mamba2 layer (zn_set_mlp_fp8 serves its fc1 / fc2)");
  if (layer < 0 || layer >= c.n_layer) ZN_FAIL(h, ZN_ERR_ARG, "zn_set_mamba_fp8: layer %d out of range", layer);
  if (h->layers[layer].kind != 1) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mamba_fp8: layer %d is an attention layer", layer);
  if (c.d_model != 2 * ZN_G16K_NKW * ZN_G16K_KCH || c.m_d_inner != 4 * ZN_G16K_NKW * ZN_G16K_KCH)
    ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_set_mamba_fp8: the FP8 kernels serve d_model 2048 and d_inner 4096 (got d_model %d, d_inner %d)", c.d_model, c.m_d_inner);
  ZN_GEN_CHECK(h, gen_call_order(h->gen, GE_SET_MAMBA_FP8));
  if (int rc = attach_fp8_pair(h, "zn_set_mamba_fp8", layer, {"in_proj", in_q, in_exp, h->layers[layer].m_in_proj, h->m_d_in_proj, c.d_model},
                               {"out_proj", out_q, out_exp, h->layers[layer].m_out_proj, c.d_model, c.m_d_inner})) return rc;
  zn_handle_s::MambaFp8& f = h->mamba_fp8[layer];
  f.in_q = (const uint8_t*)in_q; f.in_exp = (const int8_t*)in_exp; f.out_q = (const uint8_t*)out_q; f.out_exp = (const int8_t*)out_exp;
  return ZN_OK;
}

// ---- The plan queries read the step's own table (zn_step_linears.h) through step_plan and plan_post_attention, as the launches do.
extern "C" int zn_mlp_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]) {
  if (!h || !out || rows < 1) return ZN_ERR_ARG;
  const bool all = every_layer_offers(h, SL_FC1);      // 1 only when every block has a stream: a handle with some blocks attached reports 0
  const PostAttnPlans pp = plan_post_attention(h, rows, all);
  out[0] = pp.fc1.w8; out[1] = pp.fc2.w8;
  return ZN_OK;
}
extern "C" int zn_mamba_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]) {
  if (!h || !out || rows < 1) return ZN_ERR_ARG;
  const bool all = every_layer_offers(h, SL_M_IN_PROJ);      // 1 only when every Mamba2 layer has a stream
  out[0] = all && step_plan(h, SL_M_IN_PROJ, -1, rows, true).w8;
  out[1] = all && step_plan(h, SL_M_OUT_PROJ, -1, rows, true).w8;
  return ZN_OK;
}
// Activation rows per weight pass of a decode step of `rows` rows as this handle would run it now: in_proj, out_proj, fc1, fc2, heads (with FP8 streams attached to
// every block, the plans that read them).
extern "C" int zn_decode_rows_plan(zn_handle h, int32_t rows, int32_t out[5]) {
  if (!h || !out || rows < 1) return ZN_ERR_ARG;
  const PostAttnPlans pp = plan_post_attention(h, rows, every_layer_offers(h, SL_FC1));
  const LinearPlan ps[5] = {step_plan(h, SL_IN_PROJ, -1, rows, false), pp.out, pp.fc1, pp.fc2, step_plan(h, SL_HEADS, -1, rows, false)};
  for (int k = 0; k < 5; ++k) {
    if (ps[k].err) ZN_FAIL(h, ps[k].err, "%s", ps[k].msg);
    out[k] = ps[k].rows_per_launch;
  }
  return ZN_OK;
}

// The same for a hybrid decode step: the table's hybrid linears in its order, each planned for the first layer that has it; 0 where the stack has no such layer.
extern "C" int zn_hybrid_rows_plan(zn_handle h, int32_t rows, int32_t out[7]) {
  if (!h || !out || rows < 1) return ZN_ERR_ARG;
  if (h->cfg.arch != 1) ZN_FAIL(h, ZN_ERR_STATE, "zn_hybrid_rows_plan: not a hybrid handle");
  int first[2] = {-1, -1};      // the first attention layer, the first Mamba2 layer
  for (int li = h->cfg.n_layer - 1; li >= 0; --li) first[h->layers[li].kind == 1] = li;
  for (int k = 0; k < 7; ++k) out[k] = 0;
  for (int lin = SL_M_IN_PROJ; lin <= SL_H_HEADS; ++lin) {
    const int li = lin == SL_H_HEADS ? -1 : first[step_linear_offer(lin) == SO_MAMBA];
    if (lin != SL_H_HEADS && li < 0) continue;
    const LinearPlan p = step_plan(h, lin, li, rows, stream_offered(h, lin, li));
    if (p.err) ZN_FAIL(h, p.err, "%s", p.msg);
    out[lin - SL_M_IN_PROJ] = p.rows_per_launch;
  }
  return ZN_OK;
}

extern "C" int zn_op_linear(zn_handle h, const void* x, const void* ln_w, const void* ln_b, const void* W, void* out, int32_t rows,
                            int32_t N, int32_t K, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !W || !out || rows < 1 || N < 1 || K < 8 || K % 8) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear: bad argument");
  GemvArgs a = linear_args(h, W, N, K, (const bf16_t*)x, (bf16_t*)out);
  int rc;
  if (ln_w) {
    if (K > 4096) ZN_FAIL(h, ZN_ERR_UNSUPPORTED, "zn_op_linear: fused LayerNorm needs K <= 4096");
    if ((rc = check_ln_launch_fits(h, plan_linear(linear_env(h, false), PRO_LN, EPI_STORE, rows, N, K, 1024, false, false, false), rows, K, "zn_op_linear"))) return rc;
    a.ln_w = (const bf16_t*)ln_w; a.ln_b = (const bf16_t*)ln_b;
    rc = run_gemv<PRO_LN, EPI_STORE>(h, a, rows, 1024, (hipStream_t)stream, false);
  } else rc = run_gemv<PRO_NONE, EPI_STORE>(h, a, rows, 1024, (hipStream_t)stream, false);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_linear_bias(zn_handle h, const void* x, const void* W, const void* bias, void* out, int32_t rows, int32_t N, int32_t K, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !W || !out || rows < 1 || N < 1 || K < 8 || K % 8) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_linear_bias: bad argument");
  GemvArgs a = linear_args(h, W, N, K, (const bf16_t*)x, (bf16_t*)out);
  a.bias = (const bf16_t*)bias;
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0; r0 < rows; r0 += 4) {      // always the GEMV (its epilogue carries the bias); rows are few here
    GemvArgs g = a;
    advance_rows(g, r0, rows - r0 < 4 ? rows - r0 : 4, N);
    int rc = run_gemv<PRO_NONE, EPI_STORE>(h, g, g.nrows, 1024, s);
    if (rc) return rc;
  }
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_gather_rows(zn_handle h, const void* table, const int32_t* ids, void* out, int32_t n, int32_t d, int32_t table_rows, int32_t id_offset,
                                 zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!table || !ids || !out || n < 1 || d < 8 || d % 8 || table_rows < 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_gather_rows: bad argument");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table, ids, (bf16_t*)out, d, table_rows, id_offset);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_fourier(zn_handle h, const float* x, const void* weight, void* out, int32_t n, int32_t in_dim, int32_t half, float min_val, float max_val,
                             zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !weight || !out || n < 1 || in_dim < 1 || half < 1 || !(max_val > min_val)) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_fourier: bad argument");
  hipLaunchKernelGGL(fourier_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)weight, (bf16_t*)out, in_dim, half, min_val, max_val);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_silu(zn_handle h, const void* x, void* out, int64_t n, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !out || n < 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_silu: bad argument");
  const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(silu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, (size_t)n);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_layernorm(zn_handle h, const void* x, const void* w, const void* b, void* out, int32_t rows, int32_t d, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !w || !b || !out || rows < 1 || d < 8 || d % 8 || d > 4096) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_layernorm: bad argument (d <= 4096, multiple of 8)");
  hipLaunchKernelGGL(layernorm_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b,
                     (bf16_t*)out, d, h->cfg.norm_eps);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_layer_decode(zn_handle h, int32_t layer, void* x, void* kv, int32_t max_len, const int32_t* lengths,
                                  const int32_t* ext, int32_t rows, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!x || !kv || !lengths || layer < 0 || layer >= h->cfg.n_layer || rows < 1 || rows > h->max_rows || max_len < 1)
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_layer_decode: bad argument");
  int rc = ensure_attn_ws(h, max_len);
  if (rc) return rc;
  // lengths live on the device: bound the context by the capacity
  rc = layer_decode(h, layer, (bf16_t*)x, (bf16_t*)kv, max_len, lengths, ext, 0, rows, attn_fused_for(h, max_len), (hipStream_t)stream);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_backbone_forward(zn_handle h, const void* hidden_dev, void* out_dev, const void* const* caches_dev, int32_t max_len,
                                      int32_t base, int32_t S, int32_t rows, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  const zn_config& c = h->cfg;
  if (!hidden_dev || !out_dev || !caches_dev || S < 1 || rows < 1 || rows > h->max_rows || base < 0 || max_len < 1 || base + S > max_len)
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_backbone_forward: bad argument (rows %d of at most %d, positions %d + %d of %d)", rows, h->max_rows, base, S, max_len);
  if (base + S > c.rope_positions)
    ZN_FAIL(h, ZN_ERR_ARG, "sequence length %d exceeds the %d-position RoPE table (zonos/backbone/_torch.py:206)", base + S, c.rope_positions);
  hipStream_t s = (hipStream_t)stream;
  int rc = ensure_attn_ws(h, max_len);
  if (rc) return rc;
  const int d = c.d_model;
  const bf16_t* hid = (const bf16_t*)hidden_dev;
  bf16_t* out = (bf16_t*)out_dev;
  const bool batched = S > 1 && h->prefill_mode >= 1 && d % 32 == 0 && c.d_ff % 32 == 0 && (c.arch == 0 || c.m_d_inner % 32 == 0);
  if (batched) {
    const int M = rows * S;
    if (c.arch == 1) {
      if ((rc = hybrid_prefill_core(h, hid, S, rows, caches_dev, max_len, base, h->prefill_mode == 2, s))) return rc;
      launch_add_ln(h, h->pf_x, h->pf_res, 1, 0, h->norm_f_w, h->norm_f_b, out, M, s);
    } else {
      if ((rc = transformer_prefill_core(h, hid, S, rows, caches_dev, max_len, base, s))) return rc;
      hipLaunchKernelGGL(layernorm_kernel, dim3(M), dim3(64), 0, s, h->pf_x, (const bf16_t*)h->norm_f_w, (const bf16_t*)h->norm_f_b, out, d, c.norm_eps);
    }
    HIPCHK(h, hipGetLastError());
    return ZN_OK;
  }
  // position by position through the decode kernels (S = 1: the loop's step).  Attention reproduces the reference's causal
  // flash-attention blocking through the keys spanned by this position's query block.
  const int qb = qsplit(S);
  for (int p = 0; p < S; ++p) {
    hipLaunchKernelGGL(gather_pos_kernel, dim3(rows), dim3(256), 0, s, hid, h->x, S, p, d);
    hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64 > rows ? 64 : rows), 0, s, h->fw_lengths, rows, base + p);
    int ext = (p / qb) * qb + qb; if (ext > S) ext = S;
    const int attn_fused = attn_fused_for(h, base + p + 1);
    for (int li = 0; li < c.n_layer; ++li) {
      if (c.arch == 1) rc = hybrid_layer(h, li, (void*)caches_dev[li], max_len, h->fw_lengths, rows, attn_fused, s);
      else rc = layer_decode(h, li, h->x, (bf16_t*)caches_dev[li], max_len, h->fw_lengths, nullptr, S > 1 ? base + ext : 0, rows, attn_fused, s);
      if (rc) return rc;
    }
    if (c.arch == 1) launch_add_ln(h, h->x, h->res, 1, 0, h->norm_f_w, h->norm_f_b, h->nbuf, rows, s);
    else hipLaunchKernelGGL(layernorm_kernel, dim3(rows), dim3(64), 0, s, h->x, (const bf16_t*)h->norm_f_w, (const bf16_t*)h->norm_f_b, h->nbuf, d, c.norm_eps);
    hipLaunchKernelGGL(scatter_pos_kernel, dim3(rows), dim3(256), 0, s, h->nbuf, out, S, p, d);
  }
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_add_layernorm(zn_handle h, const void* hidden, void* res, const void* w, const void* b, void* out, int32_t rows,
                                   int32_t d, float eps, int32_t flags, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!hidden || !w || (!b && !(flags & 1)) || !out || rows < 1 || d < 8 || d % 8 || d > 4096) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_add_layernorm: bad argument");
  AddLnArgs a{};
  a.h = (const bf16_t*)hidden; a.res = (bf16_t*)res; a.w = (const bf16_t*)w; a.b = (const bf16_t*)b; a.out = (bf16_t*)out; a.d = d;
  a.has_res = res != nullptr; a.write_res = res != nullptr; a.eps = eps; a.rms = flags & 1; a.res32 = (flags >> 1) & 1;
  hipLaunchKernelGGL(add_ln_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_mamba_step(zn_handle h, int32_t layer, const void* x, void* state, void* out, int32_t rows, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (h->cfg.arch != 1) ZN_FAIL(h, ZN_ERR_STATE, "zn_op_mamba_step: the handle is not a hybrid backbone");
  if (!x || !state || !out || layer < 0 || layer >= h->cfg.n_layer || rows < 1 || rows > h->max_rows) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_mamba_step: bad argument");
  if (h->layers[layer].kind != 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_mamba_step: layer %d is an attention layer", layer);
  int rc = mamba_mixer(h, layer, (const bf16_t*)x, state, (bf16_t*)out, rows, (hipStream_t)stream);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_attn_decode(zn_handle h, const void* q, const void* kv, int32_t max_len, const int32_t* lengths, const int32_t* ext,
                                 void* out, int32_t rows, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!q || !lengths || !out || rows < 1 || max_len < 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_decode: bad argument");
  if (rows > h->max_rows) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_decode: rows > max_rows");
  // no bf16 cache: legal exactly where a bound code cache (zn_op_bind_kv_fp8) is what the launch reads
  if (!kv && !(h->op_kv8 && kv_fp8_attn_reads(h, rows))) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_decode: bad argument (no cache, and no bound code cache that %d rows read)", rows);
  int rc = ensure_attn_ws(h, max_len);
  if (rc) return rc;
  rc = run_attention(h, (const bf16_t*)q, (const bf16_t*)kv, max_len, lengths, ext, 0, (bf16_t*)out, rows, attn_fused_for(h, max_len), (hipStream_t)stream, nullptr, h->op_kv8);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_attn_prefill(zn_handle h, const void* q, const void* kv, int32_t max_len, void* out, int32_t positions, int32_t rows,
                                  zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!q || !kv || !out || rows < 1 || positions < 1 || max_len < positions) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_prefill: bad argument");
  const int nq = h->cfg.n_heads * h->hd;
  int rc = prefill_attention(h, (const bf16_t*)q, nq, (const bf16_t*)kv, max_len, (bf16_t*)out, nq, positions, rows, (hipStream_t)stream);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

// Test entry: prefill_attention with the two arguments the ragged prefill and the seam pass (zn_op_attn_prefill fixes them at 0 / NULL).
extern "C" int zn_op_attn_prefill_rows(zn_handle h, const void* q, const void* kv, int32_t max_len, void* out, int32_t positions, int32_t rows,
                                       int32_t base, const int32_t* row_len, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!q || !kv || !out || rows < 1 || positions < 1 || base < 0 || max_len < 1 || (int64_t)base + positions > max_len)
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_prefill_rows: bad argument (positions %d + %d of %d)", base, positions, max_len);
  if (rows > h->max_rows) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_prefill_rows: rows %d > max_rows %d", rows, h->max_rows);
  const int nq = h->cfg.n_heads * h->hd;
  int rc = prefill_attention(h, (const bf16_t*)q, nq, (const bf16_t*)kv, max_len, (bf16_t*)out, nq, positions, rows, (hipStream_t)stream, base, row_len);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

// Test entry: zn_op_attn_prefill_rows on a code cache uint8 [rows][max_len][2][Hkv][hd] - the FP8 forms of the two prefill attention kernels (zn_prefill_attn_fp8_kernels.h)
extern "C" int zn_op_attn_prefill_rows_fp8(zn_handle h, const void* q, const void* codes, int32_t max_len, void* out, int32_t positions, int32_t rows,
                                           int32_t base, const int32_t* row_len, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!q || !codes || !out || rows < 1 || positions < 1 || base < 0 || max_len < 1 || (int64_t)base + positions > max_len)
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_prefill_rows_fp8: bad argument (positions %d + %d of %d)", base, positions, max_len);
  if (rows > h->max_rows) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_attn_prefill_rows_fp8: rows %d > max_rows %d", rows, h->max_rows);
  const int nq = h->cfg.n_heads * h->hd;
  int rc = prefill_attention(h, (const bf16_t*)q, nq, nullptr, max_len, (bf16_t*)out, nq, positions, rows, (hipStream_t)stream, base, row_len, (const uint8_t*)codes);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_embed(zn_handle h, const int32_t* codes, void* out, int32_t batch, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!codes || !out || batch < 1) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_embed: bad argument");
  if (!h->has_io) ZN_FAIL(h, ZN_ERR_STATE, "zn_op_embed: handle was created without embeddings");
  const zn_config& c = h->cfg;
  EmbedArgs e{};
  e.tables = h->emb_tables_dev; e.codes = codes; e.sb = c.n_codebooks; e.si = 1; e.col = 0; e.n_q = c.n_codebooks; e.d = c.d_model;
  e.batch = batch; e.vocab_embed = c.vocab_embed; e.out = (bf16_t*)out; e.dup = 0;
  hipLaunchKernelGGL(embed_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, e);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_assemble_prefill(zn_handle h, const void* cond_dev, int32_t L_c, const int32_t* cond_len_dev, const int32_t* delayed_codes_dev,
                                      int32_t t_total, const int32_t* prefix_len_dev, int32_t batch, int32_t rows, void* hidden_dev, int32_t S, int32_t* row_len_dev,
                                      zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!cond_dev || !cond_len_dev || !delayed_codes_dev || !prefix_len_dev || !hidden_dev || !row_len_dev || L_c < 1 || t_total < 1 || S < 1 || batch < 1 ||
      (rows != batch && rows != 2 * batch))
    ZN_FAIL(h, ZN_ERR_ARG, "zn_op_assemble_prefill: null argument, a non-positive size, or rows %d not batch %d or twice it", rows, batch);
  if (!h->has_io) ZN_FAIL(h, ZN_ERR_STATE, "zn_op_assemble_prefill: handle was created without embeddings");
  const zn_config& c = h->cfg;
  AssembleArgs a{};
  a.cond = (const bf16_t*)cond_dev; a.cond_len = cond_len_dev; a.codes = delayed_codes_dev; a.prefix_len = prefix_len_dev;
  a.hidden = (bf16_t*)hidden_dev; a.row_len = row_len_dev; a.L_c = L_c; a.t_total = t_total; a.S = S; a.batch = batch;
  a.em.tables = h->emb_tables_dev; a.em.n_q = c.n_codebooks; a.em.d = c.d_model; a.em.vocab_embed = c.vocab_embed;
  hipLaunchKernelGGL(assemble_prefill_kernel, dim3(S, rows), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_sample_rows(zn_handle h, const float* logits, const int32_t* recent, int32_t window, const zn_row_params* rows_dev,
                                 uint64_t draw_index, int32_t* tokens, float* probs_out, int32_t batch, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!logits || !rows_dev || !tokens || batch < 1 || (recent && window < 1)) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_sample_rows: bad argument");
  SampleArgs a = make_sample_args(h, zn_sampling{});
  a.raw = logits; a.mix = 0; a.apply_bias = 0; a.batch = batch; a.recent = recent; a.window = window; a.rows = rows_dev;
  a.use_penalty = recent != nullptr; a.tokens = tokens; a.probs_out = probs_out; a.draw = draw_index;
  hipLaunchKernelGGL(sample_kernel, dim3(h->cfg.n_codebooks, batch), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

extern "C" int zn_op_sample(zn_handle h, const float* logits, const int32_t* recent, int32_t window, const zn_sampling* sp,
                            uint64_t draw_index, int32_t* tokens, float* probs_out, int32_t batch, zn_stream stream) {
  if (!h) return ZN_ERR_ARG;
  if (!logits || !sp || !tokens || batch < 1 || (recent && window < 1)) ZN_FAIL(h, ZN_ERR_ARG, "zn_op_sample: bad argument");
  SampleArgs a = make_sample_args(h, *sp);
  a.raw = logits; a.mix = 0; a.apply_bias = 0; a.batch = batch; a.recent = recent; a.window = window;
  a.use_penalty = (recent != nullptr && sp->repetition_penalty != 1.0f); a.tokens = tokens; a.probs_out = probs_out; a.draw = draw_index;
  hipLaunchKernelGGL(sample_kernel, dim3(h->cfg.n_codebooks, batch), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(h, hipGetLastError());
  return ZN_OK;
}

// The host side of one generation: the record zn_gen_begin starts afresh, the call order of the entry points, the rules of
// their host arrays, the slot bookkeeping of a session.  Plain C++: no HIP type, no device call - tests/gen_state_check.cpp runs all of it on
// the CPU against the messages typed in from the code this header replaced.
#pragma once
#include "../../include/zonos_hip.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

// What a check answers: ZN_OK, or the code and the message of zn_last_error.
struct GenErr {
  int code = ZN_OK;
  char msg[1024];
  GenErr() { msg[0] = 0; }
};
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
static inline GenErr gen_fail(int code, const char* fmt, ...) {
  GenErr e;
  e.code = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(e.msg, sizeof e.msg, fmt, ap);
  va_end(ap);
  return e;
}

// Host record of one generation: everything zn_gen_begin sets or resets.  A new per-generation flag goes here (begin() then resets it), and into
// persist_eligible() if it bars the persistent kernels - and into same() and reset() of tests/gen_state_check.cpp, whose size check asks for it.
// What outlives a generation (tuning keys, counters, graphs, last_plan, the FP8 modes) is the handle's.
struct GenHost {
  bool gen_active = false;
  bool gen_ended = false;        // zn_gen_end was called: the state stays readable, no further steps until the next zn_gen_begin
  bool gen_prefilled = false;    // zn_prefill / zn_prefill_rows / zn_gen_admit has run since zn_gen_begin
  bool rows_set = false;         // this generation's samplers read row_tab (zn_gen_set_rows)
  bool pairs_set = false;        // some entry of row_tab names a row pair (a mixed generation): the samplers follow it
  bool prefix_set = false;       // some shift is not 0: this generation's embedding, sampler and bookkeeping launches read prefix_shift
  bool slots_open = false;       // slotted session (zn_gen_open_slots): requests join the running generation slot by slot
  bool rows_unequal2 = false;    // this generation's two unguided rows have different lengths: its steps run the launches path
  bool gen_timed_out = false;    // this generation reported a hand-off timeout
  bool stop_pending = false;     // zn_all_stopped_begin's copy has not been read yet
  bool emb_valid = false;        // x_emb holds the embedding of column st->offset
  bool persist_ok = true;        // this handle may launch the persistent kernels (zn_gen_begin: it holds the device's tenancy, or nobody competes)
  int batch = 0, rows = 0, max_len = 0, t_total = 0, offset0 = 0, max_new = 0;
  float cfg_scale = 2.f;
  zn_sampling sp{};
  int len_hi = 0;                // host-side upper bound of the rows' KV lengths (keys already cached)
  int slot_slack = 0;            // steps a request may run past its own end before it is retired
  std::vector<int> slot_len;     // [batch] host mirror of a busy slot's lengths[b] (they advance by one per step), 0 = idle
  std::vector<char> slot_busy;
  std::vector<const void*> kv_layers, kv8_layers;   // the caller's caches; kv8_layers: the code caches (zn_gen_bind_kv_fp8; empty: none bound)
  int *lengths = nullptr, *codes = nullptr;
  unsigned dbg_pause = 0;        // ChainArgs::dbg_pause of this generation's whole-step launches

  // zn_gen_begin: a fresh record and the call's arguments.  gen_active, persist_ok, dbg_pause, len_hi and the caches follow once zn_gen_begin knows them.
  void begin(int batch_, int rows_, int max_len_, int t_total_, int offset0_, int max_new_, float cfg_scale_, const zn_sampling& sp_, int* lengths_, int* codes_) {
    *this = GenHost{};
    batch = batch_; rows = rows_; max_len = max_len_; t_total = t_total_; offset0 = offset0_; max_new = max_new_;
    cfg_scale = cfg_scale_; sp = sp_; lengths = lengths_; codes = codes_;
  }
  bool running() const { return gen_active && !gen_ended; }
  // With guidance every utterance has a conditional and an unconditional row (rows = 2 batch); cfg_scale == 1: one row per utterance.
  bool guided() const { return rows == 2 * batch; }
  // The generation's half of persist_allowed (zn_api.hip, which holds the reasons): the tenancy, and none of the modes whose launches the persistent kernels do not make.
  bool persist_eligible() const { return persist_ok && !rows_unequal2 && !prefix_set && !slots_open && !pairs_set; }

  // ---- slotted session.  The host bound of the rows' KV lengths in a session: the longest busy slot (an idle slot's rows stay at 0).
  void slots_len_hi() {
    len_hi = 0;
    for (int b = 0; b < batch; ++b) if (slot_busy[b] && slot_len[b] > len_hi) len_hi = slot_len[b];
  }
  void open_slots(int slack) {
    slot_len.assign(batch, 0); slot_busy.assign(batch, 0);
    slot_slack = slack;
    rows_set = prefix_set = slots_open = true;
    pairs_set = !guided();       // a session begun without guidance may admit row pairs at any point: its samplers (captured graphs included) follow the entries' pair words from the start
  }
  void slots_admitted(const zn_admit* a, int n) {
    for (int j = 0; j < n; ++j) { slot_busy[a[j].slot] = 1; slot_len[a[j].slot] = a[j].row_len; }
    slots_len_hi();
  }
  void slots_advance(int n) {
    for (int b = 0; b < batch; ++b) if (slot_busy[b]) slot_len[b] += n;
    slots_len_hi();
  }
  void slot_retired(int slot) {
    slot_busy[slot] = 0; slot_len[slot] = 0;
    slots_len_hi();
  }
};

// ------------------------------------------------------------------------------------------------ call order
enum GenEntry {
  GE_PREFILL, GE_PREFILL_ROWS, GE_SET_ROWS, GE_SET_PREFIX_ROWS, GE_OPEN_SLOTS, GE_ADMIT, GE_RETIRE, GE_ROW_STATE, GE_SAMPLE_FIRST, GE_DECODE_STEPS,
  GE_BIND_KV_FP8, GE_SET_MLP_FP8, GE_SET_MAMBA_FP8, GE_SET_KV_FP8, GE_SET_KV_FP8_ONLY, GE_NENTRIES
};
// One row per entry point; the rules are asked in the order of the columns.
struct GenEntryRule {
  const char* name;
  bool outside;            // belongs outside a generation (no other rule): refused between zn_gen_begin and zn_gen_end
  bool ended_ok;           // a generation that zn_gen_end has closed still serves it
  const char* slotted;     // refused in a slotted session, with this reason (nullptr: accepted there)
  const char* prefilled;   // refused once the generation has prefilled, with these words after "after " (nullptr: accepted then)
  bool fresh;              // refused when the generation has a row table, column shifts or slots already
  bool session;            // refused outside a slotted session
};
#define ZN_GE_ADMIT_FILLS "zn_gen_admit fills the slots"
static const GenEntryRule kGenEntryRules[GE_NENTRIES] = {
    {"zn_prefill", false, false, ZN_GE_ADMIT_FILLS, nullptr, false, false},
    {"zn_prefill_rows", false, false, ZN_GE_ADMIT_FILLS, nullptr, false, false},
    {"zn_gen_set_rows", false, false, ZN_GE_ADMIT_FILLS, "zn_prefill: the table belongs between zn_gen_begin and the generation's prefill", false, false},
    {"zn_gen_set_prefix_rows", false, false, ZN_GE_ADMIT_FILLS, "zn_prefill: the prefix lengths belong between zn_gen_begin and the generation's prefill", false, false},
    {"zn_gen_open_slots", false, false, nullptr, "zn_prefill: a session is opened between zn_gen_begin and the generation's first prefill", true, false},
    {"zn_gen_admit", false, false, nullptr, nullptr, false, true},
    {"zn_gen_retire", false, false, nullptr, nullptr, false, true},
    {"zn_gen_row_state", false, false, nullptr, nullptr, false, true},
    // ended_ok: zn_sample_first alone never asked whether zn_gen_end had been called.  Kept as it was found, not chosen.
    {"zn_sample_first", false, true, "zn_gen_admit samples each slot's first frame", nullptr, false, false},
    {"zn_decode_steps", false, false, nullptr, nullptr, false, false},
    {"zn_gen_bind_kv_fp8", false, false, nullptr, "the generation's prefill: the code caches are bound between zn_gen_begin and the first prefill or admission", false, false},
    {"zn_set_mlp_fp8", true, false, nullptr, nullptr, false, false},
    {"zn_set_mamba_fp8", true, false, nullptr, nullptr, false, false},
    {"zn_set_kv_fp8", true, false, nullptr, nullptr, false, false},
    {"zn_set_kv_fp8_only", true, false, nullptr, nullptr, false, false},
};
#undef ZN_GE_ADMIT_FILLS

// May entry point `e` be called on `g` now?  ZN_OK, or ZN_ERR_STATE and why.
static inline GenErr gen_call_order(const GenHost& g, GenEntry e) {
  const GenEntryRule& r = kGenEntryRules[e];
  if (r.outside) return g.running() ? gen_fail(ZN_ERR_STATE, "%s inside a generation (between zn_gen_begin and zn_gen_end)", r.name) : GenErr{};
  if (!g.gen_active || (g.gen_ended && !r.ended_ok)) return gen_fail(ZN_ERR_STATE, "%s before zn_gen_begin", r.name);
  if (r.slotted && g.slots_open) return gen_fail(ZN_ERR_STATE, "%s in a slotted session: %s", r.name, r.slotted);
  if (r.prefilled && g.gen_prefilled) return gen_fail(ZN_ERR_STATE, "%s after %s", r.name, r.prefilled);
  if (r.fresh && (g.slots_open || g.rows_set || g.prefix_set)) return gen_fail(ZN_ERR_STATE, "%s: the generation already has a row table, column shifts or slots", r.name);
  if (r.session && !g.slots_open) return gen_fail(ZN_ERR_STATE, "%s: the generation is not a slotted session (zn_gen_open_slots)", r.name);
  return GenErr{};
}

// ------------------------------------------------------------------------------------------------ request rules
// A guided entry of a generation begun without guidance (a mixed generation): legal exactly when it names a row pair
// (reserved[0] = cond_row + 1, reserved[1] = uncond_row + 1), both rows in range and distinct, one of them the entry's own, and the partner's
// entry - present in the same call - names the same pair with byte-equal parameters.  `slot_of(j)`: the row of entry j of the call; `entry(j)`.
// Returns the index of the partner's entry, or -1 with `why` set.
template <typename SlotOf, typename Entry>
static int pair_partner(int j, int n, int B, SlotOf slot_of, Entry entry, const char** why) {
  const zn_row_params& r = entry(j);
  const int own = slot_of(j), rc = r.reserved[0] - 1, ru = r.reserved[1] - 1;
  if (r.reserved[0] <= 0 && r.reserved[1] <= 0) { *why = "has a cfg_scale != 1 in a generation begun without guidance and names no row pair"; return -1; }
  if (rc < 0 || rc >= B || ru < 0 || ru >= B) { *why = "names a row pair out of range"; return -1; }
  if (rc == ru) { *why = "names the same row twice as its pair"; return -1; }
  if (rc != own && ru != own) { *why = "names a row pair that does not hold its own row"; return -1; }
  const int other = rc == own ? ru : rc;
  for (int k = 0; k < n; ++k) {
    if (slot_of(k) != other) continue;
    if (memcmp(&entry(k), &r, sizeof(zn_row_params)) != 0) { *why = "and its pair's other row differ in their entries (the same pair, byte-equal parameters)"; return -1; }
    return k;
  }
  *why = "names a row pair whose other row is not part of this call";
  return -1;
}

// The words in which the two callers of gen_row_entry differ.
struct GenRowNouns { const char *fn, *row, *gen, *scale_note; };
static const GenRowNouns kSetRowsNouns = {"zn_gen_set_rows", "utterance", "generation", " (cfg_scale == 1 for every row or for none)"};
static const GenRowNouns kAdmitNouns = {"zn_gen_admit", "slot", "session", ""};

// Entry j of the n entries of a zn_gen_set_rows / zn_gen_admit call over B rows: the penalty window, the caller's own bounds of max_new_tokens (`budget(r)`,
// asked second), then cfg_scale against the layout zn_gen_begin fixed and the row pair.  *partner: the entry of the pair's other row, -1 where entry j names no pair.
template <typename SlotOf, typename Entry, typename Budget>
static GenErr gen_row_entry(const GenHost& g, const GenRowNouns& w, int j, int n, int B, SlotOf slot_of, Entry entry, Budget budget, int* partner) {
  const zn_row_params& r = entry(j);
  const int id = slot_of(j);
  *partner = -1;
  if (r.sp.repetition_penalty_window < 0 || r.sp.repetition_penalty_window > 64) return gen_fail(ZN_ERR_ARG, "%s: %s %d: repetition_penalty_window out of range", w.fn, w.row, id);
  if (const GenErr e = budget(r); e.code) return e;
  const bool named = r.reserved[0] != 0 || r.reserved[1] != 0;
  if (named && (g.guided() || r.cfg_scale == 1.0f)) {
    char where[64] = "at cfg_scale == 1";
    if (g.guided()) snprintf(where, sizeof where, "in a %s begun with guidance", w.gen);
    return gen_fail(ZN_ERR_ARG, "%s: %s %d names a row pair %s (pairs belong to guided entries of a %s begun with cfg_scale == 1)", w.fn, w.row, id, where, w.gen);
  }
  if (!g.guided() && r.cfg_scale != 1.0f) {
    const char* why = nullptr;
    if ((*partner = pair_partner(j, n, B, slot_of, entry, &why)) < 0) return gen_fail(ZN_ERR_ARG, "%s: %s %d %s", w.fn, w.row, id, why);
  } else if ((r.cfg_scale == 1.0f) == g.guided())
    return gen_fail(ZN_ERR_ARG, "%s: %s %d has cfg_scale %g in a %s begun %s guidance%s", w.fn, w.row, id, (double)r.cfg_scale, w.gen, g.guided() ? "with" : "without", w.scale_note);
  return GenErr{};
}

// zn_gen_set_rows.  rem[b] = max_new_tokens_b + n_q - 1; *pairs: some entry names a row pair.
static inline GenErr gen_check_set_rows(const GenHost& g, int nq, const zn_row_params* rows_host, int n, std::vector<int>* rem, bool* pairs) {
  if (!rows_host) return gen_fail(ZN_ERR_ARG, "zn_gen_set_rows: null argument");
  if (n != g.batch) return gen_fail(ZN_ERR_ARG, "zn_gen_set_rows: %d entries for a generation of %d utterances", n, g.batch);
  const int top = g.t_total - g.offset0 - nq + 1;   // zn_gen_begin's max_new_tokens (t_total = prefix + max_new_tokens + n_q)
  rem->assign(n, 0);
  *pairs = false;
  for (int b = 0; b < n; ++b) {
    int partner;
    const GenErr e = gen_row_entry(g, kSetRowsNouns, b, n, n, [](int j) { return j; }, [&](int j) -> const zn_row_params& { return rows_host[j]; },
                                   [&](const zn_row_params& r) {
                                     return r.max_new_tokens < 1 || r.max_new_tokens > top
                                                ? gen_fail(ZN_ERR_ARG, "zn_gen_set_rows: utterance %d: max_new_tokens %d not in 1..%d (the generation's own)", b, r.max_new_tokens, top)
                                                : GenErr{};
                                   }, &partner);
    if (e.code) return e;
    *pairs = *pairs || partner >= 0;
    (*rem)[b] = rows_host[b].max_new_tokens + nq - 1;
  }
  return GenErr{};
}

// zn_gen_set_prefix_rows.  shift[b] = p_b - p_call (<= 0); *any: some shift is not 0.
static inline GenErr gen_check_prefix_rows(const GenHost& g, const int32_t* prefix_len_host, int n, std::vector<int>* shift, bool* any) {
  if (!prefix_len_host) return gen_fail(ZN_ERR_ARG, "zn_gen_set_prefix_rows: null argument");
  if (n != g.batch) return gen_fail(ZN_ERR_ARG, "zn_gen_set_prefix_rows: %d entries for a generation of %d utterances", n, g.batch);
  const int p_call = g.offset0 - 1;        // zn_gen_begin's offset0 = the longest prefix + 1
  shift->assign(n, 0);
  bool longest = false;
  *any = false;
  for (int b = 0; b < n; ++b) {
    const int p = prefix_len_host[b];
    if (p < 0 || p > p_call) return gen_fail(ZN_ERR_ARG, "zn_gen_set_prefix_rows: utterance %d: prefix length %d not in 0..%d (zn_gen_begin's offset0 - 1)", b, p, p_call);
    (*shift)[b] = p - p_call;
    longest = longest || p == p_call; *any = *any || p != p_call;
  }
  if (!longest) return gen_fail(ZN_ERR_ARG, "zn_gen_set_prefix_rows: no utterance has the %d prefix frames zn_gen_begin's offset0 stands for", p_call);
  return GenErr{};
}

// zn_prefill_rows' lengths.  *uniform: every row holds S positions (zn_prefill's launches); *unequal2: two unguided rows of different lengths.
static inline GenErr gen_check_prefill_rows(const GenHost& g, const int32_t* row_len, int S, bool* uniform, bool* unequal2) {
  const int R = g.rows, B = g.batch;
  int hi = 0;
  *uniform = true;
  for (int r = 0; r < R; ++r) {
    if (row_len[r] < 1 || row_len[r] > S) return gen_fail(ZN_ERR_ARG, "zn_prefill_rows: row %d holds %d positions, not in 1..%d", r, row_len[r], S);
    if (row_len[r] > hi) hi = row_len[r];
    *uniform = *uniform && row_len[r] == S;
  }
  if (hi != S) return gen_fail(ZN_ERR_ARG, "zn_prefill_rows: the longest row holds %d positions, S is %d (no row may be all padding at its end)", hi, S);
  if (R == 2 * B)
    for (int b = 0; b < B; ++b)
      if (row_len[b] != row_len[B + b])
        return gen_fail(ZN_ERR_ARG, "zn_prefill_rows: utterance %d has %d conditional and %d unconditional positions (a guided pair advances in lockstep)", b, row_len[b], row_len[B + b]);
  *unequal2 = R == 2 && B == 2 && row_len[0] != row_len[1];
  return GenErr{};
}

// zn_gen_open_slots' arguments.
static inline GenErr gen_check_open_slots(const GenHost& g, int slack) {
  if (slack < 0) return gen_fail(ZN_ERR_ARG, "zn_gen_open_slots: slack %d < 0", slack);
  if (g.len_hi != 0) return gen_fail(ZN_ERR_ARG, "zn_gen_open_slots: the session's lengths array must be zero (every slot begins idle)");
  return GenErr{};
}

// zn_gen_admit, the call as a whole (have_ptrs: neither the requests nor the hidden states are NULL) ...
static inline GenErr gen_check_admit_call(const GenHost& g, bool have_ptrs, int n, int S) {
  if (!have_ptrs || n < 1 || n > g.batch) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: null argument or %d requests for a session of %d slots", n, g.batch);
  if (S < 1 || S > g.max_len) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: bad S=%d (max_len %d)", S, g.max_len);
  if (g.stop_pending) return gen_fail(ZN_ERR_STATE, "zn_gen_admit: steps are still owed to a deferred stop read-back (zn_all_stopped_end first)");
  return GenErr{};
}
// ... and its requests.  *uniform: every request holds S positions.
static inline GenErr gen_check_admit(const GenHost& g, int nq, const zn_admit* a, int n, int S, bool* uniform) {
  const int B = g.batch;
  bool longest = false;
  *uniform = true;
  for (int j = 0; j < n; ++j) {
    const zn_admit& q = a[j];
    if (q.slot < 0 || q.slot >= B) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d out of range 0..%d", q.slot, B - 1);
    for (int k = 0; k < j; ++k) if (a[k].slot == q.slot) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d named twice in one call", q.slot);
    if (g.slot_busy[q.slot]) return gen_fail(ZN_ERR_STATE, "zn_gen_admit: slot %d is busy (zn_gen_retire first)", q.slot);
    if (q.row_len < 1 || q.row_len > S) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d: %d positions, not in 1..%d", q.slot, q.row_len, S);
    if (q.prefix_len < 0 || q.prefix_len > q.row_len - 2)
      return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d: prefix length %d not in 0..%d (row_len = conditioning + prefix + 1)", q.slot, q.prefix_len, q.row_len - 2);
    int k;
    const GenErr e = gen_row_entry(g, kAdmitNouns, j, n, B, [&](int i) { return (int)a[i].slot; }, [&](int i) -> const zn_row_params& { return a[i].params; },
                                   [&](const zn_row_params& r) {
                                     if (r.max_new_tokens < 1) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d: max_new_tokens %d < 1", q.slot, r.max_new_tokens);
                                     if ((long long)q.row_len - 1 + r.max_new_tokens + nq + g.slot_slack > g.max_len)
                                       return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d: %d positions + %d frames + %d + slack %d exceed the session's max_len %d", q.slot, q.row_len - 1,
                                                       r.max_new_tokens, nq, g.slot_slack, g.max_len);
                                     if ((long long)q.prefix_len + r.max_new_tokens + nq + g.slot_slack > g.t_total)
                                       return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d: %d prefix frames + %d frames + %d + slack %d exceed the code buffer's width %d", q.slot, q.prefix_len,
                                                       r.max_new_tokens, nq, g.slot_slack, g.t_total);
                                     return GenErr{};
                                   }, &k);
    if (e.code) return e;
    if (k >= 0 && (a[k].row_len != q.row_len || a[k].prefix_len != q.prefix_len))
      return gen_fail(ZN_ERR_ARG, "zn_gen_admit: slot %d and its pair's other slot %d differ in row_len or prefix_len", q.slot, a[k].slot);
    longest = longest || q.row_len == S;
    *uniform = *uniform && q.row_len == S;
  }
  if (!longest) return gen_fail(ZN_ERR_ARG, "zn_gen_admit: no request holds S = %d positions (no row may be all padding at its end)", S);
  return GenErr{};
}

// zn_decode_steps in a session: no busy slot may pass max_len.
static inline GenErr gen_check_steps(const GenHost& g, int n) {
  if (g.slots_open)
    for (int b = 0; b < g.batch; ++b)
      if (g.slot_busy[b] && g.slot_len[b] + n > g.max_len)
        return gen_fail(ZN_ERR_STATE, "zn_decode_steps: %d steps would take slot %d (%d positions) past max_len %d: retire it first", n, b, g.slot_len[b], g.max_len);
  return GenErr{};
}

static inline GenErr gen_check_retire(const GenHost& g, int slot) {
  if (slot < 0 || slot >= g.batch) return gen_fail(ZN_ERR_ARG, "zn_gen_retire: slot %d out of range 0..%d", slot, g.batch - 1);
  if (!g.slot_busy[slot]) return gen_fail(ZN_ERR_STATE, "zn_gen_retire: slot %d is idle already", slot);
  return GenErr{};
}

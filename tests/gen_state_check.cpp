// CPU walk of a generation's host rules (zonos_amd/csrc/zn_gen_state.h) against the codes and messages the entry points of zn_api.hip carried before the header
// existed: see tests/test_gen_state.py.  Every expected string below is typed in from that code; nothing here is computed by the header.  Each refusal is also printed as
// "label | code | message": tools/gen_refusals.py prints the same calls made through the C ABI.
#include "zn_gen_state.h"

#include <climits>
#include <initializer_list>
#include <string>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 30) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void accepted(const char* label, const GenErr& e) { CHECK(e.code == ZN_OK && e.msg[0] == 0, "%s: expected acceptance, got %d \"%s\"", label, e.code, e.msg); }
static void refused(const char* label, const GenErr& e, int code, const char* msg) {
  CHECK(e.code == code && strcmp(e.msg, msg) == 0, "%s: expected %d \"%s\", got %d \"%s\"", label, code, msg, e.code, e.msg);
  printf("%s | %d | %s\n", label, e.code, e.msg);
}

static const int NQ = 9;
static zn_sampling sampling(float penalty = 1.f, int window = 2) {
  zn_sampling sp{};
  sp.repetition_penalty = penalty; sp.repetition_penalty_window = window;
  return sp;
}
static GenHost begun(int batch, bool guided, int max_len, int t_total, int offset0, int max_new) {
  GenHost g;
  g.begin(batch, guided ? 2 * batch : batch, max_len, t_total, offset0, max_new, guided ? 2.f : 1.f, sampling(), nullptr, nullptr);
  g.gen_active = true;
  return g;
}
static zn_row_params entry(float cfg_scale, int max_new, float penalty = 2.f, int w0 = 0, int w1 = 0, int window = 2) {
  zn_row_params r{};
  r.sp = sampling(penalty, window); r.cfg_scale = cfg_scale; r.max_new_tokens = max_new; r.reserved[0] = w0; r.reserved[1] = w1;
  return r;
}
static zn_row_params pair_entry(int o, int f, int n = 6, float penalty = 3.f) { return entry(2.f, n, penalty, o + 1, f + 1); }
static zn_admit request(int slot, int row_len, int prefix_len, const zn_row_params& p) {
  zn_admit a{};
  a.slot = slot; a.row_len = row_len; a.prefix_len = prefix_len; a.params = p;
  return a;
}

// ------------------------------------------------------------------------------------------------ 1. call order
static void call_order() {
  enum { NONE, BEGUN, ROWS, PREFIX, PREFILLED, SESSION, BUSY, ENDED, NSTATES };
  static const char* const state_name[NSTATES] = {"no generation", "begun", "row table set", "prefix shifts set", "prefilled", "session opened", "session with a busy slot", "ended"};
  GenHost st[NSTATES];
  for (int s = BEGUN; s < NSTATES; ++s) st[s] = begun(2, true, 48, 42, 1, 8);
  st[ROWS].rows_set = true;
  st[PREFIX].prefix_set = true;
  st[PREFILLED].gen_prefilled = true;
  st[SESSION].open_slots(24);
  st[BUSY].open_slots(24);
  const zn_admit a = request(0, 8, 0, entry(2.f, 8));
  st[BUSY].slots_admitted(&a, 1); st[BUSY].gen_prefilled = true;      // (zn_gen_admit marks the generation prefilled)
  st[ENDED].gen_ended = true;
  const char* const ok = nullptr;
#define BEFORE(fn) fn " before zn_gen_begin"
#define SLOTTED(fn) fn " in a slotted session: zn_gen_admit fills the slots"
#define NO_SESSION(fn) fn ": the generation is not a slotted session (zn_gen_open_slots)"
#define INSIDE(fn) fn " inside a generation (between zn_gen_begin and zn_gen_end)"
#define FIRST_SLOTTED "zn_sample_first in a slotted session: zn_gen_admit samples each slot's first frame"
#define ROWS_AFTER "zn_gen_set_rows after zn_prefill: the table belongs between zn_gen_begin and the generation's prefill"
#define PREFIX_AFTER "zn_gen_set_prefix_rows after zn_prefill: the prefix lengths belong between zn_gen_begin and the generation's prefill"
#define OPEN_AFTER "zn_gen_open_slots after zn_prefill: a session is opened between zn_gen_begin and the generation's first prefill"
#define OPEN_ALREADY "zn_gen_open_slots: the generation already has a row table, column shifts or slots"
#define BIND_AFTER "zn_gen_bind_kv_fp8 after the generation's prefill: the code caches are bound between zn_gen_begin and the first prefill or admission"
  static const struct { GenEntry e; const char* name; const char* want[NSTATES]; } rows[] = {
      //                                            none                          begun  rows  prefix  prefilled  session  busy  ended
      {GE_PREFILL, "zn_prefill", {BEFORE("zn_prefill"), ok, ok, ok, ok, SLOTTED("zn_prefill"), SLOTTED("zn_prefill"), BEFORE("zn_prefill")}},
      {GE_PREFILL_ROWS, "zn_prefill_rows", {BEFORE("zn_prefill_rows"), ok, ok, ok, ok, SLOTTED("zn_prefill_rows"), SLOTTED("zn_prefill_rows"), BEFORE("zn_prefill_rows")}},
      {GE_SET_ROWS, "zn_gen_set_rows", {BEFORE("zn_gen_set_rows"), ok, ok, ok, ROWS_AFTER, SLOTTED("zn_gen_set_rows"), SLOTTED("zn_gen_set_rows"), BEFORE("zn_gen_set_rows")}},
      {GE_SET_PREFIX_ROWS, "zn_gen_set_prefix_rows",
       {BEFORE("zn_gen_set_prefix_rows"), ok, ok, ok, PREFIX_AFTER, SLOTTED("zn_gen_set_prefix_rows"), SLOTTED("zn_gen_set_prefix_rows"), BEFORE("zn_gen_set_prefix_rows")}},
      {GE_OPEN_SLOTS, "zn_gen_open_slots", {BEFORE("zn_gen_open_slots"), ok, OPEN_ALREADY, OPEN_ALREADY, OPEN_AFTER, OPEN_ALREADY, OPEN_AFTER, BEFORE("zn_gen_open_slots")}},
      {GE_ADMIT, "zn_gen_admit", {BEFORE("zn_gen_admit"), NO_SESSION("zn_gen_admit"), NO_SESSION("zn_gen_admit"), NO_SESSION("zn_gen_admit"), NO_SESSION("zn_gen_admit"), ok, ok, BEFORE("zn_gen_admit")}},
      {GE_RETIRE, "zn_gen_retire", {BEFORE("zn_gen_retire"), NO_SESSION("zn_gen_retire"), NO_SESSION("zn_gen_retire"), NO_SESSION("zn_gen_retire"), NO_SESSION("zn_gen_retire"), ok, ok, BEFORE("zn_gen_retire")}},
      {GE_ROW_STATE, "zn_gen_row_state",
       {BEFORE("zn_gen_row_state"), NO_SESSION("zn_gen_row_state"), NO_SESSION("zn_gen_row_state"), NO_SESSION("zn_gen_row_state"), NO_SESSION("zn_gen_row_state"), ok, ok, BEFORE("zn_gen_row_state")}},
      {GE_SAMPLE_FIRST, "zn_sample_first", {BEFORE("zn_sample_first"), ok, ok, ok, ok, FIRST_SLOTTED, FIRST_SLOTTED, ok}},      // an ended generation is accepted: as found
      {GE_DECODE_STEPS, "zn_decode_steps", {BEFORE("zn_decode_steps"), ok, ok, ok, ok, ok, ok, BEFORE("zn_decode_steps")}},
      {GE_BIND_KV_FP8, "zn_gen_bind_kv_fp8", {BEFORE("zn_gen_bind_kv_fp8"), ok, ok, ok, BIND_AFTER, ok, BIND_AFTER, BEFORE("zn_gen_bind_kv_fp8")}},
      {GE_SET_MLP_FP8, "zn_set_mlp_fp8", {ok, INSIDE("zn_set_mlp_fp8"), INSIDE("zn_set_mlp_fp8"), INSIDE("zn_set_mlp_fp8"), INSIDE("zn_set_mlp_fp8"), INSIDE("zn_set_mlp_fp8"), INSIDE("zn_set_mlp_fp8"), ok}},
      {GE_SET_MAMBA_FP8, "zn_set_mamba_fp8",
       {ok, INSIDE("zn_set_mamba_fp8"), INSIDE("zn_set_mamba_fp8"), INSIDE("zn_set_mamba_fp8"), INSIDE("zn_set_mamba_fp8"), INSIDE("zn_set_mamba_fp8"), INSIDE("zn_set_mamba_fp8"), ok}},
      {GE_SET_KV_FP8, "zn_set_kv_fp8", {ok, INSIDE("zn_set_kv_fp8"), INSIDE("zn_set_kv_fp8"), INSIDE("zn_set_kv_fp8"), INSIDE("zn_set_kv_fp8"), INSIDE("zn_set_kv_fp8"), INSIDE("zn_set_kv_fp8"), ok}},
      {GE_SET_KV_FP8_ONLY, "zn_set_kv_fp8_only",
       {ok, INSIDE("zn_set_kv_fp8_only"), INSIDE("zn_set_kv_fp8_only"), INSIDE("zn_set_kv_fp8_only"), INSIDE("zn_set_kv_fp8_only"), INSIDE("zn_set_kv_fp8_only"), INSIDE("zn_set_kv_fp8_only"), ok}},
  };
  static_assert(sizeof rows / sizeof rows[0] == GE_NENTRIES, "one row per entry point of the table");
  for (const auto& r : rows)
    for (int s = 0; s < NSTATES; ++s) {
      const std::string label = std::string("order: ") + r.name + ", " + state_name[s];
      CHECK(strcmp(kGenEntryRules[r.e].name, r.name) == 0, "the table's row %d is %s", (int)r.e, kGenEntryRules[r.e].name);
      if (r.want[s]) refused(label.c_str(), gen_call_order(st[s], r.e), ZN_ERR_STATE, r.want[s]);
      else accepted(label.c_str(), gen_call_order(st[s], r.e));
    }
}

// ------------------------------------------------------------------------------------------------ 2, 3. request rules and what they derive
static GenErr set_rows(const GenHost& g, std::initializer_list<zn_row_params> rows, std::vector<int>* rem = nullptr, bool* pairs = nullptr) {
  std::vector<zn_row_params> t(rows);
  std::vector<int> r; bool p = false;
  const GenErr e = gen_check_set_rows(g, NQ, t.data(), (int)t.size(), &r, &p);
  if (rem) *rem = r;
  if (pairs) *pairs = p;
  return e;
}
static void set_rows_rules() {
  // tests/test_gpu_requests.py: two guided utterances, no prefix, max_new_tokens 8: t_total = 0 + 8 + n_q, offset0 = 1
  const GenHost g = begun(2, true, 32, 17, 1, 8);
  const zn_row_params row = entry(2.f, 5);
  std::vector<int> rem; bool pairs = true;
  refused("set_rows: null", gen_check_set_rows(g, NQ, nullptr, 2, &rem, &pairs), ZN_ERR_ARG, "zn_gen_set_rows: null argument");
  refused("set_rows: 3 entries", set_rows(g, {row, row, row}), ZN_ERR_ARG, "zn_gen_set_rows: 3 entries for a generation of 2 utterances");
  refused("set_rows: cfg_scale 1 with guidance", set_rows(g, {row, entry(1.f, 5)}), ZN_ERR_ARG,
          "zn_gen_set_rows: utterance 1 has cfg_scale 1 in a generation begun with guidance (cfg_scale == 1 for every row or for none)");
  refused("set_rows: cfg_scale 1 twice with guidance", set_rows(g, {entry(1.f, 5), entry(1.f, 5)}), ZN_ERR_ARG,
          "zn_gen_set_rows: utterance 0 has cfg_scale 1 in a generation begun with guidance (cfg_scale == 1 for every row or for none)");
  refused("set_rows: max_new_tokens 0", set_rows(g, {entry(2.f, 0), row}), ZN_ERR_ARG, "zn_gen_set_rows: utterance 0: max_new_tokens 0 not in 1..8 (the generation's own)");
  refused("set_rows: max_new_tokens budget + 1", set_rows(g, {row, entry(2.f, 9)}), ZN_ERR_ARG, "zn_gen_set_rows: utterance 1: max_new_tokens 9 not in 1..8 (the generation's own)");
  refused("set_rows: window 65", set_rows(g, {entry(2.f, 5, 2.f, 0, 0, 65), row}), ZN_ERR_ARG, "zn_gen_set_rows: utterance 0: repetition_penalty_window out of range");
  refused("set_rows: window -1", set_rows(g, {row, entry(2.f, 5, 2.f, 0, 0, -1)}), ZN_ERR_ARG, "zn_gen_set_rows: utterance 1: repetition_penalty_window out of range");
  refused("set_rows: window before budget", set_rows(g, {entry(2.f, 0, 2.f, 0, 0, 65), row}), ZN_ERR_ARG, "zn_gen_set_rows: utterance 0: repetition_penalty_window out of range");
  refused("set_rows: a pair with guidance", set_rows(g, {pair_entry(0, 1), pair_entry(0, 1)}), ZN_ERR_ARG,
          "zn_gen_set_rows: utterance 0 names a row pair in a generation begun with guidance (pairs belong to guided entries of a generation begun with cfg_scale == 1)");
  accepted("set_rows: windows 0 and 64", set_rows(g, {entry(2.f, 5, 2.f, 0, 0, 0), entry(2.f, 5, 2.f, 0, 0, 64)}));
  accepted("set_rows: max_new_tokens budget and 1", set_rows(g, {entry(2.f, 8), entry(2.f, 1)}, &rem, &pairs));
  CHECK(rem == std::vector<int>({16, 9}) && !pairs, "rem %d %d pairs %d", rem[0], rem[1], (int)pairs);

  // tests/test_gpu_mixed.py: four rows begun without guidance
  const GenHost u = begun(4, false, 32, 17, 1, 8);
  const zn_row_params U = entry(1.f, 5);
#define UTT(b, why) "zn_gen_set_rows: utterance " #b " " why
#define DIFFER "and its pair's other row differ in their entries (the same pair, byte-equal parameters)"
  refused("set_rows: guided, no pair named", set_rows(u, {U, entry(2.f, 6, 3.f), U, U}), ZN_ERR_ARG, UTT(1, "has a cfg_scale != 1 in a generation begun without guidance and names no row pair"));
  refused("set_rows: the partner is another request", set_rows(u, {U, pair_entry(1, 3), U, U}), ZN_ERR_ARG, UTT(1, DIFFER));
  refused("set_rows: the partner does not name the pair", set_rows(u, {pair_entry(0, 1), U, U, U}), ZN_ERR_ARG, UTT(0, DIFFER));
  refused("set_rows: the partner's penalty differs", set_rows(u, {U, pair_entry(1, 3), U, pair_entry(1, 3, 6, 4.f)}), ZN_ERR_ARG, UTT(1, DIFFER));
  refused("set_rows: the partner's budget differs", set_rows(u, {U, pair_entry(1, 3), U, pair_entry(1, 3, 7)}), ZN_ERR_ARG, UTT(1, DIFFER));
  refused("set_rows: a pair row out of range", set_rows(u, {U, pair_entry(1, 4), U, U}), ZN_ERR_ARG, UTT(1, "names a row pair out of range"));
  refused("set_rows: a negative pair word", set_rows(u, {U, entry(2.f, 6, 3.f, 2, -1), U, U}), ZN_ERR_ARG, UTT(1, "names a row pair out of range"));
  refused("set_rows: the same row twice", set_rows(u, {U, pair_entry(1, 1), U, U}), ZN_ERR_ARG, UTT(1, "names the same row twice as its pair"));
  refused("set_rows: a pair of other rows", set_rows(u, {U, pair_entry(2, 3), pair_entry(2, 3), pair_entry(2, 3)}), ZN_ERR_ARG, UTT(1, "names a row pair that does not hold its own row"));
  refused("set_rows: a pair at cfg_scale 1", set_rows(u, {entry(1.f, 5, 2.f, 1, 2), entry(1.f, 5, 2.f, 1, 2), U, U}), ZN_ERR_ARG,
          "zn_gen_set_rows: utterance 0 names a row pair at cfg_scale == 1 (pairs belong to guided entries of a generation begun with cfg_scale == 1)");
  pairs = true;
  accepted("set_rows: no pair without guidance", set_rows(u, {U, U, U, U}, &rem, &pairs));
  CHECK(!pairs, "no entry names a pair");
  accepted("set_rows: a pair, f < o, rows apart", set_rows(u, {U, pair_entry(3, 1), U, pair_entry(3, 1)}, &rem, &pairs));
  CHECK(pairs && rem == std::vector<int>({13, 14, 13, 14}), "pairs %d rem %d %d %d %d", (int)pairs, rem[0], rem[1], rem[2], rem[3]);
  accepted("set_rows: a pair, o < f, adjacent", set_rows(u, {pair_entry(0, 1), pair_entry(0, 1), U, U}, nullptr, &pairs));
  CHECK(pairs, "the entries name a pair");
  accepted("set_rows: two pairs interleaved", set_rows(u, {pair_entry(0, 2), pair_entry(3, 1, 4), pair_entry(0, 2), pair_entry(3, 1, 4)}, nullptr, &pairs));
  CHECK(pairs, "the entries name two pairs");
}

static void prefix_rows_rules() {
  // tests/test_gpu_prefix_rows.py: two guided utterances, the longest prefix 5 frames: offset0 = 6
  const GenHost g = begun(2, true, 32, 22, 6, 8);
  std::vector<int> shift; bool any = false;
  auto call = [&](std::initializer_list<int32_t> p) { std::vector<int32_t> v(p); return gen_check_prefix_rows(g, v.data(), (int)v.size(), &shift, &any); };
  refused("prefix_rows: null", gen_check_prefix_rows(g, nullptr, 2, &shift, &any), ZN_ERR_ARG, "zn_gen_set_prefix_rows: null argument");
  refused("prefix_rows: 3 entries", call({5, 2, 0}), ZN_ERR_ARG, "zn_gen_set_prefix_rows: 3 entries for a generation of 2 utterances");
  refused("prefix_rows: -1", call({5, -1}), ZN_ERR_ARG, "zn_gen_set_prefix_rows: utterance 1: prefix length -1 not in 0..5 (zn_gen_begin's offset0 - 1)");
  refused("prefix_rows: p_call + 1", call({6, 5}), ZN_ERR_ARG, "zn_gen_set_prefix_rows: utterance 0: prefix length 6 not in 0..5 (zn_gen_begin's offset0 - 1)");
  refused("prefix_rows: none is the longest", call({4, 2}), ZN_ERR_ARG, "zn_gen_set_prefix_rows: no utterance has the 5 prefix frames zn_gen_begin's offset0 stands for");
  accepted("prefix_rows: 5 and 2", call({5, 2}));
  CHECK(shift == std::vector<int>({0, -3}) && any, "shift %d %d any %d", shift[0], shift[1], (int)any);
  accepted("prefix_rows: 0 and p_call", call({0, 5}));
  CHECK(shift == std::vector<int>({-5, 0}) && any, "shift %d %d any %d", shift[0], shift[1], (int)any);
  accepted("prefix_rows: every prefix the longest", call({5, 5}));
  CHECK(shift == std::vector<int>({0, 0}) && !any, "shift %d %d any %d", shift[0], shift[1], (int)any);
}

static void prefill_rows_rules() {
  // tests/test_gpu_ragged.py: two guided utterances (rows: cond 0, cond 1, uncond 0, uncond 1), S = 9
  const GenHost g = begun(2, true, 25, 12, 1, 4);
  bool uniform = false, unequal2 = true;
  auto call = [&](const GenHost& gen, std::initializer_list<int32_t> l) { std::vector<int32_t> v(l); uniform = false; unequal2 = true; return gen_check_prefill_rows(gen, v.data(), 9, &uniform, &unequal2); };
  refused("prefill_rows: a pair out of lockstep", call(g, {9, 5, 9, 6}), ZN_ERR_ARG,
          "zn_prefill_rows: utterance 1 has 5 conditional and 6 unconditional positions (a guided pair advances in lockstep)");
  refused("prefill_rows: 0 positions", call(g, {9, 0, 9, 0}), ZN_ERR_ARG, "zn_prefill_rows: row 1 holds 0 positions, not in 1..9");
  refused("prefill_rows: S + 1 positions", call(g, {9, 10, 9, 10}), ZN_ERR_ARG, "zn_prefill_rows: row 1 holds 10 positions, not in 1..9");
  refused("prefill_rows: no row of S positions", call(g, {8, 5, 8, 5}), ZN_ERR_ARG, "zn_prefill_rows: the longest row holds 8 positions, S is 9 (no row may be all padding at its end)");
  accepted("prefill_rows: 1 and S", call(g, {9, 1, 9, 1}));
  CHECK(!uniform && !unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  accepted("prefill_rows: every row S", call(g, {9, 9, 9, 9}));
  CHECK(uniform && !unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  const GenHost u2 = begun(2, false, 25, 12, 1, 4), u4 = begun(4, false, 25, 12, 1, 4), g1 = begun(1, true, 25, 12, 1, 4);
  accepted("prefill_rows: two unguided rows, unequal", call(u2, {9, 5}));
  CHECK(!uniform && unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  accepted("prefill_rows: two unguided rows, equal", call(u2, {9, 9}));
  CHECK(uniform && !unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  accepted("prefill_rows: four unguided rows", call(u4, {9, 5, 9, 9}));
  CHECK(!uniform && !unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  accepted("prefill_rows: one guided pair", call(g1, {9, 9}));
  CHECK(uniform && !unequal2, "uniform %d unequal2 %d", (int)uniform, (int)unequal2);
  refused("prefill_rows: one guided pair out of lockstep", call(g1, {9, 5}), ZN_ERR_ARG,
          "zn_prefill_rows: utterance 0 has 9 conditional and 5 unconditional positions (a guided pair advances in lockstep)");
}

// ------------------------------------------------------------------------------------------------ 2, 4. sessions
static GenErr admit(const GenHost& g, std::initializer_list<zn_admit> a, int S, bool* uniform = nullptr) {
  std::vector<zn_admit> v(a);
  bool u = false;
  const GenErr e = gen_check_admit(g, NQ, v.data(), (int)v.size(), S, &u);
  if (uniform) *uniform = u;
  return e;
}
static void session_rules() {
  // tests/test_gpu_serve.py: a guided session of two slots, max_len 48, a code buffer 42 columns wide, slack 24
  GenHost g = begun(2, true, 48, 42, 1, 8);
  refused("open_slots: slack -1", gen_check_open_slots(g, -1), ZN_ERR_ARG, "zn_gen_open_slots: slack -1 < 0");
  g.len_hi = 3;
  refused("open_slots: lengths not zero", gen_check_open_slots(g, 24), ZN_ERR_ARG, "zn_gen_open_slots: the session's lengths array must be zero (every slot begins idle)");
  g.len_hi = 0;
  accepted("open_slots: slack 0", gen_check_open_slots(g, 0));
  accepted("open_slots: slack 24", gen_check_open_slots(g, 24));
  g.open_slots(24);
  CHECK(g.rows_set && g.prefix_set && g.slots_open && !g.pairs_set && g.slot_slack == 24 && g.slot_len == std::vector<int>({0, 0}) && g.slot_busy == std::vector<char>({0, 0}), "a guided session");
  const zn_row_params p8 = entry(2.f, 8);
  refused("admit: null", gen_check_admit_call(g, false, 1, 7), ZN_ERR_ARG, "zn_gen_admit: null argument or 1 requests for a session of 2 slots");
  refused("admit: no request", gen_check_admit_call(g, true, 0, 7), ZN_ERR_ARG, "zn_gen_admit: null argument or 0 requests for a session of 2 slots");
  refused("admit: 3 requests", gen_check_admit_call(g, true, 3, 7), ZN_ERR_ARG, "zn_gen_admit: null argument or 3 requests for a session of 2 slots");
  refused("admit: S 0", gen_check_admit_call(g, true, 1, 0), ZN_ERR_ARG, "zn_gen_admit: bad S=0 (max_len 48)");
  refused("admit: S max_len + 1", gen_check_admit_call(g, true, 1, 49), ZN_ERR_ARG, "zn_gen_admit: bad S=49 (max_len 48)");
  g.stop_pending = true;
  refused("admit: a stop read-back pending", gen_check_admit_call(g, true, 1, 7), ZN_ERR_STATE, "zn_gen_admit: steps are still owed to a deferred stop read-back (zn_all_stopped_end first)");
  g.stop_pending = false;
  accepted("admit: 2 requests, S max_len", gen_check_admit_call(g, true, 2, 48));
  accepted("admit: 1 request, S 1", gen_check_admit_call(g, true, 1, 1));

  refused("admit: slot named twice", admit(g, {request(0, 7, 1, entry(2.f, 6)), request(0, 6, 0, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 0 named twice in one call");
  refused("admit: slot out of range", admit(g, {request(2, 7, 1, entry(2.f, 6))}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 2 out of range 0..1");
  refused("admit: slot -1", admit(g, {request(-1, 7, 1, entry(2.f, 6))}, 7), ZN_ERR_ARG, "zn_gen_admit: slot -1 out of range 0..1");
  refused("admit: 0 positions", admit(g, {request(0, 7, 0, p8), request(1, 0, 0, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: 0 positions, not in 1..7");
  refused("admit: S + 1 positions", admit(g, {request(1, 8, 0, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: 8 positions, not in 1..7");
  refused("admit: prefix -1", admit(g, {request(1, 7, -1, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: prefix length -1 not in 0..5 (row_len = conditioning + prefix + 1)");
  refused("admit: prefix row_len - 1", admit(g, {request(1, 7, 6, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: prefix length 6 not in 0..5 (row_len = conditioning + prefix + 1)");
  refused("admit: 1 position has no prefix", admit(g, {request(0, 7, 0, p8), request(1, 1, 0, p8)}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: prefix length 0 not in 0..-1 (row_len = conditioning + prefix + 1)");
  refused("admit: window 65", admit(g, {request(1, 7, 0, entry(2.f, 8, 2.f, 0, 0, 65))}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: repetition_penalty_window out of range");
  refused("admit: window -1", admit(g, {request(1, 7, 0, entry(2.f, 8, 2.f, 0, 0, -1))}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: repetition_penalty_window out of range");
  refused("admit: max_new_tokens 0", admit(g, {request(1, 7, 0, entry(2.f, 0))}, 7), ZN_ERR_ARG, "zn_gen_admit: slot 1: max_new_tokens 0 < 1");
  refused("admit: past max_len by one", admit(g, {request(1, 9, 0, p8)}, 9), ZN_ERR_ARG, "zn_gen_admit: slot 1: 8 positions + 8 frames + 9 + slack 24 exceed the session's max_len 48");
  refused("admit: past the width by one", admit(g, {request(1, 4, 0, entry(2.f, 10))}, 4), ZN_ERR_ARG, "zn_gen_admit: slot 1: 0 prefix frames + 10 frames + 9 + slack 24 exceed the code buffer's width 42");
  refused("admit: max_new_tokens INT32_MAX", admit(g, {request(1, 4, 0, entry(2.f, INT_MAX))}, 4), ZN_ERR_ARG,
          "zn_gen_admit: slot 1: 3 positions + 2147483647 frames + 9 + slack 24 exceed the session's max_len 48");
  refused("admit: cfg_scale 1 with guidance", admit(g, {request(1, 6, 0, entry(1.f, 4))}, 6), ZN_ERR_ARG, "zn_gen_admit: slot 1 has cfg_scale 1 in a session begun with guidance");
  refused("admit: a pair with guidance", admit(g, {request(0, 7, 1, pair_entry(0, 1)), request(1, 7, 1, pair_entry(0, 1))}, 7), ZN_ERR_ARG,
          "zn_gen_admit: slot 0 names a row pair in a session begun with guidance (pairs belong to guided entries of a session begun with cfg_scale == 1)");
  refused("admit: no request holds S", admit(g, {request(0, 7, 0, p8)}, 8), ZN_ERR_ARG, "zn_gen_admit: no request holds S = 8 positions (no row may be all padding at its end)");
  bool uniform = false;
  accepted("admit: windows 0 and 64, max_new_tokens 1", admit(g, {request(0, 7, 0, entry(2.f, 1, 2.f, 0, 0, 0)), request(1, 7, 5, entry(2.f, 1, 2.f, 0, 0, 64))}, 7, &uniform));
  CHECK(uniform, "both requests hold S positions");
  accepted("admit: max_len met exactly", admit(g, {request(1, 8, 0, p8)}, 8));                     // 7 + 8 + 9 + 24 = 48
  accepted("admit: the width met exactly", admit(g, {request(1, 4, 0, entry(2.f, 9))}, 4));       // 0 + 9 + 9 + 24 = 42
  accepted("admit: both met exactly", admit(g, {request(1, 8, 1, p8)}, 8));                        // 7 + 8 + 9 + 24 = 48, 1 + 8 + 9 + 24 = 42
  refused("admit: the width passed by the prefix", admit(g, {request(1, 8, 2, p8)}, 8), ZN_ERR_ARG, "zn_gen_admit: slot 1: 2 prefix frames + 8 frames + 9 + slack 24 exceed the code buffer's width 42");
  accepted("admit: the shortest row and S", admit(g, {request(0, 2, 0, p8), request(1, 7, 0, p8)}, 7, &uniform));
  CHECK(!uniform, "one request is shorter than S");

  // 4. admit, steps, retire, admit: len_hi is the longest busy slot after every call
  refused("retire: slot out of range", gen_check_retire(g, 2), ZN_ERR_ARG, "zn_gen_retire: slot 2 out of range 0..1");
  refused("retire: slot -1", gen_check_retire(g, -1), ZN_ERR_ARG, "zn_gen_retire: slot -1 out of range 0..1");
  refused("retire: an idle slot", gen_check_retire(g, 1), ZN_ERR_STATE, "zn_gen_retire: slot 1 is idle already");
  const zn_admit a0 = request(0, 8, 0, p8), a1 = request(1, 5, 0, p8);
  accepted("steps: no busy slot", gen_check_steps(g, 1000));
  g.slots_admitted(&a0, 1);
  CHECK(g.len_hi == 8 && g.slot_len == std::vector<int>({8, 0}) && g.slot_busy == std::vector<char>({1, 0}), "after the first admission: len_hi %d", g.len_hi);
  refused("admit: a busy slot", admit(g, {request(0, 6, 0, p8)}, 6), ZN_ERR_STATE, "zn_gen_admit: slot 0 is busy (zn_gen_retire first)");
  refused("steps: past max_len by one", gen_check_steps(g, 41), ZN_ERR_STATE, "zn_decode_steps: 41 steps would take slot 0 (8 positions) past max_len 48: retire it first");
  accepted("steps: up to max_len", gen_check_steps(g, 40));
  g.slots_advance(16);
  CHECK(g.len_hi == 24 && g.slot_len == std::vector<int>({24, 0}), "after 16 steps: len_hi %d", g.len_hi);
  g.slots_admitted(&a1, 1);
  CHECK(g.len_hi == 24 && g.slot_len == std::vector<int>({24, 5}) && g.slot_busy == std::vector<char>({1, 1}), "after the second admission: len_hi %d", g.len_hi);
  accepted("retire: a busy slot", gen_check_retire(g, 0));
  g.slots_advance(8);
  CHECK(g.len_hi == 32 && g.slot_len == std::vector<int>({32, 13}), "after 8 more steps: len_hi %d", g.len_hi);
  refused("steps: the longer slot decides", gen_check_steps(g, 17), ZN_ERR_STATE, "zn_decode_steps: 17 steps would take slot 0 (32 positions) past max_len 48: retire it first");
  accepted("steps: the longer slot reaches max_len", gen_check_steps(g, 16));
  g.slot_retired(0);
  CHECK(g.len_hi == 13 && g.slot_len == std::vector<int>({0, 13}) && g.slot_busy == std::vector<char>({0, 1}), "after the retire: len_hi %d", g.len_hi);
  refused("retire: retired already", gen_check_retire(g, 0), ZN_ERR_STATE, "zn_gen_retire: slot 0 is idle already");
  accepted("steps: the retired slot no longer counts", gen_check_steps(g, 35));
  refused("steps: the other slot past max_len by one", gen_check_steps(g, 36), ZN_ERR_STATE, "zn_decode_steps: 36 steps would take slot 1 (13 positions) past max_len 48: retire it first");
  accepted("admit: the retired slot again", admit(g, {request(0, 6, 0, p8)}, 6));
  const zn_admit again = request(0, 6, 0, p8);
  g.slots_admitted(&again, 1);
  CHECK(g.len_hi == 13 && g.slot_len == std::vector<int>({6, 13}), "after the re-admission: len_hi %d", g.len_hi);
  g.slot_retired(1);
  CHECK(g.len_hi == 6, "after the second retire: len_hi %d", g.len_hi);
  g.slot_retired(0);
  CHECK(g.len_hi == 0, "every slot idle: len_hi %d", g.len_hi);
  GenHost plain = begun(2, true, 48, 42, 1, 8);
  accepted("steps: not a session", gen_check_steps(plain, 1000));

  // tests/test_gpu_mixed.py: a session of four slots begun without guidance, slack 8
  GenHost m = begun(4, false, 48, 42, 1, 8);
  m.open_slots(8);
  CHECK(m.pairs_set && m.slot_slack == 8, "a session begun without guidance follows the pair words from the start");
  const zn_row_params G = entry(2.f, 6), other = entry(2.f, 6, 2.f), Uq = entry(1.f, 5);
  auto paired = [](zn_row_params r, int o, int f) { r.reserved[0] = o + 1; r.reserved[1] = f + 1; return r; };
  zn_row_params other_pen = paired(other, 2, 0); other_pen.sp.seed = 262;
#define SLOT2(why) "zn_gen_admit: slot 2 " why
  refused("admit: guided, no pair named", admit(m, {request(2, 7, 1, G), request(0, 7, 1, G)}, 7), ZN_ERR_ARG, SLOT2("has a cfg_scale != 1 in a generation begun without guidance and names no row pair"));
  refused("admit: the partner is missing", admit(m, {request(2, 7, 1, paired(G, 2, 0)), request(1, 6, 0, Uq)}, 7), ZN_ERR_ARG, SLOT2("names a row pair whose other row is not part of this call"));
  refused("admit: the partner is another request", admit(m, {request(2, 7, 1, paired(G, 2, 0)), request(0, 7, 1, other_pen)}, 7), ZN_ERR_ARG, SLOT2(DIFFER));
  refused("admit: the partner's row_len differs", admit(m, {request(2, 7, 1, paired(G, 2, 0)), request(0, 6, 1, paired(G, 2, 0))}, 7), ZN_ERR_ARG,
          "zn_gen_admit: slot 2 and its pair's other slot 0 differ in row_len or prefix_len");
  refused("admit: the partner's prefix_len differs", admit(m, {request(2, 7, 1, paired(G, 2, 0)), request(0, 7, 0, paired(G, 2, 0))}, 7), ZN_ERR_ARG,
          "zn_gen_admit: slot 2 and its pair's other slot 0 differ in row_len or prefix_len");
  refused("admit: a pair row out of range", admit(m, {request(2, 7, 1, paired(G, 2, 4)), request(0, 7, 1, paired(G, 2, 4))}, 7), ZN_ERR_ARG, SLOT2("names a row pair out of range"));
  refused("admit: the same row twice", admit(m, {request(2, 7, 1, paired(G, 2, 2)), request(0, 7, 1, paired(G, 2, 2))}, 7), ZN_ERR_ARG, SLOT2("names the same row twice as its pair"));
  refused("admit: a pair of other rows", admit(m, {request(2, 7, 1, paired(G, 1, 0)), request(0, 7, 1, paired(G, 1, 0))}, 7), ZN_ERR_ARG, SLOT2("names a row pair that does not hold its own row"));
  refused("admit: a pair at cfg_scale 1", admit(m, {request(1, 6, 0, paired(Uq, 1, 3)), request(3, 6, 0, paired(Uq, 1, 3))}, 6), ZN_ERR_ARG,
          "zn_gen_admit: slot 1 names a row pair at cfg_scale == 1 (pairs belong to guided entries of a session begun with cfg_scale == 1)");
  accepted("admit: a pair f < o, rows apart, beside an unguided request", admit(m, {request(2, 7, 1, paired(G, 2, 0)), request(0, 7, 1, paired(G, 2, 0)), request(1, 6, 0, Uq)}, 7));
  accepted("admit: a pair o < f", admit(m, {request(1, 7, 1, paired(G, 1, 3)), request(3, 7, 1, paired(G, 1, 3))}, 7));
  accepted("admit: the pair's entries in the other order", admit(m, {request(3, 7, 1, paired(G, 1, 3)), request(1, 7, 1, paired(G, 1, 3))}, 7));
}

// ------------------------------------------------------------------------------------------------ 5. eligibility for the persistent kernels
static void eligibility() {
  int eligible = 0;
  for (int bits = 0; bits < 32; ++bits) {
    GenHost g;
    g.persist_ok = (bits & 1) != 0; g.rows_unequal2 = (bits & 2) != 0; g.prefix_set = (bits & 4) != 0; g.slots_open = (bits & 8) != 0; g.pairs_set = (bits & 16) != 0;
    CHECK(g.persist_eligible() == (bits == 1), "flags %d", bits);
    eligible += g.persist_eligible();
  }
  CHECK(eligible == 1, "%d of 32 combinations are eligible", eligible);
  CHECK(GenHost{}.persist_eligible(), "a fresh record is eligible");
}

// ------------------------------------------------------------------------------------------------ 6. zn_gen_begin starts afresh
// same() and reset() name every field of the record by hand.  A field added to GenHost changes its size: add it to both, then to the size below.
#if defined(__x86_64__) && defined(__GLIBCXX__)
static_assert(sizeof(GenHost) == 216, "GenHost has changed: extend same() and reset() to the new field, then update this size");
#endif
static bool same(const GenHost& a, const GenHost& b) {
  return a.gen_active == b.gen_active && a.gen_ended == b.gen_ended && a.gen_prefilled == b.gen_prefilled && a.rows_set == b.rows_set && a.pairs_set == b.pairs_set &&
         a.prefix_set == b.prefix_set && a.slots_open == b.slots_open && a.rows_unequal2 == b.rows_unequal2 && a.gen_timed_out == b.gen_timed_out && a.stop_pending == b.stop_pending &&
         a.emb_valid == b.emb_valid && a.persist_ok == b.persist_ok && a.batch == b.batch && a.rows == b.rows && a.max_len == b.max_len && a.t_total == b.t_total && a.offset0 == b.offset0 &&
         a.max_new == b.max_new && a.cfg_scale == b.cfg_scale && memcmp(&a.sp, &b.sp, sizeof a.sp) == 0 && a.len_hi == b.len_hi && a.slot_slack == b.slot_slack && a.slot_len == b.slot_len &&
         a.slot_busy == b.slot_busy && a.kv_layers == b.kv_layers && a.kv8_layers == b.kv8_layers && a.lengths == b.lengths && a.codes == b.codes && a.dbg_pause == b.dbg_pause;
}
static void reset() {
  static int some[4];
  GenHost used;
  used.gen_active = used.gen_ended = used.gen_prefilled = used.rows_set = used.pairs_set = used.prefix_set = used.slots_open = used.rows_unequal2 = used.gen_timed_out = used.stop_pending =
      used.emb_valid = true;
  used.persist_ok = false;
  used.batch = 3; used.rows = 6; used.max_len = 77; used.t_total = 55; used.offset0 = 4; used.max_new = 33; used.cfg_scale = 3.5f; used.sp = sampling(1.5f, 7); used.sp.seed = 99;
  used.len_hi = 41; used.slot_slack = 5; used.slot_len = {4, 5, 6}; used.slot_busy = {1, 0, 1}; used.kv_layers = {some, some + 1}; used.kv8_layers = {some + 2};
  used.lengths = some; used.codes = some + 1; used.dbg_pause = 3000000u;
  CHECK(!same(used, GenHost{}), "the used record differs from a fresh one");
  zn_sampling sp = sampling(2.f, 3); sp.temperature = 0.5f; sp.seed = 7;
  used.begin(2, 4, 48, 42, 6, 8, 2.f, sp, some + 2, some + 3);
  GenHost fresh;
  fresh.batch = 2; fresh.rows = 4; fresh.max_len = 48; fresh.t_total = 42; fresh.offset0 = 6; fresh.max_new = 8; fresh.cfg_scale = 2.f; fresh.sp = sp; fresh.lengths = some + 2; fresh.codes = some + 3;
  CHECK(same(used, fresh), "begin() leaves nothing of the last generation");
  CHECK(!used.gen_active && used.persist_ok && used.slot_len.empty() && used.kv8_layers.empty() && used.len_hi == 0 && used.dbg_pause == 0, "the defaults");
  CHECK(used.guided() && !begun(2, false, 8, 8, 1, 1).guided(), "rows = 2 batch with guidance");
}

int main() {
  call_order();
  set_rows_rules();
  prefix_rows_rules();
  prefill_rows_rules();
  session_rules();
  eligibility();
  reset();
  if (g_fail) { printf("FAIL: %d checks\n", g_fail); return 1; }
  printf("OK\n");
  return 0;
}

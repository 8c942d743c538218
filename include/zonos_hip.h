/* zonos_hip.h — C ABI of libzonos_hip.so: the MI355X (gfx950) implementation of the Zonos TTS hot path.
 *
 * The reference (langfod/Zonos) is 100 % Python and has no FFI; its seam for this path is the Python surface
 * zonos/model.py (Zonos.generate :354-548, _compute_logits :225-234, setup_cache :305-338), the backbone plugin
 * contract zonos/backbone/__init__.py:24-36 + _torch.py:157,213, zonos/sampling.py:166-231 and
 * zonos/autoencoder.py:119-170 (DACAutoencoder.decode / decode_to_int16).  Each entry point below names the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of the reference adds.
 *
 * Conventions: extern "C", plain pointers and sizes, no torch types.  Every call returns an int status
 * (ZN_OK = 0, < 0 = error) and never throws or aborts; zn_last_error(h) gives the message.  All `*_dev`
 * pointers are device (HBM) pointers owned by the caller (torch tensors' data_ptr()); the library owns only the
 * handle-scoped workspace.  `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream), 0 = default.
 * One handle = one device; calls on one handle must not overlap in time; distinct handles are independent.
 * bf16 = raw uint16 bit pattern, row-major tensors, nn.Linear weights are [out_features][in_features].
 */
#ifndef ZONOS_HIP_H
#define ZONOS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZN_ABI_VERSION 9

enum zn_status {
  ZN_OK = 0,
  ZN_ERR_ARG = -1,          /* bad argument / shape the kernels do not support */
  ZN_ERR_HIP = -2,          /* a HIP runtime call failed */
  ZN_ERR_STATE = -3,        /* call order violated (e.g. decode before zn_gen_begin) */
  ZN_ERR_UNSUPPORTED = -4,  /* valid in the reference, not built yet */
  ZN_ERR_NOMEM = -5
};

typedef struct zn_handle_s* zn_handle;
typedef struct zn_dac_s* zn_dac;
typedef struct zn_spk_s* zn_spk;
typedef void* zn_stream;

/* Model hyper-parameters: zonos/config.py:55-84 BackboneConfig + :105-126 ZonosConfig (read from config.json
 * by the host; never hard-coded). */
typedef struct zn_config {
  int32_t d_model, n_layer, n_heads, n_heads_kv, d_ff; /* attn_mlp_d_intermediate */
  int32_t n_codebooks;     /* 9 */
  int32_t vocab_head;      /* 1025 logits per codebook (zonos/model.py:82) */
  int32_t vocab_embed;     /* 1032 embedding rows (zonos/model.py:80) */
  int32_t eos_id, mask_id; /* 1024, 1025 */
  int32_t rope_positions;  /* rows of the RoPE table, 16384 (_torch.py:206) */
  int32_t double_out_proj; /* 1 = reproduce _torch.py:419-420 (out_proj applied twice), 0 = upstream behaviour */
  float norm_eps;          /* 1e-5 */
  /* ABI 2 — hybrid backbone (zonos/backbone/_mamba_ssm.py:8-119; BackboneConfig.ssm_cfg, zonos/config.py:79).
   * arch 0: every layer is a _torch.py TransformerBlock (fields below ignored).  arch 1: mamba_ssm Block semantics
   * (fused residual-add + LayerNorm with the sum kept in fp32 for the norm, single out_proj, deferred residual),
   * layer i is a Mamba2 mixer unless zn_layer_weights.kind says attention. */
  int32_t arch;
  int32_t m_d_inner;       /* expand * d_model */
  int32_t m_headdim;       /* 64 */
  int32_t m_d_state;       /* 64 or 128 */
  int32_t m_ngroups;       /* 1 */
  int32_t m_d_conv;        /* 4 */
  /* ABI 3 - remaining BackboneConfig switches of the hybrid stack (zonos/config.py:80-84, create_block arguments at
   * _mamba_ssm.py:45-58); arch 0 ignores them (the torch backbone reads none of them). */
  int32_t rms_norm;         /* 1: every block norm and the final norm are RMSNorm (no mean; the final norm keeps its bias) */
  int32_t residual_in_fp32; /* 1: the residual stream between blocks is fp32 */
  int32_t rope_mode;        /* attention layers (mamba_ssm MHA, attn_cfg): 0 = interleaved pairs over the whole head,
                               1 = half-split (rotary_emb_interleaved = False, the library default and the Zonos-v0.1-hybrid
                               checkpoint's), 2 = no rotary (rotary_emb_dim = 0) */
} zn_config;

typedef struct zn_layer_weights { /* bf16; names = _torch.py:278-281,373-374,453-454 */
  const void *norm_w, *norm_b;     /* [d] */
  const void *in_proj;             /* [(H+2Hkv)*hd, d] */
  const void *out_proj;            /* [d, H*hd] */
  const void *norm2_w, *norm2_b;   /* [d] */
  const void *fc1;                 /* [2*d_ff, d]  rows [0,d_ff) = value, [d_ff,2d_ff) = gate */
  const void *fc2;                 /* [d, d_ff] */
  /* ABI 2: kind 0 = attention + gated MLP (fields above), 1 = Mamba2 mixer (fields below + norm_w/norm_b);
   * names = mamba_ssm Mamba2 parameters under layers.{i}.mixer. */
  int32_t kind;
  const void *m_in_proj;           /* [2*d_inner + 2*ngroups*d_state + nheads, d] */
  const void *m_conv_w, *m_conv_b; /* conv1d.weight [conv_dim, 1, d_conv], conv1d.bias [conv_dim]; conv_dim = d_inner + 2*ngroups*d_state */
  const void *m_dt_bias, *m_A_log, *m_D;   /* [nheads], nheads = d_inner / headdim */
  const void *m_norm_w;            /* mixer.norm.weight [d_inner] (RMSNormGated) */
  const void *m_out_proj;          /* [d, d_inner] */
  /* ABI 3: optional nn.Linear biases of a mamba_ssm MHA layer (attn_cfg qkv_proj_bias / out_proj_bias; NULL = none) */
  const void *in_proj_bias;        /* [(H+2Hkv)*hd] */
  const void *out_proj_bias;       /* [d] */
} zn_layer_weights;

typedef struct zn_weights {
  const void* const* embeddings;   /* host array of n_codebooks device pointers, each bf16 [vocab_embed, d] */
  const void* heads;               /* bf16 [n_codebooks*vocab_head, d]  (fused_heads, zonos/model.py:82,208-223) */
  const void *norm_f_w, *norm_f_b; /* bf16 [d] */
  const zn_layer_weights* layers;  /* host array [n_layer] */
  const float* rope_table;         /* fp32 [rope_positions, hd/2, 2] (cos,sin), built by the host exactly as
                                      _torch.py:29-34 does (torch.polar on CPU) */
} zn_weights;

/* sampling_params of Zonos.generate (zonos/sampling.py:166-178 defaults). */
typedef struct zn_sampling {
  float temperature;   /* <= 0: greedy argmax */
  float top_p; int32_t top_k; float min_p;
  float linear, conf, quad;
  float repetition_penalty; int32_t repetition_penalty_window;
  uint64_t seed;       /* device RNG stream for the Gumbel-max draw */
} zn_sampling;

/* ABI 9 - one utterance's settings in a batched generation (zn_gen_set_rows, zn_op_sample_rows): what zn_gen_begin takes once for the
 * whole batch, per row.  ZN_ROW_PARAMS_BYTES = 64 bytes exactly, so that a sampler workgroup fetches its row with one aligned load. */
#define ZN_ROW_PARAMS_BYTES 64
typedef struct zn_row_params {
  zn_sampling sp;           /* this utterance's sampling parameters; sp.seed seeds its own Gumbel stream */
  float cfg_scale;          /* guidance strength of this utterance's [cond, uncond] pair; == 1 for every row or for none (the row layout
                               is fixed by zn_gen_begin's cfg_scale) - or, in a generation begun with cfg_scale == 1, != 1 in the two
                               entries of a row pair (below) */
  int32_t max_new_tokens;   /* this utterance's budget of frames, 1 .. zn_gen_begin's max_new_tokens */
  int32_t reserved[2];      /* the row pair of a guided request in a MIXED generation: reserved[0] = cond_row + 1, reserved[1] = uncond_row + 1;
                               both 0 (what every caller wrote before pairs existed): no pair, exactly the behaviour of the layout
                               zn_gen_begin fixed */
} zn_row_params;
/* Mixed generations: guided and unguided requests in one generation or session (additive to ABI 9: the two reserved words get a meaning, all-zero
 * keeps every bit).  The generation is begun in the UNGUIDED layout - zn_gen_begin(batch = R, cfg_scale = 1): R rows, R utterance slots, row u is
 * utterance u.  An unguided request takes one slot and leaves both words 0.  A guided request takes any two slots o and f: the caller prefills
 * row o with its conditional and row f with its unconditional positions, gives both slots identical code-buffer rows, prefix length and row_len,
 * and gives both slots the SAME entry: the request's sampling parameters, seed, cfg_scale != 1, max_new_tokens and the pair (o + 1, f + 1).
 * The sampler workgroup (codebook, u) of a paired utterance reads its conditional logits from raw row reserved[0] - 1 and its unconditional ones
 * from raw row reserved[1] - 1 and mixes them as a generation begun with guidance does (uncond + (cond - uncond) * cfg_scale, the same fp32
 * operations in the same order).  Slots o and f have the same inputs, the same Gumbel key and the same history, so both sample the same token
 * into their own buffer rows; bookkeeping, lengths, remaining_steps and the stop state stay per slot, as in any unguided generation.  The
 * request's codes are row o's (row f holds the same cells).  f < o is legal; the two rows need not be adjacent.  A generation whose table names
 * a pair, and every session begun without guidance, stays off the persistent kernels (zn_decode_path_detail reports 0). */

/* Slotted sessions (additive to ABI 9: new entry points only, no existing layout or call changes) - one request admitted into a slot of a slotted session (zn_gen_admit). */
typedef struct zn_admit {
  int32_t slot;             /* 0 .. batch - 1, idle */
  int32_t row_len;          /* valid positions of the request's prefill rows: L_b + P_b + 1 (conditioning, audio prefix, the column that starts the loop) */
  int32_t prefix_len;       /* P_b audio prefix frames at the left of the slot's row of the code buffer */
  int32_t reserved;         /* set to 0 */
  zn_row_params params;     /* as for zn_gen_set_rows */
} zn_admit;

/* ---------------------------------------------------------------- lifecycle */
int zn_abi_version(void);
/* Replaces Zonos.__init__/from_local weight binding (zonos/model.py:68-86,128-176).  Weights stay owned by the
 * caller and must outlive the handle.  max_rows = rows of the largest generation, even: R = 2 B with guidance (CFG doubles rows,
 * generation_utils.py:192), R = B when cfg_scale == 1. */
int zn_create(const zn_config* cfg, const zn_weights* w, int32_t max_rows, zn_handle* out);
int zn_destroy(zn_handle h);
const char* zn_last_error(zn_handle h); /* h may be NULL: last creation error */
/* Bytes of one layer's KV cache [rows, max_len, 2, Hkv, hd] bf16 (_torch.py:305). */
size_t zn_kv_bytes_per_layer(const zn_config* cfg, int32_t rows, int32_t max_len);
/* Bytes of one Mamba2 layer's decode state (_mamba_ssm.py:65-86 -> Mamba2.allocate_inference_cache): conv_state
 * bf16 [rows, conv_dim, d_conv] followed by ssm_state bf16 [rows, nheads, headdim, d_state], one contiguous buffer
 * whose device pointer takes the layer's slot in zn_gen_begin's kv_layers_dev.  *conv_bytes (optional) receives the
 * offset of ssm_state. */
size_t zn_mamba_state_bytes_per_layer(const zn_config* cfg, int32_t rows, size_t* conv_bytes);

/* ---------------------------------------------------------------- generation (Zonos.generate, model.py:354-548) */
/* Binds the per-call state that zonos/model.py:410-463 builds: KV caches (one device pointer per layer, layout
 * [R, max_len, 2, Hkv, hd] bf16 = TorchZonosBackbone.allocate_inference_cache), lengths_per_sample int32[R]
 * (device, zeroed by the caller), the delay-patterned code buffer int32 [B, n_codebooks, t_total] with -1 for
 * unknown (model.py:414-420), the first column to write `offset0` = prefix_len + 1, cfg_scale and sampling.
 * R = 2B rows [cond ‖ uncond] with guidance; cfg_scale == 1: R = B conditional rows and no CFG mix (model.py:230).
 * R <= max_rows.  kv_layers_dev may be NULL, or hold NULL entries, exactly in a codes-only generation (zn_set_kv_fp8_only in effect for R rows): it has no bf16
 * caches, and pointers passed anyway are never read or written. */
/* (zn_gen_begin discards the hipGraphs captured for the previous generation: call it only when that generation's steps have drained from
 * their stream - `Zonos.generate` synchronises before it returns.) */
int zn_gen_begin(zn_handle h, int32_t batch, const void* const* kv_layers_dev, int32_t max_len,
                 int32_t* lengths_dev, int32_t* delayed_codes_dev, int32_t t_total, int32_t offset0,
                 int32_t max_new_tokens, float cfg_scale, const zn_sampling* sp, zn_stream stream);
/* prefill_static (generation_utils.py:206-244) + _compute_logits: hidden bf16 [R, S, d] = [cond ‖ uncond] (R = 2B), or the
 * B conditional rows when cfg_scale == 1, conditioning concatenated with embed(delayed[..., :prefix+1]); fills KV positions
 * [0,S), lengths += S and leaves the fp32 logits [B, n_codebooks, vocab_head] (CFG-mixed with guidance) in the handle. */
int zn_prefill(zn_handle h, const void* hidden_dev, int32_t S, zn_stream stream);
/* ABI 9 - per-utterance sampling parameters, seed, cfg_scale and length for the generation begun by zn_gen_begin.  rows_host: HOST array of
 * n == batch entries, copied to a device table the handle owns; every sampler workgroup (cb, b) of this generation - zn_sample_first, the
 * decode steps on every path, captured graphs included - then takes its parameters from entry b instead of zn_gen_begin's `sp` and
 * `cfg_scale`: temperature, top_p, top_k, min_p, linear, conf, quad, repetition penalty and window, cfg_scale, and the penalty context
 * min(max_new_tokens_b, 100).  Utterance b's Gumbel draw for (step, codebook cb, token t) is keyed by (sp.seed_b, draw + step, cb * V + t + 1)
 * - the key of utterance 0 of a call seeded sp.seed_b: a request's random stream does not depend on the slot it occupies and equals the
 * stream of a one-utterance generation with that seed.  remaining_steps of utterance b becomes max_new_tokens_b + n_codebooks - 1 (what a
 * generation of that length starts with); an utterance whose budget is spent counts as stopped for zn_all_stopped*, and the columns it
 * still receives beyond its own length are the caller's to cut.
 * Legal only between zn_gen_begin and the generation's first zn_prefill / zn_prefill_rows (ZN_ERR_STATE otherwise; no graph has been
 * captured yet).  ZN_ERR_ARG: n != batch, a repetition_penalty_window outside 0..64, max_new_tokens_b outside 1 .. zn_gen_begin's
 * max_new_tokens, or cfg_scale_b == 1 on a generation begun with guidance.  In a generation begun with cfg_scale == 1 an entry with
 * cfg_scale_b != 1 is legal exactly when it names a row pair (zn_row_params, "Mixed generations") and: both rows lie in 0 .. batch - 1, they are
 * distinct, one of them is b itself, and the other row's entry names the same pair with byte-equal parameters (the two entries are equal as 64
 * bytes); anything else is ZN_ERR_ARG with a message naming the utterance.  ZN_ERR_ARG as well: a pair named in a generation begun with guidance,
 * or by an entry with cfg_scale_b == 1.  An error leaves the generation as it was.  Without this call every row uses zn_gen_begin's values (the same bits as ABI 8).
 * Synchronises the generation's stream. */
int zn_gen_set_rows(zn_handle h, const zn_row_params* rows_host, int32_t n);
/* An audio prefix of its own length per utterance of the generation begun by zn_gen_begin (a column shift per row of the code buffer).  The
 * caller begins the generation for the LONGEST prefix: offset0 = P_call + 1 and t_total = P_call + max_b max_new_tokens_b + n_codebooks with
 * P_call = max_b P_b, and lays utterance b out left-aligned in its own buffer row: P_b prefix frames, its unknown cells, then the mask
 * token, under the delay pattern.  prefix_len_host: HOST array of n == batch lengths P_b; the library stores shift[b] = P_b - P_call (<= 0) in
 * a device array of its own, and at loop state `offset` utterance b's column is offset + shift[b]: zn_sample_first writes it there, every
 * decode step embeds that column, writes the next one and takes its repetition-penalty history from the columns ending there (clamped at the
 * row's own column 0, never reaching another row) - what a generation with a shared prefix of P_b frames does for that utterance.  The
 * prefill rows are the caller's (zn_prefill_rows with row_len[r] = L_b + P_b + 1; zn_op_assemble_prefill builds them).
 * Legal exactly where zn_gen_set_rows is: after zn_gen_begin, before the generation's prefill, before any graph is captured (ZN_ERR_STATE
 * otherwise).  ZN_ERR_ARG: n != batch, a length outside 0 .. P_call, or no length equal to P_call.  An error leaves the generation as it
 * was.  Without this call, or with every length equal, every shift is 0, the kernels receive a NULL array and compute what they computed
 * before.  A generation with a shift never runs the persistent kernels (zn_decode_path_detail reports 0), whose samplers do not read it -
 * two unguided utterances whose lengths advance in lockstep included.  Synchronises the generation's stream. */
int zn_gen_set_prefix_rows(zn_handle h, const int32_t* prefix_len_host, int32_t n);
/* A slotted session: requests join the running generation as slots free up.  zn_gen_open_slots turns the generation begun by
 * zn_gen_begin into a session of `batch` slots, all idle; zn_gen_begin's max_len, t_total (the width W of a row of the code buffer),
 * cfg_scale (guided or not) and batch fix the KV capacity per row, the code-buffer width, the row layout and the slot count, and its
 * lengths array must be zero.  `slack` >= 0 is the number of decode steps a request may run beyond its own end (max_new_tokens + n_codebooks
 * - 1 steps) before the caller retires it; the caller's scheduling cadence decides it (zonos_amd/serving.py: 16 + sched_every).  Legal where
 * zn_gen_set_rows is (ZN_ERR_STATE otherwise), instead of zn_gen_set_rows / zn_gen_set_prefix_rows / zn_prefill*.  The session's loop is
 *   zn_gen_admit ... | zn_decode_steps(k) | zn_gen_row_state | zn_gen_retire ... | zn_gen_admit ... | zn_decode_steps(k) | ...
 * Every slot has its own length (lengths[r]), stop state, parameter entry, column shift and step origin on the device; the rows of an idle slot
 * keep running through the steps' kernels at length 0 (each step rewrites position 0 of their own cache rows, their lengths do not advance,
 * their code cells - the caller fills an idle slot's row with anything but -1 - are not written) and nothing they compute reaches another row.
 * A session never runs the persistent kernels (zn_decode_path_detail reports 0, one and two rows included).  zn_debug_force_eos,
 * zn_debug_eos_bias and zn_debug_token_override stay call-wide, indexed by the SESSION's step (the decode steps enqueued since zn_gen_begin),
 * not by a request's own.  zn_decode_steps returns ZN_ERR_STATE when a step would take a busy slot's rows past max_len. */
int zn_gen_open_slots(zn_handle h, int32_t slack);
/* Admits n >= 1 requests into idle slots between two zn_decode_steps calls.  hidden bf16 [n * halves, S, d] (halves = 2 in a guided session:
 * [cond_0..cond_{n-1} ‖ uncond_0..uncond_{n-1}]) is right-padded as for zn_prefill_rows, request j holding a[j].row_len valid positions in
 * each of its rows.  Before the call the caller has written slot b's row of the code buffer (stream-ordered): P_b prefix frames,
 * max_new_tokens_b unknown cells (-1), the mask token up to W, under the delay pattern.  The rows are prefilled as ONE batch of n * halves
 * rows - the launches zn_prefill_rows makes for such a batch - into a scratch cache the handle owns, and one kernel moves them into the
 * slots' rows.  For every admitted slot b: KV positions [0, row_len) of cache rows b and batch + b (Mamba2: the conv and SSM states of those
 * rows), lengths = row_len, remaining_steps = max_new_tokens_b + n_codebooks - 1, stopping = 0, the parameter entry, the column shift
 * (P_b + 1 - the loop's current column: either sign) and the slot's step origin = the session's step.  The slot's first frame is then sampled
 * as zn_sample_first samples it (draw index 0 of the slot's own seed, no penalty, no logit bias) into column P_b + 1 of its row, and its
 * logits go to row b of zn_get_step_outputs.  From then on the slot's Gumbel draw at session step t is keyed by (seed_b, 1 + t - origin_b, ...):
 * the stream of a generation of that request alone.  Nothing of another slot is written: no KV position, length, logit, counter, token or
 * code cell.
 * ZN_ERR_ARG: a slot out of range or named twice, a row_len outside 1..S or none equal to S, a prefix_len outside 0 .. row_len - 2, a request
 * that does not fit (row_len - 1 + max_new_tokens + n_codebooks + slack > max_len, or prefix_len + max_new_tokens + n_codebooks + slack > W),
 * cfg_scale == 1 in a guided session, a repetition_penalty_window outside 0..64.  In a session begun with cfg_scale == 1 (hidden [n, S, d], one
 * entry per row) a request with cfg_scale != 1 is admitted as a row pair: two entries of this call, for slots o and f, with equal params that
 * name the pair (o + 1, f + 1), equal row_len and equal prefix_len, hidden row of entry o holding the conditional positions and that of entry f
 * the unconditional ones (zn_row_params, "Mixed generations").  ZN_ERR_ARG, naming the slot: no pair named, a row out of range, the same row
 * twice, a pair that does not hold the entry's own slot, the other slot missing from this call, its params not byte-equal, its row_len or
 * prefix_len different; a pair named in a guided session or at cfg_scale == 1.  The first frame is sampled per admitted slot, as for any other
 * slot: each slot of a pair mixes the two rows' logits for itself.  ZN_ERR_STATE: no session, a busy slot, steps
 * still owed to zn_all_stopped_end.  ZN_ERR_UNSUPPORTED: the position-by-position prefill (zn_debug_prefill_mode 0).  An error leaves the
 * session as it was.  The call does not synchronise (it waits for the previous admission's staged arguments to have been consumed). */
int zn_gen_admit(zn_handle h, const zn_admit* a, int32_t n, const void* hidden_dev, int32_t S, zn_stream stream);
/* Marks a busy slot idle: its rows' lengths and its remaining_steps become 0 (an idle slot counts as stopped for zn_all_stopped*) on the
 * session's stream.  ZN_ERR_STATE: no session, or the slot is idle already. */
int zn_gen_retire(zn_handle h, int32_t slot);
/* remaining_steps[0 .. batch) and every slot's own step count (session step - step origin; -1 for an idle slot) to HOST arrays (either may be
 * NULL), as of the steps enqueued so far.  Synchronises the stream; surfaces a hand-off timeout word as zn_all_stopped does. */
int zn_gen_row_state(zn_handle h, int32_t* remaining_host, int32_t* steps_host, zn_stream stream);
/* ABI 8 - zn_prefill for utterances of different prompt lengths.  hidden bf16 [R, S, d] is RIGHT-padded: row r holds row_len[r] valid
 * positions (its conditioning followed by the embedded audio prefix), then S - row_len[r] positions of padding whose contents are never
 * visible to a result: no valid query attends a pad key, no pad position reaches a logit, a Mamba2 state or a KV entry that is read
 * later (pad positions do write the cache slots [row_len[r], S) of their row; the row's own decode steps overwrite each of them before
 * the attention extent reaches it).  row_len is a HOST array of R lengths in 1..S, at least one equal to S; the library copies it to a
 * device array of its own.  Afterwards lengths[r] = row_len[r]; row r's first-frame logits come from position row_len[r] - 1, and its
 * prefill attention uses the query split and key extents of a sequence of row_len[r] positions - the result a batch of utterances of that
 * length gets.  zn_prefill(h, hidden, S, st) is this call with every length S (the same launches, the same bits).
 * ZN_ERR_ARG: a length out of range, no length equal to S, or a guided pair with row_len[b] != row_len[B + b].  ZN_ERR_UNSUPPORTED: unequal
 * lengths on the position-by-position prefill (zn_debug_prefill_mode(h, 0), and models whose dimensions fall back to it). */
int zn_prefill_rows(zn_handle h, const void* hidden_dev, int32_t S, const int32_t* row_len, zn_stream stream);
/* model.py:423-431: sample the first frame from the prefill logits (no repetition penalty, no logit bias) and
 * write it into column offset0 where that column is -1. */
int zn_sample_first(zn_handle h, zn_stream stream);
/* n iterations of the hot loop (model.py:467-502): embed column offset-1, 26 blocks, heads, CFG, logit bias,
 * repetition penalty, sample, EOS bookkeeping (tensor_ops.py:155-211), frame write (tensor_ops.py:12-53),
 * offsets += 1.  Asynchronous; replays one hipGraph per step. */
int zn_decode_steps(zn_handle h, int32_t n, zn_stream stream);
/* 1 if the decode step is currently replayed as an instantiated hipGraph, 0 if launched kernel by kernel. */
int zn_graph_active(zn_handle h);
/* 1 if the decode steps of the generation begun by zn_gen_begin run the persistent kernels (one or two rows - batch 1 with guidance,
 * batch 1 or 2 without - on a model whose shapes they serve), 0 if every op is a launch of its own.  Both paths give bit-identical results at the Zonos-v0.1 shapes (same tiles, same
 * summation order in every GEMV; ONE arithmetic for the decode attention on every path: scores on the matrix cores, contexts of one
 * 512-key block accumulated in place, longer ones block by block with the partials combined in block order). */
int zn_decode_path(zn_handle h);
/* Which kernels served the decode step enqueued last: 0 = one launch per op, 1 = one attention launch (two beyond 512 keys) + one
 * persistent chain launch per block (two rows only), 2 = the whole-step persistent kernel (every block of the step in one launch;
 * contexts up to 6144 keys: one attention workgroup per (row, kv head, 512-key block); two rows or, without guidance, one row - a
 * one-row step beyond 6144 keys runs the launches path).  All give bit-identical results.  Two unguided utterances whose rows have
 * different lengths (zn_prefill_rows) always report 0: the two-row persistent kernels are kept for rows that advance in lockstep. */
int zn_decode_path_detail(zn_handle h);
/* Hand-off timeouts are never silent: out[0] = bounded in-kernel hand-off waits that gave up and were reported on this handle (each voids
 * its generation; zn_all_stopped* returns the error), [1] generations begun, [2] batch-1 generations that ran the launches path because
 * an earlier timeout had demoted the handle, [3] 1 while the handle is demoted, [4] times it was re-armed (automatically after 4 clean
 * generations on the launches path, or by zn_debug_tune(ZN_TUNE_PERSISTENT, 1)), [5] clean generations since the demotion, [6] the longest in-kernel hand-off
 * wait any whole-step launch of this handle measured, in microseconds (0: none beyond 0.1 ms; a pause of the device shows up here with its
 * length), [7] waits beyond 0.2 ms.  n <= 8 values are written; asking for [6], [7] synchronises with the device. */
int zn_get_counters(zn_handle h, int64_t* out, int32_t n);
/* Ends the generation begun by zn_gen_begin: releases the device's persistent-kernel tenancy (below) so that another handle's next
 * generation may take it.  The handle's state stays readable (zn_decode_path, zn_get_step_outputs); further steps need a new
 * zn_gen_begin.  Optional: zn_gen_begin of the same handle and zn_destroy release too. */
int zn_gen_end(zn_handle h);
/* One generation per device and process owns the persistent decode kernels (their in-launch hand-offs need every workgroup of the
 * grid resident: two such grids on one device could starve each other).  zn_gen_begin claims the device for `h`; a generation that
 * begins while another handle holds it runs the launches path (bit-identical results).  The two primitives are exported for the
 * host-side tests: try_claim returns 1 when `owner` holds the device afterwards, release 1 when `owner` held it. */
int zn_tenant_try_claim(int32_t device, const void* owner);
int zn_tenant_release(int32_t device, const void* owner);
/* (remaining_steps <= 0).all() of tensor_ops.py:95,102 — synchronises the stream. */
int zn_all_stopped(zn_handle h, int32_t* out, zn_stream stream);
/* The same check off the critical path: zn_all_stopped_begin queues the read-back of the loop state behind the steps enqueued
 * so far and returns; zn_all_stopped_end (called after the NEXT steps have been enqueued) waits for it and reports the
 * state as of _begin.  Steps that over-run a stop write only columns the caller's cut drops (model.py:511-528). */
int zn_all_stopped_begin(zn_handle h, zn_stream stream);
int zn_all_stopped_end(zn_handle h, int32_t* all_stopped_out);
/* Copies the fp32 logits the sampler last consumed ([B, n_codebooks, vocab_head], after CFG and logit bias) and
 * the raw sampled tokens int32 [B, n_codebooks] to device buffers (either may be NULL).  For parity tests. */
int zn_get_step_outputs(zn_handle h, float* logits_dev, int32_t* tokens_dev, zn_stream stream);
/* The caller rewrote cells of delayed_codes between two zn_decode_steps calls (teacher forcing): every step's sampler launch
 * also leaves the embedding of the column it wrote for the next step, and that embedding is stale now.  The next
 * zn_decode_steps call embeds the current column again. */
int zn_codes_changed(zn_handle h);
/* Test hook: at loop step `step` (0-based) force codebook-0 EOS by setting its logit to 1e4 (-1 = off). */
int zn_debug_force_eos(zn_handle h, int32_t step);
/* Test hook: replace the sampled raw tokens of call k (0 = first frame, k = loop step k-1) by
 * tokens_dev[k] (int32 [calls, B, n_codebooks], device) so that the EOS bookkeeping, frame writes and stop
 * cadence can be checked bit-exactly against the reference's recorded token stream.  NULL = off. */
int zn_debug_token_override(zn_handle h, const int32_t* tokens_dev, int32_t calls);
/* Test hook: 1 = batched prefill (default: MFMA GEMMs + tiled causal attention over all positions), 0 = position by
 * position through the decode kernels (both reproduce the reference's rounding points). */
int zn_debug_prefill_mode(zn_handle h, int32_t mode);
/* Keys of zn_debug_tune.  Every setting gives bit-identical results unless its comment says otherwise; 1 restores a switch's default. */
enum zn_tune_key {
  ZN_TUNE_WG_IN_PROJ = 0,           /* target workgroups of the in_proj GEMV (up to 4 rows); default 256 */
  ZN_TUNE_WG_OUT_PROJ = 1,          /* ... of out_proj; default 512 */
  ZN_TUNE_WG_FC1 = 2,               /* ... of fc1; default 512 */
  ZN_TUNE_WG_FC2 = 3,               /* ... of fc2 (and the Mamba2 out_proj); default 1024 */
  ZN_TUNE_WG_HEADS = 4,             /* ... of the heads; default 512 */
  ZN_TUNE_ATTN_FUSED_MAX_KEYS = 5,  /* longest context of the one-launch decode attention; values above 512 (one block) act as 512; default 512 */
  ZN_TUNE_GRAPH_RUNS = 6,           /* 1 = single-step graphs only; default 2: graphs of 8 consecutive steps */
  ZN_TUNE_SMALL_M_LDS = 7,          /* 1 = none of the small-M projection kernels of 5..64 rows (gemm16s, gemm16k, gemm64s); default 2 */
  ZN_TUNE_PERSISTENT = 8,           /* 2 = per-op launches instead of the persistent kernels (also ZN_CHAIN=0 at zn_create); 1 = the default,
                                       and re-arms a handle demoted by a hand-off timeout */
  ZN_TUNE_FC1_LN_LAUNCH = 9,        /* 5..16 rows: 2 = fc1's LayerNorm as a launch of its own; default: fc1 normalises from statistics the preceding
                                       out_proj's epilogue left per 16-column tile (sums taken tile-wise: a bf16 ulp apart in about one value of a hundred) */
  ZN_TUNE_PREFILL_ATTN_VALU = 10,   /* 2 = the VALU prefill attention at every head size; default: matrix cores at head size 128 */
  ZN_TUNE_NO_SPLIT_SMALL_M = 11,    /* 2 = no in-workgroup-split small-M kernel (gemm16k_kernel) anywhere */
  ZN_TUNE_NO_PREFILL_GEMM16K = 12,  /* 2 = short-prompt prefill projections never take gemm16k_kernel */
  ZN_TUNE_GEMM16K_MAX_TILES = 13,   /* 16-row weight tiles from which the 64-row workgroups take over from gemm16k_kernel; default (unset) 1024 */
  ZN_TUNE_HOOK = 14,                /* not a setting: value = a one-shot test hook (enum zn_tune_hook) */
  ZN_TUNE_WHOLE_STEP = 15,          /* 2 = one chain launch per block instead of the whole-step kernel (also ZN_STACK=0 at zn_create) */
  ZN_TUNE_SAMPLER = 16,             /* batch 1: 2 = always the ticketed sampler launch, 3 = the one-workgroup step tail also with a temperature;
                                       default: the one-workgroup tail for greedy decoding */
  ZN_TUNE_RESERVED_17 = 17,         /* reserved, unused */
  ZN_TUNE_STACK_PRE = 18,           /* 2 = block 0's in_proj as a launch before the whole-step kernel; default: inside it */
  ZN_TUNE_ATTN_SPLIT_COLS = 19,     /* value-column parts of the decode attention: 1 = never split, 2 = always; default: from 5 rows on */
  ZN_TUNE_MLP_FP8 = 20,             /* 2 = ignore the FP8 streams attached by zn_set_mlp_fp8: every launch reads the bf16 fc1 / fc2 */
  ZN_TUNE_WIDE_ROWS = 21,           /* decode steps of 17..64 rows: 1 = every projection in groups of 16 rows (each weight streamed once per group);
                                       2 = up to 64 rows per weight pass also in zn_op_linear_fused / zn_op_linear_fp8; default: generation steps and
                                       zn_bench_kernel take up to 64 rows per weight pass, the per-op entry points groups of 16.  Same bits either way */
  ZN_TUNE_WIDE_HYBRID = 22,         /* the Mamba2 in_proj of a hybrid decode step of 17..64 rows (under the wide plan; ZN_TUNE_WIDE_ROWS = 1 still groups everything by 16):
                                       1 = groups of 16 rows, 2 = row groups on the grid of gemm16k_kernel (the weight tile re-read through L2 per 16 rows), 3 = the
                                       row-tile loop (gemm16k_rows_kernel: the weight tile requested once per up to 64 rows); default: the form the plan picks for the
                                       row count (wide_hybrid_form, zn_linear_plan.h).  Same bits in every form */
  ZN_TUNE_MAMBA_FP8 = 23,           /* 2 = ignore the FP8 streams attached by zn_set_mamba_fp8: every launch reads the bf16 in_proj / out_proj of the Mamba2 layers */
  ZN_TUNE_FP8_SMALL_ROWS = 24,      /* decode launches of 1..4 rows (the GEMV) of a projection with an FP8 stream attached (zn_set_mlp_fp8: fc1 / fc2; zn_set_mamba_fp8:
                                       in_proj / out_proj): 2 = they read the stream (gemv8_kernel, the next unit requested ahead), 3 = the same with a ring of two units
                                       requested ahead (measurement only: never faster, profiles/smallrowsbench.txt); unset or 1 = they read the bf16 copy.  ZN_TUNE_MLP_FP8 / ZN_TUNE_MAMBA_FP8 = 2 switch the stream off
                                       here too.  Same bits either way; the persistent kernels always read the bf16 copy, and the key never changes the path a
                                       generation takes */
  ZN_TUNE_KV_FP8 = 25,              /* 2 = the decode attention ignores the code cache of zn_set_kv_fp8 and reads the bf16 cache; the appends still round and still write both
                                       caches, so the result is the same bits.  The key never changes the path a generation takes.  Ignored for a codes-only generation
                                       (zn_set_kv_fp8_only): it has no bf16 cache to read, and its plans report the codes */
  ZN_TUNE_NKEYS = 26
};
/* Values of ZN_TUNE_HOOK.  The first three arm the next zn_gen_begin, which consumes them. */
enum zn_tune_hook {
  ZN_HOOK_TAG_WRAP = 7,             /* the generation behaves as if the hand-off tags were about to wrap */
  ZN_HOOK_TIMEOUT_WORD = 9,         /* the generation's hand-off waits find the timeout word set */
  ZN_HOOK_PAUSE = 11,               /* every whole-step launch of the generation stops all its waves for 30 ms in block 2, as a paused device would */
  ZN_HOOK_RESET_WAIT_STATS = 13     /* at once: forget the wait statistics of zn_get_counters [6], [7] */
};
/* Tuning and test hook: key in 0 .. ZN_TUNE_NKEYS - 1, value >= 1.  Drops the captured graphs. */
int zn_debug_tune(zn_handle h, int32_t key, int32_t value);
/* Diagnostic: workgroup 0 of every persistent chain launch records s_memrealtime (100 MHz) stamps of its phases into
 * stamps_dev [2 * n_layer][32] (NULL = off); rows n_layer.. hold the fused attention launch's (start, length known, scores
 * issued, scores done, P.V done, reduced, stored).  Stamp order per launch: input ready; then per op: results ready, arrived,
 * all arrived, next input ready; last: end. */
int zn_debug_chain_stamps(zn_handle h, uint64_t* stamps_dev);
/* Diagnostic: every decode step copies, per block, the residual stream after the block, the block's attention output, its
 * rotated queries, the gated MLP values m [rows][d_ff <= 4 d_model] (slots 3..6) and the residual stream after the attention
 * half (slot 7) into trace_dev [n_layer][8][rows][d_model] bf16 (NULL = off). */
int zn_debug_trace(zn_handle h, void* trace_dev);
/* Test/benchmark hook: add `bias` to the codebook-0 EOS logit on every step (-inf suppresses EOS so that all
 * max_new_tokens+7 steps run). */
int zn_debug_eos_bias(zn_handle h, float bias);

/* The backbone plugin seam (zonos/backbone/__init__.py:24-36; TorchZonosBackbone.forward _torch.py:213-238,
 * MambaSSMZonosBackbone.forward _mamba_ssm.py:88-119): hidden [rows][S][d] -> out [rows][S][d] after the final norm, the
 * caches advanced by S positions.  caches_dev: host array [n_layer] of device pointers (KV cache of an attention layer,
 * conv+SSM state buffer of a Mamba2 layer); every row holds `base` keys already (InferenceParams.seqlen_offset ==
 * lengths_per_sample in every reference call site).  S = 1 runs the decode kernels, S > 1 the batched prefill kernels
 * (Mamba2 layers: sequence conv + selective scan).  Needs no zn_gen_begin. */
int zn_op_backbone_forward(zn_handle h, const void* hidden_dev, void* out_dev, const void* const* caches_dev, int32_t max_len,
                           int32_t base, int32_t S, int32_t rows, zn_stream stream);

/* ---------------------------------------------------------------- measurement */
/* Average duration (HIP events on `stream`) of one of the decode step's weight-streaming kernels over `iters`
 * launches that cycle through the layers' weights, and its algorithmic bytes per launch (the weight matrix).
 * which: 0 = LayerNorm+fc1+SiLU-gate (5..16 rows: the one launch a decode step makes there, fc1 normalising from the statistics its
 * producer left - that producer runs once outside the timed loop; zn_debug_tune(ZN_TUNE_FC1_LN_LAUNCH, 2): the LayerNorm launch + fc1), 1 = fc2+residual, 2 = out_proj+residual, 3 = LayerNorm+heads,
 * 4 = LayerNorm+in_proj+RoPE+KV-append (into a scratch cache), 5 = the persistent post-attention chain of one block
 * (out_proj twice, LayerNorm+fc1+SiLU-gate, fc2, next block's LayerNorm+in_proj+RoPE+KV-append in ONE launch: batch 1 only;
 * bytes = those four weight matrices, out_proj counted once), 6 = the whole-step kernel (every block of a decode step and the heads in
 * ONE launch, one or two rows) on scratch KV caches of its own holding `ctx` keys per row; bytes = every weight the step reads once
 * (in_proj of block 0 included: the launch's pre-block; excluded under zn_debug_tune(ZN_TUNE_STACK_PRE, 2), where it is a launch of its own) + K/V of
 * ctx keys read and one row written per layer, 7 = the Mamba2 in_proj with its conv-window epilogue (hybrid handles; a scratch window; cycles through
 * the Mamba2 layers; every launch of the plan's launch set counts as one: ms_per_launch prices the projection over all its rows), 8 = the Mamba2 out_proj
 * (hybrid handles; store; cycles through the Mamba2 layers; no prologue from 5 rows on or with several norm groups, else - up to 4 rows - the gated norm as its prologue
 * on zeroed gated values, as a step launches it).  7 and 8 read what a decode step would read: the FP8 stream where zn_set_mamba_fp8 attached one (up to 4 rows: under
 * ZN_TUNE_FP8_SMALL_ROWS = 2 only); bytes stay those of the bf16 matrix.  0 and 1 at up to 4 rows likewise read the stream of zn_set_mlp_fp8 under that key, when every
 * block has one; from 5 rows on they price the bf16 launches.
 * rows: bits 0-7 = activation rows; bit 8 = keep streaming layer 0's weights (cache-hot variant); bits 16-30 = ctx for which == 6
 * (0 = 450, the mean context of a 10 s utterance). */
int zn_bench_kernel(zn_handle h, int32_t which, int32_t rows, int32_t iters, float* ms_per_launch,
                    double* bytes_per_launch, zn_stream stream);

/* ---------------------------------------------------------------- single ops (parity tests call these) */
/* nn.LayerNorm + nn.Linear(no bias): out[r,n] = bf16(sum_k LN(x)[r,k] W[n,k]); ln_w == NULL skips the norm. */
int zn_op_linear(zn_handle h, const void* x_dev, const void* ln_w, const void* ln_b, const void* W_dev,
                 void* out_dev, int32_t rows, int32_t N, int32_t K, zn_stream stream);
/* One fused linear through the production dispatch, for per-op tests: plan_linear over the handle's settings and workspace, then the launcher
 * the decode step and the prefill use, for the (prologue, epilogue) pairs they instantiate - no prologue or LayerNorm x {store, residual,
 * SiLU gate, fp32, split + RoPE + KV append}, gated norm x store; any other pair is ZN_ERR_UNSUPPORTED.  pro / epi: 0 none, 1 LayerNorm,
 * 2 gated RMS norm (gv: fp32 [rows][K]) / 0 store (+ optional bias), 1 residual, 2 SiLU gate (out [rows][N / 2]), 3 RoPE + KV append (q_out
 * [rows][Hq * hd], kv [rows][max_len][2][Hkv][hd], lengths int32 [rows]; head geometry and RoPE table are the handle's; prefill: activation
 * row r * pf_S + s is position pf_base + s of cache row r, and out [rows][N] receives the plain projection when plan[ZN_LP_ROPE_DONE] is 0),
 * 4 fp32 (out_f32).  want_ln_stats_out: leave LayerNorm statistics of the output rows in the handle when the plan can; ln_stats_in = 1:
 * normalise from the statistics the previous call on this handle left there.  plan[] (ZN_LP_*) is filled even on error.  ZN_ERR_ARG, before
 * any launch, when a launch would outrun a workspace of the handle (LayerNorm launch buffer, statistics buffer). */
enum zn_linear_plan_field {
  ZN_LP_KERNEL = 0,      /* 0 GEMV, 1 GEMM16, 2 GEMM16S, 3 GEMM16K, 4 GEMM64S, 5 tiled GEMM */
  ZN_LP_EPI = 1, ZN_LP_KS = 2, ZN_LP_NCH = 3, ZN_LP_UPW = 4, ZN_LP_BLOCKS = 5, ZN_LP_FULL = 6, ZN_LP_NW = 7, ZN_LP_TILE8 = 8, ZN_LP_NWV = 9,
  ZN_LP_GROUPS = 10, ZN_LP_KSPLIT = 11, ZN_LP_LNP = 12, ZN_LP_LN_PRO = 13, ZN_LP_LN_LAUNCH = 14, ZN_LP_WRITES_LN_STATS = 15,
  ZN_LP_READS_LN_STATS = 16, ZN_LP_ERR = 17, ZN_LP_ROPE_DONE = 18, ZN_LP_ROWS_PER_LAUNCH = 19,
  ZN_LP_W8 = 20,         /* 1 = the launch read the weights as an FP8 stream (zn_op_linear_fp8) */
  ZN_LP_ROW_TILES = 21,  /* 16-row activation blocks per weight pass: 1, or 2 .. 4 under the wide plan (ZN_TUNE_WIDE_ROWS; then ZN_LP_ROWS_PER_LAUNCH = 64) */
  ZN_LP_NFIELDS = 24
};
typedef struct zn_linear_op {
  int32_t pro, epi, rows, N, K, prefill, target_blocks, want_ln_stats_out, ln_stats_in;
  int32_t max_len, pf_S, pf_base;
  const void *x, *W, *ln_w, *ln_b, *gv, *bias, *resid;
  void *out, *out_f32;
  const int32_t* lengths;
  void *kv, *q_out;
  int32_t plan[24];
} zn_linear_op;
int zn_op_linear_fused(zn_handle h, zn_linear_op* op, zn_stream stream);

/* ---------------------------------------------------------------- weight-only FP8 for the MLP projections (additive to ABI 9: new entry points,
 * one new tune key, one new plan field; no existing call or layout changes.  ZN_ABI_VERSION does not tell whether a library has them: a
 * client that may meet an older libzonos_hip.so looks the symbols up (dlsym / hasattr) before it calls them)
 * Format (specification: zonos_amd/quant.py): OCP E4M3 codes uint8 [N][K] and one scale exponent int8 [N] per weight row, weight = value(code) * 2^exp.
 * exp = ceil(log2(amax_row / 448)) clamped to [-100, 100] (0 for a zero row); codes round to nearest even and saturate at +-448; the NaN codes
 * are never produced.  A code has 3 mantissa bits, so the dequantised weight is exact in bf16.  Lossy with respect to the weights quantised
 * (|Wdq - w| <= 2^-4 |w| in the codes' normal range, <= 2^-10 * 2^exp in their subnormal range), exact with respect to the dequantised ones. */
/* W bf16 [N][K] -> q uint8 [N][K], exp int8 [N].  K a multiple of 8.  Bit-identical to quantize_rows_fp8 of zonos_amd/quant.py. */
int zn_op_fp8_quantize_rows(zn_handle h, const void* W_dev, int32_t N, int32_t K, void* q_dev, void* exp_dev, zn_stream stream);
/* q, exp -> W_out bf16 [N][K] = value(q) * 2^exp, exact.  K a multiple of 8, every exp in [-100, 100] (the caller's to ensure). */
int zn_op_fp8_dequant_rows(zn_handle h, const void* q_dev, const void* exp_dev, int32_t N, int32_t K, void* W_out_dev, zn_stream stream);
/* Attaches the FP8 stream of fc1 [2 d_ff][d_model] and fc2 [d_model][d_ff] of transformer block `layer`; all four pointers NULL detaches it.
 * CONTRACT: the layer's bf16 fc1 and fc2 (zn_layer_weights) hold exactly the dequantised stream.  Decode launches of 5..64 rows per weight pass (groups of 16 rows, or
 * up to 64 under the wide plan of 17 rows and more: ZN_TUNE_WIDE_ROWS) then read the codes (half the bytes) and compute the same bits, and under ZN_TUNE_FP8_SMALL_ROWS = 2 so do the GEMV launches of 1..4 rows; every other path keeps reading the bf16 copy, so one model computes one function
 * on every path.  The library does not check the contract unless ZN_FP8_VERIFY=1 is in the environment of this call: then both matrices are
 * compared on the device and a mismatch is ZN_ERR_ARG (nothing is attached).  The caller keeps the memory alive while it is attached.  Drops the
 * captured graphs.  ZN_ERR_UNSUPPORTED: a hybrid handle (arch 1), a Mamba2 layer, d_model or d_ff no multiple of 256.  ZN_ERR_STATE: between
 * zn_gen_begin and zn_gen_end.  ZN_ERR_ARG: a layer out of range, or some but not all pointers NULL. */
int zn_set_mlp_fp8(zn_handle h, int32_t layer, const void* fc1_q, const void* fc1_exp, const void* fc2_q, const void* fc2_exp);
/* zn_op_linear_fused with the weights offered as an FP8 stream as well (op->W: the dequantised bf16 copy, still required): the production
 * plan, and where it launches gemm16s_kernel (or, 17..64 rows under the wide plan, gemm16w_kernel) in decode for no prologue or LayerNorm x SiLU gate (fc1) or no prologue x residual (fc2), that
 * launch reads W_q / W_exp - plan[ZN_LP_W8] = 1, every other plan field as zn_op_linear_fused reports it.  Refused before any launch, as
 * ZN_ERR_UNSUPPORTED: any other (prologue, epilogue) pair, a prefill op, K no multiple of 256, a plan that would not read the stream
 * (zn_debug_tune(ZN_TUNE_MLP_FP8, 2) included). */
int zn_op_linear_fp8(zn_handle h, zn_linear_op* op, const void* W_q, const void* W_exp, zn_stream stream);
/* Reads the decode step's own table of linears (zn_step_linears.h), as the launches do.
 * out[0], out[1]: whether fc1 and fc2 of a decode step over `rows` rows would read FP8 in EVERY block of this handle now (the tune keys; a
 * handle with streams attached to some blocks only reports 0, 0 although those blocks do read them).  rows <= 4 says what the launches path (the GEMV)
 * reads: 1, 1 only under zn_debug_tune(ZN_TUNE_FP8_SMALL_ROWS, 2); a generation that runs on a persistent kernel reads the bf16 copy whatever this reports. */
int zn_mlp_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]);
/* ---------------------------------------------------------------- weight-only FP8 for the Mamba2 projections of a hybrid handle (additive to ABI 9 in the same way:
 * two entry points and one tune key; look the symbols up).  Same format, same quantiser (zn_op_fp8_quantize_rows).
 * Attaches the FP8 stream of in_proj [d_in_proj][d_model] and out_proj [d_model][d_inner] of Mamba2 layer `layer`; all four pointers NULL detaches it.
 * CONTRACT, as for zn_set_mlp_fp8: the layer's bf16 m_in_proj and m_out_proj (zn_layer_weights) hold exactly the dequantised stream.  Decode launches of
 * 5..64 rows per weight pass (zn_op_mamba_step, decode steps, serving sessions, captured graphs) then read the codes and compute the same bits; rows <= 4 (the
 * GEMV with the gated-norm prologue; unless ZN_TUNE_FP8_SMALL_ROWS = 2) and the prefill keep reading the bf16 copy.  ZN_FP8_VERIFY=1 in the environment of this call: both matrices are compared on
 * the device, a mismatch is ZN_ERR_ARG and attaches nothing.  The caller keeps the memory alive while it is attached.  Drops the captured graphs.
 * ZN_ERR_UNSUPPORTED: a transformer handle, an attention layer of a hybrid handle, widths the FP8 kernels do not serve (d_model != 2048 or d_inner != 4096).
 * ZN_ERR_STATE: between zn_gen_begin and zn_gen_end.  ZN_ERR_ARG: a layer out of range, or some but not all pointers NULL. */
int zn_set_mamba_fp8(zn_handle h, int32_t layer, const void* in_q, const void* in_exp, const void* out_q, const void* out_exp);
/* Reads the decode step's own table of linears (zn_step_linears.h), as the launches do.
 * out[0], out[1]: whether in_proj and out_proj of a decode step over `rows` rows would read FP8 in EVERY Mamba2 layer of this handle now (the tune keys; a
 * handle with streams attached to some Mamba2 layers only, or with no Mamba2 layer, reports 0, 0).  rows <= 4: 1, 1 only under
 * zn_debug_tune(ZN_TUNE_FP8_SMALL_ROWS, 2), where the GEMV launches read the stream too. */
int zn_mamba_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]);
/* ---------------------------------------------------------------- FP8 KV cache for the decode attention at 5 rows and more (additive to ABI 9 in the same way: look the
 * symbols up).  Off by default; with it off nothing changes in any path, buffer or result.
 * Format (specification: kv_round_e4m3 of zonos_amd/quant.py): OCP E4M3 codes at scale exponent 0 - no scale: the fused append holds two elements of a head vector per
 * thread and cannot take an absmax.  Round to nearest even; finite values and the infinities saturate at +-448; NaN stays NaN.  Lossy with respect to the bf16 model
 * (|dq - x| <= 2^-4 |x| in the codes' normal range, <= 2^-10 below 2^-6), exact with respect to its own rounded cache.
 * While the mode is in effect - a generation or session (zn_gen_begin, zn_gen_open_slots) on a handle with the mode on whose decode step has 5 rows or more (the launches
 * path; more than 64 rows run in groups, as without the mode) - every KV append of that generation (the decode steps' in_proj epilogue, the prefill's epilogue and
 * rope_kv_rows_kernel, an admission's prefill) rounds K (after RoPE) and V to the E4M3 grid, writes the dequantised bf16 values into the cache of zn_gen_begin, so that every
 * reader, the prefill attention included, sees the rounded values, and writes the one-byte codes into a second cache uint8 [rows][max_len][2][Hkv][hd] per layer, which
 * the decode attention then reads instead (half the bytes, the same bits).  With fewer rows the mode is inert: nothing is rounded (the persistent kernels and the
 * 1..4-row GEMV).  The bf16 cache stays allocated and current: the mode costs 1.5 x the KV bytes, unless zn_set_kv_fp8_only (below) drops the bf16 cache. */
/* on != 0 switches the mode on for the generations begun afterwards.  ZN_ERR_UNSUPPORTED: a hybrid handle (arch 1: its attention layers stay bf16).  ZN_ERR_STATE: between
 * zn_gen_begin and zn_gen_end.  Drops the captured graphs. */
int zn_set_kv_fp8(zn_handle h, int32_t on);
/* Bytes of one layer's code cache [rows, max_len, 2, Hkv, hd] uint8: half of zn_kv_bytes_per_layer, which keeps reporting the bf16 cache alone. */
size_t zn_kv_fp8_bytes_per_layer(const zn_config* cfg, int32_t rows, int32_t max_len);
/* The code caches of the generation begun by zn_gen_begin: a host array of n_layer device pointers, caller-owned like the bf16 caches and with their rows and max_len.
 * Legal where zn_gen_set_rows is (before or after zn_gen_open_slots).  A generation in which the mode is in effect needs this call: its prefill, admissions and decode
 * steps return ZN_ERR_STATE without it.  Where the mode is not in effect (mode off, fewer than 5 rows) the call is accepted and the caches are never touched. */
int zn_gen_bind_kv_fp8(zn_handle h, const void* const* codes_layers_dev);
/* out[0]: whether a generation of `rows` rows begun on this handle now rounds its K/V (the mode is on and in effect at that row count); out[1]: whether its decode
 * attention reads the codes (out[0], ZN_TUNE_KV_FP8 != 2, and the row count is one the plan has not declined: see DESIGN.md 4.1k). */
int zn_kv_fp8_plan(zn_handle h, int32_t rows, int32_t out[2]);
/* Codes only: a second flag that matters only in a generation where the FP8 KV cache is in effect (zn_set_kv_fp8 on, transformer, 5 rows or more).  Such a
 * generation keeps no bf16 cache: the bound code caches (zn_gen_bind_kv_fp8) are its only KV storage - half the bytes of the bf16 model's cache, a third of the two-cache
 * mode's - and the same bits as the two-cache mode everywhere.  zn_gen_begin then accepts kv_layers_dev == NULL or NULL entries, and neither reads nor writes what is passed
 * anyway; every KV append writes the codes alone; the decode attention and the prefill attention (FP8 forms of both prefill kernels, zn_prefill_attn_fp8_kernels.h) read them;
 * an admission's library-owned scratch cache holds codes.  Without bound code caches the prefill, admissions and decode steps return ZN_ERR_STATE, as in the two-cache
 * mode: never a silent bf16 generation.  ZN_TUNE_KV_FP8 = 2 is ignored for such a generation.  With the FP8 KV cache off or not in effect the flag changes nothing.
 * The refusals of zn_set_kv_fp8: ZN_ERR_UNSUPPORTED on a hybrid handle, ZN_ERR_STATE between zn_gen_begin and zn_gen_end.  Drops the captured graphs. */
int zn_set_kv_fp8_only(zn_handle h, int32_t on);
/* out[0], out[1]: as zn_kv_fp8_plan (rounded; the decode attention reads the codes); out[2]: whether a generation of `rows` rows begun on this handle now needs the bf16
 * caches of zn_gen_begin (0: codes only). */
int zn_kv_cache_plan(zn_handle h, int32_t rows, int32_t out[3]);
/* Per-op tests: while codes_dev != NULL, zn_op_linear_fused's RoPE + KV append (decode and prefill epilogue) and zn_op_rope_kv_rows round and write the codes of the cache
 * they append to into codes_dev (same rows and max_len as that cache), and zn_op_attn_decode reads codes_dev where zn_kv_fp8_plan's out[1] would be 1 for its row count
 * with the mode on.  NULL (the default) restores the bf16 behaviour.  Independent of zn_set_kv_fp8. */
int zn_op_bind_kv_fp8(zn_handle h, void* codes_dev);
/* While a code cache is bound, the bf16 cache of those entry points may be NULL: zn_op_linear_fused's RoPE + KV append and zn_op_rope_kv_rows then write the codes alone,
 * and zn_op_attn_decode accepts kv_dev == NULL where it reads the codes.  Without a bound code cache (or where the codes are not read) a NULL cache stays ZN_ERR_ARG. */
/* The prefill's row-wise split + RoPE + KV append alone (rope_kv_rows_kernel, what follows a projection whose plan reports ZN_LP_ROPE_DONE = 0): qkv bf16
 * [rows][S][(Hq + 2 Hkv) hd], q rotated in place, k and v to positions base .. base + S - 1 of kv [rows][max_len][2][Hkv][hd]; positions at or past max_len write nothing. */
int zn_op_rope_kv_rows(zn_handle h, void* qkv_dev, void* kv_dev, int32_t max_len, int32_t S, int32_t base, int32_t rows, zn_stream stream);
/* ---------------------------------------------------------------- decode steps of 17..64 rows (additive to ABI 9, like the FP8 calls above: look the symbol up)
 * out[0..4]: activation rows per weight pass of in_proj, out_proj, fc1, fc2 and the heads in a decode step of `rows` rows as this handle would
 * run it now - the query reads the step's own table of linears (zn_step_linears.h), which the launches plan from - (4 up to 4 rows, 16 up to 16 rows and under zn_debug_tune(ZN_TUNE_WIDE_ROWS, 1), 64 where the wide plan applies): a step of R rows
 * reads the projection's weights ceil(R / out[k]) times. */
int zn_decode_rows_plan(zn_handle h, int32_t rows, int32_t out[5]);
/* The same report for a hybrid handle (arch 1), read from the same table: out[0..6] = Mamba2 in_proj, Mamba2 out_proj, attention in_proj, out_proj,
 * fc1, fc2, heads (the first layer of each kind; 0 for a kind the stack does not have).  ZN_ERR_STATE on a transformer handle. */
int zn_hybrid_rows_plan(zn_handle h, int32_t rows, int32_t out[7]);
/* Prefix-conditioner pieces (zonos/conditioning.py): nn.Linear with bias (Conditioner.project, :52-60; bias added in fp32
 * before the one bf16 rounding), nn.Embedding row gather (:364-365,467), FourierConditioner.apply_cond (:436-441), nn.SiLU. */
int zn_op_linear_bias(zn_handle h, const void* x_dev, const void* W_dev, const void* bias_dev, void* out_dev, int32_t rows,
                      int32_t N, int32_t K, zn_stream stream);
int zn_op_gather_rows(zn_handle h, const void* table_dev, const int32_t* ids_dev, void* out_dev, int32_t n, int32_t d,
                      int32_t table_rows, int32_t id_offset, zn_stream stream);
int zn_op_fourier(zn_handle h, const float* x_dev, const void* weight_dev, void* out_dev, int32_t n, int32_t in_dim,
                  int32_t half, float min_val, float max_val, zn_stream stream);
int zn_op_silu(zn_handle h, const void* x_dev, void* out_dev, int64_t n, zn_stream stream);
/* nn.LayerNorm (_torch.py:155 norm_f): bf16 [rows, d] -> bf16 [rows, d], fp32 statistics. */
int zn_op_layernorm(zn_handle h, const void* x_dev, const void* w_dev, const void* b_dev, void* out_dev, int32_t rows,
                    int32_t d, zn_stream stream);
/* One decode step of TransformerBlock `layer` (_torch.py:307-328) on x bf16 [rows, d] in place, reading and
 * appending to kv_dev at position lengths_dev[r]; ext_dev (optional, int32[rows]) = number of keys the
 * reference's CPU flash-attention block sees for that row (prefill emulation), NULL = lengths+1. */
int zn_op_layer_decode(zn_handle h, int32_t layer, void* x_dev, void* kv_dev, int32_t max_len,
                       const int32_t* lengths_dev, const int32_t* ext_dev, int32_t rows, zn_stream stream);
/* Decode attention alone (_torch.py:413-417): q bf16 [rows, Hq*hd] (post-RoPE), kv [rows, max_len, 2, Hkv, hd] holding
 * lengths[r]+1 keys -> out bf16 [rows, Hq*hd]; reproduces the CPU flash-attention rounding points. */
int zn_op_attn_decode(zn_handle h, const void* q_dev, const void* kv_dev, int32_t max_len, const int32_t* lengths_dev,
                      const int32_t* ext_dev, void* out_dev, int32_t rows, zn_stream stream);
/* Causal prefill attention alone (_torch.py:413-417 with is_causal=True, the S > 1 call): q bf16 [rows, positions, Hq*hd]
 * (post-RoPE), kv [rows, max_len, 2, Hkv, hd] holding the keys of positions 0..positions-1 -> out bf16
 * [rows, positions, Hq*hd]; same CPU flash-attention rounding points as zn_op_attn_decode, incl. its query-block split. */
int zn_op_attn_prefill(zn_handle h, const void* q_dev, const void* kv_dev, int32_t max_len, void* out_dev, int32_t positions,
                       int32_t rows, zn_stream stream);
/* Test entry: the same attention with the two arguments the ragged prefill and the seam use.  `base` keys are already cached per row:
 * position s sees keys 0..base+s, and base + positions <= max_len.  row_len_dev (int32[rows], may be NULL): row r holds
 * row_len[r] <= positions valid positions and takes the query split of a sequence of that length; positions at or past it are neither
 * read as keys nor written.  Refused before any launch: base < 0, base + positions > max_len, a null pointer, rows > max_rows. */
int zn_op_attn_prefill_rows(zn_handle h, const void* q_dev, const void* kv_dev, int32_t max_len, void* out_dev, int32_t positions,
                            int32_t rows, int32_t base, const int32_t* row_len_dev, zn_stream stream);
/* The same call on a code cache uint8 [rows, max_len, 2, Hkv, hd] of E4M3 codes (the FP8 KV cache's format, zn_set_kv_fp8): the FP8 forms of the two prefill
 * attention kernels, which a codes-only generation (zn_set_kv_fp8_only) runs.  The output has the bits of zn_op_attn_prefill_rows on the dequantised codes.  The same
 * refusals.  Additive to ABI 9: look the symbol up. */
int zn_op_attn_prefill_rows_fp8(zn_handle h, const void* q_dev, const void* codes_dev, int32_t max_len, void* out_dev, int32_t positions,
                                int32_t rows, int32_t base, const int32_t* row_len_dev, zn_stream stream);
/* mamba_ssm layer_norm_fn(prenorm=True) of the hybrid Block: s = h + res (fp32), res <- bf16(s) in place (res NULL:
 * s = h), out = bf16(LayerNorm(s)).  h/out bf16 [rows, d].  flags bit 0: RMSNorm instead of LayerNorm (rms_norm; b may be
 * NULL), bit 1: res is float [rows, d] and keeps the unrounded sum (residual_in_fp32). */
int zn_op_add_layernorm(zn_handle h, const void* hidden, void* res, const void* w, const void* b, void* out, int32_t rows,
                        int32_t d, float eps, int32_t flags, zn_stream stream);
/* One token through the Mamba2 mixer of hybrid layer `layer` (mamba_ssm Mamba2.step): x bf16 [rows, d] (already
 * normalised), state = the layer's zn_mamba_state_bytes_per_layer buffer (updated), out bf16 [rows, d]. */
int zn_op_mamba_step(zn_handle h, int32_t layer, const void* x, void* state, void* out, int32_t rows, zn_stream stream);
/* embed_codes_static (codec_utils.py:37): codes int32 [B, n_codebooks] -> bf16 [B, d], sequential bf16 adds. */
int zn_op_embed(zn_handle h, const int32_t* codes_dev, void* out_dev, int32_t batch, zn_stream stream);
/* sample_from_logits (sampling.py:166-231) on fp32 logits [B, n_codebooks, vocab_head]; recent int32
 * [B, n_codebooks, window] or NULL; tokens int32 [B, n_codebooks]; probs_out (optional) receives the filtered
 * probabilities the Gumbel-max draw uses. */
int zn_op_sample(zn_handle h, const float* logits_dev, const int32_t* recent_dev, int32_t window,
                 const zn_sampling* sp, uint64_t draw_index, int32_t* tokens_dev, float* probs_out_dev,
                 int32_t batch, zn_stream stream);
/* The right-padded prefill rows of utterances with conditionings and audio prefixes of their own lengths, in one launch: for the `rows`
 * rows (rows == batch, or 2 * batch = [cond ‖ uncond]; b = r mod batch) hidden bf16 [rows, S, d] receives
 * [cond_dev[r, :L_b] ‖ embed(delayed_codes_dev[b, :, 0 : P_b + 1]) ‖ zeros] and row_len_dev[r] = L_b + P_b + 1.  cond_dev bf16
 * [rows, L_c, d]; cond_len_dev, prefix_len_dev int32 [batch] (DEVICE; clamped to L_c and t_total - 1); delayed_codes_dev int32
 * [batch, n_codebooks, t_total]; S >= max_b (L_b + P_b + 1) is the caller's to ensure (positions at or beyond S are not written).  The
 * embedded positions carry the bits of zn_op_embed. */
int zn_op_assemble_prefill(zn_handle h, const void* cond_dev, int32_t L_c, const int32_t* cond_len_dev, const int32_t* delayed_codes_dev,
                           int32_t t_total, const int32_t* prefix_len_dev, int32_t batch, int32_t rows, void* hidden_dev, int32_t S,
                           int32_t* row_len_dev, zn_stream stream);
/* ABI 9 - zn_op_sample with a table: rows_dev is a DEVICE array of `batch` entries, row b sampled with rows_dev[b].sp (cfg_scale and
 * max_new_tokens are not used: the logits are final) and the slot-independent key of zn_gen_set_rows.  Row b's tokens and probabilities
 * equal zn_op_sample(batch = 1) on row b's logits and history with rows_dev[b].sp. */
int zn_op_sample_rows(zn_handle h, const float* logits_dev, const int32_t* recent_dev, int32_t window, const zn_row_params* rows_dev,
                      uint64_t draw_index, int32_t* tokens_dev, float* probs_out_dev, int32_t batch, zn_stream stream);

/* ---------------------------------------------------------------- DAC decode (autoencoder.py:119-170) */
typedef struct zn_dac_config { /* transformers DacConfig fields used by decode / encode */
  int32_t n_codebooks, codebook_size, codebook_dim, hidden_size, decoder_hidden_size;
  int32_t n_ratios; int32_t ratios[8]; /* upsampling_ratios, e.g. 8,8,4,2 (downsampling_ratios = reversed) */
  int32_t encoder_hidden_size;         /* 64; 0 = no encoder */
} zn_dac_config;
typedef struct zn_dac_tensor { const char* name; const float* data_dev; int64_t numel; } zn_dac_tensor;
/* Weights by their transformers state-dict names (fp32, device).  The library re-lays them out once.  Decode runs on the bf16 matrix
 * cores with three-term fp32 operands (zn_conv3_kernels.h; waveform RMS error vs the reference 1e-6, as on the fp32 matrix cores);
 * ZONOS_DAC_CONV=fp32 in the environment of this call keeps the decoder on the fp32 matrix cores (development: A/B of the two). */
int zn_dac_create(const zn_dac_config* cfg, const zn_dac_tensor* tensors, int32_t n_tensors, zn_dac* out);
int zn_dac_destroy(zn_dac d);
const char* zn_dac_last_error(zn_dac d);
/* DACAutoencoder.decode: codes int32 [B, n_codebooks, T] -> wav fp32 [B, 1, hop*T]. */
int zn_dac_decode(zn_dac d, const int32_t* codes_dev, int32_t batch, int32_t T, float* wav_dev, zn_stream stream);
/* ABI 7 - span decode (streaming).  A window of code frames [c0, c0 + n) of a longer sequence; at_end != 0 says that c0 + n is the
 * sequence's true end.  zn_dac_span (host only, no handle, no device) gives the largest sample range [s0, s1) whose receptive field
 * lies inside the window: frame 0 is a true left edge (the decoder's zero padding applies there), c0 + n a right edge only when
 * at_end.  s0 == s1 when the window holds no complete sample.  The receptive field follows from cfg->ratios (7-tap residual convs with
 * dilations 1/3/9, ConvTranspose1d k = 2s pad ceil(s/2), the 7-tap convs at both ends). */
int zn_dac_span(const zn_dac_config* cfg, int32_t c0, int32_t n, int32_t at_end, int64_t* s0, int64_t* s1);
/* codes int32 [B, n_codebooks, n] = frames [c0, c0 + n) -> wav fp32 [B, s1 - s0]: samples [s0, s1) of zn_dac_span, bit-identical to the
 * same samples of a whole-sequence zn_dac_decode on the three-term path.  No state is kept between calls.  ZN_ERR_UNSUPPORTED on a
 * handle built with ZONOS_DAC_CONV=fp32; ZN_ERR_ARG when the range is empty. */
int zn_dac_decode_span(zn_dac d, const int32_t* codes_dev, int32_t batch, int32_t c0, int32_t n, int32_t at_end, float* wav_dev,
                       zn_stream stream);
/* Ragged span decode (Zonos.serve_stream): one pass over the decoder's layers for `rows` windows, each with its own place in its own
 * sequence (1 <= rows <= 64).  ZN_ERR_ARG, naming the row and launching nothing, when a row's span is empty, n_r > n_max or
 * s1_r - s0_r > t_max; ZN_ERR_UNSUPPORTED on a ZONOS_DAC_CONV=fp32 handle or when one row's window passes zn_dac_decode_span's limit. */
typedef struct zn_dac_span_row { int32_t c0, n, at_end; } zn_dac_span_row;   /* HOST array */
/* codes int32 [rows, n_codebooks, n_max]: row r holds frames [c0_r, c0_r + n_r) in its first n_r columns (cells beyond n_r are never
 * read); wav fp32 [rows, t_max]: row r receives samples [s0_r, s1_r) of zn_dac_span(c0_r, n_r, at_end_r) in its first s1_r - s0_r
 * entries (entries beyond are never written).  Row r's samples carry the bits of zn_dac_decode_span(batch = 1) on row r alone. */
int zn_dac_decode_spans(zn_dac d, const int32_t* codes_dev, int32_t n_max, const zn_dac_span_row* rows_host, int32_t rows,
                        float* wav_dev, int64_t t_max, zn_stream stream);
/* DACAutoencoder.encode (zonos/autoencoder.py:103-117 -> DacModel.encode): wav fp32 [B, T] at the codec rate, T a
 * positive multiple of the hop (preprocess pads) -> codes int32 [B, n_codebooks, T / hop].  Needs the encoder.* and
 * quantizer.quantizers.{i}.in_proj tensors at zn_dac_create. */
int zn_dac_encode(zn_dac d, const float* wav_dev, int32_t batch, int32_t T, int32_t* codes_dev, zn_stream stream);

/* ---------------------------------------------------------------- output resampling */
/* Additions (no existing call or layout changes; ZN_ABI_VERSION does not tell whether a library has them).  The filter is
 * torchaudio's sinc_interp_hann polyphase filter (zonos_amd/resample.py is the specification): with g = gcd(orig_freq, new_freq),
 * o = orig_freq / g, n = new_freq / g, base = min(o, n) * rolloff, width = ceil(lowpass_filter_width * o / base), the table
 * k fp32 [n][2 * width + o] is computed in double and rounded once; phase p's support [lo_p, hi_p) is the smallest interval holding its
 * nonzero fp32 taps.  Output j = q * n + p of a signal x of T samples (0 <= j < ceil(n * T / o)) is ONE fp32 chain
 *   acc = 0; for i = lo_p .. hi_p - 1 ascending: acc = fma(k[p][i], x[q * o - width + i], acc)        (x = 0 outside [0, T))
 * so its value depends on j and the signal only: any window that holds the inputs it reads gives the same bits. */
typedef struct zn_resampler_s* zn_resampler;
/* Host only (no handle, no device).  Writes o, n, width (each optional) and, where the pointers are given, lo / hi (int32 [n], needs
 * phases_cap >= n) and the table (fp32 [n][2 * width + o], needs table_cap >= n * (2 * width + o) elements).  ZN_ERR_ARG: a rate or
 * lowpass_filter_width < 1, rolloff outside (0, 1], a buffer too small (o, n, width are written first: call once without buffers to
 * size them).  ZN_ERR_UNSUPPORTED: a table of more than 2^22 entries.  Messages through zn_resampler_last_error(NULL). */
int zn_resample_plan(int32_t orig_freq, int32_t new_freq, int32_t lowpass_filter_width, double rolloff, int32_t* o, int32_t* n,
                     int32_t* width, int32_t* lo, int32_t* hi, int32_t phases_cap, float* table, int64_t table_cap);
/* Host only, like zn_dac_span: the arithmetic of a stream.  With `avail` input samples [0, avail) known (at_end != 0: they are the
 * whole signal), *n_final = how many leading outputs are final - output j is final once q * o - width + hi_p <= avail, and every one
 * of the ceil(n * avail / o) outputs is when at_end.  *first_in = the first input that the outputs from out_index on still read
 * (min over them of max(0, q * o - width + lo_p)); out_index < 0 stands for *n_final.  Either pointer may be NULL. */
int zn_resample_span(int32_t orig_freq, int32_t new_freq, int32_t lowpass_filter_width, double rolloff, int64_t avail, int32_t at_end,
                     int64_t out_index, int64_t* n_final, int64_t* first_in);
/* A handle keeps the plan's table on the device, laid out [tap][phase] over the supports only (consecutive lanes read consecutive
 * words); it is uploaded to the device current at the handle's first launch, so creating a handle touches no device.  orig_freq == new_freq gives the identity (o = n = 1, one tap of 1.0): no resampling, for the PCM16
 * conversion alone.  Errors before a handle exists through zn_resampler_last_error(NULL). */
int zn_resampler_create(int32_t orig_freq, int32_t new_freq, int32_t lowpass_filter_width, double rolloff, zn_resampler* out);
int zn_resampler_destroy(zn_resampler r);
const char* zn_resampler_last_error(zn_resampler r);
/* One row of zn_resample_rows (HOST array): the row holds input samples [in0, in0 + in_len) of its own signal and receives outputs
 * [out0, out0 + out_count); at_end != 0: in0 + in_len is the signal's end. */
typedef struct zn_resample_row { int64_t in0; int32_t in_len; int64_t out0; int32_t out_count; int32_t at_end; } zn_resample_row;
/* in fp32 [rows, in_max] (cells beyond in_len are never read) -> out fp32, or int16 when out_is_int16 (clamp(y * 32767, +-32767)
 * truncated toward zero, decode_to_int16's arithmetic), [rows, out_max]: row r's outputs in its first out_count cells (cells beyond
 * are never written).  One launch, one output per lane; 1 <= rows <= 64; a uniform batch is `rows` equal entries.  ZN_ERR_ARG, naming
 * the row and launching nothing: in_len > in_max, out_count > out_max, a negative field, an output that reads an input outside the
 * row's window (allowed only before sample 0, or past the end of a row with at_end), or, with at_end, an output at or beyond
 * ceil(n * (in0 + in_len) / o).  A call whose rows all have out_count == 0 launches nothing. */
int zn_resample_rows(zn_resampler r, const float* in_dev, int64_t in_max, const zn_resample_row* rows_host, int32_t rows, void* out_dev,
                     int64_t out_max, int32_t out_is_int16, zn_stream stream);

/* ---------------------------------------------------------------- speaker embedding (zonos/speaker_cloning.py) */
/* ResNet293_based (speaker_cloning.py:419-472: ResNet293 of SimAM blocks -> ASP -> bottleneck Linear) and the LDA Linear
 * of SpeakerEmbeddingLDA (:800-883), fp32.  Tensors by the reference's state-dict names (front.*, pooling.*,
 * bottleneck.*; optionally lda.weight / lda.bias), device pointers that must outlive the handle; BatchNorm is folded
 * when the handle is built.  Runs once per speaker, outside the decode loop. */
int zn_spk_create(const zn_dac_tensor* tensors, int32_t n_tensors, zn_spk* out);
int zn_spk_destroy(zn_spk d);
const char* zn_spk_last_error(zn_spk d);
/* feat fp32 [B, n_mels, T]: mean-normalised log-mel features (what logFbankCal returns, speaker_cloning.py:81-87), T >= 8
 * -> emb fp32 [B, emb_dim] (bottleneck output) and, if lda_out != NULL, lda_out fp32 [B, lda_dim]. */
int zn_spk_embed(zn_spk d, const float* feat_dev, int32_t batch, int32_t T, float* emb_dev, float* lda_out_dev, zn_stream stream);

#ifdef __cplusplus
}
#endif
#endif

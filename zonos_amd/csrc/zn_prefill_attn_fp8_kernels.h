// The FP8 forms of the prefill attention (zn_set_kv_fp8_only): attn_prefill_fp8_kernel and attn_prefill_mfma_fp8_kernel are the bodies of
// attn_prefill_kernel and attn_prefill_mfma_kernel (zn_prefill_kernels.h) with the source of the staged K and V tiles changed and nothing else.
// The code cache has the layout of the bf16 cache with one byte per element, so every address is the bf16 kernel's element offset (clamped the
// same way).  For each 16-byte piece slot of the LDS tile a lane requests the 8 codes (8 bytes) of the same 8 elements, widens them with
// v_cvt_scalef32_pk_bf16_fp8 at scale 1 (AttnKvFp8::ld8) and stores the 16 bytes into the slot the bf16 form fills; the select that zeroes the rows
// at or past the workgroup's last visible key follows the widening, as it follows the load in the bf16 form.  A code is exact in bf16, so the LDS
// tiles hold what the bf16 form stages from the dequantised cache: MFMA operands, the two passes, summation orders, masking and the epilogue are
// shared source, and the result is the same bits.  (16 codes per request and two piece slots per lane: measured, 0.7 us of a 37 us launch at 200
// positions and nothing at 2600 - declined)
#pragma once
#include "zn_prefill_kernels.h"
#include "zn_attn_fp8_kernels.h"

struct PrefillKvFp8 : AttnKvFp8 {
  static ZN_DEVINL const elem* cache(const PrefillAttnArgs& a) { return a.kv8; }
};

template <int HD, int G>
__global__ __launch_bounds__(256) void attn_prefill_fp8_kernel(PrefillAttnArgs a) { attn_prefill_body<HD, G, PrefillKvFp8>(a); }
template <int G>
__global__ __launch_bounds__(256) void attn_prefill_mfma_fp8_kernel(PrefillAttnArgs a) { attn_prefill_mfma_body<G, PrefillKvFp8>(a); }

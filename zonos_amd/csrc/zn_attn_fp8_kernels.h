// The FP8 forms of the decode attention (zn_set_kv_fp8): attn_scores_fp8_kernel and attn_block_fp8_kernel are the bodies of
// attn_scores_kernel and attn_block_kernel (zn_decode_kernels.h) with the source of the K tile and of the V tile changed and nothing else.
// The code cache has the layout of the bf16 cache with one byte per element, so every address is the bf16 kernel's element offset
// (clamped the same way); a lane requests 8 codes (8 bytes) where the bf16 form requests 8 bf16 (16 bytes) - 4 or 2 where a value-column
// part is narrower - and widens them with v_cvt_scalef32_pk_bf16_fp8 at scale 1 into the registers the bf16 form loads.  A code is exact in bf16
// and the appends keep the bf16 cache equal to the dequantised codes (kv_fp8_round_pair), so the MFMAs see the operands of the bf16 form reading
// that cache: LDS layouts, operands, summation orders and masking are shared source, and the result is the same bits.
#pragma once
#include "zn_decode_kernels.h"

struct AttnKvFp8 {
  typedef uint8_t elem;
  static ZN_DEVINL const elem* cache(const AttnArgs& a) { return a.kv8; }
  static ZN_DEVINL u32x4 ld8(const elem* p) { return fp8x8_to_bf16(*(const u32x2*)p, 1.0f); }
  static ZN_DEVINL u32x2 ld4(const elem* p) { return fp8x4_to_bf16(*(const unsigned*)p, 1.0f); }
  static ZN_DEVINL unsigned ld2(const elem* p) { return kv_fp8x2_to_bf16(*(const unsigned short*)p); }
};

template <int HD, int G>
__global__ __launch_bounds__(256) void attn_scores_fp8_kernel(AttnArgs a) { attn_scores_body<HD, G, AttnKvFp8>(a); }
template <int HD, int G, bool FUSED, int DS = 1>
__global__ __launch_bounds__(512) void attn_block_fp8_kernel(AttnArgs a) { attn_block_body<HD, G, FUSED, DS, AttnKvFp8>(a); }

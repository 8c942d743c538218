// Weight-only FP8 (OCP E4M3 codes, one power-of-two scale 2^k per weight row; specification: zonos_amd/quant.py).  A code has 3 mantissa
// bits, so code * 2^k is exact in bf16: the FP8 bytes are a compressed stream of bf16 weights, and a kernel that reads them hands the same
// bf16 operands to the same MFMAs as one that reads the bf16 copy.  Here: the dequantisation every reader shares, the load-time quantiser,
// the dequantiser and the compare kernel behind ZN_FP8_VERIFY.  The hot path is gemm16s_kernel<., NWV | ZN_G16S_W8> (zn_decode_kernels.h).
#pragma once
#include "zn_common.h"

#ifndef ZN_FP8_CVT_SCALEF32
#define ZN_FP8_CVT_SCALEF32 1      // 0: fp8x4_to_bf16 through v_cvt_pk_f32_fp8 + fp32 multiplies (see there)
#endif
#define ZN_FP8_EXP_MIN (-100)
#define ZN_FP8_EXP_MAX 100

typedef __attribute__((ext_vector_type(2))) float zn_f32x2;

// 2^k as fp32, k in [-100, 100] (a normal number)
ZN_DEVINL float fp8_row_scale(int k) { return __uint_as_float((unsigned)(k + 127) << 23); }

// 4 codes (byte i of v = element i) and the row's scale -> 4 bf16 (lo: elements 0, 1; hi: 2, 3), exactly: a 3-bit mantissa fits bf16's 7 and
// |value| lies in [2^-109, 448 * 2^100] - no denormals, no overflow, nothing rounds.  Two forms, both held to the CPU table on every finite code
// in every byte position at the exponents -100, -17, -1, 0, 1, 17, 100 (tests/test_gpu_fp8.py):
//   1 (default)  v_cvt_scalef32_pk_bf16_fp8: one instruction per pair, the scale operand 2^k as fp32 multiplies the decoded value.  That test
//                decided that it may be used; 2 instructions per 4 codes.  fc1 at 16 rows 16.9 us per launch, a batch-8 step 1.367 ms.
//   0            v_cvt_pk_f32_fp8, an fp32 multiply by 2^k, the high 16 bits: 2 cvt + 4 mul + 2 pack per 4 codes.  fc1 20.2 us, step 1.474 ms
//                (the bf16 stream: 18.0 us, 1.436 ms) - the conversion arithmetic in front of the LDS writes was what made FP8 slower than bf16.
ZN_DEVINL u32x2 fp8x4_to_bf16(unsigned v, float scale) {
#if ZN_FP8_CVT_SCALEF32
  return u32x2{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, scale, false)),
               __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, scale, true))};
#else
  const zn_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, true);
  const unsigned a0 = __float_as_uint(a.x * scale), a1 = __float_as_uint(a.y * scale), b0 = __float_as_uint(b.x * scale), b1 = __float_as_uint(b.y * scale);
  return u32x2{(a0 >> 16) | (a1 & 0xffff0000u), (b0 >> 16) | (b1 & 0xffff0000u)};
#endif
}
// 8 codes -> 8 bf16 (one 16-byte LDS piece)
ZN_DEVINL u32x4 fp8x8_to_bf16(u32x2 v, float scale) {
  const u32x2 lo = fp8x4_to_bf16(v.x, scale), hi = fp8x4_to_bf16(v.y, scale);
  return u32x4{lo.x, lo.y, hi.x, hi.y};
}

// The scale exponent of a row from the bits of its largest bf16 magnitude: the smallest k with amax <= 448 * 2^k, clamped; a zero row: 0.
ZN_DEVINL int fp8_row_exponent(unsigned mag) {
  if (mag == 0) return 0;
  const int e = (int)(mag >> 7), f = (int)(mag & 0x7f);
  if (e == 0) return ZN_FP8_EXP_MIN;                                   // bf16 denormals lie below 448 * 2^-100
  const int k = e - 127 - 8 + (f > 96 ? 1 : 0);                        // amax = (1 + f / 128) 2^(e - 127); 448 = 1.75 * 2^8
  return k < ZN_FP8_EXP_MIN ? ZN_FP8_EXP_MIN : k > ZN_FP8_EXP_MAX ? ZN_FP8_EXP_MAX : k;
}
// One bf16 weight -> its code: round to nearest even on the E4M3 grid in integer arithmetic, saturating at 448 (0x7E).  v = |w| 2^-k is exact
// in fp32 unless it underflows, and whatever an underflow leaves is below 2^-10 and rounds to zero.
ZN_DEVINL unsigned fp8_encode(bf16_t w, float inv_scale) {
  const unsigned sign = (w >> 8) & 0x80u;
  const float v = bf2f(w & 0x7fff) * inv_scale;
  unsigned code;
  if (v < 0.015625f) code = (unsigned)__float2int_rn(v * 512.0f);     // subnormal range: steps of 2^-9; 8 = the smallest normal code
  else {
    const unsigned u = __float_as_uint(v);
    code = ((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3);    // a carry out of the mantissa moves into the exponent field
  }
  return sign | (code > 0x7eu ? 0x7eu : code);                         // beyond 464: saturate at 448 (never a NaN code)
}

// ---- the FP8 KV cache (kv_round_e4m3 of zonos_amd/quant.py): a K or V element's code at scale exponent 0.  Finite values and the infinities
// saturate at +-448; a NaN keeps its sign and becomes the NaN code.
ZN_DEVINL unsigned kv_fp8_encode(bf16_t w) {
  if ((w & 0x7fffu) > 0x7f80u) return ((w >> 8) & 0x80u) | 0x7fu;
  return fp8_encode(w, 1.0f);
}
// A packed bf16 pair as the KV appends hold it -> the pair rounded to the E4M3 grid (one v_cvt_scalef32_pk_bf16_fp8 at scale 1 decodes the two
// codes: the bits every FP8 reader of the cache widens them to) and its two codes (byte 0 = the low element).
ZN_DEVINL unsigned kv_fp8_round_pair(unsigned pr, unsigned& codes) {
  codes = kv_fp8_encode((bf16_t)(pr & 0xffffu)) | (kv_fp8_encode((bf16_t)(pr >> 16)) << 8);
  return fp8x4_to_bf16(codes, 1.0f).x;
}
// 2 / 4 / 8 codes -> as many bf16 at scale 1 (the widening of the FP8 decode attention's loaders, zn_attn_fp8_kernels.h)
ZN_DEVINL unsigned kv_fp8x2_to_bf16(unsigned v) { return fp8x4_to_bf16(v, 1.0f).x; }

// One workgroup (256 threads) per weight row: row amax, exponent, codes.  K a multiple of 8.  Load time, not the hot path.
__global__ __launch_bounds__(256) void fp8_quantize_rows_kernel(const bf16_t* __restrict__ W, int K, uint8_t* __restrict__ q, int8_t* __restrict__ exps) {
  __shared__ unsigned s_max[4];
  const size_t row = blockIdx.x;
  const bf16_t* w = W + row * K;
  unsigned m = 0;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    const u32x4 v = ld16(w + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned lo = v[j] & 0x7fffu, hi = (v[j] >> 16) & 0x7fffu;
      m = m > lo ? m : lo;
      m = m > hi ? m : hi;
    }
  }
  m = (unsigned)wave_max((float)m);                                  // (magnitudes are below 2^15: exact as floats)
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  m = s_max[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) m = m > s_max[j] ? m : s_max[j];
  const int k = fp8_row_exponent(m);
  if (threadIdx.x == 0) exps[row] = (int8_t)k;
  const float inv = fp8_row_scale(-k);
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    const u32x4 v = ld16(w + i);
    unsigned c[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[2 * j] = fp8_encode((bf16_t)(v[j] & 0xffffu), inv); c[2 * j + 1] = fp8_encode((bf16_t)(v[j] >> 16), inv); }
    *(u32x2*)(q + row * K + i) = u32x2{c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24)};
  }
}

// q [N][K], exps [N] -> bf16 [N][K]; one workgroup per row, K a multiple of 8.
__global__ __launch_bounds__(256) void fp8_dequant_rows_kernel(const uint8_t* __restrict__ q, const int8_t* __restrict__ exps, int K, bf16_t* __restrict__ W) {
  const size_t row = blockIdx.x;
  const float scale = fp8_row_scale(exps[row]);
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) *(u32x4*)(W + row * K + i) = fp8x8_to_bf16(*(const u32x2*)(q + row * K + i), scale);
}

// ZN_FP8_VERIFY: counts the 8-element pieces in which the bf16 copy differs from the dequantised stream.
__global__ __launch_bounds__(256) void fp8_compare_rows_kernel(const uint8_t* __restrict__ q, const int8_t* __restrict__ exps, int K, const bf16_t* __restrict__ W,
                                                                unsigned* __restrict__ mismatches) {
  const size_t row = blockIdx.x;
  const float scale = fp8_row_scale(exps[row]);
  unsigned bad = 0;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    const u32x4 d = fp8x8_to_bf16(*(const u32x2*)(q + row * K + i), scale), w = ld16(W + row * K + i);
    bad += (d.x != w.x) | (d.y != w.y) | (d.z != w.z) | (d.w != w.w);
  }
  if (bad) atomicAdd(mismatches, bad);
}

// The GEMV of a decode step of 1..4 rows reading its weights as an FP8 stream (zn_fp8_kernels.h; LinearEnv::w8v_offered, ZN_TUNE_FP8_SMALL_ROWS = 2):
// gemv_kernel<R, NCH, KSPLIT, PRO, EPI, FULL> (zn_decode_kernels.h) with ONE thing changed - where a unit's weight tile comes from.  A lane keeps the eight K
// positions per chunk it has there, (c * 64 + lane) * 8 .. + 8, and requests them as 8 code bytes of W8q (one 8-byte non-temporal load, ld_nt8) together with
// the scale exponents of the unit's two weight rows.  At use fp8x8_to_bf16 turns the codes into the u32x4 the bf16 form holds - a code times 2^k is exact in
// bf16 - and everything else is restated from gemv_kernel unchanged: the prologues, the issue order (activation and prologue loads, then the first units'
// weights, sched_barrier), the masking (FULL, u_ok, b_ok), dot8 over the chunks ascending, wave_sum, the KSPLIT = 4 combine in LDS in wave order, the epilogue
// operands requested with the unit, gemv_epilogue<EPI>.  An output element sees gemv_kernel's instruction sequence on gemv_kernel's operand bits: the results
// are bit-equal to the bf16 GEMV on the dequantised weights (tests/test_gpu_gemv_fp8.py).  Row B of a half pair and units past a.units are never requested.
// A unit's tile is half the bytes of the bf16 tile, so DEPTH = 2 keeps a ring of two units ahead of the one being reduced (the register count of one bf16
// tile); DEPTH = 1 is gemv_kernel's "next unit requested before this one is reduced".  Which unit a tile belongs to does not enter its arithmetic: both
// depths give the same bits.  Measured (profiles/smallrowsbench.txt): the ring is never faster - only fc1 has more than one unit per wave (four), and there
// one unit ahead runs 9.78 / 12.09 us at 2 / 4 rows against the ring's 10.43 / 13.30 (equal within 0.5 us at 1 and 3 rows); where a wave has one unit the ring
// only costs registers (the in_proj at 1 and 2 rows: 7.38 / 6.83 against 7.75 / 7.09 us).  ZN_TUNE_FP8_SMALL_ROWS = 2 therefore launches DEPTH = 1; the ring
// stays behind = 3 for the measurement.  New kernel names, not new template arguments of gemv_kernel: that keeps its instantiation list and its generated code.
#pragma once
#include "zn_decode_kernels.h"
#include "zn_fp8_kernels.h"

#ifdef ZN_GEMV_F64
#error "zn_gemv_fp8_kernels.h restates the fp32 GEMV only: the ZN_GEMV_F64 experiment has no FP8 form"
#endif

// Weight tile of one work unit (two weight rows) held in registers as codes.
template <int NCH> struct W8Tile {
  u32x2 a[NCH], b[NCH];
  int exA, exB;     // scale exponents of the two rows
  unsigned resid;   // EPI_RESID: this lane's (row = lane) residual pair; EPI_MAMBA: the two conv biases
  u32x4 cst, cw;    // EPI_MAMBA: conv window state and taps of the pair's two channels
};

template <int NCH, int KSPLIT, int EPI, bool FULL>
ZN_DEVINL void gemv8_load_unit(const GemvArgs& a, int u, int lane, int kw, int kbase, W8Tile<NCH>& t) {
  const int F = a.N >> 1;
  const bool u_ok = FULL || u < a.units;
  int rowA, rowB;
  if constexpr (EPI == EPI_SILU) { rowA = u; rowB = u + F; }
  else { rowA = 2 * u; rowB = 2 * u + 1; }
  const bool b_ok = FULL || (u_ok && rowB < a.N);
  if constexpr (FULL) { t.exA = a.W8exp[rowA]; t.exB = a.W8exp[rowB]; }          // ahead of the codes: requests return in order
  else {
    t.exA = 0; t.exB = 0;
    if (u_ok) t.exA = a.W8exp[rowA];
    if (b_ok) t.exB = a.W8exp[rowB];
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = (c * 64 + lane) * 8;
    if constexpr (FULL) {
      t.a[c] = ld_nt8(a.W8q + (size_t)rowA * a.K + kbase + k);
      t.b[c] = ld_nt8(a.W8q + (size_t)rowB * a.K + kbase + k);
    } else {
      t.a[c] = u32x2{0, 0}; t.b[c] = u32x2{0, 0};                                // code 0 = +0.0: the zero tile of the bf16 form
      if (u_ok && k < kw) {
        t.a[c] = ld_nt8(a.W8q + (size_t)rowA * a.K + kbase + k);
        if (b_ok) t.b[c] = ld_nt8(a.W8q + (size_t)rowB * a.K + kbase + k);
      }
    }
  }
  t.resid = 0;
  if constexpr (EPI == EPI_MAMBA) { t.cst = u32x4{0, 0, 0, 0}; t.cw = u32x4{0, 0, 0, 0}; }
  if (u_ok && lane < a.nrows) {
    if constexpr (EPI == EPI_MAMBA) mamba_epi_operands(a, lane, rowA, t.resid, t.cst, t.cw);
    if constexpr (EPI == EPI_RESID) {
      const size_t o = (size_t)lane * a.N + rowA;
      t.resid = b_ok ? *(const unsigned*)(a.resid + o) : (unsigned)a.resid[o];
    }
  }
}
template <int NCH, int EPI> ZN_DEVINL void gemv8_no_unit(W8Tile<NCH>& t) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) { t.a[c] = u32x2{0, 0}; t.b[c] = u32x2{0, 0}; }
  t.exA = 0; t.exB = 0; t.resid = 0;
  if constexpr (EPI == EPI_MAMBA) { t.cst = u32x4{0, 0, 0, 0}; t.cw = u32x4{0, 0, 0, 0}; }
}

// FULL as in gemv_kernel: K == NCH*512*KSPLIT, N even, every wave's units exist, nrows == R (host-checked).
template <int R, int NCH, int KSPLIT, int PRO, int EPI, bool FULL, int DEPTH>
__global__ __launch_bounds__(256) void gemv8_kernel(GemvArgs a) {
  static_assert(EPI == EPI_SILU || EPI == EPI_RESID || EPI == EPI_MAMBA || EPI == EPI_STORE, "gemv8: fc1, fc2 and the Mamba2 projections only (lin_has_w8v)");
  static_assert(DEPTH == 1 || DEPTH == 2, "gemv8: one or two units ahead");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int K = a.K;
  const int kw = K / KSPLIT;                      // k-range of this wave
  const int kbase = (KSPLIT == 1) ? 0 : wave * kw;
  __shared__ float red[4][2][R];
  const int u0 = (KSPLIT == 1) ? (blockIdx.x * 4 + wave) * a.upw : blockIdx.x * a.upw;

  // Issue order (vmcnt retires in order): the small L2-resident loads the prologue needs first, then the first units' weights, then pin that order.
  u32x4 xr[NCH][R];
  u32x4 lng[PRO != PRO_NONE ? NCH : 1], lnb[PRO == PRO_LN ? NCH : 1];
  u32x4 zr[PRO == PRO_GATED ? NCH : 1][R];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = (c * 64 + lane) * 8;
    const bool kv_ok = FULL || k < kw;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (PRO != PRO_GATED) {
        if constexpr (FULL) xr[c][r] = ld16(a.x + (size_t)r * K + kbase + k);
        else {
          xr[c][r] = u32x4{0, 0, 0, 0};
          if (kv_ok && r < a.nrows) xr[c][r] = ld16(a.x + (size_t)r * K + kbase + k);
        }
      }
      if constexpr (PRO == PRO_GATED) {                    // eight fp32 values: xr = first four, zr = last four
        if constexpr (FULL) { xr[c][r] = ld16(a.gv + (size_t)r * K + kbase + k); zr[c][r] = ld16(a.gv + (size_t)r * K + kbase + k + 4); }
        else {
          xr[c][r] = u32x4{0, 0, 0, 0}; zr[c][r] = u32x4{0, 0, 0, 0};
          if (kv_ok && r < a.nrows) { xr[c][r] = ld16(a.gv + (size_t)r * K + kbase + k); zr[c][r] = ld16(a.gv + (size_t)r * K + kbase + k + 4); }
        }
      }
    }
    if constexpr (PRO == PRO_LN) {
      lng[c] = u32x4{0, 0, 0, 0}; lnb[c] = u32x4{0, 0, 0, 0};
      if (kv_ok) { lng[c] = ld16(a.ln_w + k); lnb[c] = ld16(a.ln_b + k); }
    }
    if constexpr (PRO == PRO_GATED) {
      lng[c] = u32x4{0, 0, 0, 0};
      if (kv_ok) lng[c] = ld16(a.ln_w + kbase + k);
    }
  }
  // the ring: w0 = the unit reduced next, w1 = (DEPTH 2) the one after it
  W8Tile<NCH> w0, w1;
  gemv8_load_unit<NCH, KSPLIT, EPI, FULL>(a, u0, lane, kw, kbase, w0);
  if constexpr (DEPTH == 2) {
    if (a.upw > 1) gemv8_load_unit<NCH, KSPLIT, EPI, FULL>(a, u0 + 1, lane, kw, kbase, w1);
    else gemv8_no_unit<NCH, EPI>(w1);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (PRO == PRO_LN) {
    // nn.LayerNorm: fp32 statistics, biased variance, affine, bf16 out.  KSPLIT == 1.
    const float invK = 1.0f / (float)K;
    float s[R], ss[R], mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) s[r] += ln_sum8(xr[c][r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mean[r] = __fmul_rn(wave_sum(s[r]), invK);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ss[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (FULL || (c * 64 + lane) * 8 < kw) ss[r] = ln_sq8(xr[c][r], mean[r], ss[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rstd[r] = ln_rstd(wave_sum(ss[r]), invK, a.eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = (c * 64 + lane) * 8;
      if (FULL || k < kw) {
#pragma unroll
        for (int r = 0; r < R; ++r) xr[c][r] = ln_norm8(xr[c][r], mean[r], rstd[r], lng[c], lnb[c]);
      }
    }
  }

  if constexpr (PRO == PRO_GATED) {
    // mamba_ssm RMSNormGated(norm_before_gate=False), one group: v = y * silu(z) arrives in fp32; out = bf16(v * rstd * w) with rstd from the mean of v^2
    // over the row.  KSPLIT == 1: every wave holds whole rows; KSPLIT == 4: a quarter each, the four partial sums meet in LDS in wave order.
    const float invK = 1.0f / (float)K;
    float ss[R], rstd[R];
    __shared__ float red_pro[4][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ss[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const u32x4 va = xr[c][r], vb = zr[c][r];
        const float v[8] = {__uint_as_float(va.x), __uint_as_float(va.y), __uint_as_float(va.z), __uint_as_float(va.w),
                            __uint_as_float(vb.x), __uint_as_float(vb.y), __uint_as_float(vb.z), __uint_as_float(vb.w)};
#pragma unroll
        for (int e = 0; e < 8; ++e) ss[r] += v[e] * v[e];
      }
    }
    if constexpr (KSPLIT == 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) rstd[r] = 1.0f / sqrtf(wave_sum(ss[r]) * invK + a.eps);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) { const float t = wave_sum(ss[r]); if (lane == 0) red_pro[wave][r] = t; }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r) rstd[r] = 1.0f / sqrtf((((red_pro[0][r] + red_pro[1][r]) + red_pro[2][r]) + red_pro[3][r]) * invK + a.eps);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const u32x4 g = lng[c];
      const float wf[8] = {lo_f(g.x), hi_f(g.x), lo_f(g.y), hi_f(g.y), lo_f(g.z), hi_f(g.z), lo_f(g.w), hi_f(g.w)};
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u32x4 va = xr[c][r], vb = zr[c][r];
        const float q = rstd[r];
        u32x4 o;
        o.x = pack2(__fmul_rn(__fmul_rn(__uint_as_float(va.x), q), wf[0]), __fmul_rn(__fmul_rn(__uint_as_float(va.y), q), wf[1]));
        o.y = pack2(__fmul_rn(__fmul_rn(__uint_as_float(va.z), q), wf[2]), __fmul_rn(__fmul_rn(__uint_as_float(va.w), q), wf[3]));
        o.z = pack2(__fmul_rn(__fmul_rn(__uint_as_float(vb.x), q), wf[4]), __fmul_rn(__fmul_rn(__uint_as_float(vb.y), q), wf[5]));
        o.w = pack2(__fmul_rn(__fmul_rn(__uint_as_float(vb.z), q), wf[6]), __fmul_rn(__fmul_rn(__uint_as_float(vb.w), q), wf[7]));
        xr[c][r] = o;
      }
    }
  }

  // ---------------- main loop over work units (the unit DEPTH ahead is requested before this one is reduced)
  const int F = a.N >> 1;  // EPI_SILU: gate rows start at N/2
  for (int it = 0; it < a.upw; ++it) {
    const int u = u0 + it;
    const bool u_ok = FULL || u < a.units;  // wave-uniform (block-uniform for KSPLIT=4)
    int rowA, rowB;
    if constexpr (EPI == EPI_SILU) { rowA = u; rowB = u + F; }
    else { rowA = 2 * u; rowB = 2 * u + 1; }
    const bool b_ok = FULL || (u_ok && rowB < a.N);
    float accA[R], accB[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { accA[r] = 0.f; accB[r] = 0.f; }
    const W8Tile<NCH> cur = w0;
    if constexpr (DEPTH == 2) {
      w0 = w1;
      if (it + 2 < a.upw) gemv8_load_unit<NCH, KSPLIT, EPI, FULL>(a, u + 2, lane, kw, kbase, w1);
    } else {
      if (it + 1 < a.upw) gemv8_load_unit<NCH, KSPLIT, EPI, FULL>(a, u + 1, lane, kw, kbase, w0);
    }
    const float scA = fp8_row_scale(cur.exA), scB = fp8_row_scale(cur.exB);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const u32x4 wa = fp8x8_to_bf16(cur.a[c], scA), wb = fp8x8_to_bf16(cur.b[c], scB);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        accA[r] = dot8(wa, xr[c][r], accA[r]);
        accB[r] = dot8(wb, xr[c][r], accB[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { accA[r] = wave_sum(accA[r]); accB[r] = wave_sum(accB[r]); }
    if constexpr (KSPLIT > 1) {
      __syncthreads();
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) { red[wave][0][r] = accA[r]; red[wave][1][r] = accB[r]; }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        accA[r] = ((red[0][0][r] + red[1][0][r]) + red[2][0][r]) + red[3][0][r];
        accB[r] = ((red[0][1][r] + red[1][1][r]) + red[2][1][r]) + red[3][1][r];
      }
      if (wave != 0) continue;
    }
    if (!u_ok) continue;
    // ---------------- epilogue: lane r finishes row r
    float vA = 0.f, vB = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) if (lane == r) { vA = accA[r]; vB = accB[r]; }
    if (lane >= (FULL ? R : a.nrows)) continue;
    if constexpr (EPI == EPI_MAMBA) gemv_epilogue<EPI>(a, lane, rowA, rowB, b_ok, u, vA, vB, cur.resid, 1.f, 0.f, 0, cur.cst, cur.cw);
    else gemv_epilogue<EPI>(a, lane, rowA, rowB, b_ok, u, vA, vB, cur.resid, 1.f, 0.f, 0);
  }
}

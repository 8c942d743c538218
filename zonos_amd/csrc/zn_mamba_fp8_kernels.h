// The Mamba2 in_proj and out_proj reading their weights as an FP8 stream (zn_fp8_kernels.h; zn_set_mamba_fp8): gemm16k_kernel<EPI, NCH, PRO_NONE>
// (zn_decode_kernels.h) and gemm16k_rows_kernel<NCH> (zn_wide_kernels.h) with ONE thing changed - where a wave's K / 8 slice of the 16-row weight tile
// comes from.  It is requested as E4M3 codes (half the bytes, half the requests) with the scale exponents of the rows a lane holds, and converted with
// fp8x8_to_bf16 on the way into the wave's private Ws region.  A code times 2^k is exact in bf16, so Ws then holds what the bf16 kernel reading the
// dequantised weights puts there, and everything behind it is restated from that kernel unchanged: the B fragments read back from Ws, the chained
// v_mfma_f32_16x16x32_bf16 sequence (chunks and steps ascending from 0.f), Ct, the eight partials added in wave order, gemv_epilogue<EPI> with
// mamba_epi_operands, the next-tile prefetch of the loop.  The outputs are bit-equal to the bf16 kernels' on the dequantised weights (tests/test_gpu_mamba_fp8.py).
// New kernel names, not new template arguments of the bf16 kernels: those keep their instantiation lists and their generated code.
#pragma once
#include "zn_decode_kernels.h"
#include "zn_fp8_kernels.h"

// Request of a wave's slice.  One chunk of one weight row is 128 codes = 128 contiguous bytes = 8 lanes x 16 B, so a wave-wide load covers 8 rows of a
// chunk: load i of chunk c = rows 8i .. 8i+7 of the tile (bf16: four loads of 4 rows x 256 B).  The eight waves of the workgroup together read the tile's
// 16 K contiguous bytes.  Rows are clamped exactly as the bf16 kernel clamps them (never out of bounds; masked in the epilogue), the exponents with them.
template <int NCH>
ZN_DEVINL void g16k8_request(const GemvArgs& a, int tile, int kbeg, int lane, u32x4 (&wr)[NCH][2], int (&ex)[2]) {
  const int wsub = lane & 7, wq = lane >> 3;
  int row[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    row[i] = min(tile * 16 + 8 * i + wq, a.N - 1);
    ex[i] = a.W8exp[row[i]];                                         // ahead of the codes: requests return in order
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i) wr[c][i] = ld_nt16(a.W8q + (size_t)row[i] * a.K + kbeg + c * ZN_G16K_KCH + 16 * wsub);
}
// One chunk into the wave's Ws region [16][LDW] as bf16: a lane's 16 codes become two 16-byte pieces, k = 16 wsub .. + 7 and + 8 .. + 15 of its row.
// ds_write_b128 works in groups of 8 consecutive lanes over 32 banks: written in k order, lanes wsub and wsub + 4 of a row (128 bytes apart) would meet
// on the same banks, so the upper four lanes write their pieces in the other order - each write then covers the 32 banks once.
ZN_DEVINL void g16k8_stage(bf16_t* ws, int lane, const u32x4 (&wr)[2], const int (&ex)[2]) {
  constexpr int LDW = ZN_G16K_KCH + 8;
  const int wsub = lane & 7, wq = lane >> 3;
  const bool sw = wsub >= 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float sc = fp8_row_scale(ex[i]);
    const u32x4 lo = fp8x8_to_bf16(u32x2{wr[i].x, wr[i].y}, sc), hi = fp8x8_to_bf16(u32x2{wr[i].z, wr[i].w}, sc);
    bf16_t* d = ws + (8 * i + wq) * LDW + 16 * wsub;
    *(u32x4*)(d + (sw ? 8 : 0)) = sw ? hi : lo;
    *(u32x4*)(d + (sw ? 0 : 8)) = sw ? lo : hi;
  }
}

// ------------------------------------------------------------------------------------------------ 16 rows per workgroup (grid y: row groups of the wide plan)
// gemm16k_kernel<EPI, NCH, PRO_NONE> for EPI_MAMBA (in_proj, NCH = 2) and EPI_STORE (out_proj, NCH = 4): grid (ceil(N / 16), ceil(rows / 16)).
template <int EPI, int NCH>      // NCH = 128-wide chunks per wave: K = 8 * 128 * NCH
__global__ __launch_bounds__(ZN_G16K_NKW * 64) void gemm16k8_kernel(GemvArgs a) {
  static_assert(EPI == EPI_MAMBA || EPI == EPI_STORE, "gemm16k8: the Mamba2 projections only");
  constexpr int NKW = ZN_G16K_NKW, KCH = ZN_G16K_KCH, LDW = KCH + 8, KS = KCH * NCH;
  __shared__ __attribute__((aligned(16))) bf16_t Ws[NKW][16 * LDW];
  __shared__ float Ct[NKW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, K = a.K, kbeg = wave * KS;
  // gridDim.y > 1 (a decode step of 17..64 rows): workgroup (tile, y) serves activation rows 16 y .. 16 y + 15, as in gemm16k_kernel
  if (blockIdx.y) {
    const size_t r0 = (size_t)blockIdx.y * 16;
    a.x += r0 * K; a.nrows -= (int)r0;
    if (a.out) a.out += r0 * a.N;
    if constexpr (EPI == EPI_MAMBA) { a.conv_state += r0 * a.conv_dim * 4; a.xbc += r0 * a.conv_dim; }
  }
  if (a.nrows > 16) a.nrows = 16;
  // epilogue operands first (item = tid < 128: activation row m, weight-row pair pj): their round trips overlap the stream's
  const int em = tid & 15, epj = (tid >> 4) & 7;
  const int erowA = tile * 16 + 2 * epj, erowB = erowA + 1;
  const bool e_on = tid < 128 && em < a.nrows && erowA < a.N, eb_ok = erowB < a.N;
  unsigned resid = 0;
  u32x4 cst = u32x4{0, 0, 0, 0}, cw = u32x4{0, 0, 0, 0};
  if constexpr (EPI == EPI_MAMBA) { if (e_on) mamba_epi_operands(a, em, erowA, resid, cst, cw); }
  u32x4 wr[NCH][2], xr[NCH][KCH / 32];
  int ex[2];
  {
    const bf16_t* xp = a.x + (size_t)min(n, a.nrows - 1) * K + kbeg + 8 * g;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int st = 0; st < KCH / 32; ++st) xr[c][st] = ld16(xp + c * KCH + 32 * st);
  }
  g16k8_request<NCH>(a, tile, kbeg, lane, wr, ex);
  bf16_t* ws = &Ws[wave][0];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    g16k8_stage(ws, lane, wr[c], ex);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the region is private to the wave: its LDS ops complete in order
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int st = 0; st < KCH / 32; ++st) {
      const u32x4 bw = *(const u32x4*)(ws + n * LDW + 32 * st + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(zn_bf16x8, xr[c][st]), __builtin_bit_cast(zn_bf16x8, bw), acc, 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // D layout: col (weight row of the tile) = lane & 15, row (activation row) = 4*(lane>>4) + reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) Ct[wave][n][4 * g + reg] = acc[reg];
  __syncthreads();
  if (e_on) {
    float vA = 0.f, vB = 0.f;
#pragma unroll
    for (int w = 0; w < NKW; ++w) { vA += Ct[w][2 * epj][em]; vB += Ct[w][2 * epj + 1][em]; }
    gemv_epilogue<EPI>(a, em, erowA, erowB, eb_ok, erowA >> 1, vA, eb_ok ? vB : 0.f, resid, 1.f, 0.f, 0, cst, cw);
  }
}

// ------------------------------------------------------------------------------------------------ the in_proj over up to four row tiles per weight pass
// gemm16k_rows_kernel<NCH>: grid (ceil(N / 16), 1); the weight tile is requested once (as codes), kept as bf16 B fragments, and the row tiles are walked.
template <int NCH>
__global__ __launch_bounds__(ZN_G16K_NKW * 64) void gemm16k8_rows_kernel(GemvArgs a) {
  constexpr int NKW = ZN_G16K_NKW, KCH = ZN_G16K_KCH, LDW = KCH + 8, KS = KCH * NCH, MAXT = ZN_WIDE_ROWS / 16;
  __shared__ __attribute__((aligned(16))) bf16_t Ws[NKW][16 * LDW];
  __shared__ float Ct[NKW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, K = a.K, kbeg = wave * KS;
  const int rows = a.nrows < ZN_WIDE_ROWS ? a.nrows : ZN_WIDE_ROWS, ntiles = (rows + 15) / 16;
  // epilogue item (tid < 128): activation row 16 rt + em, weight-row pair epj of the tile
  const int em = tid & 15, epj = (tid >> 4) & 7;
  const int erowA = tile * 16 + 2 * epj, erowB = erowA + 1;
  const bool e_col = tid < 128 && erowA < a.N, eb_ok = erowB < a.N;
  // tile 0: epilogue operands first, then the activations - both ahead of the weight stream
  unsigned resid = 0;
  u32x4 cst = u32x4{0, 0, 0, 0}, cw = u32x4{0, 0, 0, 0};
  bool e_on = e_col && em < rows;
  if (e_on) mamba_epi_operands(a, em, erowA, resid, cst, cw);
  u32x4 wr[NCH][2], xr[NCH][KCH / 32], bw[NCH][KCH / 32];
  int ex[2];
  {
    const bf16_t* xp = a.x + (size_t)min(n, rows - 1) * K + kbeg + 8 * g;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int st = 0; st < KCH / 32; ++st) xr[c][st] = ld16(xp + c * KCH + 32 * st);
  }
  g16k8_request<NCH>(a, tile, kbeg, lane, wr, ex);
  bf16_t* ws = &Ws[wave][0];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    g16k8_stage(ws, lane, wr[c], ex);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the region is private to the wave: its LDS ops complete in order
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int st = 0; st < KCH / 32; ++st) bw[c][st] = *(const u32x4*)(ws + n * LDW + 32 * st + 8 * g);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int rt = 0; rt < MAXT; ++rt) {
    if (rt >= ntiles) break;                                         // uniform
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int st = 0; st < KCH / 32; ++st)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(zn_bf16x8, xr[c][st]), __builtin_bit_cast(zn_bf16x8, bw[c][st]), acc, 0, 0, 0);
    // the next tile's activations and epilogue operands
    const int r1 = 16 * (rt + 1);
    unsigned resid_n = 0;
    u32x4 cst_n = u32x4{0, 0, 0, 0}, cw_n = u32x4{0, 0, 0, 0};
    const bool e_on_n = e_col && r1 + em < rows;
    if (r1 < rows) {                                                 // uniform
      const bf16_t* xp = a.x + (size_t)min(r1 + n, rows - 1) * K + kbeg + 8 * g;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int st = 0; st < KCH / 32; ++st) xr[c][st] = ld16(xp + c * KCH + 32 * st);
      if (e_on_n) mamba_epi_operands(a, r1 + em, erowA, resid_n, cst_n, cw_n);
    }
    // D layout: col (weight row of the tile) = lane & 15, row (activation row) = 4*(lane>>4) + reg
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) Ct[wave][n][4 * g + reg] = acc[reg];
    __syncthreads();
    if (e_on) {
      float vA = 0.f, vB = 0.f;
#pragma unroll
      for (int w = 0; w < NKW; ++w) { vA += Ct[w][2 * epj][em]; vB += Ct[w][2 * epj + 1][em]; }
      gemv_epilogue<EPI_MAMBA>(a, 16 * rt + em, erowA, erowB, eb_ok, erowA >> 1, vA, eb_ok ? vB : 0.f, resid, 1.f, 0.f, 0, cst, cw);
    }
    __syncthreads();                                                 // Ct is rewritten by the next tile
    e_on = e_on_n; resid = resid_n; cst = cst_n; cw = cw_n;
  }
}

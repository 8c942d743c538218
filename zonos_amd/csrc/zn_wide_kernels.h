// Decode steps of 17..64 rows: the wide form of the LDS-staged streaming kernel (gemm16s_kernel, zn_decode_kernels.h) for fc1 and fc2, and the
// LayerNorm launch that goes with it.  gemm16s_kernel multiplies every staged weight chunk against ONE 16-row activation block, so a step of
// 32 rows streams each weight matrix twice (launch_linear's groups of 16); here a staged chunk meets RB = 2 .. 4 staged activation blocks, so
// 64 rows read it once.  Every output bit is the grouped path's: an output element is still the chain of v_mfma_f32_16x16x32_bf16 over its K slice
// in ascending 32-wide steps (the row block only selects which activation rows ride along), the slices of a split K meet through the same
// write-through partial tiles and arrival ticket and are added in slice order from 0.f, and the residual and SiLU-gate epilogues are
// gemv_epilogue's.  What the grouped plan chose that fixes a bit - ksplit, and the order of the tile statistics - arrives as arguments
// (GemvArgs::ksplit; LSEG below); the grid over the weight rows is this kernel's own: 64 weight rows (EPI_SILU: 32 value + their 32 gate rows)
// per workgroup of four waves, one 16-row weight tile per wave, as gemm64s_kernel (zn_prefill_kernels.h) does for short prompts.
// W8: the weight chunk arrives as E4M3 codes and is dequantised on the way into Ws with its row's power-of-two scale (fp8x8_to_bf16, exact), as
// in gemm16s_kernel<., NWV | ZN_G16S_W8>.
// LDS at RB = 4: Ws and Xs, 33.8 KB each (row stride KC + 8 elements: conflict-free 16-B fragment reads); the output tile [64][16 RB + 1] fp32
// reuses Ws after the K loop.
#pragma once
#include "zn_decode_kernels.h"

// fc1's LayerNorm at 17..64 rows when out_proj handed statistics over (LinearPlan::lnp): ONE launch normalises the rows of a group into nbuf
// from the per-tile {sum, centred second moment} (GemvArgs::ln_part_in) with the arithmetic of gemm16s_kernel<EPI_SILU, ., true>, instead of
// every one of gemm16w_kernel's workgroups repeating the normalisation of 64 rows.  gemm16s_kernel adds a row's ZN_G16_LNT tiles as LSEG = 4 NWV
// segments of ZN_G16_LNT / LSEG tiles, then the segments in order; 8 and 16 segments round the mean differently, so LSEG is the grouped plan's.
// K = 16 * ZN_G16_LNT.  One workgroup of 64 lanes per row.
template <int LSEG>
__global__ __launch_bounds__(64) void ln_from_stats_kernel(const bf16_t* x, const float* ln_part_in, const bf16_t* ln_w, const bf16_t* ln_b, bf16_t* out, float eps) {
  static_assert(LSEG == 8 || LSEG == 16, "ln_from_stats: the segment counts of gemm16s_kernel<., 2 / 4, true>");
  constexpr int K = 16 * ZN_G16_LNT, LTS = ZN_G16_LNT / LSEG;
  __shared__ float s_seg[LSEG];
  __shared__ float s_mr[2];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float2* lp = (const float2*)(ln_part_in + (size_t)row * ZN_G16_LNT * 2);
  float2 pt[LTS];
  if (tid < LSEG) {
#pragma unroll
    for (int t = 0; t < LTS; ++t) pt[t] = lp[tid * LTS + t];
    float ssum = 0.f;
#pragma unroll
    for (int t = 0; t < LTS; ++t) ssum += pt[t].x;
    s_seg[tid] = ssum;
  }
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int q = 0; q < LSEG; ++q) tot += s_seg[q];
  const float invK = 1.0f / (float)K, mean = tot * invK;
  __syncthreads();
  if (tid < LSEG) {
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < LTS; ++t) {
      const float dm = pt[t].x * 0.0625f - mean;
      sq += __fmaf_rn(dm, 16.0f * dm, pt[t].y);      // gemm16s_kernel's `pt.y + 16.0f * dm * dm` as the compiler contracts it there (16 dm is exact)
    }
    s_seg[tid] = sq;
  }
  __syncthreads();
  if (tid == 0) {
    float tq = 0.f;
#pragma unroll
    for (int q = 0; q < LSEG; ++q) tq += s_seg[q];
    s_mr[0] = mean;
    s_mr[1] = ln_rstd(tq, invK, eps);
  }
  __syncthreads();
  const float m = s_mr[0], r = s_mr[1];
#pragma unroll
  for (int i = 0; i < K / (64 * 8); ++i) {
    const int k = (i * 64 + tid) * 8;
    *(u32x4*)(out + (size_t)row * K + k) = ln_norm8(ld16(x + (size_t)row * K + k), m, r, ld16(ln_w + k), ld16(ln_b + k));
  }
}

template <int EPI, bool W8, int RB>
__global__ __launch_bounds__(256) void gemm16w_kernel(GemvArgs a) {
  static_assert(EPI == EPI_SILU || EPI == EPI_RESID, "gemm16w: fc1 (SiLU gate) and fc2 (residual)");
  static_assert(RB >= 2 && RB <= 4, "gemm16w: 2 .. 4 activation blocks of 16 rows");
  constexpr int KC = ZN_G16_KC, LDW = KC + 8, NT = 256, TN = 64, HALF = TN / 2, MR = 16 * RB;
  constexpr int XP = MR * 32 / NT;                      // activation pieces of 16 B per thread and chunk
  __shared__ __attribute__((aligned(16))) bf16_t Ws[TN * LDW];
  __shared__ __attribute__((aligned(16))) bf16_t Xs[MR * LDW];
  __shared__ int s_last;
  float (*Ct)[MR + 1] = (float (*)[MR + 1])Ws;          // the output tile reuses the weight staging area after the K loop
  static_assert(TN * (MR + 1) * sizeof(float) <= sizeof(Ws), "Ct fits the staging area");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int grp = blockIdx.x, ys = blockIdx.y;
  const int K = a.K, F = a.N >> 1;
  // LDS row j of this workgroup <-> weight row (clamped: never out of bounds; masked in the epilogue)
  auto wrow = [&](int j) -> int {
    if constexpr (EPI == EPI_SILU) {
      const int r = (j < HALF) ? grp * HALF + j : F + grp * HALF + (j - HALF);
      const int lim = (j < HALF) ? F : a.N;
      return r < lim ? r : lim - 1;
    } else {
      const int r = grp * TN + j;
      return r < a.N ? r : a.N - 1;
    }
  };
  const int kslice = K / a.ksplit, kbeg = ys * kslice, nchunks = kslice / KC;
  constexpr int NQ = W8 ? 4 : 8;                        // weight pieces of 16 B per thread and chunk: 64 rows x 16 (codes) or 32 (bf16)
  u32x4 wr[NQ], xr[XP];
  const uint8_t* wp[NQ];
  int wl[NQ];
  float wqs[W8 ? NQ : 1];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    if constexpr (W8) {
      const int idx = j * NT + tid, row = idx >> 4, c16 = idx & 15, gr = wrow(row);
      wp[j] = a.W8q + (size_t)gr * K + kbeg + c16 * 16;
      wl[j] = row * LDW + c16 * 16;
      wqs[j] = fp8_row_scale(a.W8exp[gr]);
    } else {
      const int idx = j * NT + tid, row = idx >> 5, c16 = idx & 31;
      wp[j] = (const uint8_t*)(a.W + (size_t)wrow(row) * K + kbeg + c16 * 8);
      wl[j] = row * LDW + c16 * 8;
    }
  }
  const bf16_t* xp[XP];
  int xl[XP];
#pragma unroll
  for (int j = 0; j < XP; ++j) {
    const int idx = j * NT + tid, row = idx >> 5, c16 = idx & 31;
    xp[j] = a.x + (size_t)(row < a.nrows ? row : a.nrows - 1) * K + kbeg + c16 * 8;
    xl[j] = row * LDW + c16 * 8;
  }
  constexpr int WSTEP = W8 ? KC : KC * 2;               // bytes of a weight row per chunk
#pragma unroll
  for (int j = 0; j < XP; ++j) xr[j] = ld16(xp[j]);
#pragma unroll
  for (int j = 0; j < NQ; ++j) wr[j] = ld_nt16(wp[j]);
  // the residual operands of this thread's epilogue items travel with the first chunk, as in gemm16s_kernel.  Item = it * NT + tid:
  // weight-row pair pj = item % HALF (neighbouring lanes store neighbouring columns), activation row m = item / HALF
  constexpr int NIT = HALF * MR / NT;
  unsigned resid_pre[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    resid_pre[it] = 0u;
    if constexpr (EPI == EPI_RESID) {
      const int item = it * NT + tid, m = item / HALF, pj = item % HALF, rowA = grp * TN + 2 * pj;
      if (m < a.nrows && rowA < a.N) {
        const size_t o = (size_t)m * a.N + rowA;
        resid_pre[it] = (rowA + 1 < a.N) ? *(const unsigned*)(a.resid + o) : (unsigned)a.resid[o];
      }
    }
  }
  f32x4 acc[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();                                    // the previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < XP; ++j) *(u32x4*)&Xs[xl[j]] = xr[j];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      if constexpr (W8) {
        *(u32x4*)&Ws[wl[j]] = fp8x8_to_bf16(u32x2{wr[j].x, wr[j].y}, wqs[j]);
        *(u32x4*)&Ws[wl[j] + 8] = fp8x8_to_bf16(u32x2{wr[j].z, wr[j].w}, wqs[j]);
      } else *(u32x4*)&Ws[wl[j]] = wr[j];
    }
    __syncthreads();
    if (c + 1 < nchunks) {
#pragma unroll
      for (int j = 0; j < XP; ++j) xr[j] = ld16(xp[j] + (size_t)(c + 1) * KC);
#pragma unroll
      for (int j = 0; j < NQ; ++j) wr[j] = ld_nt16(wp[j] + (size_t)(c + 1) * WSTEP);
    }
    const bf16_t* wf = &Ws[(wave * 16 + n) * LDW + 8 * g];
    const bf16_t* xf = &Xs[n * LDW + 8 * g];
#pragma unroll
    for (int st = 0; st < KC / 32; ++st) {
      const u32x4 bw = *(const u32x4*)(wf + 32 * st);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const u32x4 ax = *(const u32x4*)(xf + rb * 16 * LDW + 32 * st);
        acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(zn_bf16x8, ax), __builtin_bit_cast(zn_bf16x8, bw), acc[rb], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                      // every wave is done with Ws: it becomes Ct
  // D layout: col (LDS row wave*16 + n) = lane & 15, row (activation row of block rb) = 4*(lane>>4) + reg
  if (a.ksplit > 1) {
    // partial tiles [ksplit][MR][gridDim.x * TN] leave by write-through stores, the ticket follows once they are acknowledged; the last
    // workgroup to arrive reads every slice past L2 and adds them in slice order
    const size_t ld = (size_t)gridDim.x * TN;
    float* pp = a.part + ((size_t)ys * MR) * ld + (size_t)grp * TN + wave * 16 + n;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) st_wt(pp + (size_t)(rb * 16 + 4 * g + reg) * ld, acc[rb][reg]);
    __builtin_amdgcn_s_waitcnt(0);                      // vmcnt(0): stores acknowledged
    __syncthreads();
    if (tid == 0) {
      const int t = __hip_atomic_fetch_add(a.tickets + grp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (t == a.ksplit - 1);
      if (s_last) __hip_atomic_store(a.tickets + grp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    __syncthreads();
    if (!s_last) return;
    // MR * TN / NT = 4 RB tile elements per thread, four at a time with every slice of the four requested before the first add; the sum runs
    // from 0.f over 16 slices in order (absent ones as 0.f), as in gemm16s_kernel
    for (int i0 = 0; i0 < MR * TN / NT; i0 += 4) {
      float v[4][16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int item = (i0 + i) * NT + tid, m = item / TN, col = item % TN;
        const float* q = a.part + (size_t)m * ld + (size_t)grp * TN + col;
#pragma unroll
        for (int y = 0; y < 16; ++y) v[i][y] = (y < a.ksplit) ? ld_wt(q + (size_t)y * MR * ld) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int item = (i0 + i) * NT + tid, m = item / TN, col = item % TN;
        float sum = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) sum += v[i][y];
        Ct[col][m] = sum;
      }
    }
  } else {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) Ct[wave * 16 + n][rb * 16 + 4 * g + reg] = acc[rb][reg];
  }
  __syncthreads();
  // ---- epilogue: TN/2 row pairs x MR activation rows, 2 RB items per thread
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int item = it * NT + tid, m = item / HALF, pj = item % HALF;
    if (m >= a.nrows) continue;
    if constexpr (EPI == EPI_SILU) {
      const int u = grp * HALF + pj;
      if (u >= F) continue;
      gemv_epilogue<EPI>(a, m, u, F + u, true, u, Ct[pj][m], Ct[HALF + pj][m], 0u, 1.f, 0.f, 0);
    } else {
      const int rowA = grp * TN + 2 * pj, rowB = rowA + 1;
      if (rowA >= a.N) continue;
      const bool b_ok = rowB < a.N;
      gemv_epilogue<EPI>(a, m, rowA, rowB, b_ok, rowA >> 1, Ct[2 * pj][m], b_ok ? Ct[2 * pj + 1][m] : 0.f, resid_pre[it], 1.f, 0.f, 0);
    }
  }
}

// ------------------------------------------------------------------------------------------------ the Mamba2 in_proj over up to four row tiles per weight pass
// gemm16k_kernel<EPI_MAMBA, NCH, PRO_NONE> (zn_decode_kernels.h) over 17..64 rows without the re-read per 16 rows: grid (ceil(N / 16), 1).  The workgroup
// requests its 16-row weight tile ONCE - each wave its K / 8 slice, through its Ws into B fragments, exactly as gemm16k_kernel does - keeps the B
// fragments in registers (NCH * 16 VGPRs) and walks the ceil(min(rows, 64) / 16) activation tiles.  Per tile: the A fragments of rows 16 rt .., the tile's
// epilogue operands (window state, taps, bias), the same chained v_mfma_f32_16x16x32_bf16 sequence per wave (chunks and steps ascending from 0.f), Ct,
// barrier, the eight partial tiles added in wave order from 0.f, gemv_epilogue<EPI_MAMBA>, and a barrier before Ct is reused.  An output element
// therefore sees the instruction sequence the 16-row launch gives it.  The NEXT tile's activations and epilogue operands are requested before the
// current tile's partials meet, so their round trip hides behind the barrier and the epilogue (the tiles' window rows are disjoint: no hazard).
template <int NCH>      // NCH = 128-wide chunks per wave: K = 8 * 128 * NCH
__global__ __launch_bounds__(ZN_G16K_NKW * 64) void gemm16k_rows_kernel(GemvArgs a) {
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
  // tile 0: epilogue operands first, then the activations - both ahead of the weight stream, as in gemm16k_kernel
  unsigned resid = 0;
  u32x4 cst = u32x4{0, 0, 0, 0}, cw = u32x4{0, 0, 0, 0};
  bool e_on = e_col && em < rows;
  if (e_on) mamba_epi_operands(a, em, erowA, resid, cst, cw);
  u32x4 wr[NCH][4], xr[NCH][KCH / 32], bw[NCH][KCH / 32];
  {
    const bf16_t* xp = a.x + (size_t)min(n, rows - 1) * K + kbeg + 8 * g;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int st = 0; st < KCH / 32; ++st) xr[c][st] = ld16(xp + c * KCH + 32 * st);
  }
  // weights: load i of chunk c = rows 4i .. 4i+3 of the tile, 16 lanes x 16 B = 256 contiguous bytes of one row each
  const int wsub = lane & 15, wq = lane >> 4;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(tile * 16 + 4 * i + wq, a.N - 1);        // clamped: never out of bounds; masked in the epilogue
      wr[c][i] = ld_nt16(a.W + (size_t)row * K + kbeg + c * KCH + 8 * wsub);
    }
  bf16_t* ws = &Ws[wave][0];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4*)(ws + (4 * i + wq) * LDW + 8 * wsub) = wr[c][i];
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

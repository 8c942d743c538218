// Output resampling (include/zonos_hip.h "output resampling"): one output sample per lane.
//
// Output j = q * n + p of a row is the fp32 chain  acc = fma(k[p][i], x[q * o - width + i], acc)  over the phase's support, ascending,
// with x = 0 outside the signal.  The taps lie [tap][phase] over the supports only (taps[t * n + p] = k[p][lo_p + t]), so consecutive
// lanes - consecutive outputs, consecutive phases - read consecutive words; the inputs of neighbouring lanes overlap almost entirely
// and come from the cache.  The value depends on j and the signal alone: a row may hold any window of its signal that covers what its
// outputs read (the host checks that before the launch), and the per-row integers travel by value in the kernel arguments.
// Every load is range-checked against the row's in_len, every store against its out_count.  No atomics, no cross-workgroup waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RS_MAX_ROWS 64
#define RS_THREADS 256

struct RsRow { long long out0, in0; int in_len, out_count; };
struct RsRows { RsRow r[RS_MAX_ROWS]; };

template <bool I16>
__global__ __launch_bounds__(RS_THREADS) void resample_rows_kernel(const float* __restrict__ in, long long in_max, void* __restrict__ out,
                                                                   long long out_max, const float* __restrict__ taps,
                                                                   const int* __restrict__ lo, const int* __restrict__ len, int o, int n,
                                                                   int width, RsRows g) {
  const RsRow r = g.r[blockIdx.y];
  const long long jl = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (jl >= r.out_count) return;
  const long long j = r.out0 + jl, q = j / n;
  const int p = (int)(j - q * n);
  const long long first = q * o - width + lo[p] - r.in0;          // the support's first input, as an index into the row's window
  const int m = len[p];
  const float* x = in + (long long)blockIdx.y * in_max;
  float acc = 0.f;
  for (int t = 0; t < m; ++t) {
    const long long i = first + t;
    const float v = (i >= 0 && i < r.in_len) ? x[i] : 0.f;
    acc = fmaf(taps[(long long)t * n + p], v, acc);
  }
  const long long at = (long long)blockIdx.y * out_max + jl;
  if (I16) {
    const float s = fminf(fmaxf(acc * 32767.0f, -32767.0f), 32767.0f);
    ((short*)out)[at] = (short)(int)s;
  } else {
    ((float*)out)[at] = acc;
  }
}

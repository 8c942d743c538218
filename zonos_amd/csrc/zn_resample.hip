// Output resampling: the plan (host, double), the stream arithmetic (host) and the rows launch.  include/zonos_hip.h "output resampling";
// zonos_amd/resample.py is the specification and tests/test_resample_cpu.py holds this file's host side to it.
#include "../../include/zonos_hip.h"
#include "zn_resample_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

static thread_local std::string g_rs_err;

struct RsPlan {
  int o = 1, n = 1, width = 0, taps = 1;       // taps = 2 * width + o: entries per phase of the full table
  std::vector<float> k;                         // [n][taps]
  std::vector<int> lo, hi;                      // [n]: the support [lo_p, hi_p) of phase p
  int mmax = 1, hi_max = 1;                     // longest support; largest hi_p
};

struct zn_resampler_s {
  std::shared_ptr<const RsPlan> plan;
  float* taps_dev = nullptr;                    // [mmax][n]
  int *lo_dev = nullptr, *len_dev = nullptr;    // [n]
  std::string err;
};

#define RFAIL(r, code, ...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); if (r) (r)->err = _b; else g_rs_err = _b; return (code); } while (0)
#define RHIP(r, call) do { hipError_t _e = (call); if (_e != hipSuccess) RFAIL(r, ZN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); } while (0)

static void rs_supports(RsPlan& P) {
  P.lo.assign(P.n, 0); P.hi.assign(P.n, 0);
  P.mmax = 1; P.hi_max = 0;
  for (int p = 0; p < P.n; ++p) {
    int lo = P.taps, hi = 0;
    for (int i = 0; i < P.taps; ++i)
      if (P.k[(size_t)p * P.taps + i] != 0.0f) { lo = std::min(lo, i); hi = i + 1; }
    if (hi == 0) lo = 0;                        // (a phase of zeros: an empty support)
    P.lo[p] = lo; P.hi[p] = hi;
    P.mmax = std::max(P.mmax, hi - lo); P.hi_max = std::max(P.hi_max, hi);
  }
}

// torchaudio's sinc_interp_hann kernel (functional.py _get_sinc_resample_kernel), every operation in double in its published order
static int rs_build(int orig, int nw, int lfw, double rolloff, RsPlan& P) {
  if (orig < 1 || nw < 1) RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "resample: rates must be >= 1, got %d -> %d", orig, nw);
  if (lfw < 1 || !(rolloff > 0.0) || rolloff > 1.0)
    RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "resample: lowpass_filter_width %d must be >= 1 and rolloff %g lie in (0, 1]", lfw, rolloff);
  int a = orig, b = nw;
  while (b) { const int t = a % b; a = b; b = t; }
  P.o = orig / a; P.n = nw / a;
  const double base = std::min(P.o, P.n) * rolloff;
  const double w = std::ceil((double)lfw * P.o / base);
  if (w > (double)(1 << 22) || ((double)2 * w + P.o) * P.n > (double)(1 << 22))
    RFAIL((zn_resampler) nullptr, ZN_ERR_UNSUPPORTED, "resample: %d -> %d needs a filter table of more than 2^22 entries", orig, nw);
  P.width = (int)w; P.taps = 2 * P.width + P.o;
  P.k.resize((size_t)P.n * P.taps);
  const double pi = 3.14159265358979323846;
  for (int p = 0; p < P.n; ++p)
    for (int i = 0; i < P.taps; ++i) {
      double t = ((double)(-p) / P.n + (double)(i - P.width) / P.o) * base;
      t = std::min(std::max(t, -(double)lfw), (double)lfw);
      const double c = std::cos(t * pi / lfw / 2), window = c * c;
      t = t * pi;
      P.k[(size_t)p * P.taps + i] = (float)((t == 0.0 ? 1.0 : std::sin(t) / t) * window * (base / P.o));
    }
  rs_supports(P);
  return ZN_OK;
}

// plans by their arguments: a stream asks for the same one at every chunk
static int rs_plan(int orig, int nw, int lfw, double rolloff, std::shared_ptr<const RsPlan>& out) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, double>, std::shared_ptr<const RsPlan>> cache;
  const auto key = std::make_tuple(orig, nw, lfw, rolloff);
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(key);
  if (it == cache.end()) {
    auto P = std::make_shared<RsPlan>();
    const int rc = rs_build(orig, nw, lfw, rolloff, *P);
    if (rc != ZN_OK) return rc;
    if (cache.size() >= 32) cache.clear();
    it = cache.emplace(key, std::move(P)).first;
  }
  out = it->second;
  return ZN_OK;
}

static inline int64_t rs_floordiv(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
static inline int64_t rs_total(const RsPlan& P, int64_t T) { return (P.n * T + P.o - 1) / P.o; }     // ceil(n T / o)

extern "C" const char* zn_resampler_last_error(zn_resampler r) { return r ? r->err.c_str() : g_rs_err.c_str(); }

extern "C" int zn_resample_plan(int32_t orig, int32_t nw, int32_t lfw, double rolloff, int32_t* o, int32_t* n, int32_t* width, int32_t* lo,
                                int32_t* hi, int32_t phases_cap, float* table, int64_t table_cap) {
  std::shared_ptr<const RsPlan> P;
  const int rc = rs_plan(orig, nw, lfw, rolloff, P);
  if (rc != ZN_OK) return rc;
  if (o) *o = P->o;
  if (n) *n = P->n;
  if (width) *width = P->width;
  if ((lo || hi) && phases_cap < P->n) RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "zn_resample_plan: %d phases, the buffers hold %d", P->n, phases_cap);
  if (table && table_cap < (int64_t)P->k.size())
    RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "zn_resample_plan: a table of %lld entries, the buffer holds %lld", (long long)P->k.size(), (long long)table_cap);
  if (lo) std::copy(P->lo.begin(), P->lo.end(), lo);
  if (hi) std::copy(P->hi.begin(), P->hi.end(), hi);
  if (table) std::copy(P->k.begin(), P->k.end(), table);
  return ZN_OK;
}

// leading final outputs with `avail` inputs known and no end in sight: every phase of the frames q < qf is final (qf from the largest
// hi_p), then the leading phases of frame qf that are final too
static int64_t rs_final(const RsPlan& P, int64_t avail) {
  const int64_t qf = std::max<int64_t>(0, rs_floordiv(avail + P.width - P.hi_max, P.o) + 1);
  int64_t c = qf * P.n;
  for (int p = 0; p < P.n && qf * P.o - P.width + P.hi[p] <= avail; ++p) ++c;
  return c;
}
// the first input that the outputs from j on read: the minimum over one period of phases (later frames read later inputs)
static int64_t rs_first_in(const RsPlan& P, int64_t j) {
  int64_t best = INT64_MAX;
  for (int64_t jj = j; jj < j + P.n; ++jj) {
    const int64_t q = jj / P.n; const int p = (int)(jj % P.n);
    best = std::min(best, q * P.o - P.width + P.lo[p]);
  }
  return std::max<int64_t>(best, 0);
}

extern "C" int zn_resample_span(int32_t orig, int32_t nw, int32_t lfw, double rolloff, int64_t avail, int32_t at_end, int64_t out_index,
                                int64_t* n_final, int64_t* first_in) {
  std::shared_ptr<const RsPlan> P;
  const int rc = rs_plan(orig, nw, lfw, rolloff, P);
  if (rc != ZN_OK) return rc;
  if (avail < 0 || avail > ((int64_t)1 << 40)) RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "zn_resample_span: avail = %lld out of range", (long long)avail);
  const int64_t fin = at_end ? rs_total(*P, avail) : rs_final(*P, avail);
  if (n_final) *n_final = fin;
  if (first_in) *first_in = rs_first_in(*P, out_index < 0 ? fin : out_index);
  return ZN_OK;
}

extern "C" int zn_resampler_destroy(zn_resampler r) {
  if (!r) return ZN_OK;
  if (r->taps_dev) (void)hipFree(r->taps_dev);
  if (r->lo_dev) (void)hipFree(r->lo_dev);
  if (r->len_dev) (void)hipFree(r->len_dev);
  delete r;
  return ZN_OK;
}

extern "C" int zn_resampler_create(int32_t orig, int32_t nw, int32_t lfw, double rolloff, zn_resampler* out) {
  if (!out) RFAIL((zn_resampler) nullptr, ZN_ERR_ARG, "zn_resampler_create: out is NULL");
  *out = nullptr;
  std::shared_ptr<const RsPlan> P;
  if (orig >= 1 && orig == nw) {                       // the identity: y[j] = fma(1, x[j], 0)
    auto I = std::make_shared<RsPlan>();
    I->k.assign(1, 1.0f);
    rs_supports(*I);
    P = I;
  } else {
    const int rc = rs_plan(orig, nw, lfw, rolloff, P);
    if (rc != ZN_OK) return rc;
  }
  zn_resampler r = new zn_resampler_s();
  r->plan = P;
  *out = r;
  return ZN_OK;
}

// The table goes to the device current at the handle's first launch (creating a handle touches no device).
static int rs_upload(zn_resampler r) {
  if (r->taps_dev) return ZN_OK;
  const RsPlan& P = *r->plan;
  const int n = P.n, mmax = P.mmax;
  std::vector<float> taps((size_t)mmax * n, 0.0f);
  std::vector<int> len(n);
  for (int p = 0; p < n; ++p) {
    len[p] = P.hi[p] - P.lo[p];
    for (int t = 0; t < len[p]; ++t) taps[(size_t)t * n + p] = P.k[(size_t)p * P.taps + P.lo[p] + t];
  }
  float* td = nullptr; int *ld = nullptr, *nd = nullptr;
  auto drop = [&]() { if (td) (void)hipFree(td); if (ld) (void)hipFree(ld); if (nd) (void)hipFree(nd); };
#define RS_TRY(call) do { hipError_t _e = (call); if (_e != hipSuccess) { drop(); RFAIL(r, ZN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); } } while (0)
  RS_TRY(hipMalloc(&td, taps.size() * sizeof(float)));
  RS_TRY(hipMalloc(&ld, n * sizeof(int)));
  RS_TRY(hipMalloc(&nd, n * sizeof(int)));
  RS_TRY(hipMemcpy(td, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  RS_TRY(hipMemcpy(ld, P.lo.data(), n * sizeof(int), hipMemcpyHostToDevice));
  RS_TRY(hipMemcpy(nd, len.data(), n * sizeof(int), hipMemcpyHostToDevice));
#undef RS_TRY
  r->taps_dev = td; r->lo_dev = ld; r->len_dev = nd;
  return ZN_OK;
}

// The host side of zn_resample_rows: every row checked, the kernel's per-row integers filled.  No device is touched.  *max_count
// receives the largest out_count.
static int rs_check_rows(zn_resampler r, const RsPlan& P, int64_t in_max, const zn_resample_row* rh, int32_t rows, int64_t out_max, RsRows& g,
                         int64_t* max_count) {
  if (rows < 1 || rows > RS_MAX_ROWS) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: %d rows, one call holds 1..%d", rows, RS_MAX_ROWS);
  if (!rh || in_max < 0 || out_max < 0) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: bad argument");
  *max_count = 0;
  for (int i = 0; i < rows; ++i) {
    const zn_resample_row& w = rh[i];
    if (w.in0 < 0 || w.in_len < 0 || w.out0 < 0 || w.out_count < 0 || w.in0 > ((int64_t)1 << 40) || w.out0 > ((int64_t)1 << 40))
      RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: a negative or oversized field", i);
    if (w.in_len > in_max) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: %d input samples, the rows hold in_max = %lld", i, w.in_len, (long long)in_max);
    if (w.out_count > out_max) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: %d outputs, the rows hold out_max = %lld", i, w.out_count, (long long)out_max);
    const int64_t in1 = w.in0 + w.in_len, out1 = w.out0 + w.out_count;
    if (w.at_end && out1 > rs_total(P, in1))
      RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: outputs up to %lld, a signal of %lld samples has %lld", i, (long long)out1, (long long)in1,
            (long long)rs_total(P, in1));
    // a phase's reads move on by o per frame: the first period of outputs holds the earliest read, the last period the latest
    const int64_t per = std::min<int64_t>(w.out_count, P.n);
    for (int64_t j = w.out0; j < w.out0 + per; ++j) {
      const int64_t q = j / P.n; const int p = (int)(j % P.n);
      const int64_t a = q * P.o - P.width + P.lo[p], b = q * P.o - P.width + P.hi[p];
      if (b > 0 && b > a && std::max<int64_t>(a, 0) < w.in0)
        RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: output %lld reads input %lld, the row's window starts at %lld", i, (long long)j,
              (long long)std::max<int64_t>(a, 0), (long long)w.in0);
    }
    for (int64_t j = out1 - per; j < out1; ++j) {
      const int64_t q = j / P.n; const int p = (int)(j % P.n);
      const int64_t a = q * P.o - P.width + P.lo[p], b = q * P.o - P.width + P.hi[p];
      if (b > a && b > in1 && !w.at_end)
        RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: row %d: output %lld reads input %lld, the row's window ends at %lld (not its signal's end)", i,
              (long long)j, (long long)(b - 1), (long long)in1);
    }
    g.r[i].out0 = w.out0; g.r[i].in0 = w.in0; g.r[i].in_len = w.in_len; g.r[i].out_count = w.out_count;
    *max_count = std::max<int64_t>(*max_count, w.out_count);
  }
  return ZN_OK;
}

extern "C" int zn_resample_rows(zn_resampler r, const float* in, int64_t in_max, const zn_resample_row* rh, int32_t rows, void* out,
                                int64_t out_max, int32_t out_is_int16, zn_stream stream) {
  if (!r) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: no handle");
  const RsPlan& P = *r->plan;
  RsRows g{};
  int64_t max_count = 0;
  const int rc = rs_check_rows(r, P, in_max, rh, rows, out_max, g, &max_count);
  if (rc != ZN_OK) return rc;
  if (max_count == 0) return ZN_OK;
  if (!in || !out) RFAIL(r, ZN_ERR_ARG, "zn_resample_rows: bad argument");
  const int up = rs_upload(r);
  if (up != ZN_OK) return up;
  const dim3 grid((unsigned)((max_count + RS_THREADS - 1) / RS_THREADS), (unsigned)rows);
  hipStream_t s = (hipStream_t)stream;
  if (out_is_int16)
    hipLaunchKernelGGL(resample_rows_kernel<true>, grid, dim3(RS_THREADS), 0, s, in, (long long)in_max, out, (long long)out_max, r->taps_dev,
                       r->lo_dev, r->len_dev, P.o, P.n, P.width, g);
  else
    hipLaunchKernelGGL(resample_rows_kernel<false>, grid, dim3(RS_THREADS), 0, s, in, (long long)in_max, out, (long long)out_max, r->taps_dev,
                       r->lo_dev, r->len_dev, P.o, P.n, P.width, g);
  RHIP(r, hipGetLastError());
  return ZN_OK;
}

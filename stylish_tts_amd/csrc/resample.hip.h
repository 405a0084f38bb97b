// Windowed-sinc sample-rate conversion: torchaudio.transforms.Resample / functional.resample from its published definition, with the float64 result
// as the target (torchaudio's own fp32 roundings of the coefficients and of the phase offset p / n are NOT mirrored).
//   o, n   = orig_freq, new_freq divided by their gcd;  base = min(o, n) * rolloff;  width = ceil(lpw * o / base);  taps = 2 width + o
//   t      = clamp((-p / n + j / o) * base, -lpw, lpw)            phase p in [0, n), tap j in [-width, width + o)
//   coef   = sinc(pi t) * window(t) * base / o                     Hann: cos(pi t / (2 lpw))^2;  Kaiser: I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)
//   out[q n + p] = sum_j coef[p][j] * x[q o + j]                   samples outside the utterance are zero;  ceil(n len / o) outputs
// Two kernels.  resample_table_kernel builds the coefficients on the device in fp64, unrounded, TAP-major ([taps][n]: the threads of a block hold
// consecutive phases and read consecutive doubles).  resample_kernel gives every thread R outputs of one phase at consecutive input steps q, which
// share every coefficient: the input span of the block is staged in LDS a chunk of taps at a time, products and the sums are fp64, each output's
// taps are added in tap order and its sum is rounded once, to fp32.  An output's arithmetic does not depend on the block it falls in or on the batch
// around its utterance.  Built without packed-fp32 instructions.
#pragma once
#include <cmath>
#include <tuple>
#include <vector>

#include "model.hip.h"

namespace stts {

constexpr int kResampleThreads = 256;
constexpr int kResampleChunk = 512;   // taps per staging pass
constexpr int kResampleStage = 4096;  // fp32 samples of LDS per block
constexpr int kResampleR = 4;         // outputs per thread (DESIGN.md 5m records 1 and 2 beside it)
constexpr int kResampleMaxFreq = 1024;
constexpr long kResampleMaxTable = 1L << 20;
constexpr int kResampleMaxLpw = 256;

enum { RESAMPLE_HANN = 0, RESAMPLE_KAISER = 1 };

// I0 by its power series sum_k (x^2 / 4)^k / (k!)^2: every term positive, so no cancellation; x <= 512 (the entry point checks) ends within 800 terms
__device__ __forceinline__ double resample_i0(double x) {
  const double h = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= h / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

// tab[j * n + p], j in [0, taps) standing for tap j - width.  The offset (-p / n + j / o) is formed as one exact integer over n o.
__global__ void __launch_bounds__(256) STTS_NO_PK resample_table_kernel(double* __restrict__ tab, int o, int n, int width, int taps, int lpw, double rolloff,
                                                                        int method, double beta) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)taps * n) return;
  const int j = (int)(e / n), p = (int)(e % n);
  const double base = (double)(o < n ? o : n) * rolloff;
  const long num = (long)(j - width) * n - (long)p * o;
  double t = (double)num / ((double)n * (double)o) * base;
  t = fmin(fmax(t, -(double)lpw), (double)lpw);
  double win;
  if (method == RESAMPLE_HANN) {
    const double c = cos(t * M_PI / (double)lpw / 2.0);
    win = c * c;
  } else {
    const double r = t / (double)lpw;
    win = resample_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / resample_i0(beta);
  }
  const double a = t * M_PI;
  const double s = a == 0.0 ? 1.0 : sin(a) / a;
  tab[e] = s * win * (base / (double)o);
}

// Grid (q blocks x phase chunks, n_utt), kResampleThreads threads.  A block takes G R consecutive input steps q and a chunk of P <= 256 phases
// (resample_plan): thread (g, p) computes outputs (q_lo + g R + r) n + p, r < R, one coefficient load for R products.  Utterance u: samples
// [off_in[u], off_in[u + 1]) of x, outputs [off_out[u], off_out[u + 1]) of y.
template <int R>
__global__ void __launch_bounds__(kResampleThreads) STTS_NO_PK resample_kernel(const float* __restrict__ x, const int* __restrict__ off_in,
                                                                               const int* __restrict__ off_out, const double* __restrict__ tab, int o, int n,
                                                                               int width, int taps, int P, int G, float* __restrict__ y) {
  __shared__ float stage[kResampleStage];
  const int u = blockIdx.y;
  const long L = (long)off_in[u + 1] - off_in[u], M = (long)off_out[u + 1] - off_out[u];
  const int pchunks = (n + P - 1) / P;
  const long q_lo = (long)(blockIdx.x / pchunks) * (G * R);
  const int p0 = (int)(blockIdx.x % pchunks) * P;
  if (q_lo * n + p0 >= M) return;  // the whole block leaves
  const int g = threadIdx.x / P, p = p0 + (int)threadIdx.x % P;
  const bool live = g < G && p < n;
  const int span = (G * R - 1) * o;  // + a chunk of taps staged per pass: at most kResampleStage (resample_plan)
  const float* xu = x + off_in[u];
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  for (int c0 = 0; c0 < taps; c0 += kResampleChunk) {
    const int nc = taps - c0 < kResampleChunk ? taps - c0 : kResampleChunk;
    const long s0 = q_lo * o - width + c0;
    if (c0) __syncthreads();
    for (int k = threadIdx.x; k < span + nc; k += kResampleThreads) {
      const long m = s0 + k;
      stage[k] = (m >= 0 && m < L) ? xu[m] : 0.f;
    }
    __syncthreads();
    if (live) {
      const double* tp = tab + (long)c0 * n + p;
      const float* sp = stage + g * R * o;
      for (int j = 0; j < nc; ++j) {
        const double c = tp[(long)j * n];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma(c, (double)sp[r * o + j], acc[r]);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long i = (q_lo + g * R + r) * n + p;
      if (i < M) y[off_out[u] + i] = (float)acc[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct ResampleGeom {
  int o = 0, n = 0, width = 0, taps = 0;
};

inline long resample_gcd(long a, long b) {
  while (b) {
    const long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the interface conditions, every refusal with its numbers; *g is filled when they hold
inline int resample_geometry(int orig, int fresh, int lpw, double rolloff, ResampleGeom* g) {
  STTS_CHECK(orig >= 1 && fresh >= 1, "resample: orig_freq %d / new_freq %d must be positive", orig, fresh);
  STTS_CHECK(lpw >= 1 && lpw <= kResampleMaxLpw, "resample: lowpass_filter_width %d is outside [1, %d]", lpw, kResampleMaxLpw);
  STTS_CHECK(rolloff > 0.0 && rolloff <= 1.0, "resample: rolloff %g is outside (0, 1]", rolloff);
  const int d = (int)resample_gcd(orig, fresh);
  const int o = orig / d, n = fresh / d;
  STTS_CHECK(o <= kResampleMaxFreq, "resample: orig_freq %d / gcd %d = %d is above %d", orig, d, o, kResampleMaxFreq);
  STTS_CHECK(n <= kResampleMaxFreq, "resample: new_freq %d / gcd %d = %d is above %d", fresh, d, n, kResampleMaxFreq);
  const double base = (double)std::min(o, n) * rolloff;
  const double w = std::ceil((double)lpw * (double)o / base);
  STTS_CHECK(w * 2.0 + o <= (double)kResampleMaxTable, "resample: %g taps (rolloff %g) are above %ld", w * 2.0 + o, rolloff, kResampleMaxTable);
  const int width = (int)w, taps = 2 * width + o;
  STTS_CHECK((long)n * taps <= kResampleMaxTable, "resample: %d phases x %d taps = %ld coefficients are above %ld", n, taps, (long)n * taps, kResampleMaxTable);
  g->o = o;
  g->n = n;
  g->width = width;
  g->taps = taps;
  return 0;
}

inline long resample_out_length(long len, int o, int n) { return ((long)n * len + o - 1) / o; }

// The block shape at R = kResampleR outputs per thread: P = min(n, 256) phases per block, G = as many groups of R input steps as the threads and the staging
// buffer hold - (G R - 1) o samples plus a chunk of taps, at most kResampleStage; G = 1 fits at every o <= 1024 while (R - 1) 1024 + 512 <= 4096.
struct ResamplePlan {
  int P, G;
  int steps() const { return G * kResampleR; }  // input steps q per block
};
inline ResamplePlan resample_plan(int o, int n) {
  ResamplePlan p;
  p.P = std::min(n, kResampleThreads);
  p.G = std::max(1, std::min(kResampleThreads / p.P, ((kResampleStage - kResampleChunk) / o + 1) / kResampleR));
  return p;
}
static_assert((kResampleR - 1) * kResampleMaxFreq + kResampleChunk <= kResampleStage, "the staging buffer must hold one group of R steps at the largest o");

// Consecutive outputs of an utterance that one row of blocks computes: G R input steps of n outputs each.
inline int resample_tile(int o, int n) { return resample_plan(o, n).steps() * n; }

struct ResampleTable {
  double* tab = nullptr;  // [taps][n]
};
using ResampleKey = std::tuple<int, int, int, double, int, double>;  // o, n, lpw, rolloff, method, beta (0 under Hann)

// The table of (o, n, lpw, rolloff, method, beta): built by resample_table_kernel on first use and kept for the context's lifetime
// (stts_ctx::resample).  The first use waits for the table kernel, so that later calls on any stream find it complete.
inline int resample_table(stts_ctx* c, hipStream_t st, const ResampleGeom& g, int lpw, double rolloff, int method, double beta, const ResampleTable** out) {
  std::lock_guard<std::mutex> lk(c->resample_mu);
  const ResampleKey key{g.o, g.n, lpw, rolloff, method, method == RESAMPLE_KAISER ? beta : 0.0};
  auto it = c->resample.find(key);
  if (it == c->resample.end()) {
    auto t = std::make_shared<ResampleTable>();
    const long elems = (long)g.taps * g.n;
    void* p = nullptr;
    STTS_HIP(hipMalloc(&p, (size_t)elems * sizeof(double)));
    c->allocs.push_back(p);
    c->alloc_tag.push_back(0);
    t->tab = (double*)p;
    hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, t->tab, g.o, g.n, g.width, g.taps, lpw, rolloff, method, beta);
    STTS_HIP(hipGetLastError());
    STTS_HIP(hipStreamSynchronize(st));
    it = c->resample.emplace(key, t).first;
  }
  *out = static_cast<const ResampleTable*>(it->second.get());
  return 0;
}

// offsets of a packed ragged batch: every utterance at least one sample, its outputs exactly ceil(n len / o); *max_out = the longest output
inline int resample_check_offsets(int n_utt, const int32_t* off_in, const int32_t* off_out, const ResampleGeom& g, long* max_out) {
  STTS_CHECK(n_utt > 0 && n_utt <= 65535, "resample: %d utterances are outside [1, 65535]", n_utt);
  STTS_CHECK(off_in && off_out && off_in[0] == 0 && off_out[0] == 0, "resample: bad offsets");
  *max_out = 0;
  long total = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long len = (long)off_in[u + 1] - off_in[u], m = (long)off_out[u + 1] - off_out[u];
    STTS_CHECK(len >= 1, "resample: utterance %d has %ld samples; at least 1 is needed", u, len);
    const long want = resample_out_length(len, g.o, g.n);
    STTS_CHECK(m == want, "resample: utterance %d: %ld output samples for %ld input samples at %d -> %d, the formula gives %ld", u, m, len, g.o, g.n, want);
    total += want;
    STTS_CHECK(total <= 0x7fffffffL, "resample: %ld output samples overflow the int32 offsets at utterance %d", total, u);
    *max_out = std::max(*max_out, m);
  }
  return 0;
}

inline int launch_resample(hipStream_t st, const ResampleTable& t, const ResampleGeom& g, int n_utt, long max_out, const int* off_in, const int* off_out,
                           const float* x, float* y) {
  const ResamplePlan pl = resample_plan(g.o, g.n);
  STTS_CHECK((long)(pl.steps() - 1) * g.o + kResampleChunk <= kResampleStage, "resample: %d steps of %d samples do not fit the staging buffer", pl.steps(), g.o);
  const long qmax = (max_out + g.n - 1) / g.n;
  const long blocks = ((qmax + pl.steps() - 1) / pl.steps()) * ((g.n + pl.P - 1) / pl.P);
  STTS_CHECK(blocks <= 0x7fffffffL, "resample: %ld blocks per utterance", blocks);
  hipLaunchKernelGGL(resample_kernel<kResampleR>, dim3((unsigned)blocks, n_utt), dim3(kResampleThreads), 0, st, x, off_in, off_out, t.tab, g.o, g.n, g.width,
                     g.taps, pl.P, pl.G, y);
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

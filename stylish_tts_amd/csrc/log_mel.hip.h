// Normalised log-mel front end of a recording: torchaudio.transforms.MelSpectrogram(n_mels, n_fft, win_length, hop_length, sample_rate) with its
// defaults (power 2, center=True / reflect, periodic Hann, HTK scale, f_min 0, f_max sample_rate / 2, norm None) followed by
// calculate_mel (train/stage_type.py:1023-1032), preprocess (train/dataprep/align_text.py:112-117), log_norm (train/utils.py:71-77) and
// compute_log_mel_stats (train/utils.py:80-148).
// One wave per frame on the one-wave transforms of signal_geom.hip.h, everything up to the output rounding in fp64: window product, the
// n_fft-point real transform as one n_fft/2-point complex one, power re^2 + im^2 (no square root), mel m = the nonzero band of filter m summed in
// bin order, log(1e-5 + mel), the normalisation.  Sums over the mel axis (energy, the statistics' per-frame partials) run lane m mod 64 in mel
// order, then a fixed xor butterfly: no result depends on the batch around a frame.  Built without packed-fp32 instructions.
#pragma once
#include <array>
#include <cmath>
#include <vector>

#include "signal_geom.hip.h"

namespace stts {

constexpr int kLogMelMaxMels = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Grid (ceil(max frames / kWaves), n_utt).  Utterance u: samples [samp_off[u], samp_off[u + 1]) of wave, frames = row_off[u + 1] - row_off[u] (at most
// samples / hop + 1: the entry point checks).  band[3 m .. 3 m + 2] = first bin, one past the last bin, offset of the filter's weights in wts.
// Every output is optional: out / raw rows [row][ld] (columns >= n_mels untouched), energy [row], part [row][2] = sum and sum of squares of the row's
// log(1e-5 + mel) over the mel axis.
// T2 = double2: the transform and the power in fp64 (what the engine runs).  T2 = float2: the same in fp32, for comparisons (STTS_LOG_MEL_F32=1 at the
// first call; DESIGN.md section 5l has its accuracy and time); the mel sums and everything after them stay fp64.
template <int LOGH, typename T2>
__global__ void __launch_bounds__(64 * GeomFft<LOGH>::kWaves) STTS_NO_PK
log_mel_kernel(const float* __restrict__ wave, const int* __restrict__ samp_off, const int* __restrict__ row_off, int hop, int win,
               const double* __restrict__ hann, const double2* __restrict__ twiddle, const int* __restrict__ band, const float* __restrict__ wts, int n_mels,
               double mean, double stdv, float* __restrict__ out, int ld, float* __restrict__ energy, float* __restrict__ raw, double* __restrict__ part) {
  using G = GeomFft<LOGH>;
  constexpr int H = G::H;
  using T = decltype(T2::x);
  __shared__ T2 bufs[G::kWaves][G::kBuf];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int nfr = row_off[u + 1] - row_off[u];
  if (f >= nfr) return;  // whole waves leave: nothing below synchronises across waves
  T2* Z = bufs[wv];
  const int wlo = (2 * H - win) / 2;
  const long L = samp_off[u + 1] - samp_off[u];
  const float* x = wave + samp_off[u];
  auto sample = [&](int p) -> T {
    if (p < wlo || p >= wlo + win) return (T)0;
    long m = (long)f * hop - H + p;
    if (m < 0) m = -m;
    if (m >= L) m = 2 * (L - 1) - m;
    m = m < 0 ? 0 : (m >= L ? L - 1 : m);  // in bounds whatever the length (the entry point refuses what cannot be reflected)
    return (T)((double)x[m] * hann[p - wlo]);
  };
  if constexpr (LOGH == 10) {
    const FftTw tw = fft_load_tw(twiddle, lane);
    T2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane + 64 * r;
      v[r].x = sample(2 * n);
      v[r].y = sample(2 * n + 1);
    }
    fft1024_wave<T2, false>(v, Z, tw, lane);
  } else {
#pragma unroll
    for (int r = 0; r < H / 64; ++r) {
      const int n = lane + 64 * r;
      T2 z;
      z.x = sample(2 * n);
      z.y = sample(2 * n + 1);
      Z[fphys(n)] = z;
    }
    wave_lds_fence();
    fft_wave_r2<T2, LOGH, false>(Z, twiddle, lane);
  }
  // power of bins 0 .. H into registers, then over the transform's buffer as a plain array P[0 .. H]
  const T2 z0 = Z[0];
  T pw[H / 64];
#pragma unroll
  for (int r = 0; r < H / 64; ++r) {
    const int k = lane + 64 * r;
    T re, im = (T)0;
    if (k == 0) {
      re = z0.x + z0.y;
    } else {
      const T2 a = Z[fphys(k)], b = Z[fphys(H - k)], w = to_t2<T2>(twiddle[k], false);  // w = exp(-2 pi i k / 2H)
      const T er = (T)0.5 * (a.x + b.x), ei = (T)0.5 * (a.y - b.y);
      const T orr = (T)0.5 * (a.y + b.y), oi = (T)-0.5 * (a.x - b.x);
      re = er + orr * w.x - oi * w.y;
      im = ei + orr * w.y + oi * w.x;
    }
    pw[r] = re * re + im * im;
  }
  wave_lds_fence();
  T* P = reinterpret_cast<T*>(Z);  // H + 1 of the buffer's 2 kBuf scalars
#pragma unroll
  for (int r = 0; r < H / 64; ++r) P[lane + 64 * r] = pw[r];
  if (lane == 0) P[H] = (z0.x - z0.y) * (z0.x - z0.y);
  wave_lds_fence();
  const long row = row_off[u] + f;
  double es = 0.0, s1 = 0.0, s2 = 0.0;
  for (int m = lane; m < n_mels; m += 64) {
    const int lo = band[3 * m], hi = band[3 * m + 1];
    const float* bw = wts + band[3 * m + 2];
    double s = 0.0;
    for (int k = lo; k < hi; ++k) s = fma((double)bw[k - lo], (double)P[k], s);
    const double v = 1e-5 + s, lg = log(v);
    if (out) out[row * ld + m] = (float)((lg - mean) / stdv);
    if (raw) raw[row * ld + m] = (float)lg;
    if (energy) es += pow(v, 0.33);
    s1 += lg;
    s2 += lg * lg;
  }
  if (energy) {
    es = wave_sum_f64(es);
    if (lane == 0) energy[row] = (float)es;
  }
  if (part) {
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (lane == 0) {
      part[2 * row] = s1;
      part[2 * row + 1] = s2;
    }
  }
}

// compute_log_mel_stats' reduction: thread t sums rows t, t + 256, ... in order, a fixed tree joins the 256 sums; stats = (mean, std, count) with
// the unbiased variance and its 1e-12 clamp (16 for a single value).  One block.
__global__ void __launch_bounds__(256) STTS_NO_PK log_mel_stats_kernel(const double* __restrict__ part, long rows, int n_mels, double* __restrict__ stats) {
  __shared__ double a[256], b[256];
  double s1 = 0.0, s2 = 0.0;
  for (long r = threadIdx.x; r < rows; r += 256) {
    s1 += part[2 * r];
    s2 += part[2 * r + 1];
  }
  a[threadIdx.x] = s1;
  b[threadIdx.x] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      a[threadIdx.x] += a[threadIdx.x + o];
      b[threadIdx.x] += b[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double count = (double)rows * (double)n_mels;
    const double mu = a[0] / count;
    const double var = count > 1.0 ? (b[0] - count * mu * mu) / (count - 1.0) : 16.0;
    stats[0] = mu;
    stats[1] = sqrt(fmax(var, 1e-12));
    stats[2] = count;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// torchaudio.functional.melscale_fbanks(n_fft / 2 + 1, 0, sample_rate // 2, n_mels, sample_rate, norm=None, mel_scale="htk") in float64, rounded
// once to fp32: band[2 m], band[2 m + 1] = the nonzero bins [first, one past the last) of filter m (first = last = 0 for an empty filter),
// dense [n_mels][n_fft / 2 + 1].
inline void log_mel_filters(int n_fft, int n_mels, int sample_rate, std::vector<int>* band, std::vector<float>* dense) {
  const int bins = n_fft / 2 + 1;
  const double f_max = (double)(sample_rate / 2);
  const double m_max = 2595.0 * std::log10(1.0 + f_max / 700.0);
  std::vector<double> fp(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) fp[i] = 700.0 * (std::pow(10.0, (m_max * i / (n_mels + 1)) / 2595.0) - 1.0);
  band->assign(2 * (size_t)n_mels, 0);
  dense->assign((size_t)n_mels * bins, 0.f);
  for (int m = 0; m < n_mels; ++m) {
    int lo = 0, hi = 0;
    bool any = false;
    for (int k = 0; k < bins; ++k) {
      const double fr = f_max * k / (bins - 1);
      const double down = (fr - fp[m]) / (fp[m + 1] - fp[m]), up = (fp[m + 2] - fr) / (fp[m + 2] - fp[m + 1]);
      const float w = (float)std::max(0.0, std::min(down, up));
      (*dense)[(size_t)m * bins + k] = w;
      if (w > 0.f) {
        if (!any) lo = k;
        any = true;
        hi = k + 1;
      }
    }
    (*band)[2 * m] = lo;
    (*band)[2 * m + 1] = hi;
  }
}

struct LogMelTables {
  double* hann = nullptr;  // periodic Hann(win) in fp64
  double2* tw = nullptr;   // exp(-2 pi i m / n_fft), m < n_fft / 2
  int* band = nullptr;     // [n_mels][3]: first bin, one past the last, offset into wts
  float* wts = nullptr;    // the filters' nonzero bands, one after the other
};

inline int log_mel_check_geometry(int n_fft, int win, int hop, int n_mels, int sample_rate) {
  STTS_CHECK(n_fft > 0 && (n_fft & (n_fft - 1)) == 0, "log_mel: n_fft %d is not a power of two", n_fft);
  STTS_CHECK(n_fft >= 256 && n_fft <= 4096, "log_mel: n_fft %d is outside [256, 4096]", n_fft);
  STTS_CHECK(win >= 1 && win <= n_fft, "log_mel: win_length %d is outside [1, n_fft = %d]", win, n_fft);
  STTS_CHECK(hop >= 1, "log_mel: hop_length %d is not positive", hop);
  STTS_CHECK(n_mels >= 1 && n_mels <= kLogMelMaxMels, "log_mel: n_mels %d is outside [1, %d]", n_mels, kLogMelMaxMels);
  STTS_CHECK(sample_rate >= 2, "log_mel: sample_rate %d is not positive", sample_rate);
  return 0;
}

// The tables of (n_fft, win, n_mels, sample_rate), built and uploaded on first use and kept for the context's lifetime (stts_ctx::log_mel).
inline int log_mel_tables(stts_ctx* c, int n_fft, int win, int n_mels, int sample_rate, const LogMelTables** out) {
  std::lock_guard<std::mutex> lk(c->log_mel_mu);
  const std::array<int, 4> key{n_fft, win, n_mels, sample_rate};
  auto it = c->log_mel.find(key);
  if (it == c->log_mel.end()) {
    auto t = std::make_shared<LogMelTables>();
    std::vector<float> hann32;
    std::vector<double2> tw;
    signal_tables(n_fft, win, &hann32, &tw);
    std::vector<double> hann(win);
    for (int i = 0; i < win; ++i) hann[i] = 0.5 - 0.5 * cos(2.0 * M_PI * i / win);
    std::vector<int> band2;
    std::vector<float> dense;
    log_mel_filters(n_fft, n_mels, sample_rate, &band2, &dense);
    const int bins = n_fft / 2 + 1;
    std::vector<int> band(3 * (size_t)n_mels);
    std::vector<float> wts;
    for (int m = 0; m < n_mels; ++m) {
      band[3 * m] = band2[2 * m];
      band[3 * m + 1] = band2[2 * m + 1];
      band[3 * m + 2] = (int)wts.size();
      for (int k = band2[2 * m]; k < band2[2 * m + 1]; ++k) wts.push_back(dense[(size_t)m * bins + k]);
    }
    PackScope scope(c, engine_mode(c));  // context lifetime
    STTS_TRY(dev_upload(c, hann, &t->hann));
    STTS_TRY(dev_upload(c, tw, &t->tw));
    STTS_TRY(dev_upload(c, band, &t->band));
    STTS_TRY(dev_upload(c, wts, &t->wts));
    it = c->log_mel.emplace(key, t).first;
  }
  *out = static_cast<const LogMelTables*>(it->second.get());
  return 0;
}

// offsets of a packed ragged batch: every utterance longer than n_fft / 2 samples (torch.stft's reflect padding), 1 <= frames <= samples / hop + 1
inline int log_mel_check_offsets(int n_utt, const int32_t* samp_off, const int32_t* row_off, int n_fft, int hop, int* max_fr) {
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && samp_off && row_off && samp_off[0] == 0 && row_off[0] == 0, "log_mel: bad offsets");
  *max_fr = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)samp_off[u + 1] - samp_off[u], fr = (long)row_off[u + 1] - row_off[u];
    STTS_CHECK(n > n_fft / 2, "log_mel: utterance %d has %ld samples; the reflect padding needs more than n_fft / 2 = %d", u, n, n_fft / 2);
    STTS_CHECK(fr >= 1 && fr <= n / hop + 1, "log_mel: utterance %d: %ld frames for %ld samples at hop %d (1 .. %ld)", u, fr, n, hop, n / hop + 1);
    *max_fr = std::max(*max_fr, (int)fr);
  }
  return 0;
}

inline int launch_log_mel(hipStream_t st, const LogMelTables& t, int n_fft, int win, int hop, int n_mels, int n_utt, int max_fr, const int* samp_off,
                          const int* row_off, const float* wave, double mean, double stdv, float* out, int ld, float* energy, float* raw, double* part) {
  static const bool f32 = getenv("STTS_LOG_MEL_F32") && atoi(getenv("STTS_LOG_MEL_F32")) != 0;  // comparisons: the fp32 transform
#define STTS_LOG_MEL_T(LG, T2)                                                                                                                            \
  hipLaunchKernelGGL((log_mel_kernel<LG, T2>), dim3(ceil_div(max_fr, GeomFft<LG>::kWaves), n_utt), dim3(64 * GeomFft<LG>::kWaves), 0, st, wave, samp_off, \
                     row_off, hop, win, t.hann, t.tw, t.band, t.wts, n_mels, mean, stdv, out, ld, energy, raw, part)
#define STTS_LOG_MEL(LG)             \
  if (f32) {                         \
    STTS_LOG_MEL_T(LG, float2);      \
  } else {                           \
    STTS_LOG_MEL_T(LG, double2);     \
  }
  switch (n_fft) {
    case 256: STTS_LOG_MEL(7); break;
    case 512: STTS_LOG_MEL(8); break;
    case 1024: STTS_LOG_MEL(9); break;
    case 2048: STTS_LOG_MEL(10); break;
    case 4096: STTS_LOG_MEL(11); break;
    default: return fail("log_mel: n_fft %d not instantiated", n_fft);
  }
#undef STTS_LOG_MEL
#undef STTS_LOG_MEL_T
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

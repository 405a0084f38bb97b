// Validation scores of the reference's validate_* functions (train/stage_type.py): MultiSpectrogram (train/multi_spectrogram.py) feeding
// MultiResolutionSTFTLoss ("mel", train/losses.py:14-35), MagPhaseLoss ("mag" / "phase", losses.py:38-154) and smooth_l1_loss ("pitch" / "energy");
// at the end of the kernels the sums of DurationLoss ("duration_ce" / "duration", losses.py:429-476) and of l1_loss / mse_loss ("linear_pitch",
// "mel_l2", "normed_pitch_l2").
//   calculate_single, per resolution (fft, hop, window): X = torch.stft(audio, fft, hop, window, periodic Hann(window)) (center=True, reflect,
//   one-sided, unnormalised); fft_mag = |X|; phase = (fft_mag > 1e-3) * angle(X); mag = log1p(MelScale(128, sample_rate, fft / 2 + 1)(fft_mag))
//   (HTK, norm None, f_min 0, f_max sample_rate / 2: the filters of log_mel.hip.h).
// One wave per frame on the one-wave transforms of signal_geom.hip.h, everything in fp64: window product, the n_fft-point real transform as one
// n_fft/2-point complex one, sqrt(re^2 + im^2), mel m = the nonzero band of filter m summed in bin order (lanes take mels m, m + 64, ...), log1p.
// Sums over a frame run lane by lane in a fixed order, then the fixed xor butterfly of wave_sum_f64; sums over an utterance's frames run thread t
// over rows t, t + 256, ... in order, then a fixed tree: no result depends on the batch around an utterance, none uses an atomic.  Every kernel is
// built without packed-fp32 instructions.  The caller owns every buffer (stts_val_sizes); no kernel allocates.
#pragma once
#include <array>
#include <cmath>
#include <vector>

#include "log_mel.hip.h"

namespace stts {

constexpr double kValMask = 1e-3;       // the reference's magnitude threshold of a phase that counts
constexpr double kValMaskedOff = 8.0;   // scratch value of a masked-off bin: outside atan2's range [-pi, pi]
constexpr int kValMelsPerLane = kLogMelMaxMels / 64;

// |d - 2 pi round(d / 2 pi)| (anti_wrapping_loss, losses.py:38-40; torch.round rounds halves to even, like rint)
__device__ __forceinline__ double val_anti_wrap(double d) {
  constexpr double two_pi = 2.0 * M_PI;
  return fabs(d - two_pi * rint(d / two_pi));
}

// Frame f of the signal x[0 .. L): windowed, transformed by this wave in Z (natural order, fphys layout).  log_mel_kernel's indexing.
template <int LOGH>
__device__ __forceinline__ void val_transform(const float* __restrict__ x, long L, int f, int hop, int win, const double* __restrict__ hann,
                                              const double2* __restrict__ twiddle, double2* Z, int lane) {
  constexpr int H = 1 << LOGH;
  const int wlo = (2 * H - win) / 2;
  auto sample = [&](int p) -> double {
    if (p < wlo || p >= wlo + win) return 0.0;
    long m = (long)f * hop - H + p;
    if (m < 0) m = -m;
    if (m >= L) m = 2 * (L - 1) - m;
    m = m < 0 ? 0 : (m >= L ? L - 1 : m);  // in bounds whatever the length (the entry point refuses what cannot be reflected)
    return (double)x[m] * hann[p - wlo];
  };
  if constexpr (LOGH == 10) {
    const FftTw tw = fft_load_tw(twiddle, lane);
    double2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane + 64 * r;
      v[r].x = sample(2 * n);
      v[r].y = sample(2 * n + 1);
    }
    fft1024_wave<double2, false>(v, Z, tw, lane);
  } else {
#pragma unroll
    for (int r = 0; r < H / 64; ++r) {
      const int n = lane + 64 * r;
      double2 z;
      z.x = sample(2 * n);
      z.y = sample(2 * n + 1);
      Z[fphys(n)] = z;
    }
    wave_lds_fence();
    fft_wave_r2<double2, LOGH, false>(Z, twiddle, lane);
  }
}

// bin k (0 < k < H) of the 2H-point real transform from the H-point complex one in Z
template <int LOGH>
__device__ __forceinline__ void val_bin(const double2* Z, const double2* __restrict__ twiddle, int k, double& re, double& im) {
  constexpr int H = 1 << LOGH;
  const double2 a = Z[fphys(k)], b = Z[fphys(H - k)], w = twiddle[k];  // w = exp(-2 pi i k / 2H)
  const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
  const double orr = 0.5 * (a.y + b.y), oi = -0.5 * (a.x - b.x);
  re = er + orr * w.x - oi * w.y;
  im = ei + orr * w.y + oi * w.x;
}

// calculate_single of one frame: fft_mag / masked phase rows (optional, [row][ld_bins], bins 0 .. H) and lm[j] = log1p(mel lane + 64 j), also
// written to mag [row][ld_mag] when given.  Leaves Z free for the next frame.
template <int LOGH>
__device__ __forceinline__ void val_frame(const float* __restrict__ x, long L, int f, int hop, int win, const double* __restrict__ hann,
                                          const double2* __restrict__ twiddle, const int* __restrict__ band, const float* __restrict__ wts, int n_mels,
                                          double2* Z, int lane, long row, float* __restrict__ mag, int ld_mag, float* __restrict__ fft_mag,
                                          float* __restrict__ phase, int ld_bins, double (&lm)[kValMelsPerLane]) {
  constexpr int H = 1 << LOGH;
  val_transform<LOGH>(x, L, f, hop, win, hann, twiddle, Z, lane);
  const double2 z0 = Z[0];
  double mg[H / 64];
#pragma unroll
  for (int r = 0; r < H / 64; ++r) {
    const int k = lane + 64 * r;
    double re, im = 0.0;
    if (k == 0) {
      re = z0.x + z0.y;
    } else {
      val_bin<LOGH>(Z, twiddle, k, re, im);
    }
    mg[r] = sqrt(re * re + im * im);
    if (fft_mag) fft_mag[row * ld_bins + k] = (float)mg[r];
    if (phase) phase[row * ld_bins + k] = mg[r] > kValMask ? (float)atan2(im, re) : 0.f;
  }
  wave_lds_fence();
  double* P = reinterpret_cast<double*>(Z);  // H + 1 of the buffer's 2 kBuf scalars
#pragma unroll
  for (int r = 0; r < H / 64; ++r) P[lane + 64 * r] = mg[r];
  if (lane == 0) {
    const double re = z0.x - z0.y, m = fabs(re);
    P[H] = m;
    if (fft_mag) fft_mag[row * ld_bins + H] = (float)m;
    if (phase) phase[row * ld_bins + H] = m > kValMask ? (float)atan2(0.0, re) : 0.f;
  }
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < kValMelsPerLane; ++j) {
    const int m = lane + 64 * j;
    lm[j] = 0.0;
    if (m < n_mels) {
      const int lo = band[3 * m], hi = band[3 * m + 1];
      const float* bw = wts + band[3 * m + 2];
      double s = 0.0;
      for (int k = lo; k < hi; ++k) s = fma((double)bw[k - lo], P[k], s);
      lm[j] = log1p(s);
      if (mag) mag[row * ld_mag + m] = (float)lm[j];
    }
  }
  wave_lds_fence();
}

// Grid (ceil(max frames / kWaves), n_utt).  Utterance u: samples [samp_off[u], samp_off[u + 1]) of a (and of b), frames = row_off[u + 1] - row_off[u].
// PAIR = false, MultiSpectrogram: a's mag [row][ld_mag] (columns >= n_mels untouched), fft_mag and masked phase [row][ld_bins] (columns > H untouched),
// each optional, each rounded once from fp64.  PAIR = true, the fused score: the wave transforms frame f of the target a and of the prediction b
// and writes part[row] = (sum_m |t - p|, sum_m |t|) of their log1p mel rows; no spectrogram is written.
template <int LOGH, bool PAIR>
__global__ void __launch_bounds__(64 * GeomFft<LOGH>::kWaves) STTS_NO_PK
val_spec_kernel(const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ samp_off, const int* __restrict__ row_off, int hop, int win,
                const double* __restrict__ hann, const double2* __restrict__ twiddle, const int* __restrict__ band, const float* __restrict__ wts, int n_mels,
                float* __restrict__ mag, int ld_mag, float* __restrict__ fft_mag, float* __restrict__ phase, int ld_bins, double* __restrict__ part) {
  using G = GeomFft<LOGH>;
  __shared__ double2 bufs[G::kWaves][G::kBuf];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int nfr = row_off[u + 1] - row_off[u];
  if (f >= nfr) return;  // whole waves leave: nothing below synchronises across waves
  double2* Z = bufs[wv];
  const long L = samp_off[u + 1] - samp_off[u];
  const long row = row_off[u] + f;
  double lt[kValMelsPerLane];
  if constexpr (!PAIR) {
    val_frame<LOGH>(a + samp_off[u], L, f, hop, win, hann, twiddle, band, wts, n_mels, Z, lane, row, mag, ld_mag, fft_mag, phase, ld_bins, lt);
  } else {
    double lp[kValMelsPerLane];
    val_frame<LOGH>(a + samp_off[u], L, f, hop, win, hann, twiddle, band, wts, n_mels, Z, lane, row, nullptr, 0, nullptr, nullptr, 0, lt);
    val_frame<LOGH>(b + samp_off[u], L, f, hop, win, hann, twiddle, band, wts, n_mels, Z, lane, row, nullptr, 0, nullptr, nullptr, 0, lp);
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int j = 0; j < kValMelsPerLane; ++j) {  // mels past n_mels hold 0 on both sides
      num += fabs(lt[j] - lp[j]);
      den += fabs(lt[j]);
    }
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    if (lane == 0) {
      part[2 * row] = num;
      part[2 * row + 1] = den;
    }
  }
}

// sums[u][0 .. NC) = the utterance's rows of part [row][NC] added in a fixed order: thread t takes rows t, t + 256, ... in order, a fixed tree joins
// the 256 sums.  One block per utterance.
template <int NC>
__global__ void __launch_bounds__(256) STTS_NO_PK val_reduce_kernel(const double* __restrict__ part, const int* __restrict__ row_off, double* __restrict__ sums) {
  __shared__ double acc[NC][256];
  const int u = blockIdx.x;
  const long lo = row_off[u], n = row_off[u + 1] - lo;
  double s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  for (long r = threadIdx.x; r < n; r += 256) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] += part[NC * (lo + r) + c];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c][threadIdx.x] += acc[c][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < NC) sums[NC * u + threadIdx.x] = acc[threadIdx.x][0];
}

// MagPhaseLoss.forward, the part of a frame that needs no neighbour.  One wave per frame of the recording gt; Y = its transform.
//   target_mag = |Y| + 1e-14, on = target_mag > 1e-3, tp = on ? atan2(im, re) : 0, pp = on ? phase_rows[row][k] : 0 (the input is not modified)
//   part[row][0] = sum_k |logamp_rows[row][k] - log(target_mag + 1e-9)|
//   part[row][1] = sum_k w_k aw(pp[k] - tp[k])                                         aw = val_anti_wrap
//   part[row][2] = sum_k w_k aw((pp[k-1] - pp[k]) - (tp[k-1] - tp[k])), pp[-1] = tp[-1] = 0   (freq_matrix, losses.py:52-62)
//   scratch[row][k] = on ? tp : kValMaskedOff  (fp64, [rows][H + 1]): what val_phase_time_kernel differences along the frames
template <int LOGH>
__global__ void __launch_bounds__(64 * GeomFft<LOGH>::kWaves) STTS_NO_PK
val_magphase_kernel(const float* __restrict__ gt, const int* __restrict__ samp_off, const int* __restrict__ row_off, int hop, int win,
                    const double* __restrict__ hann, const double2* __restrict__ twiddle, const double* __restrict__ wk, const float* __restrict__ logamp,
                    const float* __restrict__ pphase, int ld, double* __restrict__ scratch, double* __restrict__ part) {
  using G = GeomFft<LOGH>;
  constexpr int H = G::H;
  __shared__ double2 bufs[G::kWaves][G::kBuf];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int nfr = row_off[u + 1] - row_off[u];
  if (f >= nfr) return;  // whole waves leave: nothing below synchronises across waves
  double2* Z = bufs[wv];
  const long L = samp_off[u + 1] - samp_off[u];
  const long row = row_off[u] + f;
  val_transform<LOGH>(gt + samp_off[u], L, f, hop, win, hann, twiddle, Z, lane);
  const float* la = logamp + row * ld;
  const float* ph = pphase + row * ld;
  double* sc = scratch + row * (H + 1);
  double s_mag = 0.0;
  // (tp, pp) of bin k from its (re, im); adds the bin's magnitude term
  auto bin = [&](int k, double re, double im, double& tp, double& pp) {
    const double tm = sqrt(re * re + im * im) + 1e-14;
    const bool on = tm > kValMask;
    s_mag += fabs((double)la[k] - log(tm + 1e-9));
    tp = on ? atan2(im, re) : 0.0;
    pp = on ? (double)ph[k] : 0.0;
    sc[k] = on ? tp : kValMaskedOff;
  };
  const double2 z0 = Z[0];
  double tp[H / 64], pp[H / 64];
#pragma unroll
  for (int r = 0; r < H / 64; ++r) {
    const int k = lane + 64 * r;
    double re, im = 0.0;
    if (k == 0) {
      re = z0.x + z0.y;
    } else {
      val_bin<LOGH>(Z, twiddle, k, re, im);
    }
    bin(k, re, im, tp[r], pp[r]);
  }
  wave_lds_fence();
  double* TP = reinterpret_cast<double*>(Z);  // 2 (H + 1) of the buffer's 2 kBuf scalars
  double* PP = TP + (H + 1);
#pragma unroll
  for (int r = 0; r < H / 64; ++r) {
    TP[lane + 64 * r] = tp[r];
    PP[lane + 64 * r] = pp[r];
  }
  if (lane == 0) {
    double t, p;
    bin(H, z0.x - z0.y, 0.0, t, p);
    TP[H] = t;
    PP[H] = p;
  }
  wave_lds_fence();
  double s_inst = 0.0, s_freq = 0.0;
  for (int k = lane; k <= H; k += 64) {
    const double w = wk[k], t = TP[k], p = PP[k];
    const double tl = k > 0 ? TP[k - 1] : 0.0, pl = k > 0 ? PP[k - 1] : 0.0;
    s_inst += w * val_anti_wrap(p - t);
    s_freq += w * val_anti_wrap((pl - p) - (tl - t));
  }
  s_mag = wave_sum_f64(s_mag);
  s_inst = wave_sum_f64(s_inst);
  s_freq = wave_sum_f64(s_freq);
  if (lane == 0) {
    part[4 * row] = s_mag;
    part[4 * row + 1] = s_inst;
    part[4 * row + 2] = s_freq;
  }
}

// part[row][3] = sum_k w_k aw((pp[f-1][k] - pp[f][k]) - (tp[f-1][k] - tp[f][k])), frame -1 = 0 (time_matrix, losses.py:64-73), from the scratch rows
// of val_magphase_kernel.  One wave per frame, four to a block; grid (ceil(max frames / 4), n_utt).
__global__ void __launch_bounds__(256) STTS_NO_PK
val_phase_time_kernel(const int* __restrict__ row_off, int bins, const double* __restrict__ wk, const float* __restrict__ pphase, int ld,
                      const double* __restrict__ scratch, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * 4 + wv;
  const int nfr = row_off[u + 1] - row_off[u];
  if (f >= nfr) return;
  const long row = row_off[u] + f;
  double s = 0.0;
  for (int k = lane; k < bins; k += 64) {
    const double sv = scratch[row * bins + k];
    const bool on = sv < 0.5 * kValMaskedOff;
    const double t = on ? sv : 0.0, p = on ? (double)pphase[row * ld + k] : 0.0;
    double tl = 0.0, pl = 0.0;
    if (f > 0) {
      const double sl = scratch[(row - 1) * bins + k];
      if (sl < 0.5 * kValMaskedOff) {
        tl = sl;
        pl = (double)pphase[(row - 1) * ld + k];
      }
    }
    s += wk[k] * val_anti_wrap((pl - p) - (tl - t));
  }
  s = wave_sum_f64(s);
  if (lane == 0) part[4 * row + 3] = s;
}

// sums[u] = sum over the utterance's values of smooth_l1(a - b), beta 1: 0.5 d^2 below |d| = 1, |d| - 0.5 from there on, in fp64.  One block per
// utterance: thread t takes values t, t + 256, ... in order, a fixed tree joins the 256 sums.
__global__ void __launch_bounds__(256) STTS_NO_PK val_smooth_l1_kernel(const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ off,
                                                                       double* __restrict__ sums) {
  __shared__ double acc[256];
  const int u = blockIdx.x;
  const long lo = off[u], n = off[u + 1] - lo;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double d = fabs((double)a[lo + i] - (double)b[lo + i]);
    s += d < 1.0 ? 0.5 * d * d : d - 0.5;
  }
  acc[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[u] = acc[0];
}

// The sibling of val_smooth_l1_kernel for mse_loss / l1_loss: sums[u] = sum of |a - b| (KIND 0) or of (a - b)^2 (KIND 1) in fp64, same order.
template <int KIND>
__global__ void __launch_bounds__(256) STTS_NO_PK val_diff_kernel(const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ off,
                                                                  double* __restrict__ sums) {
  __shared__ double acc[256];
  const int u = blockIdx.x;
  const long lo = off[u], n = off[u + 1] - lo;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double d = (double)a[lo + i] - (double)b[lo + i];
    s += KIND == 0 ? fabs(d) : d * d;
  }
  acc[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[u] = acc[0];
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// The sums of CDW_CCELoss (train/losses.py:429-459, alpha = 2) over one utterance's token rows.  One wave per row, lane c = class c < C <= 64:
// softmax and log-softmax in fp64 from the fp32 logits, t = the row's target class clamped to [0, C - 1], d[t][c] = min(|t - c|, 7)^2:
//   sums[u][0] = sum_p lsm[p][t] * w[t]      sums[u][1] = sum_p w[t]      sums[u][2] = sum_p sum_c log(1 - sm[p][c] + 1e-9) * (d[t][c] / sum_c d[t][c])
// Wave w of the block's four takes rows w, w + 4, ... in order; the four waves' sums are joined in wave order.  grid n_utt, block 256.
__global__ void __launch_bounds__(256) STTS_NO_PK val_duration_kernel(const float* __restrict__ logits, int ld, int C, const int* __restrict__ targets,
                                                                      const float* __restrict__ weight, const int* __restrict__ p_off, double* __restrict__ sums) {
  __shared__ double acc[4][3];
  const int u = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long lo = p_off[u], n = p_off[u + 1] - lo;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long p = wv; p < n; p += 4) {
    const double x = lane < C ? (double)logits[(lo + p) * ld + lane] : -INFINITY;
    const double m = wave_max_f64(x);
    const double ex = lane < C ? exp(x - m) : 0.0;
    const double tot = wave_sum_f64(ex);
    const double lsm = (x - m) - log(tot), sm = ex / tot;
    const int t = min(max(targets[lo + p], 0), C - 1);
    const int k = min(abs(t - lane), 7);
    const double d = lane < C ? (double)(k * k) : 0.0;
    const double D = wave_sum_f64(d);
    const double cdw = lane < C ? log((1.0 - sm) + 1e-9) * (d / D) : 0.0;
    const double w = (double)weight[t];
    s0 += __shfl(lsm, t, 64) * w;
    s1 += w;
    s2 += wave_sum_f64(cdw);
  }
  if (lane == 0) {
    acc[wv][0] = s0;
    acc[wv][1] = s1;
    acc[wv][2] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3) sums[3 * u + threadIdx.x] = ((acc[0][threadIdx.x] + acc[1][threadIdx.x]) + acc[2][threadIdx.x]) + acc[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ host side
struct ValTables {
  double* hann = nullptr;  // periodic Hann(win) in fp64
  double2* tw = nullptr;   // exp(-2 pi i m / n_fft), m < n_fft / 2
  double* wk = nullptr;    // base^k, k <= n_fft / 2, base = exp(ln 2.5 / ((n_fft / 2 + 1) / 2)) (differential_phase_loss, losses.py:43-48)
};

// The tables of (n_fft, win), built and uploaded on first use and kept for the context's lifetime (stts_ctx::val_scores).
inline int val_tables(stts_ctx* c, int n_fft, int win, const ValTables** out) {
  std::lock_guard<std::mutex> lk(c->val_scores_mu);
  const std::array<int, 2> key{n_fft, win};
  auto it = c->val_scores.find(key);
  if (it == c->val_scores.end()) {
    auto t = std::make_shared<ValTables>();
    std::vector<float> hann32;
    std::vector<double2> tw;
    signal_tables(n_fft, win, &hann32, &tw);
    std::vector<double> hann(win);
    for (int i = 0; i < win; ++i) hann[i] = 0.5 - 0.5 * cos(2.0 * M_PI * i / win);
    const int bins = n_fft / 2 + 1;
    const double base = std::exp(std::log(2.5) / (bins / 2));
    std::vector<double> wk(bins);
    for (int k = 0; k < bins; ++k) wk[k] = std::pow(base, (double)k);
    PackScope scope(c, engine_mode(c));  // context lifetime
    STTS_TRY(dev_upload(c, hann, &t->hann));
    STTS_TRY(dev_upload(c, tw, &t->tw));
    STTS_TRY(dev_upload(c, wk, &t->wk));
    it = c->val_scores.emplace(key, t).first;
  }
  *out = static_cast<const ValTables*>(it->second.get());
  return 0;
}

// Every utterance with all of its samples / hop + 1 frames (the scores are means over whole spectrograms); the rest as log_mel_check_offsets.
inline int val_check_offsets(const char* what, int n_utt, const int32_t* samp_off, const int32_t* row_off, int n_fft, int hop, int* max_fr) {
  STTS_TRY(log_mel_check_offsets(n_utt, samp_off, row_off, n_fft, hop, max_fr));
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)samp_off[u + 1] - samp_off[u], fr = (long)row_off[u + 1] - row_off[u];
    STTS_CHECK(fr == n / hop + 1, "%s: utterance %d has %ld rows; its %ld samples at hop %d make %ld frames", what, u, fr, n, hop, n / hop + 1);
  }
  return 0;
}

#define STTS_VAL_SWITCH(n_fft, MACRO)                                        \
  switch (n_fft) {                                                           \
    case 256: MACRO(7); break;                                               \
    case 512: MACRO(8); break;                                               \
    case 1024: MACRO(9); break;                                              \
    case 2048: MACRO(10); break;                                             \
    case 4096: MACRO(11); break;                                             \
    default: return fail("val_scores: n_fft %d not instantiated", n_fft);    \
  }

// b = nullptr: MultiSpectrogram's rows of a; otherwise the fused score of (a, b) into part, reduced per utterance into sums [n_utt][2]
inline int launch_val_spec(hipStream_t st, const LogMelTables& t, int n_fft, int win, int hop, int n_mels, int n_utt, int max_fr, const int* samp_off,
                           const int* row_off, const float* a, const float* b, float* mag, int ld_mag, float* fft_mag, float* phase, int ld_bins, double* part,
                           double* sums) {
#define STTS_VAL_SPEC_T(LG, PAIR)                                                                                                                   \
  hipLaunchKernelGGL((val_spec_kernel<LG, PAIR>), dim3(ceil_div(max_fr, GeomFft<LG>::kWaves), n_utt), dim3(64 * GeomFft<LG>::kWaves), 0, st, a, b, \
                     samp_off, row_off, hop, win, t.hann, t.tw, t.band, t.wts, n_mels, mag, ld_mag, fft_mag, phase, ld_bins, part)
#define STTS_VAL_SPEC(LG)        \
  if (b) {                       \
    STTS_VAL_SPEC_T(LG, true);   \
  } else {                       \
    STTS_VAL_SPEC_T(LG, false);  \
  }
  STTS_VAL_SWITCH(n_fft, STTS_VAL_SPEC)
#undef STTS_VAL_SPEC
#undef STTS_VAL_SPEC_T
  STTS_HIP(hipGetLastError());
  if (b) {
    hipLaunchKernelGGL(val_reduce_kernel<2>, dim3(n_utt), dim3(256), 0, st, part, row_off, sums);
    STTS_HIP(hipGetLastError());
  }
  return 0;
}

inline int launch_val_magphase(hipStream_t st, const ValTables& t, int n_fft, int win, int hop, int n_utt, int max_fr, const int* samp_off, const int* row_off,
                               const float* gt, const float* logamp, const float* pphase, int ld, double* scratch, double* part, double* sums) {
#define STTS_VAL_MP(LG)                                                                                                                                \
  hipLaunchKernelGGL(val_magphase_kernel<LG>, dim3(ceil_div(max_fr, GeomFft<LG>::kWaves), n_utt), dim3(64 * GeomFft<LG>::kWaves), 0, st, gt, samp_off, \
                     row_off, hop, win, t.hann, t.tw, t.wk, logamp, pphase, ld, scratch, part)
  STTS_VAL_SWITCH(n_fft, STTS_VAL_MP)
#undef STTS_VAL_MP
  STTS_HIP(hipGetLastError());
  hipLaunchKernelGGL(val_phase_time_kernel, dim3(ceil_div(max_fr, 4), n_utt), dim3(256), 0, st, row_off, n_fft / 2 + 1, t.wk, pphase, ld, scratch, part);
  STTS_HIP(hipGetLastError());
  hipLaunchKernelGGL(val_reduce_kernel<4>, dim3(n_utt), dim3(256), 0, st, part, row_off, sums);
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

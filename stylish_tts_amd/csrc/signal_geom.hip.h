// Harmonic source, STFT and iSTFT at a run-time STFT geometry (model.yml n_fft / win_length / hop_length other than
// 2048 / 1200 / 300).  The kernels of signal.hip.h stay specialised for the default geometry and are what the engine runs
// there; these run every other geometry (and the default one under STTS_SIGNAL_GENERIC=1, for comparisons).
//   n_fft = 2H, H = 2^LOGH in [128, 2048]; 1 <= win <= n_fft, periodic Hann(win) centred at (n_fft - win) / 2; vocoder hop h = hop / 4.
// Same arithmetic as signal.hip.h: fp64 phase prefix and fp64 forward transform, fp32 inverse without packed-fp32 instructions,
// one wave per frame.  Transforms of H != 1024 points are a radix-2 Stockham by one wave, in place in a per-wave LDS buffer
// (every lane holds its stage inputs in registers across the exchange); H = 1024 uses fft1024_wave.
#pragma once
#include <vector>

#include "gemm.hip.h"
#include "signal.hip.h"

namespace stts {

// generate_pcph with hop h (see pcph_prep_kernel / pcph_kernel; the reference binds the sample rate to 24000 whatever model.yml says,
// models/generator.py:372)
__global__ void __launch_bounds__(256) pcph_prep_geom_kernel(const float* __restrict__ f0, const int* __restrict__ seg_off, int hop,
                                                             double* __restrict__ prefix, float* __restrict__ stats) {
  __shared__ double part[256];
  __shared__ float mn[256];
  __shared__ int anyv[256];
  const int u = blockIdx.x;
  const int lo = seg_off[u], n = seg_off[u + 1] - lo;
  const int per = (n + 255) / 256;
  const int a = threadIdx.x * per, b = min(n, a + per);
  double s = 0.0;
  float m = INFINITY;
  int av = 0;
  for (int j = a; j < b; ++j) {
    const float f = f0[lo + j];
    s += (double)hop * ((double)f / (double)kSampleRate);
    if (f > 20.0f) m = fminf(m, f);
    if (f > 10.0f) av = 1;
  }
  part[threadIdx.x] = s;
  mn[threadIdx.x] = m;
  anyv[threadIdx.x] = av;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    float mm = INFINITY;
    int aa = 0;
    for (int i = 0; i < 256; ++i) {
      const double t = part[i];
      part[i] = run;
      run += t;
      mm = fminf(mm, mn[i]);
      aa |= anyv[i];
    }
    stats[2 * u] = mm;
    stats[2 * u + 1] = (float)aa;
  }
  __syncthreads();
  double run = part[threadIdx.x];
  for (int j = a; j < b; ++j) {
    prefix[lo + j] = run;
    run += (double)hop * ((double)f0[lo + j] / (double)kSampleRate);
  }
}

__global__ void __launch_bounds__(256) pcph_geom_kernel(const float* __restrict__ f0, const int* __restrict__ seg_off, int n_utt, int hop, int half_nfft,
                                                        const double* __restrict__ prefix, const float* __restrict__ stats,
                                                        const float* __restrict__ noise, const float* __restrict__ init_phase, int batch_scope,
                                                        float* __restrict__ out, int* __restrict__ err) {
  const int u = blockIdx.y;
  const int lo = seg_off[u], nfr = seg_off[u + 1] - lo;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (long)nfr * hop <= half_nfft) atomicOr(err, 4);  // too short for the reflect pad
  float mnf = stats[2 * u];
  int anyv = stats[2 * u + 1] > 0.5f;
  if (batch_scope) {
    for (int v = threadIdx.x & 63; v < n_utt; v += 64) {
      mnf = fminf(mnf, stats[2 * v]);
      anyv |= stats[2 * v + 1] > 0.5f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mnf = fminf(mnf, __shfl_xor(mnf, o, 64));
      anyv |= __shfl_xor(anyv, o, 64);
    }
  }
  int K = 0;
  if (anyv) {
    if (isinf(mnf)) {
      if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(err, 1);
      K = 16;
    } else {
      K = min(16, (int)(12000.0 / (double)mnf));
    }
  }
  const double ph0 = (double)init_phase[0];
  const long nsamp = (long)nfr * hop, base = (long)lo * hop;
  for (long sidx = (long)blockIdx.x * 256 + threadIdx.x; sidx < nsamp; sidx += (long)gridDim.x * 256) {
    const int j = (int)(sidx / hop), i = (int)(sidx % hop);
    const float f = f0[lo + j];
    float val = 0.01f * noise[base + sidx];
    if (f > 10.0f && K > 0) {
      const double rad = ph0 + prefix[lo + j] + (double)(i + 1) * ((double)f / (double)kSampleRate);
      const float nh = (kSampleRate * 0.5f) / f;
      const float amp = 0.1f * sqrtf(2.0f / nh);
      double s1, c1;
      sincospi(2.0 * (rad - floor(rad)), &s1, &c1);
      const double tc = 2.0 * c1;
      double sp = 0.0, sk = s1;
      float acc = 0.f;
      for (int k = 1; k <= K; ++k) {
        if (f * (float)k <= kSampleRate * 0.5f) acc += (float)sk;
        const double nx = tc * sk - sp;
        sp = sk;
        sk = nx;
      }
      val += amp * acc;
    }
    out[base + sidx] = val;
  }
}

// per-wave LDS buffer (fphys padding, one slot past point H for the Nyquist bin) and waves per block: two waves at H = 2048 (35 KB of fp64
// each: two blocks per CU), four below
template <int LOGH>
struct GeomFft {
  static_assert(LOGH >= 7 && LOGH <= 11, "H = 128 .. 2048 points");
  static constexpr int H = 1 << LOGH;
  static constexpr int kBuf = H + H / 16 + 4;
  static constexpr int kWaves = LOGH == 11 ? 2 : 4;
};

// H-point complex FFT by one wave, radix-2 Stockham autosort, in place in buf (fphys layout, natural order in and out).  Stage Ns:
// butterfly j < H/2, k = j mod Ns: in[j], in[j + H/2] * exp(-+2 pi i k / 2Ns) -> out[2(j - k) + k], out[2(j - k) + k + Ns].
// tw[m] = exp(-2 pi i m / 2H), m < H (the model's n_fft table); the inverse conjugates.
template <typename T2, int LOGH, bool INV>
__device__ __forceinline__ void fft_wave_r2(T2* buf, const double2* __restrict__ tw, int lane) {
  constexpr int H = 1 << LOGH, P = H / 128;  // butterflies per lane and stage
#pragma unroll 1
  for (int Ns = 1; Ns < H; Ns <<= 1) {
    T2 a[P], b[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int j = lane + 64 * q;
      a[q] = buf[fphys(j)];
      b[q] = buf[fphys(j + H / 2)];
    }
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int j = lane + 64 * q, k = j & (Ns - 1);
      const T2 t = Ns == 1 ? b[q] : cmul2(b[q], to_t2<T2>(tw[k * (H / Ns)], INV));
      const int j0 = ((j - k) << 1) + k;
      T2 o;
      o.x = a[q].x + t.x; o.y = a[q].y + t.y; buf[fphys(j0)] = o;
      o.x = a[q].x - t.x; o.y = a[q].y - t.y; buf[fphys(j0 + Ns)] = o;
    }
    wave_lds_fence();
  }
}

// Forward STFT + magnitude / atan2 phase at geometry (2H, win, hop): stft_kernel's arithmetic and output format.  Frame f of
// utterance u covers samples [hop f - H, hop f + H) of the reflect-padded signal; the window occupies [wlo, wlo + win) of it.
// Grid (ceil(max frames / kWaves), n_utt).  Writes columns [0, ld): bins 0..H, zeros beyond.
template <int LOGH>
__global__ void __launch_bounds__(64 * GeomFft<LOGH>::kWaves) stft_geom_kernel(const float* __restrict__ sig, const int* __restrict__ seg_off, int hop,
                                                                               int win, const float* __restrict__ hann,
                                                                               const double2* __restrict__ twiddle, float* __restrict__ spec,
                                                                               float* __restrict__ phase, int ld, int out16) {
  using G = GeomFft<LOGH>;
  constexpr int H = G::H;
  __shared__ double2 bufs[G::kWaves][G::kBuf];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int lo = seg_off[u], nfr = seg_off[u + 1] - lo;
  if (f >= nfr) return;  // whole waves leave: nothing below synchronises across waves
  double2* Z = bufs[wv];
  const int wlo = (2 * H - win) / 2;
  const long L = (long)nfr * hop;
  const float* x = sig + (long)lo * hop;
  auto sample = [&](int p) -> double {
    if (p < wlo || p >= wlo + win) return 0.0;
    long m = (long)f * hop - H + p;
    if (m < 0) m = -m;
    if (m >= L) m = 2 * (L - 1) - m;
    m = m < 0 ? 0 : (m >= L ? L - 1 : m);  // in bounds even for a signal too short to reflect (pcph_geom_kernel raises error bit 4 for it)
    return (double)(x[m] * hann[p - wlo]);  // the product is formed in fp32 like torch.stft's windowing
  };
  if constexpr (LOGH == 10) {
    const FftTw tw = fft_load_tw(twiddle, lane);
    double2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane + 64 * r;
      v[r] = make_double2(sample(2 * n), sample(2 * n + 1));
    }
    fft1024_wave<double2, false>(v, Z, tw, lane);
  } else {
#pragma unroll
    for (int r = 0; r < H / 64; ++r) {
      const int n = lane + 64 * r;
      Z[fphys(n)] = make_double2(sample(2 * n), sample(2 * n + 1));
    }
    wave_lds_fence();
    fft_wave_r2<double2, LOGH, false>(Z, twiddle, lane);
  }
  const long row = lo + f;
  const double2 z0 = Z[0];
  for (int k = lane; k < ld; k += 64) {
    float m = 0.f, p = 0.f;
    if (k <= H) {
      double re, im;
      if (k == 0 || k == H) {
        re = k == 0 ? z0.x + z0.y : z0.x - z0.y;
        im = 0.0;
      } else {
        const double2 a = Z[fphys(k)], b = Z[fphys(H - k)], w = twiddle[k];  // w = exp(-2 pi i k / 2H)
        const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
        const double orr = 0.5 * (a.y + b.y), oi = -0.5 * (a.x - b.x);
        re = er + orr * w.x - oi * w.y;
        im = ei + orr * w.y + oi * w.x;
      }
      const float fr = (float)re, fi = (float)im;
      m = __builtin_amdgcn_sqrtf(fr * fr + fi * fi);
      p = atan2_poly(fi, fr);
    }
    if (out16 == 0) {
      spec[row * ld + k] = m;
      phase[row * ld + k] = p;
    } else if (out16 == 1) {
      reinterpret_cast<__bf16*>(spec)[row * ld + k] = (__bf16)m;
      reinterpret_cast<__bf16*>(phase)[row * ld + k] = (__bf16)p;
    } else {
      reinterpret_cast<_Float16*>(spec)[row * ld + k] = (_Float16)m;
      reinterpret_cast<_Float16*>(phase)[row * ld + k] = (_Float16)p;
    }
  }
}

// Inverse, frames: istft_frames_kernel at geometry (2H, win): frame f in [0, T4] (the last repeats row T4 - 1), X = exp(logamp) e^{i phase}
// over bins 0..H, Hermitian C2R as one H-point complex inverse, 1/H, window.  yw rows of `win` samples; utterance u starts at row
// seg_off[u] + u.  No packed-fp32 instructions (the hazard seen with them is not understood).
template <int LOGH>
__attribute__((target("no-packed-fp32-ops")))
__global__ void __launch_bounds__(64 * GeomFft<LOGH>::kWaves) istft_geom_frames_kernel(const float* __restrict__ logamp, const float* __restrict__ phase,
                                                                                       int ld, const int* __restrict__ seg_off, int win,
                                                                                       const float* __restrict__ hann, const double2* __restrict__ twiddle,
                                                                                       float* __restrict__ yw) {
  using G = GeomFft<LOGH>;
  constexpr int H = G::H, P = H / 64;
  __shared__ float2 bufs[G::kWaves][G::kBuf];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int lo = seg_off[u], nfr = seg_off[u + 1] - lo;
  if (f > nfr) return;
  float2* Z = bufs[wv];
  const long row = lo + min(f, nfr - 1);
  const float* la = logamp + row * ld;
  const float* ph = phase + row * ld;
  for (int k = lane; k <= H; k += 64) {
    const float a = expf(la[k]);
    float sn, cs;
    sincos_unit(ph[k], sn, cs);
    float re = a * cs, im = a * sn;
    if (k == 0 || k == H) im = 0.f;  // a C2R transform ignores them (torch.istft / pocketfft)
    Z[fphys(k)] = make_float2(re, im);
  }
  wave_lds_fence();
  float2 v[P];
#pragma unroll
  for (int r = 0; r < P; ++r) {
    const int k = lane + 64 * r;
    const float2 x = Z[fphys(k)], y = Z[fphys(H - k)];
    const float er = 0.5f * (x.x + y.x), ei = 0.5f * (x.y - y.y);    // E = (X[k] + conj(X[H-k]))/2
    const float dr = 0.5f * (x.x - y.x), di = 0.5f * (x.y + y.y);    // D = (X[k] - conj(X[H-k]))/2
    const float2 w = to_t2<float2>(twiddle[k], false);               // exp(-2 pi i k / 2H); conj(w) = e^{+2 pi i k/N}
    const float orr = dr * w.x + di * w.y, oi = di * w.x - dr * w.y; // O = D * conj(w)
    v[r] = make_float2(er - oi, ei + orr);                           // Z = E + i O
  }
  wave_lds_fence();
  if constexpr (LOGH == 10) {
    const FftTw tw = fft_load_tw(twiddle, lane);
    fft1024_wave<float2, true>(v, Z, tw, lane);
  } else {
#pragma unroll
    for (int r = 0; r < P; ++r) Z[fphys(lane + 64 * r)] = v[r];
    wave_lds_fence();
    fft_wave_r2<float2, LOGH, true>(Z, twiddle, lane);
  }
  const int wlo = (2 * H - win) / 2;
  float* o = yw + (long)(lo + u + f) * win;
  for (int i = lane; i < win; i += 64) {
    const int p = wlo + i;
    const float2 z = Z[fphys(p >> 1)];
    o[i] = ((p & 1) ? z.y : z.x) * (1.0f / H) * hann[i];
  }
}

// Inverse, overlap-add + window-envelope normalisation + centre trim + tanh (istft_ola_kernel at geometry (n_fft, win, hop)): out sample
// s of utterance u (0 <= s < hop T4) is position s + n_fft/2 of the untrimmed signal, i.e. offset t = s + n_fft/2 - wlo inside frame 0's window.
__global__ void __launch_bounds__(256) istft_geom_ola_kernel(const float* __restrict__ yw, const int* __restrict__ seg_off, int hop, int win, int n_fft,
                                                             const float* __restrict__ hann, float* __restrict__ audio) {
  const int u = blockIdx.y;
  const int lo = seg_off[u], nfr = seg_off[u + 1] - lo;
  const long nsamp = (long)nfr * hop;
  const int wlo = (n_fft - win) / 2;
  const float* y = yw + (long)(lo + u) * win;
  for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < nsamp; s += (long)gridDim.x * 256) {
    const long t = s + n_fft / 2 - wlo;
    long f_hi = t / hop;
    if (f_hi > nfr) f_hi = nfr;
    long f_lo = (t - (win - 1) + hop - 1) / hop;
    if (t - (win - 1) < 0) f_lo = 0;
    float acc = 0.f, env = 0.f;
    for (long f = f_lo; f <= f_hi; ++f) {
      const int i = (int)(t - f * hop);
      const float w = hann[i];
      acc += y[f * win + i];
      env += w * w;
    }
    audio[(long)lo * hop + s] = tanhf(acc / env);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The supported geometries (config.geometry in Python states the same rules): n_fft a power of two in [256, 4096], 1 <= win <= n_fft,
// hop a multiple of 4, the overlap-add envelope of Hann(win)^2 at hop / 4 nonzero (NOLA, torch.istft's threshold 1e-11), sample rate > 0.
struct SignalGeom {
  int n_fft = 0, win = 0, h = 0, bins = 0;
  bool generic = false;  // the run-time-geometry kernels of this file (every geometry but 2048 / 1200 / 300, or STTS_SIGNAL_GENERIC=1)
};

inline int signal_geometry(int n_fft, int win, int hop, int sample_rate, bool force_generic, SignalGeom* g) {
  STTS_CHECK(n_fft > 0 && (n_fft & (n_fft - 1)) == 0, "n_fft %d is not a power of two", n_fft);
  STTS_CHECK(n_fft >= 256 && n_fft <= 4096, "n_fft %d is outside [256, 4096]", n_fft);
  STTS_CHECK(win >= 1 && win <= n_fft, "win_length %d is outside [1, n_fft = %d]", win, n_fft);
  STTS_CHECK(hop > 0 && hop % 4 == 0, "hop_length %d is not a positive multiple of 4 (the vocoder runs at hop / 4)", hop);
  STTS_CHECK(sample_rate > 0, "sample_rate %d is not positive", sample_rate);
  const int h = hop / 4, wlo = (n_fft - win) / 2;
  std::vector<double> env(h, 0.0);
  for (int i = 0; i < win; ++i) {
    const float w = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / win));
    env[(wlo + i) % h] += (double)w * w;
  }
  double lowest = env[0];
  for (double e : env) lowest = std::min(lowest, e);
  STTS_CHECK(lowest > 1e-11, "NOLA: the overlap-add envelope of Hann(%d)^2 at hop %d reaches %.3g (must exceed 1e-11)", win, h, lowest);
  g->n_fft = n_fft;
  g->win = win;
  g->h = h;
  g->bins = n_fft / 2 + 1;
  g->generic = force_generic || !(n_fft == kNfft && win == kWin && h == kHop);
  return 0;
}

// window + fp64 twiddle table of a geometry: hann[i] = periodic Hann(win), tw[m] = exp(-2 pi i m / n_fft), m < n_fft / 2
inline void signal_tables(int n_fft, int win, std::vector<float>* hann, std::vector<double2>* tw64) {
  hann->resize(win);
  for (int i = 0; i < win; ++i) (*hann)[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / win));
  tw64->resize(n_fft / 2);
  for (int i = 0; i < n_fft / 2; ++i) (*tw64)[i] = make_double2(cos(2.0 * M_PI * i / n_fft), -sin(2.0 * M_PI * i / n_fft));
}

// launchers of the run-time-geometry path (the same stream / argument conventions as the specialised launches in vocoder.hip.h)
// (utterances: n_utt, device row offsets seg, R rows in all, the longest ml rows)
inline int launch_pcph_geom(hipStream_t st, const SignalGeom& g, int n_utt, const int* seg, long R, int ml, const float* pitch, const float* noise,
                            const float* init_phase, int batch_scope, double* prefix, float* stats, float* sig, int* err) {
  STTS_LAUNCH_PROF("pcph_prep_geom_kernel", (size_t)R * 12, pcph_prep_geom_kernel, dim3(n_utt), dim3(256), st, pitch, seg, g.h, prefix, stats);
  STTS_LAUNCH_PROF("pcph_geom_kernel", (size_t)R * g.h * 8, pcph_geom_kernel, dim3(std::min(1024, ceil_div(ml * g.h, 256)), n_utt), dim3(256), st,
                   pitch, seg, n_utt, g.h, g.n_fft / 2, prefix, stats, noise, init_phase, batch_scope, sig, err);
  return 0;
}

inline int launch_stft_geom(hipStream_t st, const SignalGeom& g, int n_utt, const int* seg, long R, int ml, const float* sig, const float* hann,
                            const double2* tw64, float* spec, float* phase, int ld, int out16) {
  const size_t bytes = (size_t)R * (g.h + 2 * g.bins) * 4;
#define STTS_STFT_GEOM(LG)                                                                                                                            \
  STTS_LAUNCH_PROF("stft_geom_kernel", bytes, stft_geom_kernel<LG>, dim3(ceil_div(ml, GeomFft<LG>::kWaves), n_utt), dim3(64 * GeomFft<LG>::kWaves), \
                   st, sig, seg, g.h, g.win, hann, tw64, spec, phase, ld, out16)
  switch (g.n_fft) {
    case 256: STTS_STFT_GEOM(7); break;
    case 512: STTS_STFT_GEOM(8); break;
    case 1024: STTS_STFT_GEOM(9); break;
    case 2048: STTS_STFT_GEOM(10); break;
    case 4096: STTS_STFT_GEOM(11); break;
    default: return fail("stft: n_fft %d not instantiated", g.n_fft);
  }
#undef STTS_STFT_GEOM
  return 0;
}

inline int launch_istft_geom(hipStream_t st, const SignalGeom& g, int n_utt, const int* seg, long R, int ml, const float* la, const float* ph, int ld,
                             const float* hann, const double2* tw64, float* yw, float* audio) {
#define STTS_ISTFT_GEOM(LG)                                                                                                                           \
  STTS_LAUNCH_PROF("istft_geom_frames_kernel", (size_t)R * 2 * g.bins * 4, istft_geom_frames_kernel<LG>, dim3(ceil_div(ml + 1, GeomFft<LG>::kWaves), n_utt), \
                   dim3(64 * GeomFft<LG>::kWaves), st, la, ph, ld, seg, g.win, hann, tw64, yw)
  switch (g.n_fft) {
    case 256: STTS_ISTFT_GEOM(7); break;
    case 512: STTS_ISTFT_GEOM(8); break;
    case 1024: STTS_ISTFT_GEOM(9); break;
    case 2048: STTS_ISTFT_GEOM(10); break;
    case 4096: STTS_ISTFT_GEOM(11); break;
    default: return fail("istft: n_fft %d not instantiated", g.n_fft);
  }
#undef STTS_ISTFT_GEOM
  STTS_LAUNCH_PROF("istft_geom_ola_kernel", (size_t)R * g.h * 4, istft_geom_ola_kernel, dim3(std::min(1024, ceil_div(ml * g.h, 256)), n_utt), dim3(256), st,
                   yw, seg, g.h, g.win, g.n_fft, hann, audio);
  return 0;
}

}  // namespace stts

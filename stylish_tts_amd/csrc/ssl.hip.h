// AdaptiveHubert (train/models/ssl.py:16-31): the transformers HuBERT graph in eval mode (feat_extract_norm "group", post-LN encoder,
// no conv bias, exact GELU) followed by F.interpolate(mode="nearest", size=time_dim), on packed waveforms with sample offsets.
//   feature extractor   conv0 (1 -> C0, k0, s0) + per-utterance per-channel GroupNorm over time + GELU  : ssl_conv0_kernel, ssl_gn_* kernels
//                       convs 1 .. n-1 (k, stride s, no bias) + GELU                                    : conv_gemm_f32 on a strided row view
//   feature projection  LayerNorm(C) -> Linear(C -> hidden)                                             : ssl_ln_gather_kernel, conv_gemm_f32
//   positional conv     grouped Conv1d (weight norm over dim 2, folded in double), drop the last frame
//                       of an even kernel, GELU, + hidden                                               : ssl_pos_conv_kernel (f32 matrix cores)
//   encoder             LayerNorm, then post-LN layers: q|k|v, attention, out + residual, LN, FFN, LN    : conv_gemm_f32, attention_mfma_kernel
//   rate conversion     nearest rows (torch's float index rule) into packed feats rows                  : ssl_nearest_rows_kernel
// Everything runs fp32 whatever stts_set_precision chose.  The dense contractions (convs 1 .. n-1, projection, q|k|v, out, FFN) run the split-fp32
// form on the bf16 matrix cores (gemm.hip.h PREC_X3; the f32 matrix cores on an STTS_PREC_F32_NATIVE engine), always on the 128 x 128 tile whose 16
// waves are 8 positions x 2 K-groups, with no block split-K: one k-ordered chain over K = 1536 .. 3072 rounds 3.3 - 4.3 x what the reference's blocked
// CPU sums do (measured against float64, both forms alike), two chains of K / 2 summed once 1.5 - 2.9 x.  The positional conv and the attention run on
// the f32 matrix cores (v_mfma_f32_16x16x4_f32 / 32x32x2).  One tile for every call and fixed-order statistics over the utterance's own rows make an
// utterance's features the same bit for bit alone and packed with others.
//
// Strided convs without an im2col buffer: on time-major rows [frames, C] a conv of kernel k and stride s is a plain contraction over the
// row VIEW with leading dimension s * C and k * C input columns (output row r reads k * C contiguous floats from float r * s * C).  For
// that, utterance u's rows of level i start at row cap[u] * D_i, D_i the product of the later strides, with cap[u] the smallest row
// count of the last level whose multiples hold every level of the utterance; the few rows between an utterance's frames and its
// capacity are computed from finite filler and never read by a real frame.
// Included by api.hip after hubert.hip.h.
#pragma once

namespace stts {

constexpr int kSslMaxConv = 8;
constexpr int kSslMaxLayers = 48;
constexpr int kSslT0 = 64;  // frames of conv0 per block (statistics chunk)

struct SslDims {
  int hidden = 0, layers = 0, heads = 0, inter = 0, n_conv = 0;
  int conv_dim[kSslMaxConv] = {}, conv_k[kSslMaxConv] = {}, conv_s[kSslMaxConv] = {};
  int pos_k = 0, pos_groups = 0;
  float eps = 1e-5f;
};

struct SslW {
  bool ready = false;
  SslDims d;
  float *w0 = nullptr, *gn_g = nullptr, *gn_b = nullptr;  // conv0 tap-major [k0][C0]; GroupNorm affine
  PackedConv conv[kSslMaxConv];                            // layers 1 .. n_conv - 1 as one-tap contractions over k * cin columns
  float *fp_g = nullptr, *fp_b = nullptr;
  PackedConv proj;
  float *pos_w = nullptr, *pos_b = nullptr;  // folded, [group][tap][cin / groups][cout / groups]
  float *enc_g = nullptr, *enc_b = nullptr;
  struct Layer {
    PackedConv qkv, o, f1, f2;
    float *g1, *b1, *g2, *b2;
  } layer[kSslMaxLayers];
};

// frames after the whole feature extractor, 0 when the utterance is too short for it (the reference raises there)
inline long ssl_frames_host(const SslDims& d, long samples) {
  long n = samples;
  for (int i = 0; i < d.n_conv; ++i) {
    if (n < d.conv_k[i]) return 0;
    n = (n - d.conv_k[i]) / d.conv_s[i] + 1;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------ geometry
struct SslGeom {
  int n_conv;
  int k[kSslMaxConv], s[kSslMaxConv], D[kSslMaxConv];  // D[i]: product of the strides after layer i
};

// per-utterance lengths of every level and the capacity of the last one (host and device run the same integer code)
__host__ __device__ inline int ssl_levels(const SslGeom& g, int samples, int* len) {
  int n = samples, cap = 0;
  for (int i = 0; i < g.n_conv; ++i) {
    n = n < g.k[i] ? 0 : (n - g.k[i]) / g.s[i] + 1;
    len[i] = n;
    const int need = (n + g.D[i] - 1) / g.D[i];
    cap = need > cap ? need : cap;
  }
  return cap;
}

// tab: [0 .. n] capacity offsets of the last level, [n + 1 .. 2n + 1] frame offsets (packed), then (n_conv - 1) arrays of n + 1 offsets of levels 0 ..
// n_conv - 2 ... laid out as tab[(2 + i) * (n + 1) + u] = cap_off[u] * D[i]; one thread (n_utt is small)
__global__ void ssl_offsets_kernel(SslGeom g, const int* __restrict__ samp_off, int n_utt, int* __restrict__ tab) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int n1 = n_utt + 1;
  int cap = 0, fr = 0;
  for (int u = 0; u <= n_utt; ++u) {
    tab[u] = cap;
    tab[n1 + u] = fr;
    for (int i = 0; i + 1 < g.n_conv; ++i) tab[(2 + i) * n1 + u] = cap * g.D[i];
    if (u < n_utt) {
      int len[kSslMaxConv];
      cap += ssl_levels(g, samp_off[u + 1] - samp_off[u], len);
      fr += len[g.n_conv - 1];
    }
  }
}

// ------------------------------------------------------------------------------------------------ layer 0
// conv0 of one utterance chunk: y[t][c] = sum_j w[j][c] x[s0 t + j] (taps in order), raw output rows + per-chunk per-channel sums in double
// (sum and sum of squares of fp32 values: exact enough that E[y^2] - mean^2 formed in double keeps 30+ bits).  Rows between the utterance's
// frames and its capacity are written as zeros.  grid (ceil(max cap0 / kSslT0), n_utt), block 256: thread = channels c, c + 256, ...
template <int K0>
__global__ void __launch_bounds__(256) ssl_conv0_kernel(const float* __restrict__ wave, const int* __restrict__ samp_off, const int* __restrict__ off0,
                                                        const float* __restrict__ W, int C0, int s0, float* __restrict__ Y, double* __restrict__ part, int nchunk) {
  extern __shared__ float xs[];  // s0 * kSslT0 + K0 samples
  const int u = blockIdx.y, chunk = blockIdx.x;
  const int lo = samp_off[u], ns = samp_off[u + 1] - lo;
  const int r0 = off0[u], cap0 = off0[u + 1] - r0;
  const int len0 = ns < K0 ? 0 : (ns - K0) / s0 + 1;
  const int t0 = chunk * kSslT0;
  if (t0 >= cap0) return;
  const int nt = min(kSslT0, cap0 - t0);      // rows this block writes
  const int nv = max(0, min(kSslT0, len0 - t0));  // of which real frames
  const int need = s0 * (kSslT0 - 1) + K0;
  for (int i = threadIdx.x; i < need; i += 256) {
    const int p = s0 * t0 + i;
    xs[i] = p < ns ? wave[lo + p] : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C0; c += 256) {
    float w[K0];
#pragma unroll
    for (int j = 0; j < K0; ++j) w[j] = W[j * C0 + c];
    double s = 0.0, ss = 0.0;
    float* y = Y + (long)(r0 + t0) * C0 + c;
    for (int t = 0; t < nt; ++t) {
      float a = 0.f;
      if (t < nv) {
#pragma unroll
        for (int j = 0; j < K0; ++j) a = fmaf(w[j], xs[s0 * t + j], a);
        s += (double)a;
        ss += (double)a * (double)a;
      }
      y[(long)t * C0] = a;
    }
    if (chunk < nchunk) {
      double* p = part + (((long)u * nchunk + chunk) * 2) * C0 + c;
      p[0] = s;
      p[C0] = ss;
    }
  }
}

// chunk sums in chunk order -> stats[u][0][c] = mean, stats[u][1][c] = 1 / sqrt(var + eps) (biased variance, as GroupNorm); grid (ceil(C0 / 256), n_utt)
__global__ void __launch_bounds__(256) ssl_gn_stats_kernel(const double* __restrict__ part, int nchunk, const int* __restrict__ samp_off, int k0, int s0, int C0,
                                                           float eps, float* __restrict__ stats) {
  const int u = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C0) return;
  const int ns = samp_off[u + 1] - samp_off[u];
  const int len0 = ns < k0 ? 0 : (ns - k0) / s0 + 1;
  const int used = (len0 + kSslT0 - 1) / kSslT0;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < used && k < nchunk; ++k) {
    const double* p = part + (((long)u * nchunk + k) * 2) * C0 + c;
    s += p[0];
    ss += p[C0];
  }
  const double n = (double)max(len0, 1);
  const double mean = s / n;
  const double var = fmax(ss / n - mean * mean, 0.0);
  stats[((long)u * 2) * C0 + c] = (float)mean;
  stats[((long)u * 2 + 1) * C0 + c] = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// y = gelu((y - mean) * rstd * gamma + beta) in place over the utterance's real frames; grid (ceil(max len0 * C0 / 4 / 256), n_utt)
__global__ void __launch_bounds__(256) ssl_gn_apply_kernel(float* __restrict__ Y, const int* __restrict__ off0, const int* __restrict__ samp_off, int k0, int s0,
                                                           int C0, const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int u = blockIdx.y;
  const int ns = samp_off[u + 1] - samp_off[u];
  const int len0 = ns < k0 ? 0 : (ns - k0) / s0 + 1;
  const int c4n = C0 / 4;
  const long total = (long)len0 * c4n;
  const float* mean = stats + ((long)u * 2) * C0;
  const float* rstd = mean + C0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4;
    float4* p = reinterpret_cast<float4*>(Y + ((long)off0[u] + i / c4n) * C0 + c);
    float4 v = *p;
    v.x = gelu_erf((v.x - mean[c]) * rstd[c] * gamma[c] + beta[c]);
    v.y = gelu_erf((v.y - mean[c + 1]) * rstd[c + 1] * gamma[c + 1] + beta[c + 1]);
    v.z = gelu_erf((v.z - mean[c + 2]) * rstd[c + 2] * gamma[c + 2] + beta[c + 2]);
    v.w = gelu_erf((v.w - mean[c + 3]) * rstd[c + 3] * gamma[c + 3] + beta[c + 3]);
    *p = v;
  }
}

// ------------------------------------------------------------------------------------------------ row kernels
// LayerNorm of the real frames of the last conv level (capacity offsets) into packed rows (frame offsets); one wave per row, two passes over
// registers (C <= 2048, C % 4 == 0); optional raw copy of the gathered rows (test tap).  grid (ceil(max_len / 4), n_utt)
__global__ void __launch_bounds__(256) ssl_ln_gather_kernel(const float* __restrict__ X, int ldx, const int* __restrict__ src_off, const int* __restrict__ dst_off, int C,
                                                            float eps, const float* __restrict__ g, const float* __restrict__ b, float* __restrict__ Y, int ldy,
                                                            float* __restrict__ raw, int ld_raw) {
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = dst_off[u + 1] - dst_off[u];
  if (t >= n) return;
  const float* x = X + (long)(src_off[u] + t) * ldx;
  const long orow = dst_off[u] + t;
  float4 v[8];
  const int nv = C / 4;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = lane + i * 64;
    v[i] = q < nv ? *reinterpret_cast<const float4*>(x + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += v[i].x + v[i].y + v[i].z + v[i].w;
    if (raw && q < nv) *reinterpret_cast<float4*>(raw + orow * ld_raw + q * 4) = v[i];
  }
  const float mean = wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (lane + i * 64 < nv) {
      const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      ss += a * a + bb * bb + c * c + d * d;
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = lane + i * 64;
    if (q < nv) {
      const float4 gg = *reinterpret_cast<const float4*>(g + q * 4), bv = *reinterpret_cast<const float4*>(b + q * 4);
      float4 y;
      y.x = (v[i].x - mean) * rstd * gg.x + bv.x;
      y.y = (v[i].y - mean) * rstd * gg.y + bv.y;
      y.z = (v[i].z - mean) * rstd * gg.z + bv.z;
      y.w = (v[i].w - mean) * rstd * gg.w + bv.w;
      *reinterpret_cast<float4*>(Y + orow * ldy + q * 4) = y;
    }
  }
}

// F.interpolate(mode="nearest", size = n) over the utterance's frames: src = min(floor(j * (float)L / n), L - 1), torch's float rule
__device__ __forceinline__ int ssl_nearest_src(int j, int L, int n) {
  const float scale = (float)L / (float)n;
  return min((int)floorf((float)j * scale), L - 1);
}

// out[off_T[u] + j][0 .. C) = x[off_F[u] + src(j)][0 .. C), pad columns [C, ld_out) zero; grid (ceil(max time_dim * ld_out / 4 / 256), n_utt)
__global__ void __launch_bounds__(256) ssl_nearest_rows_kernel(const float* __restrict__ X, int ldx, int C, const int* __restrict__ off_F, const int* __restrict__ off_T,
                                                               float* __restrict__ out, int ld_out) {
  const int u = blockIdx.y;
  const int L = off_F[u + 1] - off_F[u], n = off_T[u + 1] - off_T[u];
  const int c4n = ld_out / 4;
  const long total = (long)n * c4n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int j = (int)(i / c4n), c = (int)(i % c4n) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) v = *reinterpret_cast<const float4*>(X + (long)(off_F[u] + ssl_nearest_src(j, L, n)) * ldx + c);
    *reinterpret_cast<float4*>(out + (long)(off_T[u] + j) * ld_out + c) = v;
  }
}

// ------------------------------------------------------------------------------------------------ positional conv
// Grouped Conv1d(hidden, hidden, k, padding k / 2, groups) on packed rows, zero padded at the utterance's own edges, the extra last frame of an
// even kernel dropped: y[t][g Co + o] = gelu(b + sum_{tap, c} w[g][tap][c][o] x[t + tap - k / 2][g Ci + c]) + x[t][g Co + o].
// Implicit GEMM on v_mfma_f32_16x16x4_f32: a block is 32 frames of one (utterance, group); its 4 waves each take a quarter of the taps for the whole
// 32 x Co tile (2 x NT accumulators of 16 x 16), reading the frames from an LDS window of 32 + k - 1 rows and the weights from global memory
// (lane l: A[frame l & 15][channel 4 q + (l >> 4)], B[channel 4 q + (l >> 4)][o = l & 15]); the four partial tiles are summed through LDS in wave
// order.  An output is a fixed sequence of fp32 operations of its own utterance's rows.  grid (ceil(max_len / 32), groups, n_utt), block 256.
template <int NT>
__global__ void __launch_bounds__(256) ssl_pos_conv_kernel(const float* __restrict__ X, int ldx, const int* __restrict__ off, const float* __restrict__ W,
                                                           const float* __restrict__ bias, int K, int Ci, float* __restrict__ Y, int ldy) {
  extern __shared__ float sm[];
  constexpr int Co = NT * 16;
  const int u = blockIdx.z, grp = blockIdx.y;
  const int lo = off[u], n = off[u + 1] - lo;
  const int t0 = blockIdx.x * 32;
  if (t0 >= n) return;
  const int S = Ci + 1;        // LDS row stride (odd: the 16 frames of a fragment read fall in distinct banks)
  const int win = 32 + K - 1;  // window rows: frames t0 - K / 2 .. t0 + 31 + (K - 1 - K / 2)
  const int pad = K / 2;
  for (int i = threadIdx.x; i < win * Ci; i += 256) {
    const int r = i / Ci, c = i % Ci;
    const int t = t0 - pad + r;
    sm[r * S + c] = (t >= 0 && t < n) ? X[(long)(lo + t) * ldx + grp * Ci + c] : 0.f;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int tper = (K + 3) / 4, tap_lo = wv * tper, tap_hi = min(K, tap_lo + tper);
  f32x4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wg = W + (long)grp * K * Ci * Co;
  for (int tap = tap_lo; tap < tap_hi; ++tap) {
    const float* wt = wg + (long)tap * Ci * Co + lq * Co + l15;
    const float* xa = sm + (l15 + tap) * S + lq;
    for (int c0 = 0; c0 < Ci; c0 += 4) {
      const float a0 = xa[c0], a1 = xa[16 * S + c0];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float bv = wt[(long)c0 * Co + j * 16];
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the window is dead: its LDS becomes the partial tiles [wave][frame 32][Co]
  float* red = sm;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wv * 32 + m * 16 + lq * 4 + r) * Co + j * 16 + l15] = acc[m][j][r];
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * Co; i += 256) {
    const int r = i / Co, o = i % Co;
    const int t = t0 + r;
    if (t >= n) continue;
    float s = red[i];
    s += red[32 * Co + i];
    s += red[2 * 32 * Co + i];
    s += red[3 * 32 * Co + i];
    const int col = grp * Co + o;
    Y[(long)(lo + t) * ldy + col] = gelu_erf(s + bias[col]) + X[(long)(lo + t) * ldx + col];
  }
}

// ------------------------------------------------------------------------------------------------ packing
inline int ssl_upload_pair(stts_ctx* c, const std::string& p, int n, float** g, float** b) {
  STTS_GET(tg, p + ".weight");
  STTS_GET(tb, p + ".bias");
  STTS_CHECK((int)tg->data.size() == n && (int)tb->data.size() == n, "%s: expected weight and bias of %d elements", p.c_str(), n);
  STTS_TRY(dev_upload(c, tg->data, g));
  return dev_upload(c, tb->data, b);
}

inline int ssl_pack_linear(stts_ctx* c, const std::string& p, int out_n, int in_n, PackedConv* o) {
  STTS_GET(w, p + ".weight");
  STTS_CHECK(w->shape.size() == 2 && w->shape[0] == out_n && w->shape[1] == in_n, "%s.weight: expected [%d, %d]", p.c_str(), out_n, in_n);
  return pack_plain(c, p, true, 0, in_n, o);
}

// q | k | v stacked along the outputs (N = 3 hidden)
inline int ssl_pack_qkv(stts_ctx* c, const std::string& a, int C, PackedConv* out) {
  HostTensor w, b;
  const char* names[3] = {"q_proj", "k_proj", "v_proj"};
  for (int i = 0; i < 3; ++i) {
    STTS_GET(wi, a + names[i] + ".weight");
    STTS_GET(bi, a + names[i] + ".bias");
    STTS_CHECK(wi->shape.size() == 2 && wi->shape[0] == C && wi->shape[1] == C && (int)bi->data.size() == C, "%s%s: expected a Linear(%d, %d)", a.c_str(), names[i], C, C);
    w.data.insert(w.data.end(), wi->data.begin(), wi->data.end());
    b.data.insert(b.data.end(), bi->data.begin(), bi->data.end());
  }
  w.shape = {3 * C, C, 1};
  b.shape = {3 * C};
  return pack_rows(c, w, &b, plain_rows(3 * C), 0, C, round_up(C, 32), 3 * C, out);
}

// weight norm over dim 2 (gain [1, 1, k]: one norm per tap over the [cout, cin / groups] slice), folded in double
inline void ssl_fold_pos_weight(const HostTensor& g, const HostTensor& v, std::vector<float>* w) {
  const long co = v.shape[0], ci = v.shape[1], k = v.shape[2];
  w->resize(v.data.size());
  for (long t = 0; t < k; ++t) {
    double s = 0;
    for (long i = 0; i < co * ci; ++i) s += (double)v.data[i * k + t] * (double)v.data[i * k + t];
    const double scale = (double)g.data[t] / sqrt(s);
    for (long i = 0; i < co * ci; ++i) (*w)[i * k + t] = (float)((double)v.data[i * k + t] * scale);
  }
}

// p: the key prefix of the transformers model ("hubert.model." for AdaptiveHubert; WavLM, whose front end and layer body are the same, has its own)
inline int finalize_ssl(stts_ctx* c, const SslDims& d, SslW* M, const std::string& p = "hubert.model.") {
  *M = SslW();
  M->d = d;
  STTS_CHECK(d.n_conv >= 1 && d.n_conv <= kSslMaxConv, "ssl: conv layers %d outside [1, %d]", d.n_conv, kSslMaxConv);
  STTS_CHECK(d.layers >= 1 && d.layers <= kSslMaxLayers, "ssl: num_hidden_layers %d outside [1, %d]", d.layers, kSslMaxLayers);
  STTS_CHECK(d.hidden > 0 && d.hidden % 32 == 0 && d.hidden <= 2048, "ssl: hidden_size %d must be a multiple of 32, at most 2048", d.hidden);
  STTS_CHECK(d.heads > 0 && d.hidden % d.heads == 0 && attn_mfma_kc(d.hidden / d.heads), "ssl: hidden_size / num_attention_heads = %d is not a head size of the matrix-core attention (16 / 32 / 40 / 64 / 96 / 128 / 160)",
             d.heads > 0 ? d.hidden / d.heads : 0);
  STTS_CHECK(d.inter > 0 && d.inter % 32 == 0, "ssl: intermediate_size %d must be a multiple of 32", d.inter);
  for (int i = 0; i < d.n_conv; ++i) {
    STTS_CHECK(d.conv_dim[i] > 0 && d.conv_dim[i] % 32 == 0 && d.conv_dim[i] <= 2048, "ssl: conv_dim[%d] = %d must be a multiple of 32, at most 2048", i, d.conv_dim[i]);
    STTS_CHECK(d.conv_s[i] >= 1 && d.conv_k[i] >= d.conv_s[i] && d.conv_k[i] <= 16, "ssl: conv_kernel[%d] = %d / conv_stride[%d] = %d: need stride <= kernel <= 16", i, d.conv_k[i], i, d.conv_s[i]);
  }
  STTS_CHECK(d.conv_k[0] == 10 || d.conv_k[0] == 5 || d.conv_k[0] == 3, "ssl: conv_kernel[0] = %d (the layer-0 kernel is built for 10, 5 and 3 taps)", d.conv_k[0]);
  const int G = d.pos_groups;
  STTS_CHECK(G > 0 && d.hidden % G == 0 && (d.hidden / G) % 16 == 0 && d.hidden / G <= 64, "ssl: hidden_size / num_conv_pos_embedding_groups must be 16, 32, 48 or 64");
  STTS_CHECK(d.pos_k >= 1 && d.pos_k <= 256, "ssl: num_conv_pos_embeddings %d outside [1, 256]", d.pos_k);
  // layer 0
  {
    STTS_GET(w, p + "feature_extractor.conv_layers.0.conv.weight");
    const int C0 = d.conv_dim[0], k0 = d.conv_k[0];
    STTS_CHECK(w->shape.size() == 3 && w->shape[0] == C0 && w->shape[1] == 1 && w->shape[2] == k0, "feature_extractor.conv_layers.0.conv.weight: expected [%d, 1, %d]", C0, k0);
    std::vector<float> wt((size_t)k0 * C0);
    for (int ch = 0; ch < C0; ++ch)
      for (int j = 0; j < k0; ++j) wt[(size_t)j * C0 + ch] = w->data[(size_t)ch * k0 + j];
    STTS_TRY(dev_upload(c, wt, &M->w0));
    STTS_TRY(ssl_upload_pair(c, p + "feature_extractor.conv_layers.0.layer_norm", C0, &M->gn_g, &M->gn_b));
  }
  for (int i = 1; i < d.n_conv; ++i) {
    const std::string q = p + "feature_extractor.conv_layers." + std::to_string(i) + ".conv";
    STTS_GET(w, q + ".weight");
    const int cin = d.conv_dim[i - 1];
    STTS_CHECK(w->shape.size() == 3 && w->shape[0] == d.conv_dim[i] && w->shape[1] == cin && w->shape[2] == d.conv_k[i], "%s.weight: expected [%d, %d, %d]", q.c_str(),
               d.conv_dim[i], cin, d.conv_k[i]);
    STTS_CHECK(!find(c, q + ".bias"), "%s.bias is present: conv_bias must be false", q.c_str());
    STTS_TRY(pack_plain(c, q, false, 0, cin, &M->conv[i]));
    // [cout][tap][cin] with cin % 32 == 0 is [cout][1][k * cin] as it stands: one tap over the k * cin columns of the strided row view
    M->conv[i].kc = d.conv_k[i] * cin;
    M->conv[i].ntaps = 1;
    M->conv[i].cin_real = d.conv_k[i] * cin;
  }
  const int CL = d.conv_dim[d.n_conv - 1], H = d.hidden;
  STTS_TRY(ssl_upload_pair(c, p + "feature_projection.layer_norm", CL, &M->fp_g, &M->fp_b));
  STTS_TRY(ssl_pack_linear(c, p + "feature_projection.projection", H, CL, &M->proj));
  {
    const std::string q = p + "encoder.pos_conv_embed.conv";
    const HostTensor* g = find(c, q + ".parametrizations.weight.original0");
    const HostTensor* v = find(c, q + ".parametrizations.weight.original1");
    if (!g) { g = find(c, q + ".weight_g"); v = find(c, q + ".weight_v"); }
    STTS_CHECK(g && v, "missing weight '%s.parametrizations.weight.original0/1' (or weight_g / weight_v)", q.c_str());
    const int Ci = H / G;
    STTS_CHECK(v->shape.size() == 3 && v->shape[0] == H && v->shape[1] == Ci && v->shape[2] == d.pos_k, "%s: expected a weight of [%d, %d, %d]", q.c_str(), H, Ci, d.pos_k);
    STTS_CHECK((int)g->data.size() == d.pos_k, "%s: the weight-norm gain must have one element per tap (%d; weight norm over dim 2)", q.c_str(), d.pos_k);
    std::vector<float> w;
    ssl_fold_pos_weight(*g, *v, &w);
    std::vector<float> pw((size_t)H * Ci * d.pos_k);
    for (int gi = 0; gi < G; ++gi)
      for (int t = 0; t < d.pos_k; ++t)
        for (int ci = 0; ci < Ci; ++ci)
          for (int o = 0; o < Ci; ++o) pw[(((size_t)gi * d.pos_k + t) * Ci + ci) * Ci + o] = w[((size_t)(gi * Ci + o) * Ci + ci) * d.pos_k + t];
    STTS_TRY(dev_upload(c, pw, &M->pos_w));
    STTS_GET(b, q + ".bias");
    STTS_CHECK((int)b->data.size() == H, "%s.bias: expected %d elements", q.c_str(), H);
    STTS_TRY(dev_upload(c, b->data, &M->pos_b));
  }
  STTS_TRY(ssl_upload_pair(c, p + "encoder.layer_norm", H, &M->enc_g, &M->enc_b));
  for (int i = 0; i < d.layers; ++i) {
    const std::string l = p + "encoder.layers." + std::to_string(i) + ".";
    SslW::Layer& L = M->layer[i];
    STTS_TRY(ssl_pack_qkv(c, l + "attention.", H, &L.qkv));
    STTS_TRY(ssl_pack_linear(c, l + "attention.out_proj", H, H, &L.o));
    STTS_TRY(ssl_pack_linear(c, l + "feed_forward.intermediate_dense", d.inter, H, &L.f1));
    STTS_TRY(ssl_pack_linear(c, l + "feed_forward.output_dense", H, d.inter, &L.f2));
    STTS_TRY(ssl_upload_pair(c, l + "layer_norm", H, &L.g1, &L.b1));
    STTS_TRY(ssl_upload_pair(c, l + "final_layer_norm", H, &L.g2, &L.b2));
  }
  M->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ forward
inline SslGeom ssl_geom(const SslDims& d) {
  SslGeom g{};
  g.n_conv = d.n_conv;
  for (int i = 0; i < d.n_conv; ++i) { g.k[i] = d.conv_k[i]; g.s[i] = d.conv_s[i]; }
  int D = 1;
  for (int i = d.n_conv - 1; i >= 0; --i) { g.D[i] = D; D *= d.conv_s[i]; }
  return g;
}

// one dense contraction, whole (no block split-K)
inline int ssl_gemm(hipStream_t st, const Seg& s, const float* X, int ldx, const PackedConv& w, float* Y, int ldy, int act, const float* R = nullptr, int ldr = 0) {
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, X, ldx, 0, w, 0);
  a.N = w.N; a.bias = w.bias; a.Y = Y; a.ldy = ldy; a.act = act; a.R = R; a.ldr = ldr;
  // the 128 x 128 tile whose 16 waves are 8 positions x 2 K-groups, for every call: two accumulator chains of K / 2 terms summed once round less than one
  // chain of K terms (tests/test_hip_ssl.py judges every layer against float64), and one tile for every batch keeps an utterance's bits
  const int tile = 8;
  return launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, s.max_len(), tile);
}

struct SslTaps {  // optional outputs for the tests (null: skipped): packed rows at the frame offsets, except conv0 at `conv0_off` rows
  float* conv0 = nullptr;    // [rows of level 0 incl. capacity, C0]
  int32_t* conv0_off = nullptr;  // [n_utt + 1] device: first row of every utterance in conv0
  float* conv_last = nullptr;  // [frames, C_last]
  float* proj = nullptr;       // [frames, hidden]
  float* pos = nullptr;        // [frames, hidden] after positional conv + LayerNorm
  float* layers = nullptr;     // [n_layers][frames, hidden]
  float* hidden = nullptr;     // [frames, hidden] the last hidden state before the rate conversion
};

// rows of every level for the host offsets of a call
struct SslPlan {
  std::vector<int> cap_off, fr_off;       // [n_utt + 1]
  std::vector<std::vector<int>> lvl_off;  // [n_conv - 1][n_utt + 1]
  int max_cap0 = 0, max_len0 = 0, max_fr = 0;
};
inline void ssl_plan(const SslDims& d, int n_utt, const int* samp_off, SslPlan* P) {
  const SslGeom g = ssl_geom(d);
  P->cap_off.assign(n_utt + 1, 0);
  P->fr_off.assign(n_utt + 1, 0);
  P->lvl_off.assign(std::max(0, d.n_conv - 1), std::vector<int>(n_utt + 1, 0));
  for (int u = 0; u < n_utt; ++u) {
    int len[kSslMaxConv];
    const int cap = ssl_levels(g, samp_off[u + 1] - samp_off[u], len);
    P->cap_off[u + 1] = P->cap_off[u] + cap;
    P->fr_off[u + 1] = P->fr_off[u] + len[d.n_conv - 1];
    P->max_cap0 = std::max(P->max_cap0, cap * g.D[0]);
    P->max_len0 = std::max(P->max_len0, len[0]);
    P->max_fr = std::max(P->max_fr, len[d.n_conv - 1]);
  }
  for (int i = 0; i + 1 < d.n_conv; ++i)
    for (int u = 0; u <= n_utt; ++u) P->lvl_off[i][u] = P->cap_off[u] * g.D[i];
}

// What a network built on this encoder adds to it (WavLM, wavlm.hip.h); the defaults are HuBERT.
struct SslPlain {
  void carve(Arena&, long /*frames*/) {}                                                  // its own buffers, after the encoder's
  int state(hipStream_t, int /*k*/, const float* /*x*/, const Seg& /*sF*/) { return 0; }  // hidden state k (0: after the encoder LayerNorm) is in x
  // the attention of layer i over q | k | v rows (x: the layer's input)
  int attention(hipStream_t st, int /*i*/, const float* /*x*/, const Seg& sF, const float* qkv, int H, int heads, float* att) {
    // (matrix cores, keys never split over wave groups: the split depends on the longest utterance of the call)
    return run_attention(st, sF, sF, qkv, 3 * H, 0, qkv, 3 * H, H, qkv, 3 * H, 2 * H, att, H, heads, H / heads, nullptr, 0, 3);
  }
};

// The shared graph: feature extractor, projection, positional conv, encoder LayerNorm, post-LN layers.  Leaves the last hidden state in *x_out
// (packed rows at the frame offsets *fr_dev_out, host plan *P); in a dry run it returns after the carving with *x_out null.
template <class Ext>
inline int ssl_encode(const SslW& M, hipStream_t st, int n_utt, const int* samp_off_host, const int* samp_off_dev, const float* wave, const SslTaps* taps, Arena& ws,
                      Ext& ext, SslPlan& P, const float** x_out, const int** fr_dev_out) {
  const SslDims& d = M.d;
  const SslGeom g = ssl_geom(d);
  *x_out = nullptr;
  ssl_plan(d, n_utt, samp_off_host, &P);
  const int n1 = n_utt + 1, C0 = d.conv_dim[0], CL = d.conv_dim[d.n_conv - 1], H = d.hidden;
  const long cap = P.cap_off[n_utt], F = P.fr_off[n_utt];
  int* tab = ws.get<int>((size_t)(d.n_conv + 2) * n1);
  size_t na = 0, nb = 0;
  for (int i = 0; i < d.n_conv; ++i) {
    const size_t n = (size_t)cap * g.D[i] * d.conv_dim[i] + 16 * (size_t)d.conv_dim[i] + 64;
    (i % 2 == 0 ? na : nb) = std::max(i % 2 == 0 ? na : nb, n);
  }
  float* lv[2] = {ws.get<float>(na), ws.get<float>(nb)};
  const int nchunk = ceil_div(std::max(1, P.max_len0), kSslT0);
  double* part = ws.get<double>((size_t)n_utt * nchunk * 2 * C0);
  float* stats = ws.get<float>((size_t)n_utt * 2 * C0);
  float* ln = ws.get<float>(F * CL);
  float* x = ws.get<float>(F * H + 64);
  float* t = ws.get<float>(F * H);
  float* qkv = ws.get<float>(F * 3 * H);
  float* att = ws.get<float>(F * H);
  float* ff = ws.get<float>(F * d.inter);
  ext.carve(ws, F);
  STTS_CHECK(ws.ok, "ssl_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  const int* cap_dev = tab;
  const int* fr_dev = tab + n1;
  hipLaunchKernelGGL(ssl_offsets_kernel, dim3(1), dim3(64), 0, st, g, samp_off_dev, n_utt, tab);
  // ---- layer 0: conv, statistics, normalise + GELU (materialised: 19.6 MB per 3-s utterance, written once and rewritten in place)
  const int* off0 = d.n_conv > 1 ? tab + 2 * n1 : cap_dev;
  {
    const dim3 grid(ceil_div(std::max(1, P.max_cap0), kSslT0), n_utt);
    const size_t shm = (size_t)(d.conv_s[0] * (kSslT0 - 1) + d.conv_k[0]) * sizeof(float);
#define STTS_SSL_CONV0(KK) hipLaunchKernelGGL(ssl_conv0_kernel<KK>, grid, dim3(256), shm, st, wave, samp_off_dev, off0, M.w0, C0, d.conv_s[0], lv[0], part, nchunk)
    if (d.conv_k[0] == 10) STTS_SSL_CONV0(10);
    else if (d.conv_k[0] == 5) STTS_SSL_CONV0(5);
    else STTS_SSL_CONV0(3);
#undef STTS_SSL_CONV0
    hipLaunchKernelGGL(ssl_gn_stats_kernel, dim3(ceil_div(C0, 256), n_utt), dim3(256), 0, st, part, nchunk, samp_off_dev, d.conv_k[0], d.conv_s[0], C0, d.eps, stats);
    const long work = (long)P.max_len0 * (C0 / 4);
    hipLaunchKernelGGL(ssl_gn_apply_kernel, dim3((unsigned)std::max<long>(1, std::min<long>(4096, (work + 255) / 256)), n_utt), dim3(256), 0, st, lv[0], off0, samp_off_dev,
                       d.conv_k[0], d.conv_s[0], C0, stats, M.gn_g, M.gn_b);
    if (taps && taps->conv0) {
      STTS_HIP(hipMemcpyAsync(taps->conv0, lv[0], (size_t)cap * g.D[0] * C0 * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (taps->conv0_off) STTS_HIP(hipMemcpyAsync(taps->conv0_off, off0, n1 * sizeof(int), hipMemcpyDeviceToDevice, st));
    }
  }
  // ---- layers 1 .. n - 1: contractions over the strided row view, GELU in the epilogue
  for (int i = 1; i < d.n_conv; ++i) {
    const bool last = i == d.n_conv - 1;
    const std::vector<int>& oh = last ? P.cap_off : P.lvl_off[i];
    Seg s{n_utt, oh.data(), last ? cap_dev : tab + (2 + i) * n1};
    STTS_TRY(ssl_gemm(st, s, lv[(i - 1) & 1], d.conv_s[i] * d.conv_dim[i - 1], M.conv[i], lv[i & 1], d.conv_dim[i], ACT_GELU));
  }
  const float* feat = lv[(d.n_conv - 1) & 1];
  // ---- feature projection: LayerNorm of the real frames into packed rows, Linear
  Seg sF{n_utt, P.fr_off.data(), fr_dev};
  const dim3 rows4(ceil_div(std::max(1, P.max_fr), 4), n_utt);
  hipLaunchKernelGGL(ssl_ln_gather_kernel, rows4, dim3(256), 0, st, feat, CL, cap_dev, fr_dev, CL, d.eps, M.fp_g, M.fp_b, ln, CL, taps ? taps->conv_last : nullptr, CL);
  STTS_TRY(ssl_gemm(st, sF, ln, CL, M.proj, x, H, ACT_NONE));
  if (taps && taps->proj) STTS_HIP(hipMemcpyAsync(taps->proj, x, F * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  // ---- positional conv + GELU + residual, encoder LayerNorm
  {
    const int Ci = H / d.pos_groups;
    const size_t shm = std::max((size_t)(32 + d.pos_k - 1) * (Ci + 1), (size_t)4 * 32 * Ci) * sizeof(float);
    const dim3 grid(ceil_div(std::max(1, P.max_fr), 32), d.pos_groups, n_utt);
#define STTS_SSL_POS(NT) hipLaunchKernelGGL(ssl_pos_conv_kernel<NT>, grid, dim3(256), shm, st, x, H, fr_dev, M.pos_w, M.pos_b, d.pos_k, Ci, t, H)
    if (Ci == 16) STTS_SSL_POS(1);
    else if (Ci == 32) STTS_SSL_POS(2);
    else if (Ci == 48) STTS_SSL_POS(3);
    else STTS_SSL_POS(4);
#undef STTS_SSL_POS
    STTS_TRY(static_ln(st, t, H, H, F, d.eps, M.enc_g, M.enc_b, x, H, ACT_NONE));
    if (taps && taps->pos) STTS_HIP(hipMemcpyAsync(taps->pos, x, F * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  STTS_TRY(ext.state(st, 0, x, sF));
  // ---- post-LN transformer layers
  for (int i = 0; i < d.layers; ++i) {
    const SslW::Layer& L = M.layer[i];
    STTS_TRY(ssl_gemm(st, sF, x, H, L.qkv, qkv, 3 * H, ACT_NONE));
    STTS_TRY(ext.attention(st, i, x, sF, qkv, H, d.heads, att));
    STTS_TRY(ssl_gemm(st, sF, att, H, L.o, t, H, ACT_NONE, x, H));
    STTS_TRY(static_ln(st, t, H, H, F, d.eps, L.g1, L.b1, x, H, ACT_NONE));
    STTS_TRY(ssl_gemm(st, sF, x, H, L.f1, ff, d.inter, ACT_GELU));
    STTS_TRY(ssl_gemm(st, sF, ff, d.inter, L.f2, t, H, ACT_NONE, x, H));
    STTS_TRY(static_ln(st, t, H, H, F, d.eps, L.g2, L.b2, x, H, ACT_NONE));
    if (taps && taps->layers) STTS_HIP(hipMemcpyAsync(taps->layers + (size_t)i * F * H, x, F * H * sizeof(float), hipMemcpyDeviceToDevice, st));
    STTS_TRY(ext.state(st, i + 1, x, sF));
  }
  if (taps && taps->hidden) STTS_HIP(hipMemcpyAsync(taps->hidden, x, F * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipGetLastError());
  *x_out = x;
  *fr_dev_out = fr_dev;
  return 0;
}

inline int ssl_forward(const SslW& M, hipStream_t st, int n_utt, const int* samp_off_host, const int* samp_off_dev, const float* wave, const Seg& sT, float* feats,
                       int ld_feats, const SslTaps* taps, Arena& ws) {
  SslPlain plain;
  SslPlan P;
  const float* x = nullptr;
  const int* fr_dev = nullptr;
  STTS_TRY(ssl_encode(M, st, n_utt, samp_off_host, samp_off_dev, wave, taps, ws, plain, P, &x, &fr_dev));
  if (!x) return 0;  // a dry run: sized, nothing launched
  const int H = M.d.hidden;
  // ---- rate conversion straight into the packed feature rows
  {
    const long work = (long)sT.max_len() * (ld_feats / 4);
    hipLaunchKernelGGL(ssl_nearest_rows_kernel, dim3((unsigned)std::max<long>(1, std::min<long>(2048, (work + 255) / 256)), n_utt), dim3(256), 0, st, x, H, H, fr_dev,
                       sT.dev, feats, ld_feats);
  }
  STTS_HIP(hipGetLastError());
  return 0;
}

// workspace bytes for these host sample offsets: a dry run of the carving above
inline size_t ssl_workspace_bytes(const SslW& M, int n_utt, const int* samp_off) {
  const Seg none{n_utt, nullptr, nullptr};  // (the time_dim offsets: read after the carving only)
  return dry_run_bytes([&](Arena a) { (void)ssl_forward(M, nullptr, n_utt, samp_off, nullptr, nullptr, none, nullptr, 0, nullptr, a); });
}

}  // namespace stts

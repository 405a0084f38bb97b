// MelStyleEncoder on the engine: spectral-norm folding, the 2-D convolution kernels and the encoder's orchestration.
//   MelStyleEncoder               models/mel_style_encoder.py:120-151 (ResBlk :68-117, DownSample :48-65, LearnedDownSample :8-45)
//   pe_mel_style_encoder          models/models.py:57-62                (STTS_W_PE_MEL_STYLE)
//   cfm_pitch_predictor.spk_emb   models/cfm/cfm_pitch_predictor.py:25-27 (STTS_W_CFM_PITCH)
// Included by api.hip after hubert.hip.h.  Everything here is fp32 on the f32 matrix cores (v_mfma_f32_16x16x4_f32) whatever
// stts_set_precision chose: the 16-bit modes give the same bits as f32 mode.
//
// Layout: channels-last packed rows.  The input of the encoder is the mel [B, 1, F = n_mels, T]; at every
// level the activation of utterance u is the rows (off[u] + t) * F + f, t < T_u, f < F, each row ld(C) = round_up(C, 16) floats with
// the channels contiguous (the pad channels hold zeros).  A 2-D convolution is an implicit GEMM over those rows: M = output positions,
// N = cout, K = k * k * ld(cin) in tap-major order; the operand load gathers the tap's input row and zero-fills the frequency edges and
// the utterance boundaries, so no im2col buffer exists.
#pragma once

namespace stts {

constexpr int kMsBM = 64, kMsBN = 64, kMsBK = 16;  // contraction tile: 4 waves of 32 x 32, K chunk of 16 (one tap, 16 channels)
constexpr int kMsMaxBlocks = 4;
constexpr int kMsMinOut = 5;
// split-K: a contraction with K >= 2 kMsSplitK runs as ceil(K / kMsSplitK) slices whose partial sums are added in slice order by
// ms_splitk_reduce_kernel.  The slice count depends on K only (the weights), never on the batch: the bits stay batch-independent.
constexpr int kMsSplitK = 1024;  // the 5 x 5 valid conv needs 5 x 5 positions after the last downsampling

inline int ms_ld(int c) { return round_up(c, 16); }

// no packed-fp32 instructions in these fp32 kernels (-DSTTS_MS_ALLOW_PACKED builds them with, to measure the rule)
#ifdef STTS_MS_ALLOW_PACKED
#define STTS_MS_NO_PK
#else
#define STTS_MS_NO_PK __attribute__((target("no-packed-fp32-ops")))
#endif

typedef float ms_f32x4 __attribute__((ext_vector_type(4)));  // one 16 x 16 accumulator tile per lane: 4 floats

struct MsConv {  // spectral-norm-folded conv, packed [k * k * ldk][npad] (K row = (dt * k + df) * ldk + ci), bias [cout] or null
  int cout = 0, cin = 0, k = 0, ldk = 0, npad = 0;
  float* w = nullptr;
  float* b = nullptr;
};

struct MsBlockW {
  int cin = 0, cout = 0;
  bool down = false, learned_sc = false;
  MsConv conv1, conv2, sc;                  // sc: conv1x1 (no bias) when cin != cout
  float* dw_w = nullptr;                    // downsample_res: depthwise 3 x 3 stride 2, [c][kF][kT]
  float* dw_b = nullptr;
};

struct MelStyleW {
  bool ready = false;
  int n_mels = 0, c0 = 0, style_dim = 0, n_down = 0, c_last = 0;
  float* w0 = nullptr;  // shared.0: 1 -> c0, [c0][kF][kT]
  float* b0 = nullptr;
  MsBlockW blk[kMsMaxBlocks];
  MsConv conv5;         // shared.6: 5 x 5 valid
  float* wl = nullptr;  // unshared [style_dim][c_last]
  float* bl = nullptr;
  int min_frames() const {  // the shortest T whose last level still has kMsMinOut columns
    for (int T = 1;; ++T) {
      int t = T;
      for (int i = 0; i < n_down; ++i) t = (t + 1) / 2;
      if (t >= kMsMinOut) return T;
    }
  }
};

struct MelStyleModel {
  MelStyleW enc[2];  // [0] pe_mel_style_encoder, [1] cfm_pitch_predictor.spk_emb
};

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ float ms_lrelu(float v) { return v > 0.f ? v : 0.2f * v; }

// the utterance of packed time row tr: the largest u with off[u] <= tr
__device__ __forceinline__ int ms_utt(const int* __restrict__ off, int n_utt, int tr) {
  int lo = 0, hi = n_utt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= tr) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Time offsets of every level from the mel offsets, on the device (no host copy): out[l][u], l = 0 .. n_down the levels
// (T_{l+1} = ceil(T_l / 2)), l = n_down + 1 the 5 x 5 conv's output (T_last - 4).  One thread: n_utt is small.
__global__ void ms_offsets_kernel(const int* __restrict__ off, int n_utt, int n_down, int* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int l = 0; l <= n_down + 1; ++l) {
    int* o = out + l * (n_utt + 1);
    o[0] = 0;
    for (int u = 0; u < n_utt; ++u) {
      int T = off[u + 1] - off[u];
      for (int i = 0; i < l && i < n_down; ++i) T = (T + 1) / 2;
      if (l == n_down + 1) T -= kMsMinOut - 1;
      o[u + 1] = o[u] + T;
    }
  }
}

// shared.0: Conv2d(1 -> C, 3 x 3, pad 1) straight from the mel rows mel[(off[u] + t) * ldm + f].  One thread per (row, channel).
__global__ void __launch_bounds__(256) STTS_MS_NO_PK
ms_conv0_kernel(const float* __restrict__ mel, int ldm, const int* __restrict__ off, int n_utt, int F, long rows, const float* __restrict__ w,
                const float* __restrict__ b, int C, int ldc, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * ldc) return;
  const long m = i / ldc;
  const int c = (int)(i - m * ldc);
  if (c >= C) {
    Y[i] = 0.f;
    return;
  }
  const int tr = (int)(m / F), f = (int)(m - (long)tr * F);
  const int u = ms_utt(off, n_utt, tr);
  const int t = tr - off[u], T = off[u + 1] - off[u];
  float s = 0.f;
  for (int df = 0; df < 3; ++df) {
    const int fi = f + df - 1;
    if (fi < 0 || fi >= F) continue;
    for (int dt = 0; dt < 3; ++dt) {
      const int ti = t + dt - 1;
      if (ti < 0 || ti >= T) continue;
      s = fmaf(w[c * 9 + df * 3 + dt], mel[(long)(off[u] + ti) * ldm + fi], s);
    }
  }
  Y[i] = s + b[c];
}

// downsample_res ("half"): depthwise Conv2d(C, 3 x 3, stride 2, pad 1) + bias, level l -> l + 1 (F / 2 x ceil(T / 2)).
__global__ void __launch_bounds__(256) STTS_MS_NO_PK
ms_dw_down_kernel(const float* __restrict__ X, const int* __restrict__ offIn, const int* __restrict__ offOut, int n_utt, int F, long rows_out,
                  const float* __restrict__ w, const float* __restrict__ b, int C, int ldc, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows_out * ldc) return;
  const long m = i / ldc;
  const int c = (int)(i - m * ldc);
  if (c >= C) {
    Y[i] = 0.f;
    return;
  }
  const int Fo = F / 2;
  const int tr = (int)(m / Fo), fo = (int)(m - (long)tr * Fo);
  const int u = ms_utt(offOut, n_utt, tr);
  const int to = tr - offOut[u], T = offIn[u + 1] - offIn[u];
  const long base = offIn[u];
  float s = 0.f;
  for (int df = 0; df < 3; ++df) {
    const int fi = 2 * fo + df - 1;
    if (fi < 0 || fi >= F) continue;
    for (int dt = 0; dt < 3; ++dt) {
      const int ti = 2 * to + dt - 1;
      if (ti < 0 || ti >= T) continue;
      s = fmaf(w[c * 9 + df * 3 + dt], X[((base + ti) * F + fi) * ldc + c], s);
    }
  }
  Y[i] = s + b[c];
}

// DownSample("half"): the last time column replicated when T is odd, then avg_pool2d(2).  Level l -> l + 1.
__global__ void __launch_bounds__(256) STTS_MS_NO_PK
ms_pool_half_kernel(const float* __restrict__ X, const int* __restrict__ offIn, const int* __restrict__ offOut, int n_utt, int F, long rows_out, int C,
                    int ldc, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows_out * ldc) return;
  const long m = i / ldc;
  const int c = (int)(i - m * ldc);
  if (c >= C) {
    Y[i] = 0.f;
    return;
  }
  const int Fo = F / 2;
  const int tr = (int)(m / Fo), fo = (int)(m - (long)tr * Fo);
  const int u = ms_utt(offOut, n_utt, tr);
  const int to = tr - offOut[u], T = offIn[u + 1] - offIn[u];
  const long base = offIn[u];
  const int t0 = 2 * to, t1 = min(2 * to + 1, T - 1), f0 = 2 * fo;
  const float s = X[((base + t0) * F + f0) * ldc + c] + X[((base + t1) * F + f0) * ldc + c] + X[((base + t0) * F + f0 + 1) * ldc + c] +
                  X[((base + t1) * F + f0 + 1) * ldc + c];
  Y[i] = s / 4.f;
}

struct MsGemm {
  const float* X;          // input rows [(offIn[u] + t) * F + f][ldk]
  const int* offIn;        // time offsets of the input level
  const int* offOut;       // time offsets of the output level
  int n_utt, F, Fo, pad, k;
  long rows_out;           // output rows = offOut[n_utt] * Fo
  const float* W;          // [k * k * ldk][npad]
  int ldk, npad, N;
  const float* bias;       // [N] or null
  const float* R;          // residual [rows_out][ldy] or null (conv2: the shortcut)
  float div;               // the result is divided by div (conv2 of a ResBlk: sqrt(2); else 1)
  float* Y;                // [rows_out][ldy], ldy = ms_ld(N); channels N .. ldy - 1 are written as 0
  int ldy;
  int k_slice;             // K per slice (blockIdx.z); the whole K when not split
  float* P;                // split-K: raw partial sums [slices][rows_out][ldy] instead of Y (the epilogue runs in the reduce)
};

// Implicit-GEMM 2-D convolution on the f32 matrix cores.  Output (u, t, f) reads input (t + dt - pad, f + df - pad) for the k x k taps;
// positions outside [0, T_u) x [0, F) are zeros (the operand load skips them).  LRELU: LeakyReLU(0.2) on the operand as it is loaded.
// Each output element is one K loop in a fixed order (per slice), independent of the other rows: the same bits alone and in any batch.
// grid (ceil(rows_out / 64), npad / 64, slices), block 256: wave w computes rows 32 (w / 2) .., columns 32 (w % 2) .. with 2 x 2 16 x 16 MFMA tiles.
template <bool LRELU>
__global__ void __launch_bounds__(256) STTS_MS_NO_PK ms_conv_kernel(MsGemm g) {
  __shared__ float As[kMsBK][kMsBM + 4];
  __shared__ float Bs[kMsBK][kMsBN + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * kMsBM;
  const int n0 = blockIdx.y * kMsBN;
  // the A row this thread loads (4 consecutive channels of it per K chunk)
  const int ar = tid >> 2, akq = (tid & 3) * 4;
  const long m = m0 + ar;
  const bool mval = m < g.rows_out;
  int t = 0, f = 0, T = 0;
  long base = 0;
  if (mval) {
    const int tr = (int)(m / g.Fo);
    f = (int)(m - (long)tr * g.Fo);
    const int u = ms_utt(g.offOut, g.n_utt, tr);
    t = tr - g.offOut[u];
    T = g.offIn[u + 1] - g.offIn[u];
    base = g.offIn[u];
  }
  const int bk = tid >> 4, bn = (tid & 15) * 4;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  ms_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = ms_f32x4{0.f, 0.f, 0.f, 0.f};
  const int K = g.k * g.k * g.ldk;
  const int kb = blockIdx.z * g.k_slice, ke = min(K, kb + g.k_slice);
  for (int k0 = kb; k0 < ke; k0 += kMsBK) {
    const int tap = k0 / g.ldk, ci = k0 - tap * g.ldk + akq;
    const int ti = t + tap / g.k - g.pad, fi = f + tap % g.k - g.pad;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mval && ti >= 0 && ti < T && fi >= 0 && fi < g.F) {
      a = *reinterpret_cast<const float4*>(g.X + ((base + ti) * g.F + fi) * (long)g.ldk + ci);
      if (LRELU) {
        a.x = ms_lrelu(a.x);
        a.y = ms_lrelu(a.y);
        a.z = ms_lrelu(a.z);
        a.w = ms_lrelu(a.w);
      }
    }
    const float4 b = *reinterpret_cast<const float4*>(g.W + (long)(k0 + bk) * g.npad + n0 + bn);
    __syncthreads();  // the previous chunk's reads are done
    As[akq + 0][ar] = a.x;
    As[akq + 1][ar] = a.y;
    As[akq + 2][ar] = a.z;
    As[akq + 3][ar] = a.w;
    *reinterpret_cast<float4*>(&Bs[bk][bn]) = b;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kMsBK; kk += 4) {
      const int kl = kk + (lane >> 4);
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = As[kl][wm + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = Bs[kl][wn + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
  // D of a 16 x 16 tile: lane l holds rows 4 (l / 16) + r, r < 4, of column l % 16
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + j * 16 + (lane & 15);
      if (n >= g.ldy) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long mo = m0 + wm + i * 16 + 4 * (lane >> 4) + r;
        if (mo >= g.rows_out) continue;
        if (g.P) {
          g.P[((long)blockIdx.z * g.rows_out + mo) * g.ldy + n] = acc[i][j][r];
          continue;
        }
        float v = 0.f;
        if (n < g.N) {
          v = acc[i][j][r];
          if (g.bias) v += g.bias[n];
          if (g.R) v = g.R[mo * g.ldy + n] + v;
          v = v / g.div;
        }
        g.Y[mo * g.ldy + n] = v;
      }
    }
}

// Split-K epilogue: the slices' partial sums in slice order, then bias, residual and the division as ms_conv_kernel's epilogue.
__global__ void __launch_bounds__(256) STTS_MS_NO_PK
ms_splitk_reduce_kernel(const float* __restrict__ P, int slices, long rows_out, int ldy, int N, const float* __restrict__ bias, const float* __restrict__ R,
                        float div, float* __restrict__ Y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = rows_out * ldy;
  if (i >= total) return;
  const int n = (int)(i % ldy);
  float v = 0.f;
  if (n < N) {
    v = P[i];
    for (int z = 1; z < slices; ++z) v += P[(long)z * total + i];
    if (bias) v += bias[n];
    if (R) v = R[i] + v;
    v = v / div;
  }
  Y[i] = v;
}

// Tail, one block per utterance: mean of the 5 x 5 conv's output over its (F - 4) x (T - 4) positions (rows in order, fixed), LeakyReLU,
// then unshared (Linear).  No atomics: an utterance's style is the same bits alone and in a batch.
__global__ void __launch_bounds__(256) STTS_MS_NO_PK
ms_tail_kernel(const float* __restrict__ H, int ldh, const int* __restrict__ off5, int Fo, int C, const float* __restrict__ Wl, const float* __restrict__ bl,
               int S, float* __restrict__ out, int ld_out) {
  extern __shared__ float hm[];  // [C]
  const int u = blockIdx.x;
  const long r0 = (long)off5[u] * Fo, r1 = (long)off5[u + 1] * Fo;
  const float n = (float)(r1 - r0);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += H[r * ldh + c];
    hm[c] = ms_lrelu(s / n);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < S; j += blockDim.x) {
    const float* w = Wl + (long)j * C;
    float s = 0.f;
    for (int k = 0; k < C; ++k) s = fmaf(w[k], hm[k], s);
    out[(long)u * ld_out + j] = s + bl[j];
  }
}

// ------------------------------------------------------------------------------------------------ packing
// torch.nn.utils.spectral_norm in eval mode (no power iteration): W = W_orig / (u . (W_orig.view(cout, -1) @ v)) from the STORED u and v,
// folded in double.
inline int spectral_norm_weight(stts_ctx* c, const std::string& p, HostTensor* w) {
  STTS_GET(wo, p + ".weight_orig");
  STTS_GET(u, p + ".weight_u");
  STTS_GET(v, p + ".weight_v");
  const int64_t rows = wo->shape[0], per = (int64_t)wo->data.size() / rows;
  STTS_CHECK((int64_t)u->data.size() == rows && (int64_t)v->data.size() == per, "%s: weight_u / weight_v do not match weight_orig", p.c_str());
  double sigma = 0.0;
  for (int64_t r = 0; r < rows; ++r) {
    double s = 0.0;
    for (int64_t i = 0; i < per; ++i) s += (double)wo->data[r * per + i] * v->data[i];
    sigma += (double)u->data[r] * s;
  }
  STTS_CHECK(std::isfinite(sigma) && sigma != 0.0, "%s: spectral norm sigma = %g", p.c_str(), sigma);
  w->shape = wo->shape;
  w->data.resize(wo->data.size());
  for (size_t i = 0; i < wo->data.size(); ++i) w->data[i] = (float)((double)wo->data[i] / sigma);
  return 0;
}

inline int ms_pack_conv(stts_ctx* c, const std::string& p, bool bias, MsConv* o) {
  HostTensor w;
  STTS_TRY(spectral_norm_weight(c, p, &w));
  STTS_CHECK(w.shape.size() == 4 && w.shape[2] == w.shape[3], "%s: expected a square Conv2d weight", p.c_str());
  o->cout = (int)w.shape[0];
  o->cin = (int)w.shape[1];
  o->k = (int)w.shape[2];
  o->ldk = ms_ld(o->cin);
  o->npad = round_up(o->cout, kMsBN);
  const int k = o->k;
  std::vector<float> pk((size_t)k * k * o->ldk * o->npad, 0.f);
  for (int n = 0; n < o->cout; ++n)
    for (int ci = 0; ci < o->cin; ++ci)
      for (int df = 0; df < k; ++df)
        for (int dt = 0; dt < k; ++dt)
          pk[((size_t)(dt * k + df) * o->ldk + ci) * o->npad + n] = w.data[(((size_t)n * o->cin + ci) * k + df) * k + dt];
  STTS_TRY(dev_upload(c, pk, &o->w));
  if (bias) {
    STTS_GET(b, p + ".bias");
    STTS_CHECK((int)b->data.size() == o->cout, "%s.bias: %zu values for %d channels", p.c_str(), b->data.size(), o->cout);
    STTS_TRY(dev_upload(c, b->data, &o->b));
  }
  return 0;
}

inline int ms_upload_small(stts_ctx* c, const std::string& p, int C, float** w, float** b) {  // a [C, 1, 3, 3] conv (conv0 / depthwise)
  HostTensor sw;
  STTS_TRY(spectral_norm_weight(c, p, &sw));
  STTS_CHECK(sw.shape.size() == 4 && sw.shape[0] == C && sw.shape[1] == 1 && sw.shape[2] == 3 && sw.shape[3] == 3, "%s: expected [%d, 1, 3, 3]", p.c_str(), C);
  STTS_GET(sb, p + ".bias");
  STTS_CHECK((int)sb->data.size() == C, "%s.bias: expected %d values", p.c_str(), C);
  STTS_TRY(dev_upload(c, sw.data, w));
  return dev_upload(c, sb->data, b);
}

inline const char* mel_style_prefix(int which) { return which == STTS_W_PE_MEL_STYLE ? "pe_mel_style_encoder." : "cfm_pitch_predictor.spk_emb."; }

// dims from the weight shapes: n_mels = shared.0's cout (dim_in = n_mels, models/models.py:57-62, cfm_pitch_predictor.py:25-27)
inline int finalize_mel_style_one(stts_ctx* c, MelStyleW* E, int which) {
  c->pack.tag = which;
  *E = MelStyleW();
  const std::string p = mel_style_prefix(which);
  STTS_GET(w0, p + "shared.0.weight_orig");
  STTS_CHECK(w0->shape.size() == 4 && w0->shape[1] == 1 && w0->shape[2] == 3 && w0->shape[3] == 3, "%sshared.0: expected a [dim_in, 1, 3, 3] Conv2d", p.c_str());
  E->c0 = E->n_mels = (int)w0->shape[0];
  STTS_TRY(ms_upload_small(c, p + "shared.0", E->c0, &E->w0, &E->b0));
  int cin = E->c0;
  for (int i = 0; i < kMsMaxBlocks; ++i) {
    MsBlockW& B = E->blk[i];
    const std::string q = p + "shared." + std::to_string(i + 1) + ".";
    B.cin = cin;
    STTS_TRY(ms_pack_conv(c, q + "conv1", true, &B.conv1));
    STTS_TRY(ms_pack_conv(c, q + "conv2", true, &B.conv2));
    STTS_CHECK(B.conv1.k == 3 && B.conv2.k == 3 && B.conv1.cin == cin && B.conv1.cout == cin && B.conv2.cin == cin, "%s: conv1 / conv2 shapes do not chain", q.c_str());
    B.cout = B.conv2.cout;
    B.learned_sc = B.cin != B.cout;
    if (B.learned_sc) {
      STTS_TRY(ms_pack_conv(c, q + "conv1x1", false, &B.sc));
      STTS_CHECK(B.sc.k == 1 && B.sc.cin == cin && B.sc.cout == B.cout, "%sconv1x1: expected [%d, %d, 1, 1]", q.c_str(), B.cout, cin);
    }
    B.down = find(c, q + "downsample_res.conv.weight_orig") != nullptr;
    if (B.down) {
      STTS_TRY(ms_upload_small(c, q + "downsample_res.conv", cin, &B.dw_w, &B.dw_b));
      ++E->n_down;
    }
    STTS_CHECK(B.down || i == kMsMaxBlocks - 1, "%s: only the last block may skip downsampling (skip_downsamples)", q.c_str());
    cin = B.cout;
  }
  E->c_last = cin;
  // n_mels: every "half" level halves F exactly (avg_pool2d floors, the stride-2 conv rounds up: an odd F gives mismatched shapes in the
  // reference), and the 5 x 5 conv needs 5 rows after the last one
  const int fdiv = 1 << E->n_down;
  STTS_CHECK(E->n_mels % fdiv == 0 && E->n_mels / fdiv >= kMsMinOut, "n_mels = %d: the encoder needs a multiple of %d of at least %d", E->n_mels, fdiv,
             fdiv * kMsMinOut);
  STTS_TRY(ms_pack_conv(c, p + "shared.6", true, &E->conv5));
  STTS_CHECK(E->conv5.k == 5 && E->conv5.cin == cin && E->conv5.cout == cin, "%sshared.6: expected [%d, %d, 5, 5]", p.c_str(), cin, cin);
  STTS_GET(wl, p + "unshared.weight");
  STTS_GET(bl, p + "unshared.bias");
  STTS_CHECK(wl->shape.size() == 2 && wl->shape[1] == cin && (int64_t)bl->data.size() == wl->shape[0], "%sunshared: expected [style_dim, %d]", p.c_str(), cin);
  E->style_dim = (int)wl->shape[0];
  STTS_TRY(dev_upload(c, wl->data, &E->wl));
  STTS_TRY(dev_upload(c, bl->data, &E->bl));
  E->ready = true;
  return 0;
}

inline int finalize_mel_style(stts_ctx* c, MelStyleModel* M, int which) {
  if (which & STTS_W_PE_MEL_STYLE) STTS_TRY(finalize_mel_style_one(c, &M->enc[0], STTS_W_PE_MEL_STYLE));
  if (which & STTS_W_CFM_PITCH) STTS_TRY(finalize_mel_style_one(c, &M->enc[1], STTS_W_CFM_PITCH));
  return 0;
}

// ------------------------------------------------------------------------------------------------ plan + workspace
struct MsPlan {  // host view of the levels (exact rows; the device computes the same offsets itself)
  int n_lev = 0;           // n_down + 1 levels, then the 5 x 5 output
  int F[kMsMaxBlocks + 2];
  long trows[kMsMaxBlocks + 2];  // time rows (sum over utterances) of each level; [n_lev] = the 5 x 5 output
  long rows(int l) const { return trows[l] * F[l]; }
};

inline int ms_plan(const MelStyleW& E, int n_utt, const int* off, MsPlan* P) {
  P->n_lev = E.n_down + 1;
  for (int l = 0; l <= P->n_lev; ++l) P->trows[l] = 0;
  const int tmin = E.min_frames();
  for (int u = 0; u < n_utt; ++u) {
    int T = off[u + 1] - off[u];
    STTS_CHECK(T >= tmin, "utterance %d has %d mel frames; MelStyleEncoder needs at least %d (its 5 x 5 conv would see fewer than 5 columns)", u, T, tmin);
    for (int l = 0; l < P->n_lev; ++l) {
      P->trows[l] += T;
      T = (T + 1) / 2;
    }
    int t = off[u + 1] - off[u];
    for (int i = 0; i < E.n_down; ++i) t = (t + 1) / 2;
    P->trows[P->n_lev] += t - (kMsMinOut - 1);
  }
  for (int l = 0; l < P->n_lev; ++l) P->F[l] = E.n_mels >> l;
  P->F[P->n_lev] = P->F[P->n_lev - 1] - (kMsMinOut - 1);
  return 0;
}

inline int ms_slices(const MsConv& w) {
  const int K = w.k * w.k * w.ldk;
  return K >= 2 * kMsSplitK ? ceil_div(K, kMsSplitK) : 1;
}

// floats of split-K scratch (one buffer, reused by the convs one after the other): rows(l) = output rows at level l, l = n_down + 1 the 5 x 5 output
template <typename Rows>
inline size_t ms_split_floats(const MelStyleW& E, Rows rows) {
  size_t mx = 0;
  auto need = [&](const MsConv& w, size_t r) {
    if (ms_slices(w) > 1) mx = std::max(mx, (size_t)ms_slices(w) * r * ms_ld(w.cout));
  };
  int l = 0;
  for (int i = 0; i < kMsMaxBlocks; ++i) {
    const MsBlockW& B = E.blk[i];
    const int lo = B.down ? l + 1 : l;
    need(B.conv1, rows(l));
    if (B.learned_sc) need(B.sc, rows(lo));
    need(B.conv2, rows(lo));
    l = lo;
  }
  need(E.conv5, rows(E.n_down + 1));
  return mx;
}

// bytes of workspace for rows_T mel frames in n_utt utterances (upper bound over the ways rows_T can be split)
inline size_t mel_style_workspace_bytes(const MelStyleW& E, int64_t rows_T, int n_utt) {
  size_t fl = 0;
  double tr = (double)rows_T;
  const int levels = E.n_down + 1;
  size_t lev_rows[kMsMaxBlocks + 2];
  for (int l = 0; l < levels; ++l) {
    lev_rows[l] = (size_t)tr * (size_t)(E.n_mels >> l);
    tr = std::ceil(tr / 2.0) + n_utt;
  }
  fl += lev_rows[0] * ms_ld(E.c0);  // conv0
  int l = 0;
  for (int i = 0; i < kMsMaxBlocks; ++i) {
    const MsBlockW& B = E.blk[i];
    const size_t ri = lev_rows[l], ro = lev_rows[B.down ? l + 1 : l];
    fl += ri * ms_ld(B.cin);                               // conv1
    if (B.down) fl += 2 * ro * ms_ld(B.cin);               // depthwise, pooled input
    if (B.learned_sc) fl += ro * ms_ld(B.cout);            // 1 x 1 shortcut
    fl += ro * ms_ld(B.cout);                              // block output
    if (B.down) ++l;
  }
  fl += lev_rows[levels - 1] * ms_ld(E.c_last);  // 5 x 5 output (bounded by the last level)
  fl += ms_split_floats(E, [&](int lv) { return lev_rows[std::min(lv, levels - 1)]; });
  const size_t ints = (size_t)(kMsMaxBlocks + 2) * (n_utt + 1);
  return fl * sizeof(float) + ints * sizeof(int) + 64 * 256 + ((size_t)1 << 20);
}

// ------------------------------------------------------------------------------------------------ MelStyleEncoder.forward
// P: split-K partials, ms_slices(w) * rows_out * ms_ld(cout) floats (unused when the conv is not split)
inline int ms_conv(hipStream_t st, const MsConv& w, bool lrelu, const float* X, const int* offIn, const int* offOut, int n_utt, int F, int Fo, int pad, long rows_out,
                   const float* R, float div, float* Y, float* P) {
  if (rows_out == 0) return 0;
  const int slices = ms_slices(w), ldy = ms_ld(w.cout);
  STTS_CHECK(slices == 1 || P, "mel_style: no split-K scratch");
  MsGemm g{X, offIn, offOut, n_utt, F, Fo, pad, w.k, rows_out, w.w, w.ldk, w.npad, w.cout, w.b, R, div, Y, ldy,
           slices == 1 ? w.k * w.k * w.ldk : kMsSplitK, slices == 1 ? nullptr : P};
  const dim3 grid((unsigned)((rows_out + kMsBM - 1) / kMsBM), w.npad / kMsBN, slices);
  if (lrelu) hipLaunchKernelGGL(ms_conv_kernel<true>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(ms_conv_kernel<false>, grid, dim3(256), 0, st, g);
  if (slices > 1)
    hipLaunchKernelGGL(ms_splitk_reduce_kernel, dim3((unsigned)((rows_out * ldy + 255) / 256)), dim3(256), 0, st, P, slices, rows_out, ldy, w.cout, w.b, R, div, Y);
  return 0;
}

inline unsigned ms_grid(long n) { return (unsigned)((n + 255) / 256); }

// mel [rows_T, ld >= n_mels] (utterance offsets s) -> style_out [n_utt, ld_style >= style_dim].  taps (optional): the four ResBlk outputs one
// after the other, each [rows of its level][ms_ld(cout)] channels-last.
inline int mel_style_forward(const MelStyleW& E, hipStream_t st, const Seg& s, const float* mel, int ld, float* style_out, int ld_style, float* taps, Arena& ws) {
  MsPlan P;
  STTS_TRY(ms_plan(E, s.n_utt, s.host, &P));
  const int n = s.n_utt, nl = P.n_lev;
  int* offs = ws.get<int>((size_t)(nl + 1) * (n + 1));
  STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
  auto off = [&](int l) -> const int* { return l == 0 ? s.dev : offs + l * (n + 1); };
  hipLaunchKernelGGL(ms_offsets_kernel, dim3(1), dim3(64), 0, st, s.dev, n, E.n_down, offs);
  // shared.0
  float* x = ws.get<float>((size_t)P.rows(0) * ms_ld(E.c0));
  STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
  hipLaunchKernelGGL(ms_conv0_kernel, dim3(ms_grid(P.rows(0) * ms_ld(E.c0))), dim3(256), 0, st, mel, ld, s.dev, n, P.F[0], P.rows(0), E.w0, E.b0, E.c0,
                     ms_ld(E.c0), x);
  float* part = nullptr;
  if (const size_t pf = ms_split_floats(E, [&](int lv) { return (size_t)P.rows(lv); })) part = ws.get<float>(pf);
  STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
  int l = 0;
  float* tap = taps;
  for (int i = 0; i < kMsMaxBlocks; ++i) {
    const MsBlockW& B = E.blk[i];
    const int lo = B.down ? l + 1 : l;
    const long ri = P.rows(l), ro = P.rows(lo);
    const int ldi = ms_ld(B.cin), ldo = ms_ld(B.cout);
    float* h1 = ws.get<float>((size_t)ri * ldi);
    float* out = ws.get<float>((size_t)ro * ldo);
    float* hd = B.down ? ws.get<float>((size_t)ro * ldi) : h1;
    float* xp = B.down ? ws.get<float>((size_t)ro * ldi) : x;
    float* sc = B.learned_sc ? ws.get<float>((size_t)ro * ldo) : xp;
    STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
    // residual: conv1(lrelu(x)) [+ downsample_res]; the shortcut: avg-pool first, then the 1 x 1 conv (linear maps commute; 1/4 of its flops)
    STTS_TRY(ms_conv(st, B.conv1, true, x, off(l), off(l), n, P.F[l], P.F[l], 1, ri, nullptr, 1.f, h1, part));
    if (B.down) {
      hipLaunchKernelGGL(ms_dw_down_kernel, dim3(ms_grid(ro * ldi)), dim3(256), 0, st, h1, off(l), off(lo), n, P.F[l], ro, B.dw_w, B.dw_b, B.cin, ldi, hd);
      hipLaunchKernelGGL(ms_pool_half_kernel, dim3(ms_grid(ro * ldi)), dim3(256), 0, st, x, off(l), off(lo), n, P.F[l], ro, B.cin, ldi, xp);
    }
    if (B.learned_sc) STTS_TRY(ms_conv(st, B.sc, false, xp, off(lo), off(lo), n, P.F[lo], P.F[lo], 0, ro, nullptr, 1.f, sc, part));
    // out = (shortcut + conv2(lrelu(hd)) + b2) / sqrt(2)
    STTS_TRY(ms_conv(st, B.conv2, true, hd, off(lo), off(lo), n, P.F[lo], P.F[lo], 1, ro, sc, 1.41421356237309515f, out, part));
    if (tap) {
      STTS_HIP(hipMemcpyAsync(tap, out, (size_t)ro * ldo * sizeof(float), hipMemcpyDeviceToDevice, st));
      tap += (size_t)ro * ldo;
    }
    x = out;
    l = lo;
  }
  // LeakyReLU -> shared.6 (5 x 5, valid) -> mean -> LeakyReLU -> unshared
  const long r5 = P.rows(nl);
  float* h5 = ws.get<float>((size_t)r5 * ms_ld(E.c_last));
  STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
  STTS_TRY(ms_conv(st, E.conv5, true, x, off(l), off(nl), n, P.F[l], P.F[nl], 0, r5, nullptr, 1.f, h5, part));
  hipLaunchKernelGGL(ms_tail_kernel, dim3(n), dim3(256), (size_t)E.c_last * sizeof(float), st, h5, ms_ld(E.c_last), off(nl), P.F[nl], E.c_last, E.wl, E.bl,
                     E.style_dim, style_out, ld_style);
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

// MelStyleEncoder on the engine: spectral-norm folding, the 2-D convolution kernels and the encoder's orchestration.
//   MelStyleEncoder               models/mel_style_encoder.py:120-151 (ResBlk :68-117, DownSample :48-65, LearnedDownSample :8-45)
//   pe_mel_style_encoder          models/models.py:57-62                (STTS_W_PE_MEL_STYLE)
//   cfm_pitch_predictor.spk_emb   models/cfm/cfm_pitch_predictor.py:25-27 (STTS_W_CFM_PITCH)
// Included by api.hip after hubert.hip.h.  Everything here is fp32 on the f32 matrix cores (v_mfma_f32_16x16x4_f32) whatever
// stts_set_precision chose: the 16-bit modes give the same bits as f32 mode.
//
// Layout: channels-last packed rows.  The input of the encoder is the mel [B, 1, F = n_mels, T]; at every
// level the activation of utterance u is the rows (off[u] + t) * F + f, t < T_u, f < F, each row ld(C) = round_up(C, 16) floats with
// the channels contiguous (the pad channels hold zeros).  Every 3 x 3 pad-1, 1 x 1 and 5 x 5 valid conv is conv2d_kernel (conv2d.hip.h)
// with K = k * k * ld(cin), taps in the order dt * k + df, npad = round_up(cout, 64) (the 64 x 64 tile) and one fmaf chain per slice.
#pragma once

namespace stts {

constexpr int kMsMaxBlocks = 4;
constexpr int kMsMinOut = 5;  // the 5 x 5 valid conv needs 5 x 5 positions after the last downsampling
// split-K: a contraction with K >= 2 kMsSplitK runs as ceil(K / kMsSplitK) slices whose partial sums are added in slice order by
// conv2d_reduce_kernel.  The slice count depends on K only (the weights), never on the batch: the bits stay batch-independent.
constexpr int kMsSplitK = 1024;

inline int ms_ld(int c) { return round_up(c, 16); }

struct MsBlockW {
  int cin = 0, cout = 0;
  bool down = false, learned_sc = false;
  Conv2dW conv1, conv2, sc;                  // sc: conv1x1 (no bias) when cin != cout
  float* dw_w = nullptr;                    // downsample_res: depthwise 3 x 3 stride 2, [c][kF][kT]
  float* dw_b = nullptr;
};

struct MelStyleW {
  bool ready = false;
  int n_mels = 0, c0 = 0, style_dim = 0, n_down = 0, c_last = 0;
  float* w0 = nullptr;  // shared.0: 1 -> c0, [c0][kF][kT]
  float* b0 = nullptr;
  MsBlockW blk[kMsMaxBlocks];
  Conv2dW conv5;        // shared.6: 5 x 5 valid
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
__global__ void __launch_bounds__(256) STTS_NO_PK
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
  const int u = utt_of_row(off, n_utt, 0, tr);
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
__global__ void __launch_bounds__(256) STTS_NO_PK
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
  const int u = utt_of_row(offOut, n_utt, 0, tr);
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
__global__ void __launch_bounds__(256) STTS_NO_PK
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
  const int u = utt_of_row(offOut, n_utt, 0, tr);
  const int to = tr - offOut[u], T = offIn[u + 1] - offIn[u];
  const long base = offIn[u];
  const int t0 = 2 * to, t1 = min(2 * to + 1, T - 1), f0 = 2 * fo;
  const float s = X[((base + t0) * F + f0) * ldc + c] + X[((base + t1) * F + f0) * ldc + c] + X[((base + t0) * F + f0 + 1) * ldc + c] +
                  X[((base + t1) * F + f0 + 1) * ldc + c];
  Y[i] = s / 4.f;
}

// Tail, one block per utterance: mean of the 5 x 5 conv's output over its (F - 4) x (T - 4) positions (rows in order, fixed), LeakyReLU,
// then unshared (Linear).  No atomics: an utterance's style is the same bits alone and in a batch.
__global__ void __launch_bounds__(256) STTS_NO_PK
ms_tail_kernel(const float* __restrict__ H, int ldh, const int* __restrict__ off5, int Fo, int C, const float* __restrict__ Wl, const float* __restrict__ bl,
               int S, float* __restrict__ out, int ld_out) {
  extern __shared__ float hm[];  // [C]
  const int u = blockIdx.x;
  const long r0 = (long)off5[u] * Fo, r1 = (long)off5[u + 1] * Fo;
  const float n = (float)(r1 - r0);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += H[r * ldh + c];
    hm[c] = lrelu02(s / n);
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

// a spectral-norm-folded Conv2d [cout, cin, k, k] (cout < 0: any) for conv2d_kernel: taps in the order dt * k + df, tap (dt, df) reads (t + dt - pad, f + df - pad)
inline int ms_pack_conv(stts_ctx* c, const std::string& p, bool bias, int cout, int cin, int k, int pad, Conv2dW* o) {
  HostTensor w;
  STTS_TRY(spectral_norm_weight(c, p, &w));
  STTS_CHECK(w.shape.size() == 4 && (cout < 0 || w.shape[0] == cout) && w.shape[1] == cin && w.shape[2] == k && w.shape[3] == k, "%s: expected a [%d, %d, %d, %d] Conv2d weight",
             p.c_str(), cout, cin, k, k);
  cout = (int)w.shape[0];
  int dt[kConvMaxTaps], df[kConvMaxTaps];
  for (int tap = 0; tap < k * k; ++tap) {
    dt[tap] = tap / k - pad;
    df[tap] = tap % k - pad;
  }
  std::vector<double> b;
  if (bias) {
    STTS_GET(bt, p + ".bias");
    STTS_CHECK((int)bt->data.size() == cout, "%s.bias: %zu values for %d channels", p.c_str(), bt->data.size(), cout);
    b.assign(bt->data.begin(), bt->data.end());
  }
  return conv2d_pack(c, cout, round_up(cout, 64), cin, 0, ms_ld(cin), 0, k * k, dt, df,
                     [&](int n, int ci, int tap) { return (double)w.data[(((size_t)n * cin + ci) * k + tap % k) * k + tap / k]; }, bias ? &b : nullptr, o);
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
    STTS_TRY(ms_pack_conv(c, q + "conv1", true, cin, cin, 3, 1, &B.conv1));
    STTS_TRY(ms_pack_conv(c, q + "conv2", true, -1, cin, 3, 1, &B.conv2));
    B.cout = B.conv2.cout;
    B.learned_sc = B.cin != B.cout;
    if (B.learned_sc) STTS_TRY(ms_pack_conv(c, q + "conv1x1", false, B.cout, cin, 1, 0, &B.sc));
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
  STTS_TRY(ms_pack_conv(c, p + "shared.6", true, cin, cin, kMsMinOut, 0, &E->conv5));
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

inline int ms_slices(const Conv2dW& w) { return w.K >= 2 * kMsSplitK ? ceil_div(w.K, kMsSplitK) : 1; }

// floats of split-K scratch (one buffer, reused by the convs one after the other): rows(l) = output rows at level l, l = n_down + 1 the 5 x 5 output
template <typename Rows>
inline size_t ms_split_floats(const MelStyleW& E, Rows rows) {
  size_t mx = 0;
  auto need = [&](const Conv2dW& w, size_t r) {
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

// ------------------------------------------------------------------------------------------------ MelStyleEncoder.forward
// P: split-K partials, ms_slices(w) * rows_out * ms_ld(cout) floats (unused when the conv is not split)
// the base grid is the output level (offOut, Fo columns); the input level (offIn, F columns) differs from it only for the 5 x 5 valid conv
inline int ms_conv(hipStream_t st, const Conv2dW& w, bool lrelu, const float* X, const int* offIn, const int* offOut, int n_utt, int F, int Fo, long rows_out, const float* R,
                   float div, float* Y, float* P) {
  const int slices = ms_slices(w);
  Conv2dArgs g = conv2d_args(w);
  g.X0 = X;
  g.offIn = offIn;
  g.offOut = offOut;
  g.n_utt = n_utt;
  g.Fin = F;
  g.F = Fo;
  g.rows = rows_out;
  g.chunk = slices == 1 ? w.K : kMsSplitK;
  g.R = R;
  g.div = div;
  g.Y = Y;
  g.ldy = ms_ld(w.cout);
  g.P = slices == 1 ? nullptr : P;
  return conv2d_launch(st, g, lrelu, slices);
}

inline unsigned ms_grid(long n) { return (unsigned)((n + 255) / 256); }

// mel [rows_T, ld >= n_mels] (utterance offsets s) -> style_out [n_utt, ld_style >= style_dim].  taps (optional): the four ResBlk outputs one
// after the other, each [rows of its level][ms_ld(cout)] channels-last.
// The body takes the plan (the workspace query has a bounding one and no offsets); of `s` it reads n_utt and the device offsets.
inline int mel_style_planned(const MelStyleW& E, hipStream_t st, const Seg& s, const MsPlan& P, const float* mel, int ld, float* style_out, int ld_style, float* taps,
                             Arena& ws) {
  const int n = s.n_utt, nl = P.n_lev;
  // every buffer, from the plan alone and ahead of the first launch
  int* offs = ws.get<int>((size_t)(nl + 1) * (n + 1));
  float* x = ws.get<float>((size_t)P.rows(0) * ms_ld(E.c0));  // shared.0's output
  const size_t pf = ms_split_floats(E, [&](int lv) { return (size_t)P.rows(lv); });
  float* part = pf ? ws.get<float>(pf) : nullptr;
  struct { float *h1, *out, *hd, *xp, *sc; } buf[kMsMaxBlocks];  // hd / xp / sc: null where the block has no such buffer
  for (int i = 0, l = 0; i < kMsMaxBlocks; ++i) {
    const MsBlockW& B = E.blk[i];
    const int lo = B.down ? l + 1 : l;
    const size_t ri = (size_t)P.rows(l), ro = (size_t)P.rows(lo), ldi = ms_ld(B.cin), ldo = ms_ld(B.cout);
    buf[i].h1 = ws.get<float>(ri * ldi);
    buf[i].out = ws.get<float>(ro * ldo);
    buf[i].hd = B.down ? ws.get<float>(ro * ldi) : nullptr;
    buf[i].xp = B.down ? ws.get<float>(ro * ldi) : nullptr;
    buf[i].sc = B.learned_sc ? ws.get<float>(ro * ldo) : nullptr;
    l = lo;
  }
  float* h5 = ws.get<float>((size_t)P.rows(nl) * ms_ld(E.c_last));  // the 5 x 5 conv's output
  STTS_CHECK(ws.ok, "mel_style_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  auto off = [&](int l) -> const int* { return l == 0 ? s.dev : offs + l * (n + 1); };
  hipLaunchKernelGGL(ms_offsets_kernel, dim3(1), dim3(64), 0, st, s.dev, n, E.n_down, offs);
  hipLaunchKernelGGL(ms_conv0_kernel, dim3(ms_grid(P.rows(0) * ms_ld(E.c0))), dim3(256), 0, st, mel, ld, s.dev, n, P.F[0], P.rows(0), E.w0, E.b0, E.c0,
                     ms_ld(E.c0), x);
  int l = 0;
  float* tap = taps;
  for (int i = 0; i < kMsMaxBlocks; ++i) {
    const MsBlockW& B = E.blk[i];
    const int lo = B.down ? l + 1 : l;
    const long ri = P.rows(l), ro = P.rows(lo);
    const int ldi = ms_ld(B.cin), ldo = ms_ld(B.cout);
    float* h1 = buf[i].h1;
    float* out = buf[i].out;
    float* hd = B.down ? buf[i].hd : h1;
    float* xp = B.down ? buf[i].xp : x;
    float* sc = B.learned_sc ? buf[i].sc : xp;
    // residual: conv1(lrelu(x)) [+ downsample_res]; the shortcut: avg-pool first, then the 1 x 1 conv (linear maps commute; 1/4 of its flops)
    STTS_TRY(ms_conv(st, B.conv1, true, x, off(l), off(l), n, P.F[l], P.F[l], ri, nullptr, 1.f, h1, part));
    if (B.down) {
      hipLaunchKernelGGL(ms_dw_down_kernel, dim3(ms_grid(ro * ldi)), dim3(256), 0, st, h1, off(l), off(lo), n, P.F[l], ro, B.dw_w, B.dw_b, B.cin, ldi, hd);
      hipLaunchKernelGGL(ms_pool_half_kernel, dim3(ms_grid(ro * ldi)), dim3(256), 0, st, x, off(l), off(lo), n, P.F[l], ro, B.cin, ldi, xp);
    }
    if (B.learned_sc) STTS_TRY(ms_conv(st, B.sc, false, xp, off(lo), off(lo), n, P.F[lo], P.F[lo], ro, nullptr, 1.f, sc, part));
    // out = (shortcut + conv2(lrelu(hd)) + b2) / sqrt(2)
    STTS_TRY(ms_conv(st, B.conv2, true, hd, off(lo), off(lo), n, P.F[lo], P.F[lo], ro, sc, 1.41421356237309515f, out, part));
    if (tap) {
      STTS_HIP(hipMemcpyAsync(tap, out, (size_t)ro * ldo * sizeof(float), hipMemcpyDeviceToDevice, st));
      tap += (size_t)ro * ldo;
    }
    x = out;
    l = lo;
  }
  // LeakyReLU -> shared.6 (5 x 5, valid) -> mean -> LeakyReLU -> unshared
  const long r5 = P.rows(nl);
  STTS_TRY(ms_conv(st, E.conv5, true, x, off(l), off(nl), n, P.F[l], P.F[nl], r5, nullptr, 1.f, h5, part));
  hipLaunchKernelGGL(ms_tail_kernel, dim3(n), dim3(256), (size_t)E.c_last * sizeof(float), st, h5, ms_ld(E.c_last), off(nl), P.F[nl], E.c_last, E.wl, E.bl,
                     E.style_dim, style_out, ld_style);
  STTS_HIP(hipGetLastError());
  return 0;
}
inline int mel_style_forward(const MelStyleW& E, hipStream_t st, const Seg& s, const float* mel, int ld, float* style_out, int ld_style, float* taps, Arena& ws) {
  MsPlan P;
  STTS_TRY(ms_plan(E, s.n_utt, s.host, &P));
  return mel_style_planned(E, st, s, P, mel, ld, style_out, ld_style, taps, ws);
}

// Bytes of workspace for rows_T mel frames in n_utt utterances, however rows_T is split: a dry run of the forward on a bounding plan.
// Halving a level rounds every utterance up, so sum over utterances of ceil(T / 2^l) has no single worst split: level l + 1 is bounded
// by ceil(rows of level l / 2) + n_utt, and the 5 x 5 output by the last level.
inline size_t mel_style_workspace_bytes(const MelStyleW& E, int64_t rows_T, int n_utt) {
  if (rows_T <= 0 || n_utt <= 0) return 0;
  MsPlan P;
  P.n_lev = E.n_down + 1;
  P.trows[0] = rows_T;
  for (int l = 0; l < P.n_lev; ++l) {
    P.F[l] = E.n_mels >> l;
    P.trows[l + 1] = l + 1 < P.n_lev ? (P.trows[l] + 1) / 2 + n_utt : P.trows[l];
  }
  P.F[P.n_lev] = P.F[P.n_lev - 1] - (kMsMinOut - 1);
  const Seg s{n_utt, nullptr, nullptr};
  return dry_run_bytes([&](Arena a) { (void)mel_style_planned(E, nullptr, s, P, nullptr, 0, nullptr, 0, nullptr, a); });
}

}  // namespace stts

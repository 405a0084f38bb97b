// RMVPE pitch extractor on the engine: E2E0 of train/dataprep/rmvpe/{model,deepunet,seq}.py in eval mode, the decode of rmvpe/utils.py:114-131,
// the log-mel front end of rmvpe/spec.py:39-71 and the linear resampling of dataprep/pitch_extractor.py:136-141 (STTS_W_RMVPE).
//   E2E0          DeepUnet0 (5-level residual U-Net over the [time, mel] image) -> cnn (c0 -> 3) -> BiGRU(384, 256) -> Linear(512, 360) -> sigmoid
//   mel2hidden    every utterance reflect-padded on its own to the next multiple of 32 frames, the network over the padded length, the crop
// Included by api.hip after ssl.hip.h.  Everything is fp32 whatever stts_set_precision chose, and built without packed-fp32 instructions.
//
// Layout: the channels-last packed rows of mel_style.hip.h with the TIME axis first.  offP[u] is utterance u's first PADDED
// frame (a multiple of 32).  At level l (0 .. 5) utterance u owns time rows [offP[u] >> l, offP[u + 1] >> l) and F_l = 128 >> l mel columns; the
// activation row of (t, f) is ((offP[u] >> l) + t) * F_l + f, rv_ld(C) = round_up(C, 16) floats with the channels contiguous and the pad channels zero.
// Levels halve exactly, so one offset array serves every level.
//
// Every convolution is conv2d_kernel (conv2d.hip.h): the base grid and the input are the same level (offP for both row maps,
// the level as the shift), two segments read cat(upsampled, skip), up = 2 is one of the four sub-pixel convolutions of a stride-2 transposed
// convolution, and the GRU's input projection and the head are the same kernel with F = 1 and one tap.  rv_npad picks the tile.
//
// Summation: chains of kRvChunk = 256 in weight order, the chunk sums added in chunk order.  Shallow layers add them in the kernel, layers whose base
// grid is level 3 or deeper run the chunks as grid slices and conv2d_reduce_kernel adds them in the same order.  Which of the two a layer does depends
// on the layer only, and so does every other order of operations: an utterance's result is the same bits alone and in any batch.
#pragma once

namespace stts {

constexpr int kRvLevels = 5, kRvMels = 128, kRvClasses = 360, kRvHid = 256, kRvMaxBlocks = 8, kRvMaxInter = 8;
constexpr int kRvChunk = 256;     // K per accumulator chain
constexpr int kRvSplitLevel = 3;  // base grids at this level or deeper run their K chunks as grid slices
constexpr int kRvNfft = 1024, kRvHop = 160, kRvBins = 513;

inline int rv_ld(int c) { return round_up(c, 16); }

struct RvDims {
  int n_blocks = 0, inter_layers = 0, c0 = 0;
};

struct RvBlockW {  // ConvBlockRes: relu(bn(conv3x3)) twice, + shortcut
  int cin = 0, cout = 0;
  bool has_sc = false;
  Conv2dW c1, c2, sc;
};

struct RvW {
  bool ready = false;
  RvDims d;
  float bn_a = 1.f, bn_b = 0.f;                                            // encoder.bn (one channel) as an affine
  float *w0 = nullptr, *b0 = nullptr, *wsc0 = nullptr, *bsc0 = nullptr;  // the first block's cin = 1 conv (BN folded) [c0][9] and its 1 x 1 shortcut
  RvBlockW enc[kRvLevels][kRvMaxBlocks];                                   // enc[0][0].c1 / .sc are unused (w0 / wsc0)
  RvBlockW inter[kRvMaxInter][kRvMaxBlocks];
  Conv2dW up[kRvLevels][4];                                                // decoder conv1 as four sub-pixel convolutions, parity pt * 2 + pf
  RvBlockW dec[kRvLevels][kRvMaxBlocks];
  Conv2dW cnn, ih, head;
  float *whh = nullptr, *bhh = nullptr;  // [dir][k][768] (k-major), [dir][768]
  float* hann = nullptr;
  double2* tw = nullptr;
};

// ------------------------------------------------------------------------------------------------ kernels
// offP[u] = sum over v < u of round_up(T_v, 32); one thread (n_utt is small)
__global__ void rv_offsets_kernel(const int* __restrict__ off, int n_utt, int* __restrict__ offP) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int p = 0;
  for (int u = 0; u <= n_utt; ++u) {
    offP[u] = p;
    if (u < n_utt) p += (off[u + 1] - off[u] + 31) / 32 * 32;
  }
}

// The first ConvBlockRes's cin = 1 half: x = bn(mel) gathered with the reflect padding (frame p >= T reads frame 2 (T - 1) - p), zero outside the padded
// image; H = relu(conv3x3(x) + b) (BN folded), S = wsc x + bsc (the 1 x 1 shortcut).  One thread per (row, channel).
__global__ void __launch_bounds__(256) STTS_NO_PK
rv_conv0_kernel(const float* __restrict__ mel, int ldm, const int* __restrict__ off, const int* __restrict__ offP, int n_utt, long rows, float bn_a, float bn_b,
                const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ wsc, const float* __restrict__ bsc, int C, int ldc,
                float* __restrict__ H, float* __restrict__ S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * ldc) return;
  const long m = i / ldc;
  const int c = (int)(i - m * ldc);
  if (c >= C) {
    H[i] = 0.f;
    S[i] = 0.f;
    return;
  }
  const int tr = (int)(m / kRvMels), f = (int)(m - (long)tr * kRvMels);
  const int u = utt_of_row(offP, n_utt, 0, tr);
  const int t = tr - offP[u], Tp = offP[u + 1] - offP[u], T = off[u + 1] - off[u];
  const float* x = mel + (long)off[u] * ldm;
  float s = 0.f, centre = 0.f;
  for (int dt = 0; dt < 3; ++dt) {
    const int ti = t + dt - 1;
    if (ti < 0 || ti >= Tp) continue;
    const int src = ti < T ? ti : 2 * (T - 1) - ti;
    for (int df = 0; df < 3; ++df) {
      const int fi = f + df - 1;
      if (fi < 0 || fi >= kRvMels) continue;
      const float v = fmaf(bn_a, x[(long)src * ldm + fi], bn_b);
      if (dt == 1 && df == 1) centre = v;
      s = fmaf(w[c * 9 + dt * 3 + df], v, s);
    }
  }
  H[i] = fmaxf(s + b[c], 0.f);
  S[i] = fmaf(wsc[c], centre, bsc[c]);
}

// AvgPool2d(2): level l -> l + 1.  One thread per (output row, 4 channels).
__global__ void __launch_bounds__(256) STTS_NO_PK rv_pool_kernel(const float* __restrict__ X, int Fo, long rows_out, int ldc, float* __restrict__ Y) {
  const int c4n = ldc / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows_out * c4n) return;
  const long m = i / c4n;
  const int c = (int)(i - m * c4n) * 4;
  const long tr = m / Fo;
  const int f = (int)(m - tr * Fo);
  const long r00 = (2 * tr * (2 * Fo) + 2 * f) * ldc + c, r10 = r00 + (long)(2 * Fo) * ldc;
  const float4 a = *reinterpret_cast<const float4*>(X + r00), b = *reinterpret_cast<const float4*>(X + r00 + ldc);
  const float4 d = *reinterpret_cast<const float4*>(X + r10), e = *reinterpret_cast<const float4*>(X + r10 + ldc);
  float4 y;
  y.x = (a.x + b.x + d.x + e.x) * 0.25f;
  y.y = (a.y + b.y + d.y + e.y) * 0.25f;
  y.z = (a.z + b.z + d.z + e.z) * 0.25f;
  y.w = (a.w + b.w + d.w + e.w) * 0.25f;
  *reinterpret_cast<float4*>(Y + m * ldc + c) = y;
}

// GRU recurrence (torch gate order r, z, n; n = tanh(W_in x + b_in + r (W_hn h + b_hn))): one workgroup per (utterance, direction), thread j = gate row j.
// W_hh^T is [k][768]: thread j keeps the first 128 k of its row in registers and streams the other 128 from L2 every step (786 KB of W_hh are more than a
// CU holds); h lives in LDS.  xi = W_ih x + b_ih for every frame [frames][2 x 768].  Each dot product is one fmaf chain in k order.  No workgroup waits
// on another.  The backward direction starts at the last PADDED frame.
__global__ void __launch_bounds__(768) STTS_NO_PK rv_gru_kernel(const float* __restrict__ xi, const int* __restrict__ offP, const float* __restrict__ WhhT,
                                                                  const float* __restrict__ bhh, float* __restrict__ out) {
  constexpr int H = kRvHid, G = 3 * kRvHid, KR = 128;
  __shared__ __attribute__((aligned(16))) float h[H];
  __shared__ float gh[G];
  const int u = blockIdx.x, dir = blockIdx.y, j = threadIdx.x;
  const int lo = offP[u], T = offP[u + 1] - lo;
  const float* W = WhhT + (long)dir * H * G + j;
  float wreg[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) wreg[k] = W[(long)k * G];
  const float* wl = W + (long)KR * G;
  const float bias = bhh[dir * G + j];
  if (j < H) h[j] = 0.f;
  __syncthreads();
  for (int step = 0; step < T; ++step) {
    const int t = dir ? T - 1 - step : step;
    const float* x = xi + (long)(lo + t) * (2 * G) + dir * G;
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (j < H) {
      gr = x[j];
      gz = x[H + j];
      gn = x[2 * H + j];
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KR; k += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(&h[k]);
      s = fmaf(wreg[k], hv.x, s);
      s = fmaf(wreg[k + 1], hv.y, s);
      s = fmaf(wreg[k + 2], hv.z, s);
      s = fmaf(wreg[k + 3], hv.w, s);
    }
#pragma unroll 8
    for (int k = 0; k < H - KR; k += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(&h[KR + k]);
      s = fmaf(wl[(long)k * G], hv.x, s);
      s = fmaf(wl[(long)(k + 1) * G], hv.y, s);
      s = fmaf(wl[(long)(k + 2) * G], hv.z, s);
      s = fmaf(wl[(long)(k + 3) * G], hv.w, s);
    }
    gh[j] = s + bias;
    __syncthreads();  // every h[k] has been read, every gh written
    if (j < H) {
      const float r = 1.f / (1.f + expf(-(gr + gh[j])));
      const float z = 1.f / (1.f + expf(-(gz + gh[H + j])));
      const float n = tanhf(gn + r * gh[2 * H + j]);
      const float hn = (1.f - z) * n + z * h[j];
      h[j] = hn;
      out[(long)(lo + t) * (2 * H) + dir * H + j] = hn;
    }
    __syncthreads();
  }
}

// hidden[off[u] + t][0 .. 360) = HP[offP[u] + t][0 .. 360), t < T_u (the crop of mel2hidden); grid (ceil(max T * 360 / 256), n_utt)
__global__ void __launch_bounds__(256) STTS_NO_PK rv_crop_kernel(const float* __restrict__ HP, int ldh, const int* __restrict__ off, const int* __restrict__ offP,
                                                       float* __restrict__ out) {
  const int u = blockIdx.y;
  const long total = (long)(off[u + 1] - off[u]) * kRvClasses;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long t = i / kRvClasses;
    const int n = (int)(i - t * kRvClasses);
    out[(off[u] + t) * kRvClasses + n] = HP[(offP[u] + t) * ldh + n];
  }
}

// The local average of to_local_average_f0 around the centre bin c (0 <= c < 360) of one salience row s, `best` the row's largest value: shared by the
// argmax decode below and the decode around a given centre (rmvpe_viterbi.hip.h), which therefore agree bit for bit where the centres do.
__device__ __forceinline__ float rv_local_average(const float* __restrict__ s, int c, float best, float thred) {
  const int a = max(0, c - 4), b = min(kRvClasses, c + 5);
  double ps = 0.0, wsum = 0.0;
  for (int i = a; i < b; ++i) {
    const float cents = (float)(20 * i) + 1997.3794084376191f;  // the reference's mapping is an fp32 tensor
    ps += (double)s[i] * (double)cents;
    wsum += (double)s[i];
  }
  const double cents = ps / (wsum + (wsum == 0.0 ? 1.0 : 0.0));
  const float v = (float)(10.0 * exp2(cents / 1200.0));
  return best < thred ? 0.f : v;
}

// to_local_average_f0: one wave per frame.  c = the first argmax bin; the salience-weighted mean of 20 i + 1997.379... cents over [c - 4, c + 5) clipped to
// [0, 360); f0 = 10 * 2^(cents / 1200), 0 where the frame's maximum is below thred.  The nine-term sums and the power run in double (one lane).
__global__ void __launch_bounds__(256) STTS_NO_PK rv_decode_kernel(const float* __restrict__ S, int ld, long rows, float thred, float* __restrict__ f0) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * ld;
  float best = -INFINITY;
  int bi = kRvClasses;
  for (int i = lane; i < kRvClasses; i += 64) {
    const float v = s[i];
    if (v > best) {
      best = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane != 0) return;
  if (bi >= kRvClasses) bi = 0;  // a row of NaNs
  f0[row] = rv_local_average(s, bi, best, thred);
}

// F.interpolate(mode="linear", align_corners=True) of every utterance's curve from its L frames to its n frames; positions in double
__global__ void __launch_bounds__(256) STTS_NO_PK rv_resample_kernel(const float* __restrict__ X, const int* __restrict__ off_in, const int* __restrict__ off_out,
                                                           float* __restrict__ Y) {
  const int u = blockIdx.y;
  const int L = off_in[u + 1] - off_in[u], n = off_out[u + 1] - off_out[u];
  const float* x = X + off_in[u];
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    const double pos = n > 1 ? (double)j * (double)(L - 1) / (double)(n - 1) : 0.0;
    int i0 = (int)pos;
    if (i0 > L - 1) i0 = L - 1;
    const int i1 = min(i0 + 1, L - 1);
    const double lam = pos - (double)i0;
    Y[off_out[u] + j] = (float)((1.0 - lam) * (double)x[i0] + lam * (double)x[i1]);
  }
}

// Log-mel of rmvpe/spec.py (n_fft = win = 1024, hop 160, periodic Hann, center=True with reflect padding, magnitude, mel basis, log(clamp(., 1e-5))):
// one wave per frame on the one-wave FFT of signal_geom.hip.h (H = 512, fp64), the 513 magnitudes in LDS, then mel m = the basis row's nonzero band
// [band[2 m], band[2 m + 1]) summed in bin order.  Writes time-major rows [frame][ld_out >= 128]; lin (optional): the mel before the clamp and the log.
__global__ void __launch_bounds__(64 * GeomFft<9>::kWaves) STTS_NO_PK
rv_mel_kernel(const float* __restrict__ wave, const int* __restrict__ samp_off, const int* __restrict__ mel_off, const float* __restrict__ hann,
              const double2* __restrict__ twiddle, const float* __restrict__ basis, const int* __restrict__ band, float* __restrict__ out, int ld_out,
              float* __restrict__ lin) {
  using G = GeomFft<9>;
  constexpr int H = G::H;
  __shared__ double2 bufs[G::kWaves][G::kBuf];
  __shared__ float mags[G::kWaves][kRvBins + 3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, f = blockIdx.x * G::kWaves + wv;
  const int nfr = mel_off[u + 1] - mel_off[u];
  if (f >= nfr) return;  // whole waves leave: nothing below synchronises across waves
  double2* Z = bufs[wv];
  float* mg = mags[wv];
  const long L = samp_off[u + 1] - samp_off[u];
  const float* x = wave + samp_off[u];
  auto sample = [&](int p) -> double {
    long m = (long)f * kRvHop - H + p;
    if (m < 0) m = -m;
    if (m >= L) m = 2 * (L - 1) - m;
    m = m < 0 ? 0 : (m >= L ? L - 1 : m);  // in bounds whatever the length (the entry point refuses what cannot be reflected)
    return (double)(x[m] * hann[p]);
  };
#pragma unroll
  for (int r = 0; r < H / 64; ++r) {
    const int n = lane + 64 * r;
    Z[fphys(n)] = make_double2(sample(2 * n), sample(2 * n + 1));
  }
  wave_lds_fence();
  fft_wave_r2<double2, 9, false>(Z, twiddle, lane);
  const double2 z0 = Z[0];
  for (int k = lane; k <= H; k += 64) {
    double re, im;
    if (k == 0 || k == H) {
      re = k == 0 ? z0.x + z0.y : z0.x - z0.y;
      im = 0.0;
    } else {
      const double2 a = Z[fphys(k)], b = Z[fphys(H - k)], w = twiddle[k];
      const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);
      const double orr = 0.5 * (a.y + b.y), oi = -0.5 * (a.x - b.x);
      re = er + orr * w.x - oi * w.y;
      im = ei + orr * w.y + oi * w.x;
    }
    mg[k] = (float)sqrt(re * re + im * im);
  }
  wave_lds_fence();
  const long row = mel_off[u] + f;
  for (int m = lane; m < kRvMels; m += 64) {
    const int lo = band[2 * m], hi = band[2 * m + 1];
    const float* bw = basis + (long)m * kRvBins;
    float s = 0.f;
    for (int k = lo; k < hi; ++k) s = fmaf(bw[k], mg[k], s);
    if (lin) lin[row * kRvMels + m] = s;
    out[row * ld_out + m] = logf(fmaxf(s, 1e-5f));
  }
}

// ------------------------------------------------------------------------------------------------ packing
// BatchNorm2d in eval mode as (scale, shift) per channel, in double: y = scale x + shift
inline int rv_bn(stts_ctx* c, const std::string& p, int C, std::vector<double>* scale, std::vector<double>* shift) {
  STTS_GET(g, p + ".weight");
  STTS_GET(b, p + ".bias");
  STTS_GET(mu, p + ".running_mean");
  STTS_GET(var, p + ".running_var");
  STTS_CHECK((int)g->data.size() == C && (int)b->data.size() == C && (int)mu->data.size() == C && (int)var->data.size() == C, "%s: expected a BatchNorm2d of %d channels",
             p.c_str(), C);
  scale->resize(C);
  shift->resize(C);
  for (int i = 0; i < C; ++i) {
    STTS_CHECK(var->data[i] >= 0.f, "%s.running_var[%d] is negative", p.c_str(), i);
    (*scale)[i] = (double)g->data[i] / sqrt((double)var->data[i] + 1e-5);
    (*shift)[i] = (double)b->data[i] - (double)mu->data[i] * (*scale)[i];
  }
  return 0;
}

inline int rv_npad(int cout) { return cout <= 16 ? 16 : cout <= 32 ? 32 : round_up(cout, 64); }

static const int kRvDt3[9] = {-1, -1, -1, 0, 0, 0, 1, 1, 1}, kRvDf3[9] = {-1, 0, 1, -1, 0, 1, -1, 0, 1};
static const int kRvZero[1] = {0};

inline int rv_get_conv(stts_ctx* c, const std::string& name, int d0, int d1, int k, const HostTensor** w) {
  *w = find(c, name);
  STTS_CHECK(*w, "missing weight '%s'", name.c_str());
  STTS_CHECK((*w)->shape.size() == 4 && (*w)->shape[0] == d0 && (*w)->shape[1] == d1 && (*w)->shape[2] == k && (*w)->shape[3] == k, "%s: expected [%d, %d, %d, %d]", name.c_str(),
             d0, d1, k, k);
  return 0;
}

// Conv2d(cin -> cout, 3 x 3, no bias) + BatchNorm folded in double; cin = cin0 + cin1 over two segments
inline int rv_pack_conv_bn(stts_ctx* c, const std::string& conv, const std::string& bn, int cout, int cin0, int cin1, Conv2dW* o) {
  const HostTensor* w;
  STTS_TRY(rv_get_conv(c, conv + ".weight", cout, cin0 + cin1, 3, &w));
  std::vector<double> sc, sh;
  STTS_TRY(rv_bn(c, bn, cout, &sc, &sh));
  const int cin = cin0 + cin1;
  return conv2d_pack(c, cout, rv_npad(cout), cin0, cin1, rv_ld(cin0), cin1 ? rv_ld(cin1) : 0, 9, kRvDt3, kRvDf3,
                 [&](int n, int ci, int tap) { return (double)w->data[((size_t)n * cin + ci) * 9 + tap] * sc[n]; }, &sh, o);
}

// ConvBlockRes(cin0 + cin1 -> cout) at key prefix p
inline int rv_pack_block(stts_ctx* c, const std::string& p, int cin0, int cin1, int cout, RvBlockW* B) {
  const int cin = cin0 + cin1;
  B->cin = cin;
  B->cout = cout;
  B->has_sc = cin != cout;
  STTS_TRY(rv_pack_conv_bn(c, p + "conv.0", p + "conv.1", cout, cin0, cin1, &B->c1));
  STTS_TRY(rv_pack_conv_bn(c, p + "conv.3", p + "conv.4", cout, cout, 0, &B->c2));
  if (B->has_sc) {
    const HostTensor* w;
    STTS_TRY(rv_get_conv(c, p + "shortcut.weight", cout, cin, 1, &w));
    STTS_GET(b, p + "shortcut.bias");
    STTS_CHECK((int)b->data.size() == cout, "%sshortcut.bias: expected %d values", p.c_str(), cout);
    std::vector<double> bb(b->data.begin(), b->data.end());
    STTS_TRY(conv2d_pack(c, cout, rv_npad(cout), cin0, cin1, rv_ld(cin0), cin1 ? rv_ld(cin1) : 0, 1, kRvZero, kRvZero, [&](int n, int ci, int) { return (double)w->data[(size_t)n * cin + ci]; }, &bb,
                     &B->sc));
  } else {
    STTS_CHECK(!find(c, p + "shortcut.weight"), "%sshortcut is present but the block keeps its channel count", p.c_str());
  }
  return 0;
}

// per axis of ConvTranspose2d(3, stride 2, padding 1, output_padding 1): out[2 j] = x[j] w[1]; out[2 j + 1] = x[j] w[2] + x[j + 1] w[0]
inline int rv_up_taps(int parity, int* d, int* k) {
  if (parity == 0) {
    d[0] = 0;
    k[0] = 1;
    return 1;
  }
  d[0] = 0;
  k[0] = 2;
  d[1] = 1;
  k[1] = 0;
  return 2;
}

inline int finalize_rmvpe(stts_ctx* c, const RvDims& d, RvW* M) {
  *M = RvW();
  M->d = d;
  STTS_CHECK(d.n_blocks >= 1 && d.n_blocks <= kRvMaxBlocks, "rmvpe: n_blocks %d outside [1, %d]", d.n_blocks, kRvMaxBlocks);
  STTS_CHECK(d.inter_layers >= 1 && d.inter_layers <= kRvMaxInter, "rmvpe: inter_layers %d outside [1, %d]", d.inter_layers, kRvMaxInter);
  STTS_CHECK(d.c0 >= 1 && d.c0 <= 64, "rmvpe: en_out_channels %d outside [1, 64]", d.c0);
  const std::string p = "rmvpe.";
  {  // encoder.bn: one channel, applied where the mel is read (the zero padding of the first conv sees post-BN zeros, so it does not fold into the weights)
    std::vector<double> sc, sh;
    STTS_TRY(rv_bn(c, p + "unet.encoder.bn", 1, &sc, &sh));
    M->bn_a = (float)sc[0];
    M->bn_b = (float)sh[0];
  }
  // ---- encoder
  int cin = 1, cout = d.c0;
  for (int l = 0; l < kRvLevels; ++l) {
    for (int b = 0; b < d.n_blocks; ++b) {
      const std::string q = p + "unet.encoder.layers." + std::to_string(l) + ".conv." + std::to_string(b) + ".";
      RvBlockW& B = M->enc[l][b];
      if (l == 0 && b == 0) {  // cin = 1: the VALU kernel
        const HostTensor *w, *ws;
        STTS_TRY(rv_get_conv(c, q + "conv.0.weight", cout, 1, 3, &w));
        std::vector<double> sc, sh;
        STTS_TRY(rv_bn(c, q + "conv.1", cout, &sc, &sh));
        std::vector<float> w0((size_t)cout * 9), b0(cout);
        for (int n = 0; n < cout; ++n) {
          for (int t = 0; t < 9; ++t) w0[(size_t)n * 9 + t] = (float)((double)w->data[(size_t)n * 9 + t] * sc[n]);
          b0[n] = (float)sh[n];
        }
        STTS_TRY(dev_upload(c, w0, &M->w0));
        STTS_TRY(dev_upload(c, b0, &M->b0));
        STTS_CHECK(cout != 1, "rmvpe: en_out_channels = 1 leaves the first block without its shortcut conv");
        STTS_TRY(rv_get_conv(c, q + "shortcut.weight", cout, 1, 1, &ws));
        STTS_GET(bs, q + "shortcut.bias");
        STTS_CHECK((int)bs->data.size() == cout, "%sshortcut.bias: expected %d values", q.c_str(), cout);
        STTS_TRY(dev_upload(c, ws->data, &M->wsc0));
        STTS_TRY(dev_upload(c, bs->data, &M->bsc0));
        B.cin = 1;
        B.cout = cout;
        B.has_sc = true;
        STTS_TRY(rv_pack_conv_bn(c, q + "conv.3", q + "conv.4", cout, cout, 0, &B.c2));
      } else {
        STTS_TRY(rv_pack_block(c, q, b == 0 ? cin : cout, 0, cout, &B));
      }
    }
    cin = cout;
    cout *= 2;
  }
  // ---- intermediate: cin (= c0 * 16) -> cout (= c0 * 32), then cout -> cout
  for (int i = 0; i < d.inter_layers; ++i)
    for (int b = 0; b < d.n_blocks; ++b) {
      const std::string q = p + "unet.intermediate.layers." + std::to_string(i) + ".conv." + std::to_string(b) + ".";
      STTS_TRY(rv_pack_block(c, q, (i == 0 && b == 0) ? cin : cout, 0, cout, &M->inter[i][b]));
    }
  // ---- decoder: level i takes the grid of level 5 - i to level 4 - i
  int dc = cout;
  for (int i = 0; i < kRvLevels; ++i) {
    const int oc = dc / 2;
    const std::string q = p + "unet.decoder.layers." + std::to_string(i) + ".";
    const HostTensor* w;
    STTS_TRY(rv_get_conv(c, q + "conv1.0.weight", dc, oc, 3, &w));
    std::vector<double> sc, sh;
    STTS_TRY(rv_bn(c, q + "conv1.1", oc, &sc, &sh));
    for (int pt = 0; pt < 2; ++pt)
      for (int pf = 0; pf < 2; ++pf) {
        int dtt[2], kt[2], dff[2], kf[2], tdt[4], tdf[4], tk[4];
        const int nt = rv_up_taps(pt, dtt, kt), nf = rv_up_taps(pf, dff, kf);
        int ntap = 0;
        for (int a = 0; a < nt; ++a)
          for (int b = 0; b < nf; ++b) {
            tdt[ntap] = dtt[a];
            tdf[ntap] = dff[b];
            tk[ntap++] = kt[a] * 3 + kf[b];
          }
        STTS_TRY(conv2d_pack(c, oc, rv_npad(oc), dc, 0, rv_ld(dc), 0, ntap, tdt, tdf, [&](int n, int ci, int tap) { return (double)w->data[((size_t)ci * oc + n) * 9 + tk[tap]] * sc[n]; }, &sh,
                         &M->up[i][pt * 2 + pf]));
      }
    for (int b = 0; b < d.n_blocks; ++b) {
      const std::string qb = q + "conv2." + std::to_string(b) + ".";
      if (b == 0) STTS_TRY(rv_pack_block(c, qb, oc, oc, oc, &M->dec[i][b]));  // cat(upsampled, skip)
      else STTS_TRY(rv_pack_block(c, qb, oc, 0, oc, &M->dec[i][b]));
    }
    dc = oc;
  }
  STTS_CHECK(dc == d.c0, "rmvpe: the decoder ends at %d channels, not en_out_channels", dc);
  // ---- cnn: c0 -> 3, 3 x 3, bias; its output rows are 4 floats (c = 3 zero), so a frame's 128 rows are the GRU's 512 input columns f * 4 + c
  {
    const HostTensor* w;
    STTS_TRY(rv_get_conv(c, p + "cnn.weight", 3, d.c0, 3, &w));
    STTS_GET(b, p + "cnn.bias");
    STTS_CHECK((int)b->data.size() == 3, "rmvpe.cnn.bias: expected 3 values");
    std::vector<double> bb(b->data.begin(), b->data.end());
    STTS_TRY(conv2d_pack(c, 3, rv_npad(3), d.c0, 0, rv_ld(d.c0), 0, 9, kRvDt3, kRvDf3, [&](int n, int ci, int tap) { return (double)w->data[((size_t)n * d.c0 + ci) * 9 + tap]; }, &bb, &M->cnn));
  }
  // ---- BiGRU: W_ih of both directions repacked to the channels-last columns (reference feature c * 128 + f -> column f * 4 + c), W_hh transposed
  {
    const int G = 3 * kRvHid, IN = 3 * kRvMels;
    const char* sfx[2] = {"", "_reverse"};
    const HostTensor *wih[2], *whh[2], *bih[2], *bhh[2];
    for (int dir = 0; dir < 2; ++dir) {
      const std::string q = p + "fc.0.gru.";
      wih[dir] = find(c, q + "weight_ih_l0" + sfx[dir]);
      whh[dir] = find(c, q + "weight_hh_l0" + sfx[dir]);
      bih[dir] = find(c, q + "bias_ih_l0" + sfx[dir]);
      bhh[dir] = find(c, q + "bias_hh_l0" + sfx[dir]);
      STTS_CHECK(wih[dir] && whh[dir] && bih[dir] && bhh[dir], "missing weight '%sweight_ih_l0%s' (or weight_hh / bias_ih / bias_hh)", q.c_str(), sfx[dir]);
      STTS_CHECK(wih[dir]->shape.size() == 2 && wih[dir]->shape[0] == G && wih[dir]->shape[1] == IN && whh[dir]->shape.size() == 2 && whh[dir]->shape[0] == G &&
                     whh[dir]->shape[1] == kRvHid && (int)bih[dir]->data.size() == G && (int)bhh[dir]->data.size() == G,
                 "%s: expected a GRU(%d, %d)", q.c_str(), IN, kRvHid);
    }
    std::vector<double> bi(2 * G);
    for (int n = 0; n < 2 * G; ++n) bi[n] = bih[n / G]->data[n % G];
    STTS_TRY(conv2d_pack(c, 2 * G, rv_npad(2 * G), 4 * kRvMels, 0, 4 * kRvMels, 0, 1, kRvZero, kRvZero,
                     [&](int n, int col, int) {
                       const int f = col / 4, ch = col % 4;
                       return ch < 3 ? (double)wih[n / G]->data[(size_t)(n % G) * IN + ch * kRvMels + f] : 0.0;
                     },
                     &bi, &M->ih));
    std::vector<float> wt((size_t)2 * kRvHid * G), bh((size_t)2 * G);
    for (int dir = 0; dir < 2; ++dir)
      for (int j = 0; j < G; ++j) {
        for (int k = 0; k < kRvHid; ++k) wt[((size_t)dir * kRvHid + k) * G + j] = whh[dir]->data[(size_t)j * kRvHid + k];
        bh[(size_t)dir * G + j] = bhh[dir]->data[j];
      }
    STTS_TRY(dev_upload(c, wt, &M->whh));
    STTS_TRY(dev_upload(c, bh, &M->bhh));
  }
  {  // head
    STTS_GET(w, p + "fc.1.weight");
    STTS_GET(b, p + "fc.1.bias");
    STTS_CHECK(w->shape.size() == 2 && w->shape[0] == kRvClasses && w->shape[1] == 2 * kRvHid && (int)b->data.size() == kRvClasses, "rmvpe.fc.1: expected a Linear(%d, %d)",
               2 * kRvHid, kRvClasses);
    std::vector<double> bb(b->data.begin(), b->data.end());
    STTS_TRY(conv2d_pack(c, kRvClasses, rv_npad(kRvClasses), 2 * kRvHid, 0, 2 * kRvHid, 0, 1, kRvZero, kRvZero, [&](int n, int ci, int) { return (double)w->data[(size_t)n * 2 * kRvHid + ci]; }, &bb, &M->head));
  }
  {  // the front end's window and twiddles
    std::vector<float> hann;
    std::vector<double2> tw;
    signal_tables(kRvNfft, kRvNfft, &hann, &tw);
    STTS_TRY(dev_upload(c, hann, &M->hann));
    STTS_TRY(dev_upload(c, tw, &M->tw));
  }
  M->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ forward
inline long rv_padded(int n_utt, const int* off) {
  long tp = 0;
  for (int u = 0; u < n_utt; ++u) tp += round_up(off[u + 1] - off[u], 32);
  return tp;
}

inline int rv_slices(const Conv2dW& w, int sh) { return sh >= kRvSplitLevel && w.K > kRvChunk ? ceil_div(w.K, kRvChunk) : 1; }

// floats of slice scratch for Tp padded frames: the largest of every split layer (one buffer, the layers run one after the other)
inline size_t rv_partial_floats(const RvW& M, long Tp) {
  size_t mx = 0;
  auto need = [&](const Conv2dW& w, int sh) {
    if (rv_slices(w, sh) > 1) mx = std::max(mx, (size_t)rv_slices(w, sh) * (size_t)(Tp >> sh) * (kRvMels >> sh) * rv_ld(w.cout));
  };
  auto block = [&](const RvBlockW& B, int sh) {
    if (B.c1.w) need(B.c1, sh);
    need(B.c2, sh);
    if (B.has_sc && B.sc.w) need(B.sc, sh);
  };
  for (int l = 0; l < kRvLevels; ++l)
    for (int b = 0; b < M.d.n_blocks; ++b) block(M.enc[l][b], l);
  for (int i = 0; i < M.d.inter_layers; ++i)
    for (int b = 0; b < M.d.n_blocks; ++b) block(M.inter[i][b], kRvLevels);
  for (int i = 0; i < kRvLevels; ++i) {
    for (int q = 0; q < 4; ++q) need(M.up[i][q], kRvLevels - i);
    for (int b = 0; b < M.d.n_blocks; ++b) block(M.dec[i][b], kRvLevels - 1 - i);
  }
  return mx;
}

inline size_t rv_level_floats(const RvW& M, long Tp, int l, int C) { return (size_t)(Tp >> l) * (kRvMels >> l) * rv_ld(C); }

struct RvRun {
  hipStream_t st;
  const int* offP;
  int n_utt;
  long Tp;
  float* part;
};

// one convolution / contraction: base grid level sh with F columns (F = 1, sh = 0: frames)
inline int rv_launch(const RvRun& r, const Conv2dW& w, int sh, int F, int up, int pt, int pf, const float* X0, const float* X1, int act, const float* R, float* Y, int ldy) {
  const int slices = F == 1 ? 1 : rv_slices(w, sh);
  Conv2dArgs g = conv2d_args(w);
  g.X0 = X0;
  g.X1 = X1;
  g.offIn = g.offOut = r.offP;
  g.n_utt = r.n_utt;
  g.sh = sh;
  g.Fin = g.F = F;
  g.up = up;
  g.pt = pt;
  g.pf = pf;
  g.rows = (r.Tp >> sh) * F;
  g.chunk = kRvChunk;
  g.act = act;
  g.R = R;
  g.Y = Y;
  g.ldy = ldy;
  g.P = slices > 1 ? r.part : nullptr;
  return conv2d_launch(r.st, g, false, slices);
}

inline int rv_conv3(const RvRun& r, const Conv2dW& w, int l, const float* X0, const float* X1, int act, const float* R, float* Y) {
  return rv_launch(r, w, l, kRvMels >> l, 1, 0, 0, X0, X1, act, R, Y, rv_ld(w.cout));
}

// ConvBlockRes at level l: x (and x1, the second segment) -> out; h and s are scratch.  out = relu(c2(relu(c1 x))) + (sc x | x)
inline int rv_block(const RvRun& r, const RvBlockW& B, int l, const float* x, const float* x1, float* h, float* s, float* out) {
  STTS_TRY(rv_conv3(r, B.c1, l, x, x1, CONV_ACT_RELU, nullptr, h));
  const float* res = x;
  if (B.has_sc) {
    STTS_TRY(rv_conv3(r, B.sc, l, x, x1, CONV_ACT_NONE, nullptr, s));
    res = s;
  }
  return rv_conv3(r, B.c2, l, h, nullptr, CONV_ACT_RELU, res, out);
}

// floats of the taps of Tp padded frames: enc0 .. 4 (pooled), inter, dec0 .. 4, cnn [Tp * 128][4], gru [Tp][512]
inline size_t rmvpe_tap_floats(const RvDims& d, long Tp) {
  size_t fl = 0;
  for (int l = 0; l < kRvLevels; ++l) fl += (size_t)(Tp >> (l + 1)) * (kRvMels >> (l + 1)) * rv_ld(d.c0 << l);
  fl += (size_t)(Tp >> kRvLevels) * (kRvMels >> kRvLevels) * rv_ld(d.c0 << kRvLevels);
  for (int i = 0; i < kRvLevels; ++i) fl += (size_t)(Tp >> (kRvLevels - 1 - i)) * (kRvMels >> (kRvLevels - 1 - i)) * rv_ld(d.c0 << (kRvLevels - 1 - i));
  return fl + (size_t)Tp * kRvMels * 4 + (size_t)Tp * 2 * kRvHid;
}

// mel [rows_T, ld >= 128] time-major packed rows (frame offsets off) -> hidden [rows_T, 360] (optional) and f0 [rows_T] (optional)
inline int rmvpe_forward(const RvW& M, hipStream_t st, int n_utt, const int* off_host, const int* off_dev, const float* mel, int ld, float thred, float* hidden_out,
                         float* f0_out, float* taps, Arena& ws) {
  const RvDims& d = M.d;
  const long Tp = rv_padded(n_utt, off_host);
  int* offP = ws.get<int>(n_utt + 1);
  float* skip[kRvLevels];
  for (int l = 0; l < kRvLevels; ++l) skip[l] = ws.get<float>(rv_level_floats(M, Tp, l, d.c0 << l) + 64);
  float* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = ws.get<float>(rv_level_floats(M, Tp, 0, d.c0) + 64);
  const size_t pf = rv_partial_floats(M, Tp);
  float* part = ws.get<float>(pf + 64);
  float* cnn = ws.get<float>((size_t)Tp * 4 * kRvMels + 64);
  float* xi = ws.get<float>((size_t)Tp * 6 * kRvHid + 64);
  float* gru = ws.get<float>((size_t)Tp * 2 * kRvHid + 64);
  float* hp = ws.get<float>((size_t)Tp * kRvClasses + 64);
  STTS_CHECK(ws.ok, "rmvpe_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  hipLaunchKernelGGL(rv_offsets_kernel, dim3(1), dim3(64), 0, st, off_dev, n_utt, offP);
  RvRun r{st, offP, n_utt, Tp, part};
  float* tap = taps;
  auto keep = [&](const float* src, size_t n) -> int {
    if (tap) {
      STTS_HIP(hipMemcpyAsync(tap, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
      tap += n;
    }
    return 0;
  };
  // x: the running activation; `cur` is the rotating buffer that holds it (-1: none of them), the others are scratch
  const float* x = nullptr;
  int cur = -1;
  auto spare = [&](int k) -> float* {  // the k-th rotating buffer that does not hold x
    for (int i = 0; i < 4; ++i)
      if (i != cur && k-- == 0) return buf[i];
    return nullptr;
  };
  auto hold = [&](const float* p) {
    x = p;
    cur = -1;
    for (int i = 0; i < 4; ++i)
      if (buf[i] == p) cur = i;
  };
  // ---- encoder
  for (int l = 0; l < kRvLevels; ++l) {
    const int C = d.c0 << l;
    for (int b = 0; b < d.n_blocks; ++b) {
      float *h = spare(0), *s = spare(1);
      float* out = b == d.n_blocks - 1 ? skip[l] : spare(2);
      if (l == 0 && b == 0) {
        const long rows = Tp * kRvMels;
        hipLaunchKernelGGL(rv_conv0_kernel, dim3((unsigned)((rows * rv_ld(C) + 255) / 256)), dim3(256), 0, st, mel, ld, off_dev, offP, n_utt, rows, M.bn_a, M.bn_b, M.w0, M.b0,
                           M.wsc0, M.bsc0, C, rv_ld(C), h, s);
        STTS_TRY(rv_conv3(r, M.enc[0][0].c2, 0, h, nullptr, CONV_ACT_RELU, s, out));
      } else {
        STTS_TRY(rv_block(r, M.enc[l][b], l, x, nullptr, h, s, out));
      }
      hold(out);
    }
    // AvgPool2d(2) of the skip into a rotating buffer
    float* a = spare(0);
    const long ro = (Tp >> (l + 1)) * (kRvMels >> (l + 1));
    hipLaunchKernelGGL(rv_pool_kernel, dim3((unsigned)((ro * (rv_ld(C) / 4) + 255) / 256)), dim3(256), 0, st, skip[l], kRvMels >> (l + 1), ro, rv_ld(C), a);
    hold(a);
    STTS_TRY(keep(a, (size_t)ro * rv_ld(C)));
  }
  // ---- intermediate (level 5)
  for (int i = 0; i < d.inter_layers; ++i)
    for (int b = 0; b < d.n_blocks; ++b) {
      float* o = spare(2);
      STTS_TRY(rv_block(r, M.inter[i][b], kRvLevels, x, nullptr, spare(0), spare(1), o));
      hold(o);
    }
  STTS_TRY(keep(x, rv_level_floats(M, Tp, kRvLevels, d.c0 << kRvLevels)));
  // ---- decoder
  for (int i = 0; i < kRvLevels; ++i) {
    const int li = kRvLevels - i, lo = li - 1, C = d.c0 << lo;
    float* o = spare(2);
    for (int q = 0; q < 4; ++q) STTS_TRY(rv_launch(r, M.up[i][q], li, kRvMels >> li, 2, q >> 1, q & 1, x, nullptr, CONV_ACT_RELU, nullptr, o, rv_ld(C)));
    hold(o);
    for (int b = 0; b < d.n_blocks; ++b) {
      o = spare(2);
      STTS_TRY(rv_block(r, M.dec[i][b], lo, x, b == 0 ? skip[lo] : nullptr, spare(0), spare(1), o));
      hold(o);
    }
    STTS_TRY(keep(x, rv_level_floats(M, Tp, lo, C)));
  }
  // ---- cnn, BiGRU, head
  STTS_TRY(rv_launch(r, M.cnn, 0, kRvMels, 1, 0, 0, x, nullptr, CONV_ACT_NONE, nullptr, cnn, 4));
  STTS_TRY(keep(cnn, (size_t)Tp * kRvMels * 4));
  STTS_TRY(rv_launch(r, M.ih, 0, 1, 1, 0, 0, cnn, nullptr, CONV_ACT_NONE, nullptr, xi, 6 * kRvHid));
  hipLaunchKernelGGL(rv_gru_kernel, dim3(n_utt, 2), dim3(768), 0, st, xi, offP, M.whh, M.bhh, gru);
  STTS_TRY(keep(gru, (size_t)Tp * 2 * kRvHid));
  STTS_TRY(rv_launch(r, M.head, 0, 1, 1, 0, 0, gru, nullptr, CONV_ACT_SIGMOID, nullptr, hp, kRvClasses));
  int maxT = 0;
  for (int u = 0; u < n_utt; ++u) maxT = std::max(maxT, off_host[u + 1] - off_host[u]);
  float* hid = hidden_out;
  if (!hid) {  // the decode reads cropped rows
    hid = buf[0];
    STTS_CHECK(rv_level_floats(M, Tp, 0, d.c0) >= (size_t)off_host[n_utt] * kRvClasses, "rmvpe_forward: no room for the cropped salience");
  }
  hipLaunchKernelGGL(rv_crop_kernel, dim3((unsigned)std::min<long>(1024, ((long)maxT * kRvClasses + 255) / 256), n_utt), dim3(256), 0, st, hp, kRvClasses, off_dev, offP, hid);
  if (f0_out) {
    const long rows = off_host[n_utt];
    hipLaunchKernelGGL(rv_decode_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, hid, kRvClasses, rows, thred, f0_out);
  }
  STTS_HIP(hipGetLastError());
  return 0;
}

// workspace bytes for these host frame offsets: a dry run of the carving above
inline size_t rmvpe_workspace_bytes(const RvW& M, int n_utt, const int* off) {
  return dry_run_bytes([&](Arena a) { (void)rmvpe_forward(M, nullptr, n_utt, off, nullptr, nullptr, 0, 0.f, nullptr, nullptr, nullptr, a); });
}

}  // namespace stts

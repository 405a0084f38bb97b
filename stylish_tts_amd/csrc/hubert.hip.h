// HuBERT voice-conversion front ends: weight packing, kernels and stage orchestration.
//   HubertSpeechPredictor       models/speech_predictor.py:132-251  (phone_encoder + style_encoder; decoder .. generator = the frame path)
//   HubertEncoder               models/hubert_encoder.py:36-47      (input_cond_dim=None: no cond_proj, final_proj = Identity)
//   HubertPitchEnergyPredictor  models/pitch_energy_predictor.py:124-191
// Included by api.hip after model.hip.h (phoneme_model.hip.h: TextEncW, ProsodyW, encoder_layers_forward, prosody_forward, ...).
// Everything here runs fp32 on the f32 matrix cores whatever stts_set_precision chose, as the phoneme-rate predictors do.
#pragma once

namespace stts {

struct HubertSpW {  // STTS_W_HUBERT: hubert_speech_predictor.{phone_encoder, style_encoder}
  bool ready = false;
  int hubert_dim = 0, spk_dim = 0, h1 = 0, h2 = 0, sd = 0;
  PackedConv emb;  // phone_encoder.phone_emb (1x1, hubert_dim -> inter_dim)
  TextEncW enc;    // phone_encoder.encoder (layers only)
  float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;  // style_encoder.{0,3,6}, [out][in] fp32
};

struct HubertPeW {  // STTS_W_HUBERT_PE: hubert_pitch_energy_predictor.*
  bool ready = false;
  int hubert_dim = 0, spk_dim = 0, sd = 0, C = 0;
  PackedConv quant;  // phone_quant (1x1, hubert_dim -> inter_dim)
  float *ws = nullptr, *bs = nullptr;  // style_encoder (Linear spk_dim -> style_dim), [out][in] fp32
  ProsodyW pros;
  StyleTable table;
  AdainBlockW f0[3], n[3];
  float *f0_w = nullptr, *n_w = nullptr;
  float f0_b = 0.f, n_b = 0.f;
};

struct HubertModel {
  HubertSpW sp;
  HubertPeW pe;
};

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ float mish_torch(float v) { return v * tanhf(log1pf(expf(v))); }  // F.mish; v -> +inf: expf = inf, tanhf(inf) = 1: v

constexpr int kSpkChunk = 512;  // K per block of the speaker contraction (8 floats per lane)
constexpr int kSpkCols = 4;     // output columns per wave

// Stage 1 of the speaker styles: part[chunk][u][j] = sum over k in chunk of x[u][k] * W[j][k], j < na from Wa, na <= j < na + nb from Wb.
// Each wave keeps kSpkCols weight rows of its chunk in registers and streams every utterance's x past them, so the weights are read
// once per call.  The sum of one (u, j, chunk) is the same sequence of fp32 operations whatever n_utt is: an utterance's style is the
// same bit for bit alone and inside a batch.  grid (ceil((na + nb) / (4 * kSpkCols)), ceil(K / kSpkChunk)), block 256.
__global__ void __launch_bounds__(256) speaker_partial_kernel(const float* __restrict__ X, int ldx, int n_utt, int K, const float* __restrict__ Wa, int na,
                                                              const float* __restrict__ Wb, int nb, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = na + nb;
  const int j0 = (blockIdx.x * 4 + wave) * kSpkCols;
  if (j0 >= N) return;
  const int chunk = blockIdx.y, k0 = chunk * kSpkChunk;
  float w[kSpkCols][kSpkChunk / 64];
#pragma unroll
  for (int c = 0; c < kSpkCols; ++c) {
    const int j = j0 + c;
    const float* wr = j < na ? Wa + (long)j * K : (j < N ? Wb + (long)(j - na) * K : nullptr);
#pragma unroll
    for (int i = 0; i < kSpkChunk / 64; ++i) {
      const int k = k0 + i * 64 + lane;
      w[c][i] = (wr && k < K) ? wr[k] : 0.f;
    }
  }
  for (int u = 0; u < n_utt; ++u) {
    const float* x = X + (long)u * ldx;
    float xv[kSpkChunk / 64];
#pragma unroll
    for (int i = 0; i < kSpkChunk / 64; ++i) {
      const int k = k0 + i * 64 + lane;
      xv[i] = k < K ? x[k] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kSpkCols; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < kSpkChunk / 64; ++i) acc = fmaf(xv[i], w[c][i], acc);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);  // butterfly: every lane holds the same sum
      if (lane == 0 && j0 + c < N) part[((long)chunk * n_utt + u) * N + j0 + c] = acc;
    }
  }
}

// Stage 2, one block per utterance: the chunk sums in chunk order + bias; columns [0, na): Mish -> Linear(na -> n2) -> Mish ->
// Linear(n2 -> n3) -> style_out; columns [na, na + nb): pe_out (the one Linear of the pitch/energy predictor).  Fixed order throughout.
__global__ void __launch_bounds__(256) speaker_mlp_kernel(const float* __restrict__ part, int nchunk, int n_utt, int na, int nb, const float* __restrict__ ba,
                                                          const float* __restrict__ bb, const float* __restrict__ W2, const float* __restrict__ b2, int n2,
                                                          const float* __restrict__ W3, const float* __restrict__ b3, int n3, float* __restrict__ style_out,
                                                          int ld_style, float* __restrict__ pe_out, int ld_pe) {
  extern __shared__ float sh[];
  float* h1 = sh;       // [na]
  float* h2 = sh + na;  // [n2]
  const int u = blockIdx.x, N = na + nb;
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    float s = part[(long)u * N + j];
    for (int c = 1; c < nchunk; ++c) s += part[((long)c * n_utt + u) * N + j];
    if (j < na) h1[j] = mish_torch(s + ba[j]);
    else pe_out[(long)u * ld_pe + (j - na)] = s + bb[j - na];
  }
  if (na == 0) return;  // (uniform over the block)
  __syncthreads();
  for (int j = threadIdx.x; j < n2; j += blockDim.x) {
    const float* w = W2 + (long)j * na;
    float s = 0.f;
    for (int k = 0; k < na; ++k) s = fmaf(w[k], h1[k], s);
    h2[j] = mish_torch(s + b2[j]);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n3; j += blockDim.x) {
    const float* w = W3 + (long)j * n2;
    float s = 0.f;
    for (int k = 0; k < n2; ++k) s = fmaf(w[k], h2[k], s);
    style_out[(long)u * ld_style + j] = s + b3[j];
  }
}

// off4[i] = 4 * off[i]
__global__ void scale_offsets_kernel(const int* __restrict__ off, int n, int k, int* __restrict__ out) {
  for (int i = threadIdx.x; i <= n; i += blockDim.x) out[i] = k * off[i];
}

// phones.repeat_interleave(4, dim=2) after the 1x1 phone_emb (the two commute): y[4 offT[u] + 4t + r][c] = x[offT[u] + t][c], C % 4 == 0.
// grid (ceil(4 * max_len * C / 4 / 256), n_utt)
__global__ void __launch_bounds__(256) repeat_rows4_kernel(const float* __restrict__ X, int ldx, int C, const int* __restrict__ offT, float* __restrict__ Y,
                                                           int ldy) {
  const int u = blockIdx.y;
  const int r0 = offT[u], len = offT[u + 1] - r0;
  const int c4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)4 * len * c4) return;
  const int row4 = (int)(i / c4), c = (int)(i % c4) * 4;
  const float4 v = *reinterpret_cast<const float4*>(X + (long)(r0 + row4 / 4) * ldx + c);
  *reinterpret_cast<float4*>(Y + (long)(4 * r0 + row4) * ldy + c) = v;
}

// ------------------------------------------------------------------------------------------------ packing
inline int upload_linear(stts_ctx* c, const std::string& p, int* out_n, int* in_n, float** w, float** b) {
  STTS_GET(tw, p + ".weight");
  STTS_GET(tb, p + ".bias");
  STTS_CHECK(tw->shape.size() == 2 && (int64_t)tb->data.size() == tw->shape[0], "%s: expected a Linear weight [out, in] and bias [out]", p.c_str());
  *out_n = (int)tw->shape[0];
  *in_n = (int)tw->shape[1];
  STTS_TRY(dev_upload(c, tw->data, w));
  return dev_upload(c, tb->data, b);
}

inline int finalize_hubert(stts_ctx* c, HubertModel* M, int which) {
  const stts_model_dims& d = c->d;
  if (which & STTS_W_HUBERT) {
    c->pack.tag = STTS_W_HUBERT;
    HubertSpW& S = M->sp;
    S = HubertSpW();
    const std::string p = "hubert_speech_predictor.";
    STTS_GET(pe, p + "phone_encoder.phone_emb.weight");
    STTS_CHECK(pe->shape.size() == 3 && pe->shape[0] == d.inter_dim && pe->shape[2] == 1, "phone_emb must be a 1x1 conv to inter_dim (%d)", d.inter_dim);
    S.hubert_dim = (int)pe->shape[1];
    STTS_TRY(pack_plain(c, p + "phone_encoder.phone_emb", true, 0, S.hubert_dim, &S.emb));
    TextEncW& E = S.enc;
    E.C = d.inter_dim; E.inter = d.inter_dim; E.heads = d.te_heads; E.n_layers = d.te_layers; E.ffk = d.te_kernel; E.filter = d.te_filter;
    STTS_CHECK(E.C % 32 == 0 && E.C % E.heads == 0 && E.n_layers <= 16, "HuBERT encoder: inter_dim must be a multiple of 32 and of the heads, layers <= 16");
    STTS_TRY(pack_encoder_layers(c, p + "phone_encoder.encoder.", &E));
    E.ready = true;
    int in1 = 0, in2 = 0, in3 = 0;
    STTS_TRY(upload_linear(c, p + "style_encoder.0", &S.h1, &in1, &S.w1, &S.b1));
    STTS_TRY(upload_linear(c, p + "style_encoder.3", &S.h2, &in2, &S.w2, &S.b2));
    STTS_TRY(upload_linear(c, p + "style_encoder.6", &S.sd, &in3, &S.w3, &S.b3));
    STTS_CHECK(in2 == S.h1 && in3 == S.h2 && S.sd == d.style_dim, "hubert_speech_predictor.style_encoder: layer shapes do not chain to style_dim");
    S.spk_dim = in1;
    S.ready = true;
  }
  if (which & STTS_W_HUBERT_PE) {
    c->pack.tag = STTS_W_HUBERT_PE;
    HubertPeW& P = M->pe;
    P = HubertPeW();
    const std::string p = "hubert_pitch_energy_predictor.";
    STTS_GET(pq, p + "phone_quant.weight");
    STTS_CHECK(pq->shape.size() == 3 && pq->shape[0] == d.inter_dim && pq->shape[2] == 1, "phone_quant must be a 1x1 conv to inter_dim (%d)", d.inter_dim);
    P.hubert_dim = (int)pq->shape[1];
    STTS_TRY(pack_plain(c, p + "phone_quant", true, 0, P.hubert_dim, &P.quant));
    STTS_TRY(upload_linear(c, p + "style_encoder", &P.sd, &P.spk_dim, &P.ws, &P.bs));
    STTS_CHECK(P.sd == d.style_dim, "hubert_pitch_energy_predictor.style_encoder: %d outputs, style_dim is %d", P.sd, d.style_dim);
    STTS_TRY(pack_prosody(c, p + "prosody_encoder.", d.inter_dim, 3, &P.table, &P.pros));
    P.C = P.pros.C;
    for (int i = 0; i < 3; ++i) {
      STTS_TRY(pack_adain_block(c, p + "F0." + std::to_string(i), P.C, P.C, &P.table, &P.f0[i]));
      STTS_TRY(pack_adain_block(c, p + "N." + std::to_string(i), P.C, P.C, &P.table, &P.n[i]));
    }
    STTS_TRY(upload_table(c, &P.table));
    STTS_TRY(upload_vec(c, p + "F0_proj.weight", &P.f0_w));
    STTS_TRY(upload_vec(c, p + "N_proj.weight", &P.n_w));
    STTS_GET(fb, p + "F0_proj.bias");
    STTS_GET(nb, p + "N_proj.bias");
    P.f0_b = fb->data[0];
    P.n_b = nb->data[0];
    P.ready = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ speaker styles
// spk_emb [n_utt, ld >= spk_dim] -> style_out [n_utt, 64] (hubert_speech_predictor.style_encoder) and / or pe_style_out [n_utt, 64]
// (hubert_pitch_energy_predictor.style_encoder); a null output is skipped (its component need not be finalized).
inline int speaker_style(stts_ctx* c, const HubertModel& M, hipStream_t st, int n_utt, const float* spk, int ld, float* style_out, float* pe_out, Arena& ws) {
  const HubertSpW& S = M.sp;
  const HubertPeW& P = M.pe;
  const bool want_sp = style_out != nullptr, want_pe = pe_out != nullptr;
  if (!want_sp && !want_pe) return 0;
  const int K = want_sp ? S.spk_dim : P.spk_dim;
  STTS_CHECK(!(want_sp && want_pe) || S.spk_dim == P.spk_dim, "speaker embedding width: the two style encoders take %d and %d", S.spk_dim, P.spk_dim);
  STTS_CHECK(ld >= K, "speaker embedding: ld %d < spk_dim %d", ld, K);
  const int na = want_sp ? S.h1 : 0, nb = want_pe ? P.sd : 0, N = na + nb;
  const int nchunk = ceil_div(K, kSpkChunk);
  float* part = ws.get<float>((size_t)n_utt * nchunk * N);
  STTS_CHECK(ws.ok, "speaker_style: workspace too small");
  STTS_DRY_RETURN(ws);
  hipLaunchKernelGGL(speaker_partial_kernel, dim3(ceil_div(N, 4 * kSpkCols), nchunk), dim3(256), 0, st, spk, ld, n_utt, K, want_sp ? S.w1 : nullptr, na,
                     want_pe ? P.ws : nullptr, nb, part);
  const size_t shm = (size_t)(na + (want_sp ? S.h2 : 0)) * sizeof(float);
  hipLaunchKernelGGL(speaker_mlp_kernel, dim3(n_utt), dim3(256), shm, st, part, nchunk, n_utt, na, nb, want_sp ? S.b1 : nullptr, want_pe ? P.bs : nullptr,
                     want_sp ? S.w2 : nullptr, want_sp ? S.b2 : nullptr, want_sp ? S.h2 : 0, want_sp ? S.w3 : nullptr, want_sp ? S.b3 : nullptr,
                     want_sp ? S.sd : 0, style_out, want_sp ? S.sd : 0, pe_out, want_pe ? P.sd : 0);
  STTS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------ HubertEncoder.forward
// feats [rows_T, ld_f >= hubert_dim] (utterance offsets sT) -> asr [4 rows_T, ld_asr >= inter_dim]: phone_emb at T rows, each row
// written 4 times (phones.repeat_interleave(4) commutes with the 1x1 conv), then the Encoder at 4T rows masked by 4 * lengths.
inline int hubert_encoder_forward(stts_ctx* c, const HubertModel& M, hipStream_t st, const Seg& sT, const float* feats, int ld_f, float* asr, int ld_asr, Arena& ws) {
  const HubertSpW& S = M.sp;
  const TextEncW& E = S.enc;
  const int C = E.C;
  const long RT = sT.rows(), R4 = 4 * RT;
  std::vector<int> host4(sT.n_utt + 1);
  for (int u = 0; u <= sT.n_utt; ++u) host4[u] = 4 * sT.host[u];
  int* dev4 = ws.get<int>(sT.n_utt + 1);
  float* e = ws.get<float>(RT * C);
  float* x = ws.get<float>(R4 * C);
  float* t = ws.get<float>(R4 * C);
  float* qkv = ws.get<float>(R4 * 3 * C);
  float* att = ws.get<float>(R4 * C);
  float* ff = ws.get<float>(R4 * E.filter);
  STTS_CHECK(ws.ok, "hubert_encoder_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  Seg s4{sT.n_utt, host4.data(), dev4};
  hipLaunchKernelGGL(scale_offsets_kernel, dim3(1), dim3(256), 0, st, sT.dev, sT.n_utt, 4, dev4);
  STTS_TRY(gemm_store(st, sT, feats, ld_f, 0, S.emb, e, C, 0));
  hipLaunchKernelGGL(repeat_rows4_kernel, dim3(std::max(1, ceil_div(sT.max_len() * C, 256)), sT.n_utt), dim3(256), 0, st, e, C, C, sT.dev, x, C);
  STTS_TRY(encoder_layers_forward(st, E, s4, x, t, qkv, att, ff));
  STTS_HIP(hipMemcpy2DAsync(asr, (size_t)ld_asr * sizeof(float), x, (size_t)C * sizeof(float), (size_t)C * sizeof(float), R4, hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------ HubertPitchEnergyPredictor.forward
// feats [rows_T, ld_f], pe_style [n_utt, 64] -> f0, energy [rows_T]; optional prosody tap [rows_T, C = inter_dim + style_dim].
inline int hubert_pitch_energy_forward(stts_ctx* c, const HubertModel& M, hipStream_t st, const Seg& s, const float* feats, int ld_f, const float* pe_style,
                                       float* f0, float* nrg, float* prosody_out, Arena& ws) {
  (void)c;
  const HubertPeW& P = M.pe;
  const long R = s.rows();
  const int C = P.C, d = P.pros.d;
  float* q = ws.get<float>(R * d);
  float* pros = prosody_out ? prosody_out : ws.get<float>(R * C);
  float* sty = ws.get<float>((size_t)s.n_utt * P.table.ld());
  int* row_utt = ws.get<int>(R);
  float* t1 = ws.get<float>(R * C);
  float* t2 = ws.get<float>(R * C);
  BlockIO io;
  io.act1 = ws.get<float>(R * C);
  io.hbuf = ws.get<float>(R * C);
  io.act2 = ws.get<float>(R * C);
  io.ss = ws.get<float>(adain_part_floats(s, C));
  // large batches: Winograd convs (as the text predictor's blocks), every norm on its own statistics pass
  const BlockSwitches sw = block_switches();
  const ChainPlan plan = plan_adain_chain(s, PREC_F32, P.f0, 3, 0, ChainOffer{false, false, false, false}, sw);
  WinoScratch wino;
  if (plan.wino) wino.p = ws.get<float>(wino_scratch_floats(s, P.f0[0].w1));
  STTS_CHECK(ws.ok, "hubert_pitch_energy_forward: workspace too small");
  const int lds = P.table.ld();
  auto prosody = [&]() { Arena a = ws.rest(); return prosody_forward(st, P.pros, s, q, d, pe_style, sty, lds, row_utt, pros, a); };
  {
    DryScope dry;
    STTS_TRY(prosody());
  }
  STTS_DRY_RETURN(ws);
  launch_row_utt(st, s, row_utt);
  STTS_TRY(gemm_store(st, s, feats, ld_f, 0, P.quant, q, d, 0));
  STTS_TRY(run_style(st, P.table, pe_style, s.n_utt, sty));
  STTS_TRY(prosody());
  io.style = sty; io.ld_style = lds; io.ldx = io.ldy = C; io.wino = &wino;
  BlockChain chain(plan, nullptr);
  for (int br = 0; br < 2; ++br) {
    const AdainBlockW* blocks = br == 0 ? P.f0 : P.n;
    const float* cur = pros;
    float* bufs[2] = {t1, t2};
    for (int i = 0; i < 3; ++i) {
      io.x = cur; io.y = bufs[i & 1];
      STTS_TRY(adain_block(st, s, blocks[i], io, chain, sw));
      cur = bufs[i & 1];
    }
    const ChanConvSet cs{cur, br == 0 ? P.f0_w : P.n_w, br == 0 ? P.f0_b : P.n_b, br == 0 ? f0 : nrg};
    STTS_TRY(launch_single_channel_conv(st, s, 0, 1, cs, cs, C, C, 1, 1, 0));
  }
  STTS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace
// Bytes that the three entry points above accept for `rows_T` feature frames in `n_utt` utterances, the longest of `max_len` frames:
// the largest of their dry runs (speaker_style with both style encoders, where finalized; rows_T = 0: speaker_style alone).
inline size_t hubert_workspace_bytes(const stts_ctx* cc, int64_t rows_T, int n_utt, int max_len) {
  stts_ctx* c = const_cast<stts_ctx*>(cc);
  if (!c || !c->hubert || n_utt <= 0) return 0;
  const bool frames = rows_T > 0 && max_len > 0;
  const HubertModel& M = *static_cast<const HubertModel*>(c->hubert.get());
  const SynthSeg syn(rows_T, n_utt, max_len);
  const Seg s = syn.seg();
  return dry_run_bytes([&](Arena a) {
    Arena e = a, p = a;
    float* const wanted = reinterpret_cast<float*>(a.base);  // (an output that is asked for; never written)
    float* const sp = M.sp.ready ? wanted : nullptr;
    float* const pe = M.pe.ready ? wanted : nullptr;
    Arena k0 = a, k1 = a, k2 = a;  // each style alone, and the two in one call (refused when their speaker widths differ)
    (void)speaker_style(c, M, nullptr, n_utt, nullptr, 1 << 30, sp, nullptr, k0);
    (void)speaker_style(c, M, nullptr, n_utt, nullptr, 1 << 30, nullptr, pe, k1);
    (void)speaker_style(c, M, nullptr, n_utt, nullptr, 1 << 30, sp, pe, k2);
    if (frames && M.sp.ready) (void)hubert_encoder_forward(c, M, nullptr, s, nullptr, 0, nullptr, 0, e);
    if (frames && M.pe.ready) (void)hubert_pitch_energy_forward(c, M, nullptr, s, nullptr, 0, nullptr, nullptr, nullptr, nullptr, p);
  });
}

}  // namespace stts

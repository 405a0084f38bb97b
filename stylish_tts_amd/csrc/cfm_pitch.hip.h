// CfmPitchPredictor's frame-rate network (models/cfm/cfm_pitch_predictor.py:12-51): weight packing, kernels and orchestration.
//   asr [rows, asr_dim] -> asr_emb (1x1 -> Mish -> 1x1) -> 4 x generator ConvNeXtBlock(256, 1024, style 256, k 7) -> out_proj (256 -> 1)
// The speaker branch (spk_emb, a MelStyleEncoder) is component STTS_W_CFM_PITCH (mel_style.hip.h); its style is an input here, so the
// caller may run it on another stream.  Optionally fused: denorm_f0_zscore (train/stage_type.py:801-829).
// Included by api.hip after model.hip.h, cfm.hip.h (mishf) and mel_style.hip.h.  Everything runs fp32 on the f32 matrix cores whatever
// stts_set_precision chose, as the HuBERT and mel-style paths do.
#pragma once

namespace stts {

// The kernels here carry STTS_NO_PK: they run beside the split-fp32 contractions on other streams.
constexpr int kCpHidden = 256;  // hidden_dim, hard-coded in the reference
constexpr int kCpInter = 1024;  // hidden_dim * 4
constexpr int kCpBlocks = 4;
constexpr int kCpTaps = 7;      // generator.ConvNeXtBlock's default kernel_size

struct CfmPitchNetW {  // STTS_W_CFM_PITCH_NET: cfm_pitch_predictor.{asr_emb, blocks, out_proj} (in_proj is unused by forward)
  bool ready = false;
  int asr_dim = 0;
  PackedConv emb0, emb2;  // asr_emb.0 (asr_dim -> 1024), asr_emb.2 (1024 -> 256)
  ConvNextW blk[kCpBlocks];
  StyleTable table;       // the four blocks' norm.fc, K = 256 (the speaker style)
  float* out_w = nullptr;  // out_proj.weight [256]
  float out_b = 0.f;
};

// ------------------------------------------------------------------------------------------------ kernels
// in place: X[r][0, C) = mish(X[r][0, C)) over the utterances' rows (bounds from the device offsets); C % 4 == 0.
// grid (ceil(max_len * C / 4 / 256) capped, n_utt)
__global__ void STTS_NO_PK __launch_bounds__(256) cp_mish_rows_kernel(float* __restrict__ X, int ldx, int C, const int* __restrict__ seg_off) {
  const int u = blockIdx.y;
  const int lo = seg_off[u], len = seg_off[u + 1] - lo;
  const int c4 = C / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)len * c4; i += (long)gridDim.x * 256) {
    float* p = X + (long)(lo + i / c4) * ldx + (i % c4) * 4;
    float4 v = *reinterpret_cast<float4*>(p);
    v.x = mishf(v.x); v.y = mishf(v.y); v.z = mishf(v.z); v.w = mishf(v.w);
    *reinterpret_cast<float4*>(p) = v;
  }
}

// style projections with a wide style (K = 256: style_fc_kernel covers K <= 128): out[u][j] = b[j] + sum_k W[j][k] s[u][k], one wave per
// row j, lane-strided partial sums then the butterfly - the same operations for an utterance whatever n_utt is.  grid ceil(J / 4), block 256.
__global__ void STTS_NO_PK __launch_bounds__(256) cp_style_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ s,
                                                                    float* __restrict__ out, int J, int K, int n_utt, int lds_s, int ld_out) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= J) return;
  const float* w = W + (long)j * K;
  for (int u = 0; u < n_utt; ++u) {
    const float* x = s + (long)u * lds_s;
    float v = 0.f;
    for (int k = lane; k < K; k += 64) v = fmaf(w[k], x[k], v);
    v = wave_sum(v);
    if (lane == 0) out[(long)u * ld_out + j] = v + b[j];
  }
}

// out_proj (Conv1d(256, 1, 1)) as one dot product per row, a wave per row (each lane one float4 of the row per 256 channels), reading
// the last block's rows once; optionally denorm_f0_zscore fused: hz = clamp(2^(x * std + mean), 50, 1200), 0 where uv > 0.
// The product x * std and the sum are rounded separately (no FMA), as torch evaluates the reference's expression; 2^a is formed in double
// and rounded to fp32 once (correctly rounded but for ties; torch's own fp32 2**a is within 1 ulp of that).
// grid (ceil(max_len / 4), n_utt), block 256 = 4 rows.
__global__ void STTS_NO_PK __launch_bounds__(256) cp_out_kernel(const float* __restrict__ X, int ldx, int C, const int* __restrict__ seg_off,
                                                                  const float* __restrict__ w, float bias, float* __restrict__ normed,
                                                                  float* __restrict__ hz, float mean, float stdv, const float* __restrict__ uv) {
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int lo = seg_off[u], len = seg_off[u + 1] - lo;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= len) return;
  const long r = lo + t;
  const float* x = X + r * ldx;
  float acc = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(x + c);
    const float4 b = *reinterpret_cast<const float4*>(w + c);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  acc = wave_sum(acc);
  if (lane != 0) return;
  const float y = acc + bias;
  normed[r] = y;
  if (hz) {
#pragma clang fp contract(off)
    const float a = y * stdv + mean;  // (two roundings: with the default contraction this was one FMA, 1 ulp of a = 3-6 ulp of hz)
    float f = (float)exp2((double)a);
    f = fminf(fmaxf(f, 50.0f), 1200.0f);
    if (uv && uv[r] > 0.f) f = 0.f;
    hz[r] = f;
  }
}

// ------------------------------------------------------------------------------------------------ packing
// dims from the weights: asr_dim = asr_emb.0's cin; hidden 256 / 1024 checked (models/cfm/cfm_pitch_predictor.py:14-19)
inline int finalize_cfm_pitch_net(stts_ctx* c, CfmPitchNetW* W) {
  *W = CfmPitchNetW();
  const std::string p = "cfm_pitch_predictor.";
  STTS_GET(e0, p + "asr_emb.0.weight");
  STTS_GET(e2, p + "asr_emb.2.weight");
  STTS_CHECK(e0->shape.size() == 3 && e0->shape[0] == kCpInter && e0->shape[2] == 1, "%sasr_emb.0: expected a [%d, asr_dim, 1] Conv1d", p.c_str(), kCpInter);
  STTS_CHECK(e2->shape.size() == 3 && e2->shape[0] == kCpHidden && e2->shape[1] == kCpInter && e2->shape[2] == 1, "%sasr_emb.2: expected a [%d, %d, 1] Conv1d",
             p.c_str(), kCpHidden, kCpInter);
  W->asr_dim = (int)e0->shape[1];
  STTS_TRY(pack_plain(c, p + "asr_emb.0", true, 0, W->asr_dim, &W->emb0));
  STTS_TRY(pack_plain(c, p + "asr_emb.2", true, 0, kCpInter, &W->emb2));
  W->table.K = kCpHidden;
  for (int i = 0; i < kCpBlocks; ++i) {
    const std::string q = p + "blocks." + std::to_string(i) + ".";
    STTS_GET(p1, q + "pwconv1.weight");
    STTS_CHECK(p1->shape.size() == 2 && p1->shape[0] == kCpInter && p1->shape[1] == kCpHidden, "%spwconv1: expected [%d, %d]", q.c_str(), kCpInter, kCpHidden);
    STTS_GET(fc, q + "norm.fc.weight");
    STTS_CHECK(fc->shape.size() == 2 && fc->shape[1] == kCpHidden, "%snorm.fc: expected a style of %d", q.c_str(), kCpHidden);
    STTS_TRY(pack_convnext_block(c, q, kCpHidden, kCpTaps, &W->table, &W->blk[i]));
  }
  STTS_TRY(upload_table(c, &W->table));
  STTS_GET(ow, p + "out_proj.weight");
  STTS_GET(ob, p + "out_proj.bias");
  STTS_CHECK(ow->shape.size() == 3 && ow->shape[0] == 1 && ow->shape[1] == kCpHidden && ow->shape[2] == 1 && ob->data.size() == 1, "%sout_proj: expected [1, %d, 1]",
             p.c_str(), kCpHidden);
  STTS_TRY(dev_upload(c, ow->data, &W->out_w));
  W->out_b = ob->data[0];
  W->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ CfmPitchPredictor.forward (frame-rate part)
// asr [rows, ld_asr >= asr_dim] packed by s, spk [n_utt, 256] (the spk_emb style) -> normed [rows] (out_proj), optionally hz [rows]
// (denorm_f0_zscore with the given log2 statistics and uv [rows] or null).  taps (or null): [5][rows][256] = asr_emb output, then each block's.
inline int cfm_pitch_forward(const CfmPitchNetW& W, hipStream_t st, const Seg& s, const float* asr, int ld_asr, const float* spk, float* normed, float* hz,
                             float mean, float stdv, const float* uv, float* taps, Arena& ws) {
  const long R = s.rows();
  const int h = kCpHidden, inter = kCpInter, ml = s.max_len();
  const int ss_stride = ceil_div(ml, 128) * 4;
  float* U = ws.get<float>(R * inter);
  float* xa = ws.get<float>(R * h);
  float* xb = ws.get<float>(R * h);
  float* nrm = ws.get<float>(R * h);
  float* part = ws.get<float>((size_t)s.n_utt * ss_stride * inter);
  float* gscale = ws.get<float>((size_t)s.n_utt * inter);
  float* w2u = ws.get<float>((size_t)s.n_utt * W.blk[0].pw2.npad * inter);
  float* sty = ws.get<float>((size_t)s.n_utt * W.table.ld());
  STTS_CHECK(ws.ok, "cfm_pitch_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  // asr_emb: 1x1 -> Mish (a pass of its own: the shared contraction epilogue stays as it is) -> 1x1
  STTS_TRY(gemm_store(st, s, asr, ld_asr, 0, W.emb0, U, inter, 0));
  hipLaunchKernelGGL(cp_mish_rows_kernel, dim3((unsigned)std::min(1024, std::max(1, ceil_div(ml * (inter / 4), 256))), s.n_utt), dim3(256), 0, st, U, inter, inter,
                     s.dev);
  float* cur = taps ? taps : xa;
  STTS_TRY(gemm_store(st, s, U, inter, 0, W.emb2, cur, h, 0));
  hipLaunchKernelGGL(cp_style_kernel, dim3(ceil_div(W.table.J, 4)), dim3(256), 0, st, W.table.W, W.table.b, spk, sty, W.table.J, W.table.K, s.n_utt, h,
                     W.table.ld());
  // the generator's ConvNeXt blocks (fp32 weights without split planes: pwconv2 on per-utterance GRN-scaled copies); row_utt is not
  // needed, 256 channels and k = 7 always take dwconv_ln_kernel
  const ConvNextScratch cs{nullptr, nrm, U, part, ss_stride, gscale, w2u, nullptr};
  for (int i = 0; i < kCpBlocks; ++i) {
    float* nxt = taps ? taps + (size_t)(i + 1) * R * h : (cur == xa ? xb : xa);
    STTS_TRY(convnext_block_forward(st, s, W.blk[i], h, inter, sty, W.table.ld(), 0, cur, nxt, cs));
    cur = nxt;
  }
  hipLaunchKernelGGL(cp_out_kernel, dim3(ceil_div(ml, 4), s.n_utt), dim3(256), 0, st, cur, h, h, s.dev, W.out_w, W.out_b, normed, hz, mean, stdv, uv);
  STTS_HIP(hipGetLastError());
  return 0;
}

// Workspace bytes from the row count alone: a dry run with one utterance holding all the rows the others leave (the GRN partial sums
// grow with the longest utterance).
inline size_t cfm_pitch_workspace_bytes(const CfmPitchNetW& W, int64_t rows_T, int n_utt) {
  const SynthSeg syn(rows_T, n_utt, 0);
  return dry_run_bytes([&](Arena a) { (void)cfm_pitch_forward(W, nullptr, syn.seg(), nullptr, 0, nullptr, nullptr, nullptr, 0.f, 1.f, nullptr, nullptr, a); });
}

}  // namespace stts

// The posterior encoder (models/flow.py:234-293): recording -> STFT -> pre_spec | pre_phase -> 12-layer WaveNet (flow.py:17-88, k = 3) ->
// proj_mean | proj_logstd -> z = mean + noise * exp(logstd) [-> post_flow].  Component STTS_W_POSTERIOR, keys "speech_predictor.posterior_encoder.*".
// Included by api.hip after model.hip.h (context, packers, contraction launchers; vocoder.hip.h: launch_stft).  plan_posterior() chooses the WaveNet form of a
// call, posterior_forward() walks the stage.  fp32 whatever the engine's precision.
//
// wn_post_kernel<RT, LAST>: one WaveNet layer in one launch, the structure of wn_fused_kernel's direct form (wn_fused.hip.h, M = 1) with TAPS = 3, PAD = 1 and
// no coupling tail - a separate kernel: it shares no kernel code with the reverse flow's (it uses that family's unchanged helpers: pack_fragments,
// mfma4, wn_dispatch, kWnSegInline, seg_blocks):
//   x_in = wn-conv1d k3 (h)  128 -> 256 ; acts = tanh(x_in[:128] + g[:128]) * sigmoid(x_in[128:] + g[128:]) ; rs = wn-Linear(acts)  128 -> 256 (last: 128)
//   h += rs[:128] ; out (+)= rs[128:]            (last layer: out += rs, h is left alone)
// A block is RT tiles of 16 consecutive rows of ONE utterance; its rows and one halo row each side sit in LDS in MFMA-fragment order (row r of the
// block's window at tile r >> 4, slot r & 15), so tap j of row tile rt is the same image read one slot further: no per-tap copies, no barrier in the K
// loop.  v_mfma_f32_16x16x4_f32 on fp32 operands: at one wave per SIMD a block's time is its MFMA chain (~9 us per 16-row tile measured, plan_posterior
// below), and the split-fp32 form would issue three products per fp32 one and stream three times the weight bytes (0.5 MB per layer in fp32) for the
// same fp32-grade result.  Wave w of 4 owns the tanh and sigmoid
// tiles of channels [32 w, 32 w + 32); weights arrive in fragment order (packed at finalize) with coalesced 16-byte loads one 16-channel block ahead.
#pragma once

namespace stts {

constexpr int kPostC = 128;      // hidden channels the fused kernel is built for (decoder.hidden_dim / 4)
constexpr int kPostTaps = 3;     // ... and its kernel size
constexpr int kPostWaves = 4;

struct WnPostArgs {
  const float* Hin;    // [rows, 128]
  float* Hout;         // [rows, 128], another buffer than Hin: neighbouring blocks still read their halo rows (unused when LAST)
  float* Out;          // [rows, 128], updated in place (read when out_acc)
  const int* seg_off;
  const float* W1;     // in_layers, fragments [4 waves][8 blocks][3 taps][2 halves][2 tiles][64 lanes][4]
  const float* b1;     // [256] natural order: tanh rows 0..127 | sigmoid rows 128..255
  const float* W2;     // res_skip, fragments [4][8][4 (LAST: 2)][64][4]
  const float* b2;     // [256] (LAST: [128])
  const float* gate;   // [n_utt][ld_gate]: the utterance's cond row
  int ld_gate, gcol0;
  int out_acc;         // accumulate into Out (0 on the first layer)
  int n_inline;        // > 0: seg_inline holds the n_inline + 1 utterance offsets (seg_off is not read)
  int seg_inline[kWnSegInline + 1];
};

template <int RT, bool LAST>
__global__ void __launch_bounds__(256) wn_post_kernel(const WnPostArgs a) {
  constexpr int ROWS = 16 * RT, C = kPostC, KB = C / 16, NW = kPostWaves, CT = C / NW / 16, TAPS = kPostTaps;
  constexpr int NCT = LAST ? CT : 2 * CT;       // res/skip column tiles per wave
  __shared__ f32x4 Af[(RT + 1) * KB * 64];  // rows [row0 - 1, row0 + ROWS + 1) in fragment order [tile][block][lane]; slots from ROWS + 2 on are never read
  __shared__ f32x4 A2[RT * KB * 64];        // gated activations [row tile][block][lane]

  const int utt = blockIdx.y;
  const int lo = a.n_inline ? a.seg_inline[utt] : a.seg_off[utt], hi = a.n_inline ? a.seg_inline[utt + 1] : a.seg_off[utt + 1];
  const int row0 = lo + blockIdx.x * ROWS;
  if (row0 >= hi) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int nvalid = hi - row0;

  // ---- phase-1 weight stream: wave w reads its own slice [8 blocks][3 taps][2 halves][CT] fragments (1 KB each) one block ahead of the MFMAs
  constexpr int T1 = TAPS * 2 * CT;
  const f32x4* w1 = reinterpret_cast<const f32x4*>(a.W1) + (size_t)w * KB * (T1 * 64) + lane;
  f32x4 bq0[T1], bq1[T1];
  auto load1 = [&](f32x4(&dst)[T1], int u) {
#pragma unroll
    for (int j = 0; j < T1; ++j) dst[j] = w1[(u * T1 + j) * 64];
  };
  load1(bq0, 0);
  __builtin_amdgcn_sched_barrier(0);

  // ---- prologue: the block's rows and one halo row each side; rows outside the utterance are its zero padding
  for (int e = tid; e < (ROWS + 2) * (C / 4); e += 256) {
    const int r = e / (C / 4), cq = e % (C / 4);
    const int row = row0 - 1 + r;
    const bool ok = row >= lo && row < hi;
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.Hin + (long)min(max(row, lo), hi - 1) * C + 4 * cq);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    Af[((r >> 4) * KB + (cq >> 2)) * 64 + (cq & 3) * 16 + (r & 15)] = ok ? v : z;
  }
  // Orientation as in wn_fused_kernel: D^T = W x A^T, a lane holds four consecutive channels (4 lq + i of the tile) of one row (l15).
  f32x4 ba[CT], bb[CT], ga[CT], gb[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int ch = (C / NW) * w + 16 * c + 4 * lq;
    ba[c] = *reinterpret_cast<const f32x4*>(a.b1 + ch);
    bb[c] = *reinterpret_cast<const f32x4*>(a.b1 + C + ch);
    ga[c] = *reinterpret_cast<const f32x4*>(a.gate + (long)utt * a.ld_gate + a.gcol0 + ch);
    gb[c] = *reinterpret_cast<const f32x4*>(a.gate + (long)utt * a.ld_gate + a.gcol0 + C + ch);
  }
  __syncthreads();

  // ---- phase 1: RT row tiles x (tanh, sigmoid) x CT tiles, K = 3 taps x 128 channels in 8 blocks of 16 (4 MFMA k-steps each)
  f32x4 acc[RT][2][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[rt][h][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step1 = [&](int t, const f32x4(&cur)[T1]) {
    f32x4 av[TAPS][RT];
#pragma unroll
    for (int j = 0; j < TAPS; ++j)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int rr = 16 * rt + l15 + j;  // window row of (output row 16 rt + l15, tap j)
        av[j][rt] = Af[((rr >> 4) * KB + t) * 64 + lq * 16 + (rr & 15)];
      }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < TAPS; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][h][c] = mfma4(cur[(j * 2 + h) * CT + c][s], av[j][rt][s], acc[rt][h][c]);
  };
  auto interleave = [&]() {  // the T1 loads of the next block go between this block's MFMAs, one per four
#pragma unroll
    for (int q = 0; q < T1; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll 1
  for (int it = 0; it < KB / 2; ++it) {
    load1(bq1, 2 * it + 1);
    step1(2 * it, bq0);
    interleave();
    if (2 * it + 2 < KB) load1(bq0, 2 * it + 2);
    step1(2 * it + 1, bq1);
    interleave();
  }

  // ---- phase-2 operands requested now: this wave's res/skip weights, bias, the h / out values the epilogue updates (rows past the utterance's
  // end read row0 instead and are never stored)
  const f32x4* w2 = reinterpret_cast<const f32x4*>(a.W2) + (size_t)w * KB * (NCT * 64) + lane;
  f32x4 cq2[KB][NCT];
#pragma unroll
  for (int t = 0; t < KB; ++t)
#pragma unroll
    for (int c = 0; c < NCT; ++c) cq2[t][c] = w2[(t * NCT + c) * 64];
  f32x4 bv[NCT], old[RT][NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int n = 16 * NCT * w + 16 * c + 4 * lq;  // first of this lane's four res/skip output columns of tile c
    bv[c] = *reinterpret_cast<const f32x4*>(a.b2 + n);
    const bool to_h = !LAST && n < C;
    const int col = (!LAST && n >= C) ? n - C : n;
    const float* src = to_h ? a.Hin : a.Out;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rl = 16 * rt + l15;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (long)(row0 + (rl < nvalid ? rl : 0)) * C + col);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      old[rt][c] = (to_h || a.out_acc) ? v : z;
    }
  }

  // ---- gate: written to LDS as the B operand of res/skip (tanhf / __expf: the arithmetic of the contractions' EPI_GATE)
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 va = acc[rt][0][c] + ba[c] + ga[c], vb = acc[rt][1][c] + bb[c] + gb[c];
      f32x4 act;
#pragma unroll
      for (int i = 0; i < 4; ++i) act[i] = tanhf(va[i]) * (1.0f / (1.0f + __expf(-vb[i])));
      A2[(rt * KB + CT * w + c) * 64 + lq * 16 + l15] = act;
    }
  __syncthreads();

  // ---- phase 2: res/skip, K = 128 from LDS; wave w owns columns [16 NCT w, 16 NCT (w + 1)), all row tiles
  f32x4 acc2[RT][NCT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc2[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    f32x4 av[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) av[rt] = A2[(rt * KB + t) * 64 + lane];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc2[rt][c] = mfma4(cq2[t][c][s], av[rt][s], acc2[rt][c]);
  }

#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int n = 16 * NCT * w + 16 * c + 4 * lq;
    const bool to_h = !LAST && n < C;
    const int col = (!LAST && n >= C) ? n - C : n;
    float* dst = to_h ? a.Hout : a.Out;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (16 * rt + l15 < nvalid) *reinterpret_cast<f32x4*>(dst + (long)(row0 + 16 * rt + l15) * C + col) = old[rt][c] + (acc2[rt][c] + bv[c]);
  }
}

// ------------------------------------------------------------------------------------------------ weights
struct PostW {
  int hidden = 0, out_ch = 0, ksize = 0, n_layers = 0, bins = 0;
  PackedConv pre_spec, pre_phase;     // Conv1d k = 1, bins -> hidden / 2
  StyleTable cond;                    // enc.cond_layer: [2 hidden n_layers][style]
  bool has_cond = false;
  std::vector<PackedConv> in, rs;     // the generic form: paired k-tap conv (EPI_GATE), res/skip (EPI_SPLIT_ACC)
  PackedConv prior, pmean, plogstd;   // proj_mean | proj_logstd paired (EPI_PRIOR), and each alone (the optional mean / logstd outputs)
  std::vector<float*> W1, b1, W2, b2; // wn_post_kernel's fragments (hidden 128, k = 3)
  bool fused = false;
};

inline int finalize_posterior(stts_ctx* c, PostW* P) {
  *P = PostW();
  const std::string p = "speech_predictor.posterior_encoder.";
  const int bins = c->geom.bins;
  P->bins = bins;
  HostTensor ws_, wp_;
  STTS_TRY(get_weight(c, p + "pre_spec", &ws_));
  STTS_TRY(get_weight(c, p + "pre_phase", &wp_));
  STTS_CHECK(ws_.shape.size() == 3 && ws_.shape[1] == bins && ws_.shape[2] == 1 && wp_.shape == ws_.shape,
             "posterior_encoder.pre_spec / pre_phase: expected [hidden / 2, %d, 1] (n_fft / 2 + 1 input channels)", bins);
  const int H = 2 * (int)ws_.shape[0];
  P->hidden = H;
  STTS_CHECK(H > 0 && H % 32 == 0, "posterior_encoder: hidden_channels %d must be a multiple of 32", H);
  STTS_TRY(pack_plain(c, p + "pre_spec", true, 0, bins, &P->pre_spec));
  STTS_TRY(pack_plain(c, p + "pre_phase", true, 0, bins, &P->pre_phase));
  while (find(c, p + "enc.in_layers." + std::to_string(P->n_layers) + ".bias")) ++P->n_layers;
  STTS_CHECK(P->n_layers > 0, "missing weight '%senc.in_layers.0.bias'", p.c_str());
  P->cond = StyleTable();
  P->cond.K = c->d.style_dim;
  if (find(c, p + "enc.cond_layer.bias")) {
    HostTensor cw;
    STTS_TRY(get_weight(c, p + "enc.cond_layer", &cw));
    STTS_GET(cb, p + "enc.cond_layer.bias");
    STTS_CHECK(cw.shape[0] == 2 * H * P->n_layers && cw.shape[1] == c->d.style_dim && (int)cb->data.size() == 2 * H * P->n_layers,
               "posterior_encoder.enc.cond_layer: expected [%d, %d]", 2 * H * P->n_layers, c->d.style_dim);
    P->cond.add(cw, *cb);
    P->has_cond = true;
  } else {  // gin_channels = 0: the table is one zero row block (the reference's g_l = zeros)
    P->cond.hW.assign((size_t)2 * H * P->n_layers * P->cond.K, 0.f);
    P->cond.hb.assign((size_t)2 * H * P->n_layers, 0.f);
    P->cond.J = 2 * H * P->n_layers;
  }
  STTS_TRY(upload_table(c, &P->cond));
  P->in.resize(P->n_layers);
  P->rs.resize(P->n_layers);
  std::vector<HostTensor> win(P->n_layers), wrs(P->n_layers);
  for (int i = 0; i < P->n_layers; ++i) {
    const std::string qi = p + "enc.in_layers." + std::to_string(i), qr = p + "enc.res_skip_layers." + std::to_string(i);
    STTS_TRY(get_weight(c, qi, &win[i]));
    STTS_GET(b, qi + ".bias");
    const HostTensor& w = win[i];
    STTS_CHECK(w.shape[0] == 2 * H && w.shape[1] == H && w.shape[2] % 2 == 1 && (i == 0 || w.shape[2] == P->ksize) && (int)b->data.size() == 2 * H,
               "posterior_encoder.enc.in_layers.%d has an unexpected shape", i);
    P->ksize = (int)w.shape[2];
    STTS_TRY(pack_rows(c, w, b, paired_rows(H, 0, H), 0, H, H, H, &P->in[i]));
    STTS_TRY(get_weight(c, qr, &wrs[i]));
    STTS_GET(br, qr + ".bias");
    const int n_rs = i < P->n_layers - 1 ? 2 * H : H;
    STTS_CHECK(wrs[i].shape[0] == n_rs && wrs[i].shape[1] == H && (int)br->data.size() == n_rs, "posterior_encoder.enc.res_skip_layers.%d has an unexpected shape", i);
    STTS_TRY(pack_plain(c, qr, true, 0, H, &P->rs[i]));
  }
  HostTensor wm, wl;
  STTS_TRY(get_weight(c, p + "proj_mean", &wm));
  STTS_TRY(get_weight(c, p + "proj_logstd", &wl));
  STTS_GET(bm, p + "proj_mean.bias");
  STTS_GET(bl, p + "proj_logstd.bias");
  P->out_ch = (int)wm.shape[0];
  STTS_CHECK(P->out_ch > 0 && P->out_ch % 4 == 0 && wm.shape[1] == H && wl.shape == wm.shape && (int)bm->data.size() == P->out_ch && bl->data.size() == bm->data.size(),
             "posterior_encoder.proj_mean / proj_logstd have unexpected shapes");
  HostTensor wcat = wm, bcat = *bm;
  wcat.data.insert(wcat.data.end(), wl.data.begin(), wl.data.end());
  wcat.shape[0] = 2 * P->out_ch;
  bcat.data.insert(bcat.data.end(), bl->data.begin(), bl->data.end());
  STTS_TRY(pack_rows(c, wcat, &bcat, paired_rows(P->out_ch, 0, P->out_ch), 0, H, H, P->out_ch, &P->prior));
  STTS_TRY(pack_plain(c, p + "proj_mean", true, 0, H, &P->pmean));
  STTS_TRY(pack_plain(c, p + "proj_logstd", true, 0, H, &P->plogstd));
  if (H == kPostC && P->ksize == kPostTaps && !getenv("STTS_NO_WN_FUSED")) {
    const int C = kPostC;
    P->W1.resize(P->n_layers); P->b1.resize(P->n_layers); P->W2.resize(P->n_layers); P->b2.resize(P->n_layers);
    for (int i = 0; i < P->n_layers; ++i) {
      const HostTensor& w = win[i];
      std::vector<std::vector<double>> plane((size_t)kPostTaps * 2 * C, std::vector<double>(C));  // [tap][output row][cin]
      for (int k = 0; k < kPostTaps; ++k)
        for (int n = 0; n < 2 * C; ++n)
          for (int ci = 0; ci < C; ++ci) plane[(size_t)k * 2 * C + n][ci] = w.data[((size_t)n * C + ci) * kPostTaps + k];
      // wave w, tile ((tap j, half h), c): output rows h * 128 + 32 w + 16 c + col
      const std::vector<float> f1 = pack_fragments(kPostWaves, C / 16, kPostTaps * 4, [&](int wv, int t, int col) {
        return plane[(size_t)(t >> 2) * 2 * C + ((t >> 1) & 1) * C + 32 * wv + 16 * (t & 1) + col].data();
      });
      STTS_TRY(dev_upload(c, f1, &P->W1[i]));
      STTS_TRY(dev_upload(c, find(c, p + "enc.in_layers." + std::to_string(i) + ".bias")->data, &P->b1[i]));
      const HostTensor& wr = wrs[i];
      const int n_rs = (int)wr.shape[0], nct = n_rs / 16 / kPostWaves;
      std::vector<std::vector<double>> rr(n_rs, std::vector<double>(C));
      for (int n = 0; n < n_rs; ++n)
        for (int k = 0; k < C; ++k) rr[n][k] = wr.data[(size_t)n * C + k];
      const std::vector<float> f2 = pack_fragments(kPostWaves, C / 16, nct, [&](int wv, int t, int col) { return rr[(size_t)16 * nct * wv + 16 * t + col].data(); });
      STTS_TRY(dev_upload(c, f2, &P->W2[i]));
      STTS_TRY(dev_upload(c, find(c, p + "enc.res_skip_layers." + std::to_string(i) + ".bias")->data, &P->b2[i]));
    }
    P->fused = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ plan
struct PostPlan {
  bool fused = false;
  int rows = 0;  // block height of wn_post_kernel: 16 | 32 | 64
};

// Precedence: what the finalize packed (width 128 and k = 3, or the generic form) -> STTS_POST_WN (read on every call: 0 = generic, 16 / 32 / 64 =
// wn_post_kernel on that block height) -> the timing rule.
inline PostPlan plan_posterior(const stts_ctx* c, const Seg& s) {
  const PostW* P = static_cast<const PostW*>(c->posterior.get());
  if (!P || !P->fused) return {};
  if (const char* e = getenv("STTS_POST_WN")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return {true, v};
    if (v == 0 && e[0] == '0') return {};
  }
  // One block per CU is resident (one wave per SIMD), so a launch takes ceil(blocks / 256) rounds, and a block's time is its MFMA chain: ~kT0 + kTile
  // us per 16-row tile (v_mfma_f32_16x16x4_f32 at one wave per SIMD).  Every height does the same matrix work per row; what differs is how full the
  // last round is.  Measured (MI355X, tools/posterior_bench.py, whole stage, ms; forms alternated in one process, spread <= 1 %):
  //     rows (blocks of 16)     generic    16      32      64
  //       960   (60)             0.439    0.240   0.346   0.566
  //      1920  (120)             0.466    0.253   0.355   0.576
  //      7680  (480)             0.539    0.447   0.416   0.631
  //     12800  (800)             0.846    0.752   0.735   0.701
  //     51200 (3200)             2.532    2.434   2.518   2.652
  // 32 against 16 at one round each: (0.346 - 0.240) / 12 = 8.8 us per layer and tile, 64 against 32: 18.3 for two; 7680 rows (two rounds of 16-row
  // blocks against one of 32-row blocks) gives kT0 = 2.6 us.  The rule below picks the measured best of the first four rows.  From 8 rounds of 16-row
  // blocks on the rounds no longer run in step and the smallest block fills the chip most evenly: 16 wins at 51200 rows (the round model says 32).
  // The generic form is never the faster one (by 4 % at 51200 rows, 45 % at 960), so the plan keeps the fused kernel wherever it is built.
  constexpr double kT0 = 2.6, kTile = 9.0;
  auto cost = [&](int rt) { return ceil_div((int)seg_blocks(s, 16 * rt), 256) * (kT0 + kTile * rt); };
  if (ceil_div((int)seg_blocks(s, 16), 256) >= 8) return {true, 16};
  int rt = 1;
  for (int cand : {2, 4})
    if (cost(cand) < cost(rt)) rt = cand;
  return {true, 16 * rt};
}

inline void launch_wn_post(hipStream_t st, const Seg& s, int rows, bool last, WnPostArgs& a) {
  if (s.n_utt <= kWnSegInline) {
    a.n_inline = s.n_utt;
    memcpy(a.seg_inline, s.host, (s.n_utt + 1) * sizeof(int));
  }
  const dim3 grid(ceil_div(s.max_len(), rows), s.n_utt), block(64 * kPostWaves);
  GemmProfiler& prof = gemm_profiler();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof.on) {
    const double fl = 2.0 * s.rows() * kPostC * (2.0 * kPostC * kPostTaps + (last ? kPostC : 2.0 * kPostC));
    prof.add("wn_post_kernel", 0, fl, fl, 0.0);
    e0 = prof.next();
    e1 = prof.next();
  }
  wn_dispatch<16, 64, 32>(rows, [&](auto rtag) {
    constexpr int RT = decltype(rtag)::value / 16;
    if (last) STTS_LAUNCH_TIMED((wn_post_kernel<RT, true>), grid, block, st, e0, e1, a);
    else STTS_LAUNCH_TIMED((wn_post_kernel<RT, false>), grid, block, st, e0, e1, a);
  });
}

// WaveNet layer i: h (hcur -> hnext for the fused form, in place for the generic one), out (+)= skip.  Returns the buffer that holds h afterwards.
inline int posterior_layer(stts_ctx* c, hipStream_t st, const Seg& s, const PostW& P, const PostPlan& plan, int i, bool out_acc, float* hcur, float* hnext, float* out,
                           float* acts, const float* cond, int ld, float** h_after) {
  const int H = P.hidden;
  const bool last = i == P.n_layers - 1;
  if (plan.fused) {
    WnPostArgs a{};
    a.Hin = hcur; a.Hout = last ? nullptr : hnext; a.Out = out; a.seg_off = s.dev;
    a.W1 = P.W1[i]; a.b1 = P.b1[i]; a.W2 = P.W2[i]; a.b2 = P.b2[i];
    a.gate = cond; a.ld_gate = ld; a.gcol0 = i * 2 * H; a.out_acc = out_acc;
    launch_wn_post(st, s, plan.rows, last, a);
    STTS_HIP(hipGetLastError());
    *h_after = last ? hcur : hnext;
    return 0;
  }
  GemmArgs g = gemm_args(s);
  set_seg(g, 0, hcur, H, 0, P.in[i]);
  g.N = H; g.bias = P.in[i].bias; g.Y = acts; g.ldy = H;
  g.gate = cond; g.ld_gate = ld; g.gcol0 = i * 2 * H; g.gC = H;
  STTS_TRY(launch_conv_gemm(st, g, EPI_GATE, P.in[i].npad, s.n_utt, s.max_len()));
  GemmArgs q = gemm_args(s);
  set_seg(q, 0, acts, H, 0, P.rs[i]);
  q.N = P.rs[i].N; q.bias = P.rs[i].bias;
  q.D0 = hcur; q.ldd0 = H; q.acc0 = 1;          // h += rs[:H]
  q.D1 = out; q.ldd1 = H; q.acc1 = out_acc;     // out (+)= rs[H:] ; last layer: all of rs
  q.nsplit = last ? 0 : H;
  STTS_TRY(launch_conv_gemm(st, q, EPI_SPLIT_ACC, P.rs[i].npad, s.n_utt, s.max_len()));
  *h_after = hcur;
  return 0;
}

// ------------------------------------------------------------------------------------------------ stage
struct PostIO {
  const float* audio;            // [h * rows] packed, or null: har_spec / har_phase are inputs
  float *har_spec, *har_phase;   // [rows, ld_har]
  int ld_har;
  const float* style;            // [n_utt, style_dim] or null (g = None)
  const float* noise;            // [rows, out_ch]
  float *z, *mean, *logstd;      // [rows, out_ch], optional
  float* mel;                    // [rows, ld_mel] = post_flow(z), optional
  int ld_mel;
  float *x0, *wn;                // optional taps [rows, hidden]
};

inline int posterior_forward(stts_ctx* c, hipStream_t st, const Seg& s, const PostIO& io, Arena& ws) {
  const PostW& P = *static_cast<const PostW*>(c->posterior.get());
  const int H = P.hidden, oc = P.out_ch, ml = s.max_len(), ld = P.cond.ld();
  const long R = s.rows();
  const SignalGeom& g = c->geom;
  // (every buffer of either form is carved whatever the plan: the carving depends on the batch through rows() and n_utt only)
  float* h0 = ws.get<float>((size_t)R * H);
  float* h1 = ws.get<float>((size_t)R * H);
  float* out = ws.get<float>((size_t)R * H);
  float* acts = ws.get<float>((size_t)R * H);
  float* cond = ws.get<float>((size_t)s.n_utt * ld);
  float* z = io.z ? io.z : ws.get<float>((size_t)R * oc);
  STTS_CHECK(ws.ok, "posterior_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  if (io.audio)
    for (int u = 0; u < s.n_utt; ++u)
      STTS_CHECK((long)(s.host[u + 1] - s.host[u]) * g.h > g.n_fft / 2, "utterance %d too short for reflect padding (%d frames; need > %d samples)", u,
                 s.host[u + 1] - s.host[u], g.n_fft / 2);
  const PostPlan plan = plan_posterior(c, s);
  // 1. STFT of the recording, the last frame dropped (flow.py:283-286): the harmonic stage's kernels on `audio`
  if (io.audio) STTS_TRY(launch_stft(c, st, s, io.audio, io.har_spec, io.har_phase, io.ld_har, 0));
  // 2. x0 = cat[pre_spec(har_spec), pre_phase(har_phase)] (flow.py:288): two contractions into the column halves of one buffer
  for (int q = 0; q < 2; ++q) {
    const PackedConv& w = q == 0 ? P.pre_spec : P.pre_phase;
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, q == 0 ? io.har_spec : io.har_phase, io.ld_har, 0, w);
    a.N = H / 2; a.bias = w.bias; a.Y = h0; a.ldy = H; a.ycol0 = q * (H / 2);
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, ml));
  }
  if (io.x0) STTS_HIP(hipMemcpyAsync(io.x0, h0, (size_t)R * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  // 3. cond = cond_layer(style), once per call (flow.py:67-68); g = None: zeros (flow.py:76)
  if (io.style) STTS_TRY(run_style(st, P.cond, io.style, s.n_utt, cond));
  else STTS_HIP(hipMemsetAsync(cond, 0, (size_t)s.n_utt * ld * sizeof(float), st));
  // 4. the WaveNet (flow.py:70-88, x_mask = 1): `out` starts at layer 0's skip
  float* hcur = h0;
  for (int i = 0; i < P.n_layers; ++i) {
    float* after = nullptr;
    STTS_TRY(posterior_layer(c, st, s, P, plan, i, i > 0, hcur, hcur == h0 ? h1 : h0, out, acts, cond, ld, &after));
    hcur = after;
  }
  if (io.wn) STTS_HIP(hipMemcpyAsync(io.wn, out, (size_t)R * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  // 5. z = mean + noise * exp(logstd) (flow.py:290-292)
  {
    GemmArgs p = gemm_args(s);
    set_seg(p, 0, out, H, 0, P.prior);
    p.N = oc; p.bias = P.prior.bias; p.Z = z; p.ldz = oc; p.noise = io.noise; p.ldnoise = oc;
    STTS_TRY(launch_conv_gemm(st, p, EPI_PRIOR, P.prior.npad, s.n_utt, ml));
  }
  for (int q = 0; q < 2; ++q) {
    float* dst = q == 0 ? io.mean : io.logstd;
    if (!dst) continue;
    const PackedConv& w = q == 0 ? P.pmean : P.plogstd;
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, out, H, 0, w);
    a.N = oc; a.bias = w.bias; a.Y = dst; a.ldy = oc;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, ml));
  }
  // 6. mel = post_flow(z) (speech_predictor.py:109)
  if (io.mel) {
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, z, oc, 0, c->post_flow);
    a.N = c->d.dec_hidden; a.bias = c->post_flow.bias; a.Y = io.mel; a.ldy = io.ld_mel;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, c->post_flow.npad, s.n_utt, ml));
  }
  return 0;
}

// what the entry points check before anything is carved or launched
inline int posterior_check(const stts_ctx* c, const Seg& s, const PostIO& io) {
  const PostW& P = *static_cast<const PostW*>(c->posterior.get());
  STTS_CHECK(!s.cap, "the posterior encoder takes plain segments (no STTS_SEG_CAPACITY)");
  STTS_CHECK(io.har_spec && io.har_phase && io.noise, "posterior_forward: har_spec, har_phase and noise are required");
  STTS_CHECK(io.ld_har % 4 == 0 && io.ld_har >= P.pre_spec.kc, "ld_har %d: must be a multiple of 4 covering %d columns (the bins padded to the packed input width)", io.ld_har,
             P.pre_spec.kc);
  if (io.audio && !c->geom.generic) STTS_CHECK(io.ld_har <= 64 * ((kBins + 63) / 64), "ld_har %d > %d", io.ld_har, 64 * ((kBins + 63) / 64));
  STTS_CHECK(!io.style || P.has_cond, "posterior_forward: a style was given but the encoder has no cond_layer (gin_channels = 0)");
  if (io.mel) {
    STTS_CHECK(c->ready & STTS_W_FLOW, "mel_out needs post_flow: finalize STTS_W_FLOW");
    STTS_CHECK(P.out_ch == c->d.dec_hidden / 4 && io.ld_mel >= c->d.dec_hidden, "mel_out: out_channels %d is not post_flow's input width, or ld_mel %d < %d", P.out_ch, io.ld_mel,
               c->d.dec_hidden);
  }
  for (const void* ptr : {(const void*)io.har_spec, (const void*)io.har_phase, (const void*)io.noise, (const void*)io.z, (const void*)io.mean, (const void*)io.logstd,
                          (const void*)io.mel, (const void*)io.style})
    STTS_CHECK((uintptr_t)ptr % 16 == 0, "posterior_forward: buffers must be 16-byte aligned");
  return 0;
}

}  // namespace stts

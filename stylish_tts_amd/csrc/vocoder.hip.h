// The vocoder stages (models/generator.py): harmonic source + STFT, the ConvNeXt block (shared with cfm_pitch.hip.h), the prior convs, the body with its
// iSTFT.  Included by model.hip.h, which defines the context, the weight structs and the contraction / Winograd launchers used here.  frame_switches()
// reads the STTS_* switches of these stages and of frame_path.hip.h, plan_vocoder() chooses the form of a call (DESIGN.md 8 states the precedence; no
// launches, no HIP calls), the functions below it execute a plan: none of them reads a switch or a threshold again.
#pragma once

namespace stts {

// ---- the switches: experiments and comparisons
struct FrameSwitches {
  // read ONCE per process
  long side_min_rows;   // STTS_SIDE_MIN_ROWS: fp32 batches of more rows run source -> STFT -> prior convs on a side stream (frame_path.hip.h)
  bool xaff_general;    // STTS_XAFF_GENERAL: GRN's activation scale in the general scale / shift / slope form of the contraction's input affine
  // read per call (tests change it between calls)
  bool no_side_stream;  // STTS_NO_SIDE_STREAM: the single-stream order
};
inline FrameSwitches frame_switches() {
  static const FrameSwitches once{getenv("STTS_SIDE_MIN_ROWS") ? atol(getenv("STTS_SIDE_MIN_ROWS")) : 3000, getenv("STTS_XAFF_GENERAL") != nullptr, false};
  FrameSwitches sw = once;
  sw.no_side_stream = getenv("STTS_NO_SIDE_STREAM") != nullptr;
  return sw;
}

// ---- the plan: the form of the prior convs and of the body in one call
struct VocoderPlan {
  // Row precision of the body, 0 (fp32 rows) or the operand precision: every contraction input of the body is then a 16-bit row buffer written by its
  // producer (LayerNorm outputs, the SiLU output of pwconv1, the head inputs written by the prior convs and the head LayerNorm).  From rows16_threshold()
  // rows on: below that the contractions are latency-bound one-round launches and the extra copies cost more than the staging they save.
  int p16 = 0;
  bool spec16 = false;     // the spectra arrive as 16-bit rows (frame path: written by the STFT), not as fp32 rows
  bool spec_copy = false;  // fp32 spectra: the prior convs carve scratch for the rounded copy that 16-bit rows read
  bool mel16 = false;      // mel arrives with a copy already rounded to the operand precision (frame path: the flow's last contraction); else the body casts one
  // the k = 7 convs in Winograd F(6,7) form (12 instead of 42 multiplies per 6 outputs), amp / phase: each pair shares one scratch, sized by and carved for [0]
  bool wino_prior[2] = {false, false}, wino_out[2] = {false, false};
};
// Precedence, top to bottom: operand precision and rows -> which Winograd forms the finalize packed (fp32 only).  The plan of stts_vocoder_forward: the
// caller's spectra and mel are fp32 rows.
inline VocoderPlan plan_vocoder(const stts_ctx* c, const Seg& s) {
  VocoderPlan p;
  p.p16 = (c->prec != PREC_F32 && s.rows() >= rows16_threshold()) ? c->prec : 0;
  // (carved in every 16-bit-mode call, also below the threshold where nothing reads it: stts_frame_workspace_bytes is pinned, so this stays)
  p.spec_copy = c->prec != PREC_F32;
  for (int q = 0; q < 2; ++q) {
    p.wino_prior[q] = c->wino_prior[0].ready && c->wino_prior[q].ready;
    p.wino_out[q] = c->wino_out[0].ready && c->wino_out[1].ready;
  }
  return p;
}

// ------------------------------------------------------------------------------------------------
// stage: harmonic source + STFT (models/generator.py:247-315, :32-44, :406-410)
// ------------------------------------------------------------------------------------------------
// STFT of `sig` [rows * hop] into spec / phase [rows, ld] (out16: 16-bit rows of that precision): the run-time-geometry kernel or the default one
inline int launch_stft(stts_ctx* c, hipStream_t st, const Seg& s, const float* sig, float* spec, float* phase, int ld, int out16) {
  const SignalGeom& g = c->geom;
  const long R = s.rows();
  if (g.generic) STTS_TRY(launch_stft_geom(st, g, s.n_utt, s.dev, R, s.max_len(), sig, c->hann, c->twiddle64, spec, phase, ld, out16));
  else
    STTS_LAUNCH_PROF("stft_kernel", (size_t)R * (kHop + 2 * kBins) * 4, stft_kernel, dim3((s.max_len() + kFftWaves - 1) / kFftWaves, s.n_utt), dim3(64 * kFftWaves), st, sig, s.dev, c->hann, c->twiddle64, spec, phase, ld, out16);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int harmonic_stft(stts_ctx* c, hipStream_t st, const Seg& s, const float* pitch, const float* noise, const float* init_phase,
                         int batch_scope, float* prior_out, float* har_spec, float* har_phase, int ld, Arena& ws, int out16 = 0) {
  const long R = s.rows();
  double* prefix = ws.get<double>(R);
  float* stats = ws.get<float>(2 * s.n_utt);
  const SignalGeom& g = c->geom;
  float* sig = prior_out ? prior_out : ws.get<float>(R * g.h);
  STTS_CHECK(ws.ok, "harmonic_stft: workspace too small");
  if (g.generic) STTS_CHECK(ld >= g.bins, "harmonic_stft: row stride %d < %d bins", ld, g.bins);
  else STTS_CHECK(ld >= kBins && ld <= 64 * ((kBins + 63) / 64), "harmonic_stft: row stride %d outside [%d, %d]", ld, kBins, 64 * ((kBins + 63) / 64));
  STTS_DRY_RETURN(ws);
  if (!s.cap)  // (capacity segments: pcph_kernel checks the real lengths and raises the device error word 4)
    for (int u = 0; u < s.n_utt; ++u)
      STTS_CHECK((long)(s.host[u + 1] - s.host[u]) * g.h > g.n_fft / 2, "utterance %d too short for reflect padding (%d frames; need > %d samples)", u,
                 s.host[u + 1] - s.host[u], g.n_fft / 2);
  if (g.generic) {
    STTS_TRY(launch_pcph_geom(st, g, s.n_utt, s.dev, R, s.max_len(), pitch, noise, init_phase, batch_scope, prefix, stats, sig, c->d_err));
  } else {
    STTS_LAUNCH_PROF("pcph_prep_kernel", (size_t)R * 12, pcph_prep_kernel, dim3(s.n_utt), dim3(256), st, pitch, s.dev, prefix, stats);
    STTS_LAUNCH_PROF("pcph_kernel", (size_t)R * kHop * 8, pcph_kernel, dim3(std::min(1024, ceil_div(s.max_len() * kHop, 256)), s.n_utt), dim3(256), st, pitch, s.dev, s.n_utt,
                     prefix, stats, noise, init_phase, batch_scope, sig, c->d_err);
  }
  return launch_stft(c, st, s, sig, har_spec, har_phase, ld, out16);
}

// ------------------------------------------------------------------------------------------------
// stage: vocoder body + iSTFT (models/generator.py:412-433)
// ------------------------------------------------------------------------------------------------
// Scratch of convnext_block_forward: dw / nrm [rows, h], U [rows, inter], part [n_utt * ss_stride, inter] (GRN sums of squares per 32-row
// sub-tile, ss_stride >= ceil(max_len / 32)), gscale [n_utt, inter], w2u [n_utt, pw2.npad * inter] (per-utterance GRN-scaled pwconv2),
// row_utt [rows] (read only when the block does not fit dwconv_ln_kernel).
struct ConvNextScratch {
  float *dw, *nrm, *U, *part;
  int ss_stride;
  float *gscale, *w2u;
  const int* row_utt;
};

// One ConvNeXtBlock with an AdaptiveLayerNorm (models/generator.py:441-499) over packed rows: nxt = cur + block(cur, style).  sty / lds:
// the block's style table rows (its norm slot); p16: the 16-bit operand mode of the frame path (0: fp32).  Used by the vocoder
// (vocoder_body) and by CfmPitchPredictor (cfm_pitch.hip.h).
inline int convnext_block_forward(hipStream_t st, const Seg& s, const ConvNextW& B, int h, int inter, const float* sty, int lds, int p16, const float* cur,
                                  float* nxt, const ConvNextScratch& sc) {
  const long R = s.rows();
  const int ml = s.max_len();
  float *dw = sc.dw, *nrm = sc.nrm, *U = sc.U, *part = sc.part, *gscale = sc.gscale, *w2u = sc.w2u;
  const int ss_stride = sc.ss_stride;
  const int* row_utt = sc.row_utt;
  if (h <= kDwLnMaxC && h % 4 == 0 && (B.K == 3 || B.K == 7 || B.K == 15 || B.K == 31)) {
    // depthwise conv + adaptive LayerNorm in one launch (the [rows, h] intermediate never reaches HBM)
    // (32-row blocks for the long kernels - half the halo re-reads, two blocks per CU - measured no faster at B = 64: 64 vs 58 us)
    const dim3 fg(ceil_div(ml, 16), s.n_utt);
    const size_t fb = (size_t)R * h * (4 + (p16 ? 2 : 4));
#define STTS_DWLN(KK) STTS_LAUNCH_PROF("dwconv_ln_kernel", fb, (dwconv_ln_kernel<KK, 16>), fg, dim3(256), st, cur, h, h, s.dev, B.dw_wt, B.dw_b, 1e-6f, sty, lds, B.norm.col0, nrm, h, p16)
    if (B.K == 3) STTS_DWLN(3);
    else if (B.K == 7) STTS_DWLN(7);
    else if (B.K == 15) STTS_DWLN(15);
    else STTS_DWLN(31);
#undef STTS_DWLN
  } else {
    STTS_CHECK(row_utt, "convnext_block_forward: this block needs the row -> utterance table");
    STTS_LAUNCH_PROF("dwconv_kernel", (size_t)R * h * 2 * 4, (dwconv_kernel<31>), dim3(ceil_div(h, 64), ceil_div(ml, 64), s.n_utt), dim3(256), st, cur, h, dw, h, h, s.dev, B.dw_wt,
                       B.dw_b, B.K, (int)ACT_NONE);
    LnOut o0{nrm, h, 0, sty, nullptr, lds, B.norm.col0, p16}, o1{};
    STTS_TRY(ln_launch(st, dw, h, h, R, row_utt, 1e-6f, 1, 1, o0, o1, ACT_NONE, LnIn{}, s.rows_dev()));
  }
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, nrm, h, 0, B.pw1);
  a.N = inter; a.bias = B.pw1.bias; a.act = ACT_SILU;
  a.x16 = p16 != 0;
  if (p16) { a.Y = nullptr; a.Y16 = reinterpret_cast<unsigned short*>(U); a.ldy16 = inter; }  // GRN's sums of squares come from the fp32 values
  else { a.Y = U; a.ldy = inter; }
  a.sumsq_part = part; a.ld_ss = inter; a.ss_stride = ss_stride;
  STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, B.pw1.npad, s.n_utt, ml));
  STTS_LAUNCH_PROF("grn_gx_kernel", (size_t)s.n_utt * ss_stride * inter * 4, grn_gx_kernel, dim3(ceil_div(inter, 32), s.n_utt), dim3(256), st, part, inter, ss_stride, s.dev, inter, gscale, inter);
  GemmArgs b = gemm_args(s);
  set_seg(b, 0, U, inter, 0, B.pw2);
  if (B.pw2.prec == PREC_F32 && B.pw2.w16_plane > 0 && x3_enabled()) {
    // split fp32: GRN's per-(utterance, channel) factor scales the ACTIVATION while pwconv2's tile is staged (the contraction's input affine with
    // slope 1) instead of a per-utterance copy of the weight: the shared split planes of W stay valid and the scale_weight pass is gone
    hipLaunchKernelGGL(grn_xaff_kernel, dim3(s.n_utt), dim3(256), 0, st, gscale, inter, B.grn_gamma, w2u, B.pw2.kc, inter);
    b.xaff = w2u;
    b.ld_xaff = B.pw2.kc;
    b.xaff_slope = 1.0f;
    b.xaff_scale_only = B.pw2.kc == inter && !frame_switches().xaff_general;  // (no pad column: every staged value is a written one)
  } else {
    launch_scale_weight(st, dim3(128, s.n_utt), B.pw2.prec, B.pw2.W, gscale, inter, B.grn_gamma, w2u, B.pw2.npad, B.pw2.kc);
    b.seg[0].W = w2u;
    b.seg[0].W16 = reinterpret_cast<const unsigned short*>(w2u);
    b.seg[0].w16_plane = 0;
    b.seg[0].w_utt_stride = (long)B.pw2.npad * B.pw2.kc;
  }
  b.x16 = p16 != 0;
  b.N = h; b.bias = B.pw2.bias; b.Y = nxt; b.ldy = h; b.R = cur; b.ldr = h;
  STTS_TRY(launch_conv_gemm(st, b, EPI_STORE, B.pw2.npad, s.n_utt, ml));
  return 0;
}

// The harmonic spectra as the prior convs read them, rows of `ld` elements: fp32 rows (spec / phase) with copy16, scratch of rows * ld elements for the
// rounded copy that 16-bit rows need, or (is16) 16-bit rows already.
struct SpecRows {
  const float *spec, *phase;
  int ld;
  bool is16;
  unsigned short* copy16;
};
// prior convs (generator.py:412-413) write straight into the concat slots [h, h+hp) of the two head inputs.  The two
// convs are independent (and independent of decoder/flow), so the caller may put them on different streams.
// 16-bit rows (p.p16): the head inputs are 16-bit row buffers (`head` reinterpreted, [rows, hc] elements).
inline int prior_conv(stts_ctx* c, hipStream_t st, const Seg& s, const VocoderPlan& p, int which, const SpecRows& in, float* head, WinoScratch& wino) {
  const int h = c->d.gen_hidden, hp = h / 2, hc = h + hp;
  const PackedConv& w = which == 0 ? c->amp_prior : c->phase_prior;
  const float* har = which == 0 ? in.spec : in.phase;
  if (p.wino_prior[which] && wino) return run_winograd(st, s, har, in.ld, c->wino_prior[which], head + h, hc, ACT_NONE, nullptr, 0, 1.0f, wino);
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, har, in.ld, 0, w);
  a.N = hp; a.bias = w.bias;
  if (p.p16) {
    STTS_CHECK((in.copy16 || in.is16) && in.ld % 8 == 0, "prior_conv: 16-bit mode needs the rounded-copy scratch");
    if (!in.is16) launch_cast_rows(st, p.p16, har, in.ld, c->geom.bins, in.copy16, in.ld, s.rows());
    a.seg[0].X = in.is16 ? har : reinterpret_cast<const float*>(in.copy16);
    a.x16 = 1;
    a.Y = nullptr; a.Y16 = reinterpret_cast<unsigned short*>(head); a.ldy16 = hc; a.ycol16 = h;
  } else {
    a.Y = head; a.ldy = hc; a.ycol0 = h;
  }
  return launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, s.max_len());
}
// Both prior convs on `st`, their scratch (Winograd planes, rounded copy) carved from `scratch`: a region the caller hands over for these two launches only.
inline int prior_convs(stts_ctx* c, hipStream_t st, const Seg& s, const VocoderPlan& p, SpecRows in, float* headA, float* headP, Arena scratch) {
  WinoScratch wino;
  if (p.wino_prior[0]) wino.p = scratch.get<float>(wino_scratch_floats(s, c->wino_prior[0]));
  if (p.spec_copy) in.copy16 = scratch.get<unsigned short>(s.rows() * in.ld);
  STTS_CHECK(scratch.ok, "prior convs: workspace too small");
  STTS_DRY_RETURN(scratch);
  STTS_TRY(prior_conv(c, st, s, p, 0, in, headA, wino));
  return prior_conv(c, st, s, p, 1, in, headP, wino);
}

// mel as the projector reads it: fp32 rows, and (VocoderPlan::mel16) rows16 [rows, round_up(gen_input, 32)] already rounded to the operand precision by its producer
struct MelRows {
  const float* rows;
  int ld;
  const unsigned short* rows16;
};
// everything after the prior convs: projector, ConvNeXt blocks, heads, output convs, iSTFT (generator.py:414-433).
// headA / headP [rows, 768]: columns [512, 768) already hold logamp_prior / phase_prior.
inline int vocoder_body(stts_ctx* c, hipStream_t st, const Seg& s, const VocoderPlan& p, const MelRows& mel, const float* style, float* headA, float* headP,
                        float* audio, float* logamp_out, float* phase_out, int ld_lp, Arena& ws) {
  const stts_model_dims& d = c->d;
  const long R = s.rows();
  const int h = d.gen_hidden, hp = h / 2, hc = h + hp, inter = d.gen_inter, ml = s.max_len();
  const SignalGeom& geo = c->geom;
  const int ldlp = round_up(geo.bins, 32), ldm16 = round_up(d.gen_input, 32);
  float* xa = ws.get<float>(R * h);
  float* xb = ws.get<float>(R * h);
  float* dw = ws.get<float>(R * h);
  float* nrm = ws.get<float>(R * h);
  float* U = ws.get<float>(R * inter);
  const int ss_stride = ceil_div(ml, 128) * 4;
  float* part = ws.get<float>((size_t)s.n_utt * ss_stride * inter);
  float* gscale = ws.get<float>((size_t)s.n_utt * inter);
  float* w2u = ws.get<float>((size_t)s.n_utt * c->cnx[0].pw2.npad * inter);
  float* sty = ws.get<float>((size_t)s.n_utt * c->gen_style.ld());
  int* row_utt = ws.get<int>(R);
  float* la = logamp_out ? logamp_out : ws.get<float>(R * ldlp);
  float* ph = phase_out ? phase_out : ws.get<float>(R * ldlp);
  const int ldl = logamp_out ? ld_lp : ldlp;
  // 16-bit rows: nrm / U / headA / headP are reinterpreted; mel gets a rounded copy unless its producer wrote one
  const int p16 = p.p16;
  const unsigned short* mel16 = mel.rows16;
  unsigned short* mel_copy = (p16 && !p.mel16) ? ws.get<unsigned short>(R * ldm16) : nullptr;
  float* yw = ws.get<float>((R + s.n_utt) * geo.win);
  WinoScratch wino;
  if (p.wino_out[0]) wino.p = ws.get<float>(wino_scratch_floats(s, c->wino_out[0]));
  STTS_CHECK(ws.ok, "vocoder: workspace too small");
  STTS_DRY_RETURN(ws);
  STTS_CHECK(!logamp_out == !phase_out, "logamp_out and phase_out must be given together");
  const int lds = c->gen_style.ld();
  STTS_TRY(run_style(st, c->gen_style, style, s.n_utt, sty));
  STTS_LAUNCH_PROF("row_utt_kernel", (size_t)R * 4, row_utt_kernel, dim3(ceil_div(ml, 256), s.n_utt), dim3(256), st, s.dev, s.n_utt, row_utt);
  // projector over cat[mel, logamp_prior, phase_prior] as three K segments (generator.py:414)
  {
    GemmArgs a = gemm_args(s);
    if (p16) {
      if (!p.mel16) {
        launch_cast_rows(st, p16, mel.rows, mel.ld, d.gen_input, mel_copy, ldm16, R);
        mel16 = mel_copy;
      }
      set_seg(a, 0, reinterpret_cast<const float*>(mel16), ldm16, 0, c->proj_mel);
      a.x16 = 1;
    } else {
      set_seg(a, 0, mel.rows, mel.ld, 0, c->proj_mel);
    }
    set_seg(a, 1, headA, hc, h, c->proj_la);
    set_seg(a, 2, headP, hc, h, c->proj_ph);
    a.N = h; a.bias = c->proj_mel.bias; a.Y = xa; a.ldy = h;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, c->proj_mel.npad, s.n_utt, ml));
  }
  float* cur = xa;
  float* nxt = xb;
  const ConvNextScratch cs{dw, nrm, U, part, ss_stride, gscale, w2u, row_utt};
  for (int i = 0; i < 4; ++i) {
    STTS_TRY(convnext_block_forward(st, s, c->cnx[i], h, inter, sty, lds, p16, cur, nxt, cs));
    std::swap(cur, nxt);
  }
  // two AdaLN heads (eps 1e-5) into columns [0,512) of the head inputs (generator.py:417-423)
  {
    LnOut o0{headA, hc, 0, sty, nullptr, lds, c->head_amp.col0, p16}, o1{headP, hc, 0, sty, nullptr, lds, c->head_phase.col0, p16};
    STTS_TRY(ln_launch(st, cur, h, h, R, row_utt, 1e-5f, 1, 2, o0, o1, ACT_NONE, LnIn{}, s.rows_dev()));
  }
  // the two output convs: the first bins - 1 channels as a contraction, the Nyquist bin of both in one dot-product launch
  float* const head[2] = {headA, headP};
  float* const out[2] = {la, ph};
  for (int q = 0; q < 2; ++q) {
    const PackedConv& w = q == 0 ? c->amp_out : c->phase_out;
    if (p.wino_out[q] && wino) {
      STTS_TRY(run_winograd(st, s, head[q], hc, c->wino_out[q], out[q], ldl, ACT_NONE, nullptr, 0, 1.0f, wino));
      continue;
    }
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, head[q], hc, 0, w);
    a.x16 = p16 != 0;
    a.N = geo.bins - 1; a.bias = w.bias; a.Y = out[q]; a.ldy = ldl;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, ml));
  }
  const int kk = c->amp_out.ntaps;
  STTS_CHECK(kk <= kChanTaps, "output conv kernel size %d > %d", kk, kChanTaps);
  const ChanConvSet sa{headA, c->nyq_w[0], c->nyq_b[0], la}, sp{headP, c->nyq_w[1], c->nyq_b[1], ph};
  STTS_TRY(launch_single_channel_conv(st, s, p16, 2, sa, sp, hc, hc, kk, ldl, geo.bins - 1, true));
  if (geo.generic) {
    STTS_TRY(launch_istft_geom(st, geo, s.n_utt, s.dev, R, ml, la, ph, ldl, c->hann, c->twiddle64, yw, audio));
    STTS_HIP(hipGetLastError());
    return 0;
  }
  STTS_LAUNCH_PROF("istft_frames_kernel", (size_t)R * 2 * kBins * 4, istft_frames_kernel, dim3((ml + 1 + kFftWaves - 1) / kFftWaves, s.n_utt), dim3(64 * kFftWaves), st, la, ph, ldl, s.dev, c->hann, c->twiddle64, yw);
  STTS_LAUNCH_PROF("istft_ola_kernel", (size_t)R * kHop * 4, istft_ola_kernel, dim3(std::min(1024, ceil_div(ml * kHop, 256)), s.n_utt), dim3(256), st, yw, s.dev, c->hann, audio);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int vocoder_forward(stts_ctx* c, hipStream_t st, const Seg& s, const float* mel, int ld_mel, const float* style, const float* har_spec,
                           const float* har_phase, int ld_har, float* audio, float* logamp_out, float* phase_out, int ld_lp, Arena& ws) {
  const long R = s.rows();
  const int hc = c->d.gen_hidden + c->d.gen_hidden / 2;
  const VocoderPlan p = plan_vocoder(c, s);
  float* headA = ws.get<float>(R * hc);
  float* headP = ws.get<float>(R * hc);
  STTS_CHECK(ws.ok, "vocoder_forward: workspace too small");
  // (the prior convs' scratch is released again before vocoder_body carves its own buffers)
  STTS_TRY(prior_convs(c, st, s, p, SpecRows{har_spec, har_phase, ld_har, false, nullptr}, headA, headP, ws.rest()));
  return vocoder_body(c, st, s, p, MelRows{mel, ld_mel, nullptr}, style, headA, headP, audio, logamp_out, phase_out, ld_lp, ws);
}

}  // namespace stts

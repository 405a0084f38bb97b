// The frame path: decoder -> reverse flow -> vocoder in one call, next to harmonic source -> STFT -> prior convs (stts_frame_path), and the workspace
// query of every frame-rate entry point.  Included by model.hip.h after the stages it walks (adain_block.hip.h, flow.hip.h, vocoder.hip.h).  plan_frame()
// chooses the form of a call (DESIGN.md 8 states the precedence; no launches, no HIP calls), acquire_side_lane() hands out the streams and events of the
// side lane, frame_path() walks the stages once, in one host order, whichever stream the source chain goes to.
#pragma once

namespace stts {

// row stride of the harmonic spectra: the prior convs' packed input width (1056; 1088 in the 16-bit modes)
inline int har_ld(const stts_ctx* c) { return std::max(round_up(c->d.n_fft / 2 + 1, 32), c->amp_prior.kc); }

// ---- the plan
struct FramePlan {
  // The vocoder of this call.  16-bit rows: the spectra are only read by the prior convs, so the STFT writes them as 16-bit rows (spec16), and the flow's
  // last contraction also writes mel rounded (mel16) when it writes the generator's input as it is (gen_input == dec_hidden).
  VocoderPlan voc;
  // fp32, large batches: the source -> STFT -> prior-conv chain (independent of decoder and flow until the vocoder) runs on a SIDE STREAM of the caller's
  // stream (fork / join events): it fills the chip while the decoder runs its small bandwidth-bound kernels.  Same kernels, same results; same-box A/B
  // (3-s utterances): B = 8: 4.43 -> 4.38 ms per step (+1.2 %), B = 4: 2.91 -> 2.86 (+1.6 %), B = 2: +0.8 %, B = 1: 1.76 -> 1.78 (the two cross-queue
  // waits cost more than the overlap gains: off below 3 000 rows; STTS_SIDE_MIN_ROWS).  (Round 1, when the step took 7.5 ms and the prior convs were
  // direct contractions, the same experiment gained < 1 % at B = 8, 7.51 vs 7.57 ms/step: the decoder GEMMs already filled the chip.)  Not in the 16-bit
  // modes (the persistent contraction kernel of the decoder and that of the prior convs would fight for the same CUs).
  // side_scratch: the prior convs then need scratch of their own (the decoder uses the stage region at the same time).  It depends on the context and
  // rows() only, so a dry run and a real call carve alike.
  bool side_scratch = false;
  // side: this call uses the lane.  Not in a dry run, not while the per-launch profiler is on (its events belong to one stream), not with
  // STTS_NO_SIDE_STREAM.  frame_path() clears it while the caller's stream is being captured into a graph (the lane's stream and events are created on
  // first use, which a capture may not allow): that question needs the stream and a HIP call.
  bool side = false;
};
// Precedence, top to bottom: operand precision and rows (plan_vocoder) -> model dims -> rows against STTS_SIDE_MIN_ROWS and the packed Winograd form ->
// dry run / profiler -> STTS_NO_SIDE_STREAM -> (in frame_path) stream capture.
inline FramePlan plan_frame(const stts_ctx* c, const Seg& s) {
  const FrameSwitches sw = frame_switches();
  FramePlan p;
  p.voc = plan_vocoder(c, s);
  p.voc.spec16 = p.voc.p16 != 0;
  p.voc.spec_copy = false;
  p.voc.mel16 = p.voc.p16 && c->d.gen_input == c->d.dec_hidden;
  p.side_scratch = c->prec == PREC_F32 && s.rows() > sw.side_min_rows && c->wino_prior[0].ready;
  p.side = p.side_scratch && !dry_run().on && !gemm_profiler().on && !sw.no_side_stream;
  return p;
}

// ---- the side lane of a caller stream: two streams with their fork / join events, created on first use and kept in the context
inline void release_side_lane(const stts_ctx::SideLane& l) {
  if (l.fork) (void)hipEventDestroy(l.fork);
  if (l.join) (void)hipEventDestroy(l.join);
  if (l.stream) (void)hipStreamDestroy(l.stream);
  if (l.fork2) (void)hipEventDestroy(l.fork2);
  if (l.join2) (void)hipEventDestroy(l.join2);
  if (l.stream2) (void)hipStreamDestroy(l.stream2);
}
// All or nothing: the map only ever holds complete lanes, a creation that fails leaves nothing behind and the next call tries again.
inline int acquire_side_lane(stts_ctx* c, hipStream_t st, stts_ctx::SideLane* lane) {
  std::lock_guard<std::mutex> lock(c->side_mu);
  auto it = c->side_lanes.find(st);
  if (it == c->side_lanes.end()) {
    stts_ctx::SideLane l;
    const int rc = [&l]() -> int {
      STTS_HIP(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
      STTS_HIP(hipEventCreateWithFlags(&l.fork, hipEventDisableTiming));
      STTS_HIP(hipEventCreateWithFlags(&l.join, hipEventDisableTiming));
      STTS_HIP(hipStreamCreateWithFlags(&l.stream2, hipStreamNonBlocking));
      STTS_HIP(hipEventCreateWithFlags(&l.fork2, hipEventDisableTiming));
      STTS_HIP(hipEventCreateWithFlags(&l.join2, hipEventDisableTiming));
      return 0;
    }();
    if (rc) {
      release_side_lane(l);
      return rc;
    }
    it = c->side_lanes.emplace(st, l).first;
  }
  *lane = it->second;
  return 0;
}

inline int frame_path(stts_ctx* c, hipStream_t st, const Seg& s, const float* asr, int ld_asr, const float* pitch, const float* energy,
                      const float* style, const float* prior_noise, const float* src_noise, const float* init_phase, int batch_scope,
                      float* audio, void* wsp, size_t ws_bytes) {
  const long R = s.rows();
  FramePlan plan = plan_frame(c, s);
  Arena top(wsp, ws_bytes);
  const int ldh = har_ld(c), hc = c->d.gen_hidden + c->d.gen_hidden / 2, dh = c->d.dec_hidden;
  float* x = top.get<float>(R * dh);
  float* mel = top.get<float>(R * dh);
  float* hs = top.get<float>(R * ldh);
  float* hp = top.get<float>(R * ldh);
  float* headA = top.get<float>(R * hc);
  float* headP = top.get<float>(R * hc);
  const int ldm16 = round_up(c->d.gen_input, 32);
  unsigned short* mel16 = plan.voc.mel16 ? top.get<unsigned short>(R * ldm16) : nullptr;
  const size_t src_bytes = (size_t)R * (sizeof(double) + c->geom.h * sizeof(float)) + 4096 + 8 * s.n_utt;
  const size_t src_off = top.used;
  char* src_ws = top.get<char>(src_bytes);
  const size_t side_off = top.used;
  float* side_scratch = plan.side_scratch ? top.get<float>(wino_scratch_floats(s, c->wino_prior[0])) : nullptr;
  const size_t side_bytes = top.used - side_off;
  STTS_CHECK(top.ok, "frame_path: workspace too small");
  auto stage = [&]() { return top.rest(); };  // (nothing more is carved from `top`: every stage starts at the same mark)
  if (plan.side) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &capturing);
    plan.side = capturing == hipStreamCaptureStatusNone;
  }
  // The source chain goes to the lane's stream and the prior convs to the lane's scratch, or both stay with the caller's stream and the stage region.
  stts_ctx::SideLane lane;
  SideWork sw;
  if (plan.side) {
    STTS_TRY(acquire_side_lane(c, st, &lane));
    sw.stream = lane.stream2; sw.fork = lane.fork2; sw.join = lane.join2;
    STTS_HIP(hipEventRecord(lane.fork, st));
    STTS_HIP(hipStreamWaitEvent(lane.stream, lane.fork, 0));
  }
  const hipStream_t src_st = plan.side ? lane.stream : st;
  // Whatever fails from here on, the caller's stream joins the side stream before this call returns: work that is still running there reads and
  // writes the caller's workspace, which the caller is free to reuse (in stream order) as soon as it has the status.
  auto source_part = [&]() -> int {
    { Arena a(src_ws, src_bytes, src_off); STTS_TRY(harmonic_stft(c, src_st, s, pitch, src_noise, init_phase, batch_scope, nullptr, hs, hp, ldh, a, plan.voc.spec16 ? plan.voc.p16 : 0)); }
    return prior_convs(c, src_st, s, plan.voc, SpecRows{hs, hp, ldh, plan.voc.spec16, nullptr}, headA, headP,
                       plan.side ? Arena(side_scratch, side_bytes, side_off) : stage());
  };
  auto main_part = [&]() -> int {
    { Arena a = stage(); STTS_TRY(decoder_forward(c, st, s, asr, ld_asr, pitch, energy, style, x, dh, a, plan.side ? &sw : nullptr)); }
    { Arena a = stage(); STTS_TRY(prior_flow_forward(c, st, s, x, dh, style, prior_noise, mel, dh, nullptr, nullptr, a, mel16, ldm16)); }
    return 0;
  };
  int rc = source_part();
  if (plan.side) STTS_HIP(hipEventRecord(lane.join, lane.stream));
  if (rc == 0) rc = main_part();
  if (plan.side) STTS_HIP(hipStreamWaitEvent(st, lane.join, 0));
  if (rc) return rc;
  { Arena a = stage(); STTS_TRY(vocoder_body(c, st, s, plan.voc, MelRows{mel, dh, mel16}, style, headA, headP, audio, nullptr, nullptr, 0, a)); }
  return 0;
}

// Bytes of caller-owned workspace that every frame-rate entry point accepts for a batch of `R` rows in `n_utt` utterances,
// the longest `max_len` rows: a dry run of the stages themselves (dry_run_bytes), so the bound follows the model dims and
// whatever the stages really request.  Weights must be finalized (which convs have a Winograd form decides their scratch).
inline size_t frame_workspace_bytes(const stts_ctx* cc, int64_t R, int n_utt, int max_len) {
  stts_ctx* c = const_cast<stts_ctx*>(cc);
  if (R <= 0 || n_utt <= 0 || max_len <= 0) return 0;
  const SynthSeg syn(R, n_utt, max_len);
  const Seg s = syn.seg();
  return dry_run_bytes([&](Arena a) {
    (void)frame_path(c, nullptr, s, nullptr, c->d.inter_dim, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, a.base, a.cap);
    // the staged entry points start their carving at offset 0; vocoder_forward with its own head buffers is the largest of them
    Arena v = a, d = a;
    (void)vocoder_forward(c, nullptr, s, nullptr, c->d.dec_hidden, nullptr, nullptr, nullptr, har_ld(c), nullptr, nullptr, nullptr, 0, v);
    (void)decoder_forward(c, nullptr, s, nullptr, c->d.inter_dim, nullptr, nullptr, nullptr, nullptr, c->d.dec_hidden, d);
  });
}

}  // namespace stts

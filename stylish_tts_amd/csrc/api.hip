// extern "C" entry points declared in include/stylish_hip.h.  Single translation unit: hipcc compiles this file
// (which includes every kernel header) into libstylish_hip.so for gfx950.
#include "model.hip.h"
#include "cfm.hip.h"
#include "hubert.hip.h"
#include "conv2d.hip.h"
#include "mel_style.hip.h"
#include "cfm_pitch.hip.h"
#include "ssl.hip.h"
#include "wavlm.hip.h"
#include "rmvpe.hip.h"
#include "rmvpe_viterbi.hip.h"
#include "aligner.hip.h"
#include "log_mel.hip.h"
#include "resample.hip.h"
#include "val_scores.hip.h"
#include "posterior.hip.h"

using namespace stts;

namespace stts {
int finalize_flow_stats_component(stts_ctx* c);  // flow_stats.hip.h is included at the end of this file (its kernels are the code object's last)
}

#define API_BEGIN try {
#define API_END                                                         \
  }                                                                     \
  catch (const std::exception& e) { return stts::fail("exception: %s", e.what()); } \
  catch (...) { return stts::fail("unknown exception"); }

extern "C" {

const char* stts_last_error(void) { return stts::last_error().c_str(); }
int stts_version(void) { return 1; }

int stts_ctx_create(const stts_model_dims* dims, int device, stts_ctx** out) {
  API_BEGIN
  STTS_CHECK(dims && out, "null argument");
  int n = 0;
  STTS_HIP(hipGetDeviceCount(&n));
  STTS_CHECK(device >= 0 && device < n, "device %d not available (%d visible)", device, n);
  STTS_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  STTS_HIP(hipGetDeviceProperties(&prop, device));
  STTS_CHECK(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  stts_ctx* c = new stts_ctx();
  c->d = *dims;
  c->device = device;
  c->force_generic_signal = getenv("STTS_SIGNAL_GENERIC") && atoi(getenv("STTS_SIGNAL_GENERIC")) != 0;  // comparisons: signal_geom.hip.h kernels at 2048 / 1200 / 300 too
  PackScope scope(c, engine_mode(c));
  STTS_TRY(dev_upload(c, std::vector<int>(64, 0), &c->d_err));
  *out = c;
  return 0;
  API_END
}

void stts_ctx_destroy(stts_ctx* c) {
  if (!c) return;
  for (void* p : c->allocs) (void)hipFree(p);
  for (auto& kv : c->side_lanes) release_side_lane(kv.second);
  delete c;
}

int stts_set_precision(stts_ctx* c, int precision) {
  API_BEGIN
  STTS_CHECK(c, "bad argument");
  STTS_CHECK(precision >= 0 && precision <= 3, "precision must be STTS_PREC_F32, _BF16, _F16 or _F32_NATIVE");
  const int prec = precision == STTS_PREC_F32_NATIVE ? (int)PREC_F32 : precision;
  STTS_CHECK(c->ready == 0 || (prec == c->prec && (precision != STTS_PREC_F32_NATIVE) == c->allow_x3), "precision must be chosen before weights are finalized");
  c->prec = prec;
  c->allow_x3 = precision != STTS_PREC_F32_NATIVE;
  return 0;
  API_END
}

int stts_load_weight(stts_ctx* c, const char* name, const float* data, const int64_t* shape, int ndim) {
  API_BEGIN
  STTS_CHECK(c && name && data && shape && ndim >= 1 && ndim <= 4, "bad argument");
  HostTensor t;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    n *= shape[i];
  }
  t.data.assign(data, data + n);
  c->host[name] = std::move(t);
  return 0;
  API_END
}

// Every finalize below has one shape: make sure the model object exists, open a PackScope with the component's packing mode, pack, and set the
// `ready` bits on success.  The scope puts the mode back on every exit path; the engine's own precision (c->prec, c->allow_x3) is never touched.
int stts_finalize_weights(stts_ctx* c, int which) {
  API_BEGIN
  STTS_CHECK(c, "null ctx");
  STTS_HIP(hipSetDevice(c->device));
  // re-finalizing: the previous packing of these components goes away, and so do their `ready` bits - they come back only for
  // the components that finalize successfully below (a failed re-finalize must not leave a stage runnable on freed buffers)
  c->ready &= ~which;
  free_component_allocs(c, which);
  if (which & (STTS_W_DECODER | STTS_W_FLOW | STTS_W_GENERATOR)) {
    // 16-bit operand modes: input channels padded to 64 (the K tile of conv_gemm16_kernel); the stages size their rows from the packed kc
    PackScope scope(c, {c->prec, true, c->prec != PREC_F32 ? 64 : 32, 0});
    STTS_TRY(finalize_frame(c, which));  // (sets its own `ready` bits)
  }
  const int ph = which & (STTS_W_SPEECH_TEXT | STTS_W_DURATION | STTS_W_PE_TEXT | STTS_W_PE_STYLE | STTS_W_PITCH_ENERGY);
  if (ph) {
    if (!c->phoneme) c->phoneme = std::make_shared<PhonemeModel>();
    // the phoneme-rate predictors always run in fp32 (include/stylish_hip.h, stts_set_precision): durations are integers and must
    // equal the fp32 reference's bit for bit, and these stages are latency-bound (nothing to win from 16-bit operands)
    // (and on the f32 matrix cores, not the split-fp32 form: latency-bound launches, and per-utterance GRN weights in the style encoder)
    static const bool phoneme_x3 = getenv("STTS_PHONEME_X3") && atoi(getenv("STTS_PHONEME_X3")) != 0;  // experiment: the split form for the phoneme-rate contractions too
    PackScope scope(c, {PREC_F32, phoneme_x3, 32, 0});
    STTS_TRY(finalize_phoneme(c, static_cast<PhonemeModel*>(c->phoneme.get()), ph));
    c->ready |= ph;
  }
  const int hb = which & (STTS_W_HUBERT | STTS_W_HUBERT_PE);
  if (hb) {
    if (!c->hubert) c->hubert = std::make_shared<HubertModel>();
    // fp32 on the f32 matrix cores whatever the precision, as the phoneme-rate predictors above
    PackScope scope(c, {PREC_F32, false, 32, 0});
    STTS_TRY(finalize_hubert(c, static_cast<HubertModel*>(c->hubert.get()), hb));
    c->ready |= hb;
  }
  const int ms = which & (STTS_W_PE_MEL_STYLE | STTS_W_CFM_PITCH);
  if (ms) {
    if (!c->mel_style) c->mel_style = std::make_shared<MelStyleModel>();
    PackScope scope(c, engine_mode(c));  // (its packer reads only the tag: fp32 whatever the precision, mel_style.hip.h)
    STTS_TRY(finalize_mel_style(c, static_cast<MelStyleModel*>(c->mel_style.get()), ms));
    c->ready |= ms;
  }
  if (which & STTS_W_CFM_PITCH_NET) {
    if (!c->cfm_pitch) c->cfm_pitch = std::make_shared<CfmPitchNetW>();
    // fp32 on the f32 matrix cores whatever the precision, as the HuBERT front ends above (cfm_pitch.hip.h)
    PackScope scope(c, {PREC_F32, false, 32, STTS_W_CFM_PITCH_NET});
    STTS_TRY(finalize_cfm_pitch_net(c, static_cast<CfmPitchNetW*>(c->cfm_pitch.get())));
    c->ready |= STTS_W_CFM_PITCH_NET;
  }
  if (which & STTS_W_POSTERIOR) {
    if (!c->posterior) c->posterior = std::make_shared<PostW>();
    if (!c->hann) {  // the STFT geometry and its tables (context lifetime), as a frame-path finalize sets them up
      PackScope tables(c, {c->prec, true, c->prec != PREC_F32 ? 64 : 32, 0});
      STTS_TRY(finalize_frame(c, 0));
    }
    // fp32 whatever the precision; the contractions around the WaveNet in the split-fp32 form where the engine allows it
    PackScope scope(c, {PREC_F32, true, 32, STTS_W_POSTERIOR});
    STTS_TRY(finalize_posterior(c, static_cast<PostW*>(c->posterior.get())));
    c->ready |= STTS_W_POSTERIOR;
  }
  if (which & STTS_W_FLOW_STATS) STTS_TRY(finalize_flow_stats_component(c));
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

int stts_check_status(stts_ctx* c, void* stream) {
  API_BEGIN
  int e = 0;
  STTS_HIP(hipStreamSynchronize((hipStream_t)stream));
  STTS_HIP(hipMemcpy(&e, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
  if (e) {
    // bit flags (the kernels set them with atomicOr): every pending condition is reported, the most specific text first
    STTS_HIP(hipMemset(c->d_err, 0, sizeof(int)));
    std::string msg;
    if (e & 2) msg += "text encoder: token id outside [0, tokens); ";
    if (e & 4) msg += "harmonic source: an utterance is too short for the STFT's reflect padding (needs more than " + std::to_string(c->d.n_fft / 2) + " samples); ";
    if (e & 1) msg += "harmonic source: a frame is voiced (f0 > 10 Hz) but no f0 exceeds 20 Hz (reference raises: models/generator.py:285); ";
    if (e & ~7) msg += "unknown device error bits " + std::to_string(e & ~7) + "; ";
    msg.resize(msg.size() - 2);
    return stts::fail("%s", msg.c_str());
  }
  return 0;
  API_END
}

int stts_har_ld(const stts_ctx* c) {
  if (!c) return 0;
  if (c->amp_prior.kc) return har_ld(c);  // the generator is packed: the prior convs' input width
  return round_up(c->d.n_fft / 2 + 1, c->prec != PREC_F32 ? 64 : 32);  // before: what the frame path's packing mode will pad the bins to in this precision
}

size_t stts_frame_workspace_bytes(const stts_ctx* c, int64_t rows, int n_utt, int max_len) { return frame_workspace_bytes(c, rows, n_utt, max_len); }

// host offsets of n_utt utterances: present, starting at 0, none empty (`bad` / `empty`: the texts where they are not the utterance rows';
// `empty` is formatted with the utterance and its length)
static int seg_ok(int n_utt, const int32_t* h, const int32_t* d, const char* bad = "bad utterance offsets", const char* empty = "utterance %d is empty") {
  STTS_CHECK(n_utt > 0 && h && d && h[0] == 0, "%s", bad);
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(h[u + 1] > h[u], empty, u, h[u + 1] - h[u]);
  return 0;
}

// the opening of a stage entry point: its components (and the model object that holds them, `have`) are finalized; device and stream
#define READY_CHECK(have, mask)                                                      \
  STTS_CHECK(c && (have) && (c->ready & (mask)) == (mask), "weights for this stage are not finalized (need components 0x%x, have 0x%x)", (mask), c ? c->ready : 0); \
  STTS_HIP(hipSetDevice(c->device));                                                 \
  hipStream_t st = (hipStream_t)stream

#define SEG_CHECK(mask)                                                              \
  READY_CHECK(true, mask);                                                           \
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));                                \
  Seg s{n_utt, seg_off_host, seg_off_dev}

int stts_decoder_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* asr,
                         int ld_asr, const float* pitch, const float* energy, const float* style, float* x_out, int ld_x, void* ws,
                         size_t ws_bytes) {
  API_BEGIN
  SEG_CHECK(STTS_W_DECODER);
  STTS_CHECK(ld_asr >= c->d.inter_dim && ld_asr % 4 == 0 && ld_x >= c->d.dec_hidden, "bad leading dimension");
  Arena a(ws, ws_bytes);
  return decoder_forward(c, st, s, asr, ld_asr, pitch, energy, style, x_out, ld_x, a);
  API_END
}

int stts_prior_flow_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x,
                            int ld_x, const float* style, const float* prior_noise, float* mel_out, int ld_mel, float* z_prior_out,
                            float* z_flow_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  SEG_CHECK(STTS_W_FLOW);
  STTS_CHECK(ld_x % 4 == 0 && ld_x >= c->d.dec_hidden && ld_mel >= c->d.dec_hidden, "bad leading dimension");
  Arena a(ws, ws_bytes);
  return prior_flow_forward(c, st, s, x, ld_x, style, prior_noise, mel_out, ld_mel, z_prior_out, z_flow_out, a);
  API_END
}

int stts_harmonic_stft(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* pitch,
                       const float* src_noise, const float* init_phase, int batch_scope, float* prior_signal_out, float* har_spec,
                       float* har_phase, int ld_har, void* ws, size_t ws_bytes) {
  API_BEGIN
  SEG_CHECK(STTS_W_GENERATOR);
  STTS_CHECK(ld_har >= c->geom.bins, "ld_har %d < %d", ld_har, c->geom.bins);
  Arena a(ws, ws_bytes);
  return harmonic_stft(c, st, s, pitch, src_noise, init_phase, batch_scope, prior_signal_out, har_spec, har_phase, ld_har, a);
  API_END
}

int stts_vocoder_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* mel,
                         int ld_mel, const float* style, const float* har_spec, const float* har_phase, int ld_har, float* audio_out,
                         float* logamp_out, float* phase_out, int ld_lp, void* ws, size_t ws_bytes) {
  API_BEGIN
  SEG_CHECK(STTS_W_GENERATOR);
  STTS_CHECK(ld_mel % 4 == 0 && ld_har % 32 == 0 && ld_har >= har_ld(c), "har/mel leading dimension: ld_har must be a multiple of 32 covering %d columns (the prior convs' packed input width)", har_ld(c));
  STTS_CHECK(!logamp_out || ld_lp >= c->geom.bins, "ld_lp too small");
  Arena a(ws, ws_bytes);
  return vocoder_forward(c, st, s, mel, ld_mel, style, har_spec, har_phase, ld_har, audio_out, logamp_out, phase_out, ld_lp, a);
  API_END
}

int stts_frame_path(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* asr, int ld_asr,
                    const float* pitch, const float* energy, const float* style, const float* prior_noise, const float* src_noise,
                    const float* init_phase, int batch_scope, float* audio_out, void* ws, size_t ws_bytes, int seg_flags) {
  API_BEGIN
  SEG_CHECK(STTS_W_DECODER | STTS_W_FLOW | STTS_W_GENERATOR);
  s.cap = (seg_flags & STTS_SEG_CAPACITY) != 0;
  STTS_CHECK(ld_asr >= c->d.inter_dim && ld_asr % 4 == 0, "bad ld_asr");
  return frame_path(c, st, s, asr, ld_asr, pitch, energy, style, prior_noise, src_noise, init_phase, batch_scope, audio_out, ws, ws_bytes);
  API_END
}

int stts_length_regulate(stts_ctx* c, void* stream, int n_utt, const int32_t* dur, const int32_t* tok_off, const int32_t* frm_off,
                         int64_t n_frames, int rep, const float* enc, int ld_enc, int C, float* out, int ld_out, int32_t* src_row_ws) {
  API_BEGIN
  if (c) STTS_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(dur && tok_off && frm_off && enc && out && src_row_ws && n_utt > 0 && n_frames >= 0 && rep >= 1, "length_regulate: bad argument");
  STTS_CHECK(C % 4 == 0 && ld_enc % 4 == 0 && ld_out % 4 == 0, "length_regulate: channel counts must be multiples of 4");
  launch_frame_token_map(st, n_utt, dur, tok_off, frm_off, rep, src_row_ws);
  const long work = n_frames * (C / 4);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<long>(2048, std::max<long>(1, (work + 255) / 256))), dim3(256), 0, st, enc, ld_enc,
                     src_row_ws, out, ld_out, 0, C, (int)n_frames, frm_off + n_utt);  // n_frames may be a capacity: the real count is frm_off[n_utt]
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_frame_offsets(stts_ctx* c, void* stream, int n_utt, const int32_t* tok_off_dev, const int32_t* dur, const int32_t* cap_off_dev,
                       int32_t* off_T_dev, int32_t* off_T4_dev, int32_t* need_dev) {
  API_BEGIN
  STTS_CHECK(c && n_utt > 0 && tok_off_dev && dur && cap_off_dev && off_T_dev && off_T4_dev && need_dev, "frame_offsets: bad argument");
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(frame_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dur, tok_off_dev, n_utt, cap_off_dev, off_T_dev, off_T4_dev, need_dev);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_upsample4(stts_ctx* c, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T, const int32_t* off_T4, const float* x,
                   float* y) {
  API_BEGIN
  if (c) STTS_HIP(hipSetDevice(c->device));
  int ml = 0;
  for (int u = 0; u < n_utt; ++u) ml = std::max(ml, off_T_host[u + 1] - off_T_host[u]);
  hipLaunchKernelGGL(upsample4_kernel, dim3(ceil_div(4 * ml, 256), n_utt), dim3(256), 0, (hipStream_t)stream, x, off_T, off_T4, y);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_euler_step(void* stream, float* x, const float* v, float dt, int64_t n) {
  API_BEGIN
  STTS_CHECK(x && v && n >= 0, "bad argument");
  if (n) hipLaunchKernelGGL(euler_step_kernel, dim3((unsigned)std::min<int64_t>(4096, (n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, x, v, dt, (long)n);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// ------------------------------------------------------------------------------------------------ CfmMelDecoder estimator (cfm.hip.h)
int stts_cfm_finalize(stts_ctx* c, const stts_cfm_dims* dims) {
  API_BEGIN
  STTS_CHECK(c && dims, "null argument");
  STTS_HIP(hipSetDevice(c->device));
  c->ready &= ~STTS_W_CFM;
  free_component_allocs(c, STTS_W_CFM);
  CfmDims d;
  d.feat = dims->feat_dim; d.asr = dims->asr_dim; d.spk = dims->spk_dim; d.hidden = dims->hidden_dim; d.emb = dims->emb_dim; d.depth = dims->depth;
  d.enc_blocks = dims->enc_blocks; d.dec_blocks = dims->dec_blocks; d.prev_depth = dims->prev_depth; d.post_depth = dims->post_depth; d.head_dim = dims->head_dim;
  auto m = std::make_shared<CfmModel>();
  PackScope scope(c, {c->prec, false, 32, STTS_W_CFM});  // latency-bound estimator: f32 matrix cores
  STTS_TRY(finalize_cfm(c, d, m.get()));
  c->cfm = m;
  c->ready |= STTS_W_CFM;
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

size_t stts_cfm_workspace_bytes(const stts_ctx* c, int64_t rows, int n_utt) {
  if (!c || !c->cfm) return 0;
  return cfm_workspace_bytes(const_cast<stts_ctx*>(c), *static_cast<const CfmModel*>(c->cfm.get()), rows, n_utt);
}

int stts_cfm_estimator(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ld_x,
                       const float* asr, int ld_asr, const float* f0, const float* n_curve, const int32_t* curve_off_host, const int32_t* curve_off_dev,
                       const float* spk_emb, const float* t, const float* sine_noise, float* out, int ld_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && c->cfm && (c->ready & STTS_W_CFM), "the CfmMelDecoder weights are not finalized (stts_cfm_finalize)");
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  STTS_TRY(seg_ok(n_utt, curve_off_host, curve_off_dev, "bad curve offsets", "utterance %d has an empty F0 / N curve"));
  STTS_CHECK(x && asr && f0 && n_curve && spk_emb && t && sine_noise && out && ws, "null tensor");
  STTS_HIP(hipSetDevice(c->device));
  Seg s{n_utt, seg_off_host, seg_off_dev};
  Arena a(ws, ws_bytes);
  return cfm_estimator(c, *static_cast<const CfmModel*>(c->cfm.get()), (hipStream_t)stream, s, x, ld_x, asr, ld_asr, f0, n_curve, curve_off_dev, spk_emb, t,
                       sine_noise, out, ld_out, a);
  API_END
}

int stts_to_time_major(void* stream, const float* x, int B, int C, int T, float* y, int ldy) {
  API_BEGIN
  STTS_CHECK(ldy >= C, "ldy < C");
  hipLaunchKernelGGL(to_time_major_kernel, dim3(ceil_div(T, 32), ceil_div(ldy, 32), B), dim3(256), 0, (hipStream_t)stream, x, B, C, T, y, ldy, 0, ldy);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_to_channel_major(void* stream, const float* x, int ldx, int B, int C, int T, float* y) {
  API_BEGIN
  hipLaunchKernelGGL(to_channel_major_kernel, dim3(ceil_div(T, 32), ceil_div(C, 32), B), dim3(256), 0, (hipStream_t)stream, x, ldx, 0, B, C, T, y);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// ------------------------------------------------------------------------------------------------ phoneme-rate stages
#define PH_CHECK(mask)                                                               \
  READY_CHECK(c->phoneme, mask);                                                     \
  PhonemeModel& M = *static_cast<PhonemeModel*>(c->phoneme.get())

size_t stts_phoneme_workspace_bytes(const stts_ctx* c, int64_t n_tokens, int64_t n_frames, int n_utt, int max_tokens, int max_frames) {
  return phoneme_workspace_bytes(c, n_tokens, n_frames, n_utt, max_tokens, max_frames);
}

int stts_text_encoder_forward(stts_ctx* c, void* stream, int which, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                              const int64_t* tokens, float* mu_out, int ld_mu, float* x_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  const int te_mask[3] = {STTS_W_DURATION, STTS_W_SPEECH_TEXT, STTS_W_PE_TEXT};
  STTS_CHECK(which >= 0 && which < 3, "which must be 0 (duration), 1 (speech) or 2 (pitch/energy)");
  PH_CHECK(te_mask[which]);
  STTS_TRY(seg_ok(n_utt, tok_off_host, tok_off_dev));
  STTS_CHECK(ld_mu >= M.te[which].inter, "ld_mu too small");
  Seg s{n_utt, tok_off_host, tok_off_dev};
  Arena a(ws, ws_bytes);
  return text_encoder_forward(c, st, M.te[which], s, (const long*)tokens, mu_out, ld_mu, x_out, a);
  API_END
}

int stts_text_style_forward(stts_ctx* c, void* stream, int which, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev, const float* x,
                            int ldx, float* style_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  const int se_mask[3] = {STTS_W_DURATION, STTS_W_SPEECH_TEXT, STTS_W_PE_STYLE};
  STTS_CHECK(which >= 0 && which < 3, "which must be 0, 1 or 2");
  PH_CHECK(se_mask[which]);
  STTS_TRY(seg_ok(n_utt, tok_off_host, tok_off_dev));
  STTS_CHECK(ldx % 32 == 0 && ldx >= M.se[which].inter, "style encoder input: ld must be a multiple of 32 covering inter_dim");
  Seg s{n_utt, tok_off_host, tok_off_dev};
  Arena a(ws, ws_bytes);
  return text_style_forward(c, st, M.se[which], s, x, ldx, style_out, c->d.style_dim, a);
  API_END
}

int stts_duration_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev, const int64_t* tokens,
                          float* logits_out, int32_t* dur_out, float* mu_out, float* style_out, float* prosody_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  PH_CHECK(STTS_W_DURATION);
  STTS_TRY(seg_ok(n_utt, tok_off_host, tok_off_dev));
  Seg s{n_utt, tok_off_host, tok_off_dev};
  Arena a(ws, ws_bytes);
  return duration_forward(c, M, st, s, (const long*)tokens, logits_out, 16, dur_out, mu_out, style_out, prosody_out, a);
  API_END
}

int stts_pitch_energy_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                              const int32_t* frm_off_host, const int32_t* frm_off_dev, const int32_t* dur, const float* pe_enc, int ld_enc,
                              const float* pe_style, float* f0_out, float* energy_out, float* prosody_out, float* cross_out, void* ws,
                              size_t ws_bytes, int seg_flags) {
  API_BEGIN
  PH_CHECK(STTS_W_PITCH_ENERGY);
  STTS_TRY(seg_ok(n_utt, tok_off_host, tok_off_dev));
  STTS_TRY(seg_ok(n_utt, frm_off_host, frm_off_dev));
  STTS_CHECK(ld_enc >= c->d.pe_inter && ld_enc % 4 == 0, "bad ld_enc");
  Seg sp{n_utt, tok_off_host, tok_off_dev}, sf{n_utt, frm_off_host, frm_off_dev};
  sf.cap = (seg_flags & STTS_SEG_CAPACITY) != 0;
  Arena a(ws, ws_bytes);
  return pitch_energy_forward(c, M, st, sp, sf, dur, pe_enc, ld_enc, pe_style, f0_out, energy_out, prosody_out, cross_out, a);
  API_END
}

int stts_duration_decode(void* stream, const float* logits, int ld, int n_rows, int32_t* dur_out) {
  API_BEGIN
  STTS_CHECK(logits && dur_out && ld >= 16 && n_rows > 0, "bad argument");
  hipLaunchKernelGGL(duration_decode_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, logits, ld, 16, n_rows, dur_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_duration_to_alignment(void* stream, const int32_t* dur, int n_tokens, int n_frames, float* alignment_out) {
  API_BEGIN
  STTS_CHECK(dur && alignment_out && n_tokens > 0 && n_tokens <= 1024 && n_frames > 0, "bad argument (at most 1024 tokens)");
  const long total = (long)n_tokens * n_frames;
  hipLaunchKernelGGL(alignment_matrix_kernel, dim3((unsigned)std::min<long>(1024, (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dur, n_tokens,
                     n_frames, alignment_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// ------------------------------------------------------------------------------------------------ conv-form STFT (ONNX export)
static int conv_stft_tables(stts_ctx* c) {
  if (c->hann) return 0;
  STTS_HIP(hipSetDevice(c->device));
  PackScope scope(c, engine_mode(c));  // context-lifetime tables
  std::vector<float> h(kWin);
  for (int i = 0; i < kWin; ++i) h[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / kWin));
  STTS_TRY(dev_upload(c, h, &c->hann));
  std::vector<float2> tw(kNfft / 2);
  std::vector<double2> tw64(kNfft / 2);
  for (int i = 0; i < kNfft / 2; ++i) {
    tw64[i] = make_double2(cos(2.0 * M_PI * i / kNfft), -sin(2.0 * M_PI * i / kNfft));
    tw[i] = make_float2((float)tw64[i].x, (float)tw64[i].y);
  }
  STTS_TRY(dev_upload(c, tw, &c->twiddle));
  STTS_TRY(dev_upload(c, tw64, &c->twiddle64));
  return 0;
}

int stts_conv_stft_transform(stts_ctx* c, void* stream, int n_utt, const int32_t* frame_off_host, const int32_t* frame_off_dev, const float* wave,
                             int hop, float* mag, float* x, float* y, int ld) {
  API_BEGIN
  STTS_CHECK(c && wave && mag && x && y && hop > 0 && ld >= kBins, "bad argument");
  STTS_CHECK(c->d.n_fft == kNfft && c->d.win_length == kWin, "conv STFT: built for n_fft 2048 / win 1200 (model.yml)");
  STTS_TRY(seg_ok(n_utt, frame_off_host, frame_off_dev));
  STTS_TRY(conv_stft_tables(c));
  int mf = 0;
  for (int u = 0; u < n_utt; ++u) {
    STTS_CHECK(frame_off_host[u + 1] - frame_off_host[u] >= 2, "conv STFT: utterance %d needs at least 2 frames (hop samples)", u);
    mf = std::max(mf, frame_off_host[u + 1] - frame_off_host[u]);
  }
  hipLaunchKernelGGL(conv_stft_kernel, dim3(mf, n_utt), dim3(256), 0, (hipStream_t)stream, wave, frame_off_dev, hop, c->hann, c->twiddle64, mag, x, y, ld);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_conv_stft_inverse(stts_ctx* c, void* stream, int n_utt, const int32_t* frame_off_host, const int32_t* frame_off_dev, const float* mag,
                           const float* x, const float* y, int ld, int hop, float* wave_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && wave_out && mag && x && y && hop > 0 && ld >= kBins, "bad argument");
  STTS_CHECK(c->d.n_fft == kNfft && c->d.win_length == kWin, "conv STFT: built for n_fft 2048 / win 1200 (model.yml)");
  STTS_TRY(seg_ok(n_utt, frame_off_host, frame_off_dev));
  STTS_TRY(conv_stft_tables(c));
  const long frames = frame_off_host[n_utt];
  STTS_CHECK(ws && ws_bytes >= (size_t)frames * kWin * sizeof(float), "conv iSTFT: workspace needs frames * 1200 floats");
  int mf = 0;
  for (int u = 0; u < n_utt; ++u) {
    STTS_CHECK(frame_off_host[u + 1] - frame_off_host[u] >= 2, "conv iSTFT: utterance %d needs at least 2 frames", u);
    mf = std::max(mf, frame_off_host[u + 1] - frame_off_host[u]);
  }
  float* yw = (float*)ws;
  hipLaunchKernelGGL(conv_istft_frames_kernel, dim3(mf, n_utt), dim3(256), 0, (hipStream_t)stream, mag, x, y, ld, frame_off_dev, c->hann, c->twiddle, yw);
  hipLaunchKernelGGL(conv_istft_ola_kernel, dim3(std::min(1024, ceil_div((mf - 1) * hop, 256)), n_utt), dim3(256), 0, (hipStream_t)stream, yw, frame_off_dev,
                     hop, wave_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// ------------------------------------------------------------------------------------------------ profiling
int stts_profile_begin(void) {
  gemm_profiler().begin();
  return 0;
}

int stts_profile_end(void* stream, int* launches, double* total_ms, double* total_flops) {
  API_BEGIN
  GemmProfiler& p = gemm_profiler();
  p.on = false;
  STTS_HIP(hipStreamSynchronize((hipStream_t)stream));
  double ms = 0, fl = 0;
  int n = 0;
  for (size_t i = 0; i < p.recs.size() && 2 * i + 1 < p.used; ++i) {
    if (p.recs[i].kind != 0) continue;  // the contraction kernels only (the other kernels: stts_profile_report)
    float t = 0;
    STTS_HIP(hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]));
    ms += t;
    fl += p.recs[i].flops;
    ++n;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  return 0;
  API_END
}

int stts_profile_report(void* stream, char* json, size_t cap) {
  API_BEGIN
  STTS_CHECK(json && cap > 2, "bad argument");
  GemmProfiler& p = gemm_profiler();
  p.on = false;
  STTS_HIP(hipStreamSynchronize((hipStream_t)stream));
  struct Agg {
    int kind = 0, n = 0;
    double ms = 0, flops = 0, exec = 0, bytes = 0;
  };
  std::map<std::string, Agg> agg;
  std::vector<std::string> order;
  for (size_t i = 0; i < p.recs.size() && 2 * i + 1 < p.used; ++i) {
    float t = 0;
    STTS_HIP(hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]));
    const ProfRec& r = p.recs[i];
    if (getenv("STTS_PROF_DUMP"))  // diagnostics: every launch in issue order
      fprintf(stderr, "[prof] %4zu %-28s %9.2f us %10.3f GFLOP (%.3f executed) %9.3f MB\n", i, r.name, 1e3 * t, r.flops * 1e-9, r.exec_flops * 1e-9, r.bytes * 1e-6);
    if (!agg.count(r.name)) order.push_back(r.name);
    Agg& g = agg[r.name];
    g.kind = r.kind;
    ++g.n;
    g.ms += t;
    g.flops += r.flops;
    g.exec += r.exec_flops;
    g.bytes += r.bytes;
  }
  std::string out = "[";
  for (size_t k = 0; k < order.size(); ++k) {
    const Agg& g = agg[order[k]];
    char buf[512];
    snprintf(buf, sizeof(buf), "%s{\"kernel\": \"%s\", \"kind\": \"%s\", \"launches\": %d, \"ms\": %.6f, \"gflop\": %.4f, \"executed_gflop\": %.4f, \"mbytes\": %.4f}",
             k ? ", " : "", order[k].c_str(), g.kind == 0 ? "contraction" : "other", g.n, g.ms, g.flops * 1e-9, g.exec * 1e-9, g.bytes * 1e-6);
    out += buf;
  }
  out += "]";
  STTS_CHECK(out.size() + 1 <= cap, "profile report needs %zu bytes", out.size() + 1);
  memcpy(json, out.c_str(), out.size() + 1);
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ AdaptiveHubert (ssl.hip.h)
static int ssl_dims_from(const stts_ssl_dims* dims, SslDims* d) {
  STTS_CHECK(dims, "ssl: null dims");
  STTS_CHECK(dims->num_feat_extract_layers >= 1 && dims->num_feat_extract_layers <= kSslMaxConv, "ssl: num_feat_extract_layers %d outside [1, %d]",
             dims->num_feat_extract_layers, kSslMaxConv);
  d->hidden = dims->hidden_size; d->layers = dims->num_hidden_layers; d->heads = dims->num_attention_heads; d->inter = dims->intermediate_size;
  d->n_conv = dims->num_feat_extract_layers;
  for (int i = 0; i < d->n_conv; ++i) {
    d->conv_dim[i] = dims->conv_dim[i]; d->conv_k[i] = dims->conv_kernel[i]; d->conv_s[i] = dims->conv_stride[i];
    STTS_CHECK(d->conv_k[i] >= 1 && d->conv_s[i] >= 1, "ssl: conv_kernel[%d] / conv_stride[%d] must be positive", i, i);
  }
  d->pos_k = dims->num_conv_pos_embeddings; d->pos_groups = dims->num_conv_pos_embedding_groups; d->eps = dims->layer_norm_eps;
  return 0;
}

int stts_ssl_finalize(stts_ctx* c, const stts_ssl_dims* dims) {
  API_BEGIN
  STTS_CHECK(c && dims, "null argument");
  STTS_HIP(hipSetDevice(c->device));
  c->ready &= ~STTS_W_SSL;
  free_component_allocs(c, STTS_W_SSL);
  SslDims d;
  STTS_TRY(ssl_dims_from(dims, &d));
  auto m = std::make_shared<SslW>();
  // fp32 whatever the precision, as the other voice-conversion front ends; the dense contractions in the split-fp32 form (weights packed with their
  // three bf16 planes) unless the engine is STTS_PREC_F32_NATIVE (ssl.hip.h says which tile they run and why)
  PackScope scope(c, {PREC_F32, true, 32, STTS_W_SSL});
  STTS_TRY(finalize_ssl(c, d, m.get()));
  c->ssl = m;
  c->ready |= STTS_W_SSL;
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

int64_t stts_ssl_frames(const stts_ssl_dims* dims, int64_t samples) {
  SslDims d;
  if (ssl_dims_from(dims, &d) != 0 || samples < 0) return 0;
  return ssl_frames_host(d, samples);
}

static int ssl_check_offsets(const SslDims& d, int n_utt, const int32_t* sample_off_host) {
  STTS_CHECK(n_utt > 0 && sample_off_host && sample_off_host[0] == 0, "ssl: bad sample offsets");
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)sample_off_host[u + 1] - sample_off_host[u];
    STTS_CHECK(n > 0 && ssl_frames_host(d, n) > 0, "ssl: utterance %d has %ld samples, fewer than one frame of the feature extractor needs", u, n);
  }
  return 0;
}

size_t stts_ssl_workspace_bytes(const stts_ctx* c, int n_utt, const int32_t* sample_off_host) {
  if (!c || !c->ssl || !(c->ready & STTS_W_SSL)) return 0;
  const SslW& M = *static_cast<const SslW*>(c->ssl.get());
  if (ssl_check_offsets(M.d, n_utt, sample_off_host) != 0) return 0;
  return ssl_workspace_bytes(M, n_utt, sample_off_host);
}

int64_t stts_ssl_tap_rows(const stts_ssl_dims* dims, int n_utt, const int32_t* sample_off_host) {
  SslDims d;
  if (ssl_dims_from(dims, &d) != 0 || ssl_check_offsets(d, n_utt, sample_off_host) != 0) return 0;
  SslPlan P;
  ssl_plan(d, n_utt, sample_off_host, &P);
  return (int64_t)P.cap_off[n_utt] * ssl_geom(d).D[0];
}

static int ssl_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                     const int32_t* off_T_host, const int32_t* off_T_dev, float* feats, int ld_feats, const SslTaps* taps, void* ws, size_t ws_bytes) {
  STTS_CHECK(c && c->ssl && (c->ready & STTS_W_SSL), "the AdaptiveHubert weights are not finalized (stts_ssl_finalize)");
  const SslW& M = *static_cast<const SslW*>(c->ssl.get());
  STTS_CHECK(sample_off_dev && wave && off_T_host && off_T_dev && feats && ws, "ssl: null argument");
  STTS_TRY(ssl_check_offsets(M.d, n_utt, sample_off_host));
  STTS_TRY(seg_ok(n_utt, off_T_host, off_T_dev, "ssl: bad time_dim offsets", "ssl: utterance %d has a time_dim of %d"));
  STTS_CHECK(ld_feats >= round_up(M.d.hidden, 32) && ld_feats % 4 == 0, "feature rows: ld_feats %d must be a multiple of 4 covering %d columns (hidden_size %d padded to 32)",
             ld_feats, round_up(M.d.hidden, 32), M.d.hidden);
  STTS_HIP(hipSetDevice(c->device));
  Seg sT{n_utt, off_T_host, off_T_dev};
  Arena a(ws, ws_bytes);
  return ssl_forward(M, (hipStream_t)stream, n_utt, sample_off_host, sample_off_dev, wave, sT, feats, ld_feats, taps, a);
}

int stts_ssl_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                     const int32_t* off_T_host, const int32_t* off_T_dev, float* feats, int ld_feats, void* ws, size_t ws_bytes) {
  API_BEGIN
  return ssl_entry(c, stream, n_utt, sample_off_host, sample_off_dev, wave, off_T_host, off_T_dev, feats, ld_feats, nullptr, ws, ws_bytes);
  API_END
}

int stts_ssl_forward_taps(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                          const int32_t* off_T_host, const int32_t* off_T_dev, float* feats, int ld_feats, float* conv0, int32_t* conv0_off,
                          float* conv_last, float* proj, float* pos, float* layers, float* hidden, void* ws, size_t ws_bytes) {
  API_BEGIN
  SslTaps t;
  t.conv0 = conv0; t.conv0_off = conv0_off; t.conv_last = conv_last; t.proj = proj; t.pos = pos; t.layers = layers; t.hidden = hidden;
  return ssl_entry(c, stream, n_utt, sample_off_host, sample_off_dev, wave, off_T_host, off_T_dev, feats, ld_feats, &t, ws, ws_bytes);
  API_END
}

// ------------------------------------------------------------------------------------------------ WavLM and its perceptual distance (wavlm.hip.h)
int stts_wavlm_finalize(stts_ctx* c, const stts_wavlm_dims* dims) {
  API_BEGIN
  STTS_CHECK(c && dims, "null argument");
  STTS_HIP(hipSetDevice(c->device));
  c->ready &= ~STTS_W_WAVLM;
  free_component_allocs(c, STTS_W_WAVLM);
  SslDims d;
  STTS_TRY(ssl_dims_from(&dims->ssl, &d));
  auto m = std::make_shared<WavlmW>();
  // fp32 whatever the precision, packed as the AdaptiveHubert weights are
  PackScope scope(c, {PREC_F32, true, 32, STTS_W_WAVLM});
  STTS_TRY(finalize_wavlm(c, d, dims->num_buckets, dims->max_bucket_distance, m.get()));
  m->ssl.ready = true;
  c->wavlm = m;
  c->ready |= STTS_W_WAVLM;
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

// pairs > 0: n_utt = 2 pairs and utterances u, u + pairs must have one length
static int wavlm_check_offsets(const SslDims& d, int n_utt, const int32_t* sample_off_host, int pairs) {
  STTS_CHECK(n_utt > 0 && sample_off_host && sample_off_host[0] == 0, "wavlm: bad sample offsets");
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)sample_off_host[u + 1] - sample_off_host[u];
    STTS_CHECK(n > 0 && ssl_frames_host(d, n) > 0, "wavlm: utterance %d has %ld samples, fewer than one frame of the feature extractor needs", u, n);
  }
  for (int u = 0; u < pairs; ++u) {
    const long a = (long)sample_off_host[u + 1] - sample_off_host[u], b = (long)sample_off_host[u + pairs + 1] - sample_off_host[u + pairs];
    STTS_CHECK(a == b, "wavlm: pair %d has waveforms of unequal lengths (%ld and %ld samples)", u, a, b);
  }
  return 0;
}

size_t stts_wavlm_workspace_bytes(const stts_ctx* c, int n_utt, const int32_t* sample_off_host, int pairs) {
  if (!c || !c->wavlm || !(c->ready & STTS_W_WAVLM) || pairs < 0 || (pairs > 0 && n_utt != 2 * pairs)) return 0;
  const WavlmW& M = *static_cast<const WavlmW*>(c->wavlm.get());
  if (wavlm_check_offsets(M.ssl.d, n_utt, sample_off_host, pairs) != 0) return 0;
  return wavlm_workspace_bytes(M, n_utt, sample_off_host, pairs);
}

int stts_wavlm_forward_states(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave, float* states,
                              float* gate0, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && c->wavlm && (c->ready & STTS_W_WAVLM), "the WavLM weights are not finalized (stts_wavlm_finalize)");
  const WavlmW& M = *static_cast<const WavlmW*>(c->wavlm.get());
  STTS_CHECK(sample_off_dev && wave && states && ws, "wavlm: null argument");
  STTS_TRY(wavlm_check_offsets(M.ssl.d, n_utt, sample_off_host, 0));
  STTS_HIP(hipSetDevice(c->device));
  Arena a(ws, ws_bytes);
  return wavlm_forward(M, (hipStream_t)stream, n_utt, sample_off_host, sample_off_dev, wave, states, gate0, 0, nullptr, nullptr, a);
  API_END
}

int stts_wavlm_l1_sums(stts_ctx* c, void* stream, int pairs, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave, double* sums,
                       int32_t* frames, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && c->wavlm && (c->ready & STTS_W_WAVLM), "the WavLM weights are not finalized (stts_wavlm_finalize)");
  const WavlmW& M = *static_cast<const WavlmW*>(c->wavlm.get());
  STTS_CHECK(pairs > 0, "wavlm: no pairs");
  STTS_TRY(wavlm_check_offsets(M.ssl.d, 2 * pairs, sample_off_host, pairs));
  STTS_CHECK(sample_off_dev && wave && sums && frames && ws, "wavlm: null argument");
  STTS_HIP(hipSetDevice(c->device));
  Arena a(ws, ws_bytes);
  return wavlm_forward(M, (hipStream_t)stream, 2 * pairs, sample_off_host, sample_off_dev, wave, nullptr, nullptr, pairs, sums, frames, a);
  API_END
}

int stts_wavlm_bucket_table(const stts_ctx* c, int max_d, int32_t* out) {
  API_BEGIN
  STTS_CHECK(c && c->wavlm && (c->ready & STTS_W_WAVLM), "the WavLM weights are not finalized (stts_wavlm_finalize)");
  STTS_CHECK(max_d >= 0 && out, "wavlm: bad argument");
  const WavlmW& M = *static_cast<const WavlmW*>(c->wavlm.get());
  const int D = M.max_dist;
  for (int d = -max_d; d <= max_d; ++d) out[d + max_d] = M.bucket[std::max(-D, std::min(D, d)) + D];  // the clamp the attention applies
  return 0;
  API_END
}

// ------------------------------------------------------------------------------------------------ text aligner + CTC forced alignment (aligner.hip.h)
extern "C" {

static int aligner_dims_from(const stts_aligner_dims* dims, AlDims* d) {
  STTS_CHECK(dims, "aligner: null dims");
  STTS_CHECK(dims->n_tdnn >= 1 && dims->n_tdnn <= kAlMaxTdnn, "aligner: %d tdnn layers outside [1, %d]", dims->n_tdnn, kAlMaxTdnn);
  d->n_mels = dims->n_mels;
  d->hidden = dims->hidden;
  d->classes = dims->classes;
  d->n_tdnn = dims->n_tdnn;
  d->ffn_layers = dims->ffn_layers;
  for (int i = 0; i < dims->n_tdnn; ++i) d->tdnn_k[i] = dims->tdnn_kernel[i];
  return 0;
}

int stts_aligner_finalize(stts_ctx* c, const stts_aligner_dims* dims) {
  API_BEGIN
  STTS_CHECK(c && dims, "null argument");
  STTS_HIP(hipSetDevice(c->device));
  c->ready &= ~STTS_W_ALIGNER;
  free_component_allocs(c, STTS_W_ALIGNER);
  AlDims d;
  STTS_TRY(aligner_dims_from(dims, &d));
  auto m = std::make_shared<AlW>();
  // fp32 whatever the precision; the contractions in the split-fp32 form unless the engine is STTS_PREC_F32_NATIVE (aligner.hip.h)
  PackScope scope(c, {PREC_F32, true, 32, STTS_W_ALIGNER});
  STTS_TRY(finalize_aligner(c, d, m.get()));
  c->aligner = m;
  c->ready |= STTS_W_ALIGNER;
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

static int aligner_check_offsets(int n_utt, const int32_t* off_host) {
  STTS_CHECK(n_utt > 0 && off_host && off_host[0] == 0, "aligner: bad frame offsets");
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(off_host[u + 1] > off_host[u], "aligner: utterance %d has no mel frames", u);
  STTS_CHECK(off_host[n_utt] <= kAlMaxRows, "aligner: %d rows in one call, at most %ld", off_host[n_utt], kAlMaxRows);
  return 0;
}

size_t stts_aligner_workspace_bytes(const stts_ctx* c, int n_utt, const int32_t* off_host) {
  if (!c || !c->aligner || !(c->ready & STTS_W_ALIGNER)) return 0;
  if (aligner_check_offsets(n_utt, off_host) != 0) return 0;
  return aligner_workspace_bytes(*static_cast<const AlW*>(c->aligner.get()), n_utt, off_host);
}

int64_t stts_aligner_tap_floats(const stts_aligner_dims* dims, int n_utt, const int32_t* off_host) {
  AlDims d;
  if (aligner_dims_from(dims, &d) != 0 || aligner_check_offsets(n_utt, off_host) != 0) return 0;
  return (int64_t)aligner_tap_floats(d, off_host[n_utt]);
}

static int aligner_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel, int ld_mel, float* log_probs,
                         int ld_out, float* taps, void* ws, size_t ws_bytes) {
  STTS_CHECK(c && c->aligner && (c->ready & STTS_W_ALIGNER), "the text aligner's weights are not finalized (stts_aligner_finalize)");
  const AlW& M = *static_cast<const AlW*>(c->aligner.get());
  STTS_CHECK(off_dev && mel && log_probs && ws, "aligner: null argument");
  STTS_TRY(aligner_check_offsets(n_utt, off_host));
  STTS_CHECK(ld_mel >= M.d.n_mels && ld_out >= M.d.classes, "aligner: ld_mel %d < %d mel bins or ld_out %d < %d classes", ld_mel, M.d.n_mels, ld_out, M.d.classes);
  STTS_HIP(hipSetDevice(c->device));
  Seg s{n_utt, off_host, off_dev};
  Arena a(ws, ws_bytes);
  return aligner_forward(M, (hipStream_t)stream, s, mel, ld_mel, log_probs, ld_out, taps, a);
}

int stts_aligner_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel, float* log_probs,
                         int ld_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  return aligner_entry(c, stream, n_utt, off_host, off_dev, mel_rows, ld_mel, log_probs, ld_out, nullptr, ws, ws_bytes);
  API_END
}

int stts_aligner_forward_taps(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel,
                              float* log_probs, int ld_out, float* taps, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(taps, "aligner: null taps");
  return aligner_entry(c, stream, n_utt, off_host, off_dev, mel_rows, ld_mel, log_probs, ld_out, taps, ws, ws_bytes);
  API_END
}

static int ctc_check_offsets(int n_utt, const int32_t* t_off_host, const int32_t* p_off_host, const char* what = "ctc_align") {
  STTS_CHECK(n_utt > 0 && t_off_host && p_off_host && t_off_host[0] == 0 && p_off_host[0] == 0, "%s: bad offsets", what);
  for (int u = 0; u < n_utt; ++u) {
    const long T = (long)t_off_host[u + 1] - t_off_host[u], P = (long)p_off_host[u + 1] - p_off_host[u];
    STTS_CHECK(T >= 1, "%s: utterance %d has no frames", what, u);
    STTS_CHECK(P >= 1 && P <= kCtcMaxTokens, "%s: utterance %d has %ld tokens, outside [1, %d]", what, u, P, kCtcMaxTokens);
  }
  return 0;
}

size_t stts_ctc_align_workspace_bytes(int n_utt, const int32_t* t_off_host, const int32_t* p_off_host) {
  if (ctc_check_offsets(n_utt, t_off_host, p_off_host) != 0) return 0;
  return ctc_workspace_bytes(n_utt, t_off_host, p_off_host);
}

int stts_ctc_align(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const int32_t* p_off_host, const int32_t* p_off_dev,
                   const float* log_probs, int ld, int classes, int blank, const int32_t* targets, int path_given, int32_t* path, float* scores, int32_t* durations,
                   float* left, float* right, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(t_off_dev && p_off_dev && log_probs && targets && path && scores && durations && left && right, "ctc_align: null argument");
  STTS_TRY(ctc_check_offsets(n_utt, t_off_host, p_off_host));
  STTS_CHECK(classes >= 2 && ld >= classes && blank >= 0 && blank < classes, "ctc_align: %d classes in rows of %d, blank %d", classes, ld, blank);
  STTS_CHECK(path_given || (ws && ws_bytes >= ctc_workspace_bytes(n_utt, t_off_host, p_off_host)), "ctc_align: workspace too small (stts_ctc_align_workspace_bytes)");
  return ctc_align((hipStream_t)stream, n_utt, t_off_dev, p_off_dev, log_probs, ld, classes, blank, targets, path_given, path, scores, durations, left, right,
                   (unsigned char*)ws);
  API_END
}

int stts_ctc_nll(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const int32_t* p_off_host, const int32_t* p_off_dev,
                 const float* log_probs, int ld, int classes, int blank, const int32_t* targets, const double* log_priors, double prior_scale, double* nll) {
  API_BEGIN
  STTS_CHECK(t_off_dev && p_off_dev && log_probs && targets && nll, "ctc_nll: null argument");
  STTS_TRY(ctc_check_offsets(n_utt, t_off_host, p_off_host, "ctc_nll"));
  STTS_CHECK(classes >= 2 && ld >= classes && blank >= 0 && blank < classes, "ctc_nll: %d classes in rows of %d, blank %d", classes, ld, blank);
  STTS_CHECK(std::isfinite(prior_scale), "ctc_nll: prior_scale is not finite");
  return ctc_nll((hipStream_t)stream, n_utt, t_off_dev, p_off_dev, log_probs, ld, classes, blank, targets, log_priors, prior_scale, nll);
  API_END
}

// frame offsets alone: at least one frame per utterance
static int ctc_check_frames(const char* what, int n_utt, const int32_t* t_off_host) {
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && t_off_host && t_off_host[0] == 0, "%s: bad offsets", what);
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(t_off_host[u + 1] > t_off_host[u], "%s: utterance %d has no frames", what, u);
  return 0;
}

int stts_ctc_confidence_sums(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const float* scores, double* sums) {
  API_BEGIN
  STTS_TRY(ctc_check_frames("ctc_confidence_sums", n_utt, t_off_host));
  STTS_CHECK(t_off_dev && scores && sums, "ctc_confidence_sums: null argument");
  hipLaunchKernelGGL(ctc_confidence_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, scores, t_off_dev, sums);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

size_t stts_ctc_prior_sums_workspace_bytes(int n_utt, const int32_t* t_off_host, int classes) {
  if (classes < 1 || ctc_check_frames("ctc_prior_sums", n_utt, t_off_host) != 0) return 0;
  return ctc_prior_workspace_bytes(t_off_host[n_utt], classes);
}

int stts_ctc_prior_sums(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const float* log_probs, int ld, int classes,
                        double* log_sums, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_TRY(ctc_check_frames("ctc_prior_sums", n_utt, t_off_host));
  STTS_CHECK(t_off_dev && log_probs && log_sums, "ctc_prior_sums: null argument");
  STTS_CHECK(classes >= 1 && ld >= classes, "ctc_prior_sums: %d classes in rows of %d", classes, ld);
  STTS_CHECK(ws && ws_bytes >= ctc_prior_workspace_bytes(t_off_host[n_utt], classes) && (uintptr_t)ws % 8 == 0,
             "ctc_prior_sums: workspace too small (stts_ctc_prior_sums_workspace_bytes)");
  return ctc_prior_sums((hipStream_t)stream, t_off_host[n_utt], log_probs, ld, classes, log_sums, (double*)ws);
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ RMVPE pitch extractor (rmvpe.hip.h)
extern "C" {

static int rmvpe_dims_from(const stts_rmvpe_dims* dims, RvDims* d) {
  STTS_CHECK(dims, "rmvpe: null dims");
  STTS_CHECK(dims->en_de_layers == kRvLevels && dims->kernel_h == 2 && dims->kernel_w == 2 && dims->n_gru == 1 && dims->n_mels == kRvMels,
             "rmvpe: en_de_layers = %d, kernel_size = (%d, %d), n_gru = %d, n_mels = %d: only 5, (2, 2), 1 and 128 are built", dims->en_de_layers, dims->kernel_h,
             dims->kernel_w, dims->n_gru, dims->n_mels);
  d->n_blocks = dims->n_blocks;
  d->inter_layers = dims->inter_layers;
  d->c0 = dims->en_out_channels;
  return 0;
}

int stts_rmvpe_finalize(stts_ctx* c, const stts_rmvpe_dims* dims) {
  API_BEGIN
  STTS_CHECK(c && dims, "null argument");
  STTS_HIP(hipSetDevice(c->device));
  c->ready &= ~STTS_W_RMVPE;
  free_component_allocs(c, STTS_W_RMVPE);
  RvDims d;
  STTS_TRY(rmvpe_dims_from(dims, &d));
  auto m = std::make_shared<RvW>();
  PackScope scope(c, {PREC_F32, false, 32, STTS_W_RMVPE});  // fp32 on the f32 matrix cores whatever the precision (its packer reads only the tag)
  STTS_TRY(finalize_rmvpe(c, d, m.get()));
  c->rmvpe = m;
  c->ready |= STTS_W_RMVPE;
  STTS_HIP(hipDeviceSynchronize());
  return 0;
  API_END
}

static int rmvpe_check_offsets(int n_utt, const int32_t* off_host) {
  STTS_CHECK(n_utt > 0 && off_host && off_host[0] == 0, "rmvpe: bad frame offsets");
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)off_host[u + 1] - off_host[u];
    STTS_CHECK(n >= 17, "rmvpe: utterance %d has %ld mel frames; the reflect padding to a multiple of 32 frames needs at least 17", u, n);
  }
  return 0;
}

size_t stts_rmvpe_workspace_bytes(const stts_ctx* c, int n_utt, const int32_t* off_host) {
  if (!c || !c->rmvpe || !(c->ready & STTS_W_RMVPE)) return 0;
  if (rmvpe_check_offsets(n_utt, off_host) != 0) return 0;
  return rmvpe_workspace_bytes(*static_cast<const RvW*>(c->rmvpe.get()), n_utt, off_host);
}

int64_t stts_rmvpe_tap_floats(const stts_rmvpe_dims* dims, int n_utt, const int32_t* off_host) {
  RvDims d;
  if (rmvpe_dims_from(dims, &d) != 0 || rmvpe_check_offsets(n_utt, off_host) != 0) return 0;
  return (int64_t)rmvpe_tap_floats(d, rv_padded(n_utt, off_host));
}

static int rmvpe_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel, int ld, float thred, float* hidden_out,
                       float* f0_out, float* taps, void* ws, size_t ws_bytes) {
  STTS_CHECK(c && c->rmvpe && (c->ready & STTS_W_RMVPE), "the RMVPE weights are not finalized (stts_rmvpe_finalize)");
  const RvW& M = *static_cast<const RvW*>(c->rmvpe.get());
  STTS_CHECK(off_dev && mel && ws && (hidden_out || f0_out), "rmvpe: null argument");
  STTS_TRY(rmvpe_check_offsets(n_utt, off_host));
  STTS_CHECK(ld >= kRvMels, "mel rows: ld %d < 128 mel bins", ld);
  STTS_CHECK(std::isfinite(thred), "rmvpe: thred must be finite");
  STTS_HIP(hipSetDevice(c->device));
  Arena a(ws, ws_bytes);
  return rmvpe_forward(M, (hipStream_t)stream, n_utt, off_host, off_dev, mel, ld, thred, hidden_out, f0_out, taps, a);
}

int stts_rmvpe_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel, float thred,
                       float* hidden_out, float* f0_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  return rmvpe_entry(c, stream, n_utt, off_host, off_dev, mel_rows, ld_mel, thred, hidden_out, f0_out, nullptr, ws, ws_bytes);
  API_END
}

int stts_rmvpe_forward_taps(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel, float thred,
                            float* hidden_out, float* f0_out, float* taps, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(taps, "rmvpe: null taps");
  return rmvpe_entry(c, stream, n_utt, off_host, off_dev, mel_rows, ld_mel, thred, hidden_out, f0_out, taps, ws, ws_bytes);
  API_END
}

int stts_rmvpe_mel(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* mel_off_host,
                   const int32_t* mel_off_dev, const float* wave, const float* mel_basis, const int32_t* band, float* mel_out, int ld_mel, float* mel_lin) {
  API_BEGIN
  STTS_CHECK(c && c->rmvpe && (c->ready & STTS_W_RMVPE), "the RMVPE weights are not finalized (stts_rmvpe_finalize)");
  const RvW& M = *static_cast<const RvW*>(c->rmvpe.get());
  STTS_CHECK(n_utt > 0 && sample_off_host && sample_off_dev && mel_off_host && mel_off_dev && wave && mel_basis && band && mel_out, "rmvpe_mel: null argument");
  STTS_CHECK(sample_off_host[0] == 0 && mel_off_host[0] == 0 && ld_mel >= kRvMels, "rmvpe_mel: bad offsets or ld_mel %d < 128", ld_mel);
  int max_fr = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)sample_off_host[u + 1] - sample_off_host[u];
    STTS_CHECK(n > kRvNfft / 2, "rmvpe_mel: utterance %d has %ld samples; the reflect padding needs more than %d", u, n, kRvNfft / 2);
    const int fr = mel_off_host[u + 1] - mel_off_host[u];
    STTS_CHECK(fr == n / kRvHop + 1, "rmvpe_mel: utterance %d: %d mel rows for %ld samples (samples / 160 + 1 = %ld)", u, fr, n, n / kRvHop + 1);
    max_fr = std::max(max_fr, fr);
  }
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(rv_mel_kernel, dim3(ceil_div(max_fr, GeomFft<9>::kWaves), n_utt), dim3(64 * GeomFft<9>::kWaves), 0, (hipStream_t)stream, wave, sample_off_dev,
                     mel_off_dev, M.hann, M.tw, mel_basis, band, mel_out, ld_mel, mel_lin);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_rmvpe_decode(stts_ctx* c, void* stream, int64_t n_rows, const float* salience, int ld, float thred, float* f0_out) {
  API_BEGIN
  STTS_CHECK(c && n_rows > 0 && salience && f0_out && ld >= kRvClasses && std::isfinite(thred), "rmvpe_decode: bad argument");
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(rv_decode_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, salience, ld, (long)n_rows, thred, f0_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_rmvpe_decode_at(stts_ctx* c, void* stream, int64_t n_rows, const float* salience, int ld, const int32_t* center, float thred, float* f0_out) {
  API_BEGIN
  STTS_CHECK(c && n_rows > 0 && salience && center && f0_out && ld >= kRvClasses && std::isfinite(thred), "rmvpe_decode_at: bad argument");
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(rv_decode_at_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, salience, ld, (long)n_rows, center, thred, f0_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// at least one frame per utterance (the path search needs no padding, unlike the network)
static int rmvpe_viterbi_check_offsets(int n_utt, const int32_t* off_host) {
  STTS_CHECK(n_utt > 0 && off_host && off_host[0] == 0, "rmvpe_viterbi: bad frame offsets");
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(off_host[u + 1] > off_host[u], "rmvpe_viterbi: utterance %d has no frames", u);
  return 0;
}

size_t stts_rmvpe_viterbi_workspace_bytes(int n_utt, const int32_t* off_host) {
  if (rmvpe_viterbi_check_offsets(n_utt, off_host) != 0) return 0;
  return rmvpe_viterbi_workspace_bytes(n_utt, off_host);
}

int stts_rmvpe_viterbi(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* salience, int ld, const double* lt_band,
                       double lt_out, double eps, float thred, int32_t* path_out, double* logp_out, float* f0_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && off_dev && salience && ws && (path_out || logp_out || f0_out), "rmvpe_viterbi: null argument");
  STTS_CHECK(lt_band, "rmvpe_viterbi: null transition table");
  STTS_TRY(rmvpe_viterbi_check_offsets(n_utt, off_host));
  STTS_CHECK(ld >= kRvClasses, "rmvpe_viterbi: ld %d < 360 classes", ld);
  STTS_CHECK(std::isfinite(thred) && std::isfinite(lt_out) && eps > 0.0 && std::isfinite(eps), "rmvpe_viterbi: thred, lt_out and eps must be finite, eps positive");
  STTS_CHECK((uintptr_t)ws % 16 == 0, "rmvpe_viterbi: the workspace must be 16-byte aligned");
  STTS_HIP(hipSetDevice(c->device));
  Arena a(ws, ws_bytes);
  return rmvpe_viterbi((hipStream_t)stream, n_utt, off_host, off_dev, salience, ld, lt_band, lt_out, eps, thred, path_out, logp_out, f0_out, a);
  API_END
}

int stts_rmvpe_resample(stts_ctx* c, void* stream, int n_utt, const int32_t* off_in_dev, const int32_t* off_out_host, const int32_t* off_out_dev, const float* f0_in,
                        float* f0_out) {
  API_BEGIN
  STTS_CHECK(c && n_utt > 0 && off_in_dev && off_out_host && off_out_dev && f0_in && f0_out, "rmvpe_resample: null argument");
  int mx = 0;
  for (int u = 0; u < n_utt; ++u) {
    STTS_CHECK(off_out_host[u + 1] > off_out_host[u], "rmvpe_resample: utterance %d has no output frames", u);
    mx = std::max(mx, off_out_host[u + 1] - off_out_host[u]);
  }
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(rv_resample_kernel, dim3(ceil_div(mx, 256), n_utt), dim3(256), 0, (hipStream_t)stream, f0_in, off_in_dev, off_out_dev, f0_out);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ log-mel front end (log_mel.hip.h)
extern "C" {

int stts_log_mel_filters(int n_fft, int n_mels, int sample_rate, int32_t* band, float* weights) {
  API_BEGIN
  STTS_CHECK(band && weights, "log_mel_filters: null argument");
  STTS_TRY(log_mel_check_geometry(n_fft, n_fft, 1, n_mels, sample_rate));
  std::vector<int> b;
  std::vector<float> w;
  log_mel_filters(n_fft, n_mels, sample_rate, &b, &w);
  std::copy(b.begin(), b.end(), band);
  std::copy(w.begin(), w.end(), weights);
  return 0;
  API_END
}

static int log_mel_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* row_off_host,
                         const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length, int n_mels, int sample_rate, double mean, double stdv,
                         float* mel_rows, int ld, float* energy, float* raw_rows, double* partials) {
  STTS_CHECK(c && sample_off_dev && row_off_dev && wave, "log_mel: null argument");
  STTS_TRY(log_mel_check_geometry(n_fft, win_length, hop_length, n_mels, sample_rate));
  int max_fr = 0;
  STTS_TRY(log_mel_check_offsets(n_utt, sample_off_host, row_off_host, n_fft, hop_length, &max_fr));
  STTS_CHECK(!(mel_rows || raw_rows) || ld >= n_mels, "log_mel: ld %d < %d mel bins", ld, n_mels);
  STTS_CHECK(std::isfinite(mean) && std::isfinite(stdv) && stdv != 0.0, "log_mel: mean %g / std %g", mean, stdv);
  STTS_HIP(hipSetDevice(c->device));
  const LogMelTables* t = nullptr;
  STTS_TRY(log_mel_tables(c, n_fft, win_length, n_mels, sample_rate, &t));
  return launch_log_mel((hipStream_t)stream, *t, n_fft, win_length, hop_length, n_mels, n_utt, max_fr, sample_off_dev, row_off_dev, wave, mean, stdv, mel_rows, ld,
                        energy, raw_rows, partials);
}

int stts_log_mel_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* row_off_host,
                         const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length, int n_mels, int sample_rate, double mean, double std,
                         float* mel_rows, int ld, float* energy, float* raw_rows) {
  API_BEGIN
  STTS_CHECK(mel_rows || energy || raw_rows, "log_mel: no output");
  return log_mel_entry(c, stream, n_utt, sample_off_host, sample_off_dev, row_off_host, row_off_dev, wave, n_fft, win_length, hop_length, n_mels, sample_rate, mean, std,
                       mel_rows, ld, energy, raw_rows, nullptr);
  API_END
}

int stts_log_mel_stats(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* row_off_host,
                       const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length, int n_mels, int sample_rate, double* partials,
                       double* stats) {
  API_BEGIN
  STTS_CHECK(partials && stats, "log_mel_stats: null argument");
  STTS_CHECK(n_utt > 0 && sample_off_host && row_off_host && hop_length >= 1, "log_mel_stats: bad offsets");
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)sample_off_host[u + 1] - sample_off_host[u];
    STTS_CHECK(row_off_host[u + 1] - row_off_host[u] == n / hop_length + 1, "log_mel_stats: utterance %d must have all of its %ld frames", u, n / hop_length + 1);
  }
  STTS_TRY(log_mel_entry(c, stream, n_utt, sample_off_host, sample_off_dev, row_off_host, row_off_dev, wave, n_fft, win_length, hop_length, n_mels, sample_rate, 0.0, 1.0,
                         nullptr, 0, nullptr, nullptr, partials));
  hipLaunchKernelGGL(log_mel_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long)row_off_host[n_utt], n_mels, stats);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ validation scores (val_scores.hip.h)
extern "C" {

int stts_val_sizes(int n_utt, const int32_t* sample_off_host, int n_fft, int hop_length, int64_t* sizes) {
  API_BEGIN
  STTS_CHECK(sizes, "val_sizes: null argument");
  STTS_TRY(log_mel_check_geometry(n_fft, n_fft, hop_length, 1, 2));
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && sample_off_host && sample_off_host[0] == 0, "val_sizes: bad offsets");
  int64_t rows = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long n = (long)sample_off_host[u + 1] - sample_off_host[u];
    STTS_CHECK(n > n_fft / 2, "val_sizes: utterance %d has %ld samples; the reflect padding needs more than n_fft / 2 = %d", u, n, n_fft / 2);
    rows += n / hop_length + 1;
  }
  STTS_CHECK(rows <= INT32_MAX, "val_sizes: %lld frames do not fit 32-bit row offsets", (long long)rows);
  sizes[0] = rows;
  sizes[1] = 2 * rows;
  sizes[2] = 4 * rows;
  sizes[3] = rows * (n_fft / 2 + 1);
  return 0;
  API_END
}

static int val_spec_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* row_off_host,
                          const int32_t* row_off_dev, const float* a, const float* b, int n_fft, int win_length, int hop_length, int n_mels, int sample_rate,
                          float* mag, int ld_mag, float* fft_mag, float* phase, int ld_bins, double* partials, double* sums) {
  STTS_TRY(log_mel_check_geometry(n_fft, win_length, hop_length, n_mels, sample_rate));
  int max_fr = 0;
  STTS_TRY(val_check_offsets(b ? "val_mel_sums" : "multi_spectrogram", n_utt, sample_off_host, row_off_host, n_fft, hop_length, &max_fr));
  STTS_CHECK(c && sample_off_dev && row_off_dev && a, "val_scores: null argument");
  STTS_CHECK(!mag || ld_mag >= n_mels, "multi_spectrogram: ld_mag %d < %d mel bins", ld_mag, n_mels);
  STTS_CHECK(!(fft_mag || phase) || ld_bins >= n_fft / 2 + 1, "multi_spectrogram: ld_bins %d < %d bins", ld_bins, n_fft / 2 + 1);
  STTS_HIP(hipSetDevice(c->device));
  const LogMelTables* t = nullptr;
  STTS_TRY(log_mel_tables(c, n_fft, win_length, n_mels, sample_rate, &t));
  return launch_val_spec((hipStream_t)stream, *t, n_fft, win_length, hop_length, n_mels, n_utt, max_fr, sample_off_dev, row_off_dev, a, b, mag, ld_mag, fft_mag,
                         phase, ld_bins, partials, sums);
}

int stts_multi_spectrogram_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev,
                                   const int32_t* row_off_host, const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length,
                                   int n_mels, int sample_rate, float* mag_rows, int ld_mag, float* fft_mag_rows, float* phase_rows, int ld_bins) {
  API_BEGIN
  STTS_CHECK(mag_rows || fft_mag_rows || phase_rows, "multi_spectrogram: no output");
  return val_spec_entry(c, stream, n_utt, sample_off_host, sample_off_dev, row_off_host, row_off_dev, wave, nullptr, n_fft, win_length, hop_length, n_mels,
                        sample_rate, mag_rows, ld_mag, fft_mag_rows, phase_rows, ld_bins, nullptr, nullptr);
  API_END
}

int stts_val_mel_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* pred_off_host, const int32_t* sample_off_dev,
                      const int32_t* row_off_host, const int32_t* row_off_dev, const float* target, const float* pred, int n_fft, int win_length,
                      int hop_length, int n_mels, int sample_rate, double* partials, double* sums) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && sample_off_host && pred_off_host, "val_mel_sums: bad offsets");
  for (int u = 0; u < n_utt; ++u) {
    const long nt = (long)sample_off_host[u + 1] - sample_off_host[u], np = (long)pred_off_host[u + 1] - pred_off_host[u];
    STTS_CHECK(nt == np, "val_mel_sums: utterance %d: the target has %ld samples, the prediction %ld", u, nt, np);
  }
  STTS_CHECK(pred && partials && sums, "val_mel_sums: null argument");
  return val_spec_entry(c, stream, n_utt, sample_off_host, sample_off_dev, row_off_host, row_off_dev, target, pred, n_fft, win_length, hop_length, n_mels,
                        sample_rate, nullptr, 0, nullptr, nullptr, 0, partials, sums);
  API_END
}

int stts_val_magphase_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* row_off_host,
                           const int32_t* row_off_dev, const float* gt, const float* logamp_rows, const float* phase_rows, int ld, int n_fft, int win_length,
                           int hop_length, double* scratch, double* partials, double* sums) {
  API_BEGIN
  STTS_TRY(log_mel_check_geometry(n_fft, win_length, hop_length, 1, 2));
  int max_fr = 0;
  STTS_TRY(val_check_offsets("val_magphase_sums", n_utt, sample_off_host, row_off_host, n_fft, hop_length, &max_fr));
  STTS_CHECK(c && sample_off_dev && row_off_dev && gt && logamp_rows && phase_rows && scratch && partials && sums, "val_magphase_sums: null argument");
  STTS_CHECK(ld >= n_fft / 2 + 1, "val_magphase_sums: ld %d < %d bins", ld, n_fft / 2 + 1);
  STTS_HIP(hipSetDevice(c->device));
  const ValTables* t = nullptr;
  STTS_TRY(val_tables(c, n_fft, win_length, &t));
  return launch_val_magphase((hipStream_t)stream, *t, n_fft, win_length, hop_length, n_utt, max_fr, sample_off_dev, row_off_dev, gt, logamp_rows, phase_rows, ld,
                             scratch, partials, sums);
  API_END
}

int stts_val_smooth_l1_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b,
                            double* sums) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && off_host && off_host[0] == 0, "val_smooth_l1_sums: bad offsets");
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(off_host[u + 1] > off_host[u], "val_smooth_l1_sums: utterance %d has no values", u);
  STTS_CHECK(c && off_dev && a && b && sums, "val_smooth_l1_sums: null argument");
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(val_smooth_l1_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a, b, off_dev, sums);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_val_diff_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b, int kind,
                       double* sums) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && off_host && off_host[0] == 0, "val_diff_sums: bad offsets");
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(off_host[u + 1] > off_host[u], "val_diff_sums: utterance %d has no values", u);
  STTS_CHECK(c && off_dev && a && b && sums, "val_diff_sums: null argument");
  STTS_CHECK(kind == 0 || kind == 1, "val_diff_sums: kind must be 0 (absolute) or 1 (squared), got %d", kind);
  STTS_HIP(hipSetDevice(c->device));
  if (kind == 0) hipLaunchKernelGGL(val_diff_kernel<0>, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a, b, off_dev, sums);
  else hipLaunchKernelGGL(val_diff_kernel<1>, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a, b, off_dev, sums);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

int stts_val_duration_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* p_off_host, const int32_t* p_off_dev, const float* logits, int ld, int classes,
                           const int32_t* targets, const float* weight, double* sums) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && n_utt <= 65535 && p_off_host && p_off_host[0] == 0, "val_duration_sums: bad offsets");
  for (int u = 0; u < n_utt; ++u) STTS_CHECK(p_off_host[u + 1] > p_off_host[u], "val_duration_sums: utterance %d has no tokens", u);
  STTS_CHECK(classes >= 2 && classes <= 64 && ld >= classes, "val_duration_sums: %d classes in rows of %d; one lane per class takes 2 to 64", classes, ld);
  STTS_CHECK(c && p_off_dev && logits && targets && weight && sums, "val_duration_sums: null argument");
  STTS_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(val_duration_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, logits, ld, classes, targets, weight, p_off_dev, sums);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ windowed-sinc resampler (resample.hip.h)
extern "C" {

int stts_resample_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int* o, int* n, int* width, int* taps) {
  API_BEGIN
  ResampleGeom g;
  STTS_TRY(resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff, &g));
  if (o) *o = g.o;
  if (n) *n = g.n;
  if (width) *width = g.width;
  if (taps) *taps = g.taps;
  return 0;
  API_END
}

int64_t stts_resample_out_length(int64_t samples, int orig_freq, int new_freq) {
  if (samples < 0 || orig_freq < 1 || new_freq < 1) return -1;
  const long d = resample_gcd(orig_freq, new_freq);
  return resample_out_length(samples, (int)(orig_freq / d), (int)(new_freq / d));
}

int stts_resample_tile(int orig_freq, int new_freq) {
  if (orig_freq < 1 || new_freq < 1) return -1;
  const long d = resample_gcd(orig_freq, new_freq);
  if (orig_freq / d > kResampleMaxFreq || new_freq / d > kResampleMaxFreq) return -1;
  return resample_tile((int)(orig_freq / d), (int)(new_freq / d));
}

int stts_resample_forward(stts_ctx* c, void* stream, int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int method, double beta, int n_utt,
                          const int32_t* off_in_host, const int32_t* off_in_dev, const int32_t* off_out_host, const int32_t* off_out_dev, const float* in,
                          float* out) {
  API_BEGIN
  // the interface conditions first: they read host arrays only, so a caller without a context still gets the status that names the number
  ResampleGeom g;
  STTS_TRY(resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff, &g));
  STTS_CHECK(method == RESAMPLE_HANN || method == RESAMPLE_KAISER, "resample: method %d is neither 0 (sinc_interp_hann) nor 1 (sinc_interp_kaiser)", method);
  STTS_CHECK(method != RESAMPLE_KAISER || (std::isfinite(beta) && beta >= 0.0 && beta <= 512.0), "resample: beta %g is outside [0, 512]", beta);
  long max_out = 0;
  STTS_TRY(resample_check_offsets(n_utt, off_in_host, off_out_host, g, &max_out));
  STTS_CHECK(c && off_in_dev && off_out_dev && in && out, "resample: null argument");
  STTS_HIP(hipSetDevice(c->device));
  if (g.o == g.n) {  // equal rates: the input bits
    STTS_HIP(hipMemcpyAsync(out, in, (size_t)off_in_host[n_utt] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
  }
  const ResampleTable* t = nullptr;
  STTS_TRY(resample_table(c, (hipStream_t)stream, g, lowpass_filter_width, rolloff, method, beta, &t));
  return launch_resample((hipStream_t)stream, *t, g, n_utt, max_out, off_in_dev, off_out_dev, in, out);
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ HuBERT voice conversion (hubert.hip.h)
extern "C" {

#define HB_CHECK(mask)                                                               \
  READY_CHECK(c->hubert, mask);                                                      \
  HubertModel& H = *static_cast<HubertModel*>(c->hubert.get())

size_t stts_hubert_workspace_bytes(const stts_ctx* c, int64_t rows_T, int n_utt, int max_len) { return hubert_workspace_bytes(c, rows_T, n_utt, max_len); }

int stts_speaker_style(stts_ctx* c, void* stream, int n_utt, const float* spk_emb, int ld, float* style_out, float* pe_style_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  HB_CHECK((style_out ? STTS_W_HUBERT : 0) | (pe_style_out ? STTS_W_HUBERT_PE : 0));
  STTS_CHECK(n_utt > 0 && spk_emb, "speaker_style: bad argument");
  Arena a(ws, ws_bytes);
  return speaker_style(c, H, st, n_utt, spk_emb, ld, style_out, pe_style_out, a);
  API_END
}

int stts_hubert_encoder_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* feats, int ld_feats,
                                float* asr_out, int ld_asr, void* ws, size_t ws_bytes) {
  API_BEGIN
  HB_CHECK(STTS_W_HUBERT);
  STTS_TRY(seg_ok(n_utt, off_T_host, off_T_dev));
  STTS_CHECK(feats && asr_out, "hubert_encoder: null argument");
  STTS_CHECK(ld_feats >= round_up(H.sp.hubert_dim, 32) && ld_feats % 4 == 0, "feature rows: ld_feats %d must be a multiple of 4 covering %d columns (hubert.hidden_dim %d padded to 32)",
             ld_feats, round_up(H.sp.hubert_dim, 32), H.sp.hubert_dim);
  STTS_CHECK(ld_asr >= H.sp.enc.C, "ld_asr too small");
  Seg s{n_utt, off_T_host, off_T_dev};
  Arena a(ws, ws_bytes);
  return hubert_encoder_forward(c, H, st, s, feats, ld_feats, asr_out, ld_asr, a);
  API_END
}

int stts_hubert_pitch_energy_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* feats, int ld_feats,
                                     const float* pe_style, float* f0_out, float* energy_out, float* prosody_tap, void* ws, size_t ws_bytes) {
  API_BEGIN
  HB_CHECK(STTS_W_HUBERT_PE);
  STTS_TRY(seg_ok(n_utt, off_T_host, off_T_dev));
  STTS_CHECK(feats && pe_style && f0_out && energy_out, "hubert_pitch_energy: null argument");
  STTS_CHECK(ld_feats >= round_up(H.pe.hubert_dim, 32) && ld_feats % 4 == 0, "feature rows: ld_feats %d must be a multiple of 4 covering %d columns (hubert.hidden_dim %d padded to 32)",
             ld_feats, round_up(H.pe.hubert_dim, 32), H.pe.hubert_dim);
  Seg s{n_utt, off_T_host, off_T_dev};
  Arena a(ws, ws_bytes);
  return hubert_pitch_energy_forward(c, H, st, s, feats, ld_feats, pe_style, f0_out, energy_out, prosody_tap, a);
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ MelStyleEncoder (mel_style.hip.h)
extern "C" {

static int mel_style_get(stts_ctx* c, int which, const MelStyleW** E) {
  STTS_CHECK(c && (which == STTS_W_PE_MEL_STYLE || which == STTS_W_CFM_PITCH), "mel_style: `which` must be STTS_W_PE_MEL_STYLE or STTS_W_CFM_PITCH");
  STTS_CHECK(c->mel_style && (c->ready & which) == which, "weights for this stage are not finalized (need components 0x%x, have 0x%x)", which, c->ready);
  *E = &static_cast<MelStyleModel*>(c->mel_style.get())->enc[which == STTS_W_PE_MEL_STYLE ? 0 : 1];
  return 0;
}

size_t stts_mel_style_workspace_bytes(stts_ctx* c, int which, int64_t rows_T, int n_utt) {
  const MelStyleW* E = nullptr;
  if (mel_style_get(c, which, &E) != 0) return 0;
  return mel_style_workspace_bytes(*E, rows_T, n_utt);
}

static int mel_style_entry(stts_ctx* c, void* stream, int which, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* mel,
                           int ld, float* style_out, float* taps, void* ws, size_t ws_bytes) {
  const MelStyleW* E = nullptr;
  STTS_TRY(mel_style_get(c, which, &E));
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  STTS_CHECK(mel && style_out, "mel_style: null argument");
  STTS_CHECK(ld >= E->n_mels, "mel rows: ld %d < n_mels %d", ld, E->n_mels);
  STTS_HIP(hipSetDevice(c->device));
  Seg s{n_utt, seg_off_host, seg_off_dev};
  Arena a(ws, ws_bytes);
  return mel_style_forward(*E, (hipStream_t)stream, s, mel, ld, style_out, E->style_dim, taps, a);
}

int stts_mel_style_forward(stts_ctx* c, void* stream, int which, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* mel, int ld,
                           float* style_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  return mel_style_entry(c, stream, which, n_utt, seg_off_host, seg_off_dev, mel, ld, style_out, nullptr, ws, ws_bytes);
  API_END
}

int stts_mel_style_forward_taps(stts_ctx* c, void* stream, int which, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* mel,
                                int ld, float* style_out, float* block_taps, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(block_taps, "mel_style: null block_taps");
  return mel_style_entry(c, stream, which, n_utt, seg_off_host, seg_off_dev, mel, ld, style_out, block_taps, ws, ws_bytes);
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ CfmPitchPredictor (cfm_pitch.hip.h)
extern "C" {

static int cfm_pitch_get(stts_ctx* c, const CfmPitchNetW** W) {
  STTS_CHECK(c && c->cfm_pitch && (c->ready & STTS_W_CFM_PITCH_NET), "weights for this stage are not finalized (need components 0x%x, have 0x%x)",
             STTS_W_CFM_PITCH_NET, c ? c->ready : 0);
  *W = static_cast<const CfmPitchNetW*>(c->cfm_pitch.get());
  return 0;
}

size_t stts_cfm_pitch_workspace_bytes(stts_ctx* c, int64_t rows_T, int n_utt) {
  const CfmPitchNetW* W = nullptr;
  if (cfm_pitch_get(c, &W) != 0) return 0;
  return cfm_pitch_workspace_bytes(*W, rows_T, n_utt);
}

static int cfm_pitch_entry(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* asr, int ld_asr,
                           const float* spk_style, float* out_normed, float* out_hz, float mean, float stdv, const float* uv, float* taps, void* ws,
                           size_t ws_bytes) {
  const CfmPitchNetW* W = nullptr;
  STTS_TRY(cfm_pitch_get(c, &W));
  STTS_TRY(seg_ok(n_utt, off_host, off_dev));
  STTS_CHECK(asr && spk_style && out_normed && ws, "cfm_pitch: null argument");
  STTS_CHECK(ld_asr >= W->asr_dim && ld_asr % 4 == 0, "asr rows: ld %d must be >= asr_dim %d and a multiple of 4", ld_asr, W->asr_dim);
  STTS_CHECK(!out_hz || (std::isfinite(mean) && std::isfinite(stdv)), "cfm_pitch: the F0 log2 statistics must be finite");
  STTS_HIP(hipSetDevice(c->device));
  Seg s{n_utt, off_host, off_dev};
  Arena a(ws, ws_bytes);
  return cfm_pitch_forward(*W, (hipStream_t)stream, s, asr, ld_asr, spk_style, out_normed, out_hz, mean, stdv, out_hz ? uv : nullptr, taps, a);
}

int stts_cfm_pitch_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* asr, int ld_asr,
                           const float* spk_style, float* out_normed, float* out_hz, float f0_log2_mean, float f0_log2_std, const float* uv, void* ws,
                           size_t ws_bytes) {
  API_BEGIN
  return cfm_pitch_entry(c, stream, n_utt, off_T_host, off_T_dev, asr, ld_asr, spk_style, out_normed, out_hz, f0_log2_mean, f0_log2_std, uv, nullptr, ws,
                         ws_bytes);
  API_END
}

int stts_cfm_pitch_forward_taps(stts_ctx* c, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* asr, int ld_asr,
                                const float* spk_style, float* out_normed, float* out_hz, float f0_log2_mean, float f0_log2_std, const float* uv,
                                float* taps, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(taps, "cfm_pitch: null taps");
  return cfm_pitch_entry(c, stream, n_utt, off_T_host, off_T_dev, asr, ld_asr, spk_style, out_normed, out_hz, f0_log2_mean, f0_log2_std, uv, taps, ws,
                         ws_bytes);
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ PosteriorEncoder (posterior.hip.h)
extern "C" {

size_t stts_posterior_workspace_bytes(const stts_ctx* c, int64_t rows, int n_utt, int max_len) {
  if (!c || !c->posterior || !(c->ready & STTS_W_POSTERIOR) || rows <= 0 || n_utt <= 0) return 0;
  const SynthSeg syn(rows, n_utt, max_len);
  return dry_run_bytes([&](Arena a) {
    PostIO io{};
    (void)posterior_forward(const_cast<stts_ctx*>(c), nullptr, syn.seg(), io, a);
  });
}

int stts_posterior_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* audio, float* har_spec,
                           float* har_phase, int ld_har, const float* style, const float* noise, float* z_out, float* mean_out, float* logstd_out, float* mel_out,
                           int ld_mel, float* x0_out, float* wn_out, void* ws, size_t ws_bytes, int seg_flags) {
  API_BEGIN
  READY_CHECK(c->posterior, STTS_W_POSTERIOR);
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  Seg s{n_utt, seg_off_host, seg_off_dev};
  s.cap = (seg_flags & STTS_SEG_CAPACITY) != 0;
  const PostIO io{audio, har_spec, har_phase, ld_har, style, noise, z_out, mean_out, logstd_out, mel_out, ld_mel, x0_out, wn_out};
  STTS_TRY(posterior_check(c, s, io));
  Arena a(ws, ws_bytes);
  return posterior_forward(c, st, s, io, a);
  API_END
}

#ifdef STTS_TEST_OPS
int stts_op_posterior_layer(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int layer, int form, int out_acc,
                            const float* h_in, const float* out_in, const float* cond, int ld_cond, float* h_out, float* out_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  READY_CHECK(c->posterior, STTS_W_POSTERIOR);
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  const PostW& P = *static_cast<const PostW*>(c->posterior.get());
  const Seg s{n_utt, seg_off_host, seg_off_dev};
  const int H = P.hidden;
  STTS_CHECK(layer >= 0 && layer < P.n_layers, "op_posterior_layer: layer %d of %d", layer, P.n_layers);
  STTS_CHECK(form == 0 || ((form == 16 || form == 32 || form == 64) && P.fused), "op_posterior_layer: form %d is not built for this encoder", form);
  STTS_CHECK(h_in && out_in && cond && h_out && out_out && h_out != h_in && out_out != out_in, "op_posterior_layer: null or aliased buffers");
  STTS_CHECK(ld_cond % 4 == 0 && ld_cond >= 2 * H * P.n_layers, "op_posterior_layer: ld_cond %d < %d", ld_cond, 2 * H * P.n_layers);
  for (const void* ptr : {(const void*)h_in, (const void*)out_in, (const void*)cond, (const void*)h_out, (const void*)out_out})
    STTS_CHECK((uintptr_t)ptr % 16 == 0, "op_posterior_layer: buffers must be 16-byte aligned");
  Arena a(ws, ws_bytes);
  float* acts = a.get<float>((size_t)s.rows() * H);
  STTS_CHECK(a.ok, "op_posterior_layer: workspace too small");
  const size_t bytes = (size_t)s.rows() * H * sizeof(float);
  const bool last = layer == P.n_layers - 1, fused = form != 0;
  STTS_HIP(hipMemcpyAsync(out_out, out_in, bytes, hipMemcpyDeviceToDevice, st));
  // the fused form writes h into another buffer (h_out); the generic one and the last layer work on a copy
  if (!fused || last) STTS_HIP(hipMemcpyAsync(h_out, h_in, bytes, hipMemcpyDeviceToDevice, st));
  float* after = nullptr;
  const PostPlan plan{fused, form};
  if (fused) STTS_TRY(posterior_layer(c, st, s, P, plan, layer, out_acc != 0, const_cast<float*>(h_in), h_out, out_out, acts, cond, ld_cond, &after));
  else STTS_TRY(posterior_layer(c, st, s, P, plan, layer, out_acc != 0, h_out, nullptr, out_out, acts, cond, ld_cond, &after));
  return 0;
  API_END
}
#endif

}  // extern "C"

#include "mrf_block.hip.h"
#ifdef STTS_TEST_OPS  // single-layer test operators + the contraction micro-benchmark (not part of the product surface)
#include "test_ops.hip.h"
#endif

// ------------------------------------------------------------------------------------------------ flow statistics (flow_stats.hip.h)
#include "flow_stats.hip.h"

namespace stts {
int finalize_flow_stats_component(stts_ctx* c) {
  if (!c->flow_stats) c->flow_stats = std::make_shared<FStatW>();
  // fp32 whatever the precision; the contractions in the split-fp32 form where the engine allows it
  PackScope scope(c, {PREC_F32, true, 32, STTS_W_FLOW_STATS});
  STTS_TRY(finalize_flow_stats(c, static_cast<FStatW*>(c->flow_stats.get())));
  c->ready |= STTS_W_FLOW_STATS;
  return 0;
}
}  // namespace stts

extern "C" {

size_t stts_flow_stats_workspace_bytes(const stts_ctx* c, int64_t rows, int n_utt, int max_len) {
  if (!c || !c->flow_stats || !(c->ready & STTS_W_FLOW_STATS) || rows <= 0 || n_utt <= 0) return 0;
  const SynthSeg syn(rows, n_utt, max_len);
  // exactly what the stage carves (dry_run_bytes adds 4 KiB of slack for stages whose sub-arenas round on their own; this one carves from one arena,
  // every piece a multiple of 256 bytes): one byte less is refused
  return dry_run_bytes([&](Arena a) {
    FStatIO io{};
    (void)flow_stats_forward(const_cast<stts_ctx*>(c), nullptr, syn.seg(), io, a);
  }) - 4096;
}

int stts_flow_stats_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int reverse, const float* z_in,
                            const float* mean_in, const float* logstd_in, const float* style, float* z_out, float* mean_out, float* logstd_out, void* ws, size_t ws_bytes,
                            int seg_flags) {
  API_BEGIN
  READY_CHECK(c->flow_stats, STTS_W_FLOW_STATS);
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  Seg s{n_utt, seg_off_host, seg_off_dev};
  s.cap = (seg_flags & STTS_SEG_CAPACITY) != 0;
  const FStatIO io{reverse, z_in, mean_in, logstd_in, style, z_out, mean_out, logstd_out};
  STTS_TRY(flow_stats_check(c, s, io));
  Arena a(ws, ws_bytes);
  return flow_stats_forward(c, st, s, io, a);
  API_END
}

int stts_prior_stats_forward(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ld_x, const float* noise,
                             float* z_out, float* mean_out, float* logstd_out, void* ws, size_t ws_bytes, int seg_flags) {
  API_BEGIN
  READY_CHECK(c->flow_stats, STTS_W_FLOW_STATS);
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  Seg s{n_utt, seg_off_host, seg_off_dev};
  STTS_CHECK(!(seg_flags & STTS_SEG_CAPACITY), "the flow statistics take plain segments (no STTS_SEG_CAPACITY)");
  const FStatW& P = *static_cast<const FStatW*>(c->flow_stats.get());
  STTS_CHECK(x && noise && z_out && mean_out && logstd_out, "prior_stats_forward: null argument");
  STTS_CHECK(ld_x % 4 == 0 && ld_x >= P.in_ch, "prior_stats_forward: ld_x %d must be a multiple of 4 covering the %d columns the packer built", ld_x, P.in_ch);
  for (const void* ptr : {(const void*)x, (const void*)noise, (const void*)z_out, (const void*)mean_out, (const void*)logstd_out})
    STTS_CHECK((uintptr_t)ptr % 16 == 0, "prior_stats_forward: buffers must be 16-byte aligned");
  Arena a(ws, ws_bytes);
  return prior_stats_forward(c, st, s, x, ld_x, noise, z_out, mean_out, logstd_out, a);
  API_END
}

int stts_val_kl_sums(stts_ctx* c, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, int kind, const float* a, const float* b, const float* cc,
                     const float* d, int ld, int C, double* sums, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c, "null ctx");
  STTS_HIP(hipSetDevice(c->device));
  STTS_TRY(seg_ok(n_utt, off_host, off_dev));
  STTS_CHECK(kind == 0 || kind == 1, "val_kl_sums: kind must be 0 (kl_loss) or 1 (kl_loss_normal)");
  STTS_CHECK(a && b && cc && d && sums, "val_kl_sums: null argument");
  STTS_CHECK(C > 0 && ld >= C, "val_kl_sums: ld %d < C %d", ld, C);
  const Seg s{n_utt, off_host, off_dev};
  Arena ar(ws, ws_bytes);
  return val_kl_sums((hipStream_t)stream, s, kind, a, b, cc, d, ld, C, sums, ar);
  API_END
}

#ifdef STTS_TEST_OPS
int stts_op_flow_stats_layer(stts_ctx* c, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int layer, int reverse, int form,
                             const float* z_in, const float* mean_in, const float* logstd_in, const float* style, float* z_out, float* mean_out, float* logstd_out,
                             float* h0_out, void* ws, size_t ws_bytes) {
  API_BEGIN
  READY_CHECK(c->flow_stats, STTS_W_FLOW_STATS);
  STTS_TRY(seg_ok(n_utt, seg_off_host, seg_off_dev));
  const Seg s{n_utt, seg_off_host, seg_off_dev};
  const FStatW& P = *static_cast<const FStatW*>(c->flow_stats.get());
  STTS_CHECK(layer >= 0 && layer < 8, "op_flow_stats_layer: layer %d of 8", layer);
  STTS_CHECK(form == 0 || ((form == 16 || form == 32 || form == 64) && P.fused), "op_flow_stats_layer: form %d is not built for this flow", form);
  const FStatIO io{reverse, z_in, mean_in, logstd_in, style, z_out, mean_out, logstd_out};
  STTS_TRY(flow_stats_check(c, s, io));
  STTS_CHECK(!h0_out || (uintptr_t)h0_out % 16 == 0, "op_flow_stats_layer: buffers must be 16-byte aligned");
  Arena a(ws, ws_bytes);
  const FStatBufs b = flow_stats_carve(P, s, a);
  STTS_CHECK(a.ok, "op_flow_stats_layer: workspace too small");
  const size_t bytes = (size_t)s.rows() * P.fh * sizeof(float);
  STTS_HIP(hipMemcpyAsync(z_out, z_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipMemcpyAsync(mean_out, mean_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipMemcpyAsync(logstd_out, logstd_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_TRY(run_style(st, P.cond, style, n_utt, b.cond));
  if (form == 0) return flow_stats_layer(st, s, P, layer, reverse, z_out, mean_out, logstd_out, b);  // (runs its own `pre`; hands back no next h_0)
  const int next = reverse ? layer - 1 : (layer < 7 ? layer + 1 : -1);
  float* h = b.hf;
  STTS_TRY(flow_stats_pre(st, s, P, layer, z_out, h));
  STTS_TRY(flow_stats_layer_fused(st, s, P, form, layer, next, reverse, z_out, mean_out, logstd_out, b, &h));
  if (next >= 0 && h0_out) STTS_HIP(hipMemcpyAsync(h0_out, h, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
  API_END
}
#endif

}  // extern "C"

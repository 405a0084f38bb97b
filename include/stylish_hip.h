/* stylish_hip.h — C-ABI of the MI355X (gfx950) implementation of the Stylish-TTS inference hot path.
 *
 * The reference (Fannovel16/stylish-tts) is 100 % Python: it has no FFI, plugin or operator interface, only
 * nn.Module.forward() signatures.  This library sits UNDERNEATH those modules: the Python
 * shims in stylish_tts_amd/modules.py keep the reference's constructor arguments, forward() signatures and
 * state_dict keys and call the entry points below through ctypes.  Each entry point names the reference
 * function it replaces (paths relative to /root/reference/src/stylish_tts/).
 *
 * Conventions
 *  - plain C: pointers, sizes, int status (0 = ok; stts_last_error() gives the text).  Never throws.
 *  - `stream` is a hipStream_t passed as void*.  All work is enqueued on it; nothing synchronises unless stated.
 *  - device tensors are fp32, TIME-MAJOR packed rows: X[utterance offset + frame][channel], row stride `ld`
 *    floats (a multiple of 4).  Utterances are described by seg_off[n_utt + 1] (int32 row offsets), passed both
 *    as a host array (grid sizing) and as a device array (kernels).
 *  - the caller owns inputs, outputs and the workspace; the library owns the context and the packed weights.
 *  - noise is an explicit input (the reference draws it from the global torch generator:
 *    models/flow.py:314, models/generator.py:272,306).
 */
#ifndef STYLISH_HIP_H_
#define STYLISH_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct stts_ctx stts_ctx;

/* Model shape: the hot-path keys of ModelConfig (lib/config_loader.py:369-414, train/config/model.yml). */
typedef struct stts_model_dims {
  int32_t n_fft, win_length, hop_length, sample_rate; /* 2048, 1200, 300, 24000 (vocoder hop = hop_length/4) */
  int32_t style_dim, inter_dim;                      /* 64, 128 */
  int32_t dec_hidden, dec_residual;                  /* decoder.hidden_dim 512, residual_dim 64 */
  int32_t gen_input, gen_hidden, gen_inter, gen_io_kernel; /* generator.* : 512, 512, 1536, 7 */
  int32_t tokens, te_hidden, te_filter, te_heads, te_layers, te_kernel; /* text_encoder.* */
  int32_t style_layers;                              /* style_encoder.layers */
  int32_t dur_layers, dur_classes, dur_max;          /* duration_predictor.n_layer, duration_classes, max_duration */
  int32_t pe_inter;                                  /* pitch_energy_predictor.inter_dim */
} stts_model_dims;

const char* stts_last_error(void);
int stts_version(void);

/* Context: device selection + weights.  Weight tensors are handed over by their reference state_dict name,
 * prefixed with the module name used by build_model (models/models.py:79-101), e.g.
 * "speech_predictor.decoder.encode.conv1.parametrizations.weight.original1".  Data is copied (host fp32). */
int stts_ctx_create(const stts_model_dims* dims, int device, stts_ctx** out);
void stts_ctx_destroy(stts_ctx* ctx);
int stts_load_weight(stts_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim);
/* Fold weight-norm (w = g*v/||v||), re-lay out every conv/linear as W[cout][tap][cin] padded for the MFMA
 * tiles, upload.  `which` is a bit mask of the components whose weights have been loaded (one per reference
 * sub-module, so that a single module can be dropped in on its own): */
enum {
  STTS_W_DECODER = 1,        /* speech_predictor.decoder                                   models/decoder.py */
  STTS_W_FLOW = 2,           /* speech_predictor.{prior_encoder, flow, post_flow}          models/flow.py */
  STTS_W_GENERATOR = 4,      /* speech_predictor.generator                                 models/generator.py */
  STTS_W_SPEECH_TEXT = 8,    /* speech_predictor.{text_encoder, style_encoder}             models/speech_predictor.py:17-25 */
  STTS_W_DURATION = 16,      /* duration_predictor.*                                       models/duration_predictor.py */
  STTS_W_PE_TEXT = 32,       /* pe_text_encoder                                            models/models.py:49-52 */
  STTS_W_PE_STYLE = 64,      /* pe_text_style_encoder                                      models/models.py:53-57 */
  STTS_W_PITCH_ENERGY = 128, /* pitch_energy_predictor.*                                   models/pitch_energy_predictor.py */
  STTS_W_FRAME_PATH = 7,
  STTS_W_ALL = 255,
  STTS_W_CFM = 256,          /* cfm_mel_decoder.* (finalized by stts_cfm_finalize, not part of STTS_W_ALL)  models/cfm/cfm_mel_decoder.py */
  STTS_W_HUBERT = 512,       /* hubert_speech_predictor.{phone_encoder, style_encoder} (not part of STTS_W_ALL) models/speech_predictor.py:132-148 */
  STTS_W_HUBERT_PE = 1024,   /* hubert_pitch_energy_predictor.* (not part of STTS_W_ALL)   models/pitch_energy_predictor.py:124-191 */
  STTS_W_PE_MEL_STYLE = 2048, /* pe_mel_style_encoder.* (not part of STTS_W_ALL)            models/models.py:57-62 */
  STTS_W_CFM_PITCH = 4096,   /* cfm_pitch_predictor.spk_emb.* (not part of STTS_W_ALL)     models/cfm/cfm_pitch_predictor.py:25-27 */
  STTS_W_CFM_PITCH_NET = 8192, /* cfm_pitch_predictor.{asr_emb, blocks, out_proj} (in_proj.* is accepted and ignored; not part of STTS_W_ALL) */
  STTS_W_SSL = 16384,        /* hubert.model.* = AdaptiveHubert (finalized by stts_ssl_finalize, not part of STTS_W_ALL)      train/models/ssl.py:16-31 */
  STTS_W_RMVPE = 32768,      /* rmvpe.* = the RMVPE pitch extractor E2E0 (finalized by stts_rmvpe_finalize, not part of STTS_W_ALL) train/dataprep/rmvpe/model.py:49-86 */
  STTS_W_ALIGNER = 65536,    /* text_aligner.* = the TDNN CTC aligner (finalized by stts_aligner_finalize, not part of STTS_W_ALL)           train/models/text_aligner.py */
  STTS_W_WAVLM = 131072,     /* wavlm.* = transformers' WavLMModel, the network of the "slm" distance (finalized by stts_wavlm_finalize, not part of STTS_W_ALL) train/losses.py:408-426 */
  STTS_W_POSTERIOR = 262144, /* speech_predictor.posterior_encoder.* (stts_finalize_weights; not part of STTS_W_ALL)                       models/flow.py:234-293 */
  STTS_W_FLOW_STATS = 524288 /* speech_predictor.flow.flows.* + prior_encoder.* packed again in fp32 for the flow statistics (stts_finalize_weights; not part of STTS_W_ALL) */
};
int stts_finalize_weights(stts_ctx* ctx, int which);
/* Operand precision of the FRAME-RATE Conv1d / Linear contractions (call before the first stts_finalize_weights).
 * F32 is the reference's arithmetic (BASELINE cfg2).  BF16 / F16 (BASELINE cfg3 / cfg5): the operands of every matrix-core
 * contraction of the decoder, the flow and the vocoder are rounded to nearest-even exactly once - weights when they are packed,
 * activations either when a tile is staged for the matrix cores (calls of < 3 840 rows: they stay fp32 in HBM) or by the kernel
 * that produces them (larger calls: contraction inputs are 16-bit rows in HBM; the same arithmetic) - and products accumulate
 * in fp32; norms, gates, style projections, FFTs and every non-contraction kernel stay fp32.
 * The PHONEME-RATE predictors (text encoders, style encoders, duration and pitch / energy predictors) always run in fp32:
 * durations are integers (bit-exact against the fp32 reference in every mode) and those stages are latency-bound.
 * F32, how the fp32 products are formed (round 4): every finite fp32 operand with |x| >= 2^-110 is the EXACT sum of three bf16 numbers
 * (8 + 8 + 8 significand bits; from 0x7F7F8000 up the top term is 0x7F7F, not a rounding to Inf), so x * w is nine bf16 x bf16 products,
 * each exact in fp32; the frame-rate contractions run the six largest on the bf16 matrix cores with fp32 accumulation (the three dropped
 * terms are <= 2^-23 |x w|, 2^-27 |x w| rms, zero-mean: below the rounding of the fp32 accumulation that both forms share).  Nothing is
 * rounded to 16 bits: results agree with the f32 matrix cores' to fp32 accumulation noise (tests/test_hip_split_fp32.py,
 * tests/test_hip_split_fp32_edges.py: one exposed product per output, every tile and variant, against float64).  The domain:
 *  - |x| < 2^-110: the low terms are bf16 subnormals (step 2^-133), so an operand is off by at most 2^-134 - an absolute error of
 *    2^-134 |w| per product; v_mfma_f32_32x32x16_bf16 keeps bf16 subnormal inputs (measured: 2^40 * 2^-130 = 2^-90 exactly);
 *  - +-Inf is split (0, 0, +-Inf): its only nonzero term meets the other operand's top term, so products are IEEE's (+-Inf, NaN for
 *    Inf * 0) except Inf * Inf (NaN) and Inf times an fp32 subnormal below 2^-134 (its top term is 0: NaN); NaN stays NaN;
 *  - the Winograd forms (the k = 3 / 7 convs of long calls): a non-finite input turns its whole F(6, k) group of outputs NaN, and the
 *    transforms can overflow where the direct form would not (inputs near FLT_MAX);
 *  - pad columns of an activation (channels between the real count and the 32-aligned row width) must hold finite values: they meet
 *    zero weights, and Inf or NaN times zero is NaN.
 * F32_NATIVE keeps every fp32 contraction on v_mfma_f32_32x32x2_f32 (rounds 1-3; also process-wide with STTS_NO_X3=1). */
enum { STTS_PREC_F32 = 0, STTS_PREC_BF16 = 1, STTS_PREC_F16 = 2, STTS_PREC_F32_NATIVE = 3 };
int stts_set_precision(stts_ctx* ctx, int precision);
/* Reads the device-side error word (sets last_error): 1 = a voiced frame exists but no f0 > 20 Hz (the reference raises there,
 * models/generator.py:285), 2 = a token id outside the embedding table, 4 = an utterance
 * too short for the STFT's reflect padding.  Synchronises the stream. */
int stts_check_status(stts_ctx* ctx, void* stream);

/* Workspace the frame-rate stages need for `rows` vocoder frames (sum of T4) in `n_utt` utterances,
 * the longest having `max_len` frames. */
size_t stts_frame_workspace_bytes(const stts_ctx* ctx, int64_t rows, int n_utt, int max_len);
/* Row stride (floats) of the harmonic spectra `har_spec` / `har_phase` that stts_harmonic_stft writes and stts_vocoder_forward reads: the
 * n_fft/2 + 1 bins padded to the packed input width of the prior convs (32 in fp32, 64 in the 16-bit operand modes).  Valid after
 * stts_set_precision; callers size their buffers with it instead of mirroring the padding rule. */
int stts_har_ld(const stts_ctx* ctx);

/* Decoder.forward (models/decoder.py:47-60) incl. every AdaptiveDecoderBlock (models/ada_norm.py:166-182).
 * asr [rows, ld_asr>=128], pitch/energy [rows] (already at the hop/4 rate), style [n_utt, 64] -> x [rows, 512]. */
int stts_decoder_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                         const float* asr, int ld_asr, const float* pitch, const float* energy, const float* style,
                         float* x_out, int ld_x, void* ws, size_t ws_bytes);

/* PriorEncoder.forward (models/flow.py:311-315) + ResidualCouplingBlock.forward(reverse=True)
 * (models/flow.py:132-151) + post_flow (models/speech_predictor.py:111).
 * x [rows,512], prior_noise [rows,128] ~ N(0,1) -> mel [rows,512]; optional z_prior / z_flow [rows,128]. */
int stts_prior_flow_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                            const float* x, int ld_x, const float* style, const float* prior_noise, float* mel_out, int ld_mel,
                            float* z_prior_out, float* z_flow_out, void* ws, size_t ws_bytes);

/* generate_pcph (models/generator.py:247-315) + TorchSTFT.transform + atan2 (models/generator.py:32-44,406-410).
 * pitch [rows], src_noise [75*rows] ~ N(0,1), init_phase: device pointer to ONE float in [0,1) shared by the call.
 * batch_scope != 0: harmonic count from the min f0 of the whole call (reference semantics of a batched call);
 * 0: per utterance (the reference called per utterance).  Outputs har_spec / har_phase [rows, ld>=1025],
 * optional prior_signal [75*rows].
 * PARITY NOTE (conditional): har_phase = atan2(Im, Re) is discontinuous and feeds phase_prior_conv linearly
 * (models/generator.py:408-413).  With center=True reflect padding frame 0 is even-symmetric, so its spectrum is real up to FFT
 * rounding and every negative-real bin is +pi or -pi by the sign of rounding noise - in torch.stft too; ~0-magnitude bins have
 * arbitrary phase.  This entry computes the transform in fp64 (the signs of the exact transform); it does NOT reproduce torch's
 * coin flips.  Consequence: waveforms match the reference within 1e-3 everywhere only after the reference's value is adopted at
 * those ill-conditioned bins (~0.09 % of the bins; tests do so through oracle.align_branch, which accepts a bin only if the two
 * angles agree mod 2 pi within 5e-3 or the magnitude is < 2e-4).  Un-adopted (what stts_frame_path computes) the first ~40 frames of
 * an utterance can differ from a given torch run by up to ~0.2, the rest by <= 1.5e-2; tests/test_hip_benchmarked_path.py pins
 * that every such difference lies inside the receptive field of an adopted bin. */
int stts_harmonic_stft(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                       const float* pitch, const float* src_noise, const float* init_phase, int batch_scope,
                       float* prior_signal_out, float* har_spec, float* har_phase, int ld_har, void* ws, size_t ws_bytes);

/* Generator.forward body + TorchSTFT.inverse + tanh (models/generator.py:412-433, ConvNeXtBlock :468-485,
 * GRN :496-499, AdaptiveLayerNorm models/ada_norm.py:193-201).
 * mel [rows,512], style [n_utt,64], har_spec/har_phase [rows, ld_har] -> audio [75*rows];
 * optional logamp / phase [rows, ld_lp>=1025] (row T4 of the reference's replicate pad equals row T4-1). */
int stts_vocoder_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                         const float* mel, int ld_mel, const float* style, const float* har_spec, const float* har_phase, int ld_har,
                         float* audio_out, float* logamp_out, float* phase_out, int ld_lp, void* ws, size_t ws_bytes);

/* PosteriorEncoder.forward (models/flow.py:282-293) [+ post_flow, models/speech_predictor.py:109]: a recording -> z ~ q(z | audio), the
 * latent that copy-synthesis vocodes.  Component STTS_W_POSTERIOR (keys "speech_predictor.posterior_encoder.*", either weight-norm flavour;
 * 12 layers, hidden 128, k = 3 at model.yml; dilation 1 only); fp32 arithmetic whatever stts_set_precision says.
 *   audio [75*rows] packed (h = hop_length / 4 samples per row), or NULL: har_spec / har_phase [rows, ld_har] are read as given (columns from
 *   n_fft/2 + 1 up to the packed input width - the bins rounded up to 32 - must be finite); with audio they are WRITTEN: the vocoder's STFT of
 *   the recording, its last frame dropped (flow.py:283-286).  ld_har: a multiple of 4, >= the bins rounded up to 32 (stts_har_ld fits).
 *   style [n_utt, 64], or NULL = the reference's g=None (no conditioning).  noise [rows,128] ~ N(0,1): the one draw (flow.py:292).
 *   z_out / mean_out / logstd_out [rows,128]: any of them optional.  mel_out [rows, ld_mel >= 512] (optional) = post_flow(z): needs STTS_W_FLOW.
 *   x0_out / wn_out [rows,128] (optional taps): cat[pre_spec, pre_phase] and the WaveNet's output.
 * Utterances are ragged and packed, each its own sequence with zero padding at its ends (the reference at B = 1).  seg_flags must be 0: capacity
 * segments are refused, as are an utterance too short for the STFT's reflect padding (from audio), a small ld_har, mel_out without STTS_W_FLOW and
 * a small workspace - each with stts_last_error set and nothing launched.  The WaveNet runs one fused launch per layer (wn_post_kernel) or as plain
 * contractions; STTS_POST_WN (read per call) = 0 | 16 | 32 | 64 forces the generic form or the fused one on that block height.
 * PARITY NOTE: as stts_harmonic_stft's - from audio, frame 0's negative-real bins are +-pi by rounding noise and pre_phase is linear in the
 * phase; tests adopt the reference's branch at those bins (oracle.align_branch) before they compare. */
int stts_posterior_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* audio,
                           float* har_spec, float* har_phase, int ld_har, const float* style, const float* noise, float* z_out, float* mean_out,
                           float* logstd_out, float* mel_out, int ld_mel, float* x0_out, float* wn_out, void* ws, size_t ws_bytes, int seg_flags);
/* Workspace stts_posterior_forward accepts for `rows` rows in `n_utt` utterances, the longest having `max_len` (a dry run of its own carving;
 * 0 before STTS_W_POSTERIOR is finalized). */
size_t stts_posterior_workspace_bytes(const stts_ctx* ctx, int64_t rows, int n_utt, int max_len);

/* Flow statistics: ResidualCouplingBlock.forward in both directions with the reference's three streams (models/flow.py:132-151, :196-218), the
 * prior with its three outputs (:311-315) and the sums behind kl_text / kl_audio (train/losses.py:157-222).  Component STTS_W_FLOW_STATS packs
 * its own fp32 copy of the already loaded keys "speech_predictor.flow.flows.{0,2,..,14}.*" (either weight-norm flavour) and
 * "speech_predictor.prior_encoder.*"; it may be finalized alone, before or after STTS_W_FLOW, with the same results bit for bit, and is fp32
 * whatever stts_set_precision says (validation numbers).
 *   z_in / mean_in / logstd_in [rows,128], style [n_utt,64] -> z_out / mean_out / logstd_out [rows,128] (other buffers than the inputs).
 *   reverse 0: layers 0 .. 7, each followed by a Flip:   z1 = m + z1 exp(s),    mean1 = m + mean1 exp(s),    logstd1 += s
 *   reverse 1: Flip, layer 7, ..., Flip, layer 0:        z1 = (z1 - m) exp(-s), mean1 = (mean1 - m) exp(-s), logstd1 -= s
 *   with m, s = proj_mean, proj_logstd of the WaveNet's output on the z stream's other half.  Layer f reads half f & 1 and updates the other; the
 *   half it reads leaves the layer bit-identical; after eight layers the halves are in their natural order.
 * Utterances are ragged and packed, each its own sequence with zero padding at its ends (the reference at B = 1, z_mask = 1).  Refused with
 * stts_last_error set and nothing launched: capacity segments (seg_flags must be 0), a small workspace, outputs that alias inputs, a missing component.
 * A coupling layer runs as plain contractions and one row kernel for the coupling (the generic form, any width) or as wn_stats_kernel, one fused launch
 * per WaveNet layer (width 128); STTS_FSTAT_WN (read per call) = 0 | 16 | 32 | 64 forces the generic form or the fused one on that block height. */
int stts_flow_stats_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int reverse, const float* z_in,
                            const float* mean_in, const float* logstd_in, const float* style, float* z_out, float* mean_out, float* logstd_out, void* ws,
                            size_t ws_bytes, int seg_flags);
/* Workspace stts_flow_stats_forward accepts (a dry run of its own carving, exact: one byte less is refused; 0 before STTS_W_FLOW_STATS is finalized). */
size_t stts_flow_stats_workspace_bytes(const stts_ctx* ctx, int64_t rows, int n_utt, int max_len);
/* PriorEncoder.forward with all three outputs: x [rows, ld_x >= 512] (the decoder's output), noise [rows,128] ~ N(0,1) -> mean_out, logstd_out and
 * z_out = mean + noise exp(logstd), each [rows,128].  Needs no workspace.  Refusals as above, and an ld_x that does not cover the packed input width. */
int stts_prior_stats_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ld_x,
                             const float* noise, float* z_out, float* mean_out, float* logstd_out, void* ws, size_t ws_bytes, int seg_flags);
/* sums[u] (device double [n_utt]) = utterance u's sum over rows and the C channels of the KL term, accumulated in fp64 from the fp32 rows [rows, ld]
 * on, in a fixed order, no atomics.  kind 0 = kl_loss(z_p = a, logs_q = b, m_p = c, logs_p = d): d - b - 0.5 + 0.5 (a - c)^2 exp(-2 d); kind 1 =
 * kl_loss_normal(m_q = a, ...): d - b - 0.5 + 0.5 (exp(2 b) + (a - c)^2) exp(-2 d).  The reference's score is sum(sums) / rows (its mask sums to
 * B T, not B T C).  ws: rows doubles (rounded up to 256 bytes). */
int stts_val_kl_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, int kind, const float* a, const float* b,
                     const float* c, const float* d, int ld, int C, double* sums, void* ws, size_t ws_bytes);

/* Utterance offsets of a frame-rate call may be CAPACITY SEGMENTS (seg_flags & STTS_SEG_CAPACITY): the host array then holds
 * upper bounds (cumulative capacities - every buffer, workspace and grid is sized by them), the device array the real offsets,
 * which only exist on the device (stts_frame_offsets).  Rows of utterance u are [dev[u], dev[u+1]) - packed, dev[u] <= host[u] -
 * so outputs are packed by the REAL lengths and the caller reads the device offsets once, together with the output.  This is
 * what removes the host round trip between the duration predictor and everything frame-rate (train/test_onnx.py:65-66). */
enum { STTS_SEG_CAPACITY = 1 };

/* The frame-rate hot path in one call: decoder -> prior -> reverse flow -> post_flow -> harmonic source ->
 * STFT -> vocoder -> iSTFT (models/speech_predictor.py:92-118).  This is the benchmarked unit.  seg_flags: 0 or STTS_SEG_CAPACITY. */
int stts_frame_path(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                    const float* asr, int ld_asr, const float* pitch, const float* energy, const float* style,
                    const float* prior_noise, const float* src_noise, const float* init_phase, int batch_scope,
                    float* audio_out, void* ws, size_t ws_bytes, int seg_flags);

/* ---- phoneme-rate predictors.  Sequences are packed: tok_off[n_utt+1] token offsets, tokens int64 [n_tok]. ---- */
/* Workspace the four stages below accept for `n_tokens` tokens and `n_frames` frames in `n_utt` utterances, the longest having
 * `max_tokens` tokens and `max_frames` frames.  Like every stts_*_workspace_bytes query but the CTC one it is a dry run of the
 * stages' own carving, so the finalized components decide it. */
size_t stts_phoneme_workspace_bytes(const stts_ctx* ctx, int64_t n_tokens, int64_t n_frames, int n_utt, int max_tokens, int max_frames);

/* TextEncoder.forward (models/text_encoder.py:433-462).  which: 0 duration_predictor.text_encoder,
 * 1 speech_predictor.text_encoder, 2 pe_text_encoder.  -> mu [n_tok, ld_mu >= inter_dim] (proj_m), optional x [n_tok, 128]. */
int stts_text_encoder_forward(stts_ctx* ctx, void* stream, int which, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                              const int64_t* tokens, float* mu_out, int ld_mu, float* x_out, void* ws, size_t ws_bytes);
/* TextStyleEncoder.forward (models/text_style_encoder.py:20-26; BasicConvNeXtBlock models/conv_next.py:38-51).
 * which as above (0 duration_predictor.style_encoder, 1 speech_predictor.style_encoder, 2 pe_text_style_encoder).
 * x [n_tok, ldx] -> style [n_utt, 64].  Statistics are per utterance over its own tokens (the reference at B = 1). */
int stts_text_style_forward(stts_ctx* ctx, void* stream, int which, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                            const float* x, int ldx, float* style_out, void* ws, size_t ws_bytes);
/* DurationPredictor.forward (models/duration_predictor.py:30-36) -> logits [n_tok, 16]; optional
 * DurationProcessor.prediction_to_duration (train/utils.py:468-474) -> dur int32 [n_tok]; optional taps
 * text_encoder mu [n_tok,128], style [n_utt,64], prosody [n_tok,192]. */
int stts_duration_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                          const int64_t* tokens, float* logits_out, int32_t* dur_out, float* mu_out, float* style_out, float* prosody_out,
                          void* ws, size_t ws_bytes);
/* PitchEnergyPredictor.forward (models/pitch_energy_predictor.py:104-121) incl. compute_cross (:83-102) with the
 * reference's inverted band mask (:194-212 vs models/text_encoder.py:255-262).  The alignment is given as integer
 * durations (train/utils.py:476-489).  pe_enc [n_tok, ld_enc >= 256], pe_style [n_utt,64] -> f0, energy [n_frames]
 * at the mel-frame rate; optional taps prosody [n_tok,320], cross [n_frames,320]. */
int stts_pitch_energy_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* tok_off_host, const int32_t* tok_off_dev,
                              const int32_t* frm_off_host, const int32_t* frm_off_dev, const int32_t* dur, const float* pe_enc, int ld_enc,
                              const float* pe_style, float* f0_out, float* energy_out, float* prosody_out, float* cross_out, void* ws,
                              size_t ws_bytes, int seg_flags /* 0 or STTS_SEG_CAPACITY: applies to the frame offsets */);

/* The host side of DurationProcessor between the two models (train/test_onnx.py:65-66 reads the durations on the host to size the
 * alignment), on the device: from the integer durations of a packed batch, off_T [n_utt+1] = cumulative mel frames per utterance,
 * off_T4 = 4 x (vocoder frames), need [n_utt] = frames of each utterance.  cap_off [n_utt+1] (device): the capacity layout the caller
 * sized its buffers by (mel frames).  An utterance that exceeds its capacity is truncated to it - every later stage stays in
 * bounds, its output is invalid - and need[u] > capacity tells the caller, who reads `need` once together with the output, to repeat
 * the call with capacities >= need (no shared error state: calls may be in flight on several streams).  All pointers are device
 * pointers; nothing synchronises. */
int stts_frame_offsets(stts_ctx* ctx, void* stream, int n_utt, const int32_t* tok_off_dev, const int32_t* dur, const int32_t* cap_off_dev,
                       int32_t* off_T_dev, int32_t* off_T4_dev, int32_t* need_dev);

/* DurationProcessor.prediction_to_duration (train/utils.py:468-474): logits [n_rows, ld >= 16] -> int32 durations. */
int stts_duration_decode(void* stream, const float* logits, int ld, int n_rows, int32_t* dur_out);
/* DurationProcessor.duration_to_alignment (train/utils.py:476-489): durations [P] -> 0/1 matrix [P, T = sum(dur)]. */
int stts_duration_to_alignment(void* stream, const int32_t* dur, int n_tokens, int n_frames, float* alignment_out);

/* Length regulator (train/utils.py:476-489 + models/speech_predictor.py:88-93): integer durations per token ->
 * time-major gather of the phoneme encoding at rate rep (1: mel frames, 4: vocoder frames).
 * dur [n_tok] int32 (device), tok_off [n_utt+1], frm_off [n_utt+1] (= rep * cumulative durations), both device.
 * enc [n_tok, ld_enc] -> out [frames, ld_out] columns [0, C).  Any number of tokens per utterance (the durations are
 * scanned in chunks); limits elsewhere: attention with heads other than 16 / 32 / 40 / 64 / 96 / 128 / 160 channels takes at most 1024 keys per utterance (the
 * reference's own limit is 510 tokens, train/dataloader.py:106-109; those head sizes run on the matrix-core kernel, which streams
 * the keys and has no limit) and stts_duration_to_alignment at most 1024 tokens. */
int stts_length_regulate(stts_ctx* ctx, void* stream, int n_utt, const int32_t* dur, const int32_t* tok_off, const int32_t* frm_off,
                         int64_t n_frames, int rep, const float* enc, int ld_enc, int C, float* out, int ld_out, int32_t* src_row_ws);
/* nn.Upsample(scale_factor=4, mode="linear") of pitch / energy (models/speech_predictor.py:64,89-90). */
int stts_upsample4(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T, const int32_t* off_T4,
                   const float* x, float* y);

/* One explicit-Euler update of the flow-matching sampler, x += dt * v over n floats
 * (models/cfm/cfm.py:65-84, CfmSampler.solve_euler: `x = x + dt * dphi_dt`). */
int stts_euler_step(void* stream, float* x, const float* v, float dt, int64_t n);

/* The estimator of that sampler in the reference: CfmMelDecoder._forward (models/cfm/cfm_mel_decoder.py:318-398; XUT transformer,
 * models/xut/), inference mode.  Its dimensions are constructor keywords in the reference (:190-206), hence this struct.
 * Weights: stts_load_weight(ctx, "cfm_mel_decoder.<state_dict key>", ...) then stts_cfm_finalize.
 * One evaluation on a packed batch: x [rows, ld_x] time-major (feat_dim columns), asr [rows, ld_asr] (ld_asr a multiple of 32, pad
 * columns finite), f0 / n_curve: per-utterance curves back to back with offsets curve_off (resampled to the utterance's frames by
 * F.interpolate's nearest rule, :322-323), spk_emb [n_utt, spk_dim], t [n_utt], sine_noise [rows] = the one RNG draw inside the
 * estimator (SineGenerator's additive noise, :99; the caller draws it), out [rows, ld_out] = dphi/dt.  All tensors on the device.
 * Limits: head_dim 16 / 32 / 40 / 64 (the class default) / 96 / 128 / 160 for utterances beyond 1024 frames - other head sizes keep an utterance's
 * attention scores in LDS (<= 1024 keys); SineGenerator without overtones (the reference's configuration). */
typedef struct stts_cfm_dims {
  int32_t feat_dim, asr_dim, spk_dim, hidden_dim, emb_dim, depth, enc_blocks, dec_blocks, prev_depth, post_depth, head_dim;
} stts_cfm_dims;
int stts_cfm_finalize(stts_ctx* ctx, const stts_cfm_dims* dims);
size_t stts_cfm_workspace_bytes(const stts_ctx* ctx, int64_t rows, int n_utt);
int stts_cfm_estimator(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ld_x,
                       const float* asr, int ld_asr, const float* f0, const float* n_curve, const int32_t* curve_off_host,
                       const int32_t* curve_off_dev, const float* spk_emb, const float* t, const float* sine_noise, float* out, int ld_out,
                       void* workspace, size_t workspace_bytes);

/* ---- AdaptiveHubert, the HuBERT content encoder of the voice-conversion stages (train/models/ssl.py:16-31, called as
 * train.hubert(audio, time_dim), train/stage_type.py:685-688): the transformers HuBERT graph in eval mode with feat_extract_norm "group",
 * do_stable_layer_norm false, conv_bias false and exact GELU, then F.interpolate(mode="nearest", size=time_dim) over the frames.  Its
 * dimensions are the HubertConfig fields, hence this struct (conv lists: the first num_feat_extract_layers entries count).
 * Weights: stts_load_weight(ctx, "hubert.<AdaptiveHubert state_dict key>", ...), i.e. "hubert.model.feature_extractor..." (the positional
 * conv in either weight-norm spelling; masked_spec_embed and final_proj.* are accepted and ignored), then stts_ssl_finalize.
 * wave: packed mono samples at hubert.sr, utterance u = [sample_off[u], sample_off[u + 1]); off_T: the time_dim of every utterance as row
 * offsets of feats [rows_T, ld_feats] (ld_feats a multiple of 4 covering hidden_size padded to 32, pad columns written as zeros) - the
 * layout stts_hubert_encoder_forward / stts_cfm_pitch_forward take.  Every statistic and every attention stays inside the utterance (the
 * reference at B = 1); an utterance's rows are the same bit for bit alone and in any batch.  Always fp32, whatever stts_set_precision chose
 * (dense contractions in the split-fp32 form, on the f32 matrix cores for STTS_PREC_F32_NATIVE; positional conv and attention on the f32 matrix cores).  An utterance shorter than the feature extractor's receptive field (400 samples for HuBERT-base), or a
 * time_dim of 0, is an error status. */
typedef struct stts_ssl_dims {
  int32_t hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, num_feat_extract_layers;
  int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
  int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups;
  float layer_norm_eps;
} stts_ssl_dims;
int stts_ssl_finalize(stts_ctx* ctx, const stts_ssl_dims* dims);
/* frames of the feature extractor for an utterance of `samples` samples (0: too short, the reference raises) */
int64_t stts_ssl_frames(const stts_ssl_dims* dims, int64_t samples);
size_t stts_ssl_workspace_bytes(const stts_ctx* ctx, int n_utt, const int32_t* sample_off_host);
int stts_ssl_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                     const int32_t* off_T_host, const int32_t* off_T_dev, float* feats, int ld_feats, void* ws, size_t ws_bytes);
/* The same, plus intermediate rows for the tests (any may be null).  conv0 [rows0, conv_dim[0]]: layer 0 after GroupNorm + GELU, utterance u's
 * frames from row conv0_off[u] on (conv0_off: device int32 [n_utt + 1]; rows0 = conv0_rows of stts_ssl_tap_rows); the others are packed at
 * the utterances' frame counts: conv_last [frames, conv_dim[-1]], proj [frames, hidden] after the feature projection, pos after positional
 * conv + LayerNorm, layers [num_hidden_layers][frames, hidden], hidden = the last hidden state. */
int stts_ssl_forward_taps(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                          const int32_t* off_T_host, const int32_t* off_T_dev, float* feats, int ld_feats, float* conv0, int32_t* conv0_off,
                          float* conv_last, float* proj, float* pos, float* layers, float* hidden, void* ws, size_t ws_bytes);
/* rows of the conv0 tap buffer of a call (its utterances start at multiples of the later strides' product) */
int64_t stts_ssl_tap_rows(const stts_ssl_dims* dims, int n_utt, const int32_t* sample_off_host);

/* ---- WavLM and the reference's perceptual distance over its hidden states (WavLMLoss, train/losses.py:408-426, logged as "slm"): transformers'
 * WavLMModel in eval mode with feat_extract_norm "group", do_stable_layer_norm false, conv_bias false, exact GELU and heads of 64.  Front end and
 * layer body are AdaptiveHubert's (above); every layer's attention adds gate[query][head] * rel_attn_embed[bucket(key - query)][head] to its scores
 * (the gate from gru_rel_pos_linear / gru_rel_pos_const of the layer's input, the table from layer 0; num_buckets a multiple of 4,
 * num_buckets / 4 < max_bucket_distance <= 2048).  Weights: stts_load_weight(ctx, "wavlm.<WavLMModel state_dict key>", ...) (masked_spec_embed is
 * accepted and ignored), then stts_wavlm_finalize.  fp32 whatever stts_set_precision chose; an utterance's results are the same bit for bit alone
 * and packed with others.  An utterance below the feature extractor's receptive field (400 samples for the base model), or a pair of unequal
 * lengths, is an error status before any launch. */
typedef struct stts_wavlm_dims {
  stts_ssl_dims ssl;
  int32_t num_buckets, max_bucket_distance;
} stts_wavlm_dims;
int stts_wavlm_finalize(stts_ctx* ctx, const stts_wavlm_dims* dims);
/* pairs 0: a stts_wavlm_forward_states call of n_utt utterances; pairs > 0: a stts_wavlm_l1_sums call (n_utt = 2 pairs).  0 on bad arguments. */
size_t stts_wavlm_workspace_bytes(const stts_ctx* ctx, int n_utt, const int32_t* sample_off_host, int pairs);
/* wave: packed mono samples at 16 kHz -> states [num_hidden_layers + 1][frames, hidden_size]: state 0 is the encoder LayerNorm's output, state l + 1
 * layer l's (transformers' hidden_states), rows packed at the utterances' frame counts (stts_ssl_frames).  gate0 (may be null): layer 0's gate
 * [frames, num_attention_heads]. */
int stts_wavlm_forward_states(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave,
                              float* states, float* gate0, void* ws, size_t ws_bytes);
/* 2 * pairs packed waveforms, utterances u and u + pairs of equal length -> sums [pairs][num_hidden_layers + 1] (device doubles): the sum of
 * |state(u) - state(u + pairs)| over the pair's frames and channels, accumulated in double in a fixed order (no atomics; two calls give the same
 * bits), and frames [pairs] (device int32).  No hidden state is kept and nothing is read back by the host. */
int stts_wavlm_l1_sums(stts_ctx* ctx, void* stream, int pairs, const int32_t* sample_off_host, const int32_t* sample_off_dev, const float* wave, double* sums,
                       int32_t* frames, void* ws, size_t ws_bytes);
/* out [2 max_d + 1] (host): the bucket of rel_attn_embed the attention reads at distance d = key - query, for d = -max_d .. max_d (beyond
 * max_bucket_distance the distance is clamped: the buckets have saturated by then) */
int stts_wavlm_bucket_table(const stts_ctx* ctx, int max_d, int32_t* out);

/* ---- RMVPE pitch extractor (train/dataprep/rmvpe/: E2E0 of model.py / deepunet.py / seq.py in eval mode, mel2hidden of inference.py:28-35, the decode
 * of utils.py:114-131, the log-mel of spec.py:39-71, the resampling of dataprep/pitch_extractor.py:136-141).  Weights are loaded under "rmvpe." with the
 * reference's E2E0 state_dict keys; every BatchNorm (eps 1e-5, running statistics) is folded in double.  n_blocks, inter_layers and en_out_channels shape
 * the network; en_de_layers = 5, kernel_size = (2, 2), n_gru = 1 and n_mels = 128 are the only values accepted.  Always fp32 on the f32 matrix cores,
 * whatever stts_set_precision chose.  mel: packed time-major rows [rows_T, ld_mel >= 128] of log-mel frames at 100 frames / s, utterance u = rows
 * [off[u], off[u + 1]), at least 17 frames each (the reflect padding to a multiple of 32 frames needs pad < frames).  Every utterance is padded on
 * its own, the network - both GRU directions included - runs over the padded length, and the outputs are cropped: hidden [rows_T, 360] (the
 * salience, may be null) and f0 [rows_T] in Hz (0 where the frame's largest salience is below thred; may be null).  An utterance's outputs are the
 * same bit for bit alone and in any batch. */
typedef struct stts_rmvpe_dims {
  int32_t n_blocks, inter_layers, en_out_channels; /* 4, 4, 16 */
  int32_t en_de_layers, kernel_h, kernel_w, n_gru, n_mels; /* fixed: 5, 2, 2, 1, 128 */
} stts_rmvpe_dims;
int stts_rmvpe_finalize(stts_ctx* ctx, const stts_rmvpe_dims* dims);
size_t stts_rmvpe_workspace_bytes(const stts_ctx* ctx, int n_utt, const int32_t* off_host);
int stts_rmvpe_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel, float thred,
                       float* hidden_out, float* f0_out, void* ws, size_t ws_bytes);
/* The same, plus intermediate activations for the tests, one after the other in `taps` (stts_rmvpe_tap_floats floats), each over the PADDED frames
 * (utterance u's time rows start at its padded offset >> level) as channels-last rows [time row * F + f][round_up(C, 16)]: the five encoder levels'
 * pooled outputs (level l: F = 64 >> l, C = en_out_channels << l), the intermediate's output (F = 4, C = 32 en_out_channels), the five decoder
 * levels' outputs (level i: F = 8 << i, C = en_out_channels << (4 - i)), cnn [padded frames * 128][4] (3 channels), gru [padded frames][512]. */
int stts_rmvpe_forward_taps(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel,
                            float thred, float* hidden_out, float* f0_out, float* taps, void* ws, size_t ws_bytes);
int64_t stts_rmvpe_tap_floats(const stts_rmvpe_dims* dims, int n_utt, const int32_t* off_host);
/* Log-mel front end: wave = packed mono samples at 16 kHz, utterance u = [sample_off[u], sample_off[u + 1]), more than 512 samples each (reflect
 * padding); STFT n_fft = win = 1024, hop 160, periodic Hann, center = True, samples / 160 + 1 frames (mel_off: their row offsets), magnitude,
 * mel_basis [128, 513] (device) @ magnitude summed over band [128][2] (device int32: first and one-past-last nonzero bin of every filter),
 * log(max(., 1e-5)) -> mel_out [rows, ld_mel >= 128]; mel_lin (optional) [rows, 128]: the mel before the clamp and the log.  Needs STTS_W_RMVPE. */
int stts_rmvpe_mel(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev, const int32_t* mel_off_host,
                   const int32_t* mel_off_dev, const float* wave, const float* mel_basis, const int32_t* band, float* mel_out, int ld_mel, float* mel_lin);
/* to_local_average_f0 of a salience [n_rows, ld >= 360] -> f0 [n_rows] (no weights needed) */
int stts_rmvpe_decode(stts_ctx* ctx, void* stream, int64_t n_rows, const float* salience, int ld, float thred, float* f0_out);
/* The same local average around a GIVEN centre bin per row (center [n_rows] int32 on the device, clamped to [0, 360)); f0 is 0 where the row's
 * largest salience is below thred.  With center = the row's first argmax the result equals stts_rmvpe_decode's bit for bit. */
int stts_rmvpe_decode_at(stts_ctx* ctx, void* stream, int64_t n_rows, const float* salience, int ld, const int32_t* center, float thred, float* f0_out);
/* to_viterbi_f0 (rmvpe/utils.py:134-150): the best path through the 360 classes of every utterance's salience rows [off[u], off[u + 1]) (at least
 * one frame each; no weights needed), one workgroup per utterance, fp64.  Objective: e[t][j] = log(s[t][j] / sum_j s[t][j] + eps), sum, quotient and
 * log in fp64 (a NaN or negative salience counts as 0; a frame whose sum is 0 or not finite gets p = 0 everywhere); v[0][j] = e[0][j] +
 * log(1 / 360 + eps); v[t][j] = e[t][j] + max_i (v[t - 1][i] + lt[i][j]); every argmax takes the lowest index among equals.  lt comes from the
 * caller in band form, fp64 on the device: lt_band[j][k] = lt[j - 29 + k][j] for k < 59 (-inf where that predecessor does not exist), and lt_out =
 * the one value of every lt[i][j] with |i - j| > 29.  A jump across the band is allowed at that cost: a state scans the rest of the row exactly when
 * max_i v[t - 1][i] + lt_out reaches its band maximum, so the result is the optimum of the full 360 x 360 recursion.  Outputs (each may be null,
 * not all): path_out [rows] int32, logp_out [n_utt] fp64 = the path's score, f0_out [rows] = stts_rmvpe_decode_at around the path.  An utterance's
 * outputs are the same bit for bit alone and in any batch.  The stated deviation from the reference: it normalises and takes logs in fp32. */
size_t stts_rmvpe_viterbi_workspace_bytes(int n_utt, const int32_t* off_host);
int stts_rmvpe_viterbi(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* salience, int ld,
                       const double* lt_band, double lt_out, double eps, float thred, int32_t* path_out, double* logp_out, float* f0_out, void* ws,
                       size_t ws_bytes);
/* F.interpolate(mode="linear", align_corners=True) of every utterance's curve from its frames (off_in) to the frames of off_out, on the device */
int stts_rmvpe_resample(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_in_dev, const int32_t* off_out_host, const int32_t* off_out_dev,
                        const float* f0_in, float* f0_out);

/* ---- Text aligner and CTC forced alignment (train/models/text_aligner.py: tdnn_blstm_ctc_model, CTCModel.forward in eval mode;
 * train/dataprep/align_text.py:159-210: torch_align), component STTS_W_ALIGNER with the keys "text_aligner.*".  Always fp32, whatever
 * stts_set_precision chose.  The layer spec: n_tdnn x ("tdnn", tdnn_kernel[i], stride 1, dilation 1) - Conv1d with "same" zero padding, ReLU, then
 * BatchNorm1d(affine=False) in eval mode - followed by one ("ffn", ffn_layers) with its skip add, and encoder_output_layer hidden -> classes
 * (classes = tokens + 1).  A "blstm" entry cannot be built in the reference and has no form here. */
typedef struct stts_aligner_dims {
  int32_t n_mels, hidden, classes; /* 80, 640, 179 for tdnn_blstm_ctc_model_base(80, 178) */
  int32_t n_tdnn, ffn_layers;      /* 3, 5 */
  int32_t tdnn_kernel[4];          /* 5, 3, 3 (odd, at most 7) */
} stts_aligner_dims;
int stts_aligner_finalize(stts_ctx* ctx, const stts_aligner_dims* dims);
size_t stts_aligner_workspace_bytes(const stts_ctx* ctx, int n_utt, const int32_t* off_host);
/* mel_rows [rows, ld_mel >= n_mels]: the normalised log-mel as packed time-major rows with off[n_utt + 1] row offsets (host and device copies of
 * the SAME offsets) -> log_probs [rows, ld_out >= classes] = log_softmax of the output layer.  A segment's convolutions see zeros beyond its own
 * rows (the reference's length mask before every TDNN layer), and an utterance's rows are the same bit for bit alone and in any batch. */
int stts_aligner_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel,
                         float* log_probs, int ld_out, void* ws, size_t ws_bytes);
/* The same, also writing taps (stts_aligner_tap_floats floats): the output of every TDNN layer after its BatchNorm [rows, hidden] each, the Ffn
 * output [rows, hidden], the logits [rows, classes], one after the other. */
int stts_aligner_forward_taps(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* mel_rows, int ld_mel,
                              float* log_probs, int ld_out, float* taps, void* ws, size_t ws_bytes);
int64_t stts_aligner_tap_floats(const stts_aligner_dims* dims, int n_utt, const int32_t* off_host);
/* CTC forced alignment (what the reference takes from its audio library, one utterance at a time on the CPU) and torch_align's post-processing,
 * one workgroup per utterance, no weights.  log_probs [sum T, ld >= classes] with frame offsets t_off, targets [sum P] int32 with token offsets
 * p_off (1 <= P <= 510 per utterance), blank the blank id.  Viterbi over the 2 P + 1 states (blank, token, blank, ..): stay, +1, and +2 only into a
 * token state whose token differs from the token two states back; start in state 0 or 1, end in state 2 P or 2 P - 1.  Ties: the smaller jump
 * wins; at the end the final blank wins.  Outputs: path [sum T] the label of every frame, scores [sum T] = log_probs[t][path[t]], durations
 * [sum P] = frames of token p plus the blank frames that follow it (blank frames in front of the first token count to token 0: the reference's loop
 * trips its own assert on such a path), left / right [sum P]: torch_align's boundary probabilities, 0 in the last entry.  path_given != 0: path is
 * an INPUT and only the post-processing runs (no workspace needed).  A (T, targets) pair with fewer frames than tokens plus adjacent equal pairs
 * has no valid path: the outputs are then meaningless, every access still in bounds (the Python shim refuses such input). */
size_t stts_ctc_align_workspace_bytes(int n_utt, const int32_t* t_off_host, const int32_t* p_off_host);
int stts_ctc_align(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const int32_t* p_off_host, const int32_t* p_off_dev,
                   const float* log_probs, int ld, int classes, int blank, const int32_t* targets, int path_given, int32_t* path, float* scores,
                   int32_t* durations, float* left, float* right, void* ws, size_t ws_bytes);
/* The CTC negative log-likelihood (what the reference takes from k2.ctc_loss, here the exact sum over ALL paths, unpruned): the same states and
 * jumps as stts_ctc_align over the log semiring, in fp64 from the fp32 log_probs; nll [n_utt] (fp64) = -log of the summed path probabilities, +inf
 * (never NaN) where (T, targets) has no path.  log_priors (null, or [classes] fp64): every emission becomes log_probs[t][c] - prior_scale *
 * log_priors[c] (CTCLossWithLabelPriors' "train" branch) without a second log-prob tensor.  Same refusals as stts_ctc_align; no workspace; an
 * utterance's value does not depend on the batch around it. */
int stts_ctc_nll(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const int32_t* p_off_host, const int32_t* p_off_dev,
                 const float* log_probs, int ld, int classes, int blank, const int32_t* targets, const double* log_priors, double prior_scale, double* nll);
/* sums [n_utt] (fp64) = each utterance's sum of exp(scores[t]) over the path log-probs stts_ctc_align writes, added in a fixed order, no atomics
 * (validate_alignment's "confidence" = sum of the sums / frames; align_text's per-file score = sums[u] / T_u). */
int stts_ctc_confidence_sums(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const float* scores, double* sums);
/* log_sums [classes] (fp64) = logsumexp over every frame of the batch of log_probs[t][c] (CTCLossWithLabelPriors' log_batch_priors_sum,
 * train/losses.py:563-580): (max, sum) partials of 64-row chunks in ws, merged in chunk order; an all -inf column gives -inf. */
size_t stts_ctc_prior_sums_workspace_bytes(int n_utt, const int32_t* t_off_host, int classes);
int stts_ctc_prior_sums(void* stream, int n_utt, const int32_t* t_off_host, const int32_t* t_off_dev, const float* log_probs, int ld, int classes,
                        double* log_sums, void* ws, size_t ws_bytes);

/* ---- HuBERT voice conversion (the reference's hubert_acoustic models, train/stage_type.py:907-1015).  Inputs are HuBERT features at the
 * mel-frame rate as packed time-major rows feats [rows_T, ld_feats] (ld_feats a multiple of 4 covering hubert.hidden_dim padded to 32, pad
 * columns finite) with off_T[n_utt+1] row offsets, and wespeaker embeddings spk_emb [n_utt, ld >= speaker_embedder.hidden_dim].  The HuBERT
 * and speaker widths are taken from the weights (phone_emb / phone_quant, style_encoder.0).  Statistics are per utterance over its own
 * frames (the reference at B = 1).  These stages always run fp32, whatever stts_set_precision chose; the frame path that follows
 * (stts_frame_path, on the hubert_speech_predictor's decoder .. generator weights loaded under "speech_predictor.") follows it. */
size_t stts_hubert_workspace_bytes(const stts_ctx* ctx, int64_t rows_T, int n_utt, int max_len);
/* Speaker styles: hubert_speech_predictor.style_encoder (Linear -> Mish -> Linear -> Mish -> Linear, models/speech_predictor.py:137-147,
 * dropout = identity) -> style_out [n_utt, 64], and hubert_pitch_energy_predictor.style_encoder (one Linear, models/pitch_energy_predictor.py:139)
 * -> pe_style_out [n_utt, 64].  Either output may be null (its component need not be finalized).  An utterance's rows are the same bit
 * for bit alone and in any batch (fixed-order split-K sums, no atomics). */
int stts_speaker_style(stts_ctx* ctx, void* stream, int n_utt, const float* spk_emb, int ld, float* style_out, float* pe_style_out, void* ws,
                       size_t ws_bytes);
/* HubertEncoder.forward with input_cond_dim=None (models/hubert_encoder.py:36-47, called at models/speech_predictor.py:211-213):
 * phone_emb (1x1) at T rows, repeat_interleave(4) (the two commute), the transformer Encoder (models/text_encoder.py:332-393) at 4T rows
 * masked by 4 x lengths.  feats (offsets off_T) -> asr_out [4 rows_T, ld_asr >= inter_dim] = the decoder input of stts_frame_path
 * (offsets 4 x off_T).  Heads of 16 / 32 / 40 / 64 / 96 / 128 / 160 channels take any length; others at most 1024 positions (4T). */
int stts_hubert_encoder_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* feats,
                                int ld_feats, float* asr_out, int ld_asr, void* ws, size_t ws_bytes);
/* HubertPitchEnergyPredictor.forward (models/pitch_energy_predictor.py:176-191): phone_quant (1x1), ProsodyEncoder (3 layers), two chains of
 * 3 AdaptiveDecoderBlocks + 1x1 projections.  feats, pe_style [n_utt, 64] (stts_speaker_style) -> f0_out, energy_out [rows_T]; optional
 * prosody_tap [rows_T, inter_dim + style_dim]. */
int stts_hubert_pitch_energy_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* feats,
                                     int ld_feats, const float* pe_style, float* f0_out, float* energy_out, float* prosody_tap, void* ws,
                                     size_t ws_bytes);

/* ---- MelStyleEncoder (models/mel_style_encoder.py:120-151): mel -> style vector, as pe_mel_style_encoder (which = STTS_W_PE_MEL_STYLE,
 * models/models.py:57-62) or as cfm_pitch_predictor.spk_emb (which = STTS_W_CFM_PITCH, models/cfm/cfm_pitch_predictor.py:25-27).
 * Input: the normalised mel as packed time-major rows mel [rows_T, ld >= n_mels] with seg_off[n_utt+1] row offsets; output
 * style_out [n_utt, style_dim].  Dims come from the weights (shared.0 gives n_mels; n_mels must be a multiple of 2^downsamplings with at least
 * 5 rows after them, 40 for the model.yml encoders); spectral norm is folded at finalize from the stored weight_u / weight_v (eval mode).
 * An utterance shorter than the 5 x 5 conv allows (33 mel frames with three downsamplings) is an error, as the reference fails there.
 * seg_off_host and seg_off_dev must hold the SAME offsets (no STTS_SEG_CAPACITY upper bounds): buffers, grids and the length check are
 * planned from the host copy, the kernels index with the device copy.
 * Each utterance is the reference at B = 1, the same bits alone and in any batch.  Always fp32 (the f32 matrix cores), whatever
 * stts_set_precision chose: the 16-bit modes give the same bits as f32. */
size_t stts_mel_style_workspace_bytes(stts_ctx* ctx, int which, int64_t rows_T, int n_utt);
int stts_mel_style_forward(stts_ctx* ctx, void* stream, int which, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* mel,
                           int ld, float* style_out, void* ws, size_t ws_bytes);
/* The same, also writing the four ResBlk outputs to block_taps one after the other, each [rows of its level][round_up(cout, 16)]
 * channels-last (row (off_l[u] + t) * F_l + f, F_l = n_mels / 2^l, off_l the per-level time offsets, T halved rounding up). */
int stts_mel_style_forward_taps(stts_ctx* ctx, void* stream, int which, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                                const float* mel, int ld, float* style_out, float* block_taps, void* ws, size_t ws_bytes);

/* ---- CfmPitchPredictor's frame-rate network (models/cfm/cfm_pitch_predictor.py:12-51), component STTS_W_CFM_PITCH_NET: asr_emb (1x1,
 * Mish, 1x1), four generator ConvNeXt blocks (256 / 1024 channels, k = 7) conditioned on the speaker style, out_proj (256 -> 1).
 * Input: asr features as packed time-major rows asr [rows_T, ld_asr >= asr_dim, ld_asr % 4 == 0] with off_T[n_utt+1] row offsets (the
 * pitch-frame rate), and spk_style [n_utt, 256] = stts_mel_style_forward(STTS_W_CFM_PITCH) of the reference mel (any stream).
 * Output: out_normed [rows_T] (the normed F0, packed by the real lengths).  out_hz (or null) [rows_T] = denorm_f0_zscore of it
 * (train/stage_type.py:801-829): clamp(2^(x * f0_log2_std + f0_log2_mean), 50, 1200), 0 where uv[row] > 0 (uv [rows_T] or null).
 * The log2 statistics are the training set's (not in the checkpoint).  GRN's norm runs over each utterance's own rows: every utterance
 * is the reference at B = 1.  off_T_host / off_T_dev must hold the same offsets.  Always fp32, whatever stts_set_precision chose. */
size_t stts_cfm_pitch_workspace_bytes(stts_ctx* ctx, int64_t rows_T, int n_utt);
int stts_cfm_pitch_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* asr, int ld_asr,
                           const float* spk_style, float* out_normed, float* out_hz, float f0_log2_mean, float f0_log2_std, const float* uv, void* ws,
                           size_t ws_bytes);
/* The same, also writing taps [5][rows_T][256]: the asr_emb output, then the output of each ConvNeXt block. */
int stts_cfm_pitch_forward_taps(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_T_host, const int32_t* off_T_dev, const float* asr, int ld_asr,
                                const float* spk_style, float* out_normed, float* out_hz, float f0_log2_mean, float f0_log2_std, const float* uv,
                                float* taps, void* ws, size_t ws_bytes);

/* ---- Log-mel front end of a recording: torchaudio.transforms.MelSpectrogram(n_mels, n_fft, win_length, hop_length, sample_rate) at its defaults
 * (power 2, torch.stft center=True / pad_mode="reflect", periodic Hann(win_length) centred in the frame, HTK mel scale, f_min 0,
 * f_max sample_rate / 2, norm None) followed by the reference's own arithmetic:
 *   mel_rows = (log(1e-5 + mel) - mean) / std    calculate_mel (train/stage_type.py:1023-1032), preprocess (train/dataprep/align_text.py:112-117)
 *   energy   = sum_m (1e-5 + mel)^0.33           log_norm of that normalised mel (train/utils.py:71-77; the mean / std cancel)
 *   raw_rows = log(1e-5 + mel)                   what compute_log_mel_stats averages (train/utils.py:80-148)
 * wave: packed mono audio at sample_rate, utterance u = samples [sample_off[u], sample_off[u+1]), more than n_fft / 2 of them (torch.stft refuses
 * less); it gets row_off[u+1] - row_off[u] frames, between 1 and samples / hop_length + 1: frame f is centred on sample hop_length * f of the
 * utterance's own reflect-padded signal.  The caller resolves the frame policy into row_off (calculate_mel: samples / hop + 1 rounded down
 * to even; preprocess: samples / hop; all: samples / hop + 1).  mel_rows / raw_rows: time-major [rows, ld >= n_mels] (columns >= n_mels are not
 * written) - the layout stts_mel_style_forward and stts_aligner_forward read; energy [rows].  Each of the three may be null, not all.
 * n_fft a power of two in [256, 4096], 1 <= win_length <= n_fft, hop_length >= 1, 1 <= n_mels <= 256.  The transform, the mel sums, the log and the
 * normalisation run in fp64 and round once to fp32.  The tables of (n_fft, win_length, n_mels, sample_rate) are built on first use and kept in
 * the context.  Every frame's results are independent of the batch around it.  *_host / *_dev must hold the same offsets. */
int stts_log_mel_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev,
                         const int32_t* row_off_host, const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length, int n_mels,
                         int sample_rate, double mean, double std, float* mel_rows, int ld, float* energy, float* raw_rows);
/* compute_log_mel_stats (train/utils.py:80-148) over the same packed batch with ALL samples / hop_length + 1 frames of every utterance:
 * partials [rows][2] (fp64) = each frame's sum of log(1e-5 + mel) and of its square over the mel axis; stats [3] (fp64, device) = mean, std
 * (unbiased variance, clamped at 1e-12) and the value count rows * n_mels, reduced from the partials in a fixed order: bit-identical from run to run. */
int stts_log_mel_stats(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev,
                       const int32_t* row_off_host, const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length, int n_mels,
                       int sample_rate, double* partials, double* stats);
/* The mel filters stts_log_mel_forward uses (torchaudio.functional.melscale_fbanks(n_fft / 2 + 1, 0, sample_rate // 2, n_mels, sample_rate,
 * norm=None, mel_scale="htk"), built in float64 and rounded once to fp32), on the host: weights [n_mels][n_fft / 2 + 1], band [n_mels][2] = the
 * nonzero bins [first, one past the last) of every filter (0, 0: an empty filter).  No context, no GPU. */
int stts_log_mel_filters(int n_fft, int n_mels, int sample_rate, int32_t* band, float* weights);

/* ---- Validation scores: what every validate_* of the reference logs about its audio (train/stage_type.py).  MultiSpectrogram
 * (train/multi_spectrogram.py) per resolution (n_fft, hop_length, win_length):
 *   X = torch.stft(audio, n_fft, hop_length, win_length, periodic Hann(win_length)) (center=True / reflect, one-sided, unnormalised)
 *   fft_mag = |X|      phase = (fft_mag > 1e-3) * angle(X)      mag = log1p(MelScale(n_mels, sample_rate, n_fft / 2 + 1)(fft_mag))
 * with MelScale at torchaudio's defaults: the filters of stts_log_mel_filters.  wave: packed mono audio, utterance u = samples
 * [sample_off[u], sample_off[u+1]), more than n_fft / 2 of them; it has ALL of its samples / hop_length + 1 frames, rows [row_off[u], row_off[u+1]).
 * Geometry rules: those of stts_log_mel_forward.  One wave per frame, everything in fp64 (window product, transform, sqrt(re^2 + im^2), mel sums
 * in bin order, log1p, atan2); sums are added in fixed orders without atomics: every result is bit-identical from run to run and independent of the
 * batch around its utterance.  The caller owns every buffer (stts_val_sizes has the sizes); nothing is allocated per call.  The tables of a
 * geometry are built on first use and kept in the context.  *_host / *_dev must hold the same offsets. */
/* Host only (no context, no GPU): sizes[0] = rows = sum of samples / hop_length + 1, sizes[1] = doubles of stts_val_mel_sums' partials (2 rows),
 * sizes[2] = doubles of stts_val_magphase_sums' partials (4 rows), sizes[3] = doubles of its scratch (rows * (n_fft / 2 + 1)).  A nonzero status
 * names the rule or the utterance too short for the reflect padding. */
int stts_val_sizes(int n_utt, const int32_t* sample_off_host, int n_fft, int hop_length, int64_t* sizes);
/* MultiSpectrogram.calculate_single as time-major rows: mag_rows [rows, ld_mag >= n_mels], fft_mag_rows and phase_rows [rows, ld_bins >= n_fft / 2 + 1];
 * each value is rounded once from fp64 to fp32, columns beyond the width are not written.  Each of the three may be null, not all; an output's
 * bits do not depend on which others are asked for. */
int stts_multi_spectrogram_forward(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev,
                                   const int32_t* row_off_host, const int32_t* row_off_dev, const float* wave, int n_fft, int win_length, int hop_length,
                                   int n_mels, int sample_rate, float* mag_rows, int ld_mag, float* fft_mag_rows, float* phase_rows, int ld_bins);
/* The sums of MultiResolutionSTFTLoss.spectral_convergence_loss (train/losses.py:24-25) at one resolution, without writing a spectrogram: one
 * launch transforms frame f of the target and of the prediction in the same wave; partials [rows][2] (fp64) = (sum_m |t - p|, sum_m |t|) of the
 * frame's log1p mel values, sums [n_utt][2] (fp64) = each utterance's partials added in a fixed order.  target / pred: packed alike; an utterance
 * whose sample counts differ (sample_off_host against pred_off_host) gives a nonzero status naming it.  An identical pair gives a numerator of
 * exactly 0.  The reference's number over an equal-length batch is sum_u sums[u][0] / (sum_u sums[u][1] + 1e-6), averaged over the resolutions. */
int stts_val_mel_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* pred_off_host, const int32_t* sample_off_dev,
                      const int32_t* row_off_host, const int32_t* row_off_dev, const float* target, const float* pred, int n_fft, int win_length,
                      int hop_length, int n_mels, int sample_rate, double* partials, double* sums);
/* The sums of MagPhaseLoss.forward (train/losses.py:85-154).  gt: the packed recordings; hop_length: the hop of the transform (the reference's
 * hop_length // 4); logamp_rows / phase_rows: the prediction's log-magnitude and phase as time-major rows [rows, ld >= n_fft / 2 + 1], utterance u
 * with exactly samples / hop_length + 1 rows (a nonzero status names an utterance with another count).  With Y the transform of gt,
 * target_mag = |Y| + 1e-14, on = target_mag > 1e-3, tp = on * angle(Y), pp = on * phase_rows (the input is NOT modified),
 * aw(d) = |d - 2 pi round(d / 2 pi)|, w_k = base^k, base = exp(ln 2.5 / ((n_fft / 2 + 1) / 2)):
 *   sums[u][0] = sum |logamp - log(target_mag + 1e-9)|                                      "mag" = its mean
 *   sums[u][1] = sum w_k aw(pp - tp)
 *   sums[u][2] = sum w_k aw((pp[k-1] - pp[k]) - (tp[k-1] - tp[k])), bin -1 = 0
 *   sums[u][3] = sum w_k aw((pp[f-1] - pp[f]) - (tp[f-1] - tp[f])), frame -1 = 0            "phase" = the sum of the three means
 * partials [rows][4] and sums [n_utt][4] in fp64; scratch [rows][n_fft / 2 + 1] fp64 holds the masked target phase between the two launches. */
int stts_val_magphase_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* sample_off_host, const int32_t* sample_off_dev,
                           const int32_t* row_off_host, const int32_t* row_off_dev, const float* gt, const float* logamp_rows, const float* phase_rows, int ld,
                           int n_fft, int win_length, int hop_length, double* scratch, double* partials, double* sums);
/* sums [n_utt] (fp64) = each utterance's sum of smooth_l1(a - b) at beta 1 (0.5 d^2 below |d| = 1, |d| - 0.5 from there on) over the packed fp32
 * vectors a and b, utterance u = values [off[u], off[u+1]), at least one; added in a fixed order. */
int stts_val_smooth_l1_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b,
                            double* sums);
/* The same for l1_loss / mse_loss: sums [n_utt] (fp64) = each utterance's sum of |a - b| (kind 0) or (a - b)^2 (kind 1). */
int stts_val_diff_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b, int kind,
                       double* sums);
/* The sums of DurationLoss / CDW_CCELoss (train/losses.py:429-476, alpha = 2) over packed token rows logits [sum P, ld >= classes] (fp32),
 * 2 <= classes <= 64, targets [sum P] int32 classes (clamped to [0, classes - 1]), weight [classes] fp32.  With sm / lsm the row's softmax and
 * log-softmax in fp64, t = the row's target and d[t][c] = min(|t - c|, 7)^2, sums [n_utt][3] (fp64) =
 *   sum_p lsm[p][t] * w[t],   sum_p w[t],   sum_p sum_c log(1 - sm[p][c] + 1e-9) * (d[t][c] / sum_c d[t][c])
 * added in a fixed order.  The reference's numbers: duration_ce = mean_u -s0 / (s1 + 1e-9), duration = mean_u -100 * s2 / P_u. */
int stts_val_duration_sums(stts_ctx* ctx, void* stream, int n_utt, const int32_t* p_off_host, const int32_t* p_off_dev, const float* logits, int ld,
                           int classes, const int32_t* targets, const float* weight, double* sums);

/* ---- Windowed-sinc sample-rate conversion: torchaudio.transforms.Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff,
 * beta) / functional.resample from their published definition, with the float64 result as the target:
 *   o, n = orig_freq, new_freq over their gcd;  base = min(o, n) * rolloff;  width = ceil(lowpass_filter_width * o / base);  taps = 2 width + o
 *   coefficient[p][j] = sinc(pi t) * window(t) * base / o,  t = clamp((-p / n + j / o) * base, -lpw, lpw),  p in [0, n), j in [-width, width + o)
 *   window: method 0 = sinc_interp_hann, cos(pi t / (2 lpw))^2;  method 1 = sinc_interp_kaiser, I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)
 *   output q n + p of an utterance = sum_j coefficient[p][j] * sample[q o + j], samples outside the utterance zero;  ceil(n samples / o) outputs
 * The coefficients are built on the device in fp64 and kept unrounded (torchaudio rounds them, and p / n, to fp32: not mirrored); products and the sum
 * are fp64, the taps are added in tap order and the sum is rounded once to fp32.  Every output is independent of the batch around its utterance.
 * Limits (a nonzero status names the number): o, n <= 1024, n * taps <= 2^20, 1 <= lowpass_filter_width <= 256, 0 < rolloff <= 1, 0 <= beta <= 512,
 * every utterance at least 1 sample.  Equal rates copy the input. */
/* Host arithmetic only (no context, no GPU): the reduced rates, width and taps; any out pointer may be null. */
int stts_resample_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int* o, int* n, int* width, int* taps);
/* ceil(new_freq * samples / orig_freq) on the reduced rates; -1 for a negative count or a rate below 1.  Host only. */
int64_t stts_resample_out_length(int64_t samples, int orig_freq, int new_freq);
/* Consecutive outputs of an utterance that one row of blocks of the resampling kernel computes at these rates (what tests place their lengths
 * around); -1 for rates out of range.  Host only. */
int stts_resample_tile(int orig_freq, int new_freq);
/* in: packed mono audio at orig_freq, utterance u = samples [off_in[u], off_in[u+1]); out: packed, utterance u = [off_out[u], off_out[u+1]), which must
 * hold exactly stts_resample_out_length of its input count.  beta is read under method 1 only.  The table of (o, n, lowpass_filter_width, rolloff,
 * method, beta) is built on first use (that call waits for it) and kept in the context.  *_host / *_dev must hold the same offsets. */
int stts_resample_forward(stts_ctx* ctx, void* stream, int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int method, double beta,
                          int n_utt, const int32_t* off_in_host, const int32_t* off_in_dev, const int32_t* off_out_host, const int32_t* off_out_dev,
                          const float* in, float* out);

/* Layout bridge for the nn.Module shims: reference [B, C, T] (equal T) <-> time-major rows. */
int stts_to_time_major(void* stream, const float* x_bct, int B, int C, int T, float* y, int ldy);
int stts_to_channel_major(void* stream, const float* x, int ldx, int B, int C, int T, float* y_bct);

/* STFT.transform / STFT.inverse of models/stft.py:98-187: the conv1d / conv_transpose1d DFT-matrix STFT that the
 * reference's ONNX export swaps into the generator (train/convert_to_onnx.py:31-36).  Not torch.stft: replicate padding, the
 * Hann window at the start of the frame, magnitude sqrt(re^2 + im^2 + 1e-14) with re/mag and im/mag as outputs; the inverse
 * sums the bins one-sided, scales by 1/n_fft and overlap-adds without window-envelope normalisation.  n_fft 2048 / window
 * 1200 (model.yml), any hop.  Utterance u: F_u = frame_off[u+1] - frame_off[u] >= 2 frames <-> (F_u - 1) * hop samples,
 * packed at sample offset hop * (frame_off[u] - u).  mag / x / y: time-major [frames, ld >= 1025] (pad columns zeroed by
 * the transform).  The inverse needs frames * 1200 floats of workspace.
 * (With the export's own arguments - hop 300 against the generator's hop 75 - the reference's generator raises at
 * models/generator.py:414, tests/golden/onnx_stft_wiring_evidence.json, so these are pinned as a standalone module.) */
int stts_conv_stft_transform(stts_ctx* ctx, void* stream, int n_utt, const int32_t* frame_off_host, const int32_t* frame_off_dev,
                             const float* wave, int hop, float* mag, float* x, float* y, int ld);
int stts_conv_stft_inverse(stts_ctx* ctx, void* stream, int n_utt, const int32_t* frame_off_host, const int32_t* frame_off_dev,
                           const float* mag, const float* x, const float* y, int ld, int hop, float* wave_out, void* ws, size_t ws_bytes);

/* Measurement hook (bench.py roofline leg): between begin and end every conv_gemm_f32 / wn_layer_kernel launch carries a
 * HIP start/stop event pair on its own stream.  end() synchronises and returns the launch count, the summed kernel time and
 * the summed ALGORITHMIC flops (2 * rows * cout * cin * taps, un-padded sizes). */
int stts_profile_begin(void);
int stts_profile_end(void* stream, int* launches, double* total_ms, double* total_flops);
/* The same measurement per kernel, for every launch of the frame path (the bandwidth-bound kernels included): a JSON array
 * [{"kernel", "kind": "contraction"|"other", "launches", "ms", "gflop" (algorithmic), "executed_gflop" (what the matrix
 * cores execute: less for the Winograd forms), "mbytes" (algorithmic HBM bytes)}] summed over the launches
 * since stts_profile_begin.  Ends the measurement like stts_profile_end. */
int stts_profile_report(void* stream, char* json, size_t json_capacity);

/* AdaptiveGeneratorBlock.forward (HiFi-GAN MRF + Snake, models/ada_norm.py:109-120); standalone block only: the enclosing
 * UpsampleGenerator cannot be instantiated in the reference. */
int stts_op_mrf_block(stts_ctx* ctx, void* stream, const char* prefix, int n_utt, const int32_t* seg_off_host,
                      const int32_t* seg_off_dev, const float* x, int ldx, int channels, int kernel, const float* style, float* y,
                      int ldy, void* ws, size_t ws_bytes);

#ifdef STTS_TEST_OPS
/* Test surface, only in a library built with -DSTTS_TEST_OPS (tests/ and tools/; not part of the product ABI).
 * Single operators for parity tests (the same kernels the stages use): */
/* F.conv1d(stride 1, zero pad (k-1)/2*dil) on time-major rows; w is the reference layout [cout, cin, k] on the HOST. */
int stts_op_conv1d(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ldx, int cin,
                   const float* w_host, const float* bias_host, int cout, int k, int dil, int act, float* y, int ldy, int force_tile, int precision);
/* The fp32 contraction variants stts_op_conv1d does not reach (precision STTS_PREC_F32 or _F32_NATIVE, no activation):
 * F.conv1d over the channel concatenation [x, x2] (w [cout, cin + cin2, k]; x2 may be null) as two segments of one launch;
 * an input affine of x staged with the tile, x' = lrelu_slope(x * scale + shift) with aff_host [n_utt][2][ldx] (scale 0: pad column;
 * xaff_mode 1 = scale / shift, 2 = the scale-only form: shift 0, slope 1, cin == ldx, no x2; 0 = none, aff_host null);
 * presplit 1: the activations are split into the three bf16 planes of the split-fp32 form before the contraction (tiles 25 - 28). */
int stts_op_conv1d_x3(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ldx, int cin,
                      const float* x2, int ldx2, int cin2, const float* w_host, const float* bias_host, int cout, int k, int dil, const float* aff_host,
                      int xaff_mode, float slope, int presplit, float* y, int ldy, int force_tile, int precision);
/* The store contraction of the 16-bit operand modes with its WHOLE epilogue (tests/test_hip_gemm16_epilogues.py):
 *   v = (act(sum_i conv1d(x_i, w_i) + bias) + R) * alpha  ->  Y (fp32), Y16 (v rounded to the mode), GRN sums of squares, AdaIN statistics.
 * One or two K segments, each with its own fp32 rows x_i [rows, ldx_i] (rounded to the mode by the operator; pad columns cin_i .. ldx_i
 * may hold any finite values), host weight [cout, cin_i, k_i] (k_i odd), dilation; the packed weights have cin_i padded to 64 and cout to 256,
 * so force_tile 19 (conv_gemm16_kernel) is eligible for any cin; other tiles: conv_gemm_f32 on 16-bit rows (5, 6, 14 - 18).
 * Every output is optional (null) and caller-owned; *_elems is the element count of the caller's buffer: a launch that could reach
 * beyond one of them is refused.  sumsq [utt * ss_stride + 32-row slot][ld_ss]; stat [((utt * stat_nchunk + 128-row chunk) * 2 + {mean, M2})][ld_stat]
 * (tile 19 only).  tune: 0 or 0x4000 (conv_gemm16_kernel's generic store body).  capacity 1: seg_off_host are cumulative capacities,
 * seg_off_dev the real offsets (STTS_SEG_CAPACITY).  precision: STTS_PREC_BF16 or _F16. */
typedef struct stts_conv_epi_seg {
  const float* x;
  const float* w_host;
  int64_t x_elems;
  int32_t ldx, cin, k, dil;
} stts_conv_epi_seg;
typedef struct stts_conv_epi_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  stts_conv_epi_seg seg[2];
  const float* bias_host;
  const float* r;
  float* y;
  uint16_t* y16;
  float* sumsq;
  float* stat;
  int64_t r_elems, y_elems, y16_elems, sumsq_elems, stat_elems;
  int32_t n_utt, capacity, nseg, cout, act;
  float alpha;
  int32_t ldr, rcol0, ldy, ycol0, ldy16, ycol16, ld_ss, ss_stride, ld_stat, stat_nchunk;
  int32_t force_tile, tune, precision;
} stts_conv_epi_args;
int stts_op_conv1d_epi(void* stream, const stts_conv_epi_args* args);
/* The kernels BETWEEN the contractions, one at a time (tests/test_hip_norm_kernels.py).  Like stts_op_conv1d_epi: one args struct per operator, every
 * tensor caller-owned and on the device unless named *_host, *_elems the element count of the caller's buffer; a launch that could reach beyond one of
 * them, or a shape outside a kernel's stated domain, is refused before anything is launched.  Host and device offsets must agree (no capacity form).
 *
 * stts_op_adain: chunk statistics -> merge -> apply of AdaIN (models/ada_norm.py:129-139), each step selectable.
 *   producer 0: adain_partial_kernel, chunks of 128 rows; 1: the same kernel, chunks of 24 rows (the Winograd statistics' chunking);
 *            2: adain_partial_reduce_kernel: x (channels < split_n) is FINISHED here from ksplit partial slices [ksplit][slice_rows][ld_part] as
 *               (act(sum_k + bias) [+ r]) * alpha and written, the statistics come from the values in flight (chunks of 128 rows).
 *   consumer 0: none; 1: adain_affine_kernel (serial merge); 2: adain_affine_lanes_kernel (16 lanes) -> aff [n_utt][2][ld_aff];
 *            3: adain_apply_kernel through run_adain on the table the producer left (producer 0 or 2; ldp == round_up(C, 32), nchunk ==
 *               ceil(max_len / 128)) -> y [rows, ldy] (out16: 0 fp32, STTS_PREC_BF16 / _F16: 16-bit elements), rb 64 or 256, act, snake (null: none).
 *   part [((u * nchunk + chunk) * 2 + {mean, M2})][ldp]; gb [n_utt][ld_gb]: gamma at gcol0 + c, beta at gcol0 + C + c. */
typedef struct stts_adain_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  float* x;
  float* part;
  const float* partial;
  const float* bias;
  const float* r;
  const float* gb;
  const float* snake;
  float* aff;
  void* y;
  int64_t x_elems, part_elems, partial_elems, bias_elems, r_elems, gb_elems, snake_elems, aff_elems, y_elems;
  int32_t n_utt, producer, consumer, C, ldx, ldp, nchunk;
  int32_t ksplit, slice_rows, ld_part, split_n, split_act, ldr, rcol0;
  float split_alpha;
  int32_t ld_gb, gcol0, ld_aff, ldy, rb, act, out16;
} stts_adain_args;
int stts_op_adain(void* stream, const stts_adain_args* args);
/* F.conv1d (k 3 or 7, dilation 1) in Winograd form as stts_op_conv1d's force_tile -4, with the AdaIN statistics winograd_output_kernel<N, true> leaves
 * next to Y: stat [((u * stat_nchunk + 24-row chunk) * 2 + {mean, M2})][ld_stat], stat_nchunk == ceil(ceil(max_len / 6) / 4).  x, y, stat on the device. */
typedef struct stts_wino_stat_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* x;
  const float* w_host;
  const float* bias_host;
  float* y;
  float* stat;
  int64_t x_elems, y_elems, stat_elems;
  int32_t n_utt, ldx, cin, cout, k, act, ldy, ld_stat, stat_nchunk, precision;
} stts_wino_stat_args;
int stts_op_wino_stat(void* stream, const stts_wino_stat_args* args);
/* row_layernorm_kernel through ln_launch: LayerNorm over C channels (C % 4 == 0, C <= 2048) of n_rows rows, one or two outputs.
 * static: out.g / out.b = gamma / beta [C]; adaptive: out.g = style table [n_utt][ld_g], gamma at gcol0 + c, beta at gcol0 + C + c (the offsets are then
 * needed and must sum to n_rows).  partial != null: the row is finished from ksplit split-K slices [ksplit][slice_rows][ld_part] as
 * (act(sum_k + bias) [+ r]) * alpha (LnIn), x is not read.  n_rows_real >= 0: passed as the device-side row count (rows from there on are skipped). */
typedef struct stts_ln_out {
  void* y;
  const float* g;
  const float* b;
  int64_t y_elems, g_elems, b_elems;
  int32_t ldy, ycol0, ld_g, gcol0, prec16;
} stts_ln_out;
typedef struct stts_row_layernorm_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* x;
  const float* partial;
  const float* bias;
  const float* r;
  int64_t x_elems, partial_elems, bias_elems, r_elems;
  stts_ln_out out[2];
  int32_t n_utt, n_rows, n_rows_real, C, ldx, adaptive, nout, act;
  float eps;
  int32_t ksplit, slice_rows, ld_part, in_act, ldr, rcol0;
  float in_alpha;
} stts_row_layernorm_args;
int stts_op_row_layernorm(void* stream, const stts_row_layernorm_args* args);
/* Depthwise Conv1d along time, zero padding inside the utterance (w_host [C][K] = the reference's [C, 1, K], bias_host [C]; C % 4 == 0).
 *   form 0: dwconv_kernel<31> (K odd, <= 31) with act -> y fp32;
 *   form 1: dwconv_ln_kernel<K, 16>: + adaptive LayerNorm (eps 1e-6), C <= 512, K in {3, 7, 15, 31} - the dispatch of convnext_block_forward;
 *   form 2: form 0 into a scratch, then row_layernorm_kernel: that function's fallback.
 * forms 1, 2: style [n_utt][ld_style], gamma at gcol0 + c, beta at gcol0 + C + c; y fp32 or (prec16) 16-bit elements. */
typedef struct stts_dwconv_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* x;
  const float* w_host;
  const float* bias_host;
  const float* style;
  void* y;
  int64_t x_elems, style_elems, y_elems;
  int32_t n_utt, form, C, K, act, ldx, ldy, ld_style, gcol0, prec16;
} stts_dwconv_args;
int stts_op_dwconv(void* stream, const stts_dwconv_args* args);
/* GRN (models/generator.py:496-499) from a caller-supplied table of per-32-row-slot sums of squares part [n_utt][ss_stride][ld_ss]:
 * grn_gx_kernel -> gx [n_utt][ld_gx], then mode 0: nothing; 1: grn_xaff_kernel -> xaff [n_utt][2][ld_xaff]; 2: launch_scale_weight (prec 0 / _BF16 / _F16)
 * of w [npad][kc] -> wu [n_utt][npad][kc] (fp32 or 16-bit elements; kc == C, C % 4 == 0: the kernel averages gx over kc columns). */
typedef struct stts_grn_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* part;
  const float* gamma;
  const float* w;
  float* gx;
  float* xaff;
  void* wu;
  int64_t part_elems, gamma_elems, w_elems, gx_elems, xaff_elems, wu_elems;
  int32_t n_utt, mode, C, ld_ss, ss_stride, ld_gx, ld_xaff, npad, kc, prec;
} stts_grn_args;
int stts_op_grn(void* stream, const stts_grn_args* args);
/* The 2-D implicit-GEMM convolution (csrc/conv2d.hip.h; tests/test_hip_conv2d.py): conv2d_pack of w_host [cout][cin0 + cin1][ntap] (bias_host [cout] or
 * null) at width npad (16 / 32 / a multiple of 64: the tile), then one conv2d_launch.  Channels-last packed rows: x0 [((off_in[u] >> sh) + t) * Fin + f][ld0],
 * x1 the same with ld1 (null when ld1 == 0); base grid of (off_out[u + 1] - off_out[u]) >> sh rows of F columns per utterance; tap i of base position
 * (t, f) reads input position (t + dt[i], f + df[i]), zeros outside the utterance's [0, T_u) x [0, Fin); the result goes to row
 * (t' * up + pt) * (F * up) + f * up + pf of y [.][ldy] (t' the base time row within the batch), columns cout .. ldy - 1 written as 0:
 *   y = (act(sum + bias) + r) / div, act 0 none, 1 ReLU, 2 sigmoid; r [output rows][ldy] or null; lrelu 1: LeakyReLU(0.2) on the operand (npad % 64 == 0).
 * K = ntap * (ld0 + ld1) is summed in chains of `chunk` (a multiple of 16); sliced 0: the chunk sums are added in the kernel, 1: one chunk per grid slice
 * into a scratch the operator allocates, added by conv2d_reduce_kernel (the launch has slices only when there is more than one chunk).
 * Refused before anything is launched: whatever conv2d_pack / conv2d_launch refuse (row strides not multiples of 16, cout > ldy, ldy > npad, ...),
 * offsets that decrease, differ between host and device or are no multiples of 1 << sh, up outside {1, 2}, pt / pf outside [0, up), ntap > 25, and
 * every buffer shorter than the rows a launch can reach: (off_in[n_utt] >> sh) * Fin * ld for x0 / x1, (largest output row + 1) * ldy for y and r. */
typedef struct stts_conv2d_args {
  const float* w_host;
  const float* bias_host;
  const int32_t* off_in_host;
  const int32_t* off_in_dev;
  const int32_t* off_out_host;
  const int32_t* off_out_dev;
  const float* x0;
  const float* x1;
  const float* r;
  float* y;
  int64_t x0_elems, x1_elems, r_elems, y_elems;
  int32_t dt[25], df[25];
  int32_t ntap, cout, cin0, cin1, ld0, ld1, npad, lrelu, chunk, sliced;
  int32_t n_utt, sh, Fin, F, up, pt, pf, act;
  float div;
  int32_t ldy;
} stts_conv2d_args;
int stts_op_conv2d(void* stream, const stts_conv2d_args* args);
/* The flow-matching estimator's row kernels (csrc/cfm.hip.h) and the sequence rotary embedding (csrc/phoneme.hip.h), one launch per call through the launch
 * helpers the estimator itself uses (tests/test_hip_cfm_kernels.py).  Conventions of the operators above: every tensor caller-owned and on the device,
 * *_elems the element count of the caller's buffer, refusal before anything is launched, host and device offsets must agree.
 *
 * stts_op_cfm_elem   kind 0: mish_kernel in place on x, n float4s;  1: swiglu_kernel, x = A [n rows][2 C] -> y [n rows][C] = silu(A[:, :C]) * A[:, C:];
 *                    2: gated_residual_kernel, y = x + t * (ada[u][2 C + c] + 1) over packed rows [rows, C], ada [n_utt][3 C].  C % 4 == 0. */
typedef struct stts_cfm_elem_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  float* x;
  const float* t;
  const float* ada;
  float* y;
  int64_t x_elems, t_elems, ada_elems, y_elems, n;
  int32_t n_utt, kind, C;
} stts_cfm_elem_args;
int stts_op_cfm_elem(void* stream, const stts_cfm_elem_args* args);
/* rms_adaln_kernel: y = x' / rms(x') * w * (ada[u][c] + 1) + ada[u][C + c] with x' = x, or (t != null) x' = x + t * (ada_prev[u][2 C + c] + 1); xout (optional)
 * receives x'.  x [rows, ldx], y [rows, ldy] (y may be x itself with ldy == ldx), t and xout [rows, C], w [C], ada / ada_prev [n_utt][3 C].  C <= 1024. */
typedef struct stts_rms_adaln_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* x;
  const float* w;
  const float* ada;
  float* y;
  const float* t;
  const float* ada_prev;
  float* xout;
  int64_t x_elems, w_elems, ada_elems, y_elems, t_elems, ada_prev_elems, xout_elems;
  int32_t n_utt, C, ldx, ldy;
} stts_rms_adaln_args;
int stts_op_rms_adaln(void* stream, const stts_rms_adaln_args* args);
/* Rotary embeddings in place on the column block [col0, col0 + heads * kc) of x [rows, ldx], and on the block at col1 (-1: none).
 *   kind 0: axial_rope_kernel, interleaved pairs of whole heads (kc == d), position linspace(-1, 1, n), freq [heads][d / 2];
 *   kind 1: rope_kernel through run_rope, half-split pairs on the first d = int(kc / 2) features of every head, position = row in the utterance.
 * d even and <= kc; both blocks inside ldx and apart. */
typedef struct stts_rope_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  float* x;
  const float* freq;
  int64_t x_elems, freq_elems;
  int32_t n_utt, kind, ldx, col0, col1, heads, kc, d;
} stts_rope_args;
int stts_op_rope(void* stream, const stts_rope_args* args);
/* One row per utterance.  kind 0: small_linear_kernel, y [n_rows, ldy] = act(x [n_rows, ldx] w [N][K]^T + b) (b optional; act 0 none, 1 Mish);
 *   1: small_layernorm_kernel over N channels (eps 1e-5), w = gamma, b = beta;  2: cfm_time_embed_kernel, x = t [n_rows], w = freqs [N] -> y = cos | sin (ldy >= 2 N). */
typedef struct stts_cfm_small_args {
  const float* x;
  const float* w;
  const float* b;
  float* y;
  int64_t x_elems, w_elems, b_elems, y_elems;
  int32_t kind, n_rows, N, K, act, ldx, ldy;
} stts_cfm_small_args;
int stts_op_cfm_small(void* stream, const stts_cfm_small_args* args);
/* cfm_source_kernel: har [rows, 32] = (tanh(merge_w * sine source), N resampled to the frames, t[u], 0 ...) from f0 / ncurve packed by the curve offsets and
 * the SineGenerator's noise draw [rows].  An utterance with frames needs a curve of at least one point; ldh must be 32. */
typedef struct stts_cfm_source_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const int32_t* curve_off_host;
  const int32_t* curve_off_dev;
  const float* f0;
  const float* ncurve;
  const float* t;
  const float* noise;
  float* har;
  int64_t f0_elems, ncurve_elems, t_elems, noise_elems, har_elems;
  int32_t n_utt, ldh;
  float merge_w;
} stts_cfm_source_args;
int stts_op_cfm_source(void* stream, const stts_cfm_source_args* args);
/* The small kernels between the stages, one at a time through the launch functions the stages themselves call (tests/test_hip_glue_kernels.py).  Conventions as
 * above: every tensor caller-owned and on the device (w_host / b_host excepted), *_elems the element count of the caller's buffer, refusal before any launch.
 *   kind 0  decoder_front_kernel: x = phoneme encoding [rows, ldx >= C], x2 = pitch, x3 = energy [rows]; F0 = wf . pitch + bf, N = wn . energy + bn (3 taps, zero
 *           outside the utterance) -> y = encode input [rows, ldy] = [x | F0 | N | 0 ..], y2 / y3 = concat buffers [rows, ld2]: columns from c_hidden + c_res on
 *           = [F0 | N | 0 ..], the columns before them untouched.
 *   kind 1  run_style (style_fc_kernel / style_fc_batch_kernel, the launcher's own choice): y [n_utt, ldy = J rounded up to 4] = x [n_utt, K] w_host [J, K]^T + b_host.
 *   kind 2  embed_kernel: y [n_rows, ldy] = x [vocab = J, C] rows picked by tokens (int64 [n_rows]) times sqrt(C); an id outside the vocabulary sets bit 1 of *err.
 *   kind 3  mean_rows_kernel: y [n_utt, ldy] = mean over utterance u's rows of x [rows, ldx] (C columns).
 *   kind 4  broadcast_style_kernel: y [rows, ldy] columns [col0, col0 + C) = x [n_utt, ldx] of the row's utterance.
 *   kind 5  row_utt_kernel: iy [rows] = utterance of the row.
 *   kind 6  frame_token_map_kernel, then local_token_kernel: seg_off = frame offsets, tok_off = token offsets, dur [tokens] -> iy [frames] = token row of
 *           every frame at rate `rep`, iy2 [frames] = iy - tok_off[u]. */
typedef struct stts_glue_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const int32_t* tok_off_host;
  const int32_t* tok_off_dev;
  const float* x;
  const float* x2;
  const float* x3;
  const float* w_host;
  const float* b_host;
  const int64_t* tokens;
  const int32_t* dur;
  float* y;
  float* y2;
  float* y3;
  int32_t* iy;
  int32_t* iy2;
  int32_t* err;
  int64_t x_elems, x2_elems, x3_elems, tokens_elems, dur_elems, y_elems, y2_elems, y3_elems, iy_elems, iy2_elems;
  int32_t n_utt, kind, n_rows, C, K, J, ldx, ldy, ld2, col0, rep, c_hidden, c_res;
  float wf[3], bf, wn[3], bn;
} stts_glue_args;
int stts_op_glue(void* stream, const stts_glue_args* args);
/* single_channel_conv_kernel: y[r][ycol] = bias + sum over taps t and channels c of w[t][c] x[r + t - (ntaps - 1) / 2][c], zero outside the utterance, for one or two
 * (x, w, bias, y) sets in one launch.  prec16 0: x fp32 [rows, ldx]; STTS_PREC_BF16 / _F16: 16-bit rows (x_elems counts 16-bit elements).  w fp32 [ntaps][C] on the
 * device, y [rows, ldy].  C and ldx multiples of 4, ntaps odd and at most 7. */
typedef struct stts_chan_conv_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const void* x0;
  const void* x1;
  const float* w0;
  const float* w1;
  float* y0;
  float* y1;
  int64_t x0_elems, x1_elems, w0_elems, w1_elems, y0_elems, y1_elems;
  int32_t n_utt, prec16, nsets, ntaps, C, ldx, ldy, ycol;
  float bias0, bias1;
} stts_chan_conv_args;
int stts_op_chan_conv(void* stream, const stts_chan_conv_args* args);
/* AdaptiveDecoderBlock.forward (models/ada_norm.py:166-182) with weights named `prefix` + reference keys. */
int stts_op_adain_block(stts_ctx* ctx, void* stream, const char* prefix, int n_utt, const int32_t* seg_off_host,
                        const int32_t* seg_off_dev, const float* x, int ldx, int cin, int cout, const float* style, float* y, int ldy,
                        void* ws, size_t ws_bytes);
/* One AdaptiveDecoderBlock, or two chained ones A -> B (B reads [y_A | constant columns]), in any form the block plan can take at any row count: the caller
 * sets the thresholds and flags of the plan (csrc/adain_block.hip.h BlockSwitches; the environment is not read for them) and what it offers, and gets back
 * every block's output and the plan that ran.  Weights named `prefix` + reference keys, packed in the context's precision on first use.
 *   x [rows, ldx >= cin padded as the precision packs it (32; 64 in the 16-bit modes)], style [n_utt, style_dim], ws: workspace of stts_frame_workspace_bytes.
 *   blocks[i].y [rows, ldy >= cout]: the block's output.  Two blocks: blocks[0].y is B's input, so its ldy covers B's padded channels and the CALLER has
 *   filled its columns [cout_A, cin_B) with the constant columns and the rest with zeros; the operator runs the one statistics pass over them, hands
 *   their table to the bridge and rounds them into 16-bit rows, as Decoder.forward does.
 *   blocks[i].y16 (optional, 16-bit modes) [rows, ldy16]: y rounded to the mode's format; blocks[0].y16 of a pair has ldy16 == ldy and serves as B's rounded input.
 *   offer_wino: Winograd scratch; offer_stats: buffers for statistics the producers leave behind; offer_rows16: 16-bit scratch for the rounded inputs;
 *   offer_side: a second stream with fork / join events (owned by the operator) for the learned shortcuts; defer: a folded conv2's split-K reduce may be
 *   left to the next statistics launch (finished on its own after the last block); force_tile: tile of the direct contractions (0: the plan's).
 *   plan_out (host, 8 + 16 * nblocks integers): {wino, sc_out, rows16, wino_stats, stats, bridge_w, side, 0} of the chain plan, then per block {conv1, conv2,
 *   rows16, norm1, norm2, next_norm1, take_pending, defer_conv2, shortcut, cast_x16, y16, affine_serial, bridge_w, force_tile, pending, 0} (the enums of BlockPlan, in
 *   their order; pending: the split-K factor of the reduce conv2 left to the chain, 0 if none).  A negative fold_rows / fold16_rows / rows16 / sc_side_min_rows: the engine's own.  Written before the block's launches, so a refused or failed call still shows what was planned up to there. */
typedef struct stts_adain_chain_block {
  const char* prefix;
  float* y;
  uint16_t* y16;
  int64_t y_elems, y16_elems;
  int32_t cin, cout, ldy, ldy16;
} stts_adain_chain_block;
typedef struct stts_adain_chain_args {
  const int32_t* seg_off_host;
  const int32_t* seg_off_dev;
  const float* x;
  const float* style;
  void* ws;
  int32_t* plan_out;
  int64_t x_elems, style_elems, ws_bytes;
  int32_t n_utt, nblocks, ldx;
  int32_t fold_rows, fold16_rows, rows16, sc_side_min_rows, affine_serial, no_wino_conv2sc, no_stat_fuse, no_wino_stats, bridge;
  int32_t offer_wino, offer_stats, offer_rows16, offer_side, defer, force_tile;
  stts_adain_chain_block blocks[2];
} stts_adain_chain_args;
int stts_op_adain_chain(stts_ctx* ctx, void* stream, const stts_adain_chain_args* args);
/* Multi-head scaled-dot-product attention on packed sequences (MultiHeadAttention.attention, models/text_encoder.py:233-277;
 * models/xut/attention.py): q [q rows, heads * kc], k / v [k rows, heads * kc], o [q rows, heads * kc]; utterance u's queries see its
 * own keys only.  band_centre (optional, [q rows] int32) + window: the pitch/energy predictor's inverted band mask.
 * kernel: 0 = the stage's own choice, 1 = one wave per four queries (attention_kernel), 2 = matrix cores (attention_mfma_kernel,
 * kc 16 / 32 / 40 / 64 / 96 / 128 / 160; heads of 64 split the keys over two wave groups from 128 keys on), 3 = matrix cores, never split. */
int stts_op_attention(void* stream, int n_utt, const int32_t* q_off_host, const int32_t* q_off_dev, const int32_t* k_off_host,
                      const int32_t* k_off_dev, const float* q, const float* k, const float* v, float* o, int heads, int kc,
                      const int32_t* band_centre, int window, int kernel);
/* wavlm_l1_kernel alone: sums[u] (device double) = sum |a - b| over utterance u's rows of two row buffers packed alike ([rows, ld], C real columns);
 * part: device scratch of n_utt * ceil(max_len / 8) doubles; frames (may be null): device int32 [n_utt]. */
int stts_op_wavlm_l1(void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b, int ld, int C, double* part,
                     double* sums, int32_t* frames);
/* The vocoder's STFT / iSTFT at a geometry (n_fft, win, vocoder hop h = hop_length / 4; the rules of stts_finalize_weights) without a model.
 * Utterance u has seg_off[u+1] - seg_off[u] frames and h samples per frame, packed.  generic 0: the kernels the engine would run (the
 * specialised ones at 2048 / 1200 / 75), 1: the run-time-geometry kernels always.
 * stft: sig -> spec = |X|, phase = atan2 [frames, ld] time-major (bins 0 .. n_fft/2, zeros up to ld).
 * istft: logamp, phase [frames, ld] -> audio = tanh(iSTFT(exp(logamp) e^{i phase})) over frames 0 .. T4 (the last repeats row T4 - 1). */
int stts_op_stft_geom(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int n_fft, int win, int h, const float* sig,
                      float* spec, float* phase, int ld, int generic);
int stts_op_istft_geom(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int n_fft, int win, int h, const float* logamp,
                       const float* phase, int ld, float* audio, int generic);
/* WaveNet layer `layer` of the finalized posterior encoder (STTS_W_POSTERIOR) alone: h_in, out_in [rows, hidden], cond [n_utt, ld_cond] (the
 * cond_layer rows; layer i reads columns [i * 2 hidden, (i + 1) * 2 hidden)) -> h_out, out_out [rows, hidden] (other buffers than the inputs).
 * form: 0 = plain contractions, 16 | 32 | 64 = wn_post_kernel on that block height.  out_acc 0: out = skip (what layer 0 does), else out_in + skip.
 * The last layer leaves h alone (h_out = h_in).  ws: rows * hidden floats of scratch. */
int stts_op_posterior_layer(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int layer, int form,
                            int out_acc, const float* h_in, const float* out_in, const float* cond, int ld_cond, float* h_out, float* out_out,
                            void* ws, size_t ws_bytes);
/* Coupling layer `layer` of the flow statistics (STTS_W_FLOW_STATS) alone, in the direction `reverse`: three streams [rows,128] and style [n_utt,64]
 * in, three streams out (other buffers).  form: 0 = the generic form, 16 | 32 | 64 = wn_stats_kernel on that block height.  h0_out [rows,128]: the next
 * coupling layer's h_0 = pre(z') where the form produces it (a fused form, and a next layer exists: f + 1 forward, f - 1 in reverse); otherwise left
 * untouched (may be NULL).  ws: stts_flow_stats_workspace_bytes. */
int stts_op_flow_stats_layer(stts_ctx* ctx, void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int layer, int reverse, int form,
                             const float* z_in, const float* mean_in, const float* logstd_in, const float* style, float* z_out, float* mean_out,
                             float* logstd_out, float* h0_out, void* ws, size_t ws_bytes);
/* Tuning aid (tools/gemm_bench.py): average time of `iters` back-to-back contraction launches on synthetic data.
 * tile: 0 = the launcher's own choice; tune bits: 128 bf16 operands, 256 fp16 operands; only in a library built with
 * -DSTTS_GEMM_TRACE: 2/4/8/16 K-loop ablations (results invalid, timing only), 64 block-timeline trace. */
int stts_bench_gemm(void* stream, int n_utt, int rows_per_utt, int cin, int cout, int k, int tile, int iters, double* avg_ms, int tune);
#endif /* STTS_TEST_OPS */

#ifdef __cplusplus
}
#endif
#endif /* STYLISH_HIP_H_ */

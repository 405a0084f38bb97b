// Context, weight packing and stage orchestration (host side of the library).
#pragma once
#include <math.h>

#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/stylish_hip.h"
#include "common.h"
#include "elementwise.hip.h"
#include "gemm.hip.h"
#include "gemm16.hip.h"
#include "signal.hip.h"
#include "signal_geom.hip.h"
#include "phoneme.hip.h"
#include "wn_layer.hip.h"
#include "wn_layer_small.hip.h"
#include "wn_fused.hip.h"
#include "wn_fused16.hip.h"
#include "wn_block16.hip.h"
#include "wn_fused_x3.hip.h"
#include "wn_block_x3.hip.h"
#include "winograd.hip.h"

namespace stts {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  int64_t dim(int i) const { return shape[i]; }
};

struct PackedConv {
  float* W = nullptr;
  unsigned short* W16 = nullptr;  // bf16 / fp16 copy (16-bit operand modes), same layout; fp32 mode: the three bf16 planes of the exact split (gemm.hip.h, PREC_X3)
  long w16_plane = 0;             // fp32 mode: elements between two of those planes (0: no split form)
  int prec = 0;                   // PREC_* the copy was rounded to
  float* bias = nullptr;
  int npad = 0, N = 0, kc = 0, ntaps = 1;
  int cin_real = 0, rows_real = 0;  // un-padded sizes (FLOP accounting)
};

// Winograd F(6, r) form of a 'same' conv (winograd.hip.h): the n weight planes G_j g as one packed tensor [n][npad][1][kc].
struct WinoConv {
  PackedConv planes;  // W: n planes of npad x kc (plane stride npad * kc); bias: the conv's own bias [npad]
  WinoMats mats;
  int pad = 0;
  bool ready = false;
};

// one entry of a style-projection table
struct StyleSlot {
  int col0 = 0, C = 0;
};

struct StyleTable {
  std::vector<float> hW, hb;  // host staging [J][K], [J]
  float* W = nullptr;
  float* b = nullptr;
  int J = 0, K = 64;
  int add(const HostTensor& w, const HostTensor& bias) {  // returns col0 (4-aligned)
    while (J % 4) {
      hW.insert(hW.end(), K, 0.f);
      hb.push_back(0.f);
      ++J;
    }
    const int c0 = J;
    hW.insert(hW.end(), w.data.begin(), w.data.end());
    hb.insert(hb.end(), bias.data.begin(), bias.data.end());
    J += (int)bias.data.size();
    return c0;
  }
  int ld() const { return round_up(J, 4); }
};

struct AdainBlockW {
  int cin = 0, cout = 0, kcin = 0;  // kcin = cin padded to 32
  PackedConv conv1, conv2, sc;      // sc.W == nullptr: identity shortcut
  WinoConv w1, w2;                  // conv1 / conv2 (identity-shortcut blocks only) in Winograd form (fp32 mode, k = 3), large batches
  StyleSlot n1, n2;
};

// fragment-order weights of one coupling layer for wn_fused_kernel (fp32 mode; wn_fused.hip.h)
struct WnFusedW {
  float* W1[3][4] = {};  // [0: F(2,5), 1: F(4,5), 2: direct (M = 1)][WaveNet layer]: transformed in_layers planes
  float* b1[4] = {};     // in_layers bias, natural order [256]
  float* W2[4] = {};     // res_skip_layers
  float* b2[4] = {};
  float* W3 = nullptr;   // post: proj_mean | proj_logstd
  float* b3m = nullptr;
  float* b3s = nullptr;
  float* W4 = nullptr;   // this layer's own `pre` (run by the tail of the layer before it in reverse order)
  float* b4 = nullptr;
  // 16-bit operand modes (wn_fused16_kernel): the same matrices as 16-bit fragments, conv in direct (tap-major) form
  unsigned short* H1[4] = {};
  unsigned short* H2[4] = {};
  unsigned short* H2b[4] = {};  // res_skip in wn_block16_kernel's tile order (wave w: res 32w.., skip 32w..; layer 3: skip only)
  unsigned short* H3 = nullptr;
  unsigned short* H4 = nullptr;
  // split fp32 (wn_fused_x3_kernel): the 16-bit kernels' fragment arrays as the three bf16 planes of the exact split, direct (tap-major) conv
  unsigned short* X1[4] = {};
  unsigned short* X2[4] = {};
  unsigned short* X2b[4] = {};  // res_skip in wn_block_x3_kernel's tile order (as H2b)
  unsigned short* X3 = nullptr;
  unsigned short* X4 = nullptr;
  long xp1 = 0, xp2[4] = {}, xp3 = 0, xp4 = 0;  // f32x4 units between two planes
  bool ready = false;    // fp32 fragments packed
  bool ready16 = false;  // 16-bit fragments packed
  bool ready_x3 = false; // split-fp32 fragments packed
};

struct FlowLayerW {
  PackedConv pre, in[4], rs[4], proj;
  WnFusedW fused;
  int cond_col0 = 0;
};

struct ConvNextW {
  float* dw_wt = nullptr;  // [K][C] tap-major
  float* dw_b = nullptr;
  int K = 0;
  StyleSlot norm;
  PackedConv pw1, pw2;  // pw2.bias already includes W2 @ grn.beta
  float* grn_gamma = nullptr;
};

struct MrfW {
  PackedConv c1[3], c2[3];
  StyleSlot a1[3], a2[3];
  float* alpha1[3];
  float* alpha2[3];
  int dil[3] = {1, 3, 5};
  int channels = 0, kernel = 0;
  StyleTable table;
};

// How the packers pack while a finalize runs: installed on stts_ctx::pack by a PackScope (below), never by hand.
struct PackMode {
  int prec;      // operand precision the weights are packed for (PREC_*); -1: no scope is open
  bool x3;       // fp32: also the three bf16 planes of every weight (split-fp32 contractions, gemm.hip.h PREC_X3), where the engine allows them
  int kc_align;  // input channels of a packed conv are padded to this (64 for the frame path in a 16-bit mode: conv_gemm16_kernel's K tile)
  int tag;       // STTS_W_* component the allocations belong to (0: context lifetime); a finalize assigns it as it moves between components
};

}  // namespace stts

struct stts_ctx {
  stts_model_dims d;
  int device = 0;
  std::map<std::string, stts::HostTensor> host;
  std::vector<void*> allocs;
  std::vector<int> alloc_tag;  // STTS_W_* component a device allocation belongs to (0: context lifetime); same length as allocs
  int* d_err = nullptr;
  // side streams of stts_frame_path (fp32, large batches): one per caller stream (several host threads may run the path on their own streams)
  struct SideLane {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    // second side stream: short independent contractions inside a stage (the decoder blocks' learned shortcuts, stts::SideWork)
    hipStream_t stream2 = nullptr;
    hipEvent_t fork2 = nullptr, join2 = nullptr;
  };
  std::map<hipStream_t, SideLane> side_lanes;
  std::mutex side_mu;
  int ready = 0;  // STTS_W_* components finalized
  // the engine's precision: written by stts_set_precision only, read by the stages (a finalize packs by `pack`, not by these)
  int prec = 0;   // contraction operand precision (stts::PREC_*), fixed before the first finalize
  bool allow_x3 = true;  // false: STTS_PREC_F32_NATIVE - fp32 contractions on the f32 matrix cores only
  stts::PackMode pack{-1, true, 32, 0};  // what the packers read; valid only inside a stts::PackScope
  // STFT geometry of the frame path (set by finalize_frame from d.n_fft / win_length / hop_length); STTS_SIGNAL_GENERIC=1 at context
  // creation: the run-time-geometry kernels (signal_geom.hip.h) at the default geometry too, for comparisons
  stts::SignalGeom geom;
  bool force_generic_signal = false;
  // shared tables
  float* hann = nullptr;      // periodic Hann(win)
  float2* twiddle = nullptr;  // exp(-2 pi i m / n_fft), m < n_fft/2
  double2* twiddle64 = nullptr;
  // decoder
  float front_wf[3], front_bf, front_wn[3], front_bn;
  stts::PackedConv asr_res;
  stts::AdainBlockW dec[5];
  stts::StyleTable dec_style;
  // prior + flow
  stts::PackedConv prior, post_flow;
  stts::FlowLayerW flow[8];
  stts::StyleTable flow_style;
  // generator
  stts::PackedConv amp_prior, phase_prior, proj_mel, proj_la, proj_ph, amp_out, phase_out;  // *_out: the first n_fft/2 channels
  stts::WinoConv wino_prior[2], wino_out[2];  // the four k = 7 convs of the vocoder in Winograd form (fp32 mode)
  float* nyq_w[2] = {nullptr, nullptr};  // last (Nyquist) output channel of amp/phase output convs, [taps][cin]
  float nyq_b[2] = {0.f, 0.f};
  stts::ConvNextW cnx[4];
  stts::StyleSlot head_amp, head_phase;
  stts::StyleTable gen_style;
  // on-demand op caches (tests)
  std::map<std::string, std::unique_ptr<stts::AdainBlockW>> op_blocks;
  std::map<std::string, std::unique_ptr<stts::StyleTable>> op_tables;
  std::map<std::string, std::unique_ptr<stts::MrfW>> op_mrf;
  std::shared_ptr<void> phoneme;  // stts::PhonemeModel (phoneme_model.hip.h)
  std::shared_ptr<void> cfm;      // stts::CfmModel (cfm.hip.h)
  std::shared_ptr<void> hubert;   // stts::HubertModel (hubert.hip.h)
  std::shared_ptr<void> mel_style;  // stts::MelStyleModel (mel_style.hip.h)
  std::shared_ptr<void> cfm_pitch;  // stts::CfmPitchNetW (cfm_pitch.hip.h)
  std::shared_ptr<void> ssl;        // stts::SslW (ssl.hip.h)
  std::shared_ptr<void> rmvpe;      // stts::RvW (rmvpe.hip.h)
  std::shared_ptr<void> aligner;    // stts::AlW (aligner.hip.h)
  std::shared_ptr<void> wavlm;      // stts::WavlmW (wavlm.hip.h)
  std::shared_ptr<void> posterior;  // stts::PostW (posterior.hip.h)
  std::shared_ptr<void> flow_stats; // stts::FStatW (flow_stats.hip.h)
  // log-mel front end (log_mel.hip.h): window, twiddles and mel filters per (n_fft, win_length, n_mels, sample_rate), context lifetime
  std::map<std::array<int, 4>, std::shared_ptr<void>> log_mel;  // stts::LogMelTables
  std::mutex log_mel_mu;
  // resampler (resample.hip.h): the fp64 coefficient table per (o, n, lowpass_filter_width, rolloff, method, beta), context lifetime
  std::map<std::tuple<int, int, int, double, int, double>, std::shared_ptr<void>> resample;  // stts::ResampleTable
  std::mutex resample_mu;
  // validation scores (val_scores.hip.h): window, twiddles and the phase weights w_k per (n_fft, win_length), context lifetime
  std::map<std::array<int, 2>, std::shared_ptr<void>> val_scores;  // stts::ValTables
  std::mutex val_scores_mu;
};

namespace stts {

// ------------------------------------------------------------------------------------------------
// small host utilities
// ------------------------------------------------------------------------------------------------
// Installs a packing mode for the lifetime of the scope and puts the previous one back on every exit path, an exception included.  Scopes nest.
struct PackScope {
  stts_ctx* c;
  PackMode saved;
  PackScope(stts_ctx* ctx, const PackMode& m) : c(ctx), saved(ctx->pack) { c->pack = m; }
  ~PackScope() { c->pack = saved; }
  PackScope(const PackScope&) = delete;
  PackScope& operator=(const PackScope&) = delete;
};
// the mode of everything that is not a model finalize (context-lifetime tables, the test operators' on-demand packing)
inline PackMode engine_mode(const stts_ctx* c) { return {c->prec, true, 32, 0}; }
inline bool packs_x3(const stts_ctx* c) { return c->allow_x3 && c->pack.x3 && x3_enabled(); }

template <typename T>
inline int dev_upload(stts_ctx* c, const std::vector<T>& h, T** out) {
  STTS_CHECK(c->pack.prec >= 0, "dev_upload outside a PackScope");
  void* p = nullptr;
  STTS_HIP(hipMalloc(&p, std::max<size_t>(h.size(), 1) * sizeof(T)));
  c->allocs.push_back(p);
  c->alloc_tag.push_back(c->pack.tag);
  if (!h.empty()) STTS_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)p;
  return 0;
}

// Re-finalizing a component (a shim re-bound with other weights) releases the device buffers of its previous packing.
inline void free_component_allocs(stts_ctx* c, int mask) {
  bool any = false;
  for (size_t i = 0; i < c->allocs.size(); ++i) any = any || (c->alloc_tag[i] & mask);
  if (!any) return;
  (void)hipDeviceSynchronize();  // kernels that read the old buffers may still be queued
  size_t k = 0;
  for (size_t i = 0; i < c->allocs.size(); ++i) {
    if (c->alloc_tag[i] & mask) {
      (void)hipFree(c->allocs[i]);
    } else {
      c->allocs[k] = c->allocs[i];
      c->alloc_tag[k++] = c->alloc_tag[i];
    }
  }
  c->allocs.resize(k);
  c->alloc_tag.resize(k);
}

inline const HostTensor* find(stts_ctx* c, const std::string& name) {
  auto it = c->host.find(name);
  return it == c->host.end() ? nullptr : &it->second;
}
#define STTS_GET(var, name)                                   \
  const stts::HostTensor* var = stts::find(c, (name));        \
  if (!var) return stts::fail("missing weight '%s'", std::string(name).c_str())

// w = g * v / ||v||, norm over all dims but 0 (torch weight_norm dim=0; reference: models/decoder.py:35-45
// parametrization keys original0/original1, models/flow.py:40,52,60 legacy keys weight_g/weight_v)
inline HostTensor fold_weight_norm(const HostTensor& g, const HostTensor& v) {
  HostTensor w;
  w.shape = v.shape;
  w.data.resize(v.data.size());
  const int64_t rows = v.shape[0], per = (int64_t)v.data.size() / rows;
  for (int64_t r = 0; r < rows; ++r) {
    double s = 0;
    for (int64_t i = 0; i < per; ++i) s += (double)v.data[r * per + i] * v.data[r * per + i];
    const float scale = g.data[r] / (float)sqrt(s);
    for (int64_t i = 0; i < per; ++i) w.data[r * per + i] = v.data[r * per + i] * scale;
  }
  return w;
}

// fetch a conv/linear weight by module path, folding whichever weight-norm flavour is present
inline int get_weight(stts_ctx* c, const std::string& p, HostTensor* w) {
  if (const HostTensor* g = find(c, p + ".parametrizations.weight.original0")) {
    STTS_GET(v, p + ".parametrizations.weight.original1");
    *w = fold_weight_norm(*g, *v);
  } else if (const HostTensor* g2 = find(c, p + ".weight_g")) {
    STTS_GET(v, p + ".weight_v");
    *w = fold_weight_norm(*g2, *v);
  } else {
    STTS_GET(v, p + ".weight");
    *w = *v;
  }
  if (w->shape.size() == 2) w->shape.push_back(1);  // Linear == conv k=1
  return 0;
}

// Pack rows of a [cout][cin][k] weight: out[n'][tap][ci] for ci in [0,kc) taking input channel cin_lo+ci.
// row_of[n'] = source row (or -1 for zero padding); bias follows the same row order.
// host-side round-to-nearest-even conversions for the 16-bit weight copies
inline unsigned short f32_to_bf16(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);  // NaN
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(unsigned short h) {
  const unsigned u = (unsigned)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// exact three-term bf16 split of an fp32 value (gemm.hip.h split3_bf16, PREC_X3): f = p0 + p1 + p2, every term the RNE bf16 of what is left;
// the top term that of f clamped to +-0x7F7F7FFF (finite from 0x7F7F8000 up, where it would round to Inf); +-Inf is (0, 0, +-Inf); NaN stays NaN
inline void split3_host(float f, unsigned short* p0, unsigned short* p1, unsigned short* p2) {
  if (std::isinf(f)) {
    *p0 = *p1 = 0;
    *p2 = f32_to_bf16(f);
    return;
  }
  const unsigned tbits = 0x7f7f7fffu;
  float tmax;
  memcpy(&tmax, &tbits, 4);
  *p0 = f32_to_bf16(f != f ? f : std::fmin(std::fmax(f, -tmax), tmax));
  const float r1 = f - bf16_to_f32(*p0);
  *p1 = f32_to_bf16(r1);
  *p2 = f32_to_bf16(r1 - bf16_to_f32(*p1));
}
inline unsigned short f32_to_f16(float f) {
  const _Float16 h = (_Float16)f;  // IEEE RNE, saturates to inf
  unsigned short r;
  memcpy(&r, &h, 2);
  return r;
}

inline int pack_rows(stts_ctx* c, const HostTensor& w, const HostTensor* bias, const std::vector<int>& row_of, int cin_lo, int cin_n,
                     int kc, int N, PackedConv* out, float scale = 1.0f) {
  STTS_CHECK(c->pack.prec >= 0, "pack_rows outside a PackScope");
  const int prec = c->pack.prec;
  const int cin = (int)w.shape[1], k = (int)w.shape[2];
  const int npad = (int)row_of.size();
  std::vector<float> pw((size_t)npad * k * kc, 0.f), pb(npad, 0.f);
  for (int n = 0; n < npad; ++n) {
    const int r = row_of[n];
    if (r < 0) continue;
    for (int t = 0; t < k; ++t)
      for (int ci = 0; ci < cin_n; ++ci) pw[((size_t)n * k + t) * kc + ci] = w.data[((size_t)r * cin + cin_lo + ci) * k + t] * scale;
    if (bias) pb[n] = bias->data[r] * scale;
  }
  STTS_TRY(dev_upload(c, pw, &out->W));
  STTS_TRY(dev_upload(c, pb, &out->bias));
  out->prec = prec;
  out->W16 = nullptr;
  out->w16_plane = 0;
  if (prec != PREC_F32 || packs_x3(c)) {
    const bool split = prec == PREC_F32;
    std::vector<unsigned short> h(pw.size() * (split ? 3 : 1));
    if (split) {
      out->w16_plane = (long)pw.size();
      for (size_t i = 0; i < pw.size(); ++i) split3_host(pw[i], &h[i], &h[pw.size() + i], &h[2 * pw.size() + i]);
    } else
    for (size_t i = 0; i < pw.size(); ++i) h[i] = prec == PREC_BF16 ? f32_to_bf16(pw[i]) : f32_to_f16(pw[i]);
    STTS_TRY(dev_upload(c, h, &out->W16));
  }
  out->npad = npad;
  out->N = N;
  out->kc = kc;
  out->ntaps = k;
  out->cin_real = cin_n;
  out->rows_real = 0;
  for (int r : row_of) out->rows_real += r >= 0;
  return 0;
}

inline std::vector<int> plain_rows(int cout) {
  std::vector<int> r(round_up(cout, 128), -1);
  for (int i = 0; i < cout; ++i) r[i] = i;
  return r;
}
// paired packing: result channel ch has its 'a' row at a_lo+ch and its 'b' row at b_lo+ch; within every 64 packed rows
// the first 32 are 'a' rows and the next 32 the matching 'b' rows (see EPI_GATE in gemm.hip.h).
inline std::vector<int> paired_rows(int nres, int a_lo, int b_lo) {
  std::vector<int> r(round_up(2 * nres, 128), -1);
  for (int ch = 0; ch < nres; ++ch) {
    const int g = ch / 32, q = ch % 32;
    r[g * 64 + q] = a_lo + ch;
    r[g * 64 + 32 + q] = b_lo + ch;
  }
  return r;
}

inline int pack_plain(stts_ctx* c, const std::string& p, bool has_bias, int cin_lo, int cin_n, PackedConv* out, float scale = 1.0f) {
  HostTensor w;
  STTS_TRY(get_weight(c, p, &w));
  const HostTensor* b = has_bias ? find(c, p + ".bias") : nullptr;
  if (has_bias && !b) return fail("missing weight '%s.bias'", p.c_str());
  if (cin_n < 0) cin_n = (int)w.shape[1] - cin_lo;
  return pack_rows(c, w, b, plain_rows((int)w.shape[0]), cin_lo, cin_n, round_up(cin_n, c->pack.kc_align), (int)w.shape[0], out, scale);
}

inline int upload_table(stts_ctx* c, StyleTable* t) {
  while (t->J % 4) {
    t->hW.insert(t->hW.end(), t->K, 0.f);
    t->hb.push_back(0.f);
    ++t->J;
  }
  STTS_TRY(dev_upload(c, t->hW, &t->W));
  STTS_TRY(dev_upload(c, t->hb, &t->b));
  return 0;
}

inline int add_style(stts_ctx* c, StyleTable* t, const std::string& p, int C, StyleSlot* slot) {
  STTS_GET(w, p + ".fc.weight");
  STTS_GET(b, p + ".fc.bias");
  STTS_CHECK((int)b->data.size() == 2 * C, "%s.fc has %zu outputs, expected %d", p.c_str(), b->data.size(), 2 * C);
  slot->col0 = t->add(*w, *b);
  slot->C = C;
  return 0;
}

inline int pack_winograd(stts_ctx* c, const HostTensor& w, const HostTensor* bias, int cin_lo, int cin_n, int cout_used, WinoConv* out) {
  static const bool disabled = getenv("STTS_NO_WINOGRAD") != nullptr;  // debugging aid: every conv then runs in its direct form
  if (disabled) return 0;  // out->ready stays false
  STTS_CHECK(c->pack.prec >= 0, "pack_winograd outside a PackScope");
  const int cin = (int)w.shape[1], r = (int)w.shape[2];
  STTS_CHECK(wino_matrices(r, &out->mats), "winograd: unsupported kernel size %d (or self-check failed)", r);
  const int n = out->mats.n, npad = round_up(cout_used, 128), kc = round_up(cin_n, 32);
  HostTensor wp;
  wp.shape = {(int64_t)n * cout_used, cin, 1};
  wp.data.assign((size_t)n * cout_used * cin, 0.f);
  for (int j = 0; j < n; ++j)
    for (int co = 0; co < cout_used; ++co)
      for (int ci = 0; ci < cin; ++ci) {
        double acc = 0;
        for (int k = 0; k < r; ++k) acc += out->mats.G[j][k] * (double)w.data[((size_t)co * cin + ci) * r + k];
        wp.data[((size_t)j * cout_used + co) * cin + ci] = (float)acc;
      }
  std::vector<int> row_of((size_t)n * npad, -1);
  for (int j = 0; j < n; ++j)
    for (int co = 0; co < cout_used; ++co) row_of[(size_t)j * npad + co] = j * cout_used + co;
  {
    PackMode f32 = c->pack;
    f32.prec = PREC_F32;  // the transformed weights span ~3 decades (G up to 729): fp32 operands only
    PackScope scope(c, f32);
    STTS_TRY(pack_rows(c, wp, nullptr, row_of, cin_lo, cin_n, kc, cout_used, &out->planes));
  }
  out->planes.npad = npad;
  out->planes.cin_real = cin_n;
  out->planes.rows_real = cout_used;
  if (bias) {
    std::vector<float> pb(npad, 0.f);
    for (int co = 0; co < cout_used; ++co) pb[co] = bias->data[co];
    STTS_TRY(dev_upload(c, pb, &out->planes.bias));
  } else {
    out->planes.bias = nullptr;
  }
  out->pad = (r - 1) / 2;
  out->ready = true;
  return 0;
}

// one ConvNeXtBlock with an AdaptiveLayerNorm (models/generator.py:441-499) at h channels and a k-tap depthwise conv; its norm.fc goes into `table`
inline int pack_convnext_block(stts_ctx* c, const std::string& q, int h, int k, StyleTable* table, ConvNextW* o) {
  ConvNextW& B = *o;
  STTS_GET(dw, q + "dwconv.weight");
  STTS_GET(db, q + "dwconv.bias");
  STTS_CHECK(dw->shape.size() == 3 && dw->shape[0] == h && dw->shape[1] == 1 && dw->shape[2] == k, "%sdwconv: expected [%d, 1, %d]", q.c_str(), h, k);
  B.K = k;
  std::vector<float> wt((size_t)B.K * h);
  for (int ch = 0; ch < h; ++ch)
    for (int kk = 0; kk < B.K; ++kk) wt[(size_t)kk * h + ch] = dw->data[(size_t)ch * B.K + kk];
  STTS_TRY(dev_upload(c, wt, &B.dw_wt));
  STTS_TRY(dev_upload(c, db->data, &B.dw_b));
  STTS_TRY(add_style(c, table, q + "norm", h, &B.norm));
  STTS_TRY(pack_plain(c, q + "pwconv1", true, 0, h, &B.pw1));
  // pwconv2 with GRN's beta folded into the bias: W2 (U*s + beta) + b2 = (W2*s) U + (W2 beta + b2)
  HostTensor w2;
  STTS_TRY(get_weight(c, q + "pwconv2", &w2));
  STTS_GET(b2, q + "pwconv2.bias");
  STTS_GET(gg, q + "grn.gamma");
  STTS_GET(gb, q + "grn.beta");
  HostTensor b2f = *b2;
  const int ci = (int)w2.shape[1];
  for (int r = 0; r < (int)w2.shape[0]; ++r) {
    double s = 0;
    for (int kk = 0; kk < ci; ++kk) s += (double)w2.data[(size_t)r * ci + kk] * gb->data[kk];
    b2f.data[r] = (float)((double)b2->data[r] + s);
  }
  STTS_TRY(pack_rows(c, w2, &b2f, plain_rows((int)w2.shape[0]), 0, ci, round_up(ci, 32), (int)w2.shape[0], &B.pw2));
  return dev_upload(c, gg->data, &B.grn_gamma);
}

inline int pack_adain_block(stts_ctx* c, const std::string& p, int cin, int cout, StyleTable* table, AdainBlockW* o) {
  o->cin = cin;
  o->cout = cout;
  o->kcin = round_up(cin, c->pack.kc_align);
  STTS_TRY(pack_plain(c, p + ".conv1", true, 0, cin, &o->conv1));
  o->w1 = WinoConv();
  if (c->pack.prec == PREC_F32) {
    HostTensor w1;
    STTS_TRY(get_weight(c, p + ".conv1", &w1));
    if (w1.shape[2] == 3) STTS_TRY(pack_winograd(c, w1, find(c, p + ".conv1.bias"), 0, cin, cout, &o->w1));
  }
  STTS_TRY(pack_plain(c, p + ".conv2", true, 0, cout, &o->conv2));
  o->w2 = WinoConv();
  if (find(c, p + ".conv1x1.parametrizations.weight.original0") || find(c, p + ".conv1x1.weight")) STTS_TRY(pack_plain(c, p + ".conv1x1", false, 0, cin, &o->sc));
  if (c->pack.prec == PREC_F32) {  // conv2 is a plain conv + residual (the block's input, or its learned 1x1 shortcut computed first): it has a Winograd form too
    HostTensor w2;
    STTS_TRY(get_weight(c, p + ".conv2", &w2));
    if (w2.shape[2] == 3) STTS_TRY(pack_winograd(c, w2, find(c, p + ".conv2.bias"), 0, cout, cout, &o->w2));
  }
  STTS_TRY(add_style(c, table, p + ".norm1", cin, &o->n1));
  STTS_TRY(add_style(c, table, p + ".norm2", cout, &o->n2));
  return 0;
}

// wn_fused_kernel operands of coupling layer `q` (prefix "...flow.flows.N."): every matrix in MFMA-fragment order
// (wn_fused.hip.h: pack_fragments), the k = 5 conv as F(2,5) and F(4,5) planes G_j g computed in double.
inline int pack_wn_fused(stts_ctx* c, const std::string& q, const HostTensor& pm, const HostTensor& pl, const HostTensor& pmb, const HostTensor& plb,
                         WnFusedW* o) {
  const int C = kWnC;
  auto rows_of = [](const HostTensor& w) {  // [rows][K] (k = 1) as double
    const int rows = (int)w.shape[0], K = (int)(w.data.size() / rows);
    std::vector<std::vector<double>> r(rows, std::vector<double>(K));
    for (int n = 0; n < rows; ++n)
      for (int k = 0; k < K; ++k) r[n][k] = w.data[(size_t)n * K + k];
    return r;
  };
  for (int i = 0; i < 4; ++i) {
    HostTensor w, wr;
    STTS_TRY(get_weight(c, q + "enc.in_layers." + std::to_string(i), &w));
    STTS_GET(b, q + "enc.in_layers." + std::to_string(i) + ".bias");
    STTS_CHECK(w.shape[0] == 2 * C && w.shape[1] == C && w.shape[2] == 5 && (int)b->data.size() == 2 * C, "wn_fused: in_layers.%d has an unexpected shape", i);
    if (c->pack.prec != PREC_F32) {
      // direct form, K-major rows [tap][cin] so that k-step s = tap * 4 + (cin / 32) covers K offsets [32 s, 32 s + 32)
      std::vector<std::vector<float>> kr((size_t)2 * C, std::vector<float>(5 * C));
      for (int n = 0; n < 2 * C; ++n)
        for (int ci = 0; ci < C; ++ci)
          for (int k = 0; k < 5; ++k) kr[n][(size_t)k * C + ci] = w.data[((size_t)n * C + ci) * 5 + k];
      // wave w, tile (half h, c): output rows h * 128 + 32 w + 16 c + col
      const std::vector<unsigned short> f16v = pack_fragments16(c->pack.prec, kWnWaves, 5 * C / 32, 4, [&](int wv, int t, int col) {
        return kr[(size_t)(t >> 1) * C + 32 * wv + 16 * (t & 1) + col].data();
      }, f32_to_bf16, f32_to_f16);
      STTS_TRY(dev_upload(c, f16v, &o->H1[i]));
    }
    const bool x3pack = c->pack.prec == PREC_F32 && packs_x3(c);
    if (x3pack) {
      std::vector<std::vector<float>> kr((size_t)2 * C, std::vector<float>(5 * C));
      for (int n = 0; n < 2 * C; ++n)
        for (int ci = 0; ci < C; ++ci)
          for (int k = 0; k < 5; ++k) kr[n][(size_t)k * C + ci] = w.data[((size_t)n * C + ci) * 5 + k];
      const std::vector<unsigned short> fx = pack_fragments_x3(kWnWaves, 5 * C / 32, 4, [&](int wv, int t, int col) {
        return kr[(size_t)(t >> 1) * C + 32 * wv + 16 * (t & 1) + col].data();
      }, split3_host);
      STTS_TRY(dev_upload(c, fx, &o->X1[i]));
      o->xp1 = (long)(fx.size() / 3 / 8);
    }
    for (int v = 0; v < 3 && c->pack.prec == PREC_F32; ++v) {
      WnFusedMats mt;
      const int vm = v == 0 ? 2 : (v == 1 ? 4 : 1);
      STTS_CHECK(wn_fused_matrices(vm, &mt), "wn_fused: F(%d,5) matrices failed their self-check", vm);
      const int nc = mt.n;
      std::vector<std::vector<double>> plane((size_t)nc * 2 * C, std::vector<double>(C));  // [component][output row][cin]
      for (int j = 0; j < nc; ++j)
        for (int n = 0; n < 2 * C; ++n)
          for (int ci = 0; ci < C; ++ci) {
            double acc = 0;
            for (int k = 0; k < 5; ++k) acc += mt.G[j][k] * (double)w.data[((size_t)n * C + ci) * 5 + k];
            plane[(size_t)j * 2 * C + n][ci] = acc;
          }
      // wave w, tile ((component j, half h), c): output rows h * 128 + 32 w + 16 c + col  (tanh rows 0..127 | sigmoid rows 128..255)
      const std::vector<float> f = pack_fragments(kWnWaves, C / 16, nc * 4, [&](int wv, int t, int col) {
        return plane[(size_t)(t >> 2) * 2 * C + ((t >> 1) & 1) * C + 32 * wv + 16 * (t & 1) + col].data();
      });
      STTS_TRY(dev_upload(c, f, &o->W1[v][i]));
    }
    STTS_TRY(dev_upload(c, b->data, &o->b1[i]));
    STTS_TRY(get_weight(c, q + "enc.res_skip_layers." + std::to_string(i), &wr));
    STTS_GET(br, q + "enc.res_skip_layers." + std::to_string(i) + ".bias");
    const int n_rs = (int)wr.shape[0];
    STTS_CHECK((n_rs == 2 * C || n_rs == C) && wr.shape[1] == C && (n_rs == C) == (i == 3), "wn_fused: res_skip_layers.%d has an unexpected shape", i);
    const auto rr = rows_of(wr);
    const int nct = n_rs / 16 / kWnWaves;  // column tiles per wave
    if (c->pack.prec == PREC_F32) {
      const std::vector<float> f2 = pack_fragments(kWnWaves, C / 16, nct, [&](int wv, int t, int col) { return rr[(size_t)16 * nct * wv + 16 * t + col].data(); });
      STTS_TRY(dev_upload(c, f2, &o->W2[i]));
      if (x3pack) {
        const std::vector<unsigned short> fx = pack_fragments_x3(kWnWaves, C / 32, nct, [&](int wv, int t, int col) {
          return wr.data.data() + ((size_t)16 * nct * wv + 16 * t + col) * C;
        }, split3_host);
        STTS_TRY(dev_upload(c, fx, &o->X2[i]));
        o->xp2[i] = (long)(fx.size() / 3 / 8);
        // wn_block_x3_kernel: wave w owns the res rows AND the skip rows [32 w, 32 w + 32) (tiles: res, res + 16, skip, skip + 16; layer 3: skip, skip + 16)
        const int nctb = n_rs == 2 * C ? 4 : 2;
        const std::vector<unsigned short> fxb = pack_fragments_x3(kWnWaves, C / 32, nctb, [&](int wv, int t, int col) {
          const int row = n_rs == 2 * C ? (t < 2 ? 32 * wv + 16 * t + col : C + 32 * wv + 16 * (t - 2) + col) : 32 * wv + 16 * t + col;
          return wr.data.data() + (size_t)row * C;
        }, split3_host);
        STTS_TRY(dev_upload(c, fxb, &o->X2b[i]));  // (same size as X2[i]: xp2[i] is its plane stride too)
      }
    } else {
      const std::vector<unsigned short> f2 = pack_fragments16(c->pack.prec, kWnWaves, C / 32, nct, [&](int wv, int t, int col) {
        return wr.data.data() + ((size_t)16 * nct * wv + 16 * t + col) * C;
      }, f32_to_bf16, f32_to_f16);
      STTS_TRY(dev_upload(c, f2, &o->H2[i]));
      // wn_block16_kernel: wave w owns the res rows AND the skip rows [32 w, 32 w + 32) (tiles: res, res + 16, skip, skip + 16; layer 3: skip, skip + 16)
      const int nctb = n_rs == 2 * C ? 4 : 2;
      const std::vector<unsigned short> f2b = pack_fragments16(c->pack.prec, kWnWaves, C / 32, nctb, [&](int wv, int t, int col) {
        const int row = n_rs == 2 * C ? (t < 2 ? 32 * wv + 16 * t + col : C + 32 * wv + 16 * (t - 2) + col) : 32 * wv + 16 * t + col;
        return wr.data.data() + (size_t)row * C;
      }, f32_to_bf16, f32_to_f16);
      STTS_TRY(dev_upload(c, f2b, &o->H2b[i]));
    }
    STTS_TRY(dev_upload(c, br->data, &o->b2[i]));
  }
  STTS_CHECK(pm.shape[0] == C / 2 && pm.shape[1] == C && pl.shape[0] == C / 2, "wn_fused: proj has an unexpected shape");
  const auto rm = rows_of(pm), rl = rows_of(pl);
  if (c->pack.prec == PREC_F32) {
    const std::vector<float> f3 = pack_fragments(kWnWaves, C / 16, 2, [&](int wv, int t, int col) { return (t == 0 ? rm : rl)[(size_t)16 * wv + col].data(); });
    STTS_TRY(dev_upload(c, f3, &o->W3));
    if (packs_x3(c)) {
      const std::vector<unsigned short> fx = pack_fragments_x3(kWnWaves, C / 32, 2, [&](int wv, int t, int col) {
        return (t == 0 ? pm : pl).data.data() + ((size_t)16 * wv + col) * C;
      }, split3_host);
      STTS_TRY(dev_upload(c, fx, &o->X3));
      o->xp3 = (long)(fx.size() / 3 / 8);
    }
  } else {
    const std::vector<unsigned short> f3 = pack_fragments16(c->pack.prec, kWnWaves, C / 32, 2, [&](int wv, int t, int col) {
      return (t == 0 ? pm : pl).data.data() + ((size_t)16 * wv + col) * C;
    }, f32_to_bf16, f32_to_f16);
    STTS_TRY(dev_upload(c, f3, &o->H3));
  }
  STTS_TRY(dev_upload(c, pmb.data, &o->b3m));
  STTS_TRY(dev_upload(c, plb.data, &o->b3s));
  HostTensor wp;
  STTS_TRY(get_weight(c, q + "pre", &wp));
  STTS_GET(bp, q + "pre.bias");
  STTS_CHECK(wp.shape[0] == C && wp.shape[1] == C / 2, "wn_fused: pre has an unexpected shape");
  const auto rp = rows_of(wp);
  if (c->pack.prec == PREC_F32) {
    const std::vector<float> f4 = pack_fragments(kWnWaves, C / 32, 2, [&](int wv, int t, int col) { return rp[(size_t)32 * wv + 16 * t + col].data(); });
    STTS_TRY(dev_upload(c, f4, &o->W4));
    if (packs_x3(c)) {
      const std::vector<unsigned short> fx = pack_fragments_x3(kWnWaves, C / 64, 2, [&](int wv, int t, int col) {
        return wp.data.data() + ((size_t)32 * wv + 16 * t + col) * (C / 2);
      }, split3_host);
      STTS_TRY(dev_upload(c, fx, &o->X4));
      o->xp4 = (long)(fx.size() / 3 / 8);
    }
  } else {
    const std::vector<unsigned short> f4 = pack_fragments16(c->pack.prec, kWnWaves, C / 64, 2, [&](int wv, int t, int col) {
      return wp.data.data() + ((size_t)32 * wv + 16 * t + col) * (C / 2);
    }, f32_to_bf16, f32_to_f16);
    STTS_TRY(dev_upload(c, f4, &o->H4));
  }
  STTS_TRY(dev_upload(c, bp->data, &o->b4));
  o->ready = c->pack.prec == PREC_F32;
  o->ready16 = c->pack.prec != PREC_F32;
  o->ready_x3 = c->pack.prec == PREC_F32 && packs_x3(c);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// finalize: frame-rate path
// ------------------------------------------------------------------------------------------------
inline int finalize_frame(stts_ctx* c, int which) {
  const stts_model_dims& d = c->d;
  // STFT geometry: 2048 / 1200 / 300 runs the specialised kernels of signal.hip.h, every other supported one those of signal_geom.hip.h
  STTS_TRY(signal_geometry(d.n_fft, d.win_length, d.hop_length, d.sample_rate, c->force_generic_signal, &c->geom));
  const SignalGeom& geo = c->geom;
  // channel sizes come from the model config (lib/config_loader.py:369-414); what the kernels need: 16-byte rows and column
  // offsets (multiples of 32 for the concatenated widths) and the generator reading the decoder's width
  STTS_CHECK(d.style_dim > 0 && d.style_dim % 4 == 0 && d.inter_dim > 0 && d.inter_dim % 4 == 0, "style_dim / inter_dim must be multiples of 4");
  STTS_CHECK(d.dec_hidden > 0 && d.dec_hidden % 32 == 0 && d.dec_residual >= 0 && d.dec_residual % 4 == 0,
             "decoder.hidden_dim must be a multiple of 32 (the flow runs on hidden_dim / 4 channels split in two halves), residual_dim a multiple of 4 (16-byte columns)");
  STTS_CHECK(d.gen_input == d.dec_hidden, "generator.input_dim (%d) must equal decoder.hidden_dim (%d): post_flow feeds the generator", d.gen_input, d.dec_hidden);
  STTS_CHECK(d.gen_hidden > 0 && d.gen_hidden % 32 == 0 && d.gen_inter > 0 && d.gen_inter % 32 == 0,
             "generator.hidden_dim / conv_intermediate_dim must be multiples of 32");
  const std::string sp = "speech_predictor.";
  // tables (context lifetime: the scope opens with tag 0)
  if (!c->hann) {
    std::vector<float> h;
    std::vector<double2> tw64;
    signal_tables(geo.n_fft, geo.win, &h, &tw64);
    STTS_TRY(dev_upload(c, h, &c->hann));
    std::vector<float2> tw(geo.n_fft / 2);
    for (int i = 0; i < geo.n_fft / 2; ++i) tw[i] = make_float2((float)cos(2.0 * M_PI * i / geo.n_fft), (float)-sin(2.0 * M_PI * i / geo.n_fft));
    STTS_TRY(dev_upload(c, tw, &c->twiddle));
    STTS_TRY(dev_upload(c, tw64, &c->twiddle64));
  }
  // decoder (models/decoder.py:6-45)
  if (which & STTS_W_DECODER) {
    c->pack.tag = STTS_W_DECODER;
    c->dec_style = StyleTable();
    c->dec_style.K = d.style_dim;
    HostTensor wf, wn;
    STTS_TRY(get_weight(c, sp + "decoder.F0_conv", &wf));
    STTS_TRY(get_weight(c, sp + "decoder.N_conv", &wn));
    STTS_GET(bf, sp + "decoder.F0_conv.bias");
    STTS_GET(bn, sp + "decoder.N_conv.bias");
    for (int i = 0; i < 3; ++i) {
      c->front_wf[i] = wf.data[i];
      c->front_wn[i] = wn.data[i];
    }
    c->front_bf = bf->data[0];
    c->front_bn = bn->data[0];
    STTS_TRY(pack_plain(c, sp + "decoder.asr_res.0", true, 0, d.inter_dim, &c->asr_res));
    STTS_TRY(pack_adain_block(c, sp + "decoder.encode", d.inter_dim + 2, d.dec_hidden, &c->dec_style, &c->dec[0]));
    for (int i = 0; i < 4; ++i)
      STTS_TRY(pack_adain_block(c, sp + "decoder.decode." + std::to_string(i), d.dec_hidden + 2 + d.dec_residual, d.dec_hidden,
                                &c->dec_style, &c->dec[i + 1]));
    STTS_TRY(upload_table(c, &c->dec_style));
  }
  // prior + flow + post_flow (models/flow.py, models/speech_predictor.py:36-62)
  if (which & STTS_W_FLOW) {
    c->pack.tag = STTS_W_FLOW;
    c->flow_style = StyleTable();
    c->flow_style.K = d.style_dim;
    const int fh = d.dec_hidden / 4, half = fh / 2;
    HostTensor wm, wl;
    STTS_TRY(get_weight(c, sp + "prior_encoder.proj_mean", &wm));
    STTS_TRY(get_weight(c, sp + "prior_encoder.proj_logstd", &wl));
    STTS_GET(bm, sp + "prior_encoder.proj_mean.bias");
    STTS_GET(bl, sp + "prior_encoder.proj_logstd.bias");
    HostTensor wcat = wm, bcat = *bm;
    wcat.data.insert(wcat.data.end(), wl.data.begin(), wl.data.end());
    wcat.shape[0] = 2 * fh;
    bcat.data.insert(bcat.data.end(), bl->data.begin(), bl->data.end());
    STTS_TRY(pack_rows(c, wcat, &bcat, paired_rows(fh, 0, fh), 0, d.dec_hidden, d.dec_hidden, fh, &c->prior));
    for (int f = 0; f < 8; ++f) {
      const std::string q = sp + "flow.flows." + std::to_string(2 * f) + ".";
      FlowLayerW& L = c->flow[f];
      STTS_TRY(pack_plain(c, q + "pre", true, 0, half, &L.pre));
      for (int i = 0; i < 4; ++i) {
        HostTensor w;
        STTS_TRY(get_weight(c, q + "enc.in_layers." + std::to_string(i), &w));
        STTS_GET(b, q + "enc.in_layers." + std::to_string(i) + ".bias");
        STTS_TRY(pack_rows(c, w, b, paired_rows(fh, 0, fh), 0, fh, fh, fh, &L.in[i]));
        STTS_TRY(pack_plain(c, q + "enc.res_skip_layers." + std::to_string(i), true, 0, fh, &L.rs[i]));
      }
      HostTensor pm, pl;
      STTS_TRY(get_weight(c, q + "proj_mean", &pm));
      STTS_TRY(get_weight(c, q + "proj_logstd", &pl));
      STTS_GET(pmb, q + "proj_mean.bias");
      STTS_GET(plb, q + "proj_logstd.bias");
      HostTensor pc = pm, pcb = *pmb;
      pc.data.insert(pc.data.end(), pl.data.begin(), pl.data.end());
      pc.shape[0] = 2 * half;
      pcb.data.insert(pcb.data.end(), plb->data.begin(), plb->data.end());
      STTS_TRY(pack_rows(c, pc, &pcb, paired_rows(half, 0, half), 0, fh, fh, half, &L.proj));
      L.fused = WnFusedW();
      if (fh == kWnC && !getenv("STTS_NO_WN_FUSED")) STTS_TRY(pack_wn_fused(c, q, pm, pl, *pmb, *plb, &L.fused));
      HostTensor cw;
      STTS_TRY(get_weight(c, q + "enc.cond_layer", &cw));
      STTS_GET(cb, q + "enc.cond_layer.bias");
      L.cond_col0 = c->flow_style.add(cw, *cb);
    }
    STTS_TRY(upload_table(c, &c->flow_style));
    STTS_TRY(pack_plain(c, sp + "post_flow", true, 0, fh, &c->post_flow));
  }
  // generator (models/generator.py:340-438)
  if (which & STTS_W_GENERATOR) {
    c->pack.tag = STTS_W_GENERATOR;
    c->gen_style = StyleTable();
    c->gen_style.K = d.style_dim;
    const std::string g = sp + "generator.";
    const int h = d.gen_hidden, hp = h / 2;
    STTS_TRY(pack_plain(c, g + "amp_prior_conv", true, 0, geo.bins, &c->amp_prior));
    STTS_TRY(pack_plain(c, g + "phase_prior_conv", true, 0, geo.bins, &c->phase_prior));
    for (int q = 0; q < 2; ++q) c->wino_prior[q] = c->wino_out[q] = WinoConv();
    if (c->pack.prec == PREC_F32) {
      for (int q = 0; q < 2; ++q) {
        const std::string nm = g + (q == 0 ? "amp_prior_conv" : "phase_prior_conv");
        HostTensor wq;
        STTS_TRY(get_weight(c, nm, &wq));
        if (wq.shape[2] == 7) STTS_TRY(pack_winograd(c, wq, find(c, nm + ".bias"), 0, geo.bins, hp, &c->wino_prior[q]));
      }
    }
    STTS_TRY(pack_plain(c, g + "projector", true, 0, d.gen_input, &c->proj_mel));
    STTS_TRY(pack_plain(c, g + "projector", false, d.gen_input, hp, &c->proj_la));
    STTS_TRY(pack_plain(c, g + "projector", false, d.gen_input + hp, hp, &c->proj_ph));
    // output convs: n_fft/2 + 1 = 8*128 + 1 channels -> GEMM for the first 1024, a dot-product kernel for the last (other geometries: n_fft/2 =
    // 128 .. 2048 GEMM channels, the same split)
    for (int which = 0; which < 2; ++which) {
      const std::string nm = g + (which == 0 ? "amp_output_conv" : "phase_output_conv");
      HostTensor w;
      STTS_TRY(get_weight(c, nm, &w));
      STTS_GET(b, nm + ".bias");
      const int nmain = geo.bins - 1, ci = (int)w.shape[1], kk = (int)w.shape[2];
      STTS_CHECK((int)w.shape[0] == geo.bins && ci == h + hp, "%s: unexpected shape", nm.c_str());
      STTS_TRY(pack_rows(c, w, b, plain_rows(nmain), 0, ci, round_up(ci, 32), nmain, which == 0 ? &c->amp_out : &c->phase_out));
      if (c->pack.prec == PREC_F32 && kk == 7) STTS_TRY(pack_winograd(c, w, b, 0, ci, nmain, &c->wino_out[which]));
      std::vector<float> last((size_t)kk * ci);
      for (int t = 0; t < kk; ++t)
        for (int q = 0; q < ci; ++q) last[(size_t)t * ci + q] = w.data[((size_t)nmain * ci + q) * kk + t];
      STTS_TRY(dev_upload(c, last, &c->nyq_w[which]));
      c->nyq_b[which] = b->data[nmain];
    }
    const int ks[4] = {31, 15, 7, 3};
    for (int i = 0; i < 4; ++i) STTS_TRY(pack_convnext_block(c, g + "convnext." + std::to_string(i) + ".", h, ks[i], &c->gen_style, &c->cnx[i]));
    STTS_TRY(add_style(c, &c->gen_style, g + "amp_final_layer_norm", h, &c->head_amp));
    STTS_TRY(add_style(c, &c->gen_style, g + "phase_final_layer_norm", h, &c->head_phase));
    STTS_TRY(upload_table(c, &c->gen_style));
  }
  c->ready |= which & (STTS_W_DECODER | STTS_W_FLOW | STTS_W_GENERATOR);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// workspace bump allocator (caller-owned memory)
// ------------------------------------------------------------------------------------------------
// Workspace sizing by dry run (every stts_*_workspace_bytes query but the CTC one): a stage carves ALL its buffers from an Arena, checks
// `ok`, and only then launches; under dry_run().on it is handed an Arena over a fake address range with null device pointers, records how
// far it got (STTS_DRY_RETURN) and returns before its first launch.  A stage that calls sub-stages walks them over rest() first.  So the
// bound is what the code asks for, whatever the dims, precision or STTS_* switches; no host code ahead of STTS_DRY_RETURN may read
// through a device pointer.
struct DryRun {
  bool on = false;
  size_t peak = 0;
};
inline DryRun& dry_run() {
  static thread_local DryRun d;
  return d;
}
#define STTS_DRY_RETURN(arena)                                                   \
  do {                                                                            \
    if (stts::dry_run().on) {                                                     \
      stts::dry_run().peak = std::max(stts::dry_run().peak, (arena).offset0 + (arena).used); \
      return 0;                                                                   \
    }                                                                             \
  } while (0)

struct Arena {
  char* base;
  size_t cap, used = 0;
  size_t offset0 = 0;  // where this arena starts inside the caller's workspace (dry-run accounting)
  bool ok = true;
  Arena(void* p, size_t n, size_t off0 = 0) : base((char*)p), cap(n), offset0(off0) {}
  template <typename T>
  T* get(size_t count) {
    const size_t bytes = (count * sizeof(T) + 255) / 256 * 256;
    if (used + bytes > cap) {
      ok = false;
      return nullptr;
    }
    T* p = (T*)(base + used);
    used += bytes;
    return p;
  }
  // the unused tail, for a sub-stage (or scratch that is released again when the sub-arena goes out of scope)
  Arena rest() const { return Arena(base + used, cap - used, offset0 + used); }
};

// Dry mode for a scope; on every exit path it goes back to what it was.  A stage that calls sub-stages walks them under a DryScope over
// rest() before its own first launch: in a query that records their peak, in a real call a workspace too small for any of them is
// refused before anything is launched.
struct DryScope {
  const bool was = dry_run().on;
  DryScope() { dry_run().on = true; }
  ~DryScope() { dry_run().on = was; }
};

// Bytes that `walk` carves: walk(arena) runs one or more stages in dry mode, each over a copy of the (fake, never touched) arena it is
// given; what they return is ignored (a stage that refuses its arguments has carved nothing).
template <typename Walk>
inline size_t dry_run_bytes(Walk&& walk) {
  DryScope dry;
  dry_run().peak = 0;
  walk(Arena(reinterpret_cast<char*>((uintptr_t)1 << 20), (size_t)1 << 46));
  return dry_run().peak + 4096;
}

struct Seg {
  int n_utt;
  const int* host;
  const int* dev;
  // capacity segments: `host` holds UPPER BOUNDS (cumulative capacities; every buffer and grid is sized by them), `dev` the real
  // offsets, known on the device only (frame_offsets_kernel).  The rows of utterance u are [dev[u], dev[u+1]) - packed, so the
  // rows in [dev[n_utt], host[n_utt]) are unused.  dev[u] <= host[u] for every u.
  bool cap = false;
  const int* rows_dev() const { return cap ? dev + n_utt : nullptr; }  // the real row count, for kernels that walk all rows
  int rows() const { return host[n_utt]; }
  int max_len() const {
    int m = 0;
    for (int i = 0; i < n_utt; ++i) m = std::max(m, host[i + 1] - host[i]);
    return m;
  }
};

// Host offsets for a workspace query that knows only (rows, n_utt, max_len): lengths with that total, count and maximum, every
// utterance non-empty (max_len is clipped to what the others leave; <= 0 = unknown: one utterance holds all rows the others leave).
// THE RULE this stands on: a stage's carving may depend on a Seg only through rows(), n_utt and max_len(), and is non-decreasing
// in each - so any batch with these three numbers, or smaller ones, fits.  (A count that depends on how the rows are split, like
// sum over utterances of ceil(len / 4), is carved in its capacity form: wino_plane_rows.)
struct SynthSeg {
  std::vector<int> off;
  SynthSeg(int64_t rows, int n_utt, int64_t max_len) : off(std::max(n_utt, 1) + 1, 0) {
    n_utt = std::max(n_utt, 1);
    rows = std::max<int64_t>(rows, n_utt);
    const int64_t most = rows - (n_utt - 1);
    max_len = max_len <= 0 ? most : std::max(std::min(max_len, most), (rows + n_utt - 1) / n_utt);  // (too small for the total: raised)
    int64_t rest = rows - max_len;
    off[1] = (int)max_len;
    for (int u = 1; u < n_utt; ++u) {
      const int64_t len = std::max<int64_t>(1, std::min(max_len, rest - (n_utt - 1 - u)));
      off[u + 1] = off[u] + (int)len;
      rest -= len;
    }
  }
  Seg seg() const { return Seg{(int)off.size() - 1, off.data(), nullptr}; }
};

inline GemmArgs gemm_args(const Seg& s) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.seg_off = s.dev;
  a.seg_host = s.host;
  a.n_utt = s.n_utt;
  a.rows_total = s.rows();
  a.capacity = s.cap;
  if (!s.cap && s.host && s.n_utt > 0) {  // equal lengths (known on the host): the kernels' tile lookup is arithmetic
    const int len = s.host[1] - s.host[0];
    bool same = len > 0;
    for (int u = 1; u < s.n_utt && same; ++u) same = s.host[u + 1] - s.host[u] == len;
    if (same) { a.uniform_len = len; a.uniform_lo0 = s.host[0]; }
  }
  a.alpha = 1.0f;
  a.xaff_slope = 0.2f;
  a.zeros = zero_page();
  return a;
}
inline void set_seg(GemmArgs& a, int i, const float* X, int ldx, int xcol0, const PackedConv& w, int pad = -1, int dil = 1) {
  GemmSeg& g = a.seg[i];
  g.X = X;
  g.W = w.W;
  g.W16 = w.W16;
  g.w16_plane = w.w16_plane;
  if (i == 0) a.prec = w.prec;
  g.w_utt_stride = 0;
  g.ldx = ldx;
  g.xcol0 = xcol0;
  g.kc = w.kc;
  g.ntaps = w.ntaps;
  g.dil = dil;
  g.pad = pad >= 0 ? pad : (w.ntaps - 1) / 2;
  g.kreal = w.cin_real;
  if (i == 0) a.wrows = w.rows_real;
  if (a.nseg < i + 1) a.nseg = i + 1;
}

// Y = conv(X) through the Winograd form (winograd.hip.h).  Scratch: wino_scratch_floats(s, wc) floats; its head holds the
// group offsets of the batch (wino_setup_kernel), computed once per scratch and shared by every conv that uses it.
struct WinoScratch {
  float* p = nullptr;
  bool setup = false;
  int mp_kc = 0;  // > 0: every conv's M planes start behind input planes of this many columns (chained convs, winograd_bridge_kernel: conv A's M planes and conv B's input planes are live together); 0: behind the conv's own
  explicit operator bool() const { return p != nullptr; }
};
// which of a Winograd-form conv's three launches run: all of them, or (chained convs, winograd_bridge_kernel) the contraction with
// its input planes already in the scratch and / or its M planes left there for the next bridge
struct WinoForm {
  bool planes_ready = false;  // no input transform
  bool stop = false;          // no output transform
};
inline size_t wino_scratch_floats(const Seg& s, const WinoConv& wc) {
  const long pr = wino_plane_rows(s.rows(), s.n_utt);
  // (input planes: fp32, or the three bf16 planes of the split form - 6 bytes per element - when the contraction runs as split fp32)
  return (size_t)wc.mats.n * pr * (wc.planes.kc * 3 / 2 + round_up(wc.planes.N, 32)) + round_up(s.n_utt + 1 + 16, 32) + 32;
}
template <int N>
inline int run_winograd_n(hipStream_t st, const Seg& s, const float* X, int ldx, const WinoConv& wc, float* Y, int ldy, int act, const float* R, int ldr,
                          float alpha, WinoScratch& scratch, const float* aff = nullptr, int ld_aff = 0, float* stat = nullptr, int ld_stat = 0, WinoForm form = WinoForm{}) {
  const int n = wc.mats.n, kc = wc.planes.kc, ldm = round_up(wc.planes.N, 32), ml = s.max_len();
  long pr = 0;  // rows of a component plane: the groups of 4 output rows of all utterances, packed
  for (int u = 0; u < s.n_utt; ++u) pr += ceil_div(s.host[u + 1] - s.host[u], kWinoM);
  const long pr_cap = wino_plane_rows(s.rows(), s.n_utt);
  int* segp = reinterpret_cast<int*>(scratch.p);  // [kWinoMaxN + 1] plane offsets j * plane rows: the contraction's "utterances"
  int* goff = segp + 16;                          // [n_utt + 1] first group of every utterance
  float* Xp = scratch.p + round_up(s.n_utt + 1 + 16, 32);
  // split fp32: the input transform writes the three bf16 planes of every component plane (the contraction stages them as they are)
  // (built, parity-tested, NOT selected: with the planes pre-split the contraction's K loop has no split arithmetic and, on tiles 27 / 28, no register
  //  staging at all - and runs exactly as fast, 78.1 vs 78.7 us on the decoder's conv2 at B = 8, while this transform writes 1.5 x the bytes and the
  //  launch loses its remainder-round plan: cfg2 2 037 vs 2 145 utt/s.  STTS_X3_PRESPLIT=1 switches it on for experiments.)
  static const bool presplit_env = getenv("STTS_X3_PRESPLIT") && atoi(getenv("STTS_X3_PRESPLIT")) != 0;
  const bool presplit = presplit_env && x3_enabled() && wc.planes.w16_plane > 0 && wc.planes.prec == PREC_F32 && kc % 8 == 0;
  STTS_CHECK(!(form.planes_ready || form.stop || scratch.mp_kc) || (!presplit && scratch.mp_kc >= kc), "winograd conv: chained form with pre-split planes or without a common plane layout");
  const long xplane = (long)n * pr_cap * kc;  // elements between two split planes
  float* Mp = Xp + (size_t)n * pr_cap * (scratch.mp_kc ? scratch.mp_kc : kc) * 3 / 2;
  WinoIn ti;
  WinoOut to;
  memcpy(ti.Bt, wc.mats.Bt, sizeof(ti.Bt));
  memcpy(to.At, wc.mats.At, sizeof(to.At));
  const int groups = ceil_div(ml, kWinoM);
  // measurement (bench.py roofline leg): the conv is timed as a whole (both transforms + contraction, stream markers) and
  // credited with the ALGORITHMIC flops of the direct convolution, 2 * rows * cout * cin * taps
  GemmProfiler& prof = gemm_profiler();
  const bool timed = prof.on;
  if (timed) {
    (void)hipEventRecord(prof.next(), st);
    prof.on = false;
  }
  if (!scratch.setup) {
    hipLaunchKernelGGL(wino_setup_kernel, dim3(1), dim3(64), 0, st, s.dev, s.n_utt, kWinoMaxN, goff, segp);
    scratch.setup = true;
  }
  if (form.planes_ready) {  // (a bridge wrote them)
  } else if (presplit)
    hipLaunchKernelGGL((winograd_input_kernel<N, true>), dim3(ceil_div(groups, 4), ceil_div(kc / 4, 64), s.n_utt), dim3(64, 4), 0, st, X, ldx,
                       wc.planes.cin_real, s.dev, wc.pad, ti, Xp, kc, goff, aff, ld_aff, xplane);
  else
  hipLaunchKernelGGL((winograd_input_kernel<N>), dim3(ceil_div(groups, 4), ceil_div(kc / 4, 64), s.n_utt), dim3(64, 4), 0, st, X, ldx,
                     wc.planes.cin_real, s.dev, wc.pad, ti, Xp, kc, goff, aff, ld_aff, 0L);
  std::vector<int> seg_h(n + 1);
  for (int j = 0; j <= n; ++j) seg_h[j] = (int)(j * pr);
  Seg sp{n, seg_h.data(), segp};
  sp.cap = s.cap;  // capacity segments: the planes' host offsets (j * pr) are upper bounds of the device ones (j * real groups) too
  GemmArgs a = gemm_args(sp);
  set_seg(a, 0, Xp, kc, 0, wc.planes, 0);
  a.seg[0].w_utt_stride = (long)wc.planes.npad * kc;
  if (presplit) {
    a.x16 = 1;
    a.seg[0].x_plane = xplane;
  }
  a.N = wc.planes.N; a.bias = nullptr; a.Y = Mp; a.ldy = ldm;
  {
    const int rc = launch_conv_gemm(st, a, EPI_STORE, wc.planes.npad, n, (int)pr);
    if (rc) {
      prof.on = timed;
      return rc;
    }
  }
  // stat: the output transform also leaves the AdaIN statistics of Y per chunk of kWinoStatChunk rows (wino_stat_chunks(s) chunks per utterance)
  if (form.stop) {
  } else if (stat)
    hipLaunchKernelGGL((winograd_output_kernel<N, true>), dim3(ceil_div(groups, 4), ceil_div(ceil_div(wc.planes.N, 4), 64), s.n_utt), dim3(64, 4), 0, st, Mp, ldm, goff,
                       s.dev, to, wc.planes.bias, act, R, ldr, alpha, Y, ldy, wc.planes.N, stat, ld_stat, ceil_div(groups, 4));
  else
    hipLaunchKernelGGL((winograd_output_kernel<N, false>), dim3(ceil_div(groups, 4), ceil_div(ceil_div(wc.planes.N, 4), 64), s.n_utt), dim3(64, 4), 0, st, Mp, ldm, goff,
                       s.dev, to, wc.planes.bias, act, R, ldr, alpha, Y, ldy, wc.planes.N, nullptr, 0, 0);
  if (timed) {
    prof.on = true;
    (void)hipEventRecord(prof.next(), st);
    prof.add((x3_enabled() && wc.planes.w16_plane > 0) ? "winograd_conv_x3" : "winograd_conv", 0, 2.0 * (double)s.rows() * wc.planes.rows_real * wc.planes.cin_real * wc.mats.r,
             2.0 * (double)n * (double)pr * wc.planes.rows_real * wc.planes.cin_real, 0.0);
  }
  STTS_HIP(hipGetLastError());
  return 0;
}
inline int wino_stat_chunks(const Seg& s) { return ceil_div(ceil_div(s.max_len(), kWinoM), 4); }
inline int run_winograd(hipStream_t st, const Seg& s, const float* X, int ldx, const WinoConv& wc, float* Y, int ldy, int act, const float* R, int ldr,
                        float alpha, WinoScratch& scratch, const float* aff = nullptr, int ld_aff = 0, float* stat = nullptr, int ld_stat = 0, WinoForm form = WinoForm{}) {
  STTS_CHECK(wc.ready && (wc.mats.n == 8 || wc.mats.n == 12), "winograd conv not packed");
  STTS_CHECK(ldx % 4 == 0 && ldy % 4 == 0 && (!R || ldr % 4 == 0), "winograd conv: leading dimensions must be multiples of 4");
  STTS_CHECK(!stat || (ld_stat % 4 == 0 && ld_stat >= round_up(wc.planes.N, 4)), "winograd conv: statistics rows of %d floats do not cover %d channels", ld_stat, wc.planes.N);
  return wc.mats.n == 8 ? run_winograd_n<8>(st, s, X, ldx, wc, Y, ldy, act, R, ldr, alpha, scratch, aff, ld_aff, stat, ld_stat, form)
                        : run_winograd_n<12>(st, s, X, ldx, wc, Y, ldy, act, R, ldr, alpha, scratch, aff, ld_aff, stat, ld_stat, form);
}

// The one launch between two chained F(6,3) convs A -> AdaIN -> LeakyReLU -> B (winograd_bridge_kernel, slabs of W channels): A ran with WinoForm::stop (its M
// planes are in the scratch), B runs with WinoForm::planes_ready.  Y = (A's output + bias [+ R]) * alpha is written only if given.  gb / gcol0 / C: the style
// columns and channel count of the norm.  B's input columns beyond A's cout are constant columns: their chunk statistics (part, chunks of kWinoStatChunk rows,
// wino_stat_chunks(s) per utterance) and rows (Xc) come from the caller.
// A block holds one thread per (group, 4 channels) of its utterance: utterances of up to kWinoBridgeGroups groups (1 536 rows).
inline bool wino_bridge_fits(const Seg& s, const WinoConv& A, const WinoConv& Bc, int W) {
  return A.ready && Bc.ready && A.mats.n == 8 && Bc.mats.n == 8 && Bc.pad == 1 && A.planes.N % W == 0 && Bc.planes.kc % W == 0 && Bc.planes.kc >= A.planes.N &&
         W == 16 && ceil_div(s.max_len(), kWinoM) <= kWinoBridgeGroups;
}
inline int run_wino_bridge(hipStream_t st, const Seg& s, const WinoConv& A, const float* R, int ldr, float alpha, float* Y, int ldy, const WinoConv& Bc,
                           const float* gb, int ld_gb, int gcol0, int C, const float* part, int ldpart, const float* Xc, int ldxc, WinoScratch& scratch, int W) {
  STTS_CHECK(wino_bridge_fits(s, A, Bc, W), "winograd bridge: unsupported convs or utterance length");
  STTS_CHECK(scratch.setup && scratch.mp_kc >= Bc.planes.kc && scratch.mp_kc >= A.planes.kc, "winograd bridge: the scratch holds no planes in the common layout");
  STTS_CHECK(Bc.planes.kc == A.planes.N || (part && Xc && ldxc % 4 == 0), "winograd bridge: constant columns without statistics or rows");
  STTS_CHECK((!R || ldr % 4 == 0) && (!Y || ldy % 4 == 0) && C <= Bc.planes.kc && C >= A.planes.N, "winograd bridge: bad leading dimensions or channel count");
  const long pr_cap = wino_plane_rows(s.rows(), s.n_utt);
  WinoBridge a;
  memset(&a, 0, sizeof(a));
  int* segp = reinterpret_cast<int*>(scratch.p);
  float* Xp = scratch.p + round_up(s.n_utt + 1 + 16, 32);
  a.Mp = Xp + (size_t)A.mats.n * pr_cap * scratch.mp_kc * 3 / 2;
  a.ldm = round_up(A.planes.N, 32);
  a.bias = A.planes.bias; a.act = ACT_NONE; a.R = R; a.ldr = ldr; a.alpha = alpha; a.Y = Y; a.ldy = ldy; a.Nout = A.planes.N;
  a.gb = gb; a.ld_gb = ld_gb; a.gcol0 = gcol0; a.C = C; a.eps = 1e-5f;
  a.part = part; a.ldpart = ldpart; a.nchunk = wino_stat_chunks(s); a.Xc = Xc; a.ldxc = ldxc;
  a.Xp = Xp; a.kc = Bc.planes.kc;
  a.goff = segp + 16; a.seg_off = s.dev;
  memcpy(a.to.At, A.mats.At, sizeof(a.to.At));
  memcpy(a.ti.Bt, Bc.mats.Bt, sizeof(a.ti.Bt));
  const dim3 grid(Bc.planes.kc / W, s.n_utt), block(std::max(256, round_up(ceil_div(s.max_len(), kWinoM) * (W / 4), 64)));
  // measurement: the bridge is transform time of conv B - a record of B's family with no flops of its own (bench.py's roofline times a Winograd-form conv with its transforms)
  GemmProfiler& prof = gemm_profiler();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof.on) {
    e0 = prof.next();
    e1 = prof.next();
    prof.add((x3_enabled() && Bc.planes.w16_plane > 0) ? "winograd_conv_x3" : "winograd_conv", 0, 0.0, 0.0, 0.0);
  }
  if (e0) hipExtLaunchKernelGGL((winograd_bridge_kernel<8, 16>), grid, block, 0, st, e0, e1, 0, a);
  else hipLaunchKernelGGL((winograd_bridge_kernel<8, 16>), grid, block, 0, st, a);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int run_style(hipStream_t st, const StyleTable& t, const float* style, int n_utt, float* out) {
  // both kernels hold a weight row in two registers per lane (style_fc_kernel) / 128 floats of LDS (style_fc_batch_kernel): a wider table would lose its columns from 128 on
  STTS_CHECK(t.K > 0 && t.K <= 128, "run_style: a style table of K = %d columns (the style kernels cover 1 .. 128)", t.K);
  if (n_utt >= 16 && t.K % 4 == 0 && t.K <= 128) {  // lane = utterance: no per-utterance reduction (same sums, other order: ~1e-7)
    STTS_LAUNCH_PROF("style_fc_batch_kernel", (size_t)t.J * (t.K + n_utt) * 4, style_fc_batch_kernel, dim3(ceil_div(t.J, 4)), dim3(256), st, t.W, t.b, style, out,
                     t.J, t.K, n_utt, t.K, t.ld());
    STTS_HIP(hipGetLastError());
    return 0;
  }
  STTS_LAUNCH_PROF("style_fc_kernel", (size_t)t.J * (t.K + n_utt) * 4, style_fc_kernel, dim3(ceil_div(t.J, 4)), dim3(256), st, t.W, t.b, style, out, t.J, t.K, n_utt, t.K, t.ld());
  STTS_HIP(hipGetLastError());
  return 0;
}

inline dim3 rows_grid(const Seg& s, int per_row_work) {
  const long total = (long)s.max_len() * per_row_work;
  return dim3((unsigned)std::min<long>(std::max<long>(1, ceil_div((int)std::min<long>(total, 1 << 30), 256)), 512), s.n_utt);
}

// ------------------------------------------------------------------------------------------------
// Launches of the small kernels between the stages (index maps, gathers, broadcasts, one-channel projections): one function per kernel,
// called by the stages and by the test operators (test_ops.hip.h: stts_op_glue / stts_op_chan_conv), so a test runs the stage's own grid.
// ------------------------------------------------------------------------------------------------
inline void launch_embed(hipStream_t st, const long* tokens, const float* emb, int C, int vocab, float* x, int ldx, long R, int* err) {
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)std::min<long>(1024, ceil_div((int)(R * C / 4), 256))), dim3(256), 0, st, tokens, emb, C, vocab, sqrtf((float)C), x, ldx, (int)R, err);
}
inline void launch_mean_rows(hipStream_t st, const Seg& s, const float* x, int ldx, int C, float* out, int ld_out) {
  hipLaunchKernelGGL(mean_rows_kernel, dim3(s.n_utt), dim3(256), 0, st, x, ldx, C, s.dev, out, ld_out);
}
inline void launch_broadcast_style(hipStream_t st, const Seg& s, const float* style, int ld_style, int C, float* y, int ldy, int col0) {
  hipLaunchKernelGGL(broadcast_style_kernel, dim3(std::max(1, ceil_div(s.max_len() * C, 256)), s.n_utt), dim3(256), 0, st, style, ld_style, C, y, ldy, col0, s.dev);
}
inline void launch_row_utt(hipStream_t st, const Seg& s, int* row_utt) {
  hipLaunchKernelGGL(row_utt_kernel, dim3(ceil_div(s.max_len(), 256), s.n_utt), dim3(256), 0, st, s.dev, s.n_utt, row_utt);
}
inline void launch_frame_token_map(hipStream_t st, int n_utt, const int* dur, const int* tok_off, const int* frm_off, int rep, int* src_row) {
  hipLaunchKernelGGL(frame_token_map_kernel, dim3(n_utt), dim3(256), 0, st, dur, tok_off, frm_off, rep, src_row);
}
inline void launch_local_token(hipStream_t st, const Seg& sf, const Seg& sp, const int* src_row, int* centre) {
  hipLaunchKernelGGL(local_token_kernel, dim3(ceil_div(sf.max_len(), 256), sf.n_utt), dim3(256), 0, st, src_row, sf.dev, sp.dev, centre);
}
// nsets 1: s0 alone; 2: both sets in one launch (grid.y).  x16: 0 = fp32 rows, PREC_BF16 / PREC_F16 = 16-bit rows (ldx in elements).  prof: a record for
// the profiler (the vocoder's Nyquist bins).
inline int launch_single_channel_conv(hipStream_t st, const Seg& s, int x16, int nsets, const ChanConvSet& s0, const ChanConvSet& s1, int ldx, int C, int ntaps, int ldy, int ycol,
                                      bool prof = false) {
  STTS_CHECK(ntaps >= 1 && ntaps <= kChanTaps && ntaps % 2 == 1, "single-channel conv: kernel size %d (odd, at most %d)", ntaps, kChanTaps);
  STTS_CHECK((nsets == 1 || nsets == 2) && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldx >= C, "single-channel conv: one or two sets, C and ldx multiples of 4, ldx >= C");
  const dim3 cg((unsigned)ceil_div(s.max_len(), 4 * kChanRows), nsets, s.n_utt);
  if (cg.x == 0) return 0;
  if (prof) {
    const size_t cb = (size_t)nsets * s.rows() * (ldx * (x16 ? 2 : 4) + 4);
    if (x16 == PREC_BF16) STTS_LAUNCH_PROF("single_channel_conv_kernel", cb, single_channel_conv_kernel<PREC_BF16>, cg, dim3(256), st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
    else if (x16 == PREC_F16) STTS_LAUNCH_PROF("single_channel_conv_kernel", cb, single_channel_conv_kernel<PREC_F16>, cg, dim3(256), st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
    else STTS_LAUNCH_PROF("single_channel_conv_kernel", cb, single_channel_conv_kernel<0>, cg, dim3(256), st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
  } else if (x16 == PREC_BF16) {
    hipLaunchKernelGGL(single_channel_conv_kernel<PREC_BF16>, cg, dim3(256), 0, st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
  } else if (x16 == PREC_F16) {
    hipLaunchKernelGGL(single_channel_conv_kernel<PREC_F16>, cg, dim3(256), 0, st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
  } else {
    hipLaunchKernelGGL(single_channel_conv_kernel<0>, cg, dim3(256), 0, st, s0, s1, ldx, C, s.dev, ntaps, ldy, ycol);
  }
  return 0;
}
inline void launch_decoder_front(hipStream_t st, const Seg& s, const FrontArgs& fa) {
  STTS_LAUNCH_PROF("decoder_front_kernel", (size_t)s.rows() * (fa.c_asr + 2 + fa.ld_enc + 2 * 4) * 4, decoder_front_kernel, rows_grid(s, fa.ld_enc / 4), dim3(256), st, fa, s.dev);
}

// row LayerNorm (plain or adaptive, one or two outputs): the vocoder, the ConvNeXt block, the phoneme-rate stages and the test operators
inline int ln_launch(hipStream_t st, const float* X, int ldx, int C, long n_rows, const int* row_utt, float eps, int adaptive, int nout,
                     const LnOut& o0, const LnOut& o1, int act, const LnIn& in = LnIn{}, const int* n_rows_dev = nullptr) {
  STTS_LAUNCH_PROF("row_layernorm_kernel", (size_t)n_rows * C * (1 + nout) * 4, row_layernorm_kernel, dim3((unsigned)ceil_div((int)n_rows, 4)), dim3(256), st, X, ldx, C, (int)n_rows, row_utt, eps,
                     adaptive, nout, o0, o1, act, in, n_rows_dev);
  STTS_HIP(hipGetLastError());
  return 0;
}
}  // namespace stts

#include "adain_block.hip.h"
#include "flow.hip.h"
#include "vocoder.hip.h"
#include "frame_path.hip.h"

#include "phoneme_model.hip.h"

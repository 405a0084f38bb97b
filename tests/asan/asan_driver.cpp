// Sanitizer driver (CPU): loads a weight dump, finalizes every component and walks the stage entry points over the shapes of
// BASELINE's configs with the HIP runtime stubbed out (hip_stub.cpp).  Exercised under -fsanitize=address,undefined:
// weight-norm folding, row / Winograd / fragment packing, style tables, the workspace queries (dry runs of the stages' own carving)
// against the real calls (a stage returns "workspace too small" if the bound is wrong), and the launch planning of every contraction.
// Every stage walk but the frame path's is then repeated one 256-byte unit below the smallest workspace the stage accepts: it must be
// refused with "workspace too small" before anything is launched (`refusal <precision> <case> <stage> : ...`).
// It also says what the packers wrote: after every finalize a line `digest <precision> <what> <hex>` with the stub's digest of the device
// allocations made since the context was created.  Per precision a second context finalizes the same components in another order, with one
// finalize in the middle that must fail, and has to end at the first context's digest: packing must not depend on what was packed before.
// And it says which kernels the reverse flow launches: a line `flowtrace <precision> <case> <switches> : <trace>` per batch shape and setting of the
// STTS_WN_* switches (flow_section below; the trace is the stub's run-length-encoded list of kernel, grid and block in issue order), in all four
// precisions.  tests/test_asan_host.py compares the default choices with the forced ones; two builds plan the same launches exactly when these lines agree.
// The same for the contractions: `gemmtrace <precision> <case> <force_tile> : <trace>` per case of gemm_section below (stts_op_conv1d / stts_op_conv1d_x3, so the
// library is built with -DSTTS_TEST_OPS; a call that fails prints `error` in front of whatever it launched before failing), and
// `launchtrace <precision> <case> : <trace>` around every stage walk.  In the compact grid of conv_gemm_f32, grid.y is the row-tile count and grid.z the split-K factor.
// A second weight dump (a model with 96 flow channels) adds `flowtrace <precision> generic96* -` lines: the flow as plain contractions with the gate,
// split-accumulate and couple epilogues.
// The AdaptiveDecoderBlock chains the same way: `blocktrace <precision> <case> <switches> : <trace>` per case of block_section below, in all four precisions;
// `asan_driver <weights> block` prints those lines only (fp32 and bf16), for one process per setting of the block's process-wide switches.
// The vocoder and the frame path the same way: `frametrace <precision> <call>_<rows> <switches> : <workspace bytes> | <launches on the caller's stream>+<on any other> | <trace>`
// per case of frametrace_section below, in every precision the frame path is walked in.
// `asan_driver <weights> gemm` prints the gemmtrace lines only (no finalize): the STTS_* switches of the contractions are read once per process, so
// tests/asan/build_and_run.py starts one process per setting.
#include <algorithm>
#include <array>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stylish_hip.h"

extern "C" long stts_stub_launch_count();
extern "C" uint64_t stts_stub_digest();
extern "C" void stts_stub_trace_begin();
extern "C" const char* stts_stub_trace_end();
extern "C" long stts_stub_trace_side_count();

#define CK(expr)                                                                  \
  do {                                                                            \
    if ((expr) != 0) {                                                            \
      fprintf(stderr, "FAILED %s:%d %s: %s\n", __FILE__, __LINE__, #expr, stts_last_error()); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static std::vector<float> buf(size_t n) { return std::vector<float>(n ? n : 1, 0.5f); }

static int g_prec = 0;  // precision of the context being walked (for the launchtrace lines)
static void launchtrace(const char* what, const char* trace) {
  std::string tag = what;
  std::replace(tag.begin(), tag.end(), ' ', '_');
  printf("launchtrace %d %s : %s\n", g_prec, tag.c_str(), trace);
}

// `call(bytes)` runs one stage entry point on `bytes` of workspace, which the stage's query sized (`query` bytes: accepted, the caller has
// checked).  Finds the smallest size the stage accepts - acceptance is monotone in the size, so bisection over 256-byte units ends where
// walking down from the query would - and runs the call once more one unit below: refused, by that message, nothing launched.
template <typename Call>
static int refuse_below(const char* what, const char* stage, size_t query, Call call) {
  size_t lo = 0, hi = query / 256;  // units: lo refused, hi accepted
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    (call(mid * 256) == 0 ? hi : lo) = mid;
  }
  const long before = stts_stub_launch_count();
  const int rc = call((hi - 1) * 256);
  const long launched = stts_stub_launch_count() - before;
  if (rc == 0 || !strstr(stts_last_error(), "workspace too small") || launched != 0) {
    fprintf(stderr, "FAILED %s %s: %zu bytes (one unit below the least accepted size): status %d, %ld launches, \"%s\"\n", what, stage, (hi - 1) * 256, rc, launched,
            rc ? stts_last_error() : "");
    return 1;
  }
  std::string tag = what;
  std::replace(tag.begin(), tag.end(), ' ', '_');
  printf("refusal %d %s %s : query %zu bytes, least accepted %zu, refused below it with nothing launched\n", g_prec, tag.c_str(), stage, query, hi * 256);
  return 0;
}
#define REFUSE(what, query, stage, ...)                                                         \
  do {                                                                                          \
    if (refuse_below(what, stage, query, [&](size_t bytes) { return __VA_ARGS__; })) return 1; \
  } while (0)

static std::vector<int32_t> offsets(const std::vector<int>& lens, int scale = 1) {
  std::vector<int32_t> off(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + scale * lens[i];
  return off;
}

static int frame_case(stts_ctx* c, const std::vector<int>& lens, const char* what) {
  const int n = (int)lens.size();
  std::vector<int32_t> off(n + 1, 0);
  int ml = 0;
  for (int i = 0; i < n; ++i) {
    off[i + 1] = off[i] + lens[i];
    ml = lens[i] > ml ? lens[i] : ml;
  }
  const long R = off[n];
  const size_t wsb = stts_frame_workspace_bytes(c, R, n, ml);
  struct Ws {  // untouched (tens of GB for the large configs: the host code only computes pointers into it)
    char* p;
    explicit Ws(size_t n) : p((char*)malloc(n)) {}
    ~Ws() { free(p); }
    char* data() { return p; }
  } ws(wsb);
  if (!ws.p) {
    fprintf(stderr, "cannot reserve %zu bytes of address space\n", wsb);
    return 1;
  }
  auto asr = buf(R * 128), pitch = buf(R), energy = buf(R), style = buf((size_t)n * 64), pn = buf(R * 128), sn = buf(R * 75), ph = buf(1), audio = buf(R * 75);
  auto x = buf(R * 512), mel = buf(R * 512), hs = buf(R * 1088), hp = buf(R * 1088);  // 1088: the spectrum row stride every operand mode accepts (fp32 needs >= 1056, the 16-bit modes 1088)
  stts_stub_trace_begin();
  const long before = stts_stub_launch_count();
  CK(stts_frame_path(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), pn.data(), sn.data(), ph.data(), 0,
                     audio.data(), ws.data(), wsb, 0));
  const long fused = stts_stub_launch_count() - before;
  // the same call with capacity segments (STTS_SEG_CAPACITY: the host offsets are upper bounds, the device ones - the same array here - real)
  CK(stts_frame_path(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), pn.data(), sn.data(), ph.data(), 0,
                     audio.data(), ws.data(), wsb, STTS_SEG_CAPACITY));
  // the staged entry points carve the same workspace stage by stage
  CK(stts_decoder_forward(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), x.data(), 512, ws.data(), wsb));
  CK(stts_prior_flow_forward(c, nullptr, n, off.data(), off.data(), x.data(), 512, style.data(), pn.data(), mel.data(), 512, nullptr, nullptr, ws.data(), wsb));
  CK(stts_harmonic_stft(c, nullptr, n, off.data(), off.data(), pitch.data(), sn.data(), ph.data(), 1, nullptr, hs.data(), hp.data(), 1088, ws.data(), wsb));
  CK(stts_vocoder_forward(c, nullptr, n, off.data(), off.data(), mel.data(), 512, style.data(), hs.data(), hp.data(), 1088, audio.data(), nullptr, nullptr, 0,
                          ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s rows %8ld  workspace %8.1f MB  %ld launches per frame-path call\n", what, R, wsb / 1048576.0, fused);
  return 0;
}

// One stts_frame_path call and one stts_vocoder_forward call over utterances of `lens` rows, each traced on its own:
// `frametrace <precision> <call>_<rows> <switches> : <stts_frame_workspace_bytes> | <launches on the caller's (null) stream>+<launches on any other stream> | <trace>`.
// switches: "-" or "STTS_NO_SIDE_STREAM=1" (read per call).  The shapes sit on the two thresholds of the frame path and the vocoder: 3 000 rows (the side
// stream of the source -> STFT -> prior-conv chain, fp32) and 3 840 rows (16-bit rows in the 16-bit modes).
static int frametrace_case(stts_ctx* c, const std::vector<int>& lens, const char* switches) {
  const int n = (int)lens.size();
  const std::vector<int32_t> off = offsets(lens);
  const long R = off[n];
  const int ml = *std::max_element(lens.begin(), lens.end());
  const size_t wsb = stts_frame_workspace_bytes(c, R, n, ml);
  std::vector<char> ws(wsb);
  auto asr = buf(R * 128), pitch = buf(R), energy = buf(R), style = buf((size_t)n * 64), pn = buf(R * 128), sn = buf(R * 75), ph = buf(1), audio = buf(R * 75);
  auto mel = buf(R * 512), hs = buf(R * 1088), hp = buf(R * 1088);
  unsetenv("STTS_NO_SIDE_STREAM");
  if (strcmp(switches, "-") != 0) setenv("STTS_NO_SIDE_STREAM", strchr(switches, '=') + 1, 1);
  auto line = [&](const char* call, long launched) {
    const char* trace = stts_stub_trace_end();  // (the counts are read after the trace has ended and before the next one begins)
    const long side = stts_stub_trace_side_count();
    printf("frametrace %d %s_%ld %s : %zu | %ld+%ld | %s\n", g_prec, call, R, switches, wsb, launched - side, side, trace);
  };
  stts_stub_trace_begin();
  long before = stts_stub_launch_count();
  int rc = stts_frame_path(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), pn.data(), sn.data(), ph.data(), 0,
                           audio.data(), ws.data(), wsb, 0);
  line("frame_path", stts_stub_launch_count() - before);
  if (rc == 0) {
    stts_stub_trace_begin();
    before = stts_stub_launch_count();
    rc = stts_vocoder_forward(c, nullptr, n, off.data(), off.data(), mel.data(), 512, style.data(), hs.data(), hp.data(), 1088, audio.data(), nullptr, nullptr, 0,
                              ws.data(), wsb);
    line("vocoder_forward", stts_stub_launch_count() - before);
  }
  unsetenv("STTS_NO_SIDE_STREAM");
  if (rc != 0) fprintf(stderr, "FAILED frametrace %ld rows %s: %s\n", R, switches, stts_last_error());
  return rc != 0;
}
static int frametrace_section(stts_ctx* c) {
  for (const char* sw : {"-", "STTS_NO_SIDE_STREAM=1"})
    if (frametrace_case(c, {1000, 1000, 1000}, sw) || frametrace_case(c, {1000, 1000, 1001}, sw)) return 1;
  return frametrace_case(c, {1280, 1280, 1279}, "-") || frametrace_case(c, {1280, 1280, 1280}, "-");
}

// One stts_prior_flow_forward call under `switches` ("NAME=value,NAME=value" or "-"; every other STTS_WN_* switch unset), traced.  want_z: pass a
// z_flow_out (STTS_WN_DEBUG needs one).
static int flow_case(stts_ctx* c, int prec, const std::vector<int>& lens, const char* what, const std::string& switches, bool want_z = false) {
  for (const char* k : {"STTS_WN_M", "STTS_WN_RT", "STTS_WN_X3", "STTS_WN_X3B", "STTS_WN_X3_WAVES", "STTS_WN_DEBUG"}) unsetenv(k);
  for (size_t i = 0; switches != "-" && i < switches.size();) {
    const size_t eq = switches.find('=', i), end = std::min(switches.find(',', i), switches.size());
    setenv(switches.substr(i, eq - i).c_str(), switches.substr(eq + 1, end - eq - 1).c_str(), 1);
    i = end + 1;
  }
  const int n = (int)lens.size();
  std::vector<int32_t> off(n + 1, 0);
  int ml = 0;
  for (int i = 0; i < n; ++i) {
    off[i + 1] = off[i] + lens[i];
    ml = lens[i] > ml ? lens[i] : ml;
  }
  const long R = off[n];
  const size_t wsb = stts_frame_workspace_bytes(c, R, n, ml);
  char* ws = (char*)malloc(wsb);  // untouched but for what the stub's copies move (the STTS_WN_DEBUG hand-back, z_flow_out)
  if (!ws) {
    fprintf(stderr, "cannot reserve %zu bytes of address space\n", wsb);
    return 1;
  }
  auto x = buf(R * 512), style = buf((size_t)n * 64), pn = buf(R * 128), mel = buf(R * 512), zf = buf(want_z ? R * 128 : 0);
  stts_stub_trace_begin();
  const int rc = stts_prior_flow_forward(c, nullptr, n, off.data(), off.data(), x.data(), 512, style.data(), pn.data(), mel.data(), 512, nullptr,
                                         want_z ? zf.data() : nullptr, ws, wsb);
  const char* trace = stts_stub_trace_end();
  free(ws);
  CK(rc);
  printf("flowtrace %d %s %s : %s\n", prec, what, switches.c_str(), trace);
  return 0;
}

// The flow cases of one precision: the batch shapes around the thresholds of the kernel choice with no switch set, the forced choices they must
// equal (tests/test_asan_host.py PINS), and the ragged batch of tests/test_hip_flow_layers.py under every switch that test file and the precision tests use.
static int flow_section(stts_ctx* c, int prec) {
  const std::vector<int> ragged = {1, 2, 15, 16, 17, 31, 33, 47, 49, 63, 65, 97, 130};
  auto x960 = [](int b) { return std::vector<int>(b, 960); };
#define FLOW(...)                                  \
  do {                                             \
    if (flow_case(c, prec, __VA_ARGS__)) return 1; \
  } while (0)
  if (prec == 0 || prec == 3) {
    FLOW(x960(1), "1x960", "-");
    FLOW(x960(8), "8x960", "-");
    FLOW(x960(16), "16x960", "-");
    const char* forced[3] = {prec == 0 ? "STTS_WN_M=1,STTS_WN_X3=1" : "STTS_WN_M=1", prec == 0 ? "STTS_WN_M=2,STTS_WN_X3=2" : "STTS_WN_M=2",
                             prec == 0 ? "STTS_WN_M=4,STTS_WN_X3=4" : "STTS_WN_M=4"};
    FLOW(x960(1), "1x960", forced[0]);
    FLOW(x960(8), "8x960", forced[1]);
    FLOW(x960(16), "16x960", forced[2]);
  }
  if (prec == 3)
    for (const char* sw : {"STTS_WN_M=1", "STTS_WN_M=2", "STTS_WN_M=4", "STTS_WN_M=16"}) FLOW(ragged, "ragged", sw);
  if (prec == 0) {
    std::vector<int> many;
    for (int i = 0; i < 7; ++i)
      for (int l : {1, 2, 15, 16, 17, 31, 33, 63, 65, 130}) many.push_back(l);
    FLOW(std::vector<int>(64, 3200), "64x3200", "-");
    FLOW(ragged, "ragged", "-");
    FLOW(many, "many", "-");
    for (const char* rt : {"1", "2", "4"})  // VARIANTS of tests/test_hip_flow_layers.py
      for (const char* nw : {"8", "4"}) FLOW(ragged, "ragged", std::string("STTS_WN_M=2,STTS_WN_X3=") + rt + ",STTS_WN_X3_WAVES=" + nw);
    for (const char* sw : {"STTS_WN_M=2,STTS_WN_X3=2,STTS_WN_X3B=3", "STTS_WN_M=2,STTS_WN_X3=2,STTS_WN_X3B=4", "STTS_WN_M=1,STTS_WN_X3=-1", "STTS_WN_M=2,STTS_WN_X3=-1",
                           "STTS_WN_M=4,STTS_WN_X3=-1", "STTS_WN_M=16,STTS_WN_X3=-1"})
      FLOW(ragged, "ragged", sw);
    for (const char* k : {"0", "3", "-3", "4", "-4", "32", "-32"}) FLOW(ragged, "ragged", std::string("STTS_WN_DEBUG=") + k, true);
  }
  if (prec == 1 || prec == 2) {
    FLOW(x960(8), "8x960", "-");
    FLOW(x960(23), "23x960", "-");
    FLOW(x960(24), "24x960", "-");
    FLOW(std::vector<int>(64, 3200), "64x3200", "-");
    FLOW(x960(23), "23x960", "STTS_WN_RT=4");
    FLOW(x960(24), "24x960", "STTS_WN_RT=16");
    for (const char* sw : {"STTS_WN_RT=-1", "STTS_WN_RT=4", "STTS_WN_RT=8", "STTS_WN_RT=16"}) FLOW(ragged, "ragged", sw);
  }
#undef FLOW
  for (const char* k : {"STTS_WN_M", "STTS_WN_RT", "STTS_WN_X3", "STTS_WN_X3B", "STTS_WN_X3_WAVES", "STTS_WN_DEBUG"}) unsetenv(k);
  return 0;
}

static int phoneme_case(stts_ctx* c, const std::vector<int>& toks, const std::vector<int>& frames, const char* what) {
  const int n = (int)toks.size();
  std::vector<int32_t> to(n + 1, 0), fo(n + 1, 0), fo4(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    to[i + 1] = to[i] + toks[i];
    fo[i + 1] = fo[i] + frames[i];
    fo4[i + 1] = fo4[i] + 4 * frames[i];
  }
  const long P = to[n], T = fo[n];
  const size_t wsb = stts_phoneme_workspace_bytes(c, P, T, n, *std::max_element(toks.begin(), toks.end()), *std::max_element(frames.begin(), frames.end()));
  std::vector<char> ws(wsb);
  std::vector<int64_t> tokens(P, 3);
  std::vector<int32_t> dur(P, 1);
  auto mu = buf(P * 256), xh = buf(P * 128), sty = buf((size_t)n * 64), logits = buf(P * 16), f0 = buf(T), en = buf(T), enc4 = buf(4 * T * 256), up = buf(4 * T);
  std::vector<int32_t> dur_out(P), idx(4 * T + 1);
  stts_stub_trace_begin();
  for (int which = 0; which < 3; ++which) {
    CK(stts_text_encoder_forward(c, nullptr, which, n, to.data(), to.data(), tokens.data(), mu.data(), 256, xh.data(), ws.data(), wsb));
    CK(stts_text_style_forward(c, nullptr, which, n, to.data(), to.data(), mu.data(), 256, sty.data(), ws.data(), wsb));
  }
  CK(stts_duration_forward(c, nullptr, n, to.data(), to.data(), tokens.data(), logits.data(), dur_out.data(), nullptr, nullptr, nullptr, ws.data(), wsb));
  CK(stts_pitch_energy_forward(c, nullptr, n, to.data(), to.data(), fo.data(), fo.data(), dur.data(), mu.data(), 256, sty.data(), f0.data(), en.data(), nullptr,
                               nullptr, ws.data(), wsb, 0));
  CK(stts_pitch_energy_forward(c, nullptr, n, to.data(), to.data(), fo.data(), fo.data(), dur.data(), mu.data(), 256, sty.data(), f0.data(), en.data(), nullptr,
                               nullptr, ws.data(), wsb, STTS_SEG_CAPACITY));
  {
    std::vector<int32_t> offT(n + 1), offT4(n + 1), need(n);
    CK(stts_frame_offsets(c, nullptr, n, to.data(), dur.data(), fo.data(), offT.data(), offT4.data(), need.data()));
  }
  CK(stts_length_regulate(c, nullptr, n, dur.data(), to.data(), fo4.data(), 4 * T, 4, mu.data(), 256, 128, enc4.data(), 128, idx.data()));
  CK(stts_upsample4(c, nullptr, n, fo.data(), fo.data(), fo4.data(), f0.data(), up.data()));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s tokens %6ld frames %7ld  workspace %8.1f MB (%zu bytes)\n", what, P, T, wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "text_encoder", stts_text_encoder_forward(c, nullptr, 0, n, to.data(), to.data(), tokens.data(), mu.data(), 256, xh.data(), ws.data(), bytes));
  REFUSE(what, wsb, "text_style", stts_text_style_forward(c, nullptr, 0, n, to.data(), to.data(), mu.data(), 256, sty.data(), ws.data(), bytes));
  REFUSE(what, wsb, "duration", stts_duration_forward(c, nullptr, n, to.data(), to.data(), tokens.data(), logits.data(), dur_out.data(), nullptr, nullptr, nullptr, ws.data(), bytes));
  REFUSE(what, wsb, "pitch_energy", stts_pitch_energy_forward(c, nullptr, n, to.data(), to.data(), fo.data(), fo.data(), dur.data(), mu.data(), 256, sty.data(), f0.data(), en.data(),
                                                   nullptr, nullptr, ws.data(), bytes, 0));
  return 0;
}

// sizes the driver cannot know from the dims structs: read off the weights
struct Widths {
  int hubert_dim, spk_dim, n_mels, pitch_asr;
};

// The HuBERT voice-conversion stages over `frames` feature frames per utterance, each sized by stts_hubert_workspace_bytes.
static int hubert_case(stts_ctx* c, const stts_model_dims& d, const Widths& wd, const std::vector<int>& frames, const char* what) {
  const int n = (int)frames.size();
  const std::vector<int32_t> off = offsets(frames);
  const long T = off[n];
  const int ldf = (wd.hubert_dim + 31) / 32 * 32;
  const size_t wsb = stts_hubert_workspace_bytes(c, T, n, *std::max_element(frames.begin(), frames.end()));
  std::vector<char> ws(wsb);
  auto spk = buf((size_t)n * wd.spk_dim), sty = buf((size_t)n * d.style_dim), pe = buf((size_t)n * d.style_dim), feats = buf(T * ldf), asr = buf(4 * T * d.inter_dim);
  auto f0 = buf(T), en = buf(T);
  stts_stub_trace_begin();
  CK(stts_speaker_style(c, nullptr, n, spk.data(), wd.spk_dim, sty.data(), pe.data(), ws.data(), wsb));
  CK(stts_hubert_encoder_forward(c, nullptr, n, off.data(), off.data(), feats.data(), ldf, asr.data(), d.inter_dim, ws.data(), wsb));
  CK(stts_hubert_pitch_energy_forward(c, nullptr, n, off.data(), off.data(), feats.data(), ldf, pe.data(), f0.data(), en.data(), nullptr, ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s frames %7ld  workspace %8.1f MB (%zu bytes)\n", what, T, wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "speaker_style", stts_speaker_style(c, nullptr, n, spk.data(), wd.spk_dim, sty.data(), pe.data(), ws.data(), bytes));
  REFUSE(what, wsb, "hubert_encoder", stts_hubert_encoder_forward(c, nullptr, n, off.data(), off.data(), feats.data(), ldf, asr.data(), d.inter_dim, ws.data(), bytes));
  REFUSE(what, wsb, "hubert_pitch_energy", stts_hubert_pitch_energy_forward(c, nullptr, n, off.data(), off.data(), feats.data(), ldf, pe.data(), f0.data(), en.data(), nullptr,
                                                                 ws.data(), bytes));
  return 0;
}

// MelStyleEncoder (both of them) and CfmPitchPredictor's network over `frames` mel frames per utterance.
static int mel_case(stts_ctx* c, const Widths& wd, const std::vector<int>& frames, const char* what) {
  const int n = (int)frames.size();
  const std::vector<int32_t> off = offsets(frames);
  const long T = off[n];
  auto mel = buf(T * wd.n_mels), style = buf((size_t)n * 256), asr = buf(T * wd.pitch_asr), normed = buf(T), hz = buf(T);
  for (int which : {STTS_W_PE_MEL_STYLE, STTS_W_CFM_PITCH}) {
    const size_t wsb = stts_mel_style_workspace_bytes(c, which, T, n);
    std::vector<char> ws(wsb);
    const std::string name = std::string(what) + (which == STTS_W_PE_MEL_STYLE ? " pe_mel_style" : " spk_emb");
    stts_stub_trace_begin();
    CK(stts_mel_style_forward(c, nullptr, which, n, off.data(), off.data(), mel.data(), wd.n_mels, style.data(), ws.data(), wsb));
    launchtrace(name.c_str(), stts_stub_trace_end());
    printf("  %-44s frames %7ld  workspace %8.1f MB (%zu bytes)\n", name.c_str(), T, wsb / 1048576.0, wsb);
    REFUSE(name.c_str(), wsb, "mel_style", stts_mel_style_forward(c, nullptr, which, n, off.data(), off.data(), mel.data(), wd.n_mels, style.data(), ws.data(), bytes));
  }
  const size_t wsb = stts_cfm_pitch_workspace_bytes(c, T, n);
  std::vector<char> ws(wsb);
  const std::string name = std::string(what) + " cfm_pitch";
  stts_stub_trace_begin();
  CK(stts_cfm_pitch_forward(c, nullptr, n, off.data(), off.data(), asr.data(), wd.pitch_asr, style.data(), normed.data(), hz.data(), 7.f, 1.f, nullptr, ws.data(), wsb));
  launchtrace(name.c_str(), stts_stub_trace_end());
  printf("  %-44s frames %7ld  workspace %8.1f MB (%zu bytes)\n", name.c_str(), T, wsb / 1048576.0, wsb);
  REFUSE(name.c_str(), wsb, "cfm_pitch", stts_cfm_pitch_forward(c, nullptr, n, off.data(), off.data(), asr.data(), wd.pitch_asr, style.data(), normed.data(), hz.data(), 7.f, 1.f, nullptr,
                                             ws.data(), bytes));
  return 0;
}

// AdaptiveHubert over `samples` per utterance, resampled to `frames` feature frames.
static int ssl_case(stts_ctx* c, const stts_ssl_dims& sd, const std::vector<int>& samples, const std::vector<int>& frames, const char* what) {
  const int n = (int)samples.size();
  const std::vector<int32_t> so = offsets(samples), fo = offsets(frames);
  const int ldf = (sd.hidden_size + 31) / 32 * 32;
  const size_t wsb = stts_ssl_workspace_bytes(c, n, so.data());
  std::vector<char> ws(wsb);
  auto wave = buf(so[n]), feats = buf((size_t)fo[n] * ldf);
  stts_stub_trace_begin();
  CK(stts_ssl_forward(c, nullptr, n, so.data(), so.data(), wave.data(), fo.data(), fo.data(), feats.data(), ldf, ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s samples %7d  workspace %8.1f MB (%zu bytes)\n", what, so[n], wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "ssl", stts_ssl_forward(c, nullptr, n, so.data(), so.data(), wave.data(), fo.data(), fo.data(), feats.data(), ldf, ws.data(), bytes));
  return 0;
}

// One evaluation of the CFM estimator over `frames` rows per utterance (F0 / N curves of the same lengths).
static int cfm_case(stts_ctx* c, const stts_cfm_dims& cd, const std::vector<int>& frames, const char* what) {
  const int n = (int)frames.size();
  const std::vector<int32_t> off = offsets(frames);
  const long R = off[n];
  const int lda = (cd.asr_dim + 31) / 32 * 32;
  const size_t wsb = stts_cfm_workspace_bytes(c, R, n);
  std::vector<char> ws(wsb);
  auto x = buf(R * cd.feat_dim), asr = buf(R * lda), f0 = buf(R), nc = buf(R), spk = buf((size_t)n * cd.spk_dim), t = buf(n), noise = buf(R), out = buf(R * cd.feat_dim);
  stts_stub_trace_begin();
  CK(stts_cfm_estimator(c, nullptr, n, off.data(), off.data(), x.data(), cd.feat_dim, asr.data(), lda, f0.data(), nc.data(), off.data(), off.data(), spk.data(), t.data(),
                        noise.data(), out.data(), cd.feat_dim, ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s rows %7ld  workspace %8.1f MB (%zu bytes)\n", what, R, wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "cfm_estimator", stts_cfm_estimator(c, nullptr, n, off.data(), off.data(), x.data(), cd.feat_dim, asr.data(), lda, f0.data(), nc.data(), off.data(), off.data(),
                                             spk.data(), t.data(), noise.data(), out.data(), cd.feat_dim, ws.data(), bytes));
  return 0;
}

// The text aligner and RMVPE over `frames` mel frames per utterance (their queries take the real offsets).
static int aligner_case(stts_ctx* c, const stts_aligner_dims& ad, const std::vector<int>& frames, const char* what) {
  const int n = (int)frames.size();
  const std::vector<int32_t> off = offsets(frames);
  const long R = off[n];
  const size_t wsb = stts_aligner_workspace_bytes(c, n, off.data());
  std::vector<char> ws(wsb);
  auto mel = buf(R * ad.n_mels), lp = buf(R * ad.classes);
  stts_stub_trace_begin();
  CK(stts_aligner_forward(c, nullptr, n, off.data(), off.data(), mel.data(), ad.n_mels, lp.data(), ad.classes, ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s rows %7ld  workspace %8.1f MB (%zu bytes)\n", what, R, wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "aligner", stts_aligner_forward(c, nullptr, n, off.data(), off.data(), mel.data(), ad.n_mels, lp.data(), ad.classes, ws.data(), bytes));
  return 0;
}
static int rmvpe_case(stts_ctx* c, const std::vector<int>& frames, const char* what) {
  const int n = (int)frames.size();
  const std::vector<int32_t> off = offsets(frames);
  const long R = off[n];
  const size_t wsb = stts_rmvpe_workspace_bytes(c, n, off.data());
  std::vector<char> ws(wsb);
  auto mel = buf(R * 128), hidden = buf(R * 360), f0 = buf(R);
  stts_stub_trace_begin();
  CK(stts_rmvpe_forward(c, nullptr, n, off.data(), off.data(), mel.data(), 128, 0.03f, hidden.data(), f0.data(), ws.data(), wsb));
  launchtrace(what, stts_stub_trace_end());
  printf("  %-44s rows %7ld  workspace %8.1f MB (%zu bytes)\n", what, R, wsb / 1048576.0, wsb);
  REFUSE(what, wsb, "rmvpe", stts_rmvpe_forward(c, nullptr, n, off.data(), off.data(), mel.data(), 128, 0.03f, hidden.data(), f0.data(), ws.data(), bytes));
  return 0;
}

// One contraction through the test operators, traced: prec 0 = fp32 (split fp32), 1 = bf16, 2 = fp16, 3 = fp32 on the f32 matrix cores.  force as the operators take it
// (100 + t: 16-bit activation rows in the 16-bit modes); presplit: stts_op_conv1d_x3 with pre-split activation planes.  A failing call is a result, not a driver failure.
static void gemm_case(int prec, const char* what, const std::vector<int>& lens, int cin, int cout, int k, int dil, int force, bool presplit = false) {
  const int n = (int)lens.size();
  std::vector<int32_t> off(n + 1, 0);
  for (int i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
  const long R = off[n];
  const int ldx = (cin + 31) / 32 * 32, ldy = (cout + 31) / 32 * 32;
  auto x = buf(R * ldx), w = buf((size_t)cout * cin * k), b = buf(cout), y = buf(R * ldy);
  stts_stub_trace_begin();
  const int rc = (presplit || ((prec == 0 || prec == 3) && force == 0))
                     ? stts_op_conv1d_x3(nullptr, n, off.data(), off.data(), x.data(), ldx, cin, nullptr, 0, 0, w.data(), b.data(), cout, k, dil, nullptr, 0, 1.0f, presplit,
                                         y.data(), ldy, force, prec)
                     : stts_op_conv1d(nullptr, n, off.data(), off.data(), x.data(), ldx, cin, w.data(), b.data(), cout, k, dil, 0, y.data(), ldy, force, prec);
  const char* trace = stts_stub_trace_end();
  printf("gemmtrace %d %s %d : %s%s\n", prec, what, force, rc ? "error " : "", trace);
}

// The contraction cases (tests/test_asan_host.py GEMM_CASES has the same list).  The batch sizes around a threshold follow from launch_conv_gemm's rules
// (csrc/gemm_plan.hip.h), 256 CUs: see the comment of each group.
static void gemm_section() {
  const std::vector<int> ragged = {1, 63, 64, 65, 129};
  auto uni = [](int b, int len) { return std::vector<int>(b, len); };
  // every tile, forced, in each operand form it exists in (7: no such tile), 64 -> 130 channels, k = 3
  for (int t : {2, 3, 4, 5, 6, 8, 20, 21, 22, 7}) gemm_case(0, "forced", ragged, 64, 130, 3, 1, t);
  for (int t : {25, 26, 27, 28}) gemm_case(0, "forced", ragged, 64, 130, 3, 1, t, true);
  for (int t : {2, 3, 4, 5, 6, 8, 11, 13}) gemm_case(3, "forced", ragged, 64, 130, 3, 1, t);
  for (int prec : {1, 2}) {
    for (int t : {2, 3, 4, 5, 6, 8, 14, 15}) gemm_case(prec, "forced", ragged, 64, 130, 3, 1, t);
    for (int t : {2, 3, 4, 5, 6, 14, 15, 16, 17, 18, 19}) gemm_case(prec, "forced", ragged, 64, 130, 3, 1, 100 + t);
  }
  for (int prec : {0, 3}) {
    // the AUTO geometries and the two dispatch-path shapes of tests/test_hip_split_fp32_edges.py, tile left to the plan
    gemm_case(prec, "auto32x1025", ragged, 32, 1025, 1, 1, 0);
    gemm_case(prec, "auto33x130", ragged, 33, 130, 3, 3, 0);
    gemm_case(prec, "auto578x512", ragged, 578, 512, 3, 1, 0);
    gemm_case(prec, "auto1536x64", ragged, 1536, 64, 7, 3, 0);
    gemm_case(prec, "splitK", {1, 63}, 1536, 64, 7, 1, 0);
    gemm_case(prec, "tile22", uni(16, 257), 32, 2048, 1, 1, 0);
    // ... and the tiles the first two are meant to take, forced, on the same shapes
    gemm_case(prec, "auto32x1025", ragged, 32, 1025, 1, 1, 6);
    gemm_case(prec, "auto33x130", ragged, 33, 130, 3, 3, 4);
    // remainder launch: 300 x 20 rows, 128 -> 64 channels, k = 3: 12 K iterations, 300 blocks of 64 rows = 256 whole + 44 with K cut in 3 (f32 matrix cores);
    // split fp32 keeps launches whole
    gemm_case(prec, "300x20", uni(300, 20), 128, 64, 3, 1, 0);
  }
  gemm_case(0, "tile22", uni(16, 257), 32, 2048, 1, 1, 22);
  // tile 8 (f32 matrix cores): 128 x 128 blocks <= 256.  cout 128: one block per 128-row utterance
  for (int b : {256, 257}) gemm_case(3, b == 256 ? "tile8_256" : "tile8_257", uni(b, 128), 64, 128, 3, 1, 0);
  gemm_case(3, "tile8_256", uni(256, 128), 64, 128, 3, 1, 8);
  // tile 22 (split fp32): blocks of 256 rows >= 640, or >= 440 with the last chip round whole or filled to 80 % (204 of 256).  cout 128: one block per 256-row
  // utterance; 440 itself leaves 184 in its last round, so the first launch of the second kind is 460
  for (int b : {439, 440, 459, 460, 639, 640}) {
    const std::string what = "tile22_" + std::to_string(b);
    gemm_case(0, what.c_str(), uni(b, 256), 32, 128, 1, 1, 0);
    gemm_case(0, what.c_str(), uni(b, 256), 32, 128, 1, 1, 22);
  }
  for (int prec : {1, 2}) {
    // 16-bit activation rows.  Tile 15: row tiles of 256 x (npad / 128) >= 384; cout 384 (npad 384: neither tile 14 nor conv_gemm16_kernel) -> 128 utterances of 256 rows
    for (int b : {127, 128})
      for (int f : {100, 115}) gemm_case(prec, b == 127 ? "tile15_127" : "tile15_128", uni(b, 256), 64, 384, 1, 1, f);
    // tile 14: npad % 256 == 0, K iterations >= 128, row tiles of 256 x (npad / 256) >= 384; cout 1022 (npad 1024; N % 4 != 0 keeps it off conv_gemm16_kernel) -> 96
    // utterances of 256 rows, 128 channels x 33 taps = 132 iterations (95 utterances: tile 15)
    for (int b : {95, 96})
      for (int f : {100, 114, 115}) gemm_case(prec, b == 95 ? "tile14_95" : "tile14_96", uni(b, 256), 128, 1022, 33, 1, f);
    // conv_gemm16_kernel: 256 x 256 tiles >= 192; cout 256 -> 192 utterances of 256 rows
    for (int b : {191, 192})
      for (int f : {100, 119}) gemm_case(prec, b == 191 ? "gemm16_191" : "gemm16_192", uni(b, 256), 64, 256, 1, 1, f);
  }
}

// stts_op_conv1d_epi (the store contraction of the 16-bit modes with its whole epilogue, tests/test_hip_gemm16_epilogues.py): its host side - the argument
// checks against the caller's element counts, the 256-row packing of each segment, the offsets read back in capacity mode - on three launches that must go
// through and on the combinations it must refuse BEFORE anything is launched.  `epitrace <case> : [error ]<trace>`.
static void epi_case(const char* what, int prec, int tile, const std::vector<int>& caps, const std::vector<int>& lens, std::vector<std::array<int, 3>> segs, int cout,
                     int ldy, int ycol0, int ldy16, int ycol16, int ldr, int rcol0, bool ss, int ld_stat, int shrink = 0) {
  const int n = (int)lens.size();
  const bool capacity = caps != lens;
  std::vector<int32_t> host(n + 1, 0), dev(n + 1, 0);
  int max_len = 0;
  for (int i = 0; i < n; ++i) {
    host[i + 1] = host[i] + caps[i];
    dev[i + 1] = dev[i] + lens[i];
    max_len = std::max(max_len, caps[i]);
  }
  const long R = host[n];
  stts_conv_epi_args a;
  memset(&a, 0, sizeof(a));
  std::vector<std::vector<float>> keep;
  a.seg_off_host = host.data();
  a.seg_off_dev = dev.data();
  a.n_utt = n;
  a.capacity = capacity;
  a.nseg = (int)segs.size();
  a.cout = cout;
  a.alpha = 0.5f;
  a.force_tile = tile;
  a.precision = prec;
  for (int i = 0; i < a.nseg; ++i) {
    const int cin = segs[i][0], k = segs[i][1], ldx = (cin + 63) / 64 * 64;
    keep.push_back(buf(R * ldx));
    a.seg[i].x = keep.back().data();
    a.seg[i].x_elems = R * ldx;
    keep.push_back(buf((size_t)cout * cin * k));
    a.seg[i].w_host = keep.back().data();
    a.seg[i].ldx = ldx; a.seg[i].cin = cin; a.seg[i].k = k; a.seg[i].dil = segs[i][2];
  }
  auto bias = buf(cout);
  a.bias_host = bias.data();
  std::vector<float> y, r, sums, stat;
  std::vector<uint16_t> y16;
  if (ldy) { y.assign(R * ldy - shrink, 0.f); a.y = y.data(); a.y_elems = (int64_t)y.size(); a.ldy = ldy; a.ycol0 = ycol0; }
  if (ldy16) { y16.assign(R * ldy16, 0); a.y16 = y16.data(); a.y16_elems = (int64_t)y16.size(); a.ldy16 = ldy16; a.ycol16 = ycol16; }
  if (ldr) { r = buf(R * ldr); a.r = r.data(); a.r_elems = (int64_t)r.size(); a.ldr = ldr; a.rcol0 = rcol0; }
  if (ss) {
    a.ss_stride = (max_len + 31) / 32; a.ld_ss = (cout + 31) / 32 * 32;
    sums.assign((size_t)n * a.ss_stride * a.ld_ss, 0.f); a.sumsq = sums.data(); a.sumsq_elems = (int64_t)sums.size();
  }
  if (ld_stat) {
    a.stat_nchunk = (max_len + 127) / 128; a.ld_stat = ld_stat;
    stat.assign((size_t)n * a.stat_nchunk * 2 * ld_stat, 0.f); a.stat = stat.data(); a.stat_elems = (int64_t)stat.size();
  }
  stts_stub_trace_begin();
  const int rc = stts_op_conv1d_epi(nullptr, &a);
  const char* trace = stts_stub_trace_end();
  printf("epitrace %s : %s%s\n", what, rc ? "error " : "", trace);
}

static void epi_section() {
  const std::vector<int> lens = {257, 128, 5}, caps = {300, 128, 261};
  // go through: conv2 (k 3) + shortcut (k 1) with both outputs and statistics on conv_gemm16_kernel; windows, a residual and GRN sums on a 16-bit-row tile; capacity segments
  epi_case("two_segments", 1, 19, lens, lens, {{256, 3, 1}, {130, 1, 1}}, 256, 256, 0, 256, 0, 0, 0, false, 320);
  epi_case("windows_tile15", 2, 15, lens, lens, {{64, 3, 3}}, 132, 160, 8, 136, 4, 288, 12, true, 0);
  epi_case("capacity", 1, 19, caps, lens, {{64, 3, 1}}, 512, 512, 0, 512, 0, 0, 0, true, 0);
  // refused: statistics off tile 19; a Y window past its row; a Y buffer one element short; the residual of tile 19 without room for the whole channel tile;
  // a tile id without a row; real lengths beyond their capacities
  epi_case("refuse_stat_tile15", 1, 15, lens, lens, {{64, 1, 1}}, 256, 256, 0, 0, 0, 0, 0, false, 256);
  epi_case("refuse_window", 1, 19, lens, lens, {{64, 1, 1}}, 256, 256, 4, 0, 0, 0, 0, false, 0);
  epi_case("refuse_short_buffer", 1, 19, lens, lens, {{64, 1, 1}}, 256, 256, 0, 0, 0, 0, 0, false, 0, 1);
  epi_case("refuse_residual_room", 1, 19, lens, lens, {{64, 1, 1}}, 132, 160, 0, 0, 0, 136, 4, false, 0);
  epi_case("refuse_tile", 1, 7, lens, lens, {{64, 1, 1}}, 256, 256, 0, 0, 0, 0, 0, false, 0);
  epi_case("refuse_overflow", 1, 19, lens, caps, {{64, 1, 1}}, 256, 256, 0, 0, 0, 0, 0, false, 0);
}

// stts_op_adain / _wino_stat / _row_layernorm / _dwconv / _grn (the kernels between the contractions, tests/test_hip_norm_kernels.py) and stts_op_conv2d (the 2-D
// convolution, tests/test_hip_conv2d.py): per operator one call
// that goes through and one that is refused before anything is launched (a buffer one element short, or a shape outside the kernel's domain).
// `normtrace <case> : [error ]<trace>`.
template <typename Call>
static void norm_case(const char* what, Call call) {
  stts_stub_trace_begin();
  const int rc = call();
  const char* trace = stts_stub_trace_end();
  printf("normtrace %s : %s%s\n", what, rc ? "error " : "", trace);
}

static void norm_section() {
  const int n = 3;
  const std::vector<int32_t> off = {0, 130, 130, 171};  // (an utterance of zero rows in the middle)
  const long R = off[n];
  for (int refuse = 0; refuse < 2; ++refuse) {
    const char* tag = refuse ? "refuse_" : "";
    auto name = [&](const char* s) { return std::string(tag) + s; };
    {  // producer 2 + the apply through run_adain; refused: the chunk table one element short
      const int C = 130, ldx = 160, ldp = 160, nchunk = 2, ksplit = 3, ld_part = 104, Nf = 100;
      auto x = buf(R * ldx), part = buf((size_t)n * nchunk * 2 * ldp - refuse), partial = buf((size_t)ksplit * R * ld_part), bias = buf(Nf), r = buf(R * 136), gb = buf(n * 2 * C),
           snake = buf(C), y = buf(R * 192);
      stts_adain_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.n_utt = n; a.producer = 2; a.consumer = 3; a.C = C; a.ldx = ldx; a.ldp = ldp; a.nchunk = nchunk;
      a.x = x.data(); a.x_elems = (int64_t)x.size(); a.part = part.data(); a.part_elems = (int64_t)part.size();
      a.partial = partial.data(); a.partial_elems = (int64_t)partial.size(); a.ksplit = ksplit; a.slice_rows = (int)R; a.ld_part = ld_part; a.split_n = Nf;
      a.bias = bias.data(); a.bias_elems = Nf; a.split_act = 4; a.r = r.data(); a.r_elems = (int64_t)r.size(); a.ldr = 136; a.rcol0 = 8; a.split_alpha = 0.5f;
      a.gb = gb.data(); a.gb_elems = (int64_t)gb.size(); a.ld_gb = 2 * C; a.snake = snake.data(); a.snake_elems = C;
      a.y = y.data(); a.y_elems = (int64_t)y.size(); a.ldy = 192; a.rb = 256; a.out16 = 0;
      norm_case(name("adain_reduce_apply").c_str(), [&] { return stts_op_adain(nullptr, &a); });
      // the 24-row chunking with the 16-lane merge; refused: an affine table narrower than C
      auto aff = buf((size_t)n * 2 * ldx);
      a.producer = 1; a.consumer = 2; a.nchunk = 6; part = buf((size_t)n * 6 * 2 * ldp); a.part = part.data(); a.part_elems = (int64_t)part.size();
      a.aff = aff.data(); a.aff_elems = (int64_t)aff.size(); a.ld_aff = refuse ? C - 2 : ldx;
      norm_case(name("adain_lanes24").c_str(), [&] { return stts_op_adain(nullptr, &a); });
    }
    {  // refused: a statistics table with the wrong chunk count
      const int cin = 64, cout = 132, ldy = 160, ld_stat = 136, nchunk = 6;
      auto x = buf(R * cin), w = buf((size_t)cout * cin * 3), b = buf(cout), y = buf(R * ldy), stat = buf((size_t)n * nchunk * 2 * ld_stat);
      stts_wino_stat_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.n_utt = n; a.x = x.data(); a.x_elems = (int64_t)x.size(); a.ldx = cin; a.cin = cin; a.w_host = w.data(); a.bias_host = b.data(); a.cout = cout; a.k = 3;
      a.y = y.data(); a.y_elems = (int64_t)y.size(); a.ldy = ldy; a.stat = stat.data(); a.stat_elems = (int64_t)stat.size(); a.ld_stat = ld_stat; a.stat_nchunk = nchunk - refuse;
      norm_case(name("wino_stat").c_str(), [&] { return stts_op_wino_stat(nullptr, &a); });
    }
    {  // adaptive, two outputs (the second 16-bit in a window), LnIn, a device-side row count; refused: C not a multiple of 4
      const int C = refuse ? 130 : 260, ksplit = 3, ld_part = 264;
      auto partial = buf((size_t)ksplit * (R + 2) * ld_part), bias = buf(C), r = buf(R * 272), sty = buf((size_t)n * (4 * C + 8)), y0 = buf(R * (C + 8));
      std::vector<uint16_t> y1(R * (C + 40), 0);
      stts_row_layernorm_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.n_utt = n; a.n_rows = (int)R; a.n_rows_real = (int)R - 3; a.C = C; a.adaptive = 1; a.nout = 2; a.act = 3; a.eps = 1e-5f;
      a.partial = partial.data(); a.partial_elems = (int64_t)partial.size(); a.ksplit = ksplit; a.slice_rows = (int)R + 2; a.ld_part = ld_part;
      a.bias = bias.data(); a.bias_elems = C; a.in_act = 4; a.r = r.data(); a.r_elems = (int64_t)r.size(); a.ldr = 272; a.rcol0 = 4; a.in_alpha = 0.5f;
      a.out[0].y = y0.data(); a.out[0].y_elems = (int64_t)y0.size(); a.out[0].ldy = C + 8; a.out[0].g = sty.data(); a.out[0].g_elems = (int64_t)sty.size();
      a.out[0].ld_g = 4 * C + 8; a.out[0].gcol0 = 4;
      a.out[1] = a.out[0];
      a.out[1].y = y1.data(); a.out[1].y_elems = (int64_t)y1.size(); a.out[1].ldy = C + 40; a.out[1].ycol0 = 32; a.out[1].gcol0 = 4 + 2 * C; a.out[1].prec16 = 1;
      norm_case(name("row_layernorm").c_str(), [&] { return stts_op_row_layernorm(nullptr, &a); });
    }
    for (int form = 0; form < 3; ++form) {  // refused: K = 5 in the fused form, C above 512 there, an output one element short elsewhere
      const int C = (refuse && form == 1) ? 516 : 260, K = 15;
      auto x = buf(R * (C + 4)), w = buf((size_t)C * K), b = buf(C), sty = buf((size_t)n * (2 * C + 8)), y = buf(R * (C + 4) - ((refuse && form != 1) ? 5 : 0));
      stts_dwconv_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.n_utt = n; a.form = form; a.C = C; a.K = K; a.x = x.data(); a.x_elems = (int64_t)x.size(); a.ldx = C + 4; a.w_host = w.data(); a.bias_host = b.data();
      a.style = sty.data(); a.style_elems = (int64_t)sty.size(); a.ld_style = 2 * C + 8; a.gcol0 = 4; a.y = y.data(); a.y_elems = (int64_t)y.size(); a.ldy = C + 4;
      a.act = form == 0 ? 1 : 0;
      norm_case((name("dwconv_form") + std::to_string(form)).c_str(), [&] { return stts_op_dwconv(nullptr, &a); });
      if (refuse && form == 1) {
        a.C = 260; a.K = 5;
        norm_case("refuse_dwconv_form1_k5", [&] { return stts_op_dwconv(nullptr, &a); });
      }
    }
    for (int mode = 1; mode < 3; ++mode) {  // refused: a slot table with too few slots per utterance; scaled weights with kc != C
      const int C = 132, ld = 160, ss = 5, npad = 8;
      auto part = buf((size_t)n * ss * ld), gamma = buf(C), gx = buf((size_t)n * ld), xaff = buf((size_t)n * 2 * ld), w = buf((size_t)npad * C), wu = buf((size_t)n * npad * C);
      stts_grn_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.n_utt = n; a.mode = mode; a.C = C; a.part = part.data(); a.part_elems = (int64_t)part.size(); a.ld_ss = ld; a.ss_stride = (refuse && mode == 1) ? ss - 1 : ss;
      a.gamma = gamma.data(); a.gamma_elems = C; a.gx = gx.data(); a.gx_elems = (int64_t)gx.size(); a.ld_gx = ld;
      a.xaff = xaff.data(); a.xaff_elems = (int64_t)xaff.size(); a.ld_xaff = ld;
      a.w = w.data(); a.w_elems = (int64_t)w.size(); a.wu = wu.data(); a.wu_elems = (int64_t)wu.size(); a.npad = npad; a.kc = (refuse && mode == 2) ? C - 4 : C; a.prec = 1;
      norm_case((name("grn_mode") + std::to_string(mode)).c_str(), [&] { return stts_op_grn(nullptr, &a); });
    }
    {  // stts_op_conv2d: 3 x 3 on 171 x 4 positions, two segments, three grid slices and the reduce; refused: a row stride that is no multiple of 16
      const int F = 4, cin0 = 5, cin1 = 20, ld0 = refuse ? 8 : 16, ld1 = 32, cout = 33, ldy = 48;
      auto x0 = buf(R * F * ld0), x1 = buf(R * F * ld1), w = buf((size_t)cout * (cin0 + cin1) * 9), b = buf(cout), r = buf(R * F * ldy), y = buf(R * F * ldy);
      stts_conv2d_args a;
      memset(&a, 0, sizeof(a));
      a.off_in_host = a.off_in_dev = a.off_out_host = a.off_out_dev = off.data();
      a.n_utt = n; a.w_host = w.data(); a.bias_host = b.data(); a.x0 = x0.data(); a.x0_elems = (int64_t)x0.size(); a.x1 = x1.data(); a.x1_elems = (int64_t)x1.size();
      a.r = r.data(); a.r_elems = (int64_t)r.size(); a.y = y.data(); a.y_elems = (int64_t)y.size(); a.ldy = ldy;
      a.ntap = 9;
      for (int i = 0; i < 9; ++i) { a.dt[i] = i / 3 - 1; a.df[i] = i % 3 - 1; }
      a.cout = cout; a.cin0 = cin0; a.cin1 = cin1; a.ld0 = ld0; a.ld1 = ld1; a.npad = 64; a.lrelu = 1; a.chunk = 192; a.sliced = 1;
      a.Fin = a.F = F; a.up = 1; a.act = 1; a.div = 1.5f;
      norm_case(name("conv2d_sliced").c_str(), [&] { return stts_op_conv2d(nullptr, &a); });
    }
  }
}

// stts_op_cfm_elem / _rms_adaln / _rope / _cfm_small / _cfm_source (the flow-matching estimator's row kernels, tests/test_hip_cfm_kernels.py): every kind of every
// operator once, and per operator one call that is refused before anything is launched.  `cfmtrace <case> : [error ]<trace>`.
template <typename Call>
static void cfm_op_case(const char* what, Call call) {
  stts_stub_trace_begin();
  const int rc = call();
  const char* trace = stts_stub_trace_end();
  printf("cfmtrace %s : %s%s\n", what, rc ? "error " : "", trace);
}

static void cfm_ops_section() {
  const int n = 3;
  const std::vector<int32_t> off = {0, 1100, 1100, 1103}, coff = {0, 300, 300, 303}, coff0 = {0, 300, 300, 300};  // (an utterance of zero rows in the middle)
  const long R = off[n];
  {
    const int C = 1024, M = 2048;
    auto x = buf(R * 2 * M), t = buf(R * C), ada = buf((size_t)n * 3 * C), y = buf(R * M);
    stts_cfm_elem_args a;
    memset(&a, 0, sizeof(a));
    a.seg_off_host = a.seg_off_dev = off.data();
    a.n_utt = n; a.x = x.data(); a.x_elems = (int64_t)x.size(); a.t = t.data(); a.t_elems = (int64_t)t.size(); a.ada = ada.data(); a.ada_elems = (int64_t)ada.size();
    a.y = y.data(); a.y_elems = (int64_t)y.size();
    a.kind = 0; a.n = 2048 * 256 + 3;  // the capped grid
    cfm_op_case("elem_mish", [&] { return stts_op_cfm_elem(nullptr, &a); });
    a.kind = 1; a.C = M; a.n = R;
    cfm_op_case("elem_swiglu", [&] { return stts_op_cfm_elem(nullptr, &a); });
    a.kind = 2; a.C = C;
    cfm_op_case("elem_gated", [&] { return stts_op_cfm_elem(nullptr, &a); });
    a.kind = 1; a.C = 6;  // refused: four columns at a time
    cfm_op_case("refuse_elem", [&] { return stts_op_cfm_elem(nullptr, &a); });
  }
  for (int refuse = 0; refuse < 2; ++refuse) {  // refused: C above the 16 registers per lane
    const int C = refuse ? 1028 : 1024, ldx = 1060;
    auto x = buf(R * ldx), w = buf(C), ada = buf((size_t)n * 3 * C), ap = buf((size_t)n * 3 * C), t = buf(R * C), xo = buf(R * C);
    stts_rms_adaln_args a;
    memset(&a, 0, sizeof(a));
    a.seg_off_host = a.seg_off_dev = off.data();
    a.n_utt = n; a.C = C; a.ldx = a.ldy = ldx; a.x = x.data(); a.y = x.data(); a.x_elems = a.y_elems = (int64_t)x.size(); a.w = w.data(); a.w_elems = C;
    a.ada = ada.data(); a.ada_elems = (int64_t)ada.size(); a.ada_prev = ap.data(); a.ada_prev_elems = (int64_t)ap.size(); a.t = t.data(); a.t_elems = (int64_t)t.size();
    a.xout = xo.data(); a.xout_elems = (int64_t)xo.size();
    cfm_op_case(refuse ? "refuse_rms_adaln" : "rms_adaln", [&] { return stts_op_rms_adaln(nullptr, &a); });
  }
  {
    const int heads = 8, d = 64, dim = heads * d;
    auto x = buf(R * 3 * dim), freq = buf(heads * d / 2);
    stts_rope_args a;
    memset(&a, 0, sizeof(a));
    a.seg_off_host = a.seg_off_dev = off.data();
    a.n_utt = n; a.x = x.data(); a.x_elems = (int64_t)x.size(); a.freq = freq.data(); a.freq_elems = (int64_t)freq.size(); a.ldx = 3 * dim; a.col0 = 0; a.col1 = dim;
    a.kind = 0; a.heads = heads; a.kc = a.d = d;
    cfm_op_case("rope_axial", [&] { return stts_op_rope(nullptr, &a); });
    a.kind = 1; a.heads = 16; a.kc = 32; a.d = 16;
    cfm_op_case("rope_sequence", [&] { return stts_op_rope(nullptr, &a); });
    a.kc = 6; a.d = 3;  // refused: an odd number of rotated features
    cfm_op_case("refuse_rope", [&] { return stts_op_rope(nullptr, &a); });
  }
  {
    const int N = 5, K = 100, rows = 3;
    auto x = buf(rows * (K + 8)), w = buf(N * K), b = buf(N), y = buf(rows * (2 * N + 4));
    stts_cfm_small_args a;
    memset(&a, 0, sizeof(a));
    a.x = x.data(); a.x_elems = (int64_t)x.size(); a.w = w.data(); a.w_elems = (int64_t)w.size(); a.b = b.data(); a.b_elems = N; a.y = y.data(); a.y_elems = (int64_t)y.size();
    a.n_rows = rows; a.N = N; a.K = K; a.act = 1; a.ldx = K + 8; a.ldy = 2 * N + 4;
    for (int kind = 0; kind < 3; ++kind) {
      a.kind = kind;
      cfm_op_case(("small_kind" + std::to_string(kind)).c_str(), [&] { return stts_op_cfm_small(nullptr, &a); });
    }
    a.ldy = 2 * N - 1;  // refused: cos | sin do not fit a row
    cfm_op_case("refuse_small", [&] { return stts_op_cfm_small(nullptr, &a); });
  }
  for (int refuse = 0; refuse < 2; ++refuse) {  // refused: an utterance with frames and a curve of zero points
    auto f0 = buf(303), nc = buf(303), t = buf(n), noise = buf(R), har = buf(R * 32);
    stts_cfm_source_args a;
    memset(&a, 0, sizeof(a));
    a.seg_off_host = a.seg_off_dev = off.data();
    a.curve_off_host = a.curve_off_dev = refuse ? coff0.data() : coff.data();
    a.n_utt = n; a.ldh = 32; a.merge_w = 0.8f; a.f0 = f0.data(); a.f0_elems = 303; a.ncurve = nc.data(); a.ncurve_elems = 303; a.t = t.data(); a.t_elems = n;
    a.noise = noise.data(); a.noise_elems = R; a.har = har.data(); a.har_elems = (int64_t)har.size();
    cfm_op_case(refuse ? "refuse_source" : "source", [&] { return stts_op_cfm_source(nullptr, &a); });
  }
}

// The AdaptiveDecoderBlock chains (csrc/adain_block.hip.h: plan_adain_block / plan_adain_chain): `blocktrace <precision> <case> <switches> : [error ]<trace>` of one
// entry-point call under `switches` ("STTS_ADAIN_BRIDGE=0|1" or "-": the switch is read per call).  The block's other switches are read once per process:
// `asan_driver <weights> block` prints these lines alone and tests/asan/build_and_run.py starts one such process per setting.
template <typename Call>
static void block_case(int prec, const std::string& what, const char* switches, Call call) {
  unsetenv("STTS_ADAIN_BRIDGE");
  if (strcmp(switches, "-") != 0) setenv("STTS_ADAIN_BRIDGE", strchr(switches, '=') + 1, 1);
  stts_stub_trace_begin();
  const int rc = call();
  const char* trace = stts_stub_trace_end();
  unsetenv("STTS_ADAIN_BRIDGE");
  if (rc) fprintf(stderr, "blocktrace %d %s %s: %s\n", prec, what.c_str(), switches, stts_last_error());
  printf("blocktrace %d %s %s : %s%s\n", prec, what.c_str(), switches, rc ? "error " : "", trace);
}

struct Workspace {  // untouched: the host code only computes pointers into it
  char* p;
  size_t bytes;
  explicit Workspace(size_t n) : p((char*)malloc(n ? n : 1)), bytes(n) {}
  ~Workspace() { free(p); }
};

// stts_decoder_forward (frame: stts_frame_path, whose decoder may put the learned shortcuts on a side lane) over utterances of `lens` rows
static void decoder_block_case(stts_ctx* c, int prec, const std::vector<int>& lens, const std::string& what, const char* switches, bool frame = false) {
  const int n = (int)lens.size();
  const std::vector<int32_t> off = offsets(lens);
  const long R = off[n];
  Workspace ws(stts_frame_workspace_bytes(c, R, n, *std::max_element(lens.begin(), lens.end())));
  auto asr = buf(R * 128), pitch = buf(R), energy = buf(R), style = buf((size_t)n * 64), x = buf(frame ? 0 : R * 512);
  auto pn = buf(frame ? R * 128 : 0), sn = buf(frame ? R * 75 : 0), ph = buf(1), audio = buf(frame ? R * 75 : 0);
  block_case(prec, (frame ? "frame_" : "dec_") + what, switches, [&] {
    return frame ? stts_frame_path(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), pn.data(), sn.data(), ph.data(), 0,
                                   audio.data(), ws.p, ws.bytes, 0)
                 : stts_decoder_forward(c, nullptr, n, off.data(), off.data(), asr.data(), 128, pitch.data(), energy.data(), style.data(), x.data(), 512, ws.p, ws.bytes);
  });
}

static void block_section(stts_ctx* c, int prec, const Widths& wd, const stts_model_dims& d, bool phoneme_rate) {
  auto uni = [](int b, int len) { return std::vector<int>(b, len); };
  const bool f32 = prec == 0 || prec == 3;
  if (f32) {
    // fold -> Winograd: AdaIN rides in the contractions' staging up to fold_rows() = 2 500 rows
    for (int len : {300, 2500, 2501}) decoder_block_case(c, prec, {len}, "1x" + std::to_string(len), "-");
    // the bridge: 96 <= utterances x 32 slabs <= 384 and every utterance within the 256 groups of six rows (1 536) a bridge block holds
    const std::vector<std::pair<std::string, std::vector<int>>> shapes = {{"2x1300", uni(2, 1300)}, {"3x960", uni(3, 960)},   {"4x700", uni(4, 700)},
                                                                          {"12x960", uni(12, 960)}, {"13x960", uni(13, 960)}, {"1537+2x960", {1537, 960, 960}}};
    for (const auto& sh : shapes)
      for (const char* sw : {"-", "STTS_ADAIN_BRIDGE=0", "STTS_ADAIN_BRIDGE=1"}) decoder_block_case(c, prec, sh.second, sh.first, sw);
  } else {
    // 16-bit rows from rows16_threshold() = 3 840 rows, folded up to 4 096: two long utterances around both; the 110 x (30 .. 50) batch of
    // tests/test_hip_gemm16_epilogues.py (4 400 rows: conv_gemm16_kernel with the statistics from its epilogues) and its first 100 utterances (3 960 rows: folded)
    decoder_block_case(c, prec, {300}, "1x300", "-");
    for (int rows : {3839, 3840, 4096, 4097}) decoder_block_case(c, prec, {rows - rows / 2, rows / 2}, std::to_string(rows) + "rows", "-");
    std::vector<int> lens;
    for (int i = 0; i < 110; ++i) lens.push_back(30 + i % 21);
    decoder_block_case(c, prec, lens, "110utt", "-");
    lens.resize(100);
    decoder_block_case(c, prec, lens, "100utt", "-");
  }
  if (prec == 0)  // the learned shortcuts on the caller's stream below 12 000 rows, on the side lane from there
    for (int b : {12, 13})
      for (const char* sw : {"-", "STTS_ADAIN_BRIDGE=0"}) decoder_block_case(c, prec, uni(b, 960), std::to_string(b) + "x960", sw, true);
  {  // stts_op_adain_block: one block with neither Winograd scratch nor a chain (folded, then the apply pass)
    const int cin = d.inter_dim + 2, ldx = (cin + 31) / 32 * 32;
    for (const std::vector<int>& lens : {uni(1, 300), uni(2, 2049)}) {
      const int n = (int)lens.size();
      const std::vector<int32_t> off = offsets(lens);
      const long R = off[n];
      Workspace ws(stts_frame_workspace_bytes(c, R, n, lens[0]));
      auto x = buf(R * ldx), style = buf((size_t)n * 64), y = buf(R * d.dec_hidden);
      block_case(prec, "op_" + std::to_string(n) + "x" + std::to_string(lens[0]), "-", [&] {
        return stts_op_adain_block(c, nullptr, "speech_predictor.decoder.encode", n, off.data(), off.data(), x.data(), ldx, cin, d.dec_hidden, style.data(), y.data(), d.dec_hidden,
                                   ws.p, ws.bytes);
      });
    }
  }
  {  // stts_op_adain_chain: encode -> decode.0 at 300 / 301 / 500 / 501 rows with the thresholds brought down to them (fp32: fold up to 300 rows; 16-bit modes:
     // 16-bit rows from 300 rows, folded up to 500 - the window of the defaults at 3 840 .. 4 096 rows), everything offered; `blockplan` = the plan it returns
    const int cin = d.inter_dim + 2, ccat = d.dec_hidden + d.dec_residual + 2, al = f32 ? 32 : 64;
    const int ldx = (cin + al - 1) / al * al, ldcat = (ccat + al - 1) / al * al;
    for (int rows : {300, 301, 500, 501}) {
      const std::vector<int> lens = {rows - 143, 143};
      const std::vector<int32_t> off = offsets(lens);
      Workspace ws(stts_frame_workspace_bytes(c, rows, 2, lens[0]));
      auto x = buf((size_t)rows * ldx), style = buf(2 * 64), ya = buf((size_t)rows * ldcat), yb = buf((size_t)rows * d.dec_hidden);
      std::vector<uint16_t> y16((size_t)rows * ldcat);
      int32_t plan[8 + 32] = {};
      stts_adain_chain_args a;
      memset(&a, 0, sizeof(a));
      a.seg_off_host = a.seg_off_dev = off.data();
      a.x = x.data(); a.x_elems = (int64_t)x.size(); a.ldx = ldx; a.style = style.data(); a.style_elems = (int64_t)style.size();
      a.ws = ws.p; a.ws_bytes = (int64_t)ws.bytes; a.plan_out = plan; a.n_utt = 2; a.nblocks = 2;
      a.fold_rows = 300; a.fold16_rows = 500; a.rows16 = 300; a.sc_side_min_rows = 12000; a.bridge = 0;
      a.offer_wino = a.offer_stats = a.offer_rows16 = a.offer_side = a.defer = 1;
      a.blocks[0].prefix = "speech_predictor.decoder.encode"; a.blocks[0].cin = cin; a.blocks[0].cout = d.dec_hidden;
      a.blocks[0].y = ya.data(); a.blocks[0].y_elems = (int64_t)ya.size(); a.blocks[0].ldy = ldcat;
      if (!f32) { a.blocks[0].y16 = y16.data(); a.blocks[0].y16_elems = (int64_t)y16.size(); a.blocks[0].ldy16 = ldcat; }
      a.blocks[1].prefix = "speech_predictor.decoder.decode.0"; a.blocks[1].cin = ccat; a.blocks[1].cout = d.dec_hidden;
      a.blocks[1].y = yb.data(); a.blocks[1].y_elems = (int64_t)yb.size(); a.blocks[1].ldy = d.dec_hidden;
      const std::string what = "chain_" + std::to_string(rows) + "rows";
      block_case(prec, what, "-", [&] { return stts_op_adain_chain(c, nullptr, &a); });
      printf("blockplan %d %s :", prec, what.c_str());
      for (int v : plan) printf(" %d", v);
      printf("\n");
    }
  }
  if (!phoneme_rate) return;
  // the pitch/energy predictor's two branches of three blocks (always fp32 operands): three utterances of 2 500 and of 2 501 frames
  for (int last : {840, 841}) {
    const std::vector<int> toks = uni(3, 50), frames = {830, 830, last};
    const std::vector<int32_t> to = offsets(toks), fo = offsets(frames);
    const long P = to[3], T = fo[3];
    Workspace ws(stts_phoneme_workspace_bytes(c, P, T, 3, 50, last));
    std::vector<int32_t> dur(P, 1);
    auto mu = buf(P * 256), sty = buf(3 * 64), f0 = buf(T), en = buf(T);
    block_case(prec, "pe_" + std::to_string(T) + "frames", "-", [&] {
      return stts_pitch_energy_forward(c, nullptr, 3, to.data(), to.data(), fo.data(), fo.data(), dur.data(), mu.data(), 256, sty.data(), f0.data(), en.data(), nullptr, nullptr,
                                       ws.p, ws.bytes, 0);
    });
  }
  for (const std::vector<int>& frames : {std::vector<int>{240, 17, 96}, uni(2, 1300)}) {  // HubertPitchEnergyPredictor: no statistics chain
    const int n = (int)frames.size(), ldf = (wd.hubert_dim + 31) / 32 * 32;
    const std::vector<int32_t> off = offsets(frames);
    const long T = off[n];
    Workspace ws(stts_hubert_workspace_bytes(c, T, n, frames[0]));
    auto pe = buf((size_t)n * d.style_dim), feats = buf(T * ldf), f0 = buf(T), en = buf(T);
    block_case(prec, "hubert_" + std::to_string(T) + "frames", "-", [&] {
      return stts_hubert_pitch_energy_forward(c, nullptr, n, off.data(), off.data(), feats.data(), ldf, pe.data(), f0.data(), en.data(), nullptr, ws.p, ws.bytes);
    });
  }
}

struct Tensor {
  std::string name;
  int ndim;
  int64_t shape[4];
  std::vector<float> v;
};

// STTS_W_* masks of stts_finalize_weights: text-to-speech (frame path + phoneme-rate), the HuBERT pair, the mel-style pair, CfmPitchPredictor's network
static const int kTts = 255, kHubert = 512 | 1024, kMelStyle = 2048 | 4096, kPitchNet = 8192;

static int new_ctx(const stts_model_dims& d, int prec, const std::vector<Tensor>& w, stts_ctx** out) {
  CK(stts_ctx_create(&d, 0, out));
  CK(stts_set_precision(*out, prec));
  for (const Tensor& t : w) CK(stts_load_weight(*out, t.name.c_str(), t.v.data(), t.shape, t.ndim));
  return 0;
}

struct Dims {
  stts_model_dims d;
  stts_cfm_dims cd;
  stts_ssl_dims sd;
  stts_aligner_dims ad;
  stts_rmvpe_dims rd;
};

// a weight dump: the five dims structs, then (name, shape, fp32 data) per tensor
static int read_weights(const char* path, Dims& dims, std::vector<Tensor>& w) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    return 2;
  }
  if (fread(&dims.d, sizeof(dims.d), 1, f) != 1 || fread(&dims.cd, sizeof(dims.cd), 1, f) != 1 || fread(&dims.sd, sizeof(dims.sd), 1, f) != 1 ||
      fread(&dims.ad, sizeof(dims.ad), 1, f) != 1 || fread(&dims.rd, sizeof(dims.rd), 1, f) != 1)
    return 2;
  for (;;) {
    int32_t name_len = 0;
    Tensor t;
    if (fread(&name_len, 4, 1, f) != 1) break;
    t.name.assign(name_len, '\0');
    if (fread(&t.name[0], 1, name_len, f) != (size_t)name_len || fread(&t.ndim, 4, 1, f) != 1) return 2;
    int64_t count = 1;
    for (int i = 0; i < 4; ++i) t.shape[i] = 1;
    for (int i = 0; i < t.ndim; ++i) {
      if (fread(&t.shape[i], 8, 1, f) != 1) return 2;
      count *= t.shape[i];
    }
    t.v.resize(count);
    if (fread(t.v.data(), 4, count, f) != (size_t)count) return 2;
    w.push_back(std::move(t));
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: asan_driver <weights.bin> [gemm | block | <narrow weights.bin>]\n");
    return 2;
  }
  const bool block_only = argc > 2 && strcmp(argv[2], "block") == 0;
  if (!block_only) {
    gemm_section();
    if (argc > 2 && strcmp(argv[2], "gemm") == 0) return 0;
    epi_section();
    norm_section();
    cfm_ops_section();
  }
  Dims dims;
  std::vector<Tensor> w;
  if (read_weights(argv[1], dims, w)) return 2;
  const stts_model_dims& d = dims.d;
  const stts_cfm_dims& cd = dims.cd;
  const stts_ssl_dims& sd = dims.sd;
  const stts_aligner_dims& ad = dims.ad;
  stts_aligner_dims ad1 = ad;  // the same aligner with one TDNN layer (its Ffn is then layer 1: the dump has those weights too)
  ad1.n_tdnn = 1;
  auto width = [&](const char* name, int axis) {
    for (const Tensor& t : w)
      if (t.name == name) return (int)t.shape[axis];
    fprintf(stderr, "FAILED: no tensor %s in the dump\n", name);
    exit(2);
  };
  const Widths wd{width("hubert_speech_predictor.phone_encoder.phone_emb.weight", 1), width("hubert_speech_predictor.style_encoder.0.weight", 1),
                  width("pe_mel_style_encoder.shared.0.weight_orig", 0), width("cfm_pitch_predictor.asr_emb.0.weight", 1)};
  if (block_only) {  // the block cases alone, fp32 and bf16: one process per setting of the block's once-per-process switches
    for (int prec : {0, 1}) {
      stts_ctx* cb = nullptr;
      if (new_ctx(d, prec, w, &cb)) return 1;
      CK(stts_finalize_weights(cb, prec == 0 ? STTS_W_FRAME_PATH | STTS_W_PITCH_ENERGY | STTS_W_HUBERT_PE : STTS_W_DECODER));
      block_section(cb, prec, wd, d, prec == 0);
      stts_ctx_destroy(cb);
    }
    return 0;
  }
  for (int prec = 0; prec <= 3; ++prec) {  // fp32, fp16 operands (16-bit weight copies are packed too), fp32 on the f32 matrix cores
    if (prec == 1) {  // bf16: the reverse flow and the decoder alone (their kernel choices have branches of their own; the packing is fp16's with another rounding)
      stts_ctx* cf = nullptr;
      if (new_ctx(d, prec, w, &cf)) return 1;
      CK(stts_finalize_weights(cf, STTS_W_FLOW | STTS_W_DECODER));
      if (flow_section(cf, prec)) return 1;
      block_section(cf, prec, wd, d, false);
      stts_ctx_destroy(cf);
      continue;
    }
    uint64_t base = stts_stub_digest();  // (what outlives a context: the library's lazily created process-wide buffers)
    uint64_t first = 0;
    stts_ctx* c = nullptr;
    if (new_ctx(d, prec, w, &c)) return 1;
    g_prec = prec;
    auto digest = [&](const char* what) {
      first = stts_stub_digest() - base;
      printf("digest %d %s %016" PRIx64 "\n", prec, what, first);
    };
    CK(stts_finalize_weights(c, kTts));
    digest("tts");
    CK(stts_finalize_weights(c, kHubert));
    digest("hubert");
    CK(stts_finalize_weights(c, kMelStyle));
    digest("mel_style");
    CK(stts_finalize_weights(c, kPitchNet));
    digest("cfm_pitch_net");
    CK(stts_ssl_finalize(c, &sd));
    digest("ssl");
    CK(stts_cfm_finalize(c, &cd));
    digest("cfm");
    CK(stts_aligner_finalize(c, &ad));
    digest("aligner");
    CK(stts_rmvpe_finalize(c, &dims.rd));
    digest("rmvpe");
    printf("precision %d: %zu tensors loaded and packed\n", prec, w.size());
    if (flow_section(c, prec)) return 1;
    block_section(c, prec, wd, d, true);
    if (prec != 3) {  // the stage walks: once per operand width
      if (frame_case(c, std::vector<int>(8, 960), "cfg2: 8 x 3 s")) return 1;
      if (frame_case(c, {960}, "B = 1 x 3 s")) return 1;
      if (frame_case(c, {40, 131, 76, 14, 15, 16, 17, 33}, "short ragged utterances")) return 1;
      if (prec == 0) {  // (ASan shadow-poisons the 28 GB workspace reservation: once is enough)
        std::vector<int> lens;  // cfg4: 256 utterances of 0.25 - 10 s (same generator as tests/test_hip_full_size.py would give a similar spread)
        unsigned s = 4;
        for (int i = 0; i < 256; ++i) {
          s = s * 1664525u + 1013904223u;
          lens.push_back(4 * (20 + (int)((s >> 8) % 781)));
        }
        if (frame_case(c, lens, "cfg4: 256 utterances of 0.25-10 s")) return 1;
      }
      if (frame_case(c, std::vector<int>(64, 3200), "cfg5 per GPU: 64 x 10 s")) return 1;
      if (frametrace_section(c)) return 1;
      if (phoneme_case(c, std::vector<int>(64, 50), std::vector<int>(64, 240), "cfg3: 64 x 50 tokens")) return 1;
      if (phoneme_case(c, {510, 2, 160}, {1020, 4, 800}, "token-count extremes")) return 1;
      // skewed batches: the per-utterance statistics buffers grow with (utterances x longest utterance).  256 utterances, one of 4 000 frames; and 24 with
      // one of 2 400 frames, just over the row count from which the Winograd branch (and its statistics buffers) is taken
      std::vector<int> tok256(256, 3), frm256(256, 20), tok24(24, 1), frm24(24, 8), mel24(24, 65);  // (65 frames: the shortest MelStyleEncoder takes)
      tok256[0] = 500; frm256[0] = 4000; tok24[0] = 300; frm24[0] = mel24[0] = 2400;
      if (phoneme_case(c, tok256, frm256, "skew256: 1 x 4000 + 255 x 20 frames")) return 1;
      if (phoneme_case(c, tok24, frm24, "skew24: 1 x 2400 + 23 x 8 frames")) return 1;
      if (hubert_case(c, d, wd, {240, 17, 96}, "hubert: 3 utterances")) return 1;
      if (hubert_case(c, d, wd, frm256, "hubert skew256")) return 1;
      if (hubert_case(c, d, wd, frm24, "hubert skew24")) return 1;
      if (mel_case(c, wd, {300, 97, 161}, "mel: 3 utterances")) return 1;
      if (mel_case(c, wd, mel24, "mel skew24")) return 1;
      if (ssl_case(c, sd, {16000, 4000, 9001}, {50, 12, 28}, "ssl: 3 utterances")) return 1;
      if (cfm_case(c, cd, {120, 37, 64}, "cfm: 3 utterances")) return 1;
      if (cfm_case(c, cd, frm24, "cfm skew24")) return 1;
      if (aligner_case(c, ad, {300, 1, 97}, "aligner: 3 utterances")) return 1;
      if (rmvpe_case(c, {300, 17, 97}, "rmvpe: 3 utterances")) return 1;
      CK(stts_aligner_finalize(c, &ad1));
      if (aligner_case(c, ad1, {300, 1, 97}, "aligner, one tdnn layer")) return 1;
      CK(stts_aligner_finalize(c, &ad));  // (back to what the digest was taken of)
    }
    stts_ctx_destroy(c);
    // another order, a finalize that fails in the middle (a depth no weights were loaded for), then that component and the frame path again
    base = stts_stub_digest();
    if (new_ctx(d, prec, w, &c)) return 1;
    CK(stts_ssl_finalize(c, &sd));
    CK(stts_cfm_finalize(c, &cd));
    CK(stts_finalize_weights(c, kTts));
    CK(stts_finalize_weights(c, kPitchNet));
    stts_cfm_dims bad = cd;
    ++bad.depth;
    if (stts_cfm_finalize(c, &bad) == 0) {
      fprintf(stderr, "FAILED: stts_cfm_finalize accepted depth %d without its weights\n", bad.depth);
      return 1;
    }
    CK(stts_finalize_weights(c, kMelStyle));
    CK(stts_rmvpe_finalize(c, &dims.rd));
    CK(stts_finalize_weights(c, kHubert));
    CK(stts_aligner_finalize(c, &ad));
    CK(stts_cfm_finalize(c, &cd));
    CK(stts_finalize_weights(c, kTts));
    const uint64_t second = stts_stub_digest() - base;
    stts_ctx_destroy(c);
    if (second != first) {
      fprintf(stderr, "FAILED: precision %d packed %016" PRIx64 " in the second order, %016" PRIx64 " in the first\n", prec, second, first);
      return 1;
    }
    printf("order %d: the second order and the failed finalize end at the same digest %016" PRIx64 "\n", prec, second);
  }
  if (argc > 2) {  // a model whose flow is not 128 channels wide: every coupling layer as plain contractions with the gate / split-accumulate / couple epilogues
    Dims ndims;
    std::vector<Tensor> nw;
    if (read_weights(argv[2], ndims, nw)) return 2;
    const stts_model_dims& nd = ndims.d;
    for (int prec : {0, 2, 3}) {
      stts_ctx* cf = nullptr;
      if (new_ctx(nd, prec, nw, &cf)) return 1;
      CK(stts_finalize_weights(cf, STTS_W_FLOW));
      if (flow_case(cf, prec, {1, 63, 64, 65, 129}, "generic96", "-") || flow_case(cf, prec, std::vector<int>(8, 960), "generic96_8x960", "-")) return 1;
      stts_ctx_destroy(cf);
    }
  }
  printf("asan driver: all cases ran, %ld stubbed launches\n", stts_stub_launch_count());
  return 0;
}

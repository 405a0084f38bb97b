// Sanitizer driver for the posterior encoder's entry points (include/stylish_hip.h: stts_posterior_forward / stts_posterior_workspace_bytes), linked
// against the HIP stub like asan_driver.cpp and run as a stand-alone program by tests/asan/posterior_build_and_run.py:
//   posterior_driver <weights.bin>
// weights.bin: stts_model_dims, then the speech predictor's and the posterior encoder's tensors (name, shape, fp32 data).  With nothing executed on a
// device:
//   - STTS_W_POSTERIOR finalizes alone (a second context) and after STTS_W_ALL; before it the entry point is an error status
//   - the stage accepts the workspace its query sized and is refused one 256-byte unit below the least accepted size, before any launch
//   - capacity segments, mel_out without STTS_W_FLOW, an utterance too short for reflect padding and a small ld_har are refused before any launch
//   - the launch trace per STTS_POST_WN value on 1 x 960, 8 x 960 and a ragged batch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stylish_hip.h"

extern "C" long stts_stub_launch_count();
extern "C" void stts_stub_trace_begin();
extern "C" const char* stts_stub_trace_end();

#define CK(expr)                                                                              \
  do {                                                                                        \
    if ((expr) != 0) {                                                                        \
      fprintf(stderr, "FAILED %s:%d %s: %s\n", __FILE__, __LINE__, #expr, stts_last_error()); \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static std::vector<int32_t> offsets(const std::vector<int>& lens) {
  std::vector<int32_t> off(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
  return off;
}

// rc != 0 with `needle` in the message and no launch
template <typename Call>
static int rejected(const char* what, const char* needle, Call call) {
  const long before = stts_stub_launch_count();
  const int rc = call();
  const long launched = stts_stub_launch_count() - before;
  if (rc == 0 || launched != 0 || !strstr(stts_last_error(), needle)) {
    fprintf(stderr, "FAILED %s: status %d, %ld launches, \"%s\"\n", what, rc, launched, rc ? stts_last_error() : "");
    return 1;
  }
  printf("rejected %s : \"%s\", nothing launched\n", what, stts_last_error());
  return 0;
}

struct Batch {
  std::vector<int32_t> off;
  int n, rows, ld, max_len;
  std::vector<float> audio, spec, phase, style, noise, z, mean, logstd, mel, x0, wn;
  Batch(const std::vector<int>& lens, int ld_har) : off(offsets(lens)), n((int)lens.size()), rows(off.back()), ld(ld_har), max_len(0) {
    for (int v : lens) max_len = v > max_len ? v : max_len;
    audio.assign((size_t)75 * rows, 0.1f);
    spec.assign((size_t)rows * ld, 1.f);
    phase.assign((size_t)rows * ld, 0.5f);
    style.assign((size_t)n * 64, 0.2f);
    noise.assign((size_t)rows * 128, 0.3f);
    for (auto* v : {&z, &mean, &logstd, &x0, &wn}) v->assign((size_t)rows * 128, 0.f);
    mel.assign((size_t)rows * 512, 0.f);
  }
};

static int forward(stts_ctx* c, Batch& b, bool from_audio, bool with_mel, std::vector<char>& ws, size_t ws_bytes, int ld, int flags) {
  return stts_posterior_forward(c, nullptr, b.n, b.off.data(), b.off.data(), from_audio ? b.audio.data() : nullptr, b.spec.data(), b.phase.data(), ld, b.style.data(),
                                b.noise.data(), b.z.data(), b.mean.data(), b.logstd.data(), with_mel ? b.mel.data() : nullptr, 512, b.x0.data(), b.wn.data(), ws.data(),
                                ws_bytes, flags);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: posterior_driver <weights.bin>\n");
    return 2;
  }
  stts_model_dims md;
  stts_ctx *c = nullptr, *alone = nullptr;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(&md, sizeof md, 1, f) != 1) return 2;
    CK(stts_ctx_create(&md, 0, &c));
    CK(stts_ctx_create(&md, 0, &alone));
    for (;;) {
      int32_t nl = 0, nd = 0;
      if (fread(&nl, 4, 1, f) != 1) break;
      std::string name((size_t)nl, '\0');
      if (fread(&name[0], 1, (size_t)nl, f) != (size_t)nl || fread(&nd, 4, 1, f) != 1) return 2;
      std::vector<int64_t> shape((size_t)nd);
      if (fread(shape.data(), 8, (size_t)nd, f) != (size_t)nd) return 2;
      size_t n = 1;
      for (int64_t s : shape) n *= (size_t)s;
      std::vector<float> data(n);
      if (fread(data.data(), 4, n, f) != n) return 2;
      CK(stts_load_weight(c, name.c_str(), data.data(), shape.data(), nd));
      if (name.find("posterior_encoder.") != std::string::npos) CK(stts_load_weight(alone, name.c_str(), data.data(), shape.data(), nd));
    }
    fclose(f);
  }
  const int ld = stts_har_ld(c);
  Batch one({16}, ld);
  std::vector<char> none(256);
  // before the finalize: an error status, a zero query
  EXPECT(stts_posterior_workspace_bytes(c, 16, 1, 16) == 0);
  if (rejected("not finalized", "not finalized", [&] { return forward(c, one, true, false, none, none.size(), ld, 0); })) return 1;
  CK(stts_finalize_weights(alone, STTS_W_POSTERIOR));
  CK(stts_finalize_weights(c, STTS_W_ALL));
  CK(stts_finalize_weights(c, STTS_W_POSTERIOR));
  printf("finalized : STTS_W_POSTERIOR alone, and after STTS_W_ALL\n");

  // ---- the workspace walk and the refusals
  {
    const size_t q = stts_posterior_workspace_bytes(c, one.rows, one.n, one.max_len);
    EXPECT(q > 0 && stts_posterior_workspace_bytes(alone, one.rows, one.n, one.max_len) == q);
    std::vector<char> ws(q);
    CK(forward(c, one, true, true, ws, q, ld, 0));
    CK(forward(alone, one, false, false, ws, q, ld, 0));
    size_t lo = 0, hi = q / 256;  // units: lo refused, hi accepted
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      (forward(c, one, true, true, ws, mid * 256, ld, 0) == 0 ? hi : lo) = mid;
    }
    if (rejected("below the least workspace", "workspace too small", [&] { return forward(c, one, true, true, ws, (hi - 1) * 256, ld, 0); })) return 1;
    if (rejected("capacity segments", "plain segments", [&] { return forward(c, one, true, true, ws, q, ld, STTS_SEG_CAPACITY); })) return 1;
    if (rejected("mel_out without STTS_W_FLOW", "STTS_W_FLOW", [&] { return forward(alone, one, true, true, ws, q, ld, 0); })) return 1;
    Batch tiny({13}, ld);
    if (rejected("an utterance of 13 rows", "too short for reflect padding", [&] { return forward(c, tiny, true, false, ws, q, ld, 0); })) return 1;
    CK(forward(c, tiny, false, false, ws, q, ld, 0));  // (from spectra there is no padding to reflect)
    if (rejected("ld_har 1024", "ld_har", [&] { return forward(c, one, true, false, ws, q, 1024, 0); })) return 1;
  }

  // ---- launch traces per form
  const std::vector<std::pair<const char*, std::vector<int>>> batches = {{"1 x 960", {960}}, {"8 x 960", std::vector<int>(8, 960)}, {"ragged", {16, 20, 36, 68, 130, 960}}};
  for (const auto& nb : batches) {
    Batch b(nb.second, ld);
    const size_t q = stts_posterior_workspace_bytes(c, b.rows, b.n, b.max_len);
    std::vector<char> ws(q);
    for (const char* form : {"0", "16", "32", "64", ""}) {
      if (*form) setenv("STTS_POST_WN", form, 1);
      else unsetenv("STTS_POST_WN");
      stts_stub_trace_begin();
      const int rc = forward(c, b, true, true, ws, q, ld, 0);
      const std::string trace = stts_stub_trace_end();
      CK(rc);
      printf("trace %s STTS_POST_WN=%s : %s\n", nb.first, *form ? form : "unset", trace.c_str());
    }
  }
  stts_ctx_destroy(c);
  stts_ctx_destroy(alone);
  printf("posterior driver: all cases ran\n");
  return 0;
}

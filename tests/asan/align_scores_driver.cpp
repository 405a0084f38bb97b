// Sanitizer driver for the alignment, duration and difference scores' entry points (include/stylish_hip.h: stts_ctc_nll / stts_ctc_confidence_sums /
// stts_ctc_prior_sums(_workspace_bytes) / stts_val_duration_sums / stts_val_diff_sums), linked against the HIP stub like flow_stats_driver.cpp and
// run as a stand-alone program by tests/asan/align_scores_build_and_run.py:
//   align_scores_driver <dims.bin>
// dims.bin: stts_model_dims (the context the two stts_val_* entries take; no weights are needed).  With nothing executed on a device:
//   - every entry accepts a ragged batch and launches what it names, the prior sums exactly at the workspace its query sized
//   - P = 0, P = 511, T = 0, more than 64 duration classes, a bad kind, a short workspace and a null output are refused before any launch
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

// rc == 0 and the launch trace printed
template <typename Call>
static int accepted(const char* what, Call call) {
  stts_stub_trace_begin();
  const int rc = call();
  const std::string trace = stts_stub_trace_end();
  if (rc != 0) {
    fprintf(stderr, "FAILED %s: %s\n", what, stts_last_error());
    return 1;
  }
  printf("trace %s : %s\n", what, trace.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: align_scores_driver <dims.bin>\n");
    return 2;
  }
  stts_model_dims md;
  stts_ctx* c = nullptr;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(&md, sizeof md, 1, f) != 1) return 2;
    fclose(f);
    CK(stts_ctx_create(&md, 0, &c));
  }
  constexpr int V = 179, LD = 192, BLANK = 178;
  const std::vector<int> T = {1, 3, 40, 520}, P = {1, 2, 14, 510};
  const std::vector<int32_t> t_off = offsets(T), p_off = offsets(P);
  const int n = (int)T.size(), rows = t_off.back(), toks = p_off.back();
  std::vector<float> lp((size_t)rows * LD, -5.f), scores((size_t)rows, -1.f), logits((size_t)toks * 64, 0.5f), weight(64, 1.f), a((size_t)toks, 1.f), b((size_t)toks, 2.f);
  std::vector<int32_t> targets((size_t)toks, 3);
  std::vector<double> priors(V, -2.0), nll((size_t)n), sums((size_t)3 * n), log_sums(V);

  // ---- stts_ctc_nll
  auto nll_call = [&](const std::vector<int32_t>& to, const std::vector<int32_t>& po, int classes, const double* pri, double* out) {
    return stts_ctc_nll(nullptr, (int)to.size() - 1, to.data(), to.data(), po.data(), po.data(), lp.data(), LD, classes, BLANK, targets.data(), pri, 0.3, out);
  };
  if (accepted("ctc_nll ragged", [&] { return nll_call(t_off, p_off, V, nullptr, nll.data()); })) return 1;
  if (accepted("ctc_nll ragged with priors", [&] { return nll_call(t_off, p_off, V, priors.data(), nll.data()); })) return 1;
  if (rejected("ctc_nll P = 0", "tokens", [&] { return nll_call(offsets({5, 4}), offsets({2, 0}), V, nullptr, nll.data()); })) return 1;
  if (rejected("ctc_nll P = 511", "511 tokens", [&] { return nll_call(offsets({600}), offsets({511}), V, nullptr, nll.data()); })) return 1;
  if (rejected("ctc_nll T = 0", "no frames", [&] { return nll_call(offsets({5, 0}), offsets({2, 2}), V, nullptr, nll.data()); })) return 1;
  if (rejected("ctc_nll blank outside the classes", "classes", [&] { return nll_call(t_off, p_off, 100, nullptr, nll.data()); })) return 1;
  if (rejected("ctc_nll null output", "null", [&] { return nll_call(t_off, p_off, V, nullptr, nullptr); })) return 1;

  // ---- stts_ctc_confidence_sums
  if (accepted("ctc_confidence_sums ragged", [&] { return stts_ctc_confidence_sums(nullptr, n, t_off.data(), t_off.data(), scores.data(), nll.data()); })) return 1;
  {
    const std::vector<int32_t> bad = offsets({5, 0});
    if (rejected("ctc_confidence_sums T = 0", "no frames", [&] { return stts_ctc_confidence_sums(nullptr, 2, bad.data(), bad.data(), scores.data(), nll.data()); })) return 1;
  }
  if (rejected("ctc_confidence_sums null output", "null", [&] { return stts_ctc_confidence_sums(nullptr, n, t_off.data(), t_off.data(), scores.data(), nullptr); })) return 1;

  // ---- stts_ctc_prior_sums
  {
    const size_t q = stts_ctc_prior_sums_workspace_bytes(n, t_off.data(), V);
    EXPECT(q == (size_t)((rows + 63) / 64) * V * 16);
    std::vector<double> ws(q / 8);
    auto prior = [&](double* out, size_t bytes) { return stts_ctc_prior_sums(nullptr, n, t_off.data(), t_off.data(), lp.data(), LD, V, out, ws.data(), bytes); };
    if (accepted("ctc_prior_sums ragged", [&] { return prior(log_sums.data(), q); })) return 1;
    if (rejected("ctc_prior_sums one byte below the workspace", "workspace too small", [&] { return prior(log_sums.data(), q - 1); })) return 1;
    if (rejected("ctc_prior_sums null output", "null", [&] { return prior(nullptr, q); })) return 1;
    const std::vector<int32_t> bad = offsets({5, 0});
    EXPECT(stts_ctc_prior_sums_workspace_bytes(2, bad.data(), V) == 0);
    if (rejected("ctc_prior_sums T = 0", "no frames", [&] { return stts_ctc_prior_sums(nullptr, 2, bad.data(), bad.data(), lp.data(), LD, V, log_sums.data(), ws.data(), q); }))
      return 1;
  }

  // ---- stts_val_duration_sums
  auto dur = [&](const std::vector<int32_t>& po, int ld, int classes, double* out) {
    return stts_val_duration_sums(c, nullptr, (int)po.size() - 1, po.data(), po.data(), logits.data(), ld, classes, targets.data(), weight.data(), out);
  };
  if (accepted("val_duration_sums ragged, 16 classes", [&] { return dur(p_off, 16, 16, sums.data()); })) return 1;
  if (accepted("val_duration_sums ragged, 64 classes", [&] { return dur(p_off, 64, 64, sums.data()); })) return 1;
  if (rejected("val_duration_sums 65 classes", "2 to 64", [&] { return dur(offsets({3}), 80, 65, sums.data()); })) return 1;
  if (rejected("val_duration_sums P = 0", "no tokens", [&] { return dur(offsets({2, 0}), 16, 16, sums.data()); })) return 1;
  if (rejected("val_duration_sums null output", "null", [&] { return dur(p_off, 16, 16, nullptr); })) return 1;

  // ---- stts_val_diff_sums
  auto diff = [&](const std::vector<int32_t>& off, int kind, double* out) {
    return stts_val_diff_sums(c, nullptr, (int)off.size() - 1, off.data(), off.data(), a.data(), b.data(), kind, out);
  };
  if (accepted("val_diff_sums ragged, absolute", [&] { return diff(p_off, 0, nll.data()); })) return 1;
  if (accepted("val_diff_sums ragged, squared", [&] { return diff(p_off, 1, nll.data()); })) return 1;
  if (rejected("val_diff_sums kind 2", "kind must be", [&] { return diff(p_off, 2, nll.data()); })) return 1;
  if (rejected("val_diff_sums an empty utterance", "no values", [&] { return diff(offsets({2, 0}), 0, nll.data()); })) return 1;
  if (rejected("val_diff_sums null output", "null", [&] { return diff(p_off, 0, nullptr); })) return 1;

  stts_ctx_destroy(c);
  printf("align scores driver: all cases ran\n");
  return 0;
}

// Sanitizer driver for the WavLM entry points (include/stylish_hip.h: stts_wavlm_*), linked against the HIP stub like asan_driver.cpp and run as a
// stand-alone program by tests/asan/wavlm_build_and_run.py:
//   wavlm_driver <weights.bin> <buckets.bin>
// weights.bin: stts_model_dims, stts_wavlm_dims, then the narrow network's tensors (name, shape, fp32 data); buckets.bin: the reference's integer
// buckets for d = -4095 .. 4095 at the narrow configuration (int32).  Checks, with nothing executed on a device:
//   - the bucket table the library built equals the reference's integers at every distance (the clamp beyond max_bucket_distance included)
//   - both entry points accept the workspace their query sized and are refused one 256-byte unit below the least accepted size, before any launch
//   - a pair of unequal lengths and a recording below the receptive field are error statuses before any launch; the workspace query returns 0 for them
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stylish_hip.h"

extern "C" long stts_stub_launch_count();

#define CK(expr)                                                                              \
  do {                                                                                        \
    if ((expr) != 0) {                                                                        \
      fprintf(stderr, "FAILED %s:%d %s: %s\n", __FILE__, __LINE__, #expr, stts_last_error()); \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      fprintf(stderr, "FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                    \
    }                                                              \
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

template <typename Call>
static int refuse_below(const char* what, size_t query, Call call) {
  size_t lo = 0, hi = query / 256;  // units: lo refused, hi accepted
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    (call(mid * 256) == 0 ? hi : lo) = mid;
  }
  return rejected(what, "workspace too small", [&] { return call((hi - 1) * 256); });
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: wavlm_driver <weights.bin> <buckets.bin>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  stts_model_dims md;
  stts_wavlm_dims wd;
  if (fread(&md, sizeof md, 1, f) != 1 || fread(&wd, sizeof wd, 1, f) != 1) return 2;
  stts_ctx* c = nullptr;
  CK(stts_ctx_create(&md, 0, &c));
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
  }
  fclose(f);
  // before the finalize every entry point is an error status
  {
    int32_t out[3];
    EXPECT(stts_wavlm_bucket_table(c, 1, out) != 0 && strstr(stts_last_error(), "not finalized"));
  }
  CK(stts_wavlm_finalize(c, &wd));

  // ---- the bucket table against the reference's integers
  {
    const int N = 4095;
    std::vector<int32_t> want(2 * N + 1), got(2 * N + 1);
    FILE* b = fopen(argv[2], "rb");
    if (!b || fread(want.data(), 4, want.size(), b) != want.size()) return 2;
    fclose(b);
    CK(stts_wavlm_bucket_table(c, N, got.data()));
    for (int i = 0; i < 2 * N + 1; ++i)
      if (got[i] != want[i]) {
        fprintf(stderr, "FAILED bucket of distance %d: %d, the reference has %d\n", i - N, got[i], want[i]);
        return 1;
      }
    printf("buckets : %d distances equal the reference's\n", 2 * N + 1);
  }

  const int H = wd.ssl.hidden_size, NS = wd.ssl.num_hidden_layers + 1;
  // ---- states of a ragged batch
  {
    const std::vector<int> lens = {16000, 720, 400};
    const auto so = offsets(lens);
    const int n = (int)lens.size();
    long frames = 0;
    for (int v : lens) frames += stts_ssl_frames(&wd.ssl, v);
    const size_t wsb = stts_wavlm_workspace_bytes(c, n, so.data(), 0);
    EXPECT(wsb > 0);
    std::vector<float> wave((size_t)so[n], 0.25f), states((size_t)NS * frames * H), gate((size_t)frames * wd.ssl.num_attention_heads);
    std::vector<char> ws(wsb);
    const long before = stts_stub_launch_count();
    CK(stts_wavlm_forward_states(c, nullptr, n, so.data(), so.data(), wave.data(), states.data(), gate.data(), ws.data(), wsb));
    printf("states : %ld frames, workspace %zu bytes, %ld launches\n", frames, wsb, stts_stub_launch_count() - before);
    if (refuse_below("states below the least workspace", wsb, [&](size_t bytes) {
          return stts_wavlm_forward_states(c, nullptr, n, so.data(), so.data(), wave.data(), states.data(), nullptr, ws.data(), bytes);
        }))
      return 1;
  }
  // ---- the distance of two pairs
  {
    const std::vector<int> lens = {16000, 720, 16000, 720};
    const auto so = offsets(lens);
    const size_t wsb = stts_wavlm_workspace_bytes(c, 4, so.data(), 2);
    EXPECT(wsb > 0);
    std::vector<float> wave((size_t)so[4], 0.25f);
    std::vector<double> sums((size_t)2 * NS);
    std::vector<int32_t> fr(2);
    std::vector<char> ws(wsb);
    const long before = stts_stub_launch_count();
    CK(stts_wavlm_l1_sums(c, nullptr, 2, so.data(), so.data(), wave.data(), sums.data(), fr.data(), ws.data(), wsb));
    printf("l1_sums : workspace %zu bytes, %ld launches\n", wsb, stts_stub_launch_count() - before);
    if (refuse_below("l1_sums below the least workspace", wsb, [&](size_t bytes) {
          return stts_wavlm_l1_sums(c, nullptr, 2, so.data(), so.data(), wave.data(), sums.data(), fr.data(), ws.data(), bytes);
        }))
      return 1;
    // an unequal pair, a recording below the receptive field: statuses before any launch, and the query says 0
    const auto uneq = offsets({16000, 720, 16000, 721});
    EXPECT(stts_wavlm_workspace_bytes(c, 4, uneq.data(), 2) == 0);
    if (rejected("unequal pair", "unequal lengths", [&] { return stts_wavlm_l1_sums(c, nullptr, 2, uneq.data(), uneq.data(), wave.data(), sums.data(), fr.data(), ws.data(), wsb); }))
      return 1;
    const auto brief = offsets({16000, 399, 16000, 399});
    EXPECT(stts_wavlm_workspace_bytes(c, 4, brief.data(), 2) == 0);
    if (rejected("pair of 399 samples", "fewer than one frame", [&] { return stts_wavlm_l1_sums(c, nullptr, 2, brief.data(), brief.data(), wave.data(), sums.data(), fr.data(), ws.data(), wsb); }))
      return 1;
    const auto one = offsets({399});
    std::vector<float> st((size_t)NS * H);
    EXPECT(stts_wavlm_workspace_bytes(c, 1, one.data(), 0) == 0);
    if (rejected("states of 399 samples", "fewer than one frame", [&] { return stts_wavlm_forward_states(c, nullptr, 1, one.data(), one.data(), wave.data(), st.data(), nullptr, ws.data(), wsb); }))
      return 1;
    if (rejected("no pairs", "no pairs", [&] { return stts_wavlm_l1_sums(c, nullptr, 0, so.data(), so.data(), wave.data(), sums.data(), fr.data(), ws.data(), wsb); })) return 1;
  }
  stts_ctx_destroy(c);
  printf("wavlm driver: all cases ran\n");
  return 0;
}

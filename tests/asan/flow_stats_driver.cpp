// Sanitizer driver for the flow statistics' entry points (include/stylish_hip.h: stts_flow_stats_forward / stts_flow_stats_workspace_bytes /
// stts_prior_stats_forward / stts_val_kl_sums), linked against the HIP stub like posterior_driver.cpp and run as a stand-alone program by
// tests/asan/flow_stats_build_and_run.py:
//   flow_stats_driver <weights.bin>
// weights.bin: stts_model_dims, then the speech predictor's tensors (name, shape, fp32 data).  With nothing executed on a device:
//   - STTS_W_FLOW_STATS finalizes alone (a second context) and after STTS_W_ALL; before it the entry points are an error status
//   - the stage accepts exactly the workspace its query sized and is refused one byte below it, before any launch
//   - capacity segments, aliased outputs, a small ld_x, a bad KL kind and a small KL workspace are refused before any launch
//   - the launch trace per STTS_FSTAT_WN value and direction on 1 x 960, 8 x 960 and a ragged batch
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

// (vectors of 16-byte aligned storage: the entry points check the alignment of every buffer)
struct Buf {
  std::vector<float> v;
  float* p = nullptr;
  void assign(size_t n, float x) {
    v.assign(n + 4, x);
    p = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(v.data()) + 15) & ~uintptr_t(15));
  }
};

struct Batch {
  std::vector<int32_t> off;
  int n, rows, max_len;
  Buf z, mean, logstd, style, x, noise, oz, omean, ologstd;
  explicit Batch(const std::vector<int>& lens) : off(offsets(lens)), n((int)lens.size()), rows(off.back()), max_len(0) {
    for (int v : lens) max_len = v > max_len ? v : max_len;
    for (Buf* b : {&z, &mean, &logstd, &noise, &oz, &omean, &ologstd}) b->assign((size_t)rows * 128, 0.1f);
    style.assign((size_t)n * 64, 0.2f);
    x.assign((size_t)rows * 512, 0.3f);
  }
};

static int flow(stts_ctx* c, Batch& b, int reverse, std::vector<char>& ws, size_t ws_bytes, int flags, float* z_out = nullptr) {
  return stts_flow_stats_forward(c, nullptr, b.n, b.off.data(), b.off.data(), reverse, b.z.p, b.mean.p, b.logstd.p, b.style.p, z_out ? z_out : b.oz.p, b.omean.p,
                                 b.ologstd.p, ws.data(), ws_bytes, flags);
}
static int prior(stts_ctx* c, Batch& b, int ld_x, int flags) {
  return stts_prior_stats_forward(c, nullptr, b.n, b.off.data(), b.off.data(), b.x.p, ld_x, b.noise.p, b.oz.p, b.omean.p, b.ologstd.p, nullptr, 0, flags);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: flow_stats_driver <weights.bin>\n");
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
      if (name.find("speech_predictor.flow.") == 0 || name.find("speech_predictor.prior_encoder.") == 0) CK(stts_load_weight(alone, name.c_str(), data.data(), shape.data(), nd));
    }
    fclose(f);
  }
  Batch one({16, 5});
  std::vector<char> none(256);
  // before the finalize: an error status, a zero query
  EXPECT(stts_flow_stats_workspace_bytes(c, one.rows, one.n, one.max_len) == 0);
  if (rejected("flow not finalized", "not finalized", [&] { return flow(c, one, 1, none, none.size(), 0); })) return 1;
  if (rejected("prior not finalized", "not finalized", [&] { return prior(c, one, 512, 0); })) return 1;
  CK(stts_finalize_weights(alone, STTS_W_FLOW_STATS));
  CK(stts_finalize_weights(c, STTS_W_ALL));
  CK(stts_finalize_weights(c, STTS_W_FLOW_STATS));
  CK(stts_finalize_weights(c, STTS_W_FLOW_STATS));  // (again: the previous packing is released)
  printf("finalized : STTS_W_FLOW_STATS alone, and after STTS_W_ALL, and again\n");

  // ---- the workspace dry run and the refusals
  {
    const size_t q = stts_flow_stats_workspace_bytes(c, one.rows, one.n, one.max_len);
    EXPECT(q > 0 && q % 256 == 0 && stts_flow_stats_workspace_bytes(alone, one.rows, one.n, one.max_len) == q);
    std::vector<char> ws(q);
    for (int reverse = 0; reverse < 2; ++reverse) {
      CK(flow(c, one, reverse, ws, q, 0));
      CK(flow(alone, one, reverse, ws, q, 0));
    }
    CK(prior(c, one, 512, 0));
    CK(prior(alone, one, 512, 0));
    if (rejected("one byte below the workspace", "workspace too small", [&] { return flow(c, one, 0, ws, q - 1, 0); })) return 1;
    if (rejected("capacity segments", "plain segments", [&] { return flow(c, one, 0, ws, q, STTS_SEG_CAPACITY); })) return 1;
    if (rejected("capacity segments (prior)", "plain segments", [&] { return prior(c, one, 512, STTS_SEG_CAPACITY); })) return 1;
    if (rejected("an output that is an input", "other buffers", [&] { return flow(c, one, 0, ws, q, 0, one.z.p); })) return 1;
    if (rejected("reverse 2", "reverse must be", [&] { return flow(c, one, 2, ws, q, 0); })) return 1;
    if (rejected("ld_x 256", "ld_x", [&] { return prior(c, one, 256, 0); })) return 1;
    std::vector<double> sums((size_t)one.n), part((size_t)one.rows + 32);
    auto kl = [&](int kind, int C, size_t bytes) {
      return stts_val_kl_sums(c, nullptr, one.n, one.off.data(), one.off.data(), kind, one.z.p, one.logstd.p, one.mean.p, one.logstd.p, 128, C, sums.data(), part.data(), bytes);
    };
    CK(kl(0, 128, part.size() * 8));
    CK(kl(1, 128, part.size() * 8));
    if (rejected("KL kind 2", "kind must be", [&] { return kl(2, 128, part.size() * 8); })) return 1;
    if (rejected("KL width 256 in rows of 128", "ld 128 < C 256", [&] { return kl(0, 256, part.size() * 8); })) return 1;
    if (rejected("KL workspace of 8 bytes", "workspace too small", [&] { return kl(0, 128, 8); })) return 1;
  }

  // ---- launch traces per form and direction
  const std::vector<std::pair<const char*, std::vector<int>>> batches = {{"1 x 960", {960}}, {"8 x 960", std::vector<int>(8, 960)}, {"ragged", {1, 2, 17, 33, 68, 130, 960}}};
  for (const auto& nb : batches) {
    Batch b(nb.second);
    const size_t q = stts_flow_stats_workspace_bytes(c, b.rows, b.n, b.max_len);
    std::vector<char> ws(q);
    for (const char* form : {"0", "16", "32", "64", ""}) {
      if (*form) setenv("STTS_FSTAT_WN", form, 1);
      else unsetenv("STTS_FSTAT_WN");
      for (int reverse = 0; reverse < 2; ++reverse) {
        stts_stub_trace_begin();
        const int rc = flow(c, b, reverse, ws, q, 0);
        const std::string trace = stts_stub_trace_end();
        CK(rc);
        printf("trace %s reverse=%d STTS_FSTAT_WN=%s : %s\n", nb.first, reverse, *form ? form : "unset", trace.c_str());
      }
    }
  }
  stts_ctx_destroy(c);
  stts_ctx_destroy(alone);
  printf("flow stats driver: all cases ran\n");
  return 0;
}

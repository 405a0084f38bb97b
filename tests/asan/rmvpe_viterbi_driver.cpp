// Sanitizer driver for the Viterbi pitch decoding's entry points (include/stylish_hip.h: stts_rmvpe_viterbi(_workspace_bytes), stts_rmvpe_decode_at),
// linked against the HIP stub like align_scores_driver.cpp and run as a stand-alone program by tests/asan/rmvpe_viterbi_build_and_run.py:
//   rmvpe_viterbi_driver <dims.bin>
// dims.bin: stts_model_dims (the context the entries take; no weights are needed).  With nothing executed on a device:
//   - the workspace query sizes what the entry point carves: a ragged batch runs exactly at the queried size and is refused one byte below it
//   - a caller's path buffer makes the carving smaller, never larger
//   - T = 0, no utterances, null tables, null outputs, a short row stride and a bad eps are refused before any launch
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
    fprintf(stderr, "usage: rmvpe_viterbi_driver <dims.bin>\n");
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
  constexpr int LD = 368;
  const std::vector<int> T = {1, 2, 17, 64, 65, 66, 257};
  const std::vector<int32_t> off = offsets(T);
  const int n = (int)T.size(), rows = off.back();
  std::vector<float> sal((size_t)rows * LD, 0.25f), f0((size_t)rows, -1.f);
  std::vector<double> lt((size_t)360 * 59, -3.0), logp((size_t)n);
  std::vector<int32_t> path((size_t)rows, -1);
  const double lt_out = -87.33654475055310898657, eps = 1.17549435082228750797e-38;

  const size_t q = stts_rmvpe_viterbi_workspace_bytes(n, off.data());
  printf("workspace for %d rows in %d utterances: %zu bytes\n", rows, n, q);
  EXPECT(q >= (size_t)rows * 360 * 2 + (size_t)rows * 8 + (size_t)rows * 4);  // back pointers, frame sums, the path
  EXPECT(q <= (size_t)rows * 360 * 2 + (size_t)rows * 8 + (size_t)rows * 4 + 3 * 256 + 4096);
  void* ws = nullptr;
  if (posix_memalign(&ws, 256, q) != 0) return 2;  // exactly the queried size: the sanitizer sees any host access past it
  auto vit = [&](const std::vector<int32_t>& o, int ld, const double* table, double e, int32_t* p, double* l, float* f, void* w, size_t bytes) {
    return stts_rmvpe_viterbi(c, nullptr, (int)o.size() - 1, o.data(), o.data(), sal.data(), ld, table, lt_out, e, 0.03f, p, l, f, w, bytes);
  };
  if (accepted("viterbi ragged, all outputs", [&] { return vit(off, LD, lt.data(), eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (accepted("viterbi ragged, f0 only", [&] { return vit(off, LD, lt.data(), eps, nullptr, nullptr, f0.data(), ws, q); })) return 1;
  if (accepted("viterbi ragged, path only", [&] { return vit(off, LD, lt.data(), eps, path.data(), nullptr, nullptr, ws, q); })) return 1;
  if (accepted("viterbi one frame", [&] { return vit(offsets({1}), 360, lt.data(), eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  // without a caller's path the carving needs all of the query (less its slack); with one it needs less
  if (rejected("viterbi a short workspace", "workspace too small", [&] { return vit(off, LD, lt.data(), eps, nullptr, nullptr, f0.data(), ws, q - 4096 - 1); })) return 1;
  if (rejected("viterbi a tiny workspace", "workspace too small", [&] { return vit(off, LD, lt.data(), eps, path.data(), nullptr, f0.data(), ws, 1024); })) return 1;
  if (accepted("viterbi with a caller's path, workspace less the path", [&] { return vit(off, LD, lt.data(), eps, path.data(), nullptr, f0.data(), ws, q - 4096 - (size_t)rows * 4); }))
    return 1;
  if (rejected("viterbi T = 0", "no frames", [&] { return vit(offsets({5, 0, 3}), LD, lt.data(), eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (rejected("viterbi no utterances", "bad frame offsets", [&] { return vit(offsets({}), LD, lt.data(), eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (rejected("viterbi null table", "transition table", [&] { return vit(off, LD, nullptr, eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (rejected("viterbi no output", "null", [&] { return vit(off, LD, lt.data(), eps, nullptr, nullptr, nullptr, ws, q); })) return 1;
  if (rejected("viterbi null workspace", "null", [&] { return vit(off, LD, lt.data(), eps, path.data(), logp.data(), f0.data(), nullptr, q); })) return 1;
  if (rejected("viterbi ld 359", "360", [&] { return vit(off, 359, lt.data(), eps, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (rejected("viterbi eps 0", "eps", [&] { return vit(off, LD, lt.data(), 0.0, path.data(), logp.data(), f0.data(), ws, q); })) return 1;
  if (rejected("viterbi a misaligned workspace", "aligned", [&] { return vit(off, LD, lt.data(), eps, path.data(), logp.data(), f0.data(), (char*)ws + 4, q - 4); })) return 1;
  {
    const std::vector<int32_t> bad = offsets({5, 0});
    EXPECT(stts_rmvpe_viterbi_workspace_bytes(2, bad.data()) == 0);
    EXPECT(stts_rmvpe_viterbi_workspace_bytes(0, off.data()) == 0);
    EXPECT(stts_rmvpe_viterbi_workspace_bytes(1, nullptr) == 0);
    // the query grows with the rows and does not depend on how they are split
    const std::vector<int32_t> one = offsets({rows});
    EXPECT(stts_rmvpe_viterbi_workspace_bytes(1, one.data()) == q);
  }

  // ---- stts_rmvpe_decode_at
  if (accepted("decode_at", [&] { return stts_rmvpe_decode_at(c, nullptr, rows, sal.data(), LD, path.data(), 0.03f, f0.data()); })) return 1;
  if (rejected("decode_at null centres", "bad argument", [&] { return stts_rmvpe_decode_at(c, nullptr, rows, sal.data(), LD, nullptr, 0.03f, f0.data()); })) return 1;
  if (rejected("decode_at no rows", "bad argument", [&] { return stts_rmvpe_decode_at(c, nullptr, 0, sal.data(), LD, path.data(), 0.03f, f0.data()); })) return 1;

  free(ws);
  stts_ctx_destroy(c);
  printf("rmvpe viterbi driver: all cases ran\n");
  return 0;
}

// Host-only stand-in for the HIP runtime, used ONLY by the CPU sanitizer build of the library's host side
// (tests/test_asan_host.py; SURVEY.md section 5: sanitizers run on the CPU build).  "Device" memory is host memory
// (64 bytes of red zone checked by AddressSanitizer like any other heap block), copies are memcpy, kernel launches
// are counted and otherwise ignored: what runs under the sanitizers is the library's own host code - weight folding and
// packing, Winograd / fragment packing, workspace carving, launch planning - over the shapes of BASELINE's configs.
// Device allocations are zero-filled and recorded, so that stts_stub_digest() can say what the packers wrote.
// Between stts_stub_trace_begin() and stts_stub_trace_end() every launch is also written down by name (the device name
// __hipRegisterFunction was given for the host handle, demangled), grid and block: which kernels the launch planning chose, as text.
// stts_stub_trace_side_count(): how many launches of the trace went to a stream other than the null one (the driver's caller stream is null, so these
// are the launches the library put on a stream of its own).
#include <hip/hip_runtime.h>

#include <cxxabi.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

static long g_launches = 0;
extern "C" long stts_stub_launch_count() { return g_launches; }

static std::map<void*, size_t>& live_allocs() {
  static std::map<void*, size_t> m;
  return m;
}
// Sum mod 2^64, over the live hipMalloc allocations, of FNV-1a 64 of (size as 8 little-endian bytes, then the bytes): a sum, so the order
// the allocations were made in does not matter and the digest of an earlier state can be subtracted.
extern "C" uint64_t stts_stub_digest() {
  uint64_t sum = 0;
  for (const auto& kv : live_allocs()) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int i = 0; i < 8; ++i) h = (h ^ ((kv.second >> (8 * i)) & 0xff)) * 0x100000001b3ull;
    const unsigned char* b = (const unsigned char*)kv.first;
    for (size_t i = 0; i < kv.second; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    sum += h;
  }
  return sum;
}

// host handle of a kernel -> its name: demangled, without the "void stts::" in front and the parameter list behind
static std::map<const void*, std::string>& kernel_names() {
  static std::map<const void*, std::string> m;
  return m;
}
static std::string short_name(const char* mangled) {
  int status = 0;
  char* dm = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string n = status == 0 && dm ? dm : mangled;
  free(dm);
  if (!n.empty() && n.back() == ')') {  // the parameter list: from the parenthesis that matches the last one
    int depth = 0;
    for (size_t i = n.size(); i-- > 0;) {
      depth += n[i] == ')' ? 1 : n[i] == '(' ? -1 : 0;
      if (depth == 0) {
        n.erase(i);
        break;
      }
    }
  }
  for (const char* lead : {"void ", "stts::"})
    if (n.compare(0, strlen(lead), lead) == 0) n.erase(0, strlen(lead));
  return n;
}
// The trace: launches in issue order, runs of the same (kernel, grid, block) written once as `<count>x <kernel> (grid)(block)`, joined by " | "
static struct {
  bool on = false;
  std::string text, last;
  long run = 0, side = 0;
  void flush() {
    if (run) text += (text.empty() ? "" : " | ") + std::to_string(run) + "x " + last;
    run = 0;
  }
} g_trace;
extern "C" void stts_stub_trace_begin() {
  g_trace.on = true;
  g_trace.text.clear();
  g_trace.run = g_trace.side = 0;
}
extern "C" long stts_stub_trace_side_count() { return g_trace.side; }
extern "C" const char* stts_stub_trace_end() {
  g_trace.flush();
  g_trace.on = false;
  return g_trace.text.c_str();
}

extern "C" {
char stts_stub_fatbin[16] = {0};

hipError_t hipMalloc(void** p, size_t n) {
  *p = calloc(n ? n : 1, 1);
  if (!*p) return hipErrorOutOfMemory;
  live_allocs()[*p] = n;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  live_allocs().erase(p);
  free(p);
  return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < h; ++r) memcpy((char*)d + r * dp, (const char*)s + r * sp, w);
  return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
  memset(d, v, n);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
  memset(d, v, n);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) {
  memset(p, 0, sizeof(*p));
  snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950:sramecc+:xnack-");
  p->multiProcessorCount = 256;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = (hipEvent_t)malloc(8);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  free(e);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = (hipStream_t)malloc(8);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  free(s);
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* status) {
  *status = hipStreamCaptureStatusNone;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.001f;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t, hipStream_t st) {
  // what a real launch would reject
  if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x * block.y * block.z == 0 || block.x * block.y * block.z > 1024 || grid.y > 65535 || grid.z > 65535) {
    fprintf(stderr, "hip_stub: invalid launch configuration grid (%u,%u,%u) block (%u,%u,%u)\n", grid.x, grid.y, grid.z, block.x, block.y, block.z);
    abort();
  }
  ++g_launches;
  if (g_trace.on) {
    const auto it = kernel_names().find(f);
    char dims[96];
    snprintf(dims, sizeof(dims), " (%u,%u,%u)(%u,%u,%u)", grid.x, grid.y, grid.z, block.x, block.y, block.z);
    const std::string entry = (it == kernel_names().end() ? std::string("?") : it->second) + dims;
    if (entry != g_trace.last) g_trace.flush();
    g_trace.last = entry;
    ++g_trace.run;
    g_trace.side += st != nullptr;
  }
  return hipSuccess;
}
hipError_t hipExtLaunchKernel(const void* f, dim3 grid, dim3 block, void** a, size_t s, hipStream_t st, hipEvent_t, hipEvent_t, int) {
  return hipLaunchKernel(f, grid, block, a, s, st);
}
void** __hipRegisterFatBinary(const void*) {
  static void* h = nullptr;
  return &h;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  kernel_names()[host_fn] = short_name(device_name);
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
static thread_local struct {
  dim3 g, b;
  size_t s;
  hipStream_t st;
} g_cfg;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) {
  g_cfg.g = g;
  g_cfg.b = b;
  g_cfg.s = s;
  g_cfg.st = st;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* s, hipStream_t* st) {
  *g = g_cfg.g;
  *b = g_cfg.b;
  *s = g_cfg.s;
  *st = g_cfg.st;
  return hipSuccess;
}
}

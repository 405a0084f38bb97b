// RMVPE's Viterbi pitch decoding (rmvpe/utils.py:134-150, to_viterbi_f0) on the engine: the smoothest-in-time path through the 360 pitch classes under
// the reference's own objective, solved exactly in fp64, and to_local_average_f0 around that path.  Included by api.hip after rmvpe.hip.h.
//
// Objective.  eps = 2^-126.  e[t][j] = log(s[t][j] / sum_j s[t][j] + eps) in fp64, a NaN or negative salience counting as 0 and a
// frame whose sum is 0 or not finite giving p = 0; lt[i][j] = log(A[i][j] + eps) with A the row-normalised max(30 - |i - j|, 0): the host hands it over
// in the band form lt_band[j][k] = lt[j - 29 + k][j] (k < 59; -inf where the predecessor does not exist) plus the one out-of-band constant
// lt_out = log(eps).  v[0][j] = e[0][j] + log(1 / 360 + eps); c = v[t - 1][i] + lt[i][j], ptr[t][j] = the first argmax over i, v[t][j] = e[t][j] + c[ptr].
//
// The band is exact by a guard, not by assumption: every out-of-band predecessor costs the same lt_out, so with M = max_i v[t - 1][i] no predecessor
// outside the band can reach a state's band maximum unless M + lt_out >= that maximum (fp64 addition is monotone), and only then does the state scan the
// rest of the row.  The scan adds the same two numbers the full recursion adds and keeps the first-index rule over the whole row.
#pragma once

namespace stts {

constexpr int kRvVitBand = 29, kRvVitTaps = 2 * kRvVitBand + 1;  // predecessors i with |i - j| <= 29
constexpr int kRvVitThreads = 384;                               // one thread per state, six waves
constexpr int kRvVitWaves = kRvVitThreads / 64;
constexpr int kRvVitChunk = 64;                                  // back-pointer rows staged in LDS per backtracking round
constexpr int kRvVitRowVec = kRvClasses * 2 / 16;                // a back-pointer row (360 uint16) as 45 uint4

__device__ __forceinline__ double rv_vit_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double rv_vit_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a NaN or negative salience counts as 0
__device__ __forceinline__ double rv_vit_clean(float s) { return s > 0.f ? (double)s : 0.0; }

__device__ __forceinline__ double rv_vit_emission(float s, double sum, double eps) {
  const double p = (sum > 0.0 && sum <= 1.7976931348623157e308) ? rv_vit_clean(s) / sum : 0.0;
  return log(p + eps);
}

// One workgroup per utterance, thread j = state j.  The previous score row lives in LDS, double buffered, with 29 cells of -inf on each side (the band
// read needs no bounds test and neighbouring threads read neighbouring cells); one barrier per frame; the next frame's salience and sum are loaded, and
// its emission computed, before the barrier; the 59 band coefficients of a state stay in registers; the row maximum for the guard comes from wave
// reductions written next to the row.  Back pointers: uint16 rows [T][360] in `bp_all` (utterance u at row off[u]; row 0 is not used).  Backtracking
// stages kRvVitChunk pointer rows at a time in LDS and thread 0 walks them there.  sums [rows] (fp64) is scratch.  T < 1 leaves everything alone
// (the entry point refuses it).  grid n_utt, block 384.
__global__ void __launch_bounds__(kRvVitThreads) STTS_NO_PK
rv_viterbi_kernel(const float* __restrict__ S, int ld, const int* __restrict__ off, const double* __restrict__ lt_band, double lt_out, double eps, double lstart,
                  double* __restrict__ sums, unsigned short* __restrict__ bp_all, int* __restrict__ path, double* __restrict__ logp) {
  __shared__ double vb[2][kRvClasses + 2 * kRvVitBand];
  __shared__ double wm[2][kRvVitWaves];
  __shared__ int wi[kRvVitWaves];
  __shared__ uint4 chunk[kRvVitChunk * kRvVitRowVec];
  const int u = blockIdx.x, j = threadIdx.x, lane = j & 63, wv = j >> 6;
  const int t0 = off[u], T = off[u + 1] - t0;
  if (T < 1) return;
  const bool live = j < kRvClasses;
  const int jr = live ? j : 0;  // the row an idle thread reads along with the others
  const float* s0 = S + (long)t0 * ld;
  unsigned short* bp = bp_all + (long)t0 * kRvClasses;

  // every frame's sum, one wave per frame: the lanes' partial sums in lane order, then the butterfly (the same order for any batch)
  for (int t = wv; t < T; t += kRvVitWaves) {
    double a = 0.0;
    for (int i = lane; i < kRvClasses; i += 64) a += rv_vit_clean(s0[(long)t * ld + i]);
    a = rv_vit_wave_sum(a);
    if (lane == 0) sums[t0 + t] = a;
  }
  double co[kRvVitTaps];
#pragma unroll
  for (int k = 0; k < kRvVitTaps; ++k) co[k] = lt_band[jr * kRvVitTaps + k];
  if (j < kRvVitBand) {
    vb[0][j] = vb[1][j] = -INFINITY;
    vb[0][kRvVitBand + kRvClasses + j] = vb[1][kRvVitBand + kRvClasses + j] = -INFINITY;
  }
  __syncthreads();  // the sums are written (and visible to this workgroup)

  double v = live ? rv_vit_emission(s0[j], sums[t0], eps) + lstart : -INFINITY;
  if (live) vb[0][kRvVitBand + j] = v;
  {
    const double m = rv_vit_wave_max(v);
    if (lane == 0) wm[0][wv] = m;
  }
  for (int t = 1; t < T; ++t) {
    const double e = rv_vit_emission(live ? s0[(long)t * ld + j] : 0.f, sums[t0 + t], eps);  // before the barrier: no score of frame t - 1 is needed
    __syncthreads();
    const double* prev = vb[(t - 1) & 1];
    double M = wm[(t - 1) & 1][0];
#pragma unroll
    for (int w = 1; w < kRvVitWaves; ++w) M = fmax(M, wm[(t - 1) & 1][w]);
    double best = prev[jr] + co[0];
    int bi = 0;
#pragma unroll
    for (int k = 1; k < kRvVitTaps; ++k) {
      const double c = prev[jr + k] + co[k];
      if (c > best) {
        best = c;
        bi = k;
      }
    }
    bi += jr - kRvVitBand;  // a predecessor that does not exist scores -inf and is never the first maximum: v is finite
    if (M + lt_out >= best) {  // the guard: some state outside the band may reach the band's maximum
      double ob = -INFINITY;
      int oi = kRvClasses;
      for (int i = 0; i < jr - kRvVitBand; ++i) {
        const double c = prev[kRvVitBand + i] + lt_out;
        if (c > ob) {
          ob = c;
          oi = i;
        }
      }
      for (int i = jr + kRvVitBand + 1; i < kRvClasses; ++i) {
        const double c = prev[kRvVitBand + i] + lt_out;
        if (c > ob) {
          ob = c;
          oi = i;
        }
      }
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    bi = min(max(bi, 0), kRvClasses - 1);
    v = live ? e + best : -INFINITY;
    if (live) {
      vb[t & 1][kRvVitBand + j] = v;
      bp[(long)t * kRvClasses + j] = (unsigned short)bi;
    }
    const double m = rv_vit_wave_max(v);
    if (lane == 0) wm[t & 1][wv] = m;
  }

  // the end state: the first argmax of the last row
  {
    double b = v;
    int bi = live ? j : kRvClasses;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(b, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > b || (ob == b && oi < bi)) {
        b = ob;
        bi = oi;
      }
    }
    __syncthreads();  // every wave has read wm of the last frame; it is reused below
    if (lane == 0) {
      wm[0][wv] = b;
      wi[wv] = bi;
    }
  }
  __syncthreads();  // also orders this workgroup's back-pointer stores before they are read below
  int st = 0;
  if (j == 0) {
    double b = wm[0][0];
    st = wi[0];
    for (int w = 1; w < kRvVitWaves; ++w)
      if (wm[0][w] > b || (wm[0][w] == b && wi[w] < st)) {
        b = wm[0][w];
        st = wi[w];
      }
    st = min(max(st, 0), kRvClasses - 1);
    if (logp) logp[u] = b;
  }
  // backtracking: pointer rows [lo, hi) of frames 1 .. T - 1 through LDS, newest chunk first
  const uint4* bpv = reinterpret_cast<const uint4*>(bp);  // a row is 720 bytes: 45 uint4, and the utterance starts on a multiple of 720 bytes
  for (int hi = T; hi > 1;) {
    const int lo = max(1, hi - kRvVitChunk);
    const int nv = (hi - lo) * kRvVitRowVec;
    for (int i = j; i < nv; i += kRvVitThreads) chunk[i] = bpv[(long)lo * kRvVitRowVec + i];
    __syncthreads();
    if (j == 0) {
      const unsigned short* rows = reinterpret_cast<const unsigned short*>(chunk);
      for (int t = hi - 1; t >= lo; --t) {
        path[t0 + t] = st;
        st = min((int)rows[(t - lo) * kRvClasses + st], kRvClasses - 1);
      }
    }
    __syncthreads();
    hi = lo;
  }
  if (j == 0) path[t0] = st;
}

// to_local_average_f0 around a given centre: one wave per frame, the row maximum as rv_decode_kernel finds it, the average by rv_local_average.
// centre values are clamped to [0, 360).
__global__ void __launch_bounds__(256) STTS_NO_PK rv_decode_at_kernel(const float* __restrict__ S, int ld, long rows, const int* __restrict__ center, float thred,
                                                                      float* __restrict__ f0) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * ld;
  float best = -INFINITY;
  for (int i = lane; i < kRvClasses; i += 64) {
    const float v = s[i];
    if (v > best) best = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    if (ob > best) best = ob;
  }
  if (lane != 0) return;
  f0[row] = rv_local_average(s, min(max(center[row], 0), kRvClasses - 1), best, thred);
}

// salience [rows, ld >= 360] with frame offsets off -> path [rows] (optional), logp [n_utt] (optional), f0 [rows] (optional).  The workspace holds the
// back pointers, the frame sums and, where the caller wants no path, the path the decode reads.
inline int rmvpe_viterbi(hipStream_t st, int n_utt, const int* off_host, const int* off_dev, const float* sal, int ld, const double* lt_band, double lt_out, double eps,
                         float thred, int* path_out, double* logp_out, float* f0_out, Arena& ws) {
  const long rows = off_host[n_utt];
  unsigned short* bp = ws.get<unsigned short>((size_t)rows * kRvClasses);
  double* sums = ws.get<double>((size_t)rows);
  int* path = path_out ? path_out : ws.get<int>((size_t)rows);
  STTS_CHECK(ws.ok, "rmvpe_viterbi: workspace too small (stts_rmvpe_viterbi_workspace_bytes)");
  STTS_DRY_RETURN(ws);
  const double lstart = std::log(1.0 / kRvClasses + eps);
  hipLaunchKernelGGL(rv_viterbi_kernel, dim3(n_utt), dim3(kRvVitThreads), 0, st, sal, ld, off_dev, lt_band, lt_out, eps, lstart, sums, bp, path, logp_out);
  if (f0_out) hipLaunchKernelGGL(rv_decode_at_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, sal, ld, rows, path, thred, f0_out);
  STTS_HIP(hipGetLastError());
  return 0;
}

// workspace bytes for these host frame offsets: a dry run of the carving above (the larger case: no path buffer from the caller)
inline size_t rmvpe_viterbi_workspace_bytes(int n_utt, const int* off) {
  return dry_run_bytes([&](Arena a) { (void)rmvpe_viterbi(nullptr, n_utt, off, nullptr, nullptr, 0, nullptr, 0.0, 0.0, 0.f, nullptr, nullptr, nullptr, a); });
}

}  // namespace stts

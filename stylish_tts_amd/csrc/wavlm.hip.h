// WavLM (transformers.models.wavlm.modeling_wavlm, eval mode, feat_extract_norm "group", post-LN encoder) and the reference's perceptual distance over
// its hidden states (WavLMLoss, train/losses.py:408-426).  The front end and the layer body are HuBERT's (ssl.hip.h: ssl_encode); what WavLM adds is
// in the attention of every layer:
//   gate    g = gru_rel_pos_linear(x viewed [frames, heads, 64]) -> 8 values per (frame, head), summed in two groups of four, sigmoid -> (a, b);
//           gate = a * (b * gru_rel_pos_const[h] - 1) + 2                                                                  : wavlm_gate_kernel
//   bias    rel_attn_embed[bucket(key - query)][h] (layer 0's table, shared by every layer; _relative_positions_bucket: bidirectional, exact below
//           num_buckets / 4, logarithmic above, saturating by max_bucket_distance), as a table over the distance built once at finalize
//   scores  q . k / sqrt(64) + gate[query][h] * bias[h][key - query], softmax                                              : attention_mfma_kernel<64, 1, BIAS>
// and, for the distance, sum |x[u] - x[u + B]| over every hidden state of a pair of equal-length waveforms run as utterances u and u + B of one
// call, in double, in a fixed order (wavlm_l1_kernel per state, one wavlm_l1_finish_kernel per call): no state is kept or fetched.
// fp32 whatever stts_set_precision chose, packed as ssl.hip.h.  Included by api.hip after ssl.hip.h.
#pragma once

namespace stts {

constexpr int kWavlmMaxDist = 2048;  // the head's table slice (2 D + 1 floats) sits in LDS next to the attention's K / V stages
constexpr int kWavlmL1Rows = 8;      // rows of one partial sum of the distance

struct WavlmW {
  SslW ssl;
  int num_buckets = 0, max_dist = 0;
  std::vector<int> bucket;  // [2 D + 1] host: bucket of distance d at d + D
  float* bias_tab = nullptr;  // [heads][2 D + 1] device
  struct Gate {
    float* w;  // [8][64] | bias [8] | const [heads]
  } gate[kSslMaxLayers];
};

// _relative_positions_bucket of one distance.  The reference forms the logarithmic part in fp32; the same expression in double lands in the same integer
// for every |d| <= 4095 at (320, 800) and (32, 40) (tests/test_wavlm_cpu.py holds the reference's integers).
inline int wavlm_bucket(int d, int num_buckets, int max_dist) {
  const int nb = num_buckets / 2, me = nb / 2;
  const int a = d < 0 ? -d : d;
  int b = d > 0 ? nb : 0;
  if (a < me) return b + a;
  const double v = log((double)a / me) / log((double)max_dist / me) * (nb - me);
  return b + std::min((int)(me + v), nb - 1);
}

// gate[row][h] from the layer's input rows.  One thread per (row, head): its 64 channels once, eight fmaf chains in channel order against the
// weights staged in LDS (every lane reads the same weight: a broadcast).  grid ceil(rows * heads / 256)
__global__ void __launch_bounds__(256) wavlm_gate_kernel(const float* __restrict__ X, int ldx, long rows, int heads, const float* __restrict__ W, float* __restrict__ gate) {
  __shared__ float w[8 * 64 + 8];
  for (int i = threadIdx.x; i < 8 * 64 + 8; i += 256) w[i] = W[i];
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * heads) return;
  const long r = i / heads;
  const int h = (int)(i % heads);
  const float* x = X + r * ldx + h * 64;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (int c = 0; c < 64; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + c);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      acc[k] = fmaf(v.x, w[k * 64 + c], acc[k]);
      acc[k] = fmaf(v.y, w[k * 64 + c + 1], acc[k]);
      acc[k] = fmaf(v.z, w[k * 64 + c + 2], acc[k]);
      acc[k] = fmaf(v.w, w[k * 64 + c + 3], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] += w[512 + k];
  const float sa = ((acc[0] + acc[1]) + acc[2]) + acc[3], sb = ((acc[4] + acc[5]) + acc[6]) + acc[7];
  const float a = 1.0f / (1.0f + expf(-sa)), b = 1.0f / (1.0f + expf(-sb));
  gate[i] = a * (b * W[8 * 64 + 8 + h] - 1.0f) + 2.0f;
}

// part[u][blk] = sum over rows [blk * kWavlmL1Rows, ...) of utterance u of |A[row][c] - B[row][c]| (the fp32 difference, summed in double): a thread
// walks its elements in order, the block's 256 sums meet in a fixed tree.  A and B are packed alike (offsets off).  VEC: float4 loads (C and ld
// multiples of 4, 16-byte aligned bases).  grid (nblk, n_utt), block 256
template <bool VEC>
__global__ void __launch_bounds__(256) wavlm_l1_kernel(const float* __restrict__ A, const float* __restrict__ B, int ld, int C, const int* __restrict__ off, int nblk,
                                                       double* __restrict__ part) {
  __shared__ double red[256];
  const int u = blockIdx.y, blk = blockIdx.x;
  const int lo = off[u], n = off[u + 1] - lo;
  const int r0 = blk * kWavlmL1Rows;
  if (r0 >= n) return;
  const int nr = min(kWavlmL1Rows, n - r0);
  double s = 0.0;
  if constexpr (VEC) {
    const int c4 = C / 4;
    for (int i = threadIdx.x; i < nr * c4; i += 256) {
      const long e = (long)(lo + r0 + i / c4) * ld + 4 * (i % c4);
      const float4 a = *reinterpret_cast<const float4*>(A + e), b = *reinterpret_cast<const float4*>(B + e);
      s += (double)fabsf(a.x - b.x);
      s += (double)fabsf(a.y - b.y);
      s += (double)fabsf(a.z - b.z);
      s += (double)fabsf(a.w - b.w);
    }
  } else {
    for (int i = threadIdx.x; i < nr * C; i += 256) {
      const long e = (long)(lo + r0 + i / C) * ld + i % C;
      s += (double)fabsf(A[e] - B[e]);
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)u * nblk + blk] = red[0];
}

// sums[u][k] = the partial sums of state k in block order; part [n_states][n_utt][nblk].  grid ceil(n_utt * n_states / 64), block 64
__global__ void __launch_bounds__(64) wavlm_l1_finish_kernel(const double* __restrict__ part, int n_states, int n_utt, int nblk, const int* __restrict__ off,
                                                             double* __restrict__ sums, int* __restrict__ frames) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_utt * n_states) return;
  const int u = i / n_states, k = i % n_states;
  const int n = off[u + 1] - off[u];
  const int used = (n + kWavlmL1Rows - 1) / kWavlmL1Rows;
  const double* p = part + ((long)k * n_utt + u) * nblk;
  double s = 0.0;
  for (int b = 0; b < used && b < nblk; ++b) s += p[b];
  sums[(long)u * n_states + k] = s;
  if (k == 0 && frames) frames[u] = n;
}

inline int launch_wavlm_l1(hipStream_t st, const float* A, const float* B, int ld, int C, int n_utt, const int* off_dev, int max_len, double* part) {
  const int nblk = ceil_div(std::max(1, max_len), kWavlmL1Rows);
  const bool vec = C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)A | (uintptr_t)B) % 16 == 0;  // (a property of the buffers, not of the batch)
  if (vec) hipLaunchKernelGGL(wavlm_l1_kernel<true>, dim3(nblk, n_utt), dim3(256), 0, st, A, B, ld, C, off_dev, nblk, part);
  else hipLaunchKernelGGL(wavlm_l1_kernel<false>, dim3(nblk, n_utt), dim3(256), 0, st, A, B, ld, C, off_dev, nblk, part);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int finalize_wavlm(stts_ctx* c, const SslDims& d, int num_buckets, int max_dist, WavlmW* M) {
  STTS_CHECK(d.heads > 0 && d.hidden == d.heads * 64, "wavlm: hidden_size / num_attention_heads = %d, the gated attention is built for heads of 64", d.heads > 0 ? d.hidden / d.heads : 0);
  STTS_CHECK(num_buckets >= 4 && num_buckets % 4 == 0, "wavlm: num_buckets %d must be a positive multiple of 4", num_buckets);
  STTS_CHECK(max_dist > num_buckets / 4 && max_dist <= kWavlmMaxDist, "wavlm: max_bucket_distance %d outside (num_buckets / 4, %d]", max_dist, kWavlmMaxDist);
  const std::string p = "wavlm.";
  STTS_TRY(finalize_ssl(c, d, &M->ssl, p));
  M->num_buckets = num_buckets;
  M->max_dist = max_dist;
  const int D = max_dist, n = 2 * D + 1, Hn = d.heads;
  M->bucket.resize(n);
  for (int i = 0; i < n; ++i) M->bucket[i] = wavlm_bucket(i - D, num_buckets, max_dist);
  {
    STTS_GET(e, p + "encoder.layers.0.attention.rel_attn_embed.weight");
    STTS_CHECK(e->shape.size() == 2 && e->shape[0] == num_buckets && e->shape[1] == Hn, "rel_attn_embed.weight: expected [%d, %d]", num_buckets, Hn);
    std::vector<float> tab((size_t)Hn * n);
    for (int h = 0; h < Hn; ++h)
      for (int i = 0; i < n; ++i) tab[(size_t)h * n + i] = e->data[(size_t)M->bucket[i] * Hn + h];
    STTS_TRY(dev_upload(c, tab, &M->bias_tab));
  }
  for (int l = 0; l < d.layers; ++l) {
    const std::string a = p + "encoder.layers." + std::to_string(l) + ".attention.";
    STTS_GET(w, a + "gru_rel_pos_linear.weight");
    STTS_GET(b, a + "gru_rel_pos_linear.bias");
    STTS_GET(k, a + "gru_rel_pos_const");
    STTS_CHECK(w->shape.size() == 2 && w->shape[0] == 8 && w->shape[1] == 64 && (int)b->data.size() == 8, "%sgru_rel_pos_linear: expected a Linear(64, 8)", a.c_str());
    STTS_CHECK((int)k->data.size() == Hn, "%sgru_rel_pos_const: expected %d elements", a.c_str(), Hn);
    std::vector<float> g(w->data);
    g.insert(g.end(), b->data.begin(), b->data.end());
    g.insert(g.end(), k->data.begin(), k->data.end());
    STTS_TRY(dev_upload(c, g, &M->gate[l].w));
  }
  return 0;
}

// the encoder's extension (ssl.hip.h: SslPlain): gate + biased attention per layer, and what happens to every hidden state
struct WavlmExt {
  const WavlmW& M;
  float* states = nullptr;  // [layers + 1][frames, hidden]: every state copied out (stts_wavlm_forward_states)
  float* gate0 = nullptr;   // [frames, heads]: layer 0's gate (test tap)
  int pairs = 0;            // > 0: utterances u and u + pairs are a pair; their distance per state goes to part
  long pair_rows = 0;       // rows of the first `pairs` utterances (host; the second half is packed alike)
  int max_len = 0;
  float* gate = nullptr;
  double* part = nullptr;
  long F = 0;
  explicit WavlmExt(const WavlmW& m) : M(m) {}
  int nblk() const { return ceil_div(std::max(1, max_len), kWavlmL1Rows); }
  void carve(Arena& ws, long frames) {
    F = frames;
    gate = ws.get<float>((size_t)frames * M.ssl.d.heads);
    if (pairs > 0) part = ws.get<double>((size_t)(M.ssl.d.layers + 1) * pairs * nblk());
  }
  int state(hipStream_t st, int k, const float* x, const Seg& sF) {
    const int H = M.ssl.d.hidden;
    if (states) STTS_HIP(hipMemcpyAsync(states + (size_t)k * F * H, x, (size_t)F * H * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (pairs > 0) STTS_TRY(launch_wavlm_l1(st, x, x + pair_rows * H, H, H, pairs, sF.dev, max_len, part + (size_t)k * pairs * nblk()));
    return 0;
  }
  int attention(hipStream_t st, int i, const float* x, const Seg& sF, const float* qkv, int H, int heads, float* att) {
    const long n = F * heads;
    hipLaunchKernelGGL(wavlm_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, H, F, heads, M.gate[i].w, gate);
    if (i == 0 && gate0) STTS_HIP(hipMemcpyAsync(gate0, gate, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    const dim3 grid(ceil_div(sF.max_len(), kAttnMfmaQ), heads, sF.n_utt);
    const size_t shm = (size_t)(2 * M.max_dist + 1) * sizeof(float);
    // (one query tile against all the keys, never key-split: the bits must not depend on the longest utterance of the call)
    hipLaunchKernelGGL((attention_mfma_kernel<64, 1, true, AttnBias>), grid, dim3(256), shm, st, qkv, 3 * H, 0, qkv, 3 * H, H, qkv, 3 * H, 2 * H, att, H, sF.dev, sF.dev,
                       (const int*)nullptr, 0, 0.125f, AttnBias{gate, heads, M.bias_tab, M.max_dist});
    STTS_HIP(hipGetLastError());
    return 0;
  }
};

// n_utt packed waveforms -> states / gate0 (either may be null); pairs > 0: n_utt = 2 pairs, sums [pairs][layers + 1] and frames [pairs]
inline int wavlm_forward(const WavlmW& M, hipStream_t st, int n_utt, const int* samp_off_host, const int* samp_off_dev, const float* wave, float* states, float* gate0,
                         int pairs, double* sums, int* frames, Arena& ws) {
  WavlmExt ext(M);
  ext.states = states;
  ext.gate0 = gate0;
  ext.pairs = pairs;
  if (pairs > 0) {
    SslPlan P;
    ssl_plan(M.ssl.d, n_utt, samp_off_host, &P);
    ext.pair_rows = P.fr_off[pairs];
    for (int u = 0; u < pairs; ++u) ext.max_len = std::max(ext.max_len, P.fr_off[u + 1] - P.fr_off[u]);
  }
  SslPlan P;
  const float* x = nullptr;
  const int* fr_dev = nullptr;
  STTS_TRY(ssl_encode(M.ssl, st, n_utt, samp_off_host, samp_off_dev, wave, nullptr, ws, ext, P, &x, &fr_dev));
  if (!x) return 0;  // a dry run
  if (pairs > 0) {
    const int ns = M.ssl.d.layers + 1;
    hipLaunchKernelGGL(wavlm_l1_finish_kernel, dim3(ceil_div(pairs * ns, 64)), dim3(64), 0, st, ext.part, ns, pairs, ext.nblk(), fr_dev, sums, frames);
    STTS_HIP(hipGetLastError());
  }
  return 0;
}

inline size_t wavlm_workspace_bytes(const WavlmW& M, int n_utt, const int* samp_off, int pairs) {
  return dry_run_bytes([&](Arena a) { (void)wavlm_forward(M, nullptr, n_utt, samp_off, nullptr, nullptr, nullptr, nullptr, pairs, nullptr, nullptr, a); });
}

}  // namespace stts

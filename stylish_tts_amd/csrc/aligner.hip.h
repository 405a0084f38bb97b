// The text aligner (train/models/text_aligner.py: tdnn_blstm_ctc_model, CTCModel.forward in eval mode) and the CTC forced alignment behind it
// (train/dataprep/align_text.py:159-210, torch_align) on packed rows of normalised log-mel [sum T, n_mels].
//   TDNN layers   Conv1d (k odd, stride 1, dilation 1, "same" zero padding at the utterance's own edges) + ReLU in the contraction's epilogue; the
//                 BatchNorm1d(affine = False) that FOLLOWS the ReLU is a per-channel scale / shift folded in double at finalize and applied where
//                 the next contraction stages its input tile (GemmArgs::xaff, slope 1): rows beyond an utterance stay zero, which is the reference's
//                 length mask before every TDNN layer.  The last TDNN layer's BatchNorm is applied by one row pass (aligner_affine_rows_kernel):
//                 its output is both the Ffn's input and its skip operand                                        : conv_gemm_f32
//   Ffn           n x (Linear + ReLU), the skip add in the last epilogue                                        : conv_gemm_f32
//   output layer  Linear hidden -> classes, then log_softmax over the classes, one wave per row                 : conv_gemm_f32, aligner_log_softmax_kernel
//   alignment     Viterbi over the 2 P + 1 CTC states, one workgroup per utterance                              : ctc_viterbi_kernel
//   durations     per-token frame counts and torch_align's boundary probabilities from a label path             : ctc_durations_kernel
//   likelihood    the CTC negative log-likelihood (the same states over the log semiring, fp64), optional priors  : ctc_forward_kernel
//   sums          sum of exp(path log-probs) per utterance; per-class logsumexp over the batch's frames           : ctc_confidence_kernel, ctc_prior_*_kernel
// Everything is fp32 whatever stts_set_precision chose.  The contractions run the split-fp32 form (the f32 matrix cores on an STTS_PREC_F32_NATIVE
// engine), always on the 128 x 128 tile whose 16 waves are 8 positions x 2 K-groups and never cut over blocks - ssl.hip.h gives the reasons: two
// accumulator chains of K / 2 round less than one of K (K = 1920 in the TDNN layers), and one tile for every call makes an utterance's rows the
// same bit for bit alone and packed with others.
//
// The tie rule of the alignment, fixed: among the predecessors of a state the SMALLER jump wins (stay, then +1, then +2: a candidate replaces the
// best only when strictly greater); at the end the final blank wins over the last token unless the token's score is strictly greater.
// Included by api.hip after rmvpe.hip.h.
#pragma once

namespace stts {

constexpr int kAlMaxTdnn = 4;
constexpr int kAlMaxFfn = 8;
constexpr int kCtcMaxTokens = 510;  // the tokeniser's limit: 1021 states, one thread each
constexpr int kCtcThreads = 1024;

struct AlDims {
  int n_mels = 0, hidden = 0, classes = 0, n_tdnn = 0, ffn_layers = 0;
  int tdnn_k[kAlMaxTdnn] = {};
};

struct AlW {
  bool ready = false;
  AlDims d;
  PackedConv tdnn[kAlMaxTdnn], ffn[kAlMaxFfn], out;
  float* bn = nullptr;  // [n_tdnn][2][hidden]: scale = 1 / sqrt(running_var + eps), shift = -running_mean * scale
};

// ------------------------------------------------------------------------------------------------ row kernels
// mel rows [R, ld_in] -> [R, ld_out] with the pad columns zeroed (the first contraction reads whole 32-channel chunks), and the BatchNorm tables of
// the TDNN layers that feed another TDNN layer repeated per utterance in the layout GemmArgs::xaff wants: tab[l][u][2][H].  One launch.
__global__ void __launch_bounds__(256) aligner_prepare_kernel(const float* __restrict__ X, int ld_in, int C, const int* __restrict__ seg_off, int n_utt,
                                                              float* __restrict__ Y, int ld_out, const float* __restrict__ bn, int n_tab, int H, float* __restrict__ tab) {
  const long R = seg_off[n_utt];
  const long total = R * ld_out, step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const long r = i / ld_out;
    const int c = (int)(i - r * ld_out);
    Y[i] = c < C ? X[r * ld_in + c] : 0.f;
  }
  const long tt = (long)n_tab * n_utt * 2 * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tt; i += step) {
    const long l = i / ((long)n_utt * 2 * H);
    const int j = (int)(i % (2 * H));
    tab[i] = bn[l * 2 * H + j];
  }
}

// y = x * scale[c] + shift[c] over R rows of H channels (H % 4 == 0); Y may be X
__global__ void __launch_bounds__(256) aligner_affine_rows_kernel(const float* X, const int* __restrict__ seg_off, int n_utt, int H, const float* __restrict__ bn,
                                                                  float* Y) {
  const long total = (long)seg_off[n_utt] * (H / 4);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % (H / 4)) * 4;
    const float4 v = reinterpret_cast<const float4*>(X)[i];
    const float4 sc = *reinterpret_cast<const float4*>(bn + c), sh = *reinterpret_cast<const float4*>(bn + H + c);
    float4 y;
    y.x = v.x * sc.x + sh.x; y.y = v.y * sc.y + sh.y; y.z = v.z * sc.z + sh.z; y.w = v.w * sc.w + sh.w;
    reinterpret_cast<float4*>(Y)[i] = y;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// log_softmax over V <= 256 classes: one wave per row, four values per lane in registers; x - max - log(sum exp(x - max)) as torch forms it.
// Optional raw copy of the logits (test tap).  grid ceil(R / 4), block 256.
__global__ void __launch_bounds__(256) aligner_log_softmax_kernel(const float* __restrict__ X, int ldx, const int* __restrict__ seg_off, int n_utt, int V,
                                                                  float* __restrict__ Y, int ldy, float* __restrict__ raw) {
  const long R = seg_off[n_utt];
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const float* x = X + r * ldx;
  float v[4], m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    v[i] = c < V ? x[c] : -INFINITY;
    m = fmaxf(m, v[i]);
    if (raw && c < V) raw[r * V + c] = v[i];
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + i * 64 < V) s += expf(v[i] - m);
  const float lse = logf(wave_sum(s));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    if (c < V) Y[r * ldy + c] = (v[i] - m) - lse;
  }
}

// ------------------------------------------------------------------------------------------------ forced alignment
// bytes of back pointers in front of utterance u: sum of T * (2 P + 1) over the utterances before it (n_utt is small; every thread runs the same loop)
__device__ __forceinline__ long ctc_bp_offset(const int* __restrict__ t_off, const int* __restrict__ p_off, int u) {
  long o = 0;
  for (int i = 0; i < u; ++i) o += (long)(t_off[i + 1] - t_off[i]) * (2 * (p_off[i + 1] - p_off[i]) + 1);
  return o;
}

// Viterbi path of one utterance.  States 0 .. 2 P: even = blank, odd s = token (s - 1) / 2.  Thread s owns state s; the score row of the previous
// frame lives in LDS, double buffered, one barrier per frame; the emission of the next frame is loaded before the barrier.  Back pointers (the jump
// 0 / 1 / 2) go to `bp` [T][S] bytes; thread 0 walks them backwards and writes the label of every frame.  An utterance whose P is outside
// [1, kCtcMaxTokens] or whose T < 1 is left alone (the entry point refuses it); an infeasible (T, targets) pair walks -inf scores and still
// stays inside its rows.  Token ids are clamped to [0, V - 1].  grid n_utt, block 1024.
__global__ void __launch_bounds__(kCtcThreads) ctc_viterbi_kernel(const float* __restrict__ lp, int ld, int V, int blank, const int* __restrict__ t_off,
                                                                  const int* __restrict__ p_off, const int* __restrict__ targets, unsigned char* __restrict__ bp_all,
                                                                  int* __restrict__ path) {
  __shared__ float sc[2][kCtcThreads];
  __shared__ int tok[kCtcMaxTokens + 2];
  const int u = blockIdx.x, s = threadIdx.x;
  const int t0 = t_off[u], T = t_off[u + 1] - t0, q0 = p_off[u], P = p_off[u + 1] - q0;
  if (P < 1 || P > kCtcMaxTokens || T < 1) return;
  const int S = 2 * P + 1;
  unsigned char* bp = bp_all + ctc_bp_offset(t_off, p_off, u);
  for (int i = s; i < P; i += kCtcThreads) tok[i] = min(max(targets[q0 + i], 0), V - 1);
  __syncthreads();
  const bool live = s < S;
  const int label = (live && (s & 1)) ? tok[s >> 1] : blank;
  const bool skip = live && (s & 1) && s >= 3 && tok[s >> 1] != tok[(s >> 1) - 1];
  const float* col = lp + (long)t0 * ld + label;
  float e = live ? col[0] : 0.f;
  sc[0][s] = (live && s < 2) ? e : -INFINITY;
  if (live) bp[s] = 0;
  for (int t = 1; t < T; ++t) {
    e = live ? col[(long)t * ld] : 0.f;  // in flight across the barrier
    __syncthreads();
    const float* prev = sc[(t - 1) & 1];
    float best = prev[s];
    int j = 0;
    if (s >= 1) {
      const float a = prev[s - 1];
      if (a > best) { best = a; j = 1; }
    }
    if (skip) {
      const float a = prev[s - 2];
      if (a > best) { best = a; j = 2; }
    }
    sc[t & 1][s] = live ? best + e : -INFINITY;
    if (live) bp[(long)t * S + s] = (unsigned char)j;
  }
  __syncthreads();  // also orders this block's back-pointer stores before thread 0 reads them
  if (s == 0) {
    const float* last = sc[(T - 1) & 1];
    int st = S - 1;                                   // the final blank wins a tie
    if (last[S - 2] > last[S - 1]) st = S - 2;
    for (int t = T - 1; t >= 0; --t) {
      path[t0 + t] = (st & 1) ? tok[st >> 1] : blank;
      st -= bp[(long)t * S + st];
      st = max(st, 0);
    }
  }
}

// torch_align's post-processing of a label path (align_text.py:174-210) for one utterance: a frame starts token k + 1 when its label is no blank and
// the frame before it was blank or carried another label; dur[p] = frames of token p and of the blanks after it, the blanks in front of the first
// token counted to token 0 (the reference's loop trips its own assert on such a path: the one stated deviation).  left[i] / right[i] for i < P - 1
// from the two rows at index = dur[0] + .. + dur[i]: fp32 sums of two log-probs, exp and the quotient in double, rounded once, as the reference's
// math.exp on fp32 tensors does; the last entry is 0.  scores[t] = lp[t][path[t]].  Token indices are clamped to [0, P - 1], labels to [0, V - 1] and
// row indices to the utterance: any path stays in bounds.  grid n_utt, block 1024.
__global__ void __launch_bounds__(kCtcThreads) ctc_durations_kernel(const float* __restrict__ lp, int ld, int V, int blank, const int* __restrict__ t_off,
                                                                    const int* __restrict__ p_off, const int* __restrict__ targets, const int* __restrict__ path,
                                                                    float* __restrict__ scores, int* __restrict__ dur, float* __restrict__ left, float* __restrict__ right) {
  __shared__ int cnt[kCtcThreads];
  __shared__ int d[kCtcMaxTokens + 2];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int t0 = t_off[u], T = t_off[u + 1] - t0, q0 = p_off[u], P = p_off[u + 1] - q0;
  if (P < 1 || P > kCtcMaxTokens || T < 1) return;
  const int per = (T + kCtcThreads - 1) / kCtcThreads;
  const int lo = min(tid * per, T), hi = min(lo + per, T);
  auto starts = [&](int t) {
    const int a = path[t0 + t];
    if (a == blank) return false;
    return t == 0 || path[t0 + t - 1] != a;  // (a blank before it differs from a too)
  };
  int n = 0;
  for (int t = lo; t < hi; ++t) n += starts(t);
  cnt[tid] = n;
  for (int i = tid; i < P; i += kCtcThreads) d[i] = 0;
  __syncthreads();
  if (tid == 0) {  // exclusive scan of 1024 counts
    int acc = 0;
    for (int i = 0; i < kCtcThreads; ++i) { const int c = cnt[i]; cnt[i] = acc; acc += c; }
  }
  __syncthreads();
  int k = cnt[tid] - 1;  // token index of the frame before this chunk (-1: none yet)
  for (int t = lo; t < hi; ++t) {
    k += starts(t);
    atomicAdd(&d[min(max(k, 0), P - 1)], 1);
    const int a = min(max(path[t0 + t], 0), V - 1);
    scores[t0 + t] = lp[(long)(t0 + t) * ld + a];
  }
  __syncthreads();
  if (tid == 0) {  // dur out, inclusive sums in place
    int acc = 0;
    for (int i = 0; i < P; ++i) { dur[q0 + i] = d[i]; acc += d[i]; d[i] = acc; }
  }
  __syncthreads();
  for (int i = tid; i < P; i += kCtcThreads) {
    float l = 0.f, r = 0.f;
    if (i < P - 1 && T >= 2) {
      const int idx = min(max(d[i], 1), T - 1);
      const int lt = min(max(targets[q0 + i], 0), V - 1), rt = min(max(targets[q0 + i + 1], 0), V - 1);
      const float* r0 = lp + (long)(t0 + idx - 1) * ld;
      const float* r1 = lp + (long)(t0 + idx) * ld;
      const double lpb = exp((double)(r0[lt] + r1[lt])), sp = exp((double)(r0[lt] + r1[rt])), rp = exp((double)(r0[rt] + r1[rt]));
      const double den = lpb + sp + rp;
      l = (float)(lpb / den);
      r = (float)(rp / den);
    }
    left[q0 + i] = l;
    right[q0 + i] = r;
  }
}

// ------------------------------------------------------------------------------------------------ CTC likelihood and the sums beside it
// log(exp(a) + exp(b) + exp(c)) in fp64: m + log(sum exp(x - m)) with m the largest; -inf when all three are -inf (no inf - inf is ever formed:
// a - m with a = -inf and m finite is -inf, whose exp is 0).
__device__ __forceinline__ double ctc_lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// CTC negative log-likelihood of one utterance: the Viterbi kernel's skeleton (thread s owns state s, the previous frame's row in LDS, double
// buffered, one barrier per frame, the next frame's emission gathered before the barrier) over the log semiring, in fp64:
//   alpha[t][s] = lse(alpha[t-1][s], alpha[t-1][s-1], alpha[t-1][s-2] if the jump is allowed) + e[t][s]
//   e[t][s] = lp[t][label(s)] - prior_scale * log_priors[label(s)]   (log_priors may be null)
//   nll[u] = -lse(alpha[T-1][2P], alpha[T-1][2P-1]); +inf when no path exists.
// No back pointers, no workspace.  Token ids are clamped to [0, V - 1]; a thread past the utterance's states only meets the barriers.  An
// utterance whose P is outside [1, kCtcMaxTokens] or whose T < 1 is left alone (the entry point refuses it).  grid n_utt, block 1024.
__global__ void __launch_bounds__(kCtcThreads) STTS_NO_PK ctc_forward_kernel(const float* __restrict__ lp, int ld, int V, int blank, const int* __restrict__ t_off,
                                                                             const int* __restrict__ p_off, const int* __restrict__ targets,
                                                                             const double* __restrict__ log_priors, double prior_scale, double* __restrict__ nll) {
  __shared__ double al[2][kCtcThreads];
  __shared__ int tok[kCtcMaxTokens + 2];
  const int u = blockIdx.x, s = threadIdx.x;
  const int t0 = t_off[u], T = t_off[u + 1] - t0, q0 = p_off[u], P = p_off[u + 1] - q0;
  if (P < 1 || P > kCtcMaxTokens || T < 1) return;
  const int S = 2 * P + 1;
  for (int i = s; i < P; i += kCtcThreads) tok[i] = min(max(targets[q0 + i], 0), V - 1);
  __syncthreads();
  const bool live = s < S;
  const int label = (live && (s & 1)) ? tok[s >> 1] : blank;
  const bool skip = live && (s & 1) && s >= 3 && tok[s >> 1] != tok[(s >> 1) - 1];
  const double pc = log_priors ? prior_scale * log_priors[label] : 0.0;
  const float* col = lp + (long)t0 * ld + label;
  double e = live ? (double)col[0] - pc : 0.0;
  al[0][s] = (live && s < 2) ? e : -INFINITY;
  for (int t = 1; t < T; ++t) {
    e = live ? (double)col[(long)t * ld] - pc : 0.0;  // in flight across the barrier
    __syncthreads();
    if (live) {
      const double* prev = al[(t - 1) & 1];
      const double a = ctc_lse3(prev[s], s >= 1 ? prev[s - 1] : -INFINITY, skip ? prev[s - 2] : -INFINITY);
      al[t & 1][s] = a == -INFINITY ? -INFINITY : a + e;
    }
  }
  __syncthreads();
  if (s == 0) {
    const double* last = al[(T - 1) & 1];
    const double a = ctc_lse3(last[S - 1], last[S - 2], -INFINITY);
    nll[u] = a == -INFINITY ? INFINITY : -a;
  }
}

// sums[u] = sum over the utterance's frames of exp(scores[t]) in fp64 (scores: the path log-probs ctc_durations_kernel writes): thread i takes
// frames i, i + 256, ... in order, a fixed tree joins the 256 sums.  grid n_utt, block 256.
__global__ void __launch_bounds__(256) STTS_NO_PK ctc_confidence_kernel(const float* __restrict__ scores, const int* __restrict__ t_off, double* __restrict__ sums) {
  __shared__ double acc[256];
  const int u = blockIdx.x;
  const long lo = t_off[u], n = t_off[u + 1] - lo;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += exp((double)scores[lo + i]);
  acc[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[u] = acc[0];
}

// Per-class logsumexp over all frames of the batch (losses.py:563-580), two launches.  (1) chunk k = rows [k * kCtcPriorChunk, ..): thread c walks
// class c down the chunk's rows (a wave reads consecutive classes of one row), part[k][c] = (max, sum of exp(x - max)) in fp64; an all -inf
// column gives (-inf, 0).  (2) thread c merges the chunks of class c in chunk order: M = the largest max, sum_k s_k exp(m_k - M), M + log of it.
constexpr int kCtcPriorChunk = 64;

__global__ void __launch_bounds__(256) STTS_NO_PK ctc_prior_part_kernel(const float* __restrict__ lp, int ld, int V, long R, double* __restrict__ part) {
  const long r0 = (long)blockIdx.x * kCtcPriorChunk, r1 = r0 + kCtcPriorChunk < R ? r0 + kCtcPriorChunk : R;
  for (int c = threadIdx.x; c < V; c += 256) {
    double m = -INFINITY;
    for (long r = r0; r < r1; ++r) m = fmax(m, (double)lp[r * ld + c]);
    double s = 0.0;
    if (m != -INFINITY)
      for (long r = r0; r < r1; ++r) s += exp((double)lp[r * ld + c] - m);
    part[2 * ((long)blockIdx.x * V + c)] = m;
    part[2 * ((long)blockIdx.x * V + c) + 1] = s;
  }
}

__global__ void __launch_bounds__(256) STTS_NO_PK ctc_prior_merge_kernel(const double* __restrict__ part, int n_chunks, int V, double* __restrict__ log_sums) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= V) return;
  double M = -INFINITY;
  for (int k = 0; k < n_chunks; ++k) M = fmax(M, part[2 * ((long)k * V + c)]);
  double s = 0.0;
  if (M != -INFINITY)
    for (int k = 0; k < n_chunks; ++k) {
      const double m = part[2 * ((long)k * V + c)];
      if (m != -INFINITY) s += part[2 * ((long)k * V + c) + 1] * exp(m - M);
    }
  log_sums[c] = M == -INFINITY ? -INFINITY : M + log(s);
}

// ------------------------------------------------------------------------------------------------ packing
inline int finalize_aligner(stts_ctx* c, const AlDims& d, AlW* M) {
  *M = AlW();
  M->d = d;
  const std::string p = "text_aligner.";
  STTS_CHECK(d.n_tdnn >= 1 && d.n_tdnn <= kAlMaxTdnn, "aligner: %d tdnn layers outside [1, %d]", d.n_tdnn, kAlMaxTdnn);
  STTS_CHECK(d.ffn_layers >= 1 && d.ffn_layers <= kAlMaxFfn, "aligner: %d ffn layers outside [1, %d]", d.ffn_layers, kAlMaxFfn);
  STTS_CHECK(d.hidden > 0 && d.hidden % 32 == 0 && d.hidden <= 2048, "aligner: hidden_dim %d must be a multiple of 32, at most 2048", d.hidden);
  STTS_CHECK(d.n_mels > 0 && d.n_mels <= 1024, "aligner: n_mels %d outside [1, 1024]", d.n_mels);
  STTS_CHECK(d.classes >= 2 && d.classes <= 256, "aligner: %d classes outside [2, 256] (the row log-softmax keeps four per lane)", d.classes);
  const int H = d.hidden;
  std::vector<float> bn((size_t)d.n_tdnn * 2 * H);
  for (int i = 0; i < d.n_tdnn; ++i) {
    STTS_CHECK(d.tdnn_k[i] >= 1 && d.tdnn_k[i] <= 7 && d.tdnn_k[i] % 2 == 1, "aligner: tdnn kernel %d of layer %d must be odd, at most 7", d.tdnn_k[i], i);
    const std::string q = p + "encoder.layers." + std::to_string(i);
    const int cin = i == 0 ? d.n_mels : H;
    STTS_GET(w, q + ".0.weight");
    STTS_CHECK(w->shape.size() == 3 && w->shape[0] == H && w->shape[1] == cin && w->shape[2] == d.tdnn_k[i], "%s.0.weight: expected [%d, %d, %d]", q.c_str(), H, cin,
               d.tdnn_k[i]);
    STTS_TRY(pack_plain(c, q + ".0", true, 0, cin, &M->tdnn[i]));
    STTS_GET(mean, q + ".2.running_mean");
    STTS_GET(var, q + ".2.running_var");
    STTS_CHECK((int)mean->data.size() == H && (int)var->data.size() == H, "%s.2: expected running statistics of %d channels", q.c_str(), H);
    for (int ch = 0; ch < H; ++ch) {
      STTS_CHECK(var->data[ch] >= 0.f, "%s.2.running_var[%d] is negative", q.c_str(), ch);
      const double sc = 1.0 / sqrt((double)var->data[ch] + 1e-5);
      bn[((size_t)i * 2) * H + ch] = (float)sc;
      bn[((size_t)i * 2 + 1) * H + ch] = (float)(-(double)mean->data[ch] * sc);
    }
  }
  STTS_TRY(dev_upload(c, bn, &M->bn));
  for (int j = 0; j < d.ffn_layers; ++j) {
    const std::string q = p + "encoder.layers." + std::to_string(d.n_tdnn) + ".ffn." + std::to_string(3 * j);
    STTS_GET(w, q + ".weight");
    STTS_CHECK(w->shape.size() == 2 && w->shape[0] == H && w->shape[1] == H, "%s.weight: expected [%d, %d]", q.c_str(), H, H);
    STTS_TRY(pack_plain(c, q, true, 0, H, &M->ffn[j]));
  }
  {
    const std::string q = p + "encoder_output_layer";
    STTS_GET(w, q + ".weight");
    STTS_CHECK(w->shape.size() == 2 && w->shape[0] == d.classes && w->shape[1] == H, "%s.weight: expected [%d, %d]", q.c_str(), d.classes, H);
    STTS_TRY(pack_plain(c, q, true, 0, H, &M->out));
  }
  M->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ forward
constexpr long kAlMaxRows = 1L << 19;  // byte offsets of a [rows, 2048] fp32 buffer stay below 2^32, rows far below 2^24 (gemm.hip.h)

inline int aligner_ld_mel(const AlDims& d) { return round_up(d.n_mels, 32); }
inline int aligner_ld_logits(const AlDims& d) { return round_up(d.classes, 32); }
inline size_t aligner_tap_floats(const AlDims& d, long rows) { return (size_t)rows * ((size_t)(d.n_tdnn + 1) * d.hidden + d.classes); }

// one dense contraction, whole, on the one tile (see the head of this file)
inline int aligner_gemm(hipStream_t st, const Seg& s, const float* X, int ldx, const PackedConv& w, float* Y, int ldy, int act, const float* xaff, int ld_xaff,
                        const float* R = nullptr, int ldr = 0) {
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, X, ldx, 0, w);
  a.N = w.N; a.bias = w.bias; a.Y = Y; a.ldy = ldy; a.act = act; a.R = R; a.ldr = ldr;
  if (xaff) { a.xaff = xaff; a.ld_xaff = ld_xaff; a.xaff_slope = 1.0f; }
  return launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, s.max_len(), 8);
}

// mel [rows, ld_mel >= n_mels] -> log_probs [rows, ld_out >= classes].  taps (optional): the BatchNorm output of every TDNN layer [rows, hidden] each,
// the Ffn output [rows, hidden], the logits [rows, classes], one after the other.
inline int aligner_forward(const AlW& M, hipStream_t st, const Seg& s, const float* mel, int ld_mel, float* log_probs, int ld_out, float* taps, Arena& ws) {
  const AlDims& d = M.d;
  const int H = d.hidden, ldm = aligner_ld_mel(d), ldl = aligner_ld_logits(d), n_utt = s.n_utt, n_tab = d.n_tdnn - 1;
  const long R = s.rows();
  float* m = ws.get<float>((size_t)R * ldm);
  float* buf[3] = {ws.get<float>((size_t)R * H), ws.get<float>((size_t)R * H), ws.get<float>((size_t)R * H)};
  float* logits = ws.get<float>((size_t)R * ldl);
  float* tab = ws.get<float>((size_t)std::max(1, n_tab) * n_utt * 2 * H);
  STTS_CHECK(ws.ok, "aligner_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  const unsigned row_blocks = (unsigned)std::max<long>(1, std::min<long>(2048, (R * H / 4 + 255) / 256));
  hipLaunchKernelGGL(aligner_prepare_kernel, dim3((unsigned)std::max<long>(1, std::min<long>(1024, (R * ldm + 255) / 256))), dim3(256), 0, st, mel, ld_mel, d.n_mels, s.dev,
                     n_utt, m, ldm, M.bn, n_tab, H, tab);
  // ---- TDNN layers: conv + bias + ReLU; the BatchNorm of layer i rides on the staging of layer i + 1
  const float* x = m;
  int ldx = ldm, cur = 0;
  for (int i = 0; i < d.n_tdnn; ++i) {
    const float* aff = i > 0 ? tab + (size_t)(i - 1) * n_utt * 2 * H : nullptr;
    STTS_TRY(aligner_gemm(st, s, x, ldx, M.tdnn[i], buf[cur], H, ACT_RELU, aff, H));
    if (taps && i + 1 < d.n_tdnn)
      hipLaunchKernelGGL(aligner_affine_rows_kernel, dim3(row_blocks), dim3(256), 0, st, buf[cur], s.dev, n_utt, H, M.bn + (size_t)i * 2 * H, taps + (size_t)i * R * H);
    x = buf[cur];
    ldx = H;
    cur ^= 1;
  }
  // ---- the last BatchNorm, materialised: the Ffn's input and its skip operand
  float* x3 = const_cast<float*>(x);
  hipLaunchKernelGGL(aligner_affine_rows_kernel, dim3(row_blocks), dim3(256), 0, st, x3, s.dev, n_utt, H, M.bn + (size_t)(d.n_tdnn - 1) * 2 * H, x3);
  if (taps) STTS_HIP(hipMemcpyAsync(taps + (size_t)(d.n_tdnn - 1) * R * H, x3, (size_t)R * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  // ---- Ffn: buf[cur] and buf[2] alternate, x3 stays
  const float* f = x3;
  float* pp[2] = {buf[cur], buf[2]};
  for (int j = 0; j < d.ffn_layers; ++j) {
    const bool last = j + 1 == d.ffn_layers;
    STTS_TRY(aligner_gemm(st, s, f, H, M.ffn[j], pp[j & 1], H, ACT_RELU, nullptr, 0, last ? x3 : nullptr, H));
    f = pp[j & 1];
  }
  if (taps) STTS_HIP(hipMemcpyAsync(taps + (size_t)d.n_tdnn * R * H, f, (size_t)R * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  STTS_TRY(aligner_gemm(st, s, f, H, M.out, logits, ldl, ACT_NONE, nullptr, 0));
  hipLaunchKernelGGL(aligner_log_softmax_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, logits, ldl, s.dev, n_utt, d.classes, log_probs, ld_out,
                     taps ? taps + (size_t)(d.n_tdnn + 1) * R * H : nullptr);
  STTS_HIP(hipGetLastError());
  return 0;
}

// workspace bytes for these host offsets: a dry run of the carving above
inline size_t aligner_workspace_bytes(const AlW& M, int n_utt, const int* off) {
  const Seg s{n_utt, off, nullptr};
  return dry_run_bytes([&](Arena a) { (void)aligner_forward(M, nullptr, s, nullptr, 0, nullptr, 0, nullptr, a); });
}

// ------------------------------------------------------------------------------------------------ alignment launches
inline size_t ctc_workspace_bytes(int n_utt, const int* t_off, const int* p_off) {
  size_t b = 0;
  for (int u = 0; u < n_utt; ++u) b += (size_t)(t_off[u + 1] - t_off[u]) * (2 * (size_t)(p_off[u + 1] - p_off[u]) + 1);
  return b + 256;
}

// path_given: the label path is an input and only the post-processing runs
inline int ctc_align(hipStream_t st, int n_utt, const int* t_off_dev, const int* p_off_dev, const float* lp, int ld, int V, int blank, const int* targets,
                     int path_given, int* path, float* scores, int* dur, float* left, float* right, unsigned char* bp) {
  if (!path_given) hipLaunchKernelGGL(ctc_viterbi_kernel, dim3(n_utt), dim3(kCtcThreads), 0, st, lp, ld, V, blank, t_off_dev, p_off_dev, targets, bp, path);
  hipLaunchKernelGGL(ctc_durations_kernel, dim3(n_utt), dim3(kCtcThreads), 0, st, lp, ld, V, blank, t_off_dev, p_off_dev, targets, path, scores, dur, left, right);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int ctc_nll(hipStream_t st, int n_utt, const int* t_off_dev, const int* p_off_dev, const float* lp, int ld, int V, int blank, const int* targets,
                   const double* log_priors, double prior_scale, double* nll) {
  hipLaunchKernelGGL(ctc_forward_kernel, dim3(n_utt), dim3(kCtcThreads), 0, st, lp, ld, V, blank, t_off_dev, p_off_dev, targets, log_priors, prior_scale, nll);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline int ctc_prior_chunks(long rows) { return (int)((rows + kCtcPriorChunk - 1) / kCtcPriorChunk); }
inline size_t ctc_prior_workspace_bytes(long rows, int V) { return (size_t)ctc_prior_chunks(rows) * V * 2 * sizeof(double); }

inline int ctc_prior_sums(hipStream_t st, long rows, const float* lp, int ld, int V, double* log_sums, double* part) {
  const int n_chunks = ctc_prior_chunks(rows);
  hipLaunchKernelGGL(ctc_prior_part_kernel, dim3(n_chunks), dim3(256), 0, st, lp, ld, V, rows, part);
  hipLaunchKernelGGL(ctc_prior_merge_kernel, dim3(ceil_div(V, 256)), dim3(256), 0, st, part, n_chunks, V, log_sums);
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

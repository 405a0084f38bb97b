// The library's 2-D implicit-GEMM convolution on the f32 matrix cores (v_mfma_f32_16x16x4_f32): MelStyleEncoder (mel_style.hip.h) and RMVPE
// (rmvpe.hip.h) both run on it.  Included by api.hip before mel_style.hip.h.  fp32 whatever stts_set_precision chose, no packed-fp32.
//
// Layout: channels-last packed rows.  A level's activation of utterance u is the rows ((off[u] >> sh) + t) * F + f, t < T_u,
// f < F, each row ld(C) = round_up(C, 16) floats with the channels contiguous and the pad channels zero.  M = positions of the BASE grid (the output
// level's offsets, F columns), N = cout, K = taps x (channels of segment 0 | channels of segment 1) in tap-major order.  Tap i of base position (t, f)
// reads input position (t + dt[i], f + df[i]) of the input level's rows (its own offsets and Fin columns); positions outside [0, T_u) x [0, Fin) are
// zeros, so no im2col buffer exists, and two segments read cat(a, b) without a concat buffer.  A base position writes the output position
// (t * up + pt, f * up + pf) of a grid up * F wide: up = 1 is a plain convolution, up = 2 one of the four sub-pixel convolutions of a stride-2
// transposed convolution.  A contraction over frames is the same kernel with F = 1 and one tap.
//
// Summation: K is cut into chunks of `chunk` in weight order; a chunk is one fp32 fmaf chain on the matrix core and the chunk sums are added in chunk
// order, either in the kernel (a second accumulator) or, when the launch has slices, one chunk per grid z with conv2d_reduce_kernel adding the slices
// in the same order.  Then bias, activation, + residual, / div.  Nothing depends on the batch: an utterance's result is the same bits alone and in any
// batch.
//
// Domain (conv2d_pack and conv2d_launch refuse the rest): ld0, ld1 multiples of kConvBK = 16 (a K step never straddles a tap or a segment), npad 16, 32 or
// a multiple of 64, N <= ldy <= npad (both summation paths then write channels 0 .. N - 1 and zeros up to ldy), chunk a multiple of 16, offsets
// multiples of 1 << sh.  tests/test_hip_conv2d.py holds every tile, both summation paths and every row map to float64 through stts_op_conv2d.
#pragma once

namespace stts {

constexpr int kConvBK = 16;       // K step: one tap, 16 channels
constexpr int kConvMaxTaps = 25;  // 5 x 5

enum { CONV_ACT_NONE = 0, CONV_ACT_RELU = 1, CONV_ACT_SIGMOID = 2 };

struct Conv2dW {  // packed [K][npad], K row = tap * (ld0 + ld1) + channel (segment 0 first); bias [cout] or null
  int cout = 0, ld0 = 0, ld1 = 0, ntap = 0, npad = 0, K = 0;
  int dt[kConvMaxTaps] = {}, df[kConvMaxTaps] = {};
  float* w = nullptr;
  float* b = nullptr;
};

struct Conv2dArgs {
  const float* X0;  // segment 0 rows [((offIn[u] >> sh) + t) * Fin + f][ld0]
  const float* X1;  // segment 1 (null when ld1 == 0)
  int ld0, ld1;
  const int* offIn;   // time offsets of the input level
  const int* offOut;  // time offsets of the base grid
  int n_utt, sh;      // the offsets are used >> sh
  int Fin, F;         // input columns, base-grid columns
  int ntap;
  int dt[kConvMaxTaps], df[kConvMaxTaps];  // tap i reads input position (t + dt[i], f + df[i])
  int up, pt, pf;                          // output position (t * up + pt, f * up + pf) of a grid up * F wide
  long rows;                               // base positions
  const float* W;                          // [K][npad]
  int npad, N, K;
  int chunk;  // K per accumulator chain (a multiple of kConvBK)
  const float* bias;
  int act;
  const float* R;  // residual [output rows][ldy] or null, added after the activation
  float div;       // the result is divided by div
  float* Y;        // [output rows][ldy]; channels N .. ldy - 1 are written as 0
  int ldy;
  float* P;  // slices: partial sums [slice][base position][ldy] (the epilogue runs in conv2d_reduce_kernel)
};

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ float lrelu02(float v) { return v > 0.f ? v : 0.2f * v; }

// the utterance of time row tr of level sh: the largest u with (off[u] >> sh) <= tr
__device__ __forceinline__ int utt_of_row(const int* __restrict__ off, int n_utt, int sh, int tr) {
  int lo = 0, hi = n_utt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((off[mid] >> sh) <= tr) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct Conv2dRow {
  int t, f, T;  // base position; T = the utterance's input length
  long in0;     // first input time row of the utterance
  long orow;    // output row
};

__device__ __forceinline__ Conv2dRow conv2d_row(const Conv2dArgs& g, long m) {
  Conv2dRow r;
  const int tr = (int)(m / g.F);
  r.f = (int)(m - (long)tr * g.F);
  const int u = utt_of_row(g.offOut, g.n_utt, g.sh, tr);
  r.t = tr - (g.offOut[u] >> g.sh);
  r.in0 = g.offIn[u] >> g.sh;
  r.T = (g.offIn[u + 1] >> g.sh) - (int)r.in0;
  r.orow = ((long)tr * g.up + g.pt) * (long)(g.F * g.up) + r.f * g.up + g.pf;
  return r;
}

__device__ __forceinline__ float conv2d_epilogue(const Conv2dArgs& g, float v, int n, long orow) {
  if (g.bias) v += g.bias[n];
  if (g.act == CONV_ACT_RELU) v = fmaxf(v, 0.f);
  else if (g.act == CONV_ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
  if (g.R) v += g.R[orow * g.ldy + n];
  return v / g.div;
}

// grid (ceil(rows / BM), npad / BN, slices), block 256 = 4 waves as WM x WN, each MT x NT tiles of 16 x 16.  BM = 16 MT WM, BN = 16 NT WN.
// LRELU: LeakyReLU(0.2) on the operand as it is loaded.  The next K step's operands are loaded into registers while the matrix cores run the
// current one; the load is inlined at both of its call sites so that nothing the K loop touches is addressable memory (no scratch).  The occupancy
// hint keeps the 64 x 64 tile within 64 registers (8 waves per SIMD, what the encoder's large batches need).
template <int MT, int NT, int WM, int WN, bool LRELU>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WM == 2 ? 6 : 4, 8))) STTS_NO_PK conv2d_kernel(Conv2dArgs g) {
  static_assert(WM * WN == 4, "four waves");
  constexpr int BM = 16 * MT * WM, BN = 16 * NT * WN;
  constexpr int RA = BM / 64;                         // A rows per thread (4 channels of each per K step)
  constexpr int NB = (kConvBK * BN / 4 + 255) / 256;  // B float4s per thread
  __shared__ float As[kConvBK][BM + 4];
  __shared__ float Bs[kConvBK][BN + 4];
  __shared__ long orow_s[BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int akq = (tid & 3) * 4;
  Conv2dRow row[RA];
  bool mval[RA];
#pragma unroll
  for (int j = 0; j < RA; ++j) {
    const long m = m0 + (tid >> 2) + 64 * j;
    mval[j] = m < g.rows;
    row[j] = conv2d_row(g, mval[j] ? m : 0);
  }
  for (int r = tid; r < BM; r += 256) orow_s[r] = m0 + r < g.rows ? conv2d_row(g, m0 + r).orow : -1;
  const int Kt = g.ld0 + g.ld1;
  const int kb = g.P ? blockIdx.z * g.chunk : 0, ke = g.P ? min(g.K, kb + g.chunk) : g.K;
  float4 ra[RA], rb[NB];
  auto load = [&](int k0) __attribute__((always_inline)) {
    const int tap = k0 / Kt, cc = k0 - tap * Kt;
    const bool s1 = cc >= g.ld0;
    const float* X = s1 ? g.X1 : g.X0;
    const int ld = s1 ? g.ld1 : g.ld0, ci = (s1 ? cc - g.ld0 : cc) + akq;
    const int dt = g.dt[tap], df = g.df[tap];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      const int ti = row[j].t + dt, fi = row[j].f + df;
      ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (mval[j] && ti >= 0 && ti < row[j].T && fi >= 0 && fi < g.Fin) {
        ra[j] = *reinterpret_cast<const float4*>(X + ((row[j].in0 + ti) * g.Fin + fi) * (long)ld + ci);
        if (LRELU) {
          ra[j].x = lrelu02(ra[j].x);
          ra[j].y = lrelu02(ra[j].y);
          ra[j].z = lrelu02(ra[j].z);
          ra[j].w = lrelu02(ra[j].w);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int i = tid + 256 * j;
      if (i < kConvBK * BN / 4) rb[j] = *reinterpret_cast<const float4*>(g.W + (long)(k0 + i / (BN / 4)) * g.npad + n0 + (i % (BN / 4)) * 4);
    }
  };
  const int wm = (wave / WN) * MT * 16, wn = (wave % WN) * NT * 16;
  f32x4 acc[MT][NT], tot[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(kb);
  int kc = 0;  // K of the running chain
  for (int k0 = kb; k0 < ke; k0 += kConvBK) {
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      const int ar = (tid >> 2) + 64 * j;
      As[akq + 0][ar] = ra[j].x;
      As[akq + 1][ar] = ra[j].y;
      As[akq + 2][ar] = ra[j].z;
      As[akq + 3][ar] = ra[j].w;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int i = tid + 256 * j;
      if (i < kConvBK * BN / 4) *reinterpret_cast<float4*>(&Bs[i / (BN / 4)][(i % (BN / 4)) * 4]) = rb[j];
    }
    __syncthreads();
    if (k0 + kConvBK < ke) load(k0 + kConvBK);
#pragma unroll
    for (int kk = 0; kk < kConvBK; kk += 4) {
      const int kl = kk + (lane >> 4);
      float av[MT], bv[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) av[i] = As[kl][wm + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = Bs[kl][wn + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    kc += kConvBK;
    if (kc == g.chunk || k0 + kConvBK >= ke) {  // end of a chunk: its sum joins the total
      kc = 0;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          tot[i][j] += acc[i][j];
          acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
  // D of a 16 x 16 tile: lane l holds rows 4 (l / 16) + r, r < 4, of column l % 16
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn + j * 16 + (lane & 15);
      if (n >= g.ldy) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ml = wm + i * 16 + 4 * (lane >> 4) + r;
        const long orow = orow_s[ml];
        if (orow < 0) continue;
        if (g.P) {
          g.P[((long)blockIdx.z * g.rows + m0 + ml) * g.ldy + n] = tot[i][j][r];
          continue;
        }
        g.Y[orow * g.ldy + n] = n < g.N ? conv2d_epilogue(g, tot[i][j][r], n, orow) : 0.f;
      }
    }
}

// the slices' sums in slice order, then the epilogue of conv2d_kernel
__global__ void __launch_bounds__(256) STTS_NO_PK conv2d_reduce_kernel(Conv2dArgs g, int slices) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = g.rows * g.ldy;
  if (i >= total) return;
  const long m = i / g.ldy;
  const int n = (int)(i - m * g.ldy);
  const long orow = conv2d_row(g, m).orow;
  float v = 0.f;
  if (n < g.N) {
    v = g.P[i];
    for (int z = 1; z < slices; ++z) v += g.P[(long)z * total + i];
    v = conv2d_epilogue(g, v, n, orow);
  }
  g.Y[orow * g.ldy + n] = v;
}

// ------------------------------------------------------------------------------------------------ packing
// wf(n, channel of cat(segment 0, segment 1), tap) -> the weight in double; npad: the padded width, which picks the tile (conv2d_launch)
template <typename WF>
inline int conv2d_pack(stts_ctx* c, int cout, int npad, int cin0, int cin1, int ld0, int ld1, int ntap, const int* dt, const int* df, WF wf,
                       const std::vector<double>* bias, Conv2dW* o) {
  *o = Conv2dW();
  o->cout = cout;
  o->ld0 = ld0;
  o->ld1 = ld1;
  o->ntap = ntap;
  o->npad = npad;
  o->K = ntap * (ld0 + ld1);
  // a K step is one tap and kConvBK channels of ONE segment, so each segment's row stride is a whole number of steps (and a row a whole number of float4)
  STTS_CHECK(ld0 > 0 && ld0 % kConvBK == 0 && ld1 >= 0 && ld1 % kConvBK == 0 && cin0 >= 0 && cin0 <= ld0 && cin1 >= 0 && cin1 <= ld1 && ntap >= 1 && ntap <= kConvMaxTaps &&
                 cout >= 1 && cout <= npad && (npad == 16 || npad == 32 || (npad > 0 && npad % 64 == 0)),
             "conv2d: a conv of %d x (%d + %d) -> %d (padded to %d) does not pack: row strides are multiples of %d, the width is 16, 32 or a multiple of 64", ntap, ld0, ld1, cout,
             npad, kConvBK);
  for (int i = 0; i < ntap; ++i) {
    o->dt[i] = dt[i];
    o->df[i] = df[i];
  }
  std::vector<float> pk((size_t)o->K * o->npad, 0.f);
  for (int tap = 0; tap < ntap; ++tap)
    for (int ci = 0; ci < cin0 + cin1; ++ci) {
      const size_t k = (size_t)tap * (ld0 + ld1) + (ci < cin0 ? ci : ld0 + ci - cin0);
      for (int n = 0; n < cout; ++n) pk[k * o->npad + n] = (float)wf(n, ci, tap);
    }
  STTS_TRY(dev_upload(c, pk, &o->w));
  if (bias) {
    std::vector<float> b(cout);
    for (int n = 0; n < cout; ++n) b[n] = (float)(*bias)[n];
    STTS_TRY(dev_upload(c, b, &o->b));
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ launch
// the descriptor's weight half; the caller fills the inputs, the row maps, the grid, the epilogue and the outputs
inline Conv2dArgs conv2d_args(const Conv2dW& w) {
  Conv2dArgs g = {};
  g.ld0 = w.ld0;
  g.ld1 = w.ld1;
  g.ntap = w.ntap;
  for (int i = 0; i < kConvMaxTaps; ++i) {
    g.dt[i] = w.dt[i];
    g.df[i] = w.df[i];
  }
  g.up = 1;
  g.W = w.w;
  g.npad = w.npad;
  g.N = w.cout;
  g.K = w.K;
  g.bias = w.b;
  g.div = 1.f;
  return g;
}

// The tile follows npad: 256 x 16, 128 x 32, else 64 x 64 (the only one with the LeakyReLU operand).  slices > 1: one chunk per grid z into g.P, then
// the reduce.
inline int conv2d_launch(hipStream_t st, const Conv2dArgs& g, bool lrelu, int slices) {
  STTS_CHECK(slices == 1 ? !g.P : g.P && slices == ceil_div(g.K, g.chunk), "conv2d: %d slices without their scratch", slices);
  STTS_CHECK(g.ld1 == 0 || g.X1, "conv2d: a two-segment conv without its second input");
  STTS_CHECK(g.chunk > 0 && g.chunk % kConvBK == 0 && (!lrelu || g.npad % 64 == 0), "conv2d: chunk %d, npad %d%s", g.chunk, g.npad, lrelu ? " (LeakyReLU operand)" : "");
  // the tiles cover columns 0 .. npad - 1 and write those below ldy, so a row of Y is written whole (channels, then zeros) only when it is no wider than npad
  STTS_CHECK(g.N >= 1 && g.N <= g.ldy && g.ldy <= g.npad, "conv2d: %d channels into rows of %d floats from tiles %d wide (N <= ldy <= npad)", g.N, g.ldy, g.npad);
  if (g.rows == 0) return 0;
#define STTS_CONV2D(MT, NT, WM, WN, LRELU)                                                                                                                       \
  hipLaunchKernelGGL((conv2d_kernel<MT, NT, WM, WN, LRELU>), dim3((unsigned)((g.rows + 16 * MT * WM - 1) / (16 * MT * WM)), g.npad / (16 * NT * WN), slices), \
                     dim3(256), 0, st, g)
  if (g.npad == 16) STTS_CONV2D(4, 1, 4, 1, false);
  else if (g.npad == 32) STTS_CONV2D(2, 2, 4, 1, false);
  else if (lrelu) STTS_CONV2D(2, 2, 2, 2, true);
  else STTS_CONV2D(2, 2, 2, 2, false);
#undef STTS_CONV2D
  if (slices > 1) hipLaunchKernelGGL(conv2d_reduce_kernel, dim3((unsigned)((g.rows * g.ldy + 255) / 256)), dim3(256), 0, st, g, slices);
  return 0;
}

}  // namespace stts

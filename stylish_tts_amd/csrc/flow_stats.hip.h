// Flow statistics: ResidualCouplingBlock.forward in BOTH directions with the three streams the reference carries through it (z, mean, logstd;
// models/flow.py:132-151, the coupling layer :196-218, WN :63-88), PriorEncoder.forward with its three outputs (:311-315) and the per-utterance sums of
// the two KL scores NormalizingFlowLoss logs (train/losses.py:157-222).  Component STTS_W_FLOW_STATS: its own fp32 packing of the keys
// "speech_predictor.flow.flows.{0,2,..,14}.*" and "speech_predictor.prior_encoder.*", whatever the engine's precision - these are validation numbers.
// Included by api.hip behind every other stage, so its kernels are the last of the code object.  plan_flow_stats() chooses the form of a coupling
// layer, flow_stats_forward() walks the stage.
//
// Two forms of a coupling layer.  The generic one, the correctness baseline and what runs at any width other than 128: pre (EPI_STORE) -> 4 x { k = 5
// conv with EPI_GATE, res/skip with EPI_SPLIT_ACC } -> proj to m | s (EPI_STORE) -> flow_stats_couple_kernel, which applies the coupling to the three
// streams in the asked direction (11 launches).  The fused one: wn_stats_kernel, one launch per WaveNet layer (4 launches).
#pragma once

namespace stts {

// Coupling of the three streams, columns [col0, col0 + half) of z / mean / logstd [rows, ld]; ms [rows, ld_ms] holds m in columns [0, half) and s in
// [half, 2 half).  reverse 0: x1 = m + x1 exp(s), logstd1 += s; reverse 1: x1 = (x1 - m) exp(-s), logstd1 -= s (flow.py:209-216).  A thread owns four
// consecutive columns of one row; the other half of every stream is never touched.
__global__ void __launch_bounds__(256) STTS_NO_PK flow_stats_couple_kernel(const float* __restrict__ ms, int ld_ms, int half, long n4, int reverse, float* __restrict__ z,
                                                                           float* __restrict__ mean, float* __restrict__ logstd, int ld, int col0) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const int q = half / 4;
  const long r = e / q;
  const int j = 4 * (int)(e % q);
  const f32x4 m = *reinterpret_cast<const f32x4*>(ms + r * ld_ms + j), sv = *reinterpret_cast<const f32x4*>(ms + r * ld_ms + half + j);
  float* pz = z + r * ld + col0 + j;
  float* pm = mean + r * ld + col0 + j;
  float* pl = logstd + r * ld + col0 + j;
  f32x4 vz = *reinterpret_cast<f32x4*>(pz), vm = *reinterpret_cast<f32x4*>(pm), vl = *reinterpret_cast<f32x4*>(pl);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (reverse) {
      const float ex = expf(-sv[i]);
      vz[i] = (vz[i] - m[i]) * ex;
      vm[i] = (vm[i] - m[i]) * ex;
      vl[i] = vl[i] - sv[i];
    } else {
      const float ex = expf(sv[i]);
      vz[i] = m[i] + vz[i] * ex;
      vm[i] = m[i] + vm[i] * ex;
      vl[i] = vl[i] + sv[i];
    }
  }
  *reinterpret_cast<f32x4*>(pz) = vz;
  *reinterpret_cast<f32x4*>(pm) = vm;
  *reinterpret_cast<f32x4*>(pl) = vl;
}

// part[row] = the row's sum over C channels of the KL term, in fp64 from the fp32 values on (losses.py:174-175, :198-199):
//   kind 0 (kl_loss):        d - b - 0.5 + 0.5 (a - c)^2 exp(-2 d)                 a = z_p, b = logs_q, c = m_p, d = logs_p
//   kind 1 (kl_loss_normal): d - b - 0.5 + 0.5 (exp(2 b) + (a - c)^2) exp(-2 d)    a = m_q
// One wave per row, four to a block; lane l takes channels l, l + 64, ... in order, the xor butterfly joins the 64 sums: a fixed order, no atomics.
// Grid (ceil(max_len / 4), n_utt).
__global__ void __launch_bounds__(256) STTS_NO_PK flow_stats_kl_kernel(const int* __restrict__ off, int kind, const float* __restrict__ a, const float* __restrict__ b,
                                                                       const float* __restrict__ c, const float* __restrict__ d, int ld, int C, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.y, t = blockIdx.x * 4 + wv;
  if (t >= off[u + 1] - off[u]) return;
  const long row = (long)off[u] + t;
  double s = 0.0;
  for (int k = lane; k < C; k += 64) {
    const double va = a[row * ld + k], vb = b[row * ld + k], vc = c[row * ld + k], vd = d[row * ld + k];
    const double diff = va - vc;
    const double var = kind == 1 ? exp(2.0 * vb) + diff * diff : diff * diff;
    s += (vd - vb - 0.5) + 0.5 * var * exp(-2.0 * vd);
  }
  s = wave_sum_f64(s);
  if (lane == 0) part[row] = s;
}

// wn_stats_kernel<RT, LAST>: one WaveNet layer of a coupling layer in one launch, the structure of wn_post_kernel (posterior.hip.h) with TAPS = 5,
// PAD = 2 - a separate kernel that shares that family's unchanged helpers only (pack_fragments, mfma4, wn_dispatch, kWnSegInline, seg_blocks):
//   x_in = wn-conv1d k5 (h)  128 -> 256 ; acts = tanh(x_in[:128] + g[:128]) * sigmoid(x_in[128:] + g[128:]) ; rs = wn-Linear(acts)  128 -> 256 (LAST: 128)
//   h += rs[:128] ; out (+)= rs[128:]
//   LAST (layer 3): out += rs stays on chip ; m, s = proj(out) on the matrix cores ; the coupling of the three streams in the direction of the
//   arguments ; tail 2: the next coupling layer's h_0 = pre(z1') into Hpre.
// A block is RT tiles of 16 consecutive rows of ONE utterance; its rows and two halo rows each side sit in LDS once, in MFMA-fragment order (row r of
// the window at tile r >> 4, slot r & 15), so tap j of row tile rt is the same image read j slots further.  Rows outside the utterance are zeros, rows
// past its end are never stored, and every load is clamped into the utterance: the buffers need no slack rows.  v_mfma_f32_16x16x4_f32 on fp32
// operands; wave w of 4 owns the tanh and sigmoid tiles of channels [32 w, 32 w + 32).  The k = 5 weight prefetch is one 16-channel block ahead:
// 20 fragments per buffer and wave.
constexpr int kFsC = 128;    // flow channels the fused kernel is built for (decoder.hidden_dim / 4)
constexpr int kFsTaps = 5;   // ... and its kernel size
constexpr int kFsWaves = 4;

struct WnStatsArgs {
  const float* Hin;    // [rows, 128]
  float* Hout;         // [rows, 128], another buffer than Hin: neighbouring blocks still read their halo rows (unused when LAST)
  float* Out;          // [rows, 128], updated in place (read when out_acc; LAST: read only)
  const int* seg_off;
  const float* W1;     // in_layers, fragments [4 waves][8 blocks][5 taps][2 halves][2 tiles][64 lanes][4]
  const float* b1;     // [256] natural order: tanh rows 0..127 | sigmoid rows 128..255
  const float* W2;     // res_skip, fragments [4][8][4 (LAST: 2)][64][4]
  const float* b2;     // [256] (LAST: [128])
  const float* gate;   // [n_utt][ld_gate]: the utterance's cond row
  int ld_gate, gcol0;
  int out_acc;         // accumulate into Out (0 on the first layer)
  // LAST only
  int tail;            // 1 = proj + coupling, 2 = additionally the next coupling layer's pre
  int reverse;         // 0: x1 = m + x1 exp(s), logstd1 += s ; 1: x1 = (x1 - m) exp(-s), logstd1 -= s
  const float* W3;     // proj_mean | proj_logstd, fragments [4][8][2][64][4]
  const float* b3m;    // [64]
  const float* b3s;    // [64]
  float *Z, *Mean, *Logstd;  // [rows, ld]; columns [col0, col0 + 64) are updated in place
  int ld, col0;
  const float* W4;     // the next coupling layer's pre, fragments [4][4][2][64][4]
  const float* b4;     // [128]
  float* Hpre;         // [rows, 128], another buffer than Hin
  int n_inline;        // > 0: seg_inline holds the n_inline + 1 utterance offsets (seg_off is not read)
  int seg_inline[kWnSegInline + 1];
};

template <int RT, bool LAST>
__global__ void __launch_bounds__(256) wn_stats_kernel(const WnStatsArgs a) {
  constexpr int ROWS = 16 * RT, C = kFsC, KB = C / 16, NW = kFsWaves, CT = C / NW / 16, TAPS = kFsTaps, PAD = TAPS / 2;
  constexpr int NCT = LAST ? CT : 2 * CT;       // res/skip column tiles per wave
  __shared__ f32x4 Af[(RT + 1) * KB * 64];  // rows [row0 - 2, row0 + ROWS + 2) in fragment order [tile][block][lane]; slots from ROWS + 4 on are never read.  LAST: later z1'
  __shared__ f32x4 A2[RT * KB * 64];        // gated activations, LAST: then the finished `out` [row tile][block][lane]

  const int utt = blockIdx.y;
  const int lo = a.n_inline ? a.seg_inline[utt] : a.seg_off[utt], hi = a.n_inline ? a.seg_inline[utt + 1] : a.seg_off[utt + 1];
  const int row0 = lo + blockIdx.x * ROWS;
  if (row0 >= hi) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int nvalid = hi - row0;

  // ---- phase-1 weight stream: wave w reads its own slice [8 blocks][5 taps][2 halves][CT] fragments (1 KB each) one block ahead of the MFMAs
  constexpr int T1 = TAPS * 2 * CT;
  const f32x4* w1 = reinterpret_cast<const f32x4*>(a.W1) + (size_t)w * KB * (T1 * 64) + lane;
  f32x4 bq0[T1], bq1[T1];
  auto load1 = [&](f32x4(&dst)[T1], int u) {
#pragma unroll
    for (int j = 0; j < T1; ++j) dst[j] = w1[(u * T1 + j) * 64];
  };
  load1(bq0, 0);
  __builtin_amdgcn_sched_barrier(0);

  // ---- prologue: the block's rows and two halo rows each side; rows outside the utterance are its zero padding (the load is clamped into it)
  for (int e = tid; e < (ROWS + 2 * PAD) * (C / 4); e += 256) {
    const int r = e / (C / 4), cq = e % (C / 4);
    const int row = row0 - PAD + r;
    const bool ok = row >= lo && row < hi;
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.Hin + (long)min(max(row, lo), hi - 1) * C + 4 * cq);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    Af[((r >> 4) * KB + (cq >> 2)) * 64 + (cq & 3) * 16 + (r & 15)] = ok ? v : z;
  }
  // Orientation as in wn_post_kernel: D^T = W x A^T, a lane holds four consecutive channels (4 lq + i of the tile) of one row (l15).
  f32x4 ba[CT], bb[CT], ga[CT], gb[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int ch = (C / NW) * w + 16 * c + 4 * lq;
    ba[c] = *reinterpret_cast<const f32x4*>(a.b1 + ch);
    bb[c] = *reinterpret_cast<const f32x4*>(a.b1 + C + ch);
    ga[c] = *reinterpret_cast<const f32x4*>(a.gate + (long)utt * a.ld_gate + a.gcol0 + ch);
    gb[c] = *reinterpret_cast<const f32x4*>(a.gate + (long)utt * a.ld_gate + a.gcol0 + C + ch);
  }
  __syncthreads();

  // ---- phase 1: RT row tiles x (tanh, sigmoid) x CT tiles, K = 5 taps x 128 channels in 8 blocks of 16 (4 MFMA k-steps each)
  f32x4 acc[RT][2][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[rt][h][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step1 = [&](int t, const f32x4(&cur)[T1]) {
#pragma unroll
    for (int j = 0; j < TAPS; ++j) {  // (tap by tap: five taps' images of RT tiles at once would not fit next to the prefetch at RT = 4)
      f32x4 av[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int rr = 16 * rt + l15 + j;  // window row of (output row 16 rt + l15, tap j)
        av[rt] = Af[((rr >> 4) * KB + t) * 64 + lq * 16 + (rr & 15)];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][h][c] = mfma4(cur[(j * 2 + h) * CT + c][s], av[rt][s], acc[rt][h][c]);
    }
  };
  auto interleave = [&]() {  // the T1 loads of the next block go between this block's MFMAs, one per four
#pragma unroll
    for (int q = 0; q < T1; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll 1
  for (int it = 0; it < KB / 2; ++it) {
    load1(bq1, 2 * it + 1);
    step1(2 * it, bq0);
    interleave();
    if (2 * it + 2 < KB) load1(bq0, 2 * it + 2);
    step1(2 * it + 1, bq1);
    interleave();
  }

  // ---- phase-2 operands requested now: this wave's res/skip weights, bias, the h / out values the epilogue updates (rows past the utterance's
  // end read row0 instead and are never stored)
  const f32x4* w2 = reinterpret_cast<const f32x4*>(a.W2) + (size_t)w * KB * (NCT * 64) + lane;
  f32x4 cq2[KB][NCT];
#pragma unroll
  for (int t = 0; t < KB; ++t)
#pragma unroll
    for (int c = 0; c < NCT; ++c) cq2[t][c] = w2[(t * NCT + c) * 64];
  f32x4 bv[NCT], old[RT][NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int n = 16 * NCT * w + 16 * c + 4 * lq;  // first of this lane's four res/skip output columns of tile c
    bv[c] = *reinterpret_cast<const f32x4*>(a.b2 + n);
    const bool to_h = !LAST && n < C;
    const int col = (!LAST && n >= C) ? n - C : n;
    const float* src = to_h ? a.Hin : a.Out;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rl = 16 * rt + l15;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (long)(row0 + (rl < nvalid ? rl : 0)) * C + col);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      old[rt][c] = (to_h || a.out_acc) ? v : z;
    }
  }

  // ---- gate: written to LDS as the B operand of res/skip (tanhf / __expf: the arithmetic of the contractions' EPI_GATE)
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 va = acc[rt][0][c] + ba[c] + ga[c], vb = acc[rt][1][c] + bb[c] + gb[c];
      f32x4 act;
#pragma unroll
      for (int i = 0; i < 4; ++i) act[i] = tanhf(va[i]) * (1.0f / (1.0f + __expf(-vb[i])));
      A2[(rt * KB + CT * w + c) * 64 + lq * 16 + l15] = act;
    }
  __syncthreads();

  // ---- phase 2: res/skip, K = 128 from LDS; wave w owns columns [16 NCT w, 16 NCT (w + 1)), all row tiles
  f32x4 acc2[RT][NCT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc2[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    f32x4 av[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) av[rt] = A2[(rt * KB + t) * 64 + lane];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc2[rt][c] = mfma4(cq2[t][c][s], av[rt][s], acc2[rt][c]);
  }

  if constexpr (!LAST) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const int n = 16 * NCT * w + 16 * c + 4 * lq;
      const bool to_h = n < C;
      const int col = to_h ? n : n - C;
      float* dst = to_h ? a.Hout : a.Out;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        if (16 * rt + l15 < nvalid) *reinterpret_cast<f32x4*>(dst + (long)(row0 + 16 * rt + l15) * C + col) = old[rt][c] + (acc2[rt][c] + bv[c]);
    }
  } else {
    // ---- tail: proj + the coupling of the three streams (+ the next coupling layer's pre) on this block's rows.
    // wave w: the m tile and the s tile of channels [16 w, 16 w + 16) of the coupled half, all row tiles
    const f32x4* w3 = reinterpret_cast<const f32x4*>(a.W3) + (size_t)w * KB * (2 * 64) + lane;
    f32x4 pq[KB][2];
#pragma unroll
    for (int t = 0; t < KB; ++t) {
      pq[t][0] = w3[(t * 2 + 0) * 64];
      pq[t][1] = w3[(t * 2 + 1) * 64];
    }
    const int cc = 16 * w + 4 * lq;  // first of this lane's four channels of the coupled half
    const f32x4 pm = *reinterpret_cast<const f32x4*>(a.b3m + cc), ps = *reinterpret_cast<const f32x4*>(a.b3s + cc);
    f32x4 zo[RT], mo[RT], so[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rl = 16 * rt + l15;
      const long at = (long)(row0 + (rl < nvalid ? rl : 0)) * a.ld + a.col0 + cc;
      zo[rt] = *reinterpret_cast<const f32x4*>(a.Z + at);
      mo[rt] = *reinterpret_cast<const f32x4*>(a.Mean + at);
      so[rt] = *reinterpret_cast<const f32x4*>(a.Logstd + at);
    }
    __syncthreads();  // every wave has finished reading the gated activations
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)  // finished `out` values of (row 16 rt + l15, channels 16 (NCT w + c) + 4 lq + (0..3))
        A2[(rt * KB + NCT * w + c) * 64 + lq * 16 + l15] = old[rt][c] + (acc2[rt][c] + bv[c]);
    __syncthreads();
    f32x4 acc3[RT][2];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc3[rt][0] = acc3[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KB; ++t) {
      f32x4 av[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) av[rt] = A2[(rt * KB + t) * 64 + lane];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          acc3[rt][0] = mfma4(pq[t][0][s], av[rt][s], acc3[rt][0]);
          acc3[rt][1] = mfma4(pq[t][1][s], av[rt][s], acc3[rt][1]);
        }
    }
    // the next coupling layer's pre: weights of wave w's two column tiles, requested ahead of the coupling math
    constexpr int KB4 = KB / 2;  // K = 64
    f32x4 rq[KB4][2];
    f32x4 hb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (a.tail > 1) {
      const f32x4* w4 = reinterpret_cast<const f32x4*>(a.W4) + (size_t)w * KB4 * (2 * 64) + lane;
#pragma unroll
      for (int t = 0; t < KB4; ++t) {
        rq[t][0] = w4[(t * 2 + 0) * 64];
        rq[t][1] = w4[(t * 2 + 1) * 64];
      }
      hb[0] = *reinterpret_cast<const f32x4*>(a.b4 + 32 * w + 4 * lq);
      hb[1] = *reinterpret_cast<const f32x4*>(a.b4 + 32 * w + 16 + 4 * lq);
    }
    // [row tile][4 blocks][lane]: the coupled half of z as the B operand of `pre` (the phase-1 image in Af is long dead)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 mm = acc3[rt][0] + pm, ls = acc3[rt][1] + ps;
      f32x4 z1, m1, s1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (a.reverse) {
          const float ex = expf(-ls[i]);
          z1[i] = (zo[rt][i] - mm[i]) * ex;
          m1[i] = (mo[rt][i] - mm[i]) * ex;
          s1[i] = so[rt][i] - ls[i];
        } else {
          const float ex = expf(ls[i]);
          z1[i] = mm[i] + zo[rt][i] * ex;
          m1[i] = mm[i] + mo[rt][i] * ex;
          s1[i] = so[rt][i] + ls[i];
        }
      }
      if (16 * rt + l15 < nvalid) {
        const long at = (long)(row0 + 16 * rt + l15) * a.ld + a.col0 + cc;
        *reinterpret_cast<f32x4*>(a.Z + at) = z1;
        *reinterpret_cast<f32x4*>(a.Mean + at) = m1;
        *reinterpret_cast<f32x4*>(a.Logstd + at) = s1;
      }
      Af[(rt * KB4 + w) * 64 + lq * 16 + l15] = z1;
    }
    if (a.tail < 2) return;
    __syncthreads();
    f32x4 acc4[RT][2];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc4[rt][0] = acc4[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KB4; ++t) {
      f32x4 av[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) av[rt] = Af[(rt * KB4 + t) * 64 + lane];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          acc4[rt][0] = mfma4(rq[t][0][s], av[rt][s], acc4[rt][0]);
          acc4[rt][1] = mfma4(rq[t][1][s], av[rt][s], acc4[rt][1]);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        if (16 * rt + l15 < nvalid) *reinterpret_cast<f32x4*>(a.Hpre + (long)(row0 + 16 * rt + l15) * C + 32 * w + 16 * c + 4 * lq) = acc4[rt][c] + hb[c];
  }
}

// ------------------------------------------------------------------------------------------------ weights
struct FStatLayerW {
  PackedConv pre, in[4], rs[4], proj;  // proj: proj_mean | proj_logstd as plain rows, m in output columns [0, half), s in [half, 2 half)
  int cond_col0 = 0;
  // wn_stats_kernel's fragments (width 128): the direct k = 5 planes, res/skip, proj, this layer's own pre (run by the tail of the layer before it in the call's order)
  float *W1[4] = {}, *b1[4] = {}, *W2[4] = {}, *b2[4] = {};
  float *W3 = nullptr, *b3m = nullptr, *b3s = nullptr, *W4 = nullptr, *b4 = nullptr;
};

struct FStatW {
  int fh = 0, half = 0, in_ch = 0;
  FStatLayerW layer[8];
  StyleTable cond;                     // the eight cond_layers: [2 fh * 4 per layer][style]
  PackedConv prior, pmean, plogstd;    // prior_encoder: proj_mean | proj_logstd paired (EPI_PRIOR), and each alone
  bool fused = false;                  // wn_stats_kernel's fragments are packed (width 128)
};

// wn_stats_kernel's operands of one coupling layer, every matrix in MFMA-fragment order (wn_fused.hip.h: pack_fragments)
inline int pack_wn_stats(stts_ctx* c, const std::string& q, const HostTensor& pm, const HostTensor& pl, const HostTensor& pmb, const HostTensor& plb, FStatLayerW* L) {
  const int C = kFsC;
  auto rows_of = [](const HostTensor& w) {  // [rows][K] (k = 1) as double
    const int rows = (int)w.shape[0], K = (int)(w.data.size() / rows);
    std::vector<std::vector<double>> r(rows, std::vector<double>(K));
    for (int n = 0; n < rows; ++n)
      for (int k = 0; k < K; ++k) r[n][k] = w.data[(size_t)n * K + k];
    return r;
  };
  for (int i = 0; i < 4; ++i) {
    const std::string qi = q + "enc.in_layers." + std::to_string(i), qr = q + "enc.res_skip_layers." + std::to_string(i);
    HostTensor w, wr;
    STTS_TRY(get_weight(c, qi, &w));
    std::vector<std::vector<double>> plane((size_t)kFsTaps * 2 * C, std::vector<double>(C));  // [tap][output row][cin]
    for (int k = 0; k < kFsTaps; ++k)
      for (int n = 0; n < 2 * C; ++n)
        for (int ci = 0; ci < C; ++ci) plane[(size_t)k * 2 * C + n][ci] = w.data[((size_t)n * C + ci) * kFsTaps + k];
    // wave w, tile ((tap j, half h), c): output rows h * 128 + 32 w + 16 c + col
    const std::vector<float> f1 = pack_fragments(kFsWaves, C / 16, kFsTaps * 4, [&](int wv, int t, int col) {
      return plane[(size_t)(t >> 2) * 2 * C + ((t >> 1) & 1) * C + 32 * wv + 16 * (t & 1) + col].data();
    });
    STTS_TRY(dev_upload(c, f1, &L->W1[i]));
    STTS_TRY(dev_upload(c, find(c, qi + ".bias")->data, &L->b1[i]));
    STTS_TRY(get_weight(c, qr, &wr));
    const auto rr = rows_of(wr);
    const int nct = (int)wr.shape[0] / 16 / kFsWaves;
    const std::vector<float> f2 = pack_fragments(kFsWaves, C / 16, nct, [&](int wv, int t, int col) { return rr[(size_t)16 * nct * wv + 16 * t + col].data(); });
    STTS_TRY(dev_upload(c, f2, &L->W2[i]));
    STTS_TRY(dev_upload(c, find(c, qr + ".bias")->data, &L->b2[i]));
  }
  const auto rm = rows_of(pm), rl = rows_of(pl);
  const std::vector<float> f3 = pack_fragments(kFsWaves, C / 16, 2, [&](int wv, int t, int col) { return (t == 0 ? rm : rl)[(size_t)16 * wv + col].data(); });
  STTS_TRY(dev_upload(c, f3, &L->W3));
  STTS_TRY(dev_upload(c, pmb.data, &L->b3m));
  STTS_TRY(dev_upload(c, plb.data, &L->b3s));
  HostTensor wp;
  STTS_TRY(get_weight(c, q + "pre", &wp));
  const auto rp = rows_of(wp);
  const std::vector<float> f4 = pack_fragments(kFsWaves, C / 32, 2, [&](int wv, int t, int col) { return rp[(size_t)32 * wv + 16 * t + col].data(); });
  STTS_TRY(dev_upload(c, f4, &L->W4));
  STTS_TRY(dev_upload(c, find(c, q + "pre.bias")->data, &L->b4));
  return 0;
}

inline int finalize_flow_stats(stts_ctx* c, FStatW* P) {
  *P = FStatW();
  const std::string sp = "speech_predictor.";
  const int fh = c->d.dec_hidden / 4, half = fh / 2, dh = c->d.dec_hidden;
  STTS_CHECK(fh > 0 && fh % 32 == 0, "flow statistics: decoder.hidden_dim / 4 = %d must be a multiple of 32", fh);
  P->fh = fh; P->half = half; P->in_ch = dh;
  HostTensor wm, wl;
  STTS_TRY(get_weight(c, sp + "prior_encoder.proj_mean", &wm));
  STTS_TRY(get_weight(c, sp + "prior_encoder.proj_logstd", &wl));
  STTS_GET(bm, sp + "prior_encoder.proj_mean.bias");
  STTS_GET(bl, sp + "prior_encoder.proj_logstd.bias");
  STTS_CHECK(wm.shape[0] == fh && wm.shape[1] == dh && wl.shape == wm.shape && (int)bm->data.size() == fh && (int)bl->data.size() == fh,
             "prior_encoder.proj_mean / proj_logstd: expected [%d, %d]", fh, dh);
  HostTensor wcat = wm, bcat = *bm;
  wcat.data.insert(wcat.data.end(), wl.data.begin(), wl.data.end());
  wcat.shape[0] = 2 * fh;
  bcat.data.insert(bcat.data.end(), bl->data.begin(), bl->data.end());
  STTS_TRY(pack_rows(c, wcat, &bcat, paired_rows(fh, 0, fh), 0, dh, dh, fh, &P->prior));
  STTS_TRY(pack_plain(c, sp + "prior_encoder.proj_mean", true, 0, dh, &P->pmean));
  STTS_TRY(pack_plain(c, sp + "prior_encoder.proj_logstd", true, 0, dh, &P->plogstd));
  P->cond.K = c->d.style_dim;
  const bool fused = fh == kFsC && !getenv("STTS_NO_WN_FUSED");
  for (int f = 0; f < 8; ++f) {
    const std::string q = sp + "flow.flows." + std::to_string(2 * f) + ".";
    FStatLayerW& L = P->layer[f];
    HostTensor wp;
    STTS_TRY(get_weight(c, q + "pre", &wp));
    STTS_CHECK(wp.shape[0] == fh && wp.shape[1] == half, "%spre: expected [%d, %d]", q.c_str(), fh, half);
    STTS_TRY(pack_plain(c, q + "pre", true, 0, half, &L.pre));
    for (int i = 0; i < 4; ++i) {
      const std::string qi = q + "enc.in_layers." + std::to_string(i), qr = q + "enc.res_skip_layers." + std::to_string(i);
      HostTensor w, wr;
      STTS_TRY(get_weight(c, qi, &w));
      STTS_GET(b, qi + ".bias");
      STTS_CHECK(w.shape[0] == 2 * fh && w.shape[1] == fh && w.shape[2] == 5 && (int)b->data.size() == 2 * fh, "%s: expected [%d, %d, 5]", qi.c_str(), 2 * fh, fh);
      STTS_TRY(pack_rows(c, w, b, paired_rows(fh, 0, fh), 0, fh, fh, fh, &L.in[i]));
      STTS_TRY(get_weight(c, qr, &wr));
      STTS_GET(br, qr + ".bias");
      const int n_rs = i < 3 ? 2 * fh : fh;
      STTS_CHECK(wr.shape[0] == n_rs && wr.shape[1] == fh && (int)br->data.size() == n_rs, "%s: expected [%d, %d]", qr.c_str(), n_rs, fh);
      STTS_TRY(pack_plain(c, qr, true, 0, fh, &L.rs[i]));
    }
    HostTensor pm, pl;
    STTS_TRY(get_weight(c, q + "proj_mean", &pm));
    STTS_TRY(get_weight(c, q + "proj_logstd", &pl));
    STTS_GET(pmb, q + "proj_mean.bias");
    STTS_GET(plb, q + "proj_logstd.bias");
    STTS_CHECK(pm.shape[0] == half && pm.shape[1] == fh && pl.shape == pm.shape && (int)pmb->data.size() == half && (int)plb->data.size() == half,
               "%sproj_mean / proj_logstd: expected [%d, %d]", q.c_str(), half, fh);
    HostTensor pc = pm, pcb = *pmb;
    pc.data.insert(pc.data.end(), pl.data.begin(), pl.data.end());
    pc.shape[0] = 2 * half;
    pcb.data.insert(pcb.data.end(), plb->data.begin(), plb->data.end());
    STTS_TRY(pack_rows(c, pc, &pcb, plain_rows(2 * half), 0, fh, fh, 2 * half, &L.proj));
    HostTensor cw;
    STTS_TRY(get_weight(c, q + "enc.cond_layer", &cw));
    STTS_GET(cb, q + "enc.cond_layer.bias");
    STTS_CHECK(cw.shape[0] == 8 * fh && cw.shape[1] == c->d.style_dim && (int)cb->data.size() == 8 * fh, "%senc.cond_layer: expected [%d, %d]", q.c_str(), 8 * fh,
               c->d.style_dim);
    L.cond_col0 = P->cond.add(cw, *cb);
    if (fused) STTS_TRY(pack_wn_stats(c, q, pm, pl, *pmb, *plb, &L));
  }
  STTS_TRY(upload_table(c, &P->cond));
  P->fused = fused;
  return 0;
}

// ------------------------------------------------------------------------------------------------ plan
struct FStatPlan {
  bool fused = false;
  int rows = 0;  // block height of wn_stats_kernel: 16 | 32 | 64
};

// Pure: the form of every coupling layer of a call.  Precedence: what the finalize packed (width 128, or the generic form) -> STTS_FSTAT_WN (read on
// every call: 0 = generic, 16 / 32 / 64 = wn_stats_kernel on that block height) -> the timing rule.
inline FStatPlan plan_flow_stats(const stts_ctx* c, const Seg& s) {
  const FStatW* P = static_cast<const FStatW*>(c->flow_stats.get());
  if (!P || !P->fused) return {};
  if (const char* e = getenv("STTS_FSTAT_WN")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return {true, v};
    if (v == 0 && e[0] == '0') return {};
  }
  // Measured (MI355X, tools/flow_stats_bench.py, whole stage per direction, ms; forms alternated in one process, spread <= 1 %; both directions alike):
  //     rows (blocks of 16)     generic    16      32      64
  //       960   (60)             1.466    0.634   1.034   1.857
  //      7680  (480)             1.574    1.140   1.072   1.896
  //     51200 (3200)             7.149    6.416   6.918   7.433
  // A block's time is its MFMA chain at one wave per SIMD: 19.8 / 32.3 / 58.0 us per launch at one round (7.3 + 12.5 us per 16-row tile).  One round of
  // 16-row blocks is the shortest chain.  Past it, one round of 32-row blocks beats 16-row blocks two to a CU (the 16-row kernel's 254 registers let two
  // blocks share a CU; the 32- and 64-row kernels are alone on theirs): 33.5 against 35.6 us per launch at 7680 rows.  Once the 32-row blocks need
  // more than a round the chip runs in steady state, where the two 16-row blocks per CU hide each other's prologue and epilogue: 16.0 us per tile
  // against 17.3 at 51200 rows.  The 64-row kernel is nowhere faster than the generic form (its weight prefetch and 64 accumulators leave the MFMA
  // chain no slack) and is never planned; the generic form is nowhere the faster one of the other two, so the plan keeps the fused kernel wherever it
  // is built.
  if (seg_blocks(s, 16) > 256 && seg_blocks(s, 32) <= 256) return {true, 32};
  return {true, 16};
}

// ------------------------------------------------------------------------------------------------ stage
struct FStatBufs {
  float *hf, *hf2, *outf, *acts, *ms;  // [rows, fh] each (hf2: the fused form's second h buffer; acts, ms: the generic form's)
  float* cond;                         // [n_utt, ld]
};

// (every buffer of either form is carved whatever the plan: the carving depends on the batch through rows() and n_utt only)
inline FStatBufs flow_stats_carve(const FStatW& P, const Seg& s, Arena& ws) {
  const size_t n = (size_t)s.rows() * P.fh;
  FStatBufs b;
  b.hf = ws.get<float>(n);
  b.hf2 = ws.get<float>(n);
  b.outf = ws.get<float>(n);
  b.acts = ws.get<float>(n);
  b.ms = ws.get<float>(n);
  b.cond = ws.get<float>((size_t)s.n_utt * P.cond.ld());
  return b;
}

// h_0 = pre(z half f & 1) of coupling layer f, as a plain contraction
inline int flow_stats_pre(hipStream_t st, const Seg& s, const FStatW& P, int f, const float* z, float* h) {
  const PackedConv& pre = P.layer[f].pre;
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, z, P.fh, (f & 1) * P.half, pre);
  a.N = P.fh; a.bias = pre.bias; a.Y = h; a.ldy = P.fh;
  return launch_conv_gemm(st, a, EPI_STORE, pre.npad, s.n_utt, s.max_len());
}

// Coupling layer f on the three streams in place, the generic form: reads half p = f & 1 of z, updates the other half of z / mean / logstd.
inline int flow_stats_layer(hipStream_t st, const Seg& s, const FStatW& P, int f, int reverse, float* z, float* mean, float* logstd, const FStatBufs& b) {
  const FStatLayerW& L = P.layer[f];
  const int fh = P.fh, half = P.half, n = s.n_utt, ml = s.max_len(), ld = P.cond.ld();
  STTS_TRY(flow_stats_pre(st, s, P, f, z, b.hf));
  for (int i = 0; i < 4; ++i) {
    GemmArgs g = gemm_args(s);
    set_seg(g, 0, b.hf, fh, 0, L.in[i]);
    g.N = fh; g.bias = L.in[i].bias; g.Y = b.acts; g.ldy = fh;
    g.gate = b.cond; g.ld_gate = ld; g.gcol0 = L.cond_col0 + i * 2 * fh; g.gC = fh;
    STTS_TRY(launch_conv_gemm(st, g, EPI_GATE, L.in[i].npad, n, ml));
    GemmArgs q = gemm_args(s);
    set_seg(q, 0, b.acts, fh, 0, L.rs[i]);
    q.N = L.rs[i].N; q.bias = L.rs[i].bias;
    q.D0 = b.hf; q.ldd0 = fh; q.acc0 = 1;        // h += rs[:fh]
    q.D1 = b.outf; q.ldd1 = fh; q.acc1 = i > 0;  // out (+)= rs[fh:] ; last layer: all of rs
    q.nsplit = i < 3 ? fh : 0;
    STTS_TRY(launch_conv_gemm(st, q, EPI_SPLIT_ACC, L.rs[i].npad, n, ml));
  }
  GemmArgs p = gemm_args(s);
  set_seg(p, 0, b.outf, fh, 0, L.proj);
  p.N = 2 * half; p.bias = L.proj.bias; p.Y = b.ms; p.ldy = fh;
  STTS_TRY(launch_conv_gemm(st, p, EPI_STORE, L.proj.npad, n, ml));
  const long n4 = (long)s.rows() * (half / 4);
  hipLaunchKernelGGL(flow_stats_couple_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, b.ms, fh, half, n4, reverse, z, mean, logstd, fh, (1 - (f & 1)) * half);
  STTS_HIP(hipGetLastError());
  return 0;
}

inline void launch_wn_stats(hipStream_t st, const Seg& s, int rows, bool last, WnStatsArgs& a) {
  if (s.n_utt <= kWnSegInline) {
    a.n_inline = s.n_utt;
    memcpy(a.seg_inline, s.host, (s.n_utt + 1) * sizeof(int));
  }
  const dim3 grid(ceil_div(s.max_len(), rows), s.n_utt), block(64 * kFsWaves);
  GemmProfiler& prof = gemm_profiler();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof.on) {
    const double fl = 2.0 * s.rows() * kFsC * (2.0 * kFsC * kFsTaps + (last ? 2.0 * kFsC : 2.0 * kFsC));
    prof.add("wn_stats_kernel", 0, fl, fl, 0.0);
    e0 = prof.next();
    e1 = prof.next();
  }
  wn_dispatch<16, 64, 32>(rows, [&](auto rtag) {
    constexpr int RT = decltype(rtag)::value / 16;
    if (last) STTS_LAUNCH_TIMED((wn_stats_kernel<RT, true>), grid, block, st, e0, e1, a);
    else STTS_LAUNCH_TIMED((wn_stats_kernel<RT, false>), grid, block, st, e0, e1, a);
  });
}

// Coupling layer f, the fused form: four launches.  *h holds h_0 = pre(z half f & 1) on entry; `next` >= 0: the last launch also leaves the h_0 of
// coupling layer `next` (which reads the half this one updates) in the other h buffer, and *h points at it on return.
inline int flow_stats_layer_fused(hipStream_t st, const Seg& s, const FStatW& P, int rows, int f, int next, int reverse, float* z, float* mean, float* logstd,
                                  const FStatBufs& b, float** h) {
  const FStatLayerW& L = P.layer[f];
  float *hcur = *h, *hnext = hcur == b.hf ? b.hf2 : b.hf;
  for (int i = 0; i < 4; ++i) {
    WnStatsArgs a{};
    a.Hin = hcur; a.Hout = i < 3 ? hnext : nullptr; a.Out = b.outf; a.seg_off = s.dev;
    a.W1 = L.W1[i]; a.b1 = L.b1[i]; a.W2 = L.W2[i]; a.b2 = L.b2[i];
    a.gate = b.cond; a.ld_gate = P.cond.ld(); a.gcol0 = L.cond_col0 + i * 2 * P.fh; a.out_acc = i > 0;
    if (i == 3) {
      a.tail = next >= 0 ? 2 : 1; a.reverse = reverse;
      a.W3 = L.W3; a.b3m = L.b3m; a.b3s = L.b3s;
      a.Z = z; a.Mean = mean; a.Logstd = logstd; a.ld = P.fh; a.col0 = (1 - (f & 1)) * P.half;
      if (next >= 0) { a.W4 = P.layer[next].W4; a.b4 = P.layer[next].b4; a.Hpre = hnext; }
    }
    launch_wn_stats(st, s, rows, i == 3, a);
    std::swap(hcur, hnext);  // (after layer 3: hcur = the buffer the tail wrote the next h_0 to)
  }
  STTS_HIP(hipGetLastError());
  *h = hcur;
  return 0;
}

struct FStatIO {
  int reverse;
  const float *z_in, *mean_in, *logstd_in;  // [rows, fh]
  const float* style;                       // [n_utt, style_dim]
  float *z, *mean, *logstd;                 // [rows, fh], other buffers than the inputs
};

// what the entry points check before anything is carved or launched
inline int flow_stats_check(const stts_ctx* c, const Seg& s, const FStatIO& io) {
  (void)c;
  STTS_CHECK(!s.cap, "the flow statistics take plain segments (no STTS_SEG_CAPACITY)");
  STTS_CHECK(io.reverse == 0 || io.reverse == 1, "flow_stats_forward: reverse must be 0 or 1");
  STTS_CHECK(io.z_in && io.mean_in && io.logstd_in && io.style && io.z && io.mean && io.logstd, "flow_stats_forward: null argument");
  const float* ins[3] = {io.z_in, io.mean_in, io.logstd_in};
  float* outs[3] = {io.z, io.mean, io.logstd};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) STTS_CHECK(ins[i] != outs[j] && (i == j || outs[i] != outs[j]), "flow_stats_forward: the outputs must be other buffers than the inputs and than each other");
  for (const void* ptr : {(const void*)io.z_in, (const void*)io.mean_in, (const void*)io.logstd_in, (const void*)io.style, (const void*)io.z, (const void*)io.mean, (const void*)io.logstd})
    STTS_CHECK((uintptr_t)ptr % 16 == 0, "flow_stats_forward: buffers must be 16-byte aligned");
  return 0;
}

// reverse 0: layers 0 .. 7, each followed by a Flip; reverse 1: Flip, layer 7, ..., Flip, layer 0.  After k flips the roles of the halves swap, so in
// both orders layer f reads half f & 1 and updates the other in place; after eight layers the halves are in their natural order.
inline int flow_stats_forward(stts_ctx* c, hipStream_t st, const Seg& s, const FStatIO& io, Arena& ws) {
  const FStatW& P = *static_cast<const FStatW*>(c->flow_stats.get());
  const FStatBufs b = flow_stats_carve(P, s, ws);
  STTS_CHECK(ws.ok, "flow_stats_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  const FStatPlan plan = plan_flow_stats(c, s);
  const size_t bytes = (size_t)s.rows() * P.fh * sizeof(float);
  STTS_HIP(hipMemcpyAsync(io.z, io.z_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipMemcpyAsync(io.mean, io.mean_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_HIP(hipMemcpyAsync(io.logstd, io.logstd_in, bytes, hipMemcpyDeviceToDevice, st));
  STTS_TRY(run_style(st, P.cond, io.style, s.n_utt, b.cond));
  float* h = b.hf;
  if (plan.fused) STTS_TRY(flow_stats_pre(st, s, P, io.reverse ? 7 : 0, io.z, h));
  for (int k = 0; k < 8; ++k) {
    const int f = io.reverse ? 7 - k : k, next = k == 7 ? -1 : (io.reverse ? f - 1 : f + 1);
    if (plan.fused) STTS_TRY(flow_stats_layer_fused(st, s, P, plan.rows, f, next, io.reverse, io.z, io.mean, io.logstd, b, &h));
    else STTS_TRY(flow_stats_layer(st, s, P, f, io.reverse, io.z, io.mean, io.logstd, b));
  }
  return 0;
}

// PriorEncoder.forward (flow.py:311-315): z = mean + noise exp(logstd), and mean / logstd themselves
inline int prior_stats_forward(stts_ctx* c, hipStream_t st, const Seg& s, const float* x, int ld_x, const float* noise, float* z, float* mean, float* logstd, Arena& ws) {
  const FStatW& P = *static_cast<const FStatW*>(c->flow_stats.get());
  (void)ws;  // (nothing is carved: the three contractions read x and write the outputs)
  STTS_DRY_RETURN(ws);
  const int fh = P.fh, ml = s.max_len();
  GemmArgs p = gemm_args(s);
  set_seg(p, 0, x, ld_x, 0, P.prior);
  p.N = fh; p.bias = P.prior.bias; p.Z = z; p.ldz = fh; p.noise = noise; p.ldnoise = fh;
  STTS_TRY(launch_conv_gemm(st, p, EPI_PRIOR, P.prior.npad, s.n_utt, ml));
  for (int q = 0; q < 2; ++q) {
    const PackedConv& w = q == 0 ? P.pmean : P.plogstd;
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, x, ld_x, 0, w);
    a.N = fh; a.bias = w.bias; a.Y = q == 0 ? mean : logstd; a.ldy = fh;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, w.npad, s.n_utt, ml));
  }
  return 0;
}

// sums[u] = the utterance's sum of the KL term over rows and channels, fp64, fixed order
inline int val_kl_sums(hipStream_t st, const Seg& s, int kind, const float* a, const float* b, const float* c, const float* d, int ld, int C, double* sums, Arena& ws) {
  double* part = ws.get<double>((size_t)s.rows());
  STTS_CHECK(ws.ok, "val_kl_sums: workspace too small (%ld doubles)", (long)s.rows());
  hipLaunchKernelGGL(flow_stats_kl_kernel, dim3(ceil_div(s.max_len(), 4), s.n_utt), dim3(256), 0, st, s.dev, kind, a, b, c, d, ld, C, part);
  STTS_HIP(hipGetLastError());
  hipLaunchKernelGGL(val_reduce_kernel<1>, dim3(s.n_utt), dim3(256), 0, st, part, s.dev, sums);
  STTS_HIP(hipGetLastError());
  return 0;
}

}  // namespace stts

// The flow stage: PriorEncoder + reverse flow + post_flow (models/flow.py).  Included by model.hip.h, which defines the context, the weight structs
// (WnFusedW / FlowLayerW) and the contraction launchers used here.  plan_flow() chooses the WaveNet kernel of a call (DESIGN.md states the precedence),
// fill_*() fill the kernels' argument structs, one launcher per kernel family launches, prior_flow_forward() walks the coupling layers.
#pragma once

namespace stts {

// STTS_WN_TRACE (diagnostics build only): per-wave phase stamps of the 32 fused WaveNet launches of one flow pass, averaged to stderr
#ifdef STTS_WN_TRACE
struct WnTrace {
  long long* dev = nullptr;
  long blocks[32] = {};
  static constexpr long kMax = 1024;
};
inline WnTrace& wn_trace() {
  static WnTrace t;
  return t;
}
inline long long* wn_trace_buffer(int launch, long blocks) {
  WnTrace& t = wn_trace();
  if (!t.dev) (void)hipMalloc(&t.dev, 32 * WnTrace::kMax * 64 * sizeof(long long));
  if (blocks > WnTrace::kMax) return nullptr;
  t.blocks[launch] = blocks;
  (void)hipMemsetAsync(t.dev + launch * WnTrace::kMax * 64, 0, blocks * 64 * sizeof(long long), 0);
  return t.dev + launch * WnTrace::kMax * 64;
}
inline void wn_trace_report(hipStream_t st) {
  WnTrace& t = wn_trace();
  (void)hipStreamSynchronize(st);
  static int calls = 0;
  if (++calls % 8 != 0) return;
  std::vector<long long> h(WnTrace::kMax * 64);
  for (int kind = 0; kind < 2; ++kind) {  // plain layers, last layers
    double ph[8][6] = {}, wall = 0, clk = 0;
    long n = 0;
    for (int l = 0; l < 32; ++l) {
      if ((l % 4 == 3) != (kind == 1) || !t.blocks[l]) continue;
      (void)hipMemcpy(h.data(), t.dev + l * WnTrace::kMax * 64, t.blocks[l] * 64 * sizeof(long long), hipMemcpyDeviceToHost);
      for (long b = 0; b < t.blocks[l]; ++b) {
        const long long* r0 = &h[64 * b];
        if (!r0[5]) continue;
        for (int wv = 0; wv < kWnWaves; ++wv) {
          const long long* r = r0 + 8 * wv;
          for (int i = 0; i < 6; ++i) ph[wv][i] += (double)(r[i] - r0[0]);  // cycles since wave 0 started
        }
        wall += (double)(r0[7] - r0[6]) * 10.0;  // ns
        clk += (double)(r0[5] - r0[0]);
        ++n;
      }
    }
    if (!n) continue;
    const double ghz = clk / wall;
    fprintf(stderr, "[wn trace] %s layers: %ld blocks, wave 0: %.2f us per block at %.2f GHz; per wave, us since the block started: start | prologue end | phase-1 end | gate barrier | phase-2 end | end\n",
            kind ? "last" : "plain", n, wall / n * 1e-3, ghz);
    for (int wv = 0; wv < kWnWaves; ++wv) {
      fprintf(stderr, "    wave %d:", wv);
      for (int i = 0; i < 6; ++i) fprintf(stderr, " %6.2f", ph[wv][i] / n / ghz * 1e-3);
      fprintf(stderr, "\n");
    }
  }
}
#else
inline long long* wn_trace_buffer(int, long) { return nullptr; }
inline void wn_trace_report(hipStream_t) {}
#endif

// ---- the plan: which WaveNet kernel runs the eight coupling layers of this call (one family, one block shape)
enum WnFamily {
  WN_GENERIC,        // width != 128: every layer as plain contractions
  WN_BLOCK_X3,       // wn_block_x3_kernel<shape = RT 3 | 4>: one launch per coupling layer, split fp32 (never the default, see plan_flow)
  WN_BLOCK16,        // wn_block16_kernel: one launch per coupling layer, 16-bit operands
  WN_FUSED_X3,       // wn_fused_x3_kernel<shape = RT 1 | 2 | 4, LAST, 2 x waves / 4>: per WaveNet layer, split fp32
  WN_FUSED,          // wn_fused_kernel<shape = M 1 | 2 | 4>: per WaveNet layer, f32 matrix cores
  WN_FUSED16,        // wn_fused16_kernel<shape = RT 4 | 8>: per WaveNet layer, 16-bit operands
  WN_LAYER_ROWS16,   // wn_layer_rows16_kernel: the staged kernel on 16-row blocks (fp32)
  WN_LAYER           // wn_layer_kernel<PREC>: the staged kernel on 32-row blocks
};
struct FlowPlan {
  WnFamily family;
  int shape = 0;  // RT or M of the family (above); 0 where it has one shape only
  int waves = 0;  // WN_FUSED_X3: 8 or 4
  const char* prof_name() const {
    static const char* const names[] = {"", "wn_block_kernel_x3", "wn_block16_kernel", "wn_fused_kernel_x3", "wn_fused_kernel", "wn_fused16_kernel", "wn_layer_kernel", "wn_layer_kernel"};
    return names[family];
  }
  // executed flops of a launch with `conv` flops in its k = 5 convs and `rest` elsewhere
  double exec_flops(double conv, double rest) const {
    if (family == WN_FUSED) return conv * (shape + 4) / (5.0 * shape) + rest;  // F(M,5): M + 4 instead of 5 M products per channel and group of M rows
    if (family == WN_BLOCK_X3) return (conv + rest) * (16.0 * shape) / (16.0 * shape - 16.0);  // the halo recompute (16 RT computed rows per 16 RT - 16 output rows)
    return conv + rest;
  }
};

// Tests / tools force a kernel or a block shape (0 = unset); read on every call: the tests change them between calls.  STTS_WN_M = 1 | 2 | 4:
// wn_fused_kernel's M (1: the split kernel starts from 16-row blocks too), 16: the staged 16-row kernel.  STTS_WN_RT = 4 | 8: wn_fused16_kernel's RT,
// 16: wn_block16_kernel, -1: the staged kernel.  STTS_WN_X3 = 1 | 2 | 4: wn_fused_x3_kernel's RT, -1: the f32 kernel.  STTS_WN_X3B = 3 | 4:
// wn_block_x3_kernel's RT (experiments; -1 = unset).  STTS_WN_X3_WAVES = 4: wn_fused_x3_kernel with 4 waves per block (default: eight, wn_fused_x3.hip.h).
struct WnSwitches { int m, rt, x3, x3b, x3_waves; };
inline WnSwitches wn_switches() {
  auto num = [](const char* name) { return getenv(name) ? atoi(getenv(name)) : 0; };
  return {num("STTS_WN_M"), num("STTS_WN_RT"), num("STTS_WN_X3"), num("STTS_WN_X3B"), num("STTS_WN_X3_WAVES")};
}

// blocks of `rows` rows over the utterances (no block spans two)
inline long seg_blocks(const Seg& s, int rows) {
  long b = 0;
  for (int u = 0; u < s.n_utt; ++u) b += ceil_div(s.host[u + 1] - s.host[u], rows);
  return b;
}

// Precedence, top to bottom: width -> operand precision -> which fragments the finalize packed -> a switch -> the timing rule.
inline FlowPlan plan_flow(const stts_ctx* c, const Seg& s) {
  // the fused WaveNet kernels are built for 128 flow channels (decoder.hidden_dim 512)
  if (c->d.dec_hidden / 4 != kWnC) return {WN_GENERIC};
  const WnFusedW& packed = c->flow[0].fused;
  const WnSwitches sw = wn_switches();
  // one block per CU is resident, so a launch takes ceil(blocks / 256) rounds
  auto rounds = [&](int rows) { return ceil_div((int)seg_blocks(s, rows), 256); };
  if (c->prec != PREC_F32) {
    if (!packed.ready16 || sw.rt == -1) return {WN_LAYER};
    // wn_fused16_kernel on 64- or 128-row blocks (the taller block halves the weight stream per row; it needs ~1.5 chip rounds of blocks to pay)
    const long b128 = seg_blocks(s, 128);
    int rt = b128 >= 384 ? 8 : 4;
    // at least ~0.75 chip rounds of 128-row blocks: one launch per coupling layer with h and `out` on chip (wn_block16.hip.h)
    if (b128 >= 192) rt = 16;
    if (sw.rt == 4 || sw.rt == 8 || sw.rt == 16) rt = sw.rt;
    return rt == 16 ? FlowPlan{WN_BLOCK16} : FlowPlan{WN_FUSED16, rt};
  }
  if (!packed.ready)
    // the staged kernels, 32-row or 16-row blocks: a round takes ~38 us (32 rows) or ~21 us (16 rows: half the MFMA chain, but the weight staging per
    // block is the same).  B = 8: 240 x 38 us beats 480 blocks = 2 x 21; B = 12: 720 blocks = 3 x 21 beats 360 = 2 x 38.
    return {rounds(16) * 21 < rounds(32) * 38 ? WN_LAYER_ROWS16 : WN_LAYER};
  if (sw.m == 16) return {WN_LAYER_ROWS16};  // (kept for comparison)
  // wn_fused_kernel: a round takes ~kT2 us (F(2,5), 32-row blocks) or ~kT4 us (F(4,5), 64-row blocks).  Measured (MI355X, tools/flow_bench.py): B = 8 28 us,
  // B = 16 41 us (F(4,5)) vs 55 (F(2,5)), B = 64 150 us vs 209 per WaveNet layer; staged kernels 40 / - / 287.  The same kernel in its direct form on
  // 16-row blocks (M = 1, ~kT1 us) takes the place of the staged 16-row kernel (~22 us a round) for the smallest batches (B = 1: 19.9 vs 21.1 us per layer,
  // B = 4: 22.0 vs 23.2; F(2,5) there: 25.3 / 27.4)
  constexpr int kT1 = 21, kT2 = 28, kT4 = 41;
  const int t1 = rounds(16) * kT1, t2 = rounds(32) * kT2, t4 = rounds(64) * kT4;
  int m = t4 < t2 ? 4 : 2;
  if (t1 <= std::min(t2, t4)) m = 1;
  if (sw.m == 1 || sw.m == 2 || sw.m == 4) m = sw.m;
  if (!packed.ready_x3 || sw.x3 == -1) return {WN_FUSED, m};
  // split fp32: wn_fused_x3_kernel on 32-row blocks, 64-row blocks once those fill the chip more than once (the taller block halves the weight stream
  // per row); small batches (where the f32 kernel would run M = 1) on 16-row blocks.  Fitted to 3-s batches of 8 .. 32 (us per launch): 32-row blocks
  // 4.5 + 17.5 per round, 64-row blocks (twice the matrix work per block for one weight stream) 1.5 + 29.5 per round.  B = 8: 22 vs 31; B = 10 .. 16:
  // 40 vs 31; B = 20 / 24: 57 vs 60; B = 32: 74 vs 60 - the measured optimum at every one of them
  int rt = m == 1 ? 1 : (1.5 + 29.5 * rounds(64) < 4.5 + 17.5 * rounds(32) ? 4 : 2);
  if (sw.x3 == 1 || sw.x3 == 2 || sw.x3 == 4) rt = sw.x3;
  // one launch per COUPLING layer (wn_block_x3_kernel: 32 output rows per block, 48 computed, or 48 of 64: what fits the LDS next to the fp32 residual
  // stream): built, parity-tested, NOT selected: 8 launches of 98 us against 32 of 22.6 at B = 8 - 0.79 vs 0.72 ms per step - and 1.80 vs 1.30 ms at
  // B = 16: the 2 x 8 halo rows are 1.5 x the matrix work of a 32-row block and the four layers of a block run back to back on one wave per SIMD, which
  // costs more than the 24 launch ramps + prologues it saves.
  if (sw.x3b == 3 || sw.x3b == 4) return {WN_BLOCK_X3, sw.x3b};
  return {WN_FUSED_X3, rt, sw.x3_waves == 4 ? 4 : 8};
}

// ---- one call's state, the STTS_WN_DEBUG stop, the profiler pair
// Diagnostics (tests/test_hip_flow_layers.py; read on every call, needs z_flow_out): STTS_WN_DEBUG = +-k stops after WaveNet layer k = 4 (7 - f) + i + 1
// and hands back h after that layer (+k) or `out` (-k); k = 0: the first coupling layer's h_0 = pre(z).  After a coupling layer's last WaveNet layer
// (i = 3; the fused kernels keep the finished `out` on chip) +k hands back the next coupling layer's h_0 = pre(z) (the last coupling layer, f = 0: z) and
// -k the whole z, its coupled half updated.  wn_block_x3_kernel (one launch per coupling layer) answers k = 0 and the i = 3 numbers only,
// wn_block16_kernel k = 0 only.
struct WnDebugStop {
  int n = -1000; float* dst = nullptr; size_t bytes = 0; hipStream_t st = nullptr;  // n: +-k, -1000: off; dst: z_flow_out
  bool stopped = false; int rc = 0;                                   // rc: of the hand-back
  // after WaveNet layer i of coupling layer f (i = -1: after its `pre`): true = the flow stops here, `plus` (+k) or `minus` (-k) is in z_flow_out
  // (a null buffer: this place does not answer that sign)
  bool stop(int f, int i, const float* plus, const float* minus) {
    const int k = 4 * (7 - f) + i + 1;
    const float* src = n == k ? plus : n == -k ? minus : nullptr;
    if (!src) return false;
    stopped = true;
    rc = [&]() -> int {
      STTS_HIP(hipGetLastError());  // (a launch error of the last kernel is reported, not hidden by the early return)
      STTS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
      return 0;
    }();
    return true;
  }
};

struct FlowRun {
  stts_ctx* c; hipStream_t st; const Seg& s; FlowPlan plan;
  int fh, half, ml; long R;
  // (every [rows, fh] buffer has kWnRowPad rows of slack: the fused kernels read whole 16-row tiles, also past the last utterance; never stored)
  float *z, *hf, *hf2, *outf, *acts, *cond;  // acts: the gated activations (WN_GENERIC only)
  float* blk_in;  // the per-coupling-layer kernels: this coupling layer's h_0 (ping-pongs between hf and hf2)
  WnDebugStop dbg;
  const FlowLayerW& layer(int f) const { return c->flow[f]; }
  int gcol0(int f, int i) const { return c->flow[f].cond_col0 + i * 2 * fh; }
  // algorithmic flops of WaveNet layer i of coupling layer f: its k = 5 conv; res/skip and, behind the last layer, post + coupling and the next `pre`
  double conv_flops() const { return 2.0 * (double)R * 2 * fh * 5 * fh; }
  double rest_flops(int f, int i) const {
    return 2.0 * (double)R * (double)c->flow[f].rs[i].N * fh + (i == 3 ? 2.0 * (double)R * fh * fh + (f > 0 ? 2.0 * (double)R * fh * half : 0.0) : 0.0);
  }
};

struct ProfPair { hipEvent_t e0 = nullptr, e1 = nullptr; };
inline ProfPair wn_prof(const FlowPlan& plan, double conv, double rest) {
  GemmProfiler& prof = gemm_profiler();
  if (!prof.on) return {};
  prof.add(plan.prof_name(), 0, conv + rest, plan.exec_flops(conv, rest), 0.0);
  return {prof.next(), prof.next()};
}

// ---- argument structs: the fields the kernels' structs share by name are filled in one place per group
// post + reverse coupling, and the next coupling layer's `pre` into hpre (A: any of the fused kernels' structs; Wt: float or unsigned short fragments)
template <typename A, typename Wt>
inline void fill_coupling(A& a, const FlowRun& r, int f, bool last, const Wt* w3, const Wt* w4_next, float* hpre) {
  const WnFusedW& F = r.layer(f).fused;
  a.W3 = w3; a.b3m = F.b3m; a.b3s = F.b3s;
  if (!last) return;  // (a per-layer kernel before the coupling layer's last WaveNet layer)
  a.tail = f > 0 ? 2 : 1;
  a.Z = r.z; a.ldz = r.fh; a.zcol0 = (1 - (f & 1)) * r.half;
  if (f > 0) { a.W4 = w4_next; a.b4 = r.layer(f - 1).fused.b4; a.Hpre = hpre; }
}
// WnFusedArgs<M> / WnFused16Args (also the one inside WnFusedX3Args): WaveNet layer i of coupling layer f, hin -> hout (the last layer: -> z and hpre)
template <typename A, typename Wt>
inline void fill_layer(A& a, const FlowRun& r, int f, int i, const float* hin, float* hout, float* hpre, const Wt* w1, const Wt* w2, const Wt* w3, const Wt* w4_next) {
  const WnFusedW& F = r.layer(f).fused;
  a.Hin = hin; a.Hout = i < 3 ? hout : nullptr; a.Out = r.outf; a.seg_off = r.s.dev;
  a.W1 = w1; a.b1 = F.b1[i]; a.W2 = w2; a.b2 = F.b2[i];
  a.gate = r.cond; a.ld_gate = r.c->flow_style.ld(); a.gcol0 = r.gcol0(f, i); a.out_acc = i > 0;
  fill_coupling(a, r, f, i == 3, w3, w4_next, hpre);
  if (r.s.n_utt <= kWnSegInline && !r.s.cap) {  // (the inlined offsets are the host's: not with capacity segments)
    a.n_inline = r.s.n_utt;
    memcpy(a.seg_inline, r.s.host, (r.s.n_utt + 1) * sizeof(int));
  }
}
// WnBlock16Args / WnBlockX3Args: the whole coupling layer f, blk_in -> z and hpre
template <typename A>
inline void fill_block(A& a, const FlowRun& r, int f, unsigned short* const (&w1)[4], unsigned short* const (&w2)[4], const unsigned short* w3, const unsigned short* w4_next, float* hpre) {
  const WnFusedW& F = r.layer(f).fused;
  a.Hin = r.blk_in; a.seg_off = r.s.dev; a.gate = r.cond; a.ld_gate = r.c->flow_style.ld();
  for (int i = 0; i < 4; ++i) { a.W1[i] = w1[i]; a.b1[i] = F.b1[i]; a.W2[i] = w2[i]; a.b2[i] = F.b2[i]; a.gcol0[i] = r.gcol0(f, i); }
  fill_coupling(a, r, f, true, w3, w4_next, hpre);
}

// ---- launchers: one per family.  (The code object holds the kernels in the order this file first names them: the per-coupling-layer kernels, wn_fused_x3
// RT 4, 1, 2, wn_fused M 1, 4, 2, wn_fused16, wn_layer - the order they have always had; keep it, so that a change here moves no kernel.)
// f(std::integral_constant<int, v>{}) for the v in the list that equals `value`; the last one also stands for any other value, so a launch is never skipped
template <int... Vs, typename F>
inline void wn_dispatch(int value, F&& f) {
  if (!((value == Vs) || ...)) value = std::get<sizeof...(Vs) - 1>(std::array<int, sizeof...(Vs)>{Vs...});
  (void)std::initializer_list<int>{(value == Vs ? (f(std::integral_constant<int, Vs>{}), 0) : 0)...};
}

// One launch for the whole coupling layer: reads h_0 = pre(z0) from blk_in, writes the next coupling layer's h_0 to the other buffer (neighbouring
// blocks still read their halo rows of blk_in).
inline int couple_per_block(FlowRun& r, int f) {
  const WnFusedW& F = r.layer(f).fused;
  float* blk_out = r.blk_in == r.hf ? r.hf2 : r.hf;
  double rest = 0;
  for (int i = 0; i < 4; ++i) rest += r.rest_flops(f, i);
  const ProfPair ev = wn_prof(r.plan, 4 * r.conv_flops(), rest);
  if (r.plan.family == WN_BLOCK_X3) {
    WnBlockX3Args ba{};
    fill_block(ba, r, f, F.X1, F.X2b, F.X3, f > 0 ? r.layer(f - 1).fused.X4 : nullptr, blk_out);
    ba.p1 = F.xp1; ba.p3 = F.xp3; ba.p4 = f > 0 ? r.layer(f - 1).fused.xp4 : 0;
    for (int i = 0; i < 4; ++i) ba.p2[i] = F.xp2[i];
    const dim3 grid(ceil_div(r.ml, 16 * r.plan.shape - 2 * kWnBlockX3Halo), r.s.n_utt);
    if (r.plan.shape == 3) STTS_LAUNCH_TIMED((wn_block_x3_kernel<3>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, ba);
    else STTS_LAUNCH_TIMED((wn_block_x3_kernel<4>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, ba);
    if (r.dbg.stop(f, 3, f > 0 ? blk_out : r.z, r.z)) return r.dbg.rc;
  } else {
    WnBlock16Args ba{};
    fill_block(ba, r, f, F.H1, F.H2b, F.H3, f > 0 ? r.layer(f - 1).fused.H4 : nullptr, blk_out);
    const dim3 grid(ceil_div(r.ml, kWnBlockRows), r.s.n_utt);
    if (r.c->prec == PREC_BF16) STTS_LAUNCH_TIMED((wn_block16_kernel<PREC_BF16>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, ba);
    else STTS_LAUNCH_TIMED((wn_block16_kernel<PREC_F16>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, ba);
  }
  r.blk_in = blk_out;
  STTS_HIP(hipGetLastError());
  return 0;
}

inline void launch_wn_fused_x3(const FlowRun& r, int f, int i, const float* hin, float* hout, ProfPair ev) {
  const WnFusedW& F = r.layer(f).fused;
  WnFusedX3Args xa{};
  fill_layer(xa.b, r, f, i, hin, hout, r.hf, F.X1[i], F.X2[i], F.X3, f > 0 ? r.layer(f - 1).fused.X4 : nullptr);
  xa.p1 = F.xp1; xa.p2 = F.xp2[i]; xa.p3 = F.xp3; xa.p4 = xa.b.tail > 1 ? r.layer(f - 1).fused.xp4 : 0;
  const dim3 grid(ceil_div(r.ml, 16 * r.plan.shape), r.s.n_utt);
  xa.dbg = wn_trace_buffer(f * 4 + i, (long)grid.x * grid.y);
  wn_dispatch<4, 1, 2>(r.plan.shape, [&](auto rt) {
    wn_dispatch<2 * kWnWaves, kWnWaves>(r.plan.waves, [&](auto nw) {
      constexpr int RT = decltype(rt)::value, NW = decltype(nw)::value;
      if (i == 3) STTS_LAUNCH_TIMED((wn_fused_x3_kernel<RT, true, NW>), grid, dim3(64 * NW), r.st, ev.e0, ev.e1, xa);
      else STTS_LAUNCH_TIMED((wn_fused_x3_kernel<RT, false, NW>), grid, dim3(64 * NW), r.st, ev.e0, ev.e1, xa);
    });
  });
}

inline void launch_wn_fused(const FlowRun& r, int f, int i, const float* hin, float* hout, ProfPair ev) {
  const WnFusedW& F = r.layer(f).fused;
  wn_dispatch<1, 4, 2>(r.plan.shape, [&](auto mtag) {
    constexpr int M = decltype(mtag)::value;
    WnFusedArgs<M> fa{};
    fill_layer(fa, r, f, i, hin, hout, r.hf, F.W1[M == 2 ? 0 : (M == 4 ? 1 : 2)][i], F.W2[i], F.W3, f > 0 ? r.layer(f - 1).fused.W4 : nullptr);
    const dim3 grid(ceil_div(r.ml, 16 * M), r.s.n_utt);
    fa.dbg = wn_trace_buffer(f * 4 + i, (long)grid.x * grid.y);
    if (i == 3) STTS_LAUNCH_TIMED((wn_fused_kernel<M, true>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, fa);
    else STTS_LAUNCH_TIMED((wn_fused_kernel<M, false>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, fa);
  });
}

inline void launch_wn_fused16(const FlowRun& r, int f, int i, const float* hin, float* hout, ProfPair ev) {
  const WnFusedW& F = r.layer(f).fused;
  WnFused16Args fa{};
  fill_layer(fa, r, f, i, hin, hout, r.hf, F.H1[i], F.H2[i], F.H3, f > 0 ? r.layer(f - 1).fused.H4 : nullptr);
  wn_dispatch<PREC_BF16, PREC_F16>(r.c->prec, [&](auto prec) {
    wn_dispatch<8, 4>(r.plan.shape, [&](auto rt) {
      constexpr int RT = decltype(rt)::value, P = decltype(prec)::value;
      const dim3 grid(ceil_div(r.ml, 16 * RT), r.s.n_utt);
      if (i == 3) STTS_LAUNCH_TIMED((wn_fused16_kernel<P, RT, true>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, fa);
      else STTS_LAUNCH_TIMED((wn_fused16_kernel<P, RT, false>), grid, dim3(64 * kWnWaves), r.st, ev.e0, ev.e1, fa);
    });
  });
}

// the staged kernels (wn_layer.hip.h; fp32 small batches: 16-row blocks, twice the workgroups at half the chain length, wn_layer_small.hip.h)
inline void launch_wn_layer(const FlowRun& r, int f, int i, const float* hin, float* hout, ProfPair ev) {
  const FlowLayerW& L = r.layer(f);
  const int prec = r.c->prec;
  auto wptr = [&](const PackedConv& pc) -> const void* { return prec != PREC_F32 ? (const void*)pc.W16 : (const void*)pc.W; };
  WnArgs w;
  w.Hin = hin; w.Hout = i < 3 ? hout : nullptr; w.Out = r.outf; w.seg_off = r.s.dev;
  w.Win = wptr(L.in[i]); w.bin = L.in[i].bias; w.Wrs = wptr(L.rs[i]); w.brs = L.rs[i].bias;
  w.gate = r.cond; w.ld_gate = r.c->flow_style.ld(); w.gcol0 = r.gcol0(f, i); w.n_rs = L.rs[i].N; w.out_acc = i > 0;
  w.tail = 0; w.Wproj = w.Wpre = nullptr; w.bproj = w.bpre = nullptr; w.Z = w.Hpre = nullptr; w.ldz = w.zcol0 = 0;
  if (i == 3) {
    w.tail = f > 0 ? 2 : 1;
    w.Wproj = wptr(L.proj); w.bproj = L.proj.bias; w.Z = r.z; w.ldz = r.fh; w.zcol0 = (1 - (f & 1)) * r.half;
    if (f > 0) { w.Wpre = wptr(r.layer(f - 1).pre); w.bpre = r.layer(f - 1).pre.bias; w.Hpre = r.hf; }
  }
  const dim3 grid(ceil_div(r.ml, 32), r.s.n_utt);
  if (r.plan.family == WN_LAYER_ROWS16) STTS_LAUNCH_TIMED(wn_layer_rows16_kernel, dim3(ceil_div(r.ml, 16), r.s.n_utt), dim3(1024), r.st, ev.e0, ev.e1, w);
  else if (prec == PREC_BF16) STTS_LAUNCH_TIMED(wn_layer_kernel<PREC_BF16>, grid, dim3(1024), r.st, ev.e0, ev.e1, w);
  else if (prec == PREC_F16) STTS_LAUNCH_TIMED(wn_layer_kernel<PREC_F16>, grid, dim3(1024), r.st, ev.e0, ev.e1, w);
  else STTS_LAUNCH_TIMED(wn_layer_kernel<PREC_F32>, grid, dim3(1024), r.st, ev.e0, ev.e1, w);
}

// One launch per WaveNet layer: conv k5 + gate + res/skip + h/out update; the last one also applies the coupling layer's post projection + reverse
// coupling and the next coupling layer's pre projection to its rows (into hf: layer 3 reads hf2, hf is free and is the next coupling layer's h_0).
inline int couple_per_layer(FlowRun& r, int f) {
  float *hcur = r.hf, *hnext = r.hf2;
  for (int i = 0; i < 4; ++i) {
    const ProfPair ev = wn_prof(r.plan, r.conv_flops(), r.rest_flops(f, i));
    if (r.plan.family == WN_FUSED_X3) launch_wn_fused_x3(r, f, i, hcur, hnext, ev);
    else if (r.plan.family == WN_FUSED) launch_wn_fused(r, f, i, hcur, hnext, ev);
    else if (r.plan.family == WN_FUSED16) launch_wn_fused16(r, f, i, hcur, hnext, ev);
    else launch_wn_layer(r, f, i, hcur, hnext, ev);
    if (i < 3 ? r.dbg.stop(f, i, hnext, r.outf) : r.dbg.stop(f, i, f > 0 ? r.hf : r.z, r.z)) return r.dbg.rc;
    std::swap(hcur, hnext);
  }
  STTS_HIP(hipGetLastError());
  return 0;
}

// the coupling layer's `pre` into hf (generic: every coupling layer; the fused kernels: the first one, later ones come out of the previous tail)
inline int flow_pre(FlowRun& r, int f) {
  const PackedConv& pre = r.layer(f).pre;
  GemmArgs a = gemm_args(r.s);
  set_seg(a, 0, r.z, r.fh, (f & 1) * r.half, pre);
  a.N = r.fh; a.bias = pre.bias; a.Y = r.hf; a.ldy = r.fh;
  STTS_TRY(launch_conv_gemm(r.st, a, EPI_STORE, pre.npad, r.s.n_utt, r.ml));
  if (r.dbg.stop(f, -1, r.hf, nullptr)) return r.dbg.rc;  // k = 0, or the previous coupling layer's +k at i = 3
  return 0;
}

// ResidualCouplingLayer.forward(reverse) as plain contractions (flow.py:196-218, WN :63-88): pre -> 4 x {conv k5 with the gate in its epilogue,
// res/skip with the h / out split in its epilogue} -> post with the coupling in its epilogue; the gated activations pass through memory
inline int couple_generic(FlowRun& r, int f) {
  const FlowLayerW& L = r.layer(f);
  const int fh = r.fh, n = r.s.n_utt;
  STTS_TRY(flow_pre(r, f));
  if (r.dbg.stopped) return 0;
  for (int i = 0; i < 4; ++i) {
    GemmArgs g = gemm_args(r.s);
    set_seg(g, 0, r.hf, fh, 0, L.in[i]);
    g.N = fh; g.bias = L.in[i].bias; g.Y = r.acts; g.ldy = fh;
    g.gate = r.cond; g.ld_gate = r.c->flow_style.ld(); g.gcol0 = r.gcol0(f, i); g.gC = fh;
    STTS_TRY(launch_conv_gemm(r.st, g, EPI_GATE, L.in[i].npad, n, r.ml));
    GemmArgs q = gemm_args(r.s);
    set_seg(q, 0, r.acts, fh, 0, L.rs[i]);
    q.N = L.rs[i].N; q.bias = L.rs[i].bias;
    q.D0 = r.hf; q.ldd0 = fh; q.acc0 = 1;        // h += rs[:fh]   (every row tile reads only its own rows of `acts`)
    q.D1 = r.outf; q.ldd1 = fh; q.acc1 = i > 0;  // out (+)= rs[fh:] ; last layer: all of rs
    q.nsplit = L.rs[i].N == 2 * fh ? fh : 0;
    STTS_TRY(launch_conv_gemm(r.st, q, EPI_SPLIT_ACC, L.rs[i].npad, n, r.ml));
    if (i < 3 && r.dbg.stop(f, i, r.hf, r.outf)) return r.dbg.rc;
  }
  GemmArgs q = gemm_args(r.s);
  set_seg(q, 0, r.outf, fh, 0, L.proj);
  q.N = r.half; q.bias = L.proj.bias; q.Z = r.z; q.ldz = fh; q.zcol0 = (1 - (f & 1)) * r.half;
  STTS_TRY(launch_conv_gemm(r.st, q, EPI_COUPLE, L.proj.npad, n, r.ml));
  if (r.dbg.stop(f, 3, f == 0 ? r.z : nullptr, r.z)) return r.dbg.rc;
  return 0;
}

// ---- stage: PriorEncoder + reverse flow + post_flow (models/flow.py:311-315, :132-151, :196-218, :63-88)
inline int prior_flow_forward(stts_ctx* c, hipStream_t st, const Seg& s, const float* x, int ld_x, const float* style, const float* noise,
                              float* mel, int ld_mel, float* z_prior_out, float* z_flow_out, Arena& ws, unsigned short* mel16 = nullptr,
                              int ld_mel16 = 0) {
  // mel16: also write mel rounded to the operand precision (the vocoder's projector reads it; 16-bit modes, large batches)
  const int fh = c->d.dec_hidden / 4;
  FlowRun r{c, st, s, plan_flow(c, s), fh, fh / 2, s.max_len(), s.rows()};
  const size_t wide = (size_t)(r.R + kWnRowPad) * fh;
  r.z = ws.get<float>(wide);
  r.hf = r.blk_in = ws.get<float>(wide);
  r.hf2 = ws.get<float>(wide);
  r.outf = ws.get<float>(wide);
  r.acts = r.plan.family == WN_GENERIC ? ws.get<float>(r.R * fh) : nullptr;
  r.cond = ws.get<float>((size_t)s.n_utt * c->flow_style.ld());
  STTS_CHECK(ws.ok, "prior_flow_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  if (getenv("STTS_WN_DEBUG") && z_flow_out) r.dbg = WnDebugStop{atoi(getenv("STTS_WN_DEBUG")), z_flow_out, r.R * fh * sizeof(float), st};
  STTS_TRY(run_style(st, c->flow_style, style, s.n_utt, r.cond));
  GemmArgs p = gemm_args(s);
  set_seg(p, 0, x, ld_x, 0, c->prior);
  p.N = fh; p.bias = c->prior.bias; p.Z = r.z; p.ldz = fh; p.noise = noise; p.ldnoise = fh;
  STTS_TRY(launch_conv_gemm(st, p, EPI_PRIOR, c->prior.npad, s.n_utt, r.ml));
  if (z_prior_out) STTS_HIP(hipMemcpyAsync(z_prior_out, r.z, r.R * fh * sizeof(float), hipMemcpyDeviceToDevice, st));
  // reversed(flows) = Flip, layer 7, Flip, layer 6, ..., Flip, layer 0: after k flips the roles of the halves swap,
  // so layer f reads half p = (f odd) and updates the other half in place; after layer 0 the order is natural.
  if (r.plan.family != WN_GENERIC) STTS_TRY(flow_pre(r, 7));
  for (int f = 7; f >= 0 && !r.dbg.stopped; --f) {
    if (r.plan.family == WN_GENERIC) STTS_TRY(couple_generic(r, f));
    else if (r.plan.family == WN_BLOCK_X3 || r.plan.family == WN_BLOCK16) STTS_TRY(couple_per_block(r, f));
    else STTS_TRY(couple_per_layer(r, f));
  }
  if (r.dbg.stopped) return 0;
  if (r.plan.family == WN_FUSED || r.plan.family == WN_FUSED_X3 || r.plan.family == WN_BLOCK_X3) wn_trace_report(st);
  if (z_flow_out) STTS_HIP(hipMemcpyAsync(z_flow_out, r.z, r.R * fh * sizeof(float), hipMemcpyDeviceToDevice, st));
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, r.z, fh, 0, c->post_flow);
  a.N = c->d.dec_hidden; a.bias = c->post_flow.bias; a.Y = mel; a.ldy = ld_mel;
  if (mel16 && c->post_flow.prec != PREC_F32) { a.Y16 = mel16; a.ldy16 = ld_mel16; }
  STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, c->post_flow.npad, s.n_utt, r.ml));
  if (mel16 && c->post_flow.prec == PREC_F32) launch_cast_rows(st, c->prec, mel, ld_mel, c->d.dec_hidden, mel16, ld_mel16, r.R);
  return 0;
}

}  // namespace stts

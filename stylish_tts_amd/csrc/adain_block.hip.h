// The AdaptiveDecoderBlock stage (models/ada_norm.py:166-182) and Decoder.forward (models/decoder.py:47-60).  Included by model.hip.h, which defines the
// context, the weight structs (AdainBlockW) and the contraction / Winograd launchers used here.  block_switches() reads the STTS_* switches,
// plan_adain_chain() / plan_adain_block() choose the form of a chain and of each block (DESIGN.md 4 states the precedence; no launches, no HIP calls),
// run_adain_block() executes a plan, BlockChain carries what one block hands to the next, decoder_forward() walks the decoder's five blocks.
#pragma once

namespace stts {

// ---- the switches: experiments and comparisons
struct BlockSwitches {
  // read ONCE per process
  long fold_rows;         // STTS_FOLD_ROWS: batches up to this many rows fold AdaIN into the consuming contraction's staging; above it the fp32 convs run in Winograd form
  long fold16_rows;       // the same limit in the 16-bit operand modes (no environment switch: 4 096, measured at that size only; tests move it through stts_op_adain_chain)
  long rows16;            // STTS_ROWS16: rows from which the 16-bit operand modes keep contraction inputs as 16-bit rows in HBM
  long sc_side_min_rows;  // STTS_SC_SIDE_MIN_ROWS: rows from which the decoder's learned shortcuts run on the side lane
  bool affine_serial;     // STTS_AFFINE_SERIAL: the one-thread-per-channel merge of the chunk statistics (adain_affine_kernel)
  bool no_wino_conv2sc;   // STTS_NO_WINO_CONV2SC: a conv2 with a learned shortcut stays one direct contraction (the shortcut as its second K segment)
  bool no_stat_fuse;      // STTS_NO_STAT_FUSE: 16-bit modes, every norm runs its own statistics pass
  bool no_wino_stats;     // STTS_NO_WINO_STATS: the fp32 Winograd branch runs a statistics pass per norm
  // read per call (tests change it between calls)
  int bridge;             // STTS_ADAIN_BRIDGE: 0 = never, 1 = wherever winograd_bridge_kernel can run, -1 (unset) = the rule of plan_adain_chain
  bool x3_presplit;       // STTS_X3_PRESPLIT: pre-split input planes, a layout the bridge does not write
};
// Measured thresholds.  rows16 (B = 4 x 3 s; bf16, 3-s utterances: B = 1: 827 vs 739 utt/s without / with 16-bit rows, B = 2: 1 424 vs 1 313, B = 4: 2 272 vs
// 2 304, B = 8: 3 442 vs 3 522).  (The B = 4 pair dates from when 3 840 .. 4 096 rows planned 16-bit rows under folded
// contractions and timed a wrong result.  With the window folded on fp32 rows, B = 4 x 3 s runs at 2 509 / 2 525 utt/s in
// bf16 and 2 549 / 2 524 in f16: bench.py --batch 4, 30 steps, two runs each.)  sc_side_min_rows (3-s utterances, same box, alternated): B = 16: 5.82 -> 5.74 ms per step (+1.4 %); B = 8: 3.505 -> 3.52
// (-0.5 %), B = 4: 2.39 -> 2.42 (-1.3 %): below ~12 000 rows the two cross-queue waits per block cost what the overlap gains.
inline BlockSwitches block_switches() {
  static const BlockSwitches once = [] {
    auto num = [](const char* name, long unset) { return getenv(name) ? atol(getenv(name)) : unset; };
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    return BlockSwitches{num("STTS_FOLD_ROWS", 2500), 4096, num("STTS_ROWS16", 3840), num("STTS_SC_SIDE_MIN_ROWS", 12000), set("STTS_AFFINE_SERIAL"), set("STTS_NO_WINO_CONV2SC"),
                         set("STTS_NO_STAT_FUSE"), set("STTS_NO_WINO_STATS"), -1, false};
  }();
  BlockSwitches sw = once;
  const char* bridge = getenv("STTS_ADAIN_BRIDGE");
  sw.bridge = bridge ? (atoi(bridge) != 0) : -1;
  sw.x3_presplit = getenv("STTS_X3_PRESPLIT") && atoi(getenv("STTS_X3_PRESPLIT")) != 0;
  return sw;
}
inline long rows16_threshold() { return block_switches().rows16; }
inline long fold_rows() { return block_switches().fold_rows; }

// ---- the two small launches every form shares
inline size_t adain_part_floats(const Seg& s, int C, int chunk_rows = kStatChunk) { return (size_t)s.n_utt * ceil_div(s.max_len(), chunk_rows) * 2 * round_up(C, 32); }
// chunk statistics of X[:, :C] into `part` (ldp floats per row, chunks of chunk_rows rows: kStatChunk, or kWinoStatChunk for what merges with a Winograd output transform's)
inline void launch_adain_partial(hipStream_t st, const Seg& s, const float* X, int ldx, int C, float* part, int ldp, int chunk_rows) {
  const int nchunk = ceil_div(s.max_len(), chunk_rows);
  STTS_LAUNCH_PROF("adain_partial_kernel", (size_t)s.rows() * C * 4, adain_partial_kernel, dim3(ceil_div(C, 32), nchunk, s.n_utt), dim3(256), st, X, ldx, C, s.dev, part, ldp, nchunk, chunk_rows);
}
// chunk statistics (round_up(C, 32) floats per row) + style -> the per-(utterance, channel) scale / shift table `aff` that a contraction's staging or a Winograd
// input transform applies; serial: the one-thread-per-channel merge
inline void launch_adain_affine(hipStream_t st, const Seg& s, const float* part, int C, int chunk_rows, bool serial, const float* style_out, int ld_style, int gcol0, float* aff, int ld_aff) {
  const int nchunk = ceil_div(s.max_len(), chunk_rows), ldp = round_up(C, 32);
  if (serial)
    STTS_LAUNCH_PROF("adain_affine_kernel", (size_t)s.n_utt * nchunk * 2 * ldp * 4, adain_affine_kernel, dim3(ceil_div(ld_aff, 64), s.n_utt), dim3(64), st, part, ldp, nchunk, s.dev, style_out, ld_style, gcol0, C,
                     1e-5f, aff, ld_aff, chunk_rows);
  else
    STTS_LAUNCH_PROF("adain_affine_lanes_kernel", (size_t)s.n_utt * nchunk * 2 * ldp * 4, adain_affine_lanes_kernel, dim3(ceil_div(ld_aff, 16), s.n_utt), dim3(256), st, part, ldp, nchunk, s.dev, style_out,
                     ld_style, gcol0, C, 1e-5f, aff, ld_aff, chunk_rows);
}

// AdaIN + activation: Y[:, :ldy] = act((1+gamma) * InstanceNorm(X[:, :C]) + beta), zeros in the pad columns.
// part: scratch of adain_part_floats(s, C) floats.
// out16: PREC_BF16 / PREC_F16 = Y is a 16-bit row buffer (ldy in elements), the input of a contraction in that operand mode
inline int run_adain(hipStream_t st, const Seg& s, const float* X, int ldx, int C, float* Y, int ldy, const float* style_out, int ld_style,
                     int gcol0, int act, const float* alpha, float* part, int out16 = 0, bool have_stats = false, int force_rb = 0) {
  // force_rb (tests: stts_op_adain): 64 or 256 rows per apply block whatever the batch; have_stats: `part` already holds the chunk statistics of X (written by the producing contraction's epilogue, GemmArgs::stat_part)
  const int nchunk = ceil_div(s.max_len(), kStatChunk), ldp = round_up(C, 32);
  if (!have_stats) launch_adain_partial(st, s, X, ldx, C, part, ldp, kStatChunk);
  const int rb = force_rb ? force_rb : (long)ceil_div(ldy, 64) * ceil_div(s.rows(), 64) >= 4096 ? 256 : 64;  // rows per block
  STTS_LAUNCH_PROF("adain_apply_kernel", (size_t)s.rows() * (C * 4 + ldy * (out16 ? 2 : 4)), adain_apply_kernel, dim3(ceil_div(ldy, 64), ceil_div(s.max_len(), rb), s.n_utt), dim3(256), st, X, ldx, Y, ldy, C, s.dev,
                   part, ldp, nchunk, style_out, ld_style, gcol0, 1e-5f, act, alpha, out16, rb);
  STTS_HIP(hipGetLastError());
  return 0;
}

// A contraction whose split-K reduce pass is left to the consumer of its output (small batches: the next AdaIN's statistics kernel finishes it).
struct PendingReduce {
  SplitSrc src{};   // src.partial == nullptr: nothing pending
  float* Y = nullptr;
  int ldy = 0;
};
inline void pending_from(PendingReduce* p, const SplitInfo& info, const GemmArgs& a) {
  p->src = SplitSrc{};
  if (info.ksplit > 1) {
    p->src = SplitSrc{info.partial, info.ksplit, info.slice_rows, info.ld_part, a.N, a.bias, a.act, a.R, a.ldr, a.rcol0, a.alpha};
    p->Y = a.Y + a.ycol0;
    p->ldy = a.ldy;
  }
}
// finishes a pending reduce on its own (no consumer took it)
inline int pending_finish(hipStream_t st, PendingReduce* p) {
  if (!p->src.partial) return 0;
  const SplitSrc& r = p->src;
  const long work = (long)r.slice_rows * ((r.N + 3) / 4);
  STTS_LAUNCH_PROF("splitk_reduce_kernel", (size_t)work * 4 * 4 * (r.ksplit + 1), splitk_reduce_kernel, dim3((unsigned)std::min<long>(2048, (work + 255) / 256)), dim3(256), st, r.partial,
                   r.ksplit, r.slice_rows, 0, r.ld_part, r.N, r.bias, r.act, r.R, r.ldr, r.rcol0, r.alpha, p->Y, p->ldy, 0);
  p->src = SplitSrc{};
  STTS_HIP(hipGetLastError());
  return 0;
}

// A second stream for a contraction that is independent of the launches around it (the learned 1x1 shortcut next to conv1), with the
// fork / join events that order it against the caller's stream and an output buffer of its own ([rows, cout]).
struct SideWork {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  float* out = nullptr;
};

// ---- the chain: what a run of blocks shares and what one block hands to the next
// fp32 Winograd branch of the decoder: the slab width of winograd_bridge_kernel (one launch between an AdaIN block's chained convs), or 0 for the three
// launches (output transform with statistics, affine table, input transform).  A bridge block holds the whole time axis of its utterance, so the launch
// pays only when (utterances x slabs) covers a good part of the chip, and stops paying once there are more blocks than the chip holds at a time (two of
// ten waves per CU at 3-s utterances).  Rule: 96 <= utterances x (hidden_dim / 16) <= 384, i.e. 3 to 12 utterances at 512 channels, every utterance at most 1 536 rows.
// Measured per step, three launches -> bridge, 3-s utterances, same box, same build, alternated: B = 3: 2.112 -> 2.057 ms (-2.6 %), B = 4: 2.312 -> 2.241
// (-3.1 %), B = 6: 2.737 -> 2.665 (-2.6 %), B = 8: 3.246 -> 3.198 (-1.5 %), B = 12: 4.349 -> 4.317 (-0.7 %), B = 16: 5.538 -> 5.546 (+0.1 %: stays); cfg4
// (256 ragged utterances, calls of more than 12): 150.0 vs 149.8 ms forced on (stays); B = 1, 2 and a single 10-s utterance never reach the Winograd
// branch or exceed a block.
constexpr int kBridgeSlab = 16;
constexpr int kBridgeMinBlocks = 96, kBridgeMaxBlocks = 384;

// what the caller of a chain can offer beyond the blocks' scratch
struct ChainOffer {
  bool stats;      // buffers for statistics that the producers leave behind (BlockChain::in / mid / out)
  bool rows16;     // 16-bit copies of the blocks' inputs for the learned shortcuts
  bool bridge;     // every block's output feeds the next block's conv1 directly: winograd_bridge_kernel may chain them
  bool side_lane;  // a second stream for the learned shortcuts
};
struct ChainPlan {
  bool wino = false;        // Winograd scratch: the k = 3 convs that have a Winograd form run in it
  bool sc_out = false;      // ... and a buffer for the learned shortcuts' outputs (carved whenever the Winograd branch may run, so the size does not depend on the caller's streams)
  bool rows16 = false;      // 16-bit modes: the activations are 16-bit rows, the shortcuts read rounded copies of the blocks' inputs
  bool wino_stats = false;  // fp32 Winograd branch: statistics from the convs' output transforms (chunks of kWinoStatChunk rows)
  bool stats = false;       // the blocks hand statistics on at all (16-bit rows: from the contractions' epilogues)
  int bridge_w = 0;         // slab width of the one-launch bridge between chained Winograd convs, 0: three launches
  bool side = false;        // the learned shortcuts run on the side lane
};
// blocks[probe]: the block whose conv1 sizes the Winograd scratch.  Precedence, top to bottom: rows and packed forms -> what the caller offers -> a switch -> the timing rule.
inline ChainPlan plan_adain_chain(const Seg& s, int prec, const AdainBlockW* blocks, int nblocks, int probe, const ChainOffer& offer, const BlockSwitches& sw) {
  ChainPlan p;
  const long R = s.rows();
  // conv1 of every block in Winograd form once the batch is large enough to be throughput-bound (B = 1: 35 vs 30 us)
  p.wino = R > sw.fold_rows && blocks[probe].w1.ready;
  p.sc_out = p.wino && blocks[probe].sc.W;
  // (as plan_adain_block: a folded block keeps fp32 rows, so up to fold16_rows nothing reads the 16-bit copies and the chain carves and casts none)
  p.rows16 = offer.rows16 && R >= sw.rows16 && R > sw.fold16_rows && prec != PREC_F32 && blocks[probe].cout % 8 == 0;
  p.wino_stats = offer.stats && prec == PREC_F32 && p.wino && !sw.no_wino_stats;
  p.stats = (p.rows16 && !sw.no_stat_fuse) || p.wino_stats;
  p.side = offer.side_lane && p.sc_out && R >= sw.sc_side_min_rows;
  if (!offer.bridge || !p.wino_stats || sw.bridge == 0 || sw.x3_presplit) return p;
  for (int i = 0; i < nblocks; ++i) {  // the kernel can run: every conv pair of the chain fits a bridge block
    const AdainBlockW& B = blocks[i];
    if (!wino_bridge_fits(s, B.w1, B.w2, kBridgeSlab) || B.w2.planes.kc != B.cout) return p;
    if (i + 1 < nblocks && (!wino_bridge_fits(s, B.w2, blocks[i + 1].w1, kBridgeSlab) || blocks[i + 1].cin < B.cout)) return p;
  }
  const long nb = (long)s.n_utt * (blocks[0].cout / kBridgeSlab);
  if (sw.bridge == 1 || (nb >= kBridgeMinBlocks && nb <= kBridgeMaxBlocks)) p.bridge_w = kBridgeSlab;
  return p;
}

// The state that travels along a chain.  The runner reads in / in_ready / planes_ready and sets out_ready / planes_ready; the caller links the buffers
// before each block.  `pend`: a block's conv2 may leave its split-K reduce pass to the next block's first statistics launch (small batches).
struct BlockChain {
  bool stats = false;           // off: every norm runs its own statistics pass, nothing below is read
  bool defer = false;           // the caller finishes `pend` after the last block (finish())
  int chunk_rows = kStatChunk;  // kWinoStatChunk: fp32 Winograd branch, the statistics come out of the convs' output transforms (winograd_output_kernel<N, true>)
  int bridge_w = 0;             // ChainPlan::bridge_w: the statistics never leave the bridge block that reduces them, `mid` and `out` stay unused
  float* in = nullptr;          // statistics of x for norm1 (layout of adain_partial_kernel, round_up(cin, 32) columns)
  bool in_ready = false;
  float* mid = nullptr;         // scratch: statistics of conv1's output for norm2
  float* out = nullptr;         // where conv2 writes the statistics of y (out_ld columns per row: the next block's padded input width, whose constant columns the caller fills)
  int out_ld = 0;
  bool out_ready = false;
  const AdainBlockW* next = nullptr;  // bridge: the block whose conv1 consumes this block's output (null: the output transform writes y, nothing follows)
  const float* cst = nullptr;         // bridge: chunk statistics of the next block's constant input columns (layout of `in`, cst_ld columns)
  int cst_ld = 0;
  bool planes_ready = false;          // the previous block's bridge has written conv1's input planes
  PendingReduce pend;

  BlockChain() = default;
  BlockChain(const ChainPlan& p, float* mid_) : stats(p.stats), chunk_rows(p.wino_stats ? kWinoStatChunk : kStatChunk), bridge_w(p.bridge_w), mid(mid_) {}
  // before a block: norm1's statistics (ready = its producer left them), where conv2 leaves those of y, and the block that follows
  void link(float* in_, bool ready, float* out_, int out_ld_, const AdainBlockW* next_) {
    in = in_; in_ready = ready; out = out_; out_ld = out_ld_; next = next_;
  }
  int finish(hipStream_t st) { return pending_finish(st, &pend); }  // the last block's output has no AdaIN behind it
};

// ---- the plan of one block
enum BlockConv { CONV_FOLD, CONV_APPLY, CONV_WINO, CONV_WINO_BRIDGED };
// CONV_FOLD          direct contraction, AdaIN -> LeakyReLU folded into its staging (conv_gemm_f32<..., XAFF>): the normalised tensor is never written
// CONV_APPLY         direct contraction behind a separate apply pass (adain_apply_kernel)
// CONV_WINO          Winograd F(6,3), AdaIN -> LeakyReLU in its input transform
// CONV_WINO_BRIDGED  Winograd planes written by winograd_bridge_kernel (conv1: the previous block's second bridge, conv2: this block's first)
enum StatFrom { STAT_PASS, STAT_EPILOGUE, STAT_WINO, STAT_BRIDGE };  // own adain_partial_kernel pass | producer's conv_gemm16_kernel epilogue | Winograd output transform | inside the bridge
enum ShortcutAt { SC_IDENTITY, SC_SEGMENT, SC_STREAM, SC_SIDE };     // no learned shortcut (residual = x) | conv2's second K segment | own launch on the stream | on the side lane
enum Y16By { Y16_NONE, Y16_EPILOGUE, Y16_CAST };                     // the rounded copy of y: not wanted | conv2's epilogue | a cast pass
struct BlockPlan {
  BlockConv conv1 = CONV_FOLD, conv2 = CONV_FOLD;
  int rows16 = 0;                 // PREC_BF16 / PREC_F16: the apply passes write 16-bit rows and a learned shortcut reads the 16-bit copy of x; 0: fp32 rows
  StatFrom norm1 = STAT_PASS, norm2 = STAT_PASS;
  StatFrom next_norm1 = STAT_PASS;  // what conv2 leaves of y's statistics (STAT_PASS: nothing, the next norm1 runs its own pass)
  bool take_pending = false;      // norm1's statistics launch finishes the chain's pending reduce (else it is finished on its own first)
  bool defer_conv2 = false;       // conv2's split-K reduce is left to the chain
  ShortcutAt shortcut = SC_IDENTITY;
  bool cast_x16 = false;          // the 16-bit copy of x is not there yet: cast it
  Y16By y16 = Y16_NONE;
  bool affine_serial = false;
  int bridge_w = 0;
  int force_tile = 0;             // tile of the direct contractions (tests; any value keeps the block off the Winograd and 16-bit-row forms)
};

// buffers of one block.  x [rows, ldx] (cols >= cin may hold anything when kcin == round_up(cin) because the packed weights are zero there, but AdaIN writes zeros
// anyway).  scratch: act1 [rows, kcin], hbuf [rows, cout], act2 [rows, cout], ss [adain_part_floats(s, max(kcin, cout))]
struct BlockIO {
  const float *style = nullptr, *x = nullptr;  // style: the style table's output [n_utt, ld_style]
  float* y = nullptr;
  int ld_style = 0, ldx = 0, ldy = 0;
  float *act1 = nullptr, *hbuf = nullptr, *act2 = nullptr, *ss = nullptr;
  WinoScratch* wino = nullptr;     // null or empty: no Winograd form
  unsigned short* xs16 = nullptr;  // [rows, ldx] 16-bit scratch for the rounded copy of x a learned shortcut reads (16-bit modes, large batches)
  bool xs16_ready = false;         // it already holds that copy (the previous block's conv2 wrote it)
  unsigned short* y16 = nullptr;   // also write y rounded, as [rows, ldy16] (cout % 8 == 0: caller)
  int ldy16 = 0;
  const SideWork* side = nullptr;  // null: the learned shortcut stays on the caller's stream
};

// would launch_conv_gemm take conv_gemm16_kernel for a block's contraction?  (the arguments the runner will fill, without the buffers)
inline bool block_conv_on_gemm16(const Seg& s, const PackedConv& w, int ldx, const PackedConv* sc, int ld_sc, int N, int ldr, int ldy, int ldy16) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.seg_host = s.host; g.x16 = true; g.N = N; g.ldr = ldr; g.ldy = ldy; g.ldy16 = ldy16;
  set_seg(g, 0, nullptr, ldx, 0, w);
  if (sc) set_seg(g, 1, nullptr, ld_sc, 0, *sc);
  return gemm16_will_run(g, EPI_STORE, w.npad, s.n_utt);
}

// Precedence, top to bottom: rows (fold) -> Winograd forms packed and scratch offered -> 16-bit rows -> where the chain's statistics are -> a switch.
// Small batches are launch-latency bound: folding leaves the statistics pass and a 64-thread table kernel per norm, B = 1 frame path -4 %.  Large batches keep the
// separate apply pass: the affine in the K loop costs the 512-channel contractions ~14 % at B = 8 (142 vs 125 us), more than the 11 us pass it removes.  fp32:
// from 2 500 rows on both convs run in Winograd form instead (AdaIN rides in their input transforms, elementwise and bandwidth-bound: there the affine is free):
// 3-s utterances, same box: B = 3: 2.78 -> 2.63 ms, B = 4: 2.88 -> 2.83; B = 2: 2.16 -> 2.26 and B = 1: 1.77 -> 1.92 (fold stays).
inline BlockPlan plan_adain_block(const AdainBlockW& B, const Seg& s, const BlockIO& io, const BlockChain& ch, int force_tile, const BlockSwitches& sw) {
  BlockPlan p;
  const int prec = B.conv1.prec;
  const long rows = s.rows();
  const bool fold = rows <= (prec == PREC_F32 ? sw.fold_rows : sw.fold16_rows);
  const bool wino = !fold && io.wino && *io.wino && force_tile == 0;
  const bool wino1 = wino && B.w1.ready;
  // (learned shortcut: conv2 in Winograd form + the 1x1 shortcut as a contraction of its own, added as the Winograd conv's residual)
  const bool wino2 = wino && B.w2.ready && (!B.sc.W || !sw.no_wino_conv2sc);
  // fp32 Winograd branch: every normalised tensor is the output of a Winograd conv (conv1 -> norm2, conv2 -> the next block's norm1), whose output
  // transform leaves the chunk statistics behind: the norms keep only their affine launch
  const bool wstats = ch.stats && ch.chunk_rows == kWinoStatChunk && wino1 && wino2;
  p.bridge_w = wstats ? ch.bridge_w : 0;
  // 16-bit operand modes, large batches: the normalised activations are WRITTEN as 16-bit rows (act1 / act2 reinterpreted), so the contractions stage half
  // the bytes and convert nothing; a learned shortcut reads a rounded copy of x (xs16).
  // Not while the block folds (rows16 <= rows <= fold16_rows, 3 840 .. 4 096 rows with the defaults): no apply pass writes 16-bit rows there, and the folded
  // contraction (conv_gemm_f32<..., XAFF>) stages fp32 rows in every segment, so the shortcut segment reads x and a rounded y comes from a cast pass.
  p.rows16 = (rows >= sw.rows16 && !fold && prec != PREC_F32 && force_tile == 0 && (!B.sc.W || io.xs16) && io.ldx % 8 == 0) ? prec : 0;
  const bool fuse = ch.stats && p.rows16 && !wino1 && !wino2;  // statistics from the epilogues of conv_gemm16_kernel, where it runs

  p.take_pending = fold;
  p.affine_serial = sw.affine_serial;
  p.force_tile = force_tile;
  if (!fold) {  // (folded: both defaults, CONV_FOLD on STAT_PASS)
    if (wino1) {
      p.conv1 = p.bridge_w && ch.planes_ready ? CONV_WINO_BRIDGED : CONV_WINO;
      p.norm1 = p.conv1 == CONV_WINO_BRIDGED ? STAT_BRIDGE : (wstats && ch.in_ready) ? STAT_WINO : STAT_PASS;
    } else {
      p.conv1 = CONV_APPLY;
      p.norm1 = fuse && ch.in_ready ? STAT_EPILOGUE : STAT_PASS;
    }
    if (wino2) {
      p.conv2 = p.bridge_w ? CONV_WINO_BRIDGED : CONV_WINO;
      p.norm2 = p.bridge_w ? STAT_BRIDGE : wstats ? STAT_WINO : STAT_PASS;
    } else {
      p.conv2 = CONV_APPLY;
      if (fuse && block_conv_on_gemm16(s, B.conv1, B.kcin, nullptr, 0, B.cout, 0, B.cout, 0)) p.norm2 = STAT_EPILOGUE;  // conv1's epilogue
    }
  }
  const bool side = io.side && io.side->stream && io.side->out && wino1 && wino2 && !gemm_profiler().on;  // (the profiler's events belong to one stream)
  p.shortcut = !B.sc.W ? SC_IDENTITY : !wino2 ? SC_SEGMENT : side ? SC_SIDE : SC_STREAM;
  p.cast_x16 = B.sc.W && p.rows16 && !io.xs16_ready;
  if (io.y16 && p.conv2 != CONV_WINO_BRIDGED) p.y16 = p.rows16 && !wino2 ? Y16_EPILOGUE : Y16_CAST;  // the 16-bit contraction's epilogue rounds y for the next block's shortcut
  p.defer_conv2 = fold && ch.defer && !io.y16;  // (a rounded copy of y is cast from y right behind conv2: y must exist then)
  if (p.conv2 == CONV_WINO_BRIDGED) {
    p.next_norm1 = ch.next ? STAT_BRIDGE : STAT_PASS;
  } else if (wino2) {
    p.next_norm1 = wstats && ch.out ? STAT_WINO : STAT_PASS;  // the statistics of y for the next block's norm1 (its hidden columns)
  } else if (fuse && ch.out) {
    const bool sc = B.sc.W != nullptr;
    if (block_conv_on_gemm16(s, B.conv2, B.cout, sc ? &B.sc : nullptr, io.ldx, B.cout, sc ? 0 : io.ldx, io.ldy, p.y16 == Y16_EPILOGUE ? io.ldy16 : 0)) p.next_norm1 = STAT_EPILOGUE;
  }
  return p;
}

// ---- the runner: executes a plan
inline int run_adain_block(hipStream_t st, const Seg& s, const AdainBlockW& B, const BlockPlan& p, const BlockIO& io, BlockChain& ch) {
  const int ml = s.max_len(), nchunk = ceil_div(ml, kStatChunk);
  const float* x = io.x;
  const int ldx = io.ldx;
  STTS_CHECK(ldx >= B.kcin, "adain block: input leading dimension %d < padded channels %d", ldx, B.kcin);
  // a norm on its own statistics pass: the pass (which finishes the producer's pending split-K reduce on the way and writes X's first columns), then the table
  auto own_affine = [&](const float* X, int ld, int C, int ld_aff, int gcol0, float* aff, PendingReduce* pend) {
    if (pend && pend->src.partial) {
      STTS_LAUNCH_PROF("adain_partial_reduce_kernel", (size_t)s.rows() * C * 4 * (1 + pend->src.ksplit), adain_partial_reduce_kernel, dim3(ceil_div(C, 32), nchunk, s.n_utt), dim3(256), st,
                       const_cast<float*>(X), ld, C, s.dev, io.ss, round_up(C, 32), nchunk, pend->src);
      pend->src = SplitSrc{};
    } else {
      launch_adain_partial(st, s, X, ld, C, io.ss, round_up(C, 32), kStatChunk);
    }
    launch_adain_affine(st, s, io.ss, C, kStatChunk, p.affine_serial, io.style, io.ld_style, gcol0, aff, ld_aff);
  };
  // ... on the statistics a Winograd output transform left
  auto wino_affine = [&](const float* part, int C, int ld_aff, int gcol0, float* aff) { launch_adain_affine(st, s, part, C, kWinoStatChunk, false, io.style, io.ld_style, gcol0, aff, ld_aff); };
  auto shortcut = [&](hipStream_t sst, float* out) -> int {
    GemmArgs g = gemm_args(s);
    set_seg(g, 0, x, ldx, 0, B.sc);
    g.N = B.cout; g.bias = nullptr; g.Y = out; g.ldy = B.cout;
    return launch_conv_gemm(sst, g, EPI_STORE, B.sc.npad, s.n_utt, ml, 0);
  };

  // norm1 -> LeakyReLU -> conv1
  GemmArgs a = gemm_args(s);
  PendingReduce pend_mid;
  if (ch.pend.src.partial) STTS_CHECK(ch.pend.Y == x && ch.pend.ldy == ldx, "adain block: the pending reduce does not belong to this input");
  if (!p.take_pending) STTS_TRY(ch.finish(st));
  if (p.conv1 == CONV_FOLD) {  // the scale / shift tables live in act1 / act2
    own_affine(x, ldx, B.cin, B.kcin, B.n1.col0, io.act1, &ch.pend);
    set_seg(a, 0, x, ldx, 0, B.conv1);
    a.xaff = io.act1;
    a.ld_xaff = B.kcin;
  } else if (p.conv1 == CONV_APPLY) {
    const bool ready = p.norm1 == STAT_EPILOGUE;
    STTS_TRY(run_adain(st, s, x, ldx, B.cin, io.act1, B.kcin, io.style, io.ld_style, B.n1.col0, ACT_LRELU, nullptr, ready ? ch.in : io.ss, p.rows16, ready));
    set_seg(a, 0, io.act1, B.kcin, 0, B.conv1);
    a.x16 = p.rows16 != 0;
  }
  if (ch.stats) ch.out_ready = false;
  a.N = B.cout;
  a.bias = B.conv1.bias;
  a.Y = io.hbuf;
  a.ldy = B.cout;
  // side lane: the 1x1 shortcut contraction - it reads the block's input only - runs next to conv1's three launches (whose plane contraction fills the chip 1.25
  // times and whose transforms leave the matrix cores idle) instead of between conv1 and conv2
  if (p.shortcut == SC_SIDE) {  // x is complete in st's order here; side->out was last read by the previous block's conv2, which st has queued before this event
    STTS_HIP(hipEventRecord(io.side->fork, st));
    STTS_HIP(hipStreamWaitEvent(io.side->stream, io.side->fork, 0));
    const int rc = shortcut(io.side->stream, io.side->out);
    STTS_HIP(hipEventRecord(io.side->join, io.side->stream));  // (recorded whatever rc is: st joins below or at the caller's error path via stream order)
    if (rc) { (void)hipStreamWaitEvent(st, io.side->join, 0); return rc; }
  }
  if (p.conv1 == CONV_WINO_BRIDGED) {  // the previous block's bridge has normalised and transformed x
    STTS_TRY(run_winograd(st, s, nullptr, 0, B.w1, nullptr, 0, ACT_NONE, nullptr, 0, 1.0f, *io.wino, nullptr, 0, nullptr, 0, WinoForm{true, true}));
  } else if (p.conv1 == CONV_WINO) {  // 8 instead of 18 multiplies per 6 outputs (winograd.hip.h); its output stays in planes for a bridge, or its transform leaves norm2's statistics
    if (p.norm1 == STAT_WINO) wino_affine(ch.in, B.cin, B.kcin, B.n1.col0, io.act1);
    else own_affine(x, ldx, B.cin, B.kcin, B.n1.col0, io.act1, nullptr);
    STTS_TRY(run_winograd(st, s, x, ldx, B.w1, io.hbuf, B.cout, ACT_NONE, nullptr, 0, 1.0f, *io.wino, io.act1, B.kcin, p.norm2 == STAT_WINO ? ch.mid : nullptr, round_up(B.cout, 32),
                          WinoForm{false, p.conv2 == CONV_WINO_BRIDGED}));
  } else {
    if (p.norm2 == STAT_EPILOGUE) {
      a.stat_part = ch.mid; a.ld_stat = round_up(B.cout, 32); a.stat_nchunk = nchunk;
    }
    SplitInfo info1{};
    if (p.conv1 == CONV_FOLD) a.defer = &info1;  // norm2's statistics launch finishes a split-K conv1
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, B.conv1.npad, s.n_utt, ml, p.force_tile));
    if (p.conv1 == CONV_FOLD) pending_from(&pend_mid, info1, a);
  }

  // norm2 -> LeakyReLU -> conv2 (+ learned 1x1 shortcut | + identity residual), / sqrt(2)
  GemmArgs b = gemm_args(s);
  if (p.conv2 == CONV_FOLD) {
    own_affine(io.hbuf, B.cout, B.cout, B.cout, B.n2.col0, io.act2, &pend_mid);
    set_seg(b, 0, io.hbuf, B.cout, 0, B.conv2);
    b.xaff = io.act2;
    b.ld_xaff = B.cout;
  } else if (p.conv2 == CONV_WINO) {
    if (p.norm2 == STAT_WINO) wino_affine(ch.mid, B.cout, B.cout, B.n2.col0, io.act2);
    else own_affine(io.hbuf, B.cout, B.cout, B.cout, B.n2.col0, io.act2, nullptr);
  } else if (p.conv2 == CONV_APPLY) {
    const bool ready = p.norm2 == STAT_EPILOGUE;
    STTS_TRY(run_adain(st, s, io.hbuf, B.cout, B.cout, io.act2, B.cout, io.style, io.ld_style, B.n2.col0, ACT_LRELU, nullptr, ready ? ch.mid : io.ss, p.rows16, ready));
    set_seg(b, 0, io.act2, B.cout, 0, B.conv2);
    b.x16 = p.rows16 != 0;
  }  // (CONV_WINO_BRIDGED: norm2 rides in the bridge below)
  if (p.cast_x16) launch_cast_rows(st, p.rows16, x, ldx, B.cin, io.xs16, ldx, s.rows());
  if (p.shortcut == SC_SEGMENT) {
    set_seg(b, 1, p.rows16 ? reinterpret_cast<const float*>(io.xs16) : x, ldx, 0, B.sc);
  } else if (p.shortcut == SC_IDENTITY) {
    b.R = x;
    b.ldr = ldx;
  }
  b.N = B.cout;
  b.bias = B.conv2.bias;
  b.Y = io.y;
  b.ldy = io.ldy;
  b.alpha = 0.70710678118654752440f;
  if (p.y16 == Y16_EPILOGUE) {
    b.Y16 = io.y16;
    b.ldy16 = io.ldy16;
  }
  if (p.conv2 == CONV_WINO || p.conv2 == CONV_WINO_BRIDGED) {
    const float* res = x;
    int ld_res = ldx;
    if (p.shortcut == SC_SIDE) {
      STTS_HIP(hipStreamWaitEvent(st, io.side->join, 0));
      res = io.side->out;
      ld_res = B.cout;
    } else if (p.shortcut == SC_STREAM) {  // act1 is free again (conv1 has consumed it): the shortcut's output lives there
      STTS_TRY(shortcut(st, io.act1));
      res = io.act1;
      ld_res = B.cout;
    }
    if (p.conv2 == CONV_WINO_BRIDGED) {
      // conv1 -> norm2 -> conv2: contraction, bridge, contraction (conv1's output is needed by nobody else: hbuf stays unwritten); with a next block, conv2 ->
      // its norm1 -> its conv1 the same way - that bridge writes y (+ residual, / sqrt 2), the next block's shortcut and residual input
      STTS_TRY(run_wino_bridge(st, s, B.w1, nullptr, 0, 1.0f, nullptr, 0, B.w2, io.style, io.ld_style, B.n2.col0, B.cout, nullptr, 0, nullptr, 0, *io.wino, p.bridge_w));
      const AdainBlockW* nb = p.next_norm1 == STAT_BRIDGE ? ch.next : nullptr;
      STTS_TRY(run_winograd(st, s, nullptr, 0, B.w2, io.y, io.ldy, ACT_NONE, res, ld_res, b.alpha, *io.wino, nullptr, 0, nullptr, 0, WinoForm{true, nb != nullptr}));
      if (nb) STTS_TRY(run_wino_bridge(st, s, B.w2, res, ld_res, b.alpha, io.y, io.ldy, nb->w1, io.style, io.ld_style, nb->n1.col0, nb->cin, ch.cst, ch.cst_ld, io.y, io.ldy, *io.wino, p.bridge_w));
      ch.planes_ready = nb != nullptr;
      STTS_HIP(hipGetLastError());
      return 0;
    }
    const bool leave = p.next_norm1 == STAT_WINO;
    STTS_TRY(run_winograd(st, s, io.hbuf, B.cout, B.w2, io.y, io.ldy, ACT_NONE, res, ld_res, b.alpha, *io.wino, io.act2, B.cout, leave ? ch.out : nullptr, leave ? ch.out_ld : 0));
    if (leave) ch.out_ready = true;
  } else {
    if (p.next_norm1 == STAT_EPILOGUE) {
      b.stat_part = ch.out; b.ld_stat = ch.out_ld; b.stat_nchunk = nchunk;
      ch.out_ready = true;
    }
    SplitInfo info2{};
    if (p.defer_conv2) b.defer = &info2;
    STTS_TRY(launch_conv_gemm(st, b, EPI_STORE, B.conv2.npad, s.n_utt, ml, p.force_tile));
    if (p.defer_conv2) pending_from(&ch.pend, info2, b);
  }
  if (p.y16 == Y16_CAST) launch_cast_rows(st, B.conv1.prec, io.y, io.ldy, B.cout, io.y16, io.ldy16, s.rows(), B.cout);
  STTS_HIP(hipGetLastError());
  return 0;
}
// plan + run: what a caller with no use for the plan writes
inline int adain_block(hipStream_t st, const Seg& s, const AdainBlockW& B, const BlockIO& io, BlockChain& ch, const BlockSwitches& sw) {
  return run_adain_block(st, s, B, plan_adain_block(B, s, io, ch, 0, sw), io, ch);
}

// The constant input columns of chained blocks: block i + 1 reads [y_i | constant columns], the same columns for every block of the chain (the decoder's
// [asr_res | F0 | N]).  The statistics of a block's input come out of the previous block's conv2 (its `hidden` columns) and, for the constant columns, from ONE
// statistics pass here; the bridge reads that pass's table as BlockChain::cst; 16-bit rows hold the columns rounded once.  decoder_forward and the test operator
// stts_op_adain_chain share this.
struct ConstColumns {
  const float* x = nullptr;  // a row buffer that holds them: columns [hidden, ccat) of rows `ld` wide
  int ld = 0, hidden = 0, ccat = 0;
  float* ss_in = nullptr;    // the chain's statistics of a block's input, out_ld columns per row
  int out_ld = 0;
  bool ready = false;
  void offer_bridge(BlockChain& ch) const {
    ch.cst = ss_in;
    ch.cst_ld = out_ld;
  }
  // (once, as soon as a block has left statistics of its output: whichever block that is, the constant columns must be there before the next norm1 merges them;
  //  bridged: the first block's second bridge already merges them)
  int stats(hipStream_t st, const Seg& s, const BlockChain& ch, bool bridged) {
    if (!(ch.out_ready || bridged) || ready) return 0;
    STTS_CHECK(hidden % 32 == 0, "adain chain: the blocks' width %d must be a multiple of 32", hidden);
    launch_adain_partial(st, s, x + hidden, ld, ccat - hidden, ss_in + hidden, out_ld, ch.chunk_rows);
    ready = true;
    return 0;
  }
  // the rounded copy of the constant columns of `src` (from the 8-aligned column at or below `hidden`, pad columns included) into the 16-bit rows `dst`
  void cast_tail(hipStream_t st, int prec, const float* src, unsigned short* dst, long rows) const {
    const int ctail = hidden & ~7;
    launch_cast_rows(st, prec, src + ctail, ld, ccat - ctail, dst + ctail, ld, rows, ld - ctail);
  }
};

// ------------------------------------------------------------------------------------------------
// stage: Decoder.forward (models/decoder.py:47-60)
// ------------------------------------------------------------------------------------------------
inline int decoder_forward(stts_ctx* c, hipStream_t st, const Seg& s, const float* asr, int ld_asr, const float* pitch, const float* energy,
                           const float* style, float* x_out, int ld_x, Arena& ws, const SideWork* side_lane = nullptr) {
  const stts_model_dims& d = c->d;
  const long R = s.rows();
  const int ccat = d.dec_hidden + d.dec_residual + 2, ldcat = c->dec[1].kcin;  // 578 -> 608 (640 in the 16-bit modes): the packed input width
  const int cenc = d.inter_dim + 2, ldenc = c->dec[0].kcin;                    // 130 -> 160 (192)
  STTS_CHECK(ldcat >= ccat && ldenc >= cenc, "decoder_forward: packed widths %d / %d do not cover %d / %d channels", ldcat, ldenc, ccat, cenc);
  const BlockSwitches sw = block_switches();
  const ChainPlan plan = plan_adain_chain(s, c->prec, c->dec, 5, 1, ChainOffer{true, true, true, side_lane != nullptr}, sw);
  // (dec[0] runs on the encoder-input width, the other blocks on the concat width: scratch is sized by the wider of the two - a config
  //  with inter_dim > hidden_dim + residual_dim is legal)
  const int ldwide = std::max(ldenc, ldcat);
  float* enc_in = ws.get<float>(R * ldenc);
  float* xa = ws.get<float>(R * ldcat);
  float* xb = ws.get<float>(R * ldcat);
  BlockIO io;
  io.act1 = ws.get<float>(R * ldwide);
  io.hbuf = ws.get<float>(R * d.dec_hidden);
  io.act2 = ws.get<float>(R * d.dec_hidden);
  io.ss = ws.get<float>(adain_part_floats(s, ldwide));
  float* ss_in = ws.get<float>(adain_part_floats(s, ldwide, kWinoStatChunk));   // statistics from the producers' epilogues (BlockChain): 16-bit contractions, or
  float* ss_mid = ws.get<float>(adain_part_floats(s, ldwide, kWinoStatChunk));  // the fp32 Winograd output transforms (chunks of 24 rows: the larger footprint)
  float* sty = ws.get<float>((size_t)s.n_utt * c->dec_style.ld());
  WinoScratch wino;
  if (plan.wino) wino.p = ws.get<float>(wino_scratch_floats(s, c->dec[1].w1));
  float* sc_out = plan.sc_out ? ws.get<float>(R * d.dec_hidden) : nullptr;
  // 16-bit rows: rounded copies of the blocks' inputs for the learned shortcuts, ping-pong like xa / xb: a block's
  // conv2 epilogue writes the hidden columns of the next block's copy, the constant columns (asr_res, F0, N) are rounded once
  unsigned short* xs16a = plan.rows16 ? ws.get<unsigned short>(R * ldwide) : nullptr;
  unsigned short* xs16b = plan.rows16 ? ws.get<unsigned short>(R * ldwide) : nullptr;
  STTS_CHECK(ws.ok, "decoder_forward: workspace too small");
  STTS_DRY_RETURN(ws);
  STTS_TRY(run_style(st, c->dec_style, style, s.n_utt, sty));
  FrontArgs fa;
  fa.asr = asr; fa.ld_asr = ld_asr; fa.pitch = pitch; fa.energy = energy;
  for (int i = 0; i < 3; ++i) { fa.wf[i] = c->front_wf[i]; fa.wn[i] = c->front_wn[i]; }
  fa.bf = c->front_bf; fa.bn = c->front_bn;
  fa.enc_in = enc_in; fa.ld_enc = ldenc; fa.xa = xa; fa.xb = xb; fa.ld_x = ldcat;
  fa.c_asr = d.inter_dim; fa.c_hidden = d.dec_hidden; fa.c_res = d.dec_residual;
  launch_decoder_front(st, s, fa);
  // asr_res = wn-conv1x1(asr) into the residual columns of both concat buffers (decoder.py:54)
  for (float* dst : {xa, xb}) {
    GemmArgs a = gemm_args(s);
    set_seg(a, 0, asr, ld_asr, 0, c->asr_res);
    a.N = d.dec_residual; a.bias = c->asr_res.bias; a.Y = dst; a.ldy = ldcat; a.ycol0 = d.dec_hidden;
    STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, c->asr_res.npad, s.n_utt, s.max_len()));
  }
  // (xa and xb hold the same constant columns.  With the bridge, hbuf, ss_mid and the hidden columns of ss_in are unused.)
  BlockChain chain(plan, ss_mid);
  chain.defer = true;
  const int out_ld = round_up(ccat, 32);
  ConstColumns cst;
  cst.x = xa; cst.ld = ldcat; cst.hidden = d.dec_hidden; cst.ccat = ccat; cst.ss_in = ss_in; cst.out_ld = out_ld;
  if (plan.bridge_w) {
    cst.offer_bridge(chain);
    wino.mp_kc = c->dec[1].w1.planes.kc;  // (the scratch is sized by this conv)
    STTS_CHECK(c->dec[0].cout == d.dec_hidden, "decoder_forward: the blocks' width %d is not hidden_dim %d", c->dec[0].cout, d.dec_hidden);
    STTS_TRY(cst.stats(st, s, chain, true));
  }
  io.style = sty; io.ld_style = c->dec_style.ld();
  io.wino = &wino;
  // dec[0] rounds its own (narrow) input into xs16b as scratch, so xs16b's constant columns are filled after it
  io.x = enc_in; io.ldx = ldenc; io.y = xa; io.ldy = ldcat;
  io.xs16 = xs16b; io.y16 = xs16a; io.ldy16 = ldcat;
  chain.link(nullptr, false, ss_in, out_ld, plan.bridge_w ? &c->dec[1] : nullptr);
  STTS_TRY(adain_block(st, s, c->dec[0], io, chain, sw));
  if (plan.rows16) {
    cst.cast_tail(st, c->prec, xa, xs16a, R);
    cst.cast_tail(st, c->prec, xb, xs16b, R);
  }
  STTS_TRY(cst.stats(st, s, chain, plan.bridge_w != 0));
  float* cur = xa;
  float* nxt = xb;
  unsigned short* cur16 = xs16a;
  unsigned short* nxt16 = xs16b;
  SideWork side;
  if (plan.side) {
    side = *side_lane;
    side.out = sc_out;
    io.side = &side;
  }
  auto blocks = [&]() -> int {
    for (int i = 1; i <= 4; ++i) {
      STTS_TRY(cst.stats(st, s, chain, plan.bridge_w != 0));
      io.x = cur; io.ldx = ldcat;
      io.y = i == 4 ? x_out : nxt; io.ldy = i == 4 ? ld_x : ldcat;
      io.xs16 = cur16; io.xs16_ready = plan.rows16; io.y16 = i == 4 ? nullptr : nxt16;
      // (the previous block's conv2 - conv_gemm16_kernel's epilogue or the fp32 Winograd output transform - left the statistics of its output)
      chain.link(ss_in, chain.out_ready, i == 4 ? nullptr : ss_in, out_ld, plan.bridge_w && i < 4 ? &c->dec[i + 1] : nullptr);
      STTS_TRY(adain_block(st, s, c->dec[i], io, chain, sw));
      std::swap(cur, nxt);
      std::swap(cur16, nxt16);
    }
    return 0;
  };
  const int rc = blocks();
  if (rc && plan.side) {  // an error path may have left a shortcut running on the side lane: the caller's stream must not outrun it (it reads x and writes the workspace)
    (void)hipEventRecord(side.join, side.stream);
    (void)hipStreamWaitEvent(st, side.join, 0);
  }
  if (rc) return rc;
  return chain.finish(st);
}

}  // namespace stts

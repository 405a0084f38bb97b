// The plan of a dense contraction (included by gemm.hip.h; host code only, no kernel): the tile table, the process-wide switches, and
// plan_conv_gemm - which kernel, which tile, how many row tiles in which launch, K cut how often.  launch_conv_gemm (gemm.hip.h) validates the
// operands, asks for the plan, fetches scratch and launches; tests/asan/asan_driver.cpp traces the result on a CPU.
#pragma once
#include <climits>
#include <cstdio>

namespace stts {

// ---- the tile table: everything a tile id means.  gemm_dispatch_tile / gemm_dispatch_tile_x3 (gemm.hip.h) take their template arguments from it.
// (intra-block K-split, tiles 8-10, and 2-wave tiles measured no better than these at any layer shape: every configuration plateaus at ~80 %
//  matrix-pipe occupancy, see DESIGN.md section 8.  Id 19 is no tile of conv_gemm_f32: it forces conv_gemm16_kernel.)
enum : unsigned { FORM_F32 = 1, FORM_16 = 2, FORM_X3 = 4 };  // operand forms: f32 matrix cores, bf16 / fp16 operands, split fp32
enum TileX16 { X16_NEVER, X16_MAY, X16_MUST };               // 16-bit activation rows (16-bit forms) / pre-split activation planes (split fp32)
struct TileRow {
  int id, BM, BN, WM, WN, KS;  // BM cout x BN rows per block, WM x WN waves x KS K-groups
  bool glds;                   // staging: through registers, or LDS-DMA (global_load_lds_dwordx4)
  unsigned forms;
  TileX16 x16;
  bool store_only;  // EPI_STORE only (else also EPI_SPLIT_ACC)
  bool paired;      // may take the paired epilogues (gate / couple / prior): 64-column wave tiles
  bool xaff;        // may take an input affine (it lives on the register staging path)
  bool splitk;      // may be cut by block split-K / take a remainder launch
};
constexpr unsigned kAllForms = FORM_F32 | FORM_16 | FORM_X3;
constexpr TileRow kTiles[] = {
    // id  BM   BN  WM WN KS  glds   forms      x16        store  paired xaff   splitk
    {2, 128, 64, 2, 2, 1, false, kAllForms, X16_MAY, false, true, true, true},     // 4 waves of 64 x 32
    {3, 128, 32, 2, 1, 1, false, kAllForms, X16_MAY, false, true, true, true},     // the default of small paired launches
    {4, 128, 32, 4, 1, 1, false, kAllForms, X16_MAY, false, false, true, true},    // 32-row tile, 4 waves of one 32x32 tile each
    {5, 128, 128, 4, 2, 1, false, kAllForms, X16_MAY, false, false, true, true},   // 8 waves per block
    {6, 128, 64, 4, 2, 1, false, kAllForms, X16_MAY, false, false, true, true},    // 8 waves, 64-row tiles
    {8, 128, 128, 4, 2, 2, false, kAllForms, X16_NEVER, false, false, true, false},  // 16 waves: 8 positions x 2 K-groups
    {11, 128, 128, 4, 2, 1, true, FORM_F32, X16_NEVER, false, false, false, true},   // LDS-DMA staging, 8 waves
    {13, 128, 64, 4, 2, 1, true, FORM_F32, X16_NEVER, false, false, false, true},    // LDS-DMA staging, 64-row tile
    // 256 cout x 256 rows, 8 waves of 64 x 128 (8 accumulator tiles): 16-bit operands at large batches, where the 128x128 loop is bound by
    // L2 -> LDS staging (47 B/clk/CU needed); this tile needs 31
    {14, 256, 256, 4, 2, 1, false, FORM_16, X16_MAY, true, false, true, true},
    {15, 128, 256, 4, 2, 1, false, FORM_16, X16_MAY, true, false, true, true},
    // tiles 14 / 15 with LDS-DMA staging (three stages): 16-bit activation rows only
    {16, 256, 256, 4, 2, 1, true, FORM_16, X16_MUST, true, false, false, true},
    {17, 128, 256, 4, 2, 1, true, FORM_16, X16_MUST, true, false, false, true},
    // 128 x 128, 8 waves, LDS-DMA with eight stages: one-round launches of small batches in the 16-bit modes
    {18, 128, 128, 4, 2, 1, true, FORM_16, X16_MUST, true, false, false, true},
    {20, 128, 128, 2, 2, 1, false, FORM_X3, X16_MAY, false, true, true, true},   // 4 waves of 64 x 64
    {21, 128, 128, 2, 2, 2, false, FORM_X3, X16_MAY, false, true, true, false},  // 8 waves: 64 x 64 x two K-groups
    {22, 128, 256, 2, 4, 1, false, FORM_X3, X16_MAY, false, true, true, true},   // 8 waves of 64 x 64, 256 rows
    // pre-split activation planes (three bf16 planes written by the producer: no split, no conversion in the loop)
    {25, 128, 128, 4, 2, 1, false, FORM_X3, X16_MUST, true, false, false, false},  // tile 5, register staging
    {26, 128, 64, 4, 2, 1, false, FORM_X3, X16_MUST, true, false, false, false},   // tile 6
    {27, 128, 128, 4, 2, 1, true, FORM_X3, X16_MUST, true, false, false, false},   // tile 5, LDS-DMA (three stages)
    {28, 128, 64, 4, 2, 1, true, FORM_X3, X16_MUST, true, false, false, false},    // tile 6, LDS-DMA
};
constexpr const TileRow* find_tile(int id) {
  for (const TileRow& r : kTiles)
    if (r.id == id) return &r;
  return nullptr;
}
constexpr TileRow tile_row(int id) { return *find_tile(id); }  // (constant evaluation fails for an id without a row)
// the pre-split tile that stands for a tile of `bn` rows: the 128 x 128 or the 128 x 64 one
constexpr int presplit_tile(int bn, bool glds) {
  for (const TileRow& r : kTiles)
    if ((r.forms & FORM_X3) && r.x16 == X16_MUST && r.glds == glds && r.BN == (bn >= 128 ? 128 : 64)) return r.id;
  return 0;
}
// ---- the switches: experiments and comparisons, read ONCE per process (nothing changes them inside one)
struct GemmSwitches {
  static constexpr int kUnset = INT_MIN;
  bool no_x3;             // STTS_NO_X3=1: every fp32 contraction on v_mfma_f32_32x32x2_f32, the path of rounds 1-3
  bool x3_rem;            // STTS_X3_REM=1: split fp32 takes remainder launches too
  int x3_tile;            // STTS_X3_TILE = 5 / 6 / 22 for every large split-fp32 launch; any value switches the tile-22 rule off
  bool x3p_glds;          // STTS_X3P_GLDS: pre-split planes staged by LDS-DMA (default 1) or through registers (0)
  int tile16;             // STTS_TILE16: tile for every 16-bit-row store launch
  int splitk_min_iters;   // STTS_SPLITK_MIN_ITERS: K iterations a split-K slice must keep (0: the rule below)
  long gemm16_min_tiles;  // STTS_GEMM16_MIN_TILES: smallest launch for conv_gemm16_kernel (default 192 tiles)
};
inline const GemmSwitches& gemm_switches() {
  static const GemmSwitches sw = [] {
    auto num = [](const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
    GemmSwitches s;
    s.no_x3 = num("STTS_NO_X3", 0) != 0;
    s.x3_rem = num("STTS_X3_REM", 0) != 0;
    s.x3_tile = num("STTS_X3_TILE", GemmSwitches::kUnset);
    s.x3p_glds = num("STTS_X3P_GLDS", 1) != 0;
    s.tile16 = num("STTS_TILE16", GemmSwitches::kUnset);
    s.splitk_min_iters = getenv("STTS_SPLITK_MIN_ITERS") ? std::max(1, atoi(getenv("STTS_SPLITK_MIN_ITERS"))) : 0;
    s.gemm16_min_tiles = getenv("STTS_GEMM16_MIN_TILES") ? atol(getenv("STTS_GEMM16_MIN_TILES")) : 192;
    return s;
  }();
  return sw;
}
// Process-wide switch of the split-fp32 contractions
inline bool x3_enabled() { return !gemm_switches().no_x3; }

// ---- the plan
enum GemmRoute { ROUTE_GEMM16, ROUTE_X3, ROUTE_BF16, ROUTE_F16, ROUTE_F32 };  // conv_gemm16_kernel | conv_gemm_f32 in its four operand forms
struct GemmPlan {
  GemmRoute route = ROUTE_F32;
  int tile = 0;
  long full_rt = 0, rem_rt = 0;  // row tiles in the plain launch / in the split-K remainder launch
  int rem_ksp = 1, main_ksp = 1;
  char err[256] = "";  // a failed check; empty = ok
  bool ok() const { return err[0] == 0; }
  int bn() const { return find_tile(tile)->BN; }
};
#define STTS_PLAN_CHECK(cond, ...)                    \
  do {                                                \
    if (!(cond)) {                                    \
      snprintf(p.err, sizeof(p.err), __VA_ARGS__);    \
      return p;                                       \
    }                                                 \
  } while (0)

constexpr int kG16Tile = 256;  // conv_gemm16_kernel (gemm16.hip.h): rows and output channels per block
constexpr int kG16K = 64;      // channels per K tile
// Can this contraction run on conv_gemm16_kernel?  16-bit activation rows, store epilogue, every segment's channels a multiple of 64,
// cout padded to 256, N a multiple of 4, host offsets known (compact grid).
inline bool gemm16_eligible(const GemmArgs& a, int epi, int npad) {
  if (epi != EPI_STORE || a.prec == PREC_F32 || !a.x16 || !a.seg_host || a.xaff || npad % kG16Tile != 0 || a.N % 4 != 0) return false;
  if (a.ldy % 4 || a.ycol0 % 4 || a.ldr % 4 || a.rcol0 % 4 || a.ldy16 % 4 || a.ycol16 % 4 || a.ld_ss % 4 || a.ld_stat % 4) return false;
  for (int i = 0; i < a.nseg; ++i)
    if (a.seg[i].kc % kG16K != 0 || a.seg[i].ldx % 8 != 0 || a.seg[i].xcol0 % 8 != 0 || !a.seg[i].W16 || a.seg[i].ldx - a.seg[i].xcol0 < a.seg[i].kc) return false;
  return true;
}

// 256 x 256 tiles of the launch: exact from the host offsets (an upper bound when they are capacities)
inline long gemm16_tiles(const GemmArgs& a, int npad, int n_utt) {
  long rt = 0;
  for (int u = 0; u < n_utt; ++u) rt += ceil_div(a.seg_host[u + 1] - a.seg_host[u], kG16Tile);
  return rt * (npad / kG16Tile);
}

// Rules 1 + 2: conv_gemm16_kernel takes 16-bit activation rows, store epilogue, at least ~one 256 x 256 tile per CU.  force_tile 19 selects
// it whatever the size (tests), any other forced tile keeps the launch on conv_gemm_f32.
inline bool gemm16_route(const GemmArgs& a, int epi, int npad, int n_utt, int force_tile, const GemmSwitches& sw) {
  if (force_tile != 0 && force_tile != 19) return false;
  return gemm16_eligible(a, epi, npad) && (force_tile == 19 || gemm16_tiles(a, npad, n_utt) >= sw.gemm16_min_tiles);
}
// would launch_conv_gemm pick conv_gemm16_kernel for this call?  (plan_adain_block asks before the runner sets stat_part)
inline bool gemm16_will_run(const GemmArgs& a, int epi, int npad, int n_utt) { return gemm16_route(a, epi, npad, n_utt, 0, gemm_switches()); }

constexpr int kCUs = 256;
// row tiles of bn rows: exact when the host offsets are known (mixed lengths)
inline long gemm_row_tiles(const GemmArgs& a, int n_utt, int max_rows, int bn) {
  if (!a.seg_host) return (long)n_utt * ceil_div(max_rows, bn);
  long t = 0;
  for (int u = 0; u < n_utt; ++u) t += ceil_div(a.seg_host[u + 1] - a.seg_host[u], bn);
  return t;
}
// Rule 12.  A launch takes about ceil(blocks / 256 CUs) block-times however many blocks are co-resident: a CU's matrix pipes are
// the shared resource (block-timeline trace, profiles/).  When the last round would be mostly empty (288 tiles = 1.125
// rounds for a 3.5 s batch of 8), the whole rounds run as they are and the REMAINDER row tiles run as a second launch
// with K cut over up to 8 blocks (+ reduce pass over those rows only): 1 + ~1/8 rounds instead of 2.
struct RowPlan {
  long full_rt = 0, rem_rt = 0;
  int rem_ksp = 1;
  double cost = 0;  // in 128-row block-times
};
inline RowPlan plan_rows(long rt, int mt, int iters, bool may_split_rem, int bn, double penalty) {
  RowPlan p;
  const long blocks = rt * mt, whole = blocks / kCUs;
  p.full_rt = rt;
  p.cost = std::ceil((double)blocks / kCUs);
  if (may_split_rem && whole >= 1 && blocks % kCUs != 0) {
    const long full_rt = whole * kCUs / mt, rem_blocks = (rt - full_rt) * mt;
    const int ksp = (int)std::min<long>(8, std::min<long>(iters / 4, kCUs / std::max<long>(rem_blocks, 1)));
    if (ksp >= 2 && full_rt > 0) {
      const double hybrid = (double)(full_rt * mt) / kCUs + std::max((double)rem_blocks / kCUs, 1.0 / ksp) * 1.15 + 0.1;
      if (hybrid < p.cost) {
        p.full_rt = full_rt;
        p.rem_rt = rt - full_rt;
        p.rem_ksp = ksp;
        p.cost = hybrid;
      }
    }
  }
  p.cost *= bn * penalty;
  return p;
}
// the per-tile checks, all from the table: does `tile` exist, in this operand form, for these operands and this epilogue?
inline bool tile_fits(GemmPlan& p, int tile, const GemmArgs& a, int epi, int npad, unsigned form) {
  const TileRow* r = find_tile(tile);
  const bool paired = epi != EPI_STORE && epi != EPI_SPLIT_ACC;
  if (!r) snprintf(p.err, sizeof(p.err), "conv_gemm: no tile %d", tile);
  else if (!(r->forms & form) || (a.x16 ? r->x16 == X16_NEVER || a.xaff : r->x16 == X16_MUST) || (a.xaff && !r->xaff) || (epi != EPI_STORE && r->store_only) ||
           (paired && !r->paired) || npad % r->BM != 0)
    snprintf(p.err, sizeof(p.err), "conv_gemm: tile %d does not take this launch (operand form %u, 16-bit rows / pre-split planes %d, input affine %d, epilogue %d, cout padded to %d): see kTiles", tile, form,
              a.x16, a.xaff != nullptr, epi, npad);
  return p.ok();
}

// npad: padded cout of the packed weight (multiple of 128).  max_rows: longest utterance (rows).  No HIP call, no getenv, no allocation.
// Precedence, in the order applied:
//   1 a forced tile (19: conv_gemm16_kernel; 100 + t: tile t off the split-fp32 form)  2 conv_gemm16_kernel: eligible and large enough
//   3 split fp32: eligible?  4 small launches -> tile 4, paired epilogues -> 3 / 2  5 128- vs 64-row tiles by cost  6 split fp32 with short K -> tile 6
//   7 the 16-wave tile 8  8 16-bit activation rows -> tiles 14 / 15  9 the experiment switches STTS_TILE16, STTS_X3_TILE  10 tile 22
//   11 pre-split planes -> tiles 25 - 28  12 whole rounds + split-K remainder (plan_rows)  13 block split-K
inline GemmPlan plan_conv_gemm(const GemmArgs& a, int epi, int npad, int n_utt, int max_rows, int force_tile, const GemmSwitches& sw) {
  GemmPlan p;
  if (gemm16_route(a, epi, npad, n_utt, force_tile, sw)) {
    p.route = ROUTE_GEMM16;
    p.tile = 19;
    return p;
  }
  STTS_PLAN_CHECK(!a.stat_part, "conv_gemm: output statistics (stat_part) exist only in conv_gemm16_kernel's epilogue: ask gemm16_will_run first");
  STTS_PLAN_CHECK(force_tile != 19, "conv_gemm: tile 19 (conv_gemm16_kernel) needs 16-bit activation rows, a store epilogue, channels in multiples of 64 and cout padded to 256");
  const int mt = npad / 128;
  int iters = 0;
  for (int i = 0; i < a.nseg; ++i) iters += a.seg[i].ntaps * (a.seg[i].kc / 32);
  // (the split-K reduce pass writes fp32 Y only: launches that want the 16-bit copy, or no fp32 output at all, stay whole)
  const bool splittable = force_tile == 0 && epi == EPI_STORE && !a.sumsq_part && a.Y && !a.Y16;
  const long blocks128 = mt * gemm_row_tiles(a, n_utt, max_rows, 128);
  // split fp32: fp32 call, every segment carries the three bf16 planes of its weight, epilogue with a split instantiation
  bool x3 = a.prec == PREC_F32 && !sw.no_x3 && (epi == EPI_STORE || epi == EPI_PRIOR);
  for (int i = 0; i < a.nseg; ++i) x3 = x3 && a.seg[i].W16 != nullptr && a.seg[i].w16_plane > 0 && 6 * a.seg[i].w16_plane + 2L * 128 * a.seg[i].ntaps * a.seg[i].kc < (1L << 32);
  // pre-split activation planes (x16 on an fp32 call): store epilogue, no input affine, no block split-K (the callers know: run_winograd)
  if (a.x16 && a.prec == PREC_F32) {
    STTS_PLAN_CHECK(x3 && epi == EPI_STORE && !a.xaff && !a.sumsq_part, "conv_gemm: pre-split activation planes need the split-fp32 store contraction");
    for (int i = 0; i < a.nseg; ++i) STTS_PLAN_CHECK(a.seg[i].x_plane > 0 && a.seg[i].ldx % 8 == 0 && a.seg[i].xcol0 % 8 == 0, "conv_gemm: pre-split activation planes: segment %d misaligned", i);
  }
  if (force_tile >= 100) {  // tests / tools: 100 + t = tile t on the f32 matrix cores whatever the switch says
    x3 = false;
    force_tile -= 100;
  }
  if (force_tile != 0) {
    const TileRow* f = find_tile(force_tile);
    STTS_PLAN_CHECK(f, "conv_gemm: no tile %d", force_tile);
    if (!(f->forms & FORM_X3) || (f->x16 == X16_MUST && !a.x16)) x3 = false;  // a forced tile without a split form (LDS-DMA tiles)
  }
  // (split fp32: whole launches.  Its blocks are 1.5 x shorter, and a remainder launch + its reduce pass then cost more than the partly empty last round:
  //  cfg2 3.58 -> 3.475 ms per step without the 12 remainder launches and 11 reduce passes of the Winograd plane contractions; STTS_X3_REM=1 brings them back)
  const bool may_split_rem = (!x3 || sw.x3_rem) && splittable && a.seg_host && !a.capacity;  // (the remainder launch needs exact host offsets)
  int tile = force_tile;
  const bool paired = epi != EPI_STORE && epi != EPI_SPLIT_ACC;  // paired epilogues need 64-column wave tiles
  RowPlan rows;
  if (tile == 0) {
    // small launches: 32-row tiles; unpaired epilogues spread the 128 output channels over four waves (a wave's MFMA
    // chain per iteration is then 16 instead of 32 instructions: these launches are latency-bound on that chain)
    if (blocks128 < 24) tile = paired ? 3 : 4;
    else if (paired) tile = 2;
    else {
      // 128x128 vs 128x64 tiles by that cost (576 blocks of 128x64 cost three half-sized rounds)
      const RowPlan p5 = plan_rows(gemm_row_tiles(a, n_utt, max_rows, 128), mt, iters, may_split_rem, 128, 1.0);
      const RowPlan p6 = plan_rows(gemm_row_tiles(a, n_utt, max_rows, 64), mt, iters, may_split_rem, 64, 1.03);
      tile = p5.cost <= p6.cost ? 5 : 6;
      // split fp32, short K (at most 24 iterations: the 1 x 1 convs over 512-768 channels): the prologue and epilogue of a block are a fifth of its life, and
      // two co-resident 128 x 64 blocks hide them behind each other's K loop (B = 8, per launch inside the step: pwconv1 94.2 -> 87.3 us, the small
      // 1 x 1 convs 19.0 -> 16.9 / 18.7 -> 15.7; deep K keeps the 128 x 128 tile: pwconv2 85.7 vs 87.4)
      if (x3 && iters <= 24 && !a.xaff) tile = 6;
      rows = tile == 5 ? p5 : p6;
      // one 128x128 tile per CU (B = 8: every 512-channel layer): two K-groups of 8 waves share each staged tile, which
      // keeps the matrix pipes busier than 8 waves do (118 vs 125.5 us) and beats cutting K over two blocks plus the
      // reduce pass (131 us)
      // (fp32 only: with 16-bit operands the loop is staging-bound and 8 waves are faster, 34 vs 40 us)
      // (split fp32: the 8-wave tile is the faster one there too, and the 16-wave tile's 128-register budget spills with the input affine)
      if (tile == 5 && blocks128 <= kCUs && a.prec == PREC_F32 && !x3) tile = 8;
    }
  }
  const long rt256 = gemm_row_tiles(a, n_utt, max_rows, 256);
  if (force_tile == 0 && a.prec != PREC_F32 && a.x16 && epi == EPI_STORE) {
    // 16-bit activation rows: 256-row tiles once they fill the chip at least ~1.5 times.  128 x 256 (two blocks per CU, so
    // one block's prologue / epilogue hides behind the other's K loop) unless K is deep (the k = 7 convs: >= 128 iterations),
    // where the 256 x 256 tile's lower staging rate wins (B = 64: out conv 875 vs 896 us, prior conv 287 vs 302; but
    // pwconv1 403 vs 213, decoder convs 200 vs 137: tools/gemm_bench.py TUNE=1152)
    if (npad % 256 == 0 && iters >= 128 && rt256 * (npad / 256) >= 3 * kCUs / 2) tile = 14;
    else if (rt256 * (npad / 128) >= 3 * kCUs / 2) tile = 15;
    if (tile == 14 || tile == 15) rows = RowPlan();
    if (sw.tile16 != GemmSwitches::kUnset) {  // experiment switch
      tile = sw.tile16;
      rows = RowPlan();
    }
  }
  const unsigned form = x3 ? FORM_X3 : a.prec == PREC_F32 ? FORM_F32 : FORM_16;
  if (!tile_fits(p, tile, a, epi, npad, form)) return p;
  const bool x3_large = x3 && !a.x16 && force_tile == 0 && (tile == 5 || tile == 6);
  if (x3_large && (sw.x3_tile == 5 || sw.x3_tile == 6 || sw.x3_tile == 22)) {  // experiment switch
    tile = sw.x3_tile;
    rows = RowPlan();
  }
  // (... or a launch of at least 440 such blocks that fills its last chip round to 80 %: the output convs' Winograd planes at B = 8 are 480 blocks = 1.9
  //  rounds, 212.6 -> 193.0 and 206.5 -> 184.9 us per conv; 360 blocks = 1.4 rounds lose, pwconv1 94 -> 99)
  const long blocks22 = rt256 * mt;
  const bool fills22 = blocks22 >= 640 || (blocks22 >= 440 && (blocks22 % kCUs == 0 || blocks22 % kCUs >= kCUs * 4 / 5));
  if (x3_large && fills22 && sw.x3_tile == GemmSwitches::kUnset) {
    // split fp32, launches of at least 2.5 chip rounds of 256-row tiles: 8 waves of 64 x 64 (half the weight staging per row, 12 instead of 18 fragment
    // reads per 24 MFMAs).  B = 64 x 3 s: every layer 8-12 % faster than the 128 x 128 tile (decoder conv2 648 -> 595 us, output conv 3 637 -> 3 342);
    // B = 24: the 1536- and 1024-wide layers (1 080 / 720 blocks) gain, the 512-wide ones (360 blocks = 1.4 rounds) would lose and keep the 128-row tile
    tile = 22;
    rows = RowPlan();
  }
  if (x3 && a.x16) {  // pre-split activation planes: the 128 x 128 or the 128 x 64 tile, whole launches (no block split-K, no remainder launch)
    if (find_tile(tile)->x16 != X16_MUST) tile = presplit_tile(find_tile(tile)->BN, sw.x3p_glds);
    rows = RowPlan();
  }
  if (!tile_fits(p, tile, a, epi, npad, form)) return p;
  const TileRow& row = *find_tile(tile);
  if ((rows.full_rt == 0 && rows.rem_rt == 0) || !row.splitk) rows = RowPlan{gemm_row_tiles(a, n_utt, max_rows, row.BN), 0, 1, 0};
  p.route = x3 ? ROUTE_X3 : a.prec == PREC_BF16 ? ROUTE_BF16 : a.prec == PREC_F16 ? ROUTE_F16 : ROUTE_F32;
  p.tile = tile;
  p.full_rt = rows.full_rt;
  p.rem_rt = rows.rem_rt;
  p.rem_ksp = rows.rem_ksp;
  // Block-level split-K for launches that cannot fill the chip (phoneme-rate layers, B = 1): one wave's MFMA chain over
  // the whole K (~1 us per 32 channels x taps) is then the critical path, so K is cut over up to 8 blocks per tile.
  if (splittable && row.splitk && p.rem_rt == 0) {
    const long blocks = p.full_rt * mt;
    // (16-bit operands: a contraction that already has one tile per CU is shorter than the reduce pass it would add)
    // K iterations a slice must keep: 4; 8 once the launch has half a chip of blocks anyway (a 16-iteration contraction over 128-256 blocks cut in
    // two gained less than its reduce pass costs: CFM estimator 8 x 800 frames 7.00 -> 6.82 ms; launches with fewer blocks still gain from the cut)
    const int min_it = sw.splitk_min_iters ? sw.splitk_min_iters : (blocks >= 128 ? 8 : 4);
    // (fp32 on the f32 matrix cores: launches of 128-256 blocks take the 16-wave tile above, so 512 never cuts them; split fp32: like the 16-bit forms)
    p.main_ksp = (int)std::min<long>(8, std::min<long>(iters / min_it, ((a.prec == PREC_F32 && !x3) ? 512 : 255) / std::max<long>(blocks, 1)));
    if (p.main_ksp < 2) p.main_ksp = 1;
  }
  return p;
}

}  // namespace stts

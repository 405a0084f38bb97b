// Test operators (single layers behind the C-ABI, used by tests/ to compare one kernel at a time with the oracle) and the
// contraction micro-benchmark of tools/gemm_bench.py.  None of this is on the product path: api.hip includes this file only
// when built with -DSTTS_TEST_OPS (the default of __graft_entry__.compile, because tests/ need the operators;
// STTS_PRODUCT_ONLY=1 builds the library without them).  Uses api.hip's API_BEGIN / SEG_CHECK helpers.
#pragma once

extern "C" {

// ------------------------------------------------------------------------------------------------ test operators
int stts_op_conv1d(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ldx, int cin,
                   const float* w_host, const float* bias_host, int cout, int k, int dil, int act, float* y, int ldy, int force_tile, int precision) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(ldx % 32 == 0 && ldx >= cin, "op_conv1d: ldx must be a multiple of 32 covering cin");
  // precision 0: fp32, split-fp32 contraction (PREC_X3, the default form); 3: fp32 on the f32 matrix cores (STTS_PREC_F32_NATIVE)
  STTS_CHECK(precision >= 0 && precision <= 3, "precision must be STTS_PREC_F32, _BF16, _F16 or _F32_NATIVE");
  stts_ctx tmp;  // only for allocation bookkeeping
  tmp.prec = precision == 3 ? 0 : precision;
  tmp.allow_x3 = precision != 3;
  PackScope scope(&tmp, engine_mode(&tmp));
  struct FreeAll {  // every exit path (including the early STTS_TRY / STTS_CHECK returns) waits for the stream and frees the temporaries
    stts_ctx& t;
    hipStream_t st;
    ~FreeAll() {
      (void)hipStreamSynchronize(st);
      for (void* p : t.allocs) (void)hipFree(p);
    }
  } free_all{tmp, st};
  HostTensor w;
  w.shape = {cout, cin, k};
  w.data.assign(w_host, w_host + (size_t)cout * cin * k);
  HostTensor b;
  b.shape = {cout};
  if (bias_host) b.data.assign(bias_host, bias_host + cout);
  Seg s{n_utt, seg_off_host, seg_off_dev};
  if (force_tile == -4) {  // the Winograd F(6, k) form (k = 3 or 7, dilation 1): winograd.hip.h
    STTS_CHECK(dil == 1 && (precision == 0 || precision == 3), "op_conv1d: the Winograd form is fp32, dilation 1");
    WinoConv wc;
    STTS_TRY(pack_winograd(&tmp, w, bias_host ? &b : nullptr, 0, cin, cout, &wc));
    float* scratch = nullptr;
    STTS_HIP(hipMalloc(&scratch, wino_scratch_floats(s, wc) * sizeof(float)));
    tmp.allocs.push_back(scratch);
    WinoScratch wz;
    wz.p = scratch;
    STTS_TRY(run_winograd(st, s, x, ldx, wc, y, ldy, act, nullptr, 0, 1.0f, wz));
    STTS_HIP(hipStreamSynchronize(st));
    return 0;
  }
  PackedConv pc;
  STTS_TRY(pack_rows(&tmp, w, bias_host ? &b : nullptr, plain_rows(cout), 0, cin, round_up(cin, 32), cout, &pc));
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, x, ldx, 0, pc, (k - 1) / 2, dil);
  a.N = cout; a.bias = pc.bias; a.Y = y; a.ldy = ldy; a.act = act;
  if (force_tile >= 100) {  // tests: the contraction reads 16-bit activation rows (rounded copy of x), tile = force_tile - 100
    STTS_CHECK(precision == 1 || precision == 2, "op_conv1d: 16-bit activation rows need a 16-bit operand mode");
    unsigned short* x16 = nullptr;
    STTS_HIP(hipMalloc(&x16, (size_t)s.rows() * ldx * sizeof(unsigned short)));
    tmp.allocs.push_back(x16);
    launch_cast_rows(st, precision, x, ldx, ldx, x16, ldx, s.rows());
    a.seg[0].X = reinterpret_cast<const float*>(x16);
    a.x16 = 1;
    force_tile -= 100;
  }
  STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, pc.npad, n_utt, s.max_len(), force_tile));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

// The contraction variants a plain conv does not reach: F.conv1d over the channel concatenation [x, x2] (w [cout, cin + cin2, k]) as two
// segments of one launch (MSEG), an input affine on x staged with the tile (XAFF: x' = lrelu_slope(x * scale + shift), aff_host
// [n_utt][2][ldx], scale 0 marks a pad column; xaff_mode 2 = the scale-only instantiation: shift 0, slope 1, cin a multiple of 32, no x2),
// and activations split into three bf16 planes by launch_split_rows before the contraction (presplit: tiles 25 - 28).
int stts_op_conv1d_x3(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, const float* x, int ldx, int cin,
                      const float* x2, int ldx2, int cin2, const float* w_host, const float* bias_host, int cout, int k, int dil, const float* aff_host,
                      int xaff_mode, float slope, int presplit, float* y, int ldy, int force_tile, int precision) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(ldx % 32 == 0 && ldx >= cin && (!x2 || (ldx2 % 32 == 0 && ldx2 >= cin2 && cin2 > 0)), "op_conv1d_x3: ldx must be a multiple of 32 covering cin");
  STTS_CHECK(precision == 0 || precision == 3, "op_conv1d_x3: precision must be STTS_PREC_F32 or _F32_NATIVE");
  STTS_CHECK(xaff_mode >= 0 && xaff_mode <= 2 && (xaff_mode == 0) == (aff_host == nullptr), "op_conv1d_x3: xaff_mode 1 / 2 need the affine table");
  STTS_CHECK(xaff_mode != 2 || (!x2 && cin == ldx && slope == 1.0f), "op_conv1d_x3: the scale-only affine is single-segment, cin == ldx, slope 1");
  STTS_CHECK(!presplit || (precision == 0 && xaff_mode == 0), "op_conv1d_x3: pre-split planes are a split-fp32 form without an input affine");
  stts_ctx tmp;
  tmp.prec = 0;
  tmp.allow_x3 = precision != 3;
  PackScope scope(&tmp, engine_mode(&tmp));
  struct FreeAll {
    stts_ctx& t;
    hipStream_t st;
    ~FreeAll() {
      (void)hipStreamSynchronize(st);
      for (void* p : t.allocs) (void)hipFree(p);
    }
  } free_all{tmp, st};
  const int ctot = cin + (x2 ? cin2 : 0);
  HostTensor w;
  w.shape = {cout, ctot, k};
  w.data.assign(w_host, w_host + (size_t)cout * ctot * k);
  HostTensor b;
  b.shape = {cout};
  if (bias_host) b.data.assign(bias_host, bias_host + cout);
  Seg s{n_utt, seg_off_host, seg_off_dev};
  PackedConv pc0, pc1;
  STTS_TRY(pack_rows(&tmp, w, bias_host ? &b : nullptr, plain_rows(cout), 0, cin, round_up(cin, 32), cout, &pc0));
  if (x2) STTS_TRY(pack_rows(&tmp, w, nullptr, plain_rows(cout), cin, cin2, round_up(cin2, 32), cout, &pc1));
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, x, ldx, 0, pc0, (k - 1) / 2, dil);
  if (x2) set_seg(a, 1, x2, ldx2, 0, pc1, (k - 1) / 2, dil);
  a.N = cout; a.bias = pc0.bias; a.Y = y; a.ldy = ldy; a.act = 0;
  if (xaff_mode) {
    std::vector<float> aff(aff_host, aff_host + (size_t)n_utt * 2 * ldx);
    float* d = nullptr;
    STTS_TRY(dev_upload(&tmp, aff, &d));
    a.xaff = d;
    a.ld_xaff = ldx;
    a.xaff_slope = slope;
    a.xaff_scale_only = xaff_mode == 2;
  }
  if (presplit) {  // every segment's rows -> three bf16 planes (pad columns included: they are finite and meet zero weights)
    for (int i = 0; i < a.nseg; ++i) {
      const long plane = (long)s.rows() * a.seg[i].ldx;
      unsigned short* p = nullptr;
      STTS_HIP(hipMalloc(&p, 3 * plane * sizeof(unsigned short)));
      tmp.allocs.push_back(p);
      launch_split_rows(st, a.seg[i].X, a.seg[i].ldx, a.seg[i].ldx, p, a.seg[i].ldx, plane, s.rows());
      a.seg[i].X = reinterpret_cast<const float*>(p);
      a.seg[i].x_plane = plane;
    }
    a.x16 = 1;
  }
  STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, pc0.npad, n_utt, s.max_len(), force_tile));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

// The store contraction of the 16-bit operand modes with every epilogue feature under the caller's control (include/stylish_hip.h).  Follows the 16-bit
// branch of stts_op_conv1d; weights are packed with cin padded to 64 and cout to 256 (plain_rows pads to 128, which would make cout = 384 ineligible
// for conv_gemm16_kernel).  Every buffer the launch may touch is checked against the caller's element counts BEFORE anything is launched.
int stts_op_conv1d_epi(void* stream, const stts_conv_epi_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p && p->seg_off_host && p->seg_off_dev && p->n_utt > 0, "op_conv1d_epi: null / empty argument");
  STTS_CHECK(p->precision == PREC_BF16 || p->precision == PREC_F16, "op_conv1d_epi: precision must be STTS_PREC_BF16 or _F16");
  STTS_CHECK(p->nseg == 1 || p->nseg == 2, "op_conv1d_epi: one or two K segments");
  STTS_CHECK(p->cout > 0 && p->act >= ACT_NONE && p->act <= ACT_LRELU, "op_conv1d_epi: cout / act out of range");
  STTS_CHECK(p->tune == 0 || p->tune == 0x4000, "op_conv1d_epi: tune is 0 or 0x4000");
  STTS_CHECK(find_tile(p->force_tile) || p->force_tile == 19, "op_conv1d_epi: force_tile must name a tile");
  STTS_CHECK(p->y || p->y16, "op_conv1d_epi: no output rows requested");
  const int n_utt = p->n_utt, N = p->cout;
  // offsets: non-decreasing on both sides; capacity: the real offsets (read back here, the operator is no hot path) lie inside the capacities
  std::vector<int> dev(n_utt + 1);
  STTS_HIP(hipStreamSynchronize(st));
  STTS_HIP(hipMemcpy(dev.data(), p->seg_off_dev, dev.size() * sizeof(int), hipMemcpyDeviceToHost));
  STTS_CHECK(p->seg_off_host[0] == 0 && dev[0] == 0, "op_conv1d_epi: offsets start at 0");
  for (int u = 0; u < n_utt; ++u) {
    const int cap = p->seg_off_host[u + 1] - p->seg_off_host[u], len = dev[u + 1] - dev[u];
    STTS_CHECK(cap >= 0 && len >= 0 && len <= cap && dev[u] <= p->seg_off_host[u], "op_conv1d_epi: utterance %d: %d rows at %d, capacity %d at %d", u, len, dev[u], cap,
               p->seg_off_host[u]);
    STTS_CHECK(p->capacity || (len == cap && dev[u] == p->seg_off_host[u]), "op_conv1d_epi: host and device offsets differ without the capacity flag (utterance %d)", u);
  }
  Seg s{n_utt, p->seg_off_host, p->seg_off_dev, p->capacity != 0};
  const long R = s.rows();
  const int max_len = s.max_len();
  STTS_CHECK(R > 0, "op_conv1d_epi: no rows");
  const int npad = round_up(N, 256);
  // the widest row the kernels may touch: conv_gemm16_kernel prefetches the residual over the whole 256-channel tile (columns >= N are read, not used)
  // (`touched` columns of the last row must still lie inside the buffer; the window itself inside a row)
  auto fits = [&](long elems, int ld, int col0, int touched) { return col0 >= 0 && ld >= col0 + N && (R - 1) * ld + col0 + touched <= elems; };
  STTS_CHECK(!p->y || fits(p->y_elems, p->ldy, p->ycol0, N), "op_conv1d_epi: Y window [%d, %d) x %ld rows outside ldy %d / %ld elements", p->ycol0, p->ycol0 + N, R, p->ldy,
             (long)p->y_elems);
  STTS_CHECK(!p->y16 || fits(p->y16_elems, p->ldy16, p->ycol16, N), "op_conv1d_epi: Y16 window outside its buffer");
  STTS_CHECK(!p->r || fits(p->r_elems, p->ldr, p->rcol0, p->force_tile == 19 ? npad : N), "op_conv1d_epi: residual window (tile 19 reads whole 256-channel tiles) outside its buffer");
  STTS_CHECK(!p->sumsq || (p->ld_ss >= N && p->ss_stride >= ceil_div(max_len, 32) && (long)n_utt * p->ss_stride * p->ld_ss <= p->sumsq_elems),
             "op_conv1d_epi: sumsq_part needs ld_ss >= cout, ss_stride >= ceil(max_len / 32) and n_utt * ss_stride * ld_ss elements");
  STTS_CHECK(!p->stat || p->force_tile == 19, "op_conv1d_epi: output statistics exist only on tile 19 (conv_gemm16_kernel)");
  STTS_CHECK(!p->stat || (p->ld_stat >= N && p->stat_nchunk >= ceil_div(max_len, 128) && (long)n_utt * p->stat_nchunk * 2 * p->ld_stat <= p->stat_elems),
             "op_conv1d_epi: stat_part needs ld_stat >= cout, stat_nchunk >= ceil(max_len / 128) and n_utt * stat_nchunk * 2 * ld_stat elements");
  // (conv_gemm16_kernel stores and loads four channels at a time: gemm_plan.hip.h gemm16_eligible, asked here so that a refusal comes before the row cast)
  STTS_CHECK(p->force_tile != 19 || (N % 4 == 0 && p->ldy % 4 == 0 && p->ycol0 % 4 == 0 && p->ldy16 % 4 == 0 && p->ycol16 % 4 == 0 && p->ldr % 4 == 0 && p->rcol0 % 4 == 0 &&
                                     p->ld_ss % 4 == 0 && p->ld_stat % 4 == 0),
             "op_conv1d_epi: tile 19 needs cout, every leading dimension and every first column in multiples of 4");
  for (int i = 0; i < p->nseg; ++i) {
    const stts_conv_epi_seg& g = p->seg[i];
    STTS_CHECK(g.x && g.w_host && g.cin > 0 && g.k > 0 && g.k % 2 == 1 && g.dil > 0, "op_conv1d_epi: segment %d: null operand, or k not odd", i);
    STTS_CHECK(g.ldx % 32 == 0 && g.ldx >= round_up(g.cin, 64) && R * g.ldx <= g.x_elems, "op_conv1d_epi: segment %d: ldx must be a multiple of 32 covering cin padded to 64, x [rows, ldx]", i);
  }
  stts_ctx tmp;  // only for allocation bookkeeping
  tmp.prec = p->precision;
  tmp.allow_x3 = false;
  PackScope scope(&tmp, engine_mode(&tmp));
  struct FreeAll {  // every exit path waits for the stream and frees the temporaries
    stts_ctx& t;
    hipStream_t st;
    ~FreeAll() {
      (void)hipStreamSynchronize(st);
      for (void* q : t.allocs) (void)hipFree(q);
    }
  } free_all{tmp, st};
  std::vector<int> rows256(npad, -1);
  for (int i = 0; i < N; ++i) rows256[i] = i;
  HostTensor b;
  b.shape = {N};
  if (p->bias_host) b.data.assign(p->bias_host, p->bias_host + N);
  PackedConv pc[2];
  GemmArgs a = gemm_args(s);
  for (int i = 0; i < p->nseg; ++i) {
    const stts_conv_epi_seg& g = p->seg[i];
    HostTensor w;
    w.shape = {N, g.cin, g.k};
    w.data.assign(g.w_host, g.w_host + (size_t)N * g.cin * g.k);
    STTS_TRY(pack_rows(&tmp, w, (i == 0 && p->bias_host) ? &b : nullptr, rows256, 0, g.cin, round_up(g.cin, 64), N, &pc[i]));
    unsigned short* x16 = nullptr;
    STTS_HIP(hipMalloc(&x16, (size_t)R * g.ldx * sizeof(unsigned short)));
    tmp.allocs.push_back(x16);
    launch_cast_rows(st, p->precision, g.x, g.ldx, g.ldx, x16, g.ldx, R);
    set_seg(a, i, reinterpret_cast<const float*>(x16), g.ldx, 0, pc[i], (g.k - 1) / 2, g.dil);
  }
  a.x16 = 1;
  a.N = N; a.bias = pc[0].bias; a.act = p->act; a.alpha = p->alpha; a.tune = p->tune;
  a.Y = p->y; a.ldy = p->ldy; a.ycol0 = p->ycol0;
  a.Y16 = p->y16; a.ldy16 = p->ldy16; a.ycol16 = p->ycol16;
  a.R = p->r; a.ldr = p->ldr; a.rcol0 = p->rcol0;
  a.sumsq_part = p->sumsq; a.ld_ss = p->ld_ss; a.ss_stride = p->ss_stride;
  a.stat_part = p->stat; a.ld_stat = p->ld_stat; a.stat_nchunk = p->stat_nchunk;
  STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, npad, n_utt, max_len, p->force_tile));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

static int op_scratch(Arena& a, const Seg& s, int kc, int cout, float** act1, float** h, float** act2, float** ss, float** sty, int ld_sty) {
  const long R = s.rows();
  const int n_utt = s.n_utt;
  *act1 = a.get<float>(R * kc);
  *h = a.get<float>(R * cout);
  *act2 = a.get<float>(R * cout);
  *ss = a.get<float>(adain_part_floats(s, std::max(kc, cout)));
  *sty = a.get<float>((size_t)n_utt * ld_sty);
  STTS_CHECK(a.ok, "op: workspace too small");
  return 0;
}

int stts_op_adain_block(stts_ctx* c, void* stream, const char* prefix, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev,
                        const float* x, int ldx, int cin, int cout, const float* style, float* y, int ldy, void* ws, size_t ws_bytes) {
  API_BEGIN
  STTS_CHECK(c && prefix, "null argument");
  hipStream_t st = (hipStream_t)stream;
  std::string key = prefix;
  if (!c->op_blocks.count(key)) {
    auto blk = std::make_unique<AdainBlockW>();
    auto tab = std::make_unique<StyleTable>();
    PackScope scope(c, engine_mode(c));
    STTS_TRY(pack_adain_block(c, key, cin, cout, tab.get(), blk.get()));
    STTS_TRY(upload_table(c, tab.get()));
    c->op_blocks[key] = std::move(blk);
    c->op_tables[key] = std::move(tab);
  }
  const AdainBlockW& B = *c->op_blocks[key];
  const StyleTable& T = *c->op_tables[key];
  STTS_CHECK(ldx == B.kcin, "op_adain_block: ldx must equal cin padded to 32 (%d)", B.kcin);
  Seg s{n_utt, seg_off_host, seg_off_dev};
  Arena a(ws, ws_bytes);
  BlockIO io;  // (no Winograd scratch, no chain: the folded form or the apply pass)
  float* sty;
  STTS_TRY(op_scratch(a, s, B.kcin, B.cout, &io.act1, &io.hbuf, &io.act2, &io.ss, &sty, T.ld()));
  STTS_TRY(run_style(st, T, style, n_utt, sty));
  io.style = sty; io.ld_style = T.ld(); io.x = x; io.ldx = ldx; io.y = y; io.ldy = ldy;
  BlockChain chain;
  return adain_block(st, s, B, io, chain, block_switches());
  API_END
}

// One block, or two chained ones, under the caller's BlockSwitches and offers (include/stylish_hip.h).  The walk is decoder_forward's: chain plan, the carving,
// the constant columns (ConstColumns), block A, the rounded tail, block B, the chain's pending reduce.  Every buffer is checked before anything is launched.
int stts_op_adain_chain(stts_ctx* c, void* stream, const stts_adain_chain_args* p) {
  API_BEGIN
  STTS_CHECK(c && p && p->seg_off_host && p->seg_off_dev && p->x && p->style && p->ws && p->plan_out && p->n_utt > 0, "op_adain_chain: null / empty argument");
  STTS_CHECK(p->nblocks == 1 || p->nblocks == 2, "op_adain_chain: one or two blocks");
  hipStream_t st = (hipStream_t)stream;
  const int nb = p->nblocks;
  for (int i = 0; i < nb; ++i) STTS_CHECK(p->blocks[i].prefix && p->blocks[i].y && p->blocks[i].cin > 0 && p->blocks[i].cout > 0, "op_adain_chain: block %d: null / empty argument", i);
  std::string key = "chain:";
  for (int i = 0; i < nb; ++i) key += std::string(p->blocks[i].prefix) + "|";
  if (!c->op_tables.count(key)) {  // the blocks of a chain share one style table (the bridge reads the next block's norm1 from this block's)
    auto tab = std::make_unique<StyleTable>();
    std::unique_ptr<AdainBlockW> blk[2];
    PackScope scope(c, {c->prec, true, c->prec != PREC_F32 ? 64 : 32, 0});  // (the frame path's packing: input channels padded to conv_gemm16_kernel's K tile in the 16-bit modes)
    for (int i = 0; i < nb; ++i) {
      blk[i] = std::make_unique<AdainBlockW>();
      STTS_TRY(pack_adain_block(c, p->blocks[i].prefix, p->blocks[i].cin, p->blocks[i].cout, tab.get(), blk[i].get()));
    }
    STTS_TRY(upload_table(c, tab.get()));
    for (int i = 0; i < nb; ++i) c->op_blocks[key + std::to_string(i)] = std::move(blk[i]);
    c->op_tables[key] = std::move(tab);
  }
  AdainBlockW B[2];
  for (int i = 0; i < nb; ++i) {
    B[i] = *c->op_blocks[key + std::to_string(i)];
    STTS_CHECK(B[i].cin == p->blocks[i].cin && B[i].cout == p->blocks[i].cout, "op_adain_chain: block %d was packed as %d -> %d", i, B[i].cin, B[i].cout);
  }
  const StyleTable& T = *c->op_tables[key];
  const int prec = B[0].conv1.prec;
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  STTS_CHECK(R > 0, "op_adain_chain: no rows");
  // ---- the caller's buffers
  STTS_CHECK(p->ldx >= B[0].kcin && p->ldx % 4 == 0 && R * p->ldx <= p->x_elems, "op_adain_chain: x must be [rows, ldx >= %d, a multiple of 4]", B[0].kcin);
  STTS_CHECK((long)p->n_utt * T.K <= p->style_elems, "op_adain_chain: style must be [n_utt, %d]", T.K);
  for (int i = 0; i < nb; ++i) {
    const stts_adain_chain_block& b = p->blocks[i];
    STTS_CHECK(b.ldy >= b.cout && b.ldy % 4 == 0 && R * b.ldy <= b.y_elems, "op_adain_chain: block %d: y must be [rows, ldy >= cout, a multiple of 4]", i);
    STTS_CHECK(!b.y16 || (prec != PREC_F32 && b.cout % 8 == 0 && b.ldy16 >= b.cout && b.ldy16 % 8 == 0 && R * b.ldy16 <= b.y16_elems),
               "op_adain_chain: block %d: y16 needs a 16-bit mode, cout and ldy16 multiples of 8, [rows, ldy16 >= cout]", i);
  }
  if (nb == 2) {
    STTS_CHECK(B[1].cin >= B[0].cout && p->blocks[0].ldy >= B[1].kcin, "op_adain_chain: block 1 reads [y_0 | constant columns]: cin %d >= cout %d, ldy_0 >= %d", B[1].cin, B[0].cout, B[1].kcin);
    STTS_CHECK(!p->blocks[0].y16 || p->blocks[0].ldy16 == p->blocks[0].ldy, "op_adain_chain: the rounded copy of y_0 is block 1's rounded input: ldy16 == ldy");
  }
  // ---- switches and offers
  BlockSwitches sw = block_switches();  // (x3_presplit: per call, as everywhere)
  // (a negative threshold: the engine's own, block_switches())
  if (p->fold_rows >= 0) sw.fold_rows = p->fold_rows;
  if (p->fold16_rows >= 0) sw.fold16_rows = p->fold16_rows;
  if (p->rows16 >= 0) sw.rows16 = p->rows16;
  if (p->sc_side_min_rows >= 0) sw.sc_side_min_rows = p->sc_side_min_rows;
  sw.affine_serial = p->affine_serial != 0; sw.no_wino_conv2sc = p->no_wino_conv2sc != 0; sw.no_stat_fuse = p->no_stat_fuse != 0; sw.no_wino_stats = p->no_wino_stats != 0;
  sw.bridge = p->bridge;
  const int probe = nb - 1;  // (the wider input)
  ChainOffer offer{p->offer_stats != 0, p->offer_rows16 != 0, true, p->offer_side != 0};
  const bool scratch = p->offer_wino != 0 && p->force_tile == 0;  // (without it plan_adain_block keeps every conv a direct contraction, whatever the chain plan carved for)
  const ChainPlan plan = plan_adain_chain(s, prec, B, nb, probe, offer, sw);
  int32_t* out = p->plan_out;
  const int32_t cp[8] = {plan.wino && scratch, plan.sc_out, plan.rows16, plan.wino_stats, plan.stats, plan.bridge_w, plan.side, 0};
  std::copy(cp, cp + 8, out);
  std::fill(out + 8, out + 8 + 16 * nb, -1);
  // ---- the carving (decoder_forward's)
  int ldwide = p->ldx, cwide = 0;
  for (int i = 0; i < nb; ++i) {
    ldwide = std::max({ldwide, B[i].kcin, B[i].cout, (int)p->blocks[i].ldy});
    cwide = std::max(cwide, B[i].cout);
  }
  Arena ws(p->ws, (size_t)p->ws_bytes);
  BlockIO io;
  io.act1 = ws.get<float>(R * ldwide);
  io.hbuf = ws.get<float>(R * cwide);
  io.act2 = ws.get<float>(R * cwide);
  io.ss = ws.get<float>(adain_part_floats(s, ldwide));
  float* ss_in = ws.get<float>(adain_part_floats(s, ldwide, kWinoStatChunk));
  float* ss_mid = ws.get<float>(adain_part_floats(s, ldwide, kWinoStatChunk));
  float* sty = ws.get<float>((size_t)s.n_utt * T.ld());
  WinoScratch wino;
  if (plan.wino && scratch) {
    size_t floats = 0;
    for (int i = 0; i < nb; ++i) floats = std::max({floats, wino_scratch_floats(s, B[i].w1), B[i].w2.ready ? wino_scratch_floats(s, B[i].w2) : 0});
    wino.p = ws.get<float>(floats);
  }
  float* sc_out = plan.sc_out ? ws.get<float>(R * cwide) : nullptr;
  // (16-bit scratch wherever the caller offers it, so that a block plan that disagrees with the chain plan would show; only the chain plan's rows16 rounds the tail)
  unsigned short* xs16a = p->offer_rows16 ? ws.get<unsigned short>(R * ldwide) : nullptr;
  unsigned short* xs16b = p->offer_rows16 ? ws.get<unsigned short>(R * ldwide) : nullptr;
  STTS_CHECK(ws.ok, "op_adain_chain: workspace too small");
  struct Lane {  // the side lane: created and destroyed here, after both streams have drained
    hipStream_t main, stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    ~Lane() {
      (void)hipStreamSynchronize(main);
      if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
      if (fork) (void)hipEventDestroy(fork);
      if (join) (void)hipEventDestroy(join);
    }
  } lane{st};
  SideWork side;
  if (plan.side) {
    STTS_HIP(hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking));
    STTS_HIP(hipEventCreateWithFlags(&lane.fork, hipEventDisableTiming));
    STTS_HIP(hipEventCreateWithFlags(&lane.join, hipEventDisableTiming));
    side.stream = lane.stream; side.fork = lane.fork; side.join = lane.join; side.out = sc_out;
    io.side = &side;
  }
  STTS_TRY(run_style(st, T, p->style, s.n_utt, sty));
  io.style = sty; io.ld_style = T.ld();
  io.wino = &wino;
  BlockChain chain(plan, ss_mid);
  chain.defer = p->defer != 0;
  ConstColumns cst;
  if (nb == 2) {
    cst.x = p->blocks[0].y; cst.ld = p->blocks[0].ldy; cst.hidden = B[0].cout; cst.ccat = B[1].cin; cst.ss_in = ss_in; cst.out_ld = round_up(B[1].cin, 32);
  }
  if (plan.bridge_w) {
    wino.mp_kc = B[probe].w1.planes.kc;
    if (nb == 2) {
      cst.offer_bridge(chain);
      STTS_TRY(cst.stats(st, s, chain, true));
    }
  }
  auto block = [&](int i) -> int {
    const BlockPlan bp = plan_adain_block(B[i], s, io, chain, p->force_tile, sw);
    const int32_t v[16] = {bp.conv1, bp.conv2, bp.rows16, bp.norm1, bp.norm2, bp.next_norm1, bp.take_pending, bp.defer_conv2, bp.shortcut, bp.cast_x16, bp.y16, bp.affine_serial,
                           bp.bridge_w, bp.force_tile, 0, 0};
    std::copy(v, v + 16, out + 8 + 16 * i);
    STTS_TRY(run_adain_block(st, s, B[i], bp, io, chain));
    out[8 + 16 * i + 14] = chain.pend.src.partial ? chain.pend.src.ksplit : 0;  // what conv2 left pending: its split-K factor
    return 0;
  };
  auto blocks = [&]() -> int {
    io.x = p->x; io.ldx = p->ldx; io.y = p->blocks[0].y; io.ldy = p->blocks[0].ldy;
    io.xs16 = xs16b; io.y16 = p->blocks[0].y16; io.ldy16 = p->blocks[0].ldy16;
    // (a single block leaves the statistics of y as if a block of its own width followed)
    chain.link(nullptr, false, offer.stats ? ss_in : nullptr, nb == 2 ? cst.out_ld : round_up(B[0].cout, 32), plan.bridge_w && nb == 2 ? &B[1] : nullptr);
    STTS_TRY(block(0));
    if (nb == 1) return 0;
    unsigned short* x16 = p->blocks[0].y16 ? p->blocks[0].y16 : xs16a;
    if (plan.rows16 && x16) cst.cast_tail(st, prec, p->blocks[0].y, x16, R);
    STTS_TRY(cst.stats(st, s, chain, plan.bridge_w != 0));
    io.x = p->blocks[0].y; io.ldx = p->blocks[0].ldy; io.y = p->blocks[1].y; io.ldy = p->blocks[1].ldy;
    io.xs16 = x16; io.xs16_ready = plan.rows16 && p->blocks[0].y16; io.y16 = p->blocks[1].y16; io.ldy16 = p->blocks[1].ldy16;
    chain.link(ss_in, chain.out_ready, nullptr, cst.out_ld, nullptr);
    return block(1);
  };
  int rc = blocks();
  if (rc && plan.side) {  // an error path may have left a shortcut running on the side lane
    (void)hipEventRecord(side.join, side.stream);
    (void)hipStreamWaitEvent(st, side.join, 0);
  }
  if (rc) return rc;
  STTS_TRY(chain.finish(st));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_attention(void* stream, int n_utt, const int32_t* q_off_host, const int32_t* q_off_dev, const int32_t* k_off_host,
                      const int32_t* k_off_dev, const float* q, const float* k, const float* v, float* o, int heads, int kc,
                      const int32_t* band_centre, int window, int kernel) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && q_off_host && q_off_dev && k_off_host && k_off_dev && q && k && v && o && heads > 0, "null / empty argument");
  Seg sq{n_utt, q_off_host, q_off_dev}, sk{n_utt, k_off_host, k_off_dev};
  const int ld = heads * kc;
  return run_attention((hipStream_t)stream, sq, sk, q, ld, 0, k, ld, 0, v, ld, 0, o, ld, heads, kc, band_centre, window, kernel);
  API_END
}

// wavlm_l1_kernel + wavlm_l1_finish_kernel (wavlm.hip.h) on two row buffers packed alike: sums[u] = sum |a - b| over utterance u's rows, in double.
// part: device scratch of n_utt * ceil(max_len / 8) doubles.
int stts_op_wavlm_l1(void* stream, int n_utt, const int32_t* off_host, const int32_t* off_dev, const float* a, const float* b, int ld, int C, double* part,
                     double* sums, int32_t* frames) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && off_host && off_dev && a && b && part && sums && C > 0 && ld >= C, "null / empty argument");
  Seg s{n_utt, off_host, off_dev};
  const int ml = s.max_len();
  STTS_TRY(launch_wavlm_l1((hipStream_t)stream, a, b, ld, C, n_utt, off_dev, ml, part));
  hipLaunchKernelGGL(wavlm_l1_finish_kernel, dim3(ceil_div(n_utt, 64)), dim3(64), 0, (hipStream_t)stream, part, 1, n_utt, ceil_div(std::max(1, ml), kWavlmL1Rows), off_dev, sums,
                     frames);
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// The vocoder's STFT / iSTFT kernels at a geometry (n_fft, win, hop 4h) without a model: the launches of harmonic_stft / vocoder_body, with
// this geometry's tables.  generic 0: the kernels the engine picks (signal.hip.h at 2048 / 1200 / 300), 1: signal_geom.hip.h always.
struct GeomOpTables {
  stts_ctx tmp;  // only for allocation bookkeeping
  hipStream_t st;
  SignalGeom g;
  float* hann = nullptr;
  double2* tw64 = nullptr;
  explicit GeomOpTables(hipStream_t s) : st(s) {}
  int init(int n_fft, int win, int h, int generic) {
    STTS_TRY(signal_geometry(n_fft, win, 4 * h, 24000, generic != 0, &g));
    std::vector<float> hw;
    std::vector<double2> tw;
    signal_tables(n_fft, win, &hw, &tw);
    PackScope scope(&tmp, engine_mode(&tmp));
    STTS_TRY(dev_upload(&tmp, hw, &hann));
    STTS_TRY(dev_upload(&tmp, tw, &tw64));
    return 0;
  }
  ~GeomOpTables() {  // every exit path waits for the stream and frees the temporaries
    (void)hipStreamSynchronize(st);
    for (void* p : tmp.allocs) (void)hipFree(p);
  }
};

int stts_op_stft_geom(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int n_fft, int win, int h, const float* sig,
                      float* spec, float* phase, int ld, int generic) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && seg_off_host && seg_off_dev && sig && spec && phase, "null / empty argument");
  hipStream_t st = (hipStream_t)stream;
  GeomOpTables t(st);
  STTS_TRY(t.init(n_fft, win, h, generic));
  const SignalGeom& g = t.g;
  Seg s{n_utt, seg_off_host, seg_off_dev};
  for (int u = 0; u < n_utt; ++u)
    STTS_CHECK((long)(seg_off_host[u + 1] - seg_off_host[u]) * h > n_fft / 2, "op_stft_geom: utterance %d too short for reflect padding", u);
  if (g.generic) {
    STTS_CHECK(ld >= g.bins, "op_stft_geom: ld %d < %d bins", ld, g.bins);
    STTS_TRY(launch_stft_geom(st, g, n_utt, seg_off_dev, s.rows(), s.max_len(), sig, t.hann, t.tw64, spec, phase, ld, 0));
  } else {
    STTS_CHECK(ld >= kBins && ld <= 64 * ((kBins + 63) / 64), "op_stft_geom: ld %d outside [%d, %d]", ld, kBins, 64 * ((kBins + 63) / 64));
    hipLaunchKernelGGL(stft_kernel, dim3(ceil_div(s.max_len(), kFftWaves), n_utt), dim3(64 * kFftWaves), 0, st, sig, seg_off_dev, t.hann, t.tw64, spec, phase, ld, 0);
  }
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

// logamp / phase [frames, ld] (bins 0 .. n_fft/2) -> audio, h samples per frame (tanh of the normalised overlap-add, as the vocoder)
int stts_op_istft_geom(void* stream, int n_utt, const int32_t* seg_off_host, const int32_t* seg_off_dev, int n_fft, int win, int h, const float* logamp,
                       const float* phase, int ld, float* audio, int generic) {
  API_BEGIN
  STTS_CHECK(n_utt > 0 && seg_off_host && seg_off_dev && logamp && phase && audio, "null / empty argument");
  hipStream_t st = (hipStream_t)stream;
  GeomOpTables t(st);
  STTS_TRY(t.init(n_fft, win, h, generic));
  const SignalGeom& g = t.g;
  STTS_CHECK(ld >= g.bins, "op_istft_geom: ld %d < %d bins", ld, g.bins);
  Seg s{n_utt, seg_off_host, seg_off_dev};
  float* yw = nullptr;
  STTS_HIP(hipMalloc(&yw, (size_t)(s.rows() + n_utt) * g.win * sizeof(float)));
  t.tmp.allocs.push_back(yw);
  if (g.generic) {
    STTS_TRY(launch_istft_geom(st, g, n_utt, seg_off_dev, s.rows(), s.max_len(), logamp, phase, ld, t.hann, t.tw64, yw, audio));
  } else {
    const int ml = s.max_len();
    hipLaunchKernelGGL(istft_frames_kernel, dim3(ceil_div(ml + 1, kFftWaves), n_utt), dim3(64 * kFftWaves), 0, st, logamp, phase, ld, seg_off_dev, t.hann, t.tw64, yw);
    hipLaunchKernelGGL(istft_ola_kernel, dim3(std::min(1024, ceil_div(ml * kHop, 256)), n_utt), dim3(256), 0, st, yw, seg_off_dev, t.hann, audio);
  }
  STTS_HIP(hipGetLastError());
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ the kernels between the contractions
// stts_op_adain / _wino_stat / _row_layernorm / _dwconv / _grn (include/stylish_hip.h; tests/test_hip_norm_kernels.py).  Each follows stts_op_conv1d_epi:
// the checks come first and are complete - every index a launch can form is bounded by the caller's element counts - and only then is anything launched.
namespace {
// offsets: start at 0, non-decreasing, the same on both sides (read back here: the operators are no hot path)
int norm_op_offsets(hipStream_t st, const char* op, int n_utt, const int32_t* host, const int32_t* dev) {
  STTS_CHECK(host && dev && n_utt > 0, "%s: null / empty offsets", op);
  std::vector<int> d(n_utt + 1);
  STTS_HIP(hipStreamSynchronize(st));
  STTS_HIP(hipMemcpy(d.data(), dev, d.size() * sizeof(int), hipMemcpyDeviceToHost));
  STTS_CHECK(host[0] == 0, "%s: offsets start at 0", op);
  for (int u = 0; u <= n_utt; ++u) STTS_CHECK(d[u] == host[u] && (u == 0 || host[u] >= host[u - 1]), "%s: offsets decrease, or host and device offsets differ (utterance %d)", op, u);
  return 0;
}
// rows x [col0, col0 + cols) of a [rows, ld] buffer of `elems` elements
bool norm_op_fits(long rows, int ld, int col0, int cols, long elems) { return col0 >= 0 && cols >= 0 && ld >= col0 + cols && (rows <= 0 || (rows - 1) * (long)ld + col0 + cols <= elems); }
struct NormOpTemps {  // every exit path waits for the stream and frees the temporaries
  stts_ctx tmp;
  hipStream_t st;
  explicit NormOpTemps(hipStream_t s) : st(s) {}
  ~NormOpTemps() {
    (void)hipStreamSynchronize(st);
    for (void* q : tmp.allocs) (void)hipFree(q);
  }
};
}  // namespace

extern "C" {

int stts_op_adain(void* stream, const stts_adain_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_adain: null argument");
  STTS_TRY(norm_op_offsets(st, "op_adain", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  const int n_utt = p->n_utt, C = p->C, ml = s.max_len();
  STTS_CHECK(p->producer >= 0 && p->producer <= 2 && p->consumer >= 0 && p->consumer <= 3, "op_adain: producer 0 - 2, consumer 0 - 3");
  const int chunk_rows = p->producer == 1 ? kWinoStatChunk : kStatChunk;
  STTS_CHECK(chunk_rows <= kStatChunk, "op_adain: chunk_rows above kStatChunk");
  STTS_CHECK(C > 0 && p->x && p->part, "op_adain: C, x and part are required");
  STTS_CHECK(p->ldx % 4 == 0 && norm_op_fits(R, p->ldx, 0, round_up(C, 4), p->x_elems), "op_adain: x [%ld, ldx %d] (ldx %% 4 == 0, covering C = %d rounded up to 4) outside %ld elements", R, p->ldx, C,
             (long)p->x_elems);
  STTS_CHECK(p->ldp >= C && p->nchunk >= ceil_div(ml, chunk_rows) && (long)n_utt * p->nchunk * 2 * p->ldp <= p->part_elems,
             "op_adain: part needs ldp >= C, nchunk >= ceil(max_len / %d) and n_utt * nchunk * 2 * ldp elements", chunk_rows);
  SplitSrc src{};
  if (p->producer == 2) {
    STTS_CHECK(p->partial && p->ksplit >= 1 && p->split_n > 0 && p->split_n <= C, "op_adain: producer 2 needs partial slices and 0 < split_n <= C");
    STTS_CHECK(p->slice_rows >= R && p->ld_part >= p->split_n && (long)p->ksplit * p->slice_rows * p->ld_part <= p->partial_elems,
               "op_adain: partial [ksplit][slice_rows >= rows][ld_part >= split_n] outside its buffer");
    STTS_CHECK(!p->bias || p->bias_elems >= p->split_n, "op_adain: bias shorter than split_n");
    STTS_CHECK(!p->r || norm_op_fits(R, p->ldr, p->rcol0, p->split_n, p->r_elems), "op_adain: residual window outside its buffer");
    STTS_CHECK(p->split_act >= ACT_NONE && p->split_act <= ACT_LRELU, "op_adain: split_act out of range");
    src = SplitSrc{p->partial, p->ksplit, p->slice_rows, p->ld_part, p->split_n, p->bias, p->split_act, p->r, p->ldr, p->rcol0, p->split_alpha};
  }
  if (p->consumer) STTS_CHECK(p->gb && p->ld_gb >= 0 && p->gcol0 >= 0 && (long)(n_utt - 1) * p->ld_gb + p->gcol0 + 2 * C <= p->gb_elems, "op_adain: style rows (gamma, beta at gcol0) outside gb");
  if (p->consumer == 1 || p->consumer == 2)
    STTS_CHECK(p->aff && p->ld_aff >= C && (long)n_utt * 2 * p->ld_aff <= p->aff_elems, "op_adain: aff needs ld_aff >= C and n_utt * 2 * ld_aff elements");
  if (p->consumer == 3) {
    STTS_CHECK(p->producer != 1, "op_adain: adain_apply_kernel merges chunks of %d rows", kStatChunk);
    STTS_CHECK(p->ldp == round_up(C, 32) && p->nchunk == ceil_div(ml, kStatChunk), "op_adain: run_adain lays the table out as [ceil(max_len / 128)][2][round_up(C, 32)]");
    STTS_CHECK(p->rb == 64 || p->rb == 256, "op_adain: rb is 64 or 256");
    STTS_CHECK(p->act >= ACT_NONE && p->act <= ACT_LRELU, "op_adain: act out of range");
    STTS_CHECK(p->out16 == 0 || p->out16 == PREC_BF16 || p->out16 == PREC_F16, "op_adain: out16 is 0, STTS_PREC_BF16 or _F16");
    STTS_CHECK(p->y && p->ldy % 4 == 0 && norm_op_fits(R, p->ldy, 0, std::max(p->ldy, C), p->y_elems), "op_adain: y [rows, ldy] (ldy %% 4 == 0, ldy >= C) outside its buffer");
    STTS_CHECK(!p->snake || p->snake_elems >= C, "op_adain: snake alpha shorter than C");
  }
  if (R == 0) return 0;
  const dim3 pg(ceil_div(C, 32), std::max(1, ceil_div(ml, chunk_rows)), n_utt);
  if (p->producer == 2)
    hipLaunchKernelGGL(adain_partial_reduce_kernel, pg, dim3(256), 0, st, p->x, p->ldx, C, s.dev, p->part, p->ldp, p->nchunk, src);
  else
    hipLaunchKernelGGL(adain_partial_kernel, pg, dim3(256), 0, st, (const float*)p->x, p->ldx, C, s.dev, p->part, p->ldp, p->nchunk, chunk_rows);
  if (p->consumer == 1)
    hipLaunchKernelGGL(adain_affine_kernel, dim3(ceil_div(p->ld_aff, 64), n_utt), dim3(64), 0, st, (const float*)p->part, p->ldp, p->nchunk, s.dev, p->gb, p->ld_gb, p->gcol0, C, 1e-5f, p->aff,
                       p->ld_aff, chunk_rows);
  else if (p->consumer == 2)
    hipLaunchKernelGGL(adain_affine_lanes_kernel, dim3(ceil_div(p->ld_aff, 16), n_utt), dim3(256), 0, st, (const float*)p->part, p->ldp, p->nchunk, s.dev, p->gb, p->ld_gb, p->gcol0, C, 1e-5f,
                       p->aff, p->ld_aff, chunk_rows);
  else if (p->consumer == 3)
    STTS_TRY(run_adain(st, s, p->x, p->ldx, C, reinterpret_cast<float*>(p->y), p->ldy, p->gb, p->ld_gb, p->gcol0, p->act, p->snake, p->part, p->out16, true, p->rb));
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_wino_stat(void* stream, const stts_wino_stat_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_wino_stat: null argument");
  STTS_TRY(norm_op_offsets(st, "op_wino_stat", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  STTS_CHECK(R > 0 && p->x && p->w_host && p->y && p->stat && p->cin > 0 && p->cout > 0, "op_wino_stat: null / empty argument");
  STTS_CHECK(p->k == 3 || p->k == 7, "op_wino_stat: the Winograd forms are F(6, 3) and F(6, 7)");
  STTS_CHECK(p->precision == 0 || p->precision == 3, "op_wino_stat: precision must be STTS_PREC_F32 or _F32_NATIVE");
  STTS_CHECK(p->act >= ACT_NONE && p->act <= ACT_LRELU, "op_wino_stat: act out of range");
  STTS_CHECK(p->ldx % 32 == 0 && norm_op_fits(R, p->ldx, 0, p->ldx, p->x_elems) && p->ldx >= p->cin, "op_wino_stat: ldx must be a multiple of 32 covering cin, x [rows, ldx]");
  STTS_CHECK(p->ldy % 4 == 0 && norm_op_fits(R, p->ldy, 0, round_up(p->cout, 4), p->y_elems), "op_wino_stat: y [rows, ldy] (ldy %% 4 == 0, covering cout rounded up to 4) outside its buffer");
  STTS_CHECK(p->ld_stat % 4 == 0 && p->ld_stat >= round_up(p->cout, 4) && p->stat_nchunk == wino_stat_chunks(s) && (long)p->n_utt * p->stat_nchunk * 2 * p->ld_stat <= p->stat_elems,
             "op_wino_stat: stat needs ld_stat %% 4 == 0 covering cout, stat_nchunk == %d and n_utt * stat_nchunk * 2 * ld_stat elements", wino_stat_chunks(s));
  NormOpTemps t(st);
  stts_ctx& tmp = t.tmp;
  tmp.prec = 0;
  tmp.allow_x3 = p->precision != 3;
  PackScope scope(&tmp, engine_mode(&tmp));
  HostTensor w;
  w.shape = {p->cout, p->cin, p->k};
  w.data.assign(p->w_host, p->w_host + (size_t)p->cout * p->cin * p->k);
  HostTensor b;
  b.shape = {p->cout};
  if (p->bias_host) b.data.assign(p->bias_host, p->bias_host + p->cout);
  WinoConv wc;
  STTS_TRY(pack_winograd(&tmp, w, p->bias_host ? &b : nullptr, 0, p->cin, p->cout, &wc));
  float* scratch = nullptr;
  STTS_HIP(hipMalloc(&scratch, wino_scratch_floats(s, wc) * sizeof(float)));
  tmp.allocs.push_back(scratch);
  WinoScratch wz;
  wz.p = scratch;
  STTS_TRY(run_winograd(st, s, p->x, p->ldx, wc, p->y, p->ldy, p->act, nullptr, 0, 1.0f, wz, nullptr, 0, p->stat, p->ld_stat));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_row_layernorm(void* stream, const stts_row_layernorm_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_row_layernorm: null argument");
  const int C = p->C;
  const long R = p->n_rows;
  STTS_CHECK(C > 0 && C % 4 == 0 && C <= 2048, "op_row_layernorm: C must be a multiple of 4, at most 2048");
  STTS_CHECK(R > 0 && (p->nout == 1 || p->nout == 2) && p->act >= ACT_NONE && p->act <= ACT_LRELU, "op_row_layernorm: n_rows, nout (1 or 2) or act out of range");
  STTS_CHECK(p->n_rows_real <= R, "op_row_layernorm: n_rows_real above n_rows");
  if (p->adaptive) {
    STTS_TRY(norm_op_offsets(st, "op_row_layernorm", p->n_utt, p->seg_off_host, p->seg_off_dev));
    STTS_CHECK(p->seg_off_host[p->n_utt] == R, "op_row_layernorm: the offsets must cover n_rows");
  }
  LnIn in{};
  if (p->partial) {
    STTS_CHECK(p->ksplit >= 1 && p->slice_rows >= R && p->ld_part % 4 == 0 && p->ld_part >= C && (long)p->ksplit * p->slice_rows * p->ld_part <= p->partial_elems,
               "op_row_layernorm: partial [ksplit][slice_rows >= n_rows][ld_part >= C, %% 4 == 0] outside its buffer");
    STTS_CHECK(!p->bias || p->bias_elems >= C, "op_row_layernorm: bias shorter than C");
    STTS_CHECK(!p->r || norm_op_fits(R, p->ldr, p->rcol0, C, p->r_elems), "op_row_layernorm: residual window outside its buffer");
    STTS_CHECK(p->in_act >= ACT_NONE && p->in_act <= ACT_LRELU, "op_row_layernorm: in_act out of range");
    in = LnIn{p->partial, p->ksplit, p->slice_rows, p->ld_part, p->bias, p->in_act, p->r, p->ldr, p->rcol0, p->in_alpha};
  } else {
    STTS_CHECK(p->x && p->ldx % 4 == 0 && norm_op_fits(R, p->ldx, 0, C, p->x_elems), "op_row_layernorm: x [n_rows, ldx] (ldx %% 4 == 0, ldx >= C) outside its buffer");
  }
  LnOut o[2] = {};
  for (int k = 0; k < p->nout; ++k) {
    const stts_ln_out& q = p->out[k];
    STTS_CHECK(q.y && q.g && (q.prec16 == 0 || q.prec16 == PREC_BF16 || q.prec16 == PREC_F16), "op_row_layernorm: output %d: null tensor or prec16 out of range", k);
    STTS_CHECK(q.ldy % 4 == 0 && q.ycol0 % 4 == 0 && norm_op_fits(R, q.ldy, q.ycol0, C, q.y_elems), "op_row_layernorm: output %d: window [%d, %d) of ldy %d (multiples of 4) outside its buffer", k,
               q.ycol0, q.ycol0 + C, q.ldy);
    if (p->adaptive)
      STTS_CHECK(q.ld_g % 4 == 0 && q.gcol0 % 4 == 0 && q.gcol0 >= 0 && q.ld_g >= 0 && (long)(p->n_utt - 1) * q.ld_g + q.gcol0 + 2 * C <= q.g_elems,
                 "op_row_layernorm: output %d: style rows (ld_g, gcol0 multiples of 4) outside g", k);
    else
      STTS_CHECK(q.b && q.g_elems >= C && q.b_elems >= C, "op_row_layernorm: output %d: gamma / beta shorter than C", k);
    o[k] = LnOut{reinterpret_cast<float*>(q.y), q.ldy, q.ycol0, q.g, q.b, q.ld_g, q.gcol0, q.prec16};
  }
  NormOpTemps t(st);
  int* row_utt = nullptr;
  if (p->adaptive) {
    STTS_HIP(hipMalloc(&row_utt, R * sizeof(int)));
    t.tmp.allocs.push_back(row_utt);
    Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
    hipLaunchKernelGGL(row_utt_kernel, dim3(std::max(1, ceil_div(s.max_len(), 256)), p->n_utt), dim3(256), 0, st, p->seg_off_dev, p->n_utt, row_utt);
  }
  int* rows_dev = nullptr;
  if (p->n_rows_real >= 0) {
    STTS_HIP(hipMalloc(&rows_dev, sizeof(int)));
    t.tmp.allocs.push_back(rows_dev);
    STTS_HIP(hipMemcpy(rows_dev, &p->n_rows_real, sizeof(int), hipMemcpyHostToDevice));
  }
  STTS_TRY(ln_launch(st, p->x, p->ldx, C, R, row_utt, p->eps, p->adaptive != 0, p->nout, o[0], o[1], p->act, in, rows_dev));
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_dwconv(void* stream, const stts_dwconv_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_dwconv: null argument");
  STTS_TRY(norm_op_offsets(st, "op_dwconv", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  const int C = p->C, K = p->K, ml = s.max_len(), n_utt = p->n_utt;
  STTS_CHECK(R > 0 && p->x && p->w_host && p->bias_host && p->y, "op_dwconv: null / empty argument");
  STTS_CHECK(p->form >= 0 && p->form <= 2, "op_dwconv: form 0 - 2");
  STTS_CHECK(C > 0 && C % 4 == 0 && K >= 1 && K % 2 == 1 && K <= 31, "op_dwconv: C must be a multiple of 4, K odd and at most 31");
  STTS_CHECK(p->form != 1 || (C <= kDwLnMaxC && (K == 3 || K == 7 || K == 15 || K == 31)), "op_dwconv: the fused form takes C <= %d and K in {3, 7, 15, 31}", kDwLnMaxC);
  STTS_CHECK(p->form != 2 || C <= 2048, "op_dwconv: the LayerNorm takes C <= 2048");
  STTS_CHECK(p->ldx % 4 == 0 && norm_op_fits(R, p->ldx, 0, C, p->x_elems), "op_dwconv: x [rows, ldx] (ldx %% 4 == 0, ldx >= C) outside its buffer");
  STTS_CHECK(p->ldy % 4 == 0 && norm_op_fits(R, p->ldy, 0, C, p->y_elems), "op_dwconv: y [rows, ldy] (ldy %% 4 == 0, ldy >= C) outside its buffer");
  if (p->form == 0) {
    STTS_CHECK(p->act >= ACT_NONE && p->act <= ACT_LRELU && p->prec16 == 0, "op_dwconv: form 0 writes fp32 rows with an activation of the contraction's set");
  } else {
    STTS_CHECK(p->act == ACT_NONE && (p->prec16 == 0 || p->prec16 == PREC_BF16 || p->prec16 == PREC_F16), "op_dwconv: forms 1, 2 have no activation; prec16 is 0, STTS_PREC_BF16 or _F16");
    STTS_CHECK(p->style && p->ld_style % 4 == 0 && p->gcol0 % 4 == 0 && p->gcol0 >= 0 && p->ld_style >= 0 && (long)(n_utt - 1) * p->ld_style + p->gcol0 + 2 * C <= p->style_elems,
               "op_dwconv: style rows (ld_style, gcol0 multiples of 4) outside their buffer");
  }
  NormOpTemps t(st);
  stts_ctx& tmp = t.tmp;
  PackScope scope(&tmp, engine_mode(&tmp));
  std::vector<float> wt((size_t)K * C), bv(p->bias_host, p->bias_host + C);  // tap-major [K][C]
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < K; ++k) wt[(size_t)k * C + c] = p->w_host[(size_t)c * K + k];
  float *dwt = nullptr, *db = nullptr;
  STTS_TRY(dev_upload(&tmp, wt, &dwt));
  STTS_TRY(dev_upload(&tmp, bv, &db));
  if (p->form == 1) {
    const dim3 fg(ceil_div(ml, 16), n_utt);
#define STTS_OP_DWLN(KK) hipLaunchKernelGGL((dwconv_ln_kernel<KK, 16>), fg, dim3(256), 0, st, p->x, p->ldx, C, s.dev, (const float*)dwt, (const float*)db, 1e-6f, p->style, p->ld_style, p->gcol0, \
                                            reinterpret_cast<float*>(p->y), p->ldy, p->prec16)
    if (K == 3) STTS_OP_DWLN(3);
    else if (K == 7) STTS_OP_DWLN(7);
    else if (K == 15) STTS_OP_DWLN(15);
    else STTS_OP_DWLN(31);
#undef STTS_OP_DWLN
  } else {
    float* dw = reinterpret_cast<float*>(p->y);
    int ld_dw = p->ldy;
    int* row_utt = nullptr;
    if (p->form == 2) {
      STTS_HIP(hipMalloc(&dw, (size_t)R * C * sizeof(float)));
      tmp.allocs.push_back(dw);
      ld_dw = C;
      STTS_HIP(hipMalloc(&row_utt, R * sizeof(int)));
      tmp.allocs.push_back(row_utt);
      hipLaunchKernelGGL(row_utt_kernel, dim3(ceil_div(ml, 256), n_utt), dim3(256), 0, st, s.dev, n_utt, row_utt);
    }
    hipLaunchKernelGGL((dwconv_kernel<31>), dim3(ceil_div(C, 64), ceil_div(ml, 64), n_utt), dim3(256), 0, st, p->x, p->ldx, dw, ld_dw, C, s.dev, (const float*)dwt, (const float*)db, K, p->act);
    if (p->form == 2) {
      LnOut o0{reinterpret_cast<float*>(p->y), p->ldy, 0, p->style, nullptr, p->ld_style, p->gcol0, p->prec16}, o1{};
      STTS_TRY(ln_launch(st, dw, ld_dw, C, R, row_utt, 1e-6f, 1, 1, o0, o1, ACT_NONE, LnIn{}, nullptr));
    }
  }
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_grn(void* stream, const stts_grn_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_grn: null argument");
  STTS_TRY(norm_op_offsets(st, "op_grn", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const int C = p->C, n_utt = p->n_utt;
  STTS_CHECK(C > 0 && p->part && p->gx && p->mode >= 0 && p->mode <= 2, "op_grn: null argument, or mode outside 0 - 2");
  STTS_CHECK(p->ld_ss >= C && p->ss_stride >= ceil_div(s.max_len(), 32) && (long)n_utt * p->ss_stride * p->ld_ss <= p->part_elems,
             "op_grn: part needs ld_ss >= C, ss_stride >= ceil(max_len / 32) and n_utt * ss_stride * ld_ss elements");
  STTS_CHECK(p->ld_gx >= C && (long)n_utt * p->ld_gx <= p->gx_elems, "op_grn: gx needs ld_gx >= C and n_utt * ld_gx elements");
  if (p->mode == 1) {
    STTS_CHECK(p->gamma && p->gamma_elems >= C && p->xaff && p->ld_xaff >= C && (long)n_utt * 2 * p->ld_xaff <= p->xaff_elems, "op_grn: xaff needs gamma [C], ld_xaff >= C and n_utt * 2 * ld_xaff elements");
  } else if (p->mode == 2) {
    STTS_CHECK(p->prec == PREC_F32 || p->prec == PREC_BF16 || p->prec == PREC_F16, "op_grn: prec is STTS_PREC_F32, _BF16 or _F16");
    STTS_CHECK(p->kc == C && C % 4 == 0 && p->ld_gx % 4 == 0, "op_grn: scale_weight_kernel averages gx over kc columns, four at a time: kc == C, C %% 4 == 0, ld_gx %% 4 == 0");
    STTS_CHECK(p->gamma && p->gamma_elems >= C && p->w && p->wu && p->npad > 0 && (long)p->npad * p->kc <= p->w_elems && (long)n_utt * p->npad * p->kc <= p->wu_elems,
               "op_grn: scale_weight needs gamma [kc], w [npad][kc] and wu [n_utt][npad][kc]");
  }
  hipLaunchKernelGGL(grn_gx_kernel, dim3(ceil_div(C, 32), n_utt), dim3(256), 0, st, p->part, p->ld_ss, p->ss_stride, s.dev, C, p->gx, p->ld_gx);
  if (p->mode == 1) hipLaunchKernelGGL(grn_xaff_kernel, dim3(n_utt), dim3(256), 0, st, (const float*)p->gx, p->ld_gx, p->gamma, p->xaff, p->ld_xaff, C);
  else if (p->mode == 2) launch_scale_weight(st, dim3(128, n_utt), p->prec, p->w, p->gx, p->ld_gx, p->gamma, p->wu, p->npad, p->kc);
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

// conv2d_kernel's four instances and conv2d_reduce_kernel through conv2d_pack and conv2d_launch (csrc/conv2d.hip.h; tests/test_hip_conv2d.py).  The extents
// are the kernel's: the load reads input time rows below offIn[n_utt] >> sh only (ti < T_u), conv2d_row forms output rows up to that of the last base position.
int stts_op_conv2d(void* stream, const stts_conv2d_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_conv2d: null argument");
  STTS_TRY(norm_op_offsets(st, "op_conv2d (input level)", p->n_utt, p->off_in_host, p->off_in_dev));
  STTS_TRY(norm_op_offsets(st, "op_conv2d (base grid)", p->n_utt, p->off_out_host, p->off_out_dev));
  const int n_utt = p->n_utt, sh = p->sh, up = p->up;
  STTS_CHECK(sh >= 0 && sh <= 16, "op_conv2d: level shift %d", sh);
  for (int u = 0; u <= n_utt; ++u)
    STTS_CHECK(p->off_in_host[u] % (1 << sh) == 0 && p->off_out_host[u] % (1 << sh) == 0, "op_conv2d: the offsets of utterance %d are no multiples of %d", u, 1 << sh);
  STTS_CHECK((up == 1 || up == 2) && p->pt >= 0 && p->pt < up && p->pf >= 0 && p->pf < up, "op_conv2d: up %d (1 or 2), pt %d, pf %d (below up)", up, p->pt, p->pf);
  STTS_CHECK(p->ntap >= 1 && p->ntap <= kConvMaxTaps, "op_conv2d: %d taps (1 .. %d)", p->ntap, kConvMaxTaps);
  STTS_CHECK(p->w_host && p->x0 && p->y && p->cout >= 1 && p->cin0 >= 1 && p->cin1 >= 0 && p->ld0 >= 1 && p->ld1 >= 0 && p->Fin >= 1 && p->F >= 1 && p->ldy >= 1 && p->chunk >= 1,
             "op_conv2d: null / empty argument");
  STTS_CHECK(p->act >= CONV_ACT_NONE && p->act <= CONV_ACT_SIGMOID && p->div != 0.f, "op_conv2d: act 0 - 2, div not 0");
  const long Tin = p->off_in_host[n_utt] >> sh, Tb = p->off_out_host[n_utt] >> sh, rows = Tb * p->F;
  const long orows = rows == 0 ? 0 : ((Tb - 1) * up + p->pt) * ((long)p->F * up) + (long)(p->F - 1) * up + p->pf + 1;  // the largest orow of conv2d_row, + 1
  STTS_CHECK(Tin * p->Fin * p->ld0 <= p->x0_elems && (uintptr_t)p->x0 % 16 == 0, "op_conv2d: x0 [%ld rows][%d] (16-byte aligned) outside its %ld elements", Tin * p->Fin, p->ld0,
             (long)p->x0_elems);
  if (p->ld1 > 0)
    STTS_CHECK(p->x1 && Tin * p->Fin * p->ld1 <= p->x1_elems && (uintptr_t)p->x1 % 16 == 0, "op_conv2d: x1 [%ld rows][%d] (16-byte aligned) outside its %ld elements", Tin * p->Fin,
               p->ld1, (long)p->x1_elems);
  STTS_CHECK(orows * p->ldy <= p->y_elems, "op_conv2d: y [%ld rows][%d] outside its %ld elements", orows, p->ldy, (long)p->y_elems);
  STTS_CHECK(!p->r || orows * p->ldy <= p->r_elems, "op_conv2d: r [%ld rows][%d] outside its %ld elements", orows, p->ldy, (long)p->r_elems);
  NormOpTemps t(st);
  stts_ctx& tmp = t.tmp;
  PackScope scope(&tmp, engine_mode(&tmp));
  const int cin = p->cin0 + p->cin1, ntap = p->ntap;
  std::vector<double> bias;
  if (p->bias_host) bias.assign(p->bias_host, p->bias_host + p->cout);
  Conv2dW w;
  STTS_TRY(conv2d_pack(&tmp, p->cout, p->npad, p->cin0, p->cin1, p->ld0, p->ld1, ntap, p->dt, p->df,
                       [&](int n, int ci, int tap) { return (double)p->w_host[((size_t)n * cin + ci) * ntap + tap]; }, p->bias_host ? &bias : nullptr, &w));
  Conv2dArgs g = conv2d_args(w);
  g.X0 = p->x0;
  g.X1 = p->ld1 > 0 ? p->x1 : nullptr;
  g.offIn = p->off_in_dev;
  g.offOut = p->off_out_dev;
  g.n_utt = n_utt;
  g.sh = sh;
  g.Fin = p->Fin;
  g.F = p->F;
  g.up = up;
  g.pt = p->pt;
  g.pf = p->pf;
  g.rows = rows;
  g.chunk = p->chunk;
  g.act = p->act;
  g.R = p->r;
  g.div = p->div;
  g.Y = p->y;
  g.ldy = p->ldy;
  const int slices = p->sliced ? ceil_div(w.K, p->chunk) : 1;
  if (slices > 1 && rows > 0) {
    STTS_HIP(hipMalloc(&g.P, (size_t)slices * rows * p->ldy * sizeof(float)));
    tmp.allocs.push_back(g.P);
  }
  STTS_TRY(conv2d_launch(st, g, p->lrelu != 0, g.P ? slices : 1));
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

// The flow-matching estimator's row kernels (csrc/cfm.hip.h) and the sequence rotary embedding (csrc/phoneme.hip.h), one launch per call through the launch
// helpers cfm_estimator itself uses (launch_* / run_small / run_rope): tests/test_hip_cfm_kernels.py.  As above: every check before any launch, every index a
// launch can form bounded by the caller's element counts, host and device offsets compared, the stream synchronised on exit.
static bool cfm_op_disjoint(const float* a, long na, const float* b, long nb) { return !a || !b || a + na <= b || b + nb <= a; }

int stts_op_cfm_elem(void* stream, const stts_cfm_elem_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p && p->kind >= 0 && p->kind <= 2, "op_cfm_elem: null argument, or kind outside 0 - 2");
  if (p->kind == 0) {  // mish_kernel in place over n float4s
    STTS_CHECK(p->x && p->n > 0 && p->n <= p->x_elems / 4 && (uintptr_t)p->x % 16 == 0, "op_cfm_elem: mish needs x (16-byte aligned) of at least 4 n = %ld elements", 4 * (long)p->n);
    launch_mish(st, p->x, (long)p->n);
  } else if (p->kind == 1) {  // swiglu_kernel: x = A [n rows][2 C] -> y [n rows][C]
    const long rows = (long)p->n, M = p->C;
    STTS_CHECK(M > 0 && M % 4 == 0, "op_cfm_elem: swiglu reads four columns at a time: C %% 4 == 0 (C = %d)", p->C);
    STTS_CHECK(p->x && p->y && rows > 0 && rows <= (1L << 40) / M && rows * 2 * M <= p->x_elems && rows * M <= p->y_elems && (uintptr_t)p->x % 16 == 0 && (uintptr_t)p->y % 16 == 0,
               "op_cfm_elem: swiglu needs x [n, 2 C] and y [n, C] (16-byte aligned) inside their buffers");
    STTS_CHECK(cfm_op_disjoint(p->x, rows * 2 * M, p->y, rows * M), "op_cfm_elem: swiglu's output overlaps its input");
    launch_swiglu(st, p->x, p->C, p->y, rows);
  } else {  // gated_residual_kernel: y = x + t * (gate_u + 1), gate = ada[u][2 C ..]
    STTS_TRY(norm_op_offsets(st, "op_cfm_elem", p->n_utt, p->seg_off_host, p->seg_off_dev));
    Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
    const long R = s.rows(), C = p->C;
    STTS_CHECK(C > 0 && C % 4 == 0, "op_cfm_elem: the gated residual reads four columns at a time: C %% 4 == 0 (C = %d)", p->C);
    STTS_CHECK((long)s.max_len() * (C / 4) < (1L << 31), "op_cfm_elem: max_len * C / 4 beyond the grid arithmetic");
    STTS_CHECK(p->x && p->t && p->ada && p->y && R * C <= p->x_elems && R * C <= p->t_elems && R * C <= p->y_elems && (long)p->n_utt * 3 * C <= p->ada_elems,
               "op_cfm_elem: the gated residual needs x, t, y [rows, C] and ada [n_utt, 3 C] inside their buffers");
    STTS_CHECK((uintptr_t)p->x % 16 == 0 && (uintptr_t)p->t % 16 == 0 && (uintptr_t)p->y % 16 == 0 && (uintptr_t)p->ada % 16 == 0, "op_cfm_elem: 16-byte alignment");
    STTS_CHECK(cfm_op_disjoint(p->x, R * C, p->y, R * C) && cfm_op_disjoint(p->t, R * C, p->y, R * C), "op_cfm_elem: the gated residual's output overlaps an input");
    if (R > 0) launch_gated_residual(st, s, p->x, p->t, p->C, p->ada, p->y);
  }
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_rms_adaln(void* stream, const stts_rms_adaln_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_rms_adaln: null argument");
  STTS_TRY(norm_op_offsets(st, "op_rms_adaln", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows(), C = p->C;
  STTS_CHECK(C > 0 && C <= 1024, "op_rms_adaln: rms_adaln_kernel keeps a row in 16 registers per lane: 0 < C <= 1024 (C = %d)", p->C);
  STTS_CHECK(p->x && p->w && p->ada && p->y, "op_rms_adaln: x, w, ada and y are required");
  STTS_CHECK(norm_op_fits(R, p->ldx, 0, p->C, p->x_elems), "op_rms_adaln: x [%ld, ldx %d] (ldx >= C = %d) outside %ld elements", R, p->ldx, p->C, (long)p->x_elems);
  STTS_CHECK(norm_op_fits(R, p->ldy, 0, p->C, p->y_elems), "op_rms_adaln: y [%ld, ldy %d] (ldy >= C = %d) outside %ld elements", R, p->ldy, p->C, (long)p->y_elems);
  STTS_CHECK(p->w_elems >= C && (long)p->n_utt * 3 * C <= p->ada_elems, "op_rms_adaln: w [C] or ada [n_utt, 3 C] shorter than that");
  STTS_CHECK((p->t == nullptr) == (p->ada_prev == nullptr), "op_rms_adaln: t and ada_prev come together");
  STTS_CHECK(!p->t || (R * C <= p->t_elems && (long)p->n_utt * 3 * C <= p->ada_prev_elems), "op_rms_adaln: t [rows, C] or ada_prev [n_utt, 3 C] shorter than that");
  STTS_CHECK(!p->xout || R * C <= p->xout_elems, "op_rms_adaln: xout [rows, C] shorter than that");
  const long xspan = R > 0 ? (R - 1) * p->ldx + C : 0, yspan = R > 0 ? (R - 1) * p->ldy + C : 0;
  STTS_CHECK((p->y == p->x && p->ldy == p->ldx) || cfm_op_disjoint(p->x, xspan, p->y, yspan), "op_rms_adaln: y may alias x row for row (the same pointer and leading dimension), not overlap it");
  STTS_CHECK(cfm_op_disjoint(p->xout, R * C, p->x, xspan) && cfm_op_disjoint(p->xout, R * C, p->y, yspan) && cfm_op_disjoint(p->xout, R * C, p->t, R * C) &&
                 cfm_op_disjoint(p->t, R * C, p->y, yspan),
             "op_rms_adaln: xout or t overlaps another tensor");
  if (R > 0) launch_rms_adaln(st, s, p->x, p->ldx, p->C, p->w, p->ada, p->y, p->ldy, p->t, p->ada_prev, p->xout);
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_rope(void* stream, const stts_rope_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p && (p->kind == 0 || p->kind == 1), "op_rope: null argument, or kind outside 0 (axial) / 1 (sequence)");
  STTS_TRY(norm_op_offsets(st, "op_rope", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  const int heads = p->heads, kc = p->kc, d = p->d;
  STTS_CHECK(heads > 0 && kc > 0 && d > 0 && d % 2 == 0 && d <= kc, "op_rope: the rotated features come in pairs inside a head: d even, 0 < d <= kc (d = %d, kc = %d)", d, kc);
  STTS_CHECK(p->kind != 0 || (kc == d && p->freq && (long)heads * (d / 2) <= p->freq_elems), "op_rope: the axial form turns whole heads (kc == d) by freq [heads, d / 2]");
  STTS_CHECK(p->kind != 1 || d == (int)(kc * 0.5), "op_rope: the sequence form turns the first int(kc / 2) features of a head (d = %d, kc = %d)", d, kc);
  const long width = (long)heads * kc;
  STTS_CHECK(p->col0 >= 0 && p->col0 + width <= p->ldx, "op_rope: column block [%d, %ld) outside ldx %d", p->col0, p->col0 + width, p->ldx);
  STTS_CHECK(p->col1 == -1 || (p->col1 >= 0 && p->col1 + width <= p->ldx && (p->col1 >= p->col0 + width || p->col0 >= p->col1 + width)),
             "op_rope: second column block at %d outside ldx %d, or overlapping the first (-1: none)", p->col1, p->ldx);
  STTS_CHECK(p->x && (R == 0 || (R - 1) * (long)p->ldx + std::max(p->col0, p->col1) + width <= p->x_elems), "op_rope: x [%ld, ldx %d] outside %ld elements", R, p->ldx, (long)p->x_elems);
  STTS_CHECK((long)s.max_len() * heads * (d / 2) * 2 < (1L << 31), "op_rope: max_len * heads * d beyond the grid arithmetic");
  if (R > 0) {
    if (p->kind == 0) launch_axial_rope(st, s, p->x, p->ldx, p->col0, p->col1, heads, d, p->freq);
    else run_rope(st, s, p->x, p->ldx, p->col0, heads, kc, p->col1);
  }
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_cfm_small(void* stream, const stts_cfm_small_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p && p->kind >= 0 && p->kind <= 2, "op_cfm_small: null argument, or kind outside 0 - 2");
  const long rows = p->n_rows, N = p->N, K = p->K;
  STTS_CHECK(rows > 0 && N > 0 && p->x && p->w && p->y && rows * N < (1L << 31), "op_cfm_small: null / empty argument");
  if (p->kind == 0) {  // small_linear_kernel: y [rows, N] = act(x [rows, K] w[N, K]^T + b)
    STTS_CHECK(K > 0 && (p->act == 0 || p->act == 1), "op_cfm_small: linear needs K > 0 and act 0 (none) or 1 (Mish)");
    STTS_CHECK(norm_op_fits(rows, p->ldx, 0, p->K, p->x_elems) && norm_op_fits(rows, p->ldy, 0, p->N, p->y_elems), "op_cfm_small: x [rows, ldx >= K] or y [rows, ldy >= N] outside its buffer");
    STTS_CHECK(N * K <= p->w_elems && (!p->b || N <= p->b_elems), "op_cfm_small: w [N, K] or b [N] shorter than that");
    SmallLinear w;
    w.W = const_cast<float*>(p->w);
    w.b = const_cast<float*>(p->b);
    w.N = p->N;
    w.K = p->K;
    STTS_TRY(run_small(st, w, p->x, p->ldx, p->act, p->y, p->ldy, p->n_rows));
  } else if (p->kind == 1) {  // small_layernorm_kernel over N channels: w = gamma, b = beta
    STTS_CHECK(p->b && N <= p->w_elems && N <= p->b_elems, "op_cfm_small: layernorm needs gamma (w) and beta (b) of N elements");
    STTS_CHECK(norm_op_fits(rows, p->ldx, 0, p->N, p->x_elems) && norm_op_fits(rows, p->ldy, 0, p->N, p->y_elems), "op_cfm_small: x [rows, ldx >= N] or y [rows, ldy >= N] outside its buffer");
    launch_small_layernorm(st, p->x, p->ldx, p->N, p->w, p->b, p->y, p->ldy, p->n_rows);
  } else {  // cfm_time_embed_kernel: x = t [rows], w = freqs [N = half] -> y [rows, ldy] = cos | sin
    STTS_CHECK(rows <= p->x_elems && N <= p->w_elems, "op_cfm_small: time embedding needs t (x) [rows] and freqs (w) [N]");
    STTS_CHECK(norm_op_fits(rows, p->ldy, 0, 2 * p->N, p->y_elems), "op_cfm_small: y [rows, ldy >= 2 N] outside its buffer");
    launch_time_embed(st, p->x, p->w, p->N, p->y, p->ldy, p->n_rows);
  }
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_cfm_source(void* stream, const stts_cfm_source_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_cfm_source: null argument");
  STTS_TRY(norm_op_offsets(st, "op_cfm_source (frames)", p->n_utt, p->seg_off_host, p->seg_off_dev));
  STTS_TRY(norm_op_offsets(st, "op_cfm_source (curves)", p->n_utt, p->curve_off_host, p->curve_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows(), Lc = p->curve_off_host[p->n_utt];
  STTS_CHECK(p->ldh == 32, "op_cfm_source: the source rows are 32 columns wide (ldh = %d)", p->ldh);
  for (int u = 0; u < p->n_utt; ++u)
    STTS_CHECK(p->seg_off_host[u + 1] == p->seg_off_host[u] || p->curve_off_host[u + 1] > p->curve_off_host[u], "op_cfm_source: utterance %d has frames but a curve of zero points", u);
  STTS_CHECK(p->f0 && p->ncurve && p->t && p->noise && p->har, "op_cfm_source: null tensor");
  STTS_CHECK(Lc <= p->f0_elems && Lc <= p->ncurve_elems && p->n_utt <= p->t_elems && R <= p->noise_elems && R * 32 <= p->har_elems,
             "op_cfm_source: f0 / ncurve [%ld], t [%d], noise [%ld] or har [%ld, 32] shorter than that", Lc, p->n_utt, R, R);
  launch_cfm_source(st, s, p->f0, p->ncurve, p->curve_off_dev, p->t, p->noise, p->merge_w, p->har, p->ldh);
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

// The small kernels between the stages (index maps, gathers, broadcasts, style projection, decoder front), one launch per call through the launch_* / run_style
// functions of model.hip.h that the stages call: tests/test_hip_glue_kernels.py.  As above: every check before any launch.
int stts_op_glue(void* stream, const stts_glue_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p && p->kind >= 0 && p->kind <= 6, "op_glue: null argument, or kind outside 0 - 6");
  const int kind = p->kind;
  long R = 0;
  Seg s{};
  if (kind != 1 && kind != 2) {
    STTS_TRY(norm_op_offsets(st, "op_glue", p->n_utt, p->seg_off_host, p->seg_off_dev));
    s = Seg{p->n_utt, p->seg_off_host, p->seg_off_dev};
    R = s.rows();
  }
  const int C = p->C;
  if (kind == 0) {  // decoder_front_kernel
    const int cc = p->c_hidden + p->c_res;
    STTS_CHECK(p->x && p->x2 && p->x3 && p->y && p->y2 && p->y3, "op_glue: decoder front needs x, x2, x3, y, y2, y3");
    STTS_CHECK(C > 0 && C % 4 == 0 && p->ldx % 4 == 0 && p->ldy % 4 == 0 && p->ld2 % 4 == 0 && cc % 4 == 0 && p->c_hidden >= 0 && p->c_res >= 0,
               "op_glue: decoder front moves four columns at a time: C, ldx, ldy, ld2 and c_hidden + c_res are multiples of 4");
    STTS_CHECK(p->ldy >= C + 4 && p->ld2 >= cc + 4, "op_glue: decoder front needs ldy >= C + 4 and ld2 >= c_hidden + c_res + 4 (the F0 / N quad)");
    STTS_CHECK(norm_op_fits(R, p->ldx, 0, C, p->x_elems) && R <= p->x2_elems && R <= p->x3_elems && norm_op_fits(R, p->ldy, 0, p->ldy, p->y_elems) &&
                   norm_op_fits(R, p->ld2, 0, p->ld2, p->y2_elems) && norm_op_fits(R, p->ld2, 0, p->ld2, p->y3_elems),
               "op_glue: decoder front: a tensor is shorter than its rows");
    STTS_CHECK((uintptr_t)p->x % 16 == 0 && (uintptr_t)p->y % 16 == 0 && (uintptr_t)p->y2 % 16 == 0 && (uintptr_t)p->y3 % 16 == 0, "op_glue: 16-byte alignment");
    FrontArgs fa;
    fa.asr = p->x; fa.ld_asr = p->ldx; fa.pitch = p->x2; fa.energy = p->x3;
    for (int i = 0; i < 3; ++i) { fa.wf[i] = p->wf[i]; fa.wn[i] = p->wn[i]; }
    fa.bf = p->bf; fa.bn = p->bn;
    fa.enc_in = p->y; fa.ld_enc = p->ldy; fa.xa = p->y2; fa.xb = p->y3; fa.ld_x = p->ld2;
    fa.c_asr = C; fa.c_hidden = p->c_hidden; fa.c_res = p->c_res;
    if (R > 0) launch_decoder_front(st, s, fa);
  } else if (kind == 1) {  // run_style: the table is built and padded as the stages' tables are (StyleTable / upload_table)
    const int n_utt = p->n_utt, J = p->J, K = p->K;
    STTS_CHECK(n_utt > 0 && J > 0 && K > 0 && p->w_host && p->b_host && p->x && p->y, "op_glue: run_style needs n_utt, J, K, w_host, b_host, x, y");
    STTS_CHECK(p->ldy == round_up(J, 4) && (long)n_utt * K <= p->x_elems && (long)n_utt * p->ldy <= p->y_elems && (uintptr_t)p->x % 16 == 0,
               "op_glue: run_style needs x [n_utt, K] (16-byte aligned) and y [n_utt, ldy = J rounded up to 4]");
    NormOpTemps t(st);
    PackScope scope(&t.tmp, engine_mode(&t.tmp));
    StyleTable tab;
    tab.K = K;
    tab.J = J;
    tab.hW.assign(p->w_host, p->w_host + (size_t)J * K);
    tab.hb.assign(p->b_host, p->b_host + J);
    STTS_TRY(upload_table(&t.tmp, &tab));
    STTS_TRY(run_style(st, tab, p->x, n_utt, p->y));
    STTS_HIP(hipStreamSynchronize(st));
    return 0;
  } else if (kind == 2) {  // embed_kernel
    const long rows = p->n_rows;
    STTS_CHECK(rows > 0 && C > 0 && C % 4 == 0 && p->J > 0 && p->ldy % 4 == 0 && p->x && p->tokens && p->y && p->err, "op_glue: embed needs n_rows, C %% 4 == 0, J (vocabulary), ldy %% 4 == 0, x, tokens, y, err");
    STTS_CHECK((long)p->J * C <= p->x_elems && rows <= p->tokens_elems && norm_op_fits(rows, p->ldy, 0, C, p->y_elems) && rows * C < (1L << 31),
               "op_glue: embed: x [J, C], tokens [n_rows] or y [n_rows, ldy >= C] shorter than that");
    STTS_CHECK((uintptr_t)p->x % 16 == 0 && (uintptr_t)p->y % 16 == 0, "op_glue: 16-byte alignment");
    launch_embed(st, reinterpret_cast<const long*>(p->tokens), p->x, C, p->J, p->y, p->ldy, rows, p->err);
  } else if (kind == 3) {  // mean_rows_kernel
    STTS_CHECK(C > 0 && p->x && p->y && norm_op_fits(R, p->ldx, 0, C, p->x_elems) && norm_op_fits(p->n_utt, p->ldy, 0, C, p->y_elems),
               "op_glue: mean_rows needs x [rows, ldx >= C] and y [n_utt, ldy >= C]");
    launch_mean_rows(st, s, p->x, p->ldx, C, p->y, p->ldy);
  } else if (kind == 4) {  // broadcast_style_kernel
    STTS_CHECK(C > 0 && p->x && p->y && norm_op_fits(p->n_utt, p->ldx, 0, C, p->x_elems) && norm_op_fits(R, p->ldy, p->col0, C, p->y_elems),
               "op_glue: broadcast_style needs x [n_utt, ldx >= C] and y [rows, ldy >= col0 + C]");
    STTS_CHECK((long)s.max_len() * C < (1L << 31), "op_glue: max_len * C beyond the grid arithmetic");
    if (R > 0) launch_broadcast_style(st, s, p->x, p->ldx, C, p->y, p->ldy, p->col0);
  } else if (kind == 5) {  // row_utt_kernel
    STTS_CHECK(p->iy && R <= p->iy_elems && s.max_len() > 0, "op_glue: row_utt needs iy [rows] and at least one row");
    launch_row_utt(st, s, p->iy);
  } else {  // frame_token_map_kernel + local_token_kernel, as pitch_energy_forward chains them
    STTS_TRY(norm_op_offsets(st, "op_glue (tokens)", p->n_utt, p->tok_off_host, p->tok_off_dev));
    Seg sp{p->n_utt, p->tok_off_host, p->tok_off_dev};
    STTS_CHECK(p->dur && p->iy && p->iy2 && p->rep >= 1 && sp.rows() <= p->dur_elems && R <= p->iy_elems && R <= p->iy2_elems && s.max_len() > 0,
               "op_glue: token map needs dur [tokens], iy / iy2 [frames], rep >= 1 and at least one frame");
    for (int u = 0; u < p->n_utt; ++u)
      STTS_CHECK(p->tok_off_host[u + 1] > p->tok_off_host[u] || p->seg_off_host[u + 1] == p->seg_off_host[u], "op_glue: utterance %d has frames but no token", u);
    launch_frame_token_map(st, p->n_utt, p->dur, sp.dev, s.dev, p->rep, p->iy);
    launch_local_token(st, s, sp, p->iy, p->iy2);
  }
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

int stts_op_chan_conv(void* stream, const stts_chan_conv_args* p) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  STTS_CHECK(p, "op_chan_conv: null argument");
  STTS_TRY(norm_op_offsets(st, "op_chan_conv", p->n_utt, p->seg_off_host, p->seg_off_dev));
  Seg s{p->n_utt, p->seg_off_host, p->seg_off_dev};
  const long R = s.rows();
  const int C = p->C;
  STTS_CHECK(p->prec16 == 0 || p->prec16 == PREC_BF16 || p->prec16 == PREC_F16, "op_chan_conv: prec16 is 0, STTS_PREC_BF16 or _F16");
  STTS_CHECK(p->nsets == 1 || p->nsets == 2, "op_chan_conv: one or two sets");
  STTS_CHECK(R > 0 && C > 0 && p->ntaps >= 1 && p->ycol >= 0 && p->ycol < p->ldy, "op_chan_conv: no rows, or C / ntaps / ycol out of range");
  STTS_CHECK((long)s.max_len() * p->ldx < (1L << 28), "op_chan_conv: max_len * ldx beyond the kernel's 32-bit byte offsets");
  auto set_ok = [&](const void* x, long xe, const float* w, long we, const float* y, long ye) {
    return x && w && y && norm_op_fits(R, p->ldx, 0, C, xe) && (long)p->ntaps * C <= we && (R - 1) * (long)p->ldy + p->ycol + 1 <= ye && (uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0;
  };
  STTS_CHECK(set_ok(p->x0, p->x0_elems, p->w0, p->w0_elems, p->y0, p->y0_elems), "op_chan_conv: set 0: x [rows, ldx >= C], w [ntaps, C] (16-byte aligned) or y [rows, ldy] outside its buffer");
  STTS_CHECK(p->nsets == 1 || set_ok(p->x1, p->x1_elems, p->w1, p->w1_elems, p->y1, p->y1_elems), "op_chan_conv: set 1: x, w or y outside its buffer");
  const ChanConvSet s0{reinterpret_cast<const float*>(p->x0), p->w0, p->bias0, p->y0};
  const ChanConvSet s1 = p->nsets == 2 ? ChanConvSet{reinterpret_cast<const float*>(p->x1), p->w1, p->bias1, p->y1} : s0;
  STTS_TRY(launch_single_channel_conv(st, s, p->prec16, p->nsets, s0, s1, p->ldx, C, p->ntaps, p->ldy, p->ycol));
  STTS_HIP(hipGetLastError());
  STTS_HIP(hipStreamSynchronize(st));
  return 0;
  API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ kernel microbench
// Times `iters` back-to-back launches of conv_gemm_f32 on synthetic data (tuning aid for tools/gemm_bench.py).
extern "C" int stts_bench_gemm(void* stream, int n_utt, int rows_per_utt, int cin, int cout, int k, int tile, int iters, double* avg_ms, int tune) {
  API_BEGIN
  hipStream_t st = (hipStream_t)stream;
  const long R = (long)n_utt * rows_per_utt;
  const int kc = round_up(cin, 32), npad = round_up(cout, 128), ldy = round_up(cout, 32);
  float *X, *W, *Y, *B;
  int* so;
  STTS_HIP(hipMalloc(&X, R * kc * sizeof(float)));
  STTS_HIP(hipMalloc(&W, (size_t)npad * k * kc * sizeof(float)));
  STTS_HIP(hipMalloc(&Y, R * ldy * sizeof(float)));
  STTS_HIP(hipMalloc(&B, npad * sizeof(float)));
  STTS_HIP(hipMalloc(&so, (n_utt + 1) * sizeof(int)));
  std::vector<int> h(n_utt + 1);
  for (int i = 0; i <= n_utt; ++i) h[i] = i * rows_per_utt;
  STTS_HIP(hipMemcpy(so, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  // pseudo-random fill (zeros would flatter the clock: guide §5.4 rule 25)
  std::vector<float> hw((size_t)npad * k * kc);
  {
    std::vector<float> t((size_t)std::max<long>(R * kc, (long)npad * k * kc));
    uint32_t s = 12345;
    for (auto& v : t) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xFFFF) / 32768.0f - 1.0f; }
    STTS_HIP(hipMemcpy(X, t.data(), R * kc * sizeof(float), hipMemcpyHostToDevice));
    STTS_HIP(hipMemcpy(W, t.data(), (size_t)npad * k * kc * sizeof(float), hipMemcpyHostToDevice));
    std::copy(t.begin(), t.begin() + hw.size(), hw.begin());
    STTS_HIP(hipMemset(B, 0, npad * sizeof(float)));
  }
  PackedConv pc;
  pc.W = W; pc.bias = B; pc.npad = npad; pc.N = cout; pc.kc = kc; pc.ntaps = k; pc.cin_real = cin; pc.rows_real = cout;
  unsigned short* W16 = nullptr;
  if (tune & 384) {  // bit 7: bf16 operands, bit 8: fp16 operands
    std::vector<unsigned short> h16((size_t)npad * k * kc);
    uint32_t s2 = 777;
    for (auto& v : h16) { s2 = s2 * 1664525u + 1013904223u; v = f32_to_bf16(((s2 >> 8) & 0xFFFF) / 32768.0f - 1.0f); }
    STTS_HIP(hipMalloc(&W16, h16.size() * 2));
    STTS_HIP(hipMemcpy(W16, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
    pc.W16 = W16;
    pc.prec = (tune & 128) ? PREC_BF16 : PREC_F16;
  }
  if (tune & 2048) {  // bit 11: split-fp32 contraction (the three bf16 planes of W)
    std::vector<unsigned short> h3(hw.size() * 3);
    for (size_t i = 0; i < hw.size(); ++i) split3_host(hw[i], &h3[i], &h3[hw.size() + i], &h3[2 * hw.size() + i]);
    STTS_HIP(hipMalloc(&W16, h3.size() * 2));
    STTS_HIP(hipMemcpy(W16, h3.data(), h3.size() * 2, hipMemcpyHostToDevice));
    pc.W16 = W16;
    pc.w16_plane = (long)hw.size();
  }
  Seg s{n_utt, h.data(), so};
  GemmArgs a = gemm_args(s);
  set_seg(a, 0, X, kc, 0, pc);
  a.N = cout; a.bias = B; a.Y = Y; a.ldy = ldy; a.tune = tune & 63;
  if ((tune & 2048) && !x3_enabled()) return stts::fail("split-fp32 contractions are switched off (STTS_NO_X3)");
  unsigned short* X16 = nullptr;
  if ((tune & 1024) && (tune & 384)) {  // bit 10: 16-bit activation rows (X rounded once, outside the timed launches)
    STTS_HIP(hipMalloc(&X16, R * kc * sizeof(unsigned short)));
    launch_cast_rows(st, pc.prec, X, kc, kc, X16, kc, R);
    a.seg[0].X = reinterpret_cast<const float*>(X16);
    a.x16 = 1;
  }
  if ((tune & 4096) && (tune & 2048)) {  // bit 12: pre-split activation planes (split once, outside the timed launches)
    STTS_HIP(hipMalloc(&X16, 3 * R * kc * sizeof(unsigned short)));
    launch_split_rows(st, X, kc, kc, X16, kc, R * kc, R);
    a.seg[0].X = reinterpret_cast<const float*>(X16);
    a.seg[0].x_plane = R * kc;
    a.x16 = 1;
  }
  long long* dbg = nullptr;
  const size_t dbg_n = 8 * 16384;
  if (tune & 64) { STTS_HIP(hipMalloc(&dbg, dbg_n * 8)); STTS_HIP(hipMemset(dbg, 0, dbg_n * 8)); }
  a.dbg = dbg;
  hipEvent_t e0, e1;
  STTS_HIP(hipEventCreate(&e0));
  STTS_HIP(hipEventCreate(&e1));
  if (tune & 512) {  // the Winograd F(6, k) form of the same conv, transforms included (k = 3 or 7)
    stts_ctx tmp;
    HostTensor hw;
    hw.shape = {cout, cin, k};
    hw.data.resize((size_t)cout * cin * k);
    uint32_t s3 = 4242;
    for (auto& v : hw.data) { s3 = s3 * 1664525u + 1013904223u; v = (((s3 >> 8) & 0xFFFF) / 32768.0f - 1.0f) * 0.05f; }
    WinoConv wc;
    PackScope scope(&tmp, engine_mode(&tmp));
    STTS_TRY(pack_winograd(&tmp, hw, nullptr, 0, cin, cout, &wc));
    float* scratch = nullptr;
    STTS_HIP(hipMalloc(&scratch, wino_scratch_floats(s, wc) * sizeof(float)));
    WinoScratch wz;
    wz.p = scratch;
    for (int i = 0; i < 2; ++i) STTS_TRY(run_winograd(st, s, X, kc, wc, Y, ldy, 0, nullptr, 0, 1.0f, wz));
    STTS_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) STTS_TRY(run_winograd(st, s, X, kc, wc, Y, ldy, 0, nullptr, 0, 1.0f, wz));
    STTS_HIP(hipEventRecord(e1, st));
    STTS_HIP(hipEventSynchronize(e1));
    float msw = 0;
    STTS_HIP(hipEventElapsedTime(&msw, e0, e1));
    *avg_ms = msw / iters;
    (void)hipFree(scratch);
    for (void* p : tmp.allocs) (void)hipFree(p);
    (void)hipFree(X); (void)hipFree(W); (void)hipFree(Y); (void)hipFree(B); (void)hipFree(so);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
  }
  for (int i = 0; i < 2; ++i) STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, npad, n_utt, rows_per_utt, tile));
  STTS_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) STTS_TRY(launch_conv_gemm(st, a, EPI_STORE, npad, n_utt, rows_per_utt, tile));
  STTS_HIP(hipEventRecord(e1, st));
  STTS_HIP(hipEventSynchronize(e1));
  float ms = 0;
  STTS_HIP(hipEventElapsedTime(&ms, e0, e1));
  *avg_ms = ms / iters;
  if (dbg) {
    std::vector<long long> hdb(dbg_n);
    STTS_HIP(hipMemcpy(hdb.data(), dbg, dbg_n * 8, hipMemcpyDeviceToHost));
    // per-block records of the LAST launch: [t0, t1, t2, t3, iters, hw_id, xcc_id, -]
    long long tmin = -1, tmax = 0;
    std::map<long long, std::vector<std::pair<long long, long long>>> cu;
    int nb = 0;
    double pro = 0, loop = 0, epi = 0;
    for (size_t b = 0; b < dbg_n / 8; ++b) {
      const long long* r = &hdb[8 * b];
      if (!r[0]) continue;
      ++nb;
      if (tmin < 0 || r[0] < tmin) tmin = r[0];
      if (r[3] > tmax) tmax = r[3];
      pro += r[1] - r[0]; loop += r[2] - r[1]; epi += r[3] - r[2];
      const long long hw = r[5], key = ((r[6] & 15) << 16) | (hw & 0xFF00);  // xcc | se, sh, cu
      cu[key].push_back({r[0], r[3]});
    }
    int hist[8] = {0};
    long long worst = 0;
    for (auto& kv : cu) {
      hist[std::min<size_t>(kv.second.size(), 7)]++;
      long long e = 0;
      for (auto& p : kv.second) e = std::max(e, p.second);
      worst = std::max(worst, e - tmin);
    }
    fprintf(stderr, "  blocks %d on %zu CUs; blocks/CU histogram 1:%d 2:%d 3:%d 4:%d 5+:%d; span %.1f us; avg prologue %.1f loop %.1f epilogue %.1f us\n", nb,
            cu.size(), hist[1], hist[2], hist[3], hist[4], hist[5] + hist[6] + hist[7], (tmax - tmin) * 0.01, pro / nb * 0.01, loop / nb * 0.01,
            epi / nb * 0.01);
    // start-time spread and per-block duration spread
    long long smax = 0, dmin = 1LL << 60, dmax = 0;
    for (size_t b = 0; b < dbg_n / 8; ++b) {
      const long long* r = &hdb[8 * b];
      if (!r[0]) continue;
      smax = std::max(smax, r[0] - tmin);
      dmin = std::min(dmin, r[3] - r[0]);
      dmax = std::max(dmax, r[3] - r[0]);
    }
    fprintf(stderr, "  latest start +%.1f us; block duration min %.1f max %.1f us\n", smax * 0.01, dmin * 0.01, dmax * 0.01);
    double xd[8] = {0}, xc[8] = {0}; int xn[8] = {0};
    for (size_t b = 0; b < dbg_n / 8; ++b) {
      const long long* r = &hdb[8 * b];
      if (!r[0]) continue;
      const int x = r[6] & 7;
      xd[x] += (r[3] - r[0]) * 0.01; xc[x] += (double)r[7] / ((r[3] - r[0]) * 0.01); xn[x]++;
    }
    {
      std::vector<double> du;
      for (size_t b = 0; b < dbg_n / 8; ++b) if (hdb[8 * b]) du.push_back((hdb[8 * b + 3] - hdb[8 * b]) * 0.01);
      std::sort(du.begin(), du.end());
      fprintf(stderr, "  duration percentiles us: p5 %.0f p25 %.0f p50 %.0f p75 %.0f p95 %.0f max %.0f\n", du[du.size() / 20], du[du.size() / 4], du[du.size() / 2],
              du[du.size() * 3 / 4], du[du.size() * 19 / 20], du.back());
      // by original linear block id modulo 64 (8 XCDs x 8): shows placement patterns
      const int gx = npad / 128;
      double byd[16] = {0}; int byn[16] = {0};
      for (size_t b = 0; b < dbg_n / 8; ++b) {
        if (!hdb[8 * b]) continue;
        const int cuid = (hdb[8 * b + 5] >> 8) & 15;
        byd[cuid] += (hdb[8 * b + 3] - hdb[8 * b]) * 0.01; byn[cuid]++;
      }
      (void)gx;
      fprintf(stderr, "  avg by cu_id:");
      for (int i = 0; i < 16; ++i) if (byn[i]) fprintf(stderr, " %d:%.0f(%d)", i, byd[i] / byn[i], byn[i]);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "  per XCC avg block us / shader MHz:");
    for (int x = 0; x < 8; ++x) if (xn[x]) fprintf(stderr, " %d:%.0f/%.0f", x, xd[x] / xn[x], xc[x] / xn[x]);
    fprintf(stderr, "\n");
    (void)hipFree(dbg);
  }
  (void)hipFree(X); (void)hipFree(W); (void)hipFree(Y); (void)hipFree(B); (void)hipFree(so);
  if (W16) (void)hipFree(W16);
  if (X16) (void)hipFree(X16);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return 0;
  API_END
}


"""int64 / float64 restatements of the small operations between the stages (frame offsets, frame -> token maps, duration decoding, alignment matrix, embedding,
style broadcast / mean / projection, x4 upsampling, the decoder's front end, the one-channel conv), the inputs tests/test_hip_glue_kernels.py runs the kernels on,
and one comparison function per kernel.  tests/test_glue64_cpu.py checks the references against oracle/stylish_oracle.py and shows, with small fp32 / int32 models
of the kernels and mutated copies of them, that these shapes and bounds tell a correct kernel from a subtly wrong one.  Test infrastructure, modelled on cfm64.py.

Written from the operations' definitions (the reference lines the kernels' comments cite), not from the kernels:
  frame offsets        T_u = sum of utterance u's durations (negative entries count 0), truncated to the caller's capacity; offsets = running sums, x4 at the vocoder rate
  frame -> token map   frame f of utterance u belongs to the token whose run of rep * dur frames contains f (alignment.repeat_interleave(rep), enc @ alignment);
                       frames past the last run take the last token, frames past the utterance's own frame count do not exist
  duration decode      DurationProcessor.prediction_to_duration: hard = table[argmax] (first maximum), soft = max(round_half_even(softmax . table), 1); hard if hard < 7
  alignment            DurationProcessor.duration_to_alignment: 0 / 1 [P, T]
  upsample             nn.Upsample(scale_factor=4, mode="linear", align_corners=False)
  decoder front        F0 = conv1d(1 -> 1, k 3, zero padding)(pitch), N likewise on energy; [asr | F0 | N | 0 ..]
  one-channel conv     F.conv1d to a single output channel, zero padding (k - 1) / 2, per utterance

Bounds of the arithmetic kernels: a sum of n products in fp32, in any order, fused or not, is within n u sum|a_k b_k| of the exact sum (u = 2^-24), and its rounding to the
output (after the bias) adds u |result|:  |got - ref| <= (n + 4) u sum|a b| + u |ref|.  The comparison functions return the largest error as a fraction of that bound.
"""
import functools

import numpy as np

from stylish_tts_amd import synth

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
U = 2.0 ** -24
SENT32 = 0x7FC0BEEF  # quiet NaN: the canary of every float output buffer
SENTI = -0x41104111  # the canary of every int output buffer
CLASS_TO_DUR = np.array([1, 2, 3, 4, 5, 6, 7, 9, 12, 15, 18, 22, 27, 32, 38, 46], F64)


def offsets(lengths):
    o = np.zeros(len(lengths) + 1, I64)
    o[1:] = np.cumsum(lengths)
    return o


def ints(name, n, lo, hi):
    """n integers in [lo, hi], from the hash generator."""
    return np.minimum(lo + np.floor(synth.uniform(name, (n,)).astype(F64) * (hi - lo + 1)), hi).astype(I64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def sent(shape):
    return np.full(shape, SENT32, np.uint32).view(F32)


def ratio(got, ref, bound):
    """Largest |got - ref| / bound; where the bound is 0 the values must be equal."""
    err = np.abs(np.asarray(got, F64) - ref)
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def dot_bound(n, sumabs, ref):
    return (n + 4) * U * sumabs + U * np.abs(ref)


def round_to(a, prec):
    """fp32 values rounded (nearest even) to the row type: 0 fp32, 1 bf16, 2 f16."""
    a = np.ascontiguousarray(a, F32)
    if prec == 1:
        u = a.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(F32)
    if prec == 2:
        return a.astype(np.float16).astype(F32)
    return a


# ------------------------------------------------------------------------------------------------ frame offsets
OFFSETS_N_UTT = (1, 16, 17, 33, 64, 100)
TOKEN_COUNTS = (1, 63, 64, 65, 129, 510)


def offsets_ref(dur, tok_off, caps):
    need = np.array([np.maximum(dur[tok_off[u]:tok_off[u + 1]].astype(I64), 0).sum() for u in range(len(caps))], I64)
    off_T = offsets(np.minimum(need, np.asarray(caps, I64)))
    return need, off_T, 4 * off_T


@functools.lru_cache(maxsize=None)
def offsets_case(n_utt):
    """Token counts from TOKEN_COUNTS (510 first, so one utterance alone walks its tokens 8 times), durations 0 .. 46 with negative entries; three capacity
    layouts: exact (= need), over (every third utterance at half its need, every fifth from the second at 0) and zero (all 0)."""
    pick = ints(f"glue.offsets.pick.{n_utt}", n_utt, 0, 5)
    P = [TOKEN_COUNTS[(5 - u) % 6] if u < 6 else TOKEN_COUNTS[pick[u]] for u in range(n_utt)]
    tok_off = offsets(P)
    dur = ints(f"glue.offsets.dur.{n_utt}", int(tok_off[-1]), 0, 46)
    dur[::37] = -3
    dur[5::101] = -46
    need = offsets_ref(dur, tok_off, np.zeros(n_utt, I64))[0]
    over = need.copy()
    over[::3] //= 2
    over[1::5] = 0
    caps = {"exact": need, "over": over, "zero": np.zeros(n_utt, I64)}
    return dict(n_utt=n_utt, P=P, tok_off=tok_off, dur=dur.astype(I32), caps=caps, ref={k: offsets_ref(dur, tok_off, c) for k, c in caps.items()})


def offsets_equal(ref, need, off_T, off_T4):
    return all(np.array_equal(np.asarray(g, I64), r) for g, r in zip((need, off_T, off_T4), ref))


def offsets_model(dur, tok_off, caps, mutant=None):
    """int32 model of frame_offsets_kernel.  Mutants: tok64 (an utterance's sum stops after 64 tokens), utt16 (only 16 utterances are summed), noclamp."""
    n = len(caps)
    need = np.zeros(n, I32)
    for u in range(n if mutant != "utt16" else min(n, 16)):
        hi = tok_off[u + 1] if mutant != "tok64" else min(tok_off[u + 1], tok_off[u] + 64)
        need[u] = np.maximum(dur[tok_off[u]:hi], 0).sum(dtype=I32)
    take = need if mutant == "noclamp" else np.minimum(need, np.asarray(caps, I32))
    off = np.zeros(n + 1, I32)
    off[1:] = np.cumsum(take, dtype=I32)
    return need, off, (4 * off).astype(I32)


# ------------------------------------------------------------------------------------------------ frame -> token map, length regulator, token-local index
REGULATE_CASES = {  # name: (tokens per utterance, rep, C)
    "rep4_c4": ((1, 255, 256, 257, 511, 512, 513, 1500), 4, 4),
    "rep1_c128_17utt": ((1, 255, 256, 257, 511, 512, 513, 1500, 1, 1, 2, 3, 1, 255, 1, 257, 1), 1, 128),
    "rep4_c132": ((513, 1, 256, 1500), 4, 132),
    "rep1_c4": ((513, 1, 256, 1500), 1, 4),
}


def token_map_ref(dur, tok_off, frm_off, rep):
    """src[f] = packed token row of frame f, for the frames of every utterance's own range [frm_off[u], frm_off[u + 1])."""
    src = np.zeros(int(frm_off[-1]), I64)
    for u in range(len(tok_off) - 1):
        t0, P = int(tok_off[u]), int(tok_off[u + 1] - tok_off[u])
        nf = int(frm_off[u + 1] - frm_off[u])
        seq = np.repeat(np.arange(P, dtype=I64), rep * np.maximum(dur[t0:t0 + P].astype(I64), 0))
        if len(seq) < nf:
            seq = np.concatenate([seq, np.full(nf - len(seq), max(P - 1, 0), I64)])
        src[frm_off[u]:frm_off[u + 1]] = t0 + seq[:nf]
    return src


@functools.lru_cache(maxsize=None)
def regulate_case(name):
    """Durations 0 .. 46, most of them small (so the frame counts stay small), 46 then 0 on both sides of every 256-token boundary.  Frame offsets per utterance in
    turn: consistent, 7 frames short (truncation inside a token), 300 frames long (the last token fills the tail).  n_frames = the frame count + 5 (a capacity)."""
    P, rep, C = REGULATE_CASES[name]
    tok_off = offsets(P)
    n_tok = int(tok_off[-1])
    dur = np.floor(synth.uniform(f"glue.regulate.dur.{name}", (n_tok,)).astype(F64) ** 8 * 47).astype(I64)
    for u, p in enumerate(P):
        for b in range(255, p, 256):
            dur[tok_off[u] + b] = 46
            if b + 1 < p:
                dur[tok_off[u] + b + 1] = 0
        if p > 3:
            dur[tok_off[u]] = 0
            dur[tok_off[u + 1] - 1] = 46
    total = np.array([rep * dur[tok_off[u]:tok_off[u + 1]].sum() for u in range(len(P))], I64)
    nf = np.array([t if u % 3 == 0 else max(t - 7, 0) if u % 3 == 1 else t + 300 for u, t in enumerate(total)], I64)
    frm_off = offsets(nf)
    src = token_map_ref(dur, tok_off, frm_off, rep)
    enc = synth.normal(f"glue.regulate.enc.{name}", (n_tok, C + 4))
    utt = np.repeat(np.arange(len(P)), nf)
    return dict(P=P, rep=rep, C=C, tok_off=tok_off, frm_off=frm_off, dur=dur.astype(I32), total=total, enc=enc, src=src, centre=src - tok_off[utt], n=int(frm_off[-1]),
                n_frames=int(frm_off[-1]) + 5)


def token_map_equal(case, src_row):
    """src_row: the whole int buffer; everything past the frames must still hold the canary."""
    n = case["n"]
    return bool(np.array_equal(np.asarray(src_row[:n], I64), case["src"]) and (np.asarray(src_row[n:]) == SENTI).all())


def local_token_equal(case, centre):
    n = case["n"]
    return bool(np.array_equal(np.asarray(centre[:n], I64), case["centre"]) and (np.asarray(centre[n:]) == SENTI).all())


def regulate_equal(case, out):
    """out: the whole float buffer [rows, ld]: rows [0, n) x columns [0, C) = the gathered encoding, bit for bit; every other element the canary."""
    n, C = case["n"], case["C"]
    want = bits(sent(out.shape)).copy()
    want[:n, :C] = bits(case["enc"][case["src"], :C])
    return bool(np.array_equal(bits(out), want))


def token_map_model(case, n_buf, mutant=None):
    """int32 model of frame_token_map_kernel (256 tokens per pass, running carry).  Mutants: carry (dropped at the 256-token boundary), rep_first (rep scales a
    token's first frame but not its last), tail0 (the frames past the last run take token 0)."""
    dur, tok_off, frm_off, rep = case["dur"], case["tok_off"], case["frm_off"], case["rep"]
    out = np.full(n_buf, SENTI, I32)
    for u in range(len(tok_off) - 1):
        t0, P = int(tok_off[u]), int(tok_off[u + 1] - tok_off[u])
        f0, nf = int(frm_off[u]), int(frm_off[u + 1] - frm_off[u])
        carry = 0
        for base in range(0, P, 256):
            d = np.maximum(dur[t0 + base:t0 + min(base + 256, P)], 0).astype(I32)
            end = carry + np.cumsum(d, dtype=I32)
            for i in range(len(d)):
                lo = rep * (end[i] - d[i])
                hi = min(end[i] if mutant == "rep_first" else rep * end[i], nf)
                if hi > lo:
                    out[f0 + lo:f0 + hi] = t0 + base + i
            if mutant != "carry":
                carry = int(end[-1])
        if rep * carry < nf:
            out[f0 + rep * carry:f0 + nf] = t0 if mutant == "tail0" else t0 + max(P - 1, 0)
    return out


# ------------------------------------------------------------------------------------------------ alignment matrix
ALIGN_P = (1, 2, 1024)


def alignment_ref(dur):
    d = np.asarray(dur, I64)
    end = np.cumsum(d)
    t = np.arange(int(end[-1]))
    return ((t[None, :] >= (end - d)[:, None]) & (t[None, :] < end[:, None])).astype(F32)


@functools.lru_cache(maxsize=None)
def alignment_case(P):
    if P == 1:
        dur = np.array([5], I32)
    elif P == 2:
        dur = np.array([0, 3], I32)
    else:
        dur = (synth.uniform(f"glue.align.{P}", (P,)) < 0.08).astype(I32)
        dur[-1] = 2
    return dict(P=P, dur=dur, T=int(dur.sum()), ref=alignment_ref(dur))


def alignment_equal(case, out):
    """out: flat float buffer, P * T matrix elements then canaries."""
    n = case["P"] * case["T"]
    return bool(np.array_equal(bits(out[:n]), bits(case["ref"].ravel())) and (bits(out[n:]) == SENT32).all())


# ------------------------------------------------------------------------------------------------ duration decode
DECODE_SCALES = (1.0, 8.0, 40.0)
DECODE_ROWS = 4096
DECODE_N_ROWS = (1, 255, 256, 257)
DECODE_MARGIN = 2e-4  # three times the ~7e-5 an fp32 softmax of 16 terms times a table value <= 46 can be off by (25 roundings of 6e-8 x 46)
TIE_PAIRS = ((9, 12), (7, 46), (15, 18), (12, 15))  # durations; half-integer means 10.5 -> 10, 26.5 -> 26, 16.5 -> 16, 13.5 -> 14
TIE_EXPECT = (10, 26, 16, 14)


def decode_ref(logits):
    """-> (dur int64, sure, expected float64).  sure: the row's rounding does not hang on an fp32 softmax (hard branch, or the expected duration further than
    DECODE_MARGIN from a half-integer)."""
    l = np.asarray(logits, F64)
    e = np.exp(l - l.max(-1, keepdims=True))
    exp = (e / e.sum(-1, keepdims=True)) @ CLASS_TO_DUR
    hard = CLASS_TO_DUR[np.argmax(l, -1)]  # (the first maximum)
    dur = np.where(hard < 7, hard, np.maximum(np.rint(exp), 1.0)).astype(I64)
    sure = (hard < 7) | (np.abs(exp - np.floor(exp) - 0.5) > DECODE_MARGIN)
    return dur, sure, exp


def _tie_row(classes, value=100.0):
    r = np.full(16, -1e4, F32)
    r[list(classes)] = value
    return r


@functools.lru_cache(maxsize=None)
def decode_case():
    """random: DECODE_ROWS rows per scale;  ties: two equal logits (100, all others -1e4) on TIE_PAIRS, argmax ties across the hard / soft boundary, all-equal rows;
    large: logits of +-80."""
    idx = {int(d): i for i, d in enumerate(CLASS_TO_DUR)}
    rand = {s: (synth.normal(f"glue.decode.{s}", (DECODE_ROWS, 16)) * F32(s)).astype(F32) for s in DECODE_SCALES}
    ties = [_tie_row((idx[a], idx[b])) for a, b in TIE_PAIRS]
    ties += [_tie_row(c) for c in ((5, 6), (6, 7), (5, 15), (0, 15), (2, 6, 9), (6, 15))]
    ties += [np.full(16, v, F32) for v in (0.0, 100.0, -1e4)]
    large = np.where(synth.normal("glue.decode.large", (512, 16)) > 0, F32(80), F32(-80)).astype(F32)
    return dict(rand=rand, ties=np.stack(ties), large=large)


def decode_equal(ref_dur, sure, got):
    return bool(np.array_equal(np.asarray(got, I64)[sure], ref_dur[sure]))


def decode_model(logits, mutant=None):
    """fp32 model of duration_decode_kernel.  Mutants: half_away (round half away from zero), argmax_last, no_max (softmax without subtracting the maximum)."""
    l = np.asarray(logits, F32)
    am = 15 - np.argmax(l[:, ::-1], -1) if mutant == "argmax_last" else np.argmax(l, -1)
    mx = np.zeros((len(l), 1), F32) if mutant == "no_max" else l.max(-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(l - mx, dtype=F32)
        den = np.zeros(len(l), F32)
        for k in range(16):
            den = den + e[:, k]
        soft = np.zeros(len(l), F32)
        for k in range(16):
            soft = soft + (e[:, k] / den) * F32(CLASS_TO_DUR[k])
        soft = np.floor(soft + F32(0.5)) if mutant == "half_away" else np.rint(soft)
        soft = np.maximum(soft, F32(1))
    hard = CLASS_TO_DUR[am].astype(F32)
    out = np.where(hard < 7, hard, soft)
    return np.where(np.isfinite(out), out, -1).astype(I64)


# ------------------------------------------------------------------------------------------------ embedding, style broadcast, row -> utterance, transposes (exact)
EMBED_CASES = ((178, 4, 9), (178, 132, 37), (64, 512, 2100))  # (vocabulary, C, rows); 2100 x 512 / 4 float4s exceed the grid's 1024 blocks: the stride loop runs


@functools.lru_cache(maxsize=None)
def embed_case(vocab, C, rows):
    emb = synth.normal(f"glue.embed.{vocab}.{C}", (vocab, C))
    tok = ints(f"glue.embed.tok.{vocab}.{C}", rows, 0, vocab - 1)
    tok[0], tok[-1] = 0, vocab - 1
    if rows > 2:
        tok[1] = vocab - 1
    bad = tok.copy()  # the same with ids outside the vocabulary
    bad[rows // 2] = vocab
    bad[rows // 3] = -1
    return dict(emb=emb, tokens=tok, bad=bad)


def embed_ref(emb, tokens):
    """-> (rows, status bit): emb[token] * sqrt(C) as fp32 (one product, correctly rounded: exact to compare); an id outside the vocabulary takes row 0."""
    t = np.asarray(tokens, I64)
    oor = (t < 0) | (t >= len(emb))
    return (emb[np.where(oor, 0, t)] * np.sqrt(F32(emb.shape[1]))).astype(F32), 2 if oor.any() else 0


def window_equal(out, want, rows, col0, cols):
    """out [rows_buf, ld]: rows [0, rows) x columns [col0, col0 + cols) = want bit for bit, every other element the canary."""
    w = bits(sent(out.shape)).copy()
    w[:rows, col0:col0 + cols] = bits(want)
    return bool(np.array_equal(bits(out), w))


BROADCAST_LENGTHS = (1, 5, 300, 2, 1)
ROW_UTT_LENGTHS = (1, 300, 0, 257, 1, 256)
TRANSPOSE_SHAPES = ((3, 130, 77), (2, 1, 1), (2, 33, 31), (1, 33, 33), (2, 1, 33), (1, 40, 1))


def row_utt_ref(lengths):
    return np.repeat(np.arange(len(lengths), dtype=I64), lengths)


# ------------------------------------------------------------------------------------------------ one-channel conv
CHAN_LENGTHS = (1, 2, 7, 8, 9, 31, 32, 33, 100)
CHAN_NTAPS = (1, 3, 7)
CHAN_C = (64, 256, 260)
CHAN_PREC = (0, 1, 2)
CHAN_LDY, CHAN_YCOL = 12, 7  # the output column: the last one the conv owns, inside a wider row (as the Nyquist bin 1024 of 1056)


def chan_ref(x, w, bias, lengths):
    """x [rows, C], w [ntaps, C] -> (y, sum|a b| + |bias|) in float64, zero padding per utterance."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    k = len(w)
    pad = (k - 1) // 2
    off = offsets(lengths)
    y, sa = np.zeros(len(x), F64), np.zeros(len(x), F64)
    for u, L in enumerate(lengths):
        xp = np.zeros((L + 2 * pad, x.shape[1]), F64)
        xp[pad:pad + L] = x[off[u]:off[u + 1]]
        for t in range(k):
            y[off[u]:off[u + 1]] += xp[t:t + L] @ w[t]
            sa[off[u]:off[u + 1]] += np.abs(xp[t:t + L]) @ np.abs(w[t])
    return y + bias, sa + abs(bias)


@functools.lru_cache(maxsize=None)
def chan_case(prec, ntaps, C):
    """Two (x, w, bias) sets.  The first and last three rows of every utterance and all pad columns of x are 1e3 times larger than the rest; x holds values of the
    row type `prec` exactly."""
    R, ldx = sum(CHAN_LENGTHS), C + 8
    off = offsets(CHAN_LENGTHS)
    edge = np.zeros(R, bool)
    for u in range(len(CHAN_LENGTHS)):
        edge[off[u]:min(off[u] + 3, off[u + 1])] = True
        edge[max(off[u + 1] - 3, off[u]):off[u + 1]] = True
    sets = []
    for i in range(2):
        x = synth.normal(f"glue.chan.x{i}.{ntaps}.{C}", (R, ldx)).astype(F32)
        x[edge, :C] *= F32(1e3)
        x[:, C:] *= F32(1e3)
        x = round_to(x, prec)
        w = (synth.normal(f"glue.chan.w{i}.{ntaps}.{C}", (ntaps, C)) * F32(0.1)).astype(F32)
        bias = float(F32(0.75 - 2.0 * i))
        y, sa = chan_ref(x[:, :C], w, bias, CHAN_LENGTHS)
        sets.append(dict(x=x, w=w, bias=bias, ref=y, sumabs=sa))
    return dict(prec=prec, ntaps=ntaps, C=C, ldx=ldx, R=R, n=ntaps * C, sets=sets)


def chan_ratio(case, i, got):
    s = case["sets"][i]
    return ratio(got, s["ref"], dot_bound(case["n"], s["sumabs"], s["ref"]))


def chan_model(x, w, bias, lengths, mutant=None):
    """fp32 model of single_channel_conv_kernel on x [rows, C].  Mutants: halo (a row outside the utterance is read from the neighbour where it should be zero),
    taps_reversed, no_bias."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    if mutant == "taps_reversed":
        w = w[::-1]
    k = len(w)
    pad = (k - 1) // 2
    off = offsets(lengths)
    R = len(x)
    y = np.zeros(R, F32)
    for u in range(len(lengths)):
        for r in range(off[u], off[u + 1]):
            acc = F32(0)
            for t in range(k):
                g = r + t - pad
                inside = off[u] <= g < off[u + 1]
                if inside or (mutant == "halo" and 0 <= g < R):
                    acc = acc + np.dot(x[g], w[t])
            y[r] = acc + (F32(0) if mutant == "no_bias" else F32(bias))
    return y


# ------------------------------------------------------------------------------------------------ decoder front
FRONT_LENGTHS = (1, 2, 3, 64, 257)
FRONT = dict(C=128, ld_asr=132, ld_enc=160, c_hidden=512, c_res=64, ld_x=608)
FRONT_WF, FRONT_BF, FRONT_WN, FRONT_BN = (0.3, -1.1, 0.7), 0.25, (-0.6, 0.9, 0.2), -1.5


def tap3_ref(x, wt, b, lengths):
    y, sa = chan_ref(np.asarray(x, F64)[:, None], np.asarray([[F32(v)] for v in wt], F64), float(F32(b)), lengths)
    return y, sa


@functools.lru_cache(maxsize=None)
def front_case():
    R = sum(FRONT_LENGTHS)
    asr = synth.normal("glue.front.asr", (R, FRONT["ld_asr"])).astype(F32)
    asr[:, FRONT["C"]:] *= F32(1e3)
    pitch = (80 + 220 * synth.uniform("glue.front.pitch", (R,))).astype(F32)
    pitch[::11] = 0  # unvoiced frames
    energy = (2 + 2 * synth.uniform("glue.front.energy", (R,))).astype(F32)
    f0, f0_abs = tap3_ref(pitch, FRONT_WF, FRONT_BF, FRONT_LENGTHS)
    n, n_abs = tap3_ref(energy, FRONT_WN, FRONT_BN, FRONT_LENGTHS)
    return dict(R=R, asr=asr, pitch=pitch, energy=energy, f0=f0, f0_abs=f0_abs, n=n, n_abs=n_abs)


def front_check(case, enc_in, xa, xb):
    """The whole buffers (rows past R included).  -> dict(exact=..., f0=ratio, n=ratio): exact covers the copied encoding, the zeros, the untouched columns and rows,
    and that the three buffers carry the same F0 / N bits."""
    R, C, cc = case["R"], FRONT["C"], FRONT["c_hidden"] + FRONT["c_res"]
    zero = np.uint32(0)
    ok = np.array_equal(bits(enc_in[:R, :C]), bits(case["asr"][:, :C])) and (bits(enc_in[:R, C + 2:]) == zero).all() and (bits(enc_in[R:]) == SENT32).all()
    for x in (xa, xb):
        ok = ok and (bits(x[:, :cc]) == SENT32).all() and (bits(x[R:]) == SENT32).all() and (bits(x[:R, cc + 2:]) == zero).all()
        ok = ok and np.array_equal(bits(x[:R, cc:cc + 2]), bits(enc_in[:R, C:C + 2]))
    return dict(exact=bool(ok), f0=ratio(enc_in[:R, C], case["f0"], dot_bound(3, case["f0_abs"], case["f0"])),
                n=ratio(enc_in[:R, C + 1], case["n"], dot_bound(3, case["n_abs"], case["n"])))


def front_model(case, mutant=None):
    """fp32 model of decoder_front_kernel -> (enc_in, xa, xb) with a canary row behind.  Mutant: f0_on_energy (the F0 filter and bias applied to the energy curve)."""
    R, C, cc = case["R"], FRONT["C"], FRONT["c_hidden"] + FRONT["c_res"]
    f0 = chan_model(case["pitch"][:, None], np.array(FRONT_WF, F32)[:, None], FRONT_BF, FRONT_LENGTHS)
    if mutant == "f0_on_energy":
        n = chan_model(case["energy"][:, None], np.array(FRONT_WF, F32)[:, None], FRONT_BF, FRONT_LENGTHS)
    else:
        n = chan_model(case["energy"][:, None], np.array(FRONT_WN, F32)[:, None], FRONT_BN, FRONT_LENGTHS)
    enc_in, xa, xb = sent((R + 1, FRONT["ld_enc"])).copy(), sent((R + 1, FRONT["ld_x"])).copy(), sent((R + 1, FRONT["ld_x"])).copy()
    enc_in[:R] = 0
    enc_in[:R, :C] = case["asr"][:, :C]
    enc_in[:R, C], enc_in[:R, C + 1] = f0, n
    for x in (xa, xb):
        x[:R, cc:] = 0
        x[:R, cc], x[:R, cc + 1] = f0, n
    return enc_in, xa, xb


# ------------------------------------------------------------------------------------------------ style projection
STYLE_K = (64, 128)
STYLE_J = (4, 130, 1026)
STYLE_N_UTT = (1, 15, 16, 17, 64, 65, 130)  # both sides of the switch between the two kernels (16) and of the 64-lane pass


@functools.lru_cache(maxsize=None)
def style_case(K, J):
    W = (synth.normal(f"glue.style.w.{K}.{J}", (J, K)) * F32(0.2)).astype(F32)
    b = synth.normal(f"glue.style.b.{K}.{J}", (J,)).astype(F32)
    s = synth.normal(f"glue.style.s.{K}", (max(STYLE_N_UTT), K)).astype(F32)
    ref = s.astype(F64) @ W.astype(F64).T + b
    sa = np.abs(s.astype(F64)) @ np.abs(W.astype(F64)).T + np.abs(b)
    return dict(K=K, J=J, ld=(J + 3) // 4 * 4, W=W, b=b, s=s, ref=ref, sumabs=sa)


def style_check(case, n_utt, out):
    """out [n_utt + 1, ld]: -> (exact: pad columns 0, the row behind untouched; ratio over [n_utt, J])."""
    J = case["J"]
    exact = bool((bits(out[:n_utt, J:]) == 0).all() and (bits(out[n_utt:]) == SENT32).all())
    return exact, ratio(out[:n_utt, :J], case["ref"][:n_utt], dot_bound(case["K"], case["sumabs"][:n_utt], case["ref"][:n_utt]))


def style_model(case, n_utt, mutant=None):
    """fp32 model of the style projection.  Mutant: cols64 (the style columns from 64 on are ignored)."""
    K = 64 if mutant == "cols64" else case["K"]
    out = sent((n_utt + 1, case["ld"])).copy()
    out[:n_utt] = 0
    out[:n_utt, :case["J"]] = (case["s"][:n_utt, :K] @ case["W"][:, :K].T + case["b"]).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ mean over an utterance's rows
MEAN_LENGTHS = (1, 2, 255, 1000)
MEAN_C = (64, 130)


@functools.lru_cache(maxsize=None)
def mean_case(C):
    """Mean 100, deviation 1 (a lost term moves the mean by 100 / n); pad columns 1e3 times larger."""
    R = sum(MEAN_LENGTHS)
    x = (100 + synth.normal(f"glue.mean.{C}", (R, C + 6))).astype(F32)
    x[:, C:] *= F32(1e3)
    off = offsets(MEAN_LENGTHS)
    ref = np.stack([x[off[u]:off[u + 1], :C].astype(F64).mean(0) for u in range(len(MEAN_LENGTHS))])
    sa = np.stack([np.abs(x[off[u]:off[u + 1], :C].astype(F64)).mean(0) for u in range(len(MEAN_LENGTHS))])
    return dict(C=C, R=R, x=x, ref=ref, sumabs=sa)


def mean_ratio(case, got):
    """n = the utterance's length: the sum of n terms, then one division (the output rounding)."""
    n = np.array(MEAN_LENGTHS, F64)[:, None]
    return ratio(got, case["ref"], dot_bound(n, case["sumabs"], case["ref"]))


def mean_model(case, mutant=None):
    """fp32 model of mean_rows_kernel.  Mutants: div_max (divided by the batch's longest length), drop_last (the last row is not summed)."""
    off = offsets(MEAN_LENGTHS)
    out = []
    for u, L in enumerate(MEAN_LENGTHS):
        rows = case["x"][off[u]:off[u + 1], :case["C"]]
        if mutant == "drop_last" and L > 1:
            rows = rows[:-1]
        s = np.zeros(case["C"], F32)
        for r in rows:
            s = s + r
        out.append(s / F32(max(MEAN_LENGTHS) if mutant == "div_max" else L))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ x4 linear upsample
UPSAMPLE_LENGTHS = (1, 2, 3, 0, 255, 256, 257)  # a zero-length utterance between two others


def upsample_ref(x):
    """One utterance [T] -> (y [4 T], |x_i0| + |x_i1|) in float64."""
    x = np.asarray(x, F64)
    T = len(x)
    o = np.arange(4 * T)
    src = np.maximum((o + 0.5) / 4 - 0.5, 0.0)
    i0 = np.floor(src).astype(I64)
    i1 = np.minimum(i0 + 1, T - 1)
    lam = src - i0
    return (1 - lam) * x[i0] + lam * x[i1], np.abs(x[i0]) + np.abs(x[i1])


@functools.lru_cache(maxsize=None)
def upsample_case():
    R = sum(UPSAMPLE_LENGTHS)
    x = (150 + 60 * synth.normal("glue.upsample", (R,))).astype(F32)
    off = offsets(UPSAMPLE_LENGTHS)
    parts = [upsample_ref(x[off[u]:off[u + 1]]) for u in range(len(UPSAMPLE_LENGTHS))]
    return dict(R=R, x=x, ref=np.concatenate([p[0] for p in parts]), mag=np.concatenate([p[1] for p in parts]))


def upsample_ratio(case, got):
    return ratio(got, case["ref"], 3 * U * case["mag"])


def upsample_model(case, mutant=None):
    """fp32 model of upsample4_kernel.  Mutant: align_corners (the align_corners=True source positions)."""
    off = offsets(UPSAMPLE_LENGTHS)
    out = []
    for u, T in enumerate(UPSAMPLE_LENGTHS):
        x = case["x"][off[u]:off[u + 1]]
        o = np.arange(4 * T, dtype=F32)
        if mutant == "align_corners":
            src = o * F32((T - 1) / max(4 * T - 1, 1))
        else:
            src = np.maximum((o + F32(0.5)) * F32(0.25) - F32(0.5), F32(0))
        i0 = np.floor(src).astype(I64)
        i1 = np.minimum(i0 + 1, T - 1)
        lam = (src - i0.astype(F32)).astype(F32)
        out.append(((F32(1) - lam) * x[i0] + lam * x[i1]).astype(F32) if T else np.zeros(0, F32))
    return np.concatenate(out)

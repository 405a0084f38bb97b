"""The text aligner and the CTC forced alignment on the engine (csrc/aligner.hip.h) against the reference fixtures of
tests/golden/gen_golden_aligner.py and the float64 dynamic programme of tests/aligner64.py.

The network is judged against the FLOAT64 run of the reference: for every tap the fixture holds the reference's own fp32 values and the float64
values at the same sampled indices, and the engine's max-abs and rms error against float64 must be at most BAR = 4 x the reference fp32 run's own
error there (the bar and the reasoning of tests/test_hip_ssl.py).  The Viterbi kernel runs on log-probs that are multiples of 2^-8 in [-16, 0]:
every fp32 sum over up to 600 frames is then exact (|sum| <= 9600 < 2^14, 14 + 8 = 22 bits), so its path's score must EQUAL the float64 optimum.
Inputs are regenerated from their names (the generator's recipes)."""
import os

import numpy as np
import pytest

import aligner64 as A

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 4.0
N_MELS, TOKENS, V = 80, 178, 179
CASE_OF = dict(t1="short", t2="short", t5="short", t17="short", t33="short", t40="t40", t100="t100", dense="dense")


def mel_input(run, B, T):
    from stylish_tts_amd import synth

    return torch.from_numpy(synth.normal("aligner.mel." + run, (B, T, N_MELS)).astype(np.float32))


def targets_for(run, P):
    from stylish_tts_amd import synth

    t = np.clip((synth.uniform("aligner.targets." + run, (P,)).astype(np.float64) * TOKENS).astype(np.int64), 0, TOKENS - 1)
    if P >= 4:
        t[2] = t[1]
    return t


def gold(run):
    return np.load(os.path.join(GOLD, f"aligner_{CASE_OF[run]}.npz"))


_ENGINES, _MODS = {}, {}


def aligner(precision="f32"):
    """The aligner with the fixtures' synthetic weights (seed 0) on an engine of the given precision (one engine per precision)."""
    from stylish_tts_amd import modules
    from stylish_tts_amd.runtime import HipModel

    if precision not in _MODS:
        _ENGINES[precision] = HipModel(None, 0, precision=precision)
        _MODS[precision] = modules.TextAligner(N_MELS, TOKENS, engine=_ENGINES[precision]).load_synthetic(0)
    return _MODS[precision]


# ------------------------------------------------------------------------------------------------ a. the network
@pytest.mark.parametrize("run,B,T", [("t1", 1, 1), ("t2", 1, 2), ("t5", 1, 5), ("t17", 1, 17), ("t33", 1, 33), ("t100", 1, 100), ("dense", 2, 64)])
def test_network_every_tap_against_float64(run, B, T):
    g = gold(run)
    lp, seg, taps = aligner().packed(mel_input(run, B, T), taps=True)
    got = {k: v.cpu().double().numpy().ravel() for k, v in taps.items()}
    bad, worst = [], [0.0, 0.0]
    for tap in ("tdnn0", "tdnn1", "tdnn2", "ffn", "logits"):
        idx, f32, f64 = g[f"{run}_{tap}_idx"].astype(np.int64), g[f"{run}_{tap}_f32"].astype(np.float64), g[f"{run}_{tap}_f64"]
        ref_e, my_e = f32 - f64, got[tap][idx] - f64
        ref_max, ref_rms = np.abs(ref_e).max(), np.sqrt((ref_e**2).mean())
        my_max, my_rms = np.abs(my_e).max(), np.sqrt((my_e**2).mean())
        worst[0], worst[1] = max(worst[0], my_max / ref_max), max(worst[1], my_rms / ref_rms)
        print(f"{run:>6s} {tap:>6s}: engine max {my_max:.2e} rms {my_rms:.2e} | reference fp32 max {ref_max:.2e} rms {ref_rms:.2e} | ratio {my_max / ref_max:.2f} {my_rms / ref_rms:.2f}")
        if not (my_max <= BAR * ref_max and my_rms <= BAR * ref_rms):
            bad.append((tap, my_max, ref_max, my_rms, ref_rms))
    lp64, lp32 = g[f"{run}_lp64"].reshape(-1, V), g[f"{run}_lp32"].reshape(-1, V).astype(np.float64)
    mine = lp.cpu().double().numpy()
    assert mine.shape == lp64.shape
    ref_e, my_e = lp32 - lp64, mine - lp64
    r = np.abs(my_e).max() / np.abs(ref_e).max(), np.sqrt((my_e**2).mean()) / np.sqrt((ref_e**2).mean())
    print(f"{run:>6s} log_probs: engine max {np.abs(my_e).max():.2e} | reference fp32 max {np.abs(ref_e).max():.2e} | ratio {r[0]:.2f} {r[1]:.2f}; worst tap ratio {worst[0]:.2f} {worst[1]:.2f}")
    if not (r[0] <= BAR and r[1] <= BAR):
        bad.append(("log_probs",) + r)
    assert not bad, bad
    assert np.abs(np.exp(mine).sum(axis=1) - 1).max() < 1e-5


def test_forward_has_the_reference_layout():
    m = aligner()
    mel = torch.zeros(2, 33, N_MELS)
    mel[0], mel[1, :17] = mel_input("t33", 1, 33)[0], mel_input("t17", 1, 17)[0]
    out, none = m(mel, torch.tensor([33, 17]))
    assert none is None and tuple(out.shape) == (33, 2, V)
    assert np.array_equal(out[:, 0].cpu().numpy(), m.packed(mel[:1])[0].cpu().numpy())
    assert torch.equal(out[:17, 1], m.packed(mel[1:, :17])[0]) and not out[17:, 1].any()


# ------------------------------------------------------------------------------------------------ b. the Viterbi kernel on exact inputs
def exact_log_probs(name, T):
    from stylish_tts_amd import synth

    return -(np.floor(synth.uniform("aligner.exact." + name, (T, V)).astype(np.float64) * 4097).clip(0, 4096)) / 256.0


def tokens_for(name, P, repeats=True):
    from stylish_tts_amd import synth

    t = np.clip((synth.uniform("aligner.tok." + name, (P,)).astype(np.float64) * TOKENS).astype(np.int64), 0, TOKENS - 1)
    for i in range(1, P):  # no accidental repeats ...
        if t[i] == t[i - 1]:
            t[i] = (t[i] + 1) % TOKENS
    if repeats and P >= 8:  # ... and two deliberate ones
        t[3] = t[2]
        t[P - 1] = t[P - 2]
    return t


VITERBI_CASES = {
    "p1_t1": (1, 1, None), "p1_t7": (1, 7, None), "t_equals_p": (24, 24, "distinct"), "one_token": (20, 39, "same"), "p32": (32, 80, None),
    "p33": (33, 80, None), "p128": (128, 300, None), "p510": (510, 600, None),
}


def viterbi_case(name):
    P, T, kind = VITERBI_CASES[name]
    tg = np.full(P, 7, np.int64) if kind == "same" else tokens_for(name, P, repeats=kind != "distinct")
    assert A.min_frames(tg) <= T and (kind is None or A.min_frames(tg) == T)
    return exact_log_probs(name, T), tg


def run_ctc(cases, path=None):
    """cases: list of (log_probs [T, V] float64-valued, targets [P]) -> the engine's outputs per utterance, as numpy"""
    from stylish_tts_amd.runtime import Segments

    eng = aligner().engine
    seg_t, seg_p = Segments([c[0].shape[0] for c in cases], eng.device), Segments([len(c[1]) for c in cases], eng.device)
    lp = torch.from_numpy(np.concatenate([c[0] for c in cases]).astype(np.float32))
    tg = torch.from_numpy(np.concatenate([c[1] for c in cases]).astype(np.int32))
    r = eng.ctc_align(seg_t, lp, seg_p, tg, TOKENS, path=None if path is None else torch.from_numpy(np.concatenate(path).astype(np.int32)))
    r = {k: v.cpu().numpy() for k, v in r.items()}
    out = []
    for u in range(len(cases)):
        a, b, p, q = seg_t.host[u], seg_t.host[u + 1], seg_p.host[u], seg_p.host[u + 1]
        out.append(dict(path=r["path"][a:b], scores=r["scores"][a:b], durations=r["durations"][p:q], left=r["left"][p:q], right=r["right"][p:q]))
    return out


def check_exact(lp, tg, got):
    T, P = lp.shape[0], len(tg)
    _, best = A.viterbi(lp, tg, TOKENS)
    A.path_states(got["path"], tg, TOKENS)  # monotone, every token in order, equal neighbours separated by a blank, allowed start and end
    assert A.path_score(lp, got["path"]) == best, (A.path_score(lp, got["path"]), best)
    assert np.array_equal(got["scores"].astype(np.float64), lp[np.arange(T), got["path"]])
    d = got["durations"]
    assert d.sum() == T and d.min() >= 1 and np.array_equal(d, A.durations(got["path"], P, TOKENS))
    assert got["left"][-1] == 0 and got["right"][-1] == 0


@pytest.mark.parametrize("name", list(VITERBI_CASES))
def test_viterbi_path_is_valid_and_optimal_on_exact_inputs(name):
    lp, tg = viterbi_case(name)
    got = run_ctc([(lp, tg)])[0]
    check_exact(lp, tg, got)
    again = run_ctc([(lp, tg)])[0]
    assert all(np.array_equal(got[k], again[k]) for k in got)  # the tie rule is fixed: the same path every time


def test_viterbi_ragged_batch_on_exact_inputs():
    cases = [viterbi_case(n) for n in ("p33", "p1_t1", "p128", "one_token")]
    batch = run_ctc(cases)
    for (lp, tg), got in zip(cases, batch):
        check_exact(lp, tg, got)
        solo = run_ctc([(lp, tg)])[0]
        assert all(np.array_equal(got[k], solo[k]) for k in got)


# ------------------------------------------------------------------------------------------------ c. the post-processing alone
@pytest.mark.parametrize("run,P", [("t5", 2), ("t33", 9), ("t40", 12), ("t100", 30)])
def test_post_processing_of_the_fixture_path(run, P):
    g = gold(run)
    lp32, tg, path = g[f"{run}_lp32"][0].astype(np.float64), g[f"{run}_targets"].astype(np.int64), g[f"{run}_path"]
    assert len(tg) == P
    got = run_ctc([(lp32, tg)], path=[path])[0]
    assert np.array_equal(got["path"], path) and np.array_equal(got["durations"], g[f"{run}_dur"])
    assert np.array_equal(got["scores"], g[f"{run}_lp32"][0][np.arange(len(path)), path])
    for side in ("left", "right"):
        f32, f64 = g[f"{run}_{side}32"].astype(np.float64), g[f"{run}_{side}64"]
        ref_e, my_e = np.abs(f32 - f64).max(), np.abs(got[side].astype(np.float64) - f64).max()
        print(f"{run} {side}: engine {my_e:.2e} | reference fp32 loop {ref_e:.2e} | ratio {my_e / ref_e:.2f}")
        assert my_e <= BAR * ref_e
        assert got[side][-1] == 0


def test_post_processing_counts_leading_blanks_to_the_first_token():
    """The one stated deviation from torch_align: its loop advances text_index at the first token of a path that begins with blanks and trips its
    own assert; here those frames belong to token 0.  Checked against aligner64 on the fixture's fp32 log-probs.  Tolerance: the engine adds two
    log-probs in fp32 like the reference (|sum| <= 2 max|lp|, so 2^-24 * 2 max|lp| absolute in each exponent = relative in each product), forms the
    quotient in double and rounds it once to fp32; two products differ in a quotient."""
    b = TOKENS
    lp = gold("t33")["t33_lp32"][0][:10].astype(np.float64)
    tg = np.array([5, 5, 9])
    path = np.array([b, b, 5, 5, b, 5, 9, 9, b, b])
    got = run_ctc([(lp, tg)], path=[path])[0]
    d = A.durations(path, 3, b)
    assert d.tolist() == [5, 1, 4] and np.array_equal(got["durations"], d)
    left, right = A.boundaries(lp, tg, d)
    tol = 2 * (2.0**-24 * 2 * np.abs(lp).max()) + 2.0**-24
    assert np.abs(got["left"] - left).max() <= tol and np.abs(got["right"] - right).max() <= tol
    assert left[0] == pytest.approx(1 / 3) and 0 < left[1] < 1


# ------------------------------------------------------------------------------------------------ d. ragged batches
def test_ragged_batch_equals_solo_runs_bit_for_bit():
    m = aligner()
    L, PL = [5, 33, 100], [2, 9, 30]
    runs = ["t5", "t33", "t100"]
    mel = torch.zeros(3, 100, N_MELS)
    text = torch.zeros(3, 30, dtype=torch.int64)
    for b, (run, n, p) in enumerate(zip(runs, L, PL)):
        mel[b, :n] = mel_input(run, 1, n)[0]
        text[b, :p] = torch.from_numpy(targets_for(run, p))
    lp, seg = m.packed(mel, L)
    stacks, scores = m.align(mel, L, text, PL)
    eng = m.engine
    from stylish_tts_amd.runtime import Segments

    paths = eng.ctc_align(seg, lp, Segments(PL, eng.device), torch.cat([text[b, :p] for b, p in enumerate(PL)]).to(torch.int32), TOKENS)["path"]
    for b, (n, p) in enumerate(zip(L, PL)):
        lp1, seg1 = m.packed(mel[b : b + 1, :n])
        assert torch.equal(lp[seg.host[b] : seg.host[b + 1]], lp1), b
        s1, sc1 = m.align(mel[b : b + 1, :n], [n], text[b : b + 1, :p], [p])
        assert tuple(stacks[b].shape) == (3, p) and torch.equal(stacks[b], s1[0]) and torch.equal(scores[b], sc1[0]), b
        p1 = eng.ctc_align(seg1, lp1, Segments([p], eng.device), text[b, :p].to(torch.int32), TOKENS)["path"]
        assert torch.equal(paths[seg.host[b] : seg.host[b + 1]], p1), b
        assert float(stacks[b][0].sum()) == n and float(stacks[b][0].min()) >= 1


# ------------------------------------------------------------------------------------------------ e. end to end against float64
@pytest.mark.parametrize("run,T,P", [("t40", 40, 12), ("t100", 100, 30)])
def test_align_end_to_end_against_float64(run, T, P):
    """Test (a) holds the engine's log-probs within delta = 4 x the reference fp32 run's max-abs error of the float64 ones.  A path's score moves
    by at most T delta under such a perturbation, so the best path of the perturbed problem, scored on the float64 log-probs, is within 2 T delta
    of the float64 optimum; the engine's fp32 accumulation adds at most T 2^-23 max|score| to what it compares.  Nothing is taken from the code
    under test.  (With synthetic weights the log-probs are nearly flat: durations are not compared token by token here.)"""
    from stylish_tts_amd.runtime import Segments

    g = gold(run)
    m = aligner()
    mel, tg = mel_input(run, 1, T), g[f"{run}_targets"].astype(np.int64)
    assert np.array_equal(tg, targets_for(run, P))
    stacks, scores = m.align(mel, [T], torch.from_numpy(tg)[None], [P])
    lp, seg = m.packed(mel)
    eng = m.engine
    r = eng.ctc_align(seg, lp, Segments([P], eng.device), torch.from_numpy(tg).to(torch.int32), TOKENS)
    path = r["path"].cpu().numpy()
    assert torch.equal(stacks[0][0], r["durations"].float()) and torch.equal(scores[0], r["scores"])
    lp64 = g[f"{run}_lp64"][0]
    A.path_states(path, tg, TOKENS)
    _, best = A.viterbi(lp64, tg, TOKENS)
    assert best >= float(g[f"{run}_best64"]) - 1e-9  # (the fixture's optimum is restricted to a start on the first token)
    delta = BAR * float(g[f"{run}_lp_full_err"][0])
    bound = 2 * T * delta + T * 2.0**-23 * abs(best)
    mine = A.path_score(lp64, path)
    print(f"{run}: float64 optimum {best:.6f}, the engine's path {mine:.6f}, gap {best - mine:.2e}, bound {bound:.2e}")
    assert best - bound <= mine <= best + 1e-9
    d = stacks[0][0].cpu().numpy()
    assert d.sum() == T and d.min() >= 1 and float(stacks[0][1][-1]) == 0 and float(stacks[0][2][-1]) == 0
    assert ((stacks[0][1:] >= 0) & (stacks[0][1:] <= 1)).all()


# ------------------------------------------------------------------------------------------------ f. precision
def test_16_bit_engine_gives_the_fp32_bits():
    mel, tg = mel_input("t40", 1, 40), torch.from_numpy(targets_for("t40", 12))[None]
    a, b = aligner("f32"), aligner("bf16")
    assert torch.equal(a.packed(mel)[0].cpu(), b.packed(mel)[0].cpu())
    (sa, ca), (sb, cb) = a.align(mel, [40], tg, [12]), b.align(mel, [40], tg, [12])
    assert torch.equal(sa[0].cpu(), sb[0].cpu()) and torch.equal(ca[0].cpu(), cb[0].cpu())

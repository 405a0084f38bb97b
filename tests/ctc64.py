"""numpy float64 restatement of what csrc/aligner.hip.h (ctc_forward_kernel, the confidence and prior sums) and csrc/val_scores.hip.h (the duration
and difference sums) compute: the targets of tests/test_hip_align_scores.py, pinned against torch in tests/test_ctc64_cpu.py.  Plain numpy over
the definition; nothing here is shared with the code under test."""
import numpy as np

NEG = -np.inf


def _lse(xs):
    """log(sum exp(x)) as m + log(sum exp(x - m)); -inf when every x is -inf."""
    m = max(xs)
    if m == NEG:
        return NEG
    return m + np.log(sum(np.exp(x - m) for x in xs))


def ctc_nll(lp, targets, blank, log_priors=None, prior_scale=0.0):
    """lp [T, >= classes] log-probs of one utterance, targets a list of P >= 1 token ids -> -log of the summed probability of every CTC path
    (states blank, token, blank, ..; stay, +1, and +2 only into a token that differs from the token two states back; start in state 0 or 1, end
    in state 2 P or 2 P - 1), +inf where there is none.  log_priors [classes]: emission = lp - prior_scale * log_priors."""
    lp = np.asarray(lp, np.float64)
    T, P = lp.shape[0], len(targets)
    S = 2 * P + 1
    labels = [targets[s >> 1] if s & 1 else blank for s in range(S)]
    em = lp[:, labels]
    if log_priors is not None:
        em = em - float(prior_scale) * np.asarray(log_priors, np.float64)[labels]
    skip = np.array([bool(s & 1) and s >= 3 and labels[s] != labels[s - 2] for s in range(S)])
    a = np.full(S, NEG)
    a[0] = em[0, 0]
    a[1] = em[0, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(1, T):  # every state of a frame at once: x = (stay, +1, +2), m + log(sum exp(x - m)) + e, -inf where m is
            x = np.stack([a, np.concatenate([[NEG], a[:-1]]), np.where(skip, np.concatenate([[NEG, NEG], a[:-2]]), NEG)])
            m = x.max(0)
            dead = np.isneginf(m)
            z = np.exp(x - np.where(dead, 0.0, m))
            a = np.where(dead, NEG, m + np.log((z[0] + z[1]) + z[2]) + em[t])
    v = _lse([a[S - 1], a[S - 2]])
    return np.inf if v == NEG else -v


def make_log_probs(seed, T, classes=179, scale=3.0):
    """[T, classes] float32 rows of a float64 log-softmax of normal draws."""
    x = np.random.default_rng(seed).standard_normal((T, classes)) * scale
    x = x - x.max(1, keepdims=True)
    return (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)


def make_tokens(seed, P, symbols=178, equal_pairs=0):
    """P token ids in [0, symbols) with no two neighbours equal, then `equal_pairs` adjacent equal pairs at positions (0, 1), (3, 4), ..."""
    rng = np.random.default_rng(seed)
    t = [int(rng.integers(0, symbols))]
    while len(t) < P:
        v = int(rng.integers(0, symbols))
        if v != t[-1]:
            t.append(v)
    for k in range(equal_pairs):
        i = 3 * k + 1
        assert i < P
        t[i] = t[i - 1]
        if i + 1 < P and t[i + 1] == t[i]:
            t[i + 1] = (t[i] + 1) % symbols
    return t


def min_frames(targets):
    """The fewest frames that have a path: tokens plus adjacent equal pairs."""
    return len(targets) + sum(1 for i in range(1, len(targets)) if targets[i] == targets[i - 1])


def single_path_nll(lp, targets, blank):
    """At T = min_frames there is one path (a blank exactly between equal neighbours): minus the float64 sum of its log-probs."""
    lp = np.asarray(lp, np.float64)
    path = []
    for i, tk in enumerate(targets):
        if i and targets[i - 1] == tk:
            path.append(blank)
        path.append(tk)
    assert len(path) == lp.shape[0]
    tot = 0.0
    for t, c in enumerate(path):
        tot += lp[t, c]
    return -tot


def confidence_sum(scores):
    return float(np.exp(np.asarray(scores, np.float64)).sum())


def prior_sums(lp, classes):
    """Per-class logsumexp over all rows of lp [R, >= classes]."""
    x = np.asarray(lp, np.float64)[:, :classes]
    m = x.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isneginf(m), 0.0, np.exp(x - np.where(np.isneginf(m), 0.0, m)).sum(0))
        return np.where(np.isneginf(m), NEG, m + np.log(s))


def distance_weight(classes, alpha=2.0, cap=7):
    i = np.arange(classes)
    return np.minimum(np.abs(i[:, None] - i[None, :]), cap).astype(np.float64) ** alpha


def duration_sums(logits, targets, weight):
    """logits [P, C], targets [P], weight [C] -> (sum lsm[p][t] w[t], sum w[t], sum_p sum_c log(1 - sm + 1e-9) d[t][c] / sum_c d[t][c]) in float64."""
    x = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.int64)
    w = np.asarray(weight, np.float64)
    z = x - x.max(1, keepdims=True)
    ex = np.exp(z)
    tot = ex.sum(1, keepdims=True)
    lsm, sm = z - np.log(tot), ex / tot
    d = distance_weight(x.shape[1])[t]
    idx = np.arange(x.shape[0])
    return np.array([(lsm[idx, t] * w[t]).sum(), w[t].sum(), (np.log((1.0 - sm) + 1e-9) * (d / d.sum(1, keepdims=True))).sum()])


def duration_scores(sums, lengths):
    """sums [B, 3], token counts [B] -> (duration_ce, duration, their per-utterance values), DurationLoss.forward's means over the utterances."""
    ce = [-float(s[0]) / (float(s[1]) + 1e-9) for s in sums]
    cdw = [-100.0 * float(s[2]) / float(n) for s, n in zip(sums, lengths)]
    return sum(ce) / len(ce), sum(cdw) / len(cdw), ce, cdw


def diff_sum(a, b, kind):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.abs(d).sum() if kind == "l1" else (d * d).sum())

"""Float64 restatement of the CTC forced alignment and of torch_align's post-processing (the reference's train/dataprep/align_text.py:159-210),
beside flow64.py: the dynamic programme, a path checker, a brute-force enumeration for tiny cases, and the durations / boundary probabilities of a
label path.  numpy only; the tests and tests/golden/gen_golden_aligner.py import it.

States of P tokens: 0 .. 2 P, even = blank, odd s = token (s - 1) / 2.  Transitions: stay, +1, and +2 only into a token state whose token differs
from the token two states back.  A path starts in state 0 or 1 and ends in state 2 P or 2 P - 1."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def state_labels(targets: Sequence[int], blank: int) -> np.ndarray:
    lab = np.full(2 * len(targets) + 1, blank, np.int64)
    lab[1::2] = np.asarray(targets, np.int64)
    return lab


def min_frames(targets: Sequence[int]) -> int:
    t = list(targets)
    return len(t) + sum(1 for a, b in zip(t, t[1:]) if a == b)


def viterbi(log_probs, targets: Sequence[int], blank: int, leading_blank: bool = True) -> Tuple[np.ndarray, float]:
    """The best path's labels [T] and its score, in float64.  Ties: the smaller jump wins, at the end the final blank wins (the engine's rule;
    nothing here depends on it).  leading_blank=False: the path must start in state 1 (what the reference's torch_align loop can digest)."""
    lp = np.asarray(log_probs, np.float64)
    T, P = lp.shape[0], len(targets)
    if P < 1 or T < min_frames(targets):
        raise ValueError(f"{T} frames cannot hold {P} tokens ({min_frames(targets)} needed)")
    lab = state_labels(targets, blank)
    S = lab.size
    skip = np.zeros(S, bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    score = np.full(S, -np.inf)
    score[1] = lp[0, lab[1]]
    if leading_blank:
        score[0] = lp[0, lab[0]]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        best, j = score.copy(), np.zeros(S, np.int8)
        a1 = np.concatenate([[-np.inf], score[:-1]])
        m = a1 > best
        best[m], j[m] = a1[m], 1
        a2 = np.concatenate([[-np.inf, -np.inf], score[:-2]])
        m = skip & (a2 > best)
        best[m], j[m] = a2[m], 2
        score = best + lp[t, lab]
        bp[t] = j
    s = S - 1 if score[S - 1] >= score[S - 2] else S - 2
    total = float(score[s])
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = lab[s]
        s -= int(bp[t, s])
    return path, total


def path_states(path: Sequence[int], targets: Sequence[int], blank: int) -> List[int]:
    """The state sequence of a label path, or ValueError naming the first rule it breaks: an allowed start, monotone steps of at most one token,
    every token in order, equal neighbours separated by a blank, an allowed end."""
    lab = state_labels(targets, blank)
    S = lab.size
    path = [int(v) for v in path]
    if not path:
        raise ValueError("empty path")
    if path[0] == blank:
        s = 0
    elif path[0] == lab[1]:
        s = 1
    else:
        raise ValueError(f"frame 0 carries label {path[0]}: neither blank nor the first token")
    states = [s]
    for t, a in enumerate(path[1:], 1):
        if a == blank:
            if s % 2 == 1:
                s += 1  # (s + 1 <= 2 P always)
        elif s % 2 == 1 and a == lab[s]:
            pass  # stay (a jump of two into an equal token is forbidden, so this is the only reading)
        elif s % 2 == 0:
            if s + 1 >= S or a != lab[s + 1]:
                raise ValueError(f"frame {t}: label {a} after a blank in state {s} is not the next token")
            s += 1
        else:
            if s + 2 >= S or a != lab[s + 2]:
                raise ValueError(f"frame {t}: label {a} after token state {s} is neither that token nor the next one")
            s += 2
        states.append(s)
    if s < S - 2:
        raise ValueError(f"the path ends in state {s} of {S}: tokens are left over")
    return states


def path_score(log_probs, path: Sequence[int]) -> float:
    lp = np.asarray(log_probs, np.float64)
    return float(sum(lp[t, int(a)] for t, a in enumerate(path)))


def brute_force(log_probs, targets: Sequence[int], blank: int) -> float:
    """The best score over ALL valid state sequences, by enumerating them one by one (tiny T and P only); -inf when there is none."""
    lp = np.asarray(log_probs, np.float64)
    T = lp.shape[0]
    lab = state_labels(targets, blank)
    S = lab.size
    best = [-np.inf]

    def walk(t: int, s: int, acc: float):
        acc += lp[t, lab[s]]
        if t == T - 1:
            if s >= S - 2:
                best[0] = max(best[0], acc)
            return
        for d in (0, 1, 2):
            b = s + d
            if b >= S or (d == 2 and (b % 2 == 0 or lab[b] == lab[s])):
                continue
            walk(t + 1, b, acc)

    for s0 in (0, 1):
        walk(0, s0, 0.0)
    return float(best[0])


def durations(path: Sequence[int], n_tokens: int, blank: int) -> np.ndarray:
    """pred_dur of torch_align's first loop: frames of token p plus the blank frames that follow it.  Blank frames in front of the first token count
    to token 0 - the one stated deviation: the reference's loop advances text_index at the first token there and trips its own assert."""
    dur = np.zeros(n_tokens, np.int64)
    k, prev = -1, blank
    for a in path:
        a = int(a)
        if a != blank and a != prev:
            k += 1
        dur[min(max(k, 0), n_tokens - 1)] += 1
        prev = a
    return dur


def boundaries(log_probs, targets: Sequence[int], pred_dur: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """left / right of torch_align's second loop (align_text.py:190-209) in float64."""
    lp = np.asarray(log_probs, np.float64)
    P = len(targets)
    left, right = np.zeros(P), np.zeros(P)
    index = 0
    for i in range(P - 1):
        index += int(pred_dur[i])
        lt, rt = int(targets[i]), int(targets[i + 1])
        lpb = np.exp(lp[index - 1, lt] + lp[index, lt])
        sp = np.exp(lp[index - 1, lt] + lp[index, rt])
        rp = np.exp(lp[index - 1, rt] + lp[index, rt])
        den = lpb + sp + rp
        left[i], right[i] = lpb / den, rp / den
    return left, right

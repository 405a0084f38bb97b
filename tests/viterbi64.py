"""Float64 oracle of RMVPE's Viterbi pitch decoding (the reference's to_viterbi_f0, rmvpe/utils.py:134-150): the objective as
that section states it, solved by the FULL 360 x 360 recursion with no band shortcut, the decision margins, and to_local_average_f0 around a centre.
The targets of tests/test_hip_rmvpe_viterbi.py, checked on their own in tests/test_rmvpe_viterbi_oracle.py.  Plain numpy, written from the
formulas, sharing no code with stylish_tts_amd/rmvpe.py or the kernel."""
import numpy as np

N = 360
EPS = float(np.ldexp(1.0, -126))  # the smallest normal fp32
CENTS_0 = np.float32(1997.3794084376191)


def transition():
    """lt[i][j] = log(A[i][j] + eps), A = w / rowsum(w), w[i][j] = max(30 - |i - j|, 0); float64."""
    xx, yy = np.meshgrid(range(N), range(N))
    w = np.maximum(30 - abs(xx - yy), 0).astype(np.float64)
    return np.log(w / w.sum(axis=1, keepdims=True) + EPS)


_LT = None


def lt():
    global _LT
    if _LT is None:
        _LT = transition()
    return _LT


def emissions(sal):
    """e[t][j] = log(s / sum_j s + eps) in float64; NaN or negative salience = 0; a frame whose sum is 0 or not finite: p = 0 everywhere."""
    s = np.asarray(sal, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(s > 0, s, 0.0)  # NaN > 0 is False
    tot = s.sum(axis=1)
    ok = (tot > 0) & np.isfinite(tot)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where(ok[:, None], s / np.where(ok, tot, 1.0)[:, None], 0.0)
    return np.log(p + EPS)


def viterbi(sal):
    """sal [T, 360] -> dict(path [T] int64, logp, margin, ties).  margin = the smallest gap between the best and the second-best predecessor over
    all (t, j), and at the final argmax; ties = frames t whose decision on the returned path was an exact tie (the final one counts to T - 1).
    Every argmax takes the lowest index among equals (np.argmax)."""
    e = emissions(sal)
    T = e.shape[0]
    L = lt()
    v = e[0] + np.log(1.0 / N + EPS)
    ptr = np.zeros((T, N), np.int64)
    margin = np.inf
    gaps = np.zeros((T, N))
    for t in range(1, T):
        c = v[:, None] + L  # c[i][j]
        ptr[t] = np.argmax(c, axis=0)
        top2 = np.partition(c, N - 2, axis=0)[N - 2 :]
        gaps[t] = top2[1] - top2[0]
        margin = min(margin, float(gaps[t].min()))
        v = e[t] + c[ptr[t], np.arange(N)]
    path = np.zeros(T, np.int64)
    path[T - 1] = int(np.argmax(v))
    top2 = np.partition(v, N - 2)[N - 2 :]
    end_gap = float(top2[1] - top2[0])
    margin = min(margin, end_gap)
    for t in range(T - 1, 0, -1):
        path[t - 1] = ptr[t][path[t]]
    ties = [t for t in range(1, T) if gaps[t][path[t]] == 0.0] + ([T - 1] if end_gap == 0.0 else [])
    return dict(path=path, logp=float(v[path[T - 1]]), margin=margin, ties=sorted(set(ties)))


def score(sal, path):
    """The objective of a given path, added in the recursion's order: ((e0 + start) + lt) -> e + (.) ..."""
    e = emissions(sal)
    L = lt()
    path = np.asarray(path, np.int64)
    v = e[0][path[0]] + np.log(1.0 / N + EPS)
    for t in range(1, len(path)):
        v = e[t][path[t]] + (v + L[path[t - 1], path[t]])
    return float(v)


def local_average_f0(sal, center, thred=0.03):
    """to_local_average_f0 around ``center`` [T] in float64 (the cents mapping is the reference's fp32 tensor): weights = the raw salience on
    [c - 4, c + 5) clipped to [0, 360), added in bin order; f0 = 0 where the frame's largest salience (NaNs ignored) is below thred."""
    s = np.asarray(sal, np.float32)
    out = np.zeros(s.shape[0], np.float64)
    for t, c in enumerate(np.asarray(center, np.int64)):
        a, b = max(0, c - 4), min(N, c + 5)
        ps = wsum = 0.0
        for i in range(a, b):
            cents = np.float32(20 * i) + CENTS_0
            ps += float(s[t, i]) * float(cents)
            wsum += float(s[t, i])
        cents = ps / (wsum + (1.0 if wsum == 0.0 else 0.0))
        row = s[t][~np.isnan(s[t])]
        best = row.max() if row.size else -np.inf
        out[t] = 0.0 if best < np.float32(thred) else 10.0 * 2.0 ** (cents / 1200.0)
    return out


def logp_bound(T, logp):
    """8 T 2^-53 max(1, |logp|): T two-add steps of fp64 rounding, a factor 4 for the device logarithm."""
    return 8.0 * T * 2.0**-53 * max(1.0, abs(logp))


def ulp32(x):
    """The fp32 unit in the last place at |x| (x float64)."""
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def jump_case(switch=10, T=20, a=10, b=300):
    """T frames one-hot at bin a, from frame ``switch`` on at bin b: the optimum jumps across the band."""
    s = np.zeros((T, N), np.float32)
    s[:switch, a] = 1.0
    s[switch:, b] = 1.0
    return s


def pitch_like(T=257, seed=5):
    """A seeded pitch-like salience: a Gaussian bump on a slowly moving track over a noise floor, with a stretch of frames whose harmonic an octave
    (60 bins) above is briefly the larger peak - what the Viterbi decode exists to bridge."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    track = 140.0 + 25.0 * np.sin(t / 31.0) + 6.0 * np.sin(t / 5.3)
    j = np.arange(N)[None, :]
    s = 0.9 * np.exp(-0.5 * ((j - track[:, None]) / 2.2) ** 2)
    harm = np.exp(-0.5 * ((j - track[:, None] - 60.0) / 2.2) ** 2)
    amp = np.full(T, 0.35)
    amp[100:131] = 1.0  # the excursion: 31 frames
    s = s * np.where((t >= 100) & (t < 131), 0.8, 1.0)[:, None] + amp[:, None] * harm * 0.9
    s = s + 0.02 * rng.random((T, N))
    return np.clip(s, 0.0, 1.0).astype(np.float32)

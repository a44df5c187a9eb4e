"""Oracles for dicow_orc_distance (csrc/orc_distance.hip), independent of the module under test: plain Python / numpy only.

  * ``orc_brute``  every assignment of the U utterances to the H streams; per stream a triple-loop Levenshtein table of the assigned
                   utterances' concatenation against the stream, with the cell rule of dicow_edit_distance (key = errors * 2^15 - hits, the
                   diagonal step open only without intervals or when rb < he && hb < re); the minimum of the summed keys.
  * ``orc_dp``     the dynamic program of include/dicow_hip.h over the product of the streams, in numpy: per utterance and per axis one
                   Levenshtein row update per word along that axis, then the elementwise minimum over the axes.

Both return ``(errors, hits)``.  ``utts`` / ``hyps``: lists of integer sequences; ``uiv`` / ``hiv``: None, or lists of ``[len, 2]`` (begin,
end) arrays, one per utterance / stream."""
import itertools

import numpy as np

UNIT = 1 << 15


def _unpack(key):
    e = (int(key) + UNIT - 1) >> 15
    return e, e * UNIT - int(key)


def pair_key(ref, hyp, riv=None, hiv=None):
    """The key of dicow_edit_distance for one pair, by the full table."""
    m, n = len(ref), len(hyp)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        D[0][j] = j * UNIT
    for i in range(1, m + 1):
        D[i][0] = i * UNIT
        for j in range(1, n + 1):
            best = min(D[i - 1][j], D[i][j - 1]) + UNIT
            if riv is None or (riv[i - 1][0] < hiv[j - 1][1] and hiv[j - 1][0] < riv[i - 1][1]):
                best = min(best, D[i - 1][j - 1] + (-1 if ref[i - 1] == hyp[j - 1] else UNIT))
            D[i][j] = best
    return D[m][n]


def assignment_key(assignment, utts, hyps, uiv=None, hiv=None):
    """The summed key of one assignment (a stream index per utterance); with no stream: every reference word deleted."""
    if not hyps:
        return sum(len(u) for u in utts) * UNIT
    total = 0
    for h, hyp in enumerate(hyps):
        ref = [int(w) for u, a in zip(utts, assignment) if a == h for w in u]
        riv = None if uiv is None else [tuple(iv) for u, a in zip(uiv, assignment) if a == h for iv in np.asarray(u).reshape(-1, 2).tolist()]
        total += pair_key(ref, [int(w) for w in hyp], riv, None if hiv is None else np.asarray(hiv[h]).reshape(-1, 2).tolist())
    return total


def orc_brute(utts, hyps, uiv=None, hiv=None):
    if not hyps:
        return _unpack(assignment_key((), utts, hyps))
    return _unpack(min(assignment_key(a, utts, hyps, uiv, hiv) for a in itertools.product(range(len(hyps)), repeat=len(utts))))


def orc_dp(utts, hyps, uiv=None, hiv=None):
    if not hyps:
        return _unpack(assignment_key((), utts, hyps))
    H = len(hyps)
    shape = tuple(len(h) + 1 for h in hyps)
    L = np.zeros(shape, np.int64)
    for ax, n in enumerate(shape):
        L += (np.arange(n, dtype=np.int64) * UNIT).reshape([-1 if a == ax else 1 for a in range(H)])
    for u, utt in enumerate(utts):
        if len(utt) == 0:
            continue
        new = None
        for ax in range(H):
            hyp = np.asarray(hyps[ax], np.int64)
            T = np.moveaxis(L, ax, 0).copy()                                   # [n_ax + 1, ...]: the axis in front
            for i, w in enumerate(utt):
                cost = np.where(hyp == int(w), -1, UNIT).astype(np.int64)
                if uiv is not None:
                    rb, re = (int(v) for v in np.asarray(uiv[u]).reshape(-1, 2)[i])
                    hv = np.asarray(hiv[ax], np.int64).reshape(-1, 2)
                    open_ = (rb < hv[:, 1]) & (hv[:, 0] < re)
                else:
                    open_ = np.ones(len(hyp), bool)
                # a[j] = min(old[j] + UNIT, old[j-1] + cost) and new[j] = min(a[j], new[j-1] + UNIT): with j * UNIT taken off, a running minimum
                a = T + UNIT
                col = (-1,) + (1,) * (H - 1)                                   # a vector along the axis in front
                diag = T[:-1] + cost.reshape(col)
                a[1:] = np.where(open_.reshape(col), np.minimum(a[1:], diag), a[1:])
                ramp = (np.arange(T.shape[0], dtype=np.int64) * UNIT).reshape(col)
                T = np.minimum.accumulate(a - ramp, axis=0) + ramp
            T = np.moveaxis(T, 0, ax)
            new = T if new is None else np.minimum(new, T)
        L = new
    return _unpack(L[tuple(n - 1 for n in shape)])


def random_case(rng, max_streams=3, max_utts=5, max_words=5, alphabet=4, timed=False):
    """One seeded case of the host and GPU tests: (utts, hyps, uiv, hiv)."""
    H, U = int(rng.integers(1, max_streams + 1)), int(rng.integers(1, max_utts + 1))
    utts = [rng.integers(0, alphabet, int(rng.integers(0, max_words + 1))) for _ in range(U)]
    hyps = [rng.integers(0, alphabet, int(rng.integers(0, max_words + 1))) for _ in range(H)]
    if not timed:
        return utts, hyps, None, None

    def ivs(seq):
        b = rng.integers(0, 12, len(seq))
        return np.stack([b, b + rng.integers(0, 6, len(seq))], axis=1).astype(np.int64).reshape(-1, 2)
    return utts, hyps, [ivs(u) for u in utts], [ivs(h) for h in hyps]


def seeded_cases(n=60, seed=2024):
    """The 60 brute-force cases: H <= 3, U <= 5, at most 5 words each, an alphabet of 4, every second one with intervals."""
    rng = np.random.default_rng(seed)
    return [random_case(rng, timed=bool(k % 2)) for k in range(n)]

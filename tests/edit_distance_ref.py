"""Oracles for tests/test_host_scoring.py and tests/test_gpu_scoring.py: the definition of dicow_edit_distance as a plain triple loop,
a numpy restatement of it for long inputs, the S / D / I identities, the pseudo-word timing of tcpWER, and a brute-force cpWER.

The definition: unit costs; cell (i, j) may take the diagonal step (a hit if ref[i] == hyp[j], a substitution otherwise) only without
intervals or when rb < he and hb < re; among the alignments with the fewest errors the one with the most hits: the lexicographic minimum
of the additive key (errors, -hits)."""
import itertools

import numpy as np

UNIT = 1 << 32                                 # the packed key of the numpy restatement: errors * UNIT - hits
BIG = 1 << 60


def dp_loops(ref, hyp, riv=None, hiv=None):
    """(errors, hits) by the triple loop: rows, columns, the three steps; keys are Python tuples (errors, -hits)."""
    n, m = len(ref), len(hyp)
    D = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = (i + j, 0)
                continue
            steps = [(D[i - 1][j], (1, 0)), (D[i][j - 1], (1, 0))]
            if riv is None or (riv[i - 1][0] < hiv[j - 1][1] and hiv[j - 1][0] < riv[i - 1][1]):
                steps.append((D[i - 1][j - 1], (0, -1) if ref[i - 1] == hyp[j - 1] else (1, 0)))
            best = None
            for (e, h), (de, dh) in steps:
                cand = (e + de, h + dh)
                if best is None or cand < best:
                    best = cand
            D[i][j] = best
    return D[n][m][0], -D[n][m][1]


def dp_numpy(ref, hyp, riv=None, hiv=None):
    """The same, one row at a time on the packed int64 key.  The deletion and diagonal steps are elementwise; the insertion chain
    cur[j] = min_k (t[k] + (j - k) UNIT) is minimum.accumulate(t - j UNIT) + j UNIT."""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    n, m = len(ref), len(hyp)
    ramp = np.arange(m + 1, dtype=np.int64) * UNIT
    prev = ramp.copy()
    if riv is not None:
        riv, hiv = np.asarray(riv, np.int64).reshape(-1, 2), np.asarray(hiv, np.int64).reshape(-1, 2)
    for i in range(n):
        step = np.where(hyp == ref[i], -1, UNIT)
        if riv is not None:
            step = np.where((riv[i, 0] < hiv[:, 1]) & (hiv[:, 0] < riv[i, 1]), step, BIG)
        t = np.empty(m + 1, np.int64)
        t[0] = (i + 1) * UNIT
        t[1:] = np.minimum(prev[1:] + UNIT, prev[:-1] + step)
        prev = np.minimum.accumulate(t - ramp) + ramp
    key = int(prev[m])
    e = -(-key // UNIT)
    return e, e * UNIT - key


def sdi(e, h, n_ref, n_hyp):
    """(substitutions, deletions, insertions) from (errors, hits) and the lengths."""
    return n_ref + n_hyp - 2 * h - e, e + h - n_hyp, e - n_ref + h


def word_spans(start_s, end_s, words):
    """Reference-side pseudo-word timing in ticks of 1 ms: the segment's span split in proportion to the words' character counts,
    boundaries floored."""
    s, e = int(round(start_s * 1000)), int(round(end_s * 1000))
    total = sum(len(w) for w in words)
    bounds = [s + (e - s) * sum(len(w) for w in words[:k]) // total for k in range(len(words) + 1)]
    return [(bounds[k], bounds[k + 1]) for k in range(len(words))]


def word_points(start_s, end_s, words, collar_s):
    """Hypothesis side: the centre of each such span, widened by the collar on both sides."""
    c = int(round(collar_s * 1000))
    return [((b + e) // 2 - c, (b + e) // 2 + c) for b, e in word_spans(start_s, end_s, words)]


def streams(segments, timing=None):
    """{speaker: (words, intervals)} of (speaker, start_s, end_s, text) tuples: segments by start time, words concatenated."""
    out = {}
    for spk, start, end, text in sorted(segments, key=lambda s: s[1]):
        words, ivs = out.setdefault(spk, ([], []))
        w = text.split()
        words += w
        if timing is not None:
            ivs += timing(start, end, w)
    return out


def brute_assignment(cost):
    """(minimal total, every permutation that reaches it) of a square matrix."""
    cost = np.asarray(cost)
    n = cost.shape[0]
    best, argbest = None, []
    for perm in itertools.permutations(range(n)):
        tot = int(sum(cost[i, perm[i]] for i in range(n)))
        if best is None or tot < best:
            best, argbest = tot, [perm]
        elif tot == best:
            argbest.append(perm)
    return best, argbest


def brute_cp(ref_segments, hyp_segments, collar_s=None):
    """cpWER (collar_s None) or tcpWER by trying every permutation: (errors, length, [assignments that reach it]); an assignment is a
    list of (ref speaker | None, hyp speaker | None)."""
    timed = collar_s is not None
    ref = streams(ref_segments, word_spans if timed else None)
    hyp = streams(hyp_segments, (lambda s, e, w: word_points(s, e, w, collar_s)) if timed else None)
    rk, hk = sorted(ref, key=str), sorted(hyp, key=str)
    n = max(len(rk), len(hk))
    cost = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            rw, riv = ref[rk[i]] if i < len(rk) else ([], [])
            hw, hiv = hyp[hk[j]] if j < len(hk) else ([], [])
            ids = {w: k for k, w in enumerate(dict.fromkeys(rw + hw))}
            cost[i, j] = dp_numpy([ids[w] for w in rw], [ids[w] for w in hw], riv if timed else None, hiv if timed else None)[0]
    best, perms = brute_assignment(cost)
    assignments = [[(rk[i] if i < len(rk) else None, hk[p[i]] if p[i] < len(hk) else None) for i in range(n)] for p in perms]
    return best, sum(len(ref[k][0]) for k in rk), assignments

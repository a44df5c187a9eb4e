"""Two independent oracles for dicow_diar_score and the diarization metrics built on it, in plain numpy and Python.

  * dense:  per-tick boolean masks [S, n] (n <= 200 000), the unscored mask, and the definitions of include/dicow_hip.h taken literally;
  * sweep:  Python integers over the sorted distinct endpoints, for coordinates no mask can hold.

A table is a triple ``(bounds int64 [E + 1], active uint64 [E], S)``; ``unscored`` an int [n, 2] array of half-open intervals.  Both return
``{"C": int64 [Sr, Sh], "R": [Sr], "H": [Sh], "scored", "total", "missed", "false_alarm", "matched"}`` in ticks.  The metrics' formulas are
restated here on their own (``best_correct`` by brute force over all assignments), not imported from the package."""
import bisect
import itertools

import numpy as np

SCALARS = ("scored", "total", "missed", "false_alarm", "matched")
DENSE_MAX = 200000


def table_of(segs):
    return (segs.bounds, segs.active, segs.S)


def masks(table, n):
    bounds, active, S = table
    m = np.zeros((S, n), bool)
    for e in range(len(active)):
        a, b = int(bounds[e]), int(bounds[e + 1])
        assert 0 <= a < b <= n, (a, b, n)
        for s in range(S):
            if (int(active[e]) >> s) & 1:
                m[s, a:b] = True
    return m


def extent(ref, hyp):
    pts = [int(t[0][i]) for t in (ref, hyp) if len(t[1]) for i in (0, -1)]
    return (min(pts), max(pts)) if pts else (0, 0)


def dense_counts(ref, hyp, unscored, skip_overlap, n):
    assert n <= DENSE_MAX
    r, h = masks(ref, n), masks(hyp, n)
    uns = np.zeros(n, bool)
    for a, b in np.asarray(unscored if unscored is not None else [], np.int64).reshape(-1, 2):
        uns[max(0, int(a)):min(n, int(b))] = True
    n_ref, n_hyp = r.sum(0).astype(np.int64), h.sum(0).astype(np.int64)
    scored = ~uns
    if skip_overlap:
        scored &= n_ref <= 1
    lo, hi = extent(ref, hyp)
    inside = np.zeros(n, bool)
    inside[lo:hi] = True
    rs, hs = (r & scored).astype(np.int64), (h & scored).astype(np.int64)
    return {"C": rs @ hs.T, "R": rs.sum(1), "H": hs.sum(1), "scored": int((scored & inside).sum()), "total": int(n_ref[scored].sum()),
            "missed": int(np.maximum(n_ref - n_hyp, 0)[scored].sum()), "false_alarm": int(np.maximum(n_hyp - n_ref, 0)[scored].sum()),
            "matched": int(np.minimum(n_ref, n_hyp)[scored].sum())}


def sweep_counts(ref, hyp, unscored, skip_overlap):
    unscored = [(int(a), int(b)) for a, b in np.asarray(unscored if unscored is not None else [], np.int64).reshape(-1, 2)]
    pts = set()
    for bounds, active, _ in (ref, hyp):
        if len(active):
            pts.update(int(x) for x in bounds)
    for a, b in unscored:
        pts.update((a, b))
    pts = sorted(pts)
    lo, hi = extent(ref, hyp)
    Sr, Sh = ref[2], hyp[2]
    C = [[0] * Sh for _ in range(Sr)]
    R, H = [0] * Sr, [0] * Sh
    out = dict.fromkeys(SCALARS, 0)

    def bits(table, s):
        bounds, active, _ = table
        if not len(active):
            return 0
        q = bisect.bisect_right([int(x) for x in bounds], s)
        return int(active[q - 1]) if 1 <= q <= len(active) else 0

    for s, e in zip(pts[:-1], pts[1:]):
        dur = e - s
        if any(a <= s < b for a, b in unscored):
            continue
        rb, hb = bits(ref, s), bits(hyp, s)
        nr, nh = bin(rb).count("1"), bin(hb).count("1")
        if skip_overlap and nr > 1:
            continue
        if lo <= s < hi:
            out["scored"] += dur
        out["total"] += dur * nr
        out["missed"] += dur * max(0, nr - nh)
        out["false_alarm"] += dur * max(0, nh - nr)
        out["matched"] += dur * min(nr, nh)
        for i in range(Sr):
            if (rb >> i) & 1:
                R[i] += dur
                for j in range(Sh):
                    if (hb >> j) & 1:
                        C[i][j] += dur
        for j in range(Sh):
            if (hb >> j) & 1:
                H[j] += dur
    out.update(C=np.asarray(C, np.int64).reshape(Sr, Sh), R=np.asarray(R, np.int64), H=np.asarray(H, np.int64))
    return out


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("C", "R", "H")) and all(int(a[k]) == int(b[k]) for k in SCALARS)


def best_correct(C):
    """The largest sum of C[i][pi(i)] over all one-to-one assignments: brute force for up to 6 speakers a side, scipy above."""
    C = np.asarray(C, np.int64)
    Sr, Sh = C.shape
    if Sr == 0 or Sh == 0:
        return 0
    if max(Sr, Sh) <= 6:
        if Sr > Sh:
            C, Sr, Sh = C.T, Sh, Sr
        return max(sum(int(C[i, p[i]]) for i in range(Sr)) for p in itertools.permutations(range(Sh), Sr))
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(-C)
    return int(C[rows, cols].sum())


def der(counts, rate=16000):
    """pyannote's keys from the counts, with the brute-force maximum as `correct`."""
    correct = best_correct(counts["C"])
    conf = counts["matched"] - correct
    err, total = counts["missed"] + counts["false_alarm"] + conf, counts["total"]
    return {"total": total / rate, "correct": correct / rate, "missed detection": counts["missed"] / rate,
            "false alarm": counts["false_alarm"] / rate, "confusion": conf / rate,
            "diarization error rate": err / total if total else (0.0 if err == 0 else 1.0)}


def jer(counts, mapping):
    """mapping: {ref index: hyp index}.  The speakers in ascending order, as the package adds them (the float sum's order)."""
    err, n = 0.0, 0
    for i in range(len(counts["R"])):
        r = int(counts["R"][i])
        if r == 0:
            continue
        n += 1
        c = int(counts["C"][i][mapping[i]]) if i in mapping else 0
        if c > 0:
            h = int(counts["H"][mapping[i]])
            err += (r + h - 2 * c) / (r + h - c)
        else:
            err += 1.0
    return {"speaker error": err, "speaker count": n, "jaccard error rate": err / n if n else 0.0}


def random_table(rng, S, E, n, p_active=0.35, lo=0, top_bit=False):
    """A table with E entries on distinct positions of [lo, n]; every mask drawn bit by bit (silences included)."""
    if E == 0:
        return (np.zeros(1, np.int64), np.zeros(0, np.uint64), S)
    bounds = np.sort(rng.choice(np.arange(lo, n + 1), size=E + 1, replace=False)).astype(np.int64)
    on = rng.random((E, S)) < p_active
    if top_bit:
        on[::2, S - 1] = True
    active = np.zeros(E, np.uint64)
    for s in range(S):
        active |= np.where(on[:, s], np.uint64(1) << np.uint64(s), np.uint64(0))
    return (bounds, active, S)


def random_unscored(rng, k, n, width=40):
    """k sorted disjoint intervals inside [0, n]; neighbours may touch."""
    if k == 0:
        return np.zeros((0, 2), np.int64)
    cuts = np.sort(rng.choice(np.arange(0, n + 1), size=2 * k, replace=False)).astype(np.int64).reshape(k, 2)
    cuts[:, 1] = np.minimum(cuts[:, 1], cuts[:, 0] + width)
    if k > 1:
        cuts[0, 1] = cuts[1, 0]                                                # one touching pair
    return cuts

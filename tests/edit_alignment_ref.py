"""Oracle for tests/test_host_edit_alignment.py and tests/test_gpu_edit_alignment.py: the definition of dicow_edit_alignment in plain
Python.  The full table D of keys (errors, -hits) as Python tuples, as tests/edit_distance_ref.py::dp_loops builds it; then the walk back
from (N_ref, N_hyp): at each cell the first of
  1. the diagonal step, open only without intervals or when rb < he and hb < re: a hit (0) if the ids are equal, else a substitution (1),
  2. a deletion (2), from D[i-1][j],
  3. an insertion (3), from D[i][j-1]
that attains D[i][j]; on row or column 0 only one step is open.  And a checker that applies ops to ref and must obtain hyp."""
import numpy as np

HIT, SUB, DEL, INS = 0, 1, 2, 3


def _open(riv, hiv, i, j):
    return riv is None or (riv[i - 1][0] < hiv[j - 1][1] and hiv[j - 1][0] < riv[i - 1][1])


def table(ref, hyp, riv=None, hiv=None):
    """D[i][j] = (errors, -hits) of the first i reference and j hypothesis words."""
    n, m = len(ref), len(hyp)
    D = [[(i + j, 0) if i == 0 or j == 0 else None for j in range(m + 1)] for i in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            best = min((D[i - 1][j][0] + 1, D[i - 1][j][1]), (D[i][j - 1][0] + 1, D[i][j - 1][1]))
            if _open(riv, hiv, i, j):
                e, h = D[i - 1][j - 1]
                best = min(best, (e, h - 1) if ref[i - 1] == hyp[j - 1] else (e + 1, h))
            D[i][j] = best
    return D


def align(ref, hyp, riv=None, hiv=None):
    """((errors, hits), ops in forward order as a list of ints)."""
    ref, hyp = [int(v) for v in ref], [int(v) for v in hyp]
    if riv is not None:
        riv, hiv = np.asarray(riv).reshape(-1, 2).tolist(), np.asarray(hiv).reshape(-1, 2).tolist()
    D = table(ref, hyp, riv, hiv)
    i, j, ops = len(ref), len(hyp), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and _open(riv, hiv, i, j):
            e, h = D[i - 1][j - 1]
            eq = ref[i - 1] == hyp[j - 1]
            if ((e, h - 1) if eq else (e + 1, h)) == D[i][j]:
                ops.append(HIT if eq else SUB)
                i, j = i - 1, j - 1
                continue
        if i > 0 and (D[i - 1][j][0] + 1, D[i - 1][j][1]) == D[i][j]:
            ops.append(DEL)
            i -= 1
            continue
        assert j > 0 and (D[i][j - 1][0] + 1, D[i][j - 1][1]) == D[i][j]
        ops.append(INS)
        j -= 1
    return (D[len(ref)][len(hyp)][0], -D[len(ref)][len(hyp)][1]), ops[::-1]


def check_ops(ref, hyp, ops, riv=None, hiv=None):
    """Applies ops to ref and must obtain hyp: a hit copies an equal word, a substitution replaces a different one, a deletion drops a
    reference word, an insertion takes a hypothesis word; with intervals every diagonal op joins two overlapping ones.  Returns
    (errors, hits, substitutions, deletions, insertions) counted from the ops."""
    ref, hyp, ops = [int(v) for v in ref], [int(v) for v in hyp], [int(v) for v in ops]
    i, j, made = 0, 0, []
    for op in ops:
        assert op in (HIT, SUB, DEL, INS), op
        if op in (HIT, SUB):
            assert i < len(ref) and j < len(hyp) and (ref[i] == hyp[j]) == (op == HIT), (i, j, op)
            if riv is not None:
                assert riv[i][0] < hiv[j][1] and hiv[j][0] < riv[i][1], ("a diagonal step across intervals that do not overlap", i, j)
            made.append(hyp[j])
            i, j = i + 1, j + 1
        elif op == DEL:
            assert i < len(ref)
            i += 1
        else:
            assert j < len(hyp)
            made.append(hyp[j])
            j += 1
    assert i == len(ref) and j == len(hyp) and made == hyp
    c = [ops.count(k) for k in range(4)]
    return c[SUB] + c[DEL] + c[INS], c[HIT], c[SUB], c[DEL], c[INS]

"""The oracle of CTC forced alignment (csrc/ctc_align.hip, include/dicow_hip.h): the definition in plain Python, nothing of the library.

Problem: targets y[0..L) against F frames of scores x[f][c].  States s = 0 .. 2L, even = blank, odd = y[(s - 1) / 2]:
    v[0][0] = x[0][blank], v[0][1] = x[0][y[0]], every other v[0][s] = -inf
    v[f][s] = x[f][label(s)] + max(v[f-1][s], v[f-1][s-1], v[f-1][s-2] if s is odd and y[(s-1)/2] != y[(s-3)/2])
The tie rule: among equal maxima s beats s - 1 and s - 1 beats s - 2; at the last frame state 2L wins over 2L - 1 only if strictly greater;
L = 0 is the all-blank path, F = 0 with L = 0 the empty path of score 0.  Infeasible (status 1): the chosen end state is at -inf (too few
frames included), or F = 0 with L > 0.

  * ``align_scalar``   the definition literally, state by state, on any Python numbers: Python integers make it EXACT (scaled dyadic inputs),
                       floats make it fp64; ``NEG`` (float -inf) compares and adds correctly with both;
  * ``align``          the same vectorised over the states with numpy, for the large cases: int64 (exact; ``NEG_INT`` stands for -inf) or
                       float64 scores [F, C];
  * ``collapse`` / ``check_path``   a path spells its targets;  ``rescore``  the fp64 total of a given path.
Results are dicts: status, score, path [F], spans [L][2], token_score [L] (the sum over the token's own frames in ascending order)."""
import numpy as np

NEG = float("-inf")
NEG_INT = -(1 << 50)                   # -inf of the int64 variant: far below any sum of 2^31 scores of 2^16


def _read_back(end, bp, em, F, L, y, blank, add):
    s, states = end, [0] * F
    for f in range(F - 1, -1, -1):
        states[f] = s
        if f > 0:
            s -= int(bp[f][s])
    path = [int(y[(s - 1) // 2]) if s & 1 else int(blank) for s in states]
    spans, token_score = [], []
    for j in range(L):
        own = [f for f in range(F) if states[f] == 2 * j + 1]
        assert own and own == list(range(own[0], own[-1] + 1))
        spans.append([own[0], own[-1] + 1])
        acc = em(own[0], 2 * j + 1)
        for f in own[1:]:
            acc = add(acc, em(f, 2 * j + 1))
        token_score.append(acc)
    return path, spans, token_score


def _infeasible(F, L):
    return dict(status=1, score=NEG, path=[-1] * F, spans=[[-1, -1]] * L, token_score=[0] * L)


def align_scalar(x, y, blank):
    """x: F rows of scores (Python ints: exact; floats: fp64; NEG = -inf in both), y: the targets."""
    F, L = len(x), len(y)
    if F == 0:
        return dict(status=0, score=0, path=[], spans=[], token_score=[]) if L == 0 else _infeasible(F, L)
    S = 2 * L + 1
    lab = [y[(s - 1) // 2] if s & 1 else blank for s in range(S)]
    v = [NEG] * S
    v[0] = x[0][blank]
    if L:
        v[1] = x[0][y[0]]
    bp = [[0] * S]
    for f in range(1, F):
        nv, row = [NEG] * S, [0] * S
        for s in range(S):
            best, code = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, code = v[s - 1], 1
            if s & 1 and s >= 3 and lab[s] != lab[s - 2] and v[s - 2] > best:
                best, code = v[s - 2], 2
            nv[s], row[s] = x[f][lab[s]] + best, code
        v = nv
        bp.append(row)
    end = 2 * L
    if L > 0 and not v[2 * L] > v[2 * L - 1]:
        end = 2 * L - 1
    if v[end] == NEG:
        return _infeasible(F, L)
    path, spans, ts = _read_back(end, bp, lambda f, s: x[f][lab[s]], F, L, y, blank, lambda a, b: a + b)
    return dict(status=0, score=v[end], path=path, spans=spans, token_score=ts)


def align(x, y, blank):
    """x: int64 [F, C] (exact; NEG_INT = -inf) or float64 [F, C]; y: the targets.  Scores come back as Python ints / floats (NEG for -inf)."""
    x = np.asarray(x)
    y = np.asarray(y, np.int64).reshape(-1)
    F, L = x.shape[0], len(y)
    exact = x.dtype.kind == "i"
    if F == 0:
        return dict(status=0, score=0, path=[], spans=[], token_score=[]) if L == 0 else _infeasible(F, L)
    neg = NEG_INT if exact else -np.inf
    S = 2 * L + 1
    lab = np.full(S, blank, np.int64)
    lab[1::2] = y
    skip = np.zeros(S, bool)
    skip[3::2] = y[1:] != y[:-1]
    em = x[:, lab].astype(np.int64 if exact else np.float64)

    def plus(a, b):
        return np.where((a <= neg) | (b <= neg), neg, a + b) if exact else a + b

    v = np.full(S, neg, em.dtype)
    v[0] = em[0, 0]
    if L:
        v[1] = em[0, 1]
    bp = np.zeros((F, S), np.int8)
    with np.errstate(invalid="ignore"):
        for f in range(1, F):
            best, code = v.copy(), bp[f]
            pad = np.concatenate([np.full(2, neg, v.dtype), v])
            p1, p2 = pad[1:S + 1], pad[:S]
            m = p1 > best
            best[m], code[m] = p1[m], 1
            m = skip & (p2 > best)
            best[m], code[m] = p2[m], 2
            v = plus(em[f], best)
    end = 2 * L
    if L > 0 and not v[2 * L] > v[2 * L - 1]:
        end = 2 * L - 1
    if v[end] <= neg:
        return _infeasible(F, L)
    conv = int if exact else float
    path, spans, ts = _read_back(end, bp, lambda f, s: conv(em[f, s]), F, L, y, blank, lambda a, b: a + b)
    return dict(status=0, score=conv(v[end]), path=path, spans=spans, token_score=ts)


def collapse(path, blank):
    """Merge consecutive repeats, drop the blanks (-1, the padding behind F, ends the path)."""
    out, last = [], None
    for t in path:
        t = int(t)
        if t < 0:
            break
        if t != last and t != blank:
            out.append(t)
        last = t
    return out


def check_path(path, y, blank):
    assert collapse(path, blank) == [int(t) for t in y], (collapse(path, blank), list(y))


def rescore(x, path):
    """The fp64 total of x along a path (x float64 [F, C])."""
    tot = 0.0
    for f, c in enumerate(path):
        tot += float(x[f][int(c)])
    return tot

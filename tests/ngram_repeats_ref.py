"""Plain-Python oracle of dicow_ngram_repeats: the definition of include/dicow_hip.h restated over ids, literally -- every run, every count and
every candidate is enumerated -- and a string front that mirrors hyp_cleanup.truncate_repeating_ngrams.  Nothing of the library is used."""


def cut(ids, fold, min_n=1, max_n=10, min_words=30, u=10, r=10):
    """One segment -> (keep, (n, i, count))."""
    W = len(ids)
    assert len(fold) == W and min_n >= 1 and u >= 1 and r >= 0
    if W < min_words:
        return W, (0, 0, 0)
    run = [0] * (W + 1)                                                   # run[i]: the maximal run of equal folded ids that starts at i
    for i in range(W - 1, -1, -1):
        run[i] = run[i + 1] + 1 if i + 1 < W and fold[i + 1] == fold[i] else 1
    candidates = []                                                       # (keep, rank of the rule, n, i, count); the least one is the answer
    if min_n == 1:
        for i in range(W - u + 1):
            if run[i] >= u:
                candidates.append((i + 1, 0, 1, i, run[i]))
                break
    for n in range(max(2, min_n), max_n + 1):
        occ = {}
        for j in range(W - n + 1):
            g = tuple(ids[j:j + n])
            occ[g] = occ.get(g, 0) + 1
        for i in range(W - n + 1):
            count = 0 if len(set(fold[i:i + n])) == 1 else occ[tuple(ids[i:i + n])]
            if count > r:
                candidates.append((i + n, 1, n, i, count))
    best = min(candidates, default=None)
    if best is None or best[0] >= W:
        return W, (0, 0, 0)
    return best[0], best[2:]


def word_ids(words):
    """Exact and folded ids of one word list (ids are only compared for equality)."""
    exact, folded = {}, {}
    return [exact.setdefault(w, len(exact)) for w in words], [folded.setdefault(w.lower(), len(folded)) for w in words]


def truncate(text, ngram_length=10, min_n=1, max_n=None, min_word_threshold=30, unigram_min_repeat=10, repeat_threshold=10):
    """One string -> (the string, cut or the very same, (n, i, count))."""
    words = text.split()
    ids, fold = word_ids(words)
    keep, reason = cut(ids, fold, min_n, ngram_length if max_n is None else max_n, min_word_threshold, unigram_min_repeat, repeat_threshold)
    return (text if keep >= len(words) else " ".join(words[:keep])), reason

"""dicow_repetition_rules (generation.repetition_rules) against transformers' RepetitionPenaltyLogitsProcessor followed by
NoRepeatNGramLogitsProcessor, run on the CPU on the same fp32 inputs.

Comparison: an entry that is neither in its row's history nor banned is BIT-EQUAL to the input; a banned entry is exactly -inf; a
penalised entry is within 2 ulp of the CPU value (the kernel performs one multiply or one divide per entry; a correctly rounded
divide and a multiply by the rounded reciprocal differ by at most that), with the sign of a zero and -inf kept exactly.  The scores
sit inside the guard bands of tests/util.py::guarded with ld > V: bands and columns >= V must keep the sentinel.

Ids outside [0, V) take part in the n-gram comparison by value and never index the scores.  HF's processors cannot index with them
either, so the reference for such rows is HF on a vocabulary widened on both sides (ids shifted, scores padded), cut back to V."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NGRAMS, PENALTIES = (1, 2, 3, 5), (1.3, 0.7)


@pytest.fixture(scope="module")
def pkg():
    import amd_pkg
    return amd_pkg.load()


def dev(t):
    return t.clone().to(DEV)                                      # (a copy whatever DEV is: the rules work in place)


def hf_reference(ids, scores, penalty, ngram):
    """ids int64 [rows, L], scores fp32 [rows, V] (CPU).  penalty None / ngram None: that processor is left out."""
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    V = scores.shape[1]
    lo = max(0, -int(ids.min()))
    width = lo + max(V, int(ids.max()) + 1)
    wide = torch.ones(scores.shape[0], width)
    wide[:, lo:lo + V] = scores
    shifted = ids + lo
    if penalty is not None:
        wide = RepetitionPenaltyLogitsProcessor(penalty=penalty)(shifted, wide)
    if ngram is not None:
        wide = NoRepeatNGramLogitsProcessor(ngram)(shifted, wide.clone())
    return wide[:, lo:lo + V].contiguous()


def ordered(x):
    """fp32 -> int64 keys whose difference is the distance in ulp (finite values; +0.0 and -0.0 share key 0)."""
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def compare(got, inp, ref, ids, what):
    """got / inp / ref fp32 [rows, V] on the CPU; ids int64 [rows, L]."""
    rows, V = inp.shape
    hist = torch.zeros(rows, V, dtype=torch.bool)
    for r in range(rows):
        ok = ids[r][(ids[r] >= 0) & (ids[r] < V)]
        hist[r, ok] = True
    assert not torch.isnan(ref).any()
    banned = torch.isneginf(ref) & ~torch.isneginf(inp)
    assert not (banned & ~hist).any(), what                      # (a banned token always follows an earlier n-gram: it is in the history)
    bits = lambda t: t.contiguous().view(torch.int32)            # noqa: E731
    free = ~hist
    assert torch.equal(bits(got)[free], bits(inp)[free]), f"{what}: an entry outside the history changed"
    assert torch.equal(bits(ref)[free], bits(inp)[free])
    assert bool(torch.isneginf(got[banned]).all()), f"{what}: a banned entry is not -inf"
    pen = hist & ~banned
    g, w = got[pen], ref[pen]
    exact = ~torch.isfinite(w) | (w == 0)
    assert torch.equal(bits(g)[exact], bits(w)[exact]), f"{what}: -inf or a signed zero not kept"
    ulp = (ordered(g[~exact]) - ordered(w[~exact])).abs()
    assert torch.isfinite(g[~exact]).all() and (ulp.numel() == 0 or int(ulp.max()) <= 2), f"{what}: {int(ulp.max())} ulp"
    return int(pen.sum()), int(banned.sum())


def make_case(rows, V, L, ngram, seed):
    """Histories over a small alphabet (many repeats and repeated n-grams) with the edge tokens planted, and scores with both signs,
    signed zeros and -inf on history and non-history columns."""
    g = torch.Generator().manual_seed(seed)
    A = min(V, 6)
    ids = torch.randint(0, A, (rows, L), generator=g)
    m = max(ngram - 1, 1)
    for r in range(rows):
        if L >= m + 3:                                            # the tail's n-gram once more, early, followed by a history token
            ids[r, 1:1 + m] = ids[r, L - m:]
        if L >= 8:
            ids[r, L // 2] = 0
            ids[r, L // 2 + 1] = V - 1
            ids[r, L // 2 - 1] = V + 3                            # skipped: never indexes the row
            ids[r, L // 2 - 2] = -2
    if rows > 1:
        ids[1, :] = V - 2 if V < 7 else 5                         # one token L times: penalised once; its n-grams overlap the tail
    if rows > 2 and L >= 2 * m + 4 and m >= 2:                    # an out-of-range id INSIDE the tail's n-gram and inside its earlier copy,
        ids[2, L - m] = V + 1                                     # and a different one in a second copy that must not match
        ids[2, 1:1 + m] = ids[2, L - m:]
        ids[2, 2 + m:2 + 2 * m] = ids[2, L - m:]
        ids[2, 2 + m] = -7
    sc = torch.randn(rows, V, generator=g) * 3.0
    for r in range(rows):
        seen = [int(t) for t in dict.fromkeys(ids[r].tolist()) if 0 <= t < V]
        for t, val in zip(seen, (-0.0, float("-inf"), 0.0)):
            sc[r, t] = val
        free = [v for v in range(V) if v not in seen][:3]
        for v, val in zip(free, (float("-inf"), -0.0, 0.0)):
            sc[r, v] = val
    return ids, sc


def run_guarded(ids, sc, penalty, ngram, ld):
    from tests.util import guarded
    from ts_asr_whisper_amd.generation import repetition_rules
    g = guarded(sc.shape, ld, torch.float32, device=DEV, init=sc, name="scores")
    out = repetition_rules(ids.to(DEV), g.view, penalty, ngram)
    assert out is g.view
    g.check()
    return g.view.cpu()


def lengths(ngram):
    return sorted({L for L in (1, ngram - 2, ngram - 1, ngram, 448) if L >= 1})


def combos(V):
    if V < 10000:                                                 # the full cross; at the real vocabulary every (n-gram size, length) once
        return [(L, n, p) for n in NGRAMS for L in lengths(n) for p in PENALTIES]
    return [(L, n, PENALTIES[(i + j) % 2]) for i, n in enumerate(NGRAMS) for j, L in enumerate(lengths(n))]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", [7, 520, 51866])
def test_repetition_rules_vs_transformers_processors(pkg, rows, V):
    n_pen = n_ban = 0
    for k, (L, ngram, penalty) in enumerate(combos(V)):
        ids, sc = make_case(rows, V, L, ngram, seed=1000 * V + 10 * k + rows)
        ref = hf_reference(ids, sc.clone(), penalty, ngram)
        got = run_guarded(ids, sc, penalty, ngram, ld=V + 6)
        a, b = compare(got, sc, ref, ids, f"rows {rows} V {V} L {L} ngram {ngram} penalty {penalty}")
        n_pen, n_ban = n_pen + a, n_ban + b
    assert n_pen > 0 and n_ban > 0


def test_each_rule_alone_and_crafted_histories(pkg):
    from ts_asr_whisper_amd.generation import repetition_rules
    V = 520
    # one token three times is penalised once: 4 / 2 = 2, not 0.5
    sc = torch.full((1, V), 4.0)
    got = repetition_rules(torch.tensor([[5, 5, 5]]), dev(sc), repetition_penalty=2.0).cpu()
    assert float(got[0, 5]) == 2.0 and int((got != 4.0).sum()) == 1
    # an n-gram whose earlier occurrence overlaps the tail: [7, 7, 7] with n-gram size 2 bans 7
    got = repetition_rules(torch.tensor([[7, 7, 7]]), dev(sc), no_repeat_ngram_size=2).cpu()
    assert float(got[0, 7]) == float("-inf") and int((got != 4.0).sum()) == 1
    # n-gram size 1 bans every history token, the edge tokens included, and skips ids outside [0, V)
    ids = torch.tensor([[0, V - 1, V, -1, 3, 2 ** 40, -2 ** 40]])
    got = repetition_rules(ids, dev(sc), no_repeat_ngram_size=1).cpu()
    assert sorted(torch.nonzero(torch.isneginf(got[0])).flatten().tolist()) == [0, 3, V - 1] and int((got != 4.0).sum()) == 3
    # each processor alone, and both, on the same random case against HF
    ids, base = make_case(3, V, 40, 3, seed=5)
    for penalty, ngram in ((1.3, None), (0.7, None), (None, 3), (None, 1), (1.3, 3), (1.0, 3), (1.3, 0)):
        ref = hf_reference(ids, base.clone(), None if penalty in (None, 1.0) else penalty, None if not ngram else ngram)
        got = run_guarded(ids, base, penalty, ngram, ld=V + 8)
        compare(got, base, ref, ids, f"penalty {penalty} ngram {ngram}")
    # a negative score is multiplied, a positive one divided, -0.0 is divided (stays -0.0), -inf stays
    sc = torch.tensor([[-2.0, 2.0, -0.0, float("-inf"), 0.0, 1.0, 1.0]])
    got = repetition_rules(torch.tensor([[0, 1, 2, 3, 4]]), dev(sc), repetition_penalty=1.3).cpu()
    want = torch.tensor([[-2.0 * 1.3, 2.0 / 1.3, -0.0, float("-inf"), 0.0, 1.0, 1.0]])
    assert (ordered(got[:, :2]) - ordered(want[:, :2])).abs().max() <= 2
    assert torch.equal(got[:, 2:].view(torch.int32), want[:, 2:].view(torch.int32))


def test_history_as_a_row_slice_of_a_wider_buffer(pkg):
    from ts_asr_whisper_amd.generation import repetition_rules
    V, L = 520, 23
    ids, sc = make_case(3, V, L, 3, seed=9)
    wide = torch.full((3, L + 9), 1, dtype=torch.long)             # (token 1 around the slice: reading outside it would penalise / ban it)
    wide[:, 4:4 + L] = ids
    view = wide.to(DEV)[:, 4:4 + L]
    assert view.stride(0) == L + 9 and not view.is_contiguous()
    got = repetition_rules(view, dev(sc), 1.3, 3).cpu()
    assert torch.equal(got.view(torch.int32), repetition_rules(ids.to(DEV), dev(sc), 1.3, 3).cpu().view(torch.int32))
    compare(got, sc, hf_reference(ids, sc.clone(), 1.3, 3), ids, "row slice")
    # a history that is not made of rows (a transposed view) is copied, not misread
    got_t = repetition_rules(ids.t().contiguous().to(DEV).t(), dev(sc), 1.3, 3).cpu()
    assert torch.equal(got_t.view(torch.int32), got.view(torch.int32))


def test_options_off_launch_nothing_and_runs_are_bit_equal(pkg, monkeypatch):
    from ts_asr_whisper_amd import _lib, generation
    ids, sc = make_case(3, 520, 30, 2, seed=3)
    a = run_guarded(ids, sc, 1.3, 2, ld=526)
    b = run_guarded(ids, sc, 1.3, 2, ld=526)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a.view(torch.int32), sc.view(torch.int32))

    def no_call(name, *args):
        raise AssertionError(f"{name} launched with both options off")
    monkeypatch.setattr(_lib, "call", no_call)
    for kw in (dict(), dict(repetition_penalty=None, no_repeat_ngram_size=None), dict(repetition_penalty=1.0, no_repeat_ngram_size=0)):
        on_dev = dev(sc)
        assert generation.repetition_rules(ids.to(DEV), on_dev, **kw) is on_dev
        assert torch.equal(on_dev.cpu().view(torch.int32), sc.view(torch.int32))


def test_bad_arguments_are_refused_by_the_library(pkg):
    from ts_asr_whisper_amd import _lib
    sc = torch.zeros(2, 16, device=DEV)
    ids = torch.zeros(2, 4, dtype=torch.long, device=DEV)
    good = [sc.data_ptr(), 16, 2, 16, ids.data_ptr(), 4, 4, 1.3, 2, _lib.stream()]
    for pos, bad in ((1, 15), (2, 0), (3, 0), (5, 3), (6, 0), (6, 8193), (7, 0.0), (7, -1.0), (0, None), (4, None)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(_lib.DicowError):
            _lib.call("dicow_repetition_rules", *args)
    torch.cuda.synchronize()
    assert int((sc != 0).sum()) == 0

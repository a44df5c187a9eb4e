"""dicow_sequence_bias (generation.sequence_bias_rules) against the plain-Python oracle of its definition (tests/sequence_bias_ref.py)
and against transformers' SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor run on CPU copies of the same fp32 inputs.

Comparison: an entry the oracle does not touch is BIT-EQUAL to the input, a touched one BIT-EQUAL to the oracle -- equality, not a ulp
bound: the kernel performs the same fp32 adds in the same order -- and the whole result equals transformers' as numbers (transformers
turns an untouched -0.0 into +0.0, the stated difference).  The scores sit inside the guard bands of tests/util.py::guarded with
ld > V: bands and columns >= V must keep the sentinel.  The history rows are slices of a wider id buffer that holds, outside the
slices, ids which WOULD complete sequences."""
import pytest
import torch

from tests import sequence_bias_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
V0 = 50


@pytest.fixture(scope="module")
def pkg():
    import amd_pkg
    return amd_pkg.load()


@pytest.fixture(scope="module")
def lib(pkg):
    from ts_asr_whisper_amd import _lib
    return _lib


def make_scores(rows, V, g):
    sc = torch.randn(rows, V, generator=g) * 3.0
    for r in range(rows):                                         # signed zeros and -inf, on every column over the rows
        sc[r, (3 * r) % V], sc[r, (3 * r + 1) % V], sc[r, (3 * r + 2) % V] = -0.0, 0.0, -INF
    return sc


def make_ids(rows, L, g, alphabet=4, V=V0):
    """Histories over a small alphabet (so that short sequences match by chance too), with ids outside [0, V) planted."""
    ids = torch.randint(0, alphabet, (rows, L), generator=g)
    for r in range(rows):
        if L >= 5 and r % 3 == 1:
            ids[r, L - 3] = -2 - r
        if L >= 5 and r % 3 == 2:
            ids[r, L - 2] = V + r
    return ids


def run(ids, sc, seqs, biases, plan=0, ld=None, pad=(3, 5)):
    """The kernel on guarded scores; the history rows as slices of a wider buffer filled with token 0 .. 3 garbage."""
    from tests.util import guarded
    from ts_asr_whisper_amd.generation import sequence_bias_rules, sequence_bias_table
    rows, V = sc.shape
    table = sequence_bias_table(seqs, biases, DEV)
    g = guarded(sc.shape, V + 6 if ld is None else ld, torch.float32, device=DEV, init=sc, name="scores")
    L = ids.shape[1]
    wide = (torch.arange(rows * (L + sum(pad))).reshape(rows, -1) % 4).to(torch.long)
    wide[:, pad[0]:pad[0] + L] = ids
    view = wide.to(DEV)[:, pad[0]:pad[0] + L]
    assert view.stride(0) == L + sum(pad)
    out = sequence_bias_rules(view, g.view, table, plan=plan)
    assert out is g.view
    torch.cuda.synchronize()
    g.check()
    return g.view.cpu()


def check(ids, sc, seqs, biases, what, plans=(0, 1, 2), hf=True):
    """Every plan against the oracle bit for bit; transformers as numbers.  Returns the number of touched entries."""
    ref, touched = R.reference(ids, sc, seqs, biases)
    for plan in plans:
        got = run(ids, sc, seqs, biases, plan)
        assert torch.equal(R.bits(got)[~touched], R.bits(sc)[~touched]), f"{what} plan {plan}: an entry no sequence heads changed"
        assert torch.equal(R.bits(got)[touched], R.bits(ref)[touched]), f"{what} plan {plan}: a touched entry differs from the oracle"
    if hf:
        assert R.same_numbers(ref, R.via_transformers(ids, sc, sequence_bias=dict(zip(seqs, biases)))), f"{what}: oracle != transformers"
    return int(touched.sum())


def tail_sequences(ids, m, V, g, n_random=6):
    """Sequences of length m around row 0's tail: the tail itself (matches when m <= L), the tail with its FIRST and with its LAST
    prefix token changed (the last and the first comparison fail), a single-token entry on the same last token, random ones."""
    L = ids.shape[1]
    t = int(torch.randint(0, V, (1,), generator=g))
    seqs = {}
    if m == 1:
        seqs[(t,)] = 1.25
    else:
        k = m - 1
        tail = ids[0, max(L - k, 0):].tolist()
        tail = [1] * (k - len(tail)) + tail                       # (L < m - 1: padded; it cannot match)
        tail = [x if 0 <= x < V else 2 for x in tail]             # (a planted out-of-range id is not a table token)
        seqs[tuple(tail) + (t,)] = 2.5
        seqs[tuple([(tail[0] + 1) % 4] + tail[1:]) + (t,)] = -1.75
        seqs[tuple(tail[:-1] + [(tail[-1] + 1) % 4]) + (t,)] = 0.5
        seqs[(t,)] = -0.375
    for _ in range(n_random):
        s = tuple(torch.randint(0, 4, (m - 1,), generator=g).tolist()) + (int(torch.randint(0, V, (1,), generator=g)),)
        seqs.setdefault(s, float(torch.randn((), generator=g)) if len(seqs) % 3 else -INF)
    return list(seqs), list(seqs.values())


@pytest.mark.parametrize("rows", [1, 3, 80])
def test_lengths_and_histories_around_every_length(pkg, lib, rows):
    """Sequence lengths 1, 2, 3 and the maximum; L = 1, m - 2, m - 1, m, m + 1: L = m - 1 is the 'longer than the context' rule with
    the whole history equal to the prefix (ignored), L = m the 'sequence is the whole history' case (matches)."""
    g = torch.Generator().manual_seed(100 + rows)
    touched = 0
    for m in (1, 2, 3, lib.SEQ_BIAS_MAX_LEN):
        for L in sorted({x for x in (1, m - 2, m - 1, m, m + 1) if x >= 1}):
            ids = make_ids(rows, L, g)
            seqs, biases = tail_sequences(ids, m, V0, g)
            sc = make_scores(rows, V0, g)
            touched += check(ids, sc, seqs, biases, f"rows {rows} m {m} L {L}")
            if m > 1:                                             # row 0 against its own tail: matched exactly when the history is long enough
                in_vocab = all(0 <= int(x) < V0 for x in ids[0, max(L - m + 1, 0):])
                assert R.matches(seqs[0], ids[0].tolist()) == (L >= m and in_vocab), (m, L)
    assert touched > 0


@pytest.mark.parametrize("V", [V0, 1200])
def test_table_sizes_around_the_wave_and_workgroup_steps(pkg, V):
    """n_seq = 1, 63, 64, 65, 255, 256, 257, 1025.  At V = 50 the groups grow with the table (about 20 sequences each at 1025); at
    V = 1200 the groups stay short and their number passes the 256 a lane-plan workgroup holds and the 4 a wave-plan workgroup holds."""
    g = torch.Generator().manual_seed(7 + V)
    rows = 3
    ids = make_ids(rows, 6, g, V=V)
    for n_seq in (1, 63, 64, 65, 255, 256, 257, 1025):
        seqs = {}
        while len(seqs) < n_seq:
            m = int(torch.randint(1, 4, (1,), generator=g))
            s = tuple(torch.randint(0, 4, (m - 1,), generator=g).tolist()) + (int(torch.randint(0, V, (1,), generator=g)),)
            seqs.setdefault(s, float(torch.randn((), generator=g)) * 10.0 ** int(torch.randint(-2, 5, (1,), generator=g)))
        sc = make_scores(rows, V, g)
        touched = check(ids, sc, list(seqs), list(seqs.values()), f"V {V} n_seq {n_seq}")
        assert touched > 0 or n_seq == 1                          # (a lone random sequence need not match)


def test_one_group_of_300_sequences_crosses_a_wave(pkg):
    """300 sequences with ONE last token: every binary prefix of 1 .. 7 tokens (254) and 46 of 8 tokens.  A row matches one sequence of
    each length, spread over the group's five 64-sequence steps; 80 binary histories match most of the 300 between them.  The biases
    span seven orders of magnitude, so the order of the adds shows in the bits."""
    g = torch.Generator().manual_seed(300)
    v, rows, L = 17, 80, 10
    prefixes = [tuple((k >> i) & 1 for i in range(n)) for n in range(1, 9) for k in range(2 ** n)][:300]
    order = torch.randperm(300, generator=g).tolist()             # (the caller's order: lengths interleaved)
    seqs = [prefixes[i] + (v,) for i in order]
    biases = [float(torch.randn((), generator=g)) * 10.0 ** int(torch.randint(-3, 5, (1,), generator=g)) for _ in seqs]
    ids = torch.randint(0, 2, (rows, L), generator=g)
    sc = make_scores(rows, V0, g)
    check(ids, sc, seqs, biases, "group of 300")
    matched = {i for r in range(rows) for i, s in enumerate(seqs) if R.matches(s, ids[r].tolist())}
    assert len(matched) > 150                                     # "most of them"
    ref, touched = R.reference(ids, sc, seqs, biases)
    assert int(touched.sum()) == rows and bool(touched[:, v].all())
    # the order matters on this case: the same matches added in reversed table order give other bits somewhere
    rev, _ = R.reference(ids, sc, seqs[::-1], biases[::-1])
    assert not torch.equal(R.bits(rev), R.bits(ref))


def test_order_case_follows_transformers(pkg):
    """1e8, -1e8 and 1.0 on three matching sequences of one last token: 1.0 or 0.0 in fp32, depending on the order of the adds."""
    ids = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]])
    sc = torch.zeros(2, V0)
    for seqs, want in (({(3, 5): 1e8, (2, 3, 5): -1e8, (1, 2, 3, 5): 1.0}, 1.0),
                       ({(1, 2, 3, 5): 1.0, (3, 5): 1e8, (2, 3, 5): -1e8}, 0.0),
                       ({(3, 5): 1e8, (2, 3, 5): -1e8, (5,): 1.0}, 0.0),            # the single-token entry is added first
                       ({(5,): 1e8, (3, 5): -1e8, (2, 3, 5): 1.0}, 1.0)):
        hf = R.via_transformers(ids, sc, sequence_bias=seqs)
        assert float(hf[0, 5]) == want
        for plan in (0, 1, 2):
            got = run(ids, sc, list(seqs), list(seqs.values()), plan)
            assert float(got[0, 5]) == want, (seqs, plan)
            assert R.same_numbers(got, hf)


def test_infinities_zeros_and_ids_outside_the_vocabulary(pkg):
    V = V0
    #            0     1     2     3     4    5     6
    base = [-INF, -0.0, 0.0, 1.5, -INF, -0.0, 0.0] + [2.0] * (V - 7)
    sc = torch.tensor([base, base])
    ids = torch.tensor([[9, 8], [9, 7]])
    seqs = {(0,): -INF, (1,): -INF, (2,): -INF, (8, 3): -INF, (9, 8, 3): -INF,      # -inf onto -inf, -0.0, +0.0; -inf + -inf onto 1.5
            (5,): -0.0, (6,): -0.0, (8, 4): 3.0, (7, 10): 0.0}                      # b = +0.0 + -0.0 = +0.0, so a touched -0.0 ends +0.0; -inf + 3 = -inf
    check(ids, sc, list(seqs), list(seqs.values()), "inf / zero")
    got = run(ids, sc, list(seqs), list(seqs.values()))
    assert got[0, :5].tolist() == [-INF] * 5 and got[1, :3].tolist() == [-INF] * 3 and float(got[1, 3]) == 1.5
    assert R.bits(got[0, 5:7]).tolist() == [0, 0] and R.bits(got[0, 1:3]).tolist() == R.bits(torch.tensor([-INF, -INF])).tolist()
    assert float(got[1, 10]) == 2.0 and float(got[0, 10]) == 2.0
    # banned words through transformers' own class, eos filtered
    words = [[0], [8, 3], [9, 8, 3], [7]]
    from ts_asr_whisper_amd.generation import sequence_bias_options
    o = sequence_bias_options(bad_words_ids=words, eos_token_id=7, vocab_size=V)[1]
    got = run(ids, sc, *o)
    assert R.same_numbers(got, R.via_transformers(ids, sc, bad_words_ids=words, eos_token_id=7)) and float(got[0, 7]) == 2.0
    # history ids negative, >= V and far outside int32: compared by value, so they match no table token and index nothing
    big = 2 ** 32 + 3                                              # (its low 32 bits are token 3)
    ids = torch.tensor([[0, 3, 4], [0, big, 4], [0, -1, 4], [0, V, 4], [0, V + 3, 4], [0, -2 ** 40, 4]])
    sc = torch.zeros(6, V)
    seqs = {(3, 4, 6): 1.0, (4, 6): 0.5, (3, 4, 7): 2.0}
    got = run(ids, sc, list(seqs), list(seqs.values()))
    assert got[:, 6].tolist() == [1.5] + [0.5] * 5 and got[:, 7].tolist() == [2.0] + [0.0] * 5
    check(ids, sc, list(seqs), list(seqs.values()), "ids outside the vocabulary")


def test_a_row_alone_equals_the_row_among_others_and_runs_repeat(pkg):
    g = torch.Generator().manual_seed(11)
    ids = make_ids(80, 9, g)
    sc = make_scores(80, V0, g)
    seqs, biases = tail_sequences(ids, 3, V0, g, n_random=120)
    full = run(ids, sc, seqs, biases)
    assert torch.equal(R.bits(full), R.bits(run(ids, sc, seqs, biases)))
    assert not torch.equal(R.bits(full), R.bits(sc))
    for r in (0, 41, 79):
        for plan in (1, 2):
            alone = run(ids[r:r + 1], sc[r:r + 1], seqs, biases, plan)
            assert torch.equal(R.bits(alone[0]), R.bits(full[r])), (r, plan)


def test_graph_capture_and_two_replays_with_changed_histories(pkg):
    from ts_asr_whisper_amd.generation import sequence_bias_rules, sequence_bias_table
    g = torch.Generator().manual_seed(5)
    rows, L = 3, 6
    hists = [make_ids(rows, L, g) for _ in range(3)]
    seqs, biases = tail_sequences(hists[1], 3, V0, g, n_random=40)
    seqs2, biases2 = tail_sequences(hists[2], 2, V0, g, n_random=0)
    extra = {s: b for s, b in zip(seqs2, biases2) if s not in seqs}
    seqs, biases = seqs + list(extra), biases + list(extra.values())
    for plan in (1, 2):
        table = sequence_bias_table(seqs, biases, DEV)
        base = make_scores(rows, V0, g)
        sc, ids = base.to(DEV), hists[0].to(DEV)
        sequence_bias_rules(ids, sc, table, plan=plan)             # (code objects load outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sequence_bias_rules(ids, sc, table, plan=plan)
        for h in hists[1:]:
            sc.copy_(base)
            ids.copy_(h)                                          # in place: the graph holds the addresses
            graph.replay()
            torch.cuda.synchronize()
            ref, touched = R.reference(h, base, seqs, biases)
            assert touched.any() and torch.equal(R.bits(sc.cpu()), R.bits(ref))


def test_empty_table_launches_nothing(pkg, monkeypatch):
    from ts_asr_whisper_amd import _lib, generation
    sc = make_scores(3, V0, torch.Generator().manual_seed(1))
    ids = torch.zeros(3, 4, dtype=torch.long, device=DEV)
    empty = generation.sequence_bias_table([], [], DEV)
    rc = _lib.lib().dicow_sequence_bias(sc.to(DEV).data_ptr(), V0, 3, V0, ids.data_ptr(), 4, 4, None, 0, 0, 0, 0, 0, 0, _lib.stream())
    assert rc == 0                                                # the library itself: n_seq == 0 returns before any launch

    def no_call(name, *args):
        raise AssertionError(f"{name} launched with an empty table")
    monkeypatch.setattr(_lib, "call", no_call)
    for table in (None, empty):
        on_dev = sc.to(DEV)
        assert generation.sequence_bias_rules(ids, on_dev, table) is on_dev
        assert torch.equal(R.bits(on_dev.cpu()), R.bits(sc))


def test_bad_arguments_are_refused(pkg):
    from ts_asr_whisper_amd import _lib, generation
    sc = torch.zeros(2, 16, device=DEV)
    ids = torch.zeros(2, 4, dtype=torch.long, device=DEV)
    t = generation.sequence_bias_table([(0, 1), (2,), (3, 1)], [1.0, 2.0, 3.0], DEV)
    good = [sc.data_ptr(), 16, 2, 16, ids.data_ptr(), 4, 4, t.buf.data_ptr(), t.n_seq, t.n_groups, t.n_tokens, t.max_len, t.max_group, 0,
            _lib.stream()]
    for pos, bad in ((0, None), (1, 15), (2, 0), (3, 0), (4, None), (5, 3), (6, 0), (6, _lib.SEQ_BIAS_MAX_L + 1), (7, None),
                     (8, _lib.SEQ_BIAS_MAX_SEQ + 1), (8, -1), (9, 0), (9, 4), (10, 2), (10, 3 * 2 + 1), (11, 0),
                     (11, _lib.SEQ_BIAS_MAX_LEN + 1), (12, 0), (12, 4), (13, -1), (13, _lib.SEQ_BIAS_PLANS + 1)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(_lib.DicowError):
            _lib.call("dicow_sequence_bias", *args)
    torch.cuda.synchronize()
    assert int((sc != 0).sum()) == 0
    # the wrapper: a table for a wider vocabulary raises transformers' vocabulary error; a table on another device is refused
    wide = generation.sequence_bias_table([(0, 16)], [1.0], DEV)
    with pytest.raises(ValueError, match="vocabulary size is 16"):
        generation.sequence_bias_rules(ids, sc, wide)
    with pytest.raises(_lib.DicowError):
        generation.sequence_bias_rules(ids, sc, generation.sequence_bias_table([(0, 1)], [1.0], "cpu"))
    with pytest.raises(_lib.DicowError):
        generation.sequence_bias_rules(ids[:1], sc, t)
    assert int((sc != 0).sum()) == 0

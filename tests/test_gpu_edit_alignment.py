"""dicow_edit_alignment (csrc/edit_alignment.hip) and the alignment layer of the scoring module on the GPU against the oracle of
tests/edit_alignment_ref.py.  Every comparison is EXACT equality of ops, spans and (errors, hits).  Every launch made through `run` reads
flat buffers in which a sentinel id that occurs nowhere else (with an interval that overlaps everything) stands around every span, writes
ops into a buffer pre-filled with a sentinel byte that must survive outside every [first, first + length) and in a band behind the last
slot, and gets a workspace one byte larger than asked for whose last byte must survive.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import edit_alignment_ref as A

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, scoring  # noqa: E402

K, NARROW, WIDE = L.EDIT_K, L.EDIT_LANES_NARROW, L.EDIT_LANES
SENTINEL_ID, SENTINEL_IV, SENTINEL_OP, SENTINEL_WS, BAND = -7, (-10 ** 9, 10 ** 9), 0xAA, 0x5C, 256
CONFIGS = [(NARROW, 1), (NARROW, 2), (WIDE, 1), (WIDE, 2)]                # (lanes, along)

_WANT = {}


def want(ref, hyp, riv=None, hiv=None):
    """The oracle's ((errors, hits), ops), computed once per distinct input."""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    key = (ref.tobytes(), hyp.tobytes(), None if riv is None else np.asarray(riv, np.int64).tobytes(),
           None if hiv is None else np.asarray(hiv, np.int64).tobytes())
    if key not in _WANT:
        _WANT[key] = A.align(ref, hyp, riv, hiv)
    return _WANT[key]


class Packed:
    """Sequences (and their intervals) in one flat buffer, a sentinel before, between and behind them."""

    def __init__(self, seqs, ivs=None):
        ids, iv, self.starts, self.lens = [SENTINEL_ID], [SENTINEL_IV], [], []
        for k, s in enumerate(seqs):
            self.starts.append(len(ids))
            self.lens.append(len(s))
            ids += [int(v) for v in s] + [SENTINEL_ID]
            iv += ([tuple(x) for x in np.asarray(ivs[k]).reshape(-1, 2).tolist()] if ivs is not None else [(0, 0)] * len(s)) + [SENTINEL_IV]
        self.ids = torch.tensor(ids, dtype=torch.int32).cuda()
        self.iv = torch.tensor(iv, dtype=torch.int32).reshape(-1, 2).cuda() if ivs is not None else None


class Buffers:
    def __init__(self, table, lanes, along):
        n = table.shape[0]
        self.nbytes = L.lib().dicow_edit_alignment_ws_bytes(table.ctypes.data if n else None, n, lanes, along)
        assert self.nbytes >= L.ALIGN_TABLE_BYTES * n and self.nbytes % 8 == 0
        self.total = int(table[:, 1].sum() + table[:, 3].sum())
        self.out = torch.full((max(n, 1), 2), -1, dtype=torch.int32, device="cuda")
        self.ops = torch.full((self.total + BAND,), SENTINEL_OP, dtype=torch.uint8, device="cuda")
        self.spans = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
        self.ws = torch.full((self.nbytes + 8,), SENTINEL_WS, dtype=torch.uint8, device="cuda")       # one byte more than asked for, and 7

    def launch(self, rp, hp, table, lanes, along):
        """The C entry point on the current stream; nothing else (capturable)."""
        n = table.shape[0]
        L.call("dicow_edit_alignment", rp.ids.data_ptr(), rp.ids.numel(), hp.ids.data_ptr(), hp.ids.numel(), L.ptr(rp.iv), L.ptr(hp.iv),
               table.ctypes.data if n else None, n, self.out.data_ptr(), self.ops.data_ptr(), self.spans.data_ptr(), lanes, along,
               self.ws.data_ptr(), self.nbytes, L.stream())

    def result(self, table):
        """[((errors, hits), ops)] per pair, after checking the spans, the sentinels of ops and the byte behind the workspace."""
        torch.cuda.synchronize()
        n = table.shape[0]
        out, ops, spans = self.out.cpu().numpy(), self.ops.cpu().numpy(), self.spans.cpu().numpy()
        assert (self.ws[self.nbytes:].cpu().numpy() == SENTINEL_WS).all(), "the byte behind the workspace was written"
        written = np.zeros(len(ops), bool)
        ends = np.cumsum(table[:, 1] + table[:, 3])
        got = []
        for k in range(n):
            first, length = int(spans[k, 0]), int(spans[k, 1])
            assert ends[k] - (table[k, 1] + table[k, 3]) <= first and first + length <= ends[k], ("the path leaves the pair's slot", k)
            written[first:first + length] = True
            got.append(((int(out[k, 0]), int(out[k, 1])), ops[first:first + length].tolist()))
        assert (ops[~written] == SENTINEL_OP).all(), "ops written outside every [first, first + length)"
        assert (ops[written] <= 3).all()
        return got


def run_table(rp, hp, table, lanes=0, along=0):
    table = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1, 4))
    b = Buffers(table, lanes, along)
    b.launch(rp, hp, table, lanes, along)
    return b.result(table)


def run(rp, hp, pairs, lanes=0, along=0):
    """pairs: (index into rp's sequences, index into hp's)."""
    return run_table(rp, hp, [(rp.starts[i], rp.lens[i], hp.starts[j], hp.lens[j]) for i, j in pairs], lanes, along)


def check_all_configs(refs, hyps, ivr=None, ivh=None):
    """Pair k = (refs[k], hyps[k]) in one call per configuration: the oracle's result under every (lanes, along)."""
    rp, hp = Packed(refs, ivr), Packed(hyps, ivh)
    pairs = [(k, k) for k in range(len(refs))]
    exp = [want(refs[k], hyps[k], None if ivr is None else ivr[k], None if ivh is None else ivh[k]) for k in range(len(refs))]
    for lanes, along in CONFIGS + [(0, 0)]:
        got = run(rp, hp, pairs, lanes, along)
        bad = [(len(refs[k]), len(hyps[k])) for k in range(len(refs)) if got[k] != exp[k]]
        assert not bad, (lanes, along, bad[:8])
    return exp


# (ref_len, hyp_len): the empty sides; the strip's edge (K = 8) on either side; as many lanes as rows, one more and fewer (3 strips
# against 2, 3 and 4 rows); the narrow panel's edge (64 lanes x 8) and a second narrow panel under 40 rows; the wide panel's edge
SEAMS = [(0, 0), (0, 5), (5, 0), (1, 1), (K - 1, 3), (K, 3), (K + 1, 3), (3, K - 1), (3, K), (3, K + 1), (2 * K + 3, 2), (2 * K + 3, 3),
         (2 * K + 3, 4), (NARROW * K - 1, 5), (NARROW * K, 5), (NARROW * K + 1, 5), (NARROW * K + 1, 40), (40, NARROW * K + 1),
         (WIDE * K - 1, 3), (WIDE * K, 3), (WIDE * K + 1, 3)]


@pytest.mark.parametrize("alphabet", [2, 3, 50])
def test_lengths_around_the_seams(alphabet):
    rng = np.random.default_rng(100 + alphabet)
    refs = [rng.integers(0, alphabet, a) for a, _ in SEAMS]
    hyps = [rng.integers(0, alphabet, b) for _, b in SEAMS]
    exp = check_all_configs(refs, hyps)
    assert exp[0] == ((0, 0), []) and exp[1] == ((5, 0), [A.INS] * 5) and exp[2] == ((5, 0), [A.DEL] * 5)
    for k in range(len(SEAMS)):
        A.check_ops(refs[k], hyps[k], exp[k][1])


def test_the_64_bit_key_next_to_small_pairs():
    """61 500 + 3 words are past the int32 key's range (65535 - 4096), which makes the whole call int64."""
    rng = np.random.default_rng(110)
    lens = [(61500, 3), (5, 7), (0, 3), (9, 9), (3, 700)]
    refs, hyps = [rng.integers(0, 3, a) for a, _ in lens], [rng.integers(0, 3, b) for _, b in lens]
    exp = check_all_configs(refs, hyps)
    assert len(exp[0][1]) >= 61500 and exp[0][0][0] >= 61497


def _tick_intervals(rng, n, span):
    """Begins and widths on a coarse grid of ticks, so that intervals touch exactly all the time; zero widths included."""
    b = rng.integers(0, span, n) * 5
    return np.stack([b, b + rng.integers(0, 4, n) * 5], axis=1)


def test_intervals_close_the_diagonal():
    rng = np.random.default_rng(120)
    lens = [(1, 1), (5, 9), (K + 1, 70), (70, K + 1), (300, NARROW * K + 1), (130, 120), (0, 4)]
    refs, hyps = [rng.integers(0, 3, a) for a, _ in lens], [rng.integers(0, 3, b) for _, b in lens]
    ivr = [_tick_intervals(rng, a, max(a // 4, 2)) for a, _ in lens]
    ivh = [_tick_intervals(rng, b, max(b // 4, 2)) for _, b in lens]
    touching = sum(int((r[:, None, 0] == h[None, :, 1]).sum()) for r, h in zip(ivr, ivh))
    assert touching > 100                                                    # rb == he: closed
    exp = check_all_configs(refs, hyps, ivr, ivh)
    diagonal = 0
    for k in range(len(lens)):
        c = A.check_ops(refs[k], hyps[k], exp[k][1], ivr[k].tolist(), ivh[k].tolist())      # every diagonal op joins overlapping intervals
        diagonal += c[1] + c[2]
    free = [want(refs[k], hyps[k]) for k in range(len(lens))]
    assert diagonal > 0 and sum(e[0][0] for e in exp) > sum(f[0][0] for f in free)          # ... and the constraint costs errors
    # one word against itself: touching closes the diagonal, one tick of overlap opens it
    one = [np.array([7])]
    assert run(Packed(one, [np.array([[0, 5]])]), Packed(one, [np.array([[5, 9]])]), [(0, 0)]) == [((2, 0), [A.INS, A.DEL])]
    assert run(Packed(one, [np.array([[0, 5]])]), Packed(one, [np.array([[4, 9]])]), [(0, 0)]) == [((0, 1), [A.HIT])]


def test_invariants_on_larger_pairs():
    """Up to 600 x 600: the ops turn ref into hyp and their counts are edit_counts' of the same call; the oracle on three of them."""
    rng = np.random.default_rng(130)
    base = rng.integers(0, 50, 600)
    noisy = np.array([w if u > 0.15 else int(rng.integers(0, 50)) for w, u in zip(base.tolist(), rng.random(600))][:-40] + [3, 4, 5])
    refs = [rng.integers(0, 3, 600), rng.integers(0, 2, 531), rng.integers(0, 3, 600), rng.integers(0, 3, 64), base, base[100:], rng.integers(0, 50, 257)]
    hyps = [rng.integers(0, 3, 600), rng.integers(0, 2, 600), rng.integers(0, 3, 37), rng.integers(0, 3, 600), noisy, base[:450], rng.integers(0, 50, 255)]
    rp, hp = Packed(refs), Packed(hyps)
    pairs = [(k, k) for k in range(len(refs))]
    table = [(rp.starts[i], rp.lens[i], hp.starts[j], hp.lens[j]) for i, j in pairs]
    counts = scoring.edit_counts(rp.ids, hp.ids, table).tolist()
    first = None
    for lanes, along in CONFIGS + [(0, 0)]:
        got = run(rp, hp, pairs, lanes, along)
        for k in range(len(refs)):
            assert list(A.check_ops(refs[k], hyps[k], got[k][1])) == counts[k], (lanes, along, k)
            assert list(got[k][0]) == counts[k][:2]
        first = first or got
        assert got == first, (lanes, along)
    for k in (2, 3, 6):
        assert first[k] == want(refs[k], hyps[k]), k
    wc, wp = scoring.edit_alignments(rp.ids, hp.ids, table)
    assert wc.tolist() == counts and [p.tolist() for p in wp] == [g[1] for g in first] and all(p.dtype == torch.uint8 and not p.is_cuda for p in wp)


def test_a_pair_does_not_depend_on_its_neighbours():
    """The same pair alone, among others, and with other pairs reading its spans (whole, and overlapping parts of them)."""
    rng = np.random.default_rng(140)
    ref, hyp = rng.integers(0, 3, 131), rng.integers(0, 3, 150)
    alone = run(Packed([ref]), Packed([hyp]), [(0, 0)])[0]
    assert alone == want(ref, hyp)
    refs = [ref] + [rng.integers(0, 3, int(n)) for n in rng.integers(0, 40, 60)]
    hyps = [hyp] + [rng.integers(0, 3, int(n)) for n in rng.integers(0, 40, 60)]
    pairs = [(int(i), int(j)) for i, j in zip(rng.permutation(61), rng.permutation(61))]
    pairs[30:30] = [(0, 0)]
    got = run(Packed(refs), Packed(hyps), pairs)
    assert got[30] == alone and all(got[k] == want(refs[i], hyps[j]) for k, (i, j) in enumerate(pairs))
    # shared spans: every stream against every stream (what cpWER does), and raw rows that cut into the pair's spans
    rp, hp = Packed(refs[:4]), Packed(hyps[:4])
    pairs = [(i, j) for i in range(4) for j in range(4)]
    got = run(rp, hp, pairs)
    assert got[0] == alone and all(got[k] == want(refs[i], hyps[j]) for k, (i, j) in enumerate(pairs))
    got = run_table(rp, hp, [(rp.starts[0] + 30, 80, hp.starts[0], 150), (rp.starts[0], 131, hp.starts[0], 150), (rp.starts[0], 131, hp.starts[0] + 7, 90)])
    assert got == [want(ref[30:110], hyp), alone, want(ref, hyp[7:97])]


def test_nothing_is_written_for_an_empty_table():
    rp, hp = Packed([[1, 2, 3]]), Packed([[1, 9, 3, 4]])
    table = np.zeros((0, 4), np.int64)
    b = Buffers(table, 0, 0)
    assert b.nbytes == 0
    b.launch(rp, hp, table, 0, 0)
    assert b.result(table) == [] and (b.out.cpu() == -1).all() and (b.spans.cpu() == -1).all()
    counts, paths = scoring.edit_alignments(rp.ids, hp.ids, table)
    assert counts.shape == (0, 5) and paths == []
    counts, paths = scoring.edit_alignments(rp.ids, hp.ids, [(rp.starts[0], 3, hp.starts[0], 4), (rp.starts[0], 0, hp.starts[0], 2)])
    assert counts.tolist() == [[2, 2, 1, 0, 1], [2, 0, 0, 0, 2]] and [p.tolist() for p in paths] == [[0, 1, 0, 3], [3, 3]]
    with pytest.raises(L.DicowError, match="DICOW_EDIT_MAX_LEN"):
        scoring.edit_alignments(rp.ids, hp.ids, [(0, L.EDIT_MAX_LEN + 1, 0, 1)])
    with pytest.raises(L.DicowError, match="reads ref"):
        scoring.edit_alignments(rp.ids, hp.ids, [(3, 3, 0, 1)])


def test_graph_replay():
    rng = np.random.default_rng(150)
    refs = [rng.integers(0, 3, n) for n in (40, 300, 0, 513)]
    hyps = [rng.integers(0, 3, n) for n in (45, 250, 3, 20)]
    exp = [want(r, h) for r, h in zip(refs, hyps)]
    rp, hp = Packed(refs), Packed(hyps)
    table = np.array([(rp.starts[k], rp.lens[k], hp.starts[k], hp.lens[k]) for k in range(4)], np.int64)
    b = Buffers(table, 0, 0)
    b.launch(rp, hp, table, 0, 0)                                          # (code objects load outside the capture)
    assert b.result(table) == exp
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.launch(rp, hp, table, 0, 0)                                      # two linear launches behind the table copy
    for _ in range(2):
        b.out.fill_(-1)
        b.ops.fill_(SENTINEL_OP)
        b.spans.fill_(-1)
        b.ws[:b.nbytes].fill_(0)                                           # the replay uploads the tables again
        graph.replay()
        assert b.result(table) == exp


# ------------------------------------------------------------------------------------------------ the Python layer

def test_word_alignments_on_a_worked_example():
    # "down" against "sits" attains the key as a substitution, and the diagonal goes first walking back: "sat" is the deleted word
    refs = ["the cat sat down", "Hello  world", "", "a b"]
    hyps = ["the black cat sits", "hello WORLD", "q r", ""]
    chunks, measures = scoring.word_alignments(refs, hyps)
    assert chunks == [[("equal", 0, 1, 0, 1), ("insert", 1, 1, 1, 2), ("equal", 1, 2, 2, 3), ("delete", 2, 3, 3, 3), ("substitute", 3, 4, 3, 4)],
                      [("equal", 0, 2, 0, 2)], [("insert", 0, 0, 0, 2)], [("delete", 0, 2, 0, 0)]]
    assert (measures["hits"], measures["substitutions"], measures["deletions"], measures["insertions"]) == (4, 1, 3, 3)
    counts = scoring.word_error_counts(refs, hyps).sum(0)
    assert measures == scoring.measures_from_counts(counts[1], counts[2], counts[3], counts[4])
    chars, _ = scoring.word_alignments(["abc"], ["abd"], unit="char")
    assert chars == [[("equal", 0, 2, 0, 2), ("substitute", 2, 3, 2, 3)]]
    none, empty = scoring.word_alignments([], [])
    assert none == [] and np.isnan(empty.pop("wer")) and empty == {"mer": 0.0, "wil": 1.0, "wip": 0.0, "hits": 0, "substitutions": 0,
                                                                   "deletions": 0, "insertions": 0}


def _toy_session():
    """3 reference speakers, 2 hypothesis speakers: A is heard as y with one substitution and one word lost, B as x with a word too many
    and its second segment 20 s late, C by nobody."""
    ref = [("A", 0.0, 2.0, "one two three four"), ("A", 10.0, 12.0, "five six"), ("B", 3.0, 5.0, "red green blue"), ("B", 13.0, 14.0, "black white"),
           ("C", 6.0, 7.0, "lost words here")]
    hyp = [("y", 0.1, 1.9, "one too three"), ("y", 10.1, 11.9, "five six"), ("x", 3.0, 5.0, "red green uh blue"), ("x", 33.0, 34.0, "black white")]
    return ref, hyp


@pytest.mark.parametrize("timed", [True, False])
def test_session_alignment_on_a_toy_session(timed, tmp_path):
    ref, hyp = _toy_session()
    al = scoring.session_alignment(ref, hyp, timed=timed, collar=5.0)
    score = scoring.tcp_wer(ref, hyp, collar=5.0) if timed else scoring.cp_wer(ref, hyp)
    assert {k: al[k] for k in score} == score and al["timed"] is timed
    by = {spk["ref_speaker"]: spk for spk in al["speakers"]}
    assert [by[s]["hyp_speaker"] for s in "ABC"] == ["y", "x", None] and len(al["speakers"]) == 3
    ops = [row[0] for spk in al["speakers"] for row in spk["rows"]]
    assert (ops.count("substitute"), ops.count("delete"), ops.count("insert")) == (score["substitutions"], score["deletions"], score["insertions"])
    assert ops.count("equal") == al["hits"] and al["hits"] + score["substitutions"] + score["deletions"] == score["length"] == 14
    # the unmapped reference speaker: all deletions, with the reference's pseudo-word times
    assert by["C"]["rows"] == [("delete", "lost", 6.0, 6.307, None, None, None), ("delete", "words", 6.307, 6.692, None, None, None),
                               ("delete", "here", 6.692, 7.0, None, None, None)]                 # 1000 ms over 4 + 5 + 4 characters
    assert [r[0] for r in by["A"]["rows"]] == ["equal", "substitute", "equal", "delete", "equal", "equal"]
    assert by["A"]["rows"][1][1:5:3] == ("two", "too") and by["A"]["rows"][3][1] == "four"
    if timed:                                                                # 20 s late is outside the collar: no diagonal step
        assert [r[0] for r in by["B"]["rows"]] == ["equal", "equal", "insert", "equal", "insert", "insert", "delete", "delete"]
        assert by["B"]["rows"][0] == ("equal", "red", 3.0, 3.5, "red", -1.786, 8.214)            # centre of 3000 .. 3428 ms, +- 5 s
    else:
        assert [r[0] for r in by["B"]["rows"]] == ["equal", "equal", "insert", "equal", "equal", "equal"]
    assert scoring.error_breakdown(al)["substitutions"] == [(("two", "too"), 1)]
    report = scoring.save_alignment_report(al, tmp_path / "toy.json")
    assert report["breakdown"]["deletions"][0][1] == 1 and (tmp_path / "toy.json").stat().st_size > 0
    # the other way round: a hypothesis speaker nobody said comes out all insertions
    back = scoring.session_alignment(hyp, ref, timed=timed)
    extra = [spk for spk in back["speakers"] if spk["ref_speaker"] is None]
    assert len(extra) == 1 and extra[0]["hyp_speaker"] == "C" and [r[0] for r in extra[0]["rows"]] == ["insert"] * 3
    assert scoring.session_alignment([], [], timed=timed)["speakers"] == []


def test_the_wrapper_splits_a_pair_list_that_passes_the_cap(monkeypatch):
    rng = np.random.default_rng(160)
    lens = [(int(a), int(b)) for a, b in zip(rng.integers(0, 120, 40), rng.integers(0, 120, 40))]
    refs, hyps = [rng.integers(0, 3, a) for a, _ in lens], [rng.integers(0, 3, b) for _, b in lens]
    rp, hp = Packed(refs), Packed(hyps)
    table = np.array([(rp.starts[k], rp.lens[k], hp.starts[k], hp.lens[k]) for k in range(40)], np.int64)
    riv = torch.zeros((rp.ids.numel(), 2), dtype=torch.int32, device="cuda")
    riv[:, 1] = 1
    whole = scoring.edit_alignments(rp.ids, hp.ids, table, riv, torch.zeros((hp.ids.numel(), 2), dtype=torch.int32, device="cuda") + riv[:1])
    calls = []
    real = scoring._alignment_call
    monkeypatch.setattr(scoring, "_alignment_call", lambda *a: calls.append(a[2].shape[0]) or real(*a))
    one = scoring.edit_alignments(rp.ids, hp.ids, table)
    assert calls == [40]
    monkeypatch.setattr(L, "ALIGN_MAX_WS_BYTES", 8000)
    split = scoring.edit_alignments(rp.ids, hp.ids, table)
    assert len(calls) > 4 and sum(calls[1:]) == 40
    assert torch.equal(split[0], one[0]) and [p.tolist() for p in split[1]] == [p.tolist() for p in one[1]]
    assert torch.equal(whole[0], one[0])                                     # intervals that all overlap change nothing
    assert all(split[1][k].tolist() == want(refs[k], hyps[k])[1] for k in range(0, 40, 7))
    monkeypatch.setattr(L, "ALIGN_MAX_WS_BYTES", 500)
    with pytest.raises(L.DicowError, match="on its own"):
        scoring.edit_alignments(rp.ids, hp.ids, table)

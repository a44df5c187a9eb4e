"""dicow_edit_distance (csrc/edit_distance.hip) and the scoring module on the GPU against the oracles of tests/edit_distance_ref.py.
Every comparison is EXACT integer equality.  Every launch made through `run` reads flat buffers in which a sentinel id that occurs
nowhere else (with an interval that overlaps everything) stands immediately around every span, writes into an output inside the guard
bands of tests/util.py::guarded, and gets a workspace of exactly dicow_edit_distance_ws_bytes bytes inside guard bands of its own.
Run with `pytest -m gpu`."""
import types

import numpy as np
import pytest
import torch

import amd_pkg
from tests import edit_distance_ref as R
from tests.util import guarded

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, scoring  # noqa: E402

K, NARROW, WIDE = L.EDIT_K, L.EDIT_LANES_NARROW, L.EDIT_LANES
P_NARROW, P_WIDE = NARROW * K, WIDE * K
SENTINEL_ID, SENTINEL_IV = -7, (-10 ** 9, 10 ** 9)
CONFIGS = [(0, 0), (NARROW, 1), (NARROW, 2), (WIDE, 1), (WIDE, 2)]        # (lanes, along); 0 = the library's choice

_WANT = {}


def want(ref, hyp, riv=None, hiv=None):
    """The oracle's (errors, hits), computed once per distinct input (the shorter sequence along the oracle's Python loop: the key is
    symmetric, tests/test_host_scoring.py)."""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    if riv is not None:
        riv, hiv = np.asarray(riv, np.int64).reshape(-1, 2), np.asarray(hiv, np.int64).reshape(-1, 2)
    key = (ref.tobytes(), hyp.tobytes(), None if riv is None else riv.tobytes(), None if hiv is None else hiv.tobytes())
    if key not in _WANT:
        _WANT[key] = R.dp_numpy(ref, hyp, riv, hiv) if len(ref) <= len(hyp) else R.dp_numpy(hyp, ref, hiv, riv)
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


def launch(rp, hp, table, out, ws, ws_bytes, lanes=0, along=0):
    """The C entry point on the current stream; nothing else (capturable)."""
    n = table.shape[0]
    L.call("dicow_edit_distance", rp.ids.data_ptr(), rp.ids.numel(), hp.ids.data_ptr(), hp.ids.numel(), L.ptr(rp.iv), L.ptr(hp.iv),
           table.ctypes.data if n else None, n, out.data_ptr(), lanes, along, ws.data_ptr(), ws_bytes, L.stream())


def buffers(table):
    n = table.shape[0]
    nbytes = L.lib().dicow_edit_distance_ws_bytes(table.ctypes.data if n else None, n)
    assert nbytes >= 40 * n and nbytes % 8 == 0
    go = guarded((max(n, 1), 2), 2, torch.int32, name="out")
    gw = guarded((1, max(nbytes // 4, 2)), max(nbytes // 4, 2), torch.int32, name="ws")
    return go, gw, nbytes


def run(rp, hp, pairs, lanes=0, along=0):
    """pairs: (index into rp's sequences, index into hp's) -> int [n, 2] (errors, hits), after checking both guard bands."""
    table = np.array([(rp.starts[i], rp.lens[i], hp.starts[j], hp.lens[j]) for i, j in pairs], np.int64).reshape(-1, 4)
    go, gw, nbytes = buffers(table)
    launch(rp, hp, table, go.view, gw.view, nbytes, lanes, along)
    torch.cuda.synchronize()
    go.check()
    gw.check()
    assert go.untouched_inside() == 0
    return go.view.cpu().numpy()


def expect(seqs_r, seqs_h, pairs, ivs_r=None, ivs_h=None):
    return np.array([want(seqs_r[i], seqs_h[j], None if ivs_r is None else ivs_r[i], None if ivs_h is None else ivs_h[j]) for i, j in pairs])


REF_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 300]
HYP_LENS = sorted({0, 1, K - 1, K, K + 1} | {v for P in (P_NARROW, P_WIDE) for v in (P - 1, P, P + 1, 2 * P + 3)})


@pytest.mark.parametrize("lanes,along", CONFIGS)
@pytest.mark.parametrize("alphabet", [2, 1000])
def test_lengths_around_the_seams(alphabet, lanes, along):
    """Every ref_len x hyp_len around the strip (K), both panel widths (P) and two panels and a bit, in one launch; an alphabet of 2
    (ties everywhere) and of 1000 (hardly any)."""
    rng = np.random.default_rng(alphabet)
    refs = [rng.integers(0, alphabet, n) for n in REF_LENS]
    base = rng.integers(0, alphabet, max(HYP_LENS))
    hyps = [base[:n] for n in HYP_LENS]
    pairs = [(i, j) for i in range(len(refs)) for j in range(len(hyps))]
    got = run(Packed(refs), Packed(hyps), pairs, lanes, along)
    exp = expect(refs, hyps, pairs)
    assert np.array_equal(got, exp), [(REF_LENS[i], HYP_LENS[j]) for k, (i, j) in enumerate(pairs) if tuple(got[k]) != tuple(exp[k])][:8]
    for k, (i, j) in enumerate(pairs):
        if REF_LENS[i] == 0 or HYP_LENS[j] == 0:
            assert tuple(got[k]) == (REF_LENS[i] + HYP_LENS[j], 0)


@pytest.mark.parametrize("lanes,along", [(0, 0), (WIDE, 2), (NARROW, 1)])
def test_structured_pairs(lanes, along):
    rng = np.random.default_rng(5)
    refs, hyps = [], []
    for n in (K + 1, P_NARROW + 1, 700):
        a = rng.integers(0, 50, n)
        for b in (a, a + 50, a[:n // 2], a[n // 3:], np.roll(a, 5), np.roll(a, -n // 2), rng.integers(0, 2, n + 7)):
            refs.append(a)
            hyps.append(b)
    pairs = [(i, i) for i in range(len(refs))]
    got = run(Packed(refs), Packed(hyps), pairs, lanes, along)
    assert np.array_equal(got, expect(refs, hyps, pairs))
    for k in range(0, len(refs), 7):
        n = len(refs[k])
        assert tuple(got[k]) == (0, n) and tuple(got[k + 1]) == (n, 0)                     # identical; disjoint alphabets: all substituted
        assert tuple(got[k + 2]) == (n - n // 2, n // 2) and tuple(got[k + 3]) == (n // 3, n - n // 3)     # a prefix, a suffix
        assert tuple(got[k + 4])[0] <= 10                                                # a rotation by 5: at most 5 deleted + 5 inserted


def test_one_long_pair_and_the_wide_key():
    """About 5000 x (2 P + 3) through the library's own plan (the wide workgroup, three panels); and pairs whose lengths sum past the
    int32 key's range, which moves the whole call to the int64 key: narrow and wide, with either sequence along the lanes."""
    rng = np.random.default_rng(6)
    ref, hyp = rng.integers(0, 30, 5000), rng.integers(0, 30, 2 * P_WIDE + 3)
    assert tuple(run(Packed([ref]), Packed([hyp]), [(0, 0)])[0]) == want(ref, hyp)
    refs = [rng.integers(0, 4, 64000), rng.integers(0, 4, 300), [], rng.integers(0, 4, 700)]
    hyps = [rng.integers(0, 4, 50), rng.integers(0, 4, P_NARROW + 1), rng.integers(0, 4, 5), rng.integers(0, 4, 700)]
    ivr = [np.stack([np.arange(len(s)) * 10, np.arange(len(s)) * 10 + 10], 1) for s in refs]
    ivh = [np.stack([np.arange(len(s)) * 10 + 40000 * (k == 0), np.arange(len(s)) * 10 + 40000 * (k == 0) + 200], 1) for k, s in enumerate(hyps)]
    pairs = [(i, i) for i in range(4)]
    for lanes, along in ((0, 0), (WIDE, 1), (NARROW, 2)):
        assert np.array_equal(run(Packed(refs), Packed(hyps), pairs, lanes, along), expect(refs, hyps, pairs)), (lanes, along)
    assert np.array_equal(run(Packed(refs, ivr), Packed(hyps, ivh), pairs), expect(refs, hyps, pairs, ivr, ivh))


@pytest.mark.parametrize("lanes,along", [(0, 0), (WIDE, 2), (WIDE, 1)])
def test_intervals(lanes, along):
    rng = np.random.default_rng(7)
    lens = [(1, 1), (5, 9), (K + 1, 70), (300, P_NARROW + 1), (700, 650), (P_WIDE + 5, 600)]
    refs, hyps = [rng.integers(0, 3, a) for a, _ in lens], [rng.integers(0, 3, b) for _, b in lens]
    pairs = [(i, i) for i in range(len(lens))]
    span = lambda s, lo, hi: np.tile(np.array([[lo, hi]]), (len(s), 1))        # noqa: E731
    free = run(Packed(refs), Packed(hyps), pairs, lanes, along)
    assert np.array_equal(free, expect(refs, hyps, pairs))
    # all overlapping = unconstrained
    got = run(Packed(refs, [span(s, 0, 10) for s in refs]), Packed(hyps, [span(s, 9, 12) for s in hyps]), pairs, lanes, along)
    assert np.array_equal(got, free)
    # none overlapping, touching included (re == hb): insertions and deletions only
    for (r0, r1), (h0, h1) in (((0, 5), (5, 9)), ((5, 9), (0, 5)), ((0, 5), (100, 200)), ((3, 3), (3, 3))):
        got = run(Packed(refs, [span(s, r0, r1) for s in refs]), Packed(hyps, [span(s, h0, h1) for s in hyps]), pairs, lanes, along)
        assert got.tolist() == [[a + b, 0] for a, b in lens], (r0, r1, h0, h1)
    # ... while one tick of overlap opens the diagonal
    got = run(Packed(refs, [span(s, 0, 5) for s in refs]), Packed(hyps, [span(s, 4, 9) for s in hyps]), pairs, lanes, along)
    assert np.array_equal(got, free)
    # a band: word k at [10 k, 10 k + 10); the second half of the hypothesis 25 ticks late
    ivr = [np.stack([np.arange(len(s)) * 10, np.arange(len(s)) * 10 + 10], 1) for s in refs]
    ivh = [np.stack([np.arange(len(s)) * 10, np.arange(len(s)) * 10 + 10], 1) + 25 * (np.arange(len(s)) >= len(s) // 2)[:, None] for s in hyps]
    got = run(Packed(refs, ivr), Packed(hyps, ivh), pairs, lanes, along)
    assert np.array_equal(got, expect(refs, hyps, pairs, ivr, ivh)) and (got[:, 0] >= free[:, 0]).all() and (got[2:, 0] > free[2:, 0]).all()
    # random intervals, zero-width ones included
    ivr = [np.stack([b := rng.integers(0, 10 * len(s) + 1, len(s)), b + rng.integers(0, 40, len(s))], 1) for s in refs]
    ivh = [np.stack([b := rng.integers(0, 10 * len(s) + 1, len(s)), b + rng.integers(0, 40, len(s))], 1) for s in hyps]
    got = run(Packed(refs, ivr), Packed(hyps, ivh), pairs, lanes, along)
    assert np.array_equal(got, expect(refs, hyps, pairs, ivr, ivh))


def test_a_pair_does_not_depend_on_its_neighbours():
    """The same pair alone, among 300 others, and with other pairs reading its spans (whole, and overlapping parts of them)."""
    rng = np.random.default_rng(8)
    ref, hyp = rng.integers(0, 3, 531), rng.integers(0, 3, 600)
    alone = run(Packed([ref]), Packed([hyp]), [(0, 0)])[0]
    assert tuple(alone) == want(ref, hyp)
    refs = [ref] + [rng.integers(0, 3, int(n)) for n in rng.integers(0, 80, 300)]
    hyps = [hyp] + [rng.integers(0, 3, int(n)) for n in rng.integers(0, 80, 300)]
    pairs = [(int(i), int(j)) for i, j in zip(rng.permutation(301), rng.permutation(301))]
    at = 150
    pairs[at:at] = [(0, 0)]
    got = run(Packed(refs), Packed(hyps), pairs)
    assert np.array_equal(got, expect(refs, hyps, pairs)) and tuple(got[at]) == tuple(alone)
    # shared spans: every stream against every stream (what cpWER does), and raw rows that cut into the pair's spans
    rp, hp = Packed(refs[:6]), Packed(hyps[:6])
    pairs = [(i, j) for i in range(6) for j in range(6)]
    got = run(rp, hp, pairs)
    assert np.array_equal(got, expect(refs[:6], hyps[:6], pairs)) and tuple(got[0]) == tuple(alone)
    table = np.array([(rp.starts[0] + 100, 200, hp.starts[0], 600), (rp.starts[0], 531, hp.starts[0], 600), (rp.starts[0], 531, hp.starts[0] + 7, 300)])
    go, gw, nbytes = buffers(table)
    launch(rp, hp, table, go.view, gw.view, nbytes)
    torch.cuda.synchronize()
    go.check()
    gw.check()
    assert go.view.cpu().tolist() == [list(want(ref[100:300], hyp)), list(alone), list(want(ref, hyp[7:307]))]


def test_nothing_is_written_for_an_empty_table_and_the_wrapper_returns_five_counts():
    rp, hp = Packed([[1, 2, 3]]), Packed([[1, 9, 3, 4]])
    go, gw, nbytes = buffers(np.zeros((0, 4), np.int64))
    assert nbytes == 0
    launch(rp, hp, np.zeros((0, 4), np.int64), go.view, gw.view, 0)
    torch.cuda.synchronize()
    go.check()
    gw.check()
    assert go.untouched_inside() == 2 and gw.untouched_inside() == 2
    got = scoring.edit_counts(rp.ids, hp.ids, [(rp.starts[0], 3, hp.starts[0], 4), (rp.starts[0], 0, hp.starts[0], 2)])
    assert got.dtype == torch.int64 and not got.is_cuda and got.tolist() == [[2, 2, 1, 0, 1], [2, 0, 0, 0, 2]]
    assert scoring.edit_counts(rp.ids, hp.ids, np.zeros((0, 4), np.int64)).shape == (0, 5)
    with pytest.raises(L.DicowError, match="DICOW_EDIT_MAX_LEN"):
        scoring.edit_counts(rp.ids, hp.ids, [(0, L.EDIT_MAX_LEN + 1, 0, 1)])
    with pytest.raises(L.DicowError, match="reads ref"):
        scoring.edit_counts(rp.ids, hp.ids, [(3, 3, 0, 1)])


def test_side_stream_and_graph_replay():
    rng = np.random.default_rng(9)
    refs = [rng.integers(0, 3, n) for n in (40, 700, 0, 513)]
    hyps = [rng.integers(0, 3, n) for n in (45, 650, 3, 100)]
    pairs = [(i, i) for i in range(4)]
    exp = expect(refs, hyps, pairs)
    rp, hp = Packed(refs), Packed(hyps)
    table = np.array([(rp.starts[i], rp.lens[i], hp.starts[j], hp.lens[j]) for i, j in pairs], np.int64)
    go, gw, nbytes = buffers(table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(rp, hp, table, go.view, gw.view, nbytes)                  # (code objects load outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(go.view.cpu().numpy(), exp)
    go.view.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(rp, hp, table, go.view, gw.view, nbytes)                  # one linear launch behind its table copy
    # another eager call on this thread between capture and replay: the replay must not see its table.  As many pairs over the same id
    # buffers, none longer than the captured ones, so that even a stale image would stay inside `out` and `ws`
    other = [(3, 0), (0, 3), (2, 2), (0, 0)]
    table_b = np.array([(rp.starts[i], rp.lens[i], hp.starts[j], hp.lens[j]) for i, j in other], np.int64)
    gob, gwb, nbytes_b = buffers(table_b)
    assert nbytes_b <= nbytes
    launch(rp, hp, table_b, gob.view, gwb.view, nbytes_b)
    torch.cuda.synchronize()
    exp_b = expect(refs, hyps, other)
    assert np.array_equal(gob.view.cpu().numpy(), exp_b) and not np.array_equal(exp_b, exp)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(go.view.cpu().numpy(), exp)
    go.view.fill_(-1)
    gw.view.fill_(0)                                                     # the replay uploads the table again
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(go.view.cpu().numpy(), exp)
    go.check()
    gw.check()


# ------------------------------------------------------------------------------------------------ end to end

def _session():
    """3 reference speakers, 4 hypothesis speakers: the labels of A and B swapped, C's hypothesis 8 s late, D a false alarm."""
    rng = np.random.default_rng(10)
    words = {s: [f"{s.lower()}{k}" for k in range(40)] for s in "ABCD"}
    ref, hyp = [], []
    for s, label in (("A", "B"), ("B", "A"), ("C", "C")):
        for g in range(6):
            t0 = 10.0 * g + {"A": 0.0, "B": 3.0, "C": 6.0}[s]
            w = [words[s][int(k)] for k in rng.integers(0, 40, 8)]
            ref.append((s, t0, t0 + 2.5, " ".join(w)))
            h = list(w)
            h[2] = "oops"                                                # one substitution
            del h[5]                                                     # one deletion
            late = 8.0 if s == "C" else 0.0
            hyp.append((label, t0 + late + 0.1, t0 + late + 2.4, " ".join(h)))
    hyp.append(("D", 200.0, 203.0, " ".join(words["D"][:9])))
    return ref, hyp


def test_cp_wer_and_tcp_wer_on_a_session():
    ref, hyp = _session()
    cp, tcp = scoring.cp_wer(ref, hyp), scoring.tcp_wer(ref, hyp, collar=5.0)
    for got, collar in ((cp, None), (tcp, 5.0)):
        errors, length, assignments = R.brute_cp(ref, hyp, collar)
        assert len(assignments) == 1                                     # the case is built to make it unique
        assert (got["errors"], got["length"]) == (errors, length) and got["error_rate"] == errors / length
        assert sorted(got["assignment"], key=str) == sorted(assignments[0], key=str)
        assert got["insertions"] + got["deletions"] + got["substitutions"] == errors
        assert (got["missed_speaker"], got["falarm_speaker"], got["scored_speaker"]) == (0, 1, 3)
    assert set(cp) == {"error_rate", "errors", "length", "insertions", "deletions", "substitutions", "missed_speaker", "falarm_speaker",
                       "scored_speaker", "assignment"}
    assert sorted(cp["assignment"], key=str) == sorted([("A", "B"), ("B", "A"), ("C", "C"), (None, "D")], key=str)
    assert cp["length"] == 144 and cp["errors"] == 3 * 6 * 2 + 9 and tcp["errors"] > cp["errors"]
    # the other way round: a missed speaker; SegLST dicts; an empty side
    as_dict = lambda segs: [dict(speaker=s, start_time=a, end_time=b, words=w, session_id="x") for s, a, b, w in segs]      # noqa: E731
    back = scoring.cp_wer(as_dict(hyp), as_dict(ref))
    assert (back["errors"], back["missed_speaker"], back["falarm_speaker"], back["scored_speaker"]) == (cp["errors"], 1, 0, 4)
    assert back["insertions"] == cp["deletions"] and back["deletions"] == cp["insertions"]
    none = scoring.tcp_wer(ref, [])
    assert (none["errors"], none["deletions"], none["missed_speaker"], none["error_rate"]) == (144, 144, 3, 1.0)
    assert scoring.cp_wer([], [])["error_rate"] is None


class _StubTokenizer:
    pad_token_id = 0
    table = {1: "Hello", 2: "world", 3: "<|1.20|>", 4: "again", 5: "WORLD", 6: "there"}

    def batch_decode(self, ids, skip_special_tokens=False, normalize=True, decode_with_timestamps=False):
        assert skip_special_tokens and not normalize and int(np.min(ids)) >= 0
        self.seen_timestamps = decode_with_timestamps
        return [" ".join(self.table[int(t)] for t in row if int(t) != self.pad_token_id) for row in ids]


def test_compute_metrics_on_a_stub_tokenizer():
    tok = _StubTokenizer()
    fn = scoring.make_compute_metrics(tok, decode_with_timestamps=True)
    pred = types.SimpleNamespace(predictions=np.array([[1, 3, 5, -100, -100], [1, 6, 4, 4, -100], [4, -100, -100, -100, -100]]),
                                 label_ids=np.array([[1, 2, -100, -100], [1, 2, 4, -100], [-100, -100, -100, -100]]))
    m = fn(pred)
    assert tok.seen_timestamps is True and int(pred.label_ids[2, 0]) == -100
    # "hello world" / "hello world" ; "hello world again" / "hello there again again" (S + I) ; "-" / "again" (S)
    assert (m["hits"], m["substitutions"], m["deletions"], m["insertions"]) == (4, 2, 0, 1)
    assert m["wer"] == 3 / 6 and m["mer"] == 3 / 7 and m["wip"] == (4 / 6) * (4 / 7) and m["wil"] == 1 - (4 / 6) * (4 / 7)
    chars = [("hello world", "hello world"), ("hello world again", "hello there again again"), ("-", "again")]
    e = sum(R.dp_loops(list(a), list(b))[0] for a, b in chars)
    assert m["cer"] == e / sum(len(a) for a, _ in chars)
    direct = scoring.error_measures(["Hello  world", "hello world again", "-"], ["hello WORLD", "hello there again again", "again"])
    assert direct == m
    w = scoring.word_error_counts(["a b c", "", "a"], ["a x c", "q r", ""])
    assert w.tolist() == [[1, 2, 1, 0, 0], [2, 0, 0, 0, 2], [1, 0, 0, 1, 0]]

"""dicow_orc_distance (csrc/orc_distance.hip) and the ORC-WER / tcORC-WER part of the scoring module on the GPU against the oracles of
tests/orc_distance_ref.py.  Every comparison is EXACT integer equality.  Every launch made through `run` reads flat buffers in which a
sentinel id that occurs nowhere else (with an interval that overlaps everything) stands immediately around every utterance and stream,
writes (errors, hits) and the assignment into outputs inside the guard bands of tests/util.py::guarded, and gets a workspace of exactly
dicow_orc_distance_ws_bytes bytes inside guard bands of its own.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import orc_distance_ref as R
from tests.util import guarded

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, scoring  # noqa: E402

K = L.ORC_K
SENTINEL_ID, EVERYWHERE = -7, (-10 ** 9, 10 ** 9)
_WANT = {}


def want(case):
    """The oracle's (errors, hits), computed once per case object: brute force over the assignments where there are few, else orc_dp."""
    if id(case) not in _WANT:
        utts, hyps, uiv, hiv = case
        small = len(hyps) ** len(utts) <= 243 and sum(len(u) for u in utts) <= 25 and all(len(h) <= 12 for h in hyps)
        _WANT[id(case)] = (case, (R.orc_brute if small else R.orc_dp)(utts, hyps, uiv, hiv))
    return _WANT[id(case)][1]


class Packed:
    """The utterances and streams of a list of cases in two flat buffers, a sentinel before, between and behind them, and the three host
    tables.  `timed`: every word carries an interval; a case without intervals gets one that overlaps everything, which is the same."""

    def __init__(self, cases, timed):
        ref, riv, hyp, hiv, self.utts, self.streams, self.problems = [SENTINEL_ID], [EVERYWHERE], [SENTINEL_ID], [EVERYWHERE], [], [], []

        def add(ids, ivs, seq, iv, rows):
            rows.append((len(ids), len(seq)))
            ids += [int(v) for v in seq] + [SENTINEL_ID]
            ivs += ([tuple(x) for x in np.asarray(iv).reshape(-1, 2).tolist()] if iv is not None else [EVERYWHERE] * len(seq)) + [EVERYWHERE]

        for utts, hyps, uiv, hiv_ in cases:
            assert timed or uiv is None
            self.problems.append((len(self.utts), len(utts), len(self.streams), len(hyps)))
            for u, seq in enumerate(utts):
                add(ref, riv, seq, None if uiv is None else uiv[u], self.utts)
            for h, seq in enumerate(hyps):
                add(hyp, hiv, seq, None if hiv_ is None else hiv_[h], self.streams)
        self.ref = torch.tensor(ref, dtype=torch.int32).cuda()
        self.hyp = torch.tensor(hyp, dtype=torch.int32).cuda()
        self.riv = torch.tensor(riv, dtype=torch.int32).reshape(-1, 2).cuda() if timed else None
        self.hiv = torch.tensor(hiv, dtype=torch.int32).reshape(-1, 2).cuda() if timed else None
        self.problems = np.ascontiguousarray(np.asarray(self.problems, np.int64).reshape(-1, 4))
        self.utts = np.ascontiguousarray(np.asarray(self.utts, np.int64).reshape(-1, 2))
        self.streams = np.ascontiguousarray(np.asarray(self.streams, np.int64).reshape(-1, 2))


def prepare(cases, timed, assign):
    """The packed inputs, the host tables, and the three outputs inside their guard bands (the workspace: exactly ws_bytes)."""
    pk = Packed(cases, timed)
    n, rows = len(cases), len(pk.utts)
    tables = (pk.problems.ctypes.data, n, pk.utts.ctypes.data if rows else None, pk.streams.ctypes.data if len(pk.streams) else None)
    nbytes = L.lib().dicow_orc_distance_ws_bytes(*tables, int(assign))
    assert nbytes >= L.ORC_DESC_BYTES * n + L.ORC_UTT_BYTES * rows and nbytes % 8 == 0, L.lib().dicow_last_error()
    go = guarded((n, 2), 2, torch.int32, name="out")
    gw = guarded((1, nbytes // 4), nbytes // 4, torch.int32, name="ws")
    ga = guarded((1, max(rows, 1)), max(rows, 1), torch.int32, name="assignment") if assign else None
    return pk, tables, nbytes, go, gw, ga


def launch(pk, tables, nbytes, go, gw, ga):
    """The C entry point on the current stream; nothing else (capturable)."""
    L.call("dicow_orc_distance", pk.ref.data_ptr(), pk.ref.numel(), pk.hyp.data_ptr(), pk.hyp.numel(), L.ptr(pk.riv), L.ptr(pk.hiv), *tables,
           go.view.data_ptr(), ga.view.data_ptr() if ga is not None else None, gw.view.data_ptr(), nbytes, L.stream())


def run(cases, timed, assign=True):
    """-> int [n, 2] (errors, hits) and, with `assign`, the int stream per utterance row; after checking all three guard bands."""
    pk, tables, nbytes, go, gw, ga = prepare(cases, timed, assign)
    rows = len(pk.utts)
    launch(pk, tables, nbytes, go, gw, ga)
    torch.cuda.synchronize()
    go.check()
    gw.check()
    assert go.untouched_inside() == 0
    asg = None
    if assign:
        ga.check()
        assert ga.untouched_inside() == (0 if rows else 1)
        asg = ga.view.cpu().numpy().reshape(-1)[:rows]
    return go.view.cpu().numpy(), asg


def key_of_assignment(cases, asg, timed):
    """The summed (errors, hits) of the returned assignment: per case and stream the assigned utterances concatenated against the stream,
    all pairs of all cases in ONE launch of the existing dicow_edit_distance."""
    refs, rivs, hyps, hivs, owner, row = [], [], [], [], [], 0
    for c, (utts, hs, uiv, hiv) in enumerate(cases):
        a = asg[row:row + len(utts)]
        row += len(utts)
        assert all(0 <= int(x) < max(len(hs), 1) for x in a) or not hs, (c, a)
        for h, hyp in enumerate(hs):
            mine = [u for u in range(len(utts)) if int(a[u]) == h]
            refs.append(np.concatenate([np.asarray(utts[u], np.int64) for u in mine]) if mine else np.zeros(0, np.int64))
            hyps.append(np.asarray(hyp, np.int64))
            if timed:
                ev = lambda seq: np.tile(np.asarray(EVERYWHERE, np.int64), (len(seq), 1))        # noqa: E731
                rivs.append(np.concatenate([np.asarray(uiv[u], np.int64).reshape(-1, 2) if uiv is not None else ev(utts[u]) for u in mine])
                            if mine else np.zeros((0, 2), np.int64))
                hivs.append(np.asarray(hiv[h], np.int64).reshape(-1, 2) if hiv is not None else ev(hyp))
            owner.append(c)
    total = np.zeros((len(cases), 2), np.int64)
    if not refs:
        return total
    cat = lambda xs, w: torch.from_numpy(np.concatenate(xs).astype(np.int32).reshape((-1, 2) if w == 2 else (-1,))).cuda()   # noqa: E731
    rs, hs_ = np.cumsum([0] + [len(r) for r in refs]), np.cumsum([0] + [len(h) for h in hyps])
    pairs = [(rs[k], len(refs[k]), hs_[k], len(hyps[k])) for k in range(len(refs))]
    counts = scoring.edit_counts(cat(refs, 1), cat(hyps, 1), pairs, cat(rivs, 2) if timed else None, cat(hivs, 2) if timed else None).numpy()
    for k, c in enumerate(owner):
        total[c] += counts[k, :2]
    return total


def check(cases, timed):
    """The whole contract for a list of cases in one call: the oracle's (errors, hits) with and without an assignment, an assignment that
    attains them, and for a case without any stream the host's answer."""
    exp = np.array([want(c) for c in cases], np.int64).reshape(-1, 2)
    got, asg = run(cases, timed, assign=True)
    assert np.array_equal(got, exp), [(k, tuple(got[k]), tuple(exp[k])) for k in range(len(cases)) if tuple(got[k]) != tuple(exp[k])][:8]
    plain, _ = run(cases, timed, assign=False)
    assert np.array_equal(plain, exp)
    scored = key_of_assignment(cases, asg, timed)
    for k, c in enumerate(cases):
        if c[1]:
            assert tuple(scored[k]) == tuple(exp[k]), (k, tuple(scored[k]), tuple(exp[k]))
    row = 0
    for utts, hyps, _, _ in cases:
        for u, utt in enumerate(utts):
            if not hyps:
                assert asg[row + u] == -1
            elif len(utt) == 0:
                assert asg[row + u] == 0                                     # an utterance of zero words is assigned stream 0
        row += len(utts)
    return got, asg


SEEDED = R.seeded_cases()


def test_seeded_brute_force_cases_batched_and_one_by_one():
    """The 60 cases of tests/test_host_orc_scoring.py as 60 problems of one call (timed: the untimed half with intervals that overlap
    everything), the untimed half again in an untimed call, and every case alone: identical outputs, the assignment included."""
    got, asg = check(SEEDED, True)
    untimed = [c for c in SEEDED if c[2] is None]
    got_u, asg_u = check(untimed, False)
    row = row_u = k_u = 0
    for k, c in enumerate(SEEDED):
        one, a = run([c], c[2] is not None, assign=True)
        assert tuple(one[0]) == tuple(got[k]) == want(c), k
        assert np.array_equal(a, asg[row:row + len(c[0])]), k
        if c[2] is None:
            assert tuple(got_u[k_u]) == tuple(one[0]) and np.array_equal(asg_u[row_u:row_u + len(c[0])], a), k
            row_u += len(c[0])
            k_u += 1
        row += len(c[0])


def _seq(rng, n, alphabet=5):
    return rng.integers(0, alphabet, n)


def _edges():
    rng = np.random.default_rng(77)
    s = lambda *lens: [_seq(rng, n) for n in lens]                          # noqa: E731
    e = {
        "one stream": (s(3, 0, 4, 2), s(8), None, None),
        "an empty stream among others": (s(2, 3, 1), s(4, 0, 3), None, None),
        "all streams empty": (s(2, 0, 3), s(0, 0), None, None),
        "empty utterances first, in the middle and last": (s(0, 3, 0, 0, 2, 0), s(3, 4), None, None),
        "one utterance": (s(5), s(3, 4, 2), None, None),
        "the most streams": (s(2, 3, 1, 2), s(1, 2, 2, 1, 1, 2, 1, 2), None, None),
        "no stream": (s(2, 3), [], None, None),
        "no utterance": ([], s(2, 3), None, None),
        "only empty utterances": (s(0, 0), s(2, 3), None, None),
        "utterances around the chunk": (s(K, K + 1, K - 1, 2 * K + 5, 2 * K), s(9, 11), None, None),
        "64 states": (s(3, 4), s(7, 7), None, None),
        "64 states, 4 x 16": (s(3, 4), s(3, 15), None, None),
        "65 x 1 states": (s(3, K + 2), s(64, 0), None, None),
        "63 states": (s(4, 2), s(6, 8), None, None),
    }
    for n0 in (0, 1, 62, 63, 64):                                           # n_0 + 1 = 1, 2, 63, 64, 65 along the contiguous axis
        e[f"shortest stream of {n0}"] = (s(3, K + 1, 2), s(n0, max(n0, 5)), None, None)
    same = _seq(rng, 5, 2)
    e["identical streams"] = ([same[:2], same[2:4], same[4:], same[1:3]], [same, same.copy(), same.copy()], None, None)
    assert len(e["the most streams"][1]) == L.ORC_MAX_STREAMS
    return e


EDGES = _edges()


@pytest.mark.parametrize("name", list(EDGES))
def test_edge(name):
    case = EDGES[name]
    got, asg = check([case], False)
    utts, hyps = case[0], case[1]
    if len(hyps) == 1:                                                       # H = 1: dicow_edit_distance on the concatenation
        ref = torch.from_numpy(np.concatenate(utts).astype(np.int32)).cuda()
        hyp = torch.from_numpy(np.asarray(hyps[0], np.int32)).cuda()
        assert tuple(scoring.edit_counts(ref, hyp, [(0, ref.numel(), 0, hyp.numel())])[0, :2].tolist()) == tuple(got[0])
    if not hyps:
        assert tuple(got[0]) == (sum(len(u) for u in utts), 0)
    if not utts or all(len(h) == 0 for h in hyps):
        assert tuple(got[0]) == (sum(len(u) for u in utts) + sum(len(h) for h in hyps), 0)
    if name == "all streams empty":
        assert set(asg.tolist()) == {0}                                      # every assignment ties: the first stream, deterministically


def test_all_edges_in_one_call_and_determinism():
    """All edge cases as the problems of one call give what each gives alone; the same call twice is bit-identical; a problem's outputs
    do not move when other problems are added in front of and behind it."""
    cases = list(EDGES.values())
    got, asg = check(cases, False)
    again, asg2 = run(cases, False, assign=True)
    assert np.array_equal(got, again) and np.array_equal(asg, asg2)
    row = 0
    for k, c in enumerate(cases):
        one, a = run([c], False, assign=True)
        assert tuple(one[0]) == tuple(got[k]) and np.array_equal(a, asg[row:row + len(c[0])]), list(EDGES)[k]
        row += len(c[0])
    mid = EDGES["utterances around the chunk"]
    alone, a_alone = run([mid], False)
    among, a_among = run([EDGES["the most streams"], EDGES["no stream"], mid, EDGES["shortest stream of 63"]], False)
    first = len(EDGES["the most streams"][0]) + len(EDGES["no stream"][0])
    assert tuple(among[2]) == tuple(alone[0]) and np.array_equal(a_among[first:first + len(mid[0])], a_alone)


def _medium(timed):
    rng = np.random.default_rng(11)
    hyps = [_seq(rng, n, 12) for n in (37, 29, 41)]
    lens = [0, 70, 1, 33, 8, 9, 0, 17, 64, 5, 26, 12]
    utts = [_seq(rng, n, 12) for n in lens]
    if not timed:
        return utts, hyps, None, None

    def ivs(seq, width):
        b = rng.integers(0, 400, len(seq))
        return np.stack([b, b + rng.integers(0, width, len(seq))], axis=1).astype(np.int64).reshape(-1, 2)
    return utts, hyps, [ivs(u, 60) for u in utts], [ivs(h, 300) for h in hyps]


MEDIUM = {False: _medium(False), True: _medium(True)}


@pytest.mark.parametrize("timed", [False, True])
def test_medium_case_against_the_numpy_dynamic_program(timed):
    """Streams of 37, 29 and 41 words (47 880 states), 12 utterances of 0-70 words, an alphabet of 12."""
    case = MEDIUM[timed]
    assert len(case[0]) == 12 and [len(h) for h in case[1]] == [37, 29, 41]
    got, _ = check([case], timed)
    if timed:
        assert tuple(got[0]) != tuple(run([MEDIUM[False]], False, assign=False)[0][0])     # the intervals do close diagonals here


def test_side_stream_and_graph_replay():
    """The same call on a side stream, then captured into a graph and replayed twice, the second time over a wiped workspace (the replay
    uploads the descriptors again): the oracle's results and the same assignment every time."""
    cases = [SEEDED[1], EDGES["utterances around the chunk"], EDGES["no stream"], SEEDED[3], EDGES["the most streams"]]
    exp = np.array([want(c) for c in cases], np.int64)
    _, asg = run(cases, True)
    pk, tables, nbytes, go, gw, ga = prepare(cases, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(pk, tables, nbytes, go, gw, ga)                              # (code objects load outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(go.view.cpu().numpy(), exp) and np.array_equal(ga.view.cpu().numpy().reshape(-1), asg)
    graph = torch.cuda.CUDAGraph()
    go.view.fill_(-1)
    with torch.cuda.graph(graph):
        launch(pk, tables, nbytes, go, gw, ga)                              # one linear chain of launches behind the descriptor copy
    for wipe in (False, True):
        go.view.fill_(-1)
        ga.view.fill_(-5)
        if wipe:
            gw.view.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(go.view.cpu().numpy(), exp) and np.array_equal(ga.view.cpu().numpy().reshape(-1), asg), wipe
    go.check()
    gw.check()
    ga.check()


# ---------------------------------------------------------------------------------------------------------------- the host recipe

REF = [("A", 0.0, 2.0, "a b c"), ("B", 2.0, 4.0, "d e f"), ("C", 4.0, 6.0, "g h i"), ("A", 6.0, 8.0, "j k l")]
HYP = [("X", 0.0, 2.0, "a b c"), ("Y", 2.0, 4.0, "d e f"), ("X", 4.0, 6.0, "g h i"), ("Y", 6.0, 8.0, "j k x")]


def test_orc_wer_gives_an_utterance_to_the_other_speakers_stream():
    """Three reference speakers, two hypothesis streams.  By hand: A's first utterance and C's go to X (X reads exactly "a b c g h i"), B's
    and A's second go to Y ("d e f j k l" against "d e f j k x": one substitution).  'l' occurs in no stream, so one error is the least.
    cpWER must keep A's two utterances together and leave one reference speaker without a stream."""
    for res in (scoring.orc_wer(REF, HYP), scoring.tcorc_wer(REF, HYP), scoring.tcorc_wer(REF + [("B", 9.0, 9.5, "")], HYP, collar=5.0),
                scoring.session_orc_wer(REF, HYP)):
        assert res == {"error_rate": 1 / 12, "errors": 1, "length": 12, "insertions": 0, "deletions": 0, "substitutions": 1,
                       "assignment": ("X", "Y", "X", "Y")}
    cp = scoring.cp_wer(REF, HYP)
    assert cp["length"] == 12 and cp["errors"] > 1 and scoring.orc_wer(REF, HYP)["error_rate"] < cp["error_rate"]
    # no hypothesis at all: everything deleted, nobody to assign to
    assert scoring.orc_wer(REF, []) == {"error_rate": 1.0, "errors": 12, "length": 12, "insertions": 0, "deletions": 12, "substitutions": 0,
                                        "assignment": (None,) * 4}
    assert scoring.orc_wer([], HYP)["errors"] == 12 and scoring.orc_wer([], HYP)["insertions"] == 12 and scoring.orc_wer([], HYP)["error_rate"] is None


def test_tcorc_wer_closes_a_match_outside_the_collar():
    """Reference "y" spans 10-11 s; the hypothesis says "y" at 20-21 s, centre 20.5 s.  With a collar of 5 s the hypothesis interval is
    [15.5, 25.5] s and begins after the reference word ends: "y" may be neither matched nor substituted, so it is deleted and inserted.
    With a collar of 10 s ([10.5, 30.5] s) the two overlap and match."""
    ref = [("A", 0.0, 1.0, "x"), ("A", 10.0, 11.0, "y")]
    hyp = [("X", 0.0, 1.0, "x"), ("X", 20.0, 21.0, "y")]
    assert scoring.tcorc_wer(ref, hyp, collar=5.0) == {"error_rate": 1.0, "errors": 2, "length": 2, "insertions": 1, "deletions": 1, "substitutions": 0,
                                                      "assignment": ("X", "X")}
    assert scoring.tcorc_wer(ref, hyp, collar=10.0)["errors"] == 0 and scoring.orc_wer(ref, hyp)["errors"] == 0


SESSION_REF = [("A", 0.0, 2.0, "a b"), ("B", 1.0, 3.0, "c d"), ("A", 10.0, 12.0, "e f"), ("B", 20.0, 22.0, "g h"), ("A", 21.0, 23.0, "i j")]
SESSION_HYP = [("X", 0.0, 2.0, "a b"), ("Y", 1.0, 3.0, "c x"), ("X", 20.0, 22.0, "g h"), ("Y", 21.0, 23.0, "i j"), ("Y", 5.5, 6.0, "")]


def test_session_tcorc_wer_sums_its_groups():
    """Silence from 3 s to 10 s and from 12 s to 20 s, both longer than group_duration = 5 s: cuts at 5 s, 12 s and 17 s, so the reference
    falls into three groups -- before 5 s, [5, 12) s, from 17 s -- and the middle one has no hypothesis: it is scored against the dummy
    segment, two deletions.  By hand: group one has "c x" against "c d", one substitution; group three none."""
    groups = [(SESSION_REF[:2], SESSION_HYP[:2]), (SESSION_REF[2:3], []), (SESSION_REF[3:], SESSION_HYP[2:4])]
    parts = [scoring.tcorc_wer(r, h) for r, h in groups]
    res = scoring.session_tcorc_wer(SESSION_REF, SESSION_HYP)
    for k in ("errors", "length", "insertions", "deletions", "substitutions"):
        assert res[k] == sum(p[k] for p in parts), k
    assert [p["errors"] for p in parts] == [1, 2, 0]
    assert res == {"error_rate": 3 / 10, "errors": 3, "length": 10, "insertions": 0, "deletions": 2, "substitutions": 1,
                   "assignment": ("X", "Y", "", "X", "Y")}
    assert res["assignment"][:2] == parts[0]["assignment"] and res["assignment"][3:] == parts[2]["assignment"] and parts[1]["assignment"] == (None,)
    # a hypothesis segment after the last cut (23 s, where both sides fall silent) is in a group without reference: not scored, as in the reference
    assert scoring.session_tcorc_wer(SESSION_REF, SESSION_HYP + [("Z", 23.5, 24.0, "k")]) == res
    # one group only when no silence is long enough
    assert scoring.session_tcorc_wer(SESSION_REF, SESSION_HYP, group_duration=60)["errors"] == scoring.tcorc_wer(SESSION_REF, SESSION_HYP)["errors"]


def test_session_metrics_has_the_reference_columns():
    res = scoring.session_metrics(SESSION_REF, SESSION_HYP, ["cp_wer", "tcp_wer", "tcorc_wer", "orc_wer"])
    short = ["wer", "errors", "length", "insertions", "deletions", "substitutions", "assignment"]
    full = short[:-1] + ["missed_speaker", "falarm_speaker", "scored_speaker", "assignment"]
    assert set(res) == {f"{p}_{k}" for p, keys in (("cp", full), ("tcp", full), ("tcorc", short), ("orc", short)) for k in keys}
    assert res["tcorc_errors"] == 3 and res["tcorc_wer"] == 3 / 10 and res["orc_length"] == res["cp_length"] == 10
    assert res["orc_errors"] <= res["cp_errors"] and res["tcorc_errors"] >= res["orc_errors"]
    assert set(scoring.session_metrics(SESSION_REF, SESSION_HYP, ["orc_wer"])) == {f"orc_{k}" for k in short}
    agg = scoring.aggregate_session_metrics([res, res], ["cp_wer", "tcp_wer", "tcorc_wer", "orc_wer"])
    assert agg["tcorc_errors"] == 6 and agg["tcorc_wer"] == 3 / 10 and agg["cp_mean_scored_speaker"] == 2

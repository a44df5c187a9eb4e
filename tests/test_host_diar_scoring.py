"""CPU tests of diarization scoring's host side: the two oracles of tests/diar_score_ref.py against each other, the collar, the formulas of
DER / JER / the mapping on hand-made counts, relabelling and the RTTM round trip, the corpus aggregation, and every refusal the library
makes before any launch.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import amd_pkg
from tests import diar_score_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, diar_scoring as D  # noqa: E402
from ts_asr_whisper_amd.diar_front_end import SpeakerSegments  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    assert re.search(r"^int\s+dicow_diar_score\s*\(", stable, flags=re.M) and re.search(r"^int64_t\s+dicow_diar_score_ws_bytes\s*\(", stable, flags=re.M)
    for name, val in (("CHUNK", _lib.DIAR_SCORE_CHUNK), ("ROW", _lib.DIAR_SCORE_ROW), ("OUT_WORDS", _lib.DIAR_SCORE_OUT_WORDS),
                      ("DESC_BYTES", _lib.DIAR_SCORE_DESC_BYTES), ("MAX_E", _lib.DIAR_SCORE_MAX_E), ("MAX_TICK", _lib.DIAR_SCORE_MAX_TICK),
                      ("MAX_WS_BYTES", _lib.DIAR_SCORE_MAX_WS_BYTES)):
        m = re.search(rf"^#define\s+DICOW_DIAR_SCORE_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.DIAR_SCORE_OUT_WORDS == 64 * 64 + 64 + 64 + 8
    assert {"dicow_diar_score", "dicow_diar_score_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_diar_score.restype is _lib.c_i and lib.dicow_diar_score_ws_bytes.restype is _lib.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("unscored_intervals", "diar_score_counts", "diarization_error", "jaccard_error", "optimal_mapping", "score_diarizations",
                 "aggregate_diarization_scores", "error_from_counts", "jaccard_from_counts", "mapping_from_counts", "split_counts"):
        assert getattr(pkg, name) is getattr(D, name) and name in pkg.__all__


# ------------------------------------------------------------------------------------------------ the oracles

@pytest.mark.parametrize("seed", range(6))
def test_the_two_oracles_agree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 400))
    Sr, Sh = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    ref = R.random_table(rng, Sr, int(rng.integers(0, 20)), n)
    hyp = R.random_table(rng, Sh, int(rng.integers(0, 20)), n)
    uns = R.random_unscored(rng, int(rng.integers(0, 5)), n)
    for skip in (False, True):
        d, s = R.dense_counts(ref, hyp, uns, skip, n), R.sweep_counts(ref, hyp, uns, skip)
        assert R.same(d, s), (seed, skip)
        assert d["matched"] + d["missed"] == d["total"] and d["total"] == int(d["R"].sum()) and d["C"].sum() >= d["matched"]


def test_oracles_on_a_case_worked_out_by_hand():
    # ref: a on [0, 10), b on [5, 15)      hyp: x on [2, 12)      unscored [9, 11)
    ref = (np.array([0, 5, 10, 15]), np.array([1, 3, 2], np.uint64), 2)
    hyp = (np.array([2, 12]), np.array([1], np.uint64), 1)
    want = {"C": [[7], [5]], "R": [9, 8], "H": [8], "scored": 13, "total": 17, "missed": 9, "false_alarm": 0, "matched": 8}
    want_skip = {"C": [[3], [1]], "R": [5, 4], "H": [4], "scored": 9, "total": 9, "missed": 5, "false_alarm": 0, "matched": 4}
    for skip, w in ((False, want), (True, want_skip)):
        w = dict(w, C=np.array(w["C"]), R=np.array(w["R"]), H=np.array(w["H"]))
        assert R.same(R.dense_counts(ref, hyp, [(9, 11)], skip, 20), w) and R.same(R.sweep_counts(ref, hyp, [(9, 11)], skip), w)
    big = 1 << 40
    far = (np.array([big - 15, big - 10, big - 5, big]), ref[1], 2)
    assert R.sweep_counts(far, (np.array([big - 13, big - 3]), hyp[1], 1), [(big - 6, big - 4)], False)["C"].tolist() == [[7], [5]]
    assert R.best_correct([[3, 5], [4, 9]]) == 12 and R.best_correct([[3, 5, 1]]) == 5 and R.best_correct(np.zeros((0, 3))) == 0
    assert R.best_correct(np.eye(8, dtype=np.int64)[::-1] * 7) == 56        # (the scipy branch)


# ------------------------------------------------------------------------------------------------ the collar

def _segs(d, n=160000):
    return SpeakerSegments(d, n)


def test_unscored_intervals():
    # touching segments of one speaker keep the collar at their common boundary, where the speaker's activity does not change
    ref = _segs({"a": [(16000, 32000), (32000, 48000)]})
    assert ref.active.tolist() == [1, 1]
    assert D.unscored_intervals(ref, 0.25).tolist() == [[14000, 18000], [30000, 34000], [46000, 50000]]
    # overlapping and touching collars merge; the first is clipped at 0
    ref = _segs({"a": [(1000, 5000)], "b": [(4000, 9000), (13000, 20000)]})
    assert D.unscored_intervals(ref, 0.25).tolist() == [[0, 15000], [18000, 22000]]
    assert D.unscored_intervals(ref, 0.0).shape == (0, 2) and D.unscored_intervals(ref, 0.0).dtype == np.int64
    # the half width is round(collar * 16000 / 2): 0.0001 s -> 0.8 -> 1 tick, 0.00005 s -> 0.4 -> none
    one = _segs({"a": [(100, 200)]})
    assert D.unscored_intervals(one, 0.0001).tolist() == [[99, 101], [199, 201]]
    assert D.unscored_intervals(one, 0.00005).shape == (0, 2)
    assert D.unscored_intervals(one, 0.5).tolist() == [[0, 4200]]
    with pytest.raises(ValueError):
        D.unscored_intervals(one, -1.0)


# ------------------------------------------------------------------------------------------------ the formulas

def _counts(C, R_, H, matched, missed, fa):
    C = np.asarray(C, np.int64).reshape(len(R_), len(H))
    return {"C": C, "R": np.asarray(R_, np.int64), "H": np.asarray(H, np.int64), "scored": 0, "total": matched + missed, "missed": missed,
            "false_alarm": fa, "matched": matched}


def test_error_and_jaccard_formulas_on_hand_made_counts():
    # 2 x 3, in ticks of 1/16000 s: the best assignment is 0 -> 1, 1 -> 0 (16000 + 8000), not the greedy 0 -> 0
    c = _counts([[12000, 16000, 0], [8000, 0, 0]], [32000, 16000], [24000, 16000, 4000], matched=30000, missed=18000, fa=14000)
    assert D.mapping_from_counts(c) == {0: 1, 1: 0}
    e = D.error_from_counts(c)
    assert e == {"total": 3.0, "correct": 1.5, "missed detection": 1.125, "false alarm": 0.875, "confusion": 0.375,
                 "diarization error rate": (18000 + 14000 + 6000) / 48000}
    assert e == R.der(c)
    j = D.jaccard_from_counts(c)
    want = (32000 + 16000 - 32000) / (32000 + 16000 - 16000) + (16000 + 24000 - 16000) / (16000 + 24000 - 8000)
    assert j == {"speaker error": want, "speaker count": 2, "jaccard error rate": want / 2} and j == R.jer(c, {0: 1, 1: 0})
    # 4 x 2 with a pair that shares nothing: speaker 2 is paired by nobody, speaker 1 only with a zero -> no pair, Jaccard error 1.0 each;
    # speaker 3 has no scored time and does not count
    c = _counts([[5, 0], [0, 0], [0, 0], [0, 0]], [10, 7, 3, 0], [5, 9], matched=5, missed=15, fa=9)
    assert D.mapping_from_counts(c) == {0: 0}
    j = D.jaccard_from_counts(c)
    assert j == {"speaker error": (10 + 5 - 10) / (10 + 5 - 5) + 2.0, "speaker count": 3, "jaccard error rate": (0.5 + 2.0) / 3}
    assert D.error_from_counts(c)["confusion"] == 0.0 and D.error_from_counts(c)["diarization error rate"] == 24 / 20
    # total == 0: 0.0 when nothing is wrong, 1.0 when something is
    z = _counts([[0]], [0], [0], matched=0, missed=0, fa=0)
    assert D.error_from_counts(z)["diarization error rate"] == 0.0 and D.jaccard_from_counts(z)["jaccard error rate"] == 0.0
    assert D.mapping_from_counts(z) == {}
    z = _counts([[0]], [0], [40], matched=0, missed=0, fa=40)
    assert D.error_from_counts(z)["diarization error rate"] == 1.0 and D.error_from_counts(z)["total"] == 0.0
    # the assignment reaches the brute-force maximum on random rectangular matrices
    rng = np.random.default_rng(5)
    for _ in range(20):
        Sr, Sh = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        C = rng.integers(0, 50, (Sr, Sh)) * (rng.random((Sr, Sh)) < 0.6)
        c = _counts(C, C.sum(1) + 1, C.sum(0) + 1, matched=int(C.sum()), missed=3, fa=2)
        m = D.mapping_from_counts(c)
        assert sum(int(C[i, j]) for i, j in m.items()) == R.best_correct(C) and all(C[i, j] > 0 for i, j in m.items())
        assert len(set(m.values())) == len(m)
    # split_counts reads the library's row layout
    row = np.zeros(_lib.DIAR_SCORE_OUT_WORDS, np.int64)
    row[1 * 64 + 2], row[4096 + 1], row[4160 + 2], row[4224:4229] = 9, 11, 13, (1, 2, 3, 4, 5)
    s = D.split_counts(row, 2, 3)
    assert s["C"].tolist() == [[0, 0, 0], [0, 0, 9]] and s["R"].tolist() == [0, 11] and s["H"].tolist() == [0, 0, 13]
    assert [s[k] for k in D.SCALARS] == [1, 2, 3, 4, 5]


def test_aggregation_of_a_corpus_from_given_components():
    recs = [{"total": 10.0, "missed detection": 1.0, "false alarm": 0.5, "confusion": 0.25, "speaker error": 0.75, "speaker count": 3,
             "speaker count error": 1},
            {"total": 30.0, "missed detection": 3.0, "false alarm": 2.5, "confusion": 0.75, "speaker error": 1.25, "speaker count": 5,
             "speaker count error": 2},
            {"total": 0.0, "missed detection": 0.0, "false alarm": 1.0, "confusion": 0.0, "speaker error": 0.0, "speaker count": 0,
             "speaker count error": 3}]
    a = D.aggregate_diarization_scores(recs)
    assert a == {"MSCE": 2.0, "JER": 2.0 / 8, "DER": 9.0 / 40.0, "Miss": 4.0 / 40.0, "FA": 4.0 / 40.0, "Conf": 1.0 / 40.0}
    assert D.aggregate_diarization_scores([recs[2]]) == {"MSCE": 3.0, "JER": 0.0, "DER": 1.0, "Miss": 0.0, "FA": 1.0, "Conf": 0.0}
    assert D.aggregate_diarization_scores([]) == {"MSCE": 0.0, "JER": 0.0, "DER": 0.0, "Miss": 0.0, "FA": 0.0, "Conf": 0.0}


# ------------------------------------------------------------------------------------------------ relabelling and RTTM

def test_relabelled_and_rttm_round_trip(tmp_path):
    hyp = _segs({"spk0": [(0, 1000), (5000, 6000)], "spk1": [(500, 2000)], "spk2": [(1500, 3000), (7000, 8000)], "spk3": [(6000, 6500)]})
    out = hyp.relabelled({"spk0": "alice", "spk1": "bob"})
    assert out.speakers == ["-1", "alice", "bob"] and out.n_samples == hyp.n_samples
    assert out.intervals == {"alice": [(0, 1000), (5000, 6000)], "bob": [(500, 2000)], "-1": [(1500, 3000), (6000, 6500), (7000, 8000)]}
    both = hyp.relabelled({"spk0": "x", "spk1": "x", "spk2": "y", "spk3": "x"}, default="unk")
    assert both.intervals == {"x": [(0, 2000), (5000, 6500)], "y": [(1500, 3000), (7000, 8000)]}       # overlapping and touching ones joined
    assert hyp.relabelled({}, default="nobody").speakers == ["nobody"]
    path = str(tmp_path / "out.rttm")
    odd = SpeakerSegments({"a": [(1, 7), (123457, 1234567)], "b": [(3, 16001), (99999, 100000)]}, 1234570)
    odd.to_rttm(path, "rec1")
    lines = open(path).read().splitlines()
    assert len(lines) == 4 and lines[0].split()[:3] == ["SPEAKER", "rec1", "1"] and lines[0].split()[7] == "a"
    back = SpeakerSegments.from_rttm(path, "rec1", n_samples=odd.n_samples)
    assert back.intervals == odd.intervals and back.bounds.tolist() == odd.bounds.tolist() and back.active.tolist() == odd.active.tolist()
    with pytest.raises(ValueError):
        SpeakerSegments.from_rttm(path, "another")


# ------------------------------------------------------------------------------------------------ the library's refusals

def _call(lib, problems, chunk=0, wsb=None, out=4096, ws=8192, edit=None):
    """dicow_diar_score with never-dereferenced device pointers: every call made through here is refused, or launches nothing."""
    b, a, u, pt = D.pack_problems(problems)
    if edit is not None:
        edit(b, a, u, pt)
    t = D.table_args(b, a, u, pt, chunk)
    need = lib.dicow_diar_score_ws_bytes(*t)
    rc = lib.dicow_diar_score(*t, out, ws, max(need, 0) if wsb is None else wsb, None)
    return need, rc, lib.dicow_last_error()


def test_library_refuses_bad_tables_before_any_launch():
    lib = _lib.lib()
    ref = (np.array([0, 10, 20, 35]), np.array([1, 3, 2], np.uint64), 2)
    hyp = (np.array([5, 30]), np.array([1], np.uint64), 1)
    uns = np.array([(8, 12), (12, 14), (30, 40)])
    ok = [(ref, hyp, uns, False), (hyp, ref, None, True)]
    b, a, u, pt = D.pack_problems(ok)
    need = lib.dicow_diar_score_ws_bytes(*D.table_args(b, a, u, pt))
    # descriptors + the three arrays + per problem M endpoints and n_chunks partials of 64 Sr + 136 words
    assert need == 2 * 120 + 8 * (12 + 8 + 6) + 8 * (12 + 1 * (64 * 2 + 136)) + 8 * (6 + 1 * (64 * 1 + 136))
    assert lib.dicow_diar_score_ws_bytes(*D.table_args(b, a, u, pt, 4)) == need + 8 * (2 * (64 * 2 + 136) + 1 * (64 * 1 + 136))
    assert lib.dicow_diar_score_ws_bytes(None, 0, None, 0, None, 0, None, 0, 0) == 0
    assert lib.dicow_diar_score(None, 0, None, 0, None, 0, None, 0, 0, None, None, 0, None) == 0      # nothing to do: nothing launched

    def swap_bounds(b, a, u, pt): b[1], b[2] = b[2], b[1]
    def equal_bounds(b, a, u, pt): b[2] = b[1]
    def stray_bit(b, a, u, pt): a[3] |= np.uint64(2)                      # the hypothesis of problem 0 has one speaker
    def top_bit(b, a, u, pt): a[0] |= np.uint64(1) << np.uint64(63)
    def overlap(b, a, u, pt): u[1, 0] = 11
    def unsorted(b, a, u, pt): u[2] = (2, 4)
    def empty_iv(b, a, u, pt): u[0] = (8, 8)
    def negative(b, a, u, pt): u[0, 0] = -1
    def too_far(b, a, u, pt): b[3] = (1 << 40) + 1
    def outside(b, a, u, pt): pt[1, 0] = 11
    def outside_a(b, a, u, pt): pt[0, 5] = 8
    def outside_u(b, a, u, pt): pt[0, 9] = 4
    def many_spk(b, a, u, pt): pt[0, 3] = 65
    def bad_flag(b, a, u, pt): pt[0, 10] = 2
    def neg_e(b, a, u, pt): pt[0, 2] = -1

    for edit, word in ((swap_bounds, b"not strictly increasing"), (equal_bounds, b"not strictly increasing"), (stray_bit, b"names a speaker >= S=1"),
                       (top_bit, b"names a speaker >= S=2"), (overlap, b"overlap or are not sorted"), (unsorted, b"overlap or are not sorted"),
                       (empty_iv, b"empty or reversed"), (negative, b"leaves"), (too_far, b"leave"), (outside, b"reads bounds"),
                       (outside_a, b"reads active"), (outside_u, b"reads unscored"), (many_spk, b"outside [0, 64]"), (bad_flag, b"skip_overlap"),
                       (neg_e, b"entries")):
        got, rc, err = _call(lib, ok, edit=edit)
        assert got == -1 and rc == -1 and word in err and b"diar_score" in err, (edit.__name__, err)
    for kw, word in ((dict(wsb=need - 8), b"ws_bytes"), (dict(wsb=0), b"ws_bytes"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                     (dict(out=4100), b"aligned"), (dict(ws=8196), b"aligned"), (dict(chunk=-1), b"chunk"),
                     (dict(chunk=_lib.DIAR_SCORE_CHUNK + 1), b"chunk")):
        got, rc, err = _call(lib, ok, **kw)
        assert rc == -1 and word in err, (kw, err)
    # bit 63 is an ordinary speaker of a 64-speaker table
    wide = (np.array([0, 5]), np.array([(1 << 63) | 1], np.uint64), 64)
    b, a, u, pt = D.pack_problems([(wide, wide, None, False)])
    assert lib.dicow_diar_score_ws_bytes(*D.table_args(b, a, u, pt)) == 120 + 8 * 6 + 8 * (4 + 64 * 64 + 136)
    # the wrapper: shapes of a table, and no CPU fallback
    with pytest.raises(_lib.DicowError, match="bounds"):
        D.pack_problems([((np.array([0, 5, 9]), np.array([1], np.uint64), 1), hyp, None, False)])
    with pytest.raises(_lib.DicowError, match="GPU"):
        D.diar_score_counts(ok, device="cpu")

"""CPU tests of the scoring module's host side: the C-ABI entry points and their binding, the refusals made before any launch, the two
oracles of tests/edit_distance_ref.py against each other, the S / D / I identities, the Hungarian solver against brute force, the
measure formulas and the pseudo-word timing on hand-worked cases.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import edit_distance_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, scoring  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_edit_distance\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const int32_t* ref_ids", "int64_t n_ref", "const int32_t* hyp_ids", "int64_t n_hyp", "const int32_t* ref_iv",
                    "const int32_t* hyp_iv", "const int64_t* pairs", "int n_pairs", "int32_t* out", "int lanes", "int along", "void* ws",
                    "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_edit_distance_ws_bytes\s*\(\s*const int64_t\* pairs,\s*int n_pairs\s*\);", stable, flags=re.M)
    for name, val in (("MAX_LEN", _lib.EDIT_MAX_LEN), ("K", _lib.EDIT_K), ("LANES", _lib.EDIT_LANES), ("LANES_NARROW", _lib.EDIT_LANES_NARROW)):
        m = re.search(rf"^#define\s+DICOW_EDIT_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.EDIT_MAX_LEN >= 65535
    c = _lib
    assert _lib._SIGS["dicow_edit_distance"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_i, c.c_i, c.c_vp,
                                                 c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_edit_distance_ws_bytes"] == [c.c_vp, c.c_i]
    assert {"dicow_edit_distance", "dicow_edit_distance_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_edit_distance.restype is c.c_i and lib.dicow_edit_distance_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("edit_counts", "Vocabulary", "word_error_counts", "error_measures", "make_compute_metrics", "cp_wer", "tcp_wer",
                 "pseudo_word_intervals", "hungarian"):
        assert getattr(pkg, name) is getattr(scoring, name) and name in pkg.__all__


def _table(pairs):
    return np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 4))


def _call(lib, pairs, **kw):
    """dicow_edit_distance with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    t = _table(pairs)
    a = dict(ref=p, n_ref=1000, hyp=2 * p, n_hyp=1000, riv=None, hiv=None, pairs=t.ctypes.data if len(t) else None, n=len(t), out=3 * p,
             lanes=0, along=0, ws=4 * p, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = max(0, lib.dicow_edit_distance_ws_bytes(a["pairs"], a["n"]))
    return lib.dicow_edit_distance(a["ref"], a["n_ref"], a["hyp"], a["n_hyp"], a["riv"], a["hiv"], a["pairs"], a["n"], a["out"], a["lanes"],
                                   a["along"], a["ws"], a["wsb"], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    K, narrow = _lib.EDIT_K, _lib.EDIT_LANES_NARROW
    ws = lambda pairs: lib.dicow_edit_distance_ws_bytes(_table(pairs).ctypes.data, len(pairs))    # noqa: E731
    # the table (40 bytes a pair), and two 8-byte columns of the longer side for a pair some plan may cut into panels
    assert lib.dicow_edit_distance_ws_bytes(None, 0) == 0
    assert ws([(0, 5, 0, 7)]) == 40 and ws([(0, narrow * K, 0, 7), (0, 0, 0, 0)]) == 80
    assert ws([(0, narrow * K + 1, 0, 7)]) == 40 + 16 * (narrow * K + 1) and ws([(0, 3, 9, 5000), (0, 600, 0, 100)]) == 80 + 16 * 5600
    for bad, word in (((None, -1), b"negative n_pairs"), ((None, 2), b"null pair table")):
        assert lib.dicow_edit_distance_ws_bytes(*bad) == -1 and b"edit_distance_ws_bytes" in lib.dicow_last_error()
        assert word in lib.dicow_last_error()
    for bad, word in (([(0, -1, 0, 5)], b"negative length"), ([(0, 5, 0, -2)], b"negative length"),
                      ([(0, _lib.EDIT_MAX_LEN + 1, 0, 5)], b"DICOW_EDIT_MAX_LEN"), ([(0, 5, 0, 1 << 40)], b"DICOW_EDIT_MAX_LEN")):
        assert ws(bad) == -1 and b"edit_distance_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error()
    ok = [(0, 600, 0, 700), (600, 400, 100, 900)]
    big = dict(n_ref=1 << 20, n_hyp=1 << 20)
    for bad, word in ((dict(pairs=[(0, -1, 0, 5)]), b"negative length"), (dict(pairs=[(0, 5, 0, -1)]), b"negative length"),
                      (dict(pairs=[(-1, 5, 0, 5)]), b"reads ref"), (dict(pairs=[(0, 5, -3, 5)]), b"reads hyp"),
                      (dict(pairs=[(990, 11, 0, 5)]), b"reads ref"), (dict(pairs=[(0, 5, 1001, 0)]), b"reads hyp"),
                      (dict(pairs=[(0, 5, 0, 5), (0, 5, 500, 501)]), b"pair 1 reads hyp"),
                      (dict(pairs=[(0, _lib.EDIT_MAX_LEN + 1, 0, 5)], **big), b"DICOW_EDIT_MAX_LEN"),
                      (dict(pairs=[(0, 5, 0, _lib.EDIT_MAX_LEN + 1)], **big), b"DICOW_EDIT_MAX_LEN"),
                      (dict(pairs=ok, riv=4096), b"one side only"), (dict(pairs=ok, hiv=4096), b"one side only"),
                      (dict(pairs=ok, n_ref=-1), b"negative buffer"), (dict(pairs=ok, n_hyp=-1), b"negative buffer"),
                      (dict(pairs=ok, lanes=128), b"lanes"), (dict(pairs=ok, lanes=-1), b"lanes"), (dict(pairs=ok, along=3), b"along"),
                      (dict(pairs=ok, out=None), b"null"), (dict(pairs=ok, ws=None), b"null"), (dict(pairs=ok, ref=None), b"null"),
                      (dict(pairs=ok, hyp=None), b"null"), (dict(pairs=ok, ref=4098), b"aligned"), (dict(pairs=ok, out=4097), b"aligned"),
                      (dict(pairs=ok, ws=4100), b"aligned"), (dict(pairs=ok, riv=4096, hiv=4098), b"aligned"),
                      (dict(pairs=ok, wsb=80 + 16 * 1600 - 1), b"ws_bytes"), (dict(pairs=ok, wsb=0), b"ws_bytes"),
                      (dict(pairs=ok, n=-1), b"negative n_pairs")):
        rc = _call(lib, **bad)
        assert rc == -1, bad
        assert b"edit_distance" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    assert lib.dicow_edit_distance(4096, 10, 8192, 10, None, None, None, 2, 12288, 0, 0, 16384, 1 << 20, None) == -1
    assert b"null pair table" in lib.dicow_last_error()
    # an empty table launches nothing and needs nothing
    assert _call(lib, [], ref=None, hyp=None, out=None, ws=None, wsb=0) == 0


def test_workspace_size_at_the_plan_boundaries():
    """dicow_edit_distance_ws_bytes on pair lists that cross each boundary of the plan it shares with dicow_edit_alignment: the header's
    formula (40 bytes a pair, 16 bytes a symbol of the longer side when that exceeds DICOW_EDIT_LANES_NARROW * DICOW_EDIT_K), and the
    values the library returned before the two plans were merged.  (The longer side at the narrow panel and one past it, and a pair of
    two empty sides, are in test_entry_points_refuse_bad_arguments_before_any_launch.)"""
    lib = _lib.lib()
    K, narrow, wide = _lib.EDIT_K, _lib.EDIT_LANES_NARROW, _lib.EDIT_LANES
    assert 30000 + 31439 == 65535 - wide * K
    for pairs, recorded in (([(0, narrow * K, 0, narrow * K + 50), (5, 7, 3, 9)], 9072),           # the shorter side at the narrow panel
                            ([(0, narrow * K + 1, 0, narrow * K + 60), (5, 7, 3, 9)], 9232),       # one past it: the wide workgroup
                            ([(0, 30000, 0, 31439), (0, 3, 1, 4)], 503104),                        # the int32 key's limit
                            ([(0, 30000, 0, 31440), (0, 3, 1, 4)], 503120),                        # one past it: the int64 key
                            ([(0, 0, 0, 9), (0, 300, 0, 0), (0, 0, 0, 0), (2, 40, 1, 33)], 160)):  # empty sides
        got = lib.dicow_edit_distance_ws_bytes(_table(pairs).ctypes.data, len(pairs))
        assert got == 40 * len(pairs) + sum(16 * max(p[1], p[3]) for p in pairs if max(p[1], p[3]) > narrow * K) == recorded, pairs


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.DicowError, match="GPU"):
        scoring.edit_counts(ids, ids, [(0, 4, 0, 4)])
    with pytest.raises(_lib.DicowError, match="GPU"):
        scoring.edit_counts(np.zeros(4, np.int32), ids, [(0, 4, 0, 4)])
    with pytest.raises(ValueError):
        scoring.word_error_counts(["a"], ["a", "b"])
    with pytest.raises(ValueError):
        scoring.hungarian(np.zeros((2, 3)))


def _random_pair(rng, alphabet=3, max_len=12):
    n, m = int(rng.integers(0, max_len + 1)), int(rng.integers(0, max_len + 1))
    return rng.integers(0, alphabet, n).tolist(), rng.integers(0, alphabet, m).tolist()


def _random_intervals(rng, n, span=20, width=6):
    b = rng.integers(0, span, n)
    return np.stack([b, b + rng.integers(0, width, n)], axis=1).tolist()      # zero-width intervals included


def test_numpy_oracle_equals_the_triple_loop():
    rng = np.random.default_rng(11)
    ties = 0
    for case in range(200):
        ref, hyp = _random_pair(rng)
        riv = hiv = None
        if case % 2:
            riv, hiv = _random_intervals(rng, len(ref)), _random_intervals(rng, len(hyp))
        e, h = R.dp_loops(ref, hyp, riv, hiv)
        assert R.dp_numpy(ref, hyp, riv, hiv) == (e, h), (ref, hyp, riv, hiv)
        assert R.dp_numpy(hyp, ref, hiv, riv) == (e, h)                       # the key is symmetric in the two sequences
        s, d, i = R.sdi(e, h, len(ref), len(hyp))
        assert min(s, d, i, h) >= 0 and s + d + i == e and h + s + d == len(ref) and h + s + i == len(hyp)
        ties += (e, h) != R.dp_loops(ref[::-1], hyp[::-1], None if riv is None else riv[::-1], None if hiv is None else hiv[::-1])
    assert ties == 0                                                          # ... and under reversing both
    # hand-worked: the most hits among the minimal alignments; no overlap leaves insertions and deletions only; touching is not overlapping
    assert R.dp_loops([1, 2, 3], [1, 9, 3]) == (1, 2) and R.dp_loops([], [4, 4]) == (2, 0) and R.dp_loops([4], []) == (1, 0)
    assert R.dp_loops([0, 1], [1, 0]) == (2, 1)                                # S + S would be (2, 0): D + I keeps one hit
    assert R.dp_loops([7], [7], [(0, 5)], [(5, 9)]) == (2, 0) and R.dp_loops([7], [7], [(0, 5)], [(4, 9)]) == (0, 1)
    assert R.dp_numpy([7], [7], [(0, 5)], [(5, 9)]) == (2, 0) and R.dp_numpy([7], [7], [(5, 9)], [(0, 5)]) == (2, 0)


def test_counts_follow_from_errors_hits_and_the_lengths():
    rng = np.random.default_rng(12)
    pairs, eh, want = [], [], []
    for _ in range(50):
        ref, hyp = _random_pair(rng)
        e, h = R.dp_loops(ref, hyp)
        pairs.append((3, len(ref), 5, len(hyp)))
        eh.append((e, h))
        want.append((e, h) + R.sdi(e, h, len(ref), len(hyp)))
    got = scoring.counts_from(np.array(eh, np.int32), np.array(pairs))
    assert got.dtype == torch.int64 and got.tolist() == [list(w) for w in want]
    assert scoring.counts_from(np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int64)).shape == (0, 5)


def test_hungarian_equals_brute_force():
    rng = np.random.default_rng(13)
    for r in range(1, 6):
        for h in range(1, 6):
            for rep in range(6):
                n = max(r, h)
                cost = np.zeros((n, n), np.int64)
                cost[:r, :h] = rng.integers(0, 4 if rep % 2 else 50, (r, h))      # small values: many ties
                cost[:r, h:] = rng.integers(0, 50, (r, 1))                        # rectangular, padded as the session scorer pads
                cost[r:, :h] = rng.integers(0, 50, (1, h))
                col = scoring.hungarian(cost)
                best, perms = R.brute_assignment(cost)
                assert sorted(col) == list(range(n)) and tuple(col) in perms, (cost, col)
                assert sum(int(cost[i, col[i]]) for i in range(n)) == best
    assert scoring.hungarian(np.zeros((0, 0))) == [] and scoring.hungarian([[5]]) == [0]
    assert scoring.hungarian([[4, 1, 3], [2, 0, 5], [3, 2, 2]]) == [1, 0, 2]


def test_measure_formulas_on_hand_worked_cases():
    m = scoring.measures_from_counts(hits=3, substitutions=0, deletions=0, insertions=0)                  # identical strings
    assert (m["wer"], m["mer"], m["wil"], m["wip"]) == (0.0, 0.0, 0.0, 1.0) and m["hits"] == 3
    m = scoring.measures_from_counts(hits=0, substitutions=0, deletions=3, insertions=0)                  # an empty hypothesis
    assert (m["wer"], m["mer"], m["wil"], m["wip"]) == (1.0, 1.0, 1.0, 0.0) and m["deletions"] == 3
    m = scoring.measures_from_counts(hits=2, substitutions=1, deletions=0, insertions=0)                  # one substitution in three words
    assert m["wer"] == 1 / 3 and m["mer"] == 1 / 3 and m["wip"] == (2 / 3) * (2 / 3) and m["wil"] == 1 - (2 / 3) * (2 / 3)
    m = scoring.measures_from_counts(hits=2, substitutions=0, deletions=0, insertions=2)                  # insertions count in mer, not in wer's length
    assert m["wer"] == 1.0 and m["mer"] == 0.5 and m["wip"] == 0.5
    assert set(m) == {"wer", "mer", "wil", "wip", "hits", "substitutions", "deletions", "insertions"}


def test_vocabulary_and_default_normaliser():
    v = scoring.Vocabulary()
    assert v.ids(["b", "a", "b"]) == [0, 1, 0] and v.ids(["c", "a"]) == [2, 1] and len(v) == 3
    assert scoring._default_norm("  Hello   WORLD \n") == "hello world"
    assert scoring._tokens("ab c", "word") == ["ab", "c"] and scoring._tokens("ab c", "char") == ["a", "b", " ", "c"]
    with pytest.raises(ValueError):
        scoring._tokens("x", "syllable")


def test_pseudo_word_timing_on_hand_worked_segments():
    # 2.0 s .. 5.0 s, words of 2, 1 and 3 characters: boundaries at 2000, 3000, 3500, 5000 ms
    words = ["ab", "c", "def"]
    assert scoring.pseudo_word_intervals(2.0, 5.0, words) == [(2000, 3000), (3000, 3500), (3500, 5000)] == R.word_spans(2.0, 5.0, words)
    assert scoring.pseudo_word_intervals(2.0, 5.0, words, points=True) == [(2500, 2500), (3250, 3250), (4250, 4250)]
    assert scoring.pseudo_word_intervals(2.0, 5.0, words, points=True, collar_s=5.0) == [(-2500, 7500), (-1750, 8250), (-750, 9250)]
    assert scoring.pseudo_word_intervals(2.0, 5.0, words, points=True, collar_s=5.0) == R.word_points(2.0, 5.0, words, 5.0)
    # floored boundaries: 1 s over 3 equal words
    assert scoring.pseudo_word_intervals(0.0, 1.0, ["a", "b", "c"]) == [(0, 333), (333, 666), (666, 1000)]
    assert scoring.pseudo_word_intervals(1.0, 2.0, []) == []
    # streams: segments by start time per speaker, dicts with the SegLST keys or tuples
    segs = [("B", 4.0, 5.0, "x y"), {"speaker": "A", "start_time": 3.0, "end_time": 4.0, "words": "late"}, ("A", 0.0, 2.0, "so early")]
    st = scoring._streams(segs, False, 0.0)
    assert list(st) == ["A", "B"] and st["A"][0] == ["so", "early", "late"] and st["A"][1] == [(0, 571), (571, 2000), (3000, 4000)]
    assert st["B"] == (["x", "y"], [(4000, 4500), (4500, 5000)])
    ref = R.streams([s if isinstance(s, tuple) else ("A", 3.0, 4.0, "late") for s in segs], R.word_spans)
    assert {k: (v[0], v[1]) for k, v in ref.items()} == st

"""CPU tests of ORC-WER / tcORC-WER scoring's host side: the two C-ABI entry points and their binding, every refusal made before any
launch, the workspace formula of DESIGN.md section 8, the two oracles of tests/orc_distance_ref.py against each other (which pins the
definition without a GPU), and the restated host recipe of the reference on cases worked out by hand.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import orc_distance_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, scoring  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_orc_distance\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const int32_t* ref_ids", "int64_t n_ref", "const int32_t* hyp_ids", "int64_t n_hyp", "const int32_t* ref_iv",
                    "const int32_t* hyp_iv", "const int64_t* problems", "int n_problems", "const int64_t* utts", "const int64_t* streams",
                    "int32_t* out", "int32_t* assignment", "void* ws", "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_orc_distance_ws_bytes\s*\(\s*const int64_t\* problems,\s*int n_problems,\s*const int64_t\* utts,\s*"
                     r"const int64_t\* streams,\s*int want_assignment\s*\);", stable, flags=re.M)
    for name, val in (("MAX_STREAMS", _lib.ORC_MAX_STREAMS), ("K", _lib.ORC_K), ("MAX_WORDS", _lib.ORC_MAX_WORDS), ("MAX_STATES", _lib.ORC_MAX_STATES),
                      ("MAX_WS_BYTES", _lib.ORC_MAX_WS_BYTES), ("DESC_BYTES", _lib.ORC_DESC_BYTES), ("UTT_BYTES", _lib.ORC_UTT_BYTES)):
        m = re.search(rf"^#define\s+DICOW_ORC_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.ORC_MAX_STREAMS == 8
    assert _lib.ORC_MAX_WORDS + _lib.ORC_K <= 65535                       # (E + the chunk's padding rows) * 2^15 stays inside int32
    c = _lib
    assert _lib._SIGS["dicow_orc_distance"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_vp, c.c_vp, c.c_vp,
                                                c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_orc_distance_ws_bytes"] == [c.c_vp, c.c_i, c.c_vp, c.c_vp, c.c_i]
    assert {"dicow_orc_distance", "dicow_orc_distance_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_orc_distance.restype is c.c_i and lib.dicow_orc_distance_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("orc_counts", "orc_wer", "tcorc_wer", "filter_empty_segments", "create_vad_mask", "find_group_splits", "map_utterance_to_split",
                 "merge_streams", "create_dummy_seg_list", "session_tcorc_wer", "session_orc_wer", "session_metrics", "aggregate_session_metrics"):
        assert getattr(pkg, name) is getattr(scoring, name) and name in pkg.__all__


def _t(rows, w):
    return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, w))


def _ws(lib, problems, utts, streams, assign=0):
    p, u, s = _t(problems, 4), _t(utts, 2), _t(streams, 2)
    return lib.dicow_orc_distance_ws_bytes(p.ctypes.data if len(p) else None, len(p), u.ctypes.data if len(u) else None,
                                           s.ctypes.data if len(s) else None, assign)


def _call(lib, problems, utts, streams, **kw):
    """dicow_orc_distance with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    pg = 4096
    p, u, s = _t(problems, 4), _t(utts, 2), _t(streams, 2)
    a = dict(ref=pg, n_ref=1000, hyp=2 * pg, n_hyp=1000, riv=None, hiv=None, problems=p.ctypes.data if len(p) else None, n=len(p),
             utts=u.ctypes.data if len(u) else None, streams=s.ctypes.data if len(s) else None, out=3 * pg, asg=None, ws=4 * pg, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = max(0, lib.dicow_orc_distance_ws_bytes(a["problems"], a["n"], a["utts"], a["streams"], int(a["asg"] is not None)))
    return lib.dicow_orc_distance(a["ref"], a["n_ref"], a["hyp"], a["n_hyp"], a["riv"], a["hiv"], a["problems"], a["n"], a["utts"], a["streams"],
                                  a["out"], a["asg"], a["ws"], a["wsb"], None)


def _r8(b):
    return (b + 7) // 8 * 8


def _formula(problems, utts, streams, assign):
    """descriptors, utterance rows, and per problem with a table L, the H candidate tables and the records."""
    total = len(problems) * _lib.ORC_DESC_BYTES + sum(p[1] for p in problems) * _lib.ORC_UTT_BYTES
    for uf, U, sf, H in problems:
        if U == 0 or H == 0:
            continue
        S = int(np.prod([streams[sf + h][1] + 1 for h in range(H)]))
        total += _r8(4 * S) + (8 * H * S + _r8(4 * S * U) if assign else _r8(4 * H * S))
    return total


def test_workspace_bytes_follow_the_stated_formula():
    lib = _lib.lib()
    assert lib.dicow_orc_distance_ws_bytes(None, 0, None, None, 0) == 0 and lib.dicow_orc_distance_ws_bytes(None, 0, None, None, 1) == 0
    utts = [(0, 3), (3, 0), (3, 9), (12, 1)]
    streams = [(0, 2), (2, 4), (6, 0), (6, 7), (13, 62)]
    tables = ([(0, 1, 0, 1)],                                              # S = 3: every r8 rounds
              [(0, 3, 0, 3), (3, 1, 3, 2)],                                # S = 15 and 8 * 63 = 504
              [(0, 2, 0, 5), (0, 0, 0, 2), (2, 1, 0, 0), (3, 1, 4, 1)])    # S = 3 * 5 * 1 * 8 * 63; no utterance; no stream; S = 63
    for problems in tables:
        for assign in (0, 1):
            got = _ws(lib, problems, utts, streams, assign)
            assert got == _formula(problems, utts, streams, assign), (problems, assign)
            assert got % 8 == 0
    assert _ws(lib, tables[0], utts, streams, 0) == 288 + 16 + 16 + 16 and _ws(lib, tables[0], utts, streams, 1) == 288 + 16 + 16 + 24 + 16


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    utts = [(0, 5), (5, 7), (12, 0)]
    streams = [(0, 6), (6, 10), (16, 3)]
    ok = [(0, 3, 0, 3), (1, 2, 1, 2)]
    many = [(0, 1)] * 9
    big_streams = [(0, 200), (0, 200), (0, 200)]                           # 201^3 > DICOW_ORC_MAX_STATES
    long_utts = [(0, 40000), (0, 30000)]
    rec_utts = [(0, 1)] * 400                                              # 400 records of 4 * 101^3 bytes > DICOW_ORC_MAX_WS_BYTES
    rec_streams = [(0, 100)] * 3
    for bad, word in (((None, -1, None, None, 0), b"negative n_problems"), ((None, 2, None, None, 0), b"null problem table")):
        assert lib.dicow_orc_distance_ws_bytes(*bad) == -1 and b"orc_distance_ws_bytes" in lib.dicow_last_error()
        assert word in lib.dicow_last_error()
    for (p, u, s, asg), word in ((([(0, 1, 0, 9)], utts, many, 0), b"DICOW_ORC_MAX_STREAMS"), (([(0, 1, 0, 3)], utts, big_streams, 0), b"DICOW_ORC_MAX_STATES"),
                                 (([(0, 2, 0, 1)], long_utts, streams, 0), b"DICOW_ORC_MAX_WORDS"), (([(0, 1, 0, 1)], [(0, 70000)], streams, 0), b"DICOW_ORC_MAX_WORDS"),
                                 (([(0, 1, 0, 1)], utts, [(0, 70000)], 0), b"DICOW_ORC_MAX_WORDS"),
                                 (([(0, 400, 0, 3)], rec_utts, rec_streams, 1), b"DICOW_ORC_MAX_WS_BYTES"),
                                 (([(0, -1, 0, 1)], utts, streams, 0), b"negative"), (([(-1, 1, 0, 1)], utts, streams, 0), b"negative"),
                                 (([(0, 1, 0, -1)], utts, streams, 0), b"negative"), (([(0, 1, 0, 1)], [(0, -4)], streams, 0), b"negative length"),
                                 (([(0, 1, 0, 1)], utts, [(0, -4)], 0), b"negative length"),
                                 (([(0, 2, 0, 1), (1, 2, 1, 1)], utts, streams, 1), b"share utterance row")):
        assert _ws(lib, p, u, s, asg) == -1, (p, word)
        assert b"orc_distance_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error(), (p, lib.dicow_last_error())
    assert _ws(lib, [(0, 400, 0, 3)], rec_utts, rec_streams, 0) > 0         # refused for its records only: without them it runs
    assert _ws(lib, [(0, 2, 0, 1), (1, 2, 1, 1)], utts, streams, 0) > 0     # shared rows are fine without an assignment
    big = dict(n_ref=1 << 20, n_hyp=1 << 20)
    for bad, word in ((dict(problems=[(0, 1, 0, 9)], streams=many), b"DICOW_ORC_MAX_STREAMS"),
                      (dict(problems=[(0, 1, 0, 3)], streams=big_streams), b"DICOW_ORC_MAX_STATES"),
                      (dict(problems=[(0, 2, 0, 1)], utts=long_utts, **big), b"DICOW_ORC_MAX_WORDS"),
                      (dict(problems=[(0, 400, 0, 3)], utts=rec_utts, streams=rec_streams, asg=5 * 4096), b"DICOW_ORC_MAX_WS_BYTES"),
                      (dict(problems=[(0, 1, 0, 1)], utts=[(998, 3)]), b"reads ref"), (dict(problems=[(0, 1, 0, 1)], utts=[(-1, 3)]), b"reads ref"),
                      (dict(problems=[(0, 1, 0, 1)], streams=[(1001, 0)]), b"reads hyp"), (dict(problems=[(0, 1, 0, 2)], streams=[(0, 5), (996, 5)]), b"stream 1 of problem 0 reads hyp"),
                      (dict(problems=ok, riv=4096), b"one side only"), (dict(problems=ok, hiv=4096), b"one side only"),
                      (dict(problems=ok, n_ref=-1), b"negative buffer"), (dict(problems=ok, n_hyp=-1), b"negative buffer"),
                      (dict(problems=ok, out=None), b"null"), (dict(problems=ok, ws=None), b"null"), (dict(problems=ok, ref=None), b"null"),
                      (dict(problems=ok, hyp=None), b"null"), (dict(problems=ok, ref=4098), b"aligned"), (dict(problems=ok, out=4097), b"aligned"),
                      (dict(problems=ok, ws=4100), b"aligned"), (dict(problems=[ok[0]], asg=4099), b"aligned"), (dict(problems=ok, riv=4096, hiv=4098), b"aligned"),
                      (dict(problems=ok, wsb=0), b"ws_bytes"), (dict(problems=ok, wsb=_ws(lib, ok, utts, streams) - 1), b"ws_bytes"),
                      (dict(problems=ok, asg=5 * 4096, wsb=_ws(lib, ok, utts, streams, 0)), b"share utterance row"),
                      (dict(problems=[ok[0]], asg=5 * 4096, wsb=_ws(lib, [ok[0]], utts, streams, 0)), b"ws_bytes"),
                      (dict(problems=ok, n=-1), b"negative n_problems")):
        kw = dict(utts=utts, streams=streams)
        kw.update(bad)
        p, u, s = kw.pop("problems"), kw.pop("utts"), kw.pop("streams")
        rc = _call(lib, p, u, s, **kw)
        assert rc == -1, bad
        assert b"orc_distance" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    assert lib.dicow_orc_distance(4096, 10, 8192, 10, None, None, None, 2, None, None, 12288, None, 16384, 1 << 20, None) == -1
    assert b"null problem table" in lib.dicow_last_error()
    # an empty table launches nothing and needs nothing
    assert _call(lib, [], [], [], ref=None, hyp=None, out=None, ws=None, wsb=0) == 0


def test_wrapper_refuses_cpu_tensors_and_bad_tables():
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.DicowError, match="GPU"):
        scoring.orc_counts(ids, ids, [(0, 1, 0, 1)], [(0, 4)], [(0, 4)])
    with pytest.raises(ValueError, match="unknown metric"):
        scoring.session_metrics([], [], ["wer"])
    with pytest.raises(ValueError, match="unknown metric"):
        scoring.aggregate_session_metrics([], ["cp_wer", "di_cp_wer"])
    with pytest.raises(ValueError, match="no reference"):
        scoring.session_tcorc_wer([("a", 0.0, 1.0, "")], [("x", 0.0, 1.0, "hello")])


def test_the_dynamic_program_is_the_minimum_over_all_assignments():
    """orc_dp == orc_brute on 60 seeded cases (H <= 3, U <= 5, <= 5 words, an alphabet of 4, every second one timed)."""
    cases = R.seeded_cases()
    assert len(cases) == 60 and sum(c[2] is not None for c in cases) == 30
    assert max(len(c[1]) for c in cases) == 3 and max(len(c[0]) for c in cases) == 5
    for k, (utts, hyps, uiv, hiv) in enumerate(cases):
        assert R.orc_dp(utts, hyps, uiv, hiv) == R.orc_brute(utts, hyps, uiv, hiv), k
    # one stream: the pair's own key; and hand-worked: "a b" + "c" against streams "a b" and "c" -> no error, 3 hits
    assert R.orc_brute([[1, 2], [3]], [[1, 2, 3]]) == R._unpack(R.pair_key([1, 2, 3], [1, 2, 3])) == (0, 3)
    assert R.orc_dp([[1, 2], [3]], [[1, 2], [3]]) == (0, 3) and R.orc_dp([[3], [1, 2]], [[1, 2, 3]]) == (2, 2)
    assert R.orc_dp([[1], [2]], []) == (2, 0) and R.orc_dp([], [[1], [2, 3]]) == (3, 0)


# ---------------------------------------------------------------------------------------------------------------- the host recipe

def test_vad_mask_truncates_like_the_reference():
    # 0.29 / 0.01 = 28.999999999999996 -> int() = 28 (not 29); 0.07 / 0.01 = 7.000000000000001 -> 7
    assert 0.29 / 0.01 < 29 and int(0.29 / 0.01) == 28
    m = scoring.create_vad_mask([("a", 0.07, 0.29, "x")], time_step=0.01)
    assert len(m) == 29 and m.dtype == bool
    assert m.tolist() == [False] * 7 + [True] * 21 + [False]
    m = scoring.create_vad_mask([{"speaker": "a", "start_time": 0.5, "end_time": 1.0, "words": "x"}, ("b", 0.2, 0.3, "y")], time_step=0.1)
    # 11 frames: int(1.0 / 0.1) + 1; 0.3 / 0.1 = 2.9999999999999996 -> 2, so the segment from 0.2 s to 0.3 s sets no frame at all
    assert m.tolist() == [False] * 5 + [True] * 5 + [False]
    m = scoring.create_vad_mask([("a", 0.0, 0.2, "x")], time_step=0.1, total_duration=0.5)
    assert m.tolist() == [True, True, False, False, False, False]
    assert scoring.create_vad_mask(scoring.create_dummy_seg_list(), time_step=0.01).tolist() == [False]


def test_group_splits_and_the_group_of_an_utterance():
    #        frame: 0 1 2 3 4 5 6 7 8 9 10 11 12 13
    vad = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0], bool)
    # group_duration 0.3 s at 0.1 s: 3 frames.  Inactive frames 1 4 5 10 12 13: 1 < 3; 4 >= 3 -> cut, next 7; 5 no; 10 >= 7 -> cut, next 13;
    # 12 no; 13 >= 13 -> cut
    assert scoring.find_group_splits(vad, group_duration=0.3, time_step=0.1) == [4, 10, 13]
    assert scoring.find_group_splits(vad, group_duration=30, time_step=0.1) == []
    assert scoring.find_group_splits(np.ones(5, bool), group_duration=0.1, time_step=0.1) == []
    splits = np.array([4, 10, 13]) * 0.1
    assert [scoring.map_utterance_to_split(t, splits) for t in (0.0, 0.39, 0.4, 0.99, 1.0, 1.29, 1.3, 5.0)] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert scoring.map_utterance_to_split(3.0, []) == 0


def test_filter_and_dummy_segment():
    segs = [("a", 0.0, 1.0, "x"), ("a", 1.0, 2.0, ""), {"speaker": "b", "start_time": 0, "end_time": 1, "words": ""}, ("b", 2.0, 3.0, " ")]
    assert scoring.filter_empty_segments(segs) == [segs[0], segs[3]]       # only the empty string is empty, as in the reference
    d = scoring.create_dummy_seg_list("s1")
    assert d == [{"session_id": "s1", "start_time": 0, "end_time": 0, "speaker": "", "words": ""}]
    assert scoring.merge_streams(d) == d


def test_merge_streams_takes_the_first_pair_in_iteration_order():
    # A and C overlap; B overlaps neither in 10 ms frames -> the first pair of the double loop is (A, B); then AB against C overlaps
    segs = [("A", 0.0, 1.0, "a1"), ("B", 1.0, 2.0, "b1"), ("C", 0.5, 0.9, "c1"), ("A", 3.0, 4.0, "a2")]
    got = scoring.merge_streams(segs)
    assert got == [("A", 0.0, 1.0, "a1"), ("C", 0.5, 0.9, "c1"), ("A", 1.0, 2.0, "b1"), ("A", 3.0, 4.0, "a2")]
    assert segs[1] == ("B", 1.0, 2.0, "b1")                                # copies: the input is left alone
    # a chain: A-B never overlap, B-C never overlap, A-C overlap.  (A, B) comes first and wins; AB-C then overlap, so C stays alone
    chain = [{"speaker": "A", "start_time": 0.0, "end_time": 1.0, "words": "a"}, {"speaker": "B", "start_time": 1.0, "end_time": 2.0, "words": "b"},
             {"speaker": "C", "start_time": 0.5, "end_time": 0.8, "words": "c"}, {"speaker": "C", "start_time": 2.0, "end_time": 3.0, "words": "c2"}]
    got = scoring.merge_streams(chain)
    assert [(s["speaker"], s["words"]) for s in got] == [("A", "a"), ("C", "c"), ("A", "b"), ("C", "c2")]
    # in the other input order C comes first: (C, B) is the first pair that never overlaps
    got = scoring.merge_streams([chain[2], chain[3], chain[1], chain[0]])
    assert [(s["speaker"], s["words"]) for s in got] == [("A", "a"), ("C", "c"), ("C", "b"), ("C", "c2")]
    # three that all merge: A + B, then AB + C
    got = scoring.merge_streams([("A", 0.0, 1.0, "a"), ("B", 2.0, 3.0, "b"), ("C", 1.0, 2.0, "c")])
    assert got == [("A", 0.0, 1.0, "a"), ("A", 1.0, 2.0, "c"), ("A", 2.0, 3.0, "b")]


def test_aggregate_session_metrics_on_two_sessions():
    a = {"cp_wer": 0.5, "cp_errors": 5, "cp_length": 10, "cp_insertions": 1, "cp_deletions": 2, "cp_substitutions": 2, "cp_missed_speaker": 1,
         "cp_falarm_speaker": 0, "cp_scored_speaker": 3, "cp_assignment": [("a", "x")],
         "tcorc_wer": 0.2, "tcorc_errors": 2, "tcorc_length": 10, "tcorc_insertions": 0, "tcorc_deletions": 1, "tcorc_substitutions": 1,
         "tcorc_assignment": ("x", "y")}
    b = {"cp_wer": 0.1, "cp_errors": 3, "cp_length": 30, "cp_insertions": 3, "cp_deletions": 0, "cp_substitutions": 0, "cp_missed_speaker": 0,
         "cp_falarm_speaker": 2, "cp_scored_speaker": 4, "cp_assignment": [],
         "tcorc_wer": 0.5, "tcorc_errors": 15, "tcorc_length": 30, "tcorc_insertions": 5, "tcorc_deletions": 5, "tcorc_substitutions": 5,
         "tcorc_assignment": ()}
    got = scoring.aggregate_session_metrics([a, b], ["cp_wer", "tcorc_wer"])
    assert got == {"cp_wer": 8 / 40, "cp_errors": 8, "cp_length": 40, "cp_insertions": 4, "cp_deletions": 2, "cp_substitutions": 2,
                   "cp_mean_missed_speaker": 0.5, "cp_mean_falarm_speaker": 1.0, "cp_mean_scored_speaker": 3.5,
                   "tcorc_wer": 17 / 40, "tcorc_errors": 17, "tcorc_length": 40, "tcorc_insertions": 5, "tcorc_deletions": 6, "tcorc_substitutions": 6}
    # a metric that is not named keeps its summed columns, its rate included, as the reference's frame does
    got = scoring.aggregate_session_metrics([a, b], ["tcorc_wer"])
    assert got["cp_wer"] == pytest.approx(0.6) and got["cp_missed_speaker"] == 1 and got["tcorc_wer"] == 17 / 40

"""CPU tests of the word-level alignments' host side: the C-ABI entry points and their binding, the refusals made before any launch, the
oracle of tests/edit_alignment_ref.py on cases worked out by hand, and the pure-Python layer (chunks, rows, the text rendering, the error
breakdown, the report) on hand-made op strings.  No GPU needed."""
import json
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import edit_alignment_ref as A
from tests import edit_distance_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, scoring  # noqa: E402

K, NARROW, WIDE = _lib.EDIT_K, _lib.EDIT_LANES_NARROW, _lib.EDIT_LANES


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_edit_alignment\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const int32_t* ref_ids", "int64_t n_ref", "const int32_t* hyp_ids", "int64_t n_hyp", "const int32_t* ref_iv",
                    "const int32_t* hyp_iv", "const int64_t* pairs", "int n_pairs", "int32_t* out", "uint8_t* ops", "int64_t* spans",
                    "int lanes", "int along", "void* ws", "int64_t ws_bytes", "void* stream"]
    # the inputs are exactly those of dicow_edit_distance, in its order
    d = re.search(r"^int\s+dicow_edit_distance\s*\(([^;]*)\);", stable, flags=re.M)
    assert [a for a in args if a not in ("uint8_t* ops", "int64_t* spans")] == [a.strip() for a in " ".join(d.group(1).split()).split(",")]
    assert re.search(r"^int64_t\s+dicow_edit_alignment_ws_bytes\s*\(\s*const int64_t\* pairs,\s*int n_pairs,\s*int lanes,\s*int along\s*\);",
                     stable, flags=re.M)
    for name, val in (("MAX_WS_BYTES", _lib.ALIGN_MAX_WS_BYTES), ("TABLE_BYTES", _lib.ALIGN_TABLE_BYTES)):
        m = re.search(rf"^#define\s+DICOW_ALIGN_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    orc = re.search(r"^#define\s+DICOW_ORC_MAX_WS_BYTES\s+(\d+)", stable, flags=re.M)
    assert int(orc.group(1)) == _lib.ALIGN_MAX_WS_BYTES == 1 << 30
    c = _lib
    assert _lib._SIGS["dicow_edit_alignment"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_vp, c.c_vp,
                                                  c.c_i, c.c_i, c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_edit_alignment_ws_bytes"] == [c.c_vp, c.c_i, c.c_i, c.c_i]
    assert {"dicow_edit_alignment", "dicow_edit_alignment_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_edit_alignment.restype is c.c_i and lib.dicow_edit_alignment_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("edit_alignments", "alignment_chunks", "alignment_rows", "word_alignments", "format_alignment", "session_alignment",
                 "error_breakdown", "save_alignment_report"):
        assert getattr(pkg, name) is getattr(scoring, name) and name in pkg.__all__


def _table(pairs):
    return np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 4))


def _size(lib, pairs, lanes=0, along=0):
    t = _table(pairs)
    return lib.dicow_edit_alignment_ws_bytes(t.ctypes.data if len(t) else None, len(t), lanes, along)


def _records(m, n, lanes):
    """The header's formula: m words along the lanes, n along the steps."""
    if m == 0 or n == 0:
        return 0
    P = lanes * K
    q = -(-m // P)
    w = -(-(m - (q - 1) * P) // K)
    return -(-2 * ((q - 1) * (n + lanes - 1) * lanes + (n + w - 1) * w) // 8) * 8


def _call(lib, pairs, **kw):
    """dicow_edit_alignment with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    t = _table(pairs)
    a = dict(ref=p, n_ref=1000, hyp=2 * p, n_hyp=1000, riv=None, hiv=None, pairs=t.ctypes.data if len(t) else None, n=len(t), out=3 * p,
             ops=5 * p, spans=6 * p, lanes=0, along=0, ws=4 * p, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = max(0, lib.dicow_edit_alignment_ws_bytes(a["pairs"], a["n"], a["lanes"] if a["lanes"] in (0, NARROW, WIDE) else 0,
                                                            a["along"] if a["along"] in (0, 1, 2) else 0))
    return lib.dicow_edit_alignment(a["ref"], a["n_ref"], a["hyp"], a["n_hyp"], a["riv"], a["hiv"], a["pairs"], a["n"], a["out"], a["ops"],
                                    a["spans"], a["lanes"], a["along"], a["ws"], a["wsb"], None)


def test_workspace_size_follows_the_stated_formula():
    lib = _lib.lib()
    T = _lib.ALIGN_TABLE_BYTES
    assert lib.dicow_edit_alignment_ws_bytes(None, 0, 0, 0) == 0
    # the narrow workgroup, ref along the lanes: one strip of 5 columns, 7 rows
    assert _size(lib, [(0, 5, 0, 7)], NARROW, 1) == T + _records(5, 7, NARROW) == T + 16
    assert _size(lib, [(0, 5, 0, 7)], NARROW, 2) == T + _records(7, 5, NARROW)
    assert _size(lib, [(0, 0, 0, 7), (0, 5, 0, 0), (0, 0, 0, 0)]) == 3 * T
    # a second panel: the boundary columns of dicow_edit_distance (16 bytes a row of the longer side) and a full panel of records
    m, n = NARROW * K + 9, 40
    assert _size(lib, [(0, m, 0, n)], NARROW, 1) == T + 16 * m + _records(m, n, NARROW)
    assert _records(m, n, NARROW) == -(-2 * ((n + NARROW - 1) * NARROW + (n + 1) * 2) // 8) * 8
    # the library's choice: fewer steps decide which sequence lies along the lanes; the wide workgroup when a shorter side needs it
    assert _size(lib, [(0, 600, 0, 30)]) == T + 16 * 600 + _records(600, 30, NARROW)           # 2 x 93 steps against 663
    assert _size(lib, [(0, 600, 0, 700)]) == T + 16 * 700 + _records(700, 600, WIDE)           # 1111 steps against 1211
    assert _size(lib, [(0, 600, 0, 700), (0, 20, 5, 30)], WIDE, 2) == 2 * T + 16 * 700 + _records(700, 600, WIDE) + _records(30, 20, WIDE)
    # sizes add up pair by pair, which the splitting wrapper relies on
    pairs = [(0, 600, 0, 700), (0, 20, 5, 30), (3, 0, 4, 9), (0, 4097, 0, 3)]
    assert _size(lib, pairs, WIDE, 0) == sum(_size(lib, [p], WIDE, 0) for p in pairs)


# Pair lists that cross each boundary of the plan, and what dicow_edit_alignment_ws_bytes returned for them -- (lanes = 0, along = 1),
# (0, 2), (0, 0), (NARROW, 0), (WIDE, 0) -- before dicow_edit_distance and dicow_edit_alignment shared one plan.  The same lists pin
# dicow_edit_distance_ws_bytes in tests/test_host_scoring.py.
PLAN_BOUNDARIES = {
    "shorter side at NARROW * K (narrow)": ([(0, NARROW * K, 0, NARROW * K + 50), (5, 7, 3, 9)], (89128, 89992, 89136, 89136, 91784)),
    "shorter side one past it (wide)": ([(0, NARROW * K + 1, 0, NARROW * K + 60), (5, 7, 3, 9)], (91968, 93392, 93392, 91344, 93392)),
    "ref_len + hyp_len at the int32 key's limit": ([(0, 30000, 0, 31439), (0, 3, 1, 4)], (240013272, 240204736, 240204736, 236766168, 240204736)),
    "one past it (int64 key)": ([(0, 30000, 0, 31440), (0, 3, 1, 4)], (240020792, 240204752, 240204752, 236773688, 240204752)),
    "empty sides": ([(0, 0, 0, 9), (0, 300, 0, 0), (0, 0, 0, 0), (2, 40, 1, 33)], (600, 664, 600, 600, 600)),
}


def test_workspace_size_at_the_plan_boundaries():
    """The header's formula with along = 1 and 2 on lists that cross narrow -> wide and the 32- -> 64-bit key or have an empty side
    (test_workspace_size_follows_the_stated_formula covers one and two panels and the library's choice of `along` on single pairs), and
    equality with the values recorded before the two plans were merged."""
    lib = _lib.lib()
    T = _lib.ALIGN_TABLE_BYTES
    assert 30000 + 31439 == 65535 - WIDE * K
    for name, (pairs, recorded) in PLAN_BOUNDARIES.items():
        lanes = WIDE if any(min(p[1], p[3]) > NARROW * K for p in pairs) else NARROW
        bnd = sum(16 * max(p[1], p[3]) for p in pairs if max(p[1], p[3]) > NARROW * K)
        for along in (1, 2):
            rec = sum(_records(p[1], p[3], lanes) if along == 1 else _records(p[3], p[1], lanes) for p in pairs)
            assert _size(lib, pairs, 0, along) == len(pairs) * T + bnd + rec, (name, along)
        got = (_size(lib, pairs, 0, 1), _size(lib, pairs, 0, 2), _size(lib, pairs, 0, 0), _size(lib, pairs, NARROW, 0), _size(lib, pairs, WIDE, 0))
        assert got == recorded, name


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    for bad, word in (((None, -1, 0, 0), b"negative n_pairs"), ((None, 2, 0, 0), b"null pair table")):
        assert lib.dicow_edit_alignment_ws_bytes(*bad) == -1 and b"edit_alignment_ws_bytes" in lib.dicow_last_error()
        assert word in lib.dicow_last_error()
    for bad, kw, word in (([(0, -1, 0, 5)], {}, b"negative length"), ([(0, _lib.EDIT_MAX_LEN + 1, 0, 5)], {}, b"DICOW_EDIT_MAX_LEN"),
                          ([(0, 5, 0, 5)], dict(lanes=128), b"lanes"), ([(0, 5, 0, 5)], dict(along=3), b"along")):
        assert _size(lib, bad, **kw) == -1 and b"edit_alignment_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error()
    # a table over the cap needs no device memory to be refused: 2 bits per cell of 40 000 x 40 000 is 400 MB a pair
    big = [(0, 40000, 0, 40000)] * 3
    assert 0 < _size(lib, big[:2]) <= _lib.ALIGN_MAX_WS_BYTES
    assert _size(lib, big) == -1 and b"DICOW_ALIGN_MAX_WS_BYTES" in lib.dicow_last_error() and b"pair 2" in lib.dicow_last_error()
    assert _size(lib, [(0, 65535, 0, 65535)]) == -1 and b"DICOW_ALIGN_MAX_WS_BYTES" in lib.dicow_last_error()
    assert _call(lib, big, n_ref=1 << 20, n_hyp=1 << 20, wsb=1 << 40) == -1 and b"DICOW_ALIGN_MAX_WS_BYTES" in lib.dicow_last_error()
    ok = [(0, 600, 0, 700), (600, 400, 100, 900)]
    need = _size(lib, ok)
    assert need > 0
    for bad, word in ((dict(pairs=[(0, -1, 0, 5)]), b"negative length"), (dict(pairs=[(-1, 5, 0, 5)]), b"reads ref"),
                      (dict(pairs=[(0, 5, -3, 5)]), b"reads hyp"), (dict(pairs=[(990, 11, 0, 5)]), b"reads ref"),
                      (dict(pairs=[(0, 5, 0, 5), (0, 5, 500, 501)]), b"pair 1 reads hyp"),
                      (dict(pairs=ok, riv=4096), b"one side only"), (dict(pairs=ok, hiv=4096), b"one side only"),
                      (dict(pairs=ok, n_ref=-1), b"negative buffer"), (dict(pairs=ok, lanes=128), b"lanes"), (dict(pairs=ok, along=3), b"along"),
                      (dict(pairs=ok, out=None), b"null"), (dict(pairs=ok, ops=None), b"null"), (dict(pairs=ok, spans=None), b"null"),
                      (dict(pairs=ok, ws=None), b"null"), (dict(pairs=ok, ref=None), b"null"), (dict(pairs=ok, hyp=None), b"null"),
                      (dict(pairs=ok, ref=4098), b"aligned"), (dict(pairs=ok, out=4097), b"aligned"), (dict(pairs=ok, spans=4100), b"aligned"),
                      (dict(pairs=ok, ws=4100), b"aligned"), (dict(pairs=ok, riv=4096, hiv=4098), b"aligned"),
                      (dict(pairs=ok, wsb=need - 1), b"ws_bytes"), (dict(pairs=ok, wsb=0), b"ws_bytes"),
                      (dict(pairs=ok, n=-1), b"negative n_pairs")):
        rc = _call(lib, **bad)
        assert rc == -1, bad
        assert b"edit_alignment" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    # an empty table launches nothing and needs nothing
    assert _call(lib, [], ref=None, hyp=None, out=None, ops=None, spans=None, ws=None, wsb=0) == 0


def test_wrapper_refuses_cpu_tensors():
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.DicowError, match="GPU"):
        scoring.edit_alignments(ids, ids, [(0, 4, 0, 4)])
    with pytest.raises(_lib.DicowError, match="GPU"):
        scoring.edit_alignments(np.zeros(4, np.int32), ids, [(0, 4, 0, 4)])
    with pytest.raises(ValueError):
        scoring.word_alignments(["a"], ["a", "b"])


def test_oracle_on_cases_worked_out_by_hand():
    # one substitution between two hits
    assert A.align([1, 2, 3], [1, 9, 3]) == ((1, 2), [A.HIT, A.SUB, A.HIT])
    # ref 0 1 0 against hyp 1 2 1.  D[2][2] = D[2][3] = D[3][2] = (2, -1), so at (3, 3) the substitution, the deletion and the insertion
    # all give (3, -1): the diagonal goes first.  At (2, 2) only the insertion from D[2][1] = (1, -1) attains (2, -1); (2, 1) is the hit
    # of the two 1s from D[1][0]; column 0 leaves the deletion.
    D = A.table([0, 1, 0], [1, 2, 1])
    assert D[2][2] == D[2][3] == D[3][2] == (2, -1) and D[3][3] == (3, -1) and D[2][1] == (1, -1) and D[1][2] == (2, 0)
    assert A.align([0, 1, 0], [1, 2, 1]) == ((3, 1), [A.DEL, A.HIT, A.INS, A.SUB])
    # deletion before insertion where the diagonal is closed: touching intervals do not overlap
    assert A.align([7], [7], [(0, 5)], [(5, 9)]) == ((2, 0), [A.INS, A.DEL])
    assert A.align([7], [7], [(0, 5)], [(4, 9)]) == ((0, 1), [A.HIT])
    # S + S would keep no hit: D + I around the hit of the 1s; walking back the deletion is preferred, so it stands last
    assert A.align([0, 1], [1, 0]) == ((2, 1), [A.INS, A.HIT, A.DEL])
    # empty sides
    assert A.align([], []) == ((0, 0), []) and A.align([], [4, 4]) == ((2, 0), [A.INS, A.INS]) and A.align([4], []) == ((1, 0), [A.DEL])
    # the counts are those of the counting oracle, and the checker accepts the path
    rng = np.random.default_rng(21)
    for case in range(60):
        ref, hyp = rng.integers(0, 3, int(rng.integers(0, 10))).tolist(), rng.integers(0, 3, int(rng.integers(0, 10))).tolist()
        riv = hiv = None
        if case % 2:
            b = rng.integers(0, 20, len(ref))
            riv = np.stack([b, b + rng.integers(0, 6, len(ref))], 1).tolist()
            b = rng.integers(0, 20, len(hyp))
            hiv = np.stack([b, b + rng.integers(0, 6, len(hyp))], 1).tolist()
        (e, h), ops = A.align(ref, hyp, riv, hiv)
        assert (e, h) == R.dp_loops(ref, hyp, riv, hiv)
        assert A.check_ops(ref, hyp, ops, riv, hiv) == (e, h) + R.sdi(e, h, len(ref), len(hyp))
    with pytest.raises(AssertionError):
        A.check_ops([1, 2], [1, 3], [A.HIT, A.HIT])
    with pytest.raises(AssertionError):
        A.check_ops([1, 2], [1], [A.HIT])


def test_chunks_merge_runs_of_one_type():
    assert scoring.OPS == ("equal", "substitute", "delete", "insert")
    assert scoring.alignment_chunks([]) == []
    assert scoring.alignment_chunks([0, 0, 1, 2, 2, 3, 0]) == [("equal", 0, 2, 0, 2), ("substitute", 2, 3, 2, 3), ("delete", 3, 5, 3, 3),
                                                              ("insert", 5, 5, 3, 4), ("equal", 5, 6, 4, 5)]
    assert scoring.alignment_chunks(torch.tensor([3, 3, 1, 1], dtype=torch.uint8)) == [("insert", 0, 0, 0, 2), ("substitute", 0, 2, 2, 4)]
    assert scoring.alignment_chunks(np.array([2], np.uint8)) == [("delete", 0, 1, 0, 0)]


def test_rows_and_the_text_rendering():
    ref, hyp, ops = ["the", "cat", "sat", "down"], ["the", "black", "cat", "sits"], [0, 3, 0, 1, 2]
    rows = scoring.alignment_rows(ref, hyp, ops)
    assert rows == [("equal", "the", None, None, "the", None, None), ("insert", None, None, None, "black", None, None),
                    ("equal", "cat", None, None, "cat", None, None), ("substitute", "sat", None, None, "sits", None, None),
                    ("delete", "down", None, None, None, None, None)]
    timed = scoring.alignment_rows(["a"], ["b", "c"], [1, 3], [(1000, 2500)], [(-500, 500), (0, 1000)])
    assert timed == [("substitute", "a", 1.0, 2.5, "b", -0.5, 0.5), ("insert", None, None, None, "c", 0.0, 1.0)]
    with pytest.raises(ValueError):
        scoring.alignment_rows(ref, hyp, [0, 0, 0, 0, 0])
    text = scoring.format_alignment(ref, hyp, ops)
    assert text.split("\n") == ["REF: the ***** cat sat  down",
                                "HYP: the black cat sits ****",
                                "         I         S    D"]
    assert scoring.format_alignment([], [], []) == "REF:\nHYP:\n"


def test_error_breakdown_is_sorted_by_count_then_lexicographically(tmp_path):
    rows = (scoring.alignment_rows(["a", "b", "a", "z", "q"], ["c", "b", "c", "y"], [1, 0, 1, 1, 2])
            + scoring.alignment_rows(["q", "k", "b"], ["b", "u", "u"], [2, 2, 0, 3, 3])
            + scoring.alignment_rows(["a", "z"], ["b", "y"], [1, 1]))
    b = scoring.error_breakdown(rows)
    assert b == {"substitutions": [(("a", "c"), 2), (("z", "y"), 2), (("a", "b"), 1)], "deletions": [("q", 2), ("k", 1)],
                 "insertions": [("u", 2)]}
    assert scoring.error_breakdown(rows, top=1) == {"substitutions": [(("a", "c"), 2)], "deletions": [("q", 2)], "insertions": [("u", 2)]}
    assert scoring.error_breakdown([]) == {"substitutions": [], "deletions": [], "insertions": []}
    # a session's dictionary, and the report written from it
    session = {"errors": 3, "assignment": [("A", "x"), (None, "y")], "speakers": [
        {"ref_speaker": "A", "hyp_speaker": "x", "rows": scoring.alignment_rows(["a", "b"], ["c"], [1, 2], [(0, 10), (10, 20)], [(5, 5)])},
        {"ref_speaker": None, "hyp_speaker": "y", "rows": scoring.alignment_rows([], ["u"], [3], [], [(7, 9)])}]}
    assert scoring.error_breakdown(session) == {"substitutions": [(("a", "c"), 1)], "deletions": [("b", 1)], "insertions": [("u", 1)]}
    path = tmp_path / "session.json"
    scoring.save_alignment_report(session, path)
    back = json.loads(path.read_text())
    assert back["breakdown"] == {"substitutions": [["a", "c", 1]], "deletions": [["b", 1]], "insertions": [["u", 1]]}
    assert back["speakers"][0]["rows"] == [["substitute", "a", 0.0, 0.01, "c", 0.005, 0.005], ["delete", "b", 0.01, 0.02, None, None, None]]
    assert back["speakers"][1]["ref_speaker"] is None and back["assignment"] == [["A", "x"], [None, "y"]] and back["errors"] == 3

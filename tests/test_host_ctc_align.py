"""CPU tests of CTC forced alignment's host side: the oracle of tests/ctc_align_ref.py on cases worked out by hand and against
torch.nn.functional.ctc_loss, the C-ABI entry points and their binding, every refusal made before any launch (with never-dereferenced
device pointers), and the pure-Python layer (the word-grouping rule on a stub tokenizer, SegLST words).  No GPU needed."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import amd_pkg
from tests import ctc_align_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, ctc_align  # noqa: E402

NEG = R.NEG


def zeros(F, C):
    return [[0] * C for _ in range(F)]


def test_oracle_on_cases_worked_out_by_hand():
    # L = 0: the all-blank path, whatever the other columns hold
    x = [[-1, 5], [-2, 5], [-4, 5]]
    assert R.align_scalar(x, [], 0) == dict(status=0, score=-7, path=[0, 0, 0], spans=[], token_score=[])
    assert R.align_scalar([], [], 0) == dict(status=0, score=0, path=[], spans=[], token_score=[])
    assert R.align_scalar([], [1], 0)["status"] == 1
    # a repeated label forces a blank: L + 1 frames at least, and then the one path 1 0 1
    x = [[-9, -1], [-3, -9], [-9, -2]]
    assert R.align_scalar(x, [1, 1], 0) == dict(status=0, score=-6, path=[1, 0, 1], spans=[[0, 1], [2, 3]], token_score=[-1, -2])
    assert R.align_scalar(x[:2], [1, 1], 0) == dict(status=1, score=NEG, path=[-1, -1], spans=[[-1, -1]] * 2, token_score=[0, 0])
    # the minimum feasible F = L + adjacent equal targets: 1 2 2 3 needs 5 frames
    assert R.align_scalar(zeros(5, 4), [1, 2, 2, 3], 0)["path"] == [1, 2, 0, 2, 3]
    assert R.align_scalar(zeros(4, 4), [1, 2, 2, 3], 0)["status"] == 1
    assert R.align_scalar(zeros(3, 4), [1, 2, 3], 0)["path"] == [1, 2, 3] and R.align_scalar(zeros(2, 4), [1, 2, 3], 0)["status"] == 1
    # stay beats s - 1, and at the end 2L wins only if strictly greater: all zeros, y = [1], F = 2.  v[0] = (0, 0, -inf); at frame 1 state 1
    # can stay (0) or come from the blank (0): it stays; the end states 1 and 2 both hold 0: the label's wins.
    assert R.align_scalar(zeros(2, 2), [1], 0) == dict(status=0, score=0, path=[1, 1], spans=[[0, 2]], token_score=[0])
    # ... strictly greater: the blank of the last frame is worth 1
    assert R.align_scalar([[0, 0], [1, 0]], [1], 0) == dict(status=0, score=1, path=[1, 0], spans=[[0, 1]], token_score=[0])
    # stay beats s - 1 beats s - 2: all zeros, y = [1, 2], F = 3.  Frame 1: v = (0, 0, 0, 0, -inf), state 3 reached by the skip from 1.  Frame
    # 2: state 3 can stay, come from the blank 2 or skip from 1, all 0: it stays.  End: 3 (not strictly less than 4).  So 1 2 2.
    assert R.align_scalar(zeros(3, 3), [1, 2], 0) == dict(status=0, score=0, path=[1, 2, 2], spans=[[0, 1], [1, 3]], token_score=[0, 0])
    # s - 1 beats s - 2: label 2 costs 1 at frame 1, so at frame 2 staying in 3 gives -1 and both the blank (state 2) and the skip (state 1)
    # give 0: the blank's path 1 0 2 wins over 1 1 2
    x = zeros(3, 3)
    x[1][2] = -1
    assert R.align_scalar(x, [1, 2], 0) == dict(status=0, score=0, path=[1, 0, 2], spans=[[0, 1], [2, 3]], token_score=[0, 0])
    # no skip between equal labels even where it would pay: 1 1 over 3 frames must pass the blank, however bad
    x = [[0, 0], [-50, 0], [0, 0]]
    assert R.align_scalar(x, [1, 1], 0)["path"] == [1, 0, 1]
    # -inf is a legal score: a target whose column is -inf everywhere is infeasible through its end states
    x = [[0, 0, NEG], [0, 0, NEG], [0, 0, NEG]]
    assert R.align_scalar(x, [1, 2], 0)["status"] == 1 and R.align_scalar(x, [1], 0)["status"] == 0
    # token scores add over the token's own frames only
    x = [[-9, -2, -9], [-9, -3, -9], [-4, -9, -9], [-9, -9, -5]]
    assert R.align_scalar(x, [1, 2], 0) == dict(status=0, score=-14, path=[1, 1, 0, 2], spans=[[0, 2], [3, 4]], token_score=[-5, -5])


def test_vectorised_oracle_equals_the_scalar_one():
    rng = np.random.default_rng(5)
    for case in range(120):
        C, F, L = int(rng.integers(2, 6)), int(rng.integers(0, 14)), int(rng.integers(0, 6))
        blank = int(rng.integers(0, C))
        y = [int(t) for t in rng.choice([c for c in range(C) if c != blank], L)]
        xi = rng.integers(-4, 1, (F, C))
        if case % 3 == 0 and F:
            xi[rng.integers(0, F), rng.integers(0, C)] = R.NEG_INT
        xs = [[NEG if t == R.NEG_INT else int(t) for t in row] for row in xi]
        want = R.align_scalar(xs, y, blank)
        assert R.align(xi.astype(np.int64), y, blank) == want, case
        xf = np.where(xi == R.NEG_INT, -np.inf, xi.astype(np.float64))
        assert R.align(xf, y, blank) == want, case
        if want["status"] == 0:
            R.check_path(want["path"], y, blank)
            assert R.rescore(xf, want["path"]) == want["score"]
    with pytest.raises(AssertionError):
        R.check_path([1, 1, 0, 2], [1, 1, 2], 0)
    assert R.collapse([3, 3, 0, 3, 1, 0, -1, -1], 0) == [3, 3, 1]


def test_the_trellis_is_ctcs_own():
    """On log-probabilities peaked so sharply that one path carries the mass, the best path's total is -ctc_loss to fp64 rounding."""
    g = torch.Generator().manual_seed(3)
    for y, path in (([1, 2, 2, 3], [0, 1, 1, 2, 0, 2, 3, 3, 0]), ([4], [4, 4, 4]), ([], [0, 0]), ([2, 1, 2], [2, 1, 2])):
        F, C = len(path), 5
        logits = torch.rand(F, C, generator=g, dtype=torch.float64)
        logits[torch.arange(F), torch.tensor(path)] += 60.0
        lp = torch.log_softmax(logits, -1)
        got = R.align(lp.numpy(), y, 0)
        assert got["status"] == 0 and got["path"] == path
        loss = torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor([y], dtype=torch.long).reshape(1, len(y)), torch.tensor([F]),
                                            torch.tensor([len(y)]), blank=0, reduction="none", zero_infinity=False)
        assert abs(got["score"] + float(loss[0])) < 1e-12 * max(1.0, abs(got["score"])), (y, got["score"], float(loss[0]))


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_ctc_forced_align\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const void* logits", "int in_bf16", "int B", "int T", "int V1", "int64_t ld", "const float* lse", "const int32_t* alias",
                    "int blank", "const int64_t* table", "int n", "const int32_t* targets", "int64_t n_targets", "int32_t* path", "int Fmax",
                    "int32_t* spans", "int Lmax", "float* token_score", "float* score", "int32_t* status", "int plan", "void* ws",
                    "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_ctc_align_ws_bytes\s*\(\s*const int64_t\* table,\s*int n\s*\);", stable, flags=re.M)
    for name, val in (("MAX_L", _lib.CTC_ALIGN_MAX_L), ("MAX_WS_BYTES", _lib.CTC_ALIGN_MAX_WS_BYTES), ("PROB_BYTES", _lib.CTC_ALIGN_PROB_BYTES)):
        m = re.search(rf"^#define\s+DICOW_CTC_ALIGN_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert 2 * _lib.CTC_ALIGN_MAX_L + 1 <= 1024 and _lib.CTC_ALIGN_MAX_WS_BYTES == 1 << 30
    # the tie rule stands in the header, as the project's own
    assert "THE TIE RULE is the project's own" in stable and "wins over 2 L - 1 only if strictly greater" in stable
    c = _lib
    assert _lib._SIGS["dicow_ctc_forced_align"] == [c.c_vp, c.c_i, c.c_i, c.c_i, c.c_i, c.c_i64, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_i, c.c_vp,
                                                    c.c_i64, c.c_vp, c.c_i, c.c_vp, c.c_i, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_ctc_align_ws_bytes"] == [c.c_vp, c.c_i]
    assert {"dicow_ctc_forced_align", "dicow_ctc_align_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_ctc_forced_align.restype is c.c_i and lib.dicow_ctc_align_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("CtcAlignment", "ctc_forced_align", "token_timestamps", "word_timestamps", "align_segments", "words_as_segments"):
        assert getattr(pkg, name) is getattr(ctc_align, name) and name in pkg.__all__


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 5))


def _size(lib, rows):
    t = _table(rows)
    return lib.dicow_ctc_align_ws_bytes(t.ctypes.data if len(t) else None, len(t))


def _formula(rows):
    """The header's formula."""
    up = lambda v, m: -(-v // m) * m                                      # noqa: E731
    need = up(len(rows) * _lib.CTC_ALIGN_PROB_BYTES + 4 * sum(r[4] for r in rows), 16)
    for _, _, F, _, L in rows:
        bp = 4 * -(-(2 * L + 1) // 16)
        if L <= 63:
            bp = max(bp, up(L + 1, 4))
        need += 4 * F * (up(L, 8) + 4) + up(F * bp, 16)
    return need


def test_workspace_size_follows_the_stated_formula():
    lib = _lib.lib()
    assert lib.dicow_ctc_align_ws_bytes(None, 0) == 0
    for rows in ([(0, 0, 10, 0, 3)], [(0, 0, 0, 0, 0)], [(0, 0, 1, 0, 0), (1, 5, 7, 0, 63), (0, 0, 1500, 63, 64), (0, 0, 33, 0, 511)],
                 [(0, 0, 375, 0, 40)] * 7):
        assert _size(lib, rows) == _formula(rows), rows
    assert _size(lib, [(0, 0, 10, 0, 3)]) == 80 + 10 * 12 * 4 + 48      # one problem and three targets in 80 bytes; E; 10 rows of 4 bytes


def _call(lib, rows, **kw):
    """dicow_ctc_forced_align with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    t = _table(rows)
    tg = np.ascontiguousarray(np.asarray(kw.pop("targets", np.arange(1, 601) % 9 + 1), np.int32))
    a = dict(logits=p, bf=1, B=2, T=100, V1=10, ld=16, lse=2 * p, alias=None, blank=0, n=len(t), n_targets=len(tg), path=3 * p, Fmax=100,
             spans=4 * p, Lmax=511, ts=5 * p, score=6 * p, status=7 * p, plan=0, ws=8 * p, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = max(0, lib.dicow_ctc_align_ws_bytes(t.ctypes.data if len(t) else None, len(t)))
    return lib.dicow_ctc_forced_align(a["logits"], a["bf"], a["B"], a["T"], a["V1"], a["ld"], a["lse"], a["alias"], a["blank"],
                                      t.ctypes.data if len(t) else None, a["n"], tg.ctypes.data if len(tg) else None, a["n_targets"], a["path"],
                                      a["Fmax"], a["spans"], a["Lmax"], a["ts"], a["score"], a["status"], a["plan"], a["ws"], a["wsb"], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    for bad, word in (((None, -1), b"negative n"), ((None, 2), b"null problem table")):
        assert lib.dicow_ctc_align_ws_bytes(*bad) == -1 and b"ctc_align_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error()
    for bad, word in (([(0, 0, -1, 0, 3)], b"2^31"), ([(0, 0, 1 << 31, 0, 3)], b"2^31"), ([(0, 0, 5, 0, -1)], b"DICOW_CTC_ALIGN_MAX_L"),
                      ([(0, 0, 5, 0, 512)], b"DICOW_CTC_ALIGN_MAX_L")):
        assert _size(lib, bad) == -1 and b"ctc_align_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error(), bad
    # a workspace over the limit needs no device memory to be refused: 2000 frames of 511 targets are 4.6 MB a problem
    big = [(0, 0, 2000, 0, 511)] * 300
    assert 0 < _size(lib, big[:200]) <= _lib.CTC_ALIGN_MAX_WS_BYTES
    assert _size(lib, big) == -1 and b"DICOW_CTC_ALIGN_MAX_WS_BYTES" in lib.dicow_last_error() and b"split the call" in lib.dicow_last_error()
    assert _call(lib, big, T=2000, Fmax=2000, wsb=1 << 40) == -1 and b"DICOW_CTC_ALIGN_MAX_WS_BYTES" in lib.dicow_last_error()
    ok = [(0, 0, 100, 0, 5), (1, 40, 60, 5, 511)]
    need = _size(lib, ok)
    assert need > 0
    for bad, word in ((dict(rows=[(2, 0, 10, 0, 3)]), b"reads row 2 of logits with B = 2"), (dict(rows=[(-1, 0, 10, 0, 3)]), b"reads row -1"),
                      (dict(rows=[(0, 95, 6, 0, 3)]), b"past the T = 100"), (dict(rows=[(0, -1, 6, 0, 3)]), b"past the T = 100"),
                      (dict(rows=[(0, 0, 5, 0, 3), (0, 101, 0, 0, 3)]), b"problem 1 reads frames"),
                      (dict(rows=[(0, 0, 10, 0, 3)], targets=[4, 0, 5]), b"target 1 of problem 0 is the blank"),
                      (dict(rows=[(0, 0, 10, 0, 3)], targets=[4, 5, 10]), b"target 2 of problem 0 is 10, outside [0, V1 = 10)"),
                      (dict(rows=[(0, 0, 10, 0, 3)], targets=[-1, 5, 6]), b"outside [0, V1 = 10)"),
                      (dict(rows=[(0, 0, 10, 598, 3)]), b"reads targets"), (dict(rows=[(0, 0, 10, -1, 3)]), b"reads targets"),
                      (dict(rows=[(0, 0, 100, 0, 512)]), b"DICOW_CTC_ALIGN_MAX_L"),
                      (dict(rows=ok, plan=3), b"plan"), (dict(rows=ok, plan=1), b"narrow plan takes at most 63"),
                      (dict(rows=ok, blank=10), b"blank"), (dict(rows=ok, blank=-1), b"blank"), (dict(rows=ok, ld=9), b"ld >= V1"),
                      (dict(rows=ok, V1=0), b"ld >= V1"), (dict(rows=ok, Fmax=99), b"Fmax"), (dict(rows=ok, Lmax=510), b"Lmax"),
                      (dict(rows=ok, logits=None), b"null"), (dict(rows=ok, path=None), b"null"), (dict(rows=ok, spans=None), b"null"),
                      (dict(rows=ok, ts=None), b"null"), (dict(rows=ok, score=None), b"null"), (dict(rows=ok, status=None), b"null"),
                      (dict(rows=ok, ws=None), b"null"), (dict(rows=ok, logits=4097), b"aligned"), (dict(rows=ok, lse=4098), b"aligned"),
                      (dict(rows=ok, alias=4098), b"aligned"), (dict(rows=ok, path=4098), b"aligned"), (dict(rows=ok, ws=4104), b"aligned"),
                      (dict(rows=ok, wsb=need - 1), b"ws_bytes"), (dict(rows=ok, wsb=0), b"ws_bytes"), (dict(rows=ok, n=-1), b"negative n"),
                      (dict(rows=ok, n_targets=-1), b"n_targets")):
        rc = _call(lib, **bad)
        assert rc == -1, bad
        assert b"ctc_forced_align" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    # an empty table launches nothing and needs nothing
    assert _call(lib, [], logits=None, path=None, spans=None, ts=None, score=None, status=None, ws=None, wsb=0) == 0


def test_wrapper_refuses_what_it_cannot_run():
    x = torch.zeros(1, 4, 5)
    with pytest.raises(_lib.DicowError, match="GPU"):
        ctc_align.ctc_forced_align(x, [[1]], blank=0)
    with pytest.raises(_lib.DicowError, match="GPU"):
        ctc_align.ctc_forced_align(x.numpy(), [[1]], blank=0)
    model = SimpleNamespace(config=SimpleNamespace(ctc_weight=0.0), tokenizer=object())
    with pytest.raises(_lib.DicowError, match="ctc_weight"):
        ctc_align.align_segments(model, x, None, [[]])
    model = SimpleNamespace(config=SimpleNamespace(ctc_weight=0.3), tokenizer=None)
    with pytest.raises(_lib.DicowError, match="set_tokenizer"):
        ctc_align.align_segments(model, x, None, [[]])


class ByteTokenizer:
    """decode() the way a byte-level BPE tokenizer does: the tokens' bytes joined, invalid UTF-8 replaced by U+FFFD."""

    def __init__(self, pieces):
        self.pieces = [p if isinstance(p, bytes) else p.encode() for p in pieces]

    def decode(self, ids):
        return b"".join(self.pieces[i] for i in ids).decode("utf-8", errors="replace")


def test_word_grouping_rule():
    e = "é".encode()                                                      # two bytes, split over the tokens 5 and 6
    tok = ByteTokenizer([" the", " c", "at", " sat", ".", b" caf" + e[:1], e[1:], "s", " ", "Hello"])
    t = lambda i, s, e_, lp: (i, s, e_, lp)                               # noqa: E731
    import math
    # a word starts at the first token (no leading space needed) and at every token that decodes with a leading space
    words = ctc_align.word_timestamps(tok, [t(9, 0.0, 0.1, -0.1), t(0, 0.2, 0.3, -0.2), t(1, 0.5, 0.6, -0.4), t(2, 0.6, 0.9, -0.6),
                                            t(3, 1.0, 1.2, -1.0), t(4, 1.2, 1.3, -3.0)])
    assert [(w, s, e_) for w, s, e_, _ in words] == [("Hello", 0.0, 0.1), ("the", 0.2, 0.3), ("cat", 0.5, 0.9), ("sat.", 1.0, 1.3)]
    assert [round(math.log(c), 12) for _, _, _, c in words] == [-0.1, -0.2, -0.5, -2.0]
    # an incomplete UTF-8 sequence joins the token after it; the word goes on behind it
    words = ctc_align.word_timestamps(tok, [t(0, 0.0, 0.1, -1.0), t(5, 0.2, 0.4, -1.0), t(6, 0.4, 0.5, -1.0), t(7, 0.5, 0.6, -1.0)])
    assert [(w, s, e_) for w, s, e_, _ in words] == [("the", 0.0, 0.1), ("cafés", 0.2, 0.6)]
    # ... at the very end there is nothing to join: the replacement character stays
    words = ctc_align.word_timestamps(tok, [t(5, 0.2, 0.4, -1.0)])
    assert len(words) == 1 and words[0][0].startswith("caf") and words[0][1:3] == (0.2, 0.4)
    # white space alone is no word
    assert ctc_align.word_timestamps(tok, [t(8, 0.0, 0.1, -1.0)]) == [] and ctc_align.word_timestamps(tok, []) == []
    words = ctc_align.word_timestamps(tok, [t(0, 0.0, 0.1, -1.0), t(8, 0.1, 0.2, -1.0), t(3, 0.2, 0.3, -1.0)])
    assert [w for w, *_ in words] == ["the", "sat"]


def test_words_as_segments_are_seglst():
    segs = [dict(start=1.0, end=2.0, tokens=[1, 2], aligned=True, words=[("a", 1.1, 1.3, 0.9), ("b", 1.5, 1.9, 0.8)]),
            dict(start=3.0, end=4.0, tokens=[], aligned=True, words=[]),
            dict(start=5.0, end=6.0, tokens=[3], aligned=False, words=[("c", 5.0, 6.0, None)])]
    assert ctc_align.words_as_segments(segs, "spk") == [
        {"speaker": "spk", "start_time": 1.1, "end_time": 1.3, "words": "a"}, {"speaker": "spk", "start_time": 1.5, "end_time": 1.9, "words": "b"},
        {"speaker": "spk", "start_time": 5.0, "end_time": 6.0, "words": "c"}]
    assert ctc_align.words_as_segments(segs[:1], 3, session_id="s1")[0] == {"speaker": 3, "start_time": 1.1, "end_time": 1.3, "words": "a",
                                                                           "session_id": "s1"}
    ali = ctc_align.CtcAlignment(torch.tensor([[4, 4, 9, 7], [-1, -1, -1, -1]], dtype=torch.int32),
                                 torch.tensor([[[0, 2], [3, 4]], [[-1, -1], [-1, -1]]], dtype=torch.int32),
                                 torch.tensor([[-1.0, -0.5], [0.0, 0.0]]), torch.tensor([-2.0, float("-inf")]), torch.tensor([True, False]))
    got = ctc_align.token_timestamps(ali, 0.02, [10.0, 0.0])
    assert got[1] is None and [t[0] for t in got[0]] == [4, 7]
    assert [t[1:] for t in got[0]] == [pytest.approx((10.0, 10.04, -0.5), abs=1e-12), pytest.approx((10.06, 10.08, -0.5), abs=1e-12)]

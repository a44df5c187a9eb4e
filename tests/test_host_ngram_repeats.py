"""CPU tests of the hypothesis clean-up's host side: the oracle of tests/ngram_repeats_ref.py against golden F26 (the reference's own
truncate_at_repeating_ngram) and on reasons worked out by hand, the C-ABI entry points and their binding, every refusal made before any
launch (with never-dereferenced device pointers), and session_hypotheses on a stub tokenizer without truncation.  No GPU needed."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import ngram_repeats_ref as R
from tests.util import ROOT, load_golden

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, hyp_cleanup  # noqa: E402


def f26():
    z = load_golden("f26_ngram_repeats")
    for text, p, out in zip(z["texts"], z["params"], z["outs"]):
        nl, mn, mx, mw, u, r = (int(v) for v in p)
        yield str(text), dict(ngram_length=nl, min_n=mn, max_n=None if mx < 0 else mx, min_word_threshold=mw, unigram_min_repeat=u,
                              repeat_threshold=r), str(out)


def test_oracle_equals_the_reference_on_every_recorded_case():
    cases = list(f26())
    cut = 0
    for text, kw, want in cases:
        got, reason = R.truncate(text, **kw)
        assert got == want, (text, kw)
        assert (reason == (0, 0, 0)) == (want == text), (text, kw, reason)
        cut += want != text
    assert len(cases) >= 200 and 3 * cut >= len(cases) and 3 * (len(cases) - cut) >= len(cases)
    # the cases stated with the definition
    hand = {t: o for t, kw, o in cases if kw == dict(ngram_length=10, min_n=1, max_n=None, min_word_threshold=30, unigram_min_repeat=10,
                                                     repeat_threshold=10)}
    assert hand["a " * 29] == "a " * 29 and hand["a " * 30] == "a"
    assert len(hand[" ".join(f"w{k}" for k in range(25)) + " " + "a a b " * 11].split()) == 28


def ids_of(text):
    return R.word_ids(text.split())


def test_oracle_reasons_on_cases_worked_out_by_hand():
    small = dict(min_words=0, u=2, r=1)
    # below min_words nothing is looked at; a run of 30 is reported in full
    assert R.cut(*ids_of("a " * 29)) == (29, (0, 0, 0))
    assert R.cut(*ids_of("a " * 30)) == (1, (1, 0, 30))
    # 25 words, then "a a b" x 11: the trigram at 25 and the bigram "a b" at 26 both end at 28, both 11 times: the smaller n is named
    assert R.cut(*ids_of(" ".join(f"w{k}" for k in range(25)) + " " + "a a b " * 11)) == (28, (2, 26, 11))
    # the full run, not capped at u
    assert R.cut(*ids_of(" ".join(f"w{k}" for k in range(20)) + " z" * 14 + " tail")) == (21, (1, 20, 14))
    # a run of u - 1 does not cut, a count of r does not cut
    assert R.cut(*ids_of(" ".join(f"w{k}" for k in range(25)) + " z" * 9)) == (34, (0, 0, 0))
    assert R.cut(*ids_of(" ".join(f"w{k}" for k in range(30)) + " p q" * 10)) == (50, (0, 0, 0))
    assert R.cut(*ids_of(" ".join(f"w{k}" for k in range(30)) + " p q" * 11)) == (32, (2, 30, 11))
    # the unigram rule wins a tie: "b a a b a" -- the run "a a" at 1 keeps 2 words, and so does the bigram "b a" at 0 (twice)
    assert R.cut(*ids_of("b a a b a"), **small) == (2, (1, 1, 2))
    assert R.cut(*ids_of("b a a b a"), min_n=2, **small) == (2, (2, 0, 2))
    # then the smallest n: "a a b a a b" without the unigram rule -- "a a" is degenerate, "a a b" at 0 and "a b" at 1 both end at 3
    assert R.cut(*ids_of("a a b a a b"), min_n=2, **small) == (3, (2, 1, 2))
    assert R.cut(*ids_of("a a b a a b"), min_n=3, **small) == (3, (3, 0, 2))
    assert R.cut(*ids_of("a a b a a b"), **small) == (1, (1, 0, 2))
    # overlapping occurrences count: "a b" x 16 holds "a b a" 15 times
    assert R.cut(*ids_of("a b " * 16), min_n=3, r=14) == (3, (3, 0, 15))
    assert R.cut(*ids_of("a b " * 16), min_n=3, r=15) == (32, (0, 0, 0))
    # counts are case-sensitive, the degenerate test and the run are not
    assert R.cut(*ids_of("A b a b"), **small) == (4, (0, 0, 0))
    assert R.cut(*ids_of("Yes yes x Yes yes x"), min_n=2, **small) == (3, (2, 1, 2))
    assert R.cut(*ids_of("x Yes yEs YES"), min_words=0, u=3) == (2, (1, 1, 3))
    # a candidate that ends at W cuts nothing
    assert R.cut(*ids_of("a"), min_words=0, u=1) == (1, (0, 0, 0))
    assert R.cut(*ids_of("a b"), min_words=0, u=1) == (1, (1, 0, 1))
    assert R.cut(*ids_of("a b a b"), min_n=2, max_n=2, min_words=0, r=1) == (2, (2, 0, 2))
    assert R.cut(*ids_of("x y a b a b"), min_n=4, max_n=4, min_words=0, r=0) == (4, (4, 0, 1))
    assert R.cut(*ids_of("x y a b"), min_n=4, max_n=4, min_words=0, r=0) == (4, (0, 0, 0))
    assert R.cut([], []) == (0, (0, 0, 0)) and R.cut([], [], min_words=0) == (0, (0, 0, 0))
    # max_n below max(2, min_n): no n-gram rule at all
    assert R.cut(*ids_of("a b " * 20), min_n=3, max_n=2) == (40, (0, 0, 0))


def test_string_front_of_the_package_splits_and_folds_as_the_oracle_does():
    texts = ["Yes yes\tİ  ß SS", "", "  a A a\n"]
    words, flat, fold, table = hyp_cleanup.word_ids(texts)
    assert words == [["Yes", "yes", "İ", "ß", "SS"], [], ["a", "A", "a"]] and table.tolist() == [[0, 5], [5, 0], [5, 3]]
    assert flat.dtype == np.int32 and fold.dtype == np.int32
    allw = [w for ws in words for w in ws]
    for i in range(len(allw)):
        for j in range(len(allw)):
            assert (flat[i] == flat[j]) == (allw[i] == allw[j]) and (fold[i] == fold[j]) == (allw[i].lower() == allw[j].lower())
    assert hyp_cleanup.word_ids([])[3].shape == (0, 2)


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_ngram_repeats\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const int32_t* ids", "const int32_t* fold", "int64_t n_words", "const int64_t* table", "int n", "int min_n", "int max_n",
                    "int min_words", "int unigram_min_repeat", "int repeat_threshold", "int32_t* keep", "int32_t* reason", "int plan", "void* ws",
                    "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_ngram_repeats_ws_bytes\s*\(\s*const int64_t\* table,\s*int n,\s*int plan\s*\);", stable, flags=re.M)
    for name, val in (("MAX_N", _lib.NGRAM_MAX_N), ("MAX_WORDS", _lib.NGRAM_MAX_WORDS), ("PLANS", _lib.NGRAM_PLANS), ("MAX_WS_BYTES", _lib.NGRAM_MAX_WS_BYTES),
                      ("SEG_BYTES", _lib.NGRAM_SEG_BYTES), ("ITEM_BYTES", _lib.NGRAM_ITEM_BYTES)):
        m = re.search(rf"^#define\s+DICOW_NGRAM_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.NGRAM_MAX_N >= 16 and _lib.NGRAM_MAX_WORDS >= 65535 and sorted(_lib.NGRAM_PLAN_TILES) == list(range(1, _lib.NGRAM_PLANS + 1))
    assert "THE DEFINITION" in stable and "THE TIE RULE among the candidates that attain the minimum is the project's own" in stable
    c = _lib
    assert _lib._SIGS["dicow_ngram_repeats"] == [c.c_vp, c.c_vp, c.c_i64, c.c_vp, c.c_i, c.c_i, c.c_i, c.c_i, c.c_i, c.c_i, c.c_vp, c.c_vp, c.c_i,
                                                 c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_ngram_repeats_ws_bytes"] == [c.c_vp, c.c_i, c.c_i]
    assert {"dicow_ngram_repeats", "dicow_ngram_repeats_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_ngram_repeats.restype is c.c_i and lib.dicow_ngram_repeats_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("repeating_ngram_cuts", "truncate_repeating_ngrams", "truncate_at_repeating_ngram", "session_hypotheses"):
        assert getattr(pkg, name) is getattr(hyp_cleanup, name) and name in pkg.__all__


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 2))


def _size(lib, rows, plan=0):
    t = _table(rows)
    return lib.dicow_ngram_repeats_ws_bytes(t.ctypes.data if len(t) else None, len(t), plan)


def test_workspace_size_follows_the_stated_formula():
    lib = _lib.lib()
    up16 = lambda v: -(-v // 16) * 16                                     # noqa: E731
    assert lib.dicow_ngram_repeats_ws_bytes(None, 0, 0) == 0
    for rows in ([(0, 0)], [(0, 1)], [(0, 2)], [(0, 65)], [(0, 66)], [(0, 30), (30, 400), (7, 257), (0, 258)], [(0, 1025)], [(0, 65535)] * 3):
        for plan in range(0, _lib.NGRAM_PLANS + 1):
            R_ = _lib.NGRAM_PLAN_TILES[plan or 2][0]                      # the library's choice is plan 2
            items = sum(-(-max(w - 1, 0) // R_) for _, w in rows)
            want = up16(len(rows) * _lib.NGRAM_SEG_BYTES + items * _lib.NGRAM_ITEM_BYTES) + 8 * items
            assert _size(lib, rows, plan) == want, (rows, plan)
    assert _size(lib, [(0, 65)], 1) == up16(24 + 8) + 8 and _size(lib, [(0, 66)], 1) == up16(24 + 16) + 16


def _call(lib, rows, **kw):
    """dicow_ngram_repeats with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    t = _table(rows)
    a = dict(ids=p, fold=2 * p, n_words=1000, n=len(t), min_n=1, max_n=10, min_words=30, u=10, r=10, keep=3 * p, reason=4 * p, plan=0, ws=5 * p,
             wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = max(0, lib.dicow_ngram_repeats_ws_bytes(t.ctypes.data if len(t) else None, len(t), 0))
    return lib.dicow_ngram_repeats(a["ids"], a["fold"], a["n_words"], t.ctypes.data if len(t) else None, a["n"], a["min_n"], a["max_n"], a["min_words"],
                                   a["u"], a["r"], a["keep"], a["reason"], a["plan"], a["ws"], a["wsb"], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    for bad, word in (((None, -1, 0), b"negative n"), ((None, 2, 0), b"null segment table")):
        assert lib.dicow_ngram_repeats_ws_bytes(*bad) == -1 and b"ngram_repeats_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error()
    for bad, word in (([(0, -1)], b"DICOW_NGRAM_MAX_WORDS"), ([(0, 65536)], b"DICOW_NGRAM_MAX_WORDS")):
        assert _size(lib, bad) == -1 and b"ngram_repeats_ws_bytes" in lib.dicow_last_error() and word in lib.dicow_last_error(), bad
    for plan in (-1, _lib.NGRAM_PLANS + 1):
        assert _size(lib, [(0, 5)], plan) == -1 and b"plan" in lib.dicow_last_error()
    # a workspace over the limit needs no device memory to be refused: 65 535 words at 64 rows an item are 16 KB of tables a segment
    big = [(0, 65535)] * 70000
    assert 0 < _size(lib, big[:1000], 1) <= _lib.NGRAM_MAX_WS_BYTES
    assert _size(lib, big, 1) == -1 and b"DICOW_NGRAM_MAX_WS_BYTES" in lib.dicow_last_error() and b"split the call" in lib.dicow_last_error()
    assert _call(lib, big, n_words=65535, plan=1, wsb=1 << 40) == -1 and b"DICOW_NGRAM_MAX_WS_BYTES" in lib.dicow_last_error()
    ok = [(0, 100), (100, 900), (40, 0)]
    need = _size(lib, ok)
    assert need > 0
    for bad, word in ((dict(rows=[(0, 65536)]), b"DICOW_NGRAM_MAX_WORDS"), (dict(rows=[(0, -1)]), b"DICOW_NGRAM_MAX_WORDS"),
                      (dict(rows=[(0, 1001)]), b"outside the 1000 ids"), (dict(rows=[(-1, 5)]), b"outside the 1000 ids"),
                      (dict(rows=[(0, 10), (995, 6)]), b"segment 1 reads words"), (dict(rows=[(1001, 0)]), b"outside the 1000 ids"),
                      (dict(rows=ok, n_words=-1), b"n_words"), (dict(rows=ok, min_n=0), b"min_n"), (dict(rows=ok, min_n=-3), b"min_n"),
                      (dict(rows=ok, max_n=_lib.NGRAM_MAX_N + 1), b"DICOW_NGRAM_MAX_N"), (dict(rows=ok, u=0), b"unigram_min_repeat"),
                      (dict(rows=ok, r=-1), b"repeat_threshold"), (dict(rows=ok, plan=_lib.NGRAM_PLANS + 1), b"plan"), (dict(rows=ok, plan=-1), b"plan"),
                      (dict(rows=ok, ids=None), b"null"), (dict(rows=ok, fold=None), b"null"), (dict(rows=ok, keep=None), b"null"),
                      (dict(rows=ok, ws=None), b"null"), (dict(rows=ok, ids=4098), b"aligned"), (dict(rows=ok, fold=4097), b"aligned"),
                      (dict(rows=ok, keep=4098), b"aligned"), (dict(rows=ok, reason=4099), b"aligned"), (dict(rows=ok, ws=4104), b"aligned"),
                      (dict(rows=ok, wsb=need - 1), b"ws_bytes"), (dict(rows=ok, wsb=0), b"ws_bytes"), (dict(rows=ok, n=-1), b"negative n")):
        rc = _call(lib, **bad)
        assert rc == -1, bad
        assert b"ngram_repeats" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    # an empty table launches nothing and needs nothing
    assert _call(lib, [], ids=None, fold=None, keep=None, reason=None, ws=None, wsb=0) == 0


def test_wrappers_refuse_what_they_cannot_run():
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.DicowError, match="GPU"):
        hyp_cleanup.repeating_ngram_cuts(ids, ids, [(0, 4)])
    with pytest.raises(_lib.DicowError, match="GPU"):
        hyp_cleanup.repeating_ngram_cuts(ids.numpy(), ids.numpy(), [(0, 4)])


class StubTokenizer:
    """decode() joins the pieces of the ids; ids >= 100 are special tokens."""

    def __init__(self, pieces):
        self.pieces = pieces

    def decode(self, ids, skip_special_tokens=False):
        return "".join(self.pieces[i] if i < 100 else ("" if skip_special_tokens else "<|special|>") for i in ids)


def test_session_hypotheses_overflow_shift_and_empty_texts(caplog):
    tok = StubTokenizer([" hello", " world", " ", "again", " thank", " you"])
    segs = [dict(start=0.0, end=2.5, tokens=[100, 0, 1, 101]), dict(start=3.0, end=4.0, tokens=[100, 2, 101]), dict(start=4.0, end=4.5, tokens=[]),
            dict(start=10.0, end=35.0, tokens=[3]), dict(start=20.0, end=35.01, tokens=[0]), dict(start=36.0, end=39.0, tokens=[4, 5] * 40)]
    with caplog.at_level(logging.WARNING, logger=hyp_cleanup.log.name):
        got = hyp_cleanup.session_hypotheses(segs, tok, "spk1", session_id="s7", cut_start=100.0, cut_duration=30.0, truncate=False)
    # empty and white-space-only texts are dropped; end <= cut_duration + 5 stays, anything later goes with a warning; times move by cut_start
    assert got == [dict(session_id="s7", speaker="spk1", start_time=100.0, end_time=102.5, words="hello world"),
                   dict(session_id="s7", speaker="spk1", start_time=110.0, end_time=135.0, words="again")]
    assert len(caplog.records) == 2 and all("out of bounds" in r.getMessage() for r in caplog.records)
    # no cut duration: no overflow rule; truncate=False passes a loop on as it is; text_map sees the stripped text
    got = hyp_cleanup.session_hypotheses(segs, tok, 3, truncate=False, text_map=str.upper)
    assert [g["words"] for g in got] == ["HELLO WORLD", "AGAIN", "HELLO", ("THANK YOU " * 40).strip()]
    assert got[0] == dict(session_id=None, speaker=3, start_time=0.0, end_time=2.5, words="HELLO WORLD") and got[3]["end_time"] == 39.0
    assert hyp_cleanup.session_hypotheses([], tok, "a") == []
    got = hyp_cleanup.session_hypotheses(segs[:1], tok, "a", cut_duration=2.0, overflow_margin=0.5, truncate=False)
    assert [g["words"] for g in got] == ["hello world"] and hyp_cleanup.session_hypotheses(segs[:1], tok, "a", cut_duration=2.0, overflow_margin=0.4,
                                                                                            truncate=False) == []

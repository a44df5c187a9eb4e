"""CPU tests of the sequence_bias / bad_words_ids options' host side: the C-ABI entry point, the validation (transformers' error texts),
the device table's layout, phrase_sequences, the way generate() hands the options on, and the plain-Python oracle of the kernel's
definition (tests/sequence_bias_ref.py) against transformers' SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor.  No GPU needed.

The oracle and transformers are compared AS NUMBERS: transformers adds a whole [rows, V] bias tensor, so a -0.0 score that no sequence
touches comes back as +0.0 from it; the definition (and the kernel) writes only the entries a matching sequence heads, and such a -0.0
keeps its bits.  That is the one stated difference in bits; the other stated deviation is that +inf and NaN biases are refused."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import amd_pkg
from tests import sequence_bias_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, generation  # noqa: E402

INF = float("inf")


def test_sequence_bias_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_sequence_bias\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["float* scores", "int64_t ld", "int rows", "int V", "const int64_t* input_ids", "int64_t ids_stride", "int L",
                    "const int* table", "int n_seq", "int n_groups", "int n_tokens", "int max_len", "int max_group", "int plan",
                    "void* stream"]
    c = _lib
    assert _lib._SIGS["dicow_sequence_bias"] == [c.c_vp, c.c_i64, c.c_i, c.c_i, c.c_vp, c.c_i64, c.c_i, c.c_vp] + [c.c_i] * 6 + [c.c_vp]
    assert "dicow_sequence_bias" in _lib.declared_symbols()
    lib = _lib.lib()
    assert lib.dicow_sequence_bias.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name, val in (("MAX_L", _lib.SEQ_BIAS_MAX_L), ("MAX_LEN", _lib.SEQ_BIAS_MAX_LEN), ("MAX_SEQ", _lib.SEQ_BIAS_MAX_SEQ),
                      ("PLANS", _lib.SEQ_BIAS_PLANS), ("LANE", _lib.SEQ_BIAS_LANE), ("WAVE", _lib.SEQ_BIAS_WAVE)):
        assert re.search(rf"^#define DICOW_SEQ_BIAS_{name} {val}$", stable, flags=re.M), name
    assert "-0.0 stays -0.0" in " ".join(stable.split())                  # the stated difference from transformers, in the header too


def test_exports():
    assert pkg.phrase_sequences is generation.phrase_sequences and "phrase_sequences" in pkg.__all__
    for name in ("sequence_bias_options", "sequence_bias_table", "sequence_bias_rules", "phrase_sequences"):
        assert callable(getattr(generation, name))


def _hf_error(make):
    with pytest.raises(ValueError) as e:
        make()
    return str(e.value)


def test_validation_errors_equal_transformers():
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor
    opts = generation.sequence_bias_options
    for bad in ({}, [], "x", 3, {(1, 2): 1.0, 3: 2.0}, {(1, -2): 1.0}, {(): 1.0}, {(1, 2.0): 1.0}, {(1, 2): 1}, {(1,): "1.0"},
                [[[1, 2], 1]], [[[1, -2], 1.0]], [[(1, 2), 1.0]]):
        want = _hf_error(lambda: SequenceBiasLogitsProcessor(sequence_bias=bad))
        assert _hf_error(lambda: opts(sequence_bias=bad)) == want, bad
    for bad in ([], "x", [[1], 2], [[1, -1]], [[1, 2.0]]):
        want = _hf_error(lambda: NoBadWordsLogitsProcessor(bad, eos_token_id=7))
        assert _hf_error(lambda: opts(bad_words_ids=bad, eos_token_id=7)) == want, bad
    # an empty banned word, which transformers lets through (it can complete nothing), is refused
    assert "non-empty" in _hf_error(lambda: opts(bad_words_ids=[[1], []]))
    # every banned word is an eos: nothing is banned, in transformers too
    sc = torch.randn(2, 9)
    assert torch.equal(NoBadWordsLogitsProcessor([[7]], eos_token_id=[7, 8])(torch.zeros(2, 3, dtype=torch.long), sc), sc)
    assert opts(bad_words_ids=[[7]], eos_token_id=[7, 8]) is None
    # a token outside the vocabulary: transformers raises on its first call
    proc = SequenceBiasLogitsProcessor(sequence_bias={(3, 50): 1.0, (60,): -1.0})
    want = _hf_error(lambda: proc(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 50)))
    assert _hf_error(lambda: opts(sequence_bias={(3, 50): 1.0, (60,): -1.0}, vocab_size=50)) == want
    assert "[50, 60]" in want
    # the project's own refusals: +inf and NaN (transformers would return NaN scores from -inf + inf)
    for b in (INF, float("nan")):
        assert "finite or -inf" in _hf_error(lambda: opts(sequence_bias={(1, 2): b}))
    with pytest.raises(ValueError):
        opts(sequence_bias={tuple(range(1, _lib.SEQ_BIAS_MAX_LEN + 2)): 1.0})
    with pytest.raises(ValueError):
        generation.sequence_bias_table([(1, 2)], [3.5e38], "cpu")         # +inf once rounded to fp32


def test_options_results():
    opts = generation.sequence_bias_options
    assert opts() is None and opts(None, None, eos_token_id=5, vocab_size=9) is None
    assert opts(sequence_bias={(3, 4): 2.0, (5,): -INF}) == (([(3, 4), (5,)], [2.0, -INF]), None)
    # the list form is converted as transformers converts it: a repeated sequence keeps its first place and takes the later bias
    assert opts(sequence_bias=[[[3, 4], 2.0], [[5], 1.0], [[3, 4], -1.0]])[0] == ([(3, 4), (5,)], [-1.0, 1.0])
    # single-token bad words equal to an eos id are dropped; longer ones that contain it stay
    assert opts(bad_words_ids=[[7], [7, 8], [9], [8]], eos_token_id=[7, 8])[1] == ([(7, 8), (9,)], [-INF, -INF])
    assert opts(bad_words_ids=[[7], [9]], eos_token_id=torch.tensor(7))[1] == ([(9,)], [-INF])
    assert opts(bad_words_ids=[[7], [9]])[1] == ([(7,), (9,)], [-INF, -INF])
    both = opts({(1, 2): 0.5}, [[3]], 0, 10)
    assert both == (([(1, 2)], [0.5]), ([(3,)], [-INF]))


def test_table_layout_of_a_hand_made_case():
    seqs = [(7, 9), (4,), (1, 2, 9), (9,), (3, 4), (8, 8, 8, 4), (0,)]
    bias = [1.5, -2.0, -INF, 0.25, 3.0, -0.0, 8.0]
    t = generation.sequence_bias_table(seqs, bias, "cpu")
    assert (t.n_seq, t.n_groups, t.n_tokens, t.max_len, t.max_group, t.max_token) == (7, 3, 14, 4, 3, 9)
    buf = t.buf
    assert buf.dtype == torch.int32 and buf.numel() == 8 + 4 + 7 + 14
    seq_off, grp_off = buf[:8].tolist(), buf[8:12].tolist()
    b = buf[12:19].clone().view(torch.float32)
    tok = buf[19:].tolist()
    # sorted by last token (0, 4, 9), the single-token sequence first in its group, the others in the caller's order
    order = [(0,), (4,), (3, 4), (8, 8, 8, 4), (9,), (7, 9), (1, 2, 9)]
    assert [tuple(tok[seq_off[i]:seq_off[i + 1]]) for i in range(7)] == order
    assert grp_off == [0, 1, 4, 7]
    want = torch.tensor([bias[seqs.index(s)] for s in order])
    assert torch.equal(b.view(torch.int32), want.view(torch.int32))       # (-0.0 and -inf keep their bits)
    assert groups_as_table(seqs) == order
    empty = generation.sequence_bias_table([], [], "cpu")
    assert (empty.n_seq, empty.n_groups, empty.n_tokens) == (0, 0, 0)
    for bad in (([(1, 2), (1, 2)], [1.0, 2.0]), ([()], [1.0]), ([(1, -1)], [1.0]), ([(1,)], [1.0, 2.0]), ([(1,)], [INF])):
        with pytest.raises(ValueError):
            generation.sequence_bias_table(*bad, "cpu")


def groups_as_table(seqs):
    """The oracle's own grouping, flattened in ascending last-token order: the same order as the table's."""
    g = R.groups_of(seqs)
    return [seqs[i] for v in sorted(g) for i in g[v]]


class ToyTokenizer:
    """Words to ids; a leading space is its own kind of token, as in a BPE vocabulary."""
    vocab = {"hello": 3, " hello": 4, "world": 5, " world": 6, " ": 7}

    def encode(self, text, add_special_tokens=True):
        assert add_special_tokens is False
        out = []
        for i, w in enumerate(text.split(" ")):
            if w:
                out.append(self.vocab[(" " if i else "") + w])
            elif i == 0 and len(text) > 1:
                continue                                                  # the leading space belongs to the next word
            elif text == " ":
                out.append(self.vocab[" "])
        return out


def test_phrase_sequences_on_a_toy_tokenizer():
    tok = ToyTokenizer()
    assert generation.phrase_sequences(tok, ["hello world", "world"]) == [(4, 6), (3, 6), (6,), (5,)]
    assert generation.phrase_sequences(tok, "hello", variants=("plain",)) == [(3,)]
    assert generation.phrase_sequences(tok, ["hello", "hello"], variants=("space",)) == [(4,)]
    assert generation.phrase_sequences(tok, [""], variants=("plain",)) == []          # an empty encoding is left out
    with pytest.raises(ValueError):
        generation.phrase_sequences(tok, ["hello"], variants=("upper",))
    seqs = generation.phrase_sequences(tok, ["hello world"])
    assert generation.sequence_bias_options(sequence_bias={s: 2.0 for s in seqs}, bad_words_ids=[list(s) for s in seqs]) is not None


def random_case(seed, rows, V, L, n_seq, max_m=4):
    """Histories over a small alphabet, sequences drawn partly from the histories' own tails (so that many match), biases of both signs
    with -inf, scores with signed zeros and -inf."""
    g = torch.Generator().manual_seed(seed)
    A = min(V, 5)
    ids = torch.randint(0, A, (rows, L), generator=g)
    seqs = {}
    for k in range(n_seq):
        m = int(torch.randint(1, max_m + 1, (1,), generator=g))
        r = int(torch.randint(0, rows, (1,), generator=g))
        if k % 2 == 0 and m - 1 <= L:                                     # a row's tail, continued by a random token
            s = tuple(ids[r, L - (m - 1):].tolist() if m > 1 else []) + (int(torch.randint(0, V, (1,), generator=g)),)
        else:
            s = tuple(torch.randint(0, A, (m - 1,), generator=g).tolist()) + (int(torch.randint(0, V, (1,), generator=g)),)
        b = float(torch.randn((), generator=g)) * 4.0
        seqs.setdefault(s, -INF if k % 7 == 3 else float(np.float32(b)))
    sc = torch.randn(rows, V, generator=g) * 3.0
    sc[:, 0], sc[:, V - 1], sc[:, V // 2] = -0.0, -INF, 0.0
    return ids, sc, seqs


@pytest.mark.parametrize("seed", range(12))
def test_oracle_equals_transformers_processors(seed):
    rows, V, L, n = [(1, 9, 1, 5), (3, 50, 2, 30), (4, 50, 3, 60), (2, 17, 7, 90)][seed % 4]
    ids, sc, seqs = random_case(seed, rows, V, L, n)
    got, touched = R.reference(ids, sc, list(seqs), list(seqs.values()))
    want = R.via_transformers(ids, sc, sequence_bias=seqs)
    assert touched.any() and R.same_numbers(got, want)
    assert torch.equal(R.bits(got)[~touched], R.bits(sc)[~touched])
    # the stated difference: an untouched -0.0 stays -0.0 here and becomes +0.0 in transformers
    untouched_negzero = ~touched & (R.bits(sc) == R.bits(torch.tensor(-0.0)))
    if untouched_negzero.any():
        assert bool((R.bits(want)[untouched_negzero] == 0).all()) and bool((R.bits(got)[untouched_negzero] != 0).all())
    # the same sequences as banned words (eos filtered out by both)
    words = [list(s) for s in seqs]
    eos = words[0][-1]
    o = generation.sequence_bias_options(bad_words_ids=words, eos_token_id=eos, vocab_size=V)[1]
    got, _ = R.reference(ids, sc, *o)
    assert R.same_numbers(got, R.via_transformers(ids, sc, bad_words_ids=words, eos_token_id=eos))


def test_oracle_order_case_follows_transformers():
    """1e8, -1e8 and 1.0 on three matching sequences of one last token: fp32 gives 1.0 or 0.0 depending on the order."""
    ids = torch.tensor([[0, 1, 2, 3]])
    sc = torch.zeros(1, 10)
    for seqs, want in (({(3, 5): 1e8, (2, 3, 5): -1e8, (1, 2, 3, 5): 1.0}, 1.0),
                       ({(1, 2, 3, 5): 1.0, (3, 5): 1e8, (2, 3, 5): -1e8}, 0.0),
                       ({(3, 5): 1e8, (2, 3, 5): -1e8, (5,): 1.0}, 0.0),            # the single-token entry is added FIRST
                       ({(5,): 1e8, (3, 5): -1e8, (2, 3, 5): 1.0}, 1.0)):
        got, _ = R.reference(ids, sc, list(seqs), list(seqs.values()))
        assert float(got[0, 5]) == want
        assert float(R.via_transformers(ids, sc, sequence_bias=seqs)[0, 5]) == want


def test_wrapper_refuses_cpu_tensors():
    t = generation.sequence_bias_table([(1, 2)], [1.0], "cpu")
    sc = torch.zeros(2, 8)
    with pytest.raises(_lib.DicowError):
        generation.sequence_bias_rules(torch.zeros(2, 3, dtype=torch.long), sc, t)
    assert torch.equal(sc, torch.zeros(2, 8))


class _Recorder:
    """Stands in for GreedyDecoder: records the keyword arguments of the call it receives."""
    def __init__(self):
        self.calls = []

    def generate(self, feats, stno, prompt, n_new, **kw):
        self.calls.append(("generate", kw))
        return torch.cat([prompt, torch.full((feats.shape[0], 2), 7)], 1)

    def beam_search(self, feats, stno, prompt, max_length, num_beams, **kw):
        self.calls.append(("beam_search", kw))
        return torch.cat([prompt, torch.full((feats.shape[0], 2), 7)], 1), None

    def generate_with_fallback(self, feats, stno, prompt, n_new, **kw):
        self.calls.append(("generate_with_fallback", kw))
        return [[7, 8]] * feats.shape[0], [False] * feats.shape[0], [0] * feats.shape[0]


def _model():
    cfg = pkg.DiCoWConfig(vocab_size=512, num_mel_bins=80, d_model=64, encoder_layers=1, encoder_attention_heads=1, decoder_layers=1,
                          decoder_attention_heads=1, encoder_ffn_dim=64, decoder_ffn_dim=64, max_source_positions=50,
                          max_target_positions=32, pad_token_id=500, bos_token_id=500, eos_token_id=500, decoder_start_token_id=501)
    model = pkg.DiCoWForConditionalGeneration(cfg)
    model.tokenizer = None
    return model, cfg


def _picked(kw):
    return kw.get("sequence_bias"), kw.get("bad_words_ids")


def test_generate_hands_the_options_to_every_path_and_keywords_win(monkeypatch):
    model, cfg = _model()
    W = 2 * cfg.max_source_positions
    x, st = torch.zeros(2, 80, W), torch.zeros(2, 4, W // 2)
    prompt = torch.tensor([[501, 3]] * 2)
    rec = _Recorder()
    model._decoder = rec
    sb, bw = {(3, 4): 2.0}, [[9], [5, 6]]
    gc = SimpleNamespace(eos_token_id=500, pad_token_id=500, sequence_bias=sb, bad_words_ids=bw)
    call = lambda **kw: model.generate(input_features=x, stno_mask=st, decoder_input_ids=prompt, max_new_tokens=4, **kw)  # noqa: E731
    call(generation_config=gc)
    call(generation_config=gc, num_beams=3)
    call(generation_config=gc, sequence_bias={(1,): -1.0}, bad_words_ids=[[2]])
    call(generation_config=SimpleNamespace(eos_token_id=500, pad_token_id=500, sequence_bias=None, bad_words_ids=None))
    call(generation_config=SimpleNamespace(eos_token_id=500, pad_token_id=500))
    assert [(n, _picked(kw)) for n, kw in rec.calls] == [
        ("generate", (sb, bw)), ("beam_search", (sb, bw)), ("generate", ({(1,): -1.0}, [[2]])), ("generate", (None, None)),
        ("generate", (None, None))]
    # a bad value raises before anything is decoded
    n = len(rec.calls)
    for bad in (dict(sequence_bias={(3, 4): 2}), dict(bad_words_ids=[3]), dict(sequence_bias={(3, 512): 1.0}), dict(sequence_bias={(3,): INF})):
        with pytest.raises(ValueError):
            call(generation_config=gc, **bad)
    assert len(rec.calls) == n
    # the long form: greedy, beam search and the fallback ladder
    x2, st2 = torch.zeros(1, 80, W + 20), torch.zeros(1, 4, (W + 20) // 2)
    no_ts = 399

    class Tok:
        prefix_tokens = [501, 3]
        pad_token_id = 499

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 7}

    model.tokenizer = Tok()
    rec2 = _Recorder()
    monkeypatch.setattr(generation, "GreedyDecoder", lambda model, use_graphs=False: rec2)
    gc2 = SimpleNamespace(eos_token_id=500, pad_token_id=500, no_timestamps_token_id=no_ts, sequence_bias=sb, bad_words_ids=bw)
    kw = dict(input_features=x2, stno_mask=st2, attention_mask=torch.ones(1, W + 20, dtype=torch.long), generation_config=gc2,
              max_new_tokens=4)
    model.generate(**kw)
    model.generate(num_beams=2, **kw)
    model.generate(temperature=(0.0, 0.5), logprob_threshold=-1.0, **kw)
    assert {n for n, _ in rec2.calls} == {"generate", "beam_search", "generate_with_fallback"}
    assert len(rec2.calls) == 6 and all(_picked(k) == (sb, bw) for _, k in rec2.calls)

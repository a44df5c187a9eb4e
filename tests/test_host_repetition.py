"""CPU tests of the repetition penalty / no-repeat n-gram options' host side: the C-ABI entry point, the wrapper's validation and
the way DiCoWForConditionalGeneration.generate hands generation_config.repetition_penalty / .no_repeat_ngram_size to its four
decoding paths.  No GPU needed."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import amd_pkg
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, generation  # noqa: E402


def test_repetition_rules_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_repetition_rules\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["float* scores", "int64_t ld", "int rows", "int V", "const int64_t* input_ids", "int64_t ids_stride", "int L",
                    "float penalty", "int ngram", "void* stream"]
    c = _lib
    assert _lib._SIGS["dicow_repetition_rules"] == [c.c_vp, c.c_i64, c.c_i, c.c_i, c.c_vp, c.c_i64, c.c_i, c.c_f, c.c_i, c.c_vp]
    assert "dicow_repetition_rules" in _lib.declared_symbols()
    lib = _lib.lib()
    assert lib.dicow_repetition_rules.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays


def test_validation_follows_transformers_processors():
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    opts = generation.repetition_options
    for bad in (0.0, -1.3, 2, "1.2", float("nan")):
        with pytest.raises(ValueError):
            RepetitionPenaltyLogitsProcessor(penalty=bad)
        with pytest.raises(ValueError):
            opts(repetition_penalty=bad)
        with pytest.raises(ValueError):
            generation.repetition_rules(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 4), repetition_penalty=bad)
    for bad in (-1, 2.0, "3", True):
        if bad is not True:                                              # (HF takes True for an int; a flag is not an n-gram size here)
            with pytest.raises(ValueError):
                NoRepeatNGramLogitsProcessor(bad)
        with pytest.raises(ValueError):
            opts(no_repeat_ngram_size=bad)
        with pytest.raises(ValueError):
            generation.repetition_rules(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 4), no_repeat_ngram_size=bad)
    # off: None, penalty 1.0 (the GenerationConfig default; an integer 1 from a YAML file too) and n-gram size 0
    for off in (dict(), dict(repetition_penalty=None, no_repeat_ngram_size=None), dict(repetition_penalty=1.0, no_repeat_ngram_size=0),
                dict(repetition_penalty=1), dict(no_repeat_ngram_size=0)):
        assert opts(**off) is None
    assert opts(repetition_penalty=1.3) == (1.3, 0)
    assert opts(no_repeat_ngram_size=2) == (1.0, 2)
    assert opts(0.7, 5) == (0.7, 5)


def test_wrapper_refuses_cpu_tensors():
    ids, sc = torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 8)
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict()):
        with pytest.raises(_lib.DicowError):
            generation.repetition_rules(ids, sc, **kw)
    assert torch.equal(sc, torch.zeros(2, 8))


class _Recorder:
    """Stands in for GreedyDecoder: records the keyword arguments of the call it receives."""
    def __init__(self):
        self.calls = []

    def generate(self, feats, stno, prompt, n_new, **kw):
        self.calls.append(("generate", kw))
        return prompt

    def beam_search(self, feats, stno, prompt, max_length, num_beams, **kw):
        self.calls.append(("beam_search", kw))
        return prompt, None

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
    return kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size")


def test_generate_reads_the_options_from_the_generation_config_and_keywords_win():
    model, cfg = _model()
    W = 2 * cfg.max_source_positions
    x, st = torch.zeros(2, 80, W), torch.zeros(2, 4, W // 2)
    prompt = torch.tensor([[501, 3]] * 2)
    rec = _Recorder()
    model._decoder = rec
    gc = SimpleNamespace(eos_token_id=500, pad_token_id=500, repetition_penalty=1.2, no_repeat_ngram_size=3)
    call = lambda **kw: model.generate(input_features=x, stno_mask=st, decoder_input_ids=prompt, max_new_tokens=4, **kw)  # noqa: E731
    # single-pass greedy and beam: from the config; an explicit keyword wins; an attribute held as None is not set
    call(generation_config=gc)
    call(generation_config=gc, num_beams=3)
    call(generation_config=gc, repetition_penalty=1.5, no_repeat_ngram_size=2)
    call(generation_config=gc, repetition_penalty=1.0, no_repeat_ngram_size=0, num_beams=2)
    call(generation_config=SimpleNamespace(eos_token_id=500, pad_token_id=500, repetition_penalty=None, no_repeat_ngram_size=None))
    call(generation_config=SimpleNamespace(eos_token_id=500, pad_token_id=500))
    assert [(n, _picked(kw)) for n, kw in rec.calls] == [
        ("generate", (1.2, 3)), ("beam_search", (1.2, 3)), ("generate", (1.5, 2)), ("beam_search", (1.0, 0)),
        ("generate", (None, None)), ("generate", (None, None))]
    # values no processor of HF's would accept raise before anything is decoded
    n = len(rec.calls)
    with pytest.raises(ValueError):
        call(generation_config=gc, repetition_penalty=-1.0)
    with pytest.raises(ValueError):
        call(generation_config=SimpleNamespace(eos_token_id=500, pad_token_id=500, no_repeat_ngram_size=2.5))
    assert len(rec.calls) == n


def test_long_form_and_fallback_paths_receive_the_options(monkeypatch):
    """generate() -> LongFormDecoder.transcribe -> GreedyDecoder.generate / .beam_search / .generate_with_fallback."""
    model, cfg = _model()
    W = 2 * cfg.max_source_positions
    x, st = torch.zeros(1, 80, W + 20), torch.zeros(1, 4, (W + 20) // 2)
    att = torch.ones(1, W + 20, dtype=torch.long)
    no_ts = 399

    class Tok:
        prefix_tokens = [501, 3]
        pad_token_id = 499

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 7}

    model.tokenizer = Tok()
    rec = _Recorder()
    rec.generate = lambda feats, stno, prompt, n_new, **kw: (rec.calls.append(("generate", kw)),
                                                            torch.cat([prompt, torch.full((feats.shape[0], 2), 7)], 1))[1]
    rec.beam_search = lambda feats, stno, prompt, max_length, num_beams, **kw: (
        rec.calls.append(("beam_search", kw)), (torch.cat([prompt, torch.full((feats.shape[0], 2), 7)], 1), None))[1]
    monkeypatch.setattr(generation, "GreedyDecoder", lambda model, use_graphs=False: rec)
    gc = SimpleNamespace(eos_token_id=500, pad_token_id=500, no_timestamps_token_id=no_ts, repetition_penalty=1.2, no_repeat_ngram_size=3)
    kw = dict(input_features=x, stno_mask=st, attention_mask=att, generation_config=gc, max_new_tokens=4)
    model.generate(**kw)
    model.generate(num_beams=2, **kw)
    model.generate(temperature=(0.0, 0.5), logprob_threshold=-1.0, **kw)
    model.generate(no_repeat_ngram_size=5, **kw)
    names = [n for n, _ in rec.calls]
    assert set(names) == {"generate", "beam_search", "generate_with_fallback"}
    assert len(rec.calls) == 8 and all(_picked(k) == (1.2, 3) for _, k in rec.calls[:-2])      # (two windows per call)
    assert [_picked(k) for _, k in rec.calls[-2:]] == [(1.2, 5), (1.2, 5)]

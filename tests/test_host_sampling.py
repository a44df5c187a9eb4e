"""CPU tests of the device sampler's host side: the numpy oracle of dicow_sample_tokens (tests/sampling_ref.py) against transformers'
own warpers and golden F28, the C-ABI entry point, the validation of the options, the temperature ladder on token log-probabilities,
and the statistics of the oracle's Philox / Gumbel-max draw.  No GPU needed.

The oracle and transformers are compared on inputs of DISTINCT values: the library keeps or removes a tie class of top_p as a whole,
HF's sort splits it arbitrarily -- the one stated difference.  Equality of the kept masks is required except where a token's
cumulative mass lies within 2e-5 of 1 - top_p or its ratio within 1e-6 (relative) of min_p: transformers sums fp32 probabilities."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import amd_pkg
from tests import sampling_ref as R
from tests.util import ROOT, load_golden

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, generation  # noqa: E402

INF = float("inf")


def test_sample_tokens_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    assert re.search(r"^int\s+dicow_sample_tokens\s*\(const dicow_sample_args\* a, void\* stream\);", stable, flags=re.M)
    m = re.search(r"typedef struct \{([^}]*)\} dicow_sample_args;", stable)
    assert m is not None
    fields = [f.strip() for f in " ".join(m.group(1).split()).split(";") if f.strip()]
    assert fields == ["const float* scores", "int64_t ld", "int rows", "int V", "float temperature", "int top_k", "float top_p",
                      "float min_p", "uint64_t seed", "uint32_t step", "uint32_t stream", "const int64_t* row_ids", "uint8_t* unfinished",
                      "int eos", "int pad", "int64_t* next", "int64_t next_stride", "float* logprob", "float* warped", "int64_t ld_w",
                      "int plan"]
    import ctypes as C
    c = _lib
    want = dict(scores=c.c_vp, ld=c.c_i64, rows=c.c_i, V=c.c_i, temperature=c.c_f, top_k=c.c_i, top_p=c.c_f, min_p=c.c_f, seed=c.c_u64,
                step=C.c_uint32, stream=C.c_uint32, row_ids=c.c_vp, unfinished=c.c_vp, eos=c.c_i, pad=c.c_i, next=c.c_vp,
                next_stride=c.c_i64, logprob=c.c_vp, warped=c.c_vp, ld_w=c.c_i64, plan=c.c_i)
    assert [(n, t) for n, t in _lib.SampleArgs._fields_] == [(f.split()[-1].lstrip("*"), want[f.split()[-1].lstrip("*")]) for f in fields]
    assert _lib._SIGS["dicow_sample_tokens"] == [C.POINTER(_lib.SampleArgs), c.c_vp]
    assert "dicow_sample_tokens" in _lib.declared_symbols()
    lib = _lib.lib()
    assert lib.dicow_sample_tokens.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name, val in (("REG_MAX_V", _lib.SAMPLE_REG_MAX_V), ("PLANS", _lib.SAMPLE_PLANS), ("REG", _lib.SAMPLE_REG),
                      ("STREAM", _lib.SAMPLE_STREAM)):
        assert re.search(rf"^#define DICOW_SAMPLE_{name} {val}$", stable, flags=re.M), name
    assert "A tie class is kept or removed as a whole" in " ".join(stable.split())


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """No GPU here: a refusal must come before the launch, and name the limit."""
    import ctypes as C
    lib = _lib.lib()

    def err(**kw):
        a = _lib.SampleArgs(**{**dict(rows=1, V=8, ld=8), **kw})
        assert lib.dicow_sample_tokens(C.byref(a), None) == -1
        return lib.dicow_last_error().decode()

    assert "plan 3 is not 0 .. 2" in err(plan=3)
    assert "DICOW_SAMPLE_REG_MAX_V (65536)" in err(V=65537, ld=70000, plan=_lib.SAMPLE_REG)
    assert "rows=-1" in err(rows=-1)
    assert "ld=7" in err(ld=7)
    assert "NaN" in err(temperature=float("nan"))
    a = _lib.SampleArgs(rows=0, V=8, ld=8)
    assert lib.dicow_sample_tokens(C.byref(a), None) == 0               # nothing to do, nothing launched


def test_sampling_options():
    so = generation.sampling_options
    assert so() is None and so(generator=torch.Generator()) is None
    o = so(top_k=50)
    assert (o.top_k, o.top_p, o.min_p, o.seed) == (50, 1.0, 0.0, 0)
    o = so(top_p=0.9, min_p=0.05, seed=2 ** 64 - 1)
    assert (o.top_k, o.top_p, o.min_p, o.seed) == (0, 0.9, 0.05, 2 ** 64 - 1)
    assert so(top_k=0).top_k == 0 and so(top_p=1).top_p == 1.0 and so(min_p=0).min_p == 0.0 and so(min_p=1.0).min_p == 1.0
    for bad in (dict(top_k=-1), dict(top_k=2.0), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.5), dict(top_p="0.9"), dict(top_p=float("nan")),
                dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0),
                dict(seed=3, generator=torch.Generator())):
        with pytest.raises(ValueError):
            so(**bad)
    assert pkg.sample_tokens is generation.sample_tokens and "sample_tokens" in pkg.__all__
    with pytest.raises(_lib.DicowError):                                  # no CPU fallback
        generation.sample_tokens(torch.zeros(2, 8))


class _Recorder:
    def __init__(self):
        self.calls = []

    def generate(self, feats, stno, prompt, n_new, **kw):
        self.calls.append(("generate", kw))
        return torch.cat([prompt, torch.full((feats.shape[0], 2), 7)], 1)

    def generate_with_fallback(self, feats, stno, prompt, n_new, **kw):
        self.calls.append(("generate_with_fallback", kw))
        return [[7, 8]] * feats.shape[0], [False] * feats.shape[0], [0] * feats.shape[0]


def test_model_generate_validates_first_and_forwards_on_the_ladder_only(monkeypatch):
    cfg = pkg.DiCoWConfig(vocab_size=512, num_mel_bins=80, d_model=64, encoder_layers=1, encoder_attention_heads=1, decoder_layers=1,
                          decoder_attention_heads=1, encoder_ffn_dim=64, decoder_ffn_dim=64, max_source_positions=50,
                          max_target_positions=32, pad_token_id=500, bos_token_id=500, eos_token_id=500, decoder_start_token_id=501)
    model = pkg.DiCoWForConditionalGeneration(cfg)
    W = 2 * cfg.max_source_positions
    no_ts = 399

    class Tok:
        prefix_tokens = [501, 3]
        pad_token_id = 499

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 7}

    model.tokenizer = Tok()
    rec = _Recorder()
    monkeypatch.setattr(generation, "GreedyDecoder", lambda model, use_graphs=False: rec)
    x, st = torch.zeros(1, 80, W + 20), torch.zeros(1, 4, (W + 20) // 2)
    gc = SimpleNamespace(eos_token_id=500, pad_token_id=500, no_timestamps_token_id=no_ts, top_k=50, top_p=None)
    kw = dict(input_features=x, stno_mask=st, attention_mask=torch.ones(1, W + 20, dtype=torch.long), generation_config=gc, max_new_tokens=4)
    for bad in (dict(top_k=-3), dict(top_p=0.0), dict(min_p=2.0), dict(seed=-1), dict(seed=1, generator=torch.Generator())):
        with pytest.raises(ValueError):
            model.generate(temperature=(0.0, 0.5), logprob_threshold=-1.0, **bad, **kw)
    assert rec.calls == []                                                # refused before any window is decoded
    model.generate(temperature=(0.0, 0.5), logprob_threshold=-1.0, top_p=0.9, seed=11, **kw)
    model.generate(temperature=(0.0, 0.5), logprob_threshold=-1.0, top_k=7, **kw)                 # the keyword wins over the config
    model.generate(**kw)                                                  # greedy long form: the sampling options are not consulted
    pick = lambda k: tuple(k.get(n) for n in ("top_k", "top_p", "min_p", "seed", "row_ids", "stream"))  # noqa: E731
    assert [(n, pick(k)) for n, k in rec.calls] == [
        ("generate_with_fallback", (50, 0.9, None, 11, [0], 0)), ("generate_with_fallback", (50, 0.9, None, 11, [0], 16)),
        ("generate_with_fallback", (7, None, None, None, [0], 0)), ("generate_with_fallback", (7, None, None, None, [0], 16)),
        ("generate", (None,) * 6), ("generate", (None,) * 6)]
    with pytest.raises(NotImplementedError):                             # a scalar temperature > 0 still raises
        model.generate(temperature=0.7, top_k=5, **kw)
    with pytest.raises(ValueError, match="at most 16 rungs"):
        model.generate(temperature=tuple(0.05 * i for i in range(17)), logprob_threshold=-1.0, seed=1, **kw)


# ------------------------------------------------------------------------------------------------ the oracle against transformers
def _distinct_scores(rows, V, seed, scale=12.0):
    g = torch.Generator().manual_seed(seed)
    out = np.empty((rows, V), np.float32)
    for r in range(rows):
        out[r] = ((torch.randperm(4 * V, generator=g)[:V].double() - 2 * V) * (scale / (2 * V))).float().numpy()
        out[r, (5 * r + 1) % V] = -np.inf
    return out


def _assert_equals_hf(x, t, k, p, mp, hf, what):
    o = R.warp(x, t, k, p, mp)
    hf_kept = hf > -np.inf
    off = (o.kept != hf_kept) & ~o.band
    assert not off.any(), f"{what}: kept masks differ outside the band at {np.argwhere(off)[:4].tolist()}"
    both = o.kept & hf_kept
    assert np.array_equal(o.warped[both].view(np.int32), hf[both].view(np.int32)), f"{what}: a kept score is not scores / t bit for bit"
    assert o.band.mean(axis=1).max() <= 0.002, f"{what}: the band is no narrow exception"
    return o


OPTS = [(1.0, 0, 1.0, 0.0), (0.7, 5, 1.0, 0.0), (1.3, 50, 1.0, 0.0), (0.2, 0, 0.9, 0.0), (1.0, 0, 0.5, 0.0), (0.7, 0, 0.99, 0.0),
        (1.0, 0, 1e-6, 0.0), (0.7, 0, 1.0, 0.01), (1.3, 0, 1.0, 0.3), (1.0, 50, 0.9, 0.0), (0.7, 50, 0.5, 0.01), (1.3, 20, 0.99, 0.3),
        (1.0, 1, 1.0, 0.0), (0.7, 2000, 0.9, 0.0)]


@pytest.mark.parametrize("V,rows", [(50, 6), (1000, 8), (5000, 3)])
def test_oracle_equals_transformers_warpers(V, rows):
    x = _distinct_scores(rows, V, 31 + V)
    for t, k, p, mp in OPTS:
        o = _assert_equals_hf(x, t, k, p, mp, R.via_transformers(x, t, k, p, mp), f"V={V} opts={(t, k, p, mp)}")
        assert o.kept.sum(axis=1).min() >= 1
        if p <= 1e-6 or k == 1:
            assert (o.kept.sum(axis=1) == 1).all()                        # only the maximum


def test_oracle_rules_on_hand_made_rows():
    x = np.array([[1.0, 3.0, 3.0, 2.0, -INF, 0.0, -0.0, 2.0]], np.float32)
    assert R.warp(x, 1.0, top_k=1).kept[0].tolist() == [False, True, True, False, False, False, False, False]      # the tie stays
    assert R.warp(x, 1.0, top_k=3).kept[0].tolist() == [False, True, True, True, False, False, False, True]
    assert R.warp(x, 1.0, top_k=8).kept[0].tolist() == [True, True, True, True, False, True, True, True]           # -inf is never kept
    two = np.array([[-INF, 5.0, -INF, 4.0]], np.float32)
    assert R.warp(two, 0.7, top_k=3).kept[0].tolist() == [False, True, False, True]                                   # fewer than k finite
    o = R.warp(x, 1.0, top_p=0.5)                                          # masses: the two 3.0 hold 0.72: everything below goes
    assert o.kept[0].tolist() == [False, True, True, False, False, False, False, False]
    assert R.warp(x, 0.0, top_k=1, top_p=0.1, min_p=0.9).kept[0].tolist() == [True, True, True, True, False, True, True, True]   # argmax rung
    s = R.sample(x, 0.0, unfinished=[1], eos=1)
    assert s.tokens.tolist() == [1] and s.unfinished.tolist() == [False]
    s = R.sample(np.full((2, 4), -INF, np.float32), 0.7, eos=9, unfinished=[1, 0], pad=3)
    assert s.tokens.tolist() == [9, 3] and np.isnan(s.logprob[0]) and s.logprob[1] == 0.0 and s.unfinished.tolist() == [False, False]
    zeros = np.array([[-0.0, 0.0, -1.0]], np.float32)
    assert R.sample(zeros, 0.0).tokens.tolist() == [0]                    # -0.0 == +0.0: the lowest index


def test_golden_f28_pins_transformers_outputs():
    z = load_golden("f28_sampling_warpers")
    n = 0
    for V in (50, 1000):
        x = z[f"V{V}.scores"]
        assert x.shape[0] <= 8
        i = 0
        while f"V{V}.case{i}.opts" in z.files:
            t, k, p, mp = z[f"V{V}.case{i}.opts"].tolist()
            hf = z[f"V{V}.case{i}.warped"]
            _assert_equals_hf(x, t, int(k), p, mp, hf, f"F28 V={V} case {i}")
            got = R.via_transformers(x, t, int(k), p, mp)                 # the installed transformers still computes what was pinned
            assert np.array_equal(got.view(np.int32), hf.view(np.int32)), (V, i)
            i, n = i + 1, n + 1
    assert n == 24


# ------------------------------------------------------------------------------------------------ the ladder on token log-probabilities
def _as_logprob_vectors(decode):
    """decode(rows, temp) with [n, V] score tensors -> the same with each window's vector of token log-probabilities."""
    def wrapped(rows, temp):
        toks, scores, nsp = decode(rows, temp)
        out = []
        for tk, sc in zip(toks, scores):
            n = min(sc.shape[0], len(tk))
            lp = torch.log_softmax((sc[:n] * temp if temp > 0 else sc[:n]).float(), dim=-1)
            out.append(lp.gather(1, torch.as_tensor(tk[:n])[:, None])[:, 0])
        return toks, out, nsp
    return wrapped


def test_ladder_decisions_on_logprob_vectors_equal_those_on_scores():
    from tests.test_oracle_vs_golden import _check_fallback
    from ts_asr_whisper_amd.generation import decode_with_fallback, sequence_avg_logprob, token_compression_ratio
    _check_fallback(lambda decode, *a: decode_with_fallback(_as_logprob_vectors(decode), *a), token_compression_ratio, sequence_avg_logprob)
    # the scripted three-window case of tests/test_host_logic.py (the skip flag's slot), both forms
    V, eos, pad = 16, 15, 14

    def scores_for(tokens, good):
        sc = torch.full((len(tokens), V), -8.0)
        for i, t in enumerate(tokens):
            sc[i, t] = 8.0 if good else -7.9
        return sc
    good = {(0, 0): False, (1, 0): True, (2, 0): False, (0, 1): True, (2, 1): False}

    def decode(rows, temp):
        k = 0 if temp == 0.0 else 1
        toks = [[3 + r, 5, 7, eos] for r in rows]
        return toks, [scores_for(t, good[(r, k)]) for r, t in zip(rows, toks)], [0.99 if (r == 2 and k == 1) else 0.1 for r in rows]
    kw = dict(compression_ratio_threshold=None, logprob_threshold=-1.0, no_speech_threshold=0.6)
    for by_row in (False, True):
        a = decode_with_fallback(decode, 3, (0.0, 0.2), V, pad, eos, skip_by_row=by_row, **kw)
        b = decode_with_fallback(_as_logprob_vectors(decode), 3, (0.0, 0.2), V, pad, eos, skip_by_row=by_row, **kw)
        assert a == b and a[2] == [1, 0, 1]


def test_sequence_avg_logprob_from_tokens_agrees_with_the_score_form():
    from ts_asr_whisper_amd.generation import sequence_avg_logprob, sequence_avg_logprob_from_tokens
    g = torch.Generator().manual_seed(5)
    for temp in (0.0, 0.4, 1.0):
        for n, n_tok in ((7, 7), (9, 6)):                               # (more scored positions than tokens: the padding tail)
            x = torch.randn(n, 40, generator=g) * 3
            o = R.sample(x.numpy(), temp, top_k=5, seed=9, step=1)
            toks = o.tokens.tolist()[:n_tok]
            a = sequence_avg_logprob(torch.from_numpy(o.warped), toks, temp)
            b = sequence_avg_logprob_from_tokens(torch.from_numpy(o.logprob.astype(np.float32)), toks)
            assert abs(a - b) < 1e-5, (temp, n, a, b)


# ------------------------------------------------------------------------------------------------ the oracle's sampler
LOGITS8 = np.array([1.5, -0.5, 0.25, -INF, 2.0, 0.0, -1.25, 0.75], np.float32)


@pytest.mark.parametrize("seed", [1234, 2 ** 40 + 7])
@pytest.mark.parametrize("t,top_k", [(0.7, 0), (1.3, 3)])
def test_oracle_sampler_frequencies(seed, t, top_k):
    """65 536 draws (4096 row ids x 16 steps) from fixed logits: every token's count within 4 standard deviations of N p (1 - p), and
    the share of equal neighbours within 0.003 of sum p^2.  Neighbours are the draws whose Philox counters differ by one in one word:
    (row id, step) with (row id + 1, step) and with (row id, step + 1), 126 960 pairs -- both words a decoder steps through.  At that
    count 0.003 is 2.2 standard deviations of a perfect sampler (sqrt(q (1 - q) / pairs) = 0.00136 at q = 0.38); the four cases give
    0.0006, 0.0025, 0.0019 and 0.0012.  Over the 65 535 pairs of one launch order alone (1.6 standard deviations) the second case gives
    0.0040: such a pair count cannot carry the bound."""
    rows, steps = 4096, 16
    x = np.tile(LOGITS8, (rows, 1))
    o0 = R.warp(x[:1], t, top_k)
    e = np.where(o0.kept[0], np.exp(o0.y[0].astype(np.float64) - o0.y[0].max()), 0.0)
    p = e / e.sum()
    grid = np.stack([R.sample(x, t, top_k, seed=seed, step=s, row_ids=np.arange(rows)).tokens for s in range(steps)])
    draws = grid.reshape(-1)
    N = draws.size
    equal = np.concatenate([(grid[:, 1:] == grid[:, :-1]).reshape(-1), (grid[1:] == grid[:-1]).reshape(-1)])
    counts = np.bincount(draws, minlength=8)
    assert counts[~o0.kept[0]].sum() == 0
    z = (counts - N * p)[p > 0] / np.sqrt(N * p * (1 - p))[p > 0]
    print("max |z|", np.abs(z).max(), "equal neighbours", equal.mean(), "of", equal.size, "sum p^2", (p * p).sum())
    assert np.abs(z).max() < 4.0
    assert abs(equal.mean() - (p * p).sum()) < 0.003

"""Repetition penalty and no-repeat n-grams in the decoders, on the small hashed plain-Whisper model of goldens F19 / F21
(tests/golden/make_golden_generate.py, make_golden_repetition.py; DiCoW with FDDT off is that model).

  * golden F21: transformers' own WhisperForConditionalGeneration.generate with the two options -- greedy (a)-(c) followed token by
    token while HF's recorded best-vs-second gap of the processed scores exceeds 0.15 (rule and threshold of
    test_generate_end_to_end_vs_transformers_whisper_generate), beam search (d) as a whole;
  * the kernel path against transformers' two processor classes applied to the same GPU tensors, on every decoding path;
  * options off: bit-equal to a call that does not pass them, and nothing is launched."""
import ast
from types import SimpleNamespace

import pytest
import torch

from tests.util import hashed_init_, hashed_mel, hashed_uniform, load_golden

pytestmark = pytest.mark.gpu

OPTS = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)


@pytest.fixture(scope="module")
def pkg():
    import amd_pkg
    return amd_pkg.load()


def make_x(variant, B=3):
    """make_golden_generate.make_x"""
    x = torch.from_numpy(hashed_mel(B, 80, 3000)).clone() + 0.6 * hashed_uniform(f"f19.x.{variant}", (B, 80, 3000))
    x[1] = x[1].flip(-1) * 0.7
    return x.clamp(-1.5, 1.5)


@pytest.fixture(scope="module")
def f19(pkg):
    """The F19 model on the GPU, its generation-config fields, the forced prompt and one window of input."""
    z = load_golden("f19_hf_generate")
    c, gen, scale = (ast.literal_eval(str(z[k])) for k in ("cfg", "gen", "scale"))
    cfg = pkg.DiCoWConfig(use_fddt=False, **c)
    model = pkg.DiCoWForConditionalGeneration(cfg)
    hashed_init_(model)
    d = model.model.decoder
    with torch.no_grad():                                      # the golden script's apply_scale()
        from ts_asr_whisper_amd.modeling import sinusoids
        model.model.encoder.embed_positions.weight.copy_(sinusoids(cfg.max_source_positions, cfg.d_model))
        d.embed_tokens.weight.mul_(scale["embed_tokens"]); d.embed_positions.weight.mul_(scale["embed_positions"])
        d.layer_norm.weight.mul_(scale["final_ln"])
        for l in d.layers:
            l.encoder_attn.q_proj.weight.mul_(scale["cross_q"]); l.encoder_attn.out_proj.weight.mul_(scale["cross_out"])
    model = model.cuda().eval()
    model.tie_weights()
    model.tokenizer = None
    prompt = torch.tensor([[gen["decoder_start_token_id"], gen["lang_to_id"]["<|de|>"], gen["task_to_id"]["transcribe"],
                            gen["no_timestamps_token_id"]]] * 3)
    st = torch.zeros(3, 4, 1500, device="cuda"); st[:, 1] = 1.0
    kw = dict(eos_token_id=gen["eos_token_id"], pad_token_id=gen["pad_token_id"], suppress_tokens=gen["suppress_tokens"],
              begin_suppress_tokens=gen["begin_suppress_tokens"])
    return SimpleNamespace(model=model, cfg=cfg, gen=gen, prompt=prompt, st=st, x=make_x(0).cuda(), kw=kw)


def via_processors(input_ids, scores, repetition_penalty=None, no_repeat_ngram_size=None):
    """generation.repetition_rules with transformers' two processor classes on the GPU tensors in place of the kernel."""
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    from ts_asr_whisper_amd.generation import repetition_options
    opt = repetition_options(repetition_penalty, no_repeat_ngram_size)
    if opt is None:
        return scores
    ids, out = input_ids.to(scores.device), scores
    if opt[0] != 1.0:
        out = RepetitionPenaltyLogitsProcessor(penalty=opt[0])(ids, out)
    if opt[1] > 0:
        out = NoRepeatNGramLogitsProcessor(opt[1])(ids, out.clone())
    scores.copy_(out)
    return scores


def both_paths(monkeypatch, fn):
    """fn() with the kernel, then with the processors; also the number of times each was called."""
    from ts_asr_whisper_amd import generation
    calls = [0, 0]
    real = generation.repetition_rules

    def counted(which, f):
        def g(*a, **k):
            calls[which] += 1
            return f(*a, **k)
        return g
    monkeypatch.setattr(generation, "repetition_rules", counted(0, real))
    a = fn()
    monkeypatch.setattr(generation, "repetition_rules", counted(1, via_processors))
    b = fn()
    monkeypatch.setattr(generation, "repetition_rules", real)
    assert calls[0] == calls[1] > 0
    return a, b


def ulp_apart(a, b):
    i, j = (t.contiguous().view(torch.int32).to(torch.int64) for t in (a, b))
    i, j = torch.where(i < 0, -(i & 0x7FFFFFFF), i), torch.where(j < 0, -(j & 0x7FFFFFFF), j)
    return int((i - j).abs().max())


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_f21_greedy_follows_transformers_generate(f19, case):
    """Golden F21 (a) repetition_penalty 1.3, (b) no_repeat_ngram_size 2, (c) penalty 1.3 with n-gram size 3, read from the
    generation config: HF's token at every position of each row's leading run with recorded gap >= 0.15; every row is followed for
    at least 8 of its 12 positions, and the followed tokens differ from the option-free run of the same input somewhere."""
    z = load_golden("f21_repetition")
    seq, plain, gaps = z[f"{case}.seq"], z[f"{case}.plain"], z[f"{case}.gaps"]
    opts = ast.literal_eval(str(z[f"{case}.opts"]))
    B, n_new = seq.shape
    assert (B, n_new) == (3, 12)
    x = make_x(int(z[f"{case}.variant"])).cuda()
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **opts)
    out = f19.model.generate(input_features=x, stno_mask=f19.st, generation_config=gc, max_new_tokens=n_new).cpu()
    P = f19.prompt.shape[1]
    assert out[:, :P].tolist() == f19.prompt.tolist()
    differs = False
    for b in range(B):
        n = 0
        for i in range(n_new):
            if gaps[b, i] < 0.15:
                break
            assert int(out[b, P + i]) == int(seq[b, i]), (case, b, i, out[b].tolist(), seq[b].tolist())
            differs |= int(seq[b, i]) != int(plain[b, i])
            n += 1
        print(f"F21 {case} row {b}: followed {n} of {n_new} positions, gaps {[round(float(v), 2) for v in gaps[b]]}")
        assert n >= 8, (case, b, n)
    assert differs


def test_f21_beam_search_equals_transformers_generate(f19):
    """Golden F21 (d): penalty 1.3, n-gram size 3, three beams; HF's result is stable under +-0.08 noise on the processed scores."""
    z = load_golden("f21_repetition")
    opts = ast.literal_eval(str(z["d.opts"]))
    x = make_x(int(z["d.variant"])).cuda()
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **opts)
    out = f19.model.generate(input_features=x, stno_mask=f19.st, generation_config=gc, max_new_tokens=z["d.seq"].shape[1]).cpu()
    P = f19.prompt.shape[1]
    print("F21 d ours", out[:, P:].tolist(), "HF", z["d.seq"].tolist())
    assert out[:, P:].tolist() == z["d.seq"].tolist()
    assert out[:, P:].tolist() != z["d.plain"].tolist()


def test_kernel_path_equals_processor_path_greedy_scores_and_graphs(f19, monkeypatch):
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)
    run = lambda d: d.generate(f19.x, f19.st, f19.prompt, 12, return_scores=True, **f19.kw, **OPTS)    # noqa: E731
    (s_k, sc_k), (s_p, sc_p) = both_paths(monkeypatch, lambda: run(dec))
    assert torch.equal(s_k, s_p)
    assert torch.equal(torch.isfinite(sc_k), torch.isfinite(sc_p)) and torch.equal(torch.isneginf(sc_k), torch.isneginf(sc_p))
    fin = torch.isfinite(sc_k)
    assert ulp_apart(sc_k[fin], sc_p[fin]) <= 2
    plain = dec.generate(f19.x, f19.st, f19.prompt, 12, **f19.kw)
    assert not torch.equal(plain, s_k)                           # (the options decide tokens on this model)
    graphed = GreedyDecoder(f19.model, use_graphs=True)
    (g_k, _), (g_p, _) = both_paths(monkeypatch, lambda: run(graphed))
    assert torch.equal(g_k, g_p) and torch.equal(g_k, s_k)


def test_kernel_path_equals_processor_path_beam_search(f19, monkeypatch):
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)
    P = f19.prompt.shape[1]
    (s_k, f_k), (s_p, f_p) = both_paths(monkeypatch, lambda: dec.beam_search(f19.x, f19.st, f19.prompt, P + 12, 3, **f19.kw, **OPTS))
    assert torch.equal(s_k, s_p)
    assert float((f_k - f_p).abs().max()) < 1e-4
    plain, _ = dec.beam_search(f19.x, f19.st, f19.prompt, P + 12, 3, **f19.kw)
    assert plain.shape != s_k.shape or not torch.equal(plain, s_k)


def test_kernel_path_equals_processor_path_fallback_ladder(f19, monkeypatch):
    """A log-probability threshold nothing can meet: every window climbs the whole ladder, the sampling passes included."""
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)

    def run():
        g = torch.Generator(device="cuda").manual_seed(5)
        return dec.generate_with_fallback(f19.x, f19.st, f19.prompt, 8, temperatures=(0.0, 0.7, 1.3), compression_ratio_threshold=None,
                                          logprob_threshold=1.0, generator=g, **f19.kw, **OPTS)
    a, b = both_paths(monkeypatch, run)
    assert a == b and a[2] == [2, 2, 2]


def test_kernel_path_equals_processor_path_long_form(f19, monkeypatch):
    """Two windows per recording: every window's history starts from that window's prompt.  Every timestamp but <|0.20|> is
    suppressed, so a window opens with it and cannot close a segment: each window is consumed whole."""
    from ts_asr_whisper_amd.generation import LongFormDecoder
    gen, W = f19.gen, 2 * f19.cfg.max_source_positions
    no_ts = gen["no_timestamps_token_id"]
    x = torch.cat([f19.x[:2], f19.x[:2, :, :800].flip(-1)], dim=-1)
    st = torch.zeros(2, 4, x.shape[-1] // 2, device="cuda"); st[:, 1] = 1.0
    sup = [t for t in gen["suppress_tokens"] if t <= no_ts] + [t for t in range(no_ts + 1, f19.cfg.vocab_size) if t != no_ts + 11]
    lf = LongFormDecoder(f19.model)
    windows = []
    inner = lf.decoder.generate
    monkeypatch.setattr(lf.decoder, "generate", lambda *a, **k: (windows.append(a[2].shape), inner(*a, **k))[1])

    def run():
        return lf.transcribe(x, st, [W + 800, W + 500], f19.prompt[:1, :3], no_ts, eos_token_id=gen["eos_token_id"],
                             pad_token_id=gen["pad_token_id"], max_new_tokens=8, suppress_tokens=sup,
                             begin_suppress_tokens=gen["begin_suppress_tokens"], **OPTS)
    a, b = both_paths(monkeypatch, run)
    assert len(windows) == 4                                      # two batched windows per run
    assert a == b and all(len(rec) == 2 for rec in a)
    for rec in a:                                                 # n-gram size 3: no trigram twice within a window's tokens
        for seg in rec:
            t = seg["tokens"]
            tri = [tuple(t[i:i + 3]) for i in range(len(t) - 2)]
            assert len(tri) == len(set(tri))


def test_options_off_is_bit_equal_and_launches_nothing(f19, monkeypatch):
    from ts_asr_whisper_amd import _lib
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)
    P = f19.prompt.shape[1]
    s0, sc0 = dec.generate(f19.x, f19.st, f19.prompt, 10, return_scores=True, **f19.kw)
    b0, f0 = dec.beam_search(f19.x, f19.st, f19.prompt, P + 10, 3, **f19.kw)
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen)
    m0 = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=gc, max_new_tokens=10)
    real = _lib.call

    def call(name, *args):
        assert name != "dicow_repetition_rules", "launched with both options off"
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    for off in (dict(repetition_penalty=1.0, no_repeat_ngram_size=0), dict(repetition_penalty=None, no_repeat_ngram_size=None)):
        s1, sc1 = dec.generate(f19.x, f19.st, f19.prompt, 10, return_scores=True, **f19.kw, **off)
        assert torch.equal(s0, s1) and torch.equal(sc0.view(torch.int32), sc1.view(torch.int32))
        b1, f1 = dec.beam_search(f19.x, f19.st, f19.prompt, P + 10, 3, **f19.kw, **off)
        assert torch.equal(b0, b1) and torch.equal(f0.view(torch.int32), f1.view(torch.int32))
        gc1 = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **off)
        assert torch.equal(m0, f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=gc1, max_new_tokens=10))

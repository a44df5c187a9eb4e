"""sequence_bias and bad_words_ids in the decoders, on the small hashed plain-Whisper model of goldens F19 / F27
(tests/golden/make_golden_generate.py, make_golden_sequence_bias.py; DiCoW with FDDT off is that model).

  * golden F27: transformers' own WhisperForConditionalGeneration.generate with the two options -- greedy (a)-(c) followed token by
    token while HF's recorded best-vs-second gap of the processed scores exceeds 0.15 (rule and threshold of
    test_gpu_repetition_decode.py), beam search (d) as a whole;
  * the kernel path against transformers' two processor classes applied to CPU copies of the same tensors, on every decoding path;
  * options in the generation config equal options as keywords;
  * options off: bit-equal to a call that does not pass them, and nothing is launched."""
import ast
from types import SimpleNamespace

import pytest
import torch

from tests.test_gpu_repetition_decode import f19, make_x, pkg  # noqa: F401  (fixtures: the F19 model on the GPU)
from tests.util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opts():
    """Golden F27 (c)'s options -- banned words, biased sequences and repetition_penalty 1.3, chosen on input variant 0, the input of
    the `f19` fixture -- split into the decoders' keywords."""
    z = load_golden("f27_sequence_bias")
    assert int(z["c.variant"]) == 0
    o = ast.literal_eval(str(z["c.opts"]))
    assert set(o) == {"bad_words_ids", "sequence_bias", "repetition_penalty"}
    return o


def table_entries(table):
    """{sequence: bias} of a device table, in table order."""
    buf = table.buf.cpu()
    n, g = table.n_seq, table.n_groups
    off = buf[:n + 1].tolist()
    bias = buf[n + 1 + g + 1:n + 1 + g + 1 + n].clone().view(torch.float32).tolist()
    tok = buf[n + 1 + g + 1 + n:].tolist()
    return {tuple(tok[off[i]:off[i + 1]]): bias[i] for i in range(n)}


def via_processor(input_ids, scores, table, plan=0):
    """generation.sequence_bias_rules with transformers' SequenceBiasLogitsProcessor on CPU copies in place of the kernel (a table of
    -inf biases is what NoBadWordsLogitsProcessor hands to that class).  Table order keeps the caller's order within a last token,
    the only order the sum depends on."""
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    if table is None or table.n_seq == 0:
        return scores
    out = SequenceBiasLogitsProcessor(sequence_bias=table_entries(table))(input_ids.cpu(), scores.cpu().clone())
    scores.copy_(out)
    return scores


def both_paths(monkeypatch, fn):
    """fn() with the kernel, then with the processor; also the number of times each was called."""
    from ts_asr_whisper_amd import generation
    calls = [0, 0]
    real = generation.sequence_bias_rules

    def counted(which, f):
        def g(*a, **k):
            calls[which] += 1
            return f(*a, **k)
        return g
    monkeypatch.setattr(generation, "sequence_bias_rules", counted(0, real))
    a = fn()
    monkeypatch.setattr(generation, "sequence_bias_rules", counted(1, via_processor))
    b = fn()
    monkeypatch.setattr(generation, "sequence_bias_rules", real)
    assert calls[0] == calls[1] > 0
    return a, b


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_f27_greedy_follows_transformers_generate(f19, case):  # noqa: F811
    """Golden F27 (a) bad_words_ids, (b) sequence_bias, (c) both with repetition_penalty 1.3, read from the generation config: HF's
    token at every position of each row's leading run with recorded gap >= 0.15; every row is followed for at least 8 of its 12
    positions, and the followed tokens differ from the option-free run of the same input somewhere."""
    z = load_golden("f27_sequence_bias")
    seq, plain, gaps = z[f"{case}.seq"], z[f"{case}.plain"], z[f"{case}.gaps"]
    o = ast.literal_eval(str(z[f"{case}.opts"]))
    B, n_new = seq.shape
    assert (B, n_new) == (3, 12)
    x = make_x(int(z[f"{case}.variant"])).cuda()
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **o)
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
        print(f"F27 {case} row {b}: followed {n} of {n_new} positions, gaps {[round(float(v), 2) for v in gaps[b]]}")
        assert n >= 8, (case, b, n)
    assert differs


def test_f27_beam_search_equals_transformers_generate(f19):  # noqa: F811
    """Golden F27 (d): both options, penalty 1.3, three beams; HF's result is stable under +-0.08 noise on the processed scores."""
    z = load_golden("f27_sequence_bias")
    o = ast.literal_eval(str(z["d.opts"]))
    x = make_x(int(z["d.variant"])).cuda()
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **o)
    out = f19.model.generate(input_features=x, stno_mask=f19.st, generation_config=gc, max_new_tokens=z["d.seq"].shape[1]).cpu()
    P = f19.prompt.shape[1]
    print("F27 d ours", out[:, P:].tolist(), "HF", z["d.seq"].tolist())
    assert out[:, P:].tolist() == z["d.seq"].tolist()
    assert out[:, P:].tolist() != z["d.plain"].tolist()


def test_kernel_path_equals_processor_path_greedy_scores_and_graphs(f19, opts, monkeypatch):  # noqa: F811
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)
    run = lambda d: d.generate(f19.x, f19.st, f19.prompt, 12, return_scores=True, **f19.kw, **opts)    # noqa: E731
    (s_k, sc_k), (s_p, sc_p) = both_paths(monkeypatch, lambda: run(dec))
    assert torch.equal(s_k, s_p)
    assert not torch.isnan(sc_k).any() and torch.equal(sc_k, sc_p)    # (as numbers: the same adds; transformers may flip a -0.0)
    plain = dec.generate(f19.x, f19.st, f19.prompt, 12, **f19.kw)
    assert not torch.equal(plain, s_k)                           # (the options decide tokens on this model)
    # each option alone is honoured too, and differs from both options together
    for one in ("sequence_bias", "bad_words_ids"):
        (a, _), (b, _) = both_paths(monkeypatch, lambda: dec.generate(f19.x, f19.st, f19.prompt, 12, return_scores=True, **f19.kw,
                                                                      **{one: opts[one]}))
        assert torch.equal(a, b) and not torch.equal(a, plain)
    graphed = GreedyDecoder(f19.model, use_graphs=True)
    (g_k, _), (g_p, _) = both_paths(monkeypatch, lambda: run(graphed))
    assert torch.equal(g_k, g_p) and torch.equal(g_k, s_k)


def test_kernel_path_equals_processor_path_beam_search(f19, opts, monkeypatch):  # noqa: F811
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)
    P = f19.prompt.shape[1]
    (s_k, f_k), (s_p, f_p) = both_paths(monkeypatch, lambda: dec.beam_search(f19.x, f19.st, f19.prompt, P + 12, 3, **f19.kw, **opts))
    assert torch.equal(s_k, s_p) and torch.equal(f_k, f_p)
    plain, _ = dec.beam_search(f19.x, f19.st, f19.prompt, P + 12, 3, **f19.kw)
    assert plain.shape != s_k.shape or not torch.equal(plain, s_k)


def test_kernel_path_equals_processor_path_fallback_ladder(f19, opts, monkeypatch):  # noqa: F811
    """A log-probability threshold nothing can meet: every window climbs the whole ladder, the sampling passes included."""
    from ts_asr_whisper_amd.generation import GreedyDecoder
    dec = GreedyDecoder(f19.model)

    def run():
        g = torch.Generator(device="cuda").manual_seed(5)
        return dec.generate_with_fallback(f19.x, f19.st, f19.prompt, 8, temperatures=(0.0, 0.7, 1.3), compression_ratio_threshold=None,
                                          logprob_threshold=1.0, generator=g, **f19.kw, **opts)
    a, b = both_paths(monkeypatch, run)
    assert a == b and a[2] == [2, 2, 2]
    banned = {w[0] for w in opts["bad_words_ids"] if len(w) == 1}
    assert banned and not any(t in banned for toks in a[0] for t in toks)      # sampling cannot draw a banned token either


def test_kernel_path_equals_processor_path_long_form(f19, opts, monkeypatch):  # noqa: F811
    """Two windows per recording: every window's history starts from that window's prompt.  Every timestamp but <|0.20|> is
    suppressed, so a window opens with it and cannot close a segment: each window is consumed whole."""
    from ts_asr_whisper_amd.generation import LongFormDecoder
    gen, W = f19.gen, 2 * f19.cfg.max_source_positions
    no_ts = gen["no_timestamps_token_id"]
    x = torch.cat([f19.x[:2], f19.x[:2, :, :800].flip(-1)], dim=-1)
    st = torch.zeros(2, 4, x.shape[-1] // 2, device="cuda"); st[:, 1] = 1.0
    sup = [t for t in gen["suppress_tokens"] if t <= no_ts] + [t for t in range(no_ts + 1, f19.cfg.vocab_size) if t != no_ts + 11]
    lf = LongFormDecoder(f19.model)

    def run(**o):
        return lf.transcribe(x, st, [W + 800, W + 500], f19.prompt[:1, :3], no_ts, eos_token_id=gen["eos_token_id"],
                             pad_token_id=gen["pad_token_id"], max_new_tokens=8, suppress_tokens=sup,
                             begin_suppress_tokens=gen["begin_suppress_tokens"], **o)
    a, b = both_paths(monkeypatch, lambda: run(**opts))
    assert a == b and all(len(rec) == 2 for rec in a)
    assert a != run()
    pair = tuple(next(w for w in opts["bad_words_ids"] if len(w) == 2))
    for rec in a:                                                 # the banned pair occurs in no window's tokens
        for seg in rec:
            t = seg["tokens"]
            assert pair not in {tuple(t[i:i + 2]) for i in range(len(t) - 1)}


def test_generation_config_equals_keywords(f19, opts):  # noqa: F811
    base = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen)
    in_config = SimpleNamespace(**vars(base), **opts)
    for beams in (1, 3):
        a = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=in_config, max_new_tokens=10, num_beams=beams)
        b = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=base, max_new_tokens=10, num_beams=beams, **opts)
        plain = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=base, max_new_tokens=10, num_beams=beams)
        assert torch.equal(a, b) and (a.shape != plain.shape or not torch.equal(a, plain))
    # keywords win over the config
    other = dict(sequence_bias={(454, 7): 1.0}, bad_words_ids=[[3]])     # (nothing that bites: token 7 is suppressed, 3 is never chosen)
    c = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=in_config, max_new_tokens=10, **other)
    d = f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=base, max_new_tokens=10, **other,
                           repetition_penalty=opts["repetition_penalty"])
    assert torch.equal(c, d)


def test_options_off_is_bit_equal_and_launches_nothing(f19, monkeypatch):  # noqa: F811
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
        assert name != "dicow_sequence_bias", "launched with both options off"
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    off = dict(sequence_bias=None, bad_words_ids=None)
    s1, sc1 = dec.generate(f19.x, f19.st, f19.prompt, 10, return_scores=True, **f19.kw, **off)
    assert torch.equal(s0, s1) and torch.equal(sc0.view(torch.int32), sc1.view(torch.int32))
    b1, f1 = dec.beam_search(f19.x, f19.st, f19.prompt, P + 10, 3, **f19.kw, **off)
    assert torch.equal(b0, b1) and torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    gc1 = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen, **off)
    assert torch.equal(m0, f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=gc1, max_new_tokens=10))
    # banned words that are all eos ids ban nothing (transformers filters them out): still nothing is launched
    eos = f19.gen["eos_token_id"]
    s2 = dec.generate(f19.x, f19.st, f19.prompt, 10, **f19.kw, bad_words_ids=[[eos]])
    assert torch.equal(s0, s2)

"""The device sampler in the decoders, on the small hashed plain-Whisper model of golden F19 (tests/test_gpu_repetition_decode.py's
fixture): the argmax rung against today's torch loop, a sampling rung against its own warped scores, the temperature ladder on token
log-probabilities (decisions, memory, reproducibility), the long form, and the default path, which launches nothing new."""
from types import SimpleNamespace

import pytest
import torch

from tests import sampling_ref as R
from tests.test_gpu_repetition_decode import f19, make_x, pkg  # noqa: F401  (fixtures: the F19 model on the GPU)

pytestmark = pytest.mark.gpu

N_NEW = 10


@pytest.fixture(scope="module")
def dec(f19):  # noqa: F811
    from ts_asr_whisper_amd.generation import GreedyDecoder
    return GreedyDecoder(f19.model)


def test_greedy_rung_equals_the_torch_loop(f19, dec):  # noqa: F811
    s0, sc0 = dec.generate(f19.x, f19.st, f19.prompt, N_NEW, return_scores=True, **f19.kw)
    s1, lp1 = dec.generate(f19.x, f19.st, f19.prompt, N_NEW, seed=3, return_logprobs=True, **f19.kw)
    assert torch.equal(s0, s1)
    P = f19.prompt.shape[1]
    n = s0.shape[1] - P
    assert lp1.shape == (n, 3) and lp1.dtype == torch.float32
    want = torch.log_softmax(sc0.double(), dim=-1).gather(2, s0[:, P:].t()[:, :, None])[:, :, 0]
    live = torch.ones(3, dtype=torch.bool, device="cuda")
    eos = f19.kw["eos_token_id"]
    for i in range(n):                                                   # (a finished row's log-probability is 0)
        w = torch.where(live, want[i], torch.zeros_like(want[i]))
        err = (lp1[i].double() - w).abs()
        assert (err <= R.LOGPROB_REL * w.abs() + R.LOGPROB_ABS).all(), (i, lp1[i].tolist(), w.tolist())
        live = live & (s0[:, P + i] != eos)
    s2, sc2, lp2 = dec.generate(f19.x, f19.st, f19.prompt, N_NEW, seed=3, return_scores=True, return_logprobs=True, **f19.kw)
    assert torch.equal(s2, s0) and torch.equal(lp2.view(torch.int32), lp1.view(torch.int32))
    assert torch.equal(sc2.view(torch.int32), sc0.view(torch.int32))      # (the argmax rung: warped = the processed scores)
    g = dec.__class__(f19.model, use_graphs=True)
    s3, lp3 = g.generate(f19.x, f19.st, f19.prompt, N_NEW, seed=3, return_logprobs=True, **f19.kw)
    assert torch.equal(s3, s0) and torch.equal(lp3.view(torch.int32), lp1.view(torch.int32))


def test_sampling_rung(f19, dec):  # noqa: F811
    run = lambda **o: dec.generate(f19.x, f19.st, f19.prompt, N_NEW, temperature=0.7, top_k=5, return_scores=True,  # noqa: E731
                                   return_logprobs=True, **f19.kw, **o)
    s1, w1, lp1 = run(seed=11)
    s2, w2, lp2 = run(seed=11)
    assert torch.equal(s1, s2) and torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(lp1.view(torch.int32), lp2.view(torch.int32))
    s3, _, _ = run(seed=12)
    assert s3.shape != s1.shape or not torch.equal(s3, s1)
    P = f19.prompt.shape[1]
    live = torch.ones(3, dtype=torch.bool, device="cuda")
    for i in range(s1.shape[1] - P):
        kept = w1[i] > -float("inf")
        assert ((w1[i] == -float("inf")) | kept).all() and (kept.sum(1) == 5).all()      # exactly -inf outside the five kept
        top5 = torch.topk(w1[i], 5).indices
        tok = s1[:, P + i]
        assert ((top5 == tok[:, None]).any(1) | ~live).all(), f"position {i}: a token outside the five highest"
        live = live & (tok != f19.kw["eos_token_id"])
    with pytest.raises(ValueError):
        run(seed=1, generator=torch.Generator(device="cuda"))


def _ladder(dec, f19, **o):  # noqa: F811
    return dec.generate_with_fallback(f19.x, f19.st, f19.prompt, 8, temperatures=(0.0, 0.7, 1.3), compression_ratio_threshold=None,
                                      **f19.kw, **o)


def test_fallback_on_token_logprobs(f19, dec, monkeypatch):  # noqa: F811
    from ts_asr_whisper_amd import generation
    a = _ladder(dec, f19, logprob_threshold=1.0, top_k=5, seed=21)        # a threshold nothing can meet: the whole ladder
    b = _ladder(dec, f19, logprob_threshold=1.0, top_k=5, seed=21)
    assert a == b and a[2] == [2, 2, 2]
    assert _ladder(dec, f19, logprob_threshold=1.0, top_k=5, seed=22)[0] != a[0]
    # memory: no [n, B, V] tensor is held
    peaks = []
    for o in (dict(top_k=5, seed=21), dict(generator=torch.Generator(device="cuda").manual_seed(5))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _ladder(dec, f19, logprob_threshold=1.0, **o)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
    print("fallback peak memory: token log-probabilities", peaks[0], "bytes, return_scores", peaks[1], "bytes")
    assert peaks[0] < peaks[1]
    # decisions: a threshold between the windows' greedy averages; every rung's verdict must be the one sequence_avg_logprob gives on
    # the warped scores of that same decode
    seen = []
    real = generation.GreedyDecoder.generate

    def spy(self, *args, **kw):
        out = real(self, *args, **{**kw, "return_scores": True})
        seen.append((kw["temperature"], list(kw["row_ids"]), out))
        return out[0], out[2]
    monkeypatch.setattr(generation.GreedyDecoder, "generate", spy)
    P = f19.prompt.shape[1]
    eos, pad = f19.kw["eos_token_id"], f19.kw["pad_token_id"]

    def averages(temp, seqs, warped, lps, j):
        toks = seqs[j, P:].tolist()
        if toks and toks[-1] == pad:                                     # (decode_with_fallback's trimming of the padding tail)
            npad = sum(1 for t in toks if t == pad) - (1 if pad == eos else 0)
            toks = toks[:-npad] if npad else toks
        return generation.sequence_avg_logprob(warped[:, j], toks, temp), generation.sequence_avg_logprob_from_tokens(lps[:, j], toks)

    assert _ladder(dec, f19, logprob_threshold=1.0, top_k=5, seed=21) == a
    greedy = sorted(averages(seen[0][0], *seen[0][2], j)[0] for j in range(3))
    seen.clear()
    thr = 0.5 * (greedy[0] + greedy[1])                                   # the least likely window falls back, the others do not
    _, _, used = _ladder(dec, f19, logprob_threshold=thr, top_k=5, seed=21)
    assert used.count(0) == 2 and len(seen) >= 2
    for k, (temp, rows, out) in enumerate(seen):
        again = []
        for j, r in enumerate(rows):
            from_scores, from_tokens = averages(temp, *out, j)
            assert abs(from_scores - from_tokens) <= 1e-4 * max(1.0, abs(from_scores)), (k, r, from_scores, from_tokens)
            if from_scores < thr:
                again.append(r)
            elif used[r] != k:
                raise AssertionError(f"window {r} passed at rung {k} but ended at rung {used[r]}")
        if k + 1 < len(seen):
            assert seen[k + 1][1] == again, (k, again, seen[k + 1][1])
        else:
            assert not again or k == 2


def test_long_form_runs_and_reproduces(f19):  # noqa: F811
    from ts_asr_whisper_amd.generation import LongFormDecoder
    gen, W = f19.gen, 2 * f19.cfg.max_source_positions
    no_ts = gen["no_timestamps_token_id"]
    x = torch.cat([f19.x[:2], f19.x[:2, :, :800].flip(-1)], dim=-1)
    st = torch.zeros(2, 4, x.shape[-1] // 2, device="cuda"); st[:, 1] = 1.0
    sup = [t for t in gen["suppress_tokens"] if t <= no_ts] + [t for t in range(no_ts + 1, f19.cfg.vocab_size) if t != no_ts + 11]
    lf = LongFormDecoder(f19.model)
    streams = []
    real = lf.decoder.generate_with_fallback

    def spy(*a, **k):
        streams.append((list(k["row_ids"]), k["stream"]))
        return real(*a, **k)
    lf.decoder.generate_with_fallback = spy

    def run(**o):
        return lf.transcribe(x, st, [W + 800, W + 500], f19.prompt[:1, :3], no_ts, eos_token_id=gen["eos_token_id"],
                             pad_token_id=gen["pad_token_id"], max_new_tokens=8, suppress_tokens=sup,
                             begin_suppress_tokens=gen["begin_suppress_tokens"], temperatures=(0.0, 0.7), compression_ratio_threshold=None,
                             logprob_threshold=1.0, no_speech_token_id=no_ts - 1, **o)
    a = run(top_k=5, seed=31)
    assert streams == [([0, 1], 0), ([0, 1], 16)]                         # recording ids, and iteration * 16: no counter is shared
    assert a == run(top_k=5, seed=31) and all(len(rec) == 2 for rec in a)
    assert a != run(top_k=5, seed=32)

    class Tok:
        prefix_tokens = f19.prompt[0, :3].tolist()
        pad_token_id = gen["pad_token_id"]

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 220}

    f19.model.tokenizer = Tok()
    try:
        gc = SimpleNamespace(return_timestamps=True, **{**gen, "suppress_tokens": sup})
        kw = dict(input_features=x, stno_mask=st, attention_mask=(torch.arange(x.shape[-1], device="cuda")[None] <
                                                                  torch.tensor([[W + 800], [W + 500]], device="cuda")).long(),
                  decoder_input_ids=f19.prompt[:1, :3], generation_config=gc, max_new_tokens=8, temperature=(0.0, 0.7),
                  compression_ratio_threshold=None, logprob_threshold=1.0, top_k=5)
        m1 = f19.model.generate(seed=31, **kw)
        assert torch.equal(m1, f19.model.generate(seed=31, **kw))
        assert f19.model.last_segments == a
    finally:
        f19.model.tokenizer = None


def test_default_path_launches_no_sampler(f19, dec, monkeypatch):  # noqa: F811
    from ts_asr_whisper_amd import _lib
    real, real_struct = _lib.call, _lib.call_struct

    def call(name, *args):
        assert name != "dicow_sample_tokens", "launched without any sampling option"
        return real(name, *args)

    def call_struct(name, st):
        assert name != "dicow_sample_tokens", "launched without any sampling option"
        return real_struct(name, st)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "call_struct", call_struct)
    dec.generate(f19.x, f19.st, f19.prompt, 6, return_scores=True, **f19.kw)
    dec.generate(f19.x, f19.st, f19.prompt, 6, temperature=0.7, generator=torch.Generator(device="cuda").manual_seed(1), **f19.kw)
    dec.generate_with_fallback(f19.x, f19.st, f19.prompt, 6, temperatures=(0.0, 0.7), compression_ratio_threshold=None, logprob_threshold=1.0,
                               generator=torch.Generator(device="cuda").manual_seed(1), **f19.kw)
    gc = SimpleNamespace(language="de", task="transcribe", return_timestamps=False, **f19.gen)
    f19.model.generate(input_features=f19.x, stno_mask=f19.st, generation_config=gc, max_new_tokens=6)
    with pytest.raises(AssertionError, match="launched without"):        # (the spy does see the launch when an option is set)
        dec.generate(f19.x, f19.st, f19.prompt, 6, top_k=5, **f19.kw)

#!/usr/bin/env python3
"""Golden F21: transformers' own `WhisperForConditionalGeneration.generate` with `repetition_penalty` / `no_repeat_ngram_size` -- the
two options HF's generate (which the reference's delegates to) turns into RepetitionPenaltyLogitsProcessor and
NoRepeatNGramLogitsProcessor IN FRONT of Whisper's own processors -- on golden F19's small hashed model:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_repetition.py

That model, decoded plainly, soon repeats one token, so the options change almost every decision.  Cases, each with
language="de", task="transcribe", 12 new tokens, B = 3:
    (a) repetition_penalty=1.3      (b) no_repeat_ngram_size=2      (c) both, n-gram size 3      (d) = (c) with num_beams=3
Per case the fixture holds the input variant, HF's sequences, the option-free sequences of the same variant (same search) and, for
the greedy cases, the best-minus-second gap of the PROCESSED scores per position (make_golden_generate.Gaps).

Greedy cases take the first input variant (of 48) in which every row's leading run of positions with gap >= 0.25 covers at least 8
of the 12 positions and, inside those runs, at least one token differs from the option-free run.
A single-token gap says nothing about a beam search, so case (d) takes the first variant (of 16) whose result does not move when a
processor adding uniform noise of +-0.08 to the processed scores is appended (three seeds, all must agree; 0.08 = the 6e-2 bf16
score error the F19 test states, times the penalty 1.3) and differs from the option-free beam result."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np
import torch
from transformers.generation.logits_process import LogitsProcessor, LogitsProcessorList

from tests.golden.make_golden_generate import apply_scale, build, make_x, run  # noqa: F401  (apply_scale: what build() applied)

N_NEW, MIN_GAP, MIN_RUN, NOISE = 12, 0.25, 8, 0.08
BASE = dict(language="de", task="transcribe", max_new_tokens=N_NEW)
CASES = {"a": dict(repetition_penalty=1.3), "b": dict(no_repeat_ngram_size=2),
         "c": dict(repetition_penalty=1.3, no_repeat_ngram_size=3),
         "d": dict(repetition_penalty=1.3, no_repeat_ngram_size=3, num_beams=3)}


class Noise(LogitsProcessor):
    """Last processor of the chain: uniform noise in [-NOISE, NOISE) on every (finite) processed score."""
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, input_ids, scores):
        return scores + (torch.rand(scores.shape, generator=self.g) * 2.0 - 1.0) * NOISE


def leading_runs(gaps):
    """Per row: number of leading positions whose gap is >= MIN_GAP."""
    return [int((torch.cumprod((row >= MIN_GAP).long(), 0)).sum()) for row in gaps]


def greedy_case(m, opts):
    for variant in range(48):
        x = make_x(variant)
        with torch.no_grad():
            seq, gaps = run(m, x, **BASE, **opts)
            plain, _ = run(m, x, **BASE)
        runs = leading_runs(gaps)
        n = min(seq.shape[1], plain.shape[1])
        differs = any(int(seq[b, i]) != int(plain[b, i]) for b in range(seq.shape[0]) for i in range(min(runs[b], n)))
        print(opts, "variant", variant, "runs", runs, "differs", differs)
        if seq.shape[1] == N_NEW and min(runs) >= MIN_RUN and differs:
            return dict(variant=np.array(variant), seq=seq.numpy(), plain=plain.numpy(), gaps=gaps.numpy())
    raise AssertionError(f"no input variant with decisive scores for {opts}")


def beam_case(m, opts):
    for variant in range(16):
        x = make_x(variant)
        with torch.no_grad():
            seq, _ = run(m, x, **BASE, **opts)
            noisy = [m.generate(x, logits_processor=LogitsProcessorList([Noise(s)]), **BASE, **opts) for s in (1, 2, 3)]
            plain, _ = run(m, x, **BASE, num_beams=opts["num_beams"])
        stable = all(torch.equal(seq, q) for q in noisy)
        differs = seq.shape != plain.shape or not torch.equal(seq, plain)
        print(opts, "variant", variant, "stable under noise", stable, "differs", differs)
        if stable and differs:
            return dict(variant=np.array(variant), seq=seq.numpy(), plain=plain.numpy())
    raise AssertionError(f"no input variant with a noise-stable beam result for {opts}")


def main():
    m = build()
    arrs = {}
    for k, opts in CASES.items():
        got = beam_case(m, opts) if "num_beams" in opts else greedy_case(m, opts)
        arrs.update({f"{k}.{n}": v for n, v in got.items()})
        arrs[f"{k}.opts"] = np.array(repr(opts))
        print(k, "variant", int(got["variant"]), "seq", got["seq"].tolist(), "plain", got["plain"].tolist())
    import transformers
    arrs["_versions"] = np.array(f"torch {torch.__version__} transformers {transformers.__version__}")
    np.savez_compressed(os.path.join(HERE, "f21_repetition.npz"), **arrs)


if __name__ == "__main__":
    main()

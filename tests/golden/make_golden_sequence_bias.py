#!/usr/bin/env python3
"""Golden F27: transformers' own `WhisperForConditionalGeneration.generate` with `sequence_bias` / `bad_words_ids` -- the two options
HF's generate (which the reference's delegates to) turns into SequenceBiasLogitsProcessor (in front of the repetition penalty) and
NoBadWordsLogitsProcessor (behind the no-repeat n-grams), both IN FRONT of Whisper's own processors -- on golden F19's small hashed
model:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sequence_bias.py

Cases, each with language="de", task="transcribe", 12 new tokens, B = 3.  The sequences are taken from the option-free greedy run of
the SAME input variant (`options`), so that they bite:
    (a) bad_words_ids: row 0's fifth token alone, and row 1's third and fourth tokens as a pair;
    (b) sequence_bias: +BOOST on (row 0's first token, PROMOTED) -- PROMOTED is a token the plain run never chooses --, SINGLE on row 2's
        second token alone, -BOOST on (row 1's first token, row 1's second token);
    (c) both, plus repetition_penalty=1.3;            (d) = (c) with num_beams=3.
Per case the fixture holds the input variant, HF's sequences, the option-free sequences of the same variant (same search), the options
as repr and, for the greedy cases, the best-minus-second gap of the PROCESSED scores per position (make_golden_generate.Gaps).

Acceptance is golden F21's (make_golden_repetition.py), conditions and not measurements: greedy cases take the first input variant (of
48) in which every row's leading run of positions with gap >= 0.25 covers at least 8 of the 12 positions and, inside those runs, at
least one token differs from the option-free run; case (d) takes the first variant (of 16) whose result does not move when a processor
adding uniform noise of +-0.08 to the processed scores is appended (three seeds, all must agree; F21's figure: the 6e-2 bf16 score
error the F19 test states, times the penalty 1.3) and differs from the option-free beam result.  On top of that condition case (d) must
hold under twice that noise as well (MARGIN, three more seeds): a beam's score sums the log-probabilities of its tokens, the promoted
token's among them, which lies deep in the tail of its distribution, where the GPU's bf16 error is larger than the figure stated for the
scores at the top -- the first variant that met the +-0.08 condition alone (2) turned over at +-0.16 in 4 of 10 seeds.  If no variant
qualifies the script raises: change BOOST / SINGLE / the positions above (inputs), never the thresholds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np
import torch
from transformers.generation.logits_process import LogitsProcessor, LogitsProcessorList

from tests.golden.make_golden_generate import GEN, build, make_x, run

N_NEW, MIN_GAP, MIN_RUN, NOISE = 12, 0.25, 8, 0.08
MARGIN = 2.0           # the beam case must also hold under MARGIN x NOISE (see the docstring): an extra condition, NOISE itself stays
BASE = dict(language="de", task="transcribe", max_new_tokens=N_NEW)
BOOST, SINGLE, PROMOTED = 40.0, -6.0, 5
CASES = {"a": ("bad",), "b": ("bias",), "c": ("bad", "bias", "penalty"), "d": ("bad", "bias", "penalty", "beams")}


class Noise(LogitsProcessor):
    """Last processor of the chain: uniform noise in [-NOISE, NOISE) on every (finite) processed score."""
    def __init__(self, seed, scale=1.0):
        self.g, self.amp = torch.Generator().manual_seed(seed), NOISE * scale

    def __call__(self, input_ids, scores):
        return scores + (torch.rand(scores.shape, generator=self.g) * 2.0 - 1.0) * self.amp


def options(plain, parts):
    """The case's generate() options from the option-free greedy tokens [3, 12] of the input variant."""
    p = plain.tolist()
    assert PROMOTED not in GEN["suppress_tokens"] and all(PROMOTED not in row for row in p)
    opts = {}
    if "bad" in parts:
        opts["bad_words_ids"] = [[p[0][4]], [p[1][2], p[1][3]]]
    if "bias" in parts:
        opts["sequence_bias"] = {(p[0][0], PROMOTED): BOOST, (p[2][1],): SINGLE, (p[1][0], p[1][1]): -BOOST}
    if "penalty" in parts:
        opts["repetition_penalty"] = 1.3
    if "beams" in parts:
        opts["num_beams"] = 3
    return opts


def leading_runs(gaps):
    """Per row: number of leading positions whose gap is >= MIN_GAP."""
    return [int((torch.cumprod((row >= MIN_GAP).long(), 0)).sum()) for row in gaps]


def greedy_case(m, parts):
    for variant in range(48):
        x = make_x(variant)
        with torch.no_grad():
            plain, _ = run(m, x, **BASE)
            if plain.shape[1] != N_NEW:
                continue
            opts = options(plain, parts)
            seq, gaps = run(m, x, **BASE, **opts)
        runs = leading_runs(gaps)
        n = min(seq.shape[1], plain.shape[1])
        differs = any(int(seq[b, i]) != int(plain[b, i]) for b in range(seq.shape[0]) for i in range(min(runs[b], n)))
        print(parts, "variant", variant, "runs", runs, "differs", differs)
        if seq.shape[1] == N_NEW and min(runs) >= MIN_RUN and differs:
            return dict(variant=np.array(variant), seq=seq.numpy(), plain=plain.numpy(), gaps=gaps.numpy()), opts
    raise AssertionError(f"no input variant with decisive scores for {parts}")


def beam_case(m, parts):
    for variant in range(16):
        x = make_x(variant)
        with torch.no_grad():
            greedy, _ = run(m, x, **BASE)
            if greedy.shape[1] != N_NEW:
                continue
            opts = options(greedy, parts)
            seq, _ = run(m, x, **BASE, **opts)
            noisy = [m.generate(x, logits_processor=LogitsProcessorList([Noise(s, k)]), **BASE, **opts) for k in (1.0, MARGIN)
                     for s in (1, 2, 3)]
            plain, _ = run(m, x, **BASE, num_beams=opts["num_beams"])
        stable = all(torch.equal(seq, q) for q in noisy)
        differs = seq.shape != plain.shape or not torch.equal(seq, plain)
        print(parts, "variant", variant, "stable under noise", stable, "differs", differs)
        if stable and differs:
            return dict(variant=np.array(variant), seq=seq.numpy(), plain=plain.numpy()), opts
    raise AssertionError(f"no input variant with a noise-stable beam result for {parts}")


def main():
    m = build()
    arrs = {}
    for k, parts in CASES.items():
        got, opts = beam_case(m, parts) if "beams" in parts else greedy_case(m, parts)
        arrs.update({f"{k}.{n}": v for n, v in got.items()})
        arrs[f"{k}.opts"] = np.array(repr(opts))
        print(k, "variant", int(got["variant"]), "opts", opts, "seq", got["seq"].tolist(), "plain", got["plain"].tolist())
    import transformers
    arrs["_versions"] = np.array(f"torch {torch.__version__} transformers {transformers.__version__}")
    np.savez_compressed(os.path.join(HERE, "f27_sequence_bias.npz"), **arrs)


if __name__ == "__main__":
    main()

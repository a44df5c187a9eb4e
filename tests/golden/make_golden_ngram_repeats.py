#!/usr/bin/env python3
"""Golden F26: the reference's own `truncate_at_repeating_ngram` (src/data/postprocess.py:18-74; pure Python, run on the CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ngram_repeats.py

The fixture holds, per case, the text, the parameter row (ngram_length, min_n, max_n or -1 for None, min_word_threshold, unigram_min_repeat,
repeat_threshold) and the string the reference returned.  Cases: a fixed list -- every rule of the definition in include/dicow_hip.h at its
edge, named below -- and seeded random texts over alphabets of 2-4 words under a pool of parameter rows.  At least a third of the cases
are cut and at least a third untouched (asserted)."""
import importlib.util
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DICOW_REFERENCE_SRC", "/root/reference/src")
spec = importlib.util.spec_from_file_location("reference_postprocess", os.path.join(REF, "data", "postprocess.py"))
postprocess = importlib.util.module_from_spec(spec)
spec.loader.exec_module(postprocess)

DEFAULT = (10, 1, -1, 30, 10, 10)
SMALL = (10, 1, -1, 0, 2, 1)                          # min_word_threshold=0, unigram_min_repeat=2, repeat_threshold=1


def row(ngram_length=10, min_n=1, max_n=-1, min_word_threshold=30, unigram_min_repeat=10, repeat_threshold=10):
    return (ngram_length, min_n, max_n, min_word_threshold, unigram_min_repeat, repeat_threshold)


def distinct(n, tag="w"):
    return " ".join(f"{tag}{k}" for k in range(n))


def fixed_cases():
    c = []
    # the hand cases: 29 words are below the threshold, 30 equal words are a unigram run, 25 words + "a a b" x 11 give 28
    c += [("a " * 29, DEFAULT), ("a " * 30, DEFAULT), (distinct(25) + " " + "a a b " * 11, DEFAULT)]
    # W of 29, 30 and 31 words of a two-word loop
    c += [(" ".join((["x", "y"] * 16)[:n]), DEFAULT) for n in (29, 30, 31)]
    # a run of u - 1 and of u words
    c += [(distinct(25) + " z" * 9, DEFAULT), (distinct(25) + " z" * 10, DEFAULT), (distinct(25) + " z" * 14 + " tail", DEFAULT)]
    # a count of r and of r + 1
    c += [(distinct(30) + " p q" * 10, DEFAULT), (distinct(30) + " p q" * 11, DEFAULT)]
    # "Yes yes YES": the run is case-insensitive, and an n-gram whose words differ only in case is degenerate
    c += [(distinct(20) + " Yes yes YES yes Yes YES yes yes YES Yes", DEFAULT), ("Yes yes " * 15, DEFAULT), ("Yes yes " * 15, row(min_n=2)),
          ("Yes yes no " * 12, row(min_n=2))]
    # "A b" against "a b": the counts are case-sensitive
    c += [("A b " * 8 + "a b " * 8, DEFAULT), ("A b " * 8 + "a b " * 8, row(repeat_threshold=7)), ("A b " * 11 + "a b " * 11, row(min_n=2))]
    # partly degenerate windows and overlapping occurrences
    c += [("a a b " * 12, DEFAULT), ("a a b " * 12, row(min_n=2)), ("a a a b " * 8, row(repeat_threshold=7)), ("a a a b " * 8, DEFAULT),
          ("a b " * 16, row(min_n=3)), ("a b " * 16, row(min_n=3, repeat_threshold=14)), ("a b " * 16, row(min_n=3, repeat_threshold=15)),
          ("a a a b " * 12, row(min_n=2)), ("a " * 11 + "b a " * 12, row(min_n=2))]
    # tabs, newlines and double spaces: an untouched text comes back as it is, a cut one joined by single spaces
    c += [("x\ty\n" * 15, DEFAULT), ("  one\ttwo\n\nthree  four  ", DEFAULT), ("\t" + distinct(28).replace(" ", "  ") + "\n", DEFAULT),
          (distinct(22).replace(" ", "\n") + "  u\tv" * 11 + " \n", DEFAULT), (" \t\n ", DEFAULT), (" \t\n ", SMALL)]
    # lower() of "İ" is "i" + a combining dot, of "ß" it is "ß" (neither "ss" nor "SS")
    dot = "İ".lower()
    c += [(distinct(20) + (" İ " + dot) * 5, DEFAULT), (distinct(21) + (" İ i") * 5, DEFAULT), (distinct(20) + " ß SS ss" * 3 + " ß", DEFAULT),
          (distinct(20) + " ß" * 10, DEFAULT), (("İ " + dot + " ") * 15, row(min_n=2)), ("ß SS " * 15, row(min_n=2)), ("ß SS ss " * 11, DEFAULT)]
    # the parameter rows: unigram rule off, min_n = 3, max_n = 3 below ngram_length, max_n = 16, ngram_length as the default of max_n
    loop13 = "a " * 11 + "b "
    c += [("a " * 40, row(min_n=2)), (distinct(5) + " a" * 40, row(min_n=3)), ("a b c " * 12, row(min_n=3)), ("a b c " * 12, row(max_n=3)),
          ("a b c d e " * 11, row(min_n=4, max_n=3)), ("a b c d e " * 11, row(min_n=3, max_n=3)), (loop13 * 12, row(min_n=13, max_n=16)),
          (loop13 * 12, row(min_n=12, max_n=16)), (loop13 * 12, row(min_n=2, max_n=16)), (loop13 * 11, row(min_n=2, max_n=16)),
          ("a b c d e f " * 11, row(ngram_length=5, min_n=5)), ("a b c d e f " * 11, row(ngram_length=16, min_n=16)),
          ("a b c d e f " * 11, row(ngram_length=12, max_n=3)), ("a b c d e f " * 11, row(ngram_length=1)),
          ("a b c d e f " * 11, row(ngram_length=3, min_n=4, max_n=6))]
    # small thresholds, and the empty string
    c += [("", DEFAULT), ("", SMALL), ("a", SMALL), ("a a", SMALL), ("a A", SMALL), ("a b", SMALL), ("a b a b", SMALL), ("a b a", SMALL),
          ("a b c a b c", SMALL), ("b a a", SMALL), ("a b b", SMALL), ("a b c a b", row(min_word_threshold=0, repeat_threshold=1)),
          ("a b c a b", row(min_word_threshold=6, repeat_threshold=1)), ("x a b c a b", row(min_word_threshold=6, repeat_threshold=1)),
          ("a a b b a a b b", row(min_word_threshold=0, unigram_min_repeat=3, repeat_threshold=1)),
          ("a b a b a b", row(min_word_threshold=0, unigram_min_repeat=1, repeat_threshold=5)), ("a", row(min_word_threshold=0, unigram_min_repeat=1)),
          ("a b", row(min_word_threshold=0, unigram_min_repeat=1)), ("thank you " * 40, DEFAULT),
          ("so we will see " + "thank you " * 30, DEFAULT)]
    return c


POOL = [DEFAULT, DEFAULT, row(min_n=2), row(min_n=3), row(max_n=3), row(max_n=16), (5, 1, -1, 0, 2, 1), SMALL, (4, 2, -1, 10, 3, 2), (16, 1, -1, 20, 5, 3),
        (3, 1, 16, 0, 4, 2), row(min_word_threshold=0, unigram_min_repeat=4, repeat_threshold=3)]
ALPHABETS = [["a", "b"], ["a", "A", "b"], ["yes", "Yes", "no", "NO"], ["x", "y", "z"], ["İ", "İ".lower(), "i", "ß"], ["the", "cat"], ["a", "b", "c", "d"]]


def random_cases(n, seed):
    rng = random.Random(seed)
    c = []
    for k in range(n):
        alphabet = rng.choice(ALPHABETS)
        kind = k % 3
        if kind == 0:                                # a plain random text over the alphabet
            words = [rng.choice(alphabet) for _ in range(rng.randrange(0, 72))]
        elif kind == 1:                              # distinct words with a loop somewhere behind them
            period = [rng.choice(alphabet) for _ in range(rng.randrange(1, 5))]
            words = [f"w{j}" for j in range(rng.randrange(0, 40))] + period * rng.randrange(1, 16) + [f"t{j}" for j in range(rng.randrange(0, 4))]
        else:                                        # mostly distinct words, a few of the alphabet strewn in
            words = [rng.choice(alphabet) if rng.random() < 0.3 else f"w{j}" for j in range(rng.randrange(0, 60))]
        c.append((rng.choice([" ", " ", "  ", "\t", "\n"]).join(words), rng.choice(POOL)))
    return c


def main():
    cases = fixed_cases() + random_cases(150, 26)
    outs = []
    for text, (ngram_length, min_n, max_n, mwt, u, r) in cases:
        outs.append(postprocess.truncate_at_repeating_ngram(text, ngram_length=ngram_length, min_n=min_n, max_n=None if max_n < 0 else max_n,
                                                            min_word_threshold=mwt, unigram_min_repeat=u, repeat_threshold=r))
    cut = sum(o != t for (t, _), o in zip(cases, outs))
    print(f"{len(cases)} cases, {cut} cut, {len(cases) - cut} untouched")
    assert 3 * cut >= len(cases) and 3 * (len(cases) - cut) >= len(cases)
    # the hand cases
    assert outs[0] == "a " * 29 and outs[1] == "a" and len(outs[2].split()) == 28
    path = os.path.join(HERE, "f26_ngram_repeats.npz")
    np.savez_compressed(path, texts=np.array([t for t, _ in cases]), params=np.array([p for _, p in cases], np.int64), outs=np.array(outs))
    assert os.path.getsize(path) < 100_000
    z = np.load(path, allow_pickle=False)
    assert [str(t) for t in z["texts"]] == [t for t, _ in cases] and [str(o) for o in z["outs"]] == outs
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

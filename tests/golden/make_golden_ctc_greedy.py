#!/usr/bin/env python3
"""Golden F22: the reference's own `ctc_greedy_decode` (src/utils/decoding.py:6-12, the preprocess_logits_for_metrics of CTC
pre-training) run on the CPU on crafted logits [4, 40, 37]:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ctc_greedy.py

Every value is bf16-representable, so an fp32 and a bf16 run of the product see the same numbers.  Inputs and outputs only.
Cases (each: logits, blank, pad, out):
    random    noise with planted runs of 1-5 frames (blank runs among them), blank 36, pad -100
    crafted   row 0 one constant value (every frame a tie over all classes -> id 0 once), row 1 all blank, row 2 no blank and no
              repeat (n = Tn), row 3 first frame blank, a token repeated across a blank (kept twice) and without one (merged), last
              frame non-blank; blank 36, pad -100
    inf       row 0 +inf on two neighbouring frames (the second frame twice: the lower column wins), row 1 all -inf (-> id 0 once),
              rows 2-3 as `random`; blank 36, pad 5
    blank50   the logits of `random` with blank 50, an id that never occurs: nothing is dropped; pad -100
    pad5      the logits of `random` with blank 36, pad 5 (a pad id that is also a class)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"
sys.path.insert(0, REF)
import numpy as np
import torch

from utils.decoding import ctc_greedy_decode  # noqa: E402  (the reference's function)

B, TN, V1, BLANK = 4, 40, 37, 36


def noise(g):
    return (torch.rand(B, TN, V1, generator=g) * 2.0 - 1.0).bfloat16().float()


def plant(x, b, path, height=4.0):
    for t, c in enumerate(path):
        x[b, t, c] = height


def random_runs(g):
    x = noise(g)
    for b in range(B):
        path = []
        while len(path) < TN:
            c = int(torch.randint(0, V1, (1,), generator=g))
            c = BLANK if int(torch.randint(0, 3, (1,), generator=g)) == 0 else c
            path += [c] * int(torch.randint(1, 6, (1,), generator=g))
        plant(x, b, path[:TN])
    return x


def main():
    g = torch.Generator().manual_seed(22)
    cases = {}
    rnd = random_runs(g)
    cases["random"] = (rnd, BLANK, -100)
    x = noise(g)
    x[0] = 0.75
    plant(x, 1, [BLANK] * TN)
    plant(x, 2, [(3 * t + 1) % 36 for t in range(TN)])
    plant(x, 3, [BLANK, 5, 5, BLANK, 5, 5, 5, 9, BLANK, BLANK, 9] + [(t % 7) + 10 for t in range(TN - 12)] + [2])
    cases["crafted"] = (x, BLANK, -100)
    x = random_runs(g)
    x[0, 10, 7] = float("inf")
    x[0, 11, 7] = float("inf")
    x[0, 11, 20] = float("inf")
    x[1] = float("-inf")
    cases["inf"] = (x, BLANK, 5)
    cases["blank50"] = (rnd, 50, -100)
    cases["pad5"] = (rnd, BLANK, 5)
    arrs = {}
    for name, (x, blank, pad) in cases.items():
        assert torch.equal(x, x.bfloat16().float())
        out = ctc_greedy_decode(x.clone(), blank, pad)
        arrs[f"{name}.logits"] = x.numpy()
        arrs[f"{name}.blank"] = np.array(blank, dtype=np.int64)
        arrs[f"{name}.pad"] = np.array(pad, dtype=np.int64)
        arrs[f"{name}.out"] = out.numpy().astype(np.int64)
        print(name, "blank", blank, "pad", pad, "lengths", [(row != pad).sum().item() for row in out], "row 3", out[3].tolist())
    arrs["_versions"] = np.array(f"torch {torch.__version__}")
    np.savez_compressed(os.path.join(HERE, "f22_ctc_greedy.npz"), **arrs)


if __name__ == "__main__":
    main()

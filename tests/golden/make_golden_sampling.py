#!/usr/bin/env python3
"""Golden F28: transformers' own sampling warpers -- TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
MinPLogitsWarper with min_tokens_to_keep = 1, the chain HF's generate builds for do_sample=True and the rungs of Whisper's temperature
fallback decode through -- on CPU, fp32:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling.py

Inputs: rows of DISTINCT fp32 scores (a shuffled grid of spacing 2^-8 times a scale, so that no tie class exists: the one stated
difference between the library's top_p rule and HF's sort cannot show), V = 50 with 6 rows and V = 1000 with 8 rows, one -inf planted per
row.  Per case the fixture holds the inputs, the options and HF's warped scores."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np
import torch

from tests.sampling_ref import via_transformers

# (temperature, top_k, top_p, min_p)
CASES = [(1.0, 0, 1.0, 0.0), (0.7, 5, 1.0, 0.0), (1.3, 50, 1.0, 0.0), (0.2, 0, 0.9, 0.0), (1.0, 0, 0.5, 0.0), (0.7, 0, 0.99, 0.0),
         (1.0, 0, 1e-6, 0.0), (0.7, 0, 1.0, 0.01), (1.3, 0, 1.0, 0.3), (1.0, 50, 0.9, 0.0), (0.7, 50, 0.5, 0.01), (1.3, 20, 0.99, 0.3)]
SHAPES = [(6, 50), (8, 1000)]


def make_scores(rows, V, seed):
    """Distinct values per row: a permutation of a 2^-8 grid around zero, scaled by 3 sigma-ish steps; one -inf per row."""
    g = torch.Generator().manual_seed(seed)
    out = np.empty((rows, V), np.float32)
    for r in range(rows):
        grid = (torch.randperm(4 * V, generator=g)[:V].double() - 2 * V) * (2.0 ** -8) * (24.0 * 256 / (4 * V))
        out[r] = grid.float().numpy()
        out[r, (7 * r + 3) % V] = -np.inf
    return out


def main():
    arrs = {}
    for rows, V in SHAPES:
        x = make_scores(rows, V, 2800 + V)
        assert all(len(set(row[np.isfinite(row)].tolist())) == V - 1 for row in x)
        arrs[f"V{V}.scores"] = x
        for i, (t, k, p, mp) in enumerate(CASES):
            arrs[f"V{V}.case{i}.opts"] = np.array([t, k, p, mp], np.float64)
            arrs[f"V{V}.case{i}.warped"] = via_transformers(x, t, k, p, mp)
    import transformers
    arrs["_versions"] = np.array(f"torch {torch.__version__} transformers {transformers.__version__}")
    np.savez_compressed(os.path.join(HERE, "f28_sampling_warpers.npz"), **arrs)
    print("wrote f28_sampling_warpers.npz:", len(arrs), "arrays")


if __name__ == "__main__":
    main()

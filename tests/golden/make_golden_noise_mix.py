#!/usr/bin/env python3
"""Golden F23: the reference's own `RandomBackgroundNoise` (src/data/augmentations.py:382-429) run on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noise_mix.py

The reference module imports torchaudio at the top and loads every noise file through `torchaudio.load`.  torchaudio is not a dependency
of this project, so a stand-in module goes into sys.modules before the import: `load(path) -> (tensor, 16000)` serves the clips of
tests/noise_mix_ref.py from memory, keyed by file name; `torchaudio.functional` is empty (nothing is resampled).  The class itself runs
unchanged.  `random.choice` and `random.randint` are wrapped while its `__call__` runs, so the fixture holds the clip, the offset and the
SNR as the reference drew them.  The noise directory is a temporary one with empty `<k>.wav` files; `noise_files_list` is then put into
index order (glob's order is the file system's).

Outputs only: both sides regenerate the inputs from integer hashes (tests/noise_mix_ref.py: f23_inputs).  Per case of F23_CASES:
    <name>.clip / .offset (-1: none drawn) / .snr_db     the logged draws
    <name>.out     the reference's fp32 output, in full up to 20 000 samples, else util.subsample(out, 4096)
The planner sequence (SEQ_*): 64 consecutive samples at prob 0.3 after torch.manual_seed(23); random.seed(23), gated as
src/data/local_datasets.py:205-206 gates them (that module needs lhotse and cannot be imported; its gate, `prob > 0 and torch.rand(1).item()
< prob`, is restated here), each gated sample run through the reference's __call__:
    seq.gate bool [64], seq.clip / seq.offset / seq.snr_db int64 [64] (-1 where nothing was drawn),
    seq.next_torch / seq.next_random     the next value of either generator after the sequence"""
import os
import pathlib
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src"
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import noise_mix_ref as R  # noqa: E402
from tests.util import hashed_uniform, subsample  # noqa: E402

SERVED = {}                                   # file name -> raw clip [C, n]
ta = types.ModuleType("torchaudio")
ta.load = lambda path: (SERVED[os.path.basename(path)].clone(), 16000)
ta.functional = types.ModuleType("torchaudio.functional")
sys.modules["torchaudio"], sys.modules["torchaudio.functional"] = ta, ta.functional

from data.augmentations import RandomBackgroundNoise  # noqa: E402  (the reference's class)


def make(clips):
    """The reference's object over `clips` (raw tensors), its file list in index order."""
    SERVED.clear()
    with tempfile.TemporaryDirectory() as d:
        for k, c in enumerate(clips):
            SERVED[f"{k}.wav"] = c
            open(os.path.join(d, f"{k}.wav"), "wb").close()
        aug = RandomBackgroundNoise(16000, d)
        assert len(aug.noise_files_list) == len(clips)
        aug.noise_files_list = [pathlib.Path(d) / f"{k}.wav" for k in range(len(clips))]
    return aug


def logged_call(aug, audio):
    """aug(audio) with the reference's draws logged: (out, clip index, offset or -1, snr_db)."""
    log = {"clip": -1, "ints": []}
    choice, randint = random.choice, random.randint

    def choice_(seq):
        got = choice(seq)
        log["clip"] = list(seq).index(got)
        return got

    def randint_(a, b):
        got = randint(a, b)
        log["ints"].append(got)
        return got

    random.choice, random.randint = choice_, randint_
    try:
        out = aug(audio)
    finally:
        random.choice, random.randint = choice, randint
    assert len(log["ints"]) in (1, 2)
    return out, log["clip"], (log["ints"][0] if len(log["ints"]) == 2 else -1), log["ints"][-1]


def main():
    arrs = {}
    for name, (ln, ch, clen, zero_head, seed) in R.F23_CASES.items():
        audio, raw = R.f23_inputs(name)
        aug = make([raw])
        random.seed(seed)
        out, clip, off, db = logged_call(aug, audio.clone())
        out = out.reshape(-1)                                  # ([1, len]: the reference's noise keeps its channel dimension)
        assert out.dtype == torch.float32 and out.numel() == ln and bool(torch.isfinite(out).all())
        arrs[f"{name}.clip"], arrs[f"{name}.offset"], arrs[f"{name}.snr_db"] = (np.array(v, dtype=np.int64) for v in (clip, off, db))
        arrs[f"{name}.out"] = (out if ln <= R.FULL_OUT_MAX else subsample(out, 4096)).numpy()
        o64 = R.mix_restatement64(audio, R.prepare_clip(raw), max(off, 0), db)
        e = float((out.double() - o64).abs().max())
        print(f"{name:12s} len {ln:7d} clip {clen:7d} offset {off:7d} snr_db {db:2d}   e_ref {e:.3e} = {e / float(o64.abs().max()):.2e} max|o|")
    # the planner sequence
    clips = [hashed_uniform(f"f23.seq.clip{k}", (1, n)) * R.NOISE_AMP for k, n in enumerate(R.SEQ_CLIP_LENS)]
    aug = make(clips)
    lengths = R.seq_lengths()
    gate, clip, off, db = (np.full(R.SEQ_N, -1, dtype=np.int64) for _ in range(4))
    torch.manual_seed(R.SEQ_SEED)
    random.seed(R.SEQ_SEED)
    for k, ln in enumerate(lengths):
        gate[k] = int(R.SEQ_PROB > 0.0 and torch.rand(1).item() < R.SEQ_PROB)          # local_datasets.py:205
        if gate[k]:
            _, clip[k], off[k], db[k] = logged_call(aug, torch.full((ln,), 0.1))
    arrs["seq.gate"], arrs["seq.clip"], arrs["seq.offset"], arrs["seq.snr_db"] = gate.astype(np.bool_), clip, off, db
    arrs["seq.next_torch"] = torch.rand(1).numpy()
    arrs["seq.next_random"] = np.array(random.random(), dtype=np.float64)
    print("sequence: gated", int(gate.sum()), "of", R.SEQ_N, " offsets drawn", int((off >= 0).sum()), " clips", sorted(set(clip[gate == 1].tolist())))
    arrs["_versions"] = np.array(f"torch {torch.__version__}")
    np.savez_compressed(os.path.join(HERE, "f23_noise_mix.npz"), **arrs)
    print("bytes", os.path.getsize(os.path.join(HERE, "f23_noise_mix.npz")))


if __name__ == "__main__":
    main()

"""Numpy restatement of what ts-asr-whisper_amd/enrollment_mix.py computes on the device -- the sequential fp32 sum of shifted clips, and
the STNO mask of a mixture from its tracks' shifted and cut supervision intervals (through the dense masks of tests/diar_front_end_ref.py)
-- the description of the bank behind golden F25 (tests/golden/make_golden_enrollment_mix.py, which the reference's own
generate_enrollment_mixture produced), and a small deterministic bank for the GPU tests."""
import os

import numpy as np
import torch

from tests import diar_front_end_ref as D
from tests.util import hashed_uniform

SR = 16000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f25_enrollment_mix.npz")

# ---------------------------------------------------------------------------------------------------------------- the bank of F25
# (speakers, recording id, cut.start [s], cut.duration [s], supervisions in seconds relative to the clip or None = the whole clip)
F25_CLIPS = [
    (("spkA",), "rec01", 0.0, 7.31, None),
    (("spkA",), "rec02", 3.5, 12.07, None),
    (("spkA",), "rec03", 0.0, 29.5, None),
    (("spkA",), "rec04", 0.0, 31.0, None),                                  # longer than max_enrollment_len: never the target's clip
    (("spkB",), "rec01", 1.25, 9.6, None),
    (("spkB",), "rec05", 0.0, 21.4, None),
    (("spkC",), "rec06", 0.0, 18.75, None),
    (("spkC",), "rec02", 6.0, 4.2, None),
    (("spkD",), "rec07", 0.0, 24.9, None),
    (("spkD",), "rec08", 2.0, 15.3, None),
    (("spkA", "spkE"), "rec09", 0.0, 10.0, (("spkA", 0.0, 4.0), ("spkE", 3.0, 10.0), ("spkA", 8.5, 9.5))),
    (("spkE",), "rec10", 12.0, 16.5, None),                                 # start + duration = 28.5: the clamp bites from offset 1.5 on
    (("spkF",), "rec11", 20.0, 15.0, None),                                 # start + duration = 35: as a target its clamped offset is negative
    (("spkB",), "rec12", 0.0, 26.0, None),
]


def f25_description():
    """The bank as golden F25 stores it: durations, starts, speakers ('+'-joined, sorted), recording ids."""
    return {"bank.durations": np.array([c[3] for c in F25_CLIPS], dtype=np.float64),
            "bank.starts": np.array([c[2] for c in F25_CLIPS], dtype=np.float64),
            "bank.speakers": np.array(["+".join(sorted(c[0])) for c in F25_CLIPS]),
            "bank.recording_ids": np.array([c[1] for c in F25_CLIPS])}


def f25_lens():
    return [round(c[3] * SR) for c in F25_CLIPS]


def f25_supervisions():
    return [None if c[4] is None else [(s, round(a * SR), round(b * SR)) for s, a, b in c[4]] for c in F25_CLIPS]


def f25_bank(enrollment_mix, device="cpu", data=None):
    """The F25 bank as an EnrollmentBank (silent audio unless `data` is given: the planner and the masks never read it)."""
    lens = f25_lens()
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    if data is None:
        data = torch.zeros(sum(lens), dtype=torch.float32)
    return enrollment_mix.EnrollmentBank(data.to(device), starts, lens, [list(c[0]) for c in F25_CLIPS], [c[1] for c in F25_CLIPS],
                                         cut_start=[c[2] for c in F25_CLIPS], durations=[c[3] for c in F25_CLIPS],
                                         supervisions=f25_supervisions())


def load_f25():
    return np.load(GOLDEN, allow_pickle=False)


def f25_case_names(z):
    return [str(n) for n in z["cases"]]


def f25_options(z, name):
    g, n_other, lo, hi, max_len, p = (float(x) for x in z[f"{name}.options"])
    return dict(greedy_sample=bool(g), num_other_speakers=int(n_other), min_overlap_ratio=lo, max_overlap_ratio=hi, max_enrollment_len=max_len,
                randomly_shift_target_offset_p=p)


def f25_rows(z, name):
    """(targets, skip lists) of a case: one entry per row."""
    targets = [str(t) for t in z[f"{name}.targets"]]
    skips = [[s for s in str(x).split("|") if s] for x in z[f"{name}.skip_ids"]]
    return targets, skips


def tracks_in_samples(rows, clips, off_s, len_s, max_len=30.0):
    """The reference's tracks (seconds) -> int32 [n, 4] as the planner converts them: Python's round of seconds * 16000, the length capped
    at round(max_len * 16000) - offset, a track of no sample left out."""
    out = []
    for r, c, o, d in zip(rows, clips, off_s, len_s):
        o_i = round(float(o) * SR)
        ln = min(round(float(d) * SR), round(max_len * SR) - o_i)
        if ln >= 1:
            out.append((int(r), int(c), o_i, ln))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------------------- restatements
def mix(data, starts, tracks, B, n):
    """fp32 [B, n]: per sample the row's covering tracks added one by one in plan order (numpy's fp32 add rounds to nearest, as
    __fadd_rn); the first covering track's value is taken as it is; 0 where none covers."""
    data = np.asarray(data, dtype=np.float32)
    out = np.zeros((B, n), dtype=np.float32)
    covered = np.zeros((B, n), dtype=bool)
    for row, clip, off, ln in np.asarray(tracks).reshape(-1, 4).tolist():
        x = data[starts[clip]:starts[clip] + ln]
        o, c = out[row, off:off + ln], covered[row, off:off + ln]
        o[...] = np.where(c, (o + x).astype(np.float32), x)
        c[...] = True
    return out


def intervals_of_row(supervisions, tracks, row):
    """speaker -> [(start, end)] of the mixture: each track's supervision intervals clipped to [0, len) and shifted by its offset."""
    out = {}
    for r, clip, off, ln in np.asarray(tracks).reshape(-1, 4).tolist():
        if r != row:
            continue
        for spk, a, b in supervisions[clip]:
            out.setdefault(spk, [])
            a, b = max(a, 0), min(b, ln)
            if a < b:
                out[spk].append((off + a, off + b))
    return out


def stno(supervisions, tracks, row, target, mix_len):
    """fp32 [4, 1500]: dense per-sample masks of the mixture's sorted speakers over mix_len samples -> per-frame counts -> the
    reference's STNO arithmetic (tests/diar_front_end_ref.py, pinned to the reference by golden F24).  target "-1": the unknown speaker."""
    iv = intervals_of_row(supervisions, tracks, row)
    names = sorted(iv)
    cnt, _ = D.frame_counts(D.dense_masks([iv[s] for s in names], int(mix_len)))
    return D.stno(cnt, -1 if target == "-1" else names.index(target))


# ---------------------------------------------------------------------------------------------------------------- a small bank
SMALL_LENS = (1024, 9, 257, 1, 300, 2, 255, 3, 256, 5, 4, 7, 6, 8, 640, 480000)


def small_clips(lens=SMALL_LENS, pad=(1, 2, 3, 4)):
    """Clips of the given lengths with hashed values in [-1, 1); `pad` cycles through the gaps put before each clip, so that clip starts
    fall on every residue modulo 4.  -> (flat fp32 data with NaN in the gaps and 8 NaN at either end, starts, lens)."""
    parts, starts, pos = [np.full(8, np.nan, dtype=np.float32)], [], 8
    for k, ln in enumerate(lens):
        g = pad[k % len(pad)]
        parts.append(np.full(g, np.nan, dtype=np.float32))
        pos += g
        starts.append(pos)
        parts.append(hashed_uniform(f"enrollment_mix.clip{k}", (ln,)).numpy())
        pos += ln
    parts.append(np.full(8, np.nan, dtype=np.float32))
    return np.concatenate(parts), starts, list(lens)


def small_bank(enrollment_mix, device="cuda", lens=SMALL_LENS):
    """(EnrollmentBank, data as numpy, starts): one speaker per clip ("s00", "s01", ...), NaN guard bands around every clip."""
    data, starts, lens = small_clips(lens)
    bank = enrollment_mix.EnrollmentBank(torch.from_numpy(data).to(device), starts, lens, [f"s{k:02d}" for k in range(len(lens))],
                                         [f"r{k:02d}" for k in range(len(lens))])
    return bank, data, starts

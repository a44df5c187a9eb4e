"""Integer restatement, in numpy on DENSE per-sample masks, of what ts-asr-whisper_amd/diar_front_end.py computes from interval tables --
so only for small recordings -- and the cases of golden F24 (tests/golden/make_golden_diar_front_end.py), which the reference's own
functions produced.  tests/test_host_diar_front_end.py pins this file to F24; the GPU tests then compare the kernels with it bit for bit.

A case is (n_samples, intervals): `intervals` a list, one entry per speaker in sorted-name order, of half-open sample intervals."""
import os

import numpy as np

FRAME, BIN, WINDOW = 320, 1600, 300
N30, T30 = 480000, 1500
N_A = 2 * N30 + 1601            # 60.1 s: no multiple of 320 (961601 = 3005 * 320 + 1), of 1600 or of 480000
N_B = 70 * 16000 + 7            # 70 s + 7 samples
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f24_diar_front_end.npz")
STNO_FULL_MAX_T = 3000          # F24 stores every STNO frame up to this T_total, else frames [::STNO_STRIDE] plus the last 40
STNO_STRIDE = 7


def t_total(n_samples):
    return -(-n_samples // N30) * T30


def names(S):
    """Speaker names whose sorted order is their index order."""
    return [f"spk{s:02d}" for s in range(S)]


def as_dict(intervals):
    return {n: list(iv) for n, iv in zip(names(len(intervals)), intervals)}


def dense_masks(intervals, n_samples):
    """bool [S, n_samples]: the union of each speaker's intervals, clipped to the recording (what lhotse's speakers_audio_mask rasterises)."""
    m = np.zeros((len(intervals), n_samples), dtype=bool)
    for s, iv in enumerate(intervals):
        for a, b in iv:
            a, b = max(0, int(a)), min(n_samples, int(b))
            if a < b:
                m[s, a:b] = True
    return m


def frame_counts(dense):
    """(cnt, excl) int32 [S, T_total]: per 320-sample frame the samples on which a speaker is active / the only one active."""
    S, n = dense.shape
    T = t_total(n)
    solo = dense & (dense.sum(axis=0, dtype=np.int32) == 1)[None]
    out = []
    for m in (dense, solo):
        p = np.zeros((S, T * FRAME), dtype=bool)
        p[:, :n] = m
        out.append(p.reshape(S, T, FRAME).sum(axis=-1, dtype=np.int32))
    return out[0], out[1]


def stno(cnt, target):
    """fp32 [4, T] (S, T, N, O) from the counts with the reference's numpy expressions (pooled activity = count / 320 in fp32;
    src/data/local_datasets.py:176-194); target -1 = its appended zero row."""
    m = cnt.astype(np.float32) / np.float32(FRAME)
    if target == -1:
        m = np.pad(m, ((0, 1), (0, 0)), mode="constant")
    others = np.ones(m.shape[0], dtype=bool)
    others[target] = False
    sil = (1 - m).prod(axis=0)
    anyone_else = (1 - m[others]).prod(axis=0)
    tgt = m[target] * anyone_else
    non = (1 - m[target]) * (1 - anyone_else)
    ovl = m[target] - tgt
    return np.stack([sil, tgt, non, ovl], axis=0).astype(np.float32)


def window_sums(frames_row, n_samples):
    """int64 [n_windows]: samples of `frames_row` (one speaker's per-frame counts) in every 300-bin window of full bins; one entry, the
    total, when the recording has fewer than 300 bins."""
    nb = n_samples // BIN
    bins = frames_row[:5 * nb].astype(np.int64).reshape(nb, 5).sum(axis=1)
    if nb < WINDOW:
        return np.array([bins.sum()], dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(bins)])
    return P[WINDOW:] - P[:-WINDOW]


def enrollment(cnt, excl, target, n_samples):
    """(start, count, fallback, weights): the FIRST window of maximal exact solo count; from cnt when the target is never alone."""
    for fb, src in enumerate((excl, cnt)):
        w = window_sums(src[target], n_samples)
        if w.max() > 0 or fb == 1:
            return int(np.argmax(w)), int(w.max()), fb, w.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- case builders
def random_intervals(rng, S, n_samples, mean_on=3.0, mean_off=4.0, empty=()):
    """Per speaker alternating talk / pause stretches with exponential lengths (seconds), starting anywhere, ending anywhere."""
    out = []
    for s in range(S):
        iv, t = [], int(rng.exponential(mean_off) * 16000 * rng.random())
        while t < n_samples and s not in empty:
            d = 1 + int(rng.exponential(mean_on) * 16000)
            iv.append((t, min(t + d, n_samples)))
            t += d + 1 + int(rng.exponential(mean_off) * 16000)
        out.append(iv)
    return out


def dominant_stretch(rng, S, n_samples, p, head, tail, target=0):
    """A recording in which `target` has ONE best window: it talks alone on [1600 p + (1600 - head), 1600 (p + 300) + tail), a stretch that fills
    the bins p + 1 .. p + 299 and `head` / `tail` samples of the bins p and p + 300 (head != tail: the window at p or at p + 1 wins by
    |head - tail| samples), plus short turns elsewhere; the other speakers talk only outside that stretch."""
    a, b = BIN * p + (BIN - head), BIN * (p + WINDOW) + tail
    assert 0 <= a and b <= n_samples and head != tail and 0 < head <= BIN and 0 <= tail < BIN
    out = []
    for s in range(S):
        iv = [(x, y) for x, y in random_intervals(rng, 1, n_samples, 1.0, 6.0)[0] if y <= a - 16000 or x >= b + 16000]
        if s == target:
            iv.append((a, b))
        out.append(sorted(iv))
    return out


def f24_cases():
    """name -> (n_samples, intervals, targets for STNO, targets for the enrollment search)."""
    rng = np.random.default_rng(24)
    c = {}
    c["s1"] = (N_B, random_intervals(rng, 1, N_B), [0, -1], [0])
    c["s2"] = (N_A, random_intervals(rng, 2, N_A), [0, 1, -1], [0, 1])
    c["s3"] = (N_B, random_intervals(rng, 3, N_B), [0, 1, 2, -1], [0, 1, 2])
    c["s4"] = (N_A, random_intervals(rng, 4, N_A, 4.0, 3.0), [0, 3, -1], [0, 1, 2, 3])
    c["s9"] = (N_B, random_intervals(rng, 9, N_B, 2.0, 9.0), [0, 4, 8, -1], [0, 4, 8])
    c["s3_empty"] = (N_A, random_intervals(rng, 3, N_A, empty=(1,)), [0, 1, 2], [0, 2])           # speaker 1 never talks
    iv = random_intervals(rng, 2, N_B)
    iv[0] = sorted(iv[0] + [(a + (b - a) // 3, b + 9000) for a, b in iv[0][::2]] + [iv[0][1]])    # overlapping, nested and duplicate turns
    c["s2_selfovl"] = (N_B, iv, [0, 1], [0, 1])
    iv = random_intervals(rng, 3, N_A)
    iv[0] = [(a + 777, b - 333) for a, b in iv[1][::2] if b - a > 4000]                            # speaker 0 only ever talks inside speaker 1's turns
    c["never_alone"] = (N_A, iv, [0], [0, 1])
    # one best window, by construction (the generator checks: runner-up lower by at least one sample)
    for j, (n, S, p, head, tail, tg) in enumerate(((N_A, 2, 37, 900, 500, 0), (N_A, 3, 120, 500, 900, 1), (N_B, 1, 0, 1600, 1, 0),
                                                   (N_B, 4, 399, 1, 0, 3), (240 * 16000 + 801, 2, 1500, 1599, 1598, 0),
                                                   (N_A, 9, 299, 800, 801, 8), (N_B, 2, 200, 1200, 3, 1))):
        c[f"uniq{j}"] = (n, dominant_stretch(rng, S, n, p, head, tail, tg), [tg], [tg])
    # plateaus: 40 s alone (every window inside it holds 480000 samples), and a lone 10 s turn (every window that holds it whole ties)
    c["tie_long"] = (N_A, [[(1600 * 50 + 123, 1600 * 50 + 123 + 40 * 16000)], [(900000, 930000)]], [0], [0, 1])
    c["tie_short"] = (N_B, [[(500000, 660000)], [(100, 4000), (700000, 800000)]], [0], [0, 1])
    c["tie_two"] = (N_A, [[(1600 * 10, 1600 * 40), (1600 * 400, 1600 * 430)]], [0], [0])           # two equal turns 39 s apart: never in one window
    return c


DRAW_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
DRAW_CASES = ("s2", "s3", "s9", "uniq4")          # non-greedy draws: for every enrollment target of these cases, every seed


def stno_pick(T):
    """The frames of a [4, T] mask that F24 stores."""
    if T <= STNO_FULL_MAX_T:
        return np.arange(T)
    return np.unique(np.concatenate([np.arange(0, T, STNO_STRIDE), np.arange(T - 40, T)]))


def load_f24():
    return np.load(GOLDEN, allow_pickle=False)


def f24_intervals(z, name):
    """(n_samples, intervals) of a case as the fixture stores them: rows (speaker, start, end) and the speaker count."""
    rows, S = np.asarray(z[f"{name}.intervals"]), int(z[f"{name}.S"])
    return int(z[f"{name}.n_samples"]), [[(int(a), int(b)) for s, a, b in rows if s == k] for k in range(S)]

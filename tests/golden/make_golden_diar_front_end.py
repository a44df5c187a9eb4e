#!/usr/bin/env python3
"""Golden F24: the reference's STNO builder and self-enrollment search (src/data/local_datasets.py:162-292) run on the CPU on dense masks
rasterised from the intervals of tests/diar_front_end_ref.py: f24_cases:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_diar_front_end.py

The reference module imports lhotse, torchaudio, omegaconf ... at module scope; none is installed, so placeholder modules are registered
first, as make_golden.py: f1_stno does (and the reference's parent directory goes on the path for `from src.utils...`).  What runs is the
reference's own code, unchanged, on stand-ins for the two lhotse objects it touches:
  * `get_stno_mask(self, cut, speaker_id)` whole -- the padding, the fp32 pooling by 320, the unknown speaker's zero row and the static
    `_create_stno_masks` -- with `self` carrying the feature extractor's two numbers and the subsample factor, `cut.speakers_audio_mask`
    returning the dense mask, and the module's `CutSet` name bound to a stand-in whose `from_cuts([cut]).speakers` lists the speakers;
  * `select_random_internal_enrollment(self, spk_id, cut, greedy_sample)` whole -- the overlap masking, `downsample_mean`,
    `sample_enrollment_window`, the fallback -- with the real static methods on `self`; `sample_enrollment_window` is wrapped only to log
    what it returns (the method itself returns a cut, not the activity), and the module's `fastcopy` name is bound to `copy.copy`.
A speaker without any segment has a supervision of zero length in the stand-in cut, so that it keeps its place among the speakers.

Per case <name>:   .n_samples, .S, .intervals int64 [n, 3] = (speaker, start, end)
    .stno.<target>           fp32 [4, len(stno_pick(T_total))]: the reference's mask (transposed), at the frames ref.stno_pick names
    .enr.<target>            float64 [4] = (start bin, activity of the chosen window, fallback taken, activity of the first call)
    .draw.<target>           float64 [len(DRAW_SEEDS), 2] = (start, activity) of the non-greedy draw after np.random.seed(seed)
                             (DRAW_CASES only; none for a target that is never alone, where the reference raises)
    .exact.<target>          int64 [3] = (first exact maximum, its count, the number of windows that reach it): the integer restatement's
and `unique` / `tied`: the names "<case>.<target>" of the greedy searches with one exact maximum (runner-up lower by at least one sample) and with
several.  The generator refuses to write a fixture with fewer than 6 of the former or 3 of the latter, or one in which the reference's
window does not hold the maximal exact count."""
import copy
import importlib.abc
import importlib.machinery
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src"
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(REF))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests import diar_front_end_ref as R  # noqa: E402

ABSENT = ("lhotse", "torchaudio", "omegaconf", "wandb", "hydra", "peft", "meeteval", "jiwer")


class _Any(types.ModuleType):
    __path__ = []

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return type(k, (), {})


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in ABSENT:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Any(spec.name)

    def exec_module(self, module):
        pass


sys.meta_path.append(_Finder())
import data.local_datasets as LD  # noqa: E402  (the reference)

DS = LD.TS_ASR_DatasetSuperclass
ns = types.SimpleNamespace


class StandInCutSet:
    def __init__(self, cuts):
        self.speakers = [s.speaker for c in cuts for s in c.supervisions]

    @classmethod
    def from_cuts(cls, cuts):
        return cls(cuts)


LD.CutSet = StandInCutSet
LD.fastcopy = copy.copy


class StandInCut:
    sampling_rate = 16000

    def __init__(self, intervals, n_samples):
        self.dense = R.dense_masks(intervals, n_samples).astype(np.float32)
        self.names = R.names(len(intervals))
        self.supervisions = [ns(speaker=n, start=0.0, end=0.0) for n in self.names]
        self.start, self.duration = 0.0, n_samples / 16000

    end = property(lambda self: self.start + self.duration)

    def speakers_audio_mask(self, speaker_to_idx_map):
        assert [speaker_to_idx_map[n] for n in self.names] == list(range(len(self.names)))
        return self.dense.copy()


def main():
    arrs, unique, tied = {}, [], []
    log = []

    def logged(arr, window_size=30, greedy_sample=False, skew_param=5.0):
        got = DS.sample_enrollment_window(arr, window_size=window_size, greedy_sample=greedy_sample, skew_param=skew_param)
        log.append((int(got[0]), float(got[1])))
        return got

    me_stno = ns(feature_extractor=ns(n_samples=480000, hop_length=160), model_features_subsample_factor=2, _create_stno_masks=DS._create_stno_masks)
    me_enr = ns(get_cut_spks=DS.get_cut_spks, downsample_mean=DS.downsample_mean, sample_enrollment_window=logged)
    for name, (n, intervals, stno_targets, enr_targets) in R.f24_cases().items():
        cut = StandInCut(intervals, n)
        S = len(intervals)
        arrs[f"{name}.n_samples"], arrs[f"{name}.S"] = np.array(n, dtype=np.int64), np.array(S, dtype=np.int64)
        arrs[f"{name}.intervals"] = np.array([(s, a, b) for s, iv in enumerate(intervals) for a, b in iv], dtype=np.int64).reshape(-1, 3)
        cnt, excl = R.frame_counts(cut.dense.astype(bool))
        pick = R.stno_pick(R.t_total(n))
        for t in stno_targets:
            m = DS.get_stno_mask(me_stno, cut, "-1" if t == -1 else cut.names[t])
            assert m.dtype == np.float32 and m.shape == (R.t_total(n), 4), (m.dtype, m.shape)
            arrs[f"{name}.stno.{t}"] = np.ascontiguousarray(m.T[:, pick])
            assert np.array_equal(R.stno(cnt, t).view(np.int32), m.T.view(np.int32)), (name, t)          # the restatement, bit for bit
        for t in enr_targets:
            del log[:]
            new_cut = DS.select_random_internal_enrollment(me_enr, cut.names[t], cut, greedy_sample=True)
            assert len(log) in (1, 2) and new_cut.duration == 30 and new_cut.start == log[-1][0] / 10
            arrs[f"{name}.enr.{t}"] = np.array([log[-1][0], log[-1][1], len(log) - 1, log[0][1]], dtype=np.float64)
            start, count, fb, w = R.enrollment(cnt, excl, t, n)
            n_best = int((w == count).sum())
            arrs[f"{name}.exact.{t}"] = np.array([start, count, n_best], dtype=np.int64)
            assert fb == len(log) - 1, (name, t)
            assert int(w[log[-1][0]]) == count and abs(log[-1][1] - count / 1600) < 1e-9, (name, t, "the reference's window is not a best one")
            (unique if n_best == 1 else tied).append(f"{name}.{t}")
            if n_best == 1:
                assert start == log[-1][0] and np.sort(w)[-2] <= count - 1
            print(f"{name:12s} target {t}: reference start {log[-1][0]:5d} activity {log[-1][1]:.9f} fallback {fb}; exact first max {start:5d} "
                  f"count {count} ({n_best} best windows of {w.size})")
            if name in R.DRAW_CASES and fb == 1:                    # never alone: the reference's non-greedy branch raises before its fallback
                try:
                    DS.select_random_internal_enrollment(me_enr, cut.names[t], cut, greedy_sample=False)
                    raise AssertionError("expected the reference to raise")
                except ValueError as ex:
                    assert "No speaker activity" in str(ex)
            elif name in R.DRAW_CASES:
                draws = []
                for seed in R.DRAW_SEEDS:
                    del log[:]
                    np.random.seed(seed)
                    DS.select_random_internal_enrollment(me_enr, cut.names[t], cut, greedy_sample=False)
                    assert len(log) == 1
                    draws.append(log[0])
                arrs[f"{name}.draw.{t}"] = np.array(draws, dtype=np.float64)
    print("unique maximum:", unique, "\ntied:", tied)
    assert len(unique) >= 6 and len(tied) >= 3, (len(unique), len(tied))
    assert any(arrs[k][2] == 1 for k in arrs if ".enr." in k), "no case takes the fallback"
    arrs["unique"], arrs["tied"] = np.array(unique), np.array(tied)
    arrs["_versions"] = np.array(f"numpy {np.__version__}")
    path = os.path.join(HERE, "f24_diar_front_end.npz")
    np.savez_compressed(path, **arrs)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden F25: the reference's generate_enrollment_mixture (src/data/local_datasets.py:355-436, with sample_same_speaker_cut :334-353,
sample_offsets :305-332 and mix_two_recordings :294-303) run under fixed np.random / random seeds on the bank that
tests/enrollment_mix_ref.py: F25_CLIPS describes:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_enrollment_mix.py

The reference module imports lhotse, torchaudio, ... at module scope; none is installed, so placeholder modules are registered first, as
make_golden_diar_front_end.py does.  What runs is the reference's own code, whole and unchanged, on stand-ins for the lhotse objects it
touches: `MixTrack`, `MonoCut` and `MixedCut` only record their arguments; a cut is a namespace of its fields; the stand-in for a speaker's
`per_speaker_enrollments` entry has filter / __len__ / __iter__ / __getitem__, and its sample() is random.randrange over its cuts (what
lhotse's CutSet.sample() draws could not be pinned: lhotse is not installed).  `self` carries the two dicts the reference's constructor
builds (:81-92, with the reference's get_cut_spks) and the reference's own methods.  np.random.uniform / choice / rand / permutation,
random.sample, sample_offsets and mix_two_recordings are wrapped only to LOG what they return -- they draw what they would draw -- and the
log says which branches a case took.

A case is a sequence of rows under one pair of seeds and one set of options.  Per case <name>:
    .options     float64 [6] = (greedy_sample, num_other_speakers, min_overlap_ratio, max_overlap_ratio, max_enrollment_len, shift probability)
    .seeds       int64 [2] = (np.random.seed, random.seed)
    .targets     the rows' target speakers;  .skip_ids: per row the cleaned recording ids to skip, '|'-joined (the reference's re.sub)
    .tracks      float64 [n, 4] = (row, clip, offset [s], cut duration [s]) of the mixtures' final tracks, the target's first within a row
    .error       int64: 1 when the reference raised its "No valid enrollment cuts" ValueError on the last row (no tracks for that row)
    .next        float64 [2] = (np.random.rand(), random.random()) drawn right after the case: the state both generators were left in
    .branches    the branches the case took
and `cases` (the names), `bank.*` (durations, starts, speakers, recording ids of the clips).  The generator refuses to write the fixture
unless every branch of REQUIRED is reached by some case, and no case has a negative track offset."""
import importlib.abc
import importlib.machinery
import os
import random
import re
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

from tests import enrollment_mix_ref as R  # noqa: E402

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
LOG = []


class _Recorded:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class StandInMixTrack(_Recorded):
    pass


class StandInMonoCut(_Recorded):
    pass


class StandInMixedCut(_Recorded):
    pass


LD.MixTrack, LD.MonoCut, LD.MixedCut = StandInMixTrack, StandInMonoCut, StandInMixedCut


class StandInCutSet:
    def __init__(self, cuts):
        self.cuts = list(cuts)

    def filter(self, pred):
        return StandInCutSet([c for c in self.cuts if pred(c)])

    def __len__(self):
        return len(self.cuts)

    def __iter__(self):
        return iter(self.cuts)

    def __getitem__(self, i):
        return self.cuts[i]

    def sample(self):
        LOG.append(("cutset.sample", None))
        return self.cuts[random.randrange(len(self.cuts))]


def logged(name, fn):
    def wrapper(*a, **k):
        got = fn(*a, **k)
        LOG.append((name, got))
        return got
    return wrapper


for _n in ("uniform", "choice", "rand", "permutation"):
    setattr(np.random, _n, logged("np." + _n, getattr(np.random, _n)))
random.sample = logged("random.sample", random.sample)
_mix_two = DS.mix_two_recordings
DS.mix_two_recordings = staticmethod(logged("mix_two", _mix_two))
_sample_offsets = DS.sample_offsets


def sample_offsets_logged(*a, **k):
    LOG.append(("sample_offsets.enter", None))
    got = _sample_offsets(*a, **k)
    LOG.append(("sample_offsets.exit", got))
    return got


def build_self():
    cuts = []
    for k, (spk, rec, start, dur, sup) in enumerate(R.F25_CLIPS):
        sup = [(spk[0], 0.0, dur)] if sup is None else sup
        cuts.append(ns(id=f"clip{k}", recording_id=rec, start=start, duration=dur, channel=0, recording=None,
                       supervisions=[ns(speaker=s, start=a, duration=b - a) for s, a, b in sup]))
    per = {}
    for cut in cuts:                                                     # local_datasets.py:83-92
        for speaker in DS.get_cut_spks(cut):
            per.setdefault(speaker, []).append(cut)
    me = ns(enrollment_speakers=list(per.keys()), per_speaker_enrollments={s: StandInCutSet(c) for s, c in per.items()},
            sample_offsets=sample_offsets_logged)
    me.sample_same_speaker_cut = lambda *a, **k: DS.sample_same_speaker_cut(me, *a, **k)
    return me, cuts


def clip_of(cut):
    return int(cut.id[4:])


def branches_of_row(log, mix, same, opts):
    """The branches one call took, read off the log of what its draws returned."""
    greedy, n_other, lo, hi, max_len, p = opts
    names = [n for n, _ in log]
    b = {"greedy" if greedy else "nongreedy"}
    n_others = names.count("cutset.sample")
    b.add(f"others{n_others}")
    cand = [v for n, v in log if n == "random.sample"][0]
    if mix.speaker_id in cand:
        b.add("target_in_candidates")
    for n, v in log:
        if n == "mix_two":
            b.add("mix_two_a" if isinstance(v[0], int) else "mix_two_b")
    pre = 0.0
    if "sample_offsets.exit" in names:
        i0, i1 = names.index("sample_offsets.enter"), names.index("sample_offsets.exit")
        ret = log[i1][1]
        last = names[i1 - 1]                                            # (a uniform of mix_two_recordings is followed by its "mix_two" entry)
        assert names[i0 + 1] == "np.permutation" and names[i0:i1].count("mix_two") == n_others - 1
        if last == "np.uniform":
            b.add("exit1")
        else:
            assert last == "np.choice", names
            b.add("exit3" if isinstance(ret[0], int) else "exit2")
        pre = float(ret[0])
    if not greedy:
        assert "np.rand" in names
        if names[-1] == "np.uniform" and names[-2] == "np.rand":
            b.add("shift")
            pre = float(log[-1][1])
        else:
            assert names[-1] == "np.rand"
            b.add("noshift")
    if same.start + pre + same.duration > max_len:
        b.add("clamp")
        if same.start > 0:
            b.add("clamp_start")
        assert mix.tracks[0].offset == max_len - (same.start + same.duration)
    if any(isinstance(t.cut, StandInMonoCut) for t in mix.tracks):
        b.add("cut")
    if len(mix.tracks) < 1 + n_others:
        b.add("dropped")
    return b


REQUIRED = {"greedy", "nongreedy", "others0", "others1", "others2", "others3", "target_in_candidates", "mix_two_a", "mix_two_b", "exit1", "exit2",
            "exit3", "shift", "noshift", "clamp", "clamp_start", "cut", "dropped", "error_empty", "mixed_original", "several_rows"}


def run_case(me, cuts, rows, opts, seeds):
    greedy, n_other, lo, hi, max_len, p = opts
    np.random.seed(seeds[0])
    random.seed(seeds[1])
    tracks, branches, error, skips = [], set(), 0, []
    for r, (target, original) in enumerate(rows):
        if isinstance(original, StandInMixedCut):
            branches.add("mixed_original")
            skips.append("|".join(re.sub("_vp.*$", "", t.cut.recording_id) for t in original.tracks))
        else:
            skips.append(re.sub("_vp.*$", "", original.recording_id))
        del LOG[:]
        try:
            mix = DS.generate_enrollment_mixture(me, original, target, bool(greedy), max_enrollment_len=max_len, randomly_shift_target_offset_p=p,
                                                 num_other_speakers=int(n_other), min_overlap_ratio=lo, max_overlap_ratio=hi)
        except ValueError as ex:
            assert "No valid enrollment cuts" in str(ex) and r == len(rows) - 1
            branches.add("error_empty")
            error = 1
            break
        mix.speaker_id = target
        assert mix.id == f"enrollment_{target}" and target in DS.get_cut_spks(mix.tracks[0].cut)
        same = cuts[clip_of(mix.tracks[0].cut)]
        branches |= branches_of_row(list(LOG), mix, same, opts)
        for t in mix.tracks:
            assert t.cut.duration > 0 and t.cut.duration + t.offset <= max_len + 1e-9 and t.cut.start == cuts[clip_of(t.cut)].start
            tracks.append((r, clip_of(t.cut), float(t.offset), float(t.cut.duration)))
    if len(rows) > 1:
        branches.add("several_rows")
    nxt = (float(np.random.rand()), random.random())
    return dict(tracks=np.array(tracks, dtype=np.float64).reshape(-1, 4), branches=branches, error=error, next=nxt, skips=skips)


def main():
    me, cuts = build_self()
    plain = lambda rid: ns(recording_id=rid)                            # noqa: E731
    mixed = lambda *rids: StandInMixedCut(id="row", tracks=[ns(cut=ns(recording_id=r)) for r in rids])   # noqa: E731
    originals = {"spkA": [plain("rec01_vp2"), plain("sessrec02b_vp1_x"), mixed("rec03_vp1", "rec09")], "spkB": [plain("rec99"), mixed("rec05_vp1", "rec12")],
                 "spkC": [plain("rec01")], "spkD": [plain("rec08_vp4")], "spkE": [plain("rec09_vp1"), plain("rec77")]}
    configs = []
    for greedy in (0.0, 1.0):
        for n_other in (0.0, 1.0, 2.0, 3.0):
            for lo, hi in ((0.3, 1.0), (0.0, 0.2), (0.9, 1.0)):
                for p in (1.0, 0.5):
                    if greedy and p != 1.0:
                        continue
                    configs.append((greedy, n_other, lo, hi, 30.0, p))
    chosen, count = [], {b: 0 for b in REQUIRED}
    for ci, opts in enumerate(configs):
        for ti, (target, origs) in enumerate(sorted(originals.items())):
            for seed in range(6):
                if all(v >= 3 for v in count.values()) or len(chosen) >= 60:
                    break
                rows = [(target, origs[seed % len(origs)])]
                seeds = (1000 * ci + 10 * ti + seed, 7000 + 100 * ci + 10 * ti + seed)
                got = run_case(me, cuts, rows, opts, seeds)
                if any(count.get(b, 3) < 3 for b in got["branches"]):
                    for b in got["branches"] & REQUIRED:
                        count[b] += 1
                    chosen.append((rows, opts, seeds, got))
    # a search for the rare one: a track that starts at or behind 30 s and is dropped
    for seed in range(400):
        if count["dropped"] >= 2:
            break
        rows, opts, seeds = [("spkC", plain("rec02"))], (0.0, 3.0, 0.0, 0.2, 30.0, 1.0), (50000 + seed, 60000 + seed)
        got = run_case(me, cuts, rows, opts, seeds)
        if "dropped" in got["branches"]:
            for b in got["branches"] & REQUIRED:
                count[b] += 1
            chosen.append((rows, opts, seeds, got))
    # sequences of rows under one pair of seeds, and the two ways to the empty filter (every clip skipped; the only one left too long)
    extra = [([("spkA", plain("rec01_vp2")), ("spkB", mixed("rec05_vp1", "rec12")), ("spkE", plain("rec77")), ("spkD", plain("rec08_vp4")),
               ("spkC", plain("rec01")), ("spkA", mixed("rec03_vp1", "rec09"))], (0.0, 2.0, 0.3, 1.0, 30.0, 1.0), (2501, 2502)),
             ([("spkE", plain("rec09_vp1")), ("spkD", plain("x")), ("spkB", plain("rec99"))], (1.0, 3.0, 0.3, 1.0, 30.0, 1.0), (2503, 2504)),
             ([("spkA", plain("y")), ("spkC", mixed("rec06_vp1", "prerec02post_vp9"))], (0.0, 1.0, 0.3, 1.0, 30.0, 0.5), (2505, 2506)),
             ([("spkA", mixed("rec01", "rec02", "rec03", "rec09_vp3"))], (0.0, 2.0, 0.3, 1.0, 30.0, 1.0), (2507, 2508)),
             ([("spkD", plain("rec08"))], (0.0, 2.0, 0.3, 1.0, 20.0, 1.0), (2509, 2510))]          # max 20 s: clip 8 (24.9 s) is too long
    for rows, opts, seeds in extra:
        got = run_case(me, cuts, rows, opts, seeds)
        for b in got["branches"] & REQUIRED:
            count[b] += 1
        chosen.append((rows, opts, seeds, got))
    print("branch counts:", dict(sorted(count.items())))
    missing = sorted(b for b, v in count.items() if v == 0)
    assert not missing, f"branches not reached: {missing}"
    arrs = dict(R.f25_description())
    names = []
    for k, (rows, opts, seeds, got) in enumerate(chosen):
        name = f"c{k:02d}"
        names.append(name)
        assert not (got["tracks"][:, 2] < 0).any(), (name, "a negative offset")
        arrs[f"{name}.options"] = np.array(opts, dtype=np.float64)
        arrs[f"{name}.seeds"] = np.array(seeds, dtype=np.int64)
        arrs[f"{name}.targets"] = np.array([t for t, _ in rows])
        arrs[f"{name}.skip_ids"] = np.array(got["skips"] + [""] * (len(rows) - len(got["skips"])))
        arrs[f"{name}.tracks"] = got["tracks"]
        arrs[f"{name}.error"] = np.array(got["error"], dtype=np.int64)
        arrs[f"{name}.next"] = np.array(got["next"], dtype=np.float64)
        arrs[f"{name}.branches"] = np.array(sorted(got["branches"]))
        print(name, [t for t, _ in rows], opts, seeds, sorted(got["branches"]), got["tracks"].shape[0], "tracks")
    arrs["cases"] = np.array(names)
    arrs["required"] = np.array(sorted(REQUIRED))
    arrs["_versions"] = np.array(f"numpy {np.__version__} python {sys.version.split()[0]}")
    path = os.path.join(HERE, "f25_enrollment_mix.npz")
    np.savez_compressed(path, **arrs)
    print(len(names), "cases; bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()

"""CPU tests of the diarization front end's host side: the C-ABI entry points and their binding, their argument checks (the tables are
host arrays, checked before anything is launched), the sweep that builds the interval table against brute-force dense masks, the RTTM
parser, the non-greedy draw against the reference's draws, and the integer restatement the GPU tests use as their oracle, pinned to golden
F24 (which the reference's own functions produced).  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import diar_front_end_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, diar_front_end as D  # noqa: E402


@pytest.fixture(scope="module")
def f24():
    return R.load_f24()


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    c = _lib
    for name, sigs in (("dicow_diar_frame_counts", _lib._SIGS), ("dicow_stno_from_counts", _lib._SIGS), ("dicow_enrollment_windows", _lib._SIGS),
                       ("dicow_diar_table_ws_bytes", _lib._SIGS64), ("dicow_diar_targets_ws_bytes", _lib._SIGS64),
                       ("dicow_enrollment_windows_ws_bytes", _lib._SIGS64)):
        m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\);", stable, flags=re.M)
        assert m is not None, name
        args = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
        kinds = [c.c_vp if "*" in a else c.c_i64 if a.startswith("int64_t") else c.c_i for a in args]
        assert sigs[name] == kinds, (name, args)
        assert (m.group(1) == "int64_t") == (sigs is _lib._SIGS64)
        assert name in _lib.declared_symbols()
        assert getattr(_lib.lib(), name).restype is (c.c_i64 if sigs is _lib._SIGS64 else c.c_i)
    for macro, want in (("DICOW_DIAR_FRAME", 320), ("DICOW_DIAR_BIN", 1600), ("DICOW_DIAR_WINDOW", 300), ("DICOW_DIAR_MAX_SPEAKERS", 64)):
        m = re.search(r"^#define\s+" + macro + r"\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == want
    assert (_lib.DIAR_FRAME, _lib.DIAR_BIN, _lib.DIAR_WINDOW, _lib.DIAR_MAX_SPEAKERS) == (320, 1600, 300, 64) == (D.FRAME, D.BIN, D.WINDOW_BINS, D.MAX_SPEAKERS)
    assert _lib.lib().dicow_abi_version() == 7                            # additive: the version stays
    for name in ("SpeakerSegments", "stno_masks", "select_enrollment_windows", "draw_enrollment_window", "MeetingFrontEnd"):
        assert getattr(pkg, name) is getattr(D, name) and name in pkg.__all__


def _ptr(a):
    return a.ctypes.data


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    assert lib.dicow_diar_table_ws_bytes(0) == 8 and lib.dicow_diar_table_ws_bytes(10) == 21 * 8 and lib.dicow_diar_table_ws_bytes(-1) == -1
    assert lib.dicow_diar_targets_ws_bytes(0) == 0 and lib.dicow_diar_targets_ws_bytes(3) == 16 and lib.dicow_diar_targets_ws_bytes(-2) == -1
    assert lib.dicow_enrollment_windows_ws_bytes(R.N_A, 2) == 8 + 2 * (R.N_A // 1600 + 1) * 8
    assert lib.dicow_enrollment_windows_ws_bytes(-1, 2) == -1 and lib.dicow_enrollment_windows_ws_bytes(100, -1) == -1
    assert b"ws_bytes" in lib.dicow_last_error()
    p = 4096                                                              # device pointers: never dereferenced, every call below is refused
    n = 100000
    bounds, active = np.array([10, 500, 900, 4000], dtype=np.int64), np.array([1, 3, 2], dtype=np.uint64)
    ok = dict(b=_ptr(bounds), a=_ptr(active), E=3, S=2, n=n, cnt=p, excl=p, ws=p, wsb=7 * 8)
    unsorted, dup = np.array([10, 900, 500, 4000], dtype=np.int64), np.array([10, 500, 500, 4000], dtype=np.int64)
    neg, far = np.array([-1, 500, 900, 4000], dtype=np.int64), np.array([10, 500, 900, n + 1], dtype=np.int64)
    stray = np.array([1, 4, 2], dtype=np.uint64)                          # names speaker 2 of S = 2
    for bad in (dict(b=None), dict(a=None), dict(cnt=None), dict(excl=None), dict(ws=None), dict(E=-1), dict(S=0), dict(S=65), dict(n=-5),
                dict(wsb=7 * 8 - 1), dict(wsb=-8), dict(ws=p + 4), dict(b=_ptr(unsorted)), dict(b=_ptr(dup)), dict(b=_ptr(neg)),
                dict(b=_ptr(far)), dict(a=_ptr(stray))):
        a = dict(ok, **bad)
        assert lib.dicow_diar_frame_counts(a["b"], a["a"], a["E"], a["S"], a["n"], a["cnt"], a["excl"], a["ws"], a["wsb"], None) == -1, bad
        assert b"diar_frame_counts" in lib.dicow_last_error()
    tg, tg_hi, tg_lo = (np.array(v, dtype=np.int32) for v in ([0, -1, 1], [0, 2, 1], [0, -2, 1]))
    T = R.t_total(n)
    ok = dict(cnt=p, S=2, n=n, tg=_ptr(tg), k=3, out=p, ld=T, ws=p, wsb=16)
    for bad in (dict(cnt=None), dict(out=None), dict(ws=None), dict(tg=None), dict(k=-1), dict(S=0), dict(S=65), dict(n=-1), dict(ld=T - 1),
                dict(ld=-1), dict(wsb=15), dict(ws=p + 4), dict(tg=_ptr(tg_hi)), dict(tg=_ptr(tg_lo)), dict(k=1 << 16, wsb=1 << 30)):
        a = dict(ok, **bad)
        assert lib.dicow_stno_from_counts(a["cnt"], a["S"], a["n"], a["tg"], a["k"], a["out"], a["ld"], a["ws"], a["wsb"], None) == -1, bad
        assert b"stno_from_counts" in lib.dicow_last_error()
    tg, tg_unknown = np.array([0, 1, 1], dtype=np.int32), np.array([0, -1, 1], dtype=np.int32)
    need = lib.dicow_enrollment_windows_ws_bytes(n, 3)
    ok = dict(cnt=p, excl=p, S=2, n=n, tg=_ptr(tg), k=3, st=p, co=p, fb=p, w=None, ldw=0, ws=p, wsb=need)
    for bad in (dict(cnt=None), dict(excl=None), dict(st=None), dict(co=None), dict(fb=None), dict(ws=None), dict(tg=None), dict(k=-1),
                dict(S=0), dict(n=-1), dict(wsb=need - 1), dict(ws=p + 2), dict(tg=_ptr(tg_hi)), dict(tg=_ptr(tg_lo)), dict(tg=_ptr(tg_unknown)),
                dict(w=p, ldw=0), dict(w=p, ldw=-3), dict(n=500 * 1600, w=p, ldw=200, wsb=1 << 30)):
        a = dict(ok, **bad)
        rc = lib.dicow_enrollment_windows(a["cnt"], a["excl"], a["S"], a["n"], a["tg"], a["k"], a["st"], a["co"], a["fb"], a["w"], a["ldw"],
                                          a["ws"], a["wsb"], None)
        assert rc == -1, bad
        assert b"enrollment_windows" in lib.dicow_last_error()
    # nothing to do launches nothing and needs nothing
    assert lib.dicow_stno_from_counts(None, 2, n, None, 0, None, T, None, 0, None) == 0
    assert lib.dicow_enrollment_windows(None, None, 2, n, None, 0, None, None, None, None, 0, None, 0, None) == 0


def _dense_of_table(segs):
    """[S, n_samples] bool from the table alone."""
    m = np.zeros((segs.S, segs.n_samples), dtype=bool)
    for e in range(segs.E):
        for s in range(segs.S):
            if (int(segs.active[e]) >> s) & 1:
                m[s, segs.bounds[e]:segs.bounds[e + 1]] = True
    return m


def _check_table(intervals, n):
    segs = D.SpeakerSegments.from_samples(R.as_dict(intervals), n)
    assert segs.bounds.dtype == np.int64 and segs.active.dtype == np.uint64 and segs.bounds.shape == (segs.E + 1,)
    assert np.all(np.diff(segs.bounds) > 0) and segs.bounds[0] >= 0 and segs.bounds[-1] <= n
    assert segs.E <= max(2 * sum(len(v) for v in intervals) - 1, 0)
    assert np.array_equal(_dense_of_table(segs), R.dense_masks(intervals, n))
    return segs


def test_sweep_builds_the_table_of_brute_force_masks():
    rng = np.random.default_rng(7)
    for S, n in ((1, 5000), (2, 7001), (3, 9999), (9, 4000), (33, 3000), (64, 2500)):
        iv = [[tuple(sorted(rng.integers(-50, n + 50, 2).tolist())) for _ in range(rng.integers(0, 7))] for _ in range(S)]
        segs = _check_table(iv, n)
        if S == 64 and any(b > a and b > 0 and a < n for a, b in iv[63]):
            assert (segs.active >> np.uint64(63)).any()
    n = 3200
    adversarial = [[(0, 100), (100, 200), (200, 200), (150, 160), (150, 160), (3000, n), (3100, n + 77), (-5, 3)],      # touching, zero-length,
                   [(100, 200), (100, 200), (50, 400), (60, 70), (n, n + 5), (n - 1, n)],                               # nested, duplicate, at n
                   [],
                   [(0, n)]]
    segs = _check_table(adversarial, n)
    assert segs.bounds[0] == 0 and segs.bounds[-1] == n and segs.intervals["spk02"] == [] and (200, 200) not in segs.intervals["spk00"]
    empty = D.SpeakerSegments.from_samples({"a": [], "b": [(5, 5)]}, 1000)
    assert empty.E == 0 and empty.bounds.tolist() == [0] and empty.active.shape == (0,) and empty.S == 2
    assert (empty.T_total, empty.n_bins, empty.n_windows) == (1500, 0, 1)
    segs = D.SpeakerSegments.from_samples({"zed": [(0, 10)], "amy": [(5, 20)], "bob": []}, R.N_A)
    assert segs.speakers == ["amy", "bob", "zed"] and segs.bounds.tolist() == [0, 5, 10, 20] and segs.active.tolist() == [4, 5, 1]
    assert (segs.T_total, segs.n_bins, segs.n_windows) == (4500, 601, 302)
    assert segs.target_indices() == [0, 1, 2] and segs.target_indices(["zed", -1, "-1", 1]) == [2, -1, -1, 1]
    with pytest.raises(KeyError):
        segs.index_of("carl")
    with pytest.raises(ValueError):
        segs.index_of(3)
    with pytest.raises(ValueError, match="64"):
        D.SpeakerSegments.from_samples({f"s{k}": [] for k in range(65)}, 1000)
    with pytest.raises(ValueError):
        D.SpeakerSegments.from_samples({"a": [(0.5, 3)]}, 1000)
    with pytest.raises(ValueError):
        D.SpeakerSegments.from_samples({"a": [(0, 3)]}, 0)


def test_seconds_and_rttm(tmp_path):
    segs = D.SpeakerSegments.from_seconds({"b": [(0.5, 1.25), (2.00003, 2.5)], "a": [(1.0, 70.0)]}, 32000)
    assert segs.intervals == {"a": [(16000, 32000)], "b": [(8000, 20000)]}                # 2.00003 s rounds to sample 32000 = n_samples: dropped
    with pytest.raises(ValueError, match="16 kHz"):
        D.SpeakerSegments.from_seconds({"a": [(0, 1)]}, 8000, sampling_rate=8000)
    rttm = tmp_path / "m.rttm"
    rttm.write_text("SPEAKER rec1 1 0.50 1.25 <NA> <NA> spkB <NA> <NA>\n"
                    "SPKR-INFO rec1 1 <NA> <NA> <NA> unknown spkB <NA> <NA>\n"
                    "SPEAKER rec2 1 0.00 9.00 <NA> <NA> spkZ <NA> <NA>\n"
                    "\n"
                    "SPEAKER rec1 1 1.00 3.00 <NA> <NA> spkA <NA> <NA>\n"
                    "SPEAKER rec1 1 3.50 0.25 <NA> <NA> spkB <NA> <NA>\n")
    segs = D.SpeakerSegments.from_rttm(str(rttm), "rec1", n_samples=80000)
    assert segs.speakers == ["spkA", "spkB"] and segs.n_samples == 80000
    assert segs.intervals == {"spkA": [(16000, 64000)], "spkB": [(8000, 28000), (56000, 60000)]}
    assert D.SpeakerSegments.from_rttm(str(rttm), "rec1").n_samples == 64000             # default: the end of the last segment
    assert D.SpeakerSegments.from_rttm(str(rttm)).speakers == ["spkA", "spkB", "spkZ"]
    with pytest.raises(ValueError, match="no SPEAKER line"):
        D.SpeakerSegments.from_rttm(str(rttm), "rec9")


def test_restatement_is_pinned_to_the_reference_on_every_f24_case(f24):
    cases = R.f24_cases()
    assert {k.split(".")[0] for k in f24.files if k.endswith(".n_samples")} == set(cases)
    sizes, n_fallback = set(), 0
    for name, (n, intervals, stno_targets, enr_targets) in cases.items():
        n_z, iv_z = R.f24_intervals(f24, name)
        assert n_z == n and iv_z == [[(int(a), int(b)) for a, b in iv] for iv in intervals], name      # the fixture holds the builders' intervals
        sizes.add(len(intervals))
        cnt, excl = R.frame_counts(R.dense_masks(intervals, n))
        assert cnt.shape == (len(intervals), R.t_total(n)) and (excl <= cnt).all() and cnt.max() <= 320
        pick = R.stno_pick(R.t_total(n))
        for t in stno_targets:
            want = np.asarray(f24[f"{name}.stno.{t}"])
            assert want.dtype == np.float32 and np.array_equal(R.stno(cnt, t)[:, pick].view(np.int32), want.view(np.int32)), (name, t)
        for t in enr_targets:
            start, count, fb, w = R.enrollment(cnt, excl, t, n)
            ref_start, ref_act, ref_fb, _ = f24[f"{name}.enr.{t}"]
            assert fb == int(ref_fb), (name, t)
            n_fallback += fb
            assert abs(count / 1600 - ref_act) <= 1e-9, (name, t)          # the reference's 300 fp64 additions of values <= 1 err by ~1e-11;
            assert int(w[int(ref_start)]) == count, (name, t)              # one sample more or less is 6e-4: its window holds the exact maximum
            assert f24[f"{name}.exact.{t}"].tolist() == [start, count, int((w == count).sum())]
            if f"{name}.{t}" in f24["unique"].tolist():
                assert start == int(ref_start) and (np.sort(w)[-2] <= count - 1), (name, t)
            else:
                assert f"{name}.{t}" in f24["tied"].tolist() and start <= int(ref_start)
    assert {1, 2, 3, 4, 9} <= sizes and n_fallback >= 1
    assert len(f24["unique"]) >= 6 and len(f24["tied"]) >= 3
    assert any(n % 320 and n % 1600 and n % 480000 for n, _, _, _ in cases.values())
    assert any(int(f24[f"{k[:-2]}.enr.{k[-1]}"][0]) != int(f24[f"{k[:-2]}.exact.{k[-1]}"][0]) for k in f24["tied"].tolist())    # the deviation is real


def test_window_sums_under_thirty_seconds_are_the_total():
    n = 299 * 1600 + 1599
    cnt, excl = R.frame_counts(R.dense_masks([[(100, 5000), (470000, n)], [(4000, 6000)]], n))
    start, count, fb, w = R.enrollment(cnt, excl, 0, n)
    assert (start, fb, w.tolist()) == (0, 0, [count]) and count == 3900 + (299 * 1600 - 470000)      # full bins only: the last 1599 samples are trimmed


def test_draw_reproduces_the_reference_draws_of_f24(f24):
    seen = 0
    for name in R.DRAW_CASES:
        n, intervals, _, enr_targets = R.f24_cases()[name]
        cnt, excl = R.frame_counts(R.dense_masks(intervals, n))
        for t in enr_targets:
            start, count, fb, w = R.enrollment(cnt, excl, t, n)
            if fb:                                                         # never alone: the reference's non-greedy branch raises
                assert f"{name}.draw.{t}" not in f24.files
                with pytest.raises(ValueError, match="No speaker activity"):
                    D.draw_enrollment_window(R.window_sums(excl[t], n))
                continue
            want = np.asarray(f24[f"{name}.draw.{t}"])
            for seed, (ref_start, ref_act) in zip(R.DRAW_SEEDS, want):
                np.random.seed(seed)
                got = D.draw_enrollment_window(torch.from_numpy(w))
                assert got[0] == int(ref_start) and abs(got[1] / 1600 - ref_act) <= 1e-9, (name, t, seed)
                seen += 1
            assert len({int(s) for s, _ in want}) > 1 or name.startswith("uniq")
    assert seen >= 40
    rng = np.random.RandomState(3)                                         # an own generator is honoured
    a = D.draw_enrollment_window(w, rng=rng)
    np.random.seed(3)
    assert a == D.draw_enrollment_window(w) and isinstance(a[0], int)
    assert D.draw_enrollment_window(np.array([0, 0, 7, 0]), skew_param=1.0) == (2, 7)


def test_wrappers_refuse_the_cpu_and_the_unknown_speaker():
    segs = D.SpeakerSegments.from_samples({"a": [(0, 10)]}, 1000)
    with pytest.raises(_lib.DicowError, match="GPU"):
        D.stno_masks(segs, device="cpu")
    with pytest.raises(ValueError, match="unknown speaker"):
        D.select_enrollment_windows(segs, [-1])
    with pytest.raises(_lib.DicowError, match="GPU"):
        D.MeetingFrontEnd(80).prepare(torch.zeros(1000), segs)

"""CPU tests of the external enrollment mixtures' host side: the planner against the tracks the reference's own generate_enrollment_mixture
produced (golden F25), the two errors, the bank and its WAV loader, the C-ABI entry point's declaration, binding and host-side plan
validation, and the numpy restatement the GPU tests use as their oracle.  No GPU needed."""
import os
import random
import re
import wave

import numpy as np
import pytest
import torch

import amd_pkg
from tests import enrollment_mix_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, enrollment_mix as EM  # noqa: E402


@pytest.fixture(scope="module")
def f25():
    return R.load_f25(), R.f25_bank(EM, "cpu")


def test_entry_point_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_enrollment_mix\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["float* out", "int64_t ld_out", "int B", "int n", "const float* bank", "const int64_t* clip_start", "const int32_t* plan_dev",
                    "const int32_t* plan_host", "int n_tracks", "const int32_t* clip_len_host", "int n_clips", "void* stream"]
    m = re.search(r"^#define\s+DICOW_ENR_MIX_MAX_TRACKS\s+(\d+)", stable, flags=re.M)
    assert m and int(m.group(1)) == _lib.ENR_MIX_MAX_TRACKS == EM.MAX_TRACKS == 8
    c = _lib
    assert _lib._SIGS["dicow_enrollment_mix"] == [c.c_vp, c.c_i64, c.c_i, c.c_i, c.c_vp, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_i, c.c_vp]
    assert "dicow_enrollment_mix" in _lib.declared_symbols()
    lib = _lib.lib()
    assert lib.dicow_enrollment_mix.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("EnrollmentBank", "plan_enrollment_mixtures", "mix_enrollments", "enrollment_stno", "EnrollmentMixFrontEnd"):
        assert getattr(pkg, name) is getattr(EM, name) and name in pkg.__all__


def test_entry_point_validates_the_plan_on_the_host_before_any_launch():
    lib = _lib.lib()
    p = 4096                                                              # (never dereferenced: every call below is refused on the host)
    clip_len = np.array([100, 7, 2000], dtype=np.int32)

    def call(plan, B=4, n=1000, out=p, ld=1000, bank=p, cs=p, dev=p, n_clips=3, n_tracks=None, host=True):
        plan = np.ascontiguousarray(np.asarray(plan, dtype=np.int32).reshape(-1, 4))
        nt = plan.shape[0] if n_tracks is None else n_tracks
        return lib.dicow_enrollment_mix(out, ld, B, n, bank, cs, dev, plan.ctypes.data if host and plan.size else None, nt,
                                        clip_len.ctypes.data if host else None, n_clips, None)

    good = [(0, 0, 0, 100), (0, 1, 993, 7), (2, 2, 0, 1000), (3, 0, 900, 100)]
    bad_plans = {"row range": [(4, 0, 0, 10)], "negative row": [(-1, 0, 0, 10)], "rows decrease": [(2, 0, 0, 10), (1, 0, 0, 10)],
                 "clip range": [(0, 3, 0, 10)], "negative clip": [(0, -1, 0, 10)], "negative offset": [(0, 0, -1, 10)], "len 0": [(0, 0, 0, 0)],
                 "len beyond the clip": [(0, 1, 0, 8)], "ends behind n": [(0, 0, 901, 100)], "offset at n": [(0, 1, 1000, 1)],
                 "track cap": [(1, 1, 10 * k, 5) for k in range(9)]}
    for what, extra in bad_plans.items():
        assert call(extra) == -1, what
        assert b"enrollment_mix: track" in lib.dicow_last_error() or b"enrollment_mix: row" in lib.dicow_last_error(), what
        if extra[0][0] >= 2:                                               # and behind good tracks
            assert call(good[:2] + extra) == -1, what
    assert call([(1, 1, 10 * k, 5) for k in range(8)] + [(2, 1, 0, 5)], out=None) == -1            # the cap is per row: this plan passes ...
    assert b"null pointer" in lib.dicow_last_error()                                              # ... and only the missing output stops the call
    for what, kw in {"B": dict(B=-1), "B cap": dict(B=65536), "n": dict(n=-1), "ld short": dict(ld=996), "ld % 4": dict(ld=1002),
                     "n_tracks": dict(n_tracks=-1), "n_clips": dict(n_clips=-1), "no host plan": dict(host=False), "out": dict(out=None),
                     "out alignment": dict(out=p + 8), "bank": dict(bank=None), "bank alignment": dict(bank=p + 2), "clip_start": dict(cs=None),
                     "device plan": dict(dev=None)}.items():
        assert call(good, **kw) == -1, what
        assert b"enrollment_mix" in lib.dicow_last_error(), what
    # nothing to write: no launch, whatever the pointers
    assert call([], B=0, out=None, bank=None, cs=None, dev=None) == 0 and call([], n=0, ld=0, out=None, bank=None, cs=None, dev=None) == 0


def test_planner_reproduces_every_f25_case(f25):
    z, bank = f25
    for k, v in R.f25_description().items():
        assert np.array_equal(z[k], v), k
    assert [bank.durations, bank.cut_start, bank.recording_ids] == [list(z["bank.durations"]), list(z["bank.starts"]), list(z["bank.recording_ids"])]
    assert ["+".join(s) for s in bank.clip_speakers] == list(z["bank.speakers"])
    reached = set()
    for name in R.f25_case_names(z):
        opts, (targets, skips) = R.f25_options(z, name), R.f25_rows(z, name)
        want, err = np.asarray(z[f"{name}.tracks"]), int(z[f"{name}.error"])
        reached |= {str(b) for b in z[f"{name}.branches"]}
        np.random.seed(int(z[f"{name}.seeds"][0]))
        random.seed(int(z[f"{name}.seeds"][1]))
        n_ok = len(targets) - err
        tracks, off_s, len_s, mix_len = EM.plan_enrollment_mixtures(bank, targets[:n_ok], skips[:n_ok], **opts)
        if err:
            with pytest.raises(ValueError, match="No valid enrollment cuts found for speaker " + targets[-1]):
                EM.plan_enrollment_mixtures(bank, targets[-1:], skips[-1:], **opts)
        # nothing more was drawn from either generator than the reference drew, and nothing less
        assert (float(np.random.rand()), random.random()) == tuple(float(x) for x in z[f"{name}.next"]), name
        assert tracks.dtype == torch.int32 and mix_len.dtype == torch.int32 and off_s.dtype == np.float64 and len_s.dtype == np.float64
        assert tracks.shape == (want.shape[0], 4) and mix_len.shape == (n_ok,), name
        assert tracks[:, 0].tolist() == want[:, 0].tolist() and tracks[:, 1].tolist() == want[:, 1].tolist(), name      # rows and clips
        assert off_s.tolist() == want[:, 2].tolist(), name                                                                # float64, exactly
        assert len_s.tolist() == want[:, 3].tolist(), name                                                                # the cut durations
        assert np.array_equal(tracks.numpy(), R.tracks_in_samples(want[:, 0], want[:, 1], want[:, 2], want[:, 3], opts["max_enrollment_len"])), name
        n_max = round(opts["max_enrollment_len"] * 16000)
        for r in range(n_ok):
            mine = tracks[tracks[:, 0] == r]
            assert mine.shape[0] >= 1 and bank.clip_speakers[int(mine[0, 1])].count(targets[r]) == 1, name           # the target's track first
            assert int(mix_len[r]) == int((mine[:, 2] + mine[:, 3]).max()) <= n_max, name
        assert all(0 <= o and 1 <= ln <= bank.lens[c] for _, c, o, ln in tracks.tolist()), name
    assert reached >= {str(b) for b in z["required"]} and len(reached) >= 21


def test_planner_errors(f25):
    _, bank = f25
    np.random.seed(1)
    random.seed(1)
    with pytest.raises(ValueError, match="No valid enrollment cuts found for speaker spkC"):
        EM.plan_enrollment_mixtures(bank, ["spkC"], [["rec06", "xrec02y"]])                     # a substring match skips rec02 too
    with pytest.raises(ValueError, match="No valid enrollment cuts"):
        EM.plan_enrollment_mixtures(bank, ["spkD"], ["rec08"], max_enrollment_len=20.0)         # the other clip is too long
    # the reference's clamp: 30 - (20 + 15) s
    with pytest.raises(ValueError, match=r"negative offset -5\.0 s"):
        EM.plan_enrollment_mixtures(bank, ["spkF"], [[]], num_other_speakers=0)
    with pytest.raises(KeyError):
        EM.plan_enrollment_mixtures(bank, ["nobody"], [[]])
    with pytest.raises(ValueError, match="skip lists"):
        EM.plan_enrollment_mixtures(bank, ["spkA"], [])
    with pytest.raises(TypeError):
        EM.EnrollmentMixFrontEnd(bank, 80, no_such_option=1)
    with pytest.raises(ValueError, match="above 30 s"):
        EM.EnrollmentMixFrontEnd(bank, 80, max_enrollment_len=31.0)
    # no rows: no draws
    st_n, st_r = np.random.get_state()[1].copy(), random.getstate()
    tracks, off_s, len_s, mix_len = EM.plan_enrollment_mixtures(bank, [], [])
    assert tracks.shape == (0, 4) and off_s.shape == (0,) and len_s.shape == (0,) and mix_len.shape == (0,)
    assert np.array_equal(np.random.get_state()[1], st_n) and random.getstate() == st_r


def test_bank_layout_and_speaker_tables():
    g = torch.Generator().manual_seed(3)
    clips = [torch.rand(1001, generator=g) - 0.5, torch.rand(1, 777, generator=g) * 3 - 1, torch.rand(5, generator=g), torch.rand(64, generator=g)]
    sup = [None, [("zed", 0, 300), ("amy", 200, 777)], None, None]
    bank = EM.EnrollmentBank.from_tensors(clips, ["bob", ["zed", "amy"], "amy", "bob"], ["r1", "r2", "r3", "r1"], supervisions=sup, device="cpu")
    assert len(bank) == 4 and bank.lens == [1001, 777, 5, 64] and bank.starts == [0, 1001, 1778, 1783]
    assert bank.clip_start.dtype == torch.int64 and bank.clip_start.tolist() == bank.starts
    assert bank.clip_len.dtype == torch.int32 and bank.clip_len.tolist() == bank.lens
    assert bank.data.dtype == torch.float32 and bank.data.shape == (1847,)
    for c, s, n in zip(clips, bank.starts, bank.lens):
        assert torch.equal(bank.data[s:s + n], c.reshape(-1))              # as loaded: no normalisation
    assert bank.clip_speakers == [["bob"], ["amy", "zed"], ["amy"], ["bob"]]                        # sorted, as get_cut_spks
    assert bank.per_speaker == {"bob": [0, 3], "amy": [1, 2], "zed": [1]} and bank.speakers == ["bob", "amy", "zed"]
    assert bank.supervisions[0] == [("bob", 0, 1001)] and bank.supervisions[1] == sup[1]
    assert bank.durations == [n / 16000 for n in bank.lens] and bank.cut_start == [0.0] * 4 and bank.recording_ids == ["r1", "r2", "r3", "r1"]
    with pytest.raises(ValueError, match="supervision"):
        EM.EnrollmentBank.from_tensors(clips[:2], ["bob", ["zed", "amy"]], ["r1", "r2"], device="cpu")
    with pytest.raises(ValueError, match="mono"):
        EM.EnrollmentBank.from_tensors([torch.zeros(2, 100)], ["bob"], ["r1"], device="cpu")
    with pytest.raises(ValueError):
        EM.EnrollmentBank.from_tensors([], [], [], device="cpu")
    with pytest.raises(ValueError, match="duration"):
        EM.EnrollmentBank.from_tensors(clips[:1], ["bob"], ["r1"], durations=[1.0], device="cpu")    # 16000 samples claimed, 1001 held
    with pytest.raises(ValueError):
        EM.EnrollmentBank(torch.zeros(10), [0, 8], [8, 3], ["a", "b"], ["r", "r"])                    # a clip that ends behind the buffer


def _write_wav(path, pcm, rate=16000, width=2):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes() if width == 2 else bytes(width * pcm.size))


def test_bank_from_dir_reads_pcm16(tmp_path):
    rng = np.random.default_rng(4)
    pcm = {os.path.join("zed", "u2.wav"): rng.integers(-32768, 32768, (300, 1)), os.path.join("amy", "u1.wav"): rng.integers(-20000, 20000, (123, 1)),
           os.path.join("zed", "u1.wav"): rng.integers(-5, 6, (40, 1))}
    for name, x in pcm.items():
        _write_wav(str(tmp_path / "ok" / name), x)
    bank = EM.EnrollmentBank.from_dir(str(tmp_path / "ok"), "cpu")
    assert [os.path.relpath(str(f), str(tmp_path / "ok")) for f in bank.files] == sorted(pcm)
    assert bank.speakers == ["amy", "zed"] and bank.per_speaker == {"amy": [0], "zed": [1, 2]} and bank.recording_ids == ["u1", "u1", "u2"]
    for f, s, n in zip(bank.files, bank.starts, bank.lens):
        x = pcm[os.path.relpath(str(f), str(tmp_path / "ok"))]
        assert torch.equal(bank.data[s:s + n], torch.from_numpy(x[:, 0].astype(np.float32) / 32768.0))
    named = EM.EnrollmentBank.from_dir(str(tmp_path / "ok"), "cpu", speaker_of=lambda p: "x", recording_of=lambda p: p.parent.name + p.stem)
    assert named.speakers == ["x"] and named.recording_ids == ["amyu1", "zedu1", "zedu2"]
    with pytest.raises(IOError, match="does not exist"):
        EM.EnrollmentBank.from_dir(str(tmp_path / "missing"), "cpu")
    (tmp_path / "empty").mkdir()
    with pytest.raises(IOError, match="No .wav file found"):
        EM.EnrollmentBank.from_dir(str(tmp_path / "empty"), "cpu")
    _write_wav(str(tmp_path / "r8" / "s" / "x.wav"), pcm[os.path.join("zed", "u2.wav")], rate=8000)
    with pytest.raises(ValueError, match="8000 Hz"):
        EM.EnrollmentBank.from_dir(str(tmp_path / "r8"), "cpu")
    for width in (3, 4):
        _write_wav(str(tmp_path / f"w{width}" / "s" / "x.wav"), pcm[os.path.join("zed", "u2.wav")], width=width)
        with pytest.raises(ValueError, match=f"{8 * width}-bit"):
            EM.EnrollmentBank.from_dir(str(tmp_path / f"w{width}"), "cpu")
    _write_wav(str(tmp_path / "st" / "s" / "x.wav"), rng.integers(-9, 9, (50, 2)))
    with pytest.raises(ValueError, match="mono"):
        EM.EnrollmentBank.from_dir(str(tmp_path / "st"), "cpu")


def test_restatement_by_hand():
    data = np.array([np.nan, 1.0, 2.0, 3.0, np.nan, 0.5, -0.0, np.nan], dtype=np.float32)
    starts = [1, 5]
    tracks = [(0, 0, 1, 3), (0, 1, 3, 2), (0, 0, 3, 1), (2, 1, 0, 2)]
    got = R.mix(data, starts, tracks, 3, 6)
    assert got.tolist() == [[0.0, 1.0, 2.0, 4.5, 0.0, 0.0], [0.0] * 6, [0.5, 0.0, 0.0, 0.0, 0.0, 0.0]]
    assert np.signbit(got[2, 1]) and np.signbit(got[0, 4]) and not np.signbit(got[2, 2])            # one track: that clip's bits, -0 included
    # fp32, one rounding per track, in plan order
    data = np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=np.float32)
    assert R.mix(data, [0, 1, 2], [(0, 0, 0, 1), (0, 1, 0, 1), (0, 2, 0, 1)], 1, 1)[0, 0] == np.float32(1.0)
    assert R.mix(data, [0, 1, 2], [(0, 1, 0, 1), (0, 2, 0, 1), (0, 0, 0, 1)], 1, 1)[0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)
    sup = [[("a", 0, 10)], [("b", 2, 6), ("a", 8, 12)]]
    assert R.intervals_of_row(sup, [(0, 0, 5, 4), (0, 1, 0, 9), (1, 0, 0, 10)], 0) == {"a": [(5, 9), (8, 9)], "b": [(2, 6)]}
    assert R.intervals_of_row(sup, [(0, 1, 100, 2)], 0) == {"b": [], "a": []}                         # cut away: the speakers stay


def test_track_intervals_agree_with_the_restatement_on_f25(f25):
    z, bank = f25
    sup = R.f25_supervisions()
    sup = [s if s is not None else [(R.F25_CLIPS[k][0][0], 0, R.f25_lens()[k])] for k, s in enumerate(sup)]
    assert bank.supervisions == sup
    seen_multi = seen_cut = 0
    for name in R.f25_case_names(z):
        w = np.asarray(z[f"{name}.tracks"])
        tracks = R.tracks_in_samples(w[:, 0], w[:, 1], w[:, 2], w[:, 3], R.f25_options(z, name)["max_enrollment_len"])
        for r in sorted(set(tracks[:, 0].tolist())):
            assert EM.track_intervals(bank, tracks, r) == R.intervals_of_row(sup, tracks, r), (name, r)
        seen_multi += int((tracks[:, 1] == 10).any())
        seen_cut += int(any(ln < bank.lens[c] for _, c, _, ln in tracks.tolist()))
    assert seen_multi >= 2 and seen_cut >= 5


def test_wrappers_refuse_a_cpu_bank_and_front_end_passes_other_batches_on(f25):
    _, bank = f25
    with pytest.raises(_lib.DicowError, match="GPU"):
        EM.mix_enrollments(bank, torch.zeros(0, 4, dtype=torch.int32), 2, 16)
    with pytest.raises(_lib.DicowError, match="GPU"):
        EM.mix_enrollments(object(), torch.zeros(0, 4, dtype=torch.int32), 2, 16)
    seen = []
    fe = EM.EnrollmentMixFrontEnd(bank, 80, wave_front_end=lambda b: seen.append(b) or b, num_other_speakers=1)
    batch = {"input_waves": 1, "labels": 2}                                # no target speakers: nothing to mix, nothing drawn
    st_n, st_r = np.random.get_state()[1].copy(), random.getstate()
    assert fe(batch) is batch and seen == [batch]
    assert np.array_equal(np.random.get_state()[1], st_n) and random.getstate() == st_r

"""CPU tests of background-noise mixing's host side: the two C-ABI entry points and their binding, the planner against the draws the
reference made (golden F23), the noise bank's preparation and its WAV loader, and the fp64 restatement the GPU tests use as their oracle
(pinned to F23, which the reference's own class produced).  No GPU needed."""
import os
import random
import re
import wave

import numpy as np
import pytest
import torch

import amd_pkg
from tests import noise_mix_ref as R
from tests.util import ROOT, T

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, wave_augment  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_noise_mix\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const float* wave", "int64_t ld_wave", "float* out", "int64_t ld_out", "const float* bank", "const int64_t* clip_start",
                    "const int* clip_len", "const int* plan_i", "const float* plan_snr", "int n_plan", "void* ws", "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_noise_mix_ws_bytes\s*\(\s*int n_plan,\s*int max_len\s*\);", stable, flags=re.M)
    m = re.search(r"^#define\s+DICOW_NOISE_MIX_CHUNK\s+(\d+)", stable, flags=re.M)
    assert m and int(m.group(1)) == _lib.NOISE_MIX_CHUNK == wave_augment.NOISE_MIX_CHUNK and _lib.NOISE_MIX_CHUNK % 4 == 0
    c = _lib
    assert _lib._SIGS["dicow_noise_mix"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_vp, c.c_vp, c.c_vp, c.c_vp, c.c_i, c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_noise_mix_ws_bytes"] == [c.c_i, c.c_i]
    assert {"dicow_noise_mix", "dicow_noise_mix_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_noise_mix.restype is c.c_i and lib.dicow_noise_mix_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("NoiseBank", "plan_background_noise", "mix_background_noise", "WaveFrontEnd"):
        assert getattr(pkg, name) is getattr(wave_augment, name) and name in pkg.__all__


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    assert lib.dicow_noise_mix_ws_bytes(0, 0) == 0 and lib.dicow_noise_mix_ws_bytes(16, 480000) >= 16 * 2 * 8
    # a row far longer than 30 s needs no more workspace: the range of a partial grows, not the number of partials
    assert lib.dicow_noise_mix_ws_bytes(16, 1 << 30) == lib.dicow_noise_mix_ws_bytes(16, 480000)
    for bad in ((-1, 10), (3, -1)):
        assert lib.dicow_noise_mix_ws_bytes(*bad) == -1 and b"noise_mix_ws_bytes" in lib.dicow_last_error()
    p = 4096                                                              # (never dereferenced: every call below is refused on the host)
    need = lib.dicow_noise_mix_ws_bytes(2, 1000)
    ok = dict(wave=p, ldw=1000, out=2 * p, ldo=1000, bank=p, cs=p, cl=p, pi=p, ps=p, n=2, ws=p, wsb=need)
    for bad in (dict(wave=None), dict(out=None), dict(bank=None), dict(cs=None), dict(cl=None), dict(pi=None), dict(ps=None), dict(ws=None),
                dict(n=-1), dict(wsb=need - 1), dict(wsb=-8), dict(ldw=-4), dict(ldo=-4), dict(ldw=1001), dict(ldo=1002), dict(wave=p + 4),
                dict(out=p + 8), dict(bank=p + 2), dict(out=p, ldo=1004), dict(n=1 << 16, wsb=1 << 40)):
        a = dict(ok, **bad)
        rc = lib.dicow_noise_mix(a["wave"], a["ldw"], a["out"], a["ldo"], a["bank"], a["cs"], a["cl"], a["pi"], a["ps"], a["n"], a["ws"],
                                 a["wsb"], None)
        assert rc == -1, bad
        assert b"noise_mix" in lib.dicow_last_error()
    # an empty plan launches nothing and needs nothing
    assert lib.dicow_noise_mix(None, 0, None, 0, None, None, None, None, None, 0, None, 0, None) == 0


def _plan_of_sequence(z):
    torch.manual_seed(R.SEQ_SEED)
    random.seed(R.SEQ_SEED)
    return wave_augment.plan_background_noise(R.seq_lengths(), list(R.SEQ_CLIP_LENS), R.SEQ_PROB)


def test_planner_reproduces_the_reference_draws_of_f23():
    z = R.load_f23()
    gate, clip, off, db = (np.asarray(z["seq." + k]) for k in ("gate", "clip", "offset", "snr_db"))
    lengths = R.seq_lengths()
    # the fixture covers what it is there for: every clip chosen, offsets drawn and not drawn, an equal-length pair among the gated samples
    assert gate.sum() >= 16 and set(clip[gate].tolist()) == set(range(len(R.SEQ_CLIP_LENS)))
    assert (off[gate] >= 0).any() and (off[gate] < 0).any() and not (off[~gate] >= 0).any()
    assert any(g and R.SEQ_CLIP_LENS[c] == ln for g, c, ln in zip(gate, clip, lengths))
    plan_i, plan_snr = _plan_of_sequence(z)
    assert plan_i.dtype == torch.int32 and plan_snr.dtype == torch.float32 and plan_i.shape == (int(gate.sum()), 4)
    assert plan_i[:, 0].tolist() == np.nonzero(gate)[0].tolist()                                        # the gates
    assert plan_i[:, 1].tolist() == clip[gate].tolist()
    assert plan_i[:, 2].tolist() == np.maximum(off[gate], 0).tolist()                                   # (no draw: offset 0)
    assert plan_i[:, 3].tolist() == [lengths[k] for k in np.nonzero(gate)[0]]
    assert plan_snr.tolist() == [float(np.float32(10 ** (d / 10))) for d in db[gate].tolist()]
    # and nothing more was drawn from either generator than the reference drew
    assert float(torch.rand(1)) == float(z["seq.next_torch"][0]) and random.random() == float(z["seq.next_random"])
    # the independent replay of tests/noise_mix_ref.py agrees as well
    torch.manual_seed(R.SEQ_SEED)
    random.seed(R.SEQ_SEED)
    assert R.replay_draws(lengths, R.SEQ_CLIP_LENS, R.SEQ_PROB) == [(int(k), int(clip[k]), int(off[k]), int(db[k])) for k in np.nonzero(gate)[0]]


def test_planner_with_prob_zero_draws_nothing():
    torch.manual_seed(5)
    random.seed(5)
    st_t, st_r = torch.get_rng_state(), random.getstate()
    plan_i, plan_snr = wave_augment.plan_background_noise([100, 200, 300], [50, 500], 0.0)
    assert plan_i.shape == (0, 4) and plan_i.dtype == torch.int32 and plan_snr.shape == (0,) and plan_snr.dtype == torch.float32
    assert torch.equal(torch.get_rng_state(), st_t) and random.getstate() == st_r
    # prob 1: every entry, SNR inside the bounds, offsets inside the clip
    plan_i, plan_snr = wave_augment.plan_background_noise([100, 200, 300], [50, 500], 1.0, 3, 4)
    assert plan_i[:, 0].tolist() == [0, 1, 2] and plan_i[:, 3].tolist() == [100, 200, 300]
    assert all(float(s) in (float(np.float32(10 ** 0.3)), float(np.float32(10 ** 0.4))) for s in plan_snr)
    assert all(0 <= o <= max(0, (50, 500)[c] - n) for _, c, o, n in plan_i.tolist())


def test_front_end_draws_row_enrollment_row_enrollment(monkeypatch):
    """SE-DiCoW: the reference's dataset calls get_features for a row and then for its nested enrollment."""
    seen = {}

    def fake_plan(lengths, bank, prob, lo, hi):
        seen["lengths"] = list(lengths)
        # entries 1 (enrollment 0), 2 (row 1), 5 (enrollment 2)
        return torch.tensor([[1, 0, 0, 11], [2, 0, 0, 20], [5, 0, 0, 31]], dtype=torch.int32), torch.tensor([1.0, 2.0, 3.0])

    mixed = []
    monkeypatch.setattr(wave_augment, "plan_background_noise", fake_plan)
    monkeypatch.setattr(wave_augment, "mix_background_noise", lambda w, bank, pi, ps: mixed.append((w, pi.tolist(), ps.tolist())) or w)
    monkeypatch.setattr(wave_augment.features, "log_mel", lambda w, m: ("mel", w, m))
    fe = wave_augment.WaveFrontEnd(80, bank=object(), musan_augment_prob=0.3)
    wr, we = torch.zeros(3, 40), torch.ones(3, 40)
    batch = {"input_waves": wr, "wave_lengths": [10, 20, 30], "labels": 7,
             "enrollments": {"input_waves": we, "wave_lengths": torch.tensor([11, 21, 31]), "stno_mask": 8}}
    enr_in = batch["enrollments"]
    out = fe(batch)
    assert seen["lengths"] == [10, 11, 20, 21, 30, 31]
    assert [(m[0] is wr, m[1], m[2]) for m in mixed] == [(True, [[1, 0, 0, 20]], [2.0]), (False, [[0, 0, 0, 11], [2, 0, 0, 31]], [1.0, 3.0])]
    assert mixed[1][0] is we
    assert set(out) == {"input_features", "labels", "enrollments"} and set(out["enrollments"]) == {"input_features", "stno_mask"}
    assert out["input_features"] == ("mel", wr, 80) and out["enrollments"]["input_features"] == ("mel", we, 80)
    assert "input_waves" in enr_in                                         # the caller's nested dict is not modified
    with pytest.raises(ValueError):
        wave_augment.WaveFrontEnd(80, bank=None, musan_augment_prob=0.3)


def test_noise_bank_from_tensors_stores_the_reference_preparation():
    g = torch.Generator().manual_seed(3)
    clips = [torch.rand(2, 1001, generator=g) - 0.5, torch.rand(777, generator=g) * 3 - 1, torch.rand(1, 5, generator=g), torch.rand(3, 64, generator=g) - 0.2]
    bank = wave_augment.NoiseBank.from_tensors(clips, "cpu")
    assert len(bank) == 4 and bank.lens == [1001, 777, 5, 64] and bank.starts == [0, 1001, 1778, 1783]
    assert bank.clip_start.dtype == torch.int64 and bank.clip_start.tolist() == bank.starts
    assert bank.clip_len.dtype == torch.int32 and bank.clip_len.tolist() == bank.lens
    assert bank.data.dtype == torch.float32 and bank.data.shape == (1847,)
    for c, s, n in zip(clips, bank.starts, bank.lens):
        c = c if c.dim() == 2 else c[None]
        want = torch.mean(c, dim=0, keepdim=True) if c.shape[0] > 1 else c
        want = want / torch.max(torch.abs(want))
        assert torch.equal(bank.data[s:s + n], want[0])
        assert float(bank.data[s:s + n].abs().max()) == 1.0
    with pytest.raises(ValueError, match="zero"):
        wave_augment.NoiseBank.from_tensors([clips[0], torch.zeros(1, 100)], "cpu")
    with pytest.raises(ValueError):
        wave_augment.NoiseBank.from_tensors([], "cpu")
    with pytest.raises(ValueError):
        wave_augment.NoiseBank(torch.zeros(10), [0, 8], [8, 3])             # a clip that ends behind the buffer


def _write_wav(path, pcm, rate=16000, width=2):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes() if width == 2 else bytes(width * pcm.size))


def test_noise_bank_from_dir_reads_pcm16_in_glob_order(tmp_path):
    import pathlib
    rng = np.random.default_rng(4)
    pcm = {"b.wav": rng.integers(-32768, 32768, (300, 1)), "a.wav": rng.integers(-20000, 20000, (123, 2)),
           os.path.join("sub", "deep", "c.wav"): rng.integers(-5, 6, (40, 1)), os.path.join("sub", "d.wav"): rng.integers(-32768, 32768, (64, 1))}
    for name, x in pcm.items():
        _write_wav(str(tmp_path / name), x)
    (tmp_path / "notes.txt").write_text("not audio")
    bank = wave_augment.NoiseBank.from_dir(str(tmp_path), "cpu")
    order = list(pathlib.Path(str(tmp_path)).glob("**/*.wav"))
    assert len(order) == 4 and bank.files == order
    assert bank.lens == [pcm[os.path.relpath(str(f), str(tmp_path))].shape[0] for f in order]
    for f, s, n in zip(order, bank.starts, bank.lens):
        x = torch.from_numpy(pcm[os.path.relpath(str(f), str(tmp_path))].astype(np.float32) / 32768.0).t()        # what torchaudio.load returns
        want = torch.mean(x, dim=0, keepdim=True) if x.shape[0] > 1 else x
        want = want / torch.max(torch.abs(want))
        assert torch.equal(bank.data[s:s + n], want[0])
    with pytest.raises(IOError, match="does not exist"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "missing"), "cpu")
    (tmp_path / "empty").mkdir()
    with pytest.raises(IOError, match="No .wav file found"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "empty"), "cpu")
    _write_wav(str(tmp_path / "r8" / "x.wav"), pcm["b.wav"], rate=8000)
    with pytest.raises(ValueError, match="8000 Hz"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "r8"), "cpu")
    for width in (3, 4):
        _write_wav(str(tmp_path / f"w{width}" / "x.wav"), pcm["b.wav"], width=width)
        with pytest.raises(ValueError, match=f"{8 * width}-bit"):
            wave_augment.NoiseBank.from_dir(str(tmp_path / f"w{width}"), "cpu")


def test_restatement_agrees_with_the_reference_on_every_f23_case():
    """e_ref = max |ref32 - restatement64| <= 2^-20 max |restatement64|: the reference's own fp32 rounding (measured 4e-8 .. 3.3e-7 of the
    maximum); a one-sample slip of the offset or 1 dB of SNR is at least four orders larger."""
    z = R.load_f23()
    assert set(R.F23_CASES) == {k[:-4] for k in z.files if k.endswith(".out")}
    for name, (ln, ch, clen, zero_head, _) in R.F23_CASES.items():
        audio, clip, off, db, o64, ref32, pick = R.f23_case(z, name)
        assert int(z[name + ".clip"]) == 0 and ref32.dtype == torch.float32 and ref32.numel() == min(ln, 4096 if ln > R.FULL_OUT_MAX else ln)
        assert (int(z[name + ".offset"]) >= 0) == (clen > ln), name         # an offset is drawn only when the clip is longer
        e_ref, omax = R.e_ref_of(z, name)
        print(f"{name}: e_ref {e_ref:.3e} = {e_ref / omax:.2e} max|o64|")
        assert e_ref <= 2.0 ** -20 * omax, (name, e_ref, omax)
        # the fp32 torch arithmetic used for cases without a golden is the reference's, bit for bit
        assert torch.equal(pick(R.mix_reference32(audio, clip, off, db)), ref32), name
        # what the bound is there to catch
        if clen > ln and off + 1 + ln <= clen:
            slip = float((pick(R.mix_restatement64(audio, clip, off + 1, db)) - ref32.double()).abs().max())
            assert slip > 1e4 * 2.0 ** -20 * omax, (name, slip)
        wrong_db = float((pick(R.mix_restatement64(audio, clip, off, db + 1)) - ref32.double()).abs().max())
        assert wrong_db > 1e3 * 2.0 ** -20 * omax, (name, wrong_db)
    assert int(z["zero_head.offset"]) <= 4000 < int(z["zero_head.offset"]) + 5000


def test_restatement_of_a_silent_crop_is_half_the_audio():
    audio = torch.tensor([0.25, -0.5, 0.125])
    clip = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])
    assert torch.equal(R.mix_restatement64(audio, clip, 0, 5), audio.double() / 2)
    assert torch.equal(R.mix_reference32(audio, clip, 1, 5), audio / 2)
    assert not torch.equal(R.mix_restatement64(audio, clip, 2, 5), audio.double() / 2)


def test_wrapper_refuses_cpu_tensors():
    bank = wave_augment.NoiseBank.from_tensors([torch.ones(8)], "cpu")
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_augment.mix_background_noise(torch.zeros(2, 16), bank, torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0))

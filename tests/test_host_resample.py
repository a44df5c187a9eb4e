"""CPU tests of the any-rate audio intake's host side: the C-ABI entry points and their binding, the refusals made before any launch, the
filter bank's properties (the compact bank against the full one), the fp64 restatement the GPU tests use as their oracle (against the
analytic answer: torchaudio is not a dependency), the WAV reader, and the banks' unchanged default.  No GPU needed."""
import math
import os
import re
import types
import wave

import numpy as np
import pytest
import torch

import amd_pkg
from tests import resample_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, enrollment_mix, wave_augment, wave_intake  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_resample\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const void* in", "int in_int16", "int C", "int channel", "int64_t in_frames", "float* out", "int64_t out_samples",
                    "const float* taps_t", "const int32_t* first", "int o", "int n", "int width", "int S", "const int64_t* segs", "int n_segs",
                    "int frames_per_tile", "void* ws", "int64_t ws_bytes", "void* stream"]
    assert re.search(r"^int64_t\s+dicow_resample_ws_bytes\s*\(\s*int n_segs,\s*int n\s*\);", stable, flags=re.M)
    for name, val in (("LDS_BYTES", _lib.RESAMPLE_LDS_BYTES), ("MAX_RATIO", _lib.RESAMPLE_MAX_RATIO), ("MAX_CHANNELS", _lib.RESAMPLE_MAX_CHANNELS)):
        m = re.search(rf"^#define\s+DICOW_RESAMPLE_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    c = _lib
    assert _lib._SIGS["dicow_resample"] == [c.c_vp, c.c_i, c.c_i, c.c_i, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_vp, c.c_i, c.c_i, c.c_i, c.c_i,
                                            c.c_vp, c.c_i, c.c_i, c.c_vp, c.c_i64, c.c_vp]
    assert _lib._SIGS64["dicow_resample_ws_bytes"] == [c.c_i, c.c_i]
    assert {"dicow_resample", "dicow_resample_ws_bytes"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_resample.restype is c.c_i and lib.dicow_resample_ws_bytes.restype is c.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("ResamplePlan", "resample_plan", "resample_segments", "resample", "read_wav", "load_recording"):
        assert getattr(pkg, name) is getattr(wave_intake, name) and name in pkg.__all__


def _call(lib, plan, segs, **kw):
    """dicow_resample with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    segs = np.ascontiguousarray(np.asarray(segs, np.int64).reshape(-1, 3))
    first = plan.first.numpy()
    a = dict(inp=p, is16=0, C=1, ch=-1, in_frames=1000, out=2 * p, out_samples=1000, taps=p, first=first.ctypes.data, o=plan.o, n=plan.n,
             width=plan.width, S=plan.S, segs=segs.ctypes.data if len(segs) else None, n_segs=len(segs), F=0, ws=p,
             wsb=lib.dicow_resample_ws_bytes(len(segs), plan.n))
    a.update(kw)
    return lib.dicow_resample(a["inp"], a["is16"], a["C"], a["ch"], a["in_frames"], a["out"], a["out_samples"], a["taps"], a["first"], a["o"],
                              a["n"], a["width"], a["S"], a["segs"], a["n_segs"], a["F"], a["ws"], a["wsb"], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    assert lib.dicow_resample_ws_bytes(0, 1) == 8 and lib.dicow_resample_ws_bytes(3, 160) == 3 * 32 + 640
    for bad in ((-1, 1), (1, -1)):
        assert lib.dicow_resample_ws_bytes(*bad) == -1 and b"resample_ws_bytes" in lib.dicow_last_error()
    plan = wave_intake.resample_plan(44100, 16000)
    ok = [(0, 441, 0), (441, 100, 160)]                                   # 160 and ceil(160 * 100 / 441) = 37 output samples
    for bad, word in ((dict(segs=[(0, -1, 0)]), b"segment 0"), (dict(segs=[(-1, 5, 0)]), b"segment 0"), (dict(segs=[(990, 11, 0)]), b"input"),
                      (dict(segs=[(0, 441, 841)]), b"output"), (dict(segs=[(0, 441, -1)]), b"output"),
                      (dict(segs=[(0, 441, 0), (441, 100, 159)]), b"overlapping"), (dict(segs=[(0, 441, 100), (441, 441, 0)]), b"overlapping"),
                      (dict(segs=ok, o=0), b"MAX_RATIO"), (dict(segs=ok, n=(1 << 20) + 1), b"MAX_RATIO"), (dict(segs=ok, S=0), b"S="),
                      (dict(segs=ok, S=plan.K + 1), b"S="), (dict(segs=ok, width=-1), b"width"), (dict(segs=ok, is16=2), b"in_int16"),
                      (dict(segs=ok, C=2), b"mono"), (dict(segs=ok, is16=1, C=513), b"channels"), (dict(segs=ok, is16=1, C=0), b"channels"),
                      (dict(segs=ok, ch=1), b"channel"), (dict(segs=ok, is16=1, C=2, ch=2), b"channel"), (dict(segs=ok, ch=-2), b"channel"),
                      (dict(segs=ok, in_frames=-1), b"negative"), (dict(segs=ok, out_samples=-1), b"negative"), (dict(segs=ok, F=-1), b"frames_per_tile"),
                      (dict(segs=ok, F=1000), b"DICOW_RESAMPLE_LDS_BYTES"), (dict(segs=ok, first=None), b"first"),
                      (dict(segs=ok, inp=None), b"null"), (dict(segs=ok, out=None), b"null"), (dict(segs=ok, taps=None), b"null"),
                      (dict(segs=ok, ws=None), b"null"), (dict(segs=ok, inp=4098), b"aligned"), (dict(segs=ok, out=4098), b"aligned"),
                      (dict(segs=ok, taps=4100), b"aligned"), (dict(segs=ok, ws=4100), b"aligned"), (dict(segs=ok, wsb=8), b"ws_bytes"),
                      (dict(segs=ok, segs_null=True), b"null segment")):
        if bad.pop("segs_null", False):
            rc = lib.dicow_resample(4096, 0, 1, -1, 1000, 8192, 1000, 4096, plan.first.numpy().ctypes.data, plan.o, plan.n, plan.width, plan.S,
                                    None, 2, 0, 4096, 1 << 20, None)
        else:
            rc = _call(lib, plan, **bad)
        assert rc == -1, bad
        assert b"resample" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    # a phase whose first tap lies outside the bank
    bad_first = plan.first.numpy().copy()
    bad_first[3] = plan.K
    assert _call(lib, plan, ok, first=bad_first.ctypes.data) == -1 and b"first[3]" in lib.dicow_last_error()
    # a reduced ratio whose single output frame does not fit the LDS budget is refused with the limit's name: two phases whose runs start
    # 15 000 input samples apart
    huge = types.SimpleNamespace(o=20011, n=2, width=100, S=50, first=torch.tensor([0, 15000], dtype=torch.int32))
    assert _call(lib, huge, [(0, 10, 0)]) == -1 and b"DICOW_RESAMPLE_LDS_BYTES = 49152" in lib.dicow_last_error()
    # an empty table, and segments that are all empty, launch nothing and need nothing
    assert _call(lib, plan, [], inp=None, out=None, taps=None, ws=None, wsb=0) == 0
    assert _call(lib, plan, [(5, 0, 7), (0, 0, 7)], inp=None, out=None, taps=None, ws=None, wsb=0) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_intake.resample(torch.zeros(100), 8000)
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_intake.resample(torch.zeros(100, 2, dtype=torch.int16), 8000)
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_intake.resample_segments(torch.zeros(100), wave_intake.resample_plan(8000, 16000), [(0, 100, 0)], torch.zeros(200))
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_intake.resample(np.zeros(4), 8000)
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_intake.load_recording("never-opened.wav", device="cpu")
    with pytest.raises(ValueError):
        wave_intake.resample_plan(0, 16000)
    with pytest.raises(_lib.DicowError, match="limit"):
        wave_intake.resample_plan((1 << 21) + 1, 16000)


@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_bank_properties(orig, new):
    b = R.bank(orig, new)
    plan = wave_intake.resample_plan(orig, new)
    o, n, width, K = R.sizes(orig, new)
    g = math.gcd(orig, new)
    assert (o, n) == (orig // g, new // g) and width == math.ceil(6 * o / (min(o, n) * 0.99)) and K == 2 * width + o
    # S is derived here, from the fp32 rounding of the full fp64 bank
    runs = []
    for p in range(n):
        nz = np.flatnonzero(b.h32[p])
        assert nz.size > 0
        assert np.all(b.h32[p, nz[0]:nz[-1] + 1] != 0), f"a zero inside the run of phase {p}"
        runs.append((int(nz[0]), int(nz[-1] - nz[0] + 1)))
    S = max(r[1] for r in runs)
    assert S <= 2 * math.ceil(6 * o / (min(o, n) * 0.99)) + 1 and S < K
    assert (plan.o, plan.n, plan.width, plan.K, plan.S) == (o, n, width, K, S) and b.S == S
    assert plan.first.dtype == torch.int32 and plan.first.tolist() == [r[0] for r in runs]
    assert plan.taps.dtype == torch.float32 and tuple(plan.taps.shape) == (n, S)
    # the product's bank is the restatement's: both round the same fp64 expression once (numpy's and libm's sin may differ in the last
    # fp64 bit, which moves an fp32 rounding by at most one ulp)
    assert np.allclose(plan.taps.numpy(), b.taps, rtol=2.0 ** -22, atol=0.0)
    assert plan._taps_t.shape == (S, n) and torch.equal(plan._taps_t.t(), plan.taps)
    assert wave_intake.resample_plan(orig, new) is plan and wave_intake.resample_plan(2 * orig, 2 * new) is plan      # cached per reduced ratio
    # the compact bank times the input equals the full fp32 bank times the input: every dropped tap is exactly zero
    for L in (1, 7, 442, 4097):
        x = R.wave(orig, new, L).numpy()
        full, compact = R.resample64(x, b), R.resample64_compact(x, b)
        assert full.shape == compact.shape == (b.out_len(L),)
        assert float(np.max(np.abs(full - compact))) == 0.0, L
    for L in (1, 2, 7, 441, 442):
        want = -(-n * L // o)
        assert want == math.ceil(n * L / o) == plan.out_len(L) == R.resample64(np.zeros(L), b).shape[0] == R.reference32(np.zeros(L, np.float32), b).shape[0]


def test_identity_plan():
    plan = wave_intake.resample_plan(16000, 16000)
    assert plan.identity and (plan.o, plan.n, plan.width, plan.K, plan.S) == (1, 1, 0, 1, 1)
    assert plan.taps.tolist() == [[1.0]] and plan.first.tolist() == [0] and plan.out_len(12345) == 12345
    assert wave_intake.resample_plan(8000, 8000) is plan and not wave_intake.resample_plan(8000, 16000).identity


@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_restatement_resamples_a_sine(orig, new):
    """Formula sanity without torchaudio: a 440 Hz unit sine of 20 000 input samples comes out as the 440 Hz sine at the output rate, within
    1e-3 away from the ends (measured: at most 4.8e-4 over the eight ratios).  This bounds the filter's own passband ripple."""
    b = R.bank(orig, new)
    L = 20000
    x = np.sin(2 * math.pi * 440.0 * np.arange(L) / orig)
    y = R.resample64(x, b, b.h64)
    want = np.sin(2 * math.pi * 440.0 * np.arange(y.shape[0]) / new)
    assert y.shape[0] == b.out_len(L) > 800
    err = float(np.max(np.abs(y - want)[200:-200]))
    print(f"{orig} -> {new}: sine error {err:.2e}")
    assert err < 1e-3
    # and the fp32 rounding of the bank moves the answer by rounding errors only
    assert float(np.max(np.abs(R.resample64(x, b) - y))) < 1e-6


@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_sequential_fma_over_the_compact_bank_meets_the_gpu_bound(orig, new):
    """The GPU test's bound, rehearsed on the host with the order of operations the kernel uses and the plan the product builds."""
    b = R.bank(orig, new)
    plan = wave_intake.resample_plan(orig, new)
    worst = 0.0
    for L in R.LENGTHS:
        x = R.wave(orig, new, L).numpy()
        y64 = R.resample64(x, b)
        e_ref = float(np.max(np.abs(R.reference32(x, b).astype(np.float64) - y64)))
        got = R.emulate_kernel(x, plan.taps.numpy(), plan.first.numpy(), plan.o, plan.n, plan.width, plan.out_len(L))
        err = float(np.max(np.abs(got.astype(np.float64) - y64)))
        worst = max(worst, err / R.bound(y64, e_ref))
        assert err <= R.bound(y64, e_ref), (L, err, e_ref)
    print(f"{orig} -> {new}: emulated kernel at most {worst:.2f} of the bound")


def test_int16_mixdown_restatement_is_sum_then_one_division():
    """torch.mean(pcm / 32768, 0) = the exact channel sum, divided once by C and rounded once -- not a multiplication by 1 / C."""
    differs = False
    for C in (2, 3, 5, 7, 8):
        p = R.pcm(44100, 16000, 4097, C)
        want = R.mono_of(p)
        s = p.to(torch.int32).sum(1).to(torch.float64) / 32768.0            # exact
        assert torch.equal(want, (s / C).to(torch.float32)), C
        differs |= not torch.equal(want, s.to(torch.float32) * torch.tensor(1.0 / C, dtype=torch.float32))
    assert differs
    assert torch.equal(R.mono_of(R.pcm(8000, 16000, 50, 3), channel=1), R.pcm(8000, 16000, 50, 3)[:, 1].float() / 32768.0)


def _write_wav(path, pcm, rate=16000, width=2):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes() if width == 2 else bytes(width * pcm.size))


def test_read_wav_at_any_rate(tmp_path):
    rng = np.random.default_rng(7)
    stereo, mono = rng.integers(-32768, 32768, (301, 2)), rng.integers(-32768, 32768, (1000, 1))
    _write_wav(str(tmp_path / "a" / "s8.wav"), stereo, rate=8000)
    _write_wav(str(tmp_path / "a" / "m44.wav"), mono, rate=44100)
    pcm, rate = wave_intake.read_wav(tmp_path / "a" / "s8.wav")
    assert rate == 8000 and pcm.dtype == torch.int16 and tuple(pcm.shape) == (301, 2) and np.array_equal(pcm.numpy(), stereo)
    pcm, rate = wave_intake.read_wav(str(tmp_path / "a" / "m44.wav"))
    assert rate == 44100 and tuple(pcm.shape) == (1000, 1) and np.array_equal(pcm.numpy(), mono) and pcm.is_contiguous()
    for width in (1, 3, 4):
        _write_wav(str(tmp_path / f"w{width}.wav"), mono, width=width)
        with pytest.raises(ValueError, match=f"{8 * width}-bit"):
            wave_intake.read_wav(tmp_path / f"w{width}.wav")


def test_banks_still_refuse_another_rate_by_default_and_resample_on_the_cpu_is_refused(tmp_path):
    rng = np.random.default_rng(8)
    _write_wav(str(tmp_path / "n" / "x.wav"), rng.integers(-32768, 32768, (300, 1)), rate=8000)
    _write_wav(str(tmp_path / "e" / "spk" / "x.wav"), rng.integers(-32768, 32768, (300, 1)), rate=8000)
    with pytest.raises(ValueError, match="8000 Hz"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "n"), "cpu")
    with pytest.raises(ValueError, match="8000 Hz"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "n"), "cpu", resample=False)
    with pytest.raises(ValueError, match="8000 Hz"):
        enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "e"), "cpu")
    with pytest.raises(_lib.DicowError, match="GPU"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "n"), "cpu", resample=True)
    with pytest.raises(_lib.DicowError, match="GPU"):
        enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "e"), "cpu", resample=True)
    # with resample=True a directory that holds only files at the model's rate gives today's bank, bit for bit, on any device
    pcm = {"a.wav": rng.integers(-32768, 32768, (123, 2)), "b.wav": rng.integers(-3000, 3000, (77, 1))}
    for name, x in pcm.items():
        _write_wav(str(tmp_path / "n16" / name), x)
        _write_wav(str(tmp_path / "e16" / "spk" / name), x[:, :1])
    old, new = wave_augment.NoiseBank.from_dir(str(tmp_path / "n16"), "cpu"), wave_augment.NoiseBank.from_dir(str(tmp_path / "n16"), "cpu", resample=True)
    assert old.files == new.files and old.starts == new.starts and old.lens == new.lens and torch.equal(old.data, new.data)
    old = enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "e16"), "cpu")
    new = enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "e16"), "cpu", resample=True)
    assert old.files == new.files and old.lens == new.lens and torch.equal(old.data, new.data) and old.recording_ids == new.recording_ids

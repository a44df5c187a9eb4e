"""Any-rate audio intake on the GPU (csrc/resample.hip through wave_intake) vs the fp64 restatement of torchaudio's resampler
(tests/resample_ref.py, checked against the analytic sine by tests/test_host_resample.py).  Run with `pytest -m gpu`.

Tolerance of every numeric comparison, against the fp64 restatement y64 on the same fp32 bank and never against the product:
    max |k - y64| <= 4 e_ref + 2^-23 max |y64|
e_ref = max |reference fp32 - y64| on that case: the reference's formulation, fp32 conv1d(stride=o) with the full [n, 1, K] bank, on the CPU.
The kernel sums the compact run of a phase in ascending order with one fma per tap, conv1d sums K products in an order of its own: each a
rounding of the size of the reference's, hence the factor (the project's margin for another order of summation) and the ulp term.  The
mixdown of int16 input has no tolerance: it must be torch.mean's bits."""
import math
import os
import wave

import numpy as np
import pytest
import torch

import amd_pkg
from tests import resample_ref as R
from tests.util import SENTINEL16

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()

KINDS = [("fp32", None, None), ("i16c1", 1, None), ("i16c2", 2, None), ("i16c3", 3, None), ("i16c7", 7, None), ("i16c2ch1", 2, 1)]


@pytest.fixture(scope="module")
def W():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import wave_intake
    return wave_intake


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def case(orig, new, L, C, channel):
    """(what goes to the GPU, the fp32 mono signal the reference resamples) for one case."""
    if C is None:
        x = R.wave(orig, new, L)
        return x, x
    p = R.pcm(orig, new, L, C)
    return p, R.mono_of(p, channel)


_REF = {}


def expected(orig, new, L, C, channel):
    """(y64, bound) of one case, computed once."""
    key = (orig, new, L, C, channel)
    if key not in _REF:
        b = R.bank(orig, new)
        mono = case(orig, new, L, C, channel)[1].numpy()
        y64 = R.resample64(mono, b)
        e_ref = float(np.max(np.abs(R.reference32(mono, b).astype(np.float64) - y64)))
        _REF[key] = (y64, R.bound(y64, e_ref), e_ref)
    return _REF[key]


@pytest.mark.parametrize("orig,new", R.RATIOS)
def test_values_vs_restatement(W, orig, new):
    b = R.bank(orig, new)
    for kind, C, channel in KINDS:
        worst, e_lo, e_hi = 0.0, math.inf, 0.0
        for L in R.LENGTHS:
            src, _ = case(orig, new, L, C, channel)
            y64, tol, e_ref = expected(orig, new, L, C, channel)
            got = W.resample(src.cuda(), orig, new, channel=channel)
            assert got.dtype == torch.float32 and tuple(got.shape) == (b.out_len(L),) == y64.shape
            err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - y64)))
            worst, e_lo, e_hi = max(worst, err / tol), min(e_lo, e_ref), max(e_hi, e_ref)
            assert err <= tol, f"{orig} -> {new} {kind} L={L}: max|k - y64| {err:.3e} > {tol:.3e} (e_ref {e_ref:.3e})"
        print(f"resample {orig} -> {new} {kind}: max|k - y64| at most {worst:.2f} of the bound over {len(R.LENGTHS)} lengths, e_ref {e_lo:.1e} .. {e_hi:.1e}")


def test_equal_rates_are_the_mixdown_bit_for_bit(W):
    for C in (2, 3, 5, 7, 8):
        p = R.pcm(16000, 16000, 4097, C)
        got = W.resample(p.cuda(), 16000, 16000)
        assert torch.equal(got.cpu(), torch.mean(p.to(torch.float32).t() / 32768.0, 0)), C
    p = R.pcm(16000, 16000, 10007, 1)
    assert torch.equal(W.resample(p.cuda(), 16000).cpu(), p[:, 0].float() / 32768.0)
    assert torch.equal(W.resample(R.pcm(8000, 8000, 50, 3).cuda(), 8000, 8000, channel=2).cpu(), R.pcm(8000, 8000, 50, 3)[:, 2].float() / 32768.0)
    # the mixdown in front of a real ratio is the same bits: resampling int16 equals resampling its CPU mixdown
    for C, channel in ((2, None), (3, None), (7, None), (3, 1)):
        p = R.pcm(44100, 16000, 4097, C)
        assert torch.equal(W.resample(p.cuda(), 44100, channel=channel), W.resample(R.mono_of(p, channel).cuda(), 44100)), (C, channel)
    for L in (1, 3, 4, 4097):
        x = R.wave(16000, 16000, L)
        assert torch.equal(bits(W.resample(x.cuda(), 16000, 16000)), bits(x)), L


@pytest.mark.parametrize("orig,new", [(44100, 16000), (48000, 16000), (8000, 16000)])
def test_a_segment_does_not_depend_on_its_neighbours_the_run_or_the_tile(W, orig, new):
    plan = W.resample_plan(orig, new, "cuda")
    n_in = 10007
    lens = [n_in, 1, 4097, 0, 442, 7001, 50, 2, 7, 9999, 3000, 441, 882, 1, 6000, n_in]
    rows = torch.stack([R.wave(orig, new, n_in, tag=f"row{r}") for r in range(16)])
    alone = W.resample(rows[5, :lens[5]].cuda(), orig, new)
    batch = W.resample(rows.cuda(), orig, new, lengths=lens)
    again = W.resample(rows.cuda(), orig, new, lengths=lens)
    assert tuple(batch.shape) == (16, plan.out_len(n_in)) and tuple(alone.shape) == (plan.out_len(lens[5]),)
    assert torch.equal(bits(batch[5, :alone.numel()]), bits(alone)) and torch.equal(bits(batch), bits(again))
    for r, ln in enumerate(lens):                                          # every row is zero behind its own length
        m = plan.out_len(ln)
        assert not bool(batch[r, m:].any()), r
        assert ln == 0 or bool(batch[r, :m].any()), r
    # int16 stereo rows as well
    p = torch.stack([R.pcm(orig, new, n_in, 2, tag=f"row{r}") for r in range(4)])
    b16 = W.resample(p.cuda(), orig, new, lengths=[n_in, 5000, 4097, 3])
    assert torch.equal(bits(b16[1, :plan.out_len(5000)]), bits(W.resample(p[1, :5000].cuda(), orig, new)))
    # the tile: one frame per workgroup, three, and the library's choice
    flat, out_len = rows[5, :lens[5]].cuda().contiguous(), plan.out_len(lens[5])
    for F in (1, 3):
        out = torch.full((out_len,), float("nan"), device="cuda")
        W.resample_segments(flat, plan, [(0, lens[5], 0)], out, frames_per_tile=F)
        assert torch.equal(bits(out), bits(alone)), F
    flat16 = p[1, :5000].cuda().contiguous()
    out = torch.full((plan.out_len(5000),), float("nan"), device="cuda")
    W.resample_segments(flat16, plan, [(0, 5000, 0)], out, frames_per_tile=1)
    assert torch.equal(bits(out), bits(b16[1, :plan.out_len(5000)]))


def _sentinel(n, dtype):
    t = torch.empty(n, dtype=dtype)
    t.view(torch.int16).fill_(SENTINEL16)                                  # fp32: a quiet NaN; int16: 32705, close to full scale
    return t


@pytest.mark.parametrize("orig,new", [(44100, 16000), (8000, 16000)])
@pytest.mark.parametrize("kind,C", [("fp32", None), ("i16c1", 1), ("i16c2", 2), ("i16c3", 3)])
def test_guard_bands(W, orig, new, kind, C):
    """Poison before, between and behind the input segments, at buffer offsets 0-3 elements off 16-byte alignment; a canary around and
    between the output segments.  The outputs are those of the segments resampled alone, and the canary survives."""
    plan = W.resample_plan(orig, new, "cuda")
    lens, gaps = [4097, 1, 442, 1000], [5, 3, 1, 9, 6]                     # gaps: before, between, behind (frames)
    per = 1 if C is None else C
    clean = []
    for k, ln in enumerate(lens):
        src, _ = case(orig, new, ln, C, None)
        clean.append((src, W.resample(src.cuda(), orig, new).cpu()))
        assert bool(torch.isfinite(clean[-1][1]).all())
    for off in range(4):
        frames = sum(lens) + sum(gaps)
        host = _sentinel(off + frames * per + 64, torch.float32 if C is None else torch.int16)
        segs, at, out_at = [], gaps[0], 3
        for k, ln in enumerate(lens):
            host[off + at * per: off + (at + ln) * per] = clean[k][0].reshape(-1)
            segs.append((at, ln, out_at))
            at += ln + gaps[k + 1]
            out_at += plan.out_len(ln) + 2 + k                              # canary between the output segments
        dev = host.cuda()
        src = dev[off: off + frames * per]
        src = src if C is None else src.view(frames, C)
        assert src.data_ptr() % 16 == (off * (4 if C is None else 2)) % 16
        out_host = _sentinel(out_at + 61, torch.float32)
        out = out_host.cuda()
        W.resample_segments(src, plan, segs, out[1:])                      # (the output starts one element off 16-byte alignment)
        got = out.cpu()
        inside = torch.zeros(got.numel(), dtype=torch.bool)
        for (_, ln, o_at), (_, want) in zip(segs, clean):
            seg = got[1 + o_at: 1 + o_at + plan.out_len(ln)]
            assert bool(torch.isfinite(seg).all()), (off, ln)
            assert torch.equal(bits(seg), bits(want)), (off, ln)
            inside[1 + o_at: 1 + o_at + plan.out_len(ln)] = True
        assert torch.equal(got.view(torch.int32)[~inside], out_host.view(torch.int32)[~inside]), f"offset {off}: the canary was overwritten"
        assert torch.equal(dev.cpu().view(torch.int16), host.view(torch.int16))          # and the input is untouched


@pytest.mark.parametrize("orig,new", [(8000, 16000), (44100, 16000)])
def test_a_captured_call_replays_on_its_own_table(W, orig, new):
    """A captured resample_segments keeps the segment table it was captured with: another call on the same thread between capture and
    replay does not change what the replay computes.  Both tables have three rows inside the same src and out (table B: two other
    segments and an empty row), so that a replay which did read the later call's image would still read rows that exist and stay
    inside both buffers: wrong samples, never a wrong address."""
    from ts_asr_whisper_amd import ops
    plan = W.resample_plan(orig, new, "cuda")
    n_in = 4000
    src = R.wave(orig, new, n_in, tag="capture").cuda()
    seg_a = [(0, 1500, 3), (1500, 1000, 3 + plan.out_len(1500) + 2), (2600, 1400, 3 + plan.out_len(1500) + 2 + plan.out_len(1000) + 5)]
    seg_b = [(100, 1700, 40), (2000, 1900, 40 + plan.out_len(1700) + 1), (0, 0, 0)]
    total = max(s[2] + plan.out_len(s[1]) for s in seg_a + seg_b) + 61
    for segs in (seg_a, seg_b):
        assert all(0 <= s[0] and s[0] + s[1] <= n_in and 0 <= s[2] and s[2] + plan.out_len(s[1]) <= total for s in segs)
    canary = _sentinel(total, torch.float32)
    out = canary.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        W.resample_segments(src, plan, seg_a, out)                          # (code objects load outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = out.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    for in_start, in_len, out_start in seg_a:
        seg = want[out_start: out_start + plan.out_len(in_len)]
        assert torch.equal(bits(seg), bits(W.resample(src[in_start: in_start + in_len].contiguous(), orig, new)))
        inside[out_start: out_start + plan.out_len(in_len)] = True
    assert torch.equal(want.view(torch.int32)[~inside], canary.view(torch.int32)[~inside])
    out.copy_(canary)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        W.resample_segments(src, plan, seg_a, out)
        ws = ops.workspace(0, src.device)                                   # the capturing stream's workspace: the call's table lies at its head
    W.resample_segments(src, plan, seg_b, out)                              # another table, eagerly, before the first replay
    torch.cuda.synchronize()
    assert not torch.equal(bits(out), bits(want))
    for clear_ws in (False, True):
        out.copy_(canary)
        if clear_ws:
            ws[:pkg._lib.lib().dicow_resample_ws_bytes(len(seg_a), plan.n)].zero_()   # the replay uploads the table again
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want)), clear_ws


def test_wrapper_refusals_on_the_gpu(W):
    L = pkg._lib
    x = torch.zeros(100, device="cuda")
    for bad in (x.double(), torch.zeros(2, 3, 4, device="cuda"), torch.zeros(10, dtype=torch.int16, device="cuda")):
        with pytest.raises(L.DicowError):
            W.resample(bad, 8000)
    with pytest.raises(L.DicowError, match="channel"):
        W.resample(x, 8000, channel=1)
    with pytest.raises(L.DicowError, match="channel"):
        W.resample(torch.zeros(10, 2, dtype=torch.int16, device="cuda"), 8000, channel=2)
    with pytest.raises(L.DicowError, match="lengths"):
        W.resample(torch.zeros(2, 100, device="cuda"), 8000, lengths=[5, 101])
    with pytest.raises(L.DicowError, match="out"):
        W.resample(x, 8000, out=torch.zeros(199, device="cuda"))
    out = torch.empty(200, device="cuda")
    assert W.resample(x, 8000, out=out) is out and not bool(out.any())
    plan = W.resample_plan(8000, 16000, "cuda")
    with pytest.raises(L.DicowError, match="overlapping"):
        W.resample_segments(x, plan, [(0, 50, 0), (50, 50, 99)], torch.zeros(200, device="cuda"))
    with pytest.raises(L.DicowError, match="input"):
        W.resample_segments(x, plan, [(0, 101, 0)], torch.zeros(300, device="cuda"))
    with pytest.raises(L.DicowError, match="output"):
        W.resample_segments(x, plan, [(0, 100, 1)], torch.zeros(200, device="cuda"))
    assert tuple(W.resample(torch.zeros(0, device="cuda"), 8000).shape) == (0,)
    assert tuple(W.resample(torch.zeros(3, 0, 2, dtype=torch.int16, device="cuda"), 8000).shape) == (3, 0)


def _write_wav(path, pcm, rate):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.numpy().astype("<i2").tobytes())


def test_noise_bank_from_dir_resamples_other_rates(W, tmp_path):
    import pathlib
    from ts_asr_whisper_amd import wave_augment
    files = {"a16.wav": (R.pcm(16000, 16000, 3000, 2), 16000), "b8.wav": (R.pcm(8000, 16000, 1501, 1), 8000),
             os.path.join("sub", "c44.wav"): (R.pcm(44100, 16000, 10007, 2), 44100), os.path.join("sub", "d8.wav"): (R.pcm(8000, 16000, 777, 1, tag="d"), 8000)}
    for name, (p, rate) in files.items():
        _write_wav(str(tmp_path / "noise" / name), p, rate)
    bank = wave_augment.NoiseBank.from_dir(str(tmp_path / "noise"), "cuda", resample=True)
    order = list(pathlib.Path(str(tmp_path / "noise")).glob("**/*.wav"))
    assert bank.files == order and len(bank) == 4 and bank.data.is_cuda
    data = bank.data.cpu()
    for f, s, ln in zip(order, bank.starts, bank.lens):
        p, rate = files[os.path.relpath(str(f), str(tmp_path / "noise"))]
        assert ln == math.ceil(16000 * p.shape[0] / rate)
        clip = data[s:s + ln]
        assert float(clip.abs().max()) == 1.0
        if rate == 16000:                                                  # today's bank, bit for bit
            _write_wav(str(tmp_path / "only16" / "a16.wav"), p, rate)
            today = wave_augment.NoiseBank.from_dir(str(tmp_path / "only16"), "cpu")
            assert torch.equal(bits(clip), bits(today.data))
        else:                                                              # mono mean -> resample -> division by the resampled clip's peak
            y = W.resample(p.cuda(), rate, 16000)
            assert torch.equal(bits(clip), bits(y / torch.max(torch.abs(y))))
            y64 = R.resample64(R.mono_of(p).numpy(), R.bank(rate, 16000))
            assert float(np.max(np.abs(clip.numpy() * float(torch.max(torch.abs(y))) - y64))) < 1e-5
    with pytest.raises(ValueError, match="Hz"):
        wave_augment.NoiseBank.from_dir(str(tmp_path / "noise"), "cuda")
    # and the mixer runs on it
    wav = (R.wave(16000, 16000, 2 * 4096, tag="speech") * 0.1).reshape(2, 4096).cuda()
    plan_i = torch.tensor([[0, k, 10, 4000] for k in range(1)] + [[1, 2, 100, 4096]], dtype=torch.int32)
    mixed = wave_augment.mix_background_noise(wav, bank, plan_i, torch.tensor([3.0, 10.0]))
    assert bool(torch.isfinite(mixed).all()) and not torch.equal(mixed, wav)
    # the enrollment bank: mono only, unnormalised
    from ts_asr_whisper_amd import enrollment_mix
    _write_wav(str(tmp_path / "enr" / "alice" / "u1.wav"), files["b8.wav"][0], 8000)
    _write_wav(str(tmp_path / "enr" / "bob" / "u2.wav"), R.pcm(16000, 16000, 500, 1), 16000)
    eb = enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "enr"), "cuda", resample=True)
    assert eb.lens == [3002, 500] and eb.speakers == ["alice", "bob"]
    assert torch.equal(bits(eb.data[:3002]), bits(W.resample(files["b8.wav"][0].cuda(), 8000)))
    assert torch.equal(eb.data[3002:].cpu(), R.pcm(16000, 16000, 500, 1)[:, 0].float() / 32768.0)
    _write_wav(str(tmp_path / "enr2" / "carol" / "u3.wav"), files["a16.wav"][0], 8000)
    with pytest.raises(ValueError, match="mono"):
        enrollment_mix.EnrollmentBank.from_dir(str(tmp_path / "enr2"), "cuda", resample=True)


def test_load_recording_feeds_the_meeting_front_end(W, tmp_path):
    from ts_asr_whisper_amd import diar_front_end as D
    frames = 48000 * 2 + 123                                               # two seconds and a bit, 48 kHz, two channels
    p = R.pcm(48000, 16000, frames, 2)
    _write_wav(str(tmp_path / "rec" / "meeting.wav"), p, 48000)
    wav = W.load_recording(tmp_path / "rec" / "meeting.wav")
    n = math.ceil(16000 * frames / 48000)
    assert wav.is_cuda and wav.dtype == torch.float32 and tuple(wav.shape) == (n,)
    assert torch.equal(bits(wav), bits(W.resample(p.cuda(), 48000)))
    assert torch.equal(bits(W.load_recording(tmp_path / "rec" / "meeting.wav", channel=1)), bits(W.resample(p.cuda(), 48000, channel=1)))
    (tmp_path / "rec" / "meeting.rttm").write_text("SPEAKER meeting 1 0.10 0.90 <NA> <NA> alice <NA> <NA>\n"
                                                   "SPEAKER meeting 1 0.70 1.20 <NA> <NA> bob <NA> <NA>\n")
    segs = D.SpeakerSegments.from_rttm(str(tmp_path / "rec" / "meeting.rttm"), n_samples=n)
    batch = D.MeetingFrontEnd(80).prepare(wav, segs)
    K, T = 2, D.FRAMES_30S
    assert tuple(batch["input_features"].shape) == (K, 80, 2 * T) and tuple(batch["attention_mask"].shape) == (K, 2 * T)
    assert tuple(batch["stno_mask"].shape) == (K, 4, T) and int(batch["attention_mask"][0].sum()) == math.ceil(n / 160)
    assert bool(torch.isfinite(batch["input_features"]).all())

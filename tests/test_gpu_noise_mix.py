"""Background-noise mixing on the GPU (csrc/noise_mix.hip through wave_augment) vs the fp64 restatement of the reference's
RandomBackgroundNoise (tests/noise_mix_ref.py, pinned to golden F23 by tests/test_host_noise_mix.py).  Run with `pytest -m gpu`.

Tolerance of every numeric comparison, against the fp64 restatement o64 and never against the product:
    max |k - o64| <= 4 e_ref + 2^-23 max |o64|
e_ref = max |reference fp32 - o64|: from the golden for the F23 cases, else from the reference's arithmetic run in fp32 with torch on the
CPU (noise_mix_ref.mix_reference32, bit-equal to the reference on F23).  The product adds the two sums of squares in another, fixed order
than torch and contracts the last multiply-add; each is a rounding of the size of the reference's own, hence the factor and the ulp term.
Measured on the MI355X (profiles/noise_mix.txt): max |k - o64| between 0.2 and 1.0 e_ref on the F23 cases."""
import random

import pytest
import torch

import amd_pkg
from tests import noise_mix_ref as R
from tests.util import guarded, hashed_uniform, poisoned

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
CHUNK = pkg._lib.NOISE_MIX_CHUNK


@pytest.fixture(scope="module")
def wa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import wave_augment
    return wave_augment


def speech(name, shape):
    return hashed_uniform(name, shape) * R.SPEECH_AMP


def plan_of(rows):
    """rows: (row, clip, offset, len, snr_db) -> the planner's two tensors."""
    return (torch.tensor([r[:4] for r in rows], dtype=torch.int32).reshape(-1, 4),
            torch.tensor([10 ** (r[4] / 10) for r in rows], dtype=torch.float64).to(torch.float32))


def check_rows(got, wave, bank_cpu, rows, what):
    """Every planned row of `got` (CPU) against the restatement, within the module's tolerance; returns the worst (err, tol)."""
    worst = (0.0, 1.0)
    for row, clip, off, ln, db in rows:
        c = bank_cpu.data[bank_cpu.starts[clip]:bank_cpu.starts[clip] + bank_cpu.lens[clip]]
        a = wave[row, :ln]
        o64 = R.mix_restatement64(a, c, off, db)
        e_ref = float((R.mix_reference32(a, c, off, db).double() - o64).abs().max())
        tol = 4 * e_ref + 2.0 ** -23 * float(o64.abs().max())
        err = float((got[row, :ln].double() - o64).abs().max())
        assert err <= tol, f"{what}: row {row} clip {clip} offset {off} len {ln}: max|k - o64| {err:.3e} > {tol:.3e} (e_ref {e_ref:.3e})"
        if err / tol > worst[0] / worst[1]:
            worst = (err, tol)
    return worst


def test_f23_cases_vs_restatement(wa):
    z = R.load_f23()
    for name, (ln, ch, clen, zero_head, _) in R.F23_CASES.items():
        audio, clip, off, db, o64, ref32, pick = R.f23_case(z, name)
        _, raw = R.f23_inputs(name)
        bank = wa.NoiseBank.from_tensors([raw])
        assert torch.equal(bank.data.cpu(), clip)
        n = ln if ln == 480000 else ln + 5
        wave = torch.full((1, n), 0.375)
        wave[0, :ln] = audio
        pi, ps = plan_of([(0, 0, off, ln, db)])
        got = wa.mix_background_noise(wave.cuda(), bank, pi, ps).cpu()
        assert got.shape == (1, n) and torch.equal(got[0, ln:], wave[0, ln:])
        e_ref, omax = R.e_ref_of(z, name)
        err = float((pick(got[0, :ln]).double() - pick(o64)).abs().max())
        tol = 4 * e_ref + 2.0 ** -23 * omax
        print(f"F23 {name:12s} len {ln:7d}: max|k - o64| {err:.3e}   e_ref {e_ref:.3e}   bound {tol:.3e}   max|o64| {omax:.3e}")
        assert err <= tol, (name, err, tol, e_ref)
        # the full output too (the golden stores a subsample of the 30 s case): same bound, e_ref from the fp32 restatement of the reference
        full = float((got[0, :ln].double() - o64).abs().max())
        e_full = float((R.mix_reference32(audio, clip, off, db).double() - o64).abs().max())
        assert full <= 4 * e_full + 2.0 ** -23 * omax, (name, full, e_full)


def test_every_alignment_of_the_crop_and_short_lengths(wa):
    """clip 1 starts at an odd element of the bank; offsets 0..3 move the crop through every 4-byte alignment; lengths around the
    vector width and the wave width.  SNRs are 1 .. 15 dB, not 0: at len = 1 and 0 dB, a and scale * n have the same magnitude, so with
    opposite signs o64 is exactly 0 and the bound, which is relative to max |o64|, collapses to 0 -- no fp32 evaluation with a rounded
    scale meets that, the accepted fma form included."""
    clips = [hashed_uniform("nm.align.c0", (7,)), hashed_uniform("nm.align.c1", (600,))]
    bank, bank_cpu = wa.NoiseBank.from_tensors(clips), wa.NoiseBank.from_tensors(clips, "cpu")
    assert bank.starts[1] % 2 == 1
    lens = (1, 2, 3, 4, 5, 63, 64, 65, 255, 257)
    rows = [(4 * k + off, 1, off, ln, 1 + (3 * k + off) % 15) for k, ln in enumerate(lens) for off in range(4)]
    wave = speech("nm.align.wave", (len(rows), 260))
    got = wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows)).cpu()
    check_rows(got, wave, bank_cpu, rows, "alignment")
    for row, _, _, ln, _ in rows:
        assert torch.equal(got[row, ln:], wave[row, ln:]), (row, ln)


def test_chunk_boundaries(wa):
    """Lengths around one and two chunks, against a clip that ends one sample behind the crop and one that ends inside the last chunk;
    and a row longer than 64 chunks, where the range of a partial sum doubles."""
    off = 5
    lens = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
    clens = [off + ln + 1 for ln in lens] + [off + ln - 100 for ln in lens]
    clips = [hashed_uniform(f"nm.chunk.c{k}", (n,)) for k, n in enumerate(clens)]
    bank, bank_cpu = wa.NoiseBank.from_tensors(clips), wa.NoiseBank.from_tensors(clips, "cpu")
    rows = [(k, k, off, lens[k % 4], 2 * k) for k in range(8)]
    wave = speech("nm.chunk.wave", (8, 2 * CHUNK + 8))
    got = wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows)).cpu()
    check_rows(got, wave, bank_cpu, rows, "chunks")
    for row, _, _, ln, _ in rows:
        assert torch.equal(got[row, ln:], wave[row, ln:]), (row, ln)
    ln = 64 * CHUNK + 5
    clips = [hashed_uniform("nm.chunk.long", (ln + 3,))]
    bank, bank_cpu = wa.NoiseBank.from_tensors(clips), wa.NoiseBank.from_tensors(clips, "cpu")
    wave = speech("nm.chunk.longwave", (1, ln + 3))
    rows = [(0, 0, 2, ln, 7)]
    got = wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows)).cpu()
    check_rows(got, wave, bank_cpu, rows, "row of more than 64 chunks")
    assert torch.equal(got[0, ln:], wave[0, ln:])


def test_guard_bands_around_rows_and_bank(wa):
    """wave and out as padded views (ld = n + 12) inside NaN, the bank inside NaN: a read outside a row or a clip puts NaN into the
    output, a write outside a row breaks a sentinel."""
    n = 1000
    clips = [hashed_uniform("nm.guard.c0", (333,)), hashed_uniform("nm.guard.c1", (50,)), hashed_uniform("nm.guard.c2", (701,))]
    bank_cpu = wa.NoiseBank.from_tensors(clips, "cpu")
    total = bank_cpu.data.numel()
    data = poisoned(bank_cpu.data[None], total, kind="nan")[0]
    around = torch.as_strided(data, (2,), (total + 1,), data.storage_offset() - 1)        # the elements directly before and behind the bank
    assert data.is_contiguous() and data.storage_offset() > 0 and bool(torch.isnan(around).all())
    bank = wa.NoiseBank(data, bank_cpu.starts, bank_cpu.lens)
    # crops that start at the first sample of the first clip, end at the last sample of the last clip, and run past a clip's end
    rows = [(0, 0, 0, 333, 3), (1, 2, 0, 701, 9), (2, 2, 700, 1000, 0), (3, 0, 1, 999, 15), (4, 1, 49, 1, 5), (5, 2, 698, 3, 6), (6, 0, 3, 330, 1)]
    wave = speech("nm.guard.wave", (8, n))
    wave_d = poisoned(wave, n + 12, kind="nan")
    assert wave_d.stride(0) == n + 12 and wave_d.data_ptr() % 16 == 0
    out = guarded((8, n), n + 12, torch.float32, name="noise_mix out")
    got = wa.mix_background_noise(wave_d, bank, *plan_of(rows), out=out.view)
    assert got is out.view
    torch.cuda.synchronize()
    out.check()
    assert out.untouched_inside() == 0 and not bool(torch.isnan(out.view).any())
    assert torch.equal(wave_d.cpu(), wave)
    check_rows(out.view.cpu(), wave, bank_cpu, rows, "guards")
    # the same from the padded view alone (the wrapper allocates the output) and in place on the padded view
    got2 = wa.mix_background_noise(wave_d, bank, *plan_of(rows))
    assert torch.equal(got2, out.view)
    wave_g = guarded((8, n), n + 12, torch.float32, init=wave, name="noise_mix in place")
    assert wa.mix_background_noise(wave_g.view, bank, *plan_of(rows), out=wave_g.view) is wave_g.view
    wave_g.check()
    assert torch.equal(wave_g.view, out.view)
    # a batch whose rows cannot be aligned (n % 4 != 0) is copied into aligned rows by the wrapper
    odd = speech("nm.guard.odd", (3, 1001))
    rows_odd = [(0, 2, 1, 1001, 4), (2, 0, 0, 1000, 8)]
    got3 = wa.mix_background_noise(odd.cuda(), bank, *plan_of(rows_odd))
    assert got3.shape == (3, 1001) and torch.equal(got3[1].cpu(), odd[1]) and float(got3[2, 1000]) == float(odd[2, 1000])
    check_rows(got3.cpu(), odd, bank_cpu, rows_odd, "unaligned batch")


def _batch4(wa):
    clips = [hashed_uniform("nm.b4.c0", (2, 5000)), hashed_uniform("nm.b4.c1", (1200,))]
    bank, bank_cpu = wa.NoiseBank.from_tensors(clips), wa.NoiseBank.from_tensors(clips, "cpu")
    wave = speech("nm.b4.wave", (4, 3000))
    wave[wave == 0] = 0.01                                               # a non-zero pattern everywhere, behind len as well
    rows = [(1, 0, 1234, 1777, 6), (3, 1, 17, 2999, 11)]
    return bank, bank_cpu, wave, rows


def test_untouched_rows_and_tails_keep_their_bits(wa):
    bank, bank_cpu, wave, rows = _batch4(wa)
    wave_d = wave.cuda()
    got = wa.mix_background_noise(wave_d, bank, *plan_of(rows))
    assert got.data_ptr() != wave_d.data_ptr() and torch.equal(wave_d.cpu(), wave)        # out of place: the input is unchanged
    got = got.cpu()
    assert torch.equal(got[0], wave[0]) and torch.equal(got[2], wave[2])
    for row, _, _, ln, _ in rows:
        assert torch.equal(got[row, ln:], wave[row, ln:]) and not bool((got[row, :ln] == wave[row, :ln]).all())
    check_rows(got, wave, bank_cpu, rows, "B = 4")


def test_in_place_gives_the_same_bits(wa):
    bank, _, wave, rows = _batch4(wa)
    want = wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows))
    w = wave.cuda()
    got = wa.mix_background_noise(w, bank, *plan_of(rows), out=w)
    assert got is w and torch.equal(w, want)
    # out given and distinct: filled completely
    o = torch.full_like(w, float("nan"))
    assert wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows), out=o) is o and torch.equal(o, want)


def test_rows_are_independent_and_runs_reproducible(wa):
    B, n = 16, 480000
    clips = [hashed_uniform("nm.ind.c0", (600001,)), hashed_uniform("nm.ind.c1", (100000,)), hashed_uniform("nm.ind.c2", (480000,))]
    bank = wa.NoiseBank.from_tensors(clips)
    wave = speech("nm.ind.wave", (B, n)).cuda()
    rows = [(r, r % 3, (0 if r % 3 == 2 else 1000 * r + r), n if r % 4 else n - 777 * r - 1, r) for r in range(B)]
    pi, ps = plan_of(rows)
    a = wa.mix_background_noise(wave, bank, pi, ps)
    b = wa.mix_background_noise(wave, bank, pi, ps)
    assert torch.equal(a, b)
    assert not bool(torch.isnan(a).any()) and not torch.equal(a[5], wave[5])
    alone = wa.mix_background_noise(wave[5:6], bank, *plan_of([(0,) + rows[5][1:]]))
    assert torch.equal(alone[0], a[5])
    # and in another position of the plan, beside other rows
    few = wa.mix_background_noise(wave, bank, *plan_of([rows[9], rows[5], rows[2]]))
    assert torch.equal(few[5], a[5]) and torch.equal(few[9], a[9]) and torch.equal(few[0], wave[0])


def test_silent_crop_gives_half_the_audio(wa):
    """The stated deviation: the reference divides by the crop's zero norm and returns NaN on every sample."""
    raw = hashed_uniform("nm.silent.c0", (3000,))
    raw[:2000] = 0.0
    bank = wa.NoiseBank.from_tensors([raw])
    wave = speech("nm.silent.wave", (3, 1500))
    wave[2] = 0.0
    rows = [(0, 0, 100, 1500, 3), (1, 0, 499, 1500, 3), (2, 0, 1000, 1500, 3)]      # row 1 ends one sample before the zeros end
    got = wa.mix_background_noise(wave.cuda(), bank, *plan_of(rows)).cpu()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got[0], wave[0] * 0.5) and torch.equal(got[1], wave[1] * 0.5)
    assert torch.equal(got[2], torch.zeros(1500))                                    # zero audio: scale 0, as in the reference
    # one sample further the crop is not silent any more
    got = wa.mix_background_noise(wave.cuda(), bank, *plan_of([(1, 0, 501, 1500, 3)])).cpu()
    assert not torch.equal(got[1], wave[1] * 0.5) and torch.equal(got[1, :1499], wave[1, :1499] * 0.5)


def test_wrapper_refusals_and_the_empty_plan(wa):
    bank = wa.NoiseBank.from_tensors([hashed_uniform("nm.ref.c0", (100,)), hashed_uniform("nm.ref.c1", (40,))])
    wave = speech("nm.ref.wave", (3, 64)).cuda()
    E = pkg._lib.DicowError
    for rows, match in (([(1, 0, 0, 10, 3), (1, 1, 0, 10, 3)], "twice"), ([(3, 0, 0, 10, 3)], "outside the batch"), ([(-1, 0, 0, 10, 3)], "outside the batch"),
                        ([(0, 0, 0, 65, 3)], "len"), ([(0, 0, 0, 0, 3)], "len"), ([(0, 1, 40, 10, 3)], "behind clip"), ([(0, 1, -1, 10, 3)], "behind clip"),
                        ([(0, 2, 0, 10, 3)], "clip 2")):
        with pytest.raises(E, match=match):
            wa.mix_background_noise(wave, bank, *plan_of(rows))
    ok = plan_of([(0, 0, 0, 10, 3)])
    with pytest.raises(E, match="GPU"):
        wa.mix_background_noise(wave.cpu(), bank, *ok)
    with pytest.raises(E, match="fp32"):
        wa.mix_background_noise(wave.bfloat16(), bank, *ok)
    with pytest.raises(E, match="overlaps"):
        wa.mix_background_noise(wave[:2], bank, *ok, out=wave[1:])
    with pytest.raises(E, match="SNR"):
        wa.mix_background_noise(wave, bank, ok[0], torch.zeros(2))
    torch.cuda.synchronize()
    assert torch.equal(wave.cpu(), speech("nm.ref.wave", (3, 64)))                   # nothing was launched
    got = wa.mix_background_noise(wave, bank, torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0))
    assert got.data_ptr() != wave.data_ptr() and torch.equal(got, wave)
    assert wa.mix_background_noise(wave, bank, torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0), out=wave) is wave


# ------------------------------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def front(wa):
    from ts_asr_whisper_amd import features
    clips = [hashed_uniform("nm.fe.c0", (2, 500001)), hashed_uniform("nm.fe.c1", (30000,))]
    bank = wa.NoiseBank.from_tensors(clips)
    lens = [480000, 312345]
    waves = [speech(f"nm.fe.wave{k}", (n,)) for k, n in enumerate(lens)]
    wave, _ = features.pad_to_30s(waves)
    assert wave.shape == (2, 480000)
    return bank, wave.cuda(), lens


def _seed(s=7):
    torch.manual_seed(s)
    random.seed(s)


def test_front_end_equals_plan_mix_logmel_by_hand(wa, front):
    from ts_asr_whisper_amd import features
    bank, wave, lens = front
    fe = wa.WaveFrontEnd(80, bank, musan_augment_prob=1.0)
    _seed()
    out = fe({"input_waves": wave, "wave_lengths": lens, "labels": None})
    assert set(out) == {"input_features", "labels"}
    _seed()
    pi, ps = wa.plan_background_noise(lens, bank, 1.0)
    assert pi[:, 0].tolist() == [0, 1] and pi[:, 3].tolist() == lens
    mixed = wa.mix_background_noise(wave, bank, pi, ps)
    assert not torch.equal(mixed, wave) and torch.equal(mixed[1, lens[1]:], wave[1, lens[1]:])
    want = features.log_mel(mixed, 80)
    assert out["input_features"].shape == (2, 80, 3000) and torch.equal(out["input_features"], want)
    # probability 0: the plain front end, and no draw
    _seed()
    st_t, st_r = torch.get_rng_state(), random.getstate()
    out0 = wa.WaveFrontEnd(80, bank, musan_augment_prob=0.0)({"input_waves": wave, "wave_lengths": lens})
    assert set(out0) == {"input_features"} and torch.equal(out0["input_features"], features.log_mel(wave, 80))
    assert torch.equal(torch.get_rng_state(), st_t) and random.getstate() == st_r
    assert torch.equal(wa.WaveFrontEnd(80)({"input_waves": wave})["input_features"], out0["input_features"])
    # SE-DiCoW: the enrollments' waves go the same way, drawn between the rows'
    _seed()
    out2 = fe({"input_waves": wave, "wave_lengths": lens, "enrollments": {"input_waves": wave.flip(0), "wave_lengths": lens[::-1]}})
    _seed()
    pi, ps = wa.plan_background_noise([lens[0], lens[1], lens[1], lens[0]], bank, 1.0)
    rows, enr = pi[:, 0] % 2 == 0, pi[:, 0] % 2 == 1
    pr, pe = pi[rows].clone(), pi[enr].clone()
    pr[:, 0] //= 2
    pe[:, 0] //= 2
    assert torch.equal(out2["input_features"], features.log_mel(wa.mix_background_noise(wave, bank, pr, ps[rows]), 80))
    assert torch.equal(out2["enrollments"]["input_features"], features.log_mel(wa.mix_background_noise(wave.flip(0), bank, pe, ps[enr]), 80))
    assert set(out2["enrollments"]) == {"input_features"}


def test_train_step_runs_from_waves(wa, front):
    from ts_asr_whisper_amd.data import synthetic_batch
    from ts_asr_whisper_amd.trainer import TrainStep
    bank, wave, lens = front
    cfg = pkg.DiCoWConfig(vocab_size=512, num_mel_bins=80, d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=1,
                          decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256, max_source_positions=1500, max_target_positions=32,
                          pad_token_id=500, bos_token_id=500, eos_token_id=500, decoder_start_token_id=501, use_pre_pos_fddt=True,
                          non_target_fddt_value=0.5)
    torch.manual_seed(0)
    models = [pkg.DiCoWForConditionalGeneration(cfg).cuda() for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    for m in models:
        m.tie_weights()
    batch = synthetic_batch(cfg, 2, 12, seed=3)
    del batch["input_features"]
    fe = wa.WaveFrontEnd(80, bank, musan_augment_prob=1.0)
    _seed(11)
    loss_w = TrainStep(models[0], front_end=fe).step(dict(batch, input_waves=wave, wave_lengths=lens))
    _seed(11)
    feats = fe({"input_waves": wave, "wave_lengths": lens})["input_features"]
    ts = TrainStep(models[1], graph=True, front_end=fe)
    loss_f = ts.step(dict(batch, input_features=feats), eager=True)     # no waves in the batch: the front end stays out of the way
    assert bool(torch.isfinite(loss_w)) and float(loss_w) == float(loss_f) and torch.equal(loss_w, loss_f)
    with pytest.raises(NotImplementedError):                            # the planner runs on the host: refused like the augmenter
        ts.step(dict(batch, input_waves=wave, wave_lengths=lens))

"""External enrollment mixtures on the GPU (csrc/enrollment_mix.hip through enrollment_mix) vs the numpy restatement of
tests/enrollment_mix_ref.py: the sequential fp32 sum of the shifted clips and the STNO mask of the mixture, whose plans golden F25 (the
reference's own generate_enrollment_mixture) pins in tests/test_host_enrollment_mix.py.  Run with `pytest -m gpu`.

Every comparison is a bit-equality or an exact integer: the kernel adds the covering tracks of a sample one by one in plan order with
__fadd_rn, which is numpy's fp32 addition, and the masks are the integer counts and correctly rounded fp32 products of the diarization
front end.  No tolerance is involved."""
import random

import numpy as np
import pytest
import torch

import amd_pkg
from tests import enrollment_mix_ref as R
from tests.util import guarded, hashed_uniform

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
N = 1024
N30 = 480000


@pytest.fixture(scope="module")
def em():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import enrollment_mix
    return enrollment_mix


@pytest.fixture(scope="module")
def small(em):
    return R.small_bank(em)


def plan_of(rows):
    """rows: per output row a list of (clip, off, len) -> int32 [n, 4]."""
    return torch.tensor([(r, c, o, ln) for r, tr in enumerate(rows) for c, o, ln in tr], dtype=torch.int32).reshape(-1, 4)


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.shape == want.shape and np.array_equal(got.view(np.int32), np.asarray(want, dtype=np.float32).view(np.int32))


def by_residue(starts, lens):
    """residue of the clip start modulo 4 -> the longest clip (of the short ones) that starts there."""
    out = {}
    for k, (s, ln) in enumerate(zip(starts, lens)):
        if ln <= N and (s % 4 not in out or ln > lens[out[s % 4]]):
            out[s % 4] = k
    return out


def edge_rows(starts, lens):
    """The rows of the bit-equality test: 0 to 4 and 8 tracks; tracks that abut, nest, coincide and leave gaps; every combination of
    clip_start % 4 and off % 4; lengths 1 .. 9, 255 .. 257 and one that runs to the end of the row."""
    res = by_residue(starts, lens)
    assert sorted(res) == [0, 1, 2, 3] and all(lens[k] >= 5 for k in res.values()), res
    rows = [[],                                                           # no track: zeros
            [(0, 0, N)],                                                  # one track, the whole row: the clip's bits
            [(2, 10, 257), (4, 267, 300)],                                # abut
            [(0, 3, 1000), (2, 100, 257), (6, 101, 255)],                 # nested, twice
            [(8, 7, 256), (2, 7, 256), (8, 7, 256), (4, 700, 300)],       # coincide (one clip twice), then a gap
            [(14, 1, 640), (4, 2, 300), (2, 3, 257), (6, 4, 255), (8, 5, 256), (0, 6, 1018), (4, 724, 300), (14, 384, 640)]]      # 8 tracks
    for a in range(4):                                                    # clip_start % 4 = a, off % 4 = 0 .. 3, on top of a long track
        c = res[a]
        ln = min(lens[c], 37)
        rows.append([(0, 1, 1001)] + [(c, 200 * j + j, ln) for j in range(4)])
        rows.append([(c, 8 * j + j, ln) for j in range(4)])               # ... and overlapping one another
    for base in (1, 4, 7):                                                # lengths 1 .. 9, three per row, alone and on top of one another
        rows.append([(0, 100 * j + (j + base) % 4, base + j) for j in range(3)] + [(2, 99, 257)])
    rows.append([(0, 5, 255), (0, 300, 256), (0, 600, 257), (0, N - 257, 257)])
    rows.append([(0, N - 1, 1), (3, N - 1, 1), (5, N - 2, 2), (0, 0, 1), (4, N - 300, 300)])        # to the last sample, from the first
    assert all(len(r) <= 8 for r in rows) and {len(r) for r in rows} >= {0, 1, 2, 3, 4, 8}
    return rows


def test_bit_equal_to_the_restatement(em, small):
    bank, data, starts = small
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    rows = edge_rows(starts, bank.lens)
    tracks = plan_of(rows)
    assert {(starts[c] % 4, o % 4) for _, c, o, _ in tracks.tolist()} == {(a, b) for a in range(4) for b in range(4)}
    assert {ln for _, _, _, ln in tracks.tolist()} >= set(range(1, 10)) | {255, 256, 257} and any(o + ln == N for _, _, o, ln in tracks.tolist())
    got = em.mix_enrollments(bank, tracks, len(rows), N)
    want = R.mix(data, starts, tracks, len(rows), N)
    assert np.isfinite(want).all() and not want[0].any() and np.array_equal(want[1], data[starts[0]:starts[0] + N])
    assert got.shape == (len(rows), N) and got.dtype == torch.float32
    for r in range(len(rows)):
        assert same_bits(got[r], want[r]), f"row {r}: {rows[r]}: first difference at sample {int(np.nonzero(got[r].cpu().numpy() != want[r])[0][0])}"
    # a row length that is no multiple of 4: the last vector is stored sample by sample
    n = N - 3
    t2 = plan_of([[(0, 0, n)], [(2, n - 257, 257), (1, n - 9, 9), (3, n - 1, 1)], [], [(4, 1, 300)]])
    assert same_bits(em.mix_enrollments(bank, t2, 4, n), R.mix(data, starts, t2, 4, n))


def test_one_row_of_30_s(em, small):
    bank, data, starts = small
    rows = [[(15, 0, N30), (0, N30 - 1024, 1024), (14, 1, 640), (2, 239999, 257)], [(15, 3, N30 - 3), (15, 0, 1)], [(0, 479000, 1000)]]
    tracks = plan_of(rows)
    got = em.mix_enrollments(bank, tracks, 3, N30)
    assert same_bits(got, R.mix(data, starts, tracks, 3, N30))
    assert float(got[2, :479000].abs().max()) == 0.0 and float(got[2, 479000:].abs().max()) > 0.0


def test_guard_bands_around_the_clips_and_the_rows(em, small):
    """The bank holds NaN in front of, between and behind its clips; the output rows sit in a strided view inside NaN guard bands."""
    bank, data, starts = small
    assert np.isnan(data[:8]).all() and np.isnan(data[-8:]).all()
    assert all(np.isnan(data[s - 1]) and np.isnan(data[s + ln]) and np.isfinite(data[s:s + ln]).all() for s, ln in zip(starts, bank.lens))
    for n, ld in ((N, N + 8), (N - 3, N + 4)):
        rows = [[(c, 0, min(ln, n))] for c, ln in enumerate(bank.lens[:15])] + [[(c, n - min(ln, n), min(ln, n)) for c, ln in enumerate(bank.lens[:8])], []]
        tracks = plan_of(rows)
        go = guarded((len(rows), n), ld, torch.float32, name="out")
        out = em.mix_enrollments(bank, tracks, len(rows), n, out=go.view)
        assert out is go.view
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), "a sample outside a clip was read"
        go.check()
        assert go.untouched_inside() == 0
        assert same_bits(out, R.mix(data, starts, tracks, len(rows), n))


def test_rows_are_independent_and_runs_reproducible(em, small):
    bank, data, starts = small
    rows = edge_rows(starts, bank.lens)[:16]
    assert len(rows) == 16
    tracks = plan_of(rows)
    both = em.mix_enrollments(bank, tracks, 16, N)
    again = em.mix_enrollments(bank, tracks, 16, N)
    assert torch.equal(both.view(torch.int32), again.view(torch.int32))
    for r in (0, 3, 5, 9, 15):
        alone = em.mix_enrollments(bank, plan_of([rows[r]]), 1, N)
        assert torch.equal(alone.view(torch.int32)[0], both.view(torch.int32)[r]), r
    # a row's place in the batch does not matter either
    flipped = em.mix_enrollments(bank, plan_of(rows[::-1]), 16, N)
    assert torch.equal(flipped.flip(0).view(torch.int32), both.view(torch.int32))


def test_capture_into_a_graph_and_replay_on_a_second_plan(em, small):
    bank, data, starts = small
    rows1 = [[(0, 3, 1000), (2, 100, 257)], [], [(4, 700, 300), (6, 1, 255), (14, 384, 640)], [(1, 5, 9)]]
    rows2 = [[(2, 0, 257), (0, 1, 1023)], [], [(8, 768, 256), (4, 2, 299), (3, 1023, 1)], [(14, 0, 640)]]       # the same shape: 2, 0, 3, 1
    t1, t2 = plan_of(rows1), plan_of(rows2)
    plan_dev = t1.cuda()
    go = guarded((4, N), N + 4, torch.float32, name="out")
    em.mix_enrollments(bank, t1, 4, N, out=go.view, plan_dev=plan_dev)      # (code objects load outside the capture; no stream of its own:
    torch.cuda.synchronize()                                                #  a new stream would shift every later test's in torch's pool)
    go.view.fill_(7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        em.mix_enrollments(bank, t1, 4, N, out=go.view, plan_dev=plan_dev)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(go.view, R.mix(data, starts, t1, 4, N))
    plan_dev.copy_(t2)                                                     # in place: the graph holds the address
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(go.view, R.mix(data, starts, t2, 4, N))
    go.check()


def test_wrapper_refusals(em, small):
    bank, data, starts = small
    E = pkg._lib.DicowError
    out = torch.full((3, 64), 5.0, device="cuda")
    for rows, match in (([[(0, 0, 65)]], "behind the row"), ([[(0, 64, 1)]], "behind the row"), ([[(1, 0, 10)]], "outside \\[1, 9\\]"),
                        ([[(0, 0, 0)]], "outside \\[1, "), ([[(0, -1, 4)]], "negative offset"), ([[(16, 0, 4)]], "clip 16"), ([[(-1, 0, 4)]], "clip -1"),
                        ([[(3, 7 * k, 1) for k in range(9)]], "more than 8 tracks")):
        with pytest.raises(E, match=match):
            em.mix_enrollments(bank, plan_of(rows), 3, 64, out=out)
    for bad, match in ((torch.tensor([[3, 0, 0, 4]]), "row 3"), (torch.tensor([[-1, 0, 0, 4]]), "row -1"), (torch.tensor([[1, 0, 0, 4], [0, 0, 0, 4]]), "consecutive")):
        with pytest.raises(E, match=match):
            em.mix_enrollments(bank, bad, 3, 64, out=out)
    ok = plan_of([[(0, 0, 10)]])
    with pytest.raises(E, match="GPU"):
        em.mix_enrollments(bank, ok, 3, 64, out=out.cpu())
    with pytest.raises(E, match="fp32"):
        em.mix_enrollments(bank, ok, 3, 64, out=out.bfloat16())
    with pytest.raises(E, match="fp32"):
        em.mix_enrollments(bank, ok, 2, 64, out=out)
    with pytest.raises(E, match="16-byte"):
        em.mix_enrollments(bank, ok, 3, 63, out=out[:, 1:])
    with pytest.raises(E, match="16-byte"):
        em.mix_enrollments(bank, ok, 3, 32, out=out[:, ::2])
    with pytest.raises(E, match="plan_dev"):
        em.mix_enrollments(bank, ok, 3, 64, out=out, plan_dev=torch.zeros(2, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(E, match="plan_dev"):
        em.mix_enrollments(bank, ok, 3, 64, out=out, plan_dev=ok)
    cpu_bank = em.EnrollmentBank.from_tensors([torch.ones(8)], ["a"], ["r"], device="cpu")
    with pytest.raises(E, match="GPU"):
        em.mix_enrollments(cpu_bank, ok, 3, 64)
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 == float(out.max())                     # nothing was launched
    none = torch.zeros(0, 4, dtype=torch.int32)
    assert em.mix_enrollments(bank, none, 0, 64).shape == (0, 64) and em.mix_enrollments(bank, none, 2, 0).shape == (2, 0)
    assert float(em.mix_enrollments(bank, torch.zeros(0, 4, dtype=torch.int32), 3, 64, out=out).abs().max()) == 0.0       # no track: zeros


# ------------------------------------------------------------------------------------------------------------------- the masks
@pytest.fixture(scope="module")
def f25(em):
    lens = R.f25_lens()
    audio = hashed_uniform("f25.audio", (sum(lens),)) * 0.25
    return R.load_f25(), R.f25_bank(em, "cuda", audio), audio.numpy()


def test_enrollment_stno_on_the_f25_tracks(em, f25):
    z, bank, _ = f25
    sup = bank.supervisions
    multi = cut = 0
    for name in R.f25_case_names(z)[::2] + ["c40", "c41"]:
        w = np.asarray(z[f"{name}.tracks"])
        tracks = R.tracks_in_samples(w[:, 0], w[:, 1], w[:, 2], w[:, 3], R.f25_options(z, name)["max_enrollment_len"])
        if tracks.shape[0] == 0:
            continue
        B = int(tracks[:, 0].max()) + 1
        targets = R.f25_rows(z, name)[0][:B]
        mix_len = [int((tracks[tracks[:, 0] == r][:, 2:].sum(axis=1)).max()) for r in range(B)]
        got = em.enrollment_stno(bank, tracks, targets, mix_len)
        assert got.shape == (B, 4, 1500) and got.dtype == torch.float32
        for r in range(B):
            assert same_bits(got[r], R.stno(sup, tracks, r, targets[r], mix_len[r])), (name, r)
        multi += int((tracks[:, 1] == 10).any())
        cut += int(any(ln < bank.lens[c] for _, c, _, ln in tracks.tolist()))
    assert multi >= 1 and cut >= 3
    # by hand: the two-speaker clip 10 (spkA [0, 4) s and [8.5, 9.5) s, spkE [3, 10) s) cut at 9 s, so that the target spkA is only partly
    # inside; beside a clip of spkB that the end of the row cuts; targets: a speaker, the unknown speaker, a speaker whose track is cut
    sr = 16000
    tracks = np.array([(0, 10, 5 * sr + 123, 9 * sr), (0, 4, 28 * sr + 1, 2 * sr - 1), (1, 10, 0, 9 * sr), (2, 13, 4 * sr + 77, 26 * sr - 77), (2, 10, 0, 10 * sr)],
                      dtype=np.int32)
    targets, mix_len = ["spkA", "-1", "spkB"], [N30, 9 * sr, N30]
    got = em.enrollment_stno(bank, tracks, targets, mix_len)
    for r in range(3):
        want = R.stno(sup, tracks, r, targets[r], mix_len[r])
        assert same_bits(got[r], want), r
        assert 0.0 < float(want[1].sum()) or targets[r] == "-1"
    assert float(got[0, 1, (5 * sr + 123 + 9 * sr) // 320 + 1:].sum()) == 0.0          # spkA's second turn ends where the track is cut
    with pytest.raises(KeyError):
        em.enrollment_stno(bank, tracks, ["spkA", "spkE", "spkC"], mix_len)                 # spkC is not in row 2's mixture
    with pytest.raises(ValueError):
        em.enrollment_stno(bank, tracks, targets, mix_len[:2])


# ------------------------------------------------------------------------------------------------------------------- wiring
def _seed(s=7):
    np.random.seed(s)
    random.seed(s)
    torch.manual_seed(s)


@pytest.fixture(scope="module")
def rows3(f25):
    from ts_asr_whisper_amd import features
    lens = [480000, 312345, 100001]
    wave, _ = features.pad_to_30s([hashed_uniform(f"enrollment_mix.row{k}", (n,)) * 0.25 for k, n in enumerate(lens)])
    return wave.cuda(), lens, ["spkA", "spkE", "spkB"], [["rec01"], ["rec77"], ["rec05", "rec12"]]


def test_front_end_equals_plan_mix_stno_logmel_by_hand(em, f25, rows3):
    from ts_asr_whisper_amd import features
    _, bank, audio = f25
    wave, lens, targets, skips = rows3
    fe = em.EnrollmentMixFrontEnd(bank, 80, num_other_speakers=2)
    _seed()
    batch = {"input_waves": wave, "wave_lengths": lens, "target_speakers": targets, "skip_recordings": skips, "labels": None}
    out = fe(batch)
    assert set(out) == {"input_features", "labels", "enrollments"} and set(out["enrollments"]) == {"input_features", "stno_mask", "attention_mask"}
    assert "target_speakers" in batch and "enrollments" not in batch                      # the caller's dict is not modified
    _seed()
    tracks, _, _, mix_len = em.plan_enrollment_mixtures(bank, targets, skips, num_other_speakers=2)
    assert sorted(set(tracks[:, 0].tolist())) == [0, 1, 2] and tracks.shape[0] >= 6
    mixed = em.mix_enrollments(bank, tracks, 3)
    assert mixed.shape == (3, N30) and same_bits(mixed, R.mix(audio, bank.starts, tracks.numpy(), 3, N30))
    for r, ln in enumerate(mix_len.tolist()):
        assert float(mixed[r, ln:].abs().max() if ln < N30 else 0.0) == 0.0 and float(mixed[r, ln - 1]) != 0.0
    enr = out["enrollments"]
    assert enr["input_features"].shape == (3, 80, 3000) and torch.equal(enr["input_features"], features.log_mel(mixed, 80))
    assert torch.equal(enr["stno_mask"], em.enrollment_stno(bank, tracks, targets, mix_len))
    am = torch.zeros(3, 3000, dtype=torch.int32)
    for r, ln in enumerate(mix_len.tolist()):
        am[r, :-(-ln // 160)] = 1
    assert enr["attention_mask"].dtype == torch.int32 and torch.equal(enr["attention_mask"].cpu(), am)
    assert torch.equal(out["input_features"], features.log_mel(wave, 80))
    # a batch without target speakers is the wave front end's alone
    plain = fe({"input_waves": wave, "wave_lengths": lens})
    assert set(plain) == {"input_features"} and torch.equal(plain["input_features"], out["input_features"])


def test_train_step_runs_from_waves_and_target_speakers(em, f25, rows3):
    from ts_asr_whisper_amd.data import synthetic_batch
    from ts_asr_whisper_amd.trainer import TrainStep
    _, bank, _ = f25
    wave, lens, targets, skips = (x[:2] for x in rows3)
    cfg = pkg.DiCoWConfig(vocab_size=512, num_mel_bins=80, d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=1,
                          decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256, max_source_positions=1500, max_target_positions=32,
                          pad_token_id=500, bos_token_id=500, eos_token_id=500, decoder_start_token_id=501, use_pre_pos_fddt=True,
                          non_target_fddt_value=0.5, use_enrollments=True, scb_layers=1)
    torch.manual_seed(0)
    models = [pkg.DiCoWForConditionalGeneration(cfg).cuda() for _ in range(3)]
    with torch.no_grad():                                                  # the cross gate starts at 0, where the enrollment does not reach the loss
        gates = [m.cross_gate.gate.fill_(0.5) for m in models[0].modules() if hasattr(m, "cross_gate")]
    assert len(gates) == 1
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    for m in models:
        m.tie_weights()
    batch = synthetic_batch(cfg, 2, 12, seed=3)
    del batch["input_features"]
    fe = em.EnrollmentMixFrontEnd(bank, 80, num_other_speakers=1)
    waves = dict(input_waves=wave, wave_lengths=lens, target_speakers=targets, skip_recordings=skips)
    _seed(11)
    loss_w = TrainStep(models[0], front_end=fe).step(dict(batch, **waves))
    _seed(11)
    built = fe(dict(waves))
    loss_f = TrainStep(models[1]).step(dict(batch, input_features=built["input_features"], enrollments=built["enrollments"]))
    assert bool(torch.isfinite(loss_w)) and float(loss_w) == float(loss_f) and torch.equal(loss_w, loss_f)
    # and the enrollment matters to the loss: another mixture, another loss
    other = dict(built["enrollments"], input_features=built["enrollments"]["input_features"].flip(0))
    assert float(TrainStep(models[2]).step(dict(batch, input_features=built["input_features"], enrollments=other))) != float(loss_f)

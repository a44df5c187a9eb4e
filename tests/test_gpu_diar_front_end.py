"""The diarization front end on the GPU (csrc/diar_front_end.hip through ts_asr_whisper_amd.diar_front_end) vs the integer restatement on
dense masks (tests/diar_front_end_ref.py, pinned to golden F24 by tests/test_host_diar_front_end.py) and vs F24 itself, which the
reference's own functions produced.  Run with `pytest -m gpu`.

Every comparison is exact: counts, window sums and starts are integers, and the STNO masks must carry the bits numpy gave the reference.
The one tolerance is the issue's: count / 1600 against the reference's fp64 activity within 1e-9 -- its 300 additions of values <= 1 err by
about 1e-11, and a count that differs by one sample is off by 6e-4.  The recordings are 60 - 70 s (the smallest that cross a 30 s edge
twice and are no multiple of a frame, a bin or a window), one of 4 minutes from F24 and one of 20 minutes for the scan's carry."""
import ast
import functools

import numpy as np
import pytest
import torch

import amd_pkg
from tests import diar_front_end_ref as R
from tests.util import guarded, hashed_uniform, load_golden

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import diar_front_end
    return diar_front_end


@pytest.fixture(scope="module")
def f24():
    return R.load_f24()


def _edge_cases():
    rng = np.random.default_rng(5)
    c = {}
    F, W = R.FRAME, R.N30
    c["edges"] = (R.N_A, [
        [(0, 1), (F * 7, F * 9), (F * 20 + 1, F * 21 - 1), (W - 5, W + 5), (2 * W - F, 2 * W), (R.N_A - 1, R.N_A)],     # first / last sample, whole
        [(F * 8, F * 8 + 1), (F * 20 + 100, F * 30 + 319), (W, W + F), (2 * W, 2 * W + 1601)],                           # frames, across 30 s edges
        [(F * 100 + 8 * j, F * 100 + 8 * j + 3) for j in range(40)] + [(W - F, W)]], [0, 1, 2, -1], [0, 1, 2])           # one frame cut 40 times
    c["no_segments"] = (R.N_B, [[], []], [0, 1, -1], [0, 1])                                                             # E = 0
    c["one_speaker"] = (R.N_A, [[(5, 100000), (99000, 300001), (800000, R.N_A)]], [0, -1], [0])
    n = R.N30 + 1601
    for S in (33, 64):                                           # the upper word of the bitmask; most speakers talk rarely, the last two a lot
        iv = R.random_intervals(rng, S, n, 0.4, 25.0)
        iv[S - 1], iv[32] = R.random_intervals(rng, 1, n, 3.0, 2.0)[0], R.random_intervals(rng, 1, n, 3.0, 2.0)[0]
        c[f"speakers{S}"] = (n, iv, [0, 31, 32, S - 1, -1], [32, S - 1])
    n = 20 * 60 * 16000 + 333                                    # 12 000 bins: the scan carries across 12 chunks of 1024
    c["twenty_minutes"] = (n, R.random_intervals(rng, 2, n, 5.0, 5.0), [1], [0, 1])
    for nb, extra in ((299, 1599), (300, 0), (301, 5)):          # under 30 s: one window = the total; exactly one window; two
        n = nb * R.BIN + extra
        c[f"bins{nb}"] = (n, [[(1000, 200000), (300000, n)], [(150000, 310000)], [(160000, 170000)]], [0], [0, 1, 2])
    return c


EDGE_CASES = _edge_cases()
F24_CASES = R.f24_cases()
ALL_CASES = dict(F24_CASES, **EDGE_CASES)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(cnt, excl) of a case from dense masks, computed once for all the tests that need it."""
    n, intervals, _, _ = ALL_CASES[name]
    return R.frame_counts(R.dense_masks(intervals, n))


def segments(D, name):
    n, intervals, _, _ = ALL_CASES[name]
    return D.SpeakerSegments.from_samples(R.as_dict(intervals), n)


def bits(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).view(np.int32)


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_counts_and_stno_bit_equal(D, f24, name):
    n, intervals, stno_targets, _ = ALL_CASES[name]
    segs = segments(D, name)
    cnt_r, excl_r = restated(name)
    cnt, excl = D.frame_counts(segs)
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == cnt_r.shape == (len(intervals), R.t_total(n))
    assert np.array_equal(cnt.cpu().numpy(), cnt_r) and np.array_equal(excl.cpu().numpy(), excl_r)
    K, T = len(stno_targets), segs.T_total
    ld = T + 24                                                   # rows longer than T_total inside NaN guard bands
    g = guarded((K, 4, T), ld, torch.float32, strides=(4 * ld, ld, 1), name="stno")
    out = D.stno_masks(segs, stno_targets, out=g.view)
    assert out is g.view and g.untouched_inside() == 0
    g.check()
    plain = D.stno_masks(segs, stno_targets)                      # the allocating call: same bits in a contiguous tensor
    assert plain.is_contiguous() and np.array_equal(bits(plain), bits(out.contiguous()))
    pick = R.stno_pick(T)
    for k, t in enumerate(stno_targets):
        want = R.stno(cnt_r, t)
        assert np.array_equal(bits(out[k].contiguous()), want.view(np.int32)), (name, t)
        if name in F24_CASES:                                     # and the reference's own output
            assert np.array_equal(bits(out[k].contiguous())[:, pick], np.asarray(f24[f"{name}.stno.{t}"]).view(np.int32)), (name, t)
    tail = -(-n // R.FRAME)                                       # frames that hold no audio: pure silence
    if tail < T:
        assert bool((plain[:, 0, tail:] == 1).all()) and bool((plain[:, 1:, tail:] == 0).all())
    assert bool((plain.sum(1) - 1).abs().max() < 1e-6)


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_enrollment_windows_are_the_first_exact_maximum(D, f24, name):
    n, intervals, _, enr_targets = ALL_CASES[name]
    segs = segments(D, name)
    cnt_r, excl_r = restated(name)
    start, count, fb, weights = D.select_enrollment_windows(segs, enr_targets, return_weights=True)
    plain = D.select_enrollment_windows(segs, enr_targets)
    assert all(t.dtype == torch.int32 for t in (start, count, fb, weights)) and tuple(weights.shape) == (len(enr_targets), segs.n_windows)
    assert all(torch.equal(a, b) for a, b in zip(plain, (start, count, fb)))
    start, count, fb, weights = start.tolist(), count.tolist(), fb.tolist(), weights.cpu().numpy()
    for k, t in enumerate(enr_targets):
        s_r, c_r, fb_r, w_r = R.enrollment(cnt_r, excl_r, t, n)
        assert (start[k], count[k], fb[k]) == (s_r, c_r, fb_r), (name, t)
        assert np.array_equal(weights[k], w_r), (name, t)
        assert count[k] == weights[k].max() and start[k] == int(np.argmax(weights[k]))            # a plateau gives its first index
        if name in F24_CASES:
            ref_start, ref_act, ref_fb, _ = f24[f"{name}.enr.{t}"]
            assert fb[k] == int(ref_fb) and abs(count[k] / 1600 - ref_act) <= 1e-9, (name, t, count[k] / 1600, ref_act)
            if f"{name}.{t}" in f24["unique"].tolist():
                assert start[k] == int(ref_start), (name, t)


def test_edge_cases_cover_what_they_are_there_for(D):
    assert segments(D, "no_segments").E == 0
    s, c, fb = (v.tolist() for v in D.select_enrollment_windows(segments(D, "no_segments")))
    assert (s, c, fb) == ([0, 0], [0, 0], [1, 1])                 # nobody ever talks: both passes are empty, the first window it is
    assert int(segments(D, "speakers64").active.max()) >> 63 == 1 and int(segments(D, "speakers33").active.max()) >> 32 == 1
    assert any(R.enrollment(*restated(n), t, ALL_CASES[n][0])[2] == 1 for n in ("never_alone", "s9") for t in ALL_CASES[n][3])
    best = [R.enrollment(*restated(n), t, F24_CASES[n][0])[3] for n in F24_CASES for t in F24_CASES[n][3]]
    assert sum(int((w == w.max()).sum() > 1) for w in best) >= 3                                 # plateaus
    assert [segments(D, f"bins{nb}").n_windows for nb in (299, 300, 301)] == [1, 1, 2]
    cnt_r, _ = restated("edges")
    assert cnt_r[2, 100] == 120 and cnt_r[0, 0] == 1 and cnt_r[0, 7] == 320 and cnt_r[0, 20] == 318            # 40 x 3 samples in one frame
    assert segments(D, "twenty_minutes").n_bins > 11 * 1024


def test_results_are_reproducible_and_independent_of_the_other_targets(D):
    n, intervals, _, _ = ALL_CASES["s9"]
    runs = []
    for _ in range(2):
        segs = segments(D, "s9")                                  # a new object: nothing cached
        runs.append((D.frame_counts(segs), D.stno_masks(segs, list(range(8))), D.select_enrollment_windows(segs, list(range(8)), return_weights=True)))
    (c0, m0, e0), (c1, m1, e1) = runs
    assert torch.equal(c0[0], c1[0]) and torch.equal(c0[1], c1[1]) and np.array_equal(bits(m0), bits(m1))
    assert all(torch.equal(a, b) for a, b in zip(e0, e1))
    segs = segments(D, "s9")
    for t in (0, 4, 7):
        alone = D.stno_masks(segs, [t])
        assert np.array_equal(bits(alone[0]), bits(m0[t]))
        ea = D.select_enrollment_windows(segs, [t], return_weights=True)
        assert all(torch.equal(a[0], b[t]) for a, b in zip(ea, e0))
    again = D.stno_masks(segs, [4, 4, -1, 4])                     # a target asked for twice is computed twice, into its own rows
    assert np.array_equal(bits(again[0]), bits(m0[4])) and np.array_equal(bits(again[3]), bits(m0[4]))


def test_wrapper_refuses_what_the_kernels_cannot_take(D):
    segs = segments(D, "s2")
    T = segs.T_total
    for bad in (torch.empty(2, 4, T, dtype=torch.float64, device="cuda"), torch.empty(2, 4, T + 1, device="cuda"), torch.empty(2, 4, T),
                torch.empty(2, T, 4, device="cuda").transpose(1, 2), torch.empty(4, 4, T, device="cuda")[::2]):
        with pytest.raises(pkg._lib.DicowError):
            D.stno_masks(segs, [0, 1], out=bad)
    assert tuple(D.stno_masks(segs, []).shape) == (0, 4, T)
    with pytest.raises(pkg._lib.DicowError, match="samples"):
        D.MeetingFrontEnd(80).prepare(torch.zeros(1000, device="cuda"), segs)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _toy(se):
    """A toy (SE-)DiCoW with golden F8's dimensions and Whisper's window: 1500 encoder positions."""
    d = ast.literal_eval(str(load_golden("f8_e2e_se")["cfg"]))
    d.update(max_source_positions=1500, bos_token_id=d["pad_token_id"], use_enrollments=se, scb_layers=1 if se else None)
    cfg = pkg.DiCoWConfig(**d)
    torch.manual_seed(24)
    model = pkg.DiCoWForConditionalGeneration(cfg).cuda().eval()
    model.tie_weights()
    no_ts, pad = 399, 499

    class Tok:
        prefix_tokens = [cfg.decoder_start_token_id, 7]
        pad_token_id = pad

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 7}

    model.set_tokenizer(Tok())
    from types import SimpleNamespace
    gc = SimpleNamespace(eos_token_id=5, pad_token_id=pad, no_timestamps_token_id=no_ts, max_initial_timestamp_index=50,
                         decoder_start_token_id=cfg.decoder_start_token_id)
    return model, cfg, gc


def _meeting():
    n = R.N_B                                                     # 70 s + 7 samples, three speakers
    rng = np.random.default_rng(70)
    intervals = R.random_intervals(rng, 3, n, 3.0, 3.0)
    wave = hashed_uniform("f24.meeting.wave", (n,)) * 0.1
    return n, intervals, wave


def _by_hand(n, intervals, wave, targets, n_mels, se):
    """The batch from the numpy restatement on dense masks and a log-mel per row."""
    from ts_asr_whisper_amd import features
    cnt, excl = R.frame_counts(R.dense_masks(intervals, n))
    T = R.t_total(n)
    stno = torch.from_numpy(np.stack([R.stno(cnt, t) for t in targets])).cuda()
    padded = torch.zeros(len(targets), T * R.FRAME)
    padded[:, :n] = wave
    am = torch.zeros(len(targets), 2 * T, dtype=torch.int32)
    am[:, :-(-n // 160)] = 1
    batch = {"input_features": torch.cat([features.log_mel(padded[k:k + 1].cuda(), n_mels) for k in range(len(targets))]),
             "attention_mask": am.cuda(), "stno_mask": stno}
    if se:
        rows, masks = [], []
        for k, t in enumerate(targets):
            start = R.enrollment(cnt, excl, t, n)[0]
            clip = torch.zeros(1, R.N30)
            piece = wave[R.BIN * start:R.BIN * start + R.N30]
            clip[0, :piece.numel()] = piece
            rows.append(features.log_mel(clip.cuda(), n_mels))
            masks.append(stno[k, :, 5 * start:5 * start + R.T30])
        batch["enrollments"] = {"input_features": torch.cat(rows), "stno_mask": torch.stack(masks),
                                "attention_mask": torch.ones(len(targets), 2 * R.T30, dtype=torch.int32, device="cuda")}
    return batch


@pytest.mark.parametrize("se", [True, False], ids=["se_dicow", "dicow"])
def test_prepare_feeds_generate_like_a_batch_assembled_by_hand(D, se):
    model, cfg, gc = _toy(se)
    n, intervals, wave = _meeting()
    segs = D.SpeakerSegments.from_samples(R.as_dict(intervals), n)
    targets = [0, 1, 2] if se else [0, 2, -1]
    batch = D.MeetingFrontEnd(cfg.num_mel_bins, use_enrollments=se).prepare(wave.cuda(), segs, targets)
    hand = _by_hand(n, intervals, wave, targets, cfg.num_mel_bins, se)
    assert set(batch) == set(hand) and batch["input_features"].stride(0) == 0              # one log-mel, shared
    for k in ("input_features", "stno_mask"):
        assert np.array_equal(bits(batch[k]), bits(hand[k])), k
    assert torch.equal(batch["attention_mask"], hand["attention_mask"])
    if se:
        assert set(batch["enrollments"]) == set(hand["enrollments"])
        shapes = {"input_features": (3, cfg.num_mel_bins, 3000), "stno_mask": (3, 4, 1500)}
        for k in ("input_features", "stno_mask"):
            assert tuple(batch["enrollments"][k].shape) == shapes[k]
            assert np.array_equal(bits(batch["enrollments"][k]), bits(hand["enrollments"][k])), k
        assert torch.equal(batch["enrollments"]["attention_mask"], hand["enrollments"]["attention_mask"])
    got = model.generate(**batch, generation_config=gc, max_new_tokens=8)
    segs_got = model.last_segments
    want = model.generate(**hand, generation_config=gc, max_new_tokens=8)
    assert torch.equal(got, want) and got.shape[0] == 3
    assert [[s["tokens"] for s in r] for r in segs_got] == [[s["tokens"] for s in r] for r in model.last_segments]

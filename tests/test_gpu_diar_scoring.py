"""dicow_diar_score (csrc/diar_score.hip) and the diarization metrics of ts_asr_whisper_amd.diar_scoring on the GPU against the two
oracles of tests/diar_score_ref.py.  Every comparison is EXACT equality.  Every launch made through `launch` writes its int64 rows into an
output inside the guard bands of tests/util.py::guarded (as int32 pairs) and gets a workspace of exactly dicow_diar_score_ws_bytes bytes
inside guard bands of its own.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import diar_score_ref as R
from tests.util import guarded

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, diar_scoring as D  # noqa: E402
from ts_asr_whisper_amd.diar_front_end import SpeakerSegments  # noqa: E402

CHUNK, OUT = L.DIAR_SCORE_CHUNK, L.DIAR_SCORE_OUT_WORDS


def launch(problems, chunk=0):
    """-> int64 [P, OUT] on the CPU, after checking the guard bands of the output and of the workspace."""
    b, a, u, pt = D.pack_problems(problems)
    t = D.table_args(b, a, u, pt, chunk)
    nbytes = L.lib().dicow_diar_score_ws_bytes(*t)
    assert nbytes > 0 and nbytes % 8 == 0, L.lib().dicow_last_error()
    go = guarded((len(problems), 2 * OUT), 2 * OUT, torch.int32, name="out")
    gw = guarded((nbytes // 4,), 64, torch.int32, name="ws")
    L.call("dicow_diar_score", *t, go.view.data_ptr(), gw.view.data_ptr(), nbytes, L.stream())
    torch.cuda.synchronize()
    go.check()
    gw.check()
    assert go.untouched_inside() == 0                                      # every output word is written, the zeros too
    return go.view.contiguous().view(torch.int64).cpu().numpy().reshape(len(problems), OUT)


def as_counts(row, problem):
    got = D.split_counts(row, problem[0][2], problem[1][2])
    full = row[:4096].reshape(64, 64)
    assert int(full.sum()) == int(got["C"].sum()) and int(row[4096:4224].sum()) == int(got["R"].sum() + got["H"].sum())   # zeros behind S
    assert row[4229:].tolist() == [0, 0, 0]
    return got


def check(problems, wants, chunk=0):
    rows = launch(problems, chunk)
    for k, (p, w) in enumerate(zip(problems, wants)):
        got = as_counts(rows[k], p)
        assert R.same(got, w), (k, {key: (got[key], w[key]) for key in R.SCALARS})
    return rows


def n_regions(p):
    ref, hyp, uns, _ = p
    M = sum(len(t[1]) + 1 for t in (ref, hyp) if len(t[1])) + 2 * len(np.asarray(uns if uns is not None else []).reshape(-1, 2))
    return max(M - 1, 0)


@pytest.mark.parametrize("Sr,Sh", [(1, 1), (2, 3), (64, 1), (1, 64), (64, 64)])
def test_counts_equal_the_dense_oracle_for_every_speaker_count(Sr, Sh):
    rng = np.random.default_rng(100 * Sr + Sh)
    n = 3000
    ref = R.random_table(rng, Sr, 50, n, top_bit=True)
    hyp = R.random_table(rng, Sh, 37, n, top_bit=True)
    if Sr == 64:
        assert int(ref[1][0]) >> 63 == 1                                   # bit 63 is an ordinary speaker
    uns = R.random_unscored(rng, 4, n)
    problems = [(ref, hyp, uns, False), (ref, hyp, uns, True), (ref, hyp, None, False), (hyp, ref, uns, True)]
    wants = [R.dense_counts(r, h, u, s, n) for r, h, u, s in problems]
    assert wants[0]["total"] > 0 and not R.same(wants[0], wants[2])
    if Sr > 1:
        assert not R.same(wants[0], wants[1])
    check(problems, wants)


def test_empty_tables_and_coincident_endpoints():
    rng = np.random.default_rng(7)
    n = 500
    ref = R.random_table(rng, 3, 20, n)
    empty3, empty1 = R.random_table(rng, 3, 0, n), R.random_table(rng, 1, 0, n)
    uns = R.random_unscored(rng, 3, n)
    # a hypothesis on the reference's own bounds (every third), unscored intervals that start and end on bounds
    same_b = (ref[0][::3].copy(), rng.integers(0, 4, len(ref[0][::3]) - 1).astype(np.uint64), 2)
    on_b = np.array([(ref[0][2], ref[0][5]), (ref[0][5], ref[0][6]), (ref[0][9], ref[0][12])], np.int64)
    problems = [(ref, empty1, uns, False), (empty3, ref, uns, False), (empty3, empty1, uns, True), (empty3, empty1, None, False),
                (ref, same_b, on_b, False), (ref, ref, on_b, True), (same_b, ref, None, False)]
    wants = [R.dense_counts(r, h, u, s, n) for r, h, u, s in problems]
    assert wants[0]["missed"] == wants[0]["total"] > 0 and wants[1]["false_alarm"] > 0 and wants[1]["total"] == 0
    assert wants[2]["scored"] == 0 and wants[5]["missed"] == 0 and wants[5]["false_alarm"] == 0
    check(problems, wants)


@pytest.mark.parametrize("regions", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK])
def test_region_counts_around_the_chunk(regions):
    rng = np.random.default_rng(regions)
    n = 8000
    Er, Eh = regions - 11, 10
    rb = np.sort(rng.choice(np.arange(0, n + 1, 2), Er + 1, replace=False)).astype(np.int64)           # even / odd: no coincidence
    hb = np.sort(rng.choice(np.arange(1, n + 1, 2), Eh + 1, replace=False)).astype(np.int64)
    ref = (rb, rng.integers(0, 8, Er).astype(np.uint64), 3)
    hyp = (hb, rng.integers(0, 4, Eh).astype(np.uint64), 2)
    problems = [(ref, hyp, None, False), (ref, hyp, None, True)]
    assert n_regions(problems[0]) == regions
    wants = [R.dense_counts(r, h, u, s, n) for r, h, u, s in problems]
    check(problems, wants)


def _meeting(rng, S, n, k=6, names="spk"):
    out = {}
    for s in range(S):
        starts = rng.integers(0, n - 2000, k)
        out[f"{names}{s}"] = [(int(a), int(a + rng.integers(500, 12000))) for a in starts]
    return SpeakerSegments(out, n)


@pytest.mark.parametrize("collar", [0.0, 0.25, 0.5, 30.0])
def test_collars_and_skip_overlap_on_meetings(collar):
    rng = np.random.default_rng(11)
    ref, hyp = _meeting(rng, 4, 160000), _meeting(rng, 3, 150000, names="h")       # different lengths: nothing is active behind either end
    uns = D.unscored_intervals(ref, collar)
    problems = [(ref, hyp, uns, False), (ref, hyp, uns, True)]
    wants = [R.dense_counts(R.table_of(r), R.table_of(h), u, s, 200000) for r, h, u, s in problems]
    if collar == 30.0:
        assert wants[0]["total"] == 0 and wants[0]["scored"] == 0          # the collar swallows all speech
    else:
        assert 0 < wants[1]["total"] <= wants[0]["total"] and (collar > 0.0 or wants[1]["total"] < wants[0]["total"])
    rows = launch(problems)
    for k in range(2):
        assert R.same(as_counts(rows[k], (R.table_of(ref), R.table_of(hyp))), wants[k]), k
    e = D.error_from_counts(D.split_counts(rows[0], ref.S, hyp.S))
    assert e == R.der(wants[0])
    if collar == 30.0:
        assert e["total"] == 0.0 and e["diarization error rate"] == 0.0


def test_positions_near_two_to_the_forty():
    rng = np.random.default_rng(3)
    top = L.DIAR_SCORE_MAX_TICK
    lo = top - 6000
    ref = R.random_table(rng, 5, 60, top, lo=lo)
    hyp = R.random_table(rng, 64, 45, top, lo=lo, top_bit=True)
    ref[0][-1] = hyp[0][-1] = top                                          # the last legal tick, and a coincidence
    far = (np.array([0, 1, top - 1, top], np.int64), np.array([1, 3, 2], np.uint64), 2)         # one region of almost 2^40 ticks
    uns = R.random_unscored(rng, 3, 6000) + lo
    problems = [(ref, hyp, uns, False), (ref, hyp, uns, True), (far, far, None, False), (far, ref, np.array([(5, top - 3000)]), False)]
    wants = [R.sweep_counts(r, h, u, s) for r, h, u, s in problems]
    assert wants[2]["total"] == 2 * (top - 2) + 2 and wants[2]["C"][0][1] == top - 2 and wants[3]["scored"] > 1000
    check(problems, wants)


def test_bits_do_not_depend_on_the_chunk_the_neighbours_or_the_run():
    rng = np.random.default_rng(21)
    n = 4000
    mine = (R.random_table(rng, 6, 700, n), R.random_table(rng, 7, 500, n), R.random_unscored(rng, 9, n), False)
    assert n_regions(mine) > CHUNK
    others = []
    for k in range(15):
        E = [0, 1, 3, 40, 900, 2500][k % 6]
        others.append((R.random_table(rng, 1 + 9 * (k % 8), E, n), R.random_table(rng, 64 - 4 * k, [5, 0, 1300, 2][k % 4], n),
                       R.random_unscored(rng, k % 4, n), bool(k % 2)))
    want = R.dense_counts(*mine[:3], False, n)
    alone = check([mine], [want])[0]
    crowd = launch(others[:7] + [mine] + others[7:])
    assert np.array_equal(crowd[7], alone)
    assert np.array_equal(launch(others[:7] + [mine] + others[7:]), crowd)                             # two runs
    for chunk in (200, 129, 64):
        assert np.array_equal(launch([others[4], mine], chunk)[1], alone), chunk
    for k in (3, 4, 10):                                                   # the neighbours are right too
        assert R.same(as_counts(crowd[k if k < 7 else k + 1], others[k]), R.dense_counts(*others[k][:3], others[k][3], n)), k
    # the wrapper: its own workspace, a caller's output
    out = torch.full((2, OUT), -1, dtype=torch.int64, device="cuda")
    got = D.diar_score_counts([others[4], mine], out=out)
    assert got is out and np.array_equal(out[1].cpu().numpy(), alone)


def _index_mapping(ref, hyp, names):
    return {ref.speakers.index(r): hyp.speakers.index(h) for h, r in names.items()}


@pytest.mark.parametrize("seed", range(3))
def test_metrics_end_to_end_equal_the_dense_oracle(seed):
    rng = np.random.default_rng(40 + seed)
    pairs = [(_meeting(rng, int(rng.integers(1, 6)), 48000, k=4), _meeting(rng, int(rng.integers(1, 6)), 50000, k=4, names="h")) for _ in range(3)]
    for collar, skip in ((0.0, False), (0.25, True)):
        wants = [R.dense_counts(R.table_of(r), R.table_of(h), D.unscored_intervals(r, collar), skip, 60000) for r, h in pairs]
        res = D.score_diarizations(pairs, collar=collar, skip_overlap=skip)
        assert len(res["recordings"]) == len(res["mappings"]) == 3
        for (r, h), w, rec, names in zip(pairs, wants, res["recordings"], res["mappings"]):
            d = R.der(w)                                                    # `correct` is the brute-force maximum
            assert {k: rec[k] for k in d} == d
            m = _index_mapping(r, h, names)
            assert sum(int(w["C"][i][j]) for i, j in m.items()) == R.best_correct(w["C"]) and all(w["C"][i][j] > 0 for i, j in m.items())
            j = R.jer(w, m)
            assert {k: rec[k] for k in j} == j
            assert rec["speaker count error"] == abs(r.S - h.S)
            assert D.diarization_error(r, h, collar, skip) == d
            if not skip:
                names1 = D.optimal_mapping(r, h, collar)
                assert D.jaccard_error(r, h, collar) == R.jer(w, _index_mapping(r, h, names1))
        c = res["corpus"]
        tot = {k: sum(w[k] for w in wants) for k in ("total", "missed", "false_alarm", "matched")}
        conf = tot["matched"] - sum(R.best_correct(w["C"]) for w in wants)
        assert c["DER"] == (tot["missed"] + tot["false_alarm"] + conf) / tot["total"] and c["Conf"] == conf / tot["total"]
        assert c["Miss"] == tot["missed"] / tot["total"] and c["FA"] == tot["false_alarm"] / tot["total"]
        assert c["JER"] == sum(rec["speaker error"] for rec in res["recordings"]) / sum(rec["speaker count"] for rec in res["recordings"])
        assert c["MSCE"] == sum(abs(r.S - h.S) for r, h in pairs) / 3


def test_a_renamed_and_jittered_reference_scores_zero_and_maps_back():
    rng = np.random.default_rng(9)
    names = ["anna", "ben", "cleo", "dov"]
    ref, t = {k: [] for k in names}, 16000
    for q in range(12):                                                    # 3 s turns; every third one overlaps its successor by 1 s
        ref[names[(q * 3 + q // 4) % 4]].append((t, t + 48000))
        t += 32000 if q % 3 == 2 else 56000
    n = t + 64000
    ref = SpeakerSegments(ref, n)
    perm = {"anna": "s2", "ben": "s0", "cleo": "s3", "dov": "s1"}
    jit = lambda: int(rng.integers(-4800, 4801))                            # 0.3 s
    hyp = SpeakerSegments({perm[k]: [(a + jit(), b + jit()) for a, b in v] for k, v in ref.intervals.items()}, n + 1000)
    e = D.diarization_error(ref, hyp, collar=1.0)
    assert e["diarization error rate"] == 0.0 and e["missed detection"] == e["false alarm"] == e["confusion"] == 0.0 and e["correct"] == e["total"] > 0
    assert D.diarization_error(ref, hyp, collar=0.0)["diarization error rate"] > 0.0
    mapping = D.optimal_mapping(ref, hyp, collar=1.0)
    assert mapping == {v: k for k, v in perm.items()}
    back = hyp.relabelled(mapping)
    assert back.speakers == ref.speakers
    assert D.jaccard_error(ref, back, collar=1.0) == {"speaker error": 0.0, "speaker count": 4, "jaccard error rate": 0.0}
    res = D.score_diarizations([(ref, back), (ref, hyp)], collar=1.0)
    assert res["corpus"] == {"MSCE": 0.0, "JER": 0.0, "DER": 0.0, "Miss": 0.0, "FA": 0.0, "Conf": 0.0}
    assert res["mappings"][0] == {k: k for k in names}

"""dicow_bootstrap_sums on the GPU against the oracle of tests/bootstrap_ref.py: `out` EQUALS the oracle under every plan at the smallest
shapes where the kernel can go wrong -- the Philox block of four slots, the wave, the workgroup, the staging limit of the LDS plans, every
register bucket of C, a row pitch above C and a table that is not 16-byte aligned, the carry of the replicate number into the third counter
word, a seed with high bits, strata of one unit and strata off the multiples of four, entries near +-2^40 -- in both modes; a call cut into
chunks, a graph replay, the swap invariant, and the statistics end to end against the same host code on the oracle's sums."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import bootstrap_ref as B

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, significance as S  # noqa: E402

pytestmark = pytest.mark.gpu

PLANS = (0, _lib.BOOT_LANE_LDS, _lib.BOOT_WAVE_LDS, _lib.BOOT_WAVE_L2)
NS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)
RS = (1, 63, 64, 65, 257)
SEED = (0xdeadbeef << 32) | 7


def make_table(n, C, seed):
    """Entries near +-2^40 (n * 2^41 stays far below 2^62), a few of them exactly at the ends of the range."""
    t = np.random.default_rng(seed).integers(-(1 << 40), (1 << 40) + 1, (n, C))
    t[0, 0], t[-1, -1] = -(1 << 40), 1 << 40
    return t


def fits(n, C):
    return n * C * 8 <= _lib.BOOT_LDS_BYTES


def run(table, R, plan, pitch=None, shift=0, **kw):
    """The launch on a device copy of `table` with row pitch `pitch` that starts `shift` elements into its buffer."""
    n, C = table.shape
    pitch = C if pitch is None else pitch
    buf = torch.full((n * pitch + shift + 2,), 1 << 50, dtype=torch.int64, device="cuda")
    view = buf[shift:shift + n * pitch].view(n, pitch)[:, :C]
    view.copy_(torch.from_numpy(table))
    return S.bootstrap_sums(view, R, plan=plan, **kw).cpu().numpy()


def check_all_plans(table, R, mode="resample", offsets=None, seed=SEED, first=0, **kw):
    n, C = table.shape
    want = B.sums_np(table, R, seed, offsets, mode, first)
    for plan in PLANS:
        if plan in (_lib.BOOT_LANE_LDS, _lib.BOOT_WAVE_LDS) and not fits(n, C):
            with pytest.raises(_lib.DicowError, match="DICOW_BOOT_LDS_BYTES"):
                run(table, R, plan, seed=seed, strata=offsets, mode=mode, first_replicate=first, **kw)
            continue
        got = run(table, R, plan, seed=seed, strata=offsets, mode=mode, first_replicate=first, **kw)
        assert got.shape == want.shape and (got == want).all(), (n, C, R, mode, plan, kw)


@pytest.mark.parametrize("C", [1, 2, 5, 32])
def test_resample_equals_the_oracle_under_every_plan(C):
    for n in NS:
        table = make_table(n, C, 100 * C + n)
        for R in RS:
            check_all_plans(table, R)


@pytest.mark.parametrize("C", [2, 6])
def test_swap_equals_the_oracle_under_every_plan(C):
    for n in NS:
        table = make_table(n, C, 200 * C + n)
        for R in RS:
            check_all_plans(table, R, mode="swap")
    # swap mode ignores strata
    table = make_table(65, C, 7)
    assert (run(table, 9, 0, mode="swap", strata=[0, 1, 6, 7, 64, 65], seed=5) == B.sums_np(table, 9, 5, None, "swap")).all()


@pytest.mark.parametrize("C", [1, 2, 5, 32])
def test_the_staging_limit_of_the_lds_plans_and_one_unit_more(C):
    limit = _lib.BOOT_LDS_BYTES // (8 * C)
    assert fits(limit, C) and not fits(limit + 1, C)
    for n in (limit, limit + 1):
        table = make_table(n, C, n)
        check_all_plans(table, 5)
        if C % 2 == 0:
            check_all_plans(table, 5, mode="swap")
    lib = _lib.lib()
    assert lib.dicow_bootstrap_plan(limit, C) != _lib.BOOT_WAVE_L2 and lib.dicow_bootstrap_plan(limit + 1, C) == _lib.BOOT_WAVE_L2


@pytest.mark.parametrize("C", [1, 2, 5, 6, 16, 32])
def test_row_pitch_above_c_and_unaligned_tables(C):
    """pitch C + 3 or C + 2 and a buffer offset of one element: the 16-byte row reads and the 16-byte staging are taken only where they may be."""
    for n in (5, 65, 257):
        table = make_table(n, C, 300 * C + n)
        for pitch, shift in ((C + 3, 0), (C + 2, 0), (C + 2, 1), (C, 1), (C, 0)):
            check_all_plans(table, 65, pitch=pitch, shift=shift)
            if C % 2 == 0:
                check_all_plans(table, 65, mode="swap", pitch=pitch, shift=shift)


def test_replicate_numbers_across_the_carry_and_seeds_with_high_bits():
    table = make_table(65, 5, 1)
    for first in ((1 << 32) - 1, (1 << 32) - 33, (1 << 64) - 3, 1 << 40):
        check_all_plans(table, 65, first=first)
        check_all_plans(make_table(65, 6, 2), 65, mode="swap", first=first)
    for seed in (0, 1234, 1 << 63, (1 << 64) - 1):
        check_all_plans(table, 7, seed=seed)
    # the words differ from seed to seed and from replicate to replicate
    a, b = run(table, 64, 0, seed=1), run(table, 64, 0, seed=1 << 32)
    assert (a != b).any() and len({tuple(r) for r in a.tolist()}) == 64


def test_strata_of_one_unit_and_boundaries_off_the_multiples_of_four():
    offsets = [0, 1, 6, 7, 64, 65]
    for C in (1, 4, 5):
        table = make_table(65, C, 400 + C)
        for R in (1, 65, 257):
            check_all_plans(table, R, offsets=offsets)
    # every unit its own stratum: each replicate is the column total; many strata: the search for a slot's stratum
    table = make_table(257, 2, 9)
    check_all_plans(table, 3, offsets=list(range(258)))
    assert (run(table, 3, 0, strata=list(range(258))) == table.sum(0)).all()
    check_all_plans(make_table(1000, 2, 10), 5, offsets=[0] + sorted(np.random.default_rng(3).choice(np.arange(1, 1000), 300, replace=False).tolist()) + [1000])


def test_one_call_equals_its_chunks():
    table = make_table(257, 5, 11)
    for mode, t in (("resample", table), ("swap", make_table(257, 6, 12))):
        whole = run(t, 257, 0, seed=SEED, mode=mode, first_replicate=(1 << 32) - 120)
        parts = [run(t, r, plan, seed=SEED, mode=mode, first_replicate=(1 << 32) - 120 + at)
                 for at, r, plan in ((0, 100, _lib.BOOT_WAVE_L2), (100, 100, _lib.BOOT_LANE_LDS), (200, 57, _lib.BOOT_WAVE_LDS))]
        assert (np.concatenate(parts) == whole).all()
        assert (whole == B.sums_np(t, 257, SEED, None, mode, (1 << 32) - 120)).all()
    # no replicates: an empty result, nothing written
    out = torch.empty((0, 5), dtype=torch.int64, device="cuda")
    assert S.bootstrap_sums(torch.from_numpy(table).cuda(), 0, out=out) is out


def test_graph_replay_equals_the_eager_call():
    offsets = [0, 1, 6, 7, 64, 65]
    for n, C, mode, strata in ((65, 5, "resample", offsets), (65, 6, "swap", None), (2000, 8, "resample", None)):
        table = torch.from_numpy(make_table(n, C, 13)).cuda()
        out = torch.empty((257, C), dtype=torch.int64, device="cuda")
        launch = lambda: S.bootstrap_sums(table, 257, seed=SEED, strata=strata, mode=mode, first_replicate=5, out=out)      # noqa: E731
        want = launch().cpu().numpy().copy()                                     # (code objects load and the strata upload outside the capture)
        assert (want == B.sums_np(table.cpu().numpy(), 257, SEED, strata, mode, 5)).all()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch()
        for _ in range(2):
            out.fill_(7)
            graph.replay()
            assert (out.cpu().numpy() == want).all()


def test_swap_keeps_every_units_counts_in_the_total():
    table = make_table(300, 6, 14)
    out = run(table, 257, 0, mode="swap", seed=3)
    assert (out[:, :3] + out[:, 3:] == (table[:, :3] + table[:, 3:]).sum(0)).all()
    assert len({tuple(r) for r in out.tolist()}) == 257


def test_wrapper_refusals_on_the_device():
    t = torch.ones((8, 4), dtype=torch.int64, device="cuda")
    for bad, word in ((dict(table=t.int()), "int64"), (dict(table=t.t()), "stride"), (dict(table=t[:, ::2]), "stride"), (dict(table=t[0]), "int64"),
                      (dict(table=t[:, :3], mode="swap"), "odd"), (dict(table=t, mode="shuffle"), "mode"), (dict(table=t, strata=[0, 4, 4, 8]), "empty"),
                      (dict(table=t, plan=9), "plan=9"), (dict(table=t, out=torch.empty((3, 3), dtype=torch.int64, device="cuda")), "out must"),
                      (dict(table=t * (1 << 59)), "2\\^62"), (dict(table=-t * (1 << 59)), "2\\^62")):
        kw = dict(replicates=3)
        kw.update(bad)
        with pytest.raises(_lib.DicowError, match=word):
            S.bootstrap_sums(**kw)
    assert S.bootstrap_sums(t * ((1 << 59) - 1), 2).tolist() == [[8 * ((1 << 59) - 1)] * 4] * 2


def test_a_system_against_itself():
    rng = np.random.default_rng(15)
    den = rng.integers(50, 4000, 40)
    num = (den * rng.random(40) * 0.4).astype(np.int64)
    st = S.compare_ratios(num, den, num, den, replicates=1000, seed=2)
    assert st["delta"] == 0.0 and (st["lo"], st["hi"]) == (0.0, 0.0) and st["p_value"] == 1.0 and st["prob_a_better"] == 0.5 and st["se"] == 0.0
    assert st["rate_a"] == st["rate_b"] == int(num.sum()) / int(den.sum()) and st["replicates"] == 1000 and st["undefined"] == 0


def test_statistics_end_to_end_equal_the_host_rules_on_the_oracles_sums():
    rng = np.random.default_rng(16)
    # --- session dicts of two systems over the same 23 sessions, two corpora
    n, metrics = 23, ["cp_wer", "tcp_wer", "orc_wer"]
    length = rng.integers(100, 5000, n)
    corpus = ["ami" if k % 3 else "nsf" for k in range(n)]

    def system(rate):
        rows = []
        for k in range(n):
            row = {"session_id": f"s{k}"}
            for p in ("cp", "tcp", "orc"):
                row[f"{p}_errors"], row[f"{p}_length"] = int(length[k] * rate * rng.random()), int(length[k])
                row[f"{p}_wer"] = row[f"{p}_errors"] / row[f"{p}_length"]
            rows.append(row)
        return rows

    a, b = system(0.30), system(0.33)
    cols = lambda rows: np.asarray([[r[f"{p}_{k}"] for p in ("cp", "tcp", "orc") for k in ("errors", "length")] for r in rows], np.int64)  # noqa: E731
    # unstratified intervals
    got = S.session_metric_intervals(a, metrics, replicates=999, alpha=0.1, seed=4)
    sums = B.sums_np(cols(a), 999, 4)
    agg = pkg.aggregate_session_metrics(a, metrics)
    for m, p in enumerate(("cp", "tcp", "orc")):
        st = S.ratio_statistics(sums[:, 2 * m:2 * m + 2], 0.1)
        assert (got[f"{p}_wer_lo"], got[f"{p}_wer_hi"], got[f"{p}_wer_se"]) == (st["lo"], st["hi"], st["se"])
        assert st["lo"] < agg[f"{p}_wer"] < st["hi"]
    assert {k: v for k, v in got.items() if not k.endswith(("_wer_lo", "_wer_hi", "_wer_se"))} == agg
    # stratified comparison: the units sorted by label (stably), the offsets from the label counts
    order = sorted(range(n), key=lambda k: corpus[k])
    offsets = [0, corpus.count("ami"), n]
    table = np.concatenate([cols(a), cols(b)], 1)[order]
    res, swp = B.sums_np(table, 500, 9, offsets), B.sums_np(table, 500, 9, None, "swap")
    got = S.compare_session_metrics(a, b, metrics, replicates=500, seed=9, strata=corpus)
    assert list(got) == metrics
    for m, metric in enumerate(metrics):
        c = [2 * m, 2 * m + 1, 6 + 2 * m, 6 + 2 * m + 1]
        assert got[metric] == S.comparison_statistics(res[:, c], swp[:, c], table.sum(0)[c], 0.05), metric
        assert got[metric]["rate_a"] == agg[metric] and 0.0 < got[metric]["p_value"] <= 1.0
    # --- utterance tables of word_error_counts: (errors, hits, substitutions, deletions, insertions)
    def counts(n_utt, rate):
        h = rng.integers(0, 30, n_utt)
        s, d, i = (rng.binomial(10, rate, n_utt) for _ in range(3))
        return np.stack([s + d + i, h, s, d, i], 1).astype(np.int64)

    ca, cb = counts(300, 0.10), counts(300, 0.12)
    cb[:, 1] = ca[:, 1] + ca[:, 2] + ca[:, 3] - cb[:, 2] - cb[:, 3]              # the same reference length for both systems ...
    keep = cb[:, 1] >= 0                                                          # ... where that leaves a count of hits
    ca, cb = ca[keep], cb[keep]
    ref_len = lambda c: c[:, 1] + c[:, 2] + c[:, 3]                               # noqa: E731
    table = np.stack([ca[:, 0], ref_len(ca), cb[:, 0], ref_len(cb)], 1)
    got = S.compare_wer(torch.from_numpy(ca).cuda(), torch.from_numpy(cb), replicates=400, seed=21)
    assert got == S.comparison_statistics(B.sums_np(table, 400, 21), B.sums_np(table, 400, 21, None, "swap"), table.sum(0), 0.05)
    got = S.wer_interval(torch.from_numpy(ca).cuda(), replicates=400, seed=21)
    assert got == {"rate": int(table[:, 0].sum()) / int(table[:, 1].sum()), **S.ratio_statistics(B.sums_np(table[:, :2], 400, 21), 0.05)}
    assert got["lo"] <= got["rate"] <= got["hi"] and got["undefined"] == 0

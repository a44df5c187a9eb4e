"""CPU tests of the bootstrap's host side: the oracle of tests/bootstrap_ref.py against the Random123 known answers and its numpy form
against its plain-Python form, draw sanity of the definition at fixed seeds, the C-ABI entry point and its binding, every refusal made
before any launch (with never-dereferenced device pointers), and the interval, probability-of-improvement and p-value rules on arrays
made by hand.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import bootstrap_ref as B
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, significance as S  # noqa: E402


def test_oracle_philox_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert B.philox4x32_10(counter, key) == want
        assert tuple(int(x) for x in B.philox_np(*counter, *key)) == want
    # the word of a slot is that block's entry p & 3, the replicate number fills counter words 1 and 2, the seed the key
    seed, r = (0xa4093822 | (0x299f31d0 << 32)), (0x85a308d3 | (0x13198a2e << 32))
    blk = B.philox4x32_10((5, 0x85a308d3, 0x13198a2e, 1), (0xa4093822, 0x299f31d0))
    assert [B.word(seed, r, 20 + q, 1) for q in range(4)] == list(blk)


def test_numpy_oracle_equals_the_plain_one():
    rng = np.random.default_rng(1)
    for n, C, offsets, seed, first in ((1, 1, None, 0, 0), (5, 3, None, 1234, 7), (13, 4, [0, 1, 6, 7, 13], (0xdeadbeef << 32) | 7, (1 << 32) - 2),
                                       (9, 6, None, 99, (1 << 64) - 2)):
        table = rng.integers(-(1 << 40), 1 << 40, (n, C))
        plain = B.sums(table.tolist(), 5, seed, offsets, "resample", first)
        assert B.sums_np(table, 5, seed, offsets, "resample", first).tolist() == plain
        if C % 2 == 0:
            assert B.sums_np(table, 5, seed, None, "swap", first).tolist() == B.sums(table.tolist(), 5, seed, None, "swap", first)
    assert B.sums_np(np.ones((3, 2), np.int64), 0).shape == (0, 2)


def test_every_replicate_draws_each_stratum_at_its_own_size():
    offsets = [0, 1, 6, 7, 64, 65]
    for r in (0, 1, (1 << 32) - 1, 1 << 32):
        d = B.draws(65, offsets, 1234, r)
        assert len(d) == 65
        for s in range(5):
            part = d[offsets[s]:offsets[s + 1]]
            assert all(offsets[s] <= u < offsets[s + 1] for u in part)
        assert d[0] == 0 and d[6] == 6 and d[64] == 64                      # a stratum of one unit draws that unit
    # in swap mode the two halves of a unit's columns are exchanged or not: A + B is the column total in every replicate
    table = np.random.default_rng(0).integers(0, 1000, (10, 4))
    out = B.sums_np(table, 50, 3, None, "swap")
    assert (out[:, :2] + out[:, 2:] == (table[:, :2] + table[:, 2:]).sum(0)).all() and len({tuple(x) for x in out.tolist()}) > 25


# the 99.9 % quantiles of chi-square at 4, 7 and 12 degrees of freedom
CHI2_999 = {5: 18.467, 8: 24.322, 13: 32.909}


@pytest.mark.parametrize("seed", [0, 1234, (0xdeadbeef << 32) | 7])
@pytest.mark.parametrize("n", [5, 8, 13])
def test_pooled_draw_counts_are_uniform(seed, n):
    R = 4096
    u = (B.words_np(n, R, seed, 0, 0) * np.uint64(n)) >> np.uint64(32)
    counts = np.bincount(u.reshape(-1).astype(np.int64), minlength=n)
    assert counts.sum() == R * n
    chi2 = float(((counts - R) ** 2 / R).sum())
    print(f"seed {seed:#x} n {n}: chi-square {chi2:.2f} at {n - 1} degrees of freedom, bound {CHI2_999[n]}")
    assert chi2 < CHI2_999[n]


def test_entry_point_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_bootstrap_sums\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const int64_t* table", "int64_t ld", "int n", "int C", "const int64_t* strata", "const int64_t* strata_dev", "int n_strata",
                    "int64_t R", "uint64_t first_replicate", "uint64_t seed", "int mode", "int plan", "int64_t* out", "void* stream"]
    assert re.search(r"^int\s+dicow_bootstrap_plan\s*\(\s*int n,\s*int C\s*\);", stable, flags=re.M)
    for name, val in (("MAX_N", _lib.BOOT_MAX_N), ("MAX_C", _lib.BOOT_MAX_C), ("MAX_R", _lib.BOOT_MAX_R), ("LDS_BYTES", _lib.BOOT_LDS_BYTES),
                      ("PLANS", _lib.BOOT_PLANS), ("LANE_LDS", _lib.BOOT_LANE_LDS), ("WAVE_LDS", _lib.BOOT_WAVE_LDS), ("WAVE_L2", _lib.BOOT_WAVE_L2),
                      ("RESAMPLE", _lib.BOOT_RESAMPLE), ("SWAP", _lib.BOOT_SWAP)):
        m = re.search(rf"^#define\s+DICOW_BOOT_{name}\s+(\d+)", stable, flags=re.M)
        assert m and int(m.group(1)) == val, name
    assert _lib.BOOT_MAX_N == 1 << 24 and _lib.BOOT_MAX_C == 32
    # the definition is stated in the header: the generator, its constants, both modes and the bias bound
    for words in ("THE DEFINITION", "Philox4x32-10(counter = (p >> 2, r & 0xffffffff, r >> 32, t), key = (seed & 0xffffffff, seed >> 32))[p & 3]",
                  "0xD2511F53 / 0xCD9E8D57", "0x9E3779B9 / 0xBB67AE85", "table[lo_s + ((w * n_s) >> 32), c]", "table[p, (c + h*b) mod C]",
                  "bias of at most n_s / 2^32", "n * max|table| < 2^62"):
        assert words in stable, words
    c = _lib
    assert _lib._SIGS["dicow_bootstrap_sums"] == [c.c_vp, c.c_i64, c.c_i, c.c_i, c.c_vp, c.c_vp, c.c_i, c.c_i64, c.c_u64, c.c_u64, c.c_i, c.c_i,
                                                  c.c_vp, c.c_vp]
    assert _lib._SIGS["dicow_bootstrap_plan"] == [c.c_i, c.c_i]
    assert {"dicow_bootstrap_sums", "dicow_bootstrap_plan"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.dicow_bootstrap_sums.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("bootstrap_sums", "percentile_interval", "ratio_interval", "compare_ratios", "session_metric_intervals", "compare_session_metrics",
                 "wer_interval", "compare_wer"):
        assert getattr(pkg, name) is getattr(S, name) and name in pkg.__all__


def test_the_library_names_a_plan_for_every_shape_and_only_staged_plans_have_a_limit():
    lib = _lib.lib()
    for n, C in ((1, 1), (40, 16), (256, 32), (257, 32), (8192, 1), (8193, 1), (20000, 4), (1 << 24, 32)):
        plan = lib.dicow_bootstrap_plan(n, C)
        fits = n * C * 8 <= _lib.BOOT_LDS_BYTES
        assert (plan in (_lib.BOOT_LANE_LDS, _lib.BOOT_WAVE_LDS)) if fits else plan == _lib.BOOT_WAVE_L2, (n, C, plan)
    for n, C in ((0, 1), (1, 0), ((1 << 24) + 1, 1), (1, 33)):
        assert lib.dicow_bootstrap_plan(n, C) == -1


def _call(lib, **kw):
    """dicow_bootstrap_sums with never-dereferenced device pointers (every call made through here is refused, or launches nothing)."""
    p = 4096
    a = dict(table=p, ld=None, n=8, C=4, strata=None, strata_dev=2 * p, R=16, first=0, seed=0, mode=0, plan=0, out=3 * p)
    a.update(kw)
    null = isinstance(a["strata"], str)
    offs = np.ascontiguousarray(np.asarray([0, a["n"]] if a["strata"] is None or null else a["strata"], np.int64))
    return lib.dicow_bootstrap_sums(a["table"], a["C"] if a["ld"] is None else a["ld"], a["n"], a["C"], None if null else offs.ctypes.data,
                                    a["strata_dev"], a.get("n_strata", len(offs) - 1), a["R"], a["first"], a["seed"], a["mode"], a["plan"], a["out"],
                                    None)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    for bad, word in ((dict(n=0), b"DICOW_BOOT_MAX_N"), (dict(n=(1 << 24) + 1), b"DICOW_BOOT_MAX_N"), (dict(C=0), b"DICOW_BOOT_MAX_C"),
                      (dict(C=33), b"DICOW_BOOT_MAX_C"), (dict(ld=3), b"ld=3 is below C=4"), (dict(R=-1), b"DICOW_BOOT_MAX_R"),
                      (dict(R=1 << 31), b"DICOW_BOOT_MAX_R"), (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"),
                      (dict(mode=1, C=5), b"C=5 is odd"), (dict(mode=1, C=1), b"C=1 is odd"),
                      (dict(plan=-1), b"plan=-1"), (dict(plan=_lib.BOOT_PLANS + 1), b"plan=4"),
                      (dict(plan=_lib.BOOT_LANE_LDS, n=2049), b"DICOW_BOOT_LDS_BYTES"), (dict(plan=_lib.BOOT_WAVE_LDS, n=257, C=32), b"DICOW_BOOT_LDS_BYTES"),
                      (dict(strata=[0, 3, 3, 8]), b"stratum 1 is empty"), (dict(strata=[0, 5, 4, 8]), b"stratum 1 is empty or the offsets descend"),
                      (dict(strata=[1, 8]), b"not from 0 to n = 8"), (dict(strata=[0, 4, 7]), b"not from 0 to n = 8"),
                      (dict(strata=[0, 8], n_strata=0), b"n_strata=0"), (dict(strata=list(range(9)), n_strata=9), b"n_strata=9"),
                      (dict(strata="null"), b"null strata"), (dict(table=None), b"null pointer"), (dict(out=None), b"null pointer"),
                      (dict(strata=[0, 4, 8], strata_dev=None), b"null pointer"), (dict(table=4100), b"aligned"), (dict(out=4100), b"aligned"),
                      (dict(strata=[0, 4, 8], strata_dev=4100), b"aligned")):
        rc = _call(lib, **bad)
        assert rc == -1, bad
        assert b"bootstrap_sums" in lib.dicow_last_error() and word in lib.dicow_last_error(), (bad, lib.dicow_last_error())
    # no replicates: succeeds and touches nothing, whatever the pointers; the limits themselves pass the checks
    assert _call(lib, R=0, table=None, out=None, strata_dev=None) == 0
    assert _call(lib, R=0, plan=_lib.BOOT_LANE_LDS, n=2048) == 0 and _call(lib, R=0, plan=_lib.BOOT_WAVE_LDS, n=256, C=32) == 0
    assert _call(lib, R=0, plan=_lib.BOOT_WAVE_L2, n=1 << 24, C=32) == 0 and _call(lib, R=0, mode=1, strata=[0, 4, 8], strata_dev=None) == 0


def test_wrappers_refuse_what_they_cannot_run():
    t = torch.ones((4, 2), dtype=torch.int64)
    with pytest.raises(_lib.DicowError, match="GPU"):
        S.bootstrap_sums(t, 10)
    with pytest.raises(_lib.DicowError, match="GPU"):
        S.bootstrap_sums(t.numpy(), 10)
    # the offsets and the overflow bound are checked by pure host functions
    for bad in ([0, 2, 2, 4], [0, 3, 2, 4], [1, 4], [0, 3], [0]):
        with pytest.raises(_lib.DicowError, match="strat"):
            S._offsets(bad, 4, "bootstrap_sums")
    assert S._offsets(None, 4, "x").tolist() == [0, 4] and S._offsets([0, 1, 4], 4, "x").tolist() == [0, 1, 4]
    S.check_sum_bound(4, -(1 << 60) + 1, (1 << 60) - 1)
    S.check_sum_bound(1 << 24, 0, (1 << 38) - 1)
    for n, lo, hi in ((4, 0, 1 << 60), (4, -(1 << 60), 0), (1 << 24, 0, 1 << 38), (1, -(1 << 63), 0)):
        with pytest.raises(_lib.DicowError, match="2\\^62"):
            S.check_sum_bound(n, lo, hi)
    with pytest.raises(_lib.DicowError, match="integers"):
        S.ratio_interval([0.5, 1.0], [1, 1], device="cpu")
    with pytest.raises(_lib.DicowError, match="units"):
        S.compare_ratios([1, 2], [3, 4], [1], [3, 4], device="cpu")
    # a different reference for one session is refused before anything is uploaded
    a = [dict(cp_errors=3, cp_length=10, tcp_errors=4, tcp_length=10), dict(cp_errors=1, cp_length=20, tcp_errors=2, tcp_length=20)]
    b = [dict(cp_errors=2, cp_length=10, tcp_errors=4, tcp_length=10), dict(cp_errors=1, cp_length=20, tcp_errors=2, tcp_length=21)]
    with pytest.raises(_lib.DicowError, match="session 1 has tcp_length 20 for system A and 21 for system B"):
        S.compare_session_metrics(a, b, ["cp_wer", "tcp_wer"])
    with pytest.raises(_lib.DicowError, match="2 sessions of system A against 1"):
        S.compare_session_metrics(a, b[:1], ["cp_wer"])
    with pytest.raises(_lib.DicowError, match="orc_errors"):
        S.compare_session_metrics(a, a, ["orc_wer"])
    with pytest.raises(ValueError, match="unknown metric"):
        S.session_metric_intervals(a, ["wer"])
    with pytest.raises(_lib.DicowError, match=r"\[n, 5\]"):
        S.wer_interval(torch.ones((3, 4), dtype=torch.int64))


def test_strata_labels_become_sorted_units_and_offsets():
    table, offs = S._table(([10, 11, 12, 13, 14], [1, 1, 1, 1, 1]), ["b", "a", "b", "c", "a"], "cpu", "t")
    assert offs.tolist() == [0, 2, 4, 5] and table[:, 0].tolist() == [11, 14, 10, 12, 13]        # stable inside a stratum
    table, offs = S._table(([1, 2], [3, 4]), None, "cpu", "t")
    assert offs is None and table.tolist() == [[1, 3], [2, 4]] and table.dtype == torch.int64


def test_the_interval_rule_on_arrays_made_by_hand():
    for k, (lo, hi) in {1: (0, 0), 2: (0, 1), 39: (0, 38), 40: (1, 38), 41: (1, 39), 10000: (250, 9749)}.items():
        v = np.random.default_rng(k).permutation(k).astype(np.float64)      # the values are their own ranks
        assert S.percentile_interval(v, 0.05) == (float(lo), float(hi)), k
    assert S.percentile_interval(np.arange(100.0), 0.1) == (5.0, 94.0) and S.percentile_interval(np.arange(7.0), 0.5) == (1.0, 5.0)
    assert all(np.isnan(x) for x in S.percentile_interval([], 0.05))
    with pytest.raises(ValueError):
        S.percentile_interval([1.0], 1.0)
    # rates are float64 num / den; a zero denominator is counted and left out; se is the sample standard deviation
    st = S.ratio_statistics([[1, 4], [3, 4], [5, 0], [2, 4], [0, 0]], 0.05)
    assert st == {"lo": 0.25, "hi": 0.75, "se": float(np.std([0.25, 0.75, 0.5], ddof=1)), "replicates": 5, "undefined": 2}
    one = S.ratio_statistics([[1, 3]], 0.05)
    assert one["lo"] == one["hi"] == 1 / 3 and np.isnan(one["se"]) and one["undefined"] == 0
    none = S.ratio_statistics([[1, 0]], 0.05)
    assert np.isnan(none["lo"]) and np.isnan(none["hi"]) and np.isnan(none["se"]) and none["undefined"] == 1


def test_probability_of_improvement_and_p_value_on_arrays_made_by_hand():
    # a shared reference (equal denominators everywhere): integer comparisons.  deltas of the resampled rows: -, -, 0, +, 0
    res = [[3, 10, 5, 10], [1, 12, 2, 12], [4, 9, 4, 9], [6, 10, 5, 10], [0, 11, 0, 11]]
    # observed |num_a - num_b| = 2; swapped |differences| 2, 1, 3, 0, 2, 2 -> four are as extreme
    swp = [[5, 10, 3, 10], [4, 10, 5, 10], [2, 10, 5, 10], [4, 10, 4, 10], [3, 10, 5, 10], [6, 10, 4, 10]]
    st = S.comparison_statistics(res, swp, [3, 10, 5, 10], 0.05)
    assert st["rate_a"] == 0.3 and st["rate_b"] == 0.5 and st["delta"] == 0.3 - 0.5
    assert st["prob_a_better"] == (2 + 0.5 * 2) / 5 and st["p_value"] == (1 + 4) / 7
    d = [3 / 10 - 5 / 10, 1 / 12 - 2 / 12, 4 / 9 - 4 / 9, 6 / 10 - 5 / 10, 0 / 11 - 0 / 11]
    assert (st["lo"], st["hi"]) == (min(d), max(d)) and st["se"] == float(np.std(d, ddof=1)) and st["replicates"] == 5 and st["undefined"] == 0
    # ties that float64 would break: 1/3 - 1/3 against (1/3 + 1/3) - 2/3 style sums are avoided by comparing the integers
    res = [[1, 3, 1, 3]] * 4
    st = S.comparison_statistics(res, [[1, 3, 1, 3]] * 3, [1, 3, 1, 3], 0.05)
    assert st["prob_a_better"] == 0.5 and st["p_value"] == 1.0 and st["delta"] == 0.0 and (st["lo"], st["hi"]) == (0.0, 0.0)
    # different denominators: float64.  resampled deltas: 1/2 - 2/3 < 0, 2/4 - 1/2 == 0, 3/4 - 1/2 > 0, one undefined
    res = [[1, 2, 2, 3], [2, 4, 1, 2], [3, 4, 1, 2], [1, 0, 1, 2]]
    swp = [[1, 2, 2, 3], [2, 3, 1, 2], [1, 2, 1, 2], [1, 2, 1, 0]]
    st = S.comparison_statistics(res, swp, [1, 2, 2, 3], 0.05)
    assert st["prob_a_better"] == (1 + 0.5) / 3 and st["undefined"] == 1 and st["replicates"] == 4
    # |delta_obs| = 1/6: the first two swapped rows attain it, the third does not, the undefined one counts as extreme
    assert st["p_value"] == (1 + 3) / 5
    # a system that is better in every replicate
    st = S.comparison_statistics([[1, 5, 2, 5]] * 10, [[1, 5, 2, 5], [2, 5, 1, 5]] * 5, [1, 5, 2, 5], 0.05)
    assert st["prob_a_better"] == 1.0 and st["p_value"] == 1.0
    st = S.comparison_statistics([[1, 5, 2, 5]] * 10, [[1, 5, 1, 5]] * 999, [1, 5, 2, 5], 0.05)
    assert st["p_value"] == 1 / 1000

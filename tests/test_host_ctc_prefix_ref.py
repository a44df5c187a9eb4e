"""The fp64 references of the decode-time scoring kernels (tests/ctc_prefix_ref.py, tests/timestamp_rules_ref.py) against the
fp32 oracles and the golden files of the reference implementation, on the CPU: the references cannot drift from what the reference
computes.  Tolerances are those of tests/test_oracle_vs_golden.py for the same files."""
import numpy as np

from oracle import ctc_prefix as ocp
from oracle.timestamp_rules import timestamp_rules as oracle_rules
from tests import ctc_prefix_ref as ref
from tests import timestamp_rules_ref as tsref
from tests.util import load_golden


def _close_lz(got, want, tol):
    """Logzero (-1e10) in the same places and exact; real entries within tol."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    real = want > -1e9
    assert np.array_equal(real, got > -1e9)
    assert np.array_equal(got[~real], want[~real])
    return (not real.any()) or float(np.abs(got[real] - want[real]).max()) < tol


def _steps(z):
    for s in range(int(z["a.steps"])):
        act = z[f"a.{s}.active"]
        yield s, np.nonzero(act)[0], z[f"a.{s}.cs"][act], z[f"a.{s}.dl"][act], z[f"a.{s}.y"][act][:, -1], z[f"a.{s}.r_prev"][act]


def test_prefix_ref_vs_golden_and_oracle():
    """States, psi and the initial state over every golden step (prefixes of two and more labels included) against the golden
    file and against the fp32 oracle; logzero sits exactly where the fp32 arithmetic produces -1e10, and nowhere else."""
    z = load_golden("f13_ctc_prefix")
    x, blank, eos = z["a.x"], int(z["a.blank"]), int(z["a.eos"])
    assert ref.in_domain(x)
    assert _close_lz(ref.initial_state(x, blank), z["a.r0"], 1e-4)
    assert _close_lz(ref.initial_state(x, blank), ocp.initial_state(x, blank), 1e-4)
    deepest = 0
    for s, rows, cs, dl, last, r_prev in _steps(z):
        deepest = max(deepest, int(dl.max()))
        psi, r = ref.prefix_score(x, rows, cs, dl, last, r_prev, blank, eos)
        assert _close_lz(psi, z[f"a.{s}.psi"], 5e-6) and _close_lz(r, z[f"a.{s}.r"], 5e-5), s
        opsi, orr = ocp.prefix_score(x, rows, cs, dl, last, r_prev, blank, eos)
        assert _close_lz(psi, opsi, 5e-6) and _close_lz(r, orr, 5e-5), s
        assert np.array_equal(opsi == ocp.LOGZERO, psi == ref.LOGZERO) and np.array_equal(orr == ocp.LOGZERO, r == ref.LOGZERO), s
        assert np.array_equal(z[f"a.{s}.psi"] == ocp.LOGZERO, psi == ref.LOGZERO) and np.array_equal(z[f"a.{s}.r"] == ocp.LOGZERO, r == ref.LOGZERO), s
    assert deepest >= 2


def test_prefix_ref_edges_vs_oracle():
    """What the golden file does not reach: one frame, aliased columns, eos == blank, a repeated label with d = 0, and chained
    states down to a prefix as long as the utterance -- the fp32 oracle on the same values agrees, logzero places included."""
    g = np.random.default_rng(5)
    for T, C, d_max, eos_is_blank in ((1, 4, 1, False), (2, 4, 2, False), (7, 5, 7, True), (18, 6, 5, False)):
        V1 = 12
        blank, eos = V1 - 1, (V1 - 1 if eos_is_blank else 9)
        x = ref.log_probs(g.standard_normal((2, T, V1)) * 2, V1).astype(np.float32)
        rows = np.array([1, 0, 1])
        r_prev = ref.initial_state(x, blank)[rows].astype(np.float32)
        last = np.array([3, 4, 5])                                       # d = 0 with a real `last`: the repeat rule must not fire
        for d in range(d_max + 1):
            cs = g.integers(0, V1 - 1, (3, C))
            cs[:, 0], cs[:, 1], cs[:, 2] = last, eos, blank
            dl = np.full(3, d)
            psi, r = ref.prefix_score(x, rows, cs, dl, last, r_prev, blank, eos)
            opsi, orr = ocp.prefix_score(x, rows, cs, dl, last, r_prev, blank, eos)
            assert ref.in_domain(psi, r)
            assert _close_lz(psi, opsi, 5e-5) and _close_lz(r, orr, 5e-5), (T, d)
            pick = C - 1
            last = cs[:, pick]
            r_prev = r[..., pick].astype(np.float32)
    # an alias table is the same as scoring the aliased columns directly
    alias = np.arange(V1)
    alias[[4, 5]] = [1, 2]
    alias[blank] = 8
    xa = x[..., alias]
    r0 = ref.initial_state(xa, blank)[rows]
    cs = np.array([[4, 1, blank], [5, 2, 9], [0, 4, 8]])
    a = ref.prefix_score(x, rows, cs, np.zeros(3), last, r0, blank, 9, alias)
    b = ref.prefix_score(xa, rows, cs, np.zeros(3), last, r0, blank, 9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0][0, 0], a[0][0, 1]) and a[0][0, 2] == ref.LOGZERO


def test_frame_lse_ref():
    g = np.random.default_rng(6)
    z = g.standard_normal((5, 40)) * 2
    z[1, 3:9] = -np.inf
    z[2] = 1.25
    want = np.log(np.exp(z[:, :33]).sum(-1))
    assert float(np.abs(ref.frame_lse(z, 33) - want).max()) < 1e-12
    assert abs(ref.frame_lse(z, 33)[2] - (1.25 + np.log(33))) < 1e-12
    zz = np.full((1, 9), -80.0)
    zz[0, 4] = 80.0
    assert ref.frame_lse(zz, 9)[0] == 80.0


def test_timestamp_ref_vs_golden_and_oracle():
    """Outputs equal on every golden case, and equal to the oracle's on the same inputs."""
    z = load_golden("f14_timestamp_rules")
    V, eos, no_ts, ts0, begin = (int(v) for v in z["cfg"])
    assert int(z["n_cases"]) > 0
    for i in range(int(z["n_cases"])):
        mi = int(z[f"c{i}.max_init"])
        mi = None if mi < 0 else mi
        ids, sc = z[f"c{i}.ids"], z[f"c{i}.scores"]
        ban, margin, out = tsref.timestamp_rules(ids, sc, begin, eos, no_ts, mi)
        assert np.array_equal(out, z[f"c{i}.out"]), i
        assert np.array_equal(out, oracle_rules(ids, sc, begin, eos, no_ts, mi)), i
        assert out.dtype == np.float32 and ban.shape == sc.shape and margin.shape == (sc.shape[0],)
        assert bool(np.isneginf(out[ban & ~((ids.shape[1] == begin) & (np.arange(V) == eos))[None, :]]).all())


def test_timestamp_ref_minus_inf_is_zero_mass():
    """-inf among the allowed timestamp labels changes neither the margin nor the decision; the oracle (torch.logsumexp's
    semantics) agrees on every row."""
    g = np.random.default_rng(7)
    V, eos, no_ts, begin = 2600, 90, 99, 3
    ids = np.concatenate([np.full((4, begin), 7), g.integers(0, 80, (4, 2))], axis=1)
    sc = (g.standard_normal((4, V)) * 2).astype(np.float32)
    sc[:, no_ts + 1:] += 1.0
    _, m0, out0 = tsref.timestamp_rules(ids, sc, begin, eos, no_ts, None)
    assert bool((m0 > 1).all()) and bool(np.isneginf(out0[:, :no_ts + 1]).all())
    sc2 = sc.copy()
    sc2[0, no_ts + 6] = sc2[1, no_ts + 6 + 1024] = -np.inf
    sc2[2, no_ts + 1::3] = -np.inf
    sc2[3, no_ts + 1:] = -np.inf
    _, m, out = tsref.timestamp_rules(ids, sc2, begin, eos, no_ts, None)
    assert bool((np.abs(m[:2] - m0[:2]) < 1e-2).all()) and m[2] > 0 and m[3] == -np.inf
    assert np.array_equal(out, oracle_rules(ids, sc2, begin, eos, no_ts, None))
    assert bool(np.isneginf(out[:3, :no_ts + 1]).all()) and int(np.isfinite(out[3, :no_ts]).sum()) == no_ts

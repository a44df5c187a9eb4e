"""timestamp_rules_kernel (csrc/ctc_prefix.hip) against the fp64 reference tests/timestamp_rules_ref.py where the existing tests do not
go: rows that already hold -inf (a suppress list or the repetition rules ran first), the detection `logsumexp(timestamps) >
max(text)` near its threshold, the chain of processors as the decoders run it, and the structural edges of the rules.

Two geometries: a small vocabulary whose timestamp span is longer than two strides of the 1024-thread workgroup (V = 2600 in rows of
2688, <|notimestamps|> = 99), and the real one (V = 51866 in rows of 51968, <|notimestamps|> = 50364).  In every case the output row
must equal the reference's bit for bit: a label the rules ban (or a text label once timestamps are detected) is -inf, every other
score keeps the bits of the input, the eos score of the first step is restored; the columns from V on and the guard bands around
the buffer keep their fill.  Run with `pytest -m gpu`."""
import math

import numpy as np
import pytest
import torch

import amd_pkg
from tests import timestamp_rules_ref as tsref
from tests.util import guarded

pytestmark = pytest.mark.gpu
amd_pkg.load()

U = 2.0 ** -24
NEG = -np.inf
GEO = {  # V, ld, no_timestamps, eos, begin
    "small": dict(V=2600, ld=2688, no_ts=99, eos=90, begin=3),
    "real": dict(V=51866, ld=51968, no_ts=50364, eos=50257, begin=4),
}


@pytest.fixture(scope="module")
def rules():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import generation
    return generation


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _apply(rules, geo, ids, scores, max_init=None, before=None):
    """The kernel on `scores` (fp32 [B, V], CPU) held in guarded rows of geo['ld'] columns.  before(ids_dev, view): processors to run
    first on the same device rows.  Returns the rows on the CPU after checking the guards."""
    B, V = scores.shape
    gd = guarded((B, V), geo["ld"], torch.float32, init=torch.from_numpy(scores), name="scores")
    dev_ids = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    if before is not None:
        before(dev_ids, gd.view)
    out = rules.timestamp_rules(dev_ids, gd.view, geo["begin"], geo["eos"], geo["no_ts"], max_init)
    torch.cuda.synchronize()
    assert out.data_ptr() == gd.view.data_ptr()
    gd.check()
    return gd.view.cpu().numpy()


def _check(rules, geo, ids, scores, max_init=None, what=""):
    """Run and compare with the reference: the banned mask follows the rules alone, survivors keep the input's bits."""
    got = _apply(rules, geo, ids, scores, max_init)
    ban, margin, want = tsref.timestamp_rules(ids, scores, geo["begin"], geo["eos"], geo["no_ts"], max_init)
    ts0 = geo["no_ts"] + 1
    detected = margin > 0
    first = ids.shape[1] == geo["begin"]
    gone = ban | (detected[:, None] & (np.arange(scores.shape[1]) < ts0)[None, :])
    if first:
        gone[:, geo["eos"]] = False
    bad_rows = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
    assert bad_rows.size == 0, (f"{what}: rows {bad_rows[:8].tolist()} differ; margins {margin[bad_rows[:8]].tolist()}; finite text labels left "
                                f"{[int(np.isfinite(got[r, :geo['no_ts']]).sum()) for r in bad_rows[:8]]}")
    assert bool(np.isneginf(got[gone]).all()) and np.array_equal(_bits(got[~gone]), _bits(scores[~gone])), what
    return margin


def _base(geo, B, g, boost):
    sc = (g.standard_normal((B, geo["V"])) * 2).astype(np.float32)
    sc[:, geo["no_ts"] + 1:] += np.float32(boost)
    return sc


def _histories(geo, g):
    """The three states in which text is not already banned by the pairing rule: (generated suffix, first timestamp label still allowed)."""
    ts0 = geo["no_ts"] + 1
    t = [int(v) for v in g.integers(0, geo["eos"] - 1, 4)]
    return {"two_text": (t[:2], ts0),
            "one_text": (t[:1], ts0),
            "text_after_closed_pair": ([ts0 + 3, t[0], ts0 + 7, ts0 + 7, t[1]], ts0 + 8)}


@pytest.mark.parametrize("geo_name", ["small", "real"])
@pytest.mark.parametrize("state", ["two_text", "one_text", "text_after_closed_pair"])
def test_minus_inf_among_allowed_timestamps(rules, geo_name, state):
    """A timestamp label that the rules allow already holds -inf.  v is the first timestamp label its thread visits and v + 1024
    the second: -inf at v only, at v + 1024 only, at several labels, at all of them.  The timestamp mass is clearly above the best
    text score (by more than 1) except in the last row, where there is none: the detection must follow the fp64 reference."""
    geo = GEO[geo_name]
    g = np.random.default_rng(31 + ("two_text", "one_text", "text_after_closed_pair").index(state))
    gen, lo = _histories(geo, g)[state]
    ts0 = geo["no_ts"] + 1
    v = ts0 + 20
    assert v >= lo and v + 1024 < geo["V"] and v - 1024 < ts0                     # v is its thread's first timestamp label
    sc = _base(geo, 6, g, 3.0)
    sc[1, v] = NEG
    sc[2, v + 1024] = NEG
    sc[3, [v, v + 1, v + 7, v + 1024 + 3, geo["V"] - 1, lo]] = NEG
    sc[4, ts0::2] = NEG
    sc[4, v + 1] = NEG
    sc[5, ts0:] = NEG
    ids = np.array([[1] * geo["begin"] + gen] * 6, dtype=np.int64)
    margin = _check(rules, geo, ids, sc, None, f"{geo_name} {state}")
    print(f"EDGE ts -inf {geo_name} {state}: margins {np.array2string(margin, precision=3)}")
    assert bool((margin[:5] > 1).all()) and margin[5] == NEG


@pytest.mark.parametrize("geo_name", ["small", "real"])
def test_minus_inf_among_text_labels(rules, geo_name):
    geo = GEO[geo_name]
    g = np.random.default_rng(41)
    ts0, eos, begin = geo["no_ts"] + 1, geo["eos"], geo["begin"]
    sc = _base(geo, 4, g, 0.0)
    sc[0, g.integers(0, ts0, 40)] = NEG                                  # some text labels
    sc[1, :ts0][np.argsort(sc[1, :ts0])[-3:]] = NEG                      # the three best text labels
    sc[2, :ts0] = NEG                                                    # all text, finite timestamps
    sc[3, :ts0] = NEG
    sc[3, ts0:] -= 30.0
    ids = np.array([[1] * begin + [5]] * 4, dtype=np.int64)
    margin = _check(rules, geo, ids, sc, None, f"{geo_name} text -inf")
    assert margin[2] == np.inf and margin[3] == np.inf
    # the first step with everything at -inf except eos: text is banned, no timestamp mass is left, the eos restore survives
    first = np.full((2, geo["V"]), NEG, dtype=np.float32)
    first[:, eos] = [-0.25, 3.5]
    first[1, ts0 + 4] = -7.0
    ids0 = np.array([[1] * begin] * 2, dtype=np.int64)
    got = _apply(rules, geo, ids0, first, 50)
    _check(rules, geo, ids0, first, 50, f"{geo_name} first step")
    assert got[0, eos] == np.float32(-0.25) and int(np.isfinite(got[0]).sum()) == 1
    assert got[1, eos] == np.float32(3.5) and got[1, ts0 + 4] == np.float32(-7.0) and int(np.isfinite(got[1]).sum()) == 2


def _lse32_bound(ts_allowed, lse64):
    """fp32 error of the kernel's logsumexp over the n allowed timestamp scores (n <= 1501 at the real vocabulary, 2500 at the small
    one; u = 2^-24), relative to the total S = sum e^(s - max):
      * a term reaches the total as e^(s - tm) e^(tm - wm) e^(wm - max) -- the thread's, the wave's and the workgroup's running
        maxima: three expf of 1 ulp (2u each), two products (u each), and three rounded exponents whose magnitudes add up to
        a = max - s, moving the term by at most u a e^-a relative to S after weighting: summed from the data as u sum(a e^-a) / S;
      * additions on a term's way: at most 3 in its thread (ceil(2500 / 1024)), the 6-step wave tree, 16 wave partials: 25 u;
      * logf is 1 ulp: 2u |log S|; the final max + log S rounds once: u |lse|.
    The text side is a maximum of input values: exact."""
    s = ts_allowed[np.isfinite(ts_allowed)].astype(np.float64)
    a = s.max() - s
    e = np.exp(-a)
    S = e.sum()
    return U * (a * e).sum() / S + (3 * 2 + 2 + 25) * U + 2 * U * abs(math.log(S)) + U * abs(lse64)


@pytest.mark.parametrize("geo_name", ["small", "real"])
def test_detection_near_its_threshold(rules, geo_name):
    """Rows whose fp64 margin logsumexp(timestamps) - max(text) is +delta and -delta, delta in {1e-3, 1e-2, 1}; the best text label
    at column 0, at ts0 - 2 (the last text label: ts0 - 1 is <|notimestamps|>, which is banned and holds the row's largest score
    here -- it must not count), and at a column of the last wave of the workgroup (real vocabulary; the small one has text labels
    in the first two waves only and uses column 64); the timestamp mass on one label, on 8, on all.  A row is compared only if its
    margin exceeds the fp32 error bound of the kernel's logsumexp (_lse32_bound); by construction every row does."""
    geo = GEO[geo_name]
    g = np.random.default_rng(51)
    V, ts0, begin = geo["V"], geo["no_ts"] + 1, geo["begin"]
    n_ts = V - ts0
    cols = (0, ts0 - 2, 1023 + 7 * 1024 if geo_name == "real" else 64)
    plan = [(delta, sign, col, spread) for delta in (1e-3, 1e-2, 1.0) for sign in (1, -1) for col in cols for spread in (1, 8, n_ts)]
    sc = np.empty((len(plan), V), dtype=np.float32)
    for k, (delta, sign, col, spread) in enumerate(plan):
        ts = (-75.0 + g.standard_normal(n_ts)).astype(np.float32)        # e^-75: present in the fp64 margin, invisible in fp32
        hot = g.permutation(n_ts)[:spread]
        ts[hot] = (g.standard_normal(spread) * 2).astype(np.float32)
        lse = tsref._lse64(ts.astype(np.float64))
        best = np.float32(lse - sign * delta)
        text = np.minimum((g.standard_normal(ts0) * 2).astype(np.float32), best - np.float32(2.0))
        text[col] = best
        text[geo["no_ts"]] = 50.0
        sc[k, :ts0], sc[k, ts0:] = text, ts
    ids = np.array([[1] * begin + [5]] * len(plan), dtype=np.int64)
    _, margin, _ = tsref.timestamp_rules(ids, sc, begin, geo["eos"], geo["no_ts"], None)
    bounds = np.array([_lse32_bound(sc[k, ts0:], margin[k] + float(sc[k, plan[k][2]])) for k in range(len(plan))])
    keep = np.abs(margin) > bounds
    print(f"EDGE ts threshold {geo_name}: {len(plan)} rows, smallest |margin| {np.abs(margin).min():.3e}, largest lse bound {bounds.max():.3e}")
    assert bool(keep.all()), "a generated row fell inside the fp32 error bound"
    assert all((margin[k] > 0) == (plan[k][1] > 0) and abs(abs(margin[k]) - plan[k][0]) < 1e-5 for k in range(len(plan)))
    _check(rules, geo, ids, sc, None, f"{geo_name} threshold")


@pytest.mark.parametrize("geo_name", ["small", "real"])
def test_exact_tie_is_not_a_detection(rules, geo_name):
    """One timestamp label carries all the mass (every other one is -inf): its logsumexp is its score, exactly, in fp64 and in the
    kernel's fp32 alike (a sum of one term 1, log 1 = 0).  The best text score equal to it is a tie, and the rule is a strict
    `>`: text stays.  One ulp below, timestamps win; one ulp above, text does."""
    geo = GEO[geo_name]
    g = np.random.default_rng(57)
    V, ts0, begin = geo["V"], geo["no_ts"] + 1, geo["begin"]
    s = np.float32(1.7182817)
    sc = np.empty((6, V), dtype=np.float32)
    for k, (best, label) in enumerate(((s, ts0 + 20), (np.nextafter(s, np.float32(-9)), ts0 + 20), (np.nextafter(s, np.float32(9)), ts0 + 20),
                                       (s, ts0 + 20 + 1024), (s, V - 1), (s, ts0))):
        sc[k, :ts0] = np.minimum((g.standard_normal(ts0) * 2).astype(np.float32), s - np.float32(1.0))
        sc[k, (0, ts0 - 2, 64)[k % 3]] = best
        sc[k, ts0:] = NEG
        sc[k, label] = s
    ids = np.array([[1] * begin + [5]] * 6, dtype=np.int64)
    margin = _check(rules, geo, ids, sc, None, f"{geo_name} exact tie")
    assert margin[0] == 0 and margin[1] > 0 and margin[2] < 0 and bool((margin[3:] == 0).all())


@pytest.mark.parametrize("geo_name", ["small", "real"])
def test_chain_as_the_decoders_run_it(rules, geo_name):
    """repetition_rules (no-repeat n-grams, which here ban a timestamp label too), a suppress list that names a timestamp label,
    then timestamp_rules -- on the same device rows, as GreedyDecoder / BeamDecoder do.  The final rows equal the references applied
    in that order (a banned n-gram continuation is exactly -inf, so the whole chain is bit-exact)."""
    geo = GEO[geo_name]
    g = np.random.default_rng(61)
    V, ts0, begin, eos = geo["V"], geo["no_ts"] + 1, geo["begin"], geo["eos"]
    v = ts0 + 20
    w = v + 5                                                 # an allowed timestamp label (> v), first of its thread; w + 1024 stays finite
    gen = [ts0 + 3, 11, 12, v, v, 13, 11, 12, 14, 11]         # text after a closed pair; 11 was followed by 12 before
    B = 5
    ids = np.array([[1] * (begin - 2) + [12, w] + gen] * B, dtype=np.int64)     # the prompt holds (12, w): history for the n-grams only
    ids[1, -1] = 12                                           # (12, w) was seen: the n-gram rule bans the allowed timestamp label w
    ids[2, -1] = 12
    sc = _base(geo, B, g, 3.0)
    sc[3, ts0:] -= 14.0                                       # a row in which text wins
    suppress = [v + 9, 7, v + 1024 + 2]
    ngram = 2

    def before(dev_ids, view):
        rules.repetition_rules(dev_ids, view, None, ngram)
        view[:, torch.as_tensor(suppress, device=view.device)] = -float("inf")

    got = _apply(rules, geo, ids, sc, None, before)
    mid = sc.copy()
    for b in range(B):
        seq = ids[b].tolist()
        for j in range(len(seq) - ngram + 1):
            if seq[j:j + ngram - 1] == seq[len(seq) - ngram + 1:]:
                mid[b, seq[j + ngram - 1]] = NEG
    assert np.isneginf(mid[1, w]) and np.isneginf(mid[0, 12]) and np.isfinite(mid[0, w]) and w + 1024 < V
    mid[:, suppress] = NEG
    _, margin, want = tsref.timestamp_rules(ids, mid, begin, eos, geo["no_ts"], None)
    print(f"EDGE ts chain {geo_name}: margins {np.array2string(margin, precision=3)}")
    assert bool((margin[[0, 1, 2, 4]] > 1).all()) and margin[3] < -1
    bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
    assert bad.size == 0, f"rows {bad.tolist()} differ from repetition -> suppress -> timestamp references; margins {margin[bad].tolist()}"


def _sprinkled_history(geo, g, B, n_new):
    """Random text with timestamp pairs every nine tokens; some rows end on one or on two timestamps."""
    ts0 = geo["no_ts"] + 1
    span = min(geo["V"] - ts0 - 2, 1400)
    ids = g.integers(0, geo["eos"] - 1, (B, geo["begin"] + n_new))
    for b in range(B):
        for j in range(geo["begin"] + 2, geo["begin"] + n_new - 1, 9):
            ids[b, j] = ids[b, j + 1] = ts0 + min(span, 2 * j + b)
        if n_new and b % 3 == 0:
            ids[b, -1] = ts0 + span + 1
        if n_new > 1 and b % 6 == 0:
            ids[b, -2] = ts0 + span + 1
    return ids.astype(np.int64)


@pytest.mark.parametrize("geo_name,B", [("small", 1), ("small", 33), ("real", 1)])
@pytest.mark.parametrize("n_new", [0, 1, 440])
@pytest.mark.parametrize("max_init", [None, 0, 10 ** 6])
def test_structural_edges(rules, geo_name, B, n_new, max_init):
    """max_initial_timestamp_index None, 0 and past the end of the vocabulary; the first step, the second, a 440-token history;
    one row and 33.  Rows carry a few -inf entries of their own, on both sides of the first timestamp label."""
    geo = GEO[geo_name]
    g = np.random.default_rng(71 + n_new + B)
    ids = _sprinkled_history(geo, g, B, n_new)
    sc = _base(geo, B, g, 2.0 if n_new == 440 else 0.0)
    for b in range(B):
        sc[b, g.integers(0, geo["V"], 12)] = NEG
    margin = _check(rules, geo, ids, sc, max_init, f"{geo_name} B={B} n_new={n_new} max_init={max_init}")
    assert margin.shape == (B,)

"""dicow_sample_tokens (generation.sample_tokens) against the numpy / fp64 oracle of its definition (tests/sampling_ref.py) and against
transformers' TopKLogitsWarper run on CPU copies of the same fp32 inputs.

Layout: the scores sit inside the guard bands of tests/util.py::guarded with ld > V (read only: the bands and the gap keep the sentinel,
the scores keep their bits), `warped` likewise (columns >= V keep the sentinel), `next` is a strided column of a wider int64 buffer filled
with a sentinel.  Every plan is run and all outputs must be bit-identical between plans.

What is exact and what has a band.  top_k counts: exact.  The draw and top_p / min_p compare fp32 (fp64-summed) quantities with the
oracle's fp64 ones, so
  * the kept mask must equal the oracle's for every token outside the band -- cumulative mass within 2e-5 of 1 - top_p, ratio within 1e-6
    (relative) of min_p -- and at most 0.2 % of a row's tokens may lie in the band (a condition on the inputs, not a tolerance); 2e-5 is
    the fp32 budget of 51 serial adds a lane plus a 10-level tree plus a few ulps per exp, about 70 * 2^-24 = 4e-6, with 4x headroom;
  * the token must equal the oracle's Gumbel argmax wherever the oracle's two best fp64 keys differ by more than 1e-4 max(1, |key|),
    and be one of the two elsewhere; at most 1 % of the rows a test draws may fall under that exception;
  * the log-probability lies within 2^-22 |lp| + 70 * 2^-24 of the oracle's.
The figures the run saw are printed (tools/bench_sampling.py collects them into profiles/sampling.txt)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
SENT = -777
VS = [1, 2, 63, 64, 65, 1000, 1024, 1025, 51866, 70000]
ROWS = [1, 3, 16]
SEEN = dict(logprob_err=0.0, flipped_mass=0.0, draws=0, close_calls=0)


@pytest.fixture(scope="module")
def pkg():
    import amd_pkg
    return amd_pkg.load()


@pytest.fixture(scope="module")
def lib(pkg):
    from ts_asr_whisper_amd import _lib
    return _lib


def plans_for(V):
    return (0, 1, 2) if V <= 65536 else (0, 2)


_SCORES = {}


def make_scores(rows, V, special=True, variant=0):
    """randn * 3 with -inf, -0.0 and +0.0 planted per row; with three rows or more, row 1 holds two finite scores and row 2 none.
    Computed once per shape and shared (read only)."""
    key = (rows, V, special, variant)
    if key not in _SCORES:
        g = torch.Generator().manual_seed(1000 * rows + V + 100003 * variant)
        sc = torch.randn(rows, V, generator=g) * 3.0
        for r in range(rows):
            if V >= 4:
                sc[r, (3 * r) % V], sc[r, (3 * r + 1) % V], sc[r, (3 * r + 2) % V] = -0.0, 0.0, -INF
        if special and rows >= 3:
            keep = sc[1, [V // 2, V - 1]].clone()
            sc[1] = -INF
            sc[1, [V // 2, V - 1]] = keep
            sc[2] = -INF
        _SCORES[key] = sc
    return _SCORES[key]


def scores_with_narrow_bands(rows, V, option_sets):
    """make_scores' first variant (of 8) on which, for every option set, at most 0.2 % of each row's tokens lie in the band -- a
    condition on the inputs that the oracle alone decides, on the CPU (check() asserts it again).  Below 500 tokens that means none."""
    for variant in range(8):
        sc = make_scores(rows, V, variant=variant)
        if V > 2000 or all((R.warp(sc.numpy(), **o).band.sum(axis=1) <= 0.002 * V).all() for o in option_sets):
            return sc
    raise AssertionError(f"no input variant with narrow bands for rows={rows} V={V}")


def bits(t):
    return torch.as_tensor(np.ascontiguousarray(t)).contiguous().view(torch.int32)


def launch(sc, plan, unfinished=None, want_logprob=True, want_warped=True, **opts):
    """One launch on guarded buffers.  Returns tokens, logprob, warped, flags (CPU tensors)."""
    from tests.util import guarded
    from ts_asr_whisper_amd.generation import sample_tokens
    rows, V = sc.shape
    g = guarded(sc.shape, V + 5, torch.float32, device=DEV, init=sc, name="scores")
    w = guarded(sc.shape, V + 3, torch.float32, device=DEV, name="warped") if want_warped else None
    wide = torch.full((rows, 5), SENT, dtype=torch.long, device=DEV)
    lp = torch.full((rows + 2,), 123.0, device=DEV) if want_logprob else None
    fl = None if unfinished is None else torch.as_tensor(unfinished, dtype=torch.bool).to(DEV)
    out = sample_tokens(g.view, out=wide[:, 2], logprob=None if lp is None else lp[1:rows + 1], warped=None if w is None else w.view,
                        unfinished=fl, plan=plan, **opts)
    assert out.data_ptr() == wide[:, 2].data_ptr()
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(bits(g.view.cpu()), bits(sc)), "the scores were written"
    wide = wide.cpu()
    assert (wide[:, [0, 1, 3, 4]] == SENT).all(), "a neighbour of `next` was written"
    if w is not None:
        w.check()
    if lp is not None:
        assert float(lp[0]) == 123.0 and float(lp[rows + 1]) == 123.0
    return NS(tokens=wide[:, 2].clone(), logprob=None if lp is None else lp[1:rows + 1].cpu(), warped=None if w is None else w.view.cpu(),
              flags=None if fl is None else fl.cpu())


def run(sc, unfinished=None, **opts):
    """Every plan; all outputs bit-identical between plans.  Returns the first plan's."""
    got = [launch(sc, p, unfinished=unfinished, **opts) for p in plans_for(sc.shape[1])]
    for p, o in zip(plans_for(sc.shape[1])[1:], got[1:]):
        assert torch.equal(o.tokens, got[0].tokens), f"plan {p}: tokens differ"
        assert torch.equal(bits(o.logprob), bits(got[0].logprob)), f"plan {p}: logprob bits differ"
        assert torch.equal(bits(o.warped), bits(got[0].warped)), f"plan {p}: warped bits differ"
        assert unfinished is None or torch.equal(o.flags, got[0].flags)
    return got[0]


def check(sc, what, unfinished=None, eos=-1, pad=0, **opts):
    """A launch under every plan against the oracle: kept mask (outside the band), warped bits, token, log-probability, flags."""
    got = run(sc, unfinished=unfinished, eos_token_id=eos, pad_token_id=pad, **opts)
    o = R.sample(sc.numpy(), unfinished=unfinished, eos=eos, pad=pad,
                 **{k: v for k, v in opts.items() if k in ("temperature", "top_k", "top_p", "min_p", "seed", "step", "stream", "row_ids")})
    rows, V = sc.shape
    t = np.float32(opts.get("temperature", 0.0))
    y = (sc / float(t)) if t > 0 else sc                                   # torch's CPU division
    kept = got.warped.numpy() > -np.inf
    off = (kept != o.kept) & ~o.band
    assert not off.any(), f"{what}: kept mask differs from the oracle outside the band at {np.argwhere(off)[:4].tolist()}"
    assert (o.band.sum(axis=1) <= 0.002 * V).all(), f"{what}: {o.band.sum(axis=1).max()} of {V} tokens in the band"
    flipped = (kept != o.kept)
    if flipped.any():                                                    # how far from the cut a fp32 mass moved a token (top_p only)
        with np.errstate(invalid="ignore"):
            d = np.abs(o.S - (1.0 - float(np.float32(opts.get("top_p", 1.0)))))[flipped]
        if np.isfinite(d).any():
            SEEN["flipped_mass"] = max(SEEN["flipped_mass"], float(np.nanmax(d)))
    kept_t = torch.from_numpy(kept)
    assert torch.equal(bits(got.warped)[kept_t], bits(y)[kept_t]), f"{what}: a kept entry of warped is not scores / t bit for bit"
    assert (got.warped[~kept_t] == -INF).all()
    live = np.ones(rows, bool) if unfinished is None else np.asarray(unfinished, bool)
    tok = got.tokens.numpy()
    empty = ~o.kept.any(axis=1)
    for r in range(rows):
        if not live[r]:
            assert tok[r] == pad and float(got.logprob[r]) == 0.0, f"{what}: finished row {r}"
            continue
        if empty[r]:
            assert tok[r] == eos and np.isnan(float(got.logprob[r])), f"{what}: row {r} without finite scores"
            continue
        assert 0 <= tok[r] < V and kept[r, tok[r]] and (o.kept[r, tok[r]] or o.band[r, tok[r]]), f"{what}: row {r} drew outside the kept set"
        SEEN["draws"] += int(t > 0)
        decisive = o.gap[r] > 1e-4 * max(1.0, abs(o.keys[r, o.tokens[r]])) and not flipped[r].any()
        if decisive or t <= 0:
            assert tok[r] == o.tokens[r], f"{what}: row {r} drew {tok[r]}, the oracle {o.tokens[r]} (gap {o.gap[r]:.3e})"
        else:
            SEEN["close_calls"] += 1
            assert tok[r] in (o.tokens[r], o.second[r]) or flipped[r].any(), f"{what}: row {r} drew {tok[r]}, not one of the oracle's two best"
        if tok[r] == o.tokens[r] and not flipped[r].any():
            err = abs(float(got.logprob[r]) - o.logprob[r])
            SEEN["logprob_err"] = max(SEEN["logprob_err"], err)
            assert err <= R.LOGPROB_REL * abs(o.logprob[r]) + R.LOGPROB_ABS, f"{what}: row {r} logprob {float(got.logprob[r])} vs {o.logprob[r]}"
    if unfinished is not None:
        assert got.flags.numpy().tolist() == (live & (tok != eos)).tolist(), f"{what}: flags"
    return got, o


# ------------------------------------------------------------------------------------------------ the argmax rung
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_argmax_rung(pkg, V, rows):
    sc = make_scores(rows, V).clone()
    top = float(sc[sc > -INF].max()) + 1.0 if (sc > -INF).any() else 1.0
    if V > 1:
        alone = sc.clone()
        alone[0, V - 1] = top                                            # the maximum at index V - 1 alone
        assert check(alone, f"argmax last V={V} rows={rows}")[0].tokens[0] == V - 1
        sc[0, V - 1] = top                                               # ... and planted twice: at index 0 as well
    sc[0, 0] = top
    got, o = check(sc, f"argmax V={V} rows={rows}")
    assert got.tokens[0] == 0
    want = torch.where((sc > -INF).any(1), sc.argmax(-1), torch.tensor(-1))
    assert torch.equal(got.tokens, want)
    # the bookkeeping of the decoding loop on scripted flags: where(unfinished, nxt, pad) and unfinished & (nxt != eos)
    eos = int(got.tokens[0])
    flags = [(r % 3) != 1 for r in range(rows)]
    got2, _ = check(sc, f"argmax flags V={V} rows={rows}", unfinished=flags, eos=eos, pad=max(V - 2, 0))
    fl = torch.tensor(flags)
    nxt = torch.where((sc > -INF).any(1), sc.argmax(-1), torch.tensor(eos))
    assert torch.equal(got2.tokens, torch.where(fl, nxt, torch.tensor(max(V - 2, 0))))
    assert torch.equal(got2.flags, fl & (nxt != eos))
    # argmax only: no logprob, no warped
    for plan in plans_for(V):
        assert torch.equal(launch(sc, plan, want_logprob=False, want_warped=False).tokens, got.tokens)


# ------------------------------------------------------------------------------------------------ top_k
def hf_top_k(sc, t, k):
    from transformers.generation.logits_process import TopKLogitsWarper
    return TopKLogitsWarper(top_k=k, min_tokens_to_keep=1)(torch.zeros(sc.shape[0], 1, dtype=torch.long), (sc / t).clone())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_top_k(pkg, V, rows):
    sc = make_scores(rows, V)
    for i, k in enumerate(sorted({1, 2, 50, V - 1, V, V + 7} - {0})):
        for j, t in enumerate((0.2, 0.7, 1.0, 1.3)):
            if V > 2000 and (i + j) % 2:                                 # (the wide rows: half of the grid, every k and every t in it)
                continue
            got, _ = check(sc, f"top_k={k} t={t} V={V} rows={rows}", temperature=t, top_k=k, seed=5, step=i, stream=j)
            assert torch.equal(bits(got.warped), bits(hf_top_k(sc, t, k))), f"top_k={k} t={t}: warped is not transformers' TopKLogitsWarper"


@pytest.mark.parametrize("V", [65, 1025, 51866])
def test_top_k_tie_across_the_kth_value(pkg, V):
    sc = make_scores(3, V, special=False).clone()
    for k in (2, 50):
        if k >= V:
            continue
        kth = torch.sort(sc[0], descending=True)[0][k - 1]
        lower = torch.nonzero(sc[0] < kth)[:3, 0]
        sc[0, lower] = kth                                               # three more tokens tie with the k-th value: all stay
        got, o = check(sc, f"tie k={k} V={V}", temperature=0.7, top_k=k, seed=1)
        assert int((got.warped[0] > -INF).sum()) == k + 3
        assert torch.equal(bits(got.warped), bits(hf_top_k(sc, 0.7, k)))
    few = torch.full((2, V), -INF)
    few[0, [1, V - 2]] = torch.tensor([0.5, -0.25])                       # fewer than k finite scores: nothing finite is removed
    got, _ = check(few, f"few finite V={V}", temperature=1.3, top_k=50, seed=2)
    assert (got.warped[0] > -INF).sum() == 2 and (got.warped[1] == -INF).all()


# ------------------------------------------------------------------------------------------------ top_p and min_p
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_top_p_and_min_p(pkg, V, rows):
    cases = []
    for k in (0, 50):
        cases += [dict(top_k=k, top_p=p) for p in (1e-6, 0.5, 0.9, 0.99)] + [dict(top_k=k, min_p=mp) for mp in (0.01, 0.3)]
    cases.append(dict(top_k=50, top_p=0.9, min_p=0.01))
    cases = [dict(temperature=(0.7, 1.0, 1.3)[n % 3], **c) for n, c in enumerate(cases)]
    sc = scores_with_narrow_bands(rows, V, cases)
    for n, c in enumerate(cases):
        got, o = check(sc, f"{c} V={V} rows={rows}", seed=7, step=n, **c)
        if c.get("top_p") == 1e-6:                                       # only the maximum (and what ties with it)
            assert ((got.warped > -INF).sum(1) == ((sc == sc.max(1, keepdim=True)[0]) & (sc > -INF)).sum(1)).all()


def test_top_p_tie_class_goes_or_stays_as_a_whole(pkg):
    sc = torch.tensor([[2.0, 1.0, 1.0, 1.0, 0.0, -1.0, 1.0, -INF]])
    got, o = check(sc, "tie class", temperature=1.0, top_p=0.6, seed=3)   # 2.0 holds 0.36, the four 1.0 0.53: the class stays
    assert (got.warped[0] > -INF).tolist() == [True, True, True, True, False, False, True, False]
    got, o = check(sc, "tie class", temperature=1.0, top_p=0.3, seed=3)
    assert (got.warped[0] > -INF).tolist() == [True] + [False] * 7


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_draw_equals_the_oracle(pkg, V, rows):
    option_sets = (dict(temperature=1.0), dict(temperature=0.7, top_k=50), dict(temperature=1.3, top_p=0.9))
    sc = scores_with_narrow_bands(rows, V, option_sets)
    steps = 8 if V > 2000 else 4
    for s in range(steps):
        for opts in option_sets:
            check(sc, f"draw {opts} step {s} V={V} rows={rows}", seed=2 ** 40 + 7, step=s, stream=3, row_ids=list(range(10, 10 + rows)), **opts)


@pytest.mark.parametrize("V", [1000, 51866])
def test_draw_depends_on_every_coordinate_and_on_nothing_else(pkg, V):
    rows = 16
    sc = make_scores(rows, V, special=False)
    base = dict(temperature=1.0, seed=99, step=4, stream=1, row_ids=list(range(rows)))
    ref = run(sc, **base)
    for change in (dict(seed=100), dict(step=5), dict(stream=2), dict(row_ids=list(range(1, rows + 1)))):
        assert not torch.equal(run(sc, **{**base, **change}).tokens, ref.tokens), f"the draws do not depend on {list(change)}"
    assert torch.equal(run(sc, **{**base, "row_ids": None}).tokens, ref.tokens)               # (row_ids NULL: the row index)
    sub = [11, 2, 7]                                                     # a subset launched alone, same ids: identical bits
    part = run(sc[sub].contiguous(), **{**base, "row_ids": sub})
    assert torch.equal(part.tokens, ref.tokens[sub]) and torch.equal(bits(part.logprob), bits(ref.logprob[sub]))
    assert torch.equal(bits(part.warped), bits(ref.warped[sub]))


@pytest.mark.parametrize("t,top_k", [(0.7, 0), (1.3, 3)])
def test_frequencies(pkg, t, top_k):
    """65 536 draws from fixed logits (4096 identical rows, row ids 0 .. 4095, steps 0 .. 15): every token's count within 4 standard
    deviations of N p (1 - p), p in fp64; the oracle itself reaches |z| <= 1.9 (tests/test_host_sampling.py)."""
    from ts_asr_whisper_amd.generation import sample_tokens
    logits = torch.tensor([1.5, -0.5, 0.25, -INF, 2.0, 0.0, -1.25, 0.75])
    rows, steps = 4096, 16
    x = logits.repeat(rows, 1).to(DEV)
    rid = torch.arange(rows, device=DEV)
    o0 = R.warp(logits[None].numpy(), t, top_k)
    e = np.where(o0.kept[0], np.exp(o0.y[0].astype(np.float64) - o0.y[0].max()), 0.0)
    p = e / e.sum()
    draws = torch.stack([sample_tokens(x, temperature=t, top_k=top_k, seed=1234, step=s, row_ids=rid) for s in range(steps)]).cpu().numpy()
    want = np.stack([R.sample(x.cpu().numpy(), t, top_k, seed=1234, step=s, row_ids=np.arange(rows)).tokens for s in (0, 15)])
    assert (draws[[0, 15]] != want).mean() < 0.01                         # (the oracle's own draws, but for close calls)
    counts = np.bincount(draws.reshape(-1), minlength=8)
    assert counts[~o0.kept[0]].sum() == 0, "a draw outside the kept set"
    N = draws.size
    z = (counts - N * p)[p > 0] / np.sqrt(N * p * (1 - p))[p > 0]
    print(f"frequencies t={t} top_k={top_k}: max |z| {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 4.0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(pkg, lib):
    from ts_asr_whisper_amd.generation import sample_tokens
    sc = torch.zeros(2, 70000, device=DEV)
    with pytest.raises(lib.DicowError, match="DICOW_SAMPLE_REG_MAX_V"):
        sample_tokens(sc, plan=lib.SAMPLE_REG)
    with pytest.raises(lib.DicowError, match="plan 3 is not 0 .. 2"):
        sample_tokens(sc, plan=3)
    import ctypes as C
    a = lib.SampleArgs(scores=sc.data_ptr(), ld=70000, rows=-1, V=70000)
    assert lib.lib().dicow_sample_tokens(C.byref(a), None) == -1 and b"rows=-1" in lib.lib().dicow_last_error()
    with pytest.raises(lib.DicowError):
        sample_tokens(sc.cpu())
    with pytest.raises(lib.DicowError):
        sample_tokens(sc, out=torch.zeros(2, dtype=torch.int32, device=DEV))


def test_zz_figures():
    """(last in this module) the figures the module saw, and the share of close calls among all draws."""
    print("sampling kernel figures:", SEEN)
    assert SEEN["draws"] == 0 or SEEN["close_calls"] <= max(1, 0.01 * SEEN["draws"]), SEEN

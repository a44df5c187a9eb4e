"""Is the difference real?  Bootstrap intervals and paired significance for error rates, on the GPU (csrc/bootstrap.hip).

Every score of ``scoring.py`` is a ratio of summed integer counts -- errors over reference length -- and the decisions taken on them are
differences of two such ratios on a dev set of a few dozen sessions whose lengths differ tenfold.  Three standard answers reduce to one
primitive, sums of count columns over many random multisets of units, which ``dicow_bootstrap_sums`` computes for all replicates in one
launch (exact integers, a counter-based generator: the sums depend on ``(seed, replicate, slot)`` alone, never on the launch plan):

  * ``bootstrap_sums``            the launch: int64 ``[n, C]`` table of counts -> int64 ``[R, C]`` replicate sums, on the device
  * ``ratio_interval``            a bootstrap percentile interval and standard error of ``sum(num) / sum(den)`` over the resampling unit
  * ``compare_ratios``            two systems on the same units: the paired bootstrap of the difference on shared draws (Bisani & Ney's
    probability of improvement) and the paired approximate-randomisation test, which exchanges the two systems' counts unit by unit
  * ``session_metric_intervals``, ``compare_session_metrics``     over the dicts of ``session_metrics``: the unit is the SESSION
  * ``wer_interval``, ``compare_wer``                             over the ``[n, 5]`` tables of ``word_error_counts``: the unit is the utterance

The host side downloads the replicate sums once and does the rest in float64 (``percentile_interval``, ``ratio_statistics``,
``comparison_statistics``: plain numpy, usable on sums from anywhere).  The percentile rule, the multiply-high index mapping with its bias
bound (include/dicow_hip.h) and the tie handling are the project's own; they are pinned to no library.  Nothing else in
the package calls these implicitly.  No CPU fallback."""
import math
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .scoring import _check_metrics, aggregate_session_metrics

_MODES = {"resample": L.BOOT_RESAMPLE, "swap": L.BOOT_SWAP}
_strata_cache = {}                     # (device, offsets) -> the offsets on the device: uploaded once, so that a later call can be captured


def _offsets(strata, n: int, who: str) -> np.ndarray:
    offs = np.asarray([0, n] if strata is None else strata, dtype=np.int64).reshape(-1)
    if offs.size < 2 or offs[0] != 0 or offs[-1] != n:
        raise L.DicowError(f"{who}: strata are S + 1 ascending offsets from 0 to n = {n}, got {offs.tolist()[:8]}{' ...' if offs.size > 8 else ''}")
    if (np.diff(offs) <= 0).any():
        raise L.DicowError(f"{who}: stratum {int(np.argmax(np.diff(offs) <= 0))} is empty (or the offsets descend)")
    return np.ascontiguousarray(offs)


def check_sum_bound(n: int, lowest: int, highest: int, who: str = "bootstrap_sums") -> None:
    """The precondition of ``dicow_bootstrap_sums``: ``n * max|table| < 2^62``, from the table's smallest and largest entry."""
    if n * max(highest, -lowest) >= 1 << 62:
        raise L.DicowError(f"{who}: n * max|table| = {n} * {max(highest, -lowest)} is not below 2^62: the int64 sums could overflow")


def bootstrap_sums(table: torch.Tensor, replicates: int, seed: int = 0, strata=None, mode: str = "resample", first_replicate: int = 0,
                   plan: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``dicow_bootstrap_sums`` launch.  ``table``: int64 ``[n, C]`` on the GPU, last stride 1 (a row pitch above ``C`` is fine), one
    row per unit, one column per count; ``strata``: None, or ``S + 1`` ascending offsets ``0 .. n`` (units of one stratum are adjacent);
    ``mode``: ``"resample"`` (each replicate draws ``n_s`` units with replacement from every stratum) or ``"swap"`` (``C`` even: each unit's
    columns ``[0, C/2)`` and ``[C/2, C)`` are exchanged with probability 1/2).  Replicate ``first_replicate + row`` under ``seed`` is the
    same whatever the plan (0: the library's choice, 1 .. ``_lib.BOOT_PLANS``) and however the replicates are split into calls.  Returns
    int64 ``[replicates, C]`` on the device (``out``, if given: contiguous int64 of that shape).  Refused with ``DicowError``: CPU tensors,
    other dtypes, a last stride other than 1, ``n * max|table| >= 2^62`` (checked with one reduction; skipped while the stream is being
    captured, where the bound is the caller's to keep)."""
    who = "bootstrap_sums"
    if not torch.is_tensor(table) or not table.is_cuda:
        raise L.DicowError(f"{who}: table must be on the GPU (no CPU fallback)")
    if table.dtype != torch.int64 or table.dim() != 2:
        raise L.DicowError(f"{who}: table must be an int64 [n, C] tensor, got {table.dtype} {tuple(table.shape)}")
    n, C = table.shape
    if n < 1 or C < 1:
        raise L.DicowError(f"{who}: an empty table ({n} units, {C} columns)")
    if table.stride(1) != 1 or (n > 1 and table.stride(0) < C):
        raise L.DicowError(f"{who}: table must have a last stride of 1 and a row pitch of at least C, got strides {table.stride()}")
    if mode not in _MODES:
        raise L.DicowError(f"{who}: mode {mode!r} is neither 'resample' nor 'swap'")
    if mode == "swap" and C % 2:
        raise L.DicowError(f"{who}: swap mode exchanges the two halves of the columns, C = {C} is odd")
    R = int(replicates)
    if R < 0:
        raise L.DicowError(f"{who}: replicates = {R}")
    offs = _offsets(strata, n, who)
    capturing = torch.cuda.is_current_stream_capturing()
    if not capturing:
        check_sum_bound(n, *(int(v) for v in torch.aminmax(table)), who=who)
    if out is None:
        out = torch.empty((R, C), dtype=torch.int64, device=table.device)
    elif (not torch.is_tensor(out) or out.device != table.device or out.dtype != torch.int64 or tuple(out.shape) != (R, C)
          or not out.is_contiguous()):
        raise L.DicowError(f"{who}: out must be a contiguous int64 [{R}, {C}] tensor on the table's device")
    offs_dev = None
    if offs.size > 2 and mode == "resample":
        key = (table.device, offs.tobytes())
        offs_dev = _strata_cache.get(key)
        if offs_dev is None:
            if capturing:
                raise L.DicowError(f"{who}: these strata have not been used before; call once outside the capture so that they are uploaded")
            if len(_strata_cache) >= 64:
                _strata_cache.clear()
            offs_dev = _strata_cache[key] = torch.from_numpy(offs).to(table.device)
    with torch.cuda.device(table.device):
        L.call("dicow_bootstrap_sums", table.data_ptr(), table.stride(0) if n > 1 else C, n, C, offs.ctypes.data,
               L.ptr(offs_dev), offs.size - 1, R, int(first_replicate) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1), _MODES[mode], int(plan),
               out.data_ptr(), L.stream())
    return out


# ------------------------------------------------------------------------------------------------ the statistics, on the host

def percentile_interval(values, alpha: float = 0.05):
    """The percentile interval by order statistics, no interpolation: with ``v`` sorted ascending over the ``R'`` values,
    ``lo = v[floor(alpha/2 * R')]`` and ``hi = v[ceil((1 - alpha/2) * R') - 1]``.  ``alpha`` is read as the nearest fraction with a
    denominator up to 2^30 (0.05 is 1/20), so the two indices are exact integer arithmetic.  ``(nan, nan)`` for no values."""
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"percentile_interval: alpha = {alpha} is outside (0, 1)")
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    if v.size == 0:
        return float("nan"), float("nan")
    half = Fraction(alpha).limit_denominator(1 << 30) / 2
    return float(v[math.floor(half * v.size)]), float(v[math.ceil((1 - half) * v.size) - 1])


def _sd(v: np.ndarray) -> float:
    return float(np.std(v, ddof=1)) if v.size >= 2 else float("nan")


def ratio_statistics(sums, alpha: float = 0.05) -> dict:
    """``lo hi se replicates undefined`` of the rates ``sums[:, 0] / sums[:, 1]`` (float64) over replicate sums int64 ``[R, 2]``.  A
    replicate with a zero denominator is counted in ``undefined`` and left out; ``se`` is the sample standard deviation (ddof = 1)."""
    s = np.asarray(sums, dtype=np.int64).reshape(-1, 2)
    ok = s[:, 1] != 0
    v = s[ok, 0].astype(np.float64) / s[ok, 1].astype(np.float64)
    lo, hi = percentile_interval(v, alpha)
    return {"lo": lo, "hi": hi, "se": _sd(v), "replicates": int(s.shape[0]), "undefined": int((~ok).sum())}


def comparison_statistics(resampled, swapped, observed, alpha: float = 0.05) -> dict:
    """The paired statistics of two systems from replicate sums int64 ``[R, 4]`` with columns ``(num_a, den_a, num_b, den_b)``:
    ``resampled`` under shared draws, ``swapped`` under unit-wise exchanges, ``observed`` the four column totals.  A lower rate is better.
      delta = rate_a - rate_b, with the percentile interval ``lo hi`` and ``se`` of the resampled deltas (a replicate with a zero
        denominator is counted in ``undefined`` and left out);
      prob_a_better = the share of resampled replicates with delta_r < 0 plus half the share with delta_r == 0;
      p_value = (1 + #{|delta_r| >= |delta_obs|}) / (R + 1) over the swapped replicates, two-sided.
    Where the two denominators are equal in every replicate (one shared reference) the comparisons are made on the integers
    ``num_a - num_b``, so ties are exact; otherwise in float64 (and a swapped replicate with a zero denominator counts as extreme)."""
    res = np.asarray(resampled, dtype=np.int64).reshape(-1, 4)
    swp = np.asarray(swapped, dtype=np.int64).reshape(-1, 4)
    obs = [int(x) for x in np.asarray(observed, dtype=np.int64).reshape(4)]
    rate_a = obs[0] / obs[1] if obs[1] else float("nan")
    rate_b = obs[2] / obs[3] if obs[3] else float("nan")
    ok = (res[:, 1] != 0) & (res[:, 3] != 0)
    r = res[ok]
    d = r[:, 0].astype(np.float64) / r[:, 1].astype(np.float64) - r[:, 2].astype(np.float64) / r[:, 3].astype(np.float64)
    lo, hi = percentile_interval(d, alpha)
    if r.shape[0] == 0:
        prob = float("nan")
    elif (r[:, 1] == r[:, 3]).all():
        di = r[:, 0] - r[:, 2]
        prob = (int((di < 0).sum()) + 0.5 * int((di == 0).sum())) / r.shape[0]
    else:
        prob = (int((d < 0).sum()) + 0.5 * int((d == 0).sum())) / r.shape[0]
    if swp.shape[0] and obs[1] == obs[3] and (swp[:, 1] == swp[:, 3]).all():
        extreme = int((np.abs(swp[:, 0] - swp[:, 2]) >= abs(obs[0] - obs[2])).sum())
    else:
        sok = (swp[:, 1] != 0) & (swp[:, 3] != 0)
        s = swp[sok]
        ds = s[:, 0].astype(np.float64) / s[:, 1].astype(np.float64) - s[:, 2].astype(np.float64) / s[:, 3].astype(np.float64)
        extreme = int((np.abs(ds) >= abs(rate_a - rate_b)).sum()) + int((~sok).sum())
    return {"rate_a": rate_a, "rate_b": rate_b, "delta": rate_a - rate_b, "lo": lo, "hi": hi, "se": _sd(d), "prob_a_better": prob,
            "p_value": (1 + extreme) / (swp.shape[0] + 1), "replicates": int(res.shape[0]), "undefined": int((~ok).sum())}


# ------------------------------------------------------------------------------------------------ tables of counts -> launches -> statistics

def _column(x, device, who: str) -> torch.Tensor:
    t = torch.as_tensor(x)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise L.DicowError(f"{who}: counts are integers, got {t.dtype}")
    return t.reshape(-1).to(device=device, dtype=torch.int64)


def _table(columns, strata, device, who: str):
    """Columns of counts, one entry per unit -> (int64 [n, C] on the device with the units sorted by stratum label, offsets or None)."""
    cols = [_column(c, device, who) for c in columns]
    n = cols[0].numel()
    if n < 1 or any(c.numel() != n for c in cols):
        raise L.DicowError(f"{who}: the columns have {[c.numel() for c in cols]} units; they must agree and there must be one at least")
    table = torch.stack(cols, dim=1)
    if strata is None:
        return table, None
    labels = list(strata)
    if len(labels) != n:
        raise L.DicowError(f"{who}: {len(labels)} stratum labels for {n} units")
    _, inverse, counts = np.unique(np.asarray(labels), return_inverse=True, return_counts=True)
    order = np.argsort(inverse.reshape(-1), kind="stable")
    return table[torch.from_numpy(order).to(device)].contiguous(), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _device_of(x, device):
    return x.device if torch.is_tensor(x) and x.is_cuda else torch.device(device)


def ratio_interval(num, den, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None, device="cuda") -> dict:
    """A bootstrap interval of the rate ``sum(num) / sum(den)``.  ``num`` / ``den``: integer counts, one per unit (a tensor or a sequence);
    ``strata``: one label per unit, e.g. the corpus of a merged dev set -- every replicate then redraws each stratum on its own.  Returns
    ``rate lo hi se replicates undefined`` (``percentile_interval``, ``ratio_statistics``).  One launch, one download."""
    table, offs = _table((num, den), strata, _device_of(num, device), "ratio_interval")
    obs = table.sum(0).tolist()
    sums = bootstrap_sums(table, replicates, seed, offs).cpu().numpy()
    return {"rate": obs[0] / obs[1] if obs[1] else float("nan"), **ratio_statistics(sums, alpha)}


def _compare(table, offs, pairs, replicates, alpha, seed) -> list:
    """table: [n, C] with system A in the first half of the columns; pairs: (num, den) column indices into one half."""
    R, C = int(replicates), table.shape[1]
    both = torch.empty((2 * R, C), dtype=torch.int64, device=table.device)
    bootstrap_sums(table, R, seed, offs, "resample", out=both[:R])
    bootstrap_sums(table, R, seed, None, "swap", out=both[R:])
    obs = table.sum(0).cpu().numpy()
    both = both.cpu().numpy()
    out = []
    for num, den in pairs:
        cols = [num, den, C // 2 + num, C // 2 + den]
        out.append(comparison_statistics(both[:R][:, cols], both[R:][:, cols], obs[cols], alpha))
    return out


def compare_ratios(num_a, den_a, num_b, den_b, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None, device="cuda") -> dict:
    """Two systems on the same units.  Both sit in one table, so in every replicate they share the draws (resample mode) and their counts of
    a unit are exchanged together (swap mode).  Returns ``rate_a rate_b delta lo hi se prob_a_better p_value replicates undefined``
    (``comparison_statistics``).  Two launches, one download."""
    table, offs = _table((num_a, den_a, num_b, den_b), strata, _device_of(num_a, device), "compare_ratios")
    return _compare(table, offs, [(0, 1)], replicates, alpha, seed)[0]


def _prefixes(metrics_list, who):
    _check_metrics(metrics_list, who)
    return [m.split("_", maxsplit=1)[0] for m in metrics_list]


def _session_columns(rows, prefixes, who):
    cols = []
    for p in prefixes:
        for k in (f"{p}_errors", f"{p}_length"):
            try:
                cols.append([int(r[k]) for r in rows])
            except KeyError:
                raise L.DicowError(f"{who}: a session dict has no {k!r}; pass the dicts of session_metrics for the same metrics_list") from None
    return cols


def session_metric_intervals(session_dicts, metrics_list, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None,
                             device="cuda") -> dict:
    """``aggregate_session_metrics(session_dicts, metrics_list)`` with ``<p>_wer_lo``, ``<p>_wer_hi`` and ``<p>_wer_se`` added for every
    metric named.  The resampling unit is the session -- the utterances of one session share speakers, room and topic and are not
    independent -- and all metrics share the draws (one table, one launch, one download)."""
    rows = list(session_dicts)
    prefixes = _prefixes(metrics_list, "session_metric_intervals")
    out = aggregate_session_metrics(rows, metrics_list)
    if not prefixes:
        return out
    table, offs = _table(_session_columns(rows, prefixes, "session_metric_intervals"), strata, torch.device(device), "session_metric_intervals")
    sums = bootstrap_sums(table, replicates, seed, offs).cpu().numpy()
    for m, p in enumerate(prefixes):
        st = ratio_statistics(sums[:, 2 * m:2 * m + 2], alpha)
        out[f"{p}_wer_lo"], out[f"{p}_wer_hi"], out[f"{p}_wer_se"] = st["lo"], st["hi"], st["se"]
    return out


def compare_session_metrics(dicts_a, dicts_b, metrics_list, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None,
                            device="cuda") -> dict:
    """Two systems' ``session_metrics`` dicts, parallel lists over the same sessions -> ``{metric: comparison}`` with the keys of
    ``compare_ratios`` (``rate_a`` is system A's ``<p>_wer``).  Raises ``DicowError`` if a ``<p>_length`` differs between the two systems
    for a session: the reference must be the same."""
    a, b = list(dicts_a), list(dicts_b)
    who = "compare_session_metrics"
    prefixes = _prefixes(metrics_list, who)
    if len(a) != len(b):
        raise L.DicowError(f"{who}: {len(a)} sessions of system A against {len(b)} of system B")
    ca, cb = _session_columns(a, prefixes, who), _session_columns(b, prefixes, who)
    for m, p in enumerate(prefixes):
        for i, (x, y) in enumerate(zip(ca[2 * m + 1], cb[2 * m + 1])):
            if x != y:
                raise L.DicowError(f"{who}: session {i} has {p}_length {x} for system A and {y} for system B: not the same reference")
    if not prefixes:
        return {}
    table, offs = _table(ca + cb, strata, torch.device(device), who)
    stats = _compare(table, offs, [(2 * m, 2 * m + 1) for m in range(len(prefixes))], replicates, alpha, seed)
    return dict(zip(metrics_list, stats))


def _wer_columns(counts, who):
    c = torch.as_tensor(counts)
    if c.dim() != 2 or c.shape[1] != 5 or c.dtype.is_floating_point:
        raise L.DicowError(f"{who}: expected the integer [n, 5] table of word_error_counts, got {c.dtype} {tuple(c.shape)}")
    return c[:, 0], c[:, 1] + c[:, 2] + c[:, 3]


def wer_interval(counts, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None, device="cuda") -> dict:
    """``ratio_interval`` over the ``[n, 5]`` table of ``word_error_counts``: errors (column 0) over the reference length (hits +
    substitutions + deletions).  The unit is the utterance."""
    num, den = _wer_columns(counts, "wer_interval")
    return ratio_interval(num, den, replicates, alpha, seed, strata, device)


def compare_wer(counts_a, counts_b, replicates: int = 10000, alpha: float = 0.05, seed: int = 0, strata=None, device="cuda") -> dict:
    """``compare_ratios`` over two systems' ``word_error_counts`` tables for the same utterances."""
    (na, da), (nb, db) = _wer_columns(counts_a, "compare_wer"), _wer_columns(counts_b, "compare_wer")
    return compare_ratios(na, da, nb, db, replicates, alpha, seed, strata, device)

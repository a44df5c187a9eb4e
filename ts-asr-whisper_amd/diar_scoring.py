"""Scoring the diarization the model is conditioned on: DER with its shares, JER, the speaker-count error and the DER-optimal speaker
mapping, from two ``SpeakerSegments`` (csrc/diar_score.hip).

Mirrors what the reference's ``utils/compute_der_between_cutsets.py`` and ``utils/align_and_compute_der_between_cutsets.py`` get from
pyannote.metrics (``DiarizationErrorRate``, ``JaccardErrorRate``, ``optimal_mapping``) and print per corpus (``MSCE JER DER Miss FA
Conf``).  Here a diarization stays the table it is -- sorted endpoints with one speaker bitmask each, in exact sample ticks -- and one
``dicow_diar_score`` call gives, for every (reference, hypothesis) pair of a corpus at once, the cooccurrence matrix ``C``, the speakers'
scored ticks ``R`` and ``H`` and the sums ``scored total missed false_alarm matched`` as int64; no per-sample mask exists anywhere.  The
assignment (``scoring.hungarian``) and the few divisions are host work on those integers.

  * ``unscored_intervals``     the collar: ``collar`` seconds removed around every boundary of every reference segment
  * ``diar_score_counts``      one ``dicow_diar_score`` call on a list of problems -> int64 ``[P, 4232]``
  * ``split_counts``           that row as a dict ``C R H scored total missed false_alarm matched``
  * ``mapping_from_counts`` / ``error_from_counts`` / ``jaccard_from_counts``   the formulas, on such a dict
  * ``diarization_error`` / ``jaccard_error`` / ``optimal_mapping``             one pair
  * ``score_diarizations`` / ``aggregate_diarization_scores``                   a corpus in one call, and the line the reference prints

pyannote is not a dependency and was not installed while this was written, so the following are RESTATED from pyannote.metrics'
documentation and not pinned by a golden: the collar convention (``collar`` is the full width, half before and half after a boundary); a
speaker who overlaps their own segments counts once here (the table is a union) where pyannote counts tracks; ``total == 0`` gives a
rate of 0.0 when nothing is wrong and 1.0 otherwise; a mapped pair without cooccurrence is no pair (left out of the mapping, a Jaccard
error of 1.0); and which of several equally good assignments is taken -- DER does not depend on that, JER and the mapping can.
No CPU fallback.
"""
import numpy as np
import torch

from . import _lib as L
from . import ops
from .diar_front_end import SpeakerSegments, _device
from .scoring import hungarian

RATE = 16000
SCALARS = ("scored", "total", "missed", "false_alarm", "matched")


def unscored_intervals(ref: SpeakerSegments, collar: float) -> np.ndarray:
    """int64 ``[n, 2]``: the sorted disjoint half-open tick intervals pyannote's ``collar`` takes out of scoring -- ``[b - h, b + h)`` around
    every boundary ``b`` of every raw interval of ``ref`` (not of the union table: the boundary between two touching segments of one
    speaker keeps its collar), ``h = round(collar * 16000 / 2)``, clipped at 0 and merged where they overlap or touch."""
    h = int(round(float(collar) * RATE / 2))
    if h < 0:
        raise ValueError(f"unscored_intervals: negative collar {collar}")
    if h == 0:
        return np.zeros((0, 2), np.int64)
    pts = sorted({b for iv in ref.intervals.values() for ab in iv for b in ab})
    out = []
    for b in pts:
        lo, hi = max(0, b - h), b + h
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return np.asarray(out, np.int64).reshape(-1, 2)


def diar_score_counts(problems, chunk: int = 0, device="cuda", out=None) -> torch.Tensor:
    """One ``dicow_diar_score`` call.  ``problems``: a list of ``(ref, hyp, unscored, skip_overlap)``; ``ref`` and ``hyp`` are
    ``SpeakerSegments`` or ``(bounds int64 [E + 1], active uint64 [E], S)`` triples, ``unscored`` an int64 ``[n, 2]`` array (or None).
    Returns the int64 ``[P, DIAR_SCORE_OUT_WORDS]`` tensor on the device (include/dicow_hip.h has the layout; ``split_counts`` reads a
    row).  ``chunk``: regions per workgroup (0: the library's ``DICOW_DIAR_SCORE_CHUNK``, also the most it takes; profiles/diar_score.txt
    has the chunks that were measured); the result does not depend on it."""
    dev = _device(device)
    b, a, u, pt = pack_problems(problems)
    P = pt.shape[0]
    if out is None:
        out = torch.empty((P, L.DIAR_SCORE_OUT_WORDS), dtype=torch.int64, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != (P, L.DIAR_SCORE_OUT_WORDS) or not out.is_cuda
          or not out.is_contiguous()):
        raise L.DicowError(f"diar_score_counts: out must be a contiguous int64 [{P}, {L.DIAR_SCORE_OUT_WORDS}] tensor on the GPU")
    if P == 0:
        return out
    dev = out.device
    tables = table_args(b, a, u, pt, chunk)
    with torch.cuda.device(dev):
        ws, nbytes = ops.table_workspace("diar_score_counts", L.lib().dicow_diar_score_ws_bytes, *tables, device=dev)
        L.call("dicow_diar_score", *tables, out.data_ptr(), ws.data_ptr(), nbytes, L.stream())
    diar_score_counts._tables = (b, a, u, pt)                        # (kept: the stream may read the host arrays after the call returns)
    return out


def table_args(b, a, u, pt, chunk: int = 0) -> tuple:
    """The nine leading arguments of ``dicow_diar_score`` / ``dicow_diar_score_ws_bytes`` for the arrays of ``pack_problems`` (which the
    caller keeps alive until the stream has read them)."""
    return (b.ctypes.data if len(b) else None, len(b), a.ctypes.data if len(a) else None, len(a), u.ctypes.data if len(u) else None, len(u),
            pt.ctypes.data if len(pt) else None, len(pt), int(chunk))


def pack_problems(problems) -> tuple:
    """The host tables of ``dicow_diar_score`` for a list of ``(ref, hyp, unscored, skip_overlap)`` (see ``diar_score_counts``): ``bounds``
    int64, ``active`` uint64, ``unscored`` int64 ``[n, 2]`` and ``problems`` int64 ``[P, DIAR_SCORE_ROW]``, every table back to back."""
    bounds, active, uns, rows = [], [], [], []
    nb = na = nu = 0
    for ref, hyp, unscored, skip in problems:
        row = []
        for t in (ref, hyp):
            b, a, S = (t.bounds, t.active, t.S) if isinstance(t, SpeakerSegments) else t
            b, a = np.ascontiguousarray(b, np.int64).reshape(-1), np.ascontiguousarray(a, np.uint64).reshape(-1)
            if b.shape[0] != a.shape[0] + 1:
                raise L.DicowError(f"diar_score_counts: {b.shape[0]} bounds for {a.shape[0]} entries (E + 1 wanted)")
            row += [nb, na, a.shape[0], int(S)]
            bounds.append(b)
            active.append(a)
            nb, na = nb + b.shape[0], na + a.shape[0]
        u = np.zeros((0, 2), np.int64) if unscored is None else np.ascontiguousarray(unscored, np.int64).reshape(-1, 2)
        rows.append(row + [nu, u.shape[0], int(bool(skip)), 0])
        uns.append(u)
        nu += u.shape[0]
    b = np.ascontiguousarray(np.concatenate(bounds)) if nb else np.zeros(0, np.int64)
    a = np.ascontiguousarray(np.concatenate(active)) if na else np.zeros(0, np.uint64)
    u = np.ascontiguousarray(np.concatenate(uns)) if nu else np.zeros((0, 2), np.int64)
    return b, a, u, np.asarray(rows, np.int64).reshape(len(rows), L.DIAR_SCORE_ROW)


def split_counts(row, Sr: int, Sh: int) -> dict:
    """One output row of ``dicow_diar_score`` (a CPU tensor or array of ``DIAR_SCORE_OUT_WORDS`` int64) as a dict: ``C`` int64 ``[Sr, Sh]``,
    ``R`` ``[Sr]``, ``H`` ``[Sh]`` and the Python ints ``scored total missed false_alarm matched``, all in ticks."""
    w = np.asarray(row, np.int64).reshape(-1)
    d = {"C": w[:4096].reshape(64, 64)[:Sr, :Sh].copy(), "R": w[4096:4096 + Sr].copy(), "H": w[4160:4160 + Sh].copy()}
    d.update({k: int(w[4224 + i]) for i, k in enumerate(SCALARS)})
    return d


def mapping_from_counts(counts) -> dict:
    """``{ref index: hyp index}``: the one-to-one assignment that maximises the summed cooccurrence (``scoring.hungarian`` on ``-C`` padded
    with zeros to a square), keeping only the pairs with ``C > 0``."""
    C = np.asarray(counts["C"], np.int64)
    Sr, Sh = C.shape
    n = max(Sr, Sh)
    if n == 0:
        return {}
    cost = np.zeros((n, n), np.int64)
    cost[:Sr, :Sh] = -C
    col = hungarian(cost)
    return {i: col[i] for i in range(Sr) if col[i] < Sh and C[i, col[i]] > 0}


def error_from_counts(counts, mapping=None) -> dict:
    """pyannote's ``DiarizationErrorRate`` components in seconds (ticks / 16000): ``total correct missed detection false alarm confusion
    diarization error rate``.  ``correct`` = the mapped cooccurrence, ``confusion`` = ``matched - correct``; with ``total == 0`` the rate
    is 0.0 when nothing is wrong and 1.0 otherwise."""
    d = _error_ticks(counts, mapping)
    out = {k: d[k] / RATE for k in ("total", "correct", "missed detection", "false alarm", "confusion")}
    out["diarization error rate"] = _rate(d["missed detection"] + d["false alarm"] + d["confusion"], d["total"])
    return out


def _error_ticks(counts, mapping=None) -> dict:
    mapping = mapping_from_counts(counts) if mapping is None else mapping
    correct = sum(int(counts["C"][i][j]) for i, j in mapping.items())
    return {"total": int(counts["total"]), "correct": correct, "missed detection": int(counts["missed"]),
            "false alarm": int(counts["false_alarm"]), "confusion": int(counts["matched"]) - correct}


def _rate(errors: int, total: int) -> float:
    return errors / total if total else (0.0 if errors == 0 else 1.0)


def jaccard_from_counts(counts, mapping=None) -> dict:
    """pyannote's ``JaccardErrorRate`` components: over the reference speakers with ``R > 0``, a speaker i mapped to j with ``C[i][j] > 0``
    adds ``(R[i] + H[j] - 2 C[i][j]) / (R[i] + H[j] - C[i][j])``, any other 1.0.  ``speaker error``, ``speaker count`` and ``jaccard error
    rate`` (0.0 without a scored reference speaker)."""
    mapping = mapping_from_counts(counts) if mapping is None else mapping
    C, R, H = counts["C"], counts["R"], counts["H"]
    err, n = 0.0, 0
    for i in range(len(R)):
        r = int(R[i])
        if r <= 0:
            continue
        n += 1
        j = mapping.get(i)
        c = int(C[i][j]) if j is not None else 0
        err += (r + int(H[j]) - 2 * c) / (r + int(H[j]) - c) if c > 0 else 1.0
    return {"speaker error": err, "speaker count": n, "jaccard error rate": err / n if n else 0.0}


def _n_speakers(segs: SpeakerSegments) -> int:
    return sum(1 for v in segs.intervals.values() if v)


def aggregate_diarization_scores(records) -> dict:
    """The corpus line the reference's scripts print, from per-recording dicts holding the keys of ``error_from_counts`` and
    ``jaccard_from_counts`` plus ``speaker count error``: ``DER Miss FA Conf`` from the summed components (the ``total == 0`` rule
    applies to the sums), ``JER`` = the summed speaker error over the summed speaker count, ``MSCE`` = the mean speaker-count error.
    The durations may be in any one unit: ``score_diarizations`` passes ticks, so its corpus rates are ratios of exact integers."""
    records = list(records)
    tot = {k: sum(r[k] for r in records) for k in ("total", "missed detection", "false alarm", "confusion", "speaker error", "speaker count")}
    miss, fa, conf, total = tot["missed detection"], tot["false alarm"], tot["confusion"], tot["total"]
    share = (lambda x: x / total) if total else (lambda x: 0.0 if x == 0 else 1.0)
    return {"MSCE": sum(r["speaker count error"] for r in records) / len(records) if records else 0.0,
            "JER": tot["speaker error"] / tot["speaker count"] if tot["speaker count"] else 0.0,
            "DER": share(miss + fa + conf), "Miss": share(miss), "FA": share(fa), "Conf": share(conf)}


def score_diarizations(pairs, collar: float = 0.0, skip_overlap: bool = False, device="cuda") -> dict:
    """A corpus: ``pairs`` is a list of ``(ref, hyp)`` ``SpeakerSegments``, scored as the problems of ONE ``dicow_diar_score`` call.
    Returns ``{"recordings": [...], "corpus": {...}, "mappings": [...]}``: per recording the keys of ``diarization_error`` and
    ``jaccard_error`` plus ``speaker count error`` (``|#ref - #hyp|`` over the speakers with a non-empty interval); the corpus line of
    ``aggregate_diarization_scores``; per recording the ``{hyp speaker: ref speaker}`` mapping of ``optimal_mapping`` (taken at this
    collar and ``skip_overlap``).  ``ref`` and ``hyp`` need not have the same length: nothing is active behind either end."""
    pairs = list(pairs)
    out = diar_score_counts([(r, h, unscored_intervals(r, collar), skip_overlap) for r, h in pairs], device=device).cpu().numpy()
    recs, ticks, maps = [], [], []
    for (r, h), row in zip(pairs, out):
        counts = split_counts(row, r.S, h.S)
        m = mapping_from_counts(counts)
        rec = error_from_counts(counts, m)
        rec.update(jaccard_from_counts(counts, m))
        rec["speaker count error"] = abs(_n_speakers(r) - _n_speakers(h))
        recs.append(rec)
        ticks.append(dict(rec, **_error_ticks(counts, m)))
        maps.append({h.speakers[j]: r.speakers[i] for i, j in m.items()})
    return {"recordings": recs, "corpus": aggregate_diarization_scores(ticks), "mappings": maps}


def _one(ref, hyp, collar, skip_overlap, device):
    row = diar_score_counts([(ref, hyp, unscored_intervals(ref, collar), skip_overlap)], device=device).cpu().numpy()[0]
    return split_counts(row, ref.S, hyp.S)


def diarization_error(ref: SpeakerSegments, hyp: SpeakerSegments, collar: float = 0.0, skip_overlap: bool = False, device="cuda") -> dict:
    """``error_from_counts`` of one pair: pyannote's ``total correct missed detection false alarm confusion`` in seconds and the
    ``diarization error rate``, under the optimal speaker mapping."""
    return error_from_counts(_one(ref, hyp, collar, skip_overlap, device))


def jaccard_error(ref: SpeakerSegments, hyp: SpeakerSegments, collar: float = 0.0, skip_overlap: bool = False, device="cuda") -> dict:
    """``jaccard_from_counts`` of one pair: ``speaker error``, ``speaker count``, ``jaccard error rate``."""
    return jaccard_from_counts(_one(ref, hyp, collar, skip_overlap, device))


def optimal_mapping(ref: SpeakerSegments, hyp: SpeakerSegments, collar: float = 0.0, device="cuda") -> dict:
    """``{hyp speaker: ref speaker}``: the DER-optimal relabelling of the hypothesis, pairs with cooccurrence only -- what the reference's
    ``align_and_compute_der_between_cutsets.py`` applies (``hyp.relabelled(mapping)``)."""
    m = mapping_from_counts(_one(ref, hyp, collar, False, device))
    return {hyp.speakers[j]: ref.speakers[i] for i, j in m.items()}

"""Scoring what was decoded, on the GPU: WER / CER per utterance batch and cpWER / tcpWER per session, over launches of csrc/edit_distance.hip.

The last step of the reference's evaluation loop.  It scores utterances with jiwer's ``compute_measures`` + ``cer``
(src/utils/evaluation.py:32-79) and sessions with meeteval's ``cpwer`` / ``tcpwer`` at a collar of 5 s (src/utils/wer.py:30-38, 89-97).
Here the words (or characters) become dense int32 ids on the host, every Levenshtein table of a metric runs in ONE launch of
``dicow_edit_distance`` -- one workgroup per pair -- and the host only adds up integers:

  * ``edit_counts``           the thin wrapper: flat id buffers + a host table of pairs -> ``(errors, hits, substitutions, deletions, insertions)``
  * ``Vocabulary``            tokens -> dense int32 ids (a host dict, built per call over reference and hypothesis together)
  * ``word_error_counts``     lists of strings, one pair per utterance, one launch; ``unit="word"`` or ``"char"``
  * ``error_measures``        jiwer's dictionary summed over the batch (``wer mer wil wip hits substitutions deletions insertions``) + ``cer``
  * ``make_compute_metrics``  the ``compute_metrics=`` callable for ``Seq2SeqTrainer`` with the reference's behaviour
  * ``cp_wer`` / ``tcp_wer``  one session: all R x H speaker pairs in one launch, the assignment by a small Hungarian solver on the host
  * ``pseudo_word_intervals`` / ``hungarian``   their two host pieces

The kernel's definition is exact: unit costs, and among the alignments with the fewest errors the one with the most hits.  ``errors``,
``length`` and every rate that is a function of them (``wer``, ``cer``, ``error_rate``) do not depend on how ties are split.

Restated from the documentation of jiwer and meeteval and NOT pinned to them (neither is installed where this was written):
  * jiwer's aggregate formulas: ``wer = (S+D+I)/(H+S+D)``, ``mer = (S+D+I)/(H+S+D+I)``, ``wip = (H/N_ref)(H/N_hyp)`` (0 for an empty hypothesis),
    ``wil = 1 - wip``; ``cer`` over the characters of the normalised strings, spaces included;
  * how substitutions / deletions / insertions are split among alignments with the same number of errors (here: most hits first;
    the libraries backtrace one alignment of their own choosing), which moves ``mer`` / ``wip`` / ``wil`` and the three counts, never ``errors``;
  * meeteval's pseudo-word timing for tcpWER: reference words split their segment's span in proportion to their character counts
    ("character_based"), hypothesis words become the centre points of such spans ("character_based_points"), the collar is added on both
    sides of the hypothesis intervals; here in integer ticks of 1 ms with boundaries floored (``pseudo_word_intervals``).

No CPU fallback: the ids are scored on the GPU or not at all.
"""
import re
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops

TICKS_PER_SECOND = 1000
_TIMESTAMP = re.compile(r"\<\|\d+\.\d+\|\>")


def edit_counts(ref_ids: torch.Tensor, hyp_ids: torch.Tensor, pairs, ref_iv: Optional[torch.Tensor] = None,
                hyp_iv: Optional[torch.Tensor] = None, lanes: int = 0, along: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``dicow_edit_distance`` launch.  ``ref_ids`` / ``hyp_ids``: flat contiguous int32 on the GPU; ``pairs``: int64 ``[n, 4]`` on the
    host, rows ``(ref_start, ref_len, hyp_start, hyp_len)`` (spans may be shared or overlap); ``ref_iv`` / ``hyp_iv``: int32 ``[len, 2]`` of
    (begin, end) ticks per id, both or neither.  Returns int64 ``[n, 5]`` on the CPU: ``(errors, hits, substitutions, deletions,
    insertions)``.  ``lanes`` / ``along``: the workgroup width and which sequence lies along the lanes, 0 = the library's choice; the
    result depends on neither.  ``out``: a contiguous int32 ``[n, 2]`` device tensor to receive ``(errors, hits)``."""
    for t, name in ((ref_ids, "ref_ids"), (hyp_ids, "hyp_ids")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.DicowError(f"edit_counts: {name} must be on the GPU (no CPU fallback)")
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise L.DicowError(f"edit_counts: {name} must be a flat contiguous int32 tensor")
    if hyp_ids.device != ref_ids.device:
        raise L.DicowError("edit_counts: ref_ids and hyp_ids are on different devices")
    if (ref_iv is None) != (hyp_iv is None):
        raise L.DicowError("edit_counts: intervals must be given for both sides or for neither")
    for iv, ids, name in ((ref_iv, ref_ids, "ref_iv"), (hyp_iv, hyp_ids, "hyp_iv")):
        if iv is not None and (not torch.is_tensor(iv) or iv.device != ids.device or iv.dtype != torch.int32 or tuple(iv.shape) != (ids.numel(), 2)
                               or not iv.is_contiguous()):
            raise L.DicowError(f"edit_counts: {name} must be a contiguous int32 [{ids.numel()}, 2] tensor on {ids.device}")
    table = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 4))
    n = table.shape[0]
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=ref_ids.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (n, 2) or out.device != ref_ids.device
          or not out.is_contiguous()):
        raise L.DicowError(f"edit_counts: out must be a contiguous int32 [{n}, 2] tensor on {ref_ids.device}")
    with torch.cuda.device(ref_ids.device):
        nbytes = L.lib().dicow_edit_distance_ws_bytes(table.ctypes.data if n else None, n)
        if nbytes < 0:
            raise L.DicowError(f"edit_counts: {L.lib().dicow_last_error().decode()}")
        ws = ops.workspace(nbytes, ref_ids.device)
        L.call("dicow_edit_distance", ref_ids.data_ptr(), ref_ids.numel(), hyp_ids.data_ptr(), hyp_ids.numel(), L.ptr(ref_iv), L.ptr(hyp_iv),
               table.ctypes.data if n else None, n, out.data_ptr(), int(lanes), int(along), ws.data_ptr(), nbytes, L.stream())
    return counts_from(out.cpu(), table)


def counts_from(eh, table) -> torch.Tensor:
    """``(errors, hits)`` int ``[n, 2]`` and the pair table -> int64 ``[n, 5]`` ``(E, H, S, D, I)``: ``I = E - N_ref + H``,
    ``D = E + H - N_hyp``, ``S = N_ref + N_hyp - 2 H - E``."""
    eh = torch.as_tensor(np.asarray(eh)).to(torch.int64).reshape(-1, 2)
    table = torch.as_tensor(np.asarray(table)).to(torch.int64).reshape(-1, 4)
    E, H, nr, nh = eh[:, 0], eh[:, 1], table[:, 1], table[:, 3]
    return torch.stack([E, H, nr + nh - 2 * H - E, E + H - nh, E - nr + H], dim=1)


class Vocabulary:
    """Tokens (words or characters) -> dense int32 ids, in order of first appearance.  Ids are only compared for equality."""

    def __init__(self):
        self.index = {}

    def ids(self, tokens) -> list:
        index = self.index
        return [index.setdefault(tok, len(index)) for tok in tokens]

    def __len__(self):
        return len(self.index)


def _default_norm(text: str) -> str:
    return " ".join(text.lower().split())


def _tokens(text: str, unit: str):
    if unit == "word":
        return text.split()
    if unit == "char":
        return list(text)
    raise ValueError(f"unit must be 'word' or 'char', got {unit!r}")


def _flat(streams, device):
    """Lists of ids -> (flat int32 device tensor, starts, lens)."""
    lens = [len(s) for s in streams]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if streams else np.zeros(0, np.int64)
    flat = np.fromiter((i for s in streams for i in s), dtype=np.int32, count=int(sum(lens)))
    return torch.from_numpy(flat).to(device), starts, np.asarray(lens, np.int64)


def word_error_counts(refs, hyps, text_norm: Optional[Callable] = None, unit: str = "word", device="cuda") -> torch.Tensor:
    """Lists of strings, one pair per utterance, one launch -> int64 ``[n, 5]`` ``(errors, hits, substitutions, deletions, insertions)``.
    ``text_norm``: str -> str, applied to both sides (default: lower case, whitespace collapsed); ``unit``: words split at whitespace, or
    the characters of the normalised string."""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f"word_error_counts: {len(refs)} references and {len(hyps)} hypotheses")
    norm = _default_norm if text_norm is None else text_norm
    vocab = Vocabulary()
    r = [vocab.ids(_tokens(norm(s), unit)) for s in refs]
    h = [vocab.ids(_tokens(norm(s), unit)) for s in hyps]
    rf, rs, rl = _flat(r, device)
    hf, hs, hl = _flat(h, device)
    return edit_counts(rf, hf, np.stack([rs, rl, hs, hl], axis=1) if refs else np.zeros((0, 4), np.int64))


def measures_from_counts(hits: int, substitutions: int, deletions: int, insertions: int) -> dict:
    """jiwer's aggregate measures from summed counts (module docstring: restated, not pinned)."""
    H, S, D, I = int(hits), int(substitutions), int(deletions), int(insertions)
    n_ref, n_hyp = H + S + D, H + S + I
    wip = (H / n_ref) * (H / n_hyp) if n_ref and n_hyp else 0.0
    return {"wer": (S + D + I) / n_ref if n_ref else float("nan"), "mer": (S + D + I) / (H + S + D + I) if H + S + D + I else 0.0,
            "wil": 1.0 - wip, "wip": wip, "hits": H, "substitutions": S, "deletions": D, "insertions": I}


def error_measures(refs, hyps, text_norm: Optional[Callable] = None, device="cuda") -> dict:
    """jiwer's ``compute_measures`` dictionary summed over the batch plus ``cer``: one launch on words, one on characters."""
    w = word_error_counts(refs, hyps, text_norm, "word", device).sum(0)
    c = word_error_counts(refs, hyps, text_norm, "char", device).sum(0)
    out = measures_from_counts(w[1], w[2], w[3], w[4])
    n_char = int(c[1] + c[2] + c[3])
    out["cer"] = int(c[0]) / n_char if n_char else float("nan")
    return out


def make_compute_metrics(tokenizer, text_norm: Optional[Callable] = None, decode_with_timestamps: bool = False, device="cuda") -> Callable:
    """The ``compute_metrics=`` callable for ``Seq2SeqTrainer(predict_with_generate=True)`` with the behaviour of the reference's
    ``compute_metrics`` (src/utils/evaluation.py:54-79): -100 becomes the pad id, ``batch_decode(skip_special_tokens=True, normalize=False,
    decode_with_timestamps=...)``, timestamp tokens ``<|12.34|>`` become a space, the label is stripped, ``text_norm`` is applied, an empty
    label becomes ``-``; returns ``error_measures`` of labels against predictions.  The reference's wandb table and ``predictions.csv``
    are left out.  ``text_norm`` (str -> str) is the caller's normaliser; the default lower-cases and collapses whitespace."""
    norm = _default_norm if text_norm is None else text_norm

    def compute_metrics(pred) -> dict:
        preds, labels = np.asarray(pred.predictions), np.asarray(pred.label_ids)
        preds = np.where(preds == -100, tokenizer.pad_token_id, preds)
        labels = np.where(labels == -100, tokenizer.pad_token_id, labels)
        kw = dict(skip_special_tokens=True, normalize=False, decode_with_timestamps=decode_with_timestamps)
        pred_str = [norm(_TIMESTAMP.sub(" ", s)) for s in tokenizer.batch_decode(preds, **kw)]
        label_str = [norm(_TIMESTAMP.sub(" ", s).strip()) for s in tokenizer.batch_decode(labels, **kw)]
        label_str = [s if s else "-" for s in label_str]
        return error_measures(label_str, pred_str, text_norm=lambda s: s, device=device)

    return compute_metrics


# ------------------------------------------------------------------------------------------------ sessions: cpWER and tcpWER

def _segment(seg):
    """(speaker, start_s, end_s, text) from a tuple or a dict with meeteval's SegLST keys."""
    if isinstance(seg, dict):
        return seg["speaker"], float(seg["start_time"]), float(seg["end_time"]), seg["words"]
    speaker, start, end, text = seg
    return speaker, float(start), float(end), text


def _ticks(seconds: float) -> int:
    return int(round(seconds * TICKS_PER_SECOND))


def pseudo_word_intervals(start_s: float, end_s: float, words, points: bool = False, collar_s: float = 0.0):
    """Integer-tick intervals ``[(begin, end)]`` of the words of one segment.  With ``L`` = the words' total character count and ``c_k`` the
    count up to and including word k, word k spans ``[s + (e - s) c_{k-1} // L, s + (e - s) c_k // L]`` where ``s``, ``e`` are the segment's
    ends rounded to ticks ("character_based").  ``points=True``: the centre ``(begin + end) // 2`` of that span as a zero-width interval
    ("character_based_points").  ``collar_s`` widens every interval on both sides."""
    s, e, c = _ticks(start_s), _ticks(end_s), _ticks(collar_s)
    total = sum(len(w) for w in words)
    out, cum = [], 0
    for w in words:
        b0 = s + (e - s) * cum // total
        cum += len(w)
        b1 = s + (e - s) * cum // total
        if points:
            b0 = b1 = (b0 + b1) // 2
        out.append((b0 - c, b1 + c))
    return out


def _streams(segments, points: bool, collar_s: float):
    """{speaker: (words, intervals)}: per speaker the segments sorted by start time, their words concatenated."""
    by = {}
    for seg in segments:
        spk, start, end, text = _segment(seg)
        by.setdefault(spk, []).append((start, end, text))
    out = {}
    for spk in sorted(by, key=str):
        words, ivs = [], []
        for start, end, text in sorted(by[spk], key=lambda x: x[0]):
            w = text.split()
            words += w
            ivs += pseudo_word_intervals(start, end, w, points, collar_s)
        out[spk] = (words, ivs)
    return out


def hungarian(cost) -> list:
    """Minimum-cost perfect assignment of a square integer matrix: ``col[i]`` for every row i.  The O(n^3) shortest-augmenting-path method
    with row / column potentials, in plain Python (n is a number of speakers)."""
    a = np.asarray(cost)
    n = a.shape[0]
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError("hungarian: the matrix must be square (pad it)")
    a = [[int(v) for v in row] for row in a]
    INF = float("inf")
    u, v, match, way = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)     # match[j]: the row of column j (1-based, 0 = free)
    for i in range(1, n + 1):
        match[0] = i
        j0, minv, used = 0, [INF] * (n + 1), [False] * (n + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = match[j0], INF, 0
            for j in range(1, n + 1):
                if not used[j]:
                    cur = a[i0 - 1][j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(n + 1):
                if used[j]:
                    u[match[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if match[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            match[j0] = match[j1]
            j0 = j1
    col = [0] * n
    for j in range(1, n + 1):
        col[match[j] - 1] = j - 1
    return col


def _session_wer(ref_segments, hyp_segments, timed: bool, collar: float, device) -> dict:
    ref = _streams(ref_segments, False, 0.0)
    hyp = _streams(hyp_segments, True, collar)
    rk, hk = list(ref), list(hyp)
    R, H = len(rk), len(hk)
    vocab = Vocabulary()
    rf, rs, rl = _flat([vocab.ids(ref[k][0]) for k in rk], device)
    hf, hs, hl = _flat([vocab.ids(hyp[k][0]) for k in hk], device)
    n = max(R, H)
    counts = np.zeros((n, n, 5), np.int64)                                  # (E, H, S, D, I); a missing speaker is an empty stream
    if R and H:
        table = np.array([(rs[i], rl[i], hs[j], hl[j]) for i in range(R) for j in range(H)], np.int64)
        riv = hiv = None
        if timed:
            riv = torch.tensor([iv for k in rk for iv in ref[k][1]], dtype=torch.int32).reshape(-1, 2).to(device)
            hiv = torch.tensor([iv for k in hk for iv in hyp[k][1]], dtype=torch.int32).reshape(-1, 2).to(device)
        counts[:R, :H] = edit_counts(rf, hf, table, riv, hiv).numpy().reshape(R, H, 5)
    for i in range(R):
        counts[i, H:, 0] = counts[i, H:, 3] = rl[i]                         # against nobody: all deleted
    for j in range(H):
        counts[R:, j, 0] = counts[R:, j, 4] = hl[j]                         # nobody's: all inserted
    col = hungarian(counts[:, :, 0]) if n else []
    tot = sum((counts[i, col[i]] for i in range(n)), np.zeros(5, np.int64))
    length = int(rl.sum())
    assignment = [(rk[i] if i < R else None, hk[col[i]] if col[i] < H else None) for i in range(n)]
    return {"error_rate": int(tot[0]) / length if length else None, "errors": int(tot[0]), "length": length, "insertions": int(tot[4]),
            "deletions": int(tot[3]), "substitutions": int(tot[2]), "missed_speaker": max(0, R - H), "falarm_speaker": max(0, H - R),
            "scored_speaker": R, "assignment": assignment}


def cp_wer(ref_segments, hyp_segments, device="cuda") -> dict:
    """Concatenated minimum-permutation WER of one session (meeteval's ``cpwer``).  Segments: ``(speaker, start_s, end_s, text)`` tuples or
    dicts with the SegLST keys ``speaker start_time end_time words``.  Per speaker the segments are sorted by start time and their words
    concatenated; all R x H streams pairs are scored in one launch; the speaker assignment with the fewest total errors is found on the
    host (a missing speaker on either side is an empty stream).  Returns ``error_rate errors length insertions deletions substitutions
    missed_speaker falarm_speaker scored_speaker assignment`` (``assignment``: ``(ref speaker | None, hyp speaker | None)`` pairs)."""
    return _session_wer(ref_segments, hyp_segments, False, 0.0, device)


def tcp_wer(ref_segments, hyp_segments, collar: float = 5.0, device="cuda") -> dict:
    """Time-constrained cpWER (meeteval's ``tcpwer``): as ``cp_wer``, but a reference word and a hypothesis word may be matched or
    substituted only if their intervals overlap -- ``pseudo_word_intervals`` in ticks of 1 ms, reference words as spans, hypothesis words
    as centre points widened by ``collar`` seconds on both sides."""
    return _session_wer(ref_segments, hyp_segments, True, collar, device)

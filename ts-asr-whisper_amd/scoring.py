"""Scoring what was decoded, on the GPU: WER / CER per utterance batch and cpWER / tcpWER per session, over launches of csrc/edit_distance.hip;
ORC-WER / tcORC-WER per session, over csrc/orc_distance.hip.

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
  * ``edit_alignments``       the edit path behind ``edit_counts``: ``dicow_edit_alignment`` over the pairs (csrc/edit_alignment.hip), split over
    several calls when the records would pass the workspace limit -> the counts and one uint8 tensor of ops per pair
  * ``word_alignments`` / ``alignment_chunks``   per utterance the chunks of jiwer's ``process_words(...).alignments``, with the batch's measures
  * ``session_alignment``     the data behind the reference's tcp alignment view (``calc_wer(save_visualizations=True)``, src/utils/wer.py:18-27,
    154-155): the assignment of ``tcp_wer`` / ``cp_wer``, then the assigned pairs aligned in one call, as rows of words and times
  * ``alignment_rows`` / ``format_alignment`` / ``error_breakdown`` / ``save_alignment_report``   ops against words, a three-line text rendering,
    the most frequent errors, one JSON file per session -- the project's own layouts
  * ``orc_counts``            the thin wrapper of ``dicow_orc_distance``: flat id buffers + three host tables -> the same five counts per problem
  * ``orc_wer`` / ``tcorc_wer``   one session, ungrouped: every reference utterance goes to whichever hypothesis stream suits it best
  * ``session_tcorc_wer``     the reference's recipe around meeteval's ``tcorcwer`` (src/utils/wer.py:41-86): empty segments out, a VAD mask,
    the session cut at silence into groups, never-overlapping hypothesis speakers merged; ALL groups in one ``dicow_orc_distance`` call
  * ``filter_empty_segments`` / ``create_vad_mask`` / ``find_group_splits`` / ``map_utterance_to_split`` / ``merge_streams`` /
    ``create_dummy_seg_list``   that recipe's host pieces (src/utils/wer_utils.py:45-138, src/utils/general.py:102-104), in plain numpy
  * ``session_orc_wer`` / ``session_metrics`` / ``aggregate_session_metrics``   the reference's score sheet (``calc_wer``,
    ``aggregate_wer_metrics``) as dicts instead of pandas frames

The kernel's definition is exact: unit costs, and among the alignments with the fewest errors the one with the most hits.  ``errors``,
``length`` and every rate that is a function of them (``wer``, ``cer``, ``error_rate``) do not depend on how ties are split.

Restated from the documentation of jiwer and meeteval and NOT pinned to them (neither is installed where this was written):
  * jiwer's aggregate formulas: ``wer = (S+D+I)/(H+S+D)``, ``mer = (S+D+I)/(H+S+D+I)``, ``wip = (H/N_ref)(H/N_hyp)`` (0 for an empty hypothesis),
    ``wil = 1 - wip``; ``cer`` over the characters of the normalised strings, spaces included;
  * how substitutions / deletions / insertions are split among alignments with the same number of errors (here: most hits first;
    the libraries backtrace one alignment of their own choosing), which moves ``mer`` / ``wip`` / ``wil`` and the three counts, never ``errors``;
  * which of several paths of equal counts an alignment shows (here: walking back, the diagonal where it attains the key, else the
    deletion, else the insertion; jiwer / rapidfuzz and meeteval may show another), and the renderings of ``format_alignment`` and
    ``save_alignment_report``, which are this project's own;
  * meeteval's pseudo-word timing for tcpWER: reference words split their segment's span in proportion to their character counts
    ("character_based"), hypothesis words become the centre points of such spans ("character_based_points"), the collar is added on both
    sides of the hypothesis intervals; here in integer ticks of 1 ms with boundaries floored (``pseudo_word_intervals``).
  * for ORC-WER / tcORC-WER (meeteval is not installed here, and the reference's wer_utils.py imports it at the top, so neither its
    helpers nor meeteval could be run against this): that an utterance is one reference segment; the sort orders (utterances and a
    stream's segments by start time, ties in input order; speakers grouped in order of first appearance for ``merge_streams``); the
    pseudo-word timing of tcORC-WER, taken to be that of tcpWER; the split of equal-error alignments into S / D / I; the choice among
    tied assignments; the stream label of a group scored against the dummy segment.  ``errors``, ``length`` and ``error_rate`` depend on
    none of these except the timing.

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


def _check_edit_inputs(who: str, ref_ids, hyp_ids, ref_iv, hyp_iv):
    """The refusals ``edit_counts``, ``edit_alignments`` and ``orc_counts`` share: flat contiguous int32 ids on one GPU, intervals for both sides or neither."""
    for t, name in ((ref_ids, "ref_ids"), (hyp_ids, "hyp_ids")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.DicowError(f"{who}: {name} must be on the GPU (no CPU fallback)")
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise L.DicowError(f"{who}: {name} must be a flat contiguous int32 tensor")
    if hyp_ids.device != ref_ids.device:
        raise L.DicowError(f"{who}: ref_ids and hyp_ids are on different devices")
    if (ref_iv is None) != (hyp_iv is None):
        raise L.DicowError(f"{who}: intervals must be given for both sides or for neither")
    for iv, ids, name in ((ref_iv, ref_ids, "ref_iv"), (hyp_iv, hyp_ids, "hyp_iv")):
        if iv is not None and (not torch.is_tensor(iv) or iv.device != ids.device or iv.dtype != torch.int32 or tuple(iv.shape) != (ids.numel(), 2)
                               or not iv.is_contiguous()):
            raise L.DicowError(f"{who}: {name} must be a contiguous int32 [{ids.numel()}, 2] tensor on {ids.device}")


def edit_counts(ref_ids: torch.Tensor, hyp_ids: torch.Tensor, pairs, ref_iv: Optional[torch.Tensor] = None,
                hyp_iv: Optional[torch.Tensor] = None, lanes: int = 0, along: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``dicow_edit_distance`` launch.  ``ref_ids`` / ``hyp_ids``: flat contiguous int32 on the GPU; ``pairs``: int64 ``[n, 4]`` on the
    host, rows ``(ref_start, ref_len, hyp_start, hyp_len)`` (spans may be shared or overlap); ``ref_iv`` / ``hyp_iv``: int32 ``[len, 2]`` of
    (begin, end) ticks per id, both or neither.  Returns int64 ``[n, 5]`` on the CPU: ``(errors, hits, substitutions, deletions,
    insertions)``.  ``lanes`` / ``along``: the workgroup width and which sequence lies along the lanes, 0 = the library's choice; the
    result depends on neither.  ``out``: a contiguous int32 ``[n, 2]`` device tensor to receive ``(errors, hits)``."""
    _check_edit_inputs("edit_counts", ref_ids, hyp_ids, ref_iv, hyp_iv)
    table = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 4))
    n = table.shape[0]
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=ref_ids.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (n, 2) or out.device != ref_ids.device
          or not out.is_contiguous()):
        raise L.DicowError(f"edit_counts: out must be a contiguous int32 [{n}, 2] tensor on {ref_ids.device}")
    with torch.cuda.device(ref_ids.device):
        ws, nbytes = ops.table_workspace("edit_counts", L.lib().dicow_edit_distance_ws_bytes, table.ctypes.data if n else None, n,
                                         device=ref_ids.device)
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


def _utterance_pairs(who: str, refs, hyps, text_norm, unit: str, device):
    """Lists of strings -> (flat ref ids, flat hyp ids, the pair table with one row per utterance, ref tokens, hyp tokens)."""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f"{who}: {len(refs)} references and {len(hyps)} hypotheses")
    norm = _default_norm if text_norm is None else text_norm
    vocab = Vocabulary()
    rt = [_tokens(norm(s), unit) for s in refs]
    ht = [_tokens(norm(s), unit) for s in hyps]
    r = [vocab.ids(t) for t in rt]                                           # (all references first, as before: ids are only compared)
    h = [vocab.ids(t) for t in ht]
    rf, rs, rl = _flat(r, device)
    hf, hs, hl = _flat(h, device)
    return rf, hf, (np.stack([rs, rl, hs, hl], axis=1) if refs else np.zeros((0, 4), np.int64)), rt, ht


def word_error_counts(refs, hyps, text_norm: Optional[Callable] = None, unit: str = "word", device="cuda") -> torch.Tensor:
    """Lists of strings, one pair per utterance, one launch -> int64 ``[n, 5]`` ``(errors, hits, substitutions, deletions, insertions)``.
    ``text_norm``: str -> str, applied to both sides (default: lower case, whitespace collapsed); ``unit``: words split at whitespace, or
    the characters of the normalised string."""
    rf, hf, table, _, _ = _utterance_pairs("word_error_counts", refs, hyps, text_norm, unit, device)
    return edit_counts(rf, hf, table)


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


def _session_score(ref_segments, hyp_segments, timed: bool, collar: float, device):
    """(the result of ``cp_wer`` / ``tcp_wer``, what ``session_alignment`` needs to align the assigned pairs: the streams, their flat
    buffers and the assignment ``col``)."""
    ref = _streams(ref_segments, False, 0.0)
    hyp = _streams(hyp_segments, True, collar)
    rk, hk = list(ref), list(hyp)
    R, H = len(rk), len(hk)
    vocab = Vocabulary()
    rf, rs, rl = _flat([vocab.ids(ref[k][0]) for k in rk], device)
    hf, hs, hl = _flat([vocab.ids(hyp[k][0]) for k in hk], device)
    n = max(R, H)
    counts = np.zeros((n, n, 5), np.int64)                                  # (E, H, S, D, I); a missing speaker is an empty stream
    riv = hiv = None
    if R and H:
        table = np.array([(rs[i], rl[i], hs[j], hl[j]) for i in range(R) for j in range(H)], np.int64)
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
    result = {"error_rate": int(tot[0]) / length if length else None, "errors": int(tot[0]), "length": length, "insertions": int(tot[4]),
              "deletions": int(tot[3]), "substitutions": int(tot[2]), "missed_speaker": max(0, R - H), "falarm_speaker": max(0, H - R),
              "scored_speaker": R, "assignment": assignment}
    return result, dict(ref=ref, hyp=hyp, rk=rk, hk=hk, rf=rf, hf=hf, rs=rs, rl=rl, hs=hs, hl=hl, riv=riv, hiv=hiv, col=col)


def _session_wer(ref_segments, hyp_segments, timed: bool, collar: float, device) -> dict:
    return _session_score(ref_segments, hyp_segments, timed, collar, device)[0]


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


# ------------------------------------------------------------------------------------------------ sessions: ORC-WER and tcORC-WER

def orc_counts(ref_ids: torch.Tensor, hyp_ids: torch.Tensor, problems, utts, streams, ref_iv: Optional[torch.Tensor] = None,
               hyp_iv: Optional[torch.Tensor] = None, want_assignment: bool = False, out: Optional[torch.Tensor] = None):
    """One ``dicow_orc_distance`` call.  ``ref_ids`` / ``hyp_ids`` / ``ref_iv`` / ``hyp_iv``: as for ``edit_counts``.  Host tables (int64):
    ``problems`` ``[n, 4]`` rows ``(utt_first, n_utts, stream_first, n_streams)``; ``utts`` ``[.., 2]`` rows ``(ref_start, ref_len)``, one
    reference utterance each, in spoken order; ``streams`` ``[.., 2]`` rows ``(hyp_start, hyp_len)``.  Returns int64 ``[n, 5]`` on the
    CPU, ``(errors, hits, substitutions, deletions, insertions)`` per problem; with ``want_assignment`` also an int32 tensor with one
    entry per row of ``utts``: the stream within its problem the utterance was given to (-1: the problem has no stream, or no problem
    names the row).  ``out``: a contiguous int32 ``[n, 2]`` device tensor to receive ``(errors, hits)``."""
    _check_edit_inputs("orc_counts", ref_ids, hyp_ids, ref_iv, hyp_iv)
    pt = np.ascontiguousarray(np.asarray(problems, dtype=np.int64).reshape(-1, 4))
    ut = np.ascontiguousarray(np.asarray(utts, dtype=np.int64).reshape(-1, 2))
    st = np.ascontiguousarray(np.asarray(streams, dtype=np.int64).reshape(-1, 2))
    n = pt.shape[0]
    if n and (pt.min() < 0 or (pt[:, 0] + pt[:, 1]).max() > len(ut) or (pt[:, 2] + pt[:, 3]).max() > len(st)):
        raise L.DicowError("orc_counts: a problem names rows outside the utterance or stream table")
    dev = ref_ids.device
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (n, 2) or out.device != dev or not out.is_contiguous():
        raise L.DicowError(f"orc_counts: out must be a contiguous int32 [{n}, 2] tensor on {dev}")
    asg = torch.full((max(len(ut), 1),), -1, dtype=torch.int32, device=dev) if want_assignment else None
    tables = (pt.ctypes.data if n else None, n, ut.ctypes.data if len(ut) else None, st.ctypes.data if len(st) else None)
    with torch.cuda.device(dev):
        ws, nbytes = ops.table_workspace("orc_counts", L.lib().dicow_orc_distance_ws_bytes, *tables, int(bool(want_assignment)), device=dev)
        L.call("dicow_orc_distance", ref_ids.data_ptr(), ref_ids.numel(), hyp_ids.data_ptr(), hyp_ids.numel(), L.ptr(ref_iv), L.ptr(hyp_iv),
               *tables, out.data_ptr(), L.ptr(asg), ws.data_ptr(), nbytes, L.stream())
    n_ref = [int(ut[r[0]:r[0] + r[1], 1].sum()) for r in pt]
    n_hyp = [int(st[r[2]:r[2] + r[3], 1].sum()) for r in pt]
    counts = counts_from(out.cpu(), np.array([(0, a, 0, b) for a, b in zip(n_ref, n_hyp)], np.int64).reshape(-1, 4))
    return (counts, asg.cpu()[:len(ut)]) if want_assignment else counts


def _relabelled(seg, speaker):
    """A copy of the segment with another speaker, in the form it came in."""
    if isinstance(seg, dict):
        return {**seg, "speaker": speaker}
    return (speaker,) + tuple(seg[1:])


def filter_empty_segments(segments) -> list:
    """The segments whose text is not the empty string (wer_utils.py:45-46)."""
    return [seg for seg in segments if _segment(seg)[3] != ""]


def create_dummy_seg_list(session_id=None) -> list:
    """What the reference scores a group without any hypothesis against (general.py:102-104): one segment from 0 s to 0 s of speaker
    ``''`` with no words."""
    return [{"session_id": session_id, "start_time": 0, "end_time": 0, "speaker": "", "words": ""}]


def create_vad_mask(segments, time_step: float = 0.1, total_duration=None) -> np.ndarray:
    """Boolean activity per ``time_step`` (wer_utils.py:95-119): ``int(float(total) / time_step) + 1`` frames, total = the latest end
    unless given; a segment sets frames ``int(float(start) / time_step)`` up to but not including ``int(float(end) / time_step)``."""
    segs = [_segment(seg) for seg in segments]
    if total_duration is None:
        total_duration = max(end for _, _, end, _ in segs)
    mask = np.zeros(int(float(total_duration) / time_step) + 1, dtype=bool)
    for _, start, end, _ in segs:
        mask[int(float(start) / time_step):int(float(end) / time_step)] = 1
    return mask


def find_group_splits(vad, group_duration=30, time_step: float = 0.1) -> list:
    """The silent frames at which a session is cut (wer_utils.py:122-131): walking the inactive frames in order, the first one at or
    behind ``group_duration / time_step`` frames after the previous cut (or the start)."""
    splits = []
    group_shift = group_duration / time_step
    next_offset = group_shift
    for i in np.argwhere(~np.asarray(vad, dtype=bool)).squeeze(axis=-1):
        if i >= next_offset:
            splits.append(int(i))
            next_offset = i + group_shift
    return splits


def map_utterance_to_split(utterance_start_time, splits) -> int:
    """The group of an utterance (wer_utils.py:134-138): the first split its start time lies strictly before, else ``len(splits)``."""
    for i, split in enumerate(splits):
        if utterance_start_time < split:
            return i
    return len(splits)


def merge_streams(segments) -> list:
    """Hypothesis speakers that never talk at the same time become one stream (wer_utils.py:63-92): per speaker, in order of first
    appearance, a VAD mask at 10 ms; the first pair (a, b), a before b in the double loop over that order, whose masks share no frame is
    merged into a (b's segments relabelled, masks or-ed), and again until no pair is left.  Returns relabelled copies of the segments,
    sorted by start time."""
    groups = {}
    for seg in segments:
        groups.setdefault(_segment(seg)[0], []).append(seg)
    masks = {spk: create_vad_mask(segs, time_step=0.01) for spk, segs in groups.items()}
    longest = max((len(m) for m in masks.values()), default=0)
    masks = {spk: np.pad(m, (0, longest - len(m))) for spk, m in masks.items()}

    def first_pair():
        for a in groups:
            for b in groups:
                if a != b and not (masks[a] & masks[b]).any():
                    return a, b
        return None

    while True:
        pair = first_pair()
        if pair is None:
            break
        a, b = pair
        groups[a] = groups[a] + [_relabelled(seg, a) for seg in groups[b]]
        masks[a] = masks[a] | masks[b]
        del groups[b], masks[b]
    return sorted((seg for segs in groups.values() for seg in segs), key=lambda seg: _segment(seg)[1])


def _orc_score(groups, timed: bool, collar: float, device) -> dict:
    """groups: [(reference segments, hypothesis segments)], one ``dicow_orc_distance`` problem each, all in one call."""
    vocab = Vocabulary()
    ref_flat, hyp_flat, riv, hiv, utt_rows, stream_rows, problems, labels = [], [], [], [], [], [], [], []
    for ref, hyp in groups:
        problems.append([len(utt_rows), 0, len(stream_rows), 0])
        for _, start, end, text in sorted((_segment(seg) for seg in ref), key=lambda x: x[1]):
            w = text.split()
            utt_rows.append((len(ref_flat), len(w)))
            ref_flat += vocab.ids(w)
            riv += pseudo_word_intervals(start, end, w, False, 0.0)
        by = _streams(hyp, True, collar if timed else 0.0)
        for spk in by:
            stream_rows.append((len(hyp_flat), len(by[spk][0])))
            hyp_flat += vocab.ids(by[spk][0])
            hiv += by[spk][1]
        labels.append(list(by))
        problems[-1][1], problems[-1][3] = len(utt_rows) - problems[-1][0], len(stream_rows) - problems[-1][2]
    timed = timed and bool(ref_flat) and bool(hyp_flat)                     # without words on both sides no two words can be compared
    rf = torch.tensor(ref_flat, dtype=torch.int32).to(device)
    hf = torch.tensor(hyp_flat, dtype=torch.int32).to(device)
    ri = torch.tensor(riv, dtype=torch.int32).reshape(-1, 2).to(device) if timed else None
    hi = torch.tensor(hiv, dtype=torch.int32).reshape(-1, 2).to(device) if timed else None
    counts, asg = orc_counts(rf, hf, problems, utt_rows, stream_rows, ri, hi, want_assignment=True)
    tot = counts.sum(0) if len(problems) else torch.zeros(5, dtype=torch.int64)
    length = sum(n for _, n in utt_rows)
    assignment = tuple(labels[g][int(asg[u])] if labels[g] else None for g, p in enumerate(problems) for u in range(p[0], p[0] + p[1]))
    return {"error_rate": int(tot[0]) / length if length else None, "errors": int(tot[0]), "length": length, "insertions": int(tot[4]),
            "deletions": int(tot[3]), "substitutions": int(tot[2]), "assignment": assignment}


def orc_wer(ref_segments, hyp_segments, device="cuda") -> dict:
    """Optimal-reference-combination WER of one session, ungrouped (meeteval's ``orcwer``).  Segments as for ``cp_wer``; those without
    text are dropped.  A reference segment is one utterance, utterances sorted by start time; a hypothesis speaker is one stream as in
    ``cp_wer``; every utterance goes to the stream that makes the total fewest errors.  Returns ``error_rate errors length insertions
    deletions substitutions assignment`` (``assignment``: the hypothesis speaker per utterance in sorted order, None without any)."""
    return _orc_score([(filter_empty_segments(ref_segments), filter_empty_segments(hyp_segments))], False, 0.0, device)


def tcorc_wer(ref_segments, hyp_segments, collar: float = 5.0, device="cuda") -> dict:
    """Time-constrained ORC-WER (meeteval's ``tcorcwer``): as ``orc_wer`` with the word timing and the overlap rule of ``tcp_wer``."""
    return _orc_score([(filter_empty_segments(ref_segments), filter_empty_segments(hyp_segments))], True, collar, device)


def session_tcorc_wer(ref_segments, hyp_segments, collar: float = 5.0, group_duration=5, time_step: float = 0.01, device="cuda") -> dict:
    """The reference's ``calc_session_tcorc_wer`` with the defaults of its call site (wer.py:41-86, 167-168): segments without text are
    dropped; the VAD masks of both sides are or-ed; the session is cut at ``find_group_splits``; a segment belongs to the group of its
    start time; each group's hypothesis -- ``create_dummy_seg_list`` where there is none -- goes through ``merge_streams``; the groups of
    the reference are scored as tcORC-WER problems, all in ONE ``dicow_orc_distance`` call, their counts summed and their assignments
    concatenated in group order.  Hypothesis segments of a group without reference are not scored, as in the reference."""
    ref = filter_empty_segments(ref_segments)
    hyp = filter_empty_segments(hyp_segments)
    if not ref:
        raise ValueError("session_tcorc_wer: no reference segment with text")
    ref_vad = create_vad_mask(ref, time_step=time_step)
    hyp_vad = create_vad_mask(hyp, time_step=time_step) if len(hyp) > 0 else ref_vad
    n = max(len(ref_vad), len(hyp_vad))
    vad = np.pad(ref_vad, (0, n - len(ref_vad))) | np.pad(hyp_vad, (0, n - len(hyp_vad)))
    splits = np.array(find_group_splits(vad, group_duration=group_duration, time_step=time_step)) * time_step

    def grouped(segments):
        out = {}
        for seg in segments:
            out.setdefault(map_utterance_to_split(float(_segment(seg)[1]), splits) if len(splits) > 0 else 0, []).append(seg)
        return out

    ref_groups, hyp_groups = grouped(ref), grouped(hyp)
    return _orc_score([(ref_groups[g], merge_streams(hyp_groups.get(g, create_dummy_seg_list()))) for g in ref_groups], True, collar, device)


def session_orc_wer(ref_segments, hyp_segments, device="cuda") -> dict:
    """The reference's ``calc_session_orc_wer`` (wer.py:100-106): plain ``orc_wer``, no grouping."""
    return orc_wer(ref_segments, hyp_segments, device)


_SESSION_METRICS = ("cp_wer", "tcp_wer", "tcorc_wer", "orc_wer")


def _check_metrics(metrics_list, who):
    for metric in metrics_list:
        if metric not in _SESSION_METRICS:
            raise ValueError(f"{who}: unknown metric {metric!r}, expected some of {_SESSION_METRICS}")


def session_metrics(ref_segments, hyp_segments, metrics_list, collar: float = 5.0, device="cuda") -> dict:
    """One session's row of the reference's score sheet (``calc_wer``, wer.py:157-174) as a dict: for each metric named in
    ``metrics_list`` (``cp_wer tcp_wer tcorc_wer orc_wer``) the keys of its result prefixed ``cp_`` / ``tcp_`` / ``tcorc_`` / ``orc_``,
    with ``<p>_error_rate`` renamed ``<p>_wer``."""
    _check_metrics(metrics_list, "session_metrics")
    out = {}
    for metric, fn in (("cp_wer", lambda: cp_wer(ref_segments, hyp_segments, device)),
                       ("tcp_wer", lambda: tcp_wer(ref_segments, hyp_segments, collar, device)),
                       ("tcorc_wer", lambda: session_tcorc_wer(ref_segments, hyp_segments, collar, 5, 0.01, device)),
                       ("orc_wer", lambda: session_orc_wer(ref_segments, hyp_segments, device))):
        if metric in metrics_list:
            prefix = metric.split("_", maxsplit=1)[0]
            for k, v in fn().items():
                out[f"{prefix}_wer" if k == "error_rate" else f"{prefix}_{k}"] = v
    return out


def aggregate_session_metrics(session_dicts, metrics_list) -> dict:
    """The reference's ``aggregate_wer_metrics`` (wer_utils.py:167-182) over ``session_metrics`` dicts: every numeric column summed; then
    per metric named ``<p>_wer = <p>_errors / <p>_length`` and ``<p>_missed_speaker`` / ``_falarm_speaker`` / ``_scored_speaker``, where
    present, replaced by their means ``<p>_mean_...`` over the sessions."""
    _check_metrics(metrics_list, "aggregate_session_metrics")
    rows = list(session_dicts)
    numeric = [k for k in (rows[0] if rows else {})
               if all(isinstance(r.get(k), (int, float, np.integer, np.floating)) and not isinstance(r.get(k), bool) for r in rows)]
    out = {k: sum(r[k] for r in rows) for k in numeric}
    for metric in metrics_list:
        prefix = metric.split("_", maxsplit=1)[0]
        out[f"{prefix}_wer"] = out[f"{prefix}_errors"] / out[f"{prefix}_length"]
        for k in ("missed_speaker", "falarm_speaker", "scored_speaker"):
            if f"{prefix}_{k}" in out:
                out[f"{prefix}_mean_{k}"] = out.pop(f"{prefix}_{k}") / len(rows)
    return out


# ------------------------------------------------------------------------------------------------ word-level alignments

OPS = ("equal", "substitute", "delete", "insert")     # the bytes of dicow_edit_alignment's ops, by jiwer's chunk names


def _alignment_call(ref_ids, hyp_ids, table, ref_iv, hyp_iv, lanes, along, nbytes):
    """One ``dicow_edit_alignment`` call -> ((errors, hits) int32 [n, 2], ops uint8, spans int64 [n, 2]), all on the CPU."""
    n, dev = table.shape[0], ref_ids.device
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    path = torch.empty((max(int(table[:, 1].sum() + table[:, 3].sum()), 1),), dtype=torch.uint8, device=dev)
    spans = torch.empty((n, 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        # the records of a session run to hundreds of MB: past the size of the persistent scratch they are a tensor of this call
        ws = ops.workspace(nbytes, dev) if nbytes <= (64 << 20) else torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        L.call("dicow_edit_alignment", ref_ids.data_ptr(), ref_ids.numel(), hyp_ids.data_ptr(), hyp_ids.numel(), L.ptr(ref_iv), L.ptr(hyp_iv),
               table.ctypes.data, n, out.data_ptr(), path.data_ptr(), spans.data_ptr(), int(lanes), int(along), ws.data_ptr(), nbytes, L.stream())
    return out.cpu(), path.cpu(), spans.cpu()


def edit_alignments(ref_ids: torch.Tensor, hyp_ids: torch.Tensor, pairs, ref_iv: Optional[torch.Tensor] = None,
                    hyp_iv: Optional[torch.Tensor] = None, lanes: int = 0, along: int = 0):
    """The edit path behind ``edit_counts``, arguments as there: ``dicow_edit_alignment`` over the pairs.  Returns ``(counts, paths)``:
    ``counts`` int64 ``[n, 5]`` on the CPU, equal to ``edit_counts`` of the same call; ``paths`` a list with one uint8 CPU tensor per pair,
    one byte per step in forward order, ``0`` hit, ``1`` substitution, ``2`` deletion, ``3`` insertion (``OPS`` names them).  Among paths of
    the same key the one that, walking back from the end, takes the diagonal where it is open and attains the key, else the deletion, else
    the insertion.  The kernel keeps 2 bits per cell of every table of a call in its workspace: a pair list whose records pass
    ``DICOW_ALIGN_MAX_WS_BYTES`` is split over several calls (the result does not depend on the split); a pair that does not fit alone
    is refused."""
    _check_edit_inputs("edit_alignments", ref_ids, hyp_ids, ref_iv, hyp_iv)
    table = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 4))
    n = table.shape[0]
    if n == 0:
        return counts_from(np.zeros((0, 2), np.int32), table), []
    if lanes == 0 and 0 <= int(table[:, [1, 3]].min()) and int(table[:, [1, 3]].max()) <= L.EDIT_MAX_LEN:
        # the library's choice for the whole list, fixed here so that a split does not change the plan
        lanes = L.EDIT_LANES if int(table[:, [1, 3]].min(axis=1).max()) > L.EDIT_LANES_NARROW * L.EDIT_K else L.EDIT_LANES_NARROW
    size = lambda t: L.lib().dicow_edit_alignment_ws_bytes(t.ctypes.data, len(t), int(lanes), int(along))     # noqa: E731
    cap = L.ALIGN_MAX_WS_BYTES
    whole = size(table)
    if whole < 0 and b"DICOW_ALIGN_MAX_WS_BYTES" not in L.lib().dicow_last_error():
        raise L.DicowError(f"edit_alignments: {L.lib().dicow_last_error().decode()}")
    if 0 <= whole <= cap:
        cuts = [0, n]
    else:                                                                   # every byte of the workspace belongs to one pair: sizes add
        cuts, used = [0], 0
        for k in range(n):
            need = size(table[k:k + 1])
            if need < 0 or need > cap:
                raise L.DicowError(f"edit_alignments: pair {k} ({int(table[k, 1])} x {int(table[k, 3])} words) needs more workspace for its "
                                   f"records than DICOW_ALIGN_MAX_WS_BYTES = {cap} on its own")
            if used + need > cap:
                cuts.append(k)
                used = 0
            used += need
        cuts.append(n)
    eh, paths = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = np.ascontiguousarray(table[lo:hi])
        out, path, spans = _alignment_call(ref_ids, hyp_ids, part, ref_iv, hyp_iv, lanes, along, size(part))
        eh.append(out)
        paths += [path[int(first):int(first + length)] for first, length in spans.tolist()]
    return counts_from(torch.cat(eh), table), paths


def alignment_chunks(path) -> list:
    """The chunks of jiwer's ``process_words(...).alignments`` from one pair's ops: ``(type, ref_start, ref_end, hyp_start, hyp_end)`` with
    ``type`` in ``equal substitute delete insert`` and half-open word ranges; neighbouring steps of one type are one chunk."""
    out, i, j = [], 0, 0
    for op in np.asarray(path, dtype=np.uint8).tolist():
        di, dj = int(op != 3), int(op != 2)
        if out and out[-1][0] == OPS[op]:
            out[-1][2] += di
            out[-1][4] += dj
        else:
            out.append([OPS[op], i, i + di, j, j + dj])
        i, j = i + di, j + dj
    return [tuple(c) for c in out]


def alignment_rows(ref_words, hyp_words, path, ref_iv=None, hyp_iv=None) -> list:
    """One pair's ops against its words: rows ``(op, ref_word, ref_begin_s, ref_end_s, hyp_word, hyp_begin_s, hyp_end_s)``, a missing side
    ``None``; ``ref_iv`` / ``hyp_iv``: the words' (begin, end) ticks, or ``None`` for rows without times."""
    path = np.asarray(path, dtype=np.uint8).tolist()
    if sum(op != 3 for op in path) != len(ref_words) or sum(op != 2 for op in path) != len(hyp_words):
        raise ValueError(f"alignment_rows: the ops do not span {len(ref_words)} reference and {len(hyp_words)} hypothesis words")
    sec = lambda iv, k: (None, None) if iv is None else (iv[k][0] / TICKS_PER_SECOND, iv[k][1] / TICKS_PER_SECOND)     # noqa: E731
    rows, i, j = [], 0, 0
    for op in path:
        r = (ref_words[i],) + sec(ref_iv, i) if op != 3 else (None, None, None)
        h = (hyp_words[j],) + sec(hyp_iv, j) if op != 2 else (None, None, None)
        rows.append((OPS[op],) + r + h)
        i, j = i + (op != 3), j + (op != 2)
    return rows


def word_alignments(refs, hyps, text_norm: Optional[Callable] = None, unit: str = "word", device="cuda"):
    """Lists of strings, one pair per utterance, as for ``word_error_counts`` -> ``(alignments, measures)``: per utterance the chunks of
    jiwer's ``process_words(...).alignments`` (``alignment_chunks``), and jiwer's measures of the batch in that unit
    (``measures_from_counts``), both from the same ``dicow_edit_alignment`` launch."""
    rf, hf, table, _, _ = _utterance_pairs("word_alignments", refs, hyps, text_norm, unit, device)
    counts, paths = edit_alignments(rf, hf, table)
    tot = counts.sum(0)
    return [alignment_chunks(p) for p in paths], measures_from_counts(tot[1], tot[2], tot[3], tot[4])


def format_alignment(ref_words, hyp_words, path) -> str:
    """Three lines of plain text, ``REF:`` / ``HYP:`` / marks (``S`` ``D`` ``I``, blank under a hit), every column as wide as the longer of
    its two words, a missing word shown as ``*``.  The project's own layout, not jiwer's ``visualize_alignment``."""
    ref_line, hyp_line, marks = [], [], []
    for op, r, _, _, h, _, _ in alignment_rows(ref_words, hyp_words, path):
        width = max(len(r or ""), len(h or ""), 1)
        ref_line.append(("*" * width if r is None else r).ljust(width))
        hyp_line.append(("*" * width if h is None else h).ljust(width))
        marks.append({"equal": "", "substitute": "S", "delete": "D", "insert": "I"}[op].ljust(width))
    return "\n".join((head + " ".join(cols)).rstrip() for head, cols in (("REF: ", ref_line), ("HYP: ", hyp_line), ("     ", marks)))


def session_alignment(ref_segments, hyp_segments, timed: bool = True, collar: float = 5.0, device="cuda") -> dict:
    """The data behind the reference's tcp alignment view (``calc_wer(save_visualizations=True)``, src/utils/wer.py:18-27, 154-155).  The
    speaker assignment is ``tcp_wer``'s (``timed``) or ``cp_wer``'s: counts for all R x H pairs, Hungarian on the host; then ONE
    ``edit_alignments`` call over the assigned pairs.  Returns that metric's result plus ``hits``, ``timed``, ``collar`` and ``speakers``:
    per assigned pair ``{"ref_speaker", "hyp_speaker", "rows"}`` with rows ``(op, ref_word, ref_begin_s, ref_end_s, hyp_word, hyp_begin_s,
    hyp_end_s)``, ``op`` in ``equal substitute delete insert``, the missing side ``None``, times from ``pseudo_word_intervals`` (the
    hypothesis word's centre point widened by the collar).  A reference speaker without partner gives all ``delete`` rows and
    ``hyp_speaker`` None; a hypothesis speaker without partner all ``insert`` rows and ``ref_speaker`` None.  The ops sum to the result's
    ``substitutions`` / ``deletions`` / ``insertions``."""
    result, c = _session_score(ref_segments, hyp_segments, timed, collar if timed else 0.0, device)
    R, H = len(c["rk"]), len(c["hk"])
    both = [i for i in range(R) if c["col"][i] < H]
    paths = {}
    if both:
        table = np.array([(c["rs"][i], c["rl"][i], c["hs"][c["col"][i]], c["hl"][c["col"][i]]) for i in both], np.int64)
        paths = dict(zip(both, edit_alignments(c["rf"], c["hf"], table, c["riv"], c["hiv"])[1]))
    speakers, hits = [], 0
    for i, j in enumerate(c["col"]):
        rw, riv = c["ref"][c["rk"][i]] if i < R else ([], [])
        hw, hiv = c["hyp"][c["hk"][j]] if j < H else ([], [])
        path = paths[i] if i in paths else np.full(len(rw) + len(hw), 2 if rw else 3, np.uint8)
        hits += int((np.asarray(path) == 0).sum())
        speakers.append({"ref_speaker": c["rk"][i] if i < R else None, "hyp_speaker": c["hk"][j] if j < H else None,
                         "rows": alignment_rows(rw, hw, path, riv, hiv)})
    return {**result, "hits": hits, "timed": bool(timed), "collar": float(collar) if timed else None, "speakers": speakers}


def error_breakdown(alignments, top: int = 20) -> dict:
    """The most frequent errors of alignment rows: ``{"substitutions": [((ref_word, hyp_word), count)], "deletions": [(word, count)],
    "insertions": [(word, count)]}``, at most ``top`` of each, by falling count, then lexicographically.  ``alignments``: a
    ``session_alignment`` result, or any iterable of rows as ``alignment_rows`` gives them."""
    if isinstance(alignments, dict):
        alignments = (row for spk in alignments["speakers"] for row in spk["rows"])
    tally = {"substitute": {}, "delete": {}, "insert": {}}
    for row in alignments:
        key = {"substitute": (row[1], row[4]), "delete": row[1], "insert": row[4]}.get(row[0])
        if key is not None:
            tally[row[0]][key] = tally[row[0]].get(key, 0) + 1
    ranked = lambda d: sorted(d.items(), key=lambda kv: (-kv[1], kv[0]))[:top]     # noqa: E731
    return {"substitutions": ranked(tally["substitute"]), "deletions": ranked(tally["delete"]), "insertions": ranked(tally["insert"])}


def save_alignment_report(session_alignment: dict, path, top: int = 20) -> dict:
    """One JSON file per session: the ``session_alignment`` result (rows as lists) plus ``breakdown`` (``error_breakdown``; a substituted
    pair as ``[ref_word, hyp_word, count]``, a deleted or inserted word as ``[word, count]``).  Returns what was written."""
    import json
    b = error_breakdown(session_alignment, top)
    report = {**session_alignment, "assignment": [list(p) for p in session_alignment["assignment"]],
              "speakers": [{**spk, "rows": [list(r) for r in spk["rows"]]} for spk in session_alignment["speakers"]],
              "breakdown": {"substitutions": [[r, h, n] for (r, h), n in b["substitutions"]],
                            "deletions": [[w, n] for w, n in b["deletions"]], "insertions": [[w, n] for w, n in b["insertions"]]}}
    with open(path, "w") as f:
        json.dump(report, f, indent=1, ensure_ascii=False)
    return report

"""Cutting hallucinated repeats from hypotheses before they are scored, on the GPU (csrc/ngram_repeats.hip).

The reference does not pass a decoded segment on as it is: ``process_session`` (src/utils/evaluation.py:150-176) sends every segment's text
through ``truncate_at_repeating_ngram`` (src/data/postprocess.py:18-74), which cuts a looping hallucination ("thank you thank you ...",
"a b a b ...") at its first repeat, and drops the segments that end more than ``overflow_margin`` past the cut.  Here the words become
int32 ids on the host -- an exact id per distinct word and a second one for its ``lower()`` -- all segments of a corpus are the problems of
ONE ``dicow_ngram_repeats`` call, and the arithmetic is exact integers:

  * ``repeating_ngram_cuts``          the tensor level: flat id buffers + a host table of segments -> ``(keep, reason)`` on the device
  * ``truncate_repeating_ngrams``     a list of strings -> the list of (possibly cut) strings, one call for all of them
  * ``truncate_at_repeating_ngram``   the reference's signature for one string
  * ``session_hypotheses``            the reference's ``process_session`` on what ``LongFormDecoder.transcribe`` returns for one recording:
    SegLST dicts that ``session_metrics``, ``session_alignment`` and ``words_as_segments``' consumers take as they are

The definition (include/dicow_hip.h) is pinned to the reference's function by golden F26 through a plain-Python oracle.  ``reason`` -- which
rule attained the cut -- and its tie rule (the unigram rule wins, then the smallest n) are the project's own: the reference reports none.
``session_hypotheses`` takes the segments' times from the decoder's segments; the reference re-parses them out of the decoded string with
its timestamp tokens.  That step is not pinned to the reference.  Nothing else in the package calls the clean-up implicitly.
No CPU fallback."""
import logging
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .scoring import Vocabulary

log = logging.getLogger(__name__)


def repeating_ngram_cuts(ids: torch.Tensor, fold_ids: torch.Tensor, table, *, min_n: int = 1, max_n: int = 10, min_word_threshold: int = 30,
                         unigram_min_repeat: int = 10, repeat_threshold: int = 10, plan: Optional[int] = None):
    """One ``dicow_ngram_repeats`` call.  ``ids`` / ``fold_ids``: flat contiguous int32 on the GPU, equal iff the words / their lower-cased
    forms are equal; ``table``: int64 ``[n, 2]`` on the host, rows ``(start, len)``.  Returns ``(keep, reason)`` on the device: int32 ``[n]``,
    the number of leading words of each segment to keep, and int32 ``[n, 3]`` = ``(n, i, count)`` of what attained it (zeros: nothing cut;
    n = 1: the unigram rule with the full run at i).  ``plan``: None / 0 the library's choice, 1 .. 4 fix the rows a workgroup and the words
    a chunk (``_lib.NGRAM_PLAN_TILES``); the result does not depend on it.  Bad input raises ``DicowError``."""
    for t, name in ((ids, "ids"), (fold_ids, "fold_ids")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.DicowError(f"repeating_ngram_cuts: {name} must be on the GPU (no CPU fallback)")
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise L.DicowError(f"repeating_ngram_cuts: {name} must be a flat contiguous int32 tensor")
    if fold_ids.device != ids.device or fold_ids.numel() != ids.numel():
        raise L.DicowError("repeating_ngram_cuts: ids and fold_ids must have one length and lie on one device")
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 2))
    n, plan = table.shape[0], int(plan or 0)
    keep = torch.empty(n, dtype=torch.int32, device=ids.device)
    reason = torch.empty((n, 3), dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):
        ws, nbytes = ops.table_workspace("repeating_ngram_cuts", L.lib().dicow_ngram_repeats_ws_bytes, table.ctypes.data if n else None, n, plan,
                                         device=ids.device)
        L.call("dicow_ngram_repeats", ids.data_ptr(), fold_ids.data_ptr(), ids.numel(), table.ctypes.data if n else None, n, int(min_n), int(max_n),
               int(min_word_threshold), int(unigram_min_repeat), int(repeat_threshold), keep.data_ptr(), reason.data_ptr(), plan, ws.data_ptr(),
               nbytes, L.stream())
    return keep, reason


def word_ids(texts):
    """``text.split()`` of every text -> (words per text, flat exact ids, flat folded ids, the ``(start, len)`` table), all on the host.
    Exact ids are equal iff the words are equal strings (``Vocabulary``); a distinct word's folded id is the id of its ``lower()``."""
    words = [t.split() for t in texts]
    vocab, folded = Vocabulary(), Vocabulary()
    flat = np.asarray(vocab.ids(w for ws in words for w in ws), np.int32)
    fold_of = np.asarray(folded.ids(w.lower() for w in vocab.index), np.int32)       # (a dict keeps the order of first appearance: id order)
    lens = np.asarray([len(ws) for ws in words], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else lens
    return words, flat, (fold_of[flat] if flat.size else flat), np.stack([starts, lens], 1) if len(lens) else np.zeros((0, 2), np.int64)


def truncate_repeating_ngrams(texts, ngram_length: int = 10, min_n: int = 1, max_n: Optional[int] = None, min_word_threshold: int = 30,
                              unigram_min_repeat: int = 10, repeat_threshold: int = 10, return_reasons: bool = False, device="cuda"):
    """The reference's ``truncate_at_repeating_ngram`` on every text, in one launch.  An untouched text comes back as the same string, a cut
    one as ``" ".join(words[:keep])`` of its ``split()``.  ``ngram_length`` is only the default of ``max_n`` (it influences nothing else in
    the reference either).  ``return_reasons=True``: ``(texts, reasons)`` with ``reasons`` a list of ``(n, i, count)`` tuples."""
    texts = list(texts)
    words, flat, fold, table = word_ids(texts)
    dev = torch.device(device)
    keep, reason = repeating_ngram_cuts(torch.from_numpy(flat).to(dev), torch.from_numpy(np.ascontiguousarray(fold)).to(dev), table, min_n=min_n,
                                        max_n=ngram_length if max_n is None else max_n, min_word_threshold=min_word_threshold,
                                        unigram_min_repeat=unigram_min_repeat, repeat_threshold=repeat_threshold)
    keep = keep.cpu().tolist()
    out = [t if k >= len(w) else " ".join(w[:k]) for t, w, k in zip(texts, words, keep)]
    if return_reasons:
        return out, [tuple(r) for r in reason.cpu().tolist()]
    return out


def truncate_at_repeating_ngram(text: str, ngram_length: int = 10, min_n: int = 1, max_n: Optional[int] = None, min_word_threshold: int = 30,
                                unigram_min_repeat: int = 10, repeat_threshold: int = 10, device="cuda") -> str:
    """One string, with the reference's signature.  A launch for one string is no way to clean a corpus: see ``truncate_repeating_ngrams``."""
    return truncate_repeating_ngrams([text], ngram_length, min_n, max_n, min_word_threshold, unigram_min_repeat, repeat_threshold, device=device)[0]


def session_hypotheses(segments, tokenizer, speaker, session_id=None, cut_start: float = 0.0, cut_duration: Optional[float] = None,
                       overflow_margin: float = 5.0, text_map: Optional[Callable[[str], str]] = None, truncate: bool = True, device="cuda") -> list:
    """The reference's ``process_session`` for one recording.  ``segments``: the ``dict(start, end, tokens)`` list that
    ``LongFormDecoder.transcribe`` returns for it.  Every segment is decoded with ``skip_special_tokens=True`` and stripped, empty texts
    are dropped; ``text_map`` (``str -> str``) is the hook for the reference's ``add_space_between_chars``; a segment with
    ``end > cut_duration + overflow_margin`` is dropped with a logged warning (``cut_duration=None``: no such rule); the kept texts are
    truncated in ONE launch (``truncate=False``: passed on as they are, and no GPU is needed).  Returns SegLST dicts ``session_id speaker
    start_time end_time words``, the times shifted by ``cut_start``.  The times are the decoder's own."""
    kept = []
    for seg in segments:
        text = tokenizer.decode(seg["tokens"], skip_special_tokens=True).strip()
        if not text:
            continue
        if text_map is not None:
            text = text_map(text)
        start, end = float(seg["start"]), float(seg["end"])
        if cut_duration is not None and end > cut_duration + overflow_margin:
            log.warning("Detected segment out of bounds of cut: session %s speaker %s [%.2f, %.2f] %r", session_id, speaker, start + cut_start,
                        end + cut_start, text)
            continue
        kept.append((start, end, text))
    texts = [t for _, _, t in kept]
    if truncate and texts:
        texts = truncate_repeating_ngrams(texts, device=device)
    out = []
    for (start, end, _), text in zip(kept, texts):
        out.append({"session_id": session_id, "speaker": speaker, "start_time": start + cut_start, "end_time": end + cut_start, "words": text})
    return out

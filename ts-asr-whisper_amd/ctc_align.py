"""Token and word timestamps from the encoder's CTC head: CTC forced alignment on the GPU (csrc/ctc_align.hip).

The decoder's segments carry a start and an end; below the segment nothing says when a word was spoken.  The CTC head gives a per-frame
distribution over the decoder's own vocabulary plus blank (20 ms frames, 80 ms under ``pre_ctc_sub_sample``), so the best path of a
segment's KNOWN tokens through that trellis -- forced alignment, what ``torchaudio.functional.forced_align`` computes -- places every token
in time.  No attention kernel is involved.

  * ``ctc_forced_align``   all problems of a session in ONE library call: path, spans, token scores, total, feasibility -- on the device;
  * ``token_timestamps``   spans -> seconds (the one host read);
  * ``word_timestamps``    tokens -> words by the project's own grouping rule;
  * ``align_segments``     the hookup for what ``LongFormDecoder.transcribe`` / ``MeetingFrontEnd`` produce;
  * ``words_as_segments``  one SegLST dict per word, so ``tcp_wer`` / ``session_tcorc_wer`` / ``session_alignment`` take measured times.

The tie rule of the path (include/dicow_hip.h) and the word rule are the project's own; neither is pinned to another implementation.
No CPU fallback."""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ctc_decoding import chunked_ctc_logits

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


class CtcAlignment(NamedTuple):
    """path int32 [n, Fmax] (label per frame, blank on blank frames, -1 behind F); spans int32 [n, Lmax, 2] (first frame, one past the last,
    relative to the problem's first frame; -1 behind L); token_score fp32 [n, Lmax] (sum of log-probabilities over the token's own frames);
    score fp32 [n]; ok bool [n] (False: infeasible -- the whole path and all spans are -1, score -inf).  All on the device."""
    path: torch.Tensor
    spans: torch.Tensor
    token_score: torch.Tensor
    score: torch.Tensor
    ok: torch.Tensor


def _host_ints(x, n, name, default):
    if x is None:
        return np.full(n, default, np.int64) if np.isscalar(default) else np.asarray(default, np.int64)
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, np.int64).reshape(-1)
    if x.shape[0] != n:
        raise L.DicowError(f"ctc_forced_align: {name} has {x.shape[0]} entries for {n} problems")
    return x


def _groups(lib, table):
    """Runs of problems whose workspaces fit DICOW_CTC_ALIGN_MAX_WS_BYTES: [(first, last + 1)].  Normally one."""
    n = len(table)
    if lib.dicow_ctc_align_ws_bytes(table.ctypes.data if n else None, n) >= 0:
        return [(0, n)]
    out, first, acc = [], 0, 0
    for k in range(n):
        one = lib.dicow_ctc_align_ws_bytes(table[k:k + 1].ctypes.data, 1)
        if one < 0:
            raise L.DicowError(f"ctc_forced_align: problem {k}: {lib.dicow_last_error().decode()}")
        if acc and acc + one > L.CTC_ALIGN_MAX_WS_BYTES:
            out.append((first, k))
            first, acc = k, 0
        acc += one
    out.append((first, n))
    return out


def ctc_forced_align(logits, targets, target_lengths=None, *, blank, rows=None, frame_start=None, frame_len=None, alias=None, lse=None,
                     normalized=False, plan=0):
    """The best CTC path of every problem's targets through its slice of the logits -> ``CtcAlignment``.

    logits [B, T, V1] fp32 / bf16 on the GPU, read in place when frame-major with dense frames (any row stride >= V1: the 128-padded bf16
    view of ``chunked_ctc_logits`` included); anything else is copied first.  targets: a list of n id lists, or a padded integer tensor
    [n, Lmax] with ``target_lengths`` (the tables the library takes are host memory: a device tensor is read back once).  Problem i aligns
    against frames ``[frame_start[i], frame_start[i] + frame_len[i])`` of logits row ``rows[i]`` (defaults: row i, frame 0, all the frames
    behind frame_start).  alias int [V1]: the column read for a label, as ``CtcPrefixScorer`` takes it.  Log-probabilities are
    ``logit - lse``: ``lse`` fp32 [B, T] is computed with ``dicow_ctc_frame_lse`` when None; ``normalized=True`` says the logits are
    log-probabilities already and nothing is subtracted.  ``plan``: 0 the library's choice, 1 / 2 force the narrow / wide recursion (the
    result does not depend on it).  Up to 511 targets a problem; a session whose tables pass the library's 1 GiB workspace limit is
    split into several calls.  Bad input raises ``DicowError``."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise L.DicowError("ctc_forced_align: logits must be on the GPU (no CPU fallback)")
    if logits.dim() != 3:
        raise L.DicowError(f"ctc_forced_align: expected logits [B, T, V1], got {tuple(logits.shape)}")
    B, T, V1 = logits.shape
    dev = logits.device
    if logits.dtype not in (F32, BF16):
        logits = logits.float()
    if not ((logits.stride(2) == 1 or V1 == 1) and (T <= 1 or logits.stride(1) >= V1) and (B <= 1 or logits.stride(0) == T * logits.stride(1))):
        logits = logits.contiguous()
    ld = logits.stride(1) if T > 1 else (logits.stride(0) if B > 1 and T == 1 else V1)
    if isinstance(targets, torch.Tensor):
        if targets.dim() != 2 or target_lengths is None:
            raise L.DicowError("ctc_forced_align: a target tensor must be [n, Lmax] and come with target_lengths")
        tg = targets.detach().cpu().numpy()
        lens = _host_ints(target_lengths, tg.shape[0], "target_lengths", 0)
        if len(lens) and (lens.min() < 0 or lens.max() > tg.shape[1]):
            raise L.DicowError(f"ctc_forced_align: target_lengths outside [0, {tg.shape[1]}]")
        targets = [tg[i, :lens[i]] for i in range(tg.shape[0])]
    elif target_lengths is not None:
        raise L.DicowError("ctc_forced_align: target_lengths goes with a padded target tensor only")
    n = len(targets)
    lens = np.asarray([len(t) for t in targets], np.int64)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64).reshape(-1) for t in targets]) if n else np.zeros(0, np.int64))
    if flat.size and (flat.min() < -(1 << 31) or flat.max() >= 1 << 31):
        raise L.DicowError("ctc_forced_align: a target id does not fit int32")
    flat = flat.astype(np.int32)
    rows = _host_ints(rows, n, "rows", np.arange(n))
    f0 = _host_ints(frame_start, n, "frame_start", 0)
    F = _host_ints(frame_len, n, "frame_len", T - f0)
    table = np.ascontiguousarray(np.stack([rows, f0, F, np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else lens, lens], 1).astype(np.int64))
    Fmax, Lmax = max(1, int(F.max()) if n else 1), max(1, int(lens.max()) if n else 1)
    out = CtcAlignment(torch.empty(n, Fmax, dtype=I32, device=dev), torch.empty(n, Lmax, 2, dtype=I32, device=dev),
                       torch.empty(n, Lmax, dtype=F32, device=dev), torch.empty(n, dtype=F32, device=dev), None)
    status = torch.empty(n, dtype=I32, device=dev)
    if n == 0:
        return out._replace(ok=status == 0)
    if alias is not None:
        alias = alias.to(device=dev, dtype=I32).contiguous()
        if alias.numel() != V1:
            raise L.DicowError(f"ctc_forced_align: alias has {alias.numel()} entries for V1 = {V1} classes")
    if normalized:
        if lse is not None:
            raise L.DicowError("ctc_forced_align: normalized=True takes no lse")
    elif lse is None:
        if B * T == 0:
            raise L.DicowError("ctc_forced_align: no frames")
        lse = torch.empty(B * T, dtype=F32, device=dev)
        L.call("dicow_ctc_frame_lse", logits.data_ptr(), int(logits.dtype == BF16), B * T, V1, ld, lse.data_ptr(), L.stream())
    else:
        if not lse.is_cuda or lse.numel() != B * T:
            raise L.DicowError(f"ctc_forced_align: lse must hold B * T = {B * T} values on the GPU")
        lse = lse.to(F32).contiguous()
    lib = L.lib()
    for a, b in _groups(lib, table):
        sub = np.ascontiguousarray(table[a:b])
        ws, _ = ops.table_workspace("ctc_forced_align", lib.dicow_ctc_align_ws_bytes, sub.ctypes.data, b - a, device=dev, pooled=False)
        L.call("dicow_ctc_forced_align", logits.data_ptr(), int(logits.dtype == BF16), B, T, V1, ld, L.ptr(lse), L.ptr(alias), int(blank),
               sub.ctypes.data, b - a, flat.ctypes.data if flat.size else None, flat.size, out.path[a:].data_ptr(), Fmax,
               out.spans[a:].data_ptr(), Lmax, out.token_score[a:].data_ptr(), out.score[a:].data_ptr(), status[a:].data_ptr(), int(plan),
               ws.data_ptr(), ws.numel(), L.stream())
    return out._replace(ok=status == 0)


def token_timestamps(alignment, frame_seconds, offsets=None):
    """Per problem ``[(token_id, start_s, end_s, mean_logprob)]``, or None where the problem was infeasible.  A token's time is
    ``offset + frame * frame_seconds`` for its first frame and one past its last; ``offsets`` [n] are the seconds of each problem's first
    frame (default 0); mean_logprob is its token score divided by its number of frames.  The one host read of the alignment."""
    ok = alignment.ok.cpu().tolist()
    spans, path, ts = alignment.spans.cpu().numpy(), alignment.path.cpu().numpy(), alignment.token_score.cpu().numpy()
    out = []
    for i, good in enumerate(ok):
        if not good:
            out.append(None)
            continue
        off = 0.0 if offsets is None else float(offsets[i])
        toks = []
        for j in range(spans.shape[1]):
            s, e = int(spans[i, j, 0]), int(spans[i, j, 1])
            if s < 0:
                break
            toks.append((int(path[i, s]), off + s * frame_seconds, off + e * frame_seconds, float(ts[i, j]) / (e - s)))
        out.append(toks)
    return out


def word_timestamps(tokenizer, tokens):
    """One problem's ``[(token_id, start_s, end_s, mean_logprob)]`` -> ``[(word, start_s, end_s, confidence)]``.

    The grouping rule is the project's own (it is not pinned to HF's ``_split_tokens_on_unicode`` / ``_split_tokens_on_spaces``): a word
    starts at the first token and at every token whose decoded text begins with a space; a token that decodes to an incomplete UTF-8
    sequence (the replacement character) joins the token after it.  A word lasts from its first token's start to its last token's end;
    its confidence is exp of the mean of its tokens' mean log-probabilities.  Words that are nothing but white space are dropped."""
    words, pending = [], []

    def close(piece, group):
        if piece.startswith(" ") or not words:
            words.append([piece, group[0][1], group[-1][2], [t[3] for t in group]])
        else:
            w = words[-1]
            w[0] += piece
            w[2] = group[-1][2]
            w[3] += [t[3] for t in group]

    for k, tok in enumerate(tokens):
        pending.append(tok)
        piece = tokenizer.decode([t[0] for t in pending])
        if "�" in piece and k + 1 < len(tokens):                      # (U+FFFD, the replacement character)
            continue
        close(piece, pending)
        pending = []
    return [(w[0].strip(), w[1], w[2], math.exp(sum(w[3]) / len(w[3]))) for w in words if w[0].strip()]


def _text_ids(tokens, keep_below, drop):
    return [int(t) for t in tokens if 0 <= int(t) < keep_below and int(t) not in drop]


@torch.no_grad()
def align_segments(model, input_features, stno_mask, segments, *, margin_s=0.5, enrollments=None):
    """Word times for decoded segments.  ``segments``: per recording (row of ``input_features``) the list of ``dict(start, end, tokens)``
    that ``LongFormDecoder.transcribe`` returns; ``input_features`` [B, M, frames] is a whole number of encoder windows.

    The CTC logits of the whole recording are taken once (``chunked_ctc_logits``: windows abut, so CTC frame k is time
    ``k * frame_seconds``, frame_seconds = window seconds / CTC frames per window = 0.02 * 1500 / Tn for Whisper's 30 s window).  Every
    segment's tokens lose their timestamp, special and eos / pad ids, upper-cased ids read their lower-cased column
    (``tokenizer.upper_cased_tokens``, as ``CtcRescorer`` ties them), and the rest is aligned against the frames that cover
    ``[start - margin_s, end + margin_s]`` clipped to the recording -- all segments of all rows in ONE ``ctc_forced_align`` call.
    ``margin_s`` = 0.5 is a choice nobody has measured on real audio.

    Returns the segments (copies) with ``words`` = [(word, start_s, end_s, confidence)] and ``aligned`` attached.  A segment whose problem
    is infeasible keeps the even spread over [start, end] that ``scoring.pseudo_word_intervals`` gives (confidence None) and gets
    ``aligned=False``."""
    from .scoring import TICKS_PER_SECOND, pseudo_word_intervals
    cfg, tok = model.config, getattr(model, "tokenizer", None)
    if not getattr(cfg, "ctc_weight", 0.0) > 0.0:
        raise L.DicowError("align_segments: the model has no CTC head (config field ctc_weight must be > 0)")
    if tok is None:
        raise L.DicowError("align_segments needs model.set_tokenizer(): words are decoded with it")
    if enrollments is not None:
        raise L.DicowError("align_segments: enrollments are not supported yet (chunked_ctc_logits runs the encoder without them)")
    encoder = model.get_encoder()
    if len(segments) != input_features.shape[0]:
        raise L.DicowError(f"align_segments: {len(segments)} segment lists for {input_features.shape[0]} recordings")
    logits = chunked_ctc_logits(encoder, input_features, stno_mask)
    B, T, V1 = logits.shape
    Tn, _ = encoder.ctc_logits_layout()
    fs = encoder.get_max_len() * 0.01 / Tn
    vocab = tok.get_vocab()
    ts0 = vocab.get("<|0.00|>", cfg.vocab_size)
    drop = set(getattr(tok, "all_special_ids", ()) or ()) | {cfg.eos_token_id, cfg.pad_token_id}
    alias = torch.arange(V1, dtype=I32)
    for lo, up in getattr(tok, "upper_cased_tokens", {}).items():
        alias[int(up)] = int(lo)
    rows, f0s, Fs, targets, where = [], [], [], [], []
    for b, segs in enumerate(segments):
        for k, seg in enumerate(segs):
            lo = min(max(int(math.floor((float(seg["start"]) - margin_s) / fs)), 0), T)
            hi = min(max(int(math.ceil((float(seg["end"]) + margin_s) / fs)), lo), T)
            rows.append(b)
            f0s.append(lo)
            Fs.append(hi - lo)
            targets.append(_text_ids(seg["tokens"], min(ts0, V1 - 1), drop))
            where.append((b, k))
    al = ctc_forced_align(logits, targets, blank=V1 - 1, rows=rows, frame_start=f0s, frame_len=Fs, alias=alias)
    times = token_timestamps(al, fs, [f * fs for f in f0s])
    out = [[dict(seg) for seg in segs] for segs in segments]
    for i, (b, k) in enumerate(where):
        seg = out[b][k]
        seg["aligned"] = times[i] is not None
        if seg["aligned"]:
            seg["words"] = word_timestamps(tok, times[i])
        else:
            words = tok.decode(targets[i]).split()
            iv = pseudo_word_intervals(float(seg["start"]), float(seg["end"]), words) if words else []
            seg["words"] = [(w, s / TICKS_PER_SECOND, e / TICKS_PER_SECOND, None) for w, (s, e) in zip(words, iv)]
    return out


def words_as_segments(aligned_segments, speaker, session_id=None):
    """One recording's aligned segments -> SegLST dicts with ONE word each (speaker, start_time, end_time, words), in time order as the
    segments stand: ``tcp_wer``, ``session_tcorc_wer`` and ``session_alignment`` then score against the words' own times instead of the
    even spread they give a multi-word segment."""
    out = []
    for seg in aligned_segments:
        for word, start, end, _ in seg["words"]:
            d = {"speaker": speaker, "start_time": float(start), "end_time": float(end), "words": word}
            if session_id is not None:
                d["session_id"] = session_id
            out.append(d)
    return out

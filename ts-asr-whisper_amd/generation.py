"""Decoding side of the path: what the reference's evaluation drives through HF's generate.

  * ``stno_seek_windows``   reference DiCoWGenerationMixin.prepare_kwargs_for_generate (src/models/dicow/generation.py
                            :73-106): the STNO mask of each active sample's current 30 s window, padded as silence;
  * ``timestamp_rules``, ``repetition_rules``   Whisper's timestamp processor and HF's two history processors, one kernel each;
  * ``sequence_bias_rules``  HF's sequence_bias / bad_words_ids (hotwords, banned phrases): one kernel over a device table
                            (``sequence_bias_options``, ``sequence_bias_table``; ``phrase_sequences`` turns phrases into ids);
  * ``sample_tokens``       HF's sampling warpers (temperature, top_k, top_p, min_p), a counter-addressed Philox / Gumbel-max draw, the
                            token's log-probability and the end-of-sequence flags: one kernel behind the chain (``sampling_options``);
  * ``ProcessorChain``      the ONE place that orders a step's processors -- sequence bias, repetition rules, banned phrases,
                            suppress lists, timestamp rules, joint CTC / attention term (ctc_decoding.CtcRescorer) -- for greedy
                            and beam decoding alike;
  * ``GreedyDecoder``       the STNO-conditioned encoder runs ONCE per window, the cross-attention K/V of every decoder layer are
                            projected ONCE, and each new token costs one decoder step (``_step``, replayed from a hipGraph under
                            ``use_graphs``) against a per-layer self-attention KV cache.  ``generate``: greedy search or sampling
                            over one [B, P + max_new_tokens] token history; ``beam_search``: the reference's ``_beam_search`` on
                            beam-indirect caches (``advance_ancestry``); ``generate_with_fallback``: Whisper's temperature
                            ladder (``decode_with_fallback``); ``detect_language``: one decoder position;
  * ``LongFormDecoder``     the seek loop over recordings longer than one window (``retrieve_segment``); its segments go back
                            into window-relative tokens through ``fix_timestamps_from_segmentation``.

Every matrix product, attention and LayerNorm is a C-ABI kernel call (the training step's kernels; single-row queries go
through dicow_attn_fwd with Lq = 1, beam rows through dicow_attn_decode, the <= 16-row products through the weight-streaming
gemm_nt_skinny_kernel); selection, processors and seek loops are host control flow around that step.  No CPU fallback.
"""
from types import SimpleNamespace as NS

import torch

from . import _lib as L
from . import ops
from .engine import heads, linear_fwd, lora_fwd

F32, BF16 = torch.float32, torch.bfloat16


def stno_seek_windows(stno_mask, seek, max_frames, batch_idx_map, num_frames=1500):
    """stno_mask [B_all, 4, T_total] (any device); seek / max_frames: feature-frame positions per ORIGINAL sample;
    batch_idx_map: original index of each still-active sample.  Returns [len(map), 4, num_frames] on stno_mask's device."""
    out = stno_mask.new_zeros((len(batch_idx_map), stno_mask.shape[1], num_frames))
    out[:, 0, :] = 1.0                                                # padding frames are silence
    for i, prev in enumerate(int(b) for b in batch_idx_map):
        s = int(seek[prev]) // 2
        n = max(0, min(int(max_frames[prev]) // 2 - s, num_frames))
        out[i, :, :n] = stno_mask[prev, :, s:s + n]
    return out


def timestamp_rules(input_ids, scores, begin_index, eos_token_id, no_timestamps_token_id, max_initial_timestamp_index=None,
                    detect_from_logprob=True):
    """WhisperTimeStampLogitsProcessorCustom.__call__ (reference src/models/dicow/utils.py:5-14): scores fp32 [B, V] on the
    GPU are constrained IN PLACE (and returned); input_ids int64 [B, L] = prompt (begin_index tokens) + generated tokens."""
    if not scores.is_cuda or scores.dtype != F32 or scores.stride(1) != 1:
        raise L.DicowError("timestamp_rules: scores must be fp32 rows on the GPU (no CPU fallback)")
    ids = input_ids.to(device=scores.device, dtype=torch.int64).contiguous()
    B, V = scores.shape
    L.call("dicow_whisper_timestamp_rules", scores.data_ptr(), scores.stride(0), B, V, ids.data_ptr(), ids.shape[1], begin_index,
           no_timestamps_token_id + 1, eos_token_id, no_timestamps_token_id,
           -1 if max_initial_timestamp_index is None else max_initial_timestamp_index, int(detect_from_logprob), L.stream())
    return scores


def repetition_options(repetition_penalty=None, no_repeat_ngram_size=None):
    """Validation of transformers' two processors: (penalty, ngram) as the kernel takes them, or None when both are off
    (None, penalty 1.0 and n-gram size 0 mean off, as in HF's _get_logits_processor)."""
    penalty, ngram = 1.0, 0
    if repetition_penalty is not None and repetition_penalty != 1.0:
        if not isinstance(repetition_penalty, float) or not repetition_penalty > 0:
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {repetition_penalty}")
        penalty = repetition_penalty
    if no_repeat_ngram_size is not None and no_repeat_ngram_size != 0:
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, int) or no_repeat_ngram_size <= 0:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {no_repeat_ngram_size}")
        ngram = no_repeat_ngram_size
    return None if (penalty == 1.0 and ngram == 0) else (penalty, ngram)


def repetition_rules(input_ids, scores, repetition_penalty=None, no_repeat_ngram_size=None):
    """transformers' RepetitionPenaltyLogitsProcessor, then NoRepeatNGramLogitsProcessor (what HF's generate builds from
    generation_config.repetition_penalty / .no_repeat_ngram_size and runs in front of Whisper's processors): scores fp32 [B, V]
    on the GPU are changed IN PLACE (and returned); input_ids int64 [B, L] = prompt + generated tokens, rows may be slices of a
    wider buffer.  With both options off nothing is launched."""
    opt = repetition_options(repetition_penalty, no_repeat_ngram_size)
    if not scores.is_cuda or scores.dtype != F32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise L.DicowError("repetition_rules: scores must be fp32 rows on the GPU (no CPU fallback)")
    if opt is None:
        return scores
    ids = input_ids.to(device=scores.device, dtype=torch.int64)
    if ids.dim() != 2 or ids.shape[0] != scores.shape[0]:
        raise L.DicowError("repetition_rules: input_ids must be [rows, L] with one row per row of scores")
    if ids.stride(1) != 1 or ids.stride(0) < ids.shape[1]:
        ids = ids.contiguous()
    B, V = scores.shape
    L.call("dicow_repetition_rules", scores.data_ptr(), scores.stride(0), B, V, ids.data_ptr(), ids.stride(0), ids.shape[1],
           opt[0], opt[1], L.stream())
    return scores


def _is_token(t):
    import numpy as np
    return isinstance(t, (int, np.integer))


def sequence_bias_options(sequence_bias=None, bad_words_ids=None, eos_token_id=None, vocab_size=None):
    """Validation of transformers' SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor arguments, with their error texts:
    ``sequence_bias`` a dict {tuple of ids: float} or a list of [[ids], float]; ``bad_words_ids`` a list of lists of ids, of which
    single-token entries equal to an eos id are dropped; a token >= vocab_size (when given) raises transformers' vocabulary error.
    The project's own rule on top: a bias must be finite or -inf (+inf and NaN raise; transformers would compute NaN scores from
    -inf + inf).  Returns None when both are off (None), else a pair (bias, banned), each None or (sequences, biases): tuples of ids
    in the caller's order and one float per tuple (-inf for every banned sequence)."""
    import math
    bias = banned = None
    if sequence_bias is not None:
        sb = sequence_bias
        if not isinstance(sb, dict) and not isinstance(sb, list) or len(sb) == 0:
            raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
        if isinstance(sb, dict):
            if any(not isinstance(seq, tuple) for seq in sb):
                raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
            if any(any(not _is_token(t) or t < 0 for t in seq) or len(seq) == 0 for seq in sb):
                raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
            if any(not isinstance(b, float) for b in sb.values()):
                raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
        else:
            def pair_ok(e):
                return (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], list) and len(e[0]) > 0
                        and all(_is_token(t) and t > 0 for t in e[0]) and isinstance(e[1], float))
            if any(not pair_ok(e) for e in sb):
                raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, "
                                 f"but is {sb}.")
            sb = {tuple(e[0]): e[1] for e in sb}                  # (transformers' own conversion: a repeated sequence keeps its first place)
        for seq, b in sb.items():
            if math.isnan(b) or b == float("inf"):
                raise ValueError(f"`sequence_bias` values have to be finite or -inf, but {seq} has {b}")
        bias = ([tuple(int(t) for t in seq) for seq in sb], [float(b) for b in sb.values()])
    if bad_words_ids is not None:
        bw = bad_words_ids
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
        if any(not isinstance(w, list) for w in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
        if any(any(not _is_token(t) or t < 0 for t in w) for w in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
        if eos_token_id is not None:
            eos = torch.as_tensor(eos_token_id).reshape(-1).tolist()
            bw = [w for w in bw if all(w != [e] for e in eos)]
        sb = {tuple(int(t) for t in w): float("-inf") for w in bw}
        if any(len(seq) == 0 for seq in sb):                      # (transformers lets an empty list through; it can complete nothing)
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {bad_words_ids}.")
        banned = (list(sb), list(sb.values())) if sb else None    # (every entry was an eos: nothing is banned, as in transformers)
    for part in (bias, banned):
        if part is None:
            continue
        if vocab_size is not None:
            invalid = [t for seq in part[0] for t in seq if t >= vocab_size]
            if invalid:
                raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {invalid}")
        if len(part[0]) > L.SEQ_BIAS_MAX_SEQ or max(len(seq) for seq in part[0]) > L.SEQ_BIAS_MAX_LEN:
            raise ValueError(f"sequence bias tables hold at most {L.SEQ_BIAS_MAX_SEQ} sequences of at most {L.SEQ_BIAS_MAX_LEN} tokens")
    return None if bias is None and banned is None else (bias, banned)


def sequence_bias_table(sequences, biases, device):
    """The device table of dicow_sequence_bias (include/dicow_hip.h) for ``sequences`` (tuples of ids, distinct) and one bias each:
    a stable sort by last token, a group's single-token sequence first, then ONE int32 buffer
        seq_off [n + 1] | grp_off [groups + 1] | bias [n] (fp32 bits) | tok [tokens]
    uploaded once.  Returns a namespace: buf, n_seq, n_groups, n_tokens, max_len, max_group, max_token."""
    import numpy as np
    seqs = [tuple(int(t) for t in s) for s in sequences]
    if len(seqs) != len(biases) or len(set(seqs)) != len(seqs):
        raise ValueError("sequence_bias_table: one bias per sequence, every sequence once")
    if any(len(s) == 0 or len(s) > L.SEQ_BIAS_MAX_LEN or min(s) < 0 or max(s) >= 2 ** 31 for s in seqs) or len(seqs) > L.SEQ_BIAS_MAX_SEQ:
        raise ValueError(f"sequence_bias_table: at most {L.SEQ_BIAS_MAX_SEQ} sequences of 1 .. {L.SEQ_BIAS_MAX_LEN} ids >= 0")
    with np.errstate(over="ignore"):
        b32 = np.asarray(biases, dtype=np.float32).reshape(len(seqs))
    if not np.all(np.isfinite(b32) | np.isneginf(b32)):
        raise ValueError("sequence_bias_table: a bias has to be finite or -inf (in fp32)")
    order = sorted(range(len(seqs)), key=lambda i: (seqs[i][-1], len(seqs[i]) != 1))     # (stable: the caller's order within a group)
    seq_off, grp_off, tok = [0], [], []
    for k, i in enumerate(order):
        if k == 0 or seqs[i][-1] != seqs[order[k - 1]][-1]:
            grp_off.append(k)
        tok.extend(seqs[i])
        seq_off.append(len(tok))
    grp_off.append(len(order))
    n, ng = len(seqs), len(grp_off) - 1
    flat = np.concatenate([np.asarray(seq_off, np.int32), np.asarray(grp_off, np.int32), b32[order].view(np.int32) if n else
                           np.zeros(0, np.int32), np.asarray(tok, np.int32)])
    return NS(buf=torch.from_numpy(flat).to(device), n_seq=n, n_groups=ng if n else 0, n_tokens=len(tok), max_len=max(map(len, seqs), default=0),
              max_group=max((grp_off[g + 1] - grp_off[g] for g in range(ng)), default=0), max_token=max(tok, default=-1))


def sequence_bias_rules(input_ids, scores, table, plan=0):
    """transformers' SequenceBiasLogitsProcessor (NoBadWordsLogitsProcessor: biases of -inf) for the sequences of ``table``
    (``sequence_bias_table``): scores fp32 [B, V] on the GPU are changed IN PLACE (and returned); input_ids int64 [B, L] = prompt +
    generated tokens, rows may be slices of a wider buffer.  plan: 0 = the library's choice, _lib.SEQ_BIAS_LANE / _WAVE.  With an empty
    table nothing is launched.  No CPU fallback."""
    if not scores.is_cuda or scores.dtype != F32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise L.DicowError("sequence_bias_rules: scores must be fp32 rows on the GPU (no CPU fallback)")
    if table is None or table.n_seq == 0:
        return scores
    B, V = scores.shape
    if table.max_token >= V:
        raise ValueError(f"The model vocabulary size is {V}, but the following tokens were being biased: [{table.max_token}]")
    if table.buf.device != scores.device:
        raise L.DicowError("sequence_bias_rules: the table is not on the scores' device")
    ids = input_ids.to(device=scores.device, dtype=torch.int64)
    if ids.dim() != 2 or ids.shape[0] != B:
        raise L.DicowError("sequence_bias_rules: input_ids must be [rows, L] with one row per row of scores")
    if ids.stride(1) != 1 or ids.stride(0) < ids.shape[1]:
        ids = ids.contiguous()
    L.call("dicow_sequence_bias", scores.data_ptr(), scores.stride(0), B, V, ids.data_ptr(), ids.stride(0), ids.shape[1],
           table.buf.data_ptr(), table.n_seq, table.n_groups, table.n_tokens, table.max_len, table.max_group, plan, L.stream())
    return scores


MAX_LADDER_RUNGS = 16                 # the sampler's stream word is seek-loop iteration * 16 + rung


def sampling_options(top_k=None, top_p=None, min_p=None, seed=None, generator=None):
    """Validation of the sampling arguments, once per call: ``top_k`` an int >= 0 (0: off), ``top_p`` in (0, 1] (1: off), ``min_p`` in
    [0, 1] (0: off), ``seed`` an int in [0, 2^64) -- the key of the sampler's own Philox stream, which replaces ``generator`` (both
    given: ValueError).  Returns None when all four are None (the caller keeps its torch path), else a namespace
    (top_k, top_p, min_p, seed) as ``sample_tokens`` takes them."""
    if top_k is None and top_p is None and min_p is None and seed is None:
        return None
    if seed is not None and generator is not None:
        raise ValueError("`seed` keys the device sampler's own Philox stream; it cannot be combined with `generator`")
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0):
        raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")
    if top_p is not None and (isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 < float(top_p) <= 1.0):
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
    if min_p is not None and (isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= float(min_p) <= 1.0):
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"`seed` has to be an integer in [0, 2^64), but is {seed}")
    return NS(top_k=top_k or 0, top_p=1.0 if top_p is None else float(top_p), min_p=0.0 if min_p is None else float(min_p),
              seed=seed or 0)


def sample_tokens(scores, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, step=0, stream=0, row_ids=None, unfinished=None,
                  eos_token_id=-1, pad_token_id=0, out=None, logprob=None, warped=None, plan=0):
    """dicow_sample_tokens (include/dicow_hip.h): one launch that warps the processed scores fp32 [rows, V] (read only; rows may be
    slices of a wider buffer) with temperature / top_k / top_p / min_p as HF's warpers do, draws every row's token -- the argmax when
    temperature <= 0, else a Gumbel-max draw addressed by (seed, row_ids[r] or r, step, stream) -- and writes it into ``out`` (int64
    [rows], any stride: e.g. a column of the token history; allocated when None), which is returned.
    logprob: fp32 [rows] that receives the token's log-probability over the kept set at temperature 1; warped: fp32 [rows, >= V] rows
    that receive the warped scores (-inf outside the kept set); unfinished: bool / uint8 [rows] flags, updated in place: a finished row
    writes ``pad_token_id``, a row that draws ``eos_token_id`` is cleared.  plan: 0 = the library's choice, _lib.SAMPLE_REG / _STREAM.
    No CPU fallback."""
    if not scores.is_cuda or scores.dtype != F32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise L.DicowError("sample_tokens: scores must be fp32 rows on the GPU (no CPU fallback)")
    rows, V = scores.shape
    dev = scores.device
    if out is None:
        out = torch.empty(rows, dtype=torch.long, device=dev)

    def dev_tensor(t, dtypes, what, shape=(rows,)):
        if t is None:
            return None
        if t.device != dev or t.dtype not in dtypes or tuple(t.shape[:1]) != shape[:1] or t.dim() != len(shape):
            raise L.DicowError(f"sample_tokens: {what} must be a {dtypes[0]} tensor of {len(shape)} dimension(s) over the rows, on the scores' device")
        return t

    dev_tensor(out, (torch.int64,), "out")
    if dev_tensor(logprob, (F32,), "logprob") is not None and rows > 1 and logprob.stride(0) != 1:
        raise L.DicowError("sample_tokens: logprob must be contiguous")
    if dev_tensor(unfinished, (torch.bool, torch.uint8), "unfinished") is not None and rows > 1 and unfinished.stride(0) != 1:
        raise L.DicowError("sample_tokens: unfinished must be contiguous")
    if dev_tensor(warped, (F32,), "warped", (rows, V)) is not None and (warped.shape[1] < V or warped.stride(1) != 1):
        raise L.DicowError("sample_tokens: warped must be fp32 rows of at least V columns")
    if row_ids is not None:
        row_ids = dev_tensor(torch.as_tensor(row_ids, dtype=torch.int64, device=dev).contiguous(), (torch.int64,), "row_ids")
    a = L.SampleArgs(scores=scores.data_ptr(), ld=scores.stride(0) if rows > 1 else max(scores.stride(0), V), rows=rows, V=V,
                     temperature=float(temperature or 0.0), top_k=int(top_k), top_p=float(top_p), min_p=float(min_p),
                     seed=int(seed), step=int(step), stream=int(stream), row_ids=L.ptr(row_ids), unfinished=L.ptr(unfinished),
                     eos=-1 if eos_token_id is None else int(eos_token_id), pad=int(pad_token_id or 0), next=out.data_ptr(),
                     next_stride=out.stride(0) if rows > 1 else 1, logprob=L.ptr(logprob), warped=L.ptr(warped),
                     ld_w=0 if warped is None else (warped.stride(0) if rows > 1 else max(warped.stride(0), V)), plan=int(plan))
    L.call_struct("dicow_sample_tokens", a)
    return out


def phrase_sequences(tokenizer, phrases, variants=("space", "plain")):
    """Token-id tuples of every phrase for ``sequence_bias={seq: bias for seq in ...}`` or ``bad_words_ids=[list(seq) for seq in ...]``:
    per phrase the encoding with a leading space ("space": how a BPE vocabulary spells a word inside a sentence) and as written
    ("plain": at the start of the text), the two forms HF's documentation of the options asks for.  tokenizer: anything with
    ``encode(text, add_special_tokens=False)``.  Distinct tuples in order of first appearance; empty encodings are left out."""
    forms = {"space": lambda p: " " + p, "plain": lambda p: p}
    unknown = [v for v in variants if v not in forms]
    if unknown:
        raise ValueError(f"phrase_sequences: unknown variants {unknown} (known: {sorted(forms)})")
    if isinstance(phrases, str):
        phrases = [phrases]
    out = {}
    for p in phrases:
        for v in variants:
            seq = tuple(int(t) for t in tokenizer.encode(forms[v](p), add_special_tokens=False))
            if seq:
                out.setdefault(seq, None)
    return list(out)


def advance_ancestry(anc, beam_idx, pos):
    """Ancestry table of a beam search whose self-attention caches are never reordered.  anc int32 [rows, Lmax]: anc[r, t] is the
    cache slot that holds key / value t of the hypothesis now living in row r (initially anc[r, :] = r).  After the step that
    wrote position ``pos`` -- every row into its OWN slot -- row r continues the hypothesis of row beam_idx[r] (flat parent rows):
        anc[r, :pos] <- anc[beam_idx[r], :pos]      the parent's history
        anc[r, pos]  <- beam_idx[r]                 the parent wrote ``pos`` into its own slot
    In place on the persistent buffer (the captured decoder step reads it); works on CPU tensors too.  Returns anc."""
    idx = beam_idx.to(device=anc.device, dtype=torch.long)
    if pos > 0:
        anc[:, :pos] = anc[:, :pos].index_select(0, idx)             # (index_select copies before the write)
    anc[:, pos] = idx.to(anc.dtype)
    return anc


def _eos_pad(cfg, eos_token_id=None, pad_token_id=None):
    """(eos, pad): the model config's ids wherever the caller gave none."""
    return (cfg.eos_token_id if eos_token_id is None else eos_token_id, cfg.pad_token_id if pad_token_id is None else pad_token_id)


class ProcessorChain:
    """One window's logits processors, in the order the reference runs them: HF's own history processors in front of
    Whisper's, as transformers' _get_logits_processor orders them (``sequence_bias_rules`` on the sequence_bias table,
    ``repetition_rules`` -- the penalty scales a score the bias has already moved --, ``sequence_bias_rules`` on the bad_words_ids
    table), SuppressTokens / SuppressTokensAtBegin (generation.py:286-306), the timestamp rules
    (return_timestamps=True, generation.py:272-281), then the joint CTC / attention term (generation.py:249-268).
    seqb: ``sequence_bias_options``' result; its two device tables are built here, once per window.
    ``chain(ids, scores)`` processes one step's fp32 scores [rows, V] IN PLACE given the history ids [rows, cur] = prompt
    (P tokens) + the tokens chosen so far, rows = batch x num_beams.  logprobs says what ``scores`` are: True -- already
    log-probabilities (beam search: nothing more is normalised), False -- raw logits (greedy: the log-softmax sits in front of
    the CTC term and runs only when that term is on)."""

    def __init__(self, model, enc_out, prompt, eos, suppress_tokens, begin_suppress_tokens, timestamps, ctc, rep, num_beams, logprobs,
                 seqb=None):
        dev = enc_out.device
        self.P, self.eos, self.timestamps, self.rep, self.logprobs = prompt.shape[1], eos, timestamps, rep, logprobs
        self.bias, self.banned = (None if part is None else sequence_bias_table(*part, dev) for part in (seqb or (None, None)))
        self.sup = None if not suppress_tokens else torch.as_tensor(list(suppress_tokens), device=dev)
        self.bsup = None if not begin_suppress_tokens else torch.as_tensor(list(begin_suppress_tokens), device=dev)
        self.rescorer = None
        if ctc is not None and ctc.get("weight", 0.0) > 0.0:
            from .ctc_decoding import CtcRescorer
            self.rescorer = CtcRescorer(model.get_enc_logits(enc_out), model.config.vocab_size, eos, prompt[0, 0].item(),
                                        ctc["first_timestamp"], ctc.get("upper_cased", ()), ctc.get("prefix_len", self.P), ctc["weight"],
                                        ctc.get("n_score", 500), num_beams=num_beams)
            self.rows = torch.arange(prompt.shape[0] * num_beams, device=dev)

    def __call__(self, ids, scores):
        if self.bias is not None:
            scores = sequence_bias_rules(ids, scores, self.bias)
        if self.rep is not None:
            scores = repetition_rules(ids, scores, *self.rep)
        if self.banned is not None:
            scores = sequence_bias_rules(ids, scores, self.banned)
        if self.sup is not None:
            scores[:, self.sup] = -float("inf")
        if self.bsup is not None and ids.shape[1] == self.P:          # the first generated position
            scores[:, self.bsup] = -float("inf")
        if self.timestamps is not None:
            scores = timestamp_rules(ids, scores, self.P, self.eos, self.timestamps["no_timestamps_token_id"],
                                     self.timestamps.get("max_initial_timestamp_index"))
        if self.rescorer is not None:
            scores = self.rescorer(ids, scores if self.logprobs else torch.log_softmax(scores, dim=-1))
        return scores

    def advance(self, tokens, beam_idx=None):
        """tokens [rows]: what each row continues with; beam_idx [rows]: the row it continues (None: itself)."""
        if self.rescorer is not None:
            self.rescorer.update_state(tokens, self.rows if beam_idx is None else beam_idx)


def _rows3(t, B, H):
    """[B, >=H*64] column slice -> [B, H, 64] strided view."""
    return t.as_strided((B, H, 64), (t.stride(0), 64, 1), t.storage_offset())


class GreedyDecoder:
    """``GreedyDecoder(model).generate(...)`` for a ``DiCoWForConditionalGeneration`` on the GPU."""

    def __init__(self, model, use_graphs=False):
        """use_graphs: capture each decoder position's step (~55 launches) into a hipGraph the first time it runs and replay
        it afterwards (the step is launch-bound at B = 16: 0.70 -> 0.30 ms); the KV caches and the token buffer are
        persistent per batch size (beam search: per rows and beams) so that the captured pointers stay valid across windows.  Weights must not be re-allocated
        between calls (evaluation).  Beam search is captured too: its caches are never reordered (see ``beam_search``)."""
        self.model, self.cfg = model, model.config
        self.use_graphs = use_graphs
        self._persist = {}                       # rows (beam states: (rows, beams)) -> decoding state with static buffers and captured graphs

    def _step_graphed(self, ids, t, st):
        st.ids_in.copy_(ids)
        if t not in st.graphs:
            if not st.warm:                      # first-use initialisation inside the kernels' host wrappers happens eagerly
                self._step(st.ids_in, t, st)
                st.warm = True
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=st.pool):
                out = self._step(st.ids_in, t, st)
            st.graphs[t] = (g, out)
        g, out = st.graphs[t]
        g.replay()
        return out

    # ---- one decoder step for position t over the caches
    def _step(self, ids, t, st):
        model, cfg, W = self.model, self.cfg, st.W
        dec = model.model.decoder
        B, D, H = st.B, cfg.d_model, cfg.decoder_attention_heads
        dev = ids.device
        h = torch.empty(B, D, dtype=F32, device=dev)
        ops.embed_fwd(ids.view(B, 1).contiguous(), dec.embed_tokens.weight.detach(), dec.embed_positions.weight.detach()[t:], h)
        x = torch.empty(B, D, dtype=BF16, device=dev)
        o = torch.empty(B, D, dtype=BF16, device=dev)

        def ln(src, mod):
            ops.fddt_ln_fwd(src, B, D, ln_w=mod.weight.detach(), ln_b=mod.bias.detach(), y_bf16=x)
            return x

        for i, lyr in enumerate(dec.layers):
            w, c, la = W.layers[i], st.layers[i], W.layers[i].lora      # (la: the LoRA adapter groups; lora_fwd is a no-op without them)
            qkv = linear_fwd(ln(h, lyr.self_attn_layer_norm), w.sa.qkv, B, flags=L.EPI_SCALE_N, scale=0.125, scale_ncols=D)
            lora_fwd(x, la.sa_qkv, qkv, B, q_scale=0.125)
            c.k[:, t].copy_(qkv[:, D:2 * D])
            c.v[:, t].copy_(qkv[:, 2 * D:])
            ck, cv = c.k[:, :t + 1].view(B, t + 1, H, 64), c.v[:, :t + 1].view(B, t + 1, H, 64)
            if st.group == 1:
                ops.attn_fwd(heads(qkv[:, :D], B, 1, H), ck, cv, heads(o, B, 1, H))
            else:                                # beam rows: position j of row r lives in slot anc[r, j] (this step's own: anc[r, t] = r)
                ops.attn_decode(_rows3(qkv[:, :D], B, H), ck, cv, _rows3(o, B, H), anc=st.anc)
            h = linear_fwd(o, w.sa.o, B, out_dtype=F32, residual=h)
            lora_fwd(o, la.sa_o, h, B)
            q = linear_fwd(ln(h, lyr.encoder_attn_layer_norm), w.ca.q, B, flags=L.EPI_SCALE_N, scale=0.125, scale_ncols=D)
            lora_fwd(x, la.ca_q, q, B, q_scale=0.125)
            if st.group == 1:
                ops.attn_fwd(heads(q, B, 1, H), heads(c.ckv[:, :D], B, st.T, H), heads(c.ckv[:, D:], B, st.T, H), heads(o, B, 1, H))
            else:                                # the beams of a window share its cross-attention K/V
                B0 = B // st.group
                ops.attn_decode(_rows3(q, B, H), heads(c.ckv[:, :D], B0, st.T, H), heads(c.ckv[:, D:], B0, st.T, H), _rows3(o, B, H),
                                group=st.group)
            h = linear_fwd(o, w.ca.o, B, out_dtype=F32, residual=h)
            lora_fwd(o, la.ca_o, h, B)
            a = linear_fwd(ln(h, lyr.final_layer_norm), w.fc1, B, flags=0 if la.fc1 is not None else L.EPI_GELU)
            lora_fwd(x, la.fc1, a, B, gelu=True)
            h = linear_fwd(a, w.fc2, B, out_dtype=F32, residual=h)
            lora_fwd(a, la.fc2, h, B)
        logits = torch.empty(B, W.vpad, dtype=F32, device=dev)
        ops.gemm_nt(ln(h, dec.layer_norm), W.head.w, logits, B, W.vpad, D)
        return logits[:, :cfg.vocab_size]

    @torch.no_grad()
    def encode(self, input_features, stno_mask, enrollments=None, num_beams=1, reorder_caches=False):
        """Encoder once + the cross-attention K/V of every decoder layer once.  Returns the decoding state.
        num_beams > 1: the decoding state has batch x num_beams rows.  The cross-attention K/V stay [batch * T, 2D] -- one copy
        per window, read by its beams through ops.attn_decode(group=num_beams) -- and the self-attention caches are addressed
        through the ancestry table ``st.anc`` (``st.group = num_beams``).  reorder_caches=True: the layout of a greedy state
        with batch x num_beams rows instead (``st.group = 1``): the K/V repeated per beam, caches reordered by the caller."""
        model, cfg = self.model, self.cfg
        if not input_features.is_cuda:
            raise L.DicowError("GreedyDecoder: tensors must be on the GPU (no CPU fallback)")
        enc_out = model.model.encoder(input_features, stno_mask=stno_mask, enrollments=enrollments).last_hidden_state
        B0, T, D = enc_out.shape
        B = B0 * num_beams
        W = model._engine().W
        enc_bf = ops.cast_bf16(enc_out.contiguous().to(F32)).view(B0 * T, D)
        Lmax = cfg.max_target_positions
        dev = enc_out.device
        group = 1 if reorder_caches else num_beams
        Bc = B0 if group > 1 else B                                  # rows of cross-attention K/V
        key = B if group == 1 else (B, group)                        # a beam state never collides with a greedy state of as many rows
        st = self._persist.get(key) if self.use_graphs else None
        if st is None or st.W is not W or st.T != T:
            st = NS(B=B, T=T, W=W, group=group, anc=None, layers=[], graphs={}, warm=False, pool=None,
                    ids_in=torch.zeros(B, dtype=torch.long, device=dev))
            if group > 1:
                st.anc = torch.arange(B, dtype=torch.int32, device=dev)[:, None].repeat(1, Lmax)
            for w in W.layers:
                st.layers.append(NS(ckv=torch.empty(Bc * T, w.ca.kv.N, dtype=BF16, device=dev),
                                    k=torch.empty(B, Lmax, D, dtype=BF16, device=dev),
                                    v=torch.empty(B, Lmax, D, dtype=BF16, device=dev)))
            if self.use_graphs:
                st.pool = torch.cuda.graph_pool_handle()
                self._persist[key] = st
        st.enc_out = enc_out
        for w, c in zip(W.layers, st.layers):
            if Bc == B0:
                linear_fwd(enc_bf, w.ca.kv, B0 * T, out=c.ckv)
                lora_fwd(enc_bf, w.lora.ca_kv, c.ckv, B0 * T)
            else:
                kv = linear_fwd(enc_bf, w.ca.kv, B0 * T)
                lora_fwd(enc_bf, w.lora.ca_kv, kv, B0 * T)
                c.ckv.view(B0, num_beams, T, -1).copy_(kv.view(B0, 1, T, -1).expand(B0, num_beams, T, kv.shape[1]))
        return st

    @torch.no_grad()
    def detect_language(self, input_features, stno_mask, lang_token_ids, decoder_start_token_id=None, enrollments=None,
                        return_logits=False):
        """DiCoWGenerationMixin.detect_language (reference src/models/dicow/generation.py:151-221): the encoder runs on the
        first window with its STNO mask (and enrollments), the decoder runs position 0 on the start token, every logit that is
        not a language token (``generation_config.lang_to_id.values()``) is masked and the argmax is returned ([B] int64)."""
        cfg = self.cfg
        n = 2 * cfg.max_source_positions
        st = self.encode(input_features[:, :, :n].contiguous(), stno_mask[:, :, :n // 2].contiguous(), enrollments)
        start = cfg.decoder_start_token_id if decoder_start_token_id is None else decoder_start_token_id
        ids = torch.full((st.B,), start, dtype=torch.long, device=input_features.device)
        logits = self._step(ids, 0, st).float()
        lang = torch.as_tensor(list(lang_token_ids), dtype=torch.long, device=logits.device)
        masked = torch.full_like(logits, float("-inf"))
        masked[:, lang] = logits[:, lang]
        best = masked.argmax(-1)
        return (best, logits) if return_logits else best

    @torch.no_grad()
    def beam_search(self, input_features, stno_mask, decoder_input_ids, max_length, num_beams, eos_token_id=None, pad_token_id=None,
                    length_penalty=1.0, early_stopping=False, suppress_tokens=None, begin_suppress_tokens=None, enrollments=None,
                    timestamps=None, ctc=None, reorder_caches=False, repetition_penalty=None, no_repeat_ngram_size=None,
                    sequence_bias=None, bad_words_ids=None):
        """Beam search as the reference runs it (DiCoWGenerationMixin._beam_search, generation.py:815-1153, on transformers'
        vectorised beam helpers): per step the top 2K continuations over beams x vocabulary, the K best unfinished keep running,
        finished ones compete for the K result slots with length-penalised scores; the ``ProcessorChain`` acts on
        log-probabilities (where HF's beam search applies its processors); KV caches and the CTC states follow ``beam_idx``.
        Returns (sequences [B, <= max_length], scores [B]) of the best hypothesis.

        The caches follow their beams WITHOUT being copied: a window's cross-attention K/V exist once and are read by its K
        rows (ops.attn_decode, group=K); every row writes its self-attention key / value into its own slot and reads position j
        from slot ``st.anc[r, j]``, which ``advance_ancestry`` updates per token (one [B K, Lmax] int32 gather instead of
        2 x layers cache copies).  The step itself therefore touches fixed buffers only and is captured / replayed like the
        greedy one under ``use_graphs``; the top-2K selection, the processors and the ancestry update stay outside the graph.
        reorder_caches=True: the former path (K/V repeated per beam, index_select copies of every cache per token, attn_fwd) --
        the A/B partner of the tests and tools/bench_decode.py, and what K > ops' MAX_GROUP falls back to; it cannot be graphed."""
        cfg, K = self.cfg, int(num_beams)
        eos, pad = _eos_pad(cfg, eos_token_id, pad_token_id)
        reorder_caches = bool(reorder_caches) or K > L.ATTN_DECODE_MAX_GROUP
        rep = repetition_options(repetition_penalty, no_repeat_ngram_size)
        seqb = sequence_bias_options(sequence_bias, bad_words_ids, eos, cfg.vocab_size)
        if self.use_graphs and (reorder_caches or K == 1):           # (one beam: no indirect state; refused under graphs as before)
            raise L.DicowError("beam_search(reorder_caches=True) (also: more than %d beams) copies the KV caches every step: use a "
                               "decoder without graph capture" % L.ATTN_DECODE_MAX_GROUP)
        st = self.encode(input_features, stno_mask, enrollments, num_beams=K, reorder_caches=reorder_caches)
        if st.anc is not None:
            st.anc.copy_(torch.arange(st.B, dtype=torch.int32, device=st.anc.device)[:, None].expand_as(st.anc))
        step = self._step_graphed if self.use_graphs else self._step
        dev = st.enc_out.device
        prompt = decoder_input_ids.to(dev)
        B, P = prompt.shape
        V = cfg.vocab_size
        max_length = min(int(max_length), cfg.max_target_positions)
        if P < 1 or P >= max_length:
            raise ValueError(f"prompt length {P} leaves no room below max_length {max_length}")
        chain = ProcessorChain(self.model, st.enc_out, prompt, eos, suppress_tokens, begin_suppress_tokens, timestamps, ctc, rep,
                               num_beams=K, logprobs=True, seqb=seqb)
        fill = pad if pad is not None else eos
        run_seq = torch.full((B, K, max_length), fill, dtype=torch.long, device=dev)
        run_seq[:, :, :P] = prompt[:, None, :]
        seqs = run_seq.clone()
        run_sc = torch.zeros(B, K, dtype=F32, device=dev)
        run_sc[:, 1:] = -1e9
        fin_sc = torch.full((B, K), -1e9, dtype=F32, device=dev)
        is_fin = torch.zeros(B, K, dtype=torch.bool, device=dev)
        unsat = torch.ones(B, 1, dtype=torch.bool, device=dev)
        run_idx = torch.full((B, K, max_length - P), -1, dtype=torch.int32, device=dev)
        fin_idx = run_idx.clone()
        top_mask = (torch.arange(2 * K, device=dev) < K)[None, :]
        offs = (torch.arange(B, device=dev) * K)[:, None]

        def gather(t, idx):
            while idx.dim() < t.dim():
                idx = idx.unsqueeze(-1)
            return torch.take_along_dim(t, idx, dim=1)

        for t in range(P - 1):                                       # prefill: every beam of a row starts from the same prompt
            step(run_seq[:, :, t].reshape(-1), t, st)
        cur = P
        while True:
            flat = run_seq[:, :, :cur].reshape(B * K, cur)
            logp = chain(flat, torch.log_softmax(step(flat[:, -1].contiguous(), cur - 1, st).float(), dim=-1))
            acc = (logp.view(B, K, V) + run_sc[:, :, None]).reshape(B, K * V)
            tk_lp, tk = torch.topk(acc, k=2 * K)
            src = tk // V
            tk_seq, tk_idx = gather(run_seq, src).clone(), gather(run_idx, src).clone()
            tk_seq[:, :, cur] = tk % V
            tk_idx[:, :, cur - P] = (src + offs).to(torch.int32)
            hits = (tk_seq[:, :, cur] == eos) | (cur + 1 >= max_length)
            run_lp = tk_lp + hits.float() * -1e9
            nxt = torch.topk(run_lp, k=K)[1]
            run_seq, run_sc, run_idx = gather(tk_seq, nxt), gather(run_lp, nxt), gather(tk_idx, nxt)
            just = hits & top_mask
            fin = tk_lp / float((cur + 1 - P) ** length_penalty)
            fin = fin + (is_fin.all(dim=-1, keepdim=True) & (early_stopping is True)).float() * -1e9
            fin = fin + (~unsat).float() * -1e9 + (~just).float() * -1e9
            m_sc = torch.cat((fin_sc, fin), dim=1)
            top = torch.topk(m_sc, k=K)[1]
            seqs, fin_sc = gather(torch.cat((seqs, tk_seq), dim=1), top), gather(m_sc, top)
            fin_idx, is_fin = gather(torch.cat((fin_idx, tk_idx), dim=1), top), gather(torch.cat((is_fin, just), dim=1), top)
            beam_idx = run_idx[..., cur - P].reshape(-1).long()
            if st.anc is not None:                                   # the caches stay put; the table follows the beams
                advance_ancestry(st.anc, beam_idx, cur - 1)
            else:
                for c in st.layers:                                  # the caches follow their beams
                    c.k[:, :cur].copy_(c.k[:, :cur].index_select(0, beam_idx))
                    c.v[:, :cur].copy_(c.v[:, :cur].index_select(0, beam_idx))
            chain.advance(run_seq.reshape(B * K, -1)[:, cur], beam_idx)
            cur += 1
            hyp_len = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur - P)
            best = run_sc[:, :1] / float(hyp_len ** length_penalty)
            worst = torch.where(is_fin, fin_sc.min(dim=1, keepdim=True)[0], torch.full_like(fin_sc, -1e9))
            unsat = unsat & (best > worst).any(dim=-1, keepdim=True)
            go_on = bool(unsat.any()) and not (bool(is_fin.all()) and early_stopping is True) and not bool(hits.all())
            if not go_on:
                break
        gen = int(((fin_idx[:, :1] + 1) != 0).sum(dim=2).max())
        return seqs[:, 0, :P + gen], fin_sc[:, 0]

    @torch.no_grad()
    def generate(self, input_features, stno_mask, decoder_input_ids, max_new_tokens, eos_token_id=None, pad_token_id=None,
                 suppress_tokens=None, begin_suppress_tokens=None, enrollments=None, return_scores=False, ctc=None,
                 timestamps=None, temperature=0.0, generator=None, no_speech_token_id=None, repetition_penalty=None,
                 no_repeat_ngram_size=None, sequence_bias=None, bad_words_ids=None, top_k=None, top_p=None, min_p=None, seed=None,
                 row_ids=None, stream=0, return_logprobs=False):
        """decoder_input_ids int64 [B, P]: the forced prefix (start token, language / task / timestamp tokens).
        The step's raw logits go through the ``ProcessorChain``: sequence_bias, repetition_penalty / no_repeat_ngram_size,
        bad_words_ids (HF's options of those names, see ``sequence_bias_options``), the suppress lists,
        timestamps: dict(no_timestamps_token_id=..., max_initial_timestamp_index=...) for Whisper's timestamp rules, and
        ctc: dict(weight=..., first_timestamp=..., upper_cased=[(lo, up), ...], prefix_len=..., n_score=500) for the joint
        CTC / attention scoring (log-softmax, then ctc_decoding.CtcRescorer on the model's CTC head).
        temperature > 0: multinomial sampling from softmax(processed scores / temperature) (HF's sample mode, what Whisper's
        temperature fallback decodes with; `generator` makes it reproducible); the returned scores are then the temperature-scaled
        ones, as HF's are.  no_speech_token_id: also keep softmax(logits of the position after the start token)[that id] per row
        in ``self.no_speech_prob`` (HF WhisperNoSpeechDetection).
        top_k / top_p / min_p / seed (``sampling_options``), row_ids, return_logprobs: any of them moves the step's tail -- warpers,
        draw, log-probability, end-of-sequence flags -- into ONE ``sample_tokens`` launch that writes the token straight into the
        history.  The draw at history position t of row r is then addressed by (seed, row_ids[r] or r, t, stream), whatever else is in
        the batch; at temperature 0 it is the argmax.  return_logprobs: also return the chosen tokens' log-probabilities [n, B]
        (over the kept set, at temperature 1: what ``sequence_avg_logprob`` recovers from the scores) without keeping any [n, B, V]
        tensor; return_scores then returns the WARPED scores (-inf outside the kept set), as HF does.
        Returns sequences [B, P + n] (and the processed fp32 scores [n, B, V] of the generated positions; and the fp32
        log-probabilities [n, B])."""
        cfg = self.cfg
        eos, pad = _eos_pad(cfg, eos_token_id, pad_token_id)
        seqb = sequence_bias_options(sequence_bias, bad_words_ids, eos, cfg.vocab_size)
        sopt = sampling_options(top_k, top_p, min_p, seed, generator)
        on_device = sopt is not None or row_ids is not None or return_logprobs
        if on_device and generator is not None:
            raise ValueError("`generator` drives torch.multinomial; the device sampler (top_k / top_p / min_p / seed / row_ids / "
                             "return_logprobs) draws from its own Philox stream: pass `seed`")
        st = self.encode(input_features, stno_mask, enrollments)
        dev = st.enc_out.device
        ids = decoder_input_ids.to(dev)
        B, P = ids.shape
        if P < 1 or P + max_new_tokens > cfg.max_target_positions:
            raise ValueError(f"prompt {P} + max_new_tokens {max_new_tokens} exceeds max_target_positions {cfg.max_target_positions}")
        chain = ProcessorChain(self.model, st.enc_out, ids, eos, suppress_tokens, begin_suppress_tokens, timestamps, ctc,
                               repetition_options(repetition_penalty, no_repeat_ngram_size), num_beams=1, logprobs=False, seqb=seqb)
        step = self._step_graphed if self.use_graphs else self._step
        self.no_speech_prob = None
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        hist = torch.empty(B, P + max_new_tokens, dtype=torch.long, device=dev)    # the token history: position t sees hist[:, :t + 1]
        hist[:, :P] = ids
        scores, end, cur = [], P, ids[:, 0]
        if on_device:                                                # the step's tail is one launch (``_generate_on_device``)
            return self._generate_on_device(step, st, chain, hist, P, max_new_tokens, eos, pad, temperature, sopt or sampling_options(seed=0),
                                            row_ids, stream, no_speech_token_id, return_scores, return_logprobs)
        for t in range(P - 1 + max_new_tokens):
            logits = step(cur, t, st)
            if t == 0 and no_speech_token_id is not None:            # the position after the start token, before any processor
                self.no_speech_prob = torch.softmax(logits.float(), dim=-1)[:, no_speech_token_id].clone()
            if t < P - 1:                                            # inside the forced prefix: the step only fills the caches
                cur = ids[:, t + 1]
                continue
            logits = chain(hist[:, :t + 1], logits)
            if temperature and temperature > 0.0:
                logits = logits / temperature
            if return_scores:
                scores.append(logits.clone())
            if temperature and temperature > 0.0:
                nxt = torch.multinomial(torch.softmax(logits.float(), dim=-1), 1, generator=generator)[:, 0]
            else:
                nxt = logits.argmax(-1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            chain.advance(nxt)
            hist[:, t + 1] = cur = nxt
            end = t + 2
            unfinished = unfinished & (nxt != eos)
            if not bool(unfinished.any()):
                break
        out = hist[:, :end].clone()                                  # contiguous, and its own storage
        return (out, torch.stack(scores)) if return_scores else out

    def _generate_on_device(self, step, st, chain, hist, P, max_new_tokens, eos, pad, temperature, sopt, row_ids, stream, no_speech_token_id,
                            return_scores, return_logprobs):
        """generate()'s loop with ``sample_tokens`` as the step's tail: the kernel reads the processed scores, writes the token into
        hist[:, t + 1] and keeps the unfinished flags; the host reads one ``.any()`` of them per step, as the torch loop does."""
        B, V, dev = hist.shape[0], self.cfg.vocab_size, hist.device
        flags = torch.ones(B, dtype=torch.uint8, device=dev)
        lps = torch.zeros(max_new_tokens, B, dtype=F32, device=dev) if return_logprobs else None
        rid = None if row_ids is None else torch.as_tensor(row_ids, dtype=torch.int64, device=dev).contiguous()
        if rid is not None and tuple(rid.shape) != (B,):
            raise ValueError(f"row_ids must hold one id per row ({B}), but has shape {tuple(rid.shape)}")
        scores, end, cur = [], P, hist[:, 0]
        for t in range(P - 1 + max_new_tokens):
            logits = step(cur, t, st)
            if t == 0 and no_speech_token_id is not None:            # the position after the start token, before any processor
                self.no_speech_prob = torch.softmax(logits.float(), dim=-1)[:, no_speech_token_id].clone()
            cur = hist[:, t + 1]
            if t < P - 1:                                            # inside the forced prefix: the step only fills the caches
                continue
            logits = chain(hist[:, :t + 1], logits)
            if logits.dtype != F32 or logits.stride(1) != 1:
                logits = logits.float().contiguous()
            warped = torch.empty(B, V, dtype=F32, device=dev) if return_scores else None
            sample_tokens(logits, temperature, sopt.top_k, sopt.top_p, sopt.min_p, sopt.seed, step=t + 1, stream=stream, row_ids=rid,
                          unfinished=flags, eos_token_id=eos, pad_token_id=pad, out=cur, logprob=None if lps is None else lps[t + 1 - P],
                          warped=warped)
            if return_scores:
                scores.append(warped)
            chain.advance(cur)
            end = t + 2
            if not bool(flags.any()):
                break
        out = hist[:, :end].clone()                                  # contiguous, and its own storage
        return (out,) + ((torch.stack(scores),) if return_scores else ()) + ((lps[:end - P].clone(),) if return_logprobs else ())

    @torch.no_grad()
    def generate_with_fallback(self, input_features, stno_mask, decoder_input_ids, max_new_tokens, temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                               compression_ratio_threshold=1.35, logprob_threshold=-1.0, no_speech_threshold=None,
                               no_speech_token_id=None, generator=None, enrollments=None, skip_by_row=False, top_k=None, top_p=None,
                               min_p=None, seed=None, row_ids=None, stream=0, **gen_kw):
        """Whisper's temperature fallback over one batch of windows (reference generation.py:567-611 -> transformers'
        generate_with_fallback): greedy first; windows whose output is too repetitive (zlib compression ratio) or too unlikely
        (average log-probability) are decoded again -- encoder included, as in HF -- with sampling at the next temperature; a
        window that is unlikely AND looks like silence (no_speech_prob) is skipped instead.  gen_kw: generate()'s processor
        arguments (eos / pad ids, suppress lists, timestamps, ctc, repetition_penalty, no_repeat_ngram_size, sequence_bias,
        bad_words_ids).
        top_k / top_p / min_p / seed (``sampling_options``): the rungs decode through ``sample_tokens`` -- HF's warpers on every rung
        with temperature > 0 -- and the log-probability test reads the kernel's token log-probabilities (no [n, B, V] scores are
        kept).  A window's draws are addressed by its id -- row_ids[window], default its index in this batch -- and by the stream
        word ``stream + rung`` (at most MAX_LADDER_RUNGS rungs), so they do not depend on which other windows fall back with it.
        Returns (token lists of the generated positions without the eos, should_skip flags, temperature index per window)."""
        eos, pad = _eos_pad(self.cfg, gen_kw.get("eos_token_id"), gen_kw.get("pad_token_id"))
        B, P = decoder_input_ids.shape
        sopt = sampling_options(top_k, top_p, min_p, seed, generator)
        if sopt is not None or row_ids is not None:
            if len(temperatures) > MAX_LADDER_RUNGS:
                raise ValueError(f"the device sampler addresses at most {MAX_LADDER_RUNGS} rungs, but the ladder has {len(temperatures)}")
            wid = list(range(B)) if row_ids is None else [int(i) for i in row_ids]
            if len(wid) != B:
                raise ValueError(f"row_ids must hold one id per window ({B}), but has {len(wid)}")
            rung = iter(range(len(temperatures)))
        if no_speech_threshold is not None and no_speech_token_id is None:
            raise ValueError("no_speech_threshold needs no_speech_token_id")

        def decode(rows, temperature):
            idx = torch.as_tensor(rows, device=input_features.device)
            enr = None if enrollments is None else {k: v[idx] for k, v in enrollments.items()}
            if sopt is not None or row_ids is not None:
                seqs, lps = self.generate(input_features[idx], stno_mask[idx], decoder_input_ids[idx.to(decoder_input_ids.device)],
                                          max_new_tokens, enrollments=enr, temperature=temperature, no_speech_token_id=no_speech_token_id,
                                          top_k=top_k, top_p=top_p, min_p=min_p, seed=seed, row_ids=[wid[i] for i in rows],
                                          stream=stream + next(rung), return_logprobs=True, **gen_kw)
                return seqs[:, P:].tolist(), [lps[:, i] for i in range(len(rows))], self.no_speech_prob
            seqs, scores = self.generate(input_features[idx], stno_mask[idx], decoder_input_ids[idx.to(decoder_input_ids.device)],
                                         max_new_tokens, enrollments=enr, return_scores=True, temperature=temperature,
                                         generator=generator, no_speech_token_id=no_speech_token_id, **gen_kw)
            toks = seqs[:, P:].tolist()
            return toks, [scores[:, i] for i in range(len(rows))], self.no_speech_prob

        return decode_with_fallback(decode, B, tuple(temperatures), self.cfg.vocab_size, pad, eos, compression_ratio_threshold,
                                    logprob_threshold, no_speech_threshold, skip_by_row=skip_by_row)


# ------------------------------------------------------------------------------------------------ temperature fallback
# The reference's generate_with_fallback (src/models/dicow/generation.py:567-611) cuts the STNO masks to the active windows and
# hands over to transformers' WhisperGenerationMixin.generate_with_fallback; these are that method's decisions (golden F18 is
# taken from the transformers code itself, driven with scripted decoder outputs).
def token_compression_ratio(tokens, vocab_size):
    """Raw bytes / zlib-compressed bytes of the token ids (HF _retrieve_compression_ratio): repetition detector."""
    import math
    import zlib
    width = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def sequence_avg_logprob(scores, tokens, temperature):
    """Mean log-probability of the generated tokens, eos included (HF _retrieve_avg_logprobs).  scores [n, V]: the processed
    scores of the generated positions as generate(return_scores=True) returns them, i.e. divided by the temperature when
    sampling -- undone here before the fp32 log-softmax."""
    tok = torch.as_tensor(list(tokens), dtype=torch.long, device=scores.device)
    n = min(scores.shape[0], tok.numel())
    sc, tk = scores[:n], (tok if scores.shape[0] > tok.numel() else tok[-n:])[:n]
    if temperature and temperature > 0.0:
        sc = sc * temperature
    lp = torch.log_softmax(sc.float(), dim=-1).to(scores.dtype)
    return float(lp.gather(1, tk[:, None]).sum() / tok.numel())


def sequence_avg_logprob_from_tokens(logprobs, tokens):
    """``sequence_avg_logprob`` from the generated tokens' own log-probabilities: logprobs [n] as generate(return_logprobs=True)
    returns them for one window (taken over the kept set at temperature 1, which is what the log-softmax of the warped scores times
    the temperature gives).  The same alignment rule: with fewer positions than tokens the LAST n tokens are the scored ones."""
    n_tok = len(list(tokens))
    n = min(int(logprobs.shape[0]), n_tok)
    return float(logprobs[:n].float().sum() / n_tok)


def window_needs_fallback(tokens, scores, temperature, vocab_size, compression_ratio_threshold, logprob_threshold,
                          no_speech_threshold=None, no_speech_prob=None):
    """(needs_fallback, should_skip) of one decoded window (HF _need_fallback).  scores: the window's [n, V] processed scores, or the
    1-D vector of its tokens' log-probabilities."""
    needs = compression_ratio_threshold is not None and token_compression_ratio(tokens, vocab_size) > compression_ratio_threshold
    low = False
    if logprob_threshold is not None:
        avg = sequence_avg_logprob_from_tokens(scores, tokens) if scores.dim() == 1 else sequence_avg_logprob(scores, tokens, temperature)
        low = avg < logprob_threshold
        needs = needs or low
    if no_speech_threshold is not None and low and no_speech_prob is not None and no_speech_prob > no_speech_threshold:
        return False, True
    return needs, False


def decode_with_fallback(decode, n_windows, temperatures, vocab_size, pad_token_id, eos_token_id, compression_ratio_threshold=1.35,
                         logprob_threshold=-1.0, no_speech_threshold=None, skip_by_row=False):
    """Temperature ladder over a batch of windows.  decode(rows, temperature) -> (token lists of the generated positions,
    [n, V] score tensors -- or 1-D vectors of the tokens' log-probabilities --, no-speech probabilities or None) for the listed windows.  Every window keeps its latest result;
    those that fail the compression / log-probability test are decoded again at the next temperature.
    Returns (token lists without the eos, should_skip flags, index of the temperature each window ended with).

    skip_by_row=False reproduces transformers' `generate_with_fallback` (which the reference delegates to, generation.py:567-611)
    to the letter, INCLUDING its indexing quirk: `should_skip` is written at the window's position in the CURRENT fallback
    sub-batch, so after the first fallback round a silent window's flag lands on another window of the batch (golden F18 pins
    that behaviour).  skip_by_row=True is the corrected form: the flag is kept per original window and cleared when the
    window is decoded again."""
    final, used, skip = [None] * n_windows, [None] * n_windows, [False] * n_windows
    rows = list(range(n_windows))
    for k, temp in enumerate(temperatures):
        toks, scores, nsp = decode(list(rows), temp)
        again = []
        for i, row in enumerate(rows):
            seq = list(toks[i])
            if seq and seq[-1] == pad_token_id:       # drop the padding tail; with pad == eos one eos stays (it is scored)
                npad = sum(1 for t in seq if t == pad_token_id) - (1 if pad_token_id == eos_token_id else 0)
                if npad:
                    seq = seq[:-npad]
            needs, sk = window_needs_fallback(seq, scores[i], temp, vocab_size, compression_ratio_threshold, logprob_threshold,
                                              no_speech_threshold, None if nsp is None else float(nsp[i]))
            skip[row if skip_by_row else i] = sk      # (transformers indexes this list by the position in the CURRENT batch)
            final[row], used[row] = (seq[:-1] if seq and seq[-1] == eos_token_id else seq), k
            if needs:
                again.append(row)
        rows = again
        if not rows or k == len(temperatures) - 1:
            break
    return final, skip, used


# ------------------------------------------------------------------------------------------------ long-form decoding
def retrieve_segment(seq, time_offset, timestamp_begin, seek_num_frames, time_precision=0.02, input_stride=2):
    """DiCoWGenerationMixin._retrieve_segment (reference src/models/dicow/generation.py:416-534) on a plain list of the tokens
    decoded for one window (prompt removed): consecutive timestamp pairs close segments; a single trailing timestamp means
    "no more speech in this window" (the whole window is consumed), otherwise the seek pointer moves to the last closed
    segment; without any pair the window becomes one segment (or is rolled back when its only timestamp lies beyond 4 s from
    the start).  Returns ([dict(start, end, tokens)], frames to advance); host control flow, pinned by golden F16."""
    is_ts = [t >= timestamp_begin for t in seq]
    single_ending = is_ts[-2:] == [False, True]
    pairs = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    segments = []
    if pairs:
        slices = list(pairs)
        if single_ending:
            slices.append(len(seq))
        else:
            slices[-1] += 1
        last = 0
        for i, cur in enumerate(slices):
            tok = seq[last:cur]
            end_tok = tok[-1 if (i < len(slices) - 1 or single_ending) else -2]
            segments.append({"start": time_offset + (tok[0] - timestamp_begin) * time_precision,
                             "end": time_offset + (end_tok - timestamp_begin) * time_precision, "tokens": tok})
            last = cur
        offset = seek_num_frames if single_ending else (seq[last - 2] - timestamp_begin) * input_stride
    else:
        stamps = [t for t, f in zip(seq, is_ts) if f]
        start_pos, last_pos, skip, offset = 0.0, seek_num_frames // 2, False, seek_num_frames
        if len(stamps) > 1:
            start_pos, last_pos = stamps[-2] - timestamp_begin, stamps[-1] - timestamp_begin
        elif len(stamps) == 1:
            start_pos = stamps[-1] - timestamp_begin
            if start_pos > 200:
                offset, skip = start_pos * input_stride - 100, True
        elif len(seq) <= 1:
            skip = True
        if not skip:
            segments = [{"start": time_offset + start_pos * time_precision, "end": time_offset + last_pos * time_precision,
                         "tokens": list(seq)}]
            offset = seek_num_frames
    if offset <= 0:
        raise ValueError(f"Segment offset: {offset} <= 0. This should not happen!")
    return segments, int(offset)


_UNITS_PER_TICK = 100                  # integer time base of fix_timestamps_from_segmentation: 0.02 s = 100 units
_WINDOW_UNITS = 1500 * _UNITS_PER_TICK   # one 30 s window
_CARRY = -(_UNITS_PER_TICK + 1)         # the reference's Decimal(-0.02): one tick and a hair (4e-19 s) below zero


def _seconds_to_ticks(x):
    """Seconds -> 0.02 s ticks, half-up on the shortest decimal form of the float (what Decimal(str(x)) / ROUND_HALF_UP of
    reference generation.py:314-320 computes), in exact rational arithmetic."""
    from fractions import Fraction
    return int((Fraction(str(float(x))) * 50 + Fraction(1, 2)) // 1)


def fold_segments_to_windows(segments, first_timestamp_token, filler_token):
    """One recording's segments [dict(start, end, tokens)] (recording time, seconds) -> [(start, tokens, end)] with times in
    window-relative 0.02 s ticks (0..1500) or None for a stamp the reference prints as '<|-0.00|>' (not a timestamp token).
    Behaviour of DiCoWGenerationMixin._fix_timestamps_from_segmentation (reference generation.py:322-400) in integer
    arithmetic: a (30, filler, 30) entry is inserted when a 30 s block boundary is crossed, (0, filler, 30) entries bridge
    skipped blocks, a segment that is exactly 30 s long and would wrap is shortened by one tick and that tick is carried into
    the following segments.  The reference's carry is the inexact Decimal(-0.02) (a hair more than one tick); it decides block
    membership of times that land exactly on a boundary, so it is modelled as one extra unit at 100 units per tick.  Pinned by
    golden F17 (247 recordings run through the reference method)."""
    U, W = _UNITS_PER_TICK, _WINDOW_UNITS
    filler = [filler_token]
    out, prev_end, carry = [], None, 0

    def tick(u):
        return None if u < 0 else (u + U // 2) // U

    for seg in segments:
        toks = [int(t) for t in seg["tokens"]]
        if not toks or toks == [first_timestamp_token]:
            continue
        t0, t1 = _seconds_to_ticks(seg["start"]), _seconds_to_ticks(seg["end"])
        a, b = t0 * U + carry, t1 * U + carry
        if a < 0:
            raise ValueError("fold_segments_to_windows: negative segment start")
        if prev_end is None:
            out += [(0, filler, 1500)] * (t0 // 1500)
        else:
            here, before = a // W, max(prev_end - U // 20, 0) // W          # 1 ms below the previous end (generation.py:362)
            if here > before:
                out.append((1500, filler, 1500))
            out += [(0, filler, 1500)] * max(here - before - 1, 0)
        if a // W == b // W:
            out.append((tick(a % W), toks, tick(b % W)))
        elif b % W == 0:
            out.append((tick(a % W), toks, 1500))
            carry = 0
        else:
            lo, hi = a % W, b % W
            if t1 - t0 == 1500:
                if lo == 0 or lo >= W - 2:                                   # float(lo) % 30.0 == 0.0 in the reference
                    hi, carry = W, 0
                else:
                    carry = _CARRY
                    hi += carry
            else:
                carry = 0
            out.append((tick(lo), toks, tick(hi)))
        prev_end = t1 * U + carry
    return out


def fix_timestamps_from_segmentation(segments, first_timestamp_token, filler_token, pad_token_id, prefix_ids=(), suffix_ids=(),
                                     device=None):
    """segments: per recording, the [dict(start, end, tokens)] list LongFormDecoder.transcribe returns.  Returns a padded
    LongTensor [recordings, L] of ``prefix <|start|> text <|end|> ... suffix`` with window-relative timestamp tokens
    (reference generation.py:322-415).  The reference builds the text '<|s|>' + decode(tokens) + '<|e|>' and re-encodes it with the
    tokenizer (which adds its prefix / eos: pass them as prefix_ids / suffix_ids); here the ids are written directly --
    timestamp ids inside ``tokens`` are dropped exactly as Whisper's decode() drops them, text ids are kept as they are."""
    rows = []
    for rec in segments:
        ids = list(prefix_ids)
        for s, toks, e in fold_segments_to_windows(rec, first_timestamp_token, filler_token):
            if s is not None:
                ids.append(first_timestamp_token + s)
            ids += [t for t in toks if t < first_timestamp_token]
            if e is not None:
                ids.append(first_timestamp_token + e)
        rows.append(ids + list(suffix_ids))
    L_ = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), L_), pad_token_id, dtype=torch.long, device=device)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return out


class LongFormDecoder:
    """Sequential long-form decoding of recordings longer than one window, the way the reference drives HF's Whisper
    ``generate`` (temperature 0, no conditioning on previous text -- the reference raises for it, generation.py:545): every
    still-active recording contributes its current 30 s window (features from ``seek``, zero-padded; STNO mask through
    ``stno_seek_windows``), the windows are decoded as one batch (greedy or beam, timestamp rules on), each window's tokens go
    through ``retrieve_segment`` and the recording's seek pointer advances by the returned offset."""

    def __init__(self, model, num_beams=1):
        self.model, self.cfg, self.num_beams = model, model.config, num_beams
        self.decoder = GreedyDecoder(model)

    @torch.no_grad()
    def transcribe(self, input_features, stno_mask, max_frames, decoder_input_ids, no_timestamps_token_id, eos_token_id=None,
                   pad_token_id=None, max_new_tokens=None, enrollments=None, **gen_kw):
        """input_features [B, M, T_total] (T_total a multiple of nothing in particular), stno_mask [B, 4, T_total / 2],
        max_frames [B] valid feature frames per recording, decoder_input_ids [1 or B, P] the forced prompt.
        gen_kw: suppress_tokens, begin_suppress_tokens, max_initial_timestamp_index, ctc, repetition_penalty, no_repeat_ngram_size,
        sequence_bias and bad_words_ids (every window's history starts from that window's prompt, as in HF), the fallback arguments --
        with top_k / top_p / min_p / seed the ladder samples on the device: a draw is addressed by (seed, recording, history position,
        seek-loop iteration * MAX_LADDER_RUNGS + rung), so no two of one call share a Philox counter --, and for
        num_beams > 1 length_penalty, early_stopping and reorder_caches (False: beam_search's default beam-indirect caches; True: its
        former copying path).
        Returns per recording a list of segments dict(start, end, tokens) in seconds / token ids."""
        cfg = self.cfg
        eos, pad = _eos_pad(cfg, eos_token_id, pad_token_id)
        ts0 = no_timestamps_token_id + 1
        W = 2 * cfg.max_source_positions                           # feature frames per window
        B, M, _ = input_features.shape
        max_frames = [int(v) for v in max_frames]
        seek = [0] * B
        out = [[] for _ in range(B)]
        prompt = decoder_input_ids if decoder_input_ids.shape[0] == B else decoder_input_ids.expand(B, -1)
        P = prompt.shape[1]
        n_new = (cfg.max_target_positions - P) if max_new_tokens is None else max_new_tokens
        # the decoder's keywords, the same for every window (only ``enrollments`` is cut to the active rows inside the loop)
        ts = dict(no_timestamps_token_id=no_timestamps_token_id, max_initial_timestamp_index=gen_kw.get("max_initial_timestamp_index", 50))
        kw = dict(eos_token_id=eos, pad_token_id=pad, timestamps=ts,
                  **{k: gen_kw.get(k) for k in ("suppress_tokens", "begin_suppress_tokens", "ctc", "repetition_penalty", "no_repeat_ngram_size",
                                                      "sequence_bias", "bad_words_ids")})
        ladder = gen_kw.get("temperatures") is not None and self.num_beams == 1
        iteration = 0                                              # seek-loop iterations so far: part of the sampler's stream word
        if ladder:
            # temperature fallback (reference generation.py:567-611): per-window ladder, silent windows skipped (skip_by_row=True
            # keeps a silent window's flag with ITS recording; default = transformers' position in the sub-batch, see decode_with_fallback)
            kw.update({k: gen_kw[k] for k in ("temperatures", "compression_ratio_threshold", "logprob_threshold", "no_speech_threshold",
                                              "no_speech_token_id", "generator", "skip_by_row", "top_k", "top_p", "min_p", "seed") if k in gen_kw})
            on_device = sampling_options(*(kw.get(k) for k in ("top_k", "top_p", "min_p", "seed")), kw.get("generator")) is not None
            if on_device and len(kw["temperatures"]) > MAX_LADDER_RUNGS:
                raise ValueError(f"the device sampler addresses at most {MAX_LADDER_RUNGS} rungs, but the ladder has {len(kw['temperatures'])}")
        elif self.num_beams > 1:
            kw.update(length_penalty=gen_kw.get("length_penalty", 1.0), early_stopping=gen_kw.get("early_stopping", False),
                      reorder_caches=gen_kw.get("reorder_caches", False))
        while True:
            active = [b for b in range(B) if seek[b] < max_frames[b]]
            if not active:
                break
            left = [min(max_frames[b] - seek[b], W) for b in active]
            feats = input_features.new_zeros((len(active), M, W))
            for i, b in enumerate(active):
                feats[i, :, :left[i]] = input_features[b, :, seek[b]:seek[b] + left[i]]
            stno = stno_seek_windows(stno_mask, seek, max_frames, active, num_frames=cfg.max_source_positions)
            enr = None if enrollments is None else {k: v[active] for k, v in enrollments.items()}
            skip = [False] * len(active)
            if ladder:
                where = dict(row_ids=active, stream=iteration * MAX_LADDER_RUNGS) if on_device else {}
                tok_lists, skip, _ = self.decoder.generate_with_fallback(feats, stno, prompt[active], n_new, enrollments=enr, **where, **kw)
                iteration += 1
            else:
                if self.num_beams > 1:
                    seqs, _ = self.decoder.beam_search(feats, stno, prompt[active], P + n_new, self.num_beams, enrollments=enr, **kw)
                else:
                    seqs = self.decoder.generate(feats, stno, prompt[active], n_new, enrollments=enr, **kw)
                tok_lists = [seqs[i, P:].tolist() for i in range(len(active))]
            for i, b in enumerate(active):
                if skip[i]:                                          # HF: a skipped (silent) window only moves the seek pointer
                    seek[b] += left[i]
                    continue
                toks = list(tok_lists[i])
                while toks and toks[-1] in (pad, eos):              # HF strips the eos / padding tail before segmenting
                    toks.pop()
                if not toks:
                    seek[b] += left[i]
                    continue
                segs, adv = retrieve_segment(toks, seek[b] * 0.01, ts0, left[i])
                out[b].extend(segs)
                seek[b] += adv
        return out

"""Plain-Python oracle of dicow_sequence_bias' definition (include/dicow_hip.h): explicit fp32 adds through numpy float32 scalars, in
the stated order -- per last token the single-token sequence first, then the multi-token sequences in the caller's order."""
import numpy as np
import torch


def groups_of(sequences):
    """{last token: indices into ``sequences``}, the single-token sequence first, the others in the caller's order."""
    out = {}
    for i, s in enumerate(sequences):
        out.setdefault(int(s[-1]), []).append(i)
    return {v: sorted(idx, key=lambda i: len(sequences[i]) != 1) for v, idx in out.items()}     # (stable)


def matches(seq, hist):
    m = len(seq)
    if m == 1:
        return True
    if m > len(hist):
        return False
    return all(int(a) == int(b) for a, b in zip(seq[:-1], hist[len(hist) - (m - 1):]))


def reference(ids, scores, sequences, biases):
    """ids int64 [rows, L], scores fp32 [rows, V] (CPU tensors), sequences: tuples of ids, biases: floats.  Returns (result, touched):
    the scores after the rule, bit for bit, and the mask of the entries it wrote."""
    with np.errstate(over="ignore", invalid="ignore"):
        out = scores.clone().numpy()
        rows, V = out.shape
        touched = np.zeros((rows, V), dtype=bool)
        b32 = [np.float32(b) for b in biases]
        grp = groups_of(sequences)
        for r in range(rows):
            hist = ids[r].tolist()
            for v, idx in grp.items():
                b, hit = np.float32(0.0), False
                for i in idx:
                    if matches(sequences[i], hist):
                        b = np.float32(b + b32[i])
                        hit = True
                if hit:
                    assert 0 <= v < V
                    out[r, v] = np.float32(out[r, v] + b)
                    touched[r, v] = True
    return torch.from_numpy(out), torch.from_numpy(touched)


def via_transformers(ids, scores, sequence_bias=None, bad_words_ids=None, eos_token_id=None):
    """transformers' two processors on CPU copies (a fresh processor per call: they cache their length-1 bias per vocabulary)."""
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor
    out = scores.clone()
    if sequence_bias is not None:
        out = SequenceBiasLogitsProcessor(sequence_bias=dict(sequence_bias))(ids, out)
    if bad_words_ids is not None:
        out = NoBadWordsLogitsProcessor([list(w) for w in bad_words_ids], eos_token_id=eos_token_id)(ids, out)
    return out


def same_numbers(a, b):
    """Equal as numbers: +0.0 == -0.0, -inf == -inf, no NaN anywhere."""
    return not bool(torch.isnan(a).any() or torch.isnan(b).any()) and bool((a == b).all())


def bits(t):
    return t.contiguous().view(torch.int32)

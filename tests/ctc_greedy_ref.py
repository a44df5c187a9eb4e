"""The restatement of the reference's ctc_greedy_decode (src/utils/decoding.py:6-12) that the GPU tests use as their oracle;
tests/test_host_ctc_greedy.py pins it to golden F22, which the reference's own function produced.  Plain torch on the CPU."""
import torch


def greedy_restatement(logits, blank, pad):
    ids = torch.argmax(logits.detach().float().cpu(), dim=-1)           # (CPU argmax: on equal maxima the lowest index)
    out = torch.full_like(ids, pad)
    for b, row in enumerate(ids):
        kept = torch.unique_consecutive(row)
        kept = kept[kept != blank]
        out[b, :kept.numel()] = kept
    return out


F22_CASES = ("random", "crafted", "inf", "blank50", "pad5")

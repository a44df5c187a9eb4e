"""Plain fp64 references of the two training losses, written from the operations the reference performs (not from the kernels) and
shared by tests/test_host_loss_ref.py (which pins them to torch and to the oracle on the CPU) and tests/test_gpu_losses.py (which
uses them as the oracle of csrc/loss.hip and csrc/ctc.hip).  Inputs are the bf16-rounded logits as fp64, so the only difference from
a kernel is the kernel's arithmetic.  Plain torch on the CPU."""
import itertools

import torch

F64 = torch.float64


def ce_ref(logits, labels, upp_labels, soft, ts):
    """The decoder loss per row: logits fp64 [rows, V], labels / upp_labels int64 [rows] (upp_labels may be None), ts None or
    (sorted timestamp ids int64 [n_ts], weights [n_ts, n_ts]) as oracle.dicow_oracle.build_ts_smoothing returns them.
    Returns a dict: lse [rows], row_loss [rows], choice [rows] (0 = lower set, 1 = upper set), count (rows whose LOWER label is valid)
    and grad = d(sum of row losses) / d logits, all fp64.

    hard (soft=False, reference modeling_dicow.py:310-323): CrossEntropyLoss(ignore_index=-100, reduction="none") of both label sets,
    torch.stack((l1, l2), -1).min(-1) per row.  An ignored set contributes the constant 0, so a row whose upper label alone is
    ignored has loss 0 and gradient 0.
    soft (SoftLabelCreator, modeling_dicow.py:74-144, as oracle.dicow_oracle.soft_loss): target = one_hot(label clamped to >= 0),
    replaced by the dense Gaussian row [n_ts -> V] for a timestamp label; loss = -(target * log_softmax).sum(-1); BOTH losses are
    masked by the lower labels' padding only, so an ignored upper label competes as token 0.
    On an exact tie the lower set wins and takes the gradient: torch's min over the stacked pair returns index 0 on equal values and
    its backward scatters to that index (test_host_loss_ref.py::test_stacked_min_sends_a_tie_to_the_lower_set checks both on the CPU)."""
    z = logits.to(F64).detach().clone().requires_grad_(True)
    rows, V = z.shape
    logp = torch.log_softmax(z, -1)

    def hard(lab):
        return torch.nn.functional.cross_entropy(z, lab, ignore_index=-100, reduction="none")

    def softce(lab):
        target = torch.nn.functional.one_hot(lab.clamp(min=0), V).to(F64)
        if ts is not None:
            ids, w = ts[0].long(), ts[1].to(F64)
            for r in range(rows):
                hit = torch.nonzero(ids == lab[r]).flatten()
                if hit.numel():
                    dense = torch.zeros(V, dtype=F64)
                    dense[ids] = w[int(hit[0])]
                    target[r] = dense
        return -(target * logp).sum(-1)

    if soft:
        mask = (labels != -100).to(F64)
        l1 = softce(labels) * mask
        l2 = softce(upp_labels) * mask if upp_labels is not None else l1
    else:
        l1 = hard(labels)
        l2 = hard(upp_labels) if upp_labels is not None else l1
    both = torch.stack((l1, l2), -1).min(-1)
    both.values.sum().backward()
    return {"lse": torch.logsumexp(z.detach(), -1), "row_loss": both.values.detach(), "choice": both.indices,
            "count": float((labels != -100).sum()), "grad": z.grad, "l1": l1.detach(), "l2": l2.detach()}


def ctc_ref(logits, labels):
    """The CTC auxiliary loss (reference encoder.py:108-135): logits fp64 [B, T, C], labels int64 [B, Lc] with the valid targets
    first and -100 behind them; blank = C - 1, zero_infinity=True, reduction "mean" = mean_b(nll_b / max(tl_b, 1)) with infeasible
    utterances contributing 0.  torch.nn.functional.ctc_loss in fp64 on the CPU.
    Returns a dict: nll [B] (+inf for an infeasible utterance), target_len [B], loss (the mean) and grad = d loss / d logits."""
    z = logits.to(F64).detach().clone().requires_grad_(True)
    B, Tn, C = z.shape
    tl = (labels >= 0).sum(-1)
    lp = torch.log_softmax(z, -1).transpose(0, 1)
    il = torch.full((B,), Tn, dtype=torch.long)
    tgt = labels.clamp(min=0)
    nll = torch.nn.functional.ctc_loss(lp.detach(), tgt, il, tl, blank=C - 1, reduction="none", zero_infinity=False)
    loss = torch.nn.functional.ctc_loss(lp, tgt, il, tl, blank=C - 1, reduction="mean", zero_infinity=True)
    loss.backward()
    return {"nll": nll, "target_len": tl, "loss": loss.detach(), "grad": z.grad}


def ctc_enumerate(logits, labels):
    """The same quantities by brute force: every one of the C^T frame labellings is collapsed (merge repeats, drop blanks) and the
    probabilities of those that spell the target are added up.  For the tiniest case only (C^T paths are held at once)."""
    z = logits.to(F64).detach().clone().requires_grad_(True)
    B, Tn, C = z.shape
    blank = C - 1
    paths = torch.tensor(list(itertools.product(range(C), repeat=Tn)), dtype=torch.long)          # [C^T, T]
    spelled = []
    for p in paths.tolist():
        spelled.append(tuple(c for i, c in enumerate(p) if c != blank and (i == 0 or c != p[i - 1])))
    lp = torch.log_softmax(z, -1)
    tl = (labels >= 0).sum(-1)
    nll, terms = [], []
    for b in range(B):
        want = tuple(int(c) for c in labels[b] if c >= 0)
        hit = torch.tensor([s == want for s in spelled])
        if not bool(hit.any()):
            nll.append(torch.tensor(float("inf"), dtype=F64))
            continue
        plp = lp[b].gather(1, paths[hit].t()).sum(0)                                               # log p of each matching path
        nb = -torch.logsumexp(plp, 0)
        nll.append(nb)
        terms.append(nb / max(int(tl[b]), 1))
    loss = torch.stack(terms).sum() / B if terms else z.sum() * 0.0
    loss.backward()
    return {"nll": torch.stack([n.detach() for n in nll]), "target_len": tl, "loss": loss.detach(), "grad": z.grad}


# The five rows of the tiny CTC case (B = 5, T = 6, C = 5, blank = 4), shared by the host and the GPU test.
TINY_CTC_LABELS = [[0, 0, 1, -100],            # a repeat: needs a blank between the two 0s
                   [2, 2, 2, 2],               # 4 labels + 3 forced blanks = 7 frames > T = 6: infeasible
                   [-100, -100, -100, -100],   # empty target: the loss is -sum_t log p(blank), the gradient is not zero
                   [1, 2, 1, 2],
                   [3, 3, -100, -100]]
TINY_CTC_SHAPE = (5, 6, 5)


def tiny_ctc_inputs():
    """(bf16-rounded logits as fp64 [5, 6, 5], labels int64 [5, 4]) of the tiny case."""
    g = torch.Generator().manual_seed(11)
    z = (torch.randn(*TINY_CTC_SHAPE, generator=g) * 2).bfloat16().double()
    return z, torch.tensor(TINY_CTC_LABELS, dtype=torch.long)

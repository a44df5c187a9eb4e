"""tests/loss_ref.py pinned on the CPU: ce_ref against torch's cross_entropy and the oracle's hard_loss / soft_loss, ctc_ref (torch's
fp64 CTC) against a brute-force enumeration of every path, and the product's CTC label preparation against the oracle's."""
import types

import pytest
import torch

import amd_pkg
from oracle import dicow_oracle as O
from tests.loss_ref import ce_ref, ctc_enumerate, ctc_ref, tiny_ctc_inputs

amd_pkg.load()

F64 = torch.float64


def _ce_inputs(V=37, rows=24, seed=5):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(rows, V, generator=g) * 2).bfloat16().double()
    lab = torch.randint(0, V, (rows,), generator=g)
    upp = torch.randint(0, V, (rows,), generator=g)
    lab[3], upp[3] = -100, -100
    upp[5] = -100                       # lower valid, upper ignored
    lab[7] = -100                       # lower ignored, upper valid
    upp[9] = lab[9]
    return z, lab, upp


def test_stacked_min_sends_a_tie_to_the_lower_set():
    a = torch.tensor([1.5, 2.0, 0.0], dtype=F64, requires_grad=True)
    b = torch.tensor([1.5, 1.0, 0.0], dtype=F64, requires_grad=True)
    m = torch.stack((a, b), -1).min(-1)
    m.values.sum().backward()
    assert m.indices.tolist() == [0, 1, 0]
    assert a.grad.tolist() == [1.0, 0.0, 1.0] and b.grad.tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("with_upper", [True, False])
def test_ce_ref_hard_equals_torch_cross_entropy(with_upper):
    z, lab, upp = _ce_inputs()
    r = ce_ref(z, lab, upp if with_upper else None, False, None)
    zz = z.clone().requires_grad_(True)
    l1 = torch.nn.functional.cross_entropy(zz, lab, ignore_index=-100, reduction="none")
    l2 = torch.nn.functional.cross_entropy(zz, upp, ignore_index=-100, reduction="none") if with_upper else l1
    want = torch.minimum(l1, l2)
    want.sum().backward()
    assert float((r["row_loss"] - want.detach()).abs().max()) < 1e-12
    assert float((r["grad"] - zz.grad).abs().max()) < 1e-12
    assert float((r["lse"] - torch.logsumexp(z, -1)).abs().max()) < 1e-12
    assert r["count"] == float((lab != -100).sum())
    if with_upper:
        assert float(r["row_loss"][5]) == 0.0 and int(r["choice"][5]) == 1 and float(r["grad"][5].abs().max()) == 0.0
        assert float(r["row_loss"][7]) == 0.0 and int(r["choice"][7]) == 0 and float(r["grad"][7].abs().max()) == 0.0
        assert int(r["choice"][9]) == 0 and float(r["grad"][9].abs().max()) > 0.0            # equal labels: an exact tie, lower set
    # the oracle's hard loss (fp32): mean over all rows
    o = O.hard_loss(z.float()[None], lab[None], upp[None] if with_upper else None)
    assert abs(float(o) - float(r["row_loss"].mean())) < 2e-6 * max(1.0, float(o))


def _ts_vocab(V, n_ts):
    vocab = {f"tok{i}": i for i in range(V - n_ts)}
    vocab.update({f"<|{0.02 * j:.2f}|>": V - n_ts + j for j in range(n_ts)})
    return vocab


@pytest.mark.parametrize("with_upper", [True, False])
def test_ce_ref_soft_equals_oracle_soft_loss(with_upper):
    V, n_ts = 60, 20
    z, lab, upp = _ce_inputs(V=V, rows=24, seed=6)
    ts = O.build_ts_smoothing(_ts_vocab(V, n_ts))
    lab[0], upp[0] = V - n_ts, 3                     # lower timestamp (first of the table), upper ordinary
    lab[1], upp[1] = 4, V - 1                        # upper timestamp (last of the table)
    lab[2], upp[2] = V - 5, V - 7                    # both timestamps
    lab[4], upp[4] = V - 3, -100                     # timestamp against the clamped token 0
    r = ce_ref(z, lab, upp if with_upper else None, True, ts)
    zz = z.float().clone().requires_grad_(True)
    o = O.soft_loss(zz[None], lab[None], upp[None] if with_upper else None, ts)
    o.backward()
    o = o.detach()
    cnt = float((lab != -100).sum())
    assert r["count"] == cnt
    assert abs(float(o) - float(r["row_loss"].sum()) / cnt) < 2e-6 * max(1.0, float(o))
    assert float((zz.grad.double() * cnt - r["grad"]).abs().max()) < 1e-5
    if with_upper:
        # upper ignored, lower valid: the upper set competes as token 0 (not as the constant 0)
        assert abs(float(r["l2"][5]) - float(torch.logsumexp(z[5], -1) - z[5, 0])) < 1e-12 and float(r["row_loss"][5]) > 0.0
    assert float(r["row_loss"][3]) == 0.0 and float(r["row_loss"][7]) == 0.0                  # masked by the lower labels only
    assert float(r["grad"][3].abs().max()) == 0.0 and float(r["grad"][7].abs().max()) == 0.0


def test_ce_ref_soft_without_timestamps_is_the_oracle_too():
    z, lab, upp = _ce_inputs(V=11, rows=24, seed=8)
    r = ce_ref(z, lab, upp, True, None)
    o = O.soft_loss(z.float()[None], lab[None], upp[None], None)
    assert abs(float(o) - float(r["row_loss"].sum()) / r["count"]) < 2e-6 * max(1.0, float(o))


def test_ctc_ref_equals_enumeration_on_the_tiny_case():
    z, lab = tiny_ctc_inputs()
    r, e = ctc_ref(z, lab), ctc_enumerate(z, lab)
    assert r["target_len"].tolist() == [3, 4, 0, 4, 2] and e["target_len"].tolist() == [3, 4, 0, 4, 2]
    inf = torch.isinf(e["nll"])
    assert inf.tolist() == [False, True, False, False, False] and torch.isinf(r["nll"]).tolist() == inf.tolist()
    assert float((r["nll"][~inf] - e["nll"][~inf]).abs().max()) < 1e-12
    assert abs(float(r["loss"]) - float(e["loss"])) < 1e-12
    assert float((r["grad"] - e["grad"]).abs().max()) < 1e-12
    # the infeasible row's gradient is exactly zero; the empty row's is not, and its loss is -sum_t log p(blank)
    assert float(r["grad"][1].abs().max()) == 0.0 and float(e["grad"][1].abs().max()) == 0.0
    assert float(r["grad"][2].abs().max()) > 1e-3
    assert abs(float(r["nll"][2]) + float(torch.log_softmax(z[2], -1)[:, 4].sum())) < 1e-12
    # the mean is mean_b(nll_b / max(tl_b, 1)) over the feasible rows
    want = sum(float(r["nll"][b]) / max(int(r["target_len"][b]), 1) for b in (0, 2, 3, 4)) / 5
    assert abs(float(r["loss"]) - want) < 1e-12


def test_ctc_ref_equals_the_oracle_ctc_loss():
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(3, 20, 6, generator=g) * 2).bfloat16().double()
    lab = torch.tensor([[1, 1, 2, 0, -100], [3, 3, 3, 3, 3], [-100] * 5])
    r = ctc_ref(z, lab)
    assert abs(float(O.ctc_loss(z.float(), lab)) - float(r["loss"])) < 1e-5 * max(1.0, float(r["loss"]))


# ------------------------------------------------------------------------------------------------ CTC label preparation
def _label_cfg(remove):
    return O.OracleConfig(vocab_size=2000, eos_token_id=450, remove_timestamps_from_ctc=remove)


LABEL_BATCHES = {
    # first task token = 2000 - 1500 - 1 - 6 = 493; 440 / 441 are prefix tokens, 450 is eos
    "interior_pad": [[440, 441, 5, -100, 6, 7, 450, -100], [440, 441, 8, 9, -100, -100, 10, 450]],
    "eos_in_the_middle": [[440, 3, 450, 4, 5, 450], [440, 450, 450, 6, 7, 8]],
    "timestamps": [[440, 500, 3, 4, 510, 450, -100], [440, 520, 530, 5, 540, 6, 450]],
    "only_timestamps": [[440, 500, 510, 450], [440, 520, 450, -100]],
    "no_shared_prefix": [[440, 3, 4, 450], [441, 5, 450, -100]],
}


def _valid_rows(lab):
    return [[int(c) for c in row if c >= 0] for row in lab]


@pytest.mark.parametrize("remove", [False, True])
@pytest.mark.parametrize("name", sorted(LABEL_BATCHES))
def test_prepare_ctc_labels_agrees_with_the_oracle(name, remove):
    from ts_asr_whisper_amd import modeling
    cfg = _label_cfg(remove)
    labels = torch.tensor(LABEL_BATCHES[name], dtype=torch.long)
    ftt = cfg.vocab_size - 30 * 50 - 1 - 6
    got = modeling.prepare_ctc_labels(labels, cfg, (440, 441), ftt)
    want = O.ctc_prepare_labels(labels, cfg, (440, 441))
    assert got.shape == want.shape                                         # the widths (alpha / beta workspace) agree
    assert _valid_rows(got) == _valid_rows(want)                           # the same targets in the same order
    for row in got:                                                        # and the product has them as a prefix
        n = int((row >= 0).sum())
        assert bool((row[:n] >= 0).all()) and bool((row[n:] == -100).all())
    assert labels.tolist() == LABEL_BATCHES[name]                          # the caller's labels are left alone
    # get_loss applies the same remove-timestamps + valid-first steps inline (to labels whose prefix / eos are already handled):
    # run ITS code with the loss function stubbed out and compare with the oracle's preparation of the same labels
    enc = types.SimpleNamespace(config=cfg, first_task_token=ftt)
    keep = types.SimpleNamespace(apply=lambda self, logits, lab: lab)
    orig, modeling._CtcLossFn = modeling._CtcLossFn, keep
    try:
        inline = modeling.DiCoWEncoder.get_loss(enc, torch.zeros(1), labels)
    finally:
        modeling._CtcLossFn = orig
    noeos = types.SimpleNamespace(vocab_size=cfg.vocab_size, eos_token_id=-12345, remove_timestamps_from_ctc=remove)
    want2 = O.ctc_prepare_labels(labels, noeos, ())
    assert inline.shape == want2.shape and _valid_rows(inline) == _valid_rows(want2)
    for row in inline:
        n = int((row >= 0).sum())
        assert bool((row[:n] >= 0).all()) and bool((row[n:] == -100).all())


def test_prepare_ctc_labels_refuses_a_label_beyond_the_vocabulary():
    from ts_asr_whisper_amd import modeling
    cfg = _label_cfg(False)
    with pytest.raises(ValueError):
        modeling.prepare_ctc_labels(torch.tensor([[3, 2000]]), cfg, (), 493)

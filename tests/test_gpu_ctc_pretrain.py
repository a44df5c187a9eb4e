"""CTC pre-training of the encoder (stage 0 of the reference's recipe: src/pretrain_encoder.py with configs/pretrain/*.yaml -- use_fddt false,
no STNO mask in the batch, only the CTC head trains) end to end on the GPU, driven by the INSTALLED ``transformers.Trainer``.  None of the
reference's Python runs here: ``_PretrainTrainer`` restates what CustomTrainerEncoder (src/utils/trainers.py:31-103) does in its
``compute_loss`` and ``prediction_step``.

Toy encoder: d_model 128, 2 layers, vocab 300, ctc_weight 0.3, pre_ctc_sub_sample, additional_self_attention_layer, use_fddt False.
max_source_positions is 152, not 150: the CTC head's two stride-2 convolutions need a multiple of 4 (CtcEngine.encode_logits refuses anything
else), so a window is 304 mel frames -> 38 CTC frames, the long inputs are 608 and 912 frames, and 700 is the length that is no whole number
of windows.  Run with `pytest -m gpu`."""
import pytest
import torch

import amd_pkg
from tests.ctc_greedy_ref import greedy_restatement

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
# configs/pretrain/base.yaml:24,26 has lr 3e-4, weight decay 1e-6.  At 3e-4 three AdamW steps collapse this toy head onto the blank (every
# frame decodes to nothing, with the oracle on the CPU as well), which would leave the evaluation below nothing to tell rows apart by; at a
# tenth of it the head still moves in every step and the decoded rows stay non-empty and different.
LR, WD = 3e-5, 1e-6
L_LAB, WIN, TN = 10, 304, 38


def _cfg(**over):
    kw = dict(vocab_size=300, d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=1, decoder_attention_heads=2,
              encoder_ffn_dim=256, decoder_ffn_dim=256, num_mel_bins=80, max_source_positions=152, max_target_positions=32,
              pad_token_id=1, bos_token_id=1, eos_token_id=2, decoder_start_token_id=3, ctc_weight=0.3, pre_ctc_sub_sample=True,
              additional_self_attention_layer=True, use_fddt=False)
    kw.update(over)
    return pkg.DiCoWConfig(**kw)


def _encoder(cfg, freeze=True):
    torch.manual_seed(11)
    enc = pkg.DiCoWEncoder(cfg)
    if cfg.ctc_weight > 0:
        # a head that decodes to something: a freshly initialised one attends almost uniformly (every CTC frame alike) and never prefers the
        # blank.  Peaked attention, larger logits and a strong blank row give rows of tokens, repeats and blanks, different for every input.
        with torch.no_grad():
            enc.additional_self_attention_layer.q_proj.weight.mul_(30.0)
            enc.lm_head.weight.mul_(4.0)
            enc.lm_head.weight[cfg.vocab_size].mul_(8.0)
    return pkg.freeze_for_ctc_pretraining(enc) if freeze else enc


def _mel(B, frames, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 80, frames, generator=g).clamp_(-1.5, 1.5)


def _samples(n, frames, seed):
    """n items as DataCollatorForPretraining hands them over: input_features, attention_mask, labels -- no stno_mask."""
    out = []
    g = torch.Generator().manual_seed(seed)
    for i in range(n):
        lab = torch.randint(4, 200, (L_LAB,), generator=g)
        lab[0] = 3                                                       # the decoder prompt's first token, shared by the batch
        lab[-1] = 2                                                      # eos
        if i % 2:
            lab[-3:] = -100
        out.append({"input_features": _mel(1, frames, seed + 1 + i)[0], "attention_mask": torch.ones(frames, dtype=torch.long), "labels": lab})
    return out


def _collate(items):
    return {k: torch.stack([it[k] for it in items]) for k in items[0]}


class _Stream(torch.utils.data.IterableDataset):
    """Items in a fixed order, over and over (an IterableDataset: the trainer's sampler does not shuffle it)."""

    def __init__(self, items):
        self.items = items

    def __iter__(self):
        while True:
            yield from self.items


class _Tok:
    prefix_tokens = [3]
    eos_token_id = 2


def _train_labels(labels, tok):
    """What the pre-training trainer does to the labels before the loss: drop prompt tokens the whole batch shares, eos -> -100."""
    labels = labels.clone()
    for t in tok.prefix_tokens:
        if bool((labels[:, 0] == t).all()):
            labels = labels[:, 1:]
    labels[labels == tok.eos_token_id] = -100
    return labels


def _non_trivial(dec, pad=1):
    """A decode that can tell rows apart: tokens and padding in every row (so frames were dropped or merged), no two rows alike."""
    dec = torch.as_tensor(dec)
    n = (dec != pad).sum(1)
    assert bool((n > 0).all()) and bool((n < dec.shape[1]).all()), n.tolist()
    assert len({tuple(r.tolist()) for r in dec}) == dec.shape[0]
    return int(n.sum())


def _optimizer(enc):
    """reference src/models/containers.py:100-114 (`get_optimizer`) as src/pretrain_encoder.py:87 calls it: no prefixes with a higher rate,
    so every parameter sits in the first group and the second one is empty."""
    return torch.optim.AdamW([{"params": list(enc.parameters())}, {"params": [], "lr": 100.0 * LR, "weight_decay": 0.0}], lr=LR, weight_decay=WD)


@pytest.fixture(scope="module")
def enc():
    return _encoder(_cfg()).cuda()


def test_forward_without_stno_is_bit_equal_and_fddt_still_needs_it(enc):
    x = _mel(2, WIN, 1).cuda()
    st = torch.softmax(torch.randn(2, 4, 152, generator=torch.Generator().manual_seed(2)), dim=1).cuda()
    with torch.no_grad():
        a = enc(x, return_logits=True)
        b = enc(x, stno_mask=st, return_logits=True)
        c = enc(x, attention_mask=torch.ones(2, WIN, device="cuda"))
    assert a.logits.shape == (2, TN, 301) and a.logits.dtype == torch.bfloat16 and a.logits.stride() == (TN * 384, 384, 1)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.hidden_states, b.hidden_states)
    assert torch.equal(c.last_hidden_state, a.hidden_states)
    fddt = pkg.DiCoWEncoder(_cfg(use_fddt=True, fddt_is_diagonal=True)).cuda()
    with pytest.raises(ValueError, match="stno_mask is required"):
        fddt(x, return_logits=True)
    with pytest.raises(ValueError, match="stno_mask is required"):       # enrollments carry masks of their own: no stand-in for the mixture's
        enc(x, enrollments={"input_features": x, "stno_mask": st})


def test_frozen_encoder_keeps_no_activations(enc):
    """freeze_for_ctc_pretraining: grad mode on, yet the encoder proper runs its inference form -- its output is no autograd node (the
    engine's state is kept exactly when it is one) and the forward holds less memory than that of an encoder that trains everything."""
    x = _mel(2, WIN, 3).cuda()
    every = _encoder(_cfg(), freeze=False).cuda()

    def held(model):
        model(x, return_logits=True)                                     # (engines prepared, workspaces allocated)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = model(x, return_logits=True)
        torch.cuda.synchronize()
        return out, torch.cuda.memory_allocated() - before

    out, kept = held(enc)
    out_all, kept_all = held(every)
    assert out.hidden_states.grad_fn is None and not out.hidden_states.requires_grad and out.logits.requires_grad
    assert out_all.hidden_states.grad_fn is not None
    print(f"forward holds {kept} bytes frozen, {kept_all} bytes with every parameter trainable")
    assert kept < kept_all
    labels = torch.randint(4, 200, (2, 8), generator=torch.Generator().manual_seed(4)).cuda()
    enc.get_loss(out.logits, labels).backward()
    got = {n for n, p in enc.named_parameters() if p.grad is not None}
    assert got == {n for n, p in enc.named_parameters() if p.requires_grad} and all(n.startswith(enc._CTC_PREFIXES) for n in got)
    enc.zero_grad(set_to_none=True)


@pytest.mark.parametrize("frames", [608, 912])
def test_chunked_logits_equal_the_windows_side_by_side(enc, frames):
    x = _mel(2, frames, frames).cuda()
    labels = torch.randint(4, 200, (2, 12), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        got = pkg.chunked_ctc_logits(enc, x)
        parts = [enc(x[..., w:w + WIN], return_logits=True).logits for w in range(0, frames, WIN)]
        want = torch.cat(parts, dim=1)
        n = frames // WIN
        assert got.shape == (2, n * TN, 301) and got.stride() == (n * TN * 384, 384, 1) and got.dtype == torch.bfloat16
        assert torch.equal(got, want)
        # the view feeds the loss and the decoder as it is
        assert abs(float(enc.get_loss(got, labels)) - float(enc.get_loss(want, labels))) < 1e-5
        dec = pkg.ctc_greedy_decode(got, 300, 1)
        assert torch.equal(dec.cpu(), greedy_restatement(want, 300, 1))
        _non_trivial(dec.cpu())
        st = torch.softmax(torch.randn(2, 4, frames // 2, generator=torch.Generator().manual_seed(6)), dim=1).cuda()
        assert torch.equal(pkg.chunked_ctc_logits(enc, x, st), want)


def test_chunked_logits_refuse_a_short_last_window_and_grad_mode(enc):
    with torch.no_grad():
        with pytest.raises(ValueError, match="304"):
            pkg.chunked_ctc_logits(enc, _mel(2, 700, 7).cuda())
    with pytest.raises(pkg._lib.DicowError, match="no_grad"):
        pkg.chunked_ctc_logits(enc, _mel(2, 608, 7).cuda())


def test_greedy_decode_of_the_products_own_padded_view(enc):
    with torch.no_grad():
        out = enc(_mel(3, WIN, 8).cuda(), return_logits=True)
    assert out.logits.stride(1) == 384 and out.logits.shape[-1] == 301
    got = pkg.ctc_greedy_decode(out.logits, 300, 1)
    assert got.dtype == torch.int64 and got.shape == (3, TN)
    assert torch.equal(got.cpu(), greedy_restatement(out.logits.float().cpu(), 300, 1))     # the same bf16 values on both sides: exact
    _non_trivial(got.cpu())


def test_get_loss_takes_dense_bf16_logits_of_odd_width(enc):
    """What a concatenation of windows looks like (the reference's prediction_step): bf16 [B, Tn, 301] with rows 301 apart.  The CTC kernels
    read bf16 pairs from even rows, so get_loss copies such a tensor into padded rows: same loss as the padded view, and a gradient."""
    with torch.no_grad():
        out = enc(_mel(2, WIN, 9).cuda(), return_logits=True)
    labels = torch.randint(4, 200, (2, 8), generator=torch.Generator().manual_seed(10)).cuda()
    dense = out.logits.contiguous().requires_grad_(True)
    assert dense.dtype == torch.bfloat16 and dense.stride() == (TN * 301, 301, 1)
    loss = enc.get_loss(dense, labels)
    assert float(loss) == float(enc.get_loss(out.logits, labels))           # the same values through the same kernels
    loss.backward()
    assert dense.grad.shape == dense.shape and bool(torch.isfinite(dense.grad.float()).all()) and float(dense.grad.float().abs().sum()) > 0


def test_installed_trainer_pretrains_and_evaluates_with_greedy_decoding(tmp_path):
    import transformers
    from transformers import Trainer, TrainingArguments
    cfg = _cfg()
    items, long_items = _samples(4, WIN, 500), _samples(4, 2 * WIN, 600)
    tok = _Tok()

    class _PretrainTrainer(Trainer):
        """CustomTrainerEncoder in this test's words: the loss is the encoder's CTC loss of its own logits; an evaluation input longer than
        one window is cut into windows whose logits stand side by side."""

        def compute_loss(self, model, inputs, return_outputs=False, num_items_in_batch=None):
            labels = inputs.pop("labels")
            outputs = model(**inputs, return_logits=True)
            loss = model.get_loss(outputs.logits, _train_labels(labels, tok))
            return (loss, outputs) if return_outputs else loss

        def prediction_step(self, model, inputs, prediction_loss_only, ignore_keys=None):
            inputs = self._prepare_inputs(inputs)
            labels = inputs.pop("labels")
            x = inputs[model.main_input_name]
            with torch.no_grad(), self.compute_loss_context_manager():
                if x.size(-1) > model.get_max_len():
                    logits = pkg.chunked_ctc_logits(model, x)
                else:
                    logits = model(**inputs, return_logits=True).logits
                loss = model.get_loss(logits, labels).detach()
            return (loss, None, None) if prediction_loss_only else (loss, logits, labels)

    # ---- the eager twin first: plain loop, torch's clip, the same optimizer recipe, the trainer's autocast
    twin = _encoder(cfg).cuda()
    opt2 = _optimizer(twin)
    eager_losses = []
    for step in range(3):
        batch = {k: v.cuda() for k, v in _collate([items[(2 * step) % 4], items[(2 * step + 1) % 4]]).items()}
        labels = batch.pop("labels")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = twin.get_loss(twin(**batch, return_logits=True).logits, _train_labels(labels, tok))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
        opt2.step()
        opt2.zero_grad()
        eager_losses.append(float(loss))

    # ---- the installed trainer on a second copy
    model = _encoder(cfg)
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    args = TrainingArguments(output_dir=str(tmp_path / "out"), per_device_train_batch_size=2, per_device_eval_batch_size=2, max_steps=3,
                             learning_rate=LR, lr_scheduler_type="constant", weight_decay=WD, max_grad_norm=1.0, bf16=True, logging_steps=1,
                             save_strategy="no", eval_strategy="no", report_to="none", remove_unused_columns=False,
                             dataloader_num_workers=0, dataloader_pin_memory=False, seed=0, disable_tqdm=True)
    seen = {}

    def compute_metrics(pred):
        seen["pred"], seen["labels"] = pred.predictions, pred.label_ids
        return {"tokens": float((pred.predictions != cfg.pad_token_id).sum())}

    trainer = _PretrainTrainer(model=model, args=args, train_dataset=_Stream(items), eval_dataset=long_items, data_collator=_collate,
                               optimizers=(_optimizer(model), None), compute_metrics=compute_metrics,
                               preprocess_logits_for_metrics=lambda logits, labels: pkg.ctc_greedy_decode(logits, cfg.vocab_size, cfg.pad_token_id))
    out = trainer.train()
    assert out.global_step == 3
    logged = [h["loss"] for h in trainer.state.log_history if "loss" in h]
    assert len(logged) == 3
    assert logged == eager_losses                                        # logging_steps = 1: each logged value is that step's loss, bit for bit
    head = tuple(model._CTC_PREFIXES)
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n                    # every parameter, the CTC head's included, bit for bit
        if n.startswith(head):
            assert p.requires_grad and not torch.equal(p.detach().cpu(), start[n]), n       # ... and the head moved
        else:
            assert not p.requires_grad and torch.equal(p.detach().cpu(), start[n]), n       # ... and nothing else did

    # ---- evaluate(): two-window inputs -> chunked logits -> greedy CTC decoding on the GPU -> compute_metrics
    metrics = trainer.evaluate()
    assert metrics["eval_loss"] > 0 and metrics["eval_tokens"] == _non_trivial(seen["pred"], cfg.pad_token_id)
    assert seen["pred"].shape == (4, 2 * TN) and seen["pred"].dtype.kind == "i" and seen["labels"].shape == (4, L_LAB)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        direct, losses = [], []
        for i in (0, 2):
            batch = {k: v.cuda() for k, v in _collate(long_items[i:i + 2]).items()}
            logits = pkg.chunked_ctc_logits(model, batch["input_features"])
            direct.append(pkg.ctc_greedy_decode(logits, cfg.vocab_size, cfg.pad_token_id).cpu())
            losses.append(float(model.get_loss(logits, batch["labels"])))
            assert torch.equal(direct[-1], greedy_restatement(logits, cfg.vocab_size, cfg.pad_token_id))
    assert torch.equal(torch.as_tensor(seen["pred"]), torch.cat(direct))   # what the trainer collected is what a direct call returns
    assert abs(metrics["eval_loss"] - 0.5 * sum(losses)) < 1e-5
    # ---- and one-window inputs through the same prediction_step
    short = trainer.evaluate(eval_dataset=items)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        batch = {k: v.cuda() for k, v in _collate(items[:2]).items()}
        one = pkg.ctc_greedy_decode(model(batch["input_features"], return_logits=True).logits, cfg.vocab_size, cfg.pad_token_id).cpu()
    assert seen["pred"].shape == (4, TN) and torch.equal(torch.as_tensor(seen["pred"][:2]), one)
    _non_trivial(seen["pred"], cfg.pad_token_id)
    print("transformers", transformers.__version__, "losses", logged, "toy sizes (B = 2, 304 / 608 mel frames, d_model 128): train",
          {k: round(v, 4) for k, v in out.metrics.items() if isinstance(v, float)}, "eval (4 two-window items)",
          {k: round(v, 4) for k, v in metrics.items() if isinstance(v, float)}, "eval (4 one-window items)",
          {k: round(v, 4) for k, v in short.items() if isinstance(v, float)})

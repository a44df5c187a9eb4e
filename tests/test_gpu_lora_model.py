"""LoRA adapters on the decoder end to end on the GPU (add_decoder_lora -> engine.lora_fwd / lora_bwd -> dicow_lora_*): the zero-B
identity, loss and gradients against the CPU oracle on merged weights, decoding with adapters, merge_lora, and a LoRA TrainStep on a
frozen decoder.  Toy configuration of test_config_variants_end_to_end_vs_oracle, B = 2, L = 10.  Run with `pytest -m gpu`."""
import pytest
import torch

import amd_pkg
from oracle import dicow_oracle as O
from tests.util import maxdiff
from tests.test_gpu_model import _check_grads, rel

pytestmark = pytest.mark.gpu
amd_pkg.load()

KW = dict(vocab_size=512, d_model=128, encoder_layers=3, encoder_attention_heads=2, decoder_layers=2, decoder_attention_heads=2,
          encoder_ffn_dim=256, decoder_ffn_dim=256, max_source_positions=100, max_target_positions=32, pad_token_id=500,
          bos_token_id=500, eos_token_id=500, decoder_start_token_id=501, num_mel_bins=80, use_fddt=True, fddt_is_diagonal=True,
          use_pre_pos_fddt=True, fddt_init="suppressive", non_target_fddt_value=0.5)
B, L_ = 2, 10


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ts_asr_whisper_amd as p
    return p


@pytest.fixture(scope="module")
def toy(pkg):
    """(config, base state dict on the CPU, CPU batch tensors): shared, never modified."""
    cfg = pkg.DiCoWConfig(**KW)
    torch.manual_seed(3)
    model = pkg.DiCoWForConditionalGeneration(cfg)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if "fddt" in n:
                p_.add_(torch.randn(p_.shape, generator=g) * 0.05)
    state = {n: t.detach().clone() for n, t in model.state_dict().items()}
    x = torch.randn(B, 80, 200, generator=g).clamp_(-1.5, 1.5)
    st = torch.softmax(torch.randn(B, 4, 100, generator=g) * 2, dim=1)
    lab = torch.randint(0, 400, (B, L_), generator=g)
    return cfg, state, (x, st, lab)


def _model(pkg, toy, lora, random_b=False):
    cfg, state, _ = toy
    model = pkg.DiCoWForConditionalGeneration(cfg)
    model.load_state_dict(state, strict=True)
    if lora:
        torch.manual_seed(6)                   # (lora_A is drawn from the global generator: every model of this file gets the same A)
        pkg.add_decoder_lora(model)
        if random_b:
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for n, p_ in model.named_parameters():
                    if "lora_B" in n:
                        p_.copy_(torch.randn(p_.shape, generator=g) * 0.05)
    model = model.cuda()
    model.tie_weights()
    return model


def _batch(toy):
    x, st, lab = toy[2]
    return dict(input_features=x.cuda(), stno_mask=st.cuda(), labels=lab.cuda(), upp_labels=lab.cuda())


def test_zero_b_is_a_bit_exact_identity(pkg, toy):
    """Freshly attached adapters (B = 0) change no bit of logits, loss or any base gradient -- fc1's GELU, which moves from the GEMM
    epilogue into the `up` pass, and fc2's dgrad included -- while every dB is non-zero and every dA exactly zero."""
    plain, adapted = _model(pkg, toy, False), _model(pkg, toy, True)
    o0 = plain(**_batch(toy))
    o0.loss.backward()
    o1 = adapted(**_batch(toy))
    o1.loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(o0.logits, o1.logits) and torch.equal(o0.loss, o1.loss)
    g0 = {n: p.grad for n, p in plain.named_parameters()}
    n_enc = 0
    for n, p in adapted.named_parameters():
        if "lora_A" in n:
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0, n
        elif "lora_B" in n:
            assert p.grad is not None and float(p.grad.abs().max()) > 0.0, n
        elif g0[n] is None:
            assert p.grad is None, n
        else:
            assert torch.equal(p.grad, g0[n]), n
            n_enc += n.startswith("model.encoder.")
    assert n_enc >= 40


@pytest.fixture(scope="module")
def oracle_merged(pkg, toy):
    """The unchanged oracle on merged weights W + s B A (fp32 reference, and the emu=True run whose distance from it is the oracle's own
    bf16 deviation): loss and {name: gradient}, adapter gradients projected from the merged weight's: dA = s B^T dW', dB = s dW' A^T."""
    cfg, state, (x, st, lab) = toy
    model = _model(pkg, toy, True, random_b=True).cpu()
    full = {n: t.detach().clone() for n, t in model.state_dict().items()}
    mods = {n: m for n, m in model.named_modules() if isinstance(m, pkg.LoRALinear)}
    ocfg = O.OracleConfig(**{k: v for k, v in cfg.to_dict().items() if k in O.OracleConfig.__dataclass_fields__})
    out = {}
    for emu in (False, True):
        p = {n: t.clone() for n, t in full.items() if "lora_" not in n}
        for n, m in mods.items():
            p[n + ".weight"] = p[n + ".weight"] + m.scaling * (full[n + ".lora_B.weight"] @ full[n + ".lora_A.weight"])
        p = {n: t.requires_grad_(t.is_floating_point()) for n, t in p.items()}
        p["proj_out.weight"] = p["model.decoder.embed_tokens.weight"]
        ref = O.model_forward(p, ocfg, x, st, lab, lab, emu=emu)
        ref["loss"].backward()
        grads = {n: t.grad for n, t in p.items() if t.grad is not None and n != "proj_out.weight"}
        for n, m in mods.items():
            dW = grads[n + ".weight"]
            grads[n + ".lora_A.weight"] = m.scaling * (full[n + ".lora_B.weight"].T @ dW)
            grads[n + ".lora_B.weight"] = m.scaling * (dW @ full[n + ".lora_A.weight"].T)
        out[emu] = (float(ref["loss"].detach()), grads, ref["logits"].detach() if "logits" in ref else None)
    return out


def test_random_b_loss_and_gradients_vs_oracle_on_merged_weights(pkg, toy, oracle_merged):
    model = _model(pkg, toy, True, random_b=True)
    out = model(**_batch(toy))
    out.loss.backward()
    torch.cuda.synchronize()
    loss_ref, grads, _ = oracle_merged[False]
    _, grads_emu, _ = oracle_merged[True]
    print("loss", float(out.loss), "oracle fp32", loss_ref, "oracle emu", oracle_merged[True][0])
    named = {n: p for n, p in model.named_parameters() if p.grad is not None}
    assert not set(named) - set(grads) and sum("lora_" in n for n in named) == 2 * 10 * 2
    grads = {n: grads[n] for n in named}
    dev = {n: rel(grads_emu[n], grads[n]) for n in grads}
    for n in sorted(grads):                                                  # every figure before any assertion
        print(f"{n}: rel err {rel(named[n].grad.float().cpu(), grads[n]):.4f}  oracle emu-vs-fp32 {dev[n]:.4f}")
    assert abs(float(out.loss) - loss_ref) < 1e-2
    # adapter gradients: max(6e-2, 4 x the oracle's own bf16 deviation for the same projected gradient); everything else 6e-2
    worst = _check_grads(model, grads, tol_rel=6e-2, min_checked=len(named), ref_dev={n: d for n, d in dev.items() if "lora_" in n})
    print("worst grad rel err (LoRA, random B):", worst)


def test_decoding_runs_with_the_adapters(pkg, toy):
    from ts_asr_whisper_amd.generation import GreedyDecoder
    cfg, _, (x, st, _) = toy
    model = _model(pkg, toy, True, random_b=True)
    prompt = torch.tensor([[cfg.decoder_start_token_id, 7, 9]] * B)
    dec = GreedyDecoder(model)
    seq, scores = dec.generate(x.cuda(), st.cuda(), prompt, 8, eos_token_id=-1, return_scores=True)
    with torch.no_grad():
        full = model(input_features=x.cuda(), stno_mask=st.cuda(), decoder_input_ids=seq[:, :-1]).logits.float()
        plain = _model(pkg, toy, False)(input_features=x.cuda(), stno_mask=st.cuda(), decoder_input_ids=seq[:, :-1]).logits.float()
    for n in range(8):
        assert float((scores[n] - full[:, prompt.shape[1] - 1 + n]).abs().max()) < 4e-2, n
    print("adapters move the logits by", float((full - plain).abs().max()))
    assert float((full - plain).abs().max()) > 4e-2, "the adapters do not matter in this test"
    bseq, bscore = dec.beam_search(x.cuda(), st.cuda(), prompt, prompt.shape[1] + 6, 3, eos_token_id=-1)
    assert bseq.shape[0] == B and prompt.shape[1] < bseq.shape[1] <= prompt.shape[1] + 6
    assert bool(torch.isfinite(bscore.float()).all()) and bool(((bseq >= 0) & (bseq < cfg.vocab_size)).all())
    gseq = GreedyDecoder(model, use_graphs=True).generate(x.cuda(), st.cuda(), prompt, 8, eos_token_id=-1)      # the captured step
    assert torch.equal(gseq, seq)


def test_merge_lora_matches_the_unmerged_model(pkg, toy):
    cfg, state, (x, st, lab) = toy
    model = _model(pkg, toy, True, random_b=True)
    ids = torch.cat([torch.full((B, 1), cfg.decoder_start_token_id), lab[:, :-1]], 1).cuda()
    with torch.no_grad():
        before = model(input_features=x.cuda(), stno_mask=st.cuda(), decoder_input_ids=ids).logits.float()
        pkg.merge_lora(model)
        after = model(input_features=x.cuda(), stno_mask=st.cuda(), decoder_input_ids=ids).logits.float()
    assert set(model.state_dict().keys()) == set(state.keys())
    print("merge_lora: max logit difference", maxdiff(before, after))
    assert maxdiff(before, after) < 4e-2


def test_train_step_on_a_frozen_decoder_moves_only_the_adapters(pkg, toy):
    from ts_asr_whisper_amd.trainer import TrainStep

    def run():
        model = _model(pkg, toy, True, random_b=True)
        step = TrainStep(model, lr=1e-4, fddt_lr_multiplier=1.0, frozen_keywords=("decoder",), use_fddt_only_n_steps=1)
        lora = {n: p for n, p in model.named_parameters() if "lora_" in n}
        base = {n: p.detach().clone() for n, p in model.named_parameters() if "decoder" in n and "lora_" not in n}
        # frozen_keywords keeps the adapters trainable; the preheat phase (FDDT only, reference freeze_except) switches them off,
        # and the unfreeze that ends it switches them on again ("lora_" exception of trainers.py:124-126)
        assert step.warmup_phase and all(e[0] is not p for e in step.store.entries for p in base.values())
        assert {id(p) for p in lora.values()} <= {id(e[0]) for e in step.store.entries}
        start = {n: p.detach().clone() for n, p in lora.items()}
        losses, copies = [], None
        for k in range(3):
            losses.append(float(step.step(_batch(toy))))
            W = model._engine(prepare=False).W
            now = [(t.data_ptr(), t.clone()) for w in W.layers for lw in (w.sa.qkv, w.sa.o, w.ca.q, w.ca.kv, w.ca.o, w.fc1, w.fc2)
                   for t in (lw.w, lw.wt)] + [(W.head.w.data_ptr(), W.head.w.clone())]
            if k == 0:
                assert not any(p.requires_grad for p in lora.values())       # preheat step
            else:
                assert all(p.requires_grad for p in lora.values())
                assert not any(p.requires_grad for n, p in model.named_parameters() if "decoder" in n and "lora_" not in n)
            if k == 2:                                                        # steps 2 and 3 are LoRA steps: no re-cast of the base copies
                assert all(a[0] == b[0] and torch.equal(a[1], b[1]) for a, b in zip(copies, now))
            copies = now
        torch.cuda.synchronize()
        assert all(not torch.equal(p, start[n]) for n, p in lora.items()), "an adapter parameter did not move"
        assert all(torch.equal(p, base[n]) for n, p in model.named_parameters() if n in base), "a base decoder parameter moved"
        assert all(l == l and abs(l) < 1e3 for l in losses), losses
        return {n: p.detach().clone() for n, p in model.named_parameters()}

    first = run()
    second = run()
    assert all(torch.equal(first[n], second[n]) for n in first), "two identical runs differ"

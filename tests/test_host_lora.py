"""LoRA adapters on the decoder, host side (no GPU): attachment, state-dict keys, refusals, adapter files, freezing."""
import pytest
import torch

import amd_pkg

amd_pkg.load()


def _toy():
    import ts_asr_whisper_amd as pkg
    cfg = pkg.DiCoWConfig(vocab_size=512, d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=2, decoder_attention_heads=2,
                          encoder_ffn_dim=256, decoder_ffn_dim=256, max_source_positions=100, max_target_positions=32, pad_token_id=500,
                          bos_token_id=500, eos_token_id=500, decoder_start_token_id=501, num_mel_bins=80)
    torch.manual_seed(0)
    return pkg, pkg.DiCoWForConditionalGeneration(cfg), cfg


def test_add_decoder_lora_adapts_the_ten_decoder_linears_per_layer():
    pkg, model, cfg = _toy()
    base_keys = set(model.state_dict().keys())
    base_params = {n: p for n, p in model.named_parameters()}
    out = pkg.add_decoder_lora(model)
    assert out is model
    adapted = [n for n, m in model.named_modules() if isinstance(m, pkg.LoRALinear)]
    assert len(adapted) == 10 * cfg.decoder_layers and all(n.startswith("model.decoder.layers.") for n in adapted)
    assert not any(isinstance(m, pkg.LoRALinear) for m in model.model.encoder.modules())
    want = set(base_keys)
    for n in adapted:
        want |= {n + ".lora_A.weight", n + ".lora_B.weight"}
    assert set(model.state_dict().keys()) == want
    named = dict(model.named_parameters())
    assert all(named[n] is p for n, p in base_params.items()), "a base parameter was replaced"
    assert model.proj_out.weight is model.model.decoder.embed_tokens.weight
    assert all(getattr(m, "_is_hf_initialized", False) for m in model.modules())
    q = model.model.decoder.layers[0].self_attn.q_proj
    assert q.lora_A.weight.shape == (16, 128) and q.lora_B.weight.shape == (128, 16) and q.scaling == 2.0
    assert float(q.lora_B.weight.detach().abs().max()) == 0.0 and float(q.lora_A.weight.detach().abs().max()) > 0.0
    assert float(q.lora_A.weight.detach().abs().max()) <= 128 ** -0.5 + 1e-6          # kaiming-uniform, a = sqrt(5): bound 1 / sqrt(fan_in)
    fc2 = model.model.decoder.layers[1].fc2
    assert fc2.lora_A.weight.shape == (16, 256) and fc2.lora_B.weight.shape == (128, 16)


def test_add_decoder_lora_refusals():
    pkg, model, _ = _toy()
    with pytest.raises(NotImplementedError):
        pkg.add_decoder_lora(model, lora_dropout=0.1)
    with pytest.raises(NotImplementedError):
        pkg.add_decoder_lora(model, bias="all")
    with pytest.raises(ValueError):
        pkg.add_decoder_lora(model, target_modules=r".*(q_proj|v_proj)")         # matches the encoder's projections too
    with pytest.raises(ValueError):
        pkg.add_decoder_lora(model, target_modules=r"proj_out")                  # the LM head is outside the decoder layers
    with pytest.raises(ValueError):
        pkg.add_decoder_lora(model, r=12)
    with pytest.raises(ValueError):
        pkg.add_decoder_lora(model, target_modules=r"nothing_matches_this")
    assert not any(isinstance(m, pkg.LoRALinear) for m in model.modules()), "a refused call changed the model"
    pkg.add_decoder_lora(model)
    with pytest.raises(ValueError):
        pkg.add_decoder_lora(model)                                              # already attached


def test_adapter_files_round_trip(tmp_path):
    pkg, model, _ = _toy()
    pkg.add_decoder_lora(model, r=8, lora_alpha=16)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_" in n:
                p.copy_(torch.randn(p.shape, generator=g))
    model.save_adapter(str(tmp_path))
    from safetensors.torch import load_file
    sd = load_file(str(tmp_path / "adapter_model.safetensors"))
    mine = {n: p for n, p in model.named_parameters() if "lora_" in n}
    assert set(sd) == {"base_model.model." + n for n in mine} and len(sd) == 2 * 10 * 2
    assert "base_model.model.model.decoder.layers.0.self_attn.q_proj.lora_A.weight" in sd
    _, fresh, _ = _toy()
    fresh.load_adapter(str(tmp_path))                                            # attaches r = 8 adapters from adapter_config.json
    got = {n: p for n, p in fresh.named_parameters() if "lora_" in n}
    assert set(got) == set(mine) and all(torch.equal(got[n], mine[n]) for n in mine)
    assert fresh.model.decoder.layers[0].fc1.r == 8 and fresh.model.decoder.layers[0].fc1.scaling == 2.0
    _, other, _ = _toy()
    pkg.add_decoder_lora(other, target_modules=r".*decoder.*(fc1|fc2)")
    with pytest.raises(KeyError):
        other.load_adapter(str(tmp_path))


def test_merge_lora_restores_plain_linears():
    pkg, model, _ = _toy()
    keys = set(model.state_dict().keys())
    w0 = model.model.decoder.layers[0].fc1.weight.detach().clone()
    pkg.add_decoder_lora(model)
    fc1 = model.model.decoder.layers[0].fc1
    with torch.no_grad():
        fc1.lora_B.weight.normal_(generator=torch.Generator().manual_seed(2))
    delta = fc1.scaling * (fc1.lora_B.weight @ fc1.lora_A.weight).detach()
    pkg.merge_lora(model)
    assert set(model.state_dict().keys()) == keys
    assert not any(isinstance(m, pkg.LoRALinear) for m in model.modules())
    assert type(model.model.decoder.layers[0].fc1) is torch.nn.Linear
    assert torch.allclose(model.model.decoder.layers[0].fc1.weight, w0 + delta, atol=1e-6)
    assert model.proj_out.weight is model.model.decoder.embed_tokens.weight


def test_freeze_by_keyword_keeps_lora_trainable():
    pkg, model, _ = _toy()
    from ts_asr_whisper_amd.trainer import freeze_by_keyword
    pkg.add_decoder_lora(model)
    freeze_by_keyword(model, ("decoder",))
    for n, p in model.named_parameters():
        if "decoder" in n:
            assert p.requires_grad == ("lora_" in n), n
        else:
            assert p.requires_grad, n
    assert sum(p.requires_grad for n, p in model.named_parameters() if "decoder" in n) == 2 * 10 * 2

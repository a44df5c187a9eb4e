"""CPU tests of greedy CTC decoding's host side: the C-ABI entry point and its binding, the restatement of the reference's function that
the GPU tests use as their oracle (pinned to golden F22), and the wrappers' refusals.  No GPU needed."""
import os
import re

import pytest
import torch

import amd_pkg
from tests.ctc_greedy_ref import F22_CASES, greedy_restatement
from tests.util import ROOT, T, load_golden

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, ctc_decoding  # noqa: E402


def test_ctc_greedy_decode_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    m = re.search(r"^int\s+dicow_ctc_greedy_decode\s*\(([^;]*)\);", stable, flags=re.M)
    assert m is not None
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const void* logits", "int in_bf16", "int64_t batch_stride", "int64_t ld", "int B", "int Tn", "int V1", "int64_t blank",
                    "int64_t pad_id", "int* ws", "int64_t* out", "int64_t out_stride", "void* stream"]
    c = _lib
    assert _lib._SIGS["dicow_ctc_greedy_decode"] == [c.c_vp, c.c_i, c.c_i64, c.c_i64, c.c_i, c.c_i, c.c_i, c.c_i64, c.c_i64, c.c_vp, c.c_vp,
                                                     c.c_i64, c.c_vp]
    assert "dicow_ctc_greedy_decode" in _lib.declared_symbols()
    lib = _lib.lib()
    assert lib.dicow_ctc_greedy_decode.restype is c.c_i
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    p = 4096                                                              # (never dereferenced: every call below is refused on the host)
    ok = dict(logits=p, bf=1, bs=40 * 128, ld=128, B=4, Tn=40, V1=37, blank=36, pad=-100, ws=p, out=p, ostr=40)
    for bad in (dict(logits=None), dict(ws=None), dict(out=None), dict(B=0), dict(Tn=0), dict(V1=0), dict(ld=36), dict(ostr=39), dict(bs=-1),
                dict(B=1 << 16, Tn=1 << 15), dict(logits=p + 1), dict(logits=p + 2, bf=0)):
        a = dict(ok, **bad)
        rc = lib.dicow_ctc_greedy_decode(a["logits"], a["bf"], a["bs"], a["ld"], a["B"], a["Tn"], a["V1"], a["blank"], a["pad"], a["ws"],
                                         a["out"], a["ostr"], None)
        assert rc == -1, bad
        assert b"ctc_greedy_decode" in lib.dicow_last_error()


def test_restatement_reproduces_golden_f22_exactly():
    z = load_golden("f22_ctc_greedy")
    for name in F22_CASES:
        x, blank, pad = T(z, name + ".logits"), int(z[name + ".blank"]), int(z[name + ".pad"])
        assert x.shape == (4, 40, 37) and torch.equal(x, x.bfloat16().float())
        want = T(z, name + ".out")
        assert want.dtype == torch.int64
        assert torch.equal(greedy_restatement(x, blank, pad), want), name
        assert torch.equal(greedy_restatement(x.bfloat16(), blank, pad), want), name
    # the cases the fixture is there for
    c, inf = T(z, "crafted.out"), T(z, "inf.out")
    assert c[0].tolist() == [0] + [-100] * 39 and (c[1] == -100).all() and (c[2] != -100).all()
    assert c[3, :4].tolist() == [5, 5, 9, 9] and int(c[3][c[3] != -100][-1]) == 2
    assert inf[1].tolist() == [0] + [5] * 39
    assert (T(z, "blank50.out") == 36).any() and not (T(z, "random.out") == 36).any()


def test_wrappers_refuse_cpu_tensors_and_grad_mode():
    with pytest.raises(_lib.DicowError):
        ctc_decoding.ctc_greedy_decode(torch.zeros(2, 3, 5), 4, -100)
    assert pkg.ctc_greedy_decode is ctc_decoding.ctc_greedy_decode and pkg.chunked_ctc_logits is ctc_decoding.chunked_ctc_logits
    with pytest.raises(_lib.DicowError, match="no_grad"):
        ctc_decoding.chunked_ctc_logits(None, torch.zeros(1, 80, 600))


def test_encoder_surface_for_the_pretraining_trainer():
    cfg = pkg.DiCoWConfig(vocab_size=300, d_model=64, encoder_layers=1, encoder_attention_heads=1, decoder_layers=1, decoder_attention_heads=1,
                          encoder_ffn_dim=64, decoder_ffn_dim=64, max_source_positions=152, max_target_positions=32, ctc_weight=0.3,
                          pre_ctc_sub_sample=True, additional_self_attention_layer=True, use_fddt=False)
    enc = pkg.DiCoWEncoder(cfg)
    assert type(enc).main_input_name == "input_features" and enc.get_max_len() == 304
    keys = set(enc.state_dict())
    pkg.freeze_for_ctc_pretraining(enc)
    assert set(enc.state_dict()) == keys
    head = ("additional_layer.", "additional_self_attention_layer.", "subsample_conv1.", "subsample_conv2.", "lm_head.")
    train = [n for n, p in enc.named_parameters() if p.requires_grad]
    assert train and all(n.startswith(head) for n in train)
    assert all(p.requires_grad for n, p in enc.named_parameters() if n.startswith(head))
    assert [id(p) for p in enc.parameters() if p.requires_grad] == [id(p) for p in enc.ctc_parameters()]
    with pytest.raises(_lib.DicowError):
        pkg.freeze_for_ctc_pretraining(pkg.DiCoWEncoder(pkg.DiCoWConfig(vocab_size=300, d_model=64, encoder_layers=1, encoder_attention_heads=1,
                                                                         decoder_layers=1, decoder_attention_heads=1, encoder_ffn_dim=64,
                                                                         decoder_ffn_dim=64, max_source_positions=152, max_target_positions=32)))

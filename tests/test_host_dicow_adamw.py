"""CPU tests of the multi-tensor optimizer's host side (ts-asr-whisper_amd/optim.py): the C-ABI entry points, the chunk table, the
per-class scalars and the reference's param groups.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import torch

import amd_pkg
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, optim  # noqa: E402

NEW = ("dicow_multi_chunk_elems", "dicow_multi_adamw_f32", "dicow_multi_sumsq_f32", "dicow_multi_scale_f32",
       "dicow_multi_sumsq_ws_bytes")


def test_multi_tensor_abi_is_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(dicow_\w+)\s*\(", stable, flags=re.M))
    assert set(NEW) <= declared
    assert set(NEW) <= set(_lib.declared_symbols())
    assert "dicow_multi_sumsq_ws_bytes" in _lib._SIGS64
    lib = _lib.lib()
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    assert lib.dicow_multi_chunk_elems() == optim.CHUNK
    assert lib.dicow_multi_sumsq_ws_bytes(1000) >= 4 * 1000 and lib.dicow_multi_sumsq_ws_bytes(0) == 0
    m = re.search(r"#define DICOW_MT_MAX_CLASSES (\d+)", stable)
    assert int(m.group(1)) == _lib.MT_MAX_CLASSES == optim.MAX_CLASSES
    assert ctypes.sizeof(_lib.MtAdamwClasses) == 7 * 4 * _lib.MT_MAX_CLASSES + 4


def test_chunk_table_covers_every_element_once_with_int64_offsets():
    """A mixed list -- empty, tiny, odd, exactly one chunk, chunk + 1, and tensors past 2^31 elements in total (table only: nothing
    is allocated) -- each element in exactly one chunk, in table order, starts beyond int32."""
    C = optim.CHUNK
    numels = np.array([0, 1, 3, 5, 1280, 1281, C, C + 1, 4097, 1280 * 5120, 6_553_607, 3 * 2**30 + 7, 2**31 + 13], np.int64)
    T = len(numels)
    ptrs = np.zeros((T, 4), np.uint64)
    ptrs[:] = (np.arange(T, dtype=np.uint64) * np.uint64(1 << 36) + np.uint64(1 << 40))[:, None]
    ptrs[3, 2] += np.uint64(4)                                           # one misaligned exp_avg: scalar path for that tensor
    ptrs[4, 1] += np.uint64(8)                                           # one misaligned grad: scalar everywhere
    cls = np.arange(T, dtype=np.int32) % 3
    tensors, chunks = optim.build_table(ptrs, numels, cls)
    assert numels.sum() > 2**32
    assert tensors["n"].tolist() == numels.tolist() and tensors["cls"].tolist() == cls.tolist()
    flags = tensors["flags"].tolist()
    assert flags[0] == optim.ALIGNED_ALL | optim.ALIGNED_G
    assert flags[3] == optim.ALIGNED_G and flags[4] == 0
    assert chunks["start"].dtype == np.int64 and int(chunks["start"].max()) > 2**31
    assert np.all(np.diff(chunks["tensor"]) >= 0)                        # table order
    for t in range(T):
        mine = chunks[chunks["tensor"] == t]
        assert len(mine) == -(-int(numels[t]) // C)
        if len(mine):
            starts, lens = mine["start"].astype(np.int64), mine["len"].astype(np.int64)
            assert starts[0] == 0 and np.all(starts[1:] == starts[:-1] + lens[:-1])      # contiguous, no overlap, no gap
            assert int(starts[-1] + lens[-1]) == numels[t] and np.all((lens > 0) & (lens <= C))
    assert int(chunks["len"].astype(np.int64).sum()) == int(numels.sum())


def test_class_scalars_equal_torchs_double_precision_formulas():
    """What step() hands the kernel for every class is the fp32 value of torch's _single_tensor_adam host arithmetic (double)."""
    p0 = torch.nn.Parameter(torch.zeros(3))
    groups = [{"params": [p0]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.99)}]
    opt = optim.DiCoWAdamW(groups, lr=3e-4, weight_decay=0.05, eps=1e-7)
    cache = {"cls_group": [0, 0, 1], "cls_step": np.array([1, 7, 3])}
    (base, k), = opt._classes(cache)
    assert base == 0 and k.n_classes == 3
    f32 = lambda x: float(np.float32(x))
    for j, (gi, t) in enumerate([(0, 1), (0, 7), (1, 3)]):
        g = opt.param_groups[gi]
        lr, wd, (b1, b2), eps = g["lr"], g["weight_decay"], g["betas"], g["eps"]
        assert k.decay[j] == f32(1 - lr * wd)
        assert k.step_size[j] == f32(lr / (1 - b1 ** t))
        assert k.bc2_sqrt[j] == f32((1 - b2 ** t) ** 0.5)
        assert k.lerp_w[j] == f32(1 - b1) and k.beta2[j] == f32(b2) and k.one_minus_beta2[j] == f32(1 - b2) and k.eps[j] == f32(eps)
    many = {"cls_group": [0] * 70, "cls_step": np.arange(1, 71)}        # more classes than one launch carries: batches of 32
    batches = opt._classes(many)
    assert [b for b, _ in batches] == [0, 32, 64] and [k.n_classes for _, k in batches] == [32, 32, 6]


def test_dicow_optimizer_builds_the_reference_groups():
    """containers.py:100-114: every named parameter (frozen ones too) outside the prefixes at the base rate and weight decay, the
    prefixed ones at rate x multiplier with weight decay 0."""
    from ts_asr_whisper_amd.trainer import freeze_by_keyword
    cfg = pkg.DiCoWConfig(vocab_size=300, d_model=64, encoder_layers=2, encoder_attention_heads=1, decoder_layers=1,
                          decoder_attention_heads=1, encoder_ffn_dim=128, decoder_ffn_dim=128, num_mel_bins=80, max_source_positions=50,
                          max_target_positions=16, pad_token_id=1, bos_token_id=1, eos_token_id=2, decoder_start_token_id=3,
                          use_fddt=True, fddt_is_diagonal=True, use_pre_pos_fddt=True)
    with torch.device("meta"):
        model = pkg.DiCoWForConditionalGeneration(cfg)
    freeze_by_keyword(model, ("decoder",))
    opt = pkg.dicow_optimizer(model, 2e-4, weight_decay=0.01, fddt_lr_multiplier=100.0)
    prefixes = ("model.encoder.fddts", "model.encoder.initial_fddt")
    named = list(model.named_parameters())
    base = [p for n, p in named if not any(n.startswith(x) for x in prefixes)]
    new = [p for n, p in named if any(n.startswith(x) for x in prefixes)]
    assert len(opt.param_groups) == 2 and new and any(not p.requires_grad for p in base)
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in base]
    assert [id(p) for p in opt.param_groups[1]["params"]] == [id(p) for p in new]
    assert opt.param_groups[0]["lr"] == 2e-4 and opt.param_groups[0]["weight_decay"] == 0.01
    assert opt.param_groups[1]["lr"] == 100.0 * 2e-4 and opt.param_groups[1]["weight_decay"] == 0.0
    ref = torch.optim.AdamW([{"params": base}, {"params": new, "lr": 100.0 * 2e-4, "weight_decay": 0.0}], lr=2e-4, weight_decay=0.01)
    strip = lambda gs: [{k: v for k, v in g.items() if k != "params"} for g in gs]
    assert strip(opt.param_groups) == strip(ref.param_groups)           # the same group keys and values as torch's AdamW

"""``torch.optim.AdamW`` and ``torch.nn.utils.clip_grad_norm_`` over separate fp32 tensors, on the multi-tensor HIP kernels of
``csrc/optim.hip`` (include/dicow_hip.h, "multi-tensor optimizer").

``DiCoWAdamW`` is a ``torch.optim.Optimizer`` with torch's AdamW constructor and state format, so it can be handed to the HF Trainer
in place of the two-group ``torch.optim.AdamW`` of the reference recipe (src/models/containers.py:100-114; ``dicow_optimizer``
builds those groups).  One ``step()`` is one launch over every parameter that has a gradient (two with ``max_grad_norm``).

How the host drives the kernels:
  * A device table describes a call: per tensor its four pointers (p, grad, exp_avg, exp_avg_sq), int64 element count, class and
    alignment flags; per chunk of ``CHUNK`` elements the tensor and the int64 start.  It is built with numpy and uploaded through a
    pinned staging buffer guarded by an event, and only when the pointers change: a step compares a tuple of ``data_ptr()``s.
  * A class is (param group, per-parameter step count).  Its scalars (1 - lr wd, lr / (1 - beta1^t), sqrt(1 - beta2^t), ...) are
    computed in double, as torch's single-tensor AdamW computes them, and passed to the kernel as fp32 arguments.  Between two
    table builds every parameter of the table advances by one step per ``step()``, so the classes are known without reading the
    CPU step tensors.  At a table build the step tensors of the table's parameters become 0-dim views of one CPU tensor (still one
    CPU float tensor per parameter, torch's format), advanced by one ``add_`` per step.
  * No host synchronisation per step.

Differences from torch (documented, deliberate):
  * ``max_grad_norm`` (fused clip): the global 2-norm of the gradients this optimizer updates is computed on the device and the
    clip coefficient is applied INSIDE the update; ``p.grad`` is left unscaled, where ``torch.nn.utils.clip_grad_norm_`` scales it in
    place.  The norm of the last step is ``last_grad_norm`` (a 0-dim device tensor).
  * amsgrad, maximize, capturable, differentiable and a tensor lr raise ``NotImplementedError``; sparse, non-fp32, non-contiguous
    or CPU tensors raise ``DicowError`` (there is no CPU fallback).
  * The cached classes assume that ``state['step']`` changes only through ``step()`` and ``load_state_dict()``.
"""
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import ops

CHUNK = 2048                       # DICOW_MT_CHUNK (checked against the library when it is loaded)
MAX_CLASSES = L.MT_MAX_CLASSES
ALIGNED_ALL, ALIGNED_G = 1, 2
TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("cls", "<i4"), ("flags", "<i4")])
CHUNK_DT = np.dtype([("start", "<i8"), ("tensor", "<i4"), ("len", "<i4")])
assert TENSOR_DT.itemsize == 48 and CHUNK_DT.itemsize == 16
PRESET_PREFIXES = ("model.encoder.fddts", "model.encoder.initial_fddt")    # configs/base.yaml:18 prefixes_to_preheat


def build_table(ptrs, numels, cls=None):
    """Host side of the device table.  ptrs: uint64 [T, 4] (p, g, m, v; 0 where unused), numels: int64 [T], cls: int32 [T] or None.
    Returns (tensors, chunks) as numpy structured arrays (TENSOR_DT, CHUNK_DT): every element of every tensor lies in exactly one
    chunk, chunks in table order, int64 starts."""
    ptrs = np.asarray(ptrs, dtype=np.uint64).reshape(-1, 4)
    numels = np.asarray(numels, dtype=np.int64)
    T = numels.shape[0]
    tensors = np.zeros(T, TENSOR_DT)
    tensors["p"], tensors["g"], tensors["m"], tensors["v"] = ptrs[:, 0], ptrs[:, 1], ptrs[:, 2], ptrs[:, 3]
    tensors["n"] = numels
    tensors["cls"] = 0 if cls is None else np.asarray(cls, dtype=np.int32)
    aligned = (ptrs % np.uint64(16)) == 0
    tensors["flags"] = np.where(aligned.all(axis=1), ALIGNED_ALL, 0) | np.where(aligned[:, 1], ALIGNED_G, 0)
    nch = (numels + CHUNK - 1) // CHUNK
    total = int(nch.sum())
    tix = np.repeat(np.arange(T, dtype=np.int64), nch)
    start = np.arange(total, dtype=np.int64)
    start -= np.repeat(np.cumsum(nch) - nch, nch)
    start *= CHUNK
    raw = np.empty((total, 2), np.int64)                  # (start, tensor | len << 32): the CHUNK_DT layout, little-endian
    raw[:, 0] = start
    raw[:, 1] = tix | (np.minimum(numels[tix] - start, CHUNK) << 32)
    chunks = raw.view(CHUNK_DT).reshape(total)
    return tensors, chunks


def first_chunks(numels):
    """int64 [T + 1]: tensor i owns the chunks [first[i], first[i + 1]) of build_table's chunk list (table order; an empty tensor owns
    none).  What the per-tensor passes of csrc/tensor_stats.hip walk."""
    nch = (np.asarray(numels, dtype=np.int64) + CHUNK - 1) // CHUNK
    first = np.zeros(nch.shape[0] + 1, np.int64)
    np.cumsum(nch, out=first[1:])
    return first


class _DeviceTable:
    """One device copy of a table, refreshed through a pinned staging buffer.  The event of the last copy guards the staging buffer:
    it is rewritten only after the copy out of it has run (at a rebuild, never per step).  Kernels read the device copy in stream
    order on the current stream."""

    def __init__(self):
        self.dev = self.pinned = self.event = None
        self.n_chunks = 0

    def upload(self, tensors, chunks, device):
        off = (tensors.nbytes + 255) // 256 * 256
        total = off + chunks.nbytes
        if self.event is not None:
            self.event.synchronize()
        if self.pinned is None or self.pinned.numel() < total:
            self.pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        if self.dev is None or self.dev.numel() < total or self.dev.device != device:
            self.dev = torch.empty(total, dtype=torch.uint8, device=device)
        host = self.pinned.numpy()
        host[:tensors.nbytes] = tensors.view(np.uint8)
        host[off:total] = chunks.view(np.uint8)
        self.dev[:total].copy_(self.pinned[:total], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        self.tensors_ptr, self.chunks_ptr, self.n_chunks = self.dev.data_ptr(), self.dev.data_ptr() + off, len(chunks)
        return self


_SUMSQ_WS = {}


def _sumsq_ws(n_chunks, device):
    """Zeroed per-(device, stream) workspace of the deterministic sum of squares (left zero by every call)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    need = ops.multi_sumsq_ws_bytes(n_chunks)
    ws = _SUMSQ_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(max(need, 1 << 20), dtype=torch.uint8, device=device)
        _SUMSQ_WS[key] = ws
    return ws


def _check_tensor(t, what):
    if t.is_sparse:
        raise L.DicowError(f"{what}: sparse tensors are not supported")
    if not t.is_cuda:
        raise L.DicowError(f"{what}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype != torch.float32:
        raise L.DicowError(f"{what}: expected torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise L.DicowError(f"{what}: tensor must be contiguous")


def _norm_sumsq(table, device, max_norm):
    out = torch.empty(3, dtype=torch.float32, device=device)
    ops.multi_sumsq(table.tensors_ptr, table.chunks_ptr, table.n_chunks, _sumsq_ws(table.n_chunks, device), out, max_norm)
    return out


_CLIP_TABLES = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Drop-in for ``torch.nn.utils.clip_grad_norm_`` (2-norm): the total norm of every gradient as a 0-dim device tensor, gradients
    scaled in place by min(1, max_norm / (norm + 1e-6)).  Deterministic: a fixed-order reduction over a table that depends on the
    gradient sizes alone, so data-parallel replicas agree bit for bit.  ``max_norm = inf`` only measures (HF's ``_get_grad_norm``).
    ``foreach`` is accepted and ignored (always one multi-tensor pass)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm, norm_type = float(max_norm), float(norm_type)
    if norm_type != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: norm_type {norm_type} (only the 2-norm is implemented)")
    if not grads:
        return torch.tensor(0.0)
    key = tuple(g.data_ptr() for g in grads) + tuple(g.numel() for g in grads)
    table = _CLIP_TABLES.get(key)
    if table is None:
        for g in grads:
            _check_tensor(g, "clip_grad_norm_")
        device = grads[0].device
        if any(g.device != device for g in grads):
            raise L.DicowError("clip_grad_norm_: gradients on more than one device")
        ptrs = np.zeros((len(grads), 4), np.uint64)
        ptrs[:, 1] = [g.data_ptr() for g in grads]
        if len(_CLIP_TABLES) >= 8:
            _CLIP_TABLES.pop(next(iter(_CLIP_TABLES)))
        table = _CLIP_TABLES[key] = _DeviceTable().upload(*build_table(ptrs, [g.numel() for g in grads]), device)
    if table.n_chunks == 0:
        return torch.zeros((), device=grads[0].device)
    out = _norm_sumsq(table, grads[0].device, max_norm)
    total = out[1]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped.")
    if math.isfinite(max_norm):
        ops.multi_scale(table.tensors_ptr, table.chunks_ptr, table.n_chunks, out[2:])
    return total


class DiCoWAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` on the multi-tensor HIP kernels (same constructor, param groups and ``state_dict`` format: a state dict
    of either loads into the other).  ``max_grad_norm``: fused global-norm clip -- the coefficient is applied inside the update,
    ``p.grad`` stays unscaled (torch's clip scales it in place); ``last_grad_norm`` holds the norm of the last step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm: Optional[float] = None):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("DiCoWAdamW: a tensor lr is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._cache = None
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)
        if L.lib().dicow_multi_chunk_elems() != CHUNK:
            raise L.DicowError("DiCoWAdamW: the library's DICOW_MT_CHUNK differs from optim.CHUNK (stale build)")

    @staticmethod
    def _check_group(group):
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(flag, False):
                raise NotImplementedError(f"DiCoWAdamW: {flag}=True is not supported")
        if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise NotImplementedError("DiCoWAdamW: tensor lr / betas are not supported")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        self._cache = None

    def __setstate__(self, state):           # load_state_dict() lands here: new state tensors, new step counts
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True
        self._cache = None

    def _rebuild(self, key, per_group):
        """Validate, create missing state lazily (torch's format), read the step counts once, derive the classes, upload the table."""
        params, steps, ptrs, numels, cls_key = [], [], [], [], []
        device = None
        for gi, ps in enumerate(per_group):
            for p in ps:
                g = p.grad
                _check_tensor(p, "DiCoWAdamW: parameter")
                _check_tensor(g, "DiCoWAdamW: gradient")
                if g.shape != p.shape:
                    raise L.DicowError("DiCoWAdamW: gradient shape differs from its parameter's")
                device = device or p.device
                if p.device != device or g.device != device:
                    raise L.DicowError("DiCoWAdamW: parameters on more than one device")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s = st["step"]
                if s.device.type != "cpu" or s.dtype != torch.float32:
                    s = st["step"] = s.detach().to("cpu", torch.float32)
                for k in ("exp_avg", "exp_avg_sq"):
                    _check_tensor(st[k], f"DiCoWAdamW: state {k}")
                    if st[k].shape != p.shape:
                        raise L.DicowError(f"DiCoWAdamW: state {k} shape differs from its parameter's")
                params.append(p)
                steps.append(s)
                ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
                numels.append(p.numel())
                cls_key.append(gi)
        if not params:
            self._cache = None
            return None
        # the step counts of the table's parameters become 0-dim views of ONE CPU tensor (torch's format is kept: a CPU float tensor
        # per parameter), so a step advances them all with one add_
        backing = torch.stack(steps)
        for i, p in enumerate(params):
            self.state[p]["step"] = backing[i]
        now = backing.numpy().astype(np.int64)
        pairs = np.stack([np.asarray(cls_key, np.int64), now], axis=1)
        uniq, cls = np.unique(pairs, axis=0, return_inverse=True)
        tensors, chunks = build_table(np.asarray(ptrs, np.uint64), numels, cls.reshape(-1).astype(np.int32))
        old = self._cache
        table = old["table"] if old is not None else _DeviceTable()
        if len(chunks):
            table.upload(tensors, chunks, device)
        self._cache = dict(key=key, state=self.state, params=params, steps=backing, table=table, device=device,
                           n_chunks=len(chunks), cls_group=uniq[:, 0].tolist(), cls_step=uniq[:, 1].astype(np.int64))
        return self._cache

    def _classes(self, c):
        """Per-class scalars (double, as torch's _single_tensor_adam; cast to fp32) in batches of MAX_CLASSES."""
        out = []
        n = len(c["cls_group"])
        for base in range(0, n, MAX_CLASSES):
            k = L.MtAdamwClasses()
            k.n_classes = min(MAX_CLASSES, n - base)
            for j in range(k.n_classes):
                group = self.param_groups[c["cls_group"][base + j]]
                lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
                b1, b2 = (float(b) for b in group["betas"])
                t = float(c["cls_step"][base + j])
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
                k.decay[j] = 1 - lr * wd
                k.step_size[j] = lr / bc1
                k.bc2_sqrt[j] = bc2 ** 0.5
                k.lerp_w[j] = 1 - b1
                k.beta2[j] = b2
                k.one_minus_beta2[j] = 1 - b2
                k.eps[j] = eps
            out.append((base, k))
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
        per_group = [[p for p in group["params"] if p.grad is not None] for group in self.param_groups]
        flat = [p for ps in per_group for p in ps]
        try:
            key = (tuple(len(ps) for ps in per_group), tuple(p.data_ptr() for p in flat), tuple(p.grad.data_ptr() for p in flat))
        except RuntimeError:                 # a tensor without plain storage (sparse gradient): _rebuild says what is wrong
            key = None
        c = self._cache
        if c is not None and c["key"] == key and c["state"] is self.state:
            c["cls_step"] += 1
        else:
            c = self._rebuild(key, per_group)
            if c is None:
                return loss
            c["cls_step"] += 1
        c["steps"].add_(1.0)
        if c["n_chunks"]:
            table = c["table"]
            coef = None
            if self.max_grad_norm is not None:
                out = _norm_sumsq(table, c["device"], self.max_grad_norm)
                self.last_grad_norm = out[1]
                coef = out[2:]
            for base, k in self._classes(c):
                ops.multi_adamw(table.tensors_ptr, table.chunks_ptr, table.n_chunks, k, base, coef)
        # the model's bf16 weight copies are refreshed when (data_ptr, _version) changes: the kernel wrote p behind autograd's back
        torch.autograd.graph.increment_version(c["params"])
        return loss


def dicow_optimizer(model, learning_rate, weight_decay=0.0, fddt_lr_multiplier=100.0, prefixes_with_higher_lr=PRESET_PREFIXES,
                    **kwargs):
    """The reference's two groups (src/models/containers.py:100-114 ``get_optimizer``) on ``DiCoWAdamW``: every named parameter
    (frozen ones included; they have no gradient and are skipped) outside the prefixes at ``learning_rate`` / ``weight_decay``, the
    prefixed ones at ``learning_rate * fddt_lr_multiplier`` with weight decay 0.  ``kwargs`` go to ``DiCoWAdamW``."""
    prefixes = tuple(prefixes_with_higher_lr or ())
    named = list(model.named_parameters())
    base = [p for n, p in named if not any(n.startswith(x) for x in prefixes)]
    new = [p for n, p in named if any(n.startswith(x) for x in prefixes)]
    return DiCoWAdamW([{"params": base}, {"params": new, "lr": fddt_lr_multiplier * learning_rate, "weight_decay": 0.0}],
                      lr=learning_rate, weight_decay=weight_decay, **kwargs)

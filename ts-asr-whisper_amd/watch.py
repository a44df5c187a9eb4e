"""Gradient and parameter watch: per-tensor statistics and histograms of a list of fp32 GPU tensors in a handful of launches
(``csrc/tensor_stats.hip`` over the multi-tensor table of ``optim.build_table``) and one asynchronous download.

The reference turns this on with ``watch_grads`` (src/train.py:171 -> ``GradLogger``, src/utils/trainers.py:19-28 ->
``wandb.watch(model, log='all', log_freq=50)``): every 50 steps wandb's torch hook walks every parameter and gradient and, per tensor,
drops the non-finite values, takes ``min`` / ``max`` with ``.item()``, runs ``torch.histc(bins=64, min, max)``, copies it to the host and
builds ``torch.linspace(min, max, 65)`` edges under the keys ``gradients/<name>`` / ``parameters/<name>`` -- thousands of launches and
host synchronisations in one logged step.  Here:

  * ``tensor_stats(tensors, bins)``: three launches for the whole list (per-chunk partials, per-tensor fold, histogram), results stay on
    the device; ``.download()`` starts ONE copy into a pinned buffer behind an event, ``.result()`` waits for that event only.
  * ``GradWatch``: ``collect(step)`` launches the passes for the parameters and the gradients and hands the PREVIOUS collection, long
    downloaded, to the sink: logging never stalls the step that produced it.  ``flush()`` hands over the last one.
  * ``TrainStep(..., watch=GradWatch(...))`` collects at the end of every ``log_freq``-th step; ``WatchCallback`` does the same from the
    HF Trainer's ``on_pre_optimizer_step`` (the replacement for ``GradLogger``).

wandb is not a dependency: ``as_wandb(record)`` gives the ``np_histogram`` arguments, ``jsonl_sink(path)`` writes JSON lines.
There is no CPU fallback; sparse, non-fp32, non-contiguous or CPU tensors raise ``DicowError``.  What is not pinned to wandb is listed
in INTEGRATION.md ("Watching gradients and parameters").
"""
import json
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .optim import build_table, first_chunks, _check_tensor

MAX_BINS = L.STATS_MAX_BINS
REC_DT = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("min", "<f4"), ("max", "<f4"), ("absmax", "<f4"), ("reserved", "<i4"),
                   ("n_nan", "<i8"), ("n_posinf", "<i8"), ("n_neginf", "<i8"), ("n_zero", "<i8")])
assert REC_DT.itemsize == L.STATS_REC_BYTES


class _StatsTable:
    """Device copy of (tensors, chunks, first_chunk) for one list of pointers, plus the call's workspace.  Uploaded once through a
    pinned staging buffer; kernels read it in stream order."""

    def __init__(self, ptrs, numels, column, device):
        cols = np.zeros((len(ptrs), 4), np.uint64)
        cols[:, column] = ptrs
        tensors, chunks = build_table(cols, numels)
        first = first_chunks(numels)
        self.n_tensors, self.n_chunks = len(numels), len(chunks)
        self.numels = np.asarray(numels, np.int64)
        parts = [tensors.view(np.uint8), chunks.view(np.uint8), first.view(np.uint8)]
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += (a.nbytes + 255) // 256 * 256
        pinned = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        for o, a in zip(offs, parts):
            host[o:o + a.nbytes] = a.reshape(-1)
        self.dev = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        self.dev.copy_(pinned, non_blocking=True)
        self._pinned = pinned                                      # alive until the copy has run (the table outlives it)
        base = self.dev.data_ptr()
        self.tensors_ptr, self.chunks_ptr, self.first_ptr = base + offs[0], base + offs[1], base + offs[2]
        self.ws = None


_TABLES = {}


def _table(tensors, column):
    key = (column,) + tuple(t.data_ptr() for t in tensors) + tuple(t.numel() for t in tensors)
    tab = _TABLES.get(key)
    if tab is None:
        device = tensors[0].device
        for t in tensors:
            _check_tensor(t, "tensor_stats")
            if t.device != device:
                raise L.DicowError("tensor_stats: tensors on more than one device")
            if t.numel() and t.data_ptr() == 0:
                raise L.DicowError("tensor_stats: a non-empty tensor without storage (NULL column pointer)")
        if len(_TABLES) >= 8:
            _TABLES.pop(next(iter(_TABLES)))
        tab = _TABLES[key] = _StatsTable([t.data_ptr() for t in tensors], [t.numel() for t in tensors], column, device)
    return tab


def linspace_edges(lo, hi, bins):
    """wandb's edges: torch.linspace(min, max, bins + 1) on the CPU in fp32."""
    return torch.linspace(float(lo), float(hi), bins + 1, dtype=torch.float32).numpy()


class TensorStats:
    """Device results of one ``tensor_stats`` call.  ``download()`` starts the one copy and returns at once; ``result()`` waits for it."""

    def __init__(self, out, n_tensors, bins, numels):
        self._out, self.n_tensors, self.bins = out, n_tensors, bins
        self.numels = np.asarray(numels, np.int64)
        self._pinned = self._event = self._result = None

    @property
    def records(self):
        """uint8 device view of the n_tensors 64-byte records (REC_DT)."""
        return self._out[:self.n_tensors * REC_DT.itemsize]

    @property
    def hist(self):
        """int64 [n_tensors, bins] device view of the histograms."""
        return self._out[self.n_tensors * REC_DT.itemsize:].view(torch.int64).view(self.n_tensors, self.bins)

    def download(self):
        if self._event is None and self.n_tensors:
            self._pinned = torch.empty(self._out.numel(), dtype=torch.uint8, pin_memory=True)
            self._pinned.copy_(self._out, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
        return self

    def result(self):
        """dict of numpy arrays [n_tensors]: sum, sumsq (f8), min, max, absmax (f4), n_nan, n_posinf, n_neginf, n_zero, numel, n_finite
        (i8); 'hist' int64 [n_tensors, bins]; 'edges': per tensor torch.linspace(min, max, bins + 1) (empty without finite elements)."""
        if self._result is None:
            if self.n_tensors:
                self.download()
                self._event.synchronize()
                raw = self._pinned.numpy()
            else:
                raw = np.zeros(0, np.uint8)
            nrec = self.n_tensors * REC_DT.itemsize
            rec = raw[:nrec].view(REC_DT)
            res = {k: rec[k].copy() for k in REC_DT.names if k != "reserved"}
            res["numel"] = self.numels.copy()
            res["n_finite"] = self.numels - res["n_nan"] - res["n_posinf"] - res["n_neginf"]
            res["hist"] = raw[nrec:].view(np.int64).reshape(self.n_tensors, self.bins).copy()
            res["edges"] = [linspace_edges(lo, hi, self.bins) if nf > 0 and self.bins else np.zeros(0, np.float32)
                            for lo, hi, nf in zip(res["min"], res["max"], res["n_finite"])]
            self._result = res
            self._pinned = None
        return self._result


def tensor_stats(tensors, bins=64, *, column=0, grid=0):
    """Statistics and ``bins``-bin histograms (torch.histc(bins, min, max) over the finite elements; bins = 0: statistics only) of
    every tensor of a list of contiguous fp32 GPU tensors, as a ``TensorStats`` (results on the device; nothing waits).  The device
    table is cached by the tensors' pointers.  ``column`` (0..3) is the table column the pointers are placed in and read from;
    ``grid`` > 0 forces the kernels' grids (the results do not depend on either)."""
    tensors = list(tensors)
    bins = int(bins)
    if not 0 <= bins <= MAX_BINS:
        raise L.DicowError(f"tensor_stats: bins {bins} outside 0 .. {MAX_BINS} (DICOW_STATS_MAX_BINS)")
    if not 0 <= int(column) <= 3:
        raise L.DicowError(f"tensor_stats: column {column} outside 0..3 (p, g, m, v)")
    if not tensors:
        return TensorStats(torch.empty(0, dtype=torch.uint8), 0, bins, [])
    tab = _table(tensors, int(column))
    device = tensors[0].device
    need = ops.tensor_stats_ws_bytes(tab.n_tensors, tab.n_chunks, bins)
    if need and (tab.ws is None or tab.ws.numel() < need):
        tab.ws = torch.empty(need, dtype=torch.uint8, device=device)
    nrec = tab.n_tensors * REC_DT.itemsize
    out = torch.empty(nrec + tab.n_tensors * bins * 8, dtype=torch.uint8, device=device)
    hist = out[nrec:].view(torch.int64) if bins else None
    with torch.cuda.device(device):
        ops.tensor_stats(tab.tensors_ptr, tab.chunks_ptr, tab.n_tensors, tab.n_chunks, tab.first_ptr, int(column), bins, tab.ws, out[:nrec],
                         hist, grid)
    return TensorStats(out, tab.n_tensors, bins, tab.numels)


# ------------------------------------------------------------------------------------------------ records
def _entry(res, i):
    """One tensor of a TensorStats.result() as the sink's value (plain Python numbers and lists)."""
    nf, lo, hi = int(res["n_finite"][i]), float(res["min"][i]), float(res["max"][i])
    s, q = float(res["sum"][i]), float(res["sumsq"][i])
    if nf == 0 or res["hist"].shape[1] == 0:
        counts, edges = [], []
    elif lo == hi:                                                 # wandb's degenerate form: one bin [min, max] holding everything
        counts, edges = [nf], [lo, hi]
    else:
        counts, edges = res["hist"][i].tolist(), res["edges"][i].tolist()
    return {"counts": counts, "edges": edges, "min": lo, "max": hi, "absmax": float(res["absmax"][i]),
            "mean": s / nf if nf else float("nan"), "rms": math.sqrt(q / nf) if nf else float("nan"), "norm": math.sqrt(q),
            "n_nan": int(res["n_nan"][i]), "n_posinf": int(res["n_posinf"][i]), "n_neginf": int(res["n_neginf"][i]),
            "n_zero": int(res["n_zero"][i]), "numel": int(res["numel"][i])}


def as_wandb(record):
    """{key: (counts_list, edges_list)} for every ``gradients/`` / ``parameters/`` key of a sink record that has a finite element: the
    argument of ``wandb.Histogram(np_histogram=...)``.  wandb's hook logs nothing for a tensor without finite values; neither does this."""
    return {k: (list(v["counts"]), list(v["edges"])) for k, v in record.items() if isinstance(v, dict) and v["counts"]}


def jsonl_sink(path):
    """A sink that appends one JSON line per record to ``path`` (opened at the first record)."""
    state = {}

    def sink(record):
        if "f" not in state:
            state["f"] = open(path, "a")
        state["f"].write(json.dumps(record) + "\n")
        state["f"].flush()
    return sink


class GradWatch:
    """``wandb.watch(model, log=..., log_freq=...)`` on the multi-tensor kernels.  ``model_or_named_parameters``: a module, or an iterable
    of (name, parameter).  ``collect(step)`` launches the passes and starts the download for ``parameters/<name>`` (every parameter) and
    ``gradients/<name>`` (every parameter with ``requires_grad and grad is not None``), then hands the PREVIOUS collection to ``sink``;
    ``flush()`` hands over the last one.  ``sink`` receives ``{"step": k, "gradients/<name>": {...}, "parameters/<name>": {...}}`` with,
    per tensor, counts, edges, min, max, absmax, mean, rms, norm, n_nan, n_posinf, n_neginf, n_zero, numel (mean / rms / norm derived
    from the double sum / sum of squares over the finite elements).  Default sink: ``jsonl_sink("watch_grads.jsonl")``."""

    def __init__(self, model_or_named_parameters, log_freq=50, bins=64, log="all", sink=None):
        if log not in ("all", "gradients", "parameters"):
            raise ValueError(f"GradWatch: log must be 'all', 'gradients' or 'parameters', got {log!r}")
        if int(log_freq) < 1:
            raise ValueError(f"GradWatch: log_freq {log_freq} must be at least 1")
        if not 1 <= int(bins) <= MAX_BINS:
            raise ValueError(f"GradWatch: bins {bins} outside 1 .. {MAX_BINS}")
        self._source = model_or_named_parameters
        if not hasattr(model_or_named_parameters, "named_parameters"):
            self._source = list(model_or_named_parameters)
        self.log_freq, self.bins, self.log = int(log_freq), int(bins), log
        self.sink = jsonl_sink("watch_grads.jsonl") if sink is None else sink
        self._pending = None

    def _named(self):
        return list(self._source.named_parameters()) if hasattr(self._source, "named_parameters") else self._source

    def due(self, step):
        return int(step) % self.log_freq == 0

    def collect(self, step):
        named = self._named()
        parts = []
        if self.log in ("all", "gradients"):
            sel = [(n, p.grad) for n, p in named if p.requires_grad and p.grad is not None]
            if sel:
                parts.append(("gradients/", [n for n, _ in sel], tensor_stats([g.detach() for _, g in sel], self.bins).download()))
        if self.log in ("all", "parameters"):
            if named:
                parts.append(("parameters/", [n for n, _ in named], tensor_stats([p.detach() for _, p in named], self.bins).download()))
        previous, self._pending = self._pending, (int(step), parts)
        self._emit(previous)

    def flush(self):
        previous, self._pending = self._pending, None
        self._emit(previous)

    def _emit(self, pending):
        if pending is None:
            return
        step, parts = pending
        record = {"step": step}
        for prefix, names, stats in parts:
            res = stats.result()
            for i, n in enumerate(names):
                record[prefix + n] = _entry(res, i)
        self.sink(record)


_CALLBACK_CLASS = None


def WatchCallback(watch):
    """A ``transformers.TrainerCallback`` around a ``GradWatch`` (the replacement for the reference's ``GradLogger``): on the main
    process it collects in ``on_pre_optimizer_step`` -- the accumulated, already clipped gradient the optimizer is about to see and the
    parameters before that update -- at every ``log_freq``-th optimizer step, and flushes in ``on_train_end``."""
    global _CALLBACK_CLASS
    if _CALLBACK_CLASS is None:
        from transformers import TrainerCallback

        class _WatchCallback(TrainerCallback):
            def __init__(self, watch):
                self.watch = watch

            def on_pre_optimizer_step(self, args, state, control, **kwargs):
                k = int(state.global_step) + 1                     # the optimizer step about to be taken
                if getattr(state, "is_world_process_zero", True) and self.watch.due(k):
                    self.watch.collect(k)
                return control

            def on_train_end(self, args, state, control, **kwargs):
                if getattr(state, "is_world_process_zero", True):
                    self.watch.flush()
                return control

        _CALLBACK_CLASS = _WatchCallback
    return _CALLBACK_CLASS(watch)

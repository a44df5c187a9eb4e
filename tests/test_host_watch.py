"""CPU tests of the gradient / parameter watch's host side (watch.py, optim.first_chunks, the tensor-statistics entry points of
include/dicow_hip.h): ABI declarations, the chunk ranges of a mixed table, the numpy oracle of tests/tensor_stats_ref.py against CPU
torch.histc, the rendering for wandb, and GradWatch's cadence and one-step-late hand-over with a stub in place of the kernels.
No GPU needed."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests import tensor_stats_ref as R
from tests.util import ROOT

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, optim, watch as W  # noqa: E402


def test_entry_points_are_declared_in_the_stable_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")[0]
    assert re.search(r"^int\s+dicow_tensor_stats_f32\s*\(", stable, flags=re.M)
    assert re.search(r"^int64_t\s+dicow_tensor_stats_ws_bytes\s*\(", stable, flags=re.M)
    m = re.search(r"^#define\s+DICOW_STATS_MAX_BINS\s+(\d+)", stable, flags=re.M)
    assert m and int(m.group(1)) == _lib.STATS_MAX_BINS == W.MAX_BINS == 128
    assert re.search(r"^#define\s+DICOW_ABI_VERSION\s+7\s*$", hdr, flags=re.M)
    assert {"dicow_tensor_stats_f32", "dicow_tensor_stats_ws_bytes"} <= set(_lib.declared_symbols())
    assert "dicow_tensor_stats_f32" in _lib._SIGS and "dicow_tensor_stats_ws_bytes" in _lib._SIGS64
    lib = _lib.lib()
    assert lib.dicow_tensor_stats_f32.restype is _lib.c_i and lib.dicow_tensor_stats_ws_bytes.restype is _lib.c_i64
    assert lib.dicow_abi_version() == 7                                   # additive: the version stays
    for name in ("tensor_stats", "TensorStats", "GradWatch", "WatchCallback", "as_wandb", "jsonl_sink"):
        assert getattr(pkg, name) is getattr(W, name) and name in pkg.__all__


def test_the_record_is_64_bytes_with_the_headers_field_order():
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*dicow_tensor_stats_rec;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[ty]) for n in names.split(",")]

    class Rec(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(Rec) == 64 == _lib.STATS_REC_BYTES == W.REC_DT.itemsize
    for name, _ in fields:
        assert getattr(Rec, name).offset == W.REC_DT.fields[name][1], name


def test_ws_bytes_is_zero_for_an_empty_call_and_grows_with_the_chunks():
    from ts_asr_whisper_amd import ops
    assert ops.tensor_stats_ws_bytes(0, 0, 64) == 0
    sizes = [ops.tensor_stats_ws_bytes(10, n, 64) for n in (1, 100, 10_000, 1_000_000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert ops.tensor_stats_ws_bytes(3, 0, 64) == 0                      # only empty tensors: no chunk, no workspace


def test_first_chunks_of_a_mixed_list():
    C = optim.CHUNK
    numels = [5, 0, C, C + 1, 0, 3 * C, (1 << 31) + 7, 1]
    first = optim.first_chunks(numels)
    assert first.dtype == np.int64 and first.shape == (len(numels) + 1,)
    big = ((1 << 31) + 7 + C - 1) // C
    assert first.tolist() == [0, 1, 1, 2, 4, 4, 7, 7 + big, 8 + big]
    tensors, chunks = optim.build_table(np.zeros((len(numels), 4), np.uint64), numels)     # table only: nothing is allocated
    assert len(chunks) == first[-1]
    for i, n in enumerate(numels):
        mine = chunks[first[i]:first[i + 1]]
        assert (mine["tensor"] == i).all() and int(mine["len"].astype(np.int64).sum()) == n
        assert (mine["start"] == np.arange(len(mine), dtype=np.int64) * C).all()
    assert int(chunks[first[7] - 1]["start"]) + int(chunks[first[7] - 1]["len"]) == (1 << 31) + 7      # int64 starts past 2^31
    assert optim.first_chunks([]).tolist() == [0]


def _histc(x, bins):
    x = np.asarray(x, np.float32)
    f = x[np.isfinite(x)]
    return torch.histc(torch.from_numpy(f), bins=bins, min=float(f.min()), max=float(f.max())).numpy().astype(np.int64)


@pytest.mark.parametrize("bins", [64, 30, 7, 128])
def test_the_oracle_equals_cpu_histc_on_dyadic_inputs(bins):
    rng = np.random.default_rng(bins)
    for n in (3, 65, 2049, 70_001):
        x = (rng.integers(-1024, 1025, n) / 1024.0).astype(np.float32)
        for divide_first in (False, True):                              # both orders are exact on dyadic data
            assert (R.stats_ref(x, bins, divide_first)["hist"] == _histc(x, bins)).all(), (n, divide_first)


@pytest.mark.parametrize("bins", [64, 30, 7, 128])
def test_the_oracle_equals_cpu_histc_one_ulp_around_every_edge(bins):
    for mn, mx in ((-1.0, 1.0), (-0.37, 2.9), (1e-3, 1.7e-3), (-3.0e4, 11.0)):
        x = R.edge_probe_values(np.float32(mn), np.float32(mx), bins)
        assert (R.stats_ref(x, bins)["hist"] == _histc(x, bins)).all(), (mn, mx)


def test_the_oracles_degenerate_cases():
    r = R.stats_ref(np.full(5000, 0.25, np.float32), 64)
    assert r["min"] == r["max"] == 0.25 and r["hist"][0] == 5000 and r["hist"].sum() == 5000 and r["sum"] == 1250.0
    r = R.stats_ref(np.zeros(0, np.float32), 64)
    assert r["min"] == np.inf and r["max"] == -np.inf and r["absmax"] == 0 and r["hist"].sum() == 0 and r["numel"] == 0
    r = R.stats_ref(np.asarray([np.nan, np.inf, -np.inf, np.nan], np.float32), 30)
    assert (r["n_nan"], r["n_posinf"], r["n_neginf"], r["n_finite"], r["n_zero"]) == (2, 1, 1, 0, 0)
    assert r["min"] == np.inf and r["max"] == -np.inf and r["absmax"] == 0 and r["hist"].sum() == 0 and r["sum"] == 0.0
    r = R.stats_ref(np.asarray([0.0, -0.0, 0.0], np.float32), 7)
    assert r["n_zero"] == 3 and r["hist"].tolist() == [3, 0, 0, 0, 0, 0, 0]
    big = np.asarray([-3e38, 0.0, 3e38], np.float32)                     # max - min overflows fp32: the rule on halves
    r = R.stats_ref(big, 4)
    assert r["hist"].sum() == 3 and r["hist"][0] == 1 and r["hist"][3] >= 1
    r = R.stats_ref(np.asarray([1.0, np.nan, 3.0], np.float32), 2)
    assert r["hist"].tolist() == [1, 1] and r["sum"] == 4.0 and r["sumsq"] == 10.0 and r["n_nan"] == 1


class _StubStats:
    """What watch.tensor_stats returns, computed by the oracle on the host."""
    log = []

    def __init__(self, tensors, bins):
        self.tensors, self.bins, self.downloaded = [t.detach().clone() for t in tensors], bins, False
        _StubStats.log.append(self)

    def download(self):
        self.downloaded = True
        return self

    def result(self):
        assert self.downloaded
        refs = [R.stats_ref(t.numpy(), self.bins) for t in self.tensors]
        res = {k: np.asarray([r[k] for r in refs]) for k in ("sum", "sumsq", "min", "max", "absmax", "n_nan", "n_posinf", "n_neginf",
                                                                "n_zero", "numel", "n_finite")}
        res["hist"] = np.stack([r["hist"] for r in refs]) if refs else np.zeros((0, self.bins), np.int64)
        res["edges"] = [W.linspace_edges(r["min"], r["max"], self.bins) if r["n_finite"] else np.zeros(0, np.float32) for r in refs]
        return res


@pytest.fixture
def stub(monkeypatch):
    _StubStats.log = []
    monkeypatch.setattr(W, "tensor_stats", lambda tensors, bins=64: _StubStats(tensors, bins))
    return _StubStats


def _toy():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    m[1].bias.requires_grad_(False)
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.randn_like(p)
    m[0].bias.grad = None
    return m


def test_gradwatch_hands_a_collection_over_one_collection_late(stub):
    m, got = _toy(), []
    w = W.GradWatch(m, log_freq=3, bins=8, sink=got.append)
    assert [k for k in range(1, 10) if w.due(k)] == [3, 6, 9]
    w.collect(3)
    assert got == [] and len(stub.log) == 2 and all(s.downloaded for s in stub.log)      # launched and downloading, nothing handed over
    with torch.no_grad():
        m[0].weight.add_(1.0)
    w.collect(6)
    assert [r["step"] for r in got] == [3]
    w.flush()
    assert [r["step"] for r in got] == [3, 6]
    w.flush()
    assert len(got) == 2                                                  # nothing pending: flush hands nothing over
    rec = got[0]
    assert set(rec) == {"step", "gradients/0.weight", "gradients/1.weight", "parameters/0.weight", "parameters/0.bias",
                        "parameters/1.weight", "parameters/1.bias"}      # no gradient: frozen (1.bias) or grad None (0.bias)
    e = rec["gradients/0.weight"]
    assert set(e) == {"counts", "edges", "min", "max", "absmax", "mean", "rms", "norm", "n_nan", "n_posinf", "n_neginf", "n_zero", "numel"}
    g = m[0].weight.grad.double()
    assert e["numel"] == 12 and len(e["counts"]) == 8 and len(e["edges"]) == 9 and sum(e["counts"]) == 12
    assert e["mean"] == pytest.approx(float(g.mean()), rel=1e-12) and e["norm"] == pytest.approx(float(g.norm()), rel=1e-12)
    assert e["rms"] == pytest.approx(float(g.pow(2).mean().sqrt()), rel=1e-12)
    assert e["edges"] == torch.linspace(e["min"], e["max"], 9).tolist()
    assert got[1]["parameters/0.weight"]["mean"] == pytest.approx(rec["parameters/0.weight"]["mean"] + 1.0, rel=1e-6)
    json.dumps(rec)                                                       # plain numbers and lists


def test_gradwatch_log_selects_the_families(stub):
    m = _toy()
    for log, fam in (("gradients", {"gradients"}), ("parameters", {"parameters"}), ("all", {"gradients", "parameters"})):
        got = []
        w = W.GradWatch(list(m.named_parameters()), log_freq=1, log=log, sink=got.append)
        w.collect(1)
        w.flush()
        assert {k.split("/")[0] for k in got[0] if k != "step"} == fam
    with pytest.raises(ValueError):
        W.GradWatch(m, log="everything")
    with pytest.raises(ValueError):
        W.GradWatch(m, bins=129)
    with pytest.raises(ValueError):
        W.GradWatch(m, log_freq=0)


def test_as_wandb_shapes_and_the_degenerate_rendering(stub):
    named = [("const", torch.nn.Parameter(torch.full((7,), 0.5))), ("nan", torch.nn.Parameter(torch.full((3,), float("nan")))),
             ("ramp", torch.nn.Parameter(torch.arange(10.0))), ("empty", torch.nn.Parameter(torch.zeros(0)))]
    got = []
    w = W.GradWatch(named, log_freq=1, bins=5, log="parameters", sink=got.append)
    w.collect(1)
    w.flush()
    rec = got[0]
    assert rec["parameters/const"]["counts"] == [7] and rec["parameters/const"]["edges"] == [0.5, 0.5]      # wandb: one bin [min, max]
    assert rec["parameters/nan"]["counts"] == [] and rec["parameters/nan"]["n_nan"] == 3
    wb = W.as_wandb(rec)
    assert set(wb) == {"parameters/const", "parameters/ramp"}            # wandb logs nothing for a tensor without finite values
    counts, edges = wb["parameters/ramp"]
    assert isinstance(counts, list) and isinstance(edges, list) and len(counts) == 5 and len(edges) == 6 and counts == [2, 2, 2, 2, 2]
    assert wb["parameters/const"] == ([7], [0.5, 0.5])
    hist = np.histogram(np.arange(10.0), bins=np.asarray(edges))          # the pair is a valid np_histogram
    assert hist[0].tolist() == counts


def test_jsonl_sink_appends_one_line_per_record(tmp_path):
    path = tmp_path / "w.jsonl"
    sink = W.jsonl_sink(str(path))
    assert not path.exists()
    sink({"step": 1, "parameters/a": {"counts": [1], "edges": [0.0, 0.0]}})
    sink({"step": 2})
    assert [json.loads(line)["step"] for line in path.read_text().splitlines()] == [1, 2]


def test_trainstep_and_tensor_stats_signatures():
    from ts_asr_whisper_amd.trainer import TrainStep
    sig = inspect.signature(TrainStep.__init__)
    assert "watch" in sig.parameters and sig.parameters["watch"].default is None
    sig = inspect.signature(W.tensor_stats)
    assert list(sig.parameters)[:2] == ["tensors", "bins"] and sig.parameters["bins"].default == 64
    assert inspect.signature(W.GradWatch.__init__).parameters["log_freq"].default == 50


def test_tensor_stats_refuses_cpu_and_bf16_tensors_without_a_gpu():
    with pytest.raises(_lib.DicowError, match="GPU"):
        W.tensor_stats([torch.zeros(4)])
    with pytest.raises(_lib.DicowError, match="bins 129"):
        W.tensor_stats([torch.zeros(4)], bins=129)
    assert W.tensor_stats([]).result()["hist"].shape == (0, 64)


def test_watch_callback_is_a_trainer_callback(stub):
    from transformers import TrainerCallback, TrainerControl, TrainerState
    m, got = _toy(), []
    cb = W.WatchCallback(W.GradWatch(m, log_freq=2, bins=4, sink=got.append))
    assert isinstance(cb, TrainerCallback) and hasattr(TrainerCallback, "on_pre_optimizer_step")
    state, control = TrainerState(), TrainerControl()
    for k in range(5):                                                    # optimizer steps 1..5
        state.global_step = k
        cb.on_pre_optimizer_step(None, state, control)
    assert [r["step"] for r in got] == [2]                                # step 4 is pending
    cb.on_train_end(None, state, control)
    assert [r["step"] for r in got] == [2, 4]

"""The gradient / parameter watch on the GPU (csrc/tensor_stats.hip, watch.py; the reference's `watch_grads`, src/utils/trainers.py:19-28):
records and histograms EQUAL the numpy oracle of tests/tensor_stats_ref.py on exact (dyadic) data for every grid, bin count and table
column, the counts EQUAL device torch.histc, the refusals, TrainStep(watch=...) on the eager and the graph path and in the preheat
phase, and the HF callback.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import tensor_stats_ref as R

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib, ops, optim, watch as W  # noqa: E402

SIZES = [0, 1, 3, 5, 63, 64, 65, 2047, 2048, 2049, 4097, 3 * 2048 + 1, 70_001, 300_000]
OFFSET_VIEW = SIZES.index(70_001)            # this one is an offset view: 4-byte aligned only
BINS = [64, 30, 1, 128, 0]


def _host_tensors():
    """name -> fp32 numpy vector.  Every finite value is dyadic with a small exponent range per tensor: sums and sums of squares are
    exact in double whatever the order."""
    rng = np.random.default_rng(7)
    out = {}
    for n in SIZES:
        out[f"dyadic{n}"] = (rng.integers(-1024, 1025, n) / 1024.0).astype(np.float32)
    out["constant"] = np.full(5000, -0.375, np.float32)
    out["all_nan"] = np.full(3000, np.nan, np.float32)
    mixed = (rng.integers(-1024, 1025, 4097) / 1024.0).astype(np.float32)
    mixed[::7], mixed[3::11], mixed[5::13] = np.nan, np.inf, -np.inf
    mixed[-1] = np.inf                                                   # (in the count % 4 tail)
    out["mixed_nonfinite"] = mixed
    zeros = np.zeros(2049, np.float32)
    zeros[::2] = -0.0
    out["signed_zeros"] = zeros
    ends = (rng.integers(-512, 513, 3 * 2048 + 1) / 1024.0).astype(np.float32)
    ends[0], ends[-1] = -1.0, 1.0                                        # the minimum only first, the maximum only last
    out["extremes_at_the_ends"] = ends
    out["denormals"] = (rng.integers(-4000, 4001, 2500).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    span = (rng.integers(-1023, 1024, 4100).astype(np.float64) * 2.0 ** 118).astype(np.float32)      # |x| up to 3.4e38: max - min overflows
    span[17], span[4000] = np.float32(-1023 * 2.0 ** 118), np.float32(1023 * 2.0 ** 118)
    out["span_3e38"] = span
    central = np.zeros(300_000, np.float32)                              # one central bin holds all but the two extremes: a lane's 16-bit
    central[0], central[-1] = -1.0, 1.0                                  # column takes every increment and must be flushed on the way
    out["one_central_bin"] = central
    assert np.isfinite(out["span_3e38"]).all() and (out["denormals"] != 0).any() and np.abs(out["denormals"]).max() < 1.2e-38
    return out


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    host = _host_tensors()
    names = list(host)
    dev = []
    for i, k in enumerate(names):
        if i == OFFSET_VIEW:
            backing = torch.zeros(host[k].size + 1, device="cuda")
            t = backing[1:]
            t.copy_(torch.from_numpy(host[k]))
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = torch.from_numpy(host[k]).cuda()
        dev.append(t)
    return {"names": names, "host": host, "dev": dev, "ref": {}}


def _ref(data, bins):
    if bins not in data["ref"]:
        data["ref"][bins] = [R.stats_ref(data["host"][k], bins) for k in data["names"]]
    return data["ref"][bins]


def _raw(stats):
    """The device bytes of a TensorStats: records and histograms, for bit comparisons."""
    return stats.records.cpu().numpy().copy(), (stats.hist.cpu().numpy().copy() if stats.bins else None)


def _check_against_ref(res, refs, names, bins):
    for i, (k, r) in enumerate(zip(names, refs)):
        for f in ("n_nan", "n_posinf", "n_neginf", "n_zero", "numel", "n_finite"):
            assert int(res[f][i]) == r[f], (k, f, int(res[f][i]), r[f])
        for f in ("min", "max", "absmax", "sum", "sumsq"):
            assert res[f][i] == r[f], (k, f, res[f][i], r[f])
        if bins:
            assert (res["hist"][i] == r["hist"]).all(), (k, res["hist"][i].tolist(), r["hist"].tolist())
            assert int(res["hist"][i].sum()) == r["n_finite"], k


@pytest.mark.parametrize("column", [0, 1])
@pytest.mark.parametrize("bins", BINS)
def test_records_and_histograms_equal_the_oracle_for_every_grid(data, bins, column):
    refs = _ref(data, bins)
    raws = []
    for grid in (1, 3, 0, 0):                                            # forced, forced, default, default again
        st = W.tensor_stats(data["dev"], bins, column=column, grid=grid)
        res = st.result()
        _check_against_ref(res, refs, data["names"], bins)
        raws.append(_raw(st))
    for rec, hist in raws[1:]:                                           # bit-equal across the grids and across two runs
        assert (rec == raws[0][0]).all()
        assert bins == 0 or (hist == raws[0][1]).all()
    if bins:
        assert res["hist"].shape == (len(data["names"]), bins) and len(res["edges"]) == len(data["names"])
        i = data["names"].index("dyadic2049")
        assert (res["edges"][i] == torch.linspace(float(res["min"][i]), float(res["max"][i]), bins + 1).numpy()).all()
        assert res["edges"][data["names"].index("all_nan")].size == 0


@pytest.mark.parametrize("bins", [64, 30, 128])
def test_counts_equal_device_histc_on_dyadic_tensors(data, bins):
    res = W.tensor_stats(data["dev"], bins).result()
    n = 0
    for i, k in enumerate(data["names"]):
        if not k.startswith("dyadic") or not res["min"][i] < res["max"][i]:
            continue
        x = data["dev"][i]
        hc = torch.histc(x[torch.isfinite(x)], bins=bins, min=float(res["min"][i]), max=float(res["max"][i])).cpu().numpy().astype(np.int64)
        assert (res["hist"][i] == hc).all(), (k, res["hist"][i].tolist(), hc.tolist())
        n += 1
    assert n >= len(SIZES) - 3


def test_random_normal_data_counts_equal_the_oracle_and_sums_are_within_double_accumulation():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 300_000
    x = torch.randn(n, generator=torch.Generator().manual_seed(3))
    res = W.tensor_stats([x.cuda()], 64).result()
    r = R.stats_ref(x.numpy(), 64)
    assert (res["hist"][0] == r["hist"]).all() and res["min"][0] == r["min"] and res["max"][0] == r["max"]
    d = x.numpy().astype(np.float64)
    exact_s, exact_q = float(np.sum(d)), float(np.sum(d * d))
    bound_s, bound_q = n * 2.0 ** -52 * float(np.abs(d).sum()), n * 2.0 ** -52 * float((d * d).sum())
    print(f"sum {res['sum'][0]!r} vs {exact_s!r} (bound {bound_s:.3e}); sumsq {res['sumsq'][0]!r} vs {exact_q!r} (bound {bound_q:.3e})")
    assert abs(res["sum"][0] - exact_s) <= bound_s and abs(res["sumsq"][0] - exact_q) <= bound_q


def test_refusals_name_the_cause_and_launch_nothing(data):
    ts = data["dev"][3:6]
    with pytest.raises(_lib.DicowError, match="bins 129"):
        W.tensor_stats(ts, 129)
    with pytest.raises(_lib.DicowError, match="column 4"):
        W.tensor_stats(ts, 64, column=4)
    with pytest.raises(_lib.DicowError, match="float32"):
        W.tensor_stats([torch.zeros(8, device="cuda", dtype=torch.bfloat16)])
    with pytest.raises(_lib.DicowError, match="GPU"):
        W.tensor_stats([torch.zeros(8)])
    with pytest.raises(_lib.DicowError, match="contiguous"):
        W.tensor_stats([torch.zeros(8, 8, device="cuda").t()])
    # the C entry itself: the table of three small tensors, a sentinel in the outputs that must survive
    numels = [t.numel() for t in ts]
    tab = W._StatsTable([t.data_ptr() for t in ts], numels, 0, ts[0].device)
    need = ops.tensor_stats_ws_bytes(3, tab.n_chunks, 64)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((3 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    hist = torch.full((3 * 64,), -7, dtype=torch.int64, device="cuda")
    args = (tab.tensors_ptr, tab.chunks_ptr, 3, tab.n_chunks, tab.first_ptr)
    with pytest.raises(_lib.DicowError, match="bins 129"):
        ops.tensor_stats(*args, 0, 129, ws, out, torch.empty(3 * 129, dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.DicowError, match="which 4"):
        ops.tensor_stats(*args, 4, 64, ws, out, hist)
    with pytest.raises(_lib.DicowError, match=f"workspace of {need} bytes"):
        ops.tensor_stats(*args, 0, 64, ws[:need - 16], out, hist)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((hist == -7).all())
    ops.tensor_stats(*args, 0, 64, ws, out, hist)                          # (the same arguments, valid: the sentinel goes)
    assert int(hist.view(3, 64).sum()) == sum(numels)
    # nothing to do is valid: no tensor, or only empty ones
    assert W.tensor_stats([]).result()["hist"].shape == (0, 64)
    res = W.tensor_stats([torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda")], 30).result()
    assert res["min"].tolist() == [np.inf, np.inf] and res["max"].tolist() == [-np.inf, -np.inf] and int(res["hist"].sum()) == 0


# ------------------------------------------------------------------------------------------------ TrainStep
def _train(watch_on, graph, n_preheat, steps=2):
    from ts_asr_whisper_amd.trainer import TrainStep
    from ts_asr_whisper_amd.data import synthetic_batch
    cfg = pkg.DiCoWConfig.preset("whisper-tiny", use_fddt=True, fddt_is_diagonal=True, use_pre_pos_fddt=True,
                                 fddt_init="suppressive", non_target_fddt_value=0.5)
    torch.manual_seed(0)
    model = pkg.DiCoWForConditionalGeneration(cfg).cuda()
    model.tie_weights()
    got = []
    watch = W.GradWatch(model, log_freq=1, bins=64, sink=got.append) if watch_on else None
    ts = TrainStep(model, lr=1e-4, fddt_lr_multiplier=10.0, weight_decay=0.01, max_grad_norm=1.0, use_fddt_only_n_steps=n_preheat,
                   graph=graph, watch=watch)
    batches = [synthetic_batch(cfg, 2, 12, seed=90 + i) for i in range(steps)]
    losses, copies, gnorm_sq = [], [], []
    for k in range(steps):
        losses.append(ts.step(batches[k]).clone())
        if watch_on:
            copies.append(({n: p.grad.detach().cpu().numpy().reshape(-1) for n, p in model.named_parameters()
                            if p.requires_grad and p.grad is not None},
                           {n: p.detach().cpu().numpy().reshape(-1) for n, p in model.named_parameters()}))
            gnorm_sq.append(float(ts.opt.gnorm_sq))
            assert [r["step"] for r in got] == list(range(1, k + 1))       # handed over one step late
    if watch_on:
        watch.flush()
    return dict(losses=torch.stack(losses).cpu(), params=ts.store.params.detach().cpu(), got=got, copies=copies, gnorm_sq=gnorm_sq, ts=ts,
                model=model)


def _check_records(run, preheat):
    assert [r["step"] for r in run["got"]] == [1, 2]
    for rec, (grads, params), gsq in zip(run["got"], run["copies"], run["gnorm_sq"]):
        assert set(rec) == {"step"} | {"gradients/" + n for n in grads} | {"parameters/" + n for n in params}
        assert grads and len(grads) < len(params)                          # the frozen decoder has parameters/ keys only
        if preheat:
            assert all("fddt" in n for n in grads)
        else:
            assert any("layers.0.fc1" in n for n in grads)
        total = 0.0
        for prefix, host in (("gradients/", grads), ("parameters/", params)):
            for n, x in host.items():
                e, r = rec[prefix + n], R.stats_ref(x, 64)
                for f in ("min", "max", "absmax", "n_nan", "n_posinf", "n_neginf", "n_zero", "numel"):
                    assert e[f] == r[f], (prefix + n, f, e[f], r[f])
                if r["min"] == r["max"]:
                    assert e["counts"] == [r["n_finite"]] and e["edges"] == [float(r["min"]), float(r["max"])]
                else:
                    assert e["counts"] == r["hist"].tolist(), prefix + n
                    assert e["edges"] == torch.linspace(float(r["min"]), float(r["max"]), 65).tolist()
                # sum / sumsq: both are double accumulations of the same fp32 values in different orders
                nf = r["n_finite"]
                # (+ 4: e["norm"] is a rounded square root, squared again here)
                assert abs(e["norm"] ** 2 - r["sumsq"]) <= (nf + 4) * 2.0 ** -52 * r["sumsq"], prefix + n
                assert abs(e["mean"] * nf - r["sum"]) <= nf * 2.0 ** -52 * float(np.abs(x.astype(np.float64)).sum()) + 1e-300, prefix + n
                if prefix == "gradients/":
                    total += e["norm"] ** 2
        print(f"step {rec['step']}: sqrt(sum of sumsq) {total ** 0.5!r} vs sqrt(gnorm_sq) {gsq ** 0.5!r}")
        assert abs(total ** 0.5 - gsq ** 0.5) <= 1e-5 * gsq ** 0.5


@pytest.mark.parametrize("graph", [False, True])
def test_trainstep_watch_records_equal_the_oracle_and_change_nothing(graph):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    plain, watched = _train(False, graph, 0), _train(True, graph, 0)
    if graph:
        assert len(watched["ts"]._graphs) == 1                             # step 2 was captured and replayed; the watch is outside it
    assert torch.equal(plain["losses"], watched["losses"]) and torch.equal(plain["params"], watched["params"])
    _check_records(watched, preheat=False)


def test_trainstep_watch_in_the_preheat_phase_has_gradients_of_the_preheat_parameters_only():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    plain, watched = _train(False, False, 5), _train(True, False, 5)
    assert watched["ts"].warmup_phase
    assert torch.equal(plain["losses"], watched["losses"]) and torch.equal(plain["params"], watched["params"])
    _check_records(watched, preheat=True)
    pre = {n for n, p in watched["model"].named_parameters() if p.requires_grad}
    assert {k[len("gradients/"):] for k in watched["got"][0] if k.startswith("gradients/")} == pre


def test_watch_callback_by_hand_with_dicow_adamw():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import TrainerControl, TrainerState
    torch.manual_seed(1)
    m = torch.nn.Sequential(torch.nn.Linear(37, 65), torch.nn.Linear(65, 3)).cuda()
    opt = optim.DiCoWAdamW(m.parameters(), lr=1e-2)
    got = []
    cb = W.WatchCallback(W.GradWatch(m, log_freq=2, bins=30, sink=got.append))
    state, control = TrainerState(), TrainerControl()
    x = torch.randn(16, 37, device="cuda")
    seen = {}
    for k in range(5):                                                   # optimizer steps 1..5
        opt.zero_grad(set_to_none=False)
        m(x).square().mean().backward()
        state.global_step = k
        cb.on_pre_optimizer_step(None, state, control)
        if (k + 1) % 2 == 0:
            seen[k + 1] = {n: (p.grad.detach().cpu().numpy().reshape(-1), p.detach().cpu().numpy().reshape(-1)) for n, p in m.named_parameters()}
        opt.step()
    assert [r["step"] for r in got] == [2]                               # step 4 is still pending
    cb.on_train_end(None, state, control)
    assert [r["step"] for r in got] == [2, 4]
    for rec in got:
        for n, (g, p) in seen[rec["step"]].items():
            for key, x_ in (("gradients/" + n, g), ("parameters/" + n, p)):
                r = R.stats_ref(x_, 30)
                assert rec[key]["counts"] == r["hist"].tolist() and rec[key]["min"] == r["min"] and rec[key]["max"] == r["max"], key
                assert rec[key]["n_zero"] == r["n_zero"] and rec[key]["numel"] == r["numel"]

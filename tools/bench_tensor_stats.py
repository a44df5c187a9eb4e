"""The gradient / parameter watch on the headline tensor list (whisper-large-v3-turbo, decoder frozen: the trainable tensors by shape
from DiCoWConfig.preset, built on the meta device; real buffers with random values, no forward pass), gradients plus parameters:
  (a) watch.tensor_stats: device ms from events around the two calls (gradients, parameters), once with 64 bins and once with
      bins = 0 (pass A + B alone: the difference is the histogram pass), and the wall ms of GradWatch.collect + the hand-over;
  (b) the torch formulation per tensor on the same device -- what wandb's hook runs: isfinite().all(), min().item(), max().item(),
      histc(64, min, max).cpu(), linspace edges -- wall ms (it synchronises per tensor);
  (c) dicow_multi_sumsq_f32 over the same two tables: a pure read pass at this access pattern.  The watch reads the data twice, so
      2 x (c) in the same process on the same board is its floor; reported: (a) / (2 c).
(a) and (c) run in one child process, (b) in another, each under its own `timeout`; the parent never opens the GPU.
  python tools/bench_tensor_stats.py [--steps 20 --warmup 3]
  python tools/bench_tensor_stats.py --edge-probe     which order of the bin formula does torch.histc evaluate on this device?
The probe bins, for several ranges and bin counts, the fp32 values one ulp on either side of every linspace edge: device torch.histc
against (x - min) * bins / (max - min) and (x - min) / (max - min) * bins (fp32 numpy) and against the kernel."""
import argparse, json, math, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBE_RANGES = ((-1.0, 1.0), (-0.37, 2.9), (1e-3, 1.7e-3), (-3.0e4, 11.0), (-2.5e-6, 3.1e-6), (0.1, 0.7))
PROBE_BINS = (64, 30, 7, 128)


def headline_shapes(pkg, torch):
    from ts_asr_whisper_amd.trainer import freeze_by_keyword
    cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo")
    with torch.device("meta"):
        meta = pkg.DiCoWForConditionalGeneration(cfg)
    freeze_by_keyword(meta, ("decoder",))
    return [(n, tuple(p.shape)) for n, p in meta.named_parameters() if p.requires_grad]


def _timed(torch, fn, steps, warmup):
    dev, wall = [], []
    for r in range(warmup + steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r >= warmup:
            dev.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return round(statistics.median(dev), 3), round(statistics.median(wall), 3)


def _setup():
    import torch
    import amd_pkg
    pkg = amd_pkg.load()
    named = headline_shapes(pkg, torch)
    gen = torch.Generator(device="cuda").manual_seed(0)
    ps = [torch.nn.Parameter(torch.empty(s, device="cuda").normal_(0, 0.02, generator=gen)) for _, s in named]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
    return torch, pkg, named, ps


def run_ours(a):
    torch, pkg, named, ps = _setup()
    import numpy as np
    from ts_asr_whisper_amd import ops, optim, watch
    N = sum(math.prod(s) for _, s in named)
    grads, params = [p.grad for p in ps], [p.detach() for p in ps]
    out = {"variant": "ours", "tensors": 2 * len(named), "elements": 2 * N, "device": torch.cuda.get_device_name()}
    out["stats_hist64"] = _timed(torch, lambda: (watch.tensor_stats(grads, 64), watch.tensor_stats(params, 64)), a.steps, a.warmup)
    out["stats_bins0"] = _timed(torch, lambda: (watch.tensor_stats(grads, 0), watch.tensor_stats(params, 0)), a.steps, a.warmup)
    got = []
    w = watch.GradWatch(list(zip([n for n, _ in named], ps)), log_freq=1, sink=got.append)

    def collect_and_result():
        w.collect(1)
        w.flush()
    out["collect_plus_result"] = _timed(torch, collect_and_result, a.steps, a.warmup)
    tabs = []
    for ts, col in ((grads, 1), (params, 1)):
        ptrs = np.zeros((len(ts), 4), np.uint64)
        ptrs[:, col] = [t.data_ptr() for t in ts]
        tabs.append(optim._DeviceTable().upload(*optim.build_table(ptrs, [t.numel() for t in ts]), ts[0].device))
    res = torch.empty(3, device="cuda")

    def sumsq():
        for t in tabs:
            ops.multi_sumsq(t.tensors_ptr, t.chunks_ptr, t.n_chunks, optim._sumsq_ws(t.n_chunks, res.device), res, 1.0)
    out["multi_sumsq"] = _timed(torch, sumsq, a.steps, a.warmup)
    a_ms, a0_ms, c_ms = out["stats_hist64"][0], out["stats_bins0"][0], out["multi_sumsq"][0]
    out["a_over_2c"] = round(a_ms / (2 * c_ms), 3)
    out["passAB_over_c"] = round(a0_ms / c_ms, 3)
    out["passC_over_c"] = round((a_ms - a0_ms) / c_ms, 3)
    out["GBps_hist64"] = round(2 * 2 * N * 4 / a_ms / 1e6, 1)
    out["keys_in_record"] = len(got[-1]) - 1
    print(json.dumps(out), flush=True)


def run_torch(a):
    torch, pkg, named, ps = _setup()

    def wandb_sequence():
        n = 0
        for p in ps:
            for t in (p.grad, p.detach()):
                flat = t.reshape(-1)
                if not torch.isfinite(flat).all():
                    flat = flat[torch.isfinite(flat)]
                tmin, tmax = flat.min().item(), flat.max().item()
                h = torch.histc(flat, bins=64, min=tmin, max=tmax).cpu()
                torch.linspace(tmin, tmax, 65)
                n += int(h.numel())
        return n
    dev, wall = _timed(torch, wandb_sequence, max(2, a.steps // 4), 1)
    print(json.dumps({"variant": "torch_per_tensor", "tensors": 2 * len(named), "device_ms": dev, "wall_ms": wall}), flush=True)


def run_probe(a):
    import numpy as np
    import torch
    import amd_pkg
    amd_pkg.load()
    from ts_asr_whisper_amd import watch
    F = np.float32
    rows, tensors, meta = [], [], []
    for mn, mx in PROBE_RANGES:
        for bins in PROBE_BINS:
            e = torch.linspace(mn, mx, bins + 1, dtype=torch.float32).numpy()
            v = np.concatenate([e, np.nextafter(e, F(-np.inf)), np.nextafter(e, F(np.inf))]).astype(F)
            v = np.unique(v[(v >= e[0]) & (v <= e[-1])])
            meta.append((mn, mx, bins, v))
    per_bins = {}
    for mn, mx, bins, v in meta:
        per_bins.setdefault(bins, []).append(torch.from_numpy(v).cuda())
    kernel = {bins: watch.tensor_stats(ts, bins).result()["hist"] for bins, ts in per_bins.items()}
    seen = {b: 0 for b in per_bins}
    n_mul = n_div = n_ker = 0
    for mn, mx, bins, v in meta:
        lo, hi = v.min(), v.max()
        x = torch.from_numpy(v).cuda()
        hc = torch.histc(x, bins=bins, min=float(lo), max=float(hi)).cpu().numpy().astype(np.int64)
        w = F(hi - lo)
        idx = {"mul_first": ((v - lo) * F(bins)) / w, "div_first": ((v - lo) / w) * F(bins)}
        eq = {}
        for k, q in idx.items():
            b = np.minimum(q.astype(np.int64), bins - 1)
            eq[k] = bool((np.bincount(b, minlength=bins) == hc).all())
        ker = kernel[bins][seen[bins]]
        seen[bins] += 1
        eq["kernel"] = bool((ker == hc).all())
        n_mul += eq["mul_first"]; n_div += eq["div_first"]; n_ker += eq["kernel"]
        rows.append({"min": float(lo), "max": float(hi), "bins": bins, "values": int(v.size), **eq})
        print(json.dumps(rows[-1]), flush=True)
    n = len(rows)
    verdict = ("both orders equal device torch.histc on the probe set: the rule stays multiply-then-divide" if n_mul == n and n_div == n else
               "only multiply-then-divide equals device torch.histc: it is the rule" if n_mul == n else
               "only divide-then-multiply equals device torch.histc: it becomes the rule" if n_div == n else
               "neither order equals device torch.histc everywhere: the rule stays multiply-then-divide")
    print(json.dumps({"variant": "edge_probe", "cases": n, "mul_first_equal": n_mul, "div_first_equal": n_div, "kernel_equal": n_ker,
                      "device": torch.cuda.get_device_name(), "torch": torch.__version__, "verdict": verdict}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--edge-probe", action="store_true")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", default="", choices=("", "ours", "torch", "probe"))
    a = ap.parse_args()
    if a.child:
        {"ours": run_ours, "torch": run_torch, "probe": run_probe}[a.child](a)
        return 0
    for child in (("probe",) if a.edge_probe else ("ours", "torch")):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", child, "--steps", str(a.steps),
               "--warmup", str(a.warmup)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                                   # a fault, an abort or the time limit: nothing more is started
            print(f"bench_tensor_stats: child '{child}' ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""One optimizer step on the headline parameter list (whisper-large-v3-turbo, decoder frozen: 743 tensors, 637,296,640 elements, shapes
and the reference's two groups from the model built on the meta device; real buffers on the GPU, random gradients).  All variants run
interleaved in one process, one step each per round:
  torch_foreach_clip  torch.optim.AdamW (default foreach) + torch.nn.utils.clip_grad_norm_
  torch_fused_clip    torch.optim.AdamW(fused=True) + torch.nn.utils.clip_grad_norm_ (if this torch build constructs it)
  flat_adamw          the existing dicow_adamw_f32 on ONE flat buffer of the same element count (update only: the floor)
  dicow_update        DiCoWAdamW, no clip (update only: compare with flat_adamw)
  dicow_clip          optim.clip_grad_norm_ + DiCoWAdamW
  dicow_fused_clip    DiCoWAdamW(max_grad_norm=1.0)
Reported per variant: device ms per step (events around the step, median over the timed rounds), effective TB/s from the bytes the
shapes imply (AdamW 28 B/element: read p g m v, write p m v; clip +4 B/element for the norm, +8 B/element to rescale g in place) and
host ms until the step returns.   python tools/bench_optimizer.py [--steps 30 --warmup 5]"""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import amd_pkg

pkg = amd_pkg.load()
from ts_asr_whisper_amd import ops
from ts_asr_whisper_amd.optim import DiCoWAdamW, clip_grad_norm_
from ts_asr_whisper_amd.trainer import freeze_by_keyword

PRE = ("model.encoder.fddts", "model.encoder.initial_fddt")


def headline_shapes():
    cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo")
    with torch.device("meta"):
        meta = pkg.DiCoWForConditionalGeneration(cfg)
    freeze_by_keyword(meta, ("decoder",))
    return [(n, tuple(p.shape)) for n, p in meta.named_parameters() if p.requires_grad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    named = headline_shapes()
    N = sum(math.prod(s) for _, s in named)
    gen = torch.Generator(device="cuda").manual_seed(0)
    ps = [torch.nn.Parameter(torch.empty(s, device="cuda").normal_(0, 0.02, generator=gen)) for _, s in named]
    grads = [torch.randn(s, device="cuda", generator=gen) for _, s in named]
    for p, g in zip(ps, grads):
        p.grad = g
    groups = lambda: [{"params": [p for (n, _), p in zip(named, ps) if not n.startswith(PRE)]},
                      {"params": [p for (n, _), p in zip(named, ps) if n.startswith(PRE)], "lr": 2e-4, "weight_decay": 0.0}]
    LR, WD = 2e-6, 0.0
    variants = {}
    opt1 = torch.optim.AdamW(groups(), lr=LR, weight_decay=WD)
    variants["torch_foreach_clip"] = (lambda: (torch.nn.utils.clip_grad_norm_(ps, 1.0), opt1.step()), 40)
    try:
        opt2 = torch.optim.AdamW(groups(), lr=LR, weight_decay=WD, fused=True)
        variants["torch_fused_clip"] = (lambda: (torch.nn.utils.clip_grad_norm_(ps, 1.0), opt2.step()), 40)
    except Exception as e:                                           # (recorded, not fatal)
        print("torch fused AdamW unavailable:", repr(e))
    flat = [torch.randn(N, device="cuda", generator=gen) * s for s in (0.02, 1.0, 0.0, 0.0)]
    fstep = [0]

    def flat_step():
        fstep[0] += 1
        ops.adamw(flat[0], flat[1], flat[2], flat[3], LR, 0.9, 0.999, 1e-8, WD, fstep[0])
    variants["flat_adamw"] = (flat_step, 28)
    opt4 = DiCoWAdamW(groups(), lr=LR, weight_decay=WD)
    variants["dicow_update"] = (lambda: opt4.step(), 28)
    opt5 = DiCoWAdamW(groups(), lr=LR, weight_decay=WD)
    variants["dicow_clip"] = (lambda: (clip_grad_norm_(ps, 1.0), opt5.step()), 40)
    opt6 = DiCoWAdamW(groups(), lr=LR, weight_decay=WD, max_grad_norm=1.0)
    variants["dicow_fused_clip"] = (lambda: opt6.step(), 32)
    if a.only:
        variants = {k: v for k, v in variants.items() if k in a.only.split(",")}
    print(f"tensors {len(named)} elements {N} torch {torch.__version__} device {torch.cuda.get_device_name()}")
    rec = {k: [] for k in variants}
    for r in range(a.warmup + a.steps):
        for k, (fn, _) in variants.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            if r >= a.warmup:
                rec[k].append((e0, e1, (t1 - t0) * 1e3))
    torch.cuda.synchronize()
    out = {}
    for k, (_, bpe) in variants.items():
        dev = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in rec[k])
        host = statistics.median(h for _, _, h in rec[k])
        out[k] = {"device_ms": round(dev, 3), "host_ms": round(host, 3), "bytes_per_elem": bpe, "eff_TBps": round(bpe * N / dev / 1e9, 2)}
        print(f"{k:20s} device {dev:8.3f} ms   {bpe} B/elem -> {bpe * N / dev / 1e9:5.2f} TB/s   host {host:7.3f} ms")
    if "flat_adamw" in out and "dicow_update" in out:
        out["dicow_update_over_flat"] = round(out["dicow_update"]["device_ms"] / out["flat_adamw"]["device_ms"], 3)
    if "torch_foreach_clip" in out and "dicow_clip" in out:
        out["torch_foreach_clip_over_dicow_clip"] = round(out["torch_foreach_clip"]["device_ms"] / out["dicow_clip"]["device_ms"], 3)
    print(json.dumps({"tensors": len(named), "elements": N, "steps": a.steps, "variants": out}))


if __name__ == "__main__":
    main()

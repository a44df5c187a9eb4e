"""LoRA on the decoder, measured: the three dicow_lora_* kernels at the whisper-large-v3-turbo decoder shapes beside a torch copy_ that
moves the same number of bytes, and the headline TrainStep (B = 16, L = 128: bench.py's workload) in three states of the SAME tree in ONE
process -- decoder frozen (the yardstick), decoder frozen with rank-16 adapters, decoder fully trainable.  Interleaved rounds, medians.
   python tools/bench_lora.py [--out table.txt]      (REPS rounds, default 3; STEPS per step measurement, default 3; ENC_MODEL, ENC_BATCH;
   SKIP_STEP=1 / SKIP_KERNELS=1 leave a part out; LIMIT seconds per measured block, default 120: a block that runs longer ends the run)"""
import os, signal, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import ops
from ts_asr_whisper_amd.trainer import TrainStep
from ts_asr_whisper_amd.data import synthetic_batch

BF16, F32 = torch.bfloat16, torch.float32
reps, steps, limit = int(os.environ.get("REPS", "3")), int(os.environ.get("STEPS", "3")), int(os.environ.get("LIMIT", "120"))
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def _too_long(*_):
    raise SystemExit(f"bench_lora: a measured block ran longer than {limit} s -- stopping, nothing else is started")


signal.signal(signal.SIGALRM, _too_long)


def timed(fn, n, warm=1):
    signal.alarm(limit)
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    signal.alarm(0)
    return e0.elapsed_time(e1) / n


# ------------------------------------------------------------------------------------------------ kernels
def kernel_problems():
    """(label, bytes moved, launch) per kernel and shape.  Bytes: every operand once, outputs once (in place: read + write), wgrad's
    fp32 partials written and read once."""
    r, dev, probs = 16, "cuda", []
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, device=dev, generator=g) * 0.1).to(dtype)

    shapes = [(16 * 128, w, 1, "rows 16x128") for w in (1280, 5120)] + [(16 * 445, w, 1, "rows 16x445") for w in (1280, 5120)]
    shapes += [(16 * 128, 1280, 3, "rows 16x128 q/k/v"), (16 * 445, 1280, 3, "rows 16x445 q/k/v"), (16 * 1500, 1280, 2, "rows 16x1500 cross k/v")]
    for M, W, nseg, what in shapes:
        R = r * nseg
        x, A, Bt, t = rnd(M, W), rnd(R, W), rnd(R, W), rnd(M, R)
        y, y32, gA = rnd(M, nseg * W), rnd(M, W, dtype=F32), [torch.zeros(r, W, device=dev) for _ in range(nseg)]
        gB = [torch.zeros(W, r, device=dev) for _ in range(nseg)]
        tag = f"{what:24s} K=N={W:4d} R={R:2d}"
        probs.append((f"down  dense  {tag}", 2 * (M * W + R * W + M * R), lambda x=x, A=A, t=t: ops.lora_down(x, A, t, r)))
        probs.append((f"down  block  {tag}", 2 * (M * nseg * W + R * W + M * R), lambda y=y, Bt=Bt, t=t: ops.lora_down(y, Bt, t, r, block=True)))
        probs.append((f"up    block  {tag} bf16", 2 * (2 * M * nseg * W + R * W + M * R),
                      lambda y=y, Bt=Bt, t=t, n=nseg: ops.lora_up(t, Bt, y, y, r, [2.0] * n, block=True)))
        probs.append((f"up    dense  {tag} bf16", 2 * (2 * M * W + R * W + M * R), lambda x=x, A=A, t=t: ops.lora_up(t, A, x, x, r, [2.0])))
        if nseg == 1:
            probs.append((f"up    block  {tag} fp32", 8 * M * W + 2 * (R * W + M * R), lambda y=y32, Bt=Bt, t=t: ops.lora_up(t, Bt, y, y, r, [2.0], block=True)))
            probs.append((f"up    gelu   {tag} bf16", 2 * (3 * M * W + R * W + M * R),
                          lambda x=x, A=A, t=t, u=torch.empty_like(x): ops.lora_up(t, A, x, x, r, [2.0], block=True, gelu=True, aux=u)))
        else:
            probs.append((f"up    dense  {tag} fp32", 8 * M * W + 2 * (R * W + M * R), lambda y=y32, A=A, t=t: ops.lora_up(t, A, y, y, r, [2.0])))
        nsplit = max(1, min(32, -(-M // 256)))
        probs.append((f"wgrad dense  {tag} dA", 2 * (M * W + M * R) + 4 * R * W * (2 * nsplit + 2),
                      lambda x=x, t=t, gA=gA: ops.lora_wgrad(t, x, gA, r, 2.0, g_rs=W)))
        probs.append((f"wgrad block  {tag} dB", 2 * (M * nseg * W + M * R) + 4 * R * W * (2 * nsplit + 2),
                      lambda y=y, t=t, gB=gB: ops.lora_wgrad(t, y, gB, r, 2.0, block=True, g_rs=1, g_cs=r)))
    return probs


def bench_kernels():
    probs = kernel_problems()
    res = {p[0]: ([], []) for p in probs}
    copies = {}
    for rnd_ in range(reps):
        for label, nbytes, fn in probs:
            if nbytes not in copies:                  # a copy_ that moves nbytes in all: nbytes / 2 read, nbytes / 2 written
                copies[nbytes] = (torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"))
            a, b = copies[nbytes]
            res[label][0].append(timed(lambda i: fn(), 20, warm=3))
            res[label][1].append(timed(lambda i: b.copy_(a), 20, warm=3))
    say(f"{'kernel / mode / shape':62s} {'MB':>8s} {'us':>8s} {'GB/s':>8s} | copy_ {'us':>7s} {'GB/s':>8s} | kernel/copy")
    for label, nbytes, _ in probs:
        k, c = statistics.median(res[label][0]) * 1e3, statistics.median(res[label][1]) * 1e3
        say(f"{label:62s} {nbytes / 1e6:8.2f} {k:8.1f} {nbytes / k / 1e3:8.0f} |       {c:7.1f} {nbytes / c / 1e3:8.0f} | {k / c:6.2f}x")


# ------------------------------------------------------------------------------------------------ the training step
def bench_step():
    cfg = pkg.DiCoWConfig.preset(os.environ.get("ENC_MODEL", "whisper-large-v3-turbo"), use_fddt=True, fddt_is_diagonal=True,
                                 use_pre_pos_fddt=True, fddt_init="suppressive", non_target_fddt_value=0.5)
    B = int(os.environ.get("ENC_BATCH", "16"))
    batches = [synthetic_batch(cfg, B, 128, seed=1000 + i) for i in range(2)]
    states = {}
    for name in ("decoder frozen", "frozen + LoRA r=16", "decoder trainable"):
        torch.manual_seed(0)
        model = pkg.DiCoWForConditionalGeneration(cfg).cuda()
        model.tie_weights()
        if "LoRA" in name:
            pkg.add_decoder_lora(model)
            g = torch.Generator(device="cuda").manual_seed(1)
            with torch.no_grad():                     # a trained adapter: B is not zero
                for n, p in model.named_parameters():
                    if "lora_B" in n:
                        p.copy_(torch.randn(p.shape, device="cuda", generator=g) * 0.01)
        states[name] = TrainStep(model, lr=2e-6, fddt_lr_multiplier=100.0, max_grad_norm=1.0, warmup_steps=2000, max_steps=40000,
                                 frozen_keywords=() if name == "decoder trainable" else ("decoder",),
                                 preheat_prefixes=("model.encoder.fddts", "model.encoder.initial_fddt"), use_fddt_only_n_steps=0)
    res = {k: [] for k in states}
    for rnd_ in range(reps):
        for name, ts in states.items():
            res[name].append(timed(lambda i: ts.step(batches[i % 2]), steps, warm=2 if rnd_ == 0 else 1))
    base = statistics.median(res["decoder frozen"])
    say(f"TrainStep, {os.environ.get('ENC_MODEL', 'whisper-large-v3-turbo')}, B = {B}, L = 128, ms per step ({reps} interleaved rounds of {steps} steps)")
    for name, ts in states.items():
        n_tr = sum(p.numel() for p in ts.model.parameters() if p.requires_grad)
        m = statistics.median(res[name])
        say(f"  {name:20s} " + " ".join(f"{x:7.2f}" for x in res[name]) + f"   median {m:7.2f}  ({m / base:5.3f} x frozen)   trainable {n_tr / 1e6:7.1f} M")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}")
    if os.environ.get("SKIP_KERNELS") != "1":
        bench_kernels()
        say()
    if os.environ.get("SKIP_STEP") != "1":
        bench_step()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

"""The HF-shaped training step at the headline configuration (whisper-large-v3-turbo dims, decoder frozen, B = 16, L = 128 labels):
torch.autocast(bf16) -> loss.backward() -> clip at 1.0 -> optimizer.step() -> zero_grad(), the order HF's Trainer runs them in.
Two arms on two copies of the model, interleaved step by step in one process:
  torch  torch.optim.AdamW (the reference's two groups, default foreach) + torch.nn.utils.clip_grad_norm_
  dicow  optim.dicow_optimizer (DiCoWAdamW, the same groups) + optim.clip_grad_norm_
Device ms per whole step (events), median over the timed steps, and the optimizer + clip part alone.
    python tools/hf_step_time.py [--steps 10 --warmup 3]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import amd_pkg

pkg = amd_pkg.load()
from ts_asr_whisper_amd.data import synthetic_batch
from ts_asr_whisper_amd.optim import clip_grad_norm_, dicow_optimizer
from ts_asr_whisper_amd.trainer import freeze_by_keyword

PRE = ("model.encoder.fddts", "model.encoder.initial_fddt")
LR = 2e-6


def torch_optimizer(model):
    named = list(model.named_parameters())
    base = [p for n, p in named if not n.startswith(PRE)]
    new = [p for n, p in named if n.startswith(PRE)]
    return torch.optim.AdamW([{"params": base}, {"params": new, "lr": 100.0 * LR, "weight_decay": 0.0}], lr=LR, weight_decay=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo", use_fddt=True, fddt_is_diagonal=True, use_pre_pos_fddt=True,
                                 fddt_init="suppressive", non_target_fddt_value=0.5)
    arms = {}
    for name, make_opt, clip in (("torch", torch_optimizer, torch.nn.utils.clip_grad_norm_),
                                 ("dicow", lambda m: dicow_optimizer(m, LR), clip_grad_norm_)):
        torch.manual_seed(0)
        model = pkg.DiCoWForConditionalGeneration(cfg).cuda()
        model.tie_weights()
        freeze_by_keyword(model, ("decoder",))
        arms[name] = (model, make_opt(model), clip)
    batches = [synthetic_batch(cfg, a.batch, 128, seed=1000 + i) for i in range(2)]
    rec = {k: [] for k in arms}
    for i in range(a.warmup + a.steps):
        for name, (model, opt, clip) in arms.items():
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model(**batches[i % 2]).loss
            loss.backward()
            ev[1].record()
            clip(model.parameters(), 1.0)
            opt.step()
            opt.zero_grad()
            ev[2].record()
            if i >= a.warmup:
                rec[name].append(ev)
    torch.cuda.synchronize()
    out = {}
    for name in arms:
        step = statistics.median(e[0].elapsed_time(e[2]) for e in rec[name])
        optm = statistics.median(e[1].elapsed_time(e[2]) for e in rec[name])
        out[name] = {"step_ms": round(step, 2), "clip_opt_zero_grad_ms": round(optm, 2)}
        print(f"{name:6s} step {step:8.2f} ms   clip + step + zero_grad {optm:7.2f} ms")
    print(json.dumps({"batch": a.batch, "steps": a.steps, "arms": out}))


if __name__ == "__main__":
    main()

"""The sampling launch (dicow_sample_tokens) at whisper-large-v3-turbo's vocabulary, one GPU, one process.

  1. The launch alone on [16, V] and [80, V] fp32 scores -- warpers off, top_k = 50, top_p = 0.9, each plan -- against the torch
     formulation of the same step on the same device: `/ t`, topk + masked_fill, sort + softmax + cumsum + scatter, softmax,
     multinomial, log_softmax + gather, where / != on the flags.  Back-to-back calls between two device events, host wrapper
     included: launch rates, not kernel durations; --rounds repeats of --calls calls each, medians and spreads.
  2. The device memory a 16-window, 200-token sampling decode holds at the model's real dims: generate(return_scores=True) -- what the
     fallback ladder kept for its log-probability test -- against generate(return_logprobs=True).
--out FILE keeps the report; --notes FILE appends the lines of that file (the test module's figures, the compile log's spill count)."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
import amd_pkg

pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib
from ts_asr_whisper_amd.data import synthetic_batch
from ts_asr_whisper_amd.generation import GreedyDecoder, sample_tokens

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--skip-memory", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--notes", default=None)
args = ap.parse_args()

V, T = 51866, 0.7


def timed(fn, n):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def torch_step(sc, flags, top_k, top_p, eos, pad):
    """The step's tail as torch ops, HF's warpers included; returns (tokens, log-probabilities, flags)."""
    x = sc / T
    if top_k:
        x = x.masked_fill(x < torch.topk(x, top_k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        srt, idx = torch.sort(x, descending=False)
        cum = srt.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[..., -1:] = False
        x = x.masked_fill(remove.scatter(1, idx, remove), -float("inf"))
    nxt = torch.multinomial(torch.softmax(x, dim=-1), 1)[:, 0]
    lp = torch.log_softmax(x * T, dim=-1).gather(1, nxt[:, None])[:, 0]
    nxt = torch.where(flags, nxt, torch.full_like(nxt, pad))
    return nxt, lp, flags & (nxt != eos)


lines = [f"tools/bench_sampling.py: V = {V}, temperature {T}; {args.rounds} rounds of {args.calls} back-to-back calls, host side included"]
for rows in (16, 80):
    sc = torch.randn(rows, V, device="cuda") * 3.0
    flags = torch.ones(rows, dtype=torch.bool, device="cuda")
    out, lp = torch.empty(rows, dtype=torch.long, device="cuda"), torch.empty(rows, device="cuda")
    for name, k, p in (("warpers off", 0, 1.0), ("top_k = 50", 50, 1.0), ("top_p = 0.9", 0, 0.9)):
        t = {}
        for plan_name, plan in (("reg", _lib.SAMPLE_REG), ("stream", _lib.SAMPLE_STREAM)):
            fl = flags.clone()
            t[plan_name] = [timed(lambda: sample_tokens(sc, T, k, p, 0.0, seed=1, step=3, unfinished=fl, eos_token_id=-1, out=out,
                                                        logprob=lp, plan=plan), args.calls) for _ in range(args.rounds)]
        t["torch"] = [timed(lambda: torch_step(sc, flags, k, p, -1, 0), max(args.calls // 4, 10)) for _ in range(args.rounds)]
        fmt = lambda v: f"{statistics.median(v):.1f} us (spread {min(v):.1f} .. {max(v):.1f})"  # noqa: E731
        lines.append(f"scores [{rows}, {V}], {name}: register plan {fmt(t['reg'])}, streaming plan {fmt(t['stream'])}, torch formulation "
                     f"{fmt(t['torch'])} per step")

if not args.skip_memory:
    B, N = 16, 200
    cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo", use_fddt=True, fddt_is_diagonal=True, use_pre_pos_fddt=True,
                                 fddt_init="suppressive", non_target_fddt_value=0.5)
    torch.manual_seed(0)
    model = pkg.DiCoWForConditionalGeneration(cfg).cuda().eval()
    model.tie_weights()
    b = synthetic_batch(cfg, B, 8, seed=1)
    prompt = torch.tensor([[50258, 50259, 50360]] * B)
    dec = GreedyDecoder(model)
    kw = dict(eos_token_id=50257, pad_token_id=50257, suppress_tokens=[50257], temperature=T)   # (eos suppressed: all 200 positions)
    for name, extra in (("return_scores (torch tail)", dict(return_scores=True)), ("return_logprobs (one launch)", dict(return_logprobs=True, top_k=50, seed=1))):
        dec.generate(b["input_features"], b["stno_mask"], prompt, 4, **kw, **extra)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = dec.generate(b["input_features"], b["stno_mask"], prompt, N, **kw, **extra)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        lines.append(f"{B} windows x {res[0].shape[1] - 3} tokens, {name}: peak device memory above the model {(peak - base) / 2 ** 20:.1f} MiB; "
                     f"the returned tensor holds {res[1].numel() * 4 / 2 ** 20:.1f} MiB")
        del res

if args.notes:
    lines += [l.rstrip("\n") for l in open(args.notes)]
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

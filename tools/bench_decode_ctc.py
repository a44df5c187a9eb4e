"""Decoding with the whole processor chain at whisper-large-v3-turbo dims: suppress lists, timestamp rules, joint CTC/attention
scoring (500 candidates, T = 375 CTC frames), B = 16 windows, 60 new tokens.

--repetition: also the A/B of the chain with repetition_penalty / no_repeat_ngram_size off (the chain as above) and on, interleaved
in one process, and the two history kernels alone (repetition rules, timestamp rules) on [B, vocabulary] scores; --out FILE keeps
the report."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import amd_pkg

pkg = amd_pkg.load()
from ts_asr_whisper_amd.data import synthetic_batch
from ts_asr_whisper_amd.generation import GreedyDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--repetition", action="store_true", help="A/B the whole chain with the repetition options off / on")
ap.add_argument("--penalty", type=float, default=1.2)
ap.add_argument("--ngram", type=int, default=3)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, N = 16, 60
cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo", use_fddt=True, fddt_is_diagonal=True, use_pre_pos_fddt=True,
                             fddt_init="suppressive", non_target_fddt_value=0.5, ctc_weight=0.3, pre_ctc_sub_sample=True,
                             additional_self_attention_layer=True)
torch.manual_seed(0)
model = pkg.DiCoWForConditionalGeneration(cfg).cuda().eval()
model.tie_weights()
b = synthetic_batch(cfg, B, 8, seed=1)
prompt = torch.tensor([[50258, 50259, 50360]] * B)
dec = GreedyDecoder(model)
kw = dict(eos_token_id=50257, pad_token_id=50257, suppress_tokens=[1, 2, 7, 8, 9], begin_suppress_tokens=[220, 50257],
          timestamps=dict(no_timestamps_token_id=50364, max_initial_timestamp_index=50),
          ctc=dict(weight=0.3, first_timestamp=50365, upper_cased=[(i, i + 1000) for i in range(300, 400)], prefix_len=3))
dec.generate(b["input_features"], b["stno_mask"], prompt, 4, **kw)
torch.cuda.synchronize()
for name, k in (("greedy", dict(eos_token_id=-1)), ("greedy + timestamp rules + CTC rescoring", kw)):
    t0 = time.perf_counter()
    seq = dec.generate(b["input_features"], b["stno_mask"], prompt, N, **k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    print(f"{name}: B={B}, {seq.shape[1] - 3} new tokens in {dt:.1f} ms ({dt / max(1, seq.shape[1] - 3):.2f} ms per token incl. the encoder)")

if args.repetition:
    from ts_asr_whisper_amd.generation import repetition_rules, timestamp_rules
    rep = dict(repetition_penalty=args.penalty, no_repeat_ngram_size=args.ngram)
    lines = [f"tools/bench_decode_ctc.py --repetition: whisper-large-v3-turbo dims, B={B}, {N} new tokens, suppress lists + timestamp rules + "
             f"CTC rescoring; options on = repetition_penalty {args.penalty}, no_repeat_ngram_size {args.ngram}; {args.rounds} interleaved rounds"]
    dec.generate(b["input_features"], b["stno_mask"], prompt, 4, **kw, **rep)
    torch.cuda.synchronize()
    per_tok = {"off": [], "on": []}
    for r in range(args.rounds):
        for name, extra in (("off", {}), ("on", rep)):
            t0 = time.perf_counter()
            seq = dec.generate(b["input_features"], b["stno_mask"], prompt, N, **kw, **extra)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            per_tok[name].append(dt / max(1, seq.shape[1] - 3))
            lines.append(f"round {r} options {name}: {seq.shape[1] - 3} new tokens in {dt:.1f} ms ({per_tok[name][-1]:.3f} ms per token incl. the encoder)")
    off, on = statistics.median(per_tok["off"]), statistics.median(per_tok["on"])
    lines.append(f"median ms per token: off {off:.3f} (spread {min(per_tok['off']):.3f} .. {max(per_tok['off']):.3f}), "
                 f"on {on:.3f} (spread {min(per_tok['on']):.3f} .. {max(per_tok['on']):.3f}); difference {1e3 * (on - off):+.1f} us per token")
    # the two history kernels alone, device events around 200 launches each
    V, P = cfg.vocab_size, 3
    ids = torch.randint(0, 50257, (B, P + N), device="cuda")
    ids[:, :P] = prompt.cuda()
    sc = torch.randn(B, V, device="cuda")
    work = torch.empty_like(sc)

    def timed(fn, n=200):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    for L_ in (P + 1, P + N, 448):
        h = ids[:, :L_] if L_ <= ids.shape[1] else torch.randint(0, 50257, (B, L_), device="cuda")
        h = h.contiguous()
        t_rep = timed(lambda: repetition_rules(h, work, args.penalty, args.ngram))
        work.copy_(sc)
        t_ts = timed(lambda: timestamp_rules(h, work, P, 50257, 50364, 50))
        work.copy_(sc)
        lines.append(f"kernels alone, history {L_} ids, scores [{B}, {V}]: repetition rules {t_rep:.1f} us per call, "
                     f"timestamp rules {t_ts:.1f} us per call (back-to-back launches incl. the host wrapper)")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

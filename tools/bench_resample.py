"""dicow_resample against the reference's formulation on the same device, one process on one board:   python tools/bench_resample.py [rounds]

Two workloads:
  hour    one hour of 44.1 kHz stereo int16 -> 16 kHz mono fp32 (a meeting recording; `load_recording` without the file read)
  clips   16 clips of 30 s at 48 kHz, mono int16 -> 16 kHz (a directory of noise clips; one launch over 16 segments)
After a warm-up of everything, these alternate for `rounds` (default 20, at least 10) rounds of CALLS back-to-back calls between two device events:
  hip.*      wave_intake.resample into a preallocated output: the one launch plus the wrapper's checks and the table upload
  torch.*    what torchaudio.functional.resample does, on the GPU: int16 -> fp32 / 32768, torch.mean over the channels, F.pad(width,
             width + o), F.conv1d(stride=o) with the full [n, 1, K] bank, transpose, trim.  The hour runs in 60 chunks of one minute
             (torchaudio users chunk too: the padded copy and the [n, J] result of the whole hour are 2 x 230 MB on top of the input)
Reported: median (min .. max) milliseconds per call, the megabytes each call must move at least (the input read once, the output written
once), and max |hip - torch| on the clips and on the hour's first minute (0 where the convolution the library picks happens to add
the products of a phase in ascending order too)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import wave_intake as W

ROUNDS = max(10, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
CALLS = {"hour": 2, "clips": 10}
g = torch.Generator().manual_seed(0)
hour = torch.randint(-20000, 20000, (44100 * 3600, 2), generator=g, dtype=torch.int16).cuda()
clips = torch.randint(-20000, 20000, (16, 48000 * 30, 1), generator=g, dtype=torch.int16).cuda()
plans = {"hour": W.resample_plan(44100, 16000, "cuda"), "clips": W.resample_plan(48000, 16000, "cuda")}
full = {}
for k, (orig, plan) in {"hour": (44100, plans["hour"]), "clips": (48000, plans["clips"])}.items():
    full[k] = torch.from_numpy(W.full_bank64(plan.o, plan.n)[1]).float().cuda()[:, None, :]         # [n, 1, K], rounded once like the plan's
out = {"hour": torch.empty(plans["hour"].out_len(hour.shape[0]), device="cuda"),
       "clips": torch.empty(16, plans["clips"].out_len(clips.shape[1]), device="cuda")}


def torch_resample(x16, k):
    """x16 int16 [B, frames, C] -> fp32 [B, ceil(n frames / o)] as the reference computes it."""
    plan = plans[k]
    x = torch.mean(x16.to(torch.float32) / 32768.0, dim=2)
    y = F.conv1d(F.pad(x[:, None, :], (plan.width, plan.width + plan.o)), full[k], stride=plan.o)    # [B, n, J]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :plan.out_len(x.shape[1])]


def torch_hour():
    minute = 44100 * 60
    return torch.cat([torch_resample(hour[None, m * minute:(m + 1) * minute], "hour")[0] for m in range(60)])


arms = {"hip.hour": lambda: W.resample(hour, 44100, 16000, out=out["hour"]),
        "torch.hour": torch_hour,
        "hip.clips": lambda: W.resample(clips, 48000, 16000, out=out["clips"]),
        "torch.clips": lambda: torch_resample(clips, "clips")}
minute = hour[:44100 * 60]
diffs = {"clips": (arms["hip.clips"]().clone(), arms["torch.clips"]()),
         "hour[:60 s]": (W.resample(minute, 44100, 16000), torch_resample(minute[None], "hour")[0])}
for f in arms.values():
    for _ in range(2):
        f()
torch.cuda.synchronize()
ts = {k: [] for k in arms}
for _ in range(ROUNDS):
    for k, f in arms.items():
        calls = CALLS[k.split(".")[1]]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts[k].append(e0.elapsed_time(e1) / calls)
print(f"tools/bench_resample.py: {ROUNDS} rounds per arm, arms alternating after a warm-up of all; hour = 3600 s x 44.1 kHz stereo int16, "
      f"clips = 16 x 30 s x 48 kHz mono int16, both -> 16 kHz mono fp32")
mb = {"hour": (hour.numel() * 2 + out["hour"].numel() * 4) / 1e6, "clips": (clips.numel() * 2 + out["clips"].numel() * 4) / 1e6}
for k, v in ts.items():
    m = statistics.median(v)
    print(f"{k:12s} median {m:9.3f} ms (min {min(v):.3f}, max {max(v):.3f})   {mb[k.split('.')[1]]:7.1f} MB -> {mb[k.split('.')[1]] / m:7.2f} GB/s")
for w in ("hour", "clips"):
    print(f"hip.{w} / torch.{w} =", round(statistics.median(ts[f"hip.{w}"]) / statistics.median(ts[f"torch.{w}"]), 3))
for w, (a, b) in diffs.items():
    print(f"{w}: max |hip - torch| {float((a - b).abs().max()):.2e}, max |hip| {float(a.abs().max()):.3f}")

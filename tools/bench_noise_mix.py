"""dicow_noise_mix on 16 clips of 30 s against the front end it feeds, one process on one board:   python tools/bench_noise_mix.py [rounds]

After a warm-up of everything, these alternate for `rounds` (default 25, at least 20) rounds of 40 back-to-back calls between two device events:
  mix16 / mix5 / mix1    mix_background_noise in place (out is wave) with 16, 5 and 1 of the 16 rows planned -- the two launches plus the wrapper
                         and the plan upload; rows are 30 s long, crops start at odd offsets of a 40 s clip
  mix16+copy             the out-of-place call (the clone of the batch in front)
  log_mel                features.log_mel (128 mels) on the same batch
Reported: median (min .. max) microseconds per call, the bytes the mix must move at least (audio and noise read once each by either pass, one
write) and the rate that makes, and the shader clock rocm-smi showed while the rounds ran."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import features, wave_augment as WA
from bench import PowerSampler

ROUNDS, CALLS = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 25), 40
B, N = 16, features.N_SAMPLES
g = torch.Generator().manual_seed(0)
wave = (torch.randn(B, N, generator=g) * 0.1).cuda()
bank = WA.NoiseBank.from_tensors([torch.randn(2, 640001, generator=g), torch.randn(1, 640003, generator=g)])


def plan(rows):
    pi = torch.tensor([(r, r % 2, 1001 * r + 1, N) for r in rows], dtype=torch.int32)
    return pi, torch.tensor([10 ** ((r % 16) / 10) for r in rows], dtype=torch.float64).float()


work = wave.clone()
arms = {}
for k, rows in (("mix16", range(16)), ("mix5", (1, 4, 7, 10, 13)), ("mix1", (6,))):
    arms[k] = (lambda p: (lambda: WA.mix_background_noise(work, bank, *p, out=work)))(plan(rows))
arms["mix16+copy"] = (lambda p: (lambda: WA.mix_background_noise(wave, bank, *p)))(plan(range(16)))
arms["log_mel"] = lambda: features.log_mel(wave, 128)
for f in arms.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
ts = {k: [] for k in arms}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for _ in range(ROUNDS):
    for k, f in arms.items():
        work.copy_(wave)                      # (in place every call halves the row: start each round from the same values)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts[k].append(e0.elapsed_time(e1) / CALLS * 1e3)
power = ps.stop()
print(f"tools/bench_noise_mix.py: B={B} x {N} samples, {ROUNDS} rounds of {CALLS} calls per arm, arms alternating after a warm-up of all")
for k, v in ts.items():
    line = f"{k:11s} median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    if k.startswith("mix"):
        rows = 16 if "16" in k else int(k[3:])
        mb = rows * N * 4 * 5 / 1e6 + (2 * B * N * 4 / 1e6 if k == "mix16+copy" else 0.0)        # (the clone: one read, one write of the batch)
        line += f"   {mb:6.1f} MB -> {mb / statistics.median(v):5.2f} TB/s"
    print(line)
print("mix16 / log_mel =", round(statistics.median(ts["mix16"]) / statistics.median(ts["log_mel"]), 3))
print("power / clock:", power if power else "rocm-smi gave no sample")

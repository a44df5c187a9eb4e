"""dicow_enrollment_mix on 16 mixtures of 30 s against the torch ops it replaces, one process on one board:   python tools/bench_enrollment_mix.py [rounds]

After a warm-up of everything, these alternate for `rounds` (default 25, at least 20) rounds of 40 back-to-back calls between two device events:
  mix3 / mix1 / mix8     mix_enrollments into a preallocated [16, 480000] output with 3, 1 and 8 tracks per row -- the one launch plus the
                         wrapper's checks and the plan upload; 3 tracks per row is the recipe's number_of_mixed_speakers = 2
  torch3                 the same 3-track mixtures as torch.zeros + one slice-add per track (49 launches)
  stno16                 enrollment_stno for the 16 rows: per row a table sweep on the host and the two launches of stno_masks
  log_mel                features.log_mel (128 mels) on the mixed batch, the consumer
Reported: median (min .. max) microseconds per call, the bytes the mix must move at least (every covered sample read once, every output
sample written once) and the rate that makes, and the shader clock rocm-smi showed while the rounds ran."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import features, enrollment_mix as EM
from bench import PowerSampler

ROUNDS, CALLS = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 25), 40
B, N = 16, features.N_SAMPLES
g = torch.Generator().manual_seed(0)
lens = [N - 1601 * k for k in range(8)] + [160001 + 16001 * k for k in range(8)]            # 8 long clips, 8 of 10 .. 17 s
bank = EM.EnrollmentBank.from_tensors([torch.randn(n, generator=g) * 0.1 for n in lens], [f"s{k % 8}" for k in range(16)],
                                      [f"r{k}" for k in range(16)])


def plan(per_row):
    """per_row tracks for every row: the first a long clip from an odd offset to the end of the row, the others short clips spread over it."""
    t = []
    for r in range(B):
        off = 1001 * r + 1
        t.append((r, r % 8, off, min(lens[r % 8], N - off)))
        for j in range(1, per_row):
            c = 8 + (r + j) % 8
            o = (j * 7919 * (r + 1)) % (N - lens[c])
            t.append((r, c, o, lens[c]))
    return torch.tensor(t, dtype=torch.int32)


out = torch.empty(B, N, device="cuda")
plans = {k: plan(k) for k in (3, 1, 8)}


def torch_mix(tracks):
    w = torch.zeros(B, N, device="cuda")
    for r, c, o, n in tracks.tolist():
        w[r, o:o + n] += bank.data[bank.starts[c]:bank.starts[c] + n]
    return w


assert torch.equal(torch_mix(plans[3]), EM.mix_enrollments(bank, plans[3], B, N))           # (the slice-adds run in plan order too: the same sums)
targets = [f"s{r % 8}" for r in range(B)]
mix_len = [int((plans[3][plans[3][:, 0] == r][:, 2:].sum(1)).max()) for r in range(B)]
arms = {f"mix{k}": (lambda p: (lambda: EM.mix_enrollments(bank, p, B, N, out=out)))(p) for k, p in plans.items()}
arms["torch3"] = lambda: torch_mix(plans[3])
arms["stno16"] = lambda: EM.enrollment_stno(bank, plans[3], targets, mix_len)
arms["log_mel"] = lambda: features.log_mel(out, 128)
for f in arms.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
ts = {k: [] for k in arms}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for _ in range(ROUNDS):
    for k, f in arms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts[k].append(e0.elapsed_time(e1) / CALLS * 1e3)
power = ps.stop()
print(f"tools/bench_enrollment_mix.py: B={B} x {N} samples, {ROUNDS} rounds of {CALLS} calls per arm, arms alternating after a warm-up of all")
for k, v in ts.items():
    line = f"{k:8s} median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"
    if k.startswith("mix") or k == "torch3":
        p = plans[3 if k == "torch3" else int(k[3:])]
        mb = (int(p[:, 3].sum()) + B * N) * 4 / 1e6
        line += f"   {mb:6.1f} MB -> {mb / statistics.median(v):5.2f} TB/s"
    print(line)
print("mix3 / torch3 =", round(statistics.median(ts["mix3"]) / statistics.median(ts["torch3"]), 3),
      "  mix3 / log_mel =", round(statistics.median(ts["mix3"]) / statistics.median(ts["log_mel"]), 3))
print("power / clock:", power if power else "rocm-smi gave no sample")

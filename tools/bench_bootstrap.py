"""dicow_bootstrap_sums under every plan against a torch formulation on the same device and numpy on the host, one process on one board:
    python tools/bench_bootstrap.py [rounds]

Workloads, R = 100 000 replicates each, resample mode (kernelP) and swap mode (swapP) under every plan:
  session     n = 40 sessions, 4 metrics x 2 systems x (errors, length) = 16 columns: what compare_session_metrics launches
  utterance   n = 20 000 utterances, 4 columns (errors and reference length of two systems): what compare_wer launches
and, for the choice between a lane and a wave per replicate where the table fits LDS, n = 128, 256, 512 at 16 columns and n = 512, 2048
at 4 (`sweep` lines: kernel time only).
Arms, alternating round by round after a warm-up of all:
  kernelP   device events around the entry point alone under plan P (1 LANE_LDS, 2 WAVE_LDS, 3 WAVE_L2; 0 = the library's choice); a plan
            that needs the table in LDS has no row where it does not fit
  hip       significance.bootstrap_sums and the download of the sums: wall clock around a call that ends in the download's synchronise
  torch     the same sums with tensor ops: torch.randint in chunks of at most 2^25 indices, table[idx].sum(1); wall clock to the end of the
            download.  Its draws are torch's own, so only shapes, totals and moments are compared.  Rounds: fewer (it is slow), stated below
  numpy     rng.integers + table[idx].sum(1) on the host for a stated fraction of the replicates, scaled to R
Reported: median (min .. max) per call and draws per second; that every plan gives the same bits at the timed sizes, and that the first 64
replicates equal the oracle of tests/bootstrap_ref.py.  Board power over the timed window from bench.PowerSampler."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, significance as S
from tests import bootstrap_ref as B
from bench import PowerSampler

ROUNDS = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
TORCH_ROUNDS = 3
R = 100_000
SEED = 2026
rng = np.random.default_rng(0)


def workload(n, C):
    length = rng.integers(20, 4000, n) if n <= 1000 else rng.integers(1, 60, n)
    cols = []
    for c in range(C):
        cols.append(length if c % 2 else (length * 0.3 * rng.random(n)).astype(np.int64))
    host = np.ascontiguousarray(np.stack(cols, 1).astype(np.int64))
    return dict(n=n, C=C, host=host, table=torch.from_numpy(host).cuda(), out=torch.empty((R, C), dtype=torch.int64, device="cuda"),
                offs=np.asarray([0, n], np.int64), draws=float(R) * n)


W = {"session": workload(40, 16), "utterance": workload(20000, 4)}
SWEEP = {f"sweep.n{n}.C{C}": workload(n, C) for n, C in ((128, 16), (256, 16), (512, 16), (512, 4), (2048, 4))}


def plans(w):
    return [0] + [p for p in range(1, L.BOOT_PLANS + 1) if p == L.BOOT_WAVE_L2 or w["n"] * w["C"] * 8 <= L.BOOT_LDS_BYTES]


def kernel(w, plan, mode=L.BOOT_RESAMPLE):
    """The entry point alone on the current stream (no check of the bound, no download)."""
    L.call("dicow_bootstrap_sums", w["table"].data_ptr(), w["C"], w["n"], w["C"], w["offs"].ctypes.data, None, 1, R, 0, SEED, mode, plan,
           w["out"].data_ptr(), L.stream())


def hip(w):
    return S.bootstrap_sums(w["table"], R, SEED).cpu()


def torch_sums(w):
    n, table = w["n"], w["table"]
    step = max(1, (1 << 25) // n)
    parts = [table[torch.randint(n, (min(step, R - at), n), device="cuda")].sum(1) for at in range(0, R, step)]
    return torch.cat(parts).cpu()


def numpy_sums(w, reps):
    g = np.random.default_rng(1)
    return w["host"][g.integers(0, w["n"], (reps, w["n"]))].sum(1)


# ---- agreement at the timed sizes, which is the warm-up of every arm too
for k, w in {**W, **SWEEP}.items():
    ref = hip(w)
    assert (ref[:64].numpy() == B.sums_np(w["host"], 64, SEED)).all(), k
    for mode in (L.BOOT_RESAMPLE, L.BOOT_SWAP):
        kernel(w, 0, mode)
        torch.cuda.synchronize()
        first = w["out"].cpu()
        for plan in plans(w)[1:]:
            kernel(w, plan, mode)
            torch.cuda.synchronize()
            assert torch.equal(w["out"].cpu(), first), (k, plan, mode)
        if mode == L.BOOT_RESAMPLE:
            assert torch.equal(first, ref), k
        else:
            assert (first[:16].numpy() == B.sums_np(w["host"], 16, SEED, None, "swap")).all(), k
    print(f"{k}: n = {w['n']}, C = {w['C']}: plans {plans(w)} give the same bits in both modes; the first replicates equal the oracle; the library's "
          f"plan is {L.lib().dicow_bootstrap_plan(w['n'], w['C'])}")
for k, w in W.items():
    t = torch_sums(w).double()
    ours = hip(w).double()
    assert t.shape == ours.shape
    rel = ((t.mean(0) - ours.mean(0)).abs() / ours.std(0)).max().item()                # the two means, in standard deviations of one replicate
    print(f"{k}: torch's own draws: column means within {rel:.4f} standard deviations of a replicate (expected about {R ** -0.5 * 2 ** 0.5:.4f})")
    assert rel < 0.05
torch.cuda.synchronize()

names = [f"{arm}.{k}" for k, w in W.items() for arm in ["hip", "torch"] + [f"kernel{p}" for p in plans(w)] + [f"swap{p}" for p in plans(w)]]
names += [f"kernel{p}.{k}" for k, w in SWEEP.items() for p in plans(w)]
ts = {name: [] for name in names}


def timed_kernel(w, plan, mode=L.BOOT_RESAMPLE):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    kernel(w, plan, mode)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ps = PowerSampler(torch.cuda.current_device())
ps.start()
for rnd in range(ROUNDS):
    for k, w in W.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip(w)
        ts[f"hip.{k}"].append((time.perf_counter() - t0) * 1e3)
        for plan in plans(w):
            ts[f"kernel{plan}.{k}"].append(timed_kernel(w, plan))
        for plan in plans(w):
            ts[f"swap{plan}.{k}"].append(timed_kernel(w, plan, L.BOOT_SWAP))
        if rnd < TORCH_ROUNDS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_sums(w)
            ts[f"torch.{k}"].append((time.perf_counter() - t0) * 1e3)
    for k, w in SWEEP.items():
        for plan in plans(w):
            ts[f"kernel{plan}.{k}"].append(timed_kernel(w, plan))
power = ps.stop()

print(f"tools/bench_bootstrap.py: {ROUNDS} rounds of hip / kernel, {TORCH_ROUNDS} rounds of torch, arms alternating after a warm-up of all; R = {R} "
      f"replicates; kernelN = plan N (1 LANE_LDS, 2 WAVE_LDS, 3 WAVE_L2), kernel0 = the library's choice, swapN = swap mode under plan N")
allw = {**W, **SWEEP}
for name, v in ts.items():
    k = name.split(".", 1)[1]
    m = statistics.median(v)
    print(f"{name:24s} median {m:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {allw[k]['draws'] / m / 1e6:9.3f} G draws / s")
for k in W:
    best = min(plans(W[k])[1:], key=lambda p: statistics.median(ts[f"kernel{p}.{k}"]))
    print(f"{k}: fastest plan {best}; hip.{k} / torch.{k} = {statistics.median(ts[f'hip.{k}']) / statistics.median(ts[f'torch.{k}']):.5f}; "
          f"kernel{best}.{k} / torch.{k} = {statistics.median(ts[f'kernel{best}.{k}']) / statistics.median(ts[f'torch.{k}']):.5f}")
print("board power over the timed window:", power)
for k, reps in (("session", 10_000), ("utterance", 100)):
    numpy_sums(W[k], max(1, reps // 10))
    t0 = time.perf_counter()
    numpy_sums(W[k], reps)
    dt = time.perf_counter() - t0
    print(f"numpy.{k:12s} {dt * 1e3:10.1f} ms for {reps} replicates on the host: x {R // reps} = {dt * R / reps * 1e3:.0f} ms for the workload")

"""dicow_ngram_repeats against a torch formulation on the same device and the plain-Python oracle on the host, one process on one board:
    python tools/bench_ngram_repeats.py [rounds]

Workload: a corpus of 20 000 segments of 30-400 words over a skewed vocabulary of 5000 words (a twentieth of them a second casing of
their neighbour), 2 % of the segments ending in a loop of period 1-6; the reference's default parameters (min_n 1, max_n 10, 30 words,
unigram run 10, more than 10 occurrences).  A second one for the choice of the plan only: 64 segments of 8000 words.
Arms, alternating round by round after a warm-up of all:
  hip       hyp_cleanup.repeating_ngram_cuts and the download of keep and reason: the table upload, the two launches, the copy back -- wall
            clock around a call that ends in the download's synchronise; `kernel`: device events around the entry point alone (table copy +
            two launches), once per plan
  torch     the same keep with tensor ops over the flat buffer: per length n one unfold, one torch.unique(dim=0, return_counts=True) over
            (segment, n words) rows, the counts gathered back, the degenerate windows masked by an unfold of the folded ids, a scatter-min
            per segment; the unigram rule by one more unfold.  Rounds: fewer (it is slow), stated below
  oracle    tests/ngram_repeats_ref.py on the host, what rank 0 does in the reference's evaluation loop (there with ' '.join keys); timed on
            the first 1000 segments and scaled by words to the workload, as stated in its line
Reported: median (min .. max) per call, words per second, and that hip, torch and (on the timed subset) the oracle agree on every keep.
Board power over the timed window from bench.PowerSampler."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, hyp_cleanup, ops
from tests import ngram_repeats_ref as R
from bench import PowerSampler

ROUNDS = max(10, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
TORCH_ROUNDS = 3
P = dict(min_n=1, max_n=10, min_word_threshold=30, unigram_min_repeat=10, repeat_threshold=10)
rng = np.random.default_rng(0)


def segment(W, looping):
    ids = (5000 * rng.random(W) ** 3).astype(np.int32)
    if looping:
        at = int(rng.integers(0, W - 25))
        period = (5000 * rng.random(int(rng.integers(1, 7))) ** 3).astype(np.int32)
        ids[at:] = np.resize(period, W - at)
    return ids


def workload(lens, loop_share):
    segs = [segment(int(W), rng.random() < loop_share) for W in lens]
    flat = np.concatenate(segs).astype(np.int32)
    fold = np.where(flat % 20 == 1, flat - 1, flat).astype(np.int32)
    lens = np.asarray(lens, np.int64)
    table = np.ascontiguousarray(np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]), lens], 1).astype(np.int64))
    return dict(ids=torch.from_numpy(flat).cuda(), fold=torch.from_numpy(fold).cuda(), table=table, flat=flat, hfold=fold, words=float(lens.sum()),
                keep=torch.empty(len(lens), dtype=torch.int32, device="cuda"), reason=torch.empty((len(lens), 3), dtype=torch.int32, device="cuda"))


W = {"corpus": workload(rng.integers(30, 401, 20000), 0.02), "long": workload([8000] * 64, 0.25)}


def hip(w):
    keep, reason = hyp_cleanup.repeating_ngram_cuts(w["ids"], w["fold"], w["table"], **P)
    return keep.cpu(), reason.cpu()


def hip_kernel(w, plan):
    """The entry point alone on the current stream (no download)."""
    t = w["table"]
    nbytes = L.lib().dicow_ngram_repeats_ws_bytes(t.ctypes.data, len(t), plan)
    ws = ops.workspace(nbytes, w["ids"].device)
    L.call("dicow_ngram_repeats", w["ids"].data_ptr(), w["fold"].data_ptr(), w["ids"].numel(), t.ctypes.data, len(t), P["min_n"], P["max_n"],
           P["min_word_threshold"], P["unigram_min_repeat"], P["repeat_threshold"], w["keep"].data_ptr(), w["reason"].data_ptr(), plan, ws.data_ptr(),
           nbytes, L.stream())


def torch_cuts(w):
    dev = w["ids"].device
    ids, fold = w["ids"].long(), w["fold"].long()
    table = torch.from_numpy(w["table"]).to(dev)
    start, lens = table[:, 0], table[:, 1]
    n_seg, total = len(lens), ids.numel()
    seg = torch.repeat_interleave(torch.arange(n_seg, device=dev), lens)                 # the segment of every word
    pos = torch.arange(total, device=dev) - start[seg]                                  # its index in the segment
    keep = lens.clone()
    u, r = P["unigram_min_repeat"], P["repeat_threshold"]

    def windows(n):                                  # which of the total - n + 1 windows of n words lie in one segment
        return seg[:total - n + 1] == seg[n - 1:]

    if P["min_n"] == 1 and total >= u:
        f = fold.unfold(0, u, 1)
        ok = windows(u) & (f == f[:, :1]).all(1)
        keep = keep.scatter_reduce(0, seg[:total - u + 1][ok], pos[:total - u + 1][ok] + 1, "amin")
    for n in range(max(2, P["min_n"]), P["max_n"] + 1):
        if total < n:
            break
        ok = windows(n)
        rows = torch.cat([seg[:total - n + 1, None], ids.unfold(0, n, 1)], 1)[ok]
        _, inverse, counts = torch.unique(rows, dim=0, return_inverse=True, return_counts=True)
        f = fold.unfold(0, n, 1)[ok]
        count = torch.where((f == f[:, :1]).all(1), torch.zeros_like(inverse), counts[inverse])
        hit = count > r
        keep = keep.scatter_reduce(0, seg[:total - n + 1][ok][hit], pos[:total - n + 1][ok][hit] + n, "amin")
    keep = torch.where(lens < P["min_word_threshold"], lens, keep)
    return keep.cpu()


def oracle(w, n_seg):
    out = []
    for s, ln in w["table"][:n_seg].tolist():
        out.append(R.cut(w["flat"][s:s + ln].tolist(), w["hfold"][s:s + ln].tolist(), P["min_n"], P["max_n"], P["min_word_threshold"],
                         P["unigram_min_repeat"], P["repeat_threshold"]))
    return out


# ---- agreement at the timed sizes, which is the warm-up of every arm too
for k, w in W.items():
    keep, reason = hip(w)
    assert torch.equal(keep.long(), torch_cuts(w)), k
    for plan in range(1, L.NGRAM_PLANS + 1):
        hip_kernel(w, plan)
        torch.cuda.synchronize()
        assert torch.equal(w["keep"].cpu(), keep) and torch.equal(w["reason"].cpu(), reason), (k, plan)
    w["cut"] = int((keep.long() < torch.from_numpy(w["table"][:, 1])).sum())
    print(f"{k}: hip == torch on all {len(keep)} segments and every plan gives the same keep and reason; {w['cut']} segments cut, {w['words']:.3e} words")
SUB = 1000
t0 = time.perf_counter()
want = oracle(W["corpus"], SUB)
dt_oracle = time.perf_counter() - t0
keep, reason = hip(W["corpus"])
assert [k for k, _ in want] == keep[:SUB].tolist() and [list(rs) for _, rs in want] == reason[:SUB].tolist()
torch.cuda.synchronize()

ts = {f"{arm}.{k}": [] for k in W for arm in ["hip", "torch"] + [f"kernel{p}" for p in range(0, L.NGRAM_PLANS + 1)]}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for rnd in range(ROUNDS):
    for k, w in W.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip(w)
        ts[f"hip.{k}"].append((time.perf_counter() - t0) * 1e3)
        for plan in range(0, L.NGRAM_PLANS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip_kernel(w, plan)
            e1.record()
            torch.cuda.synchronize()
            ts[f"kernel{plan}.{k}"].append(e0.elapsed_time(e1))
        if rnd < TORCH_ROUNDS:
            t0 = time.perf_counter()
            torch_cuts(w)
            ts[f"torch.{k}"].append((time.perf_counter() - t0) * 1e3)
power = ps.stop()

print(f"tools/bench_ngram_repeats.py: {ROUNDS} rounds of hip / kernel, {TORCH_ROUNDS} rounds of torch, arms alternating after a warm-up of all; corpus = 20 000 "
      f"segments of 30-400 words, 2 % looping; long = 64 segments of 8000 words, a quarter looping; parameters {P}; kernelN = plan N, (R, C) = "
      f"{L.NGRAM_PLAN_TILES}, kernel0 = the library's choice")
for name, v in ts.items():
    k = name.split(".", 1)[1]
    m = statistics.median(v)
    print(f"{name:18s} median {m:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {W[k]['words'] / m / 1e6:9.3f} G words / s")
for k in W:
    print(f"hip.{k} / torch.{k} = {statistics.median(ts[f'hip.{k}']) / statistics.median(ts[f'torch.{k}']):.5f}")
print("board power over the timed window:", power)
sub = float(W["corpus"]["table"][:SUB, 1].sum())
print(f"oracle.corpus      {dt_oracle * 1e3:10.1f} ms for the first {SUB} segments ({sub / dt_oracle / 1e6:.3f} M words / s), equal to hip on each: x "
      f"{W['corpus']['words'] / sub:.1f} = {dt_oracle * W['corpus']['words'] / sub * 1e3:.0f} ms for the workload")

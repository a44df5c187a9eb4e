"""dicow_edit_distance against a torch formulation on the same device and a numpy row-scan on the host, one process on one board:
    python tools/bench_edit_distance.py [rounds]

Two workloads:
  utts      4096 utterance pairs of 20-200 words, the hypothesis a copy of the reference with about 15 % of its words substituted,
            deleted or preceded by an insertion (one evaluation pass of WER; one launch, the narrow workgroup)
  session   one session of 8 x 8 whole-meeting streams of 12 000 words, every hypothesis stream such a copy of one reference stream
            (cpWER: 64 tables of 12 000 x ~12 000 cells; one launch, the wide workgroup), without and with intervals (tcpWER: a word every
            250 ms, the hypothesis as centre points with a collar of 5 s)
Arms, alternating round by round after a warm-up of all:
  hip.*     scoring.edit_counts: the table upload, the one launch, the (errors, hits) download -- wall clock around a call that ends in
            the download's synchronise; and `kernel`, device events around the entry point alone (table copy + kernel)
  torch.*   the same key (errors * 2^32 - hits, int64) swept anti-diagonal by anti-diagonal with tensor ops over the whole batch:
            per diagonal three shifted adds and two minimum, the equality (and overlap) of the diagonal's cells from a flipped copy of the
            hypothesis, and for ragged batches the pick of the pairs that end on this diagonal.  Rounds: fewer (it is slow), stated below
  numpy.*   one row at a time on the host with minimum.accumulate for the insertion chain; timed on a subset (256 utterances, one of the
            64 session tables) and scaled to the workload, as stated in its line
Reported: median (min .. max) per call, cell updates per second (cells = sum of ref_len * hyp_len), and that hip and torch agree on every
pair.  Board power over the timed window from bench.PowerSampler."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, ops, scoring
from bench import PowerSampler

ROUNDS = max(10, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
TORCH_ROUNDS = {"utts": 5, "session": 2, "session+iv": 2}
UNIT = 1 << 32
rng = np.random.default_rng(0)


def noisy_copy(ref, vocab):
    out = []
    for w in ref.tolist():
        u = rng.random()
        if u < 0.05:
            continue
        if u < 0.10:
            out.append(int(rng.integers(0, vocab)))
        out.append(int(rng.integers(0, vocab)) if 0.10 <= u < 0.15 else w)
    return np.array(out, np.int32)


def flat(seqs):
    lens = np.array([len(s) for s in seqs], np.int64)
    return np.concatenate(seqs).astype(np.int32), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens


def workload(refs, hyps, pairs, timed):
    rf, rs, rl = flat(refs)
    hf, hs, hl = flat(hyps)
    w = dict(ref=torch.from_numpy(rf).cuda(), hyp=torch.from_numpy(hf).cuda(), riv=None, hiv=None, refs=refs, hyps=hyps, pairs=pairs,
             table=np.array([(rs[i], rl[i], hs[j], hl[j]) for i, j in pairs], np.int64), cells=float(sum(len(refs[i]) * len(hyps[j]) for i, j in pairs)))
    if timed:                                                            # a word every 250 ms; hypothesis: centre points, collar 5 s
        w["rivs"] = [np.stack([np.arange(len(s)) * 250, np.arange(len(s)) * 250 + 250], 1) for s in refs]
        w["hivs"] = [np.stack([np.arange(len(s)) * 250 + 125 - 5000, np.arange(len(s)) * 250 + 125 + 5000], 1) for s in hyps]
        w["riv"] = torch.from_numpy(np.concatenate(w["rivs"]).astype(np.int32)).cuda()
        w["hiv"] = torch.from_numpy(np.concatenate(w["hivs"]).astype(np.int32)).cuda()
    return w


utt_refs = [rng.integers(0, 5000, int(n)).astype(np.int32) for n in rng.integers(20, 201, 4096)]
utt_hyps = [noisy_copy(r, 5000) for r in utt_refs]
ses_refs = [rng.integers(0, 5000, 12000).astype(np.int32) for _ in range(8)]
ses_hyps = [noisy_copy(r, 5000) for r in ses_refs]
ses_pairs = [(i, j) for i in range(8) for j in range(8)]
W = {"utts": workload(utt_refs, utt_hyps, [(i, i) for i in range(4096)], False),
     "session": workload(ses_refs, ses_hyps, ses_pairs, False),
     "session+iv": workload(ses_refs, ses_hyps, ses_pairs, True)}


def hip(w):
    return scoring.edit_counts(w["ref"], w["hyp"], w["table"], w["riv"], w["hiv"])[:, :2]


def hip_kernel(w):
    """The entry point alone on the current stream (no download)."""
    t = w["table"]
    nbytes = L.lib().dicow_edit_distance_ws_bytes(t.ctypes.data, len(t))
    ws = ops.workspace(nbytes, w["ref"].device)
    L.call("dicow_edit_distance", w["ref"].data_ptr(), w["ref"].numel(), w["hyp"].data_ptr(), w["hyp"].numel(), L.ptr(w["riv"]), L.ptr(w["hiv"]),
           t.ctypes.data, len(t), w["out"].data_ptr(), 0, 0, ws.data_ptr(), nbytes, L.stream())


def torch_sweep(w):
    """Anti-diagonals with tensor ops.  State: the keys of diagonals d - 1 and d - 2 indexed by the row i, [B, N + 1]."""
    dev = w["ref"].device
    pairs, refs, hyps = w["pairs"], w["refs"], w["hyps"]
    B, N, M = len(pairs), max(len(refs[i]) for i, _ in pairs), max(len(hyps[j]) for _, j in pairs)
    r = torch.full((B, N), -1, dtype=torch.int32)
    hflip = torch.full((B, M), -2, dtype=torch.int32)                    # hflip[b, x] = hyp[b, M - 1 - x]; pads never match
    timed = w["riv"] is not None
    if timed:
        rb, re_ = torch.zeros((B, N), dtype=torch.int32), torch.zeros((B, N), dtype=torch.int32)
        hbf, hef = torch.zeros((B, M), dtype=torch.int32), torch.zeros((B, M), dtype=torch.int32)
    for b, (i, j) in enumerate(pairs):
        r[b, :len(refs[i])] = torch.from_numpy(refs[i])
        hflip[b, M - len(hyps[j]):] = torch.from_numpy(hyps[j][::-1].copy())
        if timed:
            rb[b, :len(refs[i])], re_[b, :len(refs[i])] = torch.from_numpy(w["rivs"][i][:, 0].copy()), torch.from_numpy(w["rivs"][i][:, 1].copy())
            hbf[b, M - len(hyps[j]):] = torch.from_numpy(w["hivs"][j][::-1, 0].copy())
            hef[b, M - len(hyps[j]):] = torch.from_numpy(w["hivs"][j][::-1, 1].copy())
    r, hflip = r.to(dev), hflip.to(dev)
    if timed:
        rb, re_, hbf, hef = rb.to(dev), re_.to(dev), hbf.to(dev), hef.to(dev)
    lr = torch.tensor([len(refs[i]) for i, _ in pairs], device=dev)
    lh = torch.tensor([len(hyps[j]) for _, j in pairs], device=dev)
    ragged = bool((lr != N).any() or (lh != M).any())
    end_d, rows = lr + lh, torch.arange(B, device=dev)
    res = torch.where(end_d <= 1, end_d * UNIT, torch.zeros_like(end_d))   # a pair that ends on diagonal 0 or 1 has an empty side
    unit, hit, closed = torch.tensor(UNIT, device=dev), torch.tensor(-1, device=dev), torch.tensor(1 << 60, device=dev)
    ramp = torch.arange(N + M + 1, device=dev, dtype=torch.int64) * UNIT
    p2 = torch.zeros((B, N + 1), dtype=torch.int64, device=dev)            # diagonal 0: D[0][0]
    p1 = torch.zeros((B, N + 1), dtype=torch.int64, device=dev)            # diagonal 1: D[0][1], D[1][0]
    p1[:, :2] = UNIT
    for d in range(2, N + M + 1):
        lo, hi = max(1, d - M), min(N, d - 1)                              # interior rows of the diagonal: j = d - i in [1, M]
        cur = torch.empty_like(p1)
        if lo <= hi:
            x0 = M - d + lo                                                # hyp[d - i - 1] = hflip[M - d + i]
            step = torch.where(r[:, lo - 1:hi] == hflip[:, x0:x0 + hi - lo + 1], hit, unit)
            if timed:
                step = torch.where((rb[:, lo - 1:hi] < hef[:, x0:x0 + hi - lo + 1]) & (hbf[:, x0:x0 + hi - lo + 1] < re_[:, lo - 1:hi]), step, closed)
            cur[:, lo:hi + 1] = torch.minimum(torch.minimum(p1[:, lo - 1:hi], p1[:, lo:hi + 1]) + UNIT, p2[:, lo - 1:hi] + step)
        if d <= M:
            cur[:, 0] = ramp[d]
        if d <= N:
            cur[:, d] = ramp[d]
        if ragged:
            res = torch.where(end_d == d, cur[rows, lr.clamp(max=N)], res)
        p2, p1 = p1, cur
    if not ragged:
        res = p1[:, N]
    e = -((-res) // UNIT)
    return torch.stack([e, e * UNIT - res], 1).cpu()


def numpy_scan(ref, hyp, riv=None, hiv=None):
    ref, hyp = ref.astype(np.int64), hyp.astype(np.int64)
    ramp = np.arange(len(hyp) + 1, dtype=np.int64) * UNIT
    prev = ramp.copy()
    for i in range(len(ref)):
        step = np.where(hyp == ref[i], -1, UNIT)
        if riv is not None:
            step = np.where((riv[i, 0] < hiv[:, 1]) & (hiv[:, 0] < riv[i, 1]), step, 1 << 60)
        t = np.empty(len(hyp) + 1, np.int64)
        t[0] = (i + 1) * UNIT
        t[1:] = np.minimum(prev[1:] + UNIT, prev[:-1] + step)
        prev = np.minimum.accumulate(t - ramp) + ramp
    e = -(-int(prev[-1]) // UNIT)
    return e, e * UNIT - int(prev[-1])


# ---- agreement at the timed sizes, which is the warm-up of every arm too
for k, w in W.items():
    w["out"] = torch.empty((len(w["table"]), 2), dtype=torch.int32, device="cuda")
    a, b = hip(w), torch_sweep(w)
    hip_kernel(w)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, w["out"].cpu().long()), k
    i, j = w["pairs"][3]
    assert tuple(a[3].tolist()) == numpy_scan(w["refs"][i], w["hyps"][j], w.get("rivs", [None] * 8)[i] if w["riv"] is not None else None,
                                              w.get("hivs", [None] * 8)[j] if w["riv"] is not None else None), k
    print(f"{k}: hip == torch on all {len(a)} pairs; errors {int(a[:, 0].sum())}, hits {int(a[:, 1].sum())}, cells {w['cells']:.3e}")
for w in W.values():
    hip(w)
torch.cuda.synchronize()

ts = {f"{arm}.{k}": [] for k in W for arm in ("hip", "kernel", "torch")}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for rnd in range(ROUNDS):
    for k, w in W.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip(w)
        ts[f"hip.{k}"].append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip_kernel(w)
        e1.record()
        torch.cuda.synchronize()
        ts[f"kernel.{k}"].append(e0.elapsed_time(e1))
        if rnd < TORCH_ROUNDS[k]:
            t0 = time.perf_counter()
            torch_sweep(w)
            ts[f"torch.{k}"].append((time.perf_counter() - t0) * 1e3)
power = ps.stop()

print(f"tools/bench_edit_distance.py: {ROUNDS} rounds of hip / kernel, {TORCH_ROUNDS} rounds of torch, arms alternating after a warm-up of all; "
      f"utts = 4096 pairs of 20-200 words, session = 8 x 8 streams of 12 000 words; K={L.EDIT_K}, lanes {L.EDIT_LANES_NARROW} / {L.EDIT_LANES}")
for name, v in ts.items():
    k = name.split(".", 1)[1]
    m = statistics.median(v)
    print(f"{name:18s} median {m:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {W[k]['cells'] / m / 1e6:9.2f} G cell updates / s")
for k in W:
    print(f"hip.{k} / torch.{k} = {statistics.median(ts[f'hip.{k}']) / statistics.median(ts[f'torch.{k}']):.5f}")
print("board power over the timed window:", power)
# ---- the host row-scan, on a subset, scaled
t0 = time.perf_counter()
for i in range(256):
    numpy_scan(utt_refs[i], utt_hyps[i])
dt = time.perf_counter() - t0
sub = float(sum(len(utt_refs[i]) * len(utt_hyps[i]) for i in range(256)))
print(f"numpy.utts         {dt * 1e3:10.1f} ms for the first 256 pairs ({sub / dt / 1e9:.3f} G cell updates / s): x {W['utts']['cells'] / sub:.1f} = "
      f"{dt * W['utts']['cells'] / sub * 1e3:.0f} ms for the workload")
for k in ("session", "session+iv"):
    w = W[k]
    t0 = time.perf_counter()
    numpy_scan(ses_refs[0], ses_hyps[0], w["rivs"][0] if k != "session" else None, w["hivs"][0] if k != "session" else None)
    dt = time.perf_counter() - t0
    sub = float(len(ses_refs[0]) * len(ses_hyps[0]))
    print(f"numpy.{k:12s} {dt * 1e3:10.1f} ms for one of the 64 tables ({sub / dt / 1e9:.3f} G cell updates / s): x {w['cells'] / sub:.1f} = "
          f"{dt * w['cells'] / sub * 1e3:.0f} ms for the workload")

"""The diarization front end on one 60-minute, 8-speaker synthetic diarization against the reference's formulation on dense masks, one process
on one board:   python tools/bench_diar_front_end.py [rounds]

After a warm-up of the GPU arms, these alternate for `rounds` (default 5) rounds, each timed with the wall clock around a device synchronisation
(the host's share is the point of the comparison):
  table          SpeakerSegments.from_samples: clipping and the one sweep over the endpoints (host only)
  front_end      a new SpeakerSegments, then stno_masks for all 8 targets and select_enrollment_windows with the weights rows: the table, its
                 upload and the three launches
  device_only    the same without the table: the cached counts dropped, so all three launches run
  dense_numpy    what the reference does per target speaker (src/data/local_datasets.py:162-194, :261-277), restated in numpy: rasterise the
                 [8, n_samples] mask, pad, cast to fp32, mean-pool by 320, the STNO formula (data.pool_speaker_mask / create_stno_masks); then
                 rasterise again, zero the overlapped samples, mean-pool the target's row by 1600 in fp64, np.convolve with 300 ones, argmax.  The
                 mask is rasterised as uint8 (the dtype lhotse's speakers_audio_mask returns was not checked; a wider one only costs more).
                 One target at a time, as the reference's dataset does; not run through lhotse, whose own cost comes on top.
Before the rounds the two sides are compared: STNO masks bit for bit, and each greedy window's exact count.
Reported: median (min .. max) milliseconds per arm, and the shader clock rocm-smi showed meanwhile."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import data, diar_front_end as D
from bench import PowerSampler

ROUNDS = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
S, N = 8, 60 * 60 * 16000 + 4321
rng = np.random.default_rng(0)
intervals = {}
for s in range(S):                       # turns of about 4 s with pauses of about 20 s: each speaker talks a sixth of the time, overlaps are common
    iv, t = [], int(rng.exponential(20.0) * 16000)
    while t < N:
        d = 1 + int(rng.exponential(4.0) * 16000)
        iv.append((t, min(t + d, N)))
        t += d + 1 + int(rng.exponential(20.0) * 16000)
    intervals[f"spk{s}"] = iv
n_iv = sum(len(v) for v in intervals.values())


def rasterise():
    m = np.zeros((S, N), dtype=np.uint8)
    for s in range(S):
        for a, b in intervals[f"spk{s}"]:
            m[s, a:b] = 1
    return m


def dense_one_target(t):
    stno = data.create_stno_masks(data.pool_speaker_mask(rasterise()), t)                 # [T, 4]
    m = rasterise()
    m[:, m.sum(axis=0) > 1] = 0
    act = np.array(m[t], dtype=float)
    nb = len(act) // 1600
    act = act[:nb * 1600].reshape(nb, 1600).mean(axis=1)
    w = np.convolve(act, np.ones(300, dtype=float), mode="valid")
    if w.max() == 0:
        act = np.array(rasterise()[t], dtype=float)[:nb * 1600].reshape(nb, 1600).mean(axis=1)
        w = np.convolve(act, np.ones(300, dtype=float), mode="valid")
    return stno, int(np.argmax(w)), float(w.max())


def front_end(segs=None):
    segs = D.SpeakerSegments.from_samples(intervals, N) if segs is None else segs
    segs._counts.clear()
    m = D.stno_masks(segs)
    e = D.select_enrollment_windows(segs, return_weights=True)
    return m, e


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


segs0 = D.SpeakerSegments.from_samples(intervals, N)
for _ in range(3):
    m, e = front_end(segs0)
torch.cuda.synchronize()
mc, start, count, w_all = m.cpu().numpy(), e[0].tolist(), e[1].tolist(), e[3].cpu().numpy()
for t in range(S):                       # the two sides agree before anything is timed
    stno, ref_start, ref_act = dense_one_target(t)
    assert np.array_equal(np.ascontiguousarray(stno.T).view(np.int32), mc[t].view(np.int32)), t
    assert abs(count[t] / 1600 - ref_act) < 1e-9 and int(w_all[t][ref_start]) == count[t] and start[t] <= ref_start, t
print("the two sides agree on all targets", flush=True)
arms = {"table": lambda: D.SpeakerSegments.from_samples(intervals, N), "front_end": front_end, "device_only": lambda: front_end(segs0),
        "dense_numpy": lambda: [dense_one_target(t) for t in range(S)]}
ts = {k: [] for k in arms}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for _ in range(ROUNDS):
    for k, f in arms.items():
        ts[k].append(timed(f)[0])
power = ps.stop()
print(f"tools/bench_diar_front_end.py: {N} samples ({N / 16000 / 60:.1f} min), {S} speakers, {n_iv} segments, table of {segs0.E} entries, "
      f"T_total {segs0.T_total}, {segs0.n_windows} windows; all {S} targets; {ROUNDS} rounds, arms alternating after a warm-up")
for k, v in ts.items():
    print(f"{k:12s} median {statistics.median(v):10.2f} ms (min {min(v):.2f}, max {max(v):.2f})")
print("dense_numpy / front_end =", round(statistics.median(ts["dense_numpy"]) / statistics.median(ts["front_end"]), 1))
print("power / clock:", power if power else "rocm-smi gave no sample")

"""dicow_diar_score against the dense-mask formulation in torch ops on the same device and against the host sweep in numpy, one process on
one board:
    python tools/bench_diar_score.py [rounds]

Two workloads (every position a multiple of 160 ticks, so the 100-frames-per-second masks of the torch arm hold them exactly):
  corpus   200 one-hour sessions of 8 x 8 speakers, 2400 reference and 2400 hypothesis segments each (the hypothesis: the reference's
           segments moved by up to 0.5 s, one in ten given to another speaker), collar 0.2 s -- 200 problems of ONE call
  single   one one-hour session of 64 x 64 speakers, 3200 segments a side (about 20 000 regions), collar 0.2 s
Arms, alternating round by round after a warm-up of all:
  hip.*          diar_scoring.diar_score_counts and the download: packing the host tables, the upload, the three launches, the copy
                 back -- wall clock around a call that ends in the download's synchronise
  kernel.*       device events around the entry point alone (its host checks and the four uploads included), tables packed beforehand,
                 at the library's chunk (DICOW_DIAR_SCORE_CHUNK regions per workgroup); kernel.c128.* / kernel.c64.*: with 128 / 64
  kernel.part.*  the same on the part of the workload the torch arm runs (the first 20 sessions of `corpus`; all of `single`)
  torch.*        per session, masks at 100 frames per second on the device (16 kHz masks of an hour do not fit the comparison): +1 / -1
                 at the segment ends, a cumulative sum, `> 0`; the unscored mask the same way; C = ref @ hyp.T in fp32 (counts below
                 2^24 are exact), R, H and the five scalars from the two count rows.  The interval lists are on the device before the
                 clock starts.  Wall clock around the loop and a synchronise.
  numpy.*        the strongest host formulation: per session np.unique over all endpoints, searchsorted for the two bitmasks and the
                 unscored parity, then bits_ref.T @ (dur[:, None] * bits_hyp) in float64 (exact below 2^53); all sessions
Before anything is timed hip, torch (x 160) and numpy must agree on everything they ran."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, ops, diar_scoring as D
from ts_asr_whisper_amd.diar_front_end import SpeakerSegments

ROUNDS = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
GRID, HOUR, COLLAR = 160, 3600 * 16000, 0.2
TORCH_PART = {"corpus": 20, "single": 1}
rng = np.random.default_rng(0)


def session(S, per_speaker):
    ref, hyp = {f"r{s}": [] for s in range(S)}, {f"h{s}": [] for s in range(S)}
    for s in range(S):
        a = rng.integers(0, (HOUR - 20 * 16000) // GRID, per_speaker) * GRID
        d = rng.integers(50, 1000, per_speaker) * GRID                     # 0.5 .. 10 s
        ja, jb = rng.integers(-50, 51, per_speaker) * GRID, rng.integers(-50, 51, per_speaker) * GRID
        to = np.where(rng.random(per_speaker) < 0.1, rng.integers(0, S, per_speaker), s)
        for k in range(per_speaker):
            ref[f"r{s}"].append((int(a[k]), int(a[k] + d[k])))
            hyp[f"h{to[k]}"].append((max(0, int(a[k] + ja[k])), int(a[k] + d[k] + jb[k])))
    return SpeakerSegments(ref, HOUR), SpeakerSegments(hyp, HOUR)


def make(pairs):
    problems = [(r, h, D.unscored_intervals(r, COLLAR), False) for r, h in pairs]
    b, a, u, pt = D.pack_problems(problems)
    w = dict(pairs=pairs, problems=problems, tables=(b, a, u, pt), out=torch.empty((len(pairs), L.DIAR_SCORE_OUT_WORDS), dtype=torch.int64, device="cuda"))
    w["regions"] = sum(r.E + 1 + h.E + 1 + 2 * len(p[2]) - 1 for (r, h), p in zip(pairs, problems))
    w["dev"] = [dense_inputs(*p[:3]) for p in problems[:TORCH_PART["corpus" if len(pairs) > 1 else "single"]]]
    return w


def hip(w):
    return D.diar_score_counts(w["problems"]).cpu()


def hip_kernel(w, chunk=0):
    t = D.table_args(*w["tables"], chunk)
    nbytes = L.lib().dicow_diar_score_ws_bytes(*t)
    assert nbytes >= 0, L.lib().dicow_last_error()
    ws = ops.workspace(nbytes, w["out"].device)
    L.call("dicow_diar_score", *t, w["out"].data_ptr(), ws.data_ptr(), nbytes, L.stream())
    return nbytes


def dense_inputs(ref, hyp, uns):
    def side(segs):
        rows = [(s, a // GRID, b // GRID) for s, spk in enumerate(segs.speakers) for a, b in segs.intervals[spk]]
        return torch.tensor(rows, dtype=torch.int64).cuda().T.contiguous(), segs.S
    u = torch.tensor([(0, a // GRID, b // GRID) for a, b in uns.tolist()], dtype=torch.int64).reshape(-1, 3).cuda().T.contiguous()
    return side(ref), side(hyp), (u, 1), HOUR // GRID


def dense_torch(inp):
    (r, Sr), (h, Sh), (u, _), n = inp

    def mask(t, S):
        d = torch.zeros(S, n + 1, dtype=torch.int32, device="cuda")
        one = torch.ones(t.shape[1], dtype=torch.int32, device="cuda")
        d.index_put_((t[0], t[1].clamp(max=n)), one, accumulate=True)
        d.index_put_((t[0], t[2].clamp(max=n)), -one, accumulate=True)
        return d.cumsum(1)[:, :n] > 0
    scored = ~mask(u, 1)[0]
    rm, hm = mask(r, Sr) & scored, mask(h, Sh) & scored
    rf, hf = rm.float(), hm.float()
    nr, nh = rf.sum(0), hf.sum(0)
    C = rf @ hf.T
    sc = torch.stack([nr.sum(), (nr - nh).clamp(min=0).sum(), (nh - nr).clamp(min=0).sum(), torch.minimum(nr, nh).sum()])
    return C, rf.sum(1), hf.sum(1), sc


def host_numpy(ref, hyp, uns):
    flat = uns.reshape(-1)
    pts = np.unique(np.concatenate([ref.bounds, hyp.bounds, flat]))
    s, dur = pts[:-1], np.diff(pts).astype(np.float64)

    def bits(t):
        q = np.searchsorted(t.bounds, s, side="right")
        m = np.where((q >= 1) & (q <= t.E), t.active[np.clip(q - 1, 0, max(t.E - 1, 0))], np.uint64(0))
        return ((m[:, None] >> np.arange(t.S, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)
    dur = np.where(np.searchsorted(flat, s, side="right") & 1, 0.0, dur)
    br, bh = bits(ref), bits(hyp)
    nr, nh = br.sum(1), bh.sum(1)
    C = br.T @ (dur[:, None] * bh)
    return C, dur @ br, dur @ bh, np.array([dur @ nr, dur @ np.maximum(nr - nh, 0), dur @ np.maximum(nh - nr, 0), dur @ np.minimum(nr, nh)])


def same(row, Sr, Sh, C, Rv, Hv, sc, scale):
    c = D.split_counts(row, Sr, Sh)
    want = [c["C"], c["R"], c["H"], np.array([c[k] for k in D.SCALARS[1:]])]
    return all(np.array_equal(np.asarray(g, np.float64) * scale, np.asarray(x, np.float64)) for g, x in zip((C, Rv, Hv, sc), want))


W = {"corpus": make([session(8, 300) for _ in range(200)]), "single": make([session(64, 50)])}

# ---- agreement, which is the warm-up of every arm too
for k, w in W.items():
    a = hip(w).numpy()
    for chunk in (128, 64, 0):
        w["bytes"] = hip_kernel(w, chunk)
        torch.cuda.synchronize()
        assert np.array_equal(a, w["out"].cpu().numpy()), (k, chunk)
    for i, inp in enumerate(w["dev"]):
        r, h = w["pairs"][i]
        assert same(a[i], r.S, h.S, *[t.cpu().numpy() for t in dense_torch(inp)], GRID), (k, i)
    w["cut"] = make(w["pairs"][:TORCH_PART[k]]) if TORCH_PART[k] < len(w["pairs"]) else w
    hip_kernel(w["cut"])
    torch.cuda.synchronize()
    assert np.array_equal(a[:TORCH_PART[k]], w["cut"]["out"].cpu().numpy()), k
    err = D.aggregate_diarization_scores([dict(D._error_ticks(c), **D.jaccard_from_counts(c), **{"speaker count error": 0})
                                          for c in (D.split_counts(a[i], 8 if k == "corpus" else 64, 8 if k == "corpus" else 64) for i in range(len(a)))])
    print(f"{k}: hip == torch x {GRID} where torch ran; {len(w['pairs'])} problems, {w['regions']} regions, workspace {w['bytes'] / 2 ** 20:.1f} MiB at chunk {L.DIAR_SCORE_CHUNK}, "
          f"DER {err['DER']:.4f} (Miss {err['Miss']:.4f} FA {err['FA']:.4f} Conf {err['Conf']:.4f}) JER {err['JER']:.4f}")
    w["all"] = a

ts = {f"{arm}.{k}": [] for k in W for arm in ("hip", "kernel", "kernel.c128", "kernel.c64", "kernel.part", "torch")}
for rnd in range(ROUNDS):
    for k, w in W.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip(w)
        ts[f"hip.{k}"].append((time.perf_counter() - t0) * 1e3)
        for arm, x, chunk in (("kernel", w, 0), ("kernel.c128", w, 128), ("kernel.c64", w, 64), ("kernel.part", w["cut"], 0)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip_kernel(x, chunk)
            e1.record()
            torch.cuda.synchronize()
            ts[f"{arm}.{k}"].append(e0.elapsed_time(e1))
        if rnd < 5:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for inp in w["dev"]:
                dense_torch(inp)
            torch.cuda.synchronize()
            ts[f"torch.{k}"].append((time.perf_counter() - t0) * 1e3)

print(f"tools/bench_diar_score.py: {ROUNDS} rounds of hip / kernel / kernel.c128 / kernel.c64 / kernel.part, 5 rounds of torch, arms alternating after a warm-up "
      f"of all; DICOW_DIAR_SCORE_CHUNK={L.DIAR_SCORE_CHUNK}")
for name, v in ts.items():
    arm, k = name.rsplit(".", 1)
    on_part = arm in ("torch", "kernel.part")
    regions = W[k]["cut"]["regions"] if on_part else W[k]["regions"]
    m = statistics.median(v)
    note = f"   on the first {TORCH_PART[k]} sessions" if on_part and k == "corpus" else ""
    print(f"{name:22s} median {m:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {regions / m / 1e3:9.3f} M regions / s{note}")
for k, w in W.items():
    print(f"kernel.part.{k} / torch.{k} = {statistics.median(ts[f'kernel.part.{k}']) / statistics.median(ts[f'torch.{k}']):.6f}")
    t0 = time.perf_counter()
    got = [host_numpy(*p[:3]) for p in w["problems"]]
    dt = (time.perf_counter() - t0) * 1e3
    assert all(same(w["all"][i], r.S, h.S, *got[i], 1) for i, (r, h) in enumerate(w["pairs"])), k    # numpy == hip on everything
    print(f"numpy.{k:16s} {dt:10.1f} ms   {w['regions'] / dt / 1e3:9.3f} M regions / s      hip.{k} / numpy.{k} = "
          f"{statistics.median(ts[f'hip.{k}']) / dt:.6f}")

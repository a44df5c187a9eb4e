"""dicow_orc_distance against the same dynamic program in torch ops on the same device and in numpy on the host, one process on one board:
    python tools/bench_orc_distance.py [rounds]

Two workloads:
  grouped    one AMI-like session cut into 200 groups: 2-4 hypothesis streams of 5-40 words (2 streams in half of the groups, 4 in one of
             seven), 1-6 reference utterances of 3-15 words, a vocabulary of 50 -- 200 problems of ONE call, as session_tcorc_wer makes it
  ungrouped  one problem of 3 streams x 80 words (531 441 states) against 40 utterances of 3-20 words
Arms, alternating round by round after a warm-up of all:
  hip.*      scoring.orc_counts: the descriptor upload, the launches, the (errors, hits) download -- wall clock around a call that ends in
             the download's synchronise; `kernel`: device events around the entry point alone; `kernel+asg`: the same with the assignment
  torch.*    per problem, utterance, axis and word: the deletion and diagonal terms as two whole-table ops, then the insertion chain as
             one sliced minimum per hypothesis word along the axis; the minimum over the axes per utterance.  int64 keys.  It is
             launch-bound and slow, so it is timed on a part of the workload (the first 20 groups; the first 8 utterances), and
             `kernel.part` is the entry point on exactly that part: the ratio is taken there, nothing is scaled
  numpy.*    the same on the host with minimum.accumulate for the insertion chain (all groups; the first 8 utterances)
Reported: median (min .. max) per call, cell updates per second (cells = sum over problems and utterances of words x streams x states).
Before anything is timed hip and torch must agree on the part torch runs; the numpy run at the end must agree with hip on all it ran."""
import os, sys, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, ops, scoring

ROUNDS = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
TORCH_PART = {"grouped": 20, "ungrouped": 8}           # problems / utterances the torch arm runs
UNIT = 1 << 15
rng = np.random.default_rng(0)


def make(problems):
    """problems: [(utts, hyps)] -> flat device buffers, the three host tables, cell updates per problem."""
    ref, hyp, ut, st, pt = [], [], [], [], []
    for utts, hyps in problems:
        pt.append((len(ut), len(utts), len(st), len(hyps)))
        for u in utts:
            ut.append((len(ref), len(u)))
            ref += u.tolist()
        for h in hyps:
            st.append((len(hyp), len(h)))
            hyp += h.tolist()
    cells = [float(sum(len(u) for u in utts) * len(hyps) * np.prod([len(h) + 1 for h in hyps])) for utts, hyps in problems]
    return dict(ref=torch.tensor(ref, dtype=torch.int32).cuda(), hyp=torch.tensor(hyp, dtype=torch.int32).cuda(), problems=problems,
                pt=np.array(pt, np.int64), ut=np.array(ut, np.int64), st=np.array(st, np.int64), cells=cells,
                out=torch.empty((len(pt), 2), dtype=torch.int32, device="cuda"), asg=torch.empty(len(ut), dtype=torch.int32, device="cuda"))


def draw(n_streams, lo, hi, n_utts, ulo, uhi, vocab=50):
    return ([rng.integers(0, vocab, int(rng.integers(ulo, uhi + 1))) for _ in range(n_utts)],
            [rng.integers(0, vocab, int(rng.integers(lo, hi + 1))) for _ in range(n_streams)])


W = {"grouped": make([draw(int(rng.choice([2, 2, 2, 3, 3, 3, 4])) if g % 2 else 2, 5, 40, int(rng.integers(1, 7)), 3, 15) for g in range(200)]),
     "ungrouped": make([draw(3, 80, 80, 40, 3, 20)])}


def hip(w):
    return scoring.orc_counts(w["ref"], w["hyp"], w["pt"], w["ut"], w["st"])[:, :2]


def hip_kernel(w, assign):
    """The entry point alone on the current stream (no download); False when the call would be refused (the workspace cap)."""
    tables = (w["pt"].ctypes.data, len(w["pt"]), w["ut"].ctypes.data, w["st"].ctypes.data)
    nbytes = L.lib().dicow_orc_distance_ws_bytes(*tables, int(assign))
    if nbytes < 0:
        return False
    ws = ops.workspace(nbytes, w["ref"].device)
    L.call("dicow_orc_distance", w["ref"].data_ptr(), w["ref"].numel(), w["hyp"].data_ptr(), w["hyp"].numel(), None, None, *tables,
           w["out"].data_ptr(), w["asg"].data_ptr() if assign else None, ws.data_ptr(), nbytes, L.stream())
    return True


def dp(utts, hyps, xp, dev=None):
    """The dynamic program with tensor ops of `xp` (torch on `dev`, or numpy)."""
    tt = xp is torch
    H, shape = len(hyps), [len(h) + 1 for h in hyps]
    arange = (lambda n: torch.arange(n, device=dev, dtype=torch.int64)) if tt else (lambda n: np.arange(n, dtype=np.int64))
    Lt = sum((arange(n) * UNIT).reshape([-1 if a == ax else 1 for a in range(H)]) for ax, n in enumerate(shape))
    Lt = Lt + (torch.zeros(shape, dtype=torch.int64, device=dev) if tt else np.zeros(shape, np.int64))
    hy = [torch.as_tensor(h, device=dev).long() if tt else h.astype(np.int64) for h in hyps]
    for utt in utts:
        new = None
        for ax in range(H):
            T = Lt.movedim(ax, 0) if tt else np.moveaxis(Lt, ax, 0)
            col = [-1] + [1] * (H - 1)
            for wd in utt.tolist():
                cost = (torch.where(hy[ax] == wd, -1, UNIT) if tt else np.where(hy[ax] == wd, -1, UNIT)).reshape(col)
                a = T + UNIT
                a[1:] = xp.minimum(a[1:], T[:-1] + cost)
                if tt:
                    for j in range(1, shape[ax]):                          # the insertion chain: one sliced minimum per hypothesis word
                        a[j] = torch.minimum(a[j], a[j - 1] + UNIT)
                else:
                    ramp = (np.arange(shape[ax], dtype=np.int64) * UNIT).reshape(col)
                    a = np.minimum.accumulate(a - ramp, axis=0) + ramp
                T = a
            T = T.movedim(0, ax) if tt else np.moveaxis(T, 0, ax)
            new = T if new is None else xp.minimum(new, T)
        if len(utt):
            Lt = new
    v = int(Lt.reshape(-1)[-1])
    e = (v + UNIT - 1) >> 15
    return e, e * UNIT - v


def part(w, k, n):
    """The first n problems (grouped) or the problem cut to its first n utterances (ungrouped), and its cell updates."""
    if k == "grouped":
        return w["problems"][:n], sum(w["cells"][:n])
    utts, hyps = w["problems"][0]
    return [(utts[:n], hyps)], w["cells"][0] * sum(len(u) for u in utts[:n]) / sum(len(u) for u in utts)


def torch_arm(probs):
    out = [dp(u, h, torch, "cuda") for u, h in probs]
    torch.cuda.synchronize()
    return out


# ---- agreement, which is the warm-up of every arm too
for k, w in W.items():
    a = hip(w)
    assert hip_kernel(w, False)
    torch.cuda.synchronize()
    assert torch.equal(a, w["out"].cpu().long()), k
    w["with_asg"] = hip_kernel(w, True)
    torch.cuda.synchronize()
    assert not w["with_asg"] or torch.equal(a, w["out"].cpu().long()), k
    probs, _ = part(w, k, TORCH_PART[k])
    w["cut"] = make(probs)
    w["part"] = [tuple(x) for x in hip(w["cut"]).tolist()]                  # hip on what torch (and for `ungrouped` numpy) runs
    assert k != "grouped" or w["part"] == [tuple(x) for x in a[:len(probs)].tolist()]
    w["all"] = [tuple(x) for x in a.tolist()]
    assert torch_arm(probs) == w["part"], k
    states = [int(np.prod([len(h) + 1 for h in hyps])) for _, hyps in w["problems"]]
    print(f"{k}: hip == torch where torch ran; {len(w['pt'])} problems, states {min(states)} .. {max(states)} (sum {sum(states)}), "
          f"errors {int(a[:, 0].sum())}, hits {int(a[:, 1].sum())}, cell updates {sum(w['cells']):.3e}; with assignment: "
          f"{'runs' if w['with_asg'] else 'refused (DICOW_ORC_MAX_WS_BYTES)'}")

ts = {f"{arm}.{k}": [] for k in W for arm in ("hip", "kernel", "kernel+asg", "kernel.part", "torch")}
for rnd in range(ROUNDS):
    for k, w in W.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip(w)
        ts[f"hip.{k}"].append((time.perf_counter() - t0) * 1e3)
        for arm, assign in (("kernel", False), ("kernel+asg", True), ("kernel.part", False)):
            if assign and not w["with_asg"]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip_kernel(w["cut"] if arm == "kernel.part" else w, assign)
            e1.record()
            torch.cuda.synchronize()
            ts[f"{arm}.{k}"].append(e0.elapsed_time(e1))
        if rnd < 2:
            probs, _ = part(w, k, TORCH_PART[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_arm(probs)
            ts[f"torch.{k}"].append((time.perf_counter() - t0) * 1e3)

print(f"tools/bench_orc_distance.py: {ROUNDS} rounds of hip / kernel / kernel+asg, 2 rounds of torch, arms alternating after a warm-up of all; "
      f"K={L.ORC_K}")
for name, v in ts.items():
    arm, k = name.rsplit(".", 1)
    if not v:
        print(f"{name:22s} not run: the call is refused (DICOW_ORC_MAX_WS_BYTES)")
        continue
    on_part = arm in ("torch", "kernel.part")
    cells = part(W[k], k, TORCH_PART[k])[1] if on_part else sum(W[k]["cells"])
    m = statistics.median(v)
    note = f"   on the first {TORCH_PART[k]} {'groups' if k == 'grouped' else 'utterances'}" if on_part else ""
    print(f"{name:22s} median {m:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {cells / m / 1e6:9.3f} G cell updates / s{note}")
for k, w in W.items():
    print(f"kernel.part.{k} / torch.{k} = {statistics.median(ts[f'kernel.part.{k}']) / statistics.median(ts[f'torch.{k}']):.6f}")
    probs, cells = (w["problems"], sum(w["cells"])) if k == "grouped" else part(w, k, TORCH_PART[k])
    t0 = time.perf_counter()
    got = [dp(u, h, np) for u, h in probs]
    dt = (time.perf_counter() - t0) * 1e3
    assert got == (w["all"] if k == "grouped" else w["part"]), k           # numpy == hip on everything numpy ran
    print(f"numpy.{k:16s} {dt:10.1f} ms{'' if k == 'grouped' else f' for the first {TORCH_PART[k]} utterances'}   {cells / dt / 1e6:9.3f} G cell updates / s")

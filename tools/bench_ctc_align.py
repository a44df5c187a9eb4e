"""dicow_ctc_forced_align: what the gather costs, what recursion and walk cost, the two plans, and the baselines, one process on one board:
    python tools/bench_ctc_align.py [rounds]

Workloads (seed 0): one session's worth of decoded segments against bf16 logits at V1 = 51 866 in rows of 51 968, four 30 s windows side
by side as chunked_ctc_logits lays them
  session.1500   400 segments of 5-60 tokens over 100-1500 frames of 20 ms (T = 6000)
  session.375    the same segments over a quarter of the frames, 80 ms each (pre_ctc_sub_sample: Tn = 375, T = 1500), never fewer than the
                 tokens need
  long.1500      64 segments of 64-400 tokens over 800-1500 frames: the wide plan's own ground
Libraries, each loaded with ctypes beside the shipped one (a missing variant drops its arms, and the output says so):
  tools/libv_cagather.so   tools/build_var.sh --file ctc_align.hip cagather "-DCA_ONLY=1" caalign "-DCA_ONLY=2" carecur "-DCA_ONLY=3":
  tools/libv_caalign.so    dicow_ctc_forced_align launching only the gather / only recursion and walk (over the E the full call before it
  tools/libv_carecur.so    left in ws) / only the recursion, without the walk
Arms, device events around the entry point alone (table copy + launches), alternating round by round after a warm-up of all:
  auto     plan 0, as shipped: narrow for L <= 63, wide otherwise        wide / narrow   the plan forced (narrow where every L <= 63)
  gather   the gather alone                                              align           recursion and walk alone
  recur    the recursion alone (back-pointers stored, nothing walked): align - recur = the walk
  lse      dicow_ctc_frame_lse over all T frames (what ctc_forced_align adds when no lse is passed)
Baselines, each on a stated subset and scaled as its line says: the same recursion as per-frame torch ops on the same device (fp32, the
kernel's own order of operations, the walk on the host), and the numpy scan of tests/ctc_align_ref.py on the host in fp64.
Before anything is timed the tool checks, on the subset, that the kernel's path, spans and score EQUAL the torch recursion's and that its
path spells the targets, and that every arm agrees with `auto` bit for bit."""
import ctypes as C
import os, sys, statistics, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L
from tests import ctc_align_ref as R
from bench import PowerSampler

ROUNDS = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
V1, LD, BLANK = 51866, 51968, 51865
rng = np.random.default_rng(0)
gen = torch.Generator(device="cuda").manual_seed(0)


def fmin(y):
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


def workload(T, lens, frames):
    logits = torch.empty(1, T, LD, dtype=torch.bfloat16, device="cuda")
    for t in range(0, T, 500):                                          # (fp32 normal draws of a whole buffer would take 4x its bytes)
        logits[0, t:t + 500] = torch.randn(min(500, T - t), LD, device="cuda", generator=gen).bfloat16()
    ys = [rng.integers(0, V1 - 1, int(n)).tolist() for n in lens]
    F = [max(int(f), fmin(y)) for f, y in zip(frames, ys)]
    f0 = [int(rng.integers(0, T - f + 1)) for f in F]
    n = len(ys)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    w = dict(logits=logits, T=T, ys=ys, F=F, f0=f0, n=n, table=np.ascontiguousarray(np.stack([np.zeros(n), f0, F, starts, lens], 1).astype(np.int64)),
             flat=np.ascontiguousarray(np.concatenate(ys).astype(np.int32)), lse=torch.empty(T, device="cuda"), Fmax=max(F), Lmax=int(max(lens)),
             cells=float(sum(f * (2 * len(y) + 1) for f, y in zip(F, ys))))
    for k, shape, dt in (("path", (n, w["Fmax"]), torch.int32), ("spans", (n, w["Lmax"], 2), torch.int32), ("ts", (n, w["Lmax"]), torch.float32),
                         ("score", (n,), torch.float32), ("status", (n,), torch.int32)):
        w[k] = torch.empty(shape, dtype=dt, device="cuda")
    return w


seg_lens, seg_frames = rng.integers(5, 61, 400), rng.integers(100, 1501, 400)
W = {"session.1500": workload(6000, seg_lens, seg_frames), "session.375": workload(1500, seg_lens, seg_frames // 4),
     "long.1500": workload(6000, rng.integers(64, 401, 64), rng.integers(800, 1501, 64))}


def bind(path):
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    for name, sig, res in (("dicow_ctc_forced_align", L._SIGS["dicow_ctc_forced_align"], L.c_i), ("dicow_ctc_align_ws_bytes", L._SIGS64["dicow_ctc_align_ws_bytes"], L.c_i64),
                           ("dicow_ctc_frame_lse", L._SIGS["dicow_ctc_frame_lse"], L.c_i)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = sig, res
    lib.dicow_last_error.restype = C.c_char_p
    return lib


LIBS = {"new": bind(L.LIB_PATH), "cagather": bind(os.path.join(ROOT, "tools", "libv_cagather.so")), "caalign": bind(os.path.join(ROOT, "tools", "libv_caalign.so")),
        "carecur": bind(os.path.join(ROOT, "tools", "libv_carecur.so"))}
need = max(LIBS["new"].dicow_ctc_align_ws_bytes(w["table"].ctypes.data, w["n"]) for w in W.values())
assert need > 0, LIBS["new"].dicow_last_error()
WS = torch.empty((need,), dtype=torch.uint8, device="cuda")
print(f"workspace {need / 2 ** 20:.1f} MiB for the largest workload (limit {L.CTC_ALIGN_MAX_WS_BYTES / 2 ** 20:.0f} MiB)")


def lse(lib, w, plan=0):
    rc = lib.dicow_ctc_frame_lse(w["logits"].data_ptr(), 1, w["T"], V1, LD, w["lse"].data_ptr(), L.stream())
    assert rc == 0, lib.dicow_last_error()


def align(lib, w, plan=0):
    rc = lib.dicow_ctc_forced_align(w["logits"].data_ptr(), 1, 1, w["T"], V1, LD, w["lse"].data_ptr(), None, BLANK, w["table"].ctypes.data, w["n"],
                                    w["flat"].ctypes.data, len(w["flat"]), w["path"].data_ptr(), w["Fmax"], w["spans"].data_ptr(), w["Lmax"],
                                    w["ts"].data_ptr(), w["score"].data_ptr(), w["status"].data_ptr(), plan, WS.data_ptr(), need, L.stream())
    assert rc == 0, lib.dicow_last_error()


def outputs(w):
    torch.cuda.synchronize()
    return [w[k].clone() for k in ("path", "spans", "ts", "score", "status")]


def emissions(w, i):
    """x fp32 [F, 2 L + 1] of problem i on the device, as the kernel forms it, and the skip mask."""
    y, f0, F = w["ys"][i], w["f0"][i], w["F"][i]
    lab = torch.full((2 * len(y) + 1,), BLANK, dtype=torch.long, device="cuda")
    lab[1::2] = torch.tensor(y, device="cuda")
    skip = torch.zeros(2 * len(y) + 1, dtype=torch.bool, device="cuda")
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    return w["logits"][0, f0:f0 + F][:, lab].float() - w["lse"][f0:f0 + F, None], skip


def torch_align(w, i):
    """The recursion as per-frame torch ops (the naive form: a handful of launches per frame), the walk on the host."""
    em, skip = emissions(w, i)
    F, S = em.shape
    ninf = torch.full((2,), -float("inf"), device="cuda")
    v = torch.full((S,), -float("inf"), device="cuda")
    v[:2] = em[0, :2]
    bp = torch.zeros(F, S, dtype=torch.int8, device="cuda")
    for f in range(1, F):
        pad = torch.cat([ninf, v])
        p1, p2 = pad[1:S + 1], pad[:S]
        m1 = p1 > v
        best = torch.where(m1, p1, v)
        m2 = skip & (p2 > best)
        best = torch.where(m2, p2, best)
        bp[f] = m1.to(torch.int8) * (~m2).to(torch.int8) + 2 * m2.to(torch.int8)
        v = em[f] + best
    v, bp = v.cpu(), bp.cpu().numpy()
    end = S - 1 if float(v[S - 1]) > float(v[S - 2]) else S - 2
    s, states = end, []
    for f in range(F - 1, -1, -1):
        states.append(s)
        s -= int(bp[f, s])
    states = states[::-1]
    return [w["ys"][i][(s - 1) // 2] if s & 1 else BLANK for s in states], float(v[end])


# ---- agreement at the timed sizes, which is the warm-up of every arm too
SUB = 6
for k, w in W.items():
    lse(LIBS["new"], w)
    align(LIBS["new"], w)
    ref = outputs(w)
    assert int(ref[4].sum()) == 0, k
    for i in range(SUB):
        path, score = torch_align(w, i)
        F, Ln = w["F"][i], len(w["ys"][i])
        assert ref[0][i, :F].cpu().tolist() == path and float(ref[3][i]) == score, (k, i)
        R.check_path(path, w["ys"][i], BLANK)
        assert all(path[a:b] == [t] * (b - a) for (a, b), t in zip(ref[1][i, :Ln].cpu().tolist(), w["ys"][i])), (k, i)
    narrow_ok = max(len(y) for y in w["ys"]) <= 63
    for lib, plan in (("new", 2), ("new", 1), ("cagather", 0), ("caalign", 0), ("carecur", 0)):
        if LIBS[lib] is None or (plan == 1 and not narrow_ok):
            continue
        for t in ("path", "spans", "ts", "score", "status"):
            w[t].fill_(0)
        align(LIBS[lib], w, plan)
        got = outputs(w)
        assert lib == "cagather" or torch.equal(got[3], ref[3]), (k, lib, plan)                    # (the score: every variant but the gather)
        assert lib in ("cagather", "carecur") or all(torch.equal(a, b) for a, b in zip(got, ref)), (k, lib, plan)
    align(LIBS["new"], w)
    print(f"{k}: {w['n']} problems, {sum(w['F'])} frames, {len(w['flat'])} targets, {w['cells']:.3e} trellis cells; the first {SUB} equal the per-frame torch "
          f"recursion (path, score) and spell their targets; every arm equals `auto` bit for bit")
print("variants missing:", [name for name, lib in LIBS.items() if lib is None] or "none")

ARMS = [("lse", "new", lse, 0), ("auto", "new", align, 0), ("wide", "new", align, 2), ("narrow", "new", align, 1), ("gather", "cagather", align, 0),
        ("align", "caalign", align, 0), ("recur", "carecur", align, 0)]
ARMS = [a for a in ARMS if LIBS[a[1]] is not None]
ts = {f"{arm}.{k}": [] for k, w in W.items() for arm, _, _, plan in ARMS if plan != 1 or max(len(y) for y in w["ys"]) <= 63}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for rnd in range(ROUNDS):
    for k, w in W.items():
        align(LIBS["new"], w)                                              # `align` needs this workload's E in WS
        for arm, name, fn, plan in ARMS:
            if f"{arm}.{k}" not in ts:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(LIBS[name], w, plan)
            e1.record()
            torch.cuda.synchronize()
            ts[f"{arm}.{k}"].append(e0.elapsed_time(e1))
            if arm == "gather":
                align(LIBS["new"], w)
power = ps.stop()

print(f"tools/bench_ctc_align.py: {ROUNDS} rounds, arms alternating after a warm-up of all")
med = {}
for name, v in ts.items():
    k = name.split(".", 1)[1]
    med[name] = statistics.median(v)
    print(f"{name:22s} median {med[name]:9.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {W[k]['cells'] / med[name] / 1e6:8.3f} G cells / s")
print("board power over the timed window:", power)

# ---- baselines
for k, w in W.items():
    sub = list(range(SUB))
    share = sum(w["F"][i] * (2 * len(w["ys"][i]) + 1) for i in sub) / w["cells"]
    frames = sum(w["F"][i] for i in sub) / sum(w["F"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in sub:
        torch_align(w, i)
    dt = time.perf_counter() - t0
    print(f"torch per-frame ops, {k}: {dt * 1e3:9.1f} ms for the first {SUB} problems ({frames:.4f} of the frames): x {1 / frames:.1f} = {dt / frames * 1e3:.0f} ms "
          f"for all {w['n']}; auto = {med[f'auto.{k}']:.3f} ms")
    host = []
    for i in sub:                                                          # the columns a problem uses, copied to the host outside the clock
        cols = sorted(set(w["ys"][i])) + [BLANK]
        x = w["logits"][0, w["f0"][i]:w["f0"][i] + w["F"][i]][:, torch.tensor(cols, device="cuda")].float() - w["lse"][w["f0"][i]:w["f0"][i] + w["F"][i], None]
        host.append((x.double().cpu().numpy(), [cols.index(t) for t in w["ys"][i]], len(cols) - 1))
    t0 = time.perf_counter()
    got = [R.align(x, y, b) for x, y, b in host]
    dt = time.perf_counter() - t0
    assert all(g["status"] == 0 for g in got)
    print(f"numpy scan on the host, {k}: {dt * 1e3:9.1f} ms for the first {SUB} problems ({share:.4f} of the cells): x {1 / share:.1f} = {dt / share * 1e3:.0f} ms "
          f"for all {w['n']}, the copy of the logits' columns to the host not counted")

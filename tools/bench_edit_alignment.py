"""dicow_edit_alignment: what recording costs, what the walk costs, and the alignment layer end to end, one process on one board:
    python tools/bench_edit_alignment.py [rounds]

Workloads, those of tools/bench_edit_distance.py (same generator, same seed):
  utts        4096 utterance pairs of 20-200 words (word_alignments; one launch, the narrow workgroup)
  session8    the 8 assigned pairs of one session of 8 x 8 streams of 12 000 words -- what session_alignment aligns after the Hungarian
              step -- without and with intervals (`+iv`); the wide workgroup, three panels a table, 37 MB of records a pair
  session24   24 of the 64 pairs of that session (three hypotheses per reference stream): as many tables as fit under
              DICOW_ALIGN_MAX_WS_BYTES in one call (all 64 would need 2.4 GB of records)
Libraries, each loaded with ctypes beside the shipped one (a missing variant drops its arms, and the output says so):
  tools/libv_parent.so   the parent commit's library: csrc/build.sh in a checkout of the parent, the .so copied here
  tools/libv_eafwd.so    tools/build_var.sh --file edit_alignment.hip eafwd "-DEA_ONLY=1" eawalk "-DEA_ONLY=2": dicow_edit_alignment
  tools/libv_eawalk.so   launching only the recording pass / only the walk (over the records the full call before it left in ws)
Arms, device events around the entry point alone (table copy + launches), alternating round by round after a warm-up of all:
  dist.parent / dist.new   dicow_edit_distance of the parent's and of this tree's library: the counts kernel before and after
  record                   the recording pass alone        record - dist.new = the cost of recording
  walk                     the walk alone
  full                     dicow_edit_alignment as shipped
End to end, wall clock: scoring.session_alignment on that session as segments of 20 words (64 counts tables, Hungarian, 8 alignments, the
rows) and scoring.word_alignments on the 4096 utterances, against a numpy row-scan that keeps one step code per cell plus a Python
traceback on the host, timed on a subset (one session table, 256 utterances) and scaled as its line says.
Before anything is timed the tool checks the full call against that host traceback on one pair of each workload, that every arm's
(errors, hits) agree, and that the ops reproduce them."""
import ctypes as C
import os, sys, statistics, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import amd_pkg
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L, scoring
from bench import PowerSampler

ROUNDS = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
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
    n, total = len(pairs), int(w["table"][:, 1].sum() + w["table"][:, 3].sum())
    w["out"] = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    w["ops"] = torch.empty((total,), dtype=torch.uint8, device="cuda")
    w["spans"] = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    return w


utt_refs = [rng.integers(0, 5000, int(n)).astype(np.int32) for n in rng.integers(20, 201, 4096)]
utt_hyps = [noisy_copy(r, 5000) for r in utt_refs]
ses_refs = [rng.integers(0, 5000, 12000).astype(np.int32) for _ in range(8)]
ses_hyps = [noisy_copy(r, 5000) for r in ses_refs]
own = [(i, i) for i in range(8)]
W = {"utts": workload(utt_refs, utt_hyps, [(i, i) for i in range(4096)], False),
     "session8": workload(ses_refs, ses_hyps, own, False),
     "session8+iv": workload(ses_refs, ses_hyps, own, True),
     "session24": workload(ses_refs, ses_hyps, [(i, (i + d) % 8) for i in range(8) for d in range(3)], False)}


def bind(path):
    """dicow_edit_distance / dicow_edit_alignment (where the library has it) of one library file, or None if the file is missing."""
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    for name, sig, res in (("dicow_edit_distance", L._SIGS["dicow_edit_distance"], L.c_i), ("dicow_edit_distance_ws_bytes", L._SIGS64["dicow_edit_distance_ws_bytes"], L.c_i64),
                           ("dicow_edit_alignment", L._SIGS["dicow_edit_alignment"], L.c_i), ("dicow_edit_alignment_ws_bytes", L._SIGS64["dicow_edit_alignment_ws_bytes"], L.c_i64)):
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = sig, res
    lib.dicow_last_error.restype = C.c_char_p
    return lib


LIBS = {"new": bind(L.LIB_PATH), "parent": bind(os.path.join(ROOT, "tools", "libv_parent.so")),
        "eafwd": bind(os.path.join(ROOT, "tools", "libv_eafwd.so")), "eawalk": bind(os.path.join(ROOT, "tools", "libv_eawalk.so"))}
need = max(LIBS["new"].dicow_edit_alignment_ws_bytes(w["table"].ctypes.data, len(w["table"]), 0, 0) for w in W.values())
assert need > 0, LIBS["new"].dicow_last_error()
WS = torch.empty((need,), dtype=torch.uint8, device="cuda")


def dist(lib, w):
    t = w["table"]
    rc = lib.dicow_edit_distance(w["ref"].data_ptr(), w["ref"].numel(), w["hyp"].data_ptr(), w["hyp"].numel(), L.ptr(w["riv"]), L.ptr(w["hiv"]), t.ctypes.data,
                                 len(t), w["out"].data_ptr(), 0, 0, WS.data_ptr(), lib.dicow_edit_distance_ws_bytes(t.ctypes.data, len(t)), L.stream())
    assert rc == 0, lib.dicow_last_error()


def align(lib, w):
    t = w["table"]
    rc = lib.dicow_edit_alignment(w["ref"].data_ptr(), w["ref"].numel(), w["hyp"].data_ptr(), w["hyp"].numel(), L.ptr(w["riv"]), L.ptr(w["hiv"]), t.ctypes.data,
                                  len(t), w["out"].data_ptr(), w["ops"].data_ptr(), w["spans"].data_ptr(), 0, 0, WS.data_ptr(),
                                  lib.dicow_edit_alignment_ws_bytes(t.ctypes.data, len(t), 0, 0), L.stream())
    assert rc == 0, lib.dicow_last_error()


def host_alignment(ref, hyp, riv=None, hiv=None):
    """The numpy row-scan of tools/bench_edit_distance.py keeping one step code per cell, then the traceback in Python: ((errors, hits), ops)."""
    ref, hyp = ref.astype(np.int64), hyp.astype(np.int64)
    n, m = len(ref), len(hyp)
    ramp = np.arange(m + 1, dtype=np.int64) * UNIT
    prev = ramp.copy()
    codes = np.empty((n, m), np.uint8)
    for i in range(n):
        eq = hyp == ref[i]
        step = np.where(eq, -1, UNIT)
        if riv is not None:
            step = np.where((riv[i, 0] < hiv[:, 1]) & (hiv[:, 0] < riv[i, 1]), step, 1 << 60)
        t = np.empty(m + 1, np.int64)
        t[0] = (i + 1) * UNIT
        t[1:] = np.minimum(prev[1:] + UNIT, prev[:-1] + step)
        cur = np.minimum.accumulate(t - ramp) + ramp
        codes[i] = np.where(prev[:-1] + step == cur[1:], np.where(eq, 0, 1), np.where(prev[1:] + UNIT == cur[1:], 2, 3))
        prev = cur
    e = -(-int(prev[-1]) // UNIT)
    i, j, ops = n, m, []
    while i > 0 and j > 0:
        c = int(codes[i - 1, j - 1])
        ops.append(c)
        i, j = i - (c != 3), j - (c != 2)
    ops += [2] * i + [3] * j
    return (e, e * UNIT - int(prev[-1])), ops[::-1]


def paths_of(w):
    ops, spans = w["ops"].cpu().numpy(), w["spans"].cpu().numpy()
    return [ops[a:a + b] for a, b in spans.tolist()]


# ---- agreement at the timed sizes, which is the warm-up of every arm too
for k, w in W.items():
    dist(LIBS["new"], w)
    torch.cuda.synchronize()
    counts = w["out"].cpu().clone()
    w["out"].fill_(-1)
    align(LIBS["new"], w)
    torch.cuda.synchronize()
    assert torch.equal(w["out"].cpu(), counts), k
    paths = paths_of(w)
    for q, (p, row) in enumerate(zip(paths, w["table"])):
        e, h = int((p != 0).sum()), int((p == 0).sum())
        assert (e, h) == tuple(counts[q].tolist()) and int((p != 3).sum()) == row[1] and int((p != 2).sum()) == row[3], (k, q)
    i, j = w["pairs"][3]
    timed = w["riv"] is not None
    ref_pair = host_alignment(w["refs"][i], w["hyps"][j], w["rivs"][i] if timed else None, w["hivs"][j] if timed else None)
    assert ref_pair == (tuple(counts[3].tolist()), paths[3].tolist()), k
    for name in ("parent", "eafwd", "eawalk"):
        if LIBS[name] is not None:
            w["out"].fill_(-1)
            (dist if name == "parent" else align)(LIBS[name], w)
            torch.cuda.synchronize()
            assert name == "eawalk" or torch.equal(w["out"].cpu(), counts), (k, name)
            assert name != "eawalk" or all(np.array_equal(a, b) for a, b in zip(paths_of(w), paths)), k
    print(f"{k}: {len(paths)} pairs, ops reproduce (errors, hits) of dicow_edit_distance; pair 3 equals the host traceback; errors {int(counts[:, 0].sum())}, "
          f"hits {int(counts[:, 1].sum())}, cells {w['cells']:.3e}, ops {sum(len(p) for p in paths)}")
print("variants missing:", [name for name, lib in LIBS.items() if lib is None] or "none")

ARMS = [("dist.parent", "parent", dist), ("dist.new", "new", dist), ("record", "eafwd", align), ("full", "new", align), ("walk", "eawalk", align)]
ARMS = [a for a in ARMS if LIBS[a[1]] is not None]
ts = {f"{arm}.{k}": [] for k in W for arm, _, _ in ARMS}
ps = PowerSampler(torch.cuda.current_device())
ps.start()
for rnd in range(ROUNDS):
    for k, w in W.items():
        for arm, name, fn in ARMS:                                        # `walk` comes right behind `full`: its records are in WS
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(LIBS[name], w)
            e1.record()
            torch.cuda.synchronize()
            ts[f"{arm}.{k}"].append(e0.elapsed_time(e1))
power = ps.stop()

print(f"tools/bench_edit_alignment.py: {ROUNDS} rounds, arms alternating after a warm-up of all; K={L.EDIT_K}, lanes {L.EDIT_LANES_NARROW} / {L.EDIT_LANES}")
med = {}
for name, v in ts.items():
    k = name.split(".")[-1]
    med[name] = statistics.median(v)
    print(f"{name:24s} median {med[name]:10.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n={len(v)})   {W[k]['cells'] / med[name] / 1e6:9.2f} G cells / s")
for k in W:
    if f"record.{k}" in med:
        print(f"recording on {k}: record - dist.new = {med[f'record.{k}'] - med[f'dist.new.{k}']:+.3f} ms ({med[f'record.{k}'] / med[f'dist.new.{k}']:.3f} x)")
    if f"dist.parent.{k}" in med:
        print(f"dicow_edit_distance on {k}: new / parent = {med[f'dist.new.{k}'] / med[f'dist.parent.{k}']:.4f}")
print("board power over the timed window:", power)

# ---- end to end
words = [f"w{v}" for v in range(5000)]


def segments(streams, prefix):
    """Segments of 20 words, 5 s each, back to back per speaker: a word every 250 ms as above."""
    return [(f"{prefix}{s}", 5.0 * g, 5.0 * g + 5.0, " ".join(words[v] for v in ids[20 * g:20 * g + 20])) for s, ids in enumerate(streams)
            for g in range((len(ids) + 19) // 20)]


ref_segs, hyp_segs = segments(ses_refs, "r"), segments(ses_hyps, "h")
utt_ref_text = [" ".join(words[v] for v in s) for s in utt_refs]
utt_hyp_text = [" ".join(words[v] for v in s) for s in utt_hyps]
for label, fn in (("session_alignment (tcp, collar 5 s)", lambda: scoring.session_alignment(ref_segs, hyp_segs, timed=True, collar=5.0)),
                  ("session_alignment (cp)", lambda: scoring.session_alignment(ref_segs, hyp_segs, timed=False)),
                  ("word_alignments (4096 utterances)", lambda: scoring.word_alignments(utt_ref_text, utt_hyp_text))):
    fn()
    v = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    print(f"end to end: {label:38s} median {statistics.median(v):9.1f} ms (min {min(v):.1f}, max {max(v):.1f}, n=3), host work included")
w = W["session8+iv"]
for label, riv, hiv in (("session, timed", w["rivs"][0], w["hivs"][0]), ("session", None, None)):
    t0 = time.perf_counter()
    host_alignment(ses_refs[0], ses_hyps[0], riv, hiv)
    dt = time.perf_counter() - t0
    print(f"host: {label:16s} {dt * 1e3:10.1f} ms for the scan with codes and the traceback of one 12 000 x 12 000 table: x 8 = {dt * 8e3:.0f} ms for the "
          f"assigned pairs, beside the 64 counts tables of the assignment (profiles/edit_distance.txt: about 35 s / 46 s as numpy row-scans)")
t0 = time.perf_counter()
for i in range(256):
    host_alignment(utt_refs[i], utt_hyps[i])
dt = time.perf_counter() - t0
print(f"host: utterances      {dt * 1e3:10.1f} ms for the first 256 pairs: x 16 = {dt * 16e3:.0f} ms for the 4096")

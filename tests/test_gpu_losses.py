"""The two loss files on the MI355X, kernel by kernel: csrc/loss.hip (fused log-softmax + cross-entropy, hard and soft-label paths)
and csrc/ctc.hip (CTC forward / backward) through ops.ce_args / ops.ctc_args against the fp64 references of tests/loss_ref.py, at
the shapes and label patterns where such kernels go wrong: repeated labels, infeasible and empty targets, the longest target the
kernel takes, colliding keys in the posterior hash table, peaked logits, every vector / tail split of the CE row loop, exact ties,
one label set ignored, timestamp (soft) targets, out-of-range labels.  Every case runs inside poison (inputs) and guard bands
(outputs) and must equal, bit for bit, the same call on exactly sized, unpoisoned buffers.  Run with `pytest -m gpu`.

Bounds (measured against the fp64 references on the MI355X, per case, in profiles/loss_kernels.txt):
  fp32 outputs (lse, row_loss, nll, the losses)   |got - ref| <= FP32_TOL * max(1, |ref|)
  d_logits (bf16)                                 |got - scale * ref| <= 2^-8 |scale * ref| + A * scale
The first term of the gradient bound is one bf16 rounding of the stored value; FP32_TOL and A are 4 x the worst measured figure
(fast-math __expf / __logf error depends on the data) and stay below what tests/test_gpu_fullsize.py allows (2e-3 and 1e-2)."""
import types

import pytest
import torch

import amd_pkg
from tests.loss_ref import ce_ref, ctc_enumerate, ctc_ref, tiny_ctc_inputs
from tests.util import guarded, poisoned

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
bf = torch.bfloat16

# profiles/loss_kernels.txt holds the measured figures, case by case.  Worst fp32 deviation: 4.140e-07 (nll of "ctc longest");
# worst gradient residual beyond the bf16 term: CTC 5.737e-06 ("ctc peaked"), CE 1.886e-13 (V = 2055, soft: the CE gradient is one
# bf16 rounding of the fp64 value everywhere except where a probability or a timestamp weight underflows).  Each bound is 4 x that.
FP32_TOL = 1.6e-6
A_CE = 7.5e-13
A_CTC = 2.2e-5
KINDS = ("nan", "big")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


def _note(case, what, value):
    """One measured figure per line (pytest -s shows them; profiles/loss_kernels.txt was collected from these lines)."""
    print(f"loss_kernels: {case:<28s} {what:<12s} {value:.3e}")


def _out(shape, ld, dtype, name, padded):
    """An output buffer: inside guard bands (padded) or exactly sized; .view is what the kernel gets, .check() the guard test."""
    if padded:
        return guarded(shape, ld, dtype, name=name)
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int16).fill_(0x7FC1)
    return types.SimpleNamespace(view=t, check=lambda: None)


def _rel(got, ref):
    """worst |got - ref| / max(1, |ref|) (NaN if anything is NaN: every `< bound` then fails)."""
    got, ref = got.double().cpu().reshape(-1), ref.double().reshape(-1)
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _grad_resid(got, ref, scale):
    """worst (|got - scale * ref| - 2^-8 |scale * ref|) / scale: what the constant A of the gradient bound has to cover."""
    r = ref.double() * scale
    return max(0.0, float(((got.double().cpu() - r).abs() - 2.0 ** -8 * r.abs()).max())) / scale


# ================================================================================================ CTC
CTC_SCALES = (1.0, 0.3)


def _ctc_call(ops, z, lab, ld, kind):
    """dicow_ctc_loss_fwd + _bwd (at both grad scales) on z (CPU bf16 [B, Tn, C]) and lab (CPU int64 [B, Lc]).  kind "nan" / "big":
    logits inside that poison with row stride ld, every output inside guard bands; kind None: exactly sized, zero-padded buffers.
    Returns the outputs as CPU tensors; the guards are checked here."""
    B, Tn, C = z.shape
    rows, Smax = B * Tn, 2 * lab.shape[1] + 1
    padded = kind is not None
    if padded:
        logits = poisoned(z.reshape(rows, C), ld, kind=kind)
    else:
        ld = C + (C & 1)
        logits = torch.zeros(rows, ld, dtype=bf, device="cuda")
        logits[:, :C] = z.reshape(rows, C).cuda()
    labd = lab.cuda().contiguous()
    o = {"lse": _out((rows,), 64, torch.float32, "lse", padded), "nll": _out((B,), 64, torch.float32, "nll", padded),
         "tlen": _out((B,), 64, torch.float32, "tlen", padded), "alpha": _out((rows, Smax), Smax, torch.float32, "alpha", padded),
         "beta": _out((rows, Smax), Smax, torch.float32, "beta", padded)}
    for s in CTC_SCALES:
        o[f"d{s}"] = _out((rows, ld), ld, bf, f"d_logits@{s}", padded)
    acc = torch.zeros(1, device="cuda")
    a = ops.ctc_args(logits, ld, B, Tn, C, labd, o["lse"].view, o["alpha"].view, o["beta"].view, o["nll"].view, o["tlen"].view, acc)
    ops.ctc_loss_fwd(a)
    for s in CTC_SCALES:
        a.d_logits = o[f"d{s}"].view.data_ptr()
        ops.ctc_loss_bwd(a, torch.full((1,), s, device="cuda"))
    torch.cuda.synchronize()
    for g in o.values():
        g.check()
    res = {k: g.view.cpu().clone() for k, g in o.items()}
    res["loss_sum"] = acc.cpu()
    for s in CTC_SCALES:
        d = res.pop(f"d{s}")
        assert float(d[:, C:].float().abs().max() if ld > C else 0.0) == 0.0, "d_logits pad columns must be exactly zero"
        res[f"d{s}"] = d[:, :C].contiguous()
    return res


def _bits_equal(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                                                  y.view(torch.int16 if y.element_size() == 2 else torch.int32)), f"{what}: {k} differs"


def _ctc_case(ops, name, z, lab, ld, enum=False):
    """Run the case poisoned (both kinds) and exact, require bit-equality, check against the fp64 reference(s)."""
    B, Tn, C = z.shape
    zb = z.bfloat16()
    runs = [_ctc_call(ops, zb, lab, ld, k) for k in KINDS] + [_ctc_call(ops, zb, lab, ld, None)]
    for r, k in zip(runs[1:], ("big", "exact")):
        _bits_equal(runs[0], r, f"{name}: nan-poisoned vs {k}")
    got = runs[0]
    refs = [ctc_ref(zb.double(), lab)] + ([ctc_enumerate(zb.double(), lab)] if enum else [])
    for ref in refs:
        feasible = torch.isfinite(ref["nll"])
        assert got["tlen"].tolist() == [float(t) for t in ref["target_len"]]
        assert torch.isposinf(got["nll"][~feasible]).all() and torch.isfinite(got["nll"][feasible]).all()
        e_lse = _rel(got["lse"], torch.logsumexp(zb.double(), -1))
        e_nll = _rel(got["nll"][feasible], ref["nll"][feasible])
        e_loss = _rel(got["loss_sum"] / B, ref["loss"])
        _note(name, "lse", e_lse), _note(name, "nll", e_nll), _note(name, "loss", e_loss)
        assert e_lse < FP32_TOL and e_nll < FP32_TOL and e_loss < FP32_TOL, (e_lse, e_nll, e_loss)
        assert torch.isfinite(got["alpha"]).all() and torch.isfinite(got["beta"]).all()
        for s in CTC_SCALES:
            d = got[f"d{s}"].float().view(B, Tn, C)
            assert torch.isfinite(d).all()
            assert float(d[~feasible].abs().max() if (~feasible).any() else 0.0) == 0.0, "an infeasible utterance has gradient 0"
            a = _grad_resid(d, ref["grad"], s)
            _note(name, f"A@{s}", a)
            assert a < A_CTC, (s, a)
    return got, refs[0]


def _ragged(lab, lens):
    for b, n in enumerate(lens):
        lab[b, n:] = -100
    return lab


def test_ctc_tiny_vs_torch_and_enumeration(ops):
    """B = 5, T = 6, C = 5, ld = 6: a repeat, an infeasible row, an empty row, alternating labels, a short repeat."""
    z, lab = tiny_ctc_inputs()
    got, ref = _ctc_case(ops, "ctc tiny", z, lab, 6, enum=True)
    assert float(ref["grad"][2].abs().max()) > 1e-3 and float(got["d1.0"].float().view(5, 6, 5)[2].abs().max()) > 1e-3


def _count_repeats(row):
    v = [int(c) for c in row if c >= 0]
    return len(v), sum(1 for i in range(1, len(v)) if v[i] == v[i - 1])


def test_ctc_repeated_labels(ops):
    """B = 8, Tn = 50, C = 7 (odd, ld = 8), Lc = 20, labels from 3 classes: about a third of the neighbours repeat, so the
    no-skip-between-equal-labels branches of both recursions decide the result.  One row is empty."""
    g = torch.Generator().manual_seed(21)
    z = torch.randn(8, 50, 7, generator=g) * 2
    lab = _ragged(torch.randint(0, 3, (8, 20), generator=g), [20, 17, 20, 0, 11, 20, 5, 19])
    reps = sum(_count_repeats(r)[1] for r in lab)
    assert reps >= 25, reps
    got, ref = _ctc_case(ops, "ctc repeats", z, lab, 8)
    assert torch.isfinite(ref["nll"]).all()


def test_ctc_repeats_single_alignment_and_one_frame_short(ops):
    """Tn = 50 again, Lc = 26 (Lc = 20 cannot reach 50 frames: 20 labels + 19 repeats = 39): a row with tl + repeats == Tn exactly
    (one alignment: the posterior is one-hot), a row with tl + repeats == Tn + 1 (infeasible by one frame), an empty row."""
    g = torch.Generator().manual_seed(22)
    z = torch.randn(4, 50, 7, generator=g) * 2
    single = [0] * 13 + [1] * 13                      # 26 labels, 12 + 12 = 24 repeats: 50 frames
    short = [2] * 26                                   # 26 labels, 25 repeats: 51 frames
    lab = torch.tensor([single, short, [-100] * 26, [0, 1] * 13])
    assert _count_repeats(lab[0]) == (26, 24) and _count_repeats(lab[1]) == (26, 25)
    got, ref = _ctc_case(ops, "ctc repeats forced", z, lab, 8)
    assert torch.isfinite(ref["nll"]).tolist() == [True, False, True, True]
    # the single alignment: nll is minus the sum of its frames' log-probabilities
    lp = torch.log_softmax(z.bfloat16().double()[0], -1)
    path = []
    for i, c in enumerate(single):
        path += ([6] if i and single[i - 1] == c else []) + [c]
    assert len(path) == 50 and abs(float(ref["nll"][0]) + float(lp[torch.arange(50), torch.tensor(path)].sum())) < 1e-9


def test_ctc_longest_target(ops):
    """B = 2, Tn = 1100, Lc = 511, C = 601: Smax = 1023 states, the kernel's limit.  Row 0: 511 distinct classes (512 keys in the
    posterior table), row 1: labels from 2 classes (about 255 repeats)."""
    g = torch.Generator().manual_seed(23)
    z = torch.randn(2, 1100, 601, generator=g) * 2
    lab = torch.stack((torch.randperm(600, generator=g)[:511], torch.randint(0, 2, (511,), generator=g) * 300 + 7))
    assert _count_repeats(lab[0]) == (511, 0) and _count_repeats(lab[1])[1] > 200
    _ctc_case(ops, "ctc longest", z, lab, 608)


def test_ctc_refuses_more_labels_than_states(ops):
    """Lc = 512 (Smax = 1025 > 1024 threads) is refused with the library's error and writes nothing."""
    from ts_asr_whisper_amd import _lib as L
    B, Tn, C, Lc, ld = 2, 1100, 601, 512, 608
    rows, Smax = B * Tn, 2 * Lc + 1
    logits = torch.zeros(rows, ld, dtype=bf, device="cuda")
    lab = torch.zeros(B, Lc, dtype=torch.long, device="cuda")
    o = [guarded((rows,), 64, torch.float32, name="lse"), guarded((rows, Smax), Smax, torch.float32, name="alpha"),
         guarded((rows, Smax), Smax, torch.float32, name="beta"), guarded((B,), 64, torch.float32, name="nll"),
         guarded((B,), 64, torch.float32, name="tlen"), guarded((1,), 64, torch.float32, name="loss_sum"),
         guarded((rows, ld), ld, bf, name="d_logits")]
    a = ops.ctc_args(logits, ld, B, Tn, C, lab, o[0].view, o[1].view, o[2].view, o[3].view, o[4].view, o[5].view)
    with pytest.raises(L.DicowError, match="at most 511 labels"):
        L.call_struct("dicow_ctc_loss_fwd", a)
    a.d_logits = o[6].view.data_ptr()
    with pytest.raises(L.DicowError, match="at most 511 labels"):
        ops.ctc_loss_bwd(a, torch.ones(1, device="cuda"))
    torch.cuda.synchronize()
    for g in o:
        g.check()
        assert g.untouched_inside() == g.view.numel(), g.name


def test_ctc_colliding_posterior_keys(ops):
    """C = 1200: the classes (4, 991), (19, 1006), (34, 1021), (49, 1036), (64, 1051) share a home slot of the posterior table
    pairwise (the table hashes class c to (c * 2654435761 mod 2^32) >> 21; up to C = 991 no two classes do (4 and 991 are the first pair), so the longest case
    has none), so one key of each pair sits in a probed slot.  Row 1 holds only one key of three pairs: a class that is NOT a
    label finds a foreign key in its home slot and has to come out with posterior 0."""
    g = torch.Generator().manual_seed(24)
    z = torch.randn(2, 30, 1200, generator=g) * 2
    lab = torch.tensor([[4, 991, 19, 1006, 34, 1021, 49, 1036, 4, 991, 64, 1051],
                        [1051, 64, 1036, 1021, 19, 991, 991, -100, -100, -100, -100, -100]])
    _ctc_case(ops, "ctc collisions", z, lab, 1216)


def test_ctc_peaked_logits(ops):
    """B = 4, Tn = 64, C = 33, Lc = 12, logits x 12: single alignments sit hundreds of nats down; the -1e30 sentinel arithmetic
    and exp(alpha + beta - lp + nll) must stay finite and right."""
    g = torch.Generator().manual_seed(25)
    z = torch.randn(4, 64, 33, generator=g) * 2 * 12
    lab = _ragged(torch.randint(0, 32, (4, 12), generator=g), [12, 7, 12, 1])
    got, ref = _ctc_case(ops, "ctc peaked", z, lab, 40)
    assert float(ref["nll"].min()) > 100.0


def test_ctc_one_frame(ops):
    """Tn = 1 with 0, 1 and 2 labels: -log p(blank), -log p(label), infeasible."""
    g = torch.Generator().manual_seed(26)
    z = torch.randn(3, 1, 6, generator=g) * 2
    lab = torch.tensor([[-100, -100], [3, -100], [1, 2]])
    got, ref = _ctc_case(ops, "ctc one frame", z, lab, 8)
    assert torch.isfinite(ref["nll"]).tolist() == [True, True, False]


def test_ctc_all_infeasible(ops):
    """Every row infeasible: loss 0, d_logits all zero, no NaN anywhere."""
    g = torch.Generator().manual_seed(27)
    z = torch.randn(3, 3, 6, generator=g) * 2
    lab = torch.tensor([[1, 1, 2, -100], [0, 1, 2, 3], [2, 2, 2, -100]])
    got, ref = _ctc_case(ops, "ctc all infeasible", z, lab, 8)
    assert float(got["loss_sum"]) == 0.0 and float(ref["loss"]) == 0.0
    assert all(float(got[f"d{s}"].float().abs().max()) == 0.0 for s in CTC_SCALES)


def test_ctc_loss_sum_is_ordered(ops):
    """B = 64, Tn = 40, Lc ragged from 0 to 12: ten forward calls give a bit-identical loss_sum (one workgroup adds the
    utterances up in index order), and it is the fp64 sum of the returned nll / max(tlen, 1)."""
    g = torch.Generator().manual_seed(28)
    B, Tn, C, Lc = 64, 40, 20, 12
    z = (torch.randn(B, Tn, C, generator=g) * 2).bfloat16()
    lab = _ragged(torch.randint(0, C - 1, (B, Lc), generator=g), [b % 13 for b in range(B)])
    logits = z.reshape(B * Tn, C).cuda()
    labd = lab.cuda()
    lse, nll, tlen = torch.empty(B * Tn, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ab = torch.empty(2, B * Tn, 2 * Lc + 1, device="cuda")
    sums = []
    for _ in range(10):
        acc = torch.zeros(1, device="cuda")
        ops.ctc_loss_fwd(ops.ctc_args(logits, C, B, Tn, C, labd, lse, ab[0], ab[1], nll, tlen, acc))
        sums.append(acc.cpu())
    assert all(torch.equal(s.view(torch.int32), sums[0].view(torch.int32)) for s in sums), [float(s) for s in sums]
    n, t = nll.double().cpu(), tlen.double().cpu()
    assert torch.isfinite(n).all() and t.tolist() == [float(b % 13) for b in range(B)]
    want = float((n / t.clamp(min=1.0)).sum())
    e = abs(float(sums[0]) - want) / max(1.0, abs(want))
    _note("ctc ordered sum", "loss_sum", e)
    assert e < FP32_TOL
    # accumulated into loss_sum, as documented
    acc = torch.full((1,), 2.5, device="cuda")
    ops.ctc_loss_fwd(ops.ctc_args(logits, C, B, Tn, C, labd, lse, ab[0], ab[1], nll, tlen, acc))
    assert abs(float(acc) - 2.5 - want) < FP32_TOL * max(1.0, abs(want))


# ================================================================================================ CE
CE_SCALE = 0.7
CE_WIDTHS = {5: 0, 8: 0, 300: 50, 2055: 355}          # V -> timestamp ids (the last n of the vocabulary)


def _ts_vocab(V, n_ts):
    vocab = {f"tok{i}": i for i in range(V - n_ts)}
    vocab.update({f"<|{0.02 * j:.2f}|>": V - n_ts + j for j in range(n_ts)})
    return vocab


def _ts_tables(V):
    """(tables on the GPU as ops.ce_args takes them, the same as ce_ref takes them), or (None, None) without timestamp ids."""
    from ts_asr_whisper_amd.modeling import build_ts_tables
    n_ts = CE_WIDTHS[V]
    if not n_ts:
        return None, None
    ts = build_ts_tables(_ts_vocab(V, n_ts), V, "cuda")
    assert ts["ids"].numel() == n_ts and ts["ids"].tolist() == list(range(V - n_ts, V))
    return ts, (ts["ids"].long().cpu(), ts["w"].double().cpu())


def _ce_rows(V):
    """About a dozen rows (more with timestamp ids): every logit pattern and every label pattern of the issue.
    Returns (logits fp32 [R, V] (bf16-exact), labels [R], upp_labels [R])."""
    n_ts = CE_WIDTHS[V]
    nt = V - n_ts                                                    # ordinary ids are [0, nt)
    g = torch.Generator().manual_seed(100 + V)
    a, b = 1, nt - 2                                                 # two different ordinary labels (1 and 3 at V = 5)
    rows = []

    def gauss():
        return (torch.randn(V, generator=g) * 2).bfloat16().float()

    rows += [(gauss(), a, b), (gauss(), a, a), (gauss(), a, -100), (gauss(), -100, b), (gauss(), -100, -100)]
    tie = gauss()
    tie[b] = tie[a]                                                  # an exact tie between two different labels
    rows.append((tie, a, b))
    rows += [(torch.full((V,), 0.75), a, b), (torch.full((V,), 0.75), b, -100)]
    hots = [h for h in (0, 7, 8, V - 1) if h < V]
    for i, h in enumerate(dict.fromkeys(hots)):
        z = torch.full((V,), -80.0)
        z[h] = 80.0
        o = (h + 3) % V
        rows.append((z, h, o) if i % 2 == 0 else (z, o, h))
    z = torch.full((V,), -80.0)
    z[V - 1] = 80.0
    rows.append((z, V - 1, -100))
    if n_ts:
        t0, tm, tl = nt, nt + n_ts // 2, V - 1                       # both ends of the timestamp table and its middle
        rows += [(gauss(), t0, a), (gauss(), a, tl), (gauss(), tm, tm + 3), (gauss(), tl, t0), (gauss(), tm, -100), (gauss(), t0, t0)]
    return torch.stack([r[0] for r in rows]), torch.tensor([r[1] for r in rows]), torch.tensor([r[2] for r in rows])


def _ce_call(ops, z, lab, upp, soft, ts, V, ld, kind):
    """dicow_ce_loss_fwd + _bwd on z (CPU bf16 [R, V]); kind as in _ctc_call.  Returns the outputs as CPU tensors."""
    R = z.shape[0]
    padded = kind is not None
    if padded:
        logits = poisoned(z, ld, kind=kind)
    else:
        ld = (V + 7) // 8 * 8
        logits = torch.zeros(R, ld, dtype=bf, device="cuda")
        logits[:, :V] = z.cuda()
    o = {"lse": _out((R,), 64, torch.float32, "lse", padded), "row_loss": _out((R,), 64, torch.float32, "row_loss", padded),
         "choice": _out((R,), 64, torch.int32, "choice", padded), "d": _out((R, ld), ld, bf, "d_logits", padded)}
    acc = torch.zeros(2, device="cuda")
    labd, uppd, scale = lab.cuda(), None if upp is None else upp.cuda(), torch.full((1,), CE_SCALE, device="cuda")
    a = ops.ce_args(logits, ld, R, V, labd, uppd, soft, ts, o["lse"].view, o["row_loss"].view, o["choice"].view, acc[0:1], acc[1:2],
                    o["d"].view)                       # (the struct holds raw pointers: every operand stays referenced until the sync)
    ops.ce_loss_fwd(a)
    ops.ce_loss_bwd(a, scale)
    torch.cuda.synchronize()
    for g in o.values():
        g.check()
    res = {k: g.view.cpu().clone() for k, g in o.items()}
    res["acc"] = acc.cpu()
    d = res.pop("d")
    assert float(d[:, V:].float().abs().max() if ld > V else 0.0) == 0.0, "d_logits pad columns must be exactly zero"
    res["d"] = d[:, :V].contiguous()
    return res


def _ce_check(name, got, ref):
    e_lse, e_row = _rel(got["lse"], ref["lse"]), _rel(got["row_loss"], ref["row_loss"])
    e_sum = _rel(got["acc"][0], ref["row_loss"].sum())
    a = _grad_resid(got["d"].float(), ref["grad"], CE_SCALE)
    _note(name, "lse", e_lse), _note(name, "row_loss", e_row), _note(name, "loss_sum", e_sum), _note(name, f"A@{CE_SCALE}", a)
    assert e_lse < FP32_TOL and e_row < FP32_TOL and e_sum < FP32_TOL, (e_lse, e_row, e_sum)
    assert float(got["acc"][1]) == ref["count"]
    # the choice is checked on every row: each is an exact tie by construction (gap 0: lower set) or decided by a wide margin
    gap = (ref["l1"] - ref["l2"]).abs()
    assert bool(((gap == 0) | (gap > 1e-2)).all()), gap
    assert got["choice"].tolist() == ref["choice"].tolist()
    assert torch.isfinite(got["d"].float()).all() and a < A_CE, a


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("V", sorted(CE_WIDTHS))
def test_ce_edges_vs_fp64(ops, V, soft, pad):
    """V = 5 runs the scalar tail only, 8 one vector and no tail, 300 both, 2055 a second trip of the 256 x 8 vector loop and a
    7-element tail; ld = V rounded up to 8, plus 64 pad columns in the second layout.  With timestamp ids (V = 300: 50, V = 2055:
    355 > 256, a second trip of the timestamp dot product) the soft path sees timestamp labels in either set or both."""
    z, lab, upp = _ce_rows(V)
    zb = z.bfloat16()
    ts, ts_ref = _ts_tables(V) if soft else (None, None)
    ld = (V + 7) // 8 * 8 + pad
    name = f"ce V={V} {'soft' if soft else 'hard'} ld={ld}"
    for u, tag in ((upp, ""), (None, " upp=None")):
        runs = [_ce_call(ops, zb, lab, u, soft, ts, V, ld, k) for k in KINDS] + [_ce_call(ops, zb, lab, u, soft, ts, V, ld, None)]
        for r, k in zip(runs[1:], ("big", "exact")):
            _bits_equal(runs[0], r, f"{name}{tag}: nan-poisoned vs {k}")
        ref = ce_ref(zb.double(), lab, u, soft, ts_ref)
        _ce_check(name + tag, runs[0], ref)
        if u is not None and not soft:
            # lower valid, upper ignored: loss 0 and gradient 0; the same on the soft path competes as token 0
            assert float(runs[0]["row_loss"][2]) == 0.0 and float(runs[0]["d"][2].float().abs().max()) == 0.0
        if u is not None and soft:
            assert float(ref["row_loss"][2]) > 0.0 and float(runs[0]["row_loss"][2]) > 0.0


@pytest.mark.parametrize("V,soft", [(8, False), (300, True)])
def test_ce_out_of_range_labels_poison_the_loss(ops, V, soft):
    """Labels V and -1 in either set: the row loss and the step's loss are NaN (loss.hip's comment), the other rows are
    untouched.  The finite poison sits where an unclamped read would land (the row pad, the previous row's pad / the lead guard,
    spare entries around the timestamp lookup), so a kernel that read there would produce a wrong finite number, not a fault."""
    g = torch.Generator().manual_seed(200 + V)
    R, ld = 8, (V + 7) // 8 * 8 + 64
    zb = (torch.randn(R, V, generator=g) * 2).bfloat16()
    lab = torch.tensor([1, V, 2, 3, -1, 1, 2, 3])
    upp = torch.tensor([2, 1, V, 3, 2, -1, -100, 0])
    bad = torch.tensor([False, True, True, False, True, True, False, False])
    ts, ts_ref = _ts_tables(V) if soft else (None, None)
    if ts is not None:
        spare = torch.full((V + 16,), -1, dtype=torch.int32, device="cuda")
        spare[8:8 + V] = ts["index"]
        ts = dict(ts, index=spare[8:8 + V])
    got = _ce_call(ops, zb, lab, upp, soft, ts, V, ld, "big")
    assert torch.isnan(got["row_loss"][bad]).all() and torch.isfinite(got["row_loss"][~bad]).all()
    assert bool(torch.isnan(got["acc"][0]))
    ok = ce_ref(zb.double(), torch.where(bad, -100, lab), torch.where(bad, -100, upp), soft, ts_ref)
    assert _rel(got["lse"], ok["lse"]) < FP32_TOL
    assert _rel(got["row_loss"][~bad], ok["row_loss"][~bad]) < FP32_TOL
    assert got["choice"][~bad].tolist() == ok["choice"][~bad].tolist()
    assert torch.isfinite(got["d"].float()).all()
    a = _grad_resid(got["d"][~bad].float(), ok["grad"][~bad], CE_SCALE)
    _note(f"ce V={V} out of range", "row_loss", _rel(got["row_loss"][~bad], ok["row_loss"][~bad]))
    _note(f"ce V={V} out of range", f"A@{CE_SCALE}", a)
    assert a < A_CE, a

"""The small HBM-bound kernels every training step passes through (csrc/elementwise.hip and the full-FDDT combine of
csrc/fddt_ln.hip), one by one on the MI355X against the references of tests/glue_ref.py, at the sizes where such kernels go wrong:
every vector / scalar-tail split, one element, sizes just past each launcher's grid cap (so that the grid-stride loop takes a second
pass and then the tail), both paths of the partial-sum reduction with each loop remainder, the first and last frame of the col2im
scatter.  Outputs sit in guard bands, strided inputs in NaN and in finite poison, and every result must equal, bit for bit, the same
call on exactly sized buffers.  Run with `pytest -m gpu`.

Three kinds of bound; each test's docstring names its own:
  E  exact: the result is determined bit for bit and compared through an integer view with an emulation in torch on the CPU.
  S  summation: fp32 sums in an order the test does not assume, |got - ref64| <= (n - 1) 2^-24 sum|terms| + 2^-24 |ref64|
     (glue_ref.sum_bound: derived, not measured); the worst fraction of the bound that was used is printed.
  M  measured: device tanhf / the GELU polynomial of common.h.  bf16 outputs |got - ref64| <= 2^-8 |ref64| + A, fp32 outputs
     <= A max(1, |ref64|), A = 4 x the worst residual measured on the MI355X per kernel (profiles/glue_kernels.txt)."""
import pytest
import torch

import amd_pkg
from tests import glue_ref as R
from tests.util import SENTINEL16, guarded, hashed_stno, poisoned, sketch, subsample

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
bf, f32 = torch.bfloat16, torch.float32
KINDS = ("nan", "big")
U = R.U

# profiles/glue_kernels.txt (pytest tests/test_gpu_glue_kernels.py -m gpu -s) holds the measured figures, case by case.  Worst
# residual beyond the bf16 term: gelu_bwd_bf16 9.295e-09 (n = 1028, g = 1), conv2_col2im_gelu_bwd 3.973e-08 ((2, 50, 384): up to
# two gradients of about 2 and 4 meet there), scb_gate_bwd's d_upd 0 (every case: one fp32 tanhf and one product lie well inside a
# bf16 rounding).  Worst fp32 deviation: scb_merge_fwd 1.730e-07 ((3, 175, 4000), gate -4), the factor 1 - tanh(gate)^2 5.759e-08
# (gate -4).  Each bound is 4 x that.
A_GELU_BWD = 3.8e-8
A_COL2IM = 1.6e-7
A_MERGE_FWD = 7.0e-7
A_GATE_DUPD = 0.0
A_GATE_FACTOR = 2.4e-7

SCB_SHAPES = [(1, 1, 4), (2, 5, 12), (3, 175, 4000)]          # the last: 2051 blocks of float4 work, past the 2048-block cap
GATES = (0.0, 0.3, -4.0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from ts_asr_whisper_amd import _lib
    return _lib


def _note(case, what, value):
    """One measured figure per line (pytest -s shows them; profiles/glue_kernels.txt was collected from these lines)."""
    print(f"glue_kernels: {case:<44s} {what:<14s} {value:.3e}")


def _sentinel_rows(t):
    """Per element of a 2- / 4-byte tensor: True where every 16-bit word still holds the guard sentinel."""
    w = t.contiguous().view(torch.int16).view(t.numel(), -1)
    return (w == SENTINEL16).all(1)


class _Plain:
    """An exactly sized output (the run the guarded ones must equal): sentinel-filled like a guarded view, no bands."""

    def __init__(self, shape, dtype, init):
        self.view = torch.empty(shape, dtype=dtype, device="cuda")
        self.view.view(torch.int16).fill_(SENTINEL16)
        if init is not None:
            self.view.copy_(init.to(dtype))

    def check(self):
        pass

    def untouched_inside(self):
        return int(_sentinel_rows(self.view).sum())


def _out(shape, dtype, name, padded, init=None, ld=None):
    """An output buffer: inside guard bands (padded) or exactly sized; .view is what the kernel gets, .check() the guard test."""
    shape = tuple(shape)
    if not padded:
        return _Plain(shape, dtype, init)
    ld = ld if ld is not None else (shape[-1] if len(shape) == 2 else 64)
    return guarded(shape, ld, dtype, name=name, init=None if init is None else init.reshape(shape))


def _finish(outs, overwritten=True):
    """Synchronise, check every guard band, (outputs that are overwritten: no sentinel left inside), return CPU copies."""
    torch.cuda.synchronize()
    res = {}
    for k, o in outs.items():
        o.check()
        if overwritten:
            assert o.untouched_inside() == 0, f"{k}: {o.untouched_inside()} elements never written"
        res[k] = o.view.cpu().clone()
    return res


def _bits_equal(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(R.bits(a[k]), R.bits(b[k])), f"{what}: {k} differs"


def _same(run, variants, what):
    """run(variant) for every variant (the last is the exactly sized one); all results bit-equal; returns the first."""
    res = [run(v) for v in variants]
    for r, v in zip(res[1:], variants[1:]):
        _bits_equal(res[0], r, f"{what}: {variants[0]} vs {v}")
    return res[0]


def _exact(got, want, what):
    ok = torch.equal(R.bits(got), R.bits(want))
    if not ok:
        bad = torch.nonzero(R.bits(got).reshape(-1) != R.bits(want).reshape(-1)).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i].float())!r}, want {float(want.reshape(-1)[i].float())!r}")


def _resid_bf16(got, ref):
    """worst (|got - ref| - 2^-8 |ref|), at least 0: what the constant A of a bf16 output's bound has to cover (NaN stays NaN)."""
    d = (got.double().reshape(-1) - ref.double().reshape(-1)).abs() - 2.0 ** -8 * ref.double().reshape(-1).abs()
    m = float(d.max())
    return m if m != m else max(0.0, m)


def _rel32(got, ref):
    """worst |got - ref| / max(1, |ref|)."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _frac(got, ref, bound):
    """worst |got - ref| / bound over the elements (0 / 0 counts as 0; NaN stays NaN so that `<= 1` fails)."""
    d = (got.double() - ref.double()).abs().reshape(-1)
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref).reshape(-1)
    f = torch.where((d == 0) & (b == 0), torch.zeros_like(d), d / b)
    return float(f.max()) if not bool(torch.isnan(f).any()) else float("nan")


# ================================================================================================ casts and packs
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1027, 4194304 + 1027])
def test_cast_bf16(ops, n):
    """E.  n = 1, 3: the scalar tail alone; 4: one vector; 5, 1023, 1027: both; 4 194 304 + 1 027: 4097 blocks of vector work on a
    4096-block grid (a second grid-stride pass) and a 3-element tail.  Ties in both parities, +-0, denormals, +-inf and the
    largest finite values sit in front and in the tail; a NaN input must give a NaN."""
    x = R.cast_values(n)
    nanpos = sorted({n // 2, n - 3}) if n >= 3 else []           # (n - 3: the first element of a 3-element tail)
    for i, p in enumerate(nanpos):
        x[p:p + 1] = torch.tensor([0x7FC00000, 0xFFC00001][i], dtype=torch.int64).to(torch.int32).view(f32)
    xd = x.cuda()

    def run(padded):
        o = _out((n,), bf, "cast", padded)
        ops.cast_bf16(xd, out=o.view)
        return _finish({"y": o})

    got = _same(run, (True, False), f"cast n={n}")["y"]
    want = x.to(bf)
    keep = torch.ones(n, dtype=torch.bool)
    for p in nanpos:
        assert bool(torch.isnan(got[p].float())), f"NaN input at {p} gave {float(got[p])}"
        keep[p] = False
    _exact(got[keep], want[keep], f"cast n={n}")


@pytest.mark.parametrize("B,M,Tin", [(2, 80, 65), (1, 128, 1), (3, 5, 130), (1, 64, 64)])
def test_mel_to_timemajor(ops, B, M, Tin):
    """E.  65 and 130 frames: a second / third 64-frame tile with one or two frames; 128 x 1: one frame; 64 x 64: exactly one tile.
    The whole [B, Tin + 2, M] output starts as sentinel and ends with none left (the two zero rows are written too)."""
    mel = R.rand((B, M, Tin), 100 + Tin, 1.5)
    md = mel.cuda()

    def run(padded):
        o = _out((B * (Tin + 2), M), bf, "timemajor", padded)
        ops.mel_to_timemajor(md, out=o.view)
        return _finish({"y": o})

    got = _same(run, (True, False), "mel_to_timemajor")["y"]
    _exact(got.view(B, Tin + 2, M), R.mel_timemajor_ref(mel), "mel_to_timemajor")


CONV_SHAPES = [(6, 5, 15), (6, 5, 24), (520, 680, 2048)]       # the last: 1 064 960 elements, past 4096 blocks x 256 threads


@pytest.mark.parametrize("which", ["dst", "dst_t", "both"])
@pytest.mark.parametrize("O,C,Kpad", CONV_SHAPES)
def test_conv_weight_pack(L, O, C, Kpad, which):
    """E.  Kpad = 3 C (no padding), Kpad > 3 C (zero columns), and a weight past the grid cap; the plain copy, the transposed copy
    and both from one launch."""
    w = R.rand((O, C, 3), 110 + C, 0.5)
    wd = w.cuda()

    def run(padded):
        o = {}
        if which != "dst_t":
            o["dst"] = _out((O, Kpad), bf, "dst", padded)
        if which != "dst":
            o["dst_t"] = _out((Kpad, O), bf, "dst_t", padded)
        L.call("dicow_conv_weight_pack", wd.data_ptr(), L.ptr(o["dst"].view) if "dst" in o else None,
               L.ptr(o["dst_t"].view) if "dst_t" in o else None, O, C, Kpad, L.stream())
        return _finish(o)

    got = _same(run, (True, False), "conv_weight_pack")
    want = R.conv_pack_ref(w, Kpad)
    if "dst" in got:
        _exact(got["dst"], want, "conv_weight_pack dst")
    if "dst_t" in got:
        _exact(got["dst_t"], want.t().contiguous(), "conv_weight_pack dst_t")


@pytest.mark.parametrize("O,C,Kpad", CONV_SHAPES)
def test_conv_weight_unpack_grad(ops, O, C, Kpad):
    """E (one fp32 add per element).  g_w is non-zero beforehand; the padded columns of g_packed hold poison and are ignored."""
    gp = R.rand((O, Kpad), 120 + C, 1.0)
    gw0 = R.rand((O, C, 3), 121 + C, 1.0)

    def run(kind):
        g = gp.clone()
        if kind == "nan":
            g[:, 3 * C:] = float("nan")
        elif kind == "big":
            g[:, 3 * C:] = 3.0e4
        else:
            g[:, 3 * C:] = 0.0
        gd = g.cuda()
        o = _out((O * C * 3,), f32, "g_w", kind is not None, init=gw0.reshape(-1))
        ops.conv_weight_unpack_grad(gd, o.view.view(O, C, 3))
        return _finish({"g_w": o})

    got = _same(run, KINDS + (None,), "conv_weight_unpack_grad")["g_w"]
    _exact(got.view(O, C, 3), R.conv_unpack_ref(gw0, gp), "conv_weight_unpack_grad")


# ================================================================================================ sums
@pytest.mark.parametrize("N", [2, 6, 512, 514, 1280])
@pytest.mark.parametrize("rows", [1, 3, 16, 17, 63, 64, 65, 100, 513])
def test_colsum_bf16(ops, rows, N):
    """S (n = rows + 1 terms: out is non-zero beforehand).  rows <= 16 with N % 4 == 0: at most 16 partial rows go through the wide
    (float4) reduce; everything else through the tall reduce, whose 16 partial-lanes see 1 ... 33 partials each: the unrolled-by-4
    loop and each count of remainder steps.  x is the column slice [:, N:2N] of a poisoned [rows, 4N] buffer."""
    x = R.rand((rows, N), 200 + rows + N, 1.0).to(bf)
    out0 = R.rand((N,), 201, 2.0)

    def run(kind):
        xd = poisoned(x, 4 * N, offset=N, kind=kind) if kind else x.cuda()
        res = []
        for rep in range(2):
            o = _out((N,), f32, "colsum", kind is not None, init=out0)
            ops.colsum_bf16(xd, o.view)
            res.append(_finish({"s": o})["s"])
        assert torch.equal(R.bits(res[0]), R.bits(res[1])), "two calls differ"
        return {"s": res[0]}

    got = _same(run, KINDS + (None,), "colsum")["s"]
    terms = torch.cat((out0[None].double(), x.double()), 0)
    ref = terms.sum(0)
    frac = _frac(got, ref, R.sum_bound(terms.abs().sum(0), rows + 1, ref))
    _note(f"colsum rows={rows} N={N}", "frac", frac)
    assert frac <= 1.0, frac


@pytest.mark.parametrize("B,TD", [(1, 4), (2, 4), (5, 4), (1, 1028), (2, 1028), (5, 1028), (2, 4194304 + 1028)])
def test_sum_over_batch(ops, B, TD):
    """E: fp32 ((out + g0) + g1) + ... in batch order, out non-zero beforehand.  The last shape: 4097 blocks of float4 work on a
    4096-block grid."""
    g = R.rand((B, TD), 300 + B, 1.0)
    out0 = R.rand((TD,), 301, 1.0)
    gd = g.cuda()

    def run(padded):
        o = _out((TD,), f32, "sum", padded, init=out0)
        ops.sum_over_batch(gd, o.view)
        return _finish({"s": o})

    got = _same(run, (True, False), "sum_over_batch")["s"]
    _exact(got, R.sum_over_batch_ref(out0, g), "sum_over_batch")


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2097152 + 1027])
def test_sumsq(ops, n):
    """S (n + 1 terms: out is non-zero beforehand; the terms are fp32 products).  The last size: 2049 blocks of vector work on a
    2048-block grid and a 3-element tail.  Three calls back to back on one stream into three outputs are each right (the ticket
    counter is back at zero for the next launch), and a repeat gives equal bits.
    E on top: for 2 097 152 elements the worst-case bound is far wider than one of the 2048 workgroup partials, so a lost partial
    would pass it.  With x in {-2, ..., 2} and whole-numbered initial values every partial sum, in any order, is a whole number
    below 2^24 and the result is exact: it must equal init + sum x^2 to the bit."""
    xi = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(401)).float()
    xid = xi.cuda()
    oi = {f"o{i}": _out((1,), f32, f"sumsq_int{i}", True, init=torch.tensor([v])) for i, v in enumerate((0.0, 3.0, -1.0))}
    for o in oi.values():
        ops.sumsq(xid, o.view)
    goti = _finish(oi)
    for i, v in enumerate((0.0, 3.0, -1.0)):
        assert float(goti[f"o{i}"]) == v + float((xi.double() ** 2).sum()), (i, float(goti[f"o{i}"]), v + float((xi.double() ** 2).sum()))
    x = R.rand((n,), 400, 1.0)
    xd = x.cuda()
    init = torch.tensor([0.0, 2.5, -1.0])

    def run(padded):
        outs = {f"o{i}": _out((1,), f32, f"sumsq{i}", padded, init=init[i:i + 1]) for i in range(3)}
        for o in outs.values():
            ops.sumsq(xd, o.view)
        return _finish(outs)

    got = _same(run, (True, False, True), "sumsq")
    ss = float((x.double() ** 2).sum())
    for i in range(3):
        ref = float(init[i]) + ss
        bound = float(R.sum_bound(abs(float(init[i])) + ss, n + 1, ref, product_terms=True))
        frac = abs(float(got[f"o{i}"]) - ref) / bound
        _note(f"sumsq n={n} call {i}", "frac", frac)
        assert frac <= 1.0, (i, float(got[f"o{i}"]), ref)


# ================================================================================================ decoder embedding
def _ids(B, Lq, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, Lq), generator=g)
    ids.reshape(-1)[0] = 0
    ids.reshape(-1)[-1] = V - 1
    return ids


@pytest.mark.parametrize("B,Lq,D", [(2, 3, 4), (3, 7, 384), (1, 1, 1280)])
def test_embed_fwd(ops, B, Lq, D):
    """E (one fp32 add).  D = 4: one float4 per row; 384: a partial trip of the 256-thread loop; 1280: a second trip.  ids
    include 0 and V - 1.  Then the decode form: Lq = 1 with `pos` a view [t:] of the table."""
    V, P, t = 11, Lq + 5, 3
    tok, pos = R.rand((V, D), 500 + D, 1.0), R.rand((P, D), 501 + D, 1.0)
    td, pd = tok.cuda(), pos.cuda()
    for name, ids, pv, pref in (("train", _ids(B, Lq, V, 502), pd, pos), ("decode", _ids(B, 1, V, 503), pd[t:], pos[t:])):
        idd = ids.cuda()
        rows = ids.numel()

        def run(padded):
            o = _out((rows, D), f32, "embed", padded)
            ops.embed_fwd(idd, td, pv, o.view)
            return _finish({"y": o})

        got = _same(run, (True, False), f"embed_fwd {name}")["y"]
        _exact(got.view(*ids.shape, D), R.embed_fwd_ref(ids, tok, pref), f"embed_fwd {name}")


@pytest.mark.parametrize("which", ["tok", "pos", "both"])
@pytest.mark.parametrize("ids_kind", ["equal", "distinct"])
@pytest.mark.parametrize("D", [384, 6])
def test_embed_bwd(ops, D, ids_kind, which):
    """S (per target element n = 1 + the number of rows that land on it; the targets are non-zero beforehand, as the token table's
    gradient is in training: the tied LM head has accumulated into it).  (B, Lq) = (3, 7): all 21 ids equal (21 rows meet in one
    target row), or all distinct.  D = 6 is no multiple of 4: the kernel allows it.  Target rows no id / position lands on keep
    their bits.
    E on top: the kernel adds the rows of a token in row order and the batches of a position in batch order, once into the target
    (no atomics), so the result equals the fp32 emulation of that order, a repeat and the exactly sized run bit for bit."""
    B, Lq, V, P = 3, 7, 23, 9
    ids = torch.full((B, Lq), 5) if ids_kind == "equal" else torch.randperm(V, generator=torch.Generator().manual_seed(7))[:B * Lq].view(B, Lq)
    _embed_bwd_case(ops, f"D={D} {ids_kind} {which}", ids, V, P, D, which)


def test_embed_bwd_rows_meet_across_scan_chunks(ops):
    """S and E as above.  (B, Lq) = (3, 200) with ids from 40 tokens and D = 260: the kernel scans the 600 ids 256 at a time and
    walks D in two trips, so rows of one token meet across chunks, and the last chunk is a partial one."""
    B, Lq, V, P, D = 3, 200, 41, 203, 260
    ids = torch.randint(0, 40, (B, Lq), generator=torch.Generator().manual_seed(8))
    _embed_bwd_case(ops, "600 rows D=260", ids, V, P, D, "both")


def _embed_bwd_case(ops, name, ids, V, P, D, which):
    B, Lq = ids.shape
    g = R.rand((B, Lq, D), 600 + D, 1.0)
    tok0, pos0 = R.rand((V, D), 601, 1.0), R.rand((P, D), 602, 1.0)
    idd, gd = ids.cuda(), g.cuda()
    d_tok, d_pos, a_tok, a_pos = R.embed_bwd_ref(ids, g, V, P)
    n_tok = torch.bincount(ids.reshape(-1), minlength=V).double()[:, None] + 1
    n_pos = torch.cat((torch.full((Lq,), B + 1.0), torch.ones(P - Lq))).double()[:, None]

    def run(padded):
        o = {}
        if which != "pos":
            o["tok"] = _out((V, D), f32, "d_tok", padded, init=tok0)
        if which != "tok":
            o["pos"] = _out((P, D), f32, "d_pos", padded, init=pos0)
        ops.embed_bwd(idd, gd, o["tok"].view if "tok" in o else None, o["pos"].view if "pos" in o else None, D)
        return _finish(o)

    got = _same(run, (True, False, True), "embed_bwd")
    e_tok, e_pos = R.embed_bwd_exact(ids, g, tok0, pos0)
    for k, init, d, a, n, e in (("tok", tok0, d_tok, a_tok, n_tok, e_tok), ("pos", pos0, d_pos, a_pos, n_pos, e_pos)):
        if k not in got:
            continue
        ref = init.double() + d
        frac = _frac(got[k], ref, R.sum_bound(init.double().abs() + a, n, ref))
        _note(f"embed_bwd {name} d_{k}", "frac", frac)
        assert frac <= 1.0, (k, frac)
        idle = (n == 1).reshape(-1)
        assert torch.equal(R.bits(got[k][idle]), R.bits(init[idle])), f"d_{k}: a row nothing lands on changed"
        _exact(got[k], e, f"d_{k} against the ordered fp32 sum")


# ================================================================================================ conv-stem backward helpers
def _gelu_case(ops, name, g, pre, padded_variants=(True, False)):
    gd, pd = g.cuda(), pre.cuda()
    n = g.numel()

    def run(padded):
        o = _out((n,), bf, "gelu_bwd", padded)
        ops.gelu_bwd_bf16(gd, pd, o.view)
        return _finish({"y": o})

    return _same(run, padded_variants, name)["y"]


@pytest.mark.parametrize("gval", [1.0, -0.37])
@pytest.mark.parametrize("n", [4, 1028])
def test_gelu_bwd_bf16(ops, n, gval):
    """M (A_GELU_BWD).  pre: +-0, +-30 and a dense grid on [-9, 9]; n = 4: one vector, 1028: two blocks."""
    pre = R.gelu_pre_grid(n)
    g = torch.full((n,), gval).to(bf)
    got = _gelu_case(ops, "gelu_bwd", g, pre)
    ref = g.double() * R.gelu_grad_ref(pre)
    a = _resid_bf16(got, ref)
    _note(f"gelu_bwd n={n} g={gval}", "A", a)
    assert torch.isfinite(got.float()).all() and a <= A_GELU_BWD, a


def test_gelu_bwd_bf16_past_the_grid_cap(ops):
    """M (A_GELU_BWD).  n = 8 388 608 + 1 028: 8193 blocks of work on an 8192-block grid.  pre tiles every bf16 value of
    [-9, 9], g alternates between 1 and -0.37.  Compared on a deterministic subsample element by element and as a whole through
    the sketch (k inner products with +-1 vectors: |sketch(got) - sketch(ref)| <= sum_i (2^-8 |ref_i| + A), the same bound summed)."""
    n = 8388608 + 1028
    pre = R.gelu_pre_grid(n)
    g = torch.tensor([1.0, -0.37]).to(bf).repeat(n // 2)
    got = _gelu_case(ops, "gelu_bwd big", g, pre, (True,))
    ref = g.double() * R.gelu_grad_ref(pre)
    a = _resid_bf16(subsample(got), subsample(ref))
    _note("gelu_bwd n=8389636 subsample", "A", a)
    assert a <= A_GELU_BWD, a
    d = (sketch(got.cuda(), "gelu_bwd").double() - sketch(ref.cuda(), "gelu_bwd").double()).abs().cpu()
    budget = float((2.0 ** -8 * ref.abs() + A_GELU_BWD).sum()) + 2.0 ** -22 * float(ref.abs().sum())   # (+ the sketch's own fp32 output)
    _note("gelu_bwd n=8389636 sketch", "frac", float(d.max()) / budget)
    assert float(d.max()) <= budget
    # (cheap on top of what the subsample sees: every element)
    a_all = _resid_bf16(got, ref)
    _note("gelu_bwd n=8389636 all", "A", a_all)
    assert a_all <= A_GELU_BWD, a_all


@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("B,T2,C", [(1, 1, 2), (2, 3, 6), (2, 50, 384)])
def test_conv2_col2im_gelu_bwd(ops, B, T2, C, with_pre):
    """pre1 = None: E (at most two bf16 terms meet in fp32, one bf16 rounding); with pre1: M (A_COL2IM) against the fp64 scatter x
    GELU'(pre1).  Frame 0 has no tap-2 partner; the last frame's tap 0 would belong to t = T2 and is dropped; each tap carries
    its own constant (1, 2, 4)."""
    dA2 = R.col2im_input(B, T2, C)
    pre1 = R.gelu_pre_grid(B * 2 * T2 * C).view(B, 2 * T2, C) if with_pre else None
    dd, pd = dA2.cuda(), None if pre1 is None else pre1.cuda()

    def run(padded):
        o = _out((B * 2 * T2, C), bf, "d_pre1", padded)
        ops.conv2_col2im_gelu_bwd(dd, pd, o.view, B, T2, C)
        return _finish({"y": o})

    got = _same(run, (True, False), "col2im")["y"].view(B, 2 * T2, C)
    if not with_pre:
        _exact(got, R.col2im_ref(dA2.float(), T2, C).to(bf), "col2im")
        # by value as well: first frame = tap 1 of t = 0 alone (about 2), last frame = tap 2 of t = T2 - 1 alone (about 4)
        assert abs(float(got[:, 0].float().mean()) - 2.0) < 0.5 and abs(float(got[:, -1].float().mean()) - 4.0) < 0.5
    else:
        ref = R.col2im_ref(dA2.double(), T2, C) * R.gelu_grad_ref(pre1)
        a = _resid_bf16(got, ref)
        _note(f"col2im+gelu B={B} T2={T2} C={C}", "A", a)
        assert torch.isfinite(got.float()).all() and a <= A_COL2IM, a


# ================================================================================================ speaker-communication block glue
@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("Bp,T,D", SCB_SHAPES)
def test_scb_split(ops, Bp, T, D, gap):
    """E.  ldcat = 2 D and 2 D + 8: only the right half of `cat` is written, the left half and the gap keep the sentinel."""
    hf = R.rand((Bp * 2 * T, D), 700 + D, 1.0)
    hd = hf.cuda()
    ldcat = 2 * D + gap

    def run(padded):
        o = {"q_in": _out((Bp * T, D), bf, "q_in", padded), "kv_in": _out((Bp * T, D), bf, "kv_in", padded)}
        cat = guarded((Bp * T, D), ldcat, bf, offset=D, name="cat") if padded else None
        if cat is None:                                    # exactly sized: [Bp T, 2 D], the left half checked by hand
            cat = _Plain((Bp * T, 2 * D), bf, None)
        ops.scb_split(hd, o["q_in"].view, o["kv_in"].view, _cat_arg(cat, padded, D, ldcat), Bp, T, D)
        res = _finish(o)
        torch.cuda.synchronize()
        cat.check()
        if padded:
            assert cat.untouched_inside() == 0
            res["cat_right"] = cat.view.cpu().clone()
        else:
            assert bool(_sentinel_rows(cat.view[:, :D]).all()), "left half of cat written"
            res["cat_right"] = cat.view[:, D:].cpu().clone()
        return res

    got = _same(run, (True, False), "scb_split")
    q, kv = R.scb_split_ref(hf, Bp, T, D)
    _exact(got["q_in"], q, "q_in"), _exact(got["kv_in"], kv, "kv_in"), _exact(got["cat_right"], q, "cat right half")


def _cat_arg(cat, padded, D, ldcat):
    """The [rows, 2 D] (row stride ldcat) tensor ops.scb_split / scb_merge_bwd take: its data_ptr is column 0, stride(0) the row stride."""
    if not padded:
        return cat.view
    rows = cat.view.shape[0]
    return cat.buf.as_strided((rows, 2 * D), (ldcat, 1), cat.lead)


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("Bp,T,D", SCB_SHAPES)
def test_scb_merge_fwd(ops, Bp, T, D, gate):
    """M (A_MERGE_FWD, fp32 output: device tanhf, and hf + upd * tanh may or may not contract).  Enrollment rows equal hf bit for bit."""
    hf = R.rand((Bp * 2 * T * D,), 710 + D, 1.0)
    upd = R.rand((Bp * T * D,), 711 + D, 1.0).to(bf)
    gt = torch.tensor([gate])
    hd, ud, gd = hf.cuda(), upd.cuda(), gt.cuda()

    def run(padded):
        o = _out((Bp * 2 * T * D,), f32, "merge", padded)
        ops.scb_merge_fwd(hd, ud, gd, o.view, Bp, T, D)
        return _finish({"y": o})

    got = _same(run, (True, False), "scb_merge_fwd")["y"]
    ref = R.scb_merge_fwd_ref(hf.double(), upd.double(), gt.double(), Bp, T, D)
    e = _rel32(got, ref)
    _note(f"scb_merge_fwd {Bp}x{T}x{D} gate={gate}", "rel", e)
    assert e <= A_MERGE_FWD, e
    _exact(got.view(Bp, 2, T * D)[:, 1], hf.view(Bp, 2, T * D)[:, 1], "enrollment rows")
    if gate == 0.0:
        _exact(got, hf, "gate 0: tanh(0) = 0, out = hf")


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("Bp,T,D", SCB_SHAPES)
def test_scb_gate_bwd(ops, Bp, T, D, gate):
    """d_upd: M (A_GATE_DUPD, bf16).  d_gate: S on the sum (n products of g and upd), against the fp64 sum x the fp64 factor:
        |got - (d0 + f S)| <= b_S (f + A_f) + A_f |S| + 2^-24 |f S| + 2^-24 |d0 + f S|
    with b_S the summation bound of S, A_f = A_GATE_FACTOR the measured error of the device's 1 - tanh(gate)^2 (read off a case
    whose sum is exactly 1: test_scb_gate_factor), and one rounding each for the product and for the accumulation.  d_gate is
    non-zero beforehand; d_gate = None leaves d_upd identical; two calls give equal bits.  The largest shape fills all 1024
    partials of the finish kernel.
    At that size b_S is far wider than one partial, so a lost partial would pass it.  Hence a second pair of inputs with g and upd
    in {-3, ..., 3}: every product and every partial sum, in any order, is a whole number below 2^24, S is exact in fp32 and b_S
    drops out of the bound."""
    g = R.rand((Bp * 2 * T * D,), 720 + D, 1.0)
    upd = R.rand((Bp * T * D,), 721 + D, 1.0).to(bf)
    gt, d0 = torch.tensor([gate]), torch.tensor([0.75])
    gd, ud, gtd = g.cuda(), upd.cuda(), gt.cuda()

    def run(v):
        padded, with_gate = v
        o = {"d_upd": _out((Bp * T * D,), bf, "d_upd", padded)}
        if with_gate:
            o["d_gate"] = _out((1,), f32, "d_gate", padded, init=d0)
        ops.scb_gate_bwd(gd, ud, gtd, o["d_upd"].view, o["d_gate"].view if with_gate else None, Bp, T, D)
        return _finish(o)

    got = run((True, True))
    _bits_equal(got, run((False, True)), "guarded vs exact")
    _bits_equal(got, run((True, True)), "repeat")
    _bits_equal({"d_upd": got["d_upd"]}, run((True, False)), "d_gate = None")
    d_upd, S, Sabs, f = R.scb_gate_bwd_ref(g, upd, gt, Bp, T, D)
    a = _resid_bf16(got["d_upd"], d_upd)
    _note(f"scb_gate_bwd {Bp}x{T}x{D} gate={gate}", "A d_upd", a)
    assert a <= A_GATE_DUPD, a
    S, Sabs, f = float(S), float(Sabs), float(f)
    ref = float(d0) + f * S
    b_s = float(R.sum_bound(Sabs, Bp * T * D, S, product_terms=True))
    bound = b_s * (f + A_GATE_FACTOR) + A_GATE_FACTOR * abs(S) + U * abs(f * S) + U * abs(ref)
    frac = abs(float(got["d_gate"]) - ref) / bound
    _note(f"scb_gate_bwd {Bp}x{T}x{D} gate={gate}", "frac d_gate", frac)
    assert frac <= 1.0, (float(got["d_gate"]), ref, bound)
    # whole-numbered inputs: S exact
    gen = torch.Generator().manual_seed(722 + D)
    gi = torch.randint(-3, 4, (Bp * 2 * T * D,), generator=gen).float()
    ui = torch.randint(-3, 4, (Bp * T * D,), generator=gen).float().to(bf)
    o = {"d_upd": _out((Bp * T * D,), bf, "d_upd", True), "d_gate": _out((1,), f32, "d_gate", True, init=d0)}
    ops.scb_gate_bwd(gi.cuda(), ui.cuda(), gtd, o["d_upd"].view, o["d_gate"].view, Bp, T, D)
    goti = _finish(o)
    _, S, Sabs, _ = R.scb_gate_bwd_ref(gi, ui, gt, Bp, T, D)
    assert float(Sabs) < 2.0 ** 24
    S = float(S)
    ref = float(d0) + f * S
    bound = A_GATE_FACTOR * abs(S) + U * abs(f * S) + U * abs(ref)
    frac = abs(float(goti["d_gate"]) - ref) / bound if bound > 0 else float(float(goti["d_gate"]) != ref)
    _note(f"scb_gate_bwd {Bp}x{T}x{D} gate={gate}", "frac ints", frac)
    assert frac <= 1.0, (float(goti["d_gate"]), ref, bound)


@pytest.mark.parametrize("gate", GATES)
def test_scb_gate_factor(ops, gate):
    """M (A_GATE_FACTOR).  g = upd = (1, 0, 0, 0) and d_gate = 0 beforehand: the sum is exactly 1, so d_gate is the device's
    1 - tanh(gate)^2 itself."""
    g = torch.tensor([1.0, 0, 0, 0, 9.0, 9.0, 9.0, 9.0])                 # (the enrollment slot must not enter)
    upd = torch.tensor([1.0, 0, 0, 0]).to(bf)
    gt = torch.tensor([gate])
    o = {"d_upd": _out((4,), bf, "d_upd", True), "d_gate": _out((1,), f32, "d_gate", True, init=torch.zeros(1))}
    ops.scb_gate_bwd(g.cuda(), upd.cuda(), gt.cuda(), o["d_upd"].view, o["d_gate"].view, 1, 1, 4)
    got = _finish(o)
    f = 1.0 - float(torch.tanh(gt.double())) ** 2
    e = abs(float(got["d_gate"]) - f)
    _note(f"scb_gate factor gate={gate}", "abs", e)
    assert e <= A_GATE_FACTOR, e


@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("Bp,T,D", SCB_SHAPES)
def test_scb_merge_bwd(ops, Bp, T, D, gap):
    """E: fp32 g + (d_qin + float(d_cat[:, D:])) on mixture rows, g + d_kvin on enrollment rows.  The left half of d_cat and the
    ld gap are poison."""
    g = R.rand((Bp * 2 * T * D,), 730 + D, 1.0)
    d_qin, d_kvin = R.rand((Bp * T * D,), 731 + D, 1.0), R.rand((Bp * T * D,), 732 + D, 1.0)
    d_cat = R.rand((Bp * T, D), 733 + D, 1.0).to(bf)
    gd, qd, kd = g.cuda(), d_qin.cuda(), d_kvin.cuda()
    ldcat = 2 * D + gap

    def run(kind):
        if kind:
            right = poisoned(d_cat, ldcat, offset=D, kind=kind)
            cat = right.as_strided((Bp * T, 2 * D), (ldcat, 1), right.storage_offset() - D)
        else:
            cat = torch.zeros(Bp * T, 2 * D, dtype=bf, device="cuda")
            cat[:, D:] = d_cat.cuda()
        o = _out((Bp * 2 * T * D,), f32, "gin", kind is not None)
        ops.scb_merge_bwd(gd, qd, cat, kd, o.view, Bp, T, D)
        return _finish({"gin": o})

    got = _same(run, KINDS + (None,), "scb_merge_bwd")["gin"]
    _exact(got, R.scb_merge_bwd_ref(g, d_qin, d_cat, d_kvin, Bp, T, D), "scb_merge_bwd")


# ================================================================================================ full-FDDT combine
COMBINE_SHAPES = [(2, 3, 4), (3, 50, 384), (2, 1650, 1272)]      # the last: 1 049 400 float4s, past 4096 blocks x 256 threads
MASKS = [0b1111, 0b0110, 0b0000]


def _stno(B, T):
    """[B, 4, T] soft masks (tests.util.hashed_stno; for T < 10 the first T frames of a longer one: its padding rule would
    otherwise make every frame silence)."""
    return hashed_stno(B, T, "glue.combine") if T >= 10 else hashed_stno(B, 30, "glue.combine")[:, :, :T].contiguous()


def _stno_dev(stno, kind):
    """(device tensor whose data_ptr is row 0, batch stride): contiguous (bstride = 4 T), or batches 4 T + 8 apart inside poison."""
    B, _, T = stno.shape
    if kind is None:
        return stno.cuda(), 4 * T
    return poisoned(stno.reshape(B, 4 * T), 4 * T + 8, kind=kind), 4 * T + 8


@pytest.mark.parametrize("h_dtype", [f32, bf], ids=["h_f32", "h_bf16"])
@pytest.mark.parametrize("use_mask", MASKS)
@pytest.mark.parametrize("B,T,D", COMBINE_SHAPES)
def test_fddt_full_combine_fwd(L, B, T, D, use_mask, h_dtype):
    """Derived bound: |got - ref64| <= 8 x 2^-24 x sum_c |m_c v_c| (four products and four additions, contraction allowed).
    The y4 slices of unused classes hold NaN: they must not be read."""
    rows = B * T
    stno = _stno(B, T)
    y4 = R.rand((B, T, 4, D), 800 + D, 1.0).to(bf)
    h = R.rand((B, T, D), 801 + D, 1.0).to(h_dtype)
    y4p = y4.clone()
    for c in range(4):
        if not (use_mask >> c) & 1:
            y4p[:, :, c] = float("nan")
    yd, hd = y4p.cuda(), h.cuda()

    def run(kind):
        sd, bstride = _stno_dev(stno, kind)
        o = _out((rows, D), f32, "h_out", kind is not None)
        L.call("dicow_fddt_full_combine_fwd", yd.data_ptr(), hd.data_ptr(), int(h_dtype == bf), sd.data_ptr(), bstride, use_mask,
               o.view.data_ptr(), rows, T, D, L.stream())
        return _finish({"y": o})

    got = _same(run, KINDS + (None,), "combine_fwd")["y"].view(B, T, D)
    ref, mag = R.combine_fwd_ref(y4, h, stno, use_mask)
    frac = _frac(got, ref, 8 * U * mag)
    _note(f"combine_fwd {B}x{T}x{D} mask={use_mask:04b} {'bf16' if h_dtype == bf else 'f32'}", "frac", frac)
    assert frac <= 1.0, frac


@pytest.mark.parametrize("use_mask", MASKS)
@pytest.mark.parametrize("B,T,D", COMBINE_SHAPES)
def test_fddt_full_combine_bwd(L, B, T, D, use_mask):
    """E: d_y4_c = bf16(fp32(g m_c)) for the used classes, dh = g (sum of the unused m_c in class order).  d_y4 starts as sentinel:
    afterwards the slices of unused classes are still all sentinel, the used ones hold none.  dh_direct = NULL is accepted and
    leaves d_y4 identical."""
    rows = B * T
    stno = _stno(B, T)
    g = R.rand((B, T, D), 810 + D, 1.0)
    gd = g.cuda()

    def run(v):
        kind, with_dh = v
        sd, bstride = _stno_dev(stno, kind)
        o = {"d_y4": _out((rows, 4 * D), bf, "d_y4", kind is not None)}
        if with_dh:
            o["dh"] = _out((rows, D), f32, "dh", kind is not None)
        L.call("dicow_fddt_full_combine_bwd", gd.data_ptr(), sd.data_ptr(), bstride, use_mask, o["d_y4"].view.data_ptr(),
               o["dh"].view.data_ptr() if with_dh else None, rows, T, D, L.stream())
        res = _finish(o, overwritten=False)
        if with_dh:
            assert o["dh"].untouched_inside() == 0
        return res

    got = _same(run, (("nan", True), ("big", True), (None, True)), "combine_bwd")
    _bits_equal({"d_y4": got["d_y4"]}, run(("nan", False)), "dh_direct = NULL")
    d_y4, dh = R.combine_bwd_ref(g, stno, use_mask)
    _exact(got["dh"].view(B, T, D), dh, "dh")
    gy = got["d_y4"].view(B, T, 4, D)
    for c in range(4):
        s = _sentinel_rows(gy[:, :, c])
        if (use_mask >> c) & 1:
            assert not bool(s.any()), f"class {c}: {int(s.sum())} elements never written"
            _exact(gy[:, :, c].contiguous(), d_y4[:, :, c].contiguous(), f"d_y4 class {c}")
        else:
            assert bool(s.all()), f"class {c} is unused: its slice must stay untouched"


# ================================================================================================ refusals
def test_argument_errors_raise_and_leave_the_library_usable(ops, L):
    """Every invalid argument set is refused with DicowError before any launch (the outputs keep the sentinel), and valid calls
    afterwards give the same bits as before."""
    x = R.cast_values(1027).cuda()
    xs = R.rand((17, 6), 900).to(bf).cuda()

    def valid():
        o = {"cast": _out((1027,), bf, "cast", True), "colsum": _out((6,), f32, "colsum", True, init=torch.ones(6))}
        ops.cast_bf16(x, out=o["cast"].view)
        ops.colsum_bf16(xs, o["colsum"].view)
        return _finish(o)

    before = valid()
    z = lambda *s: torch.ones(*s, device="cuda")                                                      # noqa: E731
    zb = lambda *s: torch.ones(*s, device="cuda", dtype=bf)                                            # noqa: E731
    ids = torch.zeros(2, 3, dtype=torch.long, device="cuda")
    o = {k: _out(s, d, k, True) for k, s, d in (
        ("colsum", (4,), f32), ("sum", (8,), f32), ("gelu", (8,), bf), ("embed", (6, 6), f32), ("q_in", (4, 8), bf),
        ("kv_in", (4, 8), bf), ("cat", (4, 16), bf), ("cat12", (4, 12), bf), ("pack", (6, 16), bf), ("pack_t", (16, 6), bf), ("h_out", (6, 8), f32))}
    bad = [
        ("colsum_bf16 N=3", lambda: ops.colsum_bf16(zb(5, 3), o["colsum"].view)),
        ("sum_over_batch TD=6", lambda: ops.sum_over_batch(z(2, 6), o["sum"].view)),
        ("gelu_bwd_bf16 n=6", lambda: ops.gelu_bwd_bf16(zb(6), zb(6), o["gelu"].view)),
        ("embed_fwd D=6", lambda: ops.embed_fwd(ids, z(4, 6), z(3, 6), o["embed"].view)),
        ("scb_split D=6", lambda: ops.scb_split(z(8, 6), o["q_in"].view, o["kv_in"].view, o["cat"].view, 2, 2, 6)),
        ("scb_split ldcat<2D", lambda: ops.scb_split(z(8, 8), o["q_in"].view, o["kv_in"].view, o["cat12"].view, 2, 2, 8)),
        ("conv_weight_pack Kpad<3C", lambda: ops.conv_weight_pack(z(6, 5, 3), 12, out=o["pack"].view, out_t=o["pack_t"].view, want_t=True)),
        ("fddt_full_combine_fwd D=6", lambda: L.call("dicow_fddt_full_combine_fwd", zb(6, 24).data_ptr(), z(6, 6).data_ptr(), 0,
                                                     z(2, 4, 3).data_ptr(), 12, 0b1111, o["h_out"].view.data_ptr(), 6, 3, 6, L.stream())),
    ]
    for name, fn in bad:
        with pytest.raises(L.DicowError):
            fn()
    torch.cuda.synchronize()
    for k, g in o.items():
        g.check()
        assert g.untouched_inside() == g.view.numel(), f"{k}: written by a refused call"
    _bits_equal(before, valid(), "valid calls after the refusals")

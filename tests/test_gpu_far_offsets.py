"""Operands past the 2 GiB and 4 GiB offset marks on the MI355X.  Every entry point of the library takes base pointers with int64
leading dimensions and batch strides; this file runs the kernels on operands whose elements lie more than 2^31 / 2^32 bytes from
the base pointer -- strided views into ONE device arena that holds a NaN sentinel everywhere else (tests/util.Arena / far_view;
the view's base lies at least its own span into the arena, so a 32-bit-wrapped address still lands inside the allocation).  The
contract: an entry point either computes correctly there or returns DICOW_ERR_INVALID before any launch.

One operand at a time goes far (the others compact), then all of them.  Each case asserts
  (a) the body that ran (GEMM dispatch log, the *_route queries);
  (b) numbers: BIT-equal to the same call on compact operands where the same body runs, parity with the fp64 reference at the bound
      the kernel's own test file uses where the guard sends the far call to another body (each bound below cites its source);
  (c) the stray-write count: the arena's non-sentinel words are exactly those of the logical operands (Arena.check).
Tall-stride views use tests/util.tall_ld: few rows, a leading dimension near 2^32 / (rows - 2) bytes, and -- wherever the row count
allows -- one row that BEGINS less than a row length below 2^32, so that its elements straddle the mark.
Every case prints a `far_offsets:` line (body, error against bound, arena bytes, wall time): profiles/far_offsets.txt.
Run with `pytest -m gpu`."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import amd_pkg
from oracle import dicow_oracle as O
from tests import ctc_prefix_ref, glue_ref
from tests.loss_ref import ce_ref
from tests.util import MARK31, MARK32, _ceil_to, _nonsentinel_words, far_arena_fixture, far_view, tall_ld
from tests.test_gpu_kernels import LN2
from tests.test_gpu_layout_edges import _bf, _err, _launched

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()
BF16, F32 = torch.bfloat16, torch.float32
GiB = 1 << 30
ARENA_BYTES = 18 * GiB       # the largest case: A, B and C of one GEMM far at once (three tall views of 4.3 GiB behind one front pad)
far_arena_module = far_arena_fixture(ARENA_BYTES, 4 * GiB)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


@pytest.fixture
def arena(far_arena_module):
    far_arena_module.reset()
    return far_arena_module


def _sentinel(shape, dtype):
    """A compact output that starts as NaN in every element (an element the kernel skips fails parity and bit-equality)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int16).fill_(0x7FC1)
    return t


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, "the far layout changed the result")


class _Clock:
    def __init__(self):
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def ms(self):
        torch.cuda.synchronize()
        return (time.perf_counter() - self.t0) * 1e3


def _record(case, body, err, bound, arena, clock):
    print(f"far_offsets: {case:<62s} body={body:<30s} err={err:.3e} bound={bound:.3e} arena_bytes={arena.used} wall_ms={clock.ms():.0f}")


# ================================================================================================ the layout itself
def test_far_view_layout_and_stray_count(arena):
    """The helpers on the device: a tall view has rows on both sides of both marks and one that straddles 2^32; the stray count sees
    one stray word anywhere in the arena, and an input that changed."""
    ld, r = tall_ld(300, 128, 2)
    assert r is not None and r * ld * 2 < MARK32 < r * ld * 2 + 256 and 299 * ld * 2 >= MARK32 and ld % 8 == 0
    assert 100 < MARK31 // (ld * 2) < 200                                                  # 2^31 falls among the middle rows
    vals = torch.randn(300, 128).bfloat16()
    v = far_view(arena, (300, 128), BF16, (ld, 1), values=vals, name="A")
    base = v.data_ptr() - arena.buf.data_ptr()
    assert base >= 299 * ld * 2 and torch.equal(v.cpu(), vals)
    out = far_view(arena, (300, 128), BF16, (ld, 1), name="C", output=True)
    assert out.data_ptr() - arena.buf.data_ptr() >= base + 299 * ld * 2
    assert arena.check() == 300 * 128                                                      # nothing written yet: the input's words
    out.copy_(vals)
    assert arena.check() == 2 * 300 * 128
    arena.buf[GiB + 2] = 1                                                                 # one stray byte, in the front pad
    with pytest.raises(AssertionError, match="1 stray"):
        arena.check()
    arena.buf[GiB + 2] = 0xC1                                                              # (the low byte of the sentinel, 0x7FC1)
    arena.check()
    v[150, 7] = 1.0
    with pytest.raises(AssertionError, match="input operand was overwritten"):
        arena.check()


# ================================================================================================ NT GEMM
# Bounds (test_gpu_layout_edges.py NT_CASES, themselves test_gpu_kernels.py's): fp32 plain 1e-4 max(1, |ref|), bf16 plain 1e-2 max(1, |ref|)
# (test_gemm_nt_plain); bias + residual 3e-2 (test_gemm_nt64_decoder_shapes / test_gemm_nt_epilogues), 4e-2 on gemm_nt128t
# (test_gemm_nt_mid_size_shapes); GELU 3e-2, MUL_AUX 4e-2, its column sums 2e-3 max(1, |ref|) + 0.15 sqrt(M) 2^-8 (test_gemm_nt_epilogues).
NT_ALIGN = {"A": 8, "B": 8, "C": 4, "res": 4, "aux": 4}          # nt_check_args: lda / ldb % 8, ldc / ldr / ldaux % 4


def _nt_problem(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A, B = _bf(torch.randn(M, K, generator=g)).cuda(), _bf(torch.randn(N, K, generator=g) * K ** -0.5).cuda()
    bias, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    daux = _bf(torch.rand(M, N, generator=g) * 1.1).cuda()
    ref = A.double() @ B.double().t()
    return dict(A=A, B=B, bias=bias, res=res, daux=daux, ref=ref, rmax=max(1.0, float(ref.abs().max())))


def _nt_run(ops, arena, p, M, N, K, dtype, far=(), lds=None, *, bias=False, res=False, aux_in=False, aux_out=False, flags=0, colsum=False):
    """One ops.gemm_nt call; the operands named in `far` (A, B, C, res, aux) are tall views of the arena (lds: a leading dimension
    given outright), the others compact.  Returns (outputs, kernels launched, {operand: straddling row})."""
    lds, strad = dict(lds or {}), {}
    shapes = {"A": (M, K), "B": (N, K), "C": (M, N), "res": (M, N), "aux": (M, N)}

    def operand(name, vals, dt, output=False):
        rows, cols = shapes[name]
        isz = torch.empty(0, dtype=dt).element_size()
        if name in far or name in lds:
            ld = lds.get(name)
            if ld is None:
                ld, strad[name] = tall_ld(rows, cols, isz, NT_ALIGN[name])
            return far_view(arena, (rows, cols), dt, (ld, 1), values=vals, name=name, output=output), ld
        return (_sentinel((rows, cols), dt) if output else vals.to(dt)), cols

    Ad, lda = operand("A", p["A"], BF16)
    Bd, ldb = operand("B", p["B"], BF16)
    Cd, ldc = operand("C", None, dtype, output=True)
    resd, ldr = operand("res", p["res"], F32) if res else (None, N)
    auxd, ldaux = (operand("aux", p["daux"], BF16) if aux_in else operand("aux", None, BF16, output=True) if aux_out else (None, N))
    csd = torch.full((N,), 0.5, device="cuda") if colsum else None
    ran = _launched(ops, lambda: ops.gemm_nt(Ad, Bd, Cd, M, N, K, lda=lda, ldb=ldb, ldc=ldc, bias=p["bias"] if bias else None, residual=resd,
                                             ldr=ldr, aux=auxd, ldaux=ldaux, flags=flags, colsum_out=csd))
    out = {"C": Cd}
    if aux_out:
        out["aux"] = auxd
    if colsum:
        out["colsum"] = csd
    return out, ran, strad


def _nt_variants(p, M, N, nt128t):
    """(name, C dtype, the operand that goes far, keywords, [(output, fp64 reference, bound)]) -- the flag sets of
    test_gemm_nt_family_on_padded_poisoned_guarded_operands that have a far-capable operand besides A and B."""
    from ts_asr_whisper_amd import _lib as L
    ref, rmax = p["ref"], p["rmax"]
    base = (ref + p["bias"].double()).float()
    daux = p["daux"].double()
    ref_cs = 0.5 + (ref * daux).sum(0)
    cs_bound = 2e-3 * max(1.0, float(ref_cs.abs().max())) + 0.15 * (M ** 0.5) * 2 ** -8
    return [
        ("C_bf16", BF16, "C", {}, [("C", ref, 1e-2 * rmax)]),
        ("C_f32", F32, "C", {}, [("C", ref, 1e-4 * rmax)]),
        ("residual", F32, "res", dict(bias=True, res=True), [("C", _bf(base).double() + p["res"].double(), 4e-2 if nt128t else 3e-2)]),
        ("aux_in_mul_aux", BF16, "aux", dict(aux_in=True, flags=L.EPI_MUL_AUX), [("C", ref * daux, 4e-2)]),
        ("aux_out_gelu_daux", BF16, "aux", dict(bias=True, aux_out=True, flags=L.EPI_GELU | L.EPI_GELU_DAUX),
         [("C", O.gelu_erf(_bf(base).double()), 3e-2)]),
        ("colsum_fallback_far_C", BF16, "C", dict(aux_in=True, flags=L.EPI_MUL_AUX, colsum=True), [("C", ref * daux, 4e-2), ("colsum", ref_cs, cs_bound)]),
    ]


@pytest.mark.parametrize("which", ["A", "B", "A_B_C"])
def test_gemm_nt_generic_body_far_a_b(ops, arena, which):
    """(300, 132, 128): compact, the plan takes gemm_nt64; with M lda 2 (N ldb 2) past 2^31 its ab32 is false and the 64-bit generic
    body runs -- parity at the plain bounds (fp32 1e-4, bf16 1e-2 times max(1, |ref|)), every C element written, nothing else."""
    M, N, K = 300, 132, 128
    p = _nt_problem(M, N, K)
    far = tuple(which.split("_"))
    for dtype, bound in ((F32, 1e-4 * p["rmax"]), (BF16, 1e-2 * p["rmax"])):
        arena.reset()
        clock = _Clock()
        got, ran, strad = _nt_run(ops, arena, p, M, N, K, dtype, far=far)
        assert ran == ["gemm_nt_kernel<2, false>"], ran
        assert all(strad[n] is not None for n in far if n != "C"), strad                   # a row of A (of B) straddles 2^32
        e = _err(got["C"], p["ref"])
        arena.check()
        _record(f"gemm_nt (300,132,128) far {which} {dtype}", ran[0], e, bound, arena, clock)
        assert e < bound, (which, dtype, e, bound)
    _, ran_compact, _ = _nt_run(ops, arena, p, M, N, K, F32)
    assert ran_compact[0].startswith("gemm_nt64_kernel"), ran_compact                      # the guard, not the shape, chose the generic body


@pytest.mark.parametrize("case", ["nt64", "nt128t"])
def test_gemm_nt_far_outputs_and_epilogue_operands(ops, arena, case):
    """gemm_nt64 (1000, 500, 128) and gemm_nt128t (2100, 1156, 128) with compact A and B: C (bf16, fp32), the residual, aux as an input
    (MUL_AUX) and as an output (GELU | GELU_DAUX) and the C of the column-sum fallback go far in turn, then all of a call's at once.
    The plan does not look at these operands, so the same body runs: bit-equal to the compact call, and every logical output word written."""
    (M, N, K), kernel = {"nt64": ((1000, 500, 128), "gemm_nt64_kernel"), "nt128t": ((2100, 1156, 128), "gemm_nt128t_kernel")}[case]
    p = _nt_problem(M, N, K)
    for name, dtype, far_op, kw, checks in _nt_variants(p, M, N, case == "nt128t"):
        plain, ran_plain, _ = _nt_run(ops, arena, p, M, N, K, dtype, **kw)
        all_far = ("C",) + (("res",) if kw.get("res") else ()) + (("aux",) if kw.get("aux_in") or kw.get("aux_out") else ())
        for far in [(far_op,)] + ([all_far] if all_far != (far_op,) else []):
            arena.reset()
            clock = _Clock()
            got, ran, strad = _nt_run(ops, arena, p, M, N, K, dtype, far=far, **kw)
            assert ran == ran_plain and len(ran) == 1 and ran[0].startswith(kernel), (name, far, ran, ran_plain)
            arena.check()
            for k in got:
                _same_bits(got[k], plain[k], (case, name, far, k))
            for k, want, bound in checks:
                e = _err(got[k], want)
                _record(f"gemm_nt {case} {name} far {'+'.join(far)} .{k}", ran[0], e, bound, arena, clock)
                assert e < bound, (name, far, k, e, bound)


RING_SHAPES = {"ring256": (6100, 2244, 128), "ring35": (12200, 1284, 192)}
RING_GUARD_BYTES = {"A": 2, "B": 2, "C": 4, "res": 4, "aux": 2}          # nt_plan's off32 counts C as 4-byte elements whatever its type


@pytest.mark.parametrize("case,operand", [("ring256", "A"), ("ring256", "B"), ("ring256", "C"), ("ring256", "res"), ("ring256", "aux"),
                                          ("ring35", "A"), ("ring35", "B"), ("ring35", "C"), ("ring35", "res"), ("ring35", "aux")])
def test_gemm_nt_ring_at_its_guard(ops, arena, case, operand):
    """The ring kernel addresses with 32-bit byte offsets; nt_plan's off32 lets it run while M * ld * bytes < 2^31 for lda, ldc, ldr and
    ldaux, and N * ldb * 2 < 2^31.  At the largest leading dimension inside the guard the ring kernel still runs and the result is bit-equal to the compact
    call; one alignment step above it no gemm_ntr_kernel appears in the log and fp64 parity holds at the existing bounds.
    ring256: the plain bf16 product; ring35: bias + residual (fp32); aux: MUL_AUX with aux as the far input."""
    from ts_asr_whisper_amd import _lib as L
    M, N, K = RING_SHAPES[case]
    p = _nt_problem(M, N, K)
    if operand == "aux":
        kw, dtype, exact = dict(aux_in=True, flags=L.EPI_MUL_AUX), BF16, None
        want, bound_of = p["ref"] * p["daux"].double(), lambda body: 4e-2
    elif case == "ring35" or operand == "res":
        kw, dtype, exact = dict(bias=True, res=True), F32, "gemm_ntr_kernel<13, 3, 5>" if case == "ring35" else None
        want = _bf((p["ref"] + p["bias"].double()).float()).double() + p["res"].double()
        bound_of = lambda body: 4e-2 if "128t" in body else 3e-2
    else:
        kw, dtype, exact = {}, BF16, "gemm_ntr_kernel<0, 4, 4>"
        want, bound_of = p["ref"], lambda body: 1e-2 * p["rmax"]
    gb, step = RING_GUARD_BYTES[operand], NT_ALIGN[operand]
    rows = N if operand == "B" else M
    ld_in = (MARK31 - 1) // (rows * gb) // step * step
    assert rows * ld_in * gb < MARK31 <= rows * (ld_in + step) * gb
    plain, ran_plain, _ = _nt_run(ops, arena, p, M, N, K, dtype, **kw)
    assert len(ran_plain) == 1 and ran_plain[0].startswith("gemm_ntr_kernel") and exact in (None, ran_plain[0]), ran_plain
    for ld, inside in ((ld_in, True), (ld_in + step, False)):
        arena.reset()
        clock = _Clock()
        got, ran, _ = _nt_run(ops, arena, p, M, N, K, dtype, lds={operand: ld}, **kw)
        arena.check()
        assert len(ran) == 1, ran
        e, bound = _err(got["C"], want), bound_of(ran[0])
        _record(f"gemm_nt {case} ld{operand}={ld} ({'inside' if inside else 'past'} the guard)", ran[0], e, bound, arena, clock)
        if inside:
            assert ran == ran_plain, (ran, ran_plain)
            _same_bits(got["C"], plain["C"], (case, operand, ld))
        else:
            assert "gemm_ntr_kernel" not in ran[0], ran
        assert e < bound, (case, operand, ld, e, bound)


@pytest.mark.parametrize("far", ["B", "C", "B_C"])
def test_gemm_nt_skinny_far_b_and_c(ops, arena, far):
    """(16, 1284, 1280), a decoding step: the skinny kernel is the one NT kernel outside the dispatch log, so NO logged kernel runs.
    B with N ldb 2 past 2^32, then C.  Same body as compact: bit-equal; bound of the plain bf16 product (1e-2 max(1, |ref|))."""
    M, N, K = 16, 1284, 1280
    p = _nt_problem(M, N, K)
    plain, ran_plain, _ = _nt_run(ops, arena, p, M, N, K, BF16)
    arena.reset()
    clock = _Clock()
    got, ran, strad = _nt_run(ops, arena, p, M, N, K, BF16, far=tuple(far.split("_")))
    assert ran == [] and ran_plain == [], (ran, ran_plain)
    assert all(v is not None for v in strad.values()), strad
    arena.check()
    _same_bits(got["C"], plain["C"], far)
    e, bound = _err(got["C"], p["ref"]), 1e-2 * p["rmax"]
    _record(f"gemm_nt skinny (16,1284,1280) far {far}", "gemm_nt_skinny_kernel", e, bound, arena, clock)
    assert e < bound


def test_gemm_nt_deep_contraction_split_far_a(ops, arena):
    """(200, 384, 8192) with far A: nt_splitk_count does not look at the leading dimensions, so the split still happens (8 ranges, the
    workspace query says so); the ranges run as batches of the generic body (ab32 is false).  Bound of
    test_gemm_nt_deep_contraction_split: 2e-3 max(1, |ref|) in fp32."""
    from ts_asr_whisper_amd import _lib as L
    M, N, K = 200, 384, 8192
    g = torch.Generator().manual_seed(M + K)
    A, B = _bf(torch.randn(M, K, generator=g) * 0.05).cuda(), _bf(torch.randn(N, K, generator=g) * 0.05).cuda()
    p = dict(A=A, B=B, ref=A.double() @ B.double().t())
    lda, row = tall_ld(M, K, 2)
    a = L.GemmArgs()
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.batch, a.flags = M, N, K, lda, K, N, 1, L.EPI_OUT_F32
    assert L.lib().dicow_gemm_nt_splitk_ws_bytes(C.byref(a)) == 8 * M * N * 4
    clock = _Clock()
    got, ran, _ = _nt_run(ops, arena, p, M, N, K, F32, lds={"A": lda})
    assert ran == ["gemm_nt_kernel<2, false>"] and row is not None, (ran, row)
    arena.check()
    e, bound = _err(got["C"], p["ref"]), 2e-3 * max(1.0, float(p["ref"].abs().max()))
    _record("gemm_nt split (200,384,8192) far A", "splitk 8 x " + ran[0], e, bound, arena, clock)
    assert e < bound


def _rows_at_wrapped_offsets(arena, view, rows, cols, ld):
    """What a kernel that reduced each row's byte offset mod 2^32 would read: [rows, cols] gathered from the arena."""
    isz = view.element_size()
    base = view.data_ptr() - arena.buf.data_ptr()
    out = torch.empty(rows, cols, dtype=view.dtype, device="cuda")
    for r in range(rows):
        off = base + (r * ld * isz) % MARK32
        out[r] = arena.buf[off:off + cols * isz].view(view.dtype)
    return out


def test_control_gemm_far_a_wrapped_rows_are_flagged(arena):
    """No kernel runs: the fp64 reference evaluated on the rows the arena holds at each row's offset mod 2^32 (what a 32-bit body
    would read of the far A of test_gemm_nt_generic_body_far_a_b) misses that test's parity assertion -- the sentinel makes it NaN,
    or the wrong rows make it wrong by orders of magnitude."""
    M, N, K = 300, 132, 128
    p = _nt_problem(M, N, K)
    lda, _ = tall_ld(M, K, 2)
    Av = far_view(arena, (M, K), BF16, (lda, 1), values=p["A"], name="A")
    Aw = _rows_at_wrapped_offsets(arena, Av, M, K, lda)
    n_same = int((_bits(Aw) == _bits(p["A"].to(BF16))).all(1).sum())
    assert 0 < n_same < M                                                                  # the rows below 2^32 are the real ones, the others not
    e = _err(Aw.double() @ p["B"].double().t(), p["ref"])
    print(f"control: gemm far A read at wrapped offsets: {M - n_same} rows differ, error {e}")
    assert not (e < 1e-2 * p["rmax"]) and (e != e or e > 100 * 1e-2 * p["rmax"])


# ================================================================================================ TN GEMM
def _tn_problem(Mk, N1, N2):
    g = torch.Generator().manual_seed(Mk + N1)
    A, B = torch.randn(Mk, N1, generator=g).to(BF16).cuda(), torch.randn(Mk, N2, generator=g).to(BF16).cuda()
    ref = A.double().t() @ B.double()
    return A, B, ref, 2e-4 * max(1.0, float(ref.abs().max()))


# (72, 264, 264) and (1032, 264, 264): the shapes at which test_gpu_layout_edges.TN_CASES found the plan taking the 256 tile (without and
# with a split).  (200, 256, 384) and (1500, 384, 1152) take the 128 tile even when compact; they are kept to pin that and the far view.
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("shape,t256", [((72, 264, 264), True), ((1032, 264, 264), True), ((200, 256, 384), False), ((1500, 384, 1152), False)])
def test_gemm_tn_far_a_b_around_the_256_tile_guard(ops, arena, shape, t256, operand):
    """The 256 x 256 TN body addresses A and B with 32-bit offsets; the plan drops it at Mk * ld * 2 >= 2^32.  Just under that the
    256 body still runs (bit-equal to the compact call); at 2^32 gemm_tn256_kernel must not run.  Bound of
    test_gemm_tn_route_on_padded_poisoned_guarded_operands: 2e-4 max(1, |ref|)."""
    Mk, N1, N2 = shape
    A, B, ref, bound = _tn_problem(Mk, N1, N2)
    plain = _sentinel((N1, N2), F32)
    ran_plain = _launched(ops, lambda: ops.gemm_tn(A, B, plain, Mk, N1, N2, accumulate=False))
    assert (ran_plain == ["gemm_tn256_kernel"]) == t256, ran_plain
    ld_in = (MARK32 - 1) // (2 * Mk) // 8 * 8
    assert Mk * ld_in * 2 < MARK32 <= Mk * (ld_in + 8) * 2
    for ld, inside in ((ld_in, True), (ld_in + 8, False)):
        arena.reset()
        clock = _Clock()
        vals, cols = (A, N1) if operand == "A" else (B, N2)
        far = far_view(arena, (Mk, cols), BF16, (ld, 1), values=vals, name=operand)
        Cd = _sentinel((N1, N2), F32)
        kw = dict(lda=ld) if operand == "A" else dict(ldb=ld)
        ran = _launched(ops, lambda: ops.gemm_tn(far if operand == "A" else A, far if operand == "B" else B, Cd, Mk, N1, N2, accumulate=False, **kw))
        arena.check()
        e = _err(Cd, ref)
        _record(f"gemm_tn {shape} ld{operand.lower()}={ld} ({'inside' if inside else 'at'} 2^32)", "+".join(ran), e, bound, arena, clock)
        if inside:
            assert ran == ran_plain, (ran, ran_plain)
            _same_bits(Cd, plain, (shape, operand, ld))
        else:
            assert ran and "gemm_tn256_kernel" not in ran and "gemm_tn256g_kernel" not in ran, ran
        assert e < bound, (shape, operand, ld, e, bound)


@pytest.mark.parametrize("shape", [(200, 256, 384), (1500, 384, 1152)])
def test_gemm_tn_far_c(ops, arena, shape):
    """C through a tall ldc (a row straddles 2^32): same body as compact, bit-equal, every C word written and no other."""
    Mk, N1, N2 = shape
    A, B, ref, bound = _tn_problem(Mk, N1, N2)
    plain = _sentinel((N1, N2), F32)
    ran_plain = _launched(ops, lambda: ops.gemm_tn(A, B, plain, Mk, N1, N2, accumulate=False))
    ldc, row = tall_ld(N1, N2, 4, 4)
    clock = _Clock()
    Cd = far_view(arena, (N1, N2), F32, (ldc, 1), name="C", output=True)
    ran = _launched(ops, lambda: ops.gemm_tn(A, B, Cd, Mk, N1, N2, ldc=ldc, accumulate=False))
    assert ran == ran_plain and row is not None, (ran, ran_plain, row)
    arena.check()
    _same_bits(Cd, plain, shape)
    e = _err(Cd, ref)
    _record(f"gemm_tn {shape} far C", "+".join(ran), e, bound, arena, clock)
    assert e < bound


# ================================================================================================ attention
ATTN_SHAPES = [(100, 100), (140, 260)]
FAR_BS = _ceil_to(MARK32 // 2 + 8, 8)          # elements: batch 1 begins past 2^32 bytes
LANE = 1 << 20                                 # an all-far call gives each operand its own 1 MiB lane of one shared far region


def attn_rs_limit(L):
    """The largest row stride (elements, % 8) of a tile-staged operand: (max(L, 65) - 1) * rs * 2 + 128 < 2^32 (attention.hip check_tile_span;
    tests/test_host_logic.py::test_attention_row_stride_limit_host_logic pins the same number without a GPU)."""
    return (MARK32 - 129) // (2 * (max(L, 65) - 1)) // 8 * 8


class _Routes:
    """While active, every struct call of the ops layer is preceded by the library's own route query for the same arguments."""

    def __enter__(self):
        from ts_asr_whisper_amd import _lib as L
        self.L, self.orig, self.seen = L, L.call_struct, []

        def call_struct(name, st):
            q = getattr(L.lib(), name + "_route", None)
            if q is not None:
                r = q(C.byref(st))
                self.seen.append(None if r is None else r.decode())
            return self.orig(name, st)
        L.call_struct = call_struct
        return self

    def __exit__(self, *exc):
        self.L.call_struct = self.orig
        return False


def _attn_problem(B, H, Lq, Lk, q_log2):
    g = torch.Generator().manual_seed(B * 1000 + Lq + 7 * Lk + H)
    mk = lambda L, sd: _bf(torch.randn(B, L, H, 64, generator=g) * sd).cuda()
    q, k, v, d_o = mk(Lq, 0.6), mk(Lk, 0.6), mk(Lk, 0.6), mk(Lq, 1.0)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("blhd,bmhd->bhlm", q64, k64) * (LN2 if q_log2 else 1.0)
    o = torch.einsum("bhlm,bmhd->blhd", torch.softmax(s, -1), v64)
    (o * d_o.double()).sum().backward()
    dq = (q64.grad / LN2 if q_log2 else q64.grad) * 0.5                                  # dq_scale = 0.5, as in test_attn_bwd
    return dict(q=q, k=k, v=v, d_o=d_o, o=o.detach(), lse=torch.logsumexp(s, -1).detach(), dq=dq, dk=k64.grad, dv=v64.grad)


def _attn_operand(arena, vals, B, L, H, place, name, lane=None, output=False):
    """place: "compact"; "bs": a batch stride that puts batch 1 past 2^32 bytes; ("rs", n): row stride n, the batches interleaved (batch
    b begins b * H * 64 elements in).  lane: which lane of the shared far region the operand takes when several are far."""
    D = H * 64
    if place == "compact":
        return _sentinel((B, L, H, 64), BF16) if output else vals.to(BF16)
    strides = (FAR_BS, D, 64, 1) if place == "bs" else (D, place[1], 64, 1)
    span = ((B - 1) * strides[0] + (L - 1) * strides[1] + D) * 2
    assert L * D * 2 + 16 < LANE
    base = None if lane is None else _ceil_to(span, LANE) + lane * LANE
    return far_view(arena, (B, L, H, 64), BF16, strides, values=vals, base_bytes=base, name=name, output=output)


def _fwd(ops, arena, p, B, H, Lq, Lk, q_log2, places, keep=None):
    """attn_fwd with each of q, k, v, o placed as `places` says (default compact); returns (o, lse, route).  keep: a dict that receives
    the outputs BEFORE the call (a refused call raises)."""
    pl = lambda n: places.get(n, "compact")
    lane = (lambda i: i) if len(places) > 1 else (lambda i: None)
    q = _attn_operand(arena, p["q"], B, Lq, H, pl("q"), "q", lane(0))
    k = _attn_operand(arena, p["k"], B, Lk, H, pl("k"), "k", lane(1))
    v = _attn_operand(arena, p["v"], B, Lk, H, pl("v"), "v", lane(2))
    o = _attn_operand(arena, None, B, Lq, H, pl("o"), "o", lane(3), output=True)
    lse = _sentinel((B, H, Lq), F32)
    if keep is not None:
        keep.update(o=o, lse=lse)
    with _Routes() as r:
        ops.attn_fwd(q, k, v, o, lse, q_log2=q_log2)
    return o, lse, r.seen[0]


@pytest.mark.parametrize("q_log2", [False, True], ids=["occ4", "occ4_spec"])
@pytest.mark.parametrize("Lq,Lk", ATTN_SHAPES)
def test_attn_fwd_far_strides(ops, arena, Lq, Lk, q_log2):
    """B = 2, H = 2.  Far batch stride on q, k, v, o in turn and on all four; far row stride on K and on V at the limit of the 32-bit tile
    offsets (right: the same body, bit-equal to the compact call) and one step past it (refused before any launch: o and lse
    untouched, and the compact call afterwards gives the same bits as before).  Bounds of test_attn_fwd: lse 2e-3, o 2e-2."""
    from ts_asr_whisper_amd import _lib as L
    B, H = 2, 2
    route = "occ4_spec" if q_log2 else "occ4"
    p = _attn_problem(B, H, Lq, Lk, q_log2)
    o0, lse0, r0 = _fwd(ops, arena, p, B, H, Lq, Lk, q_log2, {})
    assert r0 == route
    cases = [{n: "bs"} for n in ("q", "k", "v", "o")] + [{n: "bs" for n in ("q", "k", "v", "o")}]
    cases += [{n: ("rs", attn_rs_limit(Lk))} for n in ("k", "v")]
    rs31, row31 = tall_ld(Lk, H * 64, 2, 8, mark=MARK31)               # a key row begins less than a row below 2^31 and straddles it
    assert row31 is not None
    cases += [{n: ("rs", rs31)} for n in ("k", "v")]
    for places in cases:
        arena.reset()
        clock = _Clock()
        o, lse, r = _fwd(ops, arena, p, B, H, Lq, Lk, q_log2, places)
        assert r == route, (places, r)
        arena.check()
        _same_bits(o, o0, places), _same_bits(lse, lse0, places)
        e_o, e_lse = _err(o, p["o"]), _err(lse, p["lse"])
        _record(f"attn_fwd ({Lq},{Lk}) {places if len(places) < 4 else 'all four bs'}", route, e_o, 2e-2, arena, clock)
        assert e_lse < 2e-3 and e_o < 2e-2, (places, e_lse, e_o)
    for n in ("k", "v"):
        places = {n: ("rs", attn_rs_limit(Lk) + 8)}
        for o_place in ("bs", "compact"):
            arena.reset()
            keep = {}
            with pytest.raises(L.DicowError, match=r"2\^32"):
                _fwd(ops, arena, p, B, H, Lq, Lk, q_log2, dict(places, o=o_place), keep)
            arena.check()                                                                 # the inputs' words only
            assert _nonsentinel_words(keep["o"]) == 0 and _nonsentinel_words(keep["lse"]) == 0, "a refused call wrote an output"
        o, lse, _ = _fwd(ops, arena, p, B, H, Lq, Lk, q_log2, {})
        _same_bits(o, o0, "after a refusal"), _same_bits(lse, lse0, "after a refusal")
        print(f"far_offsets: attn_fwd ({Lq},{Lk}) {n} row stride {attn_rs_limit(Lk) + 8}: refused (DICOW_ERR_INVALID), outputs untouched")


BWD_IN = ("q", "k", "v", "o", "d_o")
BWD_OUT = ("dq", "dk", "dv")


def _bwd(ops, arena, p, fwd, B, H, Lq, Lk, fused, places, keep=None):
    pl = lambda n: places.get(n, "compact")
    many = len(places) > 1
    vals = dict(q=p["q"], k=p["k"], v=p["v"], o=fwd[0], d_o=p["d_o"])
    Ls = dict(q=Lq, k=Lk, v=Lk, o=Lq, d_o=Lq, dq=Lq, dk=Lk, dv=Lk)
    t = {}
    for i, n in enumerate(BWD_IN + BWD_OUT):
        t[n] = _attn_operand(arena, vals.get(n), B, Ls[n], H, pl(n), n, i if many else None, output=n in BWD_OUT)
    delta = torch.zeros(2, B, H, Lq, device="cuda")
    if keep is not None:
        keep.update({n: t[n] for n in BWD_OUT}, delta=delta)
    with _Routes() as r:
        ops.attn_bwd(t["q"], t["k"], t["v"], t["o"], t["d_o"], fwd[1], delta, t["dq"], t["dk"], t["dv"], dq_scale=0.5, fused=fused)
    if fused:
        assert ops.attn_bwd_fused_status() == 0
    return {n: t[n] for n in BWD_OUT}, r.seen[0]


@pytest.mark.parametrize("fused", [False, "force"], ids=["dq_dkv", "fused"])
@pytest.mark.parametrize("Lq,Lk", ATTN_SHAPES)
def test_attn_bwd_far_strides(ops, arena, Lq, Lk, fused):
    """The backward, two-kernel form and the fused kernel forced (dense): far batch stride on each of q, k, v, o, d_o, dq, dk, dv and on
    all eight; far row stride on K, V, Q and dO at the limit (bit-equal to compact) and one step past it (refused, dq / dk / dv
    untouched, the library usable afterwards).  Bound of test_attn_bwd: 2e-2 max(1, |ref|)."""
    from ts_asr_whisper_amd import _lib as L
    B, H = 2, 2
    route = "fused" if fused else "dq_dkv"
    p = _attn_problem(B, H, Lq, Lk, False)
    fwd = _fwd(ops, arena, p, B, H, Lq, Lk, False, {})[:2]
    g0, r0 = _bwd(ops, arena, p, fwd, B, H, Lq, Lk, fused, {})
    assert r0 == route
    Ls = dict(q=Lq, k=Lk, v=Lk, d_o=Lq)
    cases = [{n: "bs"} for n in BWD_IN + BWD_OUT] + [{n: "bs" for n in BWD_IN + BWD_OUT}]
    cases += [{n: ("rs", attn_rs_limit(Ls[n]))} for n in ("k", "v", "q", "d_o")]
    for n in ("k", "v", "q", "d_o"):                                   # ... and with a row that straddles 2^31
        rs31, row31 = tall_ld(Ls[n], H * 64, 2, 8, mark=MARK31)
        assert row31 is not None
        cases.append({n: ("rs", rs31)})
    tol = lambda ref: 2e-2 * max(1.0, float(ref.abs().max()))
    for places in cases:
        arena.reset()
        clock = _Clock()
        g, r = _bwd(ops, arena, p, fwd, B, H, Lq, Lk, fused, places)
        assert r == route, (places, r)
        arena.check()
        worst = 0.0
        for n in BWD_OUT:
            _same_bits(g[n], g0[n], (places, n))
            e = _err(g[n], p[n])
            worst = max(worst, e / tol(p[n]))
            assert e < tol(p[n]), (places, n, e)
        _record(f"attn_bwd ({Lq},{Lk}) {places if len(places) < 8 else 'all eight bs'}", route, worst, 1.0, arena, clock)
    for n in ("k", "v", "q", "d_o"):
        arena.reset()
        places = {n: ("rs", attn_rs_limit(Ls[n]) + 8), "dq": "bs"}
        keep = {}
        with pytest.raises(L.DicowError, match=r"2\^32"):
            _bwd(ops, arena, p, fwd, B, H, Lq, Lk, fused, places, keep)
        arena.check()
        assert all(_nonsentinel_words(keep[m]) == 0 for m in BWD_OUT) and not bool(keep["delta"].any()), "a refused call wrote an output"
        g, _ = _bwd(ops, arena, p, fwd, B, H, Lq, Lk, fused, {})
        for m in BWD_OUT:
            _same_bits(g[m], g0[m], "after a refusal")
        print(f"far_offsets: attn_bwd ({Lq},{Lk}) {route} {n} row stride {attn_rs_limit(Ls[n]) + 8}: refused (DICOW_ERR_INVALID), outputs untouched")


@pytest.mark.parametrize("ancestry", [False, True], ids=["shared", "ancestry"])
def test_attn_decode_far_slots(ops, arena, ancestry):
    """(B0, group, H, Lk) = (2, 4, 3, 70).  Shared mode: k_bs / v_bs put slot 1 past 2^32 bytes.  Ancestry mode: 8 slots at a stride that
    puts slot 7 past 2^32, the table mixing slots 0 and 7 (and the others).  Bit-equal to the compact caches; bound of
    test_gpu_attn_decode: 2e-2."""
    B0, group, H, Lk = 2, 4, 3, 70
    D, R = H * 64, B0 * group
    n_slots = R if ancestry else B0
    g = torch.Generator().manual_seed(100 + Lk + group)
    q = torch.randn(R, H, 64, generator=g).mul(0.5).to(BF16).cuda()
    k, v = torch.randn(n_slots, Lk, H, 64, generator=g).to(BF16).cuda(), torch.randn(n_slots, Lk, H, 64, generator=g).to(BF16).cuda()
    anc = None
    if ancestry:
        anc = torch.randint(0, R, (R, Lk), generator=g)
        anc[:, ::2] = torch.where(torch.arange(R)[:, None] % 2 == 0, 0, 7)                # every row mixes slot 0 or slot 7 in
        t = torch.arange(Lk)[None, :]
        kg, vg = k.cpu()[anc, t], v.cpu()[anc, t]
        anc = anc.to(torch.int32).cuda()
    else:
        kg, vg = k.cpu().repeat_interleave(group, dim=0), v.cpu().repeat_interleave(group, dim=0)
    s = torch.einsum("rhd,rthd->rht", q.cpu().double(), kg.double())
    ref = torch.einsum("rht,rthd->rhd", torch.softmax(s, -1), vg.double()).cuda()
    bs = _ceil_to(MARK32 // 2 // (n_slots - 1) + 8, 8)
    assert (n_slots - 1) * bs * 2 >= MARK32
    kw = dict(group=1 if ancestry else group, anc=anc)
    o0 = _sentinel((R, H, 64), BF16)
    ops.attn_decode(q, k, v, o0, **kw)
    for far in (("k",), ("v",), ("k", "v")):
        arena.reset()
        clock = _Clock()
        kd = far_view(arena, (n_slots, Lk, H, 64), BF16, (bs, D, 64, 1), values=k, name="k") if "k" in far else k
        vd = far_view(arena, (n_slots, Lk, H, 64), BF16, (bs, D, 64, 1), values=v, name="v") if "v" in far else v
        o = _sentinel((R, H, 64), BF16)
        ops.attn_decode(q, kd, vd, o, **kw)
        arena.check()
        _same_bits(o, o0, far)
        e = _err(o, ref)
        _record(f"attn_decode (2,4,3,70) {'ancestry' if ancestry else 'shared'} far {'+'.join(far)}", "attn_decode", e, 2e-2, arena, clock)
        assert e < 2e-2


# ================================================================================================ CE loss
CE_ROWS, CE_V, CE_NTS = 44, 1000, 150


def _ce_problem(device="cuda"):
    """44 rows of V = 1000 (150 timestamp ids at the end): every label pattern of test_gpu_losses._ce_rows on Gaussian logits."""
    from tests.test_gpu_losses import _ts_vocab
    from ts_asr_whisper_amd.modeling import build_ts_tables
    g = torch.Generator().manual_seed(1044)
    nt = CE_V - CE_NTS
    z = (torch.randn(CE_ROWS, CE_V, generator=g) * 2).bfloat16()
    lab, upp = [], []
    for i in range(CE_ROWS):
        a, b = (1 + 37 * i) % nt, (nt - 2 - 53 * i) % nt
        t0, tm, tl = nt, nt + CE_NTS // 2, CE_V - 1
        pats = [(a, b), (a, a), (a, -100), (-100, b), (-100, -100), (t0, a), (a, tl), (tm, tm + 3), (tl, t0), (tm, -100), (t0, t0)]
        lab.append(pats[i % len(pats)][0]), upp.append(pats[i % len(pats)][1])
    ts = build_ts_tables(_ts_vocab(CE_V, CE_NTS), CE_V, device)
    return z, torch.tensor(lab), torch.tensor(upp), ts, (ts["ids"].long().cpu(), ts["w"].double().cpu())


def _ce_run(ops, arena, z, lab, upp, soft, ts, far, backward):
    from tests.test_gpu_losses import CE_SCALE
    R, V = z.shape
    ld, row = tall_ld(R, V, 2) if far else (V, None)
    logits = far_view(arena, (R, V), BF16, (ld, 1), values=z, name="logits") if far else z.cuda()
    d = None
    if backward:                                                       # (the kernel writes all ld columns of a row: zeros past V)
        d = far_view(arena, (R, ld), BF16, (ld, 1), name="d_logits", output=True) if far else _sentinel((R, ld), BF16)
    lse, row_loss, acc = _sentinel((R,), F32), _sentinel((R,), F32), torch.zeros(2, device="cuda")
    choice = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    labd, uppd, scale = lab.cuda(), upp.cuda(), torch.full((1,), CE_SCALE, device="cuda")
    a = ops.ce_args(logits, ld, R, V, labd, uppd, soft, ts, lse, row_loss, choice, acc[0:1], acc[1:2], d)
    ops.ce_loss_fwd(a)
    if backward:
        ops.ce_loss_bwd(a, scale)
    torch.cuda.synchronize()
    res = dict(lse=lse.cpu(), row_loss=row_loss.cpu(), choice=choice.cpu(), acc=acc.cpu())
    if backward:
        for r in range(R if ld > V else 0):                            # row by row: the pad is 100 MB a row
            assert not bool(d[r, V:].view(torch.int16).any()), "d_logits pad columns must be exactly zero"
        res["d"] = d[:, :V].contiguous().cpu()
    return res, row


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "fwd_bwd"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_ce_loss_far_logits(ops, arena, soft, backward):
    """logits in a tall view (a row straddles 2^32, the middle rows begin around 2^31); the backward writes d_logits with the SAME ld, so it
    is a second tall view.  One body: bit-equal to the compact call, and test_gpu_losses' parity (FP32_TOL, A_CE) through its own
    _ce_check.  The backward's output is whole rows of ld columns (zeros past V): the stray count covers all of them."""
    from tests.test_gpu_losses import FP32_TOL, _ce_check
    z, lab, upp, ts, ts_ref = _ce_problem()
    plain, _ = _ce_run(ops, arena, z, lab, upp, soft, ts if soft else None, False, True)
    arena.reset()
    clock = _Clock()
    got, row = _ce_run(ops, arena, z, lab, upp, soft, ts if soft else None, True, backward)
    assert row is not None
    arena.check()
    for k in got:
        _same_bits(got[k], plain[k], k)
    ref = ce_ref(z.double(), lab, upp, soft, ts_ref if soft else None)
    if not backward:
        got = dict(got, d=plain["d"])
    _ce_check(f"ce far {'soft' if soft else 'hard'}", got, ref)
    e = float(((got["lse"].double() - ref["lse"]).abs() / ref["lse"].abs().clamp(min=1.0)).max())
    _record(f"ce_loss {'fwd+bwd' if backward else 'fwd'} {'soft' if soft else 'hard'} far logits", "ce_loss", e, FP32_TOL, arena, clock)


def test_control_ce_far_logits_wrapped_rows_are_flagged(arena):
    """No kernel runs: the fp64 reference on the rows the arena holds at each logits row's offset mod 2^32 misses _ce_check."""
    from tests.test_gpu_losses import CE_SCALE, _ce_check
    z, lab, upp, _, _ = _ce_problem()
    ld, _ = tall_ld(CE_ROWS, CE_V, 2)
    view = far_view(arena, (CE_ROWS, CE_V), BF16, (ld, 1), values=z, name="logits")
    zw = _rows_at_wrapped_offsets(arena, view, CE_ROWS, CE_V, ld).cpu()
    assert 0 < int((_bits(zw) == _bits(z)).all(1).sum()) < CE_ROWS
    ref, rw = ce_ref(z.double(), lab, upp, False, None), ce_ref(zw.double(), lab, upp, False, None)
    fake = dict(lse=rw["lse"].float(), row_loss=rw["row_loss"].float(), choice=rw["choice"], d=(rw["grad"] * CE_SCALE).bfloat16(),
                acc=torch.tensor([float(rw["row_loss"].sum()), float(rw["count"])]))
    with pytest.raises(AssertionError):
        _ce_check("control", fake, ref)


# ================================================================================================ ctc_frame_lse, column sums, casts
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_ctc_frame_lse_far_ld(arena, dtype):
    """40 rows of V1 = 37 (the row patterns of test_frame_lse_vs_fp64, seven draws) at a tall ld: bit-equal to compact rows and inside that
    test's derived bound (_lse_bound)."""
    from ts_asr_whisper_amd import _lib as L
    from tests.test_gpu_ctc_prefix_edges import _lse_bound, _lse_rows
    V1, R = 37, 40
    vals = torch.cat([_lse_rows(V1, torch.Generator().manual_seed(300 + i)) for i in range(7)])[:R].to(dtype).float()
    ld, row = tall_ld(R, V1, 2 if dtype == BF16 else 4, 8)
    x0 = vals.to(dtype).cuda()
    lse0, lse = _sentinel((R,), F32), _sentinel((R,), F32)
    L.call("dicow_ctc_frame_lse", x0.data_ptr(), int(dtype == BF16), R, V1, V1, lse0.data_ptr(), L.stream())
    clock = _Clock()
    x = far_view(arena, (R, V1), dtype, (ld, 1), values=vals, name="logits")
    L.call("dicow_ctc_frame_lse", x.data_ptr(), int(dtype == BF16), R, V1, ld, lse.data_ptr(), L.stream())
    arena.check()
    assert row is not None
    _same_bits(lse, lse0, "lse")
    z64 = ctc_prefix_ref.to64(vals)
    want = ctc_prefix_ref.frame_lse(z64, V1)
    bound = _lse_bound(z64, V1, want)
    err = np.abs(lse.cpu().numpy().astype(np.float64) - want)
    _record(f"ctc_frame_lse 40 x 37 {dtype} far ld", "ctc_frame_lse_kernel", float((err / bound).max()), 1.0, arena, clock)
    assert bool(np.isfinite(lse.cpu().numpy()).all()) and bool((err <= bound).all()), (err, bound)


def test_colsum_bf16_far_ld(ops, arena):
    """(100 x 514) at a tall ld: bit-equal to the compact call, inside test_colsum_bf16's bound (glue_ref.sum_bound, rows + 1 terms)."""
    rows, N = 100, 514
    x = glue_ref.rand((rows, N), 200 + rows + N, 1.0).to(BF16)
    out0 = glue_ref.rand((N,), 201, 2.0)
    ld, row = tall_ld(rows, N, 2, 8)
    o0, o = out0.cuda().clone(), out0.cuda().clone()
    ops.colsum_bf16(x.cuda(), o0)
    clock = _Clock()
    xd = far_view(arena, (rows, N), BF16, (ld, 1), values=x, name="x")
    ops.colsum_bf16(xd, o)
    arena.check()
    assert row is not None
    _same_bits(o, o0, "colsum")
    terms = torch.cat((out0[None].double(), x.double()), 0)
    ref = terms.sum(0)
    frac = float(((o.cpu().double() - ref).abs() / glue_ref.sum_bound(terms.abs().sum(0), rows + 1, ref)).max())
    _record("colsum_bf16 100 x 514 far ld", "colsum_bf16", frac, 1.0, arena, clock)
    assert frac <= 1.0


@pytest.mark.parametrize("far", ["ld", "ld_t", "both"])
def test_cast_transpose_far_ld(ops, arena, far):
    """fp32 (200 x 136) -> bf16 [200, 136] at a tall ld and / or bf16 [136, 200] at a tall ld_t: exactly torch's rounding
    (test_cast_transpose), every word of both outputs written and no other (pad columns stay untouched)."""
    Rr, Cc = 200, 136
    w = torch.randn(Rr, Cc, generator=torch.Generator().manual_seed(Rr + Cc))
    ref = w.to(BF16).cuda()
    clock = _Clock()
    ld, r1 = tall_ld(Rr, Cc, 2, 8) if far in ("ld", "both") else (Cc, 0)
    ld_t, r2 = tall_ld(Cc, Rr, 2, 8) if far in ("ld_t", "both") else (Rr, 0)
    out = far_view(arena, (Rr, Cc), BF16, (ld, 1), name="out", output=True) if ld != Cc else _sentinel((Rr, Cc), BF16)
    out_t = far_view(arena, (Cc, Rr), BF16, (ld_t, 1), name="out_t", output=True) if ld_t != Rr else _sentinel((Cc, Rr), BF16)
    ops.cast_transpose_bf16(w.cuda(), out, out_t, ld=ld, ld_t=ld_t)
    arena.check()
    assert r1 is not None and r2 is not None
    _same_bits(out, ref, "out"), _same_bits(out_t, ref.t(), "out_t")
    _record(f"cast_transpose 200 x 136 far {far}", "cast_transpose", 0.0, 0.0, arena, clock)


# ================================================================================================ flat kernels past 2^31 ELEMENTS
# The operands are compact views of the arena (nothing else of that size is allocated): the output first, at least its own span in, the
# inputs behind it -- an fp32 input of 8.6 GB begins 8.6 GB in, past the 8 GiB cap of the front pad.  Inputs are generated in place.
FLAT_N = (1 << 31) + 1027          # the element index passes `int`; the byte offsets pass 2^32 (bf16) and 2^33 (fp32)
FLAT_CHUNK = 1 << 27


def _randn_fill(scale, seed):
    def fill(view):
        g = torch.Generator(device="cuda").manual_seed(seed)
        for s in range(0, view.numel(), FLAT_CHUNK):
            m = min(view.numel(), s + FLAT_CHUNK) - s
            view[s:s + m] = (torch.randn(m, generator=g, device="cuda") * scale).to(view.dtype)
    return fill


def _tile_fill(tile):
    def fill(view):
        reps = FLAT_CHUNK // tile.numel()
        for s in range(0, view.numel(), FLAT_CHUNK):
            m = min(view.numel(), s + FLAT_CHUNK) - s
            view[s:s + m] = tile.repeat(reps)[:m]
    return fill


def _flat_record(case, body, err, bound, arena, ms):
    print(f"far_offsets: {case:<62s} body={body:<30s} err={err:.3e} bound={bound:.3e} arena_bytes={arena.used} wall_ms={ms:.0f}")


def test_cast_f32_to_bf16_past_int_elements(ops, arena):
    """n = 2^31 + 1027 (a 3-element scalar tail past the mark): every output element equals torch's rounding, compared in chunks, and
    nothing but the n output words was written."""
    t0 = _Clock()
    out = far_view(arena, (FLAT_N,), BF16, (1,), name="out", output=True)
    x = far_view(arena, (FLAT_N,), F32, (1,), name="x", fill=_randn_fill(3.0, 5))
    ops.cast_bf16(x, out=out)
    arena.check()
    for s in range(0, FLAT_N, FLAT_CHUNK):
        e = min(FLAT_N, s + FLAT_CHUNK)
        assert torch.equal(_bits(out[s:e]), _bits(x[s:e].to(BF16))), f"cast differs in elements [{s}, {e})"
    _flat_record("cast_f32_to_bf16 n=2^31+1027", "cast_f32_bf16_kernel", 0.0, 0.0, arena, t0.ms())


def test_sumsq_f32_past_int_elements(ops, arena):
    """n = 2^31 + 1027 against the chunked fp64 sum on the device, at test_sumsq's bound (glue_ref.sum_bound, n + 1 product terms); and
    exactly, with x in {-1, 0, 1} laid out so that every partial sum is a whole number below 2^24 -- a lost block would show."""
    t0 = _Clock()
    x = far_view(arena, (FLAT_N,), F32, (1,), name="x", fill=_randn_fill(1.0, 5))
    out = torch.tensor([2.5], device="cuda")
    ops.sumsq(x, out)
    arena.check()
    ss = sum(float((x[s:s + FLAT_CHUNK].double() ** 2).sum()) for s in range(0, FLAT_N, FLAT_CHUNK))
    ref = 2.5 + ss
    bound = float(glue_ref.sum_bound(2.5 + ss, FLAT_N + 1, ref, product_terms=True))
    frac = abs(float(out) - ref) / bound
    _flat_record("sumsq_f32 n=2^31+1027", "sumsq_kernel", frac, 1.0, arena, t0.ms())
    assert frac <= 1.0, frac
    ones = (FLAT_N - 1) // 1024 + 1                                    # every 1024th element, the last one past 2^31: 2097154 < 2^24
    x.zero_()
    x[::1024] = 1.0
    x[FLAT_N - 1] = -1.0                                               # (the last element of the scalar tail)
    out = torch.tensor([3.0], device="cuda")
    ops.sumsq(x, out)
    assert float(out) == 3.0 + ones + 1, (float(out), ones)


def test_gelu_bwd_bf16_past_int_elements(ops, arena):
    """n = 2^31 + 1028 (the kernel takes multiples of 4): g * gelu'(pre) against the fp64 product, chunk by chunk, at
    test_gelu_bwd_bf16's bound (one bf16 rounding + A_GELU_BWD, a constant measured for |g| <= 1: the inputs are those of
    test_gelu_bwd_bf16_past_the_grid_cap -- pre tiles every bf16 value of [-9, 9], g alternates 1 / -0.37)."""
    from tests.test_gpu_glue_kernels import A_GELU_BWD, _resid_bf16
    n = FLAT_N + 1
    t0 = _Clock()
    out = far_view(arena, (n,), BF16, (1,), name="out", output=True)
    pre = far_view(arena, (n,), BF16, (1,), name="pre", fill=_tile_fill(glue_ref.gelu_pre_grid(65536).cuda()))
    g = far_view(arena, (n,), BF16, (1,), name="g", fill=_tile_fill(torch.tensor([1.0, -0.37], device="cuda").to(BF16)))
    ops.gelu_bwd_bf16(g, pre, out)
    arena.check()
    worst = 0.0
    for s in range(0, n, FLAT_CHUNK // 4):
        e = min(n, s + FLAT_CHUNK // 4)
        a = _resid_bf16(out[s:e], g[s:e].double() * glue_ref.gelu_grad_ref(pre[s:e]))
        assert a <= A_GELU_BWD, (s, a)
        worst = max(worst, a)
    _flat_record("gelu_bwd_bf16 n=2^31+1028", "gelu_bwd_bf16_kernel", worst, A_GELU_BWD, arena, t0.ms())


# ================================================================================================ grouped casts, conv view, TN segments and group
def test_cast_transpose_group_one_far_problem(ops, arena):
    """dicow_cast_transpose_group (one pooled launch) with two problems: (200 x 136) into tall ld / ld_t views, (128 x 64) compact.
    Exactly torch's rounding in all four outputs, and nothing else written."""
    g = torch.Generator().manual_seed(77)
    w0, w1 = torch.randn(200, 136, generator=g).cuda(), torch.randn(128, 64, generator=g).cuda()
    ld, r1 = tall_ld(200, 136, 2, 8)
    ld_t, r2 = tall_ld(136, 200, 2, 8)
    clock = _Clock()
    o0 = far_view(arena, (200, 136), BF16, (ld, 1), name="out", output=True)
    o0t = far_view(arena, (136, 200), BF16, (ld_t, 1), name="out_t", output=True)
    o1, o1t = _sentinel((128, 64), BF16), _sentinel((64, 128), BF16)
    with ops.cast_group():
        ops.cast_transpose_bf16(w0, o0, o0t, ld=ld, ld_t=ld_t)
        ops.cast_transpose_bf16(w1, o1, o1t)
    arena.check()
    assert r1 is not None and r2 is not None
    _same_bits(o0, w0.to(BF16), "out"), _same_bits(o0t, w0.to(BF16).t(), "out_t")
    _same_bits(o1, w1.to(BF16), "compact out"), _same_bits(o1t, w1.to(BF16).t(), "compact out_t")
    _record("cast_transpose_group 200 x 136 far + 128 x 64 compact", "cast_transpose4_group_kernel", 0.0, 0.0, arena, clock)


def test_gemm_nt_batched_conv_view_far_batch_strides(ops, arena):
    """The batched conv view of test_gemm_nt_batched_strided_conv_view (B = 3, L = 200, C = O = 128: overlapping time-major rows, lda =
    2 C) with strideA and strideC past 2^32 bytes: utterances 1 and 2 lie 4 and 8 GiB from the base.  Same body as compact
    (gemm_nt64), bit-equal, bound 2e-4 of that test."""
    Bn, Ln, Cc, Oc = 3, 200, 128, 128
    K, T2 = 3 * Cc, Ln // 2
    g = torch.Generator().manual_seed(9)
    x = _bf(torch.randn(Bn, Cc, Ln, generator=g))
    w = _bf(torch.randn(Oc, Cc, 3, generator=g) * (3 * Cc) ** -0.5)
    bias = torch.randn(Oc, generator=g).cuda()
    ref = torch.nn.functional.conv1d(x.double(), w.double(), bias.double().cpu(), stride=2, padding=1).permute(0, 2, 1).cuda()
    xt = torch.zeros(Bn, Ln + 2, Cc)
    xt[:, 1:Ln + 1] = x.permute(0, 2, 1)
    wp = ops.conv_weight_pack(w.cuda(), K)
    plain = _sentinel((Bn, T2, Oc), F32)
    ran_plain = _launched(ops, lambda: ops.gemm_nt(xt.cuda().bfloat16(), wp, plain, T2, Oc, K, lda=2 * Cc, bias=bias, batch=Bn,
                                                   strideA=(Ln + 2) * Cc, strideC=T2 * Oc))
    sA, sC = _ceil_to(MARK32 // 2 + 8, 8), _ceil_to(MARK32 // 4 + 4, 4)                   # elements of bf16 / of fp32: just past 2^32 bytes
    for far in (("A",), ("C",), ("A", "C")):
        arena.reset()
        clock = _Clock()
        xd = far_view(arena, (Bn, Ln + 2, Cc), BF16, (sA, Cc, 1), values=xt, name="x") if "A" in far else xt.cuda().bfloat16()
        # (both far: the batch strides are the same number of bytes, so the output takes a lane 1 MiB behind the input's blocks)
        ob = xd.data_ptr() - arena.buf.data_ptr() + (1 << 20) if far == ("A", "C") else None
        od = far_view(arena, (Bn, T2, Oc), F32, (sC, Oc, 1), name="out", output=True, base_bytes=ob) if "C" in far else _sentinel((Bn, T2, Oc), F32)
        ran = _launched(ops, lambda: ops.gemm_nt(xd, wp, od, T2, Oc, K, lda=2 * Cc, bias=bias, batch=Bn,
                                                 strideA=sA if "A" in far else (Ln + 2) * Cc, strideC=sC if "C" in far else T2 * Oc))
        assert ran == ran_plain and len(ran) == 1 and ran[0].startswith("gemm_nt64_kernel"), (ran, ran_plain)
        arena.check()
        _same_bits(od, plain, far)
        e = _err(od, ref)
        _record(f"gemm_nt batched conv view far stride{'+'.join(far)}", ran[0], e, 2e-4, arena, clock)
        assert e < 2e-4


def test_gemm_tn_far_c_seg(ops, arena):
    """(1500, 384, 136) in row segments of 128 (TN_CASES "seg_split": one reduce launch per segment): each segment a tall view of its
    own (ldc is one argument for all of them).  Bit-equal to compact segments; bound 2e-4 max(1, |ref|)."""
    Mk, N1, N2, seg = 1500, 384, 136, 128
    A, B, ref, bound = _tn_problem(Mk, N1, N2)
    plain = [_sentinel((seg, N2), F32) for _ in range(3)]
    ran_plain = _launched(ops, lambda: ops.gemm_tn(A, B, plain[0], Mk, N1, N2, accumulate=False, C_seg=plain[1:], seg_rows=seg))
    ldc, row = tall_ld(seg, N2, 4, 4)
    clock = _Clock()
    segs = [far_view(arena, (seg, N2), F32, (ldc, 1), name=f"C_seg{i}", output=True) for i in range(3)]       # (one ldc for all segments)
    ran = _launched(ops, lambda: ops.gemm_tn(A, B, segs[0], Mk, N1, N2, ldc=ldc, accumulate=False, C_seg=segs[1:], seg_rows=seg))
    assert ran == ran_plain and row is not None, (ran, ran_plain, row)
    arena.check()
    got = torch.cat([t.contiguous() for t in segs], 0)
    _same_bits(got, torch.cat(plain, 0), "segments")
    e = _err(got, ref)
    _record("gemm_tn (1500,384,136) far C_seg x 3", "+".join(ran), e, bound, arena, clock)
    assert e < bound


def test_gemm_tn_group_one_far_member(ops, arena):
    """dicow_gemm_tn_group with the three problems of test_gemm_tn_pooled_group (Mk = 136, pooled into one gemm_tn256g launch), the
    middle one with a far A: just under Mk * lda * 2 = 2^32 the pooled kernel still runs and every result is bit-equal to the compact
    group; at 2^32 tn_group_plan refuses to pool (problem by problem through dicow_gemm_tn; the far member's own 256-tile guard is
    test_gemm_tn_far_a_b_around_the_256_tile_guard's) and parity holds at 2e-4 max(1, |ref|)."""
    Mk = 136
    probs = [(1800, 2048), (2048, 3000), (2048, 3200)]
    g = torch.Generator().manual_seed(3)
    data = []
    for N1, N2 in probs:
        A, B = torch.randn(Mk, N1, generator=g).to(BF16).cuda(), torch.randn(Mk, N2, generator=g).to(BF16).cuda()
        data.append((A, B, A.double().t() @ B.double()))

    def run(lda_far):
        grp, outs = ops.TnGroup(), []
        for i, ((N1, N2), (A, B, _)) in enumerate(zip(probs, data)):
            Cd = _sentinel((N1, N2), F32)
            if i == 1 and lda_far:
                grp.add(far_view(arena, (Mk, N1), BF16, (lda_far, 1), values=A, name="A1"), B, Cd, Mk, N1, N2, lda=lda_far, accumulate=False)
            else:
                grp.add(A, B, Cd, Mk, N1, N2, accumulate=False)
            outs.append(Cd)
        return outs, _launched(ops, grp.run)

    plain, ran_plain = run(None)
    assert ran_plain == ["gemm_tn256g_kernel"], ran_plain
    ld_in = (MARK32 - 1) // (2 * Mk) // 8 * 8
    assert Mk * ld_in * 2 < MARK32 <= Mk * (ld_in + 8) * 2
    for ld, inside in ((ld_in, True), (ld_in + 8, False)):
        arena.reset()
        clock = _Clock()
        outs, ran = run(ld)
        arena.check()
        if inside:
            assert ran == ran_plain, ran
        else:
            assert "gemm_tn256g_kernel" not in ran and len(ran) >= 3, ran
        worst = 0.0
        for i, (_, _, ref) in enumerate(data):
            if inside:
                _same_bits(outs[i], plain[i], ("group", i))
            e, bound = _err(outs[i], ref), 2e-4 * max(1.0, float(ref.abs().max()))
            worst = max(worst, e / bound)
            assert e < bound, (i, ld, e, bound)
        _record(f"gemm_tn_group 3 problems, far A of #1 lda={ld} ({'inside' if inside else 'at'} 2^32)", "+".join(sorted(set(ran))), worst, 1.0, arena, clock)


# ================================================================================================ CTC: greedy decode and the loss
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("far", ["batch_stride", "ld"])
def test_ctc_greedy_decode_far_logits(arena, far, dtype):
    """B = 3, Tn = 65, V1 = 37 in rows of 128, read in place.  batch_stride: utterances 1 and 2 lie 4 and 8 GiB from the base; ld: a
    tall row stride (the utterances interleaved, 128 elements apart), so the frames of every utterance lie on both sides of both
    marks.  The result is integers: equal to tests/ctc_greedy_ref.greedy_restatement and to the compact call."""
    from tests.ctc_greedy_ref import greedy_restatement
    from ts_asr_whisper_amd.ctc_decoding import ctc_greedy_decode
    B, Tn, V1, blank, pad = 3, 65, 37, 36, -100
    g = torch.Generator().manual_seed(65 + V1)
    vals = (torch.randn(B, Tn, V1, generator=g) * 2).to(dtype)
    vals[:, 10:14] = vals[:, 9:10]                                     # repeats to merge
    vals[:, 20:25, blank] = 30.0                                       # a run of blanks
    isz = vals.element_size()
    if far == "batch_stride":
        strides = (_ceil_to(MARK32 // isz + 128, 128), 128, 1)
    else:
        strides = (128, tall_ld(Tn, V1, isz, 8)[0], 1)
    want = greedy_restatement(vals.float(), blank, pad)
    plain = ctc_greedy_decode(vals.cuda(), blank, pad)
    clock = _Clock()
    x = far_view(arena, (B, Tn, V1), dtype, strides, values=vals, name="logits")
    assert (B - 1) * strides[0] * isz >= MARK32 or (Tn - 1) * strides[1] * isz >= MARK32
    out = torch.full((B, Tn), -7, dtype=torch.int64, device="cuda")
    ctc_greedy_decode(x, blank, pad, out=out)
    arena.check()
    assert torch.equal(out, plain) and torch.equal(out.cpu(), want)
    _record(f"ctc_greedy_decode 3 x 65 x 37 {dtype} far {far}", "ctc_greedy", 0.0, 0.0, arena, clock)


def test_ctc_loss_far_logits(ops, arena):
    """dicow_ctc_loss_fwd / _bwd on B = 2, Tn = 20, C = 12 (40 rows) with the logits in a tall view; d_logits shares ld, so it is a second
    tall view of whole ld-wide rows.  Bit-equal to test_gpu_losses._ctc_call on exactly sized buffers; parity at that file's FP32_TOL
    and A_CTC against tests/loss_ref.ctc_ref."""
    from tests.loss_ref import ctc_ref
    from tests.test_gpu_losses import A_CTC, FP32_TOL, _ctc_call, _grad_resid, _rel
    B, Tn, Cc, Lc = 2, 20, 12, 4
    g = torch.Generator().manual_seed(2012)
    z = (torch.randn(B, Tn, Cc, generator=g) * 2).bfloat16()
    lab = torch.randint(0, Cc - 1, (B, Lc), generator=g)
    plain = _ctc_call(ops, z, lab, None, None)
    rows, Smax = B * Tn, 2 * Lc + 1
    ld, _ = tall_ld(rows, Cc, 2, 8)
    clock = _Clock()
    logits = far_view(arena, (rows, Cc), BF16, (ld, 1), values=z.reshape(rows, Cc), name="logits")
    d = far_view(arena, (rows, ld), BF16, (ld, 1), name="d_logits", output=True)
    o = dict(lse=_sentinel((rows,), F32), nll=_sentinel((B,), F32), tlen=_sentinel((B,), F32), alpha=_sentinel((rows, Smax), F32),
             beta=_sentinel((rows, Smax), F32))
    acc = torch.zeros(1, device="cuda")
    labd, scale = lab.cuda().contiguous(), torch.full((1,), 1.0, device="cuda")          # (the struct holds raw pointers: keep every operand referenced)
    a = ops.ctc_args(logits, ld, B, Tn, Cc, labd, o["lse"], o["alpha"], o["beta"], o["nll"], o["tlen"], acc)
    ops.ctc_loss_fwd(a)
    a.d_logits = d.data_ptr()
    ops.ctc_loss_bwd(a, scale)
    arena.check()
    for r in range(rows):
        assert not bool(d[r, Cc:].view(torch.int16).any()), "d_logits pad columns must be exactly zero"
    got = {k: v.cpu() for k, v in o.items()}
    got["loss_sum"], got["d1.0"] = acc.cpu(), d[:, :Cc].contiguous().cpu()
    for k in got:
        _same_bits(got[k], plain[k], k)
    ref = ctc_ref(z.double(), lab)
    assert bool(torch.isfinite(ref["nll"]).all())
    e_nll, e_lse = _rel(got["nll"], ref["nll"]), _rel(got["lse"], torch.logsumexp(z.double(), -1))
    a_res = _grad_resid(got["d1.0"].float().view(B, Tn, Cc), ref["grad"], 1.0)
    _record("ctc_loss fwd+bwd 2 x 20 x 12 far logits and d_logits", "ctc_loss", e_nll, FP32_TOL, arena, clock)
    assert e_nll < FP32_TOL and e_lse < FP32_TOL and a_res < A_CTC, (e_nll, e_lse, a_res)


# ================================================================================================ LoRA kernels
def _lora_place(arena, vals, shape, dtype, far, name, output=False):
    if not far:
        return _sentinel(shape, dtype) if output else vals.to(dtype).cuda()
    # (the 16-column t finds its straddling row only at a stride that would not leave room for three far operands: plain recipe there)
    ld, _ = tall_ld(shape[0], shape[1], torch.empty(0, dtype=dtype).element_size(), 8, straddle=shape[1] >= 64)
    return far_view(arena, shape, dtype, (ld, 1), values=vals, name=name, output=output)


@pytest.mark.parametrize("far", ["ldx", "ldt", "ldx_ldt"])
def test_lora_down_far(ops, arena, far):
    """Case (67, 1280, 16) of test_lora_down, dense: x through a tall ldx, t through a tall ldt, both.  Bit-equal to the compact call;
    that test's bound (bf16: 1e-2 max(1, |ref|))."""
    from tests.test_gpu_lora_kernels import _bound, _normal
    M, K, R = 67, 1280, 16
    x, v = _normal((M, K), 1), _normal((R, K), 2, K ** -0.5)
    ref = (x.double() @ v.double().T).cuda()
    t0 = ops.lora_down(x.cuda(), v.cuda(), _sentinel((M, R), BF16), 16)
    clock = _Clock()
    xd = _lora_place(arena, x, (M, K), BF16, "ldx" in far, "x")
    t = _lora_place(arena, None, (M, R), BF16, "ldt" in far, "t", output=True)
    ops.lora_down(xd, v.cuda(), t, 16)
    arena.check()
    _same_bits(t, t0, far)
    e, bound = _err(t, ref), _bound(ref, BF16)
    _record(f"lora_down (67,1280,16) far {far}", "lora_down", e, bound, arena, clock)
    assert e < bound


@pytest.mark.parametrize("far", ["ldt", "ldp", "ldy", "ldt_ldp_ldy"])
def test_lora_up_far(ops, arena, far):
    """Case (67, 1280, 16) of test_lora_up, dense, bf16, p not y: t, p and y through tall leading dimensions in turn, then all three.
    Bit-equal to the compact call; that test's bound."""
    from tests.test_gpu_lora_kernels import SCALES, _bound, _up_problem
    M, N, R, r, nseg, t, u, p, ref = _up_problem((67, 1280, 16), False, BF16)
    ref = ref.to(BF16).double().cuda()
    y0 = ops.lora_up(t.cuda(), u.cuda(), p.cuda(), _sentinel((M, N), BF16), r, SCALES)
    clock = _Clock()
    td = _lora_place(arena, t, (M, R), BF16, "ldt" in far, "t")
    pd = _lora_place(arena, p, (M, N), BF16, "ldp" in far, "p")
    y = _lora_place(arena, None, (M, N), BF16, "ldy" in far, "y", output=True)
    ops.lora_up(td, u.cuda(), pd, y, r, SCALES)
    arena.check()
    _same_bits(y, y0, far)
    e, bound = _err(y, ref), _bound(ref, BF16)
    _record(f"lora_up (67,1280,16) far {far}", "lora_up", e, bound, arena, clock)
    assert e < bound


@pytest.mark.parametrize("far", ["ldt", "ldp", "ldt_ldp"])
def test_lora_wgrad_far(ops, arena, far):
    """Case (67, 1280, 16) of test_lora_wgrad, dense, [r, N] destination, accumulate = 0: t and p through tall leading dimensions.
    Bit-equal to the compact call; that test's bound (fp32: 1e-4 max(1, |ref|))."""
    from tests.test_gpu_lora_kernels import _bound, _normal
    M, N, R, r, s = 67, 1280, 16, 16, 2.0
    t, p = _normal((M, R), 6), _normal((M, N), 7)
    ref = (s * (t.double().T @ p.double())).cuda()
    g0 = _sentinel((r, N), F32)
    ops.lora_wgrad(t.cuda(), p.cuda(), [g0], r, s, accumulate=False)
    clock = _Clock()
    td = _lora_place(arena, t, (M, R), BF16, "ldt" in far, "t")
    pd = _lora_place(arena, p, (M, N), BF16, "ldp" in far, "p")
    g = _sentinel((r, N), F32)
    ops.lora_wgrad(td, pd, [g], r, s, accumulate=False)
    arena.check()
    _same_bits(g, g0, far)
    e, bound = _err(g, ref), _bound(ref, F32)
    _record(f"lora_wgrad (67,1280,16) far {far}", "lora_wgrad", e, bound, arena, clock)
    assert e < bound


# ================================================================================================ row kernels across rows * D * 4 = 2^31
ROW_CHUNK = 1 << 16


def _row_ref_chunks(h, stw, w, b, lw, lb, dy, gres, diag):
    """The fp64 reference of a row-kernel forward + backward, ROW_CHUNK rows at a time on the device (torch autograd; shares no code with
    the kernels): yields (row slice, x, y, d h) per chunk and leaves the parameter gradients summed over ALL rows in `sums`."""
    rows, D = h.shape
    par = [t.double().requires_grad_(True) for t in (list(w) + list(b) if diag else []) + [lw, lb]]
    sums = dict(colsum=torch.zeros(D, dtype=torch.float64, device="cuda"))
    for s in range(0, rows, ROW_CHUNK):
        sl = slice(s, min(rows, s + ROW_CHUNK))
        hr = h[sl].double().requires_grad_(True)
        if diag:
            sw = stw[sl].double()
            x = sum((hr * par[c] + par[4 + c]) * sw[:, c, None] for c in range(4))
        else:
            x = hr
        y = torch.nn.functional.layer_norm(x, (D,), par[-2], par[-1])
        ((y * dy[sl].double()).sum() + (x * gres[sl].double()).sum()).backward()
        sums["colsum"] += hr.grad.sum(0)
        yield sl, x.detach(), y.detach(), hr.grad
    sums.update(dln_w=par[-2].grad, dln_b=par[-1].grad)
    if diag:
        sums.update(dw=[p.grad for p in par[:4]], db=[p.grad for p in par[4:8]])
    _row_ref_chunks.sums = sums


def _fill_rows(shape, dtype, seed):
    out = torch.empty(shape, dtype=dtype, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, shape[0], ROW_CHUNK):
        m = min(shape[0], s + ROW_CHUNK) - s
        out[s:s + m] = torch.randn(m, shape[1], generator=g, device="cuda").to(dtype)
    return out


@pytest.mark.parametrize("D,diag", [(256, True), (512, False)], ids=["fddt_ln_D256", "ln_only_D512"])
@pytest.mark.parametrize("side", [-8, 8], ids=["under", "over"])
def test_row_kernels_across_the_2gib_mark(ops, side, D, diag):
    """rows * D * 4 = 2^31 -+ 8 rows (T = 8): under the mark the FDDT + LN calls run the staged bodies (forward `staged`, backward
    `staged_bf16` / `staged_f32`), over it the guard sends them to the 64-bit generic bodies; the LN-only pair (mode 0, D = 512) crosses
    the same mark on whichever bodies the plan names.  Operands are generated on the device; EVERY row of h_out, y_bf16, g_out and
    g_out_bf16 is compared with the fp64 reference (a superset of the first, last and mark rows), the column sums with the fp64 sums
    over all rows.  Bounds: ROW_BOUNDS of test_gpu_kernels.py, the sums' scaled by sqrt(rows) as in test_row_kernel_routes_at_small_shapes."""
    from tests.test_gpu_kernels import ROW_BOUNDS
    T = 8
    rows = MARK31 // (D * 4) + side
    B = rows // T
    assert rows % T == 0 and (rows * D * 4 < MARK31) == (side < 0)
    clock = _Clock()
    gd = torch.Generator(device="cuda").manual_seed(D + side)
    rnd = lambda *s: torch.randn(*s, generator=gd, device="cuda")
    h, gres, dy = _fill_rows((rows, D), F32, 1), _fill_rows((rows, D), F32, 2), _fill_rows((rows, D), BF16, 3)
    st = torch.softmax(rnd(B, 4, T), 1).contiguous()
    stw = st.permute(0, 2, 1).reshape(rows, 4)
    w, b = [1 + 0.1 * rnd(D) for _ in range(4)], [0.1 * rnd(D) for _ in range(4)]
    lw, lb = 1 + 0.1 * rnd(D), 0.1 * rnd(D)
    new = lambda *s: torch.zeros(*s, device="cuda")
    ho, yb, mean, rstd = (_sentinel((rows, D), F32) if diag else None), _sentinel((rows, D), BF16), _sentinel((rows,), F32), _sentinel((rows,), F32)
    mode = ops.MODE_DIAG if diag else ops.MODE_NONE
    fkw = dict(stno=st, T=T, w=w, b=b) if diag else {}
    routes = {}
    with _Routes() as r:
        ops.fddt_ln_fwd(h, rows, D, mode=mode, h_out=ho, ln_w=lw, ln_b=lb, y_bf16=yb, mean=mean, rstd=rstd, **fkw)
    routes["fwd"] = r.seen[0]
    runs = {}
    for want_bf16 in (True, False):
        o = dict(g=_sentinel((rows, D), F32), gb=_sentinel((rows, D), BF16) if want_bf16 else None, dln_w=new(D), dln_b=new(D), colsum=new(D),
                 dw=[new(D) for _ in range(4)], db=[new(D) for _ in range(4)])
        bkw = dict(dw=o["dw"], db=o["db"], **fkw) if diag else {}
        with _Routes() as r:
            ops.fddt_ln_bwd(h, rows, D, mode=mode, ln_w=lw, mean=mean, rstd=rstd, d_y=dy, g_res=gres, g_out=o["g"], g_out_bf16=o["gb"],
                            dln_w=o["dln_w"], dln_b=o["dln_b"], colsum_out=o["colsum"], **bkw)
        routes["bwd_bf16" if want_bf16 else "bwd_f32"] = r.seen[0]
        runs[want_bf16] = o
    if diag and side < 0:
        assert routes == dict(fwd="staged", bwd_bf16="staged_bf16", bwd_f32="staged_f32"), routes
    elif diag:
        assert not any(v is None or v.startswith("staged") for v in routes.values()), routes
    else:
        assert all(v is not None for v in routes.values()), routes
    err = dict(h_out=0.0, y_bf16=0.0, g_out=0.0, g_out_bf16=0.0)
    worst = lambda got, ref: float((got.double() - ref).abs().max())
    for sl, x, y, dh in _row_ref_chunks(h, stw, w, b, lw, lb, dy, gres, diag):
        if diag:
            err["h_out"] = max(err["h_out"], worst(ho[sl], x))
        err["y_bf16"] = max(err["y_bf16"], worst(yb[sl], y))
        for o in runs.values():
            err["g_out"] = max(err["g_out"], worst(o["g"][sl], dh))
            if o["gb"] is not None:
                err["g_out_bf16"] = max(err["g_out_bf16"], worst(o["gb"][sl], dh))
    sums, sc = _row_ref_chunks.sums, rows ** 0.5
    for tag, o in runs.items():
        err[f"ln_sums[{tag}]"] = max(worst(o["dln_w"], sums["dln_w"]), worst(o["dln_b"], sums["dln_b"]))
        fs = [worst(o["colsum"], sums["colsum"])]
        if diag:
            fs += [worst(o["dw"][c], sums["dw"][c]) for c in range(4)] + [worst(o["db"][c], sums["db"][c]) for c in range(4)]
        err[f"fddt_sums[{tag}]"] = max(fs)
    ms = clock.ms()
    for name, e in err.items():
        kind = name.split("[")[0]
        bound = ROW_BOUNDS["bf16"] if kind.endswith("bf16") else ROW_BOUNDS[kind] * sc if kind.endswith("sums") else ROW_BOUNDS[kind]
        print(f"far_offsets: {f'row kernels D={D} rows={rows} {name}':<62s} body={'/'.join(routes.values()):<30s} err={e:.3e} bound={bound:.3e} "
              f"arena_bytes=0 wall_ms={ms:.0f}")
        assert e < bound, (name, e, bound, routes)


# ================================================================================================ CTC prefix scores
@pytest.mark.parametrize("k", [1, 3], ids=["bf16_two_utterances", "f32_one_utterance"])
def test_ctc_prefix_score_far_ld(arena, k, monkeypatch):
    """dicow_ctc_prefix_score (with the frame normaliser and the initial state the scorer computes first) on logits rows at a tall ld:
    the problem, the fp64 reference and the bound are test_prefix_score_edges_vs_fp64's (T = 49, C = 65, a 5-label prefix); only the
    placement of the logits differs.  Bit-equal to the run on compact rows."""
    import ts_asr_whisper_amd.ctc_decoding as cd
    from tests import test_gpu_ctc_prefix_edges as E
    sw = E._switches(k)
    assert sw["fmt"] in ("bf16", "f32")
    p = E._build(49, 65, 5, k, sw["n3"], sw["fmt"], sw["alias"], sw["eos_is_blank"])
    psi, r, e_psi, e_r = E._reference(p)
    plain_psi, plain_r = E._run(cd, p)
    clock = _Clock()

    def far_dev(values, dtype, pad):
        Bx, T, V1 = values.shape
        ld, _ = tall_ld(Bx * T, V1, torch.empty(0, dtype=dtype).element_size(), 8, straddle=False)
        assert (Bx * T - 1) * ld * torch.empty(0, dtype=dtype).element_size() >= MARK32
        return far_view(arena, (Bx, T, V1), dtype, (T * ld, ld, 1), values=values, name="logits")

    monkeypatch.setattr(E, "_to_dev", far_dev)
    got_psi, got_r = E._run(cd, p)
    arena.check()
    assert np.array_equal(got_psi.view(np.int32), plain_psi.view(np.int32)) and np.array_equal(got_r.view(np.int32), plain_r.view(np.int32))
    E._compare(f"far ld k={k}", got_psi, got_r, psi, r, e_psi, e_r)
    _record(f"ctc_prefix_score T=49 C=65 d=5 {sw['fmt']} far ld", "ctc_prefix_score_kernel", 0.0, 0.0, arena, clock)


# ================================================================================================ decode-time rules (scores changed in place)
def _far_rows3(arena, vals, dtype, name, output):
    """[3, cols] rows a little more than 2^31 bytes apart: row 1 begins past 2^31, row 2 past 2^32."""
    isz = torch.empty(0, dtype=dtype).element_size()
    ld = _ceil_to(MARK31 // isz + 64, 64)
    view = far_view(arena, vals.shape, dtype, (ld, 1), values=None if output else vals, name=name, output=output)
    if output:                                                         # (changed in place: an output that starts with values)
        view.copy_(vals)
    assert 2 * ld * isz >= MARK32
    return view


@pytest.mark.parametrize("far", ["ld", "ids_stride"])
def test_repetition_rules_far(arena, far):
    """dicow_repetition_rules on 3 rows, V = 520 (the case builder, the transformers-processor reference and the comparison of
    test_gpu_repetition_rules.py; penalty 1.3, n-gram 3, 448 tokens of history): the score rows 2 GiB apart, then the history rows
    (slices of a wider int64 buffer) 2 GiB apart.  Bit-equal to the compact call."""
    from tests import test_gpu_repetition_rules as Rr
    from ts_asr_whisper_amd.generation import repetition_rules
    ids, sc = Rr.make_case(3, 520, 448, 3, 520)
    ref = Rr.hf_reference(ids, sc, 1.3, 3)
    plain = repetition_rules(ids.cuda(), sc.cuda().clone(), 1.3, 3)
    clock = _Clock()
    scd = _far_rows3(arena, sc, F32, "scores", True) if far == "ld" else sc.cuda().clone()
    idd = _far_rows3(arena, ids, torch.int64, "ids", False) if far == "ids_stride" else ids.cuda()
    out = repetition_rules(idd, scd, 1.3, 3)
    assert out.data_ptr() == scd.data_ptr()
    arena.check()
    _same_bits(scd, plain, far)
    pen, banned = Rr.compare(scd.cpu().contiguous(), sc, ref, ids, f"far {far}")
    assert pen > 0 and banned > 0
    _record(f"repetition_rules 3 x 520 far {far}", "repetition_rules", 0.0, 0.0, arena, clock)


def test_whisper_timestamp_rules_far_ld(arena):
    """dicow_whisper_timestamp_rules on 3 rows, V = 520 (<|notimestamps|> = 99, eos = 90, 3 prompt tokens, two text labels generated) with
    the score rows 2 GiB apart: timestamps clearly detected in two rows (margins 7.1 and 4.7), clearly not in the third (-8.8).  Every row equals tests/timestamp_rules_ref.py
    bit for bit (test_gpu_timestamp_rules_edges.py's criterion) and the compact call.  (The history is a contiguous argument of this
    entry point: it has no stride to move.)"""
    from tests import timestamp_rules_ref as tsref
    from ts_asr_whisper_amd.generation import timestamp_rules
    V, no_ts, eos, begin = 520, 99, 90, 3
    g = np.random.default_rng(520)
    sc = (g.standard_normal((3, V)) * 2).astype(np.float32)
    sc[0, no_ts + 1:] += np.float32(3.0)
    sc[2, no_ts + 1:] -= np.float32(12.0)
    ids = np.array([[1] * begin + [5, 17]] * 3, dtype=np.int64)
    _, margin, want = tsref.timestamp_rules(ids, sc, begin, eos, no_ts, None)
    assert margin[0] > 1 and margin[2] < -1
    idd, sct = torch.from_numpy(ids).cuda(), torch.from_numpy(sc)
    plain = timestamp_rules(idd, sct.cuda().clone(), begin, eos, no_ts)
    clock = _Clock()
    scd = _far_rows3(arena, sct, F32, "scores", True)
    timestamp_rules(idd, scd, begin, eos, no_ts)
    arena.check()
    _same_bits(scd, plain, "scores")
    got = scd.cpu().contiguous().numpy()
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want, dtype=np.float32).view(np.int32))
    _record("whisper_timestamp_rules 3 x 520 far ld", "timestamp_rules_kernel", 0.0, 0.0, arena, clock)


# ================================================================================================ CTC forced alignment
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_ctc_forced_align_far_ld(arena, dt):
    """Two problems on logits [2, 20, 37] read in place at a tall ld (the utterances back to back, 40 frame rows): problem 0 gathers
    the frames up to the 2^31 mark, problem 1 frames from above 2^31 to past 2^32.  Dyadic values, log-probabilities already (nothing subtracted):
    path, spans, token scores and score equal the integer oracle of tests/ctc_align_ref.py bit for bit (test_gpu_ctc_align.py's
    `expected`) and the call on compact logits."""
    from tests import test_gpu_ctc_align as A
    from ts_asr_whisper_amd.ctc_align import ctc_forced_align
    B, Tn, V1, blank = 2, 20, 37, 36
    rng = np.random.default_rng(2037)
    vals = A.dyadic(rng, (B, Tn, V1))
    problems = [(0, 0, 20, A.targets(rng, 6, V1, blank)), (1, 2, 18, A.targets(rng, 7, V1, blank))]
    dtype = A.DT[dt]
    isz = 2 if dt == "bf16" else 4
    kw = dict(blank=blank, rows=[p[0] for p in problems], frame_start=[p[1] for p in problems], frame_len=[p[2] for p in problems], normalized=True)
    tg = [p[3] for p in problems]
    plain = ctc_forced_align(torch.from_numpy(vals).to(dtype).cuda(), tg, **kw)
    ld, _ = tall_ld(B * Tn, V1, isz, 8, straddle=False)
    assert (Tn - 2) * ld * isz < MARK31 <= Tn * ld * isz and (B * Tn - 1) * ld * isz >= MARK32
    clock = _Clock()
    x = far_view(arena, (B, Tn, V1), dtype, (Tn * ld, ld, 1), values=torch.from_numpy(vals), name="logits")
    got = ctc_forced_align(x, tg, **kw)
    arena.check()
    want = A.expected(vals, problems, blank, 20, 7)
    assert bool(got.ok.all()) and want["status"].tolist() == [0, 0]
    for k in ("path", "spans", "token_score", "score"):
        g, p_, w = getattr(got, k).cpu(), getattr(plain, k).cpu(), want[k]
        assert torch.equal(g.contiguous().view(torch.int32), p_.contiguous().view(torch.int32)), (k, "far differs from compact")
        assert torch.equal(g.contiguous().view(torch.int32), w.contiguous().view(torch.int32)), (k, g, w)
    _record(f"ctc_forced_align 2 problems on [2,20,37] {dt} far ld", "ctc_forced_align", 0.0, 0.0, arena, clock)

"""dicow_gemm_nt's epilogues pinned bit for bit on every kernel family and every compile-time epilogue of the ring kernel.

Operands from the dyadic grids of tests/gemm_exact_ref.py: the fp32 accumulator is the fp64 product exactly, whatever the summation
order (tests/test_host_gemm_exact_ref.py asserts the conditions at these very shapes), so the fp64 reference with the header's rounding
points is THE answer and the results are compared with torch.equal: plain products, BIAS, BIAS | SCALE_N, BIAS | RESIDUAL, ACCUM,
MUL_AUX, the pre-activation a GELU epilogue saves, and the column sums -- the sum of the fp32 values before the store rounding on the
ring kernel's fused route, the sum of the stored bf16 values everywhere else (include/dicow_hip.h, DICOW_EPI_COLSUM).  Where a
transcendental is involved the result must be a correct bf16 rounding of something close to the fp64 value (R.rounded): within 1e-6 for
the activation (the project's bound in test_gelu_device_accuracy), within R.GELU_GRAD_D for gelu' (twice the error measured on the
dense grid below, 2 x 1.8386e-7: R.GELU_GRAD_MEASURED), within 2 R.GELU_GRAD_D max(1, |acc|) for GELU_BWD's acc * gelu'(aux).
No tolerance in this file is looser than these two comparators.

Every case asserts the kernel instantiation that ran (ops.gemm_dispatch_log(); the skinny kernel leaves no entry) and runs twice for the
same bits.  gemm_ntr_kernel<0, 3, 5> is unreachable in the stable build -- nt_plan's plain256 sends a product without epilogue work to
256 x 256 tiles -- and is not forced; the FDDT instantiation stays with test_gemm_nt_fddt_epilogue_bit_exact, which is bit-equal to the
<13, 3, 5> result pinned here followed by the row kernel.  The batched case runs no RESIDUAL (the ABI has no batch stride for it) and no
column sums (single results only).  The ring shapes assume 256 CUs, as nt_plan's rounds do.  Run with `pytest -m gpu`."""
import ctypes

import pytest
import torch

import amd_pkg
from tests import gemm_exact_ref as R

pytestmark = pytest.mark.gpu
amd_pkg.load()

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


_cache = {}


def _problem(sid):
    """Operands and the fp64 accumulator of a shape on the device: computed once, shared by the shape's cases, never written."""
    if sid not in _cache:
        _cache.clear()
        inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in R.make_inputs(sid).items()}
        _cache[sid] = (inp, R.accumulate64(inp))
    return _cache[sid]


def _launched(ops, fn):
    """Runs fn and returns {kernel name: launches} of the GEMM dispatch log it caused."""
    before = ops.gemm_dispatch_log()
    fn()
    after = ops.gemm_dispatch_log()
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _launch(ops, inp, eid):
    """One launch of the case; returns (C, aux written by a GELU epilogue or None, column sums or None)."""
    M, N, K, batch = inp["M"], inp["N"], inp["K"], inp["batch"]
    _, fl, f32, colsum = R.EPILOGUE[eid]
    C = inp["residual"].clone() if fl & R.ACCUM else _nan((batch * M, N), F32 if f32 else BF16)
    kw = {"flags": fl & ~(R.BIAS | R.RESIDUAL)}            # (ops.gemm_nt sets BIAS / RESIDUAL / OUT_F32 / COLSUM from its arguments)
    aux_out = cs = None
    if fl & R.BIAS:
        kw["bias"] = inp["bias"]
    if fl & R.RESIDUAL:
        kw["residual"] = inp["residual"]
    if fl & R.SCALE_N:
        kw.update(scale=inp["scale"], scale_ncols=inp["scale_ncols"])
    if fl & R.GELU:
        kw["aux"] = aux_out = _nan((batch * M, N), BF16)
    if fl & R.MUL_AUX:
        kw["aux"] = inp["dgelu"]
    if fl & R.GELU_BWD:
        kw["aux"] = inp["pre"]
    if colsum:
        kw["colsum_out"] = cs = torch.full((N,), 0.5, device="cuda")
    if batch > 1:
        kw.update(batch=batch, strideA=M * K, strideB=N * K, strideC=M * N, strideAux=M * N)
    ops.gemm_nt(inp["A"], inp["B"], C, M, N, K, **kw)
    return C, aux_out, cs


@pytest.mark.parametrize("sid,eid", R.cases(), ids=["%s-%s" % c for c in R.cases()])
def test_epilogue_exact(ops, sid, eid):
    from ts_asr_whisper_amd import _lib as L
    inp, acc = _problem(sid)
    fl = R.full_flags(eid)
    want = R.expected_kernel(sid, eid)
    if sid == "splitk":                                    # the log names the same kernel with and without the split
        a = L.GemmArgs()
        a.A, a.B, a.C, a.M, a.N, a.K = inp["A"].data_ptr(), inp["B"].data_ptr(), inp["A"].data_ptr(), inp["M"], inp["N"], inp["K"]
        a.lda, a.ldb, a.ldc, a.batch, a.flags = inp["K"], inp["K"], inp["N"], 1, fl
        assert L.lib().dicow_gemm_nt_splitk_ws_bytes(ctypes.byref(a)) > 0
    out = []
    ran = _launched(ops, lambda: out.append(_launch(ops, inp, eid)))
    assert ran == ({} if want is None else {want: 1}), (ran, want)
    out.append(_launch(ops, inp, eid))
    torch.cuda.synchronize()
    (C, aux, cs), (C2, aux2, cs2) = out
    same = torch.equal(C, C2) and (aux is None or torch.equal(aux, aux2)) and (cs is None or torch.equal(cs, cs2))
    ref = R.reference(acc, fl, inp)
    worst = {}
    if fl & R.GELU:
        worst["gelu"] = R.rounded_ratio(C, ref["v"], 1e-6)
        if fl & R.GELU_DAUX:
            worst["gelu'"] = R.rounded_ratio(aux, ref["aux_v"], R.GELU_GRAD_D)
        else:
            worst["aux"] = 0.0 if R.exact(aux, ref["aux"]) else float("inf")
    elif fl & R.GELU_BWD:
        worst["acc gelu'"] = R.rounded_ratio(C, ref["v"], 2 * R.GELU_GRAD_D * acc.abs().clamp(min=1.0))
    else:
        worst["C"] = 0.0 if R.exact(C, ref["C"]) else float("inf")
    if cs is not None:
        fused = want is not None and want.startswith("gemm_ntr_kernel")
        worst["colsum"] = 0.0 if R.exact(cs, 0.5 + ref["colsum_pre" if fused else "colsum_stored"]) else float("inf")
    print("EXACT_CASE %-12s %-16s %-28s %s%s" % (sid, eid, want or "gemm_nt_skinny_kernel (no entry)",
                                                 "  ".join("%s %.4f" % kv for kv in worst.items()), "" if same else "  RUNS DIFFER"))
    assert same, "two runs of the same problem differ"
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ the device GELU on every bf16 input
# route id, M, N, K, kernel of the compile-time epilogues (F = 3 and 131 on the ring: the packed gelu_cdf_pdf_p through
# nt_epilogue_math_n), kernel of the run-time-flag epilogues (the scalar gelu_erf / gelu_erf_grad of nt_epilogue_math)
DENSE = [("generic", 528, 64, 64, "gemm_nt_kernel<2, false>", "gemm_nt_kernel<2, false>"),
         ("ring44", 6200, 2244, 128, "gemm_ntr_kernel<%d, 4, 4>", "gemm_ntr_kernel<-1, 4, 4>"),
         ("ring35", 8500, 1284, 128, "gemm_ntr_kernel<%d, 3, 5>", "gemm_ntr_kernel<-1, 3, 5>")]
_dense = {}


def _dense_problem(M, N, K):
    if (M, N, K) not in _dense:
        _dense.clear()
        a = R.dense_a(M, K).cuda()
        x = a[:, torch.arange(N, device="cuda") % K].contiguous()              # what the identity product leaves in the accumulator
        _dense[(M, N, K)] = (a, R.identity_b(N, K).cuda(), x, x.double())
    return _dense[(M, N, K)]


def _share(got_bf16, ref64, min_abs=1e-4):
    """Share of the inputs with |ref| > min_abs whose bf16 result IS the rounded fp64 value."""
    big = ref64.abs() > min_abs
    return float((got_bf16.double()[big] == R.bf16(ref64)[big]).double().mean())


@pytest.mark.parametrize("route", DENSE, ids=[d[0] for d in DENSE])
def test_gelu_dense_grid(ops, route):
    """Every finite bf16 value of [-9, 9] (33 314, padded with repeats) as the pre-activation, through an identity product (B[n, k] = 1
    where n % K == k, so acc = x exactly; zero bias where the instantiation wants one): the activation within 1e-6 of fp64 erf and equal
    to the rounded fp64 value on more than 0.999 of the inputs with |gelu| > 1e-4 (test_gelu_device_accuracy's numbers), the saved
    pre-activation equal to x, and the saved derivative a correct rounding of something within R.GELU_GRAD_D of fp64 gelu', equal to the
    rounded fp64 value on more than 0.999 of the inputs with |gelu'| > 1e-4 (below that the absolute bound is what matters, as for
    the activation).  The saved pre-activation includes the bf16 subnormals: the MFMA and the conversion keep them."""
    from ts_asr_whisper_amd import _lib as L
    name, M, N, K, kern_ct, kern_rt = route
    a, b, x, x64 = _dense_problem(M, N, K)
    zero = torch.zeros(N, device="cuda")
    g64, d64 = R.gelu64(x64), R.gelu_grad64(x64)
    # BIAS | GELU, bf16: the packed path on the ring
    C, aux = _nan((M, N), BF16), _nan((M, N), BF16)
    ran = _launched(ops, lambda: ops.gemm_nt(a, b, C, M, N, K, bias=zero, aux=aux, flags=L.EPI_GELU))
    assert ran == {kern_ct % 3 if "%" in kern_ct else kern_ct: 1}, ran
    r1, s1 = R.rounded_ratio(C, g64, 1e-6), _share(C, g64)
    assert torch.equal(aux, x)
    # BIAS | GELU | GELU_DAUX, bf16
    C2, daux = _nan((M, N), BF16), _nan((M, N), BF16)
    ran = _launched(ops, lambda: ops.gemm_nt(a, b, C2, M, N, K, bias=zero, aux=daux, flags=L.EPI_GELU | L.EPI_GELU_DAUX))
    assert ran == {kern_ct % 131 if "%" in kern_ct else kern_ct: 1}, ran
    r2, s2 = R.rounded_ratio(C2, g64, 1e-6), _share(C2, g64)
    r3, s3 = R.rounded_ratio(daux, d64, R.GELU_GRAD_D), _share(daux, d64)
    # GELU, fp32 (run-time flags: the scalar path on every route)
    Cf = _nan((M, N), F32)
    ran = _launched(ops, lambda: ops.gemm_nt(a, b, Cf, M, N, K, flags=L.EPI_GELU))
    assert ran == {kern_rt: 1}, ran
    e4 = float((Cf.double() - g64).abs().max())
    print("DENSE_GELU %-8s gelu: bf16 %.4f of the bound, equal share %.5f | with gelu': %.4f, %.5f | gelu' bf16 %.4f of the bound, equal share "
          "%.5f | fp32 gelu max err %.3e"
          % (name, r1, s1, r2, s2, r3, s3, e4))
    assert torch.equal(C, C2), "the activation differs between the GELU and the GELU | GELU_DAUX epilogue"
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0 and e4 < 1e-6
    assert s1 > 0.999 and s2 > 0.999 and s3 > 0.999


@pytest.mark.parametrize("route", DENSE, ids=[d[0] for d in DENSE])
def test_gelu_bwd_dense_grid(ops, route):
    """GELU_BWD with acc = 1 exactly (A = ones against the identity B) and the dense grid as the saved pre-activation: the fp32 result
    IS the device's gelu'.  Its worst error against fp64 on the generic route is the measurement behind R.GELU_GRAD_MEASURED (printed;
    the bound is twice that); the bf16 result is a correct rounding within the bound and equals the rounded fp64 value on more than 0.999
    of the inputs with |gelu'| > 1e-4."""
    from ts_asr_whisper_amd import _lib as L
    name, M, N, K, _, kern_rt = route
    _, b, x, x64 = _dense_problem(M, N, K)
    ones = torch.ones(M, K, dtype=BF16, device="cuda")
    d64 = R.gelu_grad64(x64)
    Cf, Cb = _nan((M, N), F32), _nan((M, N), BF16)
    ran = _launched(ops, lambda: (ops.gemm_nt(ones, b, Cf, M, N, K, aux=x, flags=L.EPI_GELU_BWD),
                                  ops.gemm_nt(ones, b, Cb, M, N, K, aux=x, flags=L.EPI_GELU_BWD)))
    assert ran == {kern_rt: 2}, ran
    d = float((Cf.double() - d64).abs().max())
    rb, sb = R.rounded_ratio(Cb, d64, 2 * R.GELU_GRAD_D), _share(Cb, d64)
    print("DENSE_GELU_BWD %-8s fp32 gelu' max err d = %.4e (bound %.3e) | bf16 %.4f of the bound, equal share %.5f"
          % (name, d, R.GELU_GRAD_D, rb, sb))
    assert torch.isfinite(Cf).all() and d <= R.GELU_GRAD_D
    assert rb <= 1.0 and sb > 0.999

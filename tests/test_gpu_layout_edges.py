"""Layout edges on the MI355X: the GEMM, attention and row kernels on strided views with guard bands around every output and
poison around every input (tests/util.guarded / poisoned).  Each case asserts the kernel that runs (dispatch log, workspace
queries), (a) parity with an fp64 reference over the LOGICAL operands at the bound test_gpu_kernels.py already uses for that
kernel and epilogue, (b) bit-equality with the same call on contiguous, exactly sized, unpoisoned operands, and (c) that nothing
outside the logical output was written.  Run with `pytest -m gpu`."""
import ctypes as C
import functools

import pytest
import torch

import amd_pkg
from oracle import dicow_oracle as O
from tests.util import guarded, poisoned
from tests.test_gpu_kernels import ROW_ROUTE_CASES, _ExpectRoute, LN2

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


def _bf(x):
    return x.bfloat16().float()


def _launched(ops, fn):
    """Run fn(); the GEMM kernels the dispatch log gained meanwhile, one entry per launch."""
    before = ops.gemm_dispatch_log()
    fn()
    after = ops.gemm_dispatch_log()
    return [k for k in after for _ in range(after[k] - before.get(k, 0))]


def _err(got, ref_dev):
    """max |got - ref| on the device (NaN if anything is NaN: every `< bound` below then fails)."""
    return float((got.double() - ref_dev).abs().max())


def _check_all(guards):
    for g in guards:
        g.check()


# ================================================================================================ NT GEMM, every family of nt_plan
# Final table (family <- shape; every starting shape of the issue reached its family, none had to move):
#   generic, single k-step   (200, 132, 64)                       gemm_nt_kernel<2, false>
#   gemm_nt64                (70, 68, 448), (1000, 500, 128)      gemm_nt64_kernel<8>
#   gemm_nt128t              (2100, 1156, 128)                    170 tiles of 128 x 128, 45 of 256 x 256
#   ring 256 x 256           (6100, 2244, 128)                    plain bf16: gemm_ntr_kernel<0, 4, 4>
#   ring 192 x 320           (12200, 1284, 192)                   bias + residual: gemm_ntr_kernel<13, 3, 5>
#   skinny                   (7, 36, 5120), (16, 1284, 1280)      gemm_nt_skinny_kernel is not in the dispatch log: NO logged kernel runs
#   deep-contraction split   (200, 384, 8192)                     splitk_ws_bytes > 0; 8 ranges as the batches of gemm_nt64_kernel<8>
#   batched conv view        B = 3, L = 200, C = O = 128          gemm_nt64_kernel<8>, output rows 1..L/2 of [B, L/2 + 2, O]
# Leading dimensions: lda = K + 8, ldb = K + 16, ldc = N + 12, ldr = N + 4, ldaux = N + 8.
# Bounds (all from test_gpu_kernels.py): fp32 plain 1e-4 max(1, |ref|), bf16 plain 1e-2 max(1, |ref|) (test_gemm_nt_plain);
# bias + residual 3e-2 (test_gemm_nt64_decoder_shapes / test_gemm_nt_epilogues), 4e-2 on gemm_nt128t (test_gemm_nt_mid_size_shapes);
# GELU and its saved pre-activation 3e-2, MUL_AUX 4e-2, its column sums 2e-3 max(1, |ref|) + 0.15 sqrt(M) 2^-8, ACCUM 2e-4
# (test_gemm_nt_epilogues).
NT_CASES = {
    "generic": ((200, 132, 64), "gemm_nt_kernel<2, false>"),
    "nt64_small": ((70, 68, 448), "gemm_nt64_kernel"),
    "nt64": ((1000, 500, 128), "gemm_nt64_kernel"),
    "nt128t": ((2100, 1156, 128), "gemm_nt128t_kernel"),
    "ring256": ((6100, 2244, 128), "gemm_ntr_kernel"),
    "ring35": ((12200, 1284, 192), "gemm_ntr_kernel"),
    "skinny_small": ((7, 36, 5120), None),
    "skinny": ((16, 1284, 1280), None),
}
NT_EXACT = {("ring256", "plain_bf16"): "gemm_ntr_kernel<0, 4, 4>", ("ring35", "bias_res"): "gemm_ntr_kernel<13, 3, 5>"}


def _nt_call(ops, A, B, M, N, K, dtype, padded, *, kind="nan", bias=None, res=None, aux_in=None, aux_out=False, flags=0, colsum=False,
             init=None, m_guard=None):
    """One ops.gemm_nt call on padded + poisoned + guarded operands (padded) or on contiguous exact ones.  A, B, res, aux_in, init: CPU
    tensors of the logical values.  Returns ({name: device view}, [guards], [kernels launched]).  m_guard: rows the C guard is built
    for when that is not M (the negative control)."""
    guards, out = [], {}
    dev = lambda t, dt=None: None if t is None else (t.cuda() if dt is None else t.cuda().to(dt))
    mg = M if m_guard is None else m_guard
    if padded:
        lda, ldb, ldc, ldr, ldaux = K + 8, K + 16, N + 12, N + 4, N + 8
        Ad = poisoned(A.bfloat16(), lda, kind=kind)
        Bd = poisoned(B.bfloat16(), ldb, kind=kind)
        Cg = guarded((mg, N), ldc, dtype, init=init, name="C")
        guards.append(Cg)
        Cd = Cg.view
        resd = None if res is None else poisoned(res, ldr, kind=kind)
        auxd = None
        if aux_in is not None:
            auxd = poisoned(aux_in.bfloat16(), ldaux, kind=kind)
        elif aux_out:
            ag = guarded((mg, N), ldaux, torch.bfloat16, name="aux")
            guards.append(ag)
            auxd = ag.view
        csd = None
        if colsum:
            cg = guarded((N,), 64, torch.float32, init=torch.full((N,), 0.5), name="colsum_out")
            guards.append(cg)
            csd = cg.view
    else:
        lda = ldb = K
        ldc = ldr = ldaux = N
        Ad, Bd = dev(A, torch.bfloat16), dev(B, torch.bfloat16)
        Cd = torch.empty(M, N, dtype=dtype, device="cuda") if init is None else dev(init, dtype)
        resd = dev(res)
        auxd = dev(aux_in, torch.bfloat16) if aux_in is not None else (torch.empty(M, N, dtype=torch.bfloat16, device="cuda") if aux_out else None)
        csd = torch.full((N,), 0.5, device="cuda") if colsum else None
    ran = _launched(ops, lambda: ops.gemm_nt(Ad, Bd, Cd, M, N, K, lda=lda, ldb=ldb, ldc=ldc, bias=dev(bias), residual=resd, ldr=ldr, aux=auxd,
                                             ldaux=ldaux, flags=flags, colsum_out=csd))
    out["C"] = Cd
    if aux_out:
        out["aux"] = auxd
    if colsum:
        out["colsum"] = csd
    return out, guards, ran


@pytest.mark.parametrize("case", list(NT_CASES))
def test_gemm_nt_family_on_padded_poisoned_guarded_operands(ops, case):
    from ts_asr_whisper_amd import _lib as L
    (M, N, K), kernel = NT_CASES[case]
    ring = kernel == "gemm_ntr_kernel"
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A, B = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g) * K ** -0.5)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    daux = _bf(torch.rand(M, N, generator=g) * 1.1)                          # a saved gelu' (values in [0, 1.1])
    ref = (A.double() @ B.double().t()).cuda()
    rmax = max(1.0, float(ref.abs().max()))
    base = (ref + bias.double().cuda()).float()
    res_d, daux_d = res.cuda().double(), daux.cuda().double()
    res_bound = 4e-2 if case == "nt128t" else 3e-2

    def both(name, dtype, checks, **kw):
        """The padded run against the contiguous one: same kernel, the expected family, intact guards, equal bits; then `checks`."""
        got, guards, ran = _nt_call(ops, A, B, M, N, K, dtype, True, **kw)
        plain, _, ran_plain = _nt_call(ops, A, B, M, N, K, dtype, False, **{k: v for k, v in kw.items() if k != "kind"})
        assert ran == ran_plain, (name, ran, ran_plain)
        if kernel is None:
            assert ran == [], (name, ran)                                    # the skinny kernel (the only unlogged NT kernel) ran
        else:
            assert len(ran) == 1 and ran[0].startswith(kernel), (name, ran)
        if (case, name) in NT_EXACT:
            assert ran[0] == NT_EXACT[(case, name)], (name, ran)
        _check_all(guards)
        for k in got:
            assert torch.equal(got[k], plain[k]), (name, k, "the padded layout changed the arithmetic",
                                                   float((got[k].double() - plain[k].double()).abs().max()))
        for k, want, bound in checks:
            e = _err(got[k], want)
            print(f"nt {case} {name}.{k}: {e:.3e} (bound {bound:.3e})")
            assert e < bound, (name, k, e, bound)

    if ring:
        Ad, Bd = poisoned(A.bfloat16(), K + 8), poisoned(B.bfloat16(), K + 16)
        assert ops.gemm_nt(Ad, Bd, Ad, M, N, K, lda=K + 8, ldb=K + 16, ldc=N + 12, query_persistent=True)
    both("plain_f32", torch.float32, [("C", ref, 1e-4 * rmax)], kind="nan")
    both("plain_bf16", torch.bfloat16, [("C", ref, 1e-2 * rmax)], kind="big")
    both("bias_res", torch.float32, [("C", _bf(base).double() + res_d, res_bound)], bias=bias, res=res)
    gelu = O.gelu_erf(_bf(base).double())
    both("bias_gelu_aux", torch.bfloat16, [("C", gelu, 3e-2), ("aux", base.double(), 3e-2)], bias=bias, aux_out=True, flags=L.EPI_GELU, kind="big")
    both("accum", torch.float32, [("C", res_d + ref, 2e-4)], init=res, flags=L.EPI_ACCUM)
    if ring or case == "nt64":
        ref_cs = 0.5 + (ref * daux_d).sum(0)
        cs_bound = 2e-3 * max(1.0, float(ref_cs.abs().max())) + 0.15 * (M ** 0.5) * 2 ** -8
        both("mul_aux_colsum", torch.bfloat16, [("C", ref * daux_d, 4e-2), ("colsum", ref_cs, cs_bound)], aux_in=daux, flags=L.EPI_MUL_AUX, colsum=True)


@pytest.mark.parametrize("f32", [True, False])
def test_gemm_nt_deep_contraction_split_padded(ops, f32):
    """K = 8192 with a small output: the contraction runs as 8 ranges (the batches of one launch, operand stride = the range's k
    offset inside the PADDED rows) and a reduce pass that writes C with ldc.  Bounds and input scale of
    test_gemm_nt_deep_contraction_split: 2e-3 / 2e-2 times max(1, |ref|)."""
    from ts_asr_whisper_amd import _lib as L
    M, N, K = 200, 384, 8192
    g = torch.Generator().manual_seed(M + K)
    A, B = _bf(torch.randn(M, K, generator=g) * 0.05), _bf(torch.randn(N, K, generator=g) * 0.05)
    ref = (A.double() @ B.double().t()).cuda()
    dtype = torch.float32 if f32 else torch.bfloat16
    a = L.GemmArgs()
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.batch, a.flags = M, N, K, K + 8, K + 16, N + 12, 1, (L.EPI_OUT_F32 if f32 else 0)
    assert L.lib().dicow_gemm_nt_splitk_ws_bytes(C.byref(a)) == 8 * M * N * 4
    got, guards, ran = _nt_call(ops, A, B, M, N, K, dtype, True, kind="nan" if f32 else "big")
    plain, _, ran_plain = _nt_call(ops, A, B, M, N, K, dtype, False)
    assert ran == ran_plain and len(ran) == 1 and ran[0].startswith("gemm_nt64_kernel"), (ran, ran_plain)
    _check_all(guards)
    assert guards[0].untouched_inside() == 0
    assert torch.equal(got["C"], plain["C"])
    e, bound = _err(got["C"], ref), (2e-3 if f32 else 2e-2) * max(1.0, float(ref.abs().max()))
    print(f"nt split f32={f32}: {e:.3e} (bound {bound:.3e})")
    assert e < bound


def test_gemm_nt_batched_conv_view_into_padded_rows(ops):
    """conv1 as the engine runs it: B = 3 utterances, the overlapping time-major view (lda = 2 C), the output into rows 1 .. L/2 of
    a [B, L/2 + 2, O] buffer whose rows 0 and L/2 + 1 are conv2's zero padding -- here part of the guard, with three poisoned rows
    between the utterances of the input.  Bound of test_gemm_nt_batched_strided_conv_view: 2e-4."""
    Bn, Ln, Cc, Oc = 3, 200, 128, 128
    K, T2 = 3 * Cc, Ln // 2
    g = torch.Generator().manual_seed(9)
    x = _bf(torch.randn(Bn, Cc, Ln, generator=g))
    w = _bf(torch.randn(Oc, Cc, 3, generator=g) * (3 * Cc) ** -0.5)
    bias = torch.randn(Oc, generator=g)
    ref = torch.nn.functional.conv1d(x.double(), w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 1).cuda()
    xt = torch.zeros(Bn, Ln + 2, Cc)
    xt[:, 1:Ln + 1] = x.permute(0, 2, 1)
    wp = ops.conv_weight_pack(w.cuda(), K)
    ldb, ldc, gap = K + 16, Oc + 12, 3
    sA = (Ln + 2 + gap) * Cc
    xd = poisoned(xt.bfloat16(), Cc, strides=(sA, Cc, 1), span_rows=Bn * (Ln + 2 + gap))
    wd = poisoned(wp.cpu(), ldb, kind="big")
    og = guarded((Bn, T2, Oc), ldc, torch.float32, strides=((T2 + 2) * ldc, ldc, 1), offset=ldc, span_rows=Bn * (T2 + 2), name="conv out")
    ran = _launched(ops, lambda: ops.gemm_nt(xd, wd, og.view, T2, Oc, K, lda=2 * Cc, ldb=ldb, ldc=ldc, bias=bias.cuda(), batch=Bn, strideA=sA,
                                             strideC=(T2 + 2) * ldc))
    plain = torch.empty(Bn, T2, Oc, device="cuda")
    ran_plain = _launched(ops, lambda: ops.gemm_nt(xt.cuda().bfloat16(), wp, plain, T2, Oc, K, lda=2 * Cc, bias=bias.cuda(), batch=Bn,
                                                   strideA=(Ln + 2) * Cc, strideC=T2 * Oc))
    assert ran == ran_plain and len(ran) == 1 and ran[0].startswith("gemm_nt64_kernel"), (ran, ran_plain)
    og.check()                                                               # rows 0 and L/2 + 1 of every utterance included
    assert og.untouched_inside() == 0
    assert torch.equal(og.view, plain)
    assert _err(og.view, ref) < 2e-4


def test_negative_control_gemm_row_past_the_guard_is_flagged(ops):
    """The guard check can fail: M + 1 rows declared against a C guard built for M rows (row M of A is poison inside our own
    allocation, row M of C the first trailing guard row) -- the checker names (M, 0)."""
    M, N, K = 200, 132, 64
    g = torch.Generator().manual_seed(1)
    A, B = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g) * K ** -0.5)
    _, guards, _ = _nt_call(ops, A, B, M + 1, N, K, torch.float32, True, m_guard=M)
    assert guards[0].first_violation() == (M, 0)
    with pytest.raises(AssertionError, match=f"row {M}, col 0"):
        guards[0].check()
    assert guards[0].untouched_inside() == 0


# ================================================================================================ TN GEMM, every route
# (name: Mk, N1, N2, batch, gap rows between batches, seg_rows, kernel, splits) -- the route asserted through dicow_gemm_tn_ws_bytes
# (bytes = splits * 4 N1 N2, 0 = no split) and the dispatch log.  lda = N1 + 8, ldb = N2 + 16, ldc = N2 + 12.
# 256 tile: the plan's cost model takes it at far smaller ragged shapes than the issue's starting ones -- (72, 264, 264) without a
# split, (1032, 264, 264) with two -- and does NOT take it at (1544, 3832, 1272) (128 tile, no split: 300 workgroups fill the 512
# slots better than 75 fill 256); 4088 x 4088 at Mk = 520 does take it (no split) but costs 17 GFLOP of fp64 reference, so the
# small shapes are the cover.  A batched 256-tile split (conv-like, 4 x 200 rows) is added.
TN_CASES = {
    "t128": (200, 136, 72, 1, 0, 0, "gemm_tn_kernel", 1),
    "t128_split": (1500, 384, 1152, 1, 0, 0, "gemm_tn_kernel", 3),
    "batched_adjacent": (200, 1152, 384, 4, 0, 0, "gemm_tn_kernel", 2),       # strideA = Mk lda: a k-tail over-read is the next batch's data
    "batched_gap": (200, 1152, 384, 4, 5, 0, "gemm_tn_kernel", 2),            # five poisoned rows between the batches
    "batched_t256": (200, 384, 384, 4, 0, 0, "gemm_tn256_kernel", 2),
    "seg": (200, 384, 136, 1, 0, 128, "gemm_tn_kernel", 1),
    "seg_partial": (200, 320, 136, 1, 0, 128, "gemm_tn_kernel", 1),           # third segment: 64 rows
    "seg_split": (1500, 384, 136, 1, 0, 128, "gemm_tn_kernel", 3),            # one reduce launch per segment
    "seg_partial_split": (1500, 320, 136, 1, 0, 128, "gemm_tn_kernel", 3),
    "t256": (72, 264, 264, 1, 0, 0, "gemm_tn256_kernel", 1),
    "t256_split": (1032, 264, 264, 1, 0, 0, "gemm_tn256_kernel", 2),
}


def _tn_outputs(N1, N2, seg, padded, init):
    """C (and its row segments) as guarded buffers (padded) or plain tensors; returns (tensors, guards)."""
    bounds = [(0, N1)] if not seg else [(r, min(r + seg, N1)) for r in range(0, N1, seg)]
    ts, gs = [], []
    for i, (r0, r1) in enumerate(bounds):
        part = None if init is None else init[r0:r1]
        if padded:
            gd = guarded((r1 - r0, N2), N2 + 12, torch.float32, init=part, name=f"C segment {i}")
            gs.append(gd)
            ts.append(gd.view)
        else:
            ts.append(torch.full((r1 - r0, N2), float("nan"), device="cuda") if part is None else part.cuda().clone())
    return ts, gs


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", list(TN_CASES))
def test_gemm_tn_route_on_padded_poisoned_guarded_operands(ops, case, accumulate):
    from ts_asr_whisper_amd import _lib as L
    Mk, N1, N2, batch, gap, seg, kernel, splits = TN_CASES[case]
    g = torch.Generator().manual_seed(Mk + N1 + batch)
    A, B = _bf(torch.randn(batch, Mk, N1, generator=g)), _bf(torch.randn(batch, Mk, N2, generator=g))
    init = torch.randn(N1, N2, generator=g) if accumulate else None
    ref = torch.einsum("bmi,bmj->ij", A.double(), B.double())
    ref = (ref + init.double() if accumulate else ref).cuda()
    lda, ldb, ldc = N1 + 8, N2 + 16, N2 + 12
    sA, sB = (Mk + gap) * lda, (Mk + gap) * ldb
    # route: the library's own answer for these arguments
    q = L.GemmTnArgs()
    q.Mk, q.N1, q.N2, q.lda, q.ldb, q.ldc, q.batch, q.strideA, q.strideB, q.accumulate, q.seg_rows = Mk, N1, N2, lda, ldb, ldc, batch, sA, sB, accumulate, seg
    ws = L.lib().dicow_gemm_tn_ws_bytes(C.byref(q))
    assert ws == (splits * 4 * N1 * N2 if splits > 1 else 0), (ws, ws / (4 * N1 * N2))
    outs = {}
    for padded in (True, False):
        for kind in (("nan", "big") if padded else ("plain",)):
            if padded:
                Ad = poisoned(A.bfloat16(), lda, strides=(sA, lda, 1), span_rows=batch * (Mk + gap), kind=kind)
                Bd = poisoned(B.bfloat16(), ldb, strides=(sB, ldb, 1), span_rows=batch * (Mk + gap), kind=kind)
                kw = dict(lda=lda, ldb=ldb, ldc=ldc, strideA=sA, strideB=sB)
            else:
                Ad, Bd = A.bfloat16().cuda(), B.bfloat16().cuda()
                kw = dict(strideA=Mk * N1, strideB=Mk * N2)
            ts, gs = _tn_outputs(N1, N2, seg, padded, init)
            ran = _launched(ops, lambda: ops.gemm_tn(Ad, Bd, ts[0], Mk, N1, N2, batch=batch, accumulate=bool(accumulate),
                                                     C_seg=ts[1:] if seg else None, seg_rows=seg, **kw))
            assert ran == [kernel], (kind, ran)
            _check_all(gs)
            if padded and not accumulate:
                assert [gd.untouched_inside() for gd in gs] == [0] * len(gs)          # the NaN the region started with is gone
            outs[kind] = torch.cat(ts, 0)                                             # each segment holds exactly its rows
    assert torch.equal(outs["nan"], outs["plain"]) and torch.equal(outs["big"], outs["plain"])
    e, bound = _err(outs["nan"], ref), 2e-4 * max(1.0, float(ref.abs().max()))
    print(f"tn {case} accumulate={accumulate}: {e:.3e} (bound {bound:.3e})")
    assert e < bound


def test_gemm_tn_pooled_group(ops):
    """dicow_gemm_tn_group with three problems that pool (264 tiles of 256 x 256 on 256 CUs: one whole round, the remaining 8 tiles
    split three ways and added by the fix-up launch): problem 0 in row segments that straddle the 256-row tiles (seg_rows = 640,
    third segment 520 rows), problem 1 with N2 = 3000 (no multiple of 256), Mk = 136 (two whole k-tiles and 8 rows); accumulate
    1 / 0 / 1."""
    Mk = 136
    probs = [(1800, 2048, 640, 1), (2048, 3000, 0, 0), (2048, 3200, 0, 1)]            # (N1, N2, seg_rows, accumulate)
    g = torch.Generator().manual_seed(3)
    data = []
    for N1, N2, seg, acc in probs:
        A, B = _bf(torch.randn(Mk, N1, generator=g)), _bf(torch.randn(Mk, N2, generator=g))
        init = torch.randn(N1, N2, generator=g) if acc else None
        ref = A.double().t() @ B.double()
        data.append((A, B, init, (ref + init.double()) if acc else ref))
    results = {}
    for kind in ("nan", "big", "plain"):
        grp, keep, guards = ops.TnGroup(), [], []
        for (N1, N2, seg, acc), (A, B, init, _) in zip(probs, data):
            if kind == "plain":
                Ad, Bd, kw = A.bfloat16().cuda(), B.bfloat16().cuda(), {}
            else:
                Ad, Bd = poisoned(A.bfloat16(), N1 + 8, kind=kind), poisoned(B.bfloat16(), N2 + 16, kind=kind)
                kw = dict(lda=N1 + 8, ldb=N2 + 16, ldc=N2 + 12)
            ts, gs = _tn_outputs(N1, N2, seg, kind != "plain", init)
            grp.add(Ad, Bd, ts[0], Mk, N1, N2, accumulate=bool(acc), C_seg=ts[1:] if seg else None, seg_rows=seg, **kw)
            keep.append(ts)
            guards += gs
        ran = _launched(ops, grp.run)
        assert ran == ["gemm_tn256g_kernel"], ran                                     # pooled: one launch, not three
        _check_all(guards)
        assert [gd.untouched_inside() for gd in guards] == [0] * len(guards)
        results[kind] = [torch.cat(ts, 0) for ts in keep]
    for i, (_, _, _, ref) in enumerate(data):
        assert torch.equal(results["nan"][i], results["plain"][i]) and torch.equal(results["big"][i], results["plain"][i]), i
        e, bound = _err(results["nan"][i], ref.cuda()), 2e-4 * max(1.0, float(ref.abs().max()))
        print(f"tn group problem {i}: {e:.3e} (bound {bound:.3e})")
        assert e < bound, i


# ================================================================================================ attention
ATTN_KV_TILE = 64            # attention.hip KV_TILE: keys per tile of the forward and of the dq kernel
ATTN_Q_BLOCK = 128           # attention.hip attn_fwd_plan: query rows per workgroup (4 waves x 32 rows)
ATTN_BWD_KEY_BLOCK = 128     # attention.hip KB: keys per workgroup of attn_bwd_dkv_kernel / the fused kernel (attn_bwd_plan: nkb = ceil(Lk / 128))
DECODE_GROUPS = 64           # attn_decode.hip:18 AD_NG: key groups of a workgroup, group gi takes keys gi, gi + 64, ...
DECODE_TRIP = 64 * 4         # attn_decode.hip:41,68  AD_NG * UK keys per trip of the key loop (UK = 4 for group <= 6)
PAD_ROWS = 7                 # Lmax = L + 7
ATTN_LENGTHS = [40, ATTN_KV_TILE - 1, ATTN_KV_TILE + 1, ATTN_BWD_KEY_BLOCK - 1, ATTN_BWD_KEY_BLOCK + 1]
K_ALIGN, V_POISON = 16.0, 100.0


def _unit(gen):
    return torch.nn.functional.normalize(torch.randn(64, generator=gen), dim=0)


def _q_rows(gen, shape, u, sd, along):
    """Query rows sd * N(0, 1) with the component along u replaced by `along`: q . (c u) = c * along for every row."""
    n = torch.randn(*shape, 64, generator=gen) * sd
    return n - (n @ u)[..., None] * u + along * u


@functools.lru_cache(maxsize=None)
def _attn_case(B, H, L, causal, q_log2, p=None):
    """Packed q | k | v rows [B, L, 3D] (bf16 values), d_o, the direction u the queries share, and the fp64 forward / backward
    reference.  p: make key p dominate every row that may see it (k[p] = K_ALIGN u: score 3 K_ALIGN, the others ~ N(0, 3.4)) with
    v[p] = 4."""
    g = torch.Generator().manual_seed(B * 1000 + L + 7 * H + (0 if p is None else 31 * (p + 1)))
    D = H * 64
    u = _unit(g)
    qkv = torch.randn(B, L, 3 * D, generator=g) * 0.6
    qkv[:, :, :D] = _q_rows(g, (B, L, H), u, 0.6, 3.0).view(B, L, D)
    if p is not None:
        qkv[:, p, D:2 * D] = (K_ALIGN * u).repeat(H)
        qkv[:, p, 2 * D:] = 4.0
    qkv = _bf(qkv)
    d_o = _bf(torch.randn(B, L, H, 64, generator=g))
    q = qkv[:, :, :D].reshape(B, L, H, 64).double().requires_grad_(True)
    k = qkv[:, :, D:2 * D].reshape(B, L, H, 64).double().requires_grad_(True)
    v = qkv[:, :, 2 * D:].reshape(B, L, H, 64).double().requires_grad_(True)
    s = torch.einsum("blhd,bmhd->bhlm", q, k) * (LN2 if q_log2 else 1.0)
    if causal:
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float("-inf"))
    prob = torch.softmax(s, -1)
    o = torch.einsum("bhlm,bmhd->blhd", prob, v)
    (o * d_o.double()).sum().backward()
    if p is not None:                                                        # the construction holds: key p takes > 0.99 of every row that sees it
        assert float(prob[:, :, (p if causal else 0):, p].min()) > 0.99
    dq = (q.grad / LN2 if q_log2 else q.grad) * 0.5                          # dq_scale = 0.5, as in test_attn_bwd
    return dict(qkv=qkv, d_o=d_o, u=u, o=o.detach(), lse=torch.logsumexp(s, -1).detach(), dq=dq, dk=k.grad, dv=v.grad)


def _poison_row_packed(u, H):
    """One packed row of the aligned finite poison: q = 100, k = K_ALIGN u per head (score 3 K_ALIGN with every query), v = +100."""
    D = H * 64
    return torch.cat([torch.full((D,), 100.0), (K_ALIGN * u).repeat(H), torch.full((D,), V_POISON)])


def _packed_in(t, B, L, ld, kind, row=None):
    """[B, L, ld] logical rows inside a [B, L + 7, ld] buffer; rows L .. L + 7 of every batch and everything after the last batch
    hold the poison (kind "big" with a row pattern: the aligned poison)."""
    Lmax = L + PAD_ROWS
    return poisoned(t.bfloat16(), ld, strides=(Lmax * ld, ld, 1), span_rows=B * Lmax, kind=kind, poison_row=row if kind == "big" else None)


def _packed_out(B, L, ld, col0, ncols, name):
    """A guarded [B, L, ncols] column slice (from col0) of packed [B, L + 7, ld] rows."""
    Lmax = L + PAD_ROWS
    return guarded((B, L, ncols), ld, torch.bfloat16, strides=(Lmax * ld, ld, 1), offset=col0, span_rows=B * Lmax, name=name)


def _heads(t, H):
    return t.unflatten(-1, (H, 64))


def _attn_fwd_run(ops, c, B, H, L, causal, q_log2, kind, Lk_decl=None):
    """attn_fwd on the packed buffer filled with `kind`; kind "plain": zeros in the pad rows, contiguous exact outputs."""
    D = H * 64
    P = _packed_in(c["qkv"], B, L, 3 * D, "zero" if kind == "plain" else kind, _poison_row_packed(c["u"], H))
    q, k, v = _heads(P[:, :, :D], H), _heads(P[:, :, D:2 * D], H), _heads(P[:, :, 2 * D:], H)
    if Lk_decl is not None:                                                  # (negative control: one more key row than there is)
        k = k.as_strided((B, Lk_decl, H, 64), k.stride(), k.storage_offset())
        v = v.as_strided((B, Lk_decl, H, 64), v.stride(), v.storage_offset())
    guards = []
    if kind == "plain":
        o, lse = torch.zeros(B, L, H, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(B, H, L, device="cuda")
    else:
        og = _packed_out(B, L, 3 * D, D, D, "o")
        lg = guarded((B, H, L), 64, torch.float32, strides=(H * L, L, 1), name="lse")
        guards = [og, lg]
        o, lse = _heads(og.view, H), lg.view
    ops.attn_fwd(q, k, v, o, lse, causal=causal, q_log2=q_log2)
    return dict(o=o, lse=lse, q=q, k=k, v=v), guards


FWD_MODES = {"dense": (False, False), "causal": (True, False), "q_log2": (False, True)}


@pytest.mark.parametrize("kind", ["nan", "big"])
@pytest.mark.parametrize("mode", list(FWD_MODES))
@pytest.mark.parametrize("L", ATTN_LENGTHS)
def test_attn_fwd_poison_past_the_end_and_guards(ops, L, mode, kind):
    """Rows L .. L + 7 of every batch of the packed q | k | v buffer (and the tail) poisoned: o and lse equal, bit for bit, the run
    with zeros there, stay within the bounds of test_attn_fwd (2e-3 lse, 2e-2 o) and leave the other columns, the pad rows and
    the guards of the packed output and of lse untouched."""
    B, H = 2, 2
    causal, q_log2 = FWD_MODES[mode]
    c = _attn_case(B, H, L, causal, q_log2)
    got, guards = _attn_fwd_run(ops, c, B, H, L, causal, q_log2, kind)
    plain, _ = _attn_fwd_run(ops, c, B, H, L, causal, q_log2, "plain")
    _check_all(guards)
    assert torch.equal(got["o"], plain["o"]) and torch.equal(got["lse"], plain["lse"])
    e_lse, e_o = _err(got["lse"], c["lse"].cuda()), _err(got["o"], c["o"].cuda())
    print(f"attn fwd L={L} {mode} {kind}: lse {e_lse:.3e} o {e_o:.3e}")
    assert e_lse < 2e-3 and e_o < 2e-2


BWD_MODES = {"two_kernel": (False, False), "two_kernel_causal": (True, False), "fused": (False, "force")}


def _attn_bwd_run(ops, c, B, H, L, causal, fused, kind):
    D = H * 64
    fwd, _ = _attn_fwd_run(ops, c, B, H, L, causal, False, "plain")
    zk = "zero" if kind == "plain" else kind
    P = _packed_in(c["qkv"], B, L, 3 * D, zk, _poison_row_packed(c["u"], H))
    q, k, v = _heads(P[:, :, :D], H), _heads(P[:, :, D:2 * D], H), _heads(P[:, :, 2 * D:], H)
    d_o = _heads(_packed_in(c["d_o"].reshape(B, L, D), B, L, D, zk, torch.full((D,), V_POISON)), H)
    o_in = _heads(_packed_in(fwd["o"].cpu().reshape(B, L, D), B, L, D, zk, torch.full((D,), V_POISON)), H)
    guards = []
    if kind == "plain":
        gq = torch.zeros(B, L, D, dtype=torch.bfloat16, device="cuda")
        gkv = torch.zeros(B, L, 2 * D, dtype=torch.bfloat16, device="cuda")
        delta = torch.zeros(2, B, H, L, device="cuda")
        csq, csv = torch.full((D,), 0.25, device="cuda"), torch.full((D,), -0.5, device="cuda")
    else:
        gqg = _packed_out(B, L, 3 * D, 0, D, "dq")                           # dq: columns 0 .. D of packed rows, D .. 3D are guard
        gkvg = _packed_out(B, L, 3 * D, D, 2 * D, "dk | dv")                 # dk | dv: columns D .. 3D of another packed buffer
        # (delta is a workspace: whatever part of it a form of the backward leaves alone starts as in the plain run)
        dg = guarded((2, B, H, L), 64, torch.float32, strides=(B * H * L, H * L, L, 1), init=torch.zeros(2, B, H, L), name="delta")
        cq = guarded((D,), 64, torch.float32, init=torch.full((D,), 0.25), name="dq_colsum")
        cv = guarded((D,), 64, torch.float32, init=torch.full((D,), -0.5), name="dv_colsum")
        guards = [gqg, gkvg, dg, cq, cv]
        gq, gkv, delta, csq, csv = gqg.view, gkvg.view, dg.view, cq.view, cv.view
    dq, dk, dv = _heads(gq, H), _heads(gkv[:, :, :D], H), _heads(gkv[:, :, D:], H)
    ops.attn_bwd(q, k, v, o_in, d_o, fwd["lse"], delta, dq, dk, dv, causal=causal, dq_scale=0.5, dq_colsum=csq, dv_colsum=csv, fused=fused)
    if fused:
        assert ops.attn_bwd_fused_status() == 0
    return dict(dq=dq, dk=dk, dv=dv, delta=delta, csq=csq, csv=csv), guards


@pytest.mark.parametrize("kind", ["nan", "big"])
@pytest.mark.parametrize("mode", list(BWD_MODES))
@pytest.mark.parametrize("L", ATTN_LENGTHS)
def test_attn_bwd_poison_past_the_end_and_guards(ops, L, mode, kind):
    """The backward (two kernels, dense and causal; the fused kernel forced) with q, k, v, o and d_o in buffers whose pad rows are
    poisoned: dq, dk, dv, delta and the fused column sums equal the zero-padded run bit for bit, match the fp64 gradients within
    test_attn_bwd's tol() and column-sum bounds, and every packed output keeps its other columns, pad rows and guards."""
    B, H = 2, 2
    causal, fused = BWD_MODES[mode]
    c = _attn_case(B, H, L, causal, False)
    got, guards = _attn_bwd_run(ops, c, B, H, L, causal, fused, kind)
    plain, _ = _attn_bwd_run(ops, c, B, H, L, causal, fused, "plain")
    _check_all(guards)
    for name in got:
        assert torch.equal(got[name], plain[name]), (name, float((got[name].double() - plain[name].double()).abs().max()))
    tol = lambda ref: 2e-2 * max(1.0, float(ref.abs().max()))
    for name in ("dq", "dk", "dv"):
        e = _err(got[name], c[name].cuda())
        print(f"attn bwd L={L} {mode} {kind}: {name} {e:.3e} (tol {tol(c[name]):.3e})")
        assert e < tol(c[name]), name
    D = H * 64
    assert _err(got["csq"], 0.25 + got["dq"].double().sum((0, 1)).view(D)) < 1e-3 * (1 + B * L) ** 0.5
    assert _err(got["csv"], -0.5 + got["dv"].double().sum((0, 1)).view(D)) < 1e-3 * (1 + B * L) ** 0.5


EDGE_L = 150
EDGE_KEYS = [0, ATTN_KV_TILE - 1, ATTN_KV_TILE, ATTN_BWD_KEY_BLOCK - 1, ATTN_BWD_KEY_BLOCK, EDGE_L - 1]


@pytest.mark.parametrize("mode", list(FWD_MODES))
@pytest.mark.parametrize("p", EDGE_KEYS)
def test_attn_fwd_edge_key_dominates(ops, p, mode):
    """One key -- the first, the last of a tile or key block, the first of the next, the last of all -- takes > 0.99 of the softmax
    of every row that may see it (checked in the reference) and carries v = 4: a kernel that drops it, or shows it to a causal row
    above the diagonal, misses the bound of test_attn_fwd by about 4."""
    B, H = 1, 2
    causal, q_log2 = FWD_MODES[mode]
    c = _attn_case(B, H, EDGE_L, causal, q_log2, p)
    got, guards = _attn_fwd_run(ops, c, B, H, EDGE_L, causal, q_log2, "nan")
    _check_all(guards)
    assert float(c["o"][:, max(p, 0) if causal else 0:].min()) > 3.9
    assert _err(got["lse"], c["lse"].cuda()) < 2e-3
    assert _err(got["o"], c["o"].cuda()) < 2e-2


@pytest.mark.parametrize("mode", list(BWD_MODES))
@pytest.mark.parametrize("p", EDGE_KEYS)
def test_attn_bwd_edge_key_dominates(ops, p, mode):
    """The same construction through the backward: dv[p] (the sum of nearly every d_o row) and dk[p] match the fp64 gradients."""
    B, H = 1, 2
    causal, fused = BWD_MODES[mode]
    c = _attn_case(B, H, EDGE_L, causal, False, p)
    got, guards = _attn_bwd_run(ops, c, B, H, EDGE_L, causal, fused, "nan")
    _check_all(guards)
    tol = lambda ref: 2e-2 * max(1.0, float(ref.abs().max()))
    for name in ("dv", "dk"):
        assert _err(got[name][:, p], c[name][:, p].cuda()) < tol(c[name]), name
        assert _err(got[name], c[name].cuda()) < tol(c[name]), name
    assert _err(got["dq"], c["dq"].cuda()) < tol(c["dq"])


def test_negative_control_attn_fwd_one_key_too_many(ops):
    """The poison test can fail: the forward told Lk + 1 while row Lk holds the aligned poison (inside our own buffer: the pad rows)
    -- the comparison with the reference over Lk keys must miss the bound, and by a lot (v = 100 there)."""
    B, H, L = 2, 2, ATTN_KV_TILE + 1
    c = _attn_case(B, H, L, False, False)
    got, _ = _attn_fwd_run(ops, c, B, H, L, False, False, "big", Lk_decl=L + 1)
    e = _err(got["o"], c["o"].cuda())
    print(f"negative control: attn_fwd with Lk + 1 declared misses by {e:.3e}")
    assert not (e < 2e-2) and e > 50.0


# ---- attn_decode: K / V caches [n_slots, Lk + 7, D], rows past Lk poisoned; q rows and o rows with a padded stride
DECODE_LENGTHS = [40, DECODE_TRIP - 1, DECODE_TRIP + 1]
DECODE_MODES = {"shared_g1": (1, False), "shared_g4": (4, False), "ancestry": (3, True)}          # (group, ancestry table)
DECODE_EDGE_L = 300
DECODE_EDGE_KEYS = [0, DECODE_GROUPS - 1, DECODE_GROUPS, DECODE_TRIP - 1, DECODE_TRIP, DECODE_EDGE_L - 1]


@functools.lru_cache(maxsize=None)
def _decode_case(group, anc_mode, Lk, p=None):
    B0, H = 2, 3
    g = torch.Generator().manual_seed(100 + Lk + group + (0 if p is None else 31 * (p + 1)))
    D, R = H * 64, B0 * group
    n_slots = R if anc_mode else B0
    u = _unit(g)
    q = _bf(_q_rows(g, (R, H), u, 0.3, 1.5))
    k, v = torch.randn(n_slots, Lk, D, generator=g), torch.randn(n_slots, Lk, D, generator=g)
    if p is not None:
        k[:, p] = (2 * K_ALIGN * u).repeat(H)                                # score 3 K_ALIGN again (the queries carry 1.5 u here)
        v[:, p] = 4.0
    k, v = _bf(k), _bf(v)
    if anc_mode:
        anc = (torch.randint(0, group, (R, Lk + PAD_ROWS), generator=g) + (torch.arange(R) // group * group)[:, None]).to(torch.int32)
        t = torch.arange(Lk)
        kg, vg = k[anc[:, :Lk].long(), t[None, :]], v[anc[:, :Lk].long(), t[None, :]]
    else:
        anc = None
        kg, vg = k.repeat_interleave(group, dim=0), v.repeat_interleave(group, dim=0)
    s = torch.einsum("rhd,rthd->rht", q.double(), kg.view(R, Lk, H, 64).double())
    prob = torch.softmax(s, -1)
    if p is not None:
        assert float(prob[:, :, p].min()) > 0.99
    ref = torch.einsum("rht,rthd->rhd", prob, vg.view(R, Lk, H, 64).double())
    return dict(q=q, k=k, v=v, anc=anc, u=u, ref=ref, R=R, H=H, n_slots=n_slots)


def _decode_run(ops, c, group, Lk, kind):
    R, H, n = c["R"], c["H"], c["n_slots"]
    D = H * 64
    zk = "zero" if kind == "plain" else kind
    kd = _heads(_packed_in(c["k"], n, Lk, D, zk, (2 * K_ALIGN * c["u"]).repeat(H)), H)
    vd = _heads(_packed_in(c["v"], n, Lk, D, zk, torch.full((D,), V_POISON)), H)
    anc = None if c["anc"] is None else c["anc"].cuda()
    if kind == "plain":
        qd, o, guards = c["q"].bfloat16().cuda(), torch.zeros(R, H, 64, dtype=torch.bfloat16, device="cuda"), []
    else:
        qd = _heads(poisoned(c["q"].bfloat16().view(R, D), D + 8, kind=kind), H)
        og = guarded((R, D), D + 8, torch.bfloat16, name="o")
        o, guards = _heads(og.view, H), [og]
    ops.attn_decode(qd, kd, vd, o, group=1 if anc is not None else group, anc=anc)
    return o, guards


@pytest.mark.parametrize("kind", ["nan", "big"])
@pytest.mark.parametrize("mode", list(DECODE_MODES))
@pytest.mark.parametrize("Lk", DECODE_LENGTHS)
def test_attn_decode_poison_past_the_end_and_guards(ops, Lk, mode, kind):
    """Caches longer than Lk with the rows past Lk poisoned (shared mode, group 1 and 4; ancestry mode, whose table has Lk + 7
    columns): the output equals the zero-padded run bit for bit, stays within test_gpu_attn_decode's 2e-2 and within its rows."""
    group, anc_mode = DECODE_MODES[mode]
    c = _decode_case(group, anc_mode, Lk)
    o, guards = _decode_run(ops, c, group, Lk, kind)
    plain, _ = _decode_run(ops, c, group, Lk, "plain")
    _check_all(guards)
    assert torch.equal(o, plain)
    e = _err(o, c["ref"].cuda())
    print(f"attn_decode Lk={Lk} {mode} {kind}: {e:.3e}")
    assert e < 2e-2


@pytest.mark.parametrize("mode", list(DECODE_MODES))
@pytest.mark.parametrize("p", DECODE_EDGE_KEYS)
def test_attn_decode_edge_key_dominates(ops, p, mode):
    group, anc_mode = DECODE_MODES[mode]
    c = _decode_case(group, anc_mode, DECODE_EDGE_L, p)
    o, guards = _decode_run(ops, c, group, DECODE_EDGE_L, "nan")
    _check_all(guards)
    assert float(c["ref"].min()) > 3.9
    assert _err(o, c["ref"].cuda()) < 2e-2


# ================================================================================================ row kernels: the guard check only
@pytest.mark.parametrize("D,B,T", list(ROW_ROUTE_CASES))
def test_row_kernel_outputs_stay_inside_their_rows(ops, D, B, T):
    """The five shapes of test_row_kernel_routes_at_small_shapes (each call asserts its route) with h_out, y_bf16, mean, rstd,
    g_out and g_out_bf16 in guarded buffers: every logical element is written and nothing outside.  Parity is that test's."""
    fwd_r, bwd_r, lnf_r, lnb_r = ROW_ROUTE_CASES[(D, B, T)]
    rows = B * T
    g = torch.Generator().manual_seed(D + rows)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    h, st = rnd(rows, D), torch.softmax(torch.randn(B, 4, T, generator=g), 1).cuda()
    w, b = [1 + 0.1 * rnd(D) for _ in range(4)], [0.1 * rnd(D) for _ in range(4)]
    lw, lb = 1 + 0.1 * rnd(D), 0.1 * rnd(D)
    dy, gres = rnd(rows, D).bfloat16(), rnd(rows, D)
    mat = lambda dt, name: guarded((rows, D), D, dt, name=name)
    vec = lambda name: guarded((rows,), 64, torch.float32, name=name)
    new = lambda: torch.zeros(D, device="cuda")
    ho, yb, mean, rstd = mat(torch.float32, "h_out"), mat(torch.bfloat16, "y_bf16"), vec("mean"), vec("rstd")
    with _ExpectRoute(fwd_r):
        ops.fddt_ln_fwd(h, rows, D, mode=ops.MODE_DIAG, stno=st, T=T, w=w, b=b, h_out=ho.view, ln_w=lw, ln_b=lb, y_bf16=yb.view,
                        mean=mean.view, rstd=rstd.view)
    y2, m2, r2 = mat(torch.bfloat16, "ln y_bf16"), vec("ln mean"), vec("ln rstd")
    x = ho.view.clone()
    with _ExpectRoute(lnf_r):
        ops.fddt_ln_fwd(x, rows, D, mode=ops.MODE_NONE, ln_w=lw, ln_b=lb, y_bf16=y2.view, mean=m2.view, rstd=r2.view)
    all_guards = [ho, yb, mean, rstd, y2, m2, r2]
    for want_bf16 in (True, False):
        g0, g0b = mat(torch.float32, "g_out"), (mat(torch.bfloat16, "g_out_bf16") if want_bf16 else None)
        with _ExpectRoute(bwd_r + ("_bf16" if want_bf16 else "_f32") if bwd_r == "staged" else bwd_r):
            ops.fddt_ln_bwd(h, rows, D, mode=ops.MODE_DIAG, stno=st, T=T, w=w, b=b, ln_w=lw, mean=mean.view, rstd=rstd.view, d_y=dy, g_res=gres,
                            g_out=g0.view, g_out_bf16=None if g0b is None else g0b.view, dln_w=new(), dln_b=new(),
                            dw=[new() for _ in range(4)], db=[new() for _ in range(4)], colsum_out=new())
        all_guards += [g0] + ([g0b] if want_bf16 else [])
    g1, g1b = mat(torch.float32, "ln g_out"), mat(torch.bfloat16, "ln g_out_bf16")
    with _ExpectRoute(lnb_r):
        ops.fddt_ln_bwd(x, rows, D, mode=ops.MODE_NONE, ln_w=lw, mean=m2.view, rstd=r2.view, d_y=dy, g_res=gres, g_out=g1.view, g_out_bf16=g1b.view,
                        dln_w=new(), dln_b=new(), colsum_out=new())
    for gd in all_guards + [g1, g1b]:
        gd.check()
        assert gd.untouched_inside() == 0, gd.name

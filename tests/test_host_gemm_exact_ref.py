"""tests/gemm_exact_ref.py pinned on the CPU: the conditions under which "bit for bit" is a fair demand hold at every shape of
tests/test_gpu_gemm_epilogue_exact.py (exact accumulation in any order; the wrong rounding points are visible in at least 5 % of the
elements they concern), a correct fp32 emulation of the epilogue -- numpy fp32 accumulation in a shuffled k order -- passes both
comparators, and every wrong variant is rejected by them.  These are the negative controls: no GPU test provokes anything."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import gemm_exact_ref as R

amd_pkg.load()

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SHAPE_IDS = [s[0] for s in R.SHAPES]
# the emulation and the negative controls run where the fp64 reference of all epilogues takes well under a second on the CPU
SMALL_IDS = [s[0] for s in R.SHAPES if s[1] * s[2] * s[4] <= 3_000_000]

_cache = {}


def _problem(sid):
    if sid not in _cache:
        _cache.clear()
        inp = R.make_inputs(sid)
        _cache[sid] = (inp, R.accumulate64(inp))
    return _cache[sid]


def test_flags_are_the_librarys():
    from ts_asr_whisper_amd import _lib as L
    assert (R.BIAS, R.GELU, R.RESIDUAL, R.OUT_F32, R.SCALE_N, R.GELU_BWD, R.ACCUM, R.GELU_DAUX, R.MUL_AUX, R.COLSUM) == \
        (L.EPI_BIAS, L.EPI_GELU, L.EPI_RESIDUAL, L.EPI_OUT_F32, L.EPI_SCALE_N, L.EPI_GELU_BWD, L.EPI_ACCUM, L.EPI_GELU_DAUX, L.EPI_MUL_AUX,
         L.EPI_COLSUM)


def test_bf16_rounding_primitive():
    """R.bf16 against torch's fp32 -> bf16 conversion (one rounding, ties to even) on fp32 values, on exact ties, on every bf16 value
    (a fixed point) and on subnormals; R.ulp_bf16 against the distance between neighbouring bf16 values."""
    g = torch.Generator().manual_seed(1)
    x = torch.cat((torch.randn(20000, generator=g) * 3, torch.randn(2000, generator=g) * 1e-3, torch.randn(2000, generator=g) * 1e-39,
                   torch.arange(-1024, 1025).float() / 256, torch.tensor([0.0, -0.0, 1.0, 255.5, 256.5, 3.0e38])))
    assert torch.equal(R.bf16(x.double()), x.to(BF16).double())
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 2.0 ** -126 * (1 + 2.0 ** -8)], dtype=F64)   # (2 j + 1) half-steps
    assert torch.equal(R.bf16(ties), torch.tensor([1.0, 1.015625, -1.0, 2.0 ** -126], dtype=F64))
    assert torch.equal(R.bf16(ties[:3], "away"), torch.tensor([1.0078125, 1.015625, -1.0078125], dtype=F64))
    allb = torch.arange(0, 0x7f80, dtype=torch.int32).to(torch.int16).view(BF16).double()      # every finite bf16 value >= 0, ascending
    assert torch.equal(R.bf16(allb), allb)
    assert torch.equal(R.ulp_bf16(allb[:-1]), allb[1:] - allb[:-1])
    grid = R.dense_bf16_grid()
    assert grid.numel() == 33314 and float(grid.float().abs().max()) == 9.0


def test_case_table():
    cs = R.cases()
    assert len(set(cs)) == len(cs)
    names = {R.expected_kernel(s, e) for s, e in cs}
    want = {"gemm_nt_kernel<2, false>", "gemm_nt64_kernel<8>", "gemm_nt64_kernel<4>", "gemm_nt128t_kernel", None}
    for f in (-1,) + R.RING_CT:
        want.add("gemm_ntr_kernel<%d, 4, 4>" % f)
        if f != 0:                                         # <0, 3, 5> cannot be reached (R.expected_kernel)
            want.add("gemm_ntr_kernel<%d, 3, 5>" % f)
    assert names == want
    for sid in SHAPE_IDS:
        nc = R.scale_ncols(R.SHAPE[sid][2])
        assert nc % 4 == 0 and nc % 16 != 0 and 0 < nc < R.SHAPE[sid][2]


@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_conditions_hold(sid):
    inp, acc = _problem(sid)
    ex, ds = R.check_conditions(inp, acc, epilogues=sid != "splitk")
    print(sid, {k: "2^%.1f" % np.log2(max(v, 1.0)) for k, v in ex.items()}, {k: "%.3f" % v for k, v in ds.items()})


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation
def _acc_fp32_shuffled(inp, seed):
    """numpy fp32: the k range cut into shuffled chunks whose partial products are added one after the other."""
    M, N, K, batch = inp["M"], inp["N"], inp["K"], inp["batch"]
    A, B = inp["A"].float().numpy(), inp["B"].float().numpy()
    rng = np.random.default_rng(seed)
    out = np.zeros((batch * M, N), np.float32)
    for b in range(batch):
        perm = rng.permutation(K)
        for ch in np.array_split(perm, max(2, K // 24)):
            out[b * M:(b + 1) * M] += A[b * M:(b + 1) * M][:, ch] @ B[b * N:(b + 1) * N][:, ch].T
    return torch.from_numpy(out)


def _emulate(acc32, flags, inp):
    """A correct kernel in fp32: one fp32 operation per step of nt_epilogue_math, torch's fp32 -> bf16 conversion at the rounding points,
    the transcendentals as the fp32 rounding of their fp64 values."""
    bf = lambda t: t.to(BF16).float()
    v = acc32.clone()
    aux = None
    if flags & R.BIAS:
        v = v + inp["bias"]
    if flags & R.SCALE_N:
        v[:, :inp["scale_ncols"]] *= np.float32(inp["scale"])
    if flags & R.GELU:
        xb = bf(v)
        aux = R.gelu_grad64(xb.double()).float().to(BF16) if flags & R.GELU_DAUX else v.to(BF16)
        v = R.gelu64(xb.double()).float()
    if flags & R.MUL_AUX:
        v = v * inp["dgelu"].float()
    if flags & R.GELU_BWD:
        v = v * R.gelu_grad64(inp["pre"].double()).float()
    if flags & R.RESIDUAL:
        v = bf(v) + inp["residual"]
    if flags & R.ACCUM:
        v = v + inp["residual"]
    C = v if flags & R.OUT_F32 else v.to(BF16)
    return C, aux, v.sum(0, dtype=F32), C.float().sum(0, dtype=F32)


def _compare(eid, got_C, got_aux, ref, acc):
    """The comparator each epilogue is held to (the same choice as the GPU file's); returns the worst error in units of the bound."""
    fl = R.full_flags(eid)
    if fl & R.GELU:
        r = R.rounded_ratio(got_C, ref["v"], 1e-6)
        if fl & R.GELU_DAUX:
            return max(r, R.rounded_ratio(got_aux, ref["aux_v"], R.GELU_GRAD_D))
        return r if R.exact(got_aux, ref["aux"]) else float("inf")
    if fl & R.GELU_BWD:
        return R.rounded_ratio(got_C, ref["v"], 2 * R.GELU_GRAD_D * acc.abs().clamp(min=1.0))
    return 0.0 if R.exact(got_C, ref["C"]) else float("inf")


@pytest.mark.parametrize("sid", SMALL_IDS)
def test_fp32_emulation_in_shuffled_order_passes(sid):
    inp, acc = _problem(sid)
    a1, a2 = _acc_fp32_shuffled(inp, 1), _acc_fp32_shuffled(inp, 2)
    assert torch.equal(a1, a2) and torch.equal(a1.double(), acc)            # order independence: the accumulator IS the fp64 value
    for s, eid in R.cases():
        if s != sid:
            continue
        fl = R.full_flags(eid)
        ref = R.reference(acc, fl, inp)
        C, aux, cs_pre, cs_stored = _emulate(a1, fl, inp)
        assert _compare(eid, C, aux, ref, acc) <= 1.0, (sid, eid)
        if fl & R.COLSUM:
            assert R.exact(cs_pre, ref["colsum_pre"]) and R.exact(cs_stored, ref["colsum_stored"])


# ---------------------------------------------------------------------------------------------------------------- negative controls
WRONG = [("res_before_round", "bias_res_f32"), ("gelu_unrounded", "bias_gelu"), ("bias_after_scale", "bias_scale_f32"),
         ("bias_after_scale", "bias_scale_bf16"), ("scale_quad", "bias_scale_f32"), ("scale_quad", "bias_scale_bf16"),
         ("half_away", "plain_bf16"), ("half_away", "bias"), ("half_away", "mul_aux")]


@pytest.mark.parametrize("sid", [s for s in SMALL_IDS if s != "splitk"])
def test_wrong_variants_are_rejected(sid):
    inp, acc = _problem(sid)
    for wrong, eid in WRONG:
        fl = R.full_flags(eid)
        ref, bad = R.reference(acc, fl, inp), R.reference(acc, fl, inp, wrong)
        got = bad["C"].to(F32 if fl & R.OUT_F32 else BF16)
        aux = None if bad["aux"] is None else bad["aux"].to(BF16)
        assert _compare(eid, got, aux, ref, acc) > 1.0, (sid, wrong, eid)
    # a saved pre-activation that is not the bits the activation saw (here: one bf16 step off wherever the rounding was inexact)
    ref = R.reference(acc, R.BIAS | R.GELU, inp)
    off = ref["pre"] + (ref["pre"] - ref["aux"])
    assert not R.exact(R.bf16(off).to(BF16), ref["aux"])
    # the other meaning of the column sums
    ref = R.reference(acc, R.MUL_AUX, inp)
    assert not R.exact(ref["colsum_stored"].float(), ref["colsum_pre"]) and not R.exact(ref["colsum_pre"].float(), ref["colsum_stored"])


def test_tanh_gelu_and_a_coarse_derivative_are_rejected_on_the_dense_grid():
    x = R.dense_bf16_grid().double()
    ref = R.gelu64(x)
    assert R.rounded(ref.float().to(BF16), ref, 1e-6) and R.rounded(R.bf16(ref), ref, 0.0)
    bad = R.gelu_tanh64(x).float().to(BF16)
    n = R.rounded_violations(bad, ref, 1e-6)
    print("tanh-form GELU: %d of %d bf16 inputs violate rounded(.., 1e-6)" % (n, x.numel()))
    assert n > 100 and not R.rounded(bad, ref, 1e-6)
    # gelu' off in the fourth digit: outside the fp32 bound everywhere it matters, and outside `rounded` for the bf16 results
    dref = R.gelu_grad64(x)
    dbad = dref * (1 + 3e-4)
    assert R.within_ratio(dref.float(), dref, R.GELU_GRAD_D) <= 1.0 and R.within_ratio(dbad.float(), dref, R.GELU_GRAD_D) > 1.0
    assert R.rounded(dref.float().to(BF16), dref, R.GELU_GRAD_D) and not R.rounded(dbad.float().to(BF16), dref, R.GELU_GRAD_D)


def test_identity_product_reproduces_the_grid():
    a, b = R.dense_a(528, 64), R.identity_b(132, 64)
    c = a.double() @ b.double().T
    assert torch.equal(c[:, :64], a.double()) and torch.equal(c[:, 64:128], a.double()) and torch.equal(c[:, 128:], a.double()[:, :4])
    assert torch.unique(a.view(torch.int16)).numel() == 33314

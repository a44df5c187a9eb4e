"""Exact-arithmetic inputs and the fp64 reference of dicow_gemm_nt's epilogues (include/dicow_hip.h), shared by
tests/test_host_gemm_exact_ref.py (which checks, on the CPU, that the inputs make the accumulator exact, that the reference can tell
the wrong rounding points from the right ones and that the comparators reject them) and tests/test_gpu_gemm_epilogue_exact.py (which
uses it as the oracle for every kernel family and every epilogue instantiation).

The operands come from dyadic grids (A = i / 16, B = j / 16, bias = i / 32, ...): every product and every partial sum is a multiple of
2^-8 far below 2^24 of them, so the fp32 accumulator of ANY summation order holds the fp64 value exactly.  The reference then applies
the header's rounding points in the order of nt_epilogue_math (csrc/gemm.hip) with an explicit bf16 round-to-nearest-even, and a
kernel has to reproduce it bit for bit -- except where a transcendental is involved (GELU, gelu'), where the result has to be a correct
bf16 rounding of something within a stated distance of the fp64 value (`rounded`).

Plain torch; every function works on CPU and GPU tensors alike (integer bit operations instead of frexp / ldexp / pow)."""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

# the epilogue flags of include/dicow_hip.h (tests/test_host_gemm_exact_ref.py checks them against ts_asr_whisper_amd._lib)
BIAS, GELU, RESIDUAL, OUT_F32, SCALE_N, GELU_BWD, ACCUM, GELU_DAUX, MUL_AUX, COLSUM = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512

SCALE = 0.125
# The bound on the device's gelu' (common.h's gelu_erf_grad) against fp64: TWICE the worst fp32 error over every bf16 input of [-9, 9],
# measured once on the MI355X through the fp32-out GELU_BWD identity product on the scalar path (1.8386e-7, the same on the ring
# kernel's run-time-flag path: profiles/gemm_epilogue_exact.txt; tests/test_gpu_gemm_epilogue_exact.py::test_gelu_bwd_dense_grid prints it).
# The expression is the same instruction sequence on every board; the factor 2 covers the approximate v_exp_f32 / v_rcp_f32 alone (a
# CPU emulation of the expression with correctly rounded exp2 / rcp gives 1.8e-7).
GELU_GRAD_MEASURED = 1.8386e-7
GELU_GRAD_D = 2 * GELU_GRAD_MEASURED


# ---------------------------------------------------------------------------------------------------------------- bf16 in fp64
def ulp_bf16(x):
    """Spacing of the bf16 grid at |x| (fp64 tensor): 2^(floor(log2|x|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    e = ((x.to(F64).contiguous().view(torch.int64) >> 52) & 0x7ff) - 1023          # floor(log2 |x|) of a normal fp64
    return (((e - 7).clamp(min=-133) + 1023) << 52).view(F64)


def bf16(x, mode="even"):
    """x (fp64) rounded ONCE to the nearest bf16 value, ties to even, result in fp64.  (x.to(bfloat16) would round to fp32 first.)
    mode "away" rounds ties away from zero: a wrong variant for the negative controls."""
    x = x.to(F64)
    q = ulp_bf16(x)
    t = x / q                                                                      # exact: q is a power of two
    r = torch.round(t) if mode == "even" else torch.sign(t) * torch.floor(t.abs() + 0.5)
    return r * q


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def dense_bf16_grid():
    """Every finite bf16 value with |x| <= 9 (33 314 of them: bit patterns 0x0000 ... 0x4110 with either sign), as bf16."""
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    return allb[torch.isfinite(allb.float()) & (allb.float().abs() <= 9.0)].clone()


# ---------------------------------------------------------------------------------------------------------------- comparators
def exact(got, ref):
    """Bit equality of a kernel result (fp32 or bf16 tensor) with the fp64 reference, which must be representable in got's type."""
    r = ref.to(got.dtype)
    assert torch.equal(r.to(F64), ref.to(F64)), "the reference is not representable in the result type: the case is not exact"
    return torch.equal(got, r)


def rounded_ratio(got, ref, slack):
    """max over the elements of |got - ref| / (ulp_bf16(max(|got|, |ref|)) / 2 + slack): <= 1 says every element is a correct bf16
    rounding of something within `slack` (a float or an fp64 tensor) of the fp64 value."""
    g, r = got.to(F64), ref.to(F64)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    bound = ulp_bf16(torch.maximum(g.abs(), r.abs())) * 0.5 + slack
    return float(((g - r).abs() / bound).max())


def rounded_violations(got, ref, slack):
    g, r = got.to(F64), ref.to(F64)
    bound = ulp_bf16(torch.maximum(g.abs(), r.abs())) * 0.5 + slack
    return int(((g - r).abs() > bound).sum())


def rounded(got, ref, slack):
    return rounded_ratio(got, ref, slack) <= 1.0


def within_ratio(got, ref, slack):
    """fp32 results of a transcendental: max |got - ref| / slack (no rounding allowance at all)."""
    g = got.to(F64)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float(((g - ref.to(F64)).abs() / slack).max())


# ---------------------------------------------------------------------------------------------------------------- cases
# (id, M, N, K, batch, kernel instantiation ops.gemm_dispatch_log() must name; "ring44" / "ring35": gemm_ntr_kernel<F, 4, 4> / <F, 3, 5> with
# F from RING_CT; None: the skinny kernel, which has no log entry).  The ring shapes assume the 256 CUs nt_plan balances its rounds for.
SHAPES = [
    ("generic", 200, 132, 64, 1, "gemm_nt_kernel<2, false>"),          # one k-step
    ("nt64x8_k448", 70, 68, 448, 1, "gemm_nt64_kernel<8>"),            # 4 workgroups, 7 k-steps: fewer than the ring is deep
    ("nt64x8", 1000, 500, 128, 1, "gemm_nt64_kernel<8>"),              # 128 workgroups
    ("nt64x4", 1000, 2040, 128, 1, "gemm_nt64_kernel<4>"),             # 128 tiles of 128 x 128, 512 workgroups of 64 x 64
    ("nt128t", 2100, 1156, 128, 1, "gemm_nt128t_kernel"),              # 170 tiles of 128, 45 of 256
    ("ring44", 6100, 2244, 128, 1, "ring44"),                          # 216 tiles of 256 x 256 (N > 2048: no 192 x 320)
    ("ring44_gelu", 6200, 2244, 128, 1, "ring44"),                     # BIAS | GELU: 225 tiles against 264 of 192 x 320 (two rounds)
    ("ring35", 8500, 1284, 128, 1, "ring35"),                          # 204 tiles against 225 of 192 x 320, one round each; 4-column tail
    ("skinny16", 16, 1284, 1280, 1, None),
    ("skinny7", 7, 36, 5120, 1, None),
    ("splitk", 200, 384, 8192, 1, "gemm_nt64_kernel<8>"),              # eight k ranges as the batches of one launch + the ordered sum
    ("batched3", 100, 128, 384, 3, "gemm_nt64_kernel<8>"),             # strideA / strideC / strideAux
]
SHAPE = {s[0]: s for s in SHAPES}
# A = integers in [-a, a] / 16, a = 8 except where that misses a condition of check_conditions: with one k-step the pre-activations are
# too small for the bf16 rounding to matter in 5 % of them (4.1 % at a = 8)
A_RANGE = {"generic": 16}

# (id, flags without OUT_F32 / COLSUM, fp32 result, fused column sums)
EPILOGUES = [
    ("plain_f32", 0, True, False),
    ("plain_bf16", 0, False, False),
    ("bias", BIAS, False, False),
    ("bias_scale_f32", BIAS | SCALE_N, True, False),
    ("bias_scale_bf16", BIAS | SCALE_N, False, False),
    ("bias_gelu", BIAS | GELU, False, False),
    ("bias_res_f32", BIAS | RESIDUAL, True, False),
    ("bias_gelu_daux", BIAS | GELU | GELU_DAUX, False, False),
    ("mul_aux", MUL_AUX, False, False),
    ("mul_aux_colsum", MUL_AUX, False, True),
    ("accum", ACCUM, True, False),
    ("gelu_bwd", GELU_BWD, False, False),
]
EPILOGUE = {e[0]: e for e in EPILOGUES}
# the compile-time epilogues of gemm_ntr_kernel (NT_EPILOGUES_COMMON of csrc/gemm.hip); every other flag set runs F = -1
RING_CT = (0, BIAS, BIAS | SCALE_N, BIAS | GELU, BIAS | RESIDUAL | OUT_F32, BIAS | GELU | GELU_DAUX, MUL_AUX, MUL_AUX | COLSUM)


def full_flags(epi):
    _, fl, f32, colsum = EPILOGUE[epi]
    return fl | (OUT_F32 if f32 else 0) | (COLSUM if colsum else 0)


def cases():
    """(shape id, epilogue id) of every GPU case."""
    out = []
    for sid, *_ in SHAPES:
        for eid, fl, f32, colsum in EPILOGUES:
            if sid == "splitk" and fl != 0:
                continue                                   # the split exists for products without an epilogue only
            if sid == "ring44" and eid == "bias_gelu":
                continue                                   # BIAS | GELU takes 192 x 320 tiles at M = 6100: see ring44_gelu
            if sid == "ring44_gelu" and eid != "bias_gelu":
                continue
            if sid == "batched3" and (colsum or (fl & RESIDUAL)):
                continue                                   # the ABI has no batch stride for the residual and no batched column sums
            out.append((sid, eid))
    return out


def expected_kernel(sid, eid):
    """What the dispatch log must name.  <0, 3, 5> is unreachable in the stable build (nt_plan's plain256 sends a product without any
    epilogue work to 256 x 256 tiles whatever the padding), so the plain bf16 product of the ring35 shape asserts <0, 4, 4>."""
    kern = SHAPE[sid][5]
    if kern not in ("ring44", "ring35"):
        return kern
    fl = full_flags(eid)
    ct = fl if fl in RING_CT else -1
    tile = "4, 4" if (kern == "ring44" or fl == 0) else "3, 5"
    return "gemm_ntr_kernel<%d, %s>" % (ct, tile)


def scale_ncols(N):
    """A multiple of 4 that is no multiple of 16, near N / 2: inside a tile (and inside a 16-column group) on every route."""
    return (N // 2) // 16 * 16 + 4


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g)


def make_inputs(sid):
    """The seeded operands of a shape (CPU tensors): A, B bf16; bias, residual / initial C fp32; the saved gelu' (MUL_AUX) and the
    saved pre-activation (GELU_BWD) bf16.  Batched shapes stack the batches along the rows of A / C / aux and of B."""
    _, M, N, K, batch, _ = SHAPE[sid]
    seed = 1000 * (1 + [s[0] for s in SHAPES].index(sid))
    pre_bits = dense_bf16_grid()
    pre_bits = pre_bits[pre_bits.float().abs() <= 4.0]
    return {
        "A": (_ints((batch * M, K), -A_RANGE.get(sid, 8), A_RANGE.get(sid, 8), seed + 1).float() / 16).to(BF16),
        "B": (_ints((batch * N, K), -4, 4, seed + 2).float() / 16).to(BF16),
        "bias": _ints((N,), -32, 32, seed + 3).float() / 32,
        "residual": _ints((batch * M, N), -512, 512, seed + 4).float() / 64,
        "dgelu": (_ints((batch * M, N), 0, 9, seed + 5).float() / 8).to(BF16),
        "pre": pre_bits[_ints((batch * M, N), 0, pre_bits.numel() - 1, seed + 6)],
        "scale": SCALE, "scale_ncols": scale_ncols(N), "M": M, "N": N, "K": K, "batch": batch,
    }


def accumulate64(inp, device=None):
    """The exact product [batch * M, N] in fp64."""
    M, N, batch = inp["M"], inp["N"], inp["batch"]
    A, B = inp["A"].to(device=device, dtype=F64), inp["B"].to(device=device, dtype=F64)
    return torch.cat([A[b * M:(b + 1) * M] @ B[b * N:(b + 1) * N].T for b in range(batch)], 0)


# ---------------------------------------------------------------------------------------------------------------- the reference
def reference(acc, flags, inp, wrong=None):
    """The epilogue on the exact accumulator `acc` (fp64 [batch * M, N]), operands from `inp` (moved to acc's device), rounding points of
    include/dicow_hip.h in the order of nt_epilogue_math.  Returns fp64 tensors: "pre" (the pre-activation), "aux" (what a GELU
    epilogue saves, else None; "aux_v": before its bf16 rounding), "v" (the result before the store rounding), "C" (the stored result), "colsum_pre" / "colsum_stored"
    (column sums of v / of C over all rows: the two meanings of DICOW_EPI_COLSUM).
    wrong: None, or one of the wrong variants the tests must be able to tell from the right one -- "res_before_round" (residual added
    before the bf16 rounding), "gelu_unrounded" (GELU at the unrounded pre-activation), "bias_after_scale", "scale_quad" (the
    scale_ncols boundary one quad further), "tanh" (tanh-form GELU), "half_away" (bf16 ties away from zero)."""
    dev = acc.device
    rnd = (lambda t: bf16(t, "away")) if wrong == "half_away" else bf16
    get = lambda k: inp[k].to(device=dev, dtype=F64)
    v = acc.clone()
    if (flags & BIAS) and wrong != "bias_after_scale":
        v = v + get("bias")
    if flags & SCALE_N:
        nc = inp["scale_ncols"] + (4 if wrong == "scale_quad" else 0)
        v[:, :nc] = v[:, :nc] * inp["scale"]
    if (flags & BIAS) and wrong == "bias_after_scale":
        v = v + get("bias")
    pre, aux, aux_v = v, None, None
    if flags & GELU:
        xb = pre if wrong == "gelu_unrounded" else rnd(pre)
        v = gelu_tanh64(xb) if wrong == "tanh" else gelu64(xb)
        aux_v = gelu_grad64(xb) if flags & GELU_DAUX else pre
        aux = rnd(aux_v)
    if flags & MUL_AUX:
        v = v * get("dgelu")
    if flags & GELU_BWD:
        v = v * gelu_grad64(get("pre"))
    if flags & RESIDUAL:
        v = rnd(v + get("residual")) if wrong == "res_before_round" else rnd(v) + get("residual")
    if flags & ACCUM:
        v = v + get("residual")                            # the initial C of the ACCUM case is the residual tensor
    C = v if flags & OUT_F32 else rnd(v)
    return {"pre": pre, "aux": aux, "aux_v": aux_v, "v": v, "C": C, "colsum_pre": v.sum(0), "colsum_stored": C.sum(0)}


# ---------------------------------------------------------------------------------------------------------------- conditions
def _units(x, unit):
    """max |x| in units of the grid's last bit; asserts that x lies on the grid."""
    t = x / unit
    assert bool((t == torch.round(t)).all()), "value off the dyadic grid"
    return float(t.abs().max()) if t.numel() else 0.0


def exactness(inp, acc=None):
    """{stage: largest magnitude in units of that stage's last bit} -- every one has to stay below 2^24 for the fp32 arithmetic of ANY
    summation order to be exact.  The accumulator's bound is max(|A| |B|^T + |bias|): the largest partial sum any order can meet."""
    M, N, batch = inp["M"], inp["N"], inp["batch"]
    A, B = inp["A"].to(F64).abs(), inp["B"].to(F64).abs()
    worst = torch.cat([A[b * M:(b + 1) * M] @ B[b * N:(b + 1) * N].T for b in range(batch)], 0) + inp["bias"].to(F64).abs()
    if acc is None:
        acc = accumulate64(inp)
    res, dg = inp["residual"].to(F64), inp["dgelu"].to(F64)
    u_acc, u_scaled, u_mul = 2.0 ** -8, 2.0 ** -8 * inp["scale"], 2.0 ** -11
    out = {"acc+bias": _units(worst, u_acc), "scaled": _units(worst * inp["scale"], u_scaled),
           "residual": _units(worst + res.abs(), u_acc), "accum": _units(worst + res.abs(), u_acc),
           "mul_aux": _units(worst * dg, u_mul)}
    prod = acc * dg                                        # MUL_AUX: the fp32 value and the stored bf16 value, both on the 2^-11 grid
    out["colsum_pre"] = _units(prod.abs().sum(0), u_mul)
    out["colsum_stored"] = _units(bf16(prod).abs().sum(0), u_mul)
    return out


def distinguishing(inp, acc=None):
    """Share of the concerned elements in which each wrong variant differs from the right reference (all >= 0.05 by the module's
    contract), and the share of GELU pre-activations below 4 in magnitude (>= 0.5)."""
    if acc is None:
        acc = accumulate64(inp)
    nc = inp["scale_ncols"]
    r_res = reference(acc, BIAS | RESIDUAL | OUT_F32, inp)
    w_res = reference(acc, BIAS | RESIDUAL | OUT_F32, inp, "res_before_round")
    r_gelu = reference(acc, BIAS | GELU, inp)
    w_gelu = reference(acc, BIAS | GELU, inp, "gelu_unrounded")
    r_sc = reference(acc, BIAS | SCALE_N | OUT_F32, inp)
    w_sc = reference(acc, BIAS | SCALE_N | OUT_F32, inp, "bias_after_scale")
    r_cs = reference(acc, MUL_AUX, inp)
    share = lambda a, b: float((a != b).double().mean())
    return {"res_before_round": share(r_res["C"], w_res["C"]),
            "gelu_unrounded": share(r_gelu["C"], w_gelu["C"]),
            "bias_after_scale": share(r_sc["C"][:, :nc], w_sc["C"][:, :nc]),
            "colsum_meaning": share(r_cs["colsum_pre"], r_cs["colsum_stored"]),
            "gelu_pre_below_4": float((r_gelu["pre"].abs() < 4.0).double().mean())}


def check_conditions(inp, acc=None, epilogues=True):
    """Asserts the module's contract for one shape and returns the figures.  Shapes that run no epilogue (the split contraction) are
    checked for the exactness of the product alone."""
    ex = exactness(inp, acc)
    keys = list(ex) if epilogues else ["acc+bias"]
    for k in keys:
        assert ex[k] < 2.0 ** 24, (k, ex[k])
    if not epilogues:
        return {k: ex[k] for k in keys}, {}
    ds = distinguishing(inp, acc)
    for k in ("res_before_round", "gelu_unrounded", "bias_after_scale", "colsum_meaning"):
        assert ds[k] >= 0.05, (k, ds[k])
    assert ds["gelu_pre_below_4"] >= 0.5, ds["gelu_pre_below_4"]
    return ex, ds


# ---------------------------------------------------------------------------------------------------------------- dense grid
def identity_b(N, K):
    """B [N, K] with B[n, k] = 1 where n % K == k: A . B^T repeats A's columns, C[m, n] = A[m, n % K], exactly."""
    b = torch.zeros(N, K)
    b[torch.arange(N), torch.arange(N) % K] = 1.0
    return b.to(BF16)


def dense_a(M, K):
    """A [M, K] bf16 holding every finite bf16 value of [-9, 9] (M * K >= 33 314), padded with repeats."""
    g = dense_bf16_grid()
    assert M * K >= g.numel()
    return g.repeat(-(-M * K // g.numel()))[:M * K].view(M, K).clone()

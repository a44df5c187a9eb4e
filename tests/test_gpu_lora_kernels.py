"""dicow_lora_down / dicow_lora_up / dicow_lora_wgrad against fp64 references computed from the same bf16 inputs with the kernels'
rounding points applied (include/dicow_hip.h): t = bf16(x A^T); the low-rank product is rounded to bf16, multiplied by s, rounded to
bf16, added to the base result in fp32 and the sum rounded once to the output type.  Operands are strided views inside poison
(tests/util.poisoned), outputs sit inside guard bands (tests/util.guarded).  Run with `pytest -m gpu`.

Bounds: those of test_gemm_nt_plain for the same kinds of quantity -- fp32 results 1e-4 * max(1, max|ref|), bf16 results 1e-2 * max(1,
max|ref|).  The `up` tests draw t and U from the grid {-1, -7/8, ..., 1}: their products and the sums of up to 192 of them are exact
in fp32, so the kernel's bf16 roundings of the low-rank product fall exactly where the fp64 reference's do and the fp32 bound measures
the addition alone (with free-running values one product in ~40000 rounds to the other bf16 neighbour, an error of one bf16 ulp of the
low-rank term that is no property of the kernel).  `down` and `wgrad` use free-running normal values."""
import math

import pytest
import torch

import amd_pkg
from tests.util import guarded, poisoned

pytestmark = pytest.mark.gpu
amd_pkg.load()

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CASES = [(1, 128, 16), (3, 256, 48), (67, 1280, 16), (130, 384, 32), (257, 5120, 16), (64, 1280, 8)]      # (M, K or N, R)
IDS = ["m%d_n%d_R%d" % c for c in CASES]
SCALES = (0.25, 2.0, 1.5)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ts_asr_whisper_amd as p
    from ts_asr_whisper_amd import ops, _lib
    return p, ops, _lib


def _rank(R):
    return 8 if R == 8 else 16


def _normal(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def _grid(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, shape, generator=g).float() / 8.0).to(BF16)


def _bound(ref, dtype):
    return (1e-4 if dtype == F32 else 1e-2) * max(1.0, float(ref.abs().max()))


def _err(got, ref):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), "poison reached the result"
    return float((got - ref).abs().max())


# ------------------------------------------------------------------------------------------------ down
@pytest.mark.parametrize("block", [False, True], ids=["dense", "block"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lora_down(env, case, block):
    _, ops, _ = env
    M, K, R = case
    r = _rank(R)
    nseg = R // r if block else 1
    x, v = _normal((M, nseg * K), 1), _normal((R, K), 2, K ** -0.5)
    xd, vd = x.double(), v.double()
    if block:
        ref = torch.cat([xd[:, j * K:(j + 1) * K] @ vd[j * r:(j + 1) * r].T for j in range(nseg)], 1)
    else:
        ref = xd @ vd.T
    t = guarded((M, R), R + 4, BF16, name="t")
    ops.lora_down(poisoned(x, nseg * K + 24), poisoned(v, K + 8), t.view, r, block=block)
    torch.cuda.synchronize()
    t.check()
    assert t.untouched_inside() == 0
    e = _err(t.view, ref)
    print(f"lora_down {case} block={block}: max err {e:.3e} (bound {_bound(ref, BF16):.3e})")
    assert e < _bound(ref, BF16)


# ------------------------------------------------------------------------------------------------ up
def _up_problem(case, block, dtype):
    M, N, R = case
    r = _rank(R)
    nseg = R // r if block else 1
    t, u = _grid((M, R), 3), _grid((R, N), 4)
    p = _normal((M, nseg * N), 5).to(dtype) if dtype == BF16 else torch.randn((M, nseg * N), generator=torch.Generator().manual_seed(5))
    td, ud = t.double(), u.double()
    if block:
        lr = [td[:, j * r:(j + 1) * r] @ ud[j * r:(j + 1) * r] for j in range(nseg)]
    else:
        lr = [td @ ud]
    # the product is exact here (module docstring), so rounding it from fp64 is rounding the kernel's fp32 accumulator
    lr = torch.cat([(b.to(BF16).float() * SCALES[j]).to(BF16).double() for j, b in enumerate(lr)], 1)
    return M, N, R, r, nseg, t, u, p, p.double() + lr


def _gelu64(x):
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * cdf, cdf + x * pdf


@pytest.mark.parametrize("inplace", [True, False], ids=["p_is_y", "p_not_y"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("block", [False, True], ids=["dense", "block"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lora_up(env, case, block, dtype, inplace):
    _, ops, _ = env
    M, N, R, r, nseg, t, u, p, ref = _up_problem(case, block, dtype)
    ld = nseg * N + 8
    if inplace:
        y = guarded((M, nseg * N), ld, dtype, init=p, name="y")
        pv = y.view
    else:
        y = guarded((M, nseg * N), ld, dtype, name="y")
        pv = poisoned(p, nseg * N + 16)
    ops.lora_up(poisoned(t, R + 8), poisoned(u, N + 2), pv, y.view, r, SCALES, block=block)
    torch.cuda.synchronize()
    y.check()
    assert y.untouched_inside() == 0
    ref = ref.to(dtype).double() if dtype == BF16 else ref
    e = _err(y.view, ref)
    print(f"lora_up {case} block={block} {dtype} inplace={inplace}: max err {e:.3e} (bound {_bound(ref, dtype):.3e})")
    assert e < _bound(ref, dtype)


@pytest.mark.parametrize("block", [False, True], ids=["dense", "block"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lora_up_gelu(env, case, block):
    """The GELU flag: values against fp64 erf, and gelu / gelu' BIT-equal to gemm_nt's EPI_GELU | EPI_GELU_DAUX epilogue run on the
    same pre-activation (the plain `up` result through an identity weight, which the MFMA reproduces exactly)."""
    _, ops, L = env
    M, N, R, r, nseg, t, u, p, ref = _up_problem(case, block, BF16)
    W = nseg * N
    tc, uc, pc = t.cuda(), u.cuda(), p.cuda()
    pre = torch.empty(M, W, dtype=BF16, device="cuda")
    ops.lora_up(tc, uc, pc, pre, r, SCALES, block=block)
    y, aux = guarded((M, W), W + 8, BF16, name="y"), guarded((M, W), W + 16, BF16, name="aux")
    ops.lora_up(tc, uc, pc, y.view, r, SCALES, block=block, gelu=True, aux=aux.view)
    eye = torch.eye(W, dtype=BF16, device="cuda")
    y2, aux2 = torch.empty(M, W, dtype=BF16, device="cuda"), torch.empty(M, W, dtype=BF16, device="cuda")
    ops.gemm_nt(pre, eye, y2, M, W, W, aux=aux2, flags=L.EPI_GELU | L.EPI_GELU_DAUX)
    torch.cuda.synchronize()
    y.check()
    aux.check()
    assert torch.equal(y.view.contiguous().view(torch.int16), y2.view(torch.int16)), "gelu differs from the GEMM epilogue's"
    assert torch.equal(aux.view.contiguous().view(torch.int16), aux2.view(torch.int16)), "gelu' differs from the GEMM epilogue's"
    g, dg = _gelu64(ref.to(BF16).double())
    assert _err(y.view, g) < _bound(g, BF16) and _err(aux.view, dg) < _bound(dg, BF16)
    # without aux only y is written; the MUL_AUX epilogue multiplies the sum (fp32 P) by a saved gelu'
    y3 = torch.empty(M, W, dtype=BF16, device="cuda")
    ops.lora_up(tc, uc, pc, y3, r, SCALES, block=block, gelu=True)
    y4 = torch.empty(M, W, dtype=BF16, device="cuda")
    ops.lora_up(tc, uc, pc.float(), y4, r, SCALES, block=block, mul_aux=True, aux=aux2)
    torch.cuda.synchronize()
    assert torch.equal(y3, y2)
    want = ref * aux2.double().cpu()
    assert _err(y4, want) < _bound(want, BF16)


# ------------------------------------------------------------------------------------------------ wgrad
@pytest.mark.parametrize("layout", ["rN", "Nr"])
@pytest.mark.parametrize("block", [False, True], ids=["dense", "block"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lora_wgrad(env, case, block, layout):
    """[r, N] (dA) and [N, r] (dB) destinations; accumulate = 0 over a NaN-filled destination, accumulate = 1 on top of values, and
    two runs bit-equal."""
    _, ops, _ = env
    M, N, R = case
    r = _rank(R)
    nseg = R // r
    t, p = _normal((M, R), 6), _normal((M, (nseg if block else 1) * N), 7)
    s = 2.0
    full = s * (t.double().T @ p.double())                                                   # [R, cols]
    refs = [full[j * r:(j + 1) * r, (j * N if block else 0):(j * N if block else 0) + N] for j in range(nseg)]
    shape, kw = ((r, N), dict(g_rs=N, g_cs=1)) if layout == "rN" else ((N, r), dict(g_rs=1, g_cs=r))
    if layout == "Nr":
        refs = [x.T for x in refs]
    tv, pv = poisoned(t, R + 8), poisoned(p, p.shape[1] + 24)

    def run(init, accumulate):
        outs = [guarded(shape, shape[1], F32, init=init, name=f"g{j}") for j in range(nseg)]
        ops.lora_wgrad(tv, pv, [o.view for o in outs], r, s, block=block, accumulate=accumulate, **kw)
        torch.cuda.synchronize()
        for o in outs:
            o.check()
        return outs

    first = run(None, False)                          # the sentinel is a NaN pattern: accumulate = 0 must not read it
    for o, ref in zip(first, refs):
        assert o.untouched_inside() == 0
        e = _err(o.view, ref)
        assert e < _bound(ref, F32), (e, _bound(ref, F32))
    again = run(None, False)
    assert all(torch.equal(a.view, b.view) for a, b in zip(first, again)), "two runs differ"
    base = torch.randn(shape, generator=torch.Generator().manual_seed(8))
    for o, ref in zip(run(base, True), refs):
        assert _err(o.view, ref + base.double()) < _bound(ref + base.double(), F32)
    if nseg > 1:                                      # a None destination is skipped, the others are as before
        outs = [guarded(shape, shape[1], F32, name=f"h{j}") for j in range(nseg)]
        ops.lora_wgrad(tv, pv, [None] + [o.view for o in outs[1:]], r, s, block=block, accumulate=False, **kw)
        torch.cuda.synchronize()
        assert outs[0].untouched_inside() == outs[0].view.numel()
        assert all(torch.equal(a.view, b.view) for a, b in zip(first[1:], outs[1:]))


# ------------------------------------------------------------------------------------------------ limits
def test_lora_limits_are_errors_and_launch_nothing(env):
    _, ops, L = env
    M, K = 32, 128

    def fresh(R, ld=None):
        return guarded((M, R), R if ld is None else ld, BF16, name="t")

    x = _normal((M, K), 9).cuda()
    cases = []
    t = fresh(24)
    cases.append((t, lambda: ops.lora_down(x, _normal((24, K), 10).cuda(), t.view, 12)))                          # r = 12
    t2 = fresh(256)
    cases.append((t2, lambda: ops.lora_down(x, _normal((256, K), 11).cuda(), t2.view, 16)))                       # R = 256
    t3 = fresh(16)
    cases.append((t3, lambda: ops.lora_down(poisoned(x.cpu(), K + 4), _normal((16, K), 12).cuda(), t3.view, 16)))  # ldx % 8 != 0
    y = guarded((M, K), K, BF16, name="y")
    tt = _normal((M, 24), 13).cuda()
    cases.append((y, lambda: ops.lora_up(tt, _normal((24, K), 14).cuda(), y.view, y.view, 12, [1.0])))            # r = 12
    y2 = guarded((M, K), K + 4, BF16, name="y")
    cases.append((y2, lambda: ops.lora_up(tt[:, :16].contiguous(), _normal((16, K), 15).cuda(), y2.view, y2.view, 16, [1.0])))   # ldy % 8 != 0
    g = guarded((16, K), K, F32, name="g")
    cases.append((g, lambda: ops.lora_wgrad(_normal((M, 256), 16).cuda(), x, [g.view] * 16, 16, 1.0)))            # R = 256
    g2 = guarded((12, K), K, F32, name="g")
    cases.append((g2, lambda: ops.lora_wgrad(tt, x, [g2.view, g2.view], 12, 1.0)))                                # r = 12
    for out, call in cases:
        with pytest.raises(L.DicowError):
            call()
        torch.cuda.synchronize()
        out.check()
        assert out.untouched_inside() == out.view.numel(), "a rejected call wrote to its output"

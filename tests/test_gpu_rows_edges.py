"""The FDDT + LayerNorm row kernels (csrc/fddt_ln.hip: thirteen bodies behind dicow_fddt_ln_fwd / _bwd) on ill-conditioned rows, eps
and mask edges, against the fp64 reference of tests/rows_ref.py with its condition-number bounds
(base + C 2^-24 kappa_row scale; C from the fp32 emulation of the same formulas, tests/test_host_rows_ref.py).  Every call first
asserts the body it runs on.  Inputs: offset rows (100 + randn, 1000 + 0.01 randn) mixed with randn rows in one trip, constant and
all-zero rows, an outlier channel, variance at or below eps with three eps values, 3e4 randn, one-hot / all-zero / doubled / strided
STNO masks; bf16 h_in, fp32 d_y, pos with B = 3, absent classes, BIAS mode, both y outputs, column sums accumulating onto non-zero
contents, outputs not asked for, repeated launches.  Measured errors: profiles/rows_conditioning.txt."""
import pytest
import torch

import amd_pkg
from tests import rows_ref as R
from tests.test_gpu_kernels import _ExpectRoute

pytestmark = pytest.mark.gpu

pkg = amd_pkg.load()

SMALL_ROWS = (1, 2, 3, 5, 7)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as _ops
    return _ops


MANY_ROWS = 2062        # (2064 with B = 3) many workgroups, not a multiple of 3 or 4; the staged bodies and every backward body loop


def loop_rows(cfg, D):
    """The smallest row count (even, 2 mod 4, no multiple of 3 -- a multiple of 3 with pos, B = 3) at which the workgroups of BOTH
    bodies of a configuration are certain to take a second trip, from the constants of csrc/fddt_ln.hip alone.
    Forward: the grid is capped at 256 CUs x the resident workgroups per CU.  Staged: 2 (measured count) x ROWS_R = 4 rows -> 2048.
    The other bodies ask the occupancy API, which 32 wave slots per CU bound from above whatever the register use: floor(32 / waves
    per workgroup) workgroups of ROWS_R = 4 rows (column owners, D / 256 waves rounded up), of LNW_R x LNW_WAVES = 16 rows (ln_wave),
    of FLW_R x FLW_WAVES = 8 rows (init_wave) -- e.g. 32768 rows at D = 256, 16384 for ln_wave, 8192 for init_wave.
    Backward: the column-owner grids are cut for ROWS_R = 4 rows per workgroup and visit BWD_RS = 3 / BWD_RG = 2 / BWD_R0 = 2 rows per
    trip, so they loop from 9 rows on; ln_wave (8 rows per workgroup, at most 4 workgroups per CU) from 8192 rows on."""
    fwd, bwd = R.routes(cfg, D)
    waves = -(-D // 256)
    n = (256 * 2 * 4 if fwd == "staged" else 256 * (32 // 8) * 16 if fwd == "ln_wave" else 256 * (32 // 8) * 8 if fwd == "init_wave" else
         256 * (32 // waves) * 4)
    if bwd == "ln_wave":
        n = max(n, 256 * (32 // 8) * 8)
    n += 14
    pos = bool(R.CONFIGS[cfg].get("pos"))
    while n % 4 != 2 or (n % 3 == 0) != pos:
        n += 2
    return n


def _cu(t):
    return None if t is None else t.cuda()


def _cpu(t):
    return None if t is None else t.cpu()


def _init(D, k):
    """Non-zero initial contents of a column-sum output (they accumulate)."""
    return (0.5 * torch.cos(torch.arange(D, dtype=torch.float64) * (0.37 + 0.11 * k))).float()


def run(ops, cfg, inp, *, g_out_bf16=True, sums=True):
    """Both entry points of one configuration on the GPU: {output: CPU tensor} in the layout of rows_ref's emulations, the column
    sums with their initial contents taken off (`raw`: as they are)."""
    D, rows, T, mode = inp["D"], inp["rows"], inp["T"], inp["mode"]
    opt = R.CONFIGS[cfg]
    ln = inp["ln_w"] is not None
    fwd_r, bwd_r = R.routes(cfg, D, g_out_bf16)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device="cuda")
    h, w, b = _cu(inp["h"]), [_cu(t) for t in inp["w"]], [_cu(t) for t in inp["b"]]
    kw = dict(mode=mode, w=w, b=b, pos=_cu(inp["pos"]), T=T if (mode != R.NONE or inp["pos"] is not None) else 0)
    if mode != R.NONE:
        kw.update(stno=_cu(inp["stno_buf"]), stno_bstride=inp["stno_bstride"])
    lw, lb = _cu(inp["ln_w"]), _cu(inp["ln_b"])
    # ---- forward
    ho = nan(rows, D) if mode != R.NONE else None
    yb, yf = (nan(rows, D, dtype=torch.bfloat16), nan(rows, D) if opt.get("y_f32") else None) if ln else (None, None)
    mean, rstd = (nan(rows), nan(rows)) if ln else (None, None)
    with _ExpectRoute(fwd_r):
        ops.fddt_ln_fwd(h, rows, D, h_out=ho, ln_w=lw, ln_b=lb, y_bf16=yb, y_f32=yf, mean=mean, rstd=rstd, eps=inp["eps"], **kw)
    got = dict(x=_cpu(ho), y=_cpu(yf), y_bf16=None if yb is None else yb.float().cpu(), mean=_cpu(mean), rstd=_cpu(rstd))
    # ---- backward, from the forward's statistics
    g0, g0b = nan(rows, D), (nan(rows, D, dtype=torch.bfloat16) if g_out_bf16 else None)
    init, acc = {}, {}
    if sums:
        names = ["colsum"] + (["dln_w", "dln_b"] if ln else [])
        names += [f"dw{c}" for c in range(4) if mode == R.DIAG and w[c] is not None]
        names += [f"db{c}" for c in range(4) if mode != R.NONE and b[c] is not None]
        for k, n in enumerate(names):
            init[n] = _init(D, k)
            acc[n] = init[n].cuda()
    with _ExpectRoute(bwd_r):
        ops.fddt_ln_bwd(h, rows, D, ln_w=lw, mean=mean, rstd=rstd, d_y=_cu(inp["d_y"]), g_res=_cu(inp["g_res"]), g_out=g0, g_out_bf16=g0b,
                        dln_w=acc.get("dln_w"), dln_b=acc.get("dln_b"), dw=[acc.get(f"dw{c}") for c in range(4)],
                        db=[acc.get(f"db{c}") for c in range(4)], colsum_out=acc.get("colsum"), **kw)
    torch.cuda.synchronize()
    got.update(g_out=g0.cpu(), g_out_bf16=None if g0b is None else g0b.float().cpu())
    raw = {n: t.cpu() for n, t in acc.items()}
    off = lambda n: None if n not in raw else raw[n].double() - init[n].double()
    got.update(colsum=off("colsum"), dln_w=off("dln_w"), dln_b=off("dln_b"), dw=[off(f"dw{c}") for c in range(4)],
               db=[off(f"db{c}") for c in range(4)], raw=raw, init=init)
    return got


def check(cfg, inp, got, worst=None):
    """h_out bit-equal to the header's evaluation order in fp32; every other output inside its bound."""
    ref = R.reference(inp)
    label = inp["name"]
    if got["x"] is not None:
        assert torch.equal(got["x"], R.fddt_fp32(inp)), (label, "h_out", float(R.abs_err(got["x"], ref["x"]).max()))
    cls = inp["x_kind"] + ("" if inp["mode"] == R.NONE or (inp["mask_kind"] == "soft" and inp["stno_bstride"] == 4 * inp["T"]) else
                           " mask=" + ("strided" if inp["stno_bstride"] != 4 * inp["T"] else inp["mask_kind"]))
    cls += "" if inp["eps"] == 1e-5 else f" eps={inp['eps']:g}"
    for name, (e, b, q) in R.worst_over_bound(inp, ref, got).items():
        k = (name.split("[")[0], cls)
        if worst is not None and q >= worst.get(k, (0.0, 0.0, -1.0, ""))[2]:
            worst[k] = (e, b, q, label)
        assert q < 1.0, (label, name, e, b)


def report(tag, worst):
    for (k, cls), (e, b, q, label) in worst.items():
        print(f"rows-edges | {tag} | {cls} | {k} | {q:.3f} | {e:.3e} | {b:.3e} | {label}")


def _variants(cfg, D):
    return (True, False) if R.routes(cfg, D, True) != R.routes(cfg, D, False) else (True,)       # staged_bf16 and staged_f32


CFG_D = [(cfg, D) for cfg in R.CONFIGS for D in R.widths(cfg)]


@pytest.mark.parametrize("cfg,D", CFG_D)
def test_small_row_counts_every_input_class(ops, cfg, D):
    """1, 2, 3, 5 and 7 rows (times B = 3 in the pos configuration) of every input class on every body: fewer rows than one trip,
    partial trips."""
    worst = {}
    mult = 3 if cfg == "pos" else 1
    for x in R.X_KINDS:
        for n in SMALL_ROWS:
            inp = R.case_inputs(cfg, D, x, n * mult)
            for bf in _variants(cfg, D):
                check(cfg, inp, run(ops, cfg, inp, g_out_bf16=bf), worst)
    report(f"{cfg} D={D} small", worst)


# every body at one width at least: ln_wave and init_wave at D = 512 (their counts at 1280 would be 21 M elements)
LOOP_CFG_D = ([("layer", D) for D in R.WIDTHS] + [("ln", D) for D in (256, 512, 516, 1536, 2048, 2304)] + [("init", 512)] +
              [(c, 1280) for c in R.CONFIGS if c not in ("layer", "ln", "init")])


@pytest.mark.parametrize("cfg,D", LOOP_CFG_D)
def test_workgroups_loop_over_trips(ops, cfg, D):
    """Past the capped grid of both bodies (loop_rows): ill-conditioned rows next to ordinary ones in every trip, the strides and
    clamped tails of the wave-per-row bodies, the staged bodies' prefetch, the column sums gathered over many partial rows."""
    worst = {}
    rows = loop_rows(cfg, D)
    for x in ("offset", "const"):
        inp = R.case_inputs(cfg, D, x, rows)
        for bf in (_variants(cfg, D) if cfg == "layer" else (True,)):
            check(cfg, inp, run(ops, cfg, inp, g_out_bf16=bf), worst)
    report(f"{cfg} D={D} rows={rows}", worst)


@pytest.mark.parametrize("eps", R.EPS[1:])
@pytest.mark.parametrize("cfg,D", [(c, d) for c, d in CFG_D if c in ("layer", "ln", "bias") and not (c == "bias" and d != 1280)])
def test_eps_is_the_one_passed(ops, cfg, D, eps):
    """Variance at or below eps (1e-3 randn, 3e-3 randn) with eps 1e-6 and 1e-3 passed explicitly (1e-5: the tests above)."""
    worst = {}
    for n in (3, 7):
        inp = R.case_inputs(cfg, D, "smallvar", n, eps=eps)
        for bf in _variants(cfg, D):
            check(cfg, inp, run(ops, cfg, inp, g_out_bf16=bf), worst)
    report(f"{cfg} D={D} eps={eps:g}", worst)


MASK_CFG_D = [("layer", 256), ("layer", 516), ("layer", 1280), ("layer", 2048), ("layer", 2304), ("bias", 1280), ("diag_absent", 1280),
              ("init", 1280), ("pos", 1280), ("dy_f32", 1280)]


@pytest.mark.parametrize("mask", R.MASK_KINDS[1:])
@pytest.mark.parametrize("cfg,D", MASK_CFG_D)
def test_stno_mask_edges(ops, cfg, D, mask):
    """One-hot 0/1 masks (class 2 never occurs: its gradients stay exactly what they were), all four zero (DIAG: x = 0, y = ln_b),
    two classes both 1, a strided mask tensor with NaN in the gap; offset rows, 9 / 8 rows and MANY_ROWS."""
    worst = {}
    for rows in (9 if cfg == "pos" else 8, MANY_ROWS + 2 * (cfg in ("pos", "init"))):
        inp = R.case_inputs(cfg, D, "offset", rows, mask=mask)
        if mask == "strided":
            assert inp["B"] >= 2 and inp["stno_bstride"] > 4 * inp["T"] and bool(torch.isnan(inp["stno_buf"]).any())
        for bf in _variants(cfg, D):
            got = run(ops, cfg, inp, g_out_bf16=bf)
            check(cfg, inp, got, worst)
            if mask == "onehot":
                for n in ("dw2", "db2"):
                    if n in got["raw"]:
                        assert torch.equal(got["raw"][n], got["init"][n]), (inp["name"], n)
            if mask == "zero" and inp["mode"] == R.DIAG:
                assert torch.equal(got["g_out"], torch.zeros_like(got["g_out"]))          # g0 = g * sum_c m_c w_c
                if inp["pos"] is None and got["y_bf16"] is not None:
                    assert torch.equal(got["x"], torch.zeros_like(got["x"]))
                    lb = inp["ln_b"].double()[None]
                    assert bool(((got["y_bf16"].double() - lb).abs() <= 2.0 ** -8 * lb.abs()).all()), inp["name"]
    report(f"{cfg} D={D} mask={mask}", worst)


@pytest.mark.parametrize("cfg,D", [("layer", 256), ("layer", 1280), ("layer", 516), ("layer", 2304), ("ln", 1280), ("ln", 1536),
                                   ("bias", 1280), ("init", 1280)])
def test_repeated_launches_and_outputs_not_asked_for(ops, cfg, D):
    """Two launches give the same bits.  A backward asked for no column sum, or for no bf16 copy, writes the same g_out, and the
    column sums do not depend on the bf16 copy being asked for."""
    inp = R.case_inputs(cfg, D, "offset", MANY_ROWS + 2 * (cfg in ("pos", "init")))
    a = run(ops, cfg, inp)
    check(cfg, inp, a)
    b = run(ops, cfg, inp)
    for k in ("x", "y", "y_bf16", "mean", "rstd", "g_out", "g_out_bf16"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), (inp["name"], k)
    for n in a["raw"]:
        assert torch.equal(a["raw"][n], b["raw"][n]), (inp["name"], n)
    c = run(ops, cfg, inp, sums=False)
    assert torch.equal(c["g_out"], a["g_out"]) and torch.equal(c["g_out_bf16"], a["g_out_bf16"]) and not c["raw"]
    d = run(ops, cfg, inp, g_out_bf16=False)
    assert d["g_out_bf16"] is None and torch.equal(d["g_out"], a["g_out"])
    for n in a["raw"]:
        assert torch.equal(a["raw"][n], d["raw"][n]), (inp["name"], n)


@pytest.mark.parametrize("cfg,D", [("ln", 1280), ("ln", 1536), ("ln", 2304), ("bias", 1280), ("y_both", 1280)])
def test_forward_outputs_not_asked_for(ops, cfg, D):
    """A forward asked for the fp32 y alone -- no bf16 y, no mean, no rstd, no h_out -- runs the same body and writes the same y."""
    inp = R.case_inputs(cfg, D, "offset", MANY_ROWS)
    full = run(ops, cfg, inp)
    rows, mode = inp["rows"], inp["mode"]
    kw = dict(mode=mode, w=[_cu(t) for t in inp["w"]], b=[_cu(t) for t in inp["b"]], T=inp["T"] if mode != R.NONE else 0)
    if mode != R.NONE:
        kw.update(stno=_cu(inp["stno_buf"]), stno_bstride=inp["stno_bstride"])
    yf = torch.full((rows, D), float("nan"), device="cuda")
    with _ExpectRoute(R.routes(cfg, D)[0]):
        ops.fddt_ln_fwd(_cu(inp["h"]), rows, D, ln_w=_cu(inp["ln_w"]), ln_b=_cu(inp["ln_b"]), y_f32=yf, eps=inp["eps"], **kw)
    assert torch.equal(yf.cpu(), full["y"]), inp["name"]

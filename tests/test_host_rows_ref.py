"""tests/rows_ref.py pinned on the CPU: the fp64 reference of the FDDT + LayerNorm row kernels against torch's layer_norm, the
oracle's FDDT and golden F3; the bounds against the fp32 emulations of the same formulas -- the right form inside every bound on
every case, every wrong form a rewrite of a kernel could fall into at least 10 x outside one on a named case.  The negative controls
are what makes tests/test_gpu_rows_edges.py meaningful: a kernel that passes there is none of these forms."""
import pytest
import torch

from oracle import dicow_oracle as O
from tests import rows_ref as R
from tests.util import load_golden, T

CLS = ["silence_linear", "target_linear", "non_target_linear", "overlap_linear"]
FLAGS = ["fddt_use_silence", "fddt_use_target", "fddt_use_non_target", "fddt_use_overlap"]


@pytest.fixture(scope="module")
def table():
    """Every host case once: (label, input class, inp, reference)."""
    return [(label, cls, inp, R.reference(inp)) for label, cls, inp in R.host_cases()]


def test_reference_equals_layer_norm_and_oracle_fddt(table):
    """x against oracle.dicow_oracle.fddt (+ pos) and y against torch.nn.functional.layer_norm, both in fp64, on the case table."""
    worst = 0.0
    for label, _, inp, ref in table:
        h = inp["h"].double().view(inp["B"], inp["T"], inp["D"])
        x = h
        if inp["mode"] != R.NONE:
            cfg = O.OracleConfig(d_model=inp["D"], fddt_bias_only=inp["mode"] == R.BIAS,
                                 **{FLAGS[c]: inp["b"][c] is not None for c in range(4)})
            p = {}
            for c in range(4):
                if inp["mode"] == R.BIAS and inp["b"][c] is not None:
                    p[CLS[c]] = inp["b"][c].double()
                elif inp["w"][c] is not None:
                    p[CLS[c] + ".weight"], p[CLS[c] + ".bias"] = inp["w"][c].double(), inp["b"][c].double()
            x = O.fddt(h, inp["stno"].double(), p, "", cfg)
        if inp["pos"] is not None:
            x = x + inp["pos"].double()[None]
        x = x.reshape(inp["rows"], inp["D"])
        sc = max(1.0, float(ref["a_max"].max()))
        assert float((x - ref["x"]).abs().max()) <= 1e-15 * sc, label
        if inp["ln_w"] is not None:
            y = torch.nn.functional.layer_norm(ref["x"], (inp["D"],), inp["ln_w"].double(), inp["ln_b"].double(), inp["eps"])
            e = float(((y - ref["y"]).abs() / (1 + ref["kappa"][:, None])).max())
            worst = max(worst, e)
            assert e < 1e-13, (label, e)
    print(f"fp64 reference vs layer_norm: worst |dy| / (1 + kappa) {worst:.2e}")


@pytest.mark.parametrize("vn", ["diag", "diag_no_sil_ovl", "bias"])
def test_reference_equals_golden_f3(vn):
    z = load_golden("f3_fddt")
    h, st, go = T(z, vn + ".h"), T(z, vn + ".stno"), T(z, vn + ".gout")
    B, Tn, D = h.shape
    inp = dict(name=vn, D=D, B=B, T=Tn, rows=B * Tn, mode=R.BIAS if vn == "bias" else R.DIAG, eps=1e-5, pos=None, ln_w=None,
               ln_b=None, d_y=None, stno=st, stno_buf=st, h=h.reshape(B * Tn, D), g_res=go.reshape(B * Tn, D))
    w, b = [], []
    for c in CLS:
        if vn == "bias":
            w.append(None)
            b.append(T(z, f"{vn}.p.{c}") if f"{vn}.p.{c}" in z.files else None)
        else:
            kw = f"{vn}.p.{c}.weight"
            w.append(T(z, kw) if kw in z.files else None)
            b.append(T(z, f"{vn}.p.{c}.bias") if kw in z.files else None)
    inp["w"], inp["b"] = w, b
    assert any(t is None for t in b) == (vn == "diag_no_sil_ovl")
    ref = R.reference(inp)
    md = lambda a, r: float((a.double() - r.double().reshape(a.shape)).abs().max())
    assert md(ref["x"], T(z, vn + ".out")) < 2e-6               # (the golden is fp32)
    assert md(ref["g_out"], T(z, vn + ".gh")) < 2e-6
    for i, c in enumerate(CLS):
        if vn == "bias":
            if b[i] is not None:
                g = T(z, f"{vn}.g.{c}")
                assert md(ref["db"][i], g) < 2e-5 * max(1.0, float(g.abs().max()))
        elif w[i] is not None:
            gw, gb = T(z, f"{vn}.g.{c}.weight"), T(z, f"{vn}.g.{c}.bias")
            assert md(ref["dw"][i], gw) < 2e-5 * max(1.0, float(gw.abs().max()))
            assert md(ref["db"][i], gb) < 2e-5 * max(1.0, float(gb.abs().max()))
    # the fp32 emulation evaluates the header's order: bit-equal to the fp32 golden
    assert torch.equal(R.emulate_fwd(inp)["x"], T(z, vn + ".out").reshape(B * Tn, D))


def test_right_form_is_inside_every_bound(table):
    """The right-form emulation -- forward, backward with the forward's x, backward with the collapsed x -- on every case."""
    worst = {}
    for label, _, inp, ref in table:
        for got in R.right_form(inp, ref):
            for name, (e, b, q) in R.worst_over_bound(inp, ref, got).items():
                k = name.split("[")[0]
                if q > worst.get(k, (0, 0, 0, ""))[2]:
                    worst[k] = (e, b, q, label)
                assert q < 1.0, (label, name, e, b)
    for k, (e, b, q, label) in worst.items():
        print(f"right form {k:10s}: worst error / bound {q:.3f} ({e:.3e} / {b:.3e}) at {label}")


def test_constants_are_four_times_the_emulation():
    """C is 4 x the right-form emulation's worst ratio, rounded up to an integer.  The emulation sums in a fixed tree order, so only
    the CPU's rsqrt / division could move the re-measured ratio: it has to sit between C / 5 and C / 3.5."""
    tb = R.measure()
    for k, c in R.C.items():
        q = tb["all"][k]
        print(f"C[{k}] = {c:g}: measured ratio {q:.2f} (4 x = {4 * q:.1f})")
        assert c / 5 <= q <= c / 3.5, (k, q, c)


def _wrong(inp, ref, form):
    """The results of a wrong form: a forward form's y / mean / rstd and the right backward from ITS statistics; a backward form
    from the right statistics."""
    if form in R.FWD_FORMS:
        f = R.emulate_fwd(inp, form)
        return [f, R.emulate_bwd(inp, f["mean"], f["rstd"])]
    f = R.emulate_fwd(inp, dense=form == "mask_dense_stride")
    return [f, R.emulate_bwd(inp, f.get("mean"), f.get("rstd"), form)]


# wrong form -> the cases that reject it: (configuration, input class, mask kind, eps), at every width of the configuration
REJECTED_BY = {
    "one_pass": ("ln", "offset", "soft", 1e-5),                  # rows 100 + randn and 1000 + 0.01 randn
    "no_eps": ("ln", "smallvar", "soft", 1e-5),                  # variance below eps
    "eps_outside": ("ln", "smallvar", "soft", 1e-5),
    "eps_fixed": ("ln", "smallvar", "soft", 1e-3),               # an eps other than the default
    "no_xhat_term": ("layer", "randn", "soft", 1e-5),
    "pos_row_div_T": ("pos", "randn", "soft", 1e-5),             # B = 3, T = 3
    "mask_dense_stride": ("layer", "offset", "strided", 1e-5),   # stno_bstride = 4 T + 24, NaN in the gap
}


@pytest.mark.parametrize("form", R.WRONG_FORMS)
def test_wrong_forms_are_rejected_at_ten_times_the_bound(form):
    cfg, x, mask, eps = REJECTED_BY[form]
    for D in R.widths(cfg):
        inp = R.case_inputs(cfg, D, x, 9 if cfg == "pos" else 8, mask=mask, eps=eps)
        ref = R.reference(inp)
        best = ("", 0.0)
        for got in _wrong(inp, ref, form):
            for name, (e, b, q) in R.worst_over_bound(inp, ref, got).items():
                if q > best[1]:
                    best = (name, q)
        print(f"wrong form {form:18s} on {cfg} D={D} {x} mask={mask} eps={eps:g}: {best[0]} at {best[1]:.3g} x its bound")
        assert best[1] >= 10.0, (form, D, best)


def test_staged_forward_outputs_reject_the_forward_forms():
    """The staged forward has no fp32 y: its wrong forms have to show in rstd, mean and the bf16 y alone."""
    for form, (_, x, mask, eps) in REJECTED_BY.items():
        if form not in R.FWD_FORMS:
            continue
        for D in (256, 1280, 1536, 2048):
            inp = R.case_inputs("layer", D, x, 8, eps=eps)
            ref = R.reference(inp)
            f = R.emulate_fwd(inp, form)
            got = dict(y_bf16=f["y"].bfloat16().float(), mean=f["mean"], rstd=f["rstd"])
            q = max(v[2] for v in R.worst_over_bound(inp, ref, got).values())
            print(f"wrong form {form:12s} on layer D={D} {x} eps={eps:g}: {q:.3g} x the bound of y_bf16 / mean / rstd")
            assert q >= 10.0, (form, D, q)


def test_case_table_names_every_body():
    fwd, bwd = set(), set()
    for cfg in R.CONFIGS:
        for D in R.widths(cfg):
            for bf in (True, False):
                f, b = R.routes(cfg, D, bf)
                fwd.add(f)
                bwd.add(b)
    assert fwd == {"staged", "init_wave", "ln_wave", "generic_ln", "generic_diag", "generic", "generic_1024"}
    assert bwd == {"ln_wave", "staged_bf16", "staged_f32", "ln_only", "generic", "generic_1024"}

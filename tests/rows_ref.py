"""Reference side of the FDDT + LayerNorm row-kernel edge tests (tests/test_host_rows_ref.py, tests/test_gpu_rows_edges.py): plain
torch on the CPU, nothing from the library.

  reference(inp)          both entry points in fp64 from the formulas of include/dicow_hip.h (FDDT modes NONE / DIAG / BIAS, absent
                          classes, pos with row % T, LayerNorm with an explicit eps), the backward by autograd through that graph.
                          The inputs are taken as they reach the kernel: already rounded to fp32 or bf16.
  emulate(inp, ...)       the same formulas in fp32, in the RIGHT form (mean = fp32 sum * fp32 1/D, centred squares, rsqrt(var + eps),
                          x-hat = (x - mean) * rstd, g = rstd * (dy g - mean(dy g) - x-hat mean(dy g x-hat))) with the forward's x or
                          the collapsed one of the backward bodies, and in the WRONG forms a rewrite of a kernel could fall into.
  bounds(inp, ref)        one bound per output, base + C * 2^-24 * kappa_row * scale.

kappa_row = max|x_row| / sqrt(var_row + eps) on the post-FDDT row is what fp32 LayerNorm loses: x - mean carries ulp(x), x-hat the
same over sigma.  Where x is a sum -- FDDT terms, biases, pos -- its ulp is that of the terms, so |x| is taken as the sum of their
absolute values, sum_c m_c (|h w_c| + |b_c|) + |pos| (equal to |x| in mode NONE, and within rounding of it wherever the terms do not
cancel: a small-variance row that leaves a BIAS-mode FDDT as the difference of h and biases of 0.1 is known to no more than
ulp(0.1); there kappa is about 100 x the one of the final x).  The mean bound, 4 * 2^-24 |x_row|, takes the same |x|.  Every bound
uses max(kappa_row, 1): the outputs' own last rounding is 2^-24 * scale also where x-hat is 0 (an all-zero row has kappa 0 and still
rstd = eps^-1/2, g = rstd * (dy g - mean(dy g))).

Scales (the output's natural size):
  y           max|ln_w|
  g_out       gain_row * G_row,  G_row = rstd_row * max|dy g|_row + max|g_res|_row (the LayerNorm part of g plus the residual gradient
              added to it), gain_row = max|sum_c m_c w_c|_row in DIAG mode (g0 = g * that), 1 otherwise
  colsum_out  gain_row * G_row            db[c]  m_c,row * G_row            dw[c]  m_c,row * max|h_row| * G_row
  dln_w       max|d_y|_row                dln_b  max|d_y|_row with kappa 1 (no x-hat in it)
the column sums in quadrature over the rows, their base times sqrt(rows) like tests/test_gpu_kernels.py does.  base: ROW_BOUNDS of
tests/test_gpu_kernels.py (imported) -- h_out for the fp32 y (the fp32 forward row entry; y has none of its own), g_out, ln_sums,
fddt_sums.  A bf16 output has the bound of its fp32 twin plus 2^-8 |ref| elementwise (round-to-nearest's half ulp, reached just
above a power of two); the absolute ROW_BOUNDS["bf16"] (5e-2) is not used: it would hide every wrong form on rows of ordinary size.

C: per output, 4 x the worst error / (2^-24 kappa scale) of the right-form emulation (forward's x and collapsed x) against fp64 over
the whole case table -- the kernels' summation orders (DPP tree, per-wave partials) differ from the emulation's binary tree, each
within a small factor of the other.  Measured on the CPU, never fitted to a kernel: profiles/rows_conditioning.txt has the ratios per
input class."""
import zlib

import torch

from tests.test_gpu_kernels import ROW_BOUNDS

F32, F64 = torch.float32, torch.float64
NONE, DIAG, BIAS = 0, 1, 2
U = 2.0 ** -24

# 4 x the measured right-form ratios (tests/test_host_rows_ref.py::test_constants_are_four_times_the_emulation re-measures them)
C = dict(y=17.0, g_out=12.0, colsum=9.0, dln_w=11.0, dln_b=7.0, dw=9.0, db=9.0)

FWD_FORMS = ("right", "one_pass", "no_eps", "eps_outside", "eps_fixed")
WRONG_FORMS = ("one_pass", "no_eps", "eps_outside", "eps_fixed", "no_xhat_term", "pos_row_div_T", "mask_dense_stride")


# ------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def rows_x(kind, rows, D, g):
    """Post-FDDT rows of one input class, fp64 [rows, D].  Ill-conditioned rows alternate with ordinary randn rows, so that a
    statistic leaking between the rows of one trip shows."""
    r = torch.randn(rows, D, generator=g, dtype=F64)
    i = torch.arange(rows)[:, None]
    if kind == "randn":
        return r
    if kind == "offset":            # 100 + randn | randn | 1000 + 0.01 randn | randn
        return torch.where(i % 4 == 0, 100 + r, torch.where(i % 4 == 2, 1000 + 0.01 * r, r))
    if kind == "const":             # every column 1000.1 | randn | all zero | randn
        return torch.where(i % 4 == 0, torch.full_like(r, 1000.1), torch.where(i % 4 == 2, torch.zeros_like(r), r))
    if kind == "outlier":           # column 7 at +300, column D - 1 at -300
        r[:, 7], r[:, D - 1] = 300.0, -300.0
        return r
    if kind == "smallvar":          # 1e-3 randn | 3e-3 randn | randn: variance at or below eps
        return torch.where(i % 3 == 0, 1e-3 * r, torch.where(i % 3 == 1, 3e-3 * r, r))
    if kind == "large":
        return 3e4 * r
    raise ValueError(kind)


def masks(kind, B, T, g, gap=0):
    """[B, 4, T] fp32 STNO masks; gap > 0: a strided view (stno_bstride = 4 T + gap) of a buffer with NaN between the batches.
    Returns (view, buffer)."""
    if kind == "soft":
        m = torch.softmax(torch.randn(B, 4, T, generator=g), 1)
    elif kind == "onehot":          # class 2 never occurs: its gradients must be exactly 0
        cls = torch.randint(0, 3, (B, T), generator=g)
        cls = torch.where(cls == 2, torch.full_like(cls, 3), cls)
        m = torch.nn.functional.one_hot(cls, 4).permute(0, 2, 1).float()
    elif kind == "zero":
        m = torch.zeros(B, 4, T)
    elif kind == "two":             # two classes both 1
        m = torch.zeros(B, 4, T)
        m[:, 1], m[:, 3] = 1.0, 1.0
    else:
        raise ValueError(kind)
    buf = torch.full((B, 4 * T + gap), float("nan"))
    buf[:, :4 * T] = m.reshape(B, 4 * T)
    return buf[:, :4 * T].view(B, 4, T), buf


def make_inputs(name, D, B, T, *, mode=DIAG, x="randn", mask="soft", absent=(), pos=False, in_bf16=False, dy_f32=False, eps=1e-5,
                ln=True, gap=0):
    """The tensors of one case as they reach the kernel (CPU, fp32 / bf16).  h is built so that the post-FDDT row comes out as the
    class `x` describes (up to the rounding of h itself): h = (x - pos - sum_c m_c b_c) / sum_c m_c w_c."""
    g = _gen(name)
    rows = B * T
    rnd = lambda *s: torch.randn(*s, generator=g)
    inp = dict(name=name, D=D, B=B, T=T, rows=rows, mode=mode, eps=eps, x_kind=x, mask_kind=mask)
    w = [None if (c in absent or mode != DIAG) else 1 + 0.1 * rnd(D) for c in range(4)]
    b = [None if (c in absent or mode == NONE) else 0.1 * rnd(D) for c in range(4)]
    inp["w"], inp["b"] = w, b
    inp["pos"] = rnd(T, D) if pos else None
    if mode != NONE:
        inp["stno"], inp["stno_buf"] = masks(mask, B, T, g, gap)
        inp["stno_bstride"] = 4 * T + gap
    xt = rows_x(x, rows, D, g)
    if inp["pos"] is not None:
        xt = xt - inp["pos"].double().repeat(B, 1)
    if mode != NONE:
        m = inp["stno"].double().permute(0, 2, 1).reshape(rows, 4)
        one, zero = torch.ones(D, dtype=F64), torch.zeros(D, dtype=F64)
        sb = sum(m[:, c, None] * (zero if b[c] is None else b[c].double()) for c in range(4))
        if mode == DIAG:
            sw = sum(m[:, c, None] * (one if w[c] is None else w[c].double()) for c in range(4))
            xt = torch.where(sw.abs() > 0.25, (xt - sb) / sw.clamp_min(0.25), xt)       # (all-zero masks: x is 0 whatever h is)
        else:
            xt = xt - sb
    inp["h"] = xt.float().bfloat16() if in_bf16 else xt.float()
    if ln:
        inp["ln_w"], inp["ln_b"] = 1 + 0.1 * rnd(D), 0.1 * rnd(D)
        inp["d_y"] = rnd(rows, D) if dy_f32 else rnd(rows, D).bfloat16()
    else:
        inp["ln_w"] = inp["ln_b"] = inp["d_y"] = None
    inp["g_res"] = rnd(rows, D)
    return inp


# ------------------------------------------------------------------------------------------------ the formulas, any dtype
def _row_masks(inp, dt, dense=False):
    """[rows, 4]: the four class masks of every row.  dense: the WRONG read that ignores stno_bstride (channel c of batch bi taken
    at bi * 4 T + c T + t of the buffer)."""
    B, T = inp["B"], inp["T"]
    m = inp["stno_buf"].reshape(-1)[:B * 4 * T].view(B, 4, T) if dense else inp["stno"]
    return m.to(dt).permute(0, 2, 1).reshape(B * T, 4)


def _pos_rows(inp, dt, div=False):
    r = torch.arange(inp["rows"])
    return inp["pos"].to(dt)[(r // inp["T"]) if div else (r % inp["T"])]


def fddt(h, inp, w, b, *, collapsed=False, dense=False, pos_div=False):
    """x = FDDT(h) + pos in the dtype of h.  Default: the evaluation order of the header, ((t0 + t1) + t2) + t3 with
    t_c = (h w_c + b_c) m_c, an absent class t_c = h m_c; collapsed: h * sum_c m_c w_c + sum_c m_c b_c as the backward bodies
    recompute it.  Returns (x, sw, a) with sw = sum_c m_c w_c ([rows, D]; None outside DIAG mode) and a = the sum of the absolute
    values of the terms x is added up from (|x| itself in mode NONE without pos)."""
    dt, mode, sw = h.dtype, inp["mode"], None
    x, a = h, h.abs()
    if mode != NONE:
        m = _row_masks(inp, dt, dense)
        one, zero = torch.ones(inp["D"], dtype=dt), torch.zeros(inp["D"], dtype=dt)
    if mode == DIAG:
        sw, sb = torch.zeros_like(h), torch.zeros_like(h)
        for c in range(4):
            sw = sw + m[:, c, None] * (one if w[c] is None else w[c])
            sb = sb + m[:, c, None] * (zero if b[c] is None else b[c])
        if collapsed:
            x = h * sw + sb
        else:
            t = [(h if w[c] is None else h * w[c] + b[c]) * m[:, c, None] for c in range(4)]
            x = ((t[0] + t[1]) + t[2]) + t[3]
        a = sum(((h.abs() if w[c] is None else (h * w[c]).abs() + b[c].abs()) * m[:, c, None].abs()) for c in range(4))
    elif mode == BIAS:
        for c in range(4):
            if b[c] is not None:
                x = x + m[:, c, None] * b[c]
                a = a + (m[:, c, None] * b[c]).abs()
    if inp["pos"] is not None:
        p = _pos_rows(inp, dt, pos_div)
        x, a = x + p, a + p.abs()
    return x, sw, a


def _cast(inp, dt):
    c = lambda t: None if t is None else t.to(dt)
    return c(inp["h"]), [c(t) for t in inp["w"]], [c(t) for t in inp["b"]], c(inp["ln_w"]), c(inp["ln_b"]), c(inp["d_y"]), c(inp["g_res"])


# ------------------------------------------------------------------------------------------------ fp64 reference
def reference(inp):
    """fp64: x, and with LayerNorm mean / var / rstd / kappa / y; backward by autograd: g_out (the gradient of h), dln_w, dln_b,
    dw[4], db[4] (None for absent classes), colsum (the column sums of g_out), plus the per-row quantities the bounds need."""
    h, w, b, lw, lb, dy, gr = _cast(inp, F64)
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    h, w, b, lw, lb = leaf(h), [leaf(t) for t in w], [leaf(t) for t in b], leaf(lw), leaf(lb)
    x, sw, a = fddt(h, inp, w, b)
    ref = dict(x=x.detach(), a_max=a.detach().amax(-1))
    loss = (x * gr).sum()
    eps = inp["eps"]
    if lw is not None:
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        y = (x - mu) * rstd * lw + lb
        loss = loss + (y * dy).sum()
        ref.update(mean=mu.detach()[:, 0], var=var.detach()[:, 0], rstd=rstd.detach()[:, 0], y=y.detach(),
                   kappa=(ref["a_max"] / torch.sqrt(var.detach()[:, 0] + eps)))
    loss.backward()
    ref["g_out"] = h.grad
    ref["colsum"] = h.grad.sum(0)
    ref["dln_w"], ref["dln_b"] = (lw.grad, lb.grad) if lw is not None else (None, None)
    ref["dw"] = [None if t is None else t.grad for t in w]
    ref["db"] = [None if t is None else t.grad for t in b]
    # per-row sizes
    rows = inp["rows"]
    ref["kappa_e"] = ref["kappa"].clamp_min(1.0) if lw is not None else torch.ones(rows, dtype=F64)
    G = gr.abs().amax(-1)
    if lw is not None:
        G = G + ref["rstd"] * (dy * lw.detach()).abs().amax(-1)
        ref["dy_max"] = dy.abs().amax(-1)
    ref["G"] = G
    ref["gain"] = sw.detach().abs().amax(-1) if sw is not None else torch.ones(rows, dtype=F64)
    ref["h_max"] = h.detach().abs().amax(-1)
    ref["m"] = _row_masks(inp, F64) if inp["mode"] != NONE else None
    return ref


# ------------------------------------------------------------------------------------------------ fp32 emulations
def tree_sum(v, dim):
    """Sum along `dim` as a balanced binary tree of IEEE additions in the dtype of v (zero-padded to a power of two).  Unlike
    torch.sum its order does not depend on the CPU's vector width, so the emulations are bit-reproducible anywhere; like the
    kernels' DPP and partial-row trees its depth is log2 n."""
    v = v.movedim(dim, -1)
    n = 1 << max(v.shape[-1] - 1, 0).bit_length()
    if n != v.shape[-1]:
        v = torch.cat([v, v.new_zeros(*v.shape[:-1], n - v.shape[-1])], -1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _rsum(v):
    return tree_sum(v, -1)[:, None]


def fddt_fp32(inp):
    """x alone in fp32, in the header's evaluation order: what h_out has to equal bit for bit."""
    h, w, b = _cast(inp, F32)[:3]
    return fddt(h, inp, w, b)[0]


def emulate_fwd(inp, form="right", dense=False):
    """fp32: x (reference evaluation order), mean, rstd, y in the given form."""
    h, w, b, lw, lb, _, _ = _cast(inp, F32)
    x = fddt(h, inp, w, b, dense=dense)[0]
    out = dict(x=x)
    if lw is None:
        return out
    inv_d = torch.tensor(1.0, dtype=F32) / torch.tensor(float(inp["D"]), dtype=F32)
    eps = torch.tensor(1e-5 if form == "eps_fixed" else inp["eps"], dtype=F32)
    mu = _rsum(x) * inv_d
    if form == "one_pass":
        var = (_rsum(x * x) * inv_d - mu * mu).clamp_min(0.0)
    else:
        d = x - mu
        var = _rsum(d * d) * inv_d
    if form == "no_eps":
        rstd = torch.rsqrt(var)
    elif form == "eps_outside":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = torch.rsqrt(var + eps)
    out.update(mean=mu[:, 0], rstd=rstd[:, 0], y=(x - mu) * rstd * lw + lb)
    return out


def emulate_bwd(inp, mean, rstd, form="right", collapsed=False):
    """fp32 backward from saved statistics (fp32 [rows]): g_out, colsum, dln_w, dln_b, dw, db.  collapsed: x recomputed as the
    backward bodies do.  Wrong forms: no_xhat_term, pos_row_div_T, mask_dense_stride."""
    h, w, b, lw, _, dy, gr = _cast(inp, F32)
    dense = form == "mask_dense_stride"
    x, sw, _ = fddt(h, inp, w, b, collapsed=collapsed, dense=dense, pos_div=form == "pos_row_div_T")
    g = gr
    out = dict(dln_w=None, dln_b=None)
    if lw is not None:
        inv_d = torch.tensor(1.0, dtype=F32) / torch.tensor(float(inp["D"]), dtype=F32)
        mu, rs = mean.to(F32)[:, None], rstd.to(F32)[:, None]
        xh = (x - mu) * rs
        dxh = dy * lw
        c1 = _rsum(dxh) * inv_d
        c2 = _rsum(dxh * xh) * inv_d
        g = g + rs * ((dxh - c1) if form == "no_xhat_term" else (dxh - c1 - xh * c2))
        out["dln_w"], out["dln_b"] = tree_sum(dy * xh, 0), tree_sum(dy, 0)
    m = _row_masks(inp, F32, dense) if inp["mode"] != NONE else None
    out["dw"] = [None if t is None else tree_sum(m[:, c, None] * g * h, 0) for c, t in enumerate(w)]
    out["db"] = [None if t is None else tree_sum(m[:, c, None] * g, 0) for c, t in enumerate(b)]
    g0 = g * sw if inp["mode"] == DIAG else g
    out["g_out"], out["colsum"] = g0, tree_sum(g0, 0)
    return out


# ------------------------------------------------------------------------------------------------ bounds
def _quad(v):
    return float(torch.sqrt((v.double() ** 2).sum()))


def terms(inp, ref):
    """{output: 2^-24 * kappa * scale}: [rows, 1] for the row outputs, a float (rows in quadrature) for the column sums."""
    k, G, gain = ref["kappa_e"], ref["G"], ref["gain"]
    t = {}
    if inp["ln_w"] is not None:
        lwmax = float(inp["ln_w"].abs().max())
        t["y"] = (U * k * lwmax)[:, None]
        t["rstd"] = U * k
        t["dln_w"] = U * _quad(k * ref["dy_max"])
        t["dln_b"] = U * _quad(ref["dy_max"])
    t["g_out"] = (U * k * gain * G)[:, None]
    t["colsum"] = U * _quad(k * gain * G)
    m = ref["m"]
    t["dw"] = [None if w is None else U * _quad(k * m[:, c] * ref["h_max"] * G) for c, w in enumerate(inp["w"])]
    t["db"] = [None if b is None else U * _quad(k * m[:, c] * G) for c, b in enumerate(inp["b"])]
    return t


def bounds(inp, ref):
    """{output: bound}; broadcastable against the output.  y_bf16 / g_out_bf16: the fp32 bound plus 2^-8 |ref| elementwise."""
    c, t, sq = C, terms(inp, ref), inp["rows"] ** 0.5
    bd = {}
    if inp["ln_w"] is not None:
        bd["y"] = ROW_BOUNDS["h_out"] + c["y"] * t["y"]
        bd["y_bf16"] = bd["y"] + 2.0 ** -8 * ref["y"].abs()
        bd["mean"] = 4 * U * ref["a_max"]
        bd["rstd"] = c["y"] * t["rstd"]                      # on rstd * sqrt(var + eps) - 1
        bd["dln_w"] = ROW_BOUNDS["ln_sums"] * sq + c["dln_w"] * t["dln_w"]
        bd["dln_b"] = ROW_BOUNDS["ln_sums"] * sq + c["dln_b"] * t["dln_b"]
    bd["g_out"] = ROW_BOUNDS["g_out"] + c["g_out"] * t["g_out"]
    bd["g_out_bf16"] = bd["g_out"] + 2.0 ** -8 * ref["g_out"].abs()
    bd["colsum"] = ROW_BOUNDS["fddt_sums"] * sq + c["colsum"] * t["colsum"]
    bd["dw"] = [None if v is None else ROW_BOUNDS["fddt_sums"] * sq + c["dw"] * v for v in t["dw"]]
    bd["db"] = [None if v is None else ROW_BOUNDS["fddt_sums"] * sq + c["db"] * v for v in t["db"]]
    return bd


def abs_err(got, ref):
    """|got - ref| in fp64, a NaN or Inf of `got` counted as an infinite error."""
    e = (got.double() - ref.double()).abs()
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def outputs(got, ref):
    """Pairs (name, C key, got, ref) of every output present in `got` (an emulation's or a kernel's result dict)."""
    out = []
    for k in ("y", "g_out", "colsum", "dln_w", "dln_b"):
        if got.get(k) is not None and ref.get(k) is not None:
            out.append((k, k, got[k], ref[k]))
    for k in ("dw", "db"):
        for c in range(4):
            if got.get(k) is not None and got[k][c] is not None and ref[k][c] is not None:
                out.append((f"{k}[{c}]", k, got[k][c], ref[k][c]))
    return out


def _pick(d, name):
    return d[name[:2]][int(name[3])] if name[:3] in ("dw[", "db[") else d[name]


def ratios(inp, ref, got):
    """{C key: worst error / (2^-24 kappa scale)} of a result dict against the reference (an entry whose scale is 0 -- all-zero masks
    in DIAG mode, where g_out is exactly 0 -- is skipped: its bound is the base alone)."""
    t, out = terms(inp, ref), {}
    for name, key, g, r in outputs(got, ref):
        e, tt = abs_err(g, r), _pick(t, name)
        if torch.is_tensor(tt):
            ok = (tt > 0).expand_as(e)
            q = float((e[ok] / tt.expand_as(e)[ok]).max()) if bool(ok.any()) else 0.0
        else:
            q = float(e.max()) / tt if tt > 0 else 0.0
        out[key] = max(out.get(key, 0.0), q)
    return out


def worst_over_bound(inp, ref, got):
    """{output name: (worst error, its bound, error / bound)} of a result dict: y, g_out and the column sums, their bf16 copies
    (y_bf16, g_out_bf16), mean, and rstd as rstd * sqrt(var + eps) against 1."""
    bd, out = bounds(inp, ref), {}
    todo = [(name, abs_err(g, r), _pick(bd, name)) for name, _, g, r in outputs(got, ref)]
    for k in ("y", "g_out"):
        if got.get(k + "_bf16") is not None:
            todo.append((k + "_bf16", abs_err(got[k + "_bf16"], ref[k]), bd[k + "_bf16"]))
    if got.get("mean") is not None:
        todo.append(("mean", abs_err(got["mean"], ref["mean"]), bd["mean"]))
    if got.get("rstd") is not None:
        todo.append(("rstd", abs_err(got["rstd"].double() * torch.sqrt(ref["var"] + inp["eps"]), torch.ones_like(ref["var"])), bd["rstd"]))
    for name, e, b in todo:
        b = b.expand_as(e) if torch.is_tensor(b) else torch.full_like(e, b)
        q = torch.where(e == 0, torch.zeros_like(e), e / b)
        i = int(q.argmax())
        out[name] = (float(e.reshape(-1)[i]), float(b.reshape(-1)[i]), float(q.reshape(-1)[i]))
    return out


# ------------------------------------------------------------------------------------------------ the case table
# one wave | inactive lanes, D % 8 != 0 | staged and wave-per-row | staged | the widest staged | 1024 threads
WIDTHS = (256, 516, 1280, 1536, 2048, 2304)
X_KINDS = ("randn", "offset", "const", "outlier", "smallvar", "large")
MASK_KINDS = ("soft", "onehot", "zero", "two", "strided")
EPS = (1e-5, 1e-6, 1e-3)

# what a configuration asks of the two entry points (make_inputs arguments; y_f32: the forward is asked for the fp32 y as well)
CONFIGS = {
    "layer": dict(mode=DIAG),                                    # an encoder layer's FDDT + LayerNorm: h_out, y_bf16, mean, rstd
    "ln": dict(mode=NONE, y_f32=True),                           # LayerNorm only, y_f32 and y_bf16 together
    "bias": dict(mode=BIAS, y_f32=True),                         # BIAS mode with LayerNorm
    "bias_absent": dict(mode=BIAS, absent=(0,), y_f32=True),
    "diag_absent": dict(mode=DIAG, absent=(0, 3), y_f32=True),   # DIAG with classes absent
    "bf16_in": dict(mode=DIAG, in_bf16=True, y_f32=True),
    "dy_f32": dict(mode=DIAG, dy_f32=True),
    "pos": dict(mode=DIAG, pos=True, y_f32=True),                # B = 3: row % T wraps twice
    "y_both": dict(mode=DIAG, y_f32=True),
    "init": dict(mode=DIAG, in_bf16=True, pos=True, ln=False),   # the encoder's initial FDDT + positions
}
CONFIG_WIDTHS = {"layer": WIDTHS, "ln": WIDTHS, "dy_f32": (256, 1280, 2304), "init": (516, 1280)}      # the others: (516, 1280, 2304)

_STAGED = (256, 1280, 1536, 2048)


def widths(cfg):
    return CONFIG_WIDTHS.get(cfg, (516, 1280, 2304))


def routes(cfg, D, g_out_bf16=True):
    """(forward body, backward body) the library has to run a configuration on -- the expectation the GPU tests assert."""
    wave = D % 256 == 0 and 512 <= D <= 1280
    if D > 2048:
        return "generic_1024", "generic_1024"
    if cfg in ("layer", "dy_f32", "y_both"):       # (y_both: the fp32 y keeps the forward off the staged body, the backward is a layer's)
        fwd = "staged" if D in _STAGED and cfg != "y_both" else "generic_diag"
        bwd = "generic" if cfg == "dy_f32" or D not in _STAGED else "staged_bf16" if g_out_bf16 else "staged_f32"
        return fwd, bwd
    if cfg == "ln":
        return ("ln_wave", "ln_wave") if wave else ("generic_ln", "ln_only")
    if cfg in ("bias", "bias_absent"):
        return "generic", "generic"
    if cfg == "init":
        return ("init_wave" if wave else "generic_diag"), "generic"
    return "generic_diag", "generic"


def case_inputs(cfg, D, x, rows, *, mask="soft", eps=1e-5):
    """make_inputs for a configuration at `rows` rows: B = 3 with pos, 2 for the strided masks and for even row counts above 7."""
    kw = {k: v for k, v in CONFIGS[cfg].items() if k != "y_f32"}
    B = 3 if kw.get("pos") and rows % 3 == 0 else 2 if (rows > 7 and rows % 2 == 0) else 1
    gap = 0
    if mask == "strided":
        mask, gap = "soft", 24
    if kw["mode"] == NONE:
        mask = "soft"
    return make_inputs(f"{cfg}.{D}.{x}.{rows}.{mask}.{gap}.{eps}", D, B, rows // B, x=x, mask=mask, eps=eps, gap=gap, **kw)


def host_cases():
    """The case table at host size: every configuration at every width it runs at, every input class; the mask kinds on offset
    rows; the three eps on small-variance rows.  Yields (label, input class label, inp)."""
    for cfg in CONFIGS:
        rows = 9 if CONFIGS[cfg].get("pos") else 8
        for D in widths(cfg):
            for x in X_KINDS:
                yield f"{cfg} D={D} {x}", x, case_inputs(cfg, D, x, rows)
            if CONFIGS[cfg]["mode"] != NONE:
                for mk in MASK_KINDS[1:]:
                    yield f"{cfg} D={D} offset mask={mk}", "mask=" + mk, case_inputs(cfg, D, "offset", rows, mask=mk)
            if CONFIGS[cfg].get("ln", True):
                for e in EPS[1:]:
                    yield f"{cfg} D={D} smallvar eps={e:g}", f"smallvar eps={e:g}", case_inputs(cfg, D, "smallvar", rows, eps=e)


def right_form(inp, ref):
    """The right-form emulation's results: the forward, and the backward with the forward's x and with the collapsed x."""
    f = emulate_fwd(inp)
    mean, rstd = (f["mean"], f["rstd"]) if "mean" in f else (None, None)
    return f, emulate_bwd(inp, mean, rstd), emulate_bwd(inp, mean, rstd, collapsed=True)


def measure():
    """{input class: {C key: worst right-form ratio}} over host_cases(), and the worst of all under "all"."""
    table = {}
    for _, cls, inp in host_cases():
        ref = reference(inp)
        for got in right_form(inp, ref):
            for k, q in ratios(inp, ref, got).items():
                for c in (cls, "all"):
                    table.setdefault(c, {})
                    table[c][k] = max(table[c].get(k, 0.0), q)
    return table


if __name__ == "__main__":
    tb = measure()
    keys = list(C)
    print("right-form fp32 emulation vs fp64: worst error / (2^-24 kappa scale)")
    print(f"{'input class':28s}" + "".join(f"{k:>10s}" for k in keys))
    for cls, row in tb.items():
        print(f"{cls:28s}" + "".join(f"{row.get(k, 0.0):10.2f}" for k in keys))
    print(f"{'C (4 x all, rounded up)':28s}" + "".join(f"{C[k]:10.1f}" for k in keys))

"""fp64 reference (test infrastructure, numpy) of the four decode-time scoring kernels' CTC half (csrc/ctc_prefix.hip):
ctc_frame_lse_kernel, ctc_prefix_init_kernel and ctc_prefix_score_kernel.  Vectorised over hypotheses and candidates, one Python
loop over the frames, so a case costs milliseconds.

The recursion is the one stated at the top of ctc_prefix.hip (the reference's CTCPrefixScore, restated in fp32 with libm by
oracle/ctc_prefix.py, which is pinned to tests/golden/f13_ctc_prefix.npz; tests/test_host_ctc_prefix_ref.py pins this file to both):
    r_n[t] = logaddexp(r_n[t-1], phi[t-1]) + x[t, c]       phi = r_b(g) if c repeats the prefix's last label (d > 0), else r_n(g) (+) r_b(g)
    r_b[t] = logaddexp(r_n[t-1], r_b[t-1]) + x[t, blank]
    psi    = logaddexp(r_n[start-1], logsumexp_{t >= max(d, 1)} (phi[t-1] + x[t, c])),  start = max(d, 1)

LOGZERO IS A SYMBOL HERE.  The reference writes log(0) as -1e10 and relies on fp32 absorbing whatever is added to it; this file
carries it as -inf through the arithmetic (-inf + x = -inf, logaddexp(-inf, a) = a) and writes it out as exactly -1e10 at the end.
Inputs at or below -1e9 are read as logzero.  The two agree only while every log-probability and every real state involved stays
above about -500: half an ulp of 1e10 in fp32 is 512, and below that the reference's fp32 `-1e10 + x` stops being absorbed (it
would round to -1e10 - 1024).  Every prefix-score input of the tests that chains states (d >= 1) therefore keeps its
log-probabilities and real states above -500; `in_domain` checks it.  With d = 0 the only logzero states are r_n(g), which enters
through logaddexp alone, and r_b[0] of the output, which nothing is added to, so the magnitudes are free there (the T = 8192 case).

A prefix of d labels needs d frames: r_n[start-1] of the NEW prefix is logzero whenever d >= 1 (phi[t] is logzero for t < d - 1),
so for d > T, where the reference's index start - 1 falls outside its buffer, psi starts from logzero like every other d >= 1.
Only tests/ may import this module.
"""
import numpy as np

LOGZERO = -1e10
_NEG = -np.inf


def to64(a):
    """Exact fp64 copy of a numpy array or a torch tensor (fp32 / bf16 upcast exactly)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().float().numpy()
    return np.asarray(a, dtype=np.float64)


def _sym(a):
    """-1e10 (anything <= -1e9) -> -inf."""
    a = to64(a).copy()
    a[a <= -1e9] = _NEG
    return a


def _out(a):
    """-inf -> -1e10."""
    a = np.array(a, dtype=np.float64)
    a[np.isneginf(a)] = LOGZERO
    return a


def _lae(a, b):
    with np.errstate(invalid="ignore"):
        r = np.logaddexp(a, b)
    return np.where(np.isneginf(a) & np.isneginf(b), _NEG, r)


def _lse(z, axis):
    m = z.max(axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (ms + np.log(np.exp(z - ms).sum(axis=axis, keepdims=True))).squeeze(axis)


def frame_lse(logits, V1):
    """logits [..., ld] (ld >= V1; columns from V1 on are never read) -> fp64 logsumexp over the first V1 columns of the exact
    input values.  -inf logits carry zero mass; a row of nothing but -inf is out of scope."""
    return _lse(to64(logits)[..., :V1], -1)


def log_probs(logits, V1):
    """fp64 log-softmax over the first V1 columns -> [..., V1]."""
    z = to64(logits)[..., :V1]
    return z - frame_lse(z, V1)[..., None]


def initial_state(x, blank):
    """x [B, T, V] log-probabilities -> r [B, T, 2] of the empty prefix: channel 0 logzero, channel 1 the running sum of the blank column."""
    x = to64(x)
    r = np.full(x.shape[:2] + (2,), LOGZERO, dtype=np.float64)
    r[..., 1] = np.cumsum(x[..., blank], axis=1)
    return r


def prefix_score(x, rows, cs, decoded_len, last, r_prev, blank, eos, alias=None):
    """x [Bx, T, V] log-probabilities; rows [n] sample of each hypothesis; cs [n, C] candidate labels; decoded_len [n]; last [n] the
    prefix's last label; r_prev [n, T, 2] (-1e10 = logzero); alias [V] optional column map (label v reads column alias[v], the blank
    included).  Returns psi [n, C], r [n, T, 2, C] in fp64 with logzero written as -1e10.  T = 1 works: the sum over frames is empty."""
    x = to64(x)
    rows, cs, d, last = (np.asarray(a).astype(np.int64) for a in (rows, cs, decoded_len, last))
    n, C = cs.shape
    T = x.shape[1]
    col = cs if alias is None else np.asarray(alias).astype(np.int64)[cs]
    bcol = blank if alias is None else int(np.asarray(alias)[blank])
    xi = x[rows]                                                             # [n, T, V]
    xs = np.take_along_axis(xi, np.broadcast_to(col[:, None, :], (n, T, C)), axis=2)     # [n, T, C]
    xb = xi[:, :, bcol]                                                      # [n, T]
    rp = _sym(r_prev)
    r_sum = _lae(rp[..., 0], rp[..., 1])                                     # [n, T]
    same = (cs == last[:, None]) & (d > 0)[:, None]                          # [n, C]
    phi = np.where(same[:, None, :], rp[:, :, 1:2], r_sum[:, :, None])       # [n, T, C]
    r = np.full((n, T, 2, C), _NEG)
    r[:, 0, 0] = np.where((d == 0)[:, None], xs[:, 0], _NEG)
    psi = r[:, 0, 0].copy()                    # r_n[start - 1]: frame 0 for d <= 1; logzero for every d >= 1 (module docstring)
    if T > 1:
        t_idx = np.arange(1, T)
        terms = np.where((t_idx[None, :] >= d[:, None])[:, :, None], phi[:, :-1] + xs[:, 1:], _NEG)      # [n, T-1, C]
        psi = _lae(psi, _lse(terms, 1))
    for t in range(1, T):
        r[:, t, 0] = _lae(r[:, t - 1, 0], phi[:, t - 1]) + xs[:, t]
        r[:, t, 1] = _lae(r[:, t - 1, 0], r[:, t - 1, 1]) + xb[:, t][:, None]
    psi = np.where(cs == eos, r_sum[:, -1][:, None], psi)
    if eos != blank:
        psi = np.where(cs == blank, _NEG, psi)
    return _out(psi), _out(r)


def in_domain(*arrays, floor=-500.0):
    """True when every real (non-logzero) value of the arrays is above `floor`: the range in which logzero-as-a-symbol and the
    reference's fp32 -1e10 agree (module docstring)."""
    for a in arrays:
        a = to64(a)
        real = a > -1e9
        if real.any() and float(a[real].min()) <= floor:
            return False
    return True

"""numpy oracle of the per-tensor statistics and histograms of include/dicow_hip.h ("tensor statistics"), for ONE tensor, written from
the header's rules and not from the kernel:
  * non-finite elements are counted (NaN, +inf, -inf) and dropped; min / max / absmax / n_zero over the rest;
  * sum / sumsq in double: one partial per 2048-element chunk, each added up in index order, then the partials in chunk order;
  * histogram over the finite elements in fp32 arithmetic (np.float32 operations in the rule's order):
    min == max -> bin 0; else bin = min(bins - 1, (int)((x - min) * bins / (max - min))); where max - min overflows the same on halves.
    A quotient at or past `bins` (+inf included) is the last bin.
Test infrastructure only."""
import numpy as np

CHUNK = 2048
F32 = np.float32


def bin_index(xf, mn, mx, bins, divide_first=False):
    """fp32 bin of every (finite) element of xf for the range [mn, mx], mn < mx; int64."""
    xf = np.asarray(xf, F32)
    lo, hi = F32(mn), F32(mx)
    with np.errstate(over="ignore", invalid="ignore"):
        width = F32(hi - lo)
        if not np.isfinite(width):
            lo, hi, xf = F32(lo * F32(0.5)), F32(hi * F32(0.5)), xf * F32(0.5)
            width = F32(hi - lo)
        d = xf - lo
        q = (d / width) * F32(bins) if divide_first else (d * F32(bins)) / width
        assert q.dtype == F32
        top = q >= F32(bins)
        b = np.where(top, 0, q).astype(np.int64)
    return np.where(top, bins - 1, b)


def ordered_sums(x):
    """(sum, sumsq) of the finite elements of the fp32 vector x as the header defines them (chunk partials in index order, then the
    partials in order), in float64.  A dropped element adds +0.0, which changes no bit of a running sum that started at +0.0."""
    x = np.asarray(x, F32).reshape(-1)
    n = x.size
    if n == 0:
        return 0.0, 0.0
    d = np.where(np.isfinite(x), x, F32(0)).astype(np.float64)
    pad = (-n) % CHUNK
    if pad:
        d = np.concatenate([d, np.zeros(pad)])
    d = d.reshape(-1, CHUNK)
    ps = np.cumsum(d, axis=1)[:, -1]                               # cumsum adds strictly left to right
    pq = np.cumsum(d * d, axis=1)[:, -1]
    return float(np.cumsum(ps)[-1]), float(np.cumsum(pq)[-1])


def stats_ref(x, bins=64, divide_first=False):
    x = np.asarray(x, F32).reshape(-1)
    fin = np.isfinite(x)
    xf = x[fin]
    s, q = ordered_sums(x)
    out = {"numel": int(x.size), "n_nan": int(np.isnan(x).sum()), "n_posinf": int((x == np.inf).sum()), "n_neginf": int((x == -np.inf).sum()),
           "n_zero": int((xf == 0).sum()), "n_finite": int(xf.size), "sum": s, "sumsq": q}
    if xf.size:
        out["min"], out["max"], out["absmax"] = F32(xf.min()), F32(xf.max()), F32(np.abs(xf).max())
    else:
        out["min"], out["max"], out["absmax"] = F32(np.inf), F32(-np.inf), F32(0)
    hist = np.zeros(bins, np.int64)
    if bins and xf.size:
        if out["min"] == out["max"]:
            hist[0] = xf.size
        else:
            hist = np.bincount(bin_index(xf, out["min"], out["max"], bins, divide_first), minlength=bins).astype(np.int64)
    out["hist"] = hist
    return out


def edge_probe_values(mn, mx, bins):
    """The fp32 values one ulp on either side of every torch.linspace edge of [mn, mx] (and the edges), inside the range."""
    import torch
    e = torch.linspace(float(mn), float(mx), bins + 1, dtype=torch.float32).numpy()
    v = np.concatenate([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))]).astype(F32)
    v = v[(v >= F32(mn)) & (v <= F32(mx))]
    return np.unique(np.concatenate([v, np.asarray([mn, mx], F32)]))

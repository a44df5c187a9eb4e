"""The definition of dicow_sample_tokens (include/dicow_hip.h) in numpy: fp32 only where the definition says fp32 (the division by the
temperature, the options themselves), fp64 everywhere else.  Philox comes from tests/bootstrap_ref.py.

    y = x / temperature (fp32; x itself when temperature <= 0, and then no warper);  NaN counts as -inf
    top_k   v removed iff y_v < the k-th largest y, k = min(top_k, V)
    top_p   over what top_k kept: p = softmax(y); v removed iff S_v = sum{p_u : y_u <= y_v} <= 1 - top_p; the maximum stays
    min_p   over what is left: v removed iff ratio_v = exp(y_v - y_max) < min_p
    draw    temperature <= 0: lowest index of the maximum; else argmax over kept v of y_v - log(-log(u_v)), lowest index on ties,
            u_v = ((w_v >> 8) + 0.5) 2^-24, w_v = Philox4x32-10((v >> 2, row_id, step, stream), (seed lo, seed hi))[v & 3]
    logprob x_tok - logsumexp{x_v : v kept}
"""
from types import SimpleNamespace as NS

import numpy as np

from tests.bootstrap_ref import MASK, philox_np

TOP_P_BAND = 2e-5          # |S_v - (1 - top_p)| below which fp32 masses may decide either way (the header's budget)
MIN_P_BAND = 1e-6          # the same for |ratio_v / min_p - 1|
LOGPROB_REL, LOGPROB_ABS = 2.0 ** -22, 70 * 2.0 ** -24


def warp(scores, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0):
    """scores [rows, V] (any float array; read as fp32).  Returns a namespace of [rows, V] arrays: y (fp32), kept (bool), warped (fp32:
    y where kept, else -inf), S (fp64: the cumulative mass sum{p_u : y_u <= y_v} over what top_k kept; NaN outside), ratio (fp64:
    exp(y_v - y_max)), and band (bool: S within TOP_P_BAND of 1 - top_p or ratio within MIN_P_BAND relative of min_p, where the rule
    in question is on and the token got as far as that rule)."""
    x = np.array(scores, dtype=np.float32, copy=True)
    x[np.isnan(x)] = -np.inf
    rows, V = x.shape
    t, tp, mp = np.float32(temperature), np.float32(top_p), np.float32(min_p)
    with np.errstate(all="ignore"):
        y = (x / t).astype(np.float32) if t > 0 else x.copy()
    kept = y > -np.inf
    S = np.full((rows, V), np.nan)
    band = np.zeros((rows, V), bool)
    y64 = y.astype(np.float64)
    with np.errstate(all="ignore"):
        ymax = y64.max(axis=1, keepdims=True)
        ratio = np.exp(y64 - ymax)
    if t > 0:
        k = min(int(top_k), V)
        if top_k > 0 and k < V:
            kth = np.sort(y, axis=1)[:, V - k][:, None]
            kept &= ~(y < kth)
        if tp < 1:
            e = np.where(kept, ratio, 0.0)
            Z = e.sum(axis=1, keepdims=True)
            order = np.argsort(np.where(kept, y64, -np.inf), axis=1, kind="stable")
            sv = np.take_along_axis(np.where(kept, y64, -np.inf), order, axis=1)
            with np.errstate(all="ignore"):
                cs = np.cumsum(np.take_along_axis(e, order, axis=1), axis=1) / Z
            last = np.ones((rows, V), bool)
            last[:, :-1] = sv[:, :-1] != sv[:, 1:]                      # the last member of its tie class: the class's mass ends there
            ends = np.where(last, cs, np.inf)
            s_sorted = np.minimum.accumulate(ends[:, ::-1], axis=1)[:, ::-1]
            s_all = np.empty_like(s_sorted)
            np.put_along_axis(s_all, order, s_sorted, axis=1)
            S = np.where(kept, s_all, np.nan)
            cut = 1.0 - float(tp)
            with np.errstate(invalid="ignore"):
                band |= kept & (np.abs(S - cut) <= TOP_P_BAND) & (y64 != ymax)
                kept &= ~((S <= cut) & (y64 != ymax))
        if mp > 0:
            with np.errstate(invalid="ignore"):
                band |= kept & (np.abs(ratio / float(mp) - 1.0) <= MIN_P_BAND)
                kept &= ~(ratio < float(mp))
    warped = np.where(kept, y, np.float32(-np.inf)).astype(np.float32)
    return NS(x=x, y=y, kept=kept, warped=warped, S=S, ratio=ratio, band=band)


def words(rows_ids, V, seed, step, stream):
    """uint64 [rows, V]: the Philox word of every (row id, token)."""
    rid = np.asarray(rows_ids, dtype=np.int64).astype(np.uint64) & np.uint64(MASK)
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    w = philox_np(blocks, rid[:, None], np.uint64(step & MASK), np.uint64(stream & MASK), seed & MASK, (seed >> 32) & MASK)
    return np.stack(np.broadcast_arrays(*w), axis=2).reshape(len(rid), -1)[:, :V]


def gumbel(w):
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def sample(scores, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, step=0, stream=0, row_ids=None, unfinished=None, eos=-1,
           pad=0):
    """The whole launch.  Returns warp()'s namespace plus keys (fp64 [rows, V]: y + Gumbel noise for kept tokens, -inf elsewhere; y
    itself on the argmax rung), tokens (int64 [rows]), second (the runner-up token, -1 if none), gap (fp64: best key - runner-up key),
    logprob (fp64 [rows]) and unfinished (the flags after the launch, or None)."""
    o = warp(scores, temperature, top_k, top_p, min_p)
    rows, V = o.y.shape
    rid = np.arange(rows) if row_ids is None else np.asarray(row_ids)
    y64 = o.y.astype(np.float64)
    if np.float32(temperature) > 0:
        keys = np.where(o.kept, y64 + gumbel(words(rid, V, seed, step, stream)), -np.inf)
    else:
        keys = np.where(o.kept, y64, -np.inf)
    tok = keys.argmax(axis=1)                                           # (numpy: the first of equal maxima)
    rest = keys.copy()
    rest[np.arange(rows), tok] = -np.inf
    second = rest.argmax(axis=1)
    with np.errstate(invalid="ignore"):
        gap = keys[np.arange(rows), tok] - rest[np.arange(rows), second]
    second = np.where(rest[np.arange(rows), second] > -np.inf, second, -1)
    empty = ~o.kept.any(axis=1)
    x64 = o.x.astype(np.float64)
    with np.errstate(all="ignore"):
        xm = np.where(o.kept, x64, -np.inf).max(axis=1)
        lse = xm + np.log(np.where(o.kept, np.exp(x64 - xm[:, None]), 0.0).sum(axis=1))
        lp = x64[np.arange(rows), tok] - lse
    lp[empty] = np.nan
    tok = np.where(empty, eos, tok).astype(np.int64)
    flags = None
    if unfinished is not None:
        live = np.asarray(unfinished).astype(bool)
        tok = np.where(live, tok, pad)
        lp = np.where(live, lp, 0.0)
        flags = live & (tok != eos)
    o.keys, o.tokens, o.second, o.gap, o.logprob, o.unfinished = keys, tok, second, gap, lp, flags
    return o


def via_transformers(scores, temperature, top_k=0, top_p=1.0, min_p=0.0):
    """transformers' own chain on CPU, fp32: Temperature -> TopK -> TopP -> MinP warpers with min_tokens_to_keep = 1."""
    import torch
    from transformers.generation.logits_process import (MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    sc = torch.as_tensor(np.asarray(scores, dtype=np.float32)).clone()
    ids = torch.zeros(sc.shape[0], 1, dtype=torch.long)
    if temperature != 1.0:
        sc = TemperatureLogitsWarper(float(temperature))(ids, sc)
    if top_k > 0:
        sc = TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=1)(ids, sc)
    if top_p < 1.0:
        sc = TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=1)(ids, sc)
    if min_p > 0.0:
        sc = MinPLogitsWarper(min_p=float(min_p), min_tokens_to_keep=1)(ids, sc)
    return sc.numpy()

"""fp64 reference (test infrastructure, numpy) of timestamp_rules_kernel (csrc/ctc_prefix.hip): Whisper's timestamp rules on rows of
next-token scores, restated from oracle/timestamp_rules.py (pinned to tests/golden/f14_timestamp_rules.npz; this file is pinned to
both by tests/test_host_ctc_prefix_ref.py) with the two things the oracle does not give:
  * the banned mask of the rules alone (pairing, monotonic timestamps, first step, <|notimestamps|>), apart from the detection;
  * the detection's margin in fp64: logsumexp(allowed timestamp scores) - max(allowed text scores).  The oracle compares fp32
    log-probabilities; the log_softmax normaliser cancels in the comparison, so the margin is what decides.  A score of -inf is
    zero mass: it adds nothing to the logsumexp and never is the maximum unless nothing else is left.
Only tests/ may import this module.
"""
import numpy as np

NEG = -np.inf


def banned_mask(ids, V, begin, eos, no_ts, max_init=None):
    """bool [B, V]: labels the rules forbid whatever the scores are."""
    ids = np.asarray(ids)
    B, L = ids.shape
    ts0 = no_ts + 1
    ban = np.zeros((B, V), dtype=bool)
    if no_ts < V:
        ban[:, no_ts] = True
    for k in range(B):
        seq = [int(t) for t in ids[k, begin:]]
        last_ts = len(seq) >= 1 and seq[-1] >= ts0
        pen_ts = len(seq) < 2 or seq[-2] >= ts0
        if last_ts:
            if pen_ts:
                ban[k, ts0:] = True                      # a closed pair: text next
            else:
                ban[k, :eos] = True                      # an open pair: its closing timestamp (or eos) next
        stamps = [t for t in seq if t >= ts0]
        if stamps:
            upto = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
            ban[k, ts0:max(upto, ts0)] = True            # timestamps do not decrease
    if L == begin:
        ban[:, :ts0] = True
        if max_init is not None:
            ban[:, min(ts0 + max_init + 1, V):] = True
    return ban


def _lse64(a):
    a = a[np.isfinite(a) | np.isposinf(a)]
    if a.size == 0:
        return NEG
    m = a.max()
    return float(m + np.log(np.exp(a - m).sum()))


def timestamp_rules(ids, scores, begin, eos, no_ts, max_init=None):
    """ids int [B, L], scores fp32 [B, V].  Returns (banned bool [B, V], margin fp64 [B], out fp32 [B, V]).  margin[k] is
    logsumexp(allowed timestamps) - max(allowed text) in fp64 with -inf as zero mass: +inf when no text is left but timestamp mass
    is, -inf when no timestamp mass is left but text is, nan when neither is (then nothing is detected)."""
    ids = np.asarray(ids)
    s32 = np.asarray(scores, dtype=np.float32)
    B, V = s32.shape
    ts0 = no_ts + 1
    ban = banned_mask(ids, V, begin, eos, no_ts, max_init)
    s = np.where(ban, NEG, s32.astype(np.float64))
    out = np.where(ban, np.float32(NEG), s32)
    margin = np.empty(B, dtype=np.float64)
    for k in range(B):
        ts_lse = _lse64(s[k, ts0:])
        mt = float(s[k, :ts0].max()) if ts0 > 0 else NEG
        margin[k] = np.nan if (ts_lse == NEG and mt == NEG) else ts_lse - mt
        if ts_lse > mt:
            out[k, :ts0] = NEG
    if ids.shape[1] == begin and eos < V:
        out[:, eos] = s32[:, eos]
    return ban, margin, out

"""Audio at any rate -> mono fp32 at the model's rate, on the GPU: host planner + launches of csrc/resample.hip.

The step in front of everything else that handles waveforms here (``NoiseBank``, ``EnrollmentBank``, ``MeetingFrontEnd``,
``features.log_mel``), which all want mono fp32 at 16 kHz.  Recordings arrive as 16-bit PCM at 8 / 44.1 / 48 kHz, often with several
channels; the reference takes the mean over the channels and then calls ``torchaudio.functional.resample(noise, orig_sample_rate,
self.sample_rate)`` (src/data/augmentations.py:401-407).  This module does the same, in that order:

  * ``resample_plan``        the filter bank of ``torchaudio.functional.resample`` with its defaults (``sinc_interp_hann``,
                             ``lowpass_filter_width=6``, ``rolloff=0.99``) for one reduced ratio, built in fp64, rounded once to fp32 and
                             cut down to the one run of taps per phase that is not exactly zero
  * ``resample_segments``    ``dicow_resample`` on a table of segments of flat buffers: one launch per ratio
  * ``resample``             the same for a tensor or a padded batch
  * ``read_wav``             16-bit PCM at any rate, with the standard library -> ``(int16 [n, C], rate)``
  * ``load_recording``       a WAV file -> fp32 ``[n]`` at the model's rate on the device

The arithmetic, with ``g = gcd(orig, new)``, ``o = orig / g``, ``n = new / g``, ``base = min(o, n) * 0.99``, ``width = ceil(6 o / base)``,
``K = 2 width + o``: for phase p < n and tap k < K, ``t = clamp((-p / n + (k - width) / o) * base, -6, 6)`` and ``h[p][k] = sinc(pi t)
cos(pi t / 12)^2 base / o``; ``y[j n + p] = sum_k h[p][k] x[j o + k - width]`` with zeros outside the input; ``ceil(n L / o)`` output
samples.  The Hann window is clamped at +-6 zero crossings, so every tap outside one contiguous run per phase rounds to exactly 0 in
fp32 (a 44.1 kHz -> 16 kHz bank has 475 taps per phase and at most 34 that count): the kernel keeps ``S`` = the longest run per phase.

Not pinned to the reference (torchaudio is not installed where this was written): torchaudio evaluates the same expressions with torch
ops in the waveform's dtype, fp32 here, while this bank is built in fp64 and rounded once; and the kernel sums the compact run of a
phase in ascending order with one fma per tap, where ``conv1d`` sums all K products in an order of its own.  No CPU fallback: the
samples must be on the GPU.
"""
import math
import wave as _wave
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import ops

LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99      # torchaudio.functional.resample's defaults
MAX_CHANNELS = L.RESAMPLE_MAX_CHANNELS


class ResamplePlan:
    """The compact filter bank of one reduced ratio ``o : n``.  ``width`` and ``K = 2 width + o`` are torchaudio's; ``first`` int32 [n]
    (host) is the first tap of each phase's non-zero run in the full fp32 bank, ``S`` the longest run, ``taps`` fp32 ``[n, S]`` on
    ``device`` the runs themselves (zero behind a shorter one): ``y[j n + p] = sum_s taps[p][s] x[j o + first[p] + s - width]``.
    ``identity``: equal rates, one tap of 1.0."""

    def __init__(self, o: int, n: int, width: int, first: np.ndarray, taps: np.ndarray, device):
        self.o, self.n, self.width, self.K = int(o), int(n), int(width), 2 * int(width) + int(o)
        self.first = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int32))
        self.S = int(taps.shape[1])
        self.device = torch.device(device)
        self.taps = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).to(self.device)
        self._taps_t = self.taps.t().contiguous()               # [S, n]: what the kernel reads
        self.identity = self.o == 1 and self.n == 1

    def out_len(self, length: int) -> int:
        return -(-self.n * int(length) // self.o)


def full_bank64(o: int, n: int, p0: int = 0, p1: Optional[int] = None):
    """torchaudio's ``_get_sinc_resample_kernel`` for the reduced ratio, in fp64: ``(width, h [p1 - p0, 2 width + o])``, the phases
    ``p0 <= p < p1`` (default: all n)."""
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    t = (np.arange(-p0, -(n if p1 is None else p1), -1, dtype=np.float64)[:, None] / n + idx) * base
    t = np.clip(t, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return width, sinc * window * (base / o)


MAX_BANK_ELEMENTS = 1 << 28                  # n * K of the full bank a plan is built from (a few seconds of host work)
_PLANS = {}


def resample_plan(orig_freq: int, new_freq: int, device="cpu") -> ResamplePlan:
    """The plan for ``orig_freq -> new_freq``, cached per reduced ratio and device."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"resample_plan: sample rates must be positive, got {orig_freq} -> {new_freq}")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (o, n, str(device))
    plan = _PLANS.get(key)
    if plan is not None:
        return plan
    if max(o, n) > L.RESAMPLE_MAX_RATIO:
        raise L.DicowError(f"resample_plan: {orig_freq} -> {new_freq} reduces to {o} : {n}, outside the limit of {L.RESAMPLE_MAX_RATIO}")
    if o == n:
        plan = ResamplePlan(1, 1, 0, np.zeros(1, np.int32), np.ones((1, 1), np.float32), device)
    else:
        width = math.ceil(LOWPASS_FILTER_WIDTH * o / (min(o, n) * ROLLOFF))
        if n * (2 * width + o) > MAX_BANK_ELEMENTS:
            raise L.DicowError(f"resample_plan: {orig_freq} -> {new_freq} reduces to {o} : {n}, whose full bank of {n} x {2 * width + o} taps "
                               f"is beyond the limit of {MAX_BANK_ELEMENTS} elements")
        first, runs = np.zeros(n, np.int64), []
        for p0 in range(0, n, 1024):                            # the full bank 1024 phases at a time
            h32 = full_bank64(o, n, p0, min(n, p0 + 1024))[1].astype(np.float32)       # rounded once
            nz = h32 != 0
            f = nz.argmax(1)
            last = h32.shape[1] - 1 - nz[:, ::-1].argmax(1)
            first[p0:p0 + h32.shape[0]] = f
            runs.extend(h32[q, f[q]:last[q] + 1] for q in range(h32.shape[0]))
        S = max(r.size for r in runs)
        taps = np.zeros((n, S), np.float32)
        for p, run in enumerate(runs):
            taps[p, :run.size] = run
        plan = ResamplePlan(o, n, width, first, taps, device)
    _PLANS[key] = plan
    return plan


def resample_segments(src: torch.Tensor, plan: ResamplePlan, segs, out: torch.Tensor, channel: Optional[int] = None,
                      frames_per_tile: int = 0) -> torch.Tensor:
    """One ``dicow_resample`` launch.  ``src``: flat fp32 ``[frames]`` (mono) or int16 ``[frames, C]`` on the GPU, contiguous; ``segs``:
    int64 ``[k, 3]`` on the host, rows ``(in_start, in_len, out_start)`` in frames of ``src`` and samples of ``out``; ``out``: flat
    contiguous fp32 on the same GPU.  Segment k's ``plan.out_len(in_len)`` samples are written at ``out_start``, nothing else is; the
    output ranges must not overlap.  int16: ``channel=None`` takes the mean over the channels, ``channel=c`` that channel.
    ``frames_per_tile``: output frames (of n samples) per workgroup, 0 = the library's choice; the result does not depend on it."""
    for t, name in ((src, "src"), (out, "out")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.DicowError(f"resample_segments: {name} must be on the GPU (no CPU fallback)")
        if not t.is_contiguous():
            raise L.DicowError(f"resample_segments: {name} must be contiguous")
    if src.dtype == torch.float32 and src.dim() == 1:
        is16, C = 0, 1
    elif src.dtype == torch.int16 and src.dim() == 2 and src.shape[1] >= 1:
        is16, C = 1, int(src.shape[1])
    else:
        raise L.DicowError(f"resample_segments: src must be fp32 [frames] or int16 [frames, C], got {src.dtype} {tuple(src.shape)}")
    if out.dtype != torch.float32 or out.dim() != 1 or out.device != src.device:
        raise L.DicowError("resample_segments: out must be a flat fp32 tensor on src's device")
    if C > MAX_CHANNELS:
        raise L.DicowError(f"resample_segments: {C} channels; at most {MAX_CHANNELS}")
    ch = -1 if channel is None else int(channel)
    if not -1 <= ch < C or (channel is not None and ch < 0):
        raise L.DicowError(f"resample_segments: channel {channel} outside the {C} channels")
    if plan.device != src.device:
        raise L.DicowError(f"resample_segments: the plan is on {plan.device}, the samples on {src.device}")
    table = np.ascontiguousarray(np.asarray(segs, dtype=np.int64).reshape(-1, 3))
    k = table.shape[0]
    first = plan.first.numpy()
    with torch.cuda.device(src.device):
        nbytes = L.lib().dicow_resample_ws_bytes(k, plan.n)
        ws = ops.workspace(nbytes, src.device)
        L.call("dicow_resample", src.data_ptr(), is16, C, ch, src.shape[0], out.data_ptr(), out.numel(), plan._taps_t.data_ptr(),
               first.ctypes.data, plan.o, plan.n, plan.width, plan.S, table.ctypes.data if k else None, k, int(frames_per_tile),
               ws.data_ptr(), nbytes, L.stream())
    return out


def resample(x: torch.Tensor, orig_freq: int, new_freq: int = 16000, lengths=None, channel: Optional[int] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x`` on the GPU -- fp32 ``[n]`` / ``[B, n]`` (mono), or int16 ``[n, C]`` / ``[B, n, C]`` (interleaved, as a WAV file holds it) ->
    mono fp32 at ``new_freq``: ``[ceil(new n / orig)]``, or ``[B, max_out]`` with every row zero behind the ``ceil(new len / orig)``
    samples of its own ``lengths[b]`` (default: all n).  int16 becomes ``sample / 32768``; several channels are averaged as
    ``torch.mean`` does (``channel=c`` takes channel c instead) before the filter, the reference's order.  Equal rates run the identity
    plan: conversion and mixdown only, the values unchanged (a negative zero comes out positive).  ``out``: a contiguous fp32 tensor of the
    result's shape to fill."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise L.DicowError("resample: x must be on the GPU (no CPU fallback)")
    if x.dtype == torch.float32 and x.dim() in (1, 2):
        batched, C = x.dim() == 2, 1
        if channel not in (None, 0):
            raise L.DicowError(f"resample: channel {channel} of mono fp32 input")
        channel = None
    elif x.dtype == torch.int16 and x.dim() in (2, 3):
        batched, C = x.dim() == 3, int(x.shape[-1])
    else:
        raise L.DicowError(f"resample: x must be fp32 [n] / [B, n] or int16 [n, C] / [B, n, C], got {x.dtype} {tuple(x.shape)}")
    B, n_in = (int(x.shape[0]), int(x.shape[1])) if batched else (1, int(x.shape[0]))
    if C < 1:
        raise L.DicowError("resample: int16 input without channels")
    if lengths is None:
        lens = [n_in] * B
    else:
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lens) != B or any(not 0 <= v <= n_in for v in lens):
            raise L.DicowError(f"resample: lengths must hold {B} values in [0, {n_in}]")
    plan = resample_plan(orig_freq, new_freq, x.device)
    max_out = max([plan.out_len(v) for v in lens], default=0)
    shape = (B, max_out) if batched else (max_out,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != x.device
          or not out.is_contiguous()):
        raise L.DicowError(f"resample: out must be a contiguous fp32 tensor of shape {shape} on {x.device}")
    if any(plan.out_len(v) < max_out for v in lens):
        out.zero_()
    src = x.contiguous().reshape(-1) if C == 1 and x.dtype == torch.float32 else x.contiguous().reshape(-1, C)
    segs = [(b * n_in, lens[b], b * max_out) for b in range(B)]
    resample_segments(src, plan, segs, out.reshape(-1), channel)
    return out


def read_wav(path):
    """A 16-bit PCM WAV file at any rate -> ``(int16 [n, C] CPU tensor, rate)``, read with the standard library.  Another sample width
    is refused."""
    with _wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"read_wav: {path} has {8 * w.getsampwidth()}-bit samples; only 16-bit PCM is read")
        ch, rate = w.getnchannels(), w.getframerate()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return torch.from_numpy(pcm.astype(np.int16).reshape(-1, ch)), int(rate)


def load_recording(path, device="cuda", sample_rate: int = 16000, channel: Optional[int] = None) -> torch.Tensor:
    """A 16-bit PCM WAV file at any rate, with any number of channels -> mono fp32 ``[n]`` at ``sample_rate`` on ``device``: the mean
    over the channels (or ``channel``), then the resampler.  ``n = ceil(sample_rate * frames / rate)`` is the ``n_samples`` that a
    ``SpeakerSegments.from_rttm(..., n_samples=n)`` of this recording must carry for ``MeetingFrontEnd.prepare``."""
    if torch.device(device).type != "cuda":
        raise L.DicowError("load_recording: the device must be a GPU (no CPU fallback)")
    pcm, rate = read_wav(path)
    return resample(pcm.to(device), rate, sample_rate, channel=channel)


def bank_from_files(files, sample_rate: int, device, who: str, at_rate, mono_only: bool = False):
    """The banks' loader for ``from_dir(resample=True)``: every file read with ``read_wav``; one already at ``sample_rate`` becomes
    ``at_rate(pcm)`` (an fp32 ``[n]`` host tensor: the bank's own preparation, unchanged), every other one goes up as int16 and is mixed
    down and resampled on the device, one upload and one launch per distinct (rate, channel count).  Returns ``(data, starts, lens,
    foreign)``: the bank's flat fp32 buffer on ``device`` with clip k at ``data[starts[k] : starts[k] + lens[k]]``, and the indices of the
    clips that were resampled."""
    lens, ready, groups = [], {}, {}
    for k, f in enumerate(files):
        pcm, rate = read_wav(f)
        if pcm.shape[0] == 0 or (mono_only and pcm.shape[1] != 1):
            raise ValueError(f"{who}: clip {k} ({f}) must be {'mono, ' if mono_only else ''}[n, C] with n > 0, got {tuple(pcm.shape)}")
        if rate == sample_rate:
            ready[k] = at_rate(pcm)
            lens.append(int(ready[k].numel()))
        else:
            groups.setdefault((rate, int(pcm.shape[1])), []).append((k, pcm))
            lens.append(resample_plan(rate, sample_rate).out_len(pcm.shape[0]))
    if groups and torch.device(device).type != "cuda":
        raise L.DicowError(f"{who}: resample=True brings files at another rate to {sample_rate} Hz on the GPU; build the bank there "
                           "(no CPU fallback)")
    starts = [0]
    for n in lens[:-1]:
        starts.append(starts[-1] + n)
    data = torch.empty(sum(lens), dtype=torch.float32, device=device)
    for k, clip in ready.items():
        data[starts[k]:starts[k] + lens[k]] = clip.to(device)
    for (rate, _), members in groups.items():
        segs, at = [], 0
        for k, pcm in members:
            segs.append((at, int(pcm.shape[0]), starts[k]))
            at += int(pcm.shape[0])
        resample_segments(torch.cat([pcm for _, pcm in members]).to(data.device), resample_plan(rate, sample_rate, data.device), segs, data)
    return data, starts, lens, sorted(k for members in groups.values() for k, _ in members)

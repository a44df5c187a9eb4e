"""fp64 restatement of ``torchaudio.functional.resample`` with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), the
oracle of tests/test_host_resample.py and tests/test_gpu_resample.py.  Written from the formula, independently of
ts-asr-whisper_amd/wave_intake.py (torchaudio itself is not a dependency of this project):

    g = gcd(orig, new); o = orig / g; n = new / g; base = min(o, n) * 0.99; width = ceil(6 o / base); K = 2 width + o
    t = clamp((-p / n + (k - width) / o) * base, -6, 6);   h[p][k] = sinc(pi t) cos(pi t / 12)^2 base / o        p < n, k < K
    y[j n + p] = sum_k h[p][k] x[j o + k - width], x = 0 outside [0, L);   ceil(n L / o) output samples
"""
import math

import numpy as np
import torch

from tests.util import hashed_uniform

# (orig, new): the rates recordings arrive at, and one decimation by two
RATIOS = [(8000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000), (44100, 16000), (48000, 16000), (16000, 8000)]
LENGTHS = [1, 2, 7, 50, 442, 4097, 10007]


def sizes(orig, new):
    """(o, n, width, K) from the formula."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    return o, n, width, 2 * width + o


class Bank:
    """The full bank of one ratio: ``h64`` [n, K] in fp64, ``h32`` its single rounding to fp32, and the compact bank derived from
    ``h32``: ``first[p]`` / ``last[p]`` = the first / last tap of phase p that is not exactly zero, ``S`` the longest such run, ``taps``
    fp32 [n, S] the runs (zero behind a shorter one)."""

    def __init__(self, orig, new):
        self.orig, self.new = orig, new
        self.o, self.n, self.width, self.K = o, n, width, K = sizes(orig, new)
        base = min(o, n) * 0.99
        h = np.empty((n, K), np.float64)
        for p in range(n):
            for k in range(K):
                t = (-p / n + (k - width) / o) * base
                t = min(6.0, max(-6.0, t))
                s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
                h[p, k] = s * math.cos(math.pi * t / 12) ** 2 * base / o
        self.h64 = h
        self.h32 = h.astype(np.float32)
        nz = self.h32 != 0
        self.first = np.array([int(np.flatnonzero(nz[p])[0]) for p in range(n)])
        self.last = np.array([int(np.flatnonzero(nz[p])[-1]) for p in range(n)])
        self.S = int((self.last - self.first + 1).max())
        self.taps = np.zeros((n, self.S), np.float32)
        for p in range(n):
            self.taps[p, :self.last[p] - self.first[p] + 1] = self.h32[p, self.first[p]:self.last[p] + 1]

    def out_len(self, L):
        return -(-self.n * L // self.o)


_BANKS = {}


def bank(orig, new):
    if (orig, new) not in _BANKS:
        _BANKS[(orig, new)] = Bank(orig, new)
    return _BANKS[(orig, new)]


def _frames(x, b):
    """x [L] -> the [J, K] windows torchaudio's conv1d(stride=o) sees: J = L // o + 1 frames of the input padded by (width, width + o)."""
    L = x.shape[0]
    xp = np.concatenate([np.zeros(b.width, x.dtype), x, np.zeros(b.width + b.o, x.dtype)])
    J = L // b.o + 1
    return np.lib.stride_tricks.as_strided(xp, (J, b.K), (b.o * xp.itemsize, xp.itemsize), writeable=False)


def _apply(fr, h):
    """y[j, p] = sum_k fr[j, k] h[p, k] in fp64, k ascending (one order whatever the sizes, so an exactly zero tap changes nothing)."""
    y = np.zeros((fr.shape[0], h.shape[0]), np.float64)
    for k in range(h.shape[1]):
        y += fr[:, k, None] * h[None, :, k]
    return y


def resample64(x, b, h=None):
    """x [L] (any float dtype; taken to fp64) times the bank ``h`` (default: the fp32 bank, the values the kernel holds) in fp64."""
    x = np.asarray(x, np.float64)
    h = b.h32 if h is None else h
    return _apply(_frames(x, b), np.asarray(h, np.float64)).reshape(-1)[:b.out_len(x.shape[0])]


def resample64_compact(x, b):
    """The same with the compact bank: only taps first[p] .. first[p] + S - 1 of every phase (a run may be padded past K with zero taps,
    which then meet zero input)."""
    x = np.asarray(x, np.float64)
    fr = _frames(x, b)
    frp = np.concatenate([fr, np.zeros((fr.shape[0], b.S), np.float64)], 1)
    h = np.zeros((b.n, b.K + b.S), np.float64)
    for p in range(b.n):
        h[p, b.first[p]:b.first[p] + b.S] = b.taps[p]
    return _apply(frp, h).reshape(-1)[:b.out_len(x.shape[0])]


def reference32(x32, b):
    """The reference's formulation: fp32 ``conv1d(stride=o)`` with the full [n, 1, K] bank on the CPU, padded and trimmed as torchaudio does."""
    x = torch.as_tensor(x32, dtype=torch.float32).reshape(1, 1, -1)
    L = x.shape[-1]
    xp = torch.nn.functional.pad(x, (b.width, b.width + b.o))
    y = torch.nn.functional.conv1d(xp, torch.from_numpy(b.h32)[:, None, :], stride=b.o)     # [1, n, J]
    return y.transpose(1, 2).reshape(-1)[:b.out_len(L)].numpy()


def emulate_kernel(x32, taps, first, o, n, width, out_len):
    """What the kernel computes, on the host: per output ``acc = 0; for s ascending: acc = fmaf(taps[p][s], x[j o + first[p] + s - width],
    acc)`` -- the fp32 product is exact in fp64, so one fp64 add rounded to fp32 is the fma up to a double rounding."""
    x = np.asarray(x32, np.float32)
    L, S = x.shape[0], taps.shape[1]
    J = -(-out_len // n)
    pad_l, pad_r = width, J * o + int(np.max(first)) + S
    xp = np.concatenate([np.zeros(pad_l, np.float32), x, np.zeros(pad_r, np.float32)]).astype(np.float64)
    y = np.zeros((J, n), np.float32)
    j = np.arange(J)
    for p in range(n):
        acc = np.zeros(J, np.float32)
        for s in range(S):
            acc = (float(taps[p, s]) * xp[j * o + int(first[p]) + s] + acc.astype(np.float64)).astype(np.float32)
        y[:, p] = acc
    return y.reshape(-1)[:out_len]


def bound(y64, e_ref):
    """4 e_ref + 2^-23 max|y64|: four times the error of the reference's own fp32 formulation on the case (the project's margin for another
    order of summation, as for noise_mix) plus half an ulp of the largest output."""
    return 4.0 * e_ref + 2.0 ** -23 * float(np.max(np.abs(y64))) if y64.size else 0.0


def wave(orig, new, L, tag="x"):
    """Hashed-uniform fp32 input in [-1, 1), a pure function of its arguments."""
    return hashed_uniform(f"resample.{orig}.{new}.{L}.{tag}", (L,))


def pcm(orig, new, L, C, tag="pcm"):
    """Hashed int16 [L, C]."""
    u = hashed_uniform(f"resample.{orig}.{new}.{L}.{C}.{tag}", (L, C)).double()
    return torch.round(u * 32767.0).to(torch.int16)


def mono_of(p16, channel=None):
    """The reference's mixdown of int16 [L, C] on the CPU: ``torch.mean(pcm / 32768, 0)`` over the channels (what ``torchaudio.load`` returns,
    channels first), or one channel."""
    x = (p16.to(torch.float32) / 32768.0).t().contiguous()                  # [C, L]
    if channel is not None:
        return x[channel]
    return torch.mean(x, dim=0) if x.shape[0] > 1 else x[0]

"""From a recording and its diarization to the batch ``model.generate`` takes: STNO masks and SE-DiCoW's self-enrollment windows on the GPU
(csrc/diar_front_end.hip).

Mirrors, for one recording, what the reference's datasets compute per target speaker on dense ``[S, n_samples]`` masks
(src/data/local_datasets.py): ``get_stno_mask`` / ``_create_stno_masks`` (:162-194) and ``select_random_internal_enrollment`` with
``downsample_mean`` and ``sample_enrollment_window`` (:216-292; ``greedy_sample=True`` for evaluation :595-597, ``False`` for training
:468-470).  Here the diarization stays what it is, a few thousand interval endpoints:

  * ``SpeakerSegments``             half-open sample intervals per speaker -> the table ``bounds`` int64 [E + 1] / ``active`` uint64 [E], built
                                    in one sweep over the sorted endpoints; no per-sample array, on the host or on the device
  * ``stno_masks``                  ``dicow_diar_frame_counts`` (once per recording, cached) + ``dicow_stno_from_counts``: fp32 [K, 4, T_total],
                                    bit-equal to the reference's numpy arithmetic
  * ``select_enrollment_windows``   ``dicow_enrollment_windows``: the reference's greedy search in exact integers -- the FIRST window of
                                    maximal solo activity, or of maximal activity for a speaker who is never alone
  * ``draw_enrollment_window``      the reference's non-greedy draw from a weights row, on the host with numpy's generator
  * ``MeetingFrontEnd``             wave + segments -> ``input_features`` (one log-mel shared by all targets), ``attention_mask``,
                                    ``stno_mask`` and, for SE-DiCoW, ``enrollments``

Stated deviations from the reference: the greedy search takes the first exact maximum, where the reference's fp64 ``np.convolve`` lets
rounding noise of about 1e-11 choose among windows whose true counts are equal (its choice always has the maximal count); and a recording
under 30 s gives start 0 with the total as the count, where the reference's ``np.convolve(..., 'valid')`` swaps its operands.  16 kHz only.
No CPU fallback.
"""
import numpy as np
import torch

from . import _lib as L
from . import features, ops

FRAME, BIN, WINDOW_BINS, MAX_SPEAKERS = L.DIAR_FRAME, L.DIAR_BIN, L.DIAR_WINDOW, L.DIAR_MAX_SPEAKERS
N_SAMPLES_30S, FRAMES_30S = 480000, 1500


class SpeakerSegments:
    """A diarization of one recording: per speaker a list of half-open sample intervals ``[start, end)`` at 16 kHz (the contract; seconds
    and RTTM files are conveniences on top).  Speakers are ordered with ``sorted()`` as the reference orders them (:163); intervals are
    clipped to ``[0, n_samples)``, empty ones dropped; intervals of one speaker may overlap (the reference's mask is their union).

    ``bounds`` int64 [E + 1] (strictly increasing) and ``active`` uint64 [E] -- bit s of ``active[e]`` set when ``speakers[s]`` talks on
    ``[bounds[e], bounds[e + 1])`` -- are the table the kernels read; E is at most twice the number of intervals.  Without any interval
    E = 0 and ``bounds`` is ``[0]``."""

    def __init__(self, intervals, n_samples):
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"SpeakerSegments: n_samples must be positive, got {n_samples}")
        self.n_samples = n_samples
        self.speakers = sorted(intervals)
        if len(self.speakers) > MAX_SPEAKERS:
            raise ValueError(f"SpeakerSegments: {len(self.speakers)} speakers, at most {MAX_SPEAKERS} fit the table's bitmask")
        if not self.speakers:
            raise ValueError("SpeakerSegments: no speakers")
        self.intervals = {}
        for spk in self.speakers:
            kept = []
            for a, b in intervals[spk]:
                if int(a) != a or int(b) != b:
                    raise ValueError(f"SpeakerSegments: sample positions must be integers, got ({a}, {b}) for {spk!r}")
                a, b = max(0, int(a)), min(n_samples, int(b))
                if a < b:
                    kept.append((a, b))
            self.intervals[spk] = kept
        self.bounds, self.active = _sweep([self.intervals[s] for s in self.speakers])
        self._counts = {}

    S = property(lambda self: len(self.speakers))
    E = property(lambda self: int(self.active.shape[0]))
    T_total = property(lambda self: -(-self.n_samples // N_SAMPLES_30S) * FRAMES_30S)
    n_bins = property(lambda self: self.n_samples // BIN)
    n_windows = property(lambda self: max(self.n_bins - WINDOW_BINS + 1, 1))

    @classmethod
    def from_samples(cls, intervals, n_samples):
        return cls(intervals, n_samples)

    @classmethod
    def from_seconds(cls, intervals, n_samples, sampling_rate=16000):
        """Intervals in seconds (``n_samples`` stays in samples: it is the length of the wave), each bound rounded to a sample with Python's
        ``round`` (half to even).  The reference gets its mask from lhotse's ``Cut.speakers_audio_mask``, whose own rounding could not be
        checked while this was written (lhotse was not installed); pass samples where a boundary sample matters."""
        if sampling_rate != 16000:
            raise ValueError("SpeakerSegments: 16 kHz only (no resampling here)")
        return cls({k: [(round(a * sampling_rate), round(b * sampling_rate)) for a, b in v] for k, v in intervals.items()}, n_samples)

    @classmethod
    def from_rttm(cls, path, recording_id=None, n_samples=None, sampling_rate=16000):
        """``SPEAKER <recording> <channel> <start> <duration> <NA> <NA> <speaker> ...`` lines of an RTTM file; other line types and, when
        ``recording_id`` is given, other recordings are skipped.  RTTM does not carry the recording's length: pass the wave's ``n_samples``
        (default: the end of the last segment)."""
        out = {}
        with open(path) as f:
            for line in f:
                p = line.split()
                if len(p) < 8 or p[0] != "SPEAKER" or (recording_id is not None and p[1] != recording_id):
                    continue
                out.setdefault(p[7], []).append((float(p[3]), float(p[3]) + float(p[4])))
        if not out:
            raise ValueError(f"SpeakerSegments: no SPEAKER line{'' if recording_id is None else ' of ' + repr(recording_id)} in {path}")
        if n_samples is None:
            n_samples = max(round(b * sampling_rate) for v in out.values() for _, b in v)
        return cls.from_seconds(out, n_samples, sampling_rate)

    def index_of(self, target):
        """A target as the kernels index it: an ``int`` is taken as is (-1 = the reference's unknown speaker), anything else is looked up
        among the speakers; the string "-1" names the unknown speaker unless a speaker is called that."""
        if isinstance(target, (int, np.integer)) and not isinstance(target, bool):
            t = int(target)
            if not -1 <= t < self.S:
                raise ValueError(f"SpeakerSegments: target index {t} outside [-1, {self.S})")
            return t
        if target in self.intervals:
            return self.speakers.index(target)
        if target == "-1":
            return -1
        raise KeyError(f"SpeakerSegments: no speaker {target!r}")

    def target_indices(self, targets=None):
        return list(range(self.S)) if targets is None else [self.index_of(t) for t in targets]

    def relabelled(self, mapping, default="-1"):
        """The same diarization under other names, as ``apply_speaker_mapping`` of the reference's
        ``utils/align_and_compute_der_between_cutsets.py`` renames a hypothesis: speaker ``k`` becomes ``mapping[k]``, a speaker the mapping
        does not name becomes ``default``.  Speakers that end up under one name are merged: their intervals, sorted, with overlapping and
        touching ones joined (a union)."""
        merged, sources = {}, {}
        for spk in self.speakers:
            name = mapping.get(spk, default)
            merged.setdefault(name, []).extend(self.intervals[spk])
            sources[name] = sources.get(name, 0) + 1
        for name, iv in merged.items():
            if sources[name] > 1:
                out = []
                for a, b in sorted(iv):
                    if out and a <= out[-1][1]:
                        out[-1] = (out[-1][0], max(out[-1][1], b))
                    else:
                        out.append((a, b))
                merged[name] = out
        return SpeakerSegments(merged, self.n_samples)

    def to_rttm(self, path, recording_id, channel=1):
        """The inverse of ``from_rttm``: one ``SPEAKER`` line per raw interval, sorted by start, times in seconds with six decimals -- under
        a hundredth of a sample, so ``from_rttm(path, recording_id, n_samples)`` gives these intervals back exactly."""
        rows = sorted((a, b, spk) for spk in self.speakers for a, b in self.intervals[spk])
        with open(path, "w") as f:
            for a, b, spk in rows:
                f.write(f"SPEAKER {recording_id} {channel} {a / 16000:.6f} {(b - a) / 16000:.6f} <NA> <NA> {spk} <NA> <NA>\n")


def _sweep(per_speaker):
    """One sweep over all interval endpoints, sorted: a running count of open intervals per speaker (a speaker's intervals may overlap), read
    off behind the last event of every distinct position.  -> (bounds int64 [E + 1], active uint64 [E])."""
    n = sum(len(v) for v in per_speaker)
    if n == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint64)
    S = len(per_speaker)
    pos, spk, delta = np.empty(2 * n, np.int64), np.empty(2 * n, np.int64), np.empty(2 * n, np.int32)
    i = 0
    for s, iv in enumerate(per_speaker):
        for a, b in iv:
            pos[i], spk[i], delta[i] = a, s, 1
            pos[i + 1], spk[i + 1], delta[i + 1] = b, s, -1
            i += 2
    order = np.argsort(pos, kind="stable")
    pos, spk, delta = pos[order], spk[order], delta[order]
    step = np.zeros((2 * n, S), dtype=np.int32)
    step[np.arange(2 * n), spk] = delta
    open_ = np.cumsum(step, axis=0)
    bounds, first = np.unique(pos, return_index=True)
    last = np.append(first[1:], 2 * n) - 1                         # the last event at each distinct position
    on = open_[last[:-1]] > 0                                       # [E, S]: who talks between this position and the next
    bits = np.left_shift(np.uint64(1), np.arange(S, dtype=np.uint64))
    active = np.bitwise_or.reduce(np.where(on, bits[None, :], np.uint64(0)), axis=1).astype(np.uint64)
    return np.ascontiguousarray(bounds, dtype=np.int64), np.ascontiguousarray(active)


def _device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise L.DicowError("diar_front_end: the kernels run on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def frame_counts(segs, device=None):
    """(cnt, excl) int32 [S, T_total] on the device: per 320-sample frame the samples on which a speaker is active / the only one active.
    Computed once per ``SpeakerSegments`` and device; both consumers below read the cached pair."""
    device = _device(device)
    got = segs._counts.get(device)
    if got is None:
        with torch.cuda.device(device):
            both = torch.empty(2, segs.S, segs.T_total, dtype=torch.int32, device=device)
            nbytes = L.lib().dicow_diar_table_ws_bytes(segs.E)
            ws = ops.workspace(nbytes, device)
            L.call("dicow_diar_frame_counts", segs.bounds.ctypes.data, segs.active.ctypes.data if segs.E else None, segs.E, segs.S,
                   segs.n_samples, both[0].data_ptr(), both[1].data_ptr(), ws.data_ptr(), nbytes, L.stream())
        got = segs._counts[device] = (both[0], both[1])
    return got


def stno_masks(segs, targets=None, out=None, device=None):
    """fp32 ``[len(targets), 4, T_total]`` on the device, channels S, T, N, O: what the reference's ``get_stno_mask`` returns for each
    target (transposed to the model's layout), bit for bit.  ``targets``: speaker names or indices, -1 / "-1" for the unknown speaker
    (default: every speaker, in order).  ``out``: a tensor of that shape to fill, unit stride along T and evenly spaced rows (a view
    into longer rows is fine); nothing outside it is written."""
    idx = segs.target_indices(targets)
    K, T = len(idx), segs.T_total
    if out is None:
        out = torch.empty(K, 4, T, dtype=torch.float32, device=_device(device))
    else:
        if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (K, 4, T):
            raise L.DicowError(f"stno_masks: out must be an fp32 GPU tensor of shape {(K, 4, T)}")
        ld = out.stride(1)
        if out.stride(2) != 1 or ld < T or (K > 1 and out.stride(0) != 4 * ld):
            raise L.DicowError("stno_masks: out needs unit stride along T and rows a constant stride >= T_total apart")
    if K == 0:
        return out
    dev = out.device
    cnt, _ = frame_counts(segs, dev)
    tg = segs._targets_stno = np.asarray(idx, dtype=np.int32)        # (kept: the stream may read the host array after the call returns)
    with torch.cuda.device(dev):
        nbytes = L.lib().dicow_diar_targets_ws_bytes(K)
        ws = ops.workspace(nbytes, dev)
        L.call("dicow_stno_from_counts", cnt.data_ptr(), segs.S, segs.n_samples, tg.ctypes.data, K, out.data_ptr(), out.stride(1),
               ws.data_ptr(), nbytes, L.stream())
    return out


def select_enrollment_windows(segs, targets=None, return_weights=False, device=None):
    """The reference's greedy self-enrollment search for each target, on the device: ``(start, count, fallback)`` int32 [K] -- the first
    0.1 s bin of the 30 s window with the most samples on which the target talks alone, that number of samples, and 0; for a target that
    is never alone the window with the most samples on which it talks at all, and 1 (the reference's fallback, :271-277).  The window is
    the samples ``[1600 * start, 1600 * start + 480000)``.  ``return_weights``: also int32 ``[K, n_windows]``, every window's count (of
    the pass taken), for ``draw_enrollment_window``.  The unknown speaker (-1) has no enrollment."""
    idx = segs.target_indices(targets)
    if any(t < 0 for t in idx):
        raise ValueError("select_enrollment_windows: the unknown speaker (-1) has no enrollment window")
    dev = _device(device)
    K, nw = len(idx), segs.n_windows
    res = torch.empty(3, K, dtype=torch.int32, device=dev)
    weights = torch.empty(K, nw, dtype=torch.int32, device=dev) if return_weights else None
    if K:
        cnt, excl = frame_counts(segs, dev)
        tg = segs._targets_enr = np.asarray(idx, dtype=np.int32)     # (kept, as in stno_masks)
        with torch.cuda.device(dev):
            nbytes = L.lib().dicow_enrollment_windows_ws_bytes(segs.n_samples, K)
            ws = ops.workspace(nbytes, dev)
            L.call("dicow_enrollment_windows", cnt.data_ptr(), excl.data_ptr(), segs.S, segs.n_samples, tg.ctypes.data, K, res[0].data_ptr(),
                   res[1].data_ptr(), res[2].data_ptr(), L.ptr(weights), nw, ws.data_ptr(), nbytes, L.stream())
    return (res[0], res[1], res[2], weights) if return_weights else (res[0], res[1], res[2])


def draw_enrollment_window(weights_row, skew_param=5.0, rng=np.random):
    """The non-greedy branch of the reference's ``sample_enrollment_window`` (:229-246) on one row of ``select_enrollment_windows``'
    weights: probabilities ``(w / 1600) ** skew_param``, normalised, and one ``rng.choice`` over the window starts -- with ``rng =
    np.random`` after ``np.random.seed(s)`` the reference's own draw.  Returns ``(start, count)`` as Python ints (count in samples).
    Raises ``ValueError("No speaker activity found.")`` as the reference does when every window is empty."""
    w = weights_row.detach().cpu().numpy() if torch.is_tensor(weights_row) else np.asarray(weights_row)
    w = w.reshape(-1)
    weights = w.astype(np.float64) / float(BIN)                    # the reference's unit: 0.1 s bins of mean activity
    scaled = np.power(weights, skew_param)
    if np.all(weights == 0):
        raise ValueError("No speaker activity found.")
    probs = scaled / scaled.sum()
    start = int(rng.choice(np.arange(0, w.shape[0]), p=probs))
    return start, int(w[start])


class MeetingFrontEnd:
    """A recording and its diarization -> the keyword arguments of ``model.generate`` / ``LongFormDecoder.transcribe``, one row per target
    speaker.  ``prepare(wave, segs, targets=None)``: ``wave`` fp32 [n_samples] (or [1, n_samples]) on the GPU, ``segs`` a
    ``SpeakerSegments`` of the same length.  Returns

      * ``input_features`` [K, n_mels, 2 * T_total]: the recording's log-mel, computed once and shared by all K rows -- an expanded
        (stride-0) view when the recording is longer than one window, where the long-form loop copies every window it decodes; a real
        copy per row for a single window, which the one-pass decoder takes as it is;
      * ``attention_mask`` int32 [K, 2 * T_total]: ones on the ceil(n_samples / 160) frames that hold audio;
      * ``stno_mask`` fp32 [K, 4, T_total];
      * with ``use_enrollments``, ``enrollments`` = ``input_features`` [K, n_mels, 3000], ``stno_mask`` [K, 4, 1500], ``attention_mask``
        [K, 3000]: for each target the greedy self-enrollment window -- the wave slice ``[1600 * start, + 480000)``, zero-padded at the
        end, with a log-mel of its own (Whisper normalises per clip), and the slice ``[:, 5 * start : 5 * start + 1500]`` of the
        recording's STNO mask (the window starts on a frame boundary, so this is the mask the reference computes for the nested cut).

    Reading the chosen starts back to slice the wave is the one host synchronisation."""

    def __init__(self, n_mels, use_enrollments=False):
        self.n_mels, self.use_enrollments = int(n_mels), bool(use_enrollments)

    def prepare(self, wave, segs, targets=None):
        if not torch.is_tensor(wave) or not wave.is_cuda or wave.dtype != torch.float32:
            raise L.DicowError("MeetingFrontEnd: wave must be an fp32 tensor on the GPU (no CPU fallback)")
        wave = wave.reshape(-1)
        n = wave.numel()
        if n != segs.n_samples:
            raise L.DicowError(f"MeetingFrontEnd: the wave has {n} samples, the segments describe {segs.n_samples}")
        idx = segs.target_indices(targets)
        K, T, dev = len(idx), segs.T_total, wave.device
        padded = torch.zeros(1, T * FRAME, dtype=torch.float32, device=dev)
        padded[0, :n] = wave
        mel = features.log_mel(padded, self.n_mels)                                  # [1, M, 2 T]
        am = torch.zeros(1, 2 * T, dtype=torch.int32, device=dev)
        am[0, :-(-n // features.HOP)] = 1
        one_window = T == FRAMES_30S
        batch = {"input_features": mel.repeat(K, 1, 1) if one_window else mel.expand(K, -1, -1),
                 "attention_mask": am.expand(K, -1),
                 "stno_mask": stno_masks(segs, idx, device=dev)}
        if self.use_enrollments:
            start, _, _ = select_enrollment_windows(segs, idx, device=dev)
            starts = start.tolist()                                                  # the one synchronisation
            ew = torch.zeros(K, N_SAMPLES_30S, dtype=torch.float32, device=dev)
            eam = torch.zeros(K, 2 * FRAMES_30S, dtype=torch.int32, device=dev)
            est = torch.empty(K, 4, FRAMES_30S, dtype=torch.float32, device=dev)
            for k, s in enumerate(starts):
                got = min(N_SAMPLES_30S, n - BIN * s)
                ew[k, :got] = wave[BIN * s:BIN * s + got]
                eam[k, :-(-got // features.HOP)] = 1
                est[k] = batch["stno_mask"][k, :, 5 * s:5 * s + FRAMES_30S]
            batch["enrollments"] = {"input_features": features.log_mel(ew, self.n_mels), "stno_mask": est, "attention_mask": eam}
        return batch

"""External enrollment mixtures for SE-DiCoW training on the GPU: host planner + launches of csrc/enrollment_mix.hip.

Mirrors the second branch of the reference's ``get_conditioning_cut`` (src/data/local_datasets.py:438-450), taken when enrollment cutsets
are configured (``enrollment_cutsets``, ``number_of_mixed_speakers``, ``min/max_enrollment_mix_overlap``): ``generate_enrollment_mixture``
(:355-436) with ``sample_same_speaker_cut`` (:334-353), ``sample_offsets`` (:305-332) and ``mix_two_recordings`` (:294-303), and then the
nested ``cut_to_sample`` on the mixture -- its audio, and its STNO mask for the target speaker:

  * ``EnrollmentBank``              the utterances of the enrollment cutset, loaded once: 16 kHz mono, as loaded, resident on the device
  * ``plan_enrollment_mixtures``    the reference's draws (numpy's and Python's global generators) in its order -> a table of tracks
  * ``mix_enrollments``             ``dicow_enrollment_mix``: the shifted clips summed into zero-padded 30 s rows
  * ``enrollment_stno``             the tracks' supervision intervals, shifted and cut -> ``diar_front_end.stno_masks``, row by row
  * ``EnrollmentMixFrontEnd``       plan -> mix -> STNO for a batch dict that carries waves, then ``WaveFrontEnd``; ``TrainStep(front_end=...)``

Split of work as in ``wave_augment``: every random number is drawn on the host, so ``np.random.seed(s); random.seed(s)`` gives the
mixtures the reference's dataset would have cut; the plan is 16 bytes per track; the arithmetic runs in the kernel.

Three points rest on lhotse, which the reference calls and which could not be pinned while this was written (it was not installed):

  * **Seconds to samples.**  Offsets and lengths are drawn in seconds; a sample position is ``round(x * 16000)`` with Python's ``round``
    (half to even), as ``SpeakerSegments.from_seconds``.  lhotse's own rounding of a track offset may differ by one sample.
  * **``CutSet.sample()``** of an other speaker's clip is taken to be ``random.randrange(len(clips))`` from Python's ``random``.
  * **A negative target offset.**  The reference's "higher overlap is needed" clamp, ``max_enrollment_len - (cut.start + cut.duration)``,
    is negative when the chosen cut has ``start > 0`` and ends behind ``max_enrollment_len`` in its recording.  What lhotse's mixer does
    with it is not known here: ``plan_enrollment_mixtures`` raises ``ValueError`` instead of clipping silently.

No CPU fallback: mixing needs the bank and the output on the GPU.
"""
import pathlib
import random
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import augment, diar_front_end, features
from .wave_augment import WaveFrontEnd, _rows_aligned, read_pcm16

MAX_TRACKS = L.ENR_MIX_MAX_TRACKS            # include/dicow_hip.h DICOW_ENR_MIX_MAX_TRACKS
SAMPLE_RATE = 16000
N_SAMPLES_30S, FRAMES_30S = diar_front_end.N_SAMPLES_30S, diar_front_end.FRAMES_30S


class EnrollmentBank:
    """The utterances of the reference's ``enrollment_cutset``, kept on the device and laid out like ``NoiseBank``: one flat fp32 buffer
    ``data`` with clip k at ``data[clip_start[k] : clip_start[k] + clip_len[k]]`` (``clip_start`` int64 [n] and ``clip_len`` int32 [n] on the device;
    ``starts`` / ``lens`` are the host copies the planner, the wrapper's checks and the library's own plan check use).  The audio is stored as loaded: the reference mixes the cuts
    without normalising them.  Per clip k, on the host:

      * ``clip_speakers[k]``   its speakers, ``sorted`` as the reference's ``get_cut_spks`` orders them
      * ``recording_ids[k]``   ``cut.recording_id``, which ``sample_same_speaker_cut`` matches against the ids to skip
      * ``cut_start[k]``, ``durations[k]``   ``cut.start`` and ``cut.duration`` in seconds (defaults 0 and ``clip_len / 16000``)
      * ``supervisions[k]``    ``(speaker, start, end)`` in samples relative to the clip (default for a clip with one speaker: the whole clip)

    ``per_speaker`` maps a speaker to its clip indices in insertion order (the reference's ``per_speaker_enrollments``) and ``speakers``
    is that dict's key order (``enrollment_speakers``).  A bank built on the CPU can be planned against; mixing needs it on the GPU."""

    def __init__(self, data, starts, lens, speakers, recording_ids, cut_start=None, durations=None, supervisions=None):
        if data.dtype != torch.float32 or data.dim() != 1 or not data.is_contiguous():
            raise L.DicowError("EnrollmentBank: data must be a flat contiguous fp32 tensor")
        self.starts, self.lens = [int(s) for s in starts], [int(n) for n in lens]
        n = len(self.lens)
        if n == 0 or len(self.starts) != n or len(speakers) != n or len(recording_ids) != n:
            raise ValueError("EnrollmentBank: needs at least one clip, and a start, a speaker entry and a recording id per clip")
        for s, ln in zip(self.starts, self.lens):
            if s < 0 or ln < 1 or s + ln > data.numel() or ln >= 1 << 31:
                raise ValueError(f"EnrollmentBank: clip [{s}, {s} + {ln}) does not lie inside the {data.numel()} samples of the buffer")
        self.recording_ids = [str(r) for r in recording_ids]
        self.cut_start = [0.0] * n if cut_start is None else [float(x) for x in cut_start]
        self.durations = [ln / SAMPLE_RATE for ln in self.lens] if durations is None else [float(x) for x in durations]
        supervisions = [None] * n if supervisions is None else list(supervisions)
        if len(self.cut_start) != n or len(self.durations) != n or len(supervisions) != n:
            raise ValueError("EnrollmentBank: one cut start, one duration and one supervision list per clip")
        self.clip_speakers, self.supervisions = [], []
        for k in range(n):
            if not 0 < round(self.durations[k] * SAMPLE_RATE) <= self.lens[k]:
                raise ValueError(f"EnrollmentBank: the duration {self.durations[k]} s of clip {k} does not fit its {self.lens[k]} samples")
            spk = [speakers[k]] if isinstance(speakers[k], str) else list(speakers[k])
            if supervisions[k] is None:
                if len(spk) != 1:
                    raise ValueError(f"EnrollmentBank: clip {k} has {len(spk)} speakers and needs its supervision intervals")
                sup = [(spk[0], 0, self.lens[k])]
            else:
                sup = [(s, int(a), int(b)) for s, a, b in supervisions[k]]
                if any(a != a0 or b != b0 for (_, a, b), (_, a0, b0) in zip(sup, supervisions[k])):
                    raise ValueError(f"EnrollmentBank: the supervision intervals of clip {k} must be integer sample positions")
                if set(spk) != {s for s, _, _ in sup}:
                    raise ValueError(f"EnrollmentBank: the speakers of clip {k} are not the speakers of its supervisions")
            self.clip_speakers.append(sorted(set(spk)))
            self.supervisions.append(sup)
        self.per_speaker = {}
        for k, spk in enumerate(self.clip_speakers):
            for s in spk:
                self.per_speaker.setdefault(s, []).append(k)
        self.speakers = list(self.per_speaker)
        self.data = data
        self.clip_start = torch.tensor(self.starts, dtype=torch.int64).to(data.device)
        self.clip_len = torch.tensor(self.lens, dtype=torch.int32).to(data.device)
        self._clip_len_host = np.asarray(self.lens, dtype=np.int32)

    def __len__(self):
        return len(self.lens)

    @classmethod
    def from_tensors(cls, clips, speakers, recording_ids, cut_start=None, durations=None, supervisions=None, device="cuda") -> "EnrollmentBank":
        """clips: fp32 ``[n]`` or ``[1, n]`` CPU tensors, the audio of each cut in the enrollment cutset's order; ``speakers[k]`` a name or a
        list of names.  Stored back to back, so a clip starts wherever the one before it ended."""
        flat = []
        for k, c in enumerate(clips):
            c = torch.as_tensor(c, dtype=torch.float32).cpu()
            if c.dim() == 2 and c.shape[0] == 1:
                c = c[0]
            if c.dim() != 1 or c.numel() == 0:
                raise ValueError(f"EnrollmentBank: clip {k} must be mono, [n] or [1, n] with n > 0, got {tuple(c.shape)}")
            flat.append(c)
        if not flat:
            raise ValueError("EnrollmentBank: no clips")
        lens = [int(c.numel()) for c in flat]
        starts = [0]
        for n in lens[:-1]:
            starts.append(starts[-1] + n)
        return cls(torch.cat(flat).to(device), starts, lens, speakers, recording_ids, cut_start, durations, supervisions)

    @classmethod
    def from_dir(cls, enroll_dir, device="cuda", sample_rate: int = SAMPLE_RATE, speaker_of=None, recording_of=None,
                 resample: bool = False) -> "EnrollmentBank":
        """Every ``**/*.wav`` under enroll_dir in sorted order, one single-speaker clip each: the speaker is the name of the file's
        directory and the recording id the file's stem, unless ``speaker_of(path)`` / ``recording_of(path)`` say otherwise.  16-bit mono PCM
        at 16 kHz only, read as ``NoiseBank.from_dir`` reads (other rates and sample widths are refused) -- unless ``resample=True``: then a
        mono file at another rate is read as int16 and brought to ``sample_rate`` on the device (``wave_intake``, one launch per distinct
        rate).  The audio stays unnormalised either way."""
        root = pathlib.Path(enroll_dir)
        if not root.exists():
            raise IOError(f'Enrollment directory `{enroll_dir}` does not exist')
        files = sorted(root.glob('**/*.wav'))
        if len(files) == 0:
            raise IOError(f'No .wav file found in the enrollment directory `{enroll_dir}`')
        speaker_of = speaker_of or (lambda p: p.parent.name)
        recording_of = recording_of or (lambda p: p.stem)
        speakers, recordings = [speaker_of(f) for f in files], [recording_of(f) for f in files]
        if resample:
            bank = cls._from_files_resampled(files, speakers, recordings, device, sample_rate)
        else:
            bank = cls.from_tensors([read_pcm16(f, sample_rate, "EnrollmentBank") for f in files], speakers, recordings, device=device)
        bank.files = files
        return bank

    @classmethod
    def _from_files_resampled(cls, files, speakers, recordings, device, sample_rate):
        from . import wave_intake
        data, starts, lens, _ = wave_intake.bank_from_files(files, sample_rate, device, "EnrollmentBank", mono_only=True,
                                                           at_rate=lambda pcm: torch.from_numpy(pcm.numpy()[:, 0].astype(np.float32) / 32768.0))
        return cls(data, starts, lens, speakers, recordings)


# ------------------------------------------------------------------------------------------------------------------------ planner
def _mix_two_recordings(len_1, len_2, allowed_pause):
    """local_datasets.py:294-303."""
    rec2_offset = np.random.uniform(low=-len_1 - len_2 - allowed_pause, high=allowed_pause)
    if -rec2_offset <= len_1:
        return 0, len_1 + rec2_offset
    return -(len_1 + rec2_offset), 0


def _sample_offsets(target_duration, durations, overlap_factor, allowed_pause=2.0):
    """local_datasets.py:305-332: the others are chained pairwise in a drawn order; then the chain is placed against the target."""
    N = len(durations)
    duration_to_mix = target_duration * overlap_factor
    order = np.random.permutation(N)
    prev = durations[order[0]]
    offsets = np.zeros(N)
    for i in range(1, N):
        other = durations[order[i]]
        offset_1, offset_2 = _mix_two_recordings(prev, other, allowed_pause)
        offsets[:] += offset_1
        offsets[order[i]] = offset_2
        prev = max(offset_1 + prev, offset_2 + other)
    if prev < duration_to_mix:
        offset = np.random.uniform(low=0, high=target_duration - prev)
        return 0, offsets + offset
    if np.random.choice([-1, 1]) == 1:
        return prev - duration_to_mix, offsets
    return 0, offsets + (target_duration - duration_to_mix)


def _same_speaker_clip(bank, speaker_id, skip_ids, greedy_sample, max_duration):
    """local_datasets.py:334-353."""
    kept = [k for k in bank.per_speaker[speaker_id]
            if not any(bank.recording_ids[k] in skip_id for skip_id in skip_ids) and bank.durations[k] <= max_duration]
    if len(kept) == 0:
        raise ValueError(f"No valid enrollment cuts found for speaker {speaker_id} after skipping {skip_ids} (Max duration: {max_duration})")
    weights = np.array([bank.durations[k] for k in kept])
    if greedy_sample:
        return kept[int(np.argmax(weights))]
    return kept[int(np.random.choice(len(kept), p=weights / sum(weights)))]


def plan_enrollment_mixtures(bank, targets, skip_ids, *, num_other_speakers=2, min_overlap_ratio=0.3, max_overlap_ratio=1.0, greedy_sample=False,
                             max_enrollment_len=30.0, randomly_shift_target_offset_p=1.0):
    """The reference's ``generate_enrollment_mixture`` for consecutive rows, host only (no device access, no sync).

    ``targets[r]``: row r's target speaker, a key of ``bank.per_speaker`` (``KeyError`` otherwise, as the reference's dict raises).
    ``skip_ids[r]``: the recording ids a clip of the target must not come from, already cleaned -- the reference strips ``_vp.*$`` from
    the id of the row's cut, or of every track of a mixed cut, and then skips a clip whose ``recording_id`` is a SUBSTRING of one of them.

    Per row, in order: ``sample_same_speaker_cut`` (the filter by ``skip_ids`` and ``duration <= max_enrollment_len``; ``np.argmax`` of
    the durations when greedy, else ``np.random.choice(p=durations / sum)``); ``random.sample(bank.speakers, min(len, n + 1))`` minus
    the target, cut to ``num_other_speakers``; one clip per other speaker, ``random.randrange``; with others ``np.random.uniform(min,
    max)`` and ``sample_offsets`` (a permutation, one ``mix_two_recordings`` uniform per further clip, then a uniform or a choice of
    direction); unless greedy ``np.random.rand() < p`` and, if taken, the uniform shift of the target; the "higher overlap is needed"
    clamp; each track cut to ``max_enrollment_len`` and dropped at duration 0.

    Returns ``(tracks, track_offset_s, track_len_s, mix_len)``: ``tracks`` int32 [n, 4] = (row, clip, offset in samples, length in
    samples), the target's track first within a row; the float64 seconds behind the last two columns; ``mix_len`` int32 [B], the last
    sample any track of the row reaches (the mixture's ``wave_lengths``).

    Not pinned to lhotse (see the module docstring): a position in samples is ``round(seconds * 16000)``; ``CutSet.sample()`` is
    ``random.randrange``; a negative target offset raises ``ValueError``.  A length is further capped so that the rounded offset plus the
    rounded length stays within ``round(max_enrollment_len * 16000)``, and a track whose length rounds to no sample at all is left out.
    Raises ``ValueError`` as the reference does when no clip of the target survives the filter."""
    if len(targets) != len(skip_ids):
        raise ValueError(f"plan_enrollment_mixtures: {len(targets)} targets but {len(skip_ids)} skip lists")
    n_max = round(max_enrollment_len * SAMPLE_RATE)
    rows, off_s, len_s, mix_len = [], [], [], []
    for r, (speaker_id, skip) in enumerate(zip(targets, skip_ids)):
        skip = [skip] if isinstance(skip, str) else list(skip)
        same = _same_speaker_clip(bank, speaker_id, skip, greedy_sample, max_enrollment_len)
        same_dur = bank.durations[same]
        candidates = random.sample(bank.speakers, min(len(bank.speakers), num_other_speakers + 1))
        other_speakers = [s for s in candidates if s != speaker_id][:num_other_speakers]
        other_clips = []
        for s in other_speakers:
            clips = bank.per_speaker[s]
            other_clips.append(clips[random.randrange(len(clips))])
        other_lens = [bank.durations[k] for k in other_clips]
        if len(other_lens) > 0:
            overlap_factor = np.random.uniform(min_overlap_ratio, max_overlap_ratio)
            target_offset, other_offsets = _sample_offsets(same_dur, other_lens, overlap_factor)
        else:
            target_offset, other_offsets = 0.0, []
        if not greedy_sample and np.random.rand() < randomly_shift_target_offset_p:
            max_other_end = max([o + ln for o, ln in zip(other_offsets, other_lens)]) if other_lens else 0
            total_span = max(max_other_end, same_dur)
            target_offset = np.random.uniform(0, max(0, total_span - same_dur))
        if bank.cut_start[same] + target_offset + same_dur > max_enrollment_len:
            target_offset = max_enrollment_len - (bank.cut_start[same] + same_dur)          # "higher overlap is needed"
        if target_offset < 0:
            raise ValueError(f"plan_enrollment_mixtures: row {r}: the reference's clamp gives clip {same} (start {bank.cut_start[same]} s, "
                             f"duration {same_dur} s) the negative offset {target_offset} s")
        reach = 0
        for clip, offset in zip([same] + other_clips, [target_offset] + list(other_offsets)):
            dur, offset = bank.durations[clip], float(offset)
            if dur + offset > max_enrollment_len:
                dur = max(max_enrollment_len - offset, 0)
            if not dur > 0.0:
                continue
            o = round(offset * SAMPLE_RATE)
            ln = min(round(dur * SAMPLE_RATE), n_max - o)
            if ln < 1:
                continue
            rows.append((r, clip, o, ln))
            off_s.append(offset)
            len_s.append(float(dur))
            reach = max(reach, o + ln)
        mix_len.append(reach)
    return (torch.tensor(rows, dtype=torch.int32).reshape(-1, 4), np.asarray(off_s, dtype=np.float64), np.asarray(len_s, dtype=np.float64),
            torch.tensor(mix_len, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ device side
def _host_tracks(tracks) -> torch.Tensor:
    return torch.as_tensor(tracks, dtype=torch.int32).cpu().reshape(-1, 4).contiguous()


def mix_enrollments(bank: EnrollmentBank, tracks, B: int, n: int = N_SAMPLES_30S, out: Optional[torch.Tensor] = None,
                    plan_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``tracks`` int32 [n_tracks, 4] from ``plan_enrollment_mixtures`` (a host tensor; rows non-decreasing) -> fp32 ``[B, n]`` on the
    bank's GPU: every row the sum of its tracks in plan order, zero where no track reaches -- all ``n`` samples of all ``B`` rows are
    written.  ``out``: a tensor of that shape to fill, unit stride along a row and rows that start on 16-byte boundaries (a view into
    longer rows is fine; nothing outside it is written).  ``plan_dev``: an int32 [n_tracks, 4] tensor on the GPU that already holds the
    same table, for callers that capture the launch into a graph and rewrite the table in place between replays; by default the table
    goes up through the pinned staging slots."""
    if not isinstance(bank, EnrollmentBank) or not bank.data.is_cuda:
        raise L.DicowError("mix_enrollments: the bank must be an EnrollmentBank on the GPU (no CPU fallback)")
    dev = bank.data.device
    B, n = int(B), int(n)
    if B < 0 or n < 0:
        raise L.DicowError(f"mix_enrollments: negative size B={B} n={n}")
    tracks = _host_tracks(tracks)
    n_tracks = tracks.shape[0]
    per_row, prev = {}, 0
    for k, (row, clip, off, ln) in enumerate(tracks.tolist()):
        if not 0 <= row < B:
            raise L.DicowError(f"mix_enrollments: track {k} names row {row} outside the batch of {B}")
        if row < prev:
            raise L.DicowError(f"mix_enrollments: track {k} names row {row} behind row {prev}: the tracks of a row must be consecutive")
        prev = row
        per_row[row] = per_row.get(row, 0) + 1
        if per_row[row] > MAX_TRACKS:
            raise L.DicowError(f"mix_enrollments: row {row} has more than {MAX_TRACKS} tracks")
        if not 0 <= clip < len(bank):
            raise L.DicowError(f"mix_enrollments: clip {clip} outside the bank of {len(bank)}")
        if off < 0:
            raise L.DicowError(f"mix_enrollments: track {k} has the negative offset {off}")
        if not 1 <= ln <= bank.lens[clip]:
            raise L.DicowError(f"mix_enrollments: len {ln} of track {k} outside [1, {bank.lens[clip]}], the length of clip {clip}")
        if off + ln > n:
            raise L.DicowError(f"mix_enrollments: track {k} ends at sample {off + ln}, behind the row's {n}")
    if out is None:
        out = torch.empty(B, (n + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :n]
    else:
        if not torch.is_tensor(out) or not out.is_cuda:
            raise L.DicowError("mix_enrollments: out must be on the GPU (no CPU fallback)")
        if out.dtype != torch.float32 or tuple(out.shape) != (B, n) or out.device != dev:
            raise L.DicowError(f"mix_enrollments: out must be fp32 {(B, n)} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if B > 0 and n > 0 and not (_rows_aligned(out) if B > 1 else out.stride(1) == 1 and out.data_ptr() % 16 == 0):
            raise L.DicowError("mix_enrollments: out needs unit-stride rows that start on 16-byte boundaries")
    if B == 0 or n == 0:
        return out
    if plan_dev is None:
        plan_dev = augment._up(tracks.reshape(-1), dev) if n_tracks else None
    elif (not torch.is_tensor(plan_dev) or plan_dev.device != dev or plan_dev.dtype != torch.int32 or plan_dev.numel() != 4 * n_tracks
          or not plan_dev.is_contiguous()):
        raise L.DicowError(f"mix_enrollments: plan_dev must be a contiguous int32 [{n_tracks}, 4] tensor on {dev}")
    ld = out.stride(0) if B > 1 else n + (-n) % 4                           # (a single row: its stride is never used)
    with torch.cuda.device(dev):
        L.call("dicow_enrollment_mix", out.data_ptr(), ld, B, n, bank.data.data_ptr(), bank.clip_start.data_ptr(), L.ptr(plan_dev),
               tracks.data_ptr() if n_tracks else None, n_tracks, bank._clip_len_host.ctypes.data, len(bank), L.stream())
    return out


def track_intervals(bank: EnrollmentBank, tracks, row: int):
    """Speaker -> half-open sample intervals of the mixture of ``row``: every supervision interval of every track's clip, clipped to the
    track's (cut) length and shifted by the track's offset.  A speaker whose intervals are all cut away keeps its (empty) entry, as the
    cut the reference builds keeps the clip's supervisions."""
    out = {}
    for r, clip, off, ln in _host_tracks(tracks).tolist():
        if r != row:
            continue
        for spk, a, b in bank.supervisions[clip]:
            a, b = max(0, a), min(ln, b)
            out.setdefault(spk, [])
            if a < b:
                out[spk].append((off + a, off + b))
    return out


def enrollment_stno(bank: EnrollmentBank, tracks, targets, mix_len, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """fp32 ``[B, 4, 1500]`` on the device: for every row the reference's ``get_stno_mask`` of the mixed cut for ``targets[row]`` -- the
    mixture's speakers ``sorted``, its supervisions the tracks' own, shifted by the track offsets and cut with the tracks, the mask
    rasterised over ``mix_len[row]`` samples and padded to 30 s.  A target that does not occur in the row's mixture raises ``KeyError``
    (the reference's ``speakers_to_idx[speaker_id]``); "-1" is the unknown speaker.  One ``stno_masks`` call, two small launches, per row."""
    tracks = _host_tracks(tracks)
    mix_len = mix_len.tolist() if torch.is_tensor(mix_len) else [int(x) for x in mix_len]
    B = len(targets)
    if len(mix_len) != B:
        raise ValueError(f"enrollment_stno: {B} targets but {len(mix_len)} mixture lengths")
    if out is None:
        out = torch.empty(B, 4, FRAMES_30S, dtype=torch.float32, device=bank.data.device if device is None else device)
    elif tuple(out.shape) != (B, 4, FRAMES_30S):
        raise L.DicowError(f"enrollment_stno: out must have the shape {(B, 4, FRAMES_30S)}")
    for r in range(B):
        if not 1 <= mix_len[r] <= N_SAMPLES_30S:
            raise ValueError(f"enrollment_stno: row {r}: a mixture of {mix_len[r]} samples (one window of at most 30 s is expected)")
        segs = diar_front_end.SpeakerSegments(track_intervals(bank, tracks, r), mix_len[r])
        diar_front_end.stno_masks(segs, [targets[r]], out=out[r:r + 1])
    return out


class EnrollmentMixFrontEnd:
    """SE-DiCoW's external enrollments built on the GPU, ahead of ``WaveFrontEnd``: ``TrainStep(front_end=EnrollmentMixFrontEnd(...))``.

    ``__call__(batch)``: a batch that carries ``input_waves`` (fp32 [B, n] on the GPU), ``target_speakers`` (B names) and
    ``skip_recordings`` (B lists of cleaned recording ids, see ``plan_enrollment_mixtures``) gains ``batch["enrollments"] =
    {"input_waves" [B, 480000], "wave_lengths", "stno_mask" [B, 4, 1500], "attention_mask" int32 [B, 3000]}`` -- the attention mask with
    ones on the ceil(length / 160) frames that hold audio, as ``MeetingFrontEnd`` builds it -- and loses the two host keys.  The batch is
    then handed to ``wave_front_end`` (default: a plain ``WaveFrontEnd(n_mels)``), which turns both ``input_waves`` into
    ``input_features``; give one with a ``NoiseBank`` to mix MUSAN into rows and enrollments as before.  Any other batch goes to
    ``wave_front_end`` untouched.

    With both on, the two planners consume Python's ``random`` in another interleaving than the reference's dataset does (there: per
    sample the row's MUSAN draws, the mixture's draws, the enrollment's MUSAN draws; here: the mixtures of all rows, then MUSAN for row
    0, enrollment 0, row 1, ...).  Each planner's own sequence of draws is the reference's from the generator state it starts from."""

    def __init__(self, bank: EnrollmentBank, n_mels: int, wave_front_end=None, **plan_options):
        self.bank, self.n_mels = bank, int(n_mels)
        self.wave_front_end = WaveFrontEnd(self.n_mels) if wave_front_end is None else wave_front_end
        plan_enrollment_mixtures(bank, [], [], **plan_options)              # (refuses an option the planner does not know)
        if round(plan_options.get("max_enrollment_len", 30.0) * SAMPLE_RATE) > N_SAMPLES_30S:
            raise ValueError("EnrollmentMixFrontEnd: max_enrollment_len above 30 s does not fit the model's one-window enrollment")
        self.plan_options = plan_options

    def __call__(self, batch: dict) -> dict:
        if not all(k in batch for k in ("input_waves", "target_speakers", "skip_recordings")):
            return self.wave_front_end(batch)
        batch = dict(batch)
        targets, skip = list(batch.pop("target_speakers")), list(batch.pop("skip_recordings"))
        B = batch["input_waves"].shape[0]
        if len(targets) != B or len(skip) != B:
            raise L.DicowError(f"EnrollmentMixFrontEnd: {len(targets)} target speakers and {len(skip)} skip lists for {B} waves")
        tracks, _, _, mix_len = plan_enrollment_mixtures(self.bank, targets, skip, **self.plan_options)
        waves = mix_enrollments(self.bank, tracks, B, N_SAMPLES_30S)
        am = torch.zeros(B, 2 * FRAMES_30S, dtype=torch.int32)
        for r, ln in enumerate(mix_len.tolist()):
            am[r, :-(-ln // features.HOP)] = 1
        batch["enrollments"] = {"input_waves": waves, "wave_lengths": mix_len.tolist(),
                                "stno_mask": enrollment_stno(self.bank, tracks, targets, mix_len),
                                "attention_mask": am.to(waves.device)}
        return self.wave_front_end(batch)

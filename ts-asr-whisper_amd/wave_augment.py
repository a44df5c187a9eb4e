"""Waveform-level augmentation on the GPU, ahead of the log-mel front end: host planner + launches of csrc/noise_mix.hip.

Mirrors the reference's ``RandomBackgroundNoise`` (src/data/augmentations.py:382-429), the MUSAN augmentation the dataset applies to a
sample's waveform with probability ``musan_augment_prob`` before feature extraction (src/data/local_datasets.py:205-206), for batches
whose 16 kHz waveforms already live in HBM (``features.log_mel``):

  * ``NoiseBank``                 the reference's ``noise_files_list``, loaded once: mono, peak-normalised, resident on the device
  * ``plan_background_noise``     the reference's draws (gate, clip, offset, SNR) with the reference's generators, in its order
  * ``mix_background_noise``      ``dicow_noise_mix`` on the planned rows
  * ``WaveFrontEnd``              plan -> mix -> ``features.log_mel`` for a batch dict that carries waves; ``trainer.TrainStep(front_end=...)``

Split of work as in ``augment``: every random number is drawn on the host -- the gate from the global torch CPU generator, the rest from
Python's ``random`` module, as the reference does -- so ``torch.manual_seed(s); random.seed(s)`` gives the waveforms the reference's dataset
would have produced; the plan is a few bytes per row and goes up through the pinned staging slots; the arithmetic runs in the kernel.

Two stated deviations from the reference: a crop of the clip that is all zeros leaves ``audio / 2`` (the reference divides by the crop's
zero norm and returns NaN on every sample), and ``NoiseBank.from_dir`` refuses a clip at another sample rate unless it is told to
resample (``resample=True``, ``wave_intake``; the reference always resamples, and MUSAN is distributed at 16 kHz).  No CPU fallback:
waveforms must be on the GPU.
"""
import os
import pathlib
import random
import wave as _wave
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import augment, features, ops

NOISE_MIX_CHUNK = L.NOISE_MIX_CHUNK      # include/dicow_hip.h DICOW_NOISE_MIX_CHUNK: samples per partial sum (rows up to 64 chunks)


def _prepare_clip(noise: torch.Tensor) -> torch.Tensor:
    """augmentations.py:401-410 with the reference's torch ops on the host (bit-equal values): mono mean, peak normalisation -> fp32 [n]."""
    noise = torch.as_tensor(noise, dtype=torch.float32).cpu()
    if noise.dim() == 1:
        noise = noise[None]
    if noise.dim() != 2 or noise.shape[-1] == 0:
        raise ValueError(f"NoiseBank: a clip must be [C, n] or [n] with n > 0, got {tuple(noise.shape)}")
    if noise.shape[0] > 1:
        noise = torch.mean(noise, dim=0, keepdim=True)
    peak = torch.max(torch.abs(noise))
    if not float(peak) > 0.0:
        raise ValueError("NoiseBank: a clip is all zeros (or NaN): the reference would divide by its zero peak")
    return (noise / peak)[0]


def read_pcm16(path, sample_rate: int = 16000, who: str = "NoiseBank") -> torch.Tensor:
    """A 16-bit PCM WAV file -> fp32 ``[C, n]``, read with the standard library and scaled by 1 / 32768 as ``torchaudio.load`` normalises.
    Another sample width or another rate is refused (no resampling here)."""
    with _wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"{who}: {path} has {8 * w.getsampwidth()}-bit samples; only 16-bit PCM is read")
        if w.getframerate() != sample_rate:
            raise ValueError(f"{who}: {path} is sampled at {w.getframerate()} Hz, not {sample_rate} Hz; resample the files "
                             "first (this loader does not resample)")
        ch = w.getnchannels()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return torch.from_numpy(pcm.astype(np.float32) / 32768.0).reshape(-1, ch).t().contiguous()


class NoiseBank:
    """The noise clips of the reference's ``noise_files_list``, prepared once and kept on the device: one flat fp32 buffer ``data`` with
    clip k at ``data[clip_start[k] : clip_start[k] + clip_len[k]]`` (``clip_start`` int64 [n], ``clip_len`` int32 [n], both on the device;
    ``starts`` / ``lens`` are their host copies, which the planner and the wrapper's checks use without touching the device).  A bank
    built on the CPU can be planned against and inspected; mixing needs it on the waves' GPU.

    Size: 4 bytes per sample at 16 kHz = 230 MB per hour -- MUSAN's 6 h ``noise`` subset is about 1.4 GB, all 109 h about 25 GB."""

    def __init__(self, data: torch.Tensor, starts: Sequence[int], lens: Sequence[int]):
        if data.dtype != torch.float32 or data.dim() != 1 or not data.is_contiguous():
            raise L.DicowError("NoiseBank: data must be a flat contiguous fp32 tensor")
        self.starts, self.lens = [int(s) for s in starts], [int(n) for n in lens]
        if not self.lens or len(self.starts) != len(self.lens):
            raise ValueError("NoiseBank: needs at least one clip, and one start per length")
        for s, n in zip(self.starts, self.lens):
            if s < 0 or n < 1 or s + n > data.numel() or n >= 1 << 31:
                raise ValueError(f"NoiseBank: clip [{s}, {s} + {n}) does not lie inside the {data.numel()} samples of the buffer")
        self.data = data
        self.clip_start = torch.tensor(self.starts, dtype=torch.int64).to(data.device)
        self.clip_len = torch.tensor(self.lens, dtype=torch.int32).to(data.device)

    def __len__(self):
        return len(self.lens)

    @classmethod
    def from_tensors(cls, clips, device="cuda") -> "NoiseBank":
        """clips: fp32 ``[C, n]`` or ``[n]`` CPU tensors, what ``torchaudio.load`` returns for each file; their order is the order
        ``random.choice`` indexes.  Stored back to back, so a clip starts wherever the one before it ended."""
        prepared = [_prepare_clip(c) for c in clips]
        if not prepared:
            raise ValueError("NoiseBank: no clips")
        lens = [int(p.numel()) for p in prepared]
        starts = [0]
        for n in lens[:-1]:
            starts.append(starts[-1] + n)
        return cls(torch.cat(prepared).to(device), starts, lens)

    @classmethod
    def from_dir(cls, noise_dir, device="cuda", sample_rate: int = 16000, resample: bool = False) -> "NoiseBank":
        """Every ``**/*.wav`` under noise_dir, in the order ``pathlib.Path(noise_dir).glob('**/*.wav')`` lists them in this call (the list
        the reference builds, augmentations.py:388-393).  16-bit PCM only, read with the standard library and scaled by 1 / 32768 as
        ``torchaudio.load`` normalises; a file at another rate is refused (no resampling here) unless ``resample=True``: then it is read as
        int16 and brought to ``sample_rate`` on the device (``wave_intake``: one launch per distinct rate and channel count) in the
        reference's order, augmentations.py:401-410 -- mono mean, resample, division by the peak of the resampled clip.  Files that
        already are at ``sample_rate`` are prepared as before, bit for bit."""
        if not os.path.exists(noise_dir):
            raise IOError(f'Noise directory `{noise_dir}` does not exist')
        files = list(pathlib.Path(noise_dir).glob('**/*.wav'))
        if len(files) == 0:
            raise IOError(f'No .wav file found in the noise directory `{noise_dir}`')
        if resample:
            bank = cls._from_files_resampled(files, device, sample_rate)
        else:
            bank = cls.from_tensors([read_pcm16(f, sample_rate, "NoiseBank") for f in files], device)
        bank.files = files
        return bank

    @classmethod
    def _from_files_resampled(cls, files, device, sample_rate):
        from . import wave_intake
        data, starts, lens, foreign = wave_intake.bank_from_files(
            files, sample_rate, device, "NoiseBank",
            lambda pcm: _prepare_clip(torch.from_numpy(pcm.numpy().astype(np.float32) / 32768.0).t().contiguous()))
        for k in foreign:                                                  # (the clips at sample_rate are normalised already)
            clip = data[starts[k]:starts[k] + lens[k]]
            peak = torch.max(torch.abs(clip))
            if not float(peak) > 0.0:
                raise ValueError(f"NoiseBank: {files[k]} is all zeros (or NaN): the reference would divide by its zero peak")
            clip.div_(peak)
        return cls(data, starts, lens)


def plan_background_noise(lengths, bank, prob: float, min_snr_db: int = 0, max_snr_db: int = 15):
    """The reference's draws for consecutive samples of ``lengths[k]`` audio samples each, host only (no device access, no sync).

    Per entry, in order: the gate ``torch.rand(1).item() < prob`` from the global torch CPU generator, drawn only if ``prob > 0``
    (local_datasets.py:205); for a selected entry, from Python's ``random``: ``random.choice`` over the clips, ``random.randint(0,
    clip_len - len)`` only if the clip is longer than the audio, ``random.randint(min_snr_db, max_snr_db)`` (augmentations.py:396-423).
    Returns ``plan_i`` int32 [n, 4] = (index into ``lengths``, clip, offset, len) and ``plan_snr`` fp32 [n] = float32(10 ** (snr_db / 10)),
    empty when nothing is selected.  An entry of length 0 makes its draws and is left out of the plan.

    SE-DiCoW: the reference's ``cut_to_sample`` calls ``get_features`` for a row and then for its nested enrollment, so the dataset's
    order of draws is row 0, enrollment 0, row 1, enrollment 1, ...: pass the lengths interleaved like that (``WaveFrontEnd`` does)."""
    lens = bank.lens if isinstance(bank, NoiseBank) else [int(n) for n in bank]
    rows, snr = [], []
    for k, ln in enumerate(lengths):
        ln = int(ln)
        if not (prob > 0.0 and torch.rand(1).item() < prob):
            continue
        clip = random.choice(range(len(lens)))
        off = random.randint(0, lens[clip] - ln) if lens[clip] > ln else 0
        snr_db = random.randint(min_snr_db, max_snr_db)
        if ln > 0:
            rows.append((k, clip, off, ln))
            snr.append(10 ** (snr_db / 10))
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4), torch.tensor(snr, dtype=torch.float64).to(torch.float32)


def _rows_aligned(t: torch.Tensor) -> bool:
    return t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0


def _aligned_copy(t: torch.Tensor) -> torch.Tensor:
    """A copy of t [B, n] whose rows start on 16-byte boundaries (a view of a [B, n rounded up to 4] allocation when n % 4 != 0)."""
    B, n = t.shape
    out = torch.empty(B, (n + 3) // 4 * 4, dtype=t.dtype, device=t.device)[:, :n]
    out.copy_(t)
    return out


def mix_background_noise(wave: torch.Tensor, bank: NoiseBank, plan_i: torch.Tensor, plan_snr: torch.Tensor,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wave fp32 [B, n] on the GPU; plan_i / plan_snr from ``plan_background_noise`` (host tensors, the first column = the row).
    Returns a new tensor -- a copy of ``wave`` in which the planned rows hold ``(a + scale * noise) / 2`` on their first ``len`` samples --
    or works in place when ``out is wave``.  Rows that are not planned and samples at or behind ``len`` keep their bits."""
    for t, name in ((wave, "wave"),) + (((out, "out"),) if out is not None else ()):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.DicowError(f"mix_background_noise: {name} must be on the GPU (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise L.DicowError(f"mix_background_noise: {name} must be fp32 [B, n], got {t.dtype} {tuple(t.shape)}")
    B, n = wave.shape
    plan_i = torch.as_tensor(plan_i, dtype=torch.int32).cpu().reshape(-1, 4)
    plan_snr = torch.as_tensor(plan_snr, dtype=torch.float32).cpu().reshape(-1)
    n_plan = plan_i.shape[0]
    if plan_snr.numel() != n_plan:
        raise L.DicowError(f"mix_background_noise: {n_plan} plan rows but {plan_snr.numel()} SNR values")
    seen = set()
    for row, clip, off, ln in plan_i.tolist():
        if not 0 <= row < B:
            raise L.DicowError(f"mix_background_noise: row {row} outside the batch of {B}")
        if row in seen:
            raise L.DicowError(f"mix_background_noise: row {row} is planned twice")
        seen.add(row)
        if not 1 <= ln <= n:
            raise L.DicowError(f"mix_background_noise: len {ln} of row {row} outside [1, {n}]")
        if not 0 <= clip < len(bank):
            raise L.DicowError(f"mix_background_noise: clip {clip} outside the bank of {len(bank)}")
        if not 0 <= off < bank.lens[clip]:
            raise L.DicowError(f"mix_background_noise: offset {off} lies behind clip {clip} of {bank.lens[clip]} samples")
    if bank.data.device != wave.device:
        raise L.DicowError(f"mix_background_noise: the bank is on {bank.data.device}, the waves on {wave.device}")
    if out is None:
        out = wave.clone() if _rows_aligned(wave) and wave.is_contiguous() else _aligned_copy(wave)
        src = wave if _rows_aligned(wave) else out
    elif out is wave:
        if not _rows_aligned(wave):
            raise L.DicowError("mix_background_noise: in place needs unit-stride rows that start on 16-byte boundaries")
        src = wave
    else:
        if out.shape != wave.shape or out.device != wave.device or not _rows_aligned(out):
            raise L.DicowError("mix_background_noise: out must match wave, with unit-stride rows that start on 16-byte boundaries")
        lo_w, lo_o = wave.data_ptr(), out.data_ptr()
        hi_w, hi_o = lo_w + 4 * ((B - 1) * wave.stride(0) + n), lo_o + 4 * ((B - 1) * out.stride(0) + n)
        if lo_w < hi_o and lo_o < hi_w:
            raise L.DicowError("mix_background_noise: out overlaps wave (only out is wave is allowed)")
        out.copy_(wave)
        src = wave if _rows_aligned(wave) else out
    if n_plan == 0:
        return out
    dev = wave.device
    # one upload for both halves of the plan: [n, 4] int32, then the n SNR values' bits
    plan = augment._up(torch.cat([plan_i.reshape(-1), plan_snr.view(torch.int32)]), dev)
    nbytes = L.lib().dicow_noise_mix_ws_bytes(n_plan, int(plan_i[:, 3].max()))
    ws = ops.workspace(nbytes, dev)
    L.call("dicow_noise_mix", src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0), bank.data.data_ptr(), bank.clip_start.data_ptr(),
           bank.clip_len.data_ptr(), plan.data_ptr(), plan.data_ptr() + 16 * n_plan, n_plan, ws.data_ptr(), nbytes, L.stream())
    return out


class WaveFrontEnd:
    """Waveforms in HBM -> ``input_features``: background noise on the selected rows (the reference dataset's
    ``musan_augment_prob`` / ``RandomBackgroundNoise(16000, musan_root)``), then ``features.log_mel``.

    ``__call__(batch)``: ``batch["input_waves"]`` fp32 [B, n] on the GPU, padded as ``features.pad_to_30s`` does, and
    ``batch["wave_lengths"]``, the B unpadded lengths as host ints, become ``batch["input_features"]``; both wave keys are removed.  A
    ``batch["enrollments"]`` dict that carries the two keys is treated the same way, and the draws then alternate row, enrollment, row,
    enrollment, as the reference's dataset makes them.  Build the dataset itself with ``musan_augment_prob=0``."""

    def __init__(self, n_mels: int, bank: Optional[NoiseBank] = None, musan_augment_prob: float = 0.0, min_snr_db: int = 0,
                 max_snr_db: int = 15):
        if musan_augment_prob > 0.0 and bank is None:
            raise ValueError("WaveFrontEnd: musan_augment_prob > 0 needs a NoiseBank")
        self.n_mels, self.bank, self.musan_augment_prob = n_mels, bank, float(musan_augment_prob)
        self.min_snr_db, self.max_snr_db = min_snr_db, max_snr_db

    @staticmethod
    def _lengths(d) -> List[int]:
        ln = d["wave_lengths"]
        ln = ln.tolist() if torch.is_tensor(ln) else list(ln)
        if len(ln) != d["input_waves"].shape[0]:
            raise L.DicowError(f"WaveFrontEnd: {len(ln)} wave_lengths for {d['input_waves'].shape[0]} waves")
        return [int(x) for x in ln]

    def __call__(self, batch: dict) -> dict:
        sides = [batch]
        enr = batch.get("enrollments")
        if isinstance(enr, dict) and "input_waves" in enr:
            enr = batch["enrollments"] = dict(enr)
            sides.append(enr)
        waves = [s["input_waves"] for s in sides]
        if self.musan_augment_prob > 0.0:
            lens = [self._lengths(s) for s in sides]
            if len(sides) == 2 and len(lens[0]) != len(lens[1]):
                raise L.DicowError("WaveFrontEnd: the enrollments must hold one wave per row")
            order = [ln for pair in zip(*lens) for ln in pair]              # row 0, enrollment 0, row 1, enrollment 1, ...
            plan_i, plan_snr = plan_background_noise(order, self.bank, self.musan_augment_prob, self.min_snr_db, self.max_snr_db)
            for k, w in enumerate(waves):
                mine = plan_i[:, 0] % len(sides) == k
                pi = plan_i[mine].clone()
                pi[:, 0] //= len(sides)
                if pi.shape[0]:
                    waves[k] = mix_background_noise(w, self.bank, pi, plan_snr[mine])
        for s, w in zip(sides, waves):
            s["input_features"] = features.log_mel(w, self.n_mels)
            del s["input_waves"]
            s.pop("wave_lengths", None)
        return batch

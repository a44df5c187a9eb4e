"""What the noise-mixing tests share: the inputs of golden F23 (regenerated on both sides from integer hashes), an fp64 restatement of
the reference's RandomBackgroundNoise.__call__ (src/data/augmentations.py:395-429) that the GPU tests use as their oracle --
tests/test_host_noise_mix.py pins it to F23, which the reference's own class produced --, the same arithmetic in fp32 with torch (the
reference's own rounding, for cases without a golden), and a replay of the reference's draw order.  Plain torch on the CPU."""
import random

import numpy as np
import torch

from tests.util import hashed_uniform, load_golden, subsample, T

SPEECH_AMP, NOISE_AMP = 0.1, 0.3
FULL_OUT_MAX = 20000            # F23 stores the reference's output in full up to this many samples, else util.subsample(out, 4096)

# name -> (audio samples, clip channels, clip samples, leading zero samples of the clip, seed of Python's random)
F23_CASES = {
    "long_stereo": (480000, 2, 600001, 0, 2301),     # clip longer than 30 s of audio: mono mean + an offset drawn
    "zero_tail": (123457, 1, 1000, 0, 2302),         # clip shorter than the audio: zero padding behind it, no offset drawn
    "three": (3, 1, 50, 0, 2303),
    "equal": (900, 1, 900, 0, 2304),                 # equal lengths: no offset drawn
    "zero_head": (5000, 1, 9000, 4000, 2305),        # the clip starts with 4000 zeros; any offset in [0, 4000] keeps a non-zero part
}

# the planner sequence: 64 consecutive samples at prob 0.3 after torch.manual_seed(23); random.seed(23)
SEQ_SEED, SEQ_PROB, SEQ_N = 23, 0.3, 64
SEQ_CLIP_LENS = (1000, 16000, 48000, 900, 5000, 123, 30000)
SEQ_AUDIO_LENS = (16000, 900, 48000, 3, 20000, 480, 30000, 5000, 100000)     # 900, 5000, 16000, 30000, 48000 equal a clip's length


def seq_lengths():
    return [SEQ_AUDIO_LENS[(5 * k + k // 9) % len(SEQ_AUDIO_LENS)] for k in range(SEQ_N)]


def f23_inputs(name):
    """(audio fp32 [len], raw clip fp32 [C, clen]) of an F23 case: what the dataset hands to the augmentation and what
    torchaudio.load returns for the noise file."""
    ln, ch, clen, zero_head, _ = F23_CASES[name]
    audio = hashed_uniform(f"f23.{name}.audio", (ln,)) * SPEECH_AMP
    clip = hashed_uniform(f"f23.{name}.clip", (ch, clen)) * NOISE_AMP
    clip[:, :zero_head] = 0.0
    return audio, clip


def prepare_clip(raw):
    """augmentations.py:401-410 with the reference's torch ops: mono mean, peak normalisation -> fp32 [clen]."""
    raw = raw if raw.dim() == 2 else raw[None]
    if raw.shape[0] > 1:
        raw = torch.mean(raw, dim=0, keepdim=True)
    return (raw / torch.max(torch.abs(raw)))[0]


def crop(clip, off, ln):
    """n[i] = clip[off + i] while off + i < clen, else 0 (augmentations.py:416-420); same dtype as clip."""
    n = torch.zeros(ln, dtype=clip.dtype)
    take = max(0, min(ln, clip.numel() - off))
    n[:take] = clip[off:off + take]
    return n


def snr_f32(snr_db):
    """float32(10 ** (snr_db / 10)): torch multiplies an fp32 tensor by the Python double in fp32."""
    return float(np.float32(10 ** (snr_db / 10)))


def mix_restatement64(audio, clip, off, snr_db):
    """The mix in fp64 (snr keeps its fp32 cast) on the fp32 inputs; a crop of norm 0 gives audio / 2 (the product's stated deviation:
    the reference returns NaN there)."""
    a, n = audio.double(), crop(clip.double(), off, audio.numel())
    na, nn = a.square().sum().sqrt(), n.square().sum().sqrt()
    scale = 0.0 if float(nn) == 0.0 else na / (snr_f32(snr_db) * nn)
    return (a + scale * n) / 2


def mix_reference32(audio, clip, off, snr_db):
    """augmentations.py:422-429 operation for operation in fp32 with torch on the CPU (the reference's own rounding); a crop of norm 0
    gives audio / 2 as in the restatement."""
    n = crop(clip, off, audio.numel())
    snr = 10 ** (snr_db / 10)
    audio_power, noise_power = audio.norm(p=2), n.norm(p=2)
    if float(noise_power) == 0.0:
        return audio / 2
    noise_scale = audio_power / (snr * noise_power)
    return (audio + noise_scale * n) / 2


def replay_draws(lengths, clip_lens, prob, min_snr_db=0, max_snr_db=15):
    """The reference's draws for consecutive samples (local_datasets.py:205-206 gate, then augmentations.py:396, 417, 423), from the
    global generators: a list of (index, clip, offset or -1 when none is drawn, snr_db) for the gated samples."""
    out = []
    for k, ln in enumerate(lengths):
        if prob > 0.0 and torch.rand(1).item() < prob:
            clip = random.choice(list(range(len(clip_lens))))
            off = random.randint(0, clip_lens[clip] - ln) if clip_lens[clip] > ln else -1
            out.append((k, clip, off, random.randint(min_snr_db, max_snr_db)))
    return out


def f23_case(z, name):
    """(audio, prepared clip, offset (0 when none was drawn), snr_db, o64, ref32 as stored, index selecting the stored samples of a
    full output) of an F23 case."""
    audio, raw = f23_inputs(name)
    clip = prepare_clip(raw)
    off, db = int(z[name + ".offset"]), int(z[name + ".snr_db"])
    o64 = mix_restatement64(audio, clip, max(off, 0), db)
    full = audio.numel() <= FULL_OUT_MAX
    pick = (lambda t: t) if full else (lambda t: subsample(t, 4096))
    return audio, clip, max(off, 0), db, o64, T(z, name + ".out"), pick


def e_ref_of(z, name):
    """max |reference fp32 - restatement fp64| over the stored samples of an F23 case, and max |restatement| over the whole output."""
    _, _, _, _, o64, ref32, pick = f23_case(z, name)
    return float((ref32.double() - pick(o64)).abs().max()), float(o64.abs().max())


def load_f23():
    return load_golden("f23_noise_mix")

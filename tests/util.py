"""Shared helpers for the test-suite (fixture loading, config parsing)."""
import ast
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def golden_cfg(z):
    from oracle.dicow_oracle import OracleConfig
    d = ast.literal_eval(str(z["cfg"]))
    return OracleConfig(**{k: v for k, v in d.items() if k in OracleConfig.__dataclass_fields__})


def golden_params(z, prefix="p.", requires_grad=False, dtype=torch.float32):
    out = {}
    for k in z.files:
        if k.startswith(prefix):
            t = torch.from_numpy(z[k]).to(dtype).clone()
            out[k[len(prefix):]] = t
    if "proj_out.weight" in out and "model.decoder.embed_tokens.weight" in out:
        out["proj_out.weight"] = out["model.decoder.embed_tokens.weight"]      # tied
    if requires_grad:
        for t in set(out.values()):
            if t.is_floating_point():
                t.requires_grad_(True)
    return out


def T(z, k, dtype=None):
    t = torch.from_numpy(np.asarray(z[k]))
    if dtype is not None:
        t = t.to(dtype)
    elif t.dtype == torch.float16:
        t = t.float()
    return t


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


def hashed_mel(B, M, T):
    """Deterministic pseudo-random mel in [-1, 1] from integer arithmetic only; the inputs of golden F11's SpecAug cases
    (same formula as tests/golden/make_golden.py:hashed_mel)."""
    b = np.arange(B, dtype=np.int64)[:, None, None]
    m = np.arange(M, dtype=np.int64)[None, :, None]
    t = np.arange(T, dtype=np.int64)[None, None, :]
    h = (m * 7919 + t * 104729 + b * 1299709 + (m * t) % 613 * 31) % 2001 - 1000
    return (h.astype(np.float64) / 1000.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# Deterministic, integer-hashed parameters and inputs for the REAL-DIMENSION goldens (tests/golden/make_golden_realdims.py):
# the fixtures of whisper-tiny / -base / -large-v3-turbo sized models store OUTPUTS only -- both the reference run (build
# container) and the GPU test regenerate identical weights / inputs from these integer formulas (exact in int64 and in the
# final int -> float32 conversion, on any device).
def _crc(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def hashed_uniform(name, shape, device="cpu"):
    """float32 tensor of `shape`, uniform in [-1, 1) on a 2^-23 grid, a pure function of (name, flat index)."""
    n = 1
    for d in shape:
        n *= int(d)
    seed = _crc(name)
    out = torch.empty(n, dtype=torch.float32, device=device)
    CH = 1 << 24
    for s in range(0, n, CH):
        idx = torch.arange(s, min(n, s + CH), dtype=torch.int64, device=device)
        h = (idx * 1540483477 + seed * 40503 + 12345) & 0xFFFFFFFF
        h = h ^ (h >> 15)
        h = (h * 1103515245 + 12345) & 0xFFFFFFFF
        h = h ^ (h >> 13)
        h = (h * 1540483477) & 0xFFFFFFFF
        h = h ^ (h >> 16)
        out[s:s + idx.numel()] = ((h & 0xFFFFFF).to(torch.float32) - 8388608.0) / 8388608.0
    return out.view(*shape)


def hashed_init_(model, skip=("embed_positions",)):
    """Overwrite every parameter of a (reference or product) DiCoW model with hashed values scaled like a trained model's:
    LayerNorm weights 1 + 0.1u, diagonal FDDT weights base + 0.1u (base = the reference's suppressive initialisation),
    matrices fan_in^-0.5 * u * 1.7 (unit-variance outputs), biases / vectors 0.1u.  The encoder's sinusoidal positions stay."""
    with torch.no_grad():
        seen = set()
        for n, p in model.named_parameters():
            if id(p) in seen or any(s in n and "encoder" in n for s in skip):
                continue
            seen.add(id(p))
            u = hashed_uniform(n, tuple(p.shape), device=p.device)
            if n.endswith("layer_norm.weight"):
                v = 1.0 + 0.1 * u
            elif "fddt" in n and n.endswith(".weight") and p.dim() == 1:
                base = 0.5 if ("initial_fddt" in n and ("silence" in n or "non_target" in n)) else 1.0
                v = base + 0.1 * u
            elif "fddt" in n and n.endswith(".weight") and p.dim() == 2:
                v = torch.eye(p.shape[0], device=p.device) + 0.3 * p.shape[0] ** -0.5 * u
            elif n.endswith("gate"):
                v = 0.3 + 0.5 * u
            elif p.dim() >= 2:
                v = (1.7 * p[0].numel() ** -0.5) * u
            else:
                v = 0.1 * u
            p.copy_(v.to(p.dtype))


def hashed_stno(B, T, tag="stno"):
    """[B, 4, T] soft STNO masks (rows sum to 1; ~30 % of the frames one-hot, the last T // 10 frames silence = 1 like the
    collator's padding, reference collators.py:157-161) from integer hashes only."""
    u = hashed_uniform(tag, (B, T, 5)).double()
    e = torch.exp(2.0 * u[..., :4] * 1.5)
    s = e / e.sum(-1, keepdim=True)
    hard = torch.nn.functional.one_hot(((u[..., 0] + 1.0) * 2.0).floor().clamp(0, 3).long(), 4).double()
    pick = (u[..., 4] < -0.4).double()[..., None]
    s = pick * hard + (1 - pick) * s
    s[:, -(T // 10):, :] = 0.0
    s[:, -(T // 10):, 0] = 1.0
    return s.permute(0, 2, 1).contiguous().float()


def hashed_labels(B, L, lo, hi, tag="labels", pad_rows=()):
    """int64 [B, L] labels in [lo, hi); rows listed in pad_rows get their last L // 4 positions set to -100."""
    u = hashed_uniform(tag, (B, L)).double()
    lab = (lo + ((u + 1.0) * 0.5 * (hi - lo)).floor()).clamp(lo, hi - 1).long()
    for r in pad_rows:
        lab[r, L - L // 4:] = -100
    return lab


def subsample(t, n=256):
    """Deterministic flat subsample of a tensor: n elements at a stride that is coprime with every dimension (a stride that
    is a multiple of the row length would sample ONE column; the fixture side and the test side agree on the rule)."""
    import math
    f = t.reshape(-1)
    step = max(1, f.numel() // n)
    dims = [int(d) for d in t.shape if int(d) > 1]
    while step > 1 and any(math.gcd(step, d) != 1 for d in dims):
        step -= 1
    return f[::step][:n].clone()


def sketch(t, name, k=4):
    """k inner products of the WHOLE tensor with hashed +-1 vectors: a direction-sensitive checksum of tensors too large to store."""
    f = t.reshape(-1).double()
    out = []
    for i in range(k):
        sgn = torch.where(hashed_uniform(f"{name}.sketch{i}", (f.numel(),), device=f.device) < 0, -1.0, 1.0).double()
        out.append((f * sgn).sum())
    return torch.stack(out).float()


# ---------------------------------------------------------------------------------------------------------------------------
# F20 (training trajectory): the batches of tests/golden/make_golden_trajectory.py -- two distinct hashed batches, alternating.
F20_PREFIXES = ["model.encoder.additional_layer", "model.encoder.additional_self_attention_layer", "model.encoder.lm_head",
                "model.encoder.subsample_conv1", "model.encoder.subsample_conv2", "model.encoder.fddts",
                "model.encoder.initial_fddt", "model.encoder.ca_enrolls"]          # reference configs/base.yaml:18


def f20_batches(case, K, ts0=None):
    """case "small": 80 mels, 100 frames, B = 2, 10 labels below id 400; "small_se": the same with an enrollment per row
    (SE-DiCoW); "tiny": whisper-tiny dimensions, B = 1, 32 labels with a timestamp token (ts0 = first timestamp id) in front."""
    se = case == "small_se"
    B, L, T, M, vocab_hi = (2, 10, 100, 80, 400) if case.startswith("small") else (1, 32, 1500, 80, 50257)
    mel = torch.from_numpy(hashed_mel((4 if se else 2) * B, M, 2 * T)).clone() * 1.5
    two = []
    for j in range(2):
        lab = hashed_labels(B, L, 0, vocab_hi, f"f20.{case}.{j}.labels", pad_rows=(B - 1,) if B > 1 else ())
        if ts0 is not None:
            lab[:, 0] = ts0 + 7 + j
        b = dict(input_features=mel[j * B:(j + 1) * B], stno_mask=hashed_stno(B, T, f"f20.{case}.{j}.stno"), labels=lab,
                 upp_labels=lab.clone())
        if se:
            b["enrollments"] = {"input_features": mel[(2 + j) * B:(3 + j) * B], "stno_mask": hashed_stno(B, T, f"f20.{case}.{j}.enr.stno")}
        two.append(b)
    return [two[k % 2] for k in range(K)]


# ---------------------------------------------------------------------------------------------------------------------------
# Layout-edge helpers (tests/test_gpu_layout_edges.py): outputs inside guard bands, inputs inside poison.  Plain torch, any device.
SENTINEL16 = 0x7FC1          # every 16-bit word of a guard: bf16 0x7FC1 and fp32 0x7FC17FC1 are both quiet NaNs, so a stray
                             # read-modify-write shows as well as a stray store
GUARD_ROWS = 256             # trailing guard rows: taller than any output tile of the library (256 x 256 is the largest)
POISON_BIG = 3.0e4           # the finite poison (bf16-exact neighbourhood of 2^15): one such operand swamps a product of O(1) terms


def _flat_index_mask(total, shape, strides, offset):
    m = torch.zeros(total, dtype=torch.bool)
    m.as_strided(tuple(shape), tuple(strides), offset).fill_(True)
    return m


class Guarded:
    """One flat buffer [lead guard | span rows of `ld` elements | >= GUARD_ROWS guard rows]; `view` is the logical region (a strided
    view into the span, stride(-2) == ld for the plain 2-D case), everything else holds the sentinel.  check() compares the whole
    buffer outside the logical region with the sentinel through an integer view and names the first offending (row, col) -- row
    and col counted in the span's [*, ld] grid, so the leading guard has negative rows and the `ld - cols` gap has col >= cols."""

    def __init__(self, buf, view, lead, ld, inside, name):
        self.buf, self.view, self.lead, self.ld, self.inside, self.name = buf, view, lead, ld, inside, name

    def outside_words(self):
        """The 16-bit words of every element outside the logical region, [n_outside, itemsize / 2] (int16)."""
        w = self.buf.view(torch.int16).view(self.buf.numel(), -1)
        return w[~self.inside.to(w.device)]

    def violations(self):
        """Flat element indices (ascending) outside the logical region whose bits are not the sentinel."""
        w = self.buf.view(torch.int16).view(self.buf.numel(), -1)
        bad = (w != SENTINEL16).any(1).cpu() & ~self.inside
        return torch.nonzero(bad).flatten()

    def first_violation(self):
        """None, or the (row, col) of the first element outside the logical region that was written."""
        v = self.violations()
        if v.numel() == 0:
            return None
        i = int(v[0]) - self.lead
        return (i // self.ld, i % self.ld)          # (floor division: the leading guard gives row < 0)

    def check(self):
        rc = self.first_violation()
        assert rc is None, f"{self.name}: element outside the logical region overwritten, first at (row {rc[0]}, col {rc[1]}) of the [*, {self.ld}] grid"

    def untouched_inside(self):
        """Number of logical elements that still hold the sentinel (accumulate = 0 outputs must leave none)."""
        w = self.view.contiguous().view(torch.int16).view(self.view.numel(), -1)
        return int((w == SENTINEL16).all(1).sum())


def _layout(shape, ld, strides, offset):
    shape = tuple(int(s) for s in shape)
    if strides is None:
        assert len(shape) <= 2, "give strides for views of more than two dimensions"
        strides = (ld, 1) if len(shape) == 2 else (1,)
    last = offset + sum((n - 1) * s for n, s in zip(shape, strides))
    return shape, tuple(strides), last // ld + 1


def guarded(shape, ld, dtype, device="cuda", *, strides=None, offset=0, span_rows=None, init=None, lead_rows=4,
            trail_rows=GUARD_ROWS, name="out"):
    """An OUTPUT of logical `shape` inside guard bands.  Plain 2-D: rows x cols with row stride ld >= cols.  Any other view: give
    `strides` (elements) and `offset` (elements from the start of the span) -- e.g. the [B, L, H, 64] slice of packed [B, Lmax, 3D]
    rows.  span_rows: rows of ld elements the span holds (default: up to the last logical element's row).  init: values of the
    logical region for outputs that accumulate (None: the sentinel there too, so an output that must be overwritten can be checked
    with untouched_inside()).  The base of the view is 256-byte aligned when offset == 0 (the lead guard is a multiple of 64
    elements on top of torch's allocation alignment); dtype must have 2- or 4-byte elements."""
    assert torch.empty(0, dtype=dtype).element_size() in (2, 4)
    shape, strides, need = _layout(shape, ld, strides, offset)
    span_rows = need if span_rows is None else span_rows
    assert span_rows >= need and trail_rows >= GUARD_ROWS
    lead = -(-lead_rows * ld // 64) * 64
    total = lead + (span_rows + trail_rows) * ld
    buf = torch.empty(total, dtype=dtype, device=device)
    buf.view(torch.int16).fill_(SENTINEL16)
    view = buf.as_strided(shape, strides, lead + offset)
    if init is not None:
        view.copy_(init.to(device=device, dtype=dtype))
    return Guarded(buf, view, lead, ld, _flat_index_mask(total, shape, strides, lead + offset), name)


def poisoned(t, ld, device="cuda", *, strides=None, offset=0, span_rows=None, kind="nan", poison_row=None, lead_rows=4,
             trail_rows=2 * GUARD_ROWS):
    """An INPUT: the values of `t` in a strided view (layout arguments as in `guarded`) of one allocation in which every other
    element -- the lead, the row gaps, the rows after the last logical row, the gaps between batches, the tail -- holds poison.
    kind "nan": the NaN bit pattern of the guards; "big": +-POISON_BIG alternating by element; "zero": zeros (the run the
    poisoned ones must equal bit for bit).  poison_row ([ld] values): tile this row pattern over the whole allocation instead
    (attention: keys aligned with the queries, values +100).  The tail is 512 rows: the widest operand tile (the 320 weight rows
    of a 192 x 320 GEMM tile) stays inside the allocation even if a kernel reads it whole.  Returns the view."""
    shape, strides, need = _layout(t.shape, ld, strides, offset)
    span_rows = need if span_rows is None else span_rows
    lead = -(-lead_rows * ld // 64) * 64
    rows_total = lead // ld + 1 + span_rows + trail_rows
    total = lead + (span_rows + trail_rows) * ld
    if poison_row is not None:
        assert poison_row.numel() == ld
        # (row pattern in phase with the span: the lead is filled from its end backwards)
        flat = poison_row.to(t.dtype).repeat(rows_total + 1)
        ph = (ld - lead % ld) % ld
        buf = flat[ph:ph + total].clone().to(device)
    elif kind == "nan":
        buf = torch.empty(total, dtype=t.dtype, device=device)
        buf.view(torch.int16).fill_(SENTINEL16)
    elif kind == "big":
        buf = torch.full((total,), POISON_BIG, dtype=t.dtype, device=device)
        buf[1::2] = -POISON_BIG
    else:
        assert kind == "zero", kind
        buf = torch.zeros(total, dtype=t.dtype, device=device)
    view = buf.as_strided(shape, strides, lead + offset)
    view.copy_(t.to(device))
    return view


# ---------------------------------------------------------------------------------------------------------------------------
# Far-offset helpers (tests/test_gpu_far_offsets.py): operands whose elements lie more than 2^31 / 2^32 bytes from their base
# pointer, as strided views into ONE device arena that holds the NaN sentinel of the guards everywhere else.
MARK31, MARK32 = 1 << 31, 1 << 32
FAR_FRONT_CAP = 8 << 30      # front pad of a far view: its own span, capped here (see far_view)
ARENA_MAX_BYTES = 20 << 30
_SCAN_WORDS = 1 << 28        # 16-bit words per chunk of the device scans (512 MiB, no full-size mask)


def _word_checksum(t):
    """Sum of the 16-bit words of a (compact) tensor as integers, chunk by chunk: cheap evidence that an input was not overwritten."""
    w = t.contiguous().view(torch.int16).reshape(-1)
    return sum(int(w[s:s + _SCAN_WORDS].sum(dtype=torch.int64)) for s in range(0, w.numel(), _SCAN_WORDS))


def _nonsentinel_words(t):
    """16-bit words of a (compact) tensor that differ from the sentinel."""
    w = t.contiguous().view(torch.int16).reshape(-1)
    return sum(int((w[s:s + _SCAN_WORDS] != SENTINEL16).sum()) for s in range(0, w.numel(), _SCAN_WORDS))


class Arena:
    """One uint8 device allocation, filled with the sentinel by reset(); far_view() places logical operands in it.  check() counts
    the 16-bit words of the WHOLE arena that are not the sentinel, chunk by chunk on the device, and compares the count with the
    words of the placed views themselves (inputs as placed, outputs as they are now; a logical word whose bits happen to equal
    the sentinel counts on neither side): any store outside the logical regions makes the counts differ, and so do two views
    that overlap.  Inputs must also still hold the bits they were given."""

    def __init__(self, nbytes, device="cuda"):
        assert nbytes % 4096 == 0 and nbytes <= ARENA_MAX_BYTES
        self.nbytes, self.buf = nbytes, torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.reset()

    def reset(self):
        self.buf.view(torch.int16).fill_(SENTINEL16)
        self.inputs, self.outputs, self.used = [], [], 0

    def count_nonsentinel(self):
        return _nonsentinel_words(self.buf)

    def check(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        for name, view, vals, _ in self.inputs:
            same = torch.equal(view, vals) if torch.is_tensor(vals) else _word_checksum(view) == vals       # (filled in place: a checksum)
            assert same, f"{name}: an input operand was overwritten"
        want = sum(n for *_, n in self.inputs) + sum(_nonsentinel_words(v) for _, v in self.outputs)
        got = self.count_nonsentinel()
        assert got == want, f"arena holds {got} non-sentinel words, the logical operands {want}: {got - want} stray (or missing) words"
        return got


def far_arena_fixture(nbytes, headroom):
    """The module-scoped arena fixture of a test file (import the returned function under the name the tests use): ONE allocation of
    `nbytes`, made once; skips when the device has less than nbytes + headroom (the compact operands and references) free."""
    import pytest

    @pytest.fixture(scope="module")
    def far_arena_module():
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        need = nbytes + headroom
        if torch.cuda.mem_get_info()[0] < need:
            pytest.skip(f"needs {-(-need >> 30)} GiB of free device memory")
        arena = Arena(nbytes)
        yield arena
        arena.buf = None

    return far_arena_module


def _ceil_to(x, a):
    return -(-x // a) * a


def tall_ld(rows, row_elems, itemsize, align_elems=8, mark=MARK32, straddle=True):
    """Tall-stride recipe: a leading dimension (elements, a multiple of align_elems) near mark / (rows - 2) bytes, so that the rows
    around rows / 2 begin near mark / 2 and the last row begins past the mark.  Among the rows of the upper half the one is looked
    for that can BEGIN less than one row length below the mark, so that its elements straddle it (the carry inside a row).
    Returns (ld, straddling row or None)."""
    assert rows >= 4
    ab, rb = align_elems * itemsize, row_elems * itemsize
    for r in range(rows - 2, rows // 2 if straddle else rows - 2, -1):      # (straddle=False: the plain recipe, the smallest span)
        ldb = mark // r // ab * ab
        below = mark - r * ldb                                # row r begins `below` bytes under the mark
        if 0 < below < rb and ldb >= rb:
            assert (rows - 1) * ldb >= mark and r * ldb < mark < r * ldb + rb
            return ldb // itemsize, r
    ldb = _ceil_to(-(-mark // (rows - 2)), ab)
    assert (rows - 1) * ldb >= mark and ldb >= rb
    return ldb // itemsize, None


def far_view(arena, shape, dtype, strides, *, values=None, base_bytes=None, name="far", output=False, fill=None):
    """A strided view (strides in elements, last one 1) of the arena with the logical `values` written into it (outputs: nothing is
    written, the region keeps the sentinel; fill(view): an input too large to exist twice is generated in place).  base_bytes: where in the arena the view begins (default: after everything placed so
    far).  FRONT PAD, asserted here: the base lies at least min(span, 8 GiB) into the arena, so an offset truncated to 32 bits, taken
    as a signed 32-bit byte count or wrapped as a 32-bit ELEMENT index (2^32 elements = 8 GiB of bf16) still lands inside the
    arena -- a wrapped read sees the sentinel, a wrapped write lands where check() looks -- instead of leaving the allocation."""
    isz = torch.empty(0, dtype=dtype).element_size()
    shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
    assert len(shape) == len(strides) and strides[-1] == 1 and all(s >= 0 for s in strides)
    span = (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * isz
    front = min(span, FAR_FRONT_CAP)
    base = _ceil_to(max(arena.used, front), 256) if base_bytes is None else int(base_bytes)
    assert base % 256 == 0 and base >= front, (name, "front pad", base, front)
    assert base + span <= arena.nbytes, (name, "the arena is too small", base + span, arena.nbytes)
    # the wrapped images of every offset o < span stay inside [0, base + span): o mod 2^32 (o - 2^32 only where o >= 2^32), o as a
    # signed 32-bit byte count (o - 2^32 for o in [2^31, 2^32): >= -2^31), o / isz as a signed 32-bit element index (only where
    # o >= 2^31 isz, and then o - 2^32 isz >= -2^31 isz)
    assert base >= min(span, MARK31) and (span < MARK31 * isz or base >= MARK31 * isz)
    typed = arena.buf[base:base + span].view(dtype)
    view = typed.as_strided(shape, strides, typed.storage_offset())
    arena.used = max(arena.used, base + span)
    if output:
        assert values is None and fill is None
        arena.outputs.append((name, view))
    elif fill is not None:
        fill(view)
        arena.inputs.append((name, view, _word_checksum(view), _nonsentinel_words(view)))
    else:
        vals = values.to(device=arena.buf.device, dtype=dtype).contiguous()
        view.copy_(vals)
        arena.inputs.append((name, view, vals, _nonsentinel_words(vals)))
    return view

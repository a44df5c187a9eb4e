"""References of the log-mel front end and of the small "glue" kernels (csrc/elementwise.hip, the full-FDDT combine of
csrc/fddt_ln.hip), written from the operation each kernel stands for -- not from the kernels -- and shared by
tests/test_host_glue_ref.py (which pins them on the CPU against independent formulations: autograd, conv1d, a sequential fp32 sum) and
by tests/test_gpu_glue_kernels.py / tests/test_gpu_logmel_edges.py (which use them as the oracle).  Plain torch / numpy on the CPU:
fp64 where arithmetic is involved, exact fp32 / bf16 emulation (fp32 ops in the documented order, `.to(torch.bfloat16)` for the
roundings) where the result is determined bit for bit.  The seeded inputs of both test files live here too, so that the host test
checks the very tensors the GPU test uses."""
import math

import numpy as np
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)


def bits(t):
    """Integer view of a 2- or 4-byte tensor (bit-for-bit comparisons; NaNs compare by payload)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def rand(shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- summation bound
def sum_bound(abs_sum, n, ref, product_terms=False):
    """|fl(sum of n terms, ANY order) - exact| <= (n - 1) u sum|terms| + u |ref|, u = 2^-24: each of the n - 1 additions rounds a
    partial sum that is at most sum|terms| in magnitude (first order in u: the (n - 1) u sum|terms| term), and u |ref| covers the
    rounding of the stored result.  product_terms: every term is itself an fp32 product (x * x, g * upd) and carries one rounding of
    its own (u |term|, unless the compiler contracts it into an fma), so n counts one more.  abs_sum, ref: fp64 tensors or floats."""
    k = n - 1 + (1 if product_terms else 0)
    return k * U * abs_sum + U * abs(ref)


# ---------------------------------------------------------------------------------------------------------------- GELU'
def gelu_grad_ref(x):
    """d/dx [x Phi(x)] = Phi(x) + x phi(x) in fp64 (exact-erf GELU)."""
    x = x.to(F64)
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_pre_grid(n):
    """n bf16 pre-activations: +-0, +-30 and a dense grid on [-9, 9] (every bf16 value there when n allows: there are 33 314 of
    them; otherwise evenly spaced ones), tiled to length n."""
    special = torch.tensor([0.0, -0.0, 30.0, -30.0, 9.0, -9.0], dtype=F32).to(BF16)
    if n <= special.numel():
        return special[:n].clone()
    if n >= 40000:
        allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
        grid = allb[torch.isfinite(allb.float()) & (allb.float().abs() <= 9.0)]
    else:
        grid = torch.linspace(-9.0, 9.0, n - special.numel(), dtype=F64).to(BF16)
    base = torch.cat((special, grid))
    return base.repeat(-(-n // base.numel()))[:n].clone()


# ---------------------------------------------------------------------------------------------------------------- casts / packs
def cast_values(n, seed=11):
    """fp32 inputs of the cast: Gaussian values with, in front AND at the very end (the scalar tail), the values on which a rounding
    can go wrong: exact ties between two bf16 neighbours with an even and an odd lower neighbour (both signs), +-0, fp32 denormals
    (the largest, the smallest, one that is a tie of the bf16 denormal grid), +-inf, +-the largest finite fp32 (rounds to +-inf)."""
    special_bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties: even lower neighbour (stays), odd (goes up), both signs
                    0x3F808001, 0x3F817FFF,                              # just above / just below a tie
                    0x00000000, 0x80000000, 0x007FFFFF, 0x00000001, 0x80000001, 0x00018000, 0x00008000,
                    0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF]
    sp = torch.tensor(special_bits, dtype=torch.int64).to(torch.int32).view(F32)
    x = rand((n,), seed, 3.0)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 2 * sp.numel():
        x[-sp.numel():] = sp.flip(0)
    return x


def mel_timemajor_ref(mel):
    """[B, M, Tin] fp32 -> [B, Tin + 2, M] bf16, rows 0 and Tin + 1 zero."""
    B, M, Tin = mel.shape
    out = torch.zeros(B, Tin + 2, M, dtype=BF16)
    out[:, 1:Tin + 1] = mel.transpose(1, 2).to(BF16)
    return out


def conv_pack_ref(w, kpad):
    """Conv1d weight [O, C, 3] fp32 -> bf16 [O, kpad]: column k = tap * C + c, zero for k >= 3 C."""
    O, C, _ = w.shape
    out = torch.zeros(O, kpad, dtype=BF16)
    out[:, :3 * C] = w.permute(0, 2, 1).reshape(O, 3 * C).to(BF16)
    return out


def conv_unpack_ref(g_w, g_packed):
    """g_w [O, C, 3] + the un-permuted live columns of g_packed [O, kpad] (one fp32 add per element)."""
    O, C, _ = g_w.shape
    return g_w + g_packed[:, :3 * C].reshape(O, 3, C).permute(0, 2, 1)


def sum_over_batch_ref(out, g):
    """fp32 ((out + g[0]) + g[1]) + ... in batch order."""
    s = out.clone()
    for b in range(g.shape[0]):
        s = s + g[b]
    return s


# ---------------------------------------------------------------------------------------------------------------- embedding
def embed_fwd_ref(ids, tok, pos):
    """tok[id] + pos[l]: one fp32 add per element.  ids [B, Lq], tok [V, D], pos [>= Lq, D]."""
    return tok[ids] + pos[:ids.shape[1]][None]


def embed_bwd_ref(ids, g, V, P):
    """fp64 scatter-add of g [B, Lq, D]: (d_tok [V, D], d_pos [P, D], and the sums of |terms| of both, for the summation bound)."""
    B, Lq, D = g.shape
    g = g.to(F64)
    flat = ids.reshape(-1)
    d_tok, a_tok = torch.zeros(V, D, dtype=F64), torch.zeros(V, D, dtype=F64)
    d_tok.index_add_(0, flat, g.reshape(-1, D))
    a_tok.index_add_(0, flat, g.reshape(-1, D).abs())
    d_pos, a_pos = torch.zeros(P, D, dtype=F64), torch.zeros(P, D, dtype=F64)
    d_pos[:Lq] = g.sum(0)
    a_pos[:Lq] = g.abs().sum(0)
    return d_tok, d_pos, a_tok, a_pos


def embed_bwd_exact(ids, g, tok0, pos0):
    """The kernel's documented order in fp32: per token the rows that hold it are added up in row order and the sum is added to the
    target once; per position the batches in order.  (tok0 + d_tok, pos0 + d_pos) fp32."""
    B, Lq, D = g.shape
    flat, rows = ids.reshape(-1), g.reshape(-1, D)
    tok, pos = tok0.clone(), pos0.clone()
    for t in torch.unique(flat).tolist():
        idx = torch.nonzero(flat == t).flatten().tolist()
        s = rows[idx[0]].clone()
        for r in idx[1:]:
            s = s + rows[r]
        tok[t] = tok[t] + s
    for l in range(Lq):
        s = g[0, l].clone()
        for b in range(1, B):
            s = s + g[b, l]
        pos[l] = pos[l] + s
    return tok, pos


# ---------------------------------------------------------------------------------------------------------------- conv stem
def col2im_ref(dA2, T2, C):
    """The input gradient of a k = 3, stride-2, padding-1 convolution from its im2col gradient dA2 [B, T2, 3 C] (column tap * C + c):
    row t, tap j lands on padded frame 2 t + j, i.e. on frame s = 2 t + j - 1 of the 2 T2 frames; the left pad row (s = -1) is
    dropped.  Computed in dA2's dtype: at most two terms meet, so fp32 gives the kernel's sum bit for bit and fp64 the exact one."""
    B = dA2.shape[0]
    out = torch.zeros(B, 2 * T2 + 2, C, dtype=dA2.dtype)
    for j in range(3):
        out[:, j:j + 2 * T2:2] += dA2[:, :, j * C:(j + 1) * C]
    return out[:, 1:2 * T2 + 1]


def col2im_input(B, T2, C, seed=31):
    """bf16 [B, T2, 3 C]: noise around a distinct constant per tap (1, 2, 4), so that a swapped tap shows."""
    x = rand((B, T2, 3, C), seed, 0.25)
    x += torch.tensor([1.0, 2.0, 4.0])[None, None, :, None]
    return x.reshape(B, T2, 3 * C).to(BF16)


# ---------------------------------------------------------------------------------------------------------------- SCB glue
# Row layout [Bp][2][T][D]: slot 0 = mixture, slot 1 = enrollment.
def scb_split_ref(hf, Bp, T, D):
    """(q_in, kv_in) bf16 [Bp * T, D]: the mixture / enrollment rows of hf fp32; the right half of `cat` is q_in."""
    h = hf.reshape(Bp, 2, T * D)
    return h[:, 0].reshape(Bp * T, D).to(BF16), h[:, 1].reshape(Bp * T, D).to(BF16)


def scb_merge_fwd_ref(hf, upd, gate, Bp, T, D):
    """hf + [slot even] tanh(gate) upd, in hf's dtype (fp64 for the reference)."""
    out = hf.reshape(Bp, 2, T * D).clone()
    out[:, 0] += torch.tanh(gate.to(hf.dtype)) * upd.to(hf.dtype).reshape(Bp, T * D)
    return out.reshape(-1)


def scb_gate_bwd_ref(g, upd, gate, Bp, T, D):
    """fp64: d_upd = g_mix tanh(gate) [Bp * T * D]; S = sum g_mix upd; sum |g_mix upd|; factor = 1 - tanh(gate)^2.
    d_gate += factor * S."""
    gm = g.to(F64).reshape(Bp, 2, T * D)[:, 0].reshape(-1)
    u = upd.to(F64).reshape(-1)
    tg = torch.tanh(gate.to(F64)).reshape(())
    return gm * tg, (gm * u).sum(), (gm * u).abs().sum(), 1.0 - tg * tg


def scb_merge_bwd_ref(g, d_qin, d_cat_right, d_kvin, Bp, T, D):
    """g + (d_qin + d_cat_right) on mixture rows, g + d_kvin on enrollment rows, in g's dtype (fp32: the kernel's order)."""
    out = g.reshape(Bp, 2, T * D).clone()
    out[:, 0] = out[:, 0] + (d_qin.reshape(Bp, T * D) + d_cat_right.to(g.dtype).reshape(Bp, T * D))
    out[:, 1] = out[:, 1] + d_kvin.reshape(Bp, T * D)
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- full-FDDT combine
def combine_fwd_ref(y4, h, stno, use_mask):
    """sum_c m_c (use_c ? y4_c : h) in fp64, and sum_c |m_c v_c|.  y4 [B, T, 4, D], h [B, T, D], stno [B, 4, T]."""
    y4, h, m = y4.to(F64), h.to(F64), stno.to(F64).permute(0, 2, 1)            # m [B, T, 4]
    out, mag = torch.zeros_like(h), torch.zeros_like(h)
    for c in range(4):
        v = y4[:, :, c] if (use_mask >> c) & 1 else h
        out += m[:, :, c, None] * v
        mag += (m[:, :, c, None] * v).abs()
    return out, mag


def combine_bwd_ref(g, stno, use_mask):
    """(d_y4 bf16 [B, T, 4, D] -- slices of unused classes are not defined and returned as zeros --, dh fp32 [B, T, D]):
    d_y4_c = bf16(fp32(g m_c)); dh = g (sum of the unused classes' m_c, added up in class order from 0)."""
    B, T, D = g.shape
    m = stno.permute(0, 2, 1)
    d_y4 = torch.zeros(B, T, 4, D, dtype=BF16)
    md = torch.zeros(B, T, dtype=F32)
    for c in range(4):
        if (use_mask >> c) & 1:
            d_y4[:, :, c] = (g * m[:, :, c, None]).to(BF16)
        else:
            md = md + m[:, :, c]
    return d_y4, g * md[:, :, None]


# ---------------------------------------------------------------------------------------------------------------- log-mel
N_FFT, HOP = 400, 160
LOGMEL_LENGTHS = (640, 10240, 10400, 30720)           # 4, 64, 65 and 192 frames (the kernel works on blocks of 64 frames)
LOGMEL_N = 30720
LOGMEL_SIGNALS = ("noise", "impulses", "noise_then_zeros", "quiet", "zeros", "sine440", "square250")
LOGMEL_BATCH = ("noise", "quiet", "zeros")            # loud, quiet, silent


def logmel_signal(name, n=LOGMEL_N):
    """Seeded float32 waveforms of n samples."""
    rng = np.random.default_rng(abs(hash_name(name)) + n)
    t = np.arange(n)
    if name == "noise":
        x = rng.standard_normal(n) * 0.1
    elif name == "quiet":
        x = rng.standard_normal(n) * 1e-3
    elif name == "zeros":
        x = np.zeros(n)
    elif name == "impulses":
        x = np.zeros(n)
        x[[0, 1, 199, 200, 201, n - 201, n - 200, n - 2, n - 1]] = 0.5
    elif name == "noise_then_zeros":
        x = np.zeros(n)
        x[:7000] = rng.standard_normal(7000) * 0.1
    elif name == "sine440":
        x = 0.3 * np.sin(2.0 * np.pi * 440.0 * t / 16000.0)
    else:
        assert name == "square250", name
        x = np.where((t // 32) % 2 == 0, 1.0, -1.0)               # 64 samples per period at 16 kHz
    return x.astype(np.float32)


def hash_name(name):
    import zlib
    return zlib.crc32(name.encode()) & 0xFFFF


_LM = {}


def _logmel_tables(n_mels):
    if n_mels not in _LM:
        from oracle.logmel import mel_filter_bank
        k = np.arange(N_FFT)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / N_FFT)
        ang = 2.0 * np.pi * np.outer(k, np.arange(N_FFT // 2 + 1)) / N_FFT
        _LM[n_mels] = ((win[:, None] * np.cos(ang)).astype(np.float32), (win[:, None] * np.sin(ang)).astype(np.float32),
                       mel_filter_bank(n_mels).astype(np.float32))
    return _LM[n_mels]


def logmel_fp32(wave, n_mels):
    """An honest fp32 restatement of the front end's arithmetic: float32 matmul of the reflect-padded frames against the windowed
    cos / sin tables, power, fp32 mel projection, log10(max(., 1e-10)), clamp at max - 8, (x + 4) / 4.  [n] -> [n_mels, n / 160]."""
    c, s, fb = _logmel_tables(n_mels)
    x = np.asarray(wave, dtype=np.float32)
    xp = np.pad(x, (N_FFT // 2, N_FFT // 2), mode="reflect")
    nf = x.shape[0] // HOP                                        # (the last of the n / 160 + 1 centred frames is dropped)
    fr = xp[np.arange(N_FFT)[None, :] + HOP * np.arange(nf)[:, None]]
    re, im = fr @ c, fr @ s
    mel = (re * re + im * im) @ fb
    v = np.log10(np.maximum(mel, np.float32(1e-10))).astype(np.float32)
    v = np.maximum(v, v.max() - np.float32(8.0))
    return ((v + np.float32(4.0)) * np.float32(0.25)).T.astype(np.float32)


def logmel_oracle(wave, n_mels):
    """The fp64 oracle, per clip."""
    from oracle.logmel import log_mel
    return log_mel(np.asarray(wave, dtype=np.float32), n_mels, dtype=np.float64)

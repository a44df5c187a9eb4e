"""tests/glue_ref.py pinned on the CPU against independent formulations: the col2im reference against the input gradient of
torch's conv1d, GELU' and the SCB / full-combine references against autograd, the summation bound against a sequential fp32 sum of
the very inputs the GPU tests use, and the fp32 restatement of the log-mel front end against the fp64 oracle (so the inputs of
tests/test_gpu_logmel_edges.py are known to be ones the suite's 3e-4 is fair for)."""
import numpy as np
import pytest
import torch

from tests import glue_ref as R

F64 = torch.float64


@pytest.mark.parametrize("B,T2,C", [(1, 1, 2), (2, 3, 6), (2, 50, 384)])
def test_col2im_ref_is_the_input_gradient_of_conv1d(B, T2, C):
    """conv1d(k = 3, stride 2, padding 1) over 2 T2 frames gives T2 frames; with the weight W[o, c, j] its input gradient is the
    col2im of dA2[b, t, j C + c] = sum_o dY[b, o, t] W[o, c, j]."""
    O = 5
    x = R.rand((B, C, 2 * T2), 1, dtype=F64).requires_grad_(True)
    w = R.rand((O, C, 3), 2, dtype=F64)
    dy = R.rand((B, O, T2), 3, dtype=F64)
    y = torch.nn.functional.conv1d(x, w, stride=2, padding=1)
    assert y.shape == (B, O, T2)
    (y * dy).sum().backward()
    dA2 = torch.einsum("bot,ocj->btjc", dy, w).reshape(B, T2, 3 * C)
    got = R.col2im_ref(dA2, T2, C)                                   # [B, 2 T2, C]
    assert float((got - x.grad.transpose(1, 2)).abs().max()) < 1e-12
    # the fp32 form of the same scatter is what the kernel's sum of (at most) two bf16 values gives
    a = R.col2im_input(B, T2, C)
    assert float((R.col2im_ref(a.float(), T2, C).double() - R.col2im_ref(a.double(), T2, C)).abs().max()) == 0.0


def test_gelu_grad_ref_equals_autograd():
    x = R.gelu_pre_grid(1028).double().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    assert float((R.gelu_grad_ref(x.detach()) - x.grad).abs().max()) < 1e-14
    big = R.gelu_pre_grid(50000)
    assert big.numel() == 50000 and float(big.float().abs().max()) == 30.0
    # every bf16 value of [-9, 9]: bit patterns 0x0000 ... 0x4110 (= 9.0) with either sign
    assert torch.unique(R.bits(big[big.float().abs() <= 9.0])).numel() == 2 * (0x4110 + 1)


@pytest.mark.parametrize("gate", [0.0, 0.3, -4.0])
def test_scb_refs_equal_autograd(gate):
    """The block's element-wise steps restated in four lines of torch; `upd` stands for the attention output as an arbitrary
    differentiable function of q_in, kv_in and the right half of cat."""
    Bp, T, D = 2, 5, 12
    hf = R.rand((Bp, 2, T, D), 4, dtype=F64).requires_grad_(True)
    gt = torch.tensor([gate], dtype=F64, requires_grad=True)
    a1, a2, a3 = (R.rand((Bp, T, D), 5 + i, dtype=F64) for i in range(3))
    g = R.rand((Bp, 2, T, D), 9, dtype=F64)
    q_in, kv_in = hf[:, 0], hf[:, 1]
    cat_right = q_in
    upd = q_in * a1 + kv_in * a2 + cat_right * a3
    out = hf + torch.stack((torch.tanh(gt) * upd, torch.zeros_like(upd)), 1)
    (out * g).sum().backward()
    q_ref, kv_ref = R.scb_split_ref(hf.detach().float().reshape(-1, D), Bp, T, D)
    assert torch.equal(q_ref, q_in.detach().reshape(-1, D).float().bfloat16()) and torch.equal(kv_ref, kv_in.detach().reshape(-1, D).float().bfloat16())
    fwd = R.scb_merge_fwd_ref(hf.detach().reshape(-1), upd.detach().reshape(-1), gt.detach(), Bp, T, D)
    assert float((fwd - out.detach().reshape(-1)).abs().max()) < 1e-14
    d_upd, S, A, f = R.scb_gate_bwd_ref(g.reshape(-1), upd.detach().reshape(-1), gt.detach(), Bp, T, D)
    assert abs(float(f * S) - float(gt.grad)) < 1e-12 and float(A) >= abs(float(S))
    d_upd = d_upd.reshape(Bp, T, D)
    gin = R.scb_merge_bwd_ref(g.reshape(-1), d_upd * a1, d_upd * a3, d_upd * a2, Bp, T, D)
    assert float((gin - hf.grad.reshape(-1)).abs().max()) < 1e-13


@pytest.mark.parametrize("use_mask", [0b1111, 0b0110, 0b0000])
def test_combine_refs_equal_autograd(use_mask):
    from tests.util import hashed_stno
    B, T, D = 3, 50, 8
    stno = hashed_stno(B, T, "glue.host")
    y4 = R.rand((B, T, 4, D), 12).bfloat16().double().requires_grad_(True)
    h = R.rand((B, T, D), 13, dtype=F64).requires_grad_(True)
    g = R.rand((B, T, D), 14)
    m = stno.double().permute(0, 2, 1)
    out = sum(m[:, :, c, None] * (y4[:, :, c] if (use_mask >> c) & 1 else h) for c in range(4))
    (out * g.double()).sum().backward()
    ref, mag = R.combine_fwd_ref(y4.detach(), h.detach(), stno, use_mask)
    assert float((ref - out.detach()).abs().max()) < 1e-14 and bool((mag >= ref.abs() - 1e-14).all())
    d_y4, dh = R.combine_bwd_ref(g, stno, use_mask)
    # the exact emulation is within one fp32 + one bf16 rounding (d_y4) / a few fp32 roundings (dh) of autograd
    for c in range(4):
        if (use_mask >> c) & 1:
            want = y4.grad[:, :, c]
            assert bool(((d_y4[:, :, c].double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all())
        else:
            assert float(d_y4[:, :, c].float().abs().max()) == 0.0
    want = h.grad if use_mask != 0b1111 else torch.zeros_like(h)
    assert bool(((dh.double() - want).abs() <= 8 * R.U * want.abs() + 1e-30).all())
    if use_mask == 0b1111:
        assert float(dh.abs().max()) == 0.0


def test_exact_refs_against_plain_loops():
    """The permutation references, element by element."""
    O, C, kpad = 3, 2, 8
    w = R.rand((O, C, 3), 20)
    p = R.conv_pack_ref(w, kpad)
    gp = R.rand((O, kpad), 21)
    gw = R.rand((O, C, 3), 22)
    u = R.conv_unpack_ref(gw, gp)
    for o in range(O):
        for c in range(C):
            for j in range(3):
                assert float(p[o, j * C + c]) == float(w[o, c, j].bfloat16())
                assert float(u[o, c, j]) == float(gw[o, c, j] + gp[o, j * C + c])
        assert float(p[o, 3 * C:].float().abs().max()) == 0.0
    mel = R.rand((2, 3, 5), 23)
    tm = R.mel_timemajor_ref(mel)
    assert tm.shape == (2, 7, 3) and float(tm[:, 0].float().abs().max()) == 0.0 and float(tm[:, 6].float().abs().max()) == 0.0
    assert torch.equal(tm[1, 4], mel[1, :, 3].bfloat16())
    ids = torch.tensor([[0, 4, 4], [2, 0, 4]])
    tok, pos, g = R.rand((5, 4), 24), R.rand((6, 4), 25), R.rand((2, 3, 4), 26)
    e = R.embed_fwd_ref(ids, tok, pos)
    assert torch.equal(e[1, 2], tok[4] + pos[2])
    d_tok, d_pos, a_tok, a_pos = R.embed_bwd_ref(ids, g, 5, 6)
    assert float((d_tok[4] - (g[0, 1].double() + g[0, 2].double() + g[1, 2].double())).abs().max()) < 1e-15
    assert float((d_pos[1] - (g[0, 1].double() + g[1, 1].double())).abs().max()) < 1e-15 and float(d_pos[3:].abs().max()) == 0.0
    assert float(d_tok[1].abs().max()) == 0.0 and bool((a_tok >= d_tok.abs()).all()) and bool((a_pos >= d_pos.abs()).all())
    s = R.sum_over_batch_ref(torch.ones(4), torch.tensor([[1e8, 1.0, 2.0, 3.0], [-1e8, 1.0, 2.0, 3.0]]))
    assert s.tolist() == [0.0, 3.0, 5.0, 7.0]                        # (1 + 1e8) - 1e8 = 0 in fp32: the order is the batch order


def test_cast_values_hold_the_edges():
    x = R.cast_values(1027)
    b = x.bfloat16()
    ib = R.bits(b).int() & 0xFFFF
    assert ib[:4].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]         # ties go to the even neighbour
    assert torch.isinf(b[13:18]).all() and int(ib[18]) == 0x7F7F          # +-inf, +-max and the tie above bf16 max give inf
    assert R.bits(x[-19:]).tolist() == R.bits(x[:19]).flip(0).tolist()   # the same values sit in the scalar tail
    assert float(x[8]) != 0.0 and float(x[8]) < 1.2e-38                   # an fp32 denormal


@pytest.mark.parametrize("rows,N", [(1, 2), (17, 6), (100, 514), (513, 1280)])
def test_summation_bound_holds_for_a_sequential_fp32_sum(rows, N):
    """colsum-shaped inputs (bf16 values, a non-zero initial value as one more term): the fp32 sum in index order is within the
    bound, and the bound is tight enough to see one dropped row."""
    x = R.rand((rows, N), 200 + rows + N, 1.0).bfloat16()             # (the tensors of test_gpu_glue_kernels.py::test_colsum_bf16)
    out0 = R.rand((N,), 201, 2.0)
    terms = torch.cat((out0[None], x.float()), 0)
    seq = torch.cumsum(terms, 0, dtype=torch.float32)[-1]
    ref = terms.double().sum(0)
    bound = R.sum_bound(terms.double().abs().sum(0), rows + 1, ref)
    assert bool(((seq.double() - ref).abs() <= bound).all())
    if rows <= 100:
        dropped = ref - x[rows // 2].double()
        assert float(((dropped - ref).abs() > bound).float().mean()) > 0.5


@pytest.mark.parametrize("n", [1, 4, 1027, 2097152 + 1027])
def test_summation_bound_holds_for_sumsq(n):
    x = R.rand((n,), 400, 1.0)                                        # (the tensor of test_gpu_glue_kernels.py::test_sumsq)
    seq = torch.cumsum(x * x, 0, dtype=torch.float32)[-1]
    ref = float((x.double() ** 2).sum())
    assert abs(float(seq) - ref) <= float(R.sum_bound(ref, n + 1, ref, product_terms=True))


def _logmel_cases():
    return [(f"noise n={n}", ("noise", n)) for n in R.LOGMEL_LENGTHS[:-1]] + [(s, (s, R.LOGMEL_N)) for s in R.LOGMEL_SIGNALS]


@pytest.mark.parametrize("n_mels", [80, 128])
def test_fp32_logmel_restatement_holds_its_bound(n_mels):
    """Every waveform of tests/test_gpu_logmel_edges.py: an honest fp32 evaluation stays within 3e-5 of the fp64 oracle (measured
    on the CPU: at most 1.2e-5, the sine and the square wave), a tenth of what the suite allows the kernel."""
    worst = 0.0
    for name, (sig, n) in _logmel_cases():
        x = R.logmel_signal(sig, n)
        ref = R.logmel_oracle(x, n_mels)
        got = R.logmel_fp32(x, n_mels)
        assert got.shape == ref.shape == (n_mels, n // 160)
        d = float(np.abs(got.astype(np.float64) - ref).max())
        worst = max(worst, d)
        assert d <= 3e-5, (name, d)
        if sig == "zeros":
            assert float(np.abs(ref + 1.5).max()) == 0.0
    print(f"glue_ref: fp32 log-mel restatement, n_mels={n_mels}: worst {worst:.3e}")

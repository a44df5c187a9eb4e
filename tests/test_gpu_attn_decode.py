"""dicow_attn_decode (ops.attn_decode) on the MI355X against fp64 softmax attention: one query row per decoder row, the K/V row
chosen per query row -- by group (the beams of a window share its cross-attention K/V) or through an ancestry table (the
self-attention caches of a beam search are never reordered).  Run with `pytest -m gpu`."""
import functools

import pytest
import torch

import amd_pkg

pytestmark = pytest.mark.gpu
amd_pkg.load()

TOL = 2e-2          # the bound of test_attn_fwd_single_query_row for the same quantity at the same input scale
SHARED = [(2, 1, 3, 1), (1, 3, 2, 67), (3, 5, 2, 1500), (2, 8, 4, 448)]          # (B0, group, H, Lk)
ANCESTRY = [(2, 5, 3, 1), (3, 3, 2, 130), (2, 5, 20, 448)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ts_asr_whisper_amd import ops as o
    return o


def _bf(t):
    return t.to(torch.bfloat16)


def _attend(q, k, v):
    """fp64 softmax(q k^T) v, scaling 1: q [R,H,64], k / v [R,Lk,H,64] (already gathered per row)."""
    s = torch.einsum("rhd,rthd->rht", q.double(), k.double())
    return torch.einsum("rht,rthd->rhd", torch.softmax(s, dim=-1), v.double())


@functools.lru_cache(maxsize=None)
def _shared_case(B0, group, H, Lk):
    """Inputs on the CPU (bf16 values) and the fp64 reference, computed once per case."""
    g = torch.Generator().manual_seed(100 + Lk + group)
    D, R = H * 64, B0 * group
    q = _bf(torch.randn(R, H, 64, generator=g) * 0.3)
    ckv = _bf(torch.randn(B0 * Lk, 2 * D, generator=g))             # packed K | V rows, as the decoder's ckv
    k = ckv[:, :D].reshape(B0, Lk, H, 64)
    v = ckv[:, D:].reshape(B0, Lk, H, 64)
    ref = _attend(q, k.repeat_interleave(group, dim=0), v.repeat_interleave(group, dim=0))
    return q, ckv, ref


@functools.lru_cache(maxsize=None)
def _ancestry_case(B0, group, H, Lk):
    g = torch.Generator().manual_seed(200 + Lk + group)
    D, R, Lbuf = H * 64, B0 * group, Lk + 7
    q = _bf(torch.randn(R, H, 64, generator=g) * 0.3)
    k = _bf(torch.randn(R, Lbuf, D, generator=g))                   # independent content in every slot
    v = _bf(torch.randn(R, Lbuf, D, generator=g))
    anc = (torch.randint(0, group, (R, Lbuf), generator=g) + (torch.arange(R) // group * group)[:, None]).to(torch.int32)
    t = torch.arange(Lk)
    kg = k[anc[:, :Lk].long(), t[None, :]].reshape(R, Lk, H, 64)    # explicit gather: key t of row r from slot anc[r, t]
    vg = v[anc[:, :Lk].long(), t[None, :]].reshape(R, Lk, H, 64)
    return q, k, v, anc, _attend(q, kg, vg)


def _views(ckv, B0, Lk, H):
    """K and V as [B0, Lk, H, 64] views into the packed buffer (row stride 2D)."""
    D = H * 64
    mk = lambda t: t.as_strided((B0, Lk, H, 64), (Lk * 2 * D, 2 * D, 64, 1), t.storage_offset())
    return mk(ckv[:, :D]), mk(ckv[:, D:])


def _run_shared(ops, B0, group, H, Lk):
    q, ckv, ref = _shared_case(B0, group, H, Lk)
    qd, cd = q.cuda(), ckv.cuda()
    k, v = _views(cd, B0, Lk, H)
    o = torch.zeros_like(qd)
    ops.attn_decode(qd, k, v, o, group=group)
    torch.cuda.synchronize()
    return o, ref


def _run_ancestry(ops, B0, group, H, Lk):
    q, k, v, anc, ref = _ancestry_case(B0, group, H, Lk)
    R = q.shape[0]
    qd, kd, vd, ad = q.cuda(), k.cuda(), v.cuda(), anc.cuda()
    o = torch.zeros_like(qd)
    ops.attn_decode(qd, kd[:, :Lk].view(R, Lk, H, 64), vd[:, :Lk].view(R, Lk, H, 64), o, group=group, anc=ad)
    torch.cuda.synchronize()
    return o, ref


@pytest.mark.parametrize("B0,group,H,Lk", SHARED)
def test_shared_mode_vs_fp64(ops, B0, group, H, Lk):
    """Row r reads slot r // group: each window's K/V serve its `group` rows.  Lk 1, an Lk below one trip of the kernel, the
    encoder length 1500 (no multiple of the 128 / 256 keys a trip covers) and the largest group."""
    o, ref = _run_shared(ops, B0, group, H, Lk)
    diff = float((o.double().cpu() - ref).abs().max())
    print(f"shared {(B0, group, H, Lk)}: maxdiff {diff:.3e}")
    assert diff < TOL


@pytest.mark.parametrize("B0,group,H,Lk", ANCESTRY)
def test_ancestry_mode_vs_fp64(ops, B0, group, H, Lk):
    """Key / value t of row r come from slot anc[r, t] (random within the row's group; anc_rs = Lk + 7, caches longer than Lk).
    Every slot holds independent N(0, 1) content, so reading a wrong slot for even a few positions changes the output by O(1),
    far above the bound."""
    o, ref = _run_ancestry(ops, B0, group, H, Lk)
    diff = float((o.double().cpu() - ref).abs().max())
    print(f"ancestry {(B0, group, H, Lk)}: maxdiff {diff:.3e}")
    assert diff < TOL


def test_two_launches_are_bit_equal(ops):
    """Fixed summation order: the largest case of each mode twice."""
    a, _ = _run_shared(ops, *SHARED[2])
    b, _ = _run_shared(ops, *SHARED[2])
    assert torch.equal(a, b)
    a, _ = _run_ancestry(ops, *ANCESTRY[2])
    b, _ = _run_ancestry(ops, *ANCESTRY[2])
    assert torch.equal(a, b)


def test_argument_errors_raise_and_leave_the_library_usable(ops):
    """Every invalid argument set is refused with DicowError before any launch (the output keeps its fill value), and a valid
    launch afterwards still gives the right answer.  (Out-of-range TABLE ENTRIES are not an argument error: the kernel clamps
    them, which is reviewed in the source, not exercised here.)"""
    from ts_asr_whisper_amd import _lib as L
    B0, group, H, Lk = 2, 3, 2, 9
    D, R = H * 64, B0 * group
    g = torch.Generator().manual_seed(7)
    q = _bf(torch.randn(R, H, 64, generator=g) * 0.3).cuda()
    k = _bf(torch.randn(R, Lk, H, 64, generator=g)).cuda()
    v = _bf(torch.randn(R, Lk, H, 64, generator=g)).cuda()
    anc = torch.arange(R, dtype=torch.int32)[:, None].repeat(1, Lk).cuda()
    o = torch.full_like(q, 7.0)

    def args(shared, **over):
        a = L.AttnDecodeArgs()
        a.q, a.o, a.k, a.v = q.data_ptr(), o.data_ptr(), k.data_ptr(), v.data_ptr()
        a.q_rs = a.o_rs = D
        a.k_bs = a.v_bs = Lk * D
        a.k_rs = a.v_rs = D
        a.R, a.H, a.Lk, a.group = R, H, Lk, group
        a.n_slots = B0 if shared else R
        if not shared:
            a.anc, a.anc_rs = anc.data_ptr(), Lk
        for name, val in over.items():
            setattr(a, name, val)
        return a

    bad = [args(True, group=0, n_slots=R), args(True, group=-2), args(True, group=L.ATTN_DECODE_MAX_GROUP + 1),
           args(True, group=4), args(True, group=4, n_slots=1),                       # R % group != 0
           args(True, Lk=0), args(False, Lk=0), args(True, Lk=-3),
           args(True, n_slots=R), args(True, n_slots=B0 + 1), args(False, n_slots=B0), args(False, n_slots=R - 1),
           args(False, anc_rs=Lk - 1), args(False, anc_rs=0),
           args(True, q=None), args(True, k=None), args(True, v=None), args(True, o=None), args(False, q=None)]
    for i, a in enumerate(bad):
        with pytest.raises(L.DicowError, match="attn_decode"):
            L.call_struct("dicow_attn_decode", a)
    with pytest.raises(L.DicowError):                                # the tensor-level wrapper passes the refusal on
        ops.attn_decode(q, k[:B0], v[:B0], o, group=0)
    with pytest.raises(L.DicowError):
        ops.attn_decode(q, k, v, o, anc=anc[:, :Lk - 1])
    with pytest.raises(L.DicowError):
        ops.attn_decode(q.float(), k, v, o)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                     # nothing was launched
    ops.attn_decode(q, k[:B0], v[:B0], o, group=group)
    ref = _attend(q.cpu(), k[:B0].cpu().repeat_interleave(group, dim=0), v[:B0].cpu().repeat_interleave(group, dim=0))
    assert float((o.double().cpu() - ref).abs().max()) < TOL
    ops.attn_decode(q, k, v, o, anc=anc)                              # identity table: every row reads its own slot
    assert float((o.double().cpu() - _attend(q.cpu(), k.cpu(), v.cpu())).abs().max()) < TOL

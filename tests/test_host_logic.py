"""CPU tests of the host-side logic: STNO builder bit-exactness, config, C-ABI library symbols, state-dict surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import amd_pkg
from tests.util import load_golden, ROOT

pkg = amd_pkg.load()


def test_product_stno_builder_bit_exact_vs_reference_golden():
    from ts_asr_whisper_amd import data
    z = load_golden("f1_stno")
    for i in range(int(z["n_cases"])):
        got = data.create_stno_masks(z[f"in_{i}"].copy(), int(z[f"idx_{i}"]))
        assert np.array_equal(got, z[f"out_{i}"]), i


def test_collate_stno_padding_is_silence():
    from ts_asr_whisper_amd import data
    out = data.collate_stno([np.full((3, 4), 0.25, np.float32), np.full((5, 4), 0.25, np.float32)])
    assert out.shape == (2, 4, 5) and np.all(out[0, 0, 3:] == 1) and np.all(out[0, 1:, 3:] == 0)


def test_library_exports_every_declared_symbol():
    """include/dicow_hip.h is the ABI: every function it declares must be exported by the built library and bound."""
    from ts_asr_whisper_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dicow_hip.h")).read()
    stable, experimental = hdr.split("#ifdef DICOW_EXPERIMENTAL_ABI")
    assert set(re.findall(r"^int\s+(dicow_\w+)\s*\(", experimental, flags=re.M)) == set(_lib._SIGS_EXPERIMENTAL)
    hdr = stable                           # (the experimental tail is declared only under DICOW_EXPERIMENTAL_ABI and not exported by default)
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(dicow_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 25
    assert declared == set(_lib.declared_symbols())
    lib = _lib.lib()                       # raises loudly if the .so has not been built
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.dicow_abi_version() == 7
    if not _lib.has_experimental():        # the shipped build: nothing but the stable ABI is exported
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T dicow_" in ln}
        assert exported == declared, exported ^ declared


def test_gemm_nt_is_persistent_host_logic():
    """dicow_gemm_nt_is_persistent is host logic (no launch): the headline fc2 shape runs on the persistent kernel -- the only one
    that implements DICOW_EPI_FDDT -- and a decoder-sized or ragged-K problem does not.  Also pins the ctypes layout of
    dicow_gemm_args up to the fields the predicate reads."""
    import ctypes as C
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()

    def q(M, N, K, batch=1):
        a = _lib.GemmArgs()
        a.A = a.B = a.C = 1 << 20
        a.M, a.N, a.K = M, N, K
        a.lda, a.ldb, a.ldc, a.ldr, a.ldaux, a.batch = K, K, N, N, N, batch
        return lib.dicow_gemm_nt_is_persistent(C.byref(a))

    assert q(24000, 1280, 5120) == 1 and q(24000, 5120, 1280) == 1 and q(12000, 1536, 512) == 1
    assert q(1024, 512, 512) == 0 and q(24000, 1280, 64) == 0 and q(200, 1280, 1280) == 0
    assert q(12000, 512, 2048) == 0                      # whisper-base's N = 512 shapes stay on the 128 x 128 kernel
    assert _lib.EPI_FDDT == 1024 and C.sizeof(_lib.GemmArgs) % 8 == 0


# ------------------------------------------------------------------------------------------------ row-kernel routing
_PTR = 1 << 20          # null-but-nonzero dummy pointer: the plans read pointers only as present / absent
_ROW_WIDTHS = (252, 256, 1280, 1536, 2048, 2052, 2304, 4096)


def _rows_fwd_args(D, rows=8, mode=1, ln=True, in_bf16=False, h_out=True, y_bf16=True, y_f32=False, stats=True, pos=False, missing=None):
    from ts_asr_whisper_amd import _lib
    a = _lib.FddtLnFwdArgs()
    a.h_in, a.in_bf16, a.mode, a.rows, a.D, a.T, a.eps = _PTR, int(in_bf16), mode, rows, D, 4, 1e-5
    if mode != 0:
        a.stno, a.stno_bstride = _PTR, 16
        for c in range(4):
            a.w[c] = _PTR if mode == 1 and missing != ("w", c) else None
            a.b[c] = _PTR if missing != ("b", c) else None
    a.pos, a.h_out = (_PTR if pos else None), (_PTR if h_out else None)
    a.ln_w = a.ln_b = _PTR if ln else None
    a.y_bf16, a.y_f32 = (_PTR if y_bf16 else None), (_PTR if y_f32 else None)
    a.mean = a.rstd = _PTR if stats else None
    return a


def _rows_bwd_args(D, rows=8, mode=1, ln=True, in_bf16=False, dy_f32=False, g_res=True, g_out=True, g_out_bf16=True, pos=False, missing=None):
    from ts_asr_whisper_amd import _lib
    a = _lib.FddtLnBwdArgs()
    a.h_in, a.in_bf16, a.mode, a.rows, a.D, a.T = _PTR, int(in_bf16), mode, rows, D, 4
    if mode != 0:
        a.stno, a.stno_bstride = _PTR, 16
        for c in range(4):
            a.w[c] = _PTR if mode == 1 and missing != ("w", c) else None
            a.b[c] = _PTR if missing != ("b", c) else None
    a.pos = _PTR if pos else None
    if ln:
        a.ln_w = a.mean = a.rstd = a.d_y = _PTR
    a.dy_f32 = int(dy_f32)
    a.g_res, a.g_out, a.g_out_bf16 = (_PTR if g_res else None), (_PTR if g_out else None), (_PTR if g_out_bf16 else None)
    return a


# Expected routes, read off the dispatchers' conditions as they stood before the plans existed (block = D / 4 threads rounded up to
# a wave; "wave width" = D a multiple of 256 in 512..1280):
#   forward   staged       block <= 512, block * 4 == D, mode 1, LayerNorm, fp32 in, h_out, y_bf16, no y_f32, mean + rstd, no pos, all
#                          eight FDDT vectors, rows * D * 4 < 2^31
#             init_wave    mode 1, no LayerNorm, bf16 in, h_out, pos, no y, wave width, all eight vectors
#             ln_wave      mode 0, LayerNorm, fp32 in, no h_out, no pos, wave width, some y
#             generic_*    block > 512: generic_1024; else by mode: 0 generic_ln, 1 generic_diag, 2 generic
#   backward  ln_wave      block <= 512, mode 0, LayerNorm, fp32 in, no pos, wave width, g_out or g_out_bf16
#             generic_1024 block > 512
#             staged_*     block <= 512, block * 4 == D, mode 1, LayerNorm, fp32 in, bf16 d_y, g_res, g_out, no pos, all eight vectors,
#                          rows * D * 4 < 2^31; _bf16 with g_out_bf16, _f32 without
#             ln_only      block <= 512, mode 0, LayerNorm;   generic: the rest
# rows * D is a multiple of 256 wherever the byte guard decides, so the last size below 2^31 is 2^31 - 1024 (D = 256), not 2^31 - 4.
_LAYER, _INIT, _LN = {}, dict(ln=False, in_bf16=True, y_bf16=False, stats=False, pos=True), dict(mode=0, h_out=False)
_ROWS_FWD_ROUTES = [
    (252, _LAYER, "generic_diag"), (256, _LAYER, "staged"), (1280, _LAYER, "staged"), (1536, _LAYER, "staged"), (2048, _LAYER, "staged"),
    (2052, _LAYER, "generic_1024"), (2304, _LAYER, "generic_1024"), (4096, _LAYER, "generic_1024"),
    (1280, dict(pos=True), "generic_diag"), (1280, dict(y_f32=True), "generic_diag"), (1280, dict(in_bf16=True), "generic_diag"),
    (1280, dict(missing=("w", 2)), "generic_diag"), (1280, dict(missing=("b", 3)), "generic_diag"), (1280, dict(stats=False), "generic_diag"),
    (1280, dict(y_bf16=False, y_f32=True), "generic_diag"), (1280, dict(h_out=False), "generic_diag"),
    (256, dict(rows=(1 << 21) - 1), "staged"), (256, dict(rows=1 << 21), "generic_diag"),
    (252, _INIT, "generic_diag"), (256, _INIT, "generic_diag"), (512, _INIT, "init_wave"), (1280, _INIT, "init_wave"), (1536, _INIT, "generic_diag"),
    (2048, _INIT, "generic_diag"), (2052, _INIT, "generic_1024"), (2304, _INIT, "generic_1024"), (4096, _INIT, "generic_1024"),
    (1280, dict(_INIT, pos=False), "generic_diag"), (1280, dict(_INIT, in_bf16=False), "generic_diag"),
    (1280, dict(_INIT, missing=("b", 0)), "generic_diag"), (1280, dict(_INIT, y_f32=True), "generic_diag"),
    (252, _LN, "generic_ln"), (256, _LN, "generic_ln"), (512, _LN, "ln_wave"), (1280, _LN, "ln_wave"), (1536, _LN, "generic_ln"),
    (2048, _LN, "generic_ln"), (2052, _LN, "generic_1024"), (2304, _LN, "generic_1024"), (4096, _LN, "generic_1024"),
    (1280, dict(_LN, y_bf16=False, y_f32=True), "ln_wave"), (1280, dict(_LN, y_f32=True), "ln_wave"), (1280, dict(_LN, h_out=True), "generic_ln"),
    (1280, dict(_LN, in_bf16=True), "generic_ln"), (1280, dict(_LN, pos=True), "generic_ln"),
    (1280, dict(mode=2), "generic"), (252, dict(mode=2), "generic"), (2304, dict(mode=2), "generic_1024"),
    (1280, dict(mode=0, ln=False, y_bf16=False, stats=False), "generic_ln"),              # a plain copy
    (1282, _LAYER, None), (4100, _LAYER, None), (1280, dict(rows=0), None), (1280, dict(mode=3), None),
    (1280, dict(ln=False, h_out=False, y_bf16=False), None),
]
_BLN = dict(mode=0)
_ROWS_BWD_ROUTES = [
    (252, _LAYER, "generic"), (256, _LAYER, "staged_bf16"), (1280, _LAYER, "staged_bf16"), (1536, _LAYER, "staged_bf16"),
    (2048, _LAYER, "staged_bf16"), (2052, _LAYER, "generic_1024"), (2304, _LAYER, "generic_1024"), (4096, _LAYER, "generic_1024"),
    (256, dict(g_out_bf16=False), "staged_f32"), (1280, dict(g_out_bf16=False), "staged_f32"), (2048, dict(g_out_bf16=False), "staged_f32"),
    (252, dict(g_out_bf16=False), "generic"), (2304, dict(g_out_bf16=False), "generic_1024"),
    (1280, dict(missing=("w", 0)), "generic"), (1280, dict(missing=("b", 1)), "generic"), (1280, dict(dy_f32=True), "generic"),
    (1280, dict(in_bf16=True), "generic"), (1280, dict(pos=True), "generic"), (1280, dict(g_res=False), "generic"),
    (1280, dict(g_out=False), "generic"), (1280, dict(ln=False), "generic"),
    (256, dict(rows=(1 << 21) - 1), "staged_bf16"), (256, dict(rows=1 << 21), "generic"),
    (252, _BLN, "ln_only"), (256, _BLN, "ln_only"), (512, _BLN, "ln_wave"), (1280, _BLN, "ln_wave"), (1536, _BLN, "ln_only"),
    (2048, _BLN, "ln_only"), (2052, _BLN, "generic_1024"), (2304, _BLN, "generic_1024"), (4096, _BLN, "generic_1024"),
    (1280, dict(_BLN, g_out_bf16=False), "ln_wave"), (1280, dict(_BLN, g_out=False), "ln_wave"),
    (1280, dict(_BLN, g_out=False, g_out_bf16=False), "ln_only"), (1280, dict(_BLN, in_bf16=True), "ln_only"),
    (1280, dict(_BLN, pos=True), "ln_only"), (1280, dict(_BLN, g_res=False), "ln_wave"),
    (1280, dict(mode=0, ln=False), "generic"), (1280, dict(mode=2), "generic"), (2304, dict(mode=2), "generic_1024"),
    (1282, _LAYER, None), (4100, _LAYER, None), (1280, dict(rows=0), None), (1280, dict(mode=3), None),
    (1280, dict(mode=0, ln=False, g_res=False), None),
]


def test_row_kernel_routes_host_logic():
    """dicow_fddt_ln_fwd_route / _bwd_route are host logic (no launch): every kernel body is reached by the arguments that reached it
    before the dispatch was a plan, on both sides of every boundary -- width, pos / y_f32 / in_bf16, a missing FDDT vector, the bf16
    gradient copy, the 2 GiB guard of the LDS-staged bodies -- and rejected arguments answer NULL."""
    import ctypes as C
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()
    for table, build, query in ((_ROWS_FWD_ROUTES, _rows_fwd_args, lib.dicow_fddt_ln_fwd_route),
                                (_ROWS_BWD_ROUTES, _rows_bwd_args, lib.dicow_fddt_ln_bwd_route)):
        seen = set()
        for D, kw, want in table:
            got = query(C.byref(build(D, **kw)))
            assert (got.decode() if got is not None else None) == want, (build.__name__, D, kw, got, want)
            seen.add(want)
            seen.add(D)
        assert seen >= set(_ROW_WIDTHS)
        bodies = ({"staged", "init_wave", "ln_wave", "generic_ln", "generic_diag", "generic", "generic_1024"} if build is _rows_fwd_args
                  else {"ln_wave", "staged_bf16", "staged_f32", "ln_only", "generic", "generic_1024"})
        assert seen >= bodies | {None}
    assert query(None) is None


def test_row_backward_workspace_covers_every_route():
    """dicow_fddt_ln_bwd_ws_bytes holds the [workgroup][11][D] partial column sums of whichever backward body runs: a workgroup per 4
    rows, at most 256 x (4 LayerNorm-only / 1 staged / 2 generic; always 4 up to 256 threads) of them; the wave-per-row body one per
    8 rows, never more than the LayerNorm-only body."""
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()
    for rows in (1, 5, 1024, 1025, 24000):
        for D in _ROW_WIDTHS:
            block = (D // 4 + 63) // 64 * 64
            grids = [min((rows + 3) // 4, 256 * (4 if block <= 256 else per_cu)) for per_cu in (4, 1, 2)]
            grids.append(min((rows + 7) // 8, grids[0]))
            got = lib.dicow_fddt_ln_bwd_ws_bytes(rows, D)
            assert got >= max(grids) * 11 * D * 4, (rows, D, got)
            assert got == grids[0] * 11 * D * 4, (rows, D, got)          # and no more than the largest of them


# ------------------------------------------------------------------------------------------------ attention routing
def _attn_fwd_args(B=2, H=3, Lq=100, Lk=100, q_log2=0, causal=0, **over):
    from ts_asr_whisper_amd import _lib
    a = _lib.AttnFwdArgs()
    a.q = a.k = a.v = a.o = a.lse = _PTR
    a.B, a.H, a.Lq, a.Lk, a.causal, a.q_log2 = B, H, Lq, Lk, causal, q_log2
    a.q_rs = a.k_rs = a.v_rs = 3 * H * 64
    a.o_rs = H * 64
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = Lq * 3 * H * 64, Lk * 3 * H * 64, Lk * 3 * H * 64, Lq * H * 64
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _attn_bwd_args(B=8, H=16, Lq=256, Lk=1024, causal=0, fused_mode=0, ws="exact", colsums=False, cs_ws=True, **over):
    """ws: the fused workspace -- "exact" (dicow_attn_bwd_fused_ws_bytes), "short" (one byte less), "unaligned", or None."""
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()
    a = _lib.AttnBwdArgs()
    a.q = a.k = a.v = a.o = a.d_o = a.lse = a.delta = a.dq = a.dk = a.dv = _PTR
    a.B, a.H, a.Lq, a.Lk, a.causal, a.fused_mode, a.dq_scale = B, H, Lq, Lk, causal, fused_mode, 1.0
    for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
        setattr(a, n + "_rs", H * 64)
        setattr(a, n + "_bs", (Lq if n in ("q", "o", "do", "dq") else Lk) * H * 64)
    if ws is not None:
        a.fused_ws = _PTR + (8 if ws == "unaligned" else 0)
        a.fused_ws_bytes = lib.dicow_attn_bwd_fused_ws_bytes(B, H, Lq, Lk) - (1 if ws == "short" else 0)
    if colsums:
        a.dq_colsum = a.dv_colsum = _PTR
        if cs_ws:
            a.cs_ws, a.cs_ws_bytes = _PTR, lib.dicow_attn_bwd_colsum_ws_bytes(B, H, Lq, Lk)
    for k, v in over.items():
        setattr(a, k, v)
    return a


# Expected routes, read off dicow_attn_fwd / dicow_attn_bwd as they stood before the plans existed.
#   forward   q_log2 -> "occ4_spec", else "occ4"; invalid: a row stride not a multiple of 8, q/k/v batch strides not a multiple of 8 (o: 4),
#             an empty problem, B or H above 65535
#   backward  "fused": a 4096-aligned fused_ws of at least dicow_attn_bwd_fused_ws_bytes(), dense, B*H <= 1000, flag area
#             B*H*ceil(Lq/64)*4 * 4096 < 2^32, and -- unless fused_mode == 1 -- B*H*ceil(Lk/128) >= 1024 and Lq >= 256; else "dq_dkv";
#             invalid: fused_ws not 4096-aligned, column sums without cs_ws, a stride not a multiple of 4
_ATTN_FWD_ROUTES = [
    (dict(q_log2=0), "occ4"), (dict(q_log2=1), "occ4_spec"), (dict(q_log2=1, causal=1), "occ4_spec"), (dict(causal=1), "occ4"),
    (dict(B=65535, H=1), "occ4"), (dict(B=1, H=65535), "occ4"), (dict(B=65536, H=1), None), (dict(B=1, H=65536), None),
    (dict(q_rs=3 * 192 + 4), None), (dict(o_rs=12), None), (dict(k_bs=100 * 576 + 4), None), (dict(o_bs=100 * 192 + 4), "occ4"),
    (dict(o_bs=100 * 192 + 2), None), (dict(B=0), None), (dict(H=0), None), (dict(Lq=0), None), (dict(Lk=0), None), (dict(q=None), None),
]
_ATTN_BWD_ROUTES = [
    (dict(), "fused"), (dict(causal=1), "dq_dkv"),                                             # 8 x 16 pairs x 8 key blocks = 1024 workgroups
    (dict(Lk=896), "dq_dkv"), (dict(B=1, H=341, Lk=384), "dq_dkv"), (dict(B=2, H=256, Lk=256), "fused"),      # 896, 1023, 1024 workgroups
    (dict(Lq=255), "dq_dkv"), (dict(Lq=256), "fused"),
    (dict(B=8, H=125, Lk=256), "fused"), (dict(B=7, H=143, Lk=256), "dq_dkv"),                 # 1000 and 1001 pairs
    (dict(B=1, H=2, Lq=128, Lk=64), "dq_dkv"), (dict(B=1, H=2, Lq=128, Lk=64, fused_mode=1), "fused"),       # fused_mode 1 lifts both size thresholds
    (dict(Lq=255, fused_mode=1), "fused"), (dict(Lk=896, fused_mode=1), "fused"),
    (dict(fused_mode=1, causal=1), "dq_dkv"), (dict(B=7, H=143, Lk=256, fused_mode=1), "dq_dkv"),            # ... and nothing else
    (dict(fused_mode=1, ws=None), "dq_dkv"), (dict(fused_mode=1, ws="short"), "dq_dkv"),
    (dict(B=8, H=125, Lq=16769, Lk=256, fused_mode=1), "dq_dkv"),
    (dict(ws=None), "dq_dkv"), (dict(ws="short"), "dq_dkv"), (dict(ws="exact"), "fused"), (dict(ws="unaligned"), None),
    (dict(fused_mode=1, ws="unaligned"), None), (dict(causal=1, ws="unaligned"), None),
    (dict(B=8, H=125, Lq=16768, Lk=256), "fused"), (dict(B=8, H=125, Lq=16769, Lk=256), "dq_dkv"),          # the 2^32-byte flag area
    (dict(colsums=True), "fused"), (dict(colsums=True, ws=None), "dq_dkv"), (dict(colsums=True, cs_ws=False), None),
    (dict(colsums=True, cs_ws=False, ws=None), None), (dict(colsums=True, cs_ws_bytes=1), None),
    (dict(dq_rs=16 * 64 + 2), None), (dict(dv_bs=1024 * 1024 + 2), None), (dict(dk_rs=16 * 64 + 4), "fused"), (dict(q_rs=16 * 64 + 4), None),
    (dict(Lq=0), None), (dict(dv=None), None),
]


def test_attention_routes_host_logic():
    """dicow_attn_fwd_route / dicow_attn_bwd_route are host logic (no launch): both sides of every boundary of the dispatch as it stood
    before it was a plan, and rejected arguments answer NULL."""
    import ctypes as C
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()
    for table, build, query, names in ((_ATTN_FWD_ROUTES, _attn_fwd_args, lib.dicow_attn_fwd_route, {"occ4", "occ4_spec"}),
                                       (_ATTN_BWD_ROUTES, _attn_bwd_args, lib.dicow_attn_bwd_route, {"fused", "dq_dkv"})):
        seen = set()
        for kw, want in table:
            got = query(C.byref(build(**kw)))
            assert (got.decode() if got is not None else None) == want, (build.__name__, kw, got, want)
            seen.add(want)
        assert seen == names | {None}
        assert query(None) is None


def _attn_rs_limit(L):
    """The largest row stride (elements, a multiple of 8) attention's 32-bit tile offsets can address: (max(L, 65) - 1) * rs * 2 + 128 <
    2^32 (attention.hip check_tile_span: num_records of make_tile_src, the lane and tile offsets of stage_tile / stage_tile_x)."""
    return ((1 << 32) - 129) // (2 * (max(L, 65) - 1)) // 8 * 8


def test_attention_row_stride_limit_host_logic():
    """K and V (forward and backward), Q and dO (backward) are fetched with 32-bit byte offsets from the (batch, head) base: at the
    largest 8-multiple row stride inside the limit the route queries name a route, one step (+8) past it they answer NULL, and the
    other operands' row strides (q and o in the forward; o, dq, dk, dv in the backward) and every batch stride have no such limit."""
    import ctypes as C
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()
    for L in (100, 140, 260, 1500):
        rs = _attn_rs_limit(L)
        assert (L - 1) * rs * 2 + 128 < 1 << 32 <= (L - 1) * (rs + 8) * 2 + 128          # for L >= 65 this IS the span of the operand
    assert 64 * _attn_rs_limit(2) * 2 + 128 < 1 << 32 <= 64 * (_attn_rs_limit(2) + 8) * 2 + 128      # short operands: 65 rows count
    for Lq, Lk in ((100, 100), (140, 260), (2, 2)):
        for name, L in (("k_rs", Lk), ("v_rs", Lk)):
            rs = _attn_rs_limit(L)
            assert lib.dicow_attn_fwd_route(C.byref(_attn_fwd_args(Lq=Lq, Lk=Lk, **{name: rs}))) == b"occ4", (name, Lq, Lk)
            assert lib.dicow_attn_fwd_route(C.byref(_attn_fwd_args(Lq=Lq, Lk=Lk, **{name: rs + 8}))) is None, (name, Lq, Lk)
            assert b"2^32" in lib.dicow_last_error() and name[0].encode() in lib.dicow_last_error()
        for name in ("q_rs", "o_rs", "q_bs", "k_bs", "v_bs", "o_bs"):
            assert lib.dicow_attn_fwd_route(C.byref(_attn_fwd_args(Lq=Lq, Lk=Lk, **{name: 1 << 40}))) == b"occ4", name
        for fm, route in ((0, b"dq_dkv"), (1, b"fused")):
            kw = dict(B=2, H=2, Lq=Lq, Lk=Lk, fused_mode=fm)
            for name, L in (("k_rs", Lk), ("v_rs", Lk), ("q_rs", Lq), ("do_rs", Lq)):
                rs = _attn_rs_limit(L)
                assert lib.dicow_attn_bwd_route(C.byref(_attn_bwd_args(**kw, **{name: rs}))) == route, (name, Lq, Lk)
                assert lib.dicow_attn_bwd_route(C.byref(_attn_bwd_args(**kw, **{name: rs + 8}))) is None, (name, Lq, Lk)
                assert b"2^32" in lib.dicow_last_error()
            for name in ("o_rs", "dq_rs", "dk_rs", "dv_rs", "q_bs", "k_bs", "v_bs", "o_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs"):
                assert lib.dicow_attn_bwd_route(C.byref(_attn_bwd_args(**kw, **{name: 1 << 40}))) == route, name


def test_far_view_helpers_on_the_host():
    """tests/util's far-offset helpers without a GPU: the tall-stride recipe puts rows on both sides of the mark and finds a row that
    straddles it; far_view keeps the front pad; the stray count flags one stray byte, an overlap and a changed input."""
    from tests.util import Arena, far_view, tall_ld
    for rows, cols, isz, align in ((300, 128, 2, 8), (132, 128, 2, 8), (44, 1000, 2, 8), (1000, 500, 4, 4), (16, 1284, 2, 4)):
        ld, r = tall_ld(rows, cols, isz, align)
        assert ld % align == 0 and ld >= cols and (rows - 1) * ld * isz >= 1 << 32 and (rows // 2) * ld * isz < 1 << 32
        assert r is not None and r * ld * isz < 1 << 32 < (r * ld + cols) * isz
    ld, r = tall_ld(40, 16, 2, 8, mark=1 << 16)
    arena = Arena(1 << 20, device="cpu")
    vals = torch.randn(40, 16).bfloat16()
    v = far_view(arena, (40, 16), torch.bfloat16, (ld, 1), values=vals, name="x")
    span = (39 * ld + 16) * 2
    assert span > 1 << 16 and v.data_ptr() - arena.buf.data_ptr() >= span and torch.equal(v, vals)
    out = far_view(arena, (40, 16), torch.float32, (ld, 1), name="y", output=True)
    assert arena.check() == 40 * 16
    out.copy_(torch.randn(40, 16))
    assert arena.check() == 3 * 40 * 16
    arena.buf[6] = 0
    with pytest.raises(AssertionError, match="1 stray"):
        arena.check()
    arena.buf[6] = 0xC1
    far_view(arena, (40, 16), torch.bfloat16, (ld, 1), values=vals, base_bytes=v.data_ptr() - arena.buf.data_ptr(), name="overlap")
    with pytest.raises(AssertionError, match="stray"):
        arena.check()
    arena.inputs.pop()
    v[3, 3] = 2.0
    with pytest.raises(AssertionError, match="input operand was overwritten"):
        arena.check()
    with pytest.raises(AssertionError, match="front pad"):
        far_view(arena, (40, 16), torch.bfloat16, (ld, 1), values=vals, base_bytes=256, name="no pad")


def test_attn_bwd_fused_eligible_matches_the_former_python_rule():
    """dicow_attn_bwd_fused_eligible against the predicate that stood in ops.attn_bwd (moved here verbatim: `want` is True or "force").
    The two may differ only where the hand-off tiles would reach 2^32 bytes: the library never ran those fused, and ops.attn_bwd
    no longer allocates a workspace for them."""
    from ts_asr_whisper_amd import _lib
    lib = _lib.lib()

    def former(B, H, Lq, Lk, causal, want):
        return bool(want and not causal and B * H <= 1000 and (want == "force" or (B * H * ((Lk + 127) // 128) >= 1024 and Lq >= 256)))

    guarded, n = [], 0
    for B, H in ((1, 1), (2, 4), (27, 37), (8, 125), (7, 143)):                    # B*H = 1, 8, 999, 1000, 1001
        for Lk in (1, 127, 128, 129, 1024, 1500, 131072):
            for Lq in (1, 255, 256, 1500, 16768, 16769):
                for causal in (0, 1):
                    for fused_mode in (0, 1):
                        got = lib.dicow_attn_bwd_fused_eligible(B, H, Lq, Lk, causal, fused_mode)
                        want = former(B, H, Lq, Lk, causal, "force" if fused_mode else True)
                        n += 1
                        if B * H * ((Lq + 63) // 64) * 4 * 4096 >= 2 ** 32:        # the flag-area guard: 4 KB per (pair, 64-query tile, wave)
                            if want:
                                guarded.append((B, H, Lq, Lk, causal, fused_mode))
                            assert got == 0, (B, H, Lq, Lk, causal, fused_mode)
                        else:
                            assert got == int(want), (B, H, Lq, Lk, causal, fused_mode, got, want)
    assert n == 5 * 7 * 6 * 2 * 2 and guarded
    assert {(b * h, lq) for b, h, lq, *_ in guarded} == {(999, 16769), (1000, 16769)}


def test_no_cpu_fallback_and_oracle_not_imported_by_product():
    src_dir = os.path.join(ROOT, "ts-asr-whisper_amd")
    for fn in os.listdir(src_dir):
        if fn.endswith(".py"):
            txt = open(os.path.join(src_dir, fn)).read()
            assert "import oracle" not in txt and "from oracle" not in txt, fn
    m = pkg.FDDT(64, is_diagonal=True)
    with pytest.raises(Exception):
        m(torch.randn(1, 4, 64), torch.rand(1, 4, 4))


def test_state_dict_surface_matches_reference_keys():
    z = load_golden("f8_e2e_se")
    import ast
    d = ast.literal_eval(str(z["cfg"]))
    model = pkg.DiCoWForConditionalGeneration(pkg.DiCoWConfig(**d))
    assert set(model.state_dict().keys()) == {k[2:] for k in z.files if k.startswith("p.")}
    assert model.proj_out.weight is model.model.decoder.embed_tokens.weight


def test_reference_init_semantics():
    cfg = pkg.DiCoWConfig(d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=1, decoder_attention_heads=2,
                          encoder_ffn_dim=256, decoder_ffn_dim=256, vocab_size=512, max_source_positions=50, pad_token_id=500,
                          use_pre_pos_fddt=True, non_target_fddt_value=0.5, use_enrollments=True, scb_layers=1)
    m = pkg.DiCoWForConditionalGeneration(cfg)
    e = m.model.encoder
    for f in e.fddts:                       # per-layer FDDTs start as identity
        for c in ("silence_linear", "target_linear", "non_target_linear", "overlap_linear"):
            assert torch.all(getattr(f, c).weight == 1) and torch.all(getattr(f, c).bias == 0)
    i = e.initial_fddt
    assert torch.all(i.silence_linear.weight == 0.5) and torch.all(i.non_target_linear.weight == 0.5)
    assert torch.all(i.target_linear.weight == 1) and torch.all(i.overlap_linear.weight == 1)
    assert float(e.ca_enrolls[0].cae.cross_gate.gate) == 0.0
    assert not e.embed_positions.weight.requires_grad


def test_default_preheat_group_is_the_reference_prefix_list():
    """reference configs/base.yaml:18 + configs/train/se_dicow.yaml:13: FDDTs, the CTC branch and the enrollment cross-attention
    form the preheat group (lr x multiplier, weight decay 0, the only parameters of phase 1) -- by DEFAULT, as in the recipes."""
    from ts_asr_whisper_amd.trainer import FlatStore, REFERENCE_PREHEAT_PREFIXES, freeze_by_keyword
    cfg = pkg.DiCoWConfig(d_model=128, encoder_layers=2, encoder_attention_heads=2, decoder_layers=1, decoder_attention_heads=2,
                          encoder_ffn_dim=256, decoder_ffn_dim=256, vocab_size=512, max_source_positions=50, pad_token_id=500,
                          use_pre_pos_fddt=True, use_enrollments=True, scb_layers=1, ctc_weight=0.3, additional_layer=True,
                          additional_self_attention_layer=True, pre_ctc_sub_sample=True)
    m = pkg.DiCoWForConditionalGeneration(cfg)
    freeze_by_keyword(m, ("decoder",))
    store = FlatStore(m)
    names = {id(p): n for n, p in m.named_parameters()}
    pre = {names[id(p)] for p, _, _, is_pre in store.entries if is_pre}
    want = {n for n, p in m.named_parameters() if p.requires_grad and n.startswith(REFERENCE_PREHEAT_PREFIXES)}
    assert pre == want
    for part in ("fddts", "initial_fddt", "ca_enrolls", "lm_head", "additional_layer", "additional_self_attention_layer", "subsample_conv1"):
        assert any(("model.encoder." + part) in n for n in pre), part
    assert not any("layers." in n and "additional" not in n and "ca_enrolls" not in n for n in pre)


def test_config_rejects_unsupported():
    with pytest.raises(ValueError):
        pkg.DiCoWConfig(d_model=100, encoder_attention_heads=2, decoder_attention_heads=2)
    with pytest.raises(ValueError):
        pkg.DiCoWConfig(dropout=0.1)


def test_product_mel_filterbank_matches_oracle():
    from ts_asr_whisper_amd import features
    from oracle import logmel as ol
    for m in (80, 128):
        assert np.allclose(features.mel_filter_bank(m), ol.mel_filter_bank(m), atol=1e-12)


# ------------------------------------------------------------------------------------------------ augmentation planner
def _next_draw():
    return float(torch.rand(1))


def test_augment_planner_consumes_the_generator_like_the_reference_restatement():
    """The planner must make the same draws in the same order as the collator (pinned by the oracle against golden F11):
    after either one runs from the same seed the generator has to be in the same state."""
    from oracle import augment as oaug
    from ts_asr_whisper_amd import augment as paug
    stno = load_golden("f11_augment")["stno"]
    B, C, Tn = stno.shape
    torch.manual_seed(3)
    oaug.soft_segment_augmentation(stno.copy(), 0.3, 4, 30)
    a = _next_draw()
    torch.manual_seed(3)
    segs, coef = paug.plan_soft_segments(B, C, Tn, 0.3, 4, 30)
    assert _next_draw() == a
    assert segs.dtype == torch.int32 and segs.shape[1] == 4 and coef.shape == (segs.shape[0], 2)
    assert (segs[:, 2] > segs[:, 1]).all() and (segs[:, 2] - segs[:, 1] <= 30).all() and (segs[:, 3] < C - 1).all()
    assert torch.allclose(coef.sum(1), torch.ones(len(coef)))

    torch.manual_seed(4)
    oaug.add_gaussian_noise_and_rescale(stno.copy(), 0.2, 0.75)
    a = _next_draw()
    torch.manual_seed(4)
    rows, noise, sd = paug.plan_gaussian_noise(B, C, Tn, 0.2, 0.75)
    assert _next_draw() == a
    assert rows.numel() == int(B * 0.75) == noise.shape[0] and len(set(rows.tolist())) == rows.numel()
    assert sd == float(np.float32(0.2 ** 0.5))
    assert paug.plan_gaussian_noise(B, C, Tn, 0.2, 0.1) is None              # int(6 * 0.1) == 0 rows: no draw at all

    x = np.zeros((3, 400, 132), np.float32)
    torch.manual_seed(5)
    oaug.spec_aug(x)
    a = _next_draw()
    torch.manual_seed(5)
    plan = paug.plan_spec_aug(3, 400, 132)
    assert _next_draw() == a
    assert plan.fmask.shape == (3, 2, 2) and plan.tmask.shape == (3, 5, 2)
    assert 0 < plan.warped < 400 and abs(plan.warped - plan.center) <= 5
    assert int(plan.fmask[..., 1].max()) < 27 and int(plan.tmask[..., 1].max()) < 20
    assert int((plan.fmask[..., 0] + plan.fmask[..., 1]).max()) <= 128


def test_augment_planner_short_inputs_skip_the_warp():
    from ts_asr_whisper_amd import augment as paug
    torch.manual_seed(0)
    plan = paug.plan_spec_aug(2, 10, 132)               # T - window <= window: no warp draw (augmentations.py:101)
    assert plan.warped < 0
    assert plan.tmask.numel() == 0                      # floor(10 * 0.05) == 0: the ratio mask is skipped as well


def test_augment_refuses_cpu_tensors():
    from ts_asr_whisper_amd import augment as paug
    with pytest.raises(Exception, match="GPU"):
        paug.add_gaussian_noise_and_rescale(torch.rand(2, 4, 8), 0.2, 1.0)
    with pytest.raises(Exception, match="GPU"):
        paug.spec_aug_joint(torch.rand(1, 80, 20), torch.rand(1, 4, 10))


# ------------------------------------------------------------------------------------------------ optimizer schedule
def test_lr_schedule_matches_hf_cosine_with_warmup():
    """k-th optimizer step of FusedAdamW uses the lr HF's Trainer would (LambdaLR steps after the optimizer)."""
    import types
    import transformers
    from oracle.optim import cosine_with_warmup_lambda
    from ts_asr_whisper_amd.trainer import FusedAdamW
    store = types.SimpleNamespace(params=torch.zeros(1), runs=[])
    opt = FusedAdamW(store, lr=2e-6, warmup_steps=7, max_steps=50)
    ref_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=2e-6)
    sched = transformers.get_cosine_schedule_with_warmup(ref_opt, 7, 50)
    for k in range(1, 56):
        want = ref_opt.param_groups[0]["lr"]
        assert abs(opt.lr_at(k) - want) < 1e-18, k
        assert abs(2e-6 * cosine_with_warmup_lambda(k - 1, 7, 50) - want) < 1e-18
        ref_opt.step()
        sched.step()
    assert FusedAdamW(store, lr=1e-3).lr_at(1) == 1e-3            # no schedule configured: constant


def test_product_stno_seek_windows_match_reference_golden():
    from ts_asr_whisper_amd.generation import stno_seek_windows
    z = load_golden("f12_seek")
    for i in range(int(z["n_cases"])):
        got = stno_seek_windows(torch.from_numpy(z[f"c{i}.stno"]), z[f"c{i}.seek"], z[f"c{i}.max_frames"], z[f"c{i}.map"],
                                num_frames=int(z[f"c{i}.msp"]))
        assert np.array_equal(got.numpy(), z[f"c{i}.out"]), i


# ------------------------------------------------------------------------------------------------ checkpoints
def _tiny_cfg():
    return pkg.DiCoWConfig(vocab_size=256, d_model=64, encoder_layers=2, encoder_attention_heads=1, decoder_layers=1,
                           decoder_attention_heads=1, encoder_ffn_dim=128, decoder_ffn_dim=128, max_source_positions=20,
                           max_target_positions=16, pad_token_id=250, use_pre_pos_fddt=True)


def test_save_and_from_pretrained_round_trip(tmp_path):
    torch.manual_seed(0)
    m = pkg.DiCoWForConditionalGeneration(_tiny_cfg())
    m.save_pretrained(tmp_path / "ckpt")
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["config.json", "generation_config.json", "model.safetensors"]      # (round 6: an HF PreTrainedModel)
    m2 = pkg.DiCoWForConditionalGeneration.from_pretrained(str(tmp_path / "ckpt"))
    assert m2._load_report == {"missing": [], "unexpected": []}
    for (n, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), n
    assert m2.proj_out.weight is m2.model.decoder.embed_tokens.weight          # tied after loading
    assert m2.config.to_dict() == m.config.to_dict()


def test_from_pretrained_plain_whisper_checkpoint_keeps_fddt_init(tmp_path):
    """A checkpoint without the FDDT keys (plain Whisper): they are reported missing and keep the reference initialisation,
    overrides reach the config (containers.py:47-50 passes the DiCoW switches as from_pretrained kwargs)."""
    from safetensors.torch import save_file
    import json
    torch.manual_seed(0)
    m = pkg.DiCoWForConditionalGeneration(_tiny_cfg())
    sd = {k: v.clone() for k, v in m.state_dict().items() if "fddt" not in k and k != "proj_out.weight"}
    os.makedirs(tmp_path / "w")
    save_file(sd, str(tmp_path / "w" / "model.safetensors"))
    plain = {k: v for k, v in m.config.to_dict().items() if "fddt" not in k}
    json.dump(plain, open(tmp_path / "w" / "config.json", "w"))
    m2 = pkg.DiCoWForConditionalGeneration.from_pretrained(str(tmp_path / "w"), use_fddt=True, use_pre_pos_fddt=True,
                                                          fddt_init="suppressive", non_target_fddt_value=0.5)
    assert m2._load_report["missing"] and all("fddt" in k for k in m2._load_report["missing"]) and not m2._load_report["unexpected"]
    assert torch.equal(m2.model.encoder.layers[0].fc1.weight, m.model.encoder.layers[0].fc1.weight)
    w = m2.model.encoder.initial_fddt.non_target_linear.weight
    assert torch.allclose(w, torch.full_like(w, 0.5))                           # suppressive init with non_target_fddt_value
    m3 = pkg.DiCoWForConditionalGeneration.from_pretrained("openai/whisper-tiny", use_fddt=True)
    assert m3.config.d_model == 384 and m3._load_report["missing"] is None


def test_product_retrieve_segment_matches_reference_golden():
    from tests.test_oracle_vs_golden import _check_retrieve
    from ts_asr_whisper_amd.generation import retrieve_segment
    _check_retrieve(retrieve_segment)


def test_product_fix_timestamps_matches_reference_golden_and_oracle():
    """Integer-tick folding of recording-time segments into 30 s windows: exact against golden F17, and against the oracle's
    Decimal restatement on a few thousand further random recordings (block boundaries, exact 30 s segments, long gaps)."""
    from tests.test_oracle_vs_golden import _f17_cases
    from oracle.longform import fold_segments, folded_to_ids
    from ts_asr_whisper_amd.generation import fix_timestamps_from_segmentation
    recs, wants = [], []
    for c, segs, want, ts0, fill, pad in _f17_cases():
        assert fix_timestamps_from_segmentation([segs], ts0, fill, pad)[0].tolist() == want, c
        recs.append(segs), wants.append(want)
    batch = fix_timestamps_from_segmentation(recs[:9], ts0, fill, pad, prefix_ids=(3, 4), suffix_ids=(5,))     # padding / specials
    for row, want in zip(batch.tolist(), wants[:9]):
        assert row[:len(want) + 3] == [3, 4] + want + [5] and all(x == pad for x in row[len(want) + 3:])
    rng = np.random.default_rng(170)
    for _ in range(3000):
        t, segs = int(rng.integers(0, 3000)) * int(rng.random() < 0.6), []
        for _ in range(int(rng.integers(1, 10))):
            if rng.random() < 0.3:
                t += int(rng.integers(0, 5000))
            if rng.random() < 0.2:
                t = max(-(-t // 1500) * 1500 - int(rng.integers(0, 3)), 0)
            r = rng.random()
            d = 1500 if r < 0.25 else (-(-(t + 1) // 1500) * 1500 - t if r < 0.4 else int(rng.integers(1, 1600)))
            odd = 0.01 if rng.random() < 0.1 else 0.0
            segs.append(dict(start=round(t * 0.02 + odd, 2), end=round((t + d) * 0.02 + odd, 2),
                             tokens=[1003] + [int(x) for x in rng.integers(10, 900, 2)] + [1040]))
            t += d
        want = folded_to_ids(fold_segments(segs, 1000, 7), 1000)
        assert fix_timestamps_from_segmentation([segs], 1000, 7, 0)[0].tolist() == want, segs
    assert fix_timestamps_from_segmentation([[]], 1000, 7, 0).shape == (1, 0)


def test_product_temperature_fallback_matches_transformers_golden():
    """generation.decode_with_fallback / token_compression_ratio / sequence_avg_logprob against golden F18: transformers' own
    generate_with_fallback (what reference generation.py:567-611 delegates to) driven with scripted decoder outputs."""
    from tests.test_oracle_vs_golden import _check_fallback
    from ts_asr_whisper_amd.generation import decode_with_fallback, token_compression_ratio, sequence_avg_logprob
    _check_fallback(decode_with_fallback, token_compression_ratio, sequence_avg_logprob)


def test_fallback_skip_flag_indexing_default_is_transformers_quirk_and_skip_by_row_fixes_it():
    """Three windows: window 0 fails the log-probability test once and is fine at the next temperature, window 1 decodes
    fine, window 2 fails it and turns out to be silence when decoded again.  In the second round the sub-batch is [0, 2]:
    transformers (hence the reference, generation.py:567-611) writes window 2's should_skip at position 1 of `should_skip`
    -- window 1's slot -- and golden F18 pins that; skip_by_row=True keeps the flag with window 2."""
    import torch
    from ts_asr_whisper_amd.generation import decode_with_fallback
    V, eos, pad = 16, 15, 14
    def scores_for(tokens, good):
        sc = torch.full((len(tokens), V), -8.0)
        for i, t in enumerate(tokens):
            sc[i, t] = 8.0 if good else -7.9
        return sc
    good = {(0, 0): False, (1, 0): True, (2, 0): False, (0, 1): True, (2, 1): False}
    def decode(rows, temp):
        k = 0 if temp == 0.0 else 1
        toks = [[3 + r, 5, 7, eos] for r in rows]
        return toks, [scores_for(t, good[(r, k)]) for r, t in zip(rows, toks)], [0.99 if (r == 2 and k == 1) else 0.1 for r in rows]
    kw = dict(compression_ratio_threshold=None, logprob_threshold=-1.0, no_speech_threshold=0.6)
    final, skip, used = decode_with_fallback(decode, 3, (0.0, 0.2), V, pad, eos, **kw)
    assert used == [1, 0, 1] and skip == [False, True, False]            # the quirk: flag of window 2 sits in window 1's slot
    final2, skip2, used2 = decode_with_fallback(decode, 3, (0.0, 0.2), V, pad, eos, skip_by_row=True, **kw)
    assert used2 == used and final2 == final and skip2 == [False, False, True]


def test_graft_entry_exposes_build_and_smoke():
    import __graft_entry__ as g
    assert callable(g.build) and callable(g.smoke)


def test_no_environment_knobs_on_the_product_dispatch_path():
    """Tuning knobs read with getenv() exist only inside `#ifdef DICOW_ABLATIONS` regions of the kernels' host code (diagnostic
    builds of tools/build_*variants.sh); the shipped library's dispatch depends on its arguments alone.  The experiment routes of
    csrc/experiments/ are under the same rule."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "ts-asr-whisper_amd", "csrc")
    paths = [p for d in (csrc, os.path.join(csrc, "experiments")) for ext in ("*.hip", "*.inc") for p in glob.glob(os.path.join(d, ext))]
    assert any(os.sep + "experiments" + os.sep in p for p in paths)
    for path in sorted(paths):
        depth_abl, stack = 0, []
        for n, line in enumerate(open(path), 1):
            t = line.strip()
            if re.match(r"#\s*if", t):
                stack.append("DICOW_ABLATIONS" in t and not t.startswith("#ifndef"))
            elif re.match(r"#\s*else", t) and stack:
                stack[-1] = False
            elif re.match(r"#\s*endif", t) and stack:
                stack.pop()
            if "getenv(" in t and not t.startswith("//"):
                assert any(stack), f"{os.path.basename(path)}:{n}: getenv outside DICOW_ABLATIONS: {t}"


def test_logmel_folded_tables_equal_the_plain_dft():
    """features._tables: rows 400.. of the DFT tables (the product folded about sample 200 that dicow_logmel reads, ABI 5) give the same
    spectrum as the plain rows 0..399 -- x[n] + x[400 - n] against the cos rows, x[n] - x[400 - n] against the sin rows -- on random
    frames, in float64 (the table algebra, independent of the kernel)."""
    import numpy as np
    import torch
    from ts_asr_whisper_amd import features as F
    tw_c, tw_s, fb, rng = (t.numpy().astype(np.float64) for t in F._tables(80, torch.device("cpu")))
    assert tw_c.shape == (F.N_FFT + F.FOLD_ROWS, F.TABLE_LD) and tw_s.shape == tw_c.shape
    x = np.random.default_rng(0).standard_normal((7, F.N_FFT + 1))          # sample 400 belongs to the next hop: meets zero rows
    n = np.arange(F.FOLD_ROWS)
    xs, xd = x[:, n] + x[:, F.N_FFT - n], x[:, n] - x[:, F.N_FFT - n]
    re_f, im_f = xs @ tw_c[F.N_FFT:], xd @ tw_s[F.N_FFT:]
    re_p, im_p = x[:, :F.N_FFT] @ tw_c[:F.N_FFT], x[:, :F.N_FFT] @ tw_s[:F.N_FFT]
    scale = np.abs(re_p).max()
    assert np.abs(re_f - re_p).max() < 2e-6 * scale and np.abs(im_f - im_p).max() < 2e-6 * scale
    assert not tw_c[F.N_FFT + 201:].any() and not tw_s[F.N_FFT + 200:].any() and not tw_c[:, 201:].any()
    # ... and the plain rows are the windowed DFT itself
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(F.N_FFT) / F.N_FFT)
    ref = np.fft.rfft(x[:, :F.N_FFT] * w, axis=1)
    assert np.abs(re_p[:, :201] - ref.real).max() < 2e-6 * scale and np.abs(im_p[:, :201] - ref.imag).max() < 2e-6 * scale


# ------------------------------------------------------------------------------------------------ layout-edge helpers (tests/util.py)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guarded_checker_flags_every_kind_of_stray_write(dtype):
    """tests/util.guarded on the CPU: the logical view has the asked stride and starts as NaN in its own dtype; a write inside it
    passes; a write one row past the end, in the ld gap or in the leading guard is reported with its (row, col)."""
    from tests.util import guarded
    rows, cols, ld = 5, 12, 16
    new = lambda **kw: guarded((rows, cols), ld, dtype, "cpu", **kw)
    g = new()
    assert g.view.shape == (rows, cols) and g.view.stride() == (ld, 1) and g.view.data_ptr() % 16 == 0
    assert bool(g.view.isnan().all()) and g.untouched_inside() == rows * cols
    assert (g.buf.numel() - g.lead) // ld >= rows + 256
    g.view.copy_(torch.arange(rows * cols).view(rows, cols))                  # a clean write: every logical element, nothing else
    g.check()
    assert g.first_violation() is None and g.untouched_inside() == 0
    g = new(); g.buf[g.lead + rows * ld + 3] = 1.0                            # one row past the end
    assert g.first_violation() == (rows, 3)
    with pytest.raises(AssertionError, match=r"row 5, col 3"):
        g.check()
    g = new(); g.buf[g.lead + 2 * ld + cols] = 0.0                            # the first element of row 2's gap (a zero is a write too)
    assert g.first_violation() == (2, cols)
    g = new(); g.buf[g.lead - 1] = 1.0                                        # the last element of the leading guard
    assert g.first_violation() == (-1, ld - 1)
    g = new(); g.buf[-1] = 1.0                                                # the very last element of the trailing guard
    assert g.first_violation() == ((g.buf.numel() - g.lead - 1) // ld, ld - 1)
    g = new(); g.buf[g.lead + 2 * ld + cols] = float("nan")                   # another NaN than the sentinel's bits is still a write
    assert g.first_violation() == (2, cols)
    # accumulating outputs: the logical region starts from data, only the outside is sentinel
    init = torch.full((rows, cols), 0.5)
    g = new(init=init)
    assert torch.equal(g.view.float(), init) and g.untouched_inside() == 0
    g.view.add_(1.0)
    g.check()


def test_guarded_strided_view_and_poisoned_inputs():
    """A [B, L, 8] slice of packed [B, Lmax, 24] rows: the other columns, the rows L..Lmax of every batch and the tail are guard;
    tests/util.poisoned keeps the logical values and fills all of that with the chosen poison."""
    from tests.util import guarded, poisoned, POISON_BIG, SENTINEL16
    B, Lr, Lmax, ld = 2, 3, 5, 24
    g = guarded((B, Lr, 8), ld, torch.float32, "cpu", strides=(Lmax * ld, ld, 1), offset=8, span_rows=B * Lmax)
    g.view.zero_()
    g.check()
    g.buf[g.lead + Lr * ld + 8] = 0.0                                         # batch 0, row L (past its end), inside the column slice
    assert g.first_violation() == (Lr, 8)
    g = guarded((B, Lr, 8), ld, torch.float32, "cpu", strides=(Lmax * ld, ld, 1), offset=8, span_rows=B * Lmax)
    g.buf[g.lead + Lmax * ld + 7] = 0.0                                       # batch 1, row 0, the column left of the slice
    assert g.first_violation() == (Lmax, 7)
    t = torch.arange(B * Lr * 8, dtype=torch.float32).view(B, Lr, 8)
    for kind in ("nan", "big", "zero"):
        v = poisoned(t, ld, "cpu", strides=(Lmax * ld, ld, 1), offset=8, span_rows=B * Lmax, kind=kind)
        assert torch.equal(v, t) and v.stride() == (Lmax * ld, ld, 1)
        whole = v.as_strided((B * Lmax + 512, ld), (ld, 1), v.storage_offset() - 8)
        out = torch.ones(B * Lmax + 512, ld, dtype=torch.bool)
        for b in range(B):
            out[b * Lmax:b * Lmax + Lr, 8:16] = False
        rest = whole[out]
        if kind == "nan":
            assert bool((rest.view(torch.int16) == SENTINEL16).all())
        elif kind == "big":
            assert bool((rest.abs() == POISON_BIG).all())
        else:
            assert bool((rest == 0).all())
    row = torch.arange(ld, dtype=torch.float32) + 100
    v = poisoned(t, ld, "cpu", strides=(Lmax * ld, ld, 1), offset=8, span_rows=B * Lmax, poison_row=row)
    whole = v.as_strided((B * Lmax + 512, ld), (ld, 1), v.storage_offset() - 8)
    assert torch.equal(v, t) and torch.equal(whole[Lr], row) and torch.equal(whole[-1], row) and torch.equal(whole[0, :8], row[:8])

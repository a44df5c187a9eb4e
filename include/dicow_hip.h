/*
 * libdicow_hip.so -- C ABI of the MI355X-native (gfx950 / CDNA4) DiCoW / SE-DiCoW training-step hot path.
 *
 * The reference (BUTSpeechFIT/TS-ASR-Whisper) has NO native/FFI layer: its seam is the Python module surface
 * (SURVEY.md section 8b).  This header is therefore build-defined; every entry point cites the reference
 * arithmetic (file:line under /root/reference, or HF: = transformers' modeling_whisper.py that the reference
 * subclasses) that it replaces.  The Python host side (the .py files under ts-asr-whisper_amd/) binds these with ctypes and
 * keeps the reference's module names, constructor/forward signatures and state-dict keys.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (PyTorch's caching
 *     allocator in practice).  The library never allocates, frees or retains device memory.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it; entry points are re-entrant and
 *     may be called from any host thread (autograd runs backward on its own thread).
 *   - return 0 on success, negative DICOW_ERR_* otherwise; dicow_last_error() gives a thread-local message.
 *   - bf16 tensors are passed as void* (raw 16-bit storage), row-major, rows 16-byte aligned.
 *   - "rows" = B*T flattened (batch-major); the fp32 residual stream is [rows, D].
 *   - STNO masks are fp32 [B,4,T] with channel order 0=silence 1=target 2=non-target 3=overlap
 *     (src/data/local_datasets.py:184-194); `stno_bstride` is the element stride between batch rows so that
 *     interleaved SE-DiCoW batches (encoder.py:152-154, 210-213) need no copy.
 */
#ifndef DICOW_HIP_H
#define DICOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DICOW_OK 0
#define DICOW_ERR_INVALID (-1)  /* bad argument / unsupported shape */
#define DICOW_ERR_LAUNCH (-2)   /* HIP launch failure */

#define DICOW_ABI_VERSION 7

int dicow_abi_version(void);
/* Number of CUs the persistent NT GEMM may occupy (0 = all, the default).  Its workgroups own a whole CU each for the
 * length of the launch; when a communication kernel (RCCL: one workgroup per channel) runs beside the step, leave it
 * that many CUs -- otherwise the GEMM workgroups that find their CU taken start only when another one has finished its
 * whole tile list.  Returns the previous value. */
int dicow_set_gemm_cus(int n);
/* Names (as a profiler prints them) and launch counts of the GEMM kernel instantiations this process has dispatched,
 * "name\tcount\n" per line; returns the number of bytes written (call with buf = NULL to size it).  Measurement support:
 * bench.py quotes a committed rocprofv3 counter summary only for kernels that occur in this list. */
int dicow_gemm_dispatch_log(char* buf, int cap);
const char* dicow_last_error(void);

/* ------------------------------------------------------------------------------------------------ casts
 * AMP weight preparation (configs/base.yaml:49 `bf16: true`): fp32 master -> bf16 compute copies.      */
int dicow_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* [R,C] fp32 -> bf16 [R,C] (dst, row stride ld; may be NULL) and bf16 [C,R] (dst_t, row stride ld_t; may be NULL):
 * the transposed copy is the dgrad operand of every Linear; the strides let q/k/v land in one fused [3D,D] / [D,3D]. */
int dicow_cast_transpose_f32_to_bf16(const float* src, void* dst, int64_t ld, void* dst_t, int64_t ld_t, int R, int C,
                                     void* stream);
/* The same for up to 8 matrices in ONE launch (AMP's re-cast of a layer's weights after every optimizer step). */
#define DICOW_CAST_GROUP_MAX 8
typedef struct { const float* src; void* dst; void* dst_t; int R, C; int64_t ld, ld_t; } dicow_cast_problem;
int dicow_cast_transpose_group(const dicow_cast_problem* p, int n, void* stream);
/* Conv1d weight [O,C,3] fp32 -> bf16 [O,Kpad] (dst) and its transpose [Kpad,O] (dst_t; either may be NULL),
 * k = tap*C + c (tap-major), zero padded to Kpad >= 3C: the GEMM view of conv1/conv2 (encoder.py:167-168). */
int dicow_conv_weight_pack(const float* w, void* dst, void* dst_t, int O, int C, int Kpad, void* stream);
/* inverse mapping for the weight gradient: [O,Kpad] fp32 (tap-major) accumulated into [O,C,3] fp32 */
int dicow_conv_weight_unpack_grad(const float* g_packed, float* g_w, int O, int C, int Kpad, void* stream);
/* input_features [B,M,Tin] fp32 -> time-major bf16 [B, Tin+2, M], rows 0 and Tin+1 zero (conv padding=1). */
int dicow_mel_to_timemajor(const float* mel, void* dst, int B, int M, int Tin, void* stream);
/* column sums of a bf16 [rows, N] matrix accumulated (+=) into fp32 out[N] (bias gradients).  Two-stage (partials in
 * the caller's workspace, then a reduce pass): fp32 L2 atomics are ~20x slower than that on gfx950. */
int64_t dicow_colsum_ws_bytes(int rows, int N);
int dicow_colsum_bf16(const void* x, int64_t ld, float* out, int rows, int N, void* ws, int64_t ws_bytes, void* stream);
/* out[t,:] += sum_b g[b,t,:]   (gradient of encoder.embed_positions, encoder.py:177-179) */
int dicow_sum_over_batch(const float* g, float* out, int B, int64_t TD, void* stream);

/* Element-wise glue of the SE-DiCoW speaker-communication block (reference src/models/dicow/layers.py:145-193) on the interleaved
 * row layout [Bp][2][T][D] (slot 0 = mixture, slot 1 = enrollment; encoder.py:152-154):
 *   split      hf fp32 -> q_in / kv_in bf16 [Bp*T, D] and the right half of cat bf16 [Bp*T, ldcat] (= q_in, layers.py:161)
 *   merge_fwd  out = hf; out[mixture] += tanh(gate[0]) * upd                                            (layers.py:186-191)
 *   gate_bwd   d_upd = bf16(g[mixture] * tanh(gate));  d_gate[0] += (1 - tanh^2) * sum(g[mixture] * upd)  (d_gate may be NULL)
 *   merge_bwd  gin = g; gin[mixture] += d_qin + d_cat[:, D:2D]; gin[enrollment] += d_kvin */
int dicow_scb_split(const float* hf, void* q_in, void* kv_in, void* cat, int64_t ldcat, int Bp, int T, int D, void* stream);
int dicow_scb_merge_fwd(const float* hf, const void* upd, const float* gate, float* out, int Bp, int T, int D, void* stream);
int64_t dicow_scb_gate_bwd_ws_bytes(void);
int dicow_scb_gate_bwd(const float* g, const void* upd, const float* gate, void* d_upd, float* d_gate, int Bp, int T, int D,
                       void* ws, int64_t ws_bytes, void* stream);
int dicow_scb_merge_bwd(const float* g, const float* d_qin, const void* d_cat, int64_t ldcat, const float* d_kvin, float* gin,
                        int Bp, int T, int D, void* stream);

/* ------------------------------------------------------------------------------------------------ FDDT + LayerNorm
 * Fused row kernel.  Replaces FDDT.forward (src/models/dicow/FDDT.py:41-63) with CustomDiagonalLinear
 * (layers.py:73-77), the optional position-embedding add (encoder.py:177-179) and the LayerNorm that follows
 * in WhisperEncoderLayer (HF:modeling_whisper.py:392,402).
 *   mode 0: no FDDT (plain LayerNorm / copy)
 *   mode 1: diagonal FDDT  h' = ((wS*h+bS)*mS + (wT*h+bT)*mT) + (wN*h+bN)*mN + (wO*h+bO)*mO   -- evaluated in
 *           exactly this order with separate fp32 mul/add (no FMA contraction) => bit-exact vs the fp32 reference;
 *           a NULL w[c] means the class is disabled (identity branch, FDDT.py:55-62)
 *   mode 2: bias-only FDDT h' = h + mS*bS + mT*bT + mN*bN + mO*bO (FDDT.py:43-51), NULL b[c] = disabled
 * Class order in w[]/b[] is S,T,N,O (the stno channel order).                                             */
typedef struct {
    const void* h_in;        /* [rows,D] fp32, or bf16 when in_bf16 != 0 */
    int in_bf16;
    int mode;
    const float* stno;       /* [B,4,T] fp32 (mode != 0) */
    int64_t stno_bstride;    /* elements between consecutive batch entries (4*T when dense) */
    const float* w[4];
    const float* b[4];
    const float* pos;        /* [T,D] fp32 added after the FDDT, or NULL */
    float* h_out;            /* [rows,D] fp32 post-FDDT(+pos) residual stream, or NULL */
    const float* ln_w;       /* LayerNorm affine; NULL => no LayerNorm (h_out only) */
    const float* ln_b;
    void* y_bf16;            /* [rows,D] bf16 LayerNorm output, or NULL */
    float* y_f32;            /* [rows,D] fp32 LayerNorm output, or NULL */
    float* mean;             /* [rows] saved statistics (may be NULL) */
    float* rstd;
    int rows, T, D;
    float eps;
} dicow_fddt_ln_fwd_args;
int dicow_fddt_ln_fwd(const dicow_fddt_ln_fwd_args* a, void* stream);
/* Which kernel body dicow_fddt_ln_fwd runs these arguments on -- "staged", "init_wave", "ln_wave", "generic_ln", "generic_diag",
   "generic" or "generic_1024" -- or NULL where it would reject them (dicow_last_error says why).  Host arithmetic only: launches nothing. */
const char* dicow_fddt_ln_fwd_route(const dicow_fddt_ln_fwd_args* a);

/* Backward of the same fused row op (+ residual-gradient add):
 *   g   = g_res + LayerNormBackward(d_y; x, mean, rstd, ln_w)          (x = FDDT(h_in)+pos, recomputed)
 *   g0  = FDDTBackward(g)  (diag: g * sum_c m_c w_c ; bias-only / mode 0: g)
 * and the column reductions  dln_w += sum_r d_y*xhat, dln_b += sum_r d_y,
 *   dw[c] += sum_r m_c*h_in*g, db[c] += sum_r m_c*g, colsum_out += sum_r g0  (bias grad of the producing Linear).
 * All parameter-gradient outputs are fp32 and ACCUMULATED (+=, NULL = not needed) by a deterministic two-stage
 * reduction through the caller's workspace (no atomics).                                                */
typedef struct {
    const void* h_in; int in_bf16; int mode;
    const float* stno; int64_t stno_bstride;
    const float* w[4]; const float* b[4];
    const float* pos;
    const float* ln_w;       /* NULL => no LayerNorm in this op (g = g_res) */
    const float* mean; const float* rstd;
    const void* d_y;         /* [rows,D] bf16 grad wrt LayerNorm output (or fp32 when dy_f32 != 0) */
    int dy_f32;
    const float* g_res;      /* [rows,D] fp32 residual-path gradient, or NULL */
    float* g_out;            /* [rows,D] fp32 g0, or NULL */
    void* g_out_bf16;        /* [rows,D] bf16 copy of g0 (dgrad/wgrad GEMM operand), or NULL */
    float* dln_w; float* dln_b;
    float* dw[4]; float* db[4];
    float* colsum_out;
    float* dpos_rows;        /* unused, reserved */
    int rows, T, D;
    void* ws; int64_t ws_bytes;   /* workspace for the per-workgroup partial column sums (dicow_fddt_ln_bwd_ws_bytes) */
} dicow_fddt_ln_bwd_args;
int64_t dicow_fddt_ln_bwd_ws_bytes(int rows, int D);
int dicow_fddt_ln_bwd(const dicow_fddt_ln_bwd_args* a, void* stream);
/* ... dicow_fddt_ln_bwd: "ln_wave", "staged_bf16", "staged_f32", "ln_only", "generic" or "generic_1024"; NULL where the arguments are
   rejected (the workspace size is checked by the launch, not here) */
const char* dicow_fddt_ln_bwd_route(const dicow_fddt_ln_bwd_args* a);

/* Full (D x D) FDDT combine: y4 = h @ [W_S;W_T;W_N;W_O]^T (bf16 [rows,4D], from dicow_gemm_nt with bias) ->
 * h' = sum_c m_c * y4[:, cD:(c+1)D]; disabled classes pass y4 block = h via use_mask.  (FDDT.py:13-16, 53-62) */
int dicow_fddt_full_combine_fwd(const void* y4, const void* h_in, int in_bf16, const float* stno, int64_t stno_bstride,
                                int use_mask, float* h_out, int rows, int T, int D, void* stream);
/* backward: d_y4[:, cD:(c+1)D] = m_c * g (bf16), dh_direct = g * sum_{c disabled} m_c (fp32) */
int dicow_fddt_full_combine_bwd(const float* g, const float* stno, int64_t stno_bstride, int use_mask,
                                void* d_y4, float* dh_direct, int rows, int T, int D, void* stream);

/* ------------------------------------------------------------------------------------------------ GEMM (MFMA bf16)
 * C[M,N] = epilogue( A[M,K] . B[N,K]^T ): every Linear / conv-as-GEMM forward and dgrad on the path
 * (HF:modeling_whisper.py:279-282,309,332-333,354,403-405; encoder.py:167-168; modeling_dicow.py:302).
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16, 128x128x64 LDS tiles.
 * Requirements: K % 64 == 0, lda/ldb % 8 == 0, ldc % 4 == 0, N % 4 == 0; M, N tails handled.          */
#define DICOW_EPI_BIAS      1    /* + bias[n] */
#define DICOW_EPI_GELU      2    /* exact-erf GELU of the bf16-ROUNDED pre-activation (AMP: the Linear output is bf16); the pre-activation is stored to aux (bf16) when aux != NULL */
#define DICOW_EPI_RESIDUAL  4    /* + residual[m,n] (fp32, ld = ldr) */
#define DICOW_EPI_OUT_F32   8    /* C is fp32 (else bf16) */
#define DICOW_EPI_SCALE_N  16    /* columns n < scale_ncols multiplied by scale AFTER bias (q * head_dim^-0.5) */
#define DICOW_EPI_GELU_BWD 32    /* C = acc * gelu'(aux[m,n])  (aux = saved pre-activation, bf16) */
#define DICOW_EPI_ACCUM    64    /* C += result (fp32 C only) */
#define DICOW_EPI_GELU_DAUX 128  /* with GELU: aux receives gelu'(pre-activation) (bf16) instead of the pre-activation,  */
                                 /* so that the backward GEMM needs one multiply (MUL_AUX) and no transcendental    */
#define DICOW_EPI_MUL_AUX  256   /* C = acc * aux[m,n]  (aux = saved gelu' from GELU_DAUX, bf16)                      */
#define DICOW_EPI_COLSUM   512   /* colsum_out[n] += sum_m C[m,n] (bias gradient of the layer that produced the GEMM's */
                                 /* input gradient); needs colsum_ws of dicow_gemm_nt_colsum_ws_bytes(M, N) bytes.     */
                                 /* WHICH C is summed depends on the route: the persistent ring kernel's fused form (flags */
                                 /* == MUL_AUX | COLSUM where dicow_gemm_nt_is_persistent) adds the fp32 results BEFORE    */
                                 /* they are rounded to bf16 for the store; every other route adds the STORED bf16 values  */
                                 /* (dicow_colsum_bf16 on C).  The two differ by the store rounding of each element.       */
#define DICOW_EPI_FDDT    1024   /* with BIAS | RESIDUAL | OUT_F32: C = FDDT_next(bf16(acc + bias) + residual); persistent kernel only  */
typedef struct {
    const void* A; const void* B; void* C;
    const float* bias; const float* residual; void* aux;
    int M, N, K;
    int64_t lda, ldb, ldc, ldr, ldaux;
    int batch; int64_t strideA, strideB, strideC, strideAux;   /* grid.z batches (conv stem: per-utterance strided views) */
    int flags; float scale; int scale_ncols;
    float* colsum_out; void* colsum_ws; int64_t colsum_ws_bytes;   /* DICOW_EPI_COLSUM only (else NULL / 0) */
    /* DICOW_EPI_FDDT only (ABI 3): the diagonal FDDT of the NEXT encoder layer applied to the fp32 result row by row
       (reference FDDT.py:41-63 in its evaluation order, bit-identical to dicow_fddt_ln_fwd's h_out):
       fddt_w[c] / fddt_b[c] = the [N] fp32 weight / bias vectors of class c (S, T, N, O), fddt_rowmask = [>= M rounded up to the
       tile height + 64 rows][4] fp32, row m = the four STNO class masks of output row m */
    const float* fddt_w[4]; const float* fddt_b[4]; const float* fddt_rowmask;
    /* EXPERIMENTAL (see the end of this header; zero in the stable ABI): DICOW_EPI_LNSTAT / LNFOLD only: lnstat = [M][DICOW_LN_SLOTS][2] fp32 row partials (LNSTAT writes its 4 * N / 320 slots,
       LNFOLD sums the first ln_nslots in slot order); ln_c = [N] fp32 column sums of the folded weight; ln_inv_dim = 1 / (normalised
       width), ln_eps = LayerNorm epsilon */
    float* lnstat; const float* ln_c; float ln_inv_dim; float ln_eps; int ln_nslots;
} dicow_gemm_args;
/* 1 when dicow_gemm_nt will run this problem on the persistent ring kernel with a compile-time epilogue (the only path
   that implements DICOW_EPI_FDDT), else 0 */
int dicow_gemm_nt_is_persistent(const dicow_gemm_args* a);
int dicow_gemm_nt(const dicow_gemm_args* a, void* stream);
int64_t dicow_gemm_nt_colsum_ws_bytes(int M, int N);
/* Deep contraction, small output (K >= 8192, fewer 128 x 128 tiles than workgroup slots, no epilogue: the tied LM head's dgrad,
 * modeling_dicow.py:302): when the caller passes this many bytes in colsum_ws / colsum_ws_bytes, the contraction is cut into
 * equal ranges that run as one batched launch and are added up in a fixed order.  0 = the problem is not split. */
int64_t dicow_gemm_nt_splitk_ws_bytes(const dicow_gemm_args* a);

/* C[N1,N2] (+)= sum_m A[m,N1] * B[m,N2]  (fp32 C): every weight gradient dW = dY^T X.  When the output has too few
 * tiles to fill the chip the contraction is split over grid.z; the splits write fp32 partials to the caller's
 * workspace (dicow_gemm_tn_ws_bytes) and a reduce pass adds them into C -- deterministic, no atomics.
 * Requirements: N1 % 8 == 0, N2 % 8 == 0, lda/ldb % 8 == 0.                                              */
typedef struct {
    const void* A; const void* B; float* C;
    int Mk, N1, N2;
    int64_t lda, ldb, ldc;
    int batch; int64_t strideA, strideB;            /* extra contraction batches (conv views) */
    int accumulate;                                 /* 1: C += result, 0: C = result */
    float* C_seg[2];                                /* optional row segments: rows [seg_rows, 2*seg_rows) of the logical C */
    int seg_rows;                                   /* go to C_seg[0], rows [2*seg_rows, ..) to C_seg[1] (q/k/v weight grads
                                                       from ONE GEMM over the fused d_qkv); 0 = single C */
    void* ws; int64_t ws_bytes;                     /* workspace for split partials */
} dicow_gemm_tn_args;
int64_t dicow_gemm_tn_ws_bytes(const dicow_gemm_tn_args* a);
int dicow_gemm_tn(const dicow_gemm_tn_args* a, void* stream);

/* Several weight gradients with the same contraction length as ONE persistent launch (the four dW of an encoder layer:
 * autograd's wgrad of q/k/v, out_proj, fc1, fc2 reached from encoder.py:216-221).  Pooled, the output tiles cover the chip
 * with whole contractions and only the remainder is split; one fix-up launch adds those partials in a fixed order.  Same
 * results as calling dicow_gemm_tn on p[0..n) in turn up to fp32 summation order (deterministic); problems that cannot be
 * pooled (N < 256, batches, different Mk, fewer pooled tiles than CUs) are run one by one.  ws: dicow_gemm_tn_group_ws_bytes.
 * Up to 24 problems: a small model (whisper-base: 48 tiles per layer) pools the weight gradients of ALL its layers. */
#define DICOW_TN_GROUP_MAX 24
typedef struct {
    int n;
    dicow_gemm_tn_args p[DICOW_TN_GROUP_MAX];       /* (their own ws / ws_bytes fields are ignored) */
    void* ws; int64_t ws_bytes;
} dicow_gemm_tn_group_args;
int64_t dicow_gemm_tn_group_ws_bytes(const dicow_gemm_tn_group_args* a);
int dicow_gemm_tn_group(const dicow_gemm_tn_group_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------ attention
 * Flash-style softmax(Q K^T) V with head_dim 64, scaling 1.0 (q is pre-scaled by the projection epilogue,
 * HF:modeling_whisper.py:309,337-351).  Dense (encoder 1500x1500, SE enrollment cross-attention
 * layers.py:152-157), causal (decoder self-attention) and rectangular (decoder cross-attention) shapes.
 * q/k/v/o are bf16 with explicit strides (elements): element (b, t, h, d) at  base + b*bs + t*rs + h*64 + d.
 * Batch strides and the q / o row strides are 64-bit throughout.  K and V tiles are fetched with 32-bit byte offsets from the
 * (batch, head) base, so their row strides obey  (max(Lk, 65) - 1) * rs * 2 + 128 < 2^32;  a call past that limit returns
 * DICOW_ERR_INVALID before any launch (dicow_attn_fwd_route: NULL). */
typedef struct {
    const void* q; const void* k; const void* v; void* o;
    float* lse;                                     /* [B,H,Lq] natural-log-sum-exp, saved for backward */
    int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;
    int B, H, Lq, Lk; int causal;
    int q_log2;                                     /* 1: q carries a factor log2(e) (folded into the projection's q-scale, which the
                                                       caller then sets to head_dim^-0.5 * log2 e): the scores are base-2 exponents.
                                                       Same softmax, same lse (natural log) -- the kernel saves a multiply-add per score */
} dicow_attn_fwd_args;
int dicow_attn_fwd(const dicow_attn_fwd_args* a, void* stream);
/* Which kernel body dicow_attn_fwd would run (host logic, no launch): "occ4_spec" (q_log2: base-2 scores, speculative first pass) or
 * "occ4"; NULL where the call would return DICOW_ERR_INVALID, or for a NULL argument. */
const char* dicow_attn_fwd_route(const dicow_attn_fwd_args* a);

/* The decoder step's attention (ONE query row per decoder row) with the K/V row chosen per query row: softmax(q K^T) V, head_dim 64,
 * scaling 1.0 (q pre-scaled), bf16 in and out, fp32 inside, fixed summation order (two launches give the same bits).  Same
 * arithmetic as dicow_attn_fwd with Lq = 1 (HF:modeling_whisper.py:469-494, the decoder layer's cached self- and cross-attention),
 * but the key/value of position t of row r need not live in row r's own cache:
 *   SHARED mode   (anc == NULL): row r reads slot r / group.  The `group` beams of one window share ONE copy of the cross-attention
 *                 K/V (HF's generate repeats the encoder output num_beams times); it is read from memory once per (slot, head) and
 *                 used for all `group` rows.  n_slots == R / group; group == 1 is the plain decode step.
 *   ANCESTRY mode (anc != NULL): key and value t of row r come from slot anc[r * anc_rs + t]; n_slots == R.  This replaces the cache
 *                 reorder of beam search (the reference's _beam_search, src/models/dicow/generation.py:815-1153, calls
 *                 _temporary_reorder_cache(past_key_values, beam_idx): an index_select copy of every layer's K and V per token):
 *                 the caches stay where they were written and the table records, per row and position, which slot wrote it.
 *                 The kernel CLAMPS every table entry into [0, n_slots) before it forms an address: a wrong table gives wrong
 *                 numbers, never a read outside the n_slots caches.
 * q/o: bf16 [R, H, 64], element (r, h, d) at base + r*rs + h*64 + d.  k/v: bf16, element (slot, t, h, d) at
 * base + slot*bs + t*rs + h*64 + d.  Strides in elements; q/k/v bases 16-byte aligned, q_rs/k_rs/v_rs/k_bs/v_bs multiples of 8.
 * Any Lk >= 1, any H >= 1, group 1..DICOW_ATTN_DECODE_MAX_GROUP.  DICOW_ERR_INVALID (and no launch) for a group outside that range,
 * R % group != 0, Lk < 1, n_slots inconsistent with the mode, anc_rs < Lk or a NULL q/k/v/o. */
#define DICOW_ATTN_DECODE_MAX_GROUP 8
typedef struct {
    const void* q; void* o;
    const void* k; const void* v;
    int64_t q_rs, o_rs, k_bs, k_rs, v_bs, v_rs;
    const int32_t* anc; int64_t anc_rs;             /* NULL: shared mode */
    int R, H, Lk, group, n_slots;
} dicow_attn_decode_args;
int dicow_attn_decode(const dicow_attn_decode_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------ LoRA adapters (decoder)
 * The low-rank side of y = W x + b + s B (A x), s = alpha / r (reference src/models/containers.py:69-78: peft LoRA of rank 16 on
 * the decoder's q/k/v/out projections and fc1/fc2).  Three skinny kernels beside the base GEMMs, bf16 operands, fp32 accumulation
 * on v_mfma_f32_16x16x32_bf16; each reads its large operand once.  Adapters that share an input (or whose outputs are the column
 * segments of one fused matrix) are handled by ONE launch:
 *   DENSE mode: one contraction, all R = nseg * r stacked rows at once.
 *   BLOCK mode (DICOW_LORA_BLOCK): the wide matrix is nseg = R / r column segments of `K` / `N` columns each, segment j works
 *              with rows [j r, (j + 1) r) of the stacked small operand only.
 * r in {8, 16, 32, 64}, R % r == 0, R <= DICOW_LORA_MAX_R.  Leading dimensions in elements.  DICOW_ERR_INVALID (and no launch) for
 * anything else.  Nothing outside [M, columns] of an output is written.
 * Rounding points: t = bf16(x A^T); the low-rank product is rounded to bf16, multiplied by s, rounded to bf16 and added to the
 * base result in fp32; the sum is rounded once to the output type (peft's Linear.forward under bf16 autocast). */
#define DICOW_LORA_MAX_R 192
#define DICOW_LORA_MAX_SEG 24
#define DICOW_LORA_BLOCK   1     /* block mode (else dense) */
#define DICOW_LORA_OUT_F32 2     /* up: P and Y are fp32 (else bf16) */
#define DICOW_LORA_GELU    4     /* up (bf16 Y): Y = gelu(bf16(sum)), aux (may be NULL) <- gelu'(bf16(sum)): DICOW_EPI_GELU | DICOW_EPI_GELU_DAUX */
#define DICOW_LORA_MUL_AUX 8     /* up (bf16 Y, FP32 P != Y): Y = bf16((P + v) * aux[m, n]), aux = the saved gelu': DICOW_EPI_MUL_AUX for a dgrad that has an */
                                 /* adapter's share; P is the base dgrad's fp32 result, so that the product is rounded once, as in the GEMM epilogue      */
/* T[M, R] = X V^T (bf16).  Dense: X [M, K], V [R, K].  Block: X [M, nseg * K], V [R, K]; T[:, j r + p] = X[:, j K + k] V[j r + p, k]
 * (the backward's dt_j = dy_j B_j with V = the stacked B_j^T).  K % 32 == 0; X, V 16-byte aligned, ldx / ldv % 8 == 0; T 8-byte
 * aligned, ldt % 4 == 0. */
typedef struct {
    const void* X; const void* V; void* T;
    int64_t ldx, ldv, ldt;
    int M, K, R, r, flags;
} dicow_lora_down_args;
int dicow_lora_down(const dicow_lora_down_args* a, void* stream);
/* Y = epi(P + bf16(s_j * bf16(T_j U_j))), P the base GEMM's result (same type and shape as Y; P == Y allowed, ldp then == ldy).
 * Dense: T [M, R], U [R, N], Y [M, N], s = seg_scale[0] (dx += dt A_stacked; into the fp32 d_enc for the cross-attention k/v).
 * Block: Y [M, nseg * N], Y[:, j N + n] uses T[:, j r + p] U[j r + p, n] and s_j = seg_scale[j] (the forward's y_j with U = the
 * stacked B_j^T; the q segment carries the attention scale beside alpha / r).  N % 16 == 0 (block: N % 64 == 0); T, U: ldt % 8
 * == 0, T 16-byte aligned; P, Y, aux 16-byte aligned with ldp / ldy / ldaux % 8 == 0. */
typedef struct {
    const void* T; const void* U; const void* P; void* Y; void* aux;
    int64_t ldt, ldu, ldp, ldy, ldaux;
    int M, N, R, r, flags;
    float seg_scale[DICOW_LORA_MAX_SEG];
} dicow_lora_up_args;
int dicow_lora_up(const dicow_lora_up_args* a, void* stream);
/* G_j (+)= scale * T_j^T P_j, fp32, element (p, n) of segment j at G[j] + p * g_rs + n * g_cs (dA [r, K]: g_rs = K, g_cs = 1;
 * dB [N, r]: g_rs = 1, g_cs = r); a NULL G[j] is skipped.  Dense: T [M, R], P [M, N]: G[j] = rows [j r, (j + 1) r) of T^T P.
 * Block: P [M, nseg * N]: G[j] = T[:, j r ..]^T P[:, j N ..].  The contraction over M is cut into row blocks whose partial
 * results go to `ws` (dicow_lora_wgrad_ws_bytes) and are added in a fixed order by a second launch: no atomics, two runs give
 * the same bits.  accumulate == 0 overwrites G (its previous contents are not read).  N % 32 == 0; T, P 2-byte elements with any
 * ld >= the columns used. */
typedef struct {
    const void* T; const void* P; float* G[DICOW_LORA_MAX_SEG];
    int64_t ldt, ldp, g_rs, g_cs;
    int M, N, R, r, flags;
    float scale; int accumulate;
    void* ws; int64_t ws_bytes;
} dicow_lora_wgrad_args;
int64_t dicow_lora_wgrad_ws_bytes(int M, int N, int R, int r, int flags);
int dicow_lora_wgrad(const dicow_lora_wgrad_args* a, void* stream);

typedef struct {
    const void* q; const void* k; const void* v; const void* o; const void* d_o;
    const float* lse; float* delta;                 /* delta: workspace [2,B,H,Lq] fp32 (-rowsum(dO*O), -lse) */
    void* dq; void* dk; void* dv;                   /* bf16, same addressing as q/k/v */
    int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs, do_bs, do_rs;
    int64_t dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs;
    int B, H, Lq, Lk; int causal;
    float dq_scale;                                 /* head_dim^-0.5 folded into dq (gradient of the pre-scale) */
    /* optional fused bias gradients: dq_colsum[h*64+d] += sum_{b,q} dq (as stored), dv_colsum likewise; NULL = off.
       cs_ws: dicow_attn_bwd_colsum_ws_bytes(B, H, Lq, Lk) bytes of scratch (per-wave partial rows, reduced afterwards) */
    float* dq_colsum; float* dv_colsum; void* cs_ws; int64_t cs_ws_bytes;
    int q_log2;                                     /* as in dicow_attn_fwd_args; dq keeps its meaning (gradient of the projection
                                                       output before ANY scaling when dq_scale = head_dim^-0.5), dk = ln 2 dS^T q */
    /* ABI 7: optional workspace of the FUSED backward (one kernel, 5 matrix passes instead of 7: dQ is summed over the key-block
       workgroups of a (batch, head) in a fixed order through the XCD's L2 -- no atomics, bit-reproducible).  NULL = the two-kernel
       form.  dicow_attn_bwd_fused_ws_bytes() bytes, 4096-byte aligned, contents irrelevant on entry; used for dense problems of
       at least 1024 key-block workgroups (the encoder's self-attention), ignored otherwise. */
    void* fused_ws; int64_t fused_ws_bytes;
    int fused_mode;                                 /* 0: the library decides (above); 1: the fused kernel for EVERY dense problem it can
                                                       address (B*H <= 1000), whatever its size -- how the tests reach its edge cases */
} dicow_attn_bwd_args;
/* Strides: batch strides and the o / dq / dk / dv row strides are 64-bit throughout.  The K, V, Q and dO tiles are fetched with 32-bit
 * byte offsets from the (batch, head) base:  (max(L, 65) - 1) * rs * 2 + 128 < 2^32  for k_rs, v_rs (L = Lk) and q_rs, do_rs (L = Lq);
 * a call past that limit returns DICOW_ERR_INVALID before any launch (dicow_attn_bwd_route: NULL). */
int dicow_attn_bwd(const dicow_attn_bwd_args* a, void* stream);
int64_t dicow_attn_bwd_colsum_ws_bytes(int B, int H, int Lq, int Lk);
int64_t dicow_attn_bwd_fused_ws_bytes(int B, int H, int Lq, int Lk);
/* Which form dicow_attn_bwd would run (host logic, no launch): "fused" or "dq_dkv" (the two-kernel form); NULL where the call would
 * return DICOW_ERR_INVALID, or for a NULL argument. */
const char* dicow_attn_bwd_route(const dicow_attn_bwd_args* a);
/* The shape half of the fused rule -- everything except "fused_ws was passed and is large enough": 1 where a workspace of
 * dicow_attn_bwd_fused_ws_bytes() would make the call run fused (callers allocate it only then), else 0. */
int dicow_attn_bwd_fused_eligible(int B, int H, int Lq, int Lk, int causal, int fused_mode);
/* error bits the last fused launch left in its workspace (synchronise the stream first): 0 = fine, 1 = a hand-off wait timed
   out, 2 = a (batch, head) was spread over several XCDs; -1 = the copy failed.  dq is not to be trusted when non-zero. */
int dicow_attn_bwd_fused_status(const void* fused_ws);


/* ------------------------------------------------------------------------------------------------ loss
 * Fused log-softmax + cross-entropy on the LM-head logits (bf16 [rows, ld], V valid columns).
 * Hard-label fallback (src/models/dicow/modeling_dicow.py:310-323): CE(ignore_index=-100) for `labels` and
 * `upp_labels`, per-token min; caller divides loss_sum by rows (mean over ALL positions).
 * Soft-label loss (modeling_dicow.py:95-144, soft != 0): rows whose label is a timestamp token use the Gaussian-
 * smoothed target ts_w[ts_index[label], :] scattered at ts_ids (:35-93); both losses masked by labels != -100;
 * caller divides loss_sum by max(count, 1).
 * Backward: d_logits = grad_scale[0] * (softmax - target of the argmin branch) in bf16 (grad_scale on device so
 * that no host sync is needed for the 1/count normalisation).                                                  */
typedef struct {
    const void* logits; int64_t ld; int rows; int V;
    const int64_t* labels; const int64_t* upp_labels;   /* [rows]; upp_labels may be NULL */
    int soft;
    const int32_t* ts_index;                            /* [V] timestamp row of a token id, -1 if none (NULL: no smoothing) */
    const int32_t* ts_ids;                              /* [n_ts] sorted timestamp token ids */
    const float* ts_w;                                  /* [n_ts, n_ts] row-normalised Gaussian weights */
    int n_ts;
    float* lse; float* row_loss; int32_t* choice;       /* [rows] outputs of fwd, inputs of bwd */
    float* loss_sum; float* count;                      /* scalars, ACCUMULATED (zero them first) */
    void* d_logits;                                     /* bwd: bf16 [rows, ld] (pad columns written as 0) */
} dicow_ce_args;
int dicow_ce_loss_fwd(const dicow_ce_args* a, void* stream);
int dicow_ce_loss_bwd(const dicow_ce_args* a, const float* grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------ CTC auxiliary loss
 * torch.nn.functional.ctc_loss as called at src/models/dicow/encoder.py:108-135 on the encoder logits
 * (modeling_dicow.py:242-246, 326-336): bf16 logits [B, Tn, ld] with C = vocab+1 valid classes, blank = C-1,
 * labels [B, Lc] int64 with the valid targets as a prefix (-100 padded), zero_infinity, reduction "mean":
 * loss_sum accumulates sum_b nll_b / max(len_b, 1) (caller divides by B).  alpha/beta: workspace [B, Tn, 2*Lc+1] each.
 * Backward: d_logits = grad_scale[0] / (B * max(len_b,1)) * (softmax - label posterior), bf16, pad columns zero.   */
typedef struct {
    const void* logits; int64_t ld; int B, Tn, C;
    const int64_t* labels; int Lc; int blank;
    float* lse;                  /* [B*Tn] */
    float* alpha; float* beta;   /* [B, Tn, Smax] fp32 log-domain */
    int Smax;                    /* 2*Lc + 1 (<= 1024) */
    float* nll; float* tlen;     /* [B] */
    float* loss_sum;             /* scalar, ACCUMULATED */
    void* d_logits;              /* bwd */
} dicow_ctc_args;
int64_t dicow_ctc_ws_bytes(int B, int Tn, int Lc);
int dicow_ctc_loss_fwd(const dicow_ctc_args* a, void* stream);
int dicow_ctc_loss_bwd(const dicow_ctc_args* a, const float* grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------ decoder embedding
 * h[b,l,:] = embed_tokens[ids[b,l]] + embed_positions[l]   (HF:modeling_whisper.py:737,754-762), fp32.     */
int dicow_embed_fwd(const int64_t* ids, const float* tok, const float* pos, float* out, int B, int Lq, int D, void* stream);
/* d_tok[id] += sum of the rows g[b,l] with ids[b,l] == id, added up in row order; d_pos[l] += sum_b g[b,l] in batch order: no atomics,
 * two runs give the same bits.  Either output may be NULL (frozen). */
int dicow_embed_bwd(const int64_t* ids, const float* g, float* d_tok, float* d_pos, int B, int Lq, int D, void* stream);

/* ------------------------------------------------------------------------------------------------ conv-stem backward helpers
 * out = g * gelu'(pre)   (bf16, elementwise): gradient through the GELU after conv2 (encoder.py:168).     */
int dicow_gelu_bwd_bf16(const void* g, const void* pre, void* out, int64_t n, void* stream);
/* col2im of the conv2 (k=3,s=2,p=1) input gradient + GELU' of conv1 (encoder.py:167):
 *   dA2 bf16 [B, T2, 3*C] (tap-major im2col gradient)  ->  d_pre1 bf16 [B, 2*T2, C] = gelu'(pre1) * scatter-add
 * pre1 == NULL: plain col2im (the activation-free CTC subsample convs, encoder.py:26-41). */
int dicow_conv2_col2im_gelu_bwd(const void* dA2, const void* pre1, void* d_pre1, int B, int T2, int C, void* stream);

/* ------------------------------------------------------------------------------------------------ log-mel front end
 * Whisper features on the GPU (reference call site src/data/local_datasets.py:208-214 -> HF feature_extraction_whisper.py
 * :135-165): wave fp32 [B, n_samples] (padded to a multiple of 30 s) -> out fp32 [B, M, n_samples/160].
 * tw_cos/tw_sin: [604, 224] hann-window-folded DFT tables (201 bins, rows zero-padded to 224 = 7 blocks of 32; the DFT runs as an
 * exact-fp32 matrix product on v_mfma_f32_32x32x2_f32).  Rows 0..399: T[n][k] = w[n] cos(2 pi k n / 400) resp. -w[n] sin(..)
 * (what a direct DFT reads).  Rows 400..603 (ABI 5): the SAME product folded about sample 200 -- the kernel pairs row 400 + n with
 * x[n] + x[400 - n] (cos) resp. x[n] - x[400 - n] (sin), n = 0..203: rows 400 + n = T[n] for n < 200, row 600 = T[200] / 2 in the cos
 * table (x[200] meets itself) and zero in the sin table, rows 601..603 zero.  fb: [201, M] slaney mel filterbank, mel_range: [M][2]
 * int32, the first and one-past-the-last bin where column m of fb is non-zero (host-built once, ts-asr-whisper_amd/features.py). */
int64_t dicow_logmel_ws_bytes(int B, int n_samples);
int dicow_logmel(const float* wave, int B, int n_samples, const float* tw_cos, const float* tw_sin, const float* fb,
                 const int* mel_range, int M, float* out, void* ws, int64_t ws_bytes, void* stream);

/* Background-noise mixing on the waveform, ahead of dicow_logmel (ABI 7, additive): RandomBackgroundNoise.__call__ of the reference
 * (src/data/augmentations.py:395-429, the recipe's musan_augment_prob, gated per sample at src/data/local_datasets.py:205-206).  The draws
 * (which rows, which clip, offset, SNR) are made on the host in the reference's order (ts-asr-whisper_amd/wave_augment.py) and arrive as a plan:
 *   plan_i int32 [n_plan][4] = (row, clip, offset, len), plan_snr fp32 [n_plan] = float(10 ** (snr_db / 10)); rows distinct, len >= 1.
 *   bank fp32: the peak-normalised mono clips back to back; clip k is bank[clip_start[k] .. clip_start[k] + clip_len[k]) (int64 / int32 tables).
 * For every entry, with a = wave + row * ld_wave, o = out + row * ld_out, all arithmetic fp32:
 *     n[i]  = bank[clip_start[clip] + offset + i] while offset + i < clip_len[clip], else 0                          i < len
 *     scale = ||a[0:len)|| / (plan_snr * ||n||)     (the product first, as the reference); scale = 0 when ||n|| == 0, where the reference
 *                                                   divides by zero and returns NaN: a silent crop gives a / 2
 *     o[i]  = fma(scale, n[i], a[i]) * 0.5f                                                                          i < len
 * Nothing else is written: rows that are not in the plan and samples at or behind len are the caller's (copy them first when out != wave).
 * wave and out: 16-byte aligned, ld_wave and ld_out multiples of 4; out == wave (in place, ld_out == ld_wave) is legal, any other overlap
 * of the two is not (unchecked: the rows are device data).  The crop may start at any element of the bank; nothing outside the clip is read.
 * The two sums of squares are accumulated in fp64 per range of a row -- DICOW_NOISE_MIX_CHUNK samples up to 64 chunks, a larger multiple of
 * it for longer rows, from the row's own len only -- stored in fixed workspace slots and added in ascending order by a fixed tree: no
 * atomics, no host read, two launches, capturable into a graph, and a row's result depends on that row's inputs alone (bit-identical
 * alone or beside other rows, and from run to run).  ws: dicow_noise_mix_ws_bytes(n_plan, longest len) bytes, 8-byte aligned, any contents;
 * one call in flight per workspace.  n_plan == 0 launches nothing; n_plan <= 65535. */
#define DICOW_NOISE_MIX_CHUNK 8192
int64_t dicow_noise_mix_ws_bytes(int n_plan, int max_len);
int dicow_noise_mix(const float* wave, int64_t ld_wave, float* out, int64_t ld_out, const float* bank, const int64_t* clip_start,
                    const int* clip_len, const int* plan_i, const float* plan_snr, int n_plan, void* ws, int64_t ws_bytes, void* stream);

/* HOST TABLES.  The table-driven entry points below -- the diarization front end, dicow_resample, dicow_edit_distance,
 * dicow_edit_alignment, dicow_orc_distance, dicow_diar_score, dicow_ngram_repeats, dicow_ctc_forced_align -- take their tables (what a
 * comment calls a HOST pointer) from host memory, and one rule holds for all of them:
 *   - a table is checked in full before anything is launched; a refusal returns -1 with dicow_last_error() set and has launched nothing;
 *   - what the kernels read of it (the table itself, or descriptors built from it) is copied into the head of the caller's workspace on
 *     the stream, ahead of the launches;
 *   - the caller keeps the tables valid and unchanged until the call returns.  The library ASSUMES that a copy from pageable host memory
 *     has read its source by then: an assumption about the HIP runtime that has not been measured here.  A caller who passes pinned
 *     memory keeps it until the stream has passed the copy;
 *   - under stream capture the library keeps a copy of its own of every table for the life of the process, and the graph's copy nodes
 *     read that: a replay never reads caller memory or the image of a later call.  This is what "capturable" means below. */

/* Diarization front end (ABI 7, additive): a diarization -- (speaker, start, end) segments -- to the STNO masks and the self-enrollment
 * windows of SE-DiCoW, without a per-sample mask anywhere (reference src/data/local_datasets.py: get_stno_mask :162-182,
 * _create_stno_masks :184-194, sample_enrollment_window / downsample_mean / select_random_internal_enrollment :216-292).
 * The diarization arrives as a table the host builds in one sweep over the interval endpoints (ts-asr-whisper_amd/diar_front_end.py):
 *   bounds int64 [E + 1], strictly increasing, 0 <= bounds[0], bounds[E] <= n_samples;
 *   active uint64 [E]: bit s set when speaker s (0 <= s < S <= 64) is active on the samples [bounds[e], bounds[e + 1]).
 * `bounds`, `active` and `targets` are HOST pointers (HOST TABLES above; all three entry points are capturable); everything else is
 * device memory.
 * Frames are DICOW_DIAR_FRAME samples (one encoder frame), bins DICOW_DIAR_BIN samples (0.1 s = 5 frames), windows DICOW_DIAR_WINDOW bins
 * (30 s); T_total = ceil(n_samples / 480000) * 1500.  All three: integer arithmetic or correctly rounded fp32 in a fixed order, one writer
 * per output element, no atomics, nothing allocated, bit-identical from run to run and whatever else is asked for in the same call.
 *
 * dicow_diar_frame_counts: for s < S and t < T_total, cnt[s * T_total + t] = samples of frame t on which s is active and excl[...] =
 *   samples on which s is the only active speaker (frames behind the audio count 0).  One thread per (s, t): a binary search in bounds,
 *   then a walk over the table entries that cut the frame.  E == 0 is legal (bounds holds one element).  ws: dicow_diar_table_ws_bytes(E).
 * dicow_stno_from_counts: for target k (targets[k] = a speaker index, or -1 for the reference's unknown speaker, whose activity row is zero)
 *   and frame t, with m_s = __fdiv_rn((float)cnt[s][t], 320.0f) and every product / difference rounded on its own (no contraction):
 *     sil = prod_s (1 - m_s), s ascending;  else = the same product without the target;  tgt = m_t * else;
 *     non = (1 - m_t) * (1 - else);  ovl = m_t - tgt          out[(k * 4 + c) * ld_out + t], c = 0..3 = S, T, N, O;  ld_out >= T_total
 *   -- the bits numpy gives the reference.  Nothing outside [0, T_total) of a row is written.  ws: dicow_diar_targets_ws_bytes(n_targets).
 * dicow_enrollment_windows: per target k (a speaker index; -1 has no enrollment and is refused), with nb = n_samples / 1600 full bins and
 *   bin b = the sum of excl over the frames 5 b .. 5 b + 4:   w[i] = sum of the bins i .. i + 299, i < nw = nb - 299;  start[k] = the FIRST i
 *   with maximal w, count[k] = that w, fallback[k] = 0.  When the maximum is 0 (the target is never alone) the same from cnt, fallback[k] = 1.
 *   nb < 300 (under 30 s): nw = 1, w[0] = the sum of all bins.  weights (may be NULL): w[0 .. nw) of the pass that was taken, int32, row k at
 *   weights + k * ld_w, ld_w >= nw.  One workgroup per target: chunked int64 prefix scan with carry into the workspace, window differences,
 *   first-maximum reduction.  ws: dicow_enrollment_windows_ws_bytes(n_samples, n_targets). */
#define DICOW_DIAR_FRAME 320
#define DICOW_DIAR_BIN 1600
#define DICOW_DIAR_WINDOW 300
#define DICOW_DIAR_MAX_SPEAKERS 64
int64_t dicow_diar_table_ws_bytes(int E);
int64_t dicow_diar_targets_ws_bytes(int n_targets);
int64_t dicow_enrollment_windows_ws_bytes(int64_t n_samples, int n_targets);
int dicow_diar_frame_counts(const int64_t* bounds, const uint64_t* active, int E, int S, int64_t n_samples, int32_t* cnt, int32_t* excl,
                            void* ws, int64_t ws_bytes, void* stream);
int dicow_stno_from_counts(const int32_t* cnt, int S, int64_t n_samples, const int* targets, int n_targets, float* out, int64_t ld_out,
                           void* ws, int64_t ws_bytes, void* stream);
int dicow_enrollment_windows(const int32_t* cnt, const int32_t* excl, int S, int64_t n_samples, const int* targets, int n_targets,
                             int32_t* start, int32_t* count, int32_t* fallback, int32_t* weights, int64_t ld_w, void* ws, int64_t ws_bytes,
                             void* stream);

/* External enrollment mixtures (ABI 7, additive): the audio of the reference's generate_enrollment_mixture (src/data/local_datasets.py:
 * 355-436) -- a few utterances of an enrollment bank, shifted and summed into one 30 s input per row -- written where dicow_logmel reads
 * it.  The draws are made on the host in the reference's order (ts-asr-whisper_amd/enrollment_mix.py) and arrive as a plan of tracks:
 *   plan int32 [n_tracks][4] = (row, clip, off, len): samples [0, len) of clip `clip` land on samples [off, off + len) of row `row`;
 *   rows non-decreasing (the tracks of a row are consecutive, and their order is the order of the sum), at most
 *   DICOW_ENR_MIX_MAX_TRACKS tracks per row; a row may have none.
 *   bank fp32: the clips back to back, clip k at bank[clip_start[k] .. clip_start[k] + clip_len[k]); clips may start at any element.
 * For every row r < B and sample t < n, with x_k = bank[clip_start[clip_k] + t - off_k] over the row's tracks k, in plan order, that
 * cover t:      out[r * ld_out + t] = ((x_0 + x_1) + x_2) + ...   one __fadd_rn per further track; the bits of x_0 when one track covers t;
 *                                     exactly 0 when none does (so the call also pads the row to n samples).
 * Every sample of every row is written by exactly one thread, whatever was there before: no atomics, no workspace, no host read, nothing
 * allocated, one launch, capturable into a graph, and the result does not depend on the launch geometry (bit-identical from run to run,
 * and for a row alone or beside other rows).  16-byte loads are used only where all four samples of a vector lie inside a track, single
 * loads at its edges: nothing outside a clip is read, nothing outside [0, n) of a row is written.
 * out: 16-byte aligned, ld_out a multiple of 4 and >= n.  The plan is passed twice: plan_host (and clip_len_host, the n_clips clip
 * lengths) are HOST arrays that are checked before anything is launched -- row in [0, B), rows non-decreasing, clip in [0, n_clips),
 * off >= 0, 1 <= len <= clip_len, off + len <= n, the track cap; a failure returns -1 with dicow_last_error() set -- and plan_dev is the
 * same table in device memory, which is what the kernel reads (a captured graph replays on whatever plan_dev then holds: the caller
 * answers for a table it writes there later).  B <= 65535; n_tracks == 0 writes zeros. */
#define DICOW_ENR_MIX_MAX_TRACKS 8
int dicow_enrollment_mix(float* out, int64_t ld_out, int B, int n, const float* bank, const int64_t* clip_start, const int32_t* plan_dev,
                         const int32_t* plan_host, int n_tracks, const int32_t* clip_len_host, int n_clips, void* stream);

/* Any-rate audio intake (ABI 7, additive): interleaved int16 or mono fp32 samples at any rational rate -> mono fp32 at the model's rate,
 * in the reference's order (src/data/augmentations.py:401-407): the mean over the channels, then torchaudio.functional.resample with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).  With g = gcd(orig, new), o = orig / g, n = new / g and the bank
 * h[p][k], p < n, k < 2 width + o, of that function (built on the host in fp64 and rounded once, ts-asr-whisper_amd/wave_intake.py), only
 * one contiguous run of taps per phase is non-zero in fp32.  The bank arrives compact: first[p] = the first tap of phase p's run (HOST
 * int32 [n]) and taps_t[s * n + p] = h[p][first[p] + s] for s < S, S = the longest run, zero behind a shorter one (device fp32, tap-major).
 * One call resamples n_segs segments that share (o, n).  segs is a HOST int64 [n_segs][3] table of (in_start, in_len, out_start), in
 * frames of `in` and samples of `out`.  For every segment, with x[q] = the mono value of frame in_start + q for 0 <= q < in_len, else 0:
 *     out[out_start + j n + p] = fma(t[S-1], x[..], ... fma(t[1], x[j o + first[p] + 1 - width], fma(t[0], x[j o + first[p] - width], 0)))
 *   for j n + p < ceil(n in_len / o), t[s] = taps_t[s * n + p]: one fmaf per tap, s ascending.  o = n = 1, width 0, one tap of 1.0 is the
 *   identity (conversion and mixdown only).  in_int16 = 0: `in` is fp32 mono (C = 1, channel -1 or 0).  in_int16 = 1: `in` is int16,
 *   C <= DICOW_RESAMPLE_MAX_CHANNELS channels interleaved; channel = c takes sample / 32768 of channel c, channel = -1 the mean:
 *   sample / 32768 per channel, the channel sum (both exact), one correctly rounded division by C -- the bits of torch.mean(pcm / 32768, 0).
 * Nothing outside a segment is read (in_frames, out_samples: the sizes of the two buffers), nothing outside its ceil(n in_len / o)
 * output samples is written, and every output sample has one writer and one order of summation: its bits do not depend on
 * frames_per_tile, the grid, or the other segments of the call.  No atomics; one launch behind one copy, capturable (HOST TABLES above).
 * Checked on the host before anything is launched (-1, dicow_last_error()): 1 <= o, n <= DICOW_RESAMPLE_MAX_RATIO; 1 <= S <= 2 width + o;
 * first[p] in [0, 2 width + o); every segment inside the stated buffer sizes, lengths >= 0; the output ranges pairwise disjoint; the
 * pointers aligned (in, out: their element size; taps_t: 16 bytes; ws: 8 bytes); and the LDS budget: a workgroup keeps the input span of
 * frames_per_tile whole output frames -- (frames_per_tile - 1) o + (max first - min first) + S samples, plus 12 of padding -- and, when
 * 4 S n <= DICOW_RESAMPLE_LDS_BYTES / 2, the bank (it is read from memory otherwise) in DICOW_RESAMPLE_LDS_BYTES of LDS.  frames_per_tile = 0 lets
 * the library choose (about 4096 output samples per tile, or what fits); a ratio whose single frame does not fit is refused, and so is a
 * frames_per_tile that does not.  in and out must not overlap (unchecked: device memory).  ws: dicow_resample_ws_bytes(n_segs, n) bytes;
 * the table and first[] go there.  n_segs == 0, or segments that are all empty, launch nothing. */
#define DICOW_RESAMPLE_LDS_BYTES 49152
#define DICOW_RESAMPLE_MAX_RATIO 1048576
#define DICOW_RESAMPLE_MAX_CHANNELS 512
int64_t dicow_resample_ws_bytes(int n_segs, int n);
int dicow_resample(const void* in, int in_int16, int C, int channel, int64_t in_frames, float* out, int64_t out_samples, const float* taps_t,
                   const int32_t* first, int o, int n, int width, int S, const int64_t* segs, int n_segs, int frames_per_tile, void* ws,
                   int64_t ws_bytes, void* stream);

/* Scoring what was decoded (ABI 7, additive): a batch of Levenshtein tables over int32 symbol ids -- words or characters mapped to dense ids
 * on the host (ts-asr-whisper_amd/scoring.py) -- for WER / CER (one pair per utterance; the reference: jiwer, src/utils/evaluation.py:32-79)
 * and cpWER / tcpWER (one pair per (reference speaker, hypothesis speaker); meeteval, src/utils/wer.py:30-38, 89-97).
 * ref_ids [n_ref], hyp_ids [n_hyp]: flat device buffers.  ref_iv / hyp_iv: device int32 [n_ref][2] / [n_hyp][2] of (begin, end) in integer
 * ticks, row q belonging to id q; both NULL = unconstrained, one NULL is refused.  pairs: a HOST int64 [n_pairs][4] table of (ref_start,
 * ref_len, hyp_start, hyp_len); pairs may share or overlap spans.  out: device int32 [n_pairs][2] = (errors, hits):
 *   unit costs; cell (i, j) may take the diagonal step -- a hit if ref[i] == hyp[j], a substitution otherwise -- only without intervals or
 *   when rb < he && hb < re (touching intervals do not overlap); otherwise only insertion and deletion are open.  Among the alignments with
 *   the fewest errors E the one with the most hits H is taken, the lexicographic minimum of the additive key (E, -H).  The other counts
 *   follow: I = E - N_ref + H, D = E + H - N_hyp, S = N_ref + N_hyp - 2 H - E.  A length of 0 gives (the other length, 0).
 * One workgroup per pair; lane t keeps a strip of DICOW_EDIT_K columns in registers and rows run as a skewed pipeline, the strip's right
 * edge handed to lane t + 1 through LDS; a panel is lanes * DICOW_EDIT_K columns, and a longer sequence goes panel by panel with the
 * panel's last column, one key per row, in the pair's slice of ws.  The key is symmetric in the two sequences, so either may lie along
 * the lanes.  lanes: 0 = the library's choice for the call (DICOW_EDIT_LANES if the shorter side of some pair exceeds DICOW_EDIT_LANES_NARROW *
 * DICOW_EDIT_K symbols, DICOW_EDIT_LANES_NARROW otherwise), or one of the two; along: 0 = per pair whichever makes fewer steps, 1 = ref
 * along the lanes, 2 = hyp.  Exact integer arithmetic: the result depends on neither, nor on the other pairs of the call.  The key is
 * packed E * 2^15 - H in int32 when ref_len + hyp_len <= 65535 - DICOW_EDIT_LANES * DICOW_EDIT_K for every pair, E * 2^32 - H in int64 otherwise.
 * Checked on the host before anything is launched (-1, dicow_last_error()): lengths in [0, DICOW_EDIT_MAX_LEN], spans inside n_ref / n_hyp,
 * intervals for both sides or neither, lanes / along, pointers and their alignment, ws_bytes.  ws: dicow_edit_distance_ws_bytes(pairs,
 * n_pairs) bytes, 8-byte aligned: the table and the boundary columns; -1 for a table the call would refuse for its lengths.  One launch
 * behind one copy, no atomics, capturable (HOST TABLES above).  n_pairs == 0 launches nothing. */
#define DICOW_EDIT_MAX_LEN 65535
#define DICOW_EDIT_K 8
#define DICOW_EDIT_LANES 512
#define DICOW_EDIT_LANES_NARROW 64
int64_t dicow_edit_distance_ws_bytes(const int64_t* pairs, int n_pairs);
int dicow_edit_distance(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv, const int32_t* hyp_iv,
                        const int64_t* pairs, int n_pairs, int32_t* out, int lanes, int along, void* ws, int64_t ws_bytes, void* stream);

/* Word-level alignments (ABI 7, additive): the edit path behind the counts of dicow_edit_distance -- what jiwer's process_words(...)
 * .alignments and meeteval's tcp alignment view (the reference's calc_wer(save_visualizations=True), src/utils/wer.py:18-27, 154-155) show.
 * ref_ids / hyp_ids / ref_iv / hyp_iv / pairs / lanes / along / stream: exactly as for dicow_edit_distance.  Outputs, all device buffers:
 *   out    int32 [n_pairs][2] = (errors, hits), the values dicow_edit_distance gives;
 *   ops    uint8, one byte per step of the path: 0 hit, 1 substitution, 2 deletion (a reference word without partner), 3 insertion (a
 *          hypothesis word without partner).  Pair p owns the slot of ref_len_p + hyp_len_p bytes that starts at the sum of the earlier
 *          pairs' slot sizes; its path stands in forward order (first word first) at the END of the slot;
 *   spans  int64 [n_pairs][2] = (first, length): the index in ops of the pair's first op, and the number of ops.
 *   Nothing in ops outside [first, first + length) is written.
 * The path is defined on ref and hyp and does not depend on lanes, along or the other pairs: with D[i][j] the key of dicow_edit_distance for
 * the first i reference and j hypothesis words, from (N_ref, N_hyp) each cell takes the first of these that attains D[i][j]: the diagonal
 * step (only where rb < he && hb < re, or without intervals; a hit if the ids are equal, -1, otherwise a substitution, + 2^15 or 2^32), a
 * deletion from D[i-1][j], an insertion from D[i][j-1].  On row or column 0 one step is open; a length of 0 gives all insertions or all
 * deletions, (0, 0) gives length 0.
 * Launches: the kernel of dicow_edit_distance compiled with recording -- 2 bits per cell, one 16-bit word per lane per row of its strip,
 * stored skewed as the lanes produce them, [panel][step][lane], so a step's store is one coalesced row -- and a walk, one wave per pair,
 * that stages blocks of 128 steps x 64 strips of records in LDS, lets one lane follow the path inside the block and flushes the ops in
 * coalesced chunks.  No atomics, no waiting between workgroups, one writer per byte, capturable like dicow_edit_distance (one copy, two
 * launches).  ws: dicow_edit_alignment_ws_bytes(pairs, n_pairs, lanes, along) bytes, 8-byte aligned, at most DICOW_ALIGN_MAX_WS_BYTES: the
 * two tables (DICOW_ALIGN_TABLE_BYTES a pair), the boundary columns of dicow_edit_distance, and per pair with both lengths > 0, with m the
 * length along the lanes, n the other, P = lanes * DICOW_EDIT_K, q = ceil(m / P) and w = ceil((m - (q - 1) P) / DICOW_EDIT_K), the records:
 * 2 * ((q - 1) (n + lanes - 1) lanes + (n + w - 1) w) bytes rounded up to 8.
 * Checked on the host before anything is launched (-1, dicow_last_error()): everything dicow_edit_distance checks; the workspace limit;
 * out / ops / spans non-null, spans 8-byte aligned; ws_bytes.  dicow_edit_alignment_ws_bytes returns -1 for a table, lanes or along the
 * call would refuse.  n_pairs == 0 launches nothing. */
#define DICOW_ALIGN_MAX_WS_BYTES 1073741824LL
#define DICOW_ALIGN_TABLE_BYTES 56
int64_t dicow_edit_alignment_ws_bytes(const int64_t* pairs, int n_pairs, int lanes, int along);
int dicow_edit_alignment(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv, const int32_t* hyp_iv,
                         const int64_t* pairs, int n_pairs, int32_t* out, uint8_t* ops, int64_t* spans, int lanes, int along, void* ws,
                         int64_t ws_bytes, void* stream);

/* Scoring sessions whose speaker labels are not trusted (ABI 7, additive): optimal-reference-combination WER and its time-constrained form
 * (ORC-WER / tcORC-WER; meeteval's orcwer / tcorcwer, which the reference calls per group of a session, src/utils/wer.py:41-106) for a batch
 * of independent problems -- one problem is one group of one session.  ref_ids / hyp_ids / ref_iv / hyp_iv: as for dicow_edit_distance.
 * problems: a HOST int64 [n_problems][4] table of (utt_first, n_utts, stream_first, n_streams), rows of the two HOST int64 tables utts
 * [..][2] = (ref_start, ref_len), one reference utterance per row in the order they are spoken, and streams [..][2] = (hyp_start, hyp_len),
 * one hypothesis stream per row.  out: device int32 [n_problems][2] = (errors, hits).  assignment: NULL, or device int32 with one entry per
 * utterance row, the stream (0 .. n_streams - 1 within its problem) the utterance was given to.
 *   L[j_0, .., j_{H-1}], 0 <= j_h <= hyp_len_h, holds the key of dicow_edit_distance, errors * 2^15 - hits; at first L = (sum of j_h) * 2^15.
 *   One utterance of m words: for every stream h, every line of L along axis h (the other indices fixed) takes m Levenshtein row updates
 *   against stream h, new[0] = old[0] + 2^15, new[j] = min(old[j] + 2^15, new[j-1] + 2^15, old[j-1] + (-1 if the words are equal else 2^15)),
 *   the diagonal term open only without intervals or when rb < he && hb < re; the table after the utterance is the elementwise minimum of
 *   the H results.  An utterance of 0 words changes nothing.  The answer is L[hyp_len_0, .., hyp_len_{H-1}]: the minimum over all H^U ways
 *   to give utterances to streams of the summed keys of dicow_edit_distance(the stream's utterances concatenated, the stream).
 *   assignment: one that attains this minimum; among equal keys the stream with the smallest index, then the path that entered the
 *   stream's line earliest; an utterance of 0 words gets stream 0.  It depends on nothing but the problem.  With an assignment two
 *   problems may not share utterance rows.  No stream: (all reference words, 0), assignment -1.  No utterance: (all hypothesis words, 0).
 * The streams of a problem lie along the axes in ascending length, so the contiguous axis is the shortest stream.  Launches: one fill, per
 * utterance step one lane-per-line pass over every axis of every problem that has such an utterance (a column of DICOW_ORC_K + 1 keys in
 * registers per chunk of DICOW_ORC_K words: one read and one write per cell per chunk) and one elementwise fold, then one that reads the
 * corners and chases the assignment back; no atomics, no waiting between workgroups, capturable like dicow_edit_distance.
 * ws: dicow_orc_distance_ws_bytes(...) bytes, 8-byte aligned, at most DICOW_ORC_MAX_WS_BYTES.  With S = the product of (hyp_len_h + 1),
 * H = n_streams, U = n_utts and r8 = rounding up to 8:  n_problems * DICOW_ORC_DESC_BYTES + (all n_utts) * DICOW_ORC_UTT_BYTES, and for
 * every problem with H > 0 and U > 0:  r8(4 S) + r8(4 H S)  without assignment,  r8(4 S) + 8 H S + r8(4 S U)  with it.
 * Checked on the host before anything is launched (-1, dicow_last_error() names the limit): n_streams <= DICOW_ORC_MAX_STREAMS; reference +
 * hypothesis words of a problem <= DICOW_ORC_MAX_WORDS (the int32 key, DICOW_ORC_K rows of padding included); S <= DICOW_ORC_MAX_STATES;
 * the workspace <= DICOW_ORC_MAX_WS_BYTES (a call refused for its assignment's records may still run without); spans inside n_ref /
 * n_hyp; intervals for both sides or neither; pointers and their alignment; ws_bytes.  dicow_orc_distance_ws_bytes returns -1 for tables
 * the call would refuse for their sizes.  n_problems == 0 launches nothing. */
#define DICOW_ORC_MAX_STREAMS 8
#define DICOW_ORC_K 8
#define DICOW_ORC_MAX_WORDS 65527
#define DICOW_ORC_MAX_STATES 4194304
#define DICOW_ORC_MAX_WS_BYTES 1073741824LL
#define DICOW_ORC_DESC_BYTES 288
#define DICOW_ORC_UTT_BYTES 16
int64_t dicow_orc_distance_ws_bytes(const int64_t* problems, int n_problems, const int64_t* utts, const int64_t* streams, int want_assignment);
int dicow_orc_distance(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv, const int32_t* hyp_iv,
                       const int64_t* problems, int n_problems, const int64_t* utts, const int64_t* streams, int32_t* out, int32_t* assignment,
                       void* ws, int64_t ws_bytes, void* stream);

/* Scoring diarizations (ABI 7, additive): everything the diarization error rate, the Jaccard error rate and the optimal speaker mapping
 * are made of, for a batch of independent problems -- one problem is one (reference, hypothesis) pair at one collar -- in exact int64
 * arithmetic on ticks (samples), without a per-sample mask.  A problem has two tables of the diarization front end (bounds int64 [E + 1]
 * strictly increasing, active uint64 [E], bit s = speaker s < S <= 64 talks on [bounds[e], bounds[e + 1]); E == 0 is an empty table whose
 * one bound is not read), a sorted list of disjoint half-open UNSCORED intervals [u0, u1) (they may touch), and a skip_overlap flag.
 * All tables are HOST memory (HOST TABLES above; the three arrays are copied from where they are, without a staging copy on the host),
 * concatenated: bounds int64 [n_bounds], active uint64 [n_active], unscored int64 [n_unscored][2], and
 * problems int64 [n_problems][DICOW_DIAR_SCORE_ROW] =
 *   (ref_bounds_first, ref_active_first, Er, Sr, hyp_bounds_first, hyp_active_first, Eh, Sh, unscored_first, n_unscored, skip_overlap, 0):
 *   the reference's bounds are bounds[ref_bounds_first .. + Er], its bitmasks active[ref_active_first .. + Er - 1], and so on.
 * The elementary regions of a problem are the intervals between neighbours of the merge of its three endpoint lists; on a region the two
 * bitmasks are constant: n_ref and n_hyp are their popcounts.  A region is SCORED when it lies in no unscored interval and, with
 * skip_overlap, n_ref <= 1.  out: device int64 [n_problems][DICOW_DIAR_SCORE_OUT_WORDS], per problem
 *   [0, 4096)     C[i][j] at i * 64 + j: the scored ticks on which reference speaker i and hypothesis speaker j are both active,
 *   [4096, 4160)  R[i], [4160, 4224)  H[j]: the scored ticks of each speaker,
 *   [4224, 4232)  scored (the scored ticks between the first and the last bound of the two tables), total = sum dur * n_ref,
 *                 missed = sum dur * max(0, n_ref - n_hyp), false_alarm = sum dur * max(0, n_hyp - n_ref), matched = sum dur * min(n_ref,
 *                 n_hyp), then three zeros.  Every word is written, those of speakers >= S with 0.
 * Launches: one in which every endpoint finds its rank in the merge by two binary searches in the other lists (ties: reference before
 * hypothesis before unscored, then by index -- a permutation, so one writer per merged word); one in which a workgroup of 256 threads
 * stages (dur, ref bits, hyp bits) of `chunk` consecutive regions in LDS (dur = 0 for a region that is not scored) and walks them, every
 * thread owning 16 fixed cells of C, one wave R and one H, the scalars summed while staging, and writes the chunk's partial sums; one that
 * adds the partials of every problem in ascending chunk order.  No atomics, one writer per word, nothing read back by the host
 * (capturable); integer sums, so the result does not depend on the chunk, the grid or the other problems of the call.
 * chunk: regions per workgroup, 1 .. DICOW_DIAR_SCORE_CHUNK, or 0 for DICOW_DIAR_SCORE_CHUNK.
 * ws: dicow_diar_score_ws_bytes(...) bytes, 8-byte aligned, at most DICOW_DIAR_SCORE_MAX_WS_BYTES.  With M = the endpoints of a problem
 * ((Er + 1 if Er else 0) + (Eh + 1 if Eh else 0) + 2 n_unscored) and n_chunks = ceil(max(M - 1, 0) / chunk):
 *   n_problems * DICOW_DIAR_SCORE_DESC_BYTES + 8 * (n_bounds + n_active + 2 * n_unscored)
 *   + sum over the problems of 8 * M + 8 * n_chunks * (64 * Sr + 136).
 * Checked on the host before anything is launched (-1, dicow_last_error() says what): row ranges inside the arrays; 0 <= S <= 64;
 * E <= DICOW_DIAR_SCORE_MAX_E and n_unscored <= DICOW_DIAR_SCORE_MAX_E per problem; bounds strictly increasing; no speaker bit at or above
 * S; unscored intervals non-empty, sorted and disjoint; every position in [0, DICOW_DIAR_SCORE_MAX_TICK]; the workspace limit; pointers and
 * their alignment; ws_bytes.  dicow_diar_score_ws_bytes makes the same checks of the tables and returns -1 where the call would refuse
 * them.  n_problems == 0 launches nothing. */
#define DICOW_DIAR_SCORE_CHUNK 256
#define DICOW_DIAR_SCORE_ROW 12
#define DICOW_DIAR_SCORE_OUT_WORDS 4232
#define DICOW_DIAR_SCORE_DESC_BYTES 120
#define DICOW_DIAR_SCORE_MAX_E 16777216
#define DICOW_DIAR_SCORE_MAX_TICK 1099511627776LL
#define DICOW_DIAR_SCORE_MAX_WS_BYTES 4294967296LL
int64_t dicow_diar_score_ws_bytes(const int64_t* bounds, int64_t n_bounds, const uint64_t* active, int64_t n_active, const int64_t* unscored,
                                  int64_t n_unscored, const int64_t* problems, int n_problems, int chunk);
int dicow_diar_score(const int64_t* bounds, int64_t n_bounds, const uint64_t* active, int64_t n_active, const int64_t* unscored,
                     int64_t n_unscored, const int64_t* problems, int n_problems, int chunk, int64_t* out, void* ws, int64_t ws_bytes,
                     void* stream);

/* Cutting hallucinated repeats from hypotheses before they are scored (ABI 7, additive): where a decoded segment has to end so that a
 * looping hallucination ("thank you thank you ...", "a b a b ...") is cut at its first repeat -- the reference's
 * truncate_at_repeating_ngram (src/data/postprocess.py:18-74), which process_session (src/utils/evaluation.py:150-176) applies to every
 * segment before calc_wer sees it -- for n independent segments in one call.
 * ids / fold: device int32 [n_words]; table: a HOST int64 [n][2] table of (start, len).  Segment s is the W = len words at [start, start + W):
 *   id[0..W)    the exact ids: equal iff the words are equal strings,
 *   fold[0..W)  the folded ids: equal iff the words' lower-cased forms are equal.
 * Parameters min_n >= 1, max_n, min_words, u = unigram_min_repeat >= 1, r = repeat_threshold >= 0.  THE DEFINITION:
 *   run(i)   = the length of the maximal run fold[i] == fold[i + 1] == ... that starts at i;
 *   occ_n(i) = the number of j in [0, W - n] with id[j + k] == id[i + k] for all k < n (j == i counts, overlapping occurrences count);
 *   cnt_n(i) = 0 if fold[i .. i + n) are all equal (such an n-gram is never counted), else occ_n(i), for max(2, min_n) <= n <= max_n and
 *              i <= W - n; cnt_n = 0 for every other n.
 *   keep     = W if W < min_words; otherwise the minimum of
 *                W,
 *                i0 + 1 with i0 the smallest i <= W - u that has run(i) >= u        (this term exists only if min_n == 1),
 *                i + n over all (n, i) with cnt_n(i) > r.
 * So the counts are case-sensitive, the degenerate test and the unigram run are not, a count equal to r does not cut, and an n-gram never
 * spans two segments.  The reference's ngram_length influences nothing but the default of max_n.
 *   reason[s] = (n, i, count): what attained keep.  (0, 0, 0) if nothing was cut (keep == W); (1, i0, run(i0)) for the unigram rule, the
 *   full run, not capped; otherwise (n, i, cnt_n(i)).  THE TIE RULE among the candidates that attain the minimum is the project's own (the
 *   reference reports no reason): the unigram rule wins, then the smallest n.
 * Outputs, device buffers, one writer per element, no atomics: keep int32 [n]; reason int32 [n][3], or NULL.
 * Launches: the host cuts every segment that can be cut (W >= min_words, some n in range) into work items of R rows i; a workgroup of R
 * lanes keeps each row's window id[i .. i + max_n) in registers, streams the segment's words through LDS in chunks of C and counts for
 * every n at once the j whose match is at least n words long; it min-reduces one packed key (keep, n, count) per item.  A second launch of
 * one wave per segment folds the items, finds i0 from the run boundaries and writes keep and reason.  plan: 0 = the library's choice for the
 * call, or 1 .. DICOW_NGRAM_PLANS for (R, C) = (64, 256), (64, 1024), (256, 256), (256, 1024) (tests, measurements); a segment's result
 * depends neither on the plan nor on the other segments.  One copy and two launches, no host read: capturable (HOST TABLES above).
 * ws: dicow_ngram_repeats_ws_bytes(table, n, plan) bytes, 16-byte aligned, at most DICOW_NGRAM_MAX_WS_BYTES: DICOW_NGRAM_SEG_BYTES a
 * segment and DICOW_NGRAM_ITEM_BYTES a possible work item (ceil((W - 1) / R) a segment), rounded up to 16, and 8 bytes a possible item.
 * Checked on the host before anything is launched (-1, dicow_last_error() names the limit): W in [0, DICOW_NGRAM_MAX_WORDS]; plan; the
 * workspace limit; the spans inside n_words; min_n >= 1, max_n <= DICOW_NGRAM_MAX_N, u >= 1, r >= 0; pointers and their alignment;
 * ws_bytes.  dicow_ngram_repeats_ws_bytes checks the lengths, the plan and the limit alone.  n == 0 launches nothing. */
#define DICOW_NGRAM_MAX_N 16
#define DICOW_NGRAM_MAX_WORDS 65535
#define DICOW_NGRAM_PLANS 4
#define DICOW_NGRAM_MAX_WS_BYTES 1073741824LL
#define DICOW_NGRAM_SEG_BYTES 24
#define DICOW_NGRAM_ITEM_BYTES 8
int64_t dicow_ngram_repeats_ws_bytes(const int64_t* table, int n, int plan);
int dicow_ngram_repeats(const int32_t* ids, const int32_t* fold, int64_t n_words, const int64_t* table, int n, int min_n, int max_n,
                        int min_words, int unigram_min_repeat, int repeat_threshold, int32_t* keep, int32_t* reason, int plan, void* ws,
                        int64_t ws_bytes, void* stream);

/* Bootstrap and randomisation sums of integer count columns (ABI 7, additive): the one primitive behind a bootstrap confidence interval
 * of an error rate, the paired bootstrap of the difference of two systems and the paired approximate-randomisation test -- sums of the
 * columns of a table of counts over R random multisets of its rows, all replicates in one launch.
 * table: device int64 [n][C], row-major, leading dimension ld >= C in elements: one row per unit (session, utterance), one column per
 * count.  1 <= n <= DICOW_BOOT_MAX_N, 1 <= C <= DICOW_BOOT_MAX_C.  strata: a HOST array of S + 1 = n_strata + 1 ascending offsets with
 * offs[0] = 0 and offs[S] = n, every stratum non-empty (S = 1: no stratification); strata_dev: the same S + 1 int64 offsets in device
 * memory (may be NULL when S == 1 or mode is DICOW_BOOT_SWAP: then nothing reads them).  out: device int64 [R][C], dense.
 * THE DEFINITION.  The random word for replicate r and slot p is
 *   w(r, p, t) = Philox4x32-10(counter = (p >> 2, r & 0xffffffff, r >> 32, t), key = (seed & 0xffffffff, seed >> 32))[p & 3]
 * where r is the absolute replicate number first_replicate + row (64-bit, wrapping) and Philox4x32-10 is the Random123 function with
 * multipliers 0xD2511F53 / 0xCD9E8D57 and key increments 0x9E3779B9 / 0xBB67AE85.
 *   Resample mode (DICOW_BOOT_RESAMPLE, t = 0):  out[row, c] = sum over p in [0, n) of table[lo_s + ((w * n_s) >> 32), c]
 *     where s is the stratum that holds slot p, lo_s is its first unit and n_s is its size: each replicate draws exactly n_s units, with
 *     replacement, from each stratum.  The multiply-high mapping has a bias of at most n_s / 2^32: a unit's probability differs from
 *     1 / n_s by less than 2^-32.
 *   Swap mode (DICOW_BOOT_SWAP, t = 1, C even, h = C / 2):  b = w & 1, and out[row, c] = sum over p of table[p, (c + h*b) mod C].
 *     Columns [0, h) belong to system A and [h, C) to system B; a set bit exchanges the two systems' counts of unit p.  Strata are ignored.
 * Plain int64 adds, no atomics, one writer per output element; one replicate never spans more than one workgroup, so there is no
 * cross-workgroup reduction and no workspace; one launch, no host read: the call can be captured into a graph.  Because the sums are
 * integers and the words depend only on (seed, r, p, t), the output is identical under every plan, grid and chunking of the R replicates
 * into calls.  PRECONDITION (not checked here; the Python wrapper checks it with one reduction): n * max|table| < 2^62.  Negative entries
 * are allowed.
 * plan: 0 = the library's choice for the call (dicow_bootstrap_plan names it), or 1 .. DICOW_BOOT_PLANS (tests, measurements):
 *   1 DICOW_BOOT_LANE_LDS  a lane owns a whole replicate, the table staged in LDS (256 replicates a workgroup),
 *   2 DICOW_BOOT_WAVE_LDS  a wave owns a replicate: each lane evaluates one Philox block for four consecutive slots a step and keeps C
 *                          sums in registers, a wave reduction at the end; the table staged in LDS (64 replicates a workgroup),
 *   3 DICOW_BOOT_WAVE_L2   the same with the table read through L2 (4 replicates a workgroup).
 * Plans 1 and 2 need n * C * 8 <= DICOW_BOOT_LDS_BYTES and are refused otherwise.
 * Checked on the host before anything is launched (-1, dicow_last_error() names it): n, C, ld, R in [0, DICOW_BOOT_MAX_R], the mode (and
 * C even in swap mode), the plan and whether the table fits it, the strata (first 0, last n, ascending, none empty), pointers and their
 * 8-byte alignment.  R == 0 succeeds and writes nothing. */
#define DICOW_BOOT_MAX_N 16777216
#define DICOW_BOOT_MAX_C 32
#define DICOW_BOOT_MAX_R 2147483647LL
#define DICOW_BOOT_LDS_BYTES 65536
#define DICOW_BOOT_PLANS 3
#define DICOW_BOOT_LANE_LDS 1
#define DICOW_BOOT_WAVE_LDS 2
#define DICOW_BOOT_WAVE_L2 3
#define DICOW_BOOT_RESAMPLE 0
#define DICOW_BOOT_SWAP 1
int dicow_bootstrap_plan(int n, int C);      /* the plan that plan = 0 stands for; -1 for n or C out of range */
int dicow_bootstrap_sums(const int64_t* table, int64_t ld, int n, int C, const int64_t* strata, const int64_t* strata_dev, int n_strata,
                         int64_t R, uint64_t first_replicate, uint64_t seed, int mode, int plan, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------ batch augmentation
 * The collator's training-time augmentations (reference src/data/collators.py:189-214), applied to the batch where it
 * already lives (HBM).  The random decisions are drawn on the host from the torch CPU generator in the reference's
 * own order (ts-asr-whisper_amd/augment.py) and arrive here as small plans, so a seed reproduces the reference.
 *
 * dicow_stno_noise_rescale (collators.py:50-77): for i < n_rows, r = rows[i]:
 *     x = stno[r] + noise[i] * sd;  x -= min(min_c x, 0);  stno[r] = x / sum_c x         (in place; rows distinct)
 *   stno fp32 [B, C=4, T], rows int32 [n_rows], noise fp32 [n_rows, C, T] (N(0,1) draws), sd = sqrt(variance).
 * dicow_stno_segment_augment (collators.py:79-138): for each changed segment s (segments are disjoint):
 *     dominant = argmax_c mean_t stno[b, c, start:end];  target = the pick-th class != dominant
 *     x = keep * stno[b, :, t] + soft * onehot(target);  stno[b, :, t] = x / sum_c x      (in place)
 *   segs int32 [n_seg, 4] = (b, start, end, pick), coef fp32 [n_seg, 2] = (keep = 1 - softness, soft = softness).
 * dicow_specaug_joint (collators.py:209-214; src/data/augmentations.py:85-120 time warp, :23-79 masks, :363-379
 *   masks limited to features [:128]): x = [mel ; stno repeated `sub` times along time]  (M + 4 feature rows, T frames)
 *     time warp: frames [0, center) are resampled to [0, warped) and [center, T) to [warped, T) with torch's bicubic
 *       kernel (align_corners = false, A = -0.75, border clamp per piece);  warped < 0 disables the warp
 *     frequency masks fmask int32 [B, n_fmask, 2] = (pos, len) and time masks tmask int32 [B, n_tmask, 2] zero
 *       x[b, pos:pos+len] on feature rows < n_maskable (= min(128, M + 4) in the reference)
 *     mel_out fp32 [B, M, T] = rows < M;  stno_out fp32 [B, 4, T/sub] = mean over each `sub` frames of rows >= M.
 *   Out of place (mel_out != mel, stno_out != stno). */
int dicow_stno_noise_rescale(float* stno, const int* rows, const float* noise, int n_rows, int C, int T, float sd,
                             void* stream);
int dicow_stno_segment_augment(float* stno, const int* segs, const float* coef, int n_seg, int C, int T, void* stream);
int dicow_specaug_joint(const float* mel, const float* stno, float* mel_out, float* stno_out, int B, int M, int T, int sub,
                        int center, int warped, const int* fmask, int n_fmask, const int* tmask, int n_tmask,
                        int n_maskable, void* stream);

/* ------------------------------------------------------------------------------------------------ CTC prefix scoring
 * Joint CTC / attention decoding (reference src/models/dicow/decoding.py; CTCPrefixScore :8-163 is the hot part: a Python
 * loop over the encoder frames per decoded token).  Log-probabilities are x[b, t, c] = logits[b, t, alias[c]] - lse[b, t]:
 *   dicow_ctc_frame_lse     lse[row] = logsumexp_v logits[row, v < V1]   (the log_softmax of decoding.py:183)
 *   alias int32 [V1] or NULL: column read for label c (the reference copies lower-cased columns over the upper-cased
 *                           ones, decoding.py:181-186)
 *   dicow_ctc_prefix_init   r0 fp32 [B, T, 2] = state of the empty prefix (CTCPrefixScore.initial_state, :36-43)
 *   dicow_ctc_prefix_score  CTCPrefixScore.__call__ (:122-163) for n hypotheses x C candidate labels:
 *       rows int32 [n]         batch row of each hypothesis (the reference's `samples_to_be_decoded` mask, as indices)
 *       cs int32 [n, C]        candidate next labels;  decoded_len int32 [n] labels already in the prefix;
 *       last int32 [n]         last label of the prefix;  r_prev fp32 [n, T, 2] its state (non-blank, blank)
 *       psi fp32 [n, C]        log prefix probability of prefix + candidate (eos: probability of ending, blank: logzero)
 *       r fp32 [n, T, 2, C]    the candidates' states (the caller keeps the chosen one as the next r_prev)
 *   logits fp32 or bf16 (in_bf16) [B, T, ld >= V1], frame-major. */
typedef struct {
    const void* logits; int in_bf16; int64_t ld; const float* lse; const int* alias;
    const int* rows; const int* cs; const int* decoded_len; const int* last; const float* r_prev;
    float* psi; float* r;
    int n, C, T, blank, eos;
} dicow_ctc_prefix_args;
int dicow_ctc_frame_lse(const void* logits, int in_bf16, int64_t rows, int V1, int64_t ld, float* lse, void* stream);
int dicow_ctc_prefix_init(const void* logits, int in_bf16, int64_t ld, const float* lse, int B, int T, int blank_col, float* r0,
                          void* stream);
int dicow_ctc_prefix_score(const dicow_ctc_prefix_args* a, void* stream);

/* Whisper's timestamp rules on next-token scores, in place (reference src/models/dicow/utils.py:5-14 =
 * transformers' WhisperTimeStampLogitsProcessor + eos allowed at the first generated position):
 * scores fp32 [B, ld >= V]; input_ids int64 [B, L] (prompt + generated so far), begin_index = prompt length;
 * timestamp_begin = no_timestamps + 1; max_initial_timestamp_index < 0: no cap; detect_from_logprob: if the total
 * probability of the timestamp labels exceeds every text label's, text labels are removed. */
int dicow_whisper_timestamp_rules(float* scores, int64_t ld, int B, int V, const int64_t* input_ids, int L, int begin_index,
                                  int timestamp_begin, int eos, int no_timestamps, int max_initial_timestamp_index,
                                  int detect_from_logprob, void* stream);

/* Repetition penalty and no-repeat n-grams on next-token scores, in place (ABI 7, additive): transformers'
 * RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor, the two processors HF's generate -- which the
 * reference's delegates to -- builds from generation_config.repetition_penalty / .no_repeat_ngram_size
 * (src/utils/general.py:19-34) and runs in front of Whisper's own.
 * scores fp32 [rows, ld >= V]; row r's history (prompt + tokens generated so far) is the L >= 1 int64 entries at
 * input_ids + r * ids_stride (ids_stride >= L, L <= 8192).
 *   penalty (> 0; 1 = off): every DISTINCT history token v gets s = scores[r, v] <- s < 0 ? s * penalty : s / penalty, once however
 *     often it occurs (-inf stays -inf, -0.0 is divided);
 *   ngram (<= 0 = off): if L + 1 >= ngram, for every j in [0, L - ngram] with ids[j .. j + ngram - 2] equal to the last
 *     ngram - 1 entries of the history, scores[r, ids[j + ngram - 1]] <- -inf (ngram == 1: every history token); a token that is
 *     penalised and banned ends as -inf.
 * An id outside [0, V) takes part in the n-gram comparison by value but never indexes the scores.  Columns >= V and rows >= rows
 * are not touched.  One launch, no workspace, deterministic; with both rules off nothing is launched. */
int dicow_repetition_rules(float* scores, int64_t ld, int rows, int V, const int64_t* input_ids, int64_t ids_stride, int L,
                           float penalty, int ngram, void* stream);

/* Sequence bias and banned phrases on next-token scores, in place (ABI 7, additive): transformers' SequenceBiasLogitsProcessor, and
 * with biases of -inf its NoBadWordsLogitsProcessor -- what HF's generate builds from generation_config.sequence_bias /
 * .bad_words_ids (hotwords; forbidden phrases).
 * scores fp32 [rows, ld >= V]; row r's history is the L >= 1 int64 entries at input_ids + r * ids_stride (ids_stride >= L).
 * table: ONE device int32 array, built once per window by the caller (generation.sequence_bias_table), of
 *     seq_off [n_seq + 1] | grp_off [n_groups + 1] | bias [n_seq] (fp32 bits) | tok [n_tokens]
 *   sequence s is tok[seq_off[s] .. seq_off[s + 1]), 1 .. max_len tokens, every token in [0, V); its bias is finite or -inf (+inf and
 *   NaN are refused by the host wrapper: transformers would turn -inf + inf into NaN); the sequences stand sorted (stably) by their last
 *   token, group g = sequences grp_off[g] .. grp_off[g + 1) = all sequences of one last token, its single-token sequence (at most one)
 *   first, the others in the caller's (dict) order; max_group = the longest group.
 * Definition.  Sequence s of m tokens MATCHES row r if m == 1 (whatever the history: transformers' length-1 bias), or if m <= L and the
 * last m - 1 history entries equal tok[0 .. m - 1) of s, compared by value as int64 (a history id outside [0, V) never matches); a
 * sequence longer than the history is ignored.  For every group, v its last token: b = +0.0f; for each matching sequence in table order
 * b = b + bias_s (one fp32 rounding per add); if at least one matched, scores[r, v] = scores[r, v] + b.  Nothing else is written:
 * columns >= V, rows >= rows and every score whose token heads no matching sequence keep their bits -- so an untouched -0.0 stays -0.0,
 * where transformers' `scores + bias` over the whole row returns +0.0 (the one difference in bits; as numbers the two are equal).
 * One writer per score element, no atomics, no host table, no workspace: a row's result depends on that row's history and the table
 * alone and is bit-identical from run to run and under every plan.  One launch, capturable; with n_seq == 0 nothing is launched (table
 * may be NULL).
 * plan: 0 = the library's choice (WAVE when max_group >= 64, else LANE), DICOW_SEQ_BIAS_LANE = a lane per group,
 * DICOW_SEQ_BIAS_WAVE = a wave per group (matches balloted, added in lane order).
 * Refused before anything is launched (-1, dicow_last_error() names the limit): L > DICOW_SEQ_BIAS_MAX_L, max_len >
 * DICOW_SEQ_BIAS_MAX_LEN, n_seq > DICOW_SEQ_BIAS_MAX_SEQ, an unknown plan, counts that contradict each other.  The table's CONTENT is
 * read on the device only: an entry that breaks the layout (a range outside the table, a token outside [0, V)) matches or writes
 * nothing. */
#define DICOW_SEQ_BIAS_MAX_L 8192
#define DICOW_SEQ_BIAS_MAX_LEN 32
#define DICOW_SEQ_BIAS_MAX_SEQ 65536
#define DICOW_SEQ_BIAS_PLANS 2
#define DICOW_SEQ_BIAS_LANE 1
#define DICOW_SEQ_BIAS_WAVE 2
int dicow_sequence_bias(float* scores, int64_t ld, int rows, int V, const int64_t* input_ids, int64_t ids_stride, int L,
                        const int* table, int n_seq, int n_groups, int n_tokens, int max_len, int max_group, int plan, void* stream);

/* Sampling a step's next tokens (ABI 7, additive): the warpers HF's generate builds for do_sample=True (TemperatureLogitsWarper,
 * TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper, min_tokens_to_keep = 1), the draw, the chosen token's log-probability and the
 * end-of-sequence bookkeeping of a greedy / sampling loop, ONE launch over the processed scores fp32 [rows, ld >= V] (read only).
 * Below x_v = scores[r, v] with NaN read as -inf; temperature, top_p and min_p are the fp32 numbers of the struct; tokens are compared
 * as fp32 numbers (-0.0 == +0.0).
 * Warpers.
 *   temperature   y_v = x_v / temperature, one correctly rounded fp32 division.  temperature <= 0 (the argmax rung): y = x and no warper
 *                 is applied, whatever top_k / top_p / min_p hold.
 *   top_k (<= 0: off)   k = min(top_k, V); v is removed iff y_v < the k-th largest y (ties with the k-th value stay; with fewer than k
 *                 finite scores nothing finite is removed).  Exact: counting only.
 *   top_p (>= 1: off)   over the tokens top_k kept, e_v = exp(y_v - y_max), Z = sum e; v is removed iff
 *                 sum{e_u : y_u <= y_v} <= (1 - top_p) * Z; the maximum is always kept.  A tie class is kept or removed as a whole.  The
 *                 e_v are fp32 (one exp2 of an fp32 product each), summed in fp64 in a fixed order; 1 - top_p is formed in fp64.
 *   min_p (<= 0: off)   v is removed iff exp(y_v - y_max) < min_p over what is left, evaluated in fp64.
 *   -inf scores are removed tokens from the start.  All three rules cut the order of y from below, so the kept set is
 *   {v : y_v >= a threshold}; `warped` (fp32 [rows, ld_w >= V] or NULL) receives y_v for kept tokens and -inf for the others -- the
 *   scores HF returns.  Columns >= V are not touched.
 * The draw.
 *   temperature <= 0: the lowest index of the maximum of x.
 *   otherwise Gumbel-max:  w(v) = Philox4x32-10(counter = (v >> 2, row_id, step, stream), key = (seed lo, seed hi))[v & 3], row_id = the
 *   low 32 bits of row_ids[r] (r itself when row_ids is NULL);  u = ((w >> 8) + 0.5) * 2^-24, strictly inside (0, 1);  the token is the
 *   argmax over kept v of y_v - log(-log(u)), lowest index on ties.  (u is an fp32 number for w >> 8 < 2^23 only; above, -log(u) is
 *   evaluated as -log1p(-(1 - u)), 1 - u = ((2^24 - 1 - (w >> 8)) + 0.5) * 2^-24 being one.  The two logarithms are fp32.)  A row's
 *   token is a function of (its scores, the options, seed, row_id, step, stream) alone: not of the grid, the plan or the other rows.
 * Bookkeeping.
 *   next[r * next_stride] (int64) = the token.  logprob[r] (fp32, or NULL) = x_tok - logsumexp{x_v : v kept}: the token's log-probability
 *   at temperature 1 over the kept set (fp32 exps summed in fp64, one fp32 rounding at the end: within 2^-22 |lp| + 70 * 2^-24 of the
 *   exact value, the budget also behind the top_p band 2e-5 of the tests).
 *   unfinished (uint8 [rows], in/out, or NULL): a row whose flag is 0 writes `pad`, logprob 0, and keeps the flag; a row that draws `eos`
 *   clears its flag.  A row without any score above -inf writes `eos` (and clears its flag), logprob NaN, `warped` all -inf.
 * One workgroup of 1024 lanes per row; lane l owns tokens l, l + 1024, ...; every sum and count is reduced in a fixed order (lane-serial,
 * wave butterfly, 16 waves in order); integers and fp64 masses decide the thresholds by bisection over the order-preserving 32-bit key
 * of y.  No atomics, one writer per element, no workspace, capturable.
 * plan: 0 = the library's choice (REG when V <= DICOW_SAMPLE_REG_MAX_V), DICOW_SAMPLE_REG = the row is read once and held in registers,
 * DICOW_SAMPLE_STREAM = every pass re-reads the row (any V).  Both give identical bits in every output.
 * Refused before anything is launched (-1, dicow_last_error() names the limit): an unknown plan, DICOW_SAMPLE_REG with
 * V > DICOW_SAMPLE_REG_MAX_V, rows < 0, V < 1, ld < V, ld_w < V, next == NULL, a NaN option.  rows == 0 launches nothing. */
#define DICOW_SAMPLE_REG_MAX_V 65536
#define DICOW_SAMPLE_PLANS 2
#define DICOW_SAMPLE_REG 1
#define DICOW_SAMPLE_STREAM 2
typedef struct {
    const float* scores; int64_t ld; int rows; int V;
    float temperature; int top_k; float top_p; float min_p;
    uint64_t seed; uint32_t step; uint32_t stream;
    const int64_t* row_ids; uint8_t* unfinished; int eos; int pad;
    int64_t* next; int64_t next_stride; float* logprob; float* warped; int64_t ld_w; int plan;
} dicow_sample_args;
int dicow_sample_tokens(const dicow_sample_args* a, void* stream);

/* Greedy CTC decoding (ABI 7, additive): ctc_greedy_decode of the reference (src/utils/decoding.py:6-12: torch.argmax, then a Python
 * itertools.groupby over every row of the device tensor), the preprocess_logits_for_metrics of CTC pre-training (src/pretrain_encoder.py:82-86).
 * logits fp32 / bf16 (in_bf16): frame t of batch row b starts at element b * batch_stride + t * ld; unit stride over the V1 <= ld classes.  The
 * base pointer needs the alignment of its element type only.
 * out int64: out[b * out_stride + j], j < n_b, is the frame-wise argmax path of row b with consecutive repeats merged and every id equal
 * to `blank` dropped; out[b * out_stride + j] = pad_id for n_b <= j < Tn (out_stride >= Tn; nothing else is written).
 * The argmax is over columns < V1 only -- columns [V1, ld) are never read -- and on equal maxima the lowest index wins (torch.argmax on the
 * CPU); +-inf follow the same rule, a row of -inf gives 0.  NaN among the V1 columns is outside the contract (the id still lies in [0, V1)).
 * blank and pad_id are arbitrary: an id that never occurs drops nothing, pad_id may be negative.
 * ws: int32 [B * Tn] workspace of the caller (the frame-wise argmax).  B * Tn < 2^31.  Two launches, no host read, no atomics: the result
 * is a function of the inputs alone, and the call can be captured into a graph. */
int dicow_ctc_greedy_decode(const void* logits, int in_bf16, int64_t batch_stride, int64_t ld, int B, int Tn, int V1, int64_t blank,
                            int64_t pad_id, int* ws, int64_t* out, int64_t out_stride, void* stream);

/* CTC forced alignment (ABI 7, additive): the best path through the CTC trellis of a KNOWN target sequence, read back -- what
 * torchaudio.functional.forced_align computes -- for n independent problems in one call (all decoded segments of a session).
 * logits fp32 / bf16 (in_bf16) [B, T, ld >= V1], frame-major with dense frames, read in place; columns [V1, ld) and frames outside a
 * problem's slice are never read.  lse fp32 [B * T] (dicow_ctc_frame_lse) or NULL: the logits are log-probabilities already.  alias int32
 * [V1] or NULL (identity), as for dicow_ctc_prefix_score; an alias outside [0, V1) counts as -inf.
 * table: a HOST int64 [n][5] table of (row, f0, F, target_offset, L); targets: a HOST int32 array of n_targets ids.  Problem i aligns
 * y = targets[target_offset .. + L) against frames [f0, f0 + F) of logits row `row` with x[f][c] = logit[row, f0 + f, alias[c]] -
 * lse[row * T + f0 + f] (one fp32 subtraction).  States s = 0 .. 2 L, even = blank, odd = y[(s - 1) / 2]:
 *   v[0][0] = x[0][blank], v[0][1] = x[0][y[0]], every other v[0][s] = -inf,
 *   v[f][s] = x[f][label(s)] + max over the admissible predecessors of v[f - 1][.]        (plain fp32 addition),
 * the predecessors being s, s - 1, and s - 2 when s is odd and y[(s - 1) / 2] != y[(s - 3) / 2].
 * THE TIE RULE is the project's own (it is not pinned to any other implementation): among equal maxima staying in s beats s - 1 and s - 1
 * beats s - 2; at the last frame state 2 L wins over 2 L - 1 only if strictly greater; L = 0 gives the all-blank path; F = 0 with L = 0
 * the empty path of score 0.  -inf logits are legal.  NaN among the used columns is outside the contract (nothing is read or written out
 * of bounds).  Outputs, all device buffers, one writer per element, no atomics:
 *   path        int32 [n, Fmax]     the label id of every frame (`blank` on blank frames), -1 from F to Fmax;
 *   spans       int32 [n, Lmax, 2]  (first frame, one past the last frame) of every target, relative to f0; -1 behind L;
 *   token_score fp32  [n, Lmax]     the sum of x over the target's own frames, added in ascending frame order; 0 behind L;
 *   score       fp32  [n]           v at the chosen end state;
 *   status      int32 [n]           0 aligned; 1 infeasible: F < L + (number of adjacent equal targets), F = 0 with L > 0, or every end state
 *                                   at -inf.  An infeasible problem has -1 in its whole path and all its spans, 0 token scores, score -inf.
 * A problem's bits do not depend on plan or on the other problems of the call.
 * Launches: a gather of the compact emission matrix E (per problem F rows of W = roundup8(L) + 4 floats: the targets' x, -inf up to a
 * multiple of 8, the blank's x, three zeros), then one wave per problem: the frame recursion with 16 (wide plan) or 2 (narrow plan, L <=
 * 63) states per lane in registers, 2-bit back-pointers stored per frame, and the walk back through blocks of 64 frames of them staged in
 * LDS.  plan: 0 = narrow for every problem with L <= 63, wide otherwise; 1 / 2 force narrow / wide (tests, measurements).  One copy
 * and two launches; no host read: capturable (HOST TABLES above).
 * ws: dicow_ctc_align_ws_bytes(table, n) bytes, 16-byte aligned, at most DICOW_CTC_ALIGN_MAX_WS_BYTES: DICOW_CTC_ALIGN_PROB_BYTES a problem
 * plus 4 bytes a target, rounded up to 16; then per problem 4 F W bytes of E and F * bp_row rounded up to 16 of back-pointers, bp_row =
 * max(4 * ceil((2 L + 1) / 16), roundup4(L + 1) if L <= 63).
 * Checked on the host before anything is launched (-1, dicow_last_error() names the limit): row in [0, B); f0 >= 0 and f0 + F <= T; F in
 * [0, 2^31); L <= DICOW_CTC_ALIGN_MAX_L (2 L + 1 <= 1024 states, the ceiling of dicow_ctc_args.Smax); the targets' range in the array, every
 * id in [0, V1) and not `blank`; Fmax / Lmax not below the table's largest F / L; plan; the workspace limit; pointers and their alignment;
 * ws_bytes.  dicow_ctc_align_ws_bytes checks F, L and the limit alone and returns -1 where the call would refuse them.  n == 0 launches
 * nothing. */
#define DICOW_CTC_ALIGN_MAX_L 511
#define DICOW_CTC_ALIGN_MAX_WS_BYTES 1073741824LL
#define DICOW_CTC_ALIGN_PROB_BYTES 56
int64_t dicow_ctc_align_ws_bytes(const int64_t* table, int n);
int dicow_ctc_forced_align(const void* logits, int in_bf16, int B, int T, int V1, int64_t ld, const float* lse, const int32_t* alias, int blank,
                           const int64_t* table, int n, const int32_t* targets, int64_t n_targets, int32_t* path, int Fmax, int32_t* spans,
                           int Lmax, float* token_score, float* score, int32_t* status, int plan, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ optimizer
 * Fused AdamW + global-norm clipping on flat fp32 regions (src/models/containers.py:100-114 two param groups;
 * HF Trainer max_grad_norm 1.0).  dicow_sumsq_f32 accumulates sum(x^2) into out[0], DETERMINISTICALLY for a given input
 * (fixed summation order: data-parallel replicas must derive the same clip coefficient); one call in flight per device;
 * dicow_adamw_f32 applies
 *   g' = g * min(1, max_norm / (sqrt(gnorm_sq[0]) + 1e-6));  decoupled weight decay; bias-corrected moments.   */
int dicow_sumsq_f32(const float* x, int64_t n, float* out, void* stream);
/* Measurement aid (ABI 7; no reference counterpart): the load an 8-rank RCCL all-reduce of `bytes` at `gbps` GB/s (algorithm bandwidth)
 * puts on THIS GPU while it runs beside the backward pass, reproduced on one GPU -- `workgroups` blocks rewrite the buffer in place
 * with its own values, `passes` times (2 = reduce-scatter + all-gather), pacing themselves so that the call takes bytes / gbps.
 * The data are unchanged.  trainer.GradReducer (DICOW_EMULATE_FABRIC_GBPS) / bench.py --emulate-fabric-gbps. */
int dicow_fabric_emulate(void* buf, int64_t bytes, double gbps, int workgroups, int passes, void* stream);
int dicow_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, const float* gnorm_sq, float max_norm, void* stream);
/* The same update with the step-dependent scalars read from device memory, hyper = {lr, 1 - beta1^t, 1 - beta2^t}: a training
 * step captured in a hipGraph (reference counterpart: HF Trainer.training_step, src/utils/trainers.py:116-139, re-run every
 * step) replays with fixed kernel arguments.  dicow_adamw_hyper keeps the counters on the device (counters[0] = optimizer steps
 * taken, counters[1 + i] = updates received by run i; torch keeps state['step'] per parameter), advances them and writes
 * hyper[3 i ..] for every active run: HF's LambdaLR indexing (the k-th step uses lambda(k - 1)), linear warm-up, cosine decay
 * to max_steps (configs/train/dicow_v3.yaml:66-68) or constant, x `mult` for preheat runs (containers.py:109-111);
 * preheat_only: the other runs are frozen (trainers.py:122-137) and neither counted nor written.  lr / mult / betas are doubles and
 * the schedule and 1 - beta^t are evaluated in double on the device, as torch evaluates them on the host. */
int dicow_adamw_hyper(int* counters, float* hyper, const int* is_pre, int n_runs, int preheat_only, double lr, double mult,
                      int warmup_steps, int max_steps, int cosine, double beta1, double beta2, void* stream);
int dicow_adamw_f32_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, const float* gnorm_sq, float max_norm, void* stream);

/* ------------------------------------------------------------------------------------------------ multi-tensor optimizer (ABI 7, additive)
 * torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ over a LIST of separate fp32 tensors (optim.DiCoWAdamW / optim.clip_grad_norm_;
 * reference src/models/containers.py:100-114 hands a two-group torch AdamW to the HF Trainer).  A call is described by a DEVICE table:
 * dicow_mt_tensor[n_tensors] (four pointers, int64 element count, class index, alignment flags) and dicow_mt_chunk[n_chunks] (one
 * per DICOW_MT_CHUNK elements of each tensor, int64 start, in table order); workgroups stride over the chunks.  The table depends on the
 * pointers only: the host uploads it again only when they change.  Tensors of a sumsq / scale call may leave p, m, v NULL. */
#define DICOW_MT_CHUNK 2048
#define DICOW_MT_MAX_CLASSES 32
#define DICOW_MT_ALIGNED_ALL 1   /* p, g, m, v all 16-byte aligned: float4 path for the adamw update */
#define DICOW_MT_ALIGNED_G   2   /* g 16-byte aligned: float4 path for sumsq / scale */
typedef struct {
    float* p; float* g; float* m; float* v;
    int64_t n;              /* elements */
    int32_t cls;            /* class index (adamw): one class = one (param group, per-parameter step count) */
    int32_t flags;          /* DICOW_MT_ALIGNED_* */
} dicow_mt_tensor;          /* 48 bytes */
typedef struct { int64_t start; int32_t tensor; int32_t len; } dicow_mt_chunk;   /* elements [start, start + len) of tensors[tensor]; 16 bytes */
/* Per-class scalars (fp32 values of torch's double-precision host arithmetic): decay = 1 - lr wd, step_size = lr / (1 - beta1^t),
 * bc2_sqrt = sqrt(1 - beta2^t), lerp_w = 1 - beta1, beta2, one_minus_beta2 = 1 - beta2, eps.  Passed BY VALUE as a kernel argument. */
typedef struct {
    float decay[DICOW_MT_MAX_CLASSES]; float step_size[DICOW_MT_MAX_CLASSES]; float bc2_sqrt[DICOW_MT_MAX_CLASSES];
    float lerp_w[DICOW_MT_MAX_CLASSES]; float beta2[DICOW_MT_MAX_CLASSES]; float one_minus_beta2[DICOW_MT_MAX_CLASSES];
    float eps[DICOW_MT_MAX_CLASSES];
    int32_t n_classes;
} dicow_mt_adamw_classes;
int dicow_multi_chunk_elems(void);
/* One launch over every chunk; tensors whose class lies outside [cls_base, cls_base + n_classes) are left alone (a call with more
 * than DICOW_MT_MAX_CLASSES classes is several launches over the same table).  clip_coef: NULL, or a device float the gradients are
 * multiplied by on the fly (g itself is not written): out[2] of dicow_multi_sumsq_f32. */
int dicow_multi_adamw_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks,
                          const dicow_mt_adamw_classes* cls, int cls_base, const float* clip_coef, void* stream);
/* Deterministic (fixed order, no float atomics) sum of squares of every g: out[0] = sum, out[1] = sqrt(sum), out[2] = min(1, max_norm /
 * (out[1] + 1e-6)) (NaN propagates, as in torch's clip).  ws: dicow_multi_sumsq_ws_bytes(n_chunks) bytes, 16-byte aligned, ZERO before the first
 * call (left zero by every call); one call in flight per workspace. */
int64_t dicow_multi_sumsq_ws_bytes(int64_t n_chunks);
int dicow_multi_sumsq_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks, void* ws, int64_t ws_bytes,
                          float* out, float max_norm, void* stream);
/* g *= coef[0] in place, coef read from device memory (out + 2 of dicow_multi_sumsq_f32). */
int dicow_multi_scale_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks, const float* coef, void* stream);

/* ------------------------------------------------------------------------------------------------ tensor statistics (ABI 7, additive)
 * Per-tensor statistics and histograms over a multi-tensor table (watch.py; the reference's `watch_grads`, src/utils/trainers.py:19-28:
 * wandb.watch(log='all') logs a 64-bin histogram of every parameter and gradient).  `which` (0..3) picks the column p, g, m or v of the
 * table; first_chunk[n_tensors + 1] (device, int64) is each tensor's chunk range (chunks are in table order; optim.first_chunks).
 * Per tensor ONE 64-byte record:
 *   sum, sumsq        over the FINITE elements, in double: one partial per table chunk, a tensor's partials added in chunk order -- the
 *                     bits depend on the data and the table only, never on a grid
 *   min, max, absmax  over the finite elements; none: min = +inf, max = -inf, absmax = 0.  Which signed zero is returned is unspecified
 *   n_nan, n_posinf, n_neginf, n_zero   exact counts (n_zero: both signs); n_finite = n - n_nan - n_posinf - n_neginf
 * and, with bins >= 1, hist[t * bins + b] (int64; OVERWRITTEN, not accumulated) over the finite elements:
 *   min == max : every finite element in bin 0 (the host renders wandb's one-bin form)
 *   otherwise  : b = min(bins - 1, (int)((x - min) * (float)bins / (max - min))), every operation rounded to fp32, the division the
 *                correctly rounded one; where max - min overflows fp32 the same formula on x/2, min/2, max/2 (torch.histc is undefined
 *                there).  The conversion saturates: a quotient of +inf ((x - min) * bins overflowed) is the last bin.
 * bins = 0 skips the histogram pass (hist may be NULL).  Three launches on `stream`, no host synchronisation, capturable; integer adds
 * only (no float atomics).  ws: dicow_tensor_stats_ws_bytes() bytes, 16-byte aligned, any contents; one call in flight per workspace.
 * grid: 0 = default, > 0 forces every pass's grid (tests: the results do not depend on it).  n_tensors = 0 or only empty tensors: valid.
 * DICOW_ERR_INVALID (dicow_last_error names the limit): bins outside 0..DICOW_STATS_MAX_BINS, which outside 0..3, a short or misaligned
 * workspace, NULL arguments.  The table lives on the device, so the call cannot see a NULL column pointer of a non-empty tensor: the
 * host side (watch.tensor_stats) refuses it when it builds the table, and the kernels treat such a tensor as empty instead of reading. */
#define DICOW_STATS_MAX_BINS 128
typedef struct {
    double sum, sumsq;
    float min, max, absmax;
    int32_t reserved;       /* 0 */
    int64_t n_nan, n_posinf, n_neginf, n_zero;
} dicow_tensor_stats_rec;   /* 64 bytes */
int64_t dicow_tensor_stats_ws_bytes(int64_t n_tensors, int64_t n_chunks, int bins);
int dicow_tensor_stats_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_tensors, int64_t n_chunks,
                           const int64_t* first_chunk, int which, int bins, void* ws, int64_t ws_bytes,
                           dicow_tensor_stats_rec* out, int64_t* hist, int grid /* 0: default; >0: forced, for tests */, void* stream);


/* ------------------------------------------------------------------------------------------------ EXPERIMENTAL (not part of the stable ABI)
 * Declared only under -DDICOW_EXPERIMENTAL_ABI and exported only by a library built with -DDICOW_EXPERIMENTS (build.sh --exp -> libdicow_hip_exp.so).
 * Round 4's LayerNorm fold: built, parity-tested (tests/test_gpu_lnfold.py) and measured 3-4 % SLOWER than the two LayerNorm launches it
 * deletes (profiles/r04_lnfold.txt) -- kept for A/B builds, out of the stable ABI.  The tail fields of dicow_gemm_args (lnstat ... ln_nslots) belong to
 * it and must be zero for a stable-ABI library, which refuses the two flags. */
#ifdef DICOW_EXPERIMENTAL_ABI
/* LayerNorm folded into the GEMMs on either side of it (ABI 4; HF:modeling_whisper.py:392-405 via encoder.py:216-221: the
 * pre-LN encoder layer's self_attn_layer_norm -> q/k/v and final_layer_norm -> fc1).  With W' = bf16(gamma . W) (column scale),
 *   LN(h) W^T + b = rstd_r (bf16(h) W'^T) - rstd_r mean_r colsum(W')_n + (beta W^T + b)_n
 * so the GEMM that PRODUCES the residual stream h (out-proj / fc2 with the fp32 residual epilogue) also stores bf16(h) and per-row
 * partial (sum, sum of squares) of the fp32 h, and the GEMM that CONSUMES LN(h) reads bf16(h) as its A operand and applies the
 * row scale + rank-one correction in its epilogue: the LayerNorm launch between them disappears.  Rounding point: bf16 of the
 * un-normalised h instead of bf16 of LN(h) (one bf16 rounding per operand element either way). */
#define DICOW_EPI_LNSTAT  2048   /* producer: with BIAS | RESIDUAL | OUT_F32 (| FDDT): aux <- bf16 copy of the fp32 result (ld = ldaux), lnstat[m][slot] <- partial (sum, sum sq) */
#define DICOW_EPI_LNFOLD  4096   /* consumer: acc -> rstd_m acc - rstd_m mean_m ln_c[n] before bias / scale / GELU; A = the producer's bf16 copy, B = W', bias = beta W^T + b */
#define DICOW_LN_SLOTS 16        /* partial slots per row of lnstat: [M][16][2] fp32; slot = 4 * (column tile of 320) + 2 * wave column + {0: 128 main columns, 1: 32 tail columns} */
/* 1 when dicow_gemm_nt will run this DICOW_EPI_LNSTAT problem (flags BIAS | RESIDUAL | OUT_F32 [| FDDT] | LNSTAT) on the persistent
   ring kernel's 192 x 320 tiles -- the only producer of the row partials (needs N % 320 == 0, N <= 1280) -- else 0 */
int dicow_gemm_nt_lnstat_ok(const dicow_gemm_args* a);
/* Weights of a Linear that follows a LayerNorm, folded (once per optimizer step): W fp32 [N, K], gamma / beta fp32 [K], bias fp32 [N] or
   NULL -> Wf bf16 [N, ldw] = bf16(gamma_k W_nk), c fp32 [N] = sum_k float(Wf_nk), bf fp32 [N] = bias_n + sum_k beta_k float(bf16(W_nk)) */
int dicow_lnfold_prep(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, int64_t ldw, float* c, float* bf,
                      int N, int K, void* stream);
#endif  /* DICOW_EXPERIMENTAL_ABI */

#ifdef __cplusplus
}
#endif
#endif /* DICOW_HIP_H */

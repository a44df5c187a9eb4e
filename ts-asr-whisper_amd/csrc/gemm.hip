// bf16 MFMA GEMMs for gfx950 (v_mfma_f32_32x32x16_bf16), LDS-staged with global_load_lds (16 B/lane DMA).
//
//   dicow_gemm_nt : C[M,N] = epi(A[M,K] . B[N,K]^T)       forward Linear / conv-as-GEMM and every dgrad
//   dicow_gemm_tn : C[N1,N2] += sum_m A[m,N1] . B[m,N2]    every weight gradient
//
// Tile 128x128, K-step 64, 256 threads = 4 waves in 2x2, each wave 64x64 = 2x2 MFMA tiles of 32x32 (64 fp32
// accumulators/lane).  Two LDS stages (2 x 32 KiB) -> 2 workgroups per CU; the next stage's DMA is in flight
// while the current one is consumed (counted s_waitcnt vmcnt, raw s_barrier -- see cdna_hip_programming.md
// "Pipelining across barriers").  LDS images are lane-linear (DMA constraint) so the bank-conflict swizzle is
// applied to the per-lane SOURCE address and again on the fragment read (rule 21 of the guide).
//
// MFMA operand order is swapped (a = weight rows n, b = activation rows m) so that a lane's accumulator quad
// holds 4 CONSECUTIVE n for one m: the epilogue then issues 8-byte (bf16) / 16-byte (fp32) row-major stores
// and float4 bias / residual loads.
#include <stdlib.h>
#include "common.h"

#define BM 128
#define BN 128
#define BK 64
#define STAGE_BYTES (BM * BK * 2)          // 16 KiB per operand per stage
#define NT_LDS_BYTES (4 * STAGE_BYTES)     // A0 B0 A1 B1
#define NT_FDDT_FLAGS (DICOW_EPI_BIAS | DICOW_EPI_RESIDUAL | DICOW_EPI_OUT_F32 | DICOW_EPI_FDDT)
#define NT_RES_FLAGS (DICOW_EPI_BIAS | DICOW_EPI_RESIDUAL | DICOW_EPI_OUT_F32)
#define NT_RES_LN_FLAGS (NT_RES_FLAGS | DICOW_EPI_LNSTAT)                      /* out-proj / fc2 producing bf16 copy + row partials */
#define NT_FDDT_LN_FLAGS (NT_FDDT_FLAGS | DICOW_EPI_LNSTAT)                    /* fc2 + next layer's FDDT + partials of the conditioned rows */
#define NT_QKV_LN_FLAGS (DICOW_EPI_BIAS | DICOW_EPI_SCALE_N | DICOW_EPI_LNFOLD)
#define NT_FC1I_LN_FLAGS (DICOW_EPI_BIAS | DICOW_EPI_GELU | DICOW_EPI_LNFOLD)
#define NT_FC1T_LN_FLAGS (DICOW_EPI_BIAS | DICOW_EPI_GELU | DICOW_EPI_GELU_DAUX | DICOW_EPI_LNFOLD)

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((gbl_void_t*)gsrc, (lds_void_t*)lds_dst, 16, 0, 0);
}

#ifndef NT_GM
#define NT_GM 8           // rows of a super-tile of the grouped order (round 5 sweep: profiles/r05_gm_sweep.txt)
#endif
// grouped + XCD-aware tile order: consecutive tile ids share A/B panels; block b lands on XCD b % 8, so give
// each XCD a contiguous chunk of the grouped order (bijective for any grid size).
__device__ __forceinline__ void tile_coords_id(int ntm, int ntn, int bid, int& tm, int& tn) {
    const int nwg = ntm * ntn;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    const int GM = NT_GM;
    const int per_group = GM * ntn;
    const int group = id / per_group, rem = id - group * per_group;
    const int first_m = group * GM;
    const int gsize = (ntm - first_m) < GM ? (ntm - first_m) : GM;
    tm = first_m + rem % gsize;
    tn = rem / gsize;
}
__device__ __forceinline__ void tile_coords(int ntm, int ntn, int& tm, int& tn) { tile_coords_id(ntm, ntn, blockIdx.x, tm, tn); }

// ------------------------------------------------------------------------------------------------ NT
// LDS image of a [128 rows][64 k] bf16 tile: row stride 128 B; 16-B chunk c of row r stored at chunk
// c ^ ((r >> 1) & 7)  (conflict-free for ds_read_b128 fragment reads, 16 lanes/row-group).
__device__ __forceinline__ void nt_stage(const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
                                         int64_t lda, int64_t ldb, int M, int N, int m0, int n0, int k0, char* sA,
                                         char* sB, int wave, int lane) {
    const int rr = lane >> 3, p = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + rr;
        const int c = p ^ ((row >> 1) & 7);
        int gm = m0 + row; gm = gm < M ? gm : M - 1;
        int gn = n0 + row; gn = gn < N ? gn : N - 1;
        glds16(A + (int64_t)gm * lda + k0 + c * 8, sA + (wave * 4 + i) * 1024);
        glds16(B + (int64_t)gn * ldb + k0 + c * 8, sB + (wave * 4 + i) * 1024);
    }
}

// one (A,B) pair of the four DMA instruction pairs of a stage: lets the k-loop spread the DMA issue between its MFMA
// groups -- a burst of 8 back-to-back DMAs per wave fills the CU's vector-memory queue and BLOCKS the in-order wave
// at issue, which serialises fill and compute (measured: step time = fill + MFMA instead of max(fill, MFMA)).
__device__ __forceinline__ void nt_stage_part(const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
                                              int64_t lda, int64_t ldb, int M, int N, int m0, int n0, int k0, char* sA,
                                              char* sB, int wave, int lane, int i) {
    const int rr = lane >> 3, p = lane & 7;
    const int row = (wave * 4 + i) * 8 + rr;
    const int c = p ^ ((row >> 1) & 7);
    int gm = m0 + row; gm = gm < M ? gm : M - 1;
    int gn = n0 + row; gn = gn < N ? gn : N - 1;
    glds16(A + (int64_t)gm * lda + k0 + c * 8, sA + (wave * 4 + i) * 1024);
    glds16(B + (int64_t)gn * ldb + k0 + c * 8, sB + (wave * 4 + i) * 1024);
}

__device__ __forceinline__ bf16x8_t lds_frag_nt(const char* s, int row, int c) {
    return *reinterpret_cast<const bf16x8_t*>(s + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
}

// FLAGS >= 0: the epilogue flag set is a compile-time constant (branch-free, small code); FLAGS < 0: runtime `rflags`.
// pre_bias / pre_aux / pre_res: operand values the caller already holds (loaded ahead of the stores -- vmcnt retires in
// order, so a load issued after a burst of stores waits for all of them); NULL = load here.
template <int FLAGS = -1>
__device__ __forceinline__ void nt_epilogue_math(const dicow_gemm_args& a, int rflags, float (&v)[4], float (&dg)[4], int m, int n,
                                                 const unsigned short* aux, const float4* pre_bias, const uint2* pre_aux,
                                                 const float4* pre_res) {
    const int flags = FLAGS >= 0 ? FLAGS : rflags;
    if (flags & DICOW_EPI_BIAS) {
        const float4 bv = pre_bias ? *pre_bias : *reinterpret_cast<const float4*>(a.bias + n);
        v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
    }
    if (flags & DICOW_EPI_SCALE_N) {
        if (n < a.scale_ncols) { v[0] *= a.scale; v[1] *= a.scale; v[2] *= a.scale; v[3] *= a.scale; }
    }
    if (flags & DICOW_EPI_GELU) {
        if (flags & DICOW_EPI_GELU_DAUX) {
            // the activation and its derivative are both taken at the bf16-rounded pre-activation (AMP: fc1 output is bf16)
#pragma unroll
            for (int e = 0; e < 4; ++e) gelu_erf_both(bf2f(f2bf(v[e])), v[e], dg[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) dg[e] = v[e];         // aux receives the pre-activation
            // AMP: the Linear / conv output is a bf16 tensor, so the activation sees the ROUNDED value -- with or without a
            // saved pre-activation (the inference forward and the decoder step must give what the training forward gives)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf(bf2f(f2bf(v[e])));
        }
    }
    if (flags & (DICOW_EPI_GELU_BWD | DICOW_EPI_MUL_AUX)) {
        const uint2 u = pre_aux ? *pre_aux : *reinterpret_cast<const uint2*>(aux + (int64_t)m * a.ldaux + n);
        float f[4] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                      __uint_as_float(u.y & 0xffff0000u)};
        if (flags & DICOW_EPI_GELU_BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = gelu_erf_grad(f[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= f[e];
    }
    if (flags & DICOW_EPI_RESIDUAL) {
        const float4 rv = pre_res ? *pre_res : *reinterpret_cast<const float4*>(a.residual + (int64_t)m * a.ldr + n);
        // AMP: the Linear output is rounded to bf16 before the fp32 residual add
        v[0] = bf2f(f2bf(v[0])) + rv.x; v[1] = bf2f(f2bf(v[1])) + rv.y;
        v[2] = bf2f(f2bf(v[2])) + rv.z; v[3] = bf2f(f2bf(v[3])) + rv.w;
    }
}

// NQ quads of one pass at once (compile-time flags only), stage-major like gelu_cdf_pdf_n: v / dg hold 4 * NQ values, quad u
// at [4u, 4u + 4).  All quads share the column quad n (one bias quad); pre_aux / pre_res point at NQ consecutive entries.
// The diagonal FDDT of one output quad in the reference's evaluation order (FDDT.py:41-63: separate fp32 multiplies / adds, no
// contraction -- the same packed IEEE operations as fddt_ln.hip's fddt_diag_pair, so the result is bit-identical to the row kernel's)
typedef __attribute__((ext_vector_type(2))) float f32x2g_t;
__device__ __forceinline__ void nt_fddt_quad(float* v, const float4* w, const float4* b, const float* m) {
#pragma clang fp contract(off)
    const f32x2g_t hl = {v[0], v[1]}, hr = {v[2], v[3]};
    f32x2g_t tl[4], tr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const f32x2g_t mc = {m[c], m[c]};
        tl[c] = (hl * f32x2g_t{w[c].x, w[c].y} + f32x2g_t{b[c].x, b[c].y}) * mc;
        tr[c] = (hr * f32x2g_t{w[c].z, w[c].w} + f32x2g_t{b[c].z, b[c].w}) * mc;
    }
    const f32x2g_t ol = ((tl[0] + tl[1]) + tl[2]) + tl[3], orr = ((tr[0] + tr[1]) + tr[2]) + tr[3];
    v[0] = ol.x; v[1] = ol.y; v[2] = orr.x; v[3] = orr.y;
}
template <int FLAGS, int NQ>
__device__ __forceinline__ void nt_epilogue_math_n(const dicow_gemm_args& a, float (&v)[4 * NQ], float (&dg)[4 * NQ], int n,
                                                   const float4& bv, const uint2* pre_aux, const float4* pre_res) {
    constexpr int NE = 4 * NQ;
    if (FLAGS & DICOW_EPI_BIAS) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) { v[4 * u] += bv.x; v[4 * u + 1] += bv.y; v[4 * u + 2] += bv.z; v[4 * u + 3] += bv.w; }
    }
    if (FLAGS & DICOW_EPI_SCALE_N) {
        if (n < a.scale_ncols) {
#pragma unroll
            for (int e = 0; e < NE; ++e) v[e] *= a.scale;
        }
    }
    if (FLAGS & DICOW_EPI_GELU) {
        constexpr int NP = NE / 2;
        f32x2_t x[NP], cdf[NP], pdf[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {                                  // AMP: the activation sees the bf16-rounded Linear output
            const unsigned w = pack_bf16x2(v[2 * i], v[2 * i + 1]);
            x[i] = f32x2_t{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
        }
        gelu_cdf_pdf_p<NP, (FLAGS & DICOW_EPI_GELU_DAUX) != 0>(x, cdf, pdf);
        if (FLAGS & DICOW_EPI_GELU_DAUX) {
#pragma unroll
            for (int i = 0; i < NP; ++i) { const f32x2_t d = __builtin_elementwise_fma(x[i], pdf[i], cdf[i]); dg[2 * i] = d.x; dg[2 * i + 1] = d.y; }
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e) dg[e] = v[e];                  // aux receives the pre-activation
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) { const f32x2_t g = x[i] * cdf[i]; v[2 * i] = g.x; v[2 * i + 1] = g.y; }
    }
    if (FLAGS & (DICOW_EPI_GELU_BWD | DICOW_EPI_MUL_AUX)) {
        float f[NE];
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const uint2 w = pre_aux[u];
            f[4 * u] = __uint_as_float(w.x << 16); f[4 * u + 1] = __uint_as_float(w.x & 0xffff0000u);
            f[4 * u + 2] = __uint_as_float(w.y << 16); f[4 * u + 3] = __uint_as_float(w.y & 0xffff0000u);
        }
        if (FLAGS & DICOW_EPI_GELU_BWD) {
            constexpr int NP = NE / 2;
            f32x2_t x[NP], cdf[NP], pdf[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) x[i] = f32x2_t{f[2 * i], f[2 * i + 1]};
            gelu_cdf_pdf_p<NP, true>(x, cdf, pdf);
#pragma unroll
            for (int i = 0; i < NP; ++i) { const f32x2_t d = __builtin_elementwise_fma(x[i], pdf[i], cdf[i]); f[2 * i] = d.x; f[2 * i + 1] = d.y; }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) v[e] *= f[e];
    }
    if (FLAGS & DICOW_EPI_RESIDUAL) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const float4 rv = pre_res[u];                               // AMP: the Linear output is rounded to bf16 before the fp32 residual add
            v[4 * u] = bf2f(f2bf(v[4 * u])) + rv.x; v[4 * u + 1] = bf2f(f2bf(v[4 * u + 1])) + rv.y;
            v[4 * u + 2] = bf2f(f2bf(v[4 * u + 2])) + rv.z; v[4 * u + 3] = bf2f(f2bf(v[4 * u + 3])) + rv.w;
        }
    }
}

template <int FLAGS = -1>
__device__ __forceinline__ void nt_epilogue_quad(const dicow_gemm_args& a, int rflags, float (&v)[4], int m, int n,
                                                 unsigned short* Cb, float* Cf, unsigned short* aux,
                                                 const float4* pre_bias = nullptr, const uint2* pre_aux = nullptr,
                                                 const float4* pre_res = nullptr) {
    const int flags = FLAGS >= 0 ? FLAGS : rflags;
    float dg[4];
    nt_epilogue_math<FLAGS>(a, rflags, v, dg, m, n, aux, pre_bias, pre_aux, pre_res);
    if ((flags & DICOW_EPI_GELU) && aux)
        *reinterpret_cast<uint2*>(aux + (int64_t)m * a.ldaux + n) = make_uint2(pack_bf16x2(dg[0], dg[1]), pack_bf16x2(dg[2], dg[3]));
    if (flags & DICOW_EPI_OUT_F32) {
        float* cp = Cf + (int64_t)m * a.ldc + n;
        if (flags & DICOW_EPI_ACCUM) {
            const float4 old = *reinterpret_cast<const float4*>(cp);
            v[0] += old.x; v[1] += old.y; v[2] += old.z; v[3] += old.w;
        }
        *reinterpret_cast<float4*>(cp) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<uint2*>(Cb + (int64_t)m * a.ldc + n) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

template <int STAGES, bool PRIO>
__global__ void __launch_bounds__(256, STAGES == 2 ? 2 : 4) gemm_nt_kernel(const dicow_gemm_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
    int tm, tn;
    tile_coords(ntm, ntn, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int bz = blockIdx.z;
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.A) + (int64_t)bz * a.strideA;
    const unsigned short* B = reinterpret_cast<const unsigned short*>(a.B) + (int64_t)bz * a.strideB;
    const int wm = wave >> 1, wn = wave & 1;

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = a.K / BK;
    if (STAGES == 2) nt_stage(A, B, a.lda, a.ldb, a.M, a.N, m0, n0, 0, smem, smem + STAGE_BYTES, wave, lane);
    for (int t = 0; t < nk; ++t) {
        char* sA = smem + (STAGES == 2 ? (t & 1) * 2 * STAGE_BYTES : 0);
        char* sB = sA + STAGE_BYTES;
        if (STAGES == 1) {
            // single LDS stage (32 KiB): 4 workgroups per CU hide each other's load / barrier phases
            nt_stage(A, B, a.lda, a.ldb, a.M, a.N, m0, n0, t * BK, sA, sB, wave, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (t + 1 < nk) {
            char* nA = smem + ((t + 1) & 1) * 2 * STAGE_BYTES;
            nt_stage(A, B, a.lda, a.ldb, a.M, a.N, m0, n0, (t + 1) * BK, nA, nA + STAGE_BYTES, wave, lane);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = kk * 2 + (lane >> 5);
            bf16x8_t wf[2], xf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wf[i] = lds_frag_nt(sB, wn * 64 + i * 32 + (lane & 31), c);
#pragma unroll
            for (int j = 0; j < 2; ++j) xf[j] = lds_frag_nt(sA, wm * 64 + j * 32 + (lane & 31), c);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
        }
        if (PRIO) __builtin_amdgcn_s_setprio(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    // ---- epilogue
    const int flags = a.flags;
    const int hh = lane >> 5;
    unsigned short* Cb = reinterpret_cast<unsigned short*>(a.C) + (int64_t)bz * a.strideC;
    float* Cf = reinterpret_cast<float*>(a.C) + (int64_t)bz * a.strideC;
    unsigned short* aux = reinterpret_cast<unsigned short*>(a.aux) + (int64_t)bz * a.strideAux;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + wm * 64 + j * 32 + (lane & 31);
        if (m >= a.M) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + i * 32 + 8 * q + 4 * hh;
                if (n >= a.N) continue;
                float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                nt_epilogue_quad(a, flags, v, m, n, Cb, Cf, aux);
            }
        }
    }
}

// The 128 x 128 kernel for problems too small for the persistent ring kernel (whisper-base: M = 12000, N = 512 -- a third of that
// step), round 3.  Same tile, LDS image, step order and epilogue as gemm_nt_kernel<2, false>; the next stage is requested through
// a buffer descriptor with per-lane byte offsets computed ONCE and a scalar k offset -- no address arithmetic per step (the
// pointer form costs two 64-bit adds per request: 16 VALU instructions per step next to 16 MFMAs).  whisper-base B = 8, whole
// step from one hipGraph: 7.81-7.83 ms against 7.87-7.88 (tools/_c40.sh).
// Also tried (removed; the record is profiles/r06_base_kernel_table.txt): ONE barrier per step, the 8 requests of stage t+1 threaded behind the first eight MFMAs of
// stage t, or issued in a burst behind the barrier.  In isolation (same operands over and over: L2-warm) that form is 5-12 %
// faster on every whisper-base shape (tools/bench_base_shapes.py: fc2 47.0 -> 42.8 us, fc1 dgrad 36.4 -> 32.1); inside the step
// it is 3 % SLOWER (8.09-8.14 ms: the kernel's 116 launches 2.93 ms against 2.68): a stage then has half a step of flight
// instead of a whole one, and operands that the previous kernel has just written do not arrive that fast.
// Needs 32-bit byte offsets (the host checks) and K >= 2 k-steps.
__global__ void __launch_bounds__(256, 2) gemm_nt128t_kernel(const dicow_gemm_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
    int tm, tn;
    tile_coords(ntm, ntn, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int bz = blockIdx.z;
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.A) + (int64_t)bz * a.strideA;
    const unsigned short* B = reinterpret_cast<const unsigned short*>(a.B) + (int64_t)bz * a.strideB;
    const int wm = wave >> 1, wn = wave & 1;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(A), 0, 0xffffffffu, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(B), 0, 0xffffffffu, 0x00020000);
    unsigned offA[4], offB[4];
    {
        const int rr = lane >> 3, p = lane & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 8 + rr;
            const int c = p ^ ((row >> 1) & 7);
            int gm = m0 + row; gm = gm < a.M ? gm : a.M - 1;
            int gn = n0 + row; gn = gn < a.N ? gn : a.N - 1;
            offA[i] = (unsigned)(((int64_t)gm * a.lda + c * 8) * 2);
            offB[i] = (unsigned)(((int64_t)gn * a.ldb + c * 8) * 2);
        }
    }
    // request i < 8 of this wave: i < 4 -> A row group wave*4 + i, else B row group wave*4 + i - 4; KB = k offset in bytes
#define NT128_DMA(I, SA, KB)                                                                                                  \
    { if ((I) < 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)((SA) + (wave * 4 + (I)) * 1024), 16, offA[(I) & 3], (KB), 0, 0); \
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_t*)((SA) + STAGE_BYTES + (wave * 4 + (I) - 4) * 1024), 16, offB[(I) & 3], (KB), 0, 0); }

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = a.K / BK;
    __amdgpu_buffer_rsrc_t ra = rsA, rb = rsB;        // switched to an empty descriptor (no traffic) for the step after the last
#pragma unroll
    for (int i = 0; i < 8; ++i) NT128_DMA(i, smem, 0)
    for (int t = 0; t < nk; ++t) {
        char* sA = smem + (t & 1) * 2 * STAGE_BYTES;
        char* sB = sA + STAGE_BYTES;
        char* nA = smem + ((t + 1) & 1) * 2 * STAGE_BYTES;
        const int kb = (t + 1) * BK * 2;
        if (t + 1 == nk) {                            // keeps the step code (and its scheduling region) free of branches
            ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(A), 0, 0u, 0x00020000);
            rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(B), 0, 0u, 0x00020000);
        }
        // old order with the cheap addressing: requests of stage t+1 first (its slot was released by the barrier that ended step
        // t-1), then wait for stage t -- a stage has a whole step of flight
#pragma unroll
        for (int e = 0; e < 8; ++e) NT128_DMA(e, nA, kb)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = kk * 2 + (lane >> 5);
            bf16x8_t wf[2], xf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wf[i] = lds_frag_nt(sB, wn * 64 + i * 32 + (lane & 31), c);
#pragma unroll
            for (int j = 0; j < 2; ++j) xf[j] = lds_frag_nt(sA, wm * 64 + j * 32 + (lane & 31), c);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing (empty-descriptor) requests
#undef NT128_DMA

    // ---- epilogue (as gemm_nt_kernel)
    const int flags = a.flags;
    const int hh = lane >> 5;
    unsigned short* Cb = reinterpret_cast<unsigned short*>(a.C) + (int64_t)bz * a.strideC;
    float* Cf = reinterpret_cast<float*>(a.C) + (int64_t)bz * a.strideC;
    unsigned short* aux = reinterpret_cast<unsigned short*>(a.aux) + (int64_t)bz * a.strideAux;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + wm * 64 + j * 32 + (lane & 31);
        if (m >= a.M) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + i * 32 + 8 * q + 4 * hh;
                if (n >= a.N) continue;
                float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                nt_epilogue_quad(a, flags, v, m, n, Cb, Cf, aux);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ NT, 64 x 64 tiles, deep ring
// The decoder's GEMMs at training time (whisper-base B = 8: M = 1024 rows, N = 512 ... 2048, K = 512 / 2048 -- 74 launches per
// step) are 32-128 tiles of 128 x 128: most CUs idle, and each workgroup walks its 8-32 k-steps with ONE stage in flight, i.e. a
// full memory round trip per step (15-28 us per launch for 0.5-2 GFLOP: a fifth of that step).  Here the tile is 64 x 64 (four
// waves, one 32 x 32 accumulator block each: 4x the workgroups) and the LDS holds a ring of S stages of 16 KiB (A 64 rows x 128 B,
// B likewise) with S - 1 of them in flight: for K = 512 every k-step of the tile is requested before the first one is computed, so
// the launch costs about one round trip instead of eight.  Same LDS image, fragment reads and epilogue as gemm_nt128t_kernel;
// one barrier per step: a wave waits for its own share of stage t (vmcnt), the barrier makes everybody's visible AND says every
// wave has finished reading stage t - 1, whose slot then receives stage t + S - 1.  After the last stage the requests go to an
// empty buffer descriptor (no traffic) so that the counted waits stay uniform.  Needs 32-bit byte offsets and K % 64 == 0.
template <int S>
__global__ void __launch_bounds__(256, S > 4 ? 1 : 2) gemm_nt64_kernel(const dicow_gemm_args a) {
    constexpr int SB = 16384;                          // stage bytes: A 8 KiB + B 8 KiB
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntm = (a.M + 63) / 64, ntn = (a.N + 63) / 64;
    int tm, tn;
    tile_coords(ntm, ntn, tm, tn);
    const int m0 = tm * 64, n0 = tn * 64;
    const int bz = blockIdx.z;
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.A) + (int64_t)bz * a.strideA;
    const unsigned short* B = reinterpret_cast<const unsigned short*>(a.B) + (int64_t)bz * a.strideB;
    const int wm = wave >> 1, wn = wave & 1;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(A), 0, 0xffffffffu, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(B), 0, 0xffffffffu, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(A), 0, 0u, 0x00020000);
    unsigned offA[2], offB[2];
    {
        const int rr = lane >> 3, p = lane & 7;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (wave * 2 + i) * 8 + rr;          // row group wave*2 + i of the 64-row image (8 rows x 128 B per request)
            const int c = p ^ ((row >> 1) & 7);
            int gm = m0 + row; gm = gm < a.M ? gm : a.M - 1;
            int gn = n0 + row; gn = gn < a.N ? gn : a.N - 1;
            offA[i] = (unsigned)(((int64_t)gm * a.lda + c * 8) * 2);
            offB[i] = (unsigned)(((int64_t)gn * a.ldb + c * 8) * 2);
        }
    }
    const int nk = a.K / BK;
    // stage T (k offset T * 64) -> slot T % S; past the end: the empty descriptor
#define NT64_STAGE(T)                                                                                                          \
    {                                                                                                                          \
        const int t_ = (T);                                                                                                    \
        const bool live_ = t_ < nk;                                                                                            \
        const __amdgpu_buffer_rsrc_t ra_ = live_ ? rsA : rsE, rb_ = live_ ? rsB : rsE;                                         \
        char* d_ = smem + (t_ % S) * SB;                                                                                       \
        const int kb_ = t_ * BK * 2;                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                        \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (lds_void_t*)(d_ + (wave * 2 + i) * 1024), 16, offA[i], kb_, 0, 0);  \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (lds_void_t*)(d_ + 8192 + (wave * 2 + i) * 1024), 16, offB[i], kb_, 0, 0); \
        }                                                                                                                      \
    }
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int t = 0; t < S - 1; ++t) NT64_STAGE(t)
    for (int t = 0; t < nk; ++t) {
        // outstanding here: stages t .. t + S - 2 (4 requests each, in order): the oldest one must have landed
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(4 * (S - 2)) : "memory");   // (and my fragment reads of stage t - 1 are done)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        NT64_STAGE(t + S - 1)
        const char* sA = smem + (t % S) * SB;
        const char* sB = sA + 8192;
        bf16x8_t wf[4], xf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = kk * 2 + (lane >> 5);
            wf[kk] = lds_frag_nt(sB, wn * 32 + (lane & 31), c);
            xf[kk] = lds_frag_nt(sA, wm * 32 + (lane & 31), c);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kk], xf[kk], acc, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing (empty-descriptor) requests
#undef NT64_STAGE

    // ---- epilogue (as gemm_nt_kernel)
    const int flags = a.flags;
    const int hh = lane >> 5;
    unsigned short* Cb = reinterpret_cast<unsigned short*>(a.C) + (int64_t)bz * a.strideC;
    float* Cf = reinterpret_cast<float*>(a.C) + (int64_t)bz * a.strideC;
    unsigned short* aux = reinterpret_cast<unsigned short*>(a.aux) + (int64_t)bz * a.strideAux;
    const int m = m0 + wm * 32 + (lane & 31);
    if (m < a.M) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + wn * 32 + 8 * q + 4 * hh;
            if (n >= a.N) continue;
            float v[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
            nt_epilogue_quad(a, flags, v, m, n, Cb, Cf, aux);
        }
    }
}

#ifndef NT128W
#define NT128W 0                 // mid-size problems on 128 x 256 ring tiles, one workgroup per CU (experiments/gemm_nt128w.inc): whisper-base
#endif                           // B = 8 step 7.49 ms against 6.95-7.00 with the 128 x 128 tiles at two workgroups per CU (profiles/r04_nt128w.txt)
#if NT128W
#include "experiments/gemm_nt128w.inc"
#endif

// ------------------------------------------------------------------------------------------------ NT, skinny (M <= 16)
// One decoder step of a batch of <= 16 hypotheses: C[M, N] = x[M, K] W[N, K]^T streams the whole weight matrix once for a
// handful of rows -- HBM-bound, and the 128-row tiles above spend 25 us per call on it with N / 128 workgroups.  Here a
// workgroup owns 16 output columns: v_mfma_f32_16x16x32_bf16 with the WEIGHT rows as the A operand and x as B, so that a lane
// ends up with 4 consecutive n of one row m (what nt_epilogue_quad stores); the four waves split the k-steps (interleaved),
// every lane keeps 8 x 16-byte weight loads in flight, partial sums meet in LDS.  N / 16 workgroups: 80 for a D x D
// projection, 3248 for the tied head.
#define SKINNY_UNROLL 8
__global__ void __launch_bounds__(256) gemm_nt_skinny_kernel(const dicow_gemm_args a) {
    __shared__ float red[3][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * 16, nrow = n0 + (lane & 15), m = lane & 15, kc = (lane >> 4) * 8;
    const bool mvalid = m < a.M;
    const unsigned short* W = reinterpret_cast<const unsigned short*>(a.B) + (int64_t)(nrow < a.N ? nrow : a.N - 1) * a.ldb + kc;
    const unsigned short* X = reinterpret_cast<const unsigned short*>(a.A) + (int64_t)(mvalid ? m : 0) * a.lda + kc;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const int nsteps = a.K / 32;
    for (int s = wave; s < nsteps; s += 4 * SKINNY_UNROLL) {
        bf16x8_t wv[SKINNY_UNROLL], xv[SKINNY_UNROLL];
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) {
            const int st = s + 4 * u;
            const int so = (st < nsteps ? st : s) * 32;                      // past the end: a harmless re-read, weighted by zero
            wv[u] = *reinterpret_cast<const bf16x8_t*>(W + so);
            xv[u] = *reinterpret_cast<const bf16x8_t*>(X + so);
            if (!mvalid || st >= nsteps) xv[u] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u], xv[u], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave - 1][lane][e] = acc[e];
    }
    __syncthreads();
    if (wave > 0) return;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[e] + red[0][lane][e] + red[1][lane][e] + red[2][lane][e];
    const int n = n0 + (lane >> 4) * 4;
    if (!mvalid || n >= a.N) return;
    unsigned short* Cb = reinterpret_cast<unsigned short*>(a.C);
    float* Cf = reinterpret_cast<float*>(a.C);
    unsigned short* aux = reinterpret_cast<unsigned short*>(a.aux);
    nt_epilogue_quad(a, a.flags, v, m, n, Cb, Cf, aux);
}

// The product's big-problem kernel is gemm_ntr_kernel (gemm_ntr.inc).  Its predecessors -- the 8-wave 256 x 256 kernel with its
// ablation switches, the two-stage persistent 4-wave kernel (gemm_ntw_kernel: its header explains the one-wave-per-SIMD layout,
// the tile shapes and the LDS-transposed epilogue that the ring kernel keeps) and the staggered 4-stage experiment -- are only
// compiled into diagnostic builds (-DDICOW_ABLATIONS, selected at run time with DICOW_NT_VARIANT; tools/build_variants.sh).
#define NT256_STAGE (2 * 256 * BK * 2)       // A + B = 64 KiB
#define NT256_LDS (2 * NT256_STAGE)
#ifdef DICOW_ABLATIONS
#include "experiments/gemm_nt_two_stage.inc"      // the two-stage kernels of rounds 1-2 (A/B baselines)
#endif  // DICOW_ABLATIONS

// ---- LayerNorm fold, producer side (DICOW_EPI_LNSTAT): butterfly reductions over the lanes of a row with DPP lane moves.
// ln_merge<CTRL>(a, b, bit): two values whose partial sums live in lane pairs (l, l ^ k) -- CTRL = the DPP move that reads lane
// l ^ k -- become ONE: a lane with bit clear ends with a(l) + a(l ^ k), a lane with bit set with b(l) + b(l ^ k); the number of
// live values halves with every lane bit, and after the last one lane l holds the row total of value number (l & 15).
template <int CTRL, int BANK = 0xf>
__device__ __forceinline__ float ln_dpp(float old, float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, 0xf, BANK, false));
}
template <int CTRL>
__device__ __forceinline__ float ln_merge(float a, float b, bool bit) {
    const float keep = bit ? b : a, send = bit ? a : b;
    return keep + ln_dpp<CTRL>(0.f, send);
}
// lane l ^ 4 inside a row of 16: banks 0 / 2 read lane l + 4 (row_shl:4), banks 1 / 3 lane l - 4 (row_shr:4)
__device__ __forceinline__ float ln_xor4(float x) { return ln_dpp<0x114, 0xA>(ln_dpp<0x104, 0x5>(0.f, x), x); }
__device__ __forceinline__ float ln_merge4(float a, float b, bool bit) {
    const float keep = bit ? b : a, send = bit ? a : b;
    return keep + ln_xor4(send);
}
#include "gemm_ntr.inc"
// Round 5's two structural experiments (csrc/experiments/, compiled only into the experiments library or an A/B build that sets a mask):
// gemm_nt2_kernel (two workgroups per CU, 128 x 256 tiles) and gemm_ntq_kernel (320 x 256 tiles) -- both parity-green, both measured
// slower or equal (profiles/r05_nt2_two_workgroups.txt, r05_ntq_320x256.txt).  Class bits of the masks: 1 fp32 residual, 2 training fc1
// (GELU + gelu'), 4 inference fc1 (GELU), 8 dgrad x gelu' (+ column sums), 16 bias / bias + q scale, 32 plain; NTQ bit 1024: also where
// its rounds of workgroups pad worse than the ring kernel's.  In the experiments library DICOW_NT2_MASK / DICOW_NTQ_MASK /
// DICOW_NT2_DELAY select at run time (tests/test_gpu_experiments.py).
#ifndef NT2_MASK
#define NT2_MASK 0
#endif
#ifndef NT2_SLOTS
#define NT2_SLOTS 2               // workgroups per CU the grid is sized for (1: diagnostic, a lone workgroup per CU)
#endif
#ifndef NT2_DELAY
#define NT2_DELAY 0               // second half of the grid starts NT2_DELAY x 64 clocks late
#endif
#ifndef NTQ_MASK
#define NTQ_MASK 0
#endif
#if defined(DICOW_EXPERIMENTS) || defined(DICOW_ABLATIONS) || NT2_MASK || NTQ_MASK
#define NT_EXPERIMENT_KERNELS 1
#include "experiments/gemm_nt2.inc"
#include "experiments/gemm_ntq.inc"
#else
#define NT_EXPERIMENT_KERNELS 0
#endif

#ifdef DICOW_ABLATIONS
#include "experiments/gemm_nt256s.inc"
#endif  // DICOW_ABLATIONS

#include <atomic>
#include <mutex>
static std::atomic<int> g_gemm_cus{0};     // dicow_set_gemm_cus(): CUs the persistent kernel may occupy (0 = all)
extern "C" int dicow_set_gemm_cus(int n) { return g_gemm_cus.exchange(n > 0 ? n : 0); }

// Which GEMM kernel instantiations this process has launched (name as a profiler prints it -> count): bench.py checks the
// committed rocprofv3 counter summary against it, so that a summary taken on other kernels is refused instead of quoted.
#include <map>
#include <mutex>
#include <string>
static std::mutex g_disp_mu;
static std::map<std::string, long> g_disp;
static void disp_note(const char* fmt, int a0 = 0, int a1 = 0, int a2 = 0) {
    char b[96];
    snprintf(b, sizeof b, fmt, a0, a1, a2);
    std::lock_guard<std::mutex> lk(g_disp_mu);
    ++g_disp[b];
}
extern "C" int dicow_gemm_dispatch_log(char* buf, int cap) {
    std::lock_guard<std::mutex> lk(g_disp_mu);
    int n = 0;
    for (const auto& kv : g_disp) {
        const int w = snprintf(buf ? buf + n : nullptr, buf && cap > n ? cap - n : 0, "%s\t%ld\n", kv.first.c_str(), kv.second);
        if (w < 0) break;
        n += w;
        if (buf && n >= cap) { n = cap - 1; break; }
    }
    return n;
}

// ------------------------------------------------------------------------------------------------ NT host dispatch
// Thresholds of the plan (the -D overrides are for A/B builds, tools/build_var.sh):
// 256 x 256 tiles from which the persistent ring kernel takes over from the 128 x 128 tiles (two workgroups per CU, two barriers
// per k-step).  Below ~200 tiles the ring kernel leaves most CUs idle and its prologue / epilogue are not amortised: whisper-base
// B = 8, whose N = 512 GEMMs are 94 tiles, measured 7.72 ms per step with the threshold at 200 and 8.01-8.03 ms at 90 or 40
// (round 3, tools/_c32.sh)
#ifndef NT_BIG_TILES
#define NT_BIG_TILES 200
#endif
// 128 x 128 tile count up to which the 64 x 64 deep-ring kernel takes the problem (0: never)
#ifndef NT64_MAX_TILES128
#define NT64_MAX_TILES128 128
#endif

// The epilogue flag sets with compile-time instantiations of the persistent kernels -- the ONE list from which the kernel attributes,
// the launch switches and the logged kernel names are generated.  NT_EPILOGUES_COMMON(X): the eight sets of the training step, which
// gemm_ntr_kernel has in 256 x 256 and 192 x 320 and the experiments' gemm_nt2 / gemm_ntq / gemm_ntw kernels have as well.
// NT_EPILOGUES(BOTH, W35): all of gemm_ntr_kernel's -- BOTH(F) both tile shapes, W35(F) 192 x 320 only; -1 is the run-time-flags
// fallback for every other set.
#define NT_EPILOGUES_COMMON(X)                                                                                                  \
    X(0) X(DICOW_EPI_BIAS) X(DICOW_EPI_BIAS | DICOW_EPI_SCALE_N) X(DICOW_EPI_BIAS | DICOW_EPI_GELU) X(NT_RES_FLAGS)             \
    X(DICOW_EPI_BIAS | DICOW_EPI_GELU | DICOW_EPI_GELU_DAUX) X(DICOW_EPI_MUL_AUX) X(DICOW_EPI_MUL_AUX | DICOW_EPI_COLSUM)
#ifdef DICOW_EXPERIMENTS
#define NT_HAS_LN_EPILOGUES 1
#define NT_EPILOGUES_LN(BOTH, W35) W35(NT_RES_LN_FLAGS) W35(NT_FDDT_LN_FLAGS) BOTH(NT_QKV_LN_FLAGS) BOTH(NT_FC1I_LN_FLAGS) BOTH(NT_FC1T_LN_FLAGS)
#else
#define NT_HAS_LN_EPILOGUES 0
#define NT_EPILOGUES_LN(BOTH, W35)
#endif
#define NT_EPILOGUES(BOTH, W35) BOTH(-1) NT_EPILOGUES_COMMON(BOTH) W35(NT_FDDT_FLAGS) NT_EPILOGUES_LN(BOTH, W35)

static int g_ncu_all = 256;                // CUs of the device (gemm_nt_setup)
static int nt_ncu() {                      // CUs left to the persistent kernel (dicow_set_gemm_cus)
    const int lim = g_gemm_cus.load();
    return (lim > 0 && lim < g_ncu_all) ? lim : g_ncu_all;
}

// one-time kernel attributes (dynamic LDS sizes) and device properties; the C ABI may be entered from any host thread -- the
// forward thread and autograd's backward thread both launch GEMMs -- so this runs under std::call_once.
// This function is the first to name the template kernels, so its order is the order of the kernels in the code object: keep it (a
// build with the same kernels in another order measured +0.15 % per step, profiles/r07_nt_dispatch_refactor_ab.txt).
static void gemm_nt_setup() {
    (void)hipFuncSetAttribute((const void*)gemm_nt_kernel<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, NT_LDS_BYTES);
    (void)hipFuncSetAttribute((const void*)gemm_nt128t_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NT_LDS_BYTES);
    (void)hipFuncSetAttribute((const void*)gemm_nt64_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 16384);
    (void)hipFuncSetAttribute((const void*)gemm_nt64_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 16384);
    (void)hipFuncSetAttribute((const void*)gemm_nt_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, NT_LDS_BYTES);     // (launched by DICOW_NT_VARIANT 2 of a diagnostic build only)
#define W35(F) (void)hipFuncSetAttribute((const void*)gemm_ntr_kernel<(F), 3, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, NTR_LDS);
#define BOTH(F) (void)hipFuncSetAttribute((const void*)gemm_ntr_kernel<(F), 4, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, NTR_LDS); W35(F)
    NT_EPILOGUES(BOTH, W35)
#undef BOTH
#undef W35
    hipDeviceProp_t pr;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&pr, dev) == hipSuccess) g_ncu_all = pr.multiProcessorCount;
}

// the FLAGS template argument that serves a flag set
static int nt_ct_flags(int flags) {
    switch (flags) {
#define X(F) case (F):
        NT_EPILOGUES(X, X)
#undef X
            return flags;
        default: return -1;
    }
}
static void ntr_launch(int ct_flags, bool use35, dim3 grid, hipStream_t stream, const dicow_gemm_args& a) {
#define W35(F) case (F): hipLaunchKernelGGL((gemm_ntr_kernel<(F), 3, 5>), grid, dim3(256), NTR_LDS, stream, a); break;
#define BOTH(F) case (F):                                                                                                       \
        if (use35) hipLaunchKernelGGL((gemm_ntr_kernel<(F), 3, 5>), grid, dim3(256), NTR_LDS, stream, a);                       \
        else hipLaunchKernelGGL((gemm_ntr_kernel<(F), 4, 4>), grid, dim3(256), NTR_LDS, stream, a);                             \
        break;
    switch (ct_flags) { NT_EPILOGUES(BOTH, W35) }
#undef BOTH
#undef W35
}

// ---- the plan: which kernel runs a problem, on which tiles and grid.  Host arithmetic on the arguments alone -- no launch, no
// validation (callers that have not validated get an answer for K % 64 == 0 only) -- shared by the dispatcher and the queries of the ABI.
enum nt_family_t {
    NT_FAM_SKINNY,      // gemm_nt_skinny_kernel: a decoding step, M <= 16
    NT_FAM_RING,        // gemm_ntr_kernel, persistent: use35 / grid / colsum_rows apply
    NT_FAM_64,          // gemm_nt64_kernel<stages64>: few 128 x 128 tiles
    NT_FAM_128T,        // gemm_nt128t_kernel
    NT_FAM_GENERIC      // gemm_nt_kernel<2, false>: 64-bit operand offsets or a single k-step
};
struct nt_plan_t {
    nt_family_t family;
    bool off32, big;    // every operand within 32-bit byte offsets of its per-batch base; enough 256 x 256 tiles for the ring kernel
    int grid;           // workgroups (ring: of the balanced persistent grid; others: per batch)
    int stages64;       // NT_FAM_64: ring depth, 8 or 4
    bool use35;         // ring: 192 x 320 tiles instead of 256 x 256
    int colsum_rows;    // ring: partial rows a fused DICOW_EPI_COLSUM leaves in the workspace
    int ncu;            // ring: CUs the grid was balanced for
    bool wide_ok;       // ring: the epilogue tolerates the smaller tiles at this N
    int64_t w35, w44;   // ring: padded area of whole rounds of `ncu` workgroups, per tile shape
    int splitk;         // equal k ranges a deep contraction with a small output is cut into (1: none)
};
struct nt_knobs_t { int variant, big_tiles; };     // diagnostic builds only (experiments/gemm_nt_routes.inc); {0, NT_BIG_TILES} otherwise

// ---- deep contractions with a small output (the tied LM head's dgrad: [B L, D] = d_logits [B L, 51968] . E: 32 output tiles at
// whisper-base, 160 at large-v3-turbo, 812 k-steps each): the contraction is cut into S equal ranges that run as the S
// "batches" of one launch (operand stride = the range's k offset) writing fp32 partials to the caller's workspace; one small
// kernel adds them in range order and rounds once.  Deterministic; only taken when the caller provides the workspace.
static int nt_splitk_count(const dicow_gemm_args& a, int64_t tiles128) {
    if (a.batch > 1 || (a.flags & ~DICOW_EPI_OUT_F32) != 0 || a.bias || a.residual || a.aux) return 1;
    if (a.K % BK != 0 || a.K < 8192 || a.M <= 16) return 1;
    if (tiles128 >= 2 * g_ncu_all) return 1;                   // enough tiles already (two 128 x 128 workgroups per CU)
    const int nk = a.K / BK;
    int best = 1;
    for (int sp = 2; sp <= 64; ++sp) {
        if (nk % sp != 0 || nk / sp < 16) continue;            // equal ranges of at least 1024 columns
        best = sp;
        if (tiles128 * sp >= 2 * g_ncu_all) break;             // the first divisor that fills every workgroup slot
    }
    return best;
}

static nt_plan_t nt_plan(const dicow_gemm_args& a, int ncu, int variant = 0, int big_tiles = NT_BIG_TILES) {
    nt_plan_t p = {};
    const int batch = a.batch > 0 ? a.batch : 1;
    const int64_t tiles128 = (int64_t)dicow_cdiv(a.M, BM) * dicow_cdiv(a.N, BN);
    p.splitk = nt_splitk_count(a, tiles128);
    // the persistent kernel wins once it can put ~one workgroup on every CU; smaller problems keep the 128x128 tiles.
    // It addresses its operands with 32-bit byte offsets from a per-batch base and needs at least two 64-deep k-steps
    const bool ab32 = (int64_t)a.M * a.lda * 2 < (1ll << 31) && (int64_t)a.N * a.ldb * 2 < (1ll << 31);
    p.off32 = ab32 && (int64_t)a.M * a.ldc * 4 < (1ll << 31) && (int64_t)a.M * a.ldaux * 2 < (1ll << 31) &&
              (int64_t)a.M * a.ldr * 4 < (1ll << 31);
    const int64_t t44 = (int64_t)dicow_cdiv(a.M, 256) * dicow_cdiv(a.N, 256) * batch;
    p.big = p.off32 && a.K >= 2 * BK && t44 >= big_tiles;
    if (a.M <= 16 && batch == 1 && variant == 0) {        // a decoding step: stream the weights once
        p.family = NT_FAM_SKINNY;
        p.grid = dicow_cdiv(a.N, 16);
        return p;
    }
    if ((variant >= 4 || (variant == 0 && p.big)) && a.M >= 256 && a.N >= 256) {
        p.family = NT_FAM_RING;
        p.ncu = ncu;
        // tile shape: 192x320 where its whole rounds of `ncu` workgroups pad the problem less than 256x256 does AND the
        // output is narrow (M = 24000: the N = 1280 shapes gain 2-5 %; N = 3840 is neutral and N = 5120 with the GELU
        // epilogue loses -- more, smaller tiles mean more epilogues).  Diagnostic builds: DICOW_NT_VARIANT 21 / 22 force the
        // ring kernel's 256x256 / 192x320 tiles, 12 / 13 the two-stage kernel's
        const int64_t t35 = (int64_t)dicow_cdiv(a.M, 192) * dicow_cdiv(a.N, 320) * batch;
        p.w44 = dicow_cdiv(t44, ncu) * 256 * 256;
        p.w35 = dicow_cdiv(t35, ncu) * 192 * 320;
        // (round 3: with the cheaper GELU the inference fc1 -- bias + GELU, no saved derivative -- gains 8 us per launch from
        // the smaller tiles at N = 5120 too: encoder forward 38.86 -> 38.60 ms in-situ; the training epilogues still lose)
        p.wide_ok = a.N <= 2048 || a.flags == (DICOW_EPI_BIAS | DICOW_EPI_GELU) || a.flags == NT_FC1I_LN_FLAGS;
        // (only the 192 x 320 instantiations carry the FDDT and LNSTAT epilogues)
        const bool fddt = (a.flags & DICOW_EPI_FDDT) != 0, lnstat = (a.flags & DICOW_EPI_LNSTAT) != 0;
        // (round 6, interleaved A/B of the tile choice per epilogue kind -- profiles/r06_epilogues.txt: the choices above hold, except that a
        // PLAIN product (no epilogue work at all: the dgrads of out-proj / qkv / fc1) is 1.7-2.1 % faster on 256 x 256 at N = 1280 too)
        const bool plain256 = a.flags == 0;
        p.use35 = fddt || lnstat || variant == 13 || variant == 22 ||
                  (variant != 12 && variant != 21 && a.N >= 320 && p.wide_ok && !plain256 && p.w35 < p.w44);
        const int total = (int)(p.use35 ? t35 : t44);
        // balanced grid: with r = ceil(total / ncu) rounds needed anyway, ceil(total / r) workgroups each take r (or
        // r - 1) tiles -- e.g. 470 tiles run on 235 workgroups x 2 instead of 214 x 2 + 42 x 1: same makespan, fewer
        // CUs competing for L2 / HBM / power while the last round is partial (measured 0.304 -> 0.287 ms)
        p.grid = dicow_cdiv(total, dicow_cdiv(total, ncu));
        p.colsum_rows = 2 * dicow_cdiv(a.M, p.use35 ? 192 : 256);
        return p;
    }
    // few 128 x 128 tiles (the decoder at training time: M = batch x label length): 64 x 64 tiles on a deep ring; otherwise the
    // descriptor-addressed 128 x 128 kernel where one batch slice of A / B fits 32-bit byte offsets and K has two k-steps
    const bool t128 = ab32 && a.K >= 2 * BK;
    if (NT64_MAX_TILES128 > 0 && t128 && variant == 0 && tiles128 * batch <= NT64_MAX_TILES128) {
        p.family = NT_FAM_64;
        p.grid = dicow_cdiv(a.M, 64) * dicow_cdiv(a.N, 64);
        p.stages64 = (int64_t)p.grid * batch <= g_ncu_all ? 8 : 4;       // one workgroup per CU anyway: the whole 128 KiB ring
    } else {
        p.family = t128 ? NT_FAM_128T : NT_FAM_GENERIC;
        p.grid = (int)tiles128;
    }
    return p;
}

static int nt_splitk_plan(const dicow_gemm_args* a) { return nt_plan(*a, nt_ncu()).splitk; }
extern "C" int64_t dicow_gemm_nt_splitk_ws_bytes(const dicow_gemm_args* a) {
    if (!a) return 0;
    const int sp = nt_splitk_plan(a);
    return sp > 1 ? (int64_t)sp * a->M * a->N * 4 : 0;
}
__global__ void nt_splitk_reduce_kernel(const float* __restrict__ ws, int splits, int64_t mn, int N, void* __restrict__ C, int64_t ldc,
                                        int out_f32) {
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < mn; i += (int64_t)gridDim.x * blockDim.x * 4) {
        float4 t = *reinterpret_cast<const float4*>(ws + i);
        for (int z = 1; z < splits; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(ws + (int64_t)z * mn + i);
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const int64_t m = i / N; const int n = (int)(i - m * N);
        if (out_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(C) + m * ldc + n) = t;
        else *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(C) + m * ldc + n) = make_uint2(pack_bf16x2(t.x, t.y), pack_bf16x2(t.z, t.w));
    }
}

// ws for DICOW_EPI_COLSUM: the fused path needs 2 * ceil(M/192) partial rows (the ring kernel; 2 * ceil(M/128) for gemm_nt2_kernel
// wherever that kernel is compiled in); the fallback runs dicow_colsum_bf16 on C
extern "C" int64_t dicow_gemm_nt_colsum_ws_bytes(int M, int N) {
    const int64_t fused = (int64_t)2 * dicow_cdiv(M, NT_EXPERIMENT_KERNELS ? 128 : 192) * N * 4, fb = dicow_colsum_ws_bytes(M, N);
    return fused > fb ? fused : fb;
}

extern "C" int dicow_gemm_nt_is_persistent(const dicow_gemm_args* a) {
    return (a && a->K % BK == 0 && nt_plan(*a, nt_ncu()).family == NT_FAM_RING) ? 1 : 0;
}

#ifdef DICOW_EXPERIMENTS
extern "C" int dicow_gemm_nt_lnstat_ok(const dicow_gemm_args* a) {
    // (the LNSTAT instantiations are 192 x 320 only and the plan forces that shape for them: what remains to ask is whether
    // the problem reaches the persistent kernel at all and whether its columns are whole 320-wide tiles that fit the 16 slots)
    return (dicow_gemm_nt_is_persistent(a) && a->M >= 256 && a->N >= 320 && a->N % 320 == 0 && a->N <= 1280 &&
            (int64_t)a->M * 128 < (1ll << 31) && (a->batch <= 1)) ? 1 : 0;
}
#endif

static int gemm_nt_impl(const dicow_gemm_args* a, void* stream, bool* fused_colsum, int* colsum_rows);

extern "C" int dicow_gemm_nt(const dicow_gemm_args* a, void* stream) {
    DICOW_REQUIRE(a && a->A && a->B && a->C, "gemm_nt: null operand");
    if (!(a->flags & DICOW_EPI_COLSUM)) {
        const int sp = (a->colsum_ws && a->N % 4 == 0 && a->ldc % 4 == 0) ? nt_splitk_plan(a) : 1;
        if (sp > 1 && a->colsum_ws_bytes >= (int64_t)sp * a->M * a->N * 4) {
            dicow_gemm_args b = *a;
            b.K = a->K / sp; b.batch = sp; b.strideA = b.K; b.strideB = b.K;
            b.C = a->colsum_ws; b.ldc = a->N; b.strideC = (int64_t)a->M * a->N; b.flags = DICOW_EPI_OUT_F32;
            b.colsum_ws = nullptr; b.colsum_ws_bytes = 0; b.colsum_out = nullptr;
            const int rc = gemm_nt_impl(&b, stream, nullptr, nullptr);
            if (rc != DICOW_OK) return rc;
            const int64_t mn = (int64_t)a->M * a->N;
            int grid = (int)((mn / 4 + 255) / 256); if (grid > 2048) grid = 2048;
            hipLaunchKernelGGL(nt_splitk_reduce_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)a->colsum_ws, sp, mn,
                               a->N, a->C, a->ldc, (a->flags & DICOW_EPI_OUT_F32) ? 1 : 0);
            DICOW_CHECK_LAUNCH("nt_splitk_reduce");
            return DICOW_OK;
        }
        return gemm_nt_impl(a, stream, nullptr, nullptr);
    }
    DICOW_REQUIRE(a->colsum_out && a->colsum_ws && a->colsum_ws_bytes >= dicow_gemm_nt_colsum_ws_bytes(a->M, a->N),
                  "gemm_nt: COLSUM needs colsum_out and colsum_ws of dicow_gemm_nt_colsum_ws_bytes() bytes");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_OUT_F32) && a->batch <= 1, "gemm_nt: COLSUM supports a single bf16 result");
    bool fused = false;
    int rows = 0;
    int rc = gemm_nt_impl(a, stream, &fused, &rows);
    if (rc != DICOW_OK) return rc;
    if (fused)          // add the per-wave partial rows up: colsum_out[n] += sum_p ws[p][n]
        return dicow_launch_reduce_parts(reinterpret_cast<const float*>(a->colsum_ws), rows, a->N,
                                         a->colsum_out, a->N, (hipStream_t)stream);
    return dicow_colsum_bf16(a->C, a->ldc, a->colsum_out, a->M, a->N, a->colsum_ws, a->colsum_ws_bytes, stream);
}

// the fused column sums exist in the persistent kernels' MUL_AUX epilogue only: `flags` arrive without COLSUM and get it back here
static inline void nt_fuse_colsum(dicow_gemm_args* a, bool want_colsum, bool* fused_colsum) {
    if (want_colsum && a->flags == DICOW_EPI_MUL_AUX) { a->flags |= DICOW_EPI_COLSUM; *fused_colsum = true; }
}

// ---- the hook of the experiments: kernels and DICOW_NT_VARIANT routes of diagnostic builds live in csrc/experiments/
#define NT_NOT_ROUTED 1
#if NT_EXPERIMENT_KERNELS || NT128W
#include "experiments/gemm_nt_routes.inc"
#else
static inline nt_knobs_t nt_experiment_knobs() { return {0, NT_BIG_TILES}; }
static inline int nt_experiment_route(dicow_gemm_args*, const nt_plan_t&, int, bool, bool*, int*, hipStream_t) { return NT_NOT_ROUTED; }
#endif

static int nt_check_args(const dicow_gemm_args* a) {
    DICOW_REQUIRE(a && a->A && a->B && a->C, "gemm_nt: null operand");
    DICOW_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "gemm_nt: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    DICOW_REQUIRE(a->K % BK == 0, "gemm_nt: K=%d must be a multiple of %d (pad the operands)", a->K, BK);
    DICOW_REQUIRE(a->N % 4 == 0 && a->ldc % 4 == 0, "gemm_nt: N=%d and ldc=%ld must be multiples of 4", a->N, (long)a->ldc);
    DICOW_REQUIRE(a->lda % 8 == 0 && a->ldb % 8 == 0, "gemm_nt: lda/ldb must be multiples of 8 (16-byte rows)");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_BIAS) || a->bias, "gemm_nt: BIAS without bias pointer");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_RESIDUAL) || (a->residual && a->ldr % 4 == 0), "gemm_nt: RESIDUAL needs residual, ldr%%4==0");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_GELU_BWD) || (a->aux && a->ldaux % 4 == 0), "gemm_nt: GELU_BWD needs aux");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_ACCUM) || (a->flags & DICOW_EPI_OUT_F32), "gemm_nt: ACCUM needs OUT_F32");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_MUL_AUX) || a->aux, "gemm_nt: MUL_AUX needs aux");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_GELU_DAUX) || ((a->flags & DICOW_EPI_GELU) && a->aux), "gemm_nt: GELU_DAUX needs GELU and aux");
    DICOW_REQUIRE(!(a->aux) || a->ldaux % 4 == 0, "gemm_nt: ldaux must be a multiple of 4");
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_SCALE_N) || a->scale_ncols % 4 == 0, "gemm_nt: SCALE_N works on column quads, scale_ncols=%d", a->scale_ncols);
    return DICOW_OK;
}
// the epilogues that only the persistent kernel implements (FDDT, and the LayerNorm fold of the experiments library), against the plan
static int nt_check_ring_epilogues(const dicow_gemm_args* a, const nt_plan_t& p, int variant) {
    const int batch = a->batch > 0 ? a->batch : 1;
    const bool ring = variant == 0 && p.big && a->M >= 256 && a->N >= 320;
    DICOW_REQUIRE(NT_HAS_LN_EPILOGUES || !(a->flags & (DICOW_EPI_LNSTAT | DICOW_EPI_LNFOLD)), "gemm_nt: EPI_LNSTAT / EPI_LNFOLD are experimental (the LayerNorm fold measured slower, profiles/r04_lnfold.txt): build.sh --exp builds libdicow_hip_exp.so, which has them");
    DICOW_REQUIRE(!(a->flags & (DICOW_EPI_LNSTAT | DICOW_EPI_LNFOLD)) || ring,
                  "gemm_nt: EPI_LNSTAT / EPI_LNFOLD are implemented by the persistent kernel only (M=%d N=%d K=%d: ask dicow_gemm_nt_is_persistent / dicow_gemm_nt_lnstat_ok)", a->M, a->N, a->K);
    DICOW_REQUIRE(!(a->flags & DICOW_EPI_FDDT) || ring,
                  "gemm_nt: EPI_FDDT is implemented by the persistent kernel only (M=%d N=%d K=%d is below its threshold: ask dicow_gemm_nt_is_persistent)", a->M, a->N, a->K);
    const bool fddt = (a->flags & DICOW_EPI_FDDT) != 0, lnstat = (a->flags & DICOW_EPI_LNSTAT) != 0, lnfold = (a->flags & DICOW_EPI_LNFOLD) != 0;
    DICOW_REQUIRE(!fddt || ((a->flags == NT_FDDT_FLAGS || a->flags == NT_FDDT_LN_FLAGS) && variant == 0 && a->N >= 320 && batch == 1 && a->fddt_rowmask &&
                            a->fddt_w[0] && a->fddt_w[1] && a->fddt_w[2] && a->fddt_w[3] && a->fddt_b[0] && a->fddt_b[1] &&
                            a->fddt_b[2] && a->fddt_b[3]),
                  "gemm_nt: EPI_FDDT needs BIAS | RESIDUAL | OUT_F32, N >= 320, one batch, the eight vectors and the row masks");
    DICOW_REQUIRE(!lnstat || ((a->flags == NT_RES_LN_FLAGS || a->flags == NT_FDDT_LN_FLAGS) && variant == 0 && batch == 1 && a->aux &&
                              a->lnstat && a->N % 320 == 0 && a->N <= 1280 && (int64_t)a->M * 128 < (1ll << 31)),
                  "gemm_nt: EPI_LNSTAT needs BIAS | RESIDUAL | OUT_F32 [| FDDT], aux (the bf16 copy), lnstat, N %% 320 == 0, N <= 1280 (N=%d)", a->N);
    DICOW_REQUIRE(!lnfold || ((a->flags == NT_QKV_LN_FLAGS || a->flags == NT_FC1I_LN_FLAGS || a->flags == NT_FC1T_LN_FLAGS) && variant == 0 &&
                              batch == 1 && a->lnstat && a->ln_c && a->bias && a->ln_nslots > 0 && a->ln_nslots <= DICOW_LN_SLOTS &&
                              a->ln_nslots % 4 == 0 && a->ln_inv_dim > 0.f && (int64_t)a->M * 128 < (1ll << 31)),
                  "gemm_nt: EPI_LNFOLD needs BIAS with SCALE_N or GELU [| GELU_DAUX], lnstat, ln_c, ln_nslots (multiple of 4, <= 16), ln_inv_dim");
    return DICOW_OK;
}

static int gemm_nt_impl(const dicow_gemm_args* a_in, void* stream_, bool* fused_colsum, int* colsum_rows) {
    dicow_gemm_args a_copy = *a_in;
    dicow_gemm_args* a = &a_copy;
    const hipStream_t stream = (hipStream_t)stream_;
    const bool want_colsum = (a->flags & DICOW_EPI_COLSUM) != 0;
    a->flags &= ~DICOW_EPI_COLSUM;                    // put back where the fused epilogue exists (nt_fuse_colsum)
    int rc = nt_check_args(a);
    if (rc != DICOW_OK) return rc;
    static std::once_flag once;
    std::call_once(once, gemm_nt_setup);
    const nt_knobs_t knobs = nt_experiment_knobs();
    const nt_plan_t p = nt_plan(*a, nt_ncu(), knobs.variant, knobs.big_tiles);
    const dim3 grid(p.grid, 1, a->batch > 0 ? a->batch : 1);
    if (p.family == NT_FAM_SKINNY) {
        hipLaunchKernelGGL(gemm_nt_skinny_kernel, grid, dim3(256), 0, stream, *a);
        DICOW_CHECK_LAUNCH("gemm_nt_skinny_kernel");
        if (fused_colsum) *fused_colsum = false;
        return DICOW_OK;
    }
    rc = nt_check_ring_epilogues(a, p, knobs.variant);
    if (rc != DICOW_OK) return rc;
    rc = nt_experiment_route(a, p, knobs.variant, want_colsum, fused_colsum, colsum_rows, stream);
    if (rc != NT_NOT_ROUTED) return rc;
    switch (p.family) {
        case NT_FAM_RING: {
            nt_fuse_colsum(a, want_colsum, fused_colsum);
            if (colsum_rows) *colsum_rows = p.colsum_rows;
            const int ct = nt_ct_flags(a->flags);
            disp_note("gemm_ntr_kernel<%d, %d, %d>", ct, p.use35 ? 3 : 4, p.use35 ? 5 : 4);
            ntr_launch(ct, p.use35, dim3(p.grid), stream, *a);
            DICOW_CHECK_LAUNCH("gemm_nt (persistent)");
            return DICOW_OK;
        }
        case NT_FAM_64:
            if (p.stages64 == 8) hipLaunchKernelGGL(gemm_nt64_kernel<8>, grid, dim3(256), 8 * 16384, stream, *a);
            else hipLaunchKernelGGL(gemm_nt64_kernel<4>, grid, dim3(256), 4 * 16384, stream, *a);
            disp_note("gemm_nt64_kernel<%d>", p.stages64);
            break;
        case NT_FAM_128T:
            hipLaunchKernelGGL(gemm_nt128t_kernel, grid, dim3(256), NT_LDS_BYTES, stream, *a);
            disp_note("gemm_nt128t_kernel");
            break;
        default:
            hipLaunchKernelGGL((gemm_nt_kernel<2, false>), grid, dim3(256), NT_LDS_BYTES, stream, *a);
            disp_note("gemm_nt_kernel<2, false>");
            break;
    }
    DICOW_CHECK_LAUNCH("gemm_nt");
    return DICOW_OK;
}

// ------------------------------------------------------------------------------------------------ TN (weight gradients)
// LDS image of a [64 m][128 n] bf16 tile: row stride 256 B; 16-B chunk c of row m stored at chunk
// c ^ ((m & 3) << 2) (keeps the four rows of a ds_read_b64_tr_b16 block on distinct banks).
#define TK 64
#define TN_STAGE_BYTES (TK * 128 * 2)      // 16 KiB per operand per stage
#define TN_LDS_BYTES (4 * TN_STAGE_BYTES)

__device__ __forceinline__ void tn_stage(const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
                                         int64_t lda, int64_t ldb, int N1, int N2, int n1_0, int n2_0, int row_base,
                                         int rows_valid, char* sA, char* sB, int wave, int lane) {
    const int rr = lane >> 4, p = lane & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 4 + rr;
        const int c = p ^ ((row & 3) << 2);
        const int grow = row_base + (row < rows_valid ? row : rows_valid - 1);   // clamped (tail rows zeroed later)
        int ca = n1_0 + c * 8; ca = ca + 8 <= N1 ? ca : N1 - 8;
        int cb = n2_0 + c * 8; cb = cb + 8 <= N2 ? cb : N2 - 8;
        glds16(A + (int64_t)grow * lda + ca, sA + (wave * 4 + i) * 1024);
        glds16(B + (int64_t)grow * ldb + cb, sB + (wave * 4 + i) * 1024);
    }
}

// ds_read_b64_tr_b16: each lane supplies the address of 4 contiguous bf16; within a 16-lane group the 16x4 block
// is transposed so lane i receives element (i & 3) of lanes 4j + (i >> 2), j = 0..3  -- i.e. 4 consecutive ROWS of
// one column (probe: profiles/r01_probe_gfx950.txt).  All 8 reads of one 16-deep k-step (2 operands x 2 column
// blocks x rows {m..m+3, m+4..m+7}) and their wait are ONE asm statement so the compiler cannot touch the
// destination registers before the data has landed (cdna_hip_programming.md section 5.7 item 1).
__device__ __forceinline__ unsigned tn_tr_addr(const char* s, int m, int n) {
    return (unsigned)(uintptr_t)(s + m * 256 + ((((n >> 3) ^ ((m & 3) << 2))) << 4) + ((n & 7) << 1));
}
struct tn_frag_t { bf16x4_t r0, r1, r2, r3, r4, r5, r6, r7; };

// issue the 8 transposing reads of k-step OFF/4096 (no wait: they stay in flight behind the previous step's MFMAs)
template <int OFF>
__device__ __forceinline__ void tn_issue(tn_frag_t& f, unsigned b0, unsigned b1, unsigned a0, unsigned a1) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %8 offset:%12\n\t"
        "ds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
        "ds_read_b64_tr_b16 %2, %9 offset:%12\n\t"
        "ds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
        "ds_read_b64_tr_b16 %4, %10 offset:%12\n\t"
        "ds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
        "ds_read_b64_tr_b16 %6, %11 offset:%12\n\t"
        "ds_read_b64_tr_b16 %7, %11 offset:%13"
        : "=&v"(f.r0), "=&v"(f.r1), "=&v"(f.r2), "=&v"(f.r3), "=&v"(f.r4), "=&v"(f.r5), "=&v"(f.r6), "=&v"(f.r7)
        : "v"(b0), "v"(b1), "v"(a0), "v"(a1), "i"(OFF), "i"(OFF + 1024)
        : "memory");
}
// wait until at most N LDS reads are outstanding; names the fragment registers so that no consumer is scheduled
// above the wait and the compiler never touches them in between (cdna_hip_programming.md section 5.7 form (ii))
template <int N>
__device__ __forceinline__ void tn_wait(tn_frag_t& f) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(f.r0), "+v"(f.r1), "+v"(f.r2), "+v"(f.r3), "+v"(f.r4), "+v"(f.r5), "+v"(f.r6), "+v"(f.r7)
                 : "i"(N)
                 : "memory");
}
__device__ __forceinline__ void tn_mfma(f32x16_t (&acc)[2][2], const tn_frag_t& f) {
    const bf16x8_t f20 = __builtin_shufflevector(f.r0, f.r1, 0, 1, 2, 3, 4, 5, 6, 7);
    const bf16x8_t f21 = __builtin_shufflevector(f.r2, f.r3, 0, 1, 2, 3, 4, 5, 6, 7);
    const bf16x8_t f10 = __builtin_shufflevector(f.r4, f.r5, 0, 1, 2, 3, 4, 5, 6, 7);
    const bf16x8_t f11 = __builtin_shufflevector(f.r6, f.r7, 0, 1, 2, 3, 4, 5, 6, 7);
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f20, f10, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f20, f11, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f21, f10, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f21, f11, acc[1][1], 0, 0, 0);
}

__global__ void __launch_bounds__(256, 2) gemm_tn_kernel(const dicow_gemm_tn_args a, int tiles_per_batch, int total_tiles,
                                                         int tiles_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt1 = (a.N1 + 127) / 128, nt2 = (a.N2 + 127) / 128;
    int t1, t2;
    tile_coords(nt1, nt2, t1, t2);
    const int n1_0 = t1 * 128, n2_0 = t2 * 128;
    const int kt0 = blockIdx.z * tiles_per_split;
    int kt1 = kt0 + tiles_per_split; kt1 = kt1 < total_tiles ? kt1 : total_tiles;
    if (kt0 >= kt1) return;
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.A);
    const unsigned short* B = reinterpret_cast<const unsigned short*>(a.B);
    const int w1 = wave >> 1, w2 = wave & 1;

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto issue = [&](int kt, int buf) {
        const int b = kt / tiles_per_batch, lt = kt - b * tiles_per_batch;
        const int rv = (a.Mk - lt * TK) < TK ? (a.Mk - lt * TK) : TK;
        char* sA = smem + buf * 2 * TN_STAGE_BYTES;
        tn_stage(A + (int64_t)b * a.strideA, B + (int64_t)b * a.strideB, a.lda, a.ldb, a.N1, a.N2, n1_0, n2_0, lt * TK, rv,
                 sA, sA + TN_STAGE_BYTES, wave, lane);
    };

    issue(kt0, 0);
    // lane-constant parts of the transposing reads: group G -> 16-column block, u -> (row, 4-col) inside the block
    const int G = lane >> 4, u = lane & 15;
    const int tr_row = 8 * (G >> 1) + (u >> 2);          // + kk*16 (+4 for the second read)
    const int tr_col = 16 * (G & 1) + 4 * (u & 3);       // + 32*blk + wave offset
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        char* sA = smem + buf * 2 * TN_STAGE_BYTES;
        char* sB = sA + TN_STAGE_BYTES;
        if (kt + 1 < kt1) {
            issue(kt + 1, buf ^ 1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        {   // zero the rows of a partial contraction tile (the DMA fetched clamped duplicates there)
            const int lt = kt % tiles_per_batch;
            const int rv = (a.Mk - lt * TK) < TK ? (a.Mk - lt * TK) : TK;
            if (rv < TK) {
                for (int i = tid; i < (TK - rv) * 16; i += 256) {
                    const int off = (rv + (i >> 4)) * 256 + (i & 15) * 16;
                    *reinterpret_cast<uint4*>(sA + off) = make_uint4(0, 0, 0, 0);
                    *reinterpret_cast<uint4*>(sB + off) = make_uint4(0, 0, 0, 0);
                }
                __syncthreads();
            }
        }
        {
            const unsigned b0 = tn_tr_addr(sB, tr_row, w2 * 64 + tr_col), b1 = tn_tr_addr(sB, tr_row, w2 * 64 + 32 + tr_col);
            const unsigned a0 = tn_tr_addr(sA, tr_row, w1 * 64 + tr_col), a1 = tn_tr_addr(sA, tr_row, w1 * 64 + 32 + tr_col);
            tn_frag_t fa, fb;
            tn_issue<0>(fa, b0, b1, a0, a1);
            tn_issue<4096>(fb, b0, b1, a0, a1);
            tn_wait<8>(fa);
            tn_mfma(acc, fa);
            tn_issue<8192>(fa, b0, b1, a0, a1);
            tn_wait<8>(fb);
            tn_mfma(acc, fb);
            tn_issue<12288>(fb, b0, b1, a0, a1);
            tn_wait<8>(fa);
            tn_mfma(acc, fa);
            tn_wait<0>(fb);
            tn_mfma(acc, fb);
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    // ---- epilogue: C[n1][n2..n2+3] (+)= acc; a split contraction writes fp32 partials [split][N1][N2] to the workspace
    const int hh = lane >> 5;
    const bool to_ws = gridDim.z > 1;
    float* wsz = reinterpret_cast<float*>(a.ws) + (int64_t)blockIdx.z * a.N1 * a.N2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n1 = n1_0 + w1 * 64 + j * 32 + (lane & 31);
        if (n1 >= a.N1) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n2 = n2_0 + w2 * 64 + i * 32 + 8 * q + 4 * hh;
                if (n2 >= a.N2) continue;
                float4 v = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                if (to_ws) {
                    *reinterpret_cast<float4*>(wsz + (int64_t)n1 * a.N2 + n2) = v;
                    continue;
                }
                float* cp;
                if (a.seg_rows > 0 && n1 >= a.seg_rows) {
                    const int sg = n1 / a.seg_rows;
                    cp = a.C_seg[sg - 1] + (int64_t)(n1 - sg * a.seg_rows) * a.ldc + n2;
                } else {
                    cp = a.C + (int64_t)n1 * a.ldc + n2;
                }
                if (a.accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(cp);
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                }
                *reinterpret_cast<float4*>(cp) = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ TN, 256x256 tile
// Same pipeline as gemm_nt256_kernel (8 waves, 2 x 64 KiB stages, one barrier per 64-deep contraction step, fragments
// one k-slice ahead, last slice's MFMAs after the barrier, DMA spread two instruction pairs per slice); fragments come
// from ds_read_b64_tr_b16.  LDS image per operand: [64 m][256 n] bf16, 512-B rows, chunk c of row m at c ^ ((m&3)<<2).
#define TN256_OP (TK * 256 * 2)              // 32 KiB per operand per stage
#define TN256_STAGE (2 * TN256_OP)
#define TN256_LDS (5 * TN256_OP)              // ring of five halves

__device__ __forceinline__ unsigned tn256_tr_addr(const char* s, int m, int n) {
    return (unsigned)(uintptr_t)(s + m * 512 + ((((n >> 3) ^ ((m & 3) << 2))) << 4) + ((n & 7) << 1));
}
struct tn256_frag_t { bf16x4_t r[12]; };
template <int OFF>
__device__ __forceinline__ void tn256_issue(tn256_frag_t& f, const unsigned (&ad)[6]) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %12 offset:%18\n\t"  "ds_read_b64_tr_b16 %1, %12 offset:%19\n\t"
        "ds_read_b64_tr_b16 %2, %13 offset:%18\n\t"  "ds_read_b64_tr_b16 %3, %13 offset:%19\n\t"
        "ds_read_b64_tr_b16 %4, %14 offset:%18\n\t"  "ds_read_b64_tr_b16 %5, %14 offset:%19\n\t"
        "ds_read_b64_tr_b16 %6, %15 offset:%18\n\t"  "ds_read_b64_tr_b16 %7, %15 offset:%19\n\t"
        "ds_read_b64_tr_b16 %8, %16 offset:%18\n\t"  "ds_read_b64_tr_b16 %9, %16 offset:%19\n\t"
        "ds_read_b64_tr_b16 %10, %17 offset:%18\n\t" "ds_read_b64_tr_b16 %11, %17 offset:%19"
        : "=&v"(f.r[0]), "=&v"(f.r[1]), "=&v"(f.r[2]), "=&v"(f.r[3]), "=&v"(f.r[4]), "=&v"(f.r[5]), "=&v"(f.r[6]), "=&v"(f.r[7]),
          "=&v"(f.r[8]), "=&v"(f.r[9]), "=&v"(f.r[10]), "=&v"(f.r[11])
        : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "i"(OFF), "i"(OFF + 2048)
        : "memory");
}
template <int N>
__device__ __forceinline__ void tn256_wait(tn256_frag_t& f) {
    asm volatile("s_waitcnt lgkmcnt(%12)"
                 : "+v"(f.r[0]), "+v"(f.r[1]), "+v"(f.r[2]), "+v"(f.r[3]), "+v"(f.r[4]), "+v"(f.r[5]), "+v"(f.r[6]), "+v"(f.r[7]),
                   "+v"(f.r[8]), "+v"(f.r[9]), "+v"(f.r[10]), "+v"(f.r[11])
                 : "i"(N)
                 : "memory");
}
// r[0..3]: the two n2 blocks (lo,hi each); r[4..11]: the four n1 blocks
__device__ __forceinline__ void tn256_mfma(f32x16_t (&acc)[2][4], const tn256_frag_t& f) {
    bf16x8_t f2[2], f1[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) f2[i] = __builtin_shufflevector(f.r[2 * i], f.r[2 * i + 1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) f1[j] = __builtin_shufflevector(f.r[4 + 2 * j], f.r[5 + 2 * j], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f2[i], f1[j], acc[i][j], 0, 0, 0);
}

// (Tried and dropped: the 4-wave / 128x128-wave-tile / AGPR form that pays off for the NT kernel.  Here every MFMA operand
// comes from ds_read_b64_tr_b16 -- 16 LDS instructions per 16 MFMAs instead of 8 -- and a single wave per SIMD cannot hide
// their issue: 0.78 PF with batched reads, 0.73 PF with reads threaded between groups of 4 MFMAs, against 0.82 PF here.)
// One (output tile, contraction range) unit of the 256 x 256 TN kernel: contraction tiles [kt0, kt1) of the 256 x 256 output
// tile at (n1_0, n2_0).  wpart == nullptr: the result goes (accumulates) into C; otherwise it is a PARTIAL sum and is
// written to wpart with element (n1, n2) at wpart[(n1 - wr0) * wld + (n2 - wc0)].  Shared by the split-K kernel
// (gemm_tn256_kernel) and the grouped kernel (gemm_tn256g_kernel); the caller has made sure no LDS traffic is in flight.
__device__ __forceinline__ void tn256_unit(const dicow_gemm_tn_args& a, char* smem, int tiles_per_batch, int n1_0, int n2_0, int kt0,
                                           int kt1, float* wpart, int wr0, int wc0, int64_t wld) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.A);
    const unsigned short* B = reinterpret_cast<const unsigned short*>(a.B);
    const int w1 = wave >> 2, w2 = wave & 3;          // wave tile: n1 [w1*128, +128), n2 [w2*64, +64)

    f32x16_t acc[2][4];                               // [n2 block i][n1 block j]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int G = lane >> 4, u = lane & 15;
    const int tr_row = 8 * (G >> 1) + (u >> 2);
    const int tr_col = 16 * (G & 1) + 4 * (u & 3);
    // DMA through buffer descriptors: per-lane 32-bit byte offsets (row-in-tile * ld + swizzled, clamped column chunk) are
    // computed ONCE; a contraction tile only changes the scalar offset (and, across batches, the descriptor base).  The
    // pointer form cost ~75 VALU instructions per k-step (64-bit multiply-adds, clamps) on the issue port the 32 MFMAs
    // share.  num_records = Mk rows: the rows a partial last tile reaches past the end read as ZERO, which is exactly the
    // contribution they must make (no clamped duplicates to scrub out of LDS afterwards).
    unsigned voA[4], voB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = wave * 4 + i;                   // DMA instruction index: rows 2q, 2q+1 (1 KiB)
        const int row = 2 * q + (lane >> 5), p = lane & 31;
        const int c = p ^ ((row & 3) << 2);
        int ca = n1_0 + c * 8; ca = ca + 8 <= a.N1 ? ca : a.N1 - 8;
        int cb = n2_0 + c * 8; cb = cb + 8 <= a.N2 ? cb : a.N2 - 8;
        voA[i] = (unsigned)(((int64_t)row * a.lda + ca) * 2);
        voB[i] = (unsigned)(((int64_t)row * a.ldb + cb) * 2);
    }
    // LDS ring of five 32-KiB halves (all 160 KiB): contraction tile t (relative to kt0) keeps its A half in slot 2t mod 5 and
    // its B half in slot (2t + 1) mod 5.  At the top of step t (the barrier releases the halves of step t-1) the wave issues
    // B(t+1) and A(t+2): like gemm_ntr_kernel, the loop no longer drains its own DMA at every step (two stages + vmcnt(0) left
    // ONE stage in flight, and its latency -- not the matrix pipe -- set the step time); the counted wait lets the four newest
    // instructions (A(t+1)) stay in flight across the barrier.
    // The DMA of a half: four instructions per wave, addressed through a buffer descriptor whose num_records is ZERO once the
    // stream has run past the split's last tile -- the loop then needs no branch around its DMA (a branch ends the scheduling
    // region the instructions are threaded through) and the counted waits stay uniform; the dead loads fetch nothing.
    // (batch, tile-in-batch) of each stream advance incrementally: the division per half cost ~40 SALU instructions a step.
    struct tn_stream_t { int b, lt, rel, slot; };
    auto stream_next = [&](tn_stream_t& st) {
        if (++st.lt == tiles_per_batch) { st.lt = 0; ++st.b; }
        ++st.rel;
        st.slot = st.slot + 2 >= 5 ? st.slot - 3 : st.slot + 2;
    };
    const int b0 = kt0 / tiles_per_batch;
    tn_stream_t stA = {b0, kt0 - b0 * tiles_per_batch, 0, 0}, stB = {b0, kt0 - b0 * tiles_per_batch, 0, 1};
    const int nrel = kt1 - kt0;
    auto dmaA = [&](const tn_stream_t& st, int e0, int e1) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned short*>(A + (int64_t)st.b * a.strideA), 0, st.rel < nrel ? (unsigned)((int64_t)a.Mk * a.lda * 2) : 0u, 0x00020000);
        const int so = (int)((int64_t)st.lt * TK * a.lda * 2);
        char* dst = smem + st.slot * TN256_OP;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e >= e0 && e < e1)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(dst + (wave * 4 + e) * 1024), 16, voA[e], so, 0, 0);
    };
    auto dmaB = [&](const tn_stream_t& st, int e0, int e1) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned short*>(B + (int64_t)st.b * a.strideB), 0, st.rel < nrel ? (unsigned)((int64_t)a.Mk * a.ldb * 2) : 0u, 0x00020000);
        const int so = (int)((int64_t)st.lt * TK * a.ldb * 2);
        char* dst = smem + st.slot * TN256_OP;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e >= e0 && e < e1)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(dst + (wave * 4 + e) * 1024), 16, voB[e], so, 0, 0);
    };
    dmaA(stA, 0, 4); stream_next(stA);                // A(0)
    dmaB(stB, 0, 4); stream_next(stB);                // B(0)
    dmaA(stA, 0, 4); stream_next(stA);                // A(1)   (empty descriptor when the split has a single tile)
    tn256_frag_t f0, f1;
#pragma unroll
    for (int i = 0; i < 12; ++i) f1.r[i] = bf16x4_t{0, 0, 0, 0};      // "slice 3 of the tile before the first": adds nothing
    int sa = 0;                                       // slot of the A half of the step being computed
    // The eight DMA instructions of a step -- B(t+1), then A(t+2) -- are threaded between the MFMAs, two per slice: issued in
    // two batches next to the fragment reads each of them held the wave for ~100 cycles (a build without the DMA ran 25 %
    // faster, one that issued it and never waited ran no faster); among MFMAs in flight the issue costs a fraction of that.
#define TN_SPREAD() { __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); \
                      __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); \
                      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); }
    for (int kt = kt0; kt < kt1; ++kt) {
        const int sb = sa + 1 >= 5 ? sa - 4 : sa + 1;
        char* sA = smem + sa * TN256_OP;
        char* sB = smem + sb * TN256_OP;
        // everything but A(t+1) -- the four newest DMA instructions -- has landed
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        unsigned ad[6];
#pragma unroll
        for (int i = 0; i < 2; ++i) ad[i] = tn256_tr_addr(sB, tr_row, w2 * 64 + i * 32 + tr_col);
#pragma unroll
        for (int j = 0; j < 4; ++j) ad[2 + j] = tn256_tr_addr(sA, tr_row, w1 * 128 + j * 32 + tr_col);
        tn256_issue<0>(f0, ad);
        tn256_mfma(acc, f1);                          // slice 3 of the previous tile (landed before the barrier)
        dmaB(stB, 0, 2);
        TN_SPREAD()
        tn256_issue<8192>(f1, ad);
        tn256_wait<12>(f0);
        tn256_mfma(acc, f0);
        dmaB(stB, 2, 4); stream_next(stB);
        TN_SPREAD()
        tn256_issue<16384>(f0, ad);
        tn256_wait<12>(f1);
        tn256_mfma(acc, f1);
        dmaA(stA, 0, 2);
        TN_SPREAD()
        tn256_issue<24576>(f1, ad);
        tn256_wait<12>(f0);
        tn256_mfma(acc, f0);
        dmaA(stA, 2, 4); stream_next(stA);
        TN_SPREAD()
        sa = sa + 2 >= 5 ? sa - 3 : sa + 2;
    }
#undef TN_SPREAD
    tn256_wait<0>(f1);
    tn256_mfma(acc, f1);

    const int hh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n1 = n1_0 + w1 * 128 + j * 32 + (lane & 31);
        if (n1 >= a.N1) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n2 = n2_0 + w2 * 64 + i * 32 + 8 * q + 4 * hh;
                if (n2 >= a.N2) continue;
                float4 v = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                if (wpart) {                          // a partial sum: element (n1, n2) at wpart[(n1 - wr0) * wld + (n2 - wc0)]
                    *reinterpret_cast<float4*>(wpart + (int64_t)(n1 - wr0) * wld + (n2 - wc0)) = v;
                    continue;
                }
                float* cp;
                if (a.seg_rows > 0 && n1 >= a.seg_rows) {
                    const int sg = n1 / a.seg_rows;
                    cp = a.C_seg[sg - 1] + (int64_t)(n1 - sg * a.seg_rows) * a.ldc + n2;
                } else {
                    cp = a.C + (int64_t)n1 * a.ldc + n2;
                }
                if (a.accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(cp);
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                }
                *reinterpret_cast<float4*>(cp) = v;
            }
        }
    }
}

__global__ void __launch_bounds__(512, 2) gemm_tn256_kernel(const dicow_gemm_tn_args a, int tiles_per_batch, int total_tiles,
                                                            int tiles_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nt1 = (a.N1 + 255) / 256, nt2 = (a.N2 + 255) / 256;
    // (split, tile) pairs in split-major order, dealt to the XCDs in contiguous chunks (flat 1-D grid, block L lands on XCD
    // L % 8): the ~32 workgroups an XCD runs at a time then belong to ONE split -- the same rows of A and B -- and cover a
    // compact block of output tiles, so every 64-row slice of an operand panel is fetched into that L2 once and hit by the
    // other tiles of its row / column.  (With the split on gridDim.z an XCD held 3 tiles of each of 10 splits: a third of the
    // reuse, 3.5x the algorithmic bytes on the fabric side of L2.)
    const int ntile = nt1 * nt2;
    int split, t1, t2;
    {
        const int nwg = (int)gridDim.x, L = (int)blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = L & 7, loc = L >> 3;
        const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
        split = id / ntile;
        const int tid_ = id - split * ntile;
        const int GM = 8, per_group = GM * nt2;
        const int group = tid_ / per_group, rem = tid_ - group * per_group;
        const int first = group * GM;
        const int gsize = (nt1 - first) < GM ? (nt1 - first) : GM;
        t1 = first + rem % gsize;
        t2 = rem / gsize;
    }
    const int n1_0 = t1 * 256, n2_0 = t2 * 256;
    const int kt0 = split * tiles_per_split;
    int kt1 = kt0 + tiles_per_split; kt1 = kt1 < total_tiles ? kt1 : total_tiles;
    if (kt0 >= kt1) return;
    const bool to_ws = (int)gridDim.x > ntile;
    tn256_unit(a, smem, tiles_per_batch, n1_0, n2_0, kt0, kt1,
               to_ws ? reinterpret_cast<float*>(a.ws) + (int64_t)split * a.N1 * a.N2 : nullptr, 0, 0, a.N2);
}

// ------------------------------------------------------------------------------------------------ TN, grouped ("stream-K" over a layer)
// The four weight gradients of an encoder layer (q/k/v fused, out-proj, fc1, fc2: 75 + 25 + 100 + 100 output tiles of 256 x 256
// at large-v3-turbo dimensions, each contracted over the same M = B T rows) as ONE persistent launch.  Alone, each of them has
// fewer tiles than the chip has CUs and needs a 4...10-way split of the contraction to fill it: 400 MB of fp32 partials per
// layer written, re-read and added by six reduce launches (2.4 % of the step, round 2).  Pooled, the 300 tiles cover the 256
// CUs once with WHOLE contractions -- those tiles accumulate straight into the gradient, no partials at all -- and only the
// remaining T mod G tiles are split, s = floor(G / rem) ways, so that the last round is as full as the first: the work per
// CU is balanced like a stream-K schedule, but every workgroup of a round runs the same contraction range at the same time
// (operand panels are shared through the XCD's L2; a free-running stream-K walk offsets every CU's k position and would
// stream each operand once per TILE: ~7 GB per layer).  Partials: rem x s tiles of 256 KB (<= 64 MB), added to the
// gradients in split order by ONE fix-up launch (tn_group_fixup_kernel) -- deterministic, no atomics, no flags.
#define TN_GROUP_MAX DICOW_TN_GROUP_MAX
struct tn_group_plan_t {
    int n, G, T, R, rem, s, chunk, kiters;          // problems, workgroups, tiles, full rounds, remainder tiles, splits, tiles per split
    int tile0[TN_GROUP_MAX + 1];                    // first pooled tile id of problem p
    int nt1[TN_GROUP_MAX], nt2[TN_GROUP_MAX];
};
struct tn_group_kargs_t { dicow_gemm_tn_args p[TN_GROUP_MAX]; tn_group_plan_t plan; float* ws; };

// pooled tile id -> (problem, 256-row block t1, 256-column block t2); tiles of a problem in the grouped (8 row blocks) order
__device__ __forceinline__ void tn_group_tile(const tn_group_plan_t& pl, int id, int& p, int& t1, int& t2) {
    p = 0;
#pragma unroll
    for (int i = 1; i < TN_GROUP_MAX; ++i) if (i < pl.n && id >= pl.tile0[i]) p = i;
    const int tid_ = id - pl.tile0[p];
    const int nt1 = pl.nt1[p], nt2 = pl.nt2[p];
    const int GM = 8, per_group = GM * nt2;
    const int group = tid_ / per_group, rem = tid_ - group * per_group;
    const int first = group * GM;
    const int gsize = (nt1 - first) < GM ? (nt1 - first) : GM;
    t1 = first + rem % gsize;
    t2 = rem / gsize;
}

__global__ void __launch_bounds__(512, 2) gemm_tn256g_kernel(const tn_group_kargs_t g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const tn_group_plan_t& pl = g.plan;
    // workgroup L runs on XCD L % 8: give every XCD a contiguous chunk of each round's ids (adjacent tiles share panels)
    const int nwg = (int)gridDim.x, L = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = L & 7, loc = L >> 3;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    bool first = true;
    for (int rd = 0; rd <= pl.R; ++rd) {
        int id, kt0 = 0, kt1 = pl.kiters, split = -1;
        if (rd < pl.R) {
            id = rd * pl.G + w;
        } else {                                      // the split round: items split-major (one k range = one run of workgroups)
            if (pl.rem == 0 || w >= pl.rem * pl.s) break;
            split = w / pl.rem;
            id = pl.R * pl.G + (w - split * pl.rem);
            kt0 = split * pl.chunk;
            kt1 = kt0 + pl.chunk < pl.kiters ? kt0 + pl.chunk : pl.kiters;
        }
        int p, t1, t2;
        tn_group_tile(pl, id, p, t1, t2);
        if (!first) {                                 // the previous unit's trailing (empty) DMA and fragment reads are done
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        first = false;
        // (s == 1: the remainder tiles are whole contractions too and go straight into C)
        float* wpart = (split < 0 || pl.s == 1) ? nullptr : g.ws + ((int64_t)(id - pl.R * pl.G) * pl.s + split) * 65536;
        if (kt0 < kt1)
            tn256_unit(g.p[p], smem, pl.kiters, t1 * 256, t2 * 256, kt0, kt1, wpart, t1 * 256, t2 * 256, 256);
    }
}

#ifndef TN_W4
#define TN_W4 0               // 1: pooled weight gradients on gemm_tn256wg_kernel (experiments/gemm_tnw.inc: measured equal / slower)
#endif
#if TN_W4
#include "experiments/gemm_tnw.inc"       // the same pooled launch on four-wave workgroups (one wave per SIMD, 128 x 128 wave tiles)
#endif

// C tile (+)= sum_{split} partial[tile][split]  in split order; one workgroup = 4 rows of a 256 x 256 tile
__global__ void __launch_bounds__(256) tn_group_fixup_kernel(const tn_group_kargs_t g) {
    const tn_group_plan_t& pl = g.plan;
    const int lt = blockIdx.x >> 6, rb = blockIdx.x & 63;          // remainder tile, block of 4 rows
    int p, t1, t2;
    tn_group_tile(pl, pl.R * pl.G + lt, p, t1, t2);
    const dicow_gemm_tn_args& a = g.p[p];
    const int row = rb * 4 + (threadIdx.x >> 6), c4 = (threadIdx.x & 63) * 4;
    const int n1 = t1 * 256 + row, n2 = t2 * 256 + c4;
    if (n1 >= a.N1 || n2 >= a.N2) return;
    // (a split whose range is empty -- chunk * split >= kiters -- wrote nothing: skip it)
    const float* wp = g.ws + (int64_t)lt * pl.s * 65536 + row * 256 + c4;
    float* cp;
    if (a.seg_rows > 0 && n1 >= a.seg_rows) {
        const int sg = n1 / a.seg_rows;
        cp = a.C_seg[sg - 1] + (int64_t)(n1 - sg * a.seg_rows) * a.ldc + n2;
    } else {
        cp = a.C + (int64_t)n1 * a.ldc + n2;
    }
    float4 sacc = a.accumulate ? *reinterpret_cast<const float4*>(cp) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z = 0; z < pl.s; ++z) {
        if (z * pl.chunk >= pl.kiters) break;
        const float4 v = *reinterpret_cast<const float4*>(wp + (int64_t)z * 65536);
        sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
    }
    *reinterpret_cast<float4*>(cp) = sacc;
}

// C[r][:] (+)= sum_z ws[z][row0 + r][:]   for r < nrows   (ldc may exceed N2)
__global__ void tn_reduce_kernel(const float* __restrict__ ws, int splits, int64_t zstride, int row0, int nrows, int N2,
                                 float* __restrict__ C, int64_t ldc, int accumulate) {
    const int n24 = N2 >> 2;
    const int64_t total = (int64_t)nrows * n24;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / n24), c4 = (int)(i - (int64_t)r * n24);
        float* cp = C + (int64_t)r * ldc + c4 * 4;
        float4 s = accumulate ? *reinterpret_cast<const float4*>(cp) : make_float4(0, 0, 0, 0);
        const float* wp = ws + (int64_t)(row0 + r) * N2 + c4 * 4;
        for (int z = 0; z < splits; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(wp + (int64_t)z * zstride);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(cp) = s;
    }
}

static std::once_flag g_tn_once;
static int g_tn_ncu = 256;
// Tile size + contraction split: minimise  flops / (rate * grid-quantisation efficiency) + split-reduction traffic.
static void tn_plan(const dicow_gemm_tn_args* a, int& tpb, int& total, int& nt, int& splits, int& tps, int& tile) {
    const int batch = a->batch > 0 ? a->batch : 1;
    tpb = dicow_cdiv(a->Mk, TK);
    total = tpb * batch;
    const double flops = 2.0 * a->Mk * batch * (double)a->N1 * a->N2;
    const double cbytes = 4.0 * a->N1 * a->N2;
    double best = 1e30;
    tile = 128; splits = 1; nt = 1;
    for (int tl = 128; tl <= 256; tl += 128) {
        if (tl == 256 && (a->N1 < 256 || a->N2 < 256)) continue;
        // the 256 kernel addresses each batch's operands through 32-bit buffer offsets
        if (tl == 256 && ((int64_t)a->Mk * a->lda * 2 >= (1ll << 32) || (int64_t)a->Mk * a->ldb * 2 >= (1ll << 32))) continue;
        const int n = dicow_cdiv(a->N1, tl) * dicow_cdiv(a->N2, tl);
        const int slots = tl == 256 ? 256 : 512;               // resident workgroups on the chip
        const double rate = tl == 256 ? 0.85e15 : 0.69e15;
        for (int sp = 1; sp <= 16 && sp <= (total / 8 > 1 ? total / 8 : 1); ++sp) {
            const int blocks = n * sp;
            const double eff = (double)blocks / (slots * ((blocks + slots - 1) / slots));
            const double tsec = flops / (rate * eff) + (sp > 1 ? (sp + 2) * cbytes / 4.0e12 + 4e-6 : 0.0);
            if (tsec < best) { best = tsec; tile = tl; splits = sp; nt = n; }
        }
    }
#ifdef DICOW_ABLATIONS
    if (const char* ev = getenv("DICOW_TN_SPLITS")) splits = atoi(ev);        // tuning knobs of diagnostic builds (tools/bench_gemm.py)
    if (const char* ev = getenv("DICOW_TN_TILE")) { tile = atoi(ev); nt = dicow_cdiv(a->N1, tile) * dicow_cdiv(a->N2, tile); }
#endif
    if (splits < 1) splits = 1;
    tps = dicow_cdiv(total, splits);
    splits = dicow_cdiv(total, tps);
}

extern "C" int64_t dicow_gemm_tn_ws_bytes(const dicow_gemm_tn_args* a) {
    int tpb, total, nt, splits, tps, tile;
    tn_plan(a, tpb, total, nt, splits, tps, tile);
    return splits > 1 ? (int64_t)splits * a->N1 * a->N2 * 4 : 0;
}

extern "C" int dicow_gemm_tn(const dicow_gemm_tn_args* a, void* stream) {
    DICOW_REQUIRE(a && a->A && a->B && a->C, "gemm_tn: null operand");
    DICOW_REQUIRE(a->Mk > 0 && a->N1 >= 8 && a->N2 >= 8, "gemm_tn: empty problem");
    DICOW_REQUIRE(a->N1 % 8 == 0 && a->N2 % 8 == 0, "gemm_tn: N1=%d, N2=%d must be multiples of 8", a->N1, a->N2);
    DICOW_REQUIRE(a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 4 == 0, "gemm_tn: lda/ldb %% 8, ldc %% 4 required");
    DICOW_REQUIRE(a->seg_rows == 0 || (a->seg_rows % 128 == 0 && a->N1 <= 3 * a->seg_rows && a->C_seg[0] &&
                                        (a->N1 <= 2 * a->seg_rows || a->C_seg[1])), "gemm_tn: bad C segments");
    int tpb, total, nt, splits, tps, tile;
    tn_plan(a, tpb, total, nt, splits, tps, tile);
    DICOW_REQUIRE(splits == 1 || (a->ws && a->ws_bytes >= (int64_t)splits * a->N1 * a->N2 * 4),
                  "gemm_tn: workspace too small (need %ld bytes)", (long)splits * a->N1 * a->N2 * 4);
    static const bool attr_set = [] {       // (a function-local static initialiser runs once, under the runtime's lock)
        (void)hipFuncSetAttribute((const void*)gemm_tn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_tn256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TN256_LDS);
        return true;
    }();
    (void)attr_set;
    if (tile == 256)
        hipLaunchKernelGGL(gemm_tn256_kernel, dim3(nt * splits), dim3(512), TN256_LDS, (hipStream_t)stream, *a, tpb, total, tps);
    else
        hipLaunchKernelGGL(gemm_tn_kernel, dim3(nt, 1, splits), dim3(256), TN_LDS_BYTES, (hipStream_t)stream, *a, tpb, total, tps);
    disp_note(tile == 256 ? "gemm_tn256_kernel" : "gemm_tn_kernel");
    DICOW_CHECK_LAUNCH("gemm_tn");
    if (splits > 1) {
        const int nseg = a->seg_rows > 0 ? dicow_cdiv(a->N1, a->seg_rows) : 1;
        for (int sg = 0; sg < nseg; ++sg) {
            const int row0 = sg * (a->seg_rows > 0 ? a->seg_rows : 0);
            const int nrows = a->seg_rows > 0 ? ((a->N1 - row0) < a->seg_rows ? (a->N1 - row0) : a->seg_rows) : a->N1;
            float* C = sg == 0 ? a->C : a->C_seg[sg - 1];
            const int64_t tot4 = (int64_t)nrows * (a->N2 / 4);
            int grid = (int)((tot4 + 255) / 256); if (grid > 4096) grid = 4096;
            hipLaunchKernelGGL(tn_reduce_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)a->ws, splits,
                               (int64_t)a->N1 * a->N2, row0, nrows, a->N2, C, a->ldc, a->accumulate);
            DICOW_CHECK_LAUNCH("tn_reduce");
        }
    }
    return DICOW_OK;
}

// ---- grouped launch (see gemm_tn256g_kernel).  Eligible: every problem has N1, N2 >= 256, batch == 1, the same Mk, 32-bit
// operand offsets; anything else runs problem by problem through dicow_gemm_tn (same results as separate calls).
static bool tn_group_plan(const dicow_gemm_tn_group_args* ga, tn_group_plan_t& pl) {
    if (ga->n < 2 || ga->n > TN_GROUP_MAX) return false;
    const int Mk = ga->p[0].Mk;
    int T = 0;
    for (int i = 0; i < ga->n; ++i) {
        const dicow_gemm_tn_args& a = ga->p[i];
        if (a.Mk != Mk || (a.batch > 1) || a.N1 < 256 || a.N2 < 256) return false;
        if ((int64_t)a.Mk * a.lda * 2 >= (1ll << 32) || (int64_t)a.Mk * a.ldb * 2 >= (1ll << 32)) return false;
        pl.tile0[i] = T;
        pl.nt1[i] = dicow_cdiv(a.N1, 256); pl.nt2[i] = dicow_cdiv(a.N2, 256);
        T += pl.nt1[i] * pl.nt2[i];
    }
    for (int i = ga->n; i <= TN_GROUP_MAX; ++i) pl.tile0[i] = T;
    for (int i = ga->n; i < TN_GROUP_MAX; ++i) { pl.nt1[i] = pl.nt2[i] = 1; }
    std::call_once(g_tn_once, [] { int dev = 0; hipDeviceProp_t pr; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) g_tn_ncu = pr.multiProcessorCount; });
    const int lim = g_gemm_cus.load();
    const int G = (lim > 0 && lim < g_tn_ncu) ? lim : g_tn_ncu;
    pl.n = ga->n; pl.G = G; pl.T = T; pl.kiters = dicow_cdiv(Mk, TK);
    if (4 * T < 3 * G) return false;                // far fewer pooled tiles than CUs: the per-problem split-K plans do better
                                                    // (from 3/4 G on, one whole contraction per workgroup still beats them)
    pl.R = T / G; pl.rem = T - pl.R * G;
    pl.s = pl.rem > 0 ? G / pl.rem : 1;
    if (pl.s > pl.kiters) pl.s = pl.kiters;
    if (pl.s > 64) pl.s = 64;
    pl.chunk = dicow_cdiv(pl.kiters, pl.s);
    return true;
}

extern "C" int64_t dicow_gemm_tn_group_ws_bytes(const dicow_gemm_tn_group_args* ga) {
    if (!ga) return 0;
    tn_group_plan_t pl;
    int64_t need = 0;
    if (tn_group_plan(ga, pl) && pl.s > 1) need = (int64_t)pl.rem * pl.s * 65536 * 4;
    for (int i = 0; i < ga->n && i < TN_GROUP_MAX; ++i) {          // (the fall-back path's needs, so that one query covers both)
        const int64_t w = dicow_gemm_tn_ws_bytes(&ga->p[i]);
        need = w > need ? w : need;
    }
    return need;
}

extern "C" int dicow_gemm_tn_group(const dicow_gemm_tn_group_args* ga, void* stream) {
    DICOW_REQUIRE(ga && ga->n >= 1 && ga->n <= TN_GROUP_MAX, "gemm_tn_group: 1..%d problems", TN_GROUP_MAX);
    tn_group_plan_t pl;
    bool ok = true;
    for (int i = 0; i < ga->n; ++i) {
        const dicow_gemm_tn_args* a = &ga->p[i];
        DICOW_REQUIRE(a->A && a->B && a->C, "gemm_tn_group: null operand in problem %d", i);
        DICOW_REQUIRE(a->Mk > 0 && a->N1 >= 8 && a->N2 >= 8 && a->N1 % 8 == 0 && a->N2 % 8 == 0, "gemm_tn_group: bad shape in problem %d", i);
        DICOW_REQUIRE(a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 4 == 0, "gemm_tn_group: lda/ldb %% 8, ldc %% 4 required");
        DICOW_REQUIRE(a->seg_rows == 0 || (a->seg_rows % 128 == 0 && a->N1 <= 3 * a->seg_rows && a->C_seg[0] &&
                                            (a->N1 <= 2 * a->seg_rows || a->C_seg[1])), "gemm_tn_group: bad C segments");
    }
    ok = tn_group_plan(ga, pl);
    if (!ok) {                                      // not poolable: problem by problem
        for (int i = 0; i < ga->n; ++i) {
            dicow_gemm_tn_args a = ga->p[i];
            a.ws = ga->ws; a.ws_bytes = ga->ws_bytes;
            const int rc = dicow_gemm_tn(&a, stream);
            if (rc != DICOW_OK) return rc;
        }
        return DICOW_OK;
    }
    const int64_t need = pl.s > 1 ? (int64_t)pl.rem * pl.s * 65536 * 4 : 0;
    DICOW_REQUIRE(need == 0 || (ga->ws && ga->ws_bytes >= need), "gemm_tn_group: workspace too small (need %ld bytes)", (long)need);
    static const bool attr_set = [] {
        (void)hipFuncSetAttribute((const void*)gemm_tn256g_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TN256_LDS);
#if TN_W4
        (void)hipFuncSetAttribute((const void*)gemm_tn256wg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TN256_LDS);
#endif
        return true;
    }();
    (void)attr_set;
    tn_group_kargs_t k;
    memset(&k, 0, sizeof(k));
    for (int i = 0; i < ga->n; ++i) k.p[i] = ga->p[i];
    k.plan = pl; k.ws = reinterpret_cast<float*>(ga->ws);
#if TN_W4
    hipLaunchKernelGGL(gemm_tn256wg_kernel, dim3(pl.G), dim3(256), TN256_LDS, (hipStream_t)stream, k);
    disp_note("gemm_tn256wg_kernel");
#else
    hipLaunchKernelGGL(gemm_tn256g_kernel, dim3(pl.G), dim3(512), TN256_LDS, (hipStream_t)stream, k);
    disp_note("gemm_tn256g_kernel");
#endif
    DICOW_CHECK_LAUNCH("gemm_tn_group");
    if (pl.rem > 0 && pl.s > 1) {
        hipLaunchKernelGGL(tn_group_fixup_kernel, dim3(pl.rem * 64), dim3(256), 0, (hipStream_t)stream, k);
        DICOW_CHECK_LAUNCH("tn_group_fixup");
    }
    return DICOW_OK;
}

// dicow_lora_down / dicow_lora_up / dicow_lora_wgrad: the low-rank side of a LoRA-adapted Linear (include/dicow_hip.h).
//
// All three are skinny products: one dimension is the stacked rank R <= 192, so the 128..256-wide MFMA tiles of gemm.hip would
// spend a tile's work on 16 columns.  Here v_mfma_f32_16x16x32_bf16 runs with the SMALL operand as A and the large one as B, as in
// gemm_nt_skinny_kernel: a lane then holds 4 consecutive elements of the narrow dimension for one row of the wide operand.  The
// large operand is read once; the small one (<= 192 x 5120 bf16) comes out of L2 / L1.
//   down : 16 rows per workgroup, the four waves split the k-steps (interleaved) and meet in LDS in wave order.
//   up   : a wave keeps the U fragments of its 64-column strip in registers and walks 64 rows; the MFMA rows are permuted so that
//          a lane ends with 16 CONSECUTIVE columns of one row (two 16-byte bf16 stores, four fp32 ones; a row's 64 columns are one
//          128-byte line).
//   wgrad: the contraction runs over rows, so both operands are gathered element-wise (2-byte loads; the four 32-byte pieces of a
//          load instruction are the rows of one 8-row group, and the neighbouring strip's loads hit the same lines in L1).  Row
//          blocks write fp32 partials to the workspace, a second launch adds them in block order: no atomics.
#include "common.h"

#define LORA_THREADS 256
#define LORA_ZERO8 bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}

// ------------------------------------------------------------------------------------------------ down
template <int NT>
__global__ __launch_bounds__(LORA_THREADS) void lora_down_kernel(dicow_lora_down_args a) {
    __shared__ float red[3][NT][64][4];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, h = lane >> 4;
    const int m = blockIdx.x * 16 + i;
    const bool mvalid = m < a.M;
    const bool block = (a.flags & DICOW_LORA_BLOCK) != 0;
    const int rs = block ? a.r : a.R;                    // rows of V per column segment of X
    const int nseg = block ? a.R / a.r : 1;
    const unsigned short* X = (const unsigned short*)a.X + (int64_t)(mvalid ? m : a.M - 1) * a.ldx + 8 * h;
    const unsigned short* V = (const unsigned short*)a.V + 8 * h;
    f32x4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int sps = a.K / 32, total = nseg * sps;        // k-steps per segment / in all
    for (int ks = w; ks < total; ks += 4) {
        const int j = ks / sps, kk = (ks - j * sps) * 32;
        bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(X + (int64_t)j * a.K + kk);
        if (!mvalid) xf = LORA_ZERO8;
        const int c_lo = j * rs, c_hi = c_lo + rs;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (16 * t < c_hi && 16 * t + 16 > c_lo) {   // wave-uniform: only the tiles that touch segment j's rows of V
                const int c = 16 * t + i;
                bf16x8_t vf = LORA_ZERO8;
                if (c >= c_lo && c < c_hi) vf = *reinterpret_cast<const bf16x8_t*>(V + (int64_t)c * a.ldv + kk);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, xf, acc[t], 0, 0, 0);
            }
        }
    }
    if (w > 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[w - 1][t][lane][e] = acc[t][e];
    }
    __syncthreads();
    if (w > 0 || !mvalid) return;
    unsigned short* T = (unsigned short*)a.T + (int64_t)m * a.ldt;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = 16 * t + 4 * h;                    // R % 4 == 0: a quad is inside or outside
        if (c >= a.R) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ((acc[t][e] + red[0][t][lane][e]) + red[1][t][lane][e]) + red[2][t][lane][e];
        *reinterpret_cast<uint2*>(T + c) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

static bool lora_rank_ok(int r, int R) {
    return (r == 8 || r == 16 || r == 32 || r == 64) && R >= r && R % r == 0 && R <= DICOW_LORA_MAX_R;
}
#define LORA_REQUIRE_RANK(name, r, R) \
    DICOW_REQUIRE(lora_rank_ok(r, R), name ": rank r = %d must be 8, 16, 32 or 64 and the stacked R = %d a multiple of it, at most %d", r, R, DICOW_LORA_MAX_R)

extern "C" int dicow_lora_down(const dicow_lora_down_args* a, void* stream) {
    DICOW_REQUIRE(a && a->X && a->V && a->T, "lora_down: null operand");
    LORA_REQUIRE_RANK("lora_down", a->r, a->R);
    DICOW_REQUIRE(a->M >= 1 && a->K >= 32 && a->K % 32 == 0, "lora_down: M %d < 1 or K %d not a positive multiple of 32", a->M, a->K);
    DICOW_REQUIRE((a->flags & ~DICOW_LORA_BLOCK) == 0, "lora_down: unknown flags %d", a->flags);
    const int nseg = (a->flags & DICOW_LORA_BLOCK) ? a->R / a->r : 1;
    DICOW_REQUIRE(a->ldx % 8 == 0 && a->ldv % 8 == 0 && a->ldt % 4 == 0, "lora_down: ldx / ldv must be multiples of 8 elements, ldt of 4 "
                  "(%lld, %lld, %lld)", (long long)a->ldx, (long long)a->ldv, (long long)a->ldt);
    DICOW_REQUIRE(a->ldx >= (int64_t)nseg * a->K && a->ldv >= a->K && a->ldt >= a->R, "lora_down: a leading dimension is shorter than its row");
    DICOW_REQUIRE(((uintptr_t)a->X | (uintptr_t)a->V) % 16 == 0 && (uintptr_t)a->T % 8 == 0, "lora_down: X / V must be 16-byte aligned, T 8-byte");
    const unsigned grid = (unsigned)dicow_cdiv(a->M, 16);
    hipStream_t st = (hipStream_t)stream;
    const int nt = dicow_cdiv(a->R, 16);
#define LORA_DOWN(NT) hipLaunchKernelGGL((lora_down_kernel<NT>), dim3(grid), dim3(LORA_THREADS), 0, st, *a)
    if (nt <= 1) LORA_DOWN(1);
    else if (nt <= 2) LORA_DOWN(2);
    else if (nt <= 3) LORA_DOWN(3);
    else if (nt <= 4) LORA_DOWN(4);
    else if (nt <= 6) LORA_DOWN(6);
    else if (nt <= 8) LORA_DOWN(8);
    else LORA_DOWN(12);
#undef LORA_DOWN
    DICOW_CHECK_LAUNCH("lora_down");
    return DICOW_OK;
}

// ------------------------------------------------------------------------------------------------ up
#define LORA_UP_ROWS 64                                  // rows per wave (4 MFMA row blocks); a workgroup covers 256 rows of one strip
template <int KS, bool F32, int EPI>                    // EPI: 0 plain, 1 GELU (+ gelu' to aux), 2 multiply by aux
__global__ __launch_bounds__(LORA_THREADS) void lora_up_kernel(dicow_lora_up_args a) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, h = lane >> 4;
    const bool block = (a.flags & DICOW_LORA_BLOCK) != 0;
    const int sps = (a.N + 63) / 64;                     // strips per segment
    const int strip = blockIdx.x;
    const int j = block ? strip / sps : 0;
    const int nl0 = (strip - j * sps) * 64;              // first column of the strip inside its segment
    const int rc = block ? a.r : a.R;                    // contraction length
    const int tc0 = block ? j * a.r : 0;                 // first column of T / row of U
    const float scale = a.seg_scale[j];
    constexpr bool GELU = EPI == 1, MUL = EPI == 2;
    const int mw0 = (blockIdx.y * 4 + w) * LORA_UP_ROWS;
    if (mw0 >= a.M) return;                              // (no barrier below)

    // A operand: row i of tile q is column nl0 + 16 (i >> 2) + 4 q + (i & 3), so that result register e of tile q in lane half-row h
    // is column nl0 + 16 h + 4 q + e
    const unsigned short* U = (const unsigned short*)a.U + (int64_t)tc0 * a.ldu;
    bf16x8_t uf[KS][4];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = nl0 + 16 * (i >> 2) + 4 * q + (i & 3);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 32 * s + 8 * h + e;
                uf[s][q][e] = (k < rc && n < a.N) ? (short)U[(int64_t)k * a.ldu + n] : (short)0;
            }
        }
    const int nc = nl0 + 16 * h;                         // this lane's 16 columns inside the segment
    const bool nvalid = nc < a.N;                        // N % 16 == 0: all 16 or none
    const int64_t col = (int64_t)j * a.N + nc;           // ... inside P / Y
    for (int rb = 0; rb < LORA_UP_ROWS / 16; ++rb) {
        const int mb = mw0 + 16 * rb;
        if (mb >= a.M) break;
        const int m = mb + i;
        const bool mvalid = m < a.M;
        const unsigned short* T = (const unsigned short*)a.T + (int64_t)(mvalid ? m : a.M - 1) * a.ldt + tc0 + 8 * h;
        f32x4_t acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bf16x8_t tf = LORA_ZERO8;
            if (32 * s + 8 * h < rc) tf = *reinterpret_cast<const bf16x8_t*>(T + 32 * s);    // rc % 8 == 0: a chunk is inside or outside
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(uf[s][q], tf, acc[q], 0, 0, 0);
        }
        if (!mvalid || !nvalid) continue;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * q + e] = bf2f(f2bf(bf2f(f2bf(acc[q][e])) * scale));
        if (F32) {
            const float* P = (const float*)a.P + (int64_t)m * a.ldp + col;
            float* Y = (float*)a.Y + (int64_t)m * a.ldy + col;
            float4 p[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) p[q] = *reinterpret_cast<const float4*>(P + 4 * q);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(Y + 4 * q) = make_float4(p[q].x + v[4 * q], p[q].y + v[4 * q + 1], p[q].z + v[4 * q + 2], p[q].w + v[4 * q + 3]);
        } else {
            float g[16], dg[16];
            if (MUL) {                                   // P is the base dgrad's fp32 accumulator: ONE rounding, after the multiply, as DICOW_EPI_MUL_AUX
                const float* P = (const float*)a.P + (int64_t)m * a.ldp + col;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 p = *reinterpret_cast<const float4*>(P + 4 * q);
                    g[4 * q] = p.x + v[4 * q]; g[4 * q + 1] = p.y + v[4 * q + 1]; g[4 * q + 2] = p.z + v[4 * q + 2]; g[4 * q + 3] = p.w + v[4 * q + 3];
                }
            } else {
                const unsigned short* P = (const unsigned short*)a.P + (int64_t)m * a.ldp + col;
                const uint4 p0 = *reinterpret_cast<const uint4*>(P), p1 = *reinterpret_cast<const uint4*>(P + 8);
                const unsigned pw[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    g[2 * u] = __uint_as_float(pw[u] << 16) + v[2 * u];
                    g[2 * u + 1] = __uint_as_float(pw[u] & 0xffff0000u) + v[2 * u + 1];
                }
            }
            if (MUL) {                                   // fc2's dgrad with an adapter: the saved gelu' multiplies the COMPLETE d_a
                const unsigned short* X = (const unsigned short*)a.aux + (int64_t)m * a.ldaux + col;
                const uint4 x0 = *reinterpret_cast<const uint4*>(X), x1 = *reinterpret_cast<const uint4*>(X + 8);
                const unsigned xw[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    g[2 * u] *= __uint_as_float(xw[u] << 16);
                    g[2 * u + 1] *= __uint_as_float(xw[u] & 0xffff0000u);
                }
            }
            if (GELU) {                                  // the activation and its derivative at the bf16-rounded sum, as nt_epilogue_math
#pragma unroll
                for (int e = 0; e < 16; ++e) gelu_erf_both(bf2f(f2bf(g[e])), g[e], dg[e]);
            }
            unsigned short* Y = (unsigned short*)a.Y + (int64_t)m * a.ldy + col;
            *reinterpret_cast<uint4*>(Y) = make_uint4(pack_bf16x2(g[0], g[1]), pack_bf16x2(g[2], g[3]), pack_bf16x2(g[4], g[5]), pack_bf16x2(g[6], g[7]));
            *reinterpret_cast<uint4*>(Y + 8) = make_uint4(pack_bf16x2(g[8], g[9]), pack_bf16x2(g[10], g[11]), pack_bf16x2(g[12], g[13]), pack_bf16x2(g[14], g[15]));
            if (GELU && a.aux) {
                unsigned short* X = (unsigned short*)a.aux + (int64_t)m * a.ldaux + col;
                *reinterpret_cast<uint4*>(X) = make_uint4(pack_bf16x2(dg[0], dg[1]), pack_bf16x2(dg[2], dg[3]), pack_bf16x2(dg[4], dg[5]), pack_bf16x2(dg[6], dg[7]));
                *reinterpret_cast<uint4*>(X + 8) = make_uint4(pack_bf16x2(dg[8], dg[9]), pack_bf16x2(dg[10], dg[11]), pack_bf16x2(dg[12], dg[13]), pack_bf16x2(dg[14], dg[15]));
            }
        }
    }
}

template <int KS>
static void lora_up_launch(const dicow_lora_up_args& a, dim3 grid, hipStream_t st) {
    if (a.flags & DICOW_LORA_OUT_F32) hipLaunchKernelGGL((lora_up_kernel<KS, true, 0>), grid, dim3(LORA_THREADS), 0, st, a);
    else if (a.flags & DICOW_LORA_GELU) hipLaunchKernelGGL((lora_up_kernel<KS, false, 1>), grid, dim3(LORA_THREADS), 0, st, a);
    else if (a.flags & DICOW_LORA_MUL_AUX) hipLaunchKernelGGL((lora_up_kernel<KS, false, 2>), grid, dim3(LORA_THREADS), 0, st, a);
    else hipLaunchKernelGGL((lora_up_kernel<KS, false, 0>), grid, dim3(LORA_THREADS), 0, st, a);
}

extern "C" int dicow_lora_up(const dicow_lora_up_args* a, void* stream) {
    DICOW_REQUIRE(a && a->T && a->U && a->P && a->Y, "lora_up: null operand");
    LORA_REQUIRE_RANK("lora_up", a->r, a->R);
    DICOW_REQUIRE((a->flags & ~(DICOW_LORA_BLOCK | DICOW_LORA_OUT_F32 | DICOW_LORA_GELU | DICOW_LORA_MUL_AUX)) == 0, "lora_up: unknown flags %d", a->flags);
    const bool block = (a->flags & DICOW_LORA_BLOCK) != 0, f32 = (a->flags & DICOW_LORA_OUT_F32) != 0;
    const int epi = a->flags & (DICOW_LORA_GELU | DICOW_LORA_MUL_AUX);
    DICOW_REQUIRE(!(f32 && epi), "lora_up: the GELU / MUL_AUX epilogues need a bf16 output");
    DICOW_REQUIRE(epi != (DICOW_LORA_GELU | DICOW_LORA_MUL_AUX), "lora_up: GELU and MUL_AUX exclude each other");
    DICOW_REQUIRE(!(epi & DICOW_LORA_MUL_AUX) || (a->aux && a->P != a->Y), "lora_up: MUL_AUX needs aux and an fp32 P apart from the bf16 Y");
    DICOW_REQUIRE(a->M >= 1 && a->N >= 16 && a->N % (block ? 64 : 16) == 0, "lora_up: M %d < 1 or N %d not a positive multiple of %d", a->M,
                  a->N, block ? 64 : 16);
    const int nseg = block ? a->R / a->r : 1;
    const int64_t cols = (int64_t)nseg * a->N;
    DICOW_REQUIRE(a->ldt % 8 == 0 && a->ldp % 8 == 0 && a->ldy % 8 == 0 && (!a->aux || a->ldaux % 8 == 0),
                  "lora_up: ldt / ldp / ldy / ldaux must be multiples of 8 elements");
    DICOW_REQUIRE(a->ldt >= a->R && a->ldu >= a->N && a->ldp >= cols && a->ldy >= cols && (!a->aux || a->ldaux >= cols),
                  "lora_up: a leading dimension is shorter than its row");
    DICOW_REQUIRE(((uintptr_t)a->T | (uintptr_t)a->P | (uintptr_t)a->Y | (uintptr_t)a->aux) % 16 == 0, "lora_up: T / P / Y / aux must be 16-byte aligned");
    DICOW_REQUIRE(a->P != a->Y || a->ldp == a->ldy, "lora_up: in place (P == Y) needs ldp == ldy");
    const int64_t strips = (int64_t)nseg * dicow_cdiv(a->N, 64);
    const dim3 grid((unsigned)strips, (unsigned)dicow_cdiv(a->M, 4 * LORA_UP_ROWS));
    DICOW_REQUIRE(grid.y <= 65535u, "lora_up: M %d too large for one grid", a->M);
    hipStream_t st = (hipStream_t)stream;
    switch (dicow_cdiv(block ? a->r : a->R, 32)) {
        case 1: lora_up_launch<1>(*a, grid, st); break;
        case 2: lora_up_launch<2>(*a, grid, st); break;
        case 3: lora_up_launch<3>(*a, grid, st); break;
        case 4: lora_up_launch<4>(*a, grid, st); break;
        case 5: lora_up_launch<5>(*a, grid, st); break;
        default: lora_up_launch<6>(*a, grid, st); break;
    }
    DICOW_CHECK_LAUNCH("lora_up");
    return DICOW_OK;
}

// ------------------------------------------------------------------------------------------------ wgrad
#define LORA_WG_SPLIT_ROWS 256                           // at least this many rows per partial
#define LORA_WG_MAX_SPLITS 32
static void lora_wgrad_plan(int M, int* nsplit, int* rps) {
    int ns = dicow_cdiv(M, LORA_WG_SPLIT_ROWS);
    if (ns > LORA_WG_MAX_SPLITS) ns = LORA_WG_MAX_SPLITS;
    if (ns < 1) ns = 1;
    const int per = dicow_cdiv(dicow_cdiv(M, ns), 32) * 32;
    *nsplit = dicow_cdiv(M, per);
    *rps = per;
}

// partial [split][rt][ntot] fp32: rt = rows of T^T a strip works with (dense R, block r), ntot = all columns of P
template <int NRT>
__global__ __launch_bounds__(LORA_THREADS) void lora_wgrad_kernel(dicow_lora_wgrad_args a, int rps, int ntot) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, h = lane >> 4;
    const bool block = (a.flags & DICOW_LORA_BLOCK) != 0;
    const int sps = a.N / 32;                            // 32-column strips per segment
    const int strip = blockIdx.x * 4 + w;
    if (strip >= ntot / 32) return;                      // (no barrier below)
    const int j = block ? strip / sps : 0;
    const int rt = block ? a.r : a.R;
    const int tc0 = block ? j * a.r : 0;
    const int pc0 = strip * 32;                          // first column of the strip in P (segments are adjacent: j N + local)
    const int mlo = blockIdx.y * rps, mhi = min(a.M, mlo + rps);
    const unsigned short* P = (const unsigned short*)a.P + pc0 + i;
    const unsigned short* T = (const unsigned short*)a.T + tc0 + i;
    f32x4_t acc[NRT][2];
#pragma unroll
    for (int t = 0; t < NRT; ++t) { acc[t][0] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    for (int m0 = mlo; m0 < mhi; m0 += 32) {
        bf16x8_t pf[2], tf[NRT];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int m = m0 + 8 * h + e;
            const bool ok = m < mhi;
            const int64_t mo = ok ? m : mlo;
            pf[0][e] = ok ? (short)P[mo * a.ldp] : (short)0;
            pf[1][e] = ok ? (short)P[mo * a.ldp + 16] : (short)0;
#pragma unroll
            for (int t = 0; t < NRT; ++t) tf[t][e] = (ok && 16 * t + i < rt) ? (short)T[mo * a.ldt + 16 * t] : (short)0;
        }
#pragma unroll
        for (int t = 0; t < NRT; ++t) {
            acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf[t], pf[0], acc[t][0], 0, 0, 0);
            acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf[t], pf[1], acc[t][1], 0, 0, 0);
        }
    }
    float* ws = (float*)a.ws + (int64_t)blockIdx.y * rt * ntot + pc0 + i;
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 16 * t + 4 * h + e;
            if (p < rt) { ws[(int64_t)p * ntot] = acc[t][0][e]; ws[(int64_t)p * ntot + 16] = acc[t][1][e]; }
        }
}

__global__ __launch_bounds__(LORA_THREADS) void lora_wgrad_reduce_kernel(dicow_lora_wgrad_args a, int nsplit, int rt, int ntot) {
    const int64_t idx = (int64_t)blockIdx.x * LORA_THREADS + threadIdx.x, n_all = (int64_t)rt * ntot;
    if (idx >= n_all) return;
    const float* ws = (const float*)a.ws + idx;
    float s = ws[0];
    for (int k = 1; k < nsplit; ++k) s += ws[k * n_all];             // block order: the same sum on every run
    s *= a.scale;
    const int p = (int)(idx / ntot), n = (int)(idx - (int64_t)p * ntot);
    int seg, pr, nc;
    if (a.flags & DICOW_LORA_BLOCK) { seg = n / a.N; nc = n - seg * a.N; pr = p; }
    else { seg = p / a.r; pr = p - seg * a.r; nc = n; }
    float* g = a.G[seg];
    if (!g) return;
    g += (int64_t)pr * a.g_rs + (int64_t)nc * a.g_cs;
    *g = a.accumulate ? *g + s : s;
}

static int lora_wgrad_check(int M, int N, int R, int r, int flags) {
    LORA_REQUIRE_RANK("lora_wgrad", r, R);
    DICOW_REQUIRE((flags & ~DICOW_LORA_BLOCK) == 0, "lora_wgrad: unknown flags %d", flags);
    DICOW_REQUIRE(M >= 1 && N >= 32 && N % 32 == 0, "lora_wgrad: M %d < 1 or N %d not a positive multiple of 32", M, N);
    return DICOW_OK;
}

extern "C" int64_t dicow_lora_wgrad_ws_bytes(int M, int N, int R, int r, int flags) {
    if (lora_wgrad_check(M, N, R, r, flags) != DICOW_OK) return 0;
    const bool block = (flags & DICOW_LORA_BLOCK) != 0;
    int nsplit, rps;
    lora_wgrad_plan(M, &nsplit, &rps);
    return (int64_t)nsplit * (block ? r : R) * ((int64_t)(block ? R / r : 1) * N) * 4;
}

extern "C" int dicow_lora_wgrad(const dicow_lora_wgrad_args* a, void* stream) {
    DICOW_REQUIRE(a && a->T && a->P, "lora_wgrad: null operand");
    if (int rc = lora_wgrad_check(a->M, a->N, a->R, a->r, a->flags)) return rc;
    const bool block = (a->flags & DICOW_LORA_BLOCK) != 0;
    const int nseg = a->R / a->r, rt = block ? a->r : a->R;
    const int64_t ntot64 = (int64_t)(block ? nseg : 1) * a->N;
    DICOW_REQUIRE(ntot64 <= 0x3fffffff, "lora_wgrad: too many columns");
    const int ntot = (int)ntot64;
    DICOW_REQUIRE(a->ldt >= a->R && a->ldp >= ntot, "lora_wgrad: a leading dimension is shorter than its row");
    const int64_t need = dicow_lora_wgrad_ws_bytes(a->M, a->N, a->R, a->r, a->flags);
    DICOW_REQUIRE(a->ws && a->ws_bytes >= need && (uintptr_t)a->ws % 4 == 0, "lora_wgrad: workspace of %lld bytes needed (dicow_lora_wgrad_ws_bytes), %lld given",
                  (long long)need, (long long)(a->ws ? a->ws_bytes : 0));
    int nsplit, rps;
    lora_wgrad_plan(a->M, &nsplit, &rps);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)dicow_cdiv(ntot / 32, 4), (unsigned)nsplit);
    const int nrt = dicow_cdiv(rt, 16);
#define LORA_WG(NRT) hipLaunchKernelGGL((lora_wgrad_kernel<NRT>), grid, dim3(LORA_THREADS), 0, st, *a, rps, ntot)
    if (nrt <= 1) LORA_WG(1);
    else if (nrt <= 2) LORA_WG(2);
    else if (nrt <= 3) LORA_WG(3);
    else if (nrt <= 4) LORA_WG(4);
    else if (nrt <= 6) LORA_WG(6);
    else if (nrt <= 8) LORA_WG(8);
    else LORA_WG(12);
#undef LORA_WG
    DICOW_CHECK_LAUNCH("lora_wgrad");
    const int64_t n_all = (int64_t)rt * ntot;
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)dicow_cdiv(n_all, LORA_THREADS)), dim3(LORA_THREADS), 0, st, *a, nsplit, rt, ntot);
    DICOW_CHECK_LAUNCH("lora_wgrad_reduce");
    return DICOW_OK;
}

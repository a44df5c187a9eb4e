// dicow_attn_decode: single-query-row attention of the decoder step with the K/V row chosen per query row (include/dicow_hip.h).
//
// One workgroup per (slot, head).  SHARED mode: the workgroup streams the K/V of its (window, head) from memory ONCE and uses
// every key for all `group` query rows of that window (the beams of a beam search share one copy of the cross-attention K/V).
// ANCESTRY mode: one query row per workgroup, the slot of every key position comes from the row's ancestry table (the
// self-attention cache of a beam search is never reordered; a row reads each position from the slot that wrote it).
//
// Layout: 512 threads = 64 key groups of 8 lanes.  The 8 lanes of a group split the 64 head dims into 16-byte chunks, so a key
// (or value) row is one contiguous 128-byte read per group and a wave fetches 8 rows per load instruction.  Every group runs an
// online softmax over the keys t = gi, gi + 64, ... (UK keys per trip, all their K and V loads issued before the first is used);
// the partial results (max, sum, accumulator) are merged across the 8 groups of a wave with lane shuffles, then across the 8 waves
// through LDS, both in a fixed order: two launches on the same input give the same bits.  Plain VALU arithmetic in fp32 -- the
// kernel is meant to be bound by streaming K/V once, not by math.
#include "common.h"

#define AD_THREADS 512
#define AD_WAVES (AD_THREADS / DICOW_WAVE)
#define AD_NG (AD_THREADS / 8)          // key groups per workgroup
#define AD_NEG -1.0e30f                 // "no key yet" maximum: finite, so that the rescale factors never see inf - inf
#define AD_LOG2E 1.4426950408889634f

// sum over the 8 lanes of a key group (quad swaps, then the half-row mirror joins the two quads); fp32 addition commutes, so all
// 8 lanes end with the same bits.  Needs every lane of the wave active.
__device__ __forceinline__ float ad_oct_sum(float v) {
    int x;
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false); v += __int_as_float(x);    // quad_perm [1,0,3,2]
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false); v += __int_as_float(x);    // quad_perm [2,3,0,1]
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false); v += __int_as_float(x);   // row_half_mirror
    return v;
}

__device__ __forceinline__ void ad_unpack8(const uint4& r, float (&f)[8]) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

template <int G, bool ANC>
__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(dicow_attn_decode_args a) {
    constexpr int UK = G > 6 ? 2 : 4;                    // keys per group and trip (register budget: q and the accumulators grow with G)
    __shared__ float s_m[AD_WAVES][G], s_l[AD_WAVES][G], s_acc[AD_WAVES][G][64];
    const int tid = threadIdx.x, c = tid & 7, gi = tid >> 3;
    const int h = (int)(blockIdx.x % (unsigned)a.H);
    const int s0 = (int)(blockIdx.x / (unsigned)a.H);    // shared: the slot; ancestry (G == 1): the query row
    const int64_t r0 = (int64_t)s0 * G;                  // first query row of this workgroup (< R: the host checked R == n_slots * G)
    const int Lk = a.Lk;

    float q[G][8];                                       // this lane's 8 head dims of every query row, times log2(e): base-2 scores
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint4 r = *reinterpret_cast<const uint4*>((const bf16_t*)a.q + (r0 + g) * a.q_rs + h * 64 + c * 8);
        ad_unpack8(r, q[g]);
#pragma unroll
        for (int j = 0; j < 8; ++j) q[g][j] *= AD_LOG2E;
    }
    float m[G], l[G], acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = AD_NEG; l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }
    const bf16_t* kb = (const bf16_t*)a.k + h * 64 + c * 8;
    const bf16_t* vb = (const bf16_t*)a.v + h * 64 + c * 8;
    const int32_t* anc = ANC ? a.anc + r0 * a.anc_rs : nullptr;

    for (int t0 = 0; t0 < Lk; t0 += AD_NG * UK) {        // trip count is uniform over the workgroup: no lane leaves early (DPP sums)
        uint4 kr[UK], vr[UK];
        bool ok[UK];
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int t = t0 + u * AD_NG + gi;
            ok[u] = t < Lk;
            const int tc = ok[u] ? t : Lk - 1;           // lanes past the end re-read the last key (in bounds) and drop its weight
            int64_t slot = s0;
            if (ANC) {                                   // a wrong table gives wrong numbers, never an address outside the n_slots caches
                const int s = anc[tc];
                slot = s < 0 ? 0 : (s >= a.n_slots ? a.n_slots - 1 : s);
            }
            kr[u] = *reinterpret_cast<const uint4*>(kb + slot * a.k_bs + (int64_t)tc * a.k_rs);
            vr[u] = *reinterpret_cast<const uint4*>(vb + slot * a.v_bs + (int64_t)tc * a.v_rs);
        }
        float p[G][UK];
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            float kf[8];
            ad_unpack8(kr[u], kf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float d = q[g][0] * kf[0];
#pragma unroll
                for (int j = 1; j < 8; ++j) d = fmaf(q[g][j], kf[j], d);
                d = ad_oct_sum(d);
                p[g][u] = ok[u] ? d : AD_NEG;
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float mx = m[g];
#pragma unroll
            for (int u = 0; u < UK; ++u) mx = fmaxf(mx, p[g][u]);
            const float alpha = __builtin_amdgcn_exp2f(m[g] - mx);
            m[g] = mx;
            float ps = 0.f;
#pragma unroll
            for (int u = 0; u < UK; ++u) {
                p[g][u] = ok[u] ? __builtin_amdgcn_exp2f(p[g][u] - mx) : 0.f;
                ps += p[g][u];
            }
            l[g] = fmaf(l[g], alpha, ps);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
        }
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            float vf[8];
            ad_unpack8(vr[u], vf);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[g][j] = fmaf(p[g][u], vf[j], acc[g][j]);
        }
    }

    // merge the 8 key groups of a wave (lane offsets 8, 16, 32); lanes 0..7 end with the wave's partial result
#pragma unroll
    for (int off = 8; off < DICOW_WAVE; off <<= 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float mo = __shfl_xor(m[g], off, DICOW_WAVE), lo = __shfl_xor(l[g], off, DICOW_WAVE);
            const float mx = fmaxf(m[g], mo);
            const float ea = __builtin_amdgcn_exp2f(m[g] - mx), eb = __builtin_amdgcn_exp2f(mo - mx);
            l[g] = l[g] * ea + lo * eb;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float ao = __shfl_xor(acc[g][j], off, DICOW_WAVE);
                acc[g][j] = acc[g][j] * ea + ao * eb;
            }
            m[g] = mx;
        }
    }
    const int w = tid >> 6;
    if ((tid & 63) < 8) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (c == 0) { s_m[w][g] = m[g]; s_l[w][g] = l[g]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) s_acc[w][g][c * 8 + j] = acc[g][j];
        }
    }
    __syncthreads();
    if (tid < G * 64) {                                  // merge the waves in wave order; Lk >= 1, so the sum is positive
        const int g = tid >> 6, d = tid & 63;
        float mx = s_m[0][g];
#pragma unroll
        for (int i = 1; i < AD_WAVES; ++i) mx = fmaxf(mx, s_m[i][g]);
        float ls = 0.f, os = 0.f;
#pragma unroll
        for (int i = 0; i < AD_WAVES; ++i) {
            const float e = __builtin_amdgcn_exp2f(s_m[i][g] - mx);
            ls = fmaf(s_l[i][g], e, ls);
            os = fmaf(s_acc[i][g][d], e, os);
        }
        ((bf16_t*)a.o)[(r0 + g) * a.o_rs + h * 64 + d] = f2bf(os / ls);
    }
}

template <int G>
static void ad_launch(const dicow_attn_decode_args& a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((attn_decode_kernel<G, false>), dim3(grid), dim3(AD_THREADS), 0, st, a);
}

extern "C" int dicow_attn_decode(const dicow_attn_decode_args* a, void* stream) {
    DICOW_REQUIRE(a && a->q && a->k && a->v && a->o, "attn_decode: null operand");
    DICOW_REQUIRE(a->group >= 1 && a->group <= DICOW_ATTN_DECODE_MAX_GROUP, "attn_decode: group %d outside 1..%d", a->group,
                  DICOW_ATTN_DECODE_MAX_GROUP);
    DICOW_REQUIRE(a->R >= 1 && a->H >= 1, "attn_decode: empty problem (R %d, H %d)", a->R, a->H);
    DICOW_REQUIRE(a->R % a->group == 0, "attn_decode: R %d is not a multiple of group %d", a->R, a->group);
    DICOW_REQUIRE(a->Lk >= 1, "attn_decode: Lk %d < 1", a->Lk);
    if (a->anc) {
        DICOW_REQUIRE(a->n_slots == a->R, "attn_decode: ancestry mode needs n_slots == R (%d != %d)", a->n_slots, a->R);
        DICOW_REQUIRE(a->anc_rs >= a->Lk, "attn_decode: anc_rs %lld < Lk %d", (long long)a->anc_rs, a->Lk);
    } else {
        DICOW_REQUIRE(a->n_slots == a->R / a->group, "attn_decode: shared mode needs n_slots == R / group (%d != %d)", a->n_slots,
                      a->R / a->group);
    }
    DICOW_REQUIRE(a->q_rs % 8 == 0 && a->k_rs % 8 == 0 && a->v_rs % 8 == 0 && a->k_bs % 8 == 0 && a->v_bs % 8 == 0,
                  "attn_decode: q/k/v strides must be multiples of 8 elements (16-byte loads)");
    DICOW_REQUIRE(((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v) % 16 == 0, "attn_decode: q/k/v must be 16-byte aligned");
    DICOW_REQUIRE(a->q_rs >= (int64_t)a->H * 64 && a->o_rs >= (int64_t)a->H * 64 && a->k_rs >= (int64_t)a->H * 64 &&
                  a->v_rs >= (int64_t)a->H * 64, "attn_decode: a row stride is shorter than H * 64");
    const int64_t wgs = (int64_t)(a->anc ? a->R : a->n_slots) * a->H;
    DICOW_REQUIRE(wgs <= 0x7fffffffLL, "attn_decode: too many (slot, head) pairs for one grid");
    const unsigned grid = (unsigned)wgs;
    hipStream_t st = (hipStream_t)stream;
    if (a->anc) hipLaunchKernelGGL((attn_decode_kernel<1, true>), dim3(grid), dim3(AD_THREADS), 0, st, *a);
    else switch (a->group) {
        case 1: ad_launch<1>(*a, grid, st); break;
        case 2: ad_launch<2>(*a, grid, st); break;
        case 3: ad_launch<3>(*a, grid, st); break;
        case 4: ad_launch<4>(*a, grid, st); break;
        case 5: ad_launch<5>(*a, grid, st); break;
        case 6: ad_launch<6>(*a, grid, st); break;
        case 7: ad_launch<7>(*a, grid, st); break;
        default: ad_launch<8>(*a, grid, st); break;
    }
    DICOW_CHECK_LAUNCH("attn_decode");
    return DICOW_OK;
}

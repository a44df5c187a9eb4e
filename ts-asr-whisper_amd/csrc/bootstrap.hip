// Bootstrap and randomisation sums: out[row, c] = the sum of column c of a table of integer counts over a random multiset of its rows
// (resample mode) or with the two halves of the columns exchanged in a random subset of the rows (swap mode), R replicates a launch.
// Behind it: bootstrap intervals of an error rate, the paired bootstrap of a difference and the approximate-randomisation test
// (significance.py).  include/dicow_hip.h states the definition in full; in short
//     w(r, p, t) = Philox4x32-10(counter = (p >> 2, r lo, r hi, t), key = seed)[p & 3],        r = first_replicate + row
//     resample   out[row, c] = sum_p table[lo_s + ((w * n_s) >> 32), c]        s the stratum of slot p
//     swap       out[row, c] = sum_p table[p, (c + (C / 2) * (w & 1)) mod C]
// A word depends on its coordinates alone and the sums are integers: every plan below, every grid and every split of the replicates
// into calls gives the same bits.  Plain int64 adds, no atomics, one writer per element, one replicate in one workgroup: no workspace.
//
// One Philox block serves four consecutive slots.  The C sums of a replicate live in registers (a static array of CT = the power of two
// at or above C; columns past C are wave-uniformly skipped), so the kernels are instantiated for CT in {1, 2, 4, 8, 16, 32}.
//   plan 1 LANE_LDS   a lane owns a replicate and walks all n slots; 256 replicates a workgroup share the table in LDS.  The lanes of a wave
//                     read rows at random: 8-byte reads that conflict as random addresses do (swap mode reads one row: a broadcast).  The sums
//                     leave through LDS so that the workgroup writes its 256 rows of `out` as one contiguous run.
//   plan 2 WAVE_LDS   a wave owns a replicate: lane l takes the Philox blocks l, l + 64, ..., then a DPP wave reduction per column (no LDS
//                     traffic) and lane c writes column c.  64 replicates a workgroup (16 a wave) share the staged table.
//   plan 3 WAVE_L2    the same, the rows read from global memory: a table past DICOW_BOOT_LDS_BYTES stays in L2 (640 KB at 20 000 x 4).
// Rows are read 16 bytes a load where C and the row pitch are even (in swap mode under plan 3 with 2 or 4 columns); the staging copies 16
// bytes a lane where the table is dense.  Which plan the library picks where: dicow_bootstrap_plan, measured in profiles/bootstrap.txt.
#include "host_table.h"
#include <algorithm>

#define BS_THREADS 256
#define BS_WAVE_LDS_RPB 64                           // replicates a workgroup, plan 2: the staging is paid once per 64 replicates
#define BS_WAVE_L2_RPB 4                             // plan 3: one replicate a wave, nothing to amortise
#define BS_LANE_MAX_N 128                            // plan 0, the table fits LDS: a lane a replicate up to this n, a wave a replicate above.
                                                     // Measured at R = 10^5 (profiles/bootstrap.txt), plan 1 against plan 2: 40 x 16 0.048 / 0.178 ms,
                                                     // 128 x 16 0.139 / 0.190, 256 x 16 0.274 / 0.258, 512 x 16 0.535 / 0.522, 512 x 4 0.106 / 0.095;
                                                     // 2048 x 4 goes the other way, 0.394 / 0.430

struct bs_args {
    const int64_t* table; const int64_t* offs; int64_t* out;
    int64_t ld, R;
    uint64_t r0;
    uint32_t k0, k1;
    int n, C, S, vec_stage;
};

__device__ __forceinline__ void bs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// KIND 0: resample, 8-byte reads; 1: resample, 16-byte reads (C even, rows 16-byte aligned); 2: swap, 8-byte reads at the exchanged column;
// 3: swap, C == CT a power of two and rows 16-byte aligned: the row is read as it lies, 16 bytes a load, and (c + C / 2) mod C = c ^ (C / 2)
// picks the exchanged column among registers (`off` is then 0 or C / 2 all the same)
template <int CT, int KIND>
__device__ __forceinline__ void bs_add_row(int64_t (&acc)[CT], const int64_t* row, const int C, const int off) {
    if constexpr (KIND == 1 && CT >= 2) {
#pragma unroll
        for (int c = 0; c < CT; c += 2)
            if (c < C) {
                const longlong2 v = *reinterpret_cast<const longlong2*>(row + c);
                acc[c] += v.x;
                acc[c + 1] += v.y;
            }
    } else if constexpr (KIND == 3 && CT >= 2) {
        int64_t v[CT];
#pragma unroll
        for (int c = 0; c < CT; c += 2) {
            const longlong2 x = *reinterpret_cast<const longlong2*>(row + c);
            v[c] = x.x;
            v[c + 1] = x.y;
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] += off ? v[c ^ (CT / 2)] : v[c];
    } else if constexpr (KIND >= 2) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) {
                int i = c + off;
                i -= i >= C ? C : 0;
                acc[c] += row[i];
            }
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) acc[c] += row[c];
    }
}

// the four slots of Philox block j of replicate (rlo, rhi), added to acc.  tab / ldt: the staged table or the caller's.
template <int CT, int KIND>
__device__ __forceinline__ void bs_block(int64_t (&acc)[CT], const bs_args& a, const int64_t* tab, const int64_t ldt, const uint32_t j,
                                         const uint32_t rlo, const uint32_t rhi) {
    uint32_t w[4];
    bs_philox(j, rlo, rhi, KIND >= 2 ? 1u : 0u, a.k0, a.k1, w);
    const int p0 = (int)(j << 2);
    int s = 0, lo = 0, end = a.n;
    if (KIND < 2 && a.S > 1) {                      // the stratum of slot p0: the last s with offs[s] <= p0
        int hi = a.S;
        while (hi - s > 1) {
            const int mid = (s + hi) >> 1;
            if ((int)a.offs[mid] <= p0) s = mid; else hi = mid;
        }
        lo = (int)a.offs[s];
        end = (int)a.offs[s + 1];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = p0 + q;
        if (p < a.n) {
            int u = p, off = 0;
            if constexpr (KIND >= 2) off = (w[q] & 1u) ? (a.C >> 1) : 0;
            else {
                while (p >= end && s + 1 < a.S) { ++s; lo = end; end = (int)a.offs[s + 1]; }
                // the clamp costs two instructions and keeps every read inside the table whatever strata_dev holds
                u = min(max(lo + (int)__umulhi(w[q], (uint32_t)(end - lo)), 0), a.n - 1);
            }
            bs_add_row<CT, KIND>(acc, tab + (int64_t)u * ldt, a.C, off);
        }
    }
}

// the table, dense, into LDS: 16 bytes a lane where the caller's table is dense and aligned itself
__device__ __forceinline__ void bs_stage(const bs_args& a, int64_t* lds) {
    const int tot = a.n * a.C;
    if (a.vec_stage) {
        const longlong2* src = reinterpret_cast<const longlong2*>(a.table);
        longlong2* dst = reinterpret_cast<longlong2*>(lds);
        for (int i = (int)threadIdx.x; i < (tot >> 1); i += BS_THREADS) dst[i] = src[i];
    } else {
        for (int i = (int)threadIdx.x; i < tot; i += BS_THREADS) {
            const int r = i / a.C;
            lds[i] = a.table[(int64_t)r * a.ld + (i - r * a.C)];
        }
    }
}

// int64 wave sum with DPP (common.h wave_sum_dpp, on both halves of the value): the total, wave-uniform
__device__ __forceinline__ int64_t bs_wave_sum(int64_t v) {
#define BS_DPP_ADD(ctrl, rmask) { \
    const uint32_t xl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)v, ctrl, rmask, 0xf, false); \
    const uint32_t xh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), ctrl, rmask, 0xf, false); \
    v = (int64_t)((uint64_t)v + (((uint64_t)xh << 32) | xl)); }
    BS_DPP_ADD(0xB1, 0xf)     // quad_perm [1,0,3,2]
    BS_DPP_ADD(0x4E, 0xf)     // quad_perm [2,3,0,1]
    BS_DPP_ADD(0x141, 0xf)    // row_half_mirror
    BS_DPP_ADD(0x140, 0xf)    // row_mirror        -> every lane holds its 16-lane row sum
    BS_DPP_ADD(0x142, 0xa)    // row_bcast15 into rows 1,3
    BS_DPP_ADD(0x143, 0xc)    // row_bcast31 into rows 2,3 -> lane 63 holds the wave sum
#undef BS_DPP_ADD
    const uint32_t tl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, 63);
    const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), 63);
    return (int64_t)(((uint64_t)th << 32) | tl);
}

extern __shared__ __attribute__((aligned(16))) int64_t bs_lds[];

template <int CT, int KIND>
__global__ void __launch_bounds__(BS_THREADS) bs_lane_kernel(const bs_args a) {
    bs_stage(a, bs_lds);
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * BS_THREADS, row = base + threadIdx.x;
    int64_t acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0;
    if (row < a.R) {
        const uint64_t r = a.r0 + (uint64_t)row;
        const uint32_t nblk = (uint32_t)(a.n + 3) >> 2;
        for (uint32_t j = 0; j < nblk; ++j) bs_block<CT, KIND>(acc, a, bs_lds, a.C, j, (uint32_t)r, (uint32_t)(r >> 32));
    }
    __syncthreads();                                 // every wave is through with the table: its LDS takes the sums, [lane][C]
#pragma unroll
    for (int c = 0; c < CT; ++c)
        if (c < a.C) bs_lds[(int)threadIdx.x * a.C + c] = acc[c];
    __syncthreads();
    const int cnt = (int)(a.R - base < BS_THREADS ? a.R - base : BS_THREADS) * a.C;
    for (int i = (int)threadIdx.x; i < cnt; i += BS_THREADS) a.out[base * a.C + i] = bs_lds[i];
}

template <int CT, int KIND, bool LDS>
__global__ void __launch_bounds__(BS_THREADS) bs_wave_kernel(const bs_args a, const int rpb) {
    const int64_t* tab = a.table;
    int64_t ldt = a.ld;
    if constexpr (LDS) {
        bs_stage(a, bs_lds);
        __syncthreads();
        tab = bs_lds;
        ldt = a.C;
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * rpb, stop = base + rpb < a.R ? base + rpb : a.R;
    const uint32_t nblk = (uint32_t)(a.n + 3) >> 2;
    for (int64_t row = base + wave; row < stop; row += BS_THREADS / 64) {
        const uint64_t r = a.r0 + (uint64_t)row;
        int64_t acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0;
        for (uint32_t j = (uint32_t)lane; j < nblk; j += 64) bs_block<CT, KIND>(acc, a, tab, ldt, j, (uint32_t)r, (uint32_t)(r >> 32));
        int64_t mine = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < a.C) {
                const int64_t t = bs_wave_sum(acc[c]);
                mine = lane == c ? t : mine;
            }
        if (lane < a.C) a.out[row * a.C + lane] = mine;
    }
}

// ---- the host side
static inline bool bs_fits_lds(int n, int C) { return (int64_t)n * C * 8 <= DICOW_BOOT_LDS_BYTES; }

extern "C" int dicow_bootstrap_plan(int n, int C) {
    if (n < 1 || n > DICOW_BOOT_MAX_N || C < 1 || C > DICOW_BOOT_MAX_C) return -1;
    if (!bs_fits_lds(n, C)) return DICOW_BOOT_WAVE_L2;
    return n <= BS_LANE_MAX_N ? DICOW_BOOT_LANE_LDS : DICOW_BOOT_WAVE_LDS;
}

template <int CT, int KIND>
static void bs_launch(int plan, const bs_args& a, hipStream_t st) {
    if constexpr (KIND == 3) {                       // the whole-row swap form exists under plan 3 alone (below)
        bs_wave_kernel<CT, KIND, false><<<dim3((unsigned)((a.R + BS_WAVE_L2_RPB - 1) / BS_WAVE_L2_RPB)), BS_THREADS, 0, st>>>(a, BS_WAVE_L2_RPB);
    } else if (plan == DICOW_BOOT_LANE_LDS) {
        const size_t lds = (size_t)std::max(a.n, BS_THREADS) * a.C * 8;
        bs_lane_kernel<CT, KIND><<<dim3((unsigned)((a.R + BS_THREADS - 1) / BS_THREADS)), BS_THREADS, lds, st>>>(a);
    } else if (plan == DICOW_BOOT_WAVE_LDS) {
        const size_t lds = ((size_t)a.n * a.C * 8 + 15) / 16 * 16;
        bs_wave_kernel<CT, KIND, true><<<dim3((unsigned)((a.R + BS_WAVE_LDS_RPB - 1) / BS_WAVE_LDS_RPB)), BS_THREADS, lds, st>>>(a, BS_WAVE_LDS_RPB);
    } else {
        bs_wave_kernel<CT, KIND, false><<<dim3((unsigned)((a.R + BS_WAVE_L2_RPB - 1) / BS_WAVE_L2_RPB)), BS_THREADS, 0, st>>>(a, BS_WAVE_L2_RPB);
    }
}

template <int CT>
static void bs_launch_kind(int kind, int plan, const bs_args& a, hipStream_t st) {
    if (kind == 0) bs_launch<CT, 0>(plan, a, st);
    else if (kind == 1) bs_launch<CT, 1>(plan, a, st);
    else if (kind == 2) bs_launch<CT, 2>(plan, a, st);
    else bs_launch<CT, 3>(plan, a, st);
}

extern "C" int dicow_bootstrap_sums(const int64_t* table, int64_t ld, int n, int C, const int64_t* strata, const int64_t* strata_dev, int n_strata,
                                    int64_t R, uint64_t first_replicate, uint64_t seed, int mode, int plan, int64_t* out, void* stream) {
    DICOW_REQUIRE(n >= 1 && n <= DICOW_BOOT_MAX_N, "bootstrap_sums: n=%d, outside [1, DICOW_BOOT_MAX_N = %d]", n, DICOW_BOOT_MAX_N);
    DICOW_REQUIRE(C >= 1 && C <= DICOW_BOOT_MAX_C, "bootstrap_sums: C=%d, outside [1, DICOW_BOOT_MAX_C = %d]", C, DICOW_BOOT_MAX_C);
    DICOW_REQUIRE(ld >= C, "bootstrap_sums: ld=%lld is below C=%d", (long long)ld, C);
    DICOW_REQUIRE(R >= 0 && R <= DICOW_BOOT_MAX_R, "bootstrap_sums: R=%lld, outside [0, DICOW_BOOT_MAX_R = %lld]", (long long)R, (long long)DICOW_BOOT_MAX_R);
    DICOW_REQUIRE(mode == DICOW_BOOT_RESAMPLE || mode == DICOW_BOOT_SWAP, "bootstrap_sums: mode=%d is neither DICOW_BOOT_RESAMPLE (0) nor DICOW_BOOT_SWAP (1)",
                  mode);
    DICOW_REQUIRE(mode != DICOW_BOOT_SWAP || C % 2 == 0, "bootstrap_sums: swap mode exchanges the two halves of the columns, C=%d is odd", C);
    DICOW_REQUIRE(plan >= 0 && plan <= DICOW_BOOT_PLANS, "bootstrap_sums: plan=%d is none of 0 (the library's choice), 1 (LANE_LDS), 2 (WAVE_LDS), "
                  "3 (WAVE_L2)", plan);
    if (plan == 0) plan = dicow_bootstrap_plan(n, C);
    DICOW_REQUIRE(plan == DICOW_BOOT_WAVE_L2 || bs_fits_lds(n, C), "bootstrap_sums: plan=%d stages the table in LDS, and n * C * 8 = %lld bytes are "
                  "past DICOW_BOOT_LDS_BYTES = %d", plan, (long long)n * C * 8, DICOW_BOOT_LDS_BYTES);
    DICOW_REQUIRE(n_strata >= 1 && n_strata <= n, "bootstrap_sums: n_strata=%d, outside [1, n = %d]", n_strata, n);
    DICOW_REQUIRE(strata, "bootstrap_sums: null strata (S = 1 is the offsets {0, n})");
    DICOW_REQUIRE(strata[0] == 0 && strata[n_strata] == n, "bootstrap_sums: the strata run from %lld to %lld, not from 0 to n = %d", (long long)strata[0],
                  (long long)strata[n_strata], n);
    for (int s = 0; s < n_strata; ++s)
        DICOW_REQUIRE(strata[s + 1] > strata[s], "bootstrap_sums: stratum %d is empty or the offsets descend (%lld, then %lld)", s, (long long)strata[s],
                      (long long)strata[s + 1]);
    if (R == 0) return DICOW_OK;
    const bool reads_strata = n_strata > 1 && mode == DICOW_BOOT_RESAMPLE;
    DICOW_REQUIRE(table && out && (strata_dev || !reads_strata), "bootstrap_sums: null pointer");
    DICOW_REQUIRE(dicow_aligned(8, table, out, strata_dev),
                  "bootstrap_sums: table / out / strata_dev not 8-byte aligned");
    bs_args a;
    a.table = table; a.offs = strata_dev; a.out = out;
    a.ld = ld; a.R = R;
    a.r0 = first_replicate;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.n = n; a.C = C; a.S = reads_strata ? n_strata : 1;
    const bool aligned16 = dicow_aligned(16, table);
    a.vec_stage = ld == C && aligned16 && ((int64_t)n * C) % 2 == 0;
    int CT = 1;
    while (CT < C) CT *= 2;
    const bool rows16 = C % 2 == 0 && (plan != DICOW_BOOT_WAVE_L2 || (ld % 2 == 0 && aligned16));      // staged rows are dense and aligned
    // Swap mode reads whole rows 16 bytes a load under plan 3 with 2 or 4 columns alone.  Measured (profiles/bootstrap.txt): 20 000 x 4 through L2
    // 8.2 ms against 20.9 ms with 8-byte reads at the exchanged column.  With 16 columns the selects cost more than the reads save: under plan 1,
    // where a wave reads ONE row (a broadcast), 0.119 ms against 0.055 ms at 40 x 16, and under plan 3 0.557 ms there against 0.286 ms with the
    // 8-byte reads.  Plan 2, and 8 columns, were not measured with it.
    const int kind = mode == DICOW_BOOT_RESAMPLE ? (rows16 ? 1 : 0) : (rows16 && CT == C && C <= 4 && plan == DICOW_BOOT_WAVE_L2 ? 3 : 2);
    hipStream_t st = (hipStream_t)stream;
    switch (CT) {
        case 1: bs_launch_kind<1>(kind, plan, a, st); break;
        case 2: bs_launch_kind<2>(kind, plan, a, st); break;
        case 4: bs_launch_kind<4>(kind, plan, a, st); break;
        case 8: bs_launch_kind<8>(kind, plan, a, st); break;
        case 16: bs_launch_kind<16>(kind, plan, a, st); break;
        default: bs_launch_kind<32>(kind, plan, a, st); break;
    }
    DICOW_CHECK_LAUNCH("bootstrap_sums");
    return DICOW_OK;
}

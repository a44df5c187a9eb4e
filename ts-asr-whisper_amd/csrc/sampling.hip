// Sampling a step's next tokens (dicow_sample_tokens; definition in include/dicow_hip.h): temperature, top-k, top-p and min-p warpers, a
// counter-addressed Gumbel-max draw, the chosen token's log-probability and the finished-row bookkeeping, one launch per decoding step.
//
// One workgroup of 1024 lanes owns a row; lane l owns tokens l, l + 1024, ...  Every rule cuts the order of y = x / temperature from
// below, so the whole warper chain ends as ONE threshold on the order-preserving 32-bit key of y (-0.0 and +0.0 share a key; -inf, NaN and
// the padding past V sit below every threshold):
//   top_k   the k-th largest key: 32 rounds of count-and-reduce, bit by bit from the top (exact integers);
//   top_p   the largest key t with mass{key <= t} <= (1 - top_p) Z: the same 32 rounds over fp64 masses of fp32 exps.  The mass is
//           monotone in t (nonnegative terms added in one fixed order), so the bisection is exact for the mass as computed;
//   min_p   the smallest key whose fp64 ratio exp(y - y_max) reaches min_p: one pass and a min.
// Sums and counts go lane-serial (ascending tokens), then an xor butterfly over the wave (both partners add the same two numbers, so
// every lane holds the same bits), then the 16 wave results in order: a fixed order whatever the plan.
// The draw is a pure argmax of y_v - log(-log(u_v)) over the kept tokens, u_v from Philox4x32-10 at counter (v >> 2, row_id, step, stream):
// a second copy of bootstrap.hip's ten rounds (that file's kernels stay what they were).  Only kept tokens pay for their Philox block.
// Plans: DICOW_SAMPLE_REG reads the row once and keeps y in registers (up to 64 a lane: V <= 65536); DICOW_SAMPLE_STREAM re-reads the row (from
// L2) and divides again on every pass.  Both run the same passes in the same order on the same values: identical bits.
#include "common.h"
#include <math.h>

#define SMP_BLOCK 1024
#define SMP_WAVES (SMP_BLOCK / DICOW_WAVE)
#define SMP_NPL (DICOW_SAMPLE_REG_MAX_V / SMP_BLOCK)
#define SMP_KEY_NEG_INF 0x007fffffu                  // smp_key(-inf): every score above -inf has a larger key

struct smp_shared {
    double d[SMP_WAVES];
    float f[SMP_WAVES];
    uint32_t u[SMP_WAVES];
};

__device__ __forceinline__ uint32_t smp_key(float y) {
    uint32_t b = __float_as_uint(y);
    if (b == 0x80000000u) b = 0u;                    // -0.0 compares equal to +0.0
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// (the rounds stay a loop: the passes below are unrolled over the lane's values, and hipcc gives up on an unrolled body that large)
__device__ __forceinline__ void smp_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll 1
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// -log(-log(u)), u = ((w >> 8) + 0.5) 2^-24.  u needs 25 bits from 2^23 on: there -log(u) comes from the exact complement 1 - u
__device__ __forceinline__ float smp_gumbel(uint32_t w) {
    const uint32_t m = w >> 8;
    float l;
    if (m < 0x800000u) l = -logf(((float)m + 0.5f) * 0x1p-24f);
    else l = -log1pf(-(((float)(0xffffffu - m) + 0.5f) * 0x1p-24f));
    return -logf(l);
}

// ---- workgroup reductions; every lane of the workgroup calls them (full EXEC), every lane gets the result
__device__ __forceinline__ uint32_t smp_sum_u32(uint32_t v, smp_shared& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    if ((threadIdx.x & 63) == 0) s.u[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) t += s.u[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ uint32_t smp_min_u32(uint32_t v, smp_shared& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0) s.u[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0xffffffffu;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) t = min(t, s.u[w]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ double smp_sum_f64(double v, smp_shared& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s.d[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) t += s.d[w];
    __syncthreads();
    return t;
}
// the largest value and the lowest index that holds it (idx = 0x7fffffff: the lane saw nothing above -inf)
__device__ __forceinline__ void smp_argmax(float& val, int& idx, smp_shared& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float pv = __shfl_xor(val, o, 64);
        const int pi = __shfl_xor(idx, o, 64);
        if (pv > val || (pv == val && pi < idx)) { val = pv; idx = pi; }
    }
    if ((threadIdx.x & 63) == 0) { s.f[threadIdx.x >> 6] = val; s.u[threadIdx.x >> 6] = (uint32_t)idx; }
    __syncthreads();
    val = s.f[0]; idx = (int)s.u[0];
#pragma unroll
    for (int w = 1; w < SMP_WAVES; ++w) {
        const float pv = s.f[w];
        const int pi = (int)s.u[w];
        if (pv > val || (pv == val && pi < idx)) { val = pv; idx = pi; }
    }
    __syncthreads();
}

// the row as the passes see it: f(v, y_v) for the lane's tokens in ascending order, y = -inf for NaN and past V.  NPL > 0: the lane's NPL
// values are held in registers (the padding past V included: it sits below every threshold); NPL == 0: every pass loads and divides again
struct smp_src {
    const float* x;
    float t;
    int V, nit;
    bool scale;
    __device__ __forceinline__ float load(int v) const {
        if (v >= V) return -INFINITY;
        float a = x[v];
        if (a != a) a = -INFINITY;
        return scale ? __fdiv_rn(a, t) : a;
    }
};
template <int NPL, class F>
__device__ __forceinline__ void smp_each(const smp_src& src, const float (&y)[NPL ? NPL : 1], F&& f) {
    if constexpr (NPL > 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            float yi = y[i];
            asm volatile("" : "+v"(yi));             // what a pass derives from y is derived anew: hoisted out of the 32-round loops it
            f(i * SMP_BLOCK + (int)threadIdx.x, yi); // would double the registers (keys and exps of every value) and spill
        }
    } else {
        for (int i = 0; i < src.nit; ++i) {
            const int v = i * SMP_BLOCK + (int)threadIdx.x;
            f(v, src.load(v));
        }
    }
}

template <int NPL>
__global__ void __launch_bounds__(SMP_BLOCK) sample_tokens_kernel(const dicow_sample_args a) {
    __shared__ smp_shared sh;
    const int r = blockIdx.x;
    const int V = a.V;
    smp_src row;
    row.x = a.scores + (int64_t)r * a.ld;
    row.t = a.temperature;
    row.V = V;
    row.nit = (V + SMP_BLOCK - 1) / SMP_BLOCK;
    row.scale = a.temperature > 0.f;
    float yreg[NPL ? NPL : 1];
    if constexpr (NPL > 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) yreg[i] = row.load(i * SMP_BLOCK + (int)threadIdx.x);
    }

    // the maximum of y and its lowest index
    float ymax = -INFINITY;
    int imax = 0x7fffffff;
    smp_each<NPL>(row, yreg, [&](int v, float y) { if (y > ymax) { ymax = y; imax = v; } });
    smp_argmax(ymax, imax, sh);
    const bool any = imax != 0x7fffffff;                 // (wave- and workgroup-uniform from here on)
    const uint32_t kmax = smp_key(ymax);
    uint32_t lo = SMP_KEY_NEG_INF + 1u;                  // kept <=> smp_key(y) >= lo

    if (row.scale && any) {
        const int k = a.top_k < V ? a.top_k : V;
        if (a.top_k > 0 && k < V) {                      // the k-th largest key: the largest T with count{key >= T} >= k
            uint32_t T = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t trial = T | (1u << bit);
                uint32_t c = 0;
                smp_each<NPL>(row, yreg, [&](int, float y) { c += smp_key(y) >= trial ? 1u : 0u; });
                if (smp_sum_u32(c, sh) >= (uint32_t)k) T = trial;
            }
            lo = max(lo, T);
        }
        if (a.top_p < 1.f) {                             // the largest t with mass{lo <= key <= t} <= (1 - top_p) Z
            const uint32_t lo_k = lo;
            auto mass = [&](uint32_t upto) {
                double m = 0.0;
                smp_each<NPL>(row, yreg, [&](int, float y) {
                    const uint32_t key = smp_key(y);
                    if (key >= lo_k && key <= upto) m += (double)__builtin_amdgcn_exp2f((y - ymax) * 1.44269504088896341f);
                });
                return smp_sum_f64(m, sh);
            };
            const double cut = (1.0 - (double)a.top_p) * mass(0xffffffffu);
            uint32_t t = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t trial = t | (1u << bit);
                if (mass(trial) <= cut) t = trial;
            }
            if (t >= kmax) t = kmax - 1u;                // the maximum is always kept (kmax > SMP_KEY_NEG_INF here)
            lo = max(lo, t + 1u);
        }
        if (a.min_p > 0.f) {                             // the smallest key whose ratio reaches min_p
            const uint32_t lo_p = lo;
            const double mp = (double)a.min_p;
            uint32_t kmin = kmax;
            smp_each<NPL>(row, yreg, [&](int, float y) {
                const uint32_t key = smp_key(y);
                if (key >= lo_p && key < kmin && exp((double)y - (double)ymax) >= mp) kmin = key;
            });
            lo = max(lo, smp_min_u32(kmin, sh));
        }
    }

    if (a.warped) {
        float* w = a.warped + (int64_t)r * a.ld_w;
        smp_each<NPL>(row, yreg, [&](int v, float y) { if (v < V) w[v] = smp_key(y) >= lo ? y : -INFINITY; });
    }

    int tok = imax;
    if (row.scale && any) {                              // Gumbel-max over the kept tokens
        const int64_t rid = a.row_ids ? a.row_ids[r] : (int64_t)r;
        const uint32_t c1 = (uint32_t)rid, k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
        float best = -INFINITY;
        int ibest = 0x7fffffff;
        smp_each<NPL>(row, yreg, [&](int v, float y) {
            if (smp_key(y) < lo) return;
            uint32_t w[4];
            smp_philox((uint32_t)v >> 2, c1, a.step, a.stream, k0, k1, w);
            const float g = y + smp_gumbel(w[v & 3]);
            if (g > best || ibest == 0x7fffffff) { best = g; ibest = v; }
        });
        smp_argmax(best, ibest, sh);
        tok = ibest;
    }
    const bool drew = any && tok >= 0 && tok < V;        // (always true when `any`: the maximum is never removed)

    float lp = 0.f;
    if (a.logprob) {                                     // x_tok - logsumexp{x_v : v kept}
        if (!drew) lp = __uint_as_float(0x7fc00000u);
        else {
            const float xmax = row.x[imax], xtok = row.x[tok];
            double sum = 0.0;
            smp_each<NPL>(row, yreg, [&](int v, float y) {
                if (smp_key(y) >= lo) sum += (double)expf(row.x[v] - xmax);
            });
            sum = smp_sum_f64(sum, sh);
            lp = (float)(((double)xtok - (double)xmax) - log(sum));
        }
    }

    if (threadIdx.x == 0) {
        int64_t out = drew ? tok : a.eos;
        bool live = true;
        if (a.unfinished) {
            live = a.unfinished[r] != 0;
            if (!live) { out = a.pad; lp = 0.f; }
            else if (out == a.eos) a.unfinished[r] = 0;
        }
        a.next[(int64_t)r * a.next_stride] = out;
        if (a.logprob) a.logprob[r] = lp;
    }
}

extern "C" int dicow_sample_tokens(const dicow_sample_args* a, void* stream) {
    DICOW_REQUIRE(a, "sample_tokens: null args");
    DICOW_REQUIRE(a->rows >= 0, "sample_tokens: rows=%d is negative", a->rows);
    DICOW_REQUIRE(a->plan >= 0 && a->plan <= DICOW_SAMPLE_PLANS, "sample_tokens: plan %d is not 0 .. %d", a->plan, DICOW_SAMPLE_PLANS);
    DICOW_REQUIRE(a->V >= 1 && a->ld >= a->V, "sample_tokens: bad shape V=%d ld=%lld", a->V, (long long)a->ld);
    DICOW_REQUIRE(a->plan != DICOW_SAMPLE_REG || a->V <= DICOW_SAMPLE_REG_MAX_V,
                  "sample_tokens: V=%d exceeds DICOW_SAMPLE_REG_MAX_V (%d) of plan DICOW_SAMPLE_REG", a->V, DICOW_SAMPLE_REG_MAX_V);
    DICOW_REQUIRE(a->temperature == a->temperature && a->top_p == a->top_p && a->min_p == a->min_p,
                  "sample_tokens: temperature, top_p and min_p must not be NaN");
    if (a->rows == 0) return DICOW_OK;
    DICOW_REQUIRE(a->scores && a->next, "sample_tokens: scores and next must be given");
    DICOW_REQUIRE(!a->warped || a->ld_w >= a->V, "sample_tokens: ld_w=%lld is below V=%d", (long long)a->ld_w, a->V);
    const int plan = a->plan ? a->plan : (a->V <= DICOW_SAMPLE_REG_MAX_V ? DICOW_SAMPLE_REG : DICOW_SAMPLE_STREAM);
    const dim3 grid((unsigned)a->rows);
    const int nit = dicow_cdiv(a->V, SMP_BLOCK);          // values a lane: REG is instantiated for 4, 16, 32, 52 (V = 51 866: 51) and 64
    hipStream_t st = (hipStream_t)stream;
    if (plan != DICOW_SAMPLE_REG) sample_tokens_kernel<0><<<grid, SMP_BLOCK, 0, st>>>(*a);
    else if (nit <= 4) sample_tokens_kernel<4><<<grid, SMP_BLOCK, 0, st>>>(*a);
    else if (nit <= 16) sample_tokens_kernel<16><<<grid, SMP_BLOCK, 0, st>>>(*a);
    else if (nit <= 32) sample_tokens_kernel<32><<<grid, SMP_BLOCK, 0, st>>>(*a);
    else if (nit <= 52) sample_tokens_kernel<52><<<grid, SMP_BLOCK, 0, st>>>(*a);
    else sample_tokens_kernel<SMP_NPL><<<grid, SMP_BLOCK, 0, st>>>(*a);
    DICOW_CHECK_LAUNCH("sample_tokens_kernel");
    return DICOW_OK;
}

// Scoring a diarization against a reference: the counts behind DER, JER and the optimal speaker mapping (pyannote.metrics' quantities, which
// the reference's utils/compute_der_between_cutsets.py and utils/align_and_compute_der_between_cutsets.py print) for a batch of problems,
// in exact int64 ticks.  include/dicow_hip.h has the definition in full.  A problem is two tables of the diarization front end (sorted
// bounds, one speaker bitmask per entry), a sorted list of disjoint unscored intervals (the collars) and a skip_overlap flag; its elementary
// regions are the intervals between neighbours of the merge of the three endpoint lists, and everything asked for is a sum of
// (region length) x (a function of the two bitmasks) over the scored regions.
//   ds_merge_kernel    one lane per endpoint: its rank in the merge is its own index plus two binary searches in the other lists (ties:
//                      reference, hypothesis, unscored; then the index), so the merged list is written without a sort, a serial merge or a
//                      second writer of any word.  Coincident endpoints give regions of length 0 that add nothing.
//   ds_accum_kernel    one workgroup per chunk of `chunk` regions of one problem (found by bisection over the problems' first blocks):
//                      every lane stages regions -- length, the two bitmasks by binary search, 0 as the length of a region that is not
//                      scored -- in LDS and sums the five scalars as it goes; then every lane walks the staged chunk for the 16 cells of
//                      C it owns (row tid / 4, columns 16 (tid % 4) ..): the region read is an LDS broadcast and the skip of a region
//                      without a reference or without a hypothesis speaker is wave-uniform.  Wave 3 does R, wave 2 H (they own the rows
//                      48 .. 63 and 32 .. 47 of C, which few meetings have).  The chunk's sums go to a partial of 64 Sr + 136 words.
//   ds_reduce_kernel   one lane per output word: the sum of its partials in ascending chunk order, or 0.
// No atomics, one writer per word, integers only: the bits do not depend on the chunk size, the grid or the call's other problems.
#include "host_table.h"
#include <vector>

#define DS_THREADS 256
#define DS_CHUNK DICOW_DIAR_SCORE_CHUNK
#define DS_ROW DICOW_DIAR_SCORE_ROW
#define DS_OUT DICOW_DIAR_SCORE_OUT_WORDS
#define DS_TAIL 136             // R [64], H [64], 8 scalars behind the 64 Sr cells of C in a partial
static_assert(DS_OUT == 64 * 64 + DS_TAIL, "an output row is C, R, H and 8 scalars");

struct ds_prob {
    int64_t ref_b, ref_a, hyp_b, hyp_a, uns;    // first elements in the uploaded bounds / active / unscored (flat endpoints) arrays
    int64_t merged, part;                       // int64 words from ws: the merged endpoints [M]; the partials [n_chunks][64 Sr + 136]
    int64_t lo, hi;                             // the first and the last bound of the two tables (0, 0 when both are empty)
    int32_t Er, Eh, Nu, M;                      // Nu: unscored ENDPOINTS (twice the intervals); M: all endpoints
    int32_t Sr, Sh, skip, n_chunks;
    int32_t pt_blk0, chunk_blk0, pad[2];        // the problem's first block in the merge / the accumulation grid
};
static_assert(sizeof(ds_prob) == DICOW_DIAR_SCORE_DESC_BYTES, "DICOW_DIAR_SCORE_DESC_BYTES is the size of a problem's descriptor");

struct ds_args {
    const ds_prob* probs;
    const int64_t* bounds;
    const uint64_t* active;
    const int64_t* uns;
    int64_t* ws;
    int64_t* out;
    int n, chunk;
};

// how many of the sorted a[0 .. n) are <= v (UPPER) or < v
template <bool UPPER>
__device__ __forceinline__ int ds_count(const int64_t* __restrict__ a, int n, int64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int64_t x = a[mid];
        if (UPPER ? x <= v : x < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the last problem whose first block is <= b (a problem without blocks never owns one: it shares its first block with its successor)
template <bool MERGE>
__device__ __forceinline__ int ds_find(const ds_prob* __restrict__ probs, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((MERGE ? probs[mid].pt_blk0 : probs[mid].chunk_blk0) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(DS_THREADS) ds_merge_kernel(const ds_args a) {
    const ds_prob& pr = a.probs[ds_find<true>(a.probs, a.n, blockIdx.x)];
    const int i = (blockIdx.x - pr.pt_blk0) * DS_THREADS + threadIdx.x;
    if (i >= pr.M) return;
    const int nr = pr.Er ? pr.Er + 1 : 0, nh = pr.Eh ? pr.Eh + 1 : 0, nu = pr.Nu;
    const int64_t* __restrict__ rb = a.bounds + pr.ref_b;
    const int64_t* __restrict__ hb = a.bounds + pr.hyp_b;
    const int64_t* __restrict__ ub = a.uns + pr.uns;
    int64_t v;
    int rank;
    if (i < nr) {
        v = rb[i];
        rank = i + ds_count<false>(hb, nh, v) + ds_count<false>(ub, nu, v);
    } else if (i < nr + nh) {
        v = hb[i - nr];
        rank = i - nr + ds_count<true>(rb, nr, v) + ds_count<false>(ub, nu, v);
    } else {
        v = ub[i - nr - nh];
        rank = i - nr - nh + ds_count<true>(rb, nr, v) + ds_count<true>(hb, nh, v);
    }
    a.ws[pr.merged + rank] = v;                                                // 0 <= rank < M: the ranks of a problem are a permutation
}

// the bitmask of a table on the region that starts at the merged endpoint s
__device__ __forceinline__ uint64_t ds_bits(const int64_t* __restrict__ b, const uint64_t* __restrict__ act, int E, int64_t s) {
    if (E == 0) return 0;
    const int q = ds_count<true>(b, E + 1, s);                                 // bounds <= s
    return q >= 1 && q <= E ? act[q - 1] : 0;
}

__device__ __forceinline__ int64_t ds_wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(DS_THREADS) ds_accum_kernel(const ds_args a) {
    __shared__ int64_t s_dur[DS_CHUNK];
    __shared__ uint64_t s_rb[DS_CHUNK], s_hb[DS_CHUNK];
    __shared__ int64_t s_red[DS_THREADS / DICOW_WAVE][5];
    const ds_prob& pr = a.probs[ds_find<false>(a.probs, a.n, blockIdx.x)];
    const int tid = threadIdx.x, c = blockIdx.x - pr.chunk_blk0;
    const int k0 = c * a.chunk, n = min(a.chunk, pr.M - 1 - k0);               // 1 <= n: the grid holds the chunks that have regions
    const int64_t* __restrict__ mg = a.ws + pr.merged + k0;
    const int64_t* __restrict__ ub = a.uns + pr.uns;
    int64_t sc[5] = {0, 0, 0, 0, 0};
    for (int r = tid; r < n; r += DS_THREADS) {
        const int64_t s = mg[r];
        int64_t dur = mg[r + 1] - s;
        uint64_t rbits = 0, hbits = 0;
        if (dur > 0) {
            if (ds_count<true>(ub, pr.Nu, s) & 1) {                            // an odd number of interval ends behind it: inside one
                dur = 0;
            } else {
                rbits = ds_bits(a.bounds + pr.ref_b, a.active + pr.ref_a, pr.Er, s);
                hbits = ds_bits(a.bounds + pr.hyp_b, a.active + pr.hyp_a, pr.Eh, s);
                const int nr = __popcll(rbits), nh = __popcll(hbits);
                if (pr.skip && nr > 1) {
                    dur = 0;
                } else {
                    sc[0] += s >= pr.lo && s < pr.hi ? dur : 0;
                    sc[1] += dur * nr;
                    sc[2] += dur * max(0, nr - nh);
                    sc[3] += dur * max(0, nh - nr);
                    sc[4] += dur * min(nr, nh);
                }
            }
        }
        s_dur[r] = dur;
        s_rb[r] = rbits;
        s_hb[r] = hbits;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int64_t t = ds_wave_sum(sc[q]);
        if ((tid & (DICOW_WAVE - 1)) == 0) s_red[tid / DICOW_WAVE][q] = t;
    }
    __syncthreads();
    int64_t* __restrict__ part = a.ws + pr.part + (int64_t)c * (64 * pr.Sr + DS_TAIL);
    if (tid < 8) {
        int64_t t = 0;
        if (tid < 5)
            for (int w = 0; w < DS_THREADS / DICOW_WAVE; ++w) t += s_red[w][tid];
        part[64 * pr.Sr + 128 + tid] = t;
    }
    const int i = tid >> 2, j0 = (tid & 3) * 16;
    if (i < pr.Sr && j0 < pr.Sh) {
        int64_t acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0;
        for (int r = 0; r < n; ++r) {
            const int64_t dur = s_dur[r];
            const uint64_t rbits = s_rb[r], hbits = s_hb[r];
            if (dur == 0 || rbits == 0 || hbits == 0) continue;                // (the same words in every lane: uniform)
            const unsigned h16 = (unsigned)(hbits >> j0) & 0xffffu;
            if (((rbits >> i) & 1) == 0 || h16 == 0) continue;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] += (h16 >> q) & 1 ? dur : 0;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) part[64 * i + j0 + q] = acc[q];
    }
    if (tid >= 2 * DICOW_WAVE) {                                               // wave 3: R, wave 2: H
        const bool is_r = tid >= 3 * DICOW_WAVE;
        const int s = tid & (DICOW_WAVE - 1);
        const uint64_t* __restrict__ bits = is_r ? s_rb : s_hb;
        int64_t acc = 0;
        for (int r = 0; r < n; ++r) {
            const int64_t dur = s_dur[r];
            if (dur == 0) continue;
            acc += (bits[r] >> s) & 1 ? dur : 0;
        }
        part[64 * pr.Sr + (is_r ? 0 : 64) + s] = acc;
    }
}

__global__ void __launch_bounds__(DS_THREADS) ds_reduce_kernel(const ds_args a) {
    const ds_prob& pr = a.probs[blockIdx.x];
    const int64_t stride = 64 * pr.Sr + DS_TAIL;
    const int64_t* __restrict__ part = a.ws + pr.part;
    int64_t* __restrict__ out = a.out + (int64_t)blockIdx.x * DS_OUT;
    const int w = blockIdx.y * DS_THREADS + threadIdx.x;
    if (w < DS_OUT) {
        int src = -1;                                                          // the word's place in a partial, if the chunks wrote it
        if (w < 64 * 64) {
            const int i = w >> 6, j = w & 63;
            if (i < pr.Sr && (j & ~15) < pr.Sh) src = w;
        } else {
            src = 64 * pr.Sr + (w - 64 * 64);
        }
        int64_t sum = 0;
        if (src >= 0)
            for (int c = 0; c < pr.n_chunks; ++c) sum += part[c * stride + src];
        out[w] = sum;
    }
}

// ---- the host's plan: every check, the descriptors and the workspace layout, before anything is launched
struct ds_plan {
    std::vector<int64_t> stage;            // the descriptors: [n] ds_prob (the three arrays are uploaded from where the caller has them)
    int64_t desc_words = 0, need = 0;
    int pt_blocks = 0, chunk_blocks = 0, chunk = 0;
};

static int ds_check_table(const char* who, int k, const char* side, const int64_t* bounds, int64_t n_bounds, const uint64_t* active,
                          int64_t n_active, int64_t b0, int64_t a0, int64_t E, int64_t S) {
    DICOW_REQUIRE(S >= 0 && S <= 64, "%s: problem %d has %lld %s speakers, outside [0, 64]", who, k, (long long)S, side);
    DICOW_REQUIRE(E >= 0 && E <= DICOW_DIAR_SCORE_MAX_E, "%s: the %s table of problem %d has %lld entries, outside [0, DICOW_DIAR_SCORE_MAX_E = %d]",
                  who, side, k, (long long)E, DICOW_DIAR_SCORE_MAX_E);
    if (E == 0) return DICOW_OK;                                               // an empty table: nothing of it is read
    DICOW_REQUIRE(bounds && active, "%s: null bounds or active table", who);
    DICOW_REQUIRE(dicow_span_ok(b0, E + 1, n_bounds), "%s: the %s table of problem %d reads bounds [%lld, %lld + %lld], outside the "
                  "%lld of the array", who, side, k, (long long)b0, (long long)b0, (long long)E, (long long)n_bounds);
    DICOW_REQUIRE_SPAN(a0, E, n_active, "reads active", "of the array", "%s: the %s table of problem %d", who, side, k);
    const int64_t* b = bounds + b0;
    const uint64_t* act = active + a0;
    DICOW_REQUIRE(b[0] >= 0 && b[E] <= DICOW_DIAR_SCORE_MAX_TICK, "%s: the %s bounds of problem %d, [%lld, %lld], leave [0, DICOW_DIAR_SCORE_MAX_TICK]",
                  who, side, k, (long long)b[0], (long long)b[E]);
    const uint64_t legal = S == 64 ? ~(uint64_t)0 : (((uint64_t)1 << S) - 1);
    for (int64_t e = 0; e < E; ++e) {
        DICOW_REQUIRE(b[e] < b[e + 1], "%s: the %s bounds of problem %d are not strictly increasing at %lld (%lld, %lld)", who, side, k, (long long)e,
                      (long long)b[e], (long long)b[e + 1]);
        DICOW_REQUIRE((act[e] & ~legal) == 0, "%s: %s active[%lld] of problem %d names a speaker >= S=%lld", who, side, (long long)e, k, (long long)S);
    }
    return DICOW_OK;
}

static int ds_make_plan(const char* who, const int64_t* bounds, int64_t n_bounds, const uint64_t* active, int64_t n_active, const int64_t* unscored,
                        int64_t n_unscored, const int64_t* problems, int n, int chunk, ds_plan& pl) {
    DICOW_REQUIRE(n >= 0, "%s: negative n_problems=%d", who, n);
    DICOW_REQUIRE(n == 0 || problems, "%s: null problem table", who);
    DICOW_REQUIRE(n_bounds >= 0 && n_active >= 0 && n_unscored >= 0, "%s: negative array size n_bounds=%lld n_active=%lld n_unscored=%lld", who,
                  (long long)n_bounds, (long long)n_active, (long long)n_unscored);
    DICOW_REQUIRE((n_bounds == 0 || bounds) && (n_active == 0 || active) && (n_unscored == 0 || unscored), "%s: null bounds, active or unscored array",
                  who);
    DICOW_REQUIRE(chunk >= 0 && chunk <= DS_CHUNK, "%s: chunk=%d outside [0, DICOW_DIAR_SCORE_CHUNK = %d]", who, chunk, DS_CHUNK);
    if (chunk == 0) chunk = DS_CHUNK;
    pl.chunk = chunk;
    const int64_t head_words = (int64_t)n * (int64_t)(sizeof(ds_prob) / 8) + n_bounds + n_active + 2 * n_unscored;
    DICOW_REQUIRE(head_words * 8 <= DICOW_DIAR_SCORE_MAX_WS_BYTES, "%s: the tables take more than DICOW_DIAR_SCORE_MAX_WS_BYTES = %lld bytes", who,
                  (long long)DICOW_DIAR_SCORE_MAX_WS_BYTES);
    pl.desc_words = (int64_t)n * (int64_t)(sizeof(ds_prob) / 8);
    pl.stage.assign((size_t)pl.desc_words, 0);
    ds_prob* probs = reinterpret_cast<ds_prob*>(pl.stage.data());
    int64_t words = head_words, pt_blocks = 0, chunk_blocks = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t* row = problems + (int64_t)DS_ROW * k;
        if (int rc = ds_check_table(who, k, "reference", bounds, n_bounds, active, n_active, row[0], row[1], row[2], row[3])) return rc;
        if (int rc = ds_check_table(who, k, "hypothesis", bounds, n_bounds, active, n_active, row[4], row[5], row[6], row[7])) return rc;
        const int64_t u0 = row[8], nu = row[9];
        DICOW_REQUIRE(nu >= 0 && nu <= DICOW_DIAR_SCORE_MAX_E, "%s: problem %d has %lld unscored intervals, outside [0, DICOW_DIAR_SCORE_MAX_E = %d]",
                      who, k, (long long)nu, DICOW_DIAR_SCORE_MAX_E);
        DICOW_REQUIRE(nu == 0 || (unscored && dicow_span_ok(u0, nu, n_unscored)), "%s: problem %d reads unscored intervals "
                      "[%lld, %lld + %lld), outside the %lld of the array", who, k, (long long)u0, (long long)u0, (long long)nu, (long long)n_unscored);
        DICOW_REQUIRE((row[10] == 0 || row[10] == 1) && row[11] == 0, "%s: problem %d has skip_overlap=%lld (0 or 1) and reserved=%lld (0)", who, k,
                      (long long)row[10], (long long)row[11]);
        for (int64_t q = 0; q < nu; ++q) {
            const int64_t* iv = unscored + 2 * (u0 + q);
            DICOW_REQUIRE(iv[0] >= 0 && iv[1] <= DICOW_DIAR_SCORE_MAX_TICK, "%s: unscored interval %lld of problem %d, [%lld, %lld), leaves "
                          "[0, DICOW_DIAR_SCORE_MAX_TICK]", who, (long long)q, k, (long long)iv[0], (long long)iv[1]);
            DICOW_REQUIRE(iv[0] < iv[1], "%s: unscored interval %lld of problem %d, [%lld, %lld), is empty or reversed", who, (long long)q, k,
                          (long long)iv[0], (long long)iv[1]);
            DICOW_REQUIRE(q == 0 || iv[-1] <= iv[0], "%s: unscored intervals %lld and %lld of problem %d overlap or are not sorted (%lld > %lld)", who,
                          (long long)(q - 1), (long long)q, k, (long long)iv[-1], (long long)iv[0]);
        }
        ds_prob& pr = probs[k];
        pr.Er = (int32_t)row[2]; pr.Sr = (int32_t)row[3]; pr.Eh = (int32_t)row[6]; pr.Sh = (int32_t)row[7];
        pr.Nu = (int32_t)(2 * nu); pr.skip = (int32_t)row[10];
        pr.ref_b = pr.Er ? row[0] : 0; pr.ref_a = pr.Er ? row[1] : 0;
        pr.hyp_b = pr.Eh ? row[4] : 0; pr.hyp_a = pr.Eh ? row[5] : 0;
        pr.uns = nu ? 2 * u0 : 0;
        pr.lo = pr.hi = 0;
        if (pr.Er) { pr.lo = bounds[row[0]]; pr.hi = bounds[row[0] + pr.Er]; }
        if (pr.Eh) {
            const int64_t l = bounds[row[4]], h = bounds[row[4] + pr.Eh];
            pr.lo = pr.Er ? (l < pr.lo ? l : pr.lo) : l;
            pr.hi = pr.Er ? (h > pr.hi ? h : pr.hi) : h;
        }
        const int64_t M = (pr.Er ? (int64_t)pr.Er + 1 : 0) + (pr.Eh ? (int64_t)pr.Eh + 1 : 0) + 2 * nu;
        const int64_t n_chunks = M > 1 ? (M - 1 + chunk - 1) / chunk : 0;
        pr.M = (int32_t)M;
        pr.n_chunks = (int32_t)n_chunks;
        pr.pt_blk0 = (int32_t)pt_blocks;
        pr.chunk_blk0 = (int32_t)chunk_blocks;
        pt_blocks += (M + DS_THREADS - 1) / DS_THREADS;
        chunk_blocks += n_chunks;
        pr.merged = words;
        words += M;
        pr.part = words;
        words += n_chunks * (64 * (int64_t)pr.Sr + DS_TAIL);
        DICOW_REQUIRE(words * 8 <= DICOW_DIAR_SCORE_MAX_WS_BYTES && pt_blocks <= INT32_MAX && chunk_blocks <= INT32_MAX, "%s: the merged endpoints and "
                      "partial sums up to problem %d take more than DICOW_DIAR_SCORE_MAX_WS_BYTES = %lld bytes", who, k,
                      (long long)DICOW_DIAR_SCORE_MAX_WS_BYTES);
    }
    pl.pt_blocks = (int)pt_blocks;
    pl.chunk_blocks = (int)chunk_blocks;
    pl.need = words * 8;
    return DICOW_OK;
}

extern "C" int64_t dicow_diar_score_ws_bytes(const int64_t* bounds, int64_t n_bounds, const uint64_t* active, int64_t n_active,
                                             const int64_t* unscored, int64_t n_unscored, const int64_t* problems, int n_problems, int chunk) {
    ds_plan pl;
    if (ds_make_plan("diar_score_ws_bytes", bounds, n_bounds, active, n_active, unscored, n_unscored, problems, n_problems, chunk, pl) != DICOW_OK)
        return -1;
    return pl.need;
}

extern "C" int dicow_diar_score(const int64_t* bounds, int64_t n_bounds, const uint64_t* active, int64_t n_active, const int64_t* unscored,
                                int64_t n_unscored, const int64_t* problems, int n_problems, int chunk, int64_t* out, void* ws, int64_t ws_bytes,
                                void* stream) {
    static thread_local ds_plan pl;                          // pl.stage: the uploaded descriptors
    if (ds_make_plan("diar_score", bounds, n_bounds, active, n_active, unscored, n_unscored, problems, n_problems, chunk, pl) != DICOW_OK)
        return DICOW_ERR_INVALID;
    if (n_problems == 0) return DICOW_OK;
    DICOW_REQUIRE(out && ws, "diar_score: null pointer");
    DICOW_REQUIRE(dicow_aligned(8, out, ws), "diar_score: out or ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= pl.need, "diar_score: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)pl.need);
    hipStream_t st = (hipStream_t)stream;
    ds_args a;
    a.ws = static_cast<int64_t*>(ws);
    a.probs = reinterpret_cast<const ds_prob*>(ws);
    a.bounds = a.ws + pl.desc_words;
    a.active = reinterpret_cast<const uint64_t*>(a.bounds + n_bounds);
    a.uns = a.bounds + n_bounds + n_active;
    // four uploads: the descriptors, then the caller's three arrays from where they are
    if (int rc = dicow_upload("diar_score", ws, pl.stage.data(), pl.desc_words * 8, st)) return rc;
    if (int rc = dicow_upload("diar_score", const_cast<int64_t*>(a.bounds), bounds, n_bounds * 8, st)) return rc;
    if (int rc = dicow_upload("diar_score", const_cast<uint64_t*>(a.active), active, n_active * 8, st)) return rc;
    if (int rc = dicow_upload("diar_score", const_cast<int64_t*>(a.uns), unscored, n_unscored * 16, st)) return rc;
    a.out = out;
    a.n = n_problems;
    a.chunk = pl.chunk;
    if (pl.pt_blocks > 0) ds_merge_kernel<<<dim3((unsigned)pl.pt_blocks), DS_THREADS, 0, st>>>(a);
    if (pl.chunk_blocks > 0) ds_accum_kernel<<<dim3((unsigned)pl.chunk_blocks), DS_THREADS, 0, st>>>(a);
    ds_reduce_kernel<<<dim3((unsigned)n_problems, (DS_OUT + DS_THREADS - 1) / DS_THREADS), DS_THREADS, 0, st>>>(a);
    DICOW_CHECK_LAUNCH("diar_score kernels");
    return DICOW_OK;
}

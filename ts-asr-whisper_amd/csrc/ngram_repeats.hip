// Cutting hallucinated repeats out of hypotheses before they are scored: where the first n-gram of a decoded segment that occurs too often
// ends, and where a run of one repeated word begins (the reference's truncate_at_repeating_ngram, src/data/postprocess.py:18-74, applied
// to every segment by process_session, src/utils/evaluation.py:150-176).  All segments of a corpus are the problems of ONE call.
//
// The definition (include/dicow_hip.h states it in full): a segment of W words with exact ids id[] and folded ids fold[];
//     run(i)   the length of the maximal run fold[i] == fold[i + 1] == ... that starts at i
//     occ_n(i) the number of j in [0, W - n] with id[j .. j + n) == id[i .. i + n), j == i and overlaps included
//     cnt_n(i) occ_n(i), or 0 where fold[i .. i + n) are all equal (run(i) >= n), for max(2, min_n) <= n <= max_n
//     keep     W if W < min_words, else the minimum of W, i0 + 1 (min_n == 1; i0 the first i with run(i) >= u) and i + n over cnt_n(i) > r
// Exact integers throughout; nothing here rounds.
//
// 1. nr_count_kernel: the host cuts every segment that can be cut at all into work items of R rows, one workgroup of R threads an item,
//    one row i a lane.  A lane keeps its own window id[i .. i + max_n) in registers and the capped run d = min(run(i), max_n, W - i).  The
//    segment's words stream through LDS in chunks of C with a halo; every lane reads the SAME j (a broadcast: no bank conflicts), four
//    words a ds_read_b128, compares the first TWO words -- the shortest match that counts -- and extends only on a hit.  Extending step k
//    adds `still matching` to occ[k], the number of j whose match with the window is longer than k words: occ[n - 1] is occ_n(i) for every
//    n at once, with static register indices.  The extension is straight-line code: its LDS reads leave together and are waited for once.
//    (A looping segment's workgroup extends at every j, and the call waits for the slowest workgroup.  A first version that tested one word
//    and left the unrolled extension through a branch per step took 1.64 ms where this one takes 1.07 ms, profiles/ngram_repeats.txt.)
//    A match never runs past min(W - i, W - j): an n-gram never spans two segments.  The lane's candidate is the smallest n with n > d and
//    occ[n - 1] > r -- the smallest i + n of that row -- packed as ((i + n) * 32 + n) << 32 | count, so that the minimum of the
//    packed keys is the smallest keep, then the smallest n (which fixes i).  The workgroup min-reduces and writes one key per item.
// 2. nr_fold_kernel: one wave per segment.  It min-reduces the segment's item keys, then finds the unigram rule's i0 by run boundaries:
//    position p in [1, W] closes a run when p == W or fold[p] != fold[p - 1]; 64 positions a step, the boundaries as a ballot mask, the
//    previous boundary of a lane from the bits below it or the carry of the steps before.  The first closed run of u words or more is
//    the first such run of the segment, and its full length comes with it.  Lane 0 decides (the unigram rule wins a tie) and writes keep
//    and reason.
// No atomics, one writer per element, no waiting between workgroups; one copy (the tables, into ws, on the stream) and two launches, no
// host read: the call can be captured into a graph.  Results depend neither on the plan nor on the other segments.
#include "host_table.h"
#include <algorithm>
#include <vector>

#define NR_NONE 0xFFFFFFFFFFFFFFFFull
#define NR_HALO 32                                   // words kept behind a chunk: DICOW_NGRAM_MAX_N - 1 of halo + 3 of the 4-word read, rounded up
#define NR_AUTO_PLAN 2                               // plan 0: (64, 1024).  Measured (profiles/ngram_repeats.txt): 64 rows beat 256 by 5 % on a corpus
                                                     // of segments of 30-400 words and equal them at 8000 words; C = 256 and 1024 time alike

struct nr_seg { int64_t start; int32_t W, item0, n_items, pad_; };      // DICOW_NGRAM_SEG_BYTES
struct nr_item { int32_t seg, row0; };                                  // DICOW_NGRAM_ITEM_BYTES
static_assert(sizeof(nr_seg) == DICOW_NGRAM_SEG_BYTES && sizeof(nr_item) == DICOW_NGRAM_ITEM_BYTES, "the header states the tables' sizes");
static_assert(DICOW_NGRAM_MAX_N <= 31 && DICOW_NGRAM_MAX_WORDS < (1 << 26), "the packed key holds n in 5 bits and keep in the 27 above");

struct nr_args {
    const int32_t* ids; const int32_t* fold; const nr_seg* segs; const nr_item* items; unsigned long long* partial;
    int32_t* keep; int32_t* reason;
    int min_n, max_n, min_words, u, r;
};

__device__ __forceinline__ unsigned long long nr_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, 64);
        v = x < v ? x : v;
    }
    return v;
}

template <int R, int C>
__global__ void __launch_bounds__(R) nr_count_kernel(const nr_args a) {
    __shared__ __attribute__((aligned(16))) int32_t s[C + NR_HALO];
    const nr_item it = a.items[blockIdx.x];
    const nr_seg sg = a.segs[it.seg];
    const int W = sg.W;
    const int32_t* id = a.ids + sg.start;
    const int i = it.row0 + (int)threadIdx.x;
    const int mine = min(a.max_n, W - i);            // the longest n-gram that starts at row i
    const bool act = mine >= 2;
    int32_t w[DICOW_NGRAM_MAX_N];
#pragma unroll
    for (int k = 0; k < DICOW_NGRAM_MAX_N; ++k) w[k] = k < mine ? id[i + k] : 0;
    int d = 0;                                       // min(run(i), mine): the n-grams of n <= d words are degenerate
    if (act) {
        const int32_t* fold = a.fold + sg.start;
        const int32_t f0 = fold[i];
        d = 1;
        while (d < mine && fold[i + d] == f0) ++d;
    }
    int occ[DICOW_NGRAM_MAX_N];                      // occ[k], k >= 1: the j whose match with the window is longer than k words
#pragma unroll
    for (int k = 0; k < DICOW_NGRAM_MAX_N; ++k) occ[k] = 0;
    for (int j0 = 0; j0 < W; j0 += C) {
        const int cnt = min(C, W - j0), tot = min(C + NR_HALO, W - j0);
        __syncthreads();                             // the chunk before this one has been read by every wave
        for (int t = (int)threadIdx.x; t < C + NR_HALO; t += R) s[t] = t < tot ? id[j0 + t] : 0;
        __syncthreads();
        for (int jj = 0; jj < cnt && jj + 1 < tot; jj += 4) {      // j = j0 + jj + q <= W - 2: a match of two words, the shortest that counts
            const int4 v = *reinterpret_cast<const int4*>(&s[jj]);
            const int32_t vv[5] = {v.x, v.y, v.z, v.w, s[jj + 4]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (jj + q < cnt && jj + q + 1 < tot && act && vv[q] == w[0] && vv[q + 1] == w[1]) {
                    const int lim = min(mine, W - (j0 + jj + q));
                    int alive = 1;                   // no branch from here on: the reads below leave together and are waited for once
                    ++occ[1];
#pragma unroll
                    for (int k = 2; k < DICOW_NGRAM_MAX_N; ++k) {
                        alive &= (int)(k < lim) & (int)(s[jj + q + k] == w[k]);
                        occ[k] += alive;
                    }
                }
            }
        }
    }
    unsigned long long key = NR_NONE;
    const int lo = max(2, a.min_n);
#pragma unroll
    for (int n = DICOW_NGRAM_MAX_N; n >= 2; --n)
        if (n >= lo && n <= a.max_n && n > d && occ[n - 1] > a.r)
            key = ((unsigned long long)(unsigned)((i + n) * 32 + n) << 32) | (unsigned)occ[n - 1];
    key = nr_wave_min(key);
    if constexpr (R > 64) {
        __shared__ unsigned long long red[R / 64];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int x = 1; x < R / 64; ++x) key = red[x] < key ? red[x] : key;
        }
    }
    if (threadIdx.x == 0) a.partial[blockIdx.x] = key;
}

__global__ void __launch_bounds__(64) nr_fold_kernel(const nr_args a) {
    const nr_seg sg = a.segs[blockIdx.x];
    const int W = sg.W, lane = (int)threadIdx.x;
    unsigned long long key = NR_NONE;
    for (int t = lane; t < sg.n_items; t += 64) {
        const unsigned long long x = a.partial[sg.item0 + t];
        key = x < key ? x : key;
    }
    key = nr_wave_min(key);
    int i0 = -1, run0 = 0;
    if (a.min_n == 1 && W >= a.min_words && W >= a.u) {
        const int32_t* fold = a.fold + sg.start;
        int carry = 0;                               // where the run that is open at `base` began
        for (int base = 0; base < W; base += 64) {
            const int p = base + lane + 1;
            const bool isb = p <= W && (p == W || fold[p] != fold[p - 1]);
            const unsigned long long mask = __ballot(isb);
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const int from = below ? base + (63 - __clzll((long long)below)) + 1 : carry;
            const int run = p - from;
            const unsigned long long hit = __ballot(isb && run >= a.u);
            if (hit) {
                const int src = __ffsll((long long)hit) - 1;
                i0 = __shfl(from, src, 64);
                run0 = __shfl(run, src, 64);
                break;
            }
            if (mask) carry = base + (63 - __clzll((long long)mask)) + 1;
        }
    }
    if (lane == 0) {
        int keep = W, rn = 0, ri = 0, rc = 0;
        if (W >= a.min_words) {
            const int kn = key == NR_NONE ? W : (int)((unsigned)(key >> 32) >> 5);
            if (i0 >= 0 && i0 + 1 < W && i0 + 1 <= kn) { keep = i0 + 1; rn = 1; ri = i0; rc = run0; }
            else if (kn < W) { keep = kn; rn = (int)((unsigned)(key >> 32) & 31u); ri = kn - rn; rc = (int)(unsigned)key; }
        }
        a.keep[blockIdx.x] = keep;
        if (a.reason) {
            a.reason[3 * (int64_t)blockIdx.x] = rn;
            a.reason[3 * (int64_t)blockIdx.x + 1] = ri;
            a.reason[3 * (int64_t)blockIdx.x + 2] = rc;
        }
    }
}

// ---- the host side: the limits, the plan, the work items
struct nr_plan { int R, C; int64_t items, need; };

static inline int64_t nr_up16(int64_t x) { return (x + 15) / 16 * 16; }

// R and C of the call, the most work items any parameters can ask for (every row but the last of every segment) and the workspace for them
static int nr_make_plan(const char* who, const int64_t* table, int n, int plan, nr_plan* out) {
    DICOW_REQUIRE(n >= 0, "%s: negative n=%d", who, n);
    DICOW_REQUIRE(n == 0 || table, "%s: null segment table", who);
    DICOW_REQUIRE(plan >= 0 && plan <= DICOW_NGRAM_PLANS, "%s: plan=%d is none of 0 (the library's choice), 1 .. %d ((R, C) = (64, 256), (64, 1024), "
                  "(256, 256), (256, 1024))", who, plan, DICOW_NGRAM_PLANS);
    for (int k = 0; k < n; ++k) {
        const int64_t W = table[2 * (int64_t)k + 1];
        DICOW_REQUIRE(W >= 0 && W <= DICOW_NGRAM_MAX_WORDS, "%s: segment %d has %lld words, outside [0, DICOW_NGRAM_MAX_WORDS = %d]", who, k, (long long)W,
                      DICOW_NGRAM_MAX_WORDS);
    }
    if (plan == 0) plan = NR_AUTO_PLAN;
    out->R = plan <= 2 ? 64 : 256;
    out->C = plan % 2 ? 256 : 1024;
    out->items = 0;
    for (int k = 0; k < n; ++k) out->items += (std::max<int64_t>(table[2 * (int64_t)k + 1] - 1, 0) + out->R - 1) / out->R;
    out->need = nr_up16((int64_t)n * DICOW_NGRAM_SEG_BYTES + out->items * DICOW_NGRAM_ITEM_BYTES) + out->items * 8;
    DICOW_REQUIRE(out->need <= DICOW_NGRAM_MAX_WS_BYTES, "%s: the tables of %d segments take %lld bytes, past DICOW_NGRAM_MAX_WS_BYTES = %lld (split the call)",
                  who, n, (long long)out->need, (long long)DICOW_NGRAM_MAX_WS_BYTES);
    return DICOW_OK;
}

extern "C" int64_t dicow_ngram_repeats_ws_bytes(const int64_t* table, int n, int plan) {
    nr_plan pl;
    if (nr_make_plan("ngram_repeats_ws_bytes", table, n, plan, &pl) != DICOW_OK) return -1;
    return pl.need;
}

template <int R, int C>
static void nr_launch(int64_t items, hipStream_t st, const nr_args& a) {
    nr_count_kernel<R, C><<<dim3((unsigned)items), R, 0, st>>>(a);
}

extern "C" int dicow_ngram_repeats(const int32_t* ids, const int32_t* fold, int64_t n_words, const int64_t* table, int n, int min_n, int max_n,
                                   int min_words, int unigram_min_repeat, int repeat_threshold, int32_t* keep, int32_t* reason, int plan, void* ws,
                                   int64_t ws_bytes, void* stream) {
    nr_plan pl;
    if (nr_make_plan("ngram_repeats", table, n, plan, &pl) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(n_words >= 0, "ngram_repeats: negative buffer size n_words=%lld", (long long)n_words);
    DICOW_REQUIRE(min_n >= 1, "ngram_repeats: min_n=%d, must be >= 1", min_n);
    DICOW_REQUIRE(max_n <= DICOW_NGRAM_MAX_N, "ngram_repeats: max_n=%d is past DICOW_NGRAM_MAX_N = %d", max_n, DICOW_NGRAM_MAX_N);
    DICOW_REQUIRE(unigram_min_repeat >= 1, "ngram_repeats: unigram_min_repeat=%d, must be >= 1", unigram_min_repeat);
    DICOW_REQUIRE(repeat_threshold >= 0, "ngram_repeats: repeat_threshold=%d, must be >= 0", repeat_threshold);
    // ---- the segment and work item tables, on the host, before anything is launched
    static thread_local std::vector<int64_t> stage;          // the uploaded image: segments, then items
    stage.assign((size_t)(((int64_t)n * DICOW_NGRAM_SEG_BYTES + pl.items * DICOW_NGRAM_ITEM_BYTES) / 8), 0);
    nr_seg* sg = reinterpret_cast<nr_seg*>(stage.data());
    nr_item* it = reinterpret_cast<nr_item*>(sg + n);
    const int lo = std::max(2, min_n);
    int64_t items = 0;
    bool any = false;
    for (int k = 0; k < n; ++k) {
        const int64_t start = table[2 * (int64_t)k], W = table[2 * (int64_t)k + 1];
        DICOW_REQUIRE_SPAN(start, W, n_words, "reads words", "ids of the buffer", "ngram_repeats: segment %d", k);
        any |= W > 0;
        sg[k].start = start;
        sg[k].W = (int32_t)W;
        sg[k].item0 = (int32_t)items;
        // rows [0, W - lo] can start an n-gram; a segment below min_words, or no n in [lo, max_n], leaves nothing to count
        const int64_t rows = (W >= min_words && lo <= max_n) ? std::max<int64_t>(W - lo + 1, 0) : 0;
        sg[k].n_items = (int32_t)((rows + pl.R - 1) / pl.R);
        for (int32_t x = 0; x < sg[k].n_items; ++x) { it[items].seg = k; it[items].row0 = x * pl.R; ++items; }
    }
    if (n == 0) return DICOW_OK;
    DICOW_REQUIRE(keep && ws && ((ids && fold) || !any), "ngram_repeats: null pointer");
    DICOW_REQUIRE(dicow_aligned(4, ids, fold, keep, reason) && dicow_aligned(16, ws),
                  "ngram_repeats: ids / fold / keep / reason not 4-byte or ws not 16-byte aligned");
    DICOW_REQUIRE(ws_bytes >= pl.need, "ngram_repeats: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)pl.need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t tbytes = (int64_t)n * DICOW_NGRAM_SEG_BYTES + items * DICOW_NGRAM_ITEM_BYTES;
    if (int rc = dicow_upload("ngram_repeats", ws, stage.data(), tbytes, st)) return rc;
    nr_args a;
    a.ids = ids; a.fold = fold;
    a.segs = reinterpret_cast<const nr_seg*>(ws);
    a.items = reinterpret_cast<const nr_item*>(a.segs + n);
    a.partial = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + nr_up16(tbytes));
    a.keep = keep; a.reason = reason;
    a.min_n = min_n; a.max_n = max_n; a.min_words = min_words; a.u = unigram_min_repeat; a.r = repeat_threshold;
    if (items > 0) {
        if (pl.R == 64) { if (pl.C == 256) nr_launch<64, 256>(items, st, a); else nr_launch<64, 1024>(items, st, a); }
        else { if (pl.C == 256) nr_launch<256, 256>(items, st, a); else nr_launch<256, 1024>(items, st, a); }
        DICOW_CHECK_LAUNCH("nr_count_kernel");
    }
    nr_fold_kernel<<<dim3((unsigned)n), 64, 0, st>>>(a);
    DICOW_CHECK_LAUNCH("nr_fold_kernel");
    return DICOW_OK;
}

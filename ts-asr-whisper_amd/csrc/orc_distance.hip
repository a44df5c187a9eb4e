// Scoring sessions whose speaker labels are not trusted: meeteval's optimal-reference-combination WER (ORC-WER) and its time-constrained
// form (tcORC-WER; the reference calls them per group of a session, src/utils/wer.py:41-106).  Every reference utterance may go to
// whichever hypothesis stream suits it best.  The definition (include/dicow_hip.h has it in full): a Levenshtein table over the product
// of the H streams, L[j_0, .., j_{H-1}] with 0 <= j_h <= n_h, holding the key of dicow_edit_distance, errors * 2^15 - hits, in int32.
// One utterance of m words: along every axis h every line of L (all other indices fixed) takes m ordinary Levenshtein row updates
// against stream h -- the cell rule and the interval test rb < he && hb < re of csrc/edit_distance.hip -- which gives H candidate tables
// T_h; the new L is their elementwise minimum.  The answer is the corner L[n_0, .., n_{H-1}].
//
// Layout: axis 0 is the contiguous one; the streams of a problem are put on the axes in ascending length (stable), so the contiguous
// axis, whose lines neighbouring lanes read with a stride of n_0 + 1 keys, is the SHORTEST stream.
// Launches: one that fills every L with (sum of j_h) * 2^15, then per utterance step u two -- over all problems that have a u-th
// utterance, found as a prefix of the problems sorted by descending utterance count; a block finds its problem by bisection over the
// problems' first-block numbers -- and one that reads the corners:
//   orc_step_kernel    one lane owns one line of one axis for the whole utterance.  Per chunk of ORC_K words it walks the line once with
//                      a column of ORC_K + 1 keys in registers (the chunk against the current hypothesis word): one read and one write
//                      per cell per chunk, the words cost arithmetic only.  The first chunk reads L and writes T_h, later chunks update
//                      T_h in place (the lane re-reads its own stores).  L is not written here.
//   orc_fold_kernel    one lane per cell: L = min_h T_h.
//   orc_finish_kernel  one lane per problem: (errors, hits) from the corner, or the host's answer for a problem without a table
//                      (no stream: all deleted; no utterance: all inserted).
// With `assignment`: the keys of T_h are int64, key * 2^16 + origin, origin = the index along the line at which the utterance's path
// entered it, so min() also picks the smallest origin among equal keys; orc_fold_kernel takes the stream with the smallest index among
// equal keys and stores (axis << 16 | origin) per cell per step; orc_finish_kernel chases U such records back from the corner.  (errors,
// hits) are the same with and without.  No atomics, no wait on another workgroup: steps are ordered by launch order on the stream.
#include "host_table.h"
#include <algorithm>
#include <vector>

#define ORC_K DICOW_ORC_K
#define ORC_H DICOW_ORC_MAX_STREAMS
#define ORC_LINES 64            // lines (lanes) per block of orc_step_kernel
#define ORC_CELLS 256           // cells (lanes) per block of the init / fold kernels
#define ORC_SHIFT 15

struct orc_prob {               // one problem, in the kernel's order (descending utterance count); axes in ascending stream length
    int64_t L_off, T_off, rec_off;          // bytes from ws: L [S] int32; T [H][S] int32 (int64 with assignment); records [U][S] int32
    int64_t hyp_start[ORC_H];               // per axis
    int32_t n[ORC_H], stride[ORC_H];        // per axis: the stream's words; the distance in cells between neighbours along the axis
    int32_t orig[ORC_H];                    // per axis: the caller's stream index within the problem
    int32_t by_orig[ORC_H];                 // the axes in ascending `orig`
    int32_t line_blk[ORC_H + 1];            // per axis: its first block among the problem's line blocks; [H] = their number
    int32_t H, U, S, utt0, out_idx, line_blk0, cell_blk0, const_e, pad;   // const_e >= 0: no table, the answer is (const_e, 0)
};
static_assert(sizeof(orc_prob) == DICOW_ORC_DESC_BYTES, "DICOW_ORC_DESC_BYTES is the size of a problem's descriptor");

struct orc_utt { int64_t ref_start; int32_t len, row; };                  // row: the caller's utterance row (assignment[row])
static_assert(sizeof(orc_utt) == DICOW_ORC_UTT_BYTES, "DICOW_ORC_UTT_BYTES is the size of an utterance's descriptor");

struct orc_args {
    const int32_t* ref_ids;
    const int32_t* hyp_ids;
    const int32_t* ref_iv;
    const int32_t* hyp_iv;
    const orc_prob* probs;
    const orc_utt* utts;
    char* ws;
    int32_t* out;
    int32_t* assignment;
};

template <bool ASSIGN> struct orc_key { using T = int32_t; static constexpr int32_t ONE = 1; };
template <> struct orc_key<true> { using T = int64_t; static constexpr int64_t ONE = 65536; };

// the last of the first n_act problems whose first block is <= b (problems without blocks never own one: they precede their successor)
template <bool LINE>
__device__ __forceinline__ int orc_find(const orc_prob* __restrict__ probs, int n_act, int b) {
    int lo = 0, hi = n_act - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((LINE ? probs[mid].line_blk0 : probs[mid].cell_blk0) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(ORC_CELLS) orc_init_kernel(const orc_args a, int n_act) {
    const orc_prob& pr = a.probs[orc_find<false>(a.probs, n_act, blockIdx.x)];
    const int cell = (blockIdx.x - pr.cell_blk0) * ORC_CELLS + threadIdx.x;
    if (pr.const_e >= 0 || cell >= pr.S) return;
    int sum = 0;
    for (int ax = 0; ax < pr.H; ++ax) sum += cell / pr.stride[ax] % (pr.n[ax] + 1);
    reinterpret_cast<int32_t*>(a.ws + pr.L_off)[cell] = sum << ORC_SHIFT;
}

template <bool ASSIGN, bool IV>
__global__ void __launch_bounds__(ORC_LINES) orc_step_kernel(const orc_args a, int step, int n_act) {
    using KEY = typename orc_key<ASSIGN>::T;
    constexpr KEY ONE = orc_key<ASSIGN>::ONE, UNIT = ONE << ORC_SHIFT;
    const orc_prob& pr = a.probs[orc_find<true>(a.probs, n_act, blockIdx.x)];
    if (pr.const_e >= 0) return;
    const orc_utt ut = a.utts[pr.utt0 + step];
    const int m = ut.len;
    if (m == 0) return;                                                        // an utterance without words leaves L as it is
    int b = blockIdx.x - pr.line_blk0, ax = 0;
    while (ax + 1 < pr.H && b >= pr.line_blk[ax + 1]) ++ax;
    b -= pr.line_blk[ax];
    const int n = pr.n[ax], st = pr.stride[ax], S = pr.S;
    const int line = b * ORC_LINES + threadIdx.x;
    if (line >= S / (n + 1)) return;
    const int base = line / st * (st * (n + 1)) + line % st;                  // the line's cell at j = 0; its cells: base + j * st < S
    const int32_t* __restrict__ Lt = reinterpret_cast<const int32_t*>(a.ws + pr.L_off);
    KEY* T = reinterpret_cast<KEY*>(a.ws + pr.T_off) + (size_t)ax * S;
    const int32_t* __restrict__ ref = a.ref_ids + ut.ref_start;
    const int32_t* __restrict__ hyp = a.hyp_ids + pr.hyp_start[ax];
    const int32_t* __restrict__ riv = nullptr;
    const int32_t* __restrict__ hiv = nullptr;
    if constexpr (IV) { riv = a.ref_iv + 2 * ut.ref_start; hiv = a.hyp_iv + 2 * pr.hyp_start[ax]; }
    for (int c0 = 0; c0 < m; c0 += ORC_K) {
        const int k = min(ORC_K, m - c0);                                      // rows behind k are computed and never read: values flow down
        int32_t w[ORC_K], rb[ORC_K], re[ORC_K];
#pragma unroll
        for (int i = 0; i < ORC_K; ++i) {
            w[i] = i < k ? ref[c0 + i] : 0;
            if constexpr (IV) {
                rb[i] = i < k ? riv[2 * (c0 + i)] : 0;
                re[i] = i < k ? riv[2 * (c0 + i) + 1] : 0;
            }
        }
        auto load = [&](int j) -> KEY {                                        // row 0 of the chunk at j: L with origin j, or the line so far
            const int cell = base + j * st;
            if (c0 > 0) return T[cell];
            KEY x = (KEY)Lt[cell] * ONE;
            if constexpr (ASSIGN) x += j;
            return x;
        };
        KEY col[ORC_K + 1];                                                    // D[0 .. K][j] of the chunk's table
        KEY x = load(0);
        for (int j = 0; j <= n; ++j) {
            const KEY xn = j < n ? load(j + 1) : 0;                            // one cell ahead (in place: cell j + 1 is read before cell j is written)
            if (j == 0) {
                col[0] = x;
#pragma unroll
                for (int i = 0; i < ORC_K; ++i) col[i + 1] = col[i] + UNIT;
            } else {
                const int32_t hw = hyp[j - 1];
                int32_t hb = 0, he = 0;
                if constexpr (IV) { hb = hiv[2 * (j - 1)]; he = hiv[2 * (j - 1) + 1]; }
                KEY d = col[0];
                col[0] = x;
#pragma unroll
                for (int i = 0; i < ORC_K; ++i) {
                    const KEY left = col[i + 1];                               // D[i + 1][j - 1]
                    const KEY t = min(left, col[i]) + UNIT;
                    const KEY c = d + (w[i] == hw ? -ONE : UNIT);
                    bool open = true;
                    if constexpr (IV) open = rb[i] < he && hb < re[i];
                    col[i + 1] = open ? min(t, c) : t;
                    d = left;
                }
            }
            KEY v = col[1];
#pragma unroll
            for (int i = 2; i <= ORC_K; ++i) v = k == i ? col[i] : v;
            T[base + j * st] = v;
            x = xn;
        }
    }
}

template <bool ASSIGN>
__global__ void __launch_bounds__(ORC_CELLS) orc_fold_kernel(const orc_args a, int step, int n_act) {
    using KEY = typename orc_key<ASSIGN>::T;
    const orc_prob& pr = a.probs[orc_find<false>(a.probs, n_act, blockIdx.x)];
    if (pr.const_e >= 0 || a.utts[pr.utt0 + step].len == 0) return;
    const int S = pr.S, cell = (blockIdx.x - pr.cell_blk0) * ORC_CELLS + threadIdx.x;
    if (cell >= S) return;
    const KEY* __restrict__ T = reinterpret_cast<const KEY*>(a.ws + pr.T_off);
    int best_ax = pr.by_orig[0];
    KEY best = T[(size_t)best_ax * S + cell];
    for (int q = 1; q < pr.H; ++q) {
        const int ax = pr.by_orig[q];
        const KEY v = T[(size_t)ax * S + cell];
        const bool less = ASSIGN ? (v >> 16) < (best >> 16) : v < best;        // the key alone: among equal keys the first stream stays
        best_ax = less ? ax : best_ax;
        best = less ? v : best;
    }
    int32_t* Lt = reinterpret_cast<int32_t*>(a.ws + pr.L_off);
    if constexpr (ASSIGN) {
        Lt[cell] = (int32_t)(best >> 16);
        reinterpret_cast<int32_t*>(a.ws + pr.rec_off)[(size_t)step * S + cell] = best_ax << 16 | (int32_t)(best & 0xffff);
    } else {
        Lt[cell] = best;
    }
}

template <bool ASSIGN>
__global__ void __launch_bounds__(64) orc_finish_kernel(const orc_args a, int n_problems) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_problems) return;
    const orc_prob& pr = a.probs[p];
    int32_t* out = a.out + 2 * (int64_t)pr.out_idx;
    if (pr.const_e >= 0) {
        out[0] = pr.const_e;
        out[1] = 0;
        if constexpr (ASSIGN)
            for (int u = 0; u < pr.U; ++u) a.assignment[a.utts[pr.utt0 + u].row] = pr.H > 0 ? 0 : -1;
        return;
    }
    const int32_t v = reinterpret_cast<const int32_t*>(a.ws + pr.L_off)[pr.S - 1];
    const int32_t e = (v + ((1 << ORC_SHIFT) - 1)) >> ORC_SHIFT;               // v = E 2^15 - hits, 0 <= hits < 2^15
    out[0] = e;
    out[1] = (e << ORC_SHIFT) - v;
    if constexpr (ASSIGN) {
        const int32_t* __restrict__ rec = reinterpret_cast<const int32_t*>(a.ws + pr.rec_off);
        int cell = pr.S - 1;
        for (int u = pr.U - 1; u >= 0; --u) {
            const orc_utt ut = a.utts[pr.utt0 + u];
            if (ut.len == 0) { a.assignment[ut.row] = 0; continue; }
            const int32_t r = rec[(size_t)u * pr.S + cell];
            const int ax = r >> 16, origin = r & 0xffff;
            a.assignment[ut.row] = pr.orig[ax];
            cell -= (cell / pr.stride[ax] % (pr.n[ax] + 1) - origin) * pr.stride[ax];
        }
    }
}

// ---- the host's plan: every check, the descriptors and the workspace layout, before anything is launched
struct orc_plan {
    std::vector<int64_t> stage;            // the uploaded image: [n] orc_prob, then the utterances' orc_utt in the same order
    std::vector<int> line_end, cell_end;   // blocks of the first q + 1 problems
    std::vector<int> n_act;                // [step]: problems with an utterance at that step (a prefix of the kernel's order)
    int64_t head_bytes = 0, need = 0;
};

static inline int64_t orc_r8(int64_t b) { return (b + 7) / 8 * 8; }

// n_ref / n_hyp < 0: sizes only (the spans are not checked)
static int orc_make_plan(const char* who, const int64_t* problems, int n, const int64_t* utts, const int64_t* streams, int want_assignment,
                         int64_t n_ref, int64_t n_hyp, orc_plan& pl) {
    DICOW_REQUIRE(n >= 0, "%s: negative n_problems=%d", who, n);
    DICOW_REQUIRE(n == 0 || problems, "%s: null problem table", who);
    const bool spans = n_ref >= 0 && n_hyp >= 0;
    int64_t total_utts = 0;
    std::vector<int> order((size_t)n);
    std::vector<int64_t> steps((size_t)n);                                     // utterance steps a problem takes part in (0 without a table)
    for (int k = 0; k < n; ++k) {
        const int64_t* row = problems + 4 * (int64_t)k;
        DICOW_REQUIRE(row[0] >= 0 && row[1] >= 0 && row[2] >= 0 && row[3] >= 0 && row[0] <= INT32_MAX - row[1] && row[2] <= INT32_MAX - row[3] &&
                      row[1] <= INT32_MAX, "%s: problem %d has a negative or oversized row range (utt_first=%lld, n_utts=%lld, stream_first=%lld, "
                      "n_streams=%lld)", who, k, (long long)row[0], (long long)row[1], (long long)row[2], (long long)row[3]);
        DICOW_REQUIRE(row[3] <= ORC_H, "%s: problem %d has %lld streams, more than DICOW_ORC_MAX_STREAMS = %d", who, k, (long long)row[3], ORC_H);
        DICOW_REQUIRE((row[1] == 0 || utts) && (row[3] == 0 || streams), "%s: null utterance or stream table", who);
        total_utts += row[1];
        order[k] = k;
        steps[k] = row[3] > 0 ? row[1] : 0;
    }
    DICOW_REQUIRE(total_utts <= INT32_MAX, "%s: %lld utterances in one call", who, (long long)total_utts);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return steps[x] > steps[y]; });
    pl.head_bytes = (int64_t)n * (int64_t)sizeof(orc_prob) + total_utts * (int64_t)sizeof(orc_utt);
    DICOW_REQUIRE(pl.head_bytes <= DICOW_ORC_MAX_WS_BYTES, "%s: the descriptors of %d problems and %lld utterances take more than DICOW_ORC_MAX_WS_BYTES = "
                  "%lld bytes", who, n, (long long)total_utts, (long long)DICOW_ORC_MAX_WS_BYTES);
    pl.stage.assign((size_t)(pl.head_bytes / 8), 0);
    pl.line_end.assign((size_t)n, 0);
    pl.cell_end.assign((size_t)n, 0);
    pl.n_act.assign((size_t)(n ? steps[order[0]] : 0), 0);
    orc_prob* probs = reinterpret_cast<orc_prob*>(pl.stage.data());
    orc_utt* ut = reinterpret_cast<orc_utt*>(pl.stage.data() + (size_t)n * (sizeof(orc_prob) / 8));
    int64_t need = pl.head_bytes, line_blocks = 0, cell_blocks = 0;
    int utt0 = 0;
    std::vector<std::pair<int64_t, int64_t>> rows;                             // utterance row ranges, for the assignment's one-writer rule
    for (int q = 0; q < n; ++q) {
        const int k = order[q];
        const int64_t* row = problems + 4 * (int64_t)k;
        const int U = (int)row[1], H = (int)row[3];
        orc_prob& pr = probs[q];
        pr.H = H; pr.U = U; pr.utt0 = utt0; pr.out_idx = k;
        pr.line_blk0 = (int32_t)line_blocks; pr.cell_blk0 = (int32_t)cell_blocks;
        int64_t words = 0, hyp_words = 0;
        for (int u = 0; u < U; ++u) {
            const int64_t* r = utts + 2 * (row[0] + u);
            DICOW_REQUIRE(r[1] >= 0, "%s: utterance %d of problem %d has a negative length %lld", who, u, k, (long long)r[1]);
            DICOW_REQUIRE(r[1] <= DICOW_ORC_MAX_WORDS, "%s: utterance %d of problem %d has %lld words, more than DICOW_ORC_MAX_WORDS = %d", who, u, k,
                          (long long)r[1], DICOW_ORC_MAX_WORDS);
            if (spans) DICOW_REQUIRE_SPAN(r[0], r[1], n_ref, "reads ref", "ids of the buffer", "%s: utterance %d of problem %d", who, u, k);
            ut[utt0 + u].ref_start = r[0];
            ut[utt0 + u].len = (int32_t)r[1];
            ut[utt0 + u].row = (int32_t)(row[0] + u);
            words += r[1];
        }
        utt0 += U;
        if (U > 0) rows.emplace_back(row[0], row[0] + U);
        int axes[ORC_H];
        for (int h = 0; h < H; ++h) {
            const int64_t* r = streams + 2 * (row[2] + h);
            DICOW_REQUIRE(r[1] >= 0, "%s: stream %d of problem %d has a negative length %lld", who, h, k, (long long)r[1]);
            DICOW_REQUIRE(r[1] <= DICOW_ORC_MAX_WORDS, "%s: stream %d of problem %d has %lld words, more than DICOW_ORC_MAX_WORDS = %d", who, h, k,
                          (long long)r[1], DICOW_ORC_MAX_WORDS);
            if (spans) DICOW_REQUIRE_SPAN(r[0], r[1], n_hyp, "reads hyp", "ids of the buffer", "%s: stream %d of problem %d", who, h, k);
            hyp_words += r[1];
            axes[h] = h;
        }
        DICOW_REQUIRE(words + hyp_words <= DICOW_ORC_MAX_WORDS, "%s: problem %d has %lld reference + %lld hypothesis words, more than "
                      "DICOW_ORC_MAX_WORDS = %d (the int32 key)", who, k, (long long)words, (long long)hyp_words, DICOW_ORC_MAX_WORDS);
        pr.const_e = H == 0 ? (int32_t)words : U == 0 ? (int32_t)hyp_words : -1;
        if (pr.const_e >= 0) {
            pl.line_end[q] = (int)line_blocks;
            pl.cell_end[q] = (int)cell_blocks;
            continue;
        }
        std::stable_sort(axes, axes + H, [&](int x, int y) { return streams[2 * (row[2] + x) + 1] < streams[2 * (row[2] + y) + 1]; });
        int64_t S = 1;
        for (int ax = 0; ax < H; ++ax) {
            const int64_t* r = streams + 2 * (row[2] + axes[ax]);
            pr.hyp_start[ax] = r[0];
            pr.n[ax] = (int32_t)r[1];
            pr.stride[ax] = (int32_t)S;
            pr.orig[ax] = axes[ax];
            S *= r[1] + 1;
            DICOW_REQUIRE(S <= DICOW_ORC_MAX_STATES, "%s: problem %d has more than DICOW_ORC_MAX_STATES = %d states (the product of its streams' "
                          "lengths + 1)", who, k, DICOW_ORC_MAX_STATES);
        }
        for (int ax = 0; ax < H; ++ax) pr.by_orig[pr.orig[ax]] = ax;
        pr.S = (int32_t)S;
        int blk = 0;
        for (int ax = 0; ax < H; ++ax) {
            pr.line_blk[ax] = blk;
            blk += (int)((S / (pr.n[ax] + 1) + ORC_LINES - 1) / ORC_LINES);
        }
        pr.line_blk[H] = blk;
        line_blocks += blk;
        cell_blocks += (S + ORC_CELLS - 1) / ORC_CELLS;
        pl.line_end[q] = (int)line_blocks;
        pl.cell_end[q] = (int)cell_blocks;
        pr.L_off = need;
        need += orc_r8(4 * S);
        pr.T_off = need;
        need += (int64_t)H * S * (want_assignment ? 8 : 4);
        need = orc_r8(need);
        if (want_assignment) { pr.rec_off = need; need += orc_r8(4 * S * U); }
        DICOW_REQUIRE(need <= DICOW_ORC_MAX_WS_BYTES, "%s: the tables%s up to problem %d take more than DICOW_ORC_MAX_WS_BYTES = %lld bytes", who,
                      want_assignment ? " and the assignment's records" : "", k, (long long)DICOW_ORC_MAX_WS_BYTES);
        for (int u = 0; u < U; ++u) pl.n_act[u] = q + 1;
    }
    if (want_assignment) {
        std::sort(rows.begin(), rows.end());
        for (size_t i = 1; i < rows.size(); ++i)
            DICOW_REQUIRE(rows[i].first >= rows[i - 1].second, "%s: with an assignment two problems may not share utterance row %lld", who,
                          (long long)rows[i].first);
    }
    pl.need = need;
    return DICOW_OK;
}

extern "C" int64_t dicow_orc_distance_ws_bytes(const int64_t* problems, int n_problems, const int64_t* utts, const int64_t* streams,
                                               int want_assignment) {
    orc_plan pl;
    if (orc_make_plan("orc_distance_ws_bytes", problems, n_problems, utts, streams, want_assignment, -1, -1, pl) != DICOW_OK) return -1;
    return pl.need;
}

template <bool ASSIGN, bool IV>
static void orc_launch(const orc_plan& pl, int n, hipStream_t st, const orc_args& a) {
    if (pl.cell_end[n - 1] > 0) orc_init_kernel<<<dim3((unsigned)pl.cell_end[n - 1]), ORC_CELLS, 0, st>>>(a, n);
    for (size_t u = 0; u < pl.n_act.size(); ++u) {
        const int act = pl.n_act[u];
        orc_step_kernel<ASSIGN, IV><<<dim3((unsigned)pl.line_end[act - 1]), ORC_LINES, 0, st>>>(a, (int)u, act);
        orc_fold_kernel<ASSIGN><<<dim3((unsigned)pl.cell_end[act - 1]), ORC_CELLS, 0, st>>>(a, (int)u, act);
    }
    orc_finish_kernel<ASSIGN><<<dim3((unsigned)((n + 63) / 64)), 64, 0, st>>>(a, n);
}

extern "C" int dicow_orc_distance(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv,
                                  const int32_t* hyp_iv, const int64_t* problems, int n_problems, const int64_t* utts, const int64_t* streams,
                                  int32_t* out, int32_t* assignment, void* ws, int64_t ws_bytes, void* stream) {
    if (int rc = dicow_check_id_buffers("orc_distance", n_ref, n_hyp, ref_iv, hyp_iv)) return rc;
    static thread_local orc_plan pl;                         // pl.stage is the uploaded image
    if (orc_make_plan("orc_distance", problems, n_problems, utts, streams, assignment != nullptr, n_ref, n_hyp, pl) != DICOW_OK)
        return DICOW_ERR_INVALID;
    if (n_problems == 0) return DICOW_OK;
    bool any_ref = false, any_hyp = false;
    const orc_prob* probs = reinterpret_cast<const orc_prob*>(pl.stage.data());
    const orc_utt* ut = reinterpret_cast<const orc_utt*>(probs + n_problems);
    for (int q = 0; q < n_problems; ++q) {
        if (probs[q].const_e >= 0) continue;                 // a problem without a table reads no ids
        for (int ax = 0; ax < probs[q].H; ++ax) any_hyp |= probs[q].n[ax] > 0;
        for (int u = 0; u < probs[q].U; ++u) any_ref |= ut[probs[q].utt0 + u].len > 0;
    }
    DICOW_REQUIRE(out && ws && (ref_ids || !any_ref) && (hyp_ids || !any_hyp), "orc_distance: null pointer");
    DICOW_REQUIRE(dicow_aligned(4, ref_ids, hyp_ids, ref_iv, hyp_iv, out, assignment) && dicow_aligned(8, ws),
                  "orc_distance: ids / intervals / out / assignment not 4-byte or ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= pl.need, "orc_distance: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)pl.need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dicow_upload("orc_distance", ws, pl.stage.data(), pl.head_bytes, st)) return rc;
    orc_args a;
    a.ref_ids = ref_ids; a.hyp_ids = hyp_ids; a.ref_iv = ref_iv; a.hyp_iv = hyp_iv;
    a.probs = reinterpret_cast<const orc_prob*>(ws);
    a.utts = reinterpret_cast<const orc_utt*>(static_cast<char*>(ws) + (int64_t)n_problems * (int64_t)sizeof(orc_prob));
    a.ws = static_cast<char*>(ws);
    a.out = out;
    a.assignment = assignment;
    if (assignment) { if (ref_iv) orc_launch<true, true>(pl, n_problems, st, a); else orc_launch<true, false>(pl, n_problems, st, a); }
    else { if (ref_iv) orc_launch<false, true>(pl, n_problems, st, a); else orc_launch<false, false>(pl, n_problems, st, a); }
    DICOW_CHECK_LAUNCH("orc_distance kernels");
    return DICOW_OK;
}

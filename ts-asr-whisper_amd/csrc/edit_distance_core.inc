// The skewed-pipeline Levenshtein kernel shared by edit_distance.hip (counts) and edit_alignment.hip (counts + the step every cell took),
// with the host pieces both entry points use.  The algorithm is described at the top of edit_distance.hip.  REC = false is the kernel
// dicow_edit_distance launches; everything recording adds sits behind `if constexpr (REC)`.
//
// REC = true: beside the keys, lane t packs the step of each of its ED_K cells of a row into one 16-bit word, 2 bits per cell --
// 0 hit, 1 substitution, 2 deletion (a reference word without partner), 3 insertion (a hypothesis word without partner) -- the first of
// diagonal (if open), deletion, insertion that attains the cell's key.  Rows are the reference when cols_hyp is set, so `up` is then the
// deletion and `left` the insertion, and the other way round otherwise: the code does not depend on which sequence lies along the lanes.
// The words are stored as the lanes produce them, skewed: panel p, step s, lane t at  rec[p * T * LANES + s * W + t],  T = n + LANES - 1,
// W = the strips of the panel that hold a column <= m (LANES for every panel but the last), so one step's store is one coalesced row of W
// words.  Only rows 0 <= s - t < n of lanes t < W are written.
#pragma once
#include "host_table.h"
#include <algorithm>
#include <type_traits>
#include <vector>

#define ED_K DICOW_EDIT_K
#define ED_WIDE DICOW_EDIT_LANES
#define ED_NARROW DICOW_EDIT_LANES_NARROW
#define ED_I32_MAX_SUM (65535 - ED_WIDE * ED_K)

struct ed_pair { int64_t col_start, row_start, bnd_off; int32_t m, n, cols_hyp, pad; };      // bnd_off: bytes from ws to the pair's [2][n] keys

struct ed_args {
    const int32_t* ref_ids;
    const int32_t* hyp_ids;
    const int32_t* ref_iv;
    const int32_t* hyp_iv;
    const ed_pair* pairs;
    char* ws;
    int32_t* out;
};

struct ea_pair { int64_t rec_off, slot_end; };       // bytes from ws to the pair's records; the byte index in ops behind the pair's slot

struct ea_args : ed_args {
    const ea_pair* xp;
    uint8_t* ops;
    int64_t* spans;
};

template <bool REC> struct ed_args_of { using type = ed_args; };
template <> struct ed_args_of<true> { using type = ea_args; };

template <typename KEY> struct ed_unit;
template <> struct ed_unit<int32_t> { static constexpr int SHIFT = 15; };
template <> struct ed_unit<int64_t> { static constexpr int SHIFT = 32; };

// what flows from lane to lane: the key right of a strip, and the row it belongs to
template <typename KEY, bool IV> struct ed_msg { KEY key; int32_t sym; };
template <typename KEY> struct ed_msg<KEY, true> { KEY key; int32_t sym, ib, ie; };

template <typename KEY, bool IV, int LANES, bool REC = false>
__global__ void __launch_bounds__(LANES) edit_distance_kernel(const typename ed_args_of<REC>::type a) {
    using MSG = ed_msg<KEY, IV>;
    constexpr KEY UNIT = (KEY)1 << ed_unit<KEY>::SHIFT;
    constexpr int P = LANES * ED_K;
    __shared__ MSG hand[2][LANES];
    __shared__ MSG stage_in[LANES];
    __shared__ KEY stage_out[2][LANES];
    const int t = threadIdx.x;
    const ed_pair pr = a.pairs[blockIdx.x];
    const int m = pr.m, n = pr.n;
    int32_t* out = a.out + 2 * (int64_t)blockIdx.x;
    if (m == 0 || n == 0) {
        if (t == 0) { out[0] = m + n; out[1] = 0; }
        return;
    }
    const int32_t* col_ids = (pr.cols_hyp ? a.hyp_ids : a.ref_ids) + pr.col_start;
    const int32_t* row_ids = (pr.cols_hyp ? a.ref_ids : a.hyp_ids) + pr.row_start;
    const int32_t* col_iv = nullptr;
    const int32_t* row_iv = nullptr;
    if constexpr (IV) {
        col_iv = (pr.cols_hyp ? a.hyp_iv : a.ref_iv) + 2 * pr.col_start;
        row_iv = (pr.cols_hyp ? a.ref_iv : a.hyp_iv) + 2 * pr.row_start;
    }
    KEY* bnd = reinterpret_cast<KEY*>(a.ws + pr.bnd_off);
    const int panels = (m + P - 1) / P;
    const int T = n + LANES - 1;                                               // steps of a panel
    uint16_t* rec = nullptr;                                                   // REC: this panel's records, and its row width
    int rec_w = 0;
    KEY cur[ED_K];
    for (int p = 0; p < panels; ++p) {
        const int j0 = p * P + t * ED_K;                                       // the strip's first column (0-based; D's column j0 + 1)
        const bool has_in = p > 0, has_out = p + 1 < panels;
        const KEY* bin = bnd + (size_t)((p + 1) & 1) * n;                      // the previous panel's last column, rows 1 .. n
        KEY* bout = bnd + (size_t)(p & 1) * n;
        if constexpr (REC) {
            rec = reinterpret_cast<uint16_t*>(a.ws + a.xp[blockIdx.x].rec_off) + (int64_t)p * T * LANES;
            rec_w = min(LANES, (m - p * P + ED_K - 1) / ED_K);
        }
        int32_t asym[ED_K], ab[ED_K], ae[ED_K];
#pragma unroll
        for (int k = 0; k < ED_K; ++k) {
            const int j = j0 + k;
            cur[k] = (KEY)min(j + 1, m) * UNIT;                                // D[0][j + 1]
            asym[k] = j < m ? col_ids[j] : 0;
            if constexpr (IV) {
                ab[k] = j < m ? col_iv[2 * j] : 0;
                ae[k] = j < m ? col_iv[2 * j + 1] : 0;
            }
        }
        KEY diag = (KEY)min(j0, m) * UNIT;                                     // D[0][j0]
        auto load_row = [&](int r) {                                           // lane 0's message for row r (0-based)
            MSG g;
            g.key = 0; g.sym = 0;
            if constexpr (IV) { g.ib = 0; g.ie = 0; }
            if (r < n) {
                g.key = has_in ? bin[r] : (KEY)(r + 1) * UNIT;
                g.sym = row_ids[r];
                if constexpr (IV) { g.ib = row_iv[2 * r]; g.ie = row_iv[2 * r + 1]; }
            }
            return g;
        };
        auto flush = [&](int sf) {                                             // the last lane's keys of steps sf .. sf + LANES - 1
            const int r = sf + t - (LANES - 1);
            if (r >= 0 && r < n) bout[r] = stage_out[(sf / LANES) & 1][t];
        };
        MSG pre = load_row(t);
        for (int s0 = 0; s0 < T; s0 += LANES) {
            if (has_out && s0 > 0) flush(s0 - LANES);
            stage_in[t] = pre;                                                 // read by lane 0 at step s0 + t: behind the barrier of step s0
            pre = load_row(s0 + LANES + t);
            const int s1 = min(s0 + LANES, T);
            for (int s = s0; s < s1; ++s) {
                const int r = s - t;
                const MSG in = t == 0 ? stage_in[s - s0] : hand[(s + 1) & 1][t - 1];
                if (r >= 0 && r < n) {
                    // v[k] = min(a[k], v[k - 1] + UNIT), a[k] = min(up + UNIT, diagonal step).  With everything of column k lowered
                    // by k UNIT the chain along the strip is one min per cell; the rest has no dependence from cell to cell.
                    KEY d = diag, a[ED_K];
                    KEY via_up[ED_K], via_diag[ED_K];                          // REC: the candidates, lowered like a[]; via_diag is
                    uint32_t sub[ED_K];                                        // up + 1 (never attained) where the diagonal is closed
                    diag = in.key;
#pragma unroll
                    for (int k = 0; k < ED_K; ++k) {
                        const KEY up = cur[k];
                        const KEY c = d + (asym[k] == in.sym ? (KEY)-1 - k * UNIT : UNIT - k * UNIT);
                        const KEY x = up + (UNIT - k * UNIT);
                        bool open = true;
                        if constexpr (IV) open = in.ib < ae[k] && ab[k] < in.ie;
                        a[k] = open ? min(x, c) : x;
                        if constexpr (REC) {
                            via_up[k] = x;
                            via_diag[k] = open ? c : x + 1;
                            sub[k] = asym[k] == in.sym ? 0u : 1u;
                        }
                        d = up;
                    }
                    KEY run = in.key + UNIT;
                    uint32_t w = 0;
#pragma unroll
                    for (int k = 0; k < ED_K; ++k) {
                        const KEY left = run;                                  // the cell left of this one, + UNIT, lowered
                        run = min(run, a[k]);
                        cur[k] = run + k * UNIT;
                        if constexpr (REC) {                                   // the first of diagonal, deletion, insertion that attains run
                            const KEY deletion = pr.cols_hyp ? via_up[k] : left;
                            w |= (via_diag[k] == run ? sub[k] : deletion == run ? 2u : 3u) << (2 * k);
                        }
                    }
                    if constexpr (REC) {
                        if (t < rec_w) rec[(int64_t)s * rec_w + t] = (uint16_t)w;
                    }
                }
                MSG o = in;
                o.key = cur[ED_K - 1];
                hand[s & 1][t] = o;
                if (has_out && t == LANES - 1) stage_out[(s0 / LANES) & 1][s - s0] = cur[ED_K - 1];
                __syncthreads();
            }
        }
        if (has_out) flush((T - 1) / LANES * LANES);
        __syncthreads();                                                       // the column is visible to the next panel's loads
    }
    const int q = m - 1 - (panels - 1) * P;                                    // column m in the last panel
    if (t == q / ED_K) {
        KEY v = cur[0];
#pragma unroll
        for (int k = 1; k < ED_K; ++k) v = (q % ED_K == k) ? cur[k] : v;
        const KEY e = (v + (UNIT - 1)) >> ed_unit<KEY>::SHIFT;                 // v = E UNIT - H, 0 <= H < UNIT
        out[0] = (int32_t)e;
        out[1] = (int32_t)(e * UNIT - v);
    }
}

// ---- the host half: one plan and one launcher for both entry points
static_assert(sizeof(ed_pair) + sizeof(ea_pair) == DICOW_ALIGN_TABLE_BYTES, "the header states the tables' size");

static inline int64_t ed_steps(int64_t m, int64_t n, int lanes) { return (m + (int64_t)lanes * ED_K - 1) / ((int64_t)lanes * ED_K) * (n + lanes - 1); }

static inline int64_t ed_bnd_bytes(int64_t ref_len, int64_t hyp_len) {        // two columns of 8-byte slots when some plan may need a second panel
    const int64_t longer = std::max(ref_len, hyp_len);
    return longer > (int64_t)ED_NARROW * ED_K ? 16 * longer : 0;
}

static inline int64_t ed_rec_bytes(int64_t m, int64_t n, int lanes) {
    if (m == 0 || n == 0) return 0;
    const int64_t P = (int64_t)lanes * ED_K, panels = (m + P - 1) / P, w = (m - (panels - 1) * P + ED_K - 1) / ED_K;
    return (2 * ((panels - 1) * (n + lanes - 1) * lanes + (n + w - 1) * w) + 7) / 8 * 8;
}

static inline int ed_check_lens(const char* who, const int64_t* pairs, int n_pairs) {
    DICOW_REQUIRE(n_pairs >= 0, "%s: negative n_pairs=%d", who, n_pairs);
    DICOW_REQUIRE(n_pairs == 0 || pairs, "%s: null pair table", who);
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t rl = pairs[4 * (int64_t)k + 1], hl = pairs[4 * (int64_t)k + 3];
        DICOW_REQUIRE(rl >= 0 && hl >= 0, "%s: pair %d has a negative length (ref_len=%lld, hyp_len=%lld)", who, k, (long long)rl, (long long)hl);
        DICOW_REQUIRE(rl <= DICOW_EDIT_MAX_LEN && hl <= DICOW_EDIT_MAX_LEN, "%s: pair %d is longer (ref_len=%lld, hyp_len=%lld) than DICOW_EDIT_MAX_LEN = %d",
                      who, k, (long long)rl, (long long)hl, DICOW_EDIT_MAX_LEN);
    }
    return DICOW_OK;
}

// The call's plan, shared by the size queries and the entry points: the workgroup width, the key, which sequence of each pair lies along
// the lanes, and the workspace laid out as [n_pairs] ed_pair, the boundary columns -- or, with rec, as [n_pairs] ed_pair, [n_pairs]
// ea_pair, the boundary columns, the records.  image: null, or where to build the uploaded tables (the first table_bytes of the workspace).
struct ed_plan { int lanes; bool key64, any_ref, any_hyp; int64_t table_bytes, need; };

static int ed_make_plan(const char* who, const int64_t* pairs, int n_pairs, int lanes, int along, bool rec, std::vector<int64_t>* image, ed_plan* plan) {
    if (ed_check_lens(who, pairs, n_pairs) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(lanes == 0 || lanes == ED_NARROW || lanes == ED_WIDE, "%s: lanes=%d is none of 0, %d, %d", who, lanes, ED_NARROW, ED_WIDE);
    DICOW_REQUIRE(along >= 0 && along <= 2, "%s: along=%d is none of 0 (the library's choice), 1 (ref along the lanes), 2 (hyp)", who, along);
    bool wide = lanes == ED_WIDE;
    plan->key64 = plan->any_ref = plan->any_hyp = false;
    plan->table_bytes = (int64_t)n_pairs * (int64_t)(sizeof(ed_pair) + (rec ? sizeof(ea_pair) : 0));
    int64_t need = plan->table_bytes;                                           // behind the boundary columns: where the records begin
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        if (lanes == 0 && std::min(row[1], row[3]) > (int64_t)ED_NARROW * ED_K) wide = true;
        plan->key64 |= row[1] + row[3] > ED_I32_MAX_SUM;
        plan->any_ref |= row[1] > 0;
        plan->any_hyp |= row[3] > 0;
        need += ed_bnd_bytes(row[1], row[3]);
    }
    const int L = plan->lanes = wide ? ED_WIDE : ED_NARROW;
    plan->need = need;
    if (!rec && !image) return DICOW_OK;                                        // the counts' size query: nothing more to lay out
    if (image) image->assign((size_t)plan->table_bytes / 8, 0);
    ed_pair* e = image ? reinterpret_cast<ed_pair*>(image->data()) : nullptr;
    ea_pair* x = e && rec ? reinterpret_cast<ea_pair*>(e + n_pairs) : nullptr;
    int64_t bnd_off = plan->table_bytes, slot = 0;
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        const bool cols_hyp = along == 2 || (along == 0 && ed_steps(row[3], row[1], L) < ed_steps(row[1], row[3], L));
        const int64_t m = cols_hyp ? row[3] : row[1], n = cols_hyp ? row[1] : row[3];
        if (e) {
            e[k].col_start = cols_hyp ? row[2] : row[0];
            e[k].row_start = cols_hyp ? row[0] : row[2];
            e[k].m = (int32_t)m;
            e[k].n = (int32_t)n;
            e[k].cols_hyp = cols_hyp;
            e[k].bnd_off = bnd_off;
        }
        bnd_off += ed_bnd_bytes(row[1], row[3]);
        if (!rec) continue;
        slot += row[1] + row[3];
        if (x) { x[k].rec_off = need; x[k].slot_end = slot; }
        need += ed_rec_bytes(m, n, L);
        DICOW_REQUIRE(need <= DICOW_ALIGN_MAX_WS_BYTES, "%s: the records up to pair %d of %d bring the workspace to %lld bytes, past "
                      "DICOW_ALIGN_MAX_WS_BYTES = %lld (split the call)", who, k, n_pairs, (long long)need, (long long)DICOW_ALIGN_MAX_WS_BYTES);
    }
    plan->need = need;
    return DICOW_OK;
}

// What both entry points refuse once the plan stands: bad id buffers, a pair that reads past them.
static int ed_check_buffers(const char* who, const int64_t* pairs, int n_pairs, int64_t n_ref, int64_t n_hyp, const int32_t* ref_iv, const int32_t* hyp_iv) {
    if (int rc = dicow_check_id_buffers(who, n_ref, n_hyp, ref_iv, hyp_iv)) return rc;
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        DICOW_REQUIRE_SPAN(row[0], row[1], n_ref, "reads ref", "ids of the buffer", "%s: pair %d", who, k);
        DICOW_REQUIRE_SPAN(row[2], row[3], n_hyp, "reads hyp", "ids of the buffer", "%s: pair %d", who, k);
    }
    return DICOW_OK;
}

// The table kernel of the plan: key width x intervals x lanes.
template <bool REC>
static void ed_launch(const ed_plan& plan, int n_pairs, hipStream_t st, const typename ed_args_of<REC>::type& a) {
    auto go = [&](auto key, auto iv) {
        using KEY = decltype(key);
        constexpr bool IV = decltype(iv)::value;
        if (plan.lanes == ED_WIDE) edit_distance_kernel<KEY, IV, ED_WIDE, REC><<<dim3((unsigned)n_pairs), ED_WIDE, 0, st>>>(a);
        else edit_distance_kernel<KEY, IV, ED_NARROW, REC><<<dim3((unsigned)n_pairs), ED_NARROW, 0, st>>>(a);
    };
    if (plan.key64) { if (a.ref_iv) go(int64_t{}, std::true_type{}); else go(int64_t{}, std::false_type{}); }
    else { if (a.ref_iv) go(int32_t{}, std::true_type{}); else go(int32_t{}, std::false_type{}); }
}


// Sequence bias and banned phrases on next-token scores (dicow_sequence_bias; definition in include/dicow_hip.h).
//
// transformers' SequenceBiasLogitsProcessor (NoBadWordsLogitsProcessor is the same rule with a bias of -inf) walks the sequences in a
// Python loop of four device ops each, and adds a full [rows, V] bias tensor to the scores at the end.  Here the sequences sit in a
// device table sorted into groups of equal last token -- the one score element a group can touch -- and one launch covers every
// (row, group):
//   * matching is the parallel part: a sequence of m tokens matches when the last m - 1 history ids equal its first m - 1 tokens.  The
//     comparison runs from the last history id backwards, so nearly every sequence is dropped on its first comparison.  The row's last
//     max_len - 1 ids are staged once per workgroup in LDS (clamped to int32, -1 for an id outside [0, V): table tokens are >= 0, so
//     such an id never matches); every lane starts at hist[0], an LDS broadcast read;
//   * the sum over a group's matching sequences is the ordered part: b = +0.0f, then b = b + bias_s in table order, one rounding per
//     add, and ONE lane adds b to scores[r, v].  Groups have distinct last tokens, so every score element has one writer: no atomics,
//     no workspace, and the result is a function of the row's history and the table alone, whatever the plan.
// Plans: DICOW_SEQ_BIAS_LANE -- a lane per group, which walks its group's sequences itself (groups are short: a hotword list has
// nearly as many last tokens as entries); DICOW_SEQ_BIAS_WAVE -- a wave per group: 64 sequences are matched at a time, the matches
// are balloted and added in lane order (the ballot is wave-uniform, so is the sum; lane 0 writes).  It serves groups of hundreds of
// sequences, where one lane would walk them all.
#include "common.h"

#define SQB_BLOCK 256
#define SQB_WAVES (SQB_BLOCK / DICOW_WAVE)

struct sqb_table {
    const int* seq_off;      // [n_seq + 1]    token range of sequence s (CSR)
    const int* grp_off;      // [n_groups + 1] sequence range of group g
    const float* bias;       // [n_seq]
    const int* tok;          // [n_tokens]
    int n_seq, n_groups, n_tokens, max_len;
};

__device__ __forceinline__ sqb_table sqb_views(const int* table, int n_seq, int n_groups, int n_tokens, int max_len) {
    sqb_table t;
    t.seq_off = table;
    t.grp_off = table + n_seq + 1;
    t.bias = reinterpret_cast<const float*>(t.grp_off + n_groups + 1);
    t.tok = reinterpret_cast<const int*>(t.bias + n_seq);
    t.n_seq = n_seq; t.n_groups = n_groups; t.n_tokens = n_tokens; t.max_len = max_len;
    return t;
}

// hist[k] = the history id k places from the end (k < max_len - 1), -1 where there is none or it lies outside [0, V)
__device__ __forceinline__ void sqb_stage(int* hist, const int64_t* __restrict__ seq, int L, int V, int max_len) {
    for (int k = threadIdx.x; k < max_len - 1; k += SQB_BLOCK) {
        const int64_t v = k < L ? seq[L - 1 - k] : -1;
        hist[k] = (v >= 0 && v < V) ? (int)v : -1;
    }
    __syncthreads();
}

// does sequence s complete on this row?  (a table that breaks its own limits matches nothing: no read leaves the table or the LDS)
__device__ __forceinline__ bool sqb_match(const sqb_table& t, const int* hist, int s, int L) {
    const int o = t.seq_off[s], m = t.seq_off[s + 1] - o;
    if (m < 1 || m > t.max_len || o < 0 || o + m > t.n_tokens) return false;
    if (m == 1) return true;                              // transformers: the length-1 bias is applied whatever the history
    if (m > L) return false;                              // longer than the context: ignored
    for (int k = 0; k < m - 1; ++k)
        if (t.tok[o + m - 2 - k] != hist[k]) return false;
    return true;
}

// the group's column: the last token of its first sequence; -1 if the table is broken
__device__ __forceinline__ int sqb_column(const sqb_table& t, int s0, int V) {
    const int e = t.seq_off[s0 + 1];
    if (e < 1 || e > t.n_tokens) return -1;
    const int v = t.tok[e - 1];
    return (v >= 0 && v < V) ? v : -1;
}

__global__ void __launch_bounds__(SQB_BLOCK) sequence_bias_lane_kernel(float* __restrict__ scores, int64_t ld, int V,
                                                                       const int64_t* __restrict__ ids, int64_t ids_stride, int L,
                                                                       const int* __restrict__ table, int n_seq, int n_groups,
                                                                       int n_tokens, int max_len, int bpr) {
    __shared__ int hist[DICOW_SEQ_BIAS_MAX_LEN];
    const int r = blockIdx.x / bpr;
    const int g = (blockIdx.x % bpr) * SQB_BLOCK + threadIdx.x;
    sqb_stage(hist, ids + (int64_t)r * ids_stride, L, V, max_len);
    if (g >= n_groups) return;
    const sqb_table t = sqb_views(table, n_seq, n_groups, n_tokens, max_len);
    const int s0 = max(t.grp_off[g], 0), s1 = min(t.grp_off[g + 1], n_seq);
    float b = 0.f;
    bool any = false;
    for (int s = s0; s < s1; ++s) {
        if (!sqb_match(t, hist, s, L)) continue;
        b = __fadd_rn(b, t.bias[s]);
        any = true;
    }
    if (!any) return;
    const int v = sqb_column(t, s0, V);
    if (v < 0) return;
    float* p = scores + (int64_t)r * ld + v;
    *p = __fadd_rn(*p, b);
}

__global__ void __launch_bounds__(SQB_BLOCK) sequence_bias_wave_kernel(float* __restrict__ scores, int64_t ld, int V,
                                                                       const int64_t* __restrict__ ids, int64_t ids_stride, int L,
                                                                       const int* __restrict__ table, int n_seq, int n_groups,
                                                                       int n_tokens, int max_len, int bpr) {
    __shared__ int hist[DICOW_SEQ_BIAS_MAX_LEN];
    const int r = blockIdx.x / bpr;
    const int lane = threadIdx.x & (DICOW_WAVE - 1);
    const int g = (blockIdx.x % bpr) * SQB_WAVES + (threadIdx.x >> 6);      // (wave-uniform)
    sqb_stage(hist, ids + (int64_t)r * ids_stride, L, V, max_len);
    if (g >= n_groups) return;
    const sqb_table t = sqb_views(table, n_seq, n_groups, n_tokens, max_len);
    const int s0 = max(t.grp_off[g], 0), s1 = min(t.grp_off[g + 1], n_seq);
    float b = 0.f;
    bool any = false;
    for (int base = s0; base < s1; base += DICOW_WAVE) {
        const int s = base + lane;
        unsigned long long hits = __ballot(s < s1 && sqb_match(t, hist, s, L));
        while (hits) {                                     // table order = lane order; every lane runs the same adds
            b = __fadd_rn(b, t.bias[base + __builtin_ctzll(hits)]);
            hits &= hits - 1;
            any = true;
        }
    }
    if (!any || lane != 0) return;
    const int v = sqb_column(t, s0, V);
    if (v < 0) return;
    float* p = scores + (int64_t)r * ld + v;
    *p = __fadd_rn(*p, b);
}

extern "C" int dicow_sequence_bias(float* scores, int64_t ld, int rows, int V, const int64_t* input_ids, int64_t ids_stride, int L,
                                   const int* table, int n_seq, int n_groups, int n_tokens, int max_len, int max_group, int plan,
                                   void* stream) {
    DICOW_REQUIRE(scores && input_ids && rows > 0 && V > 0 && ld >= V && L >= 1 && ids_stride >= L,
                  "sequence_bias: bad args rows=%d V=%d ld=%lld L=%d ids_stride=%lld", rows, V, (long long)ld, L, (long long)ids_stride);
    DICOW_REQUIRE(L <= DICOW_SEQ_BIAS_MAX_L, "sequence_bias: L=%d exceeds DICOW_SEQ_BIAS_MAX_L (%d)", L, DICOW_SEQ_BIAS_MAX_L);
    DICOW_REQUIRE(plan >= 0 && plan <= DICOW_SEQ_BIAS_PLANS, "sequence_bias: plan %d is not 0 .. %d", plan, DICOW_SEQ_BIAS_PLANS);
    DICOW_REQUIRE(n_seq >= 0 && n_seq <= DICOW_SEQ_BIAS_MAX_SEQ, "sequence_bias: n_seq=%d is not 0 .. DICOW_SEQ_BIAS_MAX_SEQ (%d)", n_seq,
                  DICOW_SEQ_BIAS_MAX_SEQ);
    if (n_seq == 0) return DICOW_OK;                      // empty table: nothing to launch
    DICOW_REQUIRE(max_len >= 1 && max_len <= DICOW_SEQ_BIAS_MAX_LEN, "sequence_bias: max_len=%d is not 1 .. DICOW_SEQ_BIAS_MAX_LEN (%d)",
                  max_len, DICOW_SEQ_BIAS_MAX_LEN);
    DICOW_REQUIRE(table && n_groups >= 1 && n_groups <= n_seq && max_group >= 1 && max_group <= n_seq && n_tokens >= n_seq &&
                  (int64_t)n_tokens <= (int64_t)n_seq * max_len,
                  "sequence_bias: bad table n_seq=%d n_groups=%d n_tokens=%d max_len=%d max_group=%d", n_seq, n_groups, n_tokens, max_len,
                  max_group);
    if (plan == 0) plan = max_group >= DICOW_WAVE ? DICOW_SEQ_BIAS_WAVE : DICOW_SEQ_BIAS_LANE;
    const int bpr = dicow_cdiv(n_groups, plan == DICOW_SEQ_BIAS_WAVE ? SQB_WAVES : SQB_BLOCK);
    DICOW_REQUIRE((int64_t)rows * bpr <= 0x7fffffffLL, "sequence_bias: rows=%d x %d workgroups a row exceed the grid", rows, bpr);
    const dim3 grid((unsigned)(rows * bpr));
    if (plan == DICOW_SEQ_BIAS_WAVE)
        sequence_bias_wave_kernel<<<grid, SQB_BLOCK, 0, (hipStream_t)stream>>>(scores, ld, V, input_ids, ids_stride, L, table, n_seq,
                                                                               n_groups, n_tokens, max_len, bpr);
    else
        sequence_bias_lane_kernel<<<grid, SQB_BLOCK, 0, (hipStream_t)stream>>>(scores, ld, V, input_ids, ids_stride, L, table, n_seq,
                                                                               n_groups, n_tokens, max_len, bpr);
    DICOW_CHECK_LAUNCH("sequence_bias_kernel");
    return DICOW_OK;
}

// Word-level alignments: the edit path behind the counts of edit_distance.hip.  The same tables in the same launch shape -- the kernel of
// edit_distance_core.inc with REC = true -- record which step each cell took, 2 bits per cell, and a second kernel walks the path back from
// (N_ref, N_hyp).  The path is defined on ref and hyp, not on rows and columns: at each cell the first of diagonal (open only under the
// interval rule; a hit if the ids are equal, a substitution otherwise), deletion, insertion that attains the cell's key.  ops: one byte per
// step, 0 hit, 1 substitution, 2 deletion, 3 insertion, in forward order, right-aligned in the pair's slot of ref_len + hyp_len bytes.
//
// The walk: one wave per pair.  The records lie skewed, [panel][step s = row + strip][strip t] (edit_distance_core.inc), and along a path
// neither s nor t ever grows, so the wave stages the EA_TS steps x EA_TT strips of records that end at the path's cell -- rows of EA_TT
// 16-bit words, 128 contiguous bytes, one coalesced load per row -- into LDS, lane 0 walks inside the block until the path leaves it (or
// the panel), writing the ops backwards into an LDS buffer, and the wave flushes that buffer to `ops` with one byte per lane.  Records
// outside 0 <= row < n, and strips that hold no column <= m, were never written and are not loaded (a lane whose record is masked loads
// the path's own record again, so that no branch stands between the loads of a batch).  No atomics, one writer per byte.
#include "edit_distance_core.inc"

#define EA_TS 128                                    // steps of a staged block: along the diagonal a strip is crossed every 9 steps
#define EA_TT 64                                     // strips of a staged block: one row is 128 bytes
#define EA_BATCH 32                                  // rows of a block loaded before the first is stored to LDS
#define EA_OB 1024                                   // ops of one block, at most EA_TS + EA_TT * ED_K = 640
#ifndef EA_ONLY                                      // measurement builds (tools/bench_edit_alignment.py): 1 = the recording pass alone,
#define EA_ONLY 0                                    // 2 = the walk alone, over the records an earlier full call left in the same ws
#endif

static_assert(EA_TT == 64 && EA_TS % EA_BATCH == 0, "one lane per strip of a staged block, whole batches");

template <int LANES>
__global__ void __launch_bounds__(64) edit_walk_kernel(const ea_args a) {
    constexpr int P = LANES * ED_K;
    __shared__ uint16_t tile[EA_TS * EA_TT];
    __shared__ uint8_t obuf[EA_OB];
    __shared__ int state[3];
    const int l = threadIdx.x;
    const ed_pair pr = a.pairs[blockIdx.x];
    const ea_pair xp = a.xp[blockIdx.x];
    const int m = pr.m, n = pr.n;
    const bool rows_ref = pr.cols_hyp != 0;                                    // up = deletion, left = insertion
    const uint16_t* rec = reinterpret_cast<const uint16_t*>(a.ws + xp.rec_off);
    const int64_t T = (int64_t)n + LANES - 1;
    const int panels = (m + P - 1) / P;
    int r = n - 1, c = m - 1;                                                  // the path's cell, 0-based row and column
    int64_t pos = xp.slot_end;                                                 // ops[pos ..] are written
    while (r >= 0 && c >= 0) {
        const int p = c / P;
        const int t1 = (c - p * P) / ED_K, s1 = r + t1;
        const int t0 = max(t1 - (EA_TT - 1), 0), s0 = max(s1 - (EA_TS - 1), 0);
        const int w = p + 1 < panels ? LANES : (m - p * P + ED_K - 1) / ED_K;  // the panel's row width
        const uint16_t* base = rec + (int64_t)p * T * LANES;
        const int t = t0 + l;                                                  // EA_TT = 64: lane l stages strip t0 + l of every step
        const int64_t corner = (int64_t)s1 * w + t1;                           // the path's own record: what a masked lane loads instead
#pragma unroll 1
        for (int i0 = 0; i0 <= s1 - s0; i0 += EA_BATCH) {                      // EA_BATCH loads in flight, no branch between them
            uint16_t v[EA_BATCH];
#pragma unroll
            for (int i = 0; i < EA_BATCH; ++i) {
                const int s = s0 + i0 + i;
                const bool ok = s <= s1 && t <= t1 && s - t >= 0 && s - t < n;
                v[i] = base[ok ? (int64_t)s * w + t : corner];
            }
#pragma unroll
            for (int i = 0; i < EA_BATCH; ++i) tile[(i0 + i) * EA_TT + l] = v[i];
        }
        __syncthreads();
        if (l == 0) {
            int q = EA_OB;
            const int c_lo = p * P + t0 * ED_K;
            while (r >= 0 && c >= c_lo && q > 0) {
                const int t = (c - p * P) / ED_K, s = r + t;
                if (s < s0) break;
                const uint32_t code = (tile[(s - s0) * EA_TT + (t - t0)] >> (2 * (c % ED_K))) & 3u;
                obuf[--q] = (uint8_t)code;
                const bool up = code < 2u || ((code == 2u) == rows_ref);
                const bool left = code < 2u || ((code == 2u) != rows_ref);
                r -= up;
                c -= left;
            }
            state[0] = r; state[1] = c; state[2] = q;
        }
        __syncthreads();
        r = state[0]; c = state[1];
        const int q = state[2], cnt = EA_OB - q;
        for (int x = l; x < cnt; x += 64) a.ops[pos - cnt + x] = obuf[q + x];
        pos -= cnt;
        __syncthreads();
    }
    const int rest = (r + 1) + (c + 1);                                        // row or column 0: one step is open
    const uint8_t code = (c >= 0) == rows_ref ? 3 : 2;                         // columns left over are hypothesis words when the rows are ref
    for (int x = l; x < rest; x += 64) a.ops[pos - rest + x] = code;
    pos -= rest;
    if (l == 0) {
        a.spans[2 * (int64_t)blockIdx.x] = pos;
        a.spans[2 * (int64_t)blockIdx.x + 1] = xp.slot_end - pos;
    }
}

// The call's plan, shared by the size query and the entry point: the workgroup width, the key, and the workspace laid out as
// [n_pairs] ed_pair, [n_pairs] ea_pair, the boundary columns, the records.  image: null, or where to build the uploaded tables.
static_assert(sizeof(ed_pair) + sizeof(ea_pair) == DICOW_ALIGN_TABLE_BYTES, "the header states the tables' size");

struct ea_plan { int lanes; bool key64, any_ref, any_hyp; int64_t table_bytes, need; };

static inline int64_t ea_rec_bytes(int64_t m, int64_t n, int lanes) {
    if (m == 0 || n == 0) return 0;
    const int64_t P = (int64_t)lanes * ED_K, panels = (m + P - 1) / P, w = (m - (panels - 1) * P + ED_K - 1) / ED_K;
    return (2 * ((panels - 1) * (n + lanes - 1) * lanes + (n + w - 1) * w) + 7) / 8 * 8;
}

static int ea_make_plan(const char* who, const int64_t* pairs, int n_pairs, int lanes, int along, std::vector<int64_t>* image, ea_plan* plan) {
    if (ed_check_lens(who, pairs, n_pairs) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(lanes == 0 || lanes == ED_NARROW || lanes == ED_WIDE, "%s: lanes=%d is none of 0, %d, %d", who, lanes, ED_NARROW, ED_WIDE);
    DICOW_REQUIRE(along >= 0 && along <= 2, "%s: along=%d is none of 0 (the library's choice), 1 (ref along the lanes), 2 (hyp)", who, along);
    bool wide = lanes == ED_WIDE;
    plan->key64 = plan->any_ref = plan->any_hyp = false;
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        if (lanes == 0 && std::min(row[1], row[3]) > (int64_t)ED_NARROW * ED_K) wide = true;
        plan->key64 |= row[1] + row[3] > ED_I32_MAX_SUM;
        plan->any_ref |= row[1] > 0;
        plan->any_hyp |= row[3] > 0;
    }
    const int L = plan->lanes = wide ? ED_WIDE : ED_NARROW;
    plan->table_bytes = (int64_t)n_pairs * (int64_t)(sizeof(ed_pair) + sizeof(ea_pair));
    if (image) image->assign((size_t)plan->table_bytes / 8, 0);
    ed_pair* e = image ? reinterpret_cast<ed_pair*>(image->data()) : nullptr;
    ea_pair* x = image ? reinterpret_cast<ea_pair*>(e + n_pairs) : nullptr;
    int64_t need = plan->table_bytes, slot = 0;
    for (int k = 0; k < n_pairs; ++k) {                                         // the boundary columns
        const int64_t* row = pairs + 4 * (int64_t)k;
        if (e) e[k].bnd_off = need;
        need += ed_bnd_bytes(row[1], row[3]);
    }
    for (int k = 0; k < n_pairs; ++k) {                                         // the records
        const int64_t* row = pairs + 4 * (int64_t)k;
        const bool cols_hyp = along == 2 || (along == 0 && ed_steps(row[3], row[1], L) < ed_steps(row[1], row[3], L));
        const int64_t m = cols_hyp ? row[3] : row[1], n = cols_hyp ? row[1] : row[3];
        slot += row[1] + row[3];
        if (e) {
            e[k].col_start = cols_hyp ? row[2] : row[0];
            e[k].row_start = cols_hyp ? row[0] : row[2];
            e[k].m = (int32_t)m;
            e[k].n = (int32_t)n;
            e[k].cols_hyp = cols_hyp;
            x[k].rec_off = need;
            x[k].slot_end = slot;
        }
        need += ea_rec_bytes(m, n, L);
        DICOW_REQUIRE(need <= DICOW_ALIGN_MAX_WS_BYTES, "%s: the records up to pair %d of %d bring the workspace to %lld bytes, past "
                      "DICOW_ALIGN_MAX_WS_BYTES = %lld (split the call)", who, k, n_pairs, (long long)need, (long long)DICOW_ALIGN_MAX_WS_BYTES);
    }
    plan->need = need;
    return DICOW_OK;
}

extern "C" int64_t dicow_edit_alignment_ws_bytes(const int64_t* pairs, int n_pairs, int lanes, int along) {
    ea_plan plan;
    if (ea_make_plan("edit_alignment_ws_bytes", pairs, n_pairs, lanes, along, nullptr, &plan) != DICOW_OK) return -1;
    return plan.need;
}

template <typename KEY, bool IV>
static void ea_launch(int lanes, int n_pairs, hipStream_t st, const ea_args& a) {
    if (lanes == ED_WIDE) edit_distance_kernel<KEY, IV, ED_WIDE, true><<<dim3((unsigned)n_pairs), ED_WIDE, 0, st>>>(a);
    else edit_distance_kernel<KEY, IV, ED_NARROW, true><<<dim3((unsigned)n_pairs), ED_NARROW, 0, st>>>(a);
}

extern "C" int dicow_edit_alignment(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv,
                                    const int32_t* hyp_iv, const int64_t* pairs, int n_pairs, int32_t* out, uint8_t* ops, int64_t* spans,
                                    int lanes, int along, void* ws, int64_t ws_bytes, void* stream) {
    static thread_local std::vector<int64_t> stage;          // the uploaded image: both tables; lives until this thread's next call
    ea_plan plan;
    if (ea_make_plan("edit_alignment", pairs, n_pairs, lanes, along, &stage, &plan) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(n_ref >= 0 && n_hyp >= 0, "edit_alignment: negative buffer size n_ref=%lld n_hyp=%lld", (long long)n_ref, (long long)n_hyp);
    DICOW_REQUIRE((ref_iv == nullptr) == (hyp_iv == nullptr), "edit_alignment: intervals given for one side only (ref_iv %s, hyp_iv %s)",
                  ref_iv ? "set" : "null", hyp_iv ? "set" : "null");
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        DICOW_REQUIRE(row[0] >= 0 && row[0] <= n_ref && row[1] <= n_ref - row[0], "edit_alignment: pair %d reads ref [%lld, %lld + %lld), outside the %lld "
                      "ids of the buffer", k, (long long)row[0], (long long)row[0], (long long)row[1], (long long)n_ref);
        DICOW_REQUIRE(row[2] >= 0 && row[2] <= n_hyp && row[3] <= n_hyp - row[2], "edit_alignment: pair %d reads hyp [%lld, %lld + %lld), outside the %lld "
                      "ids of the buffer", k, (long long)row[2], (long long)row[2], (long long)row[3], (long long)n_hyp);
    }
    if (n_pairs == 0) return DICOW_OK;
    DICOW_REQUIRE(out && spans && ws && (ops || !(plan.any_ref || plan.any_hyp)) && (ref_ids || !plan.any_ref) && (hyp_ids || !plan.any_hyp),
                  "edit_alignment: null pointer");
    DICOW_REQUIRE(reinterpret_cast<uintptr_t>(ref_ids) % 4 == 0 && reinterpret_cast<uintptr_t>(hyp_ids) % 4 == 0 && reinterpret_cast<uintptr_t>(ref_iv) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(hyp_iv) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 && reinterpret_cast<uintptr_t>(spans) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(ws) % 8 == 0, "edit_alignment: ids / intervals / out not 4-byte or spans / ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= plan.need, "edit_alignment: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)plan.need);
    hipStream_t st = (hipStream_t)stream;
    const void* image = stage.data();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
    if (cs == hipStreamCaptureStatusActive) image = (new std::vector<int64_t>(stage))->data();      // a graph's copy node reads its source at every
                                                                                                   // replay: this image is kept for good
    hipError_t e = hipMemcpyAsync(ws, image, (size_t)plan.table_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) DICOW_FAIL(DICOW_ERR_LAUNCH, "edit_alignment: table upload: %s", hipGetErrorString(e));
    ea_args a;
    a.ref_ids = ref_ids; a.hyp_ids = hyp_ids; a.ref_iv = ref_iv; a.hyp_iv = hyp_iv;
    a.pairs = reinterpret_cast<const ed_pair*>(ws);
    a.ws = static_cast<char*>(ws);
    a.out = out;
    a.xp = reinterpret_cast<const ea_pair*>(a.pairs + n_pairs);
    a.ops = ops;
    a.spans = spans;
    const int L = plan.lanes;
    if (EA_ONLY != 2) {
        if (plan.key64) { if (ref_iv) ea_launch<int64_t, true>(L, n_pairs, st, a); else ea_launch<int64_t, false>(L, n_pairs, st, a); }
        else { if (ref_iv) ea_launch<int32_t, true>(L, n_pairs, st, a); else ea_launch<int32_t, false>(L, n_pairs, st, a); }
        DICOW_CHECK_LAUNCH("edit_distance_kernel (recording)");
    }
    if (EA_ONLY != 1) {
        if (L == ED_WIDE) edit_walk_kernel<ED_WIDE><<<dim3((unsigned)n_pairs), 64, 0, st>>>(a);
        else edit_walk_kernel<ED_NARROW><<<dim3((unsigned)n_pairs), 64, 0, st>>>(a);
        DICOW_CHECK_LAUNCH("edit_walk_kernel");
    }
    return DICOW_OK;
}

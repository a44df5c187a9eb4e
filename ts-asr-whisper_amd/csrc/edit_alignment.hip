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

extern "C" int64_t dicow_edit_alignment_ws_bytes(const int64_t* pairs, int n_pairs, int lanes, int along) {
    ed_plan plan;
    if (ed_make_plan("edit_alignment_ws_bytes", pairs, n_pairs, lanes, along, true, nullptr, &plan) != DICOW_OK) return -1;
    return plan.need;
}

extern "C" int dicow_edit_alignment(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv,
                                    const int32_t* hyp_iv, const int64_t* pairs, int n_pairs, int32_t* out, uint8_t* ops, int64_t* spans,
                                    int lanes, int along, void* ws, int64_t ws_bytes, void* stream) {
    static thread_local std::vector<int64_t> stage;          // the uploaded image: both tables
    ed_plan plan;
    if (ed_make_plan("edit_alignment", pairs, n_pairs, lanes, along, true, &stage, &plan) != DICOW_OK) return DICOW_ERR_INVALID;
    if (int rc = ed_check_buffers("edit_alignment", pairs, n_pairs, n_ref, n_hyp, ref_iv, hyp_iv)) return rc;
    if (n_pairs == 0) return DICOW_OK;
    DICOW_REQUIRE(out && spans && ws && (ops || !(plan.any_ref || plan.any_hyp)) && (ref_ids || !plan.any_ref) && (hyp_ids || !plan.any_hyp),
                  "edit_alignment: null pointer");
    DICOW_REQUIRE(dicow_aligned(4, ref_ids, hyp_ids, ref_iv, hyp_iv, out) && dicow_aligned(8, spans, ws),
                  "edit_alignment: ids / intervals / out not 4-byte or spans / ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= plan.need, "edit_alignment: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)plan.need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dicow_upload("edit_alignment", ws, stage.data(), plan.table_bytes, st)) return rc;
    ea_args a;
    a.ref_ids = ref_ids; a.hyp_ids = hyp_ids; a.ref_iv = ref_iv; a.hyp_iv = hyp_iv;
    a.pairs = reinterpret_cast<const ed_pair*>(ws);
    a.ws = static_cast<char*>(ws);
    a.out = out;
    a.xp = reinterpret_cast<const ea_pair*>(a.pairs + n_pairs);
    a.ops = ops;
    a.spans = spans;
    if (EA_ONLY != 2) {
        ed_launch<true>(plan, n_pairs, st, a);
        DICOW_CHECK_LAUNCH("edit_distance_kernel (recording)");
    }
    if (EA_ONLY != 1) {
        if (plan.lanes == ED_WIDE) edit_walk_kernel<ED_WIDE><<<dim3((unsigned)n_pairs), 64, 0, st>>>(a);
        else edit_walk_kernel<ED_NARROW><<<dim3((unsigned)n_pairs), 64, 0, st>>>(a);
        DICOW_CHECK_LAUNCH("edit_walk_kernel");
    }
    return DICOW_OK;
}

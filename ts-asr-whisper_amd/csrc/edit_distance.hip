// Scoring what was decoded: a batch of Levenshtein tables over int32 symbol ids, the hot path of WER / CER (one pair per utterance) and of
// cpWER / tcpWER (one pair per (reference speaker, hypothesis speaker) over whole-meeting word streams; the reference scores utterances
// with jiwer, src/utils/evaluation.py:32-79, and sessions with meeteval, src/utils/wer.py:30-38, 89-97).  Unit costs; cell (i, j) may take
// the diagonal step -- a hit when the symbols are equal, a substitution otherwise -- only if no intervals were given or the two words'
// intervals overlap, rb < he && hb < re (tcpWER's time constraint).  Among the alignments with the fewest errors E the one with the most
// hits H is taken: the lexicographic minimum of the additive key (E, -H), packed into one integer  key = E * UNIT - H  with H < UNIT, so
// a step adds UNIT (insertion, deletion, substitution) or -1 (hit) and min() on the packed value is the lexicographic min.  UNIT = 2^15
// in int32 when every pair of the call has ref_len + hyp_len <= ED_I32_MAX_SUM (then E <= 65535 and H <= 32767 in every cell, the padding
// columns of the last panel included), 2^32 in int64 otherwise.  The key is symmetric under swapping the sequences, so the host puts
// whichever of the two makes fewer steps along the lanes ("columns", m of them) and the other along the steps ("rows", n).
//
// One workgroup of LANES threads per pair.  Lane t keeps D[i][j] for its strip of ED_K consecutive columns in registers, with the strip's
// symbols (and intervals).  Rows run as a skewed pipeline: at step s lane t computes row s - t, takes the key left of its strip -- with
// that row's symbol (and interval) -- from lane t - 1's message of step s - 1 in LDS, and leaves its own right-edge key with the same row
// data for lane t + 1: two message buffers by step parity, one barrier per step.  A panel is P = LANES * ED_K columns.  Lane 0's messages
// are the panel's left boundary -- D[i][0] = i for the first panel, the previous panel's last column otherwise -- with the row's data, loaded
// LANES rows at a time one chunk ahead (a register, then LDS).  The last lane's keys of a chunk of steps are collected in LDS and written
// LANES at a time to the pair's slice of the workspace, two columns per pair by panel parity: one writer per slot, no atomics.  Columns
// behind m in the last panel are computed like the others (symbol 0, row-0 key clamped at m) and never read: values flow left to right.
// The lane that owns column m holds D[n][m] after the last panel and writes (E, H).
// The kernel and the host pieces shared with edit_alignment.hip: edit_distance_core.inc (REC = false here).
#include "edit_distance_core.inc"

extern "C" int64_t dicow_edit_distance_ws_bytes(const int64_t* pairs, int n_pairs) {
    if (ed_check_lens("edit_distance_ws_bytes", pairs, n_pairs) != DICOW_OK) return -1;
    int64_t need = (int64_t)n_pairs * (int64_t)sizeof(ed_pair);
    for (int k = 0; k < n_pairs; ++k) need += ed_bnd_bytes(pairs[4 * (int64_t)k + 1], pairs[4 * (int64_t)k + 3]);
    return need;
}

template <typename KEY, bool IV>
static void ed_launch(int lanes, int n_pairs, hipStream_t st, const ed_args& a) {
    if (lanes == ED_WIDE) edit_distance_kernel<KEY, IV, ED_WIDE><<<dim3((unsigned)n_pairs), ED_WIDE, 0, st>>>(a);
    else edit_distance_kernel<KEY, IV, ED_NARROW><<<dim3((unsigned)n_pairs), ED_NARROW, 0, st>>>(a);
}

extern "C" int dicow_edit_distance(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv,
                                   const int32_t* hyp_iv, const int64_t* pairs, int n_pairs, int32_t* out, int lanes, int along, void* ws,
                                   int64_t ws_bytes, void* stream) {
    if (ed_check_lens("edit_distance", pairs, n_pairs) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(n_ref >= 0 && n_hyp >= 0, "edit_distance: negative buffer size n_ref=%lld n_hyp=%lld", (long long)n_ref, (long long)n_hyp);
    DICOW_REQUIRE((ref_iv == nullptr) == (hyp_iv == nullptr), "edit_distance: intervals given for one side only (ref_iv %s, hyp_iv %s)",
                  ref_iv ? "set" : "null", hyp_iv ? "set" : "null");
    DICOW_REQUIRE(lanes == 0 || lanes == ED_NARROW || lanes == ED_WIDE, "edit_distance: lanes=%d is none of 0, %d, %d", lanes, ED_NARROW, ED_WIDE);
    DICOW_REQUIRE(along >= 0 && along <= 2, "edit_distance: along=%d is none of 0 (the library's choice), 1 (ref along the lanes), 2 (hyp)", along);
    // ---- the pair table, on the host, before anything is launched
    static thread_local std::vector<int64_t> stage;          // the uploaded image: [n_pairs] ed_pair; lives until this thread's next call
    stage.assign((size_t)n_pairs * (sizeof(ed_pair) / 8), 0);
    bool wide = lanes == ED_WIDE, key64 = false, any_ref = false, any_hyp = false;
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        DICOW_REQUIRE(row[0] >= 0 && row[0] <= n_ref && row[1] <= n_ref - row[0], "edit_distance: pair %d reads ref [%lld, %lld + %lld), outside the %lld "
                      "ids of the buffer", k, (long long)row[0], (long long)row[0], (long long)row[1], (long long)n_ref);
        DICOW_REQUIRE(row[2] >= 0 && row[2] <= n_hyp && row[3] <= n_hyp - row[2], "edit_distance: pair %d reads hyp [%lld, %lld + %lld), outside the %lld "
                      "ids of the buffer", k, (long long)row[2], (long long)row[2], (long long)row[3], (long long)n_hyp);
        if (lanes == 0 && std::min(row[1], row[3]) > (int64_t)ED_NARROW * ED_K) wide = true;
        key64 |= row[1] + row[3] > ED_I32_MAX_SUM;
        any_ref |= row[1] > 0;
        any_hyp |= row[3] > 0;
    }
    if (n_pairs == 0) return DICOW_OK;
    const int L = wide ? ED_WIDE : ED_NARROW;
    int64_t need = (int64_t)n_pairs * (int64_t)sizeof(ed_pair);
    const int64_t tbytes = need;
    for (int k = 0; k < n_pairs; ++k) {
        const int64_t* row = pairs + 4 * (int64_t)k;
        const bool cols_hyp = along == 2 || (along == 0 && ed_steps(row[3], row[1], L) < ed_steps(row[1], row[3], L));
        ed_pair* e = reinterpret_cast<ed_pair*>(stage.data()) + k;
        e->col_start = cols_hyp ? row[2] : row[0];
        e->row_start = cols_hyp ? row[0] : row[2];
        e->m = (int32_t)(cols_hyp ? row[3] : row[1]);
        e->n = (int32_t)(cols_hyp ? row[1] : row[3]);
        e->cols_hyp = cols_hyp;
        e->bnd_off = need;
        need += ed_bnd_bytes(row[1], row[3]);
    }
    DICOW_REQUIRE(out && ws && (ref_ids || !any_ref) && (hyp_ids || !any_hyp), "edit_distance: null pointer");
    DICOW_REQUIRE(reinterpret_cast<uintptr_t>(ref_ids) % 4 == 0 && reinterpret_cast<uintptr_t>(hyp_ids) % 4 == 0 && reinterpret_cast<uintptr_t>(ref_iv) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(hyp_iv) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
                  "edit_distance: ids / intervals / out not 4-byte or ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= need, "edit_distance: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const void* image = stage.data();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
    if (cs == hipStreamCaptureStatusActive) image = (new std::vector<int64_t>(stage))->data();      // a graph's copy node reads its source at every
                                                                                                   // replay: this image is kept for good
    hipError_t e = hipMemcpyAsync(ws, image, (size_t)tbytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) DICOW_FAIL(DICOW_ERR_LAUNCH, "edit_distance: table upload: %s", hipGetErrorString(e));
    ed_args a;
    a.ref_ids = ref_ids; a.hyp_ids = hyp_ids; a.ref_iv = ref_iv; a.hyp_iv = hyp_iv;
    a.pairs = reinterpret_cast<const ed_pair*>(ws);
    a.ws = static_cast<char*>(ws);
    a.out = out;
    if (key64) { if (ref_iv) ed_launch<int64_t, true>(L, n_pairs, st, a); else ed_launch<int64_t, false>(L, n_pairs, st, a); }
    else { if (ref_iv) ed_launch<int32_t, true>(L, n_pairs, st, a); else ed_launch<int32_t, false>(L, n_pairs, st, a); }
    DICOW_CHECK_LAUNCH("edit_distance_kernel");
    return DICOW_OK;
}

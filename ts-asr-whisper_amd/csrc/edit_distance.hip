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
    ed_plan plan;
    if (ed_make_plan("edit_distance_ws_bytes", pairs, n_pairs, 0, 0, false, nullptr, &plan) != DICOW_OK) return -1;
    return plan.need;
}

extern "C" int dicow_edit_distance(const int32_t* ref_ids, int64_t n_ref, const int32_t* hyp_ids, int64_t n_hyp, const int32_t* ref_iv,
                                   const int32_t* hyp_iv, const int64_t* pairs, int n_pairs, int32_t* out, int lanes, int along, void* ws,
                                   int64_t ws_bytes, void* stream) {
    static thread_local std::vector<int64_t> stage;          // the uploaded image: [n_pairs] ed_pair
    ed_plan plan;
    if (ed_make_plan("edit_distance", pairs, n_pairs, lanes, along, false, &stage, &plan) != DICOW_OK) return DICOW_ERR_INVALID;
    if (int rc = ed_check_buffers("edit_distance", pairs, n_pairs, n_ref, n_hyp, ref_iv, hyp_iv)) return rc;
    if (n_pairs == 0) return DICOW_OK;
    DICOW_REQUIRE(out && ws && (ref_ids || !plan.any_ref) && (hyp_ids || !plan.any_hyp), "edit_distance: null pointer");
    DICOW_REQUIRE(dicow_aligned(4, ref_ids, hyp_ids, ref_iv, hyp_iv, out) && dicow_aligned(8, ws),
                  "edit_distance: ids / intervals / out not 4-byte or ws not 8-byte aligned");
    DICOW_REQUIRE(ws_bytes >= plan.need, "edit_distance: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)plan.need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dicow_upload("edit_distance", ws, stage.data(), plan.table_bytes, st)) return rc;
    ed_args a;
    a.ref_ids = ref_ids; a.hyp_ids = hyp_ids; a.ref_iv = ref_iv; a.hyp_iv = hyp_iv;
    a.pairs = reinterpret_cast<const ed_pair*>(ws);
    a.ws = static_cast<char*>(ws);
    a.out = out;
    ed_launch<false>(plan, n_pairs, st, a);
    DICOW_CHECK_LAUNCH("edit_distance_kernel");
    return DICOW_OK;
}

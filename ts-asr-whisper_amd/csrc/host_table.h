// Host pieces of the table-driven entry points (include/dicow_hip.h, HOST TABLES): each checks a host table in full, builds descriptors
// into a staged image, copies the image to the head of the caller's workspace on the stream and launches kernels that read it there.
// What they share is the upload with its graph-capture rule and a few refusals.  Host only: kernel files that take no host table
// do not need it.
#pragma once
#include "common.h"

// Copies `bytes` of the host table `src` to `dst` on `stream`; bytes == 0 does nothing.  Outside capture it copies from `src` as given
// (a staged image lives until its thread's next call, a caller's array until the call returns).  A captured copy node reads its source
// at every replay, so under an active capture `src` is duplicated into storage that is never freed and the node reads that: a replay
// sees neither caller memory nor a later call's image.  A failure sets "<who>: table upload: <hip error>" and returns DICOW_ERR_LAUNCH.
int dicow_upload(const char* who, void* dst, const void* src, int64_t bytes, hipStream_t stream);

static inline bool dicow_misaligned(const void* p, uintptr_t k) { return reinterpret_cast<uintptr_t>(p) % k != 0; }
template <typename... P>
static inline bool dicow_aligned(uintptr_t k, const P*... p) { return !(dicow_misaligned(p, k) || ...); }   // every pointer (null included) to k bytes

// [start, start + len) lies inside [0, total) (len >= 0 is the caller's to refuse; the form cannot overflow)
static inline bool dicow_span_ok(int64_t start, int64_t len, int64_t total) { return start >= 0 && start <= total && len <= total - start; }

// "<item> <verb what> [a, a + b), outside the <total> <units>"; `item` is a format with its arguments behind, e.g. "%s: pair %d", who, k
#define DICOW_REQUIRE_SPAN(start, len, total, what, units, item, ...)                                                                     \
    DICOW_REQUIRE(dicow_span_ok(start, len, total), item " " what " [%lld, %lld + %lld), outside the %lld " units, __VA_ARGS__,          \
                  (long long)(start), (long long)(start), (long long)(len), (long long)(total))

// the refusals edit_distance, edit_alignment and orc_distance share: id buffers of negative size, intervals for one side only
static inline int dicow_check_id_buffers(const char* who, int64_t n_ref, int64_t n_hyp, const int32_t* ref_iv, const int32_t* hyp_iv) {
    DICOW_REQUIRE(n_ref >= 0 && n_hyp >= 0, "%s: negative buffer size n_ref=%lld n_hyp=%lld", who, (long long)n_ref, (long long)n_hyp);
    DICOW_REQUIRE((ref_iv == nullptr) == (hyp_iv == nullptr), "%s: intervals given for one side only (ref_iv %s, hyp_iv %s)", who,
                  ref_iv ? "set" : "null", hyp_iv ? "set" : "null");
    return DICOW_OK;
}

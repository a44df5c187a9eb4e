// External enrollment mixtures on waveforms resident in HBM (reference generate_enrollment_mixture, src/data/local_datasets.py:355-436: a
// MixedCut of one utterance of the target speaker and a few of other speakers, cut at 30 s), ahead of dicow_logmel.
//
// Per track k = (row, clip, off, len) of the plan: samples [0, len) of the clip land on samples [off, off + len) of the row.
//     out[row, t] = ((x_0 + x_1) + x_2) + ...    over the row's tracks, in plan order, that cover t;    0 where none does
// One launch over the grid (ranges of EMX_BLOCK * EMX_VPT vectors, B).  A workgroup finds its row's tracks by a binary search over the
// plan's non-decreasing row column (uniform loads), keeps at most DICOW_ENR_MIX_MAX_TRACKS (base, first, last) triples in registers, and
// every thread then owns whole 16-byte vectors of the row: per track a 4-byte-aligned 16-byte load where the vector lies inside the
// track (clips start anywhere in the bank; legal for global memory on gfx950), single loads for the samples of a vector that a track edge
// cuts, nothing where the track does not reach.  The first track that covers a sample sets it (its bits), every further one is one
// __fadd_rn; a sample no track covers is stored as 0.  Each sample of [0, n) has exactly one writer and is written once -- float4 stores,
// single stores on the up-to-three samples behind the last whole vector -- so the sum of a sample is a function of the plan alone: no
// atomics, no workspace, no dependence on the grid.  The plan is validated on the host before the launch (dicow_enrollment_mix).
#include "host_table.h"

#define EMX_BLOCK 256
#define EMX_VPT 4                         // vectors per thread
#define EMX_MAXT DICOW_ENR_MIX_MAX_TRACKS

struct __attribute__((packed, aligned(4))) emx_f4u { float x, y, z, w; };     // 16 bytes at 4-byte alignment

__global__ void __launch_bounds__(EMX_BLOCK) enrollment_mix_kernel(float* __restrict__ out, int64_t ld_out, int n, const float* __restrict__ bank,
                                                                   const int64_t* __restrict__ clip_start, const int* __restrict__ plan,
                                                                   int n_tracks) {
    const int row = blockIdx.y;
    int first = 0, hi = n_tracks;                                        // the first plan entry whose row is >= this one
    while (first < hi) {
        const int mid = (first + hi) >> 1;
        if (plan[4 * (int64_t)mid] < row) first = mid + 1; else hi = mid;
    }
    int64_t base[EMX_MAXT];                                              // bank index of the sample that lands on t = 0 (may lie before the clip)
    int t0[EMX_MAXT], t1[EMX_MAXT];                                      // the track covers [t0, t1)
    int nt = 0;
#pragma unroll
    for (int k = 0; k < EMX_MAXT; ++k) {
        const int e = first + k;
        const bool mine = e < n_tracks && plan[4 * (int64_t)(e < n_tracks ? e : 0)] == row;
        const int* pl = plan + 4 * (int64_t)(mine ? e : 0);
        base[k] = 0; t0[k] = 0; t1[k] = 0;
        if (mine) {                                                      // (the rows are sorted: `mine` never turns true again)
            const int off = pl[2];
            base[k] = clip_start[pl[1]] - off;
            t0[k] = off;
            t1[k] = off + pl[3];
            nt = k + 1;
        }
    }
    float* o = out + (int64_t)row * ld_out;
    const int nvec = (n + 3) >> 2;
#pragma unroll
    for (int u = 0; u < EMX_VPT; ++u) {
        const int64_t j = ((int64_t)blockIdx.x * EMX_VPT + u) * EMX_BLOCK + threadIdx.x;
        if (j >= nvec) break;
        const int i = (int)(4 * j);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned cov = 0;                                                // bit q: sample i + q has a value
#pragma unroll
        for (int k = 0; k < EMX_MAXT; ++k) {
            if (k >= nt || i + 4 <= t0[k] || i >= t1[k]) continue;
            const float* c = bank + (base[k] + i);                       // c[q] is read only where t0 <= i + q < t1: inside the clip
            float x[4];
            unsigned m;
            if (i >= t0[k] && i + 4 <= t1[k]) {
                const emx_f4u q = *reinterpret_cast<const emx_f4u*>(c);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
                m = 15u;
            } else {
                m = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool in = i + q >= t0[k] && i + q < t1[k];
                    x[q] = in ? c[q] : 0.f;
                    m |= (unsigned)in << q;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (m >> q & 1u) v[q] = (cov >> q & 1u) ? __fadd_rn(v[q], x[q]) : x[q];
            cov |= m;
        }
        if (i + 4 <= n) {
            *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < n) o[i + q] = v[q];
        }
    }
}

extern "C" int dicow_enrollment_mix(float* out, int64_t ld_out, int B, int n, const float* bank, const int64_t* clip_start, const int32_t* plan_dev,
                                    const int32_t* plan_host, int n_tracks, const int32_t* clip_len_host, int n_clips, void* stream) {
    DICOW_REQUIRE(B >= 0 && B <= 65535, "enrollment_mix: B=%d outside [0, 65535]", B);
    DICOW_REQUIRE(n >= 0 && n <= 0x7ffffff0, "enrollment_mix: n=%d outside [0, 2^31 - 16]", n);
    DICOW_REQUIRE(n_tracks >= 0 && n_clips >= 0, "enrollment_mix: negative size n_tracks=%d n_clips=%d", n_tracks, n_clips);
    DICOW_REQUIRE(ld_out >= n && ld_out % 4 == 0, "enrollment_mix: ld_out=%lld must be a multiple of 4 and >= n=%d", (long long)ld_out, n);
    DICOW_REQUIRE(n_tracks == 0 || (plan_host && clip_len_host), "enrollment_mix: null host plan");
    // ---- the plan, on the host, before anything is launched
    int prev_row = 0, in_row = 0;
    for (int k = 0; k < n_tracks; ++k) {
        const int32_t* p = plan_host + 4 * (int64_t)k;
        const int row = p[0], clip = p[1], off = p[2], len = p[3];
        DICOW_REQUIRE(row >= 0 && row < B, "enrollment_mix: track %d names row %d outside the batch of %d", k, row, B);
        DICOW_REQUIRE(row >= prev_row, "enrollment_mix: track %d names row %d behind row %d (rows must not decrease)", k, row, prev_row);
        in_row = row == prev_row ? in_row + 1 : 1;
        prev_row = row;
        DICOW_REQUIRE(in_row <= DICOW_ENR_MIX_MAX_TRACKS, "enrollment_mix: row %d has more than %d tracks", row, DICOW_ENR_MIX_MAX_TRACKS);
        DICOW_REQUIRE(clip >= 0 && clip < n_clips, "enrollment_mix: track %d names clip %d outside the bank of %d", k, clip, n_clips);
        DICOW_REQUIRE(off >= 0, "enrollment_mix: track %d has the negative offset %d", k, off);
        DICOW_REQUIRE(len >= 1 && len <= clip_len_host[clip], "enrollment_mix: track %d has len %d outside [1, %d], the length of clip %d", k, len,
                      clip_len_host[clip], clip);
        DICOW_REQUIRE((int64_t)off + len <= n, "enrollment_mix: track %d ends at sample %lld behind the row's n=%d", k, (long long)off + len, n);
    }
    if (B == 0 || n == 0) return DICOW_OK;
    DICOW_REQUIRE(out && (n_tracks == 0 || (bank && clip_start && plan_dev)), "enrollment_mix: null pointer");
    DICOW_REQUIRE(dicow_aligned(16, out), "enrollment_mix: out not 16-byte aligned");
    DICOW_REQUIRE(dicow_aligned(4, bank, plan_dev) && dicow_aligned(8, clip_start), "enrollment_mix: bank / plan / clip_start misaligned");
    const int nvec = (n + 3) >> 2;
    const dim3 grid(dicow_cdiv(nvec, EMX_BLOCK * EMX_VPT), B);
    enrollment_mix_kernel<<<grid, EMX_BLOCK, 0, (hipStream_t)stream>>>(out, ld_out, n, bank, clip_start, plan_dev, n_tracks);
    DICOW_CHECK_LAUNCH("enrollment_mix_kernel");
    return DICOW_OK;
}

// Greedy CTC decoding on the GPU (the evaluation half of CTC pre-training).
//
// Replaces ctc_greedy_decode of the reference (src/utils/decoding.py:6-12): torch.argmax over the classes, then a Python
// itertools.groupby over every row of the device tensor -- one host read per frame, ~6000 per evaluation batch of
// 16 x 375 frames.  Two launches, no host read, no atomics, nothing allocated:
//   1. ctc_greedy_argmax_kernel    one 256-thread workgroup per frame row reduces (value, index) pairs over the V1 real classes
//                                  and stores the winning index in the caller's int32 workspace [B * Tn].  The row is read once,
//                                  in 16-byte vectors from the first 16-byte boundary on, with a scalar head and tail (a row of a
//                                  view may start anywhere; with an odd row stride every row starts somewhere else).  Columns
//                                  >= V1 -- the zero padding of the product's 128-padded rows, or whatever a view holds there --
//                                  are never read, so they cannot win.
//   2. ctc_greedy_compact_kernel   one workgroup per batch row walks the frames in tiles of 256: a frame is kept when its id is
//                                  not `blank` and differs from the previous frame's id (read from the workspace: the tile
//                                  boundary needs no carried state); the kept ids are compacted with one 64-bit ballot per wave,
//                                  the four wave counts through LDS, and a running count carried across the tiles; the rest of
//                                  the row is filled with pad_id.
// Ties: the lowest index wins, as torch.argmax does on the CPU.  A thread meets its columns in increasing order, so a strict
// `>` keeps the first of equal values; the cross-lane steps compare (value, index).  -inf never satisfies `>`: a thread that
// found nothing above -inf answers with the first column it read, so a row of -inf gives 0.  NaN never satisfies `>` either
// (outside the contract; the stored index still lies in [0, V1)).
#include "host_table.h"

#define CGD_BLOCK 256
#define CGD_NONE 0x7fffffff

__device__ __forceinline__ void cgd_take(float v, int i, float& best, int& idx) {
    if (v > best) { best = v; idx = i; }
}
__device__ __forceinline__ void cgd_merge(float v2, int i2, float& best, int& idx) {
    if (v2 > best || (v2 == best && i2 < idx)) { best = v2; idx = i2; }
}

template <int BF>
__global__ void __launch_bounds__(CGD_BLOCK) ctc_greedy_argmax_kernel(const void* __restrict__ logits, int64_t batch_stride, int64_t ld,
                                                                      int Tn, int V1, int64_t rows, int* __restrict__ ws) {
    constexpr int ES = BF ? 2 : 4, VEC = 16 / ES;
    __shared__ float red_v[CGD_BLOCK / 64];
    __shared__ int red_i[CGD_BLOCK / 64];
    const int tid = threadIdx.x;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / Tn, t = row - b * Tn;
        const char* p = reinterpret_cast<const char*>(logits) + (b * batch_stride + t * ld) * ES;
        const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15);
        const int head = min(V1, mis ? (16 - mis) / ES : 0);          // scalar columns in front of the first 16-byte boundary
        const int nvec = (V1 - head) / VEC;
        const int tail0 = head + nvec * VEC;
        float best = -INFINITY;
        int idx = CGD_NONE, first = CGD_NONE;                           // first: the lowest column this thread reads
        if (tid < head) {
            first = tid;
            const float v = BF ? bfbits2f(reinterpret_cast<const unsigned short*>(p)[tid]) : reinterpret_cast<const float*>(p)[tid];
            cgd_take(v, tid, best, idx);
        }
        const uint4* pv = reinterpret_cast<const uint4*>(p + head * ES);
        if (tid < nvec) first = min(first, head + tid * VEC);
        auto take_vec = [&](const uint4 q, int i0) {
            if (BF) {
                cgd_take(__uint_as_float(q.x << 16), i0, best, idx);
                cgd_take(__uint_as_float(q.x & 0xffff0000u), i0 + 1, best, idx);
                cgd_take(__uint_as_float(q.y << 16), i0 + 2, best, idx);
                cgd_take(__uint_as_float(q.y & 0xffff0000u), i0 + 3, best, idx);
                cgd_take(__uint_as_float(q.z << 16), i0 + 4, best, idx);
                cgd_take(__uint_as_float(q.z & 0xffff0000u), i0 + 5, best, idx);
                cgd_take(__uint_as_float(q.w << 16), i0 + 6, best, idx);
                cgd_take(__uint_as_float(q.w & 0xffff0000u), i0 + 7, best, idx);
            } else {
                cgd_take(__uint_as_float(q.x), i0, best, idx);
                cgd_take(__uint_as_float(q.y), i0 + 1, best, idx);
                cgd_take(__uint_as_float(q.z), i0 + 2, best, idx);
                cgd_take(__uint_as_float(q.w), i0 + 3, best, idx);
            }
        };
        int j = tid;
        for (; j + 3 * CGD_BLOCK < nvec; j += 4 * CGD_BLOCK) {         // four 16-byte loads in flight per lane
            const uint4 q0 = pv[j], q1 = pv[j + CGD_BLOCK], q2 = pv[j + 2 * CGD_BLOCK], q3 = pv[j + 3 * CGD_BLOCK];
            take_vec(q0, head + j * VEC);
            take_vec(q1, head + (j + CGD_BLOCK) * VEC);
            take_vec(q2, head + (j + 2 * CGD_BLOCK) * VEC);
            take_vec(q3, head + (j + 3 * CGD_BLOCK) * VEC);
        }
        for (; j < nvec; j += CGD_BLOCK) take_vec(pv[j], head + j * VEC);
        if (tail0 + tid < V1) {                                         // fewer than VEC columns
            const int i = tail0 + tid;
            first = min(first, i);
            const float v = BF ? bfbits2f(reinterpret_cast<const unsigned short*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
            cgd_take(v, i, best, idx);
        }
        if (idx == CGD_NONE) idx = first;                               // nothing above -inf: the first column read (or none)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(best, o, 64);
            const int i2 = __shfl_xor(idx, o, 64);
            cgd_merge(v2, i2, best, idx);
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = idx; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < CGD_BLOCK / 64; ++w) cgd_merge(red_v[w], red_i[w], best, idx);
            ws[row] = (idx >= 0 && idx < V1) ? idx : 0;
        }
        __syncthreads();                                                // red_* are rewritten by the next row
    }
}

__global__ void __launch_bounds__(CGD_BLOCK) ctc_greedy_compact_kernel(const int* __restrict__ ws, int Tn, int64_t blank, int64_t pad_id,
                                                                       int64_t* __restrict__ out, int64_t out_stride) {
    __shared__ int wave_n[2][CGD_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* ids = ws + (int64_t)blockIdx.x * Tn;
    int64_t* o = out + (int64_t)blockIdx.x * out_stride;
    int count = 0;                                                      // ids kept so far (uniform over the workgroup)
    for (int t0 = 0, it = 0; t0 < Tn; t0 += CGD_BLOCK, ++it) {
        const int t = t0 + tid;
        int id = 0;
        bool keep = false;
        if (t < Tn) {
            id = ids[t];
            keep = (int64_t)id != blank && (t == 0 || id != ids[t - 1]);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[it & 1][wave] = __popcll(m);
        __syncthreads();                                                // (two buffers: a wave may be one tile ahead of the slowest)
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CGD_BLOCK / 64; ++w) {
            const int n = wave_n[it & 1][w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (keep) o[count + before + __popcll(m & ((1ull << lane) - 1ull))] = id;
        count += total;
    }
    for (int t = count + tid; t < Tn; t += CGD_BLOCK) o[t] = pad_id;
}

extern "C" int dicow_ctc_greedy_decode(const void* logits, int in_bf16, int64_t batch_stride, int64_t ld, int B, int Tn, int V1,
                                       int64_t blank, int64_t pad_id, int* ws, int64_t* out, int64_t out_stride, void* stream) {
    DICOW_REQUIRE(logits && ws && out, "ctc_greedy_decode: null pointer");
    DICOW_REQUIRE(B > 0 && Tn > 0 && V1 > 0 && (int64_t)B * Tn < (1ll << 31), "ctc_greedy_decode: bad sizes B=%d Tn=%d V1=%d", B, Tn, V1);
    DICOW_REQUIRE(ld >= V1 && batch_stride >= 0 && out_stride >= Tn, "ctc_greedy_decode: bad strides ld=%lld batch_stride=%lld out_stride=%lld",
                  (long long)ld, (long long)batch_stride, (long long)out_stride);
    DICOW_REQUIRE(dicow_aligned(in_bf16 ? 2 : 4, logits), "ctc_greedy_decode: logits not aligned to their element size");
    const int64_t rows = (int64_t)B * Tn;
    const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));
    if (in_bf16) ctc_greedy_argmax_kernel<1><<<grid, CGD_BLOCK, 0, (hipStream_t)stream>>>(logits, batch_stride, ld, Tn, V1, rows, ws);
    else ctc_greedy_argmax_kernel<0><<<grid, CGD_BLOCK, 0, (hipStream_t)stream>>>(logits, batch_stride, ld, Tn, V1, rows, ws);
    DICOW_CHECK_LAUNCH("ctc_greedy_argmax_kernel");
    ctc_greedy_compact_kernel<<<B, CGD_BLOCK, 0, (hipStream_t)stream>>>(ws, Tn, blank, pad_id, out, out_stride);
    DICOW_CHECK_LAUNCH("ctc_greedy_compact_kernel");
    return DICOW_OK;
}

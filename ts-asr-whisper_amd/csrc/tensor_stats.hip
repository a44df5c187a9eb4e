// Per-tensor statistics and histograms over a multi-tensor table (include/dicow_hip.h "tensor statistics"; the table is the one of
// optim.hip: dicow_mt_tensor[] + dicow_mt_chunk[]).  This is the device side of watch.py (the reference's `watch_grads`:
// src/utils/trainers.py:19-28 -> wandb.watch(log='all'): per parameter and per gradient, non-finite values dropped, min / max,
// torch.histc(bins, min, max)).  Three launches, no host read between them:
//   A  ts_chunk_kernel : ONE WAVE per table chunk (2048 elements: eight float4 per lane in flight, then one wave reduction): min / max /
//                        absmax, the four counts and the two double partials of the chunk go to the chunk's own 48-byte slot of the
//                        workspace.  A slot depends on its chunk's data alone.
//   B  ts_fold_kernel  : one wave per tensor folds the tensor's slots [first_chunk[t], first_chunk[t + 1]) in index order (the double
//                        partials as one serial chain: the bits depend on the data and the table only, never on a grid), writes the
//                        64-byte record and zeroes the tensor's histogram row.
//   C  ts_hist_kernel  : reads min / max from the records and bins.  A workgroup takes contiguous runs of TS_RUN_CHUNKS chunks (few
//                        tensor boundaries per run), the runs strided over the grid; its counts live in LDS as one private column
//                        per lane ([bin][lane], 16-bit counters: no atomics and no same-address serialisation in the inner loop,
//                        however concentrated the values are -- gradients sit in a few central bins) and are flushed with 64-bit
//                        integer adds once per run and tensor, long before a counter can wrap (a lane adds at most 8 per chunk).
//                        Run length, measured on the headline list (profiles/tensor_stats.txt): ONE long run per workgroup (1024
//                        streams 2.4 MB apart) reads at 1.4 TB/s -- each wave waited ~6 us for its loads, whatever the inner loop
//                        did; runs of 16 chunks (the grid's window in flight 128 MiB wide) at 4.2 TB/s; runs of 4 or 64 at 3.2 TB/s.
// Counts are integers: every summation order gives the same histogram.  No float atomics anywhere; no workspace state survives a call.
// A tensor whose column pointer is 16-byte aligned runs on float4 loads, its count % 4 tail and every misaligned tensor (a
// Parameter can be an offset view) on the scalar path, as in multi_sumsq_kernel.
#include "common.h"
#include <float.h>

#define TS_BLOCK 256
#define TS_WAVES (TS_BLOCK / 64)
#define TS_GRID_MAX 2048
#define TS_RUN_CHUNKS 16              // pass C: chunks per contiguous run of a workgroup (128 KiB)
#define TS_CU_LDS_BYTES (160 * 1024)  // gfx950: LDS per CU
#define TS_CUS 256
static_assert(DICOW_MT_CHUNK == 64 * 4 * 8, "pass A: a chunk is eight float4 per lane of ONE wave");
static_assert(DICOW_MT_CHUNK == TS_BLOCK * 4 * 2, "pass C: a chunk is two float4 per lane of a workgroup");
static_assert(sizeof(dicow_tensor_stats_rec) == 64, "dicow_tensor_stats_rec is 64 bytes");
static_assert(TS_RUN_CHUNKS * (DICOW_MT_CHUNK / TS_BLOCK) < 65536, "a 16-bit column is flushed once per run: it must not wrap inside one");

struct ts_slot {                      // one per table chunk
    double sum, sumsq;
    float mn, mx, amax;
    int n_nan, n_pinf, n_ninf, n_zero;
    int pad;
};
static_assert(sizeof(ts_slot) == 48, "ts_slot is 48 bytes");

__device__ __forceinline__ const float* ts_column(const dicow_mt_tensor& t, int which) {
    return which == 0 ? t.p : which == 1 ? t.g : which == 2 ? t.m : t.v;
}
// The column pointers come out of the device table, so hipcc sees generic pointers and emits flat loads, which it cannot tell from LDS
// traffic when it places its waits (every wait becomes vmcnt(0) lgkmcnt(0): no load stays in flight across the binning).  The
// tensors are global memory: say so.
typedef const float __attribute__((address_space(1)))* ts_gf32;
typedef const f32x4_t __attribute__((address_space(1)))* ts_gf32x4;
__device__ __forceinline__ bool ts_finite(float x) { return fabsf(x) <= FLT_MAX; }      // false for NaN and both infinities

struct ts_acc {
    double s, q;
    float mn, mx, am;
    int n_nan, n_pinf, n_ninf, n_zero;
    __device__ __forceinline__ void init() { s = 0.0; q = 0.0; mn = INFINITY; mx = -INFINITY; am = 0.f; n_nan = n_pinf = n_ninf = n_zero = 0; }
    __device__ __forceinline__ void add(float x) {
        if (ts_finite(x)) {
            mn = fminf(mn, x); mx = fmaxf(mx, x); am = fmaxf(am, fabsf(x));
            const double d = (double)x;
            s += d; q += d * d;                                    // d * d is exact in double: a contraction changes nothing
            n_zero += x == 0.f;
        } else {
            n_nan += x != x; n_pinf += x == INFINITY; n_ninf += x == -INFINITY;
        }
    }
};

// ---- pass A
__global__ void __launch_bounds__(TS_BLOCK) ts_chunk_kernel(const dicow_mt_tensor* __restrict__ tensors, const dicow_mt_chunk* __restrict__ chunks,
                                                            int64_t n_chunks, int which, ts_slot* __restrict__ slots) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t k = (int64_t)blockIdx.x * TS_WAVES + wave; k < n_chunks; k += (int64_t)gridDim.x * TS_WAVES) {
        const dicow_mt_chunk ch = chunks[k];
        const dicow_mt_tensor t = tensors[ch.tensor];
        const float* col = ts_column(t, which);
        const int len = col ? ch.len : 0;                          // (a NULL column holds nothing: the host refuses it, the kernel must not read it)
        const ts_gf32 x = (ts_gf32)(col + ch.start);
        ts_acc a;
        a.init();
        int done = 0;
        if (((uintptr_t)col & 15) == 0) {                          // chunk starts are multiples of 2048 elements: x is aligned when col is
            const int n4 = len >> 2;
            const ts_gf32x4 x4 = (ts_gf32x4)x;
            f32x4_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (lane + 64 * j < n4) v[j] = x4[lane + 64 * j];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (lane + 64 * j < n4) { a.add(v[j][0]); a.add(v[j][1]); a.add(v[j][2]); a.add(v[j][3]); }
            done = n4 << 2;
        }
        for (int i = done + lane; i < len; i += 64) a.add(x[i]);
        int c0 = a.n_nan | (a.n_pinf << 16), c1 = a.n_ninf | (a.n_zero << 16);       // at most 2048 each per wave: 16 bits hold them
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a.s += __shfl_xor(a.s, o, 64); a.q += __shfl_xor(a.q, o, 64);
            a.mn = fminf(a.mn, __shfl_xor(a.mn, o, 64)); a.mx = fmaxf(a.mx, __shfl_xor(a.mx, o, 64)); a.am = fmaxf(a.am, __shfl_xor(a.am, o, 64));
            c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64);
        }
        if (lane == 0) {
            ts_slot s;
            s.sum = a.s; s.sumsq = a.q; s.mn = a.mn; s.mx = a.mx; s.amax = a.am;
            s.n_nan = c0 & 0xffff; s.n_pinf = (c0 >> 16) & 0xffff; s.n_ninf = c1 & 0xffff; s.n_zero = (c1 >> 16) & 0xffff;
            s.pad = 0;
            slots[k] = s;
        }
    }
}

// ---- pass B
__device__ __forceinline__ double ts_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__global__ void __launch_bounds__(TS_BLOCK) ts_fold_kernel(const ts_slot* __restrict__ slots, const int64_t* __restrict__ first_chunk, int64_t n_tensors,
                                                           int bins, dicow_tensor_stats_rec* __restrict__ out, int64_t* __restrict__ hist) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t t = (int64_t)blockIdx.x * TS_WAVES + wave; t < n_tensors; t += (int64_t)gridDim.x * TS_WAVES) {
        const int64_t c0 = first_chunk[t], c1 = first_chunk[t + 1];
        double s = 0.0, q = 0.0;                                   // the serial chain, identical in every lane
        float mn = INFINITY, mx = -INFINITY, am = 0.f;
        long long n_nan = 0, n_pinf = 0, n_ninf = 0, n_zero = 0;
        for (int64_t base = c0; base < c1; base += 64) {
            const int cnt = __builtin_amdgcn_readfirstlane((int)(c1 - base < 64 ? c1 - base : 64));
            double ps = 0.0, pq = 0.0;
            if (lane < cnt) {
                const ts_slot sl = slots[base + lane];
                ps = sl.sum; pq = sl.sumsq;
                mn = fminf(mn, sl.mn); mx = fmaxf(mx, sl.mx); am = fmaxf(am, sl.amax);
                n_nan += sl.n_nan; n_pinf += sl.n_pinf; n_ninf += sl.n_ninf; n_zero += sl.n_zero;
            }
            for (int j = 0; j < cnt; ++j) { s += ts_readlane(ps, j); q += ts_readlane(pq, j); }     // chunk order
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); am = fmaxf(am, __shfl_xor(am, o, 64));
            n_nan += __shfl_xor(n_nan, o, 64); n_pinf += __shfl_xor(n_pinf, o, 64);
            n_ninf += __shfl_xor(n_ninf, o, 64); n_zero += __shfl_xor(n_zero, o, 64);
        }
        if (lane == 0) {
            dicow_tensor_stats_rec r;
            r.sum = s; r.sumsq = q; r.min = mn; r.max = mx; r.absmax = am; r.reserved = 0;
            r.n_nan = n_nan; r.n_posinf = n_pinf; r.n_neginf = n_ninf; r.n_zero = n_zero;
            out[t] = r;
        }
        for (int b = lane; b < bins; b += 64) hist[t * bins + b] = 0;                               // the call overwrites, pass C adds
    }
}

// ---- pass C
struct ts_binner {
    float lo, width, fb, scale;
    int last;
    bool any;                         // false: no finite element (min = +inf, max = -inf)
    // Branch-free form of the header's rule: min == max -> width 1, so (x - min) * bins / 1 = 0 for every finite x (they all equal
    // min); max - min overflows -> scale 1/2 (x * 1 and x / 2 are exact, denormal results aside, which the oracle rounds alike).
    __device__ __forceinline__ void set(float mn, float mx, int bins) {
        fb = (float)bins; last = bins - 1; any = mn <= mx; lo = mn; width = mx - mn; scale = 1.f;
        if (!(width > 0.f)) width = 1.f;
        else if (!ts_finite(width)) { scale = 0.5f; lo = mn * 0.5f; width = mx * 0.5f - lo; }
    }
    // multiply, then divide: the order device torch.histc evaluates (profiles/tensor_stats.txt: the other order moves elements across
    // edges for bin counts that are no power of two).  Every operation rounds to fp32; the division is the correctly rounded one.  A
    // quotient at or past `bins` (the top edge, or +inf where (x - min) * bins overflows) lands in the last bin: min(bins - 1, (int)q)
    // with a saturating conversion.  Any x, finite or not, gives an index inside [0, bins).
    __device__ __forceinline__ int bin(float x) const {
#pragma clang fp contract(off)                                     // x * scale - lo must stay two roundings
        const float qv = (x * scale - lo) * fb / width;
        const int b = (int)qv;
        return qv >= fb ? last : b < 0 ? 0 : b;
    }
};

// The counters: cnt[bin][lane] as 16-bit halves of dwords: lane l owns half (l >> 7) of dword [bin][l & 127], so the 32 lanes an LDS
// instruction serves together sit on 32 different banks whatever their bins are, and only lanes of different waves share a dword.
#define TS_ROW (TS_BLOCK / 2)
__device__ __forceinline__ void ts_count(unsigned* cnt, const ts_binner& bn, float x, int half, int slot) {
    unsigned short* p = reinterpret_cast<unsigned short*>(cnt + bn.bin(x) * TS_ROW + slot) + half;
    *p = (unsigned short)(*p + (ts_finite(x) ? 1 : 0));            // a non-finite element adds 0
}

// The workgroup's counts since the last flush -> hist row of the tensor (64-bit integer adds), counters zeroed again.  Two threads
// per bin, 64 dwords (128 lanes' counters) each, rotated by the thread index: 64 lanes on 64 banks.
__device__ __forceinline__ void ts_flush(unsigned* cnt, int bins, int64_t* __restrict__ row) {
    __syncthreads();
    const int b = threadIdx.x >> 1, h = threadIdx.x & 1;
    unsigned total = 0;
    if (b < bins) {
        unsigned* w = cnt + b * TS_ROW + h * 64;
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {
            const int jj = (j + threadIdx.x) & 63;
            const unsigned v = w[jj];
            total += (v & 0xffffu) + (v >> 16);
            w[jj] = 0u;
        }
    }
    total += __shfl_xor(total, 1, 64);
    if (h == 0 && b < bins && total) atomicAdd(reinterpret_cast<unsigned long long*>(row + b), (unsigned long long)total);
    __syncthreads();
}

// The chunks of a tensor are consecutive in the table: chunk k of tensor t starts at element (k - first_chunk[t]) * DICOW_MT_CHUNK.  The
// kernel walks a run by that arithmetic (ONE chunk descriptor read per run, one tensor descriptor per tensor it meets).  With 32 to
// 64 KiB of LDS per workgroup there is little occupancy to hide latency behind, so the loop over the full chunks of an aligned tensor
// requests the next chunk's two float4 before it bins the current one, with nothing conditional between the loads; partial chunks
// and misaligned tensors take the plain path.  One flush per (run, tensor): at most TS_RUN_CHUNKS * 8 increments per counter.
__global__ void __launch_bounds__(TS_BLOCK) ts_hist_kernel(const dicow_mt_tensor* __restrict__ tensors, const dicow_mt_chunk* __restrict__ chunks,
                                                           int64_t n_chunks, const int64_t* __restrict__ first_chunk, int64_t n_tensors, int which,
                                                           int bins, const dicow_tensor_stats_rec* __restrict__ recs, int64_t* __restrict__ hist) {
    extern __shared__ unsigned ts_cnt[];                           // [bins][TS_ROW]
    for (int i = threadIdx.x; i < bins * TS_ROW; i += TS_BLOCK) ts_cnt[i] = 0u;
    __syncthreads();
    const int half = threadIdx.x >> 7, slot = threadIdx.x & (TS_ROW - 1);     // this lane's counters: half `half` of dword [bin][slot]
    for (int64_t k0 = (int64_t)blockIdx.x * TS_RUN_CHUNKS; k0 < n_chunks; k0 += (int64_t)gridDim.x * TS_RUN_CHUNKS) {
        const int64_t k1 = k0 + TS_RUN_CHUNKS < n_chunks ? k0 + TS_RUN_CHUNKS : n_chunks;
        int64_t k = k0, t = chunks[k0].tensor;
        while (k < k1 && t < n_tensors) {                          // everything that steers these loops is workgroup-uniform
            const int64_t f0 = first_chunk[t], f1 = first_chunk[t + 1];
            if (f1 <= k) { ++t; continue; }                        // (an empty tensor)
            const int64_t kend = f1 < k1 ? f1 : k1;
            ts_binner bn;
            bn.set(recs[t].min, recs[t].max, bins);
            if (bn.any) {                                          // else nothing finite in this tensor (or a NULL column): nothing to count
                const dicow_mt_tensor td = tensors[t];
                const float* __restrict__ col = ts_column(td, which);
                int64_t kk = k;
                if (((uintptr_t)col & 15) == 0) {
                    const int64_t n_full = td.n / DICOW_MT_CHUNK;  // chunks [f0, f0 + n_full) of the tensor are full
                    const int64_t kfull = f0 + n_full < kend ? f0 + n_full : kend;
                    if (kk < kfull) {
                        ts_gf32x4 x4 = (ts_gf32x4)(col + (kk - f0) * DICOW_MT_CHUNK) + threadIdx.x;
                        f32x4_t a = x4[0], b = x4[TS_BLOCK];
                        for (; kk < kfull; ++kk) {
                            const ts_gf32x4 nx = kk + 1 < kfull ? x4 + 2 * TS_BLOCK : x4;     // (the last trip reads its own chunk again)
                            const f32x4_t na = nx[0], nb = nx[TS_BLOCK];
#pragma unroll
                            for (int e = 0; e < 4; ++e) { ts_count(ts_cnt, bn, a[e], half, slot); ts_count(ts_cnt, bn, b[e], half, slot); }
                            a = na; b = nb; x4 = nx;
                        }
                    }
                }
                for (; kk < kend; ++kk) {                          // misaligned tensors; the tensor's partial last chunk
                    const int64_t start = (kk - f0) * DICOW_MT_CHUNK, rem = td.n - start;
                    const int len = (int)(rem < DICOW_MT_CHUNK ? (rem < 0 ? 0 : rem) : DICOW_MT_CHUNK);
                    const ts_gf32 x = (ts_gf32)(col + start);
                    for (int i = threadIdx.x; i < len; i += TS_BLOCK) ts_count(ts_cnt, bn, x[i], half, slot);
                }
                ts_flush(ts_cnt, bins, hist + t * bins);
            }
            k = kend;
            ++t;
        }
    }
}

// ---- host
static int64_t ts_round256(int64_t b) { return (b + 255) / 256 * 256; }

extern "C" int64_t dicow_tensor_stats_ws_bytes(int64_t n_tensors, int64_t n_chunks, int bins) {
    (void)n_tensors; (void)bins;
    return n_chunks <= 0 ? 0 : ts_round256(n_chunks * (int64_t)sizeof(ts_slot));
}

extern "C" int dicow_tensor_stats_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_tensors, int64_t n_chunks,
                                      const int64_t* first_chunk, int which, int bins, void* ws, int64_t ws_bytes,
                                      dicow_tensor_stats_rec* out, int64_t* hist, int grid, void* stream) {
    DICOW_REQUIRE(bins >= 0 && bins <= DICOW_STATS_MAX_BINS, "tensor_stats_f32: bins %d outside 0 (no histogram) .. DICOW_STATS_MAX_BINS = %d", bins,
                  DICOW_STATS_MAX_BINS);
    DICOW_REQUIRE(which >= 0 && which <= 3, "tensor_stats_f32: which %d outside 0..3 (p, g, m, v)", which);
    DICOW_REQUIRE(n_tensors >= 0 && n_tensors <= 0x7fffffffLL && n_chunks >= 0 && n_chunks <= 0x7fffffffLL && grid >= 0 && grid <= 65535,
                  "tensor_stats_f32: bad sizes (n_tensors %lld, n_chunks %lld, grid %d; limits 2^31 - 1, 2^31 - 1, 65535)", (long long)n_tensors,
                  (long long)n_chunks, grid);
    if (n_tensors == 0) return DICOW_OK;
    DICOW_REQUIRE(tensors && first_chunk && out && (n_chunks == 0 || chunks), "tensor_stats_f32: NULL table, first_chunk or out");
    DICOW_REQUIRE(bins == 0 || hist, "tensor_stats_f32: hist is NULL with bins %d", bins);
    const int64_t need = dicow_tensor_stats_ws_bytes(n_tensors, n_chunks, bins);
    DICOW_REQUIRE(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0),
                  "tensor_stats_f32: workspace of %lld bytes (16-byte aligned) needed, %lld given", (long long)need, (long long)ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    ts_slot* slots = (ts_slot*)ws;
    if (n_chunks > 0) {
        const int64_t want = (n_chunks + TS_WAVES - 1) / TS_WAVES;
        const unsigned ga = grid > 0 ? (unsigned)grid : (unsigned)(want < TS_GRID_MAX ? want : TS_GRID_MAX);
        hipLaunchKernelGGL(ts_chunk_kernel, dim3(ga), dim3(TS_BLOCK), 0, st, tensors, chunks, n_chunks, which, slots);
        DICOW_CHECK_LAUNCH("tensor_stats_f32 (chunks)");
    }
    {
        const int64_t want = (n_tensors + TS_WAVES - 1) / TS_WAVES;
        const unsigned gb = grid > 0 ? (unsigned)grid : (unsigned)(want < TS_GRID_MAX ? want : TS_GRID_MAX);
        hipLaunchKernelGGL(ts_fold_kernel, dim3(gb), dim3(TS_BLOCK), 0, st, slots, first_chunk, n_tensors, bins, out, hist);
        DICOW_CHECK_LAUNCH("tensor_stats_f32 (fold)");
    }
    if (bins > 0 && n_chunks > 0) {
        const size_t lds = (size_t)bins * TS_ROW * sizeof(unsigned);
        int per_cu = (int)(TS_CU_LDS_BYTES / (lds + 512));
        per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
        const int64_t cap = (int64_t)TS_CUS * per_cu, want = (n_chunks + TS_RUN_CHUNKS - 1) / TS_RUN_CHUNKS;     // one workgroup per run at most
        const unsigned gc = grid > 0 ? (unsigned)grid : (unsigned)(want < cap ? want : cap);
        hipLaunchKernelGGL(ts_hist_kernel, dim3(gc), dim3(TS_BLOCK), lds, st, tensors, chunks, n_chunks, first_chunk, n_tensors, which, bins, out, hist);
        DICOW_CHECK_LAUNCH("tensor_stats_f32 (histogram)");
    }
    return DICOW_OK;
}

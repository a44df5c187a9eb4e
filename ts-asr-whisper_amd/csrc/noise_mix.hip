// Background-noise mixing on waveforms resident in HBM (the recipe's musan_augment_prob; reference RandomBackgroundNoise.__call__,
// src/data/augmentations.py:395-429, gated at src/data/local_datasets.py:205-206), ahead of dicow_logmel.
//
// Per planned row p = (row, clip, offset, len), snr:   n[i] = clip[offset + i] while offset + i < clip_len, else 0
//     scale = ||a|| / (snr * ||n||)   (0 when ||n|| == 0: the reference divides by zero there)      out[i] = (a[i] + scale n[i]) / 2,  i < len
// Two launches over the same grid (NMX_PARTS, n_plan), no atomics, no host read, nothing allocated:
//   1. noise_mix_sumsq_kernel   a row is cut into at most NMX_PARTS ranges of `span` samples, span = the smallest multiple of
//                               DICOW_NOISE_MIX_CHUNK that covers `len` with NMX_PARTS ranges (one chunk per workgroup up to 64 chunks = 32.8 s;
//                               longer rows grow the range, not the partial count).  Workgroup (part, p) sums a^2 and n^2 over its range in
//                               fp64 -- lanes take 16-byte vectors at a 256-lane stride, then a 64-lane butterfly, then the four waves in
//                               order -- and stores the two sums in slot (p, part) of the workspace.
//   2. noise_mix_apply_kernel   every wave of every workgroup adds the row's slots in ascending order by the same 64-leaf butterfly (lane =
//                               slot, unused slots count 0), so all of them derive the same scale; then out = fma(scale, n, a) * 0.5f.
// The split depends on the row's own `len` only and every slot is written by exactly one workgroup, so a row's result is a function of that
// row's inputs: bit-identical from run to run and whatever else is in the plan.
// Audio and output rows are 16-byte aligned (checked) and move as float4; the crop starts at any 4-byte boundary of the bank, so its
// vectors are 4-byte-aligned 16-byte loads (legal for global memory on gfx950).  A vector is used only where all four samples lie inside
// both [0, len) and the clip; the up-to-three samples behind the last whole vector of a row, and vectors that straddle the end of the
// clip, go element by element.  Nothing outside [0, len) of a row is written, nothing outside the clip is read.
// out == wave is legal: pass 1 only reads, and pass 2 reads each sample in the thread that then writes it.
#include "host_table.h"

#define NMX_BLOCK 256
#define NMX_PARTS 64                     // partial slots per row = lanes of the re-sum butterfly
#define NMX_SLOT_BYTES (NMX_PARTS * 2 * (int64_t)sizeof(double))

struct __attribute__((packed, aligned(4))) nmx_f4u { float x, y, z, w; };     // 16 bytes at 4-byte alignment

struct nmx_row {
    const float* a;          // audio row
    const float* c;          // clip + offset
    int len;                 // samples of the row that are mixed
    int navail;              // leading samples of the crop that exist in the clip (the rest is the zero padding)
    int i0, i1;              // this workgroup's range
    int parts;
};

// plan entry -> pointers and this workgroup's range; false: nothing to do (len <= 0, or a part behind the row's last)
__device__ __forceinline__ bool nmx_setup(const float* wave, int64_t ld_wave, const float* bank, const int64_t* clip_start, const int* clip_len,
                                          const int* plan_i, nmx_row& r) {
    const int* pl = plan_i + 4 * (int64_t)blockIdx.y;
    const int row = pl[0], clip = pl[1], off = pl[2];
    r.len = pl[3];
    if (r.len <= 0) return false;
    const int nchunks = (r.len + DICOW_NOISE_MIX_CHUNK - 1) / DICOW_NOISE_MIX_CHUNK;
    const int span = (nchunks + NMX_PARTS - 1) / NMX_PARTS * DICOW_NOISE_MIX_CHUNK;
    r.parts = (int)(((int64_t)r.len + span - 1) / span);
    if ((int)blockIdx.x >= r.parts) return false;
    r.i0 = (int)blockIdx.x * span;                                     // < len
    r.i1 = (int)min((int64_t)r.len, (int64_t)r.i0 + span);
    const int clen = clip_len[clip];
    r.navail = off < 0 ? 0 : max(0, min(r.len, clen - off));           // (a bad offset reads nothing)
    r.a = wave + (int64_t)row * ld_wave;
    r.c = bank + clip_start[clip] + (off < 0 ? 0 : off);
    return true;
}

__device__ __forceinline__ float4 nmx_noise4(const nmx_row& r, int i) {
    if (i + 4 <= r.navail) {
        const nmx_f4u q = *reinterpret_cast<const nmx_f4u*>(r.c + i);
        return make_float4(q.x, q.y, q.z, q.w);
    }
    float4 n;
    n.x = i < r.navail ? r.c[i] : 0.f;
    n.y = i + 1 < r.navail ? r.c[i + 1] : 0.f;
    n.z = i + 2 < r.navail ? r.c[i + 2] : 0.f;
    n.w = i + 3 < r.navail ? r.c[i + 3] : 0.f;
    return n;
}

__device__ __forceinline__ double nmx_butterfly(double v) {             // the fixed 64-leaf tree; every lane ends with the same bits
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(NMX_BLOCK) noise_mix_sumsq_kernel(const float* __restrict__ wave, int64_t ld_wave, const float* __restrict__ bank,
                                                                    const int64_t* __restrict__ clip_start, const int* __restrict__ clip_len,
                                                                    const int* __restrict__ plan_i, double* __restrict__ ws) {
    __shared__ double red[2][NMX_BLOCK / 64];
    nmx_row r;
    if (!nmx_setup(wave, ld_wave, bank, clip_start, clip_len, plan_i, r)) return;
    const int tid = threadIdx.x;
    const int nvec = (r.i1 - r.i0) >> 2;                                // i0 is a multiple of the chunk, hence of 4
    double sa = 0.0, sn = 0.0;
    auto take = [&](const float4 a, const float4 n) {
        sa = fma((double)a.x, (double)a.x, sa); sa = fma((double)a.y, (double)a.y, sa);
        sa = fma((double)a.z, (double)a.z, sa); sa = fma((double)a.w, (double)a.w, sa);
        sn = fma((double)n.x, (double)n.x, sn); sn = fma((double)n.y, (double)n.y, sn);
        sn = fma((double)n.z, (double)n.z, sn); sn = fma((double)n.w, (double)n.w, sn);
    };
    int j = tid;
    for (; j + 3 * NMX_BLOCK < nvec; j += 4 * NMX_BLOCK) {              // four 16-byte loads of each operand in flight per lane
        const int i = r.i0 + 4 * j;
        const float4 a0 = *reinterpret_cast<const float4*>(r.a + i), a1 = *reinterpret_cast<const float4*>(r.a + i + 4 * NMX_BLOCK);
        const float4 a2 = *reinterpret_cast<const float4*>(r.a + i + 8 * NMX_BLOCK), a3 = *reinterpret_cast<const float4*>(r.a + i + 12 * NMX_BLOCK);
        const float4 n0 = nmx_noise4(r, i), n1 = nmx_noise4(r, i + 4 * NMX_BLOCK);
        const float4 n2 = nmx_noise4(r, i + 8 * NMX_BLOCK), n3 = nmx_noise4(r, i + 12 * NMX_BLOCK);
        take(a0, n0); take(a1, n1); take(a2, n2); take(a3, n3);
    }
    for (; j < nvec; j += NMX_BLOCK) {
        const int i = r.i0 + 4 * j;
        take(*reinterpret_cast<const float4*>(r.a + i), nmx_noise4(r, i));
    }
    const int it = r.i0 + 4 * nvec + tid;                               // fewer than four samples, in the row's last range only
    if (it < r.i1) {
        const float a = r.a[it], n = it < r.navail ? r.c[it] : 0.f;
        sa = fma((double)a, (double)a, sa);
        sn = fma((double)n, (double)n, sn);
    }
    sa = nmx_butterfly(sa);
    sn = nmx_butterfly(sn);
    if ((tid & 63) == 0) { red[0][tid >> 6] = sa; red[1][tid >> 6] = sn; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < NMX_BLOCK / 64; ++w) { sa += red[0][w]; sn += red[1][w]; }
        double* slot = ws + ((int64_t)blockIdx.y * NMX_PARTS + blockIdx.x) * 2;
        slot[0] = sa;
        slot[1] = sn;
    }
}

__global__ void __launch_bounds__(NMX_BLOCK) noise_mix_apply_kernel(const float* wave, int64_t ld_wave, float* out, int64_t ld_out,
                                                                    const float* __restrict__ bank, const int64_t* __restrict__ clip_start,
                                                                    const int* __restrict__ clip_len, const int* __restrict__ plan_i,
                                                                    const float* __restrict__ plan_snr, const double* __restrict__ ws) {
    nmx_row r;
    if (!nmx_setup(wave, ld_wave, bank, clip_start, clip_len, plan_i, r)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const double* slot = ws + ((int64_t)blockIdx.y * NMX_PARTS + lane) * 2;
    const double sa = nmx_butterfly(lane < r.parts ? slot[0] : 0.0), sn = nmx_butterfly(lane < r.parts ? slot[1] : 0.0);
    const float na = (float)sqrt(sa), nn = (float)sqrt(sn);
    const float den = plan_snr[blockIdx.y] * nn;                        // the reference's order: the product first, then the division
    const float scale = nn == 0.f ? 0.f : na / den;
    float* o = out + (int64_t)plan_i[4 * (int64_t)blockIdx.y] * ld_out;
    const int nvec = (r.i1 - r.i0) >> 2;
    auto mix = [&](const float4 a, const float4 n) {
        return make_float4(fmaf(scale, n.x, a.x) * 0.5f, fmaf(scale, n.y, a.y) * 0.5f, fmaf(scale, n.z, a.z) * 0.5f, fmaf(scale, n.w, a.w) * 0.5f);
    };
    int j = tid;
    for (; j + 3 * NMX_BLOCK < nvec; j += 4 * NMX_BLOCK) {
        const int i = r.i0 + 4 * j;
        const float4 a0 = *reinterpret_cast<const float4*>(r.a + i), a1 = *reinterpret_cast<const float4*>(r.a + i + 4 * NMX_BLOCK);
        const float4 a2 = *reinterpret_cast<const float4*>(r.a + i + 8 * NMX_BLOCK), a3 = *reinterpret_cast<const float4*>(r.a + i + 12 * NMX_BLOCK);
        const float4 n0 = nmx_noise4(r, i), n1 = nmx_noise4(r, i + 4 * NMX_BLOCK);
        const float4 n2 = nmx_noise4(r, i + 8 * NMX_BLOCK), n3 = nmx_noise4(r, i + 12 * NMX_BLOCK);
        *reinterpret_cast<float4*>(o + i) = mix(a0, n0);
        *reinterpret_cast<float4*>(o + i + 4 * NMX_BLOCK) = mix(a1, n1);
        *reinterpret_cast<float4*>(o + i + 8 * NMX_BLOCK) = mix(a2, n2);
        *reinterpret_cast<float4*>(o + i + 12 * NMX_BLOCK) = mix(a3, n3);
    }
    for (; j < nvec; j += NMX_BLOCK) {
        const int i = r.i0 + 4 * j;
        *reinterpret_cast<float4*>(o + i) = mix(*reinterpret_cast<const float4*>(r.a + i), nmx_noise4(r, i));
    }
    const int it = r.i0 + 4 * nvec + tid;
    if (it < r.i1) {
        const float a = r.a[it], n = it < r.navail ? r.c[it] : 0.f;
        o[it] = fmaf(scale, n, a) * 0.5f;
    }
}

extern "C" int64_t dicow_noise_mix_ws_bytes(int n_plan, int max_len) {
    if (n_plan < 0 || max_len < 0) {
        dicow_set_error("noise_mix_ws_bytes: negative size n_plan=%d max_len=%d", n_plan, max_len);
        return -1;
    }
    return (int64_t)n_plan * NMX_SLOT_BYTES;      // (max_len does not enter: longer rows grow the range of a slot, not the slot count)
}

extern "C" int dicow_noise_mix(const float* wave, int64_t ld_wave, float* out, int64_t ld_out, const float* bank, const int64_t* clip_start,
                               const int* clip_len, const int* plan_i, const float* plan_snr, int n_plan, void* ws, int64_t ws_bytes,
                               void* stream) {
    DICOW_REQUIRE(n_plan >= 0, "noise_mix: negative n_plan=%d", n_plan);
    if (n_plan == 0) return DICOW_OK;
    DICOW_REQUIRE(wave && out && bank && clip_start && clip_len && plan_i && plan_snr && ws, "noise_mix: null pointer");
    DICOW_REQUIRE(n_plan <= 65535, "noise_mix: n_plan=%d exceeds 65535 rows per call", n_plan);
    DICOW_REQUIRE(ld_wave >= 0 && ld_out >= 0 && ld_wave % 4 == 0 && ld_out % 4 == 0, "noise_mix: row strides must be non-negative multiples of 4 "
                  "(ld_wave=%lld ld_out=%lld)", (long long)ld_wave, (long long)ld_out);
    DICOW_REQUIRE(dicow_aligned(16, wave, out), "noise_mix: wave / out not 16-byte aligned");
    DICOW_REQUIRE(dicow_aligned(4, bank) && dicow_aligned(8, ws), "noise_mix: bank / ws misaligned");
    DICOW_REQUIRE(out != wave || ld_out == ld_wave, "noise_mix: in place (out == wave) needs ld_out == ld_wave");
    DICOW_REQUIRE(ws_bytes >= (int64_t)n_plan * NMX_SLOT_BYTES, "noise_mix: ws_bytes=%lld, need %lld", (long long)ws_bytes,
                  (long long)((int64_t)n_plan * NMX_SLOT_BYTES));
    const dim3 grid(NMX_PARTS, n_plan);
    noise_mix_sumsq_kernel<<<grid, NMX_BLOCK, 0, (hipStream_t)stream>>>(wave, ld_wave, bank, clip_start, clip_len, plan_i, (double*)ws);
    DICOW_CHECK_LAUNCH("noise_mix_sumsq_kernel");
    noise_mix_apply_kernel<<<grid, NMX_BLOCK, 0, (hipStream_t)stream>>>(wave, ld_wave, out, ld_out, bank, clip_start, clip_len, plan_i, plan_snr,
                                                                        (const double*)ws);
    DICOW_CHECK_LAUNCH("noise_mix_apply_kernel");
    return DICOW_OK;
}

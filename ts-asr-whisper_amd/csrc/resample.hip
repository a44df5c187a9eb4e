// Any-rate audio intake on the GPU: windowed-sinc resampling with the channel mixdown fused into the staging, ahead of everything that
// wants mono fp32 at the model's rate (NoiseBank / EnrollmentBank / MeetingFrontEnd / dicow_logmel).  The arithmetic is
// torchaudio.functional.resample with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), which the reference applies to
// every noise clip (src/data/augmentations.py:401-407: torch.mean over the channels, then resample):
//     g = gcd(orig, new), o = orig / g, n = new / g;   y[j n + p] = sum_k h[p][k] x[j o + k - width],   x = 0 outside the segment
// The full bank h is [n][2 width + o], but the Hann window is clamped at +-6 zero crossings: all but one contiguous run per phase rounds
// to exactly 0 in fp32.  The host (ts-asr-whisper_amd/wave_intake.py) builds h in fp64, rounds it once, and hands over the compact bank:
// first[p] = the first tap of phase p's run and taps_t[s][p] = h[p][first[p] + s], s < S = the longest run, zero behind a shorter one.
//
// One launch resamples many segments (in_start, in_len, out_start) of flat buffers that share one (o, n).  A workgroup owns a tile of F
// whole output frames (F n samples) of one segment, found by a binary search over the segments' first-tile numbers:
//   1. it stages the input span the tile reads -- (Fa - 1) o + D + S mono fp32 values, D = max first - min first -- in LDS; positions
//      outside [0, in_len) of the segment become 0 and are never loaded.  fp32 mono, int16 mono and int16 stereo move as 16-byte loads
//      wherever a whole vector lies inside both the span and the segment (the LDS image is shifted by the span's misalignment so that
//      vectors stay vectors), element by element at the ragged ends; int16 with another channel count, or with one channel selected,
//      goes frame by frame.  int16 -> fp32 is sample / 32768, the integer channel sum (exact in fp32 up to 512 channels), one __fdiv_rn
//      by C: the bits of torch.mean(pcm / 32768, 0);
//   2. it stages the compact bank behind the span when the two fit the LDS budget together, and reads it from memory (tap-major, so a
//      wave reads consecutive phases from consecutive addresses) otherwise;
//   3. a thread takes one phase p of RSM_R frames of the tile, G = ceil(Fa / RSM_R) apart (a tap is read once for RSM_R products; lanes
//      with the same phase read the span o apart), and for each output  acc = 0; for s ascending: acc = fmaf(taps[p][s], x[..], acc).
// Every output sample has one writer and its sum has one order, so its bits do not depend on F, the grid, or what else is in the table.
// No atomics; the workspace holds the uploaded segment table and first[] only; one launch, capturable.  All sample positions are int64.
#include "host_table.h"
#include <algorithm>
#include <vector>

#define RSM_BLOCK 256
#define RSM_R 4                                              // frames per thread
#define RSM_LDS_FLOATS (DICOW_RESAMPLE_LDS_BYTES / 4)
#define RSM_BANK_LDS_FLOATS (RSM_LDS_FLOATS / 2)             // the bank goes to LDS when it takes at most half the budget
#define RSM_PAD 12                                           // LDS floats beside the span: its misalignment (below one 16-byte vector of
                                                             // int16, 7 frames) and the rounding of the image to whole vectors
#define RSM_TILE_OUTPUTS 4096                                // output samples per tile the default F aims at

enum { RSM_F32 = 0, RSM_I16_MONO = 1, RSM_I16_STEREO = 2, RSM_I16_ANY = 3 };

struct rsm_seg { int64_t in_start, in_len, out_start, tile0; };

struct rsm_args {
    const void* in;
    float* out;
    const float* taps_t;                                     // [S][n]
    const int* first;                                        // [n]
    const rsm_seg* segs;
    int n_segs, C, channel, o, n, S, F;
    int lo;                                                  // min first - width: the span of frame 0 starts at input position lo
    int fmin, D;                                             // min first, max first - min first
    int xs_floats;                                           // LDS floats in front of the bank
};

template <int MODE> struct rsm_in;
template <> struct rsm_in<RSM_F32> {
    static constexpr int FPV = 4, BPF = 4;                   // frames per 16-byte vector, bytes per frame
    static __device__ __forceinline__ float one(const void* in, int64_t g, int, int) { return static_cast<const float*>(in)[g]; }
    static __device__ __forceinline__ void vec(const void* p, float* x) {
        const float4 q = *static_cast<const float4*>(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    }
};
template <> struct rsm_in<RSM_I16_MONO> {
    static constexpr int FPV = 8, BPF = 2;
    static __device__ __forceinline__ float one(const void* in, int64_t g, int, int) { return (float)static_cast<const short*>(in)[g] * 0x1p-15f; }
    static __device__ __forceinline__ void vec(const void* p, float* x) {
        const int4 q = *static_cast<const int4*>(p);
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[2 * k] = (float)(short)(w[k] & 0xffff) * 0x1p-15f;
            x[2 * k + 1] = (float)(w[k] >> 16) * 0x1p-15f;
        }
    }
};
template <> struct rsm_in<RSM_I16_STEREO> {                  // the mean of two channels
    static constexpr int FPV = 4, BPF = 4;
    static __device__ __forceinline__ float pair(int w) { return __fdiv_rn((float)((int)(short)(w & 0xffff) + (w >> 16)) * 0x1p-15f, 2.0f); }
    static __device__ __forceinline__ float one(const void* in, int64_t g, int, int) { return pair(static_cast<const int*>(in)[g]); }
    static __device__ __forceinline__ void vec(const void* p, float* x) {
        const int4 q = *static_cast<const int4*>(p);
        x[0] = pair(q.x); x[1] = pair(q.y); x[2] = pair(q.z); x[3] = pair(q.w);
    }
};
template <> struct rsm_in<RSM_I16_ANY> {                     // any channel count: the mean (channel < 0) or one channel, frame by frame
    static constexpr int FPV = 1, BPF = 2;
    static __device__ __forceinline__ float one(const void* in, int64_t g, int C, int channel) {
        const short* f = static_cast<const short*>(in) + g * C;
        if (channel >= 0) return (float)f[channel] * 0x1p-15f;
        int sum = 0;
        for (int c = 0; c < C; ++c) sum += f[c];
        return __fdiv_rn((float)sum * 0x1p-15f, (float)C);   // |sum| <= 512 * 32768 = 2^24: exact
    }
    static __device__ __forceinline__ void vec(const void*, float*) {}
};

template <int MODE, bool TAPS_LDS>
__global__ void __launch_bounds__(RSM_BLOCK) resample_kernel(const rsm_args a) {
    using IN = rsm_in<MODE>;
    extern __shared__ __attribute__((aligned(16))) float rsm_lds[];
    float* xs = rsm_lds;
    float* tl = rsm_lds + a.xs_floats;
    const int tid = threadIdx.x;
    // ---- the segment of this tile: the last one whose first tile is not behind it (segments without tiles share their successor's number)
    int k = 0, hi = a.n_segs;
    while (k < hi) {
        const int mid = (k + hi) >> 1;
        if (a.segs[mid].tile0 <= (int64_t)blockIdx.x) k = mid + 1; else hi = mid;
    }
    const rsm_seg sg = a.segs[k - 1];
    const int o = a.o, n = a.n, S = a.S;
    const int64_t j0 = ((int64_t)blockIdx.x - sg.tile0) * a.F;                  // first frame of the tile
    const int64_t out_len = ((int64_t)n * sg.in_len + o - 1) / o;
    const int64_t nf = (out_len + n - 1) / n;                                   // frames of the segment; j0 < nf
    const int Fa = (int)min((int64_t)a.F, nf - j0);
    const int64_t qbase = j0 * o + a.lo;                                        // input position (in the segment) of span element 0
    const int span = (Fa - 1) * o + a.D + S;
    // ---- stage the span: element i at xs[i + sh], sh = frames from the last 16-byte boundary to the span's first frame
    const uintptr_t A = reinterpret_cast<uintptr_t>(a.in) + (uintptr_t)((sg.in_start + qbase) * IN::BPF);
    const int sh = IN::FPV == 1 ? 0 : (int)((A & 15) / IN::BPF);
    const int n_slots = (span + sh + IN::FPV - 1) / IN::FPV;
    for (int v = tid; v < n_slots; v += RSM_BLOCK) {
        const int i0 = v * IN::FPV - sh;
        const int64_t q0 = qbase + i0;
        bool whole = false;
        if constexpr (IN::FPV > 1) {
            whole = i0 >= 0 && i0 + IN::FPV <= span && q0 >= 0 && q0 + IN::FPV <= sg.in_len;
            if (whole) {
                float x[IN::FPV];
                IN::vec(static_cast<const char*>(a.in) + (sg.in_start + q0) * IN::BPF, x);
#pragma unroll
                for (int f = 0; f < IN::FPV; f += 4) *reinterpret_cast<float4*>(xs + v * IN::FPV + f) = make_float4(x[f], x[f + 1], x[f + 2], x[f + 3]);
            }
        }
        if (!whole) {
#pragma unroll
            for (int f = 0; f < IN::FPV; ++f) {
                const int i = i0 + f;
                const int64_t q = q0 + f;
                if (i >= 0 && i < span) xs[i + sh] = q >= 0 && q < sg.in_len ? IN::one(a.in, sg.in_start + q, a.C, a.channel) : 0.f;
            }
        }
    }
    if (TAPS_LDS) {
        const int nt = S * n, nt4 = nt >> 2;                                    // (taps_t is 16-byte aligned, xs_floats a multiple of 4)
        for (int v = tid; v < nt4; v += RSM_BLOCK) reinterpret_cast<float4*>(tl)[v] = reinterpret_cast<const float4*>(a.taps_t)[v];
        for (int v = 4 * nt4 + tid; v < nt; v += RSM_BLOCK) tl[v] = a.taps_t[v];
    }
    __syncthreads();
    // ---- one phase of RSM_R frames per thread and trip
    const int G = (Fa + RSM_R - 1) / RSM_R;
    const int items = G * n;
    const int64_t out_rem = out_len - j0 * n;                                   // samples of the segment from the tile's first on
    float* o_tile = a.out + sg.out_start + j0 * n;
    for (int w = tid; w < items; w += RSM_BLOCK) {
        const int wj = w / n, p = w - wj * n;
        const int fo = a.first[p] - a.fmin + sh;
        int xb[RSM_R];
        float acc[RSM_R];
#pragma unroll
        for (int r = 0; r < RSM_R; ++r) {
            xb[r] = min(wj + r * G, Fa - 1) * o + fo;                           // (a frame behind the tile repeats the last one; not stored)
            acc[r] = 0.f;
        }
        if (TAPS_LDS) {
            const float* tp = tl + p;
            for (int s = 0; s < S; ++s) {
                const float t = tp[s * n];
#pragma unroll
                for (int r = 0; r < RSM_R; ++r) acc[r] = fmaf(t, xs[xb[r] + s], acc[r]);
            }
        } else {
            const float* tp = a.taps_t + p;
            for (int s = 0; s < S; ++s) {
                const float t = tp[(int64_t)s * n];
#pragma unroll
                for (int r = 0; r < RSM_R; ++r) acc[r] = fmaf(t, xs[xb[r] + s], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RSM_R; ++r) {
            const int jj = wj + r * G;
            const int64_t m = (int64_t)jj * n + p;
            if (jj < Fa && m < out_rem) o_tile[m] = acc[r];
        }
    }
}

template <int MODE>
static void rsm_launch(bool taps_lds, int64_t tiles, size_t lds_bytes, hipStream_t st, const rsm_args& a) {
    if (taps_lds) resample_kernel<MODE, true><<<dim3((unsigned)tiles), RSM_BLOCK, lds_bytes, st>>>(a);
    else resample_kernel<MODE, false><<<dim3((unsigned)tiles), RSM_BLOCK, lds_bytes, st>>>(a);
}

static inline int64_t rsm_first_bytes(int n) { return ((int64_t)n * 4 + 7) / 8 * 8; }

extern "C" int64_t dicow_resample_ws_bytes(int n_segs, int n) {
    if (n_segs < 0 || n < 0) {
        dicow_set_error("resample_ws_bytes: negative size n_segs=%d n=%d", n_segs, n);
        return -1;
    }
    return (int64_t)n_segs * (int64_t)sizeof(rsm_seg) + rsm_first_bytes(n);
}

extern "C" int dicow_resample(const void* in, int in_int16, int C, int channel, int64_t in_frames, float* out, int64_t out_samples,
                              const float* taps_t, const int32_t* first, int o, int n, int width, int S, const int64_t* segs, int n_segs,
                              int frames_per_tile, void* ws, int64_t ws_bytes, void* stream) {
    DICOW_REQUIRE(n_segs >= 0, "resample: negative n_segs=%d", n_segs);
    DICOW_REQUIRE(o >= 1 && o <= DICOW_RESAMPLE_MAX_RATIO && n >= 1 && n <= DICOW_RESAMPLE_MAX_RATIO, "resample: reduced ratio o=%d n=%d outside "
                  "[1, DICOW_RESAMPLE_MAX_RATIO = %d]", o, n, DICOW_RESAMPLE_MAX_RATIO);
    DICOW_REQUIRE(width >= 0 && width <= (1 << 24) && S >= 1 && S <= 2 * width + o, "resample: width=%d S=%d outside 0 <= width, 1 <= S <= 2 width + o", width, S);
    DICOW_REQUIRE(in_int16 == 0 || in_int16 == 1, "resample: in_int16=%d is neither 0 nor 1", in_int16);
    DICOW_REQUIRE(in_int16 ? (C >= 1 && C <= DICOW_RESAMPLE_MAX_CHANNELS) : C == 1, "resample: C=%d (fp32 input is mono; int16 has 1..%d channels)",
                  C, DICOW_RESAMPLE_MAX_CHANNELS);
    DICOW_REQUIRE(channel >= -1 && channel < C, "resample: channel=%d outside [-1, %d)", channel, C);
    DICOW_REQUIRE(in_frames >= 0 && out_samples >= 0, "resample: negative buffer size in_frames=%lld out_samples=%lld", (long long)in_frames,
                  (long long)out_samples);
    DICOW_REQUIRE(frames_per_tile >= 0, "resample: negative frames_per_tile=%d", frames_per_tile);
    DICOW_REQUIRE(first, "resample: null first");
    int fmin = first[0], fmax = first[0];
    for (int p = 0; p < n; ++p) {
        DICOW_REQUIRE(first[p] >= 0 && first[p] < 2 * width + o, "resample: first[%d]=%d outside the %d taps of a phase", p, first[p], 2 * width + o);
        fmin = std::min(fmin, first[p]);
        fmax = std::max(fmax, first[p]);
    }
    // ---- the tile: F whole frames whose span, with the bank when it is small enough, fits the LDS budget
    const int D = fmax - fmin;
    const bool taps_lds = (int64_t)S * n <= RSM_BANK_LDS_FLOATS;
    const int64_t avail = RSM_LDS_FLOATS - RSM_PAD - (taps_lds ? (int64_t)S * n : 0);
    DICOW_REQUIRE((int64_t)D + S <= avail, "resample: one output frame of o=%d n=%d S=%d reads %lld input samples, which need %lld bytes of LDS: the limit "
                  "is DICOW_RESAMPLE_LDS_BYTES = %d", o, n, S, (long long)D + S, ((long long)D + S + RSM_PAD) * 4, DICOW_RESAMPLE_LDS_BYTES);
    const int64_t f_max = (avail - D - S) / o + 1;
    int64_t F = frames_per_tile > 0 ? frames_per_tile : std::min<int64_t>(f_max, (RSM_TILE_OUTPUTS + n - 1) / n);
    DICOW_REQUIRE(F <= f_max, "resample: frames_per_tile=%d exceeds the %lld frames that fit DICOW_RESAMPLE_LDS_BYTES = %d", frames_per_tile,
                  (long long)f_max, DICOW_RESAMPLE_LDS_BYTES);
    DICOW_REQUIRE(F * n <= (1 << 30), "resample: frames_per_tile=%d makes tiles of more than 2^30 samples (n=%d)", frames_per_tile, n);
    // ---- the segment table, on the host, before anything is launched
    DICOW_REQUIRE(n_segs == 0 || segs, "resample: null segment table");
    static thread_local std::vector<int64_t> stage;          // the uploaded image: [n_segs] rsm_seg, then first[n]
    static thread_local std::vector<std::pair<int64_t, int64_t>> spans;
    const int64_t tbytes = (int64_t)n_segs * (int64_t)sizeof(rsm_seg);
    stage.assign((size_t)((tbytes + rsm_first_bytes(n)) / 8), 0);
    spans.clear();
    int64_t tiles = 0;
    for (int k = 0; k < n_segs; ++k) {
        const int64_t in_start = segs[3 * (int64_t)k], in_len = segs[3 * (int64_t)k + 1], out_start = segs[3 * (int64_t)k + 2];
        DICOW_REQUIRE(in_len >= 0, "resample: segment %d has the negative input length %lld", k, (long long)in_len);
        DICOW_REQUIRE_SPAN(in_start, in_len, in_frames, "reads", "frames of the input", "resample: segment %d", k);
        const int64_t out_len = (n * in_len + o - 1) / o;    // (in_len < 2^63 / 2^20 is implied by any real buffer)
        DICOW_REQUIRE_SPAN(out_start, out_len, out_samples, "writes", "samples of the output", "resample: segment %d", k);
        if (out_len > 0) spans.emplace_back(out_start, out_start + out_len);
        int64_t* row = stage.data() + 4 * (int64_t)k;
        row[0] = in_start; row[1] = in_len; row[2] = out_start; row[3] = tiles;
        const int64_t nf = (out_len + n - 1) / n;
        tiles += (nf + F - 1) / F;
        DICOW_REQUIRE(tiles <= 0x7fffffff, "resample: more than 2^31 - 1 tiles in one call (segment %d)", k);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        DICOW_REQUIRE(spans[k].first >= spans[k - 1].second, "resample: two segments write overlapping output ranges [%lld, %lld) and [%lld, %lld)",
                      (long long)spans[k - 1].first, (long long)spans[k - 1].second, (long long)spans[k].first, (long long)spans[k].second);
    if (tiles == 0) return DICOW_OK;
    DICOW_REQUIRE(in && out && taps_t && ws, "resample: null pointer");
    DICOW_REQUIRE(dicow_aligned(in_int16 ? 2 : 4, in) && dicow_aligned(4, out), "resample: in / out not aligned to their element size");
    DICOW_REQUIRE(dicow_aligned(16, taps_t) && dicow_aligned(8, ws), "resample: taps_t not 16-byte or ws not 8-byte aligned");
    const int64_t need = tbytes + rsm_first_bytes(n);
    DICOW_REQUIRE(ws_bytes >= need, "resample: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)need);
    memcpy(reinterpret_cast<char*>(stage.data()) + tbytes, first, (size_t)n * 4);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dicow_upload("resample", ws, stage.data(), need, st)) return rc;
    rsm_args a;
    a.in = in; a.out = out; a.taps_t = taps_t;
    a.segs = reinterpret_cast<const rsm_seg*>(ws);
    a.first = reinterpret_cast<const int*>(static_cast<const char*>(ws) + tbytes);
    a.n_segs = n_segs; a.C = C; a.channel = channel; a.o = o; a.n = n; a.S = S; a.F = (int)F;
    a.lo = fmin - width; a.fmin = fmin; a.D = D;
    a.xs_floats = (int)(((F - 1) * o + D + S + 8 + 3) / 4 * 4);
    const size_t lds_bytes = ((size_t)a.xs_floats + (taps_lds ? (size_t)S * n : 0)) * 4;
    const int mode = !in_int16 ? RSM_F32 : C == 1 ? RSM_I16_MONO : (C == 2 && channel < 0 && dicow_aligned(4, in)) ? RSM_I16_STEREO : RSM_I16_ANY;
    switch (mode) {
        case RSM_F32: rsm_launch<RSM_F32>(taps_lds, tiles, lds_bytes, st, a); break;
        case RSM_I16_MONO: rsm_launch<RSM_I16_MONO>(taps_lds, tiles, lds_bytes, st, a); break;
        case RSM_I16_STEREO: rsm_launch<RSM_I16_STEREO>(taps_lds, tiles, lds_bytes, st, a); break;
        default: rsm_launch<RSM_I16_ANY>(taps_lds, tiles, lds_bytes, st, a); break;
    }
    DICOW_CHECK_LAUNCH("resample_kernel");
    return DICOW_OK;
}

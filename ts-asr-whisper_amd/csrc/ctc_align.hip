// CTC forced alignment: the best path through the CTC trellis of a KNOWN token sequence, read back as a label per frame, a frame span per
// token and the token's own log-probability mass (what torchaudio.functional.forced_align computes).  All problems of a call -- one per decoded
// segment of a session -- run in ONE call of two launches.
//
// Problem i aligns targets y[0..L) against frames [f0, f0 + F) of logits row r, x[f][c] = logit[r, f0 + f, alias[c]] - lse[r, f0 + f] (one
// __fsub_rn; alias NULL = identity, lse NULL = the logits are log-probabilities already).  States s = 0..2L, even = blank, odd = y[(s-1)/2]:
//     v[0][0] = x[0][blank], v[0][1] = x[0][y0], every other v[0][s] = -inf
//     v[f][s] = x[f][lab(s)] + max(v[f-1][s], v[f-1][s-1], v[f-1][s-2] if s is odd and y[(s-1)/2] != y[(s-3)/2])        (__fadd_rn, fp32)
// THE TIE RULE (the project's own): among equal maxima staying (s) beats s-1 and s-1 beats s-2; at the last frame state 2L wins over 2L-1
// only if strictly greater; L = 0 is the all-blank path; F = 0 with L = 0 is the empty path of score 0.
//
// 1. ca_gather_kernel (fully parallel): the compact emission matrix E[i][f][0..W) in the workspace, W = roundup8(L) + 4 floats a frame:
//    columns [0, L) the targets' x, [L, roundup8(L)) -inf, column roundup8(L) the blank's x, the last three 0.  The scattered 2/4-byte reads
//    out of rows of 51 866 classes happen here, once, off the sequential chain.  The -inf padding is what keeps the states above 2L at -inf
//    without a mask in the loop: they start at -inf, and a state is only ever fed from itself and from below.
// 2. ca_align_kernel: one wave per problem, no barrier in the frame loop.  A lane owns K consecutive states in registers -- K = 16 (the wide
//    plan: 64 x 16 = 1024 >= 2 * 511 + 1 states) or K = 2 (the narrow plan, L <= 63: one label and the blank before it per lane; most
//    segments of a session are this short and the wide plan would leave 56 lanes idle and walk 16 states a lane for them).  K is even, so the
//    only value that crosses a lane boundary is the lower lane's LAST state (it is s-1 of an even first state and s-2 of the odd one after
//    it): one DPP wave shift a frame.  A lane's K / 2 label columns of E are contiguous (two 16-byte loads for K = 16), the blank column is
//    one broadcast load; rows are read a chunk of frames ahead, their addresses do not depend on the recursion.  The K two-bit back-pointers
//    of a lane (0 stay, 1 from s-1, 2 from s-2) go out as one dword (K = 16) or one byte (K = 2) per lane per frame, coalesced.
//    The walk back follows in the same kernel after one workgroup barrier (the wave reads its own stores): blocks of CA_WB frames of
//    back-pointer rows are staged in LDS, lane 0 follows the path inside a block -- the serial chain is one LDS read and five ALU steps
//    a frame, a state per frame into LDS and nothing else -- then a lane per frame writes the block's labels to `path` coalesced and
//    notes where a token begins or ends by comparing its frame's state with its neighbours'; spans and token scores leave coalesced at
//    the end.  One writer per element, no atomics.
// NaN among the used columns is outside the contract; the walk clamps every state to [0, 2L] and every code to <= 2, so nothing is read or
// written out of bounds.  An alias outside [0, V1) reads nothing and counts as -inf.
#include "host_table.h"
#include <algorithm>
#include <vector>

#define CA_WB 64                                     // frames of a staged block of back-pointers
#define CA_GF 16                                     // frames of E one gather workgroup writes per trip
#define CA_NARROW_MAX_L 63                           // the narrow plan: 2 L + 1 <= 128 states, two a lane
#define CA_PF_WIDE 4                                 // frames of E read ahead: 4 x 16 states is ~1500 cycles of work, above an HBM miss
#define CA_PF_NARROW 16
#ifndef CA_ONLY                                      // measurement builds (tools/bench_ctc_align.py): 1 = the gather alone, 2 = recursion and
#define CA_ONLY 0                                    // walk alone, over the E an earlier full call left in the same ws, 3 = as 2 without
#endif                                               // the walk (score and status alone are written)

struct ca_prob {                                     // one problem as the kernels see it (DICOW_CTC_ALIGN_PROB_BYTES)
    int32_t row, f0, F, L;
    int32_t tgt_off, plan, W, Wl;                    // targets at ws_targets[tgt_off ..]; 1 narrow / 2 wide; floats a row of E; the blank's column
    int32_t bp_row, pad_;                            // bytes of a frame's back-pointers
    int64_t e_off, bp_off;                           // byte offsets into the workspace
};
static_assert(sizeof(ca_prob) == DICOW_CTC_ALIGN_PROB_BYTES, "the header states the table's size");

struct ca_args {
    const void* logits; const float* lse; const int32_t* alias; const ca_prob* probs; const int32_t* targets; char* ws;
    int32_t* path; int32_t* spans; float* token_score; float* score; int32_t* status;
    int64_t ld;
    int T, V1, blank, Fmax, Lmax;
};

template <int BF>
__global__ void __launch_bounds__(256) ca_gather_kernel(const ca_args a) {
    __shared__ int cols[DICOW_CTC_ALIGN_MAX_L + 9];  // the logits column of every column of E; -1: -inf, -2: 0
    const ca_prob p = a.probs[blockIdx.x];
    const int chunks = (p.F + CA_GF - 1) / CA_GF, tid = threadIdx.x;
    if ((int)blockIdx.y >= chunks) return;
    for (int c = tid; c < p.W; c += 256) {
        const int lab = c < p.L ? a.targets[p.tgt_off + c] : (c == p.Wl ? a.blank : -1);
        int col = (lab >= 0 && a.alias) ? a.alias[lab] : lab;
        if (col < 0 || col >= a.V1) col = -1;
        cols[c] = c > p.Wl ? -2 : col;
    }
    __syncthreads();
    float* E = reinterpret_cast<float*>(a.ws + p.e_off);
    const int64_t frame0 = (int64_t)p.row * a.T + p.f0;
    for (int chunk = blockIdx.y; chunk < chunks; chunk += gridDim.y) {
        const int f_lo = chunk * CA_GF, cnt = min(CA_GF, p.F - f_lo) * p.W;
#pragma unroll 4
        for (int idx = tid; idx < cnt; idx += 256) {
            const int df = idx / p.W, c = idx - df * p.W, col = cols[c];
            float x = col == -1 ? -INFINITY : 0.f;
            if (col >= 0) {
                const int64_t frame = frame0 + f_lo + df;
                if (BF) x = __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(a.logits)[frame * a.ld + col] << 16);
                else x = reinterpret_cast<const float*>(a.logits)[frame * a.ld + col];
                if (a.lse) x = __fsub_rn(x, a.lse[frame]);
            }
            E[(int64_t)(f_lo + df) * p.W + c] = x;
        }
    }
}

// lane l <- lane l - 1, lane 0 <- -inf (DPP wave_shr:1; bound_ctrl off, so the lane without a source keeps `old`)
__device__ __forceinline__ float ca_from_below(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(x), 0x138, 0xf, 0xf, false));
}

// The recursion of one problem: K states a lane.  Leaves the back-pointers of frames 1 .. F-1 in bp and returns v[F-1][2L], v[F-1][2L-1].
template <int K, int PF>
__device__ __forceinline__ void ca_recursion(const ca_prob& p, const float* __restrict__ E, char* __restrict__ bp, const int* ylds, int lane,
                                             float& v_blank, float& v_label) {
    constexpr int H = K / 2;
    static_assert(H == 1 || H == 8, "one label a lane, or eight as two 16-byte loads");
    const int F = p.F, L = p.L, W = p.W, Wl = p.Wl;
    const bool act = H * lane < Wl;                                            // the lane has label columns in E
    unsigned skip = 0;                                                         // bit h: label H * lane + h differs from the one before it
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = H * lane + h;
        if (j >= 1 && j < L && ylds[j] != ylds[j - 1]) skip |= 1u << h;
    }
    const float* mine = E + (act ? H * lane : 0);
    auto load = [&](int f, float (&e)[H], float& xb) {                         // (e of a lane without columns keeps its -inf)
        const int64_t o = (int64_t)min(f, F - 1) * W;
        xb = E[o + Wl];
        if (act) {
            if constexpr (H == 8) {
                const float4 lo = *reinterpret_cast<const float4*>(mine + o), hi = *reinterpret_cast<const float4*>(mine + o + 4);
                e[0] = lo.x; e[1] = lo.y; e[2] = lo.z; e[3] = lo.w; e[4] = hi.x; e[5] = hi.y; e[6] = hi.z; e[7] = hi.w;
            } else {
                e[0] = mine[o];
            }
        }
    };
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = -INFINITY;
    float ce[PF][H], cb[PF], ne[PF][H], nb[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) ce[u][h] = ne[u][h] = -INFINITY;
    load(0, ce[0], cb[0]);
    if (lane == 0) { v[0] = cb[0]; v[1] = ce[0][0]; }
    auto step = [&](int f, const float (&e)[H], float xb) {
        const float below = ca_from_below(v[K - 1]);
        unsigned bits = 0;
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {                                     // downwards: v[k - 1], v[k - 2] are still the last frame's
            float best = v[k];
            unsigned code = 0;
            const float p1 = k > 0 ? v[k - 1] : below;
            if (p1 > best) { best = p1; code = 1; }
            if (k & 1) {
                const float p2 = k >= 2 ? v[k - 2] : below;
                if (((skip >> (k >> 1)) & 1u) && p2 > best) { best = p2; code = 2; }
            }
            v[k] = __fadd_rn((k & 1) ? e[k >> 1] : xb, best);
            bits |= code << (2 * k);
        }
        char* row = bp + (int64_t)f * p.bp_row;
        if constexpr (K == 16) { if (lane * 4 < p.bp_row) reinterpret_cast<uint32_t*>(row)[lane] = bits; }
        else { if (lane < p.bp_row) reinterpret_cast<uint8_t*>(row)[lane] = (uint8_t)bits; }
    };
    int t = 1;
#pragma unroll
    for (int u = 0; u < PF; ++u) load(t + u, ce[u], cb[u]);
#pragma unroll 1
    for (; t + PF <= F; t += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) load(t + PF + u, ne[u], nb[u]);
#pragma unroll
        for (int u = 0; u < PF; ++u) step(t + u, ce[u], cb[u]);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            cb[u] = nb[u];
#pragma unroll
            for (int h = 0; h < H; ++h) ce[u][h] = ne[u][h];
        }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (t + u < F) step(t + u, ce[u], cb[u]);
    const int sb = 2 * L, sl = max(2 * L - 1, 0);
    float mb = -INFINITY, ml = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k == sb % K) mb = v[k];
        if (k == sl % K) ml = v[k];
    }
    v_blank = __shfl(mb, sb / K, 64);
    v_label = __shfl(ml, sl / K, 64);
}

__global__ void __launch_bounds__(64) ca_align_kernel(const ca_args a) {
    __shared__ uint32_t tile[CA_WB * 64];                                      // CA_WB rows of at most 256 bytes
    __shared__ int ylds[DICOW_CTC_ALIGN_MAX_L + 1];
    __shared__ int sp[2 * (DICOW_CTC_ALIGN_MAX_L + 1)];
    __shared__ short sbuf[CA_WB];
    __shared__ int carry[1];
    const int i = blockIdx.x, lane = threadIdx.x;
    const ca_prob p = a.probs[i];
    const int F = p.F, L = p.L;
    for (int j = lane; j < L; j += 64) ylds[j] = a.targets[p.tgt_off + j];
    for (int j = lane; j < 2 * L; j += 64) sp[j] = -1;
    __syncthreads();
    int32_t* path = a.path + (int64_t)i * a.Fmax;
    int32_t* spans = a.spans + (int64_t)i * a.Lmax * 2;
    float* tscore = a.token_score + (int64_t)i * a.Lmax;
    const float* E = reinterpret_cast<const float*>(a.ws + p.e_off);
    char* bp = a.ws + p.bp_off;
    bool ok = false;
    float score = -INFINITY;
    int end = 0;
    if (F > 0) {
        float vb, vl;
        if (p.plan == 1) ca_recursion<2, CA_PF_NARROW>(p, E, bp, ylds, lane, vb, vl);
        else ca_recursion<16, CA_PF_WIDE>(p, E, bp, ylds, lane, vb, vl);
        if (L > 0 && !(vb > vl)) { end = 2 * L - 1; score = vl; }
        else { end = 2 * L; score = vb; }
        ok = !(score == -INFINITY);
    } else if (L == 0) {
        ok = true;
        score = 0.f;
    }
    if (!ok) {                                                                 // infeasible: too few frames, or every end state at -inf
        for (int f = lane; f < a.Fmax; f += 64) path[f] = -1;
        for (int x = lane; x < 2 * a.Lmax; x += 64) spans[x] = -1;
        for (int j = lane; j < a.Lmax; j += 64) tscore[j] = 0.f;
        if (lane == 0) { a.score[i] = -INFINITY; a.status[i] = 1; }
        return;
    }
    if (CA_ONLY == 3) {
        if (lane == 0) { a.score[i] = score; a.status[i] = 0; }
        return;
    }
    __syncthreads();                                                           // the wave's back-pointer stores, before its lanes read them
    const int rdw = p.bp_row / 4;
    int st = end, above = -1;
    for (int b1 = F; b1 > 0;) {
        const int b0 = (b1 - 1) / CA_WB * CA_WB, r0 = max(b0, 1);              // row 0 holds no back-pointers
        const int ndw = (b1 - r0) * rdw;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bp + (int64_t)r0 * p.bp_row);
        for (int x = lane; x < ndw; x += 64) tile[x] = src[x];
        __syncthreads();
        if (lane == 0) {                                                       // the serial chain: a state per frame, nothing else
            int s = st;
            for (int f = b1 - 1; f >= b0; --f) {
                sbuf[f - b0] = (short)s;
                if (f > 0) {
                    unsigned code;
                    if (p.plan == 1) code = (reinterpret_cast<const uint8_t*>(tile)[(f - r0) * p.bp_row + (s >> 1)] >> (2 * (s & 1))) & 3u;
                    else code = (tile[(f - r0) * rdw + (s >> 4)] >> (2 * (s & 15))) & 3u;
                    s = max(s - (int)min(code, 2u), 0);
                }
            }
            carry[0] = s;                                                      // the state of frame b0 - 1
        }
        __syncthreads();
        const int below = carry[0], first = sbuf[0];
        for (int f = b0 + lane; f < b1; f += 64) {                             // labels and token boundaries: a lane per frame
            const int s = sbuf[f - b0];
            path[f] = (s & 1) ? ylds[s >> 1] : a.blank;
            if (s & 1) {                                                       // token s >> 1: sp[s - 1] its first frame, sp[s] one past its last
                const int up = f + 1 < b1 ? sbuf[f + 1 - b0] : above;
                const int dn = f > b0 ? sbuf[f - 1 - b0] : (b0 > 0 ? below : -1);
                if (s != up) sp[s] = f + 1;
                if (s != dn) sp[s - 1] = f;
            }
        }
        __syncthreads();
        st = below;
        above = first;
        b1 = b0;
    }
    for (int f = F + lane; f < a.Fmax; f += 64) path[f] = -1;
    for (int x = lane; x < 2 * a.Lmax; x += 64) spans[x] = x < 2 * L ? sp[x] : -1;
    for (int j = lane; j < a.Lmax; j += 64) {
        float acc = 0.f;
        if (j < L) {
            const int s0 = sp[2 * j], s1 = sp[2 * j + 1];
            if (s0 >= 0 && s1 > s0) {                                          // (always, inside the contract)
                acc = E[(int64_t)s0 * p.W + j];
                for (int f = s0 + 1; f < s1; ++f) acc = __fadd_rn(acc, E[(int64_t)f * p.W + j]);
            }
        }
        tscore[j] = acc;
    }
    if (lane == 0) { a.score[i] = score; a.status[i] = 0; }
}

// The call's plan, shared by the size query and the entry point.  The workspace: [n] ca_prob, the targets of all problems back to back
// (int32, the block rounded up to 16 bytes), then per problem E (F * W floats) and the back-pointers (F * bp_row bytes, rounded up to 16).
// bp_row does not depend on the plan: the larger of the wide row, 4 * ceil((2 L + 1) / 16), and (L <= 63) the narrow one, roundup4(L + 1).
struct ca_plan { int64_t table_bytes, need, n_targets; int Fmax, Lmax; };

static inline int64_t ca_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

static int ca_make_plan(const char* who, const int64_t* table, int n, int plan, std::vector<int64_t>* image, ca_plan* out) {
    DICOW_REQUIRE(n >= 0, "%s: negative n=%d", who, n);
    DICOW_REQUIRE(n == 0 || table, "%s: null problem table", who);
    DICOW_REQUIRE(plan >= 0 && plan <= 2, "%s: plan=%d is none of 0 (the library's choice), 1 (narrow, L <= %d), 2 (wide)", who, plan, CA_NARROW_MAX_L);
    int64_t total = 0;
    out->Fmax = out->Lmax = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t F = table[5 * (int64_t)k + 2], L = table[5 * (int64_t)k + 4];
        DICOW_REQUIRE(F >= 0 && F <= INT32_MAX, "%s: problem %d has F=%lld frames, outside [0, 2^31)", who, k, (long long)F);
        DICOW_REQUIRE(L >= 0 && L <= DICOW_CTC_ALIGN_MAX_L, "%s: problem %d has L=%lld targets, outside [0, DICOW_CTC_ALIGN_MAX_L = %d] (2 L + 1 "
                      "states <= 1024, the ceiling of dicow_ctc_args.Smax)", who, k, (long long)L, DICOW_CTC_ALIGN_MAX_L);
        DICOW_REQUIRE(plan != 1 || L <= CA_NARROW_MAX_L, "%s: problem %d has L=%lld targets, the narrow plan takes at most %d", who, k, (long long)L,
                      CA_NARROW_MAX_L);
        total += L;
        out->Fmax = std::max(out->Fmax, (int)F);
        out->Lmax = std::max(out->Lmax, (int)L);
    }
    out->n_targets = total;
    out->table_bytes = ca_up((int64_t)n * (int64_t)sizeof(ca_prob) + 4 * total, 16);
    DICOW_REQUIRE(out->table_bytes <= DICOW_CTC_ALIGN_MAX_WS_BYTES, "%s: the tables of %d problems take %lld bytes, past DICOW_CTC_ALIGN_MAX_WS_BYTES = %lld "
                  "(split the call)", who, n, (long long)out->table_bytes, (long long)DICOW_CTC_ALIGN_MAX_WS_BYTES);
    if (image) image->assign((size_t)out->table_bytes / 8, 0);
    ca_prob* pr = image ? reinterpret_cast<ca_prob*>(image->data()) : nullptr;
    int64_t need = out->table_bytes, off = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t* row = table + 5 * (int64_t)k;
        const int64_t F = row[2], L = row[4];
        const int64_t Wl = ca_up(L, 8), W = Wl + 4;
        int64_t bp_row = 4 * ((2 * L + 1 + 15) / 16);
        if (L <= CA_NARROW_MAX_L) bp_row = std::max(bp_row, ca_up(L + 1, 4));
        if (pr) {
            pr[k].F = (int32_t)F; pr[k].L = (int32_t)L;
            pr[k].tgt_off = (int32_t)off;
            pr[k].plan = plan ? plan : (L <= CA_NARROW_MAX_L ? 1 : 2);
            pr[k].W = (int32_t)W; pr[k].Wl = (int32_t)Wl; pr[k].bp_row = (int32_t)bp_row;
            pr[k].e_off = need;
            pr[k].bp_off = need + F * W * 4;
        }
        off += L;
        need += F * W * 4 + ca_up(F * bp_row, 16);
        DICOW_REQUIRE(need <= DICOW_CTC_ALIGN_MAX_WS_BYTES, "%s: the tables up to problem %d of %d bring the workspace to %lld bytes, past "
                      "DICOW_CTC_ALIGN_MAX_WS_BYTES = %lld (split the call)", who, k, n, (long long)need, (long long)DICOW_CTC_ALIGN_MAX_WS_BYTES);
    }
    out->need = need;
    return DICOW_OK;
}

extern "C" int64_t dicow_ctc_align_ws_bytes(const int64_t* table, int n) {
    ca_plan plan;
    if (ca_make_plan("ctc_align_ws_bytes", table, n, 0, nullptr, &plan) != DICOW_OK) return -1;
    return plan.need;
}

extern "C" int dicow_ctc_forced_align(const void* logits, int in_bf16, int B, int T, int V1, int64_t ld, const float* lse, const int32_t* alias,
                                      int blank, const int64_t* table, int n, const int32_t* targets, int64_t n_targets, int32_t* path, int Fmax,
                                      int32_t* spans, int Lmax, float* token_score, float* score, int32_t* status, int plan, void* ws,
                                      int64_t ws_bytes, void* stream) {
    static thread_local std::vector<int64_t> stage;          // the uploaded image: problems and targets
    ca_plan pl;
    if (ca_make_plan("ctc_forced_align", table, n, plan, &stage, &pl) != DICOW_OK) return DICOW_ERR_INVALID;
    DICOW_REQUIRE(B >= 0 && T >= 0 && V1 > 0 && ld >= V1, "ctc_forced_align: bad logits shape B=%d T=%d V1=%d ld=%lld (ld >= V1 > 0)", B, T, V1, (long long)ld);
    DICOW_REQUIRE(blank >= 0 && blank < V1, "ctc_forced_align: blank=%d outside [0, V1 = %d)", blank, V1);
    DICOW_REQUIRE(n_targets >= 0 && (n_targets == 0 || targets), "ctc_forced_align: n_targets=%lld with %s target array", (long long)n_targets,
                  targets ? "a" : "a null");
    ca_prob* pr = reinterpret_cast<ca_prob*>(stage.data());
    int32_t* tg = reinterpret_cast<int32_t*>(pr + n);
    for (int k = 0; k < n; ++k) {
        const int64_t* row = table + 5 * (int64_t)k;
        DICOW_REQUIRE(row[0] >= 0 && row[0] < B, "ctc_forced_align: problem %d reads row %lld of logits with B = %d rows", k, (long long)row[0], B);
        DICOW_REQUIRE(dicow_span_ok(row[1], row[2], T), "ctc_forced_align: problem %d reads frames [%lld, %lld + %lld), past the T = %d "
                      "frames of a row", k, (long long)row[1], (long long)row[1], (long long)row[2], T);
        DICOW_REQUIRE_SPAN(row[3], row[4], n_targets, "reads targets", "ids of the array", "ctc_forced_align: problem %d", k);
        pr[k].row = (int32_t)row[0];
        pr[k].f0 = (int32_t)row[1];
        for (int64_t j = 0; j < row[4]; ++j) {
            const int32_t y = targets[row[3] + j];
            DICOW_REQUIRE(y >= 0 && y < V1, "ctc_forced_align: target %lld of problem %d is %d, outside [0, V1 = %d)", (long long)j, k, y, V1);
            DICOW_REQUIRE(y != blank, "ctc_forced_align: target %lld of problem %d is the blank (%d)", (long long)j, k, y);
            tg[pr[k].tgt_off + j] = y;
        }
    }
    if (n == 0) return DICOW_OK;
    DICOW_REQUIRE(Fmax >= pl.Fmax && Lmax >= pl.Lmax, "ctc_forced_align: outputs of Fmax=%d frames and Lmax=%d targets, the table needs %d and %d", Fmax,
                  Lmax, pl.Fmax, pl.Lmax);
    DICOW_REQUIRE(logits && path && spans && token_score && score && status && ws, "ctc_forced_align: null pointer");
    DICOW_REQUIRE(dicow_aligned(in_bf16 ? 2 : 4, logits) && dicow_aligned(4, lse, alias, path, spans, token_score, score, status) && dicow_aligned(16, ws),
                  "ctc_forced_align: a pointer is not aligned to its element, or ws not 16-byte aligned");
    DICOW_REQUIRE(ws_bytes >= pl.need, "ctc_forced_align: ws_bytes=%lld, need %lld", (long long)ws_bytes, (long long)pl.need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dicow_upload("ctc_forced_align", ws, stage.data(), pl.table_bytes, st)) return rc;
    ca_args a;
    a.logits = logits; a.lse = lse; a.alias = alias;
    a.probs = reinterpret_cast<const ca_prob*>(ws);
    a.targets = reinterpret_cast<const int32_t*>(a.probs + n);
    a.ws = static_cast<char*>(ws);
    a.path = path; a.spans = spans; a.token_score = token_score; a.score = score; a.status = status;
    a.ld = ld; a.T = T; a.V1 = V1; a.blank = blank; a.Fmax = Fmax; a.Lmax = Lmax;
    if (pl.Fmax > 0 && CA_ONLY != 2 && CA_ONLY != 3) {
        const dim3 grid((unsigned)n, (unsigned)std::min((pl.Fmax + CA_GF - 1) / CA_GF, 4096));
        if (in_bf16) ca_gather_kernel<1><<<grid, 256, 0, st>>>(a);
        else ca_gather_kernel<0><<<grid, 256, 0, st>>>(a);
        DICOW_CHECK_LAUNCH("ca_gather_kernel");
    }
    if (CA_ONLY != 1) {
        ca_align_kernel<<<dim3((unsigned)n), 64, 0, st>>>(a);
        DICOW_CHECK_LAUNCH("ca_align_kernel");
    }
    return DICOW_OK;
}

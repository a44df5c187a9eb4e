// Multi-tensor optimizer kernels (torch.optim.AdamW semantics over a list of separate fp32 tensors): one launch updates every
// tensor of a call.  A device table (include/dicow_hip.h: dicow_mt_tensor[] + dicow_mt_chunk[]) describes the call; a chunk of
// DICOW_MT_CHUNK elements (or a tensor's shorter tail) is one trip of a workgroup, so 1280-element vectors and 6.5M-element
// matrices are balanced alike.  Element offsets and counts are int64.  Pure HBM streams: a tensor whose pointers are all 16-byte
// aligned runs on float4 loads / stores (two per array and lane), its count % 4 tail and every misaligned tensor (a Parameter can be
// an offset view of a larger storage) on the scalar path.
#include "common.h"

#define MT_BLOCK 256
#define MT_GRID_MAX 4096
static_assert(DICOW_MT_CHUNK == MT_BLOCK * 8, "a chunk is one trip of two float4 per lane");

// torch.lerp(m, g, w) for a scalar weight (ATen Lerp.h): the branch on w is uniform over a class
__device__ __forceinline__ float mt_lerp(float m, float g, float w) {
    return w < 0.5f ? m + w * (g - m) : g - (g - m) * (1.f - w);
}

// One element of torch's single-tensor AdamW (torch/optim/adam.py, decoupled weight decay), in torch's order:
//   p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= step_size m / (sqrt(v) / sqrt(bc2) + eps)
// (torch divides by the scalar sqrt(bc2) as a multiply by its fp32 reciprocal: BinaryDivTrueKernel's CPU-scalar path).
struct mt_cls_t { float decay, step_size, inv_bc2_sqrt, w1, b2, omb2, eps; };

__device__ __forceinline__ void mt_adamw_elem(float& p, float g, float& m, float& v, const mt_cls_t& c) {
    p = p * c.decay;
    m = mt_lerp(m, g, c.w1);
    v = v * c.b2;
    v = v + c.omb2 * g * g;
    const float denom = sqrtf(v) * c.inv_bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);
}

__global__ void __launch_bounds__(MT_BLOCK) multi_adamw_kernel(const dicow_mt_tensor* __restrict__ tensors,
                                                               const dicow_mt_chunk* __restrict__ chunks, int64_t n_chunks,
                                                               const dicow_mt_adamw_classes cls, int cls_base, const float* __restrict__ clip_coef) {
    const float coef = clip_coef ? clip_coef[0] : 1.f;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const dicow_mt_chunk ch = chunks[k];
        const dicow_mt_tensor t = tensors[ch.tensor];
        const int ci = t.cls - cls_base;
        if (ci < 0 || ci >= cls.n_classes) continue;                   // another launch's class (more than DICOW_MT_MAX_CLASSES classes)
        const mt_cls_t c = {cls.decay[ci], cls.step_size[ci], 1.f / cls.bc2_sqrt[ci], cls.lerp_w[ci], cls.beta2[ci], cls.one_minus_beta2[ci],
                            cls.eps[ci]};
        float* __restrict__ p = t.p + ch.start;
        const float* __restrict__ g = t.g + ch.start;
        float* __restrict__ m = t.m + ch.start;
        float* __restrict__ v = t.v + ch.start;
        const int len = ch.len;
        int done = 0;
        if (t.flags & DICOW_MT_ALIGNED_ALL) {                          // one trip: a chunk is MT_BLOCK x 2 float4
            const int n4 = len >> 2, i0 = threadIdx.x, i1 = threadIdx.x + MT_BLOCK;
            f32x4_t* p4 = reinterpret_cast<f32x4_t*>(p);
            const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(g);
            f32x4_t* m4 = reinterpret_cast<f32x4_t*>(m);
            f32x4_t* v4 = reinterpret_cast<f32x4_t*>(v);
            f32x4_t pp[2], gg[2], mm[2], vv[2];
            const bool has0 = i0 < n4, has1 = i1 < n4;
            if (has0) { pp[0] = p4[i0]; gg[0] = g4[i0]; mm[0] = m4[i0]; vv[0] = v4[i0]; }
            if (has1) { pp[1] = p4[i1]; gg[1] = g4[i1]; mm[1] = m4[i1]; vv[1] = v4[i1]; }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pp[u][e], me = mm[u][e], ve = vv[u][e];
                    mt_adamw_elem(pe, gg[u][e] * coef, me, ve, c);
                    pp[u][e] = pe; mm[u][e] = me; vv[u][e] = ve;
                }
            if (has0) { p4[i0] = pp[0]; m4[i0] = mm[0]; v4[i0] = vv[0]; }
            if (has1) { p4[i1] = pp[1]; m4[i1] = mm[1]; v4[i1] = vv[1]; }
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += MT_BLOCK) {
            float pv = p[i], mv = m[i], vv = v[i];
            mt_adamw_elem(pv, g[i] * coef, mv, vv, c);
            p[i] = pv; m[i] = mv; v[i] = vv;
        }
    }
}

// Workgroups stride over the chunks (consecutive chunks run side by side: the HBM window in flight stays narrow, as in the flat
// dicow_adamw_f32); a fixed grid per table, so the sum of squares below adds its partials in the same order on every replica.
static unsigned mt_grid(int64_t n_chunks) { return (unsigned)(n_chunks < MT_GRID_MAX ? n_chunks : MT_GRID_MAX); }

extern "C" int dicow_multi_chunk_elems(void) { return DICOW_MT_CHUNK; }

static int mt_check_table(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks, const char* what) {
    if (!tensors || !chunks || n_chunks <= 0 || n_chunks > 0x7fffffffLL) {
        dicow_set_error("%s: bad table (n_chunks %lld)", what, (long long)n_chunks);
        return DICOW_ERR_INVALID;
    }
    return DICOW_OK;
}

extern "C" int dicow_multi_adamw_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks,
                                     const dicow_mt_adamw_classes* cls, int cls_base, const float* clip_coef, void* stream) {
    if (int rc = mt_check_table(tensors, chunks, n_chunks, "multi_adamw_f32")) return rc;
    DICOW_REQUIRE(cls && cls->n_classes >= 1 && cls->n_classes <= DICOW_MT_MAX_CLASSES && cls_base >= 0, "multi_adamw_f32: bad classes");
    hipLaunchKernelGGL(multi_adamw_kernel, dim3(mt_grid(n_chunks)), dim3(MT_BLOCK), 0, (hipStream_t)stream, tensors, chunks, n_chunks, *cls,
                       cls_base, clip_coef);
    DICOW_CHECK_LAUNCH("multi_adamw_f32");
    return DICOW_OK;
}

// ---- deterministic sum of squares of the g arrays: every workgroup's partial goes to its own slot of the caller's workspace, the last
// workgroup to arrive (ticket word at the head of the workspace, zero on entry and left zero) adds the slots in index order in double.
// The result depends on the tensor sizes and their order only, so data-parallel replicas derive bit-identical clip coefficients.
// out[0] = sum of squares, out[1] = its square root (the global 2-norm), out[2] = min(1, max_norm / (norm + 1e-6)) (torch's clip
// coefficient; NaN stays NaN, as torch.clamp leaves it).
#define MT_WS_HEAD 256
__global__ void __launch_bounds__(MT_BLOCK) multi_sumsq_kernel(const dicow_mt_tensor* __restrict__ tensors,
                                                               const dicow_mt_chunk* __restrict__ chunks, int64_t n_chunks,
                                                               unsigned char* __restrict__ ws, float* __restrict__ out, float max_norm) {
    __shared__ double red[MT_BLOCK / 64];
    __shared__ bool last;
    float s = 0.f;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const dicow_mt_chunk ch = chunks[k];
        const dicow_mt_tensor t = tensors[ch.tensor];
        const float* __restrict__ g = t.g + ch.start;
        const int len = ch.len;
        int done = 0;
        if (t.flags & DICOW_MT_ALIGNED_G) {
            const int n4 = len >> 2, i0 = threadIdx.x, i1 = threadIdx.x + MT_BLOCK;
            const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(g);
            f32x4_t a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (i0 < n4) a = g4[i0];
            if (i1 < n4) b = g4[i1];
            s += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
            s += (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += MT_BLOCK) s += g[i] * g[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned* ticket = reinterpret_cast<unsigned*>(ws);
    float* part = reinterpret_cast<float*>(ws + MT_WS_HEAD);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double d = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += MT_BLOCK) d += (double)__builtin_nontemporal_load(&part[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ss = (float)((red[0] + red[1]) + (red[2] + red[3]));
        const float nrm = sqrtf(ss);
        const float cc = max_norm / (nrm + 1e-6f);
        const float coef = cc > 1.f ? 1.f : cc;
        out[0] = ss; out[1] = nrm; out[2] = coef;
        *ticket = 0u;
    }
}

extern "C" int64_t dicow_multi_sumsq_ws_bytes(int64_t n_chunks) { return n_chunks <= 0 ? 0 : MT_WS_HEAD + 4 * (int64_t)mt_grid(n_chunks); }

extern "C" int dicow_multi_sumsq_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks, void* ws,
                                     int64_t ws_bytes, float* out, float max_norm, void* stream) {
    if (int rc = mt_check_table(tensors, chunks, n_chunks, "multi_sumsq_f32")) return rc;
    DICOW_REQUIRE(ws && out && ws_bytes >= dicow_multi_sumsq_ws_bytes(n_chunks) && ((uintptr_t)ws & 15) == 0,
                  "multi_sumsq_f32: workspace of %lld bytes needed", (long long)dicow_multi_sumsq_ws_bytes(n_chunks));
    hipLaunchKernelGGL(multi_sumsq_kernel, dim3(mt_grid(n_chunks)), dim3(MT_BLOCK), 0, (hipStream_t)stream, tensors, chunks, n_chunks,
                       (unsigned char*)ws, out, max_norm);
    DICOW_CHECK_LAUNCH("multi_sumsq_f32");
    return DICOW_OK;
}

// ---- g *= coef[0] in place (torch.nn.utils.clip_grad_norm_'s _foreach_mul_ by the clamped coefficient)
__global__ void __launch_bounds__(MT_BLOCK) multi_scale_kernel(const dicow_mt_tensor* __restrict__ tensors,
                                                               const dicow_mt_chunk* __restrict__ chunks, int64_t n_chunks,
                                                               const float* __restrict__ coef) {
    const float c = coef[0];
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const dicow_mt_chunk ch = chunks[k];
        const dicow_mt_tensor t = tensors[ch.tensor];
        float* __restrict__ g = t.g + ch.start;
        const int len = ch.len;
        int done = 0;
        if (t.flags & DICOW_MT_ALIGNED_G) {
            const int n4 = len >> 2, i0 = threadIdx.x, i1 = threadIdx.x + MT_BLOCK;
            f32x4_t* g4 = reinterpret_cast<f32x4_t*>(g);
            f32x4_t a, b;
            if (i0 < n4) a = g4[i0];
            if (i1 < n4) b = g4[i1];
            if (i0 < n4) g4[i0] = a * c;
            if (i1 < n4) g4[i1] = b * c;
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += MT_BLOCK) g[i] = g[i] * c;
    }
}

extern "C" int dicow_multi_scale_f32(const dicow_mt_tensor* tensors, const dicow_mt_chunk* chunks, int64_t n_chunks, const float* coef,
                                     void* stream) {
    if (int rc = mt_check_table(tensors, chunks, n_chunks, "multi_scale_f32")) return rc;
    DICOW_REQUIRE(coef, "multi_scale_f32: coef is NULL");
    hipLaunchKernelGGL(multi_scale_kernel, dim3(mt_grid(n_chunks)), dim3(MT_BLOCK), 0, (hipStream_t)stream, tensors, chunks, n_chunks, coef);
    DICOW_CHECK_LAUNCH("multi_scale_f32");
    return DICOW_OK;
}

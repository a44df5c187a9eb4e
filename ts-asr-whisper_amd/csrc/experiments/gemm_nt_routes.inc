// (included by gemm.hip where an experiment kernel is compiled in: -DDICOW_EXPERIMENTS, -DDICOW_ABLATIONS, a non-zero NT2_MASK / NTQ_MASK
// or -DNT128W=1.)  The host side of the NT experiments: what gemm_nt_impl asks before it plans (nt_experiment_knobs) and the launches
// that take a problem away from the shipped kernels (nt_experiment_route).  The default build has two empty inlines instead.

#ifndef NT128W_MIN_TILES
#define NT128W_MIN_TILES 96
#endif

// DICOW_NT_VARIANT (diagnostic builds only; read per call so that a tool can interleave tile shapes in one process, tools/ab_epilogues.py):
//   1 / 2 / 3   gemm_nt_kernel<1, false> / <2, true> / <1, true> for the 128 x 128 path
//   4 ... 10    the 8-wave 256 x 256 kernel (5-8: its ablations 1-4, 9: the staggered 4-stage form), whatever the tile count
//   11 / 12 / 13  the two-stage persistent kernel: run-time-flag epilogue / 256 x 256 forced / 192 x 320 forced
//   21 / 22     the ring kernel with 256 x 256 / 192 x 320 forced (nt_plan sees these two)
// DICOW_NT_BIG overrides NT_BIG_TILES.
static nt_knobs_t nt_experiment_knobs() {
    nt_knobs_t k = {0, NT_BIG_TILES};
#ifdef DICOW_ABLATIONS
    const char* variant_ev = getenv("DICOW_NT_VARIANT");
    static const int big_tiles = getenv("DICOW_NT_BIG") ? atoi(getenv("DICOW_NT_BIG")) : NT_BIG_TILES;
    k.variant = variant_ev ? atoi(variant_ev) : 0;
    k.big_tiles = big_tiles;
#endif
    return k;
}

static void nt_experiment_setup() {
#if NT128W
    (void)hipFuncSetAttribute((const void*)gemm_nt128w_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NT128W_LDS);
#endif
#if NT_EXPERIMENT_KERNELS
#define X(F) (void)hipFuncSetAttribute((const void*)gemm_nt2_kernel<(F)>, hipFuncAttributeMaxDynamicSharedMemorySize, NT2_LDS); \
             (void)hipFuncSetAttribute((const void*)gemm_ntq_kernel<(F)>, hipFuncAttributeMaxDynamicSharedMemorySize, NTQ_LDS);
    NT_EPILOGUES_COMMON(X)
#undef X
#endif
#ifdef DICOW_ABLATIONS
    (void)hipFuncSetAttribute((const void*)gemm_nt256s_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NTS_LDS);
#define X(F) (void)hipFuncSetAttribute((const void*)gemm_ntw_kernel<(F), 4, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, NTW_LDS); \
             (void)hipFuncSetAttribute((const void*)gemm_ntw_kernel<(F), 3, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, NTW_LDS);
    NT_EPILOGUES_COMMON(X) X(-1)
#undef X
    (void)hipFuncSetAttribute((const void*)gemm_nt256_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, NT256_LDS);
    (void)hipFuncSetAttribute((const void*)gemm_nt256_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, NT256_LDS);
    (void)hipFuncSetAttribute((const void*)gemm_nt256_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, NT256_LDS);
    (void)hipFuncSetAttribute((const void*)gemm_nt256_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, NT256_LDS);
    (void)hipFuncSetAttribute((const void*)gemm_nt256_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, NT256_LDS);
#endif
}

#ifdef DICOW_ABLATIONS
// DICOW_NT_VARIANT != 0.  NT_NOT_ROUTED: the shipped kernels run the plan (21 / 22, or a problem too small for the persistent variants).
static int nt_ablation_route(dicow_gemm_args* a, const nt_plan_t& p, int variant, bool want_colsum, bool* fused_colsum, int* colsum_rows,
                             hipStream_t stream) {
    const int batch = a->batch > 0 ? a->batch : 1;
    if (p.family == NT_FAM_RING && variant >= 11 && variant <= 13) {          // the two-stage persistent kernel on the ring kernel's grid
        if (colsum_rows) *colsum_rows = p.colsum_rows;
        if (variant != 11) nt_fuse_colsum(a, want_colsum, fused_colsum);
        const int ct = variant == 11 ? -1 : nt_ct_flags(a->flags);
        disp_note("gemm_ntr_kernel<%d, %d, %d>", ct, p.use35 ? 3 : 4, p.use35 ? 5 : 4);      // (logged under the ring kernel's name, as ever)
        const dim3 gp(p.grid);
        switch (ct) {
#define X(F) case (F):                                                                                                          \
                if (p.use35) hipLaunchKernelGGL((gemm_ntw_kernel<(F), 3, 5>), gp, dim3(256), NTW_LDS, stream, *a);              \
                else hipLaunchKernelGGL((gemm_ntw_kernel<(F), 4, 4>), gp, dim3(256), NTW_LDS, stream, *a);                      \
                break;
            NT_EPILOGUES_COMMON(X)
            default: X(-1)
#undef X
        }
    } else if (p.family == NT_FAM_RING && variant < 11) {                     // 4 ... 10
        const dim3 g256(dicow_cdiv(a->M, 256) * dicow_cdiv(a->N, 256), 1, batch);
        if (variant == 9) hipLaunchKernelGGL(gemm_nt256s_kernel, g256, dim3(512), NTS_LDS, stream, *a);
        else if (variant == 5) hipLaunchKernelGGL(gemm_nt256_kernel<1>, g256, dim3(512), NT256_LDS, stream, *a);
        else if (variant == 6) hipLaunchKernelGGL(gemm_nt256_kernel<2>, g256, dim3(512), NT256_LDS, stream, *a);
        else if (variant == 7) hipLaunchKernelGGL(gemm_nt256_kernel<3>, g256, dim3(512), NT256_LDS, stream, *a);
        else if (variant == 8) hipLaunchKernelGGL(gemm_nt256_kernel<4>, g256, dim3(512), NT256_LDS, stream, *a);
        else hipLaunchKernelGGL(gemm_nt256_kernel<0>, g256, dim3(512), NT256_LDS, stream, *a);
    } else if (p.family != NT_FAM_RING && variant >= 1 && variant <= 3) {
        const dim3 grid(p.grid, 1, batch);
        if (variant == 1) hipLaunchKernelGGL((gemm_nt_kernel<1, false>), grid, dim3(256), 2 * STAGE_BYTES, stream, *a);
        else if (variant == 2) hipLaunchKernelGGL((gemm_nt_kernel<2, true>), grid, dim3(256), NT_LDS_BYTES, stream, *a);
        else hipLaunchKernelGGL((gemm_nt_kernel<1, true>), grid, dim3(256), 2 * STAGE_BYTES, stream, *a);
    } else {
        return NT_NOT_ROUTED;
    }
    DICOW_CHECK_LAUNCH(p.family == NT_FAM_RING ? "gemm_nt (persistent)" : "gemm_nt");
    return DICOW_OK;
}
#endif

#if NT_EXPERIMENT_KERNELS
// Round 5's structural experiments for the problems of the ring kernel, per epilogue class (bits of the masks: gemm.hip at NT2_MASK).
static int nt_mask_route(dicow_gemm_args* a, const nt_plan_t& p, bool want_colsum, bool* fused_colsum, int* colsum_rows, hipStream_t stream) {
#if defined(DICOW_ABLATIONS) || defined(DICOW_EXPERIMENTS)
    static const int nt2_mask = getenv("DICOW_NT2_MASK") ? atoi(getenv("DICOW_NT2_MASK")) : NT2_MASK;
    static const int nt2_delay = getenv("DICOW_NT2_DELAY") ? atoi(getenv("DICOW_NT2_DELAY")) : NT2_DELAY;
    static const int ntq_mask = getenv("DICOW_NTQ_MASK") ? atoi(getenv("DICOW_NTQ_MASK")) : NTQ_MASK;
#else
    constexpr int nt2_mask = NT2_MASK, nt2_delay = NT2_DELAY, ntq_mask = NTQ_MASK;
#endif
    const int batch = a->batch > 0 ? a->batch : 1;
    nt_fuse_colsum(a, want_colsum, fused_colsum);     // (what the ring kernel's path does with them as well)
    const int f_ = a->flags;
    const int cls = f_ == NT_RES_FLAGS ? 1 : f_ == (DICOW_EPI_BIAS | DICOW_EPI_GELU | DICOW_EPI_GELU_DAUX) ? 2 : f_ == (DICOW_EPI_BIAS | DICOW_EPI_GELU) ? 4 :
                    (f_ == DICOW_EPI_MUL_AUX || f_ == (DICOW_EPI_MUL_AUX | DICOW_EPI_COLSUM)) ? 8 :
                    (f_ == DICOW_EPI_BIAS || f_ == (DICOW_EPI_BIAS | DICOW_EPI_SCALE_N)) ? 16 : f_ == 0 ? 32 : 0;
    // 320 x 256 tiles (gemm_ntq_kernel): whole tiles only, at least three k-steps, and only where its rounds of `ncu`
    // workgroups cover no more padded area than the ring kernel's choice (M = 24000: N = 5120 -> 1500 tiles = 6 rounds)
    const int64_t tq = (int64_t)(a->M / 320) * (a->N / 256) * batch;
    const int64_t wq = dicow_cdiv(tq, p.ncu) * 320 * 256, wr = (a->N >= 320 && p.wide_ok && p.w35 < p.w44) ? p.w35 : p.w44;
    if ((ntq_mask & cls) && a->M % 320 == 0 && a->N % 256 == 0 && a->K >= 3 * BK && tq > 0 && (wq <= wr || (ntq_mask & 1024))) {
        const dim3 gq(dicow_cdiv(tq, dicow_cdiv(tq, p.ncu)));
        if (colsum_rows) *colsum_rows = 2 * (a->M / 320);
        disp_note("gemm_ntq_kernel<%d>", f_);
        switch (f_) {
#define X(F) case (F): hipLaunchKernelGGL((gemm_ntq_kernel<(F)>), gq, dim3(256), NTQ_LDS, stream, *a); break;
            NT_EPILOGUES_COMMON(X)
#undef X
        }
        DICOW_CHECK_LAUNCH("gemm_ntq (persistent, 320 x 256 tiles)");
        return DICOW_OK;
    }
    // two workgroups per CU (gemm_nt2_kernel, 128 x 256 tiles): the epilogue-heavy shapes, per NT2_MASK
    if ((nt2_mask & cls) && a->M >= 128 && a->N >= 256) {
        const int64_t t2 = (int64_t)dicow_cdiv(a->M, 128) * dicow_cdiv(a->N, 256) * batch;
        const dim3 g2(dicow_cdiv(t2, dicow_cdiv(t2, NT2_SLOTS * p.ncu)));
        if (colsum_rows) *colsum_rows = 2 * dicow_cdiv(a->M, 128);
        disp_note("gemm_nt2_kernel<%d>", f_);
        switch (f_) {
#define X(F) case (F): hipLaunchKernelGGL((gemm_nt2_kernel<(F)>), g2, dim3(256), NT2_LDS, stream, *a, nt2_delay); break;
            NT_EPILOGUES_COMMON(X)
#undef X
        }
        DICOW_CHECK_LAUNCH("gemm_nt2 (persistent, two workgroups per CU)");
        return DICOW_OK;
    }
    return NT_NOT_ROUTED;
}
#endif

// The hook of gemm_nt_impl, called with the validated arguments and the plan of a problem the skinny kernel did not take: the result of
// a launch (DICOW_OK or an error), or NT_NOT_ROUTED where the shipped kernels are to run the plan.
static int nt_experiment_route(dicow_gemm_args* a, const nt_plan_t& p, int variant, bool want_colsum, bool* fused_colsum, int* colsum_rows,
                               hipStream_t stream) {
    static std::once_flag once;
    std::call_once(once, nt_experiment_setup);
#ifdef DICOW_ABLATIONS
    if (variant != 0) return nt_ablation_route(a, p, variant, want_colsum, fused_colsum, colsum_rows, stream);
#endif
#if NT_EXPERIMENT_KERNELS
    if (p.family == NT_FAM_RING) {
        const int rc = nt_mask_route(a, p, want_colsum, fused_colsum, colsum_rows, stream);
        if (rc != NT_NOT_ROUTED) return rc;
    }
#endif
#if NT128W
    // mid-size problems on 128 x 256 ring tiles where its (one workgroup per CU) rounds are at least 70 % full
    const int64_t tw = (int64_t)dicow_cdiv(a->M, 128) * dicow_cdiv(a->N, 256) * (a->batch > 0 ? a->batch : 1);
    if (p.family == NT_FAM_128T && a->N >= 256 && a->M >= 128 && tw >= NT128W_MIN_TILES && tw * 10 >= dicow_cdiv(tw, g_ncu_all) * g_ncu_all * 7) {
        const dim3 gw(dicow_cdiv(a->M, 128) * dicow_cdiv(a->N, 256), 1, a->batch > 0 ? a->batch : 1);
        hipLaunchKernelGGL(gemm_nt128w_kernel, gw, dim3(256), NT128W_LDS, stream, *a);
        disp_note("gemm_nt128w_kernel");
        DICOW_CHECK_LAUNCH("gemm_nt");
        return DICOW_OK;
    }
#endif
    (void)variant;
    return NT_NOT_ROUTED;
}

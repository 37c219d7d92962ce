// translation unit: moment matrices of the stored states -- the sums kernel (wafer_moments.hip.h) and its launch on a context
// (the entry point of the C ABI, wafer_moment_matrices, is in wafer_engine_solve.hip)
#include "wafer_engine.h"
#include "wafer_elementwise.hip.h"
#include "wafer_moments.hip.h"

namespace {
template <typename F>
auto by_type_and_reach(const wafer_ctx *c, F &&f)
{
    const int R = c->g.R;
    if (c->f32) {
        if (R == 1) return f(float{}, std::integral_constant<int, 1>{});
        if (R == 2) return f(float{}, std::integral_constant<int, 2>{});
        return f(float{}, std::integral_constant<int, 3>{});
    }
    if (R == 1) return f(double{}, std::integral_constant<int, 1>{});
    if (R == 2) return f(double{}, std::integral_constant<int, 2>{});
    return f(double{}, std::integral_constant<int, 3>{});
}

// the partition of the context's observables launch (wafer_launch_observables_lds; ritz_sums_launch of wafer_tu_ritz.hip)
template <typename T, int R>
struct Partition {
    int zchunk, ntx, nty;
    long long nb;
    Partition(const WaferTuning &t, const WaferStepArgs &a)
    {
        constexpr int NW = WaferRitzCfg<R>::NW;
        using Cfg = WaferLdsCfg<T, R, 2, NW>;
        zchunk = wafer_lds_zchunk<T, R>(t, a.g, a.lz_hi - a.lz_lo, 2 * (NW / 4), a.target_blocks);
        ntx = (a.g.nx + Cfg::TX - 1) / Cfg::TX;
        nty = (a.g.ny + Cfg::TY - 1) / Cfg::TY;
        nb = (long long)ntx * nty * ((a.lz_hi - a.lz_lo + zchunk - 1) / zchunk);
    }
};
} // namespace

namespace wafer_eng __attribute__((visibility("hidden"))) {
// The five matrices of the first k stored states (checked by the caller) into m[(q * k + j) * k + i]: one sums launch, one reduce,
// one read-back.  The entries i > j are copies of their mirror images: l * w commutes, so the copy is exact.
int moment_matrices(wafer_ctx *c, uint32_t k, double *m)
{
    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_moment_matrices");
    const WaferStepArgs sa = ritz_args(c);
    const long long nb = by_type_and_reach(c, [&](auto t, auto r) { return Partition<decltype(t), decltype(r)::value>(c->tune, sa).nb; });
    const size_t rows = (size_t)wafer_moment_rows((int)k);
    TRY(ensure_ritz_buf(c, rows * (size_t)nb + rows));
    WaferRitzPtrs st;
    for (uint32_t i = 0; i < k; ++i) st.p[i] = c->states[i];
    double *sums = c->ritz_buf + rows * (size_t)nb;
    by_type_and_reach(c, [&](auto t, auto r) {
        using T = decltype(t);
        constexpr int R = decltype(r)::value;
        const Partition<T, R> p(c->tune, sa);
        WaferStepArgs a = sa;
        a.zchunk = p.zchunk;
        hipLaunchKernelGGL((wafer_k_moment_sums<R, T>), dim3((unsigned)p.nb, (unsigned)k), dim3(WaferRitzCfg<R>::NW * 64), 0,
                           c->s_main, a, p.ntx, p.nty, wafer_lds_opts(c->tune).swz, (int)k, st, c->ritz_buf, p.nb);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(wafer_k_reduce, dim3((unsigned)rows), dim3(256), 0, c->s_main, c->ritz_buf, nb, nb, sums);
    HIP_TRY(hipGetLastError());
    double host[WAFER_MOMENT_COUNT * WAFER_RITZ_MAX * (WAFER_RITZ_MAX + 1) / 2];
    HIP_TRY(hipMemcpyAsync(host, sums, sizeof(double) * rows, hipMemcpyDeviceToHost, c->s_main));
    HIP_TRY(hipStreamSynchronize(c->s_main));
    const size_t tri = (size_t)wafer_moment_tri((int)k);
    for (size_t q = 0; q < WAFER_MOMENT_COUNT; ++q)
        for (size_t j = 0; j < k; ++j)
            for (size_t i = 0; i <= j; ++i) {
                const double v = host[q * tri + (size_t)wafer_moment_tri((int)j) + i];
                m[(q * k + j) * k + i] = v;
                m[(q * k + i) * k + j] = v;
            }
    return WAFER_OK;
}
} // namespace wafer_eng

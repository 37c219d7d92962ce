// translation unit: Rayleigh-Ritz on the stored states -- the sums kernel, the rotation kernel (wafer_ritz.hip.h), the host solver
// (wafer_ritz.h) and the four entry points of the C ABI that combine them
#include "wafer_engine.h"
#include "wafer_elementwise.hip.h"
#include "wafer_ritz.hip.h"
#include "wafer_ritz.h"

namespace wafer_eng __attribute__((visibility("hidden"))) {
// the argument block of the context's observables launch (wafer_observables)
WaferStepArgs ritz_args(const wafer_ctx *c)
{
    WaferStepArgs sa{};
    sa.g = c->g;
    sa.lz_lo = c->g.G;
    sa.lz_hi = c->g.G + c->g.nzl;
    sa.dt = c->P.dt;
    set_den_args(c, sa);
    sa.target_blocks = c->num_cus;
    sa.v_in_range = short_forms(c) ? 1 : 0;
    return sa;
}

// ritz_buf: [2 k^2 rows of nb partials][2 k^2 sums][k^2 coefficients], for the largest k and nb asked for so far (the residual
// calls of wafer_tu_residual.hip keep their 3 k rows and sums there too)
int ensure_ritz_buf(wafer_ctx *c, size_t doubles)
{
    if (c->ritz_cap >= doubles) return WAFER_OK;
    HIP_TRY(hipStreamSynchronize(c->s_main));
    if (c->ritz_buf) (void)hipFree(c->ritz_buf);
    c->ritz_buf = nullptr;
    c->ritz_cap = 0;
    HIP_TRY(hipMalloc((void **)&c->ritz_buf, sizeof(double) * doubles));
    c->ritz_cap = doubles;
    return WAFER_OK;
}
} // namespace wafer_eng

namespace {
// the partition of the context's observables launch (wafer_launch_observables_lds) and the sums launch on it
template <typename T, int R>
hipError_t ritz_sums_launch(const WaferTuning &t, WaferStepArgs a, int k, const WaferRitzPtrs &st, const void *pv, double *partials, hipStream_t s)
{
    constexpr int NW = WaferRitzCfg<R>::NW;
    using Cfg = WaferLdsCfg<T, R, 2, NW>;
    a.zchunk = wafer_lds_zchunk<T, R>(t, a.g, a.lz_hi - a.lz_lo, 2 * (NW / 4), a.target_blocks);
    const int ntx = (a.g.nx + Cfg::TX - 1) / Cfg::TX;
    const int nty = (a.g.ny + Cfg::TY - 1) / Cfg::TY;
    const int ntz = (a.lz_hi - a.lz_lo + a.zchunk - 1) / a.zchunk;
    const long long nb = (long long)ntx * nty * ntz;
    hipLaunchKernelGGL((wafer_k_ritz_sums<R, T>), dim3((unsigned)nb, (unsigned)k), dim3(NW * 64), 0, s, a, ntx, nty, wafer_lds_opts(t).swz, k, st,
                       static_cast<const T *>(pv), partials, nb);
    return hipGetLastError();
}

template <typename T, int R>
long long ritz_blocks(const WaferTuning &t, const WaferStepArgs &a)
{
    constexpr int NW = WaferRitzCfg<R>::NW;
    using Cfg = WaferLdsCfg<T, R, 2, NW>;
    const int zc = wafer_lds_zchunk<T, R>(t, a.g, a.lz_hi - a.lz_lo, 2 * (NW / 4), a.target_blocks);
    return (long long)((a.g.nx + Cfg::TX - 1) / Cfg::TX) * ((a.g.ny + Cfg::TY - 1) / Cfg::TY) * ((a.lz_hi - a.lz_lo + zc - 1) / zc);
}

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

int check_k(const wafer_ctx *c, uint32_t k, bool need_pot)
{
    if (!c) return fail(WAFER_ERR_INVALID, "null context");
    if (k == 0 || k > WAFER_RITZ_MAX) return fail(WAFER_ERR_INVALID, "k = %u: Rayleigh-Ritz takes 1 .. %d states", k, WAFER_RITZ_MAX);
    if (c->P.z_count != 0)
        return fail(WAFER_ERR_INVALID, "Rayleigh-Ritz is not available on a context that owns a z-slab (the sums would need an all-reduce "
                                       "and the stored states their ghost planes)");
    if (k > c->states.size()) return fail(WAFER_ERR_STATE, "k = %u but w_store holds %zu states", k, c->states.size());
    if (need_pot && !c->have_pot) return fail(WAFER_ERR_STATE, "potential not set");
    return WAFER_OK;
}

int ritz_matrices_impl(wafer_ctx *c, uint32_t k, double *h, double *s)
{
    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_ritz_matrices");
    const WaferStepArgs sa = ritz_args(c);
    const long long nb = by_type_and_reach(c, [&](auto t, auto r) { return ritz_blocks<decltype(t), decltype(r)::value>(c->tune, sa); });
    const size_t rows = 2 * (size_t)k * k;
    TRY(ensure_ritz_buf(c, rows * (size_t)nb + rows + (size_t)WAFER_RITZ_MAX * WAFER_RITZ_MAX));
    WaferRitzPtrs st;
    for (uint32_t i = 0; i < k; ++i) st.p[i] = c->states[i];
    double *sums = c->ritz_buf + rows * (size_t)nb;
    const hipError_t e = by_type_and_reach(c, [&](auto t, auto r) {
        return ritz_sums_launch<decltype(t), decltype(r)::value>(c->tune, sa, (int)k, st, c->v, c->ritz_buf, c->s_main);
    });
    if (e != hipSuccess) return fail(WAFER_ERR_HIP, "Rayleigh-Ritz sums launch failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(wafer_k_reduce, dim3((unsigned)rows), dim3(256), 0, c->s_main, c->ritz_buf, nb, nb, sums);
    HIP_TRY(hipGetLastError());
    double host[2 * WAFER_RITZ_MAX * WAFER_RITZ_MAX];
    HIP_TRY(hipMemcpyAsync(host, sums, sizeof(double) * rows, hipMemcpyDeviceToHost, c->s_main));
    HIP_TRY(hipStreamSynchronize(c->s_main));
    for (size_t q = 0; q < (size_t)k * k; ++q) {
        h[q] = host[q];
        s[q] = host[(size_t)k * k + q];
    }
    return WAFER_OK;
}

int rotate_impl(wafer_ctx *c, uint32_t k, const double *coef)
{
    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_rotate_states");
    TRY(ensure_ritz_buf(c, (size_t)WAFER_RITZ_MAX * WAFER_RITZ_MAX));
    double *dcoef = c->ritz_buf + (c->ritz_cap - (size_t)WAFER_RITZ_MAX * WAFER_RITZ_MAX);
    HIP_TRY(hipMemcpyAsync(dcoef, coef, sizeof(double) * k * k, hipMemcpyHostToDevice, c->s_main));
    HIP_TRY(hipStreamSynchronize(c->s_main));   // coef is the caller's pageable memory
    WaferRitzPtrs st;
    for (uint32_t i = 0; i < k; ++i) st.p[i] = alloc_base(c, c->states[i]);
    const long long n16 = (long long)c->g.total * (long long)c->esz / 16;
    const long long want = (n16 + 255) / 256;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, (long long)c->num_cus * 8));
    if (c->f32)
        hipLaunchKernelGGL((wafer_k_rotate_states<float>), dim3(grid), dim3(256), 0, c->s_main, n16, (int)k, st, dcoef);
    else
        hipLaunchKernelGGL((wafer_k_rotate_states<double>), dim3(grid), dim3(256), 0, c->s_main, n16, (int)k, st, dcoef);
    HIP_TRY(hipGetLastError());
    // the store changed: the Gram matrix is recomputed, and the two-step pass rebuilds its images M_j on demand
    return recompute_gram(c);
}

int solve_checked(uint32_t k, const double *h, const double *s, double *evals, double *coef)
{
    switch (wafer_ritz_solve_host((int)k, h, s, evals, coef)) {
    case WAFER_RITZ_OK: return WAFER_OK;
    case WAFER_RITZ_NO_CONVERGENCE: return fail(WAFER_ERR_STATE, "Rayleigh-Ritz: the Jacobi iteration did not converge in %d sweeps", (int)WAFER_RITZ_SWEEPS);
    default: return fail(WAFER_ERR_STATE, "Rayleigh-Ritz: the overlap matrix is not positive definite (linearly dependent states, or a non-finite sum)");
    }
}
} // namespace

extern "C" {

int wafer_ritz_solve(uint32_t k, const double *h, const double *s, double *evals, double *coef)
{
    if (!h || !s || !evals || !coef) return fail(WAFER_ERR_INVALID, "null argument");
    if (k == 0 || k > WAFER_RITZ_MAX) return fail(WAFER_ERR_INVALID, "k = %u: Rayleigh-Ritz takes 1 .. %d states", k, WAFER_RITZ_MAX);
    return solve_checked(k, h, s, evals, coef);
}

int wafer_ritz_matrices(wafer_ctx *c, uint32_t k, double *h, double *s)
{
    TRY(check_k(c, k, true));
    if (!h || !s) return fail(WAFER_ERR_INVALID, "null argument");
    return ritz_matrices_impl(c, k, h, s);
}

int wafer_rotate_states(wafer_ctx *c, uint32_t k, const double *coef)
{
    TRY(check_k(c, k, false));
    if (!coef) return fail(WAFER_ERR_INVALID, "null argument");
    for (uint32_t q = 0; q < k * k; ++q)
        if (!std::isfinite(coef[q])) return fail(WAFER_ERR_INVALID, "coef[%u] is not finite", q);
    return rotate_impl(c, k, coef);
}

int wafer_ritz(wafer_ctx *c, uint32_t k, double *evals, double *coef, double *h, double *s)
{
    TRY(check_k(c, k, true));
    if (!evals || !coef) return fail(WAFER_ERR_INVALID, "null argument");
    double hm[WAFER_RITZ_MAX * WAFER_RITZ_MAX], sm[WAFER_RITZ_MAX * WAFER_RITZ_MAX];
    double ev[WAFER_RITZ_MAX], cf[WAFER_RITZ_MAX * WAFER_RITZ_MAX];
    TRY(ritz_matrices_impl(c, k, hm, sm));
    TRY(solve_checked(k, hm, sm, ev, cf));   // a failed solve leaves the store and the outputs as they were
    TRY(rotate_impl(c, k, cf));
    for (uint32_t q = 0; q < k * k; ++q) {
        coef[q] = cf[q];
        if (h) h[q] = hm[q];
        if (s) s[q] = sm[q];
    }
    for (uint32_t q = 0; q < k; ++q) evals[q] = ev[q];
    return WAFER_OK;
}

} // extern "C"

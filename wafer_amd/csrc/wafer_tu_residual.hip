// translation unit: residuals r = H l - theta l of the stored states and of phi -- the sums kernel and the writer
// (wafer_residual.hip.h) and the two entry points of the C ABI on a context (wafer_residuals, wafer_residual_to_phi); on the writer's
// partition and body, the Chebyshev filter of the stored states (wafer_filter_states, wafer_filter_coefficients: wafer_filter.h) and
// the upper bound of H's spectrum it needs (wafer_spectral_bound)
#include "wafer_engine.h"
#include "wafer_filter.h"
#include "wafer_batch_plan.h"   // (the parity of the filter's two arrays: wafer_batch_filter_src_is_shadow)
#include "wafer_elementwise.hip.h"
#include "wafer_residual.hip.h"

namespace {
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

int refuse_slab(const wafer_ctx *c)
{
    if (c->P.z_count == 0) return WAFER_OK;
    return fail(WAFER_ERR_INVALID, "residuals are not available on a context that owns a z-slab (the sums would need an all-reduce and the "
                                   "stored states their ghost planes)");
}

// one pass: the sums launch on the k sources in st with theta, the reduce, one read-back; out[j * 3 + (r2, wh, s)]
int sums_pass(wafer_ctx *c, uint32_t k, const WaferRitzPtrs &st, const WaferResidualTheta &theta, double *out)
{
    WaferStepArgs sa = ritz_args(c);
    const long long nb = by_type_and_reach(c, [&](auto t, auto r) { return Partition<decltype(t), decltype(r)::value>(c->tune, sa).nb; });
    const size_t rows = 3 * (size_t)k;
    TRY(ensure_ritz_buf(c, rows * (size_t)nb + rows));
    double *sums = c->ritz_buf + rows * (size_t)nb;
    by_type_and_reach(c, [&](auto t, auto r) {
        using T = decltype(t);
        constexpr int R = decltype(r)::value;
        const Partition<T, R> p(c->tune, sa);
        WaferStepArgs a = sa;
        a.zchunk = p.zchunk;
        hipLaunchKernelGGL((wafer_k_residual_sums<R, T>), dim3((unsigned)p.nb, (unsigned)k), dim3(WaferRitzCfg<R>::NW * 64), 0, c->s_main, a, p.ntx,
                           p.nty, wafer_lds_opts(c->tune).swz, st, theta, static_cast<const T *>(c->v), c->ritz_buf, p.nb);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(wafer_k_reduce, dim3((unsigned)rows), dim3(256), 0, c->s_main, c->ritz_buf, nb, nb, sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sums, sizeof(double) * rows, hipMemcpyDeviceToHost, c->s_main));
    HIP_TRY(hipStreamSynchronize(c->s_main));
    return WAFER_OK;
}
} // namespace

extern "C" {

int wafer_residuals(wafer_ctx *c, int source, uint32_t k, const double *theta_in, double *theta, double *r2, double *s)
{
    if (!c) return fail(WAFER_ERR_INVALID, "null context");
    if (!theta || !r2 || !s) return fail(WAFER_ERR_INVALID, "null argument");
    if (source != WAFER_RESIDUAL_STATES && source != WAFER_RESIDUAL_PHI) return fail(WAFER_ERR_INVALID, "unknown residual source %d", source);
    if (k == 0 || k > WAFER_RITZ_MAX) return fail(WAFER_ERR_INVALID, "k = %u: residuals take 1 .. %d states", k, WAFER_RITZ_MAX);
    if (source == WAFER_RESIDUAL_PHI && k != 1) return fail(WAFER_ERR_INVALID, "k = %u: the phi source is one array (k = 1)", k);
    if (theta_in)
        for (uint32_t j = 0; j < k; ++j)
            if (!std::isfinite(theta_in[j])) return fail(WAFER_ERR_INVALID, "theta_in[%u] is not finite", j);
    TRY(refuse_slab(c));
    if (source == WAFER_RESIDUAL_STATES && k > c->states.size()) return fail(WAFER_ERR_STATE, "k = %u but w_store holds %zu states", k, c->states.size());
    if (source == WAFER_RESIDUAL_PHI && !c->have_phi) return fail(WAFER_ERR_STATE, "phi not set");
    if (!c->have_pot) return fail(WAFER_ERR_STATE, "potential not set");

    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_residuals");
    WaferRitzPtrs st;
    if (source == WAFER_RESIDUAL_PHI) st.p[0] = c->phi[c->cur];
    else
        for (uint32_t j = 0; j < k; ++j) st.p[j] = c->states[j];
    WaferResidualTheta th;
    double host[3 * WAFER_RITZ_MAX];
    if (theta_in) {
        for (uint32_t j = 0; j < k; ++j) th.t[j] = theta_in[j];
    } else {   // Rayleigh mode: theta_j = wh_j / s_j of a pass with theta = 0
        TRY(sums_pass(c, k, st, th, host));
        for (uint32_t j = 0; j < k; ++j) {
            const double sj = host[j * 3 + 2];
            if (!std::isfinite(sj) || !(sj > 0.0))
                return fail(WAFER_ERR_STATE, "state %u: <l|l> = %g: no Rayleigh quotient (a zero or non-finite state)", j, sj);
            th.t[j] = host[j * 3 + 1] / sj;
        }
    }
    TRY(sums_pass(c, k, st, th, host));
    for (uint32_t j = 0; j < k; ++j) {
        theta[j] = th.t[j];
        r2[j] = host[j * 3 + 0];
        s[j] = host[j * 3 + 2];
    }
    return WAFER_OK;
}

int wafer_residual_to_phi(wafer_ctx *c, uint32_t idx, double theta)
{
    if (!c) return fail(WAFER_ERR_INVALID, "null context");
    if (!std::isfinite(theta)) return fail(WAFER_ERR_INVALID, "theta is not finite");
    TRY(refuse_slab(c));
    if (idx >= c->states.size()) return fail(WAFER_ERR_STATE, "no state %u", idx);
    if (!c->have_pot) return fail(WAFER_ERR_STATE, "potential not set");
    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_residual_to_phi");
    const WaferStepArgs sa = ritz_args(c);
    const long long n16 = (long long)c->g.total * (long long)c->esz / 16;
    by_type_and_reach(c, [&](auto t, auto r) {
        using T = decltype(t);
        constexpr int R = decltype(r)::value;
        const Partition<T, R> p(c->tune, sa);
        WaferStepArgs a = sa;
        a.zchunk = p.zchunk;
        hipLaunchKernelGGL((wafer_k_residual_write<R, T>), dim3((unsigned)p.nb), dim3(WaferRitzCfg<R>::NW * 64), 0, c->s_main, a, p.ntx, p.nty,
                           wafer_lds_opts(c->tune).swz, static_cast<const T *>(c->states[idx]), theta, static_cast<const T *>(c->v),
                           static_cast<T *>(c->phi[c->cur]), n16);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    c->have_phi = true;
    c->halo_valid = 0;
    return WAFER_OK;
}

int wafer_filter_coefficients(uint32_t degree, double a, double b, double a0, double *al, double *be, double *cc)
{
    if (!al || !be || !cc) return fail(WAFER_ERR_INVALID, "null argument");
    switch (wafer_filter_coefficients_host(degree, a, b, a0, al, be, cc)) {
    case WAFER_FILTER_OK: return WAFER_OK;
    case WAFER_FILTER_BAD_DEGREE: return fail(WAFER_ERR_INVALID, "degree = %u: the filter takes 1 .. %d", degree, WAFER_FILTER_MAX_DEGREE);
    default: return fail(WAFER_ERR_INVALID, "the interval needs finite a0 < a < b (a0 = %g, a = %g, b = %g)", a0, a, b);
    }
}

// The first k stored states through `degree` steps of the recurrence, one launch per state and step between the state's slot and the
// context's shadow array: step 1 writes the shadow (whole: zeros outside the work cells), step i >= 2 writes its result over the
// iterate before last.  After an odd degree the result stands in the shadow: the two pointers change places, as in
// wafer_evolve_states.  phi, cur, have_phi and halo_valid are not touched.
int wafer_filter_states(wafer_ctx *c, uint32_t k, uint32_t degree, double a, double b, double a0)
{
    if (!c) return fail(WAFER_ERR_INVALID, "null context");
    if (k == 0 || k > WAFER_RITZ_MAX) return fail(WAFER_ERR_INVALID, "k = %u: wafer_filter_states filters 1 .. %d states", k, WAFER_RITZ_MAX);
    if (c->P.z_count != 0)
        return fail(WAFER_ERR_INVALID, "wafer_filter_states is not available on a context that owns a z-slab (the stored states carry no ghost planes)");
    double al[WAFER_FILTER_MAX_DEGREE], be[WAFER_FILTER_MAX_DEGREE], cc = 0.0;
    TRY(wafer_filter_coefficients(degree, a, b, a0, al, be, &cc));
    if (k > c->states.size()) return fail(WAFER_ERR_STATE, "k = %u but w_store holds %zu states", k, c->states.size());
    if (!c->have_pot) return fail(WAFER_ERR_STATE, "potential not set");
    HIP_TRY(hipSetDevice(c->P.device));
    RoctxRange range_("wafer_filter_states");
    if (!c->state_shadow) TRY(alloc_grid_array(c, &c->state_shadow, c->s_main));
    const WaferStepArgs sa = ritz_args(c);
    const long long n16 = (long long)c->g.total * (long long)c->esz / 16;
    HIP_TRY(hipEventRecord(c->ev_start, c->s_main));
    // "A refused call changes nothing" ends here: it speaks of the checks above.  A HIP error below returns at once, as in
    // wafer_evolve_states: the states before j are then filtered (and, after an odd degree, have changed places with the shadow --
    // every pointer still names an array the context owns), state j is part-way, and the Gram matrix is not recomputed.  The caller
    // loads the states again or destroys the context.
    for (uint32_t j = 0; j < k; ++j) {
        void *const slot = c->states[j], *const shadow = c->state_shadow;
        for (uint32_t i = 1; i <= degree; ++i) {
            const bool from_shadow = wafer_batch_filter_src_is_shadow(i);
            const void *src = from_shadow ? shadow : slot;
            void *dst = from_shadow ? slot : shadow;
            by_type_and_reach(c, [&](auto t, auto r) {
                using T = decltype(t);
                constexpr int R = decltype(r)::value;
                const Partition<T, R> p(c->tune, sa);
                WaferStepArgs ar = sa;
                ar.zchunk = p.zchunk;
                const dim3 grid((unsigned)p.nb), block(WaferRitzCfg<R>::NW * 64);
                const int swz = wafer_lds_opts(c->tune).swz;
                if (i == 1)
                    hipLaunchKernelGGL((wafer_k_filter_step<R, T, true>), grid, block, 0, c->s_main, ar, p.ntx, p.nty, swz, static_cast<const T *>(src),
                                       static_cast<const T *>(c->v), static_cast<T *>(dst), al[0], be[0], cc, n16);
                else
                    hipLaunchKernelGGL((wafer_k_filter_step<R, T, false>), grid, block, 0, c->s_main, ar, p.ntx, p.nty, swz, static_cast<const T *>(src),
                                       static_cast<const T *>(c->v), static_cast<T *>(dst), al[i - 1], be[i - 1], cc, n16);
                return 0;
            });
            HIP_TRY(hipGetLastError());
        }
        if (degree & 1) {
            c->states[j] = shadow;
            c->state_shadow = slot;
        }
    }
    HIP_TRY(hipEventRecord(c->ev_stop, c->s_main));
    c->last_steps = degree;
    c->timing_valid = true;
    // the store changed: the Gram matrix is recomputed, and the two-step pass rebuilds its images M_j on demand
    return recompute_gram(c);
}

// ub = W_R / den + max V over the work cells (Gershgorin): no eigenvalue of the discrete H lies above it
int wafer_spectral_bound(wafer_ctx *c, double *ub)
{
    if (!c || !ub) return fail(WAFER_ERR_INVALID, "null argument");
    if (c->P.z_count != 0) return fail(WAFER_ERR_INVALID, "wafer_spectral_bound is not available on a context that owns a z-slab (the maximum would need an all-reduce)");
    if (!c->have_pot) return fail(WAFER_ERR_STATE, "potential not set");
    HIP_TRY(hipSetDevice(c->P.device));
    TRY(ensure_ritz_buf(c, 1));
    unsigned long long *word = reinterpret_cast<unsigned long long *>(c->ritz_buf), key = 0;
    HIP_TRY(hipMemsetAsync(word, 0, sizeof key, c->s_main));   // below every key
    const dim3 grid((unsigned)(((c->g.nx + 63) / 64) * ((c->g.ny + 3) / 4)), (unsigned)c->g.nzl), block(64, 4);
    if (c->f32) hipLaunchKernelGGL((wafer_k_v_max<float>), grid, block, 0, c->s_main, c->g, static_cast<const float *>(c->v), word);
    else hipLaunchKernelGGL((wafer_k_v_max<double>), grid, block, 0, c->s_main, c->g, static_cast<const double *>(c->v), word);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&key, word, sizeof key, hipMemcpyDeviceToHost, c->s_main));
    HIP_TRY(hipStreamSynchronize(c->s_main));
    *ub = wafer_stencil_abs_weight(c->g.R) / wafer_stencil_den(c->g.R, c->P.dn, c->P.mass) + wafer_order_value(key);
    return WAFER_OK;
}

} // extern "C"

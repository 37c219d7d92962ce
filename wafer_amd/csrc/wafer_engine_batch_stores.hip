// wafer_engine_batch_stores.hip -- the batch engine's calls on the state stores beyond Gram-Schmidt (the batch, its creation and every
// other batched call: wafer_engine_batch.hip; what the two units share: wafer_engine_batch.h).
// Rayleigh-Ritz on the stores (wafer_batch_ritz_matrices, wafer_batch_rotate_states, wafer_batch_ritz; kernels: wafer_ritz_batch.hip.h,
// wafer_tu_ritz_batch.hip): a context's wafer_ritz_* for every listed member with its own k -- one sums launch, one reduce and one
// read-back, the solves on the host (wafer_ritz.h), one rotation launch -- from a per-call table of (member, k, partials offset, span).
// Residuals (wafer_batch_residuals; kernels: wafer_residual_batch.hip.h, wafer_tu_residual_batch.hip): a context's wafer_residuals for
// every listed member with its own k and theta, on the stores or on phi -- one sums launch, one reduce and one read-back per pass.
// Moment matrices (wafer_batch_moment_matrices; kernels: wafer_moments_batch.hip.h, wafer_tu_moments_batch.hip): a context's
// wafer_moment_matrices for every listed member with its own k -- one sums launch, one reduce and one read-back.
// Stepping the stores (wafer_batch_evolve_states; kernels: wafer_store_step_batch.hip.h, wafer_tu_store_step_batch*.hip): the first k[m]
// stored states of every listed member advance by n plain steps, one launch per step over the listed members' workgroup table,
// between the slots and shadow slots laid out as they are; an odd n ends with one batched copy back into the slots.
// Filtering the stores (wafer_batch_filter_states; kernels: wafer_store_filter_batch.hip.h, wafer_tu_store_filter_batch*.hip): a
// degree-m Chebyshev polynomial of H itself on the same states, tables and two sets of slots, one launch per recurrence step, each
// member with its own interval; wafer_batch_spectral_bound gives the interval's upper end from one launch and one read-back.
#include "wafer_engine_batch.h"
#include "wafer_store_step_batch.hip.h"
#include "wafer_store_filter_batch.hip.h"
#include "wafer_ritz.h"

namespace {

// ---- Rayleigh-Ritz on the stores ---------------------------------------------------------------------------------------------
constexpr size_t RITZ_KK = (size_t)WAFER_RITZ_MAX * WAFER_RITZ_MAX;

// every check of a call for every listed member, before anything is uploaded or launched; *nlisted: their number
int ritz_check(const wafer_batch *b, const uint8_t *active, const uint32_t *k, bool need_pot, const char *call, int *nlisted)
{
    TRY(refuse_mixed(b, call));
    *nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (k[m] == 0 || k[m] > WAFER_RITZ_MAX)
            return fail(WAFER_ERR_INVALID, "member %u: k = %u: Rayleigh-Ritz takes 1 .. %d states", m, k[m], WAFER_RITZ_MAX);
        if (k[m] > b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: k = %u but w_store holds %u states", m, k[m], b->nst[m]);
        if (need_pot && !b->views[m]->have_pot) return fail(WAFER_ERR_STATE, "member %u: potential not set", m);
        ++*nlisted;
    }
    return WAFER_OK;
}

int ensure_ritz(wafer_batch *b)
{
    if (b->ritz_coef.dev) return WAFER_OK;   // (made last: a call that failed before it starts over)
    BUF_TRY(b->ritz_rec.make(b->n));
    BUF_TRY(b->ritz_sums.make(2 * RITZ_KK * b->n));
    BUF_TRY(b->ritz_coef.make(RITZ_KK * b->n));
    memset(b->ritz_coef.host, 0, b->ritz_coef.host.bytes());
    return WAFER_OK;
}

// What a per-call table gives its call: the listed members' number, the widest partition and the largest k among them, the grid of a
// kernel that walks their spans in 16-byte vectors, the length of their partials end to end, the first listed member and the last + 1.
struct CallTable {
    int nact = 0, max_nb = 0, max_k = 0, blocks = 1;
    size_t doubles = 0, m0 = 0, m1 = 0;
};

// The per-call table of the listed members into t's host side and to the device: member, k, the prefix sums of the member's rows of
// obs_nb partials -- 2 k^2 and the member's span in a slot allocation (WaferBatchRitzRec), 3 k and theta (WaferBatchResidualRec:
// member m's at m * WAFER_RITZ_MAX; nullptr: zeros), or 5 k (k + 1) / 2 (WaferBatchMomentRec).  partials: ritz_partials holds them when this returns, grown on demand as a
// context's ritz_buf.  The stream is idle (the callers synchronised: t's host side is not read by an earlier copy, and no launch
// reads partials that go back).
template <typename Rec>
int upload_table(wafer_batch *b, Mirror<Rec> &t, const uint8_t *listed, const uint32_t *k, const double *theta, bool partials, CallTable *c)
{
    constexpr bool ritz = std::is_same<Rec, WaferBatchRitzRec>::value, resid = std::is_same<Rec, WaferBatchResidualRec>::value;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (listed && !listed[m]) continue;
        Rec &r = t[c->nact++];
        r.member = (int)m;
        r.k = (int)k[m];
        r.poff = (long long)c->doubles;
        if constexpr (ritz) {
            r.v0 = (long long)(b->off[m] * b->esz / 16);
            r.n16 = (long long)((size_t)b->geom(m).total * b->esz / 16);
            c->blocks = std::max(c->blocks, (int)std::min<long long>((r.n16 + 255) / 256, (long long)b->num_cus * 8));
        } else if constexpr (resid) {
            for (uint32_t j = 0; j < WAFER_RITZ_MAX; ++j) r.theta[j] = (theta && j < k[m]) ? theta[(size_t)m * WAFER_RITZ_MAX + j] : 0.0;
        }
        const size_t rows = ritz ? 2 * (size_t)k[m] * k[m] : resid ? 3 * (size_t)k[m] : (size_t)wafer_moment_rows((int)k[m]);
        c->doubles += rows * (size_t)b->mem[m].obs_nb;
        c->max_nb = std::max(c->max_nb, b->mem[m].obs_nb);
        c->max_k = std::max(c->max_k, (int)k[m]);
    }
    if (!c->nact) return WAFER_OK;
    c->m0 = (size_t)t[0].member;
    c->m1 = (size_t)t[c->nact - 1].member + 1;
    if (partials) BUF_TRY(b->ritz_partials.reserve(c->doubles));
    BUF_TRY(t.upload(c->nact, b->s));
    return WAFER_OK;
}

// the allocations of the store slots (or of their shadows) the kernels may touch
WaferRitzPtrs ritz_slots(const std::vector<DevArray<char>> &v)
{
    WaferRitzPtrs st;
    for (size_t l = 0; l < WAFER_RITZ_MAX && l < v.size(); ++l) st.p[l] = v[l];
    return st;
}

// H and S of every listed member (checked: ritz_check) into ritz_sums' host side: the sums launch, the reduce, one read-back
int ritz_matrices_impl(wafer_batch *b, const uint8_t *active, const uint32_t *k)
{
    HIP_TRY(hipSetDevice(b->device));
    RoctxRange range_("wafer_batch_ritz_matrices");
    TRY(ensure_ritz(b));
    TRY(sync_members(b));
    HIP_TRY(hipStreamSynchronize(b->s));
    CallTable c;
    TRY(upload_table(b, b->ritz_rec, active, k, nullptr, true, &c));
    const WaferRitzPtrs st = ritz_slots(b->slots);
    TRY(launch(b, "Rayleigh-Ritz sums", [&](const auto &gs) {
        return wafer_entry_batch_ritz_sums(b->f32, b->g().R, gs, b->mem_dev, b->ritz_rec.dev, c.nact, c.max_nb, c.max_k, b->swz, st, b->ritz_partials,
                                           b->ritz_sums.dev, b->s);
    }));
    b->n_ritz_launches += 2;
    BUF_TRY(b->ritz_sums.download(2 * RITZ_KK * (c.m1 - c.m0), b->s, 2 * RITZ_KK * c.m0));
    HIP_TRY(hipStreamSynchronize(b->s));
    ++b->n_ritz_readbacks;
    return WAFER_OK;
}

// member m's k x k matrices out of ritz_sums' host side
void ritz_unpack(const wafer_batch *b, uint32_t m, uint32_t k, double *h, double *s)
{
    const double *r = &b->ritz_sums[(size_t)m * 2 * RITZ_KK];
    for (size_t q = 0; q < (size_t)k * k; ++q) {
        if (h) h[q] = r[q];
        if (s) s[q] = r[RITZ_KK + q];
    }
}

// the rotation of the listed members (checked; coef: member m's k[m] x k[m] at m * WAFER_RITZ_MAX^2, finite): one launch
int ritz_rotate_impl(wafer_batch *b, const uint8_t *listed, const uint32_t *k, const double *coef)
{
    HIP_TRY(hipSetDevice(b->device));
    RoctxRange range_("wafer_batch_rotate_states");
    TRY(ensure_ritz(b));
    HIP_TRY(hipStreamSynchronize(b->s));   // the pinned table and coefficients are not read by an earlier call's copy
    CallTable c;
    TRY(upload_table(b, b->ritz_rec, listed, k, nullptr, false, &c));
    if (!c.nact) return WAFER_OK;
    for (int q = 0; q < c.nact; ++q) {
        const uint32_t m = (uint32_t)b->ritz_rec[q].member;
        memcpy(&b->ritz_coef[m * RITZ_KK], coef + m * RITZ_KK, sizeof(double) * k[m] * k[m]);
    }
    BUF_TRY(b->ritz_coef.upload(RITZ_KK * (c.m1 - c.m0), b->s, RITZ_KK * c.m0));
    TRY(launched("rotation", wafer_entry_batch_rotate_states(b->f32, b->ritz_rec.dev, c.nact, c.blocks, ritz_slots(b->slots), b->ritz_coef.dev, b->s)));
    ++b->n_ritz_launches;
    for (int q = 0; q < c.nact; ++q) mark_gram_stale(b, (uint32_t)b->ritz_rec[q].member);   // the one-pass form sees the new store
    return WAFER_OK;
}

// ---- residuals of the stores and of phi ------------------------------------------------------------------------------------------
constexpr size_t RESID_ROWS = 3 * (size_t)WAFER_RITZ_MAX;

// every check of wafer_batch_residuals for every listed member, before anything is uploaded or launched; *nlisted: their number
int residual_check(const wafer_batch *b, int source, const uint8_t *active, const uint32_t *k, const double *theta_in, int *nlisted)
{
    if (source != WAFER_RESIDUAL_STATES && source != WAFER_RESIDUAL_PHI) return fail(WAFER_ERR_INVALID, "unknown residual source %d", source);
    if (source == WAFER_RESIDUAL_STATES) TRY(refuse_mixed(b, "wafer_batch_residuals (stored states)"));
    *nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (k[m] == 0 || k[m] > WAFER_RITZ_MAX)
            return fail(WAFER_ERR_INVALID, "member %u: k = %u: residuals take 1 .. %d states", m, k[m], WAFER_RITZ_MAX);
        if (source == WAFER_RESIDUAL_PHI && k[m] != 1) return fail(WAFER_ERR_INVALID, "member %u: k = %u: the phi source is one array (k = 1)", m, k[m]);
        if (theta_in)
            for (uint32_t j = 0; j < k[m]; ++j)
                if (!std::isfinite(theta_in[(size_t)m * WAFER_RITZ_MAX + j])) return fail(WAFER_ERR_INVALID, "member %u: theta_in[%u] is not finite", m, j);
        if (source == WAFER_RESIDUAL_STATES && k[m] > b->nst[m])
            return fail(WAFER_ERR_STATE, "member %u: k = %u but w_store holds %u states", m, k[m], b->nst[m]);
        if (source == WAFER_RESIDUAL_PHI && !b->views[m]->have_phi) return fail(WAFER_ERR_STATE, "member %u: phi not set", m);
        if (!b->views[m]->have_pot) return fail(WAFER_ERR_STATE, "member %u: potential not set", m);
        ++*nlisted;
    }
    return WAFER_OK;
}

int ensure_residual(wafer_batch *b)
{
    if (b->resid_sums.dev) return WAFER_OK;   // (made last: a call that failed before it starts over)
    BUF_TRY(b->resid_rec.make(b->n));
    BUF_TRY(b->resid_sums.make(RESID_ROWS * b->n));
    return WAFER_OK;
}

// One pass over the listed members (checked: residual_check; at least one): the per-call table with theta (member m's at
// m * WAFER_RITZ_MAX; nullptr: zeros), the sums launch, the reduce and one read-back into resid_sums' host side.
int residual_pass(wafer_batch *b, int source, const uint8_t *listed, const uint32_t *k, const double *theta)
{
    HIP_TRY(hipStreamSynchronize(b->s));   // the pinned table is not read by an earlier call's copy
    CallTable c;
    TRY(upload_table(b, b->resid_rec, listed, k, theta, true, &c));
    const WaferRitzPtrs st = ritz_slots(b->slots);
    TRY(launch(b, "residual sums", [&](const auto &gs) {
        return wafer_entry_batch_residual_sums(b->f32, b->g().R, gs, b->mem_dev, b->resid_rec.dev, c.nact, c.max_nb, c.max_k, b->swz,
                                               source == WAFER_RESIDUAL_PHI ? 1 : 0, st, b->ritz_partials, b->resid_sums.dev, b->s);
    }));
    b->n_resid_launches += 2;
    BUF_TRY(b->resid_sums.download(RESID_ROWS * (c.m1 - c.m0), b->s, RESID_ROWS * c.m0));
    HIP_TRY(hipStreamSynchronize(b->s));
    ++b->n_resid_readbacks;
    return WAFER_OK;
}

// ---- moment matrices of the stores -------------------------------------------------------------------------------------------
constexpr size_t MOMENT_ROWS = (size_t)WAFER_MOMENT_COUNT * RITZ_KK;

// every check of wafer_batch_moment_matrices for every listed member, before anything is uploaded or launched; *nlisted: their number
int moment_check(const wafer_batch *b, const uint8_t *active, const uint32_t *k, int *nlisted)
{
    TRY(refuse_mixed(b, "wafer_batch_moment_matrices"));
    *nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (k[m] == 0 || k[m] > WAFER_RITZ_MAX)
            return fail(WAFER_ERR_INVALID, "member %u: k = %u: moment matrices take 1 .. %d states", m, k[m], WAFER_RITZ_MAX);
        if (k[m] > b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: k = %u but w_store holds %u states", m, k[m], b->nst[m]);
        ++*nlisted;
    }
    return WAFER_OK;
}

int ensure_moments(wafer_batch *b)
{
    if (b->moment_sums.dev) return WAFER_OK;   // (made last: a call that failed before it starts over)
    BUF_TRY(b->moment_rec.make(b->n));
    BUF_TRY(b->moment_sums.make(MOMENT_ROWS * b->n));
    return WAFER_OK;
}

// the computed rows of every listed member (checked: moment_check; at least one) into moment_sums' host side: the per-call table,
// the sums launch, the reduce and one read-back
int moment_pass(wafer_batch *b, const uint8_t *active, const uint32_t *k)
{
    HIP_TRY(hipSetDevice(b->device));
    RoctxRange range_("wafer_batch_moment_matrices");
    TRY(ensure_moments(b));
    TRY(sync_members(b));
    HIP_TRY(hipStreamSynchronize(b->s));   // the pinned table is not read by an earlier call's copy
    CallTable c;
    TRY(upload_table(b, b->moment_rec, active, k, nullptr, true, &c));
    const WaferRitzPtrs st = ritz_slots(b->slots);
    TRY(launch(b, "moment sums", [&](const auto &gs) {
        return wafer_entry_batch_moment_sums(b->f32, b->g().R, gs, b->mem_dev, b->moment_rec.dev, c.nact, c.max_nb, c.max_k, b->swz, st,
                                             b->ritz_partials, b->moment_sums.dev, b->s);
    }));
    b->n_moment_launches += 2;
    BUF_TRY(b->moment_sums.download(MOMENT_ROWS * (c.m1 - c.m0), b->s, MOMENT_ROWS * c.m0));
    HIP_TRY(hipStreamSynchronize(b->s));
    ++b->n_moment_readbacks;
    return WAFER_OK;
}

// ---- stepping the stores -----------------------------------------------------------------------------------------------------
// every check of wafer_batch_evolve_states (and of wafer_batch_filter_states on its states: `call` names the one in the messages) for
// every listed member, before anything is allocated, uploaded or launched.
// A listed member with k[m] == 0 is allowed and costs nothing.  *max_k: the largest k among the listed members.
int store_step_check(const wafer_batch *b, const uint8_t *active, const uint32_t *k, const char *call, uint32_t *max_k)
{
    TRY(refuse_mixed(b, call));
    *max_k = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (k[m] > WAFER_RITZ_MAX) return fail(WAFER_ERR_INVALID, "member %u: k = %u: %s steps at most %d states", m, k[m], call, WAFER_RITZ_MAX);
        if (k[m] > b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: k = %u but w_store holds %u states", m, k[m], b->nst[m]);
        if (k[m] && !b->views[m]->have_pot) return fail(WAFER_ERR_STATE, "member %u: potential not set", m);
        *max_k = std::max(*max_k, k[m]);
    }
    return WAFER_OK;
}

// What wafer_batch_evolve_states and wafer_batch_filter_states share (checked: store_step_check gave max_k): `steps` launches of
// step_launch over the workgroup table of the listed members with k[m] > 0, between the slots and their shadows (wafer_batch_plan.h:
// wafer_batch_store_plan), and after an odd number of them one batched copy back into the slots; `counter` counts the launches.
// The caller's own table: alloc() makes it on first use, behind the pass's own allocations; upload(listed) fills and uploads it
// behind the ONE stream synchronisation, after which no earlier call's copy reads a pinned table.
// step_launch(t, gs, groups, src, dst) launches step t = 0 .. steps - 1.
template <typename Alloc, typename Upload, typename Step>
int store_pass(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint32_t max_k, const char *call, const char *what, uint64_t steps,
               uint64_t &counter, Alloc &&alloc, Upload &&upload, Step &&step_launch)
{
    HIP_TRY(hipSetDevice(b->device));
    RoctxRange range_(call);
    const WaferBatchStorePlan plan = wafer_batch_store_plan(steps, max_k);
    std::vector<uint8_t> listed(b->n);
    for (uint32_t m = 0; m < b->n; ++m) listed[m] = ((!active || active[m]) && k[m] > 0) ? 1 : 0;
    CallTable c;
    if (max_k) {
        TRY(ensure_slots(b, b->shadows, max_k));   // (zeroed: the kernel writes work cells only, frames and pads stay zeros)
        TRY(ensure_ritz(b));   // (the copy's per-call table)
        if (!b->store_k.dev) BUF_TRY(b->store_k.make(b->n));
        TRY(alloc());
        TRY(sync_members(b));
        TRY(build_blocks(b, b->blks, listed.data(), 1));
        HIP_TRY(hipStreamSynchronize(b->s));   // the pinned tables are not read by an earlier call's copy
        for (uint32_t m = 0; m < b->n; ++m) b->store_k[m] = listed[m] ? (int)k[m] : 0;
        BUF_TRY(b->store_k.upload(b->n, b->s));
        TRY(upload(listed.data()));
        if (plan.copy_back) TRY(upload_table(b, b->ritz_rec, listed.data(), k, nullptr, false, &c));
    }
    const WaferRitzPtrs slots = ritz_slots(b->slots), shadows = ritz_slots(b->shadows);   // (the kernels touch the first k[m] <= max_k of each)
    HIP_TRY(hipEventRecord(b->ev_start, b->s));
    if (max_k && !b->blks.host.empty()) {
        for (uint64_t t = 0; t < plan.steps; ++t) {   // no host synchronisation in here
            const bool from_shadow = wafer_batch_store_src_is_shadow(t);
            TRY(launch(b, what, [&](const auto &gs) { return step_launch(t, gs, plan.groups, from_shadow ? shadows : slots, from_shadow ? slots : shadows); }));
            ++counter;
        }
        if (plan.copy_back && c.nact) {
            TRY(launched("store copy", wafer_entry_batch_store_copy(b->ritz_rec.dev, c.nact, c.blocks, shadows, slots, b->s)));
            ++counter;
        }
    }
    HIP_TRY(hipEventRecord(b->ev_stop, b->s));
    b->last_steps = plan.steps;
    b->timing_valid = true;
    for (uint32_t m = 0; m < b->n; ++m)
        if (listed[m]) mark_gram_stale(b, m);   // the one-pass form sees the new store
    return WAFER_OK;
}

// n_steps plain steps (0 takes one) of the first k[m] stored states of every listed member: the store pass on the step kernel
int evolve_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint64_t n_steps)
{
    uint32_t max_k = 0;
    TRY(store_step_check(b, active, k, "wafer_batch_evolve_states", &max_k));
    const auto no_table = [](auto...) { return WAFER_OK; };
    return store_pass(b, active, k, max_k, "wafer_batch_evolve_states", "store step", n_steps == 0 ? 1 : n_steps, b->n_store_launches, no_table, no_table,
                      [&](uint64_t, const auto &gs, int groups, const WaferRitzPtrs &src, const WaferRitzPtrs &dst) {
                          return wafer_entry_batch_store_step(b->dtype, b->g().R, gs, b->mem_dev, b->blks.dev, (int)b->blks.host.size(), groups, b->store_k.dev,
                                                              src, dst, b->s);
                      });
}

// ---- filtering the stores ----------------------------------------------------------------------------------------------------
// wafer_batch_filter_states: the degree, store_step_check's checks and every listed member's interval, before anything is allocated,
// uploaded or launched; then the store pass of `degree` recurrence steps, with every step's coefficients of every member as its table.
int filter_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint32_t degree, const double *a, const double *bb, const double *a0)
{
    if (degree == 0 || degree > WAFER_FILTER_MAX_DEGREE)
        return fail(WAFER_ERR_INVALID, "degree = %u: wafer_batch_filter_states takes 1 .. %d", degree, WAFER_FILTER_MAX_DEGREE);
    uint32_t max_k = 0;
    TRY(store_step_check(b, active, k, "wafer_batch_filter_states", &max_k));
    for (uint32_t m = 0; m < b->n; ++m)
        if ((!active || active[m]) && k[m] && !wafer_filter_interval_ok(a[m], bb[m], a0[m]))
            return fail(WAFER_ERR_INVALID, "member %u: the interval needs finite a0 < a < b (a0 = %g, a = %g, b = %g)", m, a0[m], a[m], bb[m]);
    const auto alloc = [&]() -> int {
        if (!b->filt_coef.dev) BUF_TRY(b->filt_coef.make((size_t)WAFER_FILTER_MAX_DEGREE * b->n));
        return WAFER_OK;
    };
    const auto upload = [&](const uint8_t *listed) -> int {
        std::vector<double> al(degree), be(degree);
        for (uint32_t m = 0; m < b->n; ++m) {
            double cc = 0.0;
            if (listed[m]) (void)wafer_filter_coefficients_host(degree, a[m], bb[m], a0[m], al.data(), be.data(), &cc);   // (checked above)
            for (uint32_t i = 0; i < degree; ++i) b->filt_coef[(size_t)i * b->n + m] = listed[m] ? WaferFilterCoef{al[i], be[i], cc} : WaferFilterCoef{0., 0., 0.};
        }
        BUF_TRY(b->filt_coef.upload((size_t)degree * b->n, b->s));
        return WAFER_OK;
    };
    return store_pass(b, active, k, max_k, "wafer_batch_filter_states", "store filter", degree, b->n_filter_launches, alloc, upload,
                      [&](uint64_t t, const auto &gs, int groups, const WaferRitzPtrs &src, const WaferRitzPtrs &dst) {
                          return wafer_entry_batch_store_filter(b->f32, b->g().R, gs, b->mem_dev, b->blks.dev, (int)b->blks.host.size(), groups, b->store_k.dev,
                                                                b->filt_coef.dev + t * b->n, t == 0 ? 1 : 0, src, dst, b->s);
                      });
}

// ub[m] = W_R / den + max V over member m's work cells, for every listed member: one launch, one read-back
int spectral_bound(wafer_batch *b, const uint8_t *active, double *ub)
{
    int nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (!b->views[m]->have_pot) return fail(WAFER_ERR_STATE, "member %u: potential not set", m);
        ++nlisted;
    }
    if (!nlisted) return WAFER_OK;
    HIP_TRY(hipSetDevice(b->device));
    if (!b->vmax.dev) BUF_TRY(b->vmax.make(b->n));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, active, &nact));   // (synchronises the stream: vmax's host side is not read by an earlier call's copy either)
    for (int q = 0; q < nact; ++q) b->vmax[q] = 0;   // below every key
    BUF_TRY(b->vmax.upload((size_t)nact, b->s));
    int max_tiles, max_planes;
    max_tiles_planes(b, nact, false, &max_tiles, &max_planes);
    TRY(launch(b, "spectral bound", [&](const auto &gs) {
        return wafer_entry_batch_v_max(b->f32, gs, b->mem_dev, b->act.dev, nact, max_tiles, max_planes, b->vmax.dev, b->s);
    }));
    ++b->n_bound_launches;
    BUF_TRY(b->vmax.download((size_t)nact, b->s));
    HIP_TRY(hipStreamSynchronize(b->s));
    for (int q = 0; q < nact; ++q) {
        const uint32_t m = (uint32_t)b->act[q];
        const wafer_params &P = b->P[m];
        ub[m] = wafer_stencil_abs_weight(P.central_difference) / wafer_stencil_den(P.central_difference, P.dn, P.mass) + wafer_order_value(b->vmax[q]);
    }
    return WAFER_OK;
}

} // namespace

extern "C" {

int wafer_batch_ritz_matrices(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *h, double *s)
{
    if (!b || !k || !h || !s) return fail(WAFER_ERR_INVALID, "null argument");
    int nlisted = 0;
    TRY(ritz_check(b, active, k, true, "wafer_batch_ritz_matrices", &nlisted));
    if (!nlisted) return WAFER_OK;
    TRY(ritz_matrices_impl(b, active, k));
    for (uint32_t m = 0; m < b->n; ++m)
        if (!active || active[m]) ritz_unpack(b, m, k[m], h + m * RITZ_KK, s + m * RITZ_KK);
    return WAFER_OK;
}

int wafer_batch_rotate_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, const double *coef)
{
    if (!b || !k || !coef) return fail(WAFER_ERR_INVALID, "null argument");
    int nlisted = 0;
    TRY(ritz_check(b, active, k, false, "wafer_batch_rotate_states", &nlisted));
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        for (uint32_t q = 0; q < k[m] * k[m]; ++q)
            if (!std::isfinite(coef[m * RITZ_KK + q])) return fail(WAFER_ERR_INVALID, "member %u: coef[%u] is not finite", m, q);
    }
    if (!nlisted) return WAFER_OK;
    return ritz_rotate_impl(b, active, k, coef);
}

int wafer_batch_ritz(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *evals, double *coef, double *h, double *s, int *status)
{
    if (!b || !k || !evals || !coef || !status) return fail(WAFER_ERR_INVALID, "null argument");
    int nlisted = 0;
    TRY(ritz_check(b, active, k, true, "wafer_batch_ritz", &nlisted));
    if (!nlisted) return WAFER_OK;
    TRY(ritz_matrices_impl(b, active, k));
    // the solves: a member whose solve fails keeps its store and its evals / coef entries; that is its status, not the call's
    std::vector<uint8_t> solved(b->n, 0);
    std::vector<double> ev((size_t)WAFER_RITZ_MAX * b->n), cf(RITZ_KK * b->n, 0.0);
    std::string first_failure;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        double hm[RITZ_KK], sm[RITZ_KK];
        ritz_unpack(b, m, k[m], hm, sm);
        const int rc = wafer_ritz_solve_host((int)k[m], hm, sm, ev.data() + (size_t)m * WAFER_RITZ_MAX, cf.data() + m * RITZ_KK);
        solved[m] = rc == WAFER_RITZ_OK;
        if (!solved[m] && first_failure.empty()) {
            char msg[224];
            if (rc == WAFER_RITZ_NO_CONVERGENCE)
                snprintf(msg, sizeof msg, "member %u: Rayleigh-Ritz: the Jacobi iteration did not converge in %d sweeps", m, (int)WAFER_RITZ_SWEEPS);
            else
                snprintf(msg, sizeof msg, "member %u: Rayleigh-Ritz: the overlap matrix is not positive definite (linearly dependent states, "
                                          "or a non-finite sum)", m);
            first_failure = msg;
        }
    }
    TRY(ritz_rotate_impl(b, solved.data(), k, cf.data()));
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        ritz_unpack(b, m, k[m], h ? h + m * RITZ_KK : nullptr, s ? s + m * RITZ_KK : nullptr);
        status[m] = solved[m] ? WAFER_OK : WAFER_ERR_STATE;
        if (!solved[m]) continue;
        for (size_t q = 0; q < (size_t)k[m] * k[m]; ++q) coef[m * RITZ_KK + q] = cf[m * RITZ_KK + q];
        for (uint32_t q = 0; q < k[m]; ++q) evals[(size_t)m * WAFER_RITZ_MAX + q] = ev[(size_t)m * WAFER_RITZ_MAX + q];
    }
    if (!first_failure.empty()) (void)fail(WAFER_ERR_STATE, "%s", first_failure.c_str());   // wafer_last_error names the first failed member
    return WAFER_OK;
}

int wafer_batch_diag_ritz_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks)
{
    if (!b || !launches || !readbacks) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_ritz_launches;
    *readbacks = b->n_ritz_readbacks;
    return WAFER_OK;
}

int wafer_batch_residuals(wafer_batch *b, int source, const uint8_t *active, const uint32_t *k, const double *theta_in, double *theta, double *r2,
                          double *s, int *status)
{
    if (!b || !k || !theta || !r2 || !s || !status) return fail(WAFER_ERR_INVALID, "null argument");
    int nlisted = 0;
    TRY(residual_check(b, source, active, k, theta_in, &nlisted));
    if (!nlisted) return WAFER_OK;
    HIP_TRY(hipSetDevice(b->device));
    RoctxRange range_("wafer_batch_residuals");
    TRY(ensure_residual(b));
    TRY(sync_members(b));
    std::vector<uint8_t> ok(b->n, 0);
    for (uint32_t m = 0; m < b->n; ++m) ok[m] = (!active || active[m]) ? 1 : 0;
    std::vector<double> th((size_t)WAFER_RITZ_MAX * b->n, 0.0);
    std::string first_failure;
    if (theta_in) {
        for (uint32_t m = 0; m < b->n; ++m)
            for (uint32_t j = 0; ok[m] && j < k[m]; ++j) th[(size_t)m * WAFER_RITZ_MAX + j] = theta_in[(size_t)m * WAFER_RITZ_MAX + j];
    } else {   // Rayleigh mode: theta_j = wh_j / s_j of a pass with theta = 0; a member without a quotient keeps its outputs: its status
        TRY(residual_pass(b, source, ok.data(), k, nullptr));
        bool any = false;
        for (uint32_t m = 0; m < b->n; ++m) {
            if (!ok[m]) continue;
            const double *r = &b->resid_sums[m * RESID_ROWS];
            for (uint32_t j = 0; j < k[m]; ++j) {
                const double sj = r[j * 3 + 2];
                if (!std::isfinite(sj) || !(sj > 0.0)) {
                    if (first_failure.empty()) {
                        char msg[192];
                        snprintf(msg, sizeof msg, "member %u: state %u: <l|l> = %g: no Rayleigh quotient (a zero or non-finite state)", m, j, sj);
                        first_failure = msg;
                    }
                    ok[m] = 0;
                    status[m] = WAFER_ERR_STATE;
                    break;
                }
                th[(size_t)m * WAFER_RITZ_MAX + j] = r[j * 3 + 1] / sj;
            }
            any = any || ok[m];
        }
        if (!any) {   // nobody left for the second pass
            (void)fail(WAFER_ERR_STATE, "%s", first_failure.c_str());
            return WAFER_OK;
        }
    }
    TRY(residual_pass(b, source, ok.data(), k, th.data()));
    for (uint32_t m = 0; m < b->n; ++m) {
        if (!ok[m]) continue;
        const double *r = &b->resid_sums[m * RESID_ROWS];
        for (uint32_t j = 0; j < k[m]; ++j) {
            theta[(size_t)m * WAFER_RITZ_MAX + j] = th[(size_t)m * WAFER_RITZ_MAX + j];
            r2[(size_t)m * WAFER_RITZ_MAX + j] = r[j * 3 + 0];
            s[(size_t)m * WAFER_RITZ_MAX + j] = r[j * 3 + 2];
        }
        status[m] = WAFER_OK;
    }
    if (!first_failure.empty()) (void)fail(WAFER_ERR_STATE, "%s", first_failure.c_str());   // wafer_last_error names the first such member
    return WAFER_OK;
}

int wafer_batch_diag_residual_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks)
{
    if (!b || !launches || !readbacks) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_resid_launches;
    *readbacks = b->n_resid_readbacks;
    return WAFER_OK;
}

int wafer_batch_moment_matrices(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *m)
{
    if (!b || !k || !m) return fail(WAFER_ERR_INVALID, "null argument");
    int nlisted = 0;
    TRY(moment_check(b, active, k, &nlisted));
    if (!nlisted) return WAFER_OK;
    TRY(moment_pass(b, active, k));
    // the entries i > j are copies of their mirror images: l * w commutes, so the copy is exact
    for (uint32_t mb = 0; mb < b->n; ++mb) {
        if (active && !active[mb]) continue;
        const size_t kk = k[mb], tri = (size_t)wafer_moment_tri((int)kk);
        const double *r = &b->moment_sums[mb * MOMENT_ROWS];
        for (size_t q = 0; q < WAFER_MOMENT_COUNT; ++q) {
            double *out = m + (mb * WAFER_MOMENT_COUNT + q) * RITZ_KK;
            for (size_t j = 0; j < kk; ++j)
                for (size_t i = 0; i <= j; ++i) out[j * kk + i] = out[i * kk + j] = r[q * tri + (size_t)wafer_moment_tri((int)j) + i];
        }
    }
    return WAFER_OK;
}

int wafer_batch_diag_moment_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks)
{
    if (!b || !launches || !readbacks) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_moment_launches;
    *readbacks = b->n_moment_readbacks;
    return WAFER_OK;
}

int wafer_batch_evolve_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint64_t n_steps)
{
    if (!b || !k) return fail(WAFER_ERR_INVALID, "null argument");
    return evolve_states(b, active, k, n_steps);
}

int wafer_batch_filter_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint32_t degree, const double *a, const double *bb,
                              const double *a0)
{
    if (!b || !k || !a || !bb || !a0) return fail(WAFER_ERR_INVALID, "null argument");
    return filter_states(b, active, k, degree, a, bb, a0);
}

int wafer_batch_spectral_bound(wafer_batch *b, const uint8_t *active, double *ub)
{
    if (!b || !ub) return fail(WAFER_ERR_INVALID, "null argument");
    return spectral_bound(b, active, ub);
}

int wafer_batch_diag_filter_counts(wafer_batch *b, uint64_t *launches, uint64_t *bound_launches)
{
    if (!b || !launches || !bound_launches) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_filter_launches;
    *bound_launches = b->n_bound_launches;
    return WAFER_OK;
}

int wafer_batch_diag_store_step(wafer_batch *b, char *buf, size_t n)
{
    if (!b || !buf || n == 0) return fail(WAFER_ERR_INVALID, "null argument");
    snprintf(buf, n, "kernel=wafer_k_batch_store_step<%d,%s,%s> states_per_workgroup=%d shapes=%zu", b->g().R, KERNEL_TYPES[b->dtype],
             b->mixed ? "WaferBatchGeomTable" : "WaferGeom", WAFER_STORE_SG, b->geoms.size());
    return WAFER_OK;
}

int wafer_batch_diag_store_counts(wafer_batch *b, uint64_t *launches)
{
    if (!b || !launches) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_store_launches;
    return WAFER_OK;
}

} // extern "C"

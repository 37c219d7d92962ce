// wafer_engine_batch.hip -- batched ensembles (wafer_batch_*, include/wafer_hip.h): B problems on one device, one launch per step over
// the active members -- or, for ground-state steps, one launch per pass of K steps (wafer_batch_plan.h) -- (kernels:
// wafer_stencil_batch.hip.h), and for excited states a per-member state store with the normalise / Gram-Schmidt tail of every step
// (wafer_gs_batch.hip.h, wafer_tu_gs_batch.hip): 1 + 2 (1 + wnum) + 1 launches per step for the whole batch -- or, where
// wafer_batch_set_gs_variant selects the one-pass form (wnum <= WAFER_MAX_LOW), 4: step, raw sums, reduce, one apply pass with the
// member's Gram matrix.
//
// Each member is also a context VIEW: a wafer_ctx whose arrays are the member's slices of the batch's allocations and whose
// stream is the batch's.  Potentials, initial conditions, uploads and downloads go through the context entry points on that
// view, so a member is set up by the very code that sets up a single context.  The views own nothing but the a, b arrays that
// wafer_batch_download_array may have made (ensure_ab), which go back with the batch.
// Set-up of many members at once (set_potentials, set_initial_conditions: wafer_setup_batch.hip.h) writes the same cells with the same
// per-cell functions in one launch for all listed members, and every batched writer of V -- those and resample -- ends in ONE range
// check for all listed members (check_v_listed) instead of a context's check_v_range per member.
//
// One dtype per batch (member 0's): f64, f32 (float arrays, fp64 arithmetic) or f32fast (float arrays, float arithmetic in the
// ground-state step).  Every array and store slot is allocated in the element size `esz`, the geometry is the one a context of
// that dtype builds (wafer_make_geom with that element size: the context's set-up kernels run on the views), and the entry
// points of the kernels take the dtype.
//
// Shapes and layout (wafer_batch_layout, wafer_batch_plan.h).  The batch keeps a table of its distinct geometries (`geoms`, each the
// one wafer_ctx_create builds for that shape; on the device too) and every member an index into it (`shape_of`).  Storage is one
// allocation per array kind, member m at element offset off[m] = the sum of the totals of the members before it, every member
// with its own guard rows and planes.  The step tables are built over all active members at once (wafer_batch_plan.h) and every
// entry carries its member's shape index, so a step or a fused pass is ONE launch whatever the shapes.  Every other kernel runs on
// a grid of (workgroup, member) as wide as the largest launched member needs and takes what depends on the member -- its partition,
// its workgroup count, the places of its partials, its origin in a store slot -- from its WaferBatchMember record (init_partitions).
// A batch of one shape (wafer_batch_create, or wafer_batch_create_mixed with equal shapes) is the case geoms.size() == 1 of all this:
// off[m] == m * geoms[0].total, every member's partition is the same, and the widest is everyone's.  The one thing that differs is
// where the kernels read the geometry from (with_geom, the one place that chooses): a kernel argument for one shape, the device
// table for several -- the same kernel templates instantiated for either source (wafer_tu_batch.inc, wafer_tu_gs_batch.inc).
// State stores: a slot is one allocation laid out as the arrays are, and every member's Gram-Schmidt partition and the places of
// its partials come from wafer_batch_gs_partition (wafer_batch_plan.h; `gsp`, and in its WaferBatchMember).  On several shapes they
// are opt-in at creation (wafer_batch_create_mixed_states: `mixed_states`); a batch of several shapes made by
// wafer_batch_create_mixed refuses the excited-state calls as it always has (refuse_mixed).
// The calls on the state stores beyond Gram-Schmidt -- Rayleigh-Ritz, residuals, stepping and filtering the stores, the spectral
// bound -- are wafer_engine_batch_stores.hip; what the two units share is wafer_engine_batch.h.
#include <memory>
#include "wafer_engine_batch.h"
#include "wafer_stencil_lds.hip.h"
#include "wafer_gs_batch.hip.h"
#include "wafer_resample_batch.hip.h"

namespace wafer_eng __attribute__((visibility("hidden"))) {

int check_member_index(const wafer_batch *b, uint32_t m)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    if (m >= b->n) return fail(WAFER_ERR_INVALID, "member %u out of range (the batch has %u)", m, b->n);
    return WAFER_OK;
}

// the calls that need the state stores: not on a batch of several shapes; nothing has changed when this returns
int refuse_mixed(const wafer_batch *b, const char *call)
{
    if (!b->mixed || b->mixed_states) return WAFER_OK;
    return fail(WAFER_ERR_INVALID, "%s: not available on a mixed-shape batch (%zu distinct shapes): excited states need one shape per batch",
                call, b->geoms.size());
}

// the member table as the views stand now (potential range, pot_sub, current buffer), to the device if it changed
int sync_members(wafer_batch *b)
{
    bool changed = false;
    for (uint32_t m = 0; m < b->n; ++m) {
        const wafer_ctx *c = b->views[m];
        WaferBatchMember e = b->mem[m];
        e.short_forms = short_forms(c) ? 1 : 0;
        e.potsub_kind = c->potsub_kind;
        e.potsub_scalar = c->potsub_scalar;
        e.cur = c->cur;
        if (memcmp(&e, &b->mem[m], sizeof e) != 0) {
            b->mem[m] = e;
            changed = true;
        }
    }
    if (!changed) return WAFER_OK;
    HIP_TRY(hipStreamSynchronize(b->s));   // no launch in flight reads the table
    HIP_TRY(hipMemcpy(b->mem_dev, b->mem.data(), b->mem_dev.bytes(), hipMemcpyHostToDevice));
    return WAFER_OK;
}

// the active members' slots into act, host and device; returns their number
int upload_active(wafer_batch *b, const uint8_t *active, int *nact)
{
    HIP_TRY(hipStreamSynchronize(b->s));   // act's host side is read by a copy of an earlier call
    int k = 0;
    for (uint32_t m = 0; m < b->n; ++m)
        if (!active || active[m]) b->act[k++] = (int)m;
    *nact = k;
    if (k) BUF_TRY(b->act.upload(k, b->s));
    return WAFER_OK;
}

// A workgroup table on the device for this active set: the one-step kernel's (K == 1: wafer_batch_step_table) or the fused pass's
// (wafer_batch_fused_table, wafer_batch_plan.h).  Kept while the active set and K stay; an empty one too.
int build_blocks(wafer_batch *b, wafer_batch::BlockTable &t, const uint8_t *active, int K)
{
    std::vector<uint8_t> key(b->n);
    for (uint32_t m = 0; m < b->n; ++m) key[m] = (!active || active[m]) ? 1 : 0;
    if (key == t.key && K == t.K && t.dev) return WAFER_OK;
    t.host = K > 1 ? wafer_batch_fused_table(b->geoms.data(), b->shape_of.data(), key.data(), b->n, b->num_cus, K, WAFER_BATCHK_TX, WAFER_BATCHK_TY)
                   : wafer_batch_step_table(b->geoms.data(), b->shape_of.data(), key.data(), b->n, b->num_cus, WAFER_BATCH_TX, WAFER_BATCH_TY);
    HIP_TRY(hipStreamSynchronize(b->s));
    BUF_TRY(t.dev.reserve(std::max<size_t>(t.host.size(), 1)));
    if (!t.host.empty()) HIP_TRY(hipMemcpy(t.dev, t.host.data(), sizeof(WaferBatchBlock) * t.host.size(), hipMemcpyHostToDevice));
    t.key = key;
    t.K = K;
    return WAFER_OK;
}

// a launch's status as the call's: `what` names the kernel in the message
int launched(const char *what, hipError_t e)
{
    return e == hipSuccess ? WAFER_OK : fail(WAFER_ERR_HIP, "batched %s launch failed: %s", what, hipGetErrorString(e));
}

// The grid of the kernels that run one 64 x 4 tile of one plane per workgroup (normalise, symmetrise, resample): the largest tile
// and plane counts among the members in act -- of their work boxes, or (padded) of their padded boxes, frame and ghost planes
// included.
void max_tiles_planes(const wafer_batch *b, int nact, bool padded, int *max_tiles, int *max_planes)
{
    *max_tiles = *max_planes = 0;
    for (int k = 0; k < nact; ++k) {
        const WaferGeom &g = b->geom((uint32_t)b->act[k]);
        const int x = padded ? g.px : g.nx, y = padded ? g.py : g.ny;
        *max_tiles = std::max(*max_tiles, ((x + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX) * ((y + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY));
        *max_planes = std::max(*max_planes, padded ? g.lz : g.nzl);
    }
}

// member m's state l as a logical pointer (plane 0, row 0), like the views' arrays
void *slot_ptr(const wafer_batch *b, uint32_t l, uint32_t m)
{
    return b->slots[l] + (b->off[m] + (size_t)b->geom(m).base_off) * b->esz;
}

// entries [0, n) of `v` exist (zeros: frames, pads and guard zones of every member).  v: the store's slots, or their shadows
// (wafer_batch_evolve_states), laid out alike
int ensure_slots(wafer_batch *b, std::vector<DevArray<char>> &v, uint32_t n)
{
    while (v.size() < n) {
        DevArray<char> p;
        BUF_TRY(p.make(b->cells * b->esz));
        v.push_back(std::move(p));
        HIP_TRY(hipMemsetAsync(v.back(), 0, v.back().bytes(), b->s));
    }
    return WAFER_OK;
}

// member m's store changed: its Gram matrix (the one-pass form's, if it exists) is recomputed before the next one-pass call
void mark_gram_stale(wafer_batch *b, uint32_t m)
{
    if (!b->gram_stale.empty()) b->gram_stale[m] = 1;
}

} // namespace wafer_eng

namespace {

int check_member(const wafer_params *m, uint32_t i, const wafer_params *m0, bool same_shape = true)
{
    if (m->struct_size != sizeof(wafer_params))
        return fail(WAFER_ERR_INVALID, "member %u: wafer_params.struct_size %u != %zu (ABI mismatch)", i, m->struct_size, sizeof(wafer_params));
    if (m->nx < 1 || m->ny < 1 || m->nz < 1) return fail(WAFER_ERR_INVALID, "member %u: grid size must be >= 1", i);
    if (m->central_difference < 1 || m->central_difference > 3)
        return fail(WAFER_ERR_INVALID, "member %u: central_difference must be 1 (Three), 2 (Five) or 3 (SevenPoint)", i);
    if (m->dtype != WAFER_F64 && m->dtype != WAFER_F32 && m->dtype != WAFER_F32_FAST)
        return fail(WAFER_ERR_INVALID, "member %u: bad dtype %d (f64 = 0, f32 = 1, f32fast = 2)", i, (int)m->dtype);
    if (m->z_count != 0) return fail(WAFER_ERR_INVALID, "member %u: z_count must be 0 (a batch holds no z-slabs)", i);
    if (!(m->dn > 0) || !(m->dt > 0) || !(m->mass > 0)) return fail(WAFER_ERR_INVALID, "member %u: dn, dt, mass must be > 0", i);
    const double den = wafer_stencil_den(m->central_difference, m->dn, m->mass);
    if (!std::isnormal(den) || !std::isnormal(1.0 / den))
        return fail(WAFER_ERR_INVALID, "member %u: dn^2 * mass = %g is outside the range of normal doubles (or its reciprocal is)", i,
                    m->dn * m->dn * m->mass);
    if (!(m->flags & WAFER_FLAG_SKIP_DT_CHECK) && m->dt > m->dn * m->dn / 3.)   // config.rs:362-365
        return fail(WAFER_ERR_INVALID, "member %u: LargeDt: dt must be <= dn^2/3 (config.rs:363)", i);
    if (m->halo_depth != 0 && (int)m->halo_depth < m->central_difference)
        return fail(WAFER_ERR_INVALID, "member %u: halo_depth must be >= ext", i);
    if (m0) {
        if (m->dtype != m0->dtype)
            return fail(WAFER_ERR_INVALID, "member %u: dtype = %d differs from member 0's %d (a batch holds one dtype)", i, (int)m->dtype, (int)m0->dtype);
        if (same_shape) {   // (wafer_batch_create_mixed: every member its own)
            if (m->nx != m0->nx) return fail(WAFER_ERR_INVALID, "member %u: nx = %u differs from member 0's %u", i, m->nx, m0->nx);
            if (m->ny != m0->ny) return fail(WAFER_ERR_INVALID, "member %u: ny = %u differs from member 0's %u", i, m->ny, m0->ny);
            if (m->nz != m0->nz) return fail(WAFER_ERR_INVALID, "member %u: nz = %u differs from member 0's %u", i, m->nz, m0->nz);
        }
        if (m->central_difference != m0->central_difference)
            return fail(WAFER_ERR_INVALID, "member %u: central_difference = %d differs from member 0's %d", i, m->central_difference,
                        m0->central_difference);
        if (m->device != m0->device) return fail(WAFER_ERR_INVALID, "member %u: device = %d differs from member 0's %d", i, m->device, m0->device);
        if (m->halo_depth != m0->halo_depth)   // (the batch's one geometry is built with it)
            return fail(WAFER_ERR_INVALID, "member %u: halo_depth = %u differs from member 0's %u", i, m->halo_depth, m0->halo_depth);
    }
    return WAFER_OK;
}

// every active member has phi (and, with need_pot, a potential: `what` ends that message) and at least wnum stored states
int check_ready(const wafer_batch *b, const uint8_t *active, bool need_pot, const char *what, uint32_t wnum)
{
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        const wafer_ctx *c = b->views[m];
        if (need_pot && (!c->have_pot || !c->have_phi)) return fail(WAFER_ERR_STATE, "member %u: potential and phi must be set%s", m, what);
        if (!c->have_phi) return fail(WAFER_ERR_STATE, "member %u: phi not set", m);
        if (wnum > b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: wnum %u but w_store holds %u states", m, wnum, b->nst[m]);
    }
    return WAFER_OK;
}

// Steps per launch of a ground-state evolve: the fused pass where an instantiation exists and the variant asks for it.
// The default (-1), per stencil (index R), follows the measured rows of DESIGN.md section 5 "Batches".
constexpr bool WAFER_BATCH_FUSED_BY_DEFAULT[4] = {false, false, false, false};
int steps_per_pass(const wafer_batch *b)
{
    const int R = b->g().R;
    const int K = R == 1 ? 3 : 2;
    const bool fused = b->step_variant < 0 ? WAFER_BATCH_FUSED_BY_DEFAULT[R] : b->step_variant == 1;
    if (!fused || wafer_batch_stepk_lds_bytes(b->dtype, R, K) == 0) return 1;
    return K;
}

// a call's remainder of two steps is one pass where the two-step instantiation exists beside the K-step one
bool have_two_step(const wafer_batch *b, int K) { return K > 2 && wafer_batch_stepk_lds_bytes(b->dtype, b->g().R, 2) != 0; }

// the four raw sums of the active members into sums[m * 4 ..] on the host
int observables(wafer_batch *b, const uint8_t *active)
{
    HIP_TRY(hipSetDevice(b->device));
    TRY(check_ready(b, active, true, "", 0));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    if (!nact) return WAFER_OK;
    RoctxRange range_("wafer_batch_observables");
    int max_nb = 0;   // the grid is as wide as the largest launched member's partition
    for (int k = 0; k < nact; ++k) max_nb = std::max(max_nb, b->mem[b->act[k]].obs_nb);
    TRY(launch(b, "observables", [&](const auto &gs) {
        return wafer_entry_batch_observables(b->f32, b->g().R, gs, b->mem_dev, b->act.dev, nact, max_nb, b->swz, b->partials, b->sums.dev, b->s);
    }));
    BUF_TRY(b->sums.download(b->sums.host.size(), b->s));
    HIP_TRY(hipStreamSynchronize(b->s));
    return WAFER_OK;
}

void obs_of(const wafer_batch *b, uint32_t m, wafer_observables_t *o)
{
    const double *r = &b->sums[(size_t)m * 4];
    o->energy = r[0];
    o->norm2 = r[1];
    o->v_infinity = (b->views[m]->potsub_kind == WAFER_POTSUB_NONE) ? 0.0 : r[2];   // grid.rs:425
    o->r2 = r[3];
}

// normalise the active members; norm2 on the device, member m's at norm2_dev[m * stride]
int normalise(wafer_batch *b, const uint8_t *active, const double *norm2_dev, int stride)
{
    HIP_TRY(hipSetDevice(b->device));
    TRY(check_ready(b, active, false, "", 0));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    if (!nact) return WAFER_OK;
    int max_tiles, max_planes;
    max_tiles_planes(b, nact, false, &max_tiles, &max_planes);
    return launch(b, "normalise", [&](const auto &gs) {
        return wafer_entry_batch_normalise(b->f32, gs, b->mem_dev, b->act.dev, nact, max_tiles, max_planes, norm2_dev, stride, b->s);
    });
}

// config::symmetrise_wavefunction (config.rs:691-728) for every active member with a constraint, each with its own: the checks and
// the message of wafer_symmetrise, then ONE launch from phi[cur] into the members' other buffers, whose views flip.  Needs no state
// store: one shape or several.
int symmetrise(wafer_batch *b, const uint8_t *active, const int *constraints)
{
    std::vector<uint8_t> hit(b->n, 0);
    bool any = false;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (constraints[m] < WAFER_SYM_NOT_CONSTRAINED || constraints[m] > WAFER_SYM_ANTISYM_ABOUT_Y)
            return fail(WAFER_ERR_INVALID, "member %u: unknown symmetry constraint %d", m, constraints[m]);
        if (!b->views[m]->have_phi) return fail(WAFER_ERR_STATE, "member %u: phi not set", m);
        hit[m] = constraints[m] != WAFER_SYM_NOT_CONSTRAINED;
        any = any || hit[m];
    }
    if (!any) return WAFER_OK;
    if (b->g().R != 3)
        return fail(WAFER_ERR_INVALID, "symmetry constraints index the SevenPoint frame (config.rs:702-725); "
                                       "the reference runs out of bounds with central_difference ext %d", b->g().R);
    HIP_TRY(hipSetDevice(b->device));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, hit.data(), &nact));   // (synchronises the stream: sym's host side is not read by an earlier call's copy either)
    for (uint32_t m = 0; m < b->n; ++m) b->sym[m] = hit[m] ? constraints[m] : 0;
    BUF_TRY(b->sym.upload(b->n, b->s));
    int max_tiles, max_planes;   // of the padded boxes: the kernel writes the frame's zeros too
    max_tiles_planes(b, nact, true, &max_tiles, &max_planes);
    RoctxRange range_("wafer_batch_symmetrise");
    TRY(launch(b, "symmetrise", [&](const auto &gs) {
        return wafer_entry_batch_symmetrise(b->f32, gs, b->mem_dev, b->act.dev, nact, b->sym.dev, max_tiles, max_planes, b->s);
    }));
    for (uint32_t m = 0; m < b->n; ++m) {
        if (!hit[m]) continue;
        b->views[m]->cur ^= 1;
        b->views[m]->halo_valid = 0;
    }
    return sync_members(b);
}

// ---- w_store ---------------------------------------------------------------------------------------------------------------
int check_capacity(const wafer_batch *b, uint32_t m)
{
    if (b->nst[m] >= b->P[m].max_states) return fail(WAFER_ERR_STATE, "member %u: w_store is full (max_states = %u)", m, b->P[m].max_states);
    return WAFER_OK;
}

// phi of the active members to the end of their stores; nothing changes unless every one of them can take it
int push_states(wafer_batch *b, const uint8_t *active)
{
    HIP_TRY(hipSetDevice(b->device));
    uint32_t need = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (!b->views[m]->have_phi) return fail(WAFER_ERR_STATE, "member %u: phi not set", m);
        TRY(check_capacity(b, m));
        need = std::max(need, b->nst[m] + 1);
    }
    TRY(ensure_slots(b, b->slots, need));
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        const wafer_ctx *c = b->views[m];
        HIP_TRY(hipMemcpyAsync(alloc_base(c, slot_ptr(b, b->nst[m], m)), alloc_base(c, c->phi[c->cur]), (size_t)b->geom(m).total * b->esz, hipMemcpyDeviceToDevice, b->s));
        ++b->nst[m];
        mark_gram_stale(b, m);
    }
    return WAFER_OK;
}

// ---- excited states --------------------------------------------------------------------------------------------------------
// Doubles of gs_partials for kernels that write `rows` sums per workgroup (1: the sequential form; WAFER_GS_ONE_ROWS: the one-pass
// form's sums): every member's rows end to end (gsp), or every member's wafer_batch_norm2 partition end to end if that is longer --
// on float storage the two differ (the row walk's and the 64 x 4 x 4 tiles'), each with its own offsets from 0 (n2_off, gs_off),
// written and reduced by different calls in stream order.
size_t partials_doubles(const wafer_batch *b, int rows) { return std::max((size_t)b->gsp.doubles(rows), b->n2_doubles); }

int ensure_gs(wafer_batch *b)
{
    if (b->gs_scal.dev) return WAFER_OK;   // (made last: a call that failed before it starts over, and leaks nothing)
    BUF_TRY(b->gs_partials.reserve(partials_doubles(b, 1)));
    BUF_TRY(b->gs_scal.make((size_t)b->gs_stride * b->n));
    HIP_TRY(hipMemsetAsync(b->gs_scal.dev, 0, b->gs_scal.dev.bytes(), b->s));
    return WAFER_OK;
}

// the grid's extent along x: the largest partition among the members in list (one shape: everyone's)
int gs_max_nb(const wafer_batch *b, const int *list, int n)
{
    int nb = 0;
    for (int k = 0; k < n; ++k) nb = std::max(nb, b->gsp.nb[list[k]]);
    return nb;
}

// one elementwise launch (+ its reduce into slot out_slot) over the members in act; lower, dotwith: store slots, -1 none
int gs_launch(wafer_batch *b, int mode, int nact, int flip, int coef_slot, int lower, int dotwith, int out_slot)
{
    const int max_nb = gs_max_nb(b, b->act.host, nact);
    return launch(b, "Gram-Schmidt", [&](const auto &gs) {
        const WaferBatchGsArgs a{flip, b->gs_stride, coef_slot, lower >= 0 ? b->slots[lower].get() : nullptr, dotwith >= 0 ? b->slots[dotwith].get() : nullptr};
        return wafer_entry_batch_gs(b->f32, mode, gs, a, b->mem_dev, b->act.dev, nact, max_nb, b->gs_scal.dev, out_slot, b->gs_partials, b->s);
    });
}

// ---- the one-pass form ---------------------------------------------------------------------------------------------------------
// the launch path's predicate: which form a call with this wnum takes
bool use_onepass(const wafer_batch *b, uint32_t wnum) { return b->gs_variant == 1 && wnum >= 1 && wnum <= WAFER_MAX_LOW; }

// gs_partials grown to the sums kernel's rows, and the Gram storage; every member's matrix is stale
int ensure_onepass(wafer_batch *b)
{
    if (b->onepass_ready) return WAFER_OK;
    TRY(ensure_gs(b));
    HIP_TRY(hipStreamSynchronize(b->s));   // no launch in flight writes the partials that go back
    // (reserve makes the new buffer first: a failed allocation leaves the sequential form's partials in place)
    BUF_TRY(b->gs_partials.reserve(partials_doubles(b, WAFER_GS_ONE_ROWS)));
    BUF_TRY(b->gram.make((size_t)WAFER_MAX_LOW * WAFER_MAX_LOW * b->n));
    HIP_TRY(hipMemsetAsync(b->gram, 0, b->gram.bytes(), b->s));
    BUF_TRY(b->gram_partials.make((size_t)b->gsp.doubles(WAFER_GRAM_PAIRS)));
    BUF_TRY(b->gram_list.make(2 * (size_t)b->n));
    b->gram_stale.assign(b->n, 1);
    b->onepass_ready = true;
    return WAFER_OK;
}

// the one-pass kernels' arguments: the allocations of store slots [0, nslots)
WaferBatchGsOneArgs onepass_args(const wafer_batch *b, int flip, uint32_t nslots)
{
    WaferBatchGsOneArgs a;
    a.flip = flip;
    a.scal_stride = b->gs_stride;
    for (uint32_t l = 0; l < WAFER_MAX_LOW; ++l) a.low[l] = l < nslots ? b->slots[l].get() : nullptr;
    return a;
}

// the Gram matrices of the active members whose stores changed since they were formed: one launch and its reduce, in stream
// order behind the copies that changed the stores.  (Called once per call, before its first step, after upload_active's
// synchronisation: gram_list's host side is not read by an earlier call's copy any more.)
int refresh_gram(wafer_batch *b, const uint8_t *active)
{
    int nlist = 0, nl = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if ((active && !active[m]) || !b->gram_stale[m]) continue;
        b->gram_stale[m] = 0;
        const int cnt = (int)std::min<uint32_t>(b->nst[m], WAFER_MAX_LOW);
        if (cnt < 2) continue;   // no pair
        b->gram_list[nlist++] = (int)m;
        nl = std::max(nl, cnt);
    }
    if (!nlist) return WAFER_OK;
    for (int k = 0; k < nlist; ++k) b->gram_list[nlist + k] = (int)std::min<uint32_t>(b->nst[b->gram_list[k]], WAFER_MAX_LOW);
    BUF_TRY(b->gram_list.upload(2 * (size_t)nlist, b->s));
    const int max_nb = gs_max_nb(b, b->gram_list.host, nlist);
    return launch(b, "Gram matrix", [&](const auto &gs) {
        return wafer_entry_batch_gram(b->f32, nl, gs, onepass_args(b, 0, (uint32_t)nl), b->mem_dev, b->gram_list.dev, b->gram_list.dev + nlist, nlist,
                                      max_nb, b->gram, b->gram_partials, b->s);
    });
}

// sums, reduce, apply on phi[cur ^ flip] of the members in act: the step's tail (normalise_first) or orthogonalise alone
int gs_onepass(wafer_batch *b, int nact, int flip, uint32_t wnum, bool normalise_first)
{
    const int max_nb = gs_max_nb(b, b->act.host, nact);
    return launch(b, "one-pass Gram-Schmidt", [&](const auto &gs) {
        return wafer_entry_batch_gs_onepass(b->f32, (int)wnum, normalise_first, gs, onepass_args(b, flip, wnum), b->mem_dev, b->act.dev, nact, max_nb,
                                            b->gs_scal.dev, b->gram, b->gs_partials, b->s);
    });
}

// grid.rs:679-680 (normalise: norm2 and the scaling first) and :477-492 on phi[cur ^ flip] of the members in act
int gs_chain(wafer_batch *b, int nact, int flip, uint32_t wnum, bool normalise_first)
{
    if (normalise_first) {
        TRY(gs_launch(b, WAFER_GS_NORM2, nact, flip, 0, -1, -1, 0));
        TRY(gs_launch(b, WAFER_GS_SCALE, nact, flip, 0, -1, wnum ? 0 : -1, 1));
    } else if (wnum) {
        TRY(gs_launch(b, WAFER_GS_DOT, nact, flip, 0, -1, 0, 1));
    }
    for (uint32_t l = 0; l < wnum; ++l)
        TRY(gs_launch(b, WAFER_GS_AXPY, nact, flip, 1 + (int)l, (int)l, l + 1 < wnum ? (int)l + 1 : -1, 2 + (int)l));
    return WAFER_OK;
}

// n_steps steps of the active members, each followed by the normalise / Gram-Schmidt chain when wnum > 0 (grid.rs:544-687).
// wnum == 0: the call's pass sequence (wafer_batch_plan.h) -- passes of K steps, then the remainder; the source buffer flips
// once per launch.
int evolve_state(wafer_batch *b, const uint8_t *active, uint32_t wnum, uint64_t n_steps)
{
    if (wnum) TRY(refuse_mixed(b, "wafer_batch_evolve_state"));
    HIP_TRY(hipSetDevice(b->device));
    TRY(check_ready(b, active, true, " before evolve", 0));
    if (wnum) TRY(check_ready(b, active, false, "", wnum));
    const uint64_t steps = n_steps == 0 ? 1 : n_steps;   // grid.rs:682-685
    if (wnum) TRY(ensure_gs(b));
    const bool onepass = use_onepass(b, wnum);
    if (onepass) TRY(ensure_onepass(b));
    TRY(sync_members(b));
    TRY(build_blocks(b, b->blk, active, 1));
    const int K = wnum ? 1 : steps_per_pass(b);
    // excited steps compute in fp64 on every dtype, as a context's do: an f32fast batch takes the f32 step there
    const int step_dtype = (wnum && b->dtype == WAFER_F32_FAST) ? (int)WAFER_F32 : b->dtype;
    const bool have2 = have_two_step(b, K);
    if (K > 1) TRY(build_blocks(b, b->blkk, active, K));
    int nact = 0;
    if (wnum) TRY(upload_active(b, active, &nact));   // (the chain's member list; synchronises the stream, which a ground-state call must not)
    if (onepass && nact) TRY(refresh_gram(b, active));
    RoctxRange range_(wnum ? "wafer_batch_evolve_state" : "wafer_batch_evolve");
    HIP_TRY(hipEventRecord(b->ev_start, b->s));
    uint64_t launches = 0;
    if (!b->blk.host.empty()) {   // (no active member: no workgroup)
        uint64_t left = steps;
        while (left > 0) {   // no host synchronisation in here: every scalar stays on the device
            const int k = wafer_batch_next_pass(left, K, have2);
            const int flip = (int)(launches & 1);
            TRY(launch(b, "step", [&](const auto &gs) {
                return k > 1 ? wafer_entry_batch_stepk(step_dtype, b->g().R, k, gs, b->mem_dev, b->blkk.dev, (int)b->blkk.host.size(), flip, b->s)
                             : wafer_entry_batch_step(step_dtype, b->g().R, gs, b->mem_dev, b->blk.dev, (int)b->blk.host.size(), flip, b->s);
            }));
            ++launches;
            ++(k > 1 ? b->n_fused_passes : b->n_single_steps);
            left -= (uint64_t)k;
            if (onepass) TRY(gs_onepass(b, nact, (int)(launches & 1), wnum, true));
            else if (wnum) TRY(gs_chain(b, nact, (int)(launches & 1), wnum, true));
            if (wnum) ++(onepass ? b->n_onepass : b->n_sequential);
        }
    }
    HIP_TRY(hipEventRecord(b->ev_stop, b->s));
    b->last_steps = steps;
    b->timing_valid = true;
    if (wafer_batch_launch_count(steps, K, have2, nullptr) & 1)
        for (uint32_t m = 0; m < b->n; ++m)
            if (!active || active[m]) b->views[m]->cur ^= 1;
    return WAFER_OK;
}

int orthogonalise(wafer_batch *b, const uint8_t *active, uint32_t wnum)
{
    TRY(refuse_mixed(b, "wafer_batch_orthogonalise"));
    HIP_TRY(hipSetDevice(b->device));
    TRY(check_ready(b, active, false, "", wnum));
    if (wnum == 0) return WAFER_OK;
    TRY(ensure_gs(b));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    if (!nact) return WAFER_OK;
    if (use_onepass(b, wnum)) {
        TRY(ensure_onepass(b));
        TRY(refresh_gram(b, active));
        ++b->n_onepass;
        return gs_onepass(b, nact, 0, wnum, false);
    }
    ++b->n_sequential;
    return gs_chain(b, nact, 0, wnum, false);
}

// grid.rs:50-246 for every member and one state number: the loop of wafer_solve_state with one launch per operation for all
// running members.  push: a converged member's phi goes to its store (:239-242).
int solve(wafer_batch *b, uint32_t wnum, bool push, double tolerance, uint64_t screen_update, int has_max_steps, uint64_t max_steps,
          wafer_block_record *records, size_t max_records_per_member, size_t *n_records, wafer_observables_output *finals, int *status)
{
    const uint32_t n = b->n;
    std::vector<uint8_t> run(n, 1), converged(n, 0);
    std::vector<double> last_energy(n, DBL_MAX);   // grid.rs:124
    std::vector<size_t> nrec(n, 0);
    std::vector<wafer_observables_t> obs(n);
    std::string first_state_error;
    for (uint32_t m = 0; m < n; ++m) {
        status[m] = WAFER_OK;
        if (n_records) n_records[m] = 0;
        if (finals) memset(&finals[m], 0, sizeof finals[m]);
        if (wnum > b->nst[m]) {   // a short store is this member's error, not the call's: it is left as it stands
            char msg[160];
            snprintf(msg, sizeof msg, "member %u: wnum %u but w_store holds %u states", m, wnum, b->nst[m]);
            if (first_state_error.empty()) first_state_error = msg;
            status[m] = WAFER_ERR_STATE;
            run[m] = 0;
        }
    }
    uint64_t step = 0;
    auto finish = [&](uint32_t m) { // output.rs:540-547
        run[m] = 0;
        if (!finals) return;
        const wafer_observables_t &o = obs[m];
        const double r_norm = std::sqrt(o.r2 / o.norm2);
        finals[m].state = wnum;
        finals[m].energy = o.energy / o.norm2;
        finals[m].binding_energy = (o.energy - o.v_infinity) / o.norm2;
        finals[m].r = r_norm;
        finals[m].l_r = (double)b->P[m].nx / r_norm;
    };
    for (;;) {
        bool any = false;
        for (uint8_t r : run) any = any || r;
        if (!any) break;
        TRY(observables(b, run.data()));                          // :127
        std::vector<uint8_t> norm(run);
        for (uint32_t m = 0; m < n; ++m) {
            if (!run[m]) continue;
            obs_of(b, m, &obs[m]);
            const double norm_energy = obs[m].energy / obs[m].norm2;   // :128
            if (!std::isfinite(norm_energy)) {
                char msg[256];
                snprintf(msg, sizeof msg, "member %u, state %u: energy is not finite at step %llu (norm2 = %g): "
                         "the wavefunction vanished or diverged", m, wnum, (unsigned long long)step, obs[m].norm2);
                if (first_state_error.empty()) first_state_error = msg;
                status[m] = WAFER_ERR_STATE;
                run[m] = norm[m] = 0;
            }
        }
        // :130, the members' norm2 straight from the sums on the device (the same doubles the host holds)
        TRY(normalise(b, norm.data(), b->sums.dev + 1, 4));
        if (wnum) TRY(orthogonalise(b, norm.data(), wnum));        // :133-135
        for (uint32_t m = 0; m < n; ++m) {
            if (!run[m]) continue;
            const double norm_energy = obs[m].energy / obs[m].norm2;
            const double tau = (double)step * b->P[m].dt;           // :129
            const double diff = std::fabs(norm_energy - last_energy[m]); // :161
            if (records && nrec[m] < max_records_per_member) {
                wafer_block_record &r = records[(size_t)m * max_records_per_member + nrec[m]];
                r.step = step;
                r.tau = tau;
                r.obs = obs[m];
                r.diff = diff;
            }
            ++nrec[m];
            if (n_records) n_records[m] = nrec[m];
            if (diff < tolerance) { // :162-192
                converged[m] = 1;
                finish(m);
                continue;
            }
            last_energy[m] = norm_energy;                           // :194
            if (has_max_steps && step > max_steps) {                // :211-213
                status[m] = WAFER_ERR_MAX_STEP;
                finish(m);
            }
        }
        any = false;
        for (uint8_t r : run) any = any || r;
        if (!any) break;
        TRY(evolve_state(b, run.data(), wnum, screen_update));      // :216
        step += screen_update;                                      // :220
    }
    if (push) {   // :239-242; a member whose store is full keeps its result and gets the status
        for (uint32_t m = 0; m < n; ++m) {
            if (!converged[m] || check_capacity(b, m) == WAFER_OK) continue;
            if (first_state_error.empty()) first_state_error = wafer_last_error();
            status[m] = WAFER_ERR_STATE;
            converged[m] = 0;
        }
        TRY(push_states(b, converged.data()));
    }
    HIP_TRY(hipStreamSynchronize(b->s));
    if (!first_state_error.empty()) fail(WAFER_ERR_STATE, "%s", first_state_error.c_str());
    return WAFER_OK;
}

// ---- the range check of many members at once -----------------------------------------------------------------------------------
// the safe answers for the members in act, whose V was written but could not be checked: no mirrored reads, the long forms.
// Returns rc, the status of what failed.
int v_unknown(wafer_batch *b, int nact, int rc)
{
    for (int k = 0; k < nact; ++k) {
        wafer_ctx *c = b->views[b->act[k]];
        c->v_ysym = c->v_in_range = false;
        for (int &a : c->x2_agreed) a = -1;
    }
    (void)sync_members(b);
    return rc;
}

// check_v_range (wafer_engine.hip) for the members in act, whose V has just been written and whose v_ysym the writer
// cleared before its first store: the words' start values in one copy, ONE launch (wafer_k_batch_v_check), one read-back and one
// stream synchronisation, then per member the context's bookkeeping -- v_in_range by the same predicate, v_ysym, x2_agreed -- and the
// device member table as the views stand now.  A HIP error leaves every one of them with both flags off (v_unknown).
int check_v_listed(wafer_batch *b, int nact)
{
    auto run = [&]() -> int {
        BUF_TRY(StreamCopy::copy(b->vchk.dev, b->vchk_init, sizeof(unsigned long long) * 3 * (size_t)nact, true, b->s));
        int max_tiles = 0, max_planes = 0;
        for (int k = 0; k < nact; ++k) {
            const WaferGeom &g = b->geom((uint32_t)b->act[k]);
            max_tiles = std::max(max_tiles, wafer_v_check_tiles(g, (int)b->esz));
            max_planes = std::max(max_planes, g.lz);
        }
        TRY(launch(b, "range check", [&](const auto &gs) {
            return wafer_entry_batch_v_check(b->f32, gs, b->mem_dev, b->act.dev, nact, max_tiles, max_planes, b->vchk.dev, b->s);
        }));
        ++b->n_setup_launches;
        BUF_TRY(b->vchk.download(3 * (size_t)nact, b->s));
        HIP_TRY(hipStreamSynchronize(b->s));
        ++b->n_setup_readbacks;
        return WAFER_OK;
    };
    const int rc = run();
    if (rc != WAFER_OK) return v_unknown(b, nact, rc);
    for (int k = 0; k < nact; ++k) {
        wafer_ctx *c = b->views[b->act[k]];
        double lo, hi;
        memcpy(&lo, &b->vchk[3 * k], 8);
        memcpy(&hi, &b->vchk[3 * k + 1], 8);
        c->v_in_range = (lo > 0x1p-400) && (hi < 0x1p400);   // a NaN anywhere makes hi a NaN: false
        c->v_ysym = b->vchk[3 * k + 2] == 0;
        for (int &a : c->x2_agreed) a = -1;
    }
    return sync_members(b);
}

// ---- resampling --------------------------------------------------------------------------------------------------------------
// the resample scratch holds at least `doubles` doubles: grown on demand, never per call, freed with the batch
int ensure_scratch(wafer_batch *b, size_t doubles)
{
    if (doubles <= b->rs_scratch.size()) return WAFER_OK;
    HIP_TRY(hipStreamSynchronize(b->s));   // no launch in flight reads the scratch that goes back
    BUF_TRY(b->rs_scratch.reserve(doubles));
    return WAFER_OK;
}

// A host source on the device, x-fastest (wafer_resample_batch.hip.h): one upload into the batch's scratch and one transpose behind
// it, in stream order -- a later call reuses the scratch behind this call's launch.
int stage_host_source(wafer_batch *b, const double *src, int sx, int sy, int sz, WaferResampleSource *out)
{
    const size_t n = (size_t)sx * sy * sz;
    TRY(ensure_scratch(b, 2 * n));
    double *raw = b->rs_scratch, *xfast = b->rs_scratch + n;
    HIP_TRY(hipMemcpyAsync(raw, src, sizeof(double) * n, hipMemcpyHostToDevice, b->s));
    WaferXposeArgs a;
    memset(&a, 0, sizeof a);
    a.g.pitch = sx;                            // a dense [sz][sy][sx] box: only WaferGeom::at is read
    a.g.plane = (long long)sx * sy;
    a.sx = sx; a.sy = sy; a.sz = sz;
    const dim3 grid((unsigned)((sx + 31) / 32), (unsigned)sy, (unsigned)((sz + 31) / 32)), block(32, 8);
    hipLaunchKernelGGL((wafer_k_transpose<double, true>), grid, block, 0, b->s, a, raw, xfast);
    HIP_TRY(hipGetLastError());
    out->base = xfast;
    out->off0 = 0;
    out->pitch = sx;
    out->plane = (long long)sx * sy;
    out->sx = sx; out->sy = sy; out->sz = sz;
    return WAFER_OK;
}

// wafer_batch_resample (host != nullptr) and wafer_batch_resample_member: every check for every listed member, then one launch,
// then per member the bookkeeping of the context entry (wafer_upload_phi_resampled, wafer_set_potential_resampled,
// wafer_set_potsub_resampled) or of wafer_batch_load_state.
// A REFUSED call (WAFER_ERR_INVALID, WAFER_ERR_STATE) has changed nothing.  A HIP error (WAFER_ERR_HIP) is another matter, as for a
// context: before the launch it leaves every target as it was; behind it the arrays of all listed members are written, and for a
// potential a failure of refresh_ab or of the one range check for all listed members (check_v_listed) leaves EVERY listed member
// with v_ysym and v_in_range off -- the safe answers: no mirrored reads, the long arithmetic forms -- until the potential is set
// again; the a, b arrays and the have_pot bookkeeping stop at the member whose refresh_ab failed.
int resample(wafer_batch *b, const uint8_t *active, int target, uint32_t idx, const double *host, uint32_t sx, uint32_t sy, uint32_t sz,
             uint32_t src_member, int src_kind, uint32_t src_idx, int basis)
{
    if (target < WAFER_RESAMPLE_PHI || target > WAFER_RESAMPLE_STATE) return fail(WAFER_ERR_INVALID, "unknown resample target %d", target);
    if (basis != WAFER_BASIS_PADDED && basis != WAFER_BASIS_WORK) return fail(WAFER_ERR_INVALID, "unknown resample basis %d", basis);
    if (target == WAFER_RESAMPLE_POTSUB && basis != WAFER_BASIS_WORK)
        return fail(WAFER_ERR_INVALID, "pot_sub is resampled with the work size as basis (input.rs:472): WAFER_BASIS_WORK");
    if (!host) {
        if (src_member >= b->n) return fail(WAFER_ERR_INVALID, "source member %u out of range (the batch has %u)", src_member, b->n);
        if (src_kind != WAFER_RESAMPLE_PHI && src_kind != WAFER_RESAMPLE_STATE)
            return fail(WAFER_ERR_INVALID, "a member source is its phi (WAFER_RESAMPLE_PHI) or a stored state (WAFER_RESAMPLE_STATE), not %d", src_kind);
        const WaferGeom &sg = b->geom(src_member);
        sx = (uint32_t)sg.nx; sy = (uint32_t)sg.ny; sz = (uint32_t)sg.nz;
    }
    if (sx < 2 || sy < 2 || sz < 2) return fail(WAFER_ERR_INVALID, "resampling needs at least 2 points per axis");
    if (sx > 0x7fffffffu || sy > 0x7fffffffu || sz > 0x7fffffffu) return fail(WAFER_ERR_INVALID, "source size out of range");
    if (target == WAFER_RESAMPLE_STATE || (!host && src_kind == WAFER_RESAMPLE_STATE)) TRY(refuse_mixed(b, "wafer_batch_resample (stored states)"));
    if (!host) {
        if (src_kind == WAFER_RESAMPLE_PHI && !b->views[src_member]->have_phi) return fail(WAFER_ERR_STATE, "source member %u: phi not set", src_member);
        if (src_kind == WAFER_RESAMPLE_STATE && src_idx >= b->nst[src_member]) return fail(WAFER_ERR_STATE, "source member %u: no state %u", src_member, src_idx);
    }
    int nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        ++nlisted;
        if (!host && m == src_member && target == src_kind && (target == WAFER_RESAMPLE_PHI || idx == src_idx))
            return fail(WAFER_ERR_INVALID, "member %u is the source and a target in the same buffer", m);
        if (target == WAFER_RESAMPLE_POTSUB && !b->views[m]->have_pot) return fail(WAFER_ERR_STATE, "member %u: set the potential first", m);
        if (target == WAFER_RESAMPLE_STATE) {
            if (idx > b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: states must be loaded in order", m);
            if (idx == b->nst[m]) TRY(check_capacity(b, m));
        }
    }
    if (!nlisted) return WAFER_OK;

    HIP_TRY(hipSetDevice(b->device));
    if (target == WAFER_RESAMPLE_STATE) TRY(ensure_slots(b, b->slots, idx + 1));
    b->rs_timing_valid = false;   // (a call that fails below leaves no half-recorded pair behind)
    if (host) TRY(ensure_scratch(b, 2 * (size_t)sx * sy * sz));   // (before the events: growing it synchronises, frees and allocates)
    HIP_TRY(hipEventRecord(b->rs_start, b->s));
    WaferResampleSource src;
    if (host) {
        TRY(stage_host_source(b, host, (int)sx, (int)sy, (int)sz, &src));
    } else {
        const WaferGeom &sg = b->geom(src_member);
        const wafer_ctx *sc = b->views[src_member];
        src.base = src_kind == WAFER_RESAMPLE_PHI ? sc->phi[sc->cur] : slot_ptr(b, src_idx, src_member);
        src.off0 = sg.at(sg.G, sg.R, sg.R);
        src.pitch = sg.pitch;
        src.plane = sg.plane;
        src.sx = sg.nx; src.sy = sg.ny; src.sz = sg.nz;
    }
    TRY(sync_members(b));   // (the kernel reads cur)
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    // From here on the targets are written.  V is about to change: check_v_listed re-establishes the flag (cleared behind the last
    // step that can fail before the launch, so that a call that launched nothing leaves it as it was).
    if (target == WAFER_RESAMPLE_POTENTIAL)
        for (uint32_t m = 0; m < b->n; ++m)
            if (!active || active[m]) b->views[m]->v_ysym = false;
    int max_tiles, max_planes;   // of the padded boxes: the kernel writes the frame's zeros too
    max_tiles_planes(b, nact, true, &max_tiles, &max_planes);
    void *dst0 = target == WAFER_RESAMPLE_PHI ? b->alloc[0] : target == WAFER_RESAMPLE_POTENTIAL ? b->alloc[2]
               : target == WAFER_RESAMPLE_POTSUB ? b->alloc[3] : b->slots[idx];
    void *dst1 = target == WAFER_RESAMPLE_PHI ? b->alloc[1].get() : dst0;
    {
        RoctxRange range_("wafer_batch_resample");
        TRY(launch(b, "resample", [&](const auto &gs) {
            return wafer_entry_batch_trilerp(b->f32, !host && b->f32, gs, b->mem_dev, b->act.dev, nact, max_tiles, max_planes, src, dst0, dst1,
                                             target == WAFER_RESAMPLE_PHI, basis, b->s);
        }));
    }
    HIP_TRY(hipEventRecord(b->rs_stop, b->s));
    b->rs_timing_valid = true;
    if (host) HIP_TRY(hipStreamSynchronize(b->s));   // the caller's array has been read
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        wafer_ctx *c = b->views[m];
        switch (target) {
        case WAFER_RESAMPLE_PHI:
            c->have_phi = true;
            c->halo_valid = c->g.G;   // ghost planes were interpolated from the same source
            break;
        case WAFER_RESAMPLE_POTENTIAL: {
            const int rc = refresh_ab(c);
            if (rc != WAFER_OK) return v_unknown(b, nact, rc);
            c->vgen_type = 0;
            c->potsub_kind = WAFER_POTSUB_NONE;   // potential.rs:357-358: FromFile has no pot_sub of its own
            c->potsub_scalar = 0.0;
            c->have_pot = true;
            c->x2_ready = 0;
            break;
        }
        case WAFER_RESAMPLE_POTSUB:
            c->potsub_kind = WAFER_POTSUB_ARRAY;
            c->potsub_scalar = 0.0;
            break;
        default:
            if (idx == b->nst[m]) ++b->nst[m];
            mark_gram_stale(b, m);
            break;
        }
    }
    if (target == WAFER_RESAMPLE_POTENTIAL) return check_v_listed(b, nact);   // one launch and one read-back for all of them
    return WAFER_OK;
}

// ---- set-up of many members at once ------------------------------------------------------------------------------------------
// one record per member in act (upload_active has synchronised the stream: setup's host side is not read by an earlier call's copy)
int upload_setup(wafer_batch *b, int nact, const int *kinds, const uint64_t *seeds)
{
    double k[4];
    pot_host_constants(k);
    for (int i = 0; i < nact; ++i) {
        const int m = b->act[i];
        const wafer_ctx *c = b->views[m];
        WaferBatchSetupRec &r = b->setup[i];
        r.member = m;
        r.kind = kinds[m];
        r.seed = seeds ? seeds[m] : 0;
        r.dn = c->P.dn; r.dt = c->P.dt; r.mass = c->P.mass; r.sig = c->P.sig;
        r.mu_t = k[0]; r.alphas_2pit = k[1]; r.xi_coef = k[2]; r.xi_fac = k[3];
        r.pa = c->a;
        r.pb = c->b;
    }
    BUF_TRY(b->setup.upload(nact, b->s));
    return WAFER_OK;
}

// wafer_set_potential_builtin for every listed member: every check first, then one launch for V (a, b), one for the pot_sub arrays
// if a listed member is FullCornell, the context's bookkeeping per member, and the one range check.
int set_potentials(wafer_batch *b, const uint8_t *active, const int *potentials)
{
    int nlisted = 0;
    bool fullcornell = false;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        const int pot = potentials[m];
        if (pot < 0 || pot > WAFER_POT_FROMSCRIPT) return fail(WAFER_ERR_INVALID, "member %u: unknown potential %d", m, pot);
        if (pot == WAFER_POT_FROMFILE || pot == WAFER_POT_FROMSCRIPT)
            return fail(WAFER_ERR_NOT_AVAILABLE, "member %u: PotentialNotAvailable: FromFile/FromScript need wafer_set_potential_host", m);
        fullcornell = fullcornell || pot == WAFER_POT_FULLCORNELL;
        ++nlisted;
    }
    if (!nlisted) return WAFER_OK;
    HIP_TRY(hipSetDevice(b->device));
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    TRY(upload_setup(b, nact, potentials, nullptr));
    for (int k = 0; k < nact; ++k) b->views[b->act[k]]->v_ysym = false;   // V is about to change: check_v_listed re-establishes it
    int max_tiles, max_planes;
    max_tiles_planes(b, nact, true, &max_tiles, &max_planes);
    RoctxRange range_("wafer_batch_set_potentials");
    TRY(launch(b, "potential", [&](const auto &gs) {
        return wafer_entry_batch_potential(b->f32, gs, b->mem_dev, b->setup.dev, nact, max_tiles, max_planes, b->s);
    }));
    ++b->n_setup_launches;
    if (fullcornell) {
        const int rc = launch(b, "pot_sub", [&](const auto &gs) {
            return wafer_entry_batch_potsub_fullcornell(b->f32, gs, b->mem_dev, b->setup.dev, nact, max_tiles, max_planes, b->s);
        });
        if (rc != WAFER_OK) return v_unknown(b, nact, rc);
        ++b->n_setup_launches;
    }
    for (int k = 0; k < nact; ++k) builtin_potential_set(b->views[b->act[k]], potentials[b->act[k]]);
    return check_v_listed(b, nact);
}

// wafer_set_initial_condition for every listed member: every check first, then one launch into the members' phi[cur]
int set_initial_conditions(wafer_batch *b, const uint8_t *active, const int *ics, const uint64_t *seeds)
{
    int nlisted = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        if (ics[m] == WAFER_IC_FROMFILE) return fail(WAFER_ERR_NOT_AVAILABLE, "member %u: FromFile: use wafer_upload_phi", m);
        if (ics[m] < WAFER_IC_GAUSSIAN || ics[m] > WAFER_IC_BOOLEAN) return fail(WAFER_ERR_INVALID, "member %u: unknown initial condition %d", m, ics[m]);
        ++nlisted;
    }
    if (!nlisted) return WAFER_OK;
    HIP_TRY(hipSetDevice(b->device));
    TRY(sync_members(b));   // (the kernel reads cur)
    int nact = 0;
    TRY(upload_active(b, active, &nact));
    TRY(upload_setup(b, nact, ics, seeds));
    int max_tiles, max_planes;
    max_tiles_planes(b, nact, true, &max_tiles, &max_planes);
    RoctxRange range_("wafer_batch_set_initial_conditions");
    TRY(launch(b, "initial condition", [&](const auto &gs) {
        return wafer_entry_batch_initial_condition(b->f32, gs, b->mem_dev, b->setup.dev, nact, max_tiles, max_planes, b->s);
    }));
    ++b->n_setup_launches;
    for (int k = 0; k < nact; ++k) {
        wafer_ctx *c = b->views[b->act[k]];
        c->have_phi = true;
        c->halo_valid = c->g.G;   // every ghost plane was generated from global indices
    }
    return WAFER_OK;
}

// ---- creation --------------------------------------------------------------------------------------------------------------
// Every member's partition record and the places of its partials.  Observables: the partition wafer_launch_observables_lds gives a
// single context of the member's shape and storage type -- 16 bytes per lane, so tiles 128 wide on doubles and 256 wide on floats
// (WaferLdsCfg::TX), and the z-chunk that follows from them -- with its [4][obs_nb] partials end to end (one shape: member m's at
// m * 4 * obs_nb).  norm2: n2_nb workgroups, the partials end to end likewise.  The kernels read all of it from the records.
constexpr int (*LDS_ZCHUNK[2][3])(const WaferTuning &, const WaferGeom &, int, int, int) = {   // wafer_lds_zchunk<T, R> at [float storage][R - 1]
    {wafer_lds_zchunk<double, 1>, wafer_lds_zchunk<double, 2>, wafer_lds_zchunk<double, 3>},
    {wafer_lds_zchunk<float, 1>, wafer_lds_zchunk<float, 2>, wafer_lds_zchunk<float, 3>}};
int init_partitions(wafer_batch *b)
{
    const int R = b->g().R;
    const int NW = R <= 2 ? 8 : 4;
    const int TX = b->f32 ? WaferLdsCfg<float, 1, 2>::TX : WaferLdsCfg<double, 1, 2>::TX, TY = 2 * NW;
    const int ry = 2 * (NW / 4);
    b->swz = wafer_lds_opts(b->tune).swz;
    b->mem.resize(b->n);
    b->gsp = wafer_batch_gs_partition(b->geoms.data(), b->shape_of.data(), b->n, WAFER_BATCH_TX, WAFER_BATCH_TY, WAFER_GS_ZC);
    size_t obs_total = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        WaferBatchMember &e = b->mem[m];
        memset(&e, 0, sizeof e);
        const WaferGeom &g = b->geom(m);
        e.obs_zchunk = LDS_ZCHUNK[b->f32 ? 1 : 0][R - 1](b->tune, g, g.nzl, ry, b->num_cus);
        e.shape = b->shape_of[m];
        e.obs_ntx = (g.nx + TX - 1) / TX;
        e.obs_nty = (g.ny + TY - 1) / TY;
        e.obs_nb = e.obs_ntx * e.obs_nty * ((g.nzl + e.obs_zchunk - 1) / e.obs_zchunk);
        e.n2_nb = b->f32 ? wafer_rownorm2_blocks(g, (int)b->esz, b->num_cus) : wafer_gs_blocks(g);
        e.obs_off = (long long)obs_total;
        e.n2_off = (long long)b->n2_doubles;
        e.gs_nb = b->gsp.nb[m];
        e.gs_off = b->gsp.first[m];
        e.slot_off = (long long)b->off[m] + g.base_off;
        obs_total += 4 * (size_t)e.obs_nb;
        b->n2_doubles += (size_t)e.n2_nb;
    }
    BUF_TRY(b->partials.make(obs_total));
    return WAFER_OK;
}

// The members' context views on their slices of the batch's arrays (b->alloc, b->view_scal), as wafer_ctx_create sets a context up,
// and what the member records take from them: the array pointers, dt and the division plans.
int init_views(wafer_batch *b)
{
    const int R = b->g().R;
    b->views.reserve(b->n);
    for (uint32_t m = 0; m < b->n; ++m) {
        wafer_ctx *c = new wafer_ctx();
        b->views.push_back(c);
        const wafer_params &p = b->P[m];
        const WaferGeom &g = b->geom(m);
        c->P = p;
        c->g = g;
        c->f32 = b->f32;
        c->f32_arith = p.dtype == WAFER_F32_FAST;
        c->esz = b->esz;
        c->num_cus = b->num_cus;
        c->tune = b->tune;
        c->bx = (g.px + 63) / 64;
        c->by = (g.py + 3) / 4;
        c->s_main = c->s_aux = b->s;
        c->div_plan = wafer_divplan_make(wafer_stencil_den(R, p.dn, p.mass));
        if (c->f32_arith) c->div_plan_f = wafer_divplan_make_f32((float)wafer_stencil_den(R, p.dn, p.mass));
        if (p.flags & WAFER_FLAG_UNPLANNED_DIV) c->div_plan.checked = c->div_plan_f.checked = 0;
        void **arr[4] = {&c->phi[0], &c->phi[1], &c->v, &c->potsub};
        for (int k = 0; k < 4; ++k)
            *arr[k] = b->alloc[k] + (b->off[m] + (size_t)g.base_off) * b->esz;
        c->scal = b->view_scal.dev + (size_t)m * SCAL_SLOTS;
        c->scal_host = &b->view_scal[(size_t)m * SCAL_SLOTS];
        c->kernel_name = "wafer_k_batch_step";
        WaferBatchMember &e = b->mem[m];
        e.phi[0] = c->phi[0];
        e.phi[1] = c->phi[1];
        e.v = c->v;
        e.potsub = c->potsub;
        e.dt = p.dt;
        e.den = c->div_plan.den;
        e.zh = c->div_plan.zh;
        e.zl = c->div_plan.zl;
        e.den_f = (float)c->div_plan.den;   // (wafer_den<float> of a context's WaferStepArgs)
        e.zh_f = c->div_plan_f.checked ? c->div_plan_f.zh : 0.f;
        e.zl_f = c->div_plan_f.checked ? c->div_plan_f.zl : 0.f;
    }
    return WAFER_OK;
}

// wafer_batch_create (same_shape), wafer_batch_create_mixed, and wafer_batch_create_mixed_states (states: state stores on several shapes)
int create_batch(const wafer_params *members, uint32_t n_members, bool same_shape, bool states, wafer_batch **out)
{
    if (!members || !out) return fail(WAFER_ERR_INVALID, "null argument");
    if (n_members == 0) return fail(WAFER_ERR_INVALID, "a batch needs at least one member (n_members = 0)");
    for (uint32_t i = 0; i < n_members; ++i) TRY(check_member(&members[i], i, i ? &members[0] : nullptr, same_shape));
    const wafer_params &p0 = members[0];
    const int R = p0.central_difference;
    const bool f32 = p0.dtype != WAFER_F64;
    const size_t esz = f32 ? 4 : 8;
    std::vector<int> nxyz;
    for (uint32_t m = 0; m < n_members; ++m) nxyz.insert(nxyz.end(), {(int)members[m].nx, (int)members[m].ny, (int)members[m].nz});
    WaferBatchLayout L = wafer_batch_layout(nxyz.data(), n_members, R, p0.halo_depth ? (int)p0.halo_depth : R, esz);
    if (L.overflow)
        return fail(WAFER_ERR_INVALID, "%u members of %zu padded cells up to member %u overflow the size of one allocation", n_members, L.cells,
                    (uint32_t)L.off.size() - 1);
    if (L.misaligned)
        return fail(WAFER_ERR_INVALID, "a member's span in the batch's allocations does not start and end on 16 bytes (elements of %zu bytes): "
                                       "the rotation of stored states walks whole 16-byte vectors", esz);

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(WAFER_ERR_HIP, "no HIP device visible: the engine has no CPU path");
    if (p0.device < 0 || p0.device >= ndev) return fail(WAFER_ERR_INVALID, "member 0: device %d out of range", p0.device);
    HIP_TRY(hipSetDevice(p0.device));
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p0.device));

    std::unique_ptr<wafer_batch> owner(new wafer_batch());   // (a failure below frees what exists)
    wafer_batch *b = owner.get();
    b->n = n_members;
    b->P.assign(members, members + n_members);
    b->device = p0.device;
    b->num_cus = cus > 0 ? cus : 256;
    b->tune = wafer_tuning_from_env();
    b->geoms = std::move(L.geoms);
    b->shape_of = std::move(L.shape_of);
    b->off = std::move(L.off);
    b->cells = L.cells;
    b->mixed = b->geoms.size() > 1;
    b->mixed_states = b->mixed && states;   // (one distinct shape: a plain batch in every call)
    b->dtype = (int)p0.dtype;
    b->f32 = f32;
    b->esz = esz;
    b->nst.assign(n_members, 0);
    for (uint32_t m = 0; m < n_members; ++m) b->gs_stride = std::max(b->gs_stride, 1 + (int)members[m].max_states);
    if (b->mixed) {
        char name[96];
        snprintf(name, sizeof name, "wafer_k_batch_step<%d,%s,WaferBatchGeomTable>", R, KERNEL_TYPES[b->dtype]);
        b->kernel_name = name;
    }
    HIP_TRY(hipStreamCreateWithFlags(&b->s.h, hipStreamNonBlocking));
    for (hipEvent_t *e : {&b->ev_start, &b->ev_stop, &b->rs_start, &b->rs_stop}) HIP_TRY(hipEventCreate(e));
    for (DevArray<char> &a : b->alloc) {   // one allocation per array kind, zeros: frames, pads and guard zones of every member
        BUF_TRY(a.make(b->cells * esz));
        HIP_TRY(hipMemsetAsync(a, 0, a.bytes(), b->s));
    }
    BUF_TRY(b->view_scal.make((size_t)SCAL_SLOTS * n_members));
    HIP_TRY(hipMemsetAsync(b->view_scal.dev, 0, b->view_scal.dev.bytes(), b->s));
    TRY(init_partitions(b));
    BUF_TRY(b->sums.make(4 * (size_t)n_members));
    BUF_TRY(b->n2.make(n_members));
    BUF_TRY(b->act.make(n_members));
    BUF_TRY(b->sym.make(n_members));
    BUF_TRY(b->mem_dev.make(n_members));
    BUF_TRY(b->setup.make(n_members));
    BUF_TRY(b->vchk.make(3 * (size_t)n_members));
    BUF_TRY(b->vchk_init.make(3 * (size_t)n_members));
    for (uint32_t m = 0; m < n_members; ++m) {
        b->vchk_init[3 * m] = ~0ull;
        b->vchk_init[3 * m + 1] = b->vchk_init[3 * m + 2] = 0ull;
    }
    BUF_TRY(b->geoms_dev.make(b->geoms.size()));
    HIP_TRY(hipMemcpy(b->geoms_dev, b->geoms.data(), b->geoms_dev.bytes(), hipMemcpyHostToDevice));
    TRY(init_views(b));
    HIP_TRY(hipMemcpy(b->mem_dev, b->mem.data(), b->mem_dev.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(b->s));
    *out = owner.release();
    return WAFER_OK;
}

} // namespace

extern "C" {

int wafer_batch_create(const wafer_params *members, uint32_t n_members, wafer_batch **out)
{
    return create_batch(members, n_members, true, false, out);
}

int wafer_batch_create_mixed(const wafer_params *members, uint32_t n_members, wafer_batch **out)
{
    return create_batch(members, n_members, false, false, out);
}

int wafer_batch_create_mixed_states(const wafer_params *members, uint32_t n_members, wafer_batch **out)
{
    return create_batch(members, n_members, false, true, out);
}

int wafer_batch_num_shapes(wafer_batch *b, uint32_t *n_shapes)
{
    if (!b || !n_shapes) return fail(WAFER_ERR_INVALID, "null argument");
    *n_shapes = (uint32_t)b->geoms.size();
    return WAFER_OK;
}

int wafer_batch_destroy(wafer_batch *b)
{
    delete b;   // (~wafer_batch: what exists goes, the stream last)
    return WAFER_OK;
}

int wafer_batch_size(wafer_batch *b, uint32_t *n_members)
{
    if (!b || !n_members) return fail(WAFER_ERR_INVALID, "null argument");
    *n_members = b->n;
    return WAFER_OK;
}

int wafer_batch_set_potential_builtin(wafer_batch *b, uint32_t member, int potential)
{
    TRY(check_member_index(b, member));
    return wafer_set_potential_builtin(b->views[member], potential);
}

int wafer_batch_set_potential_host(wafer_batch *b, uint32_t member, const double *v, int potsub_kind, double potsub_scalar,
                                   const double *potsub)
{
    TRY(check_member_index(b, member));
    return wafer_set_potential_host(b->views[member], v, potsub_kind, potsub_scalar, potsub);
}

int wafer_batch_set_potsub(wafer_batch *b, uint32_t member, int kind, double scalar, const double *potsub)
{
    TRY(check_member_index(b, member));
    return wafer_set_potsub(b->views[member], kind, scalar, potsub);
}

int wafer_batch_resample(wafer_batch *b, const uint8_t *active, int target, uint32_t idx, const double *src, uint32_t sx, uint32_t sy,
                         uint32_t sz, int basis)
{
    if (!b || !src) return fail(WAFER_ERR_INVALID, "null argument");
    return resample(b, active, target, idx, src, sx, sy, sz, 0, 0, 0, basis);
}

int wafer_batch_resample_member(wafer_batch *b, const uint8_t *active, int target, uint32_t idx, uint32_t src_member, int src_kind,
                                uint32_t src_idx, int basis)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    return resample(b, active, target, idx, nullptr, 0, 0, 0, src_member, src_kind, src_idx, basis);
}

int wafer_batch_symmetrise(wafer_batch *b, const uint8_t *active, const int *constraints)
{
    if (!b || !constraints) return fail(WAFER_ERR_INVALID, "null argument");
    return symmetrise(b, active, constraints);
}

int wafer_batch_set_initial_condition(wafer_batch *b, uint32_t member, int ic, uint64_t seed)
{
    TRY(check_member_index(b, member));
    return wafer_set_initial_condition(b->views[member], ic, seed);
}

int wafer_batch_set_potentials_builtin(wafer_batch *b, const uint8_t *active, const int *potentials)
{
    if (!b || !potentials) return fail(WAFER_ERR_INVALID, "null argument");
    return set_potentials(b, active, potentials);
}

int wafer_batch_set_initial_conditions(wafer_batch *b, const uint8_t *active, const int *ics, const uint64_t *seeds)
{
    if (!b || !ics) return fail(WAFER_ERR_INVALID, "null argument");
    return set_initial_conditions(b, active, ics, seeds);
}

int wafer_batch_download_array(wafer_batch *b, uint32_t member, int array_id, double *out)
{
    TRY(check_member_index(b, member));
    return wafer_download_array(b->views[member], array_id, out);
}

int wafer_batch_get_potsub(wafer_batch *b, uint32_t member, int *kind, double *scalar)
{
    TRY(check_member_index(b, member));
    return wafer_get_potsub(b->views[member], kind, scalar);
}

int wafer_batch_diag_member(wafer_batch *b, uint32_t member, char *buf, size_t n)
{
    TRY(check_member_index(b, member));
    if (!buf || n == 0) return fail(WAFER_ERR_INVALID, "null argument");
    const wafer_ctx *c = b->views[member];
    snprintf(buf, n, "member=%u have_pot=%d have_phi=%d potsub_kind=%d v_in_range=%d v_ysym=%d short_forms=%d cur=%d states=%u", member,
             (int)c->have_pot, (int)c->have_phi, c->potsub_kind, (int)c->v_in_range, (int)c->v_ysym, short_forms(c) ? 1 : 0, c->cur, b->nst[member]);
    return WAFER_OK;
}

int wafer_batch_diag_setup_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks)
{
    if (!b || !launches || !readbacks) return fail(WAFER_ERR_INVALID, "null argument");
    *launches = b->n_setup_launches;
    *readbacks = b->n_setup_readbacks;
    return WAFER_OK;
}

int wafer_batch_upload_phi(wafer_batch *b, uint32_t member, const double *phi)
{
    TRY(check_member_index(b, member));
    return wafer_upload_phi(b->views[member], phi);
}

int wafer_batch_download_phi(wafer_batch *b, uint32_t member, double *phi)
{
    TRY(check_member_index(b, member));
    return wafer_download_phi(b->views[member], phi);
}

int wafer_batch_evolve(wafer_batch *b, const uint8_t *active, uint64_t n_steps)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    return evolve_state(b, active, 0, n_steps);
}

int wafer_batch_observables(wafer_batch *b, wafer_observables_t *out)
{
    if (!b || !out) return fail(WAFER_ERR_INVALID, "null argument");
    TRY(observables(b, nullptr));
    for (uint32_t m = 0; m < b->n; ++m) obs_of(b, m, &out[m]);
    return WAFER_OK;
}

int wafer_batch_normalise(wafer_batch *b, const uint8_t *active, const double *norm2)
{
    if (!b || !norm2) return fail(WAFER_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->s));   // n2's host side is read by a copy of an earlier call
    memcpy(b->n2.host, norm2, b->n2.host.bytes());
    BUF_TRY(b->n2.upload(b->n, b->s));
    return normalise(b, active, b->n2.dev, 1);
}

int wafer_batch_solve(wafer_batch *b, double tolerance, uint64_t screen_update, int has_max_steps, uint64_t max_steps,
                      wafer_block_record *records, size_t max_records_per_member, size_t *n_records,
                      wafer_observables_output *finals, int *status)
{
    if (!b || !status) return fail(WAFER_ERR_INVALID, "null argument");
    return solve(b, 0, false, tolerance, screen_update, has_max_steps, max_steps, records, max_records_per_member, n_records, finals, status);
}

int wafer_batch_solve_state(wafer_batch *b, uint32_t wnum, double tolerance, uint64_t screen_update, int has_max_steps,
                            uint64_t max_steps, wafer_block_record *records, size_t max_records_per_member, size_t *n_records,
                            wafer_observables_output *finals, int *status)
{
    if (!b || !status) return fail(WAFER_ERR_INVALID, "null argument");
    TRY(refuse_mixed(b, "wafer_batch_solve_state"));
    return solve(b, wnum, true, tolerance, screen_update, has_max_steps, max_steps, records, max_records_per_member, n_records, finals, status);
}

int wafer_batch_evolve_state(wafer_batch *b, const uint8_t *active, uint32_t wnum, uint64_t n_steps)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    return evolve_state(b, active, wnum, n_steps);
}

int wafer_batch_orthogonalise(wafer_batch *b, const uint8_t *active, uint32_t wnum)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    return orthogonalise(b, active, wnum);
}

int wafer_batch_norm2(wafer_batch *b, double *out)
{
    if (!b || !out) return fail(WAFER_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    TRY(check_ready(b, nullptr, false, "", 0));
    TRY(ensure_gs(b));
    TRY(sync_members(b));
    int nact = 0;
    TRY(upload_active(b, nullptr, &nact));
    // every member on its own shape's partition: a context's wafer_norm2 partition on float storage (wafer_rownorm2_blocks: the same
    // double), the chain's on doubles (wafer_gs_blocks)
    int max_nb = 0;
    for (uint32_t m = 0; m < b->n; ++m) max_nb = std::max(max_nb, b->mem[m].n2_nb);
    TRY(launch(b, "norm2", [&](const auto &gs) {
        return wafer_entry_batch_norm2(b->f32, gs, b->mem_dev, b->act.dev, nact, max_nb, b->gs_scal.dev, b->gs_stride, 0, b->gs_partials, b->s);
    }));
    BUF_TRY(b->gs_scal.download(b->gs_scal.host.size(), b->s));
    HIP_TRY(hipStreamSynchronize(b->s));
    for (uint32_t m = 0; m < b->n; ++m) out[m] = b->gs_scal[(size_t)m * b->gs_stride];
    return WAFER_OK;
}

int wafer_batch_push_state(wafer_batch *b, const uint8_t *active)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    TRY(refuse_mixed(b, "wafer_batch_push_state"));
    return push_states(b, active);
}

int wafer_batch_load_state(wafer_batch *b, uint32_t member, uint32_t idx, const double *state)
{
    TRY(check_member_index(b, member));
    if (!state) return fail(WAFER_ERR_INVALID, "null argument");
    TRY(refuse_mixed(b, "wafer_batch_load_state"));
    HIP_TRY(hipSetDevice(b->device));
    if (idx > b->nst[member]) return fail(WAFER_ERR_STATE, "member %u: states must be loaded in order", member);
    if (idx == b->nst[member]) TRY(check_capacity(b, member));
    TRY(ensure_slots(b, b->slots, idx + 1));
    TRY(upload_padded(b->views[member], state, slot_ptr(b, idx, member)));
    if (idx == b->nst[member]) ++b->nst[member];
    mark_gram_stale(b, member);
    return WAFER_OK;
}

int wafer_batch_download_state(wafer_batch *b, uint32_t member, uint32_t idx, double *out)
{
    TRY(check_member_index(b, member));
    if (!out) return fail(WAFER_ERR_INVALID, "null argument");
    TRY(refuse_mixed(b, "wafer_batch_download_state"));
    if (idx >= b->nst[member]) return fail(WAFER_ERR_STATE, "member %u: no state %u", member, idx);
    HIP_TRY(hipSetDevice(b->device));
    return download_padded(b->views[member], out, slot_ptr(b, idx, member));
}

int wafer_batch_num_states(wafer_batch *b, uint32_t *counts_out)
{
    if (!b || !counts_out) return fail(WAFER_ERR_INVALID, "null argument");
    for (uint32_t m = 0; m < b->n; ++m) counts_out[m] = b->nst[m];
    return WAFER_OK;
}

int wafer_batch_clear_states(wafer_batch *b, const uint8_t *active)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    TRY(refuse_mixed(b, "wafer_batch_clear_states"));
    HIP_TRY(hipSetDevice(b->device));
    uint32_t keep = 0;
    for (uint32_t m = 0; m < b->n; ++m) {
        if (!active || active[m]) {
            b->nst[m] = 0;
            mark_gram_stale(b, m);
        }
        keep = std::max(keep, b->nst[m]);
    }
    if (b->slots.size() > keep) {   // slots no member uses any more go back
        HIP_TRY(hipStreamSynchronize(b->s));
        b->slots.resize(keep);
    }
    return WAFER_OK;
}

int wafer_batch_clone_state_to_phi(wafer_batch *b, const uint8_t *active, uint32_t idx)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    TRY(refuse_mixed(b, "wafer_batch_clone_state_to_phi"));
    HIP_TRY(hipSetDevice(b->device));
    for (uint32_t m = 0; m < b->n; ++m)
        if ((!active || active[m]) && idx >= b->nst[m]) return fail(WAFER_ERR_STATE, "member %u: no state %u", m, idx);
    for (uint32_t m = 0; m < b->n; ++m) {
        if (active && !active[m]) continue;
        wafer_ctx *c = b->views[m];
        HIP_TRY(hipMemcpyAsync(alloc_base(c, c->phi[c->cur]), alloc_base(c, slot_ptr(b, idx, m)), (size_t)b->geom(m).total * b->esz, hipMemcpyDeviceToDevice, b->s));
        c->have_phi = true;
        c->halo_valid = 0;
    }
    return WAFER_OK;
}

int wafer_batch_last_evolve_ms(wafer_batch *b, float *ms, uint64_t *steps)
{
    if (!b || !ms || !steps) return fail(WAFER_ERR_INVALID, "null argument");
    if (!b->timing_valid) return fail(WAFER_ERR_STATE, "no wafer_batch_evolve has run");
    HIP_TRY(hipEventSynchronize(b->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, b->ev_start, b->ev_stop));
    *steps = b->last_steps;
    return WAFER_OK;
}

int wafer_batch_last_resample_ms(wafer_batch *b, float *ms)
{
    if (!b || !ms) return fail(WAFER_ERR_INVALID, "null argument");
    if (!b->rs_timing_valid) return fail(WAFER_ERR_STATE, "no wafer_batch_resample has run");
    HIP_TRY(hipEventSynchronize(b->rs_stop));
    HIP_TRY(hipEventElapsedTime(ms, b->rs_start, b->rs_stop));
    return WAFER_OK;
}

const char *wafer_batch_kernel_name(wafer_batch *b)
{
    return b ? b->kernel_name.c_str() : "wafer_k_batch_step";
}

int wafer_batch_steps_per_launch(wafer_batch *b)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    return steps_per_pass(b);
}

int wafer_batch_set_step_variant(wafer_batch *b, int variant)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    if (variant < -1 || variant > 1) return fail(WAFER_ERR_INVALID, "step variant must be -1 (default), 0 (one step per launch) or 1 (fused passes)");
    b->step_variant = variant;
    return WAFER_OK;
}

int wafer_batch_diag_dispatch(wafer_batch *b, char *buf, size_t n)
{
    if (!b || !buf || n == 0) return fail(WAFER_ERR_INVALID, "null argument");
    static const char *const stencils[] = {"", "ThreePoint", "FivePoint", "SevenPoint"};
    char tn[48] = "";   // the kernels' <.., T, C> beside the fp64 default; several shapes: all of them, and the geometry source after them
    if (b->mixed) snprintf(tn, sizeof tn, ",%s,WaferBatchGeomTable", KERNEL_TYPES[b->dtype]);
    else if (b->dtype != WAFER_F64) snprintf(tn, sizeof tn, ",%s", KERNEL_TYPES[b->dtype]);
    const int R = b->g().R, K = steps_per_pass(b);
    char kernel[96], tile[32];
    const char *remainder = "none";
    if (K > 1) {
        snprintf(kernel, sizeof kernel, "wafer_k_batch_stepk<%d,%d%s>", R, K, tn);
        snprintf(tile, sizeof tile, "%dx%d", WAFER_BATCHK_TX, WAFER_BATCHK_TY);
        remainder = have_two_step(b, K) ? "stepk2+step" : "step";
    } else {
        snprintf(kernel, sizeof kernel, "wafer_k_batch_step<%d%s>", R, tn);
        snprintf(tile, sizeof tile, "%dx%d", WAFER_BATCH_TX, WAFER_BATCH_TY);
    }
    const int len = snprintf(buf, n, "stencil=%s kernel=%s steps_per_pass=%d tile=%s lds_bytes=%d remainder=%s variant=%d dtype=%s", stencils[R], kernel, K,
                             tile, K > 1 ? wafer_batch_stepk_lds_bytes(b->dtype, R, K) : 0, remainder, b->step_variant, DTYPE_NAMES[b->dtype]);
    if (b->mixed && len > 0 && (size_t)len < n) snprintf(buf + len, n - (size_t)len, " shapes=%zu", b->geoms.size());
    return WAFER_OK;
}

int wafer_batch_diag_passes(wafer_batch *b, uint64_t *fused_passes, uint64_t *single_steps)
{
    if (!b || !fused_passes || !single_steps) return fail(WAFER_ERR_INVALID, "null argument");
    *fused_passes = b->n_fused_passes;
    *single_steps = b->n_single_steps;
    return WAFER_OK;
}

int wafer_batch_set_gs_variant(wafer_batch *b, int variant)
{
    if (!b) return fail(WAFER_ERR_INVALID, "null batch");
    if (variant < -1 || variant > 1) return fail(WAFER_ERR_INVALID, "gs variant must be -1 (default), 0 (sequential) or 1 (one pass)");
    if (variant == 1) TRY(refuse_mixed(b, "wafer_batch_set_gs_variant"));
    b->gs_variant = variant;
    return WAFER_OK;
}

int wafer_batch_diag_gs(wafer_batch *b, uint32_t wnum, char *buf, size_t n)
{
    if (!b || !buf || n == 0) return fail(WAFER_ERR_INVALID, "null argument");
    const char *T = b->f32 ? "float" : "double";
    // what the one-pass form allocated on first use: the Gram matrices, their partials, the member lists, and the growth of gs_partials
    const size_t onepass_bytes = !b->onepass_ready ? 0
        : sizeof(double) * (WAFER_MAX_LOW * WAFER_MAX_LOW * (size_t)b->n + (size_t)b->gsp.doubles(WAFER_GRAM_PAIRS)) + sizeof(int) * 2 * b->n +
              sizeof(double) * (partials_doubles(b, WAFER_GS_ONE_ROWS) - partials_doubles(b, 1));
    char kernels[320];
    const char *GS = b->mixed_states ? ",WaferBatchGeomTable" : "";   // several shapes name the table-reading instantiations
    int launches = 1;
    const bool onepass = use_onepass(b, wnum);
    if (onepass) {
        launches = 4;
        snprintf(kernels, sizeof kernels, "wafer_k_batch_step+wafer_k_batch_gs_sums<%u,%s%s>+wafer_k_batch_gs_reduce_sums+wafer_k_batch_gs_apply<%u,%s,true%s>",
                 wnum, T, GS, wnum, T, GS);
    } else if (wnum) {
        launches = 1 + 2 * (1 + (int)wnum) + 1;
        snprintf(kernels, sizeof kernels, "wafer_k_batch_step+wafer_k_batch_gs<NORM2|SCALE|AXPY,%s%s>+wafer_k_batch_gs_reduce", T, GS);
    } else {
        snprintf(kernels, sizeof kernels, "wafer_k_batch_step");
    }
    const int len = snprintf(buf, n, "wnum=%u form=%s launches_per_step=%d kernels=%s variant=%d dtype=%s onepass_bytes=%zu", wnum,
                             onepass ? "onepass" : "sequential", launches, kernels, b->gs_variant, DTYPE_NAMES[b->dtype], onepass_bytes);
    if (b->mixed_states && len > 0 && (size_t)len < n) snprintf(buf + len, n - (size_t)len, " shapes=%zu", b->geoms.size());
    return WAFER_OK;
}

int wafer_batch_diag_gs_steps(wafer_batch *b, uint64_t *onepass, uint64_t *sequential)
{
    if (!b || !onepass || !sequential) return fail(WAFER_ERR_INVALID, "null argument");
    *onepass = b->n_onepass;
    *sequential = b->n_sequential;
    return WAFER_OK;
}
} // extern "C"

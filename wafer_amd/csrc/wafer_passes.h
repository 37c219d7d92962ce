// wafer_passes.h -- which pass of wafer_evolve comes next (plain C++, no HIP: tests/test_host_logic.py compiles it with g++).
//
// A call of wafer_evolve is a sequence of passes.  What the next pass is -- its kind, how many steps it advances, how many ghost
// planes it needs, computes and exchanges -- is decided here, from facts that are THE SAME ON EVERY RANK of a decomposed run:
// the ranks exchange K * ext planes per pass and queue hook calls on one communicator, so a decision taken here differently on
// two ranks would leave them waiting for each other.  WaferPassFacts therefore has no field for the local slab (its thickness,
// its first plane, which sides have a neighbour).  What may differ between ranks -- the boundary-first split, which depends on
// the thickness, and the sides a launch extends to -- is decided where a pass is launched (wafer_engine_schedules.hip).
#pragma once
#include <algorithm>
#include <cstdint>

enum WaferPassKind {
    WAFER_PASS_HALVES = 0,     // the whole slab in one launch, two halves marched outwards (schedule 2)
    WAFER_PASS_PEER,           // ... whose boundary workgroups store into the neighbours' ghost planes (schedule 3)
    WAFER_PASS_FUSED,          // K ground-state steps in one pass (K = 3 or 2)
    WAFER_PASS_STEP,           // one ground-state step
    WAFER_PASS_EXCITED,        // one excited-state step of the fused-overlap kernel (normalise and project on load)
    WAFER_PASS_EXCITED_ROWS,   // one excited-state step, then normalise and Gram-Schmidt as row operations
    WAFER_PASS_X2_TAIL         // every remaining excited-state step, two per pass (x2_run)
};

// what wafer_evolve knows that every rank knows
struct WaferPassFacts {
    uint32_t wnum = 0;            // stored states to project out (0: ground state)
    bool fuse2 = false;           // the two-step kernel applies (fuse2_applies)
    bool fuse3 = false;           // the three-step kernel applies (fuse3_applies)
    int R = 1, G = 1;             // stencil extent; ghost planes every context of the run was created with
    int halo_cycle = 1;           // fused passes per halo exchange (wafer_set_halo_cycle)
    int sched = 0;                // 0 exchange after the pass, 1 boundary-first split, 2 single-launch halves, 3 peer stores
    bool decomposed = false;      // the grid is cut into z-slabs at all
    bool x2 = false;              // the ranks agreed on two excited-state steps per pass (x2_agree)
    bool one_pass = true;         // WAFER_ONE_PASS: the raw result travels to the next excited-state step
    bool excited_fused = false;   // the fused-overlap excited-state kernel serves this wnum
};

struct WaferPass {
    bool drain_first = false;   // a single-launch sequence is in flight and this pass is of another kind: wait for the sequence's last
                                // exchanges (they leave `3 * R` ghost planes current), then ask again.  Nothing else below is set.
    int kind = WAFER_PASS_STEP;
    uint64_t steps = 0;         // time steps it advances (never 0)
    int need = 0;               // ghost planes that must be current before it; where fewer are, that many are exchanged first
                                // (within a single-launch sequence the sequence's own exchanges deliver them)
    bool rendezvous = false;    // ... exchanged even where they are current: the first peer pass of a call (see launch_single)
    int extend = 0;             // planes it computes beyond the owned range, towards every neighbour (deep halos)
    int exchange = 0;           // planes exchanged after it, per side (X2_TAIL: between its passes)
    int valid_after = 0;        // ghost planes known to be current on the main stream after it
    bool first = false;         // it starts / it ends the call (the one-pass excited-state scheme starts from identity scalars and
    bool last = false;          // materialises phi at the end)
};

// steps the head of a two-steps-per-pass call advances one per pass: whatever the caller hands over (a clone of a stored state, an
// un-normalised start) is normalised and projected by the reference's own sequence before the regrouped sums take over
static inline uint64_t wafer_x2_head(uint64_t steps) { return 2 + (steps & 1); }

static inline WaferPass wafer_drain_first()
{
    WaferPass p;
    p.drain_first = true;
    return p;
}

// The pass that follows `done` of `steps` steps (done < steps), with `valid` ghost planes current and, if `in_flight`, a
// single-launch sequence whose last exchanges the main stream has not waited for.
static inline WaferPass wafer_next_pass(const WaferPassFacts &f, uint64_t done, uint64_t steps, int valid, bool in_flight)
{
    WaferPass p;
    const uint64_t left = steps - done;
    const int R = f.R;
    p.first = done == 0;
    p.last = left == 1;
    if (f.wnum == 0 && ((f.fuse3 && left >= 3) || (f.fuse2 && left >= 2))) {
        // K time steps per pass: three on the three-step kernel while at least three remain, else two
        const int K = (f.fuse3 && left >= 3) ? 3 : 2, H = K * R;   // H: ghost planes one pass consumes per side
        // Deep halos: with E = H * halo_cycle ghost planes exchanged at once, only every halo_cycle-th pass needs an exchange (and
        // the boundary-first kernels and event hops around it).  The passes in between run over the owned planes plus the ghost
        // planes that are still good for one more pass: each fused pass consumes H planes of validity per side (the neighbour
        // computes the same cells from the same values, so the bits agree).  E is a whole number of passes' worth.
        const int E = f.decomposed ? std::max(H, std::min(f.G, H * f.halo_cycle) / H * H) : H;
        p.steps = (uint64_t)K;
        p.last = left == p.steps;
        // the whole slab in one launch: three-step passes with one exchange per pass
        if (f.decomposed && (f.sched == 2 || f.sched == 3) && K == 3 && E == H) {
            p.kind = f.sched == 3 ? WAFER_PASS_PEER : WAFER_PASS_HALVES;
            p.need = E;
            p.rendezvous = f.sched == 3 && !in_flight;
            p.exchange = E;
            p.valid_after = 0;   // (inside the sequence; the drain restores E)
            return p;
        }
        if (in_flight) return wafer_drain_first();
        p.kind = WAFER_PASS_FUSED;
        p.need = valid < H ? E : H;
        const int have = std::max(valid, p.need);
        if (f.decomposed && have >= 2 * H) {
            p.extend = have - H;   // ghost planes still valid after this pass
            p.valid_after = p.extend;
            return p;
        }
        p.exchange = f.decomposed ? E : 0;
        p.valid_after = E;
        return p;
    }
    if (in_flight) return wafer_drain_first();
    p.steps = 1;
    p.need = R;
    p.exchange = f.decomposed ? R : 0;
    p.valid_after = R;
    if (f.wnum == 0) {
        p.kind = WAFER_PASS_STEP;
    } else if (f.x2 && steps >= 4 && done == wafer_x2_head(steps)) {
        p.kind = WAFER_PASS_X2_TAIL;   // pairs of steps; phi is materialised after the last pass
        p.steps = left;
        p.last = true;
        p.need = 2;                    // a pass consumes two ghost planes per side
        p.exchange = f.decomposed ? 2 : 0;
        p.valid_after = 0;
    } else if (f.excited_fused) {
        p.kind = WAFER_PASS_EXCITED;
        // the last step of the one-pass scheme materialises phi and exchanges nothing (its planes travel on demand)
        if (f.one_pass && p.last) p.exchange = p.valid_after = 0;
    } else {
        p.kind = WAFER_PASS_EXCITED_ROWS;
    }
    return p;
}

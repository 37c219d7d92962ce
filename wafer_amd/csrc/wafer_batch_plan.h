// wafer_batch_plan.h -- the host-side plan of a batched ground-state evolve (wafer_engine_batch.hip): which passes a call of
// `steps` steps launches, the workgroup table of the one-step kernel (wafer_k_batch_step) and the one of the fused K-step pass
// (wafer_k_batch_stepk, wafer_stencil_batch.hip.h), the batch's layout (its distinct shapes, every member's offset), and every
// member's partition under the excited-state kernels with the places of its partials (wafer_batch_gs_partition).
// Plain C++ with no HIP in it, so the host compiler and the sanitizers can run it (tests/test_batch_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#if !defined(__HIPCC__) && !defined(__host__)   // wafer_geom.h marks its accessors for both sides; the host compiler has neither word
#define __host__
#define __device__
#endif
#include "wafer_geom.h"

// one workgroup of a batched step: tile (x0, y0) of work cells, local planes [z0, z1) of member `member`, whose geometry is
// entry `shape` of the batch's table of distinct geometries (0 in a batch of one shape)
struct WaferBatchBlock {
    int member, x0, y0, z0, z1, shape;
};

// the fused pass's tile of work cells: 64 columns (one wave across x) by 12 rows
#define WAFER_BATCHK_TX 64
#define WAFER_BATCHK_TY 12

// The fused pass's cell order.  Level k of a K-step pass is needed on the tile grown by (K-k) R cells on every side; the cells of
// the largest region (level 0: the tile grown by K R) are numbered so that EVERY level's region is a prefix: first the tile
// row by row, then ring after ring outwards (each R cells thick: R rows above, R rows below, then R columns left and right
// of the rows between).  Cell c -> its position (lx, ly) in the level-0 region, a (TX + 2 K R) x (TY + 2 K R) layout.
__host__ __device__ inline void wafer_batchk_cell(int R, int K, int c, int &lx, int &ly)
{
    const int TX = WAFER_BATCHK_TX, TY = WAFER_BATCHK_TY, H = K * R;
    lx = H + (c % TX);
    ly = H + (c / TX);
    if (c < TX * TY) return;
    for (int j = K - 1; j >= 0; --j) {   // the ring that makes level j's region out of level j+1's
        const int mj = (K - j) * R, Wj = TX + 2 * mj, Hj = TY + 2 * mj, inner = (Wj - 2 * R) * (Hj - 2 * R);
        if (c >= Wj * Hj) continue;
        int i = c - inner;
        const int o = H - mj;
        if (i < 2 * R * Wj) {
            const int row = i / Wj, col = i % Wj;
            lx = o + col;
            ly = o + (row < R ? row : Hj - 2 * R + row);
        } else {
            i -= 2 * R * Wj;
            const int row = i / (2 * R), k = i % (2 * R);
            lx = o + (k < R ? k : Wj - 2 * R + k);
            ly = o + R + row;
        }
        return;
    }
}

// ---- pass sequence ---------------------------------------------------------------------------------------------------------
// The next launch of a call with `remaining` > 0 steps to go advances this many steps: K while at least K remain (K > 1: the
// fused pass), then one two-step pass if that instantiation exists (have2) and two remain, then single steps.  Never 0, never
// more than `remaining`.
static inline int wafer_batch_next_pass(uint64_t remaining, int K, bool have2)
{
    if (K > 1 && remaining >= (uint64_t)K) return K;
    if (have2 && remaining >= 2) return 2;
    return 1;
}

// steps of every launch of a call of n_steps steps (a call of 0 steps takes one: grid.rs:682-685)
static inline std::vector<int> wafer_batch_pass_sequence(uint64_t n_steps, int K, bool have2)
{
    std::vector<int> seq;
    uint64_t left = n_steps == 0 ? 1 : n_steps;
    while (left > 0) {
        const int k = wafer_batch_next_pass(left, K, have2);
        seq.push_back(k);
        left -= (uint64_t)k;
    }
    return seq;
}

// launches of that call, in closed form: the source buffer flips once per launch, so every active member's `cur` flips iff
// this is odd.  fused (may be null): how many of them advance more than one step.
static inline uint64_t wafer_batch_launch_count(uint64_t n_steps, int K, bool have2, uint64_t *fused)
{
    const uint64_t steps = n_steps == 0 ? 1 : n_steps;
    uint64_t nf = K > 1 ? steps / (uint64_t)K : 0;
    uint64_t rem = K > 1 ? steps % (uint64_t)K : steps;
    uint64_t n = nf;
    if (have2) {   // (K == 2: rem < 2 here; K == 1: every pair of steps is a two-step pass)
        nf += rem / 2;
        n += rem / 2;
        rem %= 2;
    }
    if (fused) *fused = nf;
    return n + rem;
}

// ---- the fused pass's z-chunks -----------------------------------------------------------------------------------------------
// Their number.  A chunk of L planes computes K L + R K (K-1) level-planes for K L useful ones, so the recomputed share
// is R (K-1) / (L + R (K-1)).  Rule: cut z so that the active members together give about two workgroups per CU (what a CU
// holds of this kernel, by LDS and by VGPRs), but no chunk shorter than 4 R (K-1) planes: the recomputed share stays <= 1/5,
// and it gets that high only where the device would otherwise stand partly idle.  A grid thinner than that is one chunk.
// The planes are shared out evenly (chunk i is [i nzl / n, (i+1) nzl / n)), so no chunk is a short remainder.
static inline int wafer_batch_fused_nchunks(int nzl, long long layer, int num_cus, int R, int K)
{
    const int min_chunk = 4 * R * (K - 1) > 1 ? 4 * R * (K - 1) : 1;
    const long long target = 2LL * (num_cus > 0 ? num_cus : 1);
    long long nch = layer > 0 ? (target + layer - 1) / layer : 1;
    const long long most = nzl / min_chunk > 1 ? nzl / min_chunk : 1;
    if (nch > most) nch = most;
    if (nch < 1) nch = 1;
    return (int)nch;
}

// ---- the workgroup tables ----------------------------------------------------------------------------------------------------
// A batch keeps a table of its distinct geometries (one entry in a batch of one shape); shape_of[m] is member m's entry.  Both
// tables below cut z by ONE layer for the whole launch: layer = sum over the active members of that member's tiles per plane, so
// the launch as a whole fills the device whatever mix of shapes is active.  An entry carries its member's shape index.

static inline long long wafer_batch_layer(const WaferGeom *geoms, const int *shape_of, const uint8_t *active, uint32_t n_members, int tx, int ty)
{
    long long layer = 0;
    for (uint32_t m = 0; m < n_members; ++m) {
        if (active && !active[m]) continue;
        const WaferGeom &g = geoms[shape_of[m]];
        layer += (long long)((g.nx + tx - 1) / tx) * ((g.ny + ty - 1) / ty);
    }
    return layer;
}

// The one-step kernel's table: tx x ty tiles (64 x 4) of every active member's work area, z cut into chunks so that the active
// members together give ~8 workgroups per CU (a CU holds 8 of these 256-thread workgroups), no chunk shorter than 8 planes:
//   nch_m = clamp(ceil(8 CUs / layer), 1, (nz_m + 7) / 8),  zchunk_m = ceil(nz_m / nch_m).
// Members in order, within a member z-chunks, tile rows, tiles.  A frozen member has no entry.
static inline std::vector<WaferBatchBlock> wafer_batch_step_table(const WaferGeom *geoms, const int *shape_of, const uint8_t *active,
                                                                  uint32_t n_members, int num_cus, int tx, int ty)
{
    std::vector<WaferBatchBlock> t;
    const long long layer = wafer_batch_layer(geoms, shape_of, active, n_members, tx, ty);
    const long long target = 8LL * num_cus;
    for (uint32_t m = 0; m < n_members; ++m) {
        if (active && !active[m]) continue;
        const int sh = shape_of[m];
        const WaferGeom &g = geoms[sh];
        const int ntx = (g.nx + tx - 1) / tx, nty = (g.ny + ty - 1) / ty;
        long long nch = layer > 0 ? (target + layer - 1) / layer : 1;
        const long long most = (long long)(g.nzl + 7) / 8;
        if (nch > most) nch = most;
        if (nch < 1) nch = 1;
        const int zchunk = (int)((g.nzl + nch - 1) / nch);
        for (int z0 = g.G; z0 < g.G + g.nzl; z0 += zchunk)
            for (int j = 0; j < nty; ++j)
                for (int i = 0; i < ntx; ++i)
                    t.push_back(WaferBatchBlock{(int)m, i * tx, j * ty, z0, z0 + zchunk < g.G + g.nzl ? z0 + zchunk : g.G + g.nzl, sh});
    }
    return t;
}

// The fused pass's table: a pure function of the geometries, the active set (null: all of n_members), the CU count and the tile.
// wafer_batch_fused_nchunks's rule with the summed layer, every member's planes shared out evenly over its own
// wafer_batch_fused_nchunks(nz_m, layer, ...) chunks.  Members in order, within a member z-chunks, tile rows, tiles: the
// workgroups of one member are neighbours in the dispatch order and share its halo planes in L2.  A frozen member has no entry.
static inline std::vector<WaferBatchBlock> wafer_batch_fused_table(const WaferGeom *geoms, const int *shape_of, const uint8_t *active,
                                                                   uint32_t n_members, int num_cus, int K, int tx, int ty)
{
    std::vector<WaferBatchBlock> t;
    const long long layer = wafer_batch_layer(geoms, shape_of, active, n_members, tx, ty);
    for (uint32_t m = 0; m < n_members; ++m) {
        if (active && !active[m]) continue;
        const int sh = shape_of[m];
        const WaferGeom &g = geoms[sh];
        if (g.nzl < 1) continue;
        const int ntx = (g.nx + tx - 1) / tx, nty = (g.ny + ty - 1) / ty;
        const int nch = wafer_batch_fused_nchunks(g.nzl, layer, num_cus, g.R, K);
        for (int c = 0; c < nch; ++c) {
            const int z0 = g.G + (int)((long long)c * g.nzl / nch), z1 = g.G + (int)((long long)(c + 1) * g.nzl / nch);
            for (int j = 0; j < nty; ++j)
                for (int i = 0; i < ntx; ++i) t.push_back(WaferBatchBlock{(int)m, i * tx, j * ty, z0, z1, sh});
        }
    }
    return t;
}

// ---- stepping the state stores (wafer_batch_evolve_states, wafer_store_step_batch.hip.h) --------------------------------------
// A workgroup of wafer_k_batch_store_step steps up to WAFER_STORE_SG states of its tile; the grid's second extent is the number of
// such groups the largest listed k needs.
#define WAFER_STORE_SG 4
static inline int wafer_batch_store_groups(uint32_t max_k) { return (int)((max_k + WAFER_STORE_SG - 1) / WAFER_STORE_SG); }

// A call of n_steps steps (0 takes one): step s reads the slots when s is even and their shadows when it is odd, and writes the
// other set, so after an odd number of steps the results stand in the shadows and ONE batched copy of the listed members' states
// brings them back (copy_back) -- a trailing copy, never a leading one.  launches: steps, or steps + 1, whatever the batch holds;
// 0 where no listed member has k > 0 (max_k == 0).
struct WaferBatchStorePlan {
    uint64_t steps = 0, launches = 0;
    int groups = 0;
    bool copy_back = false;
};
static inline bool wafer_batch_store_src_is_shadow(uint64_t s) { return (s & 1) != 0; }
static inline WaferBatchStorePlan wafer_batch_store_plan(uint64_t n_steps, uint32_t max_k)
{
    WaferBatchStorePlan p;
    p.steps = n_steps == 0 ? 1 : n_steps;
    p.groups = wafer_batch_store_groups(max_k);
    if (max_k == 0) return p;
    p.copy_back = (p.steps & 1) != 0;
    p.launches = p.steps + (p.copy_back ? 1 : 0);
    return p;
}

// ---- filtering the state stores (wafer_batch_filter_states, wafer_store_filter_batch.hip.h; wafer_filter_states) ---------------
// The launches of a call of `degree` >= 1 steps on slots and shadow slots (the context's one shadow array alike): step 1 reads the
// slots and writes the shadows; step i >= 2 reads the set step i - 1 wrote and writes its result over the iterate before last, in
// place, which lies in the other set.  So step i = 1 .. degree reads what step i - 1 of the store plan reads, and the call is the
// store plan of `degree` steps: after an odd degree the result stands in the shadows and one trailing copy brings it back (a batch),
// or the two pointers change places (a context).
using WaferBatchFilterPlan = WaferBatchStorePlan;
static inline bool wafer_batch_filter_src_is_shadow(uint64_t i) { return wafer_batch_store_src_is_shadow(i - 1); }
static inline WaferBatchFilterPlan wafer_batch_filter_plan(uint32_t degree, uint32_t max_k) { return wafer_batch_store_plan(degree, max_k); }

// ---- the batch's layout ------------------------------------------------------------------------------------------------------
// The distinct geometries of the members' shapes (nxyz: nx, ny, nz of member m at [3 m ..]) in order of first appearance, each the
// one a context of that shape builds (ghost depth G, elements of esz bytes); shape_of[m]: member m's entry; off[m]: its element
// offset in each array allocation = the sum of the padded totals of the members before it (one shape: m * geoms[0].total);
// cells: the sum over all members.  overflow: cells, or cells * esz, passed the size of one allocation at member off.size() - 1,
// where the walk stopped.  misaligned: a member's span does not start or end on 16 bytes (the batched rotation of stored states walks
// every span in whole 16-byte vectors, wafer_ritz_batch.hip.h); wafer_make_geom's pitch of whole 128-byte lines rules it out for
// 4- and 8-byte elements alike, and creation fails loudly if that ever changes.
struct WaferBatchLayout {
    std::vector<WaferGeom> geoms;
    std::vector<int> shape_of;
    std::vector<size_t> off;
    size_t cells = 0;
    bool overflow = false;
    bool misaligned = false;
};

static inline WaferBatchLayout wafer_batch_layout(const int *nxyz, uint32_t n_members, int R, int G, size_t esz)
{
    WaferBatchLayout L;
    for (uint32_t m = 0; m < n_members && !L.overflow; ++m) {
        const int nx = nxyz[3 * m], ny = nxyz[3 * m + 1], nz = nxyz[3 * m + 2];
        size_t k = 0, bytes = 0;
        while (k < L.geoms.size() && !(L.geoms[k].nx == nx && L.geoms[k].ny == ny && L.geoms[k].nz == nz)) ++k;
        if (k == L.geoms.size()) L.geoms.push_back(wafer_make_geom(nx, ny, nz, R, G, 0, nz, (int)esz));
        L.shape_of.push_back((int)k);
        L.off.push_back(L.cells);
        L.overflow = __builtin_add_overflow(L.cells, (size_t)L.geoms[k].total, &L.cells) || __builtin_mul_overflow(L.cells, esz, &bytes);
        if (!L.overflow && ((L.off.back() * esz) % 16 != 0 || bytes % 16 != 0)) L.misaligned = true;
    }
    return L;
}

// ---- the Gram-Schmidt partition ----------------------------------------------------------------------------------------------
// Workgroups of a member under the excited-state kernels (wafer_gs_batch.hip.h): tiles of tx x ty work cells (64 x 4), chunks of zc
// planes (WAFER_GS_ZC).  Fixed by the shape alone.
static inline int wafer_gs_blocks_of(const WaferGeom &g, int tx, int ty, int zc)
{
    return ((g.nx + tx - 1) / tx) * ((g.ny + ty - 1) / ty) * ((g.nzl + zc - 1) / zc);
}

// Every member's partition of the excited-state kernels and the places of its partials, one shape or several.  A kernel that
// writes `rows` sums per workgroup (1: the chain; WAFER_GS_ONE_ROWS: the one-pass form's sums; WAFER_GRAM_PAIRS: the Gram kernel)
// keeps member m's rows end to end from row_off(m, rows) on: row q, workgroup w at row_off(m, rows) + q * nb[m] + w.  first[m] is
// the sum of nb over the members before m, so no two members' rows overlap whatever `rows`, and with one shape the layout is
// the one the one-shape kernels index: row_off(m, rows) == m * rows * nb.
struct WaferBatchGsPartition {
    std::vector<int> nb;            // member m's workgroups: wafer_gs_blocks_of its shape
    std::vector<long long> first;   // the workgroups of the members before it
    long long blocks = 0;           // of all members
    int max_nb = 0;                 // the widest member's
    long long row_off(uint32_t m, int rows) const { return first[m] * rows; }
    long long doubles(int rows) const { return blocks * rows; }   // the whole partials buffer of such a kernel
};

static inline WaferBatchGsPartition wafer_batch_gs_partition(const WaferGeom *geoms, const int *shape_of, uint32_t n_members, int tx, int ty, int zc)
{
    WaferBatchGsPartition P;
    for (uint32_t m = 0; m < n_members; ++m) {
        const int nb = wafer_gs_blocks_of(geoms[shape_of[m]], tx, ty, zc);
        P.nb.push_back(nb);
        P.first.push_back(P.blocks);
        P.blocks += nb;
        if (nb > P.max_nb) P.max_nb = nb;
    }
    return P;
}

// wafer_engine_batch.h -- what the two units of the batch engine share: the batch itself, the engine's memory and copy policies with
// the holders on them (wafer_buffers.h), the dtype name tables, and the helpers that wafer_engine_batch.hip defines and
// wafer_engine_batch_stores.hip calls too (namespace wafer_eng, hidden from the library's dynamic symbols, as wafer_engine.h's).
// The kernel headers are here for the records and argument structs the batch holds; neither unit instantiates a kernel of theirs.
#pragma once
#include "wafer_engine.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_setup_batch.hip.h"
#include "wafer_ritz_batch.hip.h"
#include "wafer_residual_batch.hip.h"
#include "wafer_moments_batch.hip.h"
#include "wafer_filter.h"
#include "wafer_buffers.h"

// the engine's two memory policies and its copy policy (wafer_buffers.h), the holders on them, and a holder's status through HIP_TRY
struct DeviceMem {
    static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static int alloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
};
struct StreamCopy {
    using stream = hipStream_t;
    static int copy(void *dst, const void *src, size_t n, bool up, stream s) { return (int)hipMemcpyAsync(dst, src, n, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, s); }
};
template <typename T> using DevArray = Array<T, DeviceMem>;
template <typename T> using DevGrow = GrowArray<T, DeviceMem>;
template <typename T> using Mirror = HostDev<T, DeviceMem, PinnedMem, StreamCopy>;
#define BUF_TRY(expr) HIP_TRY((hipError_t)(expr))
// by dtype: its name in the diag_* strings, and the kernels' <.., T, C>
constexpr const char *DTYPE_NAMES[] = {"f64", "f32", "f32fast"};
constexpr const char *KERNEL_TYPES[] = {"double,double", "float,double", "float,float"};

struct wafer_batch {
    // The stream, declared first: it goes last, behind every buffer.
    struct Stream {
        hipStream_t h = nullptr;
        Stream() = default;
        Stream(const Stream &) = delete;
        ~Stream()
        {
            if (h) (void)hipStreamDestroy(h);
        }
        operator hipStream_t() const { return h; }
    } s;
    uint32_t n = 0;
    std::vector<wafer_params> P;
    int device = 0, num_cus = 256;
    WaferTuning tune;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // the layout (wafer_batch_layout): the distinct geometries in order of first appearance.  mixed: more than one
    std::vector<WaferGeom> geoms;
    std::vector<int> shape_of;                // member m's entry in geoms
    std::vector<size_t> off;                  // member m's element offset in each array allocation
    size_t cells = 0;                         // elements of each array allocation: every member's total, end to end
    DevArray<WaferGeom> geoms_dev;
    bool mixed = false;
    bool mixed_states = false;                // several shapes WITH state stores (wafer_batch_create_mixed_states)
    WaferBatchGsPartition gsp;                // every member's Gram-Schmidt partition and the places of its partials
    size_t n2_doubles = 0;                    // every member's wafer_batch_norm2 partials (mem[].n2_nb), end to end
    const WaferGeom &g() const { return geoms[0]; }               // what every shape shares (R, G), and THE geometry of one shape
    const WaferGeom &geom(uint32_t m) const { return geoms[shape_of[m]]; }
    std::string kernel_name = "wafer_k_batch_step";
    int dtype = WAFER_F64;                    // every member's (check_member)
    bool f32 = false;                         // float storage (f32 and f32fast)
    size_t esz = 8;                           // bytes per element of every array and store slot
    DevArray<char> alloc[4];                  // phi[0], phi[1], V, pot_sub: cells * esz bytes each
    std::vector<wafer_ctx *> views;
    Mirror<double> view_scal;                 // SCAL_SLOTS per view
    // device tables
    std::vector<WaferBatchMember> mem;
    DevArray<WaferBatchMember> mem_dev;
    // a workgroup table on the device, with the active set and the steps per pass it was built for
    struct BlockTable {
        std::vector<WaferBatchBlock> host;
        DevGrow<WaferBatchBlock> dev;
        std::vector<uint8_t> key;
        int K = 0;
    };
    BlockTable blk, blkk;                     // the one-step kernel's, and the fused pass's (wafer_k_batch_stepk) for the same active set
    BlockTable blks;                          // the store step's (wafer_k_batch_store_step): the one-step table over the listed members with k > 0
    int step_variant = -1;                    // wafer_batch_set_step_variant
    uint64_t n_fused_passes = 0, n_single_steps = 0;   // launches since creation (wafer_batch_diag_passes)
    Mirror<int> act;
    Mirror<int> sym;                          // [member]: the constraints of the last wafer_batch_symmetrise
    // observables: every member on the single context's partition of its shape (mem[].obs_*)
    int swz = 0;
    DevArray<double> partials;                // member m's [4][obs_nb] at mem[m].obs_off
    Mirror<double> sums;                      // [member][4]
    Mirror<double> n2;                        // [member]
    uint64_t last_steps = 0;
    bool timing_valid = false;
    // w_store: slot l of every member in one allocation laid out as the arrays are, made by the first push or load that needs it
    std::vector<DevArray<char>> slots;
    std::vector<uint32_t> nst;                // states member m holds
    // excited states: norm2 at gs_scal[m * gs_stride], the overlap with state l at [m * gs_stride + 1 + l]; made at first use
    int gs_stride = 0;
    DevGrow<double> gs_partials;              // member m's rows at gsp.row_off(m, rows); wafer_batch_norm2's at mem[m].n2_off (partials_doubles)
    Mirror<double> gs_scal;
    // the one-pass form (wafer_batch_set_gs_variant); everything below is made by its first use (ensure_onepass)
    int gs_variant = -1;
    uint64_t n_onepass = 0, n_sequential = 0;   // excited steps and orthogonalise calls in each form (wafer_batch_diag_gs_steps)
    bool onepass_ready = false;               // gs_partials holds WAFER_GS_ONE_ROWS rows per member, the Gram storage exists
    DevArray<double> gram;                    // [member][WAFER_MAX_LOW^2]: G_ji = <state j | state i>, i < j
    DevArray<double> gram_partials;           // member m's [WAFER_GRAM_PAIRS][gsp.nb[m]] at gsp.row_off(m, WAFER_GRAM_PAIRS)
    Mirror<int> gram_list;                    // the members to recompute, then their state counts: 2 n ints
    std::vector<uint8_t> gram_stale;          // member m's store changed since its Gram matrix was formed
    // wafer_batch_resample: a host source as uploaded ([sx][sy][sz]) and, behind it, transposed to x-fastest; grown on demand
    DevGrow<double> rs_scratch;
    hipEvent_t rs_start = nullptr, rs_stop = nullptr;   // around the last call's upload, transpose and launch (wafer_batch_last_resample_ms)
    bool rs_timing_valid = false;
    // batched set-up (wafer_setup_batch.hip.h): one record per listed member, and the range check's three words per listed member --
    // on the device, their start values (~0, 0, 0) and the read-back, pinned; all n entries long, made at creation
    Mirror<WaferBatchSetupRec> setup;
    Mirror<unsigned long long> vchk;
    Array<unsigned long long, PinnedMem> vchk_init;
    uint64_t n_setup_launches = 0, n_setup_readbacks = 0;   // of the batched set-up paths since creation (wafer_batch_diag_setup_counts)
    // Rayleigh-Ritz on the stores (wafer_ritz_batch.hip.h); everything below is made by the first call (ensure_ritz)
    Mirror<WaferBatchRitzRec> ritz_rec;       // the per-call table, n entries
    DevGrow<double> ritz_partials;            // the listed members' 2 k^2 rows of obs_nb partials end to end; grown on demand
    Mirror<double> ritz_sums;                 // [member][2][WAFER_RITZ_MAX^2]
    Mirror<double> ritz_coef;                 // [member][WAFER_RITZ_MAX^2]
    uint64_t n_ritz_launches = 0, n_ritz_readbacks = 0;       // of the three calls since creation (wafer_batch_diag_ritz_counts)
    // residuals (wafer_residual_batch.hip.h); made by the first call (ensure_residual).  The partials live in ritz_partials.
    Mirror<WaferBatchResidualRec> resid_rec;  // the per-call table, n entries
    Mirror<double> resid_sums;                // [member][3 WAFER_RITZ_MAX]: r2, wh, s of column j at j * 3
    uint64_t n_resid_launches = 0, n_resid_readbacks = 0;     // of wafer_batch_residuals since creation (wafer_batch_diag_residual_counts)
    // moment matrices (wafer_moments_batch.hip.h); made by the first call (ensure_moments).  The partials live in ritz_partials.
    Mirror<WaferBatchMomentRec> moment_rec;   // the per-call table, n entries
    Mirror<double> moment_sums;               // [member][WAFER_MOMENT_COUNT * WAFER_RITZ_MAX^2]: the member's 5 k (k + 1) / 2 computed rows first
    uint64_t n_moment_launches = 0, n_moment_readbacks = 0;   // of wafer_batch_moment_matrices since creation (wafer_batch_diag_moment_counts)
    // stepping the stores (wafer_store_step_batch.hip.h): shadow l is laid out as slot l is, zeroed, made by the first call that needs it
    std::vector<DevArray<char>> shadows;
    Mirror<int> store_k;                      // [member]: the call's k (0: not listed)
    uint64_t n_store_launches = 0;                            // of wafer_batch_evolve_states since creation (wafer_batch_diag_store_counts)
    // filtering the stores (wafer_store_filter_batch.hip.h), made by the first call: every step's al, be, cc of every member, step i's
    // at (i - 1) * n; and the spectral bound's one word per listed member with its pinned zeros
    Mirror<WaferFilterCoef> filt_coef;
    Mirror<unsigned long long> vmax;
    uint64_t n_filter_launches = 0, n_bound_launches = 0;     // of wafer_batch_filter_states / wafer_batch_spectral_bound since creation
    // Lets a batch go: the stream drains, the views go -- they borrow every array and the stream, except a and b (ensure_ab) -- then
    // the events; behind this body every holder frees its block, and the stream goes last.
    ~wafer_batch()
    {
        (void)hipSetDevice(device);
        if (s) (void)hipStreamSynchronize(s);
        for (wafer_ctx *v : views) {
            for (void *p : {v->a, v->b})
                if (p) (void)hipFree(alloc_base(v, p));
            delete v;
        }
        for (hipEvent_t e : {ev_start, ev_stop, rs_start, rs_stop})
            if (e) (void)hipEventDestroy(e);
    }
};

namespace wafer_eng __attribute__((visibility("hidden"))) {
// ---- wafer_engine_batch.hip (described where they are defined)
int check_member_index(const wafer_batch *b, uint32_t m);
int refuse_mixed(const wafer_batch *b, const char *call);
int sync_members(wafer_batch *b);
int upload_active(wafer_batch *b, const uint8_t *active, int *nact);
int build_blocks(wafer_batch *b, wafer_batch::BlockTable &t, const uint8_t *active, int K);
int launched(const char *what, hipError_t e);
void max_tiles_planes(const wafer_batch *b, int nact, bool padded, int *max_tiles, int *max_planes);
void *slot_ptr(const wafer_batch *b, uint32_t l, uint32_t m);
int ensure_slots(wafer_batch *b, std::vector<DevArray<char>> &v, uint32_t n);
void mark_gram_stale(wafer_batch *b, uint32_t m);

// The one place that chooses where the kernels read the geometry from: launch(gs) with the batch's one geometry (a kernel
// argument) or with its device table of several.  Every wafer_entry_batch_* entry point has an overload for either.
template <typename F>
hipError_t with_geom(const wafer_batch *b, F &&launch)
{
    return b->mixed ? launch(WaferBatchGeomTable{b->geoms_dev}) : launch(b->g());
}

template <typename F>
int launch(const wafer_batch *b, const char *what, F &&f) { return launched(what, with_geom(b, f)); }
} // namespace wafer_eng

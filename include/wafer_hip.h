/*
 * wafer_hip.h -- C ABI of the MI355X engine for Wafer's grid::evolve hot path.
 *
 * Wafer (Rust, /src/grid.rs) has no FFI or plugin interface: `grid` is a
 * private module and evolve/compute_observables/... are private fns.  The
 * boundary is therefore defined by their signatures.
 * Each entry point below names the reference item it replaces.  A Rust host
 * binds these with a plain `extern "C"` block (INTEGRATION.md shows it and
 * the four call sites in grid.rs that change).
 *
 * Conventions
 *  - Every function returns WAFER_OK (0) or a negative wafer_status;
 *    wafer_last_error() gives the message for the calling thread.  (The
 *    reference's fns are infallible and panic; its callers use error_chain
 *    Result<()>, errors.rs -- a host maps non-zero to an ErrorKind.)
 *  - One caller thread per context, non-reentrant (the reference calls these
 *    from its main thread only; parallelism is internal, main.rs:190-196).
 *  - Host arrays are ALWAYS double, C-order [x][y][z] (z contiguous), shape
 *    (nx+2e, ny+2e, nz+2e) with e = ext: exactly ndarray's Array3<R64>
 *    standard layout as the reference holds it (config.rs:224-238), so
 *    `arr.as_ptr()` can be passed straight through.  They describe the GLOBAL
 *    grid even when the context owns only a z-slab of it.
 *  - Device state (phi, V, a, b, pot_sub, w_store) stays resident in HBM
 *    between calls; only wafer_observables, norm2, download and last_evolve_ms block the host.
 */
#ifndef WAFER_HIP_H
#define WAFER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAFER_ABI_VERSION 1

typedef enum wafer_status {
    WAFER_OK = 0,
    WAFER_ERR_INVALID = -1,      /* bad argument / config (cf. ErrorKind::LargeDt, LargeWavenum) */
    WAFER_ERR_HIP = -2,          /* a HIP runtime call failed */
    WAFER_ERR_NOT_AVAILABLE = -3,/* ErrorKind::PotentialNotAvailable (potential.rs:315-317) */
    WAFER_ERR_STATE = -4,        /* w_store too short / full, potential or phi not set */
    WAFER_ERR_MAX_STEP = -5,     /* ErrorKind::MaxStep (grid.rs:244, errors.rs:111-114) */
    WAFER_ERR_COMM = -6          /* a communication hook failed */
} wafer_status;

/* config.rs:73-104, same order */
typedef enum wafer_potential {
    WAFER_POT_NOPOTENTIAL = 0,
    WAFER_POT_CUBE,
    WAFER_POT_QUADWELL,
    WAFER_POT_PERIODIC,
    WAFER_POT_COULOMB,
    WAFER_POT_COMPLEXCOULOMB,
    WAFER_POT_ELIPTICALCOULOMB,
    WAFER_POT_SIMPLECORNELL,
    WAFER_POT_FULLCORNELL,
    WAFER_POT_HARMONIC,
    WAFER_POT_COMPLEXHARMONIC,
    WAFER_POT_DODECAHEDRON,
    WAFER_POT_FROMFILE,
    WAFER_POT_FROMSCRIPT
} wafer_potential;

/* config.rs:151-170, same order */
typedef enum wafer_initial_condition {
    WAFER_IC_FROMFILE = 0,
    WAFER_IC_GAUSSIAN,
    WAFER_IC_COULOMB,
    WAFER_IC_CONSTANT,
    WAFER_IC_BOOLEAN
} wafer_initial_condition;

/* config.rs:211-239: the value is CentralDifference::ext() */
typedef enum wafer_central_difference {
    WAFER_CD_THREEPOINT = 1,
    WAFER_CD_FIVEPOINT = 2,
    WAFER_CD_SEVENPOINT = 3
} wafer_central_difference;

/* WAFER_F64: the reference's arithmetic.  WAFER_F32: fp32 STORAGE of every array, arithmetic still
 * fp64 in registers (only storage rounding is added).  WAFER_F32_FAST: the ground-state stencil
 * steps also compute in fp32 (1.5x the fp64 step rate, on the three-step kernel; sums, projections and observables stay fp64) --
 * the throughput setting of BASELINE config #5, to be cross-checked against fp64 as that config
 * prescribes. */
typedef enum wafer_dtype { WAFER_F64 = 0, WAFER_F32 = 1, WAFER_F32_FAST = 2 } wafer_dtype;

/* pot_sub: (Option<Array3<R64>>, Option<R64>) of potential.rs:24 */
typedef enum wafer_potsub_kind { WAFER_POTSUB_NONE = 0, WAFER_POTSUB_SCALAR = 1, WAFER_POTSUB_ARRAY = 2 } wafer_potsub_kind;

typedef enum wafer_array_id { WAFER_ARRAY_V = 0, WAFER_ARRAY_A = 1, WAFER_ARRAY_B = 2, WAFER_ARRAY_POTSUB = 3 } wafer_array_id;

/* The subset of Config (config.rs:292-333) the hot path reads, plus the
 * engine's own knobs.  Zero-initialise, then set struct_size = sizeof. */
typedef struct wafer_params {
    uint32_t struct_size;
    uint32_t nx, ny, nz;          /* config.grid.size: GLOBAL work area */
    int32_t central_difference;   /* wafer_central_difference */
    int32_t dtype;                /* wafer_dtype: storage + arithmetic type on the device */
    double dn, dt;                /* config.grid.dn / dt */
    double mass;                  /* config.mass */
    double sig;                   /* config.sig */
    uint32_t max_states;          /* capacity of the device-resident w_store (>= wavemax) */
    int32_t device;               /* HIP device ordinal */
    /* z-slab owned by this context: work planes [z_begin, z_begin+z_count) of
     * the global grid; z_count == 0 means the whole grid.  halo_depth = ghost
     * planes kept on each z side (0 -> ext). */
    uint32_t z_begin, z_count;
    uint32_t halo_depth;
    uint32_t flags;               /* WAFER_FLAG_* */
} wafer_params;

#define WAFER_FLAG_SKIP_DT_CHECK 1u /* do not enforce dt <= dn^2/3 (config.rs:362-365) */
#define WAFER_FLAG_UNPLANNED_DIV 2u /* ignore the verdict of the division plan (wafer_div_plan): every x / (c dn^2 m) of the step
                                     * kernels takes the extra Markstein round, as for a denominator the plan could not clear */

/* grid.rs:17-28, un-normalised, in this order */
typedef struct wafer_observables_t {
    double energy, norm2, v_infinity, r2;
} wafer_observables_t;

/* One row of the convergence table solve() prints (grid.rs:126-221,
 * output.rs:497-521): raw observables at `step`, diff = |E - E_last|. */
typedef struct wafer_block_record {
    uint64_t step;
    double tau;
    wafer_observables_t obs;
    double diff;
} wafer_block_record;

/* output.rs:32-45, 540-547 */
typedef struct wafer_observables_output {
    uint32_t state;
    double energy, binding_energy, r, l_r;
} wafer_observables_output;

typedef struct wafer_ctx wafer_ctx;

/* ---- diagnostics ------------------------------------------------------- */
int wafer_abi_version(void);
const char *wafer_last_error(void);

/* ---- lifetime: replaces the allocations of grid.rs:32-34, 560; potential.rs:101-102 */
int wafer_ctx_create(const wafer_params *params, wafer_ctx **out);
int wafer_ctx_destroy(wafer_ctx *ctx);
int wafer_synchronize(wafer_ctx *ctx);

/* ---- Potentials {v, a, b, pot_sub} (potential.rs:16-25) ----------------- */
/* potential::generate + a/b + pot_sub, on the device (potential.rs:46-62, 101-110, 134-153) */
int wafer_set_potential_builtin(wafer_ctx *ctx, int potential);
/* FromFile / FromScript: v is the padded global array; potsub is NULL, or the
 * UNPADDED nx*ny*nz array when potsub_kind == WAFER_POTSUB_ARRAY */
int wafer_set_potential_host(wafer_ctx *ctx, const double *v, int potsub_kind, double potsub_scalar, const double *potsub);
/* tests / output::potential: padded global array out (POTSUB: unpadded) */
int wafer_download_array(wafer_ctx *ctx, int array_id, double *out);
int wafer_get_potsub(wafer_ctx *ctx, int *kind, double *scalar);
/* replaces pot_sub after the potential has been set: a potential_sub file in ./input takes
 * precedence over the computed value for every potential type (potential.rs:113-131).  potsub is
 * the UNPADDED nx*ny*nz array when kind == WAFER_POTSUB_ARRAY, else ignored. */
int wafer_set_potsub(wafer_ctx *ctx, int kind, double scalar, const double *potsub);
/* the same override from a potential_sub array of another resolution: input::fill_sub_data
 * (input.rs:453-478) resamples it with trilerp_resize onto the work area, basis = (nx, ny, nz).
 * src is an UNPADDED [sx][sy][sz] array. */
int wafer_set_potsub_resampled(wafer_ctx *ctx, const double *src, uint32_t sx, uint32_t sy, uint32_t sz);

/* ---- phi: config::set_initial_conditions (config.rs:577-627), input::wavefunction, output::wavefunction */
int wafer_set_initial_condition(wafer_ctx *ctx, int ic, uint64_t seed);
int wafer_upload_phi(wafer_ctx *ctx, const double *phi);
int wafer_download_phi(wafer_ctx *ctx, double *phi);
/* the work cells of the planes this context OWNS, [nx][ny][z_count] in the reference's axis order
 * (z_count = nz without a slab): what a rank of a decomposed run saves -- its host buffer is the size
 * of its slab, not of the grid */
int wafer_download_phi_owned(wafer_ctx *ctx, double *out);
/* Restart from another resolution: input::fill_data / read_csv's resampling branch with
 * trilerp_resize (input.rs:149-176, 640-656, 667-716).  src is an UNPADDED [sx][sy][sz] array;
 * basis = the `size` the reference builds its linspace from (NULL = the padded target size, which
 * is what the reference's production call passes; its unit test passes the work-area dims). */
int wafer_upload_phi_resampled(wafer_ctx *ctx, const double *src, uint32_t sx, uint32_t sy, uint32_t sz,
                               const uint32_t *basis);
int wafer_set_potential_resampled(wafer_ctx *ctx, const double *src, uint32_t sx, uint32_t sy, uint32_t sz,
                                  const uint32_t *basis);

/* config::symmetrise_wavefunction (config.rs:691-728), applied by the reference to the initial
 * condition (config.rs:625) and to snapshots (grid.rs:138).  Constraint in the order of
 * SymmetryConstraint (config.rs:184-197).  The reference indexes the SevenPoint frame literally
 * (offset 3, extent n + 6) and would run out of bounds on a narrower one: any constraint other
 * than NOT_CONSTRAINED returns WAFER_ERR_INVALID unless central_difference is SevenPoint.  Its
 * quirks are kept: the mirror plane sits half a cell below the centre of the work area and the
 * last work cell along the axis takes the frame's zero.  About z is not available on z-slabs. */
typedef enum wafer_symmetry {
    WAFER_SYM_NOT_CONSTRAINED = 0,
    WAFER_SYM_ABOUT_Z,
    WAFER_SYM_ANTISYM_ABOUT_Z,
    WAFER_SYM_ABOUT_Y,
    WAFER_SYM_ANTISYM_ABOUT_Y
} wafer_symmetry;
int wafer_symmetrise(wafer_ctx *ctx, int constraint);

/* ---- the hot path -------------------------------------------------------- */
/* evolve (grid.rs:544-687): n_steps = config.output.screen_update; like the
 * reference, n_steps == 0 still takes one step.  wnum > 0 renormalises and
 * Gram-Schmidts against w_store[0..wnum) after every step. */
int wafer_evolve(wafer_ctx *ctx, uint32_t wnum, uint64_t n_steps);
/* compute_observables (grid.rs:303-445) */
int wafer_observables(wafer_ctx *ctx, wafer_observables_t *out);
/* get_norm_squared over the work area (grid.rs:454-457) */
int wafer_norm2(wafer_ctx *ctx, double *out);
/* normalise_wavefunction (grid.rs:465-468) */
int wafer_normalise(wafer_ctx *ctx, double norm2);
/* orthogonalise_wavefunction (grid.rs:477-492) */
int wafer_orthogonalise(wafer_ctx *ctx, uint32_t wnum);

/* ---- w_store: Vec<Array3<R64>> of grid.rs:34 ----------------------------- */
int wafer_push_state(wafer_ctx *ctx);                               /* w_store.push(phi), grid.rs:241 */
int wafer_load_state(wafer_ctx *ctx, uint32_t idx, const double *state); /* input::load_wavefunctions, grid.rs:38 */
int wafer_download_state(wafer_ctx *ctx, uint32_t idx, double *state);
int wafer_clone_state_to_phi(wafer_ctx *ctx, uint32_t idx);         /* w_store[wnum-1].clone(), grid.rs:95 */
int wafer_num_states(wafer_ctx *ctx, uint32_t *out);
int wafer_clear_states(wafer_ctx *ctx);

/* ---- Rayleigh-Ritz on w_store -------------------------------------------- */
/* The reference's Gram-Schmidt scheme (grid.rs:477-492) leaves the states of a near-degenerate shell, and any state stored
 * before it had fully converged, mixed.  One Rayleigh-Ritz step on the first k stored states unmixes them: with
 *   H_ij = <l_i| V - S / den |l_j>   (the energy integrand of compute_observables, grid.rs:325-332, between two states)
 *   S_ij = <l_i|l_j>                 (sums over the work area, fp64 whatever the dtype)
 * solve H c = e S c and replace the states by l'_a = sum_j c_ja l_j: S' = 1, H' = diag(e), e ascending, each no higher than
 * what the single states gave.  Matrices are row-major k * k doubles; h[j * k + i] is the sum of l_i times (H l_j), so
 * h[j * k + j] has the bits of wafer_observables' energy on state j and s[j * k + j] those of its norm2.
 * k == 0 or k > WAFER_RITZ_MAX, and a context that owns a z-slab (z_count != 0), are WAFER_ERR_INVALID; k above the number of
 * stored states, or no potential, WAFER_ERR_STATE.  A call that fails changes neither the store nor its outputs; phi is never
 * touched.  Stored states are rounded to the dtype's storage once, after the rotation. */
#define WAFER_RITZ_MAX 8
/* host only, no context: the generalised symmetric eigenproblem of (h + h^T)/2 and (s + s^T)/2 by Cholesky and cyclic Jacobi.
 * evals[k] ascending; coef[j * k + a] = component of input state j in output state a, each column's largest component positive.
 * s not positive definite (linearly dependent states) or a non-finite entry: WAFER_ERR_STATE. */
int wafer_ritz_solve(uint32_t k, const double *h, const double *s, double *evals, double *coef);
/* H and S of the first k stored states with the context's V, stencil and denominator */
int wafer_ritz_matrices(wafer_ctx *ctx, uint32_t k, double *h, double *s);
/* l'_a = sum_j coef[j * k + a] l_j for the first k stored states, in place (frame and padding included: zeros stay zeros);
 * everything the context derived from the store is recomputed or dropped */
int wafer_rotate_states(wafer_ctx *ctx, uint32_t k, const double *coef);
/* the three in sequence; h, s (the matrices before the rotation) may be NULL */
int wafer_ritz(wafer_ctx *ctx, uint32_t k, double *evals, double *coef, double *h, double *s);

/* ---- stepping w_store (subspace iteration) -------------------------------- */
/* The first k stored states advance by n_steps plain imaginary-time steps each (n_steps == 0 takes one): no projection and no
 * normalisation.  Afterwards every one of them holds, bit for bit, what phi would hold after wafer_evolve(ctx, 0, n_steps) had phi
 * started as that state, on every dtype -- the context runs its own ground-state passes on the state and one shadow array.  phi,
 * the current buffer, the states from k on and V keep every bit; phi need not be set.  The Gram matrix is recomputed and the
 * two-step pass's images are dropped, as after wafer_rotate_states.  Step the block, take one wafer_ritz step, compare the Ritz
 * energies with the last block's: state i then converges with the gap to the first level outside the block.
 * k == 0, k > WAFER_RITZ_MAX and a context that owns a z-slab are WAFER_ERR_INVALID; k above the number of stored states, or no
 * potential, WAFER_ERR_STATE; a refused call changes nothing.  wafer_last_evolve_ms afterwards gives the whole call's time and
 * n_steps. */
int wafer_evolve_states(wafer_ctx *ctx, uint32_t k, uint64_t n_steps);

/* ---- filtering w_store (Chebyshev-filtered subspace iteration) ------------ */
/* A degree-m scaled Chebyshev polynomial of the discrete H itself (Zhou, Saad, Tiago, Chelikowsky 2006) applied to the first k
 * stored states: [a, b] is the interval to damp, a0 < a the anchor at which the polynomial has magnitude 1.  Because the polynomial
 * is in H, the fixed points of filter + wafer_ritz are H's eigenvectors and wafer_residuals' rho falls to rounding level -- unlike
 * wafer_evolve_states, whose semi-implicit step leaves rho at O(dt V).
 * The coefficients, on the host, every operation a double operation of its own:
 *   e = (b - a) / 2    cc = (b + a) / 2    sigma = e / (a0 - cc)    gamma = 2 / sigma
 *   step 1:      al = sigma / e,  be = 0
 *   step i >= 2: s2 = 1 / (gamma - sigma)    al = (2 s2) / e    be = sigma s2    sigma = s2
 * and step i per work cell c, fp64 and unfused on every dtype, operands widened from the storage type and y rounded to it once:
 *   w = cur[c]    hw = V[c] w - S / den    t = hw - cc w    y = al t    i >= 2: y = y - be prev[c]    out[c] = y
 * with S the bracketed stencil sum of cur at c (frame cells as stored), exactly as in wafer_residual_to_phi (the step with al = 1,
 * cc = theta).  Step 1 reads the state and writes a shadow array (zeros outside the work cells); step i >= 2 writes its result over
 * the iterate before last, in place: two arrays per state, no more.  The result of an even degree keeps the state's frame cells,
 * that of an odd degree has zeros there.
 * host only, no context: al[degree], be[degree] (be[0] = 0) and cc.  degree == 0 or > WAFER_FILTER_MAX_DEGREE, a non-finite value
 * or anything but a0 < a < b: WAFER_ERR_INVALID, nothing written. */
#define WAFER_FILTER_MAX_DEGREE 256
int wafer_filter_coefficients(uint32_t degree, double a, double b, double a0, double *al, double *be, double *cc);
/* One launch per state and step.  phi, the current buffer, the states from k on and V keep every bit; phi need not be set.  The
 * Gram matrix is recomputed and the two-step pass's images are dropped, as after wafer_evolve_states.  k == 0, k > WAFER_RITZ_MAX,
 * a refused interval or degree, and a context that owns a z-slab are WAFER_ERR_INVALID; k above the number of stored states, or no
 * potential, WAFER_ERR_STATE; a refused call changes nothing.  wafer_last_evolve_ms afterwards gives the call's time and degree. */
int wafer_filter_states(wafer_ctx *ctx, uint32_t k, uint32_t degree, double a, double b, double a0);
/* An upper bound of H's spectrum for b, by Gershgorin: ub = W / den + max V over the work cells, with den the kernels' own
 * (2, 24, 360 dn^2 mass) and W = 12, 192, 3264 the sum of the absolute stencil weights, centre included.  The maximum is exact.
 * No potential: WAFER_ERR_STATE; a context that owns a z-slab: WAFER_ERR_INVALID. */
int wafer_spectral_bound(wafer_ctx *ctx, double *ub);

/* ---- residuals of w_store and of phi -------------------------------------- */
/* How far a state is from an eigenstate of the discrete H (stencil, Dirichlet frame): with r = H l - theta l over the work area,
 * some eigenvalue of H lies within rho = sqrt(r2 / s) of theta, where r2 = sum r^2 and s = sum l^2.  Per work cell c, every
 * operand widened to double and every operation fp64 and unfused, whatever the dtype:
 *   w = l[c]  vv = V[c]  S = the bracketed stencil sum of l at c (frame cells as stored)  hw = vv * w - S / den  r = hw - theta * w
 * and the sums r2 += r * r, wh += w * hw, s += w * w run on the partition of wafer_observables, without floating-point atomics:
 * s[j] has the bits of wafer_observables' norm2 and of wafer_ritz_matrices' s[j * k + j] on the same state.
 * source: the first k stored states, or the current wavefunction (k must be 1).  theta_in: k finite doubles -- one sums launch,
 * one reduce, one read-back, and theta receives a copy.  theta_in == NULL is Rayleigh mode: a first pass with theta = 0 gives
 * theta_j = wh_j / s_j on the host, a second pass with that theta gives r2 and s (one pass cannot: expanding |H l - theta l|^2
 * into three sums cancels to nothing on a nearly converged state).  If s_j is not finite or not > 0 the call fails with
 * WAFER_ERR_STATE naming the state and writes nothing.
 * Checked before any launch, and a refused call changes nothing: k == 0, k > WAFER_RITZ_MAX, k != 1 with WAFER_RESIDUAL_PHI, an
 * unknown source, a non-finite theta_in and a context that owns a z-slab are WAFER_ERR_INVALID; k above the number of stored
 * states, phi not set, or no potential, WAFER_ERR_STATE.  The call is read-only: the store, phi, the Gram matrices and the
 * two-step pass's images keep every bit.  theta, r2, s: k doubles each. */
#define WAFER_RESIDUAL_STATES 0   /* the first k stored states */
#define WAFER_RESIDUAL_PHI    1   /* the current wavefunction; k must be 1 */
int wafer_residuals(wafer_ctx *ctx, int source, uint32_t k, const double *theta_in, double *theta, double *r2, double *s);
/* phi (the current buffer) = r of stored state idx with theta, rounded to the dtype's storage once; every other element of the
 * array -- frame, pad and guard cells -- is written as zero, so phi is a valid wavefunction for every step kernel.  Sets phi;
 * leaves the store alone.  No state idx or no potential: WAFER_ERR_STATE; a non-finite theta or a z-slab: WAFER_ERR_INVALID. */
int wafer_residual_to_phi(wafer_ctx *ctx, uint32_t idx, double theta);

/* ---- moment matrices of w_store ------------------------------------------- */
/* What else a converged set of levels is asked: for the first k stored states l_0 .. l_{k-1} the five k x k matrices
 *   S_ij = <l_i|l_j>   X_ij = <l_i|x|l_j>   Y_ij = <l_i|y|l_j>   Z_ij = <l_i|z|l_j>   R2_ij = <l_i|r^2|l_j>
 * -- sizes (R2_jj / S_jj) and dipole matrix elements -- from one sums launch, one reduce and one read-back.  For a work cell c with
 * 0-based work indices (ix, iy, iz) of a grid nx x ny x nz
 *   dx = (double)ix - ((double)nx + 1.) / 2.     dy, dz likewise     r2c = dx * dx + dy * dy + dz * dz
 * which is the r^2 of wafer_observables letter for letter, in index units like wafer_observables_t's r2.  NOTE the origin: it lies
 * ONE CELL ABOVE the geometric centre (n - 1) / 2 of the work indices.  That is the reference's convention (grid.rs:428-437),
 * kept so that the diagonal ties to wafer_observables; S is returned so that a caller can move the origin without a second call:
 * <i|x - c|j> = X_ij - c * S_ij.  For column j and every i <= j, every operand widened to double and every operation fp64 and
 * unfused whatever the dtype:
 *   w = l_j[c]   l = l_i[c]   p = l * w      S_ji += p   X_ji += p * dx   Y_ji += p * dy   Z_ji += p * dz   R2_ji += p * r2c
 * over the work cells only (frame cells are never read), on the partition of wafer_observables and wafer_ritz_matrices, without
 * floating-point atomics: R2[j][j] and S[j][j] have the bits of wafer_observables' r2 and norm2 on state j, every S entry the bits
 * of wafer_ritz_matrices' s, and the entries of the columns below k do not depend on k.  The entries i > j are copies of their
 * mirror images (l * w commutes: the copy is exact).  m: WAFER_MOMENT_COUNT * k * k doubles, matrix q row-major at q * k * k.
 * Checked before any launch, and a refused call writes nothing: k == 0, k > WAFER_RITZ_MAX, m == NULL and a context that owns a
 * z-slab are WAFER_ERR_INVALID; k above the number of stored states, WAFER_ERR_STATE.  Read-only like wafer_residuals: the store,
 * phi, the Gram matrices and the two-step pass's images keep every bit.  V is not read: no potential is needed. */
#define WAFER_MOMENT_S 0
#define WAFER_MOMENT_X 1
#define WAFER_MOMENT_Y 2
#define WAFER_MOMENT_Z 3
#define WAFER_MOMENT_R2 4
#define WAFER_MOMENT_COUNT 5
int wafer_moment_matrices(wafer_ctx *ctx, uint32_t k, double *m);   /* m[(q * k + j) * k + i] */

/* ---- solve (grid.rs:50-246) for ONE state, snapshot branch excluded ------ */
/* phi must hold the starting wavefunction.  Writes up to max_records rows,
 * *n_records = rows produced.  Returns WAFER_OK when converged (phi has then
 * been pushed to w_store, grid.rs:239-242) and WAFER_ERR_MAX_STEP otherwise. */
int wafer_solve_state(wafer_ctx *ctx, uint32_t wnum, double tolerance, uint64_t screen_update,
                      int has_max_steps, uint64_t max_steps, wafer_block_record *records,
                      size_t max_records, size_t *n_records, wafer_observables_output *final_out);

/* ---- measurement ---------------------------------------------------------- */
/* HIP-event time of the kernels of the last wafer_evolve call, on the stream
 * they ran on, and the number of steps it took.  Blocks until they finish. */
int wafer_last_evolve_ms(wafer_ctx *ctx, float *ms, uint64_t *steps);
/* name of the stencil kernel a ground-state pass of this context launches (no template arguments): wafer_k_step3_fused,
 * wafer_k_step2_wide (FivePoint), wafer_k_step2_fused, wafer_k_step_lds, wafer_k_step_direct */
const char *wafer_stencil_kernel_name(wafer_ctx *ctx);
/* the template-id of the kernel the last ground-state pass launched, as a profiler prints it (e.g.
 * "wafer_k_step3_fused<double, double, true, 0, true, 1>"); the family name where the family does not record it.  Valid until
 * the next call on this context. */
const char *wafer_stencil_kernel_instance(wafer_ctx *ctx);
/* time steps one launch of that kernel advances in a ground-state evolve (2 for the fused kernel) */
int wafer_stencil_steps_per_launch(wafer_ctx *ctx);
/* choose a stencil kernel variant by index (tuning / A-B runs); -1 = default */
int wafer_set_stencil_variant(wafer_ctx *ctx, int variant);

/* Diagnostic: the device's copy ceiling -- 16 B per lane, `unroll` (1, 2, 4, 8) vectors in flight per
 * lane, grid-stride over blocks_per_cu x CUs workgroups of 256 threads, V -> phi's scratch buffer;
 * GB/s of read + written bytes.  MI355X_MICROARCH.md quotes ~6.3 TB/s for this pattern. */
int wafer_diag_copy_bw(wafer_ctx *ctx, int iters, int unroll, int blocks_per_cu, double *gbps);

/* Diagnostic: integer checksum of the current wavefunction's work cells on global work planes
 * [z_begin, z_begin + z_count), a sum mod 2^64 of a hash of each cell's bits and its GLOBAL index.  Order
 * independent, so the checksums of the slabs of a decomposed run must equal those of the same plane
 * ranges of an undecomposed run whenever the bits agree: bench.py's N > 1 parity check.
 *
 * The definition, all arithmetic in unsigned 64 bits (mod 2^64), so that any host can restate it
 * (tests/checksum_model.py does, in numpy):
 *   h(z):  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
 *   lin  = (k * ny + y) * nx + x        for the work cell (x, y, k): x in [0, nx), y in [0, ny), k the GLOBAL work plane
 *   term = h(bits ^ h(lin + 0x9e3779b97f4a7c15))
 *   *out = the sum of term over the cells counted
 * bits: the 64 bits of the stored double (dtype f64); the 32 bits of the stored float, zero-extended to 64 (dtypes
 * f32 and f32fast).  No bit is canonicalised: 0.0 and -0.0, and two NaNs of different payloads, give different terms.
 * Cells counted: the work cells of the planes k that lie in the range AND are owned by this context
 * (z_begin <= k < z_begin + z_count of its wafer_params).  Frame cells and ghost planes never count.  The range
 * is clipped to the grid's planes [0, nz): what reaches past nz is ignored, and a range with z_count = 0
 * or z_begin >= nz -- or one that misses the slab -- gives 0. */
int wafer_diag_checksum(wafer_ctx *ctx, uint32_t z_begin, uint32_t z_count, uint64_t *out);

/* Diagnostic: global padded planes [zp_begin, zp_begin + zp_count) of one device array in the reference's layout,
 * out[px][py][zp_count] (z contiguous) -- what wafer_download_array / wafer_download_phi return, restricted to a z-window, for
 * grids whose arrays do not fit the host (1024^3, 2048^3: tests/test_gpu_fullsize.py compares such windows cell by cell with the
 * oracle).  array_id: WAFER_ARRAY_V / _A / _B, or WAFER_ARRAY_PHI (the current wavefunction).  The planes must be among those the
 * context holds (its owned planes + halo_depth ghost planes per side, and the global frame): WAFER_ERR_INVALID otherwise. */
#define WAFER_ARRAY_PHI 4
int wafer_diag_download_window(wafer_ctx *ctx, int array_id, uint32_t zp_begin, uint32_t zp_count, double *out);

/* Diagnostic: which kernel a pass of wafer_evolve(ctx, wnum, .) launches for this context, as one line of key=value pairs ("wnum=0 stencil=1
 * dtype=f64 kernel=wafer_k_step3_fused steps_per_pass=3 ghost_planes_per_pass=3 tile=128x16 v=streamed remainder=wafer_k_step2_fused,wafer_k_step_lds"):
 * the launch path's own predicates, nothing launched.  tools/dispatch_table.py tabulates it (profiles/r06_dispatch_table.md). */
int wafer_diag_dispatch(wafer_ctx *ctx, uint32_t wnum, char *buf, size_t n);

/* Diagnostic: how many passes of the two-excited-steps-per-pass kernel (wafer_stencil_x2.hip.h: ThreePoint fp64, one to three
 * stored states) this context has launched so far -- tests assert that the kernel they mean to test is the one that ran. */
int wafer_diag_x2_passes(wafer_ctx *ctx, uint64_t *out);

/* Diagnostic: the divisions by loop-invariant denominators the host has not planned (the norm in the excited-state
 * transform, projection coefficients) use a hoisted reciprocal with two exact remainders instead of the IEEE
 * sequence (wafer_div_invariant(x, den), wafer_stencil.hip.h).  Draws n_operands (rounded up to 2^18) doubles
 * with uniform sign / significand and biased exponent uniform in [lo_exp, hi_exp] and counts those
 * whose quotient by `den` differs in any bit from the device's IEEE x / den. */
int wafer_diag_div_check(wafer_ctx *ctx, double den, uint64_t seed, uint64_t n_operands, int lo_exp, int hi_exp,
                         uint64_t *mismatches);

/* The division by the run's ONE stencil denominator c dn^2 m (grid.rs:569 / 594 / 626) is planned when the context is created
 * (wafer_amd/csrc/wafer_divplan.h): q = RN(x zh + RN(x zl)) with zh = RN(1/den), zl = RN(1/den - zh) (moved by zl_shift ulps if
 * that gets more operands through) is RN(x/den) except for the few dozen significands x whose quotient lies within 2^-50 ulp of
 * the midpoint of two doubles; the plan enumerates those (n_candidates) and tries each with the device's instruction sequence.
 * checked = 1: all came out as the IEEE quotient, so the three-instruction form is the division for every x (|x/den| >= 2^-960);
 * checked = 0: the kernels add one Markstein round (always correct, two instructions more). */
typedef struct wafer_div_plan_t {
    double den, zh, zl;
    int32_t checked, n_candidates, zl_shift, reserved;
} wafer_div_plan_t;
/* Host only (no GPU needed): the plan for `den`; candidates (may be NULL): up to `cap` of the enumerated significands, as doubles
 * in [2^52, 2^53), *n_written of them. */
int wafer_div_plan(double den, wafer_div_plan_t *out, double *candidates, size_t cap, size_t *n_written);
/* the plan this context's kernels run with */
int wafer_get_div_plan(wafer_ctx *ctx, wafer_div_plan_t *out);
/* Diagnostic: the planned division as the kernels perform it (wafer_div_invariant(x, WaferDen)) with the given plan -- any
 * plan, also one whose `checked` the caller has forced -- on n_random drawn operands (as wafer_diag_div_check) and on the
 * n_operands doubles at `operands` (host memory; may be NULL): the number of quotients that differ from the device's IEEE
 * x / den in any bit, separately. */
int wafer_diag_div_planned(wafer_ctx *ctx, const wafer_div_plan_t *plan, uint64_t seed, uint64_t n_random, int lo_exp, int hi_exp,
                           const double *operands, size_t n_operands, uint64_t *mismatches_random, uint64_t *mismatches_operands);

/* The same plan in fp32, for WAFER_F32_FAST contexts (whose step kernels compute in fp32): q = RN(x zh + RN(x zl)) in float, checked by
 * trying all 2^23 significands on the host (tens of milliseconds; |x/den| >= 2^-100, |den| in [2^-60, 2^60]).  Unchecked: the kernels divide. */
typedef struct wafer_div_plan_f32_t {
    float den, zh, zl;
    int32_t checked, zl_shift;
} wafer_div_plan_f32_t;
int wafer_div_plan_f32(float den, wafer_div_plan_f32_t *out);   /* host only */
/* Diagnostic: the planned fp32 division on EVERY float with a biased exponent in [lo_exp, hi_exp] (all significands, both signs)
 * against the device's IEEE x / den: the number of quotients that differ in any bit. */
int wafer_diag_div_planned_f32(wafer_ctx *ctx, const wafer_div_plan_f32_t *plan, int lo_exp, int hi_exp, uint64_t *mismatches);

/* ---- multi-GPU: communication hooks --------------------------------------- */
/* The engine never links a communication library.  A host that z-slabs the
 * grid over several contexts installs two hooks (RCCL via torch.distributed in
 * wafer_amd/slab.py; ncclSend/ncclRecv + ncclAllReduce in a Rust host):
 *  - halo: copy `bytes` from this rank's send_lo / send_hi (its first / last
 *    `planes` owned planes) into the z-neighbours' ghost planes and fill
 *    recv_lo / recv_hi from theirs.  A NULL pointer means "no neighbour on
 *    that side" (global Dirichlet frame).
 *  - allreduce: in-place sum over ranks of `count` doubles at dev_ptr.
 * Both are called with the hipStream_t the data is ordered on; on return the
 * result must be ordered on that same stream (enqueue, do not block). */
typedef int (*wafer_halo_fn)(void *user, void *send_lo, void *send_hi, void *recv_lo, void *recv_hi,
                             size_t bytes, void *hip_stream);
typedef int (*wafer_allreduce_fn)(void *user, void *dev_ptr, size_t count, void *hip_stream);
int wafer_set_comm_hooks(wafer_ctx *ctx, wafer_halo_fn halo, wafer_allreduce_fn allreduce, void *user);
/* The halo hook may be called with only one direction non-NULL (send_lo + recv_hi, or send_hi + recv_lo: the
 * single-launch pass of wafer_set_overlap mode 2 exchanges the two sides at different times): a hook must
 * tolerate a NULL on a side that has a neighbour, and pair send_lo with the lower neighbour's recv_hi. */
/* z-slabs, how the halo exchange is scheduled (modes 0 .. 6; 3 .. 6 below).  All modes give identical results.
 *  0 = the exchange follows the whole slab's update (nothing overlaps);
 *  1 = boundary planes first, then their exchange, both on a second stream, beside the interior update:
 *      three launches per pass;
 *  2 (default) = ONE launch per three-step pass updates the whole slab as two halves marched outwards from the middle plane;
 *      workgroups count themselves done and the second stream releases each half's exchange as soon as that half
 *      is complete; the ghost planes an exchange fills are announced by a device flag that only the workgroups
 *      reading them poll, shortly before the end of their column.  Ground-state three-step passes with one exchange
 *      per pass; other ground-state passes run as in mode 1, excited-state steps (one plane per side and step) as in
 *      mode 0, which measured faster for them.  The order of the halves alternates from pass to pass,
 *      so every rank must make the same sequence of wafer_evolve calls (as it must anyway).  A workgroup waits at most
 *      WAFER_HV_WAIT_MS (default 20 s) for its ghost planes; one that gives up stores NaN from there on and the next
 *      call that synchronises with the device returns WAFER_ERR_COMM.
 * Setting a mode also resets the pass bookkeeping (which half goes first, which ghost planes are current): after a
 * WAFER_ERR_COMM on any rank, call it on every rank before evolving again. */
int wafer_set_overlap(wafer_ctx *ctx, int mode);
/*  3 = mode 2's single launch with PEER STORES instead of an exchange: the boundary workgroups of a pass store their last
 *      planes into the z-neighbours' ghost planes themselves (the neighbour's buffers mapped here: directly within one process,
 *      through HIP IPC between processes of one node, over xGMI between GPUs) and count themselves into the neighbour's arrival
 *      counter; the neighbour's boundary workgroups poll that counter just before their first ghost-plane load.  No exchange
 *      kernels (RCCL's need whole CUs), no gate kernels, no second stream, no short columns.  Needs wafer_peer_connect on every
 *      rank first and at least 6 owned planes per rank; the host switches all ranks or none.  The first pass of a run of passes
 *      still takes its ghost planes from the halo hook (it is the run's rendezvous).  Other passes as in mode 2. */
/*  4 = PEER COPIES (round 6): every exchange of phi's ghost planes -- the passes' of modes 2 / 1 / 0, the excited-state steps', the ones
 *      observables and wafer_push_state ask for -- is a device copy (hipMemcpyAsync: a copy engine between GPUs, no CU of either) from
 *      this rank's boundary planes INTO the z-neighbour's ghost planes through the mapping wafer_peer_connect holds; the halo hook is
 *      not called for phi at all (the stored states' own ghost planes, exchanged once per change of w_store, keep it; so does the
 *      all-reduce).  The hook's two-sided contract is kept by a rendezvous of four words per link in the neighbours' memory
 *      (one-wave kernels in stream order: "receive k posted" -> wait -> copy -> "copy k landed" -> wait), so a rank's ghost planes are
 *      overwritten only once it would have posted the receive.  Ground-state three-step passes run as mode 2's single launch, without
 *      its short columns (no exchange kernel needs a CU).
 *  5, 6 = peer copies under mode 1's (boundary planes first, three launches per pass) / mode 0's (exchange after the pass) launches:
 *      every kernel that reads ghost planes is launched after the copy that filled them has completed, so nothing rests on what a
 *      RUNNING kernel sees of a peer's writes -- the one assumption mode 4 shares with mode 3 on the consumer side.  (WAFER_COPY_SCHED =
 *      1 / 0 turns mode 4 into these.)  Needs wafer_peer_connect on every rank first; any stencil, storage type and slab
 *      thickness.  After a WAFER_ERR_COMM under this mode the two ends of a link may disagree on their counts: export and connect
 *      again (a fresh export restarts them).  As for mode 3, contexts of ONE process on ONE device must not sit in a device-wide
 *      synchronisation (hipFree, hipDeviceSynchronize) while a neighbour context waits for their signal -- one process per GPU cannot.
 * Peer stores: what a rank publishes about itself, and the connection to its z-neighbours.  wafer_peer_export fills `out`
 * (device addresses valid in this process + HIP IPC handles of the allocations for other processes); the host carries the
 * records to the neighbours (any transport) and calls wafer_peer_connect with the lower / upper neighbour's record (NULL: no
 * neighbour on that side; a record exported by this same process is used by address, without IPC -- several contexts in one
 * process, or a slab whose neighbour is itself; a context of this process on ANOTHER device is used by address after
 * hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess, WAFER_ERR_INVALID where the devices cannot reach each other).  A neighbour
 * that is another context on the SAME device is refused (WAFER_ERR_INVALID) unless WAFER_PEER_SAME_DEVICE=1: its kernels share
 * this one's CUs, and a workgroup polling for a neighbour's stores can then keep that neighbour's kernel from running until the
 * bounded wait gives up -- tests fold ranks onto one GPU on purpose; a real run has one GPU per rank.
 * wafer_peer_disconnect unmaps; wafer_ctx_destroy does it too. */
typedef struct wafer_peer_info {
    uint32_t struct_size;
    uint32_t z_begin, z_count, halo_depth;
    uint64_t pid;                 /* of the exporting process */
    uint64_t phi_addr[2];         /* the two ping-pong buffers (plane 0, row 0) */
    uint64_t flags_addr;          /* arrival counters: [0] lower ghost side, [8] upper (64-bit words, one 64-byte line each) */
    uint64_t phi_alloc_offset[2]; /* byte offset of phi_addr inside its allocation (IPC maps allocations) */
    uint8_t phi_ipc[2][64];       /* hipIpcMemHandle_t */
    uint8_t flags_ipc[64];
    uint64_t process_nonce;       /* drawn once per process: with pid it identifies the exporting process (pids alone repeat across
                                     PID namespaces) -- the by-address shortcut is taken only when both match */
    int32_t device;               /* HIP ordinal of the exporting context's device, as the exporting process numbers them */
    uint32_t reserved;
    uint8_t device_uuid[16];      /* hipDeviceGetUuid of that device: the same GPU whatever the process calls it */
} wafer_peer_info;
int wafer_peer_export(wafer_ctx *ctx, wafer_peer_info *out);
int wafer_peer_connect(wafer_ctx *ctx, const wafer_peer_info *lower, const wafer_peer_info *upper);
int wafer_peer_disconnect(wafer_ctx *ctx);

/* z-slabs, ground state: fused passes per halo exchange.  One fused pass advances K time steps and consumes
 * K * ext ghost planes per side (K = 3 where the three-step kernel applies: ThreePoint, any dtype,
 * with halo_depth >= 3 * ext; else K = 2 -- every rank of a run must be created alike).  With `passes` > 1 the exchange moves K * ext * passes planes at once and
 * the passes in between run unsplit over the owned planes plus the ghost planes that are still valid -- fewer
 * boundary launches, exchanges and stream hops for a few redundant planes.  Needs wafer_params.halo_depth >=
 * K * ext * passes (WAFER_ERR_INVALID otherwise); the default is 1.  All settings give identical results. */
int wafer_set_halo_cycle(wafer_ctx *ctx, int passes);
/* run every kernel on a caller-owned hipStream_t (NULL = the context's own) */
int wafer_set_stream(wafer_ctx *ctx, void *hip_stream);
/* geometry of the local slab, for hosts that need it */
typedef struct wafer_slab_info {
    uint32_t z_begin, z_count, halo_depth, ext;
    uint64_t plane_elems;   /* elements per z-plane of the device layout */
    uint64_t elem_bytes;
} wafer_slab_info;
int wafer_get_slab_info(wafer_ctx *ctx, wafer_slab_info *out);
/* the device the context runs on, as its own properties describe it (printed by the benchmark
 * next to the datasheet HBM peak; the reference has no counterpart) */
typedef struct wafer_device_info {
    char name[64];
    char arch[64];
    uint32_t compute_units;
    uint32_t memory_clock_khz;
    uint32_t memory_bus_bits;
    uint32_t l2_bytes;
    uint64_t total_bytes;
} wafer_device_info;
int wafer_get_device_info(wafer_ctx *ctx, wafer_device_info *out);

/* ---- batched ensembles ------------------------------------------------------
 * A batch holds B independent ground-state problems ("members") on one device, all with the same work-area shape
 * (wafer_batch_create; wafer_batch_create_mixed lifts that: "Mixed-shape batches" below), the same
 * central_difference and the same dtype, each with its own dn, dt, mass, sig, flags, potential, pot_sub and wavefunction.  One
 * launch per step advances every ACTIVE member (a workgroup table built from the active members only: a member that is not
 * active costs nothing) -- or one launch per PASS of K ground-state steps where a fused pass is selected
 * (wafer_batch_set_step_variant; ThreePoint K = 3, FivePoint K = 2, the intermediate steps never leave the CU, the same bits);
 * observables are one launch, one reduce launch and one small download for all members.  Every member
 * computes bit for bit what a single wafer_ctx with its wafer_params computes: phi after evolve, the observables (the single
 * context's partition and reduction order), normalisation and solve.  No z-slabs (z_count must be 0).  Excited states: the
 * wafer_batch_*_state calls further down.
 * Member arrays live in one allocation per array kind (phi ping-pong, V, pot_sub) with a member stride.
 * wafer_batch_create validates every member before any HIP call (WAFER_ERR_INVALID names the member and the field).
 *
 * dtype: WAFER_F64, WAFER_F32 or WAFER_F32_FAST, ONE per batch -- a member whose dtype differs from member 0's, or lies outside
 * the enum, is WAFER_ERR_INVALID naming the member and "dtype".  The other member rules do not depend on it.  On the two float
 * dtypes every array and every store slot is float (half the bytes per cell; rows are padded to whole 1 KiB tiles as a context's
 * are, so the allocation halves only where the row pitch does), host arrays at this ABI stay
 * double -- uploads and state loads round to nearest even as a context's do, downloads widen -- and:
 *  - ground state: bit for bit a wafer_ctx of the same wafer_params under its default dispatch, under the fused pass too.
 *    a and b are formed from the STORED (float) V in the arithmetic type inside the kernel, and the result of EVERY step is
 *    rounded to float (in a fused pass each intermediate level is rounded before the next one reads it).  WAFER_F32: fp64
 *    arithmetic.  WAFER_F32_FAST: every operand and operation of the step is float, the division by c dn^2 m is the member's
 *    own fp32 plan (wafer_div_plan_f32 of (float)den; checked or not as for a context; WAFER_FLAG_UNPLANNED_DIV is honoured).
 *  - observables, normalise and solve compute in fp64 on the float arrays, on the partition and in the reduction order of a
 *    context of that dtype (16 bytes per lane: tiles twice as wide as on doubles): bit for bit that context.  normalise
 *    rounds its quotient to float.
 *  - excited states (the *_state calls, orthogonalise, evolve_state, solve_state): fp64 arithmetic throughout on both float
 *    dtypes (a WAFER_F32_FAST batch takes the fp64-arithmetic step there, as a context does), float stores, and phi rounded to
 *    float where each kernel writes it: after the step, after the scale, after each projection.  The guarantees below carry
 *    over unchanged (no dependence on B, index or active set; frozen members untouched; no floating-point atomics).
 *    wafer_batch_norm2 on the float dtypes sums in fp64 on the partition and in the order of wafer_norm2 of a context of that
 *    dtype: the same double, bit for bit.  (On WAFER_F64 it keeps the batch's own partition: rel 1e-12 against a context.) */
typedef struct wafer_batch wafer_batch;
int wafer_batch_create(const wafer_params *members, uint32_t n_members, wafer_batch **out);
/* ---- Mixed-shape batches ----
 * As wafer_batch_create, but nx, ny, nz may differ from member to member (a convergence study: one problem at several N and dn,
 * side by side in one batch).  central_difference, dtype, device, halo_depth are still the batch's (member 0's), z_count is
 * still 0, every other member rule is unchanged and reported with the same messages before any HIP call; the overflow check is
 * on the SUM of the members' allocation sizes.  Members lie in one allocation per array kind at the prefix sums of their own
 * padded sizes, each with its own guard rows and planes.
 * One distinct shape among the members: the batch behaves in every call like one made by wafer_batch_create, excited states and
 * the one-pass form included, and wafer_batch_diag_dispatch gives the same line.
 * More than one distinct shape ("mixed-shape"), the ground-state path:
 *  - evolve: every member computes, bit for bit, what a wafer_ctx with its own wafer_params computes -- with the one-step kernel
 *    and under wafer_batch_set_step_variant(b, 1) (the fused pass), on WAFER_F64, WAFER_F32 and WAFER_F32_FAST.
 *  - wafer_batch_observables follows the context's partition and reduction order FOR THAT MEMBER'S SHAPE: all four sums are the
 *    context's doubles.  wafer_batch_normalise and wafer_batch_solve give the context's bits.  wafer_batch_norm2 gives the
 *    context's double on the float dtypes; on WAFER_F64 it keeps the batch's own partition (per shape), rel 1e-12.
 *  - launches: ONE per step, or per fused pass, covers all active members whatever their shapes (not one per shape: the workgroup
 *    table runs over all of them and every entry names its member's geometry); observables stay one launch plus one reduce
 *    launch, normalise one launch.  wafer_batch_diag_passes counts launches: n single steps add n.
 *  - a member's bits do not depend on the batch size, its index, the other members' shapes or the active set; a frozen member is
 *    untouched bit for bit.  No floating-point atomics, no host synchronisation between steps.
 *  - the calls that need the state stores return WAFER_ERR_INVALID with a message that contains "mixed-shape" and names the call,
 *    and change nothing: wafer_batch_load_state, _download_state, _push_state, _clear_states, _clone_state_to_phi, _orthogonalise,
 *    _evolve_state with wnum > 0, _solve_state with any wnum, and wafer_batch_set_gs_variant(b, 1).  (Excited states on several
 *    shapes: create the batch with wafer_batch_create_mixed_states, below.)  wafer_batch_evolve_state(.., 0, ..) is
 *    wafer_batch_evolve, wafer_batch_num_states gives zeros, wafer_batch_diag_gs still answers.
 *  - wafer_batch_diag_dispatch: kernel= names the instantiation actually launched, which reads its geometry from the batch's device
 *    table -- wafer_k_batch_step<R,T,C,WaferBatchGeomTable> / wafer_k_batch_stepk<R,K,T,C,WaferBatchGeomTable> -- and the line ends
 *    with " shapes=N".  wafer_batch_kernel_name gives that one-step instantiation's name. */
int wafer_batch_create_mixed(const wafer_params *members, uint32_t n_members, wafer_batch **out);
/* Mixed-shape batches WITH state stores (opt-in at creation).  Member rules, messages, layout and everything of the ground-state
 * path are wafer_batch_create_mixed's; with one distinct shape the batch is a plain batch in every call and gives the same
 * wafer_batch_diag_dispatch line.  With several shapes NO call is refused: wafer_batch_load_state, _download_state, _push_state,
 * _clear_states, _clone_state_to_phi, _num_states, _orthogonalise, _norm2, _evolve_state with wnum > 0, _solve_state with any wnum
 * and wafer_batch_set_gs_variant(b, 0 | 1 | -1) all work (wnum is one number per call; max_states stays per member).  A store slot
 * is one allocation laid out as the arrays are.
 *  - bits: a member's phi, stored states and norm2 after any of these calls are bit for bit what the same member gets in a batch
 *    of ITS shape made by wafer_batch_create, under the same gs_variant, in the sequential and in the one-pass form, on every
 *    dtype: its Gram-Schmidt partition (tiles of 64 x 4 work cells x 4 planes) and the order of its sums are fixed by its shape
 *    alone.  So everything promised there holds here: WAFER_F64 within 1e-13 per cell of the oracle and of a wafer_ctx, norm2
 *    rel 1e-12; no floating-point atomics; no host synchronisation between steps; frozen members and every stored state untouched
 *    bit for bit; no dependence on B, the member's index, the other members' shapes or the active set.
 *  - launches: one excited step is 1 + 2 (1 + wnum) + 1 launches for all members of all shapes, 4 under the one-pass form, the
 *    Gram refresh one launch plus one reduce -- never one set per shape: the grid is (the largest launched member's workgroups,
 *    launched members) and the workgroups beyond a smaller member's partition leave at once.
 *  - wafer_batch_solve_state: per-member records, finals, statuses and pushes as in a batch of one shape; a short or a full
 *    store is that member's status, not the call's.
 *  - wafer_batch_diag_gs names the table-reading instantiations in kernels= (wafer_k_batch_gs<..,WaferBatchGeomTable>,
 *    wafer_k_batch_gs_sums<..,WaferBatchGeomTable>, wafer_k_batch_gs_apply<..,WaferBatchGeomTable>; the reduces are the same
 *    kernels for every batch) and ends with " shapes=N". */
int wafer_batch_create_mixed_states(const wafer_params *members, uint32_t n_members, wafer_batch **out);
/* number of distinct (nx, ny, nz) among the members */
int wafer_batch_num_shapes(wafer_batch *b, uint32_t *n_shapes);
int wafer_batch_destroy(wafer_batch *b);
int wafer_batch_size(wafer_batch *b, uint32_t *n_members);
/* per member, as wafer_set_potential_builtin / wafer_set_potential_host / wafer_set_initial_condition / wafer_upload_phi /
 * wafer_download_phi do for a context (same array layouts) */
int wafer_batch_set_potential_builtin(wafer_batch *b, uint32_t member, int potential);
int wafer_batch_set_potential_host(wafer_batch *b, uint32_t member, const double *v, int potsub_kind, double potsub_scalar,
                                   const double *potsub);
int wafer_batch_set_initial_condition(wafer_batch *b, uint32_t member, int ic, uint64_t seed);
/* Set-up of many members at once.  The members with active[m] != 0 (NULL: all) are LISTED; potentials / ics / seeds have n_members
 * entries (WAFER_POT_*, WAFER_IC_*; seeds NULL: 0 for all), those of members not listed are not read.  Every listed member ends bit for
 * bit as after wafer_batch_set_potential_builtin / wafer_batch_set_initial_condition on that member -- V (a, b where they exist), pot_sub
 * kind, scalar and array, phi, and every flag -- on batches of one shape and of several, on every dtype; members not listed keep
 * every bit.  The per-cell arithmetic is the context kernels' own (wafer_setup_batch.hip.h).
 * Launches, whatever n_members and the shapes: potentials -- one that generates V, one for the pot_sub arrays if and only if a listed
 * member is FullCornell, one range check, one read-back (a context pays two check launches, two read-backs and a synchronisation per
 * member); initial conditions -- one launch, no read-back.  wafer_batch_diag_setup_counts counts them.
 * All checks for all listed members run before anything is uploaded or launched, and a refused call changes nothing: a value outside
 * its enum on a listed member is WAFER_ERR_INVALID, FromFile / FromScript WAFER_ERR_NOT_AVAILABLE with the context entry's message,
 * each naming the member.  No listed member: WAFER_OK, nothing launched.  (WAFER_ERR_HIP behind the launch: V of the listed members
 * is written and every one of them has v_ysym and v_in_range off -- the safe answers -- until its potential is set again.) */
int wafer_batch_set_potentials_builtin(wafer_batch *b, const uint8_t *active, const int *potentials);
int wafer_batch_set_initial_conditions(wafer_batch *b, const uint8_t *active, const int *ics, const uint64_t *seeds);
/* wafer_download_array / wafer_get_potsub of one member: the arrays it evolves in (WAFER_ARRAY_*: V, a, b padded; pot_sub unpadded) */
int wafer_batch_download_array(wafer_batch *b, uint32_t member, int array_id, double *out);
int wafer_batch_get_potsub(wafer_batch *b, uint32_t member, int *kind, double *scalar);
/* one line of key=value pairs from the member's own host record -- member= have_pot= have_phi= potsub_kind= v_in_range= v_ysym=
 * short_forms= cur= states= -- launches nothing */
int wafer_batch_diag_member(wafer_batch *b, uint32_t member, char *buf, size_t n);
/* launches and read-backs of the batched set-up paths since creation: wafer_batch_set_potentials_builtin,
 * wafer_batch_set_initial_conditions, and the one range check behind a wafer_batch_resample(_member) onto WAFER_RESAMPLE_POTENTIAL
 * (its resampling launch is not counted) */
int wafer_batch_diag_setup_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks);
/* wafer_set_potsub for one member (after its potential is set): a potential_sub override, potential.rs:113-131 */
int wafer_batch_set_potsub(wafer_batch *b, uint32_t member, int kind, double scalar, const double *potsub);
int wafer_batch_upload_phi(wafer_batch *b, uint32_t member, const double *phi);
int wafer_batch_download_phi(wafer_batch *b, uint32_t member, double *phi);
/* n_steps ground-state steps (0 takes one, as wafer_evolve) of the members with active[m] != 0 (active NULL: all) */
int wafer_batch_evolve(wafer_batch *b, const uint8_t *active, uint64_t n_steps);
/* compute_observables of every member: out has n_members entries */
int wafer_batch_observables(wafer_batch *b, wafer_observables_t *out);
/* normalise_wavefunction of the active members, member m by norm2[m] (n_members entries) */
int wafer_batch_normalise(wafer_batch *b, const uint8_t *active, const double *norm2);
/* wafer_symmetrise for every active member at once, member m with constraints[m] (n_members entries, WAFER_SYM_*): ONE launch for
 * all members whose constraint is not WAFER_SYM_NOT_CONSTRAINED, each bit for bit what wafer_symmetrise gives a context, on batches
 * of one shape and of several.  Members that are inactive or not constrained keep their buffer and their bits.  A constraint outside
 * the enum on an active member: WAFER_ERR_INVALID; an active member without phi: WAFER_ERR_STATE; a constraint other than
 * NotConstrained on a batch whose stencil is not SevenPoint: WAFER_ERR_INVALID with wafer_symmetrise's message.  Nothing has changed
 * when it fails.  All constraints NotConstrained: succeeds on any stencil and launches nothing. */
int wafer_batch_symmetrise(wafer_batch *b, const uint8_t *active, const int *constraints);
/* Resampling in a batch: ONE source trilinearly resampled (input::trilerp_resize, input.rs:667-716) onto an array of every active
 * member (active NULL: all) in one launch, whatever the members' shapes -- each member bit for bit what the context entry
 * (wafer_upload_phi_resampled, wafer_set_potential_resampled, wafer_set_potsub_resampled) gives a context of its wafer_params, with
 * that entry's bookkeeping; WAFER_RESAMPLE_STATE writes stored state idx under wafer_batch_load_state's rules (idx <= the member's
 * count, capacity, the count grows where idx equals it; a mixed-shape batch needs its state stores).  Every element of a target that
 * is not a work cell is zero afterwards; members not listed are not touched.
 * basis: where the sample positions come from -- linspace(0, s - 1, basis size) per axis, the first n of them used.
 * WAFER_RESAMPLE_POTSUB needs the member's potential and WAFER_BASIS_WORK.
 * All checks for all listed members run before anything is uploaded or launched: a refused call changes nothing.
 * WAFER_RESAMPLE_POTENTIAL ends in ONE range check for all listed members (one launch, one read-back), not one per member.
 * (A WAFER_ERR_HIP failure is not a refusal: behind the launch the listed arrays are written, and for WAFER_RESAMPLE_POTENTIAL a
 * failed range check leaves every listed member with v_ysym and v_in_range off, the safe answers; set the potential again.)
 * WAFER_ERR_INVALID: sx, sy or sz below 2, an unknown target / src_kind / basis, src_member out of range, a member source that is
 * itself a listed target in the same buffer (its phi onto its phi, its state l onto its state l).  WAFER_ERR_STATE: a member source
 * without phi or without state src_idx, and what the per-member rules above refuse.  An empty active set: WAFER_OK. */
enum { WAFER_RESAMPLE_PHI = 0, WAFER_RESAMPLE_POTENTIAL = 1, WAFER_RESAMPLE_POTSUB = 2, WAFER_RESAMPLE_STATE = 3 };
enum { WAFER_BASIS_PADDED = 0,   /* the member's padded size: input::fill_data's production call */
       WAFER_BASIS_WORK   = 1 }; /* the member's (nx, ny, nz): fill_sub_data, and the reference's unit test */
/* one host source, an UNPADDED [sx][sy][sz] array, onto `target` of every active member (NULL: all) */
int wafer_batch_resample(wafer_batch *b, const uint8_t *active, int target, uint32_t idx,
                         const double *src, uint32_t sx, uint32_t sy, uint32_t sz, int basis);
/* the same with the work cells of src_member's phi (src_kind PHI) or stored state src_idx (STATE) as the source */
int wafer_batch_resample_member(wafer_batch *b, const uint8_t *active, int target, uint32_t idx,
                                uint32_t src_member, int src_kind, uint32_t src_idx, int basis);
/* device time of the last wafer_batch_resample / _resample_member that launched: HIP events around its upload, transpose and the
 * one launch (not the per-member bookkeeping of WAFER_RESAMPLE_POTENTIAL behind it); WAFER_ERR_STATE before the first */
int wafer_batch_last_resample_ms(wafer_batch *b, float *ms);
/* wafer_solve_state(ctx, 0, ...) for every member at once.  records: n_members * max_records_per_member rows, member m's at
 * m * max_records_per_member; n_records, finals, status: n_members entries.  status[m]: WAFER_OK (converged),
 * WAFER_ERR_MAX_STEP, or WAFER_ERR_STATE (non-finite energy; wafer_last_error names the first such member).  A member that
 * has finished is frozen: it is not normalised or advanced again.  Returns WAFER_OK unless the call itself failed. */
int wafer_batch_solve(wafer_batch *b, double tolerance, uint64_t screen_update, int has_max_steps, uint64_t max_steps,
                      wafer_block_record *records, size_t max_records_per_member, size_t *n_records,
                      wafer_observables_output *finals, int *status);
/* HIP-event time of the step launches of the last wafer_batch_evolve and its step count (blocks until they finish) */
int wafer_batch_last_evolve_ms(wafer_batch *b, float *ms, uint64_t *steps);
/* the one-step kernel of a batched step; the pass kernel: wafer_batch_diag_dispatch */
const char *wafer_batch_kernel_name(wafer_batch *b);
/* K of the pass a ground-state evolve of at least K steps launches (1: the one-step kernel) */
int wafer_batch_steps_per_launch(wafer_batch *b);
/* -1: default dispatch; 0: one step per launch; 1: fused passes of K steps wherever an instantiation exists (a call's
 * remainder runs as shorter passes and single steps).  Every variant computes the same bits. */
int wafer_batch_set_step_variant(wafer_batch *b, int variant);
/* one line of key=value pairs -- stencil= kernel= steps_per_pass= tile= lds_bytes= remainder= variant= dtype= -- from the launch
 * path's own predicates; launches nothing.  kernel= names the instantiation: wafer_k_batch_step<R> / wafer_k_batch_stepk<R,K> on
 * fp64, with the storage and arithmetic types appended on the float dtypes (<R,float,double>, <R,K,float,float>, ...). */
int wafer_batch_diag_dispatch(wafer_batch *b, char *buf, size_t n);
/* launches since creation: fused passes (more than one step each) and one-step launches */
int wafer_batch_diag_passes(wafer_batch *b, uint64_t *fused_passes, uint64_t *single_steps);

/* ---- batched excited states ------------------------------------------------
 * Every member has a state store (w_store) of its own, of capacity its wafer_params.max_states, on the device: slot l of all
 * members is one allocation with the batch's member stride, made by the first push or load that needs it (a ground-state batch
 * allocates none).  The calls mirror the single context's; where they take `active`, they act on the members with
 * active[m] != 0 (NULL: all) and leave the others bit for bit as they are.  A call that cannot be carried out for one of its
 * members (store full, store shorter than wnum or idx, phi not set) returns WAFER_ERR_STATE naming that member and changes
 * nothing; wafer_batch_solve_state alone reports a short store per member instead.
 * One excited step is 1 + 2 (1 + wnum) + 1 launches for the whole batch, with every scalar (norm2, the overlaps) on the
 * device and no host synchronisation between steps.  Sums run over a partition fixed by the shape alone, in a fixed order:
 * a member's bits do not depend on the batch size, on its index or on which other members are active.
 *
 * The one-pass form (wafer_batch_set_gs_variant(b, 1); opt-in, for wnum <= 4): the step, one pass that sums phi'^2 and the raw
 * overlaps t_j = sum l_j phi' on the un-normalised phi', one reduce, and one apply pass that forms norm = sqrt(sum phi'^2) and
 * s_j = t_j / norm - sum_{i<j} s_i G_ji from the member's Gram matrix G_ji = sum l_j l_i and writes phi = phi' / norm - sum_j l_j s_j
 * (subtractions in storage order, unfused): 4 launches per step whatever wnum and B.  The Gram matrix lives on the device, is
 * recomputed lazily in stream order after load_state, push_state, clear_states or a solve_state that pushed, and nothing is
 * allocated or launched for it unless the form is selected.  A call with wnum > 4 runs the sequential form.  Its contract:
 *  - WAFER_F64: every member within 1e-13 per cell of the reference's excited-state evolve and of a wafer_ctx, norm2 within
 *    rel 1e-12.  NOT the sequential form's bits: the overlaps come from the recurrence, not from the projected phi.
 *  - float dtypes: every operand widened, every operation fp64, phi rounded to float ONCE per step after the step kernel's own
 *    store (the sequential form rounds it 1 + wnum times): up to a few float spacings from the sequential form.  A
 *    WAFER_F32_FAST batch computes WAFER_F32's bits.
 *  - as for the sequential form: a member's bits do not depend on B, its index or the active set; frozen members and every
 *    stored state are untouched bit for bit; the same call from the same start gives the same bits; no floating-point atomics
 *    and no host synchronisation between steps.
 * wafer_batch_orthogonalise under it: the same three launches without the division (norm = 1). */
int wafer_batch_load_state(wafer_batch *b, uint32_t member, uint32_t idx, const double *state);  /* as wafer_load_state: idx <= the member's count */
int wafer_batch_download_state(wafer_batch *b, uint32_t member, uint32_t idx, double *out);
int wafer_batch_push_state(wafer_batch *b, const uint8_t *active);          /* w_store.push(phi), grid.rs:241 */
int wafer_batch_num_states(wafer_batch *b, uint32_t *counts_out);           /* n_members entries */
int wafer_batch_clear_states(wafer_batch *b, const uint8_t *active);
int wafer_batch_clone_state_to_phi(wafer_batch *b, const uint8_t *active, uint32_t idx);
/* grid.rs:477-492: modified Gram-Schmidt of phi against the first wnum stored states of each active member */
int wafer_batch_orthogonalise(wafer_batch *b, const uint8_t *active, uint32_t wnum);
/* get_norm_squared of every member: out has n_members entries */
int wafer_batch_norm2(wafer_batch *b, double *out);
/* n_steps steps (0 takes one) of state wnum of the active members, grid.rs:544-687: the step, phi /= sqrt(norm2), then
 * Gram-Schmidt against the member's first wnum states.  wnum = 0 is wafer_batch_evolve. */
int wafer_batch_evolve_state(wafer_batch *b, const uint8_t *active, uint32_t wnum, uint64_t n_steps);
/* wafer_solve_state(ctx, wnum, ...) for every member at once; the arguments after wnum are wafer_batch_solve's and
 * finals[m].state = wnum.  A member that converges has its phi pushed to its store (grid.rs:239-242); one that ends in
 * WAFER_ERR_MAX_STEP or WAFER_ERR_STATE pushes nothing.  A member whose store holds fewer than wnum states, or is full when it
 * converges, gets status WAFER_ERR_STATE; the first kind is not touched at all, and the others run.  wafer_batch_solve is
 * this call with wnum = 0 except that it pushes nothing. */
int wafer_batch_solve_state(wafer_batch *b, uint32_t wnum, double tolerance, uint64_t screen_update, int has_max_steps,
                            uint64_t max_steps, wafer_block_record *records, size_t max_records_per_member, size_t *n_records,
                            wafer_observables_output *finals, int *status);
/* the form of the excited step and of orthogonalise: -1 default dispatch (the sequential form), 0 the sequential form, 1 the
 * one-pass form wherever wnum <= 4 (a call with a larger wnum runs sequentially).  Anything else: WAFER_ERR_INVALID. */
int wafer_batch_set_gs_variant(wafer_batch *b, int variant);
/* one line of key=value pairs -- wnum= form=sequential|onepass launches_per_step= kernels= variant= dtype= onepass_bytes= -- from the
 * launch path's own predicates for an excited step with this wnum; launches nothing.  onepass_bytes: device memory the one-pass
 * form has allocated beyond the sequential form's (Gram matrices, their partials and member lists, the wider sums partials):
 * 0 until it first runs. */
int wafer_batch_diag_gs(wafer_batch *b, uint32_t wnum, char *buf, size_t n);
/* excited steps and orthogonalise calls run in each form since creation */
int wafer_batch_diag_gs_steps(wafer_batch *b, uint64_t *onepass, uint64_t *sequential);

/* ---- Rayleigh-Ritz on the stores of a batch --------------------------------
 * wafer_ritz_matrices, wafer_ritz_solve and wafer_rotate_states (above) on the first k[m] stored states of every listed member
 * (active[m] != 0; NULL: all), each with its own k: one sums launch, one reduce launch and one read-back for all listed members
 * whatever their number and shapes, the solves on the host, one rotation launch for the members that solved.  Every member gets
 * bit for bit what a wafer_ctx of its own wafer_params, holding the same states and potential, gets from the three context calls.
 * k has n_members entries; entries of members not listed are not read.  An empty list returns WAFER_OK and launches nothing.
 * Every check for every listed member runs before anything is uploaded or launched, the refusal names the member, and a refused
 * call changes no store and writes no output: k[m] == 0 or k[m] > WAFER_RITZ_MAX is WAFER_ERR_INVALID; k[m] above the member's
 * state count, or no potential on it where the matrices are needed, WAFER_ERR_STATE; a non-finite coef entry of a listed member
 * WAFER_ERR_INVALID.  A mixed-shape batch made without state stores refuses all three calls as it refuses every excited-state call.
 * phi, the states beyond k[m] and the members not listed are never touched.  After a rotation the one-pass Gram-Schmidt form
 * recomputes the rotated members' Gram matrices before its next step.
 *
 * h, s: n_members * WAFER_RITZ_MAX^2 doubles each; member m's k[m] x k[m] row-major matrices packed at m * WAFER_RITZ_MAX^2.
 * Entries of members not listed are not written. */
int wafer_batch_ritz_matrices(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *h, double *s);
/* coef: as above, member m's k[m] x k[m] at m * WAFER_RITZ_MAX^2 */
int wafer_batch_rotate_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, const double *coef);
/* the three in sequence; evals: n_members * WAFER_RITZ_MAX; h, s may be NULL; status: n_members entries.
 * A solve that fails (linearly dependent states, no Jacobi convergence) is that member's status, not the call's: the member gets
 * status[m] = WAFER_ERR_STATE, its store and its evals / coef entries stay untouched, its h / s are still written where given;
 * the other members are rotated and get WAFER_OK, the call returns WAFER_OK and wafer_last_error names the first failed member.
 * Members not listed keep their status entry as passed in. */
int wafer_batch_ritz(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *evals, double *coef,
                     double *h, double *s, int *status);
/* launches and read-backs of the three calls above since creation: wafer_batch_ritz_matrices 2 and 1, wafer_batch_rotate_states
 * 1 and 0, wafer_batch_ritz 3 and 1, whatever the number of members and shapes (the lazy Gram refresh is the next excited step's) */
int wafer_batch_diag_ritz_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks);

/* ---- residuals on a batch ---------------------------------------------------
 * wafer_residuals (above) for every listed member (active[m] != 0; NULL: all), each with its own k[m] and theta: per pass one sums
 * launch, one reduce launch and one read-back for all listed members whatever their number and shapes -- theta_in given: 2
 * launches and 1 read-back; theta_in == NULL (Rayleigh mode): twice that.  An empty list returns WAFER_OK and launches nothing.
 * Every member gets bit for bit what a wafer_ctx of its own wafer_params, holding the same source and potential, gets from
 * wafer_residuals.  k has n_members entries; theta_in, theta, r2, s hold n_members * WAFER_RITZ_MAX doubles, member m's k[m]
 * values at m * WAFER_RITZ_MAX; status has n_members entries.  Entries of members not listed are neither read nor written.
 * Every check of wafer_residuals runs for every listed member before anything is uploaded or launched and names the member.
 * WAFER_RESIDUAL_STATES on a mixed-shape batch made without state stores is refused as every excited-state call there;
 * WAFER_RESIDUAL_PHI is accepted on every batch.  In Rayleigh mode a member one of whose s_j is not finite or not > 0 gets
 * status[m] = WAFER_ERR_STATE and keeps its output entries; the others get WAFER_OK and their results, the call returns WAFER_OK
 * and wafer_last_error names the first such member.  Read-only like wafer_residuals. */
int wafer_batch_residuals(wafer_batch *b, int source, const uint8_t *active, const uint32_t *k, const double *theta_in,
                          double *theta, double *r2, double *s, int *status);
/* launches and read-backs of wafer_batch_residuals since creation */
int wafer_batch_diag_residual_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks);

/* ---- moment matrices on a batch ---------------------------------------------
 * wafer_moment_matrices (above) for every listed member (active[m] != 0; NULL: all), each with its own k[m] and the centres of its
 * own nx, ny, nz: one sums launch, one reduce launch and one read-back for all listed members whatever their number and shapes.
 * An empty list returns WAFER_OK and launches nothing.  Every member gets bit for bit what a wafer_ctx of its own wafer_params
 * holding the same states gets.  k has n_members entries; m holds n_members * WAFER_MOMENT_COUNT * WAFER_RITZ_MAX^2 doubles: member
 * mb's matrix q, k[mb] x k[mb] row-major, at (mb * WAFER_MOMENT_COUNT + q) * WAFER_RITZ_MAX^2.  Entries of members not listed are
 * not written.  Every check of wafer_moment_matrices runs for every listed member before anything is uploaded or launched and names
 * the member; a mixed-shape batch made without state stores is refused as every excited-state call there.  Read-only. */
int wafer_batch_moment_matrices(wafer_batch *b, const uint8_t *active, const uint32_t *k, double *m);
/* launches and read-backs of wafer_batch_moment_matrices since creation: 2 and 1 per call */
int wafer_batch_diag_moment_counts(wafer_batch *b, uint64_t *launches, uint64_t *readbacks);

/* ---- stepping the stores of a batch -----------------------------------------
 * wafer_evolve_states (above) for every listed member (active[m] != 0; NULL: all), each with its own k[m]: ONE launch per step
 * advances states 0 .. k[m] - 1 of all listed members, whatever their number and shapes, with V loaded and a, b formed once per
 * cell for the (up to four) states a workgroup steps.  Every stepped state holds bit for bit what phi of a wafer_ctx of the member's
 * wafer_params holds after wafer_evolve(ctx, 0, n_steps) from that state, on f64, f32 and f32fast.  phi, the states from k[m] on, V,
 * the current buffers and every member not listed keep every bit.  k has n_members entries; entries of members not listed are not
 * read, and a listed member with k[m] == 0 costs nothing.  n_steps == 0 takes one step.
 * Steps run between the slots and shadow slots laid out as they are (made and zeroed by the first call that needs them); after an
 * odd number of steps one batched copy brings the listed members' states back, so a call is n_steps launches or n_steps + 1.
 * Every check for every listed member runs before anything is allocated or launched, names the member, and a refused call changes
 * nothing: k[m] > WAFER_RITZ_MAX is WAFER_ERR_INVALID; k[m] above the member's state count, or no potential on a member with
 * k[m] > 0, WAFER_ERR_STATE; a mixed-shape batch made without state stores refuses the call as every excited-state call.
 * Afterwards the one-pass Gram-Schmidt form recomputes the listed members' Gram matrices before its next step, and
 * wafer_batch_last_evolve_ms gives the call's time and n_steps. */
int wafer_batch_evolve_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint64_t n_steps);
/* one line of key=value: kernel= (the instantiation), states_per_workgroup=, shapes= */
int wafer_batch_diag_store_step(wafer_batch *b, char *buf, size_t n);
/* launches of wafer_batch_evolve_states since creation: n_steps per call, plus one where n_steps is odd */
int wafer_batch_diag_store_counts(wafer_batch *b, uint64_t *launches);

/* ---- filtering the stores of a batch ----------------------------------------
 * wafer_filter_states (above) for every listed member (active[m] != 0; NULL: all), each with its own k[m] and its own interval
 * a0[m] < a[m] < b[m] (n_members entries each), one degree per call: ONE launch per recurrence step for all listed members
 * whatever their number and shapes, V and the member's coefficients loaded once per cell for the (up to four) states a workgroup
 * filters.  Every filtered state holds bit for bit what a wafer_ctx of the member's wafer_params holds after wafer_filter_states
 * on the same state, on f64, f32 and f32fast.  phi, the states from k[m] on, V, the current buffers and every member not listed
 * keep every bit.  Entries of members not listed are not read; a listed member with k[m] == 0 costs nothing and its interval is
 * not read.  Steps run between the slots and the shadow slots of wafer_batch_evolve_states; after an odd degree one batched copy
 * brings the states back, so a call is degree launches or degree + 1.  No new device memory beyond the shadows.
 * Every check for every listed member runs before anything is allocated or launched, names the member, and a refused call
 * changes nothing: degree == 0 or > WAFER_FILTER_MAX_DEGREE, k[m] > WAFER_RITZ_MAX or a refused interval is WAFER_ERR_INVALID;
 * k[m] above the member's state count, or no potential on a member with k[m] > 0, WAFER_ERR_STATE; a mixed-shape batch made
 * without state stores refuses the call as every excited-state call.  Afterwards the one-pass Gram-Schmidt form recomputes the
 * listed members' Gram matrices before its next step, and wafer_batch_last_evolve_ms gives the call's time and degree. */
int wafer_batch_filter_states(wafer_batch *b, const uint8_t *active, const uint32_t *k, uint32_t degree, const double *a,
                              const double *bb, const double *a0);
/* wafer_spectral_bound for every listed member into ub[m] (n_members entries; others untouched): one launch and one read-back
 * whatever the members and shapes, on every batch.  A listed member without a potential: WAFER_ERR_STATE, nothing written. */
int wafer_batch_spectral_bound(wafer_batch *b, const uint8_t *active, double *ub);
/* launches of wafer_batch_filter_states (degree per call, plus one where degree is odd) and of wafer_batch_spectral_bound (one per
 * call) since creation */
int wafer_batch_diag_filter_counts(wafer_batch *b, uint64_t *launches, uint64_t *bound_launches);

#ifdef __cplusplus
}
#endif
#endif
